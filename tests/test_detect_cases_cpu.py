"""The detection case table (tests/detect_cases.py) without a GPU: every case's own precondition
on the fp32 reference, a structural model of csrc/detect.hip that shows each case reaches the
edge its name claims, and planted mistakes -- wrong variants of the contract, written here only
-- each of which must change the output on the case meant to catch it.  A case that cannot tell
a mistake apart fails here, before anyone needs a GPU."""
import os
import re

import numpy as np
import pytest

import detect_cases as dc
import detect_ref
from replication_faster_rcnn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
BLOCK = 64          # candidates per sweep block = lanes per wave


def constants():
    src = open(os.path.join(ROOT, "replication_faster_rcnn_amd", "csrc", "detect.hip")).read()
    k = {name: int(v) for name, v in re.findall(r"constexpr int (k\w+) = (\d+);", src)}
    for name in ("kDetMaxR", "kDetMaxC", "kSmRows", "kEmitSlots"):
        assert name in k, f"{name} is gone from detect.hip"
    assert "const int nb = (cc + 63) >> 6;" in src and "for (int i = wid; i < kcount; i += nw)" in src
    return k


K = constants()


# ------------------------------------------------------------ the kernels' structure
class Model:
    """Where the kernels' edges fall for a case: thread, wave, block and workgroup indices, and by
    which route a candidate was decided.  It yields no expected output."""

    def __init__(self, case):
        self.case = case
        self.threads = (case.R + 63) // 64 * 64         # blockDim.x of det_class_nms_kernel
        self.nw = self.threads // 64
        self.max_c = K["kDetMaxC"]
        self.emit_groups = (case.max_det + K["kEmitSlots"] - 1) // K["kEmitSlots"]
        self.last_group_slots = case.max_det - (self.emit_groups - 1) * K["kEmitSlots"]
        self.softmax_groups = (case.N * case.R + K["kSmRows"] - 1) // K["kSmRows"]
        self._sweeps = {}

    @staticmethod
    def expect(cond):
        assert cond

    def cc(self, n, c):
        return len(self.case.probs(n)[1][c - 1])

    def waves(self, n, c):
        return sorted(set((self.case.probs(n)[1][c - 1] // 64).tolist()))

    def nblocks(self, n, c):
        return (self.cc(n, c) + BLOCK - 1) // BLOCK

    def last_block_rows(self, n, c):
        cc = self.cc(n, c)
        return cc - (self.nblocks(n, c) - 1) * BLOCK if cc else 0

    @staticmethod
    def block_of(rank):
        return rank // BLOCK

    def _sweep(self, n, c):
        """Per rank: "kept", "klist" (dropped by a box kept in an earlier block: the test against the
        kept list comes first) or "mask" (by one kept in its own block), and the kept-list index of
        the first box that drops it."""
        if (n, c) not in self._sweeps:
            order = self.case.ranked(n, c)
            over = dc.over_matrix(self.case.decoded(n, c, order), self.case.nms_thresh)
            kept, route, by = [], [], []
            for j in range(len(order)):
                hit = np.nonzero(over[kept, j])[0] if kept else []
                if len(hit) == 0:
                    route.append("kept")
                    by.append(None)
                    kept.append(j)
                    continue
                early = [i for i in hit if kept[i] // BLOCK < j // BLOCK]
                route.append("klist" if early else "mask")
                by.append(int(early[0] if early else hit[0]))
            self._sweeps[n, c] = (kept, route, by)
        return self._sweeps[n, c]

    def decided(self, n, c):
        return self._sweep(n, c)[1]

    def suppressor(self, n, c, rank):
        return self._sweep(n, c)[2][rank]

    def block_kept(self, n, c):
        kept = self._sweep(n, c)[0]
        return [sum(1 for j in kept if j // BLOCK == b) for b in range(self.nblocks(n, c))]

    def klist_before(self, n, c, blk):
        return sum(self.block_kept(n, c)[:blk])

    def kept_counts(self, n):
        return [len(self._sweep(n, c)[0]) for c in range(1, self.case.C)]

    def total(self, n):
        return sum(self.kept_counts(n))

    def populated(self, n):
        return [c + 1 for c, k in enumerate(self.kept_counts(n)) if k]

    def equal_offsets(self, n):
        return sum(1 for k in self.kept_counts(n) if k == 0)

    @staticmethod
    def emit_wg(slot):
        return slot // K["kEmitSlots"]

    def softmax_images(self, wg):
        rows = np.arange(wg * K["kSmRows"], min((wg + 1) * K["kSmRows"], self.case.N * self.case.R))
        return sorted(set((rows // self.case.R).tolist()))


def test_constants():
    assert (K["kDetMaxR"], K["kDetMaxC"], K["kSmRows"], K["kEmitSlots"]) == (1024, 128, 8, 1024)


@pytest.mark.parametrize("case", dc.CASES, ids=repr)
def test_case_precondition(case):
    ref = case.reference()
    assert case.check is not None
    case.check(case, ref)
    # the outputs' shape and padding, on every case
    md = case.max_det
    assert ref[0].shape == (case.N, md, 4) and all(a.shape == (case.N, md) for a in ref[1:4])
    for n in range(case.N):
        k = int(ref[4][n])
        assert k == min(int(ref[5][n]), md)
        assert (ref[1][n, k:] == -1).all() and (ref[3][n, k:] == -1).all()
        assert (dc.bits(ref[0][n, k:]) == 0).all() and (dc.bits(ref[2][n, k:]) == 0).all()
        assert (np.diff(ref[1][n, :k]) >= 0).all() and ref[1][n, :k].min(initial=1) >= 1


@pytest.mark.parametrize("case", dc.CASES, ids=repr)
def test_case_reaches_its_edge(case):
    assert case.edge is not None, "a case without a stated edge"
    case.edge(case, Model(case))


@pytest.mark.parametrize("case", dc.CASES, ids=repr)
def test_case_is_a_valid_call(case):
    """The C-ABI's argument rules (tests/test_detect_cpu.py): R, C, N and max_det in range."""
    assert 1 <= case.N <= 65535 and 1 <= case.R <= K["kDetMaxR"] and 2 <= case.C <= K["kDetMaxC"]
    assert case.max_det >= 1 and case.N * case.max_det <= 1 << 30
    assert _lib.load(require_gpu=False).frcnn_detect_workspace_size(case.N, case.R, case.C) > 0
    assert np.isfinite(case.img_h) and np.isfinite(case.img_w) and F32(case.score_thresh) == case.score_thresh


def test_table_covers_the_issue_s_edges():
    names = set(dc.NAMES)
    want = [f"cc_{n}" for n in (0, 1, 63, 64, 65, 127, 128, 129, 1023, 1024)] + ["cc_waves_0_2_15"]
    want += [f"R_{n}" for n in (1, 63, 64, 65, 1000, 1024)]
    want += [f"rcount_{t}" for t in ("m5", "0", "1", "65_of_1024", "R", "R_plus_7", "int32_max", "int32_min")]
    want += [f"emit_total_{n}" for n in (1023, 1024, 1025, 2048, 2049)] + [f"maxdet_{n}" for n in (1, 1199, 1200, 1201, 1025, 3000)]
    assert not set(want) - names, set(want) - names
    # the 16-bit subset: every case with nonzero reg, every compaction / block / emit edge
    for c in dc.CASES:
        valid = np.concatenate([c.reg[n, :c.valid_rows(n)].ravel() for n in range(c.N)])
        if valid.any():
            assert c.half, c.name
    for n in ("cc_63", "cc_64", "cc_65", "cc_1023", "cc_1024", "chain_over_block_edges", "emit_total_1024", "emit_total_1025",
              "batch_three", "klist_stride_R1024", "block_keeps_nothing", "last_block_by_block0"):
        assert n in dc.HALF_NAMES, n
    assert sum(1 for c in dc.CASES if c.nms_thresh == 0.3 and c.region is not None and c.step == 24) >= 2
    assert dc.BY_NAME["rcount_int32_max"].rcount[0] == 2 ** 31 - 1 and dc.BY_NAME["rcount_int32_min"].rcount[0] == -2 ** 31


def test_step_ious():
    for step, thr, one, two in ((8, 0.7, 56 / 72, 48 / 80), (24, 0.3, 40 / 88, 16 / 112)):
        iou = dc.iou_matrix(dc.chain_boxes([0, 0, 0, 1], [0, 1, 2, 0], step))
        assert iou[0, 1] == F32(F32(64 - step) * 32 / F32((64 + step) * 32)) and abs(iou[0, 1] - one) < 1e-6 and iou[0, 1] > thr
        assert abs(iou[0, 2] - two) < 1e-6 and iou[0, 2] < thr and iou[0, 3] == 0


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_rounding_is_torch_s(dtype):
    import torch
    g = np.random.default_rng(5)
    a = np.concatenate([g.standard_normal(4096).astype(F32) * F32(50), np.array([1e30, -1e30, 65504, 65520, 1e-8, 0, -0.0, np.inf],
                                                                                  F32)])
    a = np.concatenate([a, (np.arange(256, dtype=np.uint32) * 0x101 + 0x3F800000).view(F32)])      # ties and near-ties
    t = torch.from_numpy(a).to(torch.float16 if dtype == "f16" else torch.bfloat16).float().numpy()
    assert np.array_equal(dc.bits(dc._round(a, dtype)), dc.bits(t))


# ------------------------------------------------------------------ planted mistakes
def pipeline(case, mistake=None):
    """The contract restated once more, with one deliberate mistake switched on.  ``None`` must
    reproduce tests/detect_ref.py bit for bit on every case (test_pipeline_is_the_reference)."""
    rois, rcount, cls, reg = case.inputs()
    N, R, C, md = case.N, case.R, case.C, case.max_det
    thr = F32(case.score_thresh)
    out = (np.zeros((N, md, 4), F32), np.full((N, md), -1, np.int32), np.zeros((N, md), F32), np.full((N, md), -1, np.int32),
           np.zeros(N, np.int32), np.zeros(N, np.int32))
    for n in range(N):
        if mistake == "rcount":                                  # no clamp: the count is used as it comes
            rows = np.arange(R)[:int(rcount[n])]
        else:
            rows = np.arange(int(np.clip(rcount[n], 0, R)))
        p = detect_ref.softmax(cls[n, rows]) if len(rows) else np.zeros((0, C), F32)
        lists = []
        for c in range(1, C):
            with np.errstate(invalid="ignore"):
                m = (p[:, c] >= thr) if mistake == "ge" else (p[:, c] > thr)
            cand, sc = rows[m], p[m, c]
            order = np.lexsort((-cand if mistake == "ties" else cand, -sc))
            cand, sc = cand[order], sc[order]
            with np.errstate(over="ignore", invalid="ignore"):    # the rows past rcount hold reg of 1e30
                box = case.decoded(n, c, cand)
            over = dc.over_matrix(box, case.nms_thresh)
            kept = []
            for j in range(len(cand)):
                if mistake == "transitive":                      # a suppressed box suppresses too
                    hit = over[:j, j].any()
                elif mistake == "blocks":                        # a block forgets what earlier blocks kept
                    hit = over[[i for i in kept if i // BLOCK == j // BLOCK], j].any()
                else:
                    hit = over[kept, j].any()
                if not hit:
                    kept.append(j)
            entry = [(box[j], sc[j], cand[j]) for j in kept]
            if mistake == "tail" and len(cand) % BLOCK:           # the last block's idle lanes are kept
                entry += [(np.zeros(4, F32), F32(0), 0)] * (BLOCK - len(cand) % BLOCK)
            lists.append(entry)
        offs = np.concatenate([[0], np.cumsum([len(e) for e in lists])])
        total = int(offs[-1])
        count = min(total, md)
        if mistake == "trunc_class":                              # cut at a class boundary, not at the slot
            count = int(offs[offs <= md].max())
        for s in range(count):
            lo = int(np.searchsorted(offs, s, side="right")) - 1
            if mistake == "search":                               # the first of equal offsets: an empty class
                lo = int(np.searchsorted(offs, offs[lo], side="left"))
            e = lists[lo]
            b, v, r = e[s - offs[lo]] if s - offs[lo] < len(e) else (np.zeros(4, F32), F32(0), -1)
            out[0][n, s], out[1][n, s], out[2][n, s], out[3][n, s] = b, lo + 1, v, r
        out[4][n], out[5][n] = count, total
    return out


def differs(a, b):
    return any(not np.array_equal(dc.bits(x), dc.bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("case", dc.CASES, ids=repr)
def test_pipeline_is_the_reference(case):
    dc.same_bits(pipeline(case), case.reference(), case.name)


MISTAKES = {
    "ge": ("thresh_equal",),
    "ties": ("sort_all_equal", "sort_equal_pairs_across_waves"),
    "blocks": ("chain_over_block_edges", "last_block_by_block0", "block_keeps_nothing", "not_transitive_three_blocks",
               "klist_stride_R128", "klist_stride_R1024", "nms_just_below_one", "nms_negative"),
    "tail": ("cc_1", "cc_63", "cc_65", "cc_127", "cc_129", "cc_1023", "R_1", "R_65", "R_1000"),
    "transitive": ("not_transitive_one_block", "not_transitive_three_blocks", "chain_over_block_edges"),
    "rcount": ("rcount_m5",),
    "search": ("emit_empty_runs", "C128_class_127", "C128_classes_1_127"),
    "trunc_class": ("maxdet_1025", "maxdet_1", "maxdet_1199", "emit_empty_runs_truncated"),
}


@pytest.mark.parametrize("mistake,name", [(m, n) for m, names in MISTAKES.items() for n in names])
def test_planted_mistake_is_caught(mistake, name):
    case = dc.BY_NAME[name]
    assert differs(pipeline(case, mistake), case.reference()), f"{name} cannot tell '{mistake}' from the contract"


def test_mistakes_are_specific():
    """A mistake must not show everywhere (the variant would be broken, not subtly wrong)."""
    for mistake, quiet in (("ge", "thresh_below"), ("ties", "sort_shuffle"), ("blocks", "not_transitive_one_block"),
                           ("tail", "cc_64"), ("tail", "cc_1024"), ("transitive", "block_keeps_nothing"),
                           ("rcount", "rcount_R_plus_7"), ("search", "emit_total_2049"), ("trunc_class", "maxdet_1200")):
        case = dc.BY_NAME[quiet]
        assert not differs(pipeline(case, mistake), case.reference()), (mistake, quiet)


# ------------------------------------------------------------------ the DESIGN.md table
def test_design_table_names_existing_cases():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    start = text.index("**Detection edges and the cases that pin them.**")
    lines = text[start:].split("\n")
    rows = [ln for ln in lines[:next(i for i, ln in enumerate(lines) if i and ln.startswith(("### ", "Kernels.")))]
            if ln.startswith("|")][2:]
    assert len(rows) >= 30
    named = set()
    for row in rows:
        cells = [c.strip() for c in row.strip("|").split("|")]
        assert len(cells) == 2 and cells[0], row
        found = re.findall(r"`([^`]+)`", cells[1])
        assert found, f"no case named for: {cells[0]}"
        named.update(found)
    assert not named - set(dc.NAMES), f"DESIGN.md names cases that do not exist: {sorted(named - set(dc.NAMES))}"
    assert not set(dc.NAMES) - named, f"cases missing from DESIGN.md's table: {sorted(set(dc.NAMES) - named)}"
