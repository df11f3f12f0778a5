"""Named cases of ``ops.box_head_targets`` and ``ops.box_head_losses`` (DESIGN.md §3 "Pyramid box-head
training"): the smallest shapes at which each thing can go wrong.  Boxes are integer-valued, so IoUs are
exact quotients of small integers.  Every case carries what the kernel-name query must say for its shape
(``plan``) and, where its name promises a property, a ``check`` that asserts the property on the
restatement's result, so a case cannot silently stop testing what it is named for."""
import numpy as np
import torch

import box_head_ref as ref
from rpn_targets_ref import key_mask, philox_word0

ROIS, LABELS, MATCHED, REG, SAMPLES, NPOS, NNEG, MATCHES = range(8)


def _plan(M):
    """The parts of frcnn_box_head_targets_kernel's answer for M candidates per image."""
    blocks = (M + 255) // 256
    return (f"bht_match_kernel[M={M},blocks={blocks},tail={M - (blocks - 1) * 256}]",
            f"bht_sample_kernel[per={(M + 1023) // 1024},digits=4x12]")


class Case:
    def __init__(self, name, proposals, prop_count, gt, gt_labels, gt_count, *, seed=1, calls=0, B=16, frac=0.25,
                 fg=0.5, bg=0.5, weights=(10.0, 10.0, 5.0, 5.0), add_gt=True, key_bits=32, check=None, tv=True):
        self.name = name
        self.proposals = np.ascontiguousarray(proposals, dtype=np.float32)
        self.prop_count = np.asarray(prop_count, dtype=np.int32)
        self.gt_boxes = np.ascontiguousarray(gt, dtype=np.float32)
        self.gt_labels = np.ascontiguousarray(gt_labels, dtype=np.int32)
        self.gt_count = np.asarray(gt_count, dtype=np.int32)
        self.N, self.R = self.proposals.shape[:2]
        self.G = self.gt_boxes.shape[1]
        self.M = self.R + self.G
        assert self.gt_boxes.shape == (self.N, self.G, 4) and self.gt_labels.shape == (self.N, self.G)
        assert self.prop_count.shape == (self.N,) and self.gt_count.shape == (self.N,)
        self.seed, self.calls = seed, calls
        self.kw = dict(batch_size_per_image=B, positive_fraction=frac, fg_iou_thresh=fg, bg_iou_thresh=bg,
                       reg_weights=tuple(weights), add_gt=add_gt)
        self.B, self.key_bits = B, key_bits
        self.plan = _plan(self.M)
        self.check = check
        self.tv = tv            # torchvision's functions are defined on this case's inputs
        self._ref = {}

    def __repr__(self):
        return self.name

    def reference(self, calls=None):
        calls = self.calls if calls is None else calls
        if calls not in self._ref:
            self._ref[calls] = ref.targets(self.proposals, self.prop_count, self.gt_boxes, self.gt_labels,
                                           self.gt_count, self.seed, calls, key_bits=self.key_bits, **self.kw)
        return self._ref[calls]

    def classes(self, n):
        """(positives, negatives): the candidate indices of image n's two classes."""
        boxes, present = ref.candidates(self.proposals[n], self.prop_count[n], self.gt_boxes[n], self.gt_count[n],
                                        self.kw["add_gt"])
        m = ref.match(boxes, present, self.gt_boxes[n], self.gt_count[n], self.kw["fg_iou_thresh"],
                      self.kw["bg_iou_thresh"])
        lab = ref.labels_of(m, self.gt_labels[n])
        return np.nonzero(present & (lab >= 1))[0], np.nonzero(present & (lab == 0))[0]

    def comps(self, cand, n):
        key = philox_word0(cand, n, self.calls, self.seed) & np.uint32(key_mask(self.key_bits))
        return (key.astype(np.uint64) << np.uint64(ref.IDX_BITS)) | cand.astype(np.uint64)


def passes(comp, num):
    """The 12-bit digits, from the top of the 48, that the sample kernel's selection walks for the ``num``
    smallest of ``comp``: none for a class taken whole, and a digit whose bucket is taken whole is the last."""
    if num == 0 or num >= comp.size:
        return 0
    live, need = np.sort(comp), num
    for p in range(4):
        shift = np.uint64(12 * (3 - p))
        digit = (live >> shift) & np.uint64(4095)
        d = digit[need - 1]                       # live is sorted: the need-th smallest lies in this bucket
        need -= int((digit < d).sum())
        live = live[digit == d]
        if live.size == need:
            return p + 1
    raise AssertionError("distinct keys end in a bucket of one")


def scene(seed, N, R, G, size=64, real=None, near=0.4):
    """Integer boxes: G gt rows per image and R proposals, a share ``near`` of them a gt moved by a few
    pixels (so that IoUs fall on both sides of 0.5), the rest anywhere."""
    r = np.random.RandomState(seed)
    x1 = r.randint(0, size - 8, size=(N, G))
    y1 = r.randint(0, size - 8, size=(N, G))
    gt = np.stack([x1, y1, x1 + r.randint(8, 33, size=(N, G)), y1 + r.randint(8, 33, size=(N, G))], axis=2)
    px = r.randint(0, size - 4, size=(N, R))
    py = r.randint(0, size - 4, size=(N, R))
    prop = np.stack([px, py, px + r.randint(4, 33, size=(N, R)), py + r.randint(4, 33, size=(N, R))], axis=2)
    which = r.randint(0, G if real is None else np.maximum(np.asarray(real), 1)[:, None], size=(N, R))
    moved = np.take_along_axis(gt, which[:, :, None], axis=1) + r.randint(-3, 4, size=(N, R, 4))
    moved[..., 2:] = np.maximum(moved[..., 2:], moved[..., :2] + 1)
    prop = np.where((r.rand(N, R) < near)[:, :, None], moved, prop)
    labels = r.randint(1, 21, size=(N, G))
    count = np.full(N, G) if real is None else np.asarray(real)
    return prop.astype(np.float32), np.full(N, R), gt.astype(np.float32), labels, count


def _valid(out, n):
    return int(out[NPOS][n] + out[NNEG][n])


# ---- the properties the names promise, asserted on the restatement
def check_layout(case, out):
    for n in range(case.N):
        S = _valid(out, n)
        s, lab = out[SAMPLES][n, :S], out[LABELS][n, :S]
        assert S == case.B and (np.diff(s) > 0).all()
        pos = lab >= 1
        assert pos.any() and (~pos).any() and (np.diff(pos.astype(int)) > 0).any()   # a positive behind a negative
        assert (s < case.R).any()
        assert (out[ROIS][n * case.B:(n + 1) * case.B, 0] == n).all()
        assert out[REG][n, :S][pos].any() and not out[REG][n, :S][~pos].any()
    assert (out[SAMPLES] >= case.R).any()                                           # a gt row is sampled too


def check_gt_tie(case, out):
    m = out[MATCHES][0]
    assert (m == 0).sum() > 2 and not (m == 1).any() and (m == 2).any()      # row 1 repeats row 0
    assert m[case.R + 1] == 0                                                # the repeated row itself


def check_threshold_edges(case, out):
    m = out[MATCHES][0]
    assert m[0] == 0 and m[1] == -1 and m[2] == -1        # IoU 0.5 is a match; 0.49 and 0.25 are background


def check_threshold_band(case, out):
    m = out[MATCHES][0]
    assert m[0] == 0 and m[1] == -2 and m[2] == -2 and m[3] == -1            # 0.5; 0.49; 0.25; 0.24
    S = _valid(out, 0)
    assert 1 not in out[SAMPLES][0, :S] and 2 not in out[SAMPLES][0, :S]     # the band is never sampled


def check_gt_is_candidate(case, out):
    for n in range(case.N):
        S = _valid(out, n)
        for g in range(case.G):
            assert out[MATCHES][n, case.R + g] == g
            at = np.nonzero(out[SAMPLES][n, :S] == case.R + g)[0]
            assert at.size == 1 and out[LABELS][n, at[0]] == case.gt_labels[n, g] and out[MATCHED][n, at[0]] == g
            assert not out[REG][n, at[0]].any()                              # a gt encodes to zeros against itself
            assert np.array_equal(out[ROIS][n * case.B + at[0], 1:], case.gt_boxes[n, g])


def check_no_add_gt(case, out):
    assert (out[MATCHES][:, case.R:] == -3).all() and (out[SAMPLES] < case.R).all() and (out[NPOS] > 0).all()


def check_no_gt_image(case, out):
    S = _valid(out, 0)
    assert (out[MATCHES][0, :case.R] == -1).all() and (out[MATCHES][0, case.R:] == -3).all()
    assert S == case.B and (out[LABELS][0] == 0).all() and out[NPOS][0] == 0 and not out[REG][0].any()
    assert out[NPOS][1] > 0


def check_all_padding_gt(case, out):
    assert (out[NPOS] == 0).all() and (out[LABELS][:, :4] == 0).all() and (out[MATCHES][:, case.R:] == -3).all()


def check_invalid_gt_rows(case, out):
    m = out[MATCHES][0]
    assert set(np.unique(m[m >= 0])) == {2, 5}                  # the absent rows' indices still count
    assert (m[case.R:] == [-3, -3, 2, -3, -3, 5]).all()
    assert (out[MATCHES][1, :case.R] == -1).all()               # image 1: no present row at all


def check_gt_count_clamped(case, out):
    assert (out[MATCHES][0, case.R:] >= 0).all() and (out[MATCHES][1, case.R:] == -3).all()
    assert out[NPOS][0] > 0 and out[NPOS][1] == 0


def check_prop_count_zero(case, out):
    for n in range(case.N):
        S = _valid(out, n)
        assert (out[MATCHES][n, :case.R] == -3).all() and S == case.gt_count[n] and (out[SAMPLES][n, :S] >= case.R).all()


def check_prop_count_clamped(case, out):
    assert (out[MATCHES][0, :case.R] != -3).all() and (out[MATCHES][1, :case.R] == -3).all()


def check_rows_past_count(case, out):
    pc = int(case.prop_count[0])
    past = case.proposals[0, pc:]
    assert (past == case.gt_boxes[0, 0]).all()                  # they would match at IoU 1
    assert (out[MATCHES][0, pc:case.R] == -3).all() and not np.isin(np.arange(pc, case.R), out[SAMPLES][0]).any()


def check_nonfinite_proposal(case, out):
    bad = ~np.isfinite(case.proposals[0]).all(axis=1)
    assert bad.sum() == 4 and (out[MATCHES][0, :case.R][bad] == -1).all()
    S = _valid(out, 0)
    at = np.nonzero(np.isin(out[SAMPLES][0, :S], np.nonzero(bad)[0]))[0]
    assert at.size == 4 and (out[LABELS][0, at] == 0).all()     # sampled as background, their bits copied
    assert not np.isfinite(out[ROIS][at, 1:]).all(axis=1).any()


def check_zero_area_proposal(case, out):
    assert (out[MATCHES][0, :3] == -1).all() and (out[MATCHES][0, 3] == 0)


def check_gt_label_zero(case, out):
    m, S = out[MATCHES][0], _valid(out, 0)
    hit = np.nonzero(m == 1)[0]                                 # gt 1 carries label 0
    assert hit.size > 1
    at = np.nonzero(np.isin(out[SAMPLES][0, :S], hit))[0]
    assert at.size and (out[LABELS][0, at] == 0).all() and (out[MATCHED][0, at] == 0).all() and not out[REG][0, at].any()
    assert out[NPOS][0] == int(np.isin(m, [0, 2]).sum())        # every other match is a positive


def check_gt_label_negative(case, out):
    m, S = out[MATCHES][0], _valid(out, 0)
    hit = np.nonzero(m == 1)[0]                                 # gt 1 carries label -1: neither class
    assert hit.size > 1 and not np.isin(out[SAMPLES][0, :S], hit).any() and (out[LABELS][0, :S] >= 0).all()


def check_few_positives(case, out):
    for n in range(case.N):
        pos, neg = case.classes(n)
        assert 0 < pos.size < int(case.B * 0.25) and out[NPOS][n] == pos.size and out[NNEG][n] == case.B - pos.size
        assert neg.size > case.B - pos.size


def check_few_candidates(case, out):
    for n in range(case.N):
        S = _valid(out, n)
        pos, neg = case.classes(n)
        assert 0 < S < case.B and out[NNEG][n] == neg.size        # the negatives are taken whole: no selection
        assert (out[SAMPLES][n, S:] == -1).all() and (out[LABELS][n, S:] == -1).all() and (out[MATCHED][n, S:] == -1).all()
        assert (out[ROIS][n * case.B + S:(n + 1) * case.B] == [-1, 0, 0, 0, 0]).all() and not out[REG][n, S:].any()
        assert passes(case.comps(neg, n), int(out[NNEG][n])) == 0


def check_fraction_0(case, out):
    assert (out[NPOS] == 0).all() and (out[NNEG] == case.B).all() and (out[LABELS] == 0).all()


def check_fraction_1(case, out):
    for n in range(case.N):
        pos, _ = case.classes(n)
        assert case.B > pos.size > case.B // 4 and out[NPOS][n] == pos.size and out[NNEG][n] == case.B - pos.size


def check_weights(case, out):
    other = ref.targets(case.proposals, case.prop_count, case.gt_boxes, case.gt_labels, case.gt_count, case.seed,
                        case.calls, **{**case.kw, "reg_weights": (1.0, 1.0, 1.0, 1.0)})
    pos = out[LABELS] >= 1
    assert np.array_equal(other[SAMPLES], out[SAMPLES]) and pos.any()
    got, one = out[REG][pos], other[REG][pos]
    assert np.array_equal(got[:, 2], np.float32(3) * one[:, 2]) and np.array_equal(got[:, 3], np.float32(7) * one[:, 3])
    assert not np.array_equal(got[:, 0], one[:, 0])


def check_key_ties(case, out):
    """Ties straddle both boundaries: the last key taken is also the key of a candidate left out; the index
    decides, so the taken ones of that key are its lowest indices.  The selection walks all four digits."""
    for n in range(case.N):
        S = _valid(out, n)
        for cand, num in zip(case.classes(n), (out[NPOS][n], out[NNEG][n])):
            assert 0 < num < cand.size
            key = case.comps(cand, n) >> np.uint64(ref.IDX_BITS)
            taken = np.isin(cand, out[SAMPLES][n, :S])
            edge = key[taken].max()
            assert taken.sum() == num and (key[~taken] == edge).any() and key[~taken].min() == edge
            assert cand[taken & (key == edge)].max() < cand[~taken & (key == edge)].min()
            assert passes(case.comps(cand, n), int(num)) == 4


def check_big_state(case, out):
    assert case.seed < 0 and case.calls > 2**32
    low = ref.targets(case.proposals, case.prop_count, case.gt_boxes, case.gt_labels, case.gt_count, case.seed,
                      case.calls & 0xFFFFFFFF, **case.kw)
    assert not np.array_equal(low[SAMPLES], out[SAMPLES])       # the high word of calls is a counter word


def check_no_candidates(case, out):
    assert (out[MATCHES] == -3).all() and (out[NPOS] == 0).all() and (out[NNEG] == 0).all()
    assert (out[SAMPLES] == -1).all() and (out[ROIS] == [-1, 0, 0, 0, 0]).all()


def check_selects(case, out):
    """A shape case: both classes really are selected from (neither is taken whole)."""
    for n in range(min(case.N, 2)):
        pos, neg = case.classes(n)
        assert pos.size > out[NPOS][n] > 0 and neg.size > out[NNEG][n] > 0
        assert passes(case.comps(neg, n), int(out[NNEG][n])) >= 1


def check_g256(case, out):
    assert (out[MATCHES][0, case.R:] == np.arange(256)).all()   # every gt row, the last included, is matched
    assert (out[MATCHES][0, :8] == np.arange(248, 256)).all()


def _edges(fg, bg):
    gt = [[[0, 0, 10, 10]]]
    prop = [[[0, 0, 10, 5], [0, 0, 7, 7], [0, 0, 5, 5], [0, 0, 4, 6], [20, 20, 30, 30], [0, 0, 10, 10],
             [1, 0, 10, 10], [30, 0, 40, 10]]]
    return Case("threshold_edges" if fg == bg else "threshold_edges_band", prop, [8], gt, [[3]], [1], B=8, fg=fg, bg=bg,
                check=check_threshold_edges if fg == bg else check_threshold_band)


def _cases():
    out = []
    out.append(Case("layout", *scene(1, 2, 56, 4, near=0.3), B=16, check=check_layout))
    p, pc, gt, lab, cnt = scene(2, 2, 16, 4)
    gt[:, 1] = gt[:, 0]
    p[0, :4] = gt[0, 0]
    out.append(Case("gt_tie", p, pc, gt, lab, cnt, check=check_gt_tie))
    out += [_edges(0.5, 0.5), _edges(0.5, 0.25)]
    out.append(Case("gt_is_candidate", *scene(3, 2, 8, 3, near=0.0), B=16, frac=1.0, check=check_gt_is_candidate))
    out.append(Case("no_add_gt", *scene(4, 2, 32, 4, near=0.6), add_gt=False, check=check_no_add_gt))
    out.append(Case("no_gt_image", *scene(5, 2, 24, 4, real=[0, 3]), check=check_no_gt_image))
    out.append(Case("all_padding_gt", *scene(6, 2, 16, 4, real=[0, 0]), B=8, check=check_all_padding_gt))
    p, pc, gt, lab, cnt = scene(7, 2, 24, 6)
    gt[0, 0, 2] = np.nan
    gt[0, 1, 3] = np.inf
    gt[0, 3, 2] = gt[0, 3, 0]                       # no width
    gt[0, 4, 3] = gt[0, 4, 1] - 2                   # negative height
    gt[1, :, 0] = -np.inf
    out.append(Case("invalid_gt_rows", p, pc, gt, lab, cnt, check=check_invalid_gt_rows))
    p, pc, gt, lab, cnt = scene(8, 2, 16, 4)
    out.append(Case("gt_count_clamped", p, pc, gt, lab, [9, -3], check=check_gt_count_clamped))
    p, pc, gt, lab, cnt = scene(9, 2, 16, 4, real=[4, 2])
    out.append(Case("prop_count_zero", p, [0, 0], gt, lab, cnt, check=check_prop_count_zero))
    p, pc, gt, lab, cnt = scene(10, 2, 16, 4)
    out.append(Case("prop_count_clamped", p, [23, -2], gt, lab, cnt, check=check_prop_count_clamped))
    p, pc, gt, lab, cnt = scene(11, 2, 24, 4)
    p[0, 10:] = gt[0, 0]
    out.append(Case("rows_past_count_ignored", p, [10, 24], gt, lab, cnt, check=check_rows_past_count))
    p, pc, gt, lab, cnt = scene(12, 2, 8, 2, near=0.0)
    p[0, 0, 0] = np.nan
    p[0, 2] = [-np.inf, -np.inf, np.inf, np.inf]
    p[0, 3, 2] = np.inf
    p[0, 5] = np.nan
    out.append(Case("nonfinite_proposal", p, pc, gt, lab, cnt, B=16, check=check_nonfinite_proposal, tv=False))
    p, pc, gt, lab, cnt = scene(13, 1, 8, 2)
    gt[0, 0] = [0, 0, 10, 10]
    p[0, :4] = [[5, 0, 5, 10], [0, 5, 10, 5], [5, 5, 5, 5], [0, 0, 10, 9]]
    out.append(Case("zero_area_proposal", p, pc, gt, lab, cnt, B=8, check=check_zero_area_proposal))
    p, pc, gt, lab, cnt = scene(14, 2, 32, 3, near=0.7)
    lab[:, 1] = 0
    out.append(Case("gt_label_zero", p, pc, gt, lab, cnt, B=32, frac=1.0, check=check_gt_label_zero))
    lab = lab.copy()
    lab[:, 1] = -1
    out.append(Case("gt_label_negative", p, pc, gt, lab, cnt, B=32, frac=1.0, check=check_gt_label_negative))
    out.append(Case("few_positives", *scene(15, 2, 64, 1, near=0.0), B=16, check=check_few_positives))
    out.append(Case("few_candidates", *scene(16, 2, 8, 2), B=16, check=check_few_candidates))
    out.append(Case("fraction_0", *scene(17, 2, 32, 4), frac=0.0, check=check_fraction_0))
    out.append(Case("fraction_1", *scene(18, 2, 32, 4, near=0.15), frac=1.0, check=check_fraction_1))
    out.append(Case("weights_nondefault", *scene(19, 2, 24, 4), weights=(2.5, 0.5, 3.0, 7.0), check=check_weights))
    out.append(Case("key_ties_0", *scene(20, 2, 64, 4, near=0.5), key_bits=0, check=check_key_ties))
    out.append(Case("key_ties_4", *scene(20, 2, 64, 4, near=0.5), key_bits=4, calls=3, check=check_key_ties))   # calls: a draw
    # whose boundary keys are shared on all four boundaries (two images, two classes)
    out.append(Case("big_state", *scene(21, 2, 32, 4), seed=-0x1234567890ABCDEF, calls=2**32 + 5, check=check_big_state))
    p, pc, gt, lab, cnt = scene(22, 2, 8, 2)
    out.append(Case("no_candidates", p, [0, 0], gt, lab, [0, 0], B=8, check=check_no_candidates))
    out.append(Case("batch_1", *scene(23, 1, 32, 4), check=check_selects))
    out.append(Case("batch_1024", *scene(24, 1024, 8, 2, near=0.5), B=8, frac=0.5))
    p, pc, gt, lab, cnt = scene(25, 2, 16, 256, size=512)
    gt[0, :, 0] = 2 * np.arange(256)                # distinct rows: none ties with another
    gt[0, :, 2] = gt[0, :, 0] + 8 + np.arange(256) % 7
    p[0, :8] = gt[0, 248:]
    out.append(Case("G256", p, pc, gt, lab, cnt, B=16, check=check_g256))
    for M in (64, 65, 256, 257, 1024, 1025):
        out.append(Case(f"M_{M}", *scene(30 + M, 2, M - 4, 4, near=0.2), B=16, check=check_selects))
    out.append(Case("max_shape", *scene(26, 2, 4096, 256, size=512, near=0.3), B=1024, check=check_selects))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------- losses
class LossCase:
    """Targets as the op writes them (valid slots first, positives and negatives interleaved, padding behind)
    for ``box_head_losses``, and a head's predictions for them."""

    def __init__(self, name, N, B, C, *, seed=0, empty=False, bad_label=False, unused=None):
        self.name, self.N, self.B, self.C, self.unused = name, N, B, C, unused
        r = np.random.RandomState(1000 + seed)
        self.n_pos = np.zeros(N, np.int32) if empty else r.randint(1, max(B // 4, 2), size=N).astype(np.int32)
        self.n_neg = np.zeros(N, np.int32) if empty else r.randint(0, B - B // 4, size=N).astype(np.int32)
        self.n_neg[-1] = 0 if empty else B - self.n_pos[-1]       # the last image has no padding
        if bad_label:
            self.n_neg[0] = max(self.n_neg[0], 2)                 # slot 1 of image 0 is a valid one
        self.labels = np.full((N, B), -1, np.int32)
        self.reg_targets = np.zeros((N, B, 4), np.float32)
        for n in range(N):
            S = int(self.n_pos[n] + self.n_neg[n])
            lab = np.zeros(S, np.int32)
            at = r.permutation(S)[:self.n_pos[n]]
            lab[at] = r.randint(1, C, size=at.size)
            self.labels[n, :S] = lab
            self.reg_targets[n, :S][lab >= 1] = (r.randn(at.size, 4) * 0.3).astype(np.float32)
        if not empty:
            self.labels[0, 0] = C - 1                             # the last class, the last four columns
            self.reg_targets[0, 0] = [0.1, -0.2, 0.3, -0.4]
        if bad_label:
            self.labels[0, 1] = C + 3                             # skipped and counted, never an index
            self.labels[N - 1, 0] = 2**31 - 1
        self.bad = 2 if bad_label else 0

    def __repr__(self):
        return self.name

    def predictions(self, dtype=torch.float32):
        """(class_logits [N*B, C], box_regression [N*B, 4C]) CPU tensors of ``dtype``, the same on every call;
        differences from the targets fall on both sides of beta = 1/9."""
        g = torch.Generator().manual_seed(7 + self.C)
        rows = self.N * self.B
        cls = (torch.randn(rows, self.C, generator=g) * 3.0).to(dtype)
        reg = (torch.randn(rows, 4 * self.C, generator=g) * 0.25).to(dtype)
        return cls, reg

    def targets_np(self):
        return self.labels, self.reg_targets, self.n_pos, self.n_neg


LOSS_CASES = [LossCase(f"C{C}", 2, 16, C, seed=C) for C in (2, 21, 64, 65, 91, 128)]
LOSS_CASES += [LossCase("rows_16", 2, 8, 5, seed=1), LossCase("S_0", 2, 8, 5, empty=True),
               LossCase("label_ge_C", 2, 16, 7, seed=2, bad_label=True),
               LossCase("unused_cls", 2, 16, 21, seed=3, unused="cls"),
               LossCase("unused_box", 2, 16, 21, seed=3, unused="box"),
               LossCase("many_rows", 5, 64, 21, seed=4)]
LOSS_BY_NAME = {c.name: c for c in LOSS_CASES}
