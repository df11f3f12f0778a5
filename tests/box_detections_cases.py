"""Named cases of the pyramid box-head inference (DESIGN.md §3 "Pyramid box-head inference"): the
smallest shapes at which each edge of bd_score_kernel, bd_class_nms_kernel and bd_merge_kernel
(csrc/box_detect.hip) exists.  Plain numpy, no GPU.

Chain geometry (that of tests/detect_cases.py, in xyxy).  Rows have ``box_regression = 0`` and
integer proposals of width 64 and height 32, so a decoded box is its proposal bit for bit.  Every
row has a *region* and a *position*: region g is the band ``y in [40 g, 40 g + 32)``, position p
the columns ``x in [16 p, 16 p + 64)``.  Boxes of different regions are disjoint; two boxes of one
region suppress one another at ``nms_thresh`` 0.5 exactly when their positions differ by at most
1 (IoU 0.6 one step apart, 1/3 two apart).  ``propose_plan_cases.closed_form`` then gives every
class's keep list without one IoU, and ``check_closed_form`` holds the restatement to it.

The score order is never taken from the logits: it is the order of the restatement's own
probabilities.  Every case carries ``check(case, ref)``, its own precondition on the fp32
restatement, so that a generator change cannot empty it silently.

``half``: the case also runs in float16 and bfloat16; its logits and deltas are multiples of 1/8
of small magnitude (or the -30 of a non-candidate), which both types hold exactly.

Users: tests/test_box_detections_cpu.py and tests/test_gpu_box_detections.py.
"""
from __future__ import annotations

import numpy as np

import box_detections_ref as ref_mod
from propose_plan_cases import closed_form

F32 = np.float32
NEG = -30.0                           # logit of a class a row is no candidate of: p < 1e-12
IMG_H, IMG_W = 163840.0, 4096.0       # the chain canvas: 4,096 regions, 253 positions
STEP = 16
OUT = ("boxes", "labels", "scores", "roi", "count", "total")
ROWS, STRIDED = "rows", "strided"
DCLIP = ref_mod.DCLIP


def up(x, dtype=F32):
    return np.nextafter(dtype(x), dtype(np.inf))


def down(x, dtype=F32):
    return np.nextafter(dtype(x), dtype(-np.inf))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(got, want, what=""):
    for name, g, w in zip(OUT, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        bad = bits(g) != bits(w)
        assert not bad.any(), (f"{what}: {name}: {int(bad.sum())} of {bad.size} elements differ in their bits; "
                               f"first at {np.argwhere(bad)[0].tolist()}: {g[bad][0]!r} != {w[bad][0]!r}")


def plan_name(R, dtype="f32"):
    e = {"f32": "ElemF32", "f16": "ElemF16", "bf16": "ElemBF16"}[dtype]
    q, br = (1, ROWS) if R <= 1024 else (4, STRIDED)
    return f"bd_score_kernel<{e}> bd_class_nms_kernel<{e},{q}>[{br}] bd_merge_kernel<{e}>"


def chain_boxes(region, pos):
    region, pos = np.asarray(region, np.int64), np.asarray(pos, np.int64)
    b = np.stack([STEP * pos, 40 * region, STEP * pos + 64, 40 * region + 32], -1).astype(F32)
    assert b.min() >= 0 and b[..., 2].max() <= IMG_W and b[..., 3].max() <= IMG_H
    return b


class Case:
    def __init__(self, name, group, logits, reg, proposals, prop_count, *, image_sizes=(IMG_H, IMG_W), check=None,
                 half=False, region=None, pos=None, original_sizes=None, **kw):
        self.name, self.group = name, group
        self.proposals = np.ascontiguousarray(proposals, F32)
        self.N, self.R = self.proposals.shape[:2]
        self.logits = np.ascontiguousarray(logits, F32).reshape(self.N * self.R, -1)
        self.C = self.logits.shape[1]
        self.reg = np.ascontiguousarray(reg, F32).reshape(self.N * self.R, 4 * self.C)
        self.prop_count = np.ascontiguousarray(prop_count, np.int32).reshape(self.N)
        self.image_sizes = np.ascontiguousarray(np.broadcast_to(np.asarray(image_sizes, F32), (self.N, 2)))
        self.original_sizes = None if original_sizes is None else np.ascontiguousarray(original_sizes, F32)
        self.kw = dict(score_thresh=0.05, nms_thresh=0.5, detections_per_img=100, min_size=1e-2,
                       reg_weights=(10.0, 10.0, 5.0, 5.0))
        self.kw.update(kw)
        self.D = self.kw["detections_per_img"]
        self.check, self.half, self.region, self.pos = check, half, region, pos
        self.plan = ROWS if self.R <= 1024 else STRIDED
        for a in (self.logits, self.reg, self.proposals, self.prop_count, self.image_sizes):
            a.setflags(write=False)
        self._ref = {}

    def __repr__(self):
        return self.name

    def reference(self, mistake=None):
        """The restatement's six outputs: computed once per variant, read-only."""
        if mistake not in self._ref:
            out = ref_mod.box_detections(self.logits, self.reg, self.proposals, self.prop_count, self.image_sizes,
                                         original_sizes=self.original_sizes, mistake=mistake, **self.kw)
            for a in out:
                a.setflags(write=False)
            self._ref[mistake] = out
        return self._ref[mistake]

    def valid_rows(self, n):
        return int(np.clip(self.prop_count[n], 0, self.R))

    def probs(self, n):
        """(p [k, C], [candidate rows of class 1, 2, ...]) of the restatement."""
        p = ref_mod.probabilities(self.logits, self.prop_count, n, self.R)
        return p, ref_mod.candidates(p, self.kw["score_thresh"])

    def ranked(self, n, c):
        """Candidate rows of (n, c) in the sweep's order: probability descending, row ascending."""
        p, cand = self.probs(n)
        rows = cand[c - 1]
        return rows[np.argsort(-p[rows, c], kind="stable")]


def kept(ref, n, c=None):
    """(rows, labels) of image n's written detections, or the rows of class c."""
    k = int(ref[4][n])
    if c is None:
        return ref[3][n, :k], ref[1][n, :k]
    return ref[3][n, :k][ref[1][n, :k] == c]


def _ok(cond, *what):
    assert cond, what


def check_closed_form(case, ref):
    """A chain case: the decoded box is the proposal bit for bit, the boxes obey the region /
    position rule on either side of the threshold, and the restatement's six outputs are what the
    rule, the score order and the merge order give."""
    assert case.region is not None and case.original_sizes is None
    D, C = case.D, case.C
    boxes = np.zeros_like(ref[0])
    labels, roi = np.full_like(ref[1], -1), np.full_like(ref[3], -1)
    scores = np.zeros_like(ref[2])
    for n in range(case.N):
        p, cand = case.probs(n)
        k = case.valid_rows(n)
        assert not case.reg[n * case.R:n * case.R + k].any()
        used = np.unique(np.concatenate(cand)) if cand else np.zeros(0, np.int64)
        reg, pos = case.region[n], case.pos[n]
        if len(used):
            b, ok = ref_mod.decode(case.proposals[n, used], np.zeros((len(used), 4), F32), case.kw["reg_weights"],
                                   *case.image_sizes[n], case.kw["min_size"])
            assert ok.all() and np.array_equal(bits(b), bits(case.proposals[n, used])), "decode moved a box"
            if len(used) <= 1100:       # the rule itself, on the cases small enough for a k x k matrix of it
                r, q = reg[used], pos[used]
                rule = (r[:, None] == r[None, :]) & (np.abs(q[:, None] - q[None, :]) <= 1)
                assert np.array_equal(ref_mod.over_matrix(case.proposals[n, used], case.kw["nms_thresh"]), rule)
        out = []
        for c in range(1, C):
            order = case.ranked(n, c)
            keep = order[closed_form(reg, pos, order)] if len(order) else order
            out += [(int(ref_mod.desc_key(p[r, c:c + 1])[0]), int(r) * (C - 1) + c - 1, int(r), c) for r in keep]
        out.sort()
        assert ref[5][n] == len(out) and ref[4][n] == min(len(out), D), (case.name, n, len(out), ref[5][n])
        for s, (_, _, r, c) in enumerate(out[:D]):
            boxes[n, s], labels[n, s], scores[n, s], roi[n, s] = case.proposals[n, r], c, p[r, c], r
    same_bits((boxes, labels, scores, roi, ref[4], ref[5]), ref, case.name + " closed form")


class Img:
    """One image of a chain case: R rows, each with a region and a position (default: a region of
    its own), and per class the rows that are its candidates."""

    def __init__(self, R, C, region=None, pos=None, count=None):
        self.R, self.C = R, C
        self.cls = np.full((R, C), NEG, F32)
        self.cls[:, 0] = 0
        self.region = np.arange(R) if region is None else np.asarray(region, np.int64)
        self.pos = np.zeros(R, np.int64) if pos is None else np.asarray(pos, np.int64)
        self.count = R if count is None else count

    def put(self, c, rows, hi=4.0, step=1 / 1024):
        """Rows in the order their scores shall fall: logits hi, hi - step, ... (exact in fp32)."""
        rows = np.asarray(rows, np.int64)
        assert len(np.unique(rows)) == len(rows) and len(rows) * step <= 8
        self.cls[rows, c] = (hi - np.arange(len(rows)) * step).astype(F32)
        return self

    def put_half(self, c, rows, hi=4.0):
        """Logits on the 1/8 grid that float16 and bfloat16 hold: hi, hi - 1/8, ..., 64 levels, then
        again from hi -- rows 64 apart tie."""
        rows = np.asarray(rows, np.int64)
        self.cls[rows, c] = (hi - (np.arange(len(rows)) % 64) / 8.0).astype(F32)
        return self


def chain_case(name, group, imgs, *, check=None, **kw):
    kw.setdefault("score_thresh", 0.001)        # a row that is a candidate of two classes shares its mass
    imgs = imgs if isinstance(imgs, (list, tuple)) else [imgs]
    region, pos = np.stack([i.region for i in imgs]), np.stack([i.pos for i in imgs])
    R, C = imgs[0].R, imgs[0].C
    own = check

    def chk(case, ref):
        check_closed_form(case, ref)
        if own is not None:
            own(case, ref)

    return Case(name, group, np.stack([i.cls for i in imgs]), np.zeros((len(imgs), R, 4 * C), F32),
                chain_boxes(region, pos), [i.count for i in imgs], check=chk, region=region, pos=pos, **kw)


def _quads(R):
    """Regions of four positions: every region is a chain of four."""
    return np.arange(R) // 4, np.arange(R) % 4


def _rng(seed):
    return np.random.default_rng(seed)


CASES = []


def add(case):
    assert all(c.name != case.name for c in CASES), case.name
    CASES.append(case)
    return case


# ------------------------------------------------------------------------------ layout
def _layout():
    rng = _rng(1)
    imgs = []
    for n, (cnt, ncand) in enumerate(((70, 40), (33, 20), (64, 64))):
        im = Img(70, 4, *_quads(70), count=cnt)
        for c in (1, 2, 3):
            im.put_half(c, rng.permutation(cnt)[:ncand - 7 * c + 7])
        im.cls[cnt:, 1] = 4.0           # rows past the count would be the best candidates
        imgs.append(im)

    def chk(case, ref):
        _ok(len(set(ref[5].tolist())) == 3 and (ref[5] > 0).all(), ref[5])
        _ok(all(len(set(kept(ref, n)[1].tolist())) == 3 for n in range(3)))
    add(chain_case("n3_unlike", "layout", imgs, check=chk, half=True,
                   image_sizes=[(IMG_H, IMG_W), (IMG_H / 2, IMG_W), (IMG_H, IMG_W / 2)]))

    im = Img(9, 2, *_quads(9)).put_half(1, [8, 3, 2, 5, 0])
    add(chain_case("c2", "layout", im, half=True, check=lambda case, ref: _ok(ref[5][0] >= 3)))

    for name, classes in (("c128_class1", (1,)), ("c128_class127", (127,)), ("c128_both", (1, 127))):
        im = Img(70, 128, *_quads(70))
        for c in classes:
            im.put_half(c, _rng(c).permutation(70)[:66])

        def chk(case, ref, classes=classes):
            _ok(set(kept(ref, 0)[1].tolist()) == set(classes), kept(ref, 0)[1])
        add(chain_case(name, "layout", im, check=chk, half=name == "c128_both"))


# -------------------------------------------------------------------------- prop_count
def _counts():
    for name, cnt, want in (("count_0", 0, 0), ("count_1", 1, 1), ("count_R", 20, 20), ("count_negative", -5, 0),
                            ("count_above_R", 1 << 30, 20)):
        a = Img(20, 3, count=cnt).put_half(1, np.arange(20)).put_half(2, np.arange(0, 20, 2))
        b = Img(20, 3, count=20).put_half(2, np.arange(5))
        if want < 20:
            a.cls[want:] = np.nan           # whatever the rows past the count hold
            a.cls[want + 1:, 1] = 50.0

        def chk(case, ref, want=want):
            _ok(ref[5][0] == want + (want + 1) // 2 and ref[5][1] == 5, ref[5], want)
        add(chain_case(name, "prop_count", [a, b], check=chk, half=True))


# ------------------------------------------------------------------ candidates per class
def _cand_counts():
    for R, ks in ((1024, (0, 1, 63, 64, 65, 1023, 1024)), (1025, (1025,)), (4096, (4096,)), (1, (1,))):
        for k in ks:
            if R == 4096:       # 2,560 regions of one, 384 chains of four: more than 2,048 are kept
                region = np.concatenate([np.arange(2560), 2560 + np.arange(1536) // 4])
                pos = np.concatenate([np.zeros(2560, np.int64), np.arange(1536) % 4])
            elif R == 1:
                region, pos = np.zeros(1, np.int64), np.zeros(1, np.int64)
            else:
                region, pos = _quads(R)
            im = Img(R, 2, region, pos)
            rows = _rng(k).permutation(R)[:k]
            im.put(1, rows)

            def chk(case, ref, k=k, R=R):
                p, cand = case.probs(0)
                _ok(len(cand[0]) == k, len(cand[0]), k)
                _ok(len(np.unique(bits(p[cand[0], 1]))) == k, "scores are distinct")
                _ok(case.plan == (ROWS if R <= 1024 else STRIDED))
                if R == 4096:
                    _ok(ref[5][0] > 2048, ref[5])     # the merge reads its keys from global memory
                if k >= 63:
                    _ok(ref[5][0] < k, "the sweep suppresses")
            add(chain_case(f"cand_{k}_R{R}", "cand", im, check=chk, detections_per_img=100 if R != 1024 else 1024))


# ---------------------------------------------------------------------- score threshold
def _free_case(name, group, logits, reg, proposals, **kw):
    logits = np.asarray(logits, F32)
    N, R = np.asarray(proposals).shape[:2]
    kw.setdefault("prop_count", [R] * N)
    cnt = kw.pop("prop_count")
    return Case(name, group, logits, reg, proposals, cnt, **kw)


def _thresholds():
    R = 6
    logits = np.full((R, 3), NEG, F32)
    logits[:, 0] = 0
    logits[:, 1] = [1.0, 1.0, 0.5, 0.25, -1.0, 2.0]
    props = chain_boxes(np.arange(R), np.zeros(R, np.int64))[None]
    p = ref_mod.softmax(logits)
    t = p[0, 1]
    assert p[1, 1] == t and p[2, 1] < t

    def at(case, ref):      # rows 0 and 1 sit at the threshold's own bits: out
        _ok(F32(case.kw["score_thresh"]) == t and sorted(kept(ref, 0)[0].tolist()) == [5])

    def below(case, ref):
        _ok(up(case.kw["score_thresh"]) == t and sorted(kept(ref, 0)[0].tolist()) == [0, 1, 5])
    add(_free_case("thresh_at_bits", "thresh", logits, np.zeros((R, 12), F32), props, score_thresh=float(t), check=at))
    add(_free_case("thresh_float_below", "thresh", logits, np.zeros((R, 12), F32), props, score_thresh=float(down(t)),
                   check=below))

    logits = np.zeros((8, 3), F32)
    logits[:, 1] = 1.0
    logits[0, 2] = np.nan           # a NaN that is not the first logit
    logits[1, 0] = np.nan           # one that is
    logits[2, 1] = np.inf           # inf - inf
    logits[3, :] = -np.inf
    logits[4, 2] = -np.inf          # exp(-inf) = 0: the row stays valid
    logits[5, 0] = -np.inf
    logits[6] = [-200.0, 0.0, -200.0]   # exp(-200) is 0 in fp32: p = 1.0 exactly
    props = chain_boxes(np.arange(8), np.zeros(8, np.int64))[None]

    def special(case, ref):
        p, _ = case.probs(0)
        _ok(np.isnan(p[:4]).all() and not np.isnan(p[4:]).any())
        _ok(p[6, 1] == 1.0 and p[6, 0] == 0.0)
        rows, labels = kept(ref, 0)
        _ok(sorted(set(rows.tolist())) == [4, 5, 6, 7] and ref[2][0, 0] == 1.0 and ref[3][0, 0] == 6)
    add(_free_case("nan_inf_one_rows", "thresh", logits, np.zeros((8, 12), F32), props, check=special, half=True))


# ------------------------------------------------------------------------------ decode
def _decode():
    # dw at the clamp, one float above it and far above it: the same width
    R = 4
    logits = np.full((R, 2), 2.0, F32)
    logits[:, 0] = 0
    reg = np.zeros((R, 8), F32)
    reg[:, 6] = [DCLIP, up(DCLIP), 10.0, down(DCLIP)]
    reg[:, 7] = [0.0, DCLIP, up(DCLIP), 10.0]
    props = np.array([[[100.0, 200.0 + 600 * r, 102.0, 204.0 + 600 * r] for r in range(R)]], F32)   # one x for all

    def clamp(case, ref):
        _ok(ref[4][0] == 4)
        by = {int(r): ref[0][0, s] for s, r in enumerate(ref[3][0, :4])}
        w = {r: by[r][2] - by[r][0] for r in by}
        _ok(w[0] == w[1] == w[2] and w[3] < w[0], w)
        bad = case.reference("no_clamp")
        _ok(not np.array_equal(bits(bad[0]), bits(ref[0])))
    add(_free_case("dw_at_clamp", "decode", logits, reg, props, reg_weights=(1.0, 1.0, 1.0, 1.0), check=clamp,
                   image_sizes=(4096.0, 4096.0)))

    # a NaN delta: the box is dropped by the size filter
    R = 6
    logits = np.full((R, 2), 2.0, F32)
    reg = np.zeros((R, 8), F32)
    for r in range(4):
        reg[r, 4 + r] = np.nan
    reg[4, 4] = 0.5
    props = chain_boxes(np.arange(R), np.zeros(R, np.int64))[None]
    add(_free_case("nan_delta", "decode", logits, reg, props, half=True,
                   check=lambda case, ref: _ok(sorted(kept(ref, 0)[0].tolist()) == [4, 5])))

    # non-default weights and deltas for which x / w and x * (1 / w) differ
    rng = _rng(7)
    R = 40
    logits = np.full((R, 3), NEG, F32)
    logits[:, 0] = 0
    logits[:, 1] = rng.uniform(0, 3, R)
    logits[::3, 2] = rng.uniform(0, 3, len(logits[::3]))
    reg = rng.uniform(-1, 1, (R, 12)).astype(F32)
    xy = rng.integers(0, 600, (R, 2))
    wh = rng.integers(8, 200, (R, 2))
    props = np.concatenate([xy, xy + wh], 1).astype(F32)[None]

    def weights(case, ref):
        _ok(ref[5][0] >= 10)
        for m in ("recip_weights",):
            _ok(not np.array_equal(bits(case.reference(m)[0]), bits(ref[0])), m)
    add(_free_case("reg_weights", "decode", logits, reg, props, reg_weights=(3.0, 7.0, 1.5, 2.5), check=weights,
                   image_sizes=(700.0, 650.0)))
    add(_free_case("reg_weights_default", "decode", logits, reg, props,
                   check=lambda case, ref: _ok(not np.array_equal(bits(case.reference("recip_weights")[0]), bits(ref[0]))),
                   image_sizes=(700.0, 650.0)))

    # clipped to zero width / height: dropped, though the unclipped box is large
    R = 5
    logits = np.full((R, 2), 2.0, F32)
    props = np.array([[[500, 10, 564, 42], [10, 400, 74, 432], [-64, 10, 0, 42], [10, 10, 74, 42], [290, 10, 354, 42]]],
                     F32)

    def clipped(case, ref):
        _ok(sorted(kept(ref, 0)[0].tolist()) == [3, 4] and ref[0][0, :2, 2].max() == 300.0)
        _ok(case.reference("filter_before_clip")[5][0] == 5)
    add(_free_case("clip_zero_width", "decode", logits, np.zeros((R, 8), F32), props, image_sizes=(300.0, 300.0),
                   check=clipped, half=True))

    # a clipped width of exactly float32(min_size) is kept, the float below it is dropped
    ms = F32(1e-2)
    logits = np.full((2, 2), 2.0, F32)
    props = np.array([[[0, 0, 64, 32]], [[0, 0, 64, 32]]], F32)

    def edge(case, ref):
        _ok(ref[5].tolist() == [1, 0] and ref[0][0, 0, 2] == ms and case.image_sizes[1, 1] == down(ms))
    add(_free_case("width_at_min_size", "decode", logits, np.zeros((2, 8), F32), props,
                   image_sizes=[(100.0, ms), (100.0, down(ms))], check=edge))

    def edge_h(case, ref):
        _ok(ref[5].tolist() == [0, 1] and ref[0][1, 0, 3] == F32(3.0))
    add(_free_case("height_at_min_size", "decode", logits, np.zeros((2, 8), F32), props, min_size=3.0,
                   image_sizes=[(down(3.0), 100.0), (3.0, 100.0)], check=edge_h))


# --------------------------------------------------------------------------------- nms
def _nms():
    # IoU of rows 0 and 1 is q = fp32(1536 / 2560); the test is (double)q > thr
    logits = np.array([[0, 2.0], [0, 1.0], [0, 0.5]], F32)
    props = np.array([[[0, 0, 64, 32], [16, 0, 80, 32], [400, 0, 464, 32]]], F32)
    q = ref_mod.iou_matrix(props[0])[0, 1]
    assert q == F32(1536.0) / F32(2560.0)
    qd = float(q)
    for name, thr, both in (("iou_equal", qd, True), ("iou_double_below", down(qd, np.float64), False),
                            ("iou_float_below", float(down(q)), False), ("iou_double_above", up(qd, np.float64), True),
                            ("iou_float_above", float(up(q)), True)):
        def chk(case, ref, both=both):
            _ok(sorted(kept(ref, 0)[0].tolist()) == ([0, 1, 2] if both else [0, 2]))
        add(_free_case(name, "nms", logits, np.zeros((3, 8), F32), props, nms_thresh=float(thr), check=chk,
                       image_sizes=(100.0, 500.0)))

    # one chain of 200 positions in score order across three 64-candidate blocks, then regions of one
    R = 260
    region = np.concatenate([np.zeros(200, np.int64), 1 + np.arange(60)])
    pos = np.concatenate([np.arange(200), np.zeros(60, np.int64)])
    im = Img(R, 2, region, pos).put(1, np.arange(R))

    def chain(case, ref):
        rows = kept(ref, 0, 1)
        _ok(np.array_equal(np.sort(rows), np.concatenate([np.arange(0, 200, 2), np.arange(200, 260)])))
        _ok(case.reference("transitive")[5][0] == 61)    # row 0 would clear the whole chain
    add(chain_case("chain_block_edges", "nms", im, check=chain, detections_per_img=1024))

    # a chain of 128 with scores on the half grid: rows l and l + 64 tie and sit side by side, so the
    # tie order decides which of the two is kept; two blocks of candidates
    R = 140
    region = np.concatenate([np.zeros(128, np.int64), 1 + np.arange(12)])
    pos = np.concatenate([2 * (np.arange(128) % 64) + np.arange(128) // 64, np.zeros(12, np.int64)])
    im = Img(R, 2, region, pos).put_half(1, np.arange(R))

    def tie_chain(case, ref):
        p, _ = case.probs(0)
        _ok(bits(p[0, 1]) == bits(p[64, 1]))
        _ok(np.array_equal(np.sort(kept(ref, 0, 1)), np.concatenate([np.arange(64), np.arange(128, 140)])))
        _ok(not np.array_equal(case.reference("ties_desc_row")[3], ref[3]))
    add(chain_case("chain_ties", "nms", im, check=tie_chain, detections_per_img=1024, half=True))

    # two overlapping boxes of one score: the lower row is kept
    im = Img(4, 2, [0, 0, 1, 1], [0, 1, 0, 1]).put_half(1, [0]).put_half(1, [1]).put_half(1, [2]).put_half(1, [3])

    def tie_rows(case, ref):
        _ok(sorted(kept(ref, 0)[0].tolist()) == [0, 2])
        _ok(sorted(kept(case.reference("ties_desc_row"), 0)[0].tolist()) == [1, 3])
    add(chain_case("tie_rows", "nms", im, check=tie_rows, half=True))

    # identical boxes of two classes: both kept (rows 0, 1 are one box; each is in one class, row 2 in both)
    im = Img(3, 3, [0, 0, 1], [0, 0, 0])
    im.cls[0, 1], im.cls[1, 2], im.cls[2, 1], im.cls[2, 2] = 2.0, 2.0, 1.0, 1.0

    def two(case, ref):
        rows, labels = kept(ref, 0)
        _ok(sorted(zip(rows.tolist(), labels.tolist())) == [(0, 1), (1, 2), (2, 1), (2, 2)])
        _ok(case.reference("cross_class")[5][0] == 2)
    add(chain_case("two_classes_identical", "nms", im, check=two, half=True))

    # thresholds outside (0, 1)
    reg4, pos4 = _quads(24)
    for name, thr, want in (("nms_nan", float("nan"), 24), ("nms_one", 1.0, 24), ("nms_two", 2.0, 24),
                            ("nms_negative", -1.0, 1), ("nms_zero", 0.0, 6)):
        im = Img(24, 2, reg4, pos4).put_half(1, np.arange(24))

        def chk(case, ref, want=want):
            _ok(ref[5][0] == want, ref[5], want)
        logits = im.cls[None]
        add(_free_case(name, "nms", logits, np.zeros((24, 8), F32), chain_boxes(reg4, pos4)[None], nms_thresh=thr,
                       check=chk, half=True, score_thresh=0.001))


# ------------------------------------------------------------------------------- merge
def _merge():
    # all scores equal: the order is the flat index r * (C-1) + (c-1), across classes
    im = Img(12, 4)
    for c in (1, 2, 3):
        im.cls[:, c] = 1.0

    def equal(case, ref):
        p, _ = case.probs(0)
        _ok(len(np.unique(bits(p[:, 1:]))) == 1)
        rows, labels = kept(ref, 0)
        _ok(np.array_equal(rows, np.arange(36) // 3) and np.array_equal(labels, np.arange(36) % 3 + 1))
        _ok(not np.array_equal(case.reference("merge_class_first")[1], ref[1]))
    add(chain_case("all_equal_scores", "merge", im, check=equal, half=True))

    def cut(case, ref):     # the cut falls inside the run of ties
        _ok(ref[5][0] == 36 and ref[4][0] == 10 and np.array_equal(kept(ref, 0)[0], np.arange(10) // 3))
    add(chain_case("trunc_in_ties", "merge", im, check=cut, half=True, detections_per_img=10))

    for name, D in (("total_Dm1", 8), ("total_D", 7), ("total_Dp1", 6), ("D1", 1)):
        im = Img(10, 3).put_half(1, [4, 1, 8, 9]).put_half(2, [2, 7, 4], hi=3.5)

        def chk(case, ref, D=D):
            _ok(ref[5][0] == 7 and ref[4][0] == min(7, D))
        add(chain_case(name, "merge", im, check=chk, half=True, detections_per_img=D))

    # one class keeps D + 1: the cut is per image, total counts them all
    im = Img(9, 2).put_half(1, np.arange(9))

    def per_image(case, ref):
        _ok(ref[5][0] == 9 and ref[4][0] == 8 and case.reference("trunc_per_class")[5][0] == 8)
    add(chain_case("class_over_D", "merge", im, check=per_image, half=True, detections_per_img=8))

    # D = 1,024 of 1,200 kept in two classes: the select walks its digits, the sort is full
    rng = _rng(3)
    im = Img(1024, 3).put(1, rng.permutation(1024)[:600]).put(2, rng.permutation(1024)[:600], hi=3.9995)

    def big(case, ref):
        _ok(ref[5][0] == 1200 and ref[4][0] == 1024 and (np.diff(ref[2][0]) <= 0).all())
    add(chain_case("D1024", "merge", im, check=big, detections_per_img=1024))

    im = Img(5, 3)
    add(chain_case("total_zero", "merge", [im, Img(5, 3).put_half(2, [3])], half=True,
                   check=lambda case, ref: _ok(ref[5].tolist() == [0, 1])))


# ---------------------------------------------------------------------- original_sizes
def _original():
    rng = _rng(11)
    N, R = 2, 30
    logits = np.full((N, R, 3), NEG, F32)
    logits[..., 0] = 0
    logits[..., 1] = rng.integers(0, 24, (N, R)) / 8.0
    logits[:, ::2, 2] = rng.integers(0, 24, (N, R // 2)) / 8.0
    reg = (rng.integers(-8, 9, (N, R, 12)) / 8.0).astype(F32)
    xy = rng.integers(0, 500, (N, R, 2))
    wh = rng.integers(8, 300, (N, R, 2))
    props = np.concatenate([xy, xy + wh], -1).astype(F32)
    sizes = np.array([(800.0, 1066.0), (608.0, 800.0)], F32)
    orig = np.array([(1000.0, 1333.0), (480.0, 631.0)], F32)

    def ratio(case, ref):
        r = case.original_sizes / case.image_sizes
        m, _ = np.frexp(r)
        _ok((m != 0.5).all(), "no ratio is a power of two")
        _ok((ref[5] >= 5).all())
    add(_free_case("original_sizes", "original", logits, reg, props, image_sizes=sizes, original_sizes=orig,
                   check=ratio, half=True))
    add(_free_case("original_sizes_absent", "original", logits, reg, props, image_sizes=sizes, half=True,
                   check=lambda case, ref: _ok(not np.array_equal(ref[0], BY_NAME["original_sizes"].reference()[0]))))


for _f in (_layout, _counts, _cand_counts, _thresholds, _decode, _nms, _merge, _original):
    _f()
BY_NAME = {c.name: c for c in CASES}
HALF = [c for c in CASES if c.half]
# planted mistake -> the case that must expose it
MISTAKE_CASE = {"ge_thresh": "thresh_at_bits", "ties_desc_row": "tie_rows", "cross_class": "two_classes_identical",
                "transitive": "chain_block_edges", "no_clamp": "dw_at_clamp", "recip_weights": "reg_weights",
                "filter_before_clip": "clip_zero_width", "merge_class_first": "all_equal_scores",
                "trunc_per_class": "class_over_D"}


def representable(case):
    """The case's logits and deltas survive float16 and bfloat16 bit for bit."""
    for a in (case.logits, case.reg):
        with np.errstate(over="ignore"):
            if not np.array_equal(a.astype(np.float16).astype(F32), a, equal_nan=True):
                return False
        u = bits(a[~np.isnan(a)])
        if (u & 0xFFFF).any():
            return False
    return True
