"""Named cases of the detection stage (DESIGN.md §3 "Detection edges and the cases that pin
them"): the smallest shapes at which each branch of det_softmax_kernel, det_class_nms_kernel
and det_emit_kernel (csrc/detect.hip) exists -- compaction at wave and block edges, ``rcount``
outside [0, R], the score filter at a probability's own bits, the rank sort's ties, every route
of the 64-candidate block sweep, thresholds and degenerate boxes, the emit workgroup edge and
its binary search, and a softmax workgroup over several images.  Plain numpy, no GPU.

Chain geometry.  Rows have ``reg = 0``, so a decoded box is its RoI bit for bit; RoIs have
integer coordinates inside the image.  Every row has a *region* and a *position*: region g is
the band of rows ``[40 g, 40 g + 32)``, position p the columns ``[step p, step p + 64)``.  Boxes
of different regions are disjoint, two boxes of one region suppress one another exactly when
their positions differ by at most 1: with ``nms_thresh`` 0.7 and step 8 the IoU is 0.78 one step
apart and 0.6 two apart (the geometry of tests/propose_plan_cases.py), with the default 0.3 and
step 24 it is 0.4545 and 0.143.  ``propose_plan_cases.closed_form`` then gives every class's keep
list without one IoU; ``check_closed_form`` holds the reference to it on every such case.

The score order is never taken from the logits: it is the stable descending order of the
reference's own probabilities (``detect_ref.softmax``), which saturate and tie.  A case that needs
distinct scores asserts that they are distinct, a case about ties asserts equal bit patterns.

Every case carries ``check(case, ref)``, its own precondition on the fp32 reference, so that a
generator change cannot empty it silently, and ``edge(case, model)``, which states the kernel
edge its name claims in terms of tests/test_detect_cases_cpu.py's structural model.

Users: tests/test_detect_cases_cpu.py and tests/test_gpu_detect_cases.py.
"""
from __future__ import annotations

import numpy as np

import detect_ref
from oracle import ref_numpy as orc
from propose_plan_cases import closed_form

F32 = np.float32
NEG = -30.0                 # logit of a class a row is no candidate of: p < 1e-12
IMG_H, IMG_W = 40960.0, 4096.0      # the chain cases' canvas: 1,024 regions, 130 positions at step 24
DTYPES = ("f32", "f16", "bf16")
OUT = ("boxes", "labels", "scores", "roi", "count", "total")
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


def _round(a, dtype):
    """fp32 -> ``dtype`` -> fp32, rounded once to nearest even as ``.to`` rounds."""
    if dtype == "f32":
        return a
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return a.astype(np.float16).astype(F32)
    assert dtype == "bf16", dtype
    u = np.ascontiguousarray(a).view(np.uint32).astype(np.uint64)
    r = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32)
    r = np.where(np.isnan(a), np.uint32(0x7FC00000) | (u.astype(np.uint32) & np.uint32(0x80000000)), r)
    return r.astype(np.uint32).view(F32).reshape(a.shape)


def iou_matrix(b):
    """[k, 4] fp32 boxes -> [k, k] fp32 IoU in torchvision's operation order (csrc/nms_iou.h)."""
    b = np.asarray(b, F32)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0])
    h = np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1])
    inter = np.maximum(w, F32(0)) * np.maximum(h, F32(0))
    uni = (area[:, None] + area[None, :]) - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / uni


def over_matrix(b, thr):
    """``(double)iou > thr``: NaN (0 / 0, or a NaN threshold) is never over."""
    with np.errstate(invalid="ignore"):
        return iou_matrix(b).astype(np.float64) > float(thr)


def chain_boxes(region, pos, step):
    region, pos = np.asarray(region, np.int64), np.asarray(pos, np.int64)
    b = np.stack([40 * region, step * pos, 40 * region + 32, step * pos + 64], -1).astype(F32)
    assert b.min() >= 0 and b[..., 2].max() <= IMG_H and b[..., 3].max() <= IMG_W
    return b


class Case:
    """``region`` / ``pos`` [N, R] (chain cases; None otherwise), ``half``: also run in float16 and
    bfloat16 (the cases that cross a compaction, block or emit edge, and those with nonzero reg)."""

    def __init__(self, name, group, rois, rcount, cls, reg, *, img_h=IMG_H, img_w=IMG_W, score_thresh=0.05,
                 nms_thresh=0.3, max_det=None, check=None, edge=None, half=False, region=None, pos=None, step=None,
                 parts=None):
        self.name, self.group = name, group
        self.rois, self.cls, self.reg = (np.ascontiguousarray(a, F32) for a in (rois, cls, reg))
        self.rcount = np.ascontiguousarray(rcount, np.int32)
        self.N, self.R, self.C = self.cls.shape
        assert self.rois.shape == (self.N, self.R, 4) and self.reg.shape == (self.N, self.R, 4 * self.C)
        assert self.rcount.shape == (self.N,)
        self.img_h, self.img_w = float(img_h), float(img_w)
        self.score_thresh = float(F32(score_thresh))          # the op takes an fp32
        self.nms_thresh = float(nms_thresh)
        self.max_det = self.R * (self.C - 1) if max_det is None else int(max_det)
        self.check, self.edge, self.half = check, edge, half
        self.region, self.pos, self.step, self.parts = region, pos, step, parts
        for a in (self.rois, self.rcount, self.cls, self.reg):
            a.setflags(write=False)
        self._in, self._ref = {}, {}

    def __repr__(self):
        return self.name

    def inputs(self, dtype="f32"):
        """(rois, rcount, cls, reg) with cls and reg rounded once to ``dtype`` and widened again."""
        if dtype not in self._in:
            a = (self.rois, self.rcount, _round(self.cls, dtype), _round(self.reg, dtype))
            for x in a:
                x.setflags(write=False)
            self._in[dtype] = a
        return self._in[dtype]

    def kwargs(self):
        return dict(score_thresh=self.score_thresh, nms_thresh=self.nms_thresh, max_det=self.max_det)

    def reference(self, dtype="f32"):
        """detect_ref.detect on the widened inputs: computed once, read-only."""
        if dtype not in self._ref:
            out = detect_ref.detect(*self.inputs(dtype), self.img_h, self.img_w, **self.kwargs())
            for a in out:
                a.setflags(write=False)
            self._ref[dtype] = out
        return self._ref[dtype]

    # -------- what the checks and the structural model read
    def valid_rows(self, n):
        return int(np.clip(self.rcount[n], 0, self.R))

    def probs(self, n, dtype="f32"):
        """(p [k, C], [candidate rows of class 1, 2, ...]) of the reference."""
        rois, rc, cls, _ = self.inputs(dtype)
        return detect_ref.candidates(rois, rc, cls, n, F32(self.score_thresh))

    def ranked(self, n, c, dtype="f32"):
        """Candidate rows of (n, c) in the sweep's order: probability descending, row ascending."""
        p, cand = self.probs(n, dtype)
        rows = cand[c - 1]
        return rows[np.argsort(-p[rows, c], kind="stable")]

    def decoded(self, n, c, rows):
        b = orc.reg2bbox(self.rois[n, rows], self.reg[n, rows, 4 * c:4 * c + 4] * np.asarray(detect_ref.REG_STD, F32))
        b[:, [0, 2]] = np.clip(b[:, [0, 2]], F32(0), F32(self.img_h))
        b[:, [1, 3]] = np.clip(b[:, [1, 3]], F32(0), F32(self.img_w))
        return b


# --------------------------------------------------------------------- shared checks
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(got, want, what=""):
    for name, g, w in zip(OUT, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        bad = bits(g) != bits(w)
        assert not bad.any(), (f"{what}: det_{name}: {int(bad.sum())} of {bad.size} elements differ in their bits; "
                               f"first at {np.argwhere(bad)[0].tolist()}: {g[bad][0]!r} != {w[bad][0]!r}")


def check_closed_form(case, ref):
    """A chain case: the decoded box is the RoI bit for bit, the boxes obey the region / position
    rule on either side of the threshold, and the reference's six outputs are the rule's."""
    assert case.region is not None
    boxes = np.zeros_like(ref[0])
    labels, roi = np.full_like(ref[1], -1), np.full_like(ref[3], -1)
    scores = np.zeros_like(ref[2])
    one = two = False
    for n in range(case.N):
        p, cand = case.probs(n)
        used = np.unique(np.concatenate(cand)) if cand else np.zeros(0, np.int64)
        reg, pos = case.region[n], case.pos[n]
        assert not case.reg[n, :case.valid_rows(n)].any()
        if len(used):
            assert np.array_equal(bits(case.decoded(n, 1, used)), bits(case.rois[n, used])), "decode moved a box"
            r, q = reg[used], pos[used]
            rule = (r[:, None] == r[None, :]) & (np.abs(q[:, None] - q[None, :]) <= 1)
            assert np.array_equal(over_matrix(case.rois[n, used], case.nms_thresh), rule), "region / position rule"
            near = (r[:, None] == r[None, :]) & (np.abs(q[:, None] - q[None, :]) == 1)
            far = (r[:, None] == r[None, :]) & (np.abs(q[:, None] - q[None, :]) == 2)
            iou = iou_matrix(case.rois[n, used])
            one, two = one or near.any(), two or far.any()
            assert (iou[near] > case.nms_thresh).all() and (iou[far] < case.nms_thresh).all()
        out = []
        for c in range(1, case.C):
            order = case.ranked(n, c)
            keep = order[closed_form(reg, pos, order)] if len(order) else order
            out += [(r, c) for r in keep]
        assert ref[5][n] == len(out) and ref[4][n] == min(len(out), case.max_det), (case.name, n, len(out))
        for s, (r, c) in enumerate(out[:case.max_det]):
            boxes[n, s], labels[n, s], scores[n, s], roi[n, s] = case.rois[n, r], c, p[r, c], r
    same_bits((boxes, labels, scores, roi, ref[4], ref[5]), ref, case.name + " closed form")
    return one, two


def distinct_scores(case, n, c):
    rows = case.ranked(n, c)
    p = case.probs(n)[0][rows, c]
    assert len(np.unique(bits(p))) == len(rows) and (np.diff(p) < 0).all(), (case.name, n, c)
    return rows


def _ok(cond, *what):
    assert cond, what


def kept_rows(ref, n, c):
    k = int(ref[4][n])
    return ref[3][n, :k][ref[1][n, :k] == c]


# --------------------------------------------------------------------- builders
class Img:
    """One image of a chain case: R rows, each with a region and a position (default: a region of
    its own), and per class the rows that are its candidates in score order."""

    def __init__(self, R, C, region=None, pos=None):
        self.R, self.C = R, C
        self.cls = np.full((R, C), NEG, F32)
        self.cls[:, 0] = 0
        self.region = np.arange(R) if region is None else np.asarray(region, np.int64)
        self.pos = np.zeros(R, np.int64) if pos is None else np.asarray(pos, np.int64)
        self.rcount = R

    def put(self, c, rows, hi=4.0):
        """Rows in the order their scores shall fall: logits hi, hi - 1/256, ... (exact in fp32)."""
        rows = np.asarray(rows, np.int64)
        assert len(rows) <= 1024 and len(np.unique(rows)) == len(rows)
        self.cls[rows, c] = (hi - np.arange(len(rows)) / 256.0).astype(F32)
        return self


def chain_case(name, group, imgs, *, step=8, nms_thresh=0.7, check=None, edge=None, **kw):
    kw.setdefault("score_thresh", 0.001)        # a row that is a candidate of two classes shares its mass
    imgs = imgs if isinstance(imgs, (list, tuple)) else [imgs]
    region, pos = np.stack([i.region for i in imgs]), np.stack([i.pos for i in imgs])
    R, C = imgs[0].R, imgs[0].C
    own = check

    def chk(case, ref):
        check_closed_form(case, ref)
        if own is not None:
            own(case, ref)

    return Case(name, group, chain_boxes(region, pos, step), [i.rcount for i in imgs], np.stack([i.cls for i in imgs]),
                np.zeros((len(imgs), R, 4 * C), F32), nms_thresh=nms_thresh, check=chk, edge=edge, region=region,
                pos=pos, step=step, **kw)


def _rng(seed):
    return np.random.default_rng(seed)


def _quads(R):
    """Regions of four positions: every region is a chain of four."""
    return np.arange(R) // 4, np.arange(R) % 4


def _random_case(name, N, R, C, seed, *, scale=3.0, rcount=None, img=(100.0, 160.0), **kw):
    """Random logits and nonzero reg on overlapping RoIs (no closed form: the reference decides)."""
    g = _rng(seed)
    y0, x0 = g.integers(0, 60, (N, R)), g.integers(0, 100, (N, R))
    rois = np.stack([y0, x0, y0 + g.integers(8, 40, (N, R)), x0 + g.integers(8, 60, (N, R))], -1).astype(F32)
    cls = (g.standard_normal((N, R, C)) * scale).astype(F32)
    reg = (g.standard_normal((N, R, 4 * C)) * 0.5).astype(F32)
    rc = np.full(N, R) if rcount is None else rcount
    return Case(name, "softmax", rois, rc, cls, reg, img_h=img[0], img_w=img[1], **kw)


# ------------------------------------------------------------------------ the cases
def _build():
    cases = []
    add = cases.append

    # ================= compaction: the candidate count at each wave, block and kernel edge
    def cc_case(cc):
        R = 1024
        g = _rng(cc)
        rows = np.sort(g.permutation(R)[:cc])                       # scattered over the 16 waves
        order = rows[g.permutation(cc)]
        region = np.arange(R) // 2                                  # pairs of identical boxes
        if cc:
            region[order[-1]] = 1023                                # but the last candidate: it is kept
        im = Img(R, 2, region=region).put(1, order)

        def check(c, ref, cc=cc):
            assert len(c.probs(0)[1][0]) == cc
            if cc:
                distinct_scores(c, 0, 1)
            if cc > 64:         # the last block keeps something and, where it has 63 or 64 rows, drops something
                last = c.ranked(0, 1)[(cc - 1) // 64 * 64:]
                k = np.isin(last, kept_rows(ref, 0, 1))
                assert k.any() and (len(last) < 63 or not k.all())

        def edge(c, m, cc=cc):
            assert m.cc(0, 1) == cc and m.nblocks(0, 1) == (cc + 63) // 64
            assert m.last_block_rows(0, 1) == (((cc - 1) % 64 + 1) if cc else 0)

        return chain_case(f"cc_{cc}", "compact", im, check=check, edge=edge, half=cc >= 63)

    for cc in (0, 1, 63, 64, 65, 127, 128, 129, 1023, 1024):
        add(cc_case(cc))

    rows = np.concatenate([np.arange(5, 41), np.arange(128 + 3, 128 + 51), np.arange(961, 1024)])
    im = Img(1024, 2, *_quads(1024)).put(1, rows[_rng(3).permutation(len(rows))])
    add(chain_case("cc_waves_0_2_15", "compact", im, half=True,
                   check=lambda c, ref: distinct_scores(c, 0, 1),
                   edge=lambda c, m: (m.expect(m.waves(0, 1) == [0, 2, 15]), m.expect(m.nw == 16))))

    def r_case(R):
        im = Img(R, 3, *_quads(R))
        perm = _rng(R).permutation(R)
        im.put(1, perm).put(2, perm[::-1][:max(R // 2, 1)])          # a row is a candidate of both classes

        def edge(c, m, R=R):
            assert m.threads == (R + 63) // 64 * 64 and m.cc(0, 1) == R and m.threads - R == (-R) % 64

        return chain_case(f"R_{R}", "compact", im, edge=edge, half=R in (65, 1000),
                          check=lambda c, ref: _ok(c.R == 1 or len(kept_rows(ref, 0, 1)) < c.R))

    for R in (1, 63, 64, 65, 1000, 1024):
        add(r_case(R))

    # ================= rcount below 0, inside and above R; the rows past it hold logits of 50 and reg of 1e30
    def rcount_case(tag, R, rc):
        k = int(np.clip(rc, 0, R))
        ims = [Img(R, 3, *_quads(R)), Img(R, 3, *_quads(R))]
        for i, im in enumerate(ims):
            perm = _rng(R + i).permutation(R)
            im.put(1, perm).put(2, perm[::-2])
            im.cls[k if i == 0 else R:] = 50.0
        ims[0].rcount = rc

        def check(c, ref, k=k):
            assert c.valid_rows(0) == k and (c.cls[0, k:] == 50).all() and (c.reg[0, k:] == 1e30).all()
            assert ref[5][1] > c.R // 2 and (ref[5][0] > 0) == (k > 0) and (ref[3][0] < k).all()
            assert k == 0 or k - 1 in c.ranked(0, 1)                  # row k - 1 is in, row k is not

        def edge(c, m, k=k):
            assert m.cc(0, 1) == k and m.cc(1, 1) == c.R

        c = chain_case(f"rcount_{tag}", "rcount", ims, check=check, edge=edge, half=tag == "65_of_1024")
        reg = c.reg.copy()
        reg[0, k:] = 1e30
        return Case(c.name, "rcount", c.rois, c.rcount, c.cls, reg, score_thresh=c.score_thresh, nms_thresh=0.7,
                    check=c.check, edge=edge, half=c.half, region=c.region, pos=c.pos, step=8)

    for tag, R, rc in (("m5", 128, -5), ("0", 128, 0), ("1", 128, 1), ("65_of_1024", 1024, 65), ("R", 128, 128),
                       ("R_plus_7", 128, 135), ("int32_max", 128, I32_MAX), ("int32_min", 128, I32_MIN)):
        add(rcount_case(tag, R, rc))

    # ================= the score filter
    def filter_img():
        im = Img(64, 3, *_quads(64))
        perm = _rng(64).permutation(64)
        return im.put(1, perm, hi=1.0).put(2, perm[::-1][:20], hi=0.5), int(perm[40])

    im, row = filter_img()
    p_row = F32(detect_ref.softmax(im.cls)[row, 1])
    below = np.nextafter(p_row, F32(0))

    def check_equal(c, ref):
        p = c.probs(0)[0]
        assert bits(p[:, 1])[c.row] == bits(F32(c.score_thresh)) and c.row not in kept_rows(ref, 0, 1)
        assert (p[:, 1] > p[c.row, 1]).sum() == 40 == len(c.ranked(0, 1))          # the filter is strict

    def check_below(c, ref):
        p = c.probs(0)[0]
        assert F32(c.score_thresh) < p[c.row, 1] and np.nextafter(F32(c.score_thresh), F32(1)) == p[c.row, 1]
        assert c.ranked(0, 1)[-1] == c.row and len(c.ranked(0, 1)) == 41

    for name, thr, chk, n in (("thresh_equal", p_row, check_equal, 40), ("thresh_below", below, check_below, 41)):
        im, row = filter_img()
        c = chain_case(name, "filter", im, score_thresh=thr, check=chk, edge=lambda c, m, n=n: m.expect(m.cc(0, 1) == n))
        c.row = row
        add(c)

    nan_neg = np.array([0xFFC00001], np.uint32).view(F32)[0]
    im, row = filter_img()
    im.cls[row] = np.nan
    other = row + 1 if row < 63 else 0
    im.cls[other, 2] = nan_neg                            # one NaN logit: the whole row is NaN

    def check_nan(c, ref, row=row, other=other):
        p = c.probs(0)[0]
        assert np.isnan(p[[row, other]]).all() and not np.isin([row, other], ref[3][0]).any() and ref[5][0] > 20

    add(chain_case("nan_row", "filter", im, check=check_nan, edge=lambda c, m: m.expect(m.cc(0, 1) == 62)))

    # a negative threshold: a probability that underflowed to +0 is a candidate, a denormal one too, NaN is not
    im = Img(64, 3, *_quads(64))
    im.cls[:, 1] = np.where(np.arange(64) % 3 == 0, -200.0, np.where(np.arange(64) % 3 == 1, -100.0, 1.0))
    im.cls[:, 2] = np.where(np.arange(64) % 2 == 0, -200.0, 0.25)
    im.cls[11] = np.nan

    def check_negative(c, ref):
        p = c.probs(0)[0]
        assert (bits(p[0::3, 1][:3]) == 0).all()                     # +0
        assert 0 < p[1, 1] < np.finfo(F32).tiny                      # a denormal probability
        assert len(c.ranked(0, 1)) == 63 and 11 not in c.ranked(0, 1)
        sc = ref[2][0, :int(ref[4][0])][ref[1][0, :int(ref[4][0])] == 1]
        assert (bits(sc) == 0).any() and ((sc > 0) & (sc < np.finfo(F32).tiny)).any()    # both kinds are kept

    add(chain_case("thresh_negative", "filter", im, score_thresh=-1.0, check=check_negative,
                   edge=lambda c, m: m.expect(m.cc(0, 1) == 63 and m.cc(0, 2) == 63)))

    im = Img(64, 3, *_quads(64)).put(2, _rng(9).permutation(64)[:30])
    im.cls[7, 1], im.cls[21, 1], im.cls[40, 1] = 100.0, 200.0, 3.0

    def check_one(c, ref):
        p = c.probs(0)[0]
        assert bits(p[7, 1]) == bits(p[21, 1]) == bits(F32(1)) and p[7, 0] > 0 and p[21, 0] == 0
        assert kept_rows(ref, 0, 1).tolist() == [7, 21, 40] and bits(ref[2][0, 0]) == bits(F32(1))

    add(chain_case("prob_one", "filter", im, check=check_one, edge=lambda c, m: m.expect(m.cc(0, 1) == 3)))

    # ================= rank sort: R = 1,024 keys in 16 waves, chains of four so that the order decides the keep list
    def sort_case(name, logits, check):
        im = Img(1024, 2, *_quads(1024))
        im.cls[:, 1] = logits
        return chain_case(name, "sort", im, check=check, half=name == "sort_shuffle",
                          edge=lambda c, m: m.expect(m.cc(0, 1) == 1024 and m.nw == 16))

    def check_all_equal(c, ref):
        p = c.probs(0)[0][:, 1]
        assert len(np.unique(bits(p))) == 1
        assert np.array_equal(c.ranked(0, 1), np.arange(1024))
        assert np.array_equal(kept_rows(ref, 0, 1), np.arange(1024)[np.arange(1024) % 4 % 2 == 0])

    add(sort_case("sort_all_equal", np.full(1024, 0.75, F32), check_all_equal))

    def check_pairs(c, ref):
        p = c.probs(0)[0][:, 1]
        assert np.array_equal(bits(p[:512]), bits(p[512:])) and len(np.unique(bits(p))) == 512
        order = c.ranked(0, 1)
        assert (order[0::2] + 512 == order[1::2]).all()              # the lower row of a pair first, eight waves apart

    v = (_rng(12).permutation(512) / 128.0).astype(F32)
    add(sort_case("sort_equal_pairs_across_waves", np.concatenate([v, v]), check_pairs))
    ramp = (np.arange(1024) / 256.0).astype(F32)
    add(sort_case("sort_descending", ramp[::-1].copy(),
                  lambda c, ref: _ok(np.array_equal(distinct_scores(c, 0, 1), np.arange(1024)))))
    add(sort_case("sort_ascending", ramp,
                  lambda c, ref: _ok(np.array_equal(distinct_scores(c, 0, 1), np.arange(1024)[::-1]))))
    add(sort_case("sort_shuffle", ramp[_rng(13).permutation(1024)], lambda c, ref: distinct_scores(c, 0, 1)))

    # ================= the block sweep
    # a chain over the block edges at 64 and 128: class 1 starts at rank 0 (even ranks kept), class 2 at rank 1
    R = 131
    pos = np.arange(R)
    pos[130] = 135                       # one box off the chain's end: rank 0 of class 2
    im = Img(R, 3, region=np.zeros(R, np.int64), pos=pos)
    im.put(1, np.arange(130)).put(2, np.concatenate([[130], np.arange(130)]))

    def check_chain(c, ref):
        assert np.array_equal(distinct_scores(c, 0, 1), np.arange(130))
        assert np.array_equal(kept_rows(ref, 0, 1), np.arange(0, 130, 2))            # ranks 0, 2, 4, ...
        assert np.array_equal(kept_rows(ref, 0, 2), np.concatenate([[130], np.arange(0, 130, 2)]))

    def edge_chain(c, m):
        d1, d2 = m.decided(0, 1), m.decided(0, 2)
        assert d1[62:66] == ["kept", "mask", "kept", "mask"] and d1[126:130] == ["kept", "mask", "kept", "mask"]
        assert d2[63:66] == ["kept", "klist", "kept"] and d2[127:130] == ["kept", "klist", "kept"]
        assert m.nblocks(0, 1) == 3 and m.last_block_rows(0, 1) == 2 and m.last_block_rows(0, 2) == 3

    add(chain_case("chain_over_block_edges", "sweep", im, check=check_chain, edge=edge_chain, half=True))

    def sweep_case(name, R, special, edge, check=None, half=True, C=2):
        """Rank r is row perm[r] in a region of its own at position 0, but for ``special``
        {rank: (rank whose region it shares, pos)}."""
        perm = _rng(R + len(special)).permutation(R)
        region, pos = np.zeros(R, np.int64), np.zeros(R, np.int64)
        for rank in range(R):
            region[perm[rank]], pos[perm[rank]] = special.get(rank, (rank, 0))
        im = Img(R, C, region=region, pos=pos).put(1, perm)
        c = chain_case(name, "sweep", im, check=check, edge=edge, half=half)
        c.perm = perm
        return c

    def edge_last(c, m):
        d = m.decided(0, 1)
        assert m.nblocks(0, 1) == 16 and d[1000] == "klist" and m.suppressor(0, 1, 1000) == 5 and d.count("kept") == 1023

    add(sweep_case("last_block_by_block0", 1024, {1000: (5, 1)}, edge_last,
                   lambda c, ref: _ok(c.perm[1000] not in kept_rows(ref, 0, 1) and distinct_scores(c, 0, 1) is not None)))

    sp = {64 + t: ((t * 37) % 64, t % 2) for t in range(64)}       # block 1: duplicates and neighbours of block 0's

    def edge_empty(c, m):
        assert m.block_kept(0, 1) == [64, 0, 13] and m.klist_before(0, 1, 2) == 64
        assert set(m.decided(0, 1)[64:128]) == {"klist"}

    add(sweep_case("block_keeps_nothing", 141, sp, edge_empty))

    def edge_t1(c, m):
        assert m.decided(0, 1)[:3] == ["kept", "mask", "kept"] and m.nblocks(0, 1) == 1

    add(sweep_case("not_transitive_one_block", 40, {1: (0, 1), 2: (0, 2)}, edge_t1, half=False,
                   check=lambda c, ref: _ok(len(kept_rows(ref, 0, 1)) == 39)))

    def edge_t3(c, m):
        d = m.decided(0, 1)
        assert (d[3], d[70], d[140]) == ("kept", "klist", "kept") and m.block_of(140) == 2 and m.suppressor(0, 1, 70) == 3

    add(sweep_case("not_transitive_three_blocks", 200, {70: (3, 1), 140: (3, 2)}, edge_t3,
                   check=lambda c, ref: _ok(len(kept_rows(ref, 0, 1)) == 199)))

    # a kept list longer than the number of waves before the block that reads it: the `i += nw` stride and its
    # break.  Block 1's candidates 64 + t are suppressed by kept-list entry (37 t) mod 64, every residue of nw
    sp = {64 + t: ((t * 37) % 64, 1) for t in range(48)}
    for R in (64, 128, 1024):
        def edge_stride(c, m, R=R):
            assert m.nw == R // 64
            if R == 64:      # one wave owns at most 64 rows: one block, the kept list is written and never read
                assert m.nblocks(0, 1) == 1 and m.block_kept(0, 1) == [64]
                return
            assert m.klist_before(0, 1, 1) == 64 > m.nw and m.block_kept(0, 1)[:2] == [64, 16]
            hit = {m.suppressor(0, 1, 64 + t) % m.nw for t in range(48)}
            assert hit == set(range(m.nw)) and {m.suppressor(0, 1, 64 + t) // m.nw for t in range(48)} >= {0, 1, 3}

        add(sweep_case(f"klist_stride_R{R}", R, sp if R > 64 else {}, edge_stride, half=R == 1024))

    # ================= thresholds and degenerate boxes
    def plain(name, boxes, *, C=2, group="thr", img=(64.0, 64.0), scores=None, **kw):
        k = len(boxes)
        cls = np.full((1, k, C), NEG, F32)
        cls[0, :, 0] = 0
        cls[0, :, 1] = (4.0 - np.arange(k) / 256.0) if scores is None else scores
        if C > 2:
            cls[0, :, 2] = cls[0, ::-1, 1]
        return Case(name, group, np.asarray(boxes, F32)[None], [k], cls, np.zeros((1, k, 4 * C), F32), img_h=img[0],
                    img_w=img[1], **kw)

    pair = [[0, 0, 10, 3], [0, 1, 10, 4], [20, 0, 30, 3]]

    def check_half(c, ref):
        assert bits(iou_matrix(c.rois[0])[0, 1]) == bits(F32(0.5))
        assert kept_rows(ref, 0, 1).tolist() == ([0, 1, 2] if c.nms_thresh >= 0.5 else [0, 2])

    one_block = lambda c, m: m.expect(m.nblocks(0, 1) == 1)            # noqa: E731
    add(plain("iou_at_thresh", pair, nms_thresh=0.5, check=check_half, edge=one_block))
    add(plain("iou_over_thresh_f64", pair, nms_thresh=float(np.nextafter(0.5, 0.0)), check=check_half, edge=one_block))
    add(plain("iou_over_thresh_f32", pair, nms_thresh=float(np.nextafter(F32(0.5), F32(0))), check=check_half,
              edge=one_block))

    g = _rng(21)
    y0, x0 = g.integers(0, 40, 150), g.integers(0, 40, 150)
    crowd = np.stack([y0, x0, y0 + g.integers(4, 24, 150), x0 + g.integers(4, 24, 150)], 1)
    crowd[100:] = crowd[:50]                                            # identical pairs: IoU exactly 1

    def check_never(c, ref):
        assert ref[5][0] == 300 and over_matrix(c.rois[0], 0.3).sum() > 600

    add(plain("nms_nan", crowd, C=3, nms_thresh=float("nan"), check=check_never,
              edge=lambda c, m: m.expect(m.nblocks(0, 1) == 3 and m.block_kept(0, 1) == [64, 64, 22])))
    add(plain("nms_one", crowd, C=3, nms_thresh=1.0, check=check_never,
              edge=lambda c, m: m.expect(m.block_kept(0, 2) == [64, 64, 22])))

    def check_tight(c, ref):
        assert ref[5][0] == 200 and 100 not in kept_rows(ref, 0, 1) and 49 not in kept_rows(ref, 0, 2)

    add(plain("nms_just_below_one", crowd, C=3, nms_thresh=float(np.nextafter(1.0, 0.0)), check=check_tight,
              edge=lambda c, m: m.expect(m.decided(0, 1)[100] == "klist")))
    far = [[10 * i, 0, 10 * i + 5, 5] for i in range(6)] + [[0, 20, 5, 25]] * 2 + [[40 * i, 30, 40 * i + 9, 39] for i in range(70)]

    def check_negative_thr(c, ref):
        assert over_matrix(c.rois[0, :6], 0.0).sum() == 6                 # disjoint boxes
        assert ref[5][0] == 2 and ref[3][0, :2].tolist() == [0, 77]     # one box per class: the best of each

    add(plain("nms_negative", far, C=3, img=(4096.0, 64.0), nms_thresh=-0.5, check=check_negative_thr,
              edge=lambda c, m: m.expect(m.block_kept(0, 1) == [1, 0])))

    def zero_area(name, k, blocks):
        g = _rng(k)
        boxes = [[8, 70 + int(g.integers(0, 20)), 24, 100 + int(g.integers(0, 20))] for _ in range(k)]    # past the width
        boxes += [[40, 8 * i, 60, 8 * i + 30] for i in range(6)]

        def check(c, ref):
            rows = np.arange(k)
            b = c.decoded(0, 1, rows)
            assert (b == np.array([8, 64, 24, 64], F32)).all()          # identical, zero width
            assert np.isnan(iou_matrix(b)).all()                        # uni == 0: the quotient is 0 / 0
            assert np.isin(rows, kept_rows(ref, 0, 1)).all() and 0 < len(kept_rows(ref, 0, 1)) - k < 6

        return plain(name, boxes, img=(64.0, 64.0), check=check, scores=(4.0 - g.permutation(k + 6) / 256.0).astype(F32),
                     edge=lambda c, m: m.expect(m.nblocks(0, 1) == blocks))

    add(zero_area("zero_area_one_block", 9, 1))
    add(zero_area("zero_area_two_blocks", 90, 2))

    # the default threshold 0.3 with its own spacing: 24 along the 64-long side
    im = Img(130, 3, region=np.zeros(130, np.int64), pos=np.arange(130)).put(1, np.arange(130)).put(2, np.arange(129, -1, -1))
    add(chain_case("chain_default_thresh", "sweep", im, step=24, nms_thresh=0.3, half=True,
                   check=lambda c, ref: _ok(np.array_equal(kept_rows(ref, 0, 2), np.arange(129, -1, -2))),
                   edge=lambda c, m: m.expect(m.decided(0, 1)[63:65] == ["mask", "kept"])))
    im = Img(200, 2, np.arange(200) // 8, np.arange(200) % 8).put(1, _rng(31).permutation(200))
    add(chain_case("shuffle_default_thresh", "sweep", im, step=24, nms_thresh=0.3,
                   check=lambda c, ref: distinct_scores(c, 0, 1),
                   edge=lambda c, m: m.expect(m.nblocks(0, 1) == 4 and "klist" in m.decided(0, 1) and "mask" in m.decided(0, 1))))

    # ================= emit: 1,024 slots per workgroup
    def emit_case(name, counts, *, R=1024, C=None, max_det=None, half=False, edge=None):
        """counts {class: candidates}: disjoint boxes, so the class keeps them all."""
        C = C or max(counts) + 1
        im = Img(R, C)
        for i, (c, k) in enumerate(sorted(counts.items())):
            im.put(c, _rng(100 * c + k).permutation(R)[:k], hi=4.0 - i / 512.0)
        total = sum(counts.values())

        def check(c, ref):
            assert ref[5][0] == total and ref[4][0] == min(total, c.max_det)
            assert [int((ref[1][0] == k).sum()) for k in sorted(counts)] == [
                int(np.clip(c.max_det - sum(v for kk, v in counts.items() if kk < k), 0, counts[k])) for k in sorted(counts)]

        return chain_case(name, "emit", im, check=check, edge=edge, max_det=max_det, half=half)

    for total, counts in ((1023, {1: 1023}), (1024, {1: 1024}), (1025, {1: 1024, 2: 1})):
        add(emit_case(f"emit_total_{total}", counts, C=3, half=True,
                      edge=lambda c, m, t=total: m.expect(m.total(0) == t and m.emit_groups == 2
                                                          and m.emit_wg(t - 1) == (t - 1) // 1024)))
    for total, counts in ((2048, {1: 1024, 2: 1024}), (2049, {1: 1024, 2: 1024, 3: 1})):
        add(emit_case(f"emit_total_{total}", counts, C=4, half=True,
                      edge=lambda c, m, t=total: m.expect(m.total(0) == t and m.emit_groups == 3 and m.emit_wg(t - 1) == 2 - (t == 2048))))
    for md in (1, 1199, 1200, 1201, 1025, 3000):
        def edge_md(c, m, md=md):
            assert m.total(0) == 1200 and m.emit_groups == (md + 1023) // 1024
            assert m.last_group_slots == (md - 1) % 1024 + 1
        add(emit_case(f"maxdet_{md}", {1: 700, 2: 500}, max_det=md, half=md == 1025, edge=edge_md))
    add(emit_case("C2", {1: 77}, R=100, C=2, edge=lambda c, m: m.expect(c.C == 2 and m.total(0) == 77)))
    for name, counts in (("C128_class_1", {1: 9}), ("C128_class_127", {127: 9}), ("C128_classes_1_127", {1: 5, 127: 7})):
        add(emit_case(name, counts, R=64, C=128,
                      edge=lambda c, m, k=counts: m.expect(c.C == 128 and m.populated(0) == sorted(k))))
    runs = {3: 5, 4: 1, 9: 12, 20: 3}
    add(emit_case("emit_empty_runs", runs, R=64, C=21, half=True,
                  edge=lambda c, m: m.expect(m.populated(0) == [3, 4, 9, 20] and m.equal_offsets(0) >= 14)))
    add(emit_case("emit_empty_runs_truncated", runs, R=64, C=21, max_det=10,
                  edge=lambda c, m: m.expect(m.populated(0) == [3, 4, 9, 20] and m.total(0) == 21)))

    # ================= softmax: eight rows per workgroup, 8 x 128 logits of LDS
    def edge_span(c, m):
        spans = [m.softmax_images(w) for w in range(m.softmax_groups)]
        assert max(len(s) for s in spans) == 4 and min(len(s) for s in spans[:-1]) == 3
        assert any(len({int(c.rcount[n]) for n in s}) >= 3 for s in spans)

    def check_span(c, ref):
        assert c.rcount[:8].tolist() == [0, 1, 2, 3, 0, 1, 2, 3] and (ref[5][c.rcount == 0] == 0).all()
        assert (ref[5] > 0).sum() > 300 and (ref[3] < c.rcount[:, None]).all()

    c = _random_case("softmax_wg_spans_images", 1000, 3, 5, 41, rcount=np.arange(1000) % 4, half=True,
                     check=check_span, edge=edge_span)
    cls = c.cls.copy()
    for n in range(1000):
        cls[n, int(c.rcount[n]):] = 50.0                              # what lies past rcount must not be read
    add(Case(c.name, "softmax", c.rois, c.rcount, cls, c.reg, img_h=c.img_h, img_w=c.img_w, check=check_span,
             edge=edge_span, half=True))

    def check_c128(c, ref):
        cc = [len(r) for r in c.probs(0)[1]]
        assert max(cc) <= 16 and sum(cc) > 40 and ref[5].min() > 20

    add(_random_case("softmax_C128_rows", 2, 20, 128, 42, scale=2.5, half=True, check=check_c128,
                     edge=lambda c, m: m.expect(c.C == m.max_c and m.softmax_groups == 5)))

    c = _random_case("softmax_big_logits", 1, 40, 6, 43, half=True)
    cls = c.cls.copy()
    cls[0, :30] = np.where(_rng(44).integers(0, 2, (30, 6)) == 1, 1e4, -1e4)      # rows of +-1e4: e is 0 or 1
    cls[0, 5], cls[0, 6] = 1e4, -1e4

    def check_big(c, ref):
        p = c.probs(0)[0]
        assert np.isfinite(p).all() and (p[5] == F32(1) / F32(6)).all() and (p[6] == p[5]).all()
        assert (p[:30] == 0).any() and set(np.unique(p[:30])) <= {F32(1) / F32(k) for k in range(1, 7)} | {F32(0)}
        assert ref[5][0] > 10

    add(Case(c.name, "softmax", c.rois, c.rcount, cls, c.reg, img_h=c.img_h, img_w=c.img_w, check=check_big,
             edge=lambda c, m: m.expect(m.softmax_groups == 5), half=True))

    c = _random_case("softmax_inf_row", 1, 40, 6, 45)
    cls = c.cls.copy()
    cls[0, 3, 2] = np.inf               # inf - inf: the whole row is NaN
    cls[0, 9, 1] = -np.inf              # exp(-inf) = 0: an ordinary row
    cls[0, 12] = -np.inf                # all -inf: NaN again
    cls[0, 20, 1:] = 2.0

    def check_inf(c, ref):
        p = c.probs(0)[0]
        assert np.isnan(p[3]).all() and np.isnan(p[12]).all() and p[9, 1] == 0 and np.isfinite(p[9]).all()
        assert not np.isin([3, 12], ref[3][0]).any() and ref[5][0] > 10

    add(Case(c.name, "softmax", c.rois, c.rcount, cls, c.reg, img_h=c.img_h, img_w=c.img_w, check=check_inf,
             edge=lambda c, m: m.expect(m.cc(0, 2) <= 38 and m.softmax_groups == 5), half=True))

    # ================= a batch of three unlike images: each must come out as it does alone
    by = {c.name: c for c in cases}
    parts = [by[n] for n in ("cc_129", "sort_equal_pairs_across_waves", "cc_waves_0_2_15")]

    def check_batch(c, ref):
        for n, part in enumerate(c.parts):
            same_bits([a[n:n + 1] for a in ref], part.reference(), f"image {n} = {part.name}")
        assert len(set(int(t) for t in ref[5])) == 3

    add(Case("batch_three", "batch", np.concatenate([p.rois for p in parts]), np.concatenate([p.rcount for p in parts]),
             np.concatenate([p.cls for p in parts]), np.concatenate([p.reg for p in parts]), nms_thresh=0.7,
             check=check_batch, half=True, parts=parts,
             edge=lambda c, m: m.expect([m.cc(n, 1) for n in range(3)] == [129, 1024, 147])))
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
NAMES = tuple(BY_NAME)
HALF_NAMES = tuple(c.name for c in CASES if c.half)      # the 16-bit subset, by name
