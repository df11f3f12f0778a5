"""Named edge cases of target assignment (utils/utils.py:122-276): ties, exact
thresholds, padding, sizes at the kernels' wave / block / round edges,
non-finite boxes and non-default sampling parameters.  Plain numpy, no GPU.

Every case carries its inputs and a ``check(case, out)`` that asserts the
case's precondition on the ORACLE's outputs alone (``anchor_oracle`` /
``proposal_oracle`` below), so a change to a generator cannot silently turn a
case into an easy one.  Users: tests/test_target_cases_cpu.py (the checks),
tests/golden/make_golden.py (the genuine reference over the same table),
tests/test_oracle_golden.py (oracle == reference) and
tests/test_gpu_target_edges.py (HIP path == oracle).
"""
from __future__ import annotations

import numpy as np

from oracle import ref_numpy as orc


class AnchorCase:
    """anchors fp32 [A,4]; boxes fp64 [N,G,4] / labels fp64 [N,G] (label -1 =
    padding); kw = AnchorTargetCreator's constructor arguments; seed = numpy's
    global MT19937 seed before image 0."""

    kind = "anchor"

    def __init__(self, name, anchors, boxes, labels, check, seed=1, **kw):
        self.name, self.anchors, self.boxes, self.labels = name, anchors, boxes, labels
        self.check, self.seed, self.kw = check, seed, kw

    def gt(self, i):
        return self.boxes[i, self.labels[i] != -1]


class ProposalCase:
    """rois fp32 [N,Rp,4] with rcount [N] valid rows each; boxes / labels as
    above; kw = ProposalTargetCreator's constructor arguments; norm = the
    (mean, std) given to __call__."""

    kind = "proposal"

    def __init__(self, name, rois, rcount, boxes, labels, check, seed=1, norm=None, **kw):
        self.name, self.rois, self.rcount, self.boxes, self.labels = name, rois, rcount, boxes, labels
        self.check, self.seed, self.kw = check, seed, kw
        self.norm = norm if norm is not None else ((0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2))

    def image(self, i):
        v = self.labels[i] != -1
        return self.rois[i, :int(self.rcount[i])], self.boxes[i, v], self.labels[i][v]


# ------------------------------------------------------------------ the oracle
_cache = {}


def _with_seed(case, body):
    """body() on numpy's global RNG seeded with case.seed; the caller's state is
    restored.  Returns (images, state before, state after)."""
    saved = np.random.get_state()
    try:
        np.random.seed(case.seed)
        st0 = np.random.get_state()
        with np.errstate(all="ignore"):
            images = body()
        return images, st0, np.random.get_state()
    finally:
        np.random.set_state(saved)


def anchor_oracle(case):
    """The oracle's per-image loop over ``case`` (computed once per case): a dict
    with images = [{reg, label, argmax, max_iou, rng_pos, rng_key}], rng_in, rng_out."""
    if case.name not in _cache:
        def body():
            out = []
            for i in range(len(case.boxes)):
                reg, lab, am, mx = orc.anchor_target(case.gt(i), case.anchors, return_internals=True, **case.kw)
                st = np.random.get_state()
                out.append({"reg": reg, "label": lab, "argmax": np.asarray(am), "max_iou": np.asarray(mx, np.float64),
                            "rng_pos": st[2], "rng_key": st[1].copy()})
            return out
        images, st0, st1 = _with_seed(case, body)
        _cache[case.name] = {"images": images, "rng_in": st0, "rng_out": st1}
    return _cache[case.name]


def proposal_oracle(case):
    """As ``anchor_oracle``: images = [{roi, reg, label, rng_pos, rng_key}]."""
    if case.name not in _cache:
        def body():
            out = []
            for i in range(len(case.boxes)):
                roi, gt, gl = case.image(i)
                s_roi, s_reg, s_lab = orc.proposal_target(roi, gt, gl, reg_normalize_mean=case.norm[0],
                                                          reg_normalize_std=case.norm[1], **case.kw)
                st = np.random.get_state()
                out.append({"roi": s_roi, "reg": s_reg, "label": s_lab, "rng_pos": st[2], "rng_key": st[1].copy()})
            return out
        images, st0, st1 = _with_seed(case, body)
        _cache[case.name] = {"images": images, "rng_in": st0, "rng_out": st1}
    return _cache[case.name]


def oracle(case):
    return anchor_oracle(case) if case.kind == "anchor" else proposal_oracle(case)


def _ious(case, i):
    with np.errstate(all="ignore"):
        return orc.bbox_iou(case.anchors, case.gt(i))


def _pt_ious(case, i):
    roi, gt, _ = case.image(i)
    with np.errstate(all="ignore"):
        return orc.bbox_iou(np.concatenate([roi.astype(np.float64), gt]), gt)


def _one(boxes):
    b = np.asarray(boxes, np.float64).reshape(1, -1, 4)
    return b, np.ones(b.shape[:2])


def _int_boxes(r, n, h, w, lo=8):
    """n integer boxes (fp64) inside an h x w image, sides >= lo."""
    y0 = r.integers(0, h - lo, n)
    x0 = r.integers(0, w - lo, n)
    y1 = y0 + lo + (r.integers(0, 1 << 30, n) % (h - lo - y0 + 1))
    x1 = x0 + lo + (r.integers(0, 1 << 30, n) % (w - lo - x0 + 1))
    return np.stack([y0, x0, y1, x1], 1).astype(np.float64)


def base_grid():
    """315 anchors (7 x 5 x 9, stride 16) over a 112 x 80 image."""
    return orc.generate_anchors(orc.generate_anchor_base(), 16, 7, 5)


# ------------------------------------------------------- AnchorTarget's cases
_TIES_GT = [[0, 0, 112, 80], [4, 2, 108, 76], [0, 0, 96, 80], [16, 0, 112, 80], [8, 8, 104, 64]]


def _ties_inputs():
    B = base_grid()
    return (np.concatenate([B, B, B[:70]]),) + _one(_TIES_GT)


def _check_dup_anchor_ties(case, out):
    iou = _ious(case, 0)
    assert len(case.anchors) == 700 and iou.shape == (700, 5)
    assert ((iou == iou.max(axis=0)).sum(axis=0) >= 2).all(), "every gt column ties"
    gt_argmax = iou.argmax(axis=0)
    assert (gt_argmax < 315).all(), "the first of the tied rows"
    im = out["images"][0]
    assert (im["label"][gt_argmax] == 1).all(), "fewer than 128 positives: nothing is disabled"
    # the tied copy 315 rows later is no gt's argmax: positive only by the threshold
    dup = gt_argmax + 315
    assert np.array_equal(im["label"][dup] == 1, im["max_iou"][dup] >= 0.7) and (im["label"][dup] != 1).any()


def _check_dup_gt(case, out):
    iou = _ious(case, 0)
    G = iou.shape[1]
    gt_argmax = iou.argmax(axis=0)
    assert len(set(gt_argmax.tolist())) < G
    am, mx = out["images"][0]["argmax"], out["images"][0]["max_iou"]
    assert gt_argmax[0] == gt_argmax[1] and am[gt_argmax[0]] == 1, "identical gt: the later one at the shared anchor"
    assert gt_argmax[2] == gt_argmax[3] != gt_argmax[0] and am[gt_argmax[2]] == 3, "concentric gt: the later one"
    rows = [a for a in range(len(mx)) if a not in gt_argmax and mx[a] > 0
            and iou[a, 0] == mx[a] == iou[a, 1] and am[a] == 0]
    assert rows, "a row with two equal maxima takes the lower gt index"


def _check_no_overlap(case, out):
    iou = _ious(case, 0)
    assert iou[:, 1].max() == 0 and iou.argmax(axis=0)[1] == 0
    im = out["images"][0]
    assert im["label"][0] == 1 and im["argmax"][0] == 1 and im["max_iou"][0] > 0


def _check_thr_equal(case, out):
    im = out["images"][0]
    mx, lab = im["max_iou"], im["label"]
    gt_argmax = _ious(case, 0).argmax(axis=0)
    assert gt_argmax.tolist() == [0, 3]
    assert mx[1] == 0.7 and mx[2] == 0.7 and mx[4] == 0.3 and mx[5] == 0.3
    assert lab[1] == 1 and lab[2] == 1, "max_iou == pos_iou_thresh is positive (>=)"
    if case.kw.get("neg_iou_thresh", 0.3) == 0.3 and case.kw.get("pos_iou_thresh", 0.7) == 0.7:
        assert lab[4] == -1 and lab[5] == -1, "max_iou == neg_iou_thresh is not negative (<)"
    else:
        assert lab[4] == 1 and lab[5] == 1, "pos == neg == 0.3: >= wins over <"


_PAD_ROWS = [0, 5, 6, 7, 8, 9, 63, 64, 69]


def _check_pad_interleaved(case, out):
    lab = case.labels
    assert lab.shape == (3, 70)
    assert np.nonzero(lab[0] == -1)[0].tolist() == _PAD_ROWS
    assert (lab[1] == -1).all() and (lab[2] != -1).all()
    assert not np.isfinite(case.boxes[0, _PAD_ROWS]).all() and np.isfinite(case.gt(0)).all()
    assert not (out["images"][1]["label"] == 1).any() and not out["images"][1]["reg"].any()
    # a gt past the padding is somebody's argmax: the compaction kept the order
    assert out["images"][0]["argmax"].max() > 55 and out["images"][2]["argmax"].max() > 64


def _check_g_size(G):
    def check(case, out):
        assert case.boxes.shape == (1, G, 4) and (case.labels != -1).all() and len(case.anchors) == 315
        assert (case.boxes == np.round(case.boxes)).all()
        am = out["images"][0]["argmax"]
        assert am.max() == G - 1 or G > 64, "the last gt is used"
        assert len(set(_ious(case, 0).argmax(axis=0).tolist())) <= min(G, 315)
    return check


def _check_a_size(A):
    def check(case, out):
        assert len(case.anchors) == A and case.boxes.shape == (1, 3, 4)
        gt_argmax = _ious(case, 0).argmax(axis=0)
        assert gt_argmax[2] == A - 1, "a gt whose best anchor is the last row"
        im = out["images"][0]
        assert im["label"][A - 1] == 1 and im["argmax"][A - 1] == 2
        assert abs(im["max_iou"][A - 1] - 1.0) < 1e-6   # (the anchor's area is an fp32 product: not exactly 1)
    return check


def _check_nonfinite(case, out):
    a, b = out["images"]
    assert np.isnan(a["max_iou"]).all(), "a NaN gt coordinate poisons every row (the first NaN wins)"
    assert (np.delete(a["argmax"], 100) == 1).all() and a["argmax"][100] == 2   # (row 100: gt 0's and 2's argmax)
    assert np.nonzero(np.isnan(b["max_iou"]))[0].tolist() == [100], "the NaN anchor row"
    assert np.isinf(case.gt(1)).any() and np.isfinite(np.delete(b["max_iou"], 100)).all()
    for im in (a, b):
        assert np.isin(im["label"], (-1, 0, 1)).all() and (im["label"] == 1).any()
    assert b["label"][100] == 1, "the NaN row is every gt column's argmax"


SAMPLING = [(256, .5), (16, .25), (10, .3), (100, .29), (8, 0.0), (8, 1.0), (1, .5), (4096, .5)]


def _check_sampling(n_sample, pos_ratio):
    def check(case, out):
        iou = _ious(case, 0)
        mx = iou.max(axis=1)
        pos0 = mx >= 0.3
        pos0[iou.argmax(axis=0)] = True
        neg0 = (mx < 0.1) & ~pos0
        assert pos0.sum() > 128 and neg0.sum() > 128, (pos0.sum(), neg0.sum())
        n_pos = int(pos_ratio * n_sample)
        im = out["images"][0]
        lab = im["label"]
        want_pos = min(n_pos, pos0.sum())
        assert (lab == 1).sum() == want_pos and (lab == 0).sum() == min(n_sample - want_pos, neg0.sum())
        assert (lab[~pos0] != 1).all() and (lab[~neg0] != 0).all()
        if (n_sample, pos_ratio) == (100, .29):
            assert n_pos == 28, "int() truncates 28.999..."
        if n_pos == 0:
            assert im["reg"].dtype == np.float32 and im["reg"].shape == (700, 4) and not im["reg"].any()
        else:
            assert im["reg"].dtype == np.float64
        if (n_sample, pos_ratio) == (8, 1.0):
            assert not (lab == 0).any(), "no survivor of the negatives' call"
        unchanged = (out["rng_in"][2] == out["rng_out"][2] and np.array_equal(out["rng_in"][1], out["rng_out"][1]))
        assert unchanged == (n_sample == 4096), "only n_sample = 4096 discards nothing"
    return check


def anchor_cases():
    B = base_grid()
    cases = []
    ties = _ties_inputs()
    cases.append(AnchorCase("dup_anchor_ties", *ties, _check_dup_anchor_ties, seed=11))
    a = B[4 * 9 + 3].astype(np.float64)
    cases.append(AnchorCase("dup_gt", B, *_one([[16, 16, 80, 60], [16, 16, 80, 60], a + [2, 2, -2, -2],
                                                a + [5, 5, -5, -5]]), _check_dup_gt, seed=12))
    cases.append(AnchorCase("no_overlap", B, *_one([[10, 10, 60, 50], [500, 500, 520, 520]]), _check_no_overlap,
                            seed=13))
    thr_anchors = np.array([[0, 0, 10, 10]] * 3 + [[0, 20, 10, 30]] * 3, np.float32)
    thr_gt = _one([[0, 0, 10, 7], [0, 20, 10, 23]])
    cases.append(AnchorCase("thr_equal", thr_anchors, *thr_gt, _check_thr_equal, seed=14))
    cases.append(AnchorCase("thr_equal-0.3", thr_anchors, *thr_gt, _check_thr_equal, seed=14,
                            pos_iou_thresh=0.3, neg_iou_thresh=0.3))
    r = np.random.default_rng(15)
    boxes = _int_boxes(r, 3 * 70, 112, 80).reshape(3, 70, 4)
    labels = r.integers(1, 21, (3, 70)).astype(np.float64)
    labels[0, _PAD_ROWS] = -1
    boxes[0, _PAD_ROWS] = np.array([[np.nan, 0, 5, 5], [1e30, 1e30, -1e30, -1e30], [0, 0, 112, 80]] * 3)
    labels[1] = -1
    cases.append(AnchorCase("pad_interleaved", B, boxes, labels, _check_pad_interleaved, seed=15))
    for G in (1, 63, 64, 65, 255, 256):
        cases.append(AnchorCase(f"g_sizes-{G}", B, *_one(_int_boxes(np.random.default_rng(100 + G), G, 112, 80)),
                                _check_g_size(G), seed=16))
    grid = orc.generate_anchors(orc.generate_anchor_base(), 16, 16, 16)
    for A in (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049):
        an = grid[:A]
        cases.append(AnchorCase(f"a_sizes-{A}", an, *_one([[20, 30, 120, 140], [100, 60, 220, 200],
                                                           an[A - 1].astype(np.float64)]),
                                _check_a_size(A), seed=17))
    nf_anchors = B.copy()
    nf_anchors[100] = np.nan
    nf_boxes = np.array([[[10, 10, 60, 50], [np.nan, 10, 60, 50], [30, 20, 100, 70]],
                         [[10, 10, 60, 50], [20, 20, np.inf, 70], [0, 0, 0, 0]]], np.float64)
    nf_labels = np.array([[1, 2, 3], [4, 5, -1]], np.float64)
    cases.append(AnchorCase("nonfinite", nf_anchors, nf_boxes, nf_labels, _check_nonfinite, seed=18))
    for n_sample, pos_ratio in SAMPLING:
        cases.append(AnchorCase(f"sampling-{n_sample}-{pos_ratio}", *ties, _check_sampling(n_sample, pos_ratio),
                                seed=19, n_sample=n_sample, pos_ratio=pos_ratio, pos_iou_thresh=0.3,
                                neg_iou_thresh=0.1))
    return cases


# ----------------------------------------------------- ProposalTarget's cases
def _rand_rois(r, n, img):
    lo = r.uniform(0, img - 100, (n, 2))
    return np.concatenate([lo, lo + r.uniform(8, 300, (n, 2))], 1).clip(0, img).astype(np.float32)


T_EDGES_TOTAL = [20, 1023, 1024, 1025, 2048, 2049]


def _check_t_edges(case, out):
    assert case.rois.shape == (6, 2100, 4) and case.boxes.shape == (6, 32, 4)
    assert ((case.labels != -1).sum(axis=1) == 20).all()
    assert (case.rcount + 20).tolist() == T_EDGES_TOTAL
    for i in range(6):
        assert not np.isfinite(case.rois[i, case.rcount[i]:]).all() or case.rois[i, case.rcount[i]:].max() > 1e29
        iou = _pt_ious(case, i)
        mx = iou.max(axis=1)
        T = len(mx)
        if T > 1024:   # both lists continue past the kernel's first 1,024-row round
            assert (mx[1024:] >= 0.5).any() and (mx[:1024] >= 0.5).any() and (mx[:1024] < 0.5).any()
            assert T < 2048 or (mx[1024:] < 0.5).any()
            roi_all = np.concatenate([case.image(i)[0].astype(np.float64), case.image(i)[1]])
            late = {tuple(b) for b in roi_all[1024:]}
            s = out["images"][i]["roi"]
            if T >= 2048:
                assert any(tuple(b) in late for b in s), "a sample from a later round"
        assert len(out["images"][i]["roi"]) == min(128, T)


def _check_dup_gt_labels(case, out):
    roi, gt, gl = case.image(0)
    assert np.array_equal(gt[0], gt[1]) and gl[0] != gl[1]
    assert np.array_equal(roi[0], gt[0]) and roi[1].tolist() == [0, 5, 0, 40] and np.array_equal(roi[2], gt[2])
    iou = _pt_ious(case, 0)
    with np.errstate(all="ignore"):
        mx = iou.max(axis=1)
    nan_rows = np.nonzero(np.isnan(mx))[0]
    assert 2 in nan_rows and len(roi) + 2 in nan_rows, "0/0 for the zero-area RoI and gt"
    im = out["images"][0]
    T = len(mx)
    assert case.kw["n_sample"] >= T and len(im["roi"]) == T - len(nan_rows), "a NaN row is in neither list"
    assert not any(np.array_equal(b, gt[2]) for b in im["roi"])
    hit = [k for k, b in enumerate(im["roi"]) if np.array_equal(b, gt[0])]
    assert len(hit) == 3 and all(im["label"][k] == gl[0] for k in hit), "the lower gt index's label"


def _check_thresholds(pos, hi, lo):
    def check(case, out):
        for i in range(len(case.boxes)):
            roi, gt, _ = case.image(i)
            assert roi[0].tolist() == [0, 0, 10, 10] and gt[0].tolist() == [0, 0, 10, 5]
            mx = _pt_ious(case, i).max(axis=1)
            assert mx[0] == 0.5
            is_pos, is_neg = mx >= pos, (mx < hi) & (mx >= lo)
            im = out["images"][i]
            n_pos = int((im["label"] != 0).sum())
            assert is_pos.sum() > 3 and is_neg.sum() > 128 - n_pos and (~is_pos & ~is_neg).any()
            assert n_pos == min(64, is_pos.sum()) and len(im["roi"]) == 128
            allowed = {tuple(b) for b in np.concatenate([roi.astype(np.float64), gt])[is_pos | is_neg]}
            assert all(tuple(b) in allowed for b in im["roi"])
            if pos == 0.5:   # == pos_iou_thresh: a positive, never a negative
                assert is_pos[0] and not is_neg[0]
                assert not any(b.tolist() == [0, 0, 10, 10] for b in im["roi"][n_pos:])
            else:
                assert not is_pos[0] and not is_neg[0]
                assert not any(b.tolist() == [0, 0, 10, 10] for b in im["roi"])
    return check


ROUNDING = [(5, .5, 2), (7, .5, 4), (1, .5, 0), (128, .25, 32), (4, 0.0, 0), (4, 1.0, 4)]


def _check_rounding(n_sample, pos_ratio, want):
    def check(case, out):
        assert np.round(n_sample * pos_ratio) == want, "np.round: half to even"
        for i in range(len(case.boxes)):
            mx = _pt_ious(case, i).max(axis=1)
            P, Q = int((mx >= 0.5).sum()), int((mx < 0.5).sum())
            im = out["images"][i]
            n_pos = min(want, P)
            assert (im["label"] != 0).sum() == n_pos and len(im["roi"]) == n_pos + min(n_sample - n_pos, Q)
            assert P >= 4 and Q > 128
    return check


def proposal_cases():
    cases = []
    r = np.random.default_rng(21)
    img = 600
    rois = np.stack([_rand_rois(r, 2100, img) for _ in range(6)])
    rcount = np.array(T_EDGES_TOTAL) - 20
    for i in range(6):
        rois[i, rcount[i]::2] = np.nan
        rois[i, rcount[i] + 1::2] = 1e30
    boxes = np.zeros((6, 32, 4))
    labels = np.full((6, 32), -1.0)
    for i in range(6):
        boxes[i, :20] = _int_boxes(r, 20, img, img, lo=40)
        labels[i, :20] = r.integers(1, 21, 20)
    cases.append(ProposalCase("t_edges", rois, rcount, boxes, labels, _check_t_edges, seed=31))

    gt = np.array([[10, 10, 50, 60], [10, 10, 50, 60], [20, 30, 20, 70], [100, 100, 180, 160]], np.float64)
    rr = np.concatenate([np.array([[10, 10, 50, 60], [0, 5, 0, 40], [20, 30, 20, 70]], np.float32),
                         _rand_rois(r, 9, 200)])
    cases.append(ProposalCase("dup_gt_labels", rr[None], np.array([12]), gt[None], np.array([[3., 7., 5., 2.]]),
                              _check_dup_gt_labels, seed=32, n_sample=32))

    rois = np.stack([_rand_rois(r, 300, img) for _ in range(2)])
    rois[:, 0] = [0, 0, 10, 10]
    boxes = np.zeros((2, 8, 4))
    labels = np.full((2, 8), -1.0)
    for i, nv in enumerate((8, 5)):
        boxes[i, :nv] = _int_boxes(r, nv, img, img, lo=60)
        boxes[i, 0] = [0, 0, 10, 5]
        labels[i, :nv] = r.integers(1, 21, nv)
        # a few RoIs close to a gt, so that there are positives besides the gt rows
        rois[i, 1:9] = (boxes[i, 1 + np.arange(8) % (nv - 1)] + r.integers(-6, 7, (8, 4))).clip(0, img)
    rcount = np.array([300, 300])
    for pos, hi, lo in [(.5, .5, .1), (.6, .4, 0.0)]:
        cases.append(ProposalCase(f"thresholds-{pos}-{hi}-{lo}", rois, rcount, boxes, labels,
                                  _check_thresholds(pos, hi, lo), seed=33, pos_iou_thresh=pos,
                                  neg_iou_thresh_high=hi, neg_iou_thresh_low=lo))
    for n_sample, pos_ratio, want in ROUNDING:
        cases.append(ProposalCase(f"rounding-{n_sample}-{pos_ratio}", rois, rcount, boxes, labels,
                                  _check_rounding(n_sample, pos_ratio, want), seed=34, n_sample=n_sample,
                                  pos_ratio=pos_ratio))
    cases.append(ProposalCase("rounding-128-0.25-norm", rois, rcount, boxes, labels, _check_rounding(128, .25, 32),
                              seed=34, norm=((0.1, -0.2, 0.05, 0), (0.3, 0.1, 0.7, 0.2)), n_sample=128,
                              pos_ratio=.25))
    return cases


ANCHOR_CASES = anchor_cases()
PROPOSAL_CASES = proposal_cases()
ALL_CASES = ANCHOR_CASES + PROPOSAL_CASES
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)
