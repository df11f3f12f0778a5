"""Named cases of the segm matching (DESIGN.md "COCO segm evaluation"), on canvases of at most
16 x 16 (one of 96 x 96 for the detection-area edges).

CASES: name -> builder of dict(batches: [coco_segm_ref case], C, cap or None).
CHECKS: name -> check(st, overlaps, want): the case's precondition and its closed form, asserted
on the restatement's state alone (coco_segm_ref.State; want = its accumulate()).
"""
import numpy as np

import coco_eval_ref as cref
import coco_segm_ref as ref

CASES, CHECKS = {}, {}
S = 16
EMPTY = []


def case(name, C=2, cap=None):
    def deco(f):
        CASES[name] = lambda: dict(batches=f(), C=C, cap=cap)
        return f
    return deco


def check(name):
    def deco(f):
        CHECKS[name] = f
        return f
    return deco


def masks(st, i):
    m, ig, rank = cref.unpack_bits(st.rec_bits[i:i + 1])
    return m[0], ig[0], int(rank[0])


def iou_of(ov, n, d, g, crowd=False):
    inter, da, ga = ov
    return float(ref.iou_from_counts(inter[n, d, g:g + 1], da[n, d], ga[n, g:g + 1], np.array([crowd]))[0])


# ------------------------------------------------------------------ thresholds
@case("at_threshold")
def _():
    row = lambda x0, x1: [(0, x0, 1, x1)]                                      # noqa: E731
    return [ref.images(S, S,
                       ([(row(0, 3), 1, 0.5)], [(row(1, 4), 1, 0)]),           # i = 2, areas 3 and 3: 2 / 4
                       ([(row(0, 3), 1, 0.5)], [(row(0, 4), 1, 0)]),           # i = 3, u = 4: 0.75
                       ([(row(0, 4), 1, 0.5)], [(row(1, 5), 1, 0)]))]          # i = 3, u = 5: 3 / 5 against T[2]


@check("at_threshold")
def _(st, ovs, want):
    ov = ovs[0]
    assert ov[0][:, 0, 0].tolist() == [2, 3, 3] and ov[1][:, 0].tolist() == [3, 3, 4]
    assert iou_of(ov, 0, 0, 0) == 0.5 == cref.T[0] and iou_of(ov, 1, 0, 0) == 0.75 == cref.T[5]
    assert masks(st, 0)[0][0].tolist() == [t <= 0 for t in range(10)]
    assert masks(st, 1)[0][0].tolist() == [t <= 5 for t in range(10)]
    v = iou_of(ov, 2, 0, 0)
    assert v == 3.0 / 5.0 and abs(v - cref.T[2]) < 1e-15
    assert masks(st, 2)[0][0].tolist() == [bool(v >= cref.T[t]) for t in range(10)]     # whichever side T[2] is on


@case("zero_intersection")
def _():
    yy, xx = np.mgrid[0:S, 0:S]
    even, odd = (yy + xx) % 2 == 0, (yy + xx) % 2 == 1                          # the same box, no common pixel
    return [ref.images(S, S, ([(even, 1, 0.9)], [(odd, 1, 0), (odd, 1, 1)]))]


@check("zero_intersection")
def _(st, ovs, want):
    assert ovs[0][0][0, 0].tolist() == [0, 0] and ovs[0][1][0, 0] == 128
    m, ig, _ = masks(st, 0)
    assert not m.any() and ig[:, 0].tolist() == [False, False, True, True]     # 128 pixels: small
    assert st.npig[1].tolist() == [1, 1, 0, 0]


# ---------------------------------------------------------------------- crowds
@case("crowd")
def _():
    crowd = [(0, 0, 12, 12)]
    dets = [([(1, 1, 3, 3)], 1, 0.9), ([(4, 4, 7, 7)], 1, 0.8), ([(8, 8, 12, 12)], 1, 0.7),
            ([(13, 13, 16, 16)], 1, 0.6)]
    return [ref.images(S, S, (dets, [(crowd, 1, 1), ([(14, 0, 16, 2)], 1, 0)]))]


@check("crowd")
def _(st, ovs, want):
    ov = ovs[0]
    assert iou_of(ov, 0, 0, 0, True) == 1 and iou_of(ov, 0, 0, 0, False) < 0.5
    for i in range(3):
        m, ig, _ = masks(st, i)
        assert m[0].all() and ig[0].all()               # i / a_d = 1: matched at 0.95 too, ignored
    m, ig, _ = masks(st, 3)
    assert not m.any() and not ig[0].any()              # the one FP
    assert st.npig[1, 0] == 1


@case("regular_over_crowd")
def _():
    det, reg = [(0, 0, 4, 4)], [(0, 0, 4, 5)]
    return [ref.images(S, S, ([(det, 1, 0.9)], [(det, 1, 1), (reg, 1, 0)]))]


@check("regular_over_crowd")
def _(st, ovs, want):
    assert iou_of(ovs[0], 0, 0, 0, True) == 1 and iou_of(ovs[0], 0, 0, 1) == 0.8
    m, ig, _ = masks(st, 0)
    _, dtg = st.matched_gt[0][(1, 0)]
    assert dtg[:, 0].tolist() == [1] * 7 + [0] * 3
    assert ig[0].tolist() == [False] * 7 + [True] * 3 and m[0].all()


# ------------------------------------------------------------------------ ties
@case("equal_iou_later_gt")
def _():
    a = [(2, 2, 8, 8)]
    return [ref.images(S, S, ([(a, 1, 0.9), (a, 1, 0.8)], [(a, 1, 0), (a, 1, 0), ([(10, 10, 12, 12)], 1, 0)]))]


@check("equal_iou_later_gt")
def _(st, ovs, want):
    _, dtg = st.matched_gt[0][(1, 0)]
    assert dtg[:, 0].tolist() == [1] * 10 and dtg[:, 1].tolist() == [0] * 10


@case("taken_gt")
def _():
    a, b = [(0, 0, 10, 10)], [(0, 1, 10, 11)]            # 90 / 110
    return [ref.images(S, S, ([(a, 1, 0.9), (a, 1, 0.8), (a, 1, 0.7)], [(a, 1, 0), (b, 1, 0)]))]


@check("taken_gt")
def _(st, ovs, want):
    assert 0.8 < iou_of(ovs[0], 0, 1, 1) == 90 / 110 < 0.85
    _, dtg = st.matched_gt[0][(1, 0)]
    assert dtg[0].tolist() == [0, 1, -1] and dtg[7].tolist() == [0, -1, -1]
    m, ig, _ = masks(st, 2)
    assert not m[0].any() and not ig[0].any()


# ----------------------------------------------------------------------- areas
@case("gt_area_field")
def _():
    a = [(0, 0, 10, 10)]                                 # 100 pixels; the annotation of image 1 says 2,000
    return [ref.images(S, S, ([(a, 1, 0.9)], [(a, 1, 0, 100.0)]), ([(a, 1, 0.9)], [(a, 1, 0, 2000.0)]))]


@check("gt_area_field")
def _(st, ovs, want):
    assert ovs[0][2][:, 0].tolist() == [100, 100] and iou_of(ovs[0], 0, 0, 0) == iou_of(ovs[0], 1, 0, 0) == 1
    assert st.npig[1].tolist() == [2, 1, 1, 0]
    for i in range(2):
        m, ig, _ = masks(st, i)
        assert m.all()                                   # the IoU is 1 whatever the field says
        assert ig[:, 0].tolist() == [False, i == 1, i == 0, True]


@case("det_area_edges", C=3)
def _():
    H = 96
    return [ref.images(H, H, ([([(0, 0, 32, 32)], 1, 0.9)], [([(90, 90, 96, 96)], 1, 0)]),
                       ([([(0, 0, 96, 96)], 2, 0.9)], [([(0, 0, 2, 2)], 1, 0)]))]


@check("det_area_edges")
def _(st, ovs, want):
    assert ovs[0][1][:, 0].tolist() == [1024, 9216]
    m, ig, _ = masks(st, 0)
    assert not m.any() and ig[:, 0].tolist() == [False, False, False, True]    # 1,024: small and medium
    m, ig, _ = masks(st, 1)
    assert not m.any() and ig[:, 0].tolist() == [False, True, False, False]    # 9,216: medium and large


@case("empty_det")
def _():
    return [ref.images(S, S, ([(EMPTY, 1, 0.9)], [([(0, 0, 4, 4)], 1, 1), ([(5, 5, 8, 8)], 1, 0)]))]


@check("empty_det")
def _(st, ovs, want):
    assert ovs[0][1][0, 0] == 0
    m, ig, _ = masks(st, 0)
    assert not m.any() and ig[:, 0].tolist() == [False, False, True, True]     # an FP in "all" and "small"


@case("empty_gt")
def _():
    a = [(0, 0, 4, 4)]
    return [ref.images(S, S, ([(a, 1, 0.9)], [(EMPTY, 1, 0), (a, 1, 0)]))]


@check("empty_gt")
def _(st, ovs, want):
    assert ovs[0][2][0].tolist() == [0, 16] and st.npig[1].tolist() == [2, 2, 0, 0]      # still a gt
    _, dtg = st.matched_gt[0][(1, 0)]
    assert (dtg[:, 0] == 1).all()
    assert want["recall"][0, 1, 0, 2] == 0.5


# ---------------------------------------------------------------------- counts
@case("d101")
def _():
    gt = [(0, 0, 8, 8)]
    det = [([(0, 0, 2 + i % 5, 2 + i // 5 % 5)], 1, 1.0 - i / 256) for i in range(100)] + [(gt, 1, 0.25)]   # <= 36 / 64
    return [ref.images(S, S, (det, [(gt, 1, 0)]))]


@check("d101")
def _(st, ovs, want):
    m, ig, rank = masks(st, 100)
    assert rank == cref.RANK_OUT and not m.any() and not ig.any()
    assert ovs[0][0][0, 100, 0] == 64                    # counted by the overlap, never ranked
    assert (want["recall"][2:, 1, 0, 2] == 0).all()     # its would-be TP at 0.6 and above does not count


def batches():
    kw = dict(D=24, G=6, H=S, W=S, C=4, seed=11, n_gt=5)
    return [ref.random_case(N=2, **kw), ref.random_case(N=3, first_image=2, **kw),
            ref.random_case(N=1, first_image=5, **kw)]


CASES["several_updates"] = lambda: dict(batches=batches(), C=4, cap=None)


@check("several_updates")
def _(st, ovs, want):
    assert st.hdr[1] == 6 and st.hdr[0] == sum(int(np.clip(c["det_count"], 0, 24).sum()) for c in batches())
    m, _, _ = cref.unpack_bits(st.rec_bits[:int(st.hdr[0])])
    assert m[:, 0, 0].any() and not m[:, 0, 0].all()


CASES["random_200"] = lambda: dict(batches=[ref.random_case(N=2, D=100, G=32, H=200, W=200, C=4, seed=7)], C=4, cap=None)


@check("random_200")
def _(st, ovs, want):
    """Not vacuous: a record matched at 0.95, one unmatched at 0.5, a crowd match and a non-crowd one."""
    c = CASES["random_200"]()["batches"][0]
    n = int(st.hdr[0])
    m, ig, rank = cref.unpack_bits(st.rec_bits[:n])
    ranked = rank < cref.KEEP
    assert (m[ranked, 0, 9]).any() and (~m[ranked, 0, 0]).any()
    crowd_hit = plain_hit = False
    for img, diag in enumerate(st.matched_gt):
        for (cls, a), (slots, dtg) in diag.items():
            if a == 0:
                g = dtg[dtg >= 0]
                crowd_hit |= bool(c["gt_crowd"][img, g].any())
                plain_hit |= bool((c["gt_crowd"][img, g] == 0).any())
    assert crowd_hit and plain_hit
    assert set(np.unique(c["gt_labels"][c["gt_labels"] > 0])) == {1, 2, 3} and c["gt_crowd"].any()
    assert (c["det_count"] == [100, 93]).all() and c["det_masks"][1, 93:].any()          # junk beyond the count
    assert c["det_masks"].max() == 255 and set(np.unique(c["det_masks"][1, :93])) == {0, 1}


def dropped_capacity():
    k = [int(np.clip(c["det_count"], 0, 24).sum()) for c in batches()]
    assert k[0] + k[2] <= k[0] + k[1] - 1
    return k[0] + k[1] - 1, k                             # the second batch does not fit, the third does


CASES["dropped_batch"] = lambda: dict(batches=batches(), C=4, cap=dropped_capacity()[0])


@check("dropped_batch")
def _(st, ovs, want):
    cap, k = dropped_capacity()
    assert st.hdr[2] == 1 and st.hdr[0] == k[0] + k[2] and st.hdr[1] == 3
