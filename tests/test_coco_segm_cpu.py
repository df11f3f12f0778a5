"""The restatement of the segm matching (tests/coco_segm_ref.py) on its named cases: each case's
precondition and closed form; the IoU from counts against a second, independent form (rleIou's
walk over the column-major RLE, the union from the run lists); the two forms of the matching
loop against each other; and the named mistakes a kernel could make in the IoU, each planted
and told apart by the case named for it.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import coco_eval_ref as cref  # noqa: E402
import coco_segm_cases as sc  # noqa: E402
import coco_segm_ref as ref  # noqa: E402

_cache = {}
rle, rle_walk = ref.rle, ref.rle_walk


def reference(name):
    """(case, state, overlaps, accumulate) of the restatement: made once, never modified."""
    if name not in _cache:
        c = sc.CASES[name]()
        st, ovs = ref.run(c["batches"], c["C"], c["cap"])
        _cache[name] = (c, st, ovs, st.accumulate())
    return _cache[name]


def records(st):
    n = int(st.hdr[0])
    return st.hdr.copy(), st.rec_key[:n].copy(), st.rec_bits[:n].copy()


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(records(a), records(b)))


def test_every_case_has_its_check():
    assert sorted(sc.CASES) == sorted(sc.CHECKS)


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_case_precondition_and_closed_form(name):
    _, st, ovs, want = reference(name)
    sc.CHECKS[name](st, ovs, want)


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_two_phase_matching_equals_the_sequential_loop(name):
    c, st, _, _ = reference(name)
    two, _ = ref.run(c["batches"], c["C"], c["cap"], match=cref.match_two_phase)
    assert same(st, two)


def rle_iou(d, g, crowd):
    """maskApi.c's rleIou of two run lists: the areas from the runs, the walk, one division."""
    i = rle_walk(d, g)
    if i == 0:
        return 0.0
    a_d, a_g = int(d[1::2].sum()), int(g[1::2].sum())
    return float(np.float64(i) / np.float64(a_d if crowd else a_d + a_g - i))


@pytest.mark.parametrize("name", sorted(set(sc.CASES) - {"random_200"}))
def test_iou_from_counts_equals_the_rle_walk(name):
    c, _, ovs, _ = reference(name)
    seen = 0
    for b, (inter, da, ga) in zip(c["batches"], ovs):
        N, D = b["det_labels"].shape
        G = b["gt_labels"].shape[1]
        for n in range(N):
            ok = ref.considered(D, G, b["det_labels"][n], b["det_count"][n], b["gt_labels"][n], c["C"])
            gr = [rle(b["gt_masks"][n, g]) for g in range(G)]
            for d, g in np.argwhere(ok):
                want = rle_iou(rle(b["det_masks"][n, d]), gr[g], bool(b["gt_crowd"][n, g]))
                got = ref.iou_from_counts(inter[n, d, g:g + 1], da[n, d], ga[n, g:g + 1],
                                          b["gt_crowd"][n, g:g + 1] != 0)[0]
                assert got == want, (n, d, g, got, want)
                seen += 1
    assert seen > 0


# ----------------------------------------------------------- planted mistakes
def union_from_gt_area(i, a_d, a_g, crowd, garea):
    return ref.iou_from_counts(i, a_d, np.asarray(garea).astype(np.int64), crowd)


def crowd_over_union(i, a_d, a_g, crowd, garea):
    return ref.iou_from_counts(i, a_d, a_g, np.zeros(len(i), bool))


def zero_divided(i, a_d, a_g, crowd, garea):
    i = np.asarray(i, np.float64)
    u = np.where(crowd, np.float64(a_d), np.float64(a_d) + np.asarray(a_g, np.float64) - i)
    with np.errstate(invalid="ignore", divide="ignore"):
        return i / u                                    # 0 / 0 against a crowd when the detection is empty


@pytest.mark.parametrize("mistake,name", [(union_from_gt_area, "gt_area_field"), (crowd_over_union, "crowd"),
                                          (zero_divided, "empty_det")])
def test_planted_iou_mistake_is_told_apart_by_its_case(mistake, name):
    c, st, _, _ = reference(name)
    wrong, _ = ref.run(c["batches"], c["C"], c["cap"], iou=mistake)
    assert not same(st, wrong), (mistake.__name__, name)
    for other in ("at_threshold", "taken_gt"):          # and it is a mistake of that case, not of all
        co, so, _, _ = reference(other)
        assert same(so, ref.run(co["batches"], co["C"], co["cap"], iou=mistake)[0])


def test_several_updates_equal_one():
    c, st, _, _ = reference("several_updates")
    one, _ = ref.run([ref.concat(c["batches"])], c["C"], st.cap)
    assert same(st, one)


def test_gt_area_field_moves_the_range_not_the_iou():
    c, st, _, _ = reference("gt_area_field")
    b = dict(c["batches"][0], gt_area=None)
    plain, _ = ref.run([b], c["C"])
    assert plain.npig[1].tolist() == [2, 2, 0, 0] and st.npig[1].tolist() == [2, 1, 1, 0]
    ma, _, _ = cref.unpack_bits(st.rec_bits[:2])
    mb, _, _ = cref.unpack_bits(plain.rec_bits[:2])
    assert np.array_equal(ma, mb)
