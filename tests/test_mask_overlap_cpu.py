"""The restatement of ops.mask_overlap (tests/coco_segm_ref.py) against a second, independent
form -- a run-length walk of the column-major RLE, as maskApi.c's rleIou does it -- and against
the step-by-step model of the two kernels (tests/mask_overlap_model.py); then the model with
each named mistake planted: the case named for the mistake must tell it from the contract.
No GPU: the plan comes from the built library's host-only query."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import coco_segm_ref as ref  # noqa: E402
import mask_overlap_cases as mc  # noqa: E402
import mask_overlap_model as model  # noqa: E402
from replication_faster_rcnn_amd import _lib  # noqa: E402

_cache = {}


def built(name):
    """(case, restatement's (inter, det_area, gt_area)): made once, never modified."""
    if name not in _cache:
        c = mc.CASES[name]()
        _cache[name] = (c, ref.overlap(c["det_masks"], c["gt_masks"], c["det_labels"], c["det_count"],
                                       c["gt_labels"], c["n_class"]))
    return _cache[name]


def run_model(c, mistake=None):
    return model.overlap(c["det_masks"], c["gt_masks"], c["det_labels"], c["det_count"], c["gt_labels"],
                         c["n_class"], mistake)


# ------------------------------------------------------- the second form: RLE
rle, rle_walk = ref.rle, ref.rle_walk


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_restatement_equals_the_rle_walk(name):
    c, (inter, da, ga) = built(name)
    N, D = c["det_masks"].shape[:2]
    G = c["gt_masks"].shape[1]
    for n in range(N):
        k = D if c["det_count"] is None else int(np.clip(c["det_count"][n], 0, D))
        ok = ref.considered(D, G, None if c["det_labels"] is None else c["det_labels"][n], k,
                            None if c["gt_labels"] is None else c["gt_labels"][n], c["n_class"])
        gr = [rle(c["gt_masks"][n, g]) for g in range(G)]
        assert [int(r[1::2].sum()) for r in gr] == ga[n].tolist()
        for d in range(D):
            if d >= k:
                assert da[n, d] == 0 and not inter[n, d].any()
                continue
            dr = rle(c["det_masks"][n, d])
            assert int(dr[1::2].sum()) == da[n, d]
            gs = np.nonzero(ok[d])[0][:8]                     # eight considered pairs per detection
            assert [rle_walk(dr, gr[g]) for g in gs] == inter[n, d, gs].tolist()
            assert not inter[n, d, ~ok[d]].any()


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_closed_forms_hold_on_the_restatement(name):
    c, got = built(name)
    out = dict(zip(("inter", "det_area", "gt_area"), got))
    for (which, idx), v in c["expect"].items():
        assert out[which][idx] == v, (which, idx, out[which][idx], v)


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_plan_and_model_equal_the_restatement(name):
    c, want = built(name)
    N, D, H, W = c["det_masks"].shape
    G = c["gt_masks"].shape[1]
    plan = _lib.mask_overlap_plan(N, D, G, H, W)
    assert plan == model.plan(N, D, G, H, W)
    for k, v in c["plan"].items():
        assert plan[k] == v, (k, plan[k], v)
    assert plan["workspace"] == _lib.load(require_gpu=False).frcnn_mask_overlap_workspace_size(N, D, G, H, W)
    inter, da, ga, cells = run_model(c)
    assert np.array_equal(inter, want[0]) and np.array_equal(da, want[1]) and np.array_equal(ga, want[2])
    for idx, reads in c["cells"].items():
        assert (cells[idx] > 0) == reads, (idx, cells[idx])


def test_junk_beyond_the_count_reaches_no_output():
    c, want = built("count_below_d_junk")
    z = mc.junk_zeroed(c)
    assert not np.array_equal(z["det_masks"], c["det_masks"])
    for a, b in zip(run_model(c)[:3], run_model(z)[:3]):
        assert np.array_equal(a, b)
    assert all(np.array_equal(a, b) for a, b in zip(want, ref.overlap(z["det_masks"], z["gt_masks"], None,
                                                                      z["det_count"])))


@pytest.mark.parametrize("mistake,names", [
    ("past_w", ["first_last_bytes"]),
    ("last_word", ["one_word_overlap", "col63_both"]),
    ("and1", ["byte_values"]),
    ("alignment", ["w600", "w37_every_alignment"]),
    ("beyond", ["count_below_d_junk"]),
])
def test_planted_mistake_is_told_apart_by_its_case(mistake, names):
    assert mistake in model.MISTAKES
    for name in names:
        c, want = built(name)
        got = run_model(c, mistake)[:3]
        assert not all(np.array_equal(a, b) for a, b in zip(got, want)), (mistake, name)
        out = dict(zip(("inter", "det_area", "gt_area"), got))
        if c["expect"]:                                       # and a closed form of the case names it
            assert any(out[w][i] != v for (w, i), v in c["expect"].items()), (mistake, name)


def test_argument_limits_on_the_host():
    lib = _lib.load(require_gpu=False)
    assert lib.frcnn_mask_overlap_workspace_size(1, 1, 0, 1, 1) > 0
    for bad in [(0, 1, 1, 8, 8), (1025, 1, 1, 8, 8), (1, 0, 1, 8, 8), (1, 1025, 1, 8, 8), (1, 1, 257, 8, 8),
                (1, 1, -1, 8, 8), (1, 1, 1, 0, 8), (1, 1, 1, 8, 4097), (1, 1, 1, 4097, 8), (1, 1, 1, 4096, 4097)]:
        assert lib.frcnn_mask_overlap_workspace_size(*bad) == 0, bad
        with pytest.raises(_lib.FrcnnError):
            _lib.mask_overlap_plan(*bad)
    assert _lib.mask_overlap_plan(1024, 1024, 256, 4096, 4096)["words"] == 64
