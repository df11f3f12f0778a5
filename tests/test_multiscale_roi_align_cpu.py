"""Multi-scale RoIAlign without a GPU: the level thresholds of ``ops`` against the LevelMapper
formula evaluated here, the contract's edge sizes, the restatement at one level, and the
wrapper's refusals (DESIGN.md §3 "Multi-scale RoIAlign")."""
import ctypes

import numpy as np
import pytest
import torch

import multiscale_roi_align_ref as mref
import roi_align_ref as ref
from replication_faster_rcnn_amd import _lib, ops

F = np.float32
# (k_min, k_max, canonical_scale, canonical_level)
MAPPERS = [(2, 5, 224, 4), (3, 7, 224, 4), (2, 5, 56, 4), (2, 6, 300, 3)]
IDS = [f"k{a}-{b}-s{c}-l{d}" for a, b, c, d in MAPPERS]


def count(s, thr):
    return (np.asarray(s, F)[:, None] >= np.asarray(thr, F)[None, :]).sum(1)


@pytest.mark.parametrize("k_min,k_max,s0,lvl0", MAPPERS, ids=IDS)
def test_thresholds_agree_with_the_formula(k_min, k_max, s0, lvl0):
    thr = np.array(ops.level_thresholds(k_min, k_max, s0, lvl0), F)
    assert len(thr) == k_max - k_min and (np.diff(thr) > 0).all() and thr[0] > 0
    assert np.array_equal(thr.view(np.uint32), mref.thresholds(k_min, k_max, s0, lvl0).view(np.uint32))
    # +-1,000 bit patterns around each threshold
    for t in thr:
        b = int(t.view(np.uint32))
        s = np.arange(b - 1000, b + 1001, dtype=np.uint32).view(F)
        assert np.array_equal(count(s, thr), mref.formula(s, k_min, k_max, s0, lvl0))
    # 10^6 random positive floats: log-uniform over the sizes images have, and any bit pattern
    r = np.random.default_rng(k_min * 100 + k_max)
    for s in (np.exp(r.uniform(np.log(0.01), np.log(1e5), 500_000)).astype(F),
              r.integers(1, 0x7F800000, 500_000, dtype=np.uint32).view(F)):
        assert np.array_equal(count(s, thr), mref.formula(s, k_min, k_max, s0, lvl0))
    # torch's evaluation, which ops derives the thresholds from, says the same
    s = np.concatenate([np.arange(int(t.view(np.uint32)) - 1000, int(t.view(np.uint32)) + 1001, dtype=np.uint32)
                        for t in thr]).view(F)
    assert np.array_equal(ops.level_formula(torch.from_numpy(s), k_min, k_max, s0, lvl0).numpy(), count(s, thr))


def test_edge_sizes_map_as_the_contract_says():
    thr = np.array(ops.level_thresholds(2, 5), F)
    s = np.array([0.0, np.inf, thr[0], mref.ulp_step(thr[0], -1), thr[-1], mref.ulp_step(thr[-1], -1)], F)
    assert count(s, thr).tolist() == [0, 3, 1, 0, 3, 2]
    assert np.array_equal(count(s, thr), mref.formula(s, 2, 5))
    #            zero area        negative area    both extents negative   NaN coordinate        inf extent
    rois = np.array([[0, 5, 5, 5, 90], [0, 9, 9, 300, 2], [0, 300, 300, 0, 0], [0, np.nan, 0, 9, 9], [0, 0, 0, np.inf, 9],
                     [0, 0, 0, 500, 500]], F)
    assert np.isnan(mref.root_area(rois)[[1, 3]]).all()
    want = [0, 0, 2, 0, 3, 3]
    assert mref.levels(rois, 2, 5).tolist() == want and mref.levels_by_count(rois, thr).tolist() == want
    for t in thr:     # a box can be put on either side of every threshold
        for d in (-1, 0, 1):
            v = mref.ulp_step(t, d)
            assert mref.root_area(np.concatenate([[0], mref.box_with_root(v)]))[0] == v


def test_one_level_is_roi_align():
    case = ref.CASES[3]
    x, rois, grad = case.inputs()
    lv = mref.levels(rois, 4, 4)
    assert not lv.any() and len(mref.thresholds(4, 4)) == 0
    args = (case.sampling_ratio, case.aligned)
    out = mref.forward([x], rois, case.size, [0.0625], *args, lv)
    assert ref.same_bits(out, ref.forward(x, rois, case.size, 0.0625, *args))
    (gi,) = mref.backward(grad, rois, [x.shape], [0.0625], *args, lv)
    assert ref.same_bits(gi, ref.backward(grad, rois, x.shape, 0.0625, *args))


def test_restatement_places_rois_by_level():
    """Two levels, RoIs of both in mixed order: each output row is the single-map result of
    its level, and each map's gradient sums its own RoIs only."""
    r = np.random.default_rng(2)
    xs = [r.standard_normal((1, 3, 8, 8)).astype(F), r.standard_normal((1, 3, 4, 4)).astype(F)]
    rois = np.array([[0, 1, 1, 9, 9], [0, 0, 0, 30, 30], [0, 2, 3, 8, 12], [0, 4, 4, 28, 20]], F)
    thr = mref.thresholds(1, 2, 8, 1)             # the levels change at sqrt(area) ~ 16
    lv = mref.levels(rois, 1, 2, 8, 1)
    assert lv.tolist() == [0, 1, 0, 1] and mref.levels_by_count(rois, thr).tolist() == lv.tolist()
    out = mref.forward(xs, rois, 2, [0.5, 0.25], 2, False, lv)
    assert ref.same_bits(out[[1, 3]], ref.forward(xs[1], rois[[1, 3]], 2, 0.25, 2, False))
    g = r.standard_normal(out.shape).astype(F)
    gis = mref.backward(g, rois, [x.shape for x in xs], [0.5, 0.25], 2, False, lv)
    assert ref.same_bits(gis[0], ref.backward(g[[0, 2]], rois[[0, 2]], xs[0].shape, 0.5, 2, False))


def test_wrapper_refuses_before_any_launch():
    def maps(n, C=4, N=2, dtype=torch.float32, first=64):
        return [torch.zeros(N, C, max(first >> l, 1), max(first >> l, 1), dtype=dtype) for l in range(n)]

    boxes = torch.tensor([[0, 1.0, 1.0, 9.0, 9.0]])
    scales = [2.0 ** -(2 + l) for l in range(9)]
    with pytest.raises(RuntimeError, match="at most 8"):
        ops.multiscale_roi_align(maps(9), boxes, 7, scales, 2)
    for bad in (maps(2)[:1] + maps(2, C=5)[1:], maps(2)[:1] + maps(2, N=3)[1:],
                maps(2)[:1] + maps(2, dtype=torch.float16)[1:]):
        with pytest.raises(RuntimeError, match="share N, C and dtype"):
            ops.multiscale_roi_align(bad, boxes, 7, scales[:2], 2)
    with pytest.raises(RuntimeError, match="span"):           # 1/4 .. 1/16 is three octaves, two maps given
        ops.multiscale_roi_align(maps(2), boxes, 7, [0.25, 0.0625], 2)
    with pytest.raises(RuntimeError, match="spatial_scales"):
        ops.multiscale_roi_align(maps(3), boxes, 7, scales[:2], 2)
    with pytest.raises(RuntimeError):
        ops.multiscale_roi_align([], boxes, 7, [], 2)
    with pytest.raises(RuntimeError):
        ops.multiscale_roi_align([torch.zeros(4, 8, 8)] * 2, boxes, 7, scales[:2], 2)
    pool = ops.MultiScaleRoIAlign(["a", "b"], 7, 2)
    with pytest.raises(RuntimeError, match="two axes"):
        pool.infer_scales([torch.zeros(1, 1, 64, 32)], [(256, 256)])
    assert pool.infer_scales(maps(2, first=150) + [torch.zeros(1, 1, 38, 38)], [(600, 590), (580, 600)]) == (
        0.25, 0.125, 0.0625)


def test_capi_refuses_before_any_launch():
    lib = _lib.load(require_gpu=False)
    H = (_lib.I32 * 9)(*[8] * 9)
    sc = (_lib.F32 * 9)(*[0.25] * 9)
    ptrs = (_lib.P * 9)(*[0] * 9)

    def call(n, thr, fn=lib.frcnn_roi_align_multi_fwd_t, sr=2, dtype=0):
        t = (_lib.F32 * 8)(*thr, *([0.0] * (8 - len(thr))))
        if fn is lib.frcnn_roi_align_multi_fwd_t:
            return fn(dtype, n, ptrs, H, H, sc, t, None, 3, 1, 4, 7, 7, sr, 0, None, None, None, 0, None)
        return fn(dtype, n, None, H, H, sc, t, None, 3, 1, 4, 7, 7, sr, 0, ptrs, None, 0, None)

    for fn in (lib.frcnn_roi_align_multi_fwd_t, lib.frcnn_roi_align_multi_bwd_t):
        for n in (0, 9, -1):
            assert call(n, [1, 2], fn) == -1 and b"n_levels" in lib.frcnn_last_error()
        assert call(3, [2, 1], fn) == -1 and b"thresholds[1]" in lib.frcnn_last_error()
        assert call(3, [1, float("nan")], fn) == -1 and b"NaN" in lib.frcnn_last_error()
        assert call(2, [float("nan")], fn) == -1 and b"NaN" in lib.frcnn_last_error()
        assert call(3, [1, 2], fn, sr=17) == -1 and b"sampling_ratio" in lib.frcnn_last_error()
        assert call(3, [1, 2], fn, dtype=3) == -1 and b"dtype" in lib.frcnn_last_error()
    buf = ctypes.create_string_buffer(160)
    assert lib.frcnn_roi_align_multi_fwd_kernel(0, 9, 1, 1, 1, 7, 7, 2, buf, 160) == -1
    assert _lib.roi_align_multi_kernel("fwd", 4, 10, 2, 8, dtype=torch.float16) == mref.fwd_name("f16")
    assert _lib.roi_align_multi_kernel("bwd", 4, 10, 2, 8, dtype=torch.bfloat16) == mref.bwd_name("bf16")
