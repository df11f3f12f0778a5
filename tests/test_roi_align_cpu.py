"""RoIAlign without a GPU: the restatement (tests/roi_align_ref.py) against known
answers, its clipping against the plain loop, the guards, and the C-ABI's new
symbols and argument errors (DESIGN.md §3 "RoIAlign")."""
import ctypes
import os
import re

import numpy as np
import pytest

import roi_align_ref as ref

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "frcnn_capi.h")
SYMBOLS = ["frcnn_roi_align_fwd_t", "frcnn_roi_align_bwd_t", "frcnn_roi_align_fwd_workspace_size",
           "frcnn_roi_align_bwd_workspace_size", "frcnn_roi_align_fwd_kernel", "frcnn_roi_align_bwd_kernel",
           "frcnn_roi_align_plan", "frcnn_roi_align_multi_plan"]


def _ramps():
    h, w = np.arange(12, dtype=F)[:, None], np.arange(14, dtype=F)[None, :]
    x = np.zeros((1, 2, 12, 14), F)
    x[0, 0] = 2 * h + 3 * w
    x[0, 1] = -h + 5 * w
    return x


ROI = np.array([[0, 1, 2, 8, 9]], F)
PHG, PWG = np.arange(7, dtype=F)[:, None], np.arange(7, dtype=F)[None, :]


# ------------------------------------------------------------ known answers
@pytest.mark.parametrize("sampling_ratio", [2, -1])
def test_linear_planes_are_reproduced_exactly(sampling_ratio):
    """Bilinear samples of a linear plane average to the plane at the bin's centre; every
    quantity here is a small dyadic rational, so fp32 is exact."""
    out = ref.forward(_ramps(), ROI, 7, 1.0, sampling_ratio, False)
    assert np.array_equal(out[0, 0], 2 * (F(2.5) + PHG) + 3 * (F(1.5) + PWG))
    assert np.array_equal(out[0, 1], -(F(2.5) + PHG) + 5 * (F(1.5) + PWG))


def test_aligned_shifts_by_half_a_pixel():
    out = ref.forward(_ramps(), ROI, 7, 1.0, 2, True)
    assert np.array_equal(out[0, 0], 2 * (F(2) + PHG) + 3 * (F(1) + PWG))
    assert np.array_equal(out[0, 1], -(F(2) + PHG) + 5 * (F(1) + PWG))


def test_backward_of_ones_sums_to_the_bin_count():
    gi = ref.backward(np.ones((1, 2, 7, 7), F), ROI, (1, 2, 12, 14), 1.0, 2, False)
    assert gi.dtype == F and gi.reshape(2, -1).sum(1, dtype=np.float64).tolist() == [49.0, 49.0]
    assert (gi[0, :, :2] == 0).all() and (gi[0, :, :, 10:] == 0).all()


def test_the_order_of_rois_is_observable():
    """A backward that sums in another order fails a bit comparison."""
    r = np.random.default_rng(5)
    rois = ref.special_rois()
    g = r.standard_normal((len(rois), 16, 7, 7)).astype(F)
    a = ref.backward(g, rois, (2, 16, 12, 14), 1.0, 2, False)
    b = ref.backward(g[::-1], rois[::-1], (2, 16, 12, 14), 1.0, 2, False)
    assert np.allclose(a, b, rtol=1e-4, atol=1e-5)
    assert (ref.bits(a) != ref.bits(b)).sum() > 1000


# ----------------------------------------------------------------- clipping
@pytest.mark.parametrize("aligned", [False, True])
def test_clipped_samples_equal_the_plain_loop(aligned):
    """Adaptive grids far above SCAN points per bin (boxes up to ~300 px over a 12x14 map):
    bisecting the sample indices loses no inside sample, forward or backward."""
    r = np.random.default_rng(31)
    x = r.standard_normal((2, 3, 12, 14)).astype(F)
    rows = [[0, -150, -140, 150, 160], [1, -290, 3, 9, 7], [0, 5, -280, 9, 20], [1, 2, 2, 300, 290],
            [0, 13.2, 11.1, 200, 180], [1, -200, -200, -0.4, -0.4], [0, -130, -130, -2, -2], [1, 14.5, 0, 260, 12]]
    rows += [[b, *r.uniform(-150, 10, 2), *r.uniform(4, 160, 2)] for b in (0, 1) for _ in range(4)]
    rois = np.array(rows, F)
    g = ref.geometry(rois[0], 2, 7, 7, 1.0, -1, aligned)
    assert g.gh > 2 * ref.SCAN and g.gw > 2 * ref.SCAN
    visited = sum(len(ref.sample_range(g.sh + F(p) * g.bh, g.bh, g.gh, -1, 12, True)) for p in range(7))
    assert 0 < visited <= 12 + 2 + 7 < 7 * g.gh, "work per bin is bounded by the map"
    a = ref.forward(x, rois, 7, 1.0, -1, aligned, clip=True)
    b = ref.forward(x, rois, 7, 1.0, -1, aligned, clip=False)
    assert np.array_equal(ref.bits(a), ref.bits(b)) and np.abs(a).sum() > 0
    grad = r.standard_normal((len(rois), 3, 7, 7)).astype(F)
    ga = ref.backward(grad, rois, x.shape, 1.0, -1, aligned, clip=True)
    gb = ref.backward(grad, rois, x.shape, 1.0, -1, aligned, clip=False)
    assert np.array_equal(ref.bits(ga), ref.bits(gb)) and np.abs(ga).sum() > 0


# ------------------------------------------------------------------- guards
def test_guarded_rois_give_zeros_and_no_gradient():
    r = np.random.default_rng(2)
    x = r.standard_normal((2, 3, 12, 14)).astype(F)
    bad = np.array([[-1, 1, 1, 5, 5], [2, 1, 1, 5, 5], [np.nan, 1, 1, 5, 5], [0, 3e6, 1, 5, 5], [0, 1, -3e6, 5, 5],
                    [1, 1, 1, np.inf, 5], [1, 1, 1, 5, np.nan], [0, 1, 1, 5, -np.inf]], F)
    out = ref.forward(x, bad, 7, 1.0, 2, False)
    assert not out.any() and not np.signbit(out).any()
    gi = ref.backward(np.ones_like(out), bad, x.shape, 1.0, 2, False)
    assert not gi.any()
    assert ref.geometry([0, 2 ** 20, 0, 1, 1], 2, 7, 7, 1.0, 2, False) is not None      # the limit itself is inside
    assert ref.geometry([0, 2 ** 20, 0, 1, 1], 2, 7, 7, 1.0001, 2, False) is None       # the scaled value counts
    assert ref.geometry([-0.5, 0, 0, 1, 1], 2, 7, 7, 1.0, 2, False).b == 0              # truncation toward zero


# -------------------------------------------------------------------- C-ABI
def test_header_declares_and_library_exports_roi_align():
    from replication_faster_rcnn_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s


def _call(lib, which, dtype=0, x=1, rois=1, R=1, PH=7, PW=7, sr=2, out=1):
    """One entry point with dummy non-null pointers: only argument errors may come back."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    fn = lib.frcnn_roi_align_fwd_t if which == "fwd" else lib.frcnn_roi_align_bwd_t
    return fn(dtype, p if x else None, p if rois else None, R, 1, 1, 4, 4, PH, PW, 1.0, sr, 0, p if out else None,
              None, 0, None)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_argument_errors_come_before_any_hip_call(which):
    from replication_faster_rcnn_amd import _lib
    lib = _lib.load(require_gpu=False)
    for kw, word in [(dict(PH=0), b"output_size"), (dict(PW=-3), b"output_size"), (dict(sr=17), b"sampling_ratio"),
                     (dict(dtype=3), b"dtype"), (dict(dtype=-1), b"dtype"), (dict(rois=0), b"rois"),
                     (dict(out=0), b"grad_in" if which == "bwd" else b"out"),
                     (dict(x=0), b"grad" if which == "bwd" else b"null x")]:
        assert _call(lib, which, **kw) == -1, kw
        assert word in lib.frcnn_last_error(), (kw, lib.frcnn_last_error())
    assert lib.frcnn_roi_align_fwd_t(0, None, None, 0, 1, 1, 4, 4, 7, 7, 1.0, -1, 0, None, None, 0, None) == 0   # R == 0
    assert lib.frcnn_roi_align_fwd_workspace_size(8, 2, 4) > 0 and lib.frcnn_roi_align_bwd_workspace_size(8, 2, 7, 7) > 0


def test_kernel_names_without_a_gpu():
    import torch
    from replication_faster_rcnn_amd import _lib
    for key, dt in (("f32", torch.float32), ("f16", torch.float16), ("bf16", torch.bfloat16)):
        assert _lib.roi_align_kernel("fwd", 16, 2, 16, 12, 14, dtype=dt) == ref.fwd_name(key)
        assert _lib.roi_align_kernel("bwd", 16, 2, 16, 12, 14, dtype=dt) == ref.bwd_name(key)
    with pytest.raises(RuntimeError, match="sampling_ratio"):
        _lib.roi_align_kernel("fwd", 16, 2, 16, 12, 14, sampling_ratio=17)
    src = open(os.path.join(ROOT, "replication_faster_rcnn_amd", "csrc", "roi_align.hip")).read()
    assert int(re.search(r"kAlignScan = (\d+);", src).group(1)) == ref.SCAN
    assert int(re.search(r"kAlignTile = (\d+);", src).group(1)) == ref.TILE
    assert int(re.search(r"kAlignMaxRatio = (\d+);", src).group(1)) == ref.MAX_RATIO
