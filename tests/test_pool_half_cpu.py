"""RoIPool in float16 / bfloat16: what can be checked without a GPU.  The references
of tests/pool_half_ref.py say what they are meant to say, the C-ABI declares and binds
the typed entry points, and those validate their arguments before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch

import pool_half_ref as phr
from oracle import ref_numpy as orc
from test_capi_cpu import declared_symbols

TYPED = ["frcnn_roi_pool_fwd_t", "frcnn_roi_pool_fwd_head_t", "frcnn_roi_pool_bwd_t",
         "frcnn_roi_pool_fwd_kernel_t", "frcnn_roi_pool_bwd_kernel_t"]


@pytest.mark.parametrize("hw", [(12, 14), (38, 38)])
@pytest.mark.parametrize("dtype", phr.DTYPES)
def test_forward_ref_is_exact_but_for_flt_max(dtype, hw):
    """Max-pooling selects elements, so the rounded reference widens back to the fp32
    oracle's output bit for bit; only the oracle's -FLT_MAX (a non-empty bin in which
    nothing passed the strict '>') has no 16-bit value and becomes -inf.  Bit-exactness
    is therefore the right bar for the kernels."""
    x = phr.special_x(dtype, np.random.default_rng(7), H=hw[0], W=hw[1])
    rois = phr.special_rois()
    out, am = phr.forward_ref(x, rois, 7)
    oo, oa = orc.roi_pool_forward(x.float().numpy(), rois, 7)
    assert out.dtype == dtype and np.array_equal(am, oa)
    back = out.float().numpy()
    none = oo == -phr.FLT_MAX
    assert none.any() and (am[none] == -1).all()
    assert np.isneginf(back[none]).all()
    assert np.array_equal(back[~none].view(np.uint32), oo[~none].view(np.uint32))
    # the special planes did their work: subnormals, both zeros, +inf and the dtype's
    # lowest value were selected, empty bins gave +0
    sel = phr.bits(out)[torch.from_numpy(am >= 0)]
    vals = out[torch.from_numpy(am >= 0)].float()
    assert ((vals != 0) & (vals.abs() < torch.finfo(dtype).tiny)).any()
    assert (sel == 0).any() and (sel == -32768).any()
    assert torch.isposinf(vals).any() and (vals == torch.finfo(dtype).min).any()
    assert (phr.bits(out)[torch.from_numpy((am == -1) & ~none)] == 0).all()


@pytest.mark.parametrize("dtype", phr.DTYPES)
def test_backward_ref_separates_one_rounding_from_many(dtype):
    """On the colliding-gradient case the reference (fp32 sums, one rounding) differs
    from sums accumulated in the 16-bit type, so a kernel that accumulated in T
    could not pass the GPU test."""
    x, rois, grad = phr.colliding_case(dtype)
    out, am = phr.forward_ref(x, rois, 7)
    g = grad(out.shape)
    ref = phr.backward_ref(g, rois, am, x.shape)
    acc = phr.backward_accumulated_in_t(g, rois, am, x.shape)
    assert ref.dtype == dtype and torch.isfinite(ref.float()).all()
    ndiff = int((phr.bits(ref) != phr.bits(acc)).sum())
    assert ndiff > 0
    # and both are the same sums up to the rounding
    torch.testing.assert_close(acc.float(), ref.float(), rtol=0.1, atol=0.1)


def test_header_declares_the_typed_entries():
    syms = declared_symbols()
    for s in TYPED:
        assert s in syms, s
    text = open(__import__("test_capi_cpu").HEADER).read()
    assert "FRCNN_F32 = 0" in text and "FRCNN_F16 = 1" in text and "FRCNN_BF16 = 2" in text


def test_signatures_cover_the_typed_entries():
    from replication_faster_rcnn_amd import _lib
    for s in TYPED:
        assert s in _lib.SIGNATURES, s
    # the typed twin takes the untyped arguments behind the dtype code
    for s in TYPED:
        res, args = _lib.SIGNATURES[s]
        ures, uargs = _lib.SIGNATURES[s[:-2]]
        assert res == ures and args == [_lib.I32] + uargs, s
    assert _lib.DTYPE_CODES == {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
    with pytest.raises(RuntimeError, match="float64"):
        _lib.dtype_code(torch.float64)


def test_typed_entries_validate_without_gpu():
    """An unknown dtype code and a bad output_size are reported before any HIP call
    (rc = -1 and a message naming the offender), for every typed entry and dtype."""
    from replication_faster_rcnn_amd import _lib
    lib = _lib.load(require_gpu=False)
    name = ctypes.create_string_buffer(160)
    calls = {
        "frcnn_roi_pool_fwd_t": lambda dt, ph: lib.frcnn_roi_pool_fwd_t(
            dt, None, None, 1, 1, 1, 1, 1, ph, 7, 1.0, 0, None, None, None, 0, None),
        "frcnn_roi_pool_fwd_head_t": lambda dt, ph: lib.frcnn_roi_pool_fwd_head_t(
            dt, None, None, None, 1, 1, 1, 1, 1, ph, 7, 600.0, 1000.0, 1.0, 0, None, None, None, None, 0, None),
        "frcnn_roi_pool_bwd_t": lambda dt, ph: lib.frcnn_roi_pool_bwd_t(
            dt, None, None, None, 1, 1, 1, 1, 1, ph, 7, 1.0, None, None, 0, None),
        "frcnn_roi_pool_fwd_kernel_t": lambda dt, ph: lib.frcnn_roi_pool_fwd_kernel_t(
            dt, 1, 1, 1, 1, 1, ph, 7, 1, 1, None, name, 160),
        "frcnn_roi_pool_bwd_kernel_t": lambda dt, ph: lib.frcnn_roi_pool_bwd_kernel_t(
            dt, 1, 1, 1, 1, 1, ph, 7, name, 160),
    }
    for fn, call in calls.items():
        for code in (3, -1):
            assert call(code, 7) == -1, fn
            msg = lib.frcnn_last_error()
            assert fn.encode() in msg and b"dtype code %d" % code in msg, msg
        for dt in (0, 1, 2):
            assert call(dt, 0) == -1, (fn, dt)
            msg = lib.frcnn_last_error()
            assert b"output_size" in msg or b"bad shape" in msg, msg
    # the untyped functions answer as before
    rc = lib.frcnn_roi_pool_fwd(None, None, 1, 1, 1, 1, 1, 0, 7, 1.0, 0, None, None, None, 0, None)
    assert rc == -1 and b"output_size" in lib.frcnn_last_error()
