"""Predictions in float16 / bfloat16 (DESIGN.md §3 "Predictions in 16-bit types"): what can
be checked without a GPU.  The C-ABI declares, exports and binds the typed entry points,
they validate their arguments before any HIP call, and the loss case table survives the
rounding of its predictions, so the GPU test leaves out no case."""
import ctypes

import numpy as np
import pytest
import torch

import loss_cases
import loss_ref
from test_capi_cpu import declared_symbols

TYPED = ["frcnn_rpn_head_epilogue_t", "frcnn_losses_fwd_t", "frcnn_losses_bwd_t", "frcnn_detect_t"]
DTYPES = (torch.float16, torch.bfloat16)


def test_typed_entries_are_declared_exported_and_bound():
    from replication_faster_rcnn_amd import _lib
    syms = declared_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in TYPED:
        assert s in syms, s
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    # the typed twin takes the untyped arguments behind the dtype code (the epilogue gains `deltas`)
    for s in TYPED[1:]:
        res, args = _lib.SIGNATURES[s]
        ures, uargs = _lib.SIGNATURES[s[:-2]]
        assert res == ures and args == [_lib.I32] + uargs, s
    res, args = _lib.SIGNATURES["frcnn_rpn_head_epilogue_t"]
    ures, uargs = _lib.SIGNATURES["frcnn_rpn_head_epilogue"]
    assert res == ures and args == [_lib.I32] + uargs[:-1] + [_lib.P, uargs[-1]]


def test_dtype_helpers():
    from replication_faster_rcnn_amd import _lib
    with pytest.raises(RuntimeError, match="RoIPool"):      # the RoIPool helper keeps its own message
        _lib.dtype_code(torch.float64)
    cpu16 = torch.zeros(1, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="detect: cls must be a device tensor"):
        _lib.prediction_dtype_code("detect", (("cls", cpu16), ("reg", cpu16)))
    with pytest.raises(RuntimeError, match="detect: cls must be a device tensor"):
        _lib.prediction_dtype_code("detect", (("cls", None),))


def test_typed_entries_validate_without_gpu():
    """An unknown dtype code, and the untyped functions' shape errors for every dtype, are reported
    before any HIP call (rc = -1 and a message naming the function)."""
    from replication_faster_rcnn_amd import _lib
    lib = _lib.load(require_gpu=False)
    calls = {   # (dtype code, bad) -> rc; `bad` makes the shape invalid
        "frcnn_rpn_head_epilogue_t": lambda dt, bad: lib.frcnn_rpn_head_epilogue_t(
            dt, None, None, 1, 33 if bad else 9, 4, 4, None, None, None, None, None),
        "frcnn_losses_fwd_t": lambda dt, bad: lib.frcnn_losses_fwd_t(
            dt, 4, 129 if bad else 2, 1, None, None, None, None, 0, 1.0, None, None, None, 0, None),
        "frcnn_losses_bwd_t": lambda dt, bad: lib.frcnn_losses_bwd_t(
            dt, 4, 2, 3 if bad else 1, None, None, None, None, 0, 1.0, None, None, None, None, None, None),
        "frcnn_detect_t": lambda dt, bad: lib.frcnn_detect_t(
            dt, 1, 1025 if bad else 4, 21, None, None, None, None, None, None, 600.0, 600.0, 0.05, 0.3, 4,
            None, None, None, None, None, None, None, 0, None),
    }
    shape_words = {"frcnn_rpn_head_epilogue_t": b"bad shape", "frcnn_losses_fwd_t": b"C=129",
                   "frcnn_losses_bwd_t": b"P=3", "frcnn_detect_t": b"R=1025"}
    for fn, call in calls.items():
        for code in (3, -1):
            assert call(code, False) == -1, fn
            msg = lib.frcnn_last_error()
            assert fn.encode() in msg and b"dtype code %d" % code in msg, msg
        for dt in (0, 1, 2):
            assert call(dt, True) == -1, (fn, dt)
            msg = lib.frcnn_last_error()
            assert shape_words[fn] in msg, msg
            # a valid shape with null pointers is refused as well, still before any launch
            assert call(dt, False) == -1, (fn, dt)
            assert b"null" in lib.frcnn_last_error(), lib.frcnn_last_error()
    # the untyped functions answer as before
    assert lib.frcnn_rpn_head_epilogue(None, None, 1, 33, 4, 4, None, None, None, None) == -1
    assert b"frcnn_rpn_head_epilogue: bad shape" in lib.frcnn_last_error()
    assert lib.frcnn_losses_fwd(4, 129, 1, None, None, None, None, 0, 1.0, None, None, None, 0, None) == -1
    assert b"frcnn_losses_fwd: C=129" in lib.frcnn_last_error()
    assert lib.frcnn_detect(1, 1025, 21, None, None, None, None, None, None, 600.0, 600.0, 0.05, 0.3, 4,
                            None, None, None, None, None, None, None, 0, None) == -1
    assert b"frcnn_detect: R=1025" in lib.frcnn_last_error()
    # the strip override of the 16-bit epilogue
    try:
        for p in (b"64", b"128", b"auto"):
            assert lib.frcnn_set_path(b"rpn_epilogue_strip", p) == 0
        assert lib.frcnn_set_path(b"rpn_epilogue_strip", b"32") == -1
    finally:
        lib.frcnn_set_path(b"rpn_epilogue_strip", b"auto")


def rounded(a, dtype):
    """fp32 array -> rounded to dtype and widened back (what the kernels see), fp32."""
    return torch.from_numpy(a).to(dtype).float().numpy()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_every_loss_case_survives_the_rounding(dtype):
    """Every case of the table keeps finite predictions in its labelled rows after rounding to the
    16-bit type, and loss_ref gives finite gradients on them, so the GPU table leaves out no case.
    Only float16 gains infinities at all, and only in the garbage cases' unlabelled rows."""
    assert len(loss_cases.CASES) == 30
    gained = []
    for case in loss_cases.CASES:
        cls, reg, reg_t, lab = case.flat()
        rc, rr = rounded(cls, dtype), rounded(reg, dtype)
        labelled = loss_ref.classify_labels(lab, case.C) >= 0
        assert np.isfinite(rc[labelled]).all() and np.isfinite(rr[labelled]).all(), case.name
        if (np.isinf(rc) & ~np.isinf(cls)).any() or (np.isinf(rr) & ~np.isinf(reg)).any():
            gained.append(case.name)
        ref = loss_ref.stage(rc, rr, reg_t, lab, sigma=case.sigma, head=case.head)
        assert np.isfinite(ref["dcls"]).all() and np.isfinite(ref["dreg"]).all(), case.name
        if labelled.any():
            assert np.isfinite(ref["loss"]).all(), case.name
    want = ["garbage_unlabelled_rpn", "garbage_unlabelled_head"] if dtype == torch.float16 else []
    assert gained == want, gained
