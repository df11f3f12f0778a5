"""CPU-side checks of the detection stage: the C-ABI boundary (no compute, no
GPU), the numpy restatement against its golden file, and the generator."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detect_ref  # noqa: E402
from replication_faster_rcnn_amd import synth  # noqa: E402

NAMES = ("boxes", "labels", "scores", "roi", "count", "total")


def test_header_and_library_have_detect():
    from replication_faster_rcnn_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "frcnn_capi.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("frcnn_detect", "frcnn_detect_workspace_size"):
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES


def _call(lib, N=2, R=96, C=21, max_det=10, null_out=False, ws_short=0):
    """frcnn_detect with dummy non-null pointers: every case here is rejected
    before any pointer is used or any HIP call is made."""
    need = lib.frcnn_detect_workspace_size(2, 96, 21) if ws_short else 1 << 40
    host4 = (ctypes.c_float * 4)()
    d = ctypes.c_void_p(0x1000)
    outs = [d] * 6
    if null_out:
        outs[3] = None
    return lib.frcnn_detect(N, R, C, d, d, d, d, host4, host4, 600.0, 1000.0, 0.05, 0.3, max_det, *outs,
                            d, need - ws_short, None)


def test_detect_argument_validation_without_gpu():
    from replication_faster_rcnn_amd import _lib
    lib = _lib.load(require_gpu=False)
    for kw, word in [(dict(C=1), b"C="), (dict(N=0), b"N="), (dict(N=-3), b"N="), (dict(R=1025), b"R="),
                     (dict(R=0), b"R="), (dict(C=129), b"C="), (dict(null_out=True), b"det_roi"),
                     (dict(max_det=0), b"max_det")]:
        assert _call(lib, **kw) == -1, kw
        assert word in lib.frcnn_last_error(), (kw, lib.frcnn_last_error())
    assert _call(lib, ws_short=1) == -3
    assert b"workspace" in lib.frcnn_last_error()


def test_detect_workspace_size():
    from replication_faster_rcnn_amd import _lib
    lib = _lib.load(require_gpu=False)
    size = lib.frcnn_detect_workspace_size
    for shape in [(0, 96, 21), (2, 0, 21), (2, 1025, 21), (2, 96, 1), (2, 96, 129)]:
        assert size(*shape) == 0, shape
    base = size(2, 96, 21)
    assert base >= 2 * 96 * (21 + 20 * 6) * 4   # probabilities + the kept (row, score, box) lists
    assert size(3, 96, 21) > base and size(2, 97, 21) > base and size(2, 96, 22) > base
    assert size(65535, 1024, 128) > 0


def test_detect_ref_reproduces_golden(golden):
    g = golden("detect_small.npz")
    assert g["cls"].shape == (2, 96, 21)
    for tag, thr in (("t005", 0.05), ("t07", 0.7)):
        res = detect_ref.detect(g["rois"], g["rcount"], g["cls"], g["reg"], 600, 1000, score_thresh=thr)
        for name, a in zip(NAMES, res):
            want = g[f"{tag}_{name}"]
            assert a.dtype == want.dtype and np.array_equal(a, want), (tag, name)
    assert g["t005_count"].min() > g["t07_count"].max() >= 1   # the two thresholds are different cases


def test_golden_inputs_are_the_generator_s():
    import hashlib
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "detect_small.npz")))
    a = synth.head_outputs(2, 96, 21, 600, 1000, seed=1)
    for name, arr in zip(("rois", "rcount", "cls", "reg"), a):
        assert arr.dtype == g[name].dtype
        assert hashlib.sha1(arr.tobytes()).digest() == hashlib.sha1(g[name].tobytes()).digest(), name


def test_head_outputs_is_seeded_per_global_image():
    full = synth.head_outputs(4, 50, 21, 600, 1000, seed=9)
    part = synth.head_outputs(2, 50, 21, 600, 1000, seed=9, first_image=2)
    one = synth.head_outputs(1, 50, 21, 600, 1000, seed=9, first_image=3)
    for f, p, o in zip(full, part, one):
        assert np.array_equal(f[2:], p) and np.array_equal(f[3:], o)
    assert not np.array_equal(full[2][0], full[2][1])
    rois, rcount, cls, reg = full
    assert rois.dtype == cls.dtype == reg.dtype == np.float32 and rcount.dtype == np.int32
    assert rois.shape == (4, 50, 4) and cls.shape == (4, 50, 21) and reg.shape == (4, 50, 84)
    assert (rcount == 50).all()
    assert (rois[..., 2] > rois[..., 0]).all() and (rois[..., 3] > rois[..., 1]).all()
    assert rois.min() >= 0 and rois[..., 2].max() <= 600 and rois[..., 3].max() <= 1000
