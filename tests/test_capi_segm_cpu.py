"""The C-ABI of the segm evaluation on the host (no GPU): the built library exports the new
symbols, the plan / workspace / kernel-name queries answer without a device, and arguments
outside the limits give 0 or an error code before any HIP call."""
import ctypes
import os

import pytest

from replication_faster_rcnn_amd import _lib, ops

NEW = ("frcnn_mask_overlap", "frcnn_mask_overlap_workspace_size", "frcnn_mask_overlap_plan",
       "frcnn_mask_overlap_kernel", "frcnn_coco_segm_eval_update", "frcnn_coco_eval_kernel")


def test_library_exports_the_new_symbols():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libfrcnn_mi355x.so not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES


def test_plan_and_workspace_queries_answer_on_the_host():
    lib = _lib.load(require_gpu=False)
    plan = _lib.mask_overlap_plan(8, 100, 32, 600, 600)          # the cfg2 shape behind an FPN
    assert plan == dict(words=10, edges=1, pack_blocks=8 * 132, pair_blocks=800, items=39, band_rows=105, bands=6,
                        workspace=plan["workspace"])
    masks = 8 * 132
    assert plan["workspace"] == lib.frcnn_mask_overlap_workspace_size(8, 100, 32, 600, 600)
    assert masks * (600 * 10 * 8 + 32) <= plan["workspace"] < masks * (600 * 10 * 8 + 32) + 512
    assert _lib.mask_overlap_plan(1, 1, 0, 64, 64)["edges"] == 0
    assert ops.mask_overlap_workspace_size(8, 100, 32, 600, 600) == plan["workspace"]


def test_kernel_name_queries():
    assert ops.mask_overlap_kernel(600, 600) == "mo_pack_kernel[vec16+edges]+mo_pair_kernel"
    assert ops.mask_overlap_kernel(600, 608) == "mo_pack_kernel[vec16]+mo_pair_kernel"
    assert ops.coco_eval_kernel() == "coco_match_kernel<boxes>+coco_advance_kernel"
    assert ops.coco_eval_kernel(segm=True) == "coco_match_kernel<counts>+coco_advance_kernel"
    lib = _lib.load(require_gpu=False)
    buf = ctypes.create_string_buffer(64)
    assert lib.frcnn_mask_overlap_kernel(0, 8, buf, 64) == -1 and b"H=0" in lib.frcnn_last_error()
    assert lib.frcnn_mask_overlap_kernel(8, 8, None, 0) == -1
    assert lib.frcnn_coco_eval_kernel(2, buf, 64) == -1 and b"segm" in lib.frcnn_last_error()


def test_out_of_limit_arguments_are_rejected_before_any_launch():
    lib = _lib.load(require_gpu=False)
    for bad in [(0, 1, 1, 8, 8), (1025, 1, 1, 8, 8), (1, 1025, 1, 8, 8), (1, 1, 257, 8, 8), (1, 1, 1, 4097, 8),
                (1, 1, 1, 8, 0)]:
        assert lib.frcnn_mask_overlap_workspace_size(*bad) == 0, bad
        rc = lib.frcnn_mask_overlap(*bad, 2, None, None, None, None, None, None, None, None, None, 0, None)
        assert rc == -1 and b"frcnn_mask_overlap" in lib.frcnn_last_error(), bad
    # labels on one side only, n_class outside [2, 128] with labels, null masks
    one = ctypes.c_void_p(16)
    assert lib.frcnn_mask_overlap(1, 1, 1, 8, 8, 2, one, one, one, None, None, one, one, one, one, 1 << 20, None) == -1
    assert b"together" in lib.frcnn_last_error()
    assert lib.frcnn_mask_overlap(1, 1, 1, 8, 8, 129, one, one, one, None, one, one, one, one, one, 1 << 20, None) == -1
    assert b"n_class" in lib.frcnn_last_error()
    assert lib.frcnn_mask_overlap(1, 1, 1, 8, 8, 2, None, one, None, None, None, one, one, one, one, 1 << 20,
                                  None) == -1
    assert lib.frcnn_mask_overlap(1, 1, 1, 8, 8, 2, ctypes.c_void_p(24), one, None, None, None, one, one, one, one,
                                  1 << 20, None) == -1 and b"aligned" in lib.frcnn_last_error()
    # a workspace that is too small is its own code, still before any launch
    assert lib.frcnn_mask_overlap(1, 1, 1, 8, 8, 2, one, one, None, None, None, one, one, one, one, 8, None) == -3
    for bad in [dict(N=0), dict(M=0), dict(G=257), dict(C=1), dict(C=129), dict(cap=0), dict(cap=(1 << 24) + 1)]:
        a = dict(N=1, M=4, G=2, C=3, cap=16)
        a.update(bad)
        rc = lib.frcnn_coco_segm_eval_update(a["N"], a["M"], a["G"], a["C"], a["cap"], *([one] * 13), None)
        assert rc == -1 and b"frcnn_coco_segm_eval_update" in lib.frcnn_last_error(), bad
    rc = lib.frcnn_coco_segm_eval_update(1, 4, 2, 3, 16, one, one, one, None, one, one, one, one, None, one, one, one,
                                         one, None)
    assert rc == -1 and b"inter" in lib.frcnn_last_error()
