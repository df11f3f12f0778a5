"""ctypes binding of the C-ABI library ``libfrcnn_mi355x.so`` (include/frcnn_capi.h).

The library is built in-tree by ``__graft_entry__.build()`` (or ``make -C
replication_faster_rcnn_amd/csrc``).  There is no CPU fallback: if the
library is missing or no GPU is visible, every op raises.

torch is imported before the library is loaded so that the library's
``libamdhip64.so.7`` dependency resolves to the HIP runtime torch already
loaded (same soname): one runtime, one device-pointer space, torch streams
usable directly.
"""
from __future__ import annotations

import contextlib
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# FRCNN_LIB_PATH: A/B tools may point at another build of the same library
LIB_PATH = os.environ.get("FRCNN_LIB_PATH") or os.path.join(_HERE, "libfrcnn_mi355x.so")

P = ctypes.c_void_p
I32 = ctypes.c_int
I64 = ctypes.c_int64
F32 = ctypes.c_float
F64 = ctypes.c_double
SZ = ctypes.c_size_t


class ProposeParams(ctypes.Structure):
    """frcnn_propose_params (include/frcnn_capi.h)."""

    _fields_ = [("N", I32), ("A", I32), ("K", I32), ("feat_h", I32), ("feat_w", I32),
                ("feat_stride", I32), ("img_h", F32), ("img_w", F32), ("min_size", F32),
                ("pre_nms", I32), ("post_nms", I32), ("iou_threshold", F64)]


# name -> (restype, argtypes); must match include/frcnn_capi.h exactly
SIGNATURES = {
    "frcnn_version": (ctypes.c_char_p, []),
    "frcnn_last_error": (ctypes.c_char_p, []),
    "frcnn_device_cu_count": (I32, [P]),
    "frcnn_set_path": (I32, [ctypes.c_char_p, ctypes.c_char_p]),
    "frcnn_roi_pool_fwd_kernel": (I32, [I64, I32, I32, I32, I32, I32, I32, I32, I32, P, ctypes.c_char_p, SZ]),
    "frcnn_roi_pool_bwd_kernel": (I32, [I64, I32, I32, I32, I32, I32, I32, ctypes.c_char_p, SZ]),
    "frcnn_roi_pool_fwd_kernel_t": (I32, [I32, I64, I32, I32, I32, I32, I32, I32, I32, I32, P, ctypes.c_char_p, SZ]),
    "frcnn_roi_pool_bwd_kernel_t": (I32, [I32, I64, I32, I32, I32, I32, I32, I32, ctypes.c_char_p, SZ]),
    "frcnn_stream_create": (I32, [P, I32, P]),
    "frcnn_stream_destroy": (I32, [P]),
    "frcnn_stream_cu_count": (I32, [P, P]),
    "frcnn_probe_hw_ids": (I32, [P, I32, I32, P]),
    "frcnn_anchor_base": (I32, [P, I32, P, I32, F64, P, P]),
    "frcnn_generate_anchors": (I32, [P, I32, I32, I32, I32, P, P]),
    "frcnn_reg2bbox": (I32, [P, P, I64, P, P]),
    "frcnn_rpn_head_epilogue": (I32, [P, P, I32, I32, I32, I32, P, P, P, P]),
    "frcnn_rpn_head_epilogue_t": (I32, [I32, P, P, I32, I32, I32, I32, P, P, P, P, P]),
    "frcnn_propose_workspace_size":(SZ, [ctypes.POINTER(ProposeParams)]),
    "frcnn_propose": (I32, [ctypes.POINTER(ProposeParams), P, P, P, P, P, P, P, P, SZ, P]),
    "frcnn_nms_workspace_size": (SZ, [I64]),
    "frcnn_nms": (I32, [P, P, I64, F64, P, P, P, SZ, P]),
    "frcnn_roi_transform": (I32, [P, P, I64, F32, F32, I32, I32, P, P]),
    "frcnn_roi_pool_fwd_workspace_size": (SZ, [I64, I32, I32]),
    "frcnn_roi_pool_fwd": (I32, [P, P, I64, I32, I32, I32, I32, I32, I32, F32, I32, P, P, P, SZ, P]),
    "frcnn_roi_pool_fwd_head": (I32, [P, P, P, I64, I32, I32, I32, I32, I32, I32, F32, F32, F32, I32,
                                      P, P, P, P, SZ, P]),
    "frcnn_roi_pool_bwd_workspace_size": (SZ, [I64, I32, I32, I32]),
    "frcnn_roi_pool_bwd": (I32, [P, P, P, I64, I32, I32, I32, I32, I32, I32, F32, P, P, SZ, P]),
    "frcnn_roi_pool_fwd_t": (I32, [I32, P, P, I64, I32, I32, I32, I32, I32, I32, F32, I32, P, P, P, SZ, P]),
    "frcnn_roi_pool_fwd_head_t": (I32, [I32, P, P, P, I64, I32, I32, I32, I32, I32, I32, F32, F32, F32, I32,
                                        P, P, P, P, SZ, P]),
    "frcnn_roi_pool_bwd_t": (I32, [I32, P, P, P, I64, I32, I32, I32, I32, I32, I32, F32, P, P, SZ, P]),
    "frcnn_roi_align_fwd_workspace_size": (SZ, [I64, I32, I32]),
    "frcnn_roi_align_fwd_t": (I32, [I32, P, P, I64, I32, I32, I32, I32, I32, I32, F32, I32, I32, P, P, SZ, P]),
    "frcnn_roi_align_bwd_workspace_size": (SZ, [I64, I32, I32, I32]),
    "frcnn_roi_align_bwd_t": (I32, [I32, P, P, I64, I32, I32, I32, I32, I32, I32, F32, I32, I32, P, P, SZ, P]),
    "frcnn_roi_align_fwd_kernel": (I32, [I32, I64, I32, I32, I32, I32, I32, I32, I32, ctypes.c_char_p, SZ]),
    "frcnn_roi_align_bwd_kernel": (I32, [I32, I64, I32, I32, I32, I32, I32, I32, I32, ctypes.c_char_p, SZ]),
    "frcnn_roi_align_plan": (I32, [I64, I32, I32, I32, I32, I32, I32, P]),
    "frcnn_roi_align_multi_plan": (I32, [I32, P, P, I32, I32, I32, I32, P]),
    "frcnn_roi_align_multi_fwd_t": (I32, [I32, I32, P, P, P, P, P, P, I64, I32, I32, I32, I32, I32, I32, P, P, P, SZ, P]),
    "frcnn_roi_align_multi_bwd_t": (I32, [I32, I32, P, P, P, P, P, P, I64, I32, I32, I32, I32, I32, I32, P, P, SZ, P]),
    "frcnn_roi_align_multi_fwd_kernel": (I32, [I32, I32, I64, I32, I32, I32, I32, I32, ctypes.c_char_p, SZ]),
    "frcnn_roi_align_multi_bwd_kernel": (I32, [I32, I32, I64, I32, I32, I32, I32, I32, ctypes.c_char_p, SZ]),
    "frcnn_propose_multi_workspace_size": (SZ, [I32, I32, I32, P, P, I32, I32]),
    "frcnn_propose_multi_t": (I32, [I32, I32, P, P, P, P, P, P, P, I32, I32, P, I32, I32, F64, F32, F32, P, P, P, P, P, P,
                                    P, SZ, P]),
    "frcnn_propose_multi_kernel": (I32, [I32, I32, I32, I32, P, P, I32, I32, ctypes.c_char_p, SZ]),
    "frcnn_rpn_targets_multi_workspace_size": (SZ, [I32, I32, I32, P, P, I32, I32]),
    "frcnn_rpn_targets_multi": (I32, [I32, P, P, P, P, P, I32, I32, P, P, I32, P, I32, F64, F64, F64, I32, I32,
                                      P, P, P, P, P, P, P, SZ, P]),
    "frcnn_rpn_targets_multi_kernel": (I32, [I32, I32, I32, P, P, I32, I32, I32, ctypes.c_char_p, SZ]),
    "frcnn_rpn_losses_multi_workspace_size": (SZ, [I32, I32]),
    "frcnn_rpn_losses_multi_fwd_t": (I32, [I32, I32, P, P, P, P, I32, I32, I32, P, P, P, P, F64, P, P, P, SZ, P]),
    "frcnn_rpn_losses_multi_bwd_t": (I32, [I32, I32, P, P, P, P, I32, I32, I32, P, P, P, P, F64, P, P, P, P, P, P]),
    "frcnn_box_head_targets_workspace_size": (SZ, [I32, I32, I32, I32]),
    "frcnn_box_head_targets": (I32, [P, P, I32, I32, P, P, P, I32, P, I32, F64, F64, F64, F64, F64, F64, F64, I32, I32,
                                     P, P, P, P, P, P, P, P, P, SZ, P]),
    "frcnn_box_head_targets_kernel": (I32, [I32, I32, I32, I32, I32, ctypes.c_char_p, SZ]),
    "frcnn_box_head_losses_workspace_size": (SZ, [I32, I32]),
    "frcnn_box_head_losses_fwd_t": (I32, [I32, P, P, I32, I32, I32, P, P, P, P, F64, P, P, P, SZ, P]),
    "frcnn_box_head_losses_bwd_t": (I32, [I32, P, P, I32, I32, I32, P, P, P, P, F64, P, P, P, P, P, P]),
    "frcnn_box_detections_workspace_size": (SZ, [I32, I32, I32]),
    "frcnn_box_detections_t": (I32, [I32, I32, I32, I32, P, P, P, P, P, P, F32, F64, I32, F32, F32, F32, F32, F32,
                                     P, P, P, P, P, P, P, SZ, P]),
    "frcnn_box_detections_kernel": (I32, [I32, I32, I32, I32, ctypes.c_char_p, SZ]),
    "frcnn_mask_targets": (I32, [I32, I32, I32, I32, I32, I32, I32, P, P, P, P, P, P, P, P, P, P, P]),
    "frcnn_mask_targets_kernel": (I32, [I32, I32, I32, ctypes.c_char_p, SZ]),
    "frcnn_mask_losses_workspace_size": (SZ, [I32, I32]),
    "frcnn_mask_losses_fwd_t": (I32, [I32, I32, I32, I32, I32, P, P, P, P, P, P, P, SZ, P]),
    "frcnn_mask_losses_bwd_t": (I32, [I32, I32, I32, I32, I32, P, P, P, P, P, P, P, P]),
    "frcnn_mask_losses_kernel": (I32, [I32, I32, I32, ctypes.c_char_p, SZ]),
    "frcnn_mask_paste_t": (I32, [I32, I32, I32, I32, I32, P, P, P, P, P, P, I32, F32, I32, I32, I32, P, P]),
    "frcnn_mask_paste_kernel": (I32, [I32, I32, I32, I32, I32, ctypes.c_char_p, SZ]),
    "frcnn_bbox_iou": (I32, [P, I32, I64, P, I32, I64, P, P]),
    "frcnn_bbox2reg": (I32, [P, I32, P, I32, I64, P, P]),
    "frcnn_anchor_target_workspace_size": (SZ, [I32, I32, I32]),
    "frcnn_anchor_target": (I32, [I32, I32, I32, P, P, P, I32, F64, F64, F64, P, P, P, P, P, P,
                                  SZ, P]),
    "frcnn_anchor_target_prepare": (I32, [I32, I32, I32, P, P, P, F64, F64, P, SZ, P]),
    "frcnn_anchor_target_sample": (I32, [I32, I32, I32, P, I32, F64, P, P, P, P, P, P, SZ, P]),
    "frcnn_proposal_target_workspace_size": (SZ, [I32, I32, I32, I32]),
    "frcnn_proposal_target": (I32, [I32, I32, P, P, I32, P, P, I32, F64, F64, F64, F64, P, P, P,
                                    P, P, P, P, P, SZ, P]),
    "frcnn_anchor_target_draw": (I32, [I32, I32, I32, I32, F64, P, P, SZ, P]),
    "frcnn_anchor_target_finish": (I32, [I32, I32, I32, P, P, P, P, P, P, SZ, P]),
    "frcnn_proposal_target_draw": (I32, [I32, I32, I32, I32, F64, P, P, P, SZ, P]),
    "frcnn_proposal_target_finish": (I32, [I32, I32, I32, I32, P, P, P, P, P, P, P, SZ, P]),
    "frcnn_proposal_target_prepare": (I32, [I32, I32, P, P, I32, P, P, I32, F64, F64, F64, P, SZ, P]),
    "frcnn_proposal_target_sample": (I32, [I32, I32, I32, I32, F64, P, P, P, P, P, P, P, P, SZ, P]),
    "frcnn_anchor_target_draw_status": (I32, [I32, I32, I32, P, SZ, P]),
    "frcnn_proposal_target_draw_status": (I32, [I32, I32, I32, I32, P, SZ, P]),
    "frcnn_target_draws": (I32, [I32, I32, I32, I32, F64, P, SZ, I32, I32, I32, F64, P, SZ, P, P, P]),
    "frcnn_detect_workspace_size": (SZ, [I32, I32, I32]),
    "frcnn_detect": (I32, [I32, I32, I32, P, P, P, P, P, P, F32, F32, F32, F64, I32, P, P, P, P, P, P,
                           P, SZ, P]),
    "frcnn_detect_t": (I32, [I32, I32, I32, I32, P, P, P, P, P, P, F32, F32, F32, F64, I32, P, P, P, P, P, P,
                             P, SZ, P]),
    "frcnn_eval_update": (I32, [I32, I32, I32, I32, I64, P, P, P, P, P, P, P, F64, I32, P, P, P, P, P]),
    "frcnn_eval_ap_workspace_size": (SZ, [I32, I64]),
    "frcnn_eval_ap": (I32, [I32, I64, P, P, P, I32, P, P, P, P, SZ, P]),
    "frcnn_eval_plan": (I32, [I32, I32, I64, P]),
    "frcnn_coco_eval_update": (I32, [I32, I32, I32, I32, I64, P, P, P, P, P, P, P, P, P, P, P, P]),
    "frcnn_coco_eval_workspace_size": (SZ, [I32, I64]),
    "frcnn_coco_eval_accumulate": (I32, [I32, I64, P, P, P, P, P, P, P, P, P, SZ, P]),
    "frcnn_mask_overlap_workspace_size": (SZ, [I32, I32, I32, I32, I32]),
    "frcnn_mask_overlap": (I32, [I32, I32, I32, I32, I32, I32, P, P, P, P, P, P, P, P, P, SZ, P]),
    "frcnn_mask_overlap_plan": (I32, [I32, I32, I32, I32, I32, P]),
    "frcnn_mask_overlap_kernel": (I32, [I32, I32, ctypes.c_char_p, SZ]),
    "frcnn_coco_segm_eval_update": (I32, [I32, I32, I32, I32, I64, P, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    "frcnn_coco_eval_kernel": (I32, [I32, ctypes.c_char_p, SZ]),
    "frcnn_losses_workspace_size": (SZ, [I64, I32]),
    "frcnn_losses_fwd": (I32, [I64, I32, I32, P, P, P, P, I32, F64, P, P, P, SZ, P]),
    "frcnn_losses_bwd": (I32, [I64, I32, I32, P, P, P, P, I32, F64, P, P, P, P, P, P]),
    "frcnn_losses_fwd_t": (I32, [I32, I64, I32, I32, P, P, P, P, I32, F64, P, P, P, SZ, P]),
    "frcnn_losses_bwd_t": (I32, [I32, I64, I32, I32, P, P, P, P, I32, F64, P, P, P, P, P, P]),
    "frcnn_preprocess_workspace_size": (SZ, [I32, I32, I32, I32, I32]),
    "frcnn_preprocess": (I32, [I32, P, I64, P, P, I32, I32, I32, I32, P, P, P, P, P, SZ, P]),
    "frcnn_preprocess_plan": (I32, [I32, I32, I32, I32, I32, P]),
    "frcnn_rescale_boxes": (I32, [I32, I32, P, P, I32, I32, P, P]),
}

# diagnostic entry points of instrumented builds only (not in include/frcnn_capi.h)
DEBUG_SIGNATURES = {
    "frcnn_debug_sampler_prof": (I32, [P, I32]),  # -DFRCNN_SAMPLER_PROF (tools/probe_sampler.py)
}

# frcnn_capi.h's element-type codes of the typed RoIPool entry points
DTYPE_CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def dtype_code(dtype) -> int:
    """FRCNN_F32 / FRCNN_F16 / FRCNN_BF16 for a torch dtype (RuntimeError otherwise)."""
    try:
        return DTYPE_CODES[dtype]
    except KeyError:
        raise RuntimeError(f"RoIPool runs in float32, float16 or bfloat16; got {dtype}") from None


def prediction_dtype_code(op: str, tensors) -> int:
    """The dtype code shared by the prediction inputs of one call of ``op`` (the RPN
    epilogue, the losses, ``detect``): ``tensors`` is ((name, tensor), ...); all must be
    device tensors of one dtype out of float32 / float16 / bfloat16.  RuntimeError naming
    the first offending argument otherwise; attribute reads only."""
    first = None
    for name, t in tensors:
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{op}: {name} must be a device tensor; got {type(t).__name__}")
        if not t.is_cuda:
            raise RuntimeError(f"{op}: {name} must be a device tensor; got a {t.dtype} {t.device.type} tensor")
        if t.dtype not in DTYPE_CODES:
            raise RuntimeError(f"{op}: {name} must be float32, float16 or bfloat16; got {t.dtype}")
        if first is None:
            first = (name, t.dtype)
        elif t.dtype != first[1]:
            raise RuntimeError(f"{op}: {name} is {t.dtype} but {first[0]} is {first[1]}; the predictions of one "
                               "call share one dtype")
    return DTYPE_CODES[first[1]]


_lib = None
_gpu_checked = False


class FrcnnError(RuntimeError):
    pass


def load(require_gpu: bool = True):
    """Load the library (raises FrcnnError if it was not built).  With
    ``require_gpu`` also insist that a HIP device is visible."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FrcnnError(f"HIP library not built: {LIB_PATH} missing "
                             "(run __graft_entry__.build() or make -C replication_faster_rcnn_amd/csrc)")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            if os.environ.get("FRCNN_LIB_PATH") and not hasattr(lib, name):
                continue  # an older build under A/B: bind what it exports
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in DEBUG_SIGNATURES.items():
            if hasattr(lib, name):
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
        _lib = lib
    global _gpu_checked
    if require_gpu and not _gpu_checked:
        if not torch.cuda.is_available():
            raise FrcnnError("replication_faster_rcnn_amd needs an MI355X (no HIP device visible); "
                             "there is no CPU fallback")
        _gpu_checked = True
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        msg = _lib.frcnn_last_error().decode()
        raise FrcnnError(f"{what} failed (rc={rc}): {msg}")


_raw_stream = torch._C._cuda_getCurrentRawStream  # hipStream_t of the current torch stream (int)
_cur_device = torch._C._cuda_getDevice


def stream_ptr(device=None) -> int:
    """hipStream_t (as an int, for c_void_p arguments) of torch's current
    stream on `device` (default: the current device).  The raw torch._C
    getters are used on the issue path: torch.cuda.current_stream() builds a
    Stream object (~2.5 us per call)."""
    if device is None:
        return _raw_stream(_cur_device())
    if isinstance(device, int):
        return _raw_stream(device)
    d = torch.device(device)
    return _raw_stream(d.index if d.index is not None else _cur_device())


def ptr(t):
    """Device address of a tensor (int) or None (NULL) for c_void_p arguments."""
    return t.data_ptr() if t is not None else None


def device():
    """The device the HIP path runs on (current CUDA/HIP device)."""
    return torch.device("cuda", torch.cuda.current_device())


def workspace(nbytes: int, dev) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


_ws_cache = {}


def cached_workspace(tag: str, nbytes: int, dev) -> torch.Tensor:
    """Grow-only scratch buffer per (op, device, current stream): the C-ABI's
    workspaces are stream-ordered scratch, so one buffer per stream serves every
    call on that stream (no allocation on the issue path).  Allocated while the
    stream is current, so the caching allocator orders its reuse on that stream."""
    di = dev.index if isinstance(dev, torch.device) and dev.index is not None else _cur_device()
    key = (tag, di, _raw_stream(di))
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=torch.device("cuda", di))
        _ws_cache[key] = ws
    return ws


def cu_count() -> int:
    lib = load()
    n = ctypes.c_int(0)
    check(lib.frcnn_device_cu_count(ctypes.byref(n)), "device_cu_count")
    return int(n.value)


def cu_stream(cu_mask=None) -> torch.cuda.ExternalStream:
    """A torch stream on the CUs listed in ``cu_mask`` (iterable of CU indices,
    hipExtStreamCreateWithCUMask numbering; None = every CU).  The HIP stream
    lives as long as the process (frcnn_stream_destroy is left to the caller
    via ``stream.frcnn_handle``)."""
    lib = load()
    h = ctypes.c_void_p(0)
    if cu_mask is None:
        check(lib.frcnn_stream_create(None, 0, ctypes.byref(h)), "stream_create")
    else:
        n = cu_count()
        words = (ctypes.c_uint32 * ((n + 31) // 32))()
        for c in cu_mask:
            if not 0 <= int(c) < n:
                raise ValueError(f"CU {c} out of range [0, {n})")
            words[int(c) // 32] |= 1 << (int(c) % 32)
        check(lib.frcnn_stream_create(words, len(words), ctypes.byref(h)), "stream_create")
    s = torch.cuda.ExternalStream(h.value, device=device())
    s.frcnn_handle = h.value
    return s


def stream_cu_count(stream) -> int:
    lib = load()
    n = ctypes.c_int(0)
    check(lib.frcnn_stream_cu_count(ctypes.c_void_p(stream.cuda_stream), ctypes.byref(n)),
          "stream_cu_count")
    return int(n.value)


def roi_pool_fwd_kernel(R, N, C, H, W, PH=7, PW=7, rois_sorted=True, head=True, stream=None,
                        dtype=torch.float32) -> str:
    """frcnn_roi_pool_fwd_kernel_t: the template name of the RoIPool forward kernel
    a call of this shape and feature dtype launches on `stream` (default: the
    current stream)."""
    lib = load()
    s = stream if stream is not None else torch.cuda.current_stream()
    buf = ctypes.create_string_buffer(160)
    check(lib.frcnn_roi_pool_fwd_kernel_t(dtype_code(dtype), int(R), int(N), int(C), int(H), int(W), int(PH),
                                          int(PW), int(bool(rois_sorted)), int(bool(head)),
                                          ctypes.c_void_p(s.cuda_stream), buf, 160), "roi_pool_fwd_kernel")
    return buf.value.decode()


def roi_pool_bwd_kernel(R, N, C, H, W, PH=7, PW=7, dtype=torch.float32) -> str:
    """frcnn_roi_pool_bwd_kernel_t: the template name of the RoIPool backward kernel
    a call of this shape and gradient dtype launches."""
    lib = load()
    buf = ctypes.create_string_buffer(160)
    check(lib.frcnn_roi_pool_bwd_kernel_t(dtype_code(dtype), int(R), int(N), int(C), int(H), int(W), int(PH),
                                          int(PW), buf, 160), "roi_pool_bwd_kernel")
    return buf.value.decode()


def roi_align_kernel(which: str, R, N, C, H, W, PH=7, PW=7, sampling_ratio=-1, dtype=torch.float32) -> str:
    """frcnn_roi_align_fwd_kernel / _bwd_kernel (``which`` = "fwd" | "bwd"): the template
    name of the RoIAlign kernel a call of this shape and dtype launches.  Host only."""
    lib = load(require_gpu=False)
    buf = ctypes.create_string_buffer(160)
    fn = {"fwd": lib.frcnn_roi_align_fwd_kernel, "bwd": lib.frcnn_roi_align_bwd_kernel}[which]
    check(fn(dtype_code(dtype), int(R), int(N), int(C), int(H), int(W), int(PH), int(PW), int(sampling_ratio), buf,
             160), f"roi_align_{which}_kernel")
    return buf.value.decode()


def roi_align_multi_kernel(which: str, n_levels, R, N, C, PH=7, PW=7, sampling_ratio=-1, dtype=torch.float32) -> str:
    """frcnn_roi_align_multi_fwd_kernel / _bwd_kernel (``which`` = "fwd" | "bwd"): the template
    name of the pyramid RoIAlign kernel a call of this dtype launches.  Host only."""
    lib = load(require_gpu=False)
    buf = ctypes.create_string_buffer(160)
    fn = {"fwd": lib.frcnn_roi_align_multi_fwd_kernel, "bwd": lib.frcnn_roi_align_multi_bwd_kernel}[which]
    check(fn(dtype_code(dtype), int(n_levels), int(R), int(N), int(C), int(PH), int(PW), int(sampling_ratio), buf, 160),
          f"roi_align_multi_{which}_kernel")
    return buf.value.decode()


ROI_ALIGN_PLAN_FIELDS = ("run", "tile", "stride", "waves", "stage_bins", "scan", "lane_samples", "fwd_threads",
                         "fwd_grid", "tiles_x", "tiles_y", "cgroups", "units", "blocks", "idle", "lds_bytes", "staged")
ROI_ALIGN_MULTI_PLAN_FIELDS = ("first", "cgroups", "units", "blocks", "idle", "staged")


def roi_align_plan(R, N, C, H, W, PH=7, PW=7) -> dict:
    """frcnn_roi_align_plan: the kernels' constants and the launch numbers of the RoIAlign
    forward and backward for this shape, by ROI_ALIGN_PLAN_FIELDS.  Host only."""
    lib = load(require_gpu=False)
    plan = (ctypes.c_int64 * 17)()
    check(lib.frcnn_roi_align_plan(int(R), int(N), int(C), int(H), int(W), int(PH), int(PW), plan), "roi_align_plan")
    return dict(zip(ROI_ALIGN_PLAN_FIELDS, plan))


def roi_align_multi_plan(sizes, N, C, PH=7, PW=7) -> dict:
    """frcnn_roi_align_multi_plan for the levels' (H, W) ``sizes``: ``first`` (the nine unit
    offsets; level l owns [first[l], first[l + 1])) and the launch numbers of the pyramid
    backward, by ROI_ALIGN_MULTI_PLAN_FIELDS.  Host only."""
    lib = load(require_gpu=False)
    L = len(sizes)
    H, W = (I32 * max(L, 1))(*[int(s[0]) for s in sizes]), (I32 * max(L, 1))(*[int(s[1]) for s in sizes])
    plan = (ctypes.c_int64 * 14)()
    check(lib.frcnn_roi_align_multi_plan(L, H, W, int(N), int(C), int(PH), int(PW), plan), "roi_align_multi_plan")
    return dict(first=list(plan[:9]), **dict(zip(ROI_ALIGN_MULTI_PLAN_FIELDS[1:], plan[9:])))


PREPROCESS_PLAN_FIELDS = ("TH", "lds_rows", "lds_cols", "max_taps", "lds_bytes", "grid_x", "grid_y", "grid_z")


def preprocess_plan(N, max_hw, out_hw) -> dict:
    """frcnn_preprocess_plan: the tile height, footprint bounds, LDS bytes and grid that
    ``frcnn_preprocess`` launches with for these host bounds, by PREPROCESS_PLAN_FIELDS.  Host only."""
    lib = load(require_gpu=False)
    plan = (ctypes.c_int32 * 8)()
    check(lib.frcnn_preprocess_plan(int(N), int(max_hw[0]), int(max_hw[1]), int(out_hw[0]), int(out_hw[1]), plan),
          "preprocess_plan")
    return dict(zip(PREPROCESS_PLAN_FIELDS, plan))


EVAL_PLAN_FIELDS = ("count_step", "count_steps", "match_chunk", "match_chunks", "sort_tile", "sort_tiles",
                    "sort_passes", "scan_len", "scan_share", "walk_chunk")


def eval_plan(N, M, n_records) -> dict:
    """frcnn_eval_plan: the chunk, tile and scan numbers ``frcnn_eval_update`` (N images of M
    slots) and ``frcnn_eval_ap`` (n_records records) launch with, by EVAL_PLAN_FIELDS.  Host only."""
    lib = load(require_gpu=False)
    plan = (ctypes.c_int64 * 10)()
    check(lib.frcnn_eval_plan(int(N), int(M), int(n_records), plan), "eval_plan")
    return dict(zip(EVAL_PLAN_FIELDS, plan))


MASK_OVERLAP_PLAN_FIELDS = ("words", "edges", "pack_blocks", "pair_blocks", "workspace", "items", "band_rows", "bands")


def mask_overlap_plan(N, D, G, H, W) -> dict:
    """frcnn_mask_overlap_plan: words per row, the pack branch, the workgroups of the two
    launches, the workspace bytes and the band shape of ``frcnn_mask_overlap``, by
    MASK_OVERLAP_PLAN_FIELDS.  Host only."""
    lib = load(require_gpu=False)
    plan = (ctypes.c_int64 * 8)()
    check(lib.frcnn_mask_overlap_plan(int(N), int(D), int(G), int(H), int(W), plan), "mask_overlap_plan")
    return dict(zip(MASK_OVERLAP_PLAN_FIELDS, plan))


def set_path(op: str, path) -> None:
    """frcnn_set_path: select a kernel path ("auto" restores the default)."""
    lib = load(require_gpu=False)
    check(lib.frcnn_set_path(op.encode(), str(path).encode()), f"set_path({op}, {path})")


@contextlib.contextmanager
def kernel_path(op: str, path):
    """Run a block with one op's kernel path forced (tests / A-B tools)."""
    set_path(op, path)
    try:
        yield
    finally:
        set_path(op, "auto")
