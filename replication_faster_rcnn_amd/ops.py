"""torchvision-surface ops the reference calls, on the HIP path.

* ``nms(boxes, scores, iou_threshold)`` -- ``torchvision.ops.nms`` as called at
  nets/rpn.py:75 (imported nets/rpn.py:4, utils/utils.py:4).
* ``roi_pool(input, boxes, output_size, spatial_scale)`` -- ``torchvision.ops.
  roi_pool`` as called at nets/heads.py:48, with an autograd backward (the
  reference reaches torchvision's ``_roi_pool_backward`` from
  ``total_loss.backward()`` at train.py:126).
* ``roi_align(input, boxes, output_size, spatial_scale, sampling_ratio,
  aligned)`` -- ``torchvision.ops.roi_align`` with the semantics and summation
  order of torchvision's CPU kernel, forward and a deterministic backward (no
  reference counterpart: the RoI feature extractor users swap in for
  ``roi_pool``; DESIGN.md §3 "RoIAlign").
* ``multiscale_roi_align(features, boxes, output_size, spatial_scales,
  sampling_ratio)`` / ``MultiScaleRoIAlign`` -- ``torchvision.ops.
  MultiScaleRoIAlign``'s pooling over a feature pyramid, the level of every RoI
  decided inside one forward and one backward launch (DESIGN.md §3 "Multi-scale
  RoIAlign"); ``roi_align``'s input rule.
* ``propose(...)`` -- the batched proposal layer (nets/rpn.py:47-79 over all
  images at once, replacing the per-image loop nets/rpn.py:131-136).
* ``propose_multilevel(...)`` -- the FPN proposal layer, torchvision's
  ``RegionProposalNetwork.filter_proposals`` over a pyramid of RPN head outputs
  (no reference counterpart; DESIGN.md §3 "FPN proposals"), with
  ``pyramid_anchor_bases`` / ``pyramid_anchors`` (torchvision's ``AnchorGenerator``)
  and ``logit_threshold`` (its score threshold as a test on the raw logit).
* ``rpn_targets_multilevel(...)`` / ``rpn_losses_multilevel(...)`` -- the training half of that
  RPN: torchvision's ``assign_targets_to_anchors``, ``Matcher``, ``BalancedPositiveNegativeSampler``,
  ``BoxCoder.encode`` and ``compute_loss`` over the pyramid, with ``sampler_state`` (no reference
  counterpart; DESIGN.md §3 "Pyramid RPN training").
* ``box_head_targets(...)`` / ``box_head_losses(...)`` -- the training half of the box head behind
  it: torchvision's ``select_training_samples`` (``add_gt_proposals``, ``Matcher``, the sampler,
  ``BoxCoder.encode``) and ``fastrcnn_loss`` on ``propose_multilevel``'s proposals (no reference
  counterpart; DESIGN.md §3 "Pyramid box-head training").
* ``box_head_detections(...)`` -- the inference half of that head: torchvision's
  ``RoIHeads.postprocess_detections`` and the transform's ``resize_boxes`` on ``propose_multilevel``'s
  proposals and the head's outputs (no reference counterpart; DESIGN.md §3 "Pyramid box-head
  inference").
* ``detect(...)`` -- head outputs -> per-class decoded, thresholded and NMS-ed
  detections for the whole batch (no reference counterpart; DESIGN.md
  "Detections").
* ``eval_update(...)`` / ``eval_ap(...)`` -- PASCAL VOC evaluation of those
  detections against ground truth on the device (no reference counterpart:
  its test_eval.py is empty; DESIGN.md "Evaluation").
* ``coco_eval_update(...)`` / ``coco_eval_accumulate(...)`` -- the COCO protocol
  on the same inputs: AP over IoU 0.50:0.95, by object size, AR at 1 / 10 / 100
  detections (DESIGN.md "COCO-style evaluation").
* ``mask_overlap(...)`` / ``coco_segm_eval_update(...)`` -- the same protocol with
  iouType "segm" on ``mask_head_paste``'s masks: pixel counts of the masks and of
  their intersections, then the matching on those counts (DESIGN.md §3 "COCO segm
  evaluation").
* ``rpn_losses(...)`` / ``head_losses(...)`` -- the four training losses of
  train.py:29-57, :81-83, :112-121, fused, with their own backward (DESIGN.md
  "Losses").
* ``preprocess(...)`` / ``rescale_boxes(...)`` -- the image half of
  ``voc_data.__getitem__`` (utils/data_loader.py:38,61-75) for a batch: resize
  as ``skimage.transform.resize`` does, ``ToTensor``, ``Normalize``, and the
  boxes' rescale (DESIGN.md "Preprocessing").

Two input rules (tests/test_gpu_wrapper_inputs.py):

* The reference-signature drop-ins (``nms``, ``roi_pool*``, ``roi_pool_head``,
  ``roi_align``, ``multiscale_roi_align``, ``rpn_head_epilogue``) convert whatever they are given: inputs
  may live on the CPU (reference style), be strided views or another float type;
  they are moved to the current HIP device as contiguous fp32, and results are
  returned on the input's device.  They raise only on shapes that do not belong
  together (``roi_align`` also on a ``sampling_ratio`` above 16).
  One exception keeps its type: a float16 or bfloat16 ``input`` of ``roi_pool``,
  ``roi_pool_with_argmax``, ``roi_pool_head`` and ``roi_align`` (a backbone under autocast) is
  moved or made contiguous if needed but never widened, the pooled output and
  the gradient have the input's dtype as torchvision's do, and the kernels
  read and write the 16-bit values directly (DESIGN.md §3 "RoIPool in 16-bit
  types").  ``boxes`` / ``rois`` / ``roi_inds`` stay fp32, ``argmax`` int32.
  The same holds for float16 / bfloat16 conv outputs of ``rpn_head_epilogue``
  (both of one dtype): ``cls_nhwc`` / ``reg_nhwc`` come back in that dtype.
* The hot-path ops on device tensors (``propose``, ``propose_multilevel``, ``rpn_targets_multilevel``,
  ``rpn_losses_multilevel``, ``box_head_targets``, ``box_head_losses``, ``box_head_detections``, ``roi_transform``,
  ``detect``, ``eval_update``, ``coco_eval_update``, ``mask_overlap``, ``coco_segm_eval_update``, ``rpn_losses``, ``head_losses``, ``preprocess``,
  ``rescale_boxes``) convert nothing: every tensor must already be a
  contiguous device tensor of the documented dtype and exact shape, checked by
  attribute reads alone (no copy, no synchronisation) before any launch.
  The predictions ``cls`` / ``reg`` of ``detect``, ``rpn_losses`` and
  ``head_losses`` may be float16 or bfloat16 instead of fp32, both in the same
  dtype (DESIGN.md §3 "Predictions in 16-bit types"); so may ``class_logits`` /
  ``box_regression`` of ``box_head_losses`` and ``box_head_detections``.

Errors follow torchvision's ``TORCH_CHECK`` -> ``RuntimeError`` convention.
"""
from __future__ import annotations

import collections
from typing import List, Tuple, Union

import torch

from . import _lib


def _to_dev(t: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    # the device-resident fast path: already on the device the kernels launch on
    if t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.device.index == _lib._cur_device():
        return t
    return t.to(device=_lib.device(), dtype=dtype).contiguous()


def _require(op: str, name: str, t, dtype, shape) -> None:
    """The hot-path ops' input rule: ``t`` is a contiguous device tensor of
    ``dtype`` and exactly ``shape``.  Attribute reads only."""
    if (not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous()
            or t.shape != shape):
        got = (f"{'contiguous' if t.is_contiguous() else 'strided'} {t.dtype} {t.device.type} tensor of shape "
               f"{list(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__)
        raise RuntimeError(f"{op}: {name} must be a contiguous {dtype} device tensor of shape {list(shape)}; "
                           f"got a {got}")


# ----------------------------------------------------------------------- nms
def nms(boxes: torch.Tensor, scores: torch.Tensor, iou_threshold: float) -> torch.Tensor:
    """torchvision.ops.nms: int64 indices of kept boxes, by decreasing score."""
    lib = _lib.load()
    if boxes.dim() != 2 or boxes.size(1) != 4:
        raise RuntimeError(f"boxes should have 2 dimensions with 4 columns, got {tuple(boxes.shape)}")
    if scores.dim() != 1 or scores.size(0) != boxes.size(0):
        raise RuntimeError("boxes and scores should have the same number of elements in dim 0")
    out_dev = boxes.device
    b = _to_dev(boxes)
    s = _to_dev(scores)
    n = b.size(0)
    keep = torch.empty(max(n, 1), dtype=torch.int64, device=b.device)
    cnt = torch.zeros(1, dtype=torch.int32, device=b.device)
    ws = _lib.workspace(lib.frcnn_nms_workspace_size(n), b.device)
    _lib.check(lib.frcnn_nms(_lib.ptr(b), _lib.ptr(s), n, float(iou_threshold), _lib.ptr(keep),
                             _lib.ptr(cnt), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "nms")
    k = int(cnt.item())
    return keep[:k].to(out_dev)


# ------------------------------------------------------------------ roi_pool
_POOL_HALF = (torch.float16, torch.bfloat16)
_POOL_DTYPE_CODE = _lib.DTYPE_CODES  # torch dtype -> the C-ABI's FRCNN_F32 / FRCNN_F16 / FRCNN_BF16


def _pool_input(t: torch.Tensor) -> torch.Tensor:
    """RoIPool's feature rule: float16 / bfloat16 keep their type (moved or made
    contiguous if needed, never widened), everything else becomes fp32."""
    return _to_dev(t, t.dtype if t.dtype in _POOL_HALF else torch.float32)


def _pool_dtype_error(op: str, dtype):
    return RuntimeError(f"{op}: tensors must be float32, float16 or bfloat16; got {dtype}")


def _roi_pool_fwd(x: torch.Tensor, rois: torch.Tensor, ph: int, pw: int, ss: float,
                  rois_sorted: bool = False):
    lib = _lib.load()
    N, C, H, W = x.shape
    R = rois.size(0)
    dt = x.dtype
    code = _POOL_DTYPE_CODE.get(dt)
    if code is None:
        raise _pool_dtype_error("roi_pool forward", dt)
    out = torch.empty((R, C, ph, pw), dtype=dt, device=x.device)
    am = torch.empty((R, C, ph, pw), dtype=torch.int32, device=x.device)
    ws = _lib.cached_workspace("roi_pool_fwd", lib.frcnn_roi_pool_fwd_workspace_size(R, N, C), x.device)
    _lib.check(lib.frcnn_roi_pool_fwd_t(code, _lib.ptr(x), _lib.ptr(rois), R, N, C, H, W,
                                        ph, pw, float(ss), int(bool(rois_sorted)), _lib.ptr(out), _lib.ptr(am),
                                        _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "roi_pool forward")
    return out, am


def _sorted_by_image(boxes) -> bool:
    """Host-side check when the RoIs live on the host (the reference's case);
    device RoIs are treated as unsorted unless the caller says otherwise."""
    if isinstance(boxes, torch.Tensor) and boxes.is_cuda:
        return False
    b = (boxes.detach() if isinstance(boxes, torch.Tensor) else torch.as_tensor(boxes))[:, 0]
    bi = b.to(torch.int64)
    return bool((bi[1:] >= bi[:-1]).all()) if bi.numel() > 1 else True


def _roi_pool_bwd(grad: torch.Tensor, rois: torch.Tensor, am: torch.Tensor, shape, ss: float):
    lib = _lib.load()
    N, C, H, W = shape
    R, _, ph, pw = grad.shape
    dt = grad.dtype
    code = _POOL_DTYPE_CODE.get(dt)
    if code is None:
        raise _pool_dtype_error("roi_pool backward", dt)
    gi = torch.empty((N, C, H, W), dtype=dt, device=grad.device)
    ws = _lib.cached_workspace("roi_pool_bwd", lib.frcnn_roi_pool_bwd_workspace_size(R, N, ph, pw),
                               grad.device)
    _lib.check(lib.frcnn_roi_pool_bwd_t(code, _lib.ptr(grad), _lib.ptr(rois), _lib.ptr(am),
                                        R, N, C, H, W, ph, pw, float(ss), _lib.ptr(gi), _lib.ptr(ws), ws.numel(),
                                        _lib.stream_ptr()), "roi_pool backward")
    return gi


def _pool_grad(grad_out: torch.Tensor, dtype) -> torch.Tensor:
    """The gradient as the backward kernel reads it: contiguous, in the pooled
    output's dtype (which autograd already guarantees; the cast is a no-op then)."""
    g = grad_out if grad_out.dtype == dtype else grad_out.to(dtype)
    return g.contiguous()


class _RoIPoolFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rois, ph, pw, ss, rois_sorted=False):
        out, am = _roi_pool_fwd(x, rois, ph, pw, ss, rois_sorted)
        ctx.save_for_backward(rois, am)
        ctx.meta = (tuple(x.shape), ss, x.dtype)
        ctx.mark_non_differentiable(am)
        return out, am

    @staticmethod
    def backward(ctx, grad_out, _grad_am):
        rois, am = ctx.saved_tensors
        shape, ss, dtype = ctx.meta
        gi = _roi_pool_bwd(_pool_grad(grad_out, dtype), rois, am, shape, ss)
        return gi, None, None, None, None, None


def _roi_pool_head_fwd(x, rois, roi_inds, ph, pw, img_h, img_w, ss, rois_sorted, outs=None):
    lib = _lib.load()
    N, C, H, W = x.shape
    R = rois.size(0)
    dt = x.dtype
    code = _POOL_DTYPE_CODE.get(dt)
    if code is None:
        raise _pool_dtype_error("roi_pool_head", dt)
    if outs is None:
        boxes = torch.empty((R, 5), dtype=torch.float32, device=x.device)
        out = torch.empty((R, C, ph, pw), dtype=dt, device=x.device)
        am = torch.empty((R, C, ph, pw), dtype=torch.int32, device=x.device)
    else:  # caller-owned (out, argmax, boxes): no allocation on the issue path
        out, am, boxes = outs
        if (tuple(out.shape) != (R, C, ph, pw) or tuple(am.shape) != (R, C, ph, pw)
                or tuple(boxes.shape) != (R, 5) or out.dtype != dt
                or am.dtype != torch.int32 or boxes.dtype != torch.float32):
            what = "fp32" if dt == torch.float32 else f"{dt} (the input's dtype)"
            raise RuntimeError(f"roi_pool_head: out buffers must be {what} [R,C,ph,pw], int32 [R,C,ph,pw], "
                               "fp32 [R,5]")
    ws = _lib.cached_workspace("roi_pool_fwd", lib.frcnn_roi_pool_fwd_workspace_size(R, N, C), x.device)
    _lib.check(lib.frcnn_roi_pool_fwd_head_t(
        code, _lib.ptr(x), _lib.ptr(rois), _lib.ptr(roi_inds), R, N, C, H, W, ph, pw, float(img_h),
        float(img_w), float(ss), int(bool(rois_sorted)), _lib.ptr(boxes), _lib.ptr(out),
        _lib.ptr(am), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "roi_pool_head forward")
    return out, am, boxes


class _RoIPoolHeadFunction(torch.autograd.Function):
    """nets/heads.py:42-48 (RoI transform + pack + roi_pool) as one op; the
    backward is roi_pool's, on the [R,5] boxes the forward wrote."""

    @staticmethod
    def forward(ctx, x, rois, roi_inds, ph, pw, img_h, img_w, ss, rois_sorted):
        out, am, boxes = _roi_pool_head_fwd(x, rois, roi_inds, ph, pw, img_h, img_w, ss, rois_sorted)
        ctx.save_for_backward(boxes, am)
        ctx.meta = (tuple(x.shape), ss, x.dtype)
        ctx.mark_non_differentiable(am, boxes)
        return out, am, boxes

    @staticmethod
    def backward(ctx, grad_out, _grad_am, _grad_boxes):
        boxes, am = ctx.saved_tensors
        shape, ss, dtype = ctx.meta
        gi = _roi_pool_bwd(_pool_grad(grad_out, dtype), boxes, am, shape, ss)
        return gi, None, None, None, None, None, None, None, None


def roi_pool_head(input: torch.Tensor, rois: torch.Tensor, roi_inds: torch.Tensor, output_size,
                  img_h, img_w, spatial_scale: float = 1.0, rois_sorted: bool = False, out=None):
    """ResnetHead's RoI transform + ``[idx, box]`` pack + roi_pool
    (nets/heads.py:42-48) in one call on device tensors: rois fp32 [R,4] in
    image pixels, roi_inds [R] -> (out [R,C,ph,pw], argmax int32, boxes [R,5]).
    A float16 / bfloat16 ``input`` stays in its type and ``out`` has it too.
    ``rois_sorted`` promises RoIs grouped by non-decreasing image index (RPN
    proposals, train.py's sample_rois): then the transform runs inside the
    pool kernel.  ``out`` = caller-owned (out, argmax, boxes) buffers
    (inference only)."""
    if input.dim() != 4:
        raise RuntimeError("input must be [N, C, H, W]")
    if rois.dim() != 2 or rois.size(1) != 4 or roi_inds.dim() != 1 or roi_inds.size(0) != rois.size(0):
        raise RuntimeError(f"rois must be [R, 4] and roi_inds [R]; got {tuple(rois.shape)}, "
                           f"{tuple(roi_inds.shape)}")
    ph, pw = (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)
    x = _to_dev(input) if input.dtype is torch.float32 else _pool_input(input)
    args = (x, _to_dev(rois), _to_dev(roi_inds), int(ph), int(pw), float(img_h), float(img_w),
            float(spatial_scale), bool(rois_sorted))
    if not (torch.is_grad_enabled() and x.requires_grad):  # inference: no autograd node
        return _roi_pool_head_fwd(*args, outs=out)
    if out is not None:
        raise RuntimeError("roi_pool_head: out= is for inference (no autograd)")
    return _RoIPoolHeadFunction.apply(*args)


def _boxes_to_rois(boxes: Union[torch.Tensor, List[torch.Tensor]]) -> torch.Tensor:
    if isinstance(boxes, (list, tuple)):  # torchvision's List[Tensor[L,4]] form
        parts = [torch.cat([torch.full((b.size(0), 1), i, dtype=b.dtype, device=b.device), b], 1)
                 for i, b in enumerate(boxes)]
        boxes = torch.cat(parts, 0) if parts else torch.zeros((0, 5))
    if boxes.dim() != 2 or boxes.size(1) != 5:
        raise RuntimeError(f"boxes must be [K, 5] (batch_idx, x1, y1, x2, y2); got {tuple(boxes.shape)}")
    return boxes


def roi_pool_with_argmax(input: torch.Tensor, boxes, output_size, spatial_scale: float = 1.0,
                         rois_sorted=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """roi_pool returning (out, argmax int32) -- the torch.ops.torchvision.roi_pool pair.
    ``out`` is fp32, or float16 / bfloat16 for an input of that dtype.
    ``rois_sorted``: RoIs grouped by non-decreasing batch index (None = check
    host-resident RoIs, assume unsorted for device RoIs)."""
    if input.dim() != 4:
        raise RuntimeError("input must be [N, C, H, W]")
    ph, pw = (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)
    out_dev = input.device
    x = _pool_input(input)  # differentiable move, so CPU leaf tensors get their grad
    b = _boxes_to_rois(boxes)
    if rois_sorted is None:
        rois_sorted = _sorted_by_image(b)
    rois = _to_dev(b)
    out, am = _RoIPoolFunction.apply(x.contiguous(), rois, int(ph), int(pw), float(spatial_scale),
                                     bool(rois_sorted))
    return out.to(out_dev), am.to(out_dev)


def roi_pool(input: torch.Tensor, boxes, output_size, spatial_scale: float = 1.0,
             rois_sorted=None) -> torch.Tensor:
    """torchvision.ops.roi_pool (nets/heads.py:48)."""
    return roi_pool_with_argmax(input, boxes, output_size, spatial_scale, rois_sorted)[0]


# ----------------------------------------------------------------- roi_align
ROI_ALIGN_MAX_SAMPLING_RATIO = 16


def _roi_align_fwd(x: torch.Tensor, rois: torch.Tensor, ph: int, pw: int, ss: float, sr: int, aligned: bool):
    lib = _lib.load()
    N, C, H, W = x.shape
    R = rois.size(0)
    code = _POOL_DTYPE_CODE.get(x.dtype)
    if code is None:
        raise _pool_dtype_error("roi_align forward", x.dtype)
    out = torch.empty((R, C, ph, pw), dtype=x.dtype, device=x.device)
    _lib.check(lib.frcnn_roi_align_fwd_t(code, _lib.ptr(x), _lib.ptr(rois), R, N, C, H, W, ph, pw, float(ss), int(sr),
                                         int(bool(aligned)), _lib.ptr(out), None, 0, _lib.stream_ptr()),
               "roi_align forward")
    return out


def _roi_align_bwd(grad: torch.Tensor, rois: torch.Tensor, shape, ss: float, sr: int, aligned: bool):
    lib = _lib.load()
    N, C, H, W = shape
    R, _, ph, pw = grad.shape
    code = _POOL_DTYPE_CODE.get(grad.dtype)
    if code is None:
        raise _pool_dtype_error("roi_align backward", grad.dtype)
    gi = torch.empty((N, C, H, W), dtype=grad.dtype, device=grad.device)
    _lib.check(lib.frcnn_roi_align_bwd_t(code, _lib.ptr(grad), _lib.ptr(rois), R, N, C, H, W, ph, pw, float(ss),
                                         int(sr), int(bool(aligned)), _lib.ptr(gi), None, 0, _lib.stream_ptr()),
               "roi_align backward")
    return gi


class _RoIAlignFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rois, ph, pw, ss, sr, aligned):
        out = _roi_align_fwd(x, rois, ph, pw, ss, sr, aligned)
        ctx.save_for_backward(rois)
        ctx.meta = (tuple(x.shape), ph, pw, ss, sr, aligned, x.dtype)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (rois,) = ctx.saved_tensors
        shape, ph, pw, ss, sr, aligned, dtype = ctx.meta
        gi = _roi_align_bwd(_pool_grad(grad_out, dtype), rois, shape, ss, sr, aligned)
        return gi, None, None, None, None, None, None


def roi_align(input: torch.Tensor, boxes, output_size, spatial_scale: float = 1.0, sampling_ratio: int = -1,
              aligned: bool = False) -> torch.Tensor:
    """torchvision.ops.roi_align with the semantics and the summation order of
    torchvision's CPU kernel, forward and backward (frcnn_roi_align_fwd_t /
    _bwd_t; DESIGN.md §3 "RoIAlign" is the contract): bilinear samples on a
    ``sampling_ratio`` x ``sampling_ratio`` grid per bin (<= 0: adaptive,
    ceil(bin size); at most 16), averaged.  ``boxes`` is [K, 5] (batch_idx, x1,
    y1, x2, y2) or a list of [L, 4] tensors, in any order.  The gradient is
    deterministic and bit-equal to the CPU order of additions (torchvision's
    own GPU backward is neither).

    A reference-signature drop-in, with ``roi_pool``'s input rule: host, strided
    or other float inputs are converted and the result comes back on the
    input's device; a float16 / bfloat16 ``input`` is never widened and ``out``
    and the gradient have its dtype.  RoIs with a batch index outside [0, N) or
    a scaled coordinate that is not finite or beyond 2^20 give zeros and no
    gradient."""
    if not isinstance(input, torch.Tensor) or input.dim() != 4:
        raise RuntimeError("input must be [N, C, H, W]")
    try:
        ph, pw = (output_size, output_size) if isinstance(output_size, int) else (int(v) for v in output_size)
    except (TypeError, ValueError):
        raise RuntimeError(f"roi_align: output_size must be an int or (h, w); got {output_size!r}") from None
    if isinstance(boxes, (list, tuple)):
        if len(boxes) != input.size(0):
            raise RuntimeError(f"roi_align: a list of boxes needs one entry per image; got {len(boxes)} for "
                               f"{input.size(0)} images")
        if any(not isinstance(b, torch.Tensor) or b.dim() != 2 or b.size(1) != 4 for b in boxes):
            raise RuntimeError("roi_align: every entry of a list of boxes must be a [L, 4] tensor")
    out_dev = input.device
    x = _pool_input(input)  # differentiable move, so CPU leaf tensors get their grad
    rois = _to_dev(_boxes_to_rois(boxes))
    out = _RoIAlignFunction.apply(x, rois, int(ph), int(pw), float(spatial_scale), int(sampling_ratio),
                                  bool(aligned))
    return out.to(out_dev)


# ------------------------------------------------------ multi-scale roi_align
ROI_ALIGN_MAX_LEVELS = 8
_level_cache = {}     # (k_min, k_max, s0, lvl0) -> thresholds
_pyramid_cache = {}   # (scales, s0, lvl0) -> (k_min, k_max, thresholds)


def level_formula(s: torch.Tensor, k_min: int, k_max: int, canonical_scale=224, canonical_level=4) -> torch.Tensor:
    """torchvision's ``LevelMapper`` on ``s = sqrt(area)``, a CPU fp32 tensor: int64 levels
    counted from 0 (``floor(lvl0 + log2(s / s0) + 1e-6)`` clamped to [k_min, k_max], minus k_min)."""
    lvl = torch.floor(canonical_level + torch.log2(s / canonical_scale) + torch.tensor(1e-6, dtype=s.dtype))
    return torch.clamp(lvl, min=k_min, max=k_max).to(torch.int64) - k_min


def level_thresholds(k_min: int, k_max: int, canonical_scale=224, canonical_level=4) -> Tuple[float, ...]:
    """The ``k_max - k_min`` ascending fp32 thresholds the kernels count against
    (``level = #{k : sqrt(area) >= t_k}``): ``t_k`` is the smallest non-negative fp32 value at
    which ``level_formula`` yields at least ``k``, found by bisection over the fp32 bit
    patterns from +0 to +inf (the formula is nondecreasing).  Host only; cached."""
    key = (int(k_min), int(k_max), canonical_scale, canonical_level)
    thr = _level_cache.get(key)
    if thr is None:
        n = key[1] - key[0]
        if n < 0:
            raise RuntimeError(f"level_thresholds: k_max {k_max} is below k_min {k_min}")
        want = torch.arange(1, n + 1, dtype=torch.int64)
        lo = torch.zeros(n, dtype=torch.int32)                    # +0: level 0, below every k
        hi = torch.full((n,), 0x7F800000, dtype=torch.int32)      # +inf: level k_max - k_min
        while bool((hi - lo > 1).any()):
            mid = lo + (hi - lo) // 2
            ge = level_formula(mid.view(torch.float32), key[0], key[1], canonical_scale, canonical_level) >= want
            hi = torch.where(ge, mid, hi)
            lo = torch.where(ge, lo, mid)
        thr = tuple(float(v) for v in hi.view(torch.float32))
        _level_cache[key] = thr
    return thr


def _pyramid_levels(scales, canonical_scale, canonical_level):
    """(k_min, k_max, thresholds) of a pyramid's scales, as torchvision's ``_setup_scales``
    derives the level range: -log2 of the first and of the last scale, in fp32, truncated."""
    key = (tuple(scales), canonical_scale, canonical_level)
    hit = _pyramid_cache.get(key)
    if hit is None:
        if any(not s > 0 for s in key[0]):
            raise RuntimeError(f"multiscale_roi_align: spatial_scales must be positive; got {list(scales)}")
        k_min = int(-torch.log2(torch.tensor(key[0][0], dtype=torch.float32)).item())
        k_max = int(-torch.log2(torch.tensor(key[0][-1], dtype=torch.float32)).item())
        if len(key[0]) != k_max - k_min + 1:
            raise RuntimeError(f"multiscale_roi_align: {len(key[0])} feature maps, but scales {list(scales)} span "
                               f"the levels {k_min}..{k_max} ({k_max - k_min + 1} maps, one per octave)")
        hit = (k_min, k_max, level_thresholds(k_min, k_max, canonical_scale, canonical_level))
        _pyramid_cache[key] = hit
    return hit


class _PyramidArgs:
    """The per-level host arrays of the C-ABI pair for one call."""

    def __init__(self, shapes, scales, thresholds):
        L = len(shapes)
        self.L = L
        self.H = (_lib.I32 * L)(*[s[2] for s in shapes])
        self.W = (_lib.I32 * L)(*[s[3] for s in shapes])
        self.scales = (_lib.F32 * L)(*scales)
        self.thr = (_lib.F32 * max(L - 1, 1))(*thresholds)

    @staticmethod
    def ptrs(tensors):
        return (_lib.P * len(tensors))(*[t.data_ptr() for t in tensors])


def _multiscale_fwd(xs, rois, ph, pw, scales, thresholds, sr, aligned, want_levels):
    lib = _lib.load()
    x0 = xs[0]
    N, C = x0.shape[:2]
    R = rois.size(0)
    code = _POOL_DTYPE_CODE.get(x0.dtype)
    if code is None:
        raise _pool_dtype_error("multiscale_roi_align forward", x0.dtype)
    a = _PyramidArgs([x.shape for x in xs], scales, thresholds)
    out = torch.empty((R, C, ph, pw), dtype=x0.dtype, device=x0.device)
    levels = torch.empty((R,), dtype=torch.int32, device=x0.device) if want_levels else None
    _lib.check(lib.frcnn_roi_align_multi_fwd_t(code, a.L, a.ptrs(xs), a.H, a.W, a.scales, a.thr, _lib.ptr(rois), R, N,
                                               C, ph, pw, int(sr), int(bool(aligned)), _lib.ptr(out),
                                               _lib.ptr(levels), None, 0, _lib.stream_ptr()),
               "multiscale_roi_align forward")
    return out, levels


def _multiscale_bwd(grad, rois, shapes, scales, thresholds, sr, aligned):
    lib = _lib.load()
    N, C = shapes[0][:2]
    R, _, ph, pw = grad.shape
    code = _POOL_DTYPE_CODE.get(grad.dtype)
    if code is None:
        raise _pool_dtype_error("multiscale_roi_align backward", grad.dtype)
    a = _PyramidArgs(shapes, scales, thresholds)
    gis = [torch.empty(tuple(s), dtype=grad.dtype, device=grad.device) for s in shapes]
    _lib.check(lib.frcnn_roi_align_multi_bwd_t(code, a.L, _lib.ptr(grad), a.H, a.W, a.scales, a.thr, _lib.ptr(rois), R,
                                               N, C, ph, pw, int(sr), int(bool(aligned)), a.ptrs(gis), None, 0,
                                               _lib.stream_ptr()),
               "multiscale_roi_align backward")
    return gis


class _MultiScaleRoIAlignFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rois, ph, pw, scales, thresholds, sr, aligned, want_levels, *xs):
        out, levels = _multiscale_fwd(xs, rois, ph, pw, scales, thresholds, sr, aligned, want_levels)
        ctx.save_for_backward(rois)
        ctx.meta = ([tuple(x.shape) for x in xs], scales, thresholds, sr, aligned, xs[0].dtype)
        if levels is None:
            return out
        ctx.mark_non_differentiable(levels)
        return out, levels

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, *_):
        (rois,) = ctx.saved_tensors
        shapes, scales, thresholds, sr, aligned, dtype = ctx.meta
        gis = _multiscale_bwd(_pool_grad(grad_out, dtype), rois, shapes, scales, thresholds, sr, aligned)
        return (None,) * 8 + tuple(gis)   # a gradient for every level: zeros where no RoI mapped


def multiscale_roi_align(features, boxes, output_size, spatial_scales, sampling_ratio: int, *, canonical_scale=224,
                         canonical_level=4, aligned: bool = False, return_levels: bool = False):
    """``torchvision.ops.MultiScaleRoIAlign``'s pooling over a feature pyramid in one launch,
    forward and backward (frcnn_roi_align_multi_fwd_t / _bwd_t; DESIGN.md §3 "Multi-scale
    RoIAlign" is the contract).  ``features``: the maps [N, C, H_l, W_l], fine to coarse,
    of one N, C and dtype, at most 8; ``spatial_scales``: one per map, an octave apart
    (``k_min`` / ``k_max`` are -log2 of the first / last, as torchvision derives them);
    ``boxes``: [K, 5] (batch_idx, x1, y1, x2, y2) in image coordinates or a list of [L_i, 4]
    tensors, in any order.  Each RoI is pooled from the level torchvision's ``LevelMapper``
    gives it -- decided on the device, with no host sync -- exactly as ``roi_align`` pools
    it from that map alone; the output comes in RoI order, and the backward returns a
    deterministic gradient for every level (zeros for a level no RoI mapped to).
    ``return_levels``: also return the int32 [K] level of each RoI.

    ``roi_align``'s input rule: host, strided or other float inputs are converted, results
    come back on the first map's device, float16 / bfloat16 maps are never widened.  One map
    delegates to ``roi_align``."""
    op = "multiscale_roi_align"
    feats = list(features)
    if not feats or any(not isinstance(f, torch.Tensor) or f.dim() != 4 for f in feats):
        raise RuntimeError(f"{op}: features must be a non-empty sequence of [N, C, H, W] tensors")
    if len(feats) > ROI_ALIGN_MAX_LEVELS:
        raise RuntimeError(f"{op}: at most {ROI_ALIGN_MAX_LEVELS} levels; got {len(feats)}")
    f0 = feats[0]
    for i, f in enumerate(feats):
        if f.shape[:2] != f0.shape[:2] or f.dtype != f0.dtype:
            raise RuntimeError(f"{op}: the levels share N, C and dtype; features[{i}] is {f.dtype} "
                               f"{list(f.shape)}, features[0] is {f0.dtype} {list(f0.shape)}")
    scales = tuple(float(s) for s in spatial_scales)
    if len(scales) != len(feats):
        raise RuntimeError(f"{op}: {len(feats)} feature maps but {len(scales)} spatial_scales")
    _, _, thresholds = _pyramid_levels(scales, canonical_scale, canonical_level)
    try:
        ph, pw = (output_size, output_size) if isinstance(output_size, int) else (int(v) for v in output_size)
    except (TypeError, ValueError):
        raise RuntimeError(f"{op}: output_size must be an int or (h, w); got {output_size!r}") from None
    if isinstance(boxes, (list, tuple)):
        if len(boxes) != f0.size(0):
            raise RuntimeError(f"{op}: a list of boxes needs one entry per image; got {len(boxes)} for "
                               f"{f0.size(0)} images")
        if any(not isinstance(b, torch.Tensor) or b.dim() != 2 or b.size(1) != 4 for b in boxes):
            raise RuntimeError(f"{op}: every entry of a list of boxes must be a [L, 4] tensor")
    if len(feats) == 1:
        out = roi_align(f0, boxes, (ph, pw), scales[0], sampling_ratio, aligned)
        return (out, torch.zeros(out.size(0), dtype=torch.int32, device=out.device)) if return_levels else out
    out_dev = f0.device
    xs = [_pool_input(f) for f in feats]  # differentiable moves, so CPU leaf tensors get their grad
    rois = _to_dev(_boxes_to_rois(boxes))
    res = _MultiScaleRoIAlignFunction.apply(rois, int(ph), int(pw), scales, thresholds, int(sampling_ratio),
                                            bool(aligned), bool(return_levels), *xs)
    if return_levels:
        return res[0].to(out_dev), res[1].to(out_dev)
    return res.to(out_dev)


class MultiScaleRoIAlign(torch.nn.Module):
    """``torchvision.ops.MultiScaleRoIAlign`` on ``multiscale_roi_align``: ``forward(x, boxes,
    image_shapes)`` takes the dict of feature maps (those named in ``featmap_names`` are
    used, in the dict's order, fine to coarse), a list of [L_i, 4] boxes per image and the
    list of the images' (h, w), and returns [sum L_i, C, *output_size].  The scales are
    inferred as torchvision infers them (2 ** round(log2(map size / largest image size)) per
    axis, the two axes agreeing) on the first call and cached with the level thresholds."""

    def __init__(self, featmap_names, output_size, sampling_ratio: int, *, canonical_scale=224, canonical_level=4):
        super().__init__()
        self.featmap_names = list(featmap_names)
        self.output_size = (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)
        self.sampling_ratio = int(sampling_ratio)
        self.canonical_scale, self.canonical_level = canonical_scale, canonical_level
        self.scales = None

    @staticmethod
    def infer_scales(features, image_shapes):
        max_h, max_w = max(int(s[0]) for s in image_shapes), max(int(s[1]) for s in image_shapes)
        scales = []
        for f in features:
            per_axis = [2.0 ** float(torch.tensor(float(s) / float(o)).log2().round())
                        for s, o in zip(f.shape[-2:], (max_h, max_w))]
            if per_axis[0] != per_axis[1]:
                raise RuntimeError(f"MultiScaleRoIAlign: a {list(f.shape[-2:])} map of {max_h} x {max_w} images "
                                   f"has the scales {per_axis[0]} and {per_axis[1]} along its two axes")
            scales.append(per_axis[0])
        return tuple(scales)

    def forward(self, x, boxes, image_shapes):
        feats = [v for k, v in x.items() if k in self.featmap_names]
        if self.scales is None:
            self.scales = self.infer_scales(feats, image_shapes)
            _pyramid_levels(self.scales, self.canonical_scale, self.canonical_level)
        return multiscale_roi_align(feats, list(boxes), self.output_size, self.scales, self.sampling_ratio,
                                    canonical_scale=self.canonical_scale, canonical_level=self.canonical_level)


# ------------------------------------------------------------------ proposals
_params_cache = {}  # launch-parameter block + workspace size per layer shape (built once)


def propose(scores: torch.Tensor, deltas: torch.Tensor, *, img_w: float, img_h: float,
            pre_nms: int, post_nms: int, nms_thresh: float = 0.7, min_size: float = 16,
            anchors: torch.Tensor = None, anchor_base: torch.Tensor = None, feat_h: int = 0,
            feat_w: int = 0, feat_stride: int = 16, out=None, workspace=None):
    """Batched proposal layer on device tensors.

    scores fp32 [N, A], deltas fp32 [N, A, 4]; either explicit ``anchors``
    [A, 4] or ``anchor_base`` [K, 4] + the feature grid (anchors generated in
    the decode kernel).  Returns padded (rois [N, post, 4], anchor_idx int32
    [N, post], count int32 [N]) -- no host synchronisation.

    A hot-path op: nothing is converted.  ``scores``, ``deltas``, ``anchors``,
    ``anchor_base`` and the ``out`` buffers must be contiguous device tensors of
    the dtypes and exact shapes above (RuntimeError naming the argument
    otherwise; attribute reads only, before any launch).  A strided view such
    as ``softmax(cls, -1)[..., 1]`` needs ``.contiguous()`` first.
    """
    lib = _lib.load()
    if not isinstance(scores, torch.Tensor) or scores.dim() != 2:
        raise RuntimeError("propose: scores must be a contiguous torch.float32 device tensor of shape [N, A]")
    N, A = scores.shape
    _require("propose", "scores", scores, torch.float32, (N, A))
    _require("propose", "deltas", deltas, torch.float32, (N, A, 4))
    dev = scores.device
    if anchors is not None:
        K = 0
        _require("propose", "anchors", anchors, torch.float32, (A, 4))
    elif anchor_base is not None:
        K = anchor_base.size(0) if isinstance(anchor_base, torch.Tensor) and anchor_base.dim() == 2 else -1
        _require("propose", "anchor_base", anchor_base, torch.float32, (K, 4))
    else:
        raise RuntimeError("propose: give anchors [A, 4] or anchor_base [K, 4] with the feature grid")
    key = (N, A, K, feat_h, feat_w, feat_stride, float(img_h), float(img_w), float(min_size),
           int(pre_nms), int(post_nms), float(nms_thresh))
    cached = _params_cache.get(key)
    if cached is None:
        if anchors is None and K * feat_h * feat_w != A:
            raise RuntimeError(f"A={A} != feat_h*feat_w*K={feat_h}*{feat_w}*{K}")
        p = _lib.ProposeParams()
        p.N, p.A = N, A
        p.K, p.feat_h, p.feat_w, p.feat_stride = K, feat_h, feat_w, feat_stride
        p.img_h, p.img_w, p.min_size = float(img_h), float(img_w), float(min_size)
        p.pre_nms, p.post_nms, p.iou_threshold = int(pre_nms), int(post_nms), float(nms_thresh)
        cached = (p, int(lib.frcnn_propose_workspace_size(p)))
        _params_cache[key] = cached
    p, need = cached
    if out is None:
        rois = torch.empty((N, post_nms, 4), dtype=torch.float32, device=dev)
        idx = torch.empty((N, post_nms), dtype=torch.int32, device=dev)
        cnt = torch.empty((N,), dtype=torch.int32, device=dev)
    else:  # caller-owned outputs (static buffers of a captured HIP graph)
        if len(out) != 3:
            raise RuntimeError("propose: out buffers must be fp32 [N,post,4], int32 [N,post], int32 [N]")
        rois, idx, cnt = out
        _require("propose", "out[0] (rois)", rois, torch.float32, (N, post_nms, 4))
        _require("propose", "out[1] (anchor_idx)", idx, torch.int32, (N, post_nms))
        _require("propose", "out[2] (count)", cnt, torch.int32, (N,))
    ws = workspace if workspace is not None else _lib.cached_workspace("propose", need, dev)
    if not ws.is_cuda or ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < need:
        raise RuntimeError(f"propose: workspace must be a contiguous uint8 device tensor of at least {need} B; "
                           f"got {ws.dtype} on {ws.device.type} with {ws.numel()} elements")
    _lib.check(lib.frcnn_propose(p, _lib.ptr(scores), _lib.ptr(deltas), _lib.ptr(anchors),
                                 _lib.ptr(anchor_base), _lib.ptr(rois), _lib.ptr(idx),
                                 _lib.ptr(cnt), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
               "propose")
    return rois, idx, cnt


# -------------------------------------------------------------- FPN proposals
FPN_MAX_LEVELS, FPN_MAX_K, FPN_MAX_PRE, FPN_MAX_POST, FPN_MAX_N = 8, 32, 2048, 4096, 1024
FPN_SORT_CAP = 2048           # a level of at most this many anchors is sorted whole ("sort"), a larger one "select"
_logit_thr_cache = {}         # score_thresh -> logit threshold
_fpn_cache = {}               # shape key -> (H, W, stride_h, stride_w host arrays, workspace bytes)
_fpn_sizes_cache = {}         # (h, w, N, device index) -> fp32 [N, 2] device tensor


def pyramid_anchor_bases(sizes, aspect_ratios, device=None):
    """torchvision's ``AnchorGenerator.generate_anchors`` in fp32 with torch CPU ops:
    ``h_ratios = sqrt(ratios)``, ``w_ratios = 1 / h_ratios``, ``base = stack([-ws, -hs, ws,
    hs], 1) / 2`` rounded, rows ratio-major.  ``sizes`` is one level's tuple of numbers (-> one
    [K, 4] tensor) or a tuple of such tuples, one per level (-> a list); ``aspect_ratios``
    likewise, a flat tuple serving every level.  ``device``: where the result goes (default:
    the CPU; the op wants its bases on the device)."""
    def one(scales, ratios):
        s = torch.as_tensor(tuple(scales), dtype=torch.float32)
        r = torch.as_tensor(tuple(ratios), dtype=torch.float32)
        h_ratios = torch.sqrt(r)
        w_ratios = 1 / h_ratios
        ws = (w_ratios[:, None] * s[None, :]).view(-1)
        hs = (h_ratios[:, None] * s[None, :]).view(-1)
        base = (torch.stack([-ws, -hs, ws, hs], dim=1) / 2).round()
        return base if device is None else base.to(device)

    sizes = tuple(sizes)
    if not sizes:
        raise RuntimeError("pyramid_anchor_bases: sizes is empty")
    if not isinstance(sizes[0], (tuple, list)):
        return one(sizes, aspect_ratios)
    ratios = tuple(aspect_ratios)
    if not isinstance(ratios[0], (tuple, list)):
        ratios = (ratios,) * len(sizes)
    if len(ratios) != len(sizes):
        raise RuntimeError(f"pyramid_anchor_bases: {len(sizes)} levels of sizes but {len(ratios)} of aspect_ratios")
    return [one(s, r) for s, r in zip(sizes, ratios)]


def pyramid_anchors(anchor_bases, strides, grid_sizes):
    """torchvision's ``AnchorGenerator.grid_anchors`` with torch CPU ops: per level an fp32
    [H*W*K, 4] tensor, anchor ``(y*W + x)*K + k = base[k] + (x*stride_w, y*stride_h, x*stride_w,
    y*stride_h)``, one fp32 addition per coordinate.  ``strides``: (stride_h, stride_w) per
    level; ``grid_sizes``: (H, W) per level.  For tests and target assignment; the op forms the
    same anchors in registers."""
    out = []
    for base, (sh, sw), (H, W) in zip(anchor_bases, strides, grid_sizes):
        b = base.detach().to("cpu", torch.float32)
        xs = (torch.arange(int(W), dtype=torch.int64) * int(sw)).to(torch.float32)
        ys = (torch.arange(int(H), dtype=torch.int64) * int(sh)).to(torch.float32)
        sy, sx = torch.meshgrid(ys, xs, indexing="ij")
        shifts = torch.stack([sx.reshape(-1), sy.reshape(-1), sx.reshape(-1), sy.reshape(-1)], dim=1)
        out.append((shifts[:, None, :] + b[None, :, :]).reshape(-1, 4))
    return out


def _f32_ordinal(x: float) -> int:
    """Position of an fp32 value in the total order -inf .. -0 < +0 .. +inf (an int)."""
    i = int(torch.tensor(x, dtype=torch.float32).view(torch.int32))
    return i if i >= 0 else -(i & 0x7FFFFFFF) - 1


def _f32_from_ordinal(o: int) -> float:
    i = o if o >= 0 else ((-o - 1) | 0x80000000) - (1 << 32)
    return float(torch.tensor(i, dtype=torch.int32).view(torch.float32))


def logit_threshold(score_thresh: float) -> float:
    """The score threshold of torchvision's ``scores >= score_thresh`` as a threshold on the raw
    logit: the smallest fp32 ``t`` with ``torch.sigmoid(t) >= score_thresh`` on the CPU, found by
    bisection over the fp32 bit patterns from -inf to +inf (torch's CPU sigmoid is nondecreasing),
    so ``logit >= t`` is the same test and the kernels evaluate no sigmoid.  ``score_thresh <= 0``
    gives -inf (every non-NaN logit passes), one above 1 NaN (none does).  Host only; cached."""
    key = float(score_thresh)
    t = _logit_thr_cache.get(key)
    if t is None:
        if key != key or key > 1.0:
            t = float("nan")
        elif key <= 0.0:
            t = float("-inf")
        else:
            thr = torch.tensor(key, dtype=torch.float32)

            def passes(o):
                return bool(torch.sigmoid(torch.tensor(_f32_from_ordinal(o), dtype=torch.float32)) >= thr)

            lo, hi = _f32_ordinal(float("-inf")), _f32_ordinal(float("inf"))   # sigmoid 0 < thr <= 1 = sigmoid(+inf)
            if not passes(hi):          # a threshold that rounds above 1 in fp32 cannot occur; keep the rule total
                t = float("nan")
            else:
                while hi - lo > 1:
                    mid = (lo + hi) // 2
                    if passes(mid):
                        hi = mid
                    else:
                        lo = mid
                t = _f32_from_ordinal(hi)
        _logit_thr_cache[key] = t
    return t


def _fpn_tensor(name, t, dtype, shape):
    if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous()
            or tuple(t.shape) != tuple(shape)):
        got = (f"{'contiguous' if t.is_contiguous() else 'strided'} {t.dtype} {t.device.type} tensor of shape "
               f"{list(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__)
        raise RuntimeError(f"propose_multilevel: {name} must be a contiguous {dtype} device tensor of shape "
                           f"{list(shape)}; got a {got}")


def _fpn_shape_key(op, objectness, strides, pre, post):
    """(L, N, K, ((H, W, stride_h, stride_w), ...), pre, post) with the limits checked."""
    if not isinstance(objectness, (list, tuple)) or not 1 <= len(objectness) <= FPN_MAX_LEVELS:
        raise RuntimeError(f"{op}: objectness must be a list of 1 to {FPN_MAX_LEVELS} tensors [N, K, H, W]")
    L = len(objectness)
    o0 = objectness[0]
    if not isinstance(o0, torch.Tensor) or o0.dim() != 4:
        raise RuntimeError(f"{op}: objectness[0] must be a device tensor of shape [N, K, H, W]")
    N, K = int(o0.shape[0]), int(o0.shape[1])
    if not 1 <= N <= FPN_MAX_N:
        raise RuntimeError(f"{op}: objectness: N must be in [1, {FPN_MAX_N}]; got {N}")
    if not 1 <= K <= FPN_MAX_K:
        raise RuntimeError(f"{op}: objectness: K must be in [1, {FPN_MAX_K}]; got {K}")
    if not isinstance(strides, (list, tuple)) or len(strides) != L:
        raise RuntimeError(f"{op}: strides must list one (stride_h, stride_w) per level ({L})")
    pre, post = int(pre), int(post)
    if not 1 <= pre <= FPN_MAX_PRE:
        raise RuntimeError(f"{op}: pre_nms_top_n must be in [1, {FPN_MAX_PRE}]; got {pre}")
    if not 1 <= post <= FPN_MAX_POST:
        raise RuntimeError(f"{op}: post_nms_top_n must be in [1, {FPN_MAX_POST}]; got {post}")
    levels = []
    for l, (o, s) in enumerate(zip(objectness, strides)):
        if not isinstance(o, torch.Tensor) or o.dim() != 4:
            raise RuntimeError(f"{op}: objectness[{l}] must be a device tensor of shape [N, K, H, W]")
        try:
            sh, sw = int(s[0]), int(s[1])
        except (TypeError, ValueError, IndexError):
            raise RuntimeError(f"{op}: strides[{l}] must be (stride_h, stride_w) ints; got {s!r}") from None
        H, W = int(o.shape[2]), int(o.shape[3])
        if H < 1 or W < 1 or K * H * W >= 1 << 24:
            raise RuntimeError(f"{op}: objectness[{l}]: H, W >= 1 and K*H*W < 2^24 are required; got {list(o.shape)}")
        if sh < 1 or sw < 1 or (H - 1) * sh >= 1 << 24 or (W - 1) * sw >= 1 << 24:
            raise RuntimeError(f"{op}: strides[{l}] = {(sh, sw)}: strides >= 1 and (H-1)*stride_h, (W-1)*stride_w "
                               "below 2^24 are required")
        levels.append((H, W, sh, sw))
    return L, N, K, tuple(levels), pre, post


def propose_multilevel_kernel(objectness_shapes, dtype, pre_nms_top_n, post_nms_top_n) -> str:
    """frcnn_propose_multi_kernel: the kernels a call on maps of these [N, K, H, W] shapes
    launches, with the selection branch of every level ("sort" | "select").  Host only."""
    lib = _lib.load(require_gpu=False)
    shapes = [tuple(int(v) for v in s) for s in objectness_shapes]
    L = len(shapes)
    H = (_lib.I32 * L)(*[s[2] for s in shapes])
    W = (_lib.I32 * L)(*[s[3] for s in shapes])
    buf = _lib.ctypes.create_string_buffer(256)
    _lib.check(lib.frcnn_propose_multi_kernel(_lib.dtype_code(dtype), L, shapes[0][0], shapes[0][1], H, W,
                                              int(pre_nms_top_n), int(post_nms_top_n), buf, 256),
               "propose_multi_kernel")
    return buf.value.decode()


def propose_multilevel(objectness, deltas, anchor_bases, strides, image_sizes, *, pre_nms_top_n: int,
                       post_nms_top_n: int, nms_thresh: float = 0.7, score_thresh: float = 0.0,
                       min_size: float = 1e-3, out=None, workspace=None):
    """The FPN proposal layer: torchvision's ``RegionProposalNetwork.filter_proposals`` with
    ``BoxCoder(weights=(1, 1, 1, 1))`` for the whole batch and pyramid, four launches, no host
    synchronisation (frcnn_propose_multi_t; DESIGN.md §3 "FPN proposals" is the contract).

    ``objectness``: L tensors [N, K, H_l, W_l]; ``deltas``: L tensors [N, 4K, H_l, W_l] (channel
    4k + c) -- an ``RPNHead``'s conv outputs as they are, all fp32, float16 or bfloat16, read in
    place; ``anchor_bases``: L fp32 device tensors [K, 4] (``pyramid_anchor_bases``);
    ``strides``: L host (stride_h, stride_w); ``image_sizes``: fp32 device tensor [N, 2] of
    (h, w), or one host (h, w) for every image (expanded once, cached).

    Per image and level: the first ``min(pre_nms_top_n, A_l)`` anchors in torch's stable
    descending order of the raw logit (NaN first, -0 == +0, ties by anchor index) are decoded,
    clipped to the image, filtered (``min_size``; ``sigmoid(logit) >= score_thresh`` as a test
    on the logit, ``logit_threshold``) and swept by greedy NMS; the kept boxes of all levels are
    merged by (logit descending, level, anchor index) and the first ``post_nms_top_n`` written.

    Returns padded ``(boxes [N, post, 4], logits [N, post] (-inf), levels int32 [N, post] (-1),
    anchor_idx int32 [N, post] (-1), count int32 [N], rois [N*post, 5])``; a padding row of
    ``rois`` is (-1, 0, 0, 0, 0), which ``multiscale_roi_align`` / ``roi_align`` pool to zeros.

    A hot-path op: nothing is converted; a wrong dtype, shape, device or a strided view raises
    RuntimeError naming the argument before any launch.  ``out``: the six outputs, caller-owned;
    ``workspace``: a uint8 device tensor of at least the cached size."""
    op = "propose_multilevel"
    lib = _lib.load()
    L, N, K, levels, pre, post = key0 = _fpn_shape_key(op, objectness, strides, pre_nms_top_n, post_nms_top_n)
    if not isinstance(deltas, (list, tuple)) or len(deltas) != L:
        raise RuntimeError(f"{op}: deltas must list one tensor per level ({L})")
    if not isinstance(anchor_bases, (list, tuple)) or len(anchor_bases) != L:
        raise RuntimeError(f"{op}: anchor_bases must list one tensor per level ({L})")
    code = _lib.prediction_dtype_code(op, [(f"objectness[{l}]", t) for l, t in enumerate(objectness)] +
                                      [(f"deltas[{l}]", t) for l, t in enumerate(deltas)])
    dt = objectness[0].dtype
    dev = objectness[0].device
    for l, (H, W, _, _) in enumerate(levels):
        _fpn_tensor(f"objectness[{l}]", objectness[l], dt, (N, K, H, W))
        _fpn_tensor(f"deltas[{l}]", deltas[l], dt, (N, 4 * K, H, W))
        _fpn_tensor(f"anchor_bases[{l}]", anchor_bases[l], torch.float32, (K, 4))
    if isinstance(image_sizes, torch.Tensor):
        _fpn_tensor("image_sizes", image_sizes, torch.float32, (N, 2))
        sizes = image_sizes
    else:
        try:
            hw = (float(image_sizes[0]), float(image_sizes[1]))
            if len(image_sizes) != 2:
                raise ValueError
        except (TypeError, ValueError, IndexError):
            raise RuntimeError(f"{op}: image_sizes must be an fp32 device tensor [N, 2] of (h, w) or one host "
                               f"(h, w); got {image_sizes!r}") from None
        skey = (hw, N, dev.index)
        sizes = _fpn_sizes_cache.get(skey)
        if sizes is None:
            sizes = torch.tensor([hw] * N, dtype=torch.float32).to(dev)
            _fpn_sizes_cache[skey] = sizes
    cached = _fpn_cache.get(key0)
    if cached is None:
        Hs = (_lib.I32 * L)(*[v[0] for v in levels])
        Ws = (_lib.I32 * L)(*[v[1] for v in levels])
        shs = (_lib.I32 * L)(*[v[2] for v in levels])
        sws = (_lib.I32 * L)(*[v[3] for v in levels])
        need = int(lib.frcnn_propose_multi_workspace_size(L, N, K, Hs, Ws, pre, post))
        if need == 0:
            raise RuntimeError(f"{op}: {lib.frcnn_last_error().decode()}")
        cached = (Hs, Ws, shs, sws, need)
        _fpn_cache[key0] = cached
    Hs, Ws, shs, sws, need = cached
    shapes = (((N, post, 4), torch.float32, "boxes"), ((N, post), torch.float32, "logits"),
              ((N, post), torch.int32, "levels"), ((N, post), torch.int32, "anchor_idx"),
              ((N,), torch.int32, "count"), ((N * post, 5), torch.float32, "rois"))
    if out is None:
        outs = tuple(torch.empty(s, dtype=d, device=dev) for s, d, _ in shapes)
    else:
        if not isinstance(out, (list, tuple)) or len(out) != 6:
            raise RuntimeError(f"{op}: out must be the six outputs (boxes, logits, levels, anchor_idx, count, rois)")
        outs = tuple(out)
        for i, (s, d, nm) in enumerate(shapes):
            _fpn_tensor(f"out[{i}] ({nm})", outs[i], d, s)
    ws = workspace if workspace is not None else _lib.cached_workspace("propose_multilevel", need, dev)
    if (not isinstance(ws, torch.Tensor) or not ws.is_cuda or ws.dtype != torch.uint8 or not ws.is_contiguous()
            or ws.numel() < need):
        raise RuntimeError(f"{op}: workspace must be a contiguous uint8 device tensor of at least {need} B")
    P = _lib.P
    _lib.check(lib.frcnn_propose_multi_t(code, L, (P * L)(*[t.data_ptr() for t in objectness]),
                                         (P * L)(*[t.data_ptr() for t in deltas]),
                                         (P * L)(*[t.data_ptr() for t in anchor_bases]), Hs, Ws, shs, sws, N, K,
                                         _lib.ptr(sizes), pre, post, float(nms_thresh), logit_threshold(score_thresh),
                                         float(min_size), *[_lib.ptr(t) for t in outs], _lib.ptr(ws), ws.numel(),
                                         _lib.stream_ptr()), op)
    return outs


# ------------------------------------------------------- pyramid RPN training
RPN_TARGETS_MAX_G, RPN_TARGETS_MAX_BATCH = 256, 1024
RPNTargets = collections.namedtuple("RPNTargets", "matches sampled samples n_pos n_neg reg_targets")
_rpnt_cache = {}   # shape key -> (H, W, stride_h, stride_w host arrays, A, workspace bytes)
_rpnl_ws = {}      # (N, B) -> workspace bytes of the losses' forward


def sampler_state(seed: int, device=None) -> torch.Tensor:
    """The sampler's state for ``rpn_targets_multilevel``: an int64 device tensor ``(seed, calls)``
    with ``calls = 0``.  The op reads it on the device and adds 1 to ``calls``, so every call --
    a replayed graph included -- draws a fresh sample with nothing passed from the host."""
    seed = int(seed)
    if not -(1 << 63) <= seed < (1 << 64):
        raise RuntimeError(f"sampler_state: seed must fit 64 bits; got {seed}")
    if seed >= 1 << 63:
        seed -= 1 << 64
    return torch.tensor([seed, 0], dtype=torch.int64).to(device if device is not None else _lib.device())


def _rpnt_device(op, name, t):
    """The device every tensor of one call shares: that of its first tensor, which must be the
    current device (the kernels launch on its current stream)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        got = f"{t.dtype} {t.device.type} tensor" if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"{op}: {name} must be a device tensor; got a {got}")
    if t.device.index != _lib._cur_device():
        raise RuntimeError(f"{op}: {name} is on {t.device} but the current device is cuda:{_lib._cur_device()}; "
                           "the kernels launch on the current device's stream")
    return t.device


def _rpnt_tensor(op, name, t, dtype, shape, dev=None):
    if isinstance(t, torch.Tensor) and t.is_cuda and dev is not None and t.device != dev:
        raise RuntimeError(f"{op}: {name} is on {t.device} but the call's tensors are on {dev}; every tensor of one "
                           "call lives on one device")
    if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous()
            or tuple(t.shape) != tuple(shape)):
        got = (f"{'contiguous' if t.is_contiguous() else 'strided'} {t.dtype} {t.device.type} tensor of shape "
               f"{list(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__)
        raise RuntimeError(f"{op}: {name} must be a contiguous {dtype} device tensor of shape {list(shape)}; "
                           f"got a {got}")


def _rpnt_levels(op, K, strides, grid_sizes):
    """((H, W, stride_h, stride_w), ...) and A with the limits checked."""
    if not isinstance(grid_sizes, (list, tuple)) or not 1 <= len(grid_sizes) <= FPN_MAX_LEVELS:
        raise RuntimeError(f"{op}: grid_sizes must list 1 to {FPN_MAX_LEVELS} (H, W) pairs")
    L = len(grid_sizes)
    if not isinstance(strides, (list, tuple)) or len(strides) != L:
        raise RuntimeError(f"{op}: strides must list one (stride_h, stride_w) per level ({L})")
    if not 1 <= K <= FPN_MAX_K:
        raise RuntimeError(f"{op}: anchor_bases: K must be in [1, {FPN_MAX_K}]; got {K}")
    levels, A = [], 0
    for l, (hw, s) in enumerate(zip(grid_sizes, strides)):
        try:
            H, W = int(hw[0]), int(hw[1])
        except (TypeError, ValueError, IndexError):
            raise RuntimeError(f"{op}: grid_sizes[{l}] must be (H, W) ints; got {hw!r}") from None
        try:
            sh, sw = int(s[0]), int(s[1])
        except (TypeError, ValueError, IndexError):
            raise RuntimeError(f"{op}: strides[{l}] must be (stride_h, stride_w) ints; got {s!r}") from None
        if H < 1 or W < 1 or K * H * W >= 1 << 24:
            raise RuntimeError(f"{op}: grid_sizes[{l}] = {(H, W)}: H, W >= 1 and K*H*W < 2^24 are required")
        if sh < 1 or sw < 1 or (H - 1) * sh >= 1 << 24 or (W - 1) * sw >= 1 << 24:
            raise RuntimeError(f"{op}: strides[{l}] = {(sh, sw)}: strides >= 1 and (H-1)*stride_h, (W-1)*stride_w "
                               "below 2^24 are required")
        levels.append((H, W, sh, sw))
        A += K * H * W
    if A >= 1 << 31:
        raise RuntimeError(f"{op}: grid_sizes: {A} anchors in all; A must be below 2^31")
    return tuple(levels), A


def _rpnt_arrays(levels):
    L = len(levels)
    return tuple((_lib.I32 * L)(*[v[i] for v in levels]) for i in range(4))


def rpn_targets_multilevel_kernel(K, grid_sizes, N=1, G=1, batch_size_per_image=256, _key_bits=32) -> str:
    """frcnn_rpn_targets_multi_kernel: the kernels a call of this shape launches, with the
    part of the launch plan that the shape fixes (workgroups per image, the last one's anchors,
    the boundary-bucket keys the selection sorts in LDS, the key digits its radix passes refine
    beyond that, the 4096-anchor steps of one of its sweeps).  Host only."""
    lib = _lib.load(require_gpu=False)
    L = len(grid_sizes)
    H = (_lib.I32 * L)(*[int(s[0]) for s in grid_sizes])
    W = (_lib.I32 * L)(*[int(s[1]) for s in grid_sizes])
    buf = _lib.ctypes.create_string_buffer(256)
    _lib.check(lib.frcnn_rpn_targets_multi_kernel(L, int(N), int(K), H, W, int(G), int(batch_size_per_image),
                                                  int(_key_bits), buf, 256), "rpn_targets_multi_kernel")
    return buf.value.decode()


def rpn_targets_multilevel(gt_boxes, gt_count, anchor_bases, strides, grid_sizes, rng, *,
                           batch_size_per_image: int = 256, positive_fraction: float = 0.5,
                           fg_iou_thresh: float = 0.7, bg_iou_thresh: float = 0.3,
                           allow_low_quality_matches: bool = True, out=None, workspace=None, _key_bits: int = 32):
    """The training targets of a pyramid RPN: torchvision's ``assign_targets_to_anchors``
    (``box_iou``, ``Matcher(fg, bg, allow_low_quality_matches)``), ``BalancedPositiveNegativeSampler``
    and ``BoxCoder.encode`` with weights (1, 1, 1, 1) for the whole batch and pyramid, five
    launches, no host synchronisation (frcnn_rpn_targets_multi; DESIGN.md §3 "Pyramid RPN
    training" is the contract).

    ``gt_boxes``: fp32 device tensor [N, G, 4] of (x1, y1, x2, y2); ``gt_count``: int32 device
    tensor [N], rows past it are padding (clamped to [0, G]); ``anchor_bases``, ``strides``,
    ``grid_sizes``: as ``pyramid_anchors`` takes them, the bases on the device -- the anchors are
    formed in registers, global index ``off_l + (y*W_l + x)*K + k``, the row order of
    ``torch.cat(pyramid_anchors(...))``; ``rng``: ``sampler_state(seed)``, read on the device and
    advanced by the call.

    A gt row that is not finite or has no positive width and height is treated as absent.  The
    sample is the ``num_pos`` positives and ``num_neg`` negatives with the smallest (Philox key,
    anchor index): exact, reproducible from ``rng``, the same bits on every call.

    Returns ``RPNTargets(matches int32 [N, A] (-1 below bg, -2 between, else the gt index),
    sampled int32 [N, A] (1 / 0 / -1), samples int32 [N, B] (positives ascending, negatives
    ascending, -1), n_pos, n_neg int32 [N], reg_targets fp32 [N, B, 4])``.

    A hot-path op: nothing is converted; a wrong dtype, shape, device or a strided view raises
    RuntimeError naming the argument before any launch.  Every tensor of a call -- inputs, bases,
    ``rng``, ``out``, ``workspace`` -- lives on one device, the current one (the kernels launch on
    its current stream).  ``out``: the six outputs, caller-owned;
    ``workspace``: a uint8 device tensor of at least the cached size.  ``_key_bits`` (a test knob)
    keeps only that many top bits of every key: with 0 every key ties and the sample is the
    first candidates by index."""
    op = "rpn_targets_multilevel"
    lib = _lib.load()
    if not isinstance(gt_boxes, torch.Tensor) or gt_boxes.dim() != 3:
        raise RuntimeError(f"{op}: gt_boxes must be an fp32 device tensor of shape [N, G, 4]")
    N, G = int(gt_boxes.shape[0]), int(gt_boxes.shape[1])
    if not 1 <= N <= FPN_MAX_N:
        raise RuntimeError(f"{op}: gt_boxes: N must be in [1, {FPN_MAX_N}]; got {N}")
    if not 1 <= G <= RPN_TARGETS_MAX_G:
        raise RuntimeError(f"{op}: gt_boxes: G must be in [1, {RPN_TARGETS_MAX_G}]; got {G}")
    _rpnt_tensor(op, "gt_boxes", gt_boxes, torch.float32, (N, G, 4))
    dev = _rpnt_device(op, "gt_boxes", gt_boxes)
    _rpnt_tensor(op, "gt_count", gt_count, torch.int32, (N,), dev)
    _rpnt_tensor(op, "rng", rng, torch.int64, (2,), dev)
    if not isinstance(anchor_bases, (list, tuple)) or not 1 <= len(anchor_bases) <= FPN_MAX_LEVELS:
        raise RuntimeError(f"{op}: anchor_bases must be a list of 1 to {FPN_MAX_LEVELS} fp32 device tensors [K, 4]")
    b0 = anchor_bases[0]
    if not isinstance(b0, torch.Tensor) or b0.dim() != 2:
        raise RuntimeError(f"{op}: anchor_bases[0] must be an fp32 device tensor of shape [K, 4]")
    K = int(b0.shape[0])
    B = int(batch_size_per_image)
    if not 1 <= B <= RPN_TARGETS_MAX_BATCH:
        raise RuntimeError(f"{op}: batch_size_per_image must be in [1, {RPN_TARGETS_MAX_BATCH}]; got {B}")
    frac, fg, bg = float(positive_fraction), float(fg_iou_thresh), float(bg_iou_thresh)
    if not 0.0 <= frac <= 1.0:
        raise RuntimeError(f"{op}: positive_fraction must be in [0, 1]; got {frac}")
    if not bg <= fg:
        raise RuntimeError(f"{op}: bg_iou_thresh = {bg} must not exceed fg_iou_thresh = {fg}")
    kb = int(_key_bits)
    if not 0 <= kb <= 32:
        raise RuntimeError(f"{op}: _key_bits must be in [0, 32]; got {kb}")
    try:
        key0 = (K, tuple(tuple(int(v) for v in s) for s in strides), tuple(tuple(int(v) for v in s) for s in grid_sizes),
                N, G, B)
    except (TypeError, ValueError):
        _rpnt_levels(op, K, strides, grid_sizes)   # raises, naming the argument
        raise RuntimeError(f"{op}: strides and grid_sizes must list (stride_h, stride_w) / (H, W) ints") from None
    cached = _rpnt_cache.get(key0)
    if cached is None:
        levels, A = _rpnt_levels(op, K, strides, grid_sizes)
        arrays = _rpnt_arrays(levels)
        need = int(lib.frcnn_rpn_targets_multi_workspace_size(len(levels), N, K, arrays[0], arrays[1], G, B))
        if need == 0:
            raise RuntimeError(f"{op}: {lib.frcnn_last_error().decode()}")
        cached = _rpnt_cache[key0] = arrays + (A, need)
    Hs, Ws, shs, sws, A, need = cached
    L = len(Hs)
    if len(anchor_bases) != L:
        raise RuntimeError(f"{op}: anchor_bases must list one tensor per level ({L})")
    for l in range(L):
        _rpnt_tensor(op, f"anchor_bases[{l}]", anchor_bases[l], torch.float32, (K, 4), dev)
    shapes = (((N, A), torch.int32, "matches"), ((N, A), torch.int32, "sampled"), ((N, B), torch.int32, "samples"),
              ((N,), torch.int32, "n_pos"), ((N,), torch.int32, "n_neg"), ((N, B, 4), torch.float32, "reg_targets"))
    if out is None:
        outs = tuple(torch.empty(s, dtype=d, device=dev) for s, d, _ in shapes)
    else:
        if not isinstance(out, (list, tuple)) or len(out) != 6:
            raise RuntimeError(f"{op}: out must be the six outputs (matches, sampled, samples, n_pos, n_neg, "
                               "reg_targets)")
        outs = tuple(out)
        for i, (s, d, nm) in enumerate(shapes):
            _rpnt_tensor(op, f"out[{i}] ({nm})", outs[i], d, s, dev)
    ws = workspace if workspace is not None else _lib.cached_workspace(op, need, dev)
    if (not isinstance(ws, torch.Tensor) or not ws.is_cuda or ws.dtype != torch.uint8 or not ws.is_contiguous()
            or ws.numel() < need or ws.device != dev):
        raise RuntimeError(f"{op}: workspace must be a contiguous uint8 tensor of at least {need} B on {dev}")
    P = _lib.P
    _lib.check(lib.frcnn_rpn_targets_multi(L, (P * L)(*[t.data_ptr() for t in anchor_bases]), Hs, Ws, shs, sws, N, K,
                                           _lib.ptr(gt_boxes), _lib.ptr(gt_count), G, _lib.ptr(rng), B, frac, fg, bg,
                                           int(bool(allow_low_quality_matches)), kb, *[_lib.ptr(t) for t in outs],
                                           _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), op)
    return RPNTargets(*outs)


class _RPNLossesMultiFunction(torch.autograd.Function):
    """frcnn_rpn_losses_multi_fwd_t / _bwd_t.  ``args`` = the L objectness maps, then the L
    deltas maps; the backward hands the incoming gradients to the kernel as device pointers
    (an unused loss: None -> NULL -> that gradient all zero)."""

    @staticmethod
    def forward(ctx, targets, beta, code, L, *maps):
        lib = _lib.load()
        obj, dl = maps[:L], maps[L:]
        N, K = obj[0].shape[0], obj[0].shape[1]
        B = targets.samples.shape[1]
        dev = obj[0].device
        Hs = (_lib.I32 * L)(*[t.shape[2] for t in obj])
        Ws = (_lib.I32 * L)(*[t.shape[3] for t in obj])
        need = _rpnl_ws.get((N, B))
        if need is None:
            need = _rpnl_ws[(N, B)] = int(lib.frcnn_rpn_losses_multi_workspace_size(N, B))
        ws = _lib.cached_workspace("rpn_losses_multilevel", need, dev)
        loss = torch.empty(2, dtype=torch.float32, device=dev)
        stats = torch.empty(2, dtype=torch.int32, device=dev)
        P = _lib.P
        po, pd = (P * L)(*[t.data_ptr() for t in obj]), (P * L)(*[t.data_ptr() for t in dl])
        _lib.check(lib.frcnn_rpn_losses_multi_fwd_t(code, L, po, pd, Hs, Ws, N, K, B, _lib.ptr(targets.samples),
                                                    _lib.ptr(targets.n_pos), _lib.ptr(targets.n_neg),
                                                    _lib.ptr(targets.reg_targets), beta, _lib.ptr(loss),
                                                    _lib.ptr(stats), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                   "rpn_losses_multilevel forward")
        ctx.save_for_backward(*maps, targets.sampled, targets.samples, targets.n_pos, targets.reg_targets, stats)
        ctx.meta = (beta, code, L, N, K, B, Hs, Ws)
        ctx.set_materialize_grads(False)
        return loss[0], loss[1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_obj, g_box):
        lib = _lib.load()
        beta, code, L, N, K, B, Hs, Ws = ctx.meta
        saved = ctx.saved_tensors
        maps = saved[:2 * L]
        sampled, samples, n_pos, reg_t, stats = saved[2 * L:]
        for name, g in (("objectness_loss", g_obj), ("box_loss", g_box)):
            if g is not None and (g.dtype != torch.float32 or not g.is_cuda or g.numel() != 1):
                raise RuntimeError(f"rpn_losses_multilevel backward: the gradient of {name} must be one torch.float32 "
                                   f"on the device; got {g.dtype} on {g.device.type} with {g.numel()} elements")
        grads = [torch.empty_like(t) for t in maps]   # contiguous, the inputs' dtype: each element is stored once
        P = _lib.P
        _lib.check(lib.frcnn_rpn_losses_multi_bwd_t(code, L, (P * L)(*[t.data_ptr() for t in maps[:L]]),
                                                    (P * L)(*[t.data_ptr() for t in maps[L:]]), Hs, Ws, N, K, B,
                                                    _lib.ptr(sampled), _lib.ptr(samples), _lib.ptr(n_pos),
                                                    _lib.ptr(reg_t), beta, _lib.ptr(stats), _lib.ptr(g_obj),
                                                    _lib.ptr(g_box), (P * L)(*[t.data_ptr() for t in grads[:L]]),
                                                    (P * L)(*[t.data_ptr() for t in grads[L:]]), _lib.stream_ptr()),
                   "rpn_losses_multilevel backward")
        return (None, None, None, None, *grads)


def rpn_losses_multilevel(objectness, deltas, targets, *, beta: float = 1 / 9):
    """torchvision's ``RegionProposalNetwork.compute_loss`` on ``rpn_targets_multilevel``'s
    result, differentiable with respect to every tensor of ``objectness`` and ``deltas``
    (frcnn_rpn_losses_multi_fwd_t / _bwd_t; DESIGN.md §3 "Pyramid RPN training").

    ``objectness``: L tensors [N, K, H_l, W_l]; ``deltas``: L tensors [N, 4K, H_l, W_l] (channel
    4k + c) -- the lists ``propose_multilevel`` reads, contiguous, all fp32, float16 or bfloat16,
    read in place; ``targets``: the ``RPNTargets`` of the same pyramid.  Returns
    ``(objectness_loss, box_loss)``, 0-dim fp32 device tensors: the mean over the S sampled
    anchors of the binary cross-entropy with logits, and the smooth-L1 (``beta``) sum over the
    sampled positives divided by S.  S == 0 gives NaN and zero gradients.

    The forward reads the S samples only; the backward writes every level's gradient in full,
    each element once, in the inputs' dtype, with no atomics: the same bits on every call.
    Nothing is converted and nothing synchronises; a wrong dtype, shape, device or a strided view
    raises RuntimeError naming the argument before any launch, and so does a tensor -- of the maps or
    of ``targets`` -- that is not on ``objectness[0]``'s device, which must be the current one."""
    op = "rpn_losses_multilevel"
    _lib.load()
    if not isinstance(objectness, (list, tuple)) or not 1 <= len(objectness) <= FPN_MAX_LEVELS:
        raise RuntimeError(f"{op}: objectness must be a list of 1 to {FPN_MAX_LEVELS} tensors [N, K, H, W]")
    L = len(objectness)
    if not isinstance(deltas, (list, tuple)) or len(deltas) != L:
        raise RuntimeError(f"{op}: deltas must list one tensor per level ({L})")
    if not isinstance(targets, RPNTargets):
        raise RuntimeError(f"{op}: targets must be the RPNTargets of rpn_targets_multilevel; got "
                           f"{type(targets).__name__}")
    code = _lib.prediction_dtype_code(op, [(f"objectness[{l}]", t) for l, t in enumerate(objectness)] +
                                      [(f"deltas[{l}]", t) for l, t in enumerate(deltas)])
    o0 = objectness[0]
    if o0.dim() != 4:
        raise RuntimeError(f"{op}: objectness[0] must be a device tensor of shape [N, K, H, W]")
    N, K = int(o0.shape[0]), int(o0.shape[1])
    if not 1 <= N <= FPN_MAX_N:
        raise RuntimeError(f"{op}: objectness: N must be in [1, {FPN_MAX_N}]; got {N}")
    if not 1 <= K <= FPN_MAX_K:
        raise RuntimeError(f"{op}: objectness: K must be in [1, {FPN_MAX_K}]; got {K}")
    dev = _rpnt_device(op, "objectness[0]", o0)
    A = 0
    for l, o in enumerate(objectness):
        if o.dim() != 4:
            raise RuntimeError(f"{op}: objectness[{l}] must be a device tensor of shape [N, K, H, W]")
        H, W = int(o.shape[2]), int(o.shape[3])
        if H < 1 or W < 1 or K * H * W >= 1 << 24:
            raise RuntimeError(f"{op}: objectness[{l}]: H, W >= 1 and K*H*W < 2^24 are required; got {list(o.shape)}")
        _rpnt_tensor(op, f"objectness[{l}]", o, o0.dtype, (N, K, H, W), dev)
        _rpnt_tensor(op, f"deltas[{l}]", deltas[l], o0.dtype, (N, 4 * K, H, W), dev)
        A += K * H * W
    if targets.samples.dim() != 2:
        raise RuntimeError(f"{op}: targets.samples must be an int32 device tensor of shape [N, B]")
    B = int(targets.samples.shape[1])
    if not 1 <= B <= RPN_TARGETS_MAX_BATCH:
        raise RuntimeError(f"{op}: targets.samples: B must be in [1, {RPN_TARGETS_MAX_BATCH}]; got {B}")
    _rpnt_tensor(op, "targets.sampled", targets.sampled, torch.int32, (N, A), dev)
    _rpnt_tensor(op, "targets.samples", targets.samples, torch.int32, (N, B), dev)
    _rpnt_tensor(op, "targets.n_pos", targets.n_pos, torch.int32, (N,), dev)
    _rpnt_tensor(op, "targets.n_neg", targets.n_neg, torch.int32, (N,), dev)
    _rpnt_tensor(op, "targets.reg_targets", targets.reg_targets, torch.float32, (N, B, 4), dev)
    beta = float(beta)
    if not 0.0 <= beta < float("inf"):
        raise RuntimeError(f"{op}: beta={beta} must be finite and not negative")
    return _RPNLossesMultiFunction.apply(targets, beta, code, L, *objectness, *deltas)


# ------------------------------------------------- pyramid box-head training
BOX_HEAD_MAX_R, BOX_HEAD_MAX_C = 4096, 128
BoxHeadTargets = collections.namedtuple("BoxHeadTargets", "rois labels matched reg_targets samples n_pos n_neg matches")
_bht_ws = {}   # (N, R, G, B) -> workspace bytes of the targets
_bhl_ws = {}   # (N, B) -> workspace bytes of the losses' forward


def box_head_targets_kernel(R, G, N=1, batch_size_per_image=512, _key_bits=32) -> str:
    """frcnn_box_head_targets_kernel: the kernels a call of this shape launches, with the part
    of the launch plan that the shape fixes (M = R + G, the match kernel's workgroups per image and
    the candidates of the last one, the candidates per thread of the sample kernel's slot scan,
    the digits its selection may walk).  Host only."""
    lib = _lib.load(require_gpu=False)
    buf = _lib.ctypes.create_string_buffer(256)
    _lib.check(lib.frcnn_box_head_targets_kernel(int(N), int(R), int(G), int(batch_size_per_image), int(_key_bits), buf,
                                                 256), "box_head_targets_kernel")
    return buf.value.decode()


def box_head_targets(proposals, prop_count, gt_boxes, gt_labels, gt_count, rng, *, batch_size_per_image: int = 512,
                     positive_fraction: float = 0.25, fg_iou_thresh: float = 0.5, bg_iou_thresh: float = 0.5,
                     reg_weights=(10.0, 10.0, 5.0, 5.0), add_gt: bool = True, out=None, workspace=None,
                     _key_bits: int = 32):
    """The training samples of a box head: torchvision's ``RoIHeads.select_training_samples``
    (``add_gt_proposals``, ``box_iou``, ``Matcher(fg, bg, allow_low_quality_matches=False)``,
    ``assign_targets_to_proposals``, ``BalancedPositiveNegativeSampler``, ``BoxCoder.encode`` with
    ``reg_weights``) for the whole batch, two launches, no host synchronisation
    (frcnn_box_head_targets; DESIGN.md §3 "Pyramid box-head training" is the contract).

    ``proposals``: fp32 device tensor [N, R, 4] of (x1, y1, x2, y2) and ``prop_count``: int32
    [N] -- ``propose_multilevel``'s ``boxes`` and ``count``; ``gt_boxes`` fp32 [N, G, 4],
    ``gt_labels`` int32 [N, G], ``gt_count`` int32 [N] (counts are clamped); ``rng``:
    ``sampler_state(seed)``, read on the device and advanced by the call.

    An image's candidates are its proposals below ``prop_count`` (index c) and, with ``add_gt``,
    its present gt rows (index R + g; a row that is not finite or has no positive width and
    height is absent).  The sample is the ``num_pos`` positives (label >= 1) and ``num_neg``
    negatives (label 0) with the smallest (Philox key, index): exact, reproducible from ``rng``.

    Returns ``BoxHeadTargets(rois fp32 [N*B, 5] (n, x1, y1, x2, y2), labels int32 [N, B],
    matched int32 [N, B] (the gt index; 0 for a negative), reg_targets fp32 [N, B, 4] (0 for a
    negative), samples int32 [N, B] (candidate indices), n_pos, n_neg int32 [N], matches int32
    [N, R + G] (-1 below bg, -2 between, else the gt index, -3 absent))``.  The sampled
    candidates fill an image's slots in ascending index order; the padding behind them is
    ``rois`` (-1, 0, 0, 0, 0) -- a row ``multiscale_roi_align`` pools to zeros -- labels, matched
    and samples -1, reg_targets 0.

    A hot-path op: nothing is converted; a wrong dtype, shape, device or a strided view raises
    RuntimeError naming the argument before any launch.  Every tensor of a call lives on the
    current device.  ``out``: the eight outputs, caller-owned; ``workspace``: a uint8 device
    tensor of at least the cached size.  ``_key_bits`` (a test knob) keeps only that many top
    bits of every key."""
    op = "box_head_targets"
    lib = _lib.load()
    if not isinstance(proposals, torch.Tensor) or proposals.dim() != 3:
        raise RuntimeError(f"{op}: proposals must be an fp32 device tensor of shape [N, R, 4]")
    N, R = int(proposals.shape[0]), int(proposals.shape[1])
    if not 1 <= N <= FPN_MAX_N:
        raise RuntimeError(f"{op}: proposals: N must be in [1, {FPN_MAX_N}]; got {N}")
    if not 1 <= R <= BOX_HEAD_MAX_R:
        raise RuntimeError(f"{op}: proposals: R must be in [1, {BOX_HEAD_MAX_R}]; got {R}")
    _rpnt_tensor(op, "proposals", proposals, torch.float32, (N, R, 4))
    dev = _rpnt_device(op, "proposals", proposals)
    _rpnt_tensor(op, "prop_count", prop_count, torch.int32, (N,), dev)
    if not isinstance(gt_boxes, torch.Tensor) or gt_boxes.dim() != 3:
        raise RuntimeError(f"{op}: gt_boxes must be an fp32 device tensor of shape [N, G, 4]")
    G = int(gt_boxes.shape[1])
    if not 1 <= G <= RPN_TARGETS_MAX_G:
        raise RuntimeError(f"{op}: gt_boxes: G must be in [1, {RPN_TARGETS_MAX_G}]; got {G}")
    _rpnt_tensor(op, "gt_boxes", gt_boxes, torch.float32, (N, G, 4), dev)
    _rpnt_tensor(op, "gt_labels", gt_labels, torch.int32, (N, G), dev)
    _rpnt_tensor(op, "gt_count", gt_count, torch.int32, (N,), dev)
    _rpnt_tensor(op, "rng", rng, torch.int64, (2,), dev)
    B = int(batch_size_per_image)
    if not 1 <= B <= RPN_TARGETS_MAX_BATCH:
        raise RuntimeError(f"{op}: batch_size_per_image must be in [1, {RPN_TARGETS_MAX_BATCH}]; got {B}")
    frac, fg, bg = float(positive_fraction), float(fg_iou_thresh), float(bg_iou_thresh)
    if not 0.0 <= frac <= 1.0:
        raise RuntimeError(f"{op}: positive_fraction must be in [0, 1]; got {frac}")
    if not bg <= fg:
        raise RuntimeError(f"{op}: bg_iou_thresh = {bg} must not exceed fg_iou_thresh = {fg}")
    try:
        wts = tuple(float(w) for w in reg_weights)
    except (TypeError, ValueError):
        wts = ()
    if len(wts) != 4 or not all(0.0 < w < float("inf") for w in wts):
        raise RuntimeError(f"{op}: reg_weights must be four finite positive numbers; got {reg_weights!r}")
    kb = int(_key_bits)
    if not 0 <= kb <= 32:
        raise RuntimeError(f"{op}: _key_bits must be in [0, 32]; got {kb}")
    need = _bht_ws.get((N, R, G, B))
    if need is None:
        need = int(lib.frcnn_box_head_targets_workspace_size(N, R, G, B))
        if need == 0:
            raise RuntimeError(f"{op}: {lib.frcnn_last_error().decode()}")
        _bht_ws[(N, R, G, B)] = need
    i32, f32 = torch.int32, torch.float32
    shapes = (((N * B, 5), f32, "rois"), ((N, B), i32, "labels"), ((N, B), i32, "matched"),
              ((N, B, 4), f32, "reg_targets"), ((N, B), i32, "samples"), ((N,), i32, "n_pos"), ((N,), i32, "n_neg"),
              ((N, R + G), i32, "matches"))
    if out is None:
        outs = tuple(torch.empty(s, dtype=d, device=dev) for s, d, _ in shapes)
    else:
        if not isinstance(out, (list, tuple)) or len(out) != 8:
            raise RuntimeError(f"{op}: out must be the eight outputs (rois, labels, matched, reg_targets, samples, "
                               "n_pos, n_neg, matches)")
        outs = tuple(out)
        for i, (s, d, nm) in enumerate(shapes):
            _rpnt_tensor(op, f"out[{i}] ({nm})", outs[i], d, s, dev)
    ws = workspace if workspace is not None else _lib.cached_workspace(op, need, dev)
    if (not isinstance(ws, torch.Tensor) or not ws.is_cuda or ws.dtype != torch.uint8 or not ws.is_contiguous()
            or ws.numel() < need or ws.device != dev):
        raise RuntimeError(f"{op}: workspace must be a contiguous uint8 tensor of at least {need} B on {dev}")
    _lib.check(lib.frcnn_box_head_targets(_lib.ptr(proposals), _lib.ptr(prop_count), N, R, _lib.ptr(gt_boxes),
                                          _lib.ptr(gt_labels), _lib.ptr(gt_count), G, _lib.ptr(rng), B, frac, fg, bg,
                                          *wts, int(bool(add_gt)), kb, *[_lib.ptr(t) for t in outs], _lib.ptr(ws),
                                          ws.numel(), _lib.stream_ptr()), op)
    return BoxHeadTargets(*outs)


class _BoxHeadLossesFunction(torch.autograd.Function):
    """frcnn_box_head_losses_fwd_t / _bwd_t; the backward hands the incoming gradients to the
    kernel as device pointers (an unused loss: None -> NULL -> that gradient all zero)."""

    @staticmethod
    def forward(ctx, targets, beta, code, cls, reg):
        lib = _lib.load()
        N, B = targets.labels.shape
        C = cls.shape[1]
        dev = cls.device
        need = _bhl_ws.get((N, B))
        if need is None:
            need = _bhl_ws[(N, B)] = int(lib.frcnn_box_head_losses_workspace_size(N, B))
        ws = _lib.cached_workspace("box_head_losses", need, dev)
        loss = torch.empty(2, dtype=torch.float32, device=dev)
        stats = torch.empty(4, dtype=torch.int32, device=dev)
        _lib.check(lib.frcnn_box_head_losses_fwd_t(code, _lib.ptr(cls), _lib.ptr(reg), N, B, C, _lib.ptr(targets.labels),
                                                   _lib.ptr(targets.reg_targets), _lib.ptr(targets.n_pos),
                                                   _lib.ptr(targets.n_neg), beta, _lib.ptr(loss), _lib.ptr(stats),
                                                   _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                   "box_head_losses forward")
        ctx.save_for_backward(cls, reg, targets.labels, targets.reg_targets, targets.n_pos, targets.n_neg, stats)
        ctx.meta = (beta, code, N, B, C)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(stats)
        return loss[0], loss[1], stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_cls, g_box, _g_stats):
        lib = _lib.load()
        beta, code, N, B, C = ctx.meta
        cls, reg, labels, reg_t, n_pos, n_neg, stats = ctx.saved_tensors
        for name, g in (("classification_loss", g_cls), ("box_loss", g_box)):
            if g is not None and (g.dtype != torch.float32 or not g.is_cuda or g.numel() != 1):
                raise RuntimeError(f"box_head_losses backward: the gradient of {name} must be one torch.float32 on "
                                   f"the device; got {g.dtype} on {g.device.type} with {g.numel()} elements")
        dcls, dreg = torch.empty_like(cls), torch.empty_like(reg)   # each element is stored once
        _lib.check(lib.frcnn_box_head_losses_bwd_t(code, _lib.ptr(cls), _lib.ptr(reg), N, B, C, _lib.ptr(labels),
                                                   _lib.ptr(reg_t), _lib.ptr(n_pos), _lib.ptr(n_neg), beta,
                                                   _lib.ptr(stats), _lib.ptr(g_cls), _lib.ptr(g_box), _lib.ptr(dcls),
                                                   _lib.ptr(dreg), _lib.stream_ptr()), "box_head_losses backward")
        return None, None, None, dcls, dreg


def _box_head_losses(class_logits, box_regression, targets, beta):
    op = "box_head_losses"
    _lib.load()
    if not isinstance(targets, BoxHeadTargets):
        raise RuntimeError(f"{op}: targets must be the BoxHeadTargets of box_head_targets; got {type(targets).__name__}")
    code = _lib.prediction_dtype_code(op, (("class_logits", class_logits), ("box_regression", box_regression)))
    if class_logits.dim() != 2:
        raise RuntimeError(f"{op}: class_logits must be a device tensor of shape [N*B, C]")
    rows, C = int(class_logits.shape[0]), int(class_logits.shape[1])
    if not 2 <= C <= BOX_HEAD_MAX_C:
        raise RuntimeError(f"{op}: class_logits: C must be in [2, {BOX_HEAD_MAX_C}]; got {C}")
    dev = _rpnt_device(op, "class_logits", class_logits)
    if not isinstance(targets.labels, torch.Tensor) or targets.labels.dim() != 2:
        raise RuntimeError(f"{op}: targets.labels must be an int32 device tensor of shape [N, B]")
    N, B = int(targets.labels.shape[0]), int(targets.labels.shape[1])
    if not 1 <= N <= FPN_MAX_N:
        raise RuntimeError(f"{op}: targets.labels: N must be in [1, {FPN_MAX_N}]; got {N}")
    if not 1 <= B <= RPN_TARGETS_MAX_BATCH:
        raise RuntimeError(f"{op}: targets.labels: B must be in [1, {RPN_TARGETS_MAX_BATCH}]; got {B}")
    _rpnt_tensor(op, "class_logits", class_logits, class_logits.dtype, (N * B, C), dev)
    _rpnt_tensor(op, "box_regression", box_regression, class_logits.dtype, (N * B, 4 * C), dev)
    _rpnt_tensor(op, "targets.labels", targets.labels, torch.int32, (N, B), dev)
    _rpnt_tensor(op, "targets.reg_targets", targets.reg_targets, torch.float32, (N, B, 4), dev)
    _rpnt_tensor(op, "targets.n_pos", targets.n_pos, torch.int32, (N,), dev)
    _rpnt_tensor(op, "targets.n_neg", targets.n_neg, torch.int32, (N,), dev)
    beta = float(beta)
    if not 0.0 <= beta < float("inf"):
        raise RuntimeError(f"{op}: beta={beta} must be finite and not negative")
    return _BoxHeadLossesFunction.apply(targets, beta, code, class_logits, box_regression)


def box_head_losses(class_logits, box_regression, targets, *, beta: float = 1 / 9):
    """torchvision's ``fastrcnn_loss`` on ``box_head_targets``' result, differentiable with
    respect to both predictions (frcnn_box_head_losses_fwd_t / _bwd_t; DESIGN.md §3 "Pyramid
    box-head training").

    ``class_logits``: [N*B, C]; ``box_regression``: [N*B, 4C] (column 4c + j); both fp32, both
    float16 or both bfloat16, contiguous, row ``n*B + slot`` as ``targets.rois`` orders them.
    Returns ``(classification_loss, box_loss)``, 0-dim fp32 device tensors: the mean over the S
    sampled slots of the cross-entropy, and the smooth-L1 (``beta``) sum over the positives'
    four label columns divided by S.  Padding slots contribute nothing; a sampled slot whose
    label is >= C is skipped and counted (``box_head_losses_with_stats``), never used as an index.
    S == 0 gives NaN and zero gradients.

    The backward stores every element of both gradients once, in the inputs' dtype, with no
    atomics: the same bits on every call.  Nothing is converted and nothing synchronises; a wrong
    dtype, shape, device or a strided view raises RuntimeError naming the argument before any
    launch."""
    return _box_head_losses(class_logits, box_regression, targets, beta)[:2]


def box_head_losses_with_stats(class_logits, box_regression, targets, *, beta: float = 1 / 9):
    """``box_head_losses`` plus ``stats``: int32 device tensor (S, sampled positives, slots
    skipped for a label >= C, 0)."""
    return _box_head_losses(class_logits, box_regression, targets, beta)


# ------------------------------------------------- pyramid box-head inference
BOX_DET_MAX_D = 1024
BoxDetections = collections.namedtuple("BoxDetections", "boxes labels scores roi count total")
_bd_ws = {}   # (N, R, C) -> workspace bytes


def _bd_shape(op, R, C, D):
    R, C, D = int(R), int(C), int(D)
    if not 1 <= R <= BOX_HEAD_MAX_R:
        raise RuntimeError(f"{op}: proposals: R must be in [1, {BOX_HEAD_MAX_R}]; got {R}")
    if not 2 <= C <= BOX_HEAD_MAX_C:
        raise RuntimeError(f"{op}: class_logits: C must be in [2, {BOX_HEAD_MAX_C}]; got {C}")
    if not 1 <= D <= BOX_DET_MAX_D:
        raise RuntimeError(f"{op}: detections_per_img must be in [1, {BOX_DET_MAX_D}]; got {D}")
    return R, C, D


def box_head_detections_kernel(R, C, detections_per_img=100, dtype=torch.float32) -> str:
    """frcnn_box_detections_kernel: the kernels a ``box_head_detections`` call of this shape and
    prediction dtype launches, with the branch of the launch plan ("rows": R <= 1,024, one thread
    per row; "strided" above).  Host only."""
    R, C, D = _bd_shape("box_head_detections_kernel", R, C, detections_per_img)
    lib = _lib.load(require_gpu=False)
    buf = _lib.ctypes.create_string_buffer(256)
    _lib.check(lib.frcnn_box_detections_kernel(_lib.dtype_code(dtype), R, C, D, buf, 256), "box_detections_kernel")
    return buf.value.decode()


def box_head_detections(class_logits, box_regression, proposals, prop_count, image_sizes, *, score_thresh: float = 0.05,
                        nms_thresh: float = 0.5, detections_per_img: int = 100, min_size: float = 1e-2,
                        reg_weights=(10.0, 10.0, 5.0, 5.0), original_sizes=None, out=None, workspace=None):
    """The inference half of a box head on the pyramid path: torchvision's
    ``RoIHeads.postprocess_detections`` (softmax, ``BoxCoder(reg_weights).decode``,
    ``clip_boxes_to_image``, ``score_thresh``, ``remove_small_boxes(min_size)``, class-wise NMS,
    the best ``detections_per_img`` by score) and, with ``original_sizes``,
    ``GeneralizedRCNNTransform.postprocess``'s ``resize_boxes``, for the whole batch: three
    launches, no host synchronisation (frcnn_box_detections_t; DESIGN.md §3 "Pyramid box-head
    inference" is the contract).

    ``class_logits`` [N*R, C] and ``box_regression`` [N*R, 4C]: the head's outputs for
    ``propose_multilevel``'s ``rois`` (row n*R + r is proposal r of image n), both fp32, both
    float16 or both bfloat16, widened exactly inside the kernels; ``proposals`` fp32 [N, R, 4] of
    (x1, y1, x2, y2) and ``prop_count`` int32 [N] -- ``propose_multilevel``'s ``boxes`` and
    ``count`` (clamped; rows past the count are ignored); ``image_sizes``: fp32 device tensor
    [N, 2] of (h, w), or one host (h, w) for every image; ``original_sizes``: fp32 device tensor
    [N, 2] of (h, w), or None.

    Returns ``BoxDetections(boxes fp32 [N, D, 4] (padding 0), labels int32 [N, D] (-1), scores fp32
    [N, D] (0), roi int32 [N, D] (the proposal row; -1), count int32 [N], total int32 [N] (kept
    before the cut to D))``, an image's detections by (score descending, row, class).  The tuple
    feeds ``eval_update`` / ``coco_eval_update`` as it is.

    A hot-path op: nothing is converted; a wrong dtype, shape, device or a strided view raises
    RuntimeError naming the argument before any launch.  ``out``: the six outputs, caller-owned;
    ``workspace``: a uint8 device tensor of at least the cached size."""
    op = "box_head_detections"
    lib = _lib.load()
    code = _lib.prediction_dtype_code(op, (("class_logits", class_logits), ("box_regression", box_regression)))
    if not isinstance(proposals, torch.Tensor) or proposals.dim() != 3:
        raise RuntimeError(f"{op}: proposals must be an fp32 device tensor of shape [N, R, 4]")
    N = int(proposals.shape[0])
    if not 1 <= N <= FPN_MAX_N:
        raise RuntimeError(f"{op}: proposals: N must be in [1, {FPN_MAX_N}]; got {N}")
    if class_logits.dim() != 2:
        raise RuntimeError(f"{op}: class_logits must be a device tensor of shape [N*R, C]; got {list(class_logits.shape)}")
    R, C, D = _bd_shape(op, proposals.shape[1], class_logits.shape[1], detections_per_img)
    dev = _rpnt_device(op, "class_logits", class_logits)
    dt = class_logits.dtype
    _rpnt_tensor(op, "class_logits", class_logits, dt, (N * R, C), dev)
    _rpnt_tensor(op, "box_regression", box_regression, dt, (N * R, 4 * C), dev)
    _rpnt_tensor(op, "proposals", proposals, torch.float32, (N, R, 4), dev)
    _rpnt_tensor(op, "prop_count", prop_count, torch.int32, (N,), dev)
    if isinstance(image_sizes, torch.Tensor):
        _rpnt_tensor(op, "image_sizes", image_sizes, torch.float32, (N, 2), dev)
        sizes = image_sizes
    else:
        try:
            hw = (float(image_sizes[0]), float(image_sizes[1]))
            if len(image_sizes) != 2:
                raise ValueError
        except (TypeError, ValueError, IndexError):
            raise RuntimeError(f"{op}: image_sizes must be an fp32 device tensor [N, 2] of (h, w) or one host "
                               f"(h, w); got {image_sizes!r}") from None
        skey = (hw, N, dev.index)
        sizes = _fpn_sizes_cache.get(skey)
        if sizes is None:
            sizes = torch.tensor([hw] * N, dtype=torch.float32).to(dev)
            _fpn_sizes_cache[skey] = sizes
    if original_sizes is not None:
        _rpnt_tensor(op, "original_sizes", original_sizes, torch.float32, (N, 2), dev)
    try:
        wts = tuple(float(w) for w in reg_weights)
    except (TypeError, ValueError):
        wts = ()
    if len(wts) != 4 or not all(0.0 < w < float("inf") for w in wts):
        raise RuntimeError(f"{op}: reg_weights must be four finite positive numbers; got {reg_weights!r}")
    need = _bd_ws.get((N, R, C))
    if need is None:
        need = int(lib.frcnn_box_detections_workspace_size(N, R, C))
        if need == 0:
            raise RuntimeError(f"{op}: {lib.frcnn_last_error().decode()}")
        _bd_ws[(N, R, C)] = need
    i32, f32 = torch.int32, torch.float32
    shapes = (((N, D, 4), f32, "boxes"), ((N, D), i32, "labels"), ((N, D), f32, "scores"), ((N, D), i32, "roi"),
              ((N,), i32, "count"), ((N,), i32, "total"))
    if out is None:
        outs = tuple(torch.empty(s, dtype=d, device=dev) for s, d, _ in shapes)
    else:
        if not isinstance(out, (list, tuple)) or len(out) != 6:
            raise RuntimeError(f"{op}: out must be the six outputs (boxes, labels, scores, roi, count, total)")
        outs = tuple(out)
        for i, (s, d, nm) in enumerate(shapes):
            _rpnt_tensor(op, f"out[{i}] ({nm})", outs[i], d, s, dev)
    ws = workspace if workspace is not None else _lib.cached_workspace(op, need, dev)
    if (not isinstance(ws, torch.Tensor) or not ws.is_cuda or ws.dtype != torch.uint8 or not ws.is_contiguous()
            or ws.numel() < need or ws.device != dev):
        raise RuntimeError(f"{op}: workspace must be a contiguous uint8 tensor of at least {need} B on {dev}")
    _lib.check(lib.frcnn_box_detections_t(code, N, R, C, _lib.ptr(class_logits), _lib.ptr(box_regression),
                                          _lib.ptr(proposals), _lib.ptr(prop_count), _lib.ptr(sizes),
                                          _lib.ptr(original_sizes), float(score_thresh), float(nms_thresh), D,
                                          float(min_size), *wts, *[_lib.ptr(t) for t in outs], _lib.ptr(ws), ws.numel(),
                                          _lib.stream_ptr()), op)
    return BoxDetections(*outs)


# ------------------------------------------------------- pyramid mask head
MASK_HEAD_MAX_M, MASK_HEAD_MAX_G, MASK_HEAD_MAX_DIM, MASK_HEAD_MAX_PAD = 56, 256, 4096, 4
MaskHeadTargets = collections.namedtuple("MaskHeadTargets", "rois labels matched slot count targets")
_mhl_ws = {}   # (N, P) -> workspace bytes of the losses' forward


def _mh_name(fn, what, *args) -> str:
    buf = _lib.ctypes.create_string_buffer(256)
    _lib.check(fn(*args, buf, 256), what)
    return buf.value.decode()


def mask_head_targets_kernel(B, positives_per_image=None, mask_size=28) -> str:
    """frcnn_mask_targets_kernel: the two kernels a ``mask_head_targets`` call launches and the
    plan branch of the second ("one": M * M <= 256, a thread owns at most one bin; "strided"
    above).  Host only."""
    lib = _lib.load(require_gpu=False)
    P = int(B if positives_per_image is None else positives_per_image)
    return _mh_name(lib.frcnn_mask_targets_kernel, "mask_targets_kernel", int(B), P, int(mask_size))


def mask_head_losses_kernel(C, mask_size=28, dtype=torch.float32) -> str:
    """frcnn_mask_losses_kernel: the forward's two kernels and the backward's, with the elements
    of its 16-byte stores.  Host only."""
    lib = _lib.load(require_gpu=False)
    return _mh_name(lib.frcnn_mask_losses_kernel, "mask_losses_kernel", _lib.dtype_code(dtype), int(C), int(mask_size))


def mask_head_paste_kernel(mask_size, canvas_w, padding=1, threshold=0.5, dtype=torch.float32) -> str:
    """frcnn_mask_paste_kernel: the paste kernel of this logit dtype and output form ("u8" with a
    threshold, "f32" with ``threshold=None``) and its plan branch ("vec16" / "vec4": every row of
    the canvas is whole vectors; "+edges": rows have an unaligned head or a tail).  Host only."""
    lib = _lib.load(require_gpu=False)
    return _mh_name(lib.frcnn_mask_paste_kernel, "mask_paste_kernel", _lib.dtype_code(dtype), int(mask_size),
                    int(padding), int(canvas_w), int(threshold is not None))


def mask_head_targets(box_targets, gt_masks, *, mask_size: int = 28, positives_per_image=None, out=None):
    """The mask targets of torchvision's ``RoIHeads.forward`` / ``project_masks_on_boxes`` for the
    whole batch: two launches, no host synchronisation (frcnn_mask_targets; DESIGN.md §3 "Pyramid
    mask head" is the contract).

    ``box_targets``: the ``BoxHeadTargets`` of ``box_head_targets`` (B slots per image);
    ``gt_masks``: uint8 device tensor [N, G, Hm, Wm], read as it is (a byte v is the value v).
    An image's positives (``labels >= 1``) are compacted in slot order into rows 0..count-1 of
    its ``P = positives_per_image`` rows (default B); positives beyond P are dropped.

    Returns ``MaskHeadTargets(rois fp32 [N*P, 5], labels, matched, slot int32 [N, P], count int32
    [N], targets fp32 [N*P, M, M])``: ``targets[row]`` is ``roi_align`` of the matched mask over
    the row's box at ``(M, M)`` with ``spatial_scale=1``, ``sampling_ratio=-1``, ``aligned=False``,
    bit for bit; a ``matched`` outside [0, G) or a box that is not finite gives zeros.  Padding
    rows: ``rois`` (-1, 0, 0, 0, 0), labels / matched / slot -1, targets +0.

    A hot-path op: nothing is converted; a wrong dtype, shape, device or a strided view raises
    RuntimeError naming the argument before any launch.  ``out``: the six outputs, caller-owned."""
    op = "mask_head_targets"
    lib = _lib.load()
    if not isinstance(box_targets, BoxHeadTargets):
        raise RuntimeError(f"{op}: box_targets must be the BoxHeadTargets of box_head_targets; got "
                           f"{type(box_targets).__name__}")
    lab = box_targets.labels
    if not isinstance(lab, torch.Tensor) or lab.dim() != 2:
        raise RuntimeError(f"{op}: box_targets.labels must be an int32 device tensor of shape [N, B]")
    N, B = int(lab.shape[0]), int(lab.shape[1])
    if not 1 <= N <= FPN_MAX_N:
        raise RuntimeError(f"{op}: box_targets.labels: N must be in [1, {FPN_MAX_N}]; got {N}")
    if not 1 <= B <= RPN_TARGETS_MAX_BATCH:
        raise RuntimeError(f"{op}: box_targets.labels: B must be in [1, {RPN_TARGETS_MAX_BATCH}]; got {B}")
    dev = _rpnt_device(op, "box_targets.labels", lab)
    _rpnt_tensor(op, "box_targets.labels", lab, torch.int32, (N, B), dev)
    _rpnt_tensor(op, "box_targets.matched", box_targets.matched, torch.int32, (N, B), dev)
    _rpnt_tensor(op, "box_targets.rois", box_targets.rois, torch.float32, (N * B, 5), dev)
    if not isinstance(gt_masks, torch.Tensor) or gt_masks.dim() != 4:
        raise RuntimeError(f"{op}: gt_masks must be a uint8 device tensor of shape [N, G, Hm, Wm]")
    G, Hm, Wm = (int(v) for v in gt_masks.shape[1:])
    if not 1 <= G <= MASK_HEAD_MAX_G:
        raise RuntimeError(f"{op}: gt_masks: G must be in [1, {MASK_HEAD_MAX_G}]; got {G}")
    if not (1 <= Hm <= MASK_HEAD_MAX_DIM and 1 <= Wm <= MASK_HEAD_MAX_DIM):
        raise RuntimeError(f"{op}: gt_masks: Hm and Wm must be in [1, {MASK_HEAD_MAX_DIM}]; got {Hm} x {Wm}")
    _rpnt_tensor(op, "gt_masks", gt_masks, torch.uint8, (N, G, Hm, Wm), dev)
    M = int(mask_size)
    if not 1 <= M <= MASK_HEAD_MAX_M:
        raise RuntimeError(f"{op}: mask_size must be in [1, {MASK_HEAD_MAX_M}]; got {M}")
    P = B if positives_per_image is None else int(positives_per_image)
    if not 1 <= P <= RPN_TARGETS_MAX_BATCH:
        raise RuntimeError(f"{op}: positives_per_image must be in [1, {RPN_TARGETS_MAX_BATCH}]; got {P}")
    i32, f32 = torch.int32, torch.float32
    shapes = (((N * P, 5), f32, "rois"), ((N, P), i32, "labels"), ((N, P), i32, "matched"), ((N, P), i32, "slot"),
              ((N,), i32, "count"), ((N * P, M, M), f32, "targets"))
    if out is None:
        outs = tuple(torch.empty(s, dtype=d, device=dev) for s, d, _ in shapes)
    else:
        if not isinstance(out, (list, tuple)) or len(out) != 6:
            raise RuntimeError(f"{op}: out must be the six outputs (rois, labels, matched, slot, count, targets)")
        outs = tuple(out)
        for i, (s, d, nm) in enumerate(shapes):
            _rpnt_tensor(op, f"out[{i}] ({nm})", outs[i], d, s, dev)
    _lib.check(lib.frcnn_mask_targets(N, B, P, G, Hm, Wm, M, _lib.ptr(box_targets.rois), _lib.ptr(lab),
                                      _lib.ptr(box_targets.matched), _lib.ptr(gt_masks),
                                      *[_lib.ptr(t) for t in outs], _lib.stream_ptr()), op)
    return MaskHeadTargets(*outs)


class _MaskHeadLossesFunction(torch.autograd.Function):
    """frcnn_mask_losses_fwd_t / _bwd_t; the incoming gradient goes to the kernel as a device pointer."""

    @staticmethod
    def forward(ctx, targets, code, ws, logits):
        lib = _lib.load()
        N, P = targets.labels.shape
        C, M = int(logits.shape[1]), int(logits.shape[2])
        dev = logits.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        stats = torch.empty(4, dtype=torch.int32, device=dev)
        _lib.check(lib.frcnn_mask_losses_fwd_t(code, N, P, C, M, _lib.ptr(logits), _lib.ptr(targets.targets),
                                               _lib.ptr(targets.labels), _lib.ptr(targets.count), _lib.ptr(loss),
                                               _lib.ptr(stats), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                   "mask_head_losses forward")
        ctx.save_for_backward(logits, targets.targets, targets.labels, targets.count, stats)
        ctx.meta = (code, N, P, C, M)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(stats)
        return loss[0], stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_stats):
        lib = _lib.load()
        code, N, P, C, M = ctx.meta
        logits, tgt, labels, count, stats = ctx.saved_tensors
        if g is not None and (g.dtype != torch.float32 or not g.is_cuda or g.numel() != 1):
            raise RuntimeError("mask_head_losses backward: the gradient of the loss must be one torch.float32 on "
                               f"the device; got {g.dtype} on {g.device.type} with {g.numel()} elements")
        d = torch.empty_like(logits)   # each element is stored once
        _lib.check(lib.frcnn_mask_losses_bwd_t(code, N, P, C, M, _lib.ptr(logits), _lib.ptr(tgt), _lib.ptr(labels),
                                               _lib.ptr(count), _lib.ptr(stats), _lib.ptr(g), _lib.ptr(d),
                                               _lib.stream_ptr()), "mask_head_losses backward")
        return None, None, None, d


def _mask_head_losses(mask_logits, targets, workspace):
    op = "mask_head_losses"
    lib = _lib.load()
    if not isinstance(targets, MaskHeadTargets):
        raise RuntimeError(f"{op}: targets must be the MaskHeadTargets of mask_head_targets; got {type(targets).__name__}")
    code = _lib.prediction_dtype_code(op, (("mask_logits", mask_logits),))
    if mask_logits.dim() != 4:
        raise RuntimeError(f"{op}: mask_logits must be a device tensor of shape [N*P, C, M, M]; got "
                           f"{list(mask_logits.shape)}")
    C, M = int(mask_logits.shape[1]), int(mask_logits.shape[2])
    if not 2 <= C <= BOX_HEAD_MAX_C:
        raise RuntimeError(f"{op}: mask_logits: C must be in [2, {BOX_HEAD_MAX_C}]; got {C}")
    if not 1 <= M <= MASK_HEAD_MAX_M:
        raise RuntimeError(f"{op}: mask_logits: M must be in [1, {MASK_HEAD_MAX_M}]; got {M}")
    dev = _rpnt_device(op, "mask_logits", mask_logits)
    if not isinstance(targets.labels, torch.Tensor) or targets.labels.dim() != 2:
        raise RuntimeError(f"{op}: targets.labels must be an int32 device tensor of shape [N, P]")
    N, P = int(targets.labels.shape[0]), int(targets.labels.shape[1])
    if not 1 <= N <= FPN_MAX_N:
        raise RuntimeError(f"{op}: targets.labels: N must be in [1, {FPN_MAX_N}]; got {N}")
    if not 1 <= P <= RPN_TARGETS_MAX_BATCH:
        raise RuntimeError(f"{op}: targets.labels: P must be in [1, {RPN_TARGETS_MAX_BATCH}]; got {P}")
    _rpnt_tensor(op, "mask_logits", mask_logits, mask_logits.dtype, (N * P, C, M, M), dev)
    _rpnt_tensor(op, "targets.labels", targets.labels, torch.int32, (N, P), dev)
    _rpnt_tensor(op, "targets.count", targets.count, torch.int32, (N,), dev)
    _rpnt_tensor(op, "targets.targets", targets.targets, torch.float32, (N * P, M, M), dev)
    need = _mhl_ws.get((N, P))
    if need is None:
        need = _mhl_ws[(N, P)] = int(lib.frcnn_mask_losses_workspace_size(N, P))
    ws = workspace if workspace is not None else _lib.cached_workspace(op, need, dev)
    if (not isinstance(ws, torch.Tensor) or not ws.is_cuda or ws.dtype != torch.uint8 or not ws.is_contiguous()
            or ws.numel() < need or ws.device != dev):
        raise RuntimeError(f"{op}: workspace must be a contiguous uint8 tensor of at least {need} B on {dev}")
    return _MaskHeadLossesFunction.apply(targets, code, ws, mask_logits)


def mask_head_losses(mask_logits, targets, *, workspace=None):
    """torchvision's ``maskrcnn_loss`` on ``mask_head_targets``' result, differentiable in
    ``mask_logits`` (frcnn_mask_losses_fwd_t / _bwd_t; DESIGN.md §3 "Pyramid mask head").

    ``mask_logits``: [N*P, C, M, M] in fp32, float16 or bfloat16, contiguous, row ``n*P + r`` as
    ``targets.rois`` orders them; only channel ``labels[row]`` of the rows below their image's
    ``count`` is read.  Returns the 0-dim fp32 mean over the S*M*M elements of the
    binary cross-entropy with logits against the soft targets, S the sum of ``count`` taken on
    the device; S == 0 gives +0 and all-zero gradients.  A row whose label is >= C is skipped
    and counted (``mask_head_losses_with_stats``), never used as an index.

    The backward stores every element of the gradient once, in the input's dtype, with no
    atomics: the same bits on every call.  Nothing is converted and nothing synchronises; a wrong
    dtype, shape, device or a strided view raises RuntimeError naming the argument before any
    launch.  ``workspace``: a uint8 device tensor of at least the cached size."""
    return _mask_head_losses(mask_logits, targets, workspace)[0]


def mask_head_losses_with_stats(mask_logits, targets, *, workspace=None):
    """``mask_head_losses`` plus ``stats``: int32 device tensor (S, rows skipped for a label
    outside [0, C), 0, 0)."""
    return _mask_head_losses(mask_logits, targets, workspace)


def mask_head_paste(mask_logits, boxes, labels, count, canvas_size, *, image_sizes=None, original_sizes=None,
                    padding: int = 1, threshold=0.5, out=None):
    """torchvision's ``maskrcnn_inference`` and ``paste_masks_in_image`` for the whole batch: one
    launch, no host synchronisation (frcnn_mask_paste_t; DESIGN.md §3 "Pyramid mask head").

    ``mask_logits``: [N*D, C, M, M] in fp32, float16 or bfloat16; ``boxes`` fp32 [N, D, 4],
    ``labels`` int32 [N, D], ``count`` int32 [N]: those of ``BoxDetections``;
    ``canvas_size = (Hc, Wc)``: host ints.  ``original_sizes`` (fp32 device [N, 2] of (h, w)) clips
    each image's masks to its own size; with ``image_sizes`` as well the boxes are first mapped by
    ``resize_boxes`` as ``box_head_detections`` does it.

    Returns ``masks [N, D, Hc, Wc]``: uint8 0 / 1 of ``prob > threshold``, or the fp32
    probabilities with ``threshold=None``.  Rows at or beyond ``count``, labels outside [1, C),
    boxes that are not finite or are inverted give all-zero masks.  ``out``: the caller's tensor."""
    op = "mask_head_paste"
    lib = _lib.load()
    code = _lib.prediction_dtype_code(op, (("mask_logits", mask_logits),))
    if mask_logits.dim() != 4:
        raise RuntimeError(f"{op}: mask_logits must be a device tensor of shape [N*D, C, M, M]; got "
                           f"{list(mask_logits.shape)}")
    if not isinstance(boxes, torch.Tensor) or boxes.dim() != 3:
        raise RuntimeError(f"{op}: boxes must be an fp32 device tensor of shape [N, D, 4]")
    N, D = int(boxes.shape[0]), int(boxes.shape[1])
    if not 1 <= N <= FPN_MAX_N:
        raise RuntimeError(f"{op}: boxes: N must be in [1, {FPN_MAX_N}]; got {N}")
    if not 1 <= D <= BOX_DET_MAX_D:
        raise RuntimeError(f"{op}: boxes: D must be in [1, {BOX_DET_MAX_D}]; got {D}")
    C, M = int(mask_logits.shape[1]), int(mask_logits.shape[2])
    if not 2 <= C <= BOX_HEAD_MAX_C:
        raise RuntimeError(f"{op}: mask_logits: C must be in [2, {BOX_HEAD_MAX_C}]; got {C}")
    if not 1 <= M <= MASK_HEAD_MAX_M:
        raise RuntimeError(f"{op}: mask_logits: M must be in [1, {MASK_HEAD_MAX_M}]; got {M}")
    dev = _rpnt_device(op, "mask_logits", mask_logits)
    _rpnt_tensor(op, "mask_logits", mask_logits, mask_logits.dtype, (N * D, C, M, M), dev)
    _rpnt_tensor(op, "boxes", boxes, torch.float32, (N, D, 4), dev)
    _rpnt_tensor(op, "labels", labels, torch.int32, (N, D), dev)
    _rpnt_tensor(op, "count", count, torch.int32, (N,), dev)
    try:
        Hc, Wc = int(canvas_size[0]), int(canvas_size[1])
        if len(canvas_size) != 2:
            raise ValueError
    except (TypeError, ValueError, IndexError):
        raise RuntimeError(f"{op}: canvas_size must be two host ints (Hc, Wc); got {canvas_size!r}") from None
    if not (1 <= Hc <= MASK_HEAD_MAX_DIM and 1 <= Wc <= MASK_HEAD_MAX_DIM):
        raise RuntimeError(f"{op}: canvas_size: Hc and Wc must be in [1, {MASK_HEAD_MAX_DIM}]; got {Hc} x {Wc}")
    if original_sizes is not None:
        _rpnt_tensor(op, "original_sizes", original_sizes, torch.float32, (N, 2), dev)
    if image_sizes is not None:
        if original_sizes is None:
            raise RuntimeError(f"{op}: image_sizes maps the boxes to original_sizes, which is missing")
        _rpnt_tensor(op, "image_sizes", image_sizes, torch.float32, (N, 2), dev)
    pad = int(padding)
    if not 0 <= pad <= MASK_HEAD_MAX_PAD:
        raise RuntimeError(f"{op}: padding must be in [0, {MASK_HEAD_MAX_PAD}]; got {pad}")
    binary = threshold is not None
    thr = float(threshold) if binary else 0.0
    if thr != thr:
        raise RuntimeError(f"{op}: threshold must be a number or None; got {threshold!r}")
    odt = torch.uint8 if binary else torch.float32
    if out is None:
        out = torch.empty((N, D, Hc, Wc), dtype=odt, device=dev)
    else:
        _rpnt_tensor(op, "out", out, odt, (N, D, Hc, Wc), dev)
    _lib.check(lib.frcnn_mask_paste_t(code, N, D, C, M, _lib.ptr(mask_logits), _lib.ptr(boxes), _lib.ptr(labels),
                                      _lib.ptr(count), _lib.ptr(image_sizes), _lib.ptr(original_sizes), pad, thr,
                                      int(binary), Hc, Wc, _lib.ptr(out), _lib.stream_ptr()), op)
    return out


def detection_rois(detections):
    """``[N*D, 5]`` RoIs (n, x1, y1, x2, y2) of a ``BoxDetections`` for ``multiscale_roi_align``;
    the rows at or beyond ``count`` are the padding (-1, 0, 0, 0, 0), which it pools to zeros.
    Plain torch ops, no synchronisation."""
    boxes, count = detections.boxes, detections.count
    N, D = int(boxes.shape[0]), int(boxes.shape[1])
    real = torch.arange(D, device=boxes.device)[None, :] < count[:, None]
    idx = torch.arange(N, device=boxes.device, dtype=boxes.dtype)[:, None].expand(N, D)
    idx = torch.where(real, idx, idx.new_full((), -1.0))
    b = torch.where(real[:, :, None], boxes, boxes.new_zeros(()))
    return torch.cat([idx[:, :, None], b], 2).reshape(N * D, 5)


# ----------------------------------------------------------------- detections
REG_MEAN =(0.0, 0.0, 0.0, 0.0)   # utils/utils.py:272 (ProposalTargetCreator's normalisation)
REG_STD = (0.1, 0.1, 0.2, 0.2)
_detect_cache = {}  # host reg_mean / reg_std arrays + workspace size per shape (built once)


def detect(rois: torch.Tensor, rcount: torch.Tensor, cls: torch.Tensor, reg: torch.Tensor, *,
           img_h: float, img_w: float, score_thresh: float = 0.05, nms_thresh: float = 0.3,
           reg_mean=REG_MEAN, reg_std=REG_STD, max_det: int = None, out=None, workspace=None):
    """Head outputs -> detections on device tensors (frcnn_detect; DESIGN.md
    "Detections" is the contract): softmax, per-class decode, score threshold
    and per-class NMS for the whole batch.

    rois fp32 [N, R, 4] + rcount int32 [N] (``RPN.rois_padded`` / ``rois_count``
    as they are), cls [N, R, C] logits (``ResnetHead`` returns the
    ``[N, C, R]`` view: pass ``cls.permute(0, 2, 1).contiguous()``), reg
    [N, R, 4C]; cls and reg are both fp32, both float16 or both bfloat16 (a head
    under autocast; widened exactly inside the kernels, every output is the fp32
    op's on the widened inputs).  Returns padded (det_boxes [N, max_det, 4], det_labels int32
    [N, max_det], det_scores [N, max_det], det_roi int32 [N, max_det], det_count
    int32 [N], det_total int32 [N]) -- no host synchronisation.  ``max_det``
    defaults to R*(C-1), which never truncates.
    """
    lib = _lib.load()
    code = _lib.prediction_dtype_code("detect", (("cls", cls), ("reg", reg)))
    for name, t, dt in (("rois", rois, torch.float32), ("rcount", rcount, torch.int32),
                        ("cls", cls, cls.dtype), ("reg", reg, cls.dtype)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_cuda or not t.is_contiguous():
            raise RuntimeError(f"detect: {name} must be a contiguous {dt} device tensor")
    if cls.dim() != 3:
        raise RuntimeError(f"detect: cls must be [N, R, C]; got {tuple(cls.shape)}")
    N, R, C = cls.shape
    if tuple(rois.shape) != (N, R, 4) or tuple(rcount.shape) != (N,) or tuple(reg.shape) != (N, R, 4 * C):
        raise RuntimeError(f"detect: rois {tuple(rois.shape)} / rcount {tuple(rcount.shape)} / reg "
                           f"{tuple(reg.shape)} do not match cls {tuple(cls.shape)}")
    if max_det is None:
        max_det = R * (C - 1)
    max_det = int(max_det)
    dev = cls.device
    key = (N, R, C, tuple(float(v) for v in reg_mean), tuple(float(v) for v in reg_std))
    cached = _detect_cache.get(key)
    if cached is None:
        if len(key[3]) != 4 or len(key[4]) != 4:
            raise RuntimeError("detect: reg_mean and reg_std must have 4 values")
        cached = ((_lib.F32 * 4)(*key[3]), (_lib.F32 * 4)(*key[4]),
                  int(lib.frcnn_detect_workspace_size(N, R, C)))
        _detect_cache[key] = cached
    mean, std, need = cached
    if out is None:
        out = (torch.empty((N, max_det, 4), dtype=torch.float32, device=dev),
               torch.empty((N, max_det), dtype=torch.int32, device=dev),
               torch.empty((N, max_det), dtype=torch.float32, device=dev),
               torch.empty((N, max_det), dtype=torch.int32, device=dev),
               torch.empty((N,), dtype=torch.int32, device=dev),
               torch.empty((N,), dtype=torch.int32, device=dev))
    else:  # caller-owned outputs (static buffers of a captured HIP graph)
        want = [((N, max_det, 4), torch.float32), ((N, max_det), torch.int32), ((N, max_det), torch.float32),
                ((N, max_det), torch.int32), ((N,), torch.int32), ((N,), torch.int32)]
        if len(out) != 6 or any(tuple(t.shape) != s or t.dtype != d or not t.is_contiguous()
                                for t, (s, d) in zip(out, want)):
            raise RuntimeError("detect: out buffers must be fp32 [N,max_det,4], int32 [N,max_det], "
                               "fp32 [N,max_det], int32 [N,max_det], int32 [N], int32 [N]")
    ws = workspace if workspace is not None else _lib.cached_workspace("detect", need, dev)
    if need and ws.numel() < need:
        raise RuntimeError(f"detect: workspace of {ws.numel()} B < {need} B")
    boxes, labels, scores, roi, count, total = out
    _lib.check(lib.frcnn_detect_t(code, N, R, C, _lib.ptr(rois), _lib.ptr(rcount), _lib.ptr(cls), _lib.ptr(reg),
                                  mean, std, float(img_h), float(img_w), float(score_thresh),
                                  float(nms_thresh), max_det, _lib.ptr(boxes), _lib.ptr(labels),
                                  _lib.ptr(scores), _lib.ptr(roi), _lib.ptr(count), _lib.ptr(total),
                                  _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "detect")
    return boxes, labels, scores, roi, count, total


# ----------------------------------------------------------------- evaluation
EVAL_MAX_CAPACITY = 1 << 24   # the record index is a 24-bit field of rec_key


def eval_state(n_class: int, capacity: int, device=None):
    """An empty evaluation accumulator (DESIGN.md "Evaluation"): (hdr int64
    [4 + n_class] zeroed, rec_key int64 [capacity] -- the C-ABI's uint64 keys,
    whose top bit is never set --, rec_flag int8 [capacity], rec_image int32
    [capacity]) on the device."""
    _lib.load()
    if not 2 <= int(n_class) <= 128 or not 1 <= int(capacity) <= EVAL_MAX_CAPACITY:
        raise RuntimeError(f"eval_state: n_class={n_class} must be in [2, 128] and capacity={capacity} in "
                           f"[1, {EVAL_MAX_CAPACITY}]")
    dev = _lib.device() if device is None else device
    return (torch.zeros(4 + int(n_class), dtype=torch.int64, device=dev),
            torch.empty(int(capacity), dtype=torch.int64, device=dev),
            torch.empty(int(capacity), dtype=torch.int8, device=dev),
            torch.empty(int(capacity), dtype=torch.int32, device=dev))


def _eval_state_check(state, what):
    want = (torch.int64, torch.int64, torch.int8, torch.int32)
    if len(state) != 4 or any(not isinstance(t, torch.Tensor) or t.dtype != d or not t.is_cuda or t.dim() != 1
                              or not t.is_contiguous() for t, d in zip(state, want)):
        raise RuntimeError(f"{what}: state must be ops.eval_state's (hdr int64, rec_key int64, rec_flag int8, "
                           "rec_image int32) device tensors")
    hdr, key, flag, image = state
    if hdr.numel() < 6 or flag.numel() != key.numel() or image.numel() != key.numel() or key.numel() < 1:
        raise RuntimeError(f"{what}: state arrays of {hdr.numel()} / {key.numel()} / {flag.numel()} / "
                           f"{image.numel()} elements do not belong together")
    return hdr.numel() - 4, key.numel()


def eval_update(det, gt_boxes: torch.Tensor, gt_labels: torch.Tensor, gt_difficult: torch.Tensor = None, *,
                state, iou_thresh: float = 0.5, plus_one: bool = True) -> None:
    """Score one batch of detections against its ground truth and append the
    TP / FP / ignored records to ``state`` (frcnn_eval_update; DESIGN.md
    "Evaluation" is the contract) -- stream-ordered, no allocation, no host
    synchronisation.

    ``det`` is the tuple ``ops.detect`` returns (or ``(det_boxes, det_labels,
    det_scores, det_count)``); gt_boxes fp64 [N, G, 4] as [ymin, xmin, ymax,
    xmax], gt_labels int32 [N, G] (valid rows: 1..n_class-1), gt_difficult
    uint8 [N, G] or None; all contiguous device tensors.  A batch that does not
    fit in the state's capacity is dropped as a whole and counted in hdr[2]."""
    lib = _lib.load()
    if len(det) == 6:
        boxes, labels, scores, _, count, _ = det
    elif len(det) == 4:
        boxes, labels, scores, count = det
    else:
        raise RuntimeError("eval_update: det must be ops.detect's 6-tuple or (boxes, labels, scores, count)")
    ins = [("det_boxes", boxes, torch.float32), ("det_labels", labels, torch.int32),
           ("det_scores", scores, torch.float32), ("det_count", count, torch.int32),
           ("gt_boxes", gt_boxes, torch.float64), ("gt_labels", gt_labels, torch.int32)]
    if gt_difficult is not None:
        ins.append(("gt_difficult", gt_difficult, torch.uint8))
    for name, t, dt in ins:
        if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_cuda or not t.is_contiguous():
            raise RuntimeError(f"eval_update: {name} must be a contiguous {dt} device tensor")
    C, cap = _eval_state_check(state, "eval_update")
    if labels.dim() != 2 or gt_labels.dim() != 2:
        raise RuntimeError("eval_update: det_labels must be [N, M] and gt_labels [N, G]")
    N, M = labels.shape
    G = gt_labels.shape[1]
    if (tuple(boxes.shape) != (N, M, 4) or tuple(scores.shape) != (N, M) or tuple(count.shape) != (N,)
            or tuple(gt_boxes.shape) != (N, G, 4) or gt_labels.shape[0] != N
            or (gt_difficult is not None and tuple(gt_difficult.shape) != (N, G))):
        raise RuntimeError(f"eval_update: det {tuple(boxes.shape)} / {tuple(labels.shape)} / {tuple(scores.shape)} / "
                           f"{tuple(count.shape)} and gt {tuple(gt_boxes.shape)} / {tuple(gt_labels.shape)} do not "
                           "match")
    hdr, key, flag, image = state
    _lib.check(lib.frcnn_eval_update(N, M, G, C, cap, _lib.ptr(boxes), _lib.ptr(labels), _lib.ptr(scores),
                                     _lib.ptr(count), _lib.ptr(gt_boxes), _lib.ptr(gt_labels),
                                     _lib.ptr(gt_difficult), float(iou_thresh), int(bool(plus_one)),
                                     _lib.ptr(hdr), _lib.ptr(key), _lib.ptr(flag), _lib.ptr(image),
                                     _lib.stream_ptr()), "eval_update")


def eval_ap(state, n_records: int = None, *, use_07_metric: bool = False, return_sorted: bool = False,
            workspace=None):
    """Per-class AP and mAP of an accumulator (frcnn_eval_ap): (ap fp64 [C],
    map fp64 [1]) device tensors, plus the sorted keys (int64 [n_records]) with
    ``return_sorted``.  ``n_records`` is hdr[0]; when it is not given it is read
    from the device (a host synchronisation)."""
    lib = _lib.load()
    C, cap = _eval_state_check(state, "eval_ap")
    hdr, key, flag, _ = state
    n = int(hdr[0].item()) if n_records is None else int(n_records)
    if not 0 <= n <= cap:
        raise RuntimeError(f"eval_ap: n_records={n} outside the state's capacity {cap}")
    dev = hdr.device
    ap = torch.empty(C, dtype=torch.float64, device=dev)
    mean = torch.empty(1, dtype=torch.float64, device=dev)
    skey = torch.empty(n, dtype=torch.int64, device=dev) if return_sorted else None
    need = int(lib.frcnn_eval_ap_workspace_size(C, max(n, 1)))
    ws = workspace if workspace is not None else _lib.cached_workspace("eval_ap", need, dev)
    if ws.numel() < need:
        raise RuntimeError(f"eval_ap: workspace of {ws.numel()} B < {need} B")
    _lib.check(lib.frcnn_eval_ap(C, n, _lib.ptr(hdr), _lib.ptr(key), _lib.ptr(flag), int(bool(use_07_metric)),
                                 _lib.ptr(ap), _lib.ptr(mean), _lib.ptr(skey) if n else None, _lib.ptr(ws),
                                 ws.numel(), _lib.stream_ptr()), "eval_ap")
    return (ap, mean, skey) if return_sorted else (ap, mean)


# ------------------------------------------------------ COCO-style evaluation
def coco_eval_tables():
    """The constants of the COCO protocol as the one fp64 [119] table the kernels
    read: IoU thresholds T[10], recall thresholds R[101], area ranges A[4][2]
    (all, small, medium, large; both ends inclusive).  Host tensor."""
    import numpy as np
    t = np.linspace(.5, .95, 10)
    r = np.linspace(0, 1, 101)
    a = np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], np.float64)
    return torch.from_numpy(np.concatenate([t, r, a.reshape(-1)]))


def coco_eval_state(n_class: int, capacity: int, device=None):
    """An empty COCO-style accumulator (DESIGN.md "COCO-style evaluation"): (hdr
    int64 [4 + 4 * n_class] zeroed, rec_key int64 [capacity], rec_bits int64
    [capacity, 2] -- the C-ABI's uint64 words --, tables fp64 [119]) on the device."""
    _lib.load()
    if not 2 <= int(n_class) <= 128 or not 1 <= int(capacity) <= EVAL_MAX_CAPACITY:
        raise RuntimeError(f"coco_eval_state: n_class={n_class} must be in [2, 128] and capacity={capacity} in "
                           f"[1, {EVAL_MAX_CAPACITY}]")
    dev = _lib.device() if device is None else device
    return (torch.zeros(4 + 4 * int(n_class), dtype=torch.int64, device=dev),
            torch.empty(int(capacity), dtype=torch.int64, device=dev),
            torch.empty((int(capacity), 2), dtype=torch.int64, device=dev),
            coco_eval_tables().to(dev))


def _coco_state_check(state, what):
    want = (torch.int64, torch.int64, torch.int64, torch.float64)
    if len(state) != 4 or any(not isinstance(t, torch.Tensor) or t.dtype != d or not t.is_cuda
                              or not t.is_contiguous() for t, d in zip(state, want)):
        raise RuntimeError(f"{what}: state must be ops.coco_eval_state's (hdr int64, rec_key int64, rec_bits int64, "
                           "tables float64) device tensors")
    hdr, key, bits, tables = state
    if (hdr.dim() != 1 or hdr.numel() < 12 or (hdr.numel() - 4) % 4 or key.dim() != 1 or key.numel() < 1
            or tuple(bits.shape) != (key.numel(), 2) or tuple(tables.shape) != (119,)):
        raise RuntimeError(f"{what}: state arrays of shapes {tuple(hdr.shape)} / {tuple(key.shape)} / "
                           f"{tuple(bits.shape)} / {tuple(tables.shape)} do not belong together")
    return (hdr.numel() - 4) // 4, key.numel()


def coco_eval_update(det, gt_boxes: torch.Tensor, gt_labels: torch.Tensor, gt_crowd: torch.Tensor = None, *,
                     state) -> None:
    """Match one batch of detections against its ground truth at the ten IoU
    thresholds and four area ranges of the COCO protocol and append the records
    to ``state`` (frcnn_coco_eval_update; DESIGN.md "COCO-style evaluation" is the
    contract) -- stream-ordered, no allocation, no host synchronisation.

    ``det`` is the tuple ``ops.detect`` returns (or ``(det_boxes, det_labels,
    det_scores, det_count)``); gt_boxes fp64 [N, G, 4] as [ymin, xmin, ymax,
    xmax], gt_labels int32 [N, G] (valid rows: 1..n_class-1), gt_crowd uint8
    [N, G] or None; all contiguous device tensors.  ``gt_crowd`` is the one gt
    flag, as in pycocotools, where ``iscrowd`` overwrites ``ignore``: a flagged gt
    is an ignore region that any number of detections may match (IoU over the
    detection's area), and it counts as no positive.  Pass VOC's
    ``gt_difficult`` there to have difficult objects treated that way.  A batch
    that does not fit in the state's capacity is dropped as a whole and counted
    in hdr[2]."""
    lib = _lib.load()
    if len(det) == 6:
        boxes, labels, scores, _, count, _ = det
    elif len(det) == 4:
        boxes, labels, scores, count = det
    else:
        raise RuntimeError("coco_eval_update: det must be ops.detect's 6-tuple or (boxes, labels, scores, count)")
    ins = [("det_boxes", boxes, torch.float32), ("det_labels", labels, torch.int32),
           ("det_scores", scores, torch.float32), ("det_count", count, torch.int32),
           ("gt_boxes", gt_boxes, torch.float64), ("gt_labels", gt_labels, torch.int32)]
    if gt_crowd is not None:
        ins.append(("gt_crowd", gt_crowd, torch.uint8))
    for name, t, dt in ins:
        if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_cuda or not t.is_contiguous():
            raise RuntimeError(f"coco_eval_update: {name} must be a contiguous {dt} device tensor")
    C, cap = _coco_state_check(state, "coco_eval_update")
    if labels.dim() != 2 or gt_labels.dim() != 2:
        raise RuntimeError("coco_eval_update: det_labels must be [N, M] and gt_labels [N, G]")
    N, M = labels.shape
    G = gt_labels.shape[1]
    if (tuple(boxes.shape) != (N, M, 4) or tuple(scores.shape) != (N, M) or tuple(count.shape) != (N,)
            or tuple(gt_boxes.shape) != (N, G, 4) or gt_labels.shape[0] != N
            or (gt_crowd is not None and tuple(gt_crowd.shape) != (N, G))):
        raise RuntimeError(f"coco_eval_update: det {tuple(boxes.shape)} / {tuple(labels.shape)} / "
                           f"{tuple(scores.shape)} / {tuple(count.shape)} and gt {tuple(gt_boxes.shape)} / "
                           f"{tuple(gt_labels.shape)} do not match")
    hdr, key, bits, tables = state
    _lib.check(lib.frcnn_coco_eval_update(N, M, G, C, cap, _lib.ptr(boxes), _lib.ptr(labels), _lib.ptr(scores),
                                          _lib.ptr(count), _lib.ptr(gt_boxes), _lib.ptr(gt_labels),
                                          _lib.ptr(gt_crowd), _lib.ptr(tables), _lib.ptr(hdr), _lib.ptr(key),
                                          _lib.ptr(bits), _lib.stream_ptr()), "coco_eval_update")


def coco_eval_accumulate(state, n_records: int = None, *, workspace=None):
    """pycocotools' accumulate() and summarize() of an accumulator
    (frcnn_coco_eval_accumulate): (precision fp64 [10, 101, C, 4, 3], recall fp64
    [10, C, 4, 3], stats fp64 [12], ap_per_class fp64 [C]) device tensors; -1
    where there is no gt.  ``n_records`` is hdr[0]; when it is not given it is
    read from the device (a host synchronisation)."""
    lib = _lib.load()
    C, cap = _coco_state_check(state, "coco_eval_accumulate")
    hdr, key, bits, tables = state
    n = int(hdr[0].item()) if n_records is None else int(n_records)
    if not 0 <= n <= cap:
        raise RuntimeError(f"coco_eval_accumulate: n_records={n} outside the state's capacity {cap}")
    dev = hdr.device
    precision = torch.empty((10, 101, C, 4, 3), dtype=torch.float64, device=dev)
    recall = torch.empty((10, C, 4, 3), dtype=torch.float64, device=dev)
    stats = torch.empty(12, dtype=torch.float64, device=dev)
    apc = torch.empty(C, dtype=torch.float64, device=dev)
    need = int(lib.frcnn_coco_eval_workspace_size(C, max(n, 1)))
    ws = workspace if workspace is not None else _lib.cached_workspace("coco_eval", need, dev)
    if ws.numel() < need:
        raise RuntimeError(f"coco_eval_accumulate: workspace of {ws.numel()} B < {need} B")
    _lib.check(lib.frcnn_coco_eval_accumulate(C, n, _lib.ptr(hdr), _lib.ptr(key), _lib.ptr(bits), _lib.ptr(tables),
                                              _lib.ptr(precision), _lib.ptr(recall), _lib.ptr(stats), _lib.ptr(apc),
                                              _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "coco_eval_accumulate")
    return precision, recall, stats, apc


# ------------------------------------------------------ COCO segm evaluation
MASK_OVERLAP_MAX_N, MASK_OVERLAP_MAX_D, MASK_OVERLAP_MAX_G, MASK_OVERLAP_MAX_DIM = 1024, 1024, 256, 4096
MASK_OVERLAP_MAX_PIXELS, MASK_OVERLAP_MAX_C = 1 << 24, 128
MaskOverlap = collections.namedtuple("MaskOverlap", "inter det_area gt_area")
_mo_ws = {}   # (N, D, G, H, W) -> workspace bytes


def mask_overlap_kernel(canvas_h, canvas_w) -> str:
    """frcnn_mask_overlap_kernel: the two kernels of a ``mask_overlap`` call and the pack
    kernel's plan branch ("vec16": every row is whole 16-byte vectors; "+edges": rows have
    an unaligned head or a tail).  Host only."""
    lib = _lib.load(require_gpu=False)
    return _mh_name(lib.frcnn_mask_overlap_kernel, "mask_overlap_kernel", int(canvas_h), int(canvas_w))


def coco_eval_kernel(segm: bool = False) -> str:
    """frcnn_coco_eval_kernel: the kernels of ``coco_eval_update`` (boxes) or, with ``segm``,
    of ``coco_segm_eval_update`` (counts).  Host only."""
    lib = _lib.load(require_gpu=False)
    return _mh_name(lib.frcnn_coco_eval_kernel, "coco_eval_kernel", int(bool(segm)))


def mask_overlap_workspace_size(N, D, G, H, W) -> int:
    """frcnn_mask_overlap_workspace_size (0 outside the limits).  Host only."""
    return int(_lib.load(require_gpu=False).frcnn_mask_overlap_workspace_size(int(N), int(D), int(G), int(H), int(W)))


def mask_overlap(det_masks, gt_masks, *, det_labels=None, det_count=None, gt_labels=None, n_class=None, out=None,
                 workspace=None):
    """Pixel counts of a batch of masks and of their pairwise intersections
    (frcnn_mask_overlap; DESIGN.md "COCO segm evaluation" is the contract).

    ``det_masks`` uint8 [N, D, H, W] (``mask_head_paste``'s with a threshold) and ``gt_masks``
    uint8 [N, G, H, W] on the same canvas; a pixel is set iff its byte is non-zero.
    ``det_count`` int32 [N] (None: every row is a detection).  With ``det_labels`` int32
    [N, D], ``gt_labels`` int32 [N, G] and ``n_class`` a pair is considered iff d <
    det_count[n], the labels are equal and in [1, n_class); without labels every pair with
    d < det_count[n] is.

    Returns ``MaskOverlap(inter int32 [N, D, G], det_area int32 [N, D], gt_area int32 [N, G])``:
    ``inter`` is 0 for a pair that is not considered, ``det_area`` 0 at or beyond ``det_count``
    (those masks are not read).  Exact, and the same bits from call to call.

    A hot-path op: nothing is converted; a wrong dtype, shape, device, canvas or a strided view
    raises RuntimeError naming the argument before any launch.  ``out``: the three outputs,
    caller-owned; ``workspace``: a uint8 device tensor of at least
    ``mask_overlap_workspace_size`` bytes."""
    op = "mask_overlap"
    lib = _lib.load()
    for name, t in (("det_masks", det_masks), ("gt_masks", gt_masks)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise RuntimeError(f"{op}: {name} must be a uint8 device tensor of shape [N, {name[0].upper()}, H, W]")
    N, D, H, W = (int(v) for v in det_masks.shape)
    G = int(gt_masks.shape[1])
    if tuple(gt_masks.shape[2:]) != (H, W):
        raise RuntimeError(f"{op}: gt_masks: canvas {tuple(gt_masks.shape[2:])} is not det_masks' canvas {(H, W)}")
    if not (1 <= N <= MASK_OVERLAP_MAX_N and 1 <= D <= MASK_OVERLAP_MAX_D and 0 <= G <= MASK_OVERLAP_MAX_G
            and 1 <= H <= MASK_OVERLAP_MAX_DIM and 1 <= W <= MASK_OVERLAP_MAX_DIM
            and H * W <= MASK_OVERLAP_MAX_PIXELS):
        raise RuntimeError(f"{op}: det_masks / gt_masks: N={N} must be in [1, {MASK_OVERLAP_MAX_N}], D={D} in "
                           f"[1, {MASK_OVERLAP_MAX_D}], G={G} in [0, {MASK_OVERLAP_MAX_G}], H={H} and W={W} in "
                           f"[1, {MASK_OVERLAP_MAX_DIM}] with H*W <= 2^24")
    _require(op, "det_masks", det_masks, torch.uint8, (N, D, H, W))
    _require(op, "gt_masks", gt_masks, torch.uint8, (N, G, H, W))
    if (det_labels is None) != (gt_labels is None):
        raise RuntimeError(f"{op}: det_labels and gt_labels are given together or not at all")
    C = 0
    if det_labels is not None:
        if n_class is None or not 2 <= int(n_class) <= MASK_OVERLAP_MAX_C:
            raise RuntimeError(f"{op}: n_class must be in [2, {MASK_OVERLAP_MAX_C}] with labels; got {n_class}")
        C = int(n_class)
        _require(op, "det_labels", det_labels, torch.int32, (N, D))
        _require(op, "gt_labels", gt_labels, torch.int32, (N, G))
    if det_count is not None:
        _require(op, "det_count", det_count, torch.int32, (N,))
    dev = det_masks.device
    for name, t in (("gt_masks", gt_masks), ("det_labels", det_labels), ("det_count", det_count),
                    ("gt_labels", gt_labels)):
        if t is not None and t.device != dev:
            raise RuntimeError(f"{op}: {name} is on {t.device} but det_masks on {dev}")
    if det_masks.data_ptr() % 16 or gt_masks.data_ptr() % 16:
        raise RuntimeError(f"{op}: det_masks / gt_masks must be 16-byte aligned (a view into a larger tensor?)")
    shapes = ((N, D, G), (N, D), (N, G))
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.int32, device=dev) for s in shapes)
    else:
        if len(out) != 3:
            raise RuntimeError(f"{op}: out must be (inter, det_area, gt_area)")
        for name, t, s in zip(MaskOverlap._fields, out, shapes):
            _require(op, f"out.{name}", t, torch.int32, s)
    key = (N, D, G, H, W)
    need = _mo_ws.get(key)
    if need is None:
        need = _mo_ws[key] = int(lib.frcnn_mask_overlap_workspace_size(N, D, G, H, W))
    ws = workspace if workspace is not None else _lib.cached_workspace(op, need, dev)
    if not isinstance(ws, torch.Tensor) or ws.dtype != torch.uint8 or not ws.is_cuda or ws.numel() < need:
        raise RuntimeError(f"{op}: workspace must be a uint8 device tensor of at least {need} B")
    _lib.check(lib.frcnn_mask_overlap(N, D, G, H, W, C, _lib.ptr(det_masks), _lib.ptr(gt_masks),
                                      _lib.ptr(det_labels), _lib.ptr(det_count), _lib.ptr(gt_labels),
                                      _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.ptr(ws), ws.numel(),
                                      _lib.stream_ptr()), op)
    return MaskOverlap(*out)


def coco_segm_eval_update(det, overlap, gt_labels: torch.Tensor, gt_crowd: torch.Tensor = None, *,
                          gt_area: torch.Tensor = None, state) -> None:
    """``coco_eval_update`` with iouType "segm" (frcnn_coco_segm_eval_update; DESIGN.md "COCO
    segm evaluation"): the same records into the same ``state``, so ``coco_eval_accumulate``
    closes it unchanged -- stream-ordered, no allocation, no host synchronisation.

    ``det`` is ``(labels, scores, count)`` or a ``BoxDetections``; ``overlap`` the
    ``MaskOverlap`` of ``mask_overlap``'s labelled form for the same labels and count.  The IoU of
    a pair is 0 without a common pixel, ``i / a_d`` against a crowd gt and ``i / (a_d + a_g - i)``
    otherwise; a detection's area is its pixel count; a gt's area for the size ranges is
    ``gt_area`` (fp64 [N, G], the annotation's field) when given, else its pixel count."""
    op = "coco_segm_eval_update"
    lib = _lib.load()
    if isinstance(det, BoxDetections):
        labels, scores, count = det.labels, det.scores, det.count
    elif len(det) == 3:
        labels, scores, count = det
    else:
        raise RuntimeError(f"{op}: det must be (labels, scores, count) or a BoxDetections")
    if not isinstance(overlap, tuple) or len(overlap) != 3:
        raise RuntimeError(f"{op}: overlap must be ops.mask_overlap's MaskOverlap")
    inter, det_pix, gt_pix = overlap
    C, cap = _coco_state_check(state, op)
    if not isinstance(labels, torch.Tensor) or labels.dim() != 2 or not isinstance(gt_labels, torch.Tensor) \
            or gt_labels.dim() != 2:
        raise RuntimeError(f"{op}: det labels must be [N, M] and gt_labels [N, G]")
    N, M = (int(v) for v in labels.shape)
    G = int(gt_labels.shape[1])
    ins = [("det.labels", labels, torch.int32, (N, M)), ("det.scores", scores, torch.float32, (N, M)),
           ("det.count", count, torch.int32, (N,)), ("overlap.inter", inter, torch.int32, (N, M, G)),
           ("overlap.det_area", det_pix, torch.int32, (N, M)), ("overlap.gt_area", gt_pix, torch.int32, (N, G)),
           ("gt_labels", gt_labels, torch.int32, (N, G))]
    if gt_crowd is not None:
        ins.append(("gt_crowd", gt_crowd, torch.uint8, (N, G)))
    if gt_area is not None:
        ins.append(("gt_area", gt_area, torch.float64, (N, G)))
    for name, t, dt, shape in ins:
        _require(op, name, t, dt, shape)
    hdr, key, bits, tables = state
    _lib.check(lib.frcnn_coco_segm_eval_update(N, M, G, C, cap, _lib.ptr(labels), _lib.ptr(scores), _lib.ptr(count),
                                               _lib.ptr(inter), _lib.ptr(det_pix), _lib.ptr(gt_pix),
                                               _lib.ptr(gt_labels), _lib.ptr(gt_crowd), _lib.ptr(gt_area),
                                               _lib.ptr(tables), _lib.ptr(hdr), _lib.ptr(key), _lib.ptr(bits),
                                               _lib.stream_ptr()), op)


# ------------------------------------------------------------- RPN epilogue
class _RPNHeadEpilogueFunction(torch.autograd.Function):
    """nets/rpn.py:117-124 as one launch.  The backward of the two permutes is
    the inverse permute (plain tensor ops, in the gradients' own dtype); the fg
    scores feed only the (non-differentiable) proposal layer, as in the
    reference.  float16 / bfloat16 inputs give a fourth output, the fp32 deltas."""

    @staticmethod
    def forward(ctx, cls, reg, K):
        lib = _lib.load()
        N, C2, H, W = cls.shape
        if C2 != 2 * K or tuple(reg.shape) != (N, 4 * K, H, W):
            raise RuntimeError(f"rpn_head_epilogue: cls {tuple(cls.shape)} / reg {tuple(reg.shape)} "
                               f"do not match K={K}")
        A = H * W * K
        dt = cls.dtype  # fp32, or the 16-bit type both conv outputs share (rpn_head_epilogue's rule)
        cls_nhwc = torch.empty((N, A, 2), dtype=dt, device=cls.device)
        fg = torch.empty((N, A), dtype=torch.float32, device=cls.device)
        reg_nhwc = torch.empty((N, A, 4), dtype=dt, device=cls.device)
        if dt == torch.float32:
            _lib.check(lib.frcnn_rpn_head_epilogue(_lib.ptr(cls), _lib.ptr(reg), N, K, H, W,
                                                   _lib.ptr(cls_nhwc), _lib.ptr(fg), _lib.ptr(reg_nhwc),
                                                   _lib.stream_ptr()), "rpn_head_epilogue")
            deltas = None  # reg_nhwc is the proposal layer's input (rpn_head_epilogue_with_deltas)
        else:
            deltas = torch.empty((N, A, 4), dtype=torch.float32, device=cls.device)
            _lib.check(lib.frcnn_rpn_head_epilogue_t(_lib.DTYPE_CODES[dt], _lib.ptr(cls), _lib.ptr(reg), N, K, H, W,
                                                     _lib.ptr(cls_nhwc), _lib.ptr(fg), _lib.ptr(reg_nhwc),
                                                     _lib.ptr(deltas), _lib.stream_ptr()), "rpn_head_epilogue")
        ctx.meta = (N, K, H, W)
        if deltas is None:
            ctx.mark_non_differentiable(fg)
            return cls_nhwc, fg, reg_nhwc
        ctx.mark_non_differentiable(fg, deltas)
        return cls_nhwc, fg, reg_nhwc, deltas

    @staticmethod
    def backward(ctx, g_cls, _g_fg, g_reg, _g_deltas=None):
        N, K, H, W = ctx.meta
        gc = gr = None
        if g_cls is not None:
            gc = g_cls.reshape(N, H, W, 2 * K).permute(0, 3, 1, 2).contiguous()
        if g_reg is not None:
            gr = g_reg.reshape(N, H, W, 4 * K).permute(0, 3, 1, 2).contiguous()
        return gc, gr, None


def _epilogue_inputs(cls, reg):
    if not isinstance(cls, torch.Tensor) or not isinstance(reg, torch.Tensor) or cls.dim() != 4 or reg.dim() != 4:
        raise RuntimeError("rpn_head_epilogue: cls and reg must be NCHW")
    if cls.dtype in _POOL_HALF or reg.dtype in _POOL_HALF:
        if reg.dtype != cls.dtype:
            raise RuntimeError(f"rpn_head_epilogue: reg is {reg.dtype} but cls is {cls.dtype}; a float16 or "
                               "bfloat16 conv output needs its partner in the same dtype")
        return _to_dev(cls, cls.dtype), _to_dev(reg, reg.dtype)  # moved / made contiguous if needed, never widened
    return cls.float().contiguous(), reg.float().contiguous()


def rpn_head_epilogue_with_deltas(cls: torch.Tensor, reg: torch.Tensor, K: int):
    """``rpn_head_epilogue`` plus the proposal layer's deltas: (cls_nhwc, fg,
    reg_nhwc, deltas).  ``deltas`` is fp32 [N,A,4] and non-differentiable: for
    fp32 inputs ``reg_nhwc`` itself (detached), for float16 / bfloat16 inputs the
    widened ``reg_nhwc``, written by the same launch -- feed it to ``propose``."""
    c, r = _epilogue_inputs(cls, reg)
    out = _RPNHeadEpilogueFunction.apply(c, r, int(K))
    return out if len(out) == 4 else (*out, out[2].detach())


def rpn_head_epilogue(cls: torch.Tensor, reg: torch.Tensor, K: int):
    """nets/rpn.py:117-124: conv outputs cls [N,2K,H,W], reg [N,4K,H,W] (device)
    -> (cls_nhwc [N,A,2], fg [N,A], reg_nhwc [N,A,4]), A = H*W*K.
    ``cls_nhwc.permute(0, 2, 1)`` is the reference's returned ``cls``; ``fg`` is
    its ``cls_fg_softmax``; ``reg_nhwc`` its ``reg``.

    float16 / bfloat16 conv outputs (a network under autocast; both of the same
    dtype, RuntimeError otherwise) keep their type: ``cls_nhwc`` and ``reg_nhwc``
    then have the inputs' dtype and exactly their bit patterns (they were fp32
    before this op read 16-bit inputs itself), the gradients arrive in that dtype,
    and ``fg`` stays fp32, bit-equal to the fp32 op's on the widened inputs
    (DESIGN.md §3 "Predictions in 16-bit types").  Every other dtype is
    converted to fp32 as before."""
    return rpn_head_epilogue_with_deltas(cls, reg, K)[:3]


def roi_transform(rois: torch.Tensor, roi_inds: torch.Tensor, img_h, img_w, feat_h: int,
                  feat_w: int) -> torch.Tensor:
    """nets/heads.py:42-47 on device: fp32 [R,4] image rois + fp32 [R] inds ->
    fp32 [R,5].  A hot-path op: ``rois`` and ``roi_inds`` must be contiguous fp32
    device tensors of these shapes (RuntimeError naming the argument otherwise;
    attribute reads only, before any launch)."""
    lib = _lib.load()
    if not isinstance(rois, torch.Tensor) or rois.dim() != 2:
        raise RuntimeError("roi_transform: rois must be a contiguous torch.float32 device tensor of shape [R, 4]")
    R = rois.size(0)
    _require("roi_transform", "rois", rois, torch.float32, (R, 4))
    _require("roi_transform", "roi_inds", roi_inds, torch.float32, (R,))
    out = torch.empty((R, 5), dtype=torch.float32, device=rois.device)
    _lib.check(lib.frcnn_roi_transform(_lib.ptr(rois), _lib.ptr(roi_inds), R, float(img_h),
                                       float(img_w), int(feat_h), int(feat_w), _lib.ptr(out),
                                       _lib.stream_ptr()), "roi_transform")
    return out


# -------------------------------------------------------------------- losses
_losses_ws = {}  # workspace size per (rows, C) (asked once)


class _LossesFunction(torch.autograd.Function):
    """frcnn_losses_fwd / frcnn_losses_bwd of one stage.  ``cls`` is [N, L, C]
    contiguous, or (``permuted``) the [N, C, L] view of one; P = 1 (RPN) or C
    (head).  The backward hands the incoming gradients to the kernel as device
    pointers (an unused loss: None -> NULL -> that gradient all zero)."""

    @staticmethod
    def forward(ctx, cls, reg, reg_t, labels, sigma, P, permuted):
        lib = _lib.load()
        code = _lib.DTYPE_CODES[cls.dtype]  # cls and reg share it (_losses)
        N, L, C = cls.permute(0, 2, 1).shape if permuted else cls.shape
        rows = N * L
        dev = cls.device
        loss = torch.empty(2, dtype=torch.float32, device=dev)
        stats = torch.empty(4, dtype=torch.int32, device=dev)
        need = _losses_ws.get((rows, C))
        if need is None:
            need = _losses_ws[(rows, C)] = int(lib.frcnn_losses_workspace_size(rows, C))
        ws = _lib.cached_workspace("losses", need, dev)
        f64 = int(labels.dtype == torch.float64)
        _lib.check(lib.frcnn_losses_fwd_t(code, rows, C, P, _lib.ptr(cls), _lib.ptr(reg), _lib.ptr(reg_t),
                                          _lib.ptr(labels), f64, sigma, _lib.ptr(loss), _lib.ptr(stats),
                                          _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "losses forward")
        ctx.save_for_backward(cls, reg, reg_t, labels, stats)
        ctx.meta = (N, L, C, P, f64, sigma, permuted, code)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(stats)
        return loss[0], loss[1], stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_cls, g_reg, _g_stats):
        lib = _lib.load()
        cls, reg, reg_t, labels, stats = ctx.saved_tensors
        N, L, C, P, f64, sigma, permuted, code = ctx.meta
        for name, g in (("cls_loss", g_cls), ("reg_loss", g_reg)):
            if g is not None and (g.dtype != torch.float32 or not g.is_cuda or g.numel() != 1):
                raise RuntimeError(f"losses backward: the gradient of {name} must be one torch.float32 on the "
                                   f"device; got {g.dtype} on {g.device.type} with {g.numel()} elements")
        # gradients in the predictions' dtype: the kernel rounds each fp32 value once, at its store
        dcls = torch.empty((N, L, C), dtype=cls.dtype, device=cls.device)
        dreg = torch.empty((N, L, 4 * P), dtype=cls.dtype, device=cls.device)
        _lib.check(lib.frcnn_losses_bwd_t(code, N * L, C, P, _lib.ptr(cls), _lib.ptr(reg), _lib.ptr(reg_t),
                                          _lib.ptr(labels), f64, sigma, _lib.ptr(stats), _lib.ptr(g_cls),
                                          _lib.ptr(g_reg), _lib.ptr(dcls), _lib.ptr(dreg), _lib.stream_ptr()),
                   "losses backward")
        return (dcls.permute(0, 2, 1) if permuted else dcls), dreg, None, None, None, None, None


def _losses(op, cls, reg, reg_targets, labels, sigma, head, return_stats):
    if (not isinstance(labels, torch.Tensor) or labels.dim() != 2
            or labels.dtype not in (torch.int32, torch.float64)):
        got = f"{labels.dtype} tensor of shape {list(labels.shape)}" if isinstance(labels, torch.Tensor) \
            else type(labels).__name__
        raise RuntimeError(f"{op}: labels must be a contiguous torch.int32 or torch.float64 device tensor of shape "
                           f"[N, L]; got a {got}")
    N, L = labels.shape
    _require(op, "labels", labels, labels.dtype, (N, L))
    if not isinstance(cls, torch.Tensor) or cls.dim() != 3:
        raise RuntimeError(f"{op}: cls must be a contiguous torch.float32 device tensor of shape [N, L, C] (or the "
                           "[N, C, L] permuted view of one)")
    # [N, L, C] as it lies in memory, or the [N, C, L] view RPN.forward / ResnetHead.forward return
    permuted = not cls.is_contiguous() and cls.permute(0, 2, 1).is_contiguous()
    rows_first = cls.permute(0, 2, 1) if permuted else cls
    C = rows_first.shape[2]
    # fp32, or float16 / bfloat16 predictions of a network under autocast: cls and reg in one dtype
    dt = cls.dtype if cls.dtype in _POOL_HALF else torch.float32
    _require(op, "cls", rows_first, dt, (N, L, C))
    P = C if head else 1
    _require(op, "reg", reg, dt, (N, L, 4 * P))
    _require(op, "reg_targets", reg_targets, torch.float64, (N, L, 4))
    if not 2 <= C <= 128:
        raise RuntimeError(f"{op}: cls has C={C} classes; must be in [2, 128]")
    sigma = float(sigma)
    if not 0.0 < sigma < float("inf"):
        raise RuntimeError(f"{op}: sigma={sigma} must be positive and finite")
    out = _LossesFunction.apply(cls, reg, reg_targets, labels, sigma, P, permuted)
    return out if return_stats else out[:2]


def rpn_losses(cls: torch.Tensor, reg: torch.Tensor, reg_targets: torch.Tensor, labels: torch.Tensor,
               sigma: float = 1):
    """The RPN's two losses (train.py:81-83) in one fused op with its own
    backward (frcnn_losses_fwd / _bwd; DESIGN.md "Losses" is the contract):
    cross-entropy over the anchors with label != -1 and smooth-L1 over those
    with label > 0, divided by max(#positives, 1).

    cls fp32 [N, A, 2] -- or the [N, 2, A] view of one that ``RPN.forward``
    returns, accepted as it is --, reg fp32 [N, A, 4] (or both float16 / both
    bfloat16, the predictions of a network under autocast: widened exactly in
    the kernels, losses bit-equal to the fp32 op's on the widened inputs, the
    gradients in that dtype, each the fp32 gradient rounded once), reg_targets fp64
    [N, A, 4] and labels int32 (or fp64) [N, A] exactly as
    ``targets.anchor_targets`` returns them.  Returns (cls_loss, reg_loss), 0-dim
    fp32 device tensors.

    A hot-path op: nothing is converted, nothing synchronises.  Every input must
    be a contiguous device tensor of the dtype and exact shape above
    (RuntimeError naming the argument otherwise; attribute reads only, before
    any launch).  Labels outside -1..C-1 are skipped and counted (stats[2] of
    the C-ABI call), never used as an index.  Values in unlabelled rows, NaN
    included, influence neither the losses nor the gradients (torch's dense
    backward would let a NaN logit through; finite inputs are the contract)."""
    return _losses("rpn_losses", cls, reg, reg_targets, labels, sigma, False, False)


def head_losses(cls: torch.Tensor, reg: torch.Tensor, reg_targets: torch.Tensor, labels: torch.Tensor,
                sigma: float = 1):
    """The head's two losses (train.py:112-121) as ``rpn_losses``: cls fp32
    [N, S, C] (or ``ResnetHead.forward``'s [N, C, S] view), reg fp32 [N, S, 4C]
    ungathered -- a sample with label c uses columns 4c..4c+3, the ``reg_ind``
    gather of train.py:112-117 done inside the kernel --, reg_targets fp64
    [N, S, 4] and labels fp64 (or int32) [N, S] exactly as
    ``targets.proposal_targets`` returns them (fp64 labels truncate toward zero,
    as ``.type(LongTensor)``).  2 <= C <= 128."""
    return _losses("head_losses", cls, reg, reg_targets, labels, sigma, True, False)


def losses_with_stats(cls, reg, reg_targets, labels, sigma=1, head=False):
    """``rpn_losses`` / ``head_losses`` (``head``) also returning the int32 [4]
    device tensor (n_valid, n_pos, n_skipped, 0) of the forward."""
    return _losses("losses_with_stats", cls, reg, reg_targets, labels, sigma, head, True)


# -------------------------------------------------------------- preprocessing
IMAGE_MEAN = (0.485, 0.456, 0.406)   # utils/data_loader.py:72
IMAGE_STD = (0.229, 0.224, 0.225)
PREPROCESS_MAX_RATIO = 5             # an axis may shrink by at most this factor
_preprocess_cache = {}  # (N, max_h, max_w, out_h, out_w, mean, std) -> (mean[3], std[3], workspace bytes)


def _out_size(op, out_size):
    try:
        out_h, out_w = (int(v) for v in out_size)
    except (TypeError, ValueError):
        raise RuntimeError(f"{op}: out_size must be (out_h, out_w); got {out_size!r}") from None
    return out_h, out_w


def preprocess(pixels: torch.Tensor, offset: torch.Tensor, hw: torch.Tensor, out_size=(600, 600),
               mean=IMAGE_MEAN, std=IMAGE_STD, max_hw=None, out=None, status=None):
    """The image half of ``voc_data.__getitem__`` (utils/data_loader.py:38,61-75)
    for a batch on the device (frcnn_preprocess; DESIGN.md "Preprocessing" is
    the contract): ``skimage.transform.resize`` to ``out_size`` with its
    defaults, ``ToTensor`` and ``Normalize``, one launch.

    pixels uint8 [B]: image n is ``hw[n] = (h, w)`` HWC RGB bytes at
    ``offset[n]`` (``data.pack_images`` builds all three); offset int64 [N], hw
    int32 [N, 2].  ``max_hw`` = host-known (max h, max w) of the batch: it sizes
    the launch, no size is read back.  Without it the largest sizes the kernel
    accepts (5x ``out_size``) are assumed, which is correct for every batch but
    runs small tiles -- pass it.  Returns (images fp32 [N, 3, out_h, out_w],
    status int32 [N]): status 0 ok, 1 a size outside 1..max or an axis shrinking
    by more than 5, 2 an offset outside ``pixels``; an image with a nonzero
    status is never read and comes out as zeros.  No synchronisation.

    A hot-path op: every tensor must be a contiguous device tensor of the dtype
    and exact shape above (RuntimeError naming the argument otherwise)."""
    lib = _lib.load()
    op = "preprocess"
    if not isinstance(pixels, torch.Tensor) or pixels.dim() != 1:
        raise RuntimeError(f"{op}: pixels must be a contiguous torch.uint8 device tensor of shape [B]")
    _require(op, "pixels", pixels, torch.uint8, (pixels.shape[0],))
    if not isinstance(offset, torch.Tensor) or offset.dim() != 1:
        raise RuntimeError(f"{op}: offset must be a contiguous torch.int64 device tensor of shape [N]")
    N = offset.shape[0]
    _require(op, "offset", offset, torch.int64, (N,))
    _require(op, "hw", hw, torch.int32, (N, 2))
    out_h, out_w = _out_size(op, out_size)
    if max_hw is None:
        max_hw = (min(PREPROCESS_MAX_RATIO * out_h, 16384), min(PREPROCESS_MAX_RATIO * out_w, 16384))
    max_h, max_w = (int(v) for v in max_hw)
    key = (N, max_h, max_w, out_h, out_w, tuple(float(v) for v in mean), tuple(float(v) for v in std))
    cached = _preprocess_cache.get(key)
    if cached is None:
        if len(key[5]) != 3 or len(key[6]) != 3:
            raise RuntimeError(f"{op}: mean and std must have 3 values")
        need = int(lib.frcnn_preprocess_workspace_size(N, max_h, max_w, out_h, out_w))
        if need == 0:
            raise RuntimeError(f"{op}: N={N} must be in [1, 1024], out_size=({out_h}, {out_w}) in [1, 4096] and "
                               f"max_hw=({max_h}, {max_w}) in [1, 16384]")
        cached = ((_lib.F32 * 3)(*key[5]), (_lib.F32 * 3)(*key[6]), need)
        _preprocess_cache[key] = cached
    mean_c, std_c, need = cached
    dev = pixels.device
    if out is None:
        out = torch.empty((N, 3, out_h, out_w), dtype=torch.float32, device=dev)
    else:
        _require(op, "out", out, torch.float32, (N, 3, out_h, out_w))
    if status is None:
        status = torch.empty((N,), dtype=torch.int32, device=dev)
    else:
        _require(op, "status", status, torch.int32, (N,))
    ws = _lib.cached_workspace("preprocess", need, dev)
    _lib.check(lib.frcnn_preprocess(N, _lib.ptr(pixels), pixels.shape[0], _lib.ptr(offset), _lib.ptr(hw), max_h, max_w,
                                    out_h, out_w, mean_c, std_c, _lib.ptr(out), _lib.ptr(status), _lib.ptr(ws),
                                    ws.numel(), _lib.stream_ptr()), op)
    return out, status


def rescale_boxes(boxes: torch.Tensor, hw: torch.Tensor, out_size=(600, 600)) -> torch.Tensor:
    """``data.rescale_boxes`` (utils/data_loader.py:66-69) for a batch on the
    device, bit-exact with it (frcnn_rescale_boxes): boxes fp64 [N, G, 4] as
    [ymin, xmin, ymax, xmax] in each image's own pixels, hw int32 [N, 2] ->
    fp64 [N, G, 4] in ``out_size`` pixels, every negative entry -1; an image
    with h < 1 or w < 1 gets all -1.  A hot-path op, as ``preprocess``."""
    lib = _lib.load()
    op = "rescale_boxes"
    if not isinstance(boxes, torch.Tensor) or boxes.dim() != 3:
        raise RuntimeError(f"{op}: boxes must be a contiguous torch.float64 device tensor of shape [N, G, 4]")
    N, G = boxes.shape[:2]
    _require(op, "boxes", boxes, torch.float64, (N, G, 4))
    _require(op, "hw", hw, torch.int32, (N, 2))
    out_h, out_w = _out_size(op, out_size)
    out = torch.empty_like(boxes)
    _lib.check(lib.frcnn_rescale_boxes(N, G, _lib.ptr(boxes), _lib.ptr(hw), out_h, out_w, _lib.ptr(out),
                                       _lib.stream_ptr()), op)
    return out
