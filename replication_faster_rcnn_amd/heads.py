"""Second-stage head (nets/heads.py) on the HIP path.

``ResnetHead.forward`` keeps the reference signature (nets/heads.py:27).  The
RoI transform + ``[idx, box]`` pack (nets/heads.py:42-47) and RoIPool forward
(nets/heads.py:48) are one HIP launch (``ops.roi_pool_head``) when the RoIs
are grouped by image, with roi_pool's HIP backward; the classifier (layer4 +
avgpool) and the two FCs stay plain PyTorch (not the target).

float16 / bfloat16 features (a backbone under ``torch.autocast``) are pooled
in their own type: ``cropped`` reaches the classifier in ``x``'s dtype and
``x.grad`` comes back in it, with no widening cast on either side.

``ResnetHead(..., pool="align")`` (an extension; the default "max" is the path
above, unchanged) pools with ``ops.roi_align`` instead: ``ops.roi_transform``,
then RoIAlign forward and its deterministic HIP backward (DESIGN.md §3
"RoIAlign"), in ``x``'s dtype as well.

``BoxHeadTraining`` is the training half of a box head on the pyramid path (torchvision's
``RoIHeads.select_training_samples`` and ``fastrcnn_loss``; DESIGN.md §3 "Pyramid box-head
training").  ``BoxHeadDetections`` is the inference half: torchvision's
``RoIHeads.postprocess_detections`` and the transform's ``resize_boxes`` on
``ops.box_head_detections`` (DESIGN.md §3 "Pyramid box-head inference").  ``MaskHeadTraining`` and
``MaskHeadInference`` are the mask head of the same ``RoIHeads`` (``project_masks_on_boxes``,
``maskrcnn_loss``, ``maskrcnn_inference`` + ``paste_masks_in_image``; DESIGN.md §3 "Pyramid mask
head").  All stand beside ``ResnetHead``; neither they nor the pyramid ops are wired into
``FasterRCNN``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib, ops


class ResnetHead(nn.Module):
    def __init__(self, classifier, roi_size=7, spatial_scale=1, n_classes=21, pool="max", sampling_ratio=-1,
                 aligned=False):
        """``pool`` (extension): "max" is the reference's ``roi_pool``; "align" pools with
        ``ops.roi_align`` (``sampling_ratio``, ``aligned`` as torchvision's) on the same
        transformed boxes."""
        super().__init__()
        if pool not in ("max", "align"):
            raise ValueError(f"ResnetHead: pool must be 'max' or 'align'; got {pool!r}")
        self.pool = pool
        self.sampling_ratio = sampling_ratio
        self.aligned = aligned
        self.classifier = classifier
        self.reg = nn.Linear(in_features=512, out_features=n_classes * 4)
        self.cls = nn.Linear(in_features=512, out_features=n_classes)
        self.roi_size = roi_size
        self.spatial_scale = spatial_scale

    def forward(self, x, rois, roi_inds, img_h, img_w, rois_sorted=None):
        """-> (cls [N, n_classes, n_sample], reg [N, n_sample, n_classes*4]).

        ``rois_sorted`` (extension): True promises RoIs grouped by non-decreasing
        image index, as RPN.forward (nets/rpn.py:129-136) and train.py's sampler
        loop (:91-108) produce them -- the one-launch path.  None checks: on the
        host for host-resident indices (the reference's case, no device sync),
        with one device->host sync for device-resident ones."""
        N = x.shape[0]
        dev = _lib.device()
        if rois_sorted is None:
            bi = torch.as_tensor(roi_inds).detach().to(torch.int64)  # host tensors: no sync
            rois_sorted = bool((bi[1:] >= bi[:-1]).all()) if bi.numel() > 1 else True
        r = torch.as_tensor(rois).detach().to(dev, torch.float32).contiguous()
        ri = torch.as_tensor(roi_inds).detach().to(dev, torch.float32).contiguous()
        out_dev = x.device
        if self.pool == "align":
            boxes = ops.roi_transform(r, ri, img_h, img_w, x.shape[2], x.shape[3])
            cropped = ops.roi_align(x, boxes, (self.roi_size, self.roi_size), self.spatial_scale,
                                    self.sampling_ratio, self.aligned)
        else:
            cropped = ops.roi_pool_head(x, r, ri, (self.roi_size, self.roi_size), img_h, img_w,
                                        self.spatial_scale, rois_sorted=bool(rois_sorted))[0].to(out_dev)
        fc6 = self.classifier(cropped)
        fc6 = fc6.view(fc6.shape[0], -1)
        reg = self.reg(fc6)
        cls = self.cls(fc6)
        reg = reg.view(N, -1, reg.shape[-1])
        cls = cls.view(N, -1, cls.shape[-1])
        return cls.permute(0, 2, 1), reg


class BoxHeadTraining(nn.Module):
    """The training half of torchvision's ``RoIHeads`` for a box head on pooled pyramid features:
    ``select_training_samples`` (``add_gt_proposals``, ``Matcher(fg_iou_thresh, bg_iou_thresh,
    allow_low_quality_matches=False)``, ``BalancedPositiveNegativeSampler(batch_size_per_image,
    positive_fraction)``, ``BoxCoder(reg_weights).encode``) on ``ops.box_head_targets`` and
    ``fastrcnn_loss`` on ``ops.box_head_losses``.  The sampler's ``(seed, calls)`` state is a
    buffer of the module, advanced on the device by every ``targets`` call; nothing synchronises.

    ``targets(...).rois`` feeds ``ops.multiscale_roi_align`` as it is; the head's two predictions
    for those rows go to ``losses``."""

    def __init__(self, fg_iou_thresh=0.5, bg_iou_thresh=0.5, batch_size_per_image=512, positive_fraction=0.25,
                 reg_weights=(10, 10, 5, 5), seed=0):
        super().__init__()
        self.fg_iou_thresh = fg_iou_thresh
        self.bg_iou_thresh = bg_iou_thresh
        self.batch_size_per_image = batch_size_per_image
        self.positive_fraction = positive_fraction
        self.reg_weights = tuple(float(w) for w in reg_weights)
        self.register_buffer("rng", ops.sampler_state(seed, device="cpu"))

    def targets(self, proposals, prop_count, gt_boxes, gt_labels, gt_count):
        """-> ``ops.BoxHeadTargets``.  ``proposals`` fp32 [N, R, 4] and ``prop_count`` int32 [N] as
        ``ops.propose_multilevel`` returns them; ``gt_boxes`` fp32 [N, G, 4], ``gt_labels`` int32
        [N, G], ``gt_count`` int32 [N]."""
        if self.rng.device != proposals.device:
            self.rng = self.rng.to(proposals.device)
        return ops.box_head_targets(proposals, prop_count, gt_boxes, gt_labels, gt_count, self.rng,
                                    batch_size_per_image=self.batch_size_per_image,
                                    positive_fraction=self.positive_fraction, fg_iou_thresh=self.fg_iou_thresh,
                                    bg_iou_thresh=self.bg_iou_thresh, reg_weights=self.reg_weights)

    def losses(self, class_logits, box_regression, targets, beta=1 / 9):
        """-> (classification_loss, box_loss) of the head's predictions for ``targets.rois``."""
        return ops.box_head_losses(class_logits, box_regression, targets, beta=beta)


class BoxHeadDetections(nn.Module):
    """The inference half of torchvision's ``RoIHeads`` for a box head on pooled pyramid features:
    ``postprocess_detections`` (softmax, ``BoxCoder(reg_weights).decode``, clip, ``score_thresh``,
    ``remove_small_boxes(min_size)``, class-wise NMS at ``nms_thresh``, the best
    ``detections_per_img``) on ``ops.box_head_detections``; nothing synchronises.

    The result feeds ``evaluate.VOCEvaluator.update`` / ``COCOEvaluator.update`` as it is (boxes are
    (x1, y1, x2, y2): give the ground truth in the same axis order)."""

    def __init__(self, score_thresh=0.05, nms_thresh=0.5, detections_per_img=100, min_size=1e-2,
                 reg_weights=(10, 10, 5, 5)):
        super().__init__()
        self.score_thresh = score_thresh
        self.nms_thresh = nms_thresh
        self.detections_per_img = detections_per_img
        self.min_size = min_size
        self.reg_weights = tuple(float(w) for w in reg_weights)

    def forward(self, class_logits, box_regression, proposals, prop_count, image_sizes, original_sizes=None):
        """-> ``ops.BoxDetections``.  ``class_logits`` [N*R, C] and ``box_regression`` [N*R, 4C]: the
        head's outputs for ``ops.propose_multilevel``'s ``rois``; ``proposals`` / ``prop_count``: its
        ``boxes`` / ``count``; ``image_sizes`` as it takes them; ``original_sizes``: fp32 device
        tensor [N, 2] of (h, w) to map the boxes back to, or None."""
        return ops.box_head_detections(class_logits, box_regression, proposals, prop_count, image_sizes,
                                       score_thresh=self.score_thresh, nms_thresh=self.nms_thresh,
                                       detections_per_img=self.detections_per_img, min_size=self.min_size,
                                       reg_weights=self.reg_weights, original_sizes=original_sizes)


class MaskHeadTraining(nn.Module):
    """The training half of torchvision's ``RoIHeads`` for a mask head on pooled pyramid features:
    the positives of the box head's sample with ``project_masks_on_boxes`` on
    ``ops.mask_head_targets`` and ``maskrcnn_loss`` on ``ops.mask_head_losses`` (DESIGN.md §3
    "Pyramid mask head"); nothing synchronises.

    ``targets(...).rois`` feeds ``ops.multiscale_roi_align`` as it is; the head's logits for those
    rows go to ``losses``.  ``positives_per_image``: the rows kept per image (default: every slot;
    a sampler with ``positive_fraction`` f never yields more than ``int(B * f)``)."""

    def __init__(self, mask_size=28, positives_per_image=None):
        super().__init__()
        self.mask_size = mask_size
        self.positives_per_image = positives_per_image

    def targets(self, box_targets, gt_masks):
        """-> ``ops.MaskHeadTargets``.  ``box_targets``: the ``ops.BoxHeadTargets`` of the box head;
        ``gt_masks``: uint8 device tensor [N, G, Hm, Wm]."""
        return ops.mask_head_targets(box_targets, gt_masks, mask_size=self.mask_size,
                                     positives_per_image=self.positives_per_image)

    def losses(self, mask_logits, targets):
        """-> the mask loss of the head's logits [N*P, C, M, M] for ``targets.rois``."""
        return ops.mask_head_losses(mask_logits, targets)


class MaskHeadInference(nn.Module):
    """The inference half: torchvision's ``maskrcnn_inference`` and ``paste_masks_in_image`` on
    ``ops.mask_head_paste``; nothing synchronises.  ``ops.detection_rois(detections)`` gives the
    RoIs to pool the mask features for."""

    def __init__(self, padding=1, threshold=0.5):
        super().__init__()
        self.padding = padding
        self.threshold = threshold

    def forward(self, mask_logits, detections, canvas_size, image_sizes=None, original_sizes=None):
        """-> masks [N, D, Hc, Wc] (uint8 0 / 1, or fp32 probabilities with ``threshold=None``).
        ``mask_logits`` [N*D, C, M, M]: the head's outputs for ``ops.detection_rois(detections)``;
        ``detections``: the ``ops.BoxDetections`` of the box head."""
        return ops.mask_head_paste(mask_logits, detections.boxes, detections.labels, detections.count, canvas_size,
                                   image_sizes=image_sizes, original_sizes=original_sizes, padding=self.padding,
                                   threshold=self.threshold)
