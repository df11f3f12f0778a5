"""The assembled detector (nets/faster_rcnn.py) on the HIP path.

``FasterRCNN`` keeps the reference constructor (nets/faster_rcnn.py:12-21).
Its ``forward`` is the reference's (nets/faster_rcnn.py:24-34) with the head
called with ``img_h, img_w`` as nets/heads.py:27 requires (the reference's
own call at :32 omits them and cannot run).  ``predict`` is the stage the
reference lacks: head outputs -> per-class decode, score threshold and NMS
for the whole batch in one ``ops.detect`` call.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib, ops

ratios = [0.5, 1., 2.]        # h/w
anchor_scales = [8, 16, 32]   # 128, 256, 512


class FasterRCNN(nn.Module):
    def __init__(self, backbone, rpn, head, mode):
        super().__init__()
        self.backbone, self.classifier = backbone()
        self.rpn = rpn(ratios=ratios, anchor_scales=anchor_scales, mode=mode)
        self.head = head(self.classifier)
        self.mode = mode
        self.last_head_outputs = None
        self.last_detections = None

    def forward(self, x, width, height):
        """-> (cls, reg, rois, roi_inds, cls_output, reg_output, anchors)."""
        features = self.backbone(x)
        cls, reg, rois, roi_inds, anchors = self.rpn(features, width, height)
        cls_output, reg_output = self.head(features, rois, roi_inds, height, width, rois_sorted=True)
        return cls, reg, rois, roi_inds, cls_output, reg_output, anchors

    @torch.no_grad()
    def predict(self, x, width, height, score_thresh=0.05, nms_thresh=0.3, max_det=None):
        """Detections per image: a list of (boxes fp32 [k,4] as [ymin, xmin,
        ymax, xmax], labels int32 [k] in 1..C-1, scores fp32 [k]), class
        ascending then descending score.  The head runs on every RoI slot of
        the RPN's padded output (``rpn.rois_padded``; slots past
        ``rpn.rois_count`` are ignored by ``ops.detect``), so the whole stage
        is fixed-shape; the only host read is the final counts.  The padded
        device tensors stay in ``self.last_detections``, the head outputs as
        ``(cls [N,R,C], reg [N,R,4C])`` in ``self.last_head_outputs``, in
        their own dtype (fp32, or float16 / bfloat16 under autocast)."""
        features = self.backbone(x)
        self.rpn(features, width, height)
        rois_p, cnt = self.rpn.rois_padded, self.rpn.rois_count
        N, R = rois_p.shape[:2]
        roi_inds = torch.arange(N, dtype=torch.float32, device=rois_p.device).repeat_interleave(R)
        cls, reg = self.head(features, rois_p.view(N * R, 4), roi_inds, height, width, rois_sorted=True)
        dev = _lib.device()
        # fp32, or the float16 / bfloat16 a head under autocast returns: ops.detect reads either as it is
        keep = (torch.float32, torch.float16, torch.bfloat16)
        cls = cls.permute(0, 2, 1).to(dev, cls.dtype if cls.dtype in keep else torch.float32).contiguous()
        reg = reg.to(dev, reg.dtype if reg.dtype in keep else torch.float32).contiguous()
        self.last_head_outputs = (cls, reg)
        det = ops.detect(rois_p, cnt, cls, reg, img_h=height, img_w=width, score_thresh=score_thresh,
                         nms_thresh=nms_thresh, max_det=max_det)
        self.last_detections = det
        boxes, labels, scores, _, count, _ = det
        return [(boxes[i, :k].to(x.device), labels[i, :k].to(x.device), scores[i, :k].to(x.device))
                for i, k in enumerate(count.tolist())]

    @torch.no_grad()
    def predict_images(self, images, new_size=(600, 600), score_thresh=0.05, nms_thresh=0.3, max_det=None):
        """``predict`` from decoded images: a list of H x W x 3 uint8 arrays of
        any sizes is resized and normalised on the device
        (``data.Preprocessor``), run through ``predict`` at ``new_size``, and
        each image's boxes are mapped back to its own pixels (rows 0, 2 times
        h / out_h, rows 1, 3 times w / out_w; plain torch on the device).
        Returns ``predict``'s list; ``self.last_detections`` holds the padded
        device tensors with the mapped boxes (padding rows stay 0)."""
        from .data import Preprocessor
        out_h, out_w = int(new_size[0]), int(new_size[1])
        x, _, hw = Preprocessor((out_h, out_w))(images)
        self.predict(x, out_w, out_h, score_thresh=score_thresh, nms_thresh=nms_thresh, max_det=max_det)
        boxes, labels, scores, roi, count, total = self.last_detections
        back = (hw.to(torch.float32) / torch.tensor([out_h, out_w], dtype=torch.float32, device=hw.device)).repeat(1, 2)
        boxes = boxes * back[:, None, :]
        self.last_detections = (boxes, labels, scores, roi, count, total)
        return [(boxes[i, :k], labels[i, :k], scores[i, :k]) for i, k in enumerate(count.tolist())]
