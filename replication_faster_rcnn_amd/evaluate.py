"""PASCAL VOC and COCO-style evaluation of the detector on the device.

The reference stops before this stage (its ``test_eval.py`` is an empty
file); the protocol is the VOC devkit's ``voc_eval``, stated as a contract in
DESIGN.md "Evaluation".  ``VOCEvaluator.update`` scores one inference batch
against its ground truth with ``ops.eval_update`` -- stream-ordered, no
allocation, no host read -- and ``result`` closes the dataset with
``ops.eval_ap``: the only place that synchronises.

    ev = VOCEvaluator()
    for x, gt_boxes, gt_labels, gt_difficult in loader:
        model.predict(x, width, height)
        ev.update(model.last_detections, gt_boxes, gt_labels, gt_difficult)
    print(ev.result()["map"])

``COCOEvaluator`` has the same shape for the COCO protocol (DESIGN.md
"COCO-style evaluation"): AP averaged over IoU 0.50:0.05:0.95, AP50, AP75, AP
for small / medium / large objects and AR at 1 / 10 / 100 detections per image,
on ``ops.coco_eval_update`` and ``ops.coco_eval_accumulate``.
``COCOMaskEvaluator`` scores a mask head the same way with iouType "segm"
(DESIGN.md "COCO segm evaluation"), on ``ops.mask_overlap`` and
``ops.coco_segm_eval_update``.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops


def _dev(a, dtype):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return ops._to_dev(t, dtype)


class VOCEvaluator:
    """Accumulates TP / FP / ignored records of every detection in device
    arrays of ``capacity`` records (``ops.eval_state``), for ``n_class`` classes
    with class 0 the background.  ``plus_one`` is the devkit's pixel
    convention (+1 on box heights and widths), ``use_07_metric`` its 11-point
    AP instead of the area under the precision envelope."""

    def __init__(self, n_class: int = 21, capacity: int = 1 << 20, iou_thresh: float = 0.5,
                 use_07_metric: bool = False, plus_one: bool = True):
        self.n_class = int(n_class)
        self.capacity = int(capacity)
        self.iou_thresh = float(iou_thresh)
        self.use_07_metric = bool(use_07_metric)
        self.plus_one = bool(plus_one)
        self.state = ops.eval_state(self.n_class, self.capacity)

    def reset(self) -> None:
        """Back to the empty state (the record arrays need no clearing)."""
        self.state[0].zero_()

    def update(self, det, gt_boxes, gt_labels, gt_difficult=None) -> None:
        """One batch.  ``det``: the tuple ``ops.detect`` returns or
        ``FasterRCNN.last_detections``.  gt as the loader yields it: boxes
        [N, G, 4] and labels [N, G] of any real dtype (the loader's fp64 labels
        are converted; rows outside 1..n_class-1, such as its -1 padding, are
        no gt), ``gt_difficult`` [N, G] or None; numpy arrays and CPU tensors
        are moved to the device.  Nothing is read back."""
        if len(det) == 6:
            det = (det[0], det[1], det[2], det[4])
        if len(det) != 4:
            raise RuntimeError("VOCEvaluator.update: det must be ops.detect's 6-tuple or (boxes, labels, scores, "
                               "count)")
        det = tuple(_dev(t, dt) for t, dt in zip(det, (torch.float32, torch.int32, torch.float32, torch.int32)))
        ops.eval_update(det, _dev(gt_boxes, torch.float64), _dev(gt_labels, torch.int32),
                        None if gt_difficult is None else _dev(gt_difficult, torch.uint8),
                        state=self.state, iou_thresh=self.iou_thresh, plus_one=self.plus_one)

    def result(self) -> dict:
        """{"ap": fp64 [n_class] (NaN for the background and for classes
        without positives), "map", "npos": int64 [n_class], "n_records",
        "n_images"}.  Raises ``FrcnnError`` when a batch was dropped because the
        capacity was too small: the numbers would be of a part of the dataset."""
        hdr = self.state[0].cpu().numpy()
        if hdr[2] != 0:
            raise _lib.FrcnnError(f"VOCEvaluator: {int(hdr[2])} batch(es) did not fit in capacity={self.capacity} "
                                  f"({int(hdr[0])} records held) and were dropped; use a larger capacity")
        ap, mean = ops.eval_ap(self.state, int(hdr[0]), use_07_metric=self.use_07_metric)
        return dict(ap=ap.cpu().numpy(), map=float(mean.item()), npos=hdr[4:].copy(), n_records=int(hdr[0]),
                    n_images=int(hdr[1]))


COCO_STATS = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")


class COCOEvaluator:
    """Accumulates, for every detection, its rank within (image, class) and
    whether it is matched / ignored at each of the ten IoU thresholds and four
    area ranges of the COCO protocol, in device arrays of ``capacity`` records
    (``ops.coco_eval_state``), for ``n_class`` classes with class 0 the
    background."""

    def __init__(self, n_class: int = 21, capacity: int = 1 << 20):
        self.n_class = int(n_class)
        self.capacity = int(capacity)
        self.state = ops.coco_eval_state(self.n_class, self.capacity)

    def reset(self) -> None:
        """Back to the empty state (the record arrays need no clearing)."""
        self.state[0].zero_()

    def update(self, det, gt_boxes, gt_labels, gt_crowd=None) -> None:
        """One batch.  ``det``: the tuple ``ops.detect`` returns or
        ``FasterRCNN.last_detections``.  gt as the loader yields it: boxes
        [N, G, 4] and labels [N, G] of any real dtype (rows outside
        1..n_class-1, such as the loader's -1 padding, are no gt), ``gt_crowd``
        [N, G] or None -- the one gt flag (``ops.coco_eval_update``); pass the
        loader's ``gt_difficult`` to have VOC's difficult objects ignored.
        numpy arrays and CPU tensors are moved to the device.  Nothing is read
        back."""
        if len(det) == 6:
            det = (det[0], det[1], det[2], det[4])
        if len(det) != 4:
            raise RuntimeError("COCOEvaluator.update: det must be ops.detect's 6-tuple or (boxes, labels, scores, "
                               "count)")
        det = tuple(_dev(t, dt) for t, dt in zip(det, (torch.float32, torch.int32, torch.float32, torch.int32)))
        ops.coco_eval_update(det, _dev(gt_boxes, torch.float64), _dev(gt_labels, torch.int32),
                             None if gt_crowd is None else _dev(gt_crowd, torch.uint8), state=self.state)

    def result(self) -> dict:
        """{"stats": fp64 [12] in pycocotools' order, each of them by name ("AP",
        "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm",
        "ARl"), "ap_per_class": fp64 [n_class], "precision": fp64 [10, 101,
        n_class, 4, 3], "recall": fp64 [10, n_class, 4, 3], "npig": int64
        [n_class, 4], "n_records", "n_images"}; -1 where there is no gt.  The only
        synchronisation.  Raises ``FrcnnError`` when a batch was dropped because
        the capacity was too small: the numbers would be of a part of the
        dataset."""
        hdr = self.state[0].cpu().numpy()
        if hdr[2] != 0:
            raise _lib.FrcnnError(f"COCOEvaluator: {int(hdr[2])} batch(es) did not fit in capacity={self.capacity} "
                                  f"({int(hdr[0])} records held) and were dropped; use a larger capacity")
        precision, recall, stats, apc = ops.coco_eval_accumulate(self.state, int(hdr[0]))
        stats = stats.cpu().numpy()
        out = dict(stats=stats, ap_per_class=apc.cpu().numpy(), precision=precision.cpu().numpy(),
                   recall=recall.cpu().numpy(), npig=hdr[4:].reshape(self.n_class, 4).copy(),
                   n_records=int(hdr[0]), n_images=int(hdr[1]))
        out.update({name: float(v) for name, v in zip(COCO_STATS, stats)})
        return out


class COCOMaskEvaluator(COCOEvaluator):
    """``COCOEvaluator`` with iouType "segm" (DESIGN.md "COCO segm evaluation"): a
    detection is matched by the IoU of its pasted mask with the gt masks, and
    its area is its pixel count.  The records, ``reset`` and ``result`` are the
    parent's."""

    def __init__(self, n_class: int = 21, capacity: int = 1 << 20):
        super().__init__(n_class, capacity)
        self._out = {}   # (N, D, G) -> the MaskOverlap a batch of that shape writes

    def update(self, det, det_masks, gt_masks, gt_labels, gt_crowd=None, gt_area=None) -> None:
        """One batch.  ``det``: ``(labels, scores, count)`` or a ``BoxDetections``;
        ``det_masks`` uint8 [N, D, H, W] as ``ops.mask_head_paste`` returns them with
        a threshold; ``gt_masks`` uint8 [N, G, H, W] on the same canvas (any non-zero
        byte is a set pixel); ``gt_labels`` [N, G], ``gt_crowd`` [N, G] or None,
        ``gt_area`` [N, G] or None: the annotations' ``area`` field, which decides
        the size range of a gt instead of its pixel count.  numpy arrays and CPU
        tensors are moved to the device.  Nothing is read back."""
        if isinstance(det, ops.BoxDetections):
            det = (det.labels, det.scores, det.count)
        if len(det) != 3:
            raise RuntimeError("COCOMaskEvaluator.update: det must be (labels, scores, count) or a BoxDetections")
        labels, scores, count = (_dev(t, dt) for t, dt in zip(det, (torch.int32, torch.float32, torch.int32)))
        det_masks, gt_masks = _dev(det_masks, torch.uint8), _dev(gt_masks, torch.uint8)
        gt_labels = _dev(gt_labels, torch.int32)
        key = (det_masks.shape[0], det_masks.shape[1], gt_masks.shape[1], det_masks.device)
        out = self._out.get(key)
        if out is None:
            N, D, G, dev = key
            out = self._out[key] = tuple(torch.empty(s, dtype=torch.int32, device=dev)
                                         for s in ((N, D, G), (N, D), (N, G)))
        overlap = ops.mask_overlap(det_masks, gt_masks, det_labels=labels, det_count=count, gt_labels=gt_labels,
                                   n_class=self.n_class, out=out)
        ops.coco_segm_eval_update((labels, scores, count), overlap, gt_labels,
                                  None if gt_crowd is None else _dev(gt_crowd, torch.uint8),
                                  gt_area=None if gt_area is None else _dev(gt_area, torch.float64),
                                  state=self.state)
