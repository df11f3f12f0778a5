"""numpy restatement of the detection contract (DESIGN.md "Detections"), built
from the oracle's ``exp_cr``, ``reg2bbox`` and ``nms``.  A helper for the
detect tests, not a test: it returns the six arrays ``ops.detect`` returns."""
import numpy as np

from oracle import ref_numpy as orc

REG_MEAN = (0.0, 0.0, 0.0, 0.0)
REG_STD = (0.1, 0.1, 0.2, 0.2)


def softmax(x):
    """[k, C] logits -> probabilities: e = exp_cr(x - max), s summed in fp32 in
    ascending class order, p = e * (1 / s)."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        e = orc.exp_cr(x - x.max(axis=1, keepdims=True))
        s = e[:, 0].copy()
        for c in range(1, x.shape[1]):
            s = s + e[:, c]
        return e * (np.float32(1) / s)[:, None]


def candidates(rois, rcount, cls, n, score_thresh):
    """Per class c >= 1 of image n: candidate rows (ascending)."""
    R, C = cls.shape[1:]
    k = int(np.clip(rcount[n], 0, R))
    p = softmax(cls[n, :k]) if k else np.zeros((0, C), np.float32)
    with np.errstate(invalid="ignore"):
        return p, [np.nonzero(p[:, c] > np.float32(score_thresh))[0] for c in range(1, C)]


def detect(rois, rcount, cls, reg, img_h, img_w, score_thresh=0.05, nms_thresh=0.3, reg_mean=REG_MEAN,
           reg_std=REG_STD, max_det=None):
    rois = np.asarray(rois, np.float32)
    cls = np.asarray(cls, np.float32)
    reg = np.asarray(reg, np.float32)
    N, R, C = cls.shape
    if max_det is None:
        max_det = R * (C - 1)
    mean = np.asarray(reg_mean, np.float32)
    std = np.asarray(reg_std, np.float32)
    boxes = np.zeros((N, max_det, 4), np.float32)
    labels = np.full((N, max_det), -1, np.int32)
    scores = np.zeros((N, max_det), np.float32)
    roi = np.full((N, max_det), -1, np.int32)
    count = np.zeros(N, np.int32)
    total = np.zeros(N, np.int32)
    for n in range(N):
        p, cand = candidates(rois, rcount, cls, n, score_thresh)
        ob, ol, osc, orow = [], [], [], []
        for c in range(1, C):
            rows = cand[c - 1]
            if len(rows) == 0:
                continue
            loc = reg[n, rows, 4 * c:4 * c + 4] * std
            loc = loc + mean
            b = orc.reg2bbox(rois[n, rows], loc)
            b[:, [0, 2]] = np.clip(b[:, [0, 2]], np.float32(0), np.float32(img_h))
            b[:, [1, 3]] = np.clip(b[:, [1, 3]], np.float32(0), np.float32(img_w))
            keep = orc.nms(b, p[rows, c], nms_thresh)   # stable: ties by ascending row
            ob.append(b[keep])
            ol.append(np.full(len(keep), c, np.int32))
            osc.append(p[rows, c][keep])
            orow.append(rows[keep].astype(np.int32))
        if ob:
            ob, ol, osc, orow = (np.concatenate(a) for a in (ob, ol, osc, orow))
            total[n] = len(ol)
            k = count[n] = min(len(ol), max_det)
            boxes[n, :k], labels[n, :k], scores[n, :k], roi[n, :k] = ob[:k], ol[:k], osc[:k], orow[:k]
    return boxes, labels, scores, roi, count, total
