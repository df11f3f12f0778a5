"""Synthetic VOC-shaped inputs (SURVEY.md §8(d) "Synthetic inputs").

Every array is generated from ``numpy.random.default_rng(seed + image_index)``
so a batch sharded over ranks is bit-identical to the unsharded batch
(P-invariance), and the same inputs can be rebuilt on the GPU box without any
fixture file.  There is no dataset access here (no network): the shapes follow
the reference loader (``utils/data_loader.py:21,88-89,105,115``) and the
BASELINE.json configs.
"""
from __future__ import annotations

import numpy as np

# BASELINE.json configs -> shapes (SURVEY.md §8 header)
CONFIGS = {
    # name: (img_h, img_w, feat_h, feat_w, ratios, scales, pre_nms, post_nms, C, batch)
    "cfg1": dict(img_h=600, img_w=1000, feat_h=38, feat_w=63, scales=(8, 16, 32),
                 pre_nms=12000, post_nms=2000, C=256, batch=1),
    "cfg2": dict(img_h=600, img_w=1000, feat_h=38, feat_w=63, scales=(8, 16, 32),
                 pre_nms=6000, post_nms=300, C=256, batch=8),
    "cfg3": dict(img_h=600, img_w=1000, feat_h=38, feat_w=63, scales=(8, 16, 32),
                 pre_nms=6000, post_nms=300, C=256, batch=64),
    "cfg4": dict(img_h=800, img_w=1333, feat_h=50, feat_w=84, scales=(2, 4, 8, 16, 32),
                 pre_nms=30000, post_nms=2000, C=512, batch=1),
    "cfg5": dict(img_h=600, img_w=600, feat_h=38, feat_w=38, scales=(8, 16, 32),
                 pre_nms=12000, post_nms=600, C=256, batch=16),
}
RATIOS = (0.5, 1.0, 2.0)


def rng_for(seed: int, image_index: int, stream: int = 0) -> np.random.Generator:
    return np.random.default_rng([int(seed), int(image_index), int(stream)])


def rpn_scores(A: int, seed: int, image_index: int) -> np.ndarray:
    """Tie-free fg scores in (0,1): ``(perm(A) + 0.5) / A``."""
    r = rng_for(seed, image_index, 0)
    return ((r.permutation(A).astype(np.float64) + 0.5) / A).astype(np.float32)


def rpn_deltas(A: int, seed: int, image_index: int, sigma: float = 0.2) -> np.ndarray:
    r = rng_for(seed, image_index, 1)
    return (r.standard_normal((A, 4)) * sigma).astype(np.float32)


def features(C: int, H: int, W: int, seed: int, image_index: int) -> np.ndarray:
    r = rng_for(seed, image_index, 2)
    return r.standard_normal((C, H, W), dtype=np.float32)


def head_outputs(N: int, R: int, C: int, img_h: int, img_w: int, seed: int, first_image: int = 0,
                 objects: int = 6):
    """Second-stage inputs of ``ops.detect`` for images ``first_image ..
    first_image+N-1``: (rois fp32 [N,R,4], rcount int32 [N] = R, cls fp32
    [N,R,C] logits, reg fp32 [N,R,4C]).  Per image, ``objects`` boxes with a
    class in 1..C-1 each; two RoIs in three sit on an object (position and size
    jittered), the rest are background boxes anywhere.  Logits are N(0,1), the
    object's class raised by N(5,2), the background class by 3 on background
    RoIs; reg is N(0,0.5)."""
    rois = np.empty((N, R, 4), np.float32)
    cls = np.empty((N, R, C), np.float32)
    reg = np.empty((N, R, 4 * C), np.float32)
    for i in range(N):
        r = rng_for(seed, first_image + i, 4)
        cy = r.uniform(0.15, 0.85, objects) * img_h
        cx = r.uniform(0.15, 0.85, objects) * img_w
        oh = r.uniform(0.15, 0.5, objects) * img_h
        ow = r.uniform(0.15, 0.5, objects) * img_w
        ocls = r.integers(1, C, objects)
        share = r.dirichlet(np.full(objects, 2.0))
        obj = np.where(r.uniform(size=R) < 2.0 / 3.0, r.choice(objects, size=R, p=share), -1)
        y = np.sort(r.uniform(0, img_h, (R, 2)), axis=1)
        x = np.sort(r.uniform(0, img_w, (R, 2)), axis=1)
        box = np.stack([y[:, 0], x[:, 0], np.maximum(y[:, 1], y[:, 0] + 16), np.maximum(x[:, 1], x[:, 0] + 16)], 1)
        on = obj >= 0
        jit = r.standard_normal((R, 4))
        h = oh[obj] * np.exp(0.15 * jit[:, 2])
        w = ow[obj] * np.exp(0.15 * jit[:, 3])
        yy = cy[obj] + 0.1 * oh[obj] * jit[:, 0]
        xx = cx[obj] + 0.1 * ow[obj] * jit[:, 1]
        obox = np.stack([yy - h / 2, xx - w / 2, yy + h / 2, xx + w / 2], 1)
        box = np.where(on[:, None], obox, box)
        box[:, [0, 2]] = np.clip(box[:, [0, 2]], 0, img_h)
        box[:, [1, 3]] = np.clip(box[:, [1, 3]], 0, img_w)
        logit = r.standard_normal((R, C))
        rows = np.arange(R)
        logit[rows[on], ocls[obj[on]]] += 5.0 + 2.0 * r.standard_normal(int(on.sum()))
        logit[rows[~on], 0] += 3.0
        rois[i] = box
        cls[i] = logit
        reg[i] = 0.5 * r.standard_normal((R, 4 * C))
    return rois, np.full((N,), R, np.int32), cls, reg


def gt_boxes(img_h: int, img_w: int, G: int, seed: int, image_index: int, n_valid=None):
    """32-slot padded gt like ``utils/data_loader.py:88-115``: layout
    ``[ymin, xmin, ymax, xmax]`` fp64, ``np.around``-ed; padded rows are -1
    with label -1.  Returns (boxes [G,4] f64, labels [G] f64)."""
    r = rng_for(seed, image_index, 3)
    if n_valid is None:
        n_valid = G
    boxes = -1 * np.ones([G, 4])
    labels = -1 * np.ones(G)
    for g in range(n_valid):
        while True:
            y = np.sort(r.uniform(0, img_h, 2))
            x = np.sort(r.uniform(0, img_w, 2))
            b = np.around(np.array([y[0], x[0], y[1], x[1]]))
            if b[2] - b[0] >= 4 and b[3] - b[1] >= 4:
                break
        boxes[g] = b
        labels[g] = float(r.integers(1, 21))
    return np.around(boxes), labels


def image(h: int, w: int, seed: int, image_index: int) -> np.ndarray:
    """A decoded picture's stand-in: uint8 [h, w, 3] RGB, uniform over 0..255
    (the preprocessing kernel's time does not depend on the pixel values)."""
    r = rng_for(seed, image_index, 5)
    return r.integers(0, 256, (h, w, 3), dtype=np.uint8)
