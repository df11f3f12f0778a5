"""numpy restatement of the pyramid box-head inference contract (DESIGN.md §3 "Pyramid box-head
inference"): fp32 with every operation rounded separately, the fp64 ``exp`` rounded once.  A
helper for the box-detections tests, not a test: ``box_detections`` returns the six arrays of
``ops.box_head_detections``.

``mistake`` plants one deviation from the contract (tests/test_box_detections_cpu.py holds each
against the case named for it): "ge_thresh", "ties_desc_row", "cross_class", "transitive",
"no_clamp", "recip_weights", "filter_before_clip", "merge_class_first", "trunc_per_class".
"""
import numpy as np

F32 = np.float32
DCLIP = F32(np.log(1000.0 / 16.0))      # torchvision's bbox_xform_clip, rounded once
MISTAKES = ("ge_thresh", "ties_desc_row", "cross_class", "transitive", "no_clamp", "recip_weights",
            "filter_before_clip", "merge_class_first", "trunc_per_class")


def exp_cr(v):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp(np.asarray(v, np.float64)).astype(F32)


def softmax(x):
    """[k, C] logits -> p: m = max, e = exp_cr(x - m), s = ((e0 + e1) + e2) + ..., p = e * (1 / s).
    A row with a NaN, a +inf or only -inf logits is NaN throughout."""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e = exp_cr(x - x.max(axis=1, keepdims=True))
        s = e[:, 0].copy()
        for c in range(1, x.shape[1]):
            s = s + e[:, c]
        return e * (F32(1) / s)[:, None]


def desc_key(p):
    """csrc/common.h desc_score_key: ascending u32 keys for descending fp32 scores."""
    p = np.ascontiguousarray(p, F32)
    u = p.view(np.uint32).copy()
    u[u == 0x80000000] = 0
    asc = np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key = (~asc).astype(np.uint32)
    key[np.isnan(p)] = 0
    return key


def decode(props, d, weights, img_h, img_w, min_size, mistake=None):
    """BoxCoder.decode_single + clip_boxes_to_image for rows ``props`` [k, 4] with their class's
    deltas ``d`` [k, 4] -> (boxes [k, 4], kept by remove_small_boxes [k])."""
    props, d = np.asarray(props, F32).reshape(-1, 4), np.asarray(d, F32).reshape(-1, 4)
    wx, wy, ww, wh = (F32(v) for v in weights)
    half = F32(0.5)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        w = props[:, 2] - props[:, 0]
        h = props[:, 3] - props[:, 1]
        cx = props[:, 0] + half * w
        cy = props[:, 1] + half * h
        if mistake == "recip_weights":
            dx, dy, dw, dh = d[:, 0] * (F32(1) / wx), d[:, 1] * (F32(1) / wy), d[:, 2] * (F32(1) / ww), d[:, 3] * (F32(1) / wh)
        else:
            dx, dy, dw, dh = d[:, 0] / wx, d[:, 1] / wy, d[:, 2] / ww, d[:, 3] / wh
        if mistake != "no_clamp":
            dw = np.where(dw > DCLIP, DCLIP, dw)     # torch.clamp(max=): a NaN stays
            dh = np.where(dh > DCLIP, DCLIP, dh)
        pcx = dx * w
        pcx = pcx + cx
        pcy = dy * h
        pcy = pcy + cy
        pw = exp_cr(dw) * w
        ph = exp_cr(dh) * h
        hw, hh = half * pw, half * ph
        raw = np.stack([pcx - hw, pcy - hh, pcx + hw, pcy + hh], 1).astype(F32)
        b = raw.copy()
        b[:, [0, 2]] = np.clip(raw[:, [0, 2]], F32(0), F32(img_w))
        b[:, [1, 3]] = np.clip(raw[:, [1, 3]], F32(0), F32(img_h))
        s = raw if mistake == "filter_before_clip" else b
        ok = (s[:, 2] - s[:, 0] >= F32(min_size)) & (s[:, 3] - s[:, 1] >= F32(min_size))
    return b, ok


def iou_matrix(b):
    """[k, 4] fp32 boxes -> [k, k] fp32 IoU in torchvision's operation order (csrc/nms_iou.h)."""
    b = np.asarray(b, F32)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0])
    h = np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1])
    inter = np.maximum(w, F32(0)) * np.maximum(h, F32(0))
    uni = (area[:, None] + area[None, :]) - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / uni


def over_matrix(b, thr):
    """``(double)iou > thr``: a NaN quotient or threshold is never over."""
    with np.errstate(invalid="ignore"):
        return iou_matrix(b).astype(np.float64) > float(thr)


def greedy_nms(boxes, thr, transitive=False):
    """Positions kept of ``boxes`` given in sweep order.  ``transitive``: the planted mistake in
    which a suppressed box goes on suppressing."""
    k = len(boxes)
    if k == 0:
        return np.zeros(0, np.int64)
    over = over_matrix(boxes, thr)
    dead = np.zeros(k, bool)
    keep = []
    for i in range(k):
        if not dead[i]:
            keep.append(i)
        if not dead[i] or transitive:
            dead[i + 1:] |= over[i, i + 1:]
    return np.asarray(keep, np.int64)


def probabilities(class_logits, prop_count, n, R):
    """p [k, C] of image n's rows below its clamped count."""
    k = int(np.clip(prop_count[n], 0, R))
    C = class_logits.shape[1]
    return softmax(class_logits[n * R:n * R + k]) if k else np.zeros((0, C), F32)


def candidates(p, score_thresh, mistake=None):
    """Per class c >= 1: the rows with p > fp32(score_thresh), ascending."""
    t = F32(score_thresh)
    with np.errstate(invalid="ignore"):
        return [np.nonzero(p[:, c] >= t if mistake == "ge_thresh" else p[:, c] > t)[0] for c in range(1, p.shape[1])]


def box_detections(class_logits, box_regression, proposals, prop_count, image_sizes, *, score_thresh=0.05,
                   nms_thresh=0.5, detections_per_img=100, min_size=1e-2, reg_weights=(10.0, 10.0, 5.0, 5.0),
                   original_sizes=None, mistake=None):
    assert mistake is None or mistake in MISTAKES, mistake
    logits = np.asarray(class_logits, F32)
    reg = np.asarray(box_regression, F32)
    proposals = np.asarray(proposals, F32)
    N, R = proposals.shape[:2]
    C = logits.shape[1]
    D = int(detections_per_img)
    assert logits.shape == (N * R, C) and reg.shape == (N * R, 4 * C)
    sizes = np.broadcast_to(np.asarray(image_sizes, F32), (N, 2))
    boxes = np.zeros((N, D, 4), F32)
    labels = np.full((N, D), -1, np.int32)
    scores = np.zeros((N, D), F32)
    roi = np.full((N, D), -1, np.int32)
    count = np.zeros(N, np.int32)
    total = np.zeros(N, np.int32)
    for n in range(N):
        img_h, img_w = sizes[n]
        p = probabilities(logits, prop_count, n, R)
        kr, kc, kb = [], [], []             # kept rows, classes, boxes
        pool = []                           # the "cross_class" mistake sweeps all classes as one
        for c, rows in enumerate(candidates(p, score_thresh, mistake), 1):
            if len(rows) == 0:
                continue
            b, ok = decode(proposals[n, rows], reg[n * R + rows, 4 * c:4 * c + 4], reg_weights, img_h, img_w, min_size,
                           mistake)
            rows, b = rows[ok], b[ok]
            tie = (R - 1 - rows) if mistake == "ties_desc_row" else rows
            order = np.argsort((desc_key(p[rows, c]).astype(np.uint64) << np.uint64(32)) | tie.astype(np.uint64),
                               kind="stable")
            rows, b = rows[order], b[order]
            if mistake == "cross_class":
                pool.append((rows, np.full(len(rows), c), b))
                continue
            keep = greedy_nms(b, nms_thresh, mistake == "transitive")
            if mistake == "trunc_per_class":
                keep = keep[:D]
            kr.append(rows[keep])
            kc.append(np.full(len(keep), c))
            kb.append(b[keep])
        if pool:
            rows, cs, b = (np.concatenate(a) for a in zip(*pool))
            order = np.argsort((desc_key(p[rows, cs]).astype(np.uint64) << np.uint64(32)) |
                               (rows * (C - 1) + cs - 1).astype(np.uint64), kind="stable")
            keep = order[greedy_nms(b[order], nms_thresh)]
            kr, kc, kb = [rows[keep]], [cs[keep]], [b[keep]]
        if not kr:
            continue
        kr, kc, kb = np.concatenate(kr), np.concatenate(kc), np.concatenate(kb)
        flat = (kc - 1) * R + kr if mistake == "merge_class_first" else kr * (C - 1) + (kc - 1)
        order = np.argsort((desc_key(p[kr, kc]).astype(np.uint64) << np.uint64(32)) | flat.astype(np.uint64),
                           kind="stable")
        total[n] = len(order)
        k = count[n] = min(len(order), D)
        o = order[:k]
        b = kb[o].copy()
        if original_sizes is not None:
            orig = np.asarray(original_sizes, F32)
            ratio_h, ratio_w = orig[n, 0] / img_h, orig[n, 1] / img_w
            b[:, [0, 2]] = b[:, [0, 2]] * ratio_w
            b[:, [1, 3]] = b[:, [1, 3]] * ratio_h
        boxes[n, :k], labels[n, :k], scores[n, :k], roi[n, :k] = b, kc[o], p[kr[o], kc[o]], kr[o]
    return boxes, labels, scores, roi, count, total
