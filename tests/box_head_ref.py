"""numpy restatement of ``ops.box_head_targets`` and ``ops.box_head_losses`` (DESIGN.md §3 "Pyramid
box-head training").  The targets are restated in fp32 with every operation rounded separately, as the
kernels compute them, and are compared as bits.  The losses are restated in fp64 from the widened
inputs: the kernels evaluate them in fp32, and ``loss_bounds`` is the derived distance between the two.
Philox, the presence rule of a gt row and the IoU are ``rpn_targets_ref``'s, by import."""
import math

import numpy as np

from rpn_targets_ref import F32, iou_matrix, key_mask, philox_word0, present_rows

IDX_BITS = 13   # candidate indices are below 2^13: the order is that of key << 13 | index


def candidates(proposals, prop_count, gt, gt_count, add_gt=True):
    """(boxes fp32 [M, 4], present bool [M]) of one image: the proposals, then the gt rows."""
    R = proposals.shape[0]
    pc = min(max(int(prop_count), 0), R)
    present = np.concatenate([np.arange(R) < pc, present_rows(gt, gt_count) & bool(add_gt)])
    return np.concatenate([proposals, gt]).astype(F32), present


def match(boxes, present, gt, gt_count, fg, bg):
    """int32 [M]: -1 below bg, -2 in [bg, fg), else the gt index; -3 for an absent candidate."""
    M = boxes.shape[0]
    m = np.full(M, -3, np.int32)
    rows = np.nonzero(present_rows(gt, gt_count))[0]
    if rows.size == 0:
        m[present] = -1
        return m
    iou = iou_matrix(gt[rows], boxes)
    best, arg = iou.max(axis=0), iou.argmax(axis=0)        # the first of equals
    mm = np.where(best < F32(bg), -1, np.where(best < F32(fg), -2, rows[arg])).astype(np.int32)
    m[present] = mm[present]
    return m


def labels_of(m, gt_labels):
    """int32 [M]: the label the match gives (0 for -1, -1 for -2 and for an absent candidate)."""
    return np.where(m >= 0, gt_labels[np.maximum(m, 0)], np.where(m == -1, 0, -1)).astype(np.int32)


def encode(box, gt, weights):
    """BoxCoder.encode in torchvision's operation order, fp32; the log is correctly rounded."""
    wx, wy, ww, wh = (F32(w) for w in weights)
    with np.errstate(all="ignore"):
        w, h = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
        cx, cy = box[:, 0] + F32(0.5) * w, box[:, 1] + F32(0.5) * h
        gw, gh = gt[:, 2] - gt[:, 0], gt[:, 3] - gt[:, 1]
        gcx, gcy = gt[:, 0] + F32(0.5) * gw, gt[:, 1] + F32(0.5) * gh
        dw = ww * np.log((gw / w).astype(np.float64)).astype(F32)
        dh = wh * np.log((gh / h).astype(np.float64)).astype(F32)
        out = np.stack([(wx * (gcx - cx)) / w, (wy * (gcy - cy)) / h, dw, dh], axis=1)
    assert out.dtype == F32
    return out


def choose(cand, n, num, seed, calls, key_bits):
    """The ``num`` of the ascending candidate indices ``cand`` with the smallest (key, index), ascending."""
    if num == 0:
        return cand[:0]
    if num >= cand.size:
        return cand
    key = philox_word0(cand, n, calls, seed) & np.uint32(key_mask(key_bits))
    comp = (key.astype(np.uint64) << np.uint64(IDX_BITS)) | cand.astype(np.uint64)   # distinct: the order is total
    return np.sort(cand[np.argpartition(comp, num - 1)[:num]])


def targets(proposals, prop_count, gt_boxes, gt_labels, gt_count, seed, calls, *, batch_size_per_image=512,
            positive_fraction=0.25, fg_iou_thresh=0.5, bg_iou_thresh=0.5, reg_weights=(10.0, 10.0, 5.0, 5.0),
            add_gt=True, key_bits=32):
    """(rois, labels, matched, reg_targets, samples, n_pos, n_neg, matches) as the op returns them."""
    N, R = proposals.shape[:2]
    G, B = gt_boxes.shape[1], batch_size_per_image
    rois = np.zeros((N * B, 5), F32)
    rois[:, 0] = -1
    labels = np.full((N, B), -1, np.int32)
    matched = np.full((N, B), -1, np.int32)
    reg = np.zeros((N, B, 4), F32)
    samples = np.full((N, B), -1, np.int32)
    n_pos, n_neg = np.zeros(N, np.int32), np.zeros(N, np.int32)
    matches = np.empty((N, R + G), np.int32)
    max_pos = int(B * positive_fraction)
    for n in range(N):
        boxes, present = candidates(proposals[n], prop_count[n], gt_boxes[n], gt_count[n], add_gt)
        m = matches[n] = match(boxes, present, gt_boxes[n], gt_count[n], fg_iou_thresh, bg_iou_thresh)
        lab = labels_of(m, gt_labels[n])
        pos, neg = np.nonzero(present & (lab >= 1))[0], np.nonzero(present & (lab == 0))[0]
        num_pos = min(pos.size, max_pos)
        num_neg = min(neg.size, B - num_pos)
        sp = choose(pos, n, num_pos, seed, calls, key_bits)
        sn = choose(neg, n, num_neg, seed, calls, key_bits)
        s = np.sort(np.concatenate([sp, sn])).astype(np.int64)    # where(pos | neg): ascending, interleaved
        S = s.size
        is_pos = np.isin(s, sp)
        rois[n * B:n * B + S, 0] = n
        rois[n * B:n * B + S, 1:] = boxes[s]
        labels[n, :S] = lab[s]
        matched[n, :S] = np.where(is_pos, m[s], 0)
        reg[n, :S][is_pos] = encode(boxes[s][is_pos], gt_boxes[n][m[s][is_pos]], reg_weights)
        samples[n, :S] = s
        n_pos[n], n_neg[n] = num_pos, num_neg
    return rois, labels, matched, reg, samples, n_pos, n_neg, matches


NAMES = ("rois", "labels", "matched", "reg_targets", "samples", "n_pos", "n_neg", "matches")


def slot_labels(labels, n_pos, n_neg, C):
    """int [N, B]: 0..C-1 on a valid slot, -1 on padding (or a negative label), -2 on a valid slot whose
    label is >= C."""
    N, B = labels.shape
    valid = np.arange(B)[None, :] < (n_pos + n_neg)[:, None]
    return np.where(valid & (labels >= 0), np.where(labels >= C, -2, labels), -1)


def losses(class_logits, box_regression, labels, reg_targets, n_pos, n_neg, beta=1 / 9, g_cls=1.0, g_box=1.0):
    """The widened predictions (any float array) -> (classification_loss, box_loss, dclass_logits,
    dbox_regression, stats) in fp64.  ``g_cls`` / ``g_box``: the incoming gradients (None: unused)."""
    x = np.asarray(class_logits, np.float64)
    d = np.asarray(box_regression, np.float64)
    rows, C = x.shape
    lab = slot_labels(labels, n_pos, n_neg, C).reshape(rows)
    t = np.asarray(reg_targets, np.float64).reshape(rows, 4)
    beta = float(F32(beta))                                  # the kernels hold beta in fp32
    ok = lab >= 0
    S, n_skipped = int(ok.sum()), int((lab == -2).sum())
    gx, gd = np.zeros_like(x), np.zeros_like(d)
    if S == 0:
        return float("nan"), float("nan"), gx, gd, (0, 0, n_skipped, 0)
    xs, ls = x[ok], lab[ok]
    sh = xs - xs.max(axis=1, keepdims=True)
    e = np.exp(sh)
    ssum = e.sum(axis=1, keepdims=True)
    loss_c = float((np.log(ssum[:, 0]) - sh[np.arange(S), ls]).sum() / S)
    onehot = np.zeros_like(xs)
    onehot[np.arange(S), ls] = 1.0
    if g_cls is not None:
        gx[ok] = (e / ssum - onehot) * (float(g_cls) / S)
    pos = np.nonzero(lab >= 1)[0]
    cols = 4 * lab[pos][:, None] + np.arange(4)[None, :]
    diff = d[pos[:, None], cols] - t[pos]
    z = np.abs(diff)
    with np.errstate(all="ignore"):
        loss_b = float(np.where(z < beta, 0.5 * z * z / beta if beta > 0 else 0.0, z - 0.5 * beta).sum() / S)
        if g_box is not None:
            gd[pos[:, None], cols] = np.where(z < beta, diff / beta if beta > 0 else 0.0, np.sign(diff)) * (float(g_box) / S)
    return loss_c, loss_b, gx, gd, (S, int(pos.size), n_skipped, 0)


U = 2.0 ** -24   # the unit roundoff of fp32


def sum_depth(C):
    """Additions above one softmax term in the kernel's sum: a lane adds its classes (lane, lane + 64),
    then six butterfly levels."""
    return (C + 63) // 64 - 1 + 6


def loss_bounds(C, loss_c, loss_b, scale_c, scale_b):
    """DESIGN.md §3 "Pyramid box-head training", "Loss and gradient bound": how far the kernels' fp32
    evaluation may lie from the fp64 restatement -> (classification loss, box loss, an element of
    dclass_logits, an element of dbox_regression), for fp32 gradients; a 16-bit gradient adds the
    spacing of its format at the value."""
    k = sum_depth(C)
    ln_c = math.log(C)
    return (U * (2 + 2 * ln_c + k + 3 * abs(loss_c)), U * 7 * abs(loss_b),
            U * abs(scale_c) * (7 + ln_c + k), U * abs(scale_b) * 5)
