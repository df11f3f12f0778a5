"""The pyramid mask head's contract (DESIGN.md §3 "Pyramid mask head") restated in numpy: the
mask targets (compaction + RoIAlign of the matched mask, through roi_align_ref.forward), the mask
loss and its gradient in fp64, and the mask paste in fp32 with every operation rounded.  No GPU.

``mistake=`` plants one deviation from the contract; tests/test_mask_head_cpu.py checks that the
named cases tell each of them from the contract."""
import numpy as np

import roi_align_ref as ra

F = np.float32
U = 2.0 ** -24                 # half an ulp of 1 in fp32: the relative error of one rounding
MAX_COORD = F(2 ** 20)
TARGET_OUT = ("rois", "labels", "matched", "slot", "count", "targets")
TARGET_MISTAKES = ("thresholded_targets", "gt_order")
LOSS_MISTAKES = ("mean_over_all_rows", "wrong_channel")
PASTE_MISTAKES = ("align_corners", "no_padding", "scale_from_m", "floor", "no_plus_one", "no_clip", "non_strict")


def bits_equal(a, b):
    """Bitwise equality of two arrays of one dtype and shape (fp32: zero's sign included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == F:
        return ra.same_bits(a, b)
    return bool(np.array_equal(a, b))


# ---------------------------------------------------------------- targets
def mask_targets(bt_rois, bt_labels, bt_matched, gt_masks, M, P=None, mistake=None):
    """-> (rois [N*P,5], labels, matched, slot [N,P], count [N], targets [N*P,M,M])."""
    bt_labels = np.asarray(bt_labels, np.int32)
    bt_matched = np.asarray(bt_matched, np.int32)
    N, B = bt_labels.shape
    bt_rois = np.asarray(bt_rois, F).reshape(N, B, 5)
    G = gt_masks.shape[1]
    P = B if P is None else P
    rois = np.zeros((N, P, 5), F)
    rois[:, :, 0] = -1
    labels = np.full((N, P), -1, np.int32)
    matched = np.full((N, P), -1, np.int32)
    slot = np.full((N, P), -1, np.int32)
    count = np.zeros(N, np.int32)
    targets = np.zeros((N, P, M, M), F)
    for n in range(N):
        pos = [s for s in range(B) if bt_labels[n, s] >= 1]
        if mistake == "gt_order":
            pos.sort(key=lambda s: (bt_matched[n, s], s))
        pos = pos[:P]
        count[n] = len(pos)
        for r, s in enumerate(pos):
            rois[n, r, 0] = n
            rois[n, r, 1:] = bt_rois[n, s, 1:]
            labels[n, r], matched[n, r], slot[n, r] = bt_labels[n, s], bt_matched[n, s], s
            g = int(bt_matched[n, s])
            if 0 <= g < G:
                x = gt_masks[n, g][None, None].astype(F)
                roi = np.concatenate([[F(0)], rois[n, r, 1:]]).astype(F)
                targets[n, r] = ra.forward(x, roi[None], (M, M), 1.0, -1, False)[0, 0]
    if mistake == "thresholded_targets":
        targets = (targets >= F(0.5)).astype(F)
    return rois.reshape(N * P, 5), labels, matched, slot, count, targets.reshape(N * P, M, M)


# ----------------------------------------------------------------- losses
def _rows(labels, count, C):
    """(row, n, label) of the rows the loss reads, and the number skipped for their label."""
    N, P = labels.shape
    used, skipped = [], 0
    for n in range(N):
        for r in range(min(max(int(count[n]), 0), P)):
            lab = int(labels[n, r])
            if 0 <= lab < C:
                used.append((n * P + r, n, lab))
            else:
                skipped += 1
    return used, skipped


def mask_losses(logits, targets, labels, count, g=1.0, mistake=None):
    """fp64: -> (loss, grad [N*P,C,M,M], (S, skipped)).  ``logits``: fp32 values (16-bit inputs
    widened)."""
    x = np.asarray(logits, np.float64)
    t = np.asarray(targets, np.float64)
    labels = np.asarray(labels)
    N, P = labels.shape
    C, M = x.shape[1], x.shape[2]
    used, skipped = _rows(labels, count, C)
    S = int(sum(min(max(int(c), 0), P) for c in count))
    grad = np.zeros_like(x)
    if S == 0:
        return 0.0, grad, (0, skipped)
    denom = float(S * M * M) if mistake != "mean_over_all_rows" else float(N * P * M * M)
    total = 0.0
    with np.errstate(all="ignore"):
        for row, _, lab in used:
            ch = lab if mistake != "wrong_channel" else (lab + 1) % C
            xv, tv = x[row, ch], t[row]
            total += float(np.sum(np.maximum(xv, 0) - xv * tv + np.log1p(np.exp(-np.abs(xv)))))
            sig = np.where(xv >= 0, 1 / (1 + np.exp(-xv)), np.exp(xv) / (1 + np.exp(xv)))
            grad[row, ch] = (sig - tv) * (g / denom)
    return total / denom, grad, (S, skipped)


def loss_bounds(logits, targets, labels, count, g=1.0, dtype="f32"):
    """(loss bound, gradient bound per element) of the fp32 kernels against ``mask_losses``.

    Forward, per element l = (max(x,0) - x*t) + log1p(exp(-|x|)): x*t rounds once (U*|x*t|), the
    subtraction once (U*(|x| + |x*t|)), exp and log1p are correctly rounded and log1p is
    1-Lipschitz (2*U), the last addition once (U*(2|x| + 1)): at most U*(4|x| + 4), t in [0,1].
    The fp64 sum adds 2^-53 relative per addition, far below; the quotient is rounded to fp32 once.
    Backward, (1/(1+e) - t) * scale with e = exp(-x): e, 1+e and the quotient round once each
    (3*U absolute on a value <= 1), the difference once, scale = g / (float)(S*M*M) twice, the
    product once: at most 8*U*|scale|; a 16-bit gradient is rounded once more at the store
    (unit roundoff 2^-8 in bfloat16 with its 8 significant bits, 2^-11 in float16 with its 11, and
    2^-25 absolute below float16's normal range)."""
    x = np.asarray(logits, np.float64)
    labels = np.asarray(labels)
    C, M = x.shape[1], x.shape[2]
    used, _ = _rows(labels, count, C)
    S = int(sum(min(max(int(c), 0), labels.shape[1]) for c in count))
    gb = np.zeros_like(x)
    if S == 0:
        return 0.0, gb
    denom = float(S * M * M)
    err = sum(float(np.sum(U * (4 * np.abs(x[row, lab]) + 4))) for row, _, lab in used)
    loss, grad, _ = mask_losses(logits, targets, labels, count, g)
    lb = err / denom + 2 * U * abs(loss) + 1e-300
    scale = abs(g) / denom
    store = {"f32": 0.0, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}[dtype]
    for row, _, lab in used:
        gb[row, lab] = 8 * U * scale + store * (np.abs(grad[row, lab]) + 8 * U * scale) + (2.0 ** -25 if dtype == "f16" else 0)
    return lb, gb


# ------------------------------------------------------------------ paste
def sigmoid(x):
    """1 / (1 + exp(-x)) in fp32: exp correctly rounded, then one addition and one division."""
    with np.errstate(all="ignore"):
        e = np.exp(-np.asarray(x, F).astype(np.float64)).astype(F)
        return (F(1) / (F(1) + e)).astype(F)


def _taps(scale, d, S, align_corners=False, out=None):
    d = np.arange(d[0], d[1], dtype=np.int64)
    if align_corners:
        sc = F(S - 1) / F(out - 1) if out > 1 else F(0)
        src = (sc * d.astype(F)).astype(F)
    else:
        src = (scale * (d.astype(F) + F(0.5))).astype(F) - F(0.5)
        src = np.where(src < 0, F(0), src).astype(F)
    i0 = np.minimum(src.astype(np.int64), S - 1)
    i1 = i0 + (i0 < S - 1)
    l1 = (src - i0.astype(F)).astype(F)
    return i0, i1, (F(1) - l1).astype(F), l1


def paste_geometry(box, M, padding, mistake=None):
    """(b0, b1, b2, b3, w, h) of one finite fp32 box, or None when a coordinate leaves 2^20."""
    S = M + 2 * padding
    scale = F(S) / F(M)
    x1, y1, x2, y2 = (F(v) for v in box)
    w_half, h_half = (x2 - x1) * F(0.5), (y2 - y1) * F(0.5)
    x_c, y_c = (x2 + x1) * F(0.5), (y2 + y1) * F(0.5)
    w_half, h_half = w_half * scale, h_half * scale
    e = [x_c - w_half, y_c - h_half, x_c + w_half, y_c + h_half]
    if not all(abs(v) <= MAX_COORD for v in e):
        return None
    conv = (lambda v: int(np.floor(v))) if mistake == "floor" else (lambda v: int(v))
    b0, b1, b2, b3 = (conv(v) for v in e)
    one = 0 if mistake == "no_plus_one" else 1
    return b0, b1, b2, b3, max(b2 - b0 + one, 1), max(b3 - b1 + one, 1)


def mask_paste(logits, boxes, labels, count, canvas_size, image_sizes=None, original_sizes=None, padding=1,
               threshold=0.5, mistake=None):
    """-> masks [N,D,Hc,Wc]: uint8 (prob > threshold) or fp32 probabilities (threshold None)."""
    logits = np.asarray(logits, F)
    boxes = np.asarray(boxes, F)
    N, D = boxes.shape[:2]
    C, M = logits.shape[1], logits.shape[2]
    Hc, Wc = canvas_size
    p = 0 if mistake == "no_padding" else padding
    S = M + 2 * p
    out = np.zeros((N, D, Hc, Wc), F)
    with np.errstate(all="ignore"):
        for n in range(N):
            im_h, im_w = Hc, Wc
            if original_sizes is not None:
                oh, ow = F(original_sizes[n][0]), F(original_sizes[n][1])
                im_h = min(int(min(oh, F(4096))) if oh >= 1 else 0, Hc)
                im_w = min(int(min(ow, F(4096))) if ow >= 1 else 0, Wc)
            for d in range(min(max(int(count[n]), 0), D)):
                lab = int(labels[n, d])
                b = boxes[n, d].copy()
                if not (1 <= lab < C) or not all(abs(v) <= MAX_COORD for v in b) or b[2] < b[0] or b[3] < b[1]:
                    continue
                if original_sizes is not None and image_sizes is not None:
                    rh, rw = oh / F(image_sizes[n][0]), ow / F(image_sizes[n][1])
                    b = np.array([b[0] * rw, b[1] * rh, b[2] * rw, b[3] * rh], F)
                if mistake == "scale_from_m":
                    geo = paste_geometry(b, M, 0)
                else:
                    geo = paste_geometry(b, M, p, mistake)
                if geo is None:
                    continue
                b0, b1, b2, b3, w, h = geo
                cw, ch = (Wc, Hc) if mistake == "no_clip" else (im_w, im_h)
                x0, x1, y0, y1 = max(b0, 0), min(b2 + 1, cw, b0 + w), max(b1, 0), min(b3 + 1, ch, b1 + h)
                if x0 >= x1 or y0 >= y1:
                    continue
                prob = np.zeros((S, S), F)
                prob[p:p + M, p:p + M] = sigmoid(logits[n * D + d, lab])
                ac = mistake == "align_corners"
                ix0, ix1, l0x, l1x = _taps(F(S) / F(w), (x0 - b0, x1 - b0), S, ac, w)
                iy0, iy1, l0y, l1y = _taps(F(S) / F(h), (y0 - b1, y1 - b1), S, ac, h)
                top = l0x[None, :] * prob[iy0][:, ix0] + l1x[None, :] * prob[iy0][:, ix1]
                bot = l0x[None, :] * prob[iy1][:, ix0] + l1x[None, :] * prob[iy1][:, ix1]
                val = l0y[:, None] * top + l1y[:, None] * bot
                assert val.dtype == F
                out[n, d, y0:y1, x0:x1] = val
    if threshold is None:
        return out
    t = F(threshold)
    return (out >= t if mistake == "non_strict" else out > t).astype(np.uint8)


def interpolate_bound(S):
    """The largest difference between two fp32 evaluations of the paste's bilinear formula that
    differ in operation order or contraction (DESIGN.md §3 "Pyramid mask head"): the source
    coordinate is two roundings (a product and a difference) of values below S2 = the power of
    two at or above S, U*S2 each, on either side; the value is 1-Lipschitz in each axis' weight
    (neighbouring probabilities differ by at most 1); the weights and the three-level sum are at
    most 7 roundings of values in [0, 1] on either side."""
    S2 = 1 << int(np.ceil(np.log2(max(S, 1))))
    return 2 * (2 * 2 * U * S2) + 14 * U


def detection_rois(boxes, count):
    N, D = boxes.shape[:2]
    rois = np.zeros((N, D, 5), F)
    rois[:, :, 0] = -1
    for n in range(N):
        k = min(max(int(count[n]), 0), D)
        rois[n, :k, 0] = n
        rois[n, :k, 1:] = boxes[n, :k]
    return rois.reshape(N * D, 5)
