"""The losses contract (DESIGN.md "Losses", include/frcnn_capi.h
frcnn_losses_fwd / frcnn_losses_bwd) restated in numpy for one stage, with the
inputs as the kernels see them.  Per-element arithmetic is fp32 with every
operation separately rounded, exp and log correctly rounded (fp64, rounded
once); the sums over rows are fp64.  Rows without a valid label are never
read.  Plain numpy, no GPU.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32


def classify_labels(labels, C):
    """labels int32 or fp64 [rows] -> int64 [rows]: -1 unlabelled, 0..C-1 valid,
    -2 skipped (outside -1..C-1 after truncation toward zero; NaN included)."""
    labels = np.asarray(labels)
    if labels.dtype == np.float64:
        ok = (labels > -2.0) & (labels < float(C))      # False for NaN
        lab = np.where(ok, np.trunc(np.where(ok, labels, 0.0)), -2.0).astype(np.int64)
    else:
        lab = labels.astype(np.int64)
    return np.where((lab >= -1) & (lab < C), lab, -2)


def sigma_consts(sigma):
    """sigma^2, 1/sigma^2, 0.5*sigma^2, 0.5/sigma^2: formed in double, rounded to fp32."""
    s2 = float(sigma) ** 2
    return F32(s2), F32(1.0 / s2), F32(0.5 * s2), F32(0.5 / s2)


def stage(cls, reg, reg_t, labels, sigma=1.0, head=False, g_cls=1.0, g_reg=1.0):
    """cls fp32 [rows, C], reg fp32 [rows, 4] (or [rows, 4C] with ``head``), reg_t
    fp64 [rows, 4], labels int32 / fp64 [rows]; g_cls / g_reg: the upstream
    gradients (None = that loss is unused: its gradient is all zero).
    Returns dict(loss fp32 [2], stats int32 [4], dcls fp32 [rows, C], dreg fp32
    like reg)."""
    cls = np.asarray(cls, F32)
    reg = np.asarray(reg, F32)
    reg_t = np.asarray(reg_t, np.float64)
    rows, C = cls.shape
    P = C if head else 1
    assert reg.shape == (rows, 4 * P) and reg_t.shape == (rows, 4)
    lab = classify_labels(np.asarray(labels).reshape(rows), C)
    s2, inv_s2, half_s2, half_inv = sigma_consts(sigma)
    valid = np.nonzero(lab >= 0)[0]
    pos = np.nonzero(lab > 0)[0]
    n_valid, n_pos, n_skip = len(valid), len(pos), int((lab == -2).sum())
    dcls = np.zeros((rows, C), F32)
    dreg = np.zeros((rows, 4 * P), F32)
    with np.errstate(all="ignore"):
        # cross-entropy over the labelled rows
        x = cls[valid]
        lv = lab[valid]
        m = x.max(axis=1) if n_valid else np.zeros(0, F32)
        e = np.exp((x - m[:, None]).astype(np.float64)).astype(F32)
        s = e[:, 0].copy()
        for c in range(1, C):                               # ascending class order, fp32
            s = s + e[:, c]
        lse = np.log(s.astype(np.float64)).astype(F32)
        xl = x[np.arange(n_valid), lv]
        term = lse - (xl - m)
        cls_sum = term.astype(np.float64).sum()
        cls_loss = F32(cls_sum / np.float64(n_valid)) if n_valid else F32(np.nan)
        if g_cls is not None and n_valid:
            scale = F32(g_cls) / F32(n_valid)
            p = e / s[:, None]
            onehot = (np.arange(C)[None, :] == lv[:, None]).astype(F32)
            dcls[valid] = (p - onehot) * scale
        # smooth-L1 over the positive rows, on the label's four columns
        col0 = (lab[pos] * 4 if head else np.zeros(len(pos), np.int64))[:, None] + np.arange(4)[None, :]
        xr = reg[pos[:, None], col0]
        t = reg_t[pos].astype(F32)                           # round-to-nearest, as .float()
        diff = xr - t
        d = np.abs(diff)
        terms = np.where(d < inv_s2, half_s2 * (d * d), d - half_inv)
        reg_loss = F32(terms.astype(np.float64).sum() / np.float64(max(n_pos, 1)))
        if g_reg is not None and n_pos:
            scale = F32(g_reg) / F32(max(n_pos, 1))
            g = np.where(d < inv_s2, s2 * diff, np.sign(diff).astype(F32))
            dreg[pos[:, None], col0] = g * scale
    return dict(loss=np.array([cls_loss, reg_loss], F32),
                stats=np.array([n_valid, n_pos, n_skip, 0], np.int32), dcls=dcls, dreg=dreg)


def grad_bounds(C, n_valid, n_pos, g_cls, g_reg):
    """Absolute bounds on a kernel's gradient elements against the exact value,
    from the arithmetic: dcls is one correctly rounded exp, a C-term fp32 sum, a
    divide, a subtract near 1 and a multiply on a magnitude <= |g|/n_valid; each
    dreg element is at most |g|/n_pos (sigma^2 * d < 1 in the quadratic branch)
    after three roundings."""
    u = 2.0 ** -24
    bc = (C + 8) * u * abs(g_cls or 0.0) / max(n_valid, 1)
    br = 4 * u * abs(g_reg or 0.0) / max(n_pos, 1)
    return bc, br
