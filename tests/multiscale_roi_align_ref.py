"""The multi-scale RoIAlign contract (DESIGN.md §3 "Multi-scale RoIAlign") restated in numpy
fp32: torchvision's LevelMapper formula, the thresholds derived from it, and forward /
backward composed from tests/roi_align_ref.py level by level.  No GPU.

``out[idx_l] = roi_align_ref.forward(x_l, rois[idx_l], ..., scale_l)`` and ``grad_in_l =
roi_align_ref.backward(grad[idx_l], rois[idx_l], shape_l, ..., scale_l)`` with ``idx_l`` the
ascending indices of the RoIs of level ``l``.  Results are compared as bits."""
import numpy as np

import roi_align_ref as ref

F = np.float32
ELEM = ref.ELEM


def fwd_name(dtype):
    return f"roi_align_multi_fwd_kernel<{ELEM[dtype]}>"


def bwd_name(dtype):
    return f"roi_align_multi_bwd_tile_kernel<{ELEM[dtype]}, {ref.TILE}>"


def k_range(scales):
    """(k_min, k_max): -log2 of the first and the last scale, in fp32, truncated."""
    return int(-np.log2(F(scales[0]))), int(-np.log2(F(scales[-1])))


def formula(s, k_min, k_max, s0=224, lvl0=4):
    """LevelMapper on s = sqrt(area) (fp32, not NaN): floor(lvl0 + log2(s / s0) + 1e-6) clamped
    to [k_min, k_max], minus k_min; every operation in fp32.  int64."""
    s = np.asarray(s, F)
    assert not np.isnan(s).any()
    with np.errstate(all="ignore"):
        lvl = np.floor(F(lvl0) + np.log2(s / F(s0)) + F(1e-6))
    assert lvl.dtype == F
    return np.clip(lvl, F(k_min), F(k_max)).astype(np.int64) - k_min


def root_area(rois):
    """s = sqrt((x2 - x1) * (y2 - y1)) in fp32: two subtractions, one product, one root."""
    rois = np.asarray(rois, F).reshape(-1, 5)
    with np.errstate(all="ignore"):
        return np.sqrt((rois[:, 3] - rois[:, 1]) * (rois[:, 4] - rois[:, 2]))


def levels(rois, k_min, k_max, s0=224, lvl0=4):
    """The level of every RoI by the formula; a NaN s (a NaN coordinate, a negative area): 0."""
    s = root_area(rois)
    ok = ~np.isnan(s)
    out = np.zeros(len(s), np.int64)
    out[ok] = formula(s[ok], k_min, k_max, s0, lvl0)
    return out


def thresholds(k_min, k_max, s0=224, lvl0=4):
    """t_1 .. t_{k_max - k_min}: the smallest non-negative fp32 at which the formula yields at
    least k, by bisection over the bit patterns from +0 to +inf."""
    out = []
    for k in range(1, k_max - k_min + 1):
        lo, hi = 0, 0x7F800000              # formula(+0) = 0 < k <= formula(+inf)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if formula(np.array([mid], np.uint32).view(F), k_min, k_max, s0, lvl0)[0] >= k:
                hi = mid
            else:
                lo = mid
        out.append(np.array([hi], np.uint32).view(F)[0])
    return np.array(out, F)


def levels_by_count(rois, thr):
    """What the kernels evaluate: #{k : s >= t_k}; NaN compares false."""
    s = root_area(rois)
    with np.errstate(all="ignore"):
        return (s[:, None] >= np.asarray(thr, F)[None, :]).sum(1).astype(np.int64)


def forward(xs, rois, output_size, scales, sampling_ratio, aligned, lv):
    """out fp32 [R,C,PH,PW] for the maps xs and the levels lv (one per RoI)."""
    rois = np.asarray(rois, F).reshape(-1, 5)
    PH, PW = ref._size(output_size)
    out = np.zeros((len(rois), xs[0].shape[1], PH, PW), F)
    for l, x in enumerate(xs):
        idx = np.flatnonzero(lv == l)
        out[idx] = ref.forward(x, rois[idx], (PH, PW), scales[l], sampling_ratio, aligned)
    return out


def backward(grad, rois, shapes, scales, sampling_ratio, aligned, lv):
    """[grad_in_l fp32 [N,C,H_l,W_l]] for grad fp32 [R,C,PH,PW]."""
    rois = np.asarray(rois, F).reshape(-1, 5)
    grad = np.ascontiguousarray(grad, dtype=F)
    out = []
    for l, shape in enumerate(shapes):
        idx = np.flatnonzero(lv == l)
        out.append(ref.backward(grad[idx], rois[idx], tuple(shape), scales[l], sampling_ratio, aligned))
    return out


def box_with_root(s, x1=F(0), y1=F(0), w=F(16)):
    """A box [x1, y1, x1 + w, y1 + h] whose fp32 sqrt(area) is exactly ``s`` (finite, positive): w is
    a power of two, so w * h is exact, and with x1 = y1 = 0 both subtractions
    are exact; h is searched among the areas next to s * s."""
    s = F(s)
    a0 = F(s * s)
    for step in range(0, 8):
        for a in ((a0,) if step == 0 else (ulp_step(a0, step), ulp_step(a0, -step))):
            h = F(a / w)
            box = np.array([x1, y1, x1 + w, y1 + h], F)
            if F(h * w) == a and np.sqrt(a) == s and root_area(np.concatenate([[0], box]))[0] == s:
                return box
    raise AssertionError(f"no box with sqrt(area) == {s!r}")


def ulp_step(v, n):
    """v moved by n fp32 bit patterns (v > 0)."""
    return np.array([int(np.array([v], F).view(np.uint32)[0]) + n], np.uint32).view(F)[0]
