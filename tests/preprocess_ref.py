"""numpy fp64 reference of the image preprocessing contract and
the case table of the preprocessing tests.  No scipy, no torch: it runs
wherever the tests run.

``skimage.transform.resize(image, (oh, ow))`` with its defaults is two
``scipy.ndimage`` calls (a Gaussian filter when downscaling, then an order-1
zoom), both separable and linear, so per channel the resize is
``Wh @ p @ Ww.T`` with one matrix per axis.  ``axis_matrix`` builds it.
"""
from __future__ import annotations

import numpy as np

MEAN = (0.485, 0.456, 0.406)   # utils/data_loader.py:72
STD = (0.229, 0.224, 0.225)


def fold(i: int, n: int) -> int:
    """Mirror without edge repeat: period 2(n-1), -1 -> 1, n -> n-2; n == 1 -> 0."""
    if n == 1:
        return 0
    p = 2 * (n - 1)
    m = i % p
    return m if m < n else p - m


def sigma_radius(n_in: int, n_out: int):
    """Anti-aliasing sigma of an axis (0 when not downscaling) and the filter
    radius at ndimage's truncate=4.0."""
    s = max(0.0, (n_in / n_out - 1) / 2)
    return s, int(4.0 * s + 0.5)


def taps(n_in: int, n_out: int) -> int:
    """Source taps per output element of an axis: 2, plus the Gaussian's reach."""
    return 2 + 2 * sigma_radius(n_in, n_out)[1]


def gaussian_matrix(n: int, s: float, r: int) -> np.ndarray:
    g = np.zeros((n, n))
    if s == 0:
        return np.eye(n)
    k = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (s * s) * k ** 2)
    w = w / w.sum()
    for i in range(n):
        for kk, wk in zip(k, w):
            g[i, fold(i + int(kk), n)] += wk
    return g


def bilinear_matrix(n_in: int, n_out: int) -> np.ndarray:
    b = np.zeros((n_out, n_in))
    den = 2 * n_out
    for d in range(n_out):
        num = (2 * d + 1) * n_in - n_out      # position = num / den, exact
        i0 = num // den                       # floor, also for num < 0
        f = (num - i0 * den) / den
        b[d, fold(i0, n_in)] += 1.0 - f
        b[d, fold(i0 + 1, n_in)] += f
    return b


def axis_matrix(n_in: int, n_out: int) -> np.ndarray:
    s, r = sigma_radius(n_in, n_out)
    return bilinear_matrix(n_in, n_out) @ gaussian_matrix(n_in, s, r)


def resize(p: np.ndarray, out_hw) -> np.ndarray:
    """p fp64 [h, w, C] -> [oh, ow, C]."""
    wh = axis_matrix(p.shape[0], out_hw[0])
    ww = axis_matrix(p.shape[1], out_hw[1])
    return np.einsum("ih,hwc,jw->ijc", wh, p, ww, optimize=True)


def preprocess(img: np.ndarray, out_hw, mean=MEAN, std=STD) -> np.ndarray:
    """uint8 [h, w, 3] -> fp64 [3, oh, ow]: /255, resize, normalise, CHW."""
    p = resize(img.astype(np.float64) / 255, out_hw)
    out = (p -np.asarray(mean, np.float64)) / np.asarray(std, np.float64)
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def rescale_boxes(boxes: np.ndarray, hw: np.ndarray, out_hw) -> np.ndarray:
    """Batched utils/data_loader.py:66-69: boxes fp64 [N, G, 4], hw [N, 2].
    An image with h < 1 or w < 1 gets all -1."""
    out = np.empty_like(np.asarray(boxes, np.float64))
    for n in range(len(boxes)):
        h, w = int(hw[n][0]), int(hw[n][1])
        if h < 1 or w < 1:
            out[n] = -1
            continue
        b = np.array(boxes[n], np.float64, copy=True)
        b[:, [0, 2]] = b[:, [0, 2]] / h * out_hw[0]
        b[:, [1, 3]] = b[:, [1, 3]] / w * out_hw[1]
        b[b < 0] = -1
        out[n] = b
    return out


def tolerance(in_hw, out_hw, std=STD) -> float:
    """The derived fp32 bound of the device result against this reference:
    (4*(T_h + T_w) + 16) * 2^-24 / min(std)."""
    t = taps(in_hw[0], out_hw[0]) + taps(in_hw[1], out_hw[1])
    return (4 * t + 16) * 2.0 ** -24 / min(std)


def image(in_hw, kind="random", seed=0) -> np.ndarray:
    h, w = in_hw
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "checker":
        yy, xx = np.mgrid[:h, :w]
        return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    if kind == "zeros":
        return np.zeros((h, w, 3), np.uint8)
    if kind == "full":
        return np.full((h, w, 3), 255, np.uint8)
    raise ValueError(kind)


OTHER_MEAN = (0.1, 0.5, 0.9)
OTHER_STD = (0.5, 0.05, 1.5)

# (id, in (h, w), out (h, w), image kind, mean, std)
CASES = [
    ("identity", (4, 5), (4, 5), "random", MEAN, STD),
    ("up_5x7", (5, 7), (12, 12), "random", MEAN, STD),
    ("up_2x3", (2, 3), (8, 8), "random", MEAN, STD),
    ("one_pixel", (1, 1), (4, 4), "random", MEAN, STD),
    ("mixed", (13, 9), (6, 12), "random", MEAN, STD),
    ("down_20x31", (20, 31), (6, 7), "random", MEAN, STD),
    ("down_64x48", (64, 48), (37, 41), "random", MEAN, STD),
    ("ratio4_checker", (24, 24), (6, 6), "checker", MEAN, STD),
    ("radius_gt_image", (4, 4), (1, 1), "random", MEAN, STD),
    ("long_axis", (3, 499), (4, 600), "random", MEAN, STD),
    ("voc", (375, 500), (600, 600), "random", MEAN, STD),
    ("all_0", (5, 7), (12, 12), "zeros", MEAN, STD),
    ("all_255", (5, 7), (12, 12), "full", MEAN, STD),
    ("other_mean_std", (5, 7), (12, 12), "random", OTHER_MEAN, OTHER_STD),
]
CASE_IDS = [c[0] for c in CASES]

_ref_cache = {}


def case_data(case):
    """(uint8 image, fp64 reference [3, oh, ow]) of a case; computed once."""
    cid, in_hw, out_hw, kind, mean, std = case
    if cid not in _ref_cache:
        img = image(in_hw, kind, seed=CASE_IDS.index(cid))
        ref = preprocess(img, out_hw, mean, std)
        ref.setflags(write=False)
        img.setflags(write=False)
        _ref_cache[cid] = (img, ref)
    return _ref_cache[cid]
