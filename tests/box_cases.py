"""Named edge cases of the small box utilities (utils/utils.py:47-119,
utils/anchors.py, nets/heads.py:42-47): empty and one-row inputs, sizes around
the kernels' 256-thread blocks, every dtype combination numpy promotes
differently, and rows with zero-area, touching, inverted, NaN, infinite and
overflowing boxes.  Plain numpy, no GPU.

Users: tests/golden/make_golden.py ``box_edges`` (the genuine reference over
this table -> tests/golden/box_utils_edges.npz), tests/test_oracle_golden.py
(oracle == that file, and each case's precondition on the oracle alone) and
tests/test_gpu_box_utils.py (HIP path == oracle).

Random rows repeat with period 48 (no divisor of a wave or a block, so the
rows on either side of every block edge differ) and every coordinate is exact
in fp32, so one stored table serves the fp32 and the fp64 variants and the
golden file stays small.
"""
from __future__ import annotations

import numpy as np

PERIOD = 48
F32, F64 = np.float32, np.float64
DTYPES = ((F32, F32), (F32, F64), (F64, F32), (F64, F64))
BIG = float(np.float32(1e20))          # squares to inf in fp32, to 1e40 in fp64
FMAX = float(np.finfo(np.float32).max)
nan, inf = float("nan"), float("inf")


def tag(ta, tb):
    return ("f32" if ta == F32 else "f64") + "_" + ("f32" if tb == F32 else "f64")


def _rand_boxes(seed, n=PERIOD, lo=2.0, hi=60.0):
    """fp64 boxes [n,4] (tl < br) on a 1/8 grid: exact in fp32."""
    r = np.random.default_rng(seed)
    tl = np.round(r.uniform(0, 100, (n, 2)) * 8) / 8
    wh = np.round(r.uniform(lo, hi, (n, 2)) * 8) / 8
    return np.concatenate([tl, tl + wh], 1)


def _tile(rows, n):
    return np.concatenate([rows] * (n // len(rows) + 1))[:n].copy()


# ------------------------------------------------------------------ bbox_iou
IOU_SPECIAL = np.array([
    [5, 5, 5, 5],                    # zero area; with itself 0 / 0
    [0, 0, 10, 10],
    [10, 10, 20, 20],                # touches the row above: tl == br
    [20, 20, 10, 10],                # inverted
    [nan, 0, 10, 10],
    [0, 0, 10, nan],
    [0, 0, inf, 10],
    [-inf, -inf, inf, inf],
    [-inf, 0, 10, 10],
    [0, 0, BIG, BIG],                # fp32 area overflows
    [-BIG, -BIG, BIG, BIG],
    [2, 3, 12, 9],
], F64)
IOU_SHAPES = ((0, 3), (3, 0), (1, 1), (257, 1), (1, 257), (255, 3))


def _iou_side(n, seed):
    if n == 1:
        return IOU_SPECIAL[:1].copy()                      # the zero-area box
    if n == 3:
        return IOU_SPECIAL[[0, 4, 11]].copy()              # zero area, a NaN row, a plain row
    rows = np.concatenate([IOU_SPECIAL, _rand_boxes(seed, PERIOD - len(IOU_SPECIAL))])
    return _tile(rows, n)


def iou_cases():
    """name -> (a, b); float cases in all four dtype combinations, plus the
    int64 vectors of the reference's own self-test (utils/utils.py:280-284)."""
    out = {}
    for na, nb in IOU_SHAPES:
        a64 = _iou_side(na, 21) if na else np.zeros((0, 4))
        b64 = _iou_side(nb, 22) if nb else np.zeros((0, 4))
        for ta, tb in DTYPES:
            out[f"iou_{na}x{nb}_{tag(ta, tb)}"] = (a64.astype(ta), b64.astype(tb))
    out["iou_selftest_i64"] = (np.array([[1, 2, 3, 4], [3, 5, 7, 8], [-1, -1, -1, -1], [3, 2, 4, 5]]),
                               np.array([[2, 3, 4, 5], [5, 6, 7, 8], [1, 2, 3, 4]]))
    return out


# ------------------------------------------------------------------ bbox2reg
B2R_SIZES = (0, 1, 255, 256, 257)
#                anchor               box
B2R_SPECIAL = [([0, 0, 16, 16], [2, 2, 10, 14]),
               ([4, 0, 4, 16], [2, 2, 10, 14]),           # zero-height anchor: x / 0, log(inf)
               ([0, 0, 16, 16], [6, 2, 6, 14]),           # zero-height box: log 0
               ([0, 0, 16, 16], [10, 2, 2, 14]),          # inverted box: log of a negative
               ([0, 0, 16, 16], [nan, 2, 10, 14]),
               ([0, nan, 16, 16], [2, 2, 10, 14]),
               ([4, 0, 4, 16], [6, 2, 6, 14]),            # 0 / 0
               ([0, 0, 16, 16], [0, 0, 16, 16])]          # log 1


def b2r_table():
    """(anchors, boxes) fp64 [257,4]; the cases are prefixes of it."""
    sa = np.array([a for a, _ in B2R_SPECIAL], F64)
    sb = np.array([b for _, b in B2R_SPECIAL], F64)
    # row 0 is a plain pair, so that n = 1 has finite targets
    a = np.concatenate([_rand_boxes(31, 1), sa, _rand_boxes(32, PERIOD - 1 - len(sa))])
    b = np.concatenate([_rand_boxes(33, 1), sb, _rand_boxes(34, PERIOD - 1 - len(sb))])
    return _tile(a, 257), _tile(b, 257)


def b2r_cases():
    """name -> (anchors, boxes), n in B2R_SIZES x the four dtype combinations."""
    a64, b64 = b2r_table()
    return {f"b2r_{n}_{tag(ta, tb)}": (a64[:n].astype(ta), b64[:n].astype(tb))
            for n in B2R_SIZES for ta, tb in DTYPES}


def b2r_log_arguments():
    """The fp32 quotients the both-fp32 path takes the log of, over the table."""
    a, b = (x.astype(F32) for x in b2r_table())
    with np.errstate(all="ignore"):
        return np.concatenate([(b[:, 2] - b[:, 0]) / (a[:, 2] - a[:, 0]), (b[:, 3] - b[:, 1]) / (a[:, 3] - a[:, 1])])


# ------------------------------------------------------------------ reg2bbox
R2B_SIZES = (0, 1, 257)


def r2b_table():
    """(anchors, deltas) fp32 [257,4]."""
    r = np.random.default_rng(41)
    a = _rand_boxes(42)
    d = np.round(r.standard_normal((PERIOD, 4)) * 0.3 * 64) / 64
    row = 1                                           # row 0 stays plain (the n = 1 case)
    for col in range(4):
        for v in (inf, -inf, nan):                    # each non-finite delta in each column
            d[row, col] = v
            row += 1
    d[row, 2], d[row + 1, 3] = 88.8, 88.8             # exp overflows to inf in fp32
    d[row + 2, 2], d[row + 3, 3] = -104.0, -104.0     # exp underflows to zero
    a[row + 4] = [7, 9, 7, 9]                         # zero-size anchor x infinite exp: 0 * inf
    d[row + 4, 2:] = 88.8
    a[row + 5] = [7, 9, 7, 9]
    d[row + 5, 2:] = inf
    a[row + 6] = [7, 9, 7, 30]                        # zero height only
    d[row + 6] = [0.25, -0.5, 88.8, 0.125]
    assert row + 7 <= PERIOD
    return _tile(a, 257).astype(F32), _tile(d, 257).astype(F32)


# ------------------------------------------------------------- roi_transform
ROI_SIZES = (0, 1, 257)
ROI_IMG_H, ROI_IMG_W, ROI_FEAT_H, ROI_FEAT_W = 600, 1000, 37, 63    # 600 and 1000: no powers of two


def roi_table():
    """(rois fp32 [257,4], roi_inds fp32 [257])."""
    r = np.random.default_rng(51)
    rois = r.uniform(0, 1000, (PERIOD, 4))
    # thirds and sevenths: x / 600 * 37 and x * (37 / 600) round differently
    rois[1:9] = np.arange(32).reshape(8, 4) / 3 + np.arange(32).reshape(8, 4) / 7
    rois[9] = [-50.5, -0.25, 20, 30]
    rois[10] = [nan, 1, 2, 3]
    rois[11] = [0, inf, -inf, 7]
    rois[12] = [FMAX, -FMAX, FMAX / 2, 1e-45]
    rois[13] = [-0.0, 0.0, 600, 1000]
    inds = np.arange(PERIOD) % 4 + 0.0
    inds[3:7] = [0.5, 1.25, -1.0, 2.999]              # non-integer and negative indices pass through
    inds[10], inds[11] = nan, inf
    return _tile(rois, 257).astype(F32), _tile(inds, 257).astype(F32)


# ------------------------------------------------------------------- anchors
BASE_CASES = {                       # name -> (base_size, ratios, scales)
    "thirds": (16, (1 / 3, 1.0, 3.0), (8, 16, 32)),
    "quarters_one_scale": (16, (0.25, 4.0), (8,)),
    "sixteen_scales": (16, (0.5, 1.0, 2.0), tuple(range(1, 17))),
    "sixteen_ratios": (16, tuple(2.0 ** (k / 4) for k in range(-8, 8)), (8,)),
    "base1": (1, (1 / 3, 1.0, 3.0), (8, 16, 32)),
    "base20": (20, (0.25, 4.0), (2, 4, 8, 16, 32)),
}
TOO_MANY_RATIOS = tuple(1.0 + k / 16 for k in range(17))
GRID_CASES = {                       # name -> (base case, stride, width, height)
    "s1_7x3": ("thirds", 1, 7, 3),
    "s8_5x4": ("base20", 8, 5, 4),
    "s32_9x2": ("quarters_one_scale", 32, 9, 2),
    "g1x1": ("thirds", 16, 1, 1),
    "g1x257": ("quarters_one_scale", 16, 257, 1),     # width 257, height 1
    "g257x1": ("quarters_one_scale", 16, 1, 257),
    "g0x5": ("thirds", 16, 5, 0),                     # no rows
    "g5x0": ("thirds", 16, 0, 5),                     # no columns
}
