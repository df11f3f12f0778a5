"""Named cases of the preprocessing launch plan (DESIGN.md §3 "Preprocessing",
"Launch-plan branches and the cases that pin them"): one case per tile, tap and
fold edge of ``preprocess_kernel`` (csrc/preprocess.hip) that the case table of
tests/preprocess_ref.py does not reach.  Plain numpy, no GPU.

Three things live here.

* ``plan``: the host's launch plan (``axis_radius``, ``span_bound``,
  ``prep_lds`` and the tile-height loop) ported to Python.  The library's
  ``frcnn_preprocess_plan`` must answer the same; the CPU test sweeps both.
* ``axis_band`` / ``preprocess_banded``: the reference of preprocess_ref.py in
  banded form, ``O(n_out * taps)``: per output index the ``2 + 2r`` folded source
  indices and their fp64 weights.  The dense ``gaussian_matrix`` is ``n x n`` and
  cannot run at ``n = 16384``.
* ``tiled``: a restatement of the kernel's *structure* in fp64, tile by tile: the
  tap starts ``i0 - r``, ``r_lo`` / ``c_lo`` / ``nrows`` / ``ncols`` and their
  clamp, the folded footprint, then the horizontal and the vertical pass indexed
  relative to the footprint exactly as the kernel indexes LDS.  Global memory
  and LDS are flat arrays addressed with the kernel's own expressions, and
  whatever the kernel would read without having written it (unstaged LDS, bytes
  outside the image) reads as 0.  With no mistake planted it equals the
  reference to 1e-12; ``MISTAKES`` names the structural mistakes it can plant,
  and every case lists in ``catches`` the ones it must tell apart.

Every case names what it pins and carries the plan it is *meant* to reach at
``max_hw`` = its own size: radius and taps per axis, tile counts, the last
tile's ``ny`` / ``nx``, whether the two-tap instantiation runs, ``TH`` and the
LDS footprint.  A change to the host bound moves a case off its plan loudly:
adjust the case's shape, not its intent.

Users: tests/test_preprocess_plan_cases_cpu.py and tests/test_gpu_preprocess_plans.py.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

import preprocess_ref as R

# ------------------------------------------------------ the host plan, ported
TW = 64                 # kPrepTW
MAX_TH = 32             # kPrepMaxTH
MAX_RATIO = 5           # kPrepMaxRatio
GAUSS = 16              # kPrepGauss
TAP_ROWS = MAX_TH + TW  # kPrepTapRows
LDS_BUDGET = 64 * 1024  # kPrepLdsBudget
PLAN_FIELDS = ("TH", "lds_rows", "lds_cols", "max_taps", "lds_bytes", "grid_x", "grid_y", "grid_z")


def axis_radius(n_in: int, n_out: int) -> int:
    s = (n_in / n_out - 1.0) / 2.0
    if not s > 0.0:
        s = 0.0
    return int(4.0 * s + 0.5)


def span_bound(L: int, max_in: int, n_out: int) -> int:
    m = min(max_in, MAX_RATIO * n_out)
    return ((L - 1) * m + n_out - 1) // n_out + 2 + 2 * axis_radius(m, n_out)


def prep_lds(rows: int, cols: int, max_taps: int) -> int:
    ts = max_taps + 1
    tmp = 2 * GAUSS * 8
    tapw = tmp + rows * 3 * TW * 4
    taps = tapw + TAP_ROWS * ts * 4
    src = taps + TAP_ROWS * 4
    return (src + rows * cols * 3 + 15) // 16 * 16


def plan(N, max_hw, out_hw, min_th=1) -> dict:
    """prep_plan of csrc/preprocess.hip, by PLAN_FIELDS."""
    (max_h, max_w), (out_h, out_w) = max_hw, out_hw
    TH = MAX_TH
    cols = span_bound(TW, max_w, out_w)
    max_taps = max(span_bound(1, max_h, out_h), span_bound(1, max_w, out_w))
    while True:
        rows = span_bound(TH, max_h, out_h)
        total = prep_lds(rows, cols, max_taps)
        if total <= LDS_BUDGET or TH == min_th:
            break
        TH //= 2
    return dict(zip(PLAN_FIELDS, (TH, rows, cols, max_taps, total, (out_w + TW - 1) // TW, (out_h + TH - 1) // TH, N)))


# ------------------------------------------------- the reference, banded form
def tap_start(n_in, n_out: int, d):
    """``i0 = floor(((2d+1) n_in - n_out) / (2 n_out))`` in exact integers;
    ``n_in`` and ``d`` broadcast."""
    return ((2 * np.asarray(d, np.int64) + 1) * n_in - n_out) // (2 * n_out)


def axis_band(n_in: int, n_out: int):
    """(folded source indices int64 [n_out, T], fp64 weights [n_out, T]),
    T = 2 + 2r: row d of preprocess_ref.axis_matrix without its zeros.  Tap j
    sits at i0 - r + j and weighs (1-f) G(j-r) + f G(j-r-1), G the normalised
    Gaussian inside +-r (the identity when s == 0)."""
    s, r = R.sigma_radius(n_in, n_out)
    d = np.arange(n_out, dtype=np.int64)
    den = 2 * n_out
    num = (2 * d + 1) * n_in - n_out
    i0 = num // den
    f = (num - i0 * den) / den
    k = np.arange(-r - 1, r + 2)
    g = np.zeros(2 * r + 3)
    g[1:-1] = np.exp(-0.5 / (s * s) * k[1:-1] ** 2.0) if s > 0 else 1.0
    g /= g.sum()
    j = np.arange(2 + 2 * r)
    w = (1.0 - f)[:, None] * g[j + 1][None] + f[:, None] * g[j][None]   # G(j-r) = g[j+1], G(j-r-1) = g[j]
    idx = (i0 - r)[:, None] + j[None]
    if n_in == 1:
        idx = np.zeros_like(idx)
    else:
        p = 2 * (n_in - 1)
        m = idx % p
        idx = np.where(m < n_in, m, p - m)
    return idx, w


def band_dense(idx, w, n_in: int) -> np.ndarray:
    """The band scattered into the dense [n_out, n_in] matrix."""
    a = np.zeros((idx.shape[0], n_in))
    np.add.at(a, (np.arange(idx.shape[0])[:, None], idx), w)
    return a


def preprocess_banded(img: np.ndarray, out_hw, mean=R.MEAN, std=R.STD) -> np.ndarray:
    """preprocess_ref.preprocess through the banded matrices: uint8 [h, w, 3] -> fp64 [3, oh, ow]."""
    p = img.astype(np.float64) / 255
    ih, wh = axis_band(p.shape[0], out_hw[0])
    iw, ww = axis_band(p.shape[1], out_hw[1])
    q = (p[:, iw, :] * ww[None, :, :, None]).sum(2)          # [h, ow, 3]
    q = (q[ih] * wh[:, :, None, None]).sum(1)                # [oh, ow, 3]
    out = (q - np.asarray(mean, np.float64)) / np.asarray(std, np.float64)
    return np.ascontiguousarray(out.transpose(2, 0, 1))


# ---------------------------------------- the kernel's structure, tile by tile
MISTAKES = (
    "fold_edge_repeat",    # the fold repeats the edge pixel (period 2n: -1 -> 0, n -> n-1)
    "radius_trunc",        # r = int(4 s), without the + 0.5
    "drop_last_tap",       # the Gaussian's last tap (k = +-r) is left out of the weights
    "swap_rh_rw",          # the horizontal pass counts its taps with rh
    "c_lo_tile0",          # c_lo of the first x tile used for every tile
    "r_lo_tile0",          # r_lo of the first y tile used for every tile
    "ny_full_last",        # ny = TH in the last y tile
    "footprint_short",     # the staged footprint is one column short
    "fold_before_origin",  # fold(r) + r_lo instead of fold(r_lo + r), both axes
)


def _fold(i, n: int, edge_repeat=False):
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    if edge_repeat:
        m = i % (2 * n)
        return np.where(m < n, m, 2 * n - 1 - m)
    p = 2 * (n - 1)
    m = i % p
    return np.where(m < n, m, p - m)


def _read(mem: np.ndarray, idx) -> np.ndarray:
    """mem[idx]; what lies outside the array reads as 0."""
    idx = np.asarray(idx, np.int64)
    ok = (idx >= 0) & (idx < mem.size)
    return np.where(ok, mem[np.where(ok, idx, 0)], 0.0)


def _write(mem: np.ndarray, idx, val) -> None:
    idx, val = np.broadcast_arrays(np.asarray(idx, np.int64), val)
    ok = (idx >= 0) & (idx < mem.size)
    mem[idx[ok]] = val[ok]


def _radius(n_in: int, n_out: int, mistake):
    s = (n_in / n_out - 1.0) / 2.0
    if not s > 0.0:
        s = 0.0
    return (int(4.0 * s) if mistake == "radius_trunc" else int(4.0 * s + 0.5)), s * s


def _tap_row(d: int, n_in: int, n_out: int, r: int, s2: float, drop_last=False):
    """Step 1 of the kernel for one output index: (i0 - r, the 2 + 2r weights)."""
    num, den = (2 * d + 1) * n_in - n_out, 2 * n_out
    i0 = -1 if num < 0 else num // den
    f = (num - i0 * den) / den
    if r == 0:
        return i0, [1.0 - f, f]
    g = [1.0 if kk == 0 else (math.exp(-0.5 / s2 * (kk * kk)) if kk <= r - drop_last else 0.0)
         for kk in range(GAUSS)]
    total = g[0] + sum(2.0 * g[kk] for kk in range(1, r + 1))
    wt = []
    for j in range(2 + 2 * r):
        ka, kb = abs(j - r), abs(j - r - 1)
        ga, gb = (g[ka] if ka <= r else 0.0), (g[kb] if kb <= r else 0.0)
        wt.append(((1.0 - f) * ga + f * gb) / total)
    return i0 - r, wt


def axis_span(n_in: int, n_out: int, d0: int, L: int) -> int:
    """Source rows (columns) the tile of outputs d0 .. d0+L-1 (cut at n_out)
    reaches: what the kernel computes as nrows / ncols before its clamp."""
    r = axis_radius(n_in, n_out)
    last = min(d0 + L, n_out) - 1
    return int(tap_start(n_in, n_out, last) - tap_start(n_in, n_out, d0)) + 2 + 2 * r


def tiled(img: np.ndarray, out_hw, pl: dict, mean=R.MEAN, std=R.STD, mistake=None, trace=None) -> np.ndarray:
    """preprocess_kernel restated in fp64 for one image under the plan ``pl``:
    uint8 [h, w, 3] -> fp64 [3, oh, ow].  ``mistake`` plants one of MISTAKES;
    ``trace`` (a list) receives (y0, x0, ny, nx, nrows, ncols) per tile, the
    footprint as computed before the clamp."""
    assert mistake is None or mistake in MISTAKES, mistake
    h, w = img.shape[:2]
    out_h, out_w = out_hw
    TH, lds_rows, lds_cols, ts = pl["TH"], pl["lds_rows"], pl["lds_cols"], pl["max_taps"] + 1
    pixels = img.reshape(-1).astype(np.float64)
    plane = out_h * out_w
    out = np.full(3 * plane, np.nan)
    scale = 1.0 / (255.0 * np.asarray(std, np.float64))
    bias = -np.asarray(mean, np.float64) / np.asarray(std, np.float64)
    rh, s2h = _radius(h, out_h, mistake)
    rw, s2w = _radius(w, out_w, mistake)
    edge = mistake == "fold_edge_repeat"
    drop = mistake == "drop_last_tap"
    ch = np.arange(3)
    first_lo = None
    for y0 in range(0, out_h, TH):
        for x0 in range(0, out_w, TW):
            ny = min(out_h - y0, TH)
            if mistake == "ny_full_last":
                ny = TH
            nx = min(out_w - x0, TW)
            # 1. tap tables, rows 0..TH-1 for axis h, MAX_TH.. for axis w, ts floats per row
            taps = np.zeros(TAP_ROWS, np.int64)
            tapw = np.zeros(TAP_ROWS * ts)
            for y in range(ny):
                taps[y], wt = _tap_row(y0 + y, h, out_h, rh, s2h, drop)
                tapw[y * ts:y * ts + len(wt)] = wt
            for x in range(nx):
                taps[MAX_TH + x], wt = _tap_row(x0 + x, w, out_w, rw, s2w, drop)
                tapw[(MAX_TH + x) * ts:(MAX_TH + x) * ts + len(wt)] = wt
            r_lo, c_lo = int(taps[0]), int(taps[MAX_TH])
            if first_lo is None:
                first_lo = (r_lo, c_lo)
            if mistake == "r_lo_tile0":
                r_lo = first_lo[0]
            if mistake == "c_lo_tile0":
                c_lo = first_lo[1]
            nrows = int(taps[ny - 1]) + 2 + 2 * rh - r_lo
            ncols = int(taps[MAX_TH + nx - 1]) + 2 + 2 * rw - c_lo
            if trace is not None:
                trace.append((y0, x0, ny, nx, nrows, ncols))
            nrows, ncols = min(nrows, lds_rows), min(ncols, lds_cols)
            if mistake == "footprint_short":
                ncols -= 1
            row_b = ncols * 3
            # 2. the footprint, folded, byte for byte
            src = np.zeros(lds_rows * lds_cols * 3)
            rr, cc = np.arange(nrows), np.arange(ncols)
            if mistake == "fold_before_origin":
                g_row, g_col = _fold(rr, h) + r_lo, _fold(cc, w) + c_lo
            else:
                g_row, g_col = _fold(r_lo + rr, h, edge), _fold(c_lo + cc, w, edge)
            gi = g_row[:, None, None] * (w * 3) + g_col[None, :, None] * 3 + ch[None, None, :]
            _write(src, rr[:, None, None] * row_b + cc[None, :, None] * 3 + ch[None, None, :], _read(pixels, gi))
            # 3. horizontal pass to tmp [row][channel][64]
            lane = np.arange(nx)
            tw = 2 + 2 * (rh if mistake == "swap_rh_rw" else rw)
            sx = (taps[MAX_TH + lane] - c_lo) * 3
            j = np.arange(tw)
            si = rr[:, None, None, None] * row_b + sx[None, :, None, None] + 3 * j[None, None, :, None] + ch
            wx = _read(tapw, (MAX_TH + lane)[:, None] * ts + j[None, :])                   # [nx, tw]
            acc = (_read(src, si) * wx[None, :, :, None]).sum(2)                           # [nrows, nx, 3]
            tmp = np.zeros(lds_rows * 3 * TW)
            _write(tmp, rr[:, None, None] * 3 * TW + ch[None, None, :] * TW + lane[None, :, None], acc)
            # 4. vertical pass, normalise, store
            th = 2 + 2 * rh
            y = np.arange(ny)
            j = np.arange(th)
            ti = ((taps[y] - r_lo)[:, None, None, None] + j[None, None, :, None]) * 3 * TW + ch * TW \
                + lane[None, :, None, None]
            wy = _read(tapw, y[:, None] * ts + j[None, :])                                 # [ny, th]
            acc = (_read(tmp, ti) * wy[:, None, :, None]).sum(2)                           # [ny, nx, 3]
            oi = ch[None, None, :] * plane + (y0 + y)[:, None, None] * out_w + x0 + lane[None, :, None]
            _write(out, oi, acc * scale + bias)
    return out.reshape(3, out_h, out_w)


# ------------------------------------------------------------------ the table
Case = namedtuple("Case", "id in_hw out_hw pins r tiles last fast TH lds kinds catches")

# r = (rh, rw); tiles = (y tiles, x tiles); last = (ny, nx) of the last tile;
# fast = the two-tap instantiation runs; lds = (lds_rows, lds_cols, lds_bytes);
# all at max_hw = in_hw.  kinds = the images the GPU test runs.
CASES = [
    Case("down_x_tiles", (90, 200), (45, 100),
         "slow path at x0 = 64 (nx = 36); y tiles 16, 16, 13; plan TH 16, 36 x 132",
         (2, 2), (3, 2), (13, 36), False, 16, (36, 132, 45232), ("random",),
         ("drop_last_tap", "c_lo_tile0", "r_lo_tile0", "fold_before_origin")),
    Case("radius_rounds_up", (46, 161), (20, 70),
         "ratio 2.3: r = 3 only through the + 0.5; x tiles 64 + 6",
         (3, 3), (2, 2), (4, 6), False, 16, (43, 153, 56864), ("random",),
         ("radius_trunc", "c_lo_tile0")),
    Case("ratio5", (60, 60), (12, 12),
         "accepted limit, r = 8, 18 taps; TH 2; footprint 23 x 333",
         (8, 8), (6, 1), (2, 12), False, 2, (23, 333, 48592), ("random", "checker"),
         ("drop_last_tap", "r_lo_tile0")),
    Case("ratio5_wide", (30, 650), (6, 130),
         "r = 8 over x tiles 64, 64, 2",
         (8, 8), (3, 3), (2, 2), False, 2, (23, 333, 48592), ("random",),
         ("c_lo_tile0", "drop_last_tap")),
    Case("down_up", (120, 40), (40, 100),
         "rh = 4, rw = 0: slow path with two horizontal taps",
         (4, 0), (3, 2), (8, 36), False, 16, (55, 28, 51728), ("random",),
         ("fold_edge_repeat", "footprint_short", "r_lo_tile0")),
    Case("up_down", (20, 300), (50, 100),
         "rh = 0, rw = 4; TH 32, y tiles 32 + 18",
         (0, 4), (2, 2), (18, 36), False, 32, (15, 199, 25344), ("random",),
         ("swap_rh_rw", "r_lo_tile0", "ny_full_last", "fold_before_origin")),
    Case("w64", (10, 96), (10, 64),
         "nx == 64 exactly, one x tile",
         (0, 1), (1, 1), (10, 64), False, 32, (33, 99, 37712), ("random",),
         ("footprint_short",)),
    Case("w65", (10, 98), (10, 65),
         "a last tile of one column",
         (0, 1), (1, 2), (10, 1), False, 32, (33, 99, 37712), ("random",),
         ("fold_edge_repeat", "c_lo_tile0")),
    Case("h33_slow", (66, 20), (33, 16),
         "a last tile of one row at TH 16",
         (2, 1), (3, 1), (1, 16), False, 16, (36, 83, 39952), ("random",),
         ("r_lo_tile0", "ny_full_last")),
    # 20 -> 16 columns shrink (r = 1), so (20, 20) -> (33, 16) runs the slow instantiation: it stays
    # as h33_th32, and h33_fast takes 12 -> 16 columns to reach the two-tap one its name asks for
    Case("h33_fast", (20, 12), (33, 16),
         "a last tile of one row at TH 32, two-tap instantiation",
         (0, 0), (2, 1), (1, 16), True, 32, (21, 50, 21072), ("random",),
         ("r_lo_tile0", "ny_full_last", "footprint_short")),
    Case("h33_th32", (20, 20), (33, 16),
         "a last tile of one row at TH 32, rh = 0 beside rw = 1",
         (0, 1), (2, 1), (1, 16), False, 32, (21, 83, 23920), ("random",),
         ("r_lo_tile0", "ny_full_last")),
    Case("two_rows", (2, 40), (1, 20),
         "n = 2 rows: fold period 2 walked several times by r = 2",
         (2, 2), (1, 1), (1, 20), False, 16, (36, 132, 45232), ("random", "checker"),
         ("fold_edge_repeat", "fold_before_origin")),
    Case("two_by_two", (2, 2), (1, 1),
         "n = 2 on both axes, one output element",
         (2, 2), (1, 1), (1, 1), False, 16, (36, 132, 45232), ("random",),
         ("fold_before_origin",)),
    Case("one_row", (1, 130), (3, 65),
         "n = 1 fold on one axis, Gaussian on the other",
         (0, 2), (1, 2), (3, 1), False, 32, (13, 132, 18464), ("random",),
         ("c_lo_tile0", "swap_rh_rw")),
    Case("voc_down", (500, 375), (200, 150),
         "a realistic shrink; LDS 62,336 B of the 65,536 budget",
         (3, 3), (13, 3), (8, 22), False, 16, (46, 166, 62336), ("random",),
         ("c_lo_tile0", "r_lo_tile0", "ny_full_last")),
    Case("max_extent", (2, 16384), (1, 4096),
         "widest accepted source and output, 64 x tiles, integer positions near 2^27; banded reference only",
         (2, 6), (1, 64), (1, 64), False, 16, (36, 266, 62784), ("random",),
         ("c_lo_tile0", "swap_rh_rw")),
]
CASE_IDS = [c.id for c in CASES]
BANDED_ONLY = ("max_extent",)     # too wide for the dense n x n Gaussian matrix


def case(cid: str) -> Case:
    return CASES[CASE_IDS.index(cid)]


# The tile-height ladder: one image to out (40, 100) at host bounds under which TH takes
# each of 32, 16, 8, 4, 2.  (max_hw, TH); the first rung is the image's own size.
LADDER_IMAGE = (30, 437)
LADDER_OUT = (40, 100)
LADDER = [((30, 437), 32), ((40, 500), 16), ((80, 500), 8), ((160, 500), 4), ((200, 500), 2)]

_cache = {}


def case_image(c: Case, kind="random") -> np.ndarray:
    return R.image(c.in_hw, kind, seed=100 + CASE_IDS.index(c.id))


def case_data(c: Case, kind="random"):
    """(uint8 image, fp64 reference [3, oh, ow]) of a case and image kind;
    computed once, read-only.  The dense reference, the banded one for BANDED_ONLY."""
    key = (c.id, kind)
    if key not in _cache:
        img = case_image(c, kind)
        ref = preprocess_banded(img, c.out_hw) if c.id in BANDED_ONLY else R.preprocess(img, c.out_hw)
        ref.setflags(write=False)
        img.setflags(write=False)
        _cache[key] = (img, ref)
    return _cache[key]


def ladder_data():
    key = "ladder"
    if key not in _cache:
        img = R.image(LADDER_IMAGE, "random", seed=99)
        ref = R.preprocess(img, LADDER_OUT)
        ref.setflags(write=False)
        img.setflags(write=False)
        _cache[key] = (img, ref)
    return _cache[key]
