"""Named cases of RoIPool's launch plans (DESIGN.md §3 "Launch-plan branches"):
one case per branch of ``choose_fwd`` / ``px_plan`` / ``dense_plan`` / ``bwd_plan``
in csrc/roi_pool.hip that plain ``ops.roi_pool`` arguments reach away from the
benchmark's shapes.  Plain numpy, no GPU.

Every case carries its shape (N, C, H, W, output size), its RoIs grouped by
image plus a fixed permutation for the ungrouped run, the dtypes it runs in
and the kernel it is *meant* to reach: ``fwd`` (RoIs grouped, RoIs in any
order) and ``bwd`` (per ``roi_pool_bwd`` path).  The intent is checked in two
steps.  ``fwd_plan`` / ``bwd_plan`` below restate the host's plan functions
over the constants read from the source (``constants()``), and a case whose
intent the restated plan does not give fails tests/test_pool_plan_cases_cpu.py;
tests/test_gpu_pool_plans.py then asserts that the library's own name query
answers ``fwd_name`` / ``bwd_name`` before it compares a single value.  So a
change to a threshold moves a case off its kernel loudly: adjust the case's
shape, not its intent.

Inputs follow tests/test_gpu_parity.py::test_roi_pool_vs_oracle: normal
features partly rounded (ties: the first maximum must win), RoIs that reach
off the map or lie wholly outside it, zero-size and negative-size RoIs,
duplicated RoIs, tiny RoIs whose bins share pixels, images with 0 and 1 RoIs
and, where ``invalid`` is set, batch indices outside [0, N) (they pool to
0 / -1 and receive no gradient; torchvision reads out of bounds there, so the
references below run the oracle on the valid rows only).

Users: tests/test_pool_plan_cases_cpu.py (each case can catch what it is for,
on the oracle alone) and tests/test_gpu_pool_plans.py (HIP path == oracle).
"""
from __future__ import annotations

import math
import os
import re

import numpy as np

from oracle import ref_numpy as orc

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "replication_faster_rcnn_amd", "csrc", "roi_pool.hip")
MI355X_CUS = 256
ALL = ("f32", "f16", "bf16")
ELEM = {"f16": "__half", "bf16": "__hip_bfloat16"}
BWD_PATHS = ("auto", "ring", "plain")


# ------------------------------------------------------- the source's constants
class _K:
    pass


_consts = None


def constants():
    """The plan constants of csrc/roi_pool.hip, read from the source text."""
    global _consts
    if _consts is None:
        with open(SOURCE) as f:
            src = f.read()
        k = _K()
        for name, expr in re.findall(r"constexpr\s+(?:size_t|int)\s+(k\w+)\s*=\s*([0-9*+\s]+);", src):
            setattr(k, name, int(eval(expr, {"__builtins__": {}})))  # digits, * and + only
        k.kBwdLead = int(re.search(r"#define\s+FRCNN_BWD_LEAD_D\s+(\d+)", src).group(1))
        for need in ("kLdsPerCu", "kPlaneBudget", "kPlaneBudgetRing", "kBwdXRow", "kMaxBins", "kBwdRing",
                     "kFixPx", "kWaveScratch", "kDenseMisc"):
            assert hasattr(k, need), f"{need} not found in {SOURCE}"
        _consts = k
    return _consts


# ------------------------------------------------- the host's plans, restated
def fwd_plan(N, C, H, W, PH, PW, grouped):
    """choose_fwd under ``auto``: ("wave", cg, kps) | ("dense", cg) | ("dense_list", cg) | ("generic", vec)."""
    k = constants()
    HW, PHW = H * W, PH * PW
    generic = ("generic", (C * PHW) % 4 == 0)
    if N <= 0 or C <= 0 or HW == 0 or PHW > 64 or H > 65535 or W > 65535:
        return generic
    if grouped:  # px_plan
        reserve, min_geo = 1024, 64 * 16
        HWs = (HW + 16) & ~15

        def per_cu(tile):
            if 2 * (tile + min_geo + k.kWaveScratch + reserve) <= k.kLdsPerCu:
                return 2
            return 1 if tile + min_geo + k.kWaveScratch + reserve <= k.kLdsPerCu else 0

        for cg in (16, 8, 4):
            if C % cg:
                continue
            tile_rt = (cg // 4) * HWs * 16
            kps = cg == 16 and PH == 7 and PW == 7 and HWs <= k.kFixPx and per_cu(tile_rt) == 1
            if per_cu((cg // 4) * k.kFixPx * 16 if kps else tile_rt):
                return ("wave", cg, kps)
    HWs = (HW + 15) & ~15  # dense_plan
    fixed = 256 * 4 + k.kDenseMisc * 4 + 64
    for cg in (16, 8, 4):
        if C % cg:
            continue
        tile = (cg // 4) * HWs * 16
        if tile < 2 ** 31 and tile + fixed + 64 * (16 + 4 + 4 + 1) <= k.kLdsPerCu:
            return ("dense" if grouped else "dense_list", cg)
    return generic


def _typed(dtype, kernel, args):
    return f"{kernel}<{args}>" if dtype == "f32" else f"{kernel}_h<{ELEM[dtype]}, {args}>"


def fwd_name(dtype, N, C, H, W, PH, PW, grouped, head=False):
    """What frcnn_roi_pool_fwd_kernel_t answers under ``auto``."""
    pl = fwd_plan(N, C, H, W, PH, PW, grouped)
    fx = 7 if (PH, PW) == (7, 7) else 0
    hb = "true" if head else "false"
    if pl[0] == "wave":
        args = f"1024, {pl[1]}, {fx}, {hb}" + (f", false, {constants().kFixPx * 16}" if pl[2] else "")
        return _typed(dtype, "roi_pool_fwd_wave_kernel", args)
    if pl[0] == "dense":
        return _typed(dtype, "roi_pool_fwd_dense_kernel", f"1024, {pl[1]}, {fx}, {hb}, false")
    if pl[0] == "dense_list":
        return _typed(dtype, "roi_pool_fwd_dense_kernel", f"1024, {pl[1]}, {fx}, false, true")
    return _typed(dtype, "roi_pool_fwd_kernel", "true" if pl[1] else "false")


def bwd_plan(R, N, C, H, W, PH, PW, path="auto", cus=MI355X_CUS):
    """bwd_plan + the launch's own choice between the plain kernel's two forms:
    (kind, channels per workgroup), kind in lead | pf | plain_lds | plain_global."""
    k = constants()
    HW, PHW = H * W, PH * PW
    plane = HW * 4
    if PHW <= 64 and path != "plain" and 0 < plane <= k.kPlaneBudgetRing:
        icpw = max(1, min(-(-N * C // cus), 16, k.kPlaneBudgetRing // plane, C))
        fits = R * C * PHW * 4 < 2 ** 31
        HWs = (HW + 64 + 3) & ~3
        lead_bytes = icpw * (HWs * 4 + 2 * k.kBwdXRow * 8)
        lead = fits and path == "auto" and PHW < 64 and PW == 7 and lead_bytes <= k.kPlaneBudgetRing
        return ("lead" if lead else "pf", icpw)
    if plane <= k.kPlaneBudget:
        return ("plain_lds", min(k.kPlaneBudget // plane, 16, C))
    return ("plain_global", 4)


def bwd_name(dtype, R, N, C, H, W, PH, PW, path="auto", cus=MI355X_CUS):
    """What frcnn_roi_pool_bwd_kernel_t answers with ``roi_pool_bwd`` set to ``path``."""
    k = constants()
    kind = bwd_plan(R, N, C, H, W, PH, PW, path, cus)[0]
    if kind == "lead":
        return _typed(dtype, "roi_pool_bwd_lead_kernel", f"{k.kBwdLead}, 7, {7 if PH == 7 else 0}")
    if kind == "pf":
        return _typed(dtype, "roi_pool_bwd_pf_kernel", f"{k.kBwdRing}")
    return _typed(dtype, "roi_pool_bwd_kernel", "true" if kind == "plain_lds" else "false")


def fits_edge(C, PHW):
    """Largest R with R*C*PHW*4 < 2^31: the leader backward's descriptor precondition."""
    return (2 ** 31 - 1) // (C * PHW * 4)


# ------------------------------------------------------------------- the cases
class PoolCase:
    """group: bins (> 64 bins) | global | budget | tile | wide | partial.
    counts: RoIs per image drawn by the recipe (specials are added to the fullest image).
    fwd: intended forward kernel (grouped, ungrouped); bwd: {path: intended kind}, empty = no
    backward run.  icpw: {path: channels per workgroup on an MI355X}, for the partly filled
    cases.  head: also run through ops.roi_pool_head."""

    def __init__(self, name, group, N, C, H, W, size, counts, *, dtypes=ALL, fwd, bwd, seed, span=None,
                 invalid=False, icpw=None, head=False):
        self.name, self.group, self.N, self.C, self.H, self.W = name, group, N, C, H, W
        self.size, self.counts, self.dtypes, self.fwd, self.bwd = size, counts, dtypes, fwd, bwd
        self.seed, self.span, self.invalid, self.icpw, self.head = seed, span, invalid, icpw or {}, head
        assert len(counts) == N and 0 in counts or N == 1, name
        self._in = None

    @property
    def PHW(self):
        return self.size[0] * self.size[1]

    def __repr__(self):
        return self.name

    # -- inputs, built once
    def inputs(self):
        """(x fp32 [N,C,H,W], rois fp32 [R,5] grouped by image, perm: the ungrouped order)."""
        if self._in is None:
            r = np.random.default_rng(self.seed)
            x = r.standard_normal((self.N, self.C, self.H, self.W), dtype=F32)
            x[:, :, ::3, ::2] = np.round(x[:, :, ::3, ::2])          # ties: the first maximum wins
            x[:, :, : self.H // 2 + 1, : min(self.W, 12)] = np.round(x[:, :, : self.H // 2 + 1, : min(self.W, 12)])
            rois = _rois(r, self)
            self._in = (x, rois, r.permutation(len(rois)))
        return self._in

    @property
    def R(self):
        return len(self.inputs()[1])

    def rois(self, grouped=True):
        _, rois, perm = self.inputs()
        return rois if grouped else np.ascontiguousarray(rois[perm])

    def grad(self):
        """fp32 [R,C,PH,PW], for the grouped order."""
        r = np.random.default_rng(self.seed + 1000)
        return r.standard_normal((self.R, self.C) + tuple(self.size), dtype=F32)

    def head_inputs(self):
        """(image rois [R,4], indices [R], img_h, img_w) whose transform lands on the
        case's RoIs up to rounding: the reference's [0, 2] / [1, 3] column scaling."""
        rois = self.rois()
        img_h, img_w = 16.0 * self.H, 16.0 * self.W
        r4 = rois[:, 1:].copy()
        r4[:, [0, 2]] *= F32(img_h / self.H)
        r4[:, [1, 3]] *= F32(img_w / self.W)
        return r4.astype(F32), rois[:, 0].copy(), img_h, img_w


def _rois(r, case):
    N, H, W, m = case.N, case.H, case.W, max(case.H, case.W)
    rows = []
    full = int(np.argmax(case.counts))
    for b, n in enumerate(case.counts):
        xy = r.uniform(-3, m + 2, (n, 2))
        wh = r.uniform(-2, m, (n, 2)) if case.span is None else r.uniform(-2, case.span, (n, 2))
        if H == 1:  # one pixel row: keep the RoIs near it
            xy[:, 1] = r.uniform(-2, 2, n)
            wh[:, 1] = r.uniform(-1, 3, n)
        rows += [[b, x0, y0, x0 + w, y0 + h] for (x0, y0), (w, h) in zip(xy, wh)]
        if b != full:
            continue
        cx, cy = min(W - 1, 7), min(H - 1, 5)
        sx = W - 6 if W > 8 else 0
        rows += [
            [b, cx, cy, cx, cy],                          # zero size: one pixel
            [b, cx + 2, cy, cx - 1, cy - 2],              # negative size
            [b, -40, -30, -20, -10],                      # wholly off the map
            [b, W + 5, 0, W + 30, H - 1],                 # wholly right of it
            [b, 0, 0, W - 1, H - 1],                      # the whole map
            [b, -2, -2, 2.4, 1.4],                        # a corner, partly off
            [b, sx, max(H - 3, 0), W + 3, H + 2],         # the far corner, partly off
            # tiny RoIs: many bins on few pixels
            [b, cx, cy, cx + 0.4, cy + 0.4], [b, cx, cy, cx + 2, cy + 1], [b, cx - 1, cy, cx + 2, cy + 3],
            [b, cx, cy, cx + 3, cy + 2], [b, 1, 0, 4, 0], [b, 2, 0, 2.4, 0.4], [b, cx, cy, cx + 5, cy + 4],
        ]
        rows += rows[-9:] + rows[-4:]                     # duplicated RoIs
        if W > 60000:                                     # columns at the far end of a long row
            rows += [[b, W - 40, 0, W + 10, 0], [b, 100, 0, W - 100, 0], [b, W - 3, -1, W - 1, 1]]
    if case.invalid:
        rows = [[-3, 0, 0, 5, 5], [-1, 1, 1, 9, 9]] + rows + [[N, 2, 2, 8, 8], [N + 7, 0, 0, 3, 3]]
    rois = np.array(rows, F32)
    assert (np.diff(rois[:, 0]) >= 0).all()
    return rois


def _bins(name, size, N, C, H, W, counts, seed, **kw):
    vec = (C * size[0] * size[1]) % 4 == 0
    return PoolCase(name, "bins", N, C, H, W, size, counts, seed=seed, fwd=(("generic", vec),) * 2,
                    bwd={"auto": "plain_lds"}, head=True, **kw)


def _budget(name, H, W, auto, **kw):
    bwd = {"auto": auto, "ring": "pf" if auto != "plain_global" else "plain_global", "plain": "plain_global"}
    return PoolCase(name, "budget", 1, 2, H, W, (7, 7), [34], seed=H * 1000 + W, span=60,
                    fwd=(("generic", False),) * 2, bwd=bwd, **kw)


def _partial(name, N, counts, icpw, **kw):
    return PoolCase(name, "partial", N, 257, 8, 8, (7, 7), counts, seed=257 + N, invalid=True,
                    fwd=(("generic", False),) * 2, bwd={"auto": "lead", "ring": "pf", "plain": "plain_lds"},
                    icpw=icpw, **kw)


CASES = [
    # ---- more than 64 bins: the generic forward, roi_bwd_prep_kernel + the plain kernel's chunked walk
    _bins("bins_13x5", (13, 5), 4, 4, 20, 27, [22, 0, 1, 16], 135),                 # 65: one lane in chunk 1
    _bins("bins_9x9", (9, 9), 4, 8, 20, 27, [20, 0, 1, 14], 99, invalid=True),
    _bins("bins_14x14", (14, 14), 4, 8, 40, 40, [24, 1, 0, 16], 1414, invalid=True),
    _bins("bins_9x9_c3", (9, 9), 4, 3, 20, 27, [20, 0, 1, 12], 93, dtypes=("f32", "bf16")),  # scalar stores
    _bins("bins_1x65", (1, 65), 4, 4, 20, 27, [22, 0, 1, 16], 165),
    _bins("bins_65x1", (65, 1), 4, 4, 20, 27, [22, 0, 1, 16], 651, dtypes=("f32", "f16")),
    _bins("bins_3x341", (3, 341), 4, 4, 40, 40, [20, 1, 0, 10], 3341, dtypes=("f32", "f16")),
    _bins("bins_32x32", (32, 32), 4, 4, 40, 40, [22, 0, 1, 8], 3232, invalid=True),    # kMaxBins itself
    # ---- fp32 (and 16-bit) planes too large for any LDS budget
    PoolCase("global_130", "global", 1, 2, 130, 130, (7, 7), [34], seed=130, span=50,
             fwd=(("generic", False),) * 2, bwd={"auto": "lead", "ring": "pf", "plain": "plain_global"}),
    # ---- the 144 KB window under auto, N = 1, C = 2 (no forward tile fits either)
    _budget("budget_190", 190, 190, "lead"),
    _budget("budget_191", 191, 191, "pf"),             # the plane fits, plane + dummies + rows does not
    _budget("budget_192", 192, 192, "pf"),             # exactly kPlaneBudgetRing
    _budget("budget_192x193", 192, 193, "plain_global"),
    # ---- the 4-channel wave tile's plane limit, from below (exactly) and from above
    PoolCase("tile_98x103", "tile", 1, 4, 98, 103, (7, 7), [70], seed=98103, span=40,
             fwd=(("wave", 4, False), ("generic", True)), bwd={}),
    PoolCase("tile_99x102", "tile", 1, 4, 99, 102, (7, 7), [70], seed=99102, span=40,
             fwd=(("generic", True),) * 2, bwd={}),
    # ---- W beyond the tile kernels' 16-bit coordinates
    PoolCase("wide_65536", "wide", 1, 4, 1, 65536, (7, 7), [24], seed=65536, span=3000,
             fwd=(("generic", True),) * 2, bwd={"auto": "plain_global"}, dtypes=("f32", "bf16")),
    # ---- partly filled backward workgroups: C = 257 is prime
    _partial("partial_n2", 2, [0, 26], {"auto": 3, "ring": 3, "plain": 16}),
    _partial("partial_n3", 3, [1, 0, 25], {"auto": 4, "ring": 4, "plain": 16}),
    _partial("partial_n16", 16, [3, 0, 1, 4, 2, 3, 0, 2, 5, 1, 2, 3, 2, 0, 4, 3],
             {"auto": 16, "ring": 16, "plain": 16}),
    PoolCase("partial_130", "partial", 2, 257, 130, 130, (7, 7), [0, 26], seed=257130, span=30, dtypes=("f32",),
             fwd=(("generic", False),) * 2, bwd={"auto": "lead", "ring": "pf", "plain": "plain_global"},
             icpw={"auto": 2, "ring": 2, "plain": 4}),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
BWD_CASES = [c for c in CASES if c.bwd]
REJECTED_SIZES = [(25, 41), (0, 7)]     # 1,025 bins; no bins

# the `fits` guard (name query only): C, N, H, W of a 7x7 head whose R is set at the edge
FITS_SHAPE = dict(N=8, C=256, H=38, W=63)


# --------------------------------------------------------------- the references
_ref = {}


def valid_rows(case, grouped=True):
    b = case.rois(grouped)[:, 0].astype(np.int64)
    return (b >= 0) & (b < case.N)


def _with_invalid(valid, out_v, am_v):
    out = np.zeros((len(valid),) + out_v.shape[1:], out_v.dtype)
    am = np.full((len(valid),) + am_v.shape[1:], -1, np.int32)
    out[valid], am[valid] = out_v, am_v
    return out, am


def forward_ref(case, grouped=True, x=None, rois=None):
    """(out fp32, argmax int32) of the oracle; rows with a batch index outside [0, N)
    are 0 / -1.  ``x`` / ``rois``: other features (a widened 16-bit map) or boxes (the
    head's) for the same case -- not cached."""
    key = (case.name, grouped)
    if x is None and rois is None and key in _ref:
        return _ref[key]
    xs = case.inputs()[0] if x is None else x
    rs = case.rois(grouped) if rois is None else rois
    b = rs[:, 0].astype(np.int64)
    valid = (b >= 0) & (b < case.N)
    res = _with_invalid(valid, *orc.roi_pool_forward(xs, rs[valid], case.size, 1.0))
    if x is None and rois is None:
        for a in res:
            a.setflags(write=False)
        _ref[key] = res
    return res


def backward_ref(case, grad=None, argmax=None, rois=None):
    """fp32 grad_in of the oracle (CPU order n -> c -> ph -> pw) for the grouped RoIs."""
    grad = case.grad() if grad is None else grad
    argmax = forward_ref(case)[1] if argmax is None else argmax
    rois = case.rois() if rois is None else rois
    return orc.roi_pool_backward(grad, rois, argmax, case.inputs()[0].shape)


# ------------------------------------------------- what a case must be able to catch
def bin_windows(roi, H, W, PH, PW, ss=1.0):
    """torchvision's bin windows of one RoI, separable: (hs [PH], he [PH], ws [PW], we [PW])."""
    def rnd(v):  # roundf: halves away from zero
        v = float(F32(v) * F32(ss))
        return int(math.copysign(math.floor(abs(v) + 0.5), v))

    sw, sh, ew, eh = rnd(roi[1]), rnd(roi[2]), rnd(roi[3]), rnd(roi[4])
    rw, rh = max(ew - sw + 1, 1), max(eh - sh + 1, 1)
    bh, bw = F32(rh) / F32(PH), F32(rw) / F32(PW)
    ph, pw = np.arange(PH, dtype=F32), np.arange(PW, dtype=F32)
    hs = np.clip(np.floor(ph * bh).astype(np.int64) + sh, 0, H)
    he = np.clip(np.ceil((ph + F32(1)) * bh).astype(np.int64) + sh, 0, H)
    ws = np.clip(np.floor(pw * bw).astype(np.int64) + sw, 0, W)
    we = np.clip(np.ceil((pw + F32(1)) * bw).astype(np.int64) + sw, 0, W)
    return hs, he, ws, we


def first_max_tie(case):
    """(roi, channel, bin) of a bin whose maximum occurs more than once in its window and
    whose oracle argmax is the first occurrence in row-major order, or None.  Every window
    it looks at must agree with the oracle (a check of bin_windows itself)."""
    x, rois, _ = case.inputs()
    out, am = forward_ref(case)
    PH, PW = case.size
    for n in np.nonzero(valid_rows(case))[0]:
        hs, he, ws, we = bin_windows(rois[n], case.H, case.W, PH, PW)
        b = int(rois[n, 0])
        for ph in range(PH):
            for pw in range(PW):
                if he[ph] <= hs[ph] or we[pw] <= ws[pw]:
                    assert (am[n, :, ph, pw] == -1).all() and (out[n, :, ph, pw] == 0).all()
                    continue
                for c in range(min(case.C, 2)):
                    win = x[b, c, hs[ph]:he[ph], ws[pw]:we[pw]]
                    mx = win.max()
                    assert mx == out[n, c, ph, pw], (case.name, n, c, ph, pw)
                    i, j = np.argwhere(win == mx)[0]
                    assert (hs[ph] + i) * case.W + ws[pw] + j == am[n, c, ph, pw]
                    if (win == mx).sum() > 1:
                        return int(n), c, ph * PW + pw
    return None


def bin_stats(case):
    """(empty bins, non-empty bins) over the valid RoIs."""
    am = forward_ref(case)[1][valid_rows(case)]
    return int((am < 0).sum()), int((am >= 0).sum())


def order_sensitive_pixels(case):
    """Pixels of the reference gradient whose bits change when the RoIs are summed in
    reverse order."""
    am = forward_ref(case)[1]
    g, rois = case.grad(), case.rois()
    fwd = backward_ref(case, g, am, rois)
    rev = backward_ref(case, g[::-1], am[::-1], rois[::-1])
    return int((fwd.view(np.uint32) != rev.view(np.uint32)).sum())


def shared_pixels(case):
    """(cross, within): (RoI, channel) argmax pixels shared by bins of two different
    64-bin chunks, and by two bins of one chunk."""
    am = forward_ref(case)[1]
    R, C = am.shape[:2]
    flat = am.reshape(R * C, -1).astype(np.int64)
    chunk = np.arange(flat.shape[1]) // 64
    cross = within = 0
    for row in flat:
        sel = row >= 0
        if not sel.any():
            continue
        pix, ch = row[sel], chunk[sel]
        pairs = np.unique(pix * 64 + ch)          # distinct (pixel, chunk)
        cross += int((np.unique(pairs // 64, return_counts=True)[1] > 1).sum())
        within += int((np.unique(pix * 64 + ch, return_counts=True)[1] > 1).sum())
    return cross, within
