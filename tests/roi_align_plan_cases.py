"""The launch plan of RoIAlign (csrc/roi_align.hip) restated in numpy, and the named cases
that pin its branches (DESIGN.md §3 "RoIAlign", "Launch-plan branches and the cases that
pin them").  No GPU.

* ``consts()`` reads the kernels' constants from ``frcnn_roi_align_plan``; ``fwd_plan`` /
  ``bwd_plan`` / ``multi_first`` port the host launch numbers, which the query must repeat.
* ``bwd_path`` ports the backward's per-RoI selector (lane per sample / walk, scan / bisect per
  axis), ``staged`` / ``stage_stride`` / ``pow2_count`` / ``fwd_trim`` the other switches.
* ``cases()``: each names the branch it reaches (``pins``) and building it asserts, with the
  ported selector, that its RoIs reach it.
* ``backward_tiled`` restates the backward structurally in fp32: unit by unit, one flat LDS
  array per workgroup with the kernel's offsets, RoIs in chunks of 64 by ballot, the lane
  path with per-lane sample tables and ballot masks, the walk path with ``align_range``,
  staging, the four additions and the write-out with lane = pixel.  ``forward_threads``
  restates the forward's thread decode.  With no mistake both equal tests/roi_align_ref.py
  bit for bit.
* ``MISTAKES``: structural mistakes the restatements can plant; every case lists in
  ``catches`` those it must tell apart from the reference.

Users: tests/test_roi_align_plan_cases_cpu.py and tests/test_gpu_roi_align_plans.py.
"""
import numpy as np

import roi_align_ref as ref

F = np.float32
U64 = (1 << 64) - 1
_consts = None


class Consts:
    pass


def consts():
    """The kernels' constants, from the library's plan query (one place)."""
    global _consts
    if _consts is None:
        from replication_faster_rcnn_amd import _lib
        p = _lib.roi_align_plan(1, 1, 1, 1, 1, 1, 1)
        k = Consts()
        k.RUN, k.TILE, k.STRIDE, k.WAVES = p["run"], p["tile"], p["stride"], p["waves"]
        k.STAGE_BINS, k.SCAN, k.LANE = p["stage_bins"], p["scan"], p["lane_samples"]
        k.ACC_WORDS = k.TILE * k.TILE * k.STRIDE
        k.WAVE_WORDS = k.ACC_WORDS + 64 * k.STAGE_BINS
        assert k.TILE * k.TILE == 64 and k.SCAN == ref.SCAN and k.TILE == ref.TILE
        _consts = k
    return _consts


# ----------------------------------------------------------------- the host plan
def fwd_plan(R, N, C, H, W, PH, PW):
    k = consts()
    runs = (C + k.RUN - 1) // k.RUN
    total = R * runs * PH * PW if N and H and W else 0
    return dict(fwd_threads=total, fwd_grid=(total + 255) // 256)


def bwd_plan(N, C, H, W, PH, PW):
    """None where the launch refuses the map (2^31 tiles or workgroups)."""
    k = consts()
    tiles_x, tiles_y = (W + k.TILE - 1) // k.TILE, (H + k.TILE - 1) // k.TILE
    cgroups = (C + 63) // 64
    units = tiles_x * tiles_y * cgroups * N
    blocks = (units + k.WAVES - 1) // k.WAVES
    if tiles_x * tiles_y > 0x7fffffff or blocks > 0x7fffffff:
        return None
    return dict(tiles_x=tiles_x, tiles_y=tiles_y, cgroups=cgroups, units=units, blocks=blocks,
                idle=blocks * k.WAVES - units, lds_bytes=4 * k.WAVES * k.WAVE_WORDS, staged=int(staged(PH, PW)))


def plan(R, N, C, H, W, PH, PW):
    """What ``_lib.roi_align_plan`` answers, constants aside."""
    b = bwd_plan(N, C, H, W, PH, PW)
    return None if b is None else dict(fwd_plan(R, N, C, H, W, PH, PW), **b)


def multi_first(sizes, N, C):
    """The pyramid backward's nine unit offsets: level l owns [first[l], first[l + 1])."""
    k = consts()
    first, units = [], 0
    for l in range(9):
        first.append(units)
        if l < len(sizes):
            h, w = sizes[l]
            units += ((w + k.TILE - 1) // k.TILE) * ((h + k.TILE - 1) // k.TILE) * ((C + 63) // 64) * N
    return first


# ------------------------------------------------------------- the selectors
def staged(PH, PW):
    return PH * PW <= consts().STAGE_BINS


def stage_stride(PH, PW):
    return (PH * PW) | 1


def pow2_count(count):
    return (int(np.array([count], F).view(np.uint32)[0]) & 0x7fffff) == 0


def fwd_trim(g):
    return g > consts().SCAN


def axis_mode(g):
    return "scan" if g <= consts().SCAN else "bisect"


def bwd_path(geom, PH, PW):
    """('guarded',) | ('empty',) | ('lane',) | ('walk', y mode, x mode) for one RoI's geometry."""
    L = consts().LANE
    if geom is None:
        return ("guarded",)
    if geom.gh <= 0 or geom.gw <= 0:
        return ("empty",)
    if geom.gh <= L and geom.gw <= L and PH <= L and PW <= L and PH * geom.gh <= L and PW * geom.gw <= L:
        return ("lane",)
    return ("walk", axis_mode(geom.gh), axis_mode(geom.gw))


# ------------------------------------------------------------------ mistakes
MISTAKES = (
    "stage_limit_50", "stage_limit_56",     # staged decided at 50 / 56 bins, the buffer still 49 wide
    "unstaged_reads_stage",                 # grad_at reads the stage although nothing was staged
    "unstaged_no_channel_offset",           # the unstaged pointer lacks the lane's channel
    "stage_read_stride_phw",                # staged with stride PHW | 1, read with stride PHW
    "lane_limit_72",                        # lane path accepted up to 72 samples per axis
    "bits_mask_n64",                        # align_bits: (1 << n) - 1 also at n == 64 (the shift wraps)
    "sample_mask_wraps_at_64",              # ballot cut to PH*gh bits with a shift that wraps at 64
    "hi_incl_dropped",                      # the map's last tile does not take a sample at y == H
    "lower_r0",                             # lower bound r0 instead of r0 - 1
    "chunk_tail_dropped",                   # only whole chunks of 64 RoIs
    "chunks_reversed",                      # chunks walked last to first
    "chunk_lane63_dropped",                 # the ballot loses its top lane
    "tile_div_mod_swapped",                 # r0 from tile % tiles_x, c0 from tile / tiles_x
    "cg_b_swapped",                         # cg = unit / tiles / cgroups, b = (unit / tiles) % cgroups
    "idle_wave_live",                       # a wave past the last unit works and stores
    "recip_non_pow2",                       # x * (1 / count) for every count
    "bisect_lo_off_by_one", "bisect_hi_off_by_one",   # a bisected range one short at its start / end
    "clamped_four_word_arm",                # read-all-then-write although two of the words coincide
    "fwd_runs_c_div_8",                     # forward: runs = C / 8, rounded down
)


# ------------------------------------------------------- pieces of the kernels
def align_range(base, b, g, lo, hi, hi_incl, mistake=None):
    """[a, e) as the kernel's align_range gives it."""
    lo, hi = F(lo), F(hi)

    def below(v):
        return v < hi or (hi_incl and v == hi)

    if g <= consts().SCAN:
        a, e = max(g, 0), 0
        for i in range(g):
            v = ref.pos(base, b, g, i)
            if v >= lo and below(v):
                a, e = min(a, i), i + 1
        return a, e
    l, r = 0, g
    while l < r:
        m = l + (r - l) // 2
        if ref.pos(base, b, g, m) >= lo:
            r = m
        else:
            l = m + 1
    a, r = l, g
    while l < r:
        m = l + (r - l) // 2
        if below(ref.pos(base, b, g, m)):
            l = m + 1
        else:
            r = m
    if mistake == "bisect_lo_off_by_one":
        a += 1
    if mistake == "bisect_hi_off_by_one":
        l -= 1
    return a, l


def align_axis(v, size):
    """(lo, hi, l, h) of an inside coordinate."""
    if v <= 0:
        v = F(0)
    lo = int(v)
    if lo >= size - 1:
        hi = lo = size - 1
        v = F(lo)
    else:
        hi = lo + 1
    l = v - F(lo)
    return lo, hi, l, F(1) - l


def align_bits(m, first, n, mistake=None):
    s = (m >> first) if first < 64 else 0      # a shift of 64 or more: nothing is left
    if n >= 64 and mistake != "bits_mask_n64":
        return s
    return s & (((1 << (n % 64)) - 1) & U64)


def ctz(m):
    return (m & -m).bit_length() - 1


class Tiled:
    """What ``backward_tiled`` returns: grad_in with the guard behind it, how often each word
    was stored, and the stores that went past the guard."""

    def __init__(self, shape, guard):
        self.shape = tuple(shape)
        self.n = int(np.prod(shape))
        self.flat = np.full(self.n + guard, np.nan, F)
        self.flat[self.n:] = GUARD_VALUE
        self.stores = np.zeros(self.n + guard, np.int64)
        self.lost = 0
        self.max_stage_word = -1

    @property
    def grad_in(self):
        return self.flat[:self.n].reshape(self.shape)

    def equals(self, want):
        """Bit for bit the reference, every word stored exactly once, nothing else touched."""
        return bool(self.lost == 0 and (self.stores[:self.n] == 1).all() and not self.stores[self.n:].any()
                    and ref.same_bits(self.grad_in, want))


GUARD_VALUE = F(-77.0)


def backward_tiled(grad, rois, shape, spatial_scale=1.0, sampling_ratio=-1, aligned=False, mistake=None, guard=None):
    """roi_align_bwd_tile_kernel restated: returns a ``Tiled``."""
    k = consts()
    T, S = k.TILE, k.STRIDE
    grad = np.ascontiguousarray(grad, dtype=F)
    rois = np.asarray(rois, F).reshape(-1, 5)
    N, C, H, W = shape
    R, _, PH, PW = grad.shape
    PHW = PH * PW
    gflat = np.concatenate([grad.ravel(), np.zeros(64 * PHW + 64, F)])    # a read past the end: zeros
    p = bwd_plan(N, C, H, W, PH, PW)
    tiles_x, tiles, cgroups, units = p["tiles_x"], p["tiles_x"] * p["tiles_y"], p["cgroups"], p["units"]
    res = Tiled(shape, min(5 * C * H * W, 1 << 16) if guard is None else guard)
    lanes = np.arange(64)
    limit = {"stage_limit_50": 50, "stage_limit_56": 56}.get(mistake, k.STAGE_BINS)
    is_staged = PHW <= limit
    sstride = PHW | 1
    rstride = PHW if mistake == "stage_read_stride_phw" else sstride
    lane_limit = 72 if mistake == "lane_limit_72" else k.LANE
    geoms = [ref.geometry(r, N, PH, PW, spatial_scale, sampling_ratio, aligned) for r in rois]
    fH, fW = F(H), F(W)

    def add4(lds, al, ah, ol, oh, in_yl, in_yh, in_xl, in_xh, four, gv, w, pow2, inv, count):
        if pow2 or mistake == "recip_non_pow2":
            q = [(gv * wi) * inv for wi in w]
        else:
            q = [(gv * wi) / count for wi in w]
        if in_yl and in_yh and in_xl and in_xh and (four or mistake == "clamped_four_word_arm"):
            s = [lds[al + ol + lanes], lds[al + oh + lanes], lds[ah + ol + lanes], lds[ah + oh + lanes]]
            lds[al + ol + lanes] = s[0] + q[0]
            lds[al + oh + lanes] = s[1] + q[1]
            lds[ah + ol + lanes] = s[2] + q[2]
            lds[ah + oh + lanes] = s[3] + q[3]
        else:
            if in_yl and in_xl:
                lds[al + ol + lanes] = lds[al + ol + lanes] + q[0]
            if in_yl and in_xh:
                lds[al + oh + lanes] = lds[al + oh + lanes] + q[1]
            if in_yh and in_xl:
                lds[ah + ol + lanes] = lds[ah + ol + lanes] + q[2]
            if in_yh and in_xh:
                lds[ah + oh + lanes] = lds[ah + oh + lanes] + q[3]

    with np.errstate(all="ignore"):
        for block in range(p["blocks"]):
            lds = np.zeros(2 * k.WAVES * k.WAVE_WORDS, F)      # unwritten words read as 0; slack for stray offsets
            decoded = []
            for wid in range(k.WAVES):                         # every wave zeroes its sums first
                unit = block * k.WAVES + wid
                acc = wid * k.WAVE_WORDS
                for px in range(T * T):
                    lds[acc + px * S + lanes] = 0
                decoded.append((unit, acc, unit < units or mistake == "idle_wave_live"))
            for unit, acc, live in decoded:
                if not live or tiles == 0 or cgroups == 0:
                    continue
                stage = acc + k.ACC_WORDS
                tile = unit % tiles
                cg, b = (unit // tiles) % cgroups, unit // tiles // cgroups
                if mistake == "cg_b_swapped":
                    cg, b = b, cg
                ty_, tx_ = tile // tiles_x, tile % tiles_x
                if mistake == "tile_div_mod_swapped":
                    ty_, tx_ = tx_, ty_
                r0, c0 = ty_ * T, tx_ * T
                r1, c1 = min(r0 + T, H), min(c0 + T, W)
                c = cg * 64 + lanes
                active = c < C
                ylo, yhi, xlo, xhi = F(r0 - 1), F(r1), F(c0 - 1), F(c1)
                if mistake == "lower_r0":
                    ylo, xlo = F(r0), F(c0)
                yincl, xincl = r1 == H, c1 == W
                if mistake == "hi_incl_dropped":
                    yincl = xincl = False
                nch = min(C - cg * 64, 64)
                chunks = list(range(0, R, 64))
                if mistake == "chunk_tail_dropped":
                    chunks = [rb for rb in chunks if rb + 64 <= R]
                if mistake == "chunks_reversed":
                    chunks.reverse()
                for rbase in chunks:
                    mask = 0
                    for lane in range(64):
                        r = rbase + lane
                        if r < R and geoms[r] is not None and geoms[r].b == b:
                            mask |= 1 << lane
                    if mistake == "chunk_lane63_dropped":
                        mask &= (1 << 63) - 1
                    while mask:
                        j = ctz(mask)
                        mask &= mask - 1
                        n = rbase + j
                        g = geoms[n]
                        pow2 = pow2_count(g.count)
                        inv = F(1) / g.count
                        coff = np.where(active, c, 0)
                        if mistake == "unstaged_no_channel_offset":
                            coff = np.zeros(64, np.int64)
                        gp = (n * C + coff) * PHW

                        def stage_in():
                            if not is_staged:
                                return
                            src = (n * C + cg * 64) * PHW
                            i = np.arange(max(nch * PHW, 0))
                            ch = i // PHW
                            idx = ch * sstride + (i - ch * PHW)
                            lds[stage + idx] = gflat[src + i]
                            if len(idx):
                                res.max_stage_word = max(res.max_stage_word, int(idx.max()))

                        def grad_at(ph, pw):
                            if is_staged or mistake == "unstaged_reads_stage":
                                v = lds[stage + lanes * rstride + ph * PW + pw]
                            else:
                                v = gflat[gp + ph * PW + pw]
                            return np.where(active, v, F(0)).astype(F)

                        if (g.gh > 0 and g.gw > 0 and g.gh <= lane_limit and g.gw <= lane_limit and PH <= lane_limit
                                and PW <= lane_limit and PH * g.gh <= lane_limit and PW * g.gw <= lane_limit):
                            taby, tabx = [None] * 64, [None] * 64       # per lane: one sample of each axis
                            ymask = xmask = 0
                            for lane in range(64):
                                if lane < PH * g.gh:
                                    pb = lane // g.gh
                                    y = ref.pos(g.sh + F(pb) * g.bh, g.bh, g.gh, lane - pb * g.gh)
                                    if not (y < F(-1) or y > fH):
                                        taby[lane] = t = align_axis(y, H)
                                        if r0 <= t[0] < r1 or r0 <= t[1] < r1:
                                            ymask |= 1 << lane
                                if lane < PW * g.gw:
                                    pb = lane // g.gw
                                    x = ref.pos(g.sw + F(pb) * g.bw, g.bw, g.gw, lane - pb * g.gw)
                                    if not (x < F(-1) or x > fW):
                                        tabx[lane] = t = align_axis(x, W)
                                        if c0 <= t[0] < c1 or c0 <= t[1] < c1:
                                            xmask |= 1 << lane
                            if mistake == "sample_mask_wraps_at_64":
                                ymask &= (1 << ((PH * g.gh) % 64)) - 1
                                xmask &= (1 << ((PW * g.gw) % 64)) - 1
                            if not ymask or not xmask:
                                continue
                            pha, phe = ctz(ymask) // g.gh, (ymask.bit_length() - 1) // g.gh + 1
                            pwa, pwe = ctz(xmask) // g.gw, (xmask.bit_length() - 1) // g.gw + 1
                            stage_in()
                            for ph in range(pha, phe):
                                by = align_bits(ymask, ph * g.gh, g.gh, mistake)
                                if not by:
                                    continue
                                for pw in range(pwa, pwe):
                                    bx = align_bits(xmask, pw * g.gw, g.gw, mistake)
                                    if not bx:
                                        continue
                                    gv = grad_at(ph, pw)
                                    my = by
                                    while my:
                                        yl, yh, ly, hy = taby[ph * g.gh + ctz(my)]
                                        my &= my - 1
                                        in_yl, in_yh = r0 <= yl < r1, r0 <= yh < r1
                                        al, ah = acc + (yl - r0) * T * S, acc + (yh - r0) * T * S
                                        mx = bx
                                        while mx:
                                            xl, xh, lx, hx = tabx[pw * g.gw + ctz(mx)]
                                            mx &= mx - 1
                                            in_xl, in_xh = c0 <= xl < c1, c0 <= xh < c1
                                            add4(lds, al, ah, (xl - c0) * S, (xh - c0) * S, in_yl, in_yh, in_xl, in_xh,
                                                 yl != yh and xl != xh, gv, (hy * hx, hy * lx, ly * hx, ly * lx),
                                                 pow2, inv, g.count)
                            continue
                        # the walk: bins, then each bin's samples, narrowed to the tile
                        pha, phe, pwa, pwe = PH, 0, PW, 0
                        for ph in range(PH):
                            a, e = align_range(g.sh + F(ph) * g.bh, g.bh, g.gh, ylo, yhi, yincl, mistake)
                            if a < e:
                                pha, phe = min(pha, ph), ph + 1
                        if pha >= phe:
                            continue
                        for pw in range(PW):
                            a, e = align_range(g.sw + F(pw) * g.bw, g.bw, g.gw, xlo, xhi, xincl, mistake)
                            if a < e:
                                pwa, pwe = min(pwa, pw), pw + 1
                        if pwa >= pwe:
                            continue
                        stage_in()
                        for ph in range(pha, phe):
                            basey = g.sh + F(ph) * g.bh
                            ya, ye = align_range(basey, g.bh, g.gh, ylo, yhi, yincl, mistake)
                            if ya >= ye:
                                continue
                            for pw in range(pwa, pwe):
                                basex = g.sw + F(pw) * g.bw
                                xa, xe = align_range(basex, g.bw, g.gw, xlo, xhi, xincl, mistake)
                                if xa >= xe:
                                    continue
                                gv = grad_at(ph, pw)
                                for iy in range(ya, ye):
                                    y = ref.pos(basey, g.bh, g.gh, iy)
                                    if y < F(-1) or y > fH:
                                        continue
                                    yl, yh, ly, hy = align_axis(y, H)
                                    in_yl, in_yh = r0 <= yl < r1, r0 <= yh < r1
                                    if not in_yl and not in_yh:
                                        continue
                                    al, ah = acc + (yl - r0) * T * S, acc + (yh - r0) * T * S
                                    for ix in range(xa, xe):
                                        x = ref.pos(basex, g.bw, g.gw, ix)
                                        if x < F(-1) or x > fW:
                                            continue
                                        xl, xh, lx, hx = align_axis(x, W)
                                        in_xl, in_xh = c0 <= xl < c1, c0 <= xh < c1
                                        if not in_xl and not in_xh:
                                            continue
                                        add4(lds, al, ah, (xl - c0) * S, (xh - c0) * S, in_yl, in_yh, in_xl, in_xh,
                                             yl != yh and xl != xh, gv, (hy * hx, hy * lx, ly * hx, ly * lx), pow2,
                                             inv, g.count)
                # the barrier is behind every wave of the loop above; then lane = pixel
            for unit, acc, live in decoded:
                if not live or tiles == 0 or cgroups == 0:
                    continue
                tile = unit % tiles
                cg, b = (unit // tiles) % cgroups, unit // tiles // cgroups
                if mistake == "cg_b_swapped":
                    cg, b = b, cg
                ty_, tx_ = tile // tiles_x, tile % tiles_x
                if mistake == "tile_div_mod_swapped":
                    ty_, tx_ = tx_, ty_
                r0, c0 = ty_ * T, tx_ * T
                r1, c1 = min(r0 + T, H), min(c0 + T, W)
                nc = min(C - cg * 64, 64)
                for lane in range(64):
                    py, px = lane // T, lane % T
                    if r0 + py < r1 and c0 + px < c1 and nc > 0:
                        dst = (b * C + cg * 64) * H * W + (r0 + py) * W + (c0 + px) + np.arange(nc) * H * W
                        val = lds[acc + lane * S + np.arange(nc)]
                        ok = dst < len(res.flat)
                        res.lost += int((~ok).sum())
                        res.flat[dst[ok]] = val[ok]
                        np.add.at(res.stores, dst[ok], 1)
    return res


def forward_threads(x, rois, output_size, spatial_scale=1.0, sampling_ratio=-1, aligned=False, mistake=None):
    """roi_align_fwd_kernel restated thread by thread: the grid of 256, the decode of (n, run,
    ph, pw), the last run's channel tail, the trimmed sample ranges.  Returns (out, stores);
    an output no thread stores stays NaN with stores == 0."""
    k = consts()
    x = np.ascontiguousarray(x, dtype=F)
    rois = np.asarray(rois, F).reshape(-1, 5)
    N, C, H, W = x.shape
    PH, PW = ref._size(output_size)
    R = len(rois)
    runs = C // k.RUN if mistake == "fwd_runs_c_div_8" else (C + k.RUN - 1) // k.RUN
    total = R * runs * PH * PW
    grid = (total + 255) // 256
    out = np.full((R, C, PH, PW), np.nan, F)
    stores = np.zeros(out.shape, np.int64)
    fH, fW = F(H), F(W)
    geoms = {}
    with np.errstate(all="ignore"):
        for idx in range(grid * 256):
            if idx >= total:
                continue
            pw, ph = idx % PW, (idx // PW) % PH
            c0 = ((idx // PW // PH) % runs) * k.RUN
            n = idx // PW // PH // runs
            nc = min(C - c0, k.RUN)
            if n not in geoms:
                geoms[n] = ref.geometry(rois[n], N, PH, PW, spatial_scale, sampling_ratio, aligned)
            g = geoms[n]
            stores[n, c0:c0 + nc, ph, pw] += 1
            if g is None:
                out[n, c0:c0 + nc, ph, pw] = 0
                continue
            v = x[g.b, c0:c0 + nc]
            basey, basex = g.sh + F(ph) * g.bh, g.sw + F(pw) * g.bw
            ya, ye, xa, xe = 0, g.gh, 0, g.gw
            if fwd_trim(g.gh):
                ya, ye = align_range(basey, g.bh, g.gh, -1, fH, True)
            if fwd_trim(g.gw):
                xa, xe = align_range(basex, g.bw, g.gw, -1, fW, True)
            acc = np.zeros(nc, F)
            for iy in range(ya, ye):
                y = ref.pos(basey, g.bh, g.gh, iy)
                if y < F(-1) or y > fH:
                    continue
                yl, yh, ly, hy = align_axis(y, H)
                for ix in range(xa, xe):
                    xx = ref.pos(basex, g.bw, g.gw, ix)
                    if xx < F(-1) or xx > fW:
                        continue
                    xl, xh, lx, hx = align_axis(xx, W)
                    w1, w2, w3, w4 = hy * hx, hy * lx, ly * hx, ly * lx
                    acc = acc + (((w1 * v[:, yl, xl] + w2 * v[:, yl, xh]) + w3 * v[:, yh, xl]) + w4 * v[:, yh, xh])
            out[n, c0:c0 + nc, ph, pw] = acc / g.count
    return out, stores


def forward_equals(got, want):
    out, stores = got
    return bool((stores == 1).all() and ref.same_bits(out, want))


# --------------------------------------------------------------------- cases
def random_rois(r, n, N, H, W):
    """AlignCase's boxes: anywhere over the map and a little past it, images interleaved; the
    first two are the whole map and the far corner, where every sample clamps."""
    xy = np.stack([r.uniform(-3, W + 2, n), r.uniform(-3, H + 2, n)], 1)
    wh = np.stack([r.uniform(0, min(max(H, W), W + 4), n), r.uniform(0, min(max(H, W), H + 4), n)], 1)
    b = np.arange(n) % N
    rois = np.concatenate([b[:, None], xy, xy + wh], 1).astype(F)
    rois[0, 1:] = [0, 0, W - 1, H - 1]
    rois[1, 1:] = [W - 1.5, H - 1.5, W + 3, H + 3]
    return rois


def overlapping_rois(r, n, N):
    """Boxes that all cover the pixels around (4, 4) of a 9 x 9 map, images interleaved."""
    lo = r.uniform(1.5, 3.5, (n, 2))
    hi = r.uniform(4.5, 7.5, (n, 2))
    return np.concatenate([(np.arange(n) % N)[:, None], lo, hi], 1).astype(F)


class PlanCase:
    """``pins``: what every live RoI's path must be (``path``), the staging switch, whether the
    sample count is a power of two, and launch numbers of the plan, by name."""

    def __init__(self, name, N, C, HW, size, sr, rois, pins, catches, aligned=False, half=False, note=""):
        self.name, self.N, self.C, (self.H, self.W), self.size = name, N, C, HW, ref._size(size)
        self.sampling_ratio, self.aligned, self.half, self.note = sr, aligned, half, note
        self.pins, self.catches = pins, tuple(catches)
        self.shape = (N, C, self.H, self.W)
        r = np.random.default_rng(sum(map(ord, name)))
        self.rois = np.asarray(rois(r) if callable(rois) else rois, F).reshape(-1, 5)
        self.R = len(self.rois)
        self.check()

    def __repr__(self):
        return self.name

    def geoms(self):
        return [ref.geometry(q, self.N, *self.size, 1.0, self.sampling_ratio, self.aligned) for q in self.rois]

    def paths(self):
        return [bwd_path(g, *self.size) for g in self.geoms()]

    def plan(self):
        return plan(self.R, self.N, self.C, self.H, self.W, *self.size)

    def check(self):
        """The case reaches what it names, by the ported selector; loud if a constant moved."""
        assert set(self.catches) <= set(MISTAKES), self.name
        pins, paths, p = self.pins, self.paths(), self.plan()
        if "paths" in pins:                  # the set of paths the RoIs take, exactly
            assert set(paths) == set(pins["paths"]), (self.name, sorted(set(paths)))
        if "staged" in pins:
            assert staged(*self.size) == pins["staged"] == bool(p["staged"]), self.name
        if "stride" in pins:
            assert stage_stride(*self.size) == pins["stride"], self.name
        if "pow2" in pins:
            assert {pow2_count(g.count) for g in self.geoms() if g is not None} == {pins["pow2"]}, self.name
        if "grids" in pins:
            assert [(g.gh, g.gw) for g in self.geoms()] == pins["grids"], (self.name,
                                                                          [(g.gh, g.gw) for g in self.geoms()])
        for key in ("tiles_x", "tiles_y", "cgroups", "units", "blocks", "idle", "fwd_threads", "fwd_grid"):
            if key in pins:
                assert p[key] == pins[key], (self.name, key, p[key])
        if "samples" in pins:                # PH * gh and PW * gw of every RoI
            assert {(self.size[0] * g.gh, self.size[1] * g.gw) for g in self.geoms()} == {pins["samples"]}, self.name

    def inputs(self):
        """x fp32 [N,C,H,W], rois, grad fp32 [R,C,PH,PW]."""
        r = np.random.default_rng(sum(map(ord, self.name)) + 1)
        x = r.standard_normal(self.shape).astype(F)
        grad = r.standard_normal((self.R, self.C) + self.size).astype(F)
        return x, self.rois, grad


LANE, WALK_SS = ("lane",), ("walk", "scan", "scan")


def _edge_rois(r):
    """Dyadic boxes on a 17 x 18 map, output 2 x 2, adaptive: a 128-px side gives a grid of 64
    points a pixel apart (bisected), an 8-px side one of 4 (scanned).  Samples fall exactly at
    -1, on the interior tile edges 8 and 16, and at y == 17 == H, x == 18 == W."""
    return [[0, -3.5, -3.5, 124.5, 124.5],      # both axes bisected: samples at -3 .. 124, all integers
            [0, -3.5, 9.5, 124.5, 17.5],        # y scanned: samples at 10 .. 17 (y == H)
            [0, -3.5, -1.5, 124.5, 6.5],        # y scanned: -1 .. 6
            [0, -3.5, 4.5, 124.5, 12.5],        # y scanned: 5 .. 12, over the tile edge 8
            [0, 10.5, -3.5, 18.5, 124.5],       # x scanned: 11 .. 18 (x == W)
            [0, -1.5, -3.5, 6.5, 124.5]]        # x scanned: -1 .. 6


def edge_positions(case):
    """The exact sample coordinates of sample_on_edge's RoIs along (y, x)."""
    ys, xs = set(), set()
    for g in case.geoms():
        for p_ in range(case.size[0]):
            ys |= {float(ref.pos(g.sh + F(p_) * g.bh, g.bh, g.gh, i)) for i in range(g.gh)}
        for p_ in range(case.size[1]):
            xs |= {float(ref.pos(g.sw + F(p_) * g.bw, g.bw, g.gw, i)) for i in range(g.gw)}
    return ys, xs


def _build():
    rr = random_rois
    cases = [
        PlanCase("out14_unstaged", 2, 5, (17, 18), 14, 2, lambda r: rr(r, 6, 2, 17, 18),
                 dict(paths=[LANE], staged=False, pow2=True),
                 ["unstaged_reads_stage", "unstaged_no_channel_offset", "clamped_four_word_arm"], half=True),
        PlanCase("out5x10_first_unstaged", 2, 64, (17, 18), (5, 10), 2, lambda r: rr(r, 6, 2, 17, 18),
                 dict(paths=[LANE], staged=False, cgroups=1),
                 ["stage_limit_50", "stage_limit_56", "unstaged_reads_stage"],
                 note="64 channels: a stage of 50 bins overruns the 49-bin buffer only from channel 62 on"),
        PlanCase("stage48_full", 1, 64, (9, 17), (6, 8), 3, lambda r: rr(r, 6, 1, 9, 17),
                 dict(paths=[LANE], staged=True, stride=49, cgroups=1), ["stage_read_stride_phw"], aligned=True,
                 half=True),
        PlanCase("stage_even_small", 3, 70, (9, 17), 2, 2, lambda r: rr(r, 9, 3, 9, 17),
                 dict(paths=[LANE], staged=True, stride=5, tiles_x=3, tiles_y=2, cgroups=2, units=36, idle=4),
                 ["stage_read_stride_phw", "tile_div_mod_swapped", "cg_b_swapped"], half=True,
                 note="three images: with N == cgroups a swap of cg and b only permutes the units"),
        PlanCase("lane64_exact", 1, 3, (17, 18), 8, 8, lambda r: rr(r, 4, 1, 17, 18),
                 dict(paths=[LANE], samples=(64, 64), staged=False), ["sample_mask_wraps_at_64"]),
        PlanCase("walk72_unstaged", 1, 3, (17, 18), (9, 8), 8, lambda r: rr(r, 4, 1, 17, 18),
                 dict(paths=[WALK_SS], samples=(72, 64), staged=False, pow2=True),
                 ["lane_limit_72", "unstaged_reads_stage", "lower_r0"], half=True),
        PlanCase("sr10_divide", 2, 3, (17, 18), 7, 10, lambda r: rr(r, 5, 2, 17, 18),
                 dict(paths=[WALK_SS], staged=True, pow2=False), ["recip_non_pow2", "lower_r0"]),
        PlanCase("pw65", 1, 3, (9, 18), (1, 65), 1, lambda r: rr(r, 5, 1, 9, 18),
                 dict(paths=[WALK_SS], samples=(1, 65), staged=False), ["lane_limit_72", "unstaged_reads_stage"]),
        PlanCase("adaptive_g64_g65", 1, 3, (70, 9), 1, -1, [[0, 1, 2, 6, 66], [0, 2, 3, 7.5, 68]],
                 dict(paths=[LANE, ("walk", "bisect", "scan")], grids=[(64, 5), (65, 6)], staged=True),
                 ["bits_mask_n64", "sample_mask_wraps_at_64", "bisect_lo_off_by_one", "bisect_hi_off_by_one"]),
        PlanCase("adaptive_mixed", 1, 3, (20, 22), 7, -1,
                 [[0, 2, -10, 142, 60], [0, -10, 2, 60, 142.5], [0, -300, -300, 320, 330]],
                 dict(paths=[("walk", "scan", "bisect"), ("walk", "bisect", "scan"), ("walk", "bisect", "bisect")],
                      grids=[(10, 20), (21, 10), (90, 89)]),
                 ["bisect_lo_off_by_one", "bisect_hi_off_by_one", "lower_r0"]),
        PlanCase("sample_on_edge", 1, 2, (17, 18), 2, -1, _edge_rois,
                 dict(paths=[("walk", "bisect", "bisect"), ("walk", "scan", "bisect"), ("walk", "bisect", "scan")],
                      grids=[(64, 64)] + [(4, 64)] * 3 + [(64, 4)] * 2, pow2=True),
                 ["hi_incl_dropped", "lower_r0", "bisect_lo_off_by_one", "bisect_hi_off_by_one"]),
        PlanCase("r64", 2, 1, (9, 9), 2, 2, lambda r: overlapping_rois(r, 64, 2), dict(paths=[LANE], units=8, idle=2),
                 ["chunk_lane63_dropped"]),
        PlanCase("r65", 2, 1, (9, 9), 2, 2, lambda r: overlapping_rois(r, 65, 2), dict(paths=[LANE], units=8, idle=2),
                 ["chunk_tail_dropped", "chunks_reversed"]),
        PlanCase("r129", 2, 1, (9, 9), 2, 2, lambda r: overlapping_rois(r, 129, 2), dict(paths=[LANE], units=8, idle=2),
                 ["chunk_tail_dropped", "chunks_reversed", "chunk_lane63_dropped"]),
        PlanCase("units_1", 1, 1, (8, 8), 2, 2, lambda r: rr(r, 4, 1, 8, 8), dict(units=1, blocks=1, idle=4),
                 ["idle_wave_live"]),
        PlanCase("units_6", 2, 1, (8, 24), 2, 2, lambda r: rr(r, 5, 2, 8, 24), dict(units=6, blocks=2, idle=4),
                 ["idle_wave_live"]),
        PlanCase("fwd_decode", 2, 9, (5, 6), (3, 5), 2, lambda r: rr(r, 7, 2, 5, 6),
                 dict(fwd_threads=210, fwd_grid=1), ["fwd_runs_c_div_8"]),
    ]
    return cases


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = _build()
    return _cases


def case(name):
    return next(c for c in cases() if c.name == name)


# existing tests/roi_align_ref.py cases that are the catcher of a mistake: (case name, mistake)
REF_CATCHERS = (("map_1x1", "clamped_four_word_arm"),)

# the pyramids of tests/test_gpu_roi_align_plans.py: level sizes, N, C
STRADDLE = dict(sizes=[(17, 18), (9, 9), (5, 5)], N=2, C=5, first=[0, 18, 26], units=28)
EMPTY_MIDDLE = dict(sizes=[(9, 10), (0, 0), (3, 3)], N=2, C=5)
