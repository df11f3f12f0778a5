"""The RoIAlign contract (DESIGN.md §3 "RoIAlign") restated in numpy fp32, and the
inputs shared by test_roi_align_cpu.py and test_gpu_roi_align.py.  No GPU.

``forward`` / ``backward`` loop over RoIs, bins and samples in Python and are
vectorised over channels only, so every element sees exactly the contract's
order of operations: each product, sum and quotient below is one fp32
operation on fp32 operands.  Results are compared as bits.

``clip=True`` (the default) narrows each bin's sample indices as the kernels
do -- grids above ``SCAN`` points, which only adaptive sampling produces, by
bisection on the exact fp32 coordinate (nondecreasing in the index there) --
and then applies the exact inside test to each remaining sample; ``clip=False``
walks every sample.  The two must agree bit for bit.
"""
import numpy as np

F = np.float32
MAX_RATIO = 16
SCAN = 16            # kAlignScan
MAX_COORD = F(2 ** 20)
TILE = 8             # kAlignTile: the backward's tile edge
ELEM = {"f32": "ElemF32", "f16": "ElemF16", "bf16": "ElemBF16"}


def fwd_name(dtype):
    return f"roi_align_fwd_kernel<{ELEM[dtype]}>"


def bwd_name(dtype):
    return f"roi_align_bwd_tile_kernel<{ELEM[dtype]}, {TILE}>"


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same_bits(a, b):
    """Bitwise equality, zero's sign included; NaNs compare by position only."""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


class Geom:
    pass


def geometry(roi, N, PH, PW, scale, sampling_ratio, aligned):
    """The contract's per-RoI quantities, or None for a guarded RoI."""
    roi = np.asarray(roi, F)
    scale = F(scale)
    bf = roi[0]
    scaled = [roi[1] * scale, roi[2] * scale, roi[3] * scale, roi[4] * scale]
    if not (bf > F(-1) and bf < F(N)) or not all(abs(v) <= MAX_COORD for v in scaled):   # NaN fails both
        return None
    g = Geom()
    g.b = int(bf)
    off = F(0.5) if aligned else F(0)
    g.sw, g.sh = scaled[0] - off, scaled[1] - off
    ew, eh = scaled[2] - off, scaled[3] - off
    rw, rh = ew - g.sw, eh - g.sh
    if not aligned:
        rw, rh = max(rw, F(1)), max(rh, F(1))
    g.bh, g.bw = rh / F(PH), rw / F(PW)
    g.gh = int(sampling_ratio) if sampling_ratio > 0 else int(np.ceil(rh / F(PH)))
    g.gw = int(sampling_ratio) if sampling_ratio > 0 else int(np.ceil(rw / F(PW)))
    g.count = F(max(g.gh * g.gw, 1))
    return g


def pos(base, b, g, i):
    return base + ((F(i) + F(0.5)) * b) / F(g)


def sample_range(base, b, g, lo, hi, clip):
    """Indices of a bin's samples to visit for the interval [lo, hi]."""
    if g <= 0:
        return range(0)
    if not clip or g <= SCAN:
        return range(g)
    assert b > 0
    lo, hi = F(lo), F(hi)
    l, r = 0, g
    while l < r:
        m = (l + r) // 2
        if pos(base, b, g, m) >= lo:
            r = m
        else:
            l = m + 1
    a, r = l, g
    while l < r:
        m = (l + r) // 2
        if pos(base, b, g, m) <= hi:
            l = m + 1
        else:
            r = m
    return range(a, l)


def axis_table(start, b, g, P, size, clip):
    """Per bin p: the inside samples along one axis, in index order, as (lo, hi, l, h)."""
    table = []
    for p in range(P):
        base = start + F(p) * b
        rows = []
        for i in sample_range(base, b, g, -1, size, clip):
            v = pos(base, b, g, i)
            if v < F(-1) or v > F(size):
                continue
            if v <= 0:
                v = F(0)
            lo = int(v)
            if lo >= size - 1:
                hi = lo = size - 1
                v = F(lo)
            else:
                hi = lo + 1
            l = v - F(lo)
            rows.append((lo, hi, l, F(1) - l))
        table.append(rows)
    return table


def _tables(roi, shape, PH, PW, scale, sampling_ratio, aligned, clip):
    N, _, H, W = shape
    g = geometry(roi, N, PH, PW, scale, sampling_ratio, aligned)
    if g is None:
        return None, None, None
    return g, axis_table(g.sh, g.bh, g.gh, PH, H, clip), axis_table(g.sw, g.bw, g.gw, PW, W, clip)


def _size(output_size):
    return (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)


def forward(x, rois, output_size, spatial_scale=1.0, sampling_ratio=-1, aligned=False, clip=True):
    """out fp32 [R,C,PH,PW]."""
    x = np.ascontiguousarray(x, dtype=F)
    rois = np.asarray(rois, F).reshape(-1, 5)
    PH, PW = _size(output_size)
    C = x.shape[1]
    out = np.zeros((len(rois), C, PH, PW), F)
    with np.errstate(all="ignore"):
        for n, roi in enumerate(rois):
            g, ty, tx = _tables(roi, x.shape, PH, PW, spatial_scale, sampling_ratio, aligned, clip)
            if g is None:
                continue
            v = x[g.b]
            for ph in range(PH):
                for pw in range(PW):
                    acc = np.zeros(C, F)
                    for yl, yh, ly, hy in ty[ph]:
                        for xl, xh, lx, hx in tx[pw]:
                            w1, w2, w3, w4 = hy * hx, hy * lx, ly * hx, ly * lx
                            val = ((w1 * v[:, yl, xl] + w2 * v[:, yl, xh]) + w3 * v[:, yh, xl]) + w4 * v[:, yh, xh]
                            acc = acc + val
                    out[n, :, ph, pw] = acc / g.count
    assert out.dtype == F
    return out


def backward(grad, rois, shape, spatial_scale=1.0, sampling_ratio=-1, aligned=False, clip=True, acc_round=None):
    """grad_in fp32 [N,C,H,W] for grad fp32 [R,C,PH,PW].  ``acc_round``: what the contract
    rules out -- a function applied to the running sum after every addition (a 16-bit
    accumulator), for tests that must tell the two apart."""
    grad = np.ascontiguousarray(grad, dtype=F)
    rois = np.asarray(rois, F).reshape(-1, 5)
    PH, PW = grad.shape[2:]
    gi = np.zeros(tuple(shape), F)
    with np.errstate(all="ignore"):
        for n, roi in enumerate(rois):
            g, ty, tx = _tables(roi, shape, PH, PW, spatial_scale, sampling_ratio, aligned, clip)
            if g is None:
                continue
            t = gi[g.b]
            for ph in range(PH):
                for pw in range(PW):
                    gv = grad[n, :, ph, pw]
                    for yl, yh, ly, hy in ty[ph]:
                        for xl, xh, lx, hx in tx[pw]:
                            for py, px, w in ((yl, xl, hy * hx), (yl, xh, hy * lx), (yh, xl, ly * hx),
                                              (yh, xh, ly * lx)):
                                t[:, py, px] += (gv * w) / g.count
                                if acc_round is not None:
                                    t[:, py, px] = acc_round(t[:, py, px])
    assert gi.dtype == F
    return gi


# ------------------------------------------------------------------- inputs
# inside, tiny, empty, partly and wholly off the map (tests/pool_half_ref.py's list)
SPECIAL_WINDOWS = [(0, 0, 13, 11), (1, 2, 5, 3), (3, 3, 0, 0), (2, 1, 9, 9), (-3, -2, 20, 20),
                   (10, 8, 30, 30), (-20, -20, 5, 5), (4, 1, 1.4, 7)]


def special_rois(N=2, windows=SPECIAL_WINDOWS, scale=1.0):
    """[N * len(windows), 5]; ``scale`` > 1 gives image-space boxes for spatial_scale = 1 / scale."""
    return np.array([[b, x1 * scale, y1 * scale, (x1 + w) * scale, (y1 + h) * scale]
                     for b in range(N) for (x1, y1, w, h) in windows], F)


def special_x_f32(r, N=2, C=16, H=12, W=14):
    """fp32 [N,C,H,W]: random planes plus +-0, +-inf, NaN stripes, subnormals, a ramp."""
    x = r.standard_normal((N, C, H, W)).astype(F)
    x[0, 0] = 0.0
    x[0, 0, ::2, ::3] = -0.0
    x[0, 1] = -0.0
    x[0, 2, 3:6, 3:6] = np.inf
    x[0, 3, ::2] = np.nan
    x[0, 4, 5, :] = -np.inf
    x[0, 5] = (r.integers(0, 1 << 20, (H, W)).astype(np.uint32) | (r.integers(0, 2, (H, W)).astype(np.uint32) << 31)
               ).view(F)                                    # subnormals of either sign, +-0 among them
    x[1, 5] = np.nan
    x[1, 6] = np.round(x[1, 6])
    x[1, 7] = np.arange(H, dtype=F)[:, None] * F(2) + np.arange(W, dtype=F)[None, :] * F(3)
    x[1, 8, 0, 0] = np.inf                                  # inf * 0 at a corner weight
    x[1, 9] = F(3.0e38)                                     # sums overflow to inf
    return x


# (sampling_ratio, aligned, output_size, image scale): the grid of test_gpu_roi_align.py
PARAMS = ([(sr, al, 7, 1.0) for sr in (-1, 2, 3) for al in (False, True)]
          + [(16, False, (3, 5), 1.0), (16, True, (3, 5), 1.0)]
          + [(2, False, (3, 5), 1.0), (-1, True, 1, 1.0), (3, False, 1, 1.0)]
          + [(-1, False, 7, 16.0), (2, True, 7, 16.0)])


class AlignCase:
    """A named shape of the launch plan: the map crosses every tile edge of the backward
    (TILE-pixel tiles, 64-channel groups) where ``H``, ``W`` or ``C`` exceed them."""

    def __init__(self, name, N, C, H, W, size, n_rois, seed, sampling_ratio=2, aligned=False, span=None):
        self.name, self.N, self.C, self.H, self.W, self.size = name, N, C, H, W, _size(size)
        self.n_rois, self.seed, self.sampling_ratio, self.aligned, self.span = n_rois, seed, sampling_ratio, aligned, span

    def __repr__(self):
        return self.name

    def inputs(self):
        r = np.random.default_rng(self.seed)
        x = r.standard_normal((self.N, self.C, self.H, self.W)).astype(F)
        span = self.span or max(self.H, self.W)
        xy = np.stack([r.uniform(-3, self.W + 2, self.n_rois), r.uniform(-3, self.H + 2, self.n_rois)], 1)
        wh = np.stack([r.uniform(0, min(span, self.W + 4), self.n_rois),
                       r.uniform(0, min(span, self.H + 4), self.n_rois)], 1)
        b = r.integers(0, self.N, self.n_rois)
        rois = np.concatenate([b[:, None], xy, xy + wh], 1).astype(F)
        rois[0, 1:] = [0, 0, self.W - 1, self.H - 1]            # the whole map
        rois[1, 1:] = [self.W - 1.5, self.H - 1.5, self.W + 3, self.H + 3]   # the far corner, clamped
        grad = r.standard_normal((self.n_rois, self.C) + self.size).astype(F)
        return x, rois, grad


# one thin map per axis crossing many tile edges, channel counts on both sides of a
# 64-lane group, maps where everything clamps
CASES = [
    AlignCase("wide_3x203", 1, 5, 3, 203, 7, 12, 203, span=40),
    AlignCase("tall_203x3", 1, 5, 203, 3, 7, 12, 302, span=40),
    AlignCase("c1", 2, 1, 12, 14, 7, 10, 1),
    AlignCase("c5_adaptive", 2, 5, 12, 14, (3, 5), 10, 5, sampling_ratio=-1, aligned=True),
    AlignCase("c64", 2, 64, 9, 10, 7, 8, 64),
    AlignCase("c70", 2, 70, 9, 10, 7, 8, 70, sampling_ratio=3),
    AlignCase("map_1x1", 2, 5, 1, 1, 7, 8, 11),
    AlignCase("map_1xW", 2, 5, 1, 19, 7, 8, 119, sampling_ratio=-1),
    AlignCase("map_Hx1", 2, 5, 19, 1, 7, 8, 191, aligned=True),
    AlignCase("tile_edge_16x17", 2, 5, 16, 17, 7, 10, 1617, sampling_ratio=-1),
]
