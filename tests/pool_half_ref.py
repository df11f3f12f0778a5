"""References and inputs for RoIPool in float16 / bfloat16 (DESIGN.md §3 "RoIPool in
16-bit types"), shared by test_pool_half_cpu.py and test_gpu_pool_half.py.  No GPU.

The contract is stated against the fp32 oracle: widen, run the oracle, round once.
Values are compared as bits (``bits()``), argmax with ``array_equal``.
"""
import numpy as np
import torch

from oracle import ref_numpy as orc

DTYPES = [torch.float16, torch.bfloat16]
FLT_MAX = np.float32(3.4028235e38)
# bit pattern of 1.0 and the largest subnormal's bits
_ONE = {torch.float16: 0x3C00, torch.bfloat16: 0x3F80}
_SUB_MAX = {torch.float16: 0x03FF, torch.bfloat16: 0x007F}


def bits(t):
    """int16 view of a 16-bit tensor (on the CPU), for bit-for-bit comparisons."""
    assert t.dtype in DTYPES, t.dtype
    return t.detach().cpu().contiguous().view(torch.int16)


def from_bits(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).view(dtype)


def forward_ref(x, rois, output_size, spatial_scale=1.0):
    """(out of x's dtype, argmax int32 ndarray): the fp32 oracle on x widened,
    its output rounded to nearest even (-FLT_MAX -> -inf)."""
    assert x.dtype in DTYPES, x.dtype
    oo, oa = orc.roi_pool_forward(x.detach().cpu().float().numpy(), np.asarray(rois, np.float32), output_size,
                                  spatial_scale)
    return torch.from_numpy(oo).to(x.dtype), oa


def backward_ref(grad, rois, argmax, shape):
    """grad_in of grad's dtype: the fp32 oracle's sums (order n -> ph -> pw) on grad
    widened, rounded once."""
    assert grad.dtype in DTYPES, grad.dtype
    gi = orc.roi_pool_backward(grad.detach().cpu().float().numpy(), np.asarray(rois, np.float32),
                               np.asarray(argmax, np.int32), tuple(shape))
    return torch.from_numpy(gi).to(grad.dtype)


def backward_accumulated_in_t(grad, rois, argmax, shape):
    """What the contract rules out: the same sums with the running value rounded
    to grad's dtype after every add."""
    dt = grad.dtype
    N, C, H, W = shape
    g = grad.detach().cpu()
    acc = torch.zeros((N, C, H * W), dtype=dt)
    am = np.asarray(argmax)
    R, _, PH, PW = am.shape
    for n in range(R):
        b = int(rois[n][0])
        if not 0 <= b < N:
            continue
        for c in range(C):
            for ph in range(PH):
                for pw in range(PW):
                    a = int(am[n, c, ph, pw])
                    if a >= 0:
                        acc[b, c, a] = (acc[b, c, a].float() + g[n, c, ph, pw].float()).to(dt)
    return acc.view(N, C, H, W)


def special_x(dtype, r, N=2, C=16, H=12, W=14):
    """[N,C,H,W] of `dtype` (CPU): random planes plus the special ones -- signed-zero
    ties, the dtype's most negative finite value, -inf, NaN stripes, a +inf block, an
    all-NaN plane, a column plateau, all -0.0, rounded planes (ties), a ReLU-like plane,
    the dtype's subnormals mixed with zeros, values that differ in the last mantissa
    bit only."""
    assert N >= 2 and C >= 16
    x = torch.from_numpy(r.standard_normal((N, C, H, W)).astype(np.float32)).to(dtype)
    x[0, 0] = 0.0
    x[0, 0, ::2, ::3] = -0.0                        # +-0 ties: first zero's sign wins
    x[0, 1] = torch.finfo(dtype).min                # selected: it is above -FLT_MAX
    x[0, 2] = -np.inf                               # nothing selected: -FLT_MAX -> -inf
    x[0, 3, ::2] = np.nan
    x[0, 4, 3:6, 3:6] = np.inf
    mag = r.integers(0, _SUB_MAX[dtype] + 1, (H, W))
    mag[r.random((H, W)) < 0.3] = 0
    x[0, 5] = from_bits(mag | (r.integers(0, 2, (H, W)) << 15), dtype)   # either sign, -0 included
    assert (x[0, 5].float().abs() < torch.finfo(dtype).tiny).all() and (x[0, 5] != 0).any()
    x[0, 6] = from_bits(_ONE[dtype] + r.integers(0, 2, (H, W)), dtype)   # 1 and 1 + ulp
    x[0, 7] = from_bits(mag, dtype)                 # positive subnormals and +0 only
    x[1, 5] = np.nan
    x[1, 6, :, 5] = 7.0                             # column plateau of equal maxima
    x[1, 7] = -0.0
    x[1, 8:16] = torch.round(x[1, 8:16].float()).to(dtype)
    x[1, 9] = torch.clamp(x[1, 9].float(), min=0.0).to(dtype)   # ReLU: zero maxima, some -0
    x[1, 9, 1::4, ::3] = -0.0
    return x


# the RoIs of test_roi_pool_special_values (tests/test_gpu_parity.py): inside, tiny, empty,
# partly and wholly off the map
SPECIAL_WINDOWS = [(0, 0, 13, 11), (1, 2, 5, 3), (3, 3, 0, 0), (2, 1, 9, 9), (-3, -2, 20, 20),
                   (10, 8, 30, 30), (-20, -20, 5, 5), (4, 1, 1.4, 7)]


def special_rois(N=2, windows=SPECIAL_WINDOWS):
    return np.array([[b, x1, y1, x1 + w, y1 + h] for b in range(N) for (x1, y1, w, h) in windows], np.float32)


# the tiny-RoI list of test_roi_pool_bwd_denormal_and_colliding_grads: 49 bins share a few pixels
def colliding_case(dtype, seed=11):
    """(x [2,6,16,10] of dtype, rois [43,5] ndarray, grad builder) for the case that
    separates one rounding from accumulation in the dtype."""
    r = np.random.default_rng(seed)
    N, C, H, W = 2, 6, 16, 10
    x = torch.from_numpy(r.standard_normal((N, C, H, W)).astype(np.float32)).to(dtype)
    rows = [[0, 2, 2, 2.4, 2.4], [0, 1, 1, 2, 2], [1, 0, 0, 9, 15], [1, 3, 3, 5, 4], [0, 4, 7, 5, 8.4]] * 5
    rows += [[b, *r.uniform(0, 9, 2), *r.uniform(0, 15, 2)] for b in (0, 1) for _ in range(9)]
    rois = np.array(rows, np.float32)

    def grad(shape):
        g = r.standard_normal(tuple(shape)).astype(np.float32)
        tiny = np.float32(torch.finfo(dtype).tiny)
        g = np.where(r.random(g.shape) < 0.3, g * tiny / np.float32(64), g).astype(np.float32)
        g[r.random(g.shape) < 0.05] = -0.0
        gt = torch.from_numpy(g).to(dtype)
        nz = gt.float().abs()[gt != 0]
        assert (nz < torch.finfo(dtype).tiny).any(), "no subnormal gradients"
        return gt

    return x, rois, grad
