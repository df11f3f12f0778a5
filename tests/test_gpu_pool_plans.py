"""RoIPool at every launch-plan branch of tests/pool_plan_cases.py (DESIGN.md §3
"Launch-plan branches") vs the oracle.  Needs an MI355X.

Every test first asserts that the library's name query answers the kernel the case is
for (the host's plan restated over the source's constants at this device's CU count),
so a case that a changed threshold moved elsewhere fails instead of covering nothing.
Values are compared as bits and argmax with array_equal; there is no tolerance."""
import numpy as np
import pytest
import torch

import pool_half_ref as phr
import pool_plan_cases as ppc
from oracle import ref_numpy as orc
from pool_plan_cases import BWD_CASES, CASES
from replication_faster_rcnn_amd import _lib, heads, ops
from replication_faster_rcnn_amd.ops import _roi_pool_bwd

pytestmark = pytest.mark.gpu
DEV = "cuda"
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def pairs(cases):
    return pytest.mark.parametrize("case,dt", [(c, d) for c in cases for d in c.dtypes],
                                   ids=lambda v: v if isinstance(v, str) else v.name)


GROUPED = pytest.mark.parametrize("grouped", [True, False], ids=["grouped", "ungrouped"])


def dev(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV)


def features(case, dt):
    """The case's feature map in the run's dtype (CPU)."""
    return torch.from_numpy(case.inputs()[0]).to(TORCH[dt])


def same_bits(got, want):
    """got: device / CPU tensor; want: tensor or ndarray of the same dtype."""
    want = want if isinstance(want, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(want))
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype == torch.float32:
        return torch.equal(got.detach().cpu().view(torch.int32), want.view(torch.int32))
    return torch.equal(phr.bits(got), phr.bits(want))


_fwd = {}


def forward_ref(case, dt, grouped=True, rois=None):
    """(out tensor of the run's dtype, argmax ndarray): orc.roi_pool_forward for fp32,
    pool_half_ref.forward_ref for the 16-bit types, on the rows with a batch index in
    [0, N); the other rows 0 / -1.  Computed once per (case, dtype, order)."""
    key = (case.name, dt, grouped)
    if rois is None and key in _fwd:
        return _fwd[key]
    if dt == "f32":
        out, am = ppc.forward_ref(case, grouped, rois=rois)
        res = (torch.from_numpy(out.copy()), am)     # (the table's arrays are read-only)
    else:
        rs = case.rois(grouped) if rois is None else rois
        b = rs[:, 0].astype(np.int64)
        valid = (b >= 0) & (b < case.N)
        ov, av = phr.forward_ref(features(case, dt), rs[valid], case.size)
        out = torch.zeros((len(rs),) + tuple(ov.shape[1:]), dtype=ov.dtype)
        am = np.full((len(rs),) + av.shape[1:], -1, np.int32)
        out[torch.from_numpy(valid)], am[valid] = ov, av
        res = (out, am)
    if rois is None:
        _fwd[key] = res
    return res


def backward_ref(case, dt, grad, rois, argmax):
    if dt == "f32":
        return torch.from_numpy(ppc.backward_ref(case, grad.numpy(), argmax, rois))
    return phr.backward_ref(grad, rois, argmax, case.inputs()[0].shape)


def assert_fwd_name(case, dt, grouped, head=False):
    want = ppc.fwd_name(dt, case.N, case.C, case.H, case.W, *case.size, grouped, head=head)
    assert ppc.fwd_plan(case.N, case.C, case.H, case.W, *case.size, grouped) == case.fwd[0 if grouped else 1]
    got = _lib.roi_pool_fwd_kernel(case.R, case.N, case.C, case.H, case.W, *case.size, rois_sorted=grouped,
                                   head=head, dtype=TORCH[dt])
    assert got == want, (got, want)


# ------------------------------------------------------------------- forward
@GROUPED
@pairs(CASES)
def test_forward(case, dt, grouped):
    assert_fwd_name(case, dt, grouped)
    out, am = ops.roi_pool_with_argmax(dev(features(case, dt)), dev(case.rois(grouped)), case.size, 1.0,
                                       rois_sorted=grouped)
    ro, ra = forward_ref(case, dt, grouped)
    assert am.dtype == torch.int32 and np.array_equal(am.cpu().numpy(), ra)
    assert same_bits(out, ro)


@GROUPED
@pairs([c for c in CASES if c.head])
def test_forward_through_roi_pool_head(case, dt, grouped):
    """Above 64 bins roi_pool_head runs roi_transform and then the plain forward: boxes,
    out and argmax as the oracle's transform + pool give them."""
    assert_fwd_name(case, dt, grouped, head=True)
    r4, inds, img_h, img_w = case.head_inputs()
    if not grouped:
        perm = case.inputs()[2]
        r4, inds = r4[perm], inds[perm]
    out, am, boxes = ops.roi_pool_head(dev(features(case, dt)), dev(r4), dev(inds), case.size, img_h, img_w,
                                       rois_sorted=grouped)
    oboxes = orc.roi_transform(r4, inds, img_h, img_w, case.H, case.W)
    assert boxes.dtype == torch.float32 and same_bits(boxes, oboxes)
    ro, ra = forward_ref(case, dt, grouped, rois=oboxes)
    assert np.array_equal(am.cpu().numpy(), ra) and same_bits(out, ro)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_resnet_head_14x14(dt):
    """heads.ResnetHead with roi_size 14: the classifier sees the oracle's pooled tensor,
    and features.grad is the backward of the gradient that reached it."""
    case = ppc.BY_NAME["bins_14x14"]
    r4, inds, img_h, img_w = case.head_inputs()
    n = len(r4) - len(r4) % case.N          # the head views its outputs as [N, R / N, ...]
    r4, inds = r4[:n], inds[:n]
    torch.manual_seed(0)
    classifier = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(case.C * 196, 512))
    head = heads.ResnetHead(classifier, roi_size=14, n_classes=5).to(DEV)
    seen = {}

    def pre_hook(_mod, inp):
        seen["cropped"] = inp[0].detach().clone()
        inp[0].register_hook(lambda g: seen.__setitem__("grad", g.detach().clone()))

    head.classifier.register_forward_pre_hook(pre_hook)
    feats = dev(features(case, dt)).requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt != "f32"):
        cls, reg = head(feats, torch.from_numpy(r4), torch.from_numpy(inds), img_h, img_w, rois_sorted=True)
    assert cls.shape == (case.N, 5, n // case.N) and reg.shape == (case.N, n // case.N, 20)
    (cls.float().sum() + reg.float().square().sum()).backward()
    oboxes = orc.roi_transform(r4, inds, img_h, img_w, case.H, case.W)
    ro, ra = forward_ref(case, dt, rois=oboxes)
    assert same_bits(seen["cropped"], ro)
    assert seen["grad"].dtype == TORCH[dt] and (seen["grad"] != 0).any()
    assert same_bits(feats.grad, backward_ref(case, dt, seen["grad"].cpu(), oboxes, ra))
    assert (feats.grad != 0).any()


# ------------------------------------------------------------------ backward
@pairs(BWD_CASES)
def test_backward(case, dt):
    """From the device's own argmax, under every roi_pool_bwd path the case lists: the
    oracle's bits (CPU summation order), the same bits from path to path and from call
    to call."""
    cus = _lib.cu_count()
    shape = (case.N, case.C, case.H, case.W)
    args = (case.R,) + shape + tuple(case.size)
    for path, want in case.bwd.items():
        kind, icpw = ppc.bwd_plan(*args, path, cus)
        assert kind == want, (path, kind, cus)
        with _lib.kernel_path("roi_pool_bwd", path):
            got = _lib.roi_pool_bwd_kernel(*args, dtype=TORCH[dt])
        assert got == ppc.bwd_name(dt, *args, path, cus), (path, got)
        if case.group == "partial":
            if case.H * case.W * 4 <= ppc.constants().kPlaneBudget:
                assert case.N * case.C > 2 * cus, "too few planes for several channels per workgroup"
            assert icpw > 1 and case.C % icpw != 0, (path, icpw)
            assert cus != ppc.MI355X_CUS or icpw == case.icpw[path], (path, icpw)
    rois = case.rois()
    rd = dev(rois)
    out, am = ops.roi_pool_with_argmax(dev(features(case, dt)), rd, case.size, 1.0, rois_sorted=True)
    ra = forward_ref(case, dt)[1]
    assert np.array_equal(am.cpu().numpy(), ra)
    g = torch.from_numpy(case.grad()).to(TORCH[dt])
    gd = dev(g)
    ref = backward_ref(case, dt, g, rois, ra)
    for path in case.bwd:
        with _lib.kernel_path("roi_pool_bwd", path):
            a = _roi_pool_bwd(gd, rd, am, shape, 1.0)
            b = _roi_pool_bwd(gd, rd, am, shape, 1.0)
        assert a.dtype == TORCH[dt] and tuple(a.shape) == shape
        assert same_bits(a, ref), path          # so every path equals every other
        assert same_bits(b, ref), (path, "second call")


def test_backward_through_autograd_above_64_bins():
    """ops.roi_pool's own backward at 14 x 14, RoIs in any order (lists with batch
    indices outside [0, N))."""
    case = ppc.BY_NAME["bins_14x14"]
    rois = case.rois(False)
    x = dev(features(case, "f32")).requires_grad_()
    out = ops.roi_pool(x, dev(rois), case.size)
    ro, ra = forward_ref(case, "f32", False)
    assert same_bits(out, ro)
    g = torch.from_numpy(case.grad())
    out.backward(dev(g))
    assert same_bits(x.grad, backward_ref(case, "f32", g, rois, ra))


# ---------------------------------------------------------- guards and limits
@pytest.mark.parametrize("dt", ppc.ALL)
def test_fits_guard(dt):
    """The leader backward's buffer descriptors need R*C*PH*PW*4 < 2^31; one RoI more
    takes the ring kernel (name query only: the tensors would take gigabytes)."""
    s = ppc.FITS_SHAPE
    r = ppc.fits_edge(s["C"], 49)
    assert r * s["C"] * 49 * 4 < 2 ** 31 <= (r + 1) * s["C"] * 49 * 4
    k = ppc.constants()
    lead = f"{k.kBwdLead}, 7, 7"
    for R, kernel, args in ((r, "roi_pool_bwd_lead_kernel", lead), (r + 1, "roi_pool_bwd_pf_kernel", f"{k.kBwdRing}")):
        got = _lib.roi_pool_bwd_kernel(R, s["N"], s["C"], s["H"], s["W"], 7, 7, dtype=TORCH[dt])
        assert got == ppc._typed(dt, kernel, args), (R, got)
        assert got == ppc.bwd_name(dt, R, s["N"], s["C"], s["H"], s["W"], 7, 7, "auto", _lib.cu_count())
    assert _lib.roi_pool_bwd_kernel(r + 1, s["N"], s["C"], s["H"], s["W"], 7, 7) == "roi_pool_bwd_pf_kernel<8>"


@pytest.mark.parametrize("size", ppc.REJECTED_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rejected_output_sizes(size):
    """1,025 bins and an empty output: the C-ABI refuses them by its own message before it
    launches anything (caller buffers keep their fill), and the next valid call works."""
    r = np.random.default_rng(5)
    x = r.standard_normal((2, 4, 10, 12), dtype=np.float32)
    rois = np.array([[0, 0, 0, 5, 5], [1, 2, 1, 9, 8]], np.float32)
    xd, rd = dev(x), dev(rois)
    bins = r"output_size must have 1\.\.%d bins" % ppc.constants().kMaxBins
    with pytest.raises(_lib.FrcnnError, match="frcnn_roi_pool_fwd: " + bins):
        ops.roi_pool(xd, rd, size)
    bufs = (torch.full((2, 4) + size, 9.0, device=DEV), torch.full((2, 4) + size, 9, dtype=torch.int32, device=DEV),
            torch.full((2, 5), 9.0, device=DEV))
    with pytest.raises(_lib.FrcnnError, match="frcnn_roi_pool_fwd_head: " + bins):
        ops.roi_pool_head(xd, dev(rois[:, 1:]), dev(rois[:, 0]), size, 160.0, 192.0, rois_sorted=True, out=bufs)
    gi_shape = tuple(x.shape)
    with pytest.raises(_lib.FrcnnError, match="frcnn_roi_pool_bwd: bad output_size"):
        _roi_pool_bwd(torch.zeros((2, 4) + size, device=DEV), rd,
                      torch.zeros((2, 4) + size, dtype=torch.int32, device=DEV), gi_shape, 1.0)
    torch.cuda.synchronize()
    assert all((b == 9).all() for b in bufs)
    out, am = ops.roi_pool_with_argmax(xd, rd, (32, 32))
    oo, oa = orc.roi_pool_forward(x, rois, (32, 32))
    assert same_bits(out, oo) and np.array_equal(am.cpu().numpy(), oa)
    gi = _roi_pool_bwd(torch.ones((2, 4, 32, 32), device=DEV), rd, am, gi_shape, 1.0)
    assert same_bits(gi, orc.roi_pool_backward(np.ones((2, 4, 32, 32), np.float32), rois, oa, gi_shape))
