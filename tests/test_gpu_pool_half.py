"""RoIPool forward and backward on float16 / bfloat16 feature maps vs the references of
tests/pool_half_ref.py (DESIGN.md §3 "RoIPool in 16-bit types").  Needs an MI355X.

Everything is compared as bits: values through their int16 view, argmax with
array_equal.  The fp32 oracle on the widened input is the reference; the kernels may
differ from it by the one final rounding only, which for a max-pool is no difference
at all (bar -FLT_MAX -> -inf)."""
import numpy as np
import pytest
import torch

import pool_half_ref as phr
from oracle import ref_numpy as orc
from replication_faster_rcnn_amd import _lib, heads, ops
from replication_faster_rcnn_amd.ops import _roi_pool_bwd

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = pytest.mark.parametrize("dtype", phr.DTYPES, ids=["f16", "bf16"])
ELEM = {torch.float16: "__half", torch.bfloat16: "__hip_bfloat16"}
# forward paths: (kernel path, RoIs promised grouped by image)
FWD_PATHS = [("wave", True), ("dense", True), ("dense", False), ("generic", False)]


def dev(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(DEV)


def same_bits(got, want):
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    return torch.equal(phr.bits(got), phr.bits(want))


def check_forward(x, rois, output_size, rois_sorted, ss=1.0):
    out, am = ops.roi_pool_with_argmax(dev(x), dev(rois), output_size, ss, rois_sorted=rois_sorted)
    ro, ra = phr.forward_ref(x, rois, output_size, ss)
    assert out.dtype == x.dtype and am.dtype == torch.int32
    assert np.array_equal(am.cpu().numpy(), ra)
    assert same_bits(out, ro)
    return out, am


def random_x(r, shape, dtype, ties=None):
    x = r.standard_normal(shape).astype(np.float32)
    if ties is not None:
        x[ties] = np.round(x[ties])
    return torch.from_numpy(x).to(dtype)


def random_rois(r, b, H, W, span=None):
    """[len(b),5] RoIs reaching off the map; span None: sizes up to the map's, a few negative."""
    xy = r.uniform(-3, max(H, W) + 2, (len(b), 2)).astype(np.float32)
    wh = (r.uniform(-2, max(H, W), (len(b), 2)) if span is None else r.uniform(0, span, (len(b), 2))).astype(np.float32)
    return np.concatenate([np.asarray(b, np.float32)[:, None], xy, xy + wh], 1).astype(np.float32)


# ------------------------------------------------------------------- forward
@DT
@pytest.mark.parametrize("hw", [(12, 14), (38, 38)])
@pytest.mark.parametrize("fpath,sorted_", FWD_PATHS)
def test_forward_special_values(fpath, sorted_, hw, dtype):
    """Signed zeros, the dtype's lowest value, +-inf, NaN, subnormals and last-bit
    neighbours inside pooling windows, RoIs partly / wholly off the map, on every
    path; 38 x 38 takes the wave kernel's compile-time plane stride."""
    r = np.random.default_rng(7)
    x = phr.special_x(dtype, r, H=hw[0], W=hw[1])
    rois = phr.special_rois()
    if not sorted_:
        rois = rois[r.permutation(len(rois))]
    with _lib.kernel_path("roi_pool_fwd", fpath):
        want = {"wave": "roi_pool_fwd_wave_kernel_h<", "dense": "roi_pool_fwd_dense_kernel_h<",
                "generic": "roi_pool_fwd_kernel_h<"}[fpath] + ELEM[dtype] + ", "
        name = _lib.roi_pool_fwd_kernel(len(rois), 2, 16, hw[0], hw[1], rois_sorted=sorted_, head=False, dtype=dtype)
        assert name.startswith(want), name
        check_forward(x, rois, 7, sorted_)


@DT
@pytest.mark.parametrize("sorted_", [True, False])
@pytest.mark.parametrize("C,ph", [(12, 7), (8, 7), (3, 7), (12, 3), (8, 3), (3, 3)])
def test_forward_odd_plane_small_channel_groups(C, ph, sorted_, dtype):
    """A 9 x 11 plane (99 pixels: plane starts only 2-byte aligned) with 4 and 8
    channels per workgroup and, at C = 3, no tile path at all: the generic kernel with
    scalar stores (3 x 7 x 7 and 3 x 3 x 3 outputs are no multiple of four; its vector
    stores run in test_forward_special_values)."""
    r = np.random.default_rng(77 + C + ph)
    N, H, W, R = 2, 9, 11, 77
    x = random_x(r, (N, C, H, W), dtype, ties=(slice(None), slice(None), slice(None, None, 3), slice(None, None, 2)))
    b = np.sort(r.integers(0, N, R)) if sorted_ else r.integers(0, N, R)
    rois = random_rois(r, b, H, W)
    name = _lib.roi_pool_fwd_kernel(R, N, C, H, W, ph, ph, rois_sorted=sorted_, head=False, dtype=dtype)
    if C == 3:
        assert name == f"roi_pool_fwd_kernel_h<{ELEM[dtype]}, false>"
    else:
        assert f"_h<{ELEM[dtype]}, 1024, {4 if C == 12 else 8}, " in name, name
    check_forward(x, rois, ph, sorted_)


@DT
@pytest.mark.parametrize("sorted_", [True, False])
def test_forward_random_with_ties(sorted_, dtype):
    r = np.random.default_rng(11)
    N, C, H, W, R = 3, 32, 38, 63, 600
    x = random_x(r, (N, C, H, W), dtype, ties=(slice(None), slice(None), slice(10, 20), slice(10, 30)))
    b = np.sort(r.integers(0, N, R))
    if not sorted_:
        r.shuffle(b)
    rois = random_rois(r, b, H, W, span=40)
    check_forward(x, rois, 7, sorted_)


@DT
def test_forward_nontemporal_stores(dtype):
    r = np.random.default_rng(7)
    x = phr.special_x(dtype, r, H=38, W=38)
    rois = phr.special_rois(windows=phr.SPECIAL_WINDOWS[:5])
    with _lib.kernel_path("roi_pool_fwd", "wave"), _lib.kernel_path("roi_pool_fwd_store", "nt"):
        name = _lib.roi_pool_fwd_kernel(len(rois), 2, 16, 38, 38, head=False, dtype=dtype)
        assert name == f"roi_pool_fwd_wave_kernel_h<{ELEM[dtype]}, 1024, 16, 7, false, true, 38400>"
        check_forward(x, rois, 7, True)


@DT
@pytest.mark.parametrize("grouped", [True, False])
def test_forward_fused_head(grouped, dtype):
    """roi_pool_head with the transform inside the pool kernel (grouped) and ahead of
    it (ungrouped), with and without caller buffers: out in the input's dtype, boxes
    the fp32 call's bits."""
    r = np.random.default_rng(5 + grouped)
    N, C, H, W, R, img_h, img_w = 3, 16, 38, 63, 257, 600.0, 1000.0
    inds = np.sort(r.integers(0, N, R)).astype(np.float32)
    if not grouped:
        r.shuffle(inds)
    y1 = r.uniform(-20, img_h, R).astype(np.float32)
    x1 = r.uniform(-20, img_w, R).astype(np.float32)
    rois = np.stack([y1, x1, y1 + r.uniform(0, 400, R).astype(np.float32),
                     x1 + r.uniform(0, 600, R).astype(np.float32)], 1).astype(np.float32)
    x = random_x(r, (N, C, H, W), dtype, ties=(slice(None), slice(None), slice(5, 15), slice(5, 25)))
    xd, rd, idd = dev(x), dev(rois), dev(inds)
    out, am, boxes = ops.roi_pool_head(xd, rd, idd, 7, img_h, img_w, rois_sorted=grouped)
    boxes32 = ops.roi_pool_head(xd.float(), rd, idd, 7, img_h, img_w, rois_sorted=grouped)[2]
    assert boxes.dtype == torch.float32 and torch.equal(boxes.view(torch.int32), boxes32.view(torch.int32))
    oboxes = orc.roi_transform(rois, inds, img_h, img_w, H, W)
    assert np.array_equal(boxes.cpu().numpy().view(np.uint32), oboxes.view(np.uint32))
    ro, ra = phr.forward_ref(x, oboxes, 7)
    assert np.array_equal(am.cpu().numpy(), ra) and same_bits(out, ro)
    bufs = (torch.full((R, C, 7, 7), 9.0, dtype=dtype, device=DEV),
            torch.full((R, C, 7, 7), 9, dtype=torch.int32, device=DEV),
            torch.full((R, 5), 9.0, dtype=torch.float32, device=DEV))
    got = ops.roi_pool_head(xd, rd, idd, 7, img_h, img_w, rois_sorted=grouped, out=bufs)
    assert all(g is b for g, b in zip(got, bufs))
    assert same_bits(bufs[0], ro) and np.array_equal(bufs[1].cpu().numpy(), ra) and torch.equal(bufs[2], boxes)
    for bad_x, bad_out in ((xd, torch.float32), (xd.float(), dtype)):
        bad = (torch.empty((R, C, 7, 7), dtype=bad_out, device=DEV), bufs[1], bufs[2])
        with pytest.raises(RuntimeError, match="out buffers must be"):
            ops.roi_pool_head(bad_x, rd, idd, 7, img_h, img_w, rois_sorted=grouped, out=bad)


@DT
@pytest.mark.parametrize("sorted_", [False, True])
def test_forward_out_of_range_batch_index(sorted_, dtype):
    x = torch.randn(2, 8, 10, 12).to(dtype)
    rois = np.array([[-1, 0, 0, 5, 5], [1, 0, 0, 9, 9], [2, 1, 1, 4, 4], [7, 0, 0, 3, 3]], np.float32)
    out, am = ops.roi_pool_with_argmax(dev(x), dev(rois), 7, rois_sorted=sorted_)
    assert out.dtype == dtype
    assert (phr.bits(out[[0, 2, 3]]) == 0).all() and (am[[0, 2, 3]] == -1).all()
    ro, ra = phr.forward_ref(x, rois[1:2], 7)
    assert same_bits(out[1:2], ro) and np.array_equal(am[1:2].cpu().numpy(), ra)


@DT
def test_forward_empty_calls(dtype):
    x = torch.randn(2, 8, 10, 12, device=DEV).to(dtype)
    out, am = ops.roi_pool_with_argmax(x, torch.zeros((0, 5), device=DEV), 7)
    assert out.shape == (0, 8, 7, 7) and out.dtype == dtype and am.shape == (0, 8, 7, 7)
    rois = torch.tensor([[0, 0, 0, 5, 5]], dtype=torch.float32, device=DEV)
    out, am = ops.roi_pool_with_argmax(x[:, :0], rois, 7)
    assert out.shape == (1, 0, 7, 7) and out.dtype == dtype and am.dtype == torch.int32


def test_name_queries():
    """The fp32 answers are those of test_roi_pool_fwd_kernel_label; a 16-bit dtype
    names the _h sibling with its element type first."""
    R, N, C, H, W = 2400, 8, 256, 38, 63
    f32 = torch.float32
    assert _lib.roi_pool_fwd_kernel(R, N, C, H, W, dtype=f32) == "roi_pool_fwd_wave_kernel<1024, 16, 7, true, false, 38400>"
    assert _lib.roi_pool_fwd_kernel(R, N, C, H, W) == "roi_pool_fwd_wave_kernel<1024, 16, 7, true, false, 38400>"
    assert _lib.roi_pool_fwd_kernel(2000, 1, 512, 50, 84, dtype=f32) == "roi_pool_fwd_wave_kernel<1024, 8, 7, true>"
    assert _lib.roi_pool_bwd_kernel(2048, 16, 256, 38, 38, dtype=f32) == "roi_pool_bwd_lead_kernel<4, 7, 7>"
    assert _lib.roi_pool_bwd_kernel(2048, 16, 256, 38, 38, 5, 5) == "roi_pool_bwd_pf_kernel<8>"
    for dt, e in ELEM.items():
        assert _lib.roi_pool_fwd_kernel(R, N, C, H, W, dtype=dt) == \
            f"roi_pool_fwd_wave_kernel_h<{e}, 1024, 16, 7, true, false, 38400>"
        assert _lib.roi_pool_fwd_kernel(R, N, C, H, W, head=False, dtype=dt) == \
            f"roi_pool_fwd_wave_kernel_h<{e}, 1024, 16, 7, false, false, 38400>"
        assert _lib.roi_pool_fwd_kernel(2000, 1, 512, 50, 84, dtype=dt) == \
            f"roi_pool_fwd_wave_kernel_h<{e}, 1024, 8, 7, true>"
        assert _lib.roi_pool_fwd_kernel(R, N, C, H, W, rois_sorted=False, head=False, dtype=dt) == \
            f"roi_pool_fwd_dense_kernel_h<{e}, 1024, 16, 7, false, true>"
        assert _lib.roi_pool_bwd_kernel(2048, 16, 256, 38, 38, dtype=dt) == f"roi_pool_bwd_lead_kernel_h<{e}, 4, 7, 7>"
        assert _lib.roi_pool_bwd_kernel(2048, 16, 256, 38, 38, 9, 7, dtype=dt) == \
            f"roi_pool_bwd_lead_kernel_h<{e}, 4, 7, 0>"
        assert _lib.roi_pool_bwd_kernel(2048, 16, 256, 38, 38, 5, 5, dtype=dt) == f"roi_pool_bwd_pf_kernel_h<{e}, 8>"
        with _lib.kernel_path("roi_pool_bwd", "ring"):
            assert _lib.roi_pool_bwd_kernel(2048, 16, 256, 38, 38, dtype=dt) == f"roi_pool_bwd_pf_kernel_h<{e}, 8>"
        with _lib.kernel_path("roi_pool_bwd", "plain"):
            assert _lib.roi_pool_bwd_kernel(2048, 16, 256, 38, 38, dtype=dt) == f"roi_pool_bwd_kernel_h<{e}, true>"
            assert _lib.roi_pool_bwd_kernel(6, 1, 2, 130, 130, dtype=dt) == f"roi_pool_bwd_kernel_h<{e}, false>"


# ------------------------------------------------------------------ backward
def check_backward(x, rois, output_size, dtype, grad=None, paths=("auto",), r=None):
    """Forward on the device (its argmax feeds the backward), then every path against
    backward_ref and against each other."""
    xd, rd = dev(x), dev(rois)
    out, am = ops.roi_pool_with_argmax(xd, rd, output_size)
    g = grad(out.shape) if grad is not None else torch.from_numpy(
        r.standard_normal(tuple(out.shape)).astype(np.float32)).to(dtype)
    ref = phr.backward_ref(g, rois, am.cpu().numpy(), x.shape)
    res = []
    for p in paths:
        with _lib.kernel_path("roi_pool_bwd", p):
            gi = _roi_pool_bwd(dev(g), rd, am, x.shape, 1.0)
        assert gi.dtype == dtype and gi.shape == x.shape
        assert same_bits(gi, ref), p
        res.append(gi)
    return res[0], ref, (g, rd, am)


@DT
def test_backward_paths_agree(dtype):
    """The leader kernel (auto), the ring and the plain plane owner: identical bits,
    incl. images with 0 / 5 / 8 / 77 RoIs and duplicated RoIs."""
    r = np.random.default_rng(7)
    N, C, H, W = 4, 20, 38, 38
    x = random_x(r, (N, C, H, W), dtype)
    rows = []
    for b, k in enumerate([0, 5, 8, 77]):
        for _ in range(k):
            x0, y0 = r.uniform(-2, 30, 2)
            w, h = r.uniform(0, 20, 2)
            rows.append([b, x0, y0, x0 + w, y0 + h])
    rows += rows[-10:]  # duplicates in the last image
    rois = np.array(rows, np.float32)
    assert _lib.roi_pool_bwd_kernel(len(rois), N, C, H, W, dtype=dtype).startswith("roi_pool_bwd_lead_kernel_h<")
    check_backward(x, rois, 7, dtype, paths=("auto", "ring", "plain"), r=r)


@DT
@pytest.mark.parametrize("size,kernel", [((9, 7), "roi_pool_bwd_lead_kernel_h<{}, 4, 7, 0>"),
                                         ((5, 5), "roi_pool_bwd_pf_kernel_h<{}, 8>")])
def test_backward_other_output_sizes(size, kernel, dtype):
    r = np.random.default_rng(size[0])
    N, C, H, W, R = 3, 12, 20, 24, 150
    x = random_x(r, (N, C, H, W), dtype)
    rois = random_rois(r, np.sort(r.integers(0, N, R)), H, W)
    assert _lib.roi_pool_bwd_kernel(R, N, C, H, W, size[0], size[1], dtype=dtype) == kernel.format(ELEM[dtype])
    check_backward(x, rois, size, dtype, r=r)


@DT
def test_backward_plane_in_global_memory(dtype):
    """A 130 x 130 plane (66 KB in fp32) does not fit the plain kernel's LDS budget:
    the sums run in an fp32 scratch plane in global memory and are rounded once."""
    r = np.random.default_rng(130)
    N, C, H, W = 1, 2, 130, 130
    x = random_x(r, (N, C, H, W), dtype)
    rois = np.array([[0, 0, 0, 129, 129], [0, 3, 3, 9, 9], [0, 3, 3, 9, 9], [0, 100, 90, 140, 140],
                     [0, 50, 50, 50.4, 50.4], [0, 10, 20, 90, 60]], np.float32)
    with _lib.kernel_path("roi_pool_bwd", "plain"):
        assert _lib.roi_pool_bwd_kernel(6, N, C, H, W, dtype=dtype) == f"roi_pool_bwd_kernel_h<{ELEM[dtype]}, false>"
    check_backward(x, rois, 7, dtype, paths=("plain",), r=r)


@DT
@pytest.mark.parametrize("path", ["auto", "ring", "plain"])
def test_backward_colliding_gradients(path, dtype):
    """Tiny RoIs whose 49 bins share a few pixels, gradients with subnormals of the
    dtype and -0.0: fp32 sums in the CPU order, one rounding (test_pool_half_cpu.py
    shows that sums kept in the dtype give other bits here)."""
    x, rois, grad = phr.colliding_case(dtype)
    check_backward(x, rois, 7, dtype, grad=grad, paths=(path,))


@DT
@pytest.mark.parametrize("path", ["auto", "ring", "plain"])
def test_backward_write_out_tail(path, dtype):
    """H x W = 9 x 11: 99 pixels per plane, so the write-out takes its scalar form."""
    r = np.random.default_rng(99)
    N, C, H, W, R = 2, 12, 9, 11, 77
    x = random_x(r, (N, C, H, W), dtype)
    rois = random_rois(r, r.integers(0, N, R), H, W)
    check_backward(x, rois, 7, dtype, paths=(path,), r=r)


@DT
def test_backward_overflow(dtype):
    """Two colliding gradients of 60,000: 120,000 is beyond float16 (+inf) and within
    bfloat16."""
    r = np.random.default_rng(6)
    x = random_x(r, (1, 4, 12, 12), dtype)
    rois = np.array([[0, 1, 1, 9, 9]] * 2, np.float32)
    gi, ref, _ = check_backward(x, rois, 7, dtype, grad=lambda s: torch.full(tuple(s), 60000.0).to(dtype),
                                paths=("auto", "ring", "plain"))
    if dtype == torch.float16:
        assert torch.isposinf(gi).any() and not torch.isnan(gi).any()
    else:
        assert torch.isfinite(gi).all() and (gi.float() > 100000).any()


@DT
def test_backward_empty_and_repeat_calls(dtype):
    r = np.random.default_rng(1)
    x = random_x(r, (2, 16, 20, 20), dtype)
    gi = _roi_pool_bwd(torch.zeros((0, 16, 7, 7), dtype=dtype, device=DEV), torch.zeros((0, 5), device=DEV),
                       torch.zeros((0, 16, 7, 7), dtype=torch.int32, device=DEV), x.shape, 1.0)
    assert gi.dtype == dtype and gi.shape == x.shape and (phr.bits(gi) == 0).all()
    rois = np.array([[0, 0, 0, 19, 19], [1, 2, 2, 3, 3], [0, 5, 5, 5.4, 5.4]] * 30, np.float32)
    a, _, (g, rd, am) = check_backward(x, rois, 7, dtype, r=r)
    b = _roi_pool_bwd(dev(g), rd, am, x.shape, 1.0)
    assert same_bits(a, b)


# ------------------------------------------------------- autograd and the head
@DT
def test_autograd_keeps_the_dtype(dtype):
    r = np.random.default_rng(3)
    N, C, H, W, R = 2, 16, 20, 24, 60
    x = random_x(r, (N, C, H, W), dtype)
    rois = random_rois(r, np.sort(r.integers(0, N, R)), H, W)
    xd = dev(x).requires_grad_()
    out = ops.roi_pool(xd, dev(rois), 7)
    assert out.dtype == dtype
    ra = phr.forward_ref(x, rois, 7)[1]
    g = torch.from_numpy(r.standard_normal(tuple(out.shape)).astype(np.float32)).to(dtype)
    out.backward(dev(g))
    assert xd.grad.dtype == dtype and same_bits(xd.grad, phr.backward_ref(g, rois, ra, x.shape))
    xd.grad = None
    ops.roi_pool(xd, dev(rois), 7).sum().backward()   # an expanded (stride-0) gradient
    assert same_bits(xd.grad, phr.backward_ref(torch.ones(tuple(out.shape), dtype=dtype), rois, ra, x.shape))


@pytest.mark.parametrize("form", ["fp64", "cpu", "channels_last"])
def test_other_input_forms_still_return_fp32(form):
    r = np.random.default_rng(4)
    N, C, H, W, R = 2, 8, 12, 14, 40
    x32 = r.standard_normal((N, C, H, W)).astype(np.float32)
    rois = random_rois(r, np.sort(r.integers(0, N, R)), H, W)
    x = {"fp64": lambda: torch.from_numpy(x32).double().to(DEV),
         "cpu": lambda: torch.from_numpy(x32),
         "channels_last": lambda: torch.from_numpy(x32).to(DEV).contiguous(memory_format=torch.channels_last)}[form]()
    out, am = ops.roi_pool_with_argmax(x, torch.from_numpy(rois), 7)
    oo, oa = orc.roi_pool_forward(x32, rois, 7)
    assert out.dtype == torch.float32 and out.device == x.device
    assert np.array_equal(out.cpu().numpy().view(np.uint32), oo.view(np.uint32))
    assert np.array_equal(am.cpu().numpy(), oa)


@DT
def test_resnet_head_under_autocast(dtype):
    """ResnetHead on 16-bit features under autocast: the classifier sees the pooled
    tensor in the features' dtype, and features.grad is the 16-bit backward of the
    gradient that reached the pool output."""
    r = np.random.default_rng(8)
    N, C, H, W, R, img_h, img_w = 2, 16, 20, 24, 40, 320.0, 384.0
    x = random_x(r, (N, C, H, W), dtype)
    inds = np.sort(r.integers(0, N, R)).astype(np.float32)
    y1 = r.uniform(0, img_h - 40, R).astype(np.float32)
    x1 = r.uniform(0, img_w - 40, R).astype(np.float32)
    rois = np.stack([y1, x1, y1 + r.uniform(8, 200, R).astype(np.float32),
                     x1 + r.uniform(8, 200, R).astype(np.float32)], 1).astype(np.float32)
    torch.manual_seed(0)
    head = heads.ResnetHead(torch.nn.Conv2d(C, 512, 7), n_classes=5).to(DEV)
    seen = {}

    def pre_hook(_mod, inp):
        seen["cropped"] = inp[0].detach().clone()
        inp[0].register_hook(lambda g: seen.__setitem__("grad", g.detach().clone()))

    head.classifier.register_forward_pre_hook(pre_hook)
    feats = dev(x).requires_grad_()
    with torch.autocast("cuda", dtype=dtype):
        cls, reg = head(feats, torch.from_numpy(rois), torch.from_numpy(inds), img_h, img_w, rois_sorted=True)
    (cls.float().sum() + reg.float().square().sum()).backward()
    oboxes = orc.roi_transform(rois, inds, img_h, img_w, H, W)
    ro, ra = phr.forward_ref(x, oboxes, 7)
    assert seen["cropped"].dtype == dtype and same_bits(seen["cropped"], ro)
    assert seen["grad"].dtype == dtype and feats.grad.dtype == dtype
    assert same_bits(feats.grad, phr.backward_ref(seen["grad"], oboxes, ra, x.shape))
    assert (feats.grad != 0).any()
