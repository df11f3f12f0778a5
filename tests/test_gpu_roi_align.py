"""RoIAlign forward and backward on the HIP path against the restatement of
tests/roi_align_ref.py (DESIGN.md §3 "RoIAlign").  Needs an MI355X.

Outputs and gradients are compared as bits, zero's sign included; NaNs compare by
position only.  16-bit types: widen, run the restatement, round once."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import pool_half_ref as phr
import roi_align_ref as ref
from replication_faster_rcnn_amd import _lib, heads, ops, synth
from replication_faster_rcnn_amd.ops import _roi_align_bwd, _roi_align_fwd
from replication_faster_rcnn_amd.rpn import RPN
from replication_faster_rcnn_amd.train import Trainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
HALF = pytest.mark.parametrize("dtype", ["f16", "bf16"])
PARAM_IDS = [f"sr{sr}-{'aligned' if al else 'plain'}-out{sz}-img{int(sc)}" for sr, al, sz, sc in ref.PARAMS]


def dev(a, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def assert_same(got, want, what=""):
    """got: device tensor; want: fp32 ndarray (the restatement), rounded once to got's dtype."""
    w = torch.from_numpy(np.ascontiguousarray(want, dtype=F)).to(got.dtype)
    g = got.detach().cpu().contiguous()
    assert g.shape == w.shape, (what, g.shape, w.shape)
    gn, wn = torch.isnan(g), torch.isnan(w)
    assert torch.equal(gn, wn), f"{what}: NaNs at other places"
    view = torch.int32 if g.dtype == torch.float32 else torch.int16
    bad = (g.view(view) != w.view(view)) & ~gn
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits"


def check(x, rois, size, scale=1.0, sr=-1, aligned=False, grad=None, what=""):
    """Forward and backward of the C-ABI pair on device tensors vs the restatement; x (and
    grad) are tensors of the dtype under test."""
    PH, PW = ref._size(size)
    rd = dev(np.asarray(rois, F).reshape(-1, 5))
    xd = dev(x)
    out = _roi_align_fwd(xd, rd, PH, PW, scale, sr, aligned)
    assert out.dtype == x.dtype and out.shape == (len(rois), x.shape[1], PH, PW)
    assert_same(out, ref.forward(x.float().numpy(), rois, (PH, PW), scale, sr, aligned), what + " forward")
    if grad is None:
        r = np.random.default_rng(len(rois) + PH)
        grad = torch.from_numpy(r.standard_normal(tuple(out.shape)).astype(F)).to(x.dtype)
    gi = _roi_align_bwd(dev(grad), rd, tuple(x.shape), scale, sr, aligned)
    assert gi.dtype == x.dtype and gi.shape == x.shape
    assert_same(gi, ref.backward(grad.float().numpy(), rois, tuple(x.shape), scale, sr, aligned), what + " backward")
    return out, gi


# ------------------------------------------------------- special values, fp32
@pytest.mark.parametrize("sr,aligned,size,img", ref.PARAMS, ids=PARAM_IDS)
def test_special_values_f32(sr, aligned, size, img):
    """+-0, +-inf, NaN stripes, subnormals and overflowing sums under RoIs inside, tiny,
    empty, partly and wholly off the map; gradients with +-0, inf and subnormals."""
    r = np.random.default_rng(7)
    x = torch.from_numpy(ref.special_x_f32(r))
    rois = ref.special_rois(scale=img)
    PH, PW = ref._size(size)
    g = r.standard_normal((len(rois), 16, PH, PW)).astype(F)
    g[:, 1] = 0.0
    g[:, 2, ::2] = -0.0
    g[:, 3, 0, 0] = np.inf                         # inf * 0 -> NaN at zero-weight corners
    g[:, 4] *= F(1e-42)                            # subnormal gradients
    g[:, 5] = F(3e38)                              # sums overflow
    check(x, rois, size, 1.0 / img, sr, aligned, torch.from_numpy(g))


# ------------------------------------------------------------- 16-bit types
@HALF
@pytest.mark.parametrize("sr,aligned,size,img", [ref.PARAMS[0], ref.PARAMS[3], ref.PARAMS[7], ref.PARAMS[12]],
                         ids=[PARAM_IDS[i] for i in (0, 3, 7, 12)])
def test_special_values_half(sr, aligned, size, img, dtype):
    r = np.random.default_rng(7)
    x = phr.special_x(TORCH[dtype], r)
    rois = ref.special_rois(scale=img)
    out, gi = check(x, rois, size, 1.0 / img, sr, aligned)
    if dtype == "f16":  # a float16 sum that overflows goes to inf at the one rounding
        big = torch.full((1, 1, 4, 4), 60000.0, dtype=torch.float16)
        gbig = torch.full((1, 1, 2, 2), 60000.0, dtype=torch.float16)
        o, g = check(big, np.array([[0, 1, 1, 1.2, 1.2]] * 3, F), 2, 1.0, 2, False, gbig.expand(3, 1, 2, 2).contiguous())
        assert torch.isinf(g).any() and torch.isfinite(o).all()


@HALF
def test_backward_rounds_once_not_per_addition(dtype):
    """Many contributions on few pixels, subnormal gradients among them: the fp32 sums
    rounded once differ from sums kept in the 16-bit type, and the kernel gives the former."""
    dt = TORCH[dtype]
    x, rois, grad = phr.colliding_case(dt)
    g = grad((len(rois), x.shape[1], 7, 7))
    rd = dev(rois)
    gi = _roi_align_bwd(dev(g), rd, tuple(x.shape), 1.0, 2, False)
    once = ref.backward(g.float().numpy(), rois, tuple(x.shape), 1.0, 2, False)
    assert_same(gi, once, "one rounding")
    in_t = ref.backward(g.float().numpy(), rois, tuple(x.shape), 1.0, 2, False,
                        acc_round=lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt).float().numpy())
    a, b = torch.from_numpy(once).to(dt), torch.from_numpy(in_t).to(dt)
    assert int((a.view(torch.int16) != b.view(torch.int16)).sum()) > 50, "the case cannot tell the two apart"


# -------------------------------------------------- launch plan: named cases
# every case in fp32; the 16-bit types where a tile, channel-group or clamping edge is crossed
HALF_CASES = ("wide_3x203", "tall_203x3", "c70", "map_1x1", "tile_edge_16x17")
PLAN_PARAMS = [(c, d) for c in ref.CASES for d in ("f32", "f16", "bf16") if d == "f32" or c.name in HALF_CASES]


@pytest.mark.parametrize("case,dtype", PLAN_PARAMS, ids=[f"{c.name}-{d}" for c, d in PLAN_PARAMS])
def test_plan_cases(case, dtype):
    """Every tile edge of the backward (8-pixel tiles along a long row and a long column,
    the 64-channel group edge), maps where every sample clamps."""
    dt = TORCH[dtype]
    x, rois, grad = case.inputs()
    R = len(rois)
    args = (R, case.N, case.C, case.H, case.W, *case.size)
    assert _lib.roi_align_kernel("fwd", *args, case.sampling_ratio, dt) == ref.fwd_name(dtype)
    assert _lib.roi_align_kernel("bwd", *args, case.sampling_ratio, dt) == ref.bwd_name(dtype)
    assert (np.diff(rois[:, 0]) < 0).any() or case.N == 1, "RoIs not grouped by image"
    check(torch.from_numpy(x).to(dt), rois, case.size, 1.0, case.sampling_ratio, case.aligned,
          torch.from_numpy(grad).to(dt), case.name)


# ------------------------------------------------------------------- edges
def test_no_rois():
    x = torch.randn(2, 3, 5, 6)
    out = ops.roi_align(x.to(DEV), torch.zeros((0, 5), device=DEV), 7)
    assert out.shape == (0, 3, 7, 7)
    gi = _roi_align_bwd(torch.zeros((0, 3, 7, 7), device=DEV), torch.zeros((0, 5), device=DEV), (2, 3, 5, 6), 1.0, 2,
                        False)
    assert gi.shape == (2, 3, 5, 6) and not gi.any() and not torch.signbit(gi).any()


def test_guarded_rois_and_bounded_work():
    """Batch indices -1 and N, coordinates of 3e6 / inf / NaN (guarded: zeros, no gradient),
    a box of ~4,000 px (adaptive grids of ~570 points per bin: clipped) and one tiny RoI 30
    times (many contributions on one pixel), not grouped by image."""
    r = np.random.default_rng(3)
    x = torch.from_numpy(r.standard_normal((2, 5, 12, 14)).astype(F))
    tiny = [1, 4.25, 3.5, 4.75, 3.75]
    rows = [[-1, 1, 1, 6, 6], [0, -1990, -2000, 2010, 2003], tiny, [2, 1, 1, 6, 6], [0, 3e6, 1, 5, 5],
            [1, 1, 1, np.inf, 5], tiny, [0, np.nan, 1, 5, 5], [0, 2, 3, 7, 8], [1, -5, -3e6, 5, 5], [np.nan, 0, 0, 4, 4],
            [1, 3, 2, 3960, 9]] + [tiny] * 28
    rois = np.array(rows, F)
    for sr, aligned in ((-1, False), (-1, True), (2, False)):
        out, gi = check(x, rois, 7, 1.0, sr, aligned, what=f"sr={sr} aligned={aligned}")
        guarded = [0, 3, 4, 5, 7, 9, 10]
        assert not out[guarded].any() and out[8].any()
        assert sr > 0 or (out[1].any() and out[11].any())   # two fixed samples per bin of a huge box all miss the map


def test_pixel_offsets_past_2_to_31():
    """A feature map of more than 2^31 elements (float16: 4 GiB): the planes read and written
    last lie past 32-bit element and byte offsets.  Only those planes carry values; the
    restatement runs on them alone (the batch index only selects the plane)."""
    C, H, W, K = (1 << 19) + 3, 64, 64, 3
    assert (C - K) * H * W >= 1 << 31
    r = np.random.default_rng(31)
    dt = torch.float16
    tail = torch.from_numpy(r.standard_normal((1, K, H, W)).astype(F)).to(dt)
    x = torch.zeros((1, C, H, W), dtype=dt, device=DEV)
    x[:, -K:] = tail.to(DEV)
    rois = np.array([[0, 3.3, 2.2, 50.5, 40.1], [0, -4, 30, 70, 66]], F)
    rd = dev(rois)
    out = _roi_align_fwd(x, rd, 7, 7, 1.0, 2, False)
    assert_same(out[:, -K:], ref.forward(tail.float().numpy(), rois, 7, 1.0, 2, False), "forward")
    assert not out[:, :-K].any()
    del x
    g_tail = torch.from_numpy(r.standard_normal((2, K, 7, 7)).astype(F)).to(dt)
    grad = torch.zeros((2, C, 7, 7), dtype=dt, device=DEV)
    grad[:, -K:] = g_tail.to(DEV)
    gi = _roi_align_bwd(grad, rd, (1, C, H, W), 1.0, 2, False)
    assert_same(gi[:, -K:], ref.backward(g_tail.float().numpy(), rois, (1, K, H, W), 1.0, 2, False), "backward")
    assert not gi[:, :8].any() and not gi[:, -K - 8:-K].any()


def test_two_calls_give_the_same_bits():
    case = ref.CASES[-1]
    x, rois, grad = case.inputs()
    xd, rd, gd = dev(x), dev(rois), dev(grad)
    outs = [_roi_align_fwd(xd, rd, 7, 7, 1.0, -1, False) for _ in range(2)]
    gis = [_roi_align_bwd(gd, rd, x.shape, 1.0, -1, False) for _ in range(2)]
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert torch.equal(gis[0].view(torch.int32), gis[1].view(torch.int32))


# ----------------------------------------------------------------- autograd
def test_autograd_host_leaf_and_list_of_boxes():
    r = np.random.default_rng(9)
    xn = r.standard_normal((2, 4, 9, 11)).astype(F)
    per_image = [r.uniform(0, 8, (3, 4)).astype(F), r.uniform(0, 8, (2, 4)).astype(F)]
    for b in per_image:
        b[:, 2:] += b[:, :2]
    rois = np.concatenate([np.concatenate([np.full((len(b), 1), i, F), b], 1) for i, b in enumerate(per_image)])
    g = r.standard_normal((5, 4, 3, 3)).astype(F)
    want_out = ref.forward(xn, rois, 3, 0.5, 2, True)
    want_gi = ref.backward(g, rois, xn.shape, 0.5, 2, True)
    for boxes in (torch.from_numpy(rois), [torch.from_numpy(b) for b in per_image]):
        x = torch.from_numpy(xn.copy()).requires_grad_(True)       # a host leaf
        out = ops.roi_align(x, boxes, 3, 0.5, sampling_ratio=2, aligned=True)
        assert out.device.type == "cpu"
        assert_same(out, want_out, "forward")
        out.backward(torch.from_numpy(g))
        assert x.grad is not None and x.grad.device.type == "cpu"
        assert_same(x.grad, want_gi, "backward")
    # a strided float64 input is converted; shapes that do not belong together raise
    x64 = torch.from_numpy(xn).double().permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert_same(ops.roi_align(x64, torch.from_numpy(rois), 3, 0.5, 2, True).float(), want_out, "float64 input")
    with pytest.raises(RuntimeError):
        ops.roi_align(torch.zeros(4, 9, 11), torch.from_numpy(rois), 3)
    with pytest.raises(RuntimeError):
        ops.roi_align(torch.from_numpy(xn), torch.zeros(5, 4), 3)
    with pytest.raises(RuntimeError):
        ops.roi_align(torch.from_numpy(xn), [torch.zeros(5, 4)], 3)
    with pytest.raises(RuntimeError, match="sampling_ratio"):
        ops.roi_align(torch.from_numpy(xn), torch.from_numpy(rois), 3, sampling_ratio=17)


# ---------------------------------------------------------- head and trainer
def test_head_with_pool_align():
    torch.manual_seed(5)
    r = np.random.default_rng(5)
    N, C, H, W, img_h, img_w = 2, 6, 10, 12, 160.0, 192.0
    classifier = nn.Sequential(nn.Flatten(), nn.Linear(C * 49, 512))
    head = heads.ResnetHead(classifier, n_classes=5, pool="align", sampling_ratio=2, aligned=True).to(DEV)
    x = torch.from_numpy(r.standard_normal((N, C, H, W)).astype(F))
    lo = r.uniform(0, 100, (8, 2))
    rois = np.concatenate([lo, lo + r.uniform(8, 90, (8, 2))], 1).astype(F)      # [ymin, xmin, ymax, xmax] pixels
    inds = np.array([0, 0, 0, 0, 1, 1, 1, 1], F)
    seen = []
    handle = classifier.register_forward_pre_hook(lambda m, a: seen.append(a[0].detach()))
    xd = dev(x).requires_grad_(True)
    cls, reg = head(xd, torch.from_numpy(rois), torch.from_numpy(inds), img_h, img_w)
    handle.remove()
    boxes = ops.roi_transform(dev(rois), dev(inds), img_h, img_w, H, W).cpu().numpy()
    crop = ref.forward(x.numpy(), boxes, 7, 1.0, 2, True)
    assert_same(seen[0], crop, "the head's crop")
    with torch.no_grad():
        fc = classifier(dev(crop))
        want_cls, want_reg = head.cls(fc).view(N, -1, 5).permute(0, 2, 1), head.reg(fc).view(N, -1, 20)
    assert torch.equal(cls.detach(), want_cls) and torch.equal(reg.detach(), want_reg)
    (cls.sum() + reg.sum()).backward()
    assert xd.grad is not None and xd.grad.abs().sum() > 0
    with pytest.raises(ValueError):
        heads.ResnetHead(classifier, pool="avg")
    assert heads.ResnetHead(classifier).pool == "max"


def test_fused_training_step_with_the_align_head(rng_guard):
    IMG_H, IMG_W, FH, FW, CF = 96, 112, 6, 7, 16
    torch.manual_seed(4)
    rpn = RPN(in_channels=CF, mid_channels=CF, anchor_scales=[1, 2, 4], mode="training")
    rpn.proposal_layer.pre_nms, rpn.proposal_layer.post_nms = 200, 48
    with torch.no_grad():
        rpn.reg.weight.normal_(0, 0.5)
        rpn.cls.weight.normal_(0, 0.5)
    rpn = rpn.cuda()
    head = heads.ResnetHead(nn.Sequential(nn.Conv2d(CF, 512, 1), nn.AdaptiveAvgPool2d(1)), pool="align",
                            sampling_ratio=2).cuda()
    bl = [synth.gt_boxes(IMG_H, IMG_W, 8, 9, i, n_valid=[5, 3][i]) for i in range(2)]
    boxes, labels = np.stack([b for b, _ in bl]), np.stack([l for _, l in bl])
    feats = torch.from_numpy(np.stack([synth.features(CF, FH, FW, 9, i) for i in range(2)])).cuda()
    runs = []
    for _ in range(3):   # the first step lets the convolutions pick their algorithms; it is not compared
        for p in list(rpn.parameters()) + list(head.parameters()):
            p.grad = None
        x = feats.clone().requires_grad_(True)
        np.random.seed(11)
        losses = Trainer(rpn, head, n_sample=(32, 16), fused_losses=True).train_step(x, IMG_H, IMG_W, boxes, labels)
        runs.append(({k: float(v) for k, v in losses.items()}, x.grad.clone()))
    assert all(np.isfinite(v) for v in runs[1][0].values()) and runs[1][1].abs().sum() > 0
    assert runs[1][0] == runs[2][0]
    assert torch.equal(runs[1][1].view(torch.int32), runs[2][1].view(torch.int32))
