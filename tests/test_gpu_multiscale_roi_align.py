"""Multi-scale RoIAlign on the HIP path against the restatement of
tests/multiscale_roi_align_ref.py (DESIGN.md §3 "Multi-scale RoIAlign").  Needs an MI355X.

Levels, outputs and every level's gradient are compared as bits, zero's sign included.
16-bit types: widen, run the restatement, round once.  The levels the kernels count
against thresholds are compared with the LevelMapper formula evaluated here."""
import numpy as np
import pytest
import torch

import multiscale_roi_align_ref as mref
import roi_align_ref as ref
from replication_faster_rcnn_amd import _lib, ops
from replication_faster_rcnn_amd.ops import _multiscale_bwd, _multiscale_fwd

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def dev(a, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def assert_same(got, want, what=""):
    """got: tensor; want: fp32 ndarray (the restatement), rounded once to got's dtype."""
    w = torch.from_numpy(np.ascontiguousarray(want, dtype=F)).to(got.dtype)
    g = got.detach().cpu().contiguous()
    assert g.shape == w.shape, (what, g.shape, w.shape)
    gn, wn = torch.isnan(g), torch.isnan(w)
    assert torch.equal(gn, wn), f"{what}: NaNs at other places"
    view = torch.int32 if g.dtype == torch.float32 else torch.int16
    bad = (g.view(view) != w.view(view)) & ~gn
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits"


def all_plus_zero(t):
    return not t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).any()


class Pyramid:
    """Maps, scales and the LevelMapper's parameters of one test pyramid."""

    def __init__(self, N, C, sizes, scales, s0=224, lvl0=4, seed=0):
        self.N, self.C, self.sizes, self.scales, self.s0, self.lvl0 = N, C, sizes, list(scales), s0, lvl0
        self.k_min, self.k_max = mref.k_range(scales)
        assert self.k_max - self.k_min + 1 == len(sizes)
        self.shapes = [(N, C, h, w) for h, w in sizes]
        r = np.random.default_rng(seed)
        self.xs = [r.standard_normal(s).astype(F) for s in self.shapes]
        self.thr = ops.level_thresholds(self.k_min, self.k_max, s0, lvl0)

    def levels(self, rois):
        return mref.levels(rois, self.k_min, self.k_max, self.s0, self.lvl0)


def check(p, rois, size, sr, aligned, dtype="f32", grad=None, what=""):
    """The C-ABI pair on device tensors against the restatement: levels, output, every gradient."""
    dt = TORCH[dtype]
    PH, PW = ref._size(size)
    rois = np.asarray(rois, F).reshape(-1, 5)
    xs = [torch.from_numpy(x).to(dt) for x in p.xs]
    lv = p.levels(rois)
    rd = dev(rois)
    out, got_lv = _multiscale_fwd([dev(x) for x in xs], rd, PH, PW, p.scales, p.thr, sr, aligned, True)
    assert out.dtype == dt and out.shape == (len(rois), p.C, PH, PW)
    assert got_lv.dtype == torch.int32 and np.array_equal(got_lv.cpu().numpy(), lv), what + " levels"
    want = mref.forward([x.float().numpy() for x in xs], rois, (PH, PW), p.scales, sr, aligned, lv)
    assert_same(out, want, what + " forward")
    if grad is None:
        r = np.random.default_rng(len(rois) + PH)
        grad = torch.from_numpy(r.standard_normal(tuple(out.shape)).astype(F)).to(dt)
    gis = _multiscale_bwd(dev(grad), rd, p.shapes, p.scales, p.thr, sr, aligned)
    wants = mref.backward(grad.float().numpy(), rois, p.shapes, p.scales, sr, aligned, lv)
    assert len(gis) == len(p.shapes)
    for l, (gi, w) in enumerate(zip(gis, wants)):
        assert gi.dtype == dt
        assert_same(gi, w, f"{what} backward, level {l}")
    return out, got_lv, gis


# ------------------------------------------------------------- level edges
def test_level_edges():
    """Boxes whose fp32 sqrt(area) is one bit pattern below, at, and one above each threshold;
    zero-area, negative-extent and NaN-coordinate boxes; a box far above the last threshold."""
    p = Pyramid(1, 3, [(16, 16), (8, 8), (4, 4), (2, 2)], [2.0 ** -k for k in (2, 3, 4, 5)], seed=1)
    rows, want = [], []
    for k, t in enumerate(p.thr):
        for d in (-1, 0, 1):
            v = mref.ulp_step(t, d)
            box = mref.box_with_root(v)
            assert mref.root_area(np.concatenate([[0], box]))[0] == v
            rows.append([0, *box])
            want.append(k + (d >= 0))
    rows += [[0, 5, 5, 5, 90], [0, 5, 5, 90, 5], [0, 7, 7, 7, 7],       # zero area
             [0, 9, 9, 300, 2], [0, 300, 300, 0, 0],                    # one / both extents negative
             [0, np.nan, 0, 9, 9], [0, 0, 0, 9, np.nan],                # NaN coordinates
             [0, 0, 0, 40000, 40000], [0, 0, 0, np.inf, 9]]             # far above t_3
    want += [0, 0, 0, 0, 2, 0, 0, 3, 3]
    rois = np.array(rows, F)
    assert p.levels(rois).tolist() == want
    _, lv, _ = check(p, rois, 7, 2, False, what="edges")
    assert lv.cpu().tolist() == want
    # return_levels of the public op says the same
    _, lv2 = ops.multiscale_roi_align([dev(x) for x in p.xs], dev(rois), 7, p.scales, 2, return_levels=True)
    assert lv2.dtype == torch.int32 and lv2.cpu().tolist() == want


# ---------------------------------------------------- forward and backward
# 256 x 320 images: a canonical size of 56 px at level 4 puts the thresholds at ~28, 56 and 112 px,
# so sides of 8..400 px reach all four levels (at the default 224 px nothing below 448 px reaches the last)
MAIN = Pyramid(2, 70, [(64, 80), (32, 40), (16, 20), (8, 10)], [2.0 ** -k for k in (2, 3, 4, 5)], s0=56, seed=70)


def main_rois():
    r = np.random.default_rng(150)
    K = 150
    wh = np.exp(r.uniform(np.log(8), np.log(400), (K, 2)))
    xy = np.stack([r.uniform(-20, 300, K), r.uniform(-20, 240, K)], 1)
    b = r.integers(0, 2, K)                                     # image order shuffled
    rois = np.concatenate([b[:, None], xy, xy + wh], 1).astype(F)
    rois[10, 0], rois[60, 0], rois[110, 4] = -1, 2, np.inf      # guarded: zeros, no gradient
    return rois


MAIN_PARAMS = [(sr, al, sz) for sr in (2, -1) for al in (False, True) for sz in (7, (3, 5))]


@pytest.mark.parametrize("sr,aligned,size", MAIN_PARAMS, ids=[f"sr{a}-{'aligned' if b else 'plain'}-out{c}"
                                                               for a, b, c in MAIN_PARAMS])
def test_forward_backward_f32(sr, aligned, size):
    rois = main_rois()
    lv = MAIN.levels(rois)
    assert sorted(set(lv.tolist())) == [0, 1, 2, 3], "a level is not populated"
    assert (np.diff(rois[:, 0]) < 0).any(), "RoIs grouped by image"
    out, _, _ = check(MAIN, rois, size, sr, aligned)
    assert not out[[10, 60, 110]].any() and out[[9, 61]].any()


@pytest.mark.parametrize("dtype,sr,aligned,size", [("f16", 2, False, 7), ("bf16", -1, True, (3, 5))])
def test_forward_backward_half(dtype, sr, aligned, size):
    check(MAIN, main_rois(), size, sr, aligned, dtype)


# ------------------------------------------------------ tile and map edges
def test_tile_and_map_edges():
    """Maps that are no multiple of the backward's 8-pixel tile, and a 1 x 1 coarsest map."""
    p = Pyramid(2, 5, [(13, 9), (7, 5), (4, 3), (1, 1)], [0.25, 0.125, 0.0625, 0.03125], s0=16, seed=13)
    r = np.random.default_rng(139)
    K = 60
    wh = np.exp(r.uniform(np.log(2), np.log(80), (K, 2)))
    xy = np.stack([r.uniform(-6, 40, K), r.uniform(-6, 56, K)], 1)
    rois = np.concatenate([r.integers(0, 2, K)[:, None], xy, xy + wh], 1).astype(F)
    assert sorted(set(p.levels(rois).tolist())) == [0, 1, 2, 3]
    for sr, aligned in ((2, False), (-1, True)):
        check(p, rois, 7, sr, aligned, what=f"sr={sr}")


# -------------------------------------------------------------- empty cases
def test_all_rois_on_one_level():
    p = Pyramid(2, 6, [(20, 24), (10, 12), (5, 6)], [0.25, 0.125, 0.0625], s0=56, seed=3)
    r = np.random.default_rng(33)
    K = 20
    side = r.uniform(30, 50, (K, 2))                            # sqrt(area) in [30, 50]: level 1 of 28 / 56
    xy = r.uniform(0, 50, (K, 2))
    rois = np.concatenate([r.integers(0, 2, K)[:, None], xy, xy + side], 1).astype(F)
    assert set(p.levels(rois).tolist()) == {1}
    for dtype in ("f32", "bf16"):
        _, _, gis = check(p, rois, 7, 2, False, dtype)
        assert all_plus_zero(gis[0]) and all_plus_zero(gis[2]) and gis[1].any()


def test_no_rois():
    p = Pyramid(2, 3, [(9, 10), (5, 5)], [0.25, 0.125], seed=4)
    xs = [dev(x).requires_grad_(True) for x in p.xs]
    out = ops.multiscale_roi_align(xs, torch.zeros((0, 5), device=DEV), 7, p.scales, 2)
    assert out.shape == (0, 3, 7, 7)
    out.sum().backward()
    gis = _multiscale_bwd(torch.zeros((0, 3, 7, 7), device=DEV), torch.zeros((0, 5), device=DEV), p.shapes, p.scales,
                          p.thr, 2, False)
    for x, gi in zip(xs, gis):
        assert gi.shape == x.shape and all_plus_zero(gi)
        assert x.grad is not None and x.grad.shape == x.shape and not x.grad.any()


# -------------------------------------------------------- wrapper and launch
def test_one_level_equals_roi_align():
    case = ref.CASES[-1]
    x, rois, grad = case.inputs()
    rois[:, 1:] *= 16
    a = dev(x).requires_grad_(True)
    b = dev(x).requires_grad_(True)
    one, lv = ops.multiscale_roi_align([a], dev(rois), 7, [0.0625], -1, aligned=True, return_levels=True)
    two = ops.roi_align(b, dev(rois), 7, 0.0625, -1, True)
    assert torch.equal(one.view(torch.int32), two.view(torch.int32)) and not lv.any() and lv.shape == (len(rois),)
    one.backward(dev(grad))
    two.backward(dev(grad))
    assert torch.equal(a.grad.view(torch.int32), b.grad.view(torch.int32))
    # the kernels themselves, at one level, against the single-map restatement
    p = Pyramid(case.N, case.C, [(case.H, case.W)], [0.0625], seed=case.seed)
    check(p, rois, 7, -1, True, what="L=1")


def test_eight_levels():
    sizes = [(65, 66), (33, 33), (17, 17), (9, 9), (5, 5), (3, 3), (2, 2), (1, 1)]
    p = Pyramid(1, 5, sizes, [2.0 ** -k for k in range(1, 9)], s0=8, lvl0=4, seed=8)
    assert len(p.thr) == 7
    r = np.random.default_rng(88)
    K = 64
    wh = np.exp(r.uniform(np.log(1), np.log(300), (K, 1))) * r.uniform(0.7, 1.4, (K, 2))
    xy = r.uniform(-4, 120, (K, 2))
    rois = np.concatenate([np.zeros((K, 1)), xy, xy + wh], 1).astype(F)
    assert sorted(set(p.levels(rois).tolist())) == list(range(8))
    check(p, rois, (3, 5), 2, False, what="L=8")


def small_pyramid():
    p = Pyramid(2, 6, [(24, 32), (12, 16), (6, 8)], [0.25, 0.125, 0.0625], s0=56, seed=21)
    r = np.random.default_rng(212)
    per_image = []
    for _ in range(2):
        side = np.exp(r.uniform(np.log(8), np.log(50), (7, 2)))      # below 56: the last level stays empty
        xy = r.uniform(0, 80, (7, 2))
        per_image.append(np.concatenate([xy, xy + side], 1).astype(F))
    rois = np.concatenate([np.concatenate([np.full((len(b), 1), i, F), b], 1) for i, b in enumerate(per_image)])
    return p, per_image, rois


def test_autograd_gives_the_capi_backward():
    p, per_image, rois = small_pyramid()
    lv = p.levels(rois)
    assert set(lv.tolist()) == {0, 1}
    g = np.random.default_rng(5).standard_normal((len(rois), p.C, 7, 7)).astype(F)
    want = _multiscale_bwd(dev(g), dev(rois), p.shapes, p.scales, p.thr, 2, True)
    assert all_plus_zero(want[2])
    for where in ("cuda", "cpu"):                                    # device tensors; host leaves, a list of boxes
        xs = [torch.from_numpy(x).to(where).requires_grad_(True) for x in p.xs]
        boxes = dev(rois) if where == "cuda" else [torch.from_numpy(b) for b in per_image]
        out = ops.multiscale_roi_align(xs, boxes, 7, p.scales, 2, canonical_scale=56, aligned=True)
        assert out.device.type == where
        assert_same(out, mref.forward(p.xs, rois, 7, p.scales, 2, True, lv), "forward")
        out.backward(torch.from_numpy(g).to(where))
        for x, w in zip(xs, want):
            assert x.grad is not None and x.grad.device.type == where     # zeros, not None, for the empty level
            assert torch.equal(x.grad.cpu().view(torch.int32), w.cpu().view(torch.int32))
    # float16 maps are pooled as they are
    xs = [dev(x, torch.float16).requires_grad_(True) for x in p.xs]
    out = ops.multiscale_roi_align(xs, dev(rois), 7, p.scales, 2, canonical_scale=56)
    out.float().sum().backward()
    assert out.dtype == torch.float16 and all(x.grad.dtype == torch.float16 for x in xs)


def test_module_on_a_dict_equals_the_functional_op():
    p, per_image, rois = small_pyramid()
    feats = {"p2": dev(p.xs[0]), "p3": dev(p.xs[1]), "pool": torch.zeros(1, device=DEV), "p4": dev(p.xs[2])}
    pool = ops.MultiScaleRoIAlign(["p2", "p3", "p4"], 7, 2, canonical_scale=56)
    boxes = [dev(b) for b in per_image]
    shapes = [(96, 128), (90, 120)]
    out = pool(feats, boxes, shapes)
    assert pool.scales == (0.25, 0.125, 0.0625)
    want = ops.multiscale_roi_align([dev(x) for x in p.xs], dev(rois), 7, p.scales, 2, canonical_scale=56)
    assert out.shape == (len(rois), p.C, 7, 7) and torch.equal(out.view(torch.int32), want.view(torch.int32))
    assert_same(out, mref.forward(p.xs, rois, 7, p.scales, 2, False, p.levels(rois)), "module")
    assert torch.equal(pool(feats, boxes, [(1, 1)]).view(torch.int32), out.view(torch.int32))   # scales are cached


def test_two_calls_give_the_same_bits():
    rois = dev(main_rois())
    xs = [dev(x) for x in MAIN.xs]
    g = dev(np.random.default_rng(1).standard_normal((rois.size(0), MAIN.C, 7, 7)).astype(F))
    outs = [_multiscale_fwd(xs, rois, 7, 7, MAIN.scales, MAIN.thr, -1, False, False)[0] for _ in range(2)]
    gis = [_multiscale_bwd(g, rois, MAIN.shapes, MAIN.scales, MAIN.thr, -1, False) for _ in range(2)]
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    for a, b in zip(*gis):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_name_queries(dtype):
    assert _lib.roi_align_multi_kernel("fwd", 4, 150, 2, 70, 7, 7, 2, TORCH[dtype]) == mref.fwd_name(dtype)
    assert _lib.roi_align_multi_kernel("bwd", 4, 150, 2, 70, 7, 7, 2, TORCH[dtype]) == mref.bwd_name(dtype)
