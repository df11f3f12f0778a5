"""RoIAlign on the named launch-plan cases (tests/roi_align_plan_cases.py; DESIGN.md §3
"RoIAlign", "Launch-plan branches and the cases that pin them").  Needs an MI355X.

Every case first asserts, through ``frcnn_roi_align_plan``, that the launch has the units,
workgroups, idle waves and staging the case names, then compares forward and backward with
the restatement of tests/roi_align_ref.py as bits (zero's sign counts, NaNs by position).
The same paths run through the pyramid kernels on a pyramid whose workgroups straddle two
levels and on one whose middle level has no pixels."""
import numpy as np
import pytest
import torch

import multiscale_roi_align_ref as mref
import roi_align_plan_cases as PC
import roi_align_ref as ref
from replication_faster_rcnn_amd import _lib, ops
from replication_faster_rcnn_amd.ops import _multiscale_bwd, _multiscale_fwd, _roi_align_bwd, _roi_align_fwd

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CASES = PC.cases()
PARAMS = [(c, d) for c in CASES for d in ("f32", "f16", "bf16") if d == "f32" or c.half]
GUARD = 4096          # elements behind grad_in that must stay as they were
SENTINEL = -77.0


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


def assert_plan(c):
    """The launch is the one the case names."""
    q = _lib.roi_align_plan(c.R, c.N, c.C, c.H, c.W, *c.size)
    want = c.plan()
    assert {k: q[k] for k in want} == want, (c.name, q)
    for key in ("units", "blocks", "idle", "tiles_x", "tiles_y", "cgroups", "fwd_threads", "fwd_grid"):
        assert key not in c.pins or q[key] == c.pins[key], (c.name, key, q[key])
    assert "staged" not in c.pins or bool(q["staged"]) == c.pins["staged"]
    return q


def bwd_into_guarded_buffer(c, grad, dt):
    """frcnn_roi_align_bwd_t through the raw entry point into a buffer pre-filled with NaN,
    with GUARD elements behind it: (grad_in, guard)."""
    lib = _lib.load()
    n = int(np.prod(c.shape))
    buf = torch.full((n + GUARD,), float("nan"), dtype=dt, device=DEV)
    buf[n:] = SENTINEL
    gd, rd = dev(grad, dt), dev(c.rois)
    _lib.check(lib.frcnn_roi_align_bwd_t(_lib.dtype_code(dt), _lib.ptr(gd), _lib.ptr(rd), c.R, c.N, c.C, c.H, c.W,
                                         *c.size, 1.0, c.sampling_ratio, int(c.aligned), _lib.ptr(buf), None, 0,
                                         _lib.stream_ptr()), c.name)
    torch.cuda.synchronize()
    return buf[:n].view(c.shape), buf[n:]


# ------------------------------------------------------------ the named cases
@pytest.mark.parametrize("c,dtype", PARAMS, ids=[f"{c.name}-{d}" for c, d in PARAMS])
def test_named_case(c, dtype):
    dt = TORCH[dtype]
    assert_plan(c)
    x, rois, grad = c.inputs()
    x, grad = torch.from_numpy(x).to(dt), torch.from_numpy(grad).to(dt)
    rd = dev(rois)
    out = _roi_align_fwd(dev(x), rd, *c.size, 1.0, c.sampling_ratio, c.aligned)
    assert out.dtype == dt
    assert_same(out, ref.forward(x.float().numpy(), rois, c.size, 1.0, c.sampling_ratio, c.aligned), c.name + " forward")
    gi = _roi_align_bwd(dev(grad), rd, c.shape, 1.0, c.sampling_ratio, c.aligned)   # torch.empty: no memset helps
    assert gi.dtype == dt
    assert_same(gi, ref.backward(grad.float().numpy(), rois, c.shape, 1.0, c.sampling_ratio, c.aligned),
                c.name + " backward")


@pytest.mark.parametrize("name", ["units_1", "units_6", "stage_even_small", "out14_unstaged"])
def test_every_element_is_stored_and_nothing_behind_the_tensor(name):
    """grad_in pre-filled with NaN: none survives; the elements behind the tensor, where an
    idle wave taken for a live one would store, stay as they were."""
    c = PC.case(name)
    q = assert_plan(c)
    assert q["idle"] > 0
    _, rois, grad = c.inputs()
    gi, guard = bwd_into_guarded_buffer(c, grad, torch.float32)
    assert not torch.isnan(gi).any(), "an element of grad_in was never stored"
    assert_same(gi, ref.backward(grad, rois, c.shape, 1.0, c.sampling_ratio, c.aligned), name)
    assert bool((guard == SENTINEL).all()), "a store behind grad_in"


@pytest.mark.parametrize("name", ["walk72_unstaged", "r129"])
def test_two_calls_give_the_same_bits(name):
    c = PC.case(name)
    x, rois, grad = c.inputs()
    xd, rd, gd = dev(x), dev(rois), dev(grad)
    outs = [_roi_align_fwd(xd, rd, *c.size, 1.0, c.sampling_ratio, c.aligned) for _ in range(2)]
    gis = [_roi_align_bwd(gd, rd, c.shape, 1.0, c.sampling_ratio, c.aligned) for _ in range(2)]
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert torch.equal(gis[0].view(torch.int32), gis[1].view(torch.int32))


# ---------------------------------------------------------------- the pyramid
SCALES = [0.25, 0.125, 0.0625]
S0 = 32               # thresholds at 16 and 32 px: level 0 below 16, level 1 below 32, level 2 from 32 on


def pyramid(spec, seed):
    r = np.random.default_rng(seed)
    shapes = [(spec["N"], spec["C"], h, w) for h, w in spec["sizes"]]
    xs = [r.standard_normal(s).astype(F) for s in shapes]
    k_min, k_max = mref.k_range(SCALES)
    thr = ops.level_thresholds(k_min, k_max, S0, 4)
    return shapes, xs, thr, (k_min, k_max)


def pyramid_rois(n, N, seed):
    """Boxes of 4 .. 90 px in a 68 x 72 image, images shuffled."""
    r = np.random.default_rng(seed)
    wh = np.exp(r.uniform(np.log(4), np.log(90), (n, 2)))
    xy = np.stack([r.uniform(-8, 70, n), r.uniform(-8, 66, n)], 1)
    return np.concatenate([r.integers(0, N, n)[:, None], xy, xy + wh], 1).astype(F)


@pytest.mark.parametrize("size,sr,n_rois,staged,path", [(14, 2, 24, False, ("lane",)),
                                                        (7, 10, 12, True, ("walk", "scan", "scan"))],
                         ids=["out14_unstaged", "sr10_walk"])
def test_pyramid_workgroups_straddle_levels(size, sr, n_rois, staged, path):
    """first = [0, 18, 26], 28 units: workgroup 3 (units 15..19) holds tiles of levels 0 and 1,
    workgroup 5 (units 25..27 and two idle waves) tiles of levels 1 and 2."""
    s = PC.STRADDLE
    q = _lib.roi_align_multi_plan(s["sizes"], s["N"], s["C"], size, size)
    assert q["first"][:4] == s["first"] + [s["units"]] and q["units"] == s["units"] and q["blocks"] == 6
    assert q["idle"] == 2 and bool(q["staged"]) == staged == PC.staged(size, size)
    shapes, xs, thr, (k_min, k_max) = pyramid(s, 17)
    rois = pyramid_rois(n_rois, s["N"], 171)
    lv = mref.levels(rois, k_min, k_max, S0, 4)
    assert sorted(set(lv.tolist())) == [0, 1, 2]
    for l in range(3):
        for q_ in rois[lv == l]:
            assert PC.bwd_path(ref.geometry(q_, s["N"], size, size, SCALES[l], sr, False), size, size) == path
    rd = dev(rois)
    out, got_lv = _multiscale_fwd([dev(x) for x in xs], rd, size, size, SCALES, thr, sr, False, True)
    assert np.array_equal(got_lv.cpu().numpy(), lv)
    assert_same(out, mref.forward(xs, rois, size, SCALES, sr, False, lv), "forward")
    grad = np.random.default_rng(5).standard_normal(tuple(out.shape)).astype(F)
    gis = _multiscale_bwd(dev(grad), rd, shapes, SCALES, thr, sr, False)
    for l, (gi, w) in enumerate(zip(gis, mref.backward(grad, rois, shapes, SCALES, sr, False, lv))):
        assert gi.abs().sum() > 0
        assert_same(gi, w, f"backward, level {l}")


def test_pyramid_with_an_empty_middle_level():
    """A level without pixels between two that have them: its RoIs pool to +0 and give no
    gradient, the other levels are what they are without it."""
    s = PC.EMPTY_MIDDLE
    q = _lib.roi_align_multi_plan(s["sizes"], s["N"], s["C"])
    assert q["first"][1] == q["first"][2] == 8 and q["units"] == 10
    shapes, xs, thr, (k_min, k_max) = pyramid(s, 9)
    rois = pyramid_rois(30, s["N"], 91)
    lv = mref.levels(rois, k_min, k_max, S0, 4)
    assert sorted(set(lv.tolist())) == [0, 1, 2]
    want = np.zeros((len(rois), s["C"], 7, 7), F)
    for l in (0, 2):
        want[lv == l] = ref.forward(xs[l], rois[lv == l], 7, SCALES[l], 2, False)
    grad = np.random.default_rng(6).standard_normal(want.shape).astype(F)
    rd = dev(rois)
    out, got_lv = _multiscale_fwd([dev(x) for x in xs], rd, 7, 7, SCALES, thr, 2, False, True)
    assert np.array_equal(got_lv.cpu().numpy(), lv)
    assert_same(out, want, "forward")
    assert all_plus_zero(out[torch.from_numpy(lv == 1)]) and out[torch.from_numpy(lv != 1)].abs().sum() > 0
    gis = _multiscale_bwd(dev(grad), rd, shapes, SCALES, thr, 2, False)
    assert gis[1].shape == shapes[1] and gis[1].numel() == 0
    for l in (0, 2):
        assert_same(gis[l], ref.backward(grad[lv == l], rois[lv == l], shapes[l], SCALES[l], 2, False), f"level {l}")
    # the public op accepts the pyramid as well, autograd included
    leaves = [dev(x).requires_grad_(True) for x in xs]
    pooled = ops.multiscale_roi_align(leaves, rd, 7, SCALES, 2, canonical_scale=S0)
    assert torch.equal(pooled.detach().view(torch.int32), out.view(torch.int32))
    pooled.backward(dev(grad))
    for leaf, gi in zip(leaves, gis):
        assert leaf.grad is not None and leaf.grad.shape == gi.shape
        assert torch.equal(leaf.grad.view(torch.int32), gi.view(torch.int32))
