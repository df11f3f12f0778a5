"""The ops that read the network's predictions, on float16 / bfloat16 predictions (DESIGN.md §3
"Predictions in 16-bit types"): the RPN head epilogue, the fused losses, ops.detect, and the
modules around them under torch.autocast.

Everything is compared as bits (a 16-bit tensor through its int16 view, fp32 through int32):
what an op returns as fp32 / int32 must be the fp32 op's result on the widened inputs, a permuted
copy must hold the input's bit patterns, and a gradient must be the fp32 op's gradient rounded
once (``.to(dtype)``)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import detect_ref  # noqa: E402
import loss_cases  # noqa: E402
import loss_ref  # noqa: E402
from replication_faster_rcnn_amd import ops, synth  # noqa: E402
from replication_faster_rcnn_amd.heads import ResnetHead  # noqa: E402
from replication_faster_rcnn_amd.rpn import RPN  # noqa: E402
from replication_faster_rcnn_amd.train import Trainer  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
dtypes = pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])


def bits(t):
    """A tensor's bit patterns as integers (int16 for the 16-bit types, int32 for fp32)."""
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.contiguous().view(torch.int16)
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    return t


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------ epilogue
# one bit pattern of each kind per type: +-0, +-inf, two NaNs with payloads, the largest and the
# smallest subnormal, the largest finite value and its negative
SPECIALS = {
    torch.float16: [0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E01, 0xFD55, 0x0001, 0x83FF, 0x7BFF, 0xFBFF],
    torch.bfloat16: [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC1, 0xFFAA, 0x0001, 0x807F, 0x7F7F, 0xFF7F],
}
EPI_SHAPES = [(1, 1, 1, 1), (2, 9, 5, 13), (2, 9, 38, 38), (1, 32, 3, 7), (0, 9, 4, 4), (2, 9, 0, 5)]


def plant(t, dtype, seed):
    """Scatter the special bit patterns over t (in place, through the int16 view), every one of
    them inside channels 0 and 1 of some pixel too (for cls: one softmax pair)."""
    flat = t.view(torch.int16).view(-1)
    n = flat.numel()
    if n == 0:
        return t
    sp = torch.tensor(SPECIALS[dtype], dtype=torch.int32).to(torch.int16)
    g = torch.Generator().manual_seed(seed)
    where = torch.randperm(n, generator=g)[:min(n, 4 * len(sp))]
    flat[where] = sp.repeat(4)[:len(where)]
    N, C, H, W = t.shape
    v = t.view(torch.int16)
    for i, s in enumerate(sp):     # the pair (2k, 2k+1) of anchor k = 0 at pixel i: special in one slot
        nn_, p = (i // (H * W)) % N, i % (H * W)
        v[nn_, i % 2, p // W, p % W] = s
    return t


def epilogue_inputs(shape, dtype):
    N, K, H, W = shape
    g = torch.Generator().manual_seed(N * 1000 + K * 100 + H * 10 + W)
    cls = plant((torch.randn(N, 2 * K, H, W, generator=g) * 3).to(dtype), dtype, 1)
    reg = plant(torch.randn(N, 4 * K, H, W, generator=g).to(dtype), dtype, 2)
    return cls.cuda(), reg.cuda()


@dtypes
@pytest.mark.parametrize("shape", EPI_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_epilogue_forward_and_backward(shape, dtype):
    N, K, H, W = shape
    A = H * W * K
    cls, reg = epilogue_inputs(shape, dtype)
    if cls.numel() >= 20:
        cb = bits(cls).view(-1).tolist()
        assert all(((s + 0x8000) % 0x10000) - 0x8000 in cb for s in SPECIALS[dtype])
    cls.requires_grad_(True)
    reg.requires_grad_(True)
    c, fg, r, deltas = ops.rpn_head_epilogue_with_deltas(cls, reg, K)
    assert c.dtype == dtype and r.dtype == dtype and fg.dtype == torch.float32 and deltas.dtype == torch.float32
    assert c.shape == (N, A, 2) and r.shape == (N, A, 4) and fg.shape == (N, A) and deltas.shape == (N, A, 4)
    assert not fg.requires_grad and not deltas.requires_grad and c.requires_grad and r.requires_grad
    # permuted copies: the inputs' bit patterns, NaN payloads and signed zeros included
    assert torch.equal(bits(c), bits(cls.detach()).permute(0, 2, 3, 1).reshape(N, A, 2))
    assert torch.equal(bits(r), bits(reg.detach()).permute(0, 2, 3, 1).reshape(N, A, 4))
    # fp32 outputs: the fp32 op on the widened inputs
    c32, fg32, r32 = ops.rpn_head_epilogue(cls.detach().float(), reg.detach().float(), K)
    assert c32.dtype == torch.float32
    assert same_bits(fg, fg32) and same_bits(deltas, r32)
    # backward: the inverse permute of a 16-bit upstream gradient, bit for bit, in the 16-bit type
    g = torch.Generator().manual_seed(5)
    gc = plant(torch.randn(N, 2 * K, H, W, generator=g).to(dtype), dtype, 3).cuda()
    gr = plant(torch.randn(N, 4 * K, H, W, generator=g).to(dtype), dtype, 4).cuda()
    up_c = gc.permute(0, 2, 3, 1).reshape(N, A, 2).contiguous()
    up_r = gr.permute(0, 2, 3, 1).reshape(N, A, 4).contiguous()
    torch.autograd.backward([c, r], [up_c, up_r])
    assert same_bits(cls.grad, gc) and same_bits(reg.grad, gr)


@dtypes
def test_epilogue_strip_of_128_gives_the_same_bits(dtype):
    from replication_faster_rcnn_amd import _lib
    cls, reg = epilogue_inputs((2, 9, 15, 13), dtype)      # 195 pixels: strips of 64 + 64 + 64 + 3 or 128 + 67
    want = ops.rpn_head_epilogue_with_deltas(cls, reg, 9)
    with _lib.kernel_path("rpn_epilogue_strip", "128"):
        got = ops.rpn_head_epilogue_with_deltas(cls, reg, 9)
    for a, b in zip(got, want):
        assert same_bits(a, b)


@dtypes
def test_epilogue_unaligned_views(dtype):
    """Inputs and outputs that are only 2-byte aligned (possible through the C-ABI alone): the narrow
    loads and the head / tail stores give the same bits, and nothing outside the outputs is written."""
    from replication_faster_rcnn_amd import _lib
    lib = _lib.load()
    N, K, H, W = 2, 9, 6, 11
    A = H * W * K
    cls, reg = epilogue_inputs((N, K, H, W), dtype)
    want = ops.rpn_head_epilogue_with_deltas(cls, reg, K)
    pad = lambda t: torch.cat([t.new_zeros(1), t.reshape(-1), t.new_zeros(1)])   # noqa: E731
    cls1, reg1 = pad(cls), pad(reg)                          # the data starts at element 1
    one = torch.ones((), dtype=dtype, device="cuda")
    oc = one.repeat(N * A * 2 + 2)
    orr = one.repeat(N * A * 4 + 2)
    fg = torch.full((N * A + 2,), 7.0, device="cuda")
    de = torch.full((N * A * 4 + 2,), 7.0, device="cuda")
    _lib.check(lib.frcnn_rpn_head_epilogue_t(_lib.DTYPE_CODES[dtype], cls1.data_ptr() + 2, reg1.data_ptr() + 2, N, K, H,
                                             W, oc.data_ptr() + 2, fg.data_ptr() + 4, orr.data_ptr() + 2,
                                             de.data_ptr() + 4, _lib.stream_ptr()), "epilogue")
    assert torch.equal(bits(oc[1:-1]), bits(want[0]).view(-1)) and torch.equal(bits(orr[1:-1]), bits(want[2]).view(-1))
    assert torch.equal(bits(fg[1:-1]), bits(want[1]).view(-1)) and torch.equal(bits(de[1:-1]), bits(want[3]).view(-1))
    for t, v in ((oc, 1.0), (orr, 1.0), (fg, 7.0), (de, 7.0)):
        assert float(t[0]) == v and float(t[-1]) == v


@dtypes
def test_epilogue_three_outputs_and_dtype_rule(dtype):
    cls, reg = epilogue_inputs((2, 9, 5, 13), dtype)
    out = ops.rpn_head_epilogue(cls, reg, 9)
    assert len(out) == 3 and out[0].dtype == dtype and out[1].dtype == torch.float32 and out[2].dtype == dtype
    four = ops.rpn_head_epilogue_with_deltas(cls, reg, 9)
    for a, b in zip(out, four):
        assert same_bits(a, b)
    # fp32 inputs: deltas is reg_nhwc itself
    f = ops.rpn_head_epilogue_with_deltas(cls.float(), reg.float(), 9)
    assert f[3].dtype == torch.float32 and f[3].data_ptr() == f[2].data_ptr() and not f[3].requires_grad
    other = torch.bfloat16 if dtype == torch.float16 else torch.float16
    for c, r in ((cls, reg.float()), (cls.float(), reg), (cls, reg.to(other)), (cls.double(), reg)):
        with pytest.raises(RuntimeError, match="rpn_head_epilogue: reg is"):
            ops.rpn_head_epilogue(c, r, 9)


# -------------------------------------------------------------------- losses
GRADS = [(1.0, 1.0), (2.0, 0.5), (1.0, None), (None, 1.0)]
_ref_cache = {}


def loss_tensors(case, dtype, widen):
    """The case's inputs on the device with cls / reg rounded to dtype (and widened back to fp32
    with ``widen``: the fp32 op's inputs), both requiring grad."""
    cls = torch.from_numpy(case.cls).cuda().to(dtype)
    reg = torch.from_numpy(case.reg).cuda().to(dtype)
    if widen:
        cls, reg = cls.float(), reg.float()
    return (cls.requires_grad_(True), reg.requires_grad_(True), torch.from_numpy(case.reg_t).cuda(),
            torch.from_numpy(case.labels).cuda())


def run_losses(case, dtype, g, widen=False, permuted=False):
    cls, reg, reg_t, lab = loss_tensors(case, dtype, widen)
    cl, rl, stats = ops.losses_with_stats(cls.permute(0, 2, 1) if permuted else cls, reg, reg_t, lab,
                                          sigma=case.sigma, head=case.head)
    assert cl.dtype == torch.float32 and rl.dtype == torch.float32 and cl.shape == () and stats.dtype == torch.int32
    sum(w * t for w, t in zip(g, (cl, rl)) if w is not None).backward()
    return dict(loss=torch.stack([cl.detach(), rl.detach()]), stats=stats, dcls=cls.grad, dreg=reg.grad)


def widened_reference(case, dtype, g):
    """loss_ref.stage on the rounded and widened predictions, computed once."""
    key = (case.name, dtype, g)
    if key not in _ref_cache:
        r = case.rows
        cls = torch.from_numpy(case.cls).to(dtype).float().numpy().reshape(r, case.C)
        reg = torch.from_numpy(case.reg).to(dtype).float().numpy().reshape(r, case.reg.shape[2])
        _ref_cache[key] = loss_ref.stage(cls, reg, case.reg_t.reshape(r, 4), case.labels.reshape(r), sigma=case.sigma,
                                         head=case.head, g_cls=g[0], g_reg=g[1])
    return _ref_cache[key]


def assert_t_equals_widened_fp32(got, want, dtype, what):
    """The 16-bit op against the fp32 op on the widened inputs: losses and stats bit-equal, the
    gradients in dtype with the bits of the fp32 gradients rounded once."""
    assert same_bits(got["loss"], want["loss"]), (what, got["loss"], want["loss"])
    assert torch.equal(got["stats"], want["stats"]), what
    for k in ("dcls", "dreg"):
        assert got[k].dtype == dtype and want[k].dtype == torch.float32, (what, k)
        assert same_bits(got[k], want[k].to(dtype)), (what, k)


def assert_matches_ref(got, ref, C, g, dtype, what):
    """test_gpu_losses.assert_matches' rules, each gradient bound enlarged by the one rounding to
    dtype: half an ulp of the reference value, 2^-11 |ref| (float16, 11 significand bits) or 2^-8
    |ref| (bfloat16, 8), and in the subnormal range half the type's smallest subnormal.  Derived
    from the formats, not measured.  Zeros: where the reference is exactly zero (unlabelled rows,
    other classes' columns, an unused loss) the gradient is exactly zero; a nonzero reference value
    may round to zero only below that bound, which the error bound itself checks."""
    assert np.array_equal(got["stats"].cpu().numpy(), ref["stats"]), (what, got["stats"], ref["stats"])
    np.testing.assert_allclose(got["loss"].cpu().numpy(), ref["loss"], rtol=1e-5, atol=1e-7, equal_nan=True,
                               err_msg=what)
    bc, br = loss_ref.grad_bounds(C, int(ref["stats"][0]), int(ref["stats"][1]), g[0], g[1])
    rel = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
    half_sub = 0.5 * (2.0 ** -24 if dtype == torch.float16 else 2.0 ** -133)
    for k, bound in (("dcls", bc), ("dreg", br)):
        gk = got[k].float().cpu().numpy().reshape(ref[k].shape).astype(np.float64)
        rk = ref[k].astype(np.float64)
        assert np.isfinite(gk).all(), (what, k)
        assert not gk[rk == 0].any(), (what, k, "zero pattern")
        err = np.abs(gk - rk)
        lim = bound + rel * np.abs(rk) + half_sub
        print(f"{what}: max |d {k}| = {err.max() if err.size else 0.0:.3e} "
              f"(largest bound {lim.max() if lim.size else 0.0:.3e})")
        assert (err <= lim).all(), (what, k, float((err - lim).max()))


@dtypes
@pytest.mark.parametrize("case", loss_cases.CASES, ids=lambda c: c.name)
def test_loss_case(case, dtype):
    g = (1.0, 1.0)
    got = run_losses(case, dtype, g)
    assert_t_equals_widened_fp32(got, run_losses(case, dtype, g, widen=True), dtype, case.name)
    src = case.clean if case.clean is not None else case
    assert_matches_ref(got, widened_reference(src, dtype, g), case.C, g, dtype, case.name)
    if case.clean is not None:      # garbage in unlabelled rows: the clean twin's outputs, to the bit
        clean = run_losses(case.clean, dtype, g)
        for k in got:
            assert same_bits(got[k], clean[k]), (case.name, k)


@dtypes
@pytest.mark.parametrize("g", GRADS[1:], ids=str)
@pytest.mark.parametrize("name", ["rpn_rows_65", "rpn_rows_257", "head_3x5_c21", "head_c21_two_tiles",
                                  "head_label_0_and_last_c128", "sl1_threshold_sigma3", loss_cases.MULTI_WORKGROUP])
def test_loss_upstream_gradients(name, g, dtype):
    case = loss_cases.BY_NAME[name]
    got = run_losses(case, dtype, g)
    assert_t_equals_widened_fp32(got, run_losses(case, dtype, g, widen=True), dtype, name)
    assert_matches_ref(got, widened_reference(case, dtype, g), case.C, g, dtype, f"{name} {g}")
    if g[0] is None:
        assert not bits(got["dcls"]).any()            # all +0
    if g[1] is None:
        assert not bits(got["dreg"]).any()


@dtypes
@pytest.mark.parametrize("name", ["rpn_f64_labels_2x100", "head_3x5_c21"])
def test_loss_permuted_view(name, dtype):
    case = loss_cases.BY_NAME[name]
    g = (2.0, 0.5)
    got, plain = run_losses(case, dtype, g, permuted=True), run_losses(case, dtype, g)
    for k in got:
        assert same_bits(got[k], plain[k]), k
    cls, reg, reg_t, lab = loss_tensors(case, dtype, False)
    view = cls.permute(0, 2, 1)
    seen = []
    view.register_hook(seen.append)                   # the gradient as the op's backward hands it over
    cl, _ = (ops.head_losses if case.head else ops.rpn_losses)(view, reg, reg_t, lab)
    cl.backward()
    N, L, C = case.cls.shape
    assert len(seen) == 1 and seen[0].dtype == dtype and seen[0].shape == (N, C, L)
    assert seen[0].stride() == view.stride() and same_bits(seen[0].permute(0, 2, 1), cls.grad)


def test_loss_scaled_upstream_gradient():
    """A GradScaler's 65536 as the upstream gradient: the float16 gradients are the fp32 op's
    .to(float16), +-inf where those overflow (one labelled row: |dreg| = 65536 > 65504); bfloat16
    has fp32's range and stays finite."""
    g = (65536.0, 65536.0)
    for name in ("rpn_rows_1", "head_c21_two_tiles"):
        case = loss_cases.BY_NAME[name]
        for dtype in DTYPES:
            got = run_losses(case, dtype, g)
            want = run_losses(case, dtype, g, widen=True)
            assert torch.isfinite(want["dcls"]).all() and torch.isfinite(want["dreg"]).all()
            assert_t_equals_widened_fp32(got, want, dtype, f"{name} {dtype}")
            if dtype == torch.bfloat16 or name != "rpn_rows_1":
                assert torch.isfinite(got["dcls"].float()).all() and torch.isfinite(got["dreg"].float()).all()
            else:
                assert torch.isinf(got["dreg"].float()).any()


@dtypes
def test_loss_deterministic_on_several_workgroups(dtype):
    case = loss_cases.BY_NAME[loss_cases.MULTI_WORKGROUP]
    a, b = run_losses(case, dtype, (2.0, 0.5)), run_losses(case, dtype, (2.0, 0.5))
    for k in a:
        assert bits(a[k]).cpu().numpy().tobytes() == bits(b[k]).cpu().numpy().tobytes(), k


@dtypes
@pytest.mark.parametrize("name", ["rpn_f64_labels_2x100", "head_c21_two_tiles"])
def test_loss_no_host_synchronisation(name, dtype):
    case = loss_cases.BY_NAME[name]
    cls, reg, reg_t, lab = loss_tensors(case, dtype, False)
    op = ops.head_losses if case.head else ops.rpn_losses
    view = cls.permute(0, 2, 1)
    op(view.detach(), reg.detach(), reg_t, lab, sigma=case.sigma)        # workspace and library loaded
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        cl, rl = op(view, reg, reg_t, lab, sigma=case.sigma)
        (2 * cl + 0.5 * rl).backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    want = run_losses(case, dtype, (2.0, 0.5))
    assert same_bits(torch.stack([cl.detach(), rl.detach()]), want["loss"])
    assert same_bits(cls.grad, want["dcls"]) and same_bits(reg.grad, want["dreg"])


@dtypes
def test_loss_input_rule(dtype):
    case = loss_cases.BY_NAME["head_3x5_c21"]
    cls, reg, reg_t, lab = (t.detach() for t in loss_tensors(case, dtype, False))
    ops.head_losses(cls, reg, reg_t, lab)
    other = torch.bfloat16 if dtype == torch.float16 else torch.float16
    with pytest.raises(RuntimeError, match="head_losses: reg "):
        ops.head_losses(cls, reg.float(), reg_t, lab)
    with pytest.raises(RuntimeError, match="head_losses: reg "):
        ops.head_losses(cls, reg.to(other), reg_t, lab)
    with pytest.raises(RuntimeError, match="head_losses: reg "):
        ops.head_losses(cls.float(), reg, reg_t, lab)
    with pytest.raises(RuntimeError, match="head_losses: cls "):
        ops.head_losses(cls.double(), reg.double(), reg_t, lab)
    with pytest.raises(RuntimeError, match="head_losses: cls "):
        ops.head_losses(cls.cpu(), reg, reg_t, lab)
    with pytest.raises(RuntimeError, match="head_losses: reg "):
        ops.head_losses(cls, reg.cpu(), reg_t, lab)


# -------------------------------------------------------------------- detect
H, W = 600, 1000
NAMES = ("boxes", "labels", "scores", "roi", "count", "total")


def rounded(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def check_detect(rois, rc, cls, reg, dtype, thr, **kw):
    """ops.detect on cls / reg rounded to dtype against the fp32 op and tests/detect_ref.detect on the
    widened values; returns the reference's outputs and the widened logits."""
    c16, r16 = rounded(cls, dtype).cuda(), rounded(reg, dtype).cuda()
    rois_d, rc_d = torch.from_numpy(np.ascontiguousarray(rois)).cuda(), torch.from_numpy(rc).cuda()
    got = ops.detect(rois_d, rc_d, c16, r16, img_h=H, img_w=W, score_thresh=thr, **kw)
    f32 = ops.detect(rois_d, rc_d, c16.float(), r16.float(), img_h=H, img_w=W, score_thresh=thr, **kw)
    cw, rw = c16.float().cpu().numpy(), r16.float().cpu().numpy()
    want = detect_ref.detect(rois, rc, cw, rw, H, W, score_thresh=thr, **kw)
    for name, g, f, w in zip(NAMES, got, f32, want):
        assert same_bits(g, f), f"det_{name} differs from the fp32 op"
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), f"det_{name} differs from detect_ref"
    return want, cw


@dtypes
@pytest.mark.parametrize("thr", [0.05, 0.7])
def test_detect_golden_inputs(golden, thr, dtype):
    g = golden("detect_small.npz")
    want, _ = check_detect(g["rois"], g["rcount"], g["cls"], g["reg"], dtype, thr)
    assert want[5].max() >= 1


@dtypes
def test_detect_mixed_with_tied_scores(dtype):
    """The random case of test_gpu_detect.test_mixed, with pairs of rows that differ in fp32 and
    coincide once rounded: their scores tie exactly in every class, and the order by (score, row)
    decides between them."""
    rois, rc, cls, reg = (a.copy() for a in synth.head_outputs(3, 300, 21, H, W, seed=2))
    pairs = []
    for n in range(3):
        v = rounded(cls[n], dtype).float().numpy()
        b = int(np.nonzero(detect_ref.softmax(v)[:, 1:].max(axis=1) > 0.5)[0][0])   # a confident foreground row
        a = 299 - n
        assert a != b
        # a 16-bit value's neighbours are at least 2^-11 |v| (float16) or 2^-8 |v| (bfloat16) away:
        # v (1 + 2^-13) is another fp32 number that rounds back to v
        cls[n, a] = v[b] * np.float32(1 + 2.0 ** -13)
        assert not np.array_equal(cls[n, a], v[b]) and np.array_equal(rounded(cls[n, a], dtype).float().numpy(), v[b])
        cls[n, b] = v[b]
        # image 0: the same box (the lower row suppresses the higher); the others: disjoint boxes
        rois[n, a] = rois[n, b] if n == 0 else np.float32([0, 0, 20, 20])
        reg[n, a] = reg[n, b] if n == 0 else 0.0
        if n:                                          # two small boxes in opposite corners, away from the objects
            rois[n, b], reg[n, b] = np.float32([580, 980, 600, 1000]), 0.0
        pairs.append((a, b))
    want, cw = check_detect(rois, rc, cls, reg, dtype, 0.05)
    ties = 0
    for n in range(3):
        p = detect_ref.softmax(cw[n])
        for c in range(1, 21):
            cand = p[:, c][p[:, c] > 0.05]
            ties += len(cand) - len(np.unique(cand))
    assert ties >= 3, ties                             # candidates with exactly equal scores exist
    assert want[5].max() > 300                         # an image keeps more than R
    for n, (a, b) in enumerate(pairs):
        c = 1 + int(np.argmax(detect_ref.softmax(cw[n, b:b + 1])[0, 1:]))
        rows = list(want[3][n][want[1][n] == c])
        if n == 0:
            assert a not in rows
        else:                                          # both kept (nothing overlaps either), the lower row first
            assert a in rows and b in rows and rows.index(a) == rows.index(b) + 1 and b < a


@dtypes
def test_detect_small_shapes(dtype):
    one = synth.head_outputs(1, 1, 21, H, W, seed=5)                 # R = 1
    want, _ = check_detect(*one, dtype, 0.0)
    assert want[5][0] == 20
    two = synth.head_outputs(2, 77, 2, H, W, seed=3, objects=3)      # C = 2
    want, _ = check_detect(*two, dtype, 0.05)
    assert (want[5] >= 2).all()
    rois, _, cls, reg = (a.copy() for a in synth.head_outputs(3, 128, 21, H, W, seed=6))
    rc = np.array([0, 37, 128], np.int32)                            # an image without RoIs
    for n in range(3):
        cls[n, rc[n]:] = 50.0
        reg[n, rc[n]:] = 1e30                                         # +inf in float16: never read
    want, _ = check_detect(rois, rc, cls, reg, dtype, 0.05)
    assert want[4][0] == 0 and want[4][1] > 0
    got = check_detect(rois, rc, cls, reg, dtype, 0.05, max_det=50)[0]
    assert got[4].max() == 50


@dtypes
def test_detect_input_rule(dtype):
    rois, rc, cls, reg = synth.head_outputs(2, 77, 2, H, W, seed=3, objects=3)
    rois, rc = torch.from_numpy(rois).cuda(), torch.from_numpy(rc).cuda()
    c16, r16 = rounded(cls, dtype).cuda(), rounded(reg, dtype).cuda()
    kw = dict(img_h=H, img_w=W)
    ops.detect(rois, rc, c16, r16, **kw)
    other = torch.bfloat16 if dtype == torch.float16 else torch.float16
    for c, r, name in ((c16, r16.float(), "reg"), (c16.float(), r16, "reg"), (c16, r16.to(other), "reg"),
                       (c16.double(), r16, "cls"), (c16, r16.double(), "reg"), (c16.cpu(), r16, "cls"),
                       (c16, r16.cpu(), "reg")):
        with pytest.raises(RuntimeError, match=f"detect: {name} "):
            ops.detect(rois, rc, c, r, **kw)
    with pytest.raises(RuntimeError, match="detect: rois "):
        ops.detect(rois.to(dtype), rc, c16, r16, **kw)


# ---------------------------------------------------------------- end to end
IMG_H, IMG_W, FH, FW, CF = 96, 112, 6, 7, 16


def small_rpn(mode):
    rpn = RPN(in_channels=CF, mid_channels=CF, anchor_scales=[1, 2, 4], mode=mode)
    rpn.proposal_layer.pre_nms, rpn.proposal_layer.post_nms = 200, 48
    with torch.no_grad():
        rpn.reg.weight.normal_(0, 0.5)       # spread the proposals
        rpn.cls.weight.normal_(0, 0.5)
    return rpn.cuda()


def features(n):
    return torch.from_numpy(np.stack([synth.features(CF, FH, FW, 9, i) for i in range(n)])).cuda()


@dtypes
def test_rpn_forward_under_autocast(dtype):
    torch.manual_seed(3)
    rpn = small_rpn("training")
    x = features(2)
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        rpn(x, IMG_W, IMG_H)                                   # the convolutions pick their algorithms
        cls, reg, rois, roi_inds, _ = rpn(x, IMG_W, IMG_H)
        h = F.relu(rpn.conv1(x))
        conv_c, conv_r = rpn.cls(h), rpn.reg(h)
    A = FH * FW * rpn.K
    assert conv_c.dtype == dtype and cls.dtype == dtype and reg.dtype == dtype
    assert cls.shape == (2, 2, A) and reg.shape == (2, A, 4)
    assert rois.dtype == torch.float32 and rpn.fg_scores.dtype == torch.float32
    assert rpn.rois_padded.dtype == torch.float32
    # the fp32 route on the widened conv outputs: the same proposals, to the bit
    c32, fg32, r32 = ops.rpn_head_epilogue(conv_c.float(), conv_r.float(), rpn.K)
    assert same_bits(rpn.fg_scores, fg32)
    assert torch.equal(bits(cls.permute(0, 2, 1)), bits(c32.to(dtype))) and torch.equal(bits(reg), bits(r32.to(dtype)))
    pl = rpn.proposal_layer
    want, _, cnt = ops.propose(fg32, r32, img_w=IMG_W, img_h=IMG_H, pre_nms=pl.pre_nms, post_nms=pl.post_nms,
                               nms_thresh=pl.nms_threshold, min_size=pl.min_size, anchor_base=rpn._base_dev,
                               feat_h=FH, feat_w=FW, feat_stride=rpn.feat_stride)
    counts = cnt.tolist()
    assert min(counts) >= 8 and torch.equal(cnt, rpn.rois_count)
    for i, k in enumerate(counts):
        assert same_bits(rpn.rois_padded[i, :k], want[i, :k])
    assert same_bits(rois, torch.cat([want[i, :k] for i, k in enumerate(counts)]))


@dtypes
def test_fused_training_step_under_autocast(dtype, rng_guard):
    torch.manual_seed(4)
    rpn = small_rpn("training")
    head = ResnetHead(nn.Sequential(nn.Conv2d(CF, 512, 1), nn.AdaptiveAvgPool2d(1))).cuda()
    params = list(rpn.parameters()) + list(head.parameters())
    opt = torch.optim.SGD(params, lr=0.0)
    scaler = torch.amp.GradScaler()
    bl = [synth.gt_boxes(IMG_H, IMG_W, 8, 9, i, n_valid=[5, 3][i]) for i in range(2)]
    boxes, labels = np.stack([b for b, _ in bl]), np.stack([l for _, l in bl])
    x = features(2).requires_grad_(True)
    tr = Trainer(rpn, head, n_sample=(32, 16), fused_losses=True, grad_scaler=scaler)
    np.random.seed(11)
    with torch.autocast("cuda", dtype=dtype):
        losses = tr.train_step(x, IMG_H, IMG_W, boxes, labels)
    L = tr.last
    for k in ("cls", "reg", "cls_output", "reg_output"):
        assert L[k].dtype == dtype, k
    assert L["reg_output"].shape == (2, 16, 4 * 21)
    # the four losses: the fp32 ops on the widened predictions of that very step
    rc, rr = ops.rpn_losses(L["cls"].detach().float(), L["reg"].detach().float(), L["rpn_reg_targets"], L["rpn_labels"])
    hc, hr = ops.head_losses(L["cls_output"].detach().float(), L["reg_output"].detach().float(), L["sample_reg"],
                             L["sample_labels"])
    for k, v in (("rpn_cls", rc), ("rpn_reg", rr), ("cls", hc), ("reg", hr)):
        assert losses[k].dtype == torch.float32 and same_bits(losses[k], v), (k, losses[k], v)
        assert torch.isfinite(v), k
    scaler.unscale_(opt)
    for p in params:
        assert p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all()
    assert sum(float(p.grad.abs().sum()) for p in params) > 0
    assert x.grad is not None and torch.isfinite(x.grad).all()
    # with an optimizer the scaler steps and updates it
    tr2 = Trainer(rpn, head, n_sample=(32, 16), optimizer=opt, fused_losses=True, grad_scaler=torch.amp.GradScaler())
    np.random.seed(11)
    with torch.autocast("cuda", dtype=dtype):
        again = tr2.train_step(features(2), IMG_H, IMG_W, boxes, labels)
    assert torch.isfinite(again["total"])


@dtypes
def test_predict_under_autocast(dtype):
    from replication_faster_rcnn_amd.faster_rcnn import FasterRCNN
    torch.manual_seed(3)

    def backbone():
        return nn.Conv2d(3, CF, 1), nn.Sequential(nn.Conv2d(CF, 512, 1), nn.AdaptiveAvgPool2d(1))

    model = FasterRCNN(backbone, lambda **kw: RPN(in_channels=CF, mid_channels=CF, **kw),
                       lambda classifier: ResnetHead(classifier), "test").cuda()
    with torch.no_grad():
        model.head.cls.weight.mul_(40)        # spread the logits: some classes pass the threshold
        model.head.reg.weight.mul_(4)
        model.rpn.reg.weight.normal_(0, 3)
    x = torch.randn(2, 3, 10, 10).cuda()
    with torch.autocast("cuda", dtype=dtype):
        dets = model.predict(x, 160, 160, score_thresh=0.05)
    cls, reg = model.last_head_outputs
    assert cls.dtype == dtype and reg.dtype == dtype and cls.shape == (2, 300, 21) and reg.shape == (2, 300, 84)
    want = ops.detect(model.rpn.rois_padded, model.rpn.rois_count, cls.float(), reg.float(), img_h=160, img_w=160,
                      score_thresh=0.05)
    for g, w in zip(model.last_detections, want):
        assert same_bits(g, w)
    counts = want[4].tolist()
    assert min(counts) >= 1
    for n, (b, l, s) in enumerate(dets):
        k = counts[n]
        assert same_bits(b, want[0][n, :k]) and torch.equal(l, want[1][n, :k]) and same_bits(s, want[2][n, :k])
