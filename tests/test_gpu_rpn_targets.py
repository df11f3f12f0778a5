"""``ops.rpn_targets_multilevel`` / ``ops.rpn_losses_multilevel`` / ``rpn.MultiLevelRPNTraining`` on
the HIP path against tests/rpn_targets_ref.py, on every named case of tests/rpn_targets_cases.py
(DESIGN.md §3 "Pyramid RPN training").  Needs an MI355X.

The six target outputs are compared as bits.  Every case runs twice, the second time into pre-filled
caller-owned outputs with the workspace filled with 0xFF, and names the launch plan it reached before
anything is compared.

Gradient bound (DESIGN.md states the derivation): a box gradient is three IEEE operations on bit-equal
inputs, so it is exact; an objectness gradient may differ by 3 * 2^-23 * |g_obj / S|, from the one
place the two sides can differ, the fp64 exp under the correctly rounded fp32 exp; a 16-bit gradient
adds one spacing of its format.  Measured: 0 everywhere."""
import numpy as np
import pytest
import torch

import rpn_targets_cases as rc
import rpn_targets_ref as ref
from replication_faster_rcnn_amd import ops
from replication_faster_rcnn_amd.rpn import MultiLevelRPNTraining

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ops.RPNTargets._fields
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
MANT = {torch.float16: 10, torch.bfloat16: 7}


def state(seed, calls):
    return torch.tensor([seed, calls], dtype=torch.int64).to(DEV)


def device_inputs(case):
    return (torch.from_numpy(case.gt_boxes).to(DEV), torch.from_numpy(case.gt_count).to(DEV),
            [b.to(DEV) for b in case.bases])


def call(case, rng, **kw):
    gt, cnt, bases = device_inputs(case)
    return ops.rpn_targets_multilevel(gt, cnt, bases, case.strides, case.grids, rng, _key_bits=case.key_bits,
                                      **{**case.kw, **kw})


def assert_bits(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu().numpy()
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        bad = g.view(np.uint32) != np.ascontiguousarray(w).view(np.uint32)
        assert not bad.any(), (f"{what}: {name}: {int(bad.sum())} of {bad.size} elements differ in their bits; first at "
                               f"{np.argwhere(bad)[0].tolist()}: {g[bad][0]!r} != {w[bad][0]!r}")


def device_targets(case):
    return ops.RPNTargets(*[torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in case.reference()])


@pytest.mark.parametrize("case", rc.CASES, ids=repr)
def test_case(case):
    want = case.reference()
    if case.check is not None:
        case.check(case, want)
    name = ops.rpn_targets_multilevel_kernel(case.K, case.grids, case.N, case.G, case.B, case.key_bits)
    for part in case.plan:
        assert part in name, (part, name)
    rng = state(case.seed, case.calls)
    got = call(case, rng)
    assert_bits(got, want, case.name)
    assert rng.cpu().tolist() == [case.seed, case.calls + 1]
    # again, into caller-owned outputs (pre-filled: every element must be stored) with a dirty workspace
    N, A, B = case.N, case.A, case.B
    outs = (torch.full((N, A), 7, dtype=torch.int32, device=DEV), torch.full((N, A), 7, dtype=torch.int32, device=DEV),
            torch.full((N, B), 7, dtype=torch.int32, device=DEV), torch.full((N,), 7, dtype=torch.int32, device=DEV),
            torch.full((N,), 7, dtype=torch.int32, device=DEV), torch.full((N, B, 4), 7.0, device=DEV))
    need = max(v[-1] for k, v in ops._rpnt_cache.items() if k[3:] == (N, case.G, B) and k[0] == case.K)
    ws = torch.full((need + 512,), 0xFF, dtype=torch.uint8, device=DEV)
    ws = ws[(-ws.data_ptr()) % 256:][:need]
    again = call(case, state(case.seed, case.calls), out=outs, workspace=ws)
    assert all(a is b for a, b in zip(again, outs))
    assert_bits(again, want, f"{case.name} (caller-owned outputs, 0xFF workspace)")


def test_second_call_draws_a_fresh_sample():
    case = rc.BY_NAME["layout"]
    rng = ops.sampler_state(case.seed, DEV)
    first = call(case, rng)
    second = call(case, rng)
    assert rng.cpu().tolist() == [case.seed, 2]
    assert_bits(first, case.reference(0), "calls = 0")
    assert_bits(second, case.reference(1), "calls = 1")
    assert not torch.equal(first.samples, second.samples)
    assert torch.equal(first.matches, second.matches)


def widened(tensors):
    return [t.float().numpy() for t in tensors]


def grad_check(got, want, scale, dtype, zero_exact_only, what):
    g = got.float().cpu().numpy()
    w = want if dtype == torch.float32 else torch.from_numpy(want).to(dtype).float().numpy()
    assert np.array_equal(g != 0, w != 0), f"{what}: the zero pattern differs"
    assert not np.signbit(g[g == 0]).any(), f"{what}: a -0 off the samples"
    tol = 0.0 if zero_exact_only else 3 * 2.0 ** -23 * abs(scale)
    bound = np.full(w.shape, tol)
    if dtype != torch.float32:
        bound += np.maximum(np.abs(w) * 2.0 ** -MANT[dtype], 2.0 ** -24 if dtype == torch.float16 else 0.0) * (tol > 0)
    diff = np.abs(g.astype(np.float64) - w.astype(np.float64))
    print(f"{what}: largest difference {diff.max():.3g} (bound {bound.max():.3g})")
    assert (diff <= bound).all(), (what, diff.max())
    return diff.max()


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", rc.LOSS_CASES)
def test_losses(name, dtype):
    case, dt = rc.BY_NAME[name], DTYPES[dtype]
    tg = device_targets(case)
    obj, dl = rc.head_outputs(case, dt)
    lo, lb, dobj, ddel, S = ref.losses(widened(obj), widened(dl), case.reference(), case.K, case.grids,
                                       g_obj=0.75, g_box=1.5)

    def run(cast=None):
        o = [(t if cast is None else t.to(cast)).to(DEV).requires_grad_(True) for t in obj]
        d = [(t if cast is None else t.to(cast)).to(DEV).requires_grad_(True) for t in dl]
        a, b = ops.rpn_losses_multilevel(o, d, tg)
        (0.75 * a + 1.5 * b).backward()
        return a.detach(), b.detach(), [t.grad for t in o], [t.grad for t in d]

    a, b, go, gd = run()
    assert a.dtype == b.dtype == torch.float32 and a.dim() == b.dim() == 0
    if S == 0:
        assert torch.isnan(a) and torch.isnan(b)
    else:
        print(f"{name} {dtype}: losses {a.item()!r} {b.item()!r}, restatement {float(lo)!r} {float(lb)!r}")
        np.testing.assert_allclose(a.item(), lo, rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(b.item(), lb, rtol=1e-5, atol=1e-7)
    for l in range(len(obj)):
        assert go[l].dtype == gd[l].dtype == dt and go[l].shape == obj[l].shape and gd[l].shape == dl[l].shape
        assert go[l].is_contiguous() and gd[l].is_contiguous()
        grad_check(go[l], dobj[l], 0.75 / max(S, 1), dt, False, f"{name} {dtype} dobjectness[{l}]")
        grad_check(gd[l], ddel[l], 1.5 / max(S, 1), dt, True, f"{name} {dtype} ddeltas[{l}]")
    # the same bits on every call
    a2, b2, go2, gd2 = run()
    assert torch.equal(a.view(torch.int32), a2.view(torch.int32)) and torch.equal(b.view(torch.int32), b2.view(torch.int32))
    bits = torch.int32 if dt == torch.float32 else torch.int16
    for x, y in zip(go + gd, go2 + gd2):
        assert torch.equal(x.view(bits), y.view(bits))
    if dt != torch.float32:   # 16-bit inputs are widened exactly: the fp32 op on .float() inputs gives the same losses
        a3, b3, _, _ = run(torch.float32)
        assert torch.equal(a.view(torch.int32), a3.view(torch.int32)) and torch.equal(b.view(torch.int32), b3.view(torch.int32))


def test_an_unused_loss_gives_zeros():
    case = rc.BY_NAME["layout"]
    tg = device_targets(case)
    obj, dl = rc.head_outputs(case)
    o = [t.to(DEV).requires_grad_(True) for t in obj]
    d = [t.to(DEV).requires_grad_(True) for t in dl]
    _, b = ops.rpn_losses_multilevel(o, d, tg)
    b.backward()
    assert all(not t.grad.view(torch.int32).any() for t in o) and any(t.grad.any() for t in d)
    _, _, _, ddel, _ = ref.losses(widened(obj), widened(dl), case.reference(), case.K, case.grids, g_obj=None, g_box=1.0)
    for l in range(len(d)):
        assert np.array_equal(d[l].grad.cpu().numpy().view(np.uint32), ddel[l].view(np.uint32))


def test_no_host_sync():
    case = rc.BY_NAME["layout"]
    gt, cnt, bases = device_inputs(case)
    obj, dl = rc.head_outputs(case)
    o = [t.to(DEV).requires_grad_(True) for t in obj]
    d = [t.to(DEV).requires_grad_(True) for t in dl]
    rng = ops.sampler_state(case.seed, DEV)
    warm = ops.rpn_targets_multilevel(gt, cnt, bases, case.strides, case.grids, rng, **case.kw)   # caches
    a, b = ops.rpn_losses_multilevel(o, d, warm)
    (a + b).backward()
    rng.copy_(state(case.seed, 0))
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = ops.rpn_targets_multilevel(gt, cnt, bases, case.strides, case.grids, rng, **case.kw)
        a, b = ops.rpn_losses_multilevel(o, d, got)
        (a + b).backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert_bits(got, case.reference(), "under sync-debug")
    assert bool(torch.isfinite(a)) and bool(torch.isfinite(b))


def test_refusals():
    case = rc.BY_NAME["layout"]
    gt, cnt, bases = device_inputs(case)
    rng = ops.sampler_state(1, DEV)

    def refused(match, gt=gt, cnt=cnt, bases=bases, st=case.strides, gs=case.grids, rng=rng, **over):
        with pytest.raises(RuntimeError, match=match):
            ops.rpn_targets_multilevel(gt, cnt, bases, st, gs, rng, **over)

    refused("gt_boxes", gt=gt.double())
    refused("gt_boxes", gt=gt.cpu())
    refused("gt_boxes", gt=gt[:, :, :3].contiguous())
    refused("gt_boxes", gt=gt.transpose(0, 1))
    refused("gt_boxes", gt=torch.zeros(2, 257, 4, device=DEV))
    refused("gt_boxes", gt=torch.zeros(2, 0, 4, device=DEV))
    refused("gt_count", cnt=cnt.long())
    refused("gt_count", cnt=cnt[:1])
    refused("rng", rng=rng.int())
    refused("rng", rng=rng.cpu())
    refused("rng", rng=torch.zeros(3, dtype=torch.int64, device=DEV))
    refused(r"anchor_bases\[1\]", bases=[bases[0], bases[1][:2].contiguous(), bases[2]])
    refused(r"anchor_bases\[2\]", bases=[bases[0], bases[1], bases[2].half()])
    refused("anchor_bases", bases=bases[:2])
    refused("strides", st=case.strides[:2])
    refused(r"strides\[1\]", st=[(8, 10), (0, 20), (32, 40)])
    refused(r"grid_sizes\[0\]", gs=[(0, 18), (6, 9), (3, 5)])
    refused(r"grid_sizes\[0\]", gs=[(1 << 12, 1 << 12), (6, 9), (3, 5)])
    refused("batch_size_per_image", batch_size_per_image=0)
    refused("batch_size_per_image", batch_size_per_image=1025)
    refused("positive_fraction", positive_fraction=1.5)
    refused("positive_fraction", positive_fraction=-0.1)
    refused("bg_iou_thresh", fg_iou_thresh=0.3, bg_iou_thresh=0.7)
    refused("_key_bits", _key_bits=33)
    outs = list(ops.rpn_targets_multilevel(gt, cnt, bases, case.strides, case.grids, rng))
    refused(r"out\[0\] \(matches\)", out=[outs[0].long()] + outs[1:])
    refused(r"out\[5\] \(reg_targets\)", out=outs[:5] + [outs[5][:, :-1]])
    refused("six outputs", out=outs[:5])
    refused("workspace", workspace=torch.empty(16, dtype=torch.uint8, device=DEV))
    refused("workspace", workspace=torch.empty(1 << 20, dtype=torch.uint8))

    tg = ops.RPNTargets(*outs)
    obj, dl = rc.head_outputs(case)
    o, d = [t.to(DEV) for t in obj], [t.to(DEV) for t in dl]

    def loss_refused(match, o=o, d=d, tg=tg, **kw):
        with pytest.raises(RuntimeError, match=match):
            ops.rpn_losses_multilevel(o, d, tg, **kw)

    loss_refused(r"deltas\[1\]", d=[d[0], d[1].half(), d[2]])                       # mixed dtypes
    loss_refused(r"objectness\[0\]", o=[o[0].double(), o[1], o[2]])
    loss_refused(r"objectness\[2\]", o=[o[0], o[1], o[2].cpu()])                     # a host tensor
    loss_refused(r"deltas\[0\]", d=[d[0].transpose(2, 3), d[1], d[2]])               # a strided view
    loss_refused(r"deltas\[1\]", d=[d[0], d[1][:, :8].contiguous(), d[2]])           # 4K channels
    loss_refused(r"objectness\[1\]", o=[o[0], o[1][:1].contiguous(), o[2]])          # another N
    loss_refused(r"objectness\[1\]", o=[o[0], o[1][:, :2].contiguous(), o[2]])       # another K
    loss_refused("deltas", d=d[:2])
    loss_refused("targets", tg=tuple(outs))
    loss_refused(r"targets\.sampled", o=o[:2], d=d[:2])                              # another pyramid
    loss_refused(r"targets\.n_pos", tg=tg._replace(n_pos=tg.n_pos.long()))
    loss_refused("beta", beta=float("nan"))
    loss_refused("beta", beta=-1.0)


def test_capi_refusals():
    """The limits at the C-ABI itself: FRCNN_EINVAL with a message naming the argument, before any launch."""
    from replication_faster_rcnn_amd import _lib
    lib = _lib.load()
    I = _lib.I32
    H, W = (I * 1)(4), (I * 1)(4)
    assert lib.frcnn_rpn_targets_multi_workspace_size(1, 1, 3, H, W, 257, 256) == 0 and b"G" in lib.frcnn_last_error()
    assert lib.frcnn_rpn_targets_multi_workspace_size(9, 1, 3, H, W, 4, 256) == 0 and b"n_levels" in lib.frcnn_last_error()
    assert lib.frcnn_rpn_targets_multi_workspace_size(1, 1025, 3, H, W, 4, 256) == 0
    assert lib.frcnn_rpn_targets_multi_workspace_size(1, 1, 33, H, W, 4, 256) == 0
    assert lib.frcnn_rpn_targets_multi_workspace_size(1, 1, 3, H, W, 4, 1025) == 0
    assert b"batch_size_per_image" in lib.frcnn_last_error()
    big = (I * 8)(*[2047] * 8)
    assert lib.frcnn_rpn_targets_multi_workspace_size(8, 1, 4, big, big, 4, 256) > 0          # 8 * 16.76M < 2^31
    buf = _lib.ctypes.create_string_buffer(64)
    assert lib.frcnn_rpn_targets_multi_kernel(1, 1, 3, H, W, 4, 256, 40, buf, 64) == -1
    assert b"key_bits" in lib.frcnn_last_error()
    case = rc.BY_NAME["layout"]
    gt, cnt, bases = device_inputs(case)
    rng = ops.sampler_state(1, DEV)
    outs = ops.rpn_targets_multilevel(gt, cnt, bases, case.strides, case.grids, rng)
    key = [k for k in ops._rpnt_cache if k[3:] == (case.N, case.G, 256) and k[0] == case.K][0]
    Hs, Ws, shs, sws, A, need = ops._rpnt_cache[key]
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    pb = (_lib.P * 3)(*[b.data_ptr() for b in bases])

    def rc_of(frac=0.5, fg=0.7, bg=0.3, ws_bytes=need, kb=32):
        return lib.frcnn_rpn_targets_multi(3, pb, Hs, Ws, shs, sws, case.N, case.K, gt.data_ptr(), cnt.data_ptr(), case.G,
                                           rng.data_ptr(), 256, frac, fg, bg, 1, kb, *[t.data_ptr() for t in outs],
                                           ws.data_ptr(), ws_bytes, None)

    before = rng.cpu().tolist()
    assert rc_of(frac=1.25) == -1 and b"positive_fraction" in lib.frcnn_last_error()
    assert rc_of(fg=0.2) == -1 and b"bg_iou_thresh" in lib.frcnn_last_error()
    assert rc_of(ws_bytes=need - 1) == -1 and b"workspace" in lib.frcnn_last_error()
    assert rc_of(kb=-1) == -1 and b"key_bits" in lib.frcnn_last_error()
    torch.cuda.synchronize()
    assert rng.cpu().tolist() == before                                                      # nothing was launched


def test_module_trains_end_to_end():
    """Head convs -> proposals' inputs -> targets -> losses -> backward: gradients reach the conv weights,
    the module's state advances on the device, and the head's outputs also feed ``propose_multilevel``."""
    case = rc.BY_NAME["layout"]
    torch.manual_seed(0)
    C = 8
    conv = torch.nn.Conv2d(C, C, 3, padding=1).to(DEV)
    cls = torch.nn.Conv2d(C, case.K, 1).to(DEV)
    reg = torch.nn.Conv2d(C, 4 * case.K, 1).to(DEV)
    feats = [torch.randn(case.N, C, h, w, device=DEV) for h, w in case.grids]
    gt, cnt, bases = device_inputs(case)
    m = MultiLevelRPNTraining(seed=case.seed).to(DEV)
    assert m.rng.is_cuda and m.rng.tolist() == [case.seed, 0] and "rng" in m.state_dict()
    hidden = [torch.relu(conv(f)) for f in feats]
    objectness, deltas = [cls(h) for h in hidden], [reg(h) for h in hidden]
    obj_loss, box_loss, tg = m(objectness, deltas, gt, cnt, bases, case.strides)
    assert_bits(tg, case.reference(0), "module, first step")
    (obj_loss + box_loss).backward()
    for p in list(conv.parameters()) + list(cls.parameters()) + list(reg.parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.abs().sum() > 0)
    lo, lb, _, _, _ = ref.losses([t.detach().cpu().numpy() for t in objectness], [t.detach().cpu().numpy() for t in deltas],
                                 case.reference(0), case.K, case.grids)
    np.testing.assert_allclose(obj_loss.item(), lo, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(box_loss.item(), lb, rtol=1e-5, atol=1e-7)
    _, _, tg2 = m(objectness, deltas, gt, cnt, bases, case.strides)
    assert m.rng.tolist() == [case.seed, 2]
    assert_bits(tg2, case.reference(1), "module, second step")
    props = ops.propose_multilevel([t.detach() for t in objectness], [t.detach() for t in deltas], bases, case.strides,
                                   (88, 180), pre_nms_top_n=50, post_nms_top_n=20)
    assert int(props[4].min()) > 0
    # under autocast the head's outputs are 16-bit and go in as they are
    with torch.autocast("cuda", dtype=torch.bfloat16):
        hidden = [torch.relu(conv(f)) for f in feats]
        objectness, deltas = [cls(h) for h in hidden], [reg(h) for h in hidden]
    assert objectness[0].dtype == torch.bfloat16
    obj_loss, box_loss, _ = m(objectness, deltas, gt, cnt, bases, case.strides)
    conv.zero_grad()
    (obj_loss + box_loss).backward()
    assert bool(torch.isfinite(conv.weight.grad).all()) and bool(conv.weight.grad.abs().sum() > 0)
