"""``ops.box_head_targets`` / ``ops.box_head_losses`` / ``heads.BoxHeadTraining`` on the HIP path against
tests/box_head_ref.py, on every named case of tests/box_head_cases.py (DESIGN.md §3 "Pyramid box-head
training").  Needs an MI355X.

The eight target outputs are compared as bits.  Every case runs twice, the second time into pre-filled
caller-owned outputs with the workspace filled with 0xFF, and names the launch plan before anything is
compared.

Loss and gradient bound (DESIGN.md states the derivation; ``box_head_ref.loss_bounds`` evaluates it): with
u = 2^-24, k the additions above one softmax term (a lane's own, then six butterfly levels), the kernels'
fp32 evaluation lies within u(2 + 2 ln C + k + 3 loss) of the fp64 classification loss, 7u box_loss of the
box loss, u |g_cls / S| (7 + ln C + k) of an element of dclass_logits and 5u |g_box / S| of an element of
dbox_regression; a 16-bit gradient adds the spacing of its format at the value.  Every comparison prints
the largest measured difference beside its bound.  Measured: at most 0.23 of the bound on the losses and
the fp32 gradients, 0.48 on 16-bit gradients (the format's spacing is most of that bound)."""
import numpy as np
import pytest
import torch

import box_head_cases as bc
import box_head_ref as ref
from replication_faster_rcnn_amd import ops
from replication_faster_rcnn_amd.heads import BoxHeadTraining

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ops.BoxHeadTargets._fields
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
MANT = {torch.float16: 10, torch.bfloat16: 7}


def state(seed, calls):
    return torch.tensor([seed, calls], dtype=torch.int64).to(DEV)


def device_inputs(case):
    return tuple(torch.from_numpy(a).to(DEV) for a in (case.proposals, case.prop_count, case.gt_boxes, case.gt_labels,
                                                       case.gt_count))


def call(case, rng, **kw):
    return ops.box_head_targets(*device_inputs(case), rng, _key_bits=case.key_bits, **{**case.kw, **kw})


def assert_bits(got, want, what):
    assert NAMES == ref.NAMES
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu().numpy()
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        bad = g.view(np.uint32) != np.ascontiguousarray(w).view(np.uint32)
        assert not bad.any(), (f"{what}: {name}: {int(bad.sum())} of {bad.size} elements differ in their bits; first at "
                               f"{np.argwhere(bad)[0].tolist()}: {g[bad][0]!r} != {w[bad][0]!r}")


@pytest.mark.parametrize("case", bc.CASES, ids=repr)
def test_case(case):
    want = case.reference()
    if case.check is not None:
        case.check(case, want)
    name = ops.box_head_targets_kernel(case.R, case.G, case.N, case.B, case.key_bits)
    for part in case.plan:
        assert part in name, (part, name)
    rng = state(case.seed, case.calls)
    got = call(case, rng)
    assert_bits(got, want, case.name)
    assert rng.cpu().tolist() == [case.seed, case.calls + 1]
    # again, into caller-owned outputs (pre-filled: every element must be stored) with a dirty workspace
    N, B, M = case.N, case.B, case.M
    i32 = dict(dtype=torch.int32, device=DEV)
    outs = (torch.full((N * B, 5), 7.0, device=DEV), torch.full((N, B), 7, **i32), torch.full((N, B), 7, **i32),
            torch.full((N, B, 4), 7.0, device=DEV), torch.full((N, B), 7, **i32), torch.full((N,), 7, **i32),
            torch.full((N,), 7, **i32), torch.full((N, M), 7, **i32))
    need = ops._bht_ws[(N, case.R, case.G, B)]
    ws = torch.full((need + 512,), 0xFF, dtype=torch.uint8, device=DEV)
    ws = ws[(-ws.data_ptr()) % 256:][:need]
    again = call(case, state(case.seed, case.calls), out=outs, workspace=ws)
    assert all(a is b for a, b in zip(again, outs))
    assert_bits(again, want, f"{case.name} (caller-owned outputs, 0xFF workspace)")


def test_second_call_draws_a_fresh_sample():
    case = bc.BY_NAME["layout"]
    rng = ops.sampler_state(case.seed, DEV)
    first = call(case, rng)
    second = call(case, rng)
    assert rng.cpu().tolist() == [case.seed, 2]
    assert_bits(first, case.reference(0), "calls = 0")
    assert_bits(second, case.reference(1), "calls = 1")
    assert not torch.equal(first.samples, second.samples)
    assert torch.equal(first.matches, second.matches)


def device_targets(lc):
    """``BoxHeadTargets`` holding a loss case's labels, reg_targets and counts; the losses read nothing else."""
    N, B = lc.N, lc.B
    z = torch.zeros(1, device=DEV)
    return ops.BoxHeadTargets(z, torch.from_numpy(lc.labels).to(DEV), z, torch.from_numpy(lc.reg_targets).to(DEV), z,
                              torch.from_numpy(lc.n_pos).to(DEV), torch.from_numpy(lc.n_neg).to(DEV), z)


def grad_check(got, want, bound, dtype, what):
    g = got.float().cpu().numpy().astype(np.float64)
    assert not got.view(torch.int32 if dtype == torch.float32 else torch.int16).cpu().numpy()[want == 0].any(), \
        f"{what}: an element that must be +0 is not"
    tiny = 2.0 ** -23 if dtype == torch.float16 else 0.0        # float16 flushes what lies below its subnormals
    assert (g[np.abs(want) > tiny] != 0).all(), f"{what}: a zero where the gradient is not"
    tol = np.full(want.shape, bound)
    if dtype != torch.float32:
        tol += np.maximum(np.abs(want) * 2.0 ** -MANT[dtype], 2.0 ** -24 if dtype == torch.float16 else 0.0)
    diff = np.abs(g - want)
    print(f"{what}: largest difference {diff.max():.3g} (bound {tol.max():.3g})")
    assert (diff <= tol).all(), (what, diff.max())


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("lc", bc.LOSS_CASES, ids=repr)
def test_losses(lc, dtype):
    dt = DTYPES[dtype]
    tg = device_targets(lc)
    cls, reg = lc.predictions(dt)
    g_cls = None if lc.unused == "cls" else 0.75
    g_box = None if lc.unused == "box" else 1.5
    wc, wb, dcls, dreg, stats = ref.losses(cls.float().numpy(), reg.float().numpy(), *lc.targets_np(), g_cls=g_cls,
                                           g_box=g_box)
    S = stats[0]

    def run(cast=None):
        c = (cls if cast is None else cls.to(cast)).to(DEV).requires_grad_(True)
        r = (reg if cast is None else reg.to(cast)).to(DEV).requires_grad_(True)
        a, b, st = ops.box_head_losses_with_stats(c, r, tg)
        ((0.0 if g_cls is None else g_cls * a) + (0.0 if g_box is None else g_box * b)).backward()
        return a.detach(), b.detach(), st, c.grad, r.grad

    a, b, st, gc, gr = run()
    assert a.dtype == b.dtype == torch.float32 and a.dim() == b.dim() == 0
    assert tuple(st.cpu().tolist()) == stats
    bound_c, bound_b, bound_gc, bound_gr = ref.loss_bounds(lc.C, wc, wb, 0.75 / max(S, 1), 1.5 / max(S, 1))
    if S == 0:
        assert torch.isnan(a) and torch.isnan(b)
    else:
        print(f"{lc.name} {dtype}: losses differ by {abs(a.item() - wc):.3g} (bound {bound_c:.3g}) and "
              f"{abs(b.item() - wb):.3g} (bound {bound_b:.3g})")
        assert abs(a.item() - wc) <= bound_c and abs(b.item() - wb) <= bound_b
    assert gc.dtype == gr.dtype == dt and gc.shape == cls.shape and gr.shape == reg.shape
    assert gc.is_contiguous() and gr.is_contiguous()
    grad_check(gc, dcls, bound_gc, dt, f"{lc.name} {dtype} dclass_logits")
    grad_check(gr, dreg, bound_gr, dt, f"{lc.name} {dtype} dbox_regression")
    # the same bits on every call
    a2, b2, _, gc2, gr2 = run()
    assert torch.equal(a.view(torch.int32), a2.view(torch.int32)) and torch.equal(b.view(torch.int32), b2.view(torch.int32))
    bits = torch.int32 if dt == torch.float32 else torch.int16
    assert torch.equal(gc.view(bits), gc2.view(bits)) and torch.equal(gr.view(bits), gr2.view(bits))
    if dt != torch.float32:   # 16-bit inputs are widened exactly: the fp32 op on .float() inputs gives the same losses
        a3, b3, _, _, _ = run(torch.float32)
        assert torch.equal(a.view(torch.int32), a3.view(torch.int32)) and torch.equal(b.view(torch.int32), b3.view(torch.int32))


def test_an_unused_loss_gives_zeros():
    lc = bc.LOSS_BY_NAME["C21"]
    tg = device_targets(lc)
    cls, reg = lc.predictions()
    for use in (0, 1):
        c, r = cls.to(DEV).requires_grad_(True), reg.to(DEV).requires_grad_(True)
        ops.box_head_losses(c, r, tg)[use].backward()
        used, unused = (c.grad, r.grad) if use == 0 else (r.grad, c.grad)
        assert bool(used.any()) and not bool(unused.view(torch.int32).any())


def test_no_host_sync():
    case = bc.BY_NAME["layout"]
    ins = device_inputs(case)
    C = 21
    g = torch.Generator().manual_seed(3)
    c = torch.randn(case.N * case.B, C, generator=g).to(DEV).requires_grad_(True)
    r = torch.randn(case.N * case.B, 4 * C, generator=g).to(DEV).requires_grad_(True)
    rng = ops.sampler_state(case.seed, DEV)
    warm = ops.box_head_targets(*ins, rng, **case.kw)   # caches
    a, b = ops.box_head_losses(c, r, warm)
    (a + b).backward()
    rng.copy_(state(case.seed, 0))
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = ops.box_head_targets(*ins, rng, **case.kw)
        a, b = ops.box_head_losses(c, r, got)
        (a + b).backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert_bits(got, case.reference(), "under sync-debug")
    assert bool(torch.isfinite(a)) and bool(torch.isfinite(b))


def test_refusals():
    case = bc.BY_NAME["layout"]
    p, pc, gt, gl, gc = device_inputs(case)
    rng = ops.sampler_state(1, DEV)

    def refused(match, p=p, pc=pc, gt=gt, gl=gl, gc=gc, rng=rng, **over):
        with pytest.raises(RuntimeError, match=match):
            ops.box_head_targets(p, pc, gt, gl, gc, rng, **over)

    refused("proposals", p=p.double())
    refused("proposals", p=p.cpu())
    refused("proposals", p=p[:, :, :3].contiguous())
    refused("proposals", p=p.transpose(0, 1))
    refused("proposals", p=torch.zeros(2, 4097, 4, device=DEV))
    refused("proposals", p=torch.zeros(2, 0, 4, device=DEV))
    refused("prop_count", pc=pc.long())
    refused("prop_count", pc=pc[:1])
    refused("gt_boxes", gt=gt.half())
    refused("gt_boxes", gt=gt[:1])
    refused("gt_boxes", gt=torch.zeros(2, 257, 4, device=DEV))
    refused("gt_labels", gl=gl.long())
    refused("gt_labels", gl=gl[:, :2].contiguous())
    refused("gt_labels", gl=gl.t().contiguous().t())
    refused("gt_count", gc=gc.cpu())
    refused("rng", rng=rng.int())
    refused("rng", rng=torch.zeros(3, dtype=torch.int64, device=DEV))
    refused("batch_size_per_image", batch_size_per_image=0)
    refused("batch_size_per_image", batch_size_per_image=1025)
    refused("positive_fraction", positive_fraction=1.5)
    refused("bg_iou_thresh", fg_iou_thresh=0.3, bg_iou_thresh=0.7)
    refused("reg_weights", reg_weights=(1.0, 1.0, 0.0, 1.0))
    refused("reg_weights", reg_weights=(1.0, 1.0, 1.0))
    refused("reg_weights", reg_weights=(1.0, 1.0, float("inf"), 1.0))
    refused("_key_bits", _key_bits=33)
    outs = list(ops.box_head_targets(p, pc, gt, gl, gc, rng, **case.kw))
    refused(r"out\[0\] \(rois\)", out=[outs[0].double()] + outs[1:], **case.kw)
    refused(r"out\[7\] \(matches\)", out=outs[:7] + [outs[7][:, :-1]], **case.kw)
    refused("eight outputs", out=outs[:7], **case.kw)
    refused("workspace", workspace=torch.empty(16, dtype=torch.uint8, device=DEV))
    refused("workspace", workspace=torch.empty(1 << 20, dtype=torch.uint8))

    tg = ops.BoxHeadTargets(*outs)
    rows, C = case.N * case.B, 5
    c, r = torch.zeros(rows, C, device=DEV), torch.zeros(rows, 4 * C, device=DEV)

    def loss_refused(match, c=c, r=r, tg=tg, **kw):
        with pytest.raises(RuntimeError, match=match):
            ops.box_head_losses(c, r, tg, **kw)

    loss_refused("box_regression", r=r.half())                                   # mixed dtypes
    loss_refused("class_logits", c=c.double(), r=r.double())
    loss_refused("box_regression", r=r.cpu())
    loss_refused("class_logits", c=c.t().contiguous().t())                        # a strided view
    loss_refused("class_logits", c=c[:-1])                                        # not N*B rows
    loss_refused("box_regression", r=r[:, :-4].contiguous())                      # not 4C columns
    loss_refused("class_logits", c=torch.zeros(rows, 1, device=DEV), r=torch.zeros(rows, 4, device=DEV))
    loss_refused("class_logits", c=torch.zeros(rows, 129, device=DEV), r=torch.zeros(rows, 516, device=DEV))
    loss_refused("targets", tg=tuple(outs))
    loss_refused(r"targets\.n_pos", tg=tg._replace(n_pos=tg.n_pos.long()))
    loss_refused(r"targets\.reg_targets", tg=tg._replace(reg_targets=tg.reg_targets[:, :, :3].contiguous()))
    loss_refused("beta", beta=float("nan"))
    loss_refused("beta", beta=-1.0)


def test_capi_refusals():
    """The limits at the C-ABI itself: FRCNN_EINVAL with a message naming the argument, before any launch."""
    from replication_faster_rcnn_amd import _lib
    lib = _lib.load()
    case = bc.BY_NAME["layout"]
    p, pc, gt, gl, gc = device_inputs(case)
    rng = ops.sampler_state(1, DEV)
    outs = ops.box_head_targets(p, pc, gt, gl, gc, rng, **case.kw)
    N, R, G, B = case.N, case.R, case.G, case.B
    need = ops._bht_ws[(N, R, G, B)]
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def rc_of(frac=0.25, fg=0.5, bg=0.5, ww=5.0, ws_bytes=need, kb=32, R=R):
        return lib.frcnn_box_head_targets(p.data_ptr(), pc.data_ptr(), N, R, gt.data_ptr(), gl.data_ptr(), gc.data_ptr(), G,
                                          rng.data_ptr(), B, frac, fg, bg, 10.0, 10.0, ww, 5.0, 1, kb,
                                          *[t.data_ptr() for t in outs], ws.data_ptr(), ws_bytes, None)

    before = rng.cpu().tolist()
    assert rc_of(frac=1.25) == -1 and b"positive_fraction" in lib.frcnn_last_error()
    assert rc_of(fg=0.2) == -1 and b"bg_iou_thresh" in lib.frcnn_last_error()
    assert rc_of(ww=-1.0) == -1 and b"reg_weights" in lib.frcnn_last_error()
    assert rc_of(ww=float("nan")) == -1 and b"reg_weights" in lib.frcnn_last_error()
    assert rc_of(ws_bytes=need - 1) == -1 and b"workspace" in lib.frcnn_last_error()
    assert rc_of(kb=-1) == -1 and b"key_bits" in lib.frcnn_last_error()
    assert rc_of(R=4097) == -1 and b"R must be" in lib.frcnn_last_error()
    torch.cuda.synchronize()
    assert rng.cpu().tolist() == before                                          # nothing was launched
    C = 5
    c, r = torch.zeros(N * B, C, device=DEV), torch.zeros(N * B, 4 * C, device=DEV)
    loss, stats = torch.zeros(2, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    lws = torch.empty(int(lib.frcnn_box_head_losses_workspace_size(N, B)), dtype=torch.uint8, device=DEV)

    def fwd(dtype=0, C=C, beta=0.1, ws_bytes=lws.numel()):
        return lib.frcnn_box_head_losses_fwd_t(dtype, c.data_ptr(), r.data_ptr(), N, B, C, outs.labels.data_ptr(),
                                               outs.reg_targets.data_ptr(), outs.n_pos.data_ptr(), outs.n_neg.data_ptr(),
                                               beta, loss.data_ptr(), stats.data_ptr(), lws.data_ptr(), ws_bytes, None)

    assert fwd(dtype=3) == -1 and b"dtype" in lib.frcnn_last_error()
    assert fwd(C=1) == -1 and fwd(C=129) == -1 and b"C must be" in lib.frcnn_last_error()
    assert fwd(beta=-0.5) == -1 and b"beta" in lib.frcnn_last_error()
    assert fwd(ws_bytes=0) == -1 and b"workspace" in lib.frcnn_last_error()
    assert fwd() == 0
    assert lib.frcnn_box_head_losses_bwd_t(0, c.data_ptr(), r.data_ptr(), N, B, C, outs.labels.data_ptr(),
                                           outs.reg_targets.data_ptr(), outs.n_pos.data_ptr(), outs.n_neg.data_ptr(), 0.1,
                                           stats.data_ptr(), None, None, None, r.data_ptr(), None) == -1
    assert b"null tensor" in lib.frcnn_last_error()


def test_chain_trains_end_to_end():
    """propose_multilevel -> BoxHeadTraining.targets -> multiscale_roi_align -> one Linear per prediction ->
    .losses -> backward, on a tiny pyramid: the gradients reach the pyramid maps and the linears, padding rows
    get none, and a few SGD steps under a fixed seed lower the summed loss."""
    torch.manual_seed(0)
    N, Cf, K, C, B, post = 2, 8, 3, 5, 32, 24
    grids, strides = ((16, 24), (8, 12), (4, 6)), ((4, 4), (8, 8), (16, 16))
    bases = [b.to(DEV) for b in ops.pyramid_anchor_bases(((8,), (16,), (32,)), (0.5, 1.0, 2.0))]
    feats = [torch.randn(N, Cf, h, w, device=DEV).requires_grad_(True) for h, w in grids]
    rpn_cls = torch.nn.Conv2d(Cf, K, 1).to(DEV)
    rpn_reg = torch.nn.Conv2d(Cf, 4 * K, 1).to(DEV)
    with torch.no_grad():
        objectness, deltas = [rpn_cls(f) for f in feats], [0.1 * rpn_reg(f) for f in feats]
    boxes, _, _, _, count, _ = ops.propose_multilevel(objectness, deltas, bases, strides, (64, 96), pre_nms_top_n=200,
                                                      post_nms_top_n=post)
    gt = torch.tensor([[[8, 8, 40, 40], [50, 20, 90, 60], [0, 0, 0, 0]],
                       [[30, 10, 70, 50], [0, 0, 0, 0], [0, 0, 0, 0]]], dtype=torch.float32, device=DEV)
    gl = torch.tensor([[1, 3, 0], [4, 0, 0]], dtype=torch.int32, device=DEV)
    gc = torch.tensor([2, 1], dtype=torch.int32, device=DEV)
    m = BoxHeadTraining(batch_size_per_image=B, seed=5).to(DEV)
    assert m.rng.is_cuda and m.rng.tolist() == [5, 0] and "rng" in m.state_dict()
    fc_cls = torch.nn.Linear(Cf * 4, C).to(DEV)
    fc_reg = torch.nn.Linear(Cf * 4, 4 * C).to(DEV)
    opt = torch.optim.SGD(list(fc_cls.parameters()) + list(fc_reg.parameters()), lr=0.1)
    totals = []
    for step in range(6):
        tg = m.targets(boxes, count, gt, gl, gc)
        pooled = ops.multiscale_roi_align(feats, tg.rois, 2, (1 / 4, 1 / 8, 1 / 16), 2)
        pooled.retain_grad()
        flat = pooled.flatten(1)
        logits, regs = fc_cls(flat), fc_reg(flat)
        logits.retain_grad()
        regs.retain_grad()
        loss_c, loss_b = m.losses(logits, regs, tg)
        assert bool(torch.isfinite(loss_c)) and bool(torch.isfinite(loss_b))
        opt.zero_grad()
        for f in feats:
            f.grad = None
        (loss_c + loss_b).backward()
        if step == 0:
            S = int((tg.n_pos + tg.n_neg).sum())
            assert int(tg.n_pos.min()) > 0 and S < N * B                  # positives in both images, and padding
            pad = tg.rois[:, 0] < 0
            assert bool(pad.any()) and bool((tg.labels.view(-1)[pad] == -1).all())
            assert not bool(logits.grad[pad].any()) and not bool(regs.grad[pad].any()) and not bool(pooled.grad[pad].any())
            assert bool(logits.grad[~pad].any(dim=1).all())
            for p in list(fc_cls.parameters()) + list(fc_reg.parameters()):
                assert bool(torch.isfinite(p.grad).all()) and bool(p.grad.abs().sum() > 0)
            assert any(bool(f.grad.abs().sum() > 0) for f in feats) and all(bool(torch.isfinite(f.grad).all()) for f in feats)
            want = ref.losses(logits.detach().cpu().numpy(), regs.detach().cpu().numpy(), tg.labels.cpu().numpy(),
                              tg.reg_targets.cpu().numpy(), tg.n_pos.cpu().numpy(), tg.n_neg.cpu().numpy())
            bound_c, bound_b, _, _ = ref.loss_bounds(C, want[0], want[1], 1.0 / S, 1.0 / S)
            assert abs(loss_c.item() - want[0]) <= bound_c and abs(loss_b.item() - want[1]) <= bound_b
        opt.step()
        totals.append(float((loss_c + loss_b).detach()))
    assert m.rng.tolist() == [5, 6]
    print("summed loss per step:", [round(t, 4) for t in totals])
    assert totals[-1] < totals[0]
