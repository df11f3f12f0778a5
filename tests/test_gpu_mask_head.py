"""``ops.mask_head_targets`` / ``mask_head_losses`` / ``mask_head_paste`` and the two modules of
``heads`` on the HIP path against tests/mask_head_ref.py, on every named case of
tests/mask_head_cases.py (DESIGN.md §3 "Pyramid mask head").  Needs an MI355X.

Targets and pasted masks are compared as bits; the loss and its gradient within
``mask_head_ref.loss_bounds`` with the elements that must be +0 compared as bits.  Every case
names its launch plan first and runs twice, the second time into caller-owned outputs pre-filled
with 7 and, for the losses, an exact 256-byte aligned workspace filled with 0xFF."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import mask_head_cases as mc
import mask_head_ref as ref
import roi_align_ref as ra
from replication_faster_rcnn_amd import _lib, ops
from replication_faster_rcnn_amd.heads import (BoxHeadDetections, BoxHeadTraining, MaskHeadInference,
                                               MaskHeadTraining)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def dev(a):
    return torch.tensor(a).to(DEV)


def same(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert ref.bits_equal(g, w), f"{what}: output {i} differs"


# ---------------------------------------------------------------- targets
def box_targets(case):
    z = torch.zeros(1, device=DEV)
    return ops.BoxHeadTargets(dev(case.bt_rois), dev(case.bt_labels), dev(case.bt_matched), z, z, z, z, z)


@pytest.mark.parametrize("case", mc.TARGET_CASES, ids=repr)
def test_targets_case(case):
    want = case.reference()
    P = case.B if case.P is None else case.P
    assert ops.mask_head_targets_kernel(case.B, case.P, case.M) == f"mh_compact_kernel mh_targets_kernel[{case.plan}]"
    bt, masks = box_targets(case), dev(case.gt_masks)
    got = ops.mask_head_targets(bt, masks, mask_size=case.M, positives_per_image=case.P)
    assert isinstance(got, ops.MaskHeadTargets) and ops.MaskHeadTargets._fields == ref.TARGET_OUT
    same(got, want, case.name)
    # on the device against ops.roi_align on the gathered, widened masks
    n_idx = torch.arange(case.N, device=DEV).repeat_interleave(P)
    g = got.matched.view(-1)
    real = (g >= 0) & (g < case.G)
    k = int(real.sum())
    if k:
        x = masks[n_idx[real], g[real].long()].float()[:, None]
        rois = torch.cat([torch.arange(k, device=DEV, dtype=torch.float32)[:, None], got.rois[real][:, 1:]], 1)
        pooled = ops.roi_align(x, rois, (case.M, case.M), 1.0, -1, False)[:, 0]
        assert torch.equal(pooled.view(torch.int32), got.targets[real].view(torch.int32)), "differs from ops.roi_align"
    assert not bool(got.targets[~real].any())
    # again, into caller-owned outputs (pre-filled: every element must be stored)
    outs = tuple(torch.full_like(t, 7) for t in got)
    again = ops.mask_head_targets(bt, masks, mask_size=case.M, positives_per_image=case.P, out=outs)
    assert all(a is b for a, b in zip(again, outs))
    same(again, want, f"{case.name} (caller-owned outputs)")


def test_targets_module_and_row_limits():
    """``heads.MaskHeadTraining.targets``; B = P = 1,024 (every thread of the compaction owns a slot)."""
    case = mc.TARGETS_BY_NAME["clamp_and_drop"]
    m = MaskHeadTraining(mask_size=case.M, positives_per_image=case.P)
    same(m.targets(box_targets(case), dev(case.gt_masks)), case.reference(), "module")
    r = np.random.default_rng(0)
    B = 1024
    lab = (r.random((1, B)) < 0.1).astype(np.int32) * r.integers(1, 5, (1, B)).astype(np.int32)
    lab[0, -1] = 2
    rois = np.zeros((B, 5), np.float32)
    rois[:, 1:3] = r.uniform(0, 10, (B, 2))
    rois[:, 3:] = rois[:, 1:3] + r.uniform(1, 9, (B, 2))
    big = mc.TargetsCase("b1024", {}, N=1, B=B, G=2, H=20, W=21, M=4, seed=3)
    big.bt_rois, big.bt_labels, big.bt_matched = rois, lab, r.integers(0, 2, (1, B)).astype(np.int32)
    got = ops.mask_head_targets(box_targets(big), dev(big.gt_masks), mask_size=4)
    same(got, big.reference(), "B = P = 1024")
    assert int(got.slot[0, int(got.count[0]) - 1]) == B - 1


# ----------------------------------------------------------------- losses
def loss_targets(case):
    z = torch.zeros(1, device=DEV)
    return ops.MaskHeadTargets(z, dev(case.labels), z, z, dev(case.count), dev(case.targets))


LOSS_RUNS = [(c, "f32") for c in mc.LOSS_CASES] + [(c, d) for c in mc.LOSS_HALF for d in ("f16", "bf16")]


@pytest.mark.parametrize("case,dtype", LOSS_RUNS, ids=lambda v: v if isinstance(v, str) else repr(v))
def test_losses_case(case, dtype):
    want_loss, want_grad, (S, skipped) = case.reference()
    lb, gb = case.bounds(dtype)
    dt = DTYPES[dtype]
    e, V = ra.ELEM[dtype], 4 if dtype == "f32" else 8
    assert ops.mask_head_losses_kernel(case.C, case.M, dt) == (
        f"mh_loss_rows_kernel<{e}> mh_loss_final_kernel mh_loss_bwd_kernel<{e}>[vec{V}]")
    tg = loss_targets(case)
    need = _lib.load().frcnn_mask_losses_workspace_size(case.N, case.P)
    ws = torch.full((need + 512,), 0xFF, dtype=torch.uint8, device=DEV)
    ws = ws[(-ws.data_ptr()) % 256:][:need]
    assert ws.data_ptr() % 256 == 0 and ws.numel() == need
    results = []
    for workspace in (None, ws):
        x = dev(case.logits).to(dt).requires_grad_(True)
        assert torch.equal(x.detach().float().cpu(), torch.from_numpy(case.logits)) or dtype == "f32"
        loss, stats = ops.mask_head_losses_with_stats(x, tg, workspace=workspace)
        assert loss.dtype == torch.float32 and loss.dim() == 0
        assert stats.tolist() == [S, skipped, 0, 0]
        (loss * case.g).backward()
        assert x.grad.dtype == dt and x.grad.is_contiguous()
        g = x.grad.float().cpu().numpy()
        dl, dg = abs(float(loss.detach()) - want_loss), float(np.abs(g - want_grad).max())
        print(f"{case.name} {dtype}: |loss - fp64| = {dl:.3e} (bound {lb:.3e}); gradient {dg:.3e} (bound {gb.max():.3e})")
        assert np.isfinite(float(loss.detach())) and dl <= lb
        assert (np.abs(g - want_grad) <= gb).all()
        raw = x.grad.view(torch.int32 if dtype == "f32" else torch.int16).cpu().numpy()
        assert not raw[gb == 0].any(), "an element that must be +0 is not"
        if S == 0:
            assert float(loss.detach()) == 0.0 and not np.signbit(float(loss.detach()))
        results.append((loss.detach().clone(), x.grad.clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])


def test_losses_module_and_scaled_gradient():
    """Through ``heads.MaskHeadTraining.losses``: an incoming gradient other than 1 scales the stored
    values once (g / (S*M*M) is formed first)."""
    case = mc.LOSSES_BY_NAME["label_ge_c"]
    tg = loss_targets(case)
    x = dev(case.logits).requires_grad_(True)
    m = MaskHeadTraining(mask_size=case.M)
    (m.losses(x, tg) * 3.0).backward()
    want = ref.mask_losses(case.logits, case.targets, case.labels, case.count, 3.0)[1]
    _, gb = ref.loss_bounds(case.logits, case.targets, case.labels, case.count, 3.0)
    assert (np.abs(x.grad.cpu().numpy() - want) <= gb).all()


# ------------------------------------------------------------------ paste
def paste_call(case, dtype="f32", **over):
    kw = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in case.kw.items()}
    kw.update(over)
    return ops.mask_head_paste(dev(case.logits).to(DTYPES[dtype]), dev(case.boxes), dev(case.labels), dev(case.count),
                               case.canvas, **kw)


PASTE_RUNS = [(c, "f32") for c in mc.PASTE_CASES] + [(c, d) for c in mc.PASTE_HALF for d in ("f16", "bf16")]


@pytest.mark.parametrize("case,dtype", PASTE_RUNS, ids=lambda v: v if isinstance(v, str) else repr(v))
def test_paste_case(case, dtype):
    want = case.reference()
    assert ops.mask_head_paste_kernel(case.M, case.canvas[1], case.kw.get("padding", 1), case.kw.get("threshold", 0.5),
                                      DTYPES[dtype]) == case.plan(dtype)
    got = paste_call(case, dtype)
    assert got.shape == (case.N, case.D) + case.canvas
    g = got.cpu().numpy()
    if not ref.bits_equal(g, want):
        bad = np.argwhere(g != want)
        print(f"{case.name}: {len(bad)} elements differ, first at {bad[0]}, largest difference "
              f"{np.abs(g.astype(np.float64) - want).max():.3e}")
    assert ref.bits_equal(g, want), case.name
    out = torch.full_like(got, 7)
    again = paste_call(case, dtype, out=out)
    assert again is out and ref.bits_equal(out.cpu().numpy(), want), f"{case.name} (caller-owned output)"
    # an output that starts off a 16-byte boundary: every row has a head and a tail
    flat = torch.full((got.numel() + 16,), 7, dtype=got.dtype, device=DEV)
    off = flat[1:1 + got.numel()].view(got.shape)
    paste_call(case, dtype, out=off)
    assert ref.bits_equal(off.cpu().numpy(), want), f"{case.name} (unaligned output)"
    assert bool((flat[:1] == 7).all()) and bool((flat[1 + got.numel():] == 7).all())


def test_paste_module_and_detection_rois():
    case = mc.PASTE_BY_NAME["count_0_and_d"]
    z = torch.zeros(1, device=DEV)
    det = ops.BoxDetections(dev(case.boxes), dev(case.labels), z, z, dev(case.count), z)
    m = MaskHeadInference(padding=1, threshold=0.5)
    same([m(dev(case.logits), det, case.canvas)], [case.reference()], "module")
    same([ops.detection_rois(det)], [ref.detection_rois(case.boxes, case.count)], "detection_rois")


# --------------------------------------------------- determinism, no sync
def test_two_calls_same_bits_and_no_host_sync():
    tc, lc, pc = mc.TARGETS_BY_NAME["interleaved_m28"], mc.LOSSES_BY_NAME["m28_unaligned_planes"], mc.PASTE_BY_NAME["wc37_m28"]
    bt, masks = box_targets(tc), dev(tc.gt_masks)
    tg = loss_targets(lc)
    pin = (dev(pc.logits), dev(pc.boxes), dev(pc.labels), dev(pc.count))
    x0 = dev(lc.logits)

    def run():
        t = ops.mask_head_targets(bt, masks, mask_size=tc.M)
        x = x0.detach().requires_grad_(True)
        loss = ops.mask_head_losses(x, tg)
        loss.backward()
        p = ops.mask_head_paste(*pin, pc.canvas)
        return list(t) + [loss.detach(), x.grad, p, ops.detection_rois(ops.BoxDetections(pin[1], pin[2], None, None, pin[3], None))]

    first = run()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = run()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for a, b in zip(first, second):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8) if a.dim() else a, b.view(torch.uint8) if b.dim() else b)
    same(second[:6], tc.reference(), "under sync-debug")
    same([second[8]], [pc.reference()], "paste under sync-debug")


# --------------------------------------------------------------- refusals
def test_refusals():
    """Each limit, mixed dtypes, host tensors, strided views and wrong outputs raise a
    RuntimeError naming the argument before any launch; the C-ABI returns its codes."""
    tc = mc.TARGETS_BY_NAME["clamp_and_drop"]
    bt, masks = box_targets(tc), dev(tc.gt_masks)

    def t_refused(match, bt=bt, masks=masks, **kw):
        with pytest.raises(RuntimeError, match=match):
            ops.mask_head_targets(bt, masks, **{"mask_size": 4, **kw})

    t_refused("box_targets", bt=tuple(bt))
    t_refused("box_targets.labels", bt=bt._replace(labels=bt.labels.long()))
    t_refused("box_targets.labels", bt=bt._replace(labels=bt.labels.cpu()))
    t_refused("box_targets.matched", bt=bt._replace(matched=bt.matched[:, :-1]))
    t_refused("box_targets.matched", bt=bt._replace(matched=bt.matched.t().contiguous().t()))
    t_refused("box_targets.rois", bt=bt._replace(rois=bt.rois.double()))
    t_refused("B must", bt=bt._replace(labels=torch.zeros(1, 1025, dtype=torch.int32, device=DEV)))
    t_refused("N must", bt=bt._replace(labels=torch.zeros(1025, 1, dtype=torch.int32, device=DEV)))
    t_refused("gt_masks", masks=masks.float())
    t_refused("gt_masks", masks=masks.bool())
    t_refused("gt_masks", masks=masks.cpu())
    t_refused("gt_masks", masks=masks[:, :, :, ::2])
    t_refused("gt_masks", masks=masks[:1])
    t_refused("G must", masks=torch.zeros(2, 257, 4, 4, dtype=torch.uint8, device=DEV))
    t_refused("Hm and Wm", masks=torch.zeros(2, 1, 4097, 1, dtype=torch.uint8, device=DEV))
    t_refused("mask_size", mask_size=57)
    t_refused("mask_size", mask_size=0)
    t_refused("positives_per_image", positives_per_image=0)
    t_refused("positives_per_image", positives_per_image=1025)
    outs = list(ops.mask_head_targets(bt, masks, mask_size=4, positives_per_image=3))
    t_refused("six outputs", out=outs[:5], positives_per_image=3)
    t_refused(r"out\[5\] \(targets\)", out=outs[:5] + [outs[5].double()], positives_per_image=3)
    t_refused(r"out\[0\] \(rois\)", out=outs, positives_per_image=4)

    lc = mc.LOSSES_BY_NAME["label_ge_c"]
    tg, x = loss_targets(lc), dev(lc.logits)

    def l_refused(match, x=x, tg=tg, **kw):
        with pytest.raises(RuntimeError, match=match):
            ops.mask_head_losses(x, tg, **kw)

    l_refused("targets", tg=tuple(tg))
    l_refused("mask_logits", x=x.double())
    l_refused("mask_logits", x=x.cpu())
    l_refused("mask_logits", x=x[:-1])
    l_refused("mask_logits", x=x.transpose(2, 3))
    l_refused("mask_logits", x=x[:, :, :, :-1])
    l_refused("C must", x=x[:, :1].contiguous())
    l_refused("C must", x=torch.zeros(x.shape[0], 129, 4, 4, device=DEV))
    l_refused("targets.count", tg=tg._replace(count=tg.count.long()))
    l_refused("targets.targets", tg=tg._replace(targets=tg.targets.half()))
    l_refused("targets.labels", tg=tg._replace(labels=tg.labels.cpu()))
    l_refused("workspace", workspace=torch.empty(8, dtype=torch.uint8, device=DEV))

    pc = mc.PASTE_BY_NAME["inside"]
    pin = dict(x=dev(pc.logits), boxes=dev(pc.boxes), labels=dev(pc.labels), count=dev(pc.count), canvas=pc.canvas)

    def p_refused(match, **over):
        a = {**pin, **{k: v for k, v in over.items() if k in pin}}
        kw = {k: v for k, v in over.items() if k not in pin}
        with pytest.raises(RuntimeError, match=match):
            ops.mask_head_paste(a["x"], a["boxes"], a["labels"], a["count"], a["canvas"], **kw)

    sz = torch.tensor([[36.0, 48.0]] * pc.N, device=DEV)
    p_refused("mask_logits", x=pin["x"].double())
    p_refused("mask_logits", x=pin["x"].cpu())
    p_refused("mask_logits", x=pin["x"][1:])
    p_refused("mask_logits", x=pin["x"].transpose(2, 3))
    p_refused("boxes", boxes=pin["boxes"].double())
    p_refused("boxes", boxes=pin["boxes"][:, :, :3])
    p_refused("D must", boxes=torch.zeros(1, 1025, 4, device=DEV))
    p_refused("labels", labels=pin["labels"].long())
    p_refused("count", count=pin["count"].cpu())
    p_refused("canvas_size", canvas=(36,))
    p_refused("canvas_size", canvas=(36, 4097))
    p_refused("canvas_size", canvas=(0, 48))
    p_refused("padding", padding=5)
    p_refused("padding", padding=-1)
    p_refused("threshold", threshold=float("nan"))
    p_refused("original_sizes", original_sizes=sz.cpu())
    p_refused("image_sizes", image_sizes=sz)
    p_refused("image_sizes", image_sizes=sz.double(), original_sizes=sz)
    p_refused("out", out=torch.zeros((pc.N, pc.D) + pc.canvas, device=DEV))
    p_refused("out", out=torch.zeros((pc.N, pc.D) + pc.canvas, dtype=torch.uint8, device=DEV), threshold=None)

    # the C-ABI's own return codes, nothing launched
    lib = _lib.load()
    N, B, P, G = tc.N, tc.B, 3, tc.G
    for o in outs:
        o.fill_(7)
    ptrs = [bt.rois.data_ptr(), bt.labels.data_ptr(), bt.matched.data_ptr(), masks.data_ptr()] + [o.data_ptr() for o in outs]
    assert lib.frcnn_mask_targets(N, B, P, G, 4097, tc.W, 4, *ptrs, None) == -1 and b"Hm and Wm" in lib.frcnn_last_error()
    assert lib.frcnn_mask_targets(N, B, P, G, tc.H, tc.W, 57, *ptrs, None) == -1 and b"mask_size" in lib.frcnn_last_error()
    assert lib.frcnn_mask_targets(N, B, P, G, tc.H, tc.W, 4, *ptrs[:3], None, *ptrs[4:], None) == -1
    assert b"null input" in lib.frcnn_last_error()
    need = lib.frcnn_mask_losses_workspace_size(lc.N, lc.P)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    loss, stats = torch.full((1,), 7.0, device=DEV), torch.full((4,), 7, dtype=torch.int32, device=DEV)
    largs = (x.data_ptr(), tg.targets.data_ptr(), tg.labels.data_ptr(), tg.count.data_ptr(), loss.data_ptr(), stats.data_ptr())
    assert lib.frcnn_mask_losses_fwd_t(0, lc.N, lc.P, lc.C, lc.M, *largs, ws.data_ptr(), need - 1, None) == -3
    assert b"workspace" in lib.frcnn_last_error()
    assert lib.frcnn_mask_losses_fwd_t(3, lc.N, lc.P, lc.C, lc.M, *largs, ws.data_ptr(), need, None) == -1
    assert b"dtype" in lib.frcnn_last_error()
    d = torch.full_like(x, 7)
    assert lib.frcnn_mask_losses_bwd_t(0, lc.N, lc.P, lc.C, lc.M, x.data_ptr(), tg.targets.data_ptr(), tg.labels.data_ptr(),
                                       tg.count.data_ptr(), stats.data_ptr(), None, d.data_ptr() + 4, None) == -1
    assert b"16-byte" in lib.frcnn_last_error()
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs + [loss, stats, d])          # nothing was launched
    assert lib.frcnn_mask_targets(N, B, P, G, tc.H, tc.W, 4, *ptrs, None) == 0
    same(outs, ref.mask_targets(tc.bt_rois, tc.bt_labels, tc.bt_matched, tc.gt_masks, 4, 3), "the C-ABI call")


# ------------------------------------------------------------- end to end
def _pyramid(N, Cf, K, post, sizes):
    grids, strides = ((16, 24), (8, 12)), ((4, 4), (8, 8))
    bases = [b.to(DEV) for b in ops.pyramid_anchor_bases(((8,), (16,)), (0.5, 1.0, 2.0))]
    feats = [torch.randn(N, Cf, h, w, device=DEV) for h, w in grids]
    rpn_cls = torch.nn.Conv2d(Cf, K, 1).to(DEV)
    rpn_reg = torch.nn.Conv2d(Cf, 4 * K, 1).to(DEV)
    with torch.no_grad():
        objectness, deltas = [rpn_cls(f) for f in feats], [0.1 * rpn_reg(f) for f in feats]
        prop = ops.propose_multilevel(objectness, deltas, bases, strides, sizes, pre_nms_top_n=200, post_nms_top_n=post)
    return feats, prop


def test_chain_trains_end_to_end():
    """propose_multilevel -> BoxHeadTraining.targets -> MaskHeadTraining.targets -> multiscale_roi_align(14)
    -> a one-layer conv head -> .losses -> backward on a two-level pyramid, against the composed torch path
    (torch.where, gathered float masks, ops.roi_align, indexed binary_cross_entropy_with_logits) on the
    same tensors."""
    torch.manual_seed(0)
    N, Cf, K, C, B, P, post, M = 2, 8, 3, 5, 32, 12, 24, 14
    feats, (boxes, _, _, _, count, _) = _pyramid(N, Cf, K, post, (64, 96))
    gt = torch.tensor([[[8, 8, 40, 40], [50, 20, 90, 60], [0, 0, 0, 0]],
                       [[30, 10, 70, 50], [0, 0, 0, 0], [0, 0, 0, 0]]], dtype=torch.float32, device=DEV)
    gl = torch.tensor([[1, 3, 0], [4, 0, 0]], dtype=torch.int32, device=DEV)
    gc = torch.tensor([2, 1], dtype=torch.int32, device=DEV)
    masks = torch.zeros(N, 3, 64, 96, dtype=torch.uint8, device=DEV)
    for n in range(N):
        for g in range(int(gc[n])):
            x1, y1, x2, y2 = (int(v) for v in gt[n, g])
            masks[n, g, y1 + 3:y2 - 2, x1 + 2:x2 - 4] = 1
    bt = BoxHeadTraining(batch_size_per_image=B, seed=5).to(DEV).targets(boxes, count, gt, gl, gc)
    head = MaskHeadTraining(mask_size=M, positives_per_image=P)
    conv = torch.nn.Conv2d(Cf, C, 1).to(DEV)
    fs = [f.clone().requires_grad_(True) for f in feats]
    mt = head.targets(bt, masks)
    assert int(mt.count.min()) > 0 and int(mt.count.max()) <= P and bool((mt.count < P).any())
    logits = conv(ops.multiscale_roi_align(fs, mt.rois, M, (1 / 4, 1 / 8), 2))
    logits.retain_grad()
    loss = head.losses(logits, mt)
    loss.backward()
    got = [loss.detach().clone(), conv.weight.grad.clone(), conv.bias.grad.clone()] + [f.grad.clone() for f in fs]
    pad = mt.rois[:, 0] < 0
    assert bool(pad.any()) and not bool(logits.grad[pad].any()) and bool(logits.grad[~pad].flatten(1).any(dim=1).all())
    # the composed path
    conv.zero_grad()
    fs2 = [f.clone().requires_grad_(True) for f in feats]
    pos = torch.where(bt.labels.view(-1) > 0)[0]
    n_idx = pos // B
    x = masks[n_idx, bt.matched.view(-1)[pos].long()].float()[:, None]
    k = len(pos)
    rois = torch.cat([torch.arange(k, device=DEV, dtype=torch.float32)[:, None], bt.rois[pos][:, 1:]], 1)
    tgt = ops.roi_align(x, rois, (M, M), 1.0, -1, False)[:, 0]
    assert torch.equal(tgt, mt.targets[~pad]) and k == int(mt.count.sum())
    lg = conv(ops.multiscale_roi_align(fs2, bt.rois[pos].contiguous(), M, (1 / 4, 1 / 8), 2))
    want_loss = TF.binary_cross_entropy_with_logits(lg[torch.arange(k, device=DEV), bt.labels.view(-1)[pos].long()], tgt)
    want_loss.backward()
    want = [want_loss.detach(), conv.weight.grad, conv.bias.grad] + [f.grad for f in fs2]
    wl, _, _ = ref.mask_losses(logits.detach().cpu().numpy(), mt.targets.cpu().numpy(), mt.labels.cpu().numpy(),
                               mt.count.cpu().numpy())
    lb, _ = ref.loss_bounds(logits.detach().cpu().numpy(), mt.targets.cpu().numpy(), mt.labels.cpu().numpy(),
                            mt.count.cpu().numpy())
    print(f"training chain: {k} positives, loss {float(loss.detach()):.6f} (composed {float(want_loss):.6f}, fp64 {wl:.6f})")
    assert abs(float(loss.detach()) - wl) <= lb
    for a, b in zip(got, want):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-6), float((a - b).abs().max())


def test_chain_pastes_end_to_end():
    """propose_multilevel -> multiscale_roi_align -> BoxHeadDetections -> detection_rois -> multiscale_roi_align(14)
    -> a one-layer conv head -> MaskHeadInference with the boxes mapped to the original sizes, against the
    restatement on the head's own outputs."""
    torch.manual_seed(0)
    N, Cf, K, C, post, D, M = 2, 8, 3, 3, 24, 6, 14
    sizes = torch.tensor([[64.0, 96.0], [60.0, 90.0]], device=DEV)
    orig = torch.tensor([[128.0, 192.0], [100.0, 150.0]], device=DEV)
    feats, (boxes, _, _, _, count, rois) = _pyramid(N, Cf, K, post, sizes)
    fc_cls = torch.nn.Linear(Cf * 4, C).to(DEV)
    fc_reg = torch.nn.Linear(Cf * 4, 4 * C).to(DEV)
    conv = torch.nn.Conv2d(Cf, C, 1).to(DEV)
    with torch.no_grad():
        flat = ops.multiscale_roi_align(feats, rois, 2, (1 / 4, 1 / 8), 2).flatten(1)
        det = BoxHeadDetections(detections_per_img=D)(2.0 * fc_cls(flat), fc_reg(flat), boxes, count, sizes)
        mrois = ops.detection_rois(det)
        logits = 3.0 * conv(ops.multiscale_roi_align(feats, mrois, M, (1 / 4, 1 / 8), 2))
    assert int(det.count.min()) > 0
    got = MaskHeadInference()(logits, det, (128, 192), image_sizes=sizes, original_sizes=orig)
    want = ref.mask_paste(logits.cpu().numpy(), det.boxes.cpu().numpy(), det.labels.cpu().numpy(), det.count.cpu().numpy(),
                          (128, 192), image_sizes=sizes.cpu().numpy(), original_sizes=orig.cpu().numpy())
    assert got.dtype == torch.uint8 and ref.bits_equal(got.cpu().numpy(), want)
    assert 0 < int(got.sum()) < got.numel() and not bool(got[1, :, 100:].any()) and not bool(got[1, :, :, 150:].any())
    print("inference chain: detections", det.count.tolist(), "mask pixels", int(got.sum()))
