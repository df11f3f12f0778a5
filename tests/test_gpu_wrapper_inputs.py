"""What the Python wrappers accept.  Needs an MI355X.

Two rules (replication_faster_rcnn_amd/ops.py, targets.py):

* the hot-path ops on device tensors (``ops.propose``, ``ops.roi_transform``)
  convert nothing and raise RuntimeError, naming the argument, on anything but
  contiguous device tensors of the documented dtype and exact shape.  Every
  "raises" below is satisfied by an attribute check in Python that returns
  before any launch: no kernel ever sees the bad input;
* the reference-signature drop-ins (``utils.*``, ``ops.nms``, ``ops.roi_pool*``,
  ``region_proposal``, ``ops.rpn_head_epilogue``, ``targets.*``) convert strided
  views, other float types, numpy arrays and CPU / device tensors, with results
  identical to the call on contiguous copies of the kernels' dtypes, and raise
  on shapes that do not belong together.
"""
import numpy as np
import pytest
import torch

from oracle import ref_numpy as orc
from replication_faster_rcnn_amd import ops, synth, targets
from replication_faster_rcnn_amd import utils as U
from replication_faster_rcnn_amd.rpn import region_proposal

pytestmark = pytest.mark.gpu
DEV = "cuda"

FH, FW, IMG_H, IMG_W = 20, 30, 320, 480
N, A = 2, FH * FW * 9
_cache = {}


def rpn_inputs():
    """(anchors [A,4], scores [N,A], deltas [N,A,4]) numpy fp32, built once."""
    if "rpn" not in _cache:
        anchors = orc.generate_anchors(orc.generate_anchor_base(), 16, FW, FH)
        sc = np.stack([synth.rpn_scores(A, 21, i) for i in range(N)])
        de = np.stack([synth.rpn_deltas(A, 21, i) for i in range(N)])
        for a in (anchors, sc, de):
            a.setflags(write=False)
        _cache["rpn"] = (anchors, sc, de)
    return _cache["rpn"]


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


KW = dict(img_w=IMG_W, img_h=IMG_H, pre_nms=3000, post_nms=300)


# ------------------------------------------------------------------ ops.propose
def test_propose_rejects_views_dtypes_and_devices():
    anchors, sc, de = rpn_inputs()
    an, s, d = dev(anchors), dev(sc), dev(de)
    # the reference's cls_fg_softmax: a stride-2 view of the softmax
    logits = torch.stack([torch.log1p(-s), torch.log(s)], -1)
    fg = torch.softmax(logits, -1)[..., 1]
    assert fg.shape == s.shape and fg.stride() == (2 * A, 2)
    with pytest.raises(RuntimeError, match="scores"):
        ops.propose(fg, d, anchors=an, **KW)
    d_view = dev(np.ascontiguousarray(de.transpose(0, 2, 1))).permute(0, 2, 1)
    assert d_view.shape == d.shape and not d_view.is_contiguous()
    with pytest.raises(RuntimeError, match="deltas"):
        ops.propose(s, d_view, anchors=an, **KW)
    with pytest.raises(RuntimeError, match="scores"):
        ops.propose(s.double(), d, anchors=an, **KW)
    with pytest.raises(RuntimeError, match="deltas"):
        ops.propose(s, d.double(), anchors=an, **KW)
    with pytest.raises(RuntimeError, match="anchors"):
        ops.propose(s, d, anchors=an.half(), **KW)
    with pytest.raises(RuntimeError, match="scores"):
        ops.propose(s.cpu(), d.cpu(), anchors=an.cpu(), **KW)
    with pytest.raises(RuntimeError, match="deltas"):
        ops.propose(s, d.cpu(), anchors=an, **KW)
    with pytest.raises(RuntimeError, match="anchors"):
        ops.propose(s, d, anchors=torch.from_numpy(np.array(anchors)), **KW)
    # the same calls on contiguous fp32 device copies equal the oracle
    for sv, dv in [(fg.contiguous(), d), (s, d_view.contiguous()), (s.double().float(), d.double().float())]:
        rois, idx, cnt = ops.propose(sv, dv, anchors=an, **KW)
        for i in range(N):
            orois, oidx = orc.propose_one(anchors, sv[i].cpu().numpy(), dv[i].cpu().numpy(), IMG_W, IMG_H, 3000, 300)
            k = int(cnt[i])
            assert k == len(oidx)
            assert np.array_equal(idx[i, :k].cpu().numpy(), oidx) and np.array_equal(rois[i, :k].cpu().numpy(), orois)


def test_propose_rejects_shapes():
    anchors, sc, de = rpn_inputs()
    an, s, d = dev(anchors), dev(sc), dev(de)
    base = dev(orc.generate_anchor_base())
    grid = dict(feat_h=FH, feat_w=FW)
    with pytest.raises(RuntimeError, match="deltas"):
        ops.propose(s, d[:, :, :3].contiguous(), anchors=an, **KW)
    with pytest.raises(RuntimeError, match="deltas"):
        ops.propose(s, d[:, :A - 1].contiguous(), anchors=an, **KW)
    with pytest.raises(RuntimeError, match="deltas"):
        ops.propose(s, d[:1], anchors=an, **KW)
    with pytest.raises(RuntimeError, match="anchors"):
        ops.propose(s, d, anchors=an[:A - 1], **KW)
    with pytest.raises(RuntimeError, match="anchors"):
        ops.propose(s, d, anchors=an.reshape(-1), **KW)
    with pytest.raises(RuntimeError, match="anchor_base"):
        ops.propose(s, d, anchor_base=base[:, :3].contiguous(), **grid, **KW)
    with pytest.raises(RuntimeError, match="anchor_base"):
        ops.propose(s, d, anchor_base=base.t(), **grid, **KW)
    with pytest.raises(RuntimeError, match="feat_h"):
        ops.propose(s, d, anchor_base=base, feat_h=FH, feat_w=FW - 1, **KW)
    with pytest.raises(RuntimeError, match="anchors"):
        ops.propose(s, d, **KW)                         # neither anchors nor anchor_base
    with pytest.raises(RuntimeError, match="scores"):
        ops.propose(s[0], d, anchors=an, **KW)
    good = ops.propose(s, d, anchor_base=base, **grid, **KW)
    outs = [torch.empty_like(t) for t in good]
    with pytest.raises(RuntimeError, match=r"out\[0\]"):
        ops.propose(s, d, anchors=an, out=(outs[0][:, :299], outs[1], outs[2]), **KW)
    with pytest.raises(RuntimeError, match=r"out\[1\]"):
        ops.propose(s, d, anchors=an, out=(outs[0], outs[1].long(), outs[2]), **KW)
    with pytest.raises(RuntimeError, match=r"out\[2\]"):
        ops.propose(s, d, anchors=an, out=(outs[0], outs[1], outs[2].cpu()), **KW)
    with pytest.raises(RuntimeError, match="workspace"):
        ops.propose(s, d, anchors=an, workspace=torch.empty(16, dtype=torch.uint8, device=DEV), **KW)
    again = ops.propose(s, d, anchors=an, out=tuple(outs), **KW)     # and the good buffers still work
    for a, b in zip(good, again):
        assert torch.equal(a, b)


def test_roi_transform_rejects():
    rois = torch.rand(50, 4, device=DEV) * 300
    inds = torch.zeros(50, device=DEV)
    args = (IMG_H, IMG_W, FH, FW)
    want = orc.roi_transform(rois.cpu().numpy(), inds.cpu().numpy(), *args)
    assert np.array_equal(ops.roi_transform(rois, inds, *args).cpu().numpy(), want)
    wide = torch.rand(50, 8, device=DEV)
    for bad, name in [((wide[:, ::2], inds), "rois"), ((rois.double(), inds), "rois"), ((rois.cpu(), inds), "rois"),
                      ((rois[:, :3].contiguous(), inds), "rois"), ((rois.reshape(-1), inds), "rois"),
                      ((rois, inds.long()), "roi_inds"), ((rois, inds.cpu()), "roi_inds"),
                      ((rois, inds[:49]), "roi_inds"), ((rois, torch.zeros(100, device=DEV)[::2]), "roi_inds"),
                      ((rois, inds[:, None]), "roi_inds")]:
        with pytest.raises(RuntimeError, match=name):
            ops.roi_transform(*bad, *args)


# ------------------------------------------------- the converting drop-ins
def test_region_proposal_converts():
    anchors, sc, de = rpn_inputs()
    layer = region_proposal("test")
    want = layer(np.array(anchors), torch.from_numpy(np.array(sc[0])), torch.from_numpy(np.array(de[0])), IMG_W, IMG_H)
    assert want.device.type == "cpu" and want.dtype == torch.float32 and 0 < want.shape[0] <= 300
    orois, _ = orc.propose_one(anchors, sc[0], de[0], IMG_W, IMG_H, 3000, 300)
    assert np.array_equal(want.numpy(), orois)
    s2 = torch.from_numpy(np.stack([sc[1], sc[0]], -1))[:, 1]                    # the stride-2 slice
    d_t = torch.from_numpy(np.ascontiguousarray(de[0].T)).t()
    a_wide = torch.from_numpy(np.repeat(anchors, 2, axis=1))[:, ::2]
    assert not (s2.is_contiguous() or d_t.is_contiguous() or a_wide.is_contiguous())
    got = layer(a_wide, s2, d_t, IMG_W, IMG_H)
    assert got.device.type == "cpu" and torch.equal(got, want)
    got = layer(anchors.astype(np.float64), s2.double(), d_t.double(), IMG_W, IMG_H)   # fp32 values in fp64
    assert got.dtype == torch.float32 and torch.equal(got, want)
    s16, d16 = s2.half(), d_t.half()                                             # fp16: converted, ties and all
    assert torch.equal(layer(a_wide, s16, d16, IMG_W, IMG_H),
                       layer(np.array(anchors), s16.float().contiguous(), d16.float().contiguous(), IMG_W, IMG_H))
    got = layer(a_wide.to(DEV), s2.to(DEV), d_t.to(DEV), IMG_W, IMG_H)
    assert got.is_cuda and torch.equal(got.cpu(), want)                          # lands on reg's device


def test_reg2bbox_converts():
    anchors, _, de = rpn_inputs()
    a16 = torch.from_numpy(np.array(anchors)).half()             # fp16 inputs: converted, never reinterpreted
    d16 = torch.from_numpy(np.array(de[0])).half()
    want = U.reg2bbox(a16.float(), d16.float())
    assert want.device.type == "cpu" and np.array_equal(want.numpy(), orc.reg2bbox(a16.float().numpy(),
                                                                                    d16.float().numpy()))
    assert torch.equal(U.reg2bbox(a16, d16), want)
    assert torch.equal(U.reg2bbox(a16.double(), d16.double()), want)
    got = U.reg2bbox(a16.numpy(), d16.to(DEV))
    assert got.is_cuda and torch.equal(got.cpu(), want)
    with pytest.raises(RuntimeError, match="reg2bbox"):
        U.reg2bbox(a16[:-1], d16)


def test_nms_converts():
    r = np.random.default_rng(8)
    xy = r.uniform(0, 100, (300, 2))
    b16 = torch.from_numpy(np.concatenate([xy, xy + r.uniform(5, 40, (300, 2))], 1)).half()
    s16 = torch.from_numpy(r.permutation(300) / 300).half()
    b, s = b16.float(), s16.float()
    want = ops.nms(b, s, 0.5)
    assert want.device.type == "cpu" and want.dtype == torch.int64
    assert np.array_equal(want.numpy(), orc.nms(b.numpy(), s.numpy(), 0.5)) and 0 < len(want) < 300
    wide_b = torch.repeat_interleave(b, 2, dim=1)[:, ::2]
    wide_s = torch.stack([s, -s], 1)[:, 0]
    assert not (wide_b.is_contiguous() or wide_s.is_contiguous())
    for bb, ss in [(wide_b, wide_s), (b16, s16), (b.double(), s.double()), (b, s16), (wide_b.double(), s)]:
        got = ops.nms(bb, ss, 0.5)
        assert got.device.type == "cpu" and torch.equal(got, want)
        got = ops.nms(bb.to(DEV), ss.to(DEV), 0.5)
        assert got.is_cuda and torch.equal(got.cpu(), want)
    got = ops.nms(b.to(DEV), s, 0.5)                   # mixed devices: the result follows boxes
    assert got.is_cuda and torch.equal(got.cpu(), want)
    with pytest.raises(RuntimeError):
        ops.nms(b, s[:-1], 0.5)
    with pytest.raises(RuntimeError):
        ops.nms(b[:, :3], s, 0.5)


def test_bbox_iou_converts():
    """Strided views, tensors and device tensors equal the contiguous numpy call
    of the same dtype; numpy out, as the reference returns."""
    r = np.random.default_rng(9)
    xy = r.uniform(0, 100, (70, 2))
    a = np.concatenate([xy, xy + r.uniform(5, 40, (70, 2))], 1)
    b = a[::-1][:33].copy() + 3
    for ta, tb in [(np.float32, np.float32), (np.float64, np.float32), (np.float64, np.float64)]:
        aa, bb = a.astype(ta), b.astype(tb)
        want = U.bbox_iou(aa, bb)
        with np.errstate(all="ignore"):
            np.testing.assert_array_equal(want, orc.bbox_iou(aa, bb))
        wa, wb = np.repeat(aa, 2, axis=1)[:, ::2], np.repeat(bb, 3, axis=0)[::3]
        assert not (wa.flags.c_contiguous or wb.flags.c_contiguous)
        for x, y in [(wa, wb), (torch.from_numpy(wa), torch.from_numpy(wb)),
                     (torch.from_numpy(wa).to(DEV), torch.from_numpy(bb).to(DEV))]:
            got = U.bbox_iou(x, y)
            assert isinstance(got, np.ndarray) and got.dtype == want.dtype
            np.testing.assert_array_equal(got, want)
    with pytest.raises(IndexError):
        U.bbox_iou(a[:, :3], b)
    with pytest.raises(RuntimeError, match="bbox2reg"):
        U.bbox2reg(a[:5], b[:4])


# ------------------------------------------------------------------- roi_pool
def _pool_inputs():
    C, R = 8, 64
    x = np.stack([synth.features(C, FH, FW, 22, i) for i in range(N)])
    r = np.random.default_rng(10)
    tl = r.uniform(-2, 20, (R, 2))
    boxes = np.concatenate([np.sort(r.integers(0, N, R))[:, None], tl, tl + r.uniform(0.5, 12, (R, 2))], 1)
    return x, boxes.astype(np.float32)


def test_roi_pool_input_layouts():
    x, boxes = _pool_inputs()
    oo, oa = orc.roi_pool_forward(x, boxes, 7, 1.0)
    xt, bt = torch.from_numpy(x).to(DEV), torch.from_numpy(boxes).to(DEV)
    cl = xt.contiguous(memory_format=torch.channels_last)
    wide = torch.repeat_interleave(xt, 2, dim=1)[:, ::2]
    assert not cl.is_contiguous() and not wide.is_contiguous() and torch.equal(wide, xt)
    for xin in (cl, wide, xt.double(), xt.cpu()):
        out, am = ops.roi_pool_with_argmax(xin, bt, 7, 1.0)
        assert out.device == xin.device and out.dtype == torch.float32
        assert np.array_equal(out.cpu().numpy(), oo) and np.array_equal(am.cpu().numpy(), oa)
    # torchvision's list-of-tensors form of boxes == the [K, 5] form
    per_image = [bt[bt[:, 0] == i, 1:] for i in range(N)]
    assert sum(len(p) for p in per_image) == len(bt) and all(len(p) for p in per_image)
    out_l, am_l = ops.roi_pool_with_argmax(xt, per_image, 7, 1.0)
    assert np.array_equal(out_l.cpu().numpy(), oo) and np.array_equal(am_l.cpu().numpy(), oa)
    out_v, _ = ops.roi_pool_with_argmax(xt, torch.repeat_interleave(bt, 2, dim=1)[:, ::2], (7, 7), 1.0)
    assert np.array_equal(out_v.cpu().numpy(), oo)
    with pytest.raises(RuntimeError):
        ops.roi_pool_with_argmax(xt, bt[:, :4], 7, 1.0)
    with pytest.raises(RuntimeError):
        ops.roi_pool_with_argmax(xt[0], bt, 7, 1.0)


def test_roi_pool_backward_of_sum():
    """out.sum().backward() hands the backward an expanded, stride-0 gradient."""
    x, boxes = _pool_inputs()
    _, oa = orc.roi_pool_forward(x, boxes, 7, 1.0)
    want = orc.roi_pool_backward(np.ones((len(boxes), x.shape[1], 7, 7), np.float32), boxes, oa, x.shape)
    xg = torch.from_numpy(x).to(DEV).requires_grad_(True)
    out = ops.roi_pool(xg, torch.from_numpy(boxes).to(DEV), 7, 1.0)
    out.sum().backward()
    assert np.array_equal(xg.grad.cpu().numpy(), want)
    # the same through a channels_last leaf
    xc = torch.from_numpy(x).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    ops.roi_pool(xc, torch.from_numpy(boxes).to(DEV), 7, 1.0).sum().backward()
    assert np.array_equal(xc.grad.cpu().numpy(), want)


def test_rpn_head_epilogue_channels_last():
    g = torch.Generator().manual_seed(3)
    K, H, W = 9, 5, 7
    cls = torch.randn(N, 2 * K, H, W, generator=g).to(DEV)
    reg = torch.randn(N, 4 * K, H, W, generator=g).to(DEV)
    want = ops.rpn_head_epilogue(cls, reg, K)
    oc, ofg, orr = orc.rpn_head_epilogue(cls.cpu().numpy(), reg.cpu().numpy())
    assert np.array_equal(want[0].cpu().numpy(), oc) and np.array_equal(want[1].cpu().numpy(), ofg)
    assert np.array_equal(want[2].cpu().numpy(), orr)
    cl_c, cl_r = cls.contiguous(memory_format=torch.channels_last), reg.contiguous(memory_format=torch.channels_last)
    assert not cl_c.is_contiguous() and not cl_r.is_contiguous()
    for c, r in [(cl_c, cl_r), (cl_c, reg), (cls.double(), cl_r.double())]:
        got = ops.rpn_head_epilogue(c, r, K)
        for a, b in zip(got, want):
            assert torch.equal(a, b)


# -------------------------------------------------------------------- targets
def _target_inputs():
    anchors = rpn_inputs()[0]
    G = 8
    boxes = np.zeros((N, G, 4))
    labels = np.zeros((N, G))
    for i in range(N):
        boxes[i], labels[i] = synth.gt_boxes(IMG_H, IMG_W, G, 23, i, (5, 3)[i])
    r = np.random.default_rng(11)
    Rp = 200
    tl = r.uniform(0, 250, (N, Rp, 2))
    rois = np.concatenate([tl, tl + r.uniform(16, 200, (N, Rp, 2))], 2).astype(np.float32)
    for i in range(N):           # some proposals on the gt, so that there are positives
        v = labels[i] != -1
        rois[i, :v.sum()] = boxes[i, v] + 1
    rcount = np.array([Rp, Rp - 37], np.int32)
    return anchors, boxes, labels, rois, rcount


def _run(fn):
    np.random.seed(5)
    out = fn()
    st = np.random.get_state()
    return [t.cpu().numpy() for t in out], (st[1].copy(), st[2])


def _same(got, want):
    for a, b in zip(got[0], want[0]):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
    assert got[1][1] == want[1][1] and np.array_equal(got[1][0], want[1][0]), "RNG state"


def _input_forms(boxes, labels):
    b32 = boxes.astype(np.float32)                                 # np.around-ed pixels: exact in fp32
    assert np.array_equal(b32.astype(np.float64), boxes)
    wide = torch.from_numpy(np.repeat(boxes, 2, axis=2))[:, :, ::2]
    lab_v = torch.from_numpy(np.repeat(labels, 2, axis=1))[:, ::2]
    assert not wide.is_contiguous() and not lab_v.is_contiguous()
    return [(wide, lab_v), (b32, labels.astype(np.float32)), (torch.from_numpy(b32).to(DEV), labels),
            (torch.from_numpy(boxes).to(DEV), torch.from_numpy(labels).to(DEV).int())]


def test_anchor_targets_input_forms(rng_guard):
    anchors, boxes, labels, _, _ = _target_inputs()
    want = _run(lambda: targets.anchor_targets(boxes, labels, torch.from_numpy(np.array(anchors)), internals=True))
    assert (want[0][1] == 1).any() and (want[0][1] == 0).any()
    a_wide = torch.from_numpy(np.repeat(anchors, 2, axis=1))[:, ::2]
    forms = _input_forms(boxes, labels)
    for (b, l), a in zip(forms, [a_wide, anchors.astype(np.float64), a_wide.to(DEV), np.array(anchors).tolist()]):
        _same(_run(lambda: targets.anchor_targets(b, l, a, internals=True)), want)
    # the prepare / sample split takes the same forms
    b, l = forms[0]
    got = _run(lambda: targets.anchor_targets_sample(targets.anchor_targets_prepare(b, l, a_wide)))
    _same((got[0], got[1]), (want[0][:2], want[1]))


def test_proposal_targets_input_forms(rng_guard):
    _, boxes, labels, rois, rcount = _target_inputs()
    want = _run(lambda: targets.proposal_targets(torch.from_numpy(rois), torch.from_numpy(rcount), boxes, labels))
    assert (want[0][3] > 0).all() and (want[0][2] != 0).any()       # samples drawn, some of them positive
    padded = np.concatenate([rois, np.full((N, 9, 4), 7.0, np.float32)], 1)
    r_view = torch.from_numpy(padded)[:, :rois.shape[1]]            # a sliced view of a longer buffer
    assert not r_view.is_contiguous()
    forms = _input_forms(boxes, labels)
    roi_forms = [(r_view, torch.from_numpy(rcount)), (rois, rcount), (r_view.to(DEV), torch.from_numpy(rcount).long()),
                 (torch.from_numpy(rois).double(), rcount.astype(np.int64))]
    for (b, l), (r, c) in zip(forms, roi_forms):
        _same(_run(lambda: targets.proposal_targets(r, c, b, l)), want)
    b, l = forms[0]

    def split():
        plan = targets.proposal_targets_prepare(r_view, rcount, b, l)
        count = targets.proposal_targets_draw(plan)
        return tuple(targets.proposal_targets_finish(plan, count)) + (count,)

    _same(_run(split), want)


def test_targets_reject_mismatches(rng_guard):
    anchors, boxes, labels, rois, rcount = _target_inputs()
    r, c = torch.from_numpy(rois), torch.from_numpy(rcount)
    before = np.random.get_state()
    for fn in (targets.proposal_targets, targets.proposal_targets_prepare):
        with pytest.raises(RuntimeError, match="rois"):
            fn(torch.cat([r, r[:1]]), c, boxes, labels)               # rois for 3 images, boxes for 2
        with pytest.raises(RuntimeError, match="rcount"):
            fn(r, torch.cat([c, c[:1]]), boxes, labels)
        with pytest.raises(RuntimeError, match="rcount"):
            fn(r, c[:1], boxes, labels)
        with pytest.raises(RuntimeError, match="rois"):
            fn(r[:, :, :3], c, boxes, labels)
        with pytest.raises(RuntimeError, match="rois"):
            fn(r[0], c, boxes, labels)
        with pytest.raises(RuntimeError, match="labels"):
            fn(r, c, boxes, labels[:, :-1])
    for fn in (targets.anchor_targets, targets.anchor_targets_prepare):
        with pytest.raises(RuntimeError, match="anchors"):
            fn(boxes, labels, anchors[:, :3])
        with pytest.raises(RuntimeError, match="anchors"):
            fn(boxes, labels, anchors.reshape(-1))
        with pytest.raises(RuntimeError, match="anchors"):
            fn(boxes, labels, anchors[None])
        with pytest.raises(RuntimeError, match="boxes"):
            fn(boxes[0], labels, anchors)
    # caller-owned out= buffers of another shape, dtype, device or layout
    plan = targets.anchor_targets_prepare(boxes, labels, anchors)
    reg = torch.empty((N, A, 4), dtype=torch.float64, device=DEV)
    lab = torch.empty((N, A), dtype=torch.int32, device=DEV)
    bad = [(reg[:, :-1], lab), (reg, lab.long()), (reg.float(), lab), (reg.cpu(), lab), (reg, lab.t().contiguous().t()),
           (reg,)]
    for fn in (targets.anchor_targets_sample, targets.anchor_targets_finish):
        for out in bad:
            with pytest.raises(RuntimeError, match="out buffers"):
                fn(plan, out=out)
    pplan = targets.proposal_targets_prepare(r, c, boxes, labels)
    S = 128
    good = (torch.empty((N, S, 4), dtype=torch.float64, device=DEV), torch.empty((N, S, 4), dtype=torch.float64, device=DEV),
            torch.empty((N, S), dtype=torch.float64, device=DEV), torch.empty((N,), dtype=torch.int32, device=DEV))
    for k, wrong in enumerate([good[0][:, :-1], good[1].float(), good[2].cpu(), good[3].long()]):
        out = tuple(wrong if j == k else t for j, t in enumerate(good))
        with pytest.raises(RuntimeError, match="out buffers"):
            targets.proposal_targets_sample(pplan, out=out)
        if k < 3:
            with pytest.raises(RuntimeError, match="out buffers"):
                targets.proposal_targets_finish(pplan, good[3], out=out[:3])
    with pytest.raises(RuntimeError, match="count"):
        targets.proposal_targets_finish(pplan, good[3].long())
    after = np.random.get_state()
    assert before[2] == after[2] and np.array_equal(before[1], after[1]), "a rejected call draws nothing"
