"""``ops.propose_multilevel`` on the HIP path against tests/fpn_proposals_ref.py, on every named
case of tests/fpn_proposals_cases.py in fp32, float16 and bfloat16 (DESIGN.md §3 "FPN
proposals").  Needs an MI355X.

All six outputs are compared as bits with the reference on the widened inputs.  Every case runs
twice, the second time into caller-owned outputs with the workspace filled with 0xFF, and names
the kernels it reached."""
import numpy as np
import pytest
import torch

import fpn_proposals_cases as fc
from replication_faster_rcnn_amd import ops
from replication_faster_rcnn_amd.rpn import MultiLevelProposals

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f32": (torch.float32, "ElemF32"), "f16": (torch.float16, "ElemF16"), "bf16": (torch.bfloat16, "ElemBF16")}
NAMES = ("boxes", "logits", "levels", "anchor_idx", "count", "rois")


def device_inputs(case, dtype):
    o, d = case.inputs(dtype)
    return ([t.to(DEV) for t in o], [t.to(DEV) for t in d], [b.to(DEV) for b in case.bases],
            torch.from_numpy(case.image_sizes).to(DEV))


def call(case, dtype, **kw):
    o, d, b, s = device_inputs(case, dtype)
    return ops.propose_multilevel(o, d, b, case.strides, s, pre_nms_top_n=case.pre, post_nms_top_n=case.post,
                                  nms_thresh=case.nms_thresh, score_thresh=case.score_thresh, min_size=case.min_size,
                                  **kw)


def assert_bits(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu().numpy()
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        gv, wv = g.view(np.uint32), np.ascontiguousarray(w).view(np.uint32)
        bad = gv != wv
        assert not bad.any(), (f"{what}: {name}: {int(bad.sum())} of {bad.size} elements differ in their bits; first at "
                               f"{np.argwhere(bad)[0].tolist()}: {g[bad][0]!r} != {w[bad][0]!r}")


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", fc.CASES, ids=repr)
def test_case(case, dtype):
    dt, elem = DTYPES[dtype]
    want = case.reference(dt)
    if dt == torch.float32 and case.check is not None:
        case.check(case, want)
    name = ops.propose_multilevel_kernel([o.shape for o in case.objectness], dt, case.pre, case.post)
    assert name.startswith(f"fpn_select_decode_kernel<{elem}>[{','.join(case.branches)}] ")
    got = call(case, dt)
    assert_bits(got, want, f"{case.name} {dtype}")
    # again, into caller-owned outputs (pre-filled: every element must be stored) with a dirty workspace
    N, post = case.N, case.post
    outs = (torch.full((N, post, 4), 7.0, device=DEV), torch.full((N, post), 7.0, device=DEV),
            torch.full((N, post), 7, dtype=torch.int32, device=DEV), torch.full((N, post), 7, dtype=torch.int32, device=DEV),
            torch.full((N,), 7, dtype=torch.int32, device=DEV), torch.full((N * post, 5), 7.0, device=DEV))
    need = ops._fpn_cache[ops._fpn_shape_key("t", case.objectness, case.strides, case.pre, case.post)][4]
    ws = torch.full((need + 512,), 0xFF, dtype=torch.uint8, device=DEV)
    ws = ws[(-ws.data_ptr()) % 256:][:need]
    again = call(case, dt, out=outs, workspace=ws)
    assert all(a is b for a, b in zip(again, outs))
    assert_bits(again, want, f"{case.name} {dtype} (caller-owned outputs, 0xFF workspace)")


def test_no_host_sync():
    case = fc.BY_NAME["layout"]
    o, d, b, s = device_inputs(case, torch.float32)
    kw = dict(pre_nms_top_n=case.pre, post_nms_top_n=case.post)
    ops.propose_multilevel(o, d, b, case.strides, s, **kw)            # caches: parameters, workspace, threshold
    ops.propose_multilevel(o, d, b, case.strides, (44, 72), **kw)     # and the expanded host (h, w)
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = ops.propose_multilevel(o, d, b, case.strides, s, **kw)
        host = ops.propose_multilevel(o, d, b, case.strides, (44, 72), **kw)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert_bits(got, case.reference(), "under sync-debug")
    assert_bits(host, case.reference(), "host image size")


def test_wrapper_refusals():
    case = fc.BY_NAME["layout"]
    o, d, b, s = device_inputs(case, torch.float32)
    kw = dict(pre_nms_top_n=case.pre, post_nms_top_n=case.post)

    def refused(match, o=o, d=d, b=b, st=case.strides, s=s, **over):
        with pytest.raises(RuntimeError, match=match):
            ops.propose_multilevel(o, d, b, st, s, **{**kw, **over})

    refused(r"deltas\[1\]", d=[d[0], d[1].half(), d[2]])                              # mixed dtypes
    refused(r"objectness\[0\]", o=[o[0].double(), o[1], o[2]])
    refused(r"objectness\[2\]", o=[o[0], o[1], o[2].cpu()])
    refused(r"deltas\[0\]", d=[d[0].transpose(2, 3), d[1], d[2]])                     # a strided view
    refused(r"deltas\[1\]", d=[d[0], d[1][:, :8].contiguous(), d[2]])                 # 4K channels
    refused(r"objectness\[1\]", o=[o[0], o[1][:1].contiguous(), o[2]])                # another N
    refused(r"anchor_bases\[2\]", b=[b[0], b[1], b[2][:2].contiguous()])
    refused(r"anchor_bases\[0\]", b=[b[0].half(), b[1], b[2]])
    refused("anchor_bases", b=b[:2])
    refused("strides", st=case.strides[:2])
    refused(r"strides\[1\]", st=[(8, 10), (0, 20), (32, 40)])
    refused("image_sizes", s=s[:1].contiguous())
    refused("image_sizes", s=s.cpu())
    refused("image_sizes", s=(44,))
    refused("pre_nms_top_n", pre_nms_top_n=2049)
    refused("pre_nms_top_n", pre_nms_top_n=0)
    refused("post_nms_top_n", post_nms_top_n=4097)
    refused("objectness", o=[])
    refused("objectness", o=o * 3)
    outs = list(ops.propose_multilevel(o, d, b, case.strides, s, **kw))
    refused(r"out\[1\] \(logits\)", out=outs[:1] + [outs[1].double()] + outs[2:])
    refused(r"out\[5\] \(rois\)", out=outs[:5] + [outs[5][:-1]])
    refused("six outputs", out=outs[:5])
    refused("workspace", workspace=torch.empty(16, dtype=torch.uint8, device=DEV))
    refused("workspace", workspace=torch.empty(1 << 20, dtype=torch.uint8))


def test_module_modes_and_lists():
    case = fc.BY_NAME["layout"]
    o, d, b, s = device_inputs(case, torch.float32)
    m = MultiLevelProposals({"training": case.pre, "testing": 9}, {"training": case.post, "testing": 7}, case.nms_thresh)
    assert_bits(m(o, d, b, case.strides, s), case.reference(), "training mode")
    m.eval()
    want = case.reference(pre=9, post=7)
    assert_bits(m(o, d, b, case.strides, s), want, "testing mode")
    boxes, scores = m(o, d, b, case.strides, s, as_lists=True)
    assert len(boxes) == len(scores) == case.N
    for n in range(case.N):
        c = int(want[4][n])
        assert boxes[n].shape == (c, 4) and np.array_equal(boxes[n].cpu().numpy(), want[0][n, :c])
        assert torch.equal(scores[n].cpu(), torch.sigmoid(torch.from_numpy(want[1][n, :c].copy()).to(DEV)).cpu())
        assert (scores[n][:-1] >= scores[n][1:]).all()


def test_rois_feed_multiscale_roi_align():
    """The padded ``rois`` go into ``ops.multiscale_roi_align`` as they are: the rows of real
    proposals equal pooling the unpadded boxes, the padding rows are zeros."""
    case = fc.BY_NAME["layout"]
    post = 60                                   # above 3 x pre: padding rows in every image
    o, d, b, s = device_inputs(case, torch.float32)
    got = ops.propose_multilevel(o, d, b, case.strides, s, pre_nms_top_n=case.pre, post_nms_top_n=post)
    assert_bits(got, case.reference(post=post), "post = 60")
    boxes, count, rois = got[0], got[4].cpu().tolist(), got[5]
    assert min(count) > 0 and max(count) < post
    gen = torch.Generator().manual_seed(3)
    feats = [torch.randn(case.N, 4, h, w, generator=gen).to(DEV) for h, w in ((12, 18), (6, 9))]
    scales = (0.25, 0.125)
    pooled = ops.multiscale_roi_align(feats, rois, 3, scales, 2)
    assert pooled.shape == (case.N * post, 4, 3, 3)
    want = ops.multiscale_roi_align(feats, [boxes[n, :c] for n, c in enumerate(count)], 3, scales, 2)
    at = 0
    for n, c in enumerate(count):
        rows = pooled[n * post:(n + 1) * post]
        assert torch.equal(rows[:c].view(torch.int32), want[at:at + c].view(torch.int32)), n
        assert not rows[c:].view(torch.int32).any(), "a padding row pooled something"
        at += c
    assert bool(want.abs().sum() > 0)
