"""``ops.box_head_detections`` / ``heads.BoxHeadDetections`` on the HIP path against
tests/box_detections_ref.py, on every named case of tests/box_detections_cases.py (DESIGN.md §3
"Pyramid box-head inference").  Needs an MI355X.

All six outputs are compared as bits, in fp32 on every case and in float16 / bfloat16 on the
cases whose inputs those types hold exactly.  Every case names its launch plan first and runs
twice, the second time into caller-owned outputs pre-filled with 7 with an exact, 256-byte
aligned workspace filled with 0xFF."""
import numpy as np
import pytest
import torch

import box_detections_cases as bc
import box_detections_ref as ref_mod
from replication_faster_rcnn_amd import ops
from replication_faster_rcnn_amd.evaluate import COCOEvaluator
from replication_faster_rcnn_amd.heads import BoxHeadDetections

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
RUNS = [(c, "f32") for c in bc.CASES] + [(c, d) for c in bc.HALF for d in ("f16", "bf16")]


def device_inputs(case, dtype="f32"):
    dt = DTYPES[dtype]
    lg, rg, p, pc, sz = (torch.tensor(a).to(DEV) for a in (case.logits, case.reg, case.proposals, case.prop_count,
                                                            case.image_sizes))
    return lg.to(dt), rg.to(dt), p, pc, sz


def call(case, dtype="f32", **kw):
    orig = None if case.original_sizes is None else torch.tensor(case.original_sizes).to(DEV)
    return ops.box_head_detections(*device_inputs(case, dtype), original_sizes=orig, **{**case.kw, **kw})


def assert_bits(got, want, what):
    assert ops.BoxDetections._fields == bc.OUT
    bc.same_bits([g.cpu().numpy() for g in got], want, what)


@pytest.mark.parametrize("case,dtype", RUNS, ids=lambda v: v if isinstance(v, str) else repr(v))
def test_case(case, dtype):
    want = case.reference()         # 16-bit inputs widen to the fp32 inputs bit for bit
    assert ops.box_head_detections_kernel(case.R, case.C, case.D, DTYPES[dtype]) == bc.plan_name(case.R, dtype)
    assert case.plan in ops.box_head_detections_kernel(case.R, case.C, case.D, DTYPES[dtype])
    got = call(case, dtype)
    assert isinstance(got, ops.BoxDetections)
    assert_bits(got, want, f"{case.name} {dtype}")
    # again, into caller-owned outputs (pre-filled: every element must be stored) with a dirty workspace
    N, D = case.N, case.D
    i32 = dict(dtype=torch.int32, device=DEV)
    outs = (torch.full((N, D, 4), 7.0, device=DEV), torch.full((N, D), 7, **i32), torch.full((N, D), 7.0, device=DEV),
            torch.full((N, D), 7, **i32), torch.full((N,), 7, **i32), torch.full((N,), 7, **i32))
    need = ops._bd_ws[(N, case.R, case.C)]
    ws = torch.full((need + 512,), 0xFF, dtype=torch.uint8, device=DEV)
    ws = ws[(-ws.data_ptr()) % 256:][:need]
    assert ws.data_ptr() % 256 == 0 and ws.numel() == need
    again = call(case, dtype, out=outs, workspace=ws)
    assert all(a is b for a, b in zip(again, outs))
    assert_bits(again, want, f"{case.name} {dtype} (caller-owned outputs, 0xFF workspace)")


def test_host_image_size_and_module():
    """One host (h, w) for every image, through ``heads.BoxHeadDetections``."""
    case = bc.BY_NAME["c128_both"]
    lg, rg, p, pc, _ = device_inputs(case)
    m = BoxHeadDetections(score_thresh=case.kw["score_thresh"], detections_per_img=case.D)
    got = m(lg, rg, p, pc, (bc.IMG_H, bc.IMG_W))
    assert_bits(got, case.reference(), "module, host image size")


def test_two_calls_same_bits_and_no_host_sync():
    case = bc.BY_NAME["D1024"]
    ins = device_inputs(case)
    first = ops.box_head_detections(*ins, **case.kw)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = ops.box_head_detections(*ins, **case.kw)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert_bits(second, [a.cpu().numpy() for a in first], "second call")
    assert_bits(second, case.reference(), "under sync-debug")


def test_refusals():
    """Each limit, mixed dtypes, host tensors, strided views and a small workspace raise a
    RuntimeError naming the argument before any launch."""
    case = bc.BY_NAME["c2"]
    lg, rg, p, pc, sz = device_inputs(case)
    N, R, C = case.N, case.R, case.C

    def refused(match, lg=lg, rg=rg, p=p, pc=pc, sz=sz, **over):
        with pytest.raises(RuntimeError, match=match):
            ops.box_head_detections(lg, rg, p, pc, sz, **over)

    refused("box_regression", rg=rg.half())                                    # mixed dtypes
    refused("class_logits", lg=lg.double(), rg=rg.double())
    refused("class_logits", lg=lg.cpu())
    refused("box_regression", rg=rg.cpu())
    refused("class_logits", lg=lg.t().contiguous().t())                        # a strided view
    refused("class_logits", lg=lg[:-1])
    refused("box_regression", rg=rg[:, :-4].contiguous())
    refused("C must", lg=torch.zeros(N * R, 1, device=DEV), rg=torch.zeros(N * R, 4, device=DEV))
    refused("C must", lg=torch.zeros(N * R, 129, device=DEV), rg=torch.zeros(N * R, 516, device=DEV))
    refused("proposals", p=p.double())
    refused("proposals", p=p.cpu())
    refused("proposals", p=p[:, :, :3].contiguous())
    refused("R must", p=torch.zeros(1, 4097, 4, device=DEV))
    refused("R must", p=torch.zeros(1, 0, 4, device=DEV))
    refused("N must", p=torch.zeros(1025, 1, 4, device=DEV))
    refused("prop_count", pc=pc.long())
    refused("prop_count", pc=pc.cpu())
    refused("image_sizes", sz=sz.double())
    refused("image_sizes", sz=(1.0, 2.0, 3.0))
    refused("original_sizes", original_sizes=sz.cpu())
    refused("original_sizes", original_sizes=sz[:, :1].contiguous())
    refused("detections_per_img", detections_per_img=0)
    refused("detections_per_img", detections_per_img=1025)
    refused("reg_weights", reg_weights=(1.0, 1.0, 0.0, 1.0))
    refused("reg_weights", reg_weights=(1.0, 1.0, 1.0))
    refused("reg_weights", reg_weights=(1.0, 1.0, float("inf"), 1.0))
    refused("reg_weights", reg_weights=(1.0, float("nan"), 1.0, 1.0))
    outs = list(ops.box_head_detections(lg, rg, p, pc, sz))
    before = [o.clone() for o in outs]
    refused(r"out\[0\] \(boxes\)", out=[outs[0].double()] + outs[1:])
    refused(r"out\[3\] \(roi\)", out=outs[:3] + [outs[3][:, :-1]] + outs[4:])
    refused("six outputs", out=outs[:5])
    need = ops._bd_ws[(N, R, C)]
    refused("workspace", workspace=torch.empty(need - 1, dtype=torch.uint8, device=DEV))
    refused("workspace", workspace=torch.empty(need, dtype=torch.uint8))
    # the C-ABI itself: a small workspace and a bad limit come back before any launch
    from replication_faster_rcnn_amd import _lib
    lib = _lib.load()
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def rc_of(ws_bytes=need, D=100, ww=5.0):
        return lib.frcnn_box_detections_t(0, N, R, C, lg.data_ptr(), rg.data_ptr(), p.data_ptr(), pc.data_ptr(), sz.data_ptr(),
                                          None, 0.05, 0.5, D, 0.01, 10.0, 10.0, ww, 5.0, *[t.data_ptr() for t in outs],
                                          ws.data_ptr(), ws_bytes, None)
    for o in outs:
        o.fill_(7)
    assert rc_of(ws_bytes=need - 1) == -3 and b"workspace" in lib.frcnn_last_error()
    assert rc_of(D=1025) == -1 and b"detections_per_img" in lib.frcnn_last_error()
    assert rc_of(ww=0.0) == -1 and b"reg_weights" in lib.frcnn_last_error()
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)                             # nothing was launched
    assert rc_of() == 0
    assert_bits(outs, [b.cpu().numpy() for b in before], "the C-ABI call")


def test_chain_detects_end_to_end():
    """propose_multilevel -> multiscale_roi_align -> one Linear per prediction -> BoxHeadDetections
    -> COCOEvaluator, on a tiny pyramid: the detections are the restatement's on the head's own
    outputs, and the evaluator fed either gives the same numbers."""
    torch.manual_seed(0)
    N, Cf, K, C, post, D = 2, 8, 3, 3, 24, 10
    grids, strides = ((16, 24), (8, 12)), ((4, 4), (8, 8))
    bases = [b.to(DEV) for b in ops.pyramid_anchor_bases(((8,), (16,)), (0.5, 1.0, 2.0))]
    feats = [torch.randn(N, Cf, h, w, device=DEV) for h, w in grids]
    rpn_cls = torch.nn.Conv2d(Cf, K, 1).to(DEV)
    rpn_reg = torch.nn.Conv2d(Cf, 4 * K, 1).to(DEV)
    fc_cls = torch.nn.Linear(Cf * 4, C).to(DEV)
    fc_reg = torch.nn.Linear(Cf * 4, 4 * C).to(DEV)
    sizes = torch.tensor([[64.0, 96.0], [60.0, 90.0]], device=DEV)
    orig = torch.tensor([[128.0, 192.0], [100.0, 150.0]], device=DEV)
    with torch.no_grad():
        objectness, deltas = [rpn_cls(f) for f in feats], [0.1 * rpn_reg(f) for f in feats]
        boxes, _, _, _, count, rois = ops.propose_multilevel(objectness, deltas, bases, strides, sizes, pre_nms_top_n=200,
                                                             post_nms_top_n=post)
        flat = ops.multiscale_roi_align(feats, rois, 2, (1 / 4, 1 / 8), 2).flatten(1)
        logits, regs = 2.0 * fc_cls(flat), fc_reg(flat)
    head = BoxHeadDetections(detections_per_img=D)
    got = head(logits, regs, boxes, count, sizes, orig)
    want = ref_mod.box_detections(logits.cpu().numpy(), regs.cpu().numpy(), boxes.cpu().numpy(), count.cpu().numpy(),
                                  sizes.cpu().numpy(), detections_per_img=D, original_sizes=orig.cpu().numpy())
    assert_bits(got, want, "end to end")
    assert int(got.count.min()) > 0 and int(count.min()) > 0
    k = [int(v) for v in got.count]
    gt = np.zeros((N, 3, 4), np.float64)
    gl = np.zeros((N, 3), np.int32)
    for n in range(N):             # a detection of each image as ground truth, and a box nothing detects
        gt[n, 0], gl[n, 0] = want[0][n, 0], want[1][n, 0]
        gt[n, 1], gl[n, 1] = want[0][n, k[n] - 1], want[1][n, k[n] - 1]
        gt[n, 2], gl[n, 2] = (1.0, 1.0, 3.0, 3.0), 1
    res = []
    for det in (got, tuple(torch.from_numpy(a).to(DEV) for a in want)):
        ev = COCOEvaluator(n_class=C, capacity=1 << 10)
        ev.update(det, gt, gl)
        res.append(ev.result())
    assert res[0]["n_records"] == sum(k) and res[0]["n_images"] == N
    assert np.array_equal(res[0]["stats"], res[1]["stats"], equal_nan=True)
    assert np.array_equal(res[0]["precision"], res[1]["precision"]) and 0.0 < res[0]["AP"] <= 1.0
    print("end to end: proposals", count.tolist(), "detections", k, "AP", round(res[0]["AP"], 4))
