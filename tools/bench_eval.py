"""Time the evaluation stage (ops.eval_update per batch, VOCEvaluator.result per
dataset) against what a user could write without it: a per-batch .cpu() of the
detections and the devkit loop on the host (tests/eval_ref.py), then the AP on
the host.

    python tools/bench_eval.py [--out profiles/eval_bench.json]

Workload: the output of ops.detect on synth.head_outputs at the cfg2 detection
shape (N=8, R=300, C=21, 600x1000, score_thresh 0.05), with 8 gt slots per
image: four from synth.gt_boxes and four copied from the image's detections, one
of them difficult.  eval_update and its baseline are timed with device events
in one process, interleaved: per repetition --calls updates, then
--baseline-calls host updates; 5 repetitions, min and median reported.
result() is timed over 4,952 images' worth of records (the VOC2007 test set:
619 updates of the batch), against the host AP over the same records.  Before
timing, the device state and APs must equal the numpy restatement of the
contract.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SHAPE = dict(N=8, R=300, C=21, img_h=600, img_w=1000, seed=0)
SCORE_THRESH = 0.05
G = 8
DATASET_IMAGES = 4952
CFG2_STEP_US = 78.0   # the whole cfg2 step (8 images at ~102k images/s), for the share only


def workload():
    import numpy as np
    import torch
    from replication_faster_rcnn_amd import ops, synth
    dev = [torch.from_numpy(a).cuda() for a in synth.head_outputs(**SHAPE)]
    det = ops.detect(*dev, img_h=SHAPE["img_h"], img_w=SHAPE["img_w"], score_thresh=SCORE_THRESH)
    boxes, labels, _, _, count, _ = (t.cpu().numpy() for t in det)
    N = SHAPE["N"]
    gb, gl, gd = -np.ones((N, G, 4)), -np.ones((N, G), np.int32), np.zeros((N, G), np.uint8)
    for n in range(N):
        b, l = synth.gt_boxes(SHAPE["img_h"], SHAPE["img_w"], 4, SHAPE["seed"], n)
        gb[n, :4], gl[n, :4] = b, l.astype(np.int32)
        for i in range(4):
            s = i * int(count[n]) // 4
            gb[n, 4 + i], gl[n, 4 + i] = boxes[n, s].astype(np.float64), labels[n, s]
        gd[n, 5] = 1
    det4 = (det[0], det[1], det[2], det[4])
    return det4, (gb, gl, gd), [torch.from_numpy(a).cuda() for a in (gb, gl, gd)]


def timed(fn, calls):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls   # us per call


def summary(v):
    return dict(reps_us=[round(x, 2) for x in v], min_us=round(min(v), 2), median_us=round(statistics.median(v), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.json"))
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--baseline-calls", type=int, default=3)
    ap.add_argument("--result-calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.calls < 200 or args.reps < 5:
        ap.error("--calls >= 200 and --reps >= 5")

    import numpy as np
    import torch
    import eval_ref
    from replication_faster_rcnn_amd import ops
    from replication_faster_rcnn_amd.evaluate import VOCEvaluator

    det, gt_host, gt_dev = workload()
    C, N = SHAPE["C"], SHAPE["N"]
    M = det[1].shape[1]
    per_batch = int(det[3].clamp(0, M).sum().item())
    updates = -(-DATASET_IMAGES // N)
    assert max(args.calls, updates) * per_batch <= ops.EVAL_MAX_CAPACITY

    def host_update(state):
        d = [t.cpu().numpy() for t in det]               # the per-batch copy to the host
        state.update(*d, *gt_host)

    # the op equals the contract: one update, records and both APs
    ref = eval_ref.State(C, per_batch)
    host_update(ref)
    state = ops.eval_state(C, args.calls * per_batch)
    ops.eval_update(det, *gt_dev, state=state)
    hdr, key, flag, image = (t.cpu().numpy() for t in state)
    assert np.array_equal(hdr, ref.hdr) and np.array_equal(key[:per_batch].view(np.uint64), ref.rec_key)
    assert np.array_equal(flag[:per_batch], ref.rec_flag) and np.array_equal(image[:per_batch], ref.rec_image)
    for use_07 in (True, False):
        got = ops.eval_ap(state, per_batch, use_07_metric=use_07)[0].cpu().numpy()
        want, _, _, nper = ref.ap(use_07_metric=use_07)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert (np.isnan(want) | (np.abs(got - want) <= (0 if use_07 else 1) * nper * 2.0 ** -52)).all()

    op = lambda: ops.eval_update(det, *gt_dev, state=state)             # noqa: E731
    base_state = eval_ref.State(C, (args.baseline_calls + 1) * per_batch)
    base = lambda: host_update(base_state)                              # noqa: E731
    for _ in range(args.warmup):
        op()
    t_op, t_base = [], []
    for _ in range(args.reps):
        state[0].zero_()
        t_op.append(timed(op, args.calls))
        assert int(state[0][0].item()) == args.calls * per_batch and int(state[0][2].item()) == 0
        base_state.hdr[:] = 0
        t_base.append(timed(base, args.baseline_calls))
    flags = ref.rec_flag
    result = dict(workload=dict(SHAPE, score_thresh=SCORE_THRESH, gt_slots=G, max_det=M, generator="synth.head_outputs "
                                "-> ops.detect; gt: synth.gt_boxes + detections"),
                  device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
                  records_per_update=per_batch,
                  flags_per_update=dict(tp=int((flags == 1).sum()), fp=int((flags == 0).sum()),
                                        ignored=int((flags == -1).sum())),
                  update=dict(calls_per_rep=args.calls, baseline_calls_per_rep=args.baseline_calls,
                              baseline=".cpu() of the detections + tests/eval_ref.py's devkit loop on the host",
                              op=summary(t_op), baseline_times=summary(t_base),
                              ratio_min_over_min=round(min(t_base) / min(t_op), 1),
                              op_share_of_cfg2_step=round(min(t_op) / CFG2_STEP_US, 3)))
    print(f"update: op {result['update']['op']['min_us']} us min / {result['update']['op']['median_us']} median, "
          f"baseline {result['update']['baseline_times']['min_us']} / "
          f"{result['update']['baseline_times']['median_us']} us, {per_batch} records per update", flush=True)

    # result() over a dataset's worth of records
    ev = VOCEvaluator(n_class=C, capacity=updates * per_batch)
    for _ in range(updates):
        ev.update(det, *gt_dev)
    first = ev.result()
    assert first["n_records"] == updates * per_batch and first["n_images"] == updates * N
    host_state = eval_ref.State(C, 1)
    host_state.hdr, host_state.rec_key, host_state.rec_flag = (
        ev.state[0].cpu().numpy(), ev.state[1].cpu().numpy().view(np.uint64), ev.state[2].cpu().numpy())
    want, wmean, _, nper = host_state.ap()
    assert np.array_equal(np.isnan(first["ap"]), np.isnan(want))
    assert (np.isnan(want) | (np.abs(first["ap"] - want) <= nper * 2.0 ** -52)).all()
    t_res, t_host = [], []
    for _ in range(args.reps):
        t_res.append(timed(ev.result, args.result_calls))
        t_host.append(timed(host_state.ap, 1))
    result["result"] = dict(images=updates * N, records=first["n_records"], calls_per_rep=args.result_calls,
                            baseline_calls_per_rep=1, baseline="tests/eval_ref.py's AP on the host over the same "
                            "records (numpy sort, cumsum)", op=summary(t_res), baseline_times=summary(t_host),
                            ratio_min_over_min=round(min(t_host) / min(t_res), 1), map=first["map"])
    print(f"result: op {result['result']['op']['min_us']} us min / {result['result']['op']['median_us']} median, "
          f"baseline {result['result']['baseline_times']['min_us']} us min, {first['n_records']} records", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
