"""Time the COCO-style evaluation (COCOEvaluator.update per batch, result() per
dataset) against what a user could write without it: a per-batch .cpu() of the
detections and pycocotools' loop on the host (tests/coco_eval_ref.py), then its
accumulate on the host.  ops.eval_update (the VOC protocol) runs interleaved in
the same process, for context.

    python tools/bench_coco_eval.py [--out profiles/coco_eval_bench.json]

Workload: tools/bench_eval.py's -- the output of ops.detect on
synth.head_outputs at the cfg2 detection shape (N=8, R=300, C=21, 600x1000,
score_thresh 0.05), 8 gt slots per image, one of them flagged (difficult there,
crowd here).  Timed with device events, interleaved: per repetition --calls
COCOEvaluator.update, --calls ops.eval_update, then --baseline-calls host
updates; 5 repetitions, min and median reported.  result() is timed over 4,952
images' worth of records (619 updates of the batch) against the numpy
accumulate over the same records.  Before timing, the device state and outputs
must equal the numpy restatement of the contract.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from bench_eval import DATASET_IMAGES, G, SCORE_THRESH, SHAPE, summary, timed, workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coco_eval_bench.json"))
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--baseline-calls", type=int, default=1)
    ap.add_argument("--result-calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.calls < 200 or args.reps < 5:
        ap.error("--calls >= 200 and --reps >= 5")

    import numpy as np
    import torch
    import coco_eval_ref as ref
    from replication_faster_rcnn_amd import ops
    from replication_faster_rcnn_amd.evaluate import COCOEvaluator

    det, gt_host, gt_dev = workload()
    C, N = SHAPE["C"], SHAPE["N"]
    M = det[1].shape[1]
    per_batch = int(det[3].clamp(0, M).sum().item())
    updates = -(-DATASET_IMAGES // N)
    assert max(args.calls, updates) * per_batch <= ops.EVAL_MAX_CAPACITY

    def host_update(state):
        d = [t.cpu().numpy() for t in det]               # the per-batch copy to the host
        state.update(*d, *gt_host)

    # the op equals the contract: one update, the records and every output
    want_state = ref.State(C, per_batch)
    host_update(want_state)
    ev = COCOEvaluator(C, args.calls * per_batch)
    ev.update(det, *gt_dev)
    hdr, key, bits, _ = (t.cpu().numpy() for t in ev.state)
    assert np.array_equal(hdr, want_state.hdr) and np.array_equal(key[:per_batch].view(np.uint64), want_state.rec_key)
    assert np.array_equal(bits[:per_batch].view(np.uint64), want_state.rec_bits)
    want, got = want_state.accumulate(), ev.result()
    assert np.array_equal(got["precision"], want["precision"]) and np.array_equal(got["recall"], want["recall"])
    assert (np.abs(got["stats"] - want["stats"]) <= want["n_stats"] * 2.0 ** -52).all()

    voc = ops.eval_state(C, args.calls * per_batch)
    op = lambda: ev.update(det, *gt_dev)                                # noqa: E731
    op_voc = lambda: ops.eval_update(det, *gt_dev, state=voc)           # noqa: E731
    base_state = ref.State(C, (args.baseline_calls + 1) * per_batch)
    base = lambda: host_update(base_state)                              # noqa: E731
    for _ in range(args.warmup):
        op()
        op_voc()
    t_op, t_voc, t_base = [], [], []
    for _ in range(args.reps):
        ev.reset()
        voc[0].zero_()
        t_op.append(timed(op, args.calls))
        t_voc.append(timed(op_voc, args.calls))
        assert int(ev.state[0][0].item()) == args.calls * per_batch and int(ev.state[0][2].item()) == 0
        base_state.hdr[:] = 0
        t_base.append(timed(base, args.baseline_calls))
    m, ig, rank = ref.unpack_bits(want_state.rec_bits)
    result = dict(workload=dict(SHAPE, score_thresh=SCORE_THRESH, gt_slots=G, max_det=M, generator="synth.head_outputs "
                                "-> ops.detect; gt: synth.gt_boxes + detections (tools/bench_eval.py)"),
                  device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
                  records_per_update=per_batch,
                  records_ranked_per_update=int((rank < ref.KEEP).sum()),
                  matched_at_050_all_areas=int(m[:, 0, 0].sum()),
                  update=dict(calls_per_rep=args.calls, baseline_calls_per_rep=args.baseline_calls,
                              baseline=".cpu() of the detections + tests/coco_eval_ref.py's sequential loop on the host",
                              op=summary(t_op), voc_eval_update=summary(t_voc), baseline_times=summary(t_base),
                              ratio_min_over_min=round(min(t_base) / min(t_op), 1),
                              over_voc_eval_update=round(min(t_op) / min(t_voc), 2)))
    u = result["update"]
    print(f"update: op {u['op']['min_us']} us min / {u['op']['median_us']} median, ops.eval_update "
          f"{u['voc_eval_update']['min_us']} / {u['voc_eval_update']['median_us']}, baseline "
          f"{u['baseline_times']['min_us']} / {u['baseline_times']['median_us']} us, {per_batch} records per update",
          flush=True)

    # result() over a dataset's worth of records
    ev = COCOEvaluator(C, updates * per_batch)
    for _ in range(updates):
        ev.update(det, *gt_dev)
    first = ev.result()
    assert first["n_records"] == updates * per_batch and first["n_images"] == updates * N
    host_state = ref.State(C, 1)
    host_state.hdr, host_state.rec_key, host_state.rec_bits = (
        ev.state[0].cpu().numpy(), ev.state[1].cpu().numpy().view(np.uint64), ev.state[2].cpu().numpy().view(np.uint64))
    want = host_state.accumulate()
    assert np.array_equal(first["precision"], want["precision"]) and np.array_equal(first["recall"], want["recall"])
    assert (np.abs(first["stats"] - want["stats"]) <= want["n_stats"] * 2.0 ** -52).all()
    t_res, t_host = [], []
    for _ in range(args.reps):
        t_res.append(timed(ev.result, args.result_calls))
        t_host.append(timed(host_state.accumulate, 1))
    result["result"] = dict(images=updates * N, records=first["n_records"], calls_per_rep=args.result_calls,
                            baseline_calls_per_rep=1, baseline="tests/coco_eval_ref.py's accumulate and summarize on "
                            "the host over the same records (numpy sort, cumsum, searchsorted)",
                            op=summary(t_res), baseline_times=summary(t_host),
                            ratio_min_over_min=round(min(t_host) / min(t_res), 1),
                            stats={k: first[k] for k in ref.STATS})
    r = result["result"]
    print(f"result: op {r['op']['min_us']} us min / {r['op']['median_us']} median, baseline "
          f"{r['baseline_times']['min_us']} us min, {first['n_records']} records", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
