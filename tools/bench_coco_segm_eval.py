"""Time the COCO segm evaluation (ops.mask_overlap, ops.coco_segm_eval_update,
COCOMaskEvaluator.update) against the two paths a user composes without it.

    python tools/bench_coco_segm_eval.py [--out profiles/coco_segm_eval_bench.json]
                                         [--stats profiles/mask_overlap_kernel_stats.csv]
                                         [--bbox-rows PARENT.json TREE.json]

Shape: cfg2's batch behind an FPN -- 8 images, D = 100 detection slots, G = 32 gt masks (ellipses
in gt-like boxes), canvas 600 x 600, C = 21; the detection masks are ops.mask_head_paste's of
synthetic logits on boxes that are the gt's, jittered, so that pairs of one class overlap.
Rows, timed with device events in one process, interleaved, 5 repetitions, min and median:
  1 mask_overlap            ops.mask_overlap, the labelled form
  2 coco_segm_eval_update   the matching on its counts
  3 evaluator_update        COCOMaskEvaluator.update (both, cached outputs and workspace)
  4 composed_device         per image ((det[:, None] != 0) & (gt[None] != 0)).sum((2, 3)) on the
                            device, then the host matching of tests/coco_segm_ref.py
  5 host_numpy              a .cpu() of the masks, then numpy for the counts and the matching
Rows 4 and 5 run fewer calls.  The per-kernel times come from a rocprofv3 --kernel-trace --stats
run of its own (a child process that only calls the ops), taken before this process touches the
GPU; the pack kernel's read rate is its bytes (every live mask once) over its average time.
--bbox-rows copies the bbox update rows of two tools/bench_coco_eval.py records (the parent's
library and this tree's, run in the same visit) into the record.  Before timing, the counts, the
records and the result must equal the numpy restatement."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from bench_eval import summary, timed  # noqa: E402

SHAPE = dict(N=8, D=100, G=32, H=600, W=600, C=21, M=28, seed=0)
HBM_TBS, COPY_TBS = 8.0, 6.29     # the peak, and the copy rate recorded for preprocessing (profiles/preprocess_bench.json)


def inputs():
    """Device tensors: BoxDetections, pasted masks, gt masks / labels / crowd."""
    import numpy as np
    import torch
    from bench_mask_head import gt_like_boxes
    from replication_faster_rcnn_amd import ops
    s = SHAPE
    N, D, G, H, W, C, M = (s[k] for k in "N D G H W C M".split())
    r = np.random.default_rng(s["seed"])
    gt = np.stack([gt_like_boxes(r, G, H, W) for _ in range(N)])           # x1, y1, x2, y2
    gt_labels = r.integers(1, C, (N, G)).astype(np.int32)
    gt_crowd = (r.uniform(size=(N, G)) < 0.1).astype(np.uint8)
    gt_masks = torch.zeros(N, G, H, W, dtype=torch.uint8)
    yy, xx = torch.arange(H)[:, None], torch.arange(W)[None, :]
    for n in range(N):
        for g in range(G):       # an ellipse inside its box, 255 for set as a loader hands it over
            x1, y1, x2, y2 = gt[n, g]
            gt_masks[n, g] = ((((xx - (x1 + x2) / 2) / ((x2 - x1) / 2)) ** 2
                               + ((yy - (y1 + y2) / 2) / ((y2 - y1) / 2)) ** 2) <= 1) * 255
    src = r.integers(0, G, (N, D))
    boxes = np.take_along_axis(gt, src[:, :, None], 1) + r.uniform(-12, 12, (N, D, 4)).astype(np.float32)
    labels = np.take_along_axis(gt_labels, src, 1)
    wrong = r.uniform(size=(N, D)) < 0.15
    labels = np.where(wrong, r.integers(1, C, (N, D)), labels).astype(np.int32)
    scores = r.uniform(0.05, 1, (N, D)).astype(np.float32)
    count = np.array([D - 3 * n for n in range(N)], np.int32)
    g = torch.Generator().manual_seed(s["seed"])
    logits = (2.0 * torch.randn(N * D, C, M, M, generator=g) + 1.0).cuda()
    det = ops.BoxDetections(torch.from_numpy(boxes.astype(np.float32)).cuda(), torch.from_numpy(labels).cuda(),
                            torch.from_numpy(scores).cuda(), None, torch.from_numpy(count).cuda(), None)
    masks = ops.mask_head_paste(logits, det.boxes, det.labels, det.count, (H, W))
    return det, masks, gt_masks.cuda(), torch.from_numpy(gt_labels).cuda(), torch.from_numpy(gt_crowd).cuda()


def composed_device(det, masks, gt_masks):
    """What a user writes on the device today: the dense pairwise product, D*G*H*W booleans per image."""
    import torch
    out = []
    for n in range(masks.shape[0]):
        out.append(((masks[n][:, None] != 0) & (gt_masks[n][None] != 0)).sum((2, 3), dtype=torch.int32))
    return torch.stack(out), (masks != 0).sum((2, 3), dtype=torch.int32), (gt_masks != 0).sum((2, 3), dtype=torch.int32)


def child(calls):
    """The traced run: the ops alone."""
    import torch
    from replication_faster_rcnn_amd import ops
    det, masks, gt_masks, gt_labels, gt_crowd = inputs()
    state = ops.coco_eval_state(SHAPE["C"], calls * SHAPE["N"] * SHAPE["D"])
    for _ in range(calls):
        ov = ops.mask_overlap(masks, gt_masks, det_labels=det.labels, det_count=det.count, gt_labels=gt_labels,
                              n_class=SHAPE["C"])
        ops.coco_segm_eval_update(det, ov, gt_labels, gt_crowd, state=state)
    torch.cuda.synchronize()


def kernel_name(full):
    return full.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("frcnn::", "")


def kernel_stats(stats_path, trace_dir, calls):
    os.makedirs(trace_dir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "-o", "run", "--",
           sys.executable, os.path.abspath(__file__), "--child", str(calls)]
    subprocess.run(cmd, check=True, timeout=400, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise RuntimeError(f"rocprofv3 wrote no kernel_stats.csv under {trace_dir}")
    shutil.copyfile(files[0], stats_path)
    rows = [r for r in csv.DictReader(open(files[0])) if "mo_" in r["Name"] or "coco_" in r["Name"]]
    return [dict(name=kernel_name(r["Name"]), calls=int(r["Calls"]),
                 avg_us=round(float(r["AverageNs"]) / 1e3, 2), min_us=round(float(r["MinNs"]) / 1e3, 2),
                 max_us=round(float(r["MaxNs"]) / 1e3, 2)) for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coco_segm_eval_bench.json"))
    ap.add_argument("--stats", default=None, help="also take the rocprofv3 per-kernel statistics, into this csv")
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "build_trace", "coco_segm_eval"))
    ap.add_argument("--bbox-rows", nargs=2, metavar=("PARENT", "TREE"), default=None)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--baseline-calls", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    if args.calls < 200 or args.reps < 5:
        ap.error("--calls >= 200 and --reps >= 5")

    kernels = kernel_stats(args.stats, args.trace_dir, 50) if args.stats else []   # before this process opens the GPU

    import numpy as np
    import torch
    import coco_segm_ref as ref
    from replication_faster_rcnn_amd import _lib, ops
    from replication_faster_rcnn_amd.evaluate import COCOMaskEvaluator

    s = SHAPE
    N, D, G, H, W, C = (s[k] for k in "N D G H W C".split())
    det, masks, gt_masks, gt_labels, gt_crowd = inputs()
    per_batch = int(det.count.clamp(0, D).sum().item())
    host = lambda t: t.cpu().numpy()                                            # noqa: E731

    def overlap():
        return ops.mask_overlap(masks, gt_masks, det_labels=det.labels, det_count=det.count, gt_labels=gt_labels,
                                n_class=C)

    def host_update(state, counts):
        state.update(host(det.labels), host(det.scores), host(det.count), *counts, host(gt_labels), host(gt_crowd))

    # the ops equal the contract: the counts, the records of one update, the result
    want_ov = ref.overlap(host(masks), host(gt_masks), host(det.labels), host(det.count), host(gt_labels), C)
    ov = overlap()
    assert all(np.array_equal(host(a), b) for a, b in zip(ov, want_ov))
    comp = composed_device(det, masks, gt_masks)
    live = ref.considered(D, G)[None] & (np.arange(D)[None, :, None] < host(det.count)[:, None, None])
    same_class = host(det.labels)[:, :, None] == host(gt_labels)[:, None, :]
    assert np.array_equal(np.where(live & same_class, host(comp[0]), 0), want_ov[0])
    want_state = ref.State(C, per_batch)
    host_update(want_state, want_ov)
    ev = COCOMaskEvaluator(C, args.calls * per_batch)
    ev.update(det, masks, gt_masks, gt_labels, gt_crowd)
    hdr, key, bits, _ = (host(t) for t in ev.state)
    assert np.array_equal(hdr, want_state.hdr) and np.array_equal(key[:per_batch].view(np.uint64), want_state.rec_key)
    assert np.array_equal(bits[:per_batch].view(np.uint64), want_state.rec_bits)
    want, got = want_state.accumulate(), ev.result()
    assert np.array_equal(got["precision"], want["precision"]) and np.array_equal(got["recall"], want["recall"])

    state = ops.coco_eval_state(C, args.calls * per_batch)
    rows = dict(
        mask_overlap=(overlap, args.calls),
        coco_segm_eval_update=(lambda: ops.coco_segm_eval_update(det, ov, gt_labels, gt_crowd, state=state),
                               args.calls),
        evaluator_update=(lambda: ev.update(det, masks, gt_masks, gt_labels, gt_crowd), args.calls),
        composed_device=(lambda: host_update(ref.State(C, per_batch),
                                             [host(t) for t in composed_device(det, masks, gt_masks)]),
                         args.baseline_calls),
        host_numpy=(lambda: host_update(ref.State(C, per_batch),
                                        ref.overlap(host(masks), host(gt_masks), host(det.labels), host(det.count),
                                                    host(gt_labels), C)), args.host_calls))
    for name in ("mask_overlap", "coco_segm_eval_update", "evaluator_update"):
        for _ in range(args.warmup):
            rows[name][0]()
    rows["composed_device"][0]()
    times = {k: [] for k in rows}
    for _ in range(args.reps):
        ev.reset()
        state[0].zero_()
        for name, (fn, calls) in rows.items():
            times[name].append(timed(fn, calls))
        assert int(ev.state[0][0].item()) == args.calls * per_batch and int(state[0][2].item()) == 0
    res = {k: dict(summary(v), calls_per_rep=rows[k][1]) for k, v in times.items()}
    base = res["composed_device"]
    spread = max(base["reps_us"]) - min(base["reps_us"])
    for k in ("mask_overlap", "coco_segm_eval_update", "evaluator_update"):
        res[k]["composed_min_over_min"] = round(base["min_us"] / res[k]["min_us"], 1)
        res[k]["wins_by_more_than_spread"] = bool(max(res[k]["reps_us"]) < base["min_us"] - spread)
    live_masks = per_batch + N * G
    pack_bytes = live_masks * H * W
    result = dict(workload=dict(SHAPE, records_per_update=per_batch, live_masks=live_masks,
                                pairs_considered=int((live & same_class).sum()),
                                pairs_with_common_pixels=int((want_ov[0] > 0).sum()),
                                masks_set_fraction=round(float((masks != 0).float().mean().item()), 4),
                                generator="gt: ellipses in tools/bench_mask_head.py's gt-like boxes; detections: "
                                "ops.mask_head_paste of synthetic logits on jittered gt boxes"),
                  device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
                  plan=dict(_lib.mask_overlap_plan(N, D, G, H, W), kernels=ops.mask_overlap_kernel(H, W),
                            match=ops.coco_eval_kernel(segm=True)),
                  rows=res, pack_read_bytes=pack_bytes, dense_pairwise_bytes=N * D * G * H * W,
                  stats={k: got[k] for k in ref.cref.STATS})
    if kernels:
        result["kernels"] = kernels
        pack = [k for k in kernels if k["name"].startswith("mo_pack_kernel")]
        if pack:
            tbs = pack_bytes / (pack[0]["avg_us"] * 1e-6) / 1e12
            result["pack_read"] = dict(avg_us=pack[0]["avg_us"], tb_per_s=round(tbs, 3),
                                       of_hbm_peak=round(tbs / HBM_TBS, 3), of_copy_rate=round(tbs / COPY_TBS, 3))
    if args.bbox_rows:
        result["bbox_update"] = {}
        for name, path in zip(("parent", "tree"), args.bbox_rows):
            with open(path) as f:
                result["bbox_update"][name] = json.load(f)["update"]["op"]
        p, t = result["bbox_update"]["parent"], result["bbox_update"]["tree"]
        result["bbox_update"]["tree_min_over_parent_min"] = round(t["min_us"] / p["min_us"], 3)
        result["bbox_update"]["parent_spread_us"] = round(max(p["reps_us"]) - min(p["reps_us"]), 2)
    for k, v in res.items():
        print(f"{k}: {v['min_us']} us min / {v['median_us']} median over {v['calls_per_rep']} calls", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
