"""Time the pyramid box-head inference (ops.box_head_detections) against the path a user
composes without it: torch.softmax, a torch decode, torch.where, ops.nms per (image, class), a
sort and the cut.

    python tools/bench_box_detections.py [--out profiles/box_detections_bench.json]
                                         [--stats profiles/box_detections_kernel_stats.csv]

Shape: cfg2's batch behind an FPN -- 8 images of 600 x 600 with 1,000 real proposals each
(synth.head_outputs, its boxes turned to xyxy), at C = 21 and C = 91, score_thresh 0.05, nms 0.5,
100 detections per image.  Variants fp32 / float16 / bfloat16 and the composed path are timed with
device events in one process, interleaved: per repetition --calls calls of every variant, then
--baseline-calls of the composed path; 5 repetitions, min and median reported.  The per-kernel
breakdown comes from a rocprofv3 --kernel-trace --stats run of its own (a child process that only
calls the op, 100 calls per variant and C), taken before this process touches the GPU.  The op
must equal the numpy restatement (tests/box_detections_ref.py) bit for bit; the composed path
must select the same (row, class) pairs up to the decisions torch's own exp and division flip
(counted in the record, at most 2 % of the detections).
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SHAPE = dict(N=8, R=1000, img_h=600, img_w=600, seed=0)
CLASSES = (21, 91)
KW = dict(score_thresh=0.05, nms_thresh=0.5, detections_per_img=100)
WEIGHTS = (10.0, 10.0, 5.0, 5.0)
VARIANTS = ("fp32", "float16", "bfloat16")


def host_inputs(C):
    import numpy as np
    from replication_faster_rcnn_amd import synth
    rois, count, cls, reg = synth.head_outputs(C=C, **SHAPE)
    N, R = SHAPE["N"], SHAPE["R"]
    return (cls.reshape(N * R, C), reg.reshape(N * R, 4 * C), np.ascontiguousarray(rois[:, :, [1, 0, 3, 2]]), count,
            np.array([(SHAPE["img_h"], SHAPE["img_w"])] * N, np.float32))


def device_inputs(host, dtype):
    import torch
    lg, rg, p, pc, sz = (torch.from_numpy(a).cuda() for a in host)
    return lg.to(dtype), rg.to(dtype), p, pc, sz


def composed(lg, rg, p, pc, sz):
    """What a user writes on top of ops.nms: two host syncs per (image, class) and one per
    image.  Returns per image (rows, labels) of its detections, best first."""
    import math
    import torch
    from replication_faster_rcnn_amd import ops
    N, R = p.shape[:2]
    C = lg.shape[1]
    prob = torch.softmax(lg.float(), -1).view(N, R, C)
    d = rg.float().view(N, R, C, 4)
    a = p[:, :, None, :]
    w, h = a[..., 2] - a[..., 0], a[..., 3] - a[..., 1]
    cx, cy = a[..., 0] + 0.5 * w, a[..., 1] + 0.5 * h
    clip = math.log(1000.0 / 16)
    pcx, pcy = d[..., 0] / WEIGHTS[0] * w + cx, d[..., 1] / WEIGHTS[1] * h + cy
    pw = torch.exp((d[..., 2] / WEIGHTS[2]).clamp(max=clip)) * w
    ph = torch.exp((d[..., 3] / WEIGHTS[3]).clamp(max=clip)) * h
    boxes = torch.stack([(pcx - 0.5 * pw).clamp(0, SHAPE["img_w"]), (pcy - 0.5 * ph).clamp(0, SHAPE["img_h"]),
                         (pcx + 0.5 * pw).clamp(0, SHAPE["img_w"]), (pcy + 0.5 * ph).clamp(0, SHAPE["img_h"])], -1)
    small = ((boxes[..., 2] - boxes[..., 0]) >= 1e-2) & ((boxes[..., 3] - boxes[..., 1]) >= 1e-2)
    counts = pc.tolist()
    out = []
    for n in range(N):
        rows_n, labels_n, scores_n = [], [], []
        for c in range(1, C):
            s = prob[n, :counts[n], c]
            rows = torch.where((s > KW["score_thresh"]) & small[n, :counts[n], c])[0]
            if rows.numel():
                keep = rows[ops.nms(boxes[n, rows, c], s[rows], KW["nms_thresh"])]
                rows_n.append(keep)
                labels_n.append(torch.full_like(keep, c))
                scores_n.append(s[keep])
        if rows_n:
            rows_n, labels_n, scores_n = torch.cat(rows_n), torch.cat(labels_n), torch.cat(scores_n)
            order = scores_n.sort(descending=True)[1][:KW["detections_per_img"]]
            out.append((rows_n[order].tolist(), labels_n[order].tolist()))
        else:
            out.append(([], []))
    return out


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


def child(calls):
    """The traced run: the op alone, every variant and C."""
    import torch
    from replication_faster_rcnn_amd import ops
    for C in CLASSES:
        host = host_inputs(C)
        for name in VARIANTS:
            dev = device_inputs(host, getattr(torch, "float32" if name == "fp32" else name))
            for _ in range(calls):
                ops.box_head_detections(*dev, **KW)
    torch.cuda.synchronize()


def kernel_name(full):
    """"void frcnn::(anonymous namespace)::bd_x_kernel<frcnn::ElemF32>(args)" -> "bd_x_kernel<ElemF32>"."""
    return full.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("frcnn::", "")


def kernel_stats(stats_path, trace_dir, calls):
    os.makedirs(trace_dir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "-o", "run", "--",
           sys.executable, os.path.abspath(__file__), "--child", str(calls)]
    subprocess.run(cmd, check=True, timeout=300, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise RuntimeError(f"rocprofv3 wrote no kernel_stats.csv under {trace_dir}")
    shutil.copyfile(files[0], stats_path)
    rows = [r for r in csv.DictReader(open(files[0])) if "bd_" in r["Name"]]
    return [dict(name=kernel_name(r["Name"]), calls=int(r["Calls"]),
                 avg_us=round(float(r["AverageNs"]) / 1e3, 2), min_us=round(float(r["MinNs"]) / 1e3, 2))
            for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_detections_bench.json"))
    ap.add_argument("--stats", default=None, help="also take the rocprofv3 per-kernel statistics, into this csv")
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "build_trace", "box_detections"))
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--baseline-calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    if args.calls < 200 or args.reps < 5:
        ap.error("--calls >= 200 and --reps >= 5")

    kernels = kernel_stats(args.stats, args.trace_dir, 100) if args.stats else []   # before this process opens the GPU

    import numpy as np
    import torch
    import box_detections_ref as ref_mod
    from replication_faster_rcnn_amd import ops
    result = dict(workload=dict(SHAPE, classes=list(CLASSES), reg_weights=list(WEIGHTS), generator="synth.head_outputs",
                                **KW),
                  device=torch.cuda.get_device_name(0), calls_per_rep=args.calls,
                  baseline_calls_per_rep=args.baseline_calls, reps=args.reps, warmup=args.warmup,
                  baseline="torch.softmax + torch decode + torch.where + ops.nms per (image, class) + sort",
                  kernels_100_calls_per_variant=kernels, classes={})
    for C in CLASSES:
        host = host_inputs(C)
        devs = {v: device_inputs(host, getattr(torch, "float32" if v == "fp32" else v)) for v in VARIANTS}
        fns = {v: (lambda d=devs[v]: ops.box_head_detections(*d, **KW)) for v in VARIANTS}
        base = lambda: composed(*devs["fp32"])                                # noqa: E731
        plan = ops.box_head_detections_kernel(SHAPE["R"], C, KW["detections_per_img"])
        # every variant equal to the contract on its own widened inputs; the composed path selects the same pairs
        for v in VARIANTS:
            got = [t.cpu().numpy() for t in fns[v]()]
            want = ref_mod.box_detections(devs[v][0].float().cpu().numpy(), devs[v][1].float().cpu().numpy(), *host[2:],
                                          reg_weights=WEIGHTS, **KW)
            for g, w in zip(got, want):
                assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), f"{v}: the op differs from the restatement"
            if v == "fp32":
                ref32 = want
        pairs = base()
        differ = 0      # torch's own softmax, exp and division may flip a decision that sits on an edge
        for n in range(SHAPE["N"]):
            k = int(ref32[4][n])
            differ += len(set(zip(*pairs[n])) ^ set(zip(ref32[3][n, :k].tolist(), ref32[1][n, :k].tolist())))
        assert differ <= 0.02 * int(ref32[4].sum()), f"the composed path selects other detections ({differ} pairs)"
        for f in fns.values():
            for _ in range(args.warmup):
                f()
        base()
        t = {v: [] for v in VARIANTS}
        t_base = []
        for _ in range(args.reps):
            for v in VARIANTS:
                t[v].append(timed(fns[v], args.calls))
            t_base.append(timed(base, args.baseline_calls))
        entry = dict(plan=plan, baseline=summary(t_base), composed_pairs_that_differ=differ,
                     kept_per_image=ref32[5].tolist(),
                     detections_per_image=ref32[4].tolist(),
                     workspace_bytes=int(ops._bd_ws[(SHAPE["N"], SHAPE["R"], C)]))
        for v in VARIANTS:
            entry[v] = dict(summary(t[v]), speedup_min_over_min=round(min(t_base) / min(t[v]), 1),
                            faster_outside_spread=max(t[v]) < min(t_base))
        result["classes"][str(C)] = entry
        print(f"C={C}: " + ", ".join(f"{v} {entry[v]['min_us']} us min / {entry[v]['median_us']} median"
                                     for v in VARIANTS) +
              f"; composed {entry['baseline']['min_us']} / {entry['baseline']['median_us']} us; kept "
              f"{entry['kept_per_image']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
