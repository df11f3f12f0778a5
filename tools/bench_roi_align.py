"""Time RoIAlign forward and backward (fp32, float16, bfloat16) with ops.roi_pool at the
same shapes as the yardstick.

    python tools/bench_roi_align.py [--out profiles/roi_align_bench.json]

Shapes (tools/bench_roi_pool_half.py's workloads): cfg2, 8 x 256 x 38 x 63 features with
8 x 300 proposals from ops.propose, and cfg5, 16 x 256 x 38 x 38 features with 16 x 128
RoIs sampled by targets.proposal_targets (numpy seed 0); the RoIs grouped by image, 7 x 7
bins, boxes from ops.roi_transform.  Variants per shape and direction: RoIAlign with
sampling_ratio 2 in the three dtypes, RoIAlign fp32 with adaptive sampling, and fp32
RoIPool.  All variants are timed with device events in one process, interleaved: per
repetition --calls calls of each; 5 repetitions, min and median reported.  The calls are
ops._roi_align_fwd / _roi_align_bwd and ops._roi_pool_fwd / _roi_pool_bwd on device
tensors (each allocates its output, as the autograd functions do).  The byte counts are the
algorithmic ones (every tensor once), the fraction is of the HBM peak bench.py uses; it is
not a statement about what bounds these kernels.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

from bench_roi_pool_half import HBM_PEAK_GBS, summary, timed, workloads  # noqa: E402

SAMPLING_RATIO = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_align_bench.json"))
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.calls < 200 or args.reps < 5:
        ap.error("--calls >= 200 and --reps >= 5")

    import torch
    from replication_faster_rcnn_amd import _lib, ops
    dts = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
    esize = {"fp32": 4, "fp16": 2, "bf16": 2}
    wl = workloads()
    shapes, variants, nbytes, names = {}, {}, {}, {}

    def one(shape, w):   # a scope of its own: the callables keep this shape's tensors
        c, x32, rois, inds = w["c"], w["x"], w["rois"], w["inds"]
        N, C, H, W = x32.shape
        R = rois.shape[0]
        shapes[shape] = dict(N=N, C=C, H=H, W=W, R=R, bins="7x7", img_h=c["img_h"], img_w=c["img_w"],
                             sampling_ratio=SAMPLING_RATIO, aligned=False)
        boxes = ops.roi_transform(rois, inds, c["img_h"], c["img_w"], H, W)
        xs = {k: x32.to(t) for k, t in dts.items()}
        gen = torch.Generator(device=x32.device)
        gen.manual_seed(1)
        g32 = torch.randn((R, C, 7, 7), device=x32.device, generator=gen)
        gs = {k: g32.to(t) for k, t in dts.items()}
        _, am = ops._roi_pool_fwd(x32, boxes, 7, 7, 1.0, True)
        fv, bv, fb, bb, fn, bn = {}, {}, {}, {}, {}, {}
        for k, t in dts.items():
            fv[f"align_{k}"] = (lambda k=k: ops._roi_align_fwd(xs[k], boxes, 7, 7, 1.0, SAMPLING_RATIO, False))
            bv[f"align_{k}"] = (lambda k=k: ops._roi_align_bwd(gs[k], boxes, (N, C, H, W), 1.0, SAMPLING_RATIO, False))
            fb[f"align_{k}"] = bb[f"align_{k}"] = N * C * H * W * esize[k] + R * 20 + R * C * 49 * esize[k]
            fn[f"align_{k}"] = _lib.roi_align_kernel("fwd", R, N, C, H, W, 7, 7, SAMPLING_RATIO, t)
            bn[f"align_{k}"] = _lib.roi_align_kernel("bwd", R, N, C, H, W, 7, 7, SAMPLING_RATIO, t)
        fv["align_fp32_adaptive"] = lambda: ops._roi_align_fwd(xs["fp32"], boxes, 7, 7, 1.0, -1, False)
        bv["align_fp32_adaptive"] = lambda: ops._roi_align_bwd(gs["fp32"], boxes, (N, C, H, W), 1.0, -1, False)
        fv["roi_pool_fp32"] = lambda: ops._roi_pool_fwd(xs["fp32"], boxes, 7, 7, 1.0, True)
        bv["roi_pool_fp32"] = lambda: ops._roi_pool_bwd(gs["fp32"], boxes, am, (N, C, H, W), 1.0)
        fb["roi_pool_fp32"] = bb["roi_pool_fp32"] = N * C * H * W * 4 + R * 20 + R * C * 49 * 8
        fn["roi_pool_fp32"] = _lib.roi_pool_fwd_kernel(R, N, C, H, W, head=False)
        bn["roi_pool_fp32"] = _lib.roi_pool_bwd_kernel(R, N, C, H, W)
        # the same inputs give the same bits on every call
        for f in (fv["align_fp32"], bv["align_fp32"]):
            assert torch.equal(f().view(torch.int32), f().view(torch.int32))
        variants[(shape, "fwd")], nbytes[(shape, "fwd")], names[(shape, "fwd")] = fv, fb, fn
        variants[(shape, "bwd")], nbytes[(shape, "bwd")], names[(shape, "bwd")] = bv, bb, bn

    for shape, w in (("cfg2", wl["cfg2_fwd"]), ("cfg5", wl["cfg5"])):
        one(shape, w)

    times = {key: {v: [] for v in vs} for key, vs in variants.items()}
    for key, vs in variants.items():
        for _ in range(args.warmup):
            for f in vs.values():
                f()
        for _ in range(args.reps):
            for v, f in vs.items():
                times[key][v].append(timed(f, args.calls))
    result = dict(device=torch.cuda.get_device_name(0), calls_per_rep=args.calls, reps=args.reps, warmup=args.warmup,
                  timed="device events around --calls back-to-back calls, variants interleaved per repetition, one "
                        "process; ops._roi_align_fwd / _bwd and ops._roi_pool_fwd / _bwd on device tensors",
                  bytes="algorithmic: features (or grad_in) once, boxes, out (or grad) once; RoIPool also its argmax",
                  hbm_peak_gbs=HBM_PEAK_GBS, shapes=shapes, results={})
    for (shape, op), vs in times.items():
        rec = {}
        for v, t in vs.items():
            rec[v] = summary(t, nbytes[(shape, op)].get(v))
            if v in names[(shape, op)]:
                rec[v]["kernel"] = names[(shape, op)][v]
        for v in rec:
            rec[v]["vs_roi_pool_fp32_min"] = round(rec[v]["min_us"] / rec["roi_pool_fp32"]["min_us"], 3)
        result["results"][f"{shape}_{op}"] = rec
        print(shape, op, {v: (r["min_us"], r["median_us"]) for v, r in rec.items()}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
