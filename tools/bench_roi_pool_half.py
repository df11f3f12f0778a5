"""Time RoIPool on float16 / bfloat16 feature maps against the fp32 kernels and against
what a mixed-precision caller ran before the 16-bit kernels existed (widen, fp32 op,
narrow).

    python tools/bench_roi_pool_half.py [--out profiles/roi_pool_half_bench.json]

Shapes: cfg2's forward (8 x 256 x 38 x 63 features, 8 x 300 proposals from ops.propose)
and cfg5's forward and backward (16 x 256 x 38 x 38 features, 16 x 128 RoIs sampled by
targets.proposal_targets, numpy seed 0), the RoIs grouped by image, 7 x 7 bins,
bench.py's synthetic inputs.  Variants per shape: the fp32, float16 and bfloat16 op
alone, and for the two 16-bit types the cast-wrapped fp32 op (``x.float()`` -> op ->
``.to(T)``; backward: ``grad.float()`` -> op -> ``.to(T)``).  All variants are timed with
device events in one process, interleaved: per repetition --calls calls of each; 5
repetitions, min and median reported.  The forward is ops.roi_pool_head into caller
buffers, the backward ops._roi_pool_bwd, as bench.py calls them.  The byte counts are
the algorithmic ones (every tensor once), and the fraction is of the HBM peak bench.py
uses.  The 16-bit results must equal the fp32 op's on the widened input, narrowed.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

SEED = 0
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak, as bench.py's roofline uses it
S_CFG5 = 128
G_CFG5 = 32


def proposals(cfg):
    """(config, features fp32 [N,C,H,W], rois [N,post,4], count [N]) of a bench.py config."""
    import numpy as np
    import torch
    from replication_faster_rcnn_amd import anchors as A, ops, synth
    dev = torch.device("cuda", 0)
    c = synth.CONFIGS[cfg]
    images = range(c["batch"])
    nA = c["feat_h"] * c["feat_w"] * 3 * len(c["scales"])
    sc = torch.from_numpy(np.stack([synth.rpn_scores(nA, SEED, i) for i in images])).to(dev)
    de = torch.from_numpy(np.stack([synth.rpn_deltas(nA, SEED, i) for i in images])).to(dev)
    x = torch.from_numpy(np.stack([synth.features(c["C"], c["feat_h"], c["feat_w"], SEED, i) for i in images])).to(dev)
    base = A.generate_anchor_base_device()
    rois, _, cnt = ops.propose(sc, de, img_w=c["img_w"], img_h=c["img_h"], pre_nms=c["pre_nms"],
                               post_nms=c["post_nms"], anchor_base=base, feat_h=c["feat_h"], feat_w=c["feat_w"])
    assert cnt.tolist() == [c["post_nms"]] * x.shape[0], "the synthetic scores fill every image's proposals"
    return c, x, rois, cnt


def workloads():
    import numpy as np
    import torch
    from replication_faster_rcnn_amd import synth, targets
    dev = torch.device("cuda", 0)
    out = {}
    c, x, rois, _ = proposals("cfg2")
    N, R = x.shape[0], rois.shape[0] * rois.shape[1]
    out["cfg2_fwd"] = dict(c=c, x=x, rois=rois.view(-1, 4).contiguous(),
                           inds=torch.arange(N, device=dev, dtype=torch.float32).repeat_interleave(R // N))
    c, x, rois, cnt = proposals("cfg5")
    N = x.shape[0]
    gl = [synth.gt_boxes(c["img_h"], c["img_w"], G_CFG5, SEED, i) for i in range(N)]
    boxes = torch.from_numpy(np.stack([b for b, _ in gl])).to(dev)
    labels = torch.from_numpy(np.stack([l for _, l in gl])).to(dev)
    saved = np.random.get_state()
    np.random.seed(SEED)
    s_roi, _, _, s_cnt = targets.proposal_targets(rois, cnt, boxes, labels, n_sample=S_CFG5)
    np.random.set_state(saved)
    assert s_cnt.tolist() == [S_CFG5] * N
    out["cfg5"] = dict(c=c, x=x, rois=s_roi.float().view(-1, 4).contiguous(),
                       inds=torch.arange(N, device=dev, dtype=torch.float32).repeat_interleave(S_CFG5))
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


def summary(v, nbytes=None):
    d = dict(reps_us=[round(x, 2) for x in v], min_us=round(min(v), 2), median_us=round(statistics.median(v), 2))
    if nbytes is not None:
        d["alg_bytes"] = int(nbytes)
        d["hbm_frac_at_min"] = round(nbytes / (min(v) * 1e-6) / 1e9 / HBM_PEAK_GBS, 3)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_pool_half_bench.json"))
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.calls < 200 or args.reps < 5:
        ap.error("--calls >= 200 and --reps >= 5")

    import torch
    from replication_faster_rcnn_amd import _lib, ops
    f32 = torch.float32
    halves = {"fp16": torch.float16, "bf16": torch.bfloat16}
    esize = {"fp32": 4, "fp16": 2, "bf16": 2}
    wl = workloads()
    variants = {}   # (shape, op) -> {variant name: callable}
    nbytes = {}     # (shape, op) -> {variant name: algorithmic bytes (kernel-alone variants)}
    names = {}
    shapes = {}
    for shape, w in wl.items():
        c, x32, rois, inds = w["c"], w["x"], w["rois"], w["inds"]
        N, C, H, W = x32.shape
        R = rois.shape[0]
        shapes[shape] = dict(N=N, C=C, H=H, W=W, R=R, bins="7x7", img_h=c["img_h"], img_w=c["img_w"])
        xs = {"fp32": x32, **{k: x32.to(t) for k, t in halves.items()}}
        dts = {"fp32": f32, **halves}

        def bufs(dt):
            return (torch.empty((R, C, 7, 7), dtype=dt, device=x32.device),
                    torch.empty((R, C, 7, 7), dtype=torch.int32, device=x32.device),
                    torch.empty((R, 5), dtype=f32, device=x32.device))

        ob = {k: bufs(dt) for k, dt in dts.items()}

        def fwd(k, xin=None, c=c, rois=rois, inds=inds, ob=ob, xs=xs):
            return ops.roi_pool_head(xs[k] if xin is None else xin, rois, inds, 7, c["img_h"], c["img_w"],
                                     rois_sorted=True, out=ob[k])

        fv, fb, fn = {}, {}, {}
        for k in dts:
            fv[k] = (lambda k=k, fwd=fwd: fwd(k))
            fb[k] = N * C * H * W * esize[k] + R * 20 + R * 20 + R * C * 49 * (esize[k] + 4)
            fn[k] = _lib.roi_pool_fwd_kernel(R, N, C, H, W, dtype=dts[k])
        for k, t in halves.items():
            fv[f"{k}_via_fp32_casts"] = (lambda k=k, t=t, fwd=fwd, xs=xs: fwd("fp32", xs[k].float())[0].to(t))
        variants[(shape, "fwd")], nbytes[(shape, "fwd")], names[(shape, "fwd")] = fv, fb, fn
        # the 16-bit forward is the fp32 forward on the widened input, narrowed
        for k, t in halves.items():
            o, a, b = fwd(k)
            o32, a32, b32 = fwd("fp32", xs[k].float())
            assert torch.equal(a, a32) and torch.equal(b, b32) and torch.equal(o.view(torch.int16),
                                                                             o32.to(t).view(torch.int16)), k
        if shape != "cfg5":
            continue
        gen = torch.Generator(device=x32.device)
        gen.manual_seed(1)
        g32 = torch.randn((R, C, 7, 7), device=x32.device, generator=gen)
        gs = {"fp32": g32, **{k: g32.to(t) for k, t in halves.items()}}
        _, am, bx = fwd("fp32")
        am, bx = am.clone(), bx.clone()
        bv, bb, bn = {}, {}, {}
        for k in dts:
            bv[k] = (lambda k=k: ops._roi_pool_bwd(gs[k], bx, am, (N, C, H, W), 1.0))
            bb[k] = R * C * 49 * (esize[k] + 4) + R * 20 + N * C * H * W * esize[k]
            bn[k] = _lib.roi_pool_bwd_kernel(R, N, C, H, W, dtype=dts[k])
        for k, t in halves.items():
            bv[f"{k}_via_fp32_casts"] = (lambda k=k, t=t: ops._roi_pool_bwd(gs[k].float(), bx, am, (N, C, H, W),
                                                                             1.0).to(t))
            assert torch.equal(bv[k]().view(torch.int16), bv[f"{k}_via_fp32_casts"]().view(torch.int16)), k
        variants[(shape, "bwd")], nbytes[(shape, "bwd")], names[(shape, "bwd")] = bv, bb, bn

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
                        "process; forward = ops.roi_pool_head(out=...), backward = ops._roi_pool_bwd",
                  bytes="algorithmic: features (or grad_in) once, rois + roi_inds + boxes, out (or grad) and argmax once",
                  hbm_peak_gbs=HBM_PEAK_GBS, shapes=shapes, results={})
    for (shape, op), vs in times.items():
        rec = {}
        for v, t in vs.items():
            rec[v] = summary(t, nbytes[(shape, op)].get(v))
            if v in names[(shape, op)]:
                rec[v]["kernel"] = names[(shape, op)][v]
        for k in halves:
            rec[k]["vs_fp32_min"] = round(rec[k]["min_us"] / rec["fp32"]["min_us"], 3)
            rec[k]["vs_fp32_median"] = round(rec[k]["median_us"] / rec["fp32"]["median_us"], 3)
            rec[k]["vs_casts_min"] = round(rec[k]["min_us"] / rec[f"{k}_via_fp32_casts"]["min_us"], 3)
        result["results"][f"{shape}_{op}" if not shape.endswith(op) else shape] = rec
        print(shape, op, {v: (r["min_us"], r["median_us"]) for v, r in rec.items()}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
