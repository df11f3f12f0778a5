"""Time multi-scale RoIAlign over a feature pyramid (fp32, float16, bfloat16), forward and
backward, against the two ways of getting the same result from ops.roi_align.

    python tools/bench_multiscale_roi_align.py [--out profiles/multiscale_roi_align_bench.json]

Shape: cfg2's batch behind an FPN neck -- 8 images of 600 x 600, C = 256, maps of 150^2,
75^2, 38^2 and 19^2 (scales 1/4 .. 1/32 as ops.MultiScaleRoIAlign infers them), 8 x 300 RoIs
in shuffled image order, 7 x 7 bins, sampling_ratio 2, the default LevelMapper (224 px at
level 4).  sqrt(area) is drawn log-uniform in 40 .. 590 px with aspect ratios in 1/2 .. 2, so
every level is populated; the counts per level are recorded.

Variants per dtype and direction:
  single    ops._multiscale_fwd / _multiscale_bwd: one launch, levels decided in the kernel
  single_grouped  the same call on the same RoIs reordered so that each level's RoIs are
            contiguous (what a caller who can choose the order gets: the coarse maps then
            stay in cache while their RoIs are pooled)
  user_loop what a user writes with today's ops, as torchvision does: the LevelMapper in
            torch, then per level torch.where (a host sync), a gather of the RoIs,
            ops.roi_align and an indexed write into a zero-filled result; the backward is
            autograd's through that graph (torch.autograd.grad on a graph built once)
  presplit  L calls of ops._roi_align_fwd / _roi_align_bwd on RoIs and gradients split by
            level beforehand: no sync, no gather, no scatter -- the kernels alone
All are timed with device events in one process, interleaved: per repetition --calls calls
of each forward (--bwd-calls of each backward, which runs for milliseconds); 5 repetitions,
min and median reported.  Every call allocates its outputs, as the autograd functions do.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

from bench_roi_pool_half import summary, timed  # noqa: E402

IMG, BATCH, C, PER_IMAGE, SAMPLING_RATIO = 600, 8, 256, 300, 2
SIZES = [150, 75, 38, 19]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiscale_roi_align_bench.json"))
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--bwd-calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.calls < 200 or args.bwd_calls < 20 or args.reps < 5:
        ap.error("--calls >= 200, --bwd-calls >= 20 and --reps >= 5")

    import numpy as np
    import torch
    from replication_faster_rcnn_amd import _lib, ops
    dev = torch.device("cuda", 0)
    dts = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
    L = len(SIZES)
    shapes = [(BATCH, C, s, s) for s in SIZES]
    scales = ops.MultiScaleRoIAlign.infer_scales([torch.empty(1, 1, s, s) for s in SIZES], [(IMG, IMG)] * BATCH)
    k_min, k_max, thr = ops._pyramid_levels(scales, 224, 4)

    r = np.random.default_rng(2)
    R = BATCH * PER_IMAGE
    root = np.exp(r.uniform(np.log(40), np.log(590), R))
    aspect = np.exp(r.uniform(np.log(0.5), np.log(2), R))
    w, h = np.minimum(root * np.sqrt(aspect), IMG), np.minimum(root / np.sqrt(aspect), IMG)
    x1, y1 = r.uniform(0, IMG - w), r.uniform(0, IMG - h)
    b = r.permutation(np.repeat(np.arange(BATCH), PER_IMAGE))
    rois = torch.from_numpy(np.stack([b, x1, y1, x1 + w, y1 + h], 1).astype(np.float32)).to(dev)

    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    x32 = [torch.randn(s, device=dev, generator=gen) for s in shapes]
    g32 = torch.randn((R, C, 7, 7), device=dev, generator=gen)
    _, levels = ops._multiscale_fwd(x32, rois, 7, 7, scales, thr, SAMPLING_RATIO, False, True)
    idx = [torch.where(levels == l)[0] for l in range(L)]
    counts = [int(i.numel()) for i in idx]
    assert all(counts), counts
    split_rois = [rois[i].contiguous() for i in idx]
    order = torch.cat(idx)
    grouped_rois = rois[order].contiguous()

    def mapper(boxes):   # torchvision's LevelMapper, on the device
        s = torch.sqrt((boxes[:, 3] - boxes[:, 1]) * (boxes[:, 4] - boxes[:, 2]))
        lvl = torch.floor(4 + torch.log2(s / 224) + torch.tensor(1e-6, dtype=s.dtype, device=s.device))
        return torch.clamp(lvl, min=k_min, max=k_max).to(torch.int64) - k_min

    def user_loop(xs):
        lv = mapper(rois)
        out = torch.zeros((R, C, 7, 7), dtype=xs[0].dtype, device=dev)
        for l, x in enumerate(xs):
            i = torch.where(lv == l)[0]
            out[i] = ops.roi_align(x, rois[i], 7, scales[l], SAMPLING_RATIO, False)
        return out

    fv, bv, names = {}, {}, {}
    for k, t in dts.items():
        xs = [x.to(t) for x in x32]
        g = g32.to(t)
        split_g = [g[i].contiguous() for i in idx]
        leaves = [x.clone().requires_grad_(True) for x in xs]
        graph_out = user_loop(leaves)
        fv[f"single_{k}"] = (lambda xs=xs: ops._multiscale_fwd(xs, rois, 7, 7, scales, thr, SAMPLING_RATIO, False, False))
        bv[f"single_{k}"] = (lambda g=g: ops._multiscale_bwd(g, rois, shapes, scales, thr, SAMPLING_RATIO, False))
        gg = g[order].contiguous()
        fv[f"single_grouped_{k}"] = (lambda xs=xs: ops._multiscale_fwd(xs, grouped_rois, 7, 7, scales, thr,
                                                                       SAMPLING_RATIO, False, False))
        bv[f"single_grouped_{k}"] = (lambda gg=gg: ops._multiscale_bwd(gg, grouped_rois, shapes, scales, thr,
                                                                       SAMPLING_RATIO, False))

        def user_fwd(xs=xs):
            with torch.no_grad():
                return user_loop(xs)
        fv[f"user_loop_{k}"] = user_fwd
        bv[f"user_loop_{k}"] = (lambda o=graph_out, lv=leaves, g=g: torch.autograd.grad(o, lv, g, retain_graph=True))
        fv[f"presplit_{k}"] = (lambda xs=xs: [ops._roi_align_fwd(xs[l], split_rois[l], 7, 7, scales[l], SAMPLING_RATIO,
                                                                 False) for l in range(L)])
        bv[f"presplit_{k}"] = (lambda sg=split_g: [ops._roi_align_bwd(sg[l], split_rois[l], shapes[l], scales[l],
                                                                      SAMPLING_RATIO, False) for l in range(L)])
        names[f"single_{k}"] = names[f"single_grouped_{k}"] = tuple(
            _lib.roi_align_multi_kernel(which, L, R, BATCH, C, 7, 7, SAMPLING_RATIO, t) for which in ("fwd", "bwd"))
        # all of them give the same bits, on every call
        view = torch.int32 if t == torch.float32 else torch.int16
        one, ref = fv[f"single_{k}"]()[0], fv[f"user_loop_{k}"]()
        assert torch.equal(one.view(view), ref.view(view)) and torch.equal(one.view(view), fv[f"single_{k}"]()[0].view(view))
        parts = fv[f"presplit_{k}"]()
        assert torch.equal(fv[f"single_grouped_{k}"]()[0].view(view), one[order].view(view))
        assert all(torch.equal(one[idx[l]].view(view), parts[l].view(view)) for l in range(L))
        for a, p, u in zip(bv[f"single_{k}"](), bv[f"presplit_{k}"](), bv[f"user_loop_{k}"]()):
            assert torch.equal(a.view(view), p.view(view))
            assert torch.allclose(a.float(), u.float(), rtol=2e-2, atol=2e-2)   # autograd's scatter sums in another order

    times = {"fwd": {v: [] for v in fv}, "bwd": {v: [] for v in bv}}
    for op, vs, calls in (("fwd", fv, args.calls), ("bwd", bv, args.bwd_calls)):
        for _ in range(args.warmup):
            for f in vs.values():
                f()
        for _ in range(args.reps):
            for v, f in vs.items():
                times[op][v].append(timed(f, calls))
    result = dict(device=torch.cuda.get_device_name(0), calls_per_rep=dict(fwd=args.calls, bwd=args.bwd_calls),
                  reps=args.reps, warmup=args.warmup,
                  timed="device events around back-to-back calls, variants interleaved per repetition, one process",
                  shape=dict(N=BATCH, C=C, image=IMG, maps=SIZES, scales=list(scales), R=R, bins="7x7",
                             sampling_ratio=SAMPLING_RATIO, aligned=False, thresholds=list(thr),
                             rois_per_level=counts),
                  results={})
    for op, vs in times.items():
        rec = {v: summary(t) for v, t in vs.items()}
        for v in rec:
            k = v.rsplit("_", 1)[1]
            rec[v]["vs_presplit_min"] = round(rec[v]["min_us"] / rec[f"presplit_{k}"]["min_us"], 3)
            if v in names:
                rec[v]["kernel"] = names[v][op == "bwd"]
        result["results"][op] = rec
        print(op, {v: (r["min_us"], r["median_us"]) for v, r in rec.items()}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
