"""Time the pyramid mask head (ops.mask_head_targets / mask_head_losses / mask_head_paste) against
the paths a user composes without it.

    python tools/bench_mask_head.py [--out profiles/mask_head_bench.json]
                                    [--stats profiles/mask_head_kernel_stats.csv]

Shape: cfg2's batch behind an FPN -- 8 images, B = 512 slots with P = 128 positives each (all
real, interleaved with the negatives), G = 32 gt masks of 600 x 600, boxes of gt-like sizes,
M = 28, C = 21 and 91, D = 100 detections on a 600 x 600 canvas; logits in fp32 / float16 /
bfloat16.  Composed paths, in the same process: torch.where + ``gt_masks[n, matched].float()`` +
ops.roi_align for the targets; the indexed F.binary_cross_entropy_with_logits with autograd for
the loss (forward + backward, as the op is timed); for the paste the per-detection F.interpolate
loop of torchvision's paste_masks_in_image and one F.grid_sample per image.  Variants are timed
with device events, interleaved: per repetition --calls calls of every variant, then the composed
paths (fewer calls); 5 repetitions, min and median reported.  The per-kernel times come from a
rocprofv3 --kernel-trace --stats run of its own (a child process that only calls the ops), taken
before this process touches the GPU.  The ops must agree with their composed paths (targets
bit for bit with ops.roi_align, the loss to 1e-5, the masks on 99.9 % of the pixels).
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

SHAPE = dict(N=8, B=512, P=128, G=32, H=600, W=600, M=28, D=100, seed=0)
CLASSES = (21, 91)
VARIANTS = ("fp32", "float16", "bfloat16")
SPEC_TBS, COPY_TBS = 8.0, 6.29      # the data sheet's HBM rate; the copy rate of profiles/preprocess_bench.json


def tdtype(v):
    import torch
    return getattr(torch, "float32" if v == "fp32" else v)


def gt_like_boxes(r, n, H, W):
    import numpy as np
    w, h = r.uniform(40, 300, n), r.uniform(40, 300, n)
    x1, y1 = r.uniform(0, W - w), r.uniform(0, H - h)
    return np.stack([x1, y1, x1 + w, y1 + h], 1).astype(np.float32)


def inputs(C):
    """Device tensors of one class count: box targets, gt masks, both sets of logits, detections."""
    import numpy as np
    import torch
    from replication_faster_rcnn_amd import ops
    s = SHAPE
    N, B, P, G, H, W, M, D = (s[k] for k in "N B P G H W M D".split())
    r = np.random.default_rng(s["seed"])
    labels = np.zeros((N, B), np.int32)
    matched = np.zeros((N, B), np.int32)
    rois = np.zeros((N, B, 5), np.float32)
    gt = np.stack([gt_like_boxes(r, G, H, W) for _ in range(N)])
    masks = torch.zeros(N, G, H, W, dtype=torch.uint8)
    yy, xx = torch.arange(H)[:, None], torch.arange(W)[None, :]
    for n in range(N):
        pos = np.sort(r.choice(B, P, replace=False))
        labels[n, pos] = r.integers(1, C, P)
        matched[n] = r.integers(0, G, B)
        jitter = r.uniform(-8, 8, (B, 4)).astype(np.float32)
        rois[n, :, 0] = n
        rois[n, :, 1:] = gt[n, matched[n]] + jitter
        for g in range(G):       # an ellipse inside its box
            x1, y1, x2, y2 = gt[n, g]
            masks[n, g] = ((((xx - (x1 + x2) / 2) / ((x2 - x1) / 2)) ** 2 + ((yy - (y1 + y2) / 2) / ((y2 - y1) / 2)) ** 2) <= 1)
    z = torch.zeros(1).cuda()
    bt = ops.BoxHeadTargets(torch.from_numpy(rois.reshape(N * B, 5)).cuda(), torch.from_numpy(labels).cuda(),
                            torch.from_numpy(matched).cuda(), z, z, z, z, z)
    g = torch.Generator().manual_seed(s["seed"])
    train_logits = (2.0 * torch.randn(N * P, C, M, M, generator=g)).cuda()
    det_logits = (2.0 * torch.randn(N * D, C, M, M, generator=g)).cuda()
    det_boxes = torch.from_numpy(np.stack([gt_like_boxes(r, D, H, W) for _ in range(N)])).cuda()
    det_labels = torch.from_numpy(r.integers(1, C, (N, D)).astype(np.int32)).cuda()
    det_count = torch.full((N,), D, dtype=torch.int32).cuda()
    return bt, masks.cuda(), train_logits, det_logits, det_boxes, det_labels, det_count


def composed_targets(bt, masks):
    import torch
    from replication_faster_rcnn_amd import ops
    s = SHAPE
    pos = torch.where(bt.labels.view(-1) > 0)[0]                  # a host sync
    x = masks[pos // s["B"], bt.matched.view(-1)[pos].long()].float()[:, None]
    rois = torch.cat([torch.arange(len(pos), device=pos.device, dtype=torch.float32)[:, None], bt.rois[pos][:, 1:]], 1)
    return ops.roi_align(x, rois, (s["M"], s["M"]), 1.0, -1, False)[:, 0]


def composed_loss(logits, tg):
    import torch
    import torch.nn.functional as TF
    x = logits.detach().requires_grad_(True)
    rows = torch.arange(x.shape[0], device=x.device)
    loss = TF.binary_cross_entropy_with_logits(x[rows, tg.labels.view(-1).long()].float(), tg.targets)
    loss.backward()
    return loss.detach(), x.grad


def op_loss(logits, tg):
    from replication_faster_rcnn_amd import ops
    x = logits.detach().requires_grad_(True)
    loss = ops.mask_head_losses(x, tg)
    loss.backward()
    return loss.detach(), x.grad


def composed_paste_loop(logits, boxes, labels, canvas, padding=1):
    """torchvision's maskrcnn_inference + paste_masks_in_image: one F.interpolate and one
    slice-assign per detection, with host ints of device boxes."""
    import torch
    import torch.nn.functional as TF
    N, D = labels.shape
    M = logits.shape[-1]
    Hc, Wc = canvas
    rows = torch.arange(N * D, device=logits.device)
    prob = TF.pad(logits[rows, labels.view(-1).long()].float().sigmoid(), (padding,) * 4)
    scale = float(M + 2 * padding) / M
    b = boxes.view(-1, 4)
    wh, hh = (b[:, 2] - b[:, 0]) * 0.5 * scale, (b[:, 3] - b[:, 1]) * 0.5 * scale
    xc, yc = (b[:, 2] + b[:, 0]) * 0.5, (b[:, 3] + b[:, 1]) * 0.5
    ib = torch.stack([xc - wh, yc - hh, xc + wh, yc + hh], 1).to(torch.int64)
    out = torch.zeros(N * D, Hc, Wc, dtype=torch.uint8, device=logits.device)
    for i in range(N * D):
        x0, y0, x1, y1 = (int(v) for v in ib[i])                   # a host sync per detection
        w, h = max(x1 - x0 + 1, 1), max(y1 - y0 + 1, 1)
        m = TF.interpolate(prob[i][None, None], size=(h, w), mode="bilinear", align_corners=False)[0, 0]
        xa, xb, ya, yb = max(x0, 0), min(x1 + 1, Wc), max(y0, 0), min(y1 + 1, Hc)
        out[i, ya:yb, xa:xb] = m[ya - y0:yb - y0, xa - x0:xb - x0] > 0.5
    return out.view(N, D, Hc, Wc)


def composed_paste_grid(logits, boxes, labels, canvas, padding=1):
    """The batched formulation: one F.grid_sample per image over the whole canvas (the grid of all
    800 detections at once is 2.3 GB), no host sync."""
    import torch
    import torch.nn.functional as TF
    N, D = labels.shape
    M = logits.shape[-1]
    Hc, Wc = canvas
    S = M + 2 * padding
    dev = logits.device
    rows = torch.arange(N * D, device=dev)
    prob = TF.pad(logits[rows, labels.view(-1).long()].float().sigmoid(), (padding,) * 4).view(N, D, 1, S, S)
    scale = float(S) / M
    b = boxes
    wh, hh = (b[..., 2] - b[..., 0]) * 0.5 * scale, (b[..., 3] - b[..., 1]) * 0.5 * scale
    xc, yc = (b[..., 2] + b[..., 0]) * 0.5, (b[..., 3] + b[..., 1]) * 0.5
    ib = torch.stack([xc - wh, yc - hh, xc + wh, yc + hh], -1).to(torch.int64).float()
    w = (ib[..., 2] - ib[..., 0] + 1).clamp(min=1)
    h = (ib[..., 3] - ib[..., 1] + 1).clamp(min=1)
    X = torch.arange(Wc, device=dev, dtype=torch.float32)
    Y = torch.arange(Hc, device=dev, dtype=torch.float32)
    out = torch.empty(N, D, Hc, Wc, dtype=torch.uint8, device=dev)
    for n in range(N):
        dx, dy = X[None, :] - ib[n, :, 0:1], Y[None, :] - ib[n, :, 1:2]                       # [D, Wc], [D, Hc]
        sx = ((S / w[n])[:, None] * (dx + 0.5) - 0.5).clamp(min=0)
        sy = ((S / h[n])[:, None] * (dy + 0.5) - 0.5).clamp(min=0)
        gx, gy = (sx + 0.5) * (2.0 / S) - 1, (sy + 0.5) * (2.0 / S) - 1
        grid = torch.stack([gx[:, None, :].expand(D, Hc, Wc), gy[:, :, None].expand(D, Hc, Wc)], -1)
        v = TF.grid_sample(prob[n], grid, mode="bilinear", padding_mode="border", align_corners=False)[:, 0]
        inside = ((dx >= 0) & (dx < w[n][:, None]))[:, None, :] & ((dy >= 0) & (dy < h[n][:, None]))[:, :, None]
        out[n] = (v > 0.5) & inside
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
    """The traced run: the ops alone, every variant and C."""
    import torch
    from replication_faster_rcnn_amd import ops
    s = SHAPE
    for C in CLASSES:
        bt, masks, tl, dl, boxes, labels, count = inputs(C)
        tg = None
        for _ in range(calls):
            tg = ops.mask_head_targets(bt, masks, mask_size=s["M"], positives_per_image=s["P"])
        for v in VARIANTS:
            x, d = tl.to(tdtype(v)), dl.to(tdtype(v))
            for _ in range(calls):
                op_loss(x, tg)
                ops.mask_head_paste(d, boxes, labels, count, (s["H"], s["W"]))
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
    rows = [r for r in csv.DictReader(open(files[0])) if "mh_" in r["Name"]]
    return [dict(name=kernel_name(r["Name"]), calls=int(r["Calls"]),
                 avg_us=round(float(r["AverageNs"]) / 1e3, 2), min_us=round(float(r["MinNs"]) / 1e3, 2))
            for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_head_bench.json"))
    ap.add_argument("--stats", default=None, help="also take the rocprofv3 per-kernel statistics, into this csv")
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "build_trace", "mask_head"))
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--baseline-calls", type=int, default=10)
    ap.add_argument("--loop-calls", type=int, default=1, help="calls per repetition of the per-detection paste loop")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    if args.calls < 200 or args.reps < 5:
        ap.error("--calls >= 200 and --reps >= 5")

    kernels = kernel_stats(args.stats, args.trace_dir, 50) if args.stats else []   # before this process opens the GPU

    import torch
    from replication_faster_rcnn_amd import ops
    s = SHAPE
    N, P, M, D, canvas = s["N"], s["P"], s["M"], s["D"], (s["H"], s["W"])
    result = dict(workload=dict(SHAPE, classes=list(CLASSES)), device=torch.cuda.get_device_name(0),
                  calls_per_rep=args.calls, baseline_calls_per_rep=args.baseline_calls,
                  loop_calls_per_rep=args.loop_calls, reps=args.reps, warmup=args.warmup,
                  baselines=dict(targets="torch.where + gt_masks[n, matched].float() + ops.roi_align",
                                 losses="indexed F.binary_cross_entropy_with_logits, forward + autograd backward",
                                 paste_loop="per-detection F.interpolate + slice-assign (torchvision's paste_masks_in_image)",
                                 paste_grid_sample="one F.grid_sample per image over the canvas"),
                  kernels_50_calls_per_variant=kernels, classes={})
    for C in CLASSES:
        bt, masks, tl, dl, boxes, labels, count = inputs(C)
        tgt_fn = lambda: ops.mask_head_targets(bt, masks, mask_size=M, positives_per_image=P)   # noqa: E731
        tg = tgt_fn()
        assert int(tg.count.min()) == P
        assert torch.equal(composed_targets(bt, masks), tg.targets), "targets differ from the composed path"
        entry = dict(plans=dict(targets=ops.mask_head_targets_kernel(s["B"], P, M),
                                losses=ops.mask_head_losses_kernel(C, M), paste=ops.mask_head_paste_kernel(M, canvas[1])))
        tx = {v: tl.to(tdtype(v)) for v in VARIANTS}
        dx = {v: dl.to(tdtype(v)) for v in VARIANTS}
        loss_fns = {v: (lambda x=tx[v]: op_loss(x, tg)) for v in VARIANTS}
        loss_base = {v: (lambda x=tx[v]: composed_loss(x, tg)) for v in VARIANTS}
        paste_fns = {v: (lambda x=dx[v]: ops.mask_head_paste(x, boxes, labels, count, canvas)) for v in VARIANTS}
        paste_prob = lambda: ops.mask_head_paste(dx["fp32"], boxes, labels, count, canvas, threshold=None)  # noqa: E731
        loop = lambda: composed_paste_loop(dx["fp32"], boxes, labels, canvas)                    # noqa: E731
        grid = lambda: composed_paste_grid(dx["fp32"], boxes, labels, canvas)                    # noqa: E731
        # agreement first
        for v in VARIANTS:
            (a, ga), (b, gb) = loss_fns[v](), loss_base[v]()
            assert abs(float(a) - float(b)) <= 1e-5 * max(1.0, abs(float(b))), (v, float(a), float(b))
            assert float((ga.float() - gb.float()).abs().max()) <= 2.0 ** -7 * float(gb.float().abs().max())
        mine = paste_fns["fp32"]()
        agree = {}
        for name, fn in (("paste_loop", loop), ("paste_grid_sample", grid)):
            other = fn()
            agree[name] = round(float((other == mine).float().mean()), 6)
            assert agree[name] >= 0.999, (name, agree[name])
            del other
        entry["pixels_equal_to_composed"] = agree
        del mine
        for f in [tgt_fn] + list(loss_fns.values()) + list(paste_fns.values()) + [paste_prob]:
            for _ in range(args.warmup):
                f()
        composed_targets(bt, masks)
        grid()
        t = dict(targets=[], targets_composed=[], paste_probabilities_fp32=[], paste_loop=[], paste_grid_sample=[])
        for v in VARIANTS:
            t[f"losses_{v}"], t[f"losses_composed_{v}"], t[f"paste_{v}"] = [], [], []
        for _ in range(args.reps):
            t["targets"].append(timed(tgt_fn, args.calls))
            for v in VARIANTS:
                t[f"losses_{v}"].append(timed(loss_fns[v], args.calls))
                t[f"paste_{v}"].append(timed(paste_fns[v], args.calls))
            t["paste_probabilities_fp32"].append(timed(paste_prob, max(args.calls // 4, 1)))
            t["targets_composed"].append(timed(lambda: composed_targets(bt, masks), args.baseline_calls))
            for v in VARIANTS:
                t[f"losses_composed_{v}"].append(timed(loss_base[v], args.baseline_calls))
            t["paste_grid_sample"].append(timed(grid, args.baseline_calls))
            t["paste_loop"].append(timed(loop, args.loop_calls))
        entry["times"] = {k: summary(v) for k, v in t.items()}
        mn = {k: min(v) for k, v in t.items()}
        entry["ratio_min_over_min"] = dict(
            targets=round(mn["targets_composed"] / mn["targets"], 2),
            **{f"losses_{v}": round(mn[f"losses_composed_{v}"] / mn[f"losses_{v}"], 2) for v in VARIANTS},
            **{f"paste_{v}_over_loop": round(mn["paste_loop"] / mn[f"paste_{v}"], 1) for v in VARIANTS},
            **{f"paste_{v}_over_grid_sample": round(mn["paste_grid_sample"] / mn[f"paste_{v}"], 1) for v in VARIANTS})
        paste_bytes = N * D * canvas[0] * canvas[1]
        grad_bytes = {v: N * P * C * M * M * (4 if v == "fp32" else 2) for v in VARIANTS}
        entry["paste_bytes_written"] = paste_bytes
        entry["paste_hbm_share_of_call"] = {
            v: dict(tb_per_s=round(paste_bytes / mn[f"paste_{v}"] / 1e6, 3),
                    of_spec_8_0_TBs=round(paste_bytes / mn[f"paste_{v}"] / 1e6 / SPEC_TBS, 3),
                    of_measured_copy_6_29_TBs=round(paste_bytes / mn[f"paste_{v}"] / 1e6 / COPY_TBS, 3)) for v in VARIANTS}
        entry["loss_gradient_bytes"] = grad_bytes
        result["classes"][str(C)] = entry
        print(f"C={C}: targets {mn['targets']:.1f} us (composed {mn['targets_composed']:.1f}); " +
              ", ".join(f"losses {v} {mn[f'losses_{v}']:.1f} (composed {mn[f'losses_composed_{v}']:.1f})" for v in VARIANTS) +
              "; " + ", ".join(f"paste {v} {mn[f'paste_{v}']:.1f}" for v in VARIANTS) +
              f" (loop {mn['paste_loop']:.0f}, grid_sample {mn['paste_grid_sample']:.0f}) us", flush=True)
        del bt, masks, tl, dl, tx, dx, tg
        torch.cuda.empty_cache()
    # the paste kernel's own time from the trace, where one was taken
    for k in kernels:
        if k["name"].startswith("mh_paste_kernel"):
            by = SHAPE["N"] * SHAPE["D"] * SHAPE["H"] * SHAPE["W"]
            k["tb_per_s_at_min"] = round(by / k["min_us"] / 1e6, 3)
            k["of_spec_8_0_TBs"] = round(by / k["min_us"] / 1e6 / SPEC_TBS, 3)
            k["of_measured_copy_6_29_TBs"] = round(by / k["min_us"] / 1e6 / COPY_TBS, 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
