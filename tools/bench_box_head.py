"""Time the pyramid box head's training half (ops.box_head_targets, ops.box_head_losses forward +
backward; fp32, float16, bfloat16; C = 21 and 91) against the composed path a user writes with torch.

    python tools/bench_box_head.py [--out profiles/box_head_bench.json]
    python tools/bench_box_head.py --loop 50      # the ops alone, untimed: for a kernel trace

Shape: cfg2's batch behind an FPN -- 8 images of 600 x 600, R = 1,000 real proposals per image (a third
of them a gt moved by a few pixels, so both classes are well filled), G = 32 gt rows of which 1 .. 20 are
real, B = 512 samples per image.  Logits are standard normal, box predictions normal with sigma 0.5.

Variants:
  op_targets              ops.box_head_targets: two launches, no host sync, outputs allocated per call
  composed_targets        torchvision's select_training_samples restated with torch ops per image: cat
                          (add_gt_proposals), the dense [G, R+G] IoU, max, where, two randperms (torch's
                          stream: other samples; the counts are compared and recorded), index, encode
  op_losses_<C>_<dtype>   ops.box_head_losses and its backward (torch.autograd.grad to both predictions)
  composed_losses_<C>_<dt>  F.cross_entropy, the [S, C, 4] view indexed by the positives' labels,
                          F.smooth_l1_loss(beta, "sum") / numel, autograd

All are timed with device events in one process, interleaved: per repetition --calls calls of each op,
--composed-calls of each composed path; 5 repetitions, min and median reported.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

from bench_roi_pool_half import summary, timed  # noqa: E402

IMG, BATCH, R, G, B = 600, 8, 1000, 32, 512
COUNTS = [3, 7, 1, 12, 5, 2, 20, 9]
CLASSES = (21, 91)
WEIGHTS = (10.0, 10.0, 5.0, 5.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_head_bench.json"))
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--composed-calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop", type=int, default=0, help="run the ops this many times and exit (no timing)")
    args = ap.parse_args()
    if not args.loop and (args.calls < 200 or args.composed_calls < 10 or args.reps < 5):
        ap.error("--calls >= 200, --composed-calls >= 10 and --reps >= 5")

    import torch
    import torch.nn.functional as F
    from replication_faster_rcnn_amd import ops
    dev = torch.device("cuda", 0)
    dts = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
    cpu = torch.Generator().manual_seed(1)
    xy = torch.rand(BATCH, G, 2, generator=cpu) * (IMG - 40)
    wh = 24 + torch.rand(BATCH, G, 2, generator=cpu) ** 2 * 400
    gt = torch.cat([xy, torch.minimum(xy + wh, torch.tensor(float(IMG)))], dim=2).round()
    pxy = torch.rand(BATCH, R, 2, generator=cpu) * (IMG - 40)
    pwh = 16 + torch.rand(BATCH, R, 2, generator=cpu) ** 2 * 300
    props = torch.cat([pxy, torch.minimum(pxy + pwh, torch.tensor(float(IMG)))], dim=2).round()
    for n, c in enumerate(COUNTS):   # a third of the proposals lie near a real gt row
        near = torch.rand(R, generator=cpu) < 1 / 3
        which = torch.randint(0, c, (R,), generator=cpu)
        moved = gt[n, which] + torch.randint(-6, 7, (R, 4), generator=cpu).float()
        moved[:, 2:] = torch.maximum(moved[:, 2:], moved[:, :2] + 4)
        props[n, near] = moved[near]
    gt, props = gt.to(dev), props.to(dev).contiguous()
    gt_labels = torch.randint(1, min(CLASSES), (BATCH, G), generator=cpu).to(torch.int32).to(dev)
    gt_count = torch.tensor(COUNTS, dtype=torch.int32, device=dev)
    prop_count = torch.full((BATCH,), R, dtype=torch.int32, device=dev)
    rng = ops.sampler_state(1, dev)
    wts = torch.tensor(WEIGHTS, device=dev)

    def op_targets():
        return ops.box_head_targets(props, prop_count, gt, gt_labels, gt_count, rng, batch_size_per_image=B)

    def composed_targets():
        rois, labels, regs = [], [], []
        for n in range(BATCH):
            g, gl = gt[n, :COUNTS[n]], gt_labels[n, :COUNTS[n]].long()
            p = torch.cat((props[n], g))
            area_g = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
            area_p = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
            wh_ = (torch.min(g[:, None, 2:], p[:, 2:]) - torch.max(g[:, None, :2], p[:, :2])).clamp(min=0)
            inter = wh_[:, :, 0] * wh_[:, :, 1]
            vals, m = (inter / (area_g[:, None] + area_p - inter)).max(dim=0)
            m[vals < 0.5] = -1
            lab = gl[m.clamp(min=0)]
            lab[m == -1] = 0
            pos, neg = torch.where(lab >= 1)[0], torch.where(lab == 0)[0]
            num_pos = min(pos.numel(), B // 4)
            num_neg = min(neg.numel(), B - num_pos)
            mask = torch.zeros_like(lab, dtype=torch.bool)
            mask[pos[torch.randperm(pos.numel(), device=dev)[:num_pos]]] = True
            mask[neg[torch.randperm(neg.numel(), device=dev)[:num_neg]]] = True
            idx = torch.where(mask)[0]
            sp, sg = p[idx], g[m[idx].clamp(min=0)]
            w, h = sp[:, 2] - sp[:, 0], sp[:, 3] - sp[:, 1]
            cx, cy = sp[:, 0] + 0.5 * w, sp[:, 1] + 0.5 * h
            gw, gh = sg[:, 2] - sg[:, 0], sg[:, 3] - sg[:, 1]
            gcx, gcy = sg[:, 0] + 0.5 * gw, sg[:, 1] + 0.5 * gh
            regs.append(torch.stack([wts[0] * (gcx - cx) / w, wts[1] * (gcy - cy) / h, wts[2] * torch.log(gw / w),
                                     wts[3] * torch.log(gh / h)], dim=1))
            rois.append(sp)
            labels.append(lab[idx])
        return rois, torch.cat(labels), torch.cat(regs)

    def composed_losses(cls, reg, labels, regs):
        lc = F.cross_entropy(cls.float(), labels)
        pos = torch.where(labels > 0)[0]
        sel = reg.float().reshape(cls.shape[0], cls.shape[1], 4)[pos, labels[pos]]
        lb = F.smooth_l1_loss(sel, regs[pos], beta=1 / 9, reduction="sum") / labels.numel()
        return torch.autograd.grad(lc + lb, (cls, reg))

    tg = op_targets()
    again = ops.box_head_targets(props, prop_count, gt, gt_labels, gt_count, ops.sampler_state(1, dev),
                                 batch_size_per_image=B)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(tg, again))
    _, clabels, cregs = composed_targets()
    variants, calls = {"op_targets": op_targets, "composed_targets": composed_targets}, {}
    calls["op_targets"], calls["composed_targets"] = args.calls, args.composed_calls
    meta = dict(n_pos=tg.n_pos.cpu().tolist(), n_neg=tg.n_neg.cpu().tolist(),
                positives=[int(((tg.matches[n] >= 0)).sum()) for n in range(BATCH)],
                composed_samples=int(clabels.numel()), composed_positives=int((clabels > 0).sum()),
                kernels=ops.box_head_targets_kernel(R, G, BATCH, B))
    meta["counts_equal"] = (meta["composed_samples"] == sum(meta["n_pos"]) + sum(meta["n_neg"])
                            and meta["composed_positives"] == sum(meta["n_pos"]))
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    S = int(clabels.numel())
    for C in CLASSES:
        cls32 = torch.randn((BATCH * B, C), device=dev, generator=gen)
        reg32 = torch.randn((BATCH * B, 4 * C), device=dev, generator=gen) * 0.5
        for k, t in dts.items():
            cls, reg = cls32.to(t).requires_grad_(True), reg32.to(t).requires_grad_(True)
            ccls, creg = cls32[:S].to(t).requires_grad_(True), reg32[:S].to(t).requires_grad_(True)

            def op_losses(cls=cls, reg=reg):
                a, b = ops.box_head_losses(cls, reg, tg)
                return torch.autograd.grad(a + b, (cls, reg))
            variants[f"op_losses_{C}_{k}"], calls[f"op_losses_{C}_{k}"] = op_losses, args.calls
            variants[f"composed_losses_{C}_{k}"] = (lambda c=ccls, r=creg: composed_losses(c, r, clabels, cregs))
            calls[f"composed_losses_{C}_{k}"] = args.composed_calls

    if args.loop:
        for _ in range(args.loop):
            op_targets()
            for v, f in variants.items():
                if v.startswith("op_losses"):
                    f()
        torch.cuda.synchronize()
        print(json.dumps({"looped": args.loop}))
        return

    times = {v: [] for v in variants}
    for _ in range(args.warmup):
        for f in variants.values():
            f()
    for _ in range(args.reps):
        for v, f in variants.items():
            times[v].append(timed(f, calls[v]))
    res = {v: summary(t) for v, t in times.items()}
    for v in res:
        if v.startswith("op_"):
            res[v]["speedup_vs_composed_min"] = round(res["composed_" + v[3:]]["min_us"] / res[v]["min_us"], 2)
    res["op_targets"].update(meta)
    result = dict(device=torch.cuda.get_device_name(0), calls_per_rep=calls, reps=args.reps, warmup=args.warmup,
                  timed="device events around back-to-back calls, variants interleaved per repetition, one process",
                  shape=dict(N=BATCH, image=IMG, R=R, G=G, gt_count=COUNTS, batch_size_per_image=B, classes=list(CLASSES),
                             reg_weights=list(WEIGHTS)),
                  results=res)
    for v, r in res.items():
        print(v, r["min_us"], r["median_us"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
