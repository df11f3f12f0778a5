"""Time the pyramid RPN's training half (ops.rpn_targets_multilevel, ops.rpn_losses_multilevel
forward + backward; fp32, float16, bfloat16) against the composed path a user writes with torch.

    python tools/bench_rpn_targets.py [--out profiles/rpn_targets_bench.json]
    python tools/bench_rpn_targets.py --loop 50      # the ops alone, untimed: for a kernel trace

Shape: cfg2's batch behind an FPN -- 8 images of 600 x 600, RPN head outputs on maps of 150^2,
75^2, 38^2, 19^2 and 10^2 (strides 4 .. 64), K = 3 anchors per cell (sizes 32 .. 512, ratios
1/2, 1, 2): 90,090 anchors per image; G = 32 gt rows of which 1 .. 20 are real.  Logits are
standard normal, deltas normal with sigma 0.1.

Variants:
  op_targets            ops.rpn_targets_multilevel: five launches, no host sync, outputs allocated per call
  composed_targets      torchvision's assign_targets_to_anchors, Matcher, BalancedPositiveNegativeSampler
                        and BoxCoder.encode restated with torch ops per image: the dense [G, A] IoU,
                        max, where, two randperms (torch's stream: other samples; the counts are
                        compared and recorded, not asserted equal)
  op_losses_<dtype>     ops.rpn_losses_multilevel and its backward (torch.autograd.grad to all 10 maps)
  composed_losses_<dt>  concat_box_prediction_layers (permute + reshape + cat), index by the sampled
                        anchors, F.binary_cross_entropy_with_logits, F.smooth_l1_loss, autograd

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

IMG, BATCH, K, G, B = 600, 8, 3, 32, 256
SIZES = [150, 75, 38, 19, 10]
STRIDES = [4, 8, 16, 32, 64]
ANCHOR_SIZES = ((32,), (64,), (128,), (256,), (512,))
COUNTS = [3, 7, 1, 12, 5, 2, 20, 9]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rpn_targets_bench.json"))
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
    L = len(SIZES)
    strides = [(s, s) for s in STRIDES]
    grids = [(s, s) for s in SIZES]
    bases = ops.pyramid_anchor_bases(ANCHOR_SIZES, ((0.5, 1.0, 2.0),) * L)
    anchors = torch.cat(ops.pyramid_anchors(bases, strides, grids)).to(dev)
    bases = [b.to(dev) for b in bases]
    A = anchors.size(0)
    cpu = torch.Generator().manual_seed(1)
    xy = torch.rand(BATCH, G, 2, generator=cpu) * (IMG - 40)
    wh = 24 + torch.rand(BATCH, G, 2, generator=cpu) ** 2 * 400
    gt = torch.cat([xy, torch.minimum(xy + wh, torch.tensor(float(IMG)))], dim=2).round().to(dev)
    gt_count = torch.tensor(COUNTS, dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    obj32 = [torch.randn((BATCH, K, s, s), device=dev, generator=gen) for s in SIZES]
    del32 = [torch.randn((BATCH, 4 * K, s, s), device=dev, generator=gen) * 0.1 for s in SIZES]
    rng = ops.sampler_state(1, dev)

    def op_targets():
        return ops.rpn_targets_multilevel(gt, gt_count, bases, strides, grids, rng)

    def composed_targets():
        labels, regs = [], []
        for n in range(BATCH):
            g = gt[n, :COUNTS[n]]
            area_g = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
            area_a = (anchors[:, 2] - anchors[:, 0]) * (anchors[:, 3] - anchors[:, 1])
            wh_ = (torch.min(g[:, None, 2:], anchors[:, 2:]) - torch.max(g[:, None, :2], anchors[:, :2])).clamp(min=0)
            inter = wh_[:, :, 0] * wh_[:, :, 1]
            iou = inter / (area_g[:, None] + area_a - inter)
            vals, m = iou.max(dim=0)
            every = m.clone()
            m[vals < 0.3] = -1
            m[(vals >= 0.3) & (vals < 0.7)] = -2
            pred = torch.where(iou == iou.max(dim=1).values[:, None])[1]
            m[pred] = every[pred]
            pos, neg = torch.where(m >= 0)[0], torch.where(m == -1)[0]
            num_pos = min(pos.numel(), B // 2)
            num_neg = min(neg.numel(), B - num_pos)
            sp = pos[torch.randperm(pos.numel(), device=dev)[:num_pos]]
            sn = neg[torch.randperm(neg.numel(), device=dev)[:num_neg]]
            lab = torch.full((A,), -1.0, device=dev)
            lab[sp], lab[sn] = 1.0, 0.0
            mg = g[m.clamp(min=0)]
            aw, ah = anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
            acx, acy = anchors[:, 0] + 0.5 * aw, anchors[:, 1] + 0.5 * ah
            gw, gh = mg[:, 2] - mg[:, 0], mg[:, 3] - mg[:, 1]
            gcx, gcy = mg[:, 0] + 0.5 * gw, mg[:, 1] + 0.5 * gh
            regs.append(torch.stack([(gcx - acx) / aw, (gcy - acy) / ah, torch.log(gw / aw), torch.log(gh / ah)], dim=1))
            labels.append(lab)
        return torch.stack(labels), torch.stack(regs)

    def composed_losses(objs, dels, labels, regs):
        x = torch.cat([o.permute(0, 2, 3, 1).reshape(BATCH, -1) for o in objs], dim=1).reshape(-1)
        d = torch.cat([t.view(BATCH, K, 4, t.shape[2], t.shape[3]).permute(0, 3, 4, 1, 2).reshape(BATCH, -1, 4)
                       for t in dels], dim=1).reshape(-1, 4)
        lab, reg = labels.reshape(-1), regs.reshape(-1, 4)
        sp = torch.where(lab == 1)[0]
        si = torch.where(lab >= 0)[0]
        box = F.smooth_l1_loss(d[sp].float(), reg[sp], beta=1 / 9, reduction="sum") / si.numel()
        obj = F.binary_cross_entropy_with_logits(x[si].float(), lab[si])
        return torch.autograd.grad(obj + box, objs + dels)

    tg = op_targets()
    again = ops.rpn_targets_multilevel(gt, gt_count, bases, strides, grids, ops.sampler_state(1, dev))
    assert all(torch.equal(a, b) for a, b in zip(tg[:5], again[:5]))
    labels, regs = composed_targets()
    variants, calls = {"op_targets": op_targets, "composed_targets": composed_targets}, {}
    calls["op_targets"], calls["composed_targets"] = args.calls, args.composed_calls
    meta = dict(n_pos=tg.n_pos.cpu().tolist(), n_neg=tg.n_neg.cpu().tolist(),
                composed_n_pos=(labels == 1).sum(dim=1).cpu().tolist(), composed_n_neg=(labels == 0).sum(dim=1).cpu().tolist(),
                positives=(tg.matches >= 0).sum(dim=1).cpu().tolist(), kernels=ops.rpn_targets_multilevel_kernel(K, grids, BATCH, G, B))
    meta["counts_equal"] = meta["n_pos"] == meta["composed_n_pos"] and meta["n_neg"] == meta["composed_n_neg"]
    for k, t in dts.items():
        objs = [x.to(t).requires_grad_(True) for x in obj32]
        dels = [x.to(t).requires_grad_(True) for x in del32]

        def op_losses(objs=objs, dels=dels):
            a, b = ops.rpn_losses_multilevel(objs, dels, tg)
            return torch.autograd.grad(a + b, objs + dels)
        variants[f"op_losses_{k}"], calls[f"op_losses_{k}"] = op_losses, args.calls
        variants[f"composed_losses_{k}"] = (lambda objs=objs, dels=dels: composed_losses(objs, dels, labels, regs))
        calls[f"composed_losses_{k}"] = args.composed_calls

    if args.loop:
        for _ in range(args.loop):
            op_targets()
            for k in dts:
                variants[f"op_losses_{k}"]()
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
                  shape=dict(N=BATCH, image=IMG, maps=SIZES, strides=STRIDES, K=K, anchors_per_image=A, G=G, gt_count=COUNTS,
                             anchor_sizes=[s[0] for s in ANCHOR_SIZES], batch_size_per_image=B),
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
