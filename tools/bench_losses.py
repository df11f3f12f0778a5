"""Time the four training losses, forward and backward, fused (ops.rpn_losses +
ops.head_losses) against the dense PyTorch path Trainer.train_step runs without
``fused_losses`` (the casts, boolean-mask gathers, F.cross_entropy, the reg_ind
gather and autograd's backward of all that).

    python tools/bench_losses.py [--out profiles/losses_bench.json] [--trace-dir DIR]

Workload: the cfg5 shape of bench.py (16 images 600x600, 38x38x9 anchors, S = 128
sampled RoIs, 21 classes); synthetic logits and predictions, targets from one
real targets.anchor_targets / targets.proposal_targets call (numpy seed 0) on
ops.propose's RoIs.  Both sides are timed with device events in one process,
interleaved: per repetition --calls calls of each; 5 repetitions, min and median
reported, also as a share of the cfg5 step (profiles/r6_end_bench_cfg5a.json).
The per-kernel breakdown and the launch count come from a rocprofv3
--kernel-trace --stats run of its own (a child process that only calls the fused
path), taken before this process touches the GPU.  Both sides must agree on the
losses and the gradients.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

SHAPE = dict(N=16, img=600, feat=38, K=9, S=128, C=21, G=32, pre_nms=12000, post_nms=600, seed=0)
CFG5_RECORD = os.path.join(ROOT, "profiles", "r6_end_bench_cfg5a.json")


def device_inputs():
    """The two stages' inputs on the device: RPN (cls as the [N, 2, A] view RPN.forward returns,
    reg, reg_t fp64, labels int32) and head (cls as ResnetHead.forward's [N, C, S] view, reg
    [N, S, 4C], reg_t fp64, labels fp64), the four predictions as leaves requiring grad."""
    import numpy as np
    import torch
    from replication_faster_rcnn_amd import anchors as A, ops, synth, targets
    s = SHAPE
    dev = torch.device("cuda", 0)
    N, nA = s["N"], s["feat"] * s["feat"] * s["K"]
    base = A.generate_anchor_base_device()
    anchors = A.generate_anchors(base, 16, s["feat"], s["feat"]).to(dev)
    gl = [synth.gt_boxes(s["img"], s["img"], s["G"], s["seed"], i) for i in range(N)]
    boxes = torch.from_numpy(np.stack([b for b, _ in gl])).to(dev)
    labels = torch.from_numpy(np.stack([l for _, l in gl])).to(dev)
    sc = torch.from_numpy(np.stack([synth.rpn_scores(nA, s["seed"], i) for i in range(N)])).to(dev)
    de = torch.from_numpy(np.stack([synth.rpn_deltas(nA, s["seed"], i) for i in range(N)])).to(dev)
    rois, _, cnt = ops.propose(sc, de, img_w=s["img"], img_h=s["img"], pre_nms=s["pre_nms"], post_nms=s["post_nms"],
                               anchor_base=base, feat_h=s["feat"], feat_w=s["feat"])
    saved = np.random.get_state()
    np.random.seed(s["seed"])
    reg_t, lab = targets.anchor_targets(boxes, labels, anchors)
    _, s_reg, s_lab, s_cnt = targets.proposal_targets(rois, cnt, boxes, labels, n_sample=s["S"])
    np.random.set_state(saved)
    assert s_cnt.tolist() == [s["S"]] * N
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    leaf = lambda *shape, scale=1.0: (torch.randn(shape, device=dev, generator=gen) * scale).requires_grad_(True)  # noqa: E731
    rpn_cls, rpn_reg = leaf(N, nA, 2, scale=2.0), leaf(N, nA, 4, scale=0.2)
    head_cls, head_reg = leaf(N, s["S"], s["C"], scale=2.0), leaf(N, s["S"], 4 * s["C"], scale=0.2)
    return dict(leaves=[rpn_cls, rpn_reg, head_cls, head_reg],
                rpn=(rpn_cls.permute(0, 2, 1), rpn_reg, reg_t, lab),
                head=(head_cls.permute(0, 2, 1), head_reg, s_reg, s_lab))


def fused(inp):
    from replication_faster_rcnn_amd import ops
    for t in inp["leaves"]:
        t.grad = None
    rc, rr = ops.rpn_losses(*inp["rpn"])
    hc, hr = ops.head_losses(*inp["head"])
    (rc + rr + hc + hr).backward()
    return rc, rr, hc, hr


def dense(inp):
    """Trainer.train_step's loss lines without ``fused_losses`` (train.py:67-69, :81-83, :89-90, :112-126)."""
    import torch
    import torch.nn.functional as F
    from replication_faster_rcnn_amd.train import fast_rcnn_loc_loss
    for t in inp["leaves"]:
        t.grad = None
    cls, reg, reg_t, lab = inp["rpn"]
    reg_targets_rpn = reg_t.float()
    cls_labels_rpn = lab.float()
    rpn_reg_loss = fast_rcnn_loc_loss(reg, reg_targets_rpn, cls_labels_rpn)
    rpn_cls_loss = F.cross_entropy(cls, cls_labels_rpn.long(), ignore_index=-1)
    cls_output, reg_output, s_reg, s_lab = inp["head"]
    reg_targets_classifier = s_reg.float()
    cls_labels_classifier = s_lab.float()
    reg_ind = cls_labels_classifier.detach().unsqueeze(-1).long() * 4
    reg_ind = torch.cat([reg_ind, reg_ind + 1, reg_ind + 2, reg_ind + 3], dim=-1)
    reg_output = torch.gather(reg_output, dim=-1, index=reg_ind)
    reg_loss = fast_rcnn_loc_loss(reg_output, reg_targets_classifier, cls_labels_classifier)
    cls_loss = F.cross_entropy(cls_output, cls_labels_classifier.long(), ignore_index=-1)
    (rpn_cls_loss + rpn_reg_loss + cls_loss + reg_loss).backward()
    return rpn_cls_loss, rpn_reg_loss, cls_loss, reg_loss


def timed(fn, inp, calls):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn(inp)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls   # us per call


def summary(v):
    return dict(reps_us=[round(x, 2) for x in v], min_us=round(min(v), 2), median_us=round(statistics.median(v), 2))


def child(calls):
    """The traced run: the fused path alone."""
    import torch
    inp = device_inputs()
    for _ in range(calls):
        fused(inp)
    torch.cuda.synchronize()


def kernel_trace(trace_dir, calls):
    os.makedirs(trace_dir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "-o", "run", "--",
           sys.executable, os.path.abspath(__file__), "--child", str(calls)]
    subprocess.run(cmd, check=True, timeout=300, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise RuntimeError(f"rocprofv3 wrote no kernel_stats.csv under {trace_dir}")
    rows = [r for r in csv.DictReader(open(files[0])) if "losses_" in r["Name"]]
    kernels = [dict(name=r["Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", ""), calls=int(r["Calls"]),
                    avg_us=round(float(r["AverageNs"]) / 1e3, 2), min_us=round(float(r["MinNs"]) / 1e3, 2))
               for r in rows]
    launches = sum(k["calls"] for k in kernels) / (2.0 * calls)      # two stages per call
    return kernels, launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "losses_bench.json"))
    ap.add_argument("--trace-dir", default=None, help="also take the rocprofv3 per-kernel breakdown, into DIR")
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    if args.calls < 200 or args.reps < 5:
        ap.error("--calls >= 200 and --reps >= 5")

    kernels, launches = [], None
    if args.trace_dir:   # before this process initialises the GPU
        kernels, launches = kernel_trace(args.trace_dir, 100)

    import numpy as np
    import torch
    inp = device_inputs()
    # both sides agree: the losses at the tolerance tests/test_gpu_train.py uses, the gradients closely
    got = [float(v.detach()) for v in fused(inp)]
    g_fused = [t.grad.clone() for t in inp["leaves"]]
    want = [float(v.detach()) for v in dense(inp)]
    g_dense = [t.grad.clone() for t in inp["leaves"]]
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-7)
    grad_diff = [float((a - b).abs().max()) for a, b in zip(g_fused, g_dense)]
    for a, b in zip(g_fused, g_dense):
        assert torch.equal(a == 0, b == 0) and torch.allclose(a, b, rtol=1e-5, atol=1e-7)
    for _ in range(args.warmup):
        fused(inp)
        dense(inp)
    t_fused, t_dense = [], []
    for _ in range(args.reps):
        t_fused.append(timed(fused, inp, args.calls))
        t_dense.append(timed(dense, inp, args.calls))
    step_us = json.load(open(CFG5_RECORD))["ms_per_step"] * 1e3
    s = SHAPE
    result = dict(
        workload=dict(s, anchors_per_image=s["feat"] * s["feat"] * s["K"],
                      inputs="synthetic logits / predictions; targets from targets.anchor_targets and "
                             "targets.proposal_targets (numpy seed 0) on ops.propose's RoIs"),
        device=torch.cuda.get_device_name(0), calls_per_rep=args.calls, reps=args.reps, warmup=args.warmup,
        timed="forward + backward of the four losses (and the sum of the four), device events, interleaved",
        baseline="Trainer.train_step's dense PyTorch losses (casts, mask gathers, F.cross_entropy, reg_ind gather)",
        losses=dict(names=["rpn_cls", "rpn_reg", "cls", "reg"], fused=got, dense=want),
        grad_max_abs_diff=dict(zip(["rpn_cls", "rpn_reg", "head_cls", "head_reg"], grad_diff)),
        fused=summary(t_fused), dense=summary(t_dense),
        speedup_min_over_min=round(min(t_dense) / min(t_fused), 2),
        speedup_median_over_median=round(statistics.median(t_dense) / statistics.median(t_fused), 2),
        cfg5_step_us=round(step_us, 1), cfg5_step_record=os.path.relpath(CFG5_RECORD, ROOT),
        fused_share_of_cfg5_step=round(min(t_fused) / step_us, 3),
        dense_share_of_cfg5_step=round(min(t_dense) / step_us, 3),
        kernels=kernels, launches_per_stage=launches)
    print(f"fused {result['fused']['min_us']} us min / {result['fused']['median_us']} median, dense "
          f"{result['dense']['min_us']} / {result['dense']['median_us']} us; launches per stage {launches}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))
    assert min(t_fused) <= min(t_dense) and statistics.median(t_fused) <= statistics.median(t_dense), \
        "the fused losses are slower than the dense path"
    assert launches is None or launches <= 3, f"{launches} launches per stage"


if __name__ == "__main__":
    main()
