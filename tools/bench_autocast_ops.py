"""Time the ops that read the network's predictions on float16 / bfloat16 predictions against
their fp32 kernels and against what a mixed-precision caller ran before the 16-bit kernels
existed (``.float()`` in, fp32 op, gradients ``.to(T)`` by autograd).

    python tools/bench_autocast_ops.py [--out profiles/autocast_ops_bench.json]

Ops and shapes:
  epilogue   cfg2: conv outputs 8 x 18 x 38 x 63 and 8 x 36 x 38 x 63 -> ops.rpn_head_epilogue_with_deltas
             (forward; its backward is two torch permutes in every variant)
  rpn_losses cfg5: 16 images x 38 x 38 x 9 anchors, 2 classes, 256 labelled anchors per image
             (128 positive), forward + backward (torch.autograd.grad of cls_loss + reg_loss)
  head_losses cfg5: 16 images x 128 samples, 21 classes, 32 positive samples per image, forward + backward
  detect     cfg2: 8 images x 300 RoIs x 21 classes (synth.head_outputs), score threshold 0.05
Variants per op: (a) ``fp32``; (b) ``fp16`` / ``bf16``, the 16-bit path; (c) ``<T>_via_fp32_casts``,
the 16-bit tensors widened with ``.float()`` in front of the fp32 op (for the losses the gradients
come back through autograd's ``.to(T)``); and for the epilogue ``<T>_strip128``, the 16-bit kernel
with 128-pixel strips instead of 64 (frcnn_set_path "rpn_epilogue_strip").  All variants run in
one process, interleaved: per repetition --calls calls of each, 5 repetitions.  Per variant the
wall time per call (host clock around the calls and a final synchronise: what a caller pays,
launch latency included) and the device time per call (HIP events around the same calls), min
and median over the repetitions.  (b) must equal (c) bit for bit before anything is timed.
The Python calls are bound by the host's issue rate (an autograd Function, the output
allocations and one ctypes call per op), so the epilogue's kernel is also timed alone:
``epilogue_cfg2_kernel`` calls the C-ABI entry point back to back on preallocated outputs
(fp32, and each 16-bit type with 64- and 128-pixel strips), the A/B behind the strip width.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

SEED = 0


def timed(fn, calls):
    """(wall us per call, device us per call) of `calls` back-to-back calls."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    t1 = time.perf_counter()
    return (t1 - t0) * 1e6 / calls, e0.elapsed_time(e1) * 1e3 / calls


def summary(wall, dev, nbytes=None):
    d = dict(wall_reps_us=[round(x, 2) for x in wall], wall_min_us=round(min(wall), 2),
             wall_median_us=round(statistics.median(wall), 2),
             device_reps_us=[round(x, 2) for x in dev], device_min_us=round(min(dev), 2),
             device_median_us=round(statistics.median(dev), 2))
    if nbytes is not None:
        d["alg_bytes"] = int(nbytes)
    return d


def bits(t):
    import torch
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def build_variants():
    import numpy as np
    import torch
    from replication_faster_rcnn_amd import _lib, ops, synth
    dev = torch.device("cuda", 0)
    halves = {"fp16": torch.float16, "bf16": torch.bfloat16}
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED)
    variants, nbytes, shapes = {}, {}, {}

    # ---- epilogue, cfg2
    N, K, H, W = 8, 9, 38, 63
    cls32 = torch.randn((N, 2 * K, H, W), device=dev, generator=gen)
    reg32 = torch.randn((N, 4 * K, H, W), device=dev, generator=gen) * 0.2
    v = {"fp32": lambda: ops.rpn_head_epilogue_with_deltas(cls32, reg32, K)}
    px = N * K * H * W
    nb = {"fp32": px * (6 * 4 + 7 * 4)}
    for k, t in halves.items():
        c16, r16 = cls32.to(t), reg32.to(t)
        v[k] = (lambda c16=c16, r16=r16: ops.rpn_head_epilogue_with_deltas(c16, r16, K))
        v[f"{k}_via_fp32_casts"] = (lambda c16=c16, r16=r16: ops.rpn_head_epilogue_with_deltas(
            c16.float().contiguous(), r16.float().contiguous(), K))

        def wide(c16=c16, r16=r16):
            _lib.set_path("rpn_epilogue_strip", "128")
            try:
                return ops.rpn_head_epilogue_with_deltas(c16, r16, K)
            finally:
                _lib.set_path("rpn_epilogue_strip", "auto")

        v[f"{k}_strip128"] = wide
        nb[k] = nb[f"{k}_strip128"] = px * (6 * 2 + 6 * 2 + 5 * 4)
        a, b, s = v[k](), v[f"{k}_via_fp32_casts"](), wide()
        assert torch.equal(bits(a[1]), bits(b[1])) and torch.equal(bits(a[3]), bits(b[2])), k
        assert torch.equal(bits(a[0]), bits(b[0].to(t))) and torch.equal(bits(a[2]), bits(b[2].to(t))), k
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, s)), k
    variants["epilogue_cfg2"], nbytes["epilogue_cfg2"] = v, nb
    shapes["epilogue_cfg2"] = dict(N=N, K=K, H=H, W=W)

    # the kernel alone: the C-ABI entry point on preallocated outputs
    lib = _lib.load()
    A = H * W * K
    fg = torch.empty((N, A), device=dev)
    de = torch.empty((N, A, 4), device=dev)
    kv, knb = {}, {}
    for k, t in {"fp32": torch.float32, **halves}.items():
        c, r = cls32.to(t), reg32.to(t)
        oc, orr = torch.empty((N, A, 2), dtype=t, device=dev), torch.empty((N, A, 4), dtype=t, device=dev)
        code = _lib.DTYPE_CODES[t]

        def direct(c=c, r=r, oc=oc, orr=orr, code=code):
            _lib.check(lib.frcnn_rpn_head_epilogue_t(code, c.data_ptr(), r.data_ptr(), N, K, H, W, oc.data_ptr(),
                                                     fg.data_ptr(), orr.data_ptr(), de.data_ptr(),
                                                     _lib.stream_ptr()), "epilogue")

        if k == "fp32":
            kv[k], knb[k] = direct, nb[k]
            continue
        for strip in ("64", "128"):
            def strip_call(direct=direct, strip=strip):
                _lib.set_path("rpn_epilogue_strip", strip)
                try:
                    direct()
                finally:
                    _lib.set_path("rpn_epilogue_strip", "auto")
            kv[f"{k}_strip{strip}"], knb[f"{k}_strip{strip}"] = strip_call, nb[k]
    variants["epilogue_cfg2_kernel"], nbytes["epilogue_cfg2_kernel"] = kv, knb
    shapes["epilogue_cfg2_kernel"] = dict(N=N, K=K, H=H, W=W)

    # ---- losses, cfg5
    def stage(name, n, L, C, head, n_lab, n_pos):
        rs = np.random.RandomState(SEED + C)
        rows = n * L
        lab = np.full((n, L), -1, np.int64)
        for i in range(n):
            sel = rs.permutation(L)[:n_lab]
            lab[i, sel[:n_pos]] = rs.randint(1, C, n_pos)
            lab[i, sel[n_pos:]] = 0
        labels = torch.from_numpy(lab.astype(np.float64 if head else np.int32)).to(dev)
        c32 = torch.randn((n, L, C), device=dev, generator=gen) * 2
        r32 = torch.randn((n, L, 4 * C if head else 4), device=dev, generator=gen)
        reg_t = torch.randn((n, L, 4), device=dev, generator=gen, dtype=torch.float64) * 1.5
        op = ops.head_losses if head else ops.rpn_losses

        def step(c, r, cast):
            cl, rl = op(c.float() if cast else c, r.float() if cast else r, reg_t, labels)
            return torch.autograd.grad(cl + rl, [c, r]) + (cl.detach(), rl.detach())

        c32.requires_grad_(True)
        r32.requires_grad_(True)
        v = {"fp32": lambda: step(c32, r32, False)}
        W4 = r32.shape[2]
        fixed = rows * (8 if head else 4) + n * n_lab * 32      # labels; targets of the labelled rows
        nb = {"fp32": fixed + 2 * n * n_lab * (C + 4) * 4 + rows * (C + W4) * 4}
        for k, t in halves.items():
            c16 = c32.detach().to(t).requires_grad_(True)
            r16 = r32.detach().to(t).requires_grad_(True)
            v[k] = (lambda c16=c16, r16=r16: step(c16, r16, False))
            v[f"{k}_via_fp32_casts"] = (lambda c16=c16, r16=r16: step(c16, r16, True))
            nb[k] = fixed + 2 * n * n_lab * (C + 4) * 2 + rows * (C + W4) * 2
            a, b = v[k](), v[f"{k}_via_fp32_casts"]()
            assert all(x.dtype == y.dtype and torch.equal(bits(x), bits(y)) for x, y in zip(a, b)), (name, k)
            assert a[0].dtype == t and a[1].dtype == t
        variants[name], nbytes[name] = v, nb
        shapes[name] = dict(N=n, L=L, C=C, labelled_per_image=n_lab, positive_per_image=n_pos)

    stage("rpn_losses_cfg5", 16, 38 * 38 * 9, 2, False, 256, 128)
    stage("head_losses_cfg5", 16, 128, 21, True, 128, 32)

    # ---- detect, cfg2
    N, R, C = 8, 300, 21
    rois, rc, cls, reg = (torch.from_numpy(a).to(dev) for a in synth.head_outputs(N, R, C, 600, 1000, seed=SEED))
    kw = dict(img_h=600, img_w=1000, score_thresh=0.05)
    v = {"fp32": lambda: ops.detect(rois, rc, cls, reg, **kw)}
    other = N * R * 16 + N * 4 + N * R * C * 4 * 2 + N * R * (C - 1) * 28      # rois, rcount, prob, outputs
    nb = {"fp32": N * R * 5 * C * 4 + other}
    for k, t in halves.items():
        c16, r16 = cls.to(t), reg.to(t)
        v[k] = (lambda c16=c16, r16=r16: ops.detect(rois, rc, c16, r16, **kw))
        v[f"{k}_via_fp32_casts"] = (lambda c16=c16, r16=r16: ops.detect(rois, rc, c16.float(), r16.float(), **kw))
        nb[k] = N * R * 5 * C * 2 + other
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(v[k](), v[f"{k}_via_fp32_casts"]())), k
    variants["detect_cfg2"], nbytes["detect_cfg2"] = v, nb
    shapes["detect_cfg2"] = dict(N=N, R=R, C=C)
    return variants, nbytes, shapes, list(halves)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "autocast_ops_bench.json"))
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.calls < 200 or args.reps < 5:
        ap.error("--calls >= 200 and --reps >= 5")

    import torch
    variants, nbytes, shapes, halves = build_variants()
    result = dict(device=torch.cuda.get_device_name(0), calls_per_rep=args.calls, reps=args.reps, warmup=args.warmup,
                  timed="per repetition --calls back-to-back calls of each variant, variants interleaved, one process; "
                        "wall = host clock around the calls and a final synchronise, device = HIP events around them",
                  bytes="algorithmic: every tensor a kernel of the variant reads or writes once (losses: the "
                        "labels, the labelled rows' predictions and targets in forward and backward, both gradients)",
                  shapes=shapes, results={})
    for op, vs in variants.items():
        for _ in range(args.warmup):
            for f in vs.values():
                f()
        wall = {v: [] for v in vs}
        devt = {v: [] for v in vs}
        for _ in range(args.reps):
            for v, f in vs.items():
                w, d = timed(f, args.calls)
                wall[v].append(w)
                devt[v].append(d)
        rec = {v: summary(wall[v], devt[v], nbytes[op].get(v)) for v in vs}
        for k in halves:
            if f"{k}_via_fp32_casts" not in rec:
                continue
            b, c = rec[k], rec[f"{k}_via_fp32_casts"]
            b["vs_fp32_wall_median"] = round(b["wall_median_us"] / rec["fp32"]["wall_median_us"], 3)
            b["vs_casts_wall_median"] = round(b["wall_median_us"] / c["wall_median_us"], 3)
            b["vs_casts_device_median"] = round(b["device_median_us"] / c["device_median_us"], 3)
            # the expectation: (b)'s median is not above (c)'s by more than the repetitions' spread
            spread = max(max(x["wall_reps_us"]) - min(x["wall_reps_us"]) for x in (b, c))
            b["spread_us"] = round(spread, 2)
            b["not_above_casts"] = bool(b["wall_median_us"] <= c["wall_median_us"] + spread)
        result["results"][op] = rec
        print(op, {v: (r["wall_median_us"], r["device_median_us"]) for v, r in rec.items()}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
