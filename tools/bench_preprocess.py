"""Time the batched image preprocessing (ops.preprocess: resize as
skimage.transform.resize does + ToTensor + Normalize, one launch) against a
per-image PyTorch path on the same device and, where scipy imports, against the
two scipy.ndimage calls of the contract on the host.

    python tools/bench_preprocess.py [--out profiles/preprocess_bench.json] [--trace-dir DIR]

Workload: cfg2's batch, 8 images of 375 x 500 x 3 uint8 (synth.image, seed 0)
resized to 600 x 600; the packed pixels are uploaded once, outside the timed
region, and the outputs are caller-owned.  Device and PyTorch sides are timed
with device events in one process, interleaved: per repetition --calls calls of
each; 5 repetitions, min and median reported.  The record carries the bytes the
algorithm moves (every source byte read once, every output element written
once) and their share of the HBM rate at the min time.

The PyTorch baseline (.float() / 255, permute, F.interpolate(bilinear),
normalise, per image) clamps at the edges where the contract mirrors, and has
no anti-aliasing: it differs from the contract at the borders (by up to 0.26
before normalisation) and is there for TIME ONLY.  The scipy path is the
contract itself, in fp64 on the host, 5 x 3 calls.
The per-kernel time comes from a rocprofv3 --kernel-trace --stats run of its
own (a child process that only calls ops.preprocess), taken before this
process touches the GPU.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

SHAPE = dict(N=8, h=375, w=500, out_h=600, out_w=600, seed=0)
HBM_SPEC_TBS = 8.0        # MI355X HBM3E peak, datasheet
HBM_COPY_TBS = 6.29       # what a float4 copy kernel reaches on it


def host_images():
    from replication_faster_rcnn_amd import synth
    s = SHAPE
    return [synth.image(s["h"], s["w"], s["seed"], i) for i in range(s["N"])]


def device_inputs():
    import torch
    from replication_faster_rcnn_amd import data
    s = SHAPE
    dev = torch.device("cuda", 0)
    images = host_images()
    pixels, offset, hw, max_hw = data.pack_images(images)
    return dict(images=images, pixels=pixels.to(dev), offset=offset.to(dev), hw=hw.to(dev), max_hw=max_hw,
                per_image=[torch.from_numpy(im).to(dev) for im in images],
                out=torch.empty((s["N"], 3, s["out_h"], s["out_w"]), dtype=torch.float32, device=dev),
                out_torch=torch.empty((s["N"], 3, s["out_h"], s["out_w"]), dtype=torch.float32, device=dev),
                status=torch.empty((s["N"],), dtype=torch.int32, device=dev),
                mean=torch.tensor([0.485, 0.456, 0.406], device=dev).view(3, 1, 1),
                std=torch.tensor([0.229, 0.224, 0.225], device=dev).view(3, 1, 1))


def fused(inp):
    from replication_faster_rcnn_amd import ops
    s = SHAPE
    return ops.preprocess(inp["pixels"], inp["offset"], inp["hw"], (s["out_h"], s["out_w"]), max_hw=inp["max_hw"],
                          out=inp["out"], status=inp["status"])


def torch_path(inp):
    """Per image: ToTensor, a bilinear resize, Normalize.  Edge rule: clamp (not the contract's mirror)."""
    import torch.nn.functional as F
    s = SHAPE
    for i, im in enumerate(inp["per_image"]):
        x = (im.float() / 255).permute(2, 0, 1)[None]
        x = F.interpolate(x, size=(s["out_h"], s["out_w"]), mode="bilinear", align_corners=False)
        inp["out_torch"][i] = (x[0] - inp["mean"]) / inp["std"]
    return inp["out_torch"]


def scipy_path(images):
    """The contract on the host, fp64: img_as_float, gaussian_filter, zoom, Normalize, .float()."""
    import numpy as np
    from scipy import ndimage as ndi
    s = SHAPE
    mean, std = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
    out = np.empty((len(images), 3, s["out_h"], s["out_w"]), np.float32)
    for i, im in enumerate(images):
        p = im / 255
        h, w = p.shape[:2]
        sig = (max(0, (h / s["out_h"] - 1) / 2), max(0, (w / s["out_w"] - 1) / 2))
        for c in range(3):
            f = ndi.gaussian_filter(p[:, :, c], sig, mode="mirror")
            r = ndi.zoom(f, (s["out_h"] / h, s["out_w"] / w), order=1, mode="mirror", grid_mode=True)
            out[i, c] = (r - mean[c]) / std[c]
    return out


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
    """The traced run: ops.preprocess alone."""
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
    rows = [r for r in csv.DictReader(open(files[0])) if "preprocess_kernel" in r["Name"]]
    kernels = [dict(name=r["Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", ""),
                    calls=int(r["Calls"]), avg_us=round(float(r["AverageNs"]) / 1e3, 2),
                    min_us=round(float(r["MinNs"]) / 1e3, 2)) for r in rows]
    return kernels, sum(k["calls"] for k in kernels) / float(calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess_bench.json"))
    ap.add_argument("--trace-dir", default=None, help="also take the rocprofv3 per-kernel time, into DIR")
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
    s = SHAPE
    inp = device_inputs()
    got, status = fused(inp)
    assert status.tolist() == [0] * s["N"]
    got = got.cpu().numpy()
    base = torch_path(inp).cpu().numpy()
    diff_torch = float(np.abs(got - base).max())

    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    host, err_scipy = None, None
    if have_scipy:
        want = scipy_path(inp["images"])
        err_scipy = float(np.abs(got.astype(np.float64) - want).max())
        assert err_scipy <= 1e-5, f"device result differs from the scipy contract by {err_scipy}"
        t_host = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(3):
                scipy_path(inp["images"])
            t_host.append((time.perf_counter() - t0) * 1e6 / 3)
        host = dict(summary(t_host), calls_per_rep=3, reps=5, scipy=scipy.__version__,
                    what="gaussian_filter + zoom per channel, fp64, one host thread")

    for _ in range(args.warmup):
        fused(inp)
        torch_path(inp)
    t_fused, t_torch = [], []
    for _ in range(args.reps):
        t_fused.append(timed(fused, inp, args.calls))
        t_torch.append(timed(torch_path, inp, args.calls))
    again = fused(inp)[0].cpu().numpy()
    assert np.array_equal(again, got), "ops.preprocess is not bit-identical from call to call"

    read_b = s["N"] * 3 * s["h"] * s["w"] + s["N"] * (8 + 8)
    write_b = s["N"] * 3 * s["out_h"] * s["out_w"] * 4 + s["N"] * 4
    kernel_us = min((k["min_us"] for k in kernels), default=None)

    def share(us, peak):
        return round((read_b + write_b) / (us * 1e-6) / (peak * 1e12), 3)

    result = dict(
        workload=dict(s, inputs="synth.image (uniform uint8), packed by data.pack_images, uploaded once outside the "
                                "timed region; caller-owned outputs"),
        device=torch.cuda.get_device_name(0), calls_per_rep=args.calls, reps=args.reps, warmup=args.warmup,
        timed="one ops.preprocess call (wrapper + one launch), device events, interleaved with the PyTorch path",
        bytes=dict(read=read_b, written=write_b, total=read_b + write_b,
                   note="every source byte once, every output element once"),
        fused=summary(t_fused),
        images_per_s_at_min=round(s["N"] / (min(t_fused) * 1e-6)),
        hbm_share_of_call=dict(of_spec_8_0_TBs=share(min(t_fused), HBM_SPEC_TBS),
                               of_measured_copy_6_29_TBs=share(min(t_fused), HBM_COPY_TBS),
                               note="bytes over the min time of a whole call, launch included; bandwidth bounds it"),
        kernels=kernels, launches_per_call=launches,
        hbm_share_of_kernel=None if kernel_us is None else dict(
            of_spec_8_0_TBs=share(kernel_us, HBM_SPEC_TBS), of_measured_copy_6_29_TBs=share(kernel_us, HBM_COPY_TBS),
            note="bytes over the kernel's min time in the rocprofv3 trace"),
        torch_baseline=dict(summary(t_torch),
                            what=".float() / 255, permute, F.interpolate(bilinear, align_corners=False), normalise, "
                                 "per image on the same device",
                            caveat="a different edge rule (clamp, not mirror) and no anti-aliasing: for time only",
                            max_abs_diff_to_fused=diff_torch),
        speedup_over_torch_min_over_min=round(min(t_torch) / min(t_fused), 2),
        speedup_over_torch_median_over_median=round(statistics.median(t_torch) / statistics.median(t_fused), 2),
        scipy_host=host, max_abs_err_to_scipy=err_scipy,
        speedup_over_scipy_min_over_min=None if host is None else round(host["min_us"] / min(t_fused), 1),
        bit_identical_across_calls=True)
    print(f"fused {result['fused']['min_us']} us min / {result['fused']['median_us']} median, torch "
          f"{result['torch_baseline']['min_us']} / {result['torch_baseline']['median_us']} us, scipy host "
          f"{host and host['min_us']} us; kernel {kernel_us} us; launches per call {launches}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))
    assert launches is None or launches <= 3, f"{launches} launches per call"


if __name__ == "__main__":
    main()
