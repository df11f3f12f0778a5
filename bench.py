"""Throughput bench of the region-proposal + RoI hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config auto|cfg1..cfg5]

One "step" = one pass of the hot path over one batch of synthetic VOC-shaped
input already resident in HBM:

    propose (decode+clamp+filter+top-k+NMS+post, anchors generated in-kernel)
    [-> RCCL all-gather of the padded detections, N > 1]
    -> RoI transform + pack + RoIPool forward (nets/heads.py:42-48, one launch)

Configs (BASELINE.json): --config auto = cfg2 (configs[1]: 8 images of
600x1000, 6000->300, RoIPool 7x7x256) per GPU at every N ("scaling": "weak";
the global batch is 8N images sharded per image, so N = 8 is configs[2]'s
64-image batch over 8 GPUs).  --config cfg3 runs those 64 images strong-scaled
over the N GPUs; cfg1 / cfg4 are the single-image configs, cfg5 the training
step (configs[4]).

Multi-GPU: one process per GPU.  Under torch.distributed.run (WORLD_SIZE set)
each process is one rank; `python bench.py --gpus N` without it starts
torch.distributed.run itself as a child process before anything touches the
GPU and exits with its code.  Images are seeded by global index, so every
rank's shard is the same data as in the 1-GPU run.

Each step's proposal layer and RoIPool run back to back on one HIP stream, and
consecutive steps alternate over --prop-streams (4) streams, so step k+1's
proposals run beside step k's RoIPool without cross-stream waits (--streams 1
serialises everything; --pool-on own puts the RoIPool on a stream of its own).
Every step does all of its work.

Prints ONE JSON line (rank 0): the metric of BASELINE.json (images/sec and
ms_per_step over the --steps timed steps).  A plain run does nothing else: it
sets up, warms up, times the steps and prints the line ("roofline" and
"cpu_baseline" are null).  --full adds, after the timed steps, "roofline" (the
dominant kernel's algorithmic HBM bytes over its HIP-event time on its launch
stream, vs the 8 TB/s peak, the kernel alone, the GPU's clock state under it),
"cpu_baseline" (the reference's CPU path on this host's cores, rank 0 at N=1
only) and, for N > 1, "strong_cfg3".

--dump-outputs DIR writes what the last timed step computed (the arrays a
caller of the step receives) as DIR/<name>.npy, float32 or float64; an array of
more than 2^20 elements is written as a fixed, seeded sample of that many.  The
inputs are seeded, so two builds run with the same arguments can be compared
file by file.
"""
from __future__ import annotations

import os

# HIP hardware queues for this process (HIP's default is 4, one of them taken by
# torch's default stream): the four step streams get a queue each instead of two
# of them sharing one (cfg2: 98.4k vs 96.2k images/s at 300 steps, 91.3k vs
# 86.9k at 20; with 4 queues and 4 streams 85.9k / 79.3k; profiles/r3_experiments.md).
# Set before HIP initialises, over an environment that pins HIP's default 4
# (FRCNN_BENCH_HW_QUEUES overrides the bench's choice).
os.environ["GPU_MAX_HW_QUEUES"] = os.environ.get("FRCNN_BENCH_HW_QUEUES", "8")
HW_QUEUES = int(os.environ["GPU_MAX_HW_QUEUES"])

import argparse
import json
import socket
import subprocess
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", default="auto",
                    help="auto (cfg2 per GPU at every N, weak scaling) | cfg1 | cfg2 | cfg3 | cfg4 | cfg5")
    ap.add_argument("--streams", type=int, default=2, choices=(1, 2),
                    help="2: the proposal layer of step k+1 runs on its own HIP stream beside "
                         "step k's RoIPool (each step still does all of its work)")
    ap.add_argument("--prep-stream", choices=["prop", "own"], default="prop",
                    help="cfg5: AnchorTarget's prepare on the proposals' stream or a fourth stream")
    ap.add_argument("--target-bufs", type=int, default=3,
                    help="cfg5: target-creator workspaces in rotation (step k's prepares reuse step k-N's)")
    ap.add_argument("--rng-waits", choices=["front", "split"], default="front",
                    help="cfg5: the draws' stream waits for both prepares before its first sampler "
                         "(front) or for each before its sampler (split)")
    ap.add_argument("--prop-streams", type=int, default=4,
                    help="with --streams 2 (inference configs): proposal layers of consecutive "
                         "steps round-robin over this many HIP streams")
    ap.add_argument("--prop-prio", type=int, default=0,
                    help="HIP stream priority of the proposal streams (negative = higher; with "
                         "--pool-on split the RoIPool streams keep the default)")
    ap.add_argument("--pool-on", default="prop", choices=("prop", "own", "split"),
                    help="with --streams 2 (inference): prop = each step's RoIPool runs on that step's "
                         "proposal stream right after its proposals (consecutive steps on different "
                         "streams overlap; no cross-stream waits), own = the RoIPool on a stream of "
                         "its own, fed by events, split = each proposal stream's RoIPool on a "
                         "companion stream of its own (events)")
    ap.add_argument("--prop-cus", type=int, default=0,
                    help="with --streams 2: CUs reserved for the proposal streams (spread over the "
                         "XCDs); the RoIPool stream gets the rest.  0 = no reservation")
    ap.add_argument("--mask-pool", type=int, default=1, choices=(0, 1),
                    help="with --prop-cus: 1 = the RoIPool stream is masked to the other CUs")
    ap.add_argument("--propose-path", default="auto",
                    help="frcnn_set_path propose: auto | hybrid | lazy | wide")
    ap.add_argument("--cu-order", default="rr", choices=("rr", "blk"),
                    help="how the CU-mask numbering maps to XCDs (tools/cu_probe.py)")
    ap.add_argument("--host-io", type=int, default=0, choices=(0, 1),
                    help="1: PCIe-inclusive variant -- each step copies its inputs (scores, "
                         "deltas, features) from pinned host memory and the rois + pooled "
                         "features back, like the reference's host-resident tensors (never the "
                         "default value)")
    ap.add_argument("--dist-backend", default="auto", choices=("auto", "nccl", "gloo"),
                    help="auto: nccl (RCCL over xGMI) when every rank has a GPU of its own, "
                         "gloo (host copies) when ranks share one")
    ap.add_argument("--roi-store", default="auto", choices=("auto", "temporal", "nt"),
                    help="RoIPool forward output stores (frcnn_set_path roi_pool_fwd_store): nt = non-temporal")
    ap.add_argument("--roi-cg", default="auto",
                    help="channels per RoIPool forward workgroup (frcnn_set_path roi_pool_cg): auto | 4 | 8 | 16")
    ap.add_argument("--roi-path", default="auto",
                    help="RoIPool forward kernel (frcnn_set_path roi_pool_fwd): auto | wave | dense | generic")
    ap.add_argument("--roi-split", default="auto",
                    help="RoI shares per (image, channel group) of the RoIPool forward "
                         "(frcnn_set_path roi_pool_split): auto | 1 | 2 | ...")
    ap.add_argument("--input-sets", type=int, default=0,
                    help="distinct input sets the steps cycle through (0 = enough for > 320 MiB, "
                         "i.e. more than the Infinity Cache; 1 = the same inputs every step)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure the roofline record (the dominant kernel "
                         "alone, the GPU's clock state), the CPU baseline and, for N > 1, strong_cfg3")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy (float32 / float64; "
                         "arrays of more than 2^20 elements as a fixed, seeded sample)")
    ap.add_argument("--cpu-seconds", type=float, default=10.0,
                    help="with --full: bounded CPU-baseline sample (rank 0, N=1 only); 0 disables")
    ap.add_argument("--cpu-images", type=int, default=10, help="minimum timed CPU images (median)")
    return ap.parse_args()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def maybe_launch(args) -> None:
    """`--gpus N` without torch.distributed.run: start it as a child process
    (nothing has touched the GPU yet) and exit with its code."""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={args.gpus}", "--master-addr=127.0.0.1",
           f"--master-port={_free_port()}", os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    raise SystemExit(subprocess.call(cmd, env=env))


def setup_dist(args):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    ndev = torch.cuda.device_count()
    dev_index = local % max(ndev, 1)
    torch.cuda.set_device(dev_index)
    backend = None
    if world > 1:
        # stdout carries only rank 0's JSON line: the process group's C++ log
        # lines (gloo / RCCL) go to stderr, and so does everything of ranks > 0
        saved = os.dup(1)
        os.dup2(2, 1)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        shared = world > ndev  # more ranks than GPUs on this node: ranks share devices
        backend = args.dist_backend if args.dist_backend != "auto" else ("gloo" if shared else "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group("gloo")
        if rank == 0:
            os.dup2(saved, 1)
        os.close(saved)
    return world, rank, dev_index, backend, ndev


def resolve_config(args, world):
    """--config auto = cfg2 (configs[1]: 8 images per GPU) at EVERY N: the 1/2/4/8-GPU
    curve is one workload weak-scaled, 8 images per rank, so N = 8 runs the 64-image
    global batch of configs[2] (cfg3) sharded per image and N = 1 is the headline
    line.  --config cfg3 keeps the strong-scaled 64-image batch."""
    if args.config != "auto":
        return args.config
    return "cfg2"


def workload_name(cfg, c, N, n_total, world, C, train):
    """The record's config.workload: names the per-GPU workload the same way at every N."""
    K = 3 * len(c["scales"])
    if train:
        return (f"{cfg}: training step, {N} images/GPU {c['img_h']}x{c['img_w']}, "
                f"{c['feat_h']}x{c['feat_w']}x{K} anchors, {c['pre_nms']}->{c['post_nms']} NMS@0.7, "
                f"anchor targets vs 32 gt + proposal targets (128/img), RoIPool 7x7x{C} fwd+bwd")
    shard_txt = (f"{n_total} images sharded per image over {world} ranks" if cfg == "cfg3"
                 else f"{c['batch']} images/GPU")
    return (f"{cfg}: {shard_txt}, VOC shape {c['img_h']}x{c['img_w']}, "
            f"{c['feat_h']}x{c['feat_w']}x{K} anchors, {c['pre_nms']}->{c['post_nms']} NMS@0.7, "
            f"RoIPool 7x7x{C}")


def make_inputs(cfg, images, device, seed=0):
    from replication_faster_rcnn_amd import synth
    c = synth.CONFIGS[cfg]
    K = 3 * len(c["scales"])
    A = c["feat_h"] * c["feat_w"] * K
    sc = torch.from_numpy(np.stack([synth.rpn_scores(A, seed, i) for i in images])).to(device)
    de = torch.from_numpy(np.stack([synth.rpn_deltas(A, seed, i) for i in images])).to(device)
    x = torch.from_numpy(np.stack([synth.features(c["C"], c["feat_h"], c["feat_w"], seed, i)
                                   for i in images])).to(device)
    return c, sc, de, x


INPUT_SPAN = 320 << 20  # bytes of distinct inputs the timed steps cycle through (> 256 MiB MALL)


def make_input_sets(cfg, images, device, n_sets):
    """Input sets the steps cycle through (set s seeded by s, image by its global
    index): with more distinct bytes than the 256 MiB Infinity Cache, every
    step reads its scores / deltas / features from HBM, not from a cache the
    previous identical step left warm."""
    c, sc, de, x = make_inputs(cfg, images, device, 0)
    per = sum(t.numel() * t.element_size() for t in (sc, de, x))
    if n_sets <= 0:
        n_sets = int(min(64, max(2, -(-INPUT_SPAN // per))))
    sets = [(sc, de, x)] + [make_inputs(cfg, images, device, s)[1:] for s in range(1, n_sets)]
    return c, sets, per


# ------------------------------------------------------------- GPU clock state
class GpuState:
    """The GPU's clock / power state (amdsmi, else sysfs), so that a slow box can be
    told apart from a regression: current / min / max GFX and memory clocks, the
    power cap and draw, and the firmware's recent averages and throttle flags.
    open() finds the device (before the sampled work is queued), sample() reads it
    (while the work runs).  Never raises: failures land in the record as "error"."""

    def __init__(self, dev_index):
        self.h = self.smi = self.dpath = None
        self.err = None
        try:
            p = torch.cuda.get_device_properties(dev_index)
            self.want = "%04x:%02x:%02x" % (getattr(p, "pci_domain_id", 0), p.pci_bus_id, p.pci_device_id)
        except Exception:  # noqa: BLE001
            self.want = None
        try:
            import amdsmi
            amdsmi.amdsmi_init(amdsmi.AmdSmiInitFlags.INIT_AMD_GPUS)
            self.smi = amdsmi
            hs = amdsmi.amdsmi_get_processor_handles()
            for cand in hs:
                if self.want and str(amdsmi.amdsmi_get_gpu_device_bdf(cand)).lower().startswith(self.want):
                    self.h = cand
            if self.h is None and len(hs) == 1:
                self.h = hs[0]
            if self.h is None:
                self.err = f"amdsmi: no handle for {self.want} ({len(hs)} GPUs)"
        except Exception as e:  # noqa: BLE001
            self.err = f"amdsmi: {str(e)[:120]}"
        if self.h is None:
            import glob
            for d in glob.glob("/sys/class/drm/card*/device"):
                if self.want and os.path.basename(os.path.realpath(d)).lower().startswith(self.want):
                    self.dpath = d

    def sample(self):
        if self.h is not None:
            smi, h = self.smi, self.h
            out = {"source": "amdsmi", "bdf": str(smi.amdsmi_get_gpu_device_bdf(h))}

            def get(key, fn, keep=None):
                try:
                    d = fn()
                    out[key] = {k: (v[:8] if isinstance(v, list) else v) for k, v in d.items()
                                if keep is None or k in keep}
                except Exception as e:  # noqa: BLE001
                    out[key] = {"error": str(e)[:80]}
            get("gfx_clk_mhz", lambda: smi.amdsmi_get_clock_info(h, smi.AmdSmiClkType.GFX),
                ("clk", "min_clk", "max_clk", "clk_locked"))
            get("mem_clk_mhz", lambda: smi.amdsmi_get_clock_info(h, smi.AmdSmiClkType.MEM),
                ("clk", "min_clk", "max_clk", "clk_locked"))
            get("power_w", lambda: smi.amdsmi_get_power_info(h),
                ("current_socket_power", "average_socket_power", "power_limit"))
            get("power_cap_uw", lambda: smi.amdsmi_get_power_cap_info(h),
                ("power_cap", "default_power_cap", "min_power_cap", "max_power_cap"))
            get("metrics", lambda: smi.amdsmi_get_gpu_metrics_info(h),
                ("average_gfxclk_frequency", "current_gfxclk", "current_gfxclks", "current_uclk",
                 "average_socket_power", "current_socket_power", "temperature_hotspot", "temperature_mem",
                 "throttle_status", "indep_throttle_status", "gfxclk_lock_status", "average_gfx_activity",
                 "average_umc_activity"))
            return out
        if self.dpath:
            import glob
            out = {"source": "sysfs", "bdf": os.path.basename(os.path.realpath(self.dpath)), "amdsmi": self.err}
            for f in ("pp_dpm_sclk", "pp_dpm_mclk"):
                try:
                    out[f] = open(os.path.join(self.dpath, f)).read().strip().split("\n")[:16]
                except OSError:
                    pass
            for f in glob.glob(os.path.join(self.dpath, "hwmon", "hwmon*", "power1_*")):
                try:
                    out[os.path.basename(f)] = open(f).read().strip()
                except OSError:
                    pass
            return out
        return {"error": self.err or "no device found"}

    def close(self):
        if self.smi is not None:
            try:
                self.smi.amdsmi_shut_down()
            except Exception:  # noqa: BLE001
                pass


# ------------------------------------------------------------- CPU baseline
def _host_info():
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    try:
        isa = torch.backends.cpu.get_cpu_capability()
    except Exception:  # older torch
        isa = "unknown"
    return model, isa


def _cgroup_cpus():
    """CPUs this process may actually use per the cgroup CPU quota (v2 cpu.max
    or v1 cfs_quota/period), None when unlimited / unreadable.  The GPU box
    shows the whole machine in the affinity mask (256 CPUs) but grants a share
    of it; torch on 256 threads over a 16-CPU share spins ~25x slower."""
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            return max(1, int(-(-int(q) // int(p))))
    except (OSError, ValueError):
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        if q > 0:
            return max(1, -(-q // p))
    except (OSError, ValueError):
        pass
    return None


def cpu_threads():
    """(threads used, affinity count, cgroup quota, OMP_NUM_THREADS)."""
    aff = len(os.sched_getaffinity(0))
    cg = _cgroup_cpus()
    omp = os.environ.get("OMP_NUM_THREADS")
    omp = int(omp) if omp and omp.isdigit() and int(omp) > 0 else None
    use = min(x for x in (aff, cg, omp) if x)
    return use, aff, cg, omp


def cpu_baseline(cfg, seconds, min_images, train=False):
    """The reference's CPU path per image (nets/rpn.py:58-77 in torch CPU ops,
    nets/heads.py:42-48; for cfg5 also the numpy target creators of
    utils/utils.py:122-276 and the RoIPool backward), torch given every CPU
    this process may use (affinity, capped by the cgroup quota and
    OMP_NUM_THREADS -- the GPU box's affinity mask lists the whole machine);
    torchvision's nms / roi_pool are the oracle's C restatement of their
    (single-threaded) CPU kernels.  The thread count is the faster of that and
    1 thread on 3 probe images (small torch ops can lose to threading).
    >= 3 warm-up images, then the median over >= `min_images` images (more
    while `seconds` last)."""
    from oracle import ref_numpy as orc
    from oracle import ref_torch as ort
    from replication_faster_rcnn_amd import synth
    cores, aff, cg, omp = cpu_threads()
    c = synth.CONFIGS[cfg]
    base = orc.generate_anchor_base(anchor_scales=c["scales"])
    anchors = orc.generate_anchors(base, 16, c["feat_w"], c["feat_h"])
    A = len(anchors)
    g = np.random.default_rng(1).standard_normal((128, c["C"], 7, 7), dtype=np.float32)
    np.random.seed(0)

    def one(i):
        sc = torch.from_numpy(synth.rpn_scores(A, 0, i))
        de = torch.from_numpy(synth.rpn_deltas(A, 0, i))
        x = torch.from_numpy(synth.features(c["C"], c["feat_h"], c["feat_w"], 0, i)[None])
        if train:
            bx, lb = synth.gt_boxes(c["img_h"], c["img_w"], 32, 0, i)
            v = lb != -1
        ts = time.perf_counter()
        roi = ort.region_proposal(anchors, sc, de, c["img_w"], c["img_h"], c["pre_nms"], c["post_nms"])
        if train:  # train.py:71-108 for one image
            orc.anchor_target(bx[v], anchors)
            s_roi = orc.proposal_target(roi.numpy(), bx[v], lb[v])[0]
            roi = torch.from_numpy(s_roi.astype(np.float32))
        out, am, boxes = ort.head_roi_pool(x, roi, torch.zeros(len(roi)), c["img_h"], c["img_w"])
        if train:
            orc.roi_pool_backward(g[:len(roi)], boxes.numpy(), am.numpy(), tuple(x.shape))
        return time.perf_counter() - ts

    probe = {}
    for th in sorted({cores, 1}, reverse=True):  # 1 warm-up + 2 timed images each
        torch.set_num_threads(th)
        probe[th] = min(one(k) for k in range(3))
    threads = min(probe, key=probe.get)
    torch.set_num_threads(threads)
    times, t_all, i = [], time.perf_counter(), 3
    warm = 3
    while True:
        dt = one(i)
        i += 1
        if warm:
            warm -= 1
            continue
        times.append(dt)
        te = time.perf_counter()
        if len(times) >= min_images and te - t_all >= seconds:
            break
        if len(times) >= 10 * min_images and te - t_all >= 3:
            break
    med = float(np.median(times))
    model, isa = _host_info()
    what = "training step (proposals, anchor + proposal targets, RoIPool fwd+bwd)" if train else \
        "proposal layer + head RoIPool"
    return {"value": 1.0 / med, "unit": "images/sec", "cores": threads, "kind": "port",
            "sample": f"{cfg} {what}, one image at a time like nets/rpn.py:131: median of "
                      f"{len(times)} images after 3 warm-ups ({sum(times):.1f} s timed); torch CPU ops "
                      f"of the reference on {threads} threads, torchvision nms/roi_pool as the oracle's "
                      f"single-threaded C restatement",
            "cpu_model": model, "cpu_isa": isa, "torch_threads": torch.get_num_threads(),
            "affinity_cpus": aff, "cgroup_cpus": cg, "omp_num_threads": omp,
            "probe_ms_per_image": {str(k): v * 1e3 for k, v in probe.items()},
            "median_ms_per_image": med * 1e3}


# ------------------------------------------------------------------ steps
class _On:
    """`with _On(s):` -- torch.cuda.stream(s) without its per-entry Stream
    objects (~6 us per use on the issue path): switches torch's current stream
    to `s` and back to `home` (the stream current when the steps were built)."""

    __slots__ = ("ids", "home")

    def __init__(self, s, home):
        self.ids = (s.stream_id, s.device_index, s.device_type)
        self.home = (home.stream_id, home.device_index, home.device_type)

    def __enter__(self):
        i, d, t = self.ids
        torch._C._cuda_setStream(stream_id=i, device_index=d, device_type=t)

    def __exit__(self, *exc):
        i, d, t = self.home
        torch._C._cuda_setStream(stream_id=i, device_index=d, device_type=t)
        return False


def reserved_cus(n, k, order):
    """k CUs spread evenly over the 8 XCDs (hipExtStreamCreateWithCUMask
    numbering; `order` = how that numbering maps to XCDs: "rr" = CU i on XCD
    i % 8, "blk" = CUs 32x..32x+31 on XCD x -- tools/cu_probe.py)."""
    per = max(1, k // 8)
    xcd = [[i for i in range(n) if i % 8 == x] if order == "rr" else
           [i for i in range(n) if i // (n // 8) == x] for x in range(8)]
    return sorted(c for lst in xcd for c in lst[-per:])


def make_streams(args):
    """(list of proposal streams, RoIPool stream).  With --prop-cus K the
    proposal streams run on K reserved CUs (K/8 per XCD) and the RoIPool on the
    rest: the pool's one-workgroup-per-CU tiles hold every CU's LDS for its
    whole run, so without a reservation the next step's proposal kernels wait
    for it; the pool sizes its grid to its stream's CUs."""
    if args.streams == 1:
        s = torch.cuda.current_stream()
        return [s], s
    nps = max(1, args.prop_streams)
    if args.pool_on == "split":  # a RoIPool stream per proposal stream
        props = [torch.cuda.Stream(priority=args.prop_prio) for _ in range(nps)]
        return props, [torch.cuda.Stream() for _ in range(nps)]
    if args.prop_cus > 0:
        from replication_faster_rcnn_amd import _lib
        n = _lib.cu_count()
        res = reserved_cus(n, args.prop_cus, args.cu_order)
        rest = [i for i in range(n) if i not in set(res)]
        pool = _lib.cu_stream(rest) if args.mask_pool else torch.cuda.Stream()
        return [_lib.cu_stream(res) for _ in range(nps)], pool
    return [torch.cuda.Stream(priority=args.prop_prio) for _ in range(nps)], torch.cuda.Stream()


def inference_step_fn(args, c, sets, base, world, n_total, backend, ev):
    """cfg1-4: propose -> (all-gather of detections) -> RoI transform + pack +
    RoIPool forward (nets/rpn.py:102-138, nets/heads.py:42-48).  Every buffer
    and event is allocated once, outside the timed steps: proposal outputs per
    proposal stream (reused once the pool that read them has finished), one set
    of pooled outputs on the pool stream."""
    from replication_faster_rcnn_amd import ops
    sc, de, x = sets[0]
    N, dev = sc.size(0), sc.device
    post = c["post_nms"]
    C = x.size(1)
    inds = torch.arange(N, device=dev, dtype=torch.float32).repeat_interleave(post)
    s_props, s_pool = make_streams(args)
    nps = len(s_props)
    home = torch.cuda.current_stream()
    on_prop = [_On(sp, home) for sp in s_props]
    split = isinstance(s_pool, list)  # --pool-on split: one RoIPool stream per proposal stream
    s_pools = s_pool if split else [s_pool] * nps
    on_pools = [_On(sp, home) for sp in s_pools]
    gathers = None
    if world > 1:  # proposals written straight into each stream's preallocated send buffer
        from replication_faster_rcnn_amd import dist as fdist
        gathers = [fdist.DetectionGather(n_total, post, dev, backend) for _ in range(nps)]
        prop_out = [g.outputs() for g in gathers]
        s_comm = torch.cuda.Stream()
        on_comm = _On(s_comm, home)
        prop_done = [torch.cuda.Event() for _ in range(nps)]
        gather_done = [torch.cuda.Event() for _ in range(nps)]
        gather_pending = [False] * nps
    else:
        prop_out = [(torch.empty((N, post, 4), dtype=torch.float32, device=dev),
                     torch.empty((N, post), dtype=torch.int32, device=dev),
                     torch.empty((N,), dtype=torch.int32, device=dev)) for _ in range(nps)]
    pool_on_prop = args.pool_on == "prop" and args.streams == 2 and not args.host_io and args.prop_cus == 0
    pool_outs = [(torch.empty((N * post, C, 7, 7), dtype=torch.float32, device=dev),
                  torch.empty((N * post, C, 7, 7), dtype=torch.int32, device=dev),
                  torch.empty((N * post, 5), dtype=torch.float32, device=dev))
                 for _ in range(nps if (pool_on_prop or split) else 1)]
    pool_out = pool_outs[0]
    ready = [torch.cuda.Event() for _ in range(nps)]
    done = [None] * nps          # the pool that last read prop_out[j]
    done_ev = [torch.cuda.Event() for _ in range(nps)]
    k_step = [0]
    if args.host_io:  # reference-style host tensors: inputs H2D, rois + pooled D2H per step
        h_in = [t.cpu().pin_memory() for t in (sc, de, x)]
        d_in = [[torch.empty_like(t) for t in (sc, de, x)] for _ in s_props]
        h_rois = torch.empty((N, post, 4), dtype=torch.float32).pin_memory()
        h_pool = torch.empty((N * post, C, 7, 7), dtype=torch.float32).pin_memory()
    gathered = {}

    def gather_after(j):
        """The step's one collective, off its critical path: on a side stream
        that waits only for the step's proposals (the RoIPool on the proposal
        stream does not wait for it); the proposal stream waits for it before
        it rewrites the send buffer (nps steps later)."""
        prop_done[j].record(s_props[j])
        with on_comm:
            s_comm.wait_event(prop_done[j])
            gathered["last"] = (gathers[j], gathers[j].gather())
            gather_done[j].record(s_comm)
        gather_pending[j] = True

    def step(timed):
        j = k_step[0] % nps
        s_prop = s_props[j]
        sc, de, x = sets[k_step[0] % len(sets)]
        k_step[0] += 1
        rois, idx, cnt = prop_out[j]
        if pool_on_prop:  # the step's proposals and RoIPool back to back on its stream
            with on_prop[j]:
                if world > 1 and gather_pending[j]:
                    s_prop.wait_event(gather_done[j])  # the gather that read this send buffer
                ops.propose(sc, de, img_w=c["img_w"], img_h=c["img_h"], pre_nms=c["pre_nms"],
                            post_nms=post, anchor_base=base, feat_h=c["feat_h"], feat_w=c["feat_w"],
                            out=prop_out[j])
            if world > 1:  # the only collective: detections of all ranks, issued behind the
                gather_after(j)  # proposals (prop_done is recorded before the pool is queued)
            with on_prop[j]:
                if timed:
                    e0, e1 = ev["pairs"][ev["i"]]
                    ev["i"] += 1
                    e0.record(s_prop)
                ops.roi_pool_head(x, rois.view(-1, 4), inds, 7, c["img_h"], c["img_w"],
                                  rois_sorted=True, out=pool_outs[j])
                if timed:
                    e1.record(s_prop)
                    ev["fwd"].append((e0, e1))
            return cnt
        with on_prop[j]:
            if done[j] is not None:
                s_prop.wait_event(done[j])  # the pool that read prop_out[j] (and d_in[j]) last time
            if world > 1 and gather_pending[j]:
                s_prop.wait_event(gather_done[j])
            sc_, de_, x_ = sc, de, x
            if args.host_io:
                for d, h in zip(d_in[j], h_in):
                    d.copy_(h, non_blocking=True)
                sc_, de_, x_ = d_in[j]
            ops.propose(sc_, de_, img_w=c["img_w"], img_h=c["img_h"], pre_nms=c["pre_nms"],
                        post_nms=post, anchor_base=base, feat_h=c["feat_h"], feat_w=c["feat_w"],
                        out=prop_out[j])
            if args.host_io:
                h_rois.copy_(rois, non_blocking=True)
            ready[j].record(s_prop)
        s_pool, pool_out = s_pools[j], pool_outs[j if split else 0]
        with on_pools[j]:
            s_pool.wait_event(ready[j])
            if timed:
                e0, e1 = ev["pairs"][ev["i"]]
                ev["i"] += 1
                e0.record(s_pool)
            # ResnetHead's transform + pack + roi_pool (nets/heads.py:42-48): one launch
            ops.roi_pool_head(x_, rois.view(-1, 4), inds, 7, c["img_h"], c["img_w"],
                              rois_sorted=True, out=pool_out)
            if timed:
                e1.record(s_pool)
                ev["fwd"].append((e0, e1))
            if args.host_io:
                h_pool.copy_(pool_out[0], non_blocking=True)
            done_ev[j].record(s_pool)
            done[j] = done_ev[j]
        if world > 1:  # the only collective: detections of all ranks
            gather_after(j)
        return cnt
    step.gathered = gathered
    step.prop_out, step.pool_outs = prop_out, pool_outs  # (parity test: the per-stream buffers)

    def last_outputs():  # the buffers the last step wrote (--dump-outputs)
        j = (k_step[0] - 1) % nps
        rois, idx, cnt = prop_out[j]
        pooled, argmax, boxes = pool_outs[j if len(pool_outs) > 1 else 0]
        return {"rois": rois, "anchor_idx": idx, "count": cnt, "boxes": boxes, "pooled": pooled,
                "argmax": argmax}
    step.last_outputs = last_outputs

    def alone():  # the dominant kernel by itself (after the timed steps): the last proposals
        ops.roi_pool_head(sets[0][2], prop_out[0][0].view(-1, 4), inds, 7, c["img_h"], c["img_w"],
                          rois_sorted=True, out=pool_outs[0])
    step.alone = alone
    from replication_faster_rcnn_amd import _lib
    step.kernel = _lib.roi_pool_fwd_kernel(N * post, N, C, x.size(2), x.size(3),
                                           stream=s_props[0] if pool_on_prop else s_pools[0])
    return step


def train_step_fn(args, c, sets, base, first_image, ev):
    """cfg5 (training step, train.py:59-127 minus the dense layers): propose
    (12000->600) -> anchor targets of every image -> proposal targets of every
    image (numpy's MT19937 stream kept on the device, sync-free, in the
    reference's order: all AT, then all PT) -> sampled RoIs fp64->fp32 ->
    RoI transform + pack + RoIPool forward -> RoIPool backward of a resident
    upstream gradient (the head's dL/dpool).

    With --streams 2 the step runs on three HIP streams (HIP multiplexes streams
    onto 4 hardware queues, one of them torch's default stream, so a fourth
    stream would share a queue): the target creators' draws (the device RNG
    stream: AT(k), PT(k), AT(k+1), ... in the reference's order) on one;
    AnchorTargetCreator's RNG-free half (IoU, labels, candidate lists) and then
    the proposal layer on another -- AT(k) needs only the gt boxes and the
    anchors, so its draws start before step k's proposals are done -- and the
    RoIPool forward + backward of step k on a third, beside AT(k+1)."""
    from replication_faster_rcnn_amd import anchors as A, ops, synth, targets
    from replication_faster_rcnn_amd.utils import rng_state_to_device
    sc, de, x = sets[0]
    N, dev = sc.size(0), sc.device
    S = 128
    anchors = A.generate_anchors(base, 16, c["feat_w"], c["feat_h"]).to(dev)
    gl = [synth.gt_boxes(c["img_h"], c["img_w"], 32, 0, first_image + i) for i in range(N)]
    boxes = torch.from_numpy(np.stack([b for b, _ in gl])).to(dev)
    labels = torch.from_numpy(np.stack([l for _, l in gl])).to(dev)
    np.random.seed(0)
    rng, _ = rng_state_to_device(dev)
    inds = torch.arange(N, device=dev, dtype=torch.float32).repeat_interleave(S)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    grad = torch.randn((N * S, x.size(1), 7, 7), device=dev, generator=gen)
    if args.streams == 1:
        s_prop = s_rng = s_pool = torch.cuda.current_stream()
    else:  # three streams: HIP maps streams onto 4 hardware queues (one is torch's default)
        s_prop, s_rng, s_pool = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    # AnchorTargetCreator's prepare on the proposals' stream (default) or its own: HIP maps
    # streams onto 4 hardware queues, so a fourth stream shares one with another stream
    s_prep = torch.cuda.Stream() if (args.streams != 1 and getattr(args, "prep_stream", "prop") == "own") else s_prop
    state = {}
    # AnchorTargetCreator's RNG-free half (IoU, labels, candidate lists) of step
    # k runs on the proposal stream, ahead of step k's proposals and beside step
    # k-1's draws; --target-bufs workspaces rotate
    A_ = anchors.size(0)
    nb = getattr(args, "target_bufs", 3)  # step k's prepares wait for step k - nb's draws and finishes
    at_ws = [targets.anchor_targets_workspace(N, A_, boxes.size(1), dev) for _ in range(nb)]
    at_out = [(torch.empty((N, A_, 4), dtype=torch.float64, device=dev),
               torch.empty((N, A_), dtype=torch.int32, device=dev)) for _ in range(nb)]
    prep_ready = [torch.cuda.Event() for _ in range(nb)]
    sample_done = [None] * nb
    sample_ev = [torch.cuda.Event() for _ in range(nb)]
    # ProposalTargetCreator's RNG-free half (IoU, fg / bg lists) follows the
    # proposals on their stream; the draws' stream only runs the draws
    pt_ws = [targets.proposal_targets_workspace(N, c["post_nms"], boxes.size(1), S, dev) for _ in range(nb)]
    pt_out = [(torch.empty((N, S, 4), dtype=torch.float64, device=dev),
               torch.empty((N, S, 4), dtype=torch.float64, device=dev),
               torch.empty((N, S), dtype=torch.float64, device=dev),
               torch.empty((N,), dtype=torch.int32, device=dev)) for _ in range(nb)]
    pt_done = [None] * nb
    pt_ev = [torch.cuda.Event() for _ in range(nb)]
    k_step = [0]

    def step(timed):
        j = k_step[0] % nb
        sc, de, x = sets[k_step[0] % len(sets)]
        k_step[0] += 1
        with torch.cuda.stream(s_prep):
            if sample_done[j] is not None:
                s_prep.wait_event(sample_done[j])  # the draws that read at_ws[j] last time
            plan = targets.anchor_targets_prepare(boxes, labels, anchors, workspace=at_ws[j])
            prep_ready[j].record(s_prep)
        with torch.cuda.stream(s_prop):
            rois, _, cnt = ops.propose(sc, de, img_w=c["img_w"], img_h=c["img_h"],
                                       pre_nms=c["pre_nms"], post_nms=c["post_nms"],
                                       anchor_base=base, feat_h=c["feat_h"], feat_w=c["feat_w"])
            if pt_done[j] is not None:
                s_prop.wait_event(pt_done[j])  # the draws that read pt_ws[j] last time
            pplan = targets.proposal_targets_prepare(rois, cnt, boxes, labels, n_sample=S, workspace=pt_ws[j])
            prop_ready = torch.cuda.Event()
            prop_ready.record(s_prop)
        # the draws' stream runs only the draws (the sequential MT19937 stream);
        # the finishing kernels go with the pool, which needs their output
        with torch.cuda.stream(s_rng):
            # every event record / wait on this stream is a packet the hardware queue
            # retires between two samplers (~4-6 us each, profiles/r4_experiments.md):
            # one wait (prop_ready follows prep_ready on the same stream) and one
            # timing record per step
            if args.rng_waits == "front":  # both creators' draws as one pass (the prepares run ahead)
                s_rng.wait_event(prop_ready)
                s_cnt = targets.target_draws(plan, pplan, rng, count=pt_out[j][3])
            else:
                s_rng.wait_event(prep_ready[j])
                targets.anchor_targets_draw(plan, rng=rng)
                s_rng.wait_event(prop_ready)
                s_cnt = targets.proposal_targets_draw(pplan, rng=rng, count=pt_out[j][3])
            pt_drawn = torch.cuda.Event(enable_timing=timed)
            pt_drawn.record(s_rng)
            if timed:
                ev["draw"].append(pt_drawn)
        with torch.cuda.stream(s_pool):
            # the AnchorTarget finish waits for both draws (one event on the draws'
            # stream): it only has to precede the pool, which needs the second anyway
            s_pool.wait_event(pt_drawn)
            reg_t, lab = targets.anchor_targets_finish(plan, out=at_out[j])
            sample_ev[j].record(s_pool)
            sample_done[j] = sample_ev[j]   # at_ws[j] free for step k+nb's prepare
            s_roi, s_reg, s_lab = targets.proposal_targets_finish(pplan, s_cnt, out=pt_out[j][:3])
            sample_rois = s_roi.float().view(-1, 4)          # train.py:86,102,107
            pt_ev[j].record(s_pool)
            pt_done[j] = pt_ev[j]           # pt_ws[j], pt_out[j] free for step k+nb
            if timed:
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record(s_pool)
            pooled, am, bx = ops.roi_pool_head(x, sample_rois, inds, 7, c["img_h"], c["img_w"],
                                               rois_sorted=True)
            if timed:
                e[1].record(s_pool)
            gi = ops._roi_pool_bwd(grad, bx, am, tuple(x.shape), 1.0)
            if timed:
                e[2].record(s_pool)
                ev["fwd"].append((e[0], e[1]))
                ev["bwd"].append((e[1], e[2]))
        state.update(s_cnt=s_cnt, lab=lab, reg_t=reg_t, s_roi=s_roi, s_reg=s_reg, s_lab=s_lab, pooled=pooled,
                     gi=gi, am=am, bx=bx, xshape=tuple(x.shape))
        return s_cnt
    step.state = state
    step.fixed = dict(rng=rng, grad=grad, boxes=boxes, labels=labels, anchors=anchors)

    def last_outputs():  # what the last step returned to its caller (--dump-outputs)
        names = {"lab": "anchor_labels", "reg_t": "anchor_reg_targets", "s_roi": "sample_rois",
                 "s_reg": "sample_reg_targets", "s_lab": "sample_labels", "s_cnt": "sample_count",
                 "bx": "boxes", "pooled": "pooled", "am": "argmax", "gi": "grad_features"}
        return {name: state[k] for k, name in names.items()}
    step.last_outputs = last_outputs

    def alone():  # the RoIPool backward by itself, on the last step's inputs
        ops._roi_pool_bwd(grad, state["bx"], state["am"], state["xshape"], 1.0)
    step.alone = alone
    from replication_faster_rcnn_amd import _lib
    step.kernel = _lib.roi_pool_bwd_kernel(N * S, N, x.size(1), x.size(2), x.size(3))
    return step


def strong_cfg3(args, world, rank, dev, backend, base_of):
    """BASELINE configs[2] as written: the 64-image batch sharded per image over the
    N ranks (strong scaling), timed like the headline (barrier + sync on both sides,
    max over ranks).  Reported beside the weak-scaled cfg2 line for N > 1."""
    from replication_faster_rcnn_amd import dist as fdist
    from replication_faster_rcnn_amd import synth
    n_total = synth.CONFIGS["cfg3"]["batch"]
    mine = fdist.shard(n_total, rank, world)
    c, sets, _ = make_input_sets("cfg3", mine, dev, min(args.input_sets or 4, 4))
    base = base_of.generate_anchor_base_device(anchor_scales=c["scales"])
    ev = {"fwd": [], "bwd": [], "draw": [], "i": 0,
          "pairs": [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                    for _ in range(args.steps)]}
    step = inference_step_fn(args, c, sets, base, world, n_total, backend, ev)
    for _ in range(args.warmup):
        step(False)
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step(True)
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    t = torch.tensor([el], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    el = float(t.item())
    return {"workload": f"cfg3: {n_total} images sharded per image over {world} ranks (BASELINE configs[2])",
            "value": n_total * args.steps / el, "unit": "images/sec", "ms_per_step": el / args.steps * 1e3,
            "scaling": "strong", "global_batch": n_total, "images_per_gpu_max": len(mine)}


DUMP_ELEMS = 1 << 20     # elements written per array: larger ones as a fixed, seeded sample
DUMP_LIMIT = 64 << 20    # bytes written per run, all arrays together


def dump_outputs(outs, path, rank):
    """--dump-outputs: DIR/<name>.npy per output of the last timed step (ranks > 0:
    <name>.rank<r>.npy), float64 as it is, everything else as float32 (the integer
    outputs -- anchor indices, argmax, counts, labels -- are far below 2^24).  An array
    of more than DUMP_ELEMS elements is written as its elements at DUMP_ELEMS sorted
    flat indices drawn from a generator seeded with 0 (a function of its size alone)."""
    os.makedirs(path, exist_ok=True)
    total = 0
    for name, t in outs.items():
        t = t.detach()
        if t.numel() > DUMP_ELEMS:
            pick = np.sort(np.random.default_rng(0).integers(0, t.numel(), DUMP_ELEMS))
            t = t.reshape(-1)[torch.from_numpy(pick).to(t.device)]
        a = t.cpu().numpy()
        a = a if a.dtype == np.float64 else a.astype(np.float32)
        total += a.nbytes
        if total > DUMP_LIMIT:
            raise RuntimeError(f"--dump-outputs: more than {DUMP_LIMIT >> 20} MiB of outputs")
        np.save(os.path.join(path, name + (f".rank{rank}" if rank else "") + ".npy"), a)


def roofline_record(step, ev, train, cfg, rank, dev_index, alg_bytes, ms_step):
    """--full: the dominant kernel's roofline record.  Its per-launch event intervals
    come from the timed steps; the kernel alone and the GPU's clock state under it are
    measured here, after them."""
    # the dominant kernel (RoIPool fwd for inference, bwd for the training
    # step: same algorithmic bytes -- features / grad_in once, rois, out +
    # argmax / grad + argmax) runs once per step and each step moves its
    # algorithmic bytes once, so the chip-level rate it sustains inside the
    # pipeline is bytes per step / time per step (can only under-state the
    # kernel: the step also holds the proposal chain)
    achieved = alg_bytes / (ms_step * 1e-3) / 1e9
    # per-launch HIP-event interval on the launch stream, for reference: the
    # steps overlap on several streams, so this interval is shared with the
    # neighbouring steps' kernels and is NOT a roofline time
    ev_ms = float(np.mean([a.elapsed_time(b) for a, b in (ev["bwd"] if train else ev["fwd"])]))
    fwd_ms = float(np.mean([a.elapsed_time(b) for a, b in ev["fwd"]]))
    # the same kernel with the chip to itself (after the timed region): 50
    # back-to-back launches between two events on its launch stream
    step.alone()
    torch.cuda.synchronize()
    a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n_alone = 50
    a0.record()
    for _ in range(n_alone):
        step.alone()
    a1.record()
    torch.cuda.synchronize()
    alone_ms = a0.elapsed_time(a1) / n_alone
    clocks = None
    if rank == 0:  # the clock / power state under the same kernel: sampled while ~20 ms of it run
        gs = GpuState(dev_index)
        for _ in range(max(50, int(20.0 / max(alone_ms, 1e-3)))):
            step.alone()
        clocks = gs.sample()
        torch.cuda.synchronize()
        gs.close()
    traffic = None
    tpath = os.path.join(ROOT, "profiles", "roi_pool_bwd_traffic.json" if train
                         else "roi_pool_fwd_traffic.json")
    if os.path.exists(tpath):
        traffic = json.load(open(tpath)).get(cfg, {}).get("hbm_bytes_per_launch")
    pool_roof = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                 "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                 "kernel": step.kernel,
                 "basis": "pipeline-sustained: the kernel's algorithmic bytes per step / ms_per_step "
                          "(one launch per step)",
                 "alg_bytes_per_launch": alg_bytes,
                 "kernel_us_alone": alone_ms * 1e3,
                 "frac_alone": alg_bytes / (alone_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                 "alone_launches": n_alone,
                 "gpu_state_during_alone": clocks,
                 "event_interval_us_in_pipeline": ev_ms * 1e3}
    if not train:
        return pool_roof
    # the training step's critical path is not an HBM kernel: the target
    # creators' draws on numpy's sequential MT19937 stream, one chip-wide pass
    # for both creators (frcnn_target_draws: draw_setup / _table / _group /
    # _chain / _record kernels) on the draws' stream
    dr = ev["draw"]  # the draws' stream period: one record per step after the draws
    gaps = [a.elapsed_time(b) for a, b in zip(dr[:-1], dr[1:])]
    draw_us = float(np.mean(gaps)) * 1e3 if gaps else None  # (--steps 1: no period)
    pool_roof["fwd_event_interval_us_in_pipeline"] = fwd_ms * 1e3
    return {"bound": "latency", "kernel": "draw_setup_kernel + draw_table_kernel (chip-wide draws)",
            "unit": "us/step", "achieved": draw_us, "peak": None, "frac": None, "traffic": None,
            "basis": "the draws' stream period (both target creators' draws as one chip-wide pass: the MT19937 "
                     "state blocks twisted on one CU, per-segment step-count tables over the chip, their "
                     "chain, the recorded swaps; + the stream's wait / record packets) between consecutive "
                     "steps, HIP events; latency-bound, so no HBM / MFMA peak applies",
            "draws_share_of_step": None if draw_us is None else draw_us / (ms_step * 1e3),
            "roi_pool_bwd": pool_roof}


def main():
    args = parse()
    maybe_launch(args)
    world, rank, dev_index, backend, ndev = setup_dist(args)
    dev = torch.device("cuda", dev_index)
    from replication_faster_rcnn_amd import _lib
    from replication_faster_rcnn_amd import anchors as A
    for op, v in (("roi_pool_cg", args.roi_cg), ("roi_pool_split", args.roi_split), ("roi_pool_fwd_store", args.roi_store),
                  ("roi_pool_fwd", args.roi_path), ("propose", args.propose_path)):
        if v != "auto":
            _lib.set_path(op, v)
    from replication_faster_rcnn_amd import dist as fdist
    from replication_faster_rcnn_amd import synth
    cfg = resolve_config(args, world)
    train = cfg == "cfg5"
    if args.host_io and train:
        raise SystemExit("--host-io is measured on the inference path only")
    c_full = synth.CONFIGS[cfg]
    if cfg == "cfg3":  # configs[2]: 64 GLOBAL images sharded per image (strong scaling)
        n_total = c_full["batch"]
        scaling = "strong"
    else:              # every rank runs the config's batch (weak scaling for N > 1)
        n_total = c_full["batch"] * world
        scaling = "weak"
    mine = fdist.shard(n_total, rank, world)
    if len(mine) == 0:
        raise SystemExit(f"rank {rank}: no images ({n_total} over {world} ranks)")
    c, sets, set_bytes = make_input_sets(cfg, mine, dev, args.input_sets)
    N = sets[0][0].size(0)
    base = A.generate_anchor_base_device(anchor_scales=c["scales"])
    ev = {"fwd": [], "bwd": [], "draw": [], "i": 0,  # timing events allocated before the timed steps
          "pairs": [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                    for _ in range(args.steps)]}
    if train:
        step = train_step_fn(args, c, sets, base, mine.start, ev)
    else:
        step = inference_step_fn(args, c, sets, base, world, n_total, backend, ev)

    for _ in range(args.warmup):
        cnt = step(False)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        cnt = step(True)
    t_issue = time.perf_counter() - t0  # host time to enqueue the K steps
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([el], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
    R = int(cnt.sum().item())
    if train and R != N * 128:  # train.py:102 assumes exactly 128 samples per image
        raise RuntimeError(f"proposal targets: {cnt.tolist()} samples per image, expected 128")
    gathered = None
    if world > 1 and not train:
        dg, last = step.gathered["last"]
        g_rois, g_idx, g_cnt = dg.ordered(last)
        gathered = {"images": int(g_cnt.numel()), "rois": int(g_cnt.sum().item())}
    C, H, W = sets[0][2].shape[1:]
    alg_bytes = N * C * H * W * 4 + R * 20 + 2 * R * C * 49 * 4
    ms_step = el / args.steps * 1e3
    if args.dump_outputs:  # before anything else reuses the last step's buffers
        dump_outputs(step.last_outputs(), args.dump_outputs, rank)
    pool_roof = None
    if args.full:
        pool_roof = roofline_record(step, ev, train, cfg, rank, dev_index, alg_bytes, ms_step)
    images = n_total * args.steps
    workload = workload_name(cfg, c, N, n_total, world, C, train)
    rec = {
        "metric": "images/sec through RPN proposal+NMS+RoIPool; RoIPool HBM GB/s vs peak",
        "value": images / el, "unit": "images/sec", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": ms_step, "higher_is_better": True,
        "scaling": scaling, "vs_baseline": None, "dtype": "fp32",
        "data": f"synthetic, {len(sets)} input sets of {set_bytes / 2**20:.1f} MiB cycled (HBM-resident, "
                f"{len(sets) * set_bytes / 2**20:.0f} MiB > the 256 MiB Infinity Cache)"
                if len(sets) * set_bytes > (256 << 20) else f"synthetic, {len(sets)} input set(s) cycled",
        "config": {"workload": workload, "global_batch": n_total, "images_per_gpu": N,
                   "parallelism": f"dp{world} (per-image sharding)", "streams": args.streams,
                   "prop_streams": args.prop_streams if (args.streams == 2 and not train) else 1,
                   "pool_on": args.pool_on if (args.streams == 2 and not train) else None,
                   "host_io": bool(args.host_io), "rng_waits": args.rng_waits, "target_bufs": getattr(args, "target_bufs", 3) if train else None, "roi_path": args.roi_path, "roi_cg": args.roi_cg, "roi_split": args.roi_split, "roi_store": args.roi_store,
                   "prop_cus": args.prop_cus if (args.streams == 2 and not train) else 0,
                   "propose_path": args.propose_path,
                   "collective": (None if world == 1 else
                                  ("RCCL all_gather_into_tensor" if backend == "nccl"
                                   else "gloo all_gather_into_tensor (ranks share a GPU)")),
                   "devices": min(world, ndev), "hw_queues": HW_QUEUES},
        "roofline": pool_roof,
        "cpu_baseline": None,
        "host_issue_us_per_step": t_issue / args.steps * 1e6,
    }
    if gathered:
        rec["gathered_last_step"] = gathered
    if args.full and world > 1 and args.config == "auto" and not args.host_io:
        # configs[2] as written (64 GLOBAL images sharded per image, strong scaling),
        # beside the weak-scaled headline: the same step code, its own inputs
        try:
            rec["strong_cfg3"] = strong_cfg3(args, world, rank, dev, backend, base_of=A)
        except Exception as e:  # noqa: BLE001 -- the headline line stands on its own
            rec["strong_cfg3"] = {"error": f"{type(e).__name__}: {str(e)[:200]}"}
    if args.full and rank == 0 and world == 1 and args.cpu_seconds > 0:
        rec["cpu_baseline"] = cpu_baseline(cfg, args.cpu_seconds, args.cpu_images, train)
        rec["cpu_baseline"]["gpu_over_cpu"] = rec["value"] / rec["cpu_baseline"]["value"]
    if rank == 0:
        print(json.dumps(rec), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
