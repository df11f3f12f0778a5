"""ops.mask_overlap against the brute-force restatement (tests/coco_segm_ref.py) on the named
cases of tests/mask_overlap_cases.py.

Bars: ``inter``, ``det_area`` and ``gt_area`` are bit-exact (they are integers).  Every case first
asserts its launch plan through frcnn_mask_overlap_plan, then runs twice into outputs that were
filled with a sentinel and have guarded tails, with a workspace whose tail is guarded: every
element is stored, nothing past the end is, and two calls give the same bits."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import coco_segm_ref as ref  # noqa: E402
import mask_overlap_cases as mc  # noqa: E402
from replication_faster_rcnn_amd import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu

SENT, GUARD = -0x5A5A5A5B, 64
_cache = {}


def built(name):
    """(case, restatement's outputs): made once, never modified."""
    if name not in _cache:
        c = mc.CASES[name]()
        _cache[name] = (c, ref.overlap(c["det_masks"], c["gt_masks"], c["det_labels"], c["det_count"],
                                       c["gt_labels"], c["n_class"]))
    return _cache[name]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(shape):
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENT, dtype=torch.int32, device="cuda")
    return buf, buf[:n].view(shape)


def run_guarded(c):
    """One call into sentinel-filled, guarded outputs and a guarded workspace -> host arrays."""
    N, D, H, W = c["det_masks"].shape
    G = c["gt_masks"].shape[1]
    need = _lib.mask_overlap_plan(N, D, G, H, W)["workspace"]
    ws = torch.full((need + 4 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    bufs, outs = zip(*(guarded(s) for s in ((N, D, G), (N, D), (N, G))))
    got = ops.mask_overlap(dev(c["det_masks"]), dev(c["gt_masks"]), det_labels=dev(c["det_labels"]),
                           det_count=dev(c["det_count"]), gt_labels=dev(c["gt_labels"]), n_class=c["n_class"],
                           out=outs, workspace=ws[:need])
    assert isinstance(got, ops.MaskOverlap) and all(a is b for a, b in zip(got, outs))
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()), "the workspace's tail was written"
    for name, b, o in zip(got._fields, bufs, outs):
        assert bool((b[o.numel():] == SENT).all()), f"{name}: written past its end"
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_named_case(name):
    c, want = built(name)
    N, D, H, W = c["det_masks"].shape
    G = c["gt_masks"].shape[1]
    plan = _lib.mask_overlap_plan(N, D, G, H, W)
    for k, v in c["plan"].items():
        assert plan[k] == v, (k, plan[k], v)
    assert ops.mask_overlap_kernel(H, W) == "mo_pack_kernel[vec16%s]+mo_pair_kernel" % ("+edges" if plan["edges"] else "")
    first, second = run_guarded(c), run_guarded(c)
    for which, a, b, w in zip(("inter", "det_area", "gt_area"), first, second, want):
        assert not (a == SENT).any(), f"{which}: {int((a == SENT).sum())} elements were never stored"
        assert np.array_equal(a, w), (which, np.argwhere(a != w)[:8], a[a != w][:8], w[a != w][:8])
        assert np.array_equal(a, b), f"{which}: two calls differ"
    out = dict(zip(("inter", "det_area", "gt_area"), first))
    for (which, idx), v in c["expect"].items():
        assert out[which][idx] == v, (which, idx, out[which][idx], v)


def test_junk_beyond_the_count_reaches_no_output():
    c, _ = built("count_below_d_junk")
    z = mc.junk_zeroed(c)
    assert not np.array_equal(z["det_masks"], c["det_masks"])
    for a, b in zip(run_guarded(c), run_guarded(z)):
        assert np.array_equal(a, b)


def test_default_outputs_and_cached_workspace():
    c, want = built("w600")
    got = ops.mask_overlap(dev(c["det_masks"]), dev(c["gt_masks"]))
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
    assert [g.dtype for g in got] == [torch.int32] * 3 and got.inter.shape == (2, 3, 2)


def test_no_gt_slots():
    d = dev(mc.random_masks(400, 2, 3, 5, 20))
    got = ops.mask_overlap(d, torch.zeros((2, 0, 5, 20), dtype=torch.uint8, device="cuda"))
    assert got.inter.shape == (2, 3, 0) and got.gt_area.shape == (2, 0)
    assert np.array_equal(got.det_area.cpu().numpy(), np.count_nonzero(d.cpu().numpy(), axis=(2, 3)))


def test_wrapper_rejects_wrong_inputs_before_any_launch():
    c, _ = built("labels_differ")
    dm, gm, dl, dc, gl = (dev(c[k]) for k in ("det_masks", "gt_masks", "det_labels", "det_count", "gt_labels"))
    N, D, H, W = dm.shape
    G = gm.shape[1]
    bufs, outs = zip(*(guarded(s) for s in ((N, D, G), (N, D), (N, G))))
    good = dict(det_masks=dm, gt_masks=gm, det_labels=dl, det_count=dc, gt_labels=gl, n_class=3, out=outs)

    def refused(match, **over):
        a = dict(good, **over)
        with pytest.raises(RuntimeError, match=match):
            ops.mask_overlap(a.pop("det_masks"), a.pop("gt_masks"), **a)

    refused("det_masks", det_masks=dm.bool())
    refused("det_masks", det_masks=dm.float())
    refused("det_masks", det_masks=dm.cpu())
    refused("det_masks", det_masks=dm[0])
    refused("det_masks", det_masks=dm.transpose(2, 3).contiguous().transpose(2, 3))
    refused("gt_masks", gt_masks=gm.int())
    refused("gt_masks", gt_masks=gm.cpu())
    refused("canvas", gt_masks=gm[:, :, :, :W - 1].contiguous())
    refused("canvas", gt_masks=gm[:, :, :H - 1].contiguous())
    refused("gt_masks", gt_masks=gm.repeat(2, 1, 1, 1))             # another N
    refused("D=1025", det_masks=torch.zeros((1, 1025, 1, 16), dtype=torch.uint8, device="cuda"),
            gt_masks=torch.zeros((1, 1, 1, 16), dtype=torch.uint8, device="cuda"))
    refused("G=257", det_masks=dm[:, :, :1, :16].contiguous(),
            gt_masks=torch.zeros((N, 257, 1, 16), dtype=torch.uint8, device="cuda"))
    refused("W=4097", det_masks=torch.zeros((1, 1, 1, 4097), dtype=torch.uint8, device="cuda"),
            gt_masks=torch.zeros((1, 1, 1, 4097), dtype=torch.uint8, device="cuda"))
    refused("together", gt_labels=None)
    refused("together", det_labels=None)
    refused("n_class", n_class=None)
    refused("n_class", n_class=129)
    refused("n_class", n_class=1)
    refused("det_labels", det_labels=dl.long())
    refused("det_labels", det_labels=dl[:, :1])
    refused("gt_labels", gt_labels=gl.cpu())
    refused("det_count", det_count=dc.long())
    refused("det_count", det_count=dc.repeat(2))
    refused("aligned", det_masks=torch.zeros(N * D * H * W + 1, dtype=torch.uint8, device="cuda")[1:].view(N, D, H, W))
    refused("out", out=outs[:2])
    refused("out.inter", out=(outs[0].long(), outs[1], outs[2]))
    refused("out.gt_area", out=(outs[0], outs[1], outs[2][:, :1]))
    refused("workspace", workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))
    refused("workspace", workspace=torch.empty(1 << 16, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert all(bool((b == SENT).all()) for b in bufs), "a refused call wrote an output"
