"""The FPN proposal layer's contract (DESIGN.md §3 "FPN proposals") restated on the CPU:
torchvision's ``RegionProposalNetwork.filter_proposals`` with ``BoxCoder(weights=(1, 1, 1, 1))``,
every order it leaves open refined as the contract says.  torch CPU ops for the sort, the
clamps and the comparisons, ``oracle.ref_numpy.exp_cr`` for exp, ``oracle.ref_numpy.nms``
for the greedy sweep.  It works from materialised anchors (``ops.pyramid_anchors``) and from
NHWC-flattened predictions (``permute(0, 2, 3, 1)``), so it shares no indexing with the kernels.

Users: tests/test_fpn_proposals_cpu.py (the reference held to hand results and to the
closed forms of the case table) and tests/test_gpu_fpn_proposals.py (HIP path == reference).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import ref_numpy as orc

F32 = np.float32
BBOX_XFORM_CLIP = F32(math.log(1000.0 / 16.0))


def flatten_level(obj, dlt):
    """One level's conv outputs [N,K,H,W] / [N,4K,H,W] -> logits [N, A], deltas [N, A, 4] with
    a = (y*W + x)*K + k (torchvision's permute_and_flatten)."""
    N, K, H, W = obj.shape
    lo = obj.permute(0, 2, 3, 1).reshape(N, -1)
    de = dlt.reshape(N, K, 4, H, W).permute(0, 3, 4, 1, 2).reshape(N, -1, 4)
    return lo.contiguous(), de.contiguous()


def decode(anchors, deltas):
    """BoxCoder(weights=(1,1,1,1)).decode_single, fp32, every operation rounded separately."""
    a = np.asarray(anchors, F32)
    d = np.asarray(deltas, F32)
    half = F32(0.5)
    w = a[:, 2] - a[:, 0]
    h = a[:, 3] - a[:, 1]
    cx = a[:, 0] + half * w
    cy = a[:, 1] + half * h
    clip = torch.tensor(float(BBOX_XFORM_CLIP), dtype=torch.float32)
    dw = torch.clamp(torch.from_numpy(d[:, 2].copy()), max=clip).numpy()
    dh = torch.clamp(torch.from_numpy(d[:, 3].copy()), max=clip).numpy()
    with np.errstate(all="ignore"):
        pcx = d[:, 0] * w
        pcx = pcx + cx
        pcy = d[:, 1] * h
        pcy = pcy + cy
        pw = orc.exp_cr(dw) * w
        ph = orc.exp_cr(dh) * h
        hw = half * pw
        hh = half * ph
        out = np.stack([pcx - hw, pcy - hh, pcx + hw, pcy + hh], 1).astype(F32)
    return out


def _sweep(boxes, thr):
    """Greedy NMS over boxes already in sweep order -> kept positions."""
    if len(boxes) == 0:
        return np.zeros(0, np.int64)
    stand_in = -np.arange(len(boxes), dtype=F32)
    return orc.nms(np.ascontiguousarray(boxes, F32), stand_in, thr)


def level_candidates(logits, deltas, anchors, img_hw, pre, score_thresh, min_size):
    """Steps 1-3 for one (image, level): (boxes, logits, anchor indices) of the survivors, in
    selection order."""
    lt = torch.from_numpy(np.ascontiguousarray(logits, F32))
    order = torch.sort(lt, descending=True, stable=True).indices[:min(int(pre), len(logits))].numpy()
    box = torch.from_numpy(decode(np.asarray(anchors, F32)[order], np.asarray(deltas, F32)[order]))
    h, w = float(img_hw[0]), float(img_hw[1])
    x = torch.clamp(box[:, 0::2], min=0.0, max=torch.tensor(w, dtype=torch.float32).item())
    y = torch.clamp(box[:, 1::2], min=0.0, max=torch.tensor(h, dtype=torch.float32).item())
    box = torch.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], 1)
    ms = torch.tensor(float(min_size), dtype=torch.float32)
    keep = ((box[:, 2] - box[:, 0]) >= ms) & ((box[:, 3] - box[:, 1]) >= ms)
    sel = lt[torch.from_numpy(order)]
    keep &= torch.sigmoid(sel) >= float(score_thresh)      # torchvision's own test; a NaN fails it
    k = keep.numpy()
    return box.numpy()[k], sel.numpy()[k], order[k]


def reference(objectness, deltas, anchors, image_sizes, *, pre, post, nms_thresh=0.7, score_thresh=0.0,
              min_size=1e-3, level_aware=True):
    """The six padded outputs as numpy arrays (boxes, logits, levels, anchor_idx, count, rois).
    ``objectness`` / ``deltas``: lists of fp32 CPU tensors as the op takes them; ``anchors``: list
    of [A_l, 4]; ``image_sizes``: [N, 2] of (h, w).  ``level_aware=False``: one sweep over the
    image's candidates of all levels (what the contract rules out)."""
    L = len(objectness)
    N = objectness[0].shape[0]
    flat = [flatten_level(o.float(), d.float()) for o, d in zip(objectness, deltas)]
    sizes = np.asarray(image_sizes, F32).reshape(N, 2)
    boxes = np.zeros((N, post, 4), F32)
    logits = np.full((N, post), -np.inf, F32)
    levels = np.full((N, post), -1, np.int32)
    aidx = np.full((N, post), -1, np.int32)
    count = np.zeros(N, np.int32)
    rois = np.zeros((N * post, 5), F32)
    rois[:, 0] = -1
    for n in range(N):
        kb, kl, klev, ka = [], [], [], []
        for l in range(L):
            b, s, a = level_candidates(flat[l][0][n].numpy(), flat[l][1][n].numpy(), anchors[l].numpy(), sizes[n],
                                       pre, score_thresh, min_size)
            if level_aware:
                k = _sweep(b, nms_thresh)[:post]
                b, s, a = b[k], s[k], a[k]
            kb.append(b)
            kl.append(s)
            klev.append(np.full(len(s), l, np.int32))
            ka.append(a)
        b, s, lv, a = np.concatenate(kb), np.concatenate(kl), np.concatenate(klev), np.concatenate(ka)
        # (logit descending, level ascending, anchor ascending): a stable sort of the level-major list
        o = torch.sort(torch.from_numpy(s.copy()), descending=True, stable=True).indices.numpy()
        b, s, lv, a = b[o], s[o], lv[o], a[o]
        if not level_aware:
            k = _sweep(b, nms_thresh)
            b, s, lv, a = b[k], s[k], lv[k], a[k]
        c = min(len(s), post)
        boxes[n, :c], logits[n, :c], levels[n, :c], aidx[n, :c], count[n] = b[:c], s[:c], lv[:c], a[:c], c
        rois[n * post:n * post + c, 0] = n
        rois[n * post:n * post + c, 1:] = b[:c]
    return boxes, logits, levels, aidx, count, rois
