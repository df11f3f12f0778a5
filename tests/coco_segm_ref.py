"""numpy restatement of the COCO segm evaluation contract (DESIGN.md "COCO segm
evaluation": pycocotools.cocoeval with iouType "segm"), and the generator of its
random test case.

The overlap is brute force: ``np.count_nonzero(a & b)`` per considered pair.  The
matching is ``coco_eval_ref``'s -- its ``match_sequential`` / ``State``, imported
-- fed with an IoU matrix built from those counts as maskApi.c's ``rleIou``
builds it: 0 without a common pixel, ``i / a_d`` against a crowd, ``i / (a_d +
a_g - i)`` otherwise; exact integers, one fp64 division.
"""
import numpy as np

import coco_eval_ref as cref
from replication_faster_rcnn_amd import synth

T, A, KEEP, RANK_OUT, U = cref.T, cref.A, cref.KEEP, cref.RANK_OUT, cref.U


# --------------------------------------------------------------------- overlap
def considered(D, G, det_labels=None, det_count=None, gt_labels=None, n_class=None):
    """bool [D, G] of one image: the pairs whose intersection is counted."""
    k = D if det_count is None else int(np.clip(det_count, 0, D))
    ok = np.zeros((D, G), bool)
    ok[:k] = True
    if det_labels is not None:
        dl, gl = np.asarray(det_labels, np.int64), np.asarray(gt_labels, np.int64)
        ok &= (dl[:, None] == gl[None, :]) & ((dl >= 1) & (dl < n_class))[:, None]
    return ok


def overlap(det_masks, gt_masks, det_labels=None, det_count=None, gt_labels=None, n_class=None):
    """-> (inter int32 [N, D, G], det_area int32 [N, D], gt_area int32 [N, G]).  The masks at or
    beyond det_count are not looked at."""
    N, D = det_masks.shape[:2]
    G = gt_masks.shape[1]
    inter = np.zeros((N, D, G), np.int32)
    da = np.zeros((N, D), np.int32)
    ga = np.zeros((N, G), np.int32)
    for n in range(N):
        k = D if det_count is None else int(np.clip(det_count[n], 0, D))
        ok = considered(D, G, None if det_labels is None else det_labels[n], k,
                        None if gt_labels is None else gt_labels[n], n_class)
        for g in range(G):
            ga[n, g] = np.count_nonzero(gt_masks[n, g])
        for d in range(k):
            a = det_masks[n, d] != 0
            da[n, d] = np.count_nonzero(a)
            for g in np.nonzero(ok[d])[0]:
                inter[n, d, g] = np.count_nonzero(a & (gt_masks[n, g] != 0))
    return inter, da, ga


# ------------------------------------------ a second form of the overlap: RLE
def rle(mask):
    """Column-major run lengths, zeros first (maskApi.c's rleEncode)."""
    v = (mask != 0).reshape(-1, order="F")
    bounds = np.concatenate([[0], np.flatnonzero(v[1:] != v[:-1]) + 1, [len(v)]])
    counts = np.diff(bounds)
    return np.concatenate([[0], counts]) if v[0] else counts


def rle_walk(a, b):
    """rleIou's walk over two run lists -> pixels set in both."""
    ia = ib = 0
    ca, cb = int(a[0]), int(b[0])
    va = vb = False
    inter, ct = 0, 1
    while ct > 0:
        c = min(ca, cb)
        if va and vb:
            inter += c
        ct = 0
        ca -= c
        if not ca and ia + 1 < len(a):
            ia += 1
            ca = int(a[ia])
            va = not va
        ct += ca
        cb -= c
        if not cb and ib + 1 < len(b):
            ib += 1
            cb = int(b[ib])
            vb = not vb
        ct += cb
    return inter


# ------------------------------------------------------------------------- IoU
def iou_from_counts(i, a_d, a_g, crowd, garea=None):
    """rleIou on counts: one detection row.  i [G], a_d scalar, a_g [G] the gt's pixel counts, crowd
    bool [G] -> fp64 [G].  garea, the gt's areas for the size ranges, plays no part."""
    i = np.asarray(i, np.int64)
    u = np.where(crowd, np.int64(a_d), np.int64(a_d) + np.asarray(a_g, np.int64) - i)
    out = np.zeros(len(i), np.float64)
    nz = i != 0
    out[nz] = i[nz].astype(np.float64) / u[nz].astype(np.float64)
    return out


class State(cref.State):
    """coco_eval_ref.State with the IoU rows and areas of iouType "segm"."""

    def __init__(self, C, cap, match=cref.match_sequential, iou=iou_from_counts):
        super().__init__(C, cap, match)
        self.iou = iou

    def update(self, det_labels, det_scores, det_count, inter, det_pix, gt_pix, gt_labels, gt_crowd=None,
               gt_area=None):
        N, M = det_labels.shape
        C = self.C
        ks = np.clip(det_count.astype(np.int64), 0, M)
        nrec = int(self.hdr[0])
        if nrec + int(ks.sum()) > self.cap:
            self.hdr[2] += 1
            return
        G = gt_labels.shape[1]
        for n in range(N):
            k = int(ks[n])
            gl = gt_labels[n].astype(np.int64)
            gl = np.where((gl >= 1) & (gl < C), gl, 0)
            gc = np.zeros(G, bool) if gt_crowd is None else np.asarray(gt_crowd[n]) != 0
            garea = (gt_pix[n] if gt_area is None else gt_area[n]).astype(np.float64)
            for g in range(G):
                if gl[g] and not gc[g]:
                    for a in range(4):
                        if A[a, 0] <= garea[g] <= A[a, 1]:
                            self.npig[gl[g], a] += 1
            lab = det_labels[n, :k].astype(np.int64)
            cls = np.where((lab >= 1) & (lab < C), lab, 0)
            skey = cref.desc_score_key(det_scores[n, :k])
            idx = nrec + np.arange(k, dtype=np.int64)
            self.rec_key[nrec:nrec + k] = (cls.astype(U) << U(56)) | (skey.astype(U) << U(24)) | idx.astype(U)
            self.rec_bits[nrec:nrec + k, 0] = 0
            self.rec_bits[nrec:nrec + k, 1] = U(RANK_OUT) << U(32)
            diag = {}
            for c in np.unique(cls[cls > 0]):
                slots = np.nonzero(cls == c)[0]
                slots = slots[np.argsort(skey[slots], kind="stable")][:KEEP]
                gs = np.nonzero(gl == c)[0]
                ious = np.zeros((len(slots), len(gs)))
                for r, s in enumerate(slots):
                    ious[r] = self.iou(inter[n, s, gs], det_pix[n, s], gt_pix[n, gs], gc[gs], garea[gs])
                darea = det_pix[n, slots].astype(np.float64)
                dtm = np.zeros((4, len(T), len(slots)), bool)
                dtig = np.zeros((4, len(T), len(slots)), bool)
                for a in range(4):
                    gig = gc[gs] | (garea[gs] < A[a, 0]) | (garea[gs] > A[a, 1])
                    dtm[a], dtig[a], dtg = self.match(ious, gig, gc[gs], darea, A[a, 0], A[a, 1])
                    diag[(int(c), a)] = (slots, np.where(dtg >= 0, gs[np.maximum(dtg, 0)] if len(gs) else -1, -1))
                for rank, s in enumerate(slots):
                    self.rec_bits[nrec + s] = cref.pack_bits(dtm[:, :, rank], dtig[:, :, rank], rank)
            self.matched_gt.append(diag)
            nrec += k
        self.hdr[0] = nrec
        self.hdr[1] += N


# ----------------------------------------------------------------------- cases
ARGS = ("det_masks", "gt_masks", "det_labels", "det_scores", "det_count", "gt_labels", "gt_crowd", "gt_area")


def case(det_masks, gt_masks, det_labels, det_scores, det_count, gt_labels, gt_crowd=None, gt_area=None):
    N, G = np.asarray(gt_labels).shape
    return dict(det_masks=np.ascontiguousarray(det_masks, np.uint8), gt_masks=np.ascontiguousarray(gt_masks, np.uint8),
                det_labels=np.ascontiguousarray(det_labels, np.int32),
                det_scores=np.ascontiguousarray(det_scores, np.float32),
                det_count=np.ascontiguousarray(det_count, np.int32), gt_labels=np.ascontiguousarray(gt_labels, np.int32),
                gt_crowd=np.zeros((N, G), np.uint8) if gt_crowd is None else np.ascontiguousarray(gt_crowd, np.uint8),
                gt_area=None if gt_area is None else np.ascontiguousarray(gt_area, np.float64))


def images(H, W, *imgs, M=None, G=None, value=1):
    """imgs: (det, gt) per image with det [(mask, label, score)] and gt [(mask, label, crowd)] or
    [(mask, label, crowd, area)]; a mask is a bool / uint8 [H, W] array or a list of (y0, x0, y1, x1)
    rectangles (half-open) that are set.  Slots at or past the count hold junk."""
    M = M or max(1, max(len(d) for d, _ in imgs))
    G = G if G is not None else max(len(g) for _, g in imgs)
    N = len(imgs)
    dm = np.full((N, M, H, W), 7, np.uint8)
    gm = np.zeros((N, G, H, W), np.uint8)
    dl = np.full((N, M), cref.GARBAGE_LABEL, np.int32)
    ds = np.full((N, M), cref.GARBAGE_SCORE, np.float32)
    dc = np.zeros(N, np.int32)
    gl = -np.ones((N, G), np.int32)
    gc = np.zeros((N, G), np.uint8)
    ga = np.zeros((N, G), np.float64)
    with_area = False
    for n, (det, gt) in enumerate(imgs):
        dc[n] = len(det)
        for i, (m, l, s) in enumerate(det):
            dm[n, i], dl[n, i], ds[n, i] = draw(H, W, m, value), l, s
        for i, g in enumerate(gt):
            gm[n, i], gl[n, i], gc[n, i] = draw(H, W, g[0], value), g[1], g[2]
            ga[n, i] = np.count_nonzero(gm[n, i])
            if len(g) > 3:
                ga[n, i] = g[3]
                with_area = True
    return case(dm, gm, dl, ds, dc, gl, gc, ga if with_area else None)


def draw(H, W, m, value=1):
    if isinstance(m, np.ndarray):
        return (m != 0).astype(np.uint8) * value
    out = np.zeros((H, W), np.uint8)
    for y0, x0, y1, x1 in m:
        out[y0:y1, x0:x1] = value
    return out


def concat(cases):
    out = {k: np.concatenate([c[k] for c in cases]) for k in ARGS[:-1]}
    out["gt_area"] = None if cases[0]["gt_area"] is None else np.concatenate([c["gt_area"] for c in cases])
    return out


def run(cases, C, cap=None, match=cref.match_sequential, iou=iou_from_counts):
    """The restatement over a list of batches -> (State, [overlap of each batch])."""
    st = State(C, cap or sum(c["det_labels"].size for c in cases), match, iou)
    overlaps = []
    for c in cases:
        ov = overlap(c["det_masks"], c["gt_masks"], c["det_labels"], c["det_count"], c["gt_labels"], C)
        overlaps.append(ov)
        st.update(c["det_labels"], c["det_scores"], c["det_count"], *ov, c["gt_labels"], c["gt_crowd"], c["gt_area"])
    return st, overlaps


def blob(r, H, W, cy, cx, hh, hw):
    """A union of one to three rectangles and ellipses around (cy, cx) with half sizes about (hh, hw)."""
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), bool)
    for _ in range(int(r.integers(1, 4))):
        oy, ox = cy + r.uniform(-0.3, 0.3) * hh, cx + r.uniform(-0.3, 0.3) * hw
        sy, sx = hh * r.uniform(0.6, 1.0), hw * r.uniform(0.6, 1.0)
        if r.uniform() < 0.5:
            m |= (np.abs(yy - oy) <= sy) & (np.abs(xx - ox) <= sx)
        else:
            m |= ((yy - oy) / sy) ** 2 + ((xx - ox) / sx) ** 2 <= 1.0
    return m


def random_case(N=2, D=100, G=32, H=200, W=200, C=4, seed=7, crowd=0.2, first_image=0, n_gt=12):
    """Blobs of rectangles and ellipses, classes 1..C-1, some crowds.  Per image about 12 valid gt in
    random slots; 75 % of the detections are a gt's blob -- an exact copy (IoU 1, matched at 0.95), a
    copy with a strip removed or a margin added, or one shifted by up to half its size -- 15 % of
    those under another class; the rest are blobs anywhere.  Masks are 0 / 255 on even images and
    0 / 1 on odd ones.  Slots at or past the count hold junk bytes."""
    dm = np.zeros((N, D, H, W), np.uint8)
    gm = np.zeros((N, G, H, W), np.uint8)
    dl = np.full((N, D), cref.GARBAGE_LABEL, np.int32)
    ds = np.full((N, D), cref.GARBAGE_SCORE, np.float32)
    dc = np.zeros(N, np.int32)
    gl = -np.ones((N, G), np.int32)
    gc = np.zeros((N, G), np.uint8)
    lo, hi = min(H, W) / 50.0, 0.3 * min(H, W)          # half sizes: 4 .. 60 on a 200 x 200 canvas
    for n in range(N):
        r = synth.rng_for(seed, first_image + n, 23)
        val = 255 if n % 2 == 0 else 1
        nv = min(G, n_gt)
        slots = np.sort(r.choice(G, nv, replace=False))
        geo = {}
        for g in slots:
            hh, hw = np.exp(r.uniform(np.log(lo), np.log(hi), 2))
            cy, cx = r.uniform(hh, H - hh), r.uniform(hw, W - hw)
            geo[g] = (cy, cx, hh, hw)
            gm[n, g] = blob(r, H, W, cy, cx, hh, hw) * val
            gl[n, g] = int(r.integers(1, C))
            gc[n, g] = r.uniform() < crowd
        k = max(D - 7 * n, 0)
        dc[n] = k
        dm[n, k:] = r.integers(0, 256, (D - k, H, W), dtype=np.uint8)        # junk beyond the count
        for s in range(k):
            if r.uniform() < 0.75:
                g = int(r.choice(slots))
                cy, cx, hh, hw = geo[g]
                m = gm[n, g] != 0
                kind = r.uniform()
                if kind < 0.25:
                    pass
                elif kind < 0.5:
                    m = m.copy()
                    m[:, :int(cx - hw * r.uniform(0.3, 0.9))] = False
                elif kind < 0.75:
                    dy, dx = int(hh * r.uniform(-0.5, 0.5)), int(hw * r.uniform(-0.5, 0.5))
                    m = np.roll(np.roll(m, dy, 0), dx, 1)
                else:
                    m = m | blob(r, H, W, cy, cx, hh * 1.15, hw * 1.15)
                dm[n, s] = m * val
                dl[n, s] = gl[n, g]
                if r.uniform() < 0.15:
                    dl[n, s] = 1 + (gl[n, g] - 1 + int(r.integers(1, C - 1))) % (C - 1)
            else:
                hh, hw = np.exp(r.uniform(np.log(lo), np.log(hi), 2))
                dm[n, s] = blob(r, H, W, r.uniform(hh, H - hh), r.uniform(hw, W - hw), hh, hw) * val
                dl[n, s] = int(r.integers(1, C))
            ds[n, s] = np.round(r.uniform(0, 1) * 64) / 64
    return case(dm, gm, dl, ds, dc, gl, gc)
