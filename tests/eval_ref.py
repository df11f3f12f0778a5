"""numpy restatement of the evaluation contract (DESIGN.md "Evaluation"), and
the generator of its test cases.

The matching here is the VOC devkit's sequential loop: an image's detections
are walked in descending score order (ties by slot), each takes the first
maximum-IoU gt of its class, and a gt already taken makes the next claimant a
false positive.  The library decides "taken" in parallel, by the minimum claim
key per gt, so the two forms check each other.
"""
import numpy as np

from replication_faster_rcnn_amd import synth

GARBAGE_BOX, GARBAGE_LABEL, GARBAGE_SCORE = 1e30, 1, 9.0   # slots at or past the count

CHUNK = 256   # records per restart of the two chunk mistakes below: the kernels' workgroup size

# Planted mistakes (``mistake=``): each is one way a kernel could depart from the contract.  tests/eval_cases.py
# names the case that must tell each of them apart from the contract.
MATCH_MISTAKES = ("non_strict_threshold", "last_gt_wins_tie", "claim_by_slot", "nan_score_last", "neg_zero_below_zero",
                  "difficult_consumes", "difficult_in_npos", "plus_one_in_fp32", "invalid_label_is_fp",
                  "count_not_clamped", "prefix_first_256_images")
AP_MISTAKES = ("unstable_sort", "envelope_restarts_each_chunk", "envelope_restarts_each_chunk_from_end",
               "running_sum_restarts_each_chunk", "running_sum_restarts_each_chunk_from_end", "no_division_guard",
               "empty_class_is_nan", "tenths_by_division")
MISTAKES = MATCH_MISTAKES + AP_MISTAKES


def desc_score_key(s):
    """csrc/common.h desc_score_key: fp32 -> uint32 ascending for descending scores,
    with torch's equalities: every NaN gets key 0, -0.0 gets +0.0's key."""
    s = np.ascontiguousarray(s, np.float32)
    u = np.where(s == 0, np.float32(0), s).view(np.uint32)
    asc = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return np.where(np.isnan(s), np.uint32(0), ~asc).astype(np.uint32)


def score_key(s, mistake=None):
    """desc_score_key, or what a planted mistake makes of it: ``nan_score_last`` gives NaN the
    largest key, ``neg_zero_below_zero`` leaves -0.0 its own bit pattern's key, just after +0.0's."""
    s = np.ascontiguousarray(s, np.float32)
    k = desc_score_key(s)
    if mistake == "nan_score_last":
        k = np.where(np.isnan(s), np.uint32(0xFFFFFFFF), k)
    if mistake == "neg_zero_below_zero":
        k = np.where(s.view(np.uint32) == np.uint32(0x80000000), np.uint32(0x80000000), k)
    return k.astype(np.uint32)


def desc_order(s, mistake=None):
    """Slots in torch's own stable descending order (NaN first, -0.0 == +0.0,
    ties by slot): the order the devkit loop walks an image's detections in."""
    if mistake == "claim_by_slot":
        return list(range(len(s)))
    if mistake in ("nan_score_last", "neg_zero_below_zero"):
        return np.argsort(score_key(s, mistake), kind="stable").tolist()
    import torch
    t = torch.from_numpy(np.ascontiguousarray(s, np.float32))
    return torch.sort(t, descending=True, stable=True).indices.numpy().tolist()


def iou(a, b, plus_one=1, mistake=None):
    """bbox_iou (utils/utils.py:102-119) of one box a against boxes b [g, 4] in
    fp64, after the pixel convention's +1 on columns 2, 3 of both.  ``plus_one_in_fp32``
    adds the detection's +1 before the widening instead of after it."""
    if plus_one and mistake == "plus_one_in_fp32":
        a = np.array(a, np.float32)
        a[2:] = a[2:] + np.float32(1.0)
    a = np.array(a, np.float64).reshape(1, 4)
    b = np.array(b, np.float64).reshape(-1, 4)
    if plus_one:
        if mistake != "plus_one_in_fp32":
            a[:, 2:] = a[:, 2:] + 1.0
        b[:, 2:] = b[:, 2:] + 1.0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        tl = np.maximum(a[:, None, :2], b[:, :2])
        br = np.minimum(a[:, None, 2:], b[:, 2:])
        area_i = np.prod(br - tl, axis=2) * (tl < br).all(axis=2)
        area_a = np.prod(a[:, 2:] - a[:, :2], axis=1)
        area_b = np.prod(b[:, 2:] - b[:, :2], axis=1)
        return (area_i / (area_a[:, None] + area_b - area_i))[0]


def match_image(boxes, labels, scores, k, gt_boxes, gt_labels, gt_difficult, C, iou_thresh=0.5, plus_one=1,
                mistake=None):
    """The devkit loop on one image.  Returns per slot below k: flag (1 TP, 0
    FP, -1 ignored), record class (0 for a label outside 1..C-1) and the gt the
    slot was matched to (-1: none)."""
    flag = np.zeros(k, np.int8)
    cls = np.zeros(k, np.int64)
    best = np.full(k, -1, np.int64)
    taken = np.zeros(len(gt_labels), bool)
    for s in desc_order(scores[:k], mistake):
        lab = int(labels[s])
        if not 1 <= lab < C:
            flag[s] = 0 if mistake == "invalid_label_is_fp" else -1
            continue
        cls[s] = lab
        cand = [j for j in range(len(gt_labels)) if int(gt_labels[j]) == lab]
        ovmax, jmax = -np.inf, -1
        if cand:
            for j, ov in zip(cand, iou(boxes[s], gt_boxes[cand], plus_one, mistake)):
                # strict: a tie stays with the first gt, a NaN never wins
                if ov > ovmax or (mistake == "last_gt_wins_tie" and ov >= ovmax):
                    ovmax, jmax = ov, j
        if ovmax > iou_thresh or (mistake == "non_strict_threshold" and ovmax >= iou_thresh):
            best[s] = jmax
            if gt_difficult is not None and gt_difficult[jmax]:
                flag[s] = 0 if mistake == "difficult_consumes" and taken[jmax] else -1
                taken[jmax] = taken[jmax] or mistake == "difficult_consumes"
            elif not taken[jmax]:
                flag[s] = 1
                taken[jmax] = True
            else:
                flag[s] = 0
    return flag, cls, best


class State:
    """The accumulator arrays of the contract, on the host."""

    def __init__(self, C, cap):
        self.C, self.cap = C, cap
        self.hdr = np.zeros(4 + C, np.int64)
        self.rec_key = np.zeros(cap, np.uint64)
        self.rec_flag = np.zeros(cap, np.int8)
        self.rec_image = np.zeros(cap, np.int32)
        self.best = []   # per update and image: match_image's matched gt (diagnostics for preconditions)

    def update(self, det_boxes, det_labels, det_scores, det_count, gt_boxes, gt_labels, gt_difficult=None,
               iou_thresh=0.5, plus_one=1, mistake=None):
        N, M = det_labels.shape
        C = self.C
        ks = np.clip(det_count.astype(np.int64), 0, M)
        # what the positions are derived from: the clamped counts of all N images
        counted = det_count.astype(np.int64) if mistake == "count_not_clamped" else ks
        lim = min(N, 256) if mistake == "prefix_first_256_images" else N
        nrec = int(self.hdr[0])
        total = int(counted[:lim].sum())
        if nrec + total > self.cap:
            self.hdr[2] += 1
            return
        for n in range(N):
            k = int(ks[n])
            gl = gt_labels[n].astype(np.int64)
            valid = (gl >= 1) & (gl < C)
            gl = np.where(valid, gl, 0)
            gd = None if gt_difficult is None else gt_difficult[n]
            flag, cls, best = match_image(det_boxes[n], det_labels[n], det_scores[n], k, gt_boxes[n], gl, gd, C,
                                          iou_thresh, plus_one, mistake)
            self.best.append(best)
            idx = nrec + int(counted[:min(n, lim)].sum()) + np.arange(k, dtype=np.int64)
            key = (cls.astype(np.uint64) << np.uint64(56)) | \
                  (score_key(det_scores[n, :k], mistake).astype(np.uint64) << np.uint64(24)) | \
                  (idx.astype(np.uint64) & np.uint64(0xFFFFFF))
            ok = (idx >= 0) & (idx < self.cap)          # all of them without a mistake
            self.rec_key[idx[ok]] = key[ok]
            self.rec_flag[idx[ok]] = flag[ok]
            self.rec_image[idx[ok]] = self.hdr[1] + n
            pos = valid if gd is None or mistake == "difficult_in_npos" else valid & (np.asarray(gd) == 0)
            np.add.at(self.hdr, 4 + gl[pos], 1)
        self.hdr[0] = nrec + total
        self.hdr[1] += N

    def ap(self, use_07_metric=False, mistake=None, n_records=None):
        """-> (ap [C], map, sorted_key [n_records], records per class [C]).  ``n_records``
        (default hdr[0]): only the first n_records records count."""
        n = int(self.hdr[0]) if n_records is None else int(n_records)
        key = self.rec_key[:n]
        if mistake == "unstable_sort":                       # equal (class, score): the later record first
            sk = key[np.lexsort((-(key & np.uint64(0xFFFFFF)).astype(np.int64), key >> np.uint64(24)))]
        else:
            sk = np.sort(key)                                # keys are distinct
        ri = (sk & np.uint64(0xFFFFFF)).astype(np.int64)
        fl = np.where(ri < n, self.rec_flag[np.minimum(ri, self.cap - 1)], -1)   # a key that is no record: ignored
        kc = (sk >> np.uint64(56)).astype(np.int64)
        ap = np.full(self.C, np.nan)
        for c in range(1, self.C):
            npos = int(self.hdr[4 + c])
            if npos == 0:
                continue
            f = fl[kc == c]
            if len(f) == 0 and mistake == "empty_class_is_nan":
                continue
            tp = _running(f == 1, mistake)
            fp = _running(f == 0, mistake)
            rec = tp / float(npos)
            if mistake == "no_division_guard":
                with np.errstate(invalid="ignore", divide="ignore"):
                    prec = tp / (tp + fp).astype(np.float64)
            else:
                prec = tp / np.maximum(tp + fp, 1).astype(np.float64)
            if use_07_metric:
                a = 0.0
                for i in range(11):
                    m = prec[rec >= (i / 10 if mistake == "tenths_by_division" else i * 0.1)]
                    a = a + (m.max() if m.size else 0.0) / 11.0
            else:
                mrec = np.concatenate([[0.0], rec, [1.0]])
                mpre = np.concatenate([[0.0], prec, [0.0]])
                mpre = np.maximum.accumulate(mpre[::-1])[::-1]
                if mistake in ("envelope_restarts_each_chunk", "envelope_restarts_each_chunk_from_end"):
                    mpre[1:-1] = _chunk_envelope(prec, from_end=mistake.endswith("from_end"))
                i = np.nonzero(mrec[1:] != mrec[:-1])[0]
                a = float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))
            ap[c] = a
        s, k = 0.0, 0
        for c in range(self.C):
            if ap[c] == ap[c]:
                s, k = s + ap[c], k + 1
        return ap, (s / k if k else float("nan")), sk, np.bincount(kc, minlength=self.C)


def _chunks(n, from_end):
    """[lo, hi) of the chunks of CHUNK records of an n-record segment, counted from its first
    record or (``from_end``, the direction ev_pr_walk walks in) from its last."""
    cuts = sorted({0, n} | set(range(n % CHUNK if from_end else 0, n, CHUNK)))
    return list(zip(cuts[:-1], cuts[1:]))


def _running(hit, mistake=None):
    """Running count of ``hit`` over a segment; the two ``running_sum_restarts_each_chunk``
    mistakes start again from 0 at every chunk."""
    if mistake in ("running_sum_restarts_each_chunk", "running_sum_restarts_each_chunk_from_end") and len(hit):
        return np.concatenate([np.cumsum(hit[lo:hi]) for lo, hi in _chunks(len(hit), mistake.endswith("from_end"))])
    return np.cumsum(hit)


def _chunk_envelope(prec, from_end):
    """The suffix maximum of ``prec`` restarted at every chunk."""
    out = np.zeros(len(prec))
    for lo, hi in _chunks(len(prec), from_end):
        out[lo:hi] = np.maximum(np.maximum.accumulate(prec[lo:hi][::-1])[::-1], 0.0)
    return out


# ------------------------------------------------------------------ generator
def make_case(N, M, G, C, seed, first_image=0, img_h=600, img_w=1000, counts=None, shuffle=False, levels=16,
              max_gt=None, gt_classes=None):
    """One batch of detections and ground truth.  Per image: a random number of
    valid gt in random slots (the padding is interleaved), about a quarter of
    them difficult; about 70 % of the detections are copies of a gt jittered by
    about 6 % of its size, 15 % of those with a wrong class; the rest lie
    anywhere.  Scores are multiples of 1/levels, so ties are common.  Without
    ``shuffle`` the slots are ordered by class, then descending score, as
    ops.detect emits them.  Slots at or past the count hold the garbage the
    contract names.  Returns a dict of arrays."""
    db = np.full((N, M, 4), GARBAGE_BOX, np.float32)
    dl = np.full((N, M), GARBAGE_LABEL, np.int32)
    ds = np.full((N, M), GARBAGE_SCORE, np.float32)
    dc = np.zeros(N, np.int32)
    gb = -np.ones((N, G, 4))
    gl = -np.ones((N, G), np.int32)
    gd = np.zeros((N, G), np.uint8)
    for n in range(N):
        r = synth.rng_for(seed, first_image + n, 7)
        top = G if max_gt is None else min(G, max_gt)
        nv = int(r.integers(min(1, top), top + 1))
        slots = np.sort(r.choice(G, nv, replace=False)) if nv else np.zeros(0, np.int64)
        for g in slots:
            h, w = r.uniform(0.08, 0.5) * img_h, r.uniform(0.08, 0.5) * img_w
            y, x = r.uniform(0, img_h - h), r.uniform(0, img_w - w)
            gb[n, g] = np.around([y, x, y + h, x + w])
            gl[n, g] = int(r.choice(gt_classes)) if gt_classes is not None else int(r.integers(1, C))
            gd[n, g] = r.uniform() < 0.25
        k = int(r.integers(M // 2, M + 1)) if counts is None else int(counts[n])
        kk = min(max(k, 0), M)
        boxes = np.empty((kk, 4))
        labels = np.empty(kk, np.int32)
        for s in range(kk):
            if nv and r.uniform() < 0.7:
                g = int(r.choice(slots))
                b = gb[n, g]
                size = np.array([b[2] - b[0], b[3] - b[1], b[2] - b[0], b[3] - b[1]])
                boxes[s] = b + 0.06 * size * r.standard_normal(4)
                labels[s] = gl[n, g]
                if C > 2 and r.uniform() < 0.15:
                    labels[s] = 1 + (gl[n, g] - 1 + int(r.integers(1, C - 1))) % (C - 1)
            else:
                y = np.sort(r.uniform(0, img_h, 2))
                x = np.sort(r.uniform(0, img_w, 2))
                boxes[s] = [y[0], x[0], y[1] + 8, x[1] + 8]
                labels[s] = int(r.integers(1, C))
        scores = np.round(r.uniform(0, 1, kk) * levels) / levels
        order = r.permutation(kk) if shuffle else np.lexsort((-scores, labels))
        db[n, :kk] = boxes[order]
        dl[n, :kk] = labels[order]
        ds[n, :kk] = scores[order]
        dc[n] = k
    return dict(det_boxes=db, det_labels=dl, det_scores=ds, det_count=dc, gt_boxes=gb, gt_labels=gl,
                gt_difficult=gd)


ARGS = ("det_boxes", "det_labels", "det_scores", "det_count", "gt_boxes", "gt_labels", "gt_difficult")


def args(case):
    return [case[k] for k in ARGS]


def concat(cases):
    return {k: np.concatenate([c[k] for c in cases]) for k in ARGS}


# ------------------------------------------------ hand-derived known answers
def _case(det, gt, M=None, G=None):
    """det: [(box, label, score)], gt: [(box, label, difficult)] -> one image."""
    M, G = M or len(det), G or len(gt)
    c = dict(det_boxes=np.full((1, M, 4), GARBAGE_BOX, np.float32), det_labels=np.full((1, M), GARBAGE_LABEL, np.int32),
             det_scores=np.full((1, M), GARBAGE_SCORE, np.float32), det_count=np.array([len(det)], np.int32),
             gt_boxes=-np.ones((1, G, 4)), gt_labels=-np.ones((1, G), np.int32), gt_difficult=np.zeros((1, G), np.uint8))
    for i, (b, l, s) in enumerate(det):
        c["det_boxes"][0, i], c["det_labels"][0, i], c["det_scores"][0, i] = b, l, s
    for i, (b, l, d) in enumerate(gt):
        c["gt_boxes"][0, i], c["gt_labels"][0, i], c["gt_difficult"][0, i] = b, l, d
    return c


def known_answers():
    """name -> (case, C, plus_one, expected flags of the records)."""
    two_gt = [((10, 10, 110, 110), 1, 0), ((300, 300, 400, 420), 1, 0)]
    return {
        # flags in score order TP, FP, TP, FP: npos 2, area AP 5/6, 11-point AP 28/33; class 2 has no gt
        "tp_fp_tp_fp": (_case([((12, 9, 111, 108), 1, 0.9), ((150, 600, 250, 700), 1, 0.8),
                               ((298, 305, 405, 418), 1, 0.7), ((8, 12, 108, 112), 1, 0.6)], two_gt), 3, 1,
                        [1, 0, 1, 0]),
        # IoU exactly at the threshold is not over it
        "at_threshold": (_case([((0, 0, 10, 20), 1, 0.5)], [((0, 0, 10, 10), 1, 0)]), 2, 0, [0]),
        # two identical gt: both detections take gt 0, the second finds it taken (the devkit's behaviour)
        "identical_gt": (_case([((20, 20, 80, 90), 1, 0.9), ((20, 20, 80, 90), 1, 0.8)],
                               [((20, 20, 80, 90), 1, 0), ((20, 20, 80, 90), 1, 0)]), 2, 1, [1, 0]),
        # zero area on zero area: 0 / 0, a NaN IoU is no overlap
        "zero_area": (_case([((5, 5, 5, 5), 1, 0.5)], [((5, 5, 5, 5), 1, 0)]), 2, 0, [0]),
    }
