"""Named cases of the PASCAL VOC evaluation (DESIGN.md §3 "Evaluation"), shared by
test_eval_cases_cpu.py and test_gpu_eval_cases.py: the smallest shapes at which each chunk, tile,
scan and walk edge of ``csrc/eval.hip`` / ``csrc/eval_common.h`` can still go wrong.

Two kinds.  A ``BatchCase`` is a list of updates that go through ``eval_update`` (and then
``eval_ap``); a ``StateCase`` is an accumulator written by hand that goes through ``eval_ap`` alone.
Every case carries the launch plan it expects (``plan``: what ``frcnn_eval_plan`` must answer for
its shape, from the port below) and a ``check(case, ref)`` that asserts the property its name
promises on ``eval_ref`` alone, so a case cannot silently stop testing what it is named for.
References are computed once per (case, mistake) and never modified.

``CAUGHT_BY`` names, for each mistake planted in ``eval_ref``, the case that must tell it apart."""
import numpy as np

import eval_ref as ref

U = np.uint64
F = np.float32
NAN, INF = float("nan"), float("inf")

# ------------------------------------------------------------------ the plan
# A port of frcnn_eval_plan.  Not free copies: both test files compare plan() with the library's
# answer over a sweep of shapes, and every case compares its own plan before it runs.
THREADS = 256          # kEvThreads: images per count step, slots per match chunk, records per walk chunk
SORT_TILE = 4096       # kSortTile
SORT_BINS = 256        # kSortBins
SORT_PASSES = 5        # kSortPasses: one per key byte from bit 24 to bit 63
SORT_FIRST_BIT = 24
SCAN_THREADS = 1024    # kScanThreads
MAX_N, MAX_M, MAX_G, MAX_C, MAX_CAP = 1024, 1 << 20, 256, 128, 1 << 24   # the limits: the query refuses past them

PLAN_FIELDS = ("count_step", "count_steps", "match_chunk", "match_chunks", "sort_tile", "sort_tiles", "sort_passes",
               "scan_len", "scan_share", "walk_chunk")


def plan(N, M, n_records):
    tiles = (n_records + SORT_TILE - 1) // SORT_TILE
    scan = SORT_BINS * tiles
    return dict(count_step=THREADS, count_steps=(N + THREADS - 1) // THREADS, match_chunk=THREADS,
                match_chunks=(M + THREADS - 1) // THREADS, sort_tile=SORT_TILE, sort_tiles=tiles,
                sort_passes=SORT_PASSES, scan_len=scan, scan_share=(scan + SCAN_THREADS - 1) // SCAN_THREADS,
                walk_chunk=THREADS)


CHUNK = plan(1, 1, 0)["match_chunk"]      # 256: the edge the slot, image and segment cases sit on
TILE = plan(1, 1, 0)["sort_tile"]         # 4096
assert ref.CHUNK == CHUNK


class _Case:
    def __repr__(self):
        return self.name


# ------------------------------------------------------------------- batches
FAR = (1000.0, 1000.0, 1050.0, 1050.0)    # a detection that overlaps no gt of any case


def image(det, gt, M=None, G=None):
    """det: [(box, label, score)], gt: [(box, label, difficult)] -> one image (eval_ref._case)."""
    return ref._case(det, gt, M, G)


def stack(images, counts=None):
    c = ref.concat(images)
    if counts is not None:
        c["det_count"] = np.asarray(counts, np.int32)
    return c


class BatchCase(_Case):
    """``updates``: [(batch dict, keyword arguments of the update)]; ``cap`` defaults to the slots of all
    updates.  ``n_records`` is the reference's hdr[0] after the last update."""

    def __init__(self, name, C, updates, check, cap=None):
        self.name, self.C, self.check = name, C, check
        self.updates = [(b, dict(kw)) for b, kw in updates]
        self.cap = cap or sum(b["det_labels"].size for b, _ in self.updates)
        self._ref = {}

    def reference(self, mistake=None):
        if mistake not in self._ref:
            st = ref.State(self.C, self.cap)
            for b, kw in self.updates:
                a = ref.args(b)
                if kw.get("no_difficult"):
                    a[6] = None
                st.update(*a, iou_thresh=kw.get("iou_thresh", 0.5), plus_one=kw.get("plus_one", 1), mistake=mistake)
            self._ref[mistake] = st
        return self._ref[mistake]

    @property
    def n_records(self):
        return int(self.reference().hdr[0])

    @property
    def plans(self):
        """One per update, each with the records held after it, as eval_ap would then sort them."""
        return [plan(*s) for s in self.shapes()]

    def shapes(self):
        """(N, M, records held after the update) per update."""
        out, n = [], 0
        for b, _ in self.updates:
            N, M = b["det_labels"].shape
            k = int(np.clip(b["det_count"], 0, M).sum())
            n = n + k if n + k <= self.cap else n
            out.append((N, M, n))
        return out


def flags(st):
    return st.rec_flag[:int(st.hdr[0])].tolist()


# ---- images_257 / images_1024
COUNT_CYCLE = (-1, 0, 1, 2, 5)


def _many_images(N, M, counts, seed):
    r = np.random.default_rng(seed)
    gt = ((10, 10, 110, 110), 1, 0)
    imgs = []
    for n in range(N):
        det = [((10, 10, 110, 110) if r.random() < 0.5 else FAR, 1, float(F(r.integers(1, 9) / 8.0))) for _ in range(M)]
        imgs.append(image(det, [gt], M=M, G=1))
    return stack(imgs, counts)


def _images_257():
    N, M = CHUNK + 1, 2
    counts = [COUNT_CYCLE[(n + 3) % 5] for n in range(N)]
    return BatchCase("images_257", 2, [(_many_images(N, M, counts, 1), {})], check_images_257, cap=N * M + 64)


def check_images_257(case, st):
    b = case.updates[0][0]
    N, M = b["det_labels"].shape
    assert N == CHUNK + 1 and case.plans[0]["count_steps"] == 2
    raw = b["det_count"].astype(np.int64)
    assert set(raw.tolist()) == set(COUNT_CYCLE) and raw.min() < 0 and raw.max() > M
    ks = np.clip(raw, 0, M)
    prefix = int(ks[:CHUNK].sum())
    assert ks[CHUNK] > 0 and raw[CHUNK] > M              # the image of the second step has records, and a clamped count
    assert prefix % CHUNK and prefix % M and prefix != int(raw[:CHUNK].sum())
    first = int(np.nonzero(st.rec_image[:int(st.hdr[0])] == CHUNK)[0][0])
    assert first == prefix and st.hdr[0] == prefix + ks[CHUNK] and st.hdr[1] == N
    assert (st.rec_key[:int(st.hdr[0])] & U(0xFFFFFF)).tolist() == list(range(int(st.hdr[0])))


def _images_1024():
    N = MAX_N
    counts = [(n + 2) % 3 - 1 for n in range(N)]         # 1, -1, 0, ...: clamped to 1, 0, 0
    return BatchCase("images_1024", 2, [(_many_images(N, 1, counts, 2), {})], check_images_1024)


def check_images_1024(case, st):
    assert case.plans[0]["count_steps"] == MAX_N // CHUNK == 4
    ks = np.clip(case.updates[0][0]["det_count"], 0, 1)
    n = int(st.hdr[0])
    assert n == ks.sum() and 0 < n < MAX_N and st.hdr[1] == MAX_N
    assert np.array_equal(st.rec_image[:n], np.nonzero(ks)[0])          # every step's images, in order
    assert ks[-1] == 1 and st.rec_image[n - 1] == MAX_N - 1 and {0, 1} <= set(flags(st))


# ---- slots_k
GT0, GT1 = (10, 10, 110, 110), (300, 300, 400, 420)


def _slot_roles(k):
    """(a, b): gt 0's two claimants of equal score; (lo, hi): gt 1's claimant of the lower score in
    chunk 0 and the one of the higher score as late as the slots allow."""
    a, b = (CHUNK - 1, CHUNK) if k > CHUNK else (k - 2, k - 1)
    hi = k - 1 if k - 1 > b else a - 1
    return a, b, 0, hi


def _slots(k):
    a, b, lo, hi = _slot_roles(k)
    det = [(FAR, 1, float(F(0.9 - 0.001 * s))) for s in range(k)]       # descending, all distinct
    det[a], det[b] = (GT0, 1, 0.5), (GT0, 1, 0.5)
    det[lo], det[hi] = (GT1, 1, 0.25), (GT1, 1, 0.75)
    return BatchCase("slots_%d" % k, 2, [(image(det, [(GT0, 1, 0), (GT1, 1, 0)]), {})], check_slots)


def check_slots(case, st):
    b = case.updates[0][0]
    k = int(b["det_count"][0])
    a, bb, lo, hi = _slot_roles(k)
    assert case.plans[0]["match_chunks"] == (k + CHUNK - 1) // CHUNK and len({a, bb, lo, hi}) == 4
    best, fl, sc = st.best[0], flags(st), b["det_scores"][0]
    assert best[a] == best[bb] == 0 and sc[a] == sc[bb] and (fl[a], fl[bb]) == (1, 0)      # the tie: by slot
    assert best[lo] == best[hi] == 1 and sc[lo] < sc[hi] and lo < hi and (fl[lo], fl[hi]) == (0, 1)
    assert sum(fl) == 2 and (best >= 0).sum() == 4
    if k > CHUNK:
        assert a // CHUNK == 0 and bb // CHUNK == 1                     # the tie straddles the chunk boundary
    if k > CHUNK + 1:
        assert lo // CHUNK == 0 and hi // CHUNK == (k - 1) // CHUNK > 0  # the winner sits in the last chunk


# ---- scores_special
SPECIAL = (0.5, INF, NAN, -0.0, 0.0, -1.0, -INF, 1e-45)


def _scores_special():
    det = [(GT0, 1, s) for s in SPECIAL] + [(GT1, 1, -0.0), (GT1, 1, 0.0)]
    return BatchCase("scores_special", 2, [(image(det, [(GT0, 1, 0), (GT1, 1, 0)]), {})], check_scores_special)


def check_scores_special(case, st):
    sc = case.updates[0][0]["det_scores"][0]
    assert np.isnan(sc[2]) and np.signbit(sc[3]) and sc[3] == 0 and not np.signbit(sc[4]) and 0 < sc[7] < 1.2e-38
    order = ref.desc_order(sc)
    # NaN, +inf, 0.5, the denormal, the four zeros by slot, -1, -inf
    assert order == [2, 1, 0, 7, 3, 4, 8, 9, 5, 6]
    fl = flags(st)
    assert [s for s in range(10) if fl[s] == 1] == [2, 8]               # NaN takes gt 0; the slot decides gt 1
    assert st.best[0].tolist() == [0] * 8 + [1] * 2
    sk = st.ap()[2]
    assert (sk & U(0xFFFFFF)).tolist() == order                         # eval_ap's order is that order
    key = ref.desc_score_key(sc)
    assert key[2] == 0 and key[3] == key[4] == key[8] == key[9] and len(set(key.tolist())) == 7


# ---- best_gt_tie_first
def _best_gt_tie_first():
    d = (0, 20, 100, 120)
    gts = [((0, 0, 100, 100), 1, 0), ((0, 40, 100, 140), 1, 0)]        # mirrored about the detection's centre line
    # the third detection sits on gt 1 alone: it shows in the flags which of the two gt the first one took
    det = [(d, 1, 0.9), (d, 1, 0.8), (gts[1][0], 1, 0.7)]
    return BatchCase("best_gt_tie_first", 2, [(image(det, gts), {})], check_best_gt_tie)


def check_best_gt_tie(case, st):
    b = case.updates[0][0]
    ov = ref.iou(b["det_boxes"][0, 0], b["gt_boxes"][0])
    assert ov[0] == ov[1] > 0.5 and not np.array_equal(b["gt_boxes"][0, 0], b["gt_boxes"][0, 1])
    assert ref.iou(b["det_boxes"][0, 2], b["gt_boxes"][0])[0] < 0.5
    # the second detection is FP although gt 1 is free; the third then finds gt 1 free
    assert st.best[0].tolist() == [0, 0, 1] and flags(st) == [1, 0, 1] and st.hdr[5] == 2


# ---- difficult / difficult_null
def _difficult_batch():
    easy, hard = (0, 0, 100, 100), (0, 10, 100, 110)
    gts = [((300, 300, 400, 400), 1, 1),     # gt 0, difficult: two detections sit on it
           (hard, 1, 1),                     # gt 1, difficult: the argmax of the third detection
           (easy, 1, 0)]                     # gt 2: also over the threshold for it, but not its argmax
    det = [((300, 300, 400, 400), 1, 0.9), ((300, 300, 400, 400), 1, 0.8), ((0, 8, 100, 108), 1, 0.7)]
    return image(det, gts)


def _difficult(null):
    return BatchCase("difficult_null" if null else "difficult", 2, [(_difficult_batch(), dict(no_difficult=null))],
                     check_difficult_null if null else check_difficult)


def _difficult_ious(case):
    b = case.updates[0][0]
    return ref.iou(b["det_boxes"][0, 2], b["gt_boxes"][0])


def check_difficult(case, st):
    ov = _difficult_ious(case)
    assert ov[1] > ov[2] > 0.5 and ov[0] == 0
    assert st.best[0].tolist() == [0, 0, 1] and flags(st) == [-1, -1, -1] and st.hdr[5] == 1


def check_difficult_null(case, st):
    assert st.best[0].tolist() == [0, 0, 1] and flags(st) == [1, 0, 1] and st.hdr[5] == 3
    assert case.updates[0][0]["gt_difficult"].sum() == 2              # the same inputs: only the pointer is null


# ---- thresholds
def _thresholds():
    at75 = image([((0, 0, 10, 15), 1, 0.5)], [((0, 0, 10, 20), 1, 0)])
    apart = image([((0, 0, 10, 10), 1, 0.5)], [((50, 50, 60, 60), 1, 0)])
    nan_and_zero = image([((0, 0, 10, 10), 1, 0.5), ((5, 5, 5, 5), 2, 0.4)],
                         [((50, 50, 60, 60), 1, 0), ((5, 5, 5, 5), 2, 0)])
    same = image([((3, 4, 30, 40), 1, 0.5)], [((3, 4, 30, 40), 1, 0)])
    runs = [(at75, 0.75), (apart, 0.0), (nan_and_zero, -1.0), (same, 1.0)]
    return BatchCase("thresholds", 3, [(b, dict(iou_thresh=t, plus_one=0)) for b, t in runs], check_thresholds)


def check_thresholds(case, st):
    (a, _), (b, _), (c, _), (d, _) = case.updates
    assert ref.iou(a["det_boxes"][0, 0], a["gt_boxes"][0], 0)[0] == 0.75
    assert ref.iou(b["det_boxes"][0, 0], b["gt_boxes"][0], 0)[0] == 0.0
    assert ref.iou(c["det_boxes"][0, 0], c["gt_boxes"][0, :1], 0)[0] == 0.0
    assert np.isnan(ref.iou(c["det_boxes"][0, 1], c["gt_boxes"][0, 1:], 0)[0])
    assert ref.iou(d["det_boxes"][0, 0], d["gt_boxes"][0], 0)[0] == 1.0
    # at 0.75: not over it; at 0: not over it; at -1: IoU 0 matches, NaN does not; at 1: not over it
    assert flags(st) == [0, 0, 1, 0, 0]
    assert [x.tolist() for x in st.best] == [[-1], [-1], [0, -1], [-1]]


# ---- plus_one_widens
P24 = float(2 ** 24)


def _plus_one_widens():
    b = image([((0, 0, P24, P24), 1, 0.5)], [((0, 0, P24, 2 * P24), 1, 0)])
    return BatchCase("plus_one_widens", 2, [(b, dict(plus_one=1)), (b, dict(plus_one=0))], check_plus_one_widens)


def check_plus_one_widens(case, st):
    b = case.updates[0][0]
    d, g = b["det_boxes"][0, 0], b["gt_boxes"][0]
    assert d[2] == P24 and F(d[2] + F(1)) == d[2] and float(d[2]) + 1.0 != float(d[2])   # lost in fp32, kept in fp64
    on, off, on32 = ref.iou(d, g, 1)[0], ref.iou(d, g, 0)[0], ref.iou(d, g, 1, "plus_one_in_fp32")[0]
    assert on > 0.5 and off == 0.5 and on32 < 0.5
    assert flags(st) == [1, 0]                            # with the +1 a TP, without it exactly at the threshold
    assert flags(case.reference("plus_one_in_fp32")) == [0, 0]


# ---- labels_at_limits / classes_128 / gt_256_last_wins
def _labels_at_limits(C=5):
    box = [(10 + 200 * i, 10, 110 + 200 * i, 110) for i in range(4)]
    det = [(box[i], lab, 0.9 - 0.1 * i) for i, lab in enumerate((-1, 0, C - 1, C))]
    gts = [(box[i], lab, 0) for i, lab in enumerate((-5, 0, C - 1, C))]
    return BatchCase("labels_at_limits", C, [(image(det, gts), {})], check_labels_at_limits)


def check_labels_at_limits(case, st):
    C, b = case.C, case.updates[0][0]
    assert b["det_labels"][0].tolist() == [-1, 0, C - 1, C] and b["gt_labels"][0].tolist() == [-5, 0, C - 1, C]
    assert flags(st) == [-1, -1, 1, -1]
    assert (st.rec_key[:4] >> U(56)).tolist() == [0, 0, C - 1, 0]       # class-0 records, all ignored
    assert st.hdr[4:].tolist() == [0] * (C - 1) + [1]                   # npos from the one valid row


def _classes_128():
    C = MAX_C
    cls = (1, 64, C - 1)
    box = [(10 + 200 * i, 10, 110 + 200 * i, 110) for i in range(3)]
    det = [(box[i], c, 0.9) for i, c in enumerate(cls)] + [(box[0], C - 1, 0.8), (FAR, 64, 0.7), (box[2], C - 1, 0.6)]
    gts = [(box[i], c, 0) for i, c in enumerate(cls)]
    return BatchCase("classes_128", C, [(image(det, gts), {})], check_classes_128)


def check_classes_128(case, st):
    C = case.C
    assert C == MAX_C and flags(st) == [1, 1, 1, 0, 0, 0]
    assert np.nonzero(st.hdr[4:])[0].tolist() == [1, 64, C - 1]
    ap, mean, sk, nper = st.ap()
    assert np.nonzero(~np.isnan(ap))[0].tolist() == [1, 64, C - 1] and ap[1] == 1 and ap[64] == 1 and ap[C - 1] == 1
    assert int(sk[-1] >> U(56)) == C - 1 and nper[C - 1] == 3 and ((C - 1 + 1) << 56) == 1 << 63


def _gt_256_last_wins():
    G = MAX_G
    gts = [((0, 0, 100, 100 + (G - 1 - j)), 1, 0) for j in range(G)]    # the overlap with the detection grows with j
    det = [((0, 0, 100, 100), 1, 0.9)]
    return BatchCase("gt_256_last_wins", 2, [(image(det, gts), {})], check_gt_256_last_wins)


def check_gt_256_last_wins(case, st):
    b = case.updates[0][0]
    ov = ref.iou(b["det_boxes"][0, 0], b["gt_boxes"][0])
    assert len(ov) == MAX_G and (np.diff(ov) > 0).all() and ov[0] > 0.25
    assert st.best[0].tolist() == [MAX_G - 1] and flags(st) == [1] and st.hdr[5] == MAX_G


# ---- exact_fit_then_drop
def _exact_fit_then_drop():
    one = (GT0, 1, 0.9)
    b1 = stack([image([one, (FAR, 1, 0.5), (FAR, 1, 0.4)], [(GT0, 1, 0)]), image([one] * 3, [(GT0, 1, 0)])], [3, 2])
    b2 = stack([image([one, (FAR, 1, 0.5)], [(GT0, 1, 0)])], [2])
    b3 = stack([image([one], [(GT0, 1, 0)])], [1])
    return BatchCase("exact_fit_then_drop", 2, [(b1, {}), (b2, {}), (b3, {})], check_exact_fit_then_drop, cap=7)


def check_exact_fit_then_drop(case, st):
    assert [s[2] for s in case.shapes()] == [5, 7, 7] and case.cap == 7
    assert st.hdr[:4].tolist() == [7, 3, 1, 0] and st.hdr[5] == 3      # the dropped batch's gt is not counted either
    assert flags(st) == [1, 0, 0, 1, 0, 1, 0] and st.rec_image[:7].tolist() == [0, 0, 0, 1, 1, 2, 2]


BATCH_CASES = [_images_257(), _images_1024()] + [_slots(k) for k in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)] + [
    _scores_special(), _best_gt_tie_first(), _difficult(False), _difficult(True), _thresholds(), _plus_one_widens(),
    _labels_at_limits(), _classes_128(), _gt_256_last_wins(), _exact_fit_then_drop()]
BATCH_BY_NAME = {c.name: c for c in BATCH_CASES}


# -------------------------------------------------------------------- states
def make_keys(cls, skey, n=None):
    """class << 56 | score key << 24 | position."""
    cls, skey = np.asarray(cls).astype(U), np.asarray(skey).astype(U)
    n = len(cls) if n is None else n
    return (cls << U(56)) | (skey << U(SORT_FIRST_BIT)) | np.arange(n, dtype=U)


class StateCase(_Case):
    """An accumulator written by hand: ``keys`` uint64 [held] (record index = position), ``flags``
    int8 [held], ``npos`` [C]; ``n_records`` (default: all held) is what eval_ap is given."""

    def __init__(self, name, C, keys, flags, npos, check, n_records=None):
        self.name, self.C, self.check = name, C, check
        self.keys = np.ascontiguousarray(keys, U)
        self.flags = np.ascontiguousarray(flags, np.int8)
        self.held = len(self.keys)
        assert len(self.flags) == self.held and len(npos) == C and npos[0] == 0
        assert np.array_equal(self.keys & U(0xFFFFFF), np.arange(self.held, dtype=U)) and not (self.keys >> U(63)).any()
        self.npos = np.asarray(npos, np.int64)
        self.n_records = self.held if n_records is None else n_records
        self.cap = max(self.held, 1)
        self.plan = plan(1, 1, self.n_records)
        self._ref = {}

    def state(self):
        st = ref.State(self.C, self.cap)
        st.rec_key[:self.held], st.rec_flag[:self.held] = self.keys, self.flags
        st.hdr[0], st.hdr[1] = self.held, 1
        st.hdr[4:] = self.npos
        return st

    def reference(self, mistake=None):
        """{use_07: (ap, map, sorted keys, records per class)}."""
        if mistake not in self._ref:
            st = self.state()
            self._ref[mistake] = {m: st.ap(use_07_metric=m, mistake=mistake, n_records=self.n_records)
                                  for m in (True, False)}
        return self._ref[mistake]


def precision(flags):
    f = np.asarray(flags)
    tp, fp = np.cumsum(f == 1), np.cumsum(f == 0)
    return tp / np.maximum(tp + fp, 1).astype(np.float64)


def _sorted_classes(out):
    return (out[False][2] >> U(56)).astype(np.int64)


# ---- sort_n_* / sort_tiles_*
def _sort_n(name, n, tiles, share):
    r = np.random.default_rng(n)
    C = 4
    score = (r.integers(0, 4, n) / 4.0).astype(F)
    keys = make_keys(r.integers(1, C, n), ref.desc_score_key(score))
    fl = r.integers(-1, 2, n)

    def check(case, out):
        assert case.plan["sort_tiles"] == tiles and case.plan["scan_share"] == share
        assert case.plan["scan_len"] == tiles * SORT_BINS
        sk = out[False][2]
        assert len(sk) == n and (np.diff(sk.astype(np.int64)) > 0).all()
        if n > 1:
            assert not np.array_equal(sk, case.keys)      # the input is not already in order
    return StateCase(name, C, keys, fl, [0, 5 * n + 1, 7, n // 3 + 1], check)


SORT_N = [(1, 1), (CHUNK - 1, 1), (CHUNK, 1), (CHUNK + 1, 1), (TILE - 1, 1), (TILE, 1), (TILE + 1, 2), (2 * TILE, 2),
          (2 * TILE + 1, 3)]
# the scan's share per thread: 1 with idle threads up to 3 tiles, 1 exactly full at 4, 2 with an empty tail at 5
SCAN_FULL_TILES = SCAN_THREADS // SORT_BINS


def _sort_cases():
    out = [_sort_n("sort_n_%d" % n, n, t, 1) for n, t in SORT_N]
    out.append(_sort_n("sort_tiles_4", SCAN_FULL_TILES * TILE, SCAN_FULL_TILES, 1))
    out.append(_sort_n("sort_tiles_5", SCAN_FULL_TILES * TILE + 1, SCAN_FULL_TILES + 1, 2))
    return out


def check_scan_shares(cases):
    """Asserted once by the CPU test: the three regimes of the scan's share are all present."""
    by = {c.name: c.plan for c in cases}
    assert all(by["sort_n_%d" % n]["scan_len"] < SCAN_THREADS for n, _ in SORT_N)          # idle threads
    assert by["sort_tiles_4"]["scan_len"] == SCAN_THREADS                                   # exactly full
    p5 = by["sort_tiles_5"]
    assert p5["scan_share"] == 2 and (p5["scan_len"] + 1) // 2 < SCAN_THREADS              # an empty tail of threads


def _sort_one_digit():
    n = 700
    r = np.random.default_rng(700)
    keys = make_keys(np.ones(n), np.full(n, ref.desc_score_key(F(0.5))))

    def check(case, out):
        assert len(np.unique(case.keys >> U(SORT_FIRST_BIT))) == 1 and n > 2 * CHUNK
        assert np.array_equal(out[False][2], case.keys)   # the insertion order alone
    return StateCase("sort_one_digit", 2, keys, r.integers(-1, 2, n), [0, 300], check)


def _sort_byte(p):
    n = 600
    r = np.random.default_rng(600 + p)
    shift = SORT_FIRST_BIT + 8 * p
    top = 128 if p == SORT_PASSES - 1 else 256            # the class byte: bit 63 is never set
    digit = r.integers(0, top, n).astype(U)
    base = (U(1) << U(56)) | (U(0x3C5A963C) << U(SORT_FIRST_BIT))
    keys = ((base & ~(U(0xFF) << U(shift))) | (digit << U(shift))) | np.arange(n, dtype=U)
    C = MAX_C if p == SORT_PASSES - 1 else 2

    def check(case, out):
        diff = np.bitwise_or.reduce(case.keys ^ case.keys[0]) >> U(SORT_FIRST_BIT)
        assert diff and (diff & ~(U(0xFF) << U(8 * p))) == 0          # the keys differ in that byte only
        sk = out[False][2]
        d = ((sk >> U(shift)) & U(0xFF)).astype(np.int64)
        assert (np.diff(d) >= 0).all() and len(np.unique(d)) > 64 and (np.bincount(d) > 1).any()
        assert d.min() == 0 and d.max() == top - 1        # both ends of the byte; the class byte ends at MAX_C - 1
        same = np.diff(d) == 0
        assert (np.diff((sk & U(0xFFFFFF)).astype(np.int64))[same] > 0).all()           # stable within a digit
    npos = [0] + [3] * (C - 1)
    return StateCase("sort_byte_%d" % p, C, keys, r.integers(-1, 2, n), npos, check)


# ---- segment_*
def _segment(name, fl, npos=None, check=None):
    fl = np.asarray(fl, np.int8)
    n = len(fl)
    skey = ref.desc_score_key(np.linspace(1.0, 0.0, max(n, 1), dtype=F)[:n])   # distinct scores, already descending
    npos = int((fl == 1).sum()) + 3 if npos is None else npos
    return StateCase(name, 2, make_keys(np.ones(n), skey), fl, [0, npos], check or (lambda case, out: None))


def rising(n):
    """60 % FP records, then TP records: the precision is largest at the last record."""
    nfp = (6 * n) // 10
    return [0] * nfp + [1] * (n - nfp)


def check_rising(case, out):
    n = case.held
    p = precision(case.flags)
    assert p[-1] > p[:-1].max() and case.flags[0] == 0 and case.flags[-1] == 1
    # the envelope at record 0 is the precision of the last record: the suffix maximum crosses every chunk
    assert np.maximum.accumulate(p[::-1])[::-1][0] == p[-1]
    assert case.n_records == n and 0 < out[False][0][1] < 1 and 0 < out[True][0][1] < 1


def check_single_tp(case, out):
    (pos,) = np.nonzero(case.flags == 1)[0]
    assert (case.flags == 0).sum() == case.held - 1
    want = (1.0 / case.npos[1]) * (1.0 / (pos + 1))
    assert out[False][0][1] == want and out[True][0][1] > 0


def check_early_tp(case, out):
    p = precision(case.flags)
    assert case.flags[5] == 1 and p[5] < p[-1] and p[-1] == p.max()
    if case.held > 2 * CHUNK:                             # walked in a later chunk than the peak: a carried maximum
        assert (case.held - 1 - 5) // CHUNK >= 1


def _segment_cases():
    out = [_segment("segment_0", [], npos=4, check=lambda case, o: _eq(o, 0.0)),
           _segment("segment_1_tp", [1], npos=2, check=lambda case, o: _eq(o, 0.5, 6 / 11 * 1.0)),
           _segment("segment_1_fp", [0], npos=2, check=lambda case, o: _eq(o, 0.0))]
    for n in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
        out.append(_segment("segment_%d" % n, rising(n), check=check_rising))
        early = rising(n)
        early[5] = 1
        out.append(_segment("segment_%d_early_tp" % n, early, check=check_early_tp))
        for pos in (CHUNK - 1, CHUNK):
            if pos < n:
                fl = [0] * n
                fl[pos] = 1
                out.append(_segment("segment_%d_tp%d" % (n, pos), fl, check=check_single_tp))
    return out


def _eq(out, area, eleven=None):
    eleven = area if eleven is None else eleven
    assert out[False][0][1] == area and out[False][1] == area, out[False][:2]
    assert abs(out[True][0][1] - eleven) <= 11 * 2.0 ** -53 and out[True][1] == out[True][0][1], out[True][:2]


def _segment_all_ignored():
    return _segment("segment_all_ignored", [-1] * (CHUNK + 44), npos=4, check=lambda case, o: _eq(o, 0.0))


def _segment_ignored_first():
    lead = CHUNK + 4

    def check(case, out):
        assert (case.flags[:lead] == -1).all() and case.flags[lead:].tolist() == [1, 0, 1, 0]
        p = precision(case.flags)
        assert (p[:lead] == 0).all() and p[lead] == 1                  # 0 / max(0, 1), not 0 / 0
        _eq(out, 1 / 4 * 1.0 + 1 / 4 * (2 / 3), (3 * 1.0 + 3 * (2 / 3)) / 11)
    return _segment("segment_ignored_first", [-1] * lead + [1, 0, 1, 0], npos=4, check=check)


def _segment_across_tile():
    lo, hi = TILE - 6, TILE + 5                           # class 2 in the sorted positions 4090..4100
    sizes = {1: lo, 2: hi - lo, 3: 20}
    r = np.random.default_rng(4090)
    cls = r.permutation(np.repeat(list(sizes), list(sizes.values())))
    n = len(cls)
    score = (r.integers(0, 64, n) / 64.0).astype(F)
    fl = r.integers(0, 2, n)

    def check(case, out):
        kc = _sorted_classes(out)
        assert np.nonzero(kc == 2)[0].tolist() == list(range(TILE - 6, TILE + 5)) and case.plan["sort_tiles"] == 2
        assert 0 < out[False][0][2] < 1
    return StateCase("segment_across_tile", 4, make_keys(cls, ref.desc_score_key(score)), fl, [0, 5000, 9, 30], check)


def _class_zero_ahead():
    r = np.random.default_rng(300)
    cls = r.permutation(np.array([0] * 300 + [1] * 10))
    n = len(cls)
    score = (r.integers(0, 8, n) / 8.0).astype(F)
    fl = np.where(cls == 0, r.integers(-1, 2, n), r.integers(0, 2, n))  # class 0's flags must not matter

    def check(case, out):
        kc = _sorted_classes(out)
        assert (kc[:300] == 0).all() and (kc[300:] == 1).all() and (case.flags[case.keys >> U(56) == 0] == 1).any()
        assert np.isnan(out[False][0][0]) and 0 < out[False][0][1] <= 1 and out[False][1] == out[False][0][1]
    return StateCase("class_zero_ahead", 2, make_keys(cls, ref.desc_score_key(score)), fl, [0, 6], check)


def _classes_mixed():
    cls = [1, 3, 1, 3, 1, 3]
    fl = [1, 1, 0, 0, 1, 1]
    score = np.array([0.9, 0.9, 0.8, 0.8, 0.7, 0.7], F)

    def check(case, out):
        for m in (True, False):
            ap, mean = out[m][0], out[m][1]
            assert ap[2] == 0.0 and np.isnan(ap[3]) and np.isnan(ap[4]) and np.isnan(ap[0]) and 0 < ap[1] < 1
            assert mean == (ap[1] + 0.0) / 2                # the 0.0 counts, the NaN do not
        assert out[False][3].tolist() == [0, 3, 0, 3, 0]
    return StateCase("classes_mixed", 5, make_keys(cls, ref.desc_score_key(score)), fl, [0, 3, 2, 0, 0], check)


def _all_nan():
    def check(case, out):
        for m in (True, False):
            assert np.isnan(out[m][0]).all() and np.isnan(out[m][1])
    score = np.array([0.9, 0.8, 0.7], F)
    return StateCase("all_nan", 3, make_keys([1, 2, 1], ref.desc_score_key(score)), [1, 1, 0], [0, 0, 0], check)


def _recall_at_tenths():
    fl = [1, 1, 1, 0, 1, 1, 1, 0, 1, 0, 1]             # tp reaches 3, 6 and 7 at precisions 1, 6/7 and 7/9

    def check(case, out):
        npos = 10
        assert case.npos[1] == npos
        for i in (3, 6, 7):
            assert i * 0.1 != i / 10 and i / npos == i / 10 and not i / npos >= i * 0.1
        tp = np.cumsum(case.flags == 1)
        p = precision(case.flags)
        at = [float(p[np.nonzero(tp == i)[0][0]]) for i in (3, 6, 7)]
        assert len(set(at)) == 3 and all(a > p[tp > i].max() for a, i in zip(at, (3, 6, 7)))
        wrong = case.reference("tenths_by_division")[True][0][1]
        assert out[True][0][1] < wrong                    # dividing reaches three recall levels the product does not
    return _segment("recall_at_tenths", fl, npos=10, check=check)


def _n_below_held():
    fl = [1, 0] * 10 + [0] * 5 + [1] * 15                # the records past n_records would raise the AP
    case = _segment("n_below_held", fl, npos=30)

    def check(case, out):
        assert case.n_records == 25 < case.held == 40
        whole = case.state().ap()[0][1]
        assert len(out[False][2]) == 25 and out[False][3][1] == 25 and out[False][0][1] < whole
    case.check, case.n_records = check, 25
    case.plan = plan(1, 1, 25)
    return case


STATE_CASES = (_sort_cases() + [_sort_one_digit()] + [_sort_byte(p) for p in range(SORT_PASSES)] + _segment_cases()
               + [_segment_all_ignored(), _segment_ignored_first(), _segment_across_tile(), _class_zero_ahead(),
                  _classes_mixed(), _all_nan(), _recall_at_tenths(), _n_below_held()])
STATE_BY_NAME = {c.name: c for c in STATE_CASES}
SORT_CASES = [c for c in STATE_CASES if c.name.startswith("sort_")]
BY_NAME = dict(BATCH_BY_NAME, **STATE_BY_NAME)

# mistake -> the case that must tell it apart (test_eval_cases_cpu.py asserts each pair)
CAUGHT_BY = {
    "non_strict_threshold": "thresholds",
    "last_gt_wins_tie": "best_gt_tie_first",
    "claim_by_slot": "slots_257",
    "nan_score_last": "scores_special",
    "neg_zero_below_zero": "scores_special",
    "difficult_consumes": "difficult",
    "difficult_in_npos": "difficult",
    "plus_one_in_fp32": "plus_one_widens",
    "invalid_label_is_fp": "labels_at_limits",
    "count_not_clamped": "images_257",
    "prefix_first_256_images": "images_257",
    "unstable_sort": "sort_one_digit",
    "envelope_restarts_each_chunk": "segment_257",
    "envelope_restarts_each_chunk_from_end": "segment_513_early_tp",
    "running_sum_restarts_each_chunk": "segment_513",
    "running_sum_restarts_each_chunk_from_end": "segment_513_tp255",
    "no_division_guard": "segment_ignored_first",
    "empty_class_is_nan": "classes_mixed",
    "tenths_by_division": "recall_at_tenths",
}


def observables(case, mistake=None):
    """Everything the GPU test compares, as a flat list of arrays: what a mistake must change to be caught."""
    if isinstance(case, BatchCase):
        st = case.reference(mistake)
        n = int(st.hdr[0])
        out = [st.hdr, st.rec_key[:n], st.rec_flag[:n], st.rec_image[:n]]
        for m in (True, False):
            ap, mean, sk, _ = st.ap(use_07_metric=m, mistake=mistake)
            out += [ap, np.array([mean]), sk]
        return out
    r = case.reference(mistake)
    return [x for m in (True, False) for x in (r[m][0], np.array([r[m][1]]), r[m][2])]


def tells_apart(case, mistake):
    a, b = observables(case), observables(case, mistake)
    return any(x.shape != y.shape or not np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in zip(a, b))
