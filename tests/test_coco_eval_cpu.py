"""CPU-side checks of the COCO-style evaluation: the C-ABI boundary (no compute,
no GPU), and the numpy restatement of the contract (tests/coco_eval_ref.py) on
closed forms, against the two-phase form a kernel uses, and on maxDets as a
prefix."""
import ctypes
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import coco_eval_ref as ref  # noqa: E402

SYMBOLS = ("frcnn_coco_eval_update", "frcnn_coco_eval_workspace_size", "frcnn_coco_eval_accumulate")


def test_header_and_library_have_coco_eval():
    from replication_faster_rcnn_amd import _lib
    raw = open(os.path.join(ROOT, "include", "frcnn_capi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES
    assert raw.count('DESIGN.md "COCO-style evaluation"') >= 1


def _update(lib, N=2, M=64, G=8, C=21, cap=1000, null=None):
    """frcnn_coco_eval_update with dummy non-null pointers: every case here is
    rejected before any pointer is used or any HIP call is made."""
    d = ctypes.c_void_p(0x1000)
    p = dict(det_boxes=d, det_labels=d, det_scores=d, det_count=d, gt_boxes=d, gt_labels=d, gt_crowd=d, tables=d,
             hdr=d, rec_key=d, rec_bits=d)
    if null:
        p[null] = None
    return lib.frcnn_coco_eval_update(N, M, G, C, cap, p["det_boxes"], p["det_labels"], p["det_scores"],
                                      p["det_count"], p["gt_boxes"], p["gt_labels"], p["gt_crowd"], p["tables"],
                                      p["hdr"], p["rec_key"], p["rec_bits"], None)


def _accumulate(lib, C=21, n=100, null=None, ws=None, ws_bytes=1 << 40):
    d = ctypes.c_void_p(0x1000)
    p = dict(hdr=d, rec_key=d, rec_bits=d, tables=d, precision=d, recall=d, stats=d, ap_per_class=d)
    if null:
        p[null] = None
    return lib.frcnn_coco_eval_accumulate(C, n, p["hdr"], p["rec_key"], p["rec_bits"], p["tables"], p["precision"],
                                          p["recall"], p["stats"], p["ap_per_class"], d if ws is None else ws,
                                          ws_bytes, None)


def test_coco_eval_argument_validation_without_gpu():
    from replication_faster_rcnn_amd import _lib
    lib = _lib.load(require_gpu=False)
    for kw, word in [(dict(C=1), b"C="), (dict(G=257), b"G="), (dict(cap=0), b"cap="), (dict(N=0), b"N="),
                     (dict(N=1025), b"N="), (dict(M=0), b"M="), (dict(M=(1 << 20) + 1), b"M="), (dict(G=-1), b"G="),
                     (dict(C=129), b"C="), (dict(cap=(1 << 24) + 1), b"cap="), (dict(null="det_scores"), b"det_scores"),
                     (dict(null="gt_boxes"), b"gt_boxes"), (dict(null="tables"), b"tables"),
                     (dict(null="rec_bits"), b"rec_bits"), (dict(null="hdr"), b"hdr")]:
        assert _update(lib, **kw) == -1, kw
        assert word in lib.frcnn_last_error() and b"frcnn_coco_eval_update" in lib.frcnn_last_error(), kw
    for kw, word in [(dict(C=1), b"C="), (dict(C=129), b"C="), (dict(n=-1), b"n_records"),
                     (dict(n=(1 << 24) + 1), b"n_records"), (dict(null="precision"), b"precision"),
                     (dict(null="hdr"), b"hdr"), (dict(null="rec_bits"), b"rec_bits")]:
        assert _accumulate(lib, **kw) == -1, kw
        assert word in lib.frcnn_last_error(), (kw, lib.frcnn_last_error())
    size = lib.frcnn_coco_eval_workspace_size
    for bad in [(1, 100), (129, 100), (21, 0), (21, (1 << 24) + 1)]:
        assert size(*bad) == 0, bad
    need = size(21, 100)
    assert need >= 2 * 100 * 8
    assert _accumulate(lib, ws_bytes=need - 1) == -3 and b"workspace" in lib.frcnn_last_error()
    assert _accumulate(lib, ws=ctypes.c_void_p(0)) == -3


# --------------------------------------------------------------- closed forms
BOX = (10, 20, 110, 220)          # area 20,000: large
FAR = (400, 500, 450, 600)


def _acc(case, C):
    return ref.run([case], C).accumulate()


def test_identical_detection():
    out = _acc(ref.images(([(BOX, 1, 0.9)], [(BOX, 1, 0)])), 2)
    a = [0, 3]                                       # the ranges the gt is in
    assert (out["precision"][:, :, 1, a, :] == 1 / (1 + 2.0 ** -52)).all()
    assert (out["recall"][:, 1, a, :] == 1).all()
    assert (out["precision"][:, :, 1, 1:3, :] == -1).all() and (out["recall"][:, 1, 1:3, :] == -1).all()
    assert (out["precision"][:, :, 0] == -1).all() and (out["recall"][:, 0] == -1).all()      # class 0
    assert abs(out["stats"][0] - 1) <= 1010 * 2.0 ** -52 and out["n_stats"][0] == 1010    # a sum of 1,010 terms
    assert out["stats"][3] == -1 and out["stats"][8] == 1


def test_fp_scored_above_tp():
    out = _acc(ref.images(([(FAR, 1, 0.9), (BOX, 1, 0.8)], [(BOX, 1, 0)])), 2)
    assert (out["precision"][:, :, 1, 0, 2] == 1 / (2 + 2.0 ** -52)).all() and 1 / (2 + 2.0 ** -52) == 0.5
    assert (out["recall"][:, 1, 0, 1:] == 1).all()
    assert (out["recall"][:, 1, 0, 0] == 0).all()    # maxDet 1 keeps the FP alone
    assert (out["precision"][:, :, 1, 0, 0] == 0).all()


def test_class_with_gt_and_no_detections_and_class_without_gt():
    out = _acc(ref.images(([(BOX, 2, 0.9)], [(BOX, 1, 0)])), 3)
    assert (out["precision"][:, :, 1, [0, 3], :] == 0).all() and (out["recall"][:, 1, [0, 3], :] == 0).all()
    assert (out["precision"][:, :, 2] == -1).all() and (out["recall"][:, 2] == -1).all()
    assert out["ap_per_class"].tolist() == [-1, 0, -1]
    assert out["stats"][0] == 0 and out["n_stats"][0] == 10 * 101


def test_exact_thresholds_match():
    gt = (0, 0, 10, 10)
    for t, w in [(0, 5), (2, 6), (5, 7.5), (9, 9.5)]:
        v = ref.iou((0, 0, 10, w), gt)
        assert v == ref.T[t], (t, v)
        st = ref.run([ref.images(([((0, 0, 10, w), 1, 0.5)], [(gt, 1, 0)]))], 2)
        m, ig, rank = ref.unpack_bits(st.rec_bits[:1])
        assert m[0, 0].tolist() == [i <= t for i in range(10)] and rank[0] == 0


# ------------------------------------------------ sequential against two-phase
def test_sequential_equals_two_phase():
    n = 0
    for seed in range(60):
        c = ref.make_case(2, 24, 6, 3, seed=100 + seed, shuffle=bool(seed & 1), levels=4, crowd=0.3)
        a = ref.run([c], 3)
        b = ref.run([c], 3, match=ref.match_two_phase)
        assert np.array_equal(a.hdr, b.hdr) and np.array_equal(a.rec_key, b.rec_key)
        assert np.array_equal(a.rec_bits, b.rec_bits), seed
        n += len(a.matched_gt)
    # identical boxes: equal IoUs everywhere, the tie rules decide
    for seed in range(60):
        r = np.random.default_rng(seed)
        gt = [(BOX if r.uniform() < 0.6 else (10, 20, 110, 200), 1, int(r.uniform() < 0.3)) for _ in range(5)]
        det = [(BOX if r.uniform() < 0.6 else (10, 20, 110, 200), 1, float(r.integers(0, 3))) for _ in range(8)]
        c = ref.images((det, gt))
        a = ref.run([c], 2)
        b = ref.run([c], 2, match=ref.match_two_phase)
        assert np.array_equal(a.rec_bits, b.rec_bits), seed
        n += 1
    assert n >= 180


# ------------------------------------------------------- maxDets as a prefix
def test_maxdets_is_a_prefix():
    """Matching the first m detections of a rank order alone gives the first m
    columns of matching all of them: matching is done once, maxDets filters on rank."""
    for seed in range(20):
        c = ref.make_case(1, 40, 8, 2, seed=300 + seed, counts=[40], crowd=0.25, levels=8)
        gl = np.where((c["gt_labels"][0] >= 1) & (c["gt_labels"][0] < 2), c["gt_labels"][0], 0)
        gs = np.nonzero(gl == 1)[0]
        gc = c["gt_crowd"][0, gs] != 0
        order = np.argsort(ref.desc_score_key(c["det_scores"][0]), kind="stable")
        db = c["det_boxes"][0, order].astype(np.float64)
        ious = ref.iou_matrix(db, c["gt_boxes"][0, gs], gc)
        garea = ref.area(c["gt_boxes"][0, gs])
        for a in range(4):
            gig = gc | (garea < ref.A[a, 0]) | (garea > ref.A[a, 1])
            full = ref.match_sequential(ious, gig, gc, ref.area(db), *ref.A[a])
            for m in (1, 10):
                part = ref.match_sequential(ious[:m], gig, gc, ref.area(db[:m]), *ref.A[a])
                assert all(np.array_equal(p, f[:, :m]) for p, f in zip(part, full))


def test_generator_shapes():
    c = ref.make_case(2, 40, 6, 4, seed=5, counts=[-3, 45], bad_labels=True)
    assert c["det_count"].tolist() == [-3, 45]
    assert (c["det_boxes"][0] == np.float32(1e30)).all() and (c["det_scores"][0] == 9).all()
    assert c["gt_boxes"].dtype == np.float64 and c["gt_labels"].dtype == np.int32 and c["gt_crowd"].dtype == np.uint8
    again = ref.make_case(1, 40, 6, 4, seed=5, first_image=1, counts=[45], bad_labels=True)
    assert all(np.array_equal(c[k][1:], again[k]) for k in ref.ARGS)
