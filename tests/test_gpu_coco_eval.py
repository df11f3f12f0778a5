"""ops.coco_eval_update / ops.coco_eval_accumulate / COCOEvaluator against the
numpy restatement of the contract (tests/coco_eval_ref.py: pycocotools'
sequential matching loop and its accumulate).

Bars: the header (n_records, n_images, dropped, npig), rec_key, the rank and the
matched / ignored masks of every record, and precision and recall in full are
bit-exact.  stats and ap_per_class are within n * 2^-52 absolute, n the number
of entries averaged: both sides add the same at most n terms, each in [0, 1], in
different orders.  -1 positions are equal.  Each case asserts its precondition
on the reference alone."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import coco_eval_ref as ref  # noqa: E402
from replication_faster_rcnn_amd import _lib, ops, synth  # noqa: E402
from replication_faster_rcnn_amd.evaluate import COCO_STATS, COCOEvaluator  # noqa: E402

pytestmark = pytest.mark.gpu

U = np.uint64
_cache = {}
BOX = (10, 20, 110, 220)          # 100 x 200: large
mk = ref.make_case


def reference(name, build, C, cap=None):
    """(cases, reference state, reference accumulate) of a named list of batches: made once, never modified."""
    if name not in _cache:
        cs = build()
        st = ref.run(cs, C, cap)
        _cache[name] = (cs, st, st.accumulate())
    return _cache[name]


def update(state, case):
    db, dl, ds, dc, gb, gl, gc = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in ref.args(case))
    ops.coco_eval_update((db, dl, ds, dc), gb, gl, gc, state=state)


def host(state):
    hdr, key, bits, _ = (t.cpu().numpy() for t in state)
    return hdr, key.view(np.uint64), bits.view(np.uint64)


def assert_state(state, st):
    hdr, key, bits = host(state)
    assert np.array_equal(hdr, st.hdr), (hdr, st.hdr)
    n = int(st.hdr[0])
    assert np.array_equal(key[:n], st.rec_key[:n]), "rec_key differs"
    gm, gi, gr = ref.unpack_bits(bits[:n])
    wm, wi, wr = ref.unpack_bits(st.rec_bits[:n])
    assert np.array_equal(gr, wr), ("rank differs", np.nonzero(gr != wr)[0][:8])
    assert np.array_equal(gm, wm), ("matched masks differ", np.argwhere(gm != wm)[:8])
    assert np.array_equal(gi, wi), ("ignored masks differ", np.argwhere(gi != wi)[:8])
    assert np.array_equal(bits[:n], st.rec_bits[:n]), "unused record bits are set"


def assert_accumulate(state, st, want):
    precision, recall, stats, apc = (t.cpu().numpy() for t in ops.coco_eval_accumulate(state, int(st.hdr[0])))
    assert np.array_equal(precision, want["precision"]), np.argwhere(precision != want["precision"])[:8]
    assert np.array_equal(recall, want["recall"]), np.argwhere(recall != want["recall"])[:8]
    for got, exp, n in [(stats, want["stats"], want["n_stats"]), (apc, want["ap_per_class"], want["n_ap"])]:
        assert np.array_equal(got == -1, exp == -1), (got, exp)
        diff, bound = np.abs(got - exp), n * 2.0 ** -52
        print("largest |diff|:", float(diff.max()), "its bound:", float(bound[diff.argmax()]))
        assert (diff <= bound).all(), (got, exp, bound)
    return dict(precision=precision, recall=recall, stats=stats, ap_per_class=apc)


def run(name, build, C, cap=None):
    cs, st, want = reference(name, build, C, cap)
    state = ops.coco_eval_state(C, st.cap)
    for c in cs:
        update(state, c)
    assert_state(state, st)
    return state, st, want, assert_accumulate(state, st, want)


def cases(name):
    return _cache[name][0]


def masks(st, i):
    m, ig, rank = ref.unpack_bits(st.rec_bits[i:i + 1])
    return m[0], ig[0], int(rank[0])


# ---------------------------------------------------------------- named cases
def test_iou_exactly_at_a_threshold_matches():
    gt = (0, 0, 10, 10)
    dets = [((0, 0, 10, 5), 0), ((0, 0, 10, 6), 2), ((0, 0, 10, 7.5), 5), ((0, 0, 10, 9.5), 9)]
    imgs = [([(b, 1, 0.5)], [(gt, 1, 0)]) for b, _ in dets]
    _, st, _, _ = run("at_threshold", lambda: [ref.images(*imgs)], 2)
    for i, (b, t) in enumerate(dets):
        assert ref.iou(b, gt) == ref.T[t]
        assert masks(st, i)[0][0].tolist() == [j <= t for j in range(10)]


def test_equal_iou_later_gt_wins():
    c = ref.images(([(BOX, 1, 0.9), (BOX, 1, 0.8)], [(BOX, 1, 0), (BOX, 1, 0), ((300, 300, 340, 340), 1, 0)]))
    _, st, _, _ = run("equal_iou", lambda: [c], 2)
    slots, dtg = st.matched_gt[0][(1, 0)]
    assert dtg[:, 0].tolist() == [1] * 10 and dtg[:, 1].tolist() == [0] * 10      # gt 1 first, then gt 0


def test_taken_gt_sends_next_detection_on():
    a, b = (0, 0, 100, 100), (0, 10, 100, 110)         # IoU(a, b) = 90 / 110
    c = ref.images(([(a, 1, 0.9), (a, 1, 0.8), (a, 1, 0.7)], [(a, 1, 0), (b, 1, 0)]))
    _, st, _, _ = run("taken", lambda: [c], 2)
    _, dtg = st.matched_gt[0][(1, 0)]
    assert 0.8 < ref.iou(a, b) < 0.85
    assert dtg[0].tolist() == [0, 1, -1] and dtg[7].tolist() == [0, -1, -1]      # second-best at 0.5, FP at 0.85
    m, ig, _ = masks(st, 2)
    assert not m[0].any() and not ig[0].any()


def test_crowd_matches_many_and_uses_detection_area():
    crowd = (0, 0, 400, 400)
    small = (100, 100, 120, 120)                       # inside the crowd box: i / area_d = 1
    c = ref.images(([(small, 1, 0.9), ((50, 50, 90, 90), 1, 0.8), ((200, 200, 260, 260), 1, 0.7),
                     ((500, 500, 560, 560), 1, 0.6)], [(crowd, 1, 1), ((700, 700, 800, 800), 1, 0)]))
    _, st, want, _ = run("crowd", lambda: [c], 2)
    assert ref.iou(small, crowd, True) == 1 and ref.iou(small, crowd) < 0.5
    for i in range(3):
        m, ig, _ = masks(st, i)
        assert m[0].all() and ig[0].all()              # matched at 0.95 too, ignored: no FP
    m, ig, _ = masks(st, 3)
    assert not m[0].any() and not ig[0].any()          # the one FP
    assert st.npig[1, 0] == 1


def test_regular_gt_preferred_over_crowd():
    det, reg, crowd = (0, 0, 100, 100), (0, 0, 100, 125), (0, 0, 100, 100)
    c = ref.images(([(det, 1, 0.9)], [(crowd, 1, 1), (reg, 1, 0)]))
    _, st, _, _ = run("regular_over_crowd", lambda: [c], 2)
    assert ref.iou(det, crowd, True) == 1 and ref.iou(det, reg) == 0.8
    m, ig, _ = masks(st, 0)
    _, dtg = st.matched_gt[0][(1, 0)]
    assert dtg[:, 0].tolist() == [1] * 7 + [0] * 3                                # regular while IoU >= t
    assert ig[0].tolist() == [False] * 7 + [True] * 3 and m[0].all()


def test_area_edges():
    g1, g2 = (0, 0, 32, 32), (100, 100, 196, 196)       # areas 1,024 and 9,216
    big = (300, 300, 500, 500)
    c = ref.images(([((300, 600, 330, 630), 1, 0.9),    # unmatched, small: FP in all / small, ignored in medium / large
                     ((0, 0, 32, 36), 1, 0.8)],         # area 1,152 (medium), matched to the gt of 1,024
                    [(g1, 1, 0), (g2, 1, 0), (big, 1, 0)]))
    _, st, _, _ = run("area_edges", lambda: [c], 2)
    assert ref.area(g1) == 1024 and ref.area(g2) == 9216
    assert st.npig[1].tolist() == [3, 1, 2, 2]
    m, ig, _ = masks(st, 0)
    assert not m.any() and ig[:, 0].tolist() == [False, False, True, True]
    m, ig, _ = masks(st, 1)
    assert ref.iou((0, 0, 32, 36), g1) > 0.85
    assert m[1, :8].all() and not ig[1, :8].any()       # out of the small range itself, a TP there
    assert m[2, :8].all() and not ig[2, :8].any() and m[3, :8].all() and ig[3, :8].all()    # large: g1 is ignored


def test_101_detections_of_one_class():
    def build():
        det = [((0, 0, 50, 50 + i), 1, 1.0 - i / 256) for i in range(100)] + [(BOX, 1, 0.25)]
        return [ref.images((det, [(BOX, 1, 0)]))]
    _, st, want, _ = run("d101", build, 2)
    m, ig, rank = masks(st, 100)
    assert rank == ref.RANK_OUT and not m.any() and not ig.any()
    assert (want["recall"][:, 1, 0, 2] == 0).all()      # its would-be TP does not count


def test_ar_strictly_ordered():
    def build():
        gts = [((0, 30 * i, 20, 30 * i + 20), 1, 0) for i in range(12)]
        det = [((300, 300, 340, 340), 1, 0.99)] + [(b, 1, 0.9 - i / 64) for i, (b, _, _) in enumerate(gts)]
        return [ref.images((det, gts))]
    _, _, want, got = run("ar", build, 2)
    assert want["stats"][6] == 0 and want["stats"][7] == 9 / 12 and want["stats"][8] == 1
    assert got["stats"][6] < got["stats"][7] < got["stats"][8]


def test_equal_scores_keep_image_slot_order():
    _, st, _, _ = run("ties", lambda: [mk(3, 40, 6, 3, seed=31, levels=1, counts=[40, 33, 40])], 3)
    n = int(st.hdr[0])
    key = np.sort(st.rec_key[:n])
    score = (key >> U(24)) & U(0xFFFFFFFF)
    assert len(np.unique(score)) <= 2                   # scores 0 and 1 only
    same = (key[1:] >> U(24)) == (key[:-1] >> U(24))
    assert same.sum() > n // 2 and ((key[1:] & U(0xFFFFFF)) > (key[:-1] & U(0xFFFFFF)))[same].all()


def test_shuffled_slots():
    run("shuffled", lambda: [mk(4, 65, 5, 3, seed=32, shuffle=True, counts=[65, 64, 65, 33])], 3)
    cs = cases("shuffled")
    lab = cs[0]["det_labels"][0, :65]
    assert (np.diff(lab) < 0).any() and (np.diff(cs[0]["det_scores"][0, :65]) > 0).any()


def test_labels_outside_the_classes():
    _, st, _, _ = run("bad_labels", lambda: [mk(3, 48, 8, 4, seed=33, bad_labels=True)], 4)
    cs = cases("bad_labels")
    lab, gl = cs[0]["det_labels"][0, :int(cs[0]["det_count"][0])], cs[0]["gt_labels"]
    assert ((lab < 1) | (lab >= 4)).any() and ((gl == 0) | (gl >= 4)).any()
    zero = (st.rec_key[:int(st.hdr[0])] >> U(56)) == 0
    assert zero.any() and (ref.unpack_bits(st.rec_bits[:int(st.hdr[0])])[2][zero] == ref.RANK_OUT).all()


def test_det_count_clamped():
    _, st, _, _ = run("clamped", lambda: [mk(4, 40, 6, 4, seed=34, counts=[-3, 0, 45, 20])], 4)
    assert st.hdr[0] == 60 and st.hdr[1] == 4


def test_no_gt_slots():
    _, st, want, _ = run("g0", lambda: [mk(2, 20, 0, 3, seed=35)], 3)
    assert st.hdr[0] > 0 and (st.npig == 0).all() and (want["stats"] == -1).all()


def test_256_gt_of_one_class():
    _, st, _, _ = run("g256", lambda: [mk(1, 130, 256, 3, seed=36, counts=[130], one_class=2, crowd=0.1)], 3)
    cs = cases("g256")
    assert (cs[0]["gt_labels"] == 2).all() and st.npig[2, 0] + cs[0]["gt_crowd"].sum() == 256
    _, dtg = st.matched_gt[0][(2, 0)]
    assert (dtg >= 64).any() and (dtg >= 192).any()     # gt in every 64-bit word of the taken set


def test_two_classes():
    run("c2", lambda: [mk(2, 30, 4, 2, seed=37)], 2)


def test_128_classes():
    _, st, _, _ = run("c128", lambda: [mk(2, 300, 64, 128, seed=38, counts=[300, 280])], 128)
    assert (st.npig[:, 0] > 0).sum() > 20 and np.nonzero(st.npig[:, 0])[0].max() > 100
    assert int((st.rec_key[:int(st.hdr[0])] >> U(56)).max()) == 127


@pytest.mark.parametrize("seg", [255, 256, 257, 4097])
def test_class_segment_edges(seg):
    """A class segment of `seg` records: the accumulate kernel's 256-record chunk and the sort's 4,096-key tile."""
    def build():
        n_img = (seg + 127) // 128
        counts = [128] * (seg // 128) + ([seg % 128] if seg % 128 else [])
        c = mk(n_img, 128, 6, 3, seed=40, counts=counts, one_class=1, levels=64, crowd=0.1)
        extra = mk(1, 128, 6, 3, seed=41, counts=[77], one_class=2)
        return [c, extra]
    _, st, _, _ = run("seg%d" % seg, build, 3)
    cls = st.rec_key[:int(st.hdr[0])] >> U(56)
    assert (cls == 1).sum() == seg and (cls == 2).sum() == 77


def test_more_slots_than_the_lds_slot_table():
    """Slots from 4,096 on have their class and rank read back instead of found in LDS."""
    _, st, _, _ = run("slots4200", lambda: [mk(2, 4200, 6, 3, seed=42, counts=[4200, 100], shuffle=True,
                                               levels=1 << 16)], 3)
    rank = ref.unpack_bits(st.rec_bits[:4200])[2]
    assert (rank[4096:] < ref.KEEP).any() and (rank[:4096] < ref.KEEP).any()


def batches():
    return [mk(2, 64, 8, 5, seed=50), mk(3, 64, 8, 5, seed=50, first_image=2), mk(1, 64, 8, 5, seed=50, first_image=5)]


def test_several_updates_equal_one():
    state, st, want, got = run("batches", batches, 5)
    one = ops.coco_eval_state(5, st.cap)
    update(one, ref.concat(batches()))
    n = int(st.hdr[0])
    (h1, k1, b1), (h2, k2, b2) = host(state), host(one)
    assert np.array_equal(h1, h2) and np.array_equal(k1[:n], k2[:n]) and np.array_equal(b1[:n], b2[:n])
    again = [t.cpu().numpy() for t in ops.coco_eval_accumulate(one, int(st.hdr[0]))]
    assert all(np.array_equal(x, got[k]) for x, k in zip(again, ("precision", "recall", "stats", "ap_per_class")))


def test_batch_that_does_not_fit_is_dropped_and_result_raises():
    cs = batches()
    k = [int(np.clip(c["det_count"], 0, 64).sum()) for c in cs]
    cap = k[0] + k[1] - 1                               # the second batch does not fit, the third does
    assert k[0] + k[2] <= cap
    st = ref.run(cs, 5, cap)
    assert st.hdr[2] == 1 and st.hdr[0] == k[0] + k[2] and st.hdr[1] == 3
    ev = COCOEvaluator(5, cap)
    for c in cs:
        ev.update(ref.args(c)[:4], *ref.args(c)[4:])
    assert_state(ev.state, st)
    with pytest.raises(_lib.FrcnnError, match="dropped"):
        ev.result()
    ev.reset()
    ev.update(ref.args(cs[0])[:4], *ref.args(cs[0])[4:])
    assert ev.result()["n_records"] == k[0]


def random_cfg2():
    return [mk(8, 300, 8, 21, seed=60, crowd=0.15, jitter=0.3)]


def test_random_case_at_cfg2_scale():
    _, st, want, got = run("cfg2", random_cfg2, 21)
    p = want["precision"][:, :, 1:, 0, 2]
    ap = np.array([p[t][p[t] > -1].mean() for t in range(10)])
    assert (np.diff(ap) < 0).all(), ap                  # all ten thresholds separate
    assert (st.npig[:, 1:] > 0).any(axis=0).all()       # small, medium and large objects


def test_two_runs_give_identical_bits():
    _, st, _, got = run("cfg2", random_cfg2, 21)
    cs = cases("cfg2")
    outs = []
    for _ in range(2):
        state = ops.coco_eval_state(21, st.cap)
        state[1].zero_()
        state[2].zero_()
        update(state, cs[0])
        outs.append([t.cpu().numpy() for t in state[:3]] +
                    [t.cpu().numpy() for t in ops.coco_eval_accumulate(state, int(st.hdr[0]))])
    assert all(np.array_equal(a, b) for a, b in zip(*outs))
    assert np.array_equal(outs[0][5], got["stats"]) and np.array_equal(outs[0][6], got["ap_per_class"])


def test_coco_evaluator_result():
    cs, st, want = reference("batches", batches, 5)
    ev = COCOEvaluator(5, st.cap)
    for c in cs:                                        # host arrays in the loader's dtypes
        ev.update((c["det_boxes"], c["det_labels"], c["det_scores"], None, c["det_count"], None),
                  c["gt_boxes"].astype(np.float32).astype(np.float64), c["gt_labels"].astype(np.float64), c["gt_crowd"])
    out = ev.result()
    assert out["n_records"] == st.hdr[0] and out["n_images"] == 6 and np.array_equal(out["npig"], st.npig)
    assert np.array_equal(out["precision"], want["precision"]) and np.array_equal(out["recall"], want["recall"])
    assert [out[k] for k in COCO_STATS] == out["stats"].tolist() and len(out["ap_per_class"]) == 5
    assert 0 < out["AP"] < out["AP50"] <= 1


def test_coco_evaluator_from_detect_makes_no_host_read():
    N, C, H, W = 2, 5, 600, 1000
    dev = [torch.from_numpy(a).cuda() for a in synth.head_outputs(N, 77, C, H, W, seed=21)]
    det = ops.detect(*dev, img_h=H, img_w=W, score_thresh=0.05)
    c = mk(N, 8, 8, C, seed=70)
    gb, gl, gc = (torch.from_numpy(c[k]).cuda() for k in ("gt_boxes", "gt_labels", "gt_crowd"))
    gb[:, 0] = det[0][:, 0].double()                    # one gt on the top detection of each image
    gl[:, 0] = det[1][:, 0]
    gc[:, 0] = 0
    ev = COCOEvaluator(C, N * det[1].shape[1])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev.update(det, gb, gl, gc)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    out = ev.result()
    st = ref.State(C, ev.capacity)
    st.update(*(t.cpu().numpy() for t in (det[0], det[1], det[2], det[4], gb, gl, gc)))
    assert_state(ev.state, st)
    assert out["n_records"] == int(det[4].clamp(0, det[1].shape[1]).sum()) > 0 and out["AR100"] > 0


def test_wrapper_rejects_wrong_inputs():
    c = mk(2, 16, 4, 3, seed=80)
    db, dl, ds, dc, gb, gl, gc = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in ref.args(c))
    state = ops.coco_eval_state(3, 64)
    for bad in [dict(gb=gb.float()), dict(gl=gl.long()), dict(gc=gc.bool()), dict(db=db.cpu()), dict(ds=ds[:, ::2]),
                dict(gb=gb[:1]), dict(dc=dc[:1])]:
        a = dict(db=db, dl=dl, ds=ds, dc=dc, gb=gb, gl=gl, gc=gc)
        a.update(bad)
        with pytest.raises(RuntimeError):
            ops.coco_eval_update((a["db"], a["dl"], a["ds"], a["dc"]), a["gb"], a["gl"], a["gc"], state=state)
    with pytest.raises(RuntimeError):
        ops.coco_eval_update((db, dl, ds, dc), gb, gl, gc, state=state[:3])
    with pytest.raises(RuntimeError):
        ops.coco_eval_accumulate(state, 65)
    assert int(state[0][0]) == 0
