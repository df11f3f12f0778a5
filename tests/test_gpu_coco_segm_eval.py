"""ops.mask_overlap + ops.coco_segm_eval_update / COCOMaskEvaluator against the numpy restatement
of the contract (tests/coco_segm_ref.py) on the named cases of tests/coco_segm_cases.py.

Bars: the overlap counts, the header (n_records, n_images, dropped, npig), rec_key, the rank and
the matched / ignored masks of every record, and precision and recall in full are bit-exact.
stats and ap_per_class are within n * 2^-52 absolute, n the number of entries averaged: both
sides add the same at most n terms, each in [0, 1], in different orders.  Each case asserts its
precondition on the reference alone (tests/test_coco_segm_cpu.py does so without a GPU)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import coco_eval_ref as cref  # noqa: E402
import coco_segm_cases as sc  # noqa: E402
import coco_segm_ref as ref  # noqa: E402
from replication_faster_rcnn_amd import _lib, ops  # noqa: E402
from replication_faster_rcnn_amd.evaluate import COCO_STATS, COCOEvaluator, COCOMaskEvaluator  # noqa: E402

pytestmark = pytest.mark.gpu

_cache = {}


def reference(name):
    """(case, state, overlaps, accumulate) of the restatement: made once, never modified."""
    if name not in _cache:
        c = sc.CASES[name]()
        st, ovs = ref.run(c["batches"], c["C"], c["cap"])
        _cache[name] = (c, st, ovs, st.accumulate())
    return _cache[name]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def update(state, b, C, want_overlap=None):
    t = {k: dev(b[k]) for k in ref.ARGS}
    ov = ops.mask_overlap(t["det_masks"], t["gt_masks"], det_labels=t["det_labels"], det_count=t["det_count"],
                          gt_labels=t["gt_labels"], n_class=C)
    if want_overlap is not None:
        for name, g, w in zip(ov._fields, ov, want_overlap):
            assert np.array_equal(g.cpu().numpy(), w), (name, np.argwhere(g.cpu().numpy() != w)[:8])
    ops.coco_segm_eval_update((t["det_labels"], t["det_scores"], t["det_count"]), ov, t["gt_labels"], t["gt_crowd"],
                              gt_area=t["gt_area"], state=state)


def host(state):
    hdr, key, bits, _ = (t.cpu().numpy() for t in state)
    return hdr, key.view(np.uint64), bits.view(np.uint64)


def assert_state(state, st):
    hdr, key, bits = host(state)
    assert np.array_equal(hdr, st.hdr), (hdr, st.hdr)
    n = int(st.hdr[0])
    assert np.array_equal(key[:n], st.rec_key[:n]), "rec_key differs"
    gm, gi, gr = cref.unpack_bits(bits[:n])
    wm, wi, wr = cref.unpack_bits(st.rec_bits[:n])
    assert np.array_equal(gr, wr), ("rank differs", np.nonzero(gr != wr)[0][:8])
    assert np.array_equal(gm, wm), ("matched masks differ", np.argwhere(gm != wm)[:8])
    assert np.array_equal(gi, wi), ("ignored masks differ", np.argwhere(gi != wi)[:8])
    assert np.array_equal(bits[:n], st.rec_bits[:n]), "unused record bits are set"


def assert_accumulate(got, want):
    precision, recall, stats, apc = got
    assert np.array_equal(precision, want["precision"]), np.argwhere(precision != want["precision"])[:8]
    assert np.array_equal(recall, want["recall"]), np.argwhere(recall != want["recall"])[:8]
    for g, exp, n in [(stats, want["stats"], want["n_stats"]), (apc, want["ap_per_class"], want["n_ap"])]:
        assert np.array_equal(g == -1, exp == -1), (g, exp)
        diff, bound = np.abs(g - exp), n * 2.0 ** -52
        print("largest |diff|:", float(diff.max()), "its bound:", float(bound[diff.argmax()]))
        assert (diff <= bound).all(), (g, exp, bound)


def run_once(name):
    c, st, ovs, want = reference(name)
    state = ops.coco_eval_state(c["C"], st.cap)
    state[1].zero_()
    state[2].zero_()
    for b, ov in zip(c["batches"], ovs):
        update(state, b, c["C"], ov if int(st.hdr[2]) == 0 else None)
    assert_state(state, st)
    acc = [t.cpu().numpy() for t in ops.coco_eval_accumulate(state, int(st.hdr[0]))]
    assert_accumulate(acc, want)
    return [t.cpu().numpy() for t in state[:3]] + acc


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_named_case(name):
    c, st, ovs, want = reference(name)
    sc.CHECKS[name](st, ovs, want)                      # the precondition, on the reference alone
    first, second = run_once(name), run_once(name)
    assert all(np.array_equal(a, b) for a, b in zip(first, second)), "two runs differ"


def test_kernel_names():
    assert ops.coco_eval_kernel(segm=True) == "coco_match_kernel<counts>+coco_advance_kernel"
    assert ops.coco_eval_kernel() == "coco_match_kernel<boxes>+coco_advance_kernel"
    assert ops.mask_overlap_kernel(200, 200) == "mo_pack_kernel[vec16+edges]+mo_pair_kernel"
    assert ops.mask_overlap_kernel(16, 16) == "mo_pack_kernel[vec16]+mo_pair_kernel"


def test_several_updates_equal_one():
    c, st, _, _ = reference("several_updates")
    many, one = ops.coco_eval_state(c["C"], st.cap), ops.coco_eval_state(c["C"], st.cap)
    for b in c["batches"]:
        update(many, b, c["C"])
    update(one, ref.concat(c["batches"]), c["C"])
    n = int(st.hdr[0])
    (h1, k1, b1), (h2, k2, b2) = host(many), host(one)
    assert np.array_equal(h1, h2) and np.array_equal(k1[:n], k2[:n]) and np.array_equal(b1[:n], b2[:n])
    assert_state(one, st)


def evaluator_update(ev, b):
    ev.update((b["det_labels"], b["det_scores"], b["det_count"]), b["det_masks"], b["gt_masks"],
              b["gt_labels"].astype(np.float64), b["gt_crowd"], b["gt_area"])      # host arrays, the loader's dtypes


def test_mask_evaluator_result():
    c, st, _, want = reference("several_updates")
    ev = COCOMaskEvaluator(c["C"], st.cap)
    assert isinstance(ev, COCOEvaluator)
    for b in c["batches"]:
        evaluator_update(ev, b)
    assert_state(ev.state, st)
    out = ev.result()
    assert out["n_records"] == st.hdr[0] and out["n_images"] == 6 and np.array_equal(out["npig"], st.npig)
    assert_accumulate([out[k] for k in ("precision", "recall", "stats", "ap_per_class")], want)
    assert [out[k] for k in COCO_STATS] == out["stats"].tolist() and 0 < out["AP"] <= out["AP50"] <= 1
    ev.reset()
    evaluator_update(ev, c["batches"][2])
    assert ev.result()["n_images"] == 1


def test_mask_evaluator_takes_the_gt_area_field():
    c, st, _, want = reference("gt_area_field")
    ev = COCOMaskEvaluator(c["C"], st.cap)
    evaluator_update(ev, c["batches"][0])
    assert_state(ev.state, st)
    assert ev.result()["npig"][1].tolist() == [2, 1, 1, 0]


def test_dropped_batch_is_counted_and_result_raises():
    c, st, _, _ = reference("dropped_batch")
    ev = COCOMaskEvaluator(c["C"], st.cap)
    for b in c["batches"]:
        evaluator_update(ev, b)
    assert_state(ev.state, st)
    with pytest.raises(_lib.FrcnnError, match="dropped"):
        ev.result()


def test_box_evaluator_accumulates_a_segm_state():
    """The records are the bbox ones: COCOEvaluator's inherited result() closes a state that
    coco_segm_eval_update filled."""
    c, st, _, want = reference("random_200")
    ev = COCOEvaluator(c["C"], st.cap)
    for b in c["batches"]:
        update(ev.state, b, c["C"])
    out = ev.result()
    assert out["n_records"] == st.hdr[0] and np.array_equal(out["npig"], st.npig)
    assert_accumulate([out[k] for k in ("precision", "recall", "stats", "ap_per_class")], want)


def test_paste_to_evaluator_makes_no_host_read():
    N, D, C, M, H, W = 2, 6, 3, 14, 40, 56
    g = torch.Generator().manual_seed(5)
    logits = (torch.randn(N * D, C, M, M, generator=g) + 2.5).cuda()           # most of a box is set
    xy = torch.rand(N, D, 2, generator=g) * torch.tensor([W - 24.0, H - 20.0])
    boxes = torch.cat([xy, xy + torch.tensor([22.0, 18.0])], 2).cuda()           # x1, y1, x2, y2
    labels = torch.randint(1, C, (N, D), generator=g, dtype=torch.int32).cuda()
    scores = torch.rand(N, D, generator=g).cuda()
    count = torch.tensor([D, D - 2], dtype=torch.int32).cuda()
    det = ops.BoxDetections(boxes, labels, scores, None, count, None)
    gt_masks = torch.zeros((N, 3, H, W), dtype=torch.uint8)
    gt_labels = torch.zeros((N, 3), dtype=torch.int32)
    for n in range(N):
        for k in range(2):                              # a gt on the box of detections 0 and 1, 255 for set
            x1, y1, x2, y2 = (int(v) for v in boxes[n, k].tolist())
            gt_masks[n, k, y1:y2 + 1, x1:x2 + 1] = 255
            gt_labels[n, k] = int(labels[n, k])
    gt_masks, gt_labels = gt_masks.cuda(), gt_labels.cuda()
    gt_crowd = torch.zeros((N, 3), dtype=torch.uint8).cuda()
    ev = COCOMaskEvaluator(C, N * D)
    ev.update(det, ops.mask_head_paste(logits, boxes, labels, count, (H, W)), gt_masks, gt_labels, gt_crowd)
    ev.reset()                                          # the outputs and the workspace are cached now
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        masks = ops.mask_head_paste(logits, boxes, labels, count, (H, W))
        ev.update(det, masks, gt_masks, gt_labels, gt_crowd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    out = ev.result()
    b = ref.case(masks.cpu().numpy(), gt_masks.cpu().numpy(), labels.cpu().numpy(), scores.cpu().numpy(),
                 count.cpu().numpy(), gt_labels.cpu().numpy(), gt_crowd.cpu().numpy())
    st, _ = ref.run([b], C, N * D)
    assert_state(ev.state, st)
    assert masks.any() and out["n_records"] == 2 * D - 2 and out["AR100"] > 0


def test_wrapper_rejects_wrong_inputs_before_any_launch():
    c, st, ovs, _ = reference("taken_gt")
    b = c["batches"][0]
    t = {k: dev(b[k]) for k in ref.ARGS}
    ov = ops.MaskOverlap(*(dev(a) for a in ovs[0]))
    state = ops.coco_eval_state(2, 64)
    det = (t["det_labels"], t["det_scores"], t["det_count"])
    good = dict(det=det, overlap=ov, gt_labels=t["gt_labels"], gt_crowd=t["gt_crowd"], gt_area=None, state=state)

    def refused(match, **over):
        a = dict(good, **over)
        with pytest.raises(RuntimeError, match=match):
            ops.coco_segm_eval_update(a["det"], a["overlap"], a["gt_labels"], a["gt_crowd"], gt_area=a["gt_area"],
                                      state=a["state"])

    refused("det must be", det=det[:2])
    refused("det.labels", det=(det[0].long(), det[1], det[2]))
    refused("det.scores", det=(det[0], det[1].double(), det[2]))
    refused("det.count", det=(det[0], det[1], det[2].cpu()))
    refused("overlap must be", overlap=ov.inter)
    refused("overlap.inter", overlap=ops.MaskOverlap(ov.inter.long(), ov.det_area, ov.gt_area))
    refused("overlap.inter", overlap=ops.MaskOverlap(ov.inter[:, :, :1], ov.det_area, ov.gt_area))
    refused("overlap.det_area", overlap=ops.MaskOverlap(ov.inter, ov.det_area.float(), ov.gt_area))
    refused("overlap.gt_area", overlap=ops.MaskOverlap(ov.inter, ov.det_area, ov.gt_area.cpu()))
    refused("gt_labels", gt_labels=t["gt_labels"].long())
    refused("gt_crowd", gt_crowd=t["gt_crowd"].bool())
    refused("gt_area", gt_area=ov.gt_area.float())
    refused("gt_area", gt_area=ov.gt_area.double()[:, :1])
    refused("state", state=state[:3])
    torch.cuda.synchronize()
    assert int(state[0][0]) == 0 and int(state[0][1]) == 0
    ops.coco_segm_eval_update(det, ov, t["gt_labels"], t["gt_crowd"], state=state)
    assert int(state[0][0]) == 3
