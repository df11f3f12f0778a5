"""ops.detect and FasterRCNN.predict against the numpy restatement of the
detection contract (tests/detect_ref.py): every output bit-exact, since both
sides use the correctly rounded exp.  Each case asserts its precondition on the
reference, so a generator change cannot empty a case silently."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import detect_ref  # noqa: E402
from replication_faster_rcnn_amd import ops, synth  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = 600, 1000
_cache = {}


def inputs(name):
    """Named input sets, generated once and never modified."""
    if name not in _cache:
        if name == "mixed":
            a = synth.head_outputs(3, 300, 21, H, W, seed=2)
        elif name in ("crowd1024", "crowd600"):
            R = int(name[5:])
            rois, rc, _, reg = synth.head_outputs(1, R, 21, H, W, seed=4)
            cls = synth.rng_for(4, 0, 5).standard_normal((1, R, 21)).astype(np.float32)
            cls[:, :, 7] += 6
            a = (rois, rc, cls, reg)
        elif name == "two":
            a = synth.head_outputs(2, 77, 2, H, W, seed=3, objects=3)
        elif name == "one":
            a = synth.head_outputs(1, 1, 21, H, W, seed=5)
        _cache[name] = a
    return _cache[name]


def reference(name, thr, **kw):
    key = (name, thr, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = detect_ref.detect(*inputs(name), H, W, score_thresh=thr, **kw)
    return _cache[key]


def run(args, thr, **kw):
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args]
    return ops.detect(*dev, img_h=H, img_w=W, score_thresh=thr, **kw)


NAMES = ("boxes", "labels", "scores", "roi", "count", "total")


def assert_same(got, want):
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), f"det_{name} differs"


def cand_counts(name, thr):
    rois, rc, cls, _ = inputs(name)
    return np.array([[len(r) for r in detect_ref.candidates(rois, rc, cls, n, thr)[1]]
                     for n in range(cls.shape[0])])


@pytest.mark.parametrize("tag,thr", [("t005", 0.05), ("t07", 0.7)])
def test_golden(golden, tag, thr):
    g = golden("detect_small.npz")
    got = run((g["rois"], g["rcount"], g["cls"], g["reg"]), thr)
    assert_same(got, [g[f"{tag}_{n}"] for n in NAMES])


def test_mixed():
    want = reference("mixed", 0.05)
    assert cand_counts("mixed", 0.05).max() > 64      # more than one 64-candidate block
    assert want[5].max() > 300                        # an image keeps more than R
    assert_same(run(inputs("mixed"), 0.05), want)


def test_sparse():
    want = reference("mixed", 0.7)
    cc = cand_counts("mixed", 0.7)
    assert ((cc == 0).sum(axis=1) > 10).all() and (want[5] >= 1).all()
    assert_same(run(inputs("mixed"), 0.7), want)


@pytest.mark.parametrize("R", [1024, 600])
def test_crowd(R):
    name = f"crowd{R}"
    want = reference(name, 0.05)
    n7 = cand_counts(name, 0.05)[0, 6]
    kept7 = int((want[1][0] == 7).sum())
    assert n7 >= 600 and 0 < kept7 < n7 // 2
    assert_same(run(inputs(name), 0.05), want)


def test_two_classes():
    want = reference("two", 0.05)
    assert cand_counts("two", 0.05).max() > 32 and (want[5] >= 2).all()
    assert_same(run(inputs("two"), 0.05), want)


def test_one_row():
    want = reference("one", 0.0)
    assert want[5][0] == 20                           # every foreground class keeps its one row
    assert_same(run(inputs("one"), 0.0), want)


def test_padding_rows_are_ignored():
    rois, _, cls, reg = (a.copy() for a in synth.head_outputs(3, 128, 21, H, W, seed=6))
    rc = np.array([0, 37, 128], np.int32)
    for n in range(3):
        cls[n, rc[n]:] = 50.0
        reg[n, rc[n]:] = 1e30
    want = detect_ref.detect(rois, rc, cls, reg, H, W, score_thresh=0.05)
    assert want[4][0] == 0 and want[4][1] > 0
    got = run((rois, rc, cls, reg), 0.05)
    assert_same(got, want)
    roi = got[3].cpu().numpy()
    assert (roi[0] == -1).all() and roi[1].max() < 37
    assert (got[1][0] == -1).all() and (got[0][0] == 0).all() and (got[2][0] == 0).all()


def test_ties():
    rois, rc, cls, reg = (a.copy() for a in synth.head_outputs(1, 64, 21, H, W, seed=7))
    cls[0, 40] = cls[0, 11]                    # same logits, same box: the lower row suppresses the higher
    rois[0, 40], reg[0, 40] = rois[0, 11], reg[0, 11]
    cls[0, 50] = cls[0, 23] = 0.0              # same logits, disjoint boxes: both kept, lower row first
    cls[0, [23, 50], 3] = 9.0
    rois[0, 23], rois[0, 50] = (10, 10, 60, 60), (400, 700, 500, 900)
    reg[0, [23, 50]] = 0.0
    want = detect_ref.detect(rois, rc, cls, reg, H, W, score_thresh=0.05)
    wroi, wlab = want[3][0], want[1][0]
    assert 11 in wroi and 40 not in wroi
    pos = [int(np.nonzero((wroi == r) & (wlab == 3))[0][0]) for r in (23, 50)]
    assert pos[1] == pos[0] + 1
    assert_same(run((rois, rc, cls, reg), 0.05), want)


def test_nan_row():
    rois, rc, cls, reg = (a.copy() for a in synth.head_outputs(1, 64, 21, H, W, seed=8))
    cls[0, 17] = np.nan
    want = detect_ref.detect(rois, rc, cls, reg, H, W, score_thresh=0.05)
    assert want[5][0] > 0 and 17 not in want[3][0]
    got = run((rois, rc, cls, reg), 0.05)
    assert 17 not in got[3].cpu().numpy()
    assert_same(got, want)


def test_truncation():
    full = reference("mixed", 0.05)
    got = run(inputs("mixed"), 0.05, max_det=50)
    assert (got[4].cpu().numpy() == 50).all()
    assert np.array_equal(got[5].cpu().numpy(), full[5]) and full[5].min() > 50
    for g, w in zip(got[:4], full[:4]):
        assert np.array_equal(g.cpu().numpy(), w[:, :50])
    assert_same(got, reference("mixed", 0.05, max_det=50))


def test_no_stale_state():
    """A large call, then a small one on the same workspace and out= buffers."""
    N, R, C = 3, 1024, 21
    crowd = [np.concatenate([a] * N) for a in inputs("crowd1024")]
    sparse = list(inputs("mixed"))
    ws = torch.empty(ops._lib.load().frcnn_detect_workspace_size(N, R, C), dtype=torch.uint8, device="cuda")
    md = 300 * 20
    out = (torch.empty((N, md, 4), device="cuda"), torch.empty((N, md), dtype=torch.int32, device="cuda"),
           torch.empty((N, md), device="cuda"), torch.empty((N, md), dtype=torch.int32, device="cuda"),
           torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty(N, dtype=torch.int32, device="cuda"))
    first = run(crowd, 0.05, max_det=md, out=out, workspace=ws)
    assert first[0] is out[0]
    assert int(first[5][0]) == int(reference("crowd1024", 0.05)[5][0])
    second = run(sparse, 0.7, out=out, workspace=ws)
    assert_same(second, reference("mixed", 0.7))


def test_repeat_is_bit_identical():
    runs = [[t.cpu().numpy() for t in run(inputs("mixed"), 0.05)] for _ in range(3)]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a, b)


def test_errors():
    rois, rc, cls, reg = (torch.from_numpy(a).cuda() for a in inputs("two"))
    kw = dict(img_h=H, img_w=W)
    with pytest.raises(RuntimeError):
        ops.detect(rois, rc.long(), cls, reg, **kw)
    with pytest.raises(RuntimeError):
        ops.detect(rois, rc, cls.double(), reg, **kw)
    with pytest.raises(RuntimeError):
        ops.detect(rois[:, :-1], rc, cls, reg, **kw)
    with pytest.raises(RuntimeError):
        ops.detect(rois, rc, cls, reg[:, :, :-4].contiguous(), **kw)
    with pytest.raises(RuntimeError):
        ops.detect(rois, rc, cls.permute(0, 2, 1), reg, **kw)          # the head's [N, C, R] view
    good = ops.detect(rois, rc, cls, reg, **kw)
    with pytest.raises(RuntimeError):
        ops.detect(rois, rc, cls, reg, max_det=5, out=good, **kw)
    with pytest.raises(RuntimeError):
        ops.detect(rois, rc, cls, reg, max_det=0, **kw)
    with pytest.raises(RuntimeError):
        ops.detect(rois, rc, cls, reg, workspace=torch.empty(16, dtype=torch.uint8, device="cuda"), **kw)


def test_module_forward_and_predict():
    from replication_faster_rcnn_amd.faster_rcnn import FasterRCNN, anchor_scales, ratios
    from replication_faster_rcnn_amd.heads import ResnetHead
    from replication_faster_rcnn_amd.rpn import RPN
    assert ratios == [0.5, 1., 2.] and anchor_scales == [8, 16, 32]
    torch.manual_seed(3)
    Cf = 16

    def backbone():
        return nn.Conv2d(3, Cf, 1), nn.Sequential(nn.Conv2d(Cf, 512, 1), nn.AdaptiveAvgPool2d(1))

    model = FasterRCNN(backbone, lambda **kw: RPN(in_channels=Cf, mid_channels=Cf, **kw),
                       lambda classifier: ResnetHead(classifier), "test").cuda()
    with torch.no_grad():
        model.head.cls.weight.mul_(40)        # spread the logits: some classes pass the threshold
        model.head.reg.weight.mul_(4)
        model.rpn.reg.weight.normal_(0, 3)    # spread the proposals: NMS keeps > post_nms of them at 800 x 800
    x = torch.randn(2, 3, 10, 10).cuda()
    # predict on a 160 x 160 image: the RPN keeps fewer than its 300 slots, so rows past rois_count exist
    dets = model.predict(x, 160, 160, score_thresh=0.05)
    cls, reg = (t.cpu().numpy() for t in model.last_head_outputs)
    rois, cnt = model.rpn.rois_padded.cpu().numpy(), model.rpn.rois_count.cpu().numpy()
    N, R = rois.shape[:2]
    assert (N, R) == (2, 300) and cls.shape == (2, R, 21) and reg.shape == (2, R, 84)
    assert cnt.min() >= 1 and cnt.max() < R
    want = detect_ref.detect(rois, cnt, cls, reg, 160, 160, score_thresh=0.05)
    assert want[4].min() >= 1
    assert_same(model.last_detections, want)
    for n, (b, l, s) in enumerate(dets):
        k = want[4][n]
        assert b.device == x.device and b.shape == (k, 4) and l.shape == (k,) and s.shape == (k,)
        assert np.array_equal(b.cpu().numpy(), want[0][n, :k])
        assert np.array_equal(l.cpu().numpy(), want[1][n, :k])
        assert np.array_equal(s.cpu().numpy(), want[2][n, :k])
    # forward: the reference's 7-tuple, the head's outputs on the RPN's rois.  At 800 x 800 both
    # images fill their 300 slots (the head's view(N, -1, .) needs equal counts, as in the reference)
    with torch.no_grad():
        out = model(x, 800, 800)
        assert len(out) == 7
        rcls, rreg, frois, finds, cls_o, reg_o, anchors = out
        assert model.rpn.rois_count.tolist() == [300, 300]
        assert rcls.shape == (2, 2, 900) and rreg.shape == (2, 900, 4) and anchors.shape == (900, 4)
        assert frois.shape == (600, 4) and finds.shape == (600,)
        hc, hr = model.head(model.backbone(x), frois, finds, 800, 800, rois_sorted=True)
        # the same modules on the same inputs; the tolerance only covers the conv library picking
        # another algorithm on a second call
        torch.testing.assert_close(cls_o, hc, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(reg_o, hr, rtol=1e-5, atol=1e-6)
        assert cls_o.shape == (2, 21, 300) and reg_o.shape == (2, 300, 84)
