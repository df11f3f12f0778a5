"""ops.preprocess / ops.rescale_boxes, data.Preprocessor and
FasterRCNN.predict_images on the device against the numpy fp64 reference
(tests/preprocess_ref.py; DESIGN.md §3 "Preprocessing").  Needs an MI355X.

The tolerance per case is derived, not measured: (4*(T_h + T_w) + 16) * 2^-24 /
min(std), T the taps of an axis (preprocess_ref.tolerance)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import preprocess_ref as R  # noqa: E402
from replication_faster_rcnn_amd import data, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def run(images, out_hw, mean=R.MEAN, std=R.STD, **kw):
    """ops.preprocess of a list of uint8 images -> (numpy [N,3,oh,ow], status list)."""
    pixels, offset, hw, max_hw = data.pack_images(list(images))
    out, status = ops.preprocess(pixels.to(DEV), offset.to(DEV), hw.to(DEV), out_hw, mean=mean, std=std,
                                 max_hw=kw.pop("max_hw", max_hw), **kw)
    return out.cpu().numpy(), status.tolist()


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_preprocess_matches_reference(case):
    cid, in_hw, out_hw, _, mean, std = case
    img, ref = R.case_data(case)
    got, status = run([img], out_hw, mean, std)
    tol = R.tolerance(in_hw, out_hw, std)
    err = np.abs(got[0].astype(np.float64) - ref).max()
    print(f"{cid}: max |device - reference| = {err:.3g}, bound {tol:.3g}")
    assert status == [0] and got.shape == (1, 3) + tuple(out_hw) and got.dtype == np.float32
    assert err <= tol


def test_tile_height_does_not_change_the_bits():
    """Without max_hw the wrapper assumes the largest sizes the kernel accepts,
    which shrinks the tiles; the image's bits stay the same."""
    case = R.CASES[R.CASE_IDS.index("down_64x48")]
    img, _ = R.case_data(case)
    a, _ = run([img], case[2])
    b, sb = run([img], case[2], max_hw=None)
    c, _ = run([img], case[2], max_hw=(16384, 16384))
    assert sb == [0] and np.array_equal(a, b) and np.array_equal(a, c)


def test_batch_statuses_gaps_and_bit_identity():
    out_hw = (12, 12)
    sizes = [(5, 7), (2, 3), (1, 1), (13, 9), (20, 31), (24, 24)]
    imgs = [R.image(s, seed=40 + i) for i, s in enumerate(sizes)]
    # offsets in non-increasing order (the images laid out back to front), a 5-byte gap before image 2
    nbytes = [3 * h * w for h, w in sizes]
    offset, pos = [0] * 6, 0
    for i in reversed(range(6)):
        offset[i] = pos
        pos += nbytes[i] + (5 if i == 2 else 0)
    total = pos
    buf = np.full(total, 0xAB, np.uint8)
    for im, o, nb in zip(imgs, offset, nbytes):
        buf[o:o + nb] = im.reshape(-1)
    assert all(offset[i] > offset[i + 1] for i in range(5)) and offset[1] - offset[2] == nbytes[2] + 5
    max_hw = (24, 31)
    # three bad images: h = 0; w > max_w; offset + 3hw one byte past the buffer
    hw = sizes + [(0, 7), (5, 32), (5, 7)]
    offset = offset + [0, 0, total - 3 * 5 * 7 + 1]
    pixels = torch.from_numpy(buf).to(DEV)
    off_t = torch.tensor(offset, dtype=torch.int64, device=DEV)
    hw_t = torch.tensor(hw, dtype=torch.int32, device=DEV)
    out = torch.full((9, 3) + out_hw, float("nan"), device=DEV)     # every element is stored: no NaN survives
    status = torch.full((9,), -7, dtype=torch.int32, device=DEV)
    got, st = ops.preprocess(pixels, off_t, hw_t, out_hw, max_hw=max_hw, out=out, status=status)
    assert got is out and st is status
    assert status.tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 2]
    first = out.cpu().numpy()
    assert not np.isnan(first).any()
    assert (first[6:] == 0).all()
    for i, im in enumerate(imgs):
        alone, s = run([im], out_hw)
        assert s == [0] and np.array_equal(first[i], alone[0]), f"image {i} differs from itself preprocessed alone"
        ref = R.preprocess(im, out_hw)
        assert np.abs(first[i] - ref).max() <= R.tolerance(sizes[i], out_hw)
    again, st2 = ops.preprocess(pixels, off_t, hw_t, out_hw, max_hw=max_hw)
    assert st2.tolist() == status.tolist() and np.array_equal(again.cpu().numpy(), first)
    # a negative offset is status 2 as well; a ratio above the kernel's limit of 5 is status 1
    off_t[0] = -1
    hw_t[1] = torch.tensor([2, 61], dtype=torch.int32)
    _, st3 = ops.preprocess(pixels, off_t, hw_t, out_hw, max_hw=(24, 64))
    assert st3.tolist() == [2, 1, 0, 0, 0, 0, 1, 0, 2]


def test_rescale_boxes_is_bit_equal_to_numpy():
    rng = np.random.default_rng(5)
    N, G = 3, 32
    boxes = np.around(rng.uniform(0, 500, (N, G, 4)))
    boxes[:, 25:] = -1                      # padding rows
    boxes[0, 3, 2] = -3.0                   # a negative coordinate
    hw = np.array([[375, 500], [0, 431], [333, 499]], np.int32)
    got = ops.rescale_boxes(torch.from_numpy(boxes).to(DEV), torch.from_numpy(hw).to(DEV), (600, 608))
    assert got.dtype == torch.float64 and got.shape == (N, G, 4)
    got = got.cpu().numpy()
    for n in (0, 2):
        assert np.array_equal(got[n], data.rescale_boxes(boxes[n], hw[n], (600, 608))), n
    assert (got[1] == -1).all() and got[0, 3, 2] == -1 and (got[:, 25:] == -1).all()
    assert np.array_equal(got, R.rescale_boxes(boxes, hw, (600, 608)))


def test_wrappers_reject_wrong_inputs():
    img = R.image((5, 7), seed=1)
    pixels, offset, hw, max_hw = data.pack_images([img, img])
    p, o, h = pixels.to(DEV), offset.to(DEV), hw.to(DEV)
    good, _ = ops.preprocess(p, o, h, (12, 12), max_hw=max_hw)
    wide_hw = torch.repeat_interleave(h, 2, dim=1)[:, ::2]
    assert not wide_hw.is_contiguous() and torch.equal(wide_hw, h)
    for bad, name in [((p.float(), o, h), "pixels"), ((p.cpu(), o, h), "pixels"), ((p[None], o, h), "pixels"),
                      ((p, offset, h), "offset"), ((p, o.int(), h), "offset"),
                      ((p, o, wide_hw), "hw"), ((p, o, h.long()), "hw"), ((p, o, h[:1]), "hw")]:
        with pytest.raises(RuntimeError, match=name):
            ops.preprocess(*bad, (12, 12), max_hw=max_hw)
    with pytest.raises(RuntimeError, match="out"):
        ops.preprocess(p, o, h, (12, 12), max_hw=max_hw, out=good[:, :, :11])
    with pytest.raises(RuntimeError, match="status"):
        ops.preprocess(p, o, h, (12, 12), max_hw=max_hw, status=torch.zeros(2, device=DEV))
    with pytest.raises(RuntimeError, match="out_size"):
        ops.preprocess(p, o, h, (0, 12), max_hw=max_hw)
    with pytest.raises(RuntimeError, match="mean and std"):
        ops.preprocess(p, o, h, (12, 12), max_hw=max_hw, mean=(0.5, 0.5))
    boxes = torch.zeros(2, 4, 4, dtype=torch.float64, device=DEV)
    for bad, name in [((boxes.float(), h), "boxes"), ((boxes.cpu(), h), "boxes"), ((boxes[:, :, :3], h), "boxes"),
                      ((boxes, hw), "hw"), ((boxes, wide_hw), "hw")]:
        with pytest.raises(RuntimeError, match=name):
            ops.rescale_boxes(*bad, (12, 12))
    with pytest.raises(ValueError, match="image 1"):
        data.pack_images([img, img[:, :, :2]])
    again, _ = ops.preprocess(p, o, h, (12, 12), max_hw=max_hw)      # and the good inputs still work
    assert torch.equal(again, good)


def test_preprocessor_equals_the_ops_by_hand():
    rng = np.random.default_rng(6)
    imgs = [R.image((20, 31), seed=7), torch.from_numpy(R.image((13, 9), seed=8))]
    boxes = np.around(rng.uniform(0, 9, (2, 32, 4)))
    boxes[:, 5:] = -1
    pre = data.Preprocessor((24, 40))
    image, b, hw = pre(imgs, boxes)
    assert image.is_cuda and b.is_cuda and hw.is_cuda and pre.status.tolist() == [0, 0]
    assert image.shape == (2, 3, 24, 40) and image.dtype == torch.float32 and b.dtype == torch.float64
    pixels, offset, hw_h, max_hw = data.pack_images(imgs)
    want, _ = ops.preprocess(pixels.to(DEV), offset.to(DEV), hw_h.to(DEV), (24, 40), max_hw=max_hw)
    assert torch.equal(image, want) and torch.equal(hw.cpu(), hw_h)
    assert torch.equal(b, ops.rescale_boxes(torch.from_numpy(boxes).to(DEV), hw_h.to(DEV), (24, 40)))
    for n in range(2):
        assert np.array_equal(b[n].cpu().numpy(), data.rescale_boxes(boxes[n], hw_h[n].tolist(), (24, 40)))
    image2, none, _ = pre(imgs)
    assert none is None and torch.equal(image2, image)


def test_predict_images_maps_boxes_back():
    from replication_faster_rcnn_amd.faster_rcnn import FasterRCNN
    from replication_faster_rcnn_amd.heads import ResnetHead
    from replication_faster_rcnn_amd.rpn import RPN
    torch.manual_seed(3)
    Cf = 16

    def backbone():   # stride 16, as the RPN's anchors assume
        return (nn.Sequential(nn.AvgPool2d(16), nn.Conv2d(3, Cf, 1)),
                nn.Sequential(nn.Conv2d(Cf, 512, 1), nn.AdaptiveAvgPool2d(1)))

    model = FasterRCNN(backbone, lambda **kw: RPN(in_channels=Cf, mid_channels=Cf, **kw),
                       lambda classifier: ResnetHead(classifier), "test").cuda()
    with torch.no_grad():
        model.head.cls.weight.mul_(40)
        model.head.reg.weight.mul_(4)
        model.rpn.reg.weight.normal_(0, 3)
    sizes = [(100, 140), (131, 77)]
    # blocks of 10 x 10 pixels of one colour: features that differ from cell to cell after the pooling
    imgs = [np.ascontiguousarray(np.kron(R.image((h // 10 + 1, w // 10 + 1), seed=60 + i),
                                         np.ones((10, 10, 1), np.uint8))[:h, :w])
            for i, (h, w) in enumerate(sizes)]
    assert [im.shape for im in imgs] == [(100, 140, 3), (131, 77, 3)] and imgs[0].dtype == np.uint8
    seen = {}
    inner = model.predict

    def spy(x, width, height, **kw):      # what predict itself returned, before the mapping
        out = inner(x, width, height, **kw)
        seen["x"], seen["wh"], seen["det"] = x, (width, height), model.last_detections
        return out

    model.predict = spy
    dets = model.predict_images(imgs, new_size=(160, 176), score_thresh=0.05)
    assert seen["wh"] == (176, 160) and seen["x"].shape == (2, 3, 160, 176)
    want_x, _, _ = data.Preprocessor((160, 176))(imgs)
    assert torch.equal(seen["x"], want_x)
    raw, labels, scores, roi, count, total = seen["det"]
    boxes = model.last_detections[0]
    k = count.tolist()
    assert min(k) >= 1 and max(k) < raw.shape[1], "the case needs detections and padding rows"
    for n, (h, w) in enumerate(sizes):
        sy, sx = np.float32(h) / np.float32(160), np.float32(w) / np.float32(176)
        want = raw[n].cpu().numpy() * np.array([sy, sx, sy, sx], np.float32)
        assert np.array_equal(boxes[n].cpu().numpy(), want)
        assert (boxes[n, k[n]:] == 0).all(), "padding rows stay 0"
        b, l, s = dets[n]
        assert np.array_equal(b.cpu().numpy(), want[:k[n]]) and b.shape == (k[n], 4)
        assert torch.equal(l, labels[n, :k[n]]) and torch.equal(s, scores[n, :k[n]])
        assert not np.array_equal(want[:k[n]], raw[n, :k[n]].cpu().numpy())
    assert model.last_detections[1] is labels and model.last_detections[4] is count
