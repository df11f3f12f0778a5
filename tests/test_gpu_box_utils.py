"""The small box utilities on the HIP path (utils.bbox_iou / bbox2reg / reg2bbox,
ops.roi_transform, anchors.*) against the oracle on the edge table of
tests/box_cases.py; the oracle itself is pinned to the genuine reference's
outputs (tests/golden/box_utils_edges.npz) in tests/test_oracle_golden.py.
Needs an MI355X.

Bars: bbox_iou equal to the oracle element for element (NaN positions equal),
with numpy's output dtype and shape.  bbox2reg columns 0 and 1 bit-exact;
columns 2 and 3 within rtol 1e-12 on the fp64 paths (two fp64 ``log``
implementations) and bit-exact on the both-fp32 path, where kernel and oracle
both round the fp64 log once to fp32.  reg2bbox: the finite pattern equal and
finite values bit-exact.  roi_transform bit-exact against the oracle and the
golden.  Anchors equal to the golden.
"""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import box_cases as bc  # noqa: E402
from oracle import ref_numpy as orc  # noqa: E402
from replication_faster_rcnn_amd import anchors as A  # noqa: E402
from replication_faster_rcnn_amd import ops  # noqa: E402
from replication_faster_rcnn_amd import utils as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

IOU = bc.iou_cases()
B2R = bc.b2r_cases()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("name", list(IOU))
def test_bbox_iou_edges(name):
    a, b = IOU[name]
    with np.errstate(all="ignore"):
        want = orc.bbox_iou(a, b)
    out = U.bbox_iou(a, b)
    assert isinstance(out, np.ndarray) and out.dtype == want.dtype and out.shape == want.shape
    np.testing.assert_array_equal(out, want)


@pytest.mark.parametrize("name", list(B2R))
def test_bbox2reg_edges(name):
    a, b = B2R[name]
    with np.errstate(all="ignore"):
        want = orc.bbox2reg(a, b)
    out = U.bbox2reg(a, b)
    assert isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == want.shape
    np.testing.assert_array_equal(out[:, :2], want[:, :2])
    if name.endswith("f32_f32"):
        np.testing.assert_array_equal(out[:, 2:], want[:, 2:])
    else:
        fin = np.isfinite(want[:, 2:])
        np.testing.assert_array_equal(out[:, 2:][~fin], want[:, 2:][~fin])
        np.testing.assert_allclose(out[:, 2:][fin], want[:, 2:][fin], rtol=1e-12, atol=0)


def _check_reg2bbox(out, want):
    assert out.dtype == np.float32 and out.shape == want.shape
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(out), fin)
    assert np.array_equal(np.isnan(out), np.isnan(want))
    assert np.array_equal(out[fin], want[fin])


@pytest.mark.parametrize("n", bc.R2B_SIZES)
def test_reg2bbox_edges(n):
    anc, dl = bc.r2b_table()
    with np.errstate(all="ignore"):
        want = orc.reg2bbox(anc[:n], dl[:n])
    out = U.reg2bbox(torch.from_numpy(anc[:n]), torch.from_numpy(dl[:n]))
    assert out.device.type == "cpu"
    _check_reg2bbox(out.numpy(), want)
    # fp64 inputs (every value is exact in fp32) and strided views of wider tensors
    out64 = U.reg2bbox(torch.from_numpy(anc[:n].astype(np.float64)), torch.from_numpy(dl[:n].astype(np.float64)))
    _check_reg2bbox(out64.numpy(), want)
    wide_a = torch.from_numpy(np.repeat(anc[:n], 2, axis=1))[:, ::2]
    wide_d = torch.from_numpy(np.ascontiguousarray(dl[:n].T)).to(DEV).t()
    assert n < 2 or not (wide_a.is_contiguous() or wide_d.is_contiguous())
    out_v = U.reg2bbox(wide_a, wide_d)
    assert out_v.is_cuda                       # the output follows ``reg``
    _check_reg2bbox(out_v.cpu().numpy(), want)


@pytest.mark.parametrize("n", bc.ROI_SIZES)
def test_roi_transform_edges(golden, n):
    rois, inds = bc.roi_table()
    with np.errstate(all="ignore"):
        want = orc.roi_transform(rois[:n], inds[:n], bc.ROI_IMG_H, bc.ROI_IMG_W, bc.ROI_FEAT_H, bc.ROI_FEAT_W)
    out = ops.roi_transform(torch.from_numpy(rois[:n]).to(DEV), torch.from_numpy(inds[:n]).to(DEV),
                            bc.ROI_IMG_H, bc.ROI_IMG_W, bc.ROI_FEAT_H, bc.ROI_FEAT_W)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (n, 5)
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    np.testing.assert_array_equal(out.cpu().numpy(), golden("box_utils_edges.npz")[f"roi_{n}__boxes"])


@pytest.mark.parametrize("name", list(bc.BASE_CASES))
def test_anchor_base_edges(golden, name):
    base_size, ratios, scales = bc.BASE_CASES[name]
    base = A.generate_anchor_base(base_size, list(ratios), list(scales))
    want = golden("box_utils_edges.npz")[f"base_{name}"]
    assert base.dtype == np.float32 and base.shape == want.shape
    assert np.array_equal(base, want)


def test_anchor_base_too_many_ratios():
    assert len(bc.TOO_MANY_RATIOS) == 17
    with pytest.raises(RuntimeError, match="1..16 ratios"):
        A.generate_anchor_base(16, list(bc.TOO_MANY_RATIOS), [8])
    with pytest.raises(RuntimeError, match="1..16 ratios"):
        A.generate_anchor_base(16, [1.0], list(range(1, 18)))


@pytest.mark.parametrize("name", list(bc.GRID_CASES))
def test_generate_anchors_edges(golden, name):
    g = golden("box_utils_edges.npz")
    bname, stride, w, h = bc.GRID_CASES[name]
    a = A.generate_anchors(g[f"base_{bname}"], stride, w, h)
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == tuple(g[f"grid_{name}__shape"])
    assert sha(a) == str(g[f"grid_{name}__sha"])
    assert np.array_equal(a, orc.generate_anchors(g[f"base_{bname}"], stride, w, h))
    d = A.generate_anchors(torch.from_numpy(g[f"base_{bname}"]).to(DEV), stride, w, h)
    assert d.is_cuda and np.array_equal(d.cpu().numpy(), a)    # device base in, device anchors out
