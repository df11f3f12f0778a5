"""Score ordering on the HIP path against torch's stable descending sort, on
the named cases of tests/score_cases.py (their preconditions are asserted on
the references alone in tests/test_score_cases_cpu.py).  Needs an MI355X.

Bars: ``ops.nms`` equals the oracle's keep list exactly; ``ops.propose`` on its
three paths equals ``score_cases.propose_ref`` in anchor indices, count and
boxes, bit-exact as elsewhere; the evaluation's records equal tests/eval_ref.py,
whose matching loop walks torch's order.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eval_ref  # noqa: E402
import score_cases as sc  # noqa: E402
from replication_faster_rcnn_amd import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

_ref = {}


def _propose_reference(variant, pre, post):
    key = (variant, pre, post)
    if key not in _ref:
        anchors, s, de = sc.propose_inputs(variant)
        _ref[key] = (anchors, s, de) + sc.propose_ref(anchors, s, de, sc.IMG_W, sc.IMG_H, pre, post)
    return _ref[key]


@pytest.mark.parametrize("name", sc.NAMES)
def test_nms_score_cases(name):
    b, s, thr = sc.CASES[name]
    keep = ops.nms(torch.from_numpy(b), torch.from_numpy(s), thr)
    assert keep.dtype == torch.int64
    want = sc.reference_keep(name)
    assert np.array_equal(keep.numpy(), want), (name, keep.numpy()[:8], want[:8])


@pytest.mark.parametrize("name", sc.NAMES)
def test_nms_score_cases_device_inputs(name):
    """The same through device-resident inputs (no host round trip of the scores)."""
    b, s, thr = sc.CASES[name]
    keep = ops.nms(torch.from_numpy(b).to(DEV), torch.from_numpy(s).to(DEV), thr)
    assert keep.is_cuda
    assert np.array_equal(keep.cpu().numpy(), sc.reference_keep(name)), name


@pytest.mark.parametrize("pre,post", [(3000, 300), (2049, 4000)])
@pytest.mark.parametrize("variant", sc.VARIANTS)
@pytest.mark.parametrize("path", ["hybrid", "lazy", "wide"])
def test_propose_score_variants(path, variant, pre, post):
    anchors, s, de, orois, oidx = _propose_reference(variant, pre, post)
    with _lib.kernel_path("propose", path):
        rois, idx, cnt = ops.propose(torch.from_numpy(s)[None].to(DEV), torch.from_numpy(de)[None].to(DEV),
                                     img_w=sc.IMG_W, img_h=sc.IMG_H, pre_nms=pre, post_nms=post,
                                     anchors=torch.from_numpy(anchors).to(DEV))
        k = int(cnt[0])
    assert k == len(oidx), (k, len(oidx))
    assert np.array_equal(idx[0, :k].cpu().numpy(), oidx)
    assert np.array_equal(rois[0, :k].cpu().numpy(), orois)
    assert (idx[0, k:] == -1).all()


def _eval_case():
    """One image, one class, three gt, each claimed by two detections whose order
    only torch's equalities get right: (-0.0, slot 0) before (+0.0, slot 1);
    a sign-set NaN in slot 3 before 1.0 in slot 2; a sign-clear NaN in slot 4
    before a sign-set NaN in slot 5 (NaNs are equal, the slot decides)."""
    gt = [((10, 10, 110, 110), 1, 0), ((300, 300, 400, 420), 1, 0), ((500, 10, 600, 110), 1, 0)]
    nan_neg, nan_pos = sc.from_bits([0xffc00000, 0x7fc00000])
    det = [((10, 10, 110, 110), 1, -0.0), ((11, 10, 110, 110), 1, 0.0),
           ((300, 300, 400, 420), 1, 1.0), ((301, 300, 400, 420), 1, 0.0),
           ((500, 10, 600, 110), 1, 0.0), ((501, 10, 600, 110), 1, 0.0)]
    c = eval_ref._case(det, gt, M=8, G=4)
    c["det_scores"][0, 3], c["det_scores"][0, 4], c["det_scores"][0, 5] = nan_neg, nan_pos, nan_neg
    assert sc.bits_of(c["det_scores"][0, :6]).tolist() == [0x80000000, 0, 0x3f800000, 0xffc00000, 0x7fc00000,
                                                            0xffc00000]
    return c


def test_eval_score_order():
    c = _eval_case()
    ref = eval_ref.State(2, 8)
    ref.update(*eval_ref.args(c))
    assert ref.rec_flag[:6].tolist() == [1, 0, 0, 1, 1, 0], "precondition: torch's order decides every claim"
    state = ops.eval_state(2, 8)
    db, dl, ds, dc, gb, gl, gd = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in eval_ref.args(c))
    ops.eval_update((db, dl, ds, dc), gb, gl, gd, state=state)
    hdr, key, flag, image = (t.cpu().numpy() for t in state)
    assert np.array_equal(hdr, ref.hdr)
    assert np.array_equal(flag[:6], ref.rec_flag[:6]), (flag[:6], ref.rec_flag[:6])
    assert np.array_equal(key.view(np.uint64)[:6], ref.rec_key[:6])
    ap, mean, skey = ops.eval_ap(state, 6, return_sorted=True)
    wap, wmean, wsk, _ = ref.ap()
    assert np.array_equal(skey.cpu().numpy().view(np.uint64), wsk)
    # records in sorted order: NaN NaN NaN 1.0 0.0 0.0 -> TP FP(slot 5) .. ; both sides add at most 6 terms
    assert abs(float(ap[1]) - wap[1]) <= 6 * 2.0 ** -52, (float(ap[1]), wap[1])
