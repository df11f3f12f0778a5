"""The proposal layer and ops.nms at every launch-plan branch and sweep edge of
tests/propose_plan_cases.py (DESIGN.md "Proposal launch-plan branches") vs the oracle.
Needs an MI355X.

Every case runs under each path listed for it (``_lib.kernel_path("propose", ...)``).
Count, anchor indices and boxes are compared with the oracle bit for bit, the slots past
the count must be -1 / 0.  Each case runs twice: first into fresh outputs over the
cached workspace as the earlier cases left it, then into caller-owned ``out`` buffers
filled with a pattern and a workspace filled with 0xFF -- the library zeroes nothing,
every launch writes the state the next one reads (rank_scatter_kernel resets ss.count /
ss.done / ss.prehit, the first-chunk kernel writes hw.cc / hw.P for every image), so a
carry from another case or a read of a word no launch wrote shows as a difference.

There is no kernel-name query for proposals: that a case reaches its branch is what
tests/test_propose_plan_cases_cpu.py asserts on the restated plan."""
import numpy as np
import pytest
import torch

import propose_plan_cases as ppc
from oracle import ref_numpy as orc
from propose_plan_cases import CASES
from replication_faster_rcnn_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def runs(cases):
    return pytest.mark.parametrize("case,path", [(c, p) for c in cases for p in c.paths],
                                   ids=lambda v: v if isinstance(v, str) else v.name)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)        # (a copy: the table's arrays are read-only)


def propose(case, images=None, poisoned=False):
    """ops.propose over the case's images (``images``: a selection, in that order)."""
    anchors, scores, deltas = case.inputs()
    sel = list(range(case.N)) if images is None else list(images)
    n = len(sel)
    kw = dict(img_w=ppc.IMG, img_h=ppc.IMG, pre_nms=case.pre, post_nms=case.post, nms_thresh=ppc.THR,
              anchors=dev(anchors))
    if poisoned:
        size = _lib.cached_workspace("propose", 1, _lib.device()).numel()      # grown by the first run
        kw["workspace"] = torch.full((size,), 0xFF, dtype=torch.uint8, device=DEV)
        kw["out"] = (torch.full((n, case.post, 4), 7.5, device=DEV),
                     torch.full((n, case.post), 12345, dtype=torch.int32, device=DEV),
                     torch.full((n,), -7, dtype=torch.int32, device=DEV))
    rois, idx, cnt = ops.propose(dev(scores[sel]), dev(deltas[sel]), **kw)
    return rois.cpu().numpy(), idx.cpu().numpy(), cnt.cpu().numpy()


def assert_equals_oracle(case, got, images=None, what=""):
    rois, idx, cnt = got
    sel = list(range(case.N)) if images is None else list(images)
    assert rois.shape == (len(sel), case.post, 4) and idx.shape == (len(sel), case.post)
    for j, n in enumerate(sel):
        orois, oidx = case.reference()[n]
        k = int(cnt[j])
        assert k == len(oidx), (what, n, k, len(oidx))
        assert np.array_equal(idx[j, :k].astype(np.int64), oidx), (what, n)
        assert np.array_equal(rois[j, :k].view(np.uint32), orois.view(np.uint32)), (what, n)
        assert (idx[j, k:] == -1).all() and (rois[j, k:].view(np.uint32) == 0).all(), (what, n, "padding")


def check(case, path, images=None):
    with _lib.kernel_path("propose", path):
        first = propose(case, images)
        second = propose(case, images, poisoned=True)
    assert_equals_oracle(case, first, images, "first run")
    assert_equals_oracle(case, second, images, "caller buffers, workspace of 0xFF")


def group(*names):
    return [c for c in CASES if c.group in names]


@runs(group("ladder"))
def test_register_ladder(case, path):
    """A on both sides of each kpt step and of kFusedMaxA; the last register slot's anchors
    rank among the first ten."""
    check(case, path)


@runs(group("first"))
def test_first_chunk(case, path):
    check(case, path)


@runs(group("cont"))
def test_continuation_geometry(case, path):
    check(case, path)


@runs(group("trunc"))
def test_truncation_inside_a_block(case, path):
    check(case, path)


@runs(group("fixed"))
def test_fixed_point_chains(case, path):
    check(case, path)


@runs(group("route"))
def test_suppression_routes(case, path):
    check(case, path)


@runs(group("stage", "sort", "select"))
def test_stage_edges_sort_and_select(case, path):
    check(case, path)


@runs(group("auto"))
def test_auto_on_both_sides_of_its_rule(case, path):
    """(N, post) = (3, 1000), (3, 1001), (4, 1001) under ``auto``, each against the oracle.
    With no kernel-name query these runs show only that ``auto`` is right on both sides of
    ``N >= 4 || post <= 1000``, not which side it took; the restated selector
    (propose_plan_cases.use_fused) documents the intent."""
    check(case, path)


# ---------------------------------------------------------------- the mixed batch
@runs(group("mixed"))
def test_mixed_batch(case, path):
    """Unlike images in one call, the same images alone and the batch reversed: every image
    equals the oracle each time (so it does not depend on its batch mates)."""
    check(case, path)
    check(case, path, images=range(case.N - 1, -1, -1))
    for n in range(case.N):
        check(case, path, images=[n])


# ------------------------------------------------------------------------ ops.nms
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("n", ppc.NMS_SIZES)
def test_nms_stage_edges(n, where):
    boxes, scores, keep = ppc.nms_case(n)
    b, s = torch.from_numpy(boxes.copy()), torch.from_numpy(scores.copy())
    if where == "device":
        b, s = b.to(DEV), s.to(DEV)
    for _ in range(2):      # (the second call finds the first one's workspace)
        got = ops.nms(b, s, ppc.THR)
        assert got.dtype == torch.int64 and got.device == b.device
        assert np.array_equal(got.cpu().numpy(), keep)
    assert np.array_equal(orc.nms(boxes, scores, ppc.THR), keep)
