"""The FPN proposal layer without a GPU: the reference (tests/fpn_proposals_ref.py) held to
hand-computed results and to each named case's precondition, the anchor helpers against
torchvision's documented values, the logit form of the score threshold against
``torch.sigmoid(x) >= score_thresh``, and the C-ABI's symbols, refusals and kernel names
(host only: a refused call never reaches a launch)."""
import ctypes

import numpy as np
import pytest
import torch

import fpn_proposals_cases as fc
import fpn_proposals_ref as ref
from replication_faster_rcnn_amd import _lib, ops

F = np.float32


# ------------------------------------------------------------------ anchors
def test_anchor_bases_documented_values():
    b = ops.pyramid_anchor_bases((32,), (0.5, 1.0, 2.0))
    assert b.dtype == torch.float32
    assert b.tolist() == [[-23, -11, 23, 11], [-16, -16, 16, 16], [-11, -23, 11, 23]]
    per_level = ops.pyramid_anchor_bases(((32,), (64,)), ((0.5, 1.0, 2.0),) * 2)
    assert len(per_level) == 2 and torch.equal(per_level[0], b)
    assert per_level[1].tolist() == [[-45, -23, 45, 23], [-32, -32, 32, 32], [-23, -45, 23, 45]]
    two = ops.pyramid_anchor_bases((32, 64), (0.5, 1.0))           # rows ratio-major
    assert two.tolist() == [[-23, -11, 23, 11], [-45, -23, 45, 23], [-16, -16, 16, 16], [-32, -32, 32, 32]]


def test_pyramid_anchors_by_hand():
    base = torch.tensor([[-4.0, -2.0, 4.0, 2.0], [0.0, 0.0, 1.5, 2.5]])
    (a,) = ops.pyramid_anchors([base], [(10, 3)], [(2, 3)])        # stride_h 10, stride_w 3, H 2, W 3
    assert a.shape == (12, 4) and a.dtype == torch.float32
    for y in range(2):
        for x in range(3):
            for k in range(2):
                want = base[k] + torch.tensor([3.0 * x, 10.0 * y, 3.0 * x, 10.0 * y])
                assert torch.equal(a[(y * 3 + x) * 2 + k], want), (y, x, k)


# ---------------------------------------------------------------- reference
def test_reference_by_hand():
    base = [torch.tensor([[0.0, 0.0, 8.0, 8.0]])]
    anchors = ops.pyramid_anchors(base, [(16, 16)], [(1, 4)])
    obj = [torch.tensor([1.0, 3.0, 2.0, 0.5]).view(1, 1, 1, 4)]
    d = torch.zeros(1, 4, 1, 4)
    d[0, 0, 0, 1] = 0.5                  # anchor 1: centre moves by half a width
    d[0, 2, 0, 2] = 50.0                 # anchor 2: dw clamped to log(1000 / 16): 500 wide, clipped to the image
    d[0, 3, 0, 3] = float("-inf")        # anchor 3: zero height
    b, s, lv, ai, cnt, rois = ref.reference(obj, [d], anchors, [(8.0, 60.0)], pre=4, post=5, nms_thresh=0.7)
    assert cnt.tolist() == [3] and ai[0].tolist() == [1, 2, 0, -1, -1] and lv[0].tolist() == [0, 0, 0, -1, -1]
    assert s[0].tolist() == [3.0, 2.0, 1.0, -np.inf, -np.inf]
    assert b[0, 0].tolist() == [20.0, 0.0, 28.0, 8.0] and b[0, 2].tolist() == [0.0, 0.0, 8.0, 8.0]
    half = F(0.5) * (ref.orc.exp_cr(ref.BBOX_XFORM_CLIP) * F(8))
    assert half > 240 and b[0, 1].tolist() == [0.0, 0.0, 60.0, 8.0] and F(36) + half > 60
    assert rois[:3, 0].tolist() == [0, 0, 0] and rois[3:].tolist() == [[-1, 0, 0, 0, 0]] * 2
    assert np.array_equal(rois[:3, 1:], b[0, :3]) and (b[0, 3:] == 0).all()
    # the same with pre = 2: selection comes before the filters, so anchor 0 never gets a slot
    _, _, _, ai, cnt, _ = ref.reference(obj, [d], anchors, [(8.0, 60.0)], pre=2, post=5)
    assert cnt.tolist() == [2] and ai[0, :2].tolist() == [1, 2]
    # a NaN logit is selected first and then dropped: with pre = 2 only anchor 1 is left
    obj[0][0, 0, 0, 3] = float("nan")
    _, _, _, ai, cnt, _ = ref.reference(obj, [d], anchors, [(8.0, 60.0)], pre=2, post=5)
    assert cnt.tolist() == [1] and ai[0, 0] == 1


def test_decode_clamp_value():
    assert ref.BBOX_XFORM_CLIP.view(np.uint32) == F(np.log(1000.0 / 16.0)).view(np.uint32) == 1082413897


@pytest.mark.parametrize("case", fc.CASES, ids=repr)
def test_case_precondition(case):
    r = case.reference()
    assert r[0].shape == (case.N, case.post, 4) and r[5].shape == (case.N * case.post, 5)
    for n in range(case.N):                      # padding and the rois' layout, on every case
        c = int(r[4][n])
        assert (r[2][n, c:] == -1).all() and (r[3][n, c:] == -1).all() and np.isneginf(r[1][n, c:]).all()
        rows = r[5][n * case.post:(n + 1) * case.post]
        assert (rows[:c, 0] == n).all() and np.array_equal(rows[:c, 1:], r[0][n, :c]) and (rows[c:, 0] == -1).all()
        lg, lv, ai = r[1][n, :c], r[2][n, :c].astype(np.int64), r[3][n, :c].astype(np.int64)
        for i in range(c - 1):                   # (logit descending, level ascending, anchor ascending)
            assert lg[i] > lg[i + 1] or (lg[i] == lg[i + 1] and (lv[i], ai[i]) < (lv[i + 1], ai[i + 1])), (n, i)
    if case.check is not None:
        case.check(case, r)


def test_cases_cover_both_branches_and_their_edge():
    anchors = {case.K * h * w for case in fc.CASES for h, w in case.grids}
    assert {fc.SORT_CAP - 1, fc.SORT_CAP, fc.SORT_CAP + 1} <= anchors
    assert any(set(c.branches) == {"sort", "select"} for c in fc.CASES)
    assert ops.FPN_SORT_CAP == fc.SORT_CAP


# ------------------------------------------------------- the logit threshold
@pytest.mark.parametrize("thresh", [0.05, 0.5, 0.7, 0.95])
def test_logit_threshold_is_the_sigmoid_test(thresh):
    t = ops.logit_threshold(thresh)
    assert ops.logit_threshold(thresh) == t                     # cached
    ti = int(torch.tensor(t, dtype=torch.float32).view(torch.int32))
    near = torch.arange(ti - 1000, ti + 1001, dtype=torch.int64).to(torch.int32).view(torch.float32)
    assert not torch.isnan(near).any()
    x = torch.cat([near, torch.randn(10 ** 6, generator=torch.Generator().manual_seed(int(thresh * 100))) * 6,
                   torch.tensor([float("inf"), float("-inf"), float("nan"), 0.0, -0.0])])
    assert torch.equal(x >= t, torch.sigmoid(x) >= thresh)
    below = float(np.nextafter(F(t), F(-np.inf)))
    assert bool(torch.sigmoid(torch.tensor(t)) >= thresh) and not bool(torch.sigmoid(torch.tensor(below)) >= thresh)


def test_logit_threshold_ends():
    assert ops.logit_threshold(0.0) == float("-inf") and ops.logit_threshold(-1.0) == float("-inf")
    assert ops.logit_threshold(1.5) != ops.logit_threshold(1.5)             # NaN: nothing passes
    assert ops.logit_threshold(1.0) <= 20.0                                 # sigmoid rounds to 1 well before +inf
    assert ops._f32_from_ordinal(ops._f32_ordinal(-0.0)) == 0.0 and ops._f32_ordinal(-0.0) == -1
    assert ops._f32_ordinal(0.0) == 0 and ops._f32_ordinal(float("-inf")) < ops._f32_ordinal(-1.0) < -1


# ------------------------------------------------------------------ C-ABI
def _lvl(vals):
    return (ctypes.c_int * len(vals))(*vals)


def test_capi_symbols_exported():
    lib = _lib.load(require_gpu=False)
    for name in ("frcnn_propose_multi_workspace_size", "frcnn_propose_multi_t", "frcnn_propose_multi_kernel"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    with open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "frcnn_capi.h")) as f:
        header = f.read()
    for name in ("frcnn_propose_multi_workspace_size(", "frcnn_propose_multi_t(", "frcnn_propose_multi_kernel("):
        assert name in header


def test_capi_workspace_size_and_limits():
    lib = _lib.load(require_gpu=False)
    size = lib.frcnn_propose_multi_workspace_size
    ok = size(2, 2, 3, _lvl([10, 5]), _lvl([12, 6]), 100, 50)
    assert ok > 0 and ok % 256 == 0
    bad = [(0, 2, 3, [10], [12], 100, 50, "n_levels"), (9, 2, 3, [1] * 9, [1] * 9, 100, 50, "n_levels"),
           (1, 0, 3, [10], [12], 100, 50, "N must"), (1, 1025, 3, [10], [12], 100, 50, "N must"),
           (1, 2, 0, [10], [12], 100, 50, "K must"), (1, 2, 33, [10], [12], 100, 50, "K must"),
           (1, 2, 3, [0], [12], 100, 50, "H and W"), (1, 2, 3, [10], [-1], 100, 50, "H and W"),
           (1, 2, 4, [2048], [2048], 100, 50, "2^24"), (1, 2, 3, [10], [12], 0, 50, "pre_nms_top_n"),
           (1, 2, 3, [10], [12], 2049, 50, "pre_nms_top_n"), (1, 2, 3, [10], [12], 100, 0, "post_nms_top_n"),
           (1, 2, 3, [10], [12], 100, 4097, "post_nms_top_n")]
    for L, N, K, H, W, pre, post, word in bad:
        assert size(L, N, K, _lvl(H), _lvl(W), pre, post) == 0, word
        assert word in lib.frcnn_last_error().decode(), (word, lib.frcnn_last_error().decode())
    assert size(1, 2, 3, None, _lvl([3]), 10, 10) == 0 and "null" in lib.frcnn_last_error().decode()
    assert size(1, 1, 1, _lvl([1]), _lvl([1]), 2048, 4096) > 0        # the limits themselves are accepted


def test_capi_call_refusals_before_any_launch():
    """Every argument error returns FRCNN_EINVAL with a message; none of these reaches a HIP call."""
    lib = _lib.load(require_gpu=False)
    H, W, sh, sw = _lvl([4]), _lvl([5]), _lvl([8]), _lvl([8])
    fake = 4096                                                    # a well-aligned non-NULL address, never read
    ptrs = (ctypes.c_void_p * 1)(fake)
    nulls = (ctypes.c_void_p * 1)(None)

    def call(dtype=0, L=1, obj=ptrs, dlt=ptrs, base=ptrs, H=H, W=W, sh=sh, sw=sw, N=1, K=2, sizes=fake, pre=10,
             post=10, outs=(fake,) * 6, ws=fake, ws_bytes=1 << 30):
        return lib.frcnn_propose_multi_t(dtype, L, obj, dlt, base, H, W, sh, sw, N, K, sizes, pre, post, 0.7,
                                         float("-inf"), 1e-3, *outs, ws, ws_bytes, None)

    for kw, word in ((dict(dtype=3), "dtype"), (dict(dtype=-1), "dtype"), (dict(L=0), "n_levels"),
                     (dict(L=9), "n_levels"), (dict(K=33), "K must"), (dict(pre=2049), "pre_nms_top_n"),
                     (dict(post=4097), "post_nms_top_n"), (dict(obj=None), "null"), (dict(dlt=nulls), "null pointer"),
                     (dict(base=nulls), "null pointer"), (dict(sh=None), "null"), (dict(sizes=None), "image_sizes"),
                     (dict(outs=(fake, None, fake, fake, fake, fake)), "output"), (dict(ws=None), "workspace"),
                     (dict(ws_bytes=16), "workspace"), (dict(sh=_lvl([0])), "strides"),
                     (dict(H=_lvl([3]), sh=_lvl([1 << 23])), "2^24"),
                     (dict(dtype=1, obj=(ctypes.c_void_p * 1)(fake + 1)), "aligned"),
                     (dict(base=(ctypes.c_void_p * 1)(fake + 4)), "16-byte"), (dict(ws=fake + 64), "256-byte")):
        assert call(**kw) != 0, kw
        assert word in lib.frcnn_last_error().decode(), (kw, lib.frcnn_last_error().decode())


@pytest.mark.parametrize("case", fc.CASES, ids=repr)
def test_kernel_names_follow_the_plan(case):
    shapes = [tuple(o.shape) for o in case.objectness]
    for dtype, elem in ((torch.float32, "ElemF32"), (torch.float16, "ElemF16"), (torch.bfloat16, "ElemBF16")):
        name = ops.propose_multilevel_kernel(shapes, dtype, case.pre, case.post)
        assert name == (f"fpn_select_decode_kernel<{elem}>[{','.join(case.branches)}] fpn_nms_mask_kernel "
                        "fpn_sweep_kernel fpn_merge_kernel")


def test_module_picks_counts_by_mode():
    from replication_faster_rcnn_amd.rpn import MultiLevelProposals
    m = MultiLevelProposals({"training": 2000, "testing": 1000}, {"training": 1500, "testing": 300}, 0.7)
    assert (m.pre_nms_top_n(), m.post_nms_top_n()) == (2000, 1500)
    m.eval()
    assert (m.pre_nms_top_n(), m.post_nms_top_n()) == (1000, 300)
    with pytest.raises(RuntimeError, match="pre_nms_top_n"):
        MultiLevelProposals(2000, {"training": 1, "testing": 1}, 0.7)
