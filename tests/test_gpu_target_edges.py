"""Target assignment on the HIP path at its edges: the case table of
tests/target_cases.py (ties, exact thresholds, interleaved padding, sizes at
wave / block / round edges, non-finite boxes, non-default sampling parameters
and normalisation) and the documented limits, each against the oracle's
per-image loop on numpy's global RNG -- never against the code under test.
Needs an MI355X.

Bars (tests/test_gpu_targets.py): labels, argmax, pos / neg membership, sample
order, counts and the MT19937 key and position bit-exact; max IoU equal as
numbers with NaN positions equal; regression targets within 1e-12 relative
with non-finite positions equal.

The batched ops return fp64 targets throughout; where the reference returns
``np.zeros_like(anchor)`` (no label positive) they hold zeros, and the per-image
drop-in classes return the reference's dtype as well.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_numpy as orc
from replication_faster_rcnn_amd import _lib, targets
from replication_faster_rcnn_amd import utils as U

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import target_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture
def sampler_path(request):
    _lib.set_path("sampler", request.param)
    yield request.param
    _lib.set_path("sampler", "auto")


def _with_paths(cases, both):
    """(case name, sampler path): auto for every case, the walk too for `both`."""
    return [(c.name, p) for c in cases for p in (("auto", "walk") if c.name.startswith(both) else ("auto",))]


def _np(t):
    return t.cpu().numpy()


def _assert_reg(got, want, atol, what):
    want = np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), f"{what}: non-finite positions"
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), f"{what}: non-finite values"
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-12, atol=atol, err_msg=what)


def _assert_rng(want, what):
    st = np.random.get_state()
    assert st[2] == want[2], f"{what}: MT19937 position {st[2]} != {want[2]}"
    assert np.array_equal(st[1], want[1]), f"{what}: MT19937 key"


def _assert_anchor(case, out, reg, lab, am=None, mx=None, what=""):
    for i, im in enumerate(out["images"]):
        w = f"{case.name} {what} image {i}"
        assert np.array_equal(_np(lab[i]), im["label"]), f"{w}: labels"
        if am is not None:
            assert np.array_equal(_np(am[i]), im["argmax"]), f"{w}: argmax"
            assert np.array_equal(_np(mx[i]), im["max_iou"], equal_nan=True), f"{w}: max IoU"
        _assert_reg(_np(reg[i]), im["reg"], 0, f"{w}: regression targets")
    _assert_rng(out["rng_out"], f"{case.name} {what}")


@pytest.mark.parametrize("name,sampler_path", _with_paths(tc.ANCHOR_CASES, "sampling"), indirect=["sampler_path"])
def test_anchor_case_vs_oracle(rng_guard, name, sampler_path):
    """anchor_targets(internals=True), and anchor_targets_prepare + _sample,
    batched over the case's images, against the oracle's per-image loop."""
    case = tc.BY_NAME[name]
    out = tc.anchor_oracle(case)
    case.check(case, out)
    np.random.set_state(out["rng_in"])
    reg, lab, am, mx = targets.anchor_targets(case.boxes, case.labels, case.anchors, internals=True, **case.kw)
    _assert_anchor(case, out, reg, lab, am, mx, "one call")
    kw = dict(case.kw)
    draw = {k: kw.pop(k) for k in ("n_sample", "pos_ratio") if k in kw}
    np.random.set_state(out["rng_in"])
    plan = targets.anchor_targets_prepare(case.boxes, case.labels, case.anchors, **kw)
    reg, lab = targets.anchor_targets_sample(plan, **draw)
    _assert_anchor(case, out, reg, lab, what="prepare + sample")


def _assert_proposal(case, out, s_roi, s_reg, s_lab, s_cnt, what):
    for i, im in enumerate(out["images"]):
        w = f"{case.name} {what} image {i}"
        k = int(s_cnt[i])
        assert k == len(im["roi"]), f"{w}: count {k} != {len(im['roi'])}"
        assert np.array_equal(_np(s_roi[i, :k]), im["roi"]), f"{w}: samples"
        assert np.array_equal(_np(s_lab[i, :k]), im["label"]), f"{w}: labels"
        _assert_reg(_np(s_reg[i, :k]), im["reg"], 1e-15, f"{w}: regression targets")
    _assert_rng(out["rng_out"], f"{case.name} {what}")


@pytest.mark.parametrize("name,sampler_path", _with_paths(tc.PROPOSAL_CASES, "rounding"), indirect=["sampler_path"])
def test_proposal_case_vs_oracle(rng_guard, name, sampler_path):
    """proposal_targets, and the prepare / draw / finish split, batched over the
    case's images, against the oracle's per-image loop."""
    case = tc.BY_NAME[name]
    out = tc.proposal_oracle(case)
    case.check(case, out)
    rois = torch.from_numpy(case.rois)
    cnt = torch.from_numpy(np.asarray(case.rcount, np.int32))
    mean, std = case.norm
    np.random.set_state(out["rng_in"])
    got = targets.proposal_targets(rois, cnt, case.boxes, case.labels, reg_normalize_mean=mean,
                                   reg_normalize_std=std, **case.kw)
    _assert_proposal(case, out, *got, "one call")
    kw = dict(case.kw)
    pos_ratio = kw.pop("pos_ratio", 0.5)
    np.random.set_state(out["rng_in"])
    plan = targets.proposal_targets_prepare(rois, cnt, case.boxes, case.labels, **kw)
    count = targets.proposal_targets_draw(plan, pos_ratio=pos_ratio)
    s_roi, s_reg, s_lab = targets.proposal_targets_finish(plan, count, reg_normalize_mean=mean, reg_normalize_std=std)
    _assert_proposal(case, out, s_roi, s_reg, s_lab, count, "prepare / draw / finish")


DROPIN_ANCHOR = ["thr_equal", "thr_equal-0.3", "sampling-1-0.5", "sampling-8-0.0"]


@pytest.mark.parametrize("name", DROPIN_ANCHOR)
def test_anchor_dropin_class(rng_guard, name):
    """utils.AnchorTargetCreator with the case's constructor arguments: values,
    dtypes and shapes of the oracle -- fp32 zeros when no label is positive
    (utils/utils.py:146-150), with gt present too."""
    case = tc.BY_NAME[name]
    out = tc.anchor_oracle(case)
    np.random.set_state(out["rng_in"])
    at = U.AnchorTargetCreator(**case.kw)
    for i, im in enumerate(out["images"]):
        reg, lab, am, mx = at(case.gt(i), case.anchors, return_internals=True)
        assert lab.dtype == im["label"].dtype and np.array_equal(lab, im["label"])
        assert reg.dtype == im["reg"].dtype and reg.shape == im["reg"].shape, (reg.dtype, im["reg"].dtype)
        _assert_reg(reg, im["reg"], 0, f"{name} image {i}")
        assert np.array_equal(am, im["argmax"]) and np.array_equal(mx, im["max_iou"], equal_nan=True)
        st = np.random.get_state()
        assert st[2] == im["rng_pos"] and np.array_equal(st[1], im["rng_key"])
    if name.startswith("sampling"):
        assert out["images"][0]["reg"].dtype == np.float32 and not (out["images"][0]["label"] == 1).any()


@pytest.mark.parametrize("name", [c.name for c in tc.PROPOSAL_CASES if c.name.startswith("rounding")])
def test_proposal_dropin_class(rng_guard, name):
    """utils.ProposalTargetCreator with the case's constructor arguments."""
    case = tc.BY_NAME[name]
    out = tc.proposal_oracle(case)
    np.random.set_state(out["rng_in"])
    pt = U.ProposalTargetCreator(**case.kw)
    for i, im in enumerate(out["images"]):
        roi, gt, gl = case.image(i)
        got = pt(torch.from_numpy(roi), gt, gl, *case.norm)
        for g, key in zip(got, ("roi", "reg", "label")):
            assert g.dtype == im[key].dtype and g.shape == im[key].shape, (key, g.dtype, g.shape)
        assert np.array_equal(got[0], im["roi"]) and np.array_equal(got[2], im["label"])
        _assert_reg(got[1], im["reg"], 1e-15, f"{name} image {i}")
        st = np.random.get_state()
        assert st[2] == im["rng_pos"] and np.array_equal(st[1], im["rng_key"])


# ---------------------------------------------------------------------- limits
def test_gt_limit():
    """G = 256 works (g_sizes-256 above compares it); G = 257 raises."""
    case = tc.BY_NAME["g_sizes-256"]
    boxes = np.concatenate([case.boxes, case.boxes[:, :1]], axis=1)
    labels = np.ones(boxes.shape[:2])
    assert boxes.shape[1] == 257
    with pytest.raises(RuntimeError):
        targets.anchor_targets(boxes, labels, case.anchors)
    rois = torch.zeros((1, 8, 4))
    with pytest.raises(RuntimeError):
        targets.proposal_targets(rois, torch.tensor([8], dtype=torch.int32), boxes, labels)


def test_anchor_n_sample_limit():
    """n_sample - n_pos > 4096 survivors of the negatives' call raises; 4096 works
    (sampling-4096-0.5 above, and here with pos_ratio 0)."""
    case = tc.BY_NAME["dup_anchor_ties"]
    with pytest.raises(RuntimeError):
        targets.anchor_targets(case.boxes, case.labels, case.anchors, n_sample=4097, pos_ratio=0.0)
    with pytest.raises(RuntimeError):
        targets.anchor_targets(case.boxes, case.labels, case.anchors, n_sample=8194, pos_ratio=0.5)


def test_proposal_row_limit(rng_guard):
    """Rp + G == 4096 (one image, every row valid: the recorded swaps of one
    choice() call fill its jrec row) equals the oracle; 4097 raises."""
    r = np.random.default_rng(41)
    Rp, G = 4064, 32
    rois = tc._rand_rois(r, Rp + 1, 600)
    gt = tc._int_boxes(r, G, 600, 600, lo=40)
    gl = r.integers(1, 21, G).astype(np.float64)
    np.random.seed(42)
    s_roi, s_reg, s_lab, s_cnt = targets.proposal_targets(torch.from_numpy(rois[None, :Rp]),
                                                          torch.tensor([Rp], dtype=torch.int32), gt[None], gl[None])
    st = np.random.get_state()
    np.random.seed(42)
    o_roi, o_reg, o_lab = orc.proposal_target(rois[:Rp], gt, gl)
    k = int(s_cnt[0])
    assert k == len(o_roi) == 128
    assert np.array_equal(_np(s_roi[0, :k]), o_roi) and np.array_equal(_np(s_lab[0, :k]), o_lab)
    _assert_reg(_np(s_reg[0, :k]), o_reg, 1e-15, "Rp + G == 4096")
    _assert_rng(st, "Rp + G == 4096")
    with pytest.raises(RuntimeError):
        targets.proposal_targets(torch.from_numpy(rois[None]), torch.tensor([Rp + 1], dtype=torch.int32),
                                 gt[None], gl[None])


@pytest.mark.parametrize("N", [128, 129])
def test_anchor_batch_limit_of_chip_wide_draws(rng_guard, N):
    """N = 128 is the last batch the chip-wide draws plan (256 calls); N = 129
    has a walk-only workspace (no draw status).  Both equal the oracle's
    per-image loop, RNG state included (A = 65, G = 2, n_sample = 8 so that
    every image draws)."""
    r = np.random.default_rng(43)
    anchors = orc.generate_anchors(orc.generate_anchor_base(), 16, 16, 16)[:65]
    boxes = np.stack([tc._int_boxes(r, 2, 200, 200, lo=60) for _ in range(N)])
    labels = np.ones((N, 2))
    labels[3, 1] = -1
    np.random.seed(44)
    plan = targets.anchor_targets_prepare(boxes, labels, anchors)
    reg, lab = targets.anchor_targets_sample(plan, n_sample=8)
    status = targets.anchor_targets_draw_status(plan)
    st = np.random.get_state()
    assert (status is None) == (N == 129), status
    reg, lab = _np(reg), _np(lab)
    np.random.seed(44)
    for i in range(N):
        oreg, olab = orc.anchor_target(boxes[i, labels[i] != -1], anchors, n_sample=8)
        assert np.array_equal(lab[i], olab), f"image {i}"
        _assert_reg(reg[i], oreg, 0, f"image {i}")
        assert (olab == 1).sum() <= 4 and (olab >= 0).sum() == 8
    _assert_rng(st, f"N = {N}")


def _draws_one_pass_vs_two(anchors, boxes, labels, rois, cnt, steps=2):
    """frcnn_target_draws (auto) against anchor_targets_draw then
    proposal_targets_draw under the walk, `steps` chained steps on a device
    stream: every output and the RNG state after each step.  Returns the last
    one-pass draw status."""
    dev = torch.device("cuda")
    anchors, boxes, labels, rois, cnt = (torch.as_tensor(x).to(dev) for x in (anchors, boxes, labels, rois, cnt))

    def run(one_pass, path):
        _lib.set_path("sampler", path)
        try:
            np.random.seed(55)
            rng, _ = U.rng_state_to_device(dev)
            outs, status = [], None
            for _ in range(steps):
                ap = targets.anchor_targets_prepare(boxes, labels, anchors)
                pp = targets.proposal_targets_prepare(rois, cnt, boxes, labels)
                if one_pass:
                    c = targets.target_draws(ap, pp, rng)
                    status = targets.anchor_targets_draw_status(ap)
                else:
                    targets.anchor_targets_draw(ap, rng=rng)
                    c = targets.proposal_targets_draw(pp, rng=rng)
                outs.append(tuple(targets.anchor_targets_finish(ap)) + tuple(targets.proposal_targets_finish(pp, c))
                            + (c, rng.clone()))
            torch.cuda.synchronize()
            return outs, status
        finally:
            _lib.set_path("sampler", "auto")

    ref, _ = run(False, "walk")
    got, status = run(True, "auto")
    names = ("anchor reg", "anchor labels", "sample_roi", "gt_roi_reg", "gt_roi_label", "count", "rng")
    for k, (a, b) in enumerate(zip(ref, got)):
        for nm, x, y in zip(names, a, b):
            assert torch.equal(x, y), f"step {k}: {nm} (draw status {status})"
    assert not torch.equal(ref[0][-1], ref[1][-1]), "the stream advances"
    return status


def _draw_inputs(seed, N, Rp, G=4):
    r = np.random.default_rng(seed)
    boxes = np.stack([tc._int_boxes(r, G, 112, 80, lo=30) for _ in range(N)])
    labels = r.integers(1, 21, (N, G)).astype(np.float64)
    rois = np.stack([tc._rand_rois(r, Rp, 112) for _ in range(N)])
    cnt = np.full(N, Rp, np.int32)
    cnt[N // 2] = Rp // 2
    return tc.base_grid(), boxes, labels, rois, cnt


@pytest.mark.parametrize("N", [64, 65])
def test_target_draws_batch_limit(rng_guard, N):
    """The combined pass holds 2 * (N + N) <= 256 calls: N = 64 is planned
    chip-wide, N = 65 walks.  Either way it equals the two calls."""
    _draws_one_pass_vs_two(*_draw_inputs(45, N, 40))


def test_target_draws_small_anchor_plan_large_proposal_streams(rng_guard):
    """The combined pass plans in the AnchorTarget workspace, sized for N * A
    steps; with A = 315 and 2,000 RoIs per image the ProposalTarget streams are
    several times that.  Whether the plan holds or refuses (status['fail'], in
    the message), every output and the RNG state equal the two-call walk."""
    status = _draws_one_pass_vs_two(*_draw_inputs(46, 4, 2000))
    assert status is not None


def test_anchor_call_over_the_chip_wide_step_limit(rng_guard):
    """One choice() call of more than 65,535 steps (70,200 anchors, one small gt:
    ~70k negatives): draw_setup_kernel refuses the plan (fail != 0) and the walk
    behind it draws.  Labels and RNG state equal the oracle under auto."""
    anchors = orc.generate_anchors(orc.generate_anchor_base(anchor_scales=(2, 4, 8, 16, 32)), 16, 78, 60)
    assert len(anchors) == 70200
    gt = np.array([[[400., 500., 440., 560.]]])
    np.random.seed(47)
    plan = targets.anchor_targets_prepare(gt, np.ones((1, 1)), anchors)
    reg, lab = targets.anchor_targets_sample(plan)
    status = targets.anchor_targets_draw_status(plan)
    st = np.random.get_state()
    np.random.seed(47)
    oreg, olab, _, omx = orc.anchor_target(gt[0], anchors, return_internals=True)
    assert (omx < 0.3).sum() - 2 > 65535, "more than 65,535 steps in the negatives' call"
    assert np.array_equal(_np(lab[0]), olab)
    _assert_reg(_np(reg[0]), oreg, 0, "70,200 anchors")
    _assert_rng(st, "70,200 anchors")
    assert status["fail"] != 0, status
