"""The restatement tests/box_head_ref.py of the pyramid box head's training half against torch CPU ops
(DESIGN.md §3 "Pyramid box-head training"): matching, labels, sample counts and the encode against
torchvision's ``box_iou`` / ``Matcher`` / ``add_gt_proposals`` / ``assign_targets_to_proposals`` /
``BalancedPositiveNegativeSampler`` (its counts) / ``encode_boxes`` re-typed here, the losses and their
gradients against ``torch.nn.functional`` and autograd in fp64, every case's own property, the plan the
library states for every case's shape and the exported symbols.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import box_head_cases as bc
import box_head_ref as ref
from rpn_targets_ref import present_rows


def tv_box_iou(boxes1, boxes2):
    """torchvision.ops.boxes.box_iou."""
    area1 = (boxes1[:, 2] - boxes1[:, 0]) * (boxes1[:, 3] - boxes1[:, 1])
    area2 = (boxes2[:, 2] - boxes2[:, 0]) * (boxes2[:, 3] - boxes2[:, 1])
    lt = torch.max(boxes1[:, None, :2], boxes2[:, :2])
    rb = torch.min(boxes1[:, None, 2:], boxes2[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (area1[:, None] + area2 - inter)


def tv_matcher(mqm, high, low):
    """torchvision.models.detection._utils.Matcher.__call__, allow_low_quality_matches=False."""
    matched_vals, matches = mqm.max(dim=0)
    below = matched_vals < low
    between = (matched_vals >= low) & (matched_vals < high)
    matches[below] = -1
    matches[between] = -2
    return matches


def tv_add_gt_proposals(proposals, gt_boxes):
    """RoIHeads.add_gt_proposals, one image."""
    return torch.cat((proposals, gt_boxes))


def tv_assign_targets_to_proposals(proposals, gt_boxes, gt_labels, high, low):
    """RoIHeads.assign_targets_to_proposals, one image -> (matcher result, clamped index, labels)."""
    if gt_boxes.numel() == 0:
        z = torch.zeros(proposals.shape[0], dtype=torch.int64)
        return z - 1, z, z.clone()
    matched = tv_matcher(tv_box_iou(gt_boxes, proposals), high, low)
    clamped = matched.clamp(min=0)
    labels = gt_labels[clamped].to(torch.int64)
    labels[matched == -1] = 0
    labels[matched == -2] = -1
    return matched, clamped, labels


def tv_sampler_counts(labels, batch_size_per_image, positive_fraction):
    """The counts of BalancedPositiveNegativeSampler.__call__, one image."""
    positive = torch.where(labels >= 1)[0]
    negative = torch.where(labels == 0)[0]
    num_pos = min(positive.numel(), int(batch_size_per_image * positive_fraction))
    num_neg = min(negative.numel(), batch_size_per_image - num_pos)
    return num_pos, num_neg


def tv_encode_boxes(reference_boxes, proposals, weights):
    """torchvision.models.detection._utils.encode_boxes."""
    wx, wy, ww, wh = weights
    px1, py1, px2, py2 = (proposals[:, i].unsqueeze(1) for i in range(4))
    rx1, ry1, rx2, ry2 = (reference_boxes[:, i].unsqueeze(1) for i in range(4))
    ex_widths, ex_heights = px2 - px1, py2 - py1
    ex_ctr_x, ex_ctr_y = px1 + 0.5 * ex_widths, py1 + 0.5 * ex_heights
    gt_widths, gt_heights = rx2 - rx1, ry2 - ry1
    gt_ctr_x, gt_ctr_y = rx1 + 0.5 * gt_widths, ry1 + 0.5 * gt_heights
    dx = wx * (gt_ctr_x - ex_ctr_x) / ex_widths
    dy = wy * (gt_ctr_y - ex_ctr_y) / ex_heights
    dw = ww * torch.log(gt_widths / ex_widths)
    dh = wh * torch.log(gt_heights / ex_heights)
    return torch.cat((dx, dy, dw, dh), dim=1)


TV_CASES = [c for c in bc.CASES if c.tv]


@pytest.mark.parametrize("case", TV_CASES, ids=repr)
def test_targets_equal_torchvision_retyped(case):
    out = case.reference()
    kw = case.kw
    for n in range(min(case.N, 4)):
        gt = case.gt_boxes[n]
        rows = np.nonzero(present_rows(gt, case.gt_count[n]))[0]   # torchvision refuses degenerate boxes: drop them first
        pc = min(max(int(case.prop_count[n]), 0), case.R)
        props = torch.from_numpy(case.proposals[n, :pc])
        gtb, gtl = torch.from_numpy(gt[rows]), torch.from_numpy(case.gt_labels[n][rows])
        idx = np.arange(pc)
        if kw["add_gt"]:
            props = tv_add_gt_proposals(props, gtb)
            idx = np.concatenate([idx, case.R + rows])             # ascending: add_gt_proposals' row order
        assert np.array_equal(idx, np.nonzero(out[bc.MATCHES][n] != -3)[0]), (case.name, n)
        if idx.size == 0:
            assert out[bc.NPOS][n] == 0 and out[bc.NNEG][n] == 0
            continue
        matched, clamped, labels = tv_assign_targets_to_proposals(props, gtb, gtl, kw["fg_iou_thresh"], kw["bg_iou_thresh"])
        want = np.where(matched.numpy() >= 0, rows[clamped.numpy()] if rows.size else 0, matched.numpy())
        assert np.array_equal(out[bc.MATCHES][n][idx], want), (case.name, n)
        assert np.array_equal(ref.labels_of(out[bc.MATCHES][n], case.gt_labels[n])[idx], labels.numpy()), (case.name, n)
        assert (out[bc.NPOS][n], out[bc.NNEG][n]) == tv_sampler_counts(labels, case.B, kw["positive_fraction"])
        # the sampled slots: torchvision's rows of where(pos | neg), labels, clamped indices, and the encode
        S = int(out[bc.NPOS][n] + out[bc.NNEG][n])
        at = np.searchsorted(idx, out[bc.SAMPLES][n, :S])
        assert np.array_equal(idx[at], out[bc.SAMPLES][n, :S])
        assert np.array_equal(out[bc.ROIS][n * case.B:n * case.B + S, 1:], props[at].numpy())
        assert np.array_equal(out[bc.LABELS][n, :S], labels.numpy()[at])
        pos = out[bc.LABELS][n, :S] >= 1
        assert np.array_equal(out[bc.MATCHED][n, :S][pos], rows[clamped.numpy()[at][pos]])
        if pos.any():
            enc = tv_encode_boxes(gtb[clamped[at][pos]], props[at][pos], kw["reg_weights"]).numpy()
            got = out[bc.REG][n, :S][pos]
            assert np.array_equal(got[:, :2], enc[:, :2])          # IEEE operations in torchvision's order
            np.testing.assert_allclose(got[:, 2:], enc[:, 2:], rtol=2.0 ** -22, atol=2.0 ** -24)   # torch.log: within an ulp


@pytest.mark.parametrize("case", bc.CASES, ids=repr)
def test_case_property_and_consistency(case):
    out = case.reference()
    if case.check is not None:
        case.check(case, out)
    for n in range(min(case.N, 8)):
        p, q = int(out[bc.NPOS][n]), int(out[bc.NNEG][n])
        S, s, lab = p + q, out[bc.SAMPLES][n, :p + q], out[bc.LABELS][n, :p + q]
        assert S <= case.B and (np.diff(s) > 0).all() and (lab >= 0).all()
        assert (lab >= 1).sum() == p and (lab == 0).sum() == q
        assert (out[bc.MATCHES][n][s][lab >= 1] == out[bc.MATCHED][n, :S][lab >= 1]).all()
        assert (out[bc.MATCHED][n, :S][lab == 0] == 0).all()
        assert (out[bc.SAMPLES][n, S:] == -1).all() and (out[bc.LABELS][n, S:] == -1).all()
        assert not out[bc.REG][n, :S][lab == 0].any() and not out[bc.REG][n, S:].any()
        assert np.isfinite(out[bc.REG][n]).all()
        assert (out[bc.ROIS][n * case.B:n * case.B + S, 0] == n).all() and (out[bc.ROIS][n * case.B + S:(n + 1) * case.B, 0] == -1).all()


def test_every_issue_case_is_present():
    names = ("layout gt_tie threshold_edges threshold_edges_band gt_is_candidate no_add_gt no_gt_image all_padding_gt "
             "invalid_gt_rows gt_count_clamped prop_count_zero prop_count_clamped rows_past_count_ignored "
             "nonfinite_proposal zero_area_proposal gt_label_zero gt_label_negative few_positives few_candidates "
             "fraction_0 fraction_1 weights_nondefault key_ties_0 key_ties_4 big_state no_candidates batch_1 batch_1024 "
             "G256 M_64 M_65 M_256 M_257 M_1024 M_1025 max_shape").split()
    assert set(names) == set(bc.BY_NAME)
    big = bc.BY_NAME["max_shape"]
    assert (big.R, big.G, big.B) == (4096, 256, 1024) and bc.BY_NAME["batch_1024"].N == 1024 and bc.BY_NAME["G256"].G == 256
    assert {c.C for c in bc.LOSS_CASES} >= {2, 21, 64, 65, 91, 128}
    assert min(c.N * c.B for c in bc.LOSS_CASES) == 16


def test_selection_passes_are_counted_as_the_kernel_walks_them():
    comp = (np.arange(40, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(19)   # 45-bit, distinct
    assert bc.passes(comp, 0) == 0 and bc.passes(comp, 40) == 0 and 1 <= bc.passes(comp, 7) <= 4
    tied = np.arange(5000, dtype=np.uint64)            # all keys 0: only the index digits differ
    assert bc.passes(tied[:4000], 5) == 4 and bc.passes(tied[:4097], 4096) == 3


@pytest.mark.parametrize("case", bc.CASES, ids=repr)
def test_name_query_states_the_plan(case):
    """Host only: every case's plan is what the library says for its shape."""
    from replication_faster_rcnn_amd import ops
    name = ops.box_head_targets_kernel(case.R, case.G, case.N, case.B, case.key_bits)
    for part in case.plan:
        assert part in name, (part, name)


def test_capi_symbols_are_exported_and_refuse_without_a_gpu():
    from replication_faster_rcnn_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("frcnn_box_head_targets", "frcnn_box_head_targets_workspace_size", "frcnn_box_head_targets_kernel",
              "frcnn_box_head_losses_fwd_t", "frcnn_box_head_losses_bwd_t", "frcnn_box_head_losses_workspace_size"):
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
    lib = _lib.load(require_gpu=False)
    assert lib.frcnn_box_head_targets_workspace_size(1, 4097, 4, 512) == 0 and b"R" in lib.frcnn_last_error()
    assert lib.frcnn_box_head_targets_workspace_size(1, 1000, 257, 512) == 0 and b"G" in lib.frcnn_last_error()
    assert lib.frcnn_box_head_targets_workspace_size(1025, 1000, 4, 512) == 0
    assert lib.frcnn_box_head_targets_workspace_size(1, 1000, 4, 1025) == 0
    assert b"batch_size_per_image" in lib.frcnn_last_error()
    assert lib.frcnn_box_head_targets_workspace_size(8, 1000, 32, 512) >= 8 * 1032 * 5
    assert lib.frcnn_box_head_losses_workspace_size(8, 512) > 0 and lib.frcnn_box_head_losses_workspace_size(0, 512) == 0
    buf = ctypes.create_string_buffer(64)
    assert lib.frcnn_box_head_targets_kernel(1, 8, 4, 16, 40, buf, 64) == -1 and b"key_bits" in lib.frcnn_last_error()
    # shape and parameter errors come before any HIP call
    assert lib.frcnn_box_head_losses_fwd_t(0, None, None, 1, 16, 1, None, None, None, None, 0.1, None, None, None, 0,
                                           None) == -1 and b"C must be" in lib.frcnn_last_error()
    assert lib.frcnn_box_head_losses_bwd_t(7, None, None, 1, 16, 4, None, None, None, None, 0.1, None, None, None, None,
                                           None, None) == -1 and b"dtype" in lib.frcnn_last_error()


@pytest.mark.parametrize("case", bc.LOSS_CASES, ids=repr)
def test_losses_equal_torch_fp64(case):
    cls, reg = case.predictions()
    labels, reg_t, n_pos, n_neg = case.targets_np()
    g_cls = None if case.unused == "cls" else 0.75
    g_box = None if case.unused == "box" else 1.5
    lc, lb, dcls, dreg, stats = ref.losses(cls.numpy(), reg.numpy(), labels, reg_t, n_pos, n_neg, g_cls=g_cls, g_box=g_box)
    lab = torch.from_numpy(ref.slot_labels(labels, n_pos, n_neg, case.C).reshape(-1).astype(np.int64))
    ok, pos = lab >= 0, lab >= 1
    S = int(ok.sum())
    assert stats == (S, int(pos.sum()), case.bad, 0)
    if S == 0:
        assert np.isnan(lc) and np.isnan(lb) and not dcls.any() and not dreg.any()
        return
    x64, d64 = cls.double().requires_grad_(True), reg.double().requires_grad_(True)
    want_c = F.cross_entropy(x64[ok], lab[ok])
    sel = d64.view(-1, case.C, 4)[pos, lab[pos]]
    beta = float(np.float32(1 / 9))
    want_b = F.smooth_l1_loss(sel, torch.from_numpy(reg_t).double().view(-1, 4)[pos], beta=beta, reduction="sum") / S
    ((0.0 if g_cls is None else g_cls) * want_c + (0.0 if g_box is None else g_box) * want_b).backward()
    np.testing.assert_allclose(lc, want_c.item(), rtol=1e-12)
    np.testing.assert_allclose(lb, want_b.item(), rtol=1e-12)
    for got, t in ((dcls, x64), (dreg, d64)):
        want = t.grad.numpy() if t.grad is not None else np.zeros(t.shape)
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-15)
        assert np.array_equal(got != 0, want != 0)
    if case.unused == "cls":
        assert not dcls.any() and dreg.any()
    if case.unused == "box":
        assert dcls.any() and not dreg.any()
    # padding rows and the columns of other classes get nothing
    assert not dcls[~ok.numpy()].any() and not dreg[~pos.numpy()].any()
    assert (np.count_nonzero(dreg, axis=1) <= 4).all()
