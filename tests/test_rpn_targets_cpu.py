"""The restatement tests/rpn_targets_ref.py of the pyramid RPN's training half against torch CPU ops
(DESIGN.md §3 "Pyramid RPN training"): matching against torchvision's ``box_iou`` / ``Matcher`` /
``set_low_quality_matches_`` re-typed here, Philox known answers, the sampler's uniformity, the
losses and their gradients against ``torch.nn.functional`` and autograd in fp64.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rpn_targets_cases as rc
import rpn_targets_ref as ref


def tv_box_iou(boxes1, boxes2):
    """torchvision.ops.boxes.box_iou."""
    area1 = (boxes1[:, 2] - boxes1[:, 0]) * (boxes1[:, 3] - boxes1[:, 1])
    area2 = (boxes2[:, 2] - boxes2[:, 0]) * (boxes2[:, 3] - boxes2[:, 1])
    lt = torch.max(boxes1[:, None, :2], boxes2[:, :2])
    rb = torch.min(boxes1[:, None, 2:], boxes2[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (area1[:, None] + area2 - inter)


def tv_matcher(mqm, high, low, allow_low_quality_matches):
    """torchvision.models.detection._utils.Matcher.__call__ with set_low_quality_matches_."""
    matched_vals, matches = mqm.max(dim=0)
    all_matches = matches.clone() if allow_low_quality_matches else None
    below = matched_vals < low
    between = (matched_vals >= low) & (matched_vals < high)
    matches[below] = -1
    matches[between] = -2
    if allow_low_quality_matches:
        highest, _ = mqm.max(dim=1)
        gt_pred_pairs = torch.where(mqm == highest[:, None])
        pred = gt_pred_pairs[1]
        matches[pred] = all_matches[pred]
    return matches


@pytest.mark.parametrize("case", rc.CASES, ids=repr)
def test_matching_equals_torchvision_retyped(case):
    out = case.reference()
    if case.check is not None:
        case.check(case, out)
    anchors = torch.from_numpy(case.anchors())
    for n in range(case.N):
        gt = case.gt_boxes[n]
        ok = ref.present_rows(gt, case.gt_count[n])       # torchvision refuses degenerate boxes: drop them first
        rows = np.nonzero(ok)[0]
        if rows.size == 0:                                # its all-background branch
            want = np.full(case.A, -1, np.int64)
        else:
            m = tv_matcher(tv_box_iou(torch.from_numpy(gt[rows]), anchors), case.kw["fg_iou_thresh"],
                           case.kw["bg_iou_thresh"], case.kw["allow_low_quality_matches"]).numpy()
            want = np.where(m >= 0, rows[np.maximum(m, 0)], m)
        assert np.array_equal(out[0][n], want), (case.name, n)


@pytest.mark.parametrize("case", rc.CASES, ids=repr)
def test_name_query_states_the_plan(case):
    """Host only.  Every case's plan -- with the LDS cap the cases' bucket checks rely on -- is what the library says."""
    from replication_faster_rcnn_amd import ops
    name = ops.rpn_targets_multilevel_kernel(case.K, case.grids, case.N, case.G, case.B, case.key_bits)
    for part in case.plan:
        assert part in name, (part, name)


def test_outputs_are_consistent():
    for case in rc.CASES:
        matches, sampled, samples, n_pos, n_neg, reg = case.reference()
        for n in range(case.N):
            p, q = n_pos[n], n_neg[n]
            sp, sn = samples[n, :p], samples[n, p:p + q]
            assert (np.diff(sp) > 0).all() and (np.diff(sn) > 0).all() and (samples[n, p + q:] == -1).all()
            assert (matches[n][sp] >= 0).all() and (matches[n][sn] == -1).all()
            assert np.array_equal(np.nonzero(sampled[n] == 1)[0], sp) and np.array_equal(np.nonzero(sampled[n] == 0)[0], sn)
            assert not reg[n, p:].any() and np.isfinite(reg[n, :p]).all()


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        assert ref.philox4x32_10(ctr, key) == want
        got = ref.philox_word0(np.array([ctr[0]]), ctr[1], (ctr[3] << 32) | ctr[2], (key[1] << 32) | key[0])
        assert int(got[0]) == want[0]
    # a negative seed is its two's complement
    assert np.array_equal(ref.philox_word0(np.arange(5), 1, 3, -1), ref.philox_word0(np.arange(5), 1, 3, 2**64 - 1))


def test_sampler_is_uniform():
    # 40 candidates, 10 chosen, seed 1, image 0, calls 0..1999.  The worst deviation depends on which 40 anchor
    # indices are the candidates (they are the Philox counters): these give 1.91 standard deviations, another
    # set gives another figure of that size (1.86 has been quoted for one); the bound is 5.
    cand = np.arange(7, 7 + 3 * 40, 3)
    counts = np.zeros(40)
    for calls in range(2000):
        counts[np.isin(cand, ref.choose(cand, 0, 10, 1, calls, 32))] += 1
    sd = np.sqrt(2000 * 0.25 * 0.75)
    worst = np.abs(counts - 500).max() / sd
    print(f"worst deviation {worst:.2f} standard deviations")
    assert counts.sum() == 20000 and worst < 5


def test_key_bits_0_takes_the_first_by_index():
    cand = np.array([3, 8, 9, 40, 41, 99, 700])
    assert np.array_equal(ref.choose(cand, 1, 4, 5, 17, 0), cand[:4])
    case = rc.BY_NAME["key_ties_0"]
    case.check(case, case.reference())


@pytest.mark.parametrize("name", rc.LOSS_CASES)
def test_losses_equal_torch_fp64(name):
    case = rc.BY_NAME[name]
    tg = case.reference()
    obj, dl = rc.head_outputs(case)
    lo, lb, dobj, ddel, S = ref.losses([t.numpy() for t in obj], [t.numpy() for t in dl], tg, case.K, case.grids,
                                       g_obj=0.75, g_box=1.5)
    o64 = [t.double().requires_grad_(True) for t in obj]
    d64 = [t.double().requires_grad_(True) for t in dl]
    N = case.N
    x = torch.cat([t.permute(0, 2, 3, 1).reshape(N, -1) for t in o64], dim=1)
    d = torch.cat([t.view(N, case.K, 4, *t.shape[2:]).permute(0, 3, 4, 1, 2).reshape(N, -1, 4) for t in d64], dim=1)
    sampled = torch.from_numpy(tg[1])
    assert S == int((sampled >= 0).sum())
    if S == 0:
        assert np.isnan(lo) and np.isnan(lb) and not any(g.any() for g in dobj + ddel)
        return
    labels = (sampled == 1).double()
    tt = torch.zeros_like(d)
    for n in range(N):
        tt[n, torch.from_numpy(tg[2][n, :tg[3][n]]).long()] = torch.from_numpy(tg[5][n, :tg[3][n]]).double()
    keep = sampled >= 0
    want_o = F.binary_cross_entropy_with_logits(x[keep], labels[keep])
    want_b = F.smooth_l1_loss(d[sampled == 1], tt[sampled == 1], beta=1 / 9, reduction="sum") / S
    (0.75 * want_o + 1.5 * want_b).backward()
    np.testing.assert_allclose(lo, want_o.item(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(lb, want_b.item(), rtol=1e-5, atol=1e-7)
    for got, t in zip(dobj + ddel, o64 + d64):
        want = t.grad.numpy() if t.grad is not None else np.zeros(t.shape)
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-7)
        assert np.array_equal(got != 0, want != 0)


def test_unused_loss_gives_zero_gradients():
    case = rc.BY_NAME["layout"]
    obj, dl = rc.head_outputs(case)
    args = ([t.numpy() for t in obj], [t.numpy() for t in dl], case.reference(), case.K, case.grids)
    _, _, dobj, ddel, _ = ref.losses(*args, g_obj=None, g_box=1.0)
    assert not any(g.any() for g in dobj) and any(g.any() for g in ddel)
    _, _, dobj, ddel, _ = ref.losses(*args, g_obj=1.0, g_box=None)
    assert any(g.any() for g in dobj) and not any(g.any() for g in ddel)
