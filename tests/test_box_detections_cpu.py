"""The pyramid box-head inference contract without a GPU (DESIGN.md §3 "Pyramid box-head
inference"): every named case's precondition and closed form against the numpy restatement, the
restatement against torchvision's ``postprocess_detections`` re-typed in torch CPU ops, planted
mistakes, and the C-ABI's argument validation."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_detections_cases as bc  # noqa: E402
import box_detections_ref as ref_mod  # noqa: E402

F32 = np.float32


@pytest.mark.parametrize("case", bc.CASES, ids=repr)
def test_case_precondition_and_closed_form(case):
    ref = case.reference()
    assert [a.shape for a in ref] == [(case.N, case.D, 4), (case.N, case.D), (case.N, case.D), (case.N, case.D),
                                      (case.N,), (case.N,)]
    assert case.check is not None, "a case states what it reaches"
    case.check(case, ref)
    for n in range(case.N):         # padding and the cut
        k = int(ref[4][n])
        assert k == min(int(ref[5][n]), case.D)
        assert not ref[0][n, k:].any() and (ref[1][n, k:] == -1).all() and not ref[2][n, k:].any()
        assert (ref[3][n, k:] == -1).all() and np.isfinite(ref[0][n, :k]).all()
        assert (ref[3][n, :k] < case.valid_rows(n)).all() and (ref[1][n, :k] >= 1).all()


def test_the_table_covers_what_the_contract_lists():
    names = set(bc.BY_NAME)
    groups = {c.group for c in bc.CASES}
    assert groups == {"layout", "prop_count", "cand", "thresh", "decode", "nms", "merge", "original"}
    for k in (0, 1, 63, 64, 65, 1023, 1024):
        assert f"cand_{k}_R1024" in names
    assert {"cand_1_R1", "cand_1025_R1025", "cand_4096_R4096"} <= names
    assert bc.BY_NAME["cand_1024_R1024"].plan == bc.ROWS and bc.BY_NAME["cand_1025_R1025"].plan == bc.STRIDED
    assert max(c.R * c.C for c in bc.CASES) == 70 * 128 and max(c.R for c in bc.CASES) == 4096
    assert set(bc.MISTAKE_CASE) == set(ref_mod.MISTAKES) and set(bc.MISTAKE_CASE.values()) <= names
    assert len(bc.HALF) >= 20


@pytest.mark.parametrize("case", bc.HALF, ids=repr)
def test_half_cases_are_representable(case):
    assert bc.representable(case)


@pytest.mark.parametrize("mistake", ref_mod.MISTAKES)
def test_planted_mistake_changes_its_case(mistake):
    case = bc.BY_NAME[bc.MISTAKE_CASE[mistake]]
    good, bad = case.reference(), case.reference(mistake)
    assert any(not np.array_equal(bc.bits(g), bc.bits(b)) for g, b in zip(good, bad)), (mistake, case.name)


def test_greedy_nms_is_the_oracles():
    """The restatement's sweep against the oracle's C restatement of torchvision's nms."""
    from oracle import ref_numpy as orc
    rng = np.random.default_rng(5)
    for k in (1, 2, 65, 300):
        xy = rng.integers(0, 200, (k, 2))
        b = np.concatenate([xy, xy + rng.integers(1, 120, (k, 2))], 1).astype(F32)
        s = np.sort(rng.random(k).astype(F32))[::-1].copy()
        for thr in (0.3, 0.5, 0.7):
            assert np.array_equal(ref_mod.greedy_nms(b, thr), orc.nms(b, s, thr))


# ------------------------------------------- torchvision's postprocess_detections, re-typed
def tv_decode_single(rel_codes, boxes, weights):
    """torchvision.models.detection._utils.BoxCoder.decode_single."""
    boxes = boxes.to(rel_codes.dtype)
    widths = boxes[:, 2] - boxes[:, 0]
    heights = boxes[:, 3] - boxes[:, 1]
    ctr_x = boxes[:, 0] + 0.5 * widths
    ctr_y = boxes[:, 1] + 0.5 * heights
    wx, wy, ww, wh = weights
    dx = rel_codes[:, 0::4] / wx
    dy = rel_codes[:, 1::4] / wy
    dw = rel_codes[:, 2::4] / ww
    dh = rel_codes[:, 3::4] / wh
    clip = float(np.log(1000.0 / 16))
    dw = torch.clamp(dw, max=clip)
    dh = torch.clamp(dh, max=clip)
    pred_ctr_x = dx * widths[:, None] + ctr_x[:, None]
    pred_ctr_y = dy * heights[:, None] + ctr_y[:, None]
    pred_w = torch.exp(dw) * widths[:, None]
    pred_h = torch.exp(dh) * heights[:, None]
    c_to_c_h = torch.tensor(0.5, dtype=pred_ctr_y.dtype) * pred_h
    c_to_c_w = torch.tensor(0.5, dtype=pred_ctr_x.dtype) * pred_w
    x1, y1 = pred_ctr_x - c_to_c_w, pred_ctr_y - c_to_c_h
    x2, y2 = pred_ctr_x + c_to_c_w, pred_ctr_y + c_to_c_h
    return torch.stack((x1, y1, x2, y2), dim=2).flatten(1)


def tv_clip_boxes_to_image(boxes, size):
    boxes_x = boxes[..., 0::2].clamp(min=0, max=size[1])
    boxes_y = boxes[..., 1::2].clamp(min=0, max=size[0])
    return torch.stack((boxes_x, boxes_y), dim=boxes.dim()).reshape(boxes.shape)


def tv_remove_small_boxes(boxes, min_size):
    ws, hs = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    return torch.where((ws >= min_size) & (hs >= min_size))[0]


def tv_nms(boxes, scores, thr):
    """torchvision's CPU nms kernel, in torch ops."""
    order = scores.sort(stable=True, descending=True)[1]
    areas = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    dead = torch.zeros(len(boxes), dtype=torch.bool)
    keep = []
    for _i in range(len(order)):
        i = order[_i]
        if dead[i]:
            continue
        keep.append(int(i))
        for _j in range(_i + 1, len(order)):
            j = order[_j]
            if dead[j]:
                continue
            w = torch.clamp(torch.minimum(boxes[i, 2], boxes[j, 2]) - torch.maximum(boxes[i, 0], boxes[j, 0]), min=0)
            h = torch.clamp(torch.minimum(boxes[i, 3], boxes[j, 3]) - torch.maximum(boxes[i, 1], boxes[j, 1]), min=0)
            inter = w * h
            if float(inter / (areas[i] + areas[j] - inter)) > thr:
                dead[j] = True
    return torch.tensor(keep, dtype=torch.int64)


def tv_batched_nms_vanilla(boxes, scores, idxs, thr):
    keep_mask = torch.zeros_like(scores, dtype=torch.bool)
    for class_id in torch.unique(idxs):
        curr = torch.where(idxs == class_id)[0]
        keep_mask[curr[tv_nms(boxes[curr], scores[curr], thr)]] = True
    keep = torch.where(keep_mask)[0]
    return keep[scores[keep].sort(descending=True)[1]]


def tv_postprocess_detections(class_logits, box_regression, proposals, image_shapes, score_thresh, nms_thresh, D,
                              weights):
    """RoIHeads.postprocess_detections; also returns the proposal row of every detection."""
    C = class_logits.shape[-1]
    per = [len(b) for b in proposals]
    pred_boxes = tv_decode_single(box_regression, torch.cat(proposals), weights).reshape(sum(per), -1, 4)
    pred_scores = torch.softmax(class_logits, -1)
    out = []
    for boxes, scores, shape in zip(pred_boxes.split(per), pred_scores.split(per), image_shapes):
        boxes = tv_clip_boxes_to_image(boxes, shape)
        labels = torch.arange(C).view(1, -1).expand_as(scores)
        rows = torch.arange(len(scores)).view(-1, 1).expand_as(scores)
        boxes, scores, labels, rows = boxes[:, 1:], scores[:, 1:], labels[:, 1:], rows[:, 1:]
        boxes, scores, labels, rows = boxes.reshape(-1, 4), scores.reshape(-1), labels.reshape(-1), rows.reshape(-1)
        inds = torch.where(scores > score_thresh)[0]
        boxes, scores, labels, rows = boxes[inds], scores[inds], labels[inds], rows[inds]
        keep = tv_remove_small_boxes(boxes, 1e-2)
        boxes, scores, labels, rows = boxes[keep], scores[keep], labels[keep], rows[keep]
        keep = tv_batched_nms_vanilla(boxes, scores, labels, nms_thresh)
        total = len(keep)
        keep = keep[:D]
        out.append((boxes[keep].numpy(), labels[keep].numpy(), scores[keep].numpy(), rows[keep].numpy(), total))
    return out


N_, R_, C_, D_ = 2, 20, 4, 12
SCORE_T, NMS_T, MIN_SIZE = 0.05, 0.5, 1e-2
IMG = ((300.0, 400.0), (260.0, 340.0))
WEIGHTS = (10.0, 10.0, 5.0, 5.0)


def margin_inputs(seed):
    """Random inputs on which torch's own softmax and exp cannot change a decision: redrawn from
    the seed's generator until every margin holds (the draw count is part of the seed's input)."""
    rng = np.random.default_rng(seed)
    for draw in range(400):
        logits = rng.normal(0, 2.0, (N_ * R_, C_)).astype(F32)
        reg = rng.normal(0, 1.5, (N_ * R_, 4 * C_)).astype(F32)
        reg[:, 2::4] *= 0.5
        reg[:, 3::4] *= 0.5
        xy = rng.uniform(0, 250, (N_, R_, 2))
        props = np.concatenate([xy, xy + rng.uniform(20, 150, (N_, R_, 2))], -1).astype(F32)
        count = np.array([R_, R_ - 3], np.int32)
        ok = True
        for n in range(N_):
            p = ref_mod.probabilities(logits, count, n, R_).astype(np.float64)[:, 1:].ravel()
            near = p[p > SCORE_T / 2]
            ok &= np.abs(p - SCORE_T).min() > 1e-3 and (np.diff(np.sort(near)) > 1e-5).all()
            pf = ref_mod.probabilities(logits, count, n, R_)
            for c, rows in enumerate(ref_mod.candidates(pf, SCORE_T), 1):
                b, _ = ref_mod.decode(props[n, rows], reg[n * R_ + rows, 4 * c:4 * c + 4], WEIGHTS, *IMG[n], MIN_SIZE)
                sides = np.concatenate([b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]])
                ok &= bool((np.abs(sides - MIN_SIZE) > 1e-3).all())
                iou = ref_mod.iou_matrix(b[(sides[:len(b)] > 1) & (sides[len(b):] > 1)])
                ok &= bool((np.abs(iou[np.isfinite(iou)] - NMS_T) > 1e-3).all())
        if ok:
            return logits, reg, props, count
    raise AssertionError(f"seed {seed}: no draw with margins")


# DESIGN.md §3 "Pyramid box-head inference", "Against torchvision": relative bound on a score,
# and the bound on a coordinate from the predicted width and the coordinate's own size.
SCORE_REL = (2 * (C_ - 1) + 12) * 2.0 ** -24


def box_bound(boxes, props, reg4):
    pw = np.exp(np.minimum(reg4[:, 2:] / np.array(WEIGHTS[2:]), np.log(1000 / 16))) * (props[:, 2:] - props[:, :2])
    side = np.repeat(pw.max(1, keepdims=True), 4, 1)
    return 2.0 ** -22 * (side + np.abs(boxes))


@pytest.mark.parametrize("seed", range(8))
def test_restatement_against_torchvision_retyped(seed):
    logits, reg, props, count = margin_inputs(seed)
    ref = ref_mod.box_detections(logits, reg, props, count, np.array(IMG, F32), score_thresh=SCORE_T, nms_thresh=NMS_T,
                                 detections_per_img=D_, min_size=MIN_SIZE, reg_weights=WEIGHTS)
    # torchvision sees only the valid rows of each image
    rows = np.concatenate([n * R_ + np.arange(count[n]) for n in range(N_)])
    tv = tv_postprocess_detections(torch.from_numpy(logits[rows]), torch.from_numpy(reg[rows]),
                                   [torch.from_numpy(props[n, :count[n]]) for n in range(N_)], IMG, SCORE_T, NMS_T, D_,
                                   WEIGHTS)
    worst_s = worst_b = 0.0
    for n, (b, l, s, r, total) in enumerate(tv):
        k = int(ref[4][n])
        assert total == ref[5][n] and len(l) == k, (seed, n, total, ref[5][n])
        assert np.array_equal(r, ref[3][n, :k]) and np.array_equal(l, ref[1][n, :k]), (seed, n)
        rel = np.abs(s.astype(np.float64) - ref[2][n, :k]) / ref[2][n, :k]
        bound = box_bound(ref[0][n, :k].astype(np.float64), props[n, r].astype(np.float64),
                          np.stack([reg[n * R_ + ri, 4 * li:4 * li + 4] for ri, li in zip(r, l)]).astype(np.float64)
                          if k else np.zeros((0, 4)))
        err = np.abs(b.astype(np.float64) - ref[0][n, :k])
        worst_s = max(worst_s, float(rel.max(initial=0.0)) / SCORE_REL)
        worst_b = max(worst_b, float((err / bound).max(initial=0.0)))
        assert (rel <= SCORE_REL).all() and (err <= bound).all(), (seed, n, rel.max(), err.max())
    assert ref[5].sum() >= 6, "the seed has detections"
    print(f"seed {seed}: kept {ref[5].tolist()}; largest score difference = {worst_s:.3f} of its bound "
          f"({SCORE_REL:.3e} relative), largest box difference = {worst_b:.3f} of its bound")


# ------------------------------------------------------------------- the C-ABI, host side
def _lib():
    from replication_faster_rcnn_amd import _lib as L
    return L, L.load(require_gpu=False)


def test_kernel_names_and_branches():
    from replication_faster_rcnn_amd import ops
    for R, dt, key in ((1, torch.float32, "f32"), (1024, torch.float16, "f16"), (1025, torch.bfloat16, "bf16"),
                       (4096, torch.float32, "f32")):
        assert ops.box_head_detections_kernel(R, 2, 100, dt) == bc.plan_name(R, key)
    for bad, word in (((0, 2, 100), "R"), ((4097, 2, 100), "R"), ((8, 1, 100), "C"), ((8, 129, 100), "C"),
                      ((8, 2, 0), "detections_per_img"), ((8, 2, 1025), "detections_per_img")):
        with pytest.raises(RuntimeError, match=word):
            ops.box_head_detections_kernel(*bad)
    with pytest.raises(RuntimeError):
        ops.box_head_detections_kernel(8, 2, 100, torch.float64)


def test_capi_validates_before_any_launch():
    """Every limit is refused with FRCNN_EINVAL and a message naming it; no HIP call is made, so
    the fake non-null pointers are never followed."""
    L, lib = _lib()
    fake = 4096         # non-null, 256-byte aligned, never dereferenced
    buf = ctypes.create_string_buffer(256)

    def call(dtype=0, N=1, R=8, C=3, D=10, w=(10.0, 10.0, 5.0, 5.0), ins=(fake,) * 5, outs=(fake,) * 6, ws=fake,
             ws_bytes=1 << 30):
        return lib.frcnn_box_detections_t(dtype, N, R, C, *ins, None, 0.05, 0.5, D, 0.01, *w, *outs, ws, ws_bytes, None)

    for kw, word in ((dict(dtype=3), b"dtype"), (dict(N=0), b"N must"), (dict(N=1025), b"N must"), (dict(R=0), b"R must"),
                     (dict(R=4097), b"R must"), (dict(C=1), b"C must"), (dict(C=129), b"C must"),
                     (dict(D=0), b"detections_per_img"), (dict(D=1025), b"detections_per_img"),
                     (dict(w=(0.0, 10.0, 5.0, 5.0)), b"reg_weights"), (dict(w=(10.0, -1.0, 5.0, 5.0)), b"reg_weights"),
                     (dict(w=(10.0, 10.0, float("inf"), 5.0)), b"reg_weights"),
                     (dict(w=(10.0, 10.0, 5.0, float("nan"))), b"reg_weights"),
                     (dict(ins=(None, fake, fake, fake, fake)), b"null input"),
                     (dict(ins=(fake, fake, fake, fake, None)), b"null input"),
                     (dict(outs=(fake,) * 5 + (None,)), b"null output"), (dict(outs=(8,) + (fake,) * 5), b"16-byte"),
                     (dict(dtype=1, ins=(fake + 1, fake, fake, fake, fake)), b"aligned"),
                     (dict(ws=fake + 64), b"256-byte")):
        assert call(**kw) == -1 and word in lib.frcnn_last_error(), (kw, lib.frcnn_last_error())
    need = lib.frcnn_box_detections_workspace_size(1, 8, 3)
    assert call(ws_bytes=need - 1) == -3 and b"workspace" in lib.frcnn_last_error()
    assert call(ws=None) == -3
    for bad in ((0, 8, 3), (1025, 8, 3), (1, 0, 3), (1, 4097, 3), (1, 8, 1), (1, 8, 129)):
        assert lib.frcnn_box_detections_workspace_size(*bad) == 0
    assert lib.frcnn_box_detections_kernel(0, 8, 3, 10, None, 0) == -1
    assert lib.frcnn_box_detections_kernel(7, 8, 3, 10, buf, 256) == -1


def test_workspace_is_probabilities_plus_kept_rows():
    """DESIGN.md's formula: 4 N R C + 2 N R (C-1) + 4 N (C-1) bytes, each part rounded up to 256."""
    _, lib = _lib()
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    for N, R, C in ((1, 1, 2), (2, 70, 128), (8, 1000, 91), (8, 4096, 128), (1024, 4096, 2)):
        assert lib.frcnn_box_detections_workspace_size(N, R, C) == \
            up(4 * N * R * C) + up(2 * N * R * (C - 1)) + up(4 * N * (C - 1))
    assert lib.frcnn_box_detections_workspace_size(8, 4096, 128) < 26 << 20
