"""tests/mask_head_ref.py -- the numpy restatement of the pyramid mask head (DESIGN.md §3
"Pyramid mask head") -- against torchvision's functions re-typed in torch CPU ops (torchvision
itself is absent), and the named cases against the mistakes they must tell apart.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import mask_head_cases as mc
import mask_head_ref as ref

F = np.float32


# ------------------------------------------------------------- inventory
def test_case_inventory():
    assert len(mc.TARGET_CASES) >= 12 and len(mc.LOSS_CASES) >= 5 and len(mc.PASTE_CASES) >= 12
    for c in mc.TARGET_CASES:
        assert c.N <= 3 and c.B <= 16 and c.H <= 40 and c.W <= 50 and c.M in (4, 7, 14, 28), c
    assert sorted(c.M for c in mc.TARGET_CASES if c.M > 7) == [14, 28]
    assert {c.plan for c in mc.TARGET_CASES} == {"one", "strided"}
    for c in mc.PASTE_CASES:
        assert c.N <= 3 and c.D <= 8, c
    assert {c.canvas[1] for c in mc.PASTE_CASES} >= {5, 16, 17, 37} and any(c.canvas[0] == 1 for c in mc.PASTE_CASES)
    assert {c.C for c in mc.LOSS_CASES} >= {2, 128}


# ------------------------------------------------------------ compaction
@pytest.mark.parametrize("case", mc.TARGET_CASES, ids=repr)
def test_compaction_is_torch_where_in_slot_order(case):
    """``proposals[pos]`` / ``matched_idxs[pos]`` with ``pos = torch.where(labels > 0)[0]`` of
    torchvision's RoIHeads.forward, cut to P rows and padded."""
    rois, labels, matched, slot, count, targets = case.reference()
    N, B, M = case.N, case.B, case.M
    P = B if case.P is None else case.P
    bl, bm = torch.from_numpy(case.bt_labels), torch.from_numpy(case.bt_matched)
    br = torch.from_numpy(case.bt_rois).view(N, B, 5)
    rois, targets = rois.reshape(N, P, 5), targets.reshape(N, P, M, M)
    for n in range(N):
        pos = torch.where(bl[n] > 0)[0][:P]
        k = len(pos)
        assert count[n] == k == min(int((bl[n] > 0).sum()), P)
        assert np.array_equal(slot[n, :k], pos.numpy())
        assert np.array_equal(labels[n, :k], bl[n][pos].numpy()) and np.array_equal(matched[n, :k], bm[n][pos].numpy())
        assert np.array_equal(rois[n, :k, 1:], br[n][pos][:, 1:].numpy(), equal_nan=True) and (rois[n, :k, 0] == n).all()
        assert (labels[n, k:] == -1).all() and (matched[n, k:] == -1).all() and (slot[n, k:] == -1).all()
        assert np.array_equal(rois[n, k:], np.tile(np.array([-1, 0, 0, 0, 0], F), (P - k, 1)))
        assert not targets[n, k:].any() and not np.signbit(targets[n, k:]).any()
    assert targets.min() >= 0 and targets.max() <= 255


def test_targets_are_the_mask_values_where_the_answer_is_known():
    """A box inside a constant region pools that constant exactly (weights sum to 1 only up to
    rounding in general; for the constants 0 and 1 with one sample per bin they are exact), a box
    off the mask and an out-of-range gt index give zeros."""
    masks = np.zeros((1, 2, 24, 31), np.uint8)
    masks[0, 0, 4:20, 4:28] = 1
    c = mc.TargetsCase("known", {(0, 0): (1, 0, (6.0, 6.0, 10.0, 10.0)), (0, 1): (1, 1, (6.0, 6.0, 10.0, 10.0)),
                                 (0, 2): (1, 0, (-30.0, -30.0, -10.0, -10.0)), (0, 3): (1, 2, (6.0, 6.0, 10.0, 10.0))},
                       N=1, B=4, G=2, masks=masks)
    t = c.reference()[5]
    assert (t[0] == 1).all() and not t[1:].any()
    byte = mc.TARGETS_BY_NAME["layout_bytes_w37"].reference()[5]
    assert byte.max() > 1          # a byte of 2 or 255 is the value 2 or 255, not "true"


# ----------------------------------------------------------------- losses
def torch_mask_loss(case):
    """maskrcnn_loss: BCE-with-logits of ``mask_logits[arange, labels]`` against the targets, on
    the rows below their image's count whose label indexes a channel; fp64 autograd."""
    x = torch.tensor(case.logits, dtype=torch.float64, requires_grad=True)
    t = torch.tensor(case.targets, dtype=torch.float64)
    N, P = case.N, case.P
    real = [n * P + r for n in range(N) for r in range(min(int(case.count[n]), P))]
    S = len(real)
    rows = [i for i in real if 0 <= case.labels.reshape(-1)[i] < case.C]
    if S == 0:
        loss = x.sum() * 0
    else:
        lab = torch.tensor(case.labels.reshape(-1)[rows], dtype=torch.int64)
        sel = x[torch.tensor(rows, dtype=torch.int64), lab]
        # the mean is over the S real rows; a skipped row adds nothing (torchvision would raise on it)
        loss = TF.binary_cross_entropy_with_logits(sel, t[rows], reduction="sum") / (S * case.M * case.M)
    loss.backward()
    return float(loss.detach()), x.grad.numpy(), S, S - len(rows)


@pytest.mark.parametrize("case", mc.LOSS_CASES, ids=repr)
def test_loss_and_gradient_match_torch_bce(case):
    loss, grad, (S, skipped) = case.reference()
    tl, tg, tS, tskip = torch_mask_loss(case)
    assert (S, skipped) == (tS, tskip)
    assert np.isfinite(loss) and np.isfinite(grad).all()
    assert abs(loss - tl) <= 1e-12 * max(1.0, abs(tl)), (loss, tl)
    assert np.abs(grad - tg).max() <= 1e-15 + 1e-12 * np.abs(tg).max()
    if S == 0:
        assert loss == 0.0 and not grad.any()


@pytest.mark.parametrize("case", mc.LOSS_CASES, ids=repr)
def test_loss_bounds_hold_for_the_fp32_formula(case):
    """The kernels' per-element formulas evaluated in numpy fp32 stay inside ``loss_bounds``."""
    loss, grad, (S, _) = case.reference()
    lb, gb = case.bounds()
    used, _ = ref._rows(case.labels, case.count, case.C)
    total, g32 = 0.0, np.zeros_like(case.logits)
    with np.errstate(all="ignore"):
        for row, _, lab in used:
            x, t = case.logits[row, lab], case.targets[row]
            e = np.exp(-np.abs(x).astype(np.float64)).astype(F)
            lg = np.log1p(e.astype(np.float64)).astype(F)
            l = (np.maximum(x, F(0)) - x * t) + lg
            assert l.dtype == F
            total += float(l.astype(np.float64).sum())
            scale = F(case.g) / F(S * case.M * case.M)
            g32[row, lab] = (ref.sigmoid(x) - t) * scale
    l32 = float(F(total / (S * case.M * case.M))) if S else 0.0
    print(f"{case.name}: |loss - fp64| = {abs(l32 - loss):.3e} (bound {lb:.3e}); "
          f"gradient {np.abs(g32 - grad).max():.3e} (bound {gb.max():.3e})")
    assert abs(l32 - loss) <= lb
    assert (np.abs(g32 - grad) <= gb).all()
    assert not g32[gb == 0].any()


# ------------------------------------------------------------------ paste
def tv_expand_boxes(boxes, scale):
    w_half = (boxes[:, 2] - boxes[:, 0]) * 0.5
    h_half = (boxes[:, 3] - boxes[:, 1]) * 0.5
    x_c = (boxes[:, 2] + boxes[:, 0]) * 0.5
    y_c = (boxes[:, 3] + boxes[:, 1]) * 0.5
    w_half = w_half * scale
    h_half = h_half * scale
    out = torch.zeros_like(boxes)
    out[:, 0], out[:, 2], out[:, 1], out[:, 3] = x_c - w_half, x_c + w_half, y_c - h_half, y_c + h_half
    return out


def tv_paste_mask_in_image(mask, box, im_h, im_w, align_corners=False):
    w = max(int(box[2] - box[0] + 1), 1)
    h = max(int(box[3] - box[1] + 1), 1)
    mask = TF.interpolate(mask[None, None], size=(h, w), mode="bilinear", align_corners=align_corners)[0][0]
    im_mask = torch.zeros((im_h, im_w), dtype=mask.dtype)
    x_0, x_1 = max(int(box[0]), 0), min(int(box[2]) + 1, im_w)
    y_0, y_1 = max(int(box[1]), 0), min(int(box[3]) + 1, im_h)
    if x_0 < x_1 and y_0 < y_1:    # torchvision's boxes are clipped to the image: it never meets the other case
        im_mask[y_0:y_1, x_0:x_1] = mask[(y_0 - int(box[1])):(y_1 - int(box[1])), (x_0 - int(box[0])):(x_1 - int(box[0]))]
    return im_mask


def tv_paste(case):
    """maskrcnn_inference + paste_masks_in_image on the restatement's probabilities, fp32; the
    detections the contract zeroes by rules of its own (count, label, inverted, not finite) are
    zeroed here by the same rules."""
    kw = case.kw
    p = kw.get("padding", 1)
    M, C, (Hc, Wc) = case.M, case.C, case.canvas
    out = torch.zeros((case.N, case.D, Hc, Wc))
    for n in range(case.N):
        im_h, im_w = Hc, Wc
        boxes = torch.from_numpy(case.boxes[n].copy())
        if "original_sizes" in kw:
            oh, ow = kw["original_sizes"][n]
            im_h, im_w = min(int(oh), Hc), min(int(ow), Wc)
            if "image_sizes" in kw:    # resize_boxes
                ih, iw = kw["image_sizes"][n]
                rh, rw = torch.tensor(oh) / torch.tensor(ih), torch.tensor(ow) / torch.tensor(iw)
                boxes = torch.stack([boxes[:, 0] * rw, boxes[:, 1] * rh, boxes[:, 2] * rw, boxes[:, 3] * rh], 1)
        scale = float(M + 2 * p) / M
        ex = tv_expand_boxes(boxes, scale)
        for d in range(min(int(case.count[n]), case.D)):
            lab, b = int(case.labels[n, d]), case.boxes[n, d]
            if not 1 <= lab < C or not np.isfinite(b).all() or np.abs(b).max() > 2 ** 20 or b[2] < b[0] or b[3] < b[1]:
                continue
            prob = torch.from_numpy(ref.sigmoid(case.logits[n * case.D + d, lab]))
            padded = TF.pad(prob, (p,) * 4)
            out[n, d, :im_h, :im_w] = tv_paste_mask_in_image(padded, ex[d].to(torch.int64), im_h, im_w)
    return out.numpy()


def _prob_reference(case):
    kw = dict(case.kw, threshold=None)
    return ref.mask_paste(case.logits, case.boxes, case.labels, case.count, case.canvas, **kw)


WORST = {}


@pytest.mark.parametrize("case", mc.PASTE_CASES, ids=repr)
def test_paste_matches_retyped_torchvision(case):
    """Probabilities within ``interpolate_bound`` (torch's CPU interpolate evaluates the same
    formula in another order); binary masks equal except where the restated probability lies
    within that bound of the threshold."""
    S = case.M + 2 * case.kw.get("padding", 1)
    bound = ref.interpolate_bound(S)
    want, got = _prob_reference(case), tv_paste(case)
    diff = float(np.abs(want - got).max())
    WORST[case.name] = diff
    print(f"{case.name}: S = {S}, largest |restatement - torch| = {diff:.3e} (bound {bound:.3e})")
    assert diff <= bound
    thr = case.kw.get("threshold", 0.5)
    if thr is not None:
        near = np.abs(want - F(thr)) <= bound
        binary = case.reference()
        assert np.array_equal(binary[~near], (got > thr).astype(np.uint8)[~near])


def test_paste_binary_comparison_on_random_logits():
    """The condition of the binary comparison: on random logits at the real mask size the pixels
    whose probability lies within the bound of the threshold are at most 0.1 % of the pixels
    inside the pasted boxes, and every other pixel agrees with the re-typed torchvision path."""
    r = np.random.default_rng(5)
    dets = [[(1, (12.3, 20.1, 150.7, 170.2)), (2, (-10.0, 40.0, 90.5, 130.0)), (1, (100.0, 5.0, 210.0, 66.0)),
             (2, (60.0, 60.0, 75.0, 190.0))]]
    case = mc.PasteCase("random_m28", dets, (200, 200), M=28, seed=5)
    case.logits = (2.0 * r.standard_normal(case.logits.shape)).astype(F)
    bound = ref.interpolate_bound(30)
    want, got = _prob_reference(case), tv_paste(case)
    diff = float(np.abs(want - got).max())
    inside = int((want > 0).sum())
    near = np.abs(want - F(0.5)) <= bound
    flips = int(((want > F(0.5)) != (got > 0.5)).sum())
    print(f"random_m28: largest difference {diff:.3e} (bound {bound:.3e}); {int(near.sum())} of {inside} pixels near "
          f"the threshold; {flips} pixels differ")
    assert diff <= bound
    assert inside > 30000 and near.sum() <= 0.001 * inside
    assert np.array_equal(case.reference()[~near], (got > 0.5).astype(np.uint8)[~near])


def test_sigmoid_against_torch():
    """1 / (1 + exp(-x)) with a correctly rounded exp against torch.sigmoid: torch's vectorised
    exp is within 1 ulp, so both are within 2 ulps of the real value of a number <= 1."""
    x = np.concatenate([np.linspace(-30, 30, 4001), [88, -88, 1e4, -1e4, 0.0]]).astype(F)
    d = np.abs(ref.sigmoid(x).astype(np.float64) - torch.sigmoid(torch.from_numpy(x)).numpy().astype(np.float64))
    assert d.max() <= 4 * ref.U * 2
    assert ref.sigmoid(F(0)) == F(0.5) and ref.sigmoid(F(-1e4)) == 0 and ref.sigmoid(F(1e4)) == 1


def test_detection_rois_on_host_tensors():
    """``ops.detection_rois`` is plain torch: it runs on host tensors too."""
    from replication_faster_rcnn_amd import ops
    case = mc.PASTE_BY_NAME["count_0_and_d"]
    det = ops.BoxDetections(torch.from_numpy(case.boxes), torch.from_numpy(case.labels), None, None,
                            torch.from_numpy(case.count), None)
    got = ops.detection_rois(det)
    want = ref.detection_rois(case.boxes, case.count)
    assert got.dtype == torch.float32 and ref.bits_equal(got.numpy(), want)


def test_kernel_queries_name_the_plans():
    """The host-only queries of the C-ABI name the kernels and the plan branch."""
    from replication_faster_rcnn_amd import _lib, ops
    assert ops.mask_head_targets_kernel(8, None, 4) == "mh_compact_kernel mh_targets_kernel[one]"
    assert ops.mask_head_targets_kernel(512, 128, 28) == "mh_compact_kernel mh_targets_kernel[strided]"
    assert ops.mask_head_targets_kernel(16, 4, 16).endswith("[one]") and ops.mask_head_targets_kernel(16, 4, 17).endswith("[strided]")
    assert ops.mask_head_losses_kernel(21, 28, torch.bfloat16) == (
        "mh_loss_rows_kernel<ElemBF16> mh_loss_final_kernel mh_loss_bwd_kernel<ElemBF16>[vec8]")
    assert ops.mask_head_losses_kernel(2, 4).endswith("mh_loss_bwd_kernel<ElemF32>[vec4]")
    for c in mc.PASTE_CASES:
        assert ops.mask_head_paste_kernel(c.M, c.canvas[1], c.kw.get("padding", 1), c.kw.get("threshold", 0.5)) == c.plan()
    assert ops.mask_head_paste_kernel(28, 600, dtype=torch.float16) == "mh_paste_kernel<ElemF16,u8>[vec16+edges]"
    assert ops.mask_head_paste_kernel(28, 608) == "mh_paste_kernel<ElemF32,u8>[vec16]"
    lib = _lib.load(require_gpu=False)
    for bad in [lambda: ops.mask_head_targets_kernel(1025), lambda: ops.mask_head_targets_kernel(8, 0),
                lambda: ops.mask_head_targets_kernel(8, 8, 57), lambda: ops.mask_head_losses_kernel(1),
                lambda: ops.mask_head_losses_kernel(129), lambda: ops.mask_head_paste_kernel(28, 4097),
                lambda: ops.mask_head_paste_kernel(28, 100, padding=5)]:
        with pytest.raises(RuntimeError):
            bad()
    assert lib.frcnn_mask_losses_workspace_size(0, 4) == 0 and lib.frcnn_mask_losses_workspace_size(2, 3) == 512
    # argument checks come back before any HIP call
    assert lib.frcnn_mask_targets(1, 8, 8, 257, 10, 10, 4, *([None] * 11)) == -1 and b"G must" in lib.frcnn_last_error()
    assert lib.frcnn_mask_paste_t(0, 1, 4, 3, 4, *([None] * 6), 5, 0.5, 1, 10, 10, None, None) == -1
    assert b"padding" in lib.frcnn_last_error()


# -------------------------------------------------------- planted mistakes
def _differs(cases, mistake):
    return [c.name for c in cases if not all(ref.bits_equal(a, b) for a, b in
                                             zip(_as_tuple(c.reference()), _as_tuple(c._reference(mistake))))]


def _as_tuple(v):
    if isinstance(v, np.ndarray):
        return (v,)
    return tuple(np.asarray(a) for a in v[:2]) if isinstance(v[0], float) else tuple(v)


@pytest.mark.parametrize("mistake", ref.PASTE_MISTAKES)
def test_paste_cases_tell_the_mistake(mistake):
    names = _differs(mc.PASTE_CASES, mistake)
    print(mistake, "->", names)
    assert names
    if mistake == "non_strict":
        assert "zero_logits_strict_threshold" in names
    if mistake == "floor":
        assert "negative_coordinates" in names
    if mistake == "no_clip":
        assert "original_sizes_clip" in names


@pytest.mark.parametrize("mistake", ref.TARGET_MISTAKES)
def test_target_cases_tell_the_mistake(mistake):
    names = _differs(mc.TARGET_CASES, mistake)
    print(mistake, "->", names)
    assert names


@pytest.mark.parametrize("mistake", ref.LOSS_MISTAKES)
def test_loss_cases_tell_the_mistake(mistake):
    names = []
    for c in mc.LOSS_CASES:
        loss, grad, _ = c.reference()
        ml, mg, _ = c._reference(mistake)
        lb, gb = c.bounds()
        if abs(ml - loss) > lb or (np.abs(mg - grad) > gb).any():
            names.append(c.name)
    print(mistake, "->", names)
    assert names
