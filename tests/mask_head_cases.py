"""Named cases of the pyramid mask head (DESIGN.md §3 "Pyramid mask head"), shared by
test_mask_head_cpu.py and test_gpu_mask_head.py: the smallest shapes at which each edge of the
contract can still go wrong.  Every case computes its reference once (``reference()``)."""
import numpy as np

import mask_head_ref as ref
import roi_align_ref as ra

F = np.float32
NAN, INF = float("nan"), float("inf")


class _Case:
    def __repr__(self):
        return self.name

    def reference(self):
        if getattr(self, "_ref", None) is None:
            self._ref = self._reference()
        return self._ref


# ---------------------------------------------------------------- targets
class TargetsCase(_Case):
    """``slots``: {(image, slot): (label, matched, (x1, y1, x2, y2))}; the other slots of the
    first ``filled`` are negatives (label 0, matched 0, a random box), the rest the sampler's
    padding (rois (-1, 0, 0, 0, 0), labels and matched -1)."""

    def __init__(self, name, slots, N=2, B=8, G=3, H=24, W=31, M=4, P=None, seed=0, filled=None, masks=None):
        self.name, self.N, self.B, self.G, self.H, self.W, self.M, self.P = name, N, B, G, H, W, M, P
        r = np.random.default_rng(seed)
        filled = B if filled is None else filled
        self.bt_rois = np.zeros((N, B, 5), F)
        self.bt_rois[:, :, 0] = -1
        self.bt_labels = np.full((N, B), -1, np.int32)
        self.bt_matched = np.full((N, B), -1, np.int32)
        for n in range(N):
            for s in range(filled):
                xy = r.uniform(0, (max(W - 4, 1), max(H - 4, 1)))
                self.bt_rois[n, s] = [n, xy[0], xy[1], xy[0] + r.uniform(1, 12), xy[1] + r.uniform(1, 12)]
                self.bt_labels[n, s], self.bt_matched[n, s] = 0, 0
        for (n, s), (lab, g, box) in slots.items():
            self.bt_rois[n, s] = [n, *box]
            self.bt_labels[n, s], self.bt_matched[n, s] = lab, g
        self.bt_rois = self.bt_rois.reshape(N * B, 5)
        if masks is None:
            # blobs: a random rectangle of ones per mask over sparse noise, so bins see 0, 1 and mixtures
            masks = (r.random((N, G, H, W)) < 0.15).astype(np.uint8)
            for n in range(N):
                for g in range(G):
                    y, x = r.integers(0, max(H // 2, 1)), r.integers(0, max(W // 2, 1))
                    masks[n, g, y:y + max(H // 2, 1), x:x + max(W // 2, 1)] = 1
        self.gt_masks = np.ascontiguousarray(masks, np.uint8)
        self.plan = "one" if M * M <= 256 else "strided"

    def _reference(self, mistake=None):
        return ref.mask_targets(self.bt_rois, self.bt_labels, self.bt_matched, self.gt_masks, self.M, self.P, mistake)


def _special_slots():
    rois = ra.special_rois(N=1)            # windows with samples exactly on -1, 0, H - 1, H of a 12 x 14 map
    slots = {(0, i): (1 + i % 3, i % 2, tuple(rois[i, 1:])) for i in range(len(rois))}
    slots[(1, 0)] = (1, 0, (NAN, 1, 5, 6))
    slots[(1, 1)] = (2, 1, (1, 1, INF, 6))
    slots[(1, 2)] = (1, 0, (1, -INF, 5, 6))
    slots[(1, 3)] = (1, 1, (2, 2, 9, 2.0 ** 21))   # beyond the coordinate guard
    slots[(1, 4)] = (2, 0, (2, 2, 9, 8))
    return slots


def _layout_masks(N, G, H, W, seed):
    r = np.random.default_rng(seed)
    m = r.integers(0, 2, (N, G, H, W)).astype(np.uint8)
    m[:, 0][m[:, 0] == 1] = 2
    m[:, 1][m[:, 1] == 1] = 255
    return m


TARGET_CASES = [
    TargetsCase("interleaved_m28", {(0, 1): (3, 1, (2.5, 3.25, 30.0, 22.5)), (0, 3): (1, 0, (0.0, 0.0, 31.0, 24.0)),
                                    (0, 4): (2, 2, (10.0, 5.0, 24.5, 19.0)), (0, 7): (1, 1, (4.0, 4.0, 44.0, 41.0)),
                                    (1, 0): (5, 2, (1.0, 2.0, 12.0, 13.0)), (1, 6): (1, 0, (15.0, 3.0, 29.0, 20.0))},
                M=28, seed=1),
    TargetsCase("no_positive_image", {(0, 2): (1, 0, (3.0, 3.0, 20.0, 20.0)), (0, 5): (2, 1, (8.0, 2.0, 25.0, 17.0))}, seed=2),
    TargetsCase("all_positive_p_is_b", {(n, s): (1 + s, (n + s) % 3, (2.0 + s, 1.0 + n, 12.0 + 3 * s, 9.0 + 2 * s))
                                        for n in range(2) for s in range(4)}, B=4, seed=3),
    TargetsCase("clamp_and_drop", {(n, s): (1 + s % 2, s % 3, (1.0 + s, 2.0, 9.0 + 2 * s, 14.0 + s))
                                   for n in range(2) for s in (0, 1, 3, 4, 6, 7)}, P=3, seed=4),
    TargetsCase("matched_limits", {(0, 0): (1, 2, (3.0, 3.0, 20.0, 20.0)), (0, 2): (1, 3, (3.0, 3.0, 20.0, 20.0)),
                                   (0, 5): (2, -1, (3.0, 3.0, 20.0, 20.0)), (1, 1): (1, 2, (0.5, 0.5, 30.5, 23.5)),
                                   (1, 7): (1, 1 << 20, (1.0, 1.0, 9.0, 9.0))}, seed=5),
    TargetsCase("box_inside_m14", {(0, 0): (1, 0, (5.5, 4.25, 25.0, 19.75)), (1, 3): (2, 1, (8.0, 8.0, 15.0, 15.0))},
                M=14, seed=6),
    TargetsCase("box_over_each_edge", {(0, 0): (1, 0, (-6.0, 5.0, 9.0, 15.0)), (0, 1): (1, 1, (22.0, 5.0, 40.0, 15.0)),
                                       (0, 2): (1, 2, (8.0, -7.5, 20.0, 6.0)), (0, 3): (1, 0, (8.0, 15.0, 20.0, 33.0)),
                                       (1, 0): (1, 1, (-3.0, -3.0, 34.0, 27.0))}, M=7, seed=7),
    TargetsCase("box_outside", {(0, 1): (1, 0, (-50.0, 2.0, -20.0, 12.0)), (0, 2): (1, 1, (40.0, 40.0, 60.0, 55.0)),
                                (1, 4): (1, 2, (2.0, -30.0, 12.0, -1.5))}, seed=8),
    TargetsCase("box_narrower_than_1px", {(0, 0): (1, 0, (10.2, 3.0, 10.5, 20.0)), (0, 6): (1, 1, (5.0, 7.7, 25.0, 7.9)),
                                          (1, 2): (1, 2, (12.0, 12.0, 12.0, 12.0))}, M=7, seed=9),
    TargetsCase("box_600px_and_integer_bin", {(0, 0): (1, 0, (-280.0, -290.0, 320.0, 310.0)),
                                              (0, 1): (1, 1, (4.0, 4.0, 12.0, 20.0)),          # bins of exactly 2 x 4
                                              (0, 2): (1, 1, (4.0, 4.0, float(F(12.000001)), 20.0)),
                                              (1, 0): (1, 2, (10.0, 10.0, 78.0, 27.0))},      # 17 px bins: a clipped grid
                H=40, W=50, seed=10),
    TargetsCase("special_windows_and_non_finite", _special_slots(), H=12, W=14, M=7, seed=11),
    TargetsCase("layout_bytes_w37", {(0, 0): (1, 0, (0.0, 0.0, 37.0, 20.0)), (0, 3): (1, 1, (3.3, 1.1, 30.2, 18.9)),
                                     (1, 1): (1, 1, (30.0, 10.0, 40.0, 22.0)), (1, 2): (1, 0, (1.0, 1.0, 2.0, 2.0))},
                G=2, H=20, W=37, seed=12, masks=_layout_masks(2, 2, 20, 37, 12)),
    TargetsCase("layout_w1", {(0, 0): (1, 0, (0.0, 2.0, 1.0, 15.0)), (1, 1): (1, 1, (-2.0, 0.0, 3.0, 30.0))},
                G=2, H=30, W=1, seed=13, masks=_layout_masks(2, 2, 30, 1, 13)),
    TargetsCase("layout_h1", {(0, 0): (1, 0, (2.0, 0.0, 15.0, 1.0)), (1, 1): (1, 1, (0.0, -2.0, 30.0, 3.0))},
                G=2, H=1, W=30, seed=14, masks=_layout_masks(2, 2, 1, 30, 14)),
    TargetsCase("padding_slots_b16", {(0, 0): (1, 0, (3.0, 3.0, 20.0, 20.0)), (0, 9): (2, 1, (8.0, 2.0, 25.0, 17.0)),
                                      (2, 11): (4, 2, (1.0, 1.0, 30.0, 23.0))}, N=3, B=16, P=4, filled=12, seed=15),
]
TARGETS_BY_NAME = {c.name: c for c in TARGET_CASES}


# ----------------------------------------------------------------- losses
class LossCase(_Case):
    def __init__(self, name, labels, count, C=3, M=4, seed=0, fill=None, exact16=True):
        self.name, self.C, self.M, self.exact16 = name, C, M, exact16
        self.labels = np.asarray(labels, np.int32)
        self.count = np.asarray(count, np.int32)
        self.N, self.P = self.labels.shape
        r = np.random.default_rng(seed)
        rows = self.N * self.P
        # multiples of 1/8 in [-8, 8]: exact in float16 and bfloat16
        self.logits = (r.integers(-64, 65, (rows, C, M, M)) / 8.0).astype(F)
        if fill is not None:
            fill(self.logits)
        # soft targets: RoIAlign of 0/1 masks gives values in [0, 1]
        self.targets = r.random((rows, M, M)).astype(F)
        self.targets[r.random((rows, M, M)) < 0.3] = 0
        self.targets[r.random((rows, M, M)) < 0.3] = 1
        self.g = 1.0

    def _reference(self, mistake=None):
        return ref.mask_losses(self.logits, self.targets, self.labels, self.count, self.g, mistake)

    def bounds(self, dtype="f32"):
        return ref.loss_bounds(self.logits, self.targets, self.labels, self.count, self.g, dtype)


def _extreme(x):
    v = np.array([88.0, -88.0, 1e4, -1e4, 0.0, -0.0, 87.5, -103.0, 16.75, -16.75], F)
    x[0, 1].flat[:len(v)] = v
    x[1, 2].flat[:len(v)] = -v


LOSS_CASES = [
    LossCase("s_is_zero", [[1, 2, -1], [-1, -1, -1]], [0, 0], seed=1),
    LossCase("one_positive", [[-1, -1, -1], [2, -1, -1]], [0, 1], seed=2),
    LossCase("extreme_logits", [[1, 2, -1], [1, -1, -1]], [2, 1], seed=3, fill=_extreme, exact16=False),
    LossCase("label_ge_c", [[1, 3, 2], [7, -1, -1]], [3, 1], seed=4),
    LossCase("c2_m7", [[1, 1, 0], [1, -1, -1]], [3, 1], C=2, M=7, seed=5),
    LossCase("c128", [[127, 1], [64, 100]], [2, 2], C=128, seed=6),
    LossCase("m28_unaligned_planes", [[1, 2], [2, -1]], [2, 1], C=3, M=28, seed=7),
    LossCase("m1_vectors_span_rows", [[1, 2, 1, 0, 2], [2, 1, -1, -1, -1]], [5, 2], C=3, M=1, seed=8),
]
LOSSES_BY_NAME = {c.name: c for c in LOSS_CASES}
LOSS_HALF = [c for c in LOSS_CASES if c.exact16]


# ------------------------------------------------------------------ paste
class PasteCase(_Case):
    """``dets``: per image, a list of (label, (x1, y1, x2, y2)); ``count`` defaults to their number."""

    def __init__(self, name, dets, canvas, C=3, M=4, D=None, count=None, seed=0, zero_logits=False, **kw):
        self.name, self.C, self.M, self.canvas, self.kw = name, C, M, tuple(canvas), kw
        self.N = len(dets)
        self.D = D if D is not None else max(max(len(d) for d in dets), 1)
        r = np.random.default_rng(seed)
        self.boxes = np.zeros((self.N, self.D, 4), F)
        self.labels = np.full((self.N, self.D), -1, np.int32)
        for n, ds in enumerate(dets):
            for d, (lab, box) in enumerate(ds):
                self.boxes[n, d], self.labels[n, d] = box, lab
        self.count = np.asarray([len(d) for d in dets] if count is None else count, np.int32)
        # multiples of 1/8 in [-4, 4]: exact in float16 and bfloat16
        self.logits = (r.integers(-32, 33, (self.N * self.D, C, M, M)) / 8.0).astype(F)
        if zero_logits:
            self.logits[:] = 0
        for k in ("image_sizes", "original_sizes"):
            if k in kw:
                kw[k] = np.asarray(kw[k], F)

    def _reference(self, mistake=None):
        return ref.mask_paste(self.logits, self.boxes, self.labels, self.count, self.canvas, mistake=mistake, **self.kw)

    def plan(self, dtype="f32"):
        binary = self.kw.get("threshold", 0.5) is not None
        V = 16 if binary else 4
        return "mh_paste_kernel<%s,%s>[vec%d%s]" % (ra.ELEM[dtype], "u8" if binary else "f32", V,
                                                   "" if self.canvas[1] % V == 0 else "+edges")


def _edges(Hc, Wc):
    return [(1, (-8.0, 6.0, 9.5, 18.0)), (2, (Wc - 9.0, 5.0, Wc + 7.0, 17.0)), (1, (9.0, -7.0, 21.0, 8.5)),
            (2, (9.0, Hc - 8.0, 21.0, Hc + 9.0)), (1, (-4.0, -4.0, Wc + 4.0, Hc + 4.0))]


PASTE_CASES = [
    PasteCase("inside", [[(1, (6.3, 5.2, 30.7, 22.9)), (2, (20.0, 10.0, 41.0, 30.0))], [(2, (3.0, 3.0, 11.0, 9.0))]],
              (36, 48), seed=1),
    PasteCase("over_each_edge", [_edges(36, 48), _edges(36, 48)[::-1]], (36, 48), M=7, seed=2),
    PasteCase("outside", [[(1, (-40.0, 5.0, -12.0, 20.0)), (1, (60.0, 50.0, 80.0, 70.0)), (2, (5.0, -30.0, 20.0, -6.0))],
                          [(1, (5.0, 5.0, 20.0, 20.0))]], (36, 48), seed=3),
    PasteCase("negative_coordinates", [[(1, (-0.9, -0.9, 12.4, 10.4)), (2, (-3.5, -2.5, 9.0, 8.0)),
                                        (1, (-1.6, 4.0, 14.0, 12.0))]], (24, 40), seed=4),
    PasteCase("width_truncates_to_zero", [[(1, (10.2, 5.0, 10.6, 20.0)), (2, (4.0, 7.1, 30.0, 7.3)),
                                           (1, (12.0, 12.0, 12.0, 12.0))]], (24, 40), seed=5),
    PasteCase("inverted_and_nan", [[(1, (20.0, 5.0, 10.0, 20.0)), (1, (5.0, 20.0, 20.0, 10.0)), (2, (NAN, 5.0, 20.0, 20.0)),
                                    (2, (5.0, 5.0, INF, 20.0)), (1, (5.0, 5.0, 2.0 ** 21, 20.0)), (1, (4.0, 4.0, 20.0, 20.0))]],
              (24, 40), seed=6),
    PasteCase("label_0_and_c", [[(0, (4.0, 4.0, 20.0, 20.0)), (3, (4.0, 4.0, 20.0, 20.0)), (-1, (4.0, 4.0, 20.0, 20.0)),
                                 (2, (4.0, 4.0, 20.0, 20.0))]], (24, 40), seed=7),
    PasteCase("count_0_and_d", [[(1, (4.0, 4.0, 20.0, 20.0)), (2, (8.0, 2.0, 30.0, 19.0))],
                                [(1, (4.0, 4.0, 20.0, 20.0)), (2, (8.0, 2.0, 30.0, 19.0))]], (24, 40), count=[0, 2], seed=8),
    PasteCase("count_beyond_d", [[(1, (4.0, 4.0, 20.0, 20.0)), (2, (8.0, 2.0, 30.0, 19.0))]], (24, 40), count=[9], seed=8),
    PasteCase("wc5", [[(1, (-2.0, 1.0, 4.5, 9.0)), (2, (1.0, 2.0, 3.0, 7.0))]], (11, 5), seed=9),
    PasteCase("wc16", [[(1, (-2.0, 1.0, 14.5, 9.0)), (2, (3.0, 2.0, 18.0, 7.0))]], (11, 16), seed=10),
    PasteCase("wc17", [[(1, (-2.0, 1.0, 16.5, 9.0)), (2, (3.0, 2.0, 19.0, 7.0))]], (11, 17), seed=11),
    PasteCase("wc37_m28", [[(1, (1.0, 1.0, 35.5, 38.0)), (2, (13.0, 2.0, 40.0, 27.0)), (1, (15.0, 15.0, 17.0, 33.0))]],
              (40, 37), M=28, seed=12),
    PasteCase("hc1", [[(1, (2.0, -3.0, 30.0, 4.0)), (2, (5.0, 0.0, 12.0, 0.5))]], (1, 33), seed=13),
    PasteCase("padding_0", [[(1, (6.3, 5.2, 30.7, 22.9)), (2, (-3.0, 10.0, 41.0, 30.0))]], (36, 48), seed=14, padding=0),
    PasteCase("padding_2_m14", [[(1, (6.3, 5.2, 30.7, 22.9)), (2, (-3.0, 10.0, 41.0, 30.0))]], (36, 48), M=14, seed=15,
              padding=2),
    PasteCase("zero_logits_strict_threshold", [[(1, (6.0, 5.0, 30.0, 22.0)), (2, (-3.0, 10.0, 41.0, 30.0))]], (36, 48),
              seed=16, zero_logits=True, padding=0),
    PasteCase("probabilities", [[(1, (6.3, 5.2, 30.7, 22.9)), (2, (20.0, 10.0, 41.0, 30.0))], [(2, (3.0, 3.0, 11.0, 9.0))]],
              (36, 45), seed=17, threshold=None),
    PasteCase("original_sizes_clip", [[(1, (6.3, 5.2, 44.7, 33.9)), (2, (20.0, 10.0, 41.0, 30.0))],
                                      [(2, (3.0, 3.0, 40.0, 30.0)), (1, (-2.0, 8.0, 25.0, 34.0))]], (36, 48), seed=18,
              original_sizes=[[30.0, 40.0], [36.0, 22.0]]),
    PasteCase("resize_to_original", [[(1, (3.0, 2.5, 14.0, 11.0)), (2, (8.0, 4.0, 19.5, 12.0))],
                                     [(2, (1.0, 1.0, 12.0, 9.0)), (1, (-1.0, 3.0, 22.0, 14.0))]], (36, 48), seed=19,
              image_sizes=[[16.0, 24.0], [15.0, 20.0]], original_sizes=[[32.0, 44.0], [36.0, 50.0]], threshold=None),
    PasteCase("c128_d8", [[(1 + 18 * i, (2.0 + i, 1.0 + i, 20.0 + 2 * i, 12.0 + i)) for i in range(8)]], (24, 40), C=128,
              seed=20),
]
PASTE_BY_NAME = {c.name: c for c in PASTE_CASES}
PASTE_HALF = [PASTE_BY_NAME[n] for n in ("inside", "over_each_edge", "wc37_m28", "probabilities", "padding_2_m14")]
