"""Named cases of ``ops.rpn_targets_multilevel`` (DESIGN.md §3 "Pyramid RPN training"): the smallest
shapes at which each thing can go wrong.  Boxes and anchors are integer-valued, so IoUs are exact
quotients of small integers.  Every case carries what the kernel-name query must say for its shape
(``plan``) and, where its name promises a property, a ``check`` that asserts the property on the
restatement's result, so a case cannot silently stop testing what it is named for.  Which branch the
select kernel takes depends on the data (the population of the boundary bucket), so the cases named
for a branch assert that population, against the cap the name query reports (``lds=``)."""
import numpy as np
import torch

import rpn_targets_ref as ref
from replication_faster_rcnn_amd import ops

GRIDS = ((11, 18), (6, 9), (3, 5))
STRIDES = ((8, 10), (16, 20), (32, 40))
SIZES = ((16,), (32,), (64,))
RATIOS = (0.5, 1.0, 2.0)


_anchors = {}   # the anchors of a pyramid, shared by the cases on it (read only)


class Case:
    def __init__(self, name, gt, count, *, grids=GRIDS, strides=STRIDES, sizes=SIZES, ratios=RATIOS, seed=1, calls=0,
                 B=256, frac=0.5, fg=0.7, bg=0.3, lq=True, key_bits=32, check=None):
        self.name = name
        self.gt_boxes = np.ascontiguousarray(gt, dtype=np.float32)
        self.gt_count = np.asarray(count, dtype=np.int32)
        self.N, self.G = self.gt_boxes.shape[:2]
        self.grids, self.strides = tuple(grids), tuple(strides)
        self.bases = ops.pyramid_anchor_bases(sizes, ratios)
        self.K = int(self.bases[0].shape[0])
        self.A = sum(self.K * h * w for h, w in self.grids)
        self.seed, self.calls = seed, calls
        self.kw = dict(batch_size_per_image=B, positive_fraction=frac, fg_iou_thresh=fg, bg_iou_thresh=bg,
                       allow_low_quality_matches=lq)
        self.B, self.key_bits = B, key_bits
        self.plan = _plan(self.A, key_bits)
        self.check = check
        self._ref = {}

    def __repr__(self):
        return self.name

    def reference(self, calls=None):
        calls = self.calls if calls is None else calls
        if calls not in self._ref:
            self._ref[calls] = ref.targets(self.gt_boxes, self.gt_count, self.bases, self.strides, self.grids,
                                           self.seed, calls, key_bits=self.key_bits, anchors=self.anchors(), **self.kw)
        return self._ref[calls]

    def anchors(self):
        key = (tuple(tuple(map(tuple, b.tolist())) for b in self.bases), self.strides, self.grids)
        if key not in _anchors:
            _anchors[key] = ref.all_anchors(self.bases, self.strides, self.grids)
        return _anchors[key]


def random_gts(seed, N, G, h=88, w=180, lo=6, hi=70):
    r = np.random.RandomState(seed)
    x1 = r.randint(0, w - lo, size=(N, G))
    y1 = r.randint(0, h - lo, size=(N, G))
    bw = r.randint(lo, hi, size=(N, G))
    bh = r.randint(lo, hi, size=(N, G))
    return np.stack([x1, y1, np.minimum(x1 + bw, w), np.minimum(y1 + bh, h)], axis=2).astype(np.float32)


LDS_BUCKET = 4096   # the select kernel's kRtCap: boundary-bucket keys it sorts in LDS.  Not a free copy: every
                    # case's plan holds it as lds=, which both test files compare with the kernel-name query.


def _plan(A, key_bits):
    """The parts of frcnn_rpn_targets_multi_kernel's answer for A anchors per image."""
    chunks = (A + 1023) // 1024
    radix = "8" if key_bits <= 8 else "8+12" if key_bits <= 20 else "8+12+12"
    return (f"rpnt_gtmax_kernel[chunks={chunks},tail={A - (chunks - 1) * 1024}]",
            f"rpnt_select_kernel[lds={LDS_BUCKET},radix={radix},steps={(A + 4095) // 4096}]")


def _iou(case, n):
    ok = ref.present_rows(case.gt_boxes[n], case.gt_count[n])
    return ref.iou_matrix(case.gt_boxes[n][ok], case.anchors()), np.nonzero(ok)[0]


# ---- the properties the names promise, asserted on the restatement
def check_layout(case, out):
    off = ref.level_offsets(case.K, case.grids)
    assert off == [0, 594, 756, 801]
    for n in range(case.N):                        # positives in every level: the offsets matter
        pos = np.nonzero(out[0][n] >= 0)[0]
        assert all(((pos >= off[l]) & (pos < off[l + 1])).any() for l in range(3)), pos


def check_gt_tie(case, out):
    m = out[0]
    assert (m[0] == 0).any() and not (m[0] == 1).any() and not (m[0] == 3).any()   # rows 1 and 3 repeat row 0


def check_anchor_tie(case, out):
    iou, _ = _iou(case, 0)
    best = np.nonzero(iou[0] == iou[0].max())[0]
    assert best.size == 2 and iou[0].max() < 0.7
    assert (out[0][0][best] == 0).all() and (out[0][0] >= 0).sum() == 2


def check_restore_other_gt(case, out):
    iou, _ = _iou(case, 0)
    a = int(iou[1].argmax())                                   # the best anchor of gt 1 ...
    assert (iou[1] == iou[1].max()).sum() == 1 and iou[:, a].argmax() == 0   # ... prefers gt 0,
    assert iou[0, a] < iou[0].max() and iou[0, a] < 0.7        # is not gt 0's best and is below fg:
    assert out[0][0][a] == 0 and not (out[0][0] == 1).any()    # restored to gt 0; nobody is matched to gt 1


def check_zero_overlap_gt(case, out):
    iou, _ = _iou(case, 0)
    assert iou[1].max() == 0
    assert (out[0][0] >= 0).all() and (out[0][0][iou[0] == 0] == 0).all()   # every anchor is restored
    assert out[4][0] == 0 and out[3][0] == 128


def check_threshold_edges(case, out):
    iou, _ = _iou(case, 0)
    best = iou.max(axis=0)
    at_fg, at_bg = np.nonzero(best == np.float32(0.5))[0], np.nonzero(best == np.float32(0.25))[0]
    assert at_fg.size and at_bg.size
    assert (out[0][0][at_fg] >= 0).all() and (out[0][0][at_bg] == -2).all()


def check_empty_image(case, out):
    assert (out[0][0] == -1).all() and out[3][0] == 0 and out[4][0] == 256 and (out[0][1] >= 0).any()


def check_all_padding(case, out):
    assert (out[0] == -1).all() and (out[3] == 0).all() and (out[5] == 0).all()


def check_invalid_rows(case, out):
    m = out[0]
    assert set(np.unique(m[0][m[0] >= 0])) == {2, 5}            # the absent rows' indices still count
    assert (m[1] == -1).all()                                   # image 1: no present row at all


def check_count_clamped(case, out):
    assert (out[0][0] == -1).all() and (out[0][1] == case.G - 1).any()


def check_few_positives(case, out):
    assert (0 < out[3]).all() and (out[3] < 128).all() and (out[3] + out[4] == 256).all()


def check_few_negatives(case, out):
    m = out[0]
    assert case.A < case.B
    assert (out[3] == (m >= 0).sum(axis=1)).all() and (out[4] == (m == -1).sum(axis=1)).all() and (out[4] > 0).all()


def check_fraction_0(case, out):
    assert (out[3] == 0).all() and (out[4] == 256).all() and (out[1] != 1).all() and (out[0] >= 0).any()


def check_fraction_1(case, out):
    assert (out[3] == (out[0] >= 0).sum(axis=1)).all() and (out[3] > 0).all() and (out[3] + out[4] == 256).all()


def check_no_low_quality(case, out):
    with_lq = ref.targets(case.gt_boxes, case.gt_count, case.bases, case.strides, case.grids, case.seed, case.calls,
                          key_bits=case.key_bits, **{**case.kw, "allow_low_quality_matches": True})
    assert (with_lq[0] != out[0]).any()


def check_first_by_index(case, out):
    for n in range(case.N):
        pos, neg = np.nonzero(out[0][n] >= 0)[0], np.nonzero(out[0][n] == -1)[0]
        want = np.concatenate([pos[:out[3][n]], neg[:out[4][n]]])
        assert np.array_equal(out[2][n, :want.size], want) and pos.size > out[3][n] > 0 and neg.size > out[4][n] > 0


def check_ties_straddle(case, out):
    mask = np.uint32(ref.key_mask(case.key_bits))
    for n in range(case.N):
        for cls, num in ((out[0][n] >= 0, out[3][n]), (out[0][n] == -1, out[4][n])):
            cand = np.nonzero(cls)[0]
            key = ref.philox_word0(cand, n, case.calls, case.seed) & mask
            chosen = np.isin(cand, out[2][n])
            assert chosen.sum() == num and 0 < num < cand.size
            edge = key[chosen].max()
            assert (key[~chosen] == edge).any()                 # the boundary key is on both sides


def boundaries(case, out):
    """(candidates in the buckets below, population, samples wanted) of the first-digit (top 8 key bits)
    bucket every selection boundary falls into; a class taken whole or not at all has no boundary."""
    mask = np.uint32(ref.key_mask(case.key_bits))
    found = []
    for n in range(case.N):
        for cls, num in ((out[0][n] >= 0, out[3][n]), (out[0][n] == -1, out[4][n])):
            cand = np.nonzero(cls)[0]
            if 0 < num < cand.size:
                digit = np.sort((ref.philox_word0(cand, n, case.calls, case.seed) & mask) >> np.uint32(24))
                d = digit[num - 1]
                found.append((int((digit < d).sum()), int((digit == d).sum()), int(num)))
    return found


def boundary_buckets(case, out):
    return [bucket for _, bucket, _ in boundaries(case, out)]


def check_bucket_in_lds(case, out):
    sizes = boundary_buckets(case, out)
    assert sizes and max(sizes) <= LDS_BUCKET, sizes


def check_bucket_beyond_lds(case, out):
    sizes = boundary_buckets(case, out)
    assert sizes and max(sizes) > LDS_BUCKET, sizes


def check_radix_branch(case, out):
    """A boundary bucket beyond the LDS list whose keys differ below the first digit: the radix passes
    over the key's lower digits run, and the boundary is not settled before them."""
    mask = ref.key_mask(case.key_bits)
    assert case.key_bits > 8
    hit = [(before, bucket, num) for before, bucket, num in boundaries(case, out) if bucket > LDS_BUCKET]
    assert hit and all(0 < num - before < bucket for before, bucket, num in hit), hit
    neg = np.nonzero(out[0][0] == -1)[0]
    low = (ref.philox_word0(neg, 0, case.calls, case.seed) & np.uint32(mask)) & np.uint32(0x00FFFFFF)
    assert np.unique(low).size == min(1 << (case.key_bits - 8), 1 << 24) or np.unique(low).size > 1 << 16


def check_bucket_taken_whole(case, out):
    found = boundaries(case, out)
    assert found and all(before + bucket == num and bucket <= LDS_BUCKET for before, bucket, num in found), found


def check_bucket_at_cap(case, out):
    assert boundary_buckets(case, out) == [LDS_BUCKET] * case.N
    assert all(np.array_equal(out[2][n], np.arange(case.B)) for n in range(case.N))


def check_bucket_past_cap(case, out):
    assert boundary_buckets(case, out) == [LDS_BUCKET + 1] * case.N
    assert all(np.array_equal(out[2][n], np.arange(case.B)) for n in range(case.N))


def check_no_candidates(case, out):
    assert (out[0] == -2).all() and (out[3] == 0).all() and (out[4] == 0).all()


def _first_bucket(A, seed, key_bits):
    """Anchors of image 0 (all negatives) whose masked key lies in the lowest first-digit bucket, at calls 0."""
    key = ref.philox_word0(np.arange(A), 0, 0, seed) & np.uint32(ref.key_mask(key_bits))
    return int((key >> np.uint32(24) == 0).sum())


def _tie_box(i, j):   # a 16 x 16 box centred between level-0 cells (j, i) and (j, i + 1)
    return [10 * i + 5 - 8, 8 * j - 8, 10 * i + 5 + 8, 8 * j + 8]


_far = [5000, 5000, 5010, 5010]
_nan, _inf = float("nan"), float("inf")
_invalid = np.array([[[_nan, 0, 10, 10], [0, 0, _inf, 10], [20, 8, 52, 40], [30, 30, 30, 50], [30, 50, 60, 30],
                      [100, 40, 132, 72], [0, 0, 0, 0], [1, 1, 9, 9]],
                     [[5, 5, 5, 9], [-_inf, 0, 5, 5], [7, 9, 3, 12], [0, 0, _nan, _nan], [9, 9, 9, 9],
                      [1, 2, 3, 2], [0, 0, 0, 0], [0, 0, 0, 0]]], dtype=np.float32)
_layout = np.array([[[20, 8, 37, 24], [40, 16, 73, 48], [60, 10, 125, 74], [100, 2, 120, 40], [130, 50, 170, 80]],
                    [[92, 41, 107, 56], [10, 30, 44, 63], [80, 0, 146, 66], [150, 60, 172, 84], [0, 0, 0, 0]]])
_one = dict(grids=((16, 16),), strides=((8, 8),), sizes=((16,),))

CASES = [
    Case("layout", _layout, [5, 4], check=check_layout),
    Case("gt_tie", np.array([[[20, 8, 52, 40], [20, 8, 52, 40], [90, 30, 120, 70], [20, 8, 52, 40]]] * 2), [4, 4],
         check=check_gt_tie),
    Case("anchor_tie", np.array([[_tie_box(4, 3)]] * 2), [1, 1], check=check_anchor_tie),
    Case("restore_other_gt", np.array([[[67, 25, 92, 49], [77, 30, 85, 39]]] * 2), [2, 2],
         check=check_restore_other_gt),
    Case("zero_overlap_gt", np.array([[[20, 8, 52, 40], _far]] * 2), [2, 2], check=check_zero_overlap_gt),
    Case("threshold_edges", np.array([[[82, 32, 90, 48], [22, 8, 30, 16]]] * 2), [2, 2], fg=0.5, bg=0.25, lq=False,
         check=check_threshold_edges),
    Case("empty_image", random_gts(2, 2, 4, lo=12), [0, 3], check=check_empty_image),
    Case("all_padding", random_gts(3, 2, 4), [0, 0], check=check_all_padding),
    Case("invalid_gt_rows", _invalid, [6, 6], check=check_invalid_rows),
    Case("gt_count_clamped", random_gts(4, 2, 5, lo=16), [-3, 9], check=check_count_clamped),
    Case("G1", random_gts(5, 2, 1, lo=16), [1, 1]),
    Case("G256", random_gts(6, 2, 256), [256, 200]),
    Case("few_positives", random_gts(7, 2, 2, lo=16), [2, 1], check=check_few_positives),
    Case("few_negatives", random_gts(8, 2, 3, h=90, w=190, lo=30, hi=60), [3, 2], grids=((3, 5),), strides=((32, 40),),
         sizes=((64,),), check=check_few_negatives),
    Case("fraction_0", random_gts(9, 2, 4, lo=12), [4, 4], frac=0.0, check=check_fraction_0),
    Case("fraction_1", random_gts(10, 2, 4, lo=12), [4, 4], frac=1.0, check=check_fraction_1),
    Case("no_low_quality", random_gts(11, 2, 4, lo=12), [4, 4], lq=False, check=check_no_low_quality),
    Case("key_ties_0", random_gts(12, 2, 6, lo=12), [6, 6], B=32, fg=0.25, bg=0.1, key_bits=0,
         check=check_first_by_index),
    Case("key_ties_4", random_gts(12, 2, 6, lo=12), [6, 6], B=32, fg=0.25, bg=0.1, key_bits=4, seed=2,
         check=check_ties_straddle),
    Case("big_state", random_gts(14, 2, 4, lo=12), [4, 3], seed=-0x123456789ABCDEF, calls=(7 << 32) + 5),
    Case("no_candidates", random_gts(15, 2, 3), [3, 3], fg=2.0, bg=0.0, lq=False, check=check_no_candidates),
    Case("batch_1", random_gts(16, 2, 3, lo=12), [3, 3], B=1),
    Case("batch_1024", random_gts(17, 2, 3, lo=12), [3, 3], B=1024),
    # one workgroup of the chip-wide kernels holds 1024 anchors in four rows of 256 (64-lane waves); one
    # step of a sweep of the select kernel is four rows of 1024 (bucket_at_cap / bucket_past_cap: 4096, 4097)
    Case("chunk_exact", random_gts(18, 2, 3, h=128, w=128, lo=10, hi=40), [3, 3], ratios=(0.5, 1.0, 2.0, 1.0), **_one),
    Case("chunk_plus_one", random_gts(19, 2, 3, h=40, w=330, lo=10, hi=40), [3, 3], grids=((5, 41),), strides=((8, 8),),
         sizes=((16,),), ratios=(0.5, 1.0, 2.0, 1.0, 0.25)),
    Case("wave_plus_one", random_gts(20, 2, 2, h=16, w=104, lo=6, hi=16), [2, 2], grids=((1, 13),), strides=((8, 8),),
         sizes=((16,),), ratios=(0.5, 1.0, 2.0, 1.0, 0.25), B=16),
    Case("row_plus_one", random_gts(21, 2, 2, h=16, w=2056, lo=6, hi=16), [2, 2], grids=((1, 257),), strides=((8, 8),),
         sizes=((16,),), ratios=(1.0,), B=16),
    Case("wide", random_gts(22, 2, 8, h=600, w=600, lo=20, hi=300), [8, 5], grids=((150, 150),), strides=((4, 4),),
         sizes=((32,),), check=check_bucket_in_lds),
    # the select kernel sorts a boundary bucket of at most 4096 keys in LDS and refines a larger one by sweeps
    Case("wide_ties_0", random_gts(22, 2, 8, h=600, w=600, lo=20, hi=300), [8, 5], grids=((150, 150),), strides=((4, 4),),
         sizes=((32,),), key_bits=0, check=check_bucket_beyond_lds),
    Case("wide_ties_2", random_gts(22, 2, 8, h=600, w=600, lo=20, hi=300), [8, 5], grids=((150, 150),), strides=((4, 4),),
         sizes=((32,),), key_bits=2, seed=3, check=check_bucket_beyond_lds),
    Case("wide_ties_12", random_gts(22, 2, 8, h=600, w=600, lo=20, hi=300), [8, 5], grids=((150, 150),), strides=((4, 4),),
         sizes=((32,),), key_bits=12, check=check_bucket_in_lds),
    Case("bucket_at_cap", np.zeros((2, 1, 4)), [0, 0], grids=((32, 32),), strides=((8, 8),), sizes=((16,),),
         ratios=(0.5, 1.0, 2.0, 1.0), key_bits=0, check=check_bucket_at_cap),
    Case("bucket_past_cap", np.zeros((2, 1, 4)), [0, 0], grids=((1, 241),), strides=((8, 8),), sizes=((16,),),
         ratios=tuple(0.25 + 0.125 * i for i in range(17)), key_bits=0,
         check=check_bucket_past_cap),
    # the boundary bucket is taken whole (nothing to sort, the threshold is the bucket's last possible key): with one
    # key bit there are two buckets, and B is the population of the first
    Case("bucket_taken_whole", np.zeros((1, 1, 4)), [0], key_bits=1, B=_first_bucket(801, 1, 1), check=check_bucket_taken_whole),
    # the radix branch with key digits to refine: 1,228,800 anchors, about 4,800 negatives per first-digit bucket.
    # key_bits 9 / 20 / 21 / 32 are the two sides of each skip (key_bits <= 8 + 12 * pass): at 9 the first 12-bit
    # pass runs on one live bit and the second is skipped, at 20 it runs on twelve, at 21 the second runs on one
    Case("radix_bits_9", random_gts(23, 1, 2, h=2560, w=2560, lo=20, hi=300), [2], grids=((640, 640),),
         strides=((4, 4),), sizes=((32,),), key_bits=9, check=check_radix_branch),
    Case("radix_bits_20", random_gts(23, 1, 2, h=2560, w=2560, lo=20, hi=300), [2], grids=((640, 640),),
         strides=((4, 4),), sizes=((32,),), key_bits=20, check=check_radix_branch),
    Case("radix_bits_21", random_gts(23, 1, 2, h=2560, w=2560, lo=20, hi=300), [2], grids=((640, 640),),
         strides=((4, 4),), sizes=((32,),), key_bits=21, check=check_radix_branch),
    Case("radix_bits_32", random_gts(23, 1, 2, h=2560, w=2560, lo=20, hi=300), [2], grids=((640, 640),),
         strides=((4, 4),), sizes=((32,),), key_bits=32, check=check_radix_branch),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
LOSS_CASES = ("layout", "few_negatives", "fraction_0", "all_padding", "no_candidates", "chunk_plus_one")


def head_outputs(case, dtype=torch.float32, seed=0):
    """Per-level objectness [N, K, H, W] and deltas [N, 4K, H, W] of ``dtype`` (torch CPU tensors);
    deltas near the targets' scale so that both smooth-L1 branches occur."""
    gen = torch.Generator().manual_seed(seed + 100)
    obj = [(torch.randn(case.N, case.K, h, w, generator=gen) * 2).to(dtype) for h, w in case.grids]
    dl = [(torch.randn(case.N, 4 * case.K, h, w, generator=gen) * 0.3).to(dtype) for h, w in case.grids]
    return obj, dl
