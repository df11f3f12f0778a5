"""Named cases of the FPN proposal layer (DESIGN.md §3 "FPN proposals"): the smallest shapes
at which ``ops.propose_multilevel`` can still go wrong -- layout, levels around ``pre``, ties,
non-finite values, the filters' edges, level-wise NMS, the sweep's block edges, both selection
branches ("sort": a level of at most 2048 anchors, "select": a larger one) and empty results.
torch CPU only, no GPU.

Every case carries ``check(case, ref)``: its own precondition on the fp32 reference, so a
generator change cannot empty it silently (tests/test_fpn_proposals_cpu.py runs them).  The
chain cases use one base box of 64 x 32 on a grid of stride (40, 8) with zero deltas: rows are
disjoint, two boxes of a row overlap above 0.7 exactly when their columns differ by at most 1
(IoU 0.78 one step apart, 0.6 two apart) -- the region / position rule of
tests/propose_plan_cases.py, whose ``closed_form`` gives the keep list without one IoU.

Users: tests/test_fpn_proposals_cpu.py and tests/test_gpu_fpn_proposals.py.
"""
from __future__ import annotations

import numpy as np
import torch

import fpn_proposals_ref as ref
from propose_plan_cases import closed_form
from replication_faster_rcnn_amd import ops

F32 = torch.float32
SORT_CAP = 2048     # csrc/fpn_proposal.hip kFpnSortCap
CHAIN_BASE = torch.tensor([[0.0, 0.0, 64.0, 32.0]])
CHAIN_STRIDE = (40, 8)


class Case:
    def __init__(self, name, objectness, deltas, bases, strides, image_sizes, pre, post, *, nms_thresh=0.7,
                 score_thresh=0.0, min_size=1e-3, check=None):
        self.name, self.objectness, self.deltas, self.bases = name, objectness, deltas, bases
        self.strides = [tuple(s) for s in strides]
        self.N, self.K = objectness[0].shape[:2]
        self.L = len(objectness)
        self.grids = [tuple(o.shape[2:]) for o in objectness]
        sizes = np.asarray(image_sizes, np.float32)
        self.image_sizes = np.broadcast_to(sizes, (self.N, 2)).copy()
        self.pre, self.post, self.nms_thresh, self.score_thresh, self.min_size = pre, post, nms_thresh, score_thresh, min_size
        self.check = check
        self.branches = tuple("sort" if self.K * h * w <= SORT_CAP else "select" for h, w in self.grids)
        self._anchors = None
        self._ref = {}

    def __repr__(self):
        return self.name

    def anchors(self):
        if self._anchors is None:
            self._anchors = ops.pyramid_anchors(self.bases, self.strides, self.grids)
        return self._anchors

    def inputs(self, dtype=F32):
        """(objectness, deltas) as CPU tensors of ``dtype`` (rounded once, as ``.to`` rounds)."""
        return [o.to(dtype) for o in self.objectness], [d.to(dtype) for d in self.deltas]

    def kwargs(self):
        return dict(pre=self.pre, post=self.post, nms_thresh=self.nms_thresh, score_thresh=self.score_thresh,
                    min_size=self.min_size)

    def reference(self, dtype=F32, **over):
        """The reference's six outputs on the inputs widened from ``dtype``; computed once."""
        key = (dtype, tuple(sorted(over.items())))
        if key not in self._ref:
            o, d = self.inputs(dtype)
            kw = self.kwargs()
            level_aware = over.pop("level_aware", True)
            kw.update(over)
            out = ref.reference([t.float() for t in o], [t.float() for t in d], self.anchors(), self.image_sizes,
                                level_aware=level_aware, **kw)
            for a in out:
                a.setflags(write=False)
            self._ref[key] = out
        return self._ref[key]

    def flat(self, l, n=0):
        """(logits [A], deltas [A, 4]) of level l, image n, in anchor order."""
        lo, de = ref.flatten_level(self.objectness[l], self.deltas[l])
        return lo[n], de[n]


def set_anchor(case_obj, case_del, K, a, n, *, logit=None, delta=None):
    """Write the logit / the four deltas of anchor a = (y*W + x)*K + k of image n."""
    W = case_obj.shape[3]
    k, cell = a % K, a // K
    y, x = cell // W, cell % W
    if logit is not None:
        case_obj[n, k, y, x] = logit
    if delta is not None:
        case_del[n, 4 * k:4 * k + 4, y, x] = torch.as_tensor(delta, dtype=F32)


def distinct_logits(gen, shape, lo=-4.0, hi=4.0):
    """Distinct values on a grid of 1/64 (finer for a large level); float16 and bfloat16 round
    some of them together, which their own references then see too."""
    n = int(np.prod(shape))
    den = 64
    while (hi - lo) * den < n:
        den *= 8
    vals = torch.randperm(int((hi - lo) * den), generator=gen)[:n].to(F32) / den + lo
    assert len(vals) == n
    return vals.reshape(shape)


def random_level(gen, N, K, H, W, dscale=0.3):
    return distinct_logits(gen, (N, K, H, W)), torch.randn(N, 4 * K, H, W, generator=gen) * dscale


def chain_level(N, H, W, order_seed=None):
    """A chain grid level: zero deltas; logits decrease along each row, rows interleaved
    (``order_seed`` None), or a seeded shuffle of the same values."""
    A = H * W
    vals = (torch.arange(A, 0, -1).to(F32) / 8)          # distinct, exact in fp32
    if order_seed is not None:
        vals = vals[torch.randperm(A, generator=torch.Generator().manual_seed(order_seed))]
    obj = vals.reshape(1, 1, H, W).repeat(N, 1, 1, 1).contiguous()
    return obj, torch.zeros(N, 4, H, W)


def chain_keep(case, l, n=0):
    """Closed form of a chain level's kept anchors, in sweep order (no ``post`` limit)."""
    H, W = case.grids[l]
    logits, _ = case.flat(l, n)
    order = torch.sort(logits, descending=True, stable=True).indices[:case.pre].numpy()
    a = np.arange(H * W)
    return order[closed_form(a // W, a % W, order)]


def chain_image(grids):
    return (max(40 * h for h, _ in grids), max(8 * w + 64 for _, w in grids))


def _kept_of_level(r, l, n=0):
    c = int(r[4][n])
    return r[3][n, :c][r[2][n, :c] == l]


# ------------------------------------------------------------------------ the cases
def _build():
    cases = []
    add = cases.append
    g = torch.Generator().manual_seed(2024)

    # ---- layout: non-square maps, unequal strides, K = 3, two images
    grids = [(5, 7), (3, 4), (2, 2)]
    bases = ops.pyramid_anchor_bases(((16,), (32,), (64,)), ((0.5, 1.0, 2.0),) * 3)
    bases = [torch.cat([b[:2], b[2:] + 1.0]) for b in bases]      # no symmetry a swap could hide behind
    lv = [random_level(g, 2, 3, h, w) for h, w in grids]

    def check_layout(c, r):
        assert int(r[4].min()) >= 8
        for kind in ("hw", "kc", "yx"):
            t = transposed(c, kind).reference()
            assert not (np.array_equal(t[0], r[0]) and np.array_equal(t[3], r[3])), kind

    add(Case("layout", [o for o, _ in lv], [d for _, d in lv], bases, [(8, 10), (16, 20), (32, 40)], (44, 72), 20, 30,
             check=check_layout))

    # ---- levels around pre = 50: A = 12, 49, 50, 51
    grids = [(3, 4), (7, 7), (5, 10), (3, 17)]
    lv = [random_level(g, 1, 1, h, w, 0.1) for h, w in grids]
    b8 = torch.tensor([[0.0, 0.0, 8.0, 8.0]])

    def check_small(c, r):
        assert [h * w for h, w in c.grids] == [12, 49, 50, 51] and c.pre == 50
        lo, _ = c.flat(3)
        worst = int(torch.argmin(lo))
        assert worst not in _kept_of_level(r, 3)        # the 51st is cut
        assert len(_kept_of_level(r, 0)) == 12 and len(_kept_of_level(r, 2)) == 50

    add(Case("level_smaller_than_pre", [o for o, _ in lv], [d for _, d in lv], [b8] * 4, [(16, 16)] * 4, (400, 400), 50,
             400, check=check_small))

    # ---- ties: all logits equal within and across levels; the index cuts at pre, the level at post
    two = torch.tensor([[0.0, 0.0, 4.0, 4.0], [4.0, 4.0, 8.0, 8.0]])
    grids = [(4, 4), (3, 3)]

    def const_levels(v):
        return ([torch.full((1, 2, h, w), v) for h, w in grids], [torch.zeros(1, 8, h, w) for h, w in grids])

    def check_equal(c, r):
        n0, n1 = len(_kept_of_level(r, 0)), len(_kept_of_level(r, 1))
        assert (n0, n1) == (10, 2), (n0, n1)            # pre = 10 of 32 / 18 by index, post = 12 by level
        assert np.array_equal(_kept_of_level(r, 0), np.arange(10)) and np.array_equal(_kept_of_level(r, 1), [0, 1])

    o, d = const_levels(0.5)
    add(Case("ties_all_equal", o, d, [two, two], [(8, 8), (8, 8)], (64, 64), 10, 12, check=check_equal))
    o, d = const_levels(0.0)
    for t in o:
        t.view(-1)[::2] = -0.0

    def check_zero(c, r):
        bits = c.objectness[0].view(torch.int32)
        assert int((bits == 0).sum()) and int((bits != 0).sum())
        check_equal(c, r)
        own = np.concatenate([c.flat(l)[0].numpy()[_kept_of_level(r, l)] for l in range(2)])
        assert np.array_equal(r[1][0, :12].view(np.uint32), own.view(np.uint32))   # each zero keeps its own sign
        assert len(set(r[1][0, :12].view(np.uint32).tolist())) == 2

    add(Case("ties_signed_zero", o, d, [two, two], [(8, 8), (8, 8)], (64, 64), 10, 12, check=check_zero))

    # quantised logits: the pre-th and (pre+1)-th are equal, the anchor index decides the cut
    o1 = (torch.randint(-8, 9, (2, 2, 6, 6), generator=g).to(F32) / 4)
    o2 = (torch.randint(-8, 9, (2, 2, 4, 5), generator=g).to(F32) / 4)
    d1, d2 = torch.randn(2, 8, 6, 6, generator=g) * 0.2, torch.randn(2, 8, 4, 5, generator=g) * 0.2
    for t in (o1, o2):
        for n in range(2):          # the value at rank pre also at rank pre + 1 (1-based), whatever the draw gave
            v = t[n].view(-1)
            idx = torch.sort(v, descending=True, stable=True).indices
            v[idx[20]] = v[idx[19]]

    def check_cut(c, r):
        for l in range(2):
            lo, _ = c.flat(l)
            s = torch.sort(lo, descending=True, stable=True).values
            assert s[c.pre - 1] == s[c.pre], l

    add(Case("ties_pre_cut", [o1, o2], [d1, d2], [two * 3, two * 5], [(8, 8), (16, 16)], (50, 90), 20, 25,
             check=check_cut))

    # ---- non-finite values
    grids = [(6, 8), (3, 4)]
    lv = [random_level(g, 2, 1, h, w) for h, w in grids]
    o, d = [t for t, _ in lv], [t for _, t in lv]
    nanp, nann = torch.tensor([0x7fc00000, 0xffc00001 - (1 << 32)], dtype=torch.int32).view(F32)
    clip = float(ref.BBOX_XFORM_CLIP)
    below, above = np.nextafter(np.float32(clip), np.float32(0)), np.nextafter(np.float32(clip), np.float32(9))
    for n in range(2):
        for a, v in ((3, nanp), (17, nann), (5, float("inf")), (40, float("-inf")), (41, nanp)):
            set_anchor(o[0], d[0], 1, a, n, logit=v)
        set_anchor(o[0], d[0], 1, 7, n, logit=9.0, delta=[float("nan"), 0, 0, 0])
        set_anchor(o[0], d[0], 1, 8, n, logit=8.5, delta=[0, 0, float("nan"), 0])
        set_anchor(o[0], d[0], 1, 9, n, logit=8.0, delta=[float("inf"), 0, 0, 0])
        set_anchor(o[0], d[0], 1, 10, n, logit=7.5, delta=[0, float("-inf"), 0, 0])
        set_anchor(o[0], d[0], 1, 11, n, logit=7.0, delta=[0, 0, float("inf"), float("-inf")])
        set_anchor(o[0], d[0], 1, 12, n, logit=6.5, delta=[0, 0, float(below), float(below)])
        set_anchor(o[0], d[0], 1, 13, n, logit=6.0, delta=[0, 0, clip, clip])
        set_anchor(o[0], d[0], 1, 14, n, logit=5.5, delta=[0, 0, float(above), 50.0])
        set_anchor(o[0], d[0], 1, 15, n, logit=5.0, delta=[3e38, -3e38, 0, 0])
        set_anchor(o[1], d[1], 1, 2, n, logit=nann)
        set_anchor(o[1], d[1], 1, 3, n, logit=float("inf"), delta=[0, 0, float("-inf"), 0])

    def check_nonfinite(c, r):
        k0 = set(_kept_of_level(r, 0).tolist())
        assert not {3, 17, 41} & k0, "a NaN logit was kept"
        assert not {7, 8, 10, 11} & k0, "a NaN box was kept"      # inf - inf, 0 * inf, NaN deltas
        assert 5 in k0 and r[1][0, 0] == np.inf and r[3][0, 0] == 5
        assert np.isfinite(r[0]).all() and not np.isnan(r[1]).any()
        lo, _ = c.flat(0)
        assert int(torch.isnan(lo).sum()) == 3 and c.pre < 48      # the NaNs used three of pre's slots
        assert 3 not in _kept_of_level(r, 1) and 2 not in _kept_of_level(r, 1)

    add(Case("non_finite", o, d, [torch.tensor([[-12.0, -6.0, 12.0, 6.0]]), torch.tensor([[-20.0, -20.0, 20.0, 20.0]])],
             [(8, 8), (16, 16)], (48, 64), 30, 40, check=check_nonfinite))

    # ---- filters: min_size edge, clipping to zero width, score thresholds at t and its predecessor
    t50, t95 = ops.logit_threshold(0.5), ops.logit_threshold(0.95)
    p50, p95 = (float(np.nextafter(np.float32(t), np.float32(-np.inf))) for t in (t50, t95))

    def filter_inputs():
        gg = torch.Generator().manual_seed(7)
        o = distinct_logits(gg, (2, 1, 4, 6), 3.5, 6.0)
        d = torch.zeros(2, 4, 4, 6)
        for n in range(2):
            set_anchor(o, d, 1, 0, n, delta=[0, 0, -1e-7, 0])         # width just below 8
            for a, v in ((2, t95), (3, p95), (4, t50), (8, p50)):
                set_anchor(o, d, 1, a, n, logit=v)
        return [o], [d]

    def check_filters(c, r):
        k = [set(r[3][n, :int(r[4][n])].tolist()) for n in range(2)]
        box = ref.decode(c.anchors()[0].numpy()[:2], c.flat(0)[1].numpy()[:2])
        w = box[:, 2] - box[:, 0]
        assert w[1] == 8.0 and 8.0 - 4 * np.spacing(np.float32(7.9)) <= w[0] < 8.0 and c.min_size == 8.0
        assert 1 in k[0] and 0 not in k[0]                             # exactly min_size stays, just below goes
        assert not {5, 11, 17, 23} & k[0], "column 5 lies past the image's width"
        assert not {18, 19, 20, 21, 22} & k[0], "row 3 lies past the image's height"
        want = {0.0: {2, 3, 4, 8}, 0.5: {2, 3, 4}, 0.95: {2}}[c.score_thresh]
        assert k[0] & {2, 3, 4, 8} == want, (c.score_thresh, k[0])
        assert 9 in k[0] and k[1] == {1}         # image 1 is 20 x 24: the same predictions, one cell survives

    for st in (0.0, 0.5, 0.95):
        o, d = filter_inputs()
        add(Case(f"filters_s{int(st * 100)}", o, d, [b8], [(16, 16)], [(48, 80), (20, 24)], 24, 24, score_thresh=st,
                 min_size=8.0, check=check_filters))

    # ---- level-aware NMS: identical decoded boxes in two levels are both kept, in one level one is
    o = [distinct_logits(g, (1, 2, 3, 3)), distinct_logits(g, (1, 2, 3, 3))]
    d = [torch.zeros(1, 8, 3, 3), torch.zeros(1, 8, 3, 3)]
    same = torch.tensor([[0.0, 0.0, 16.0, 16.0], [0.0, 0.0, 16.0, 16.0]])

    def check_level_nms(c, r):
        assert int(r[4][0]) == 18                                      # 9 cells, one of each pair, two levels
        assert len(_kept_of_level(r, 0)) == 9 and len(_kept_of_level(r, 1)) == 9
        blind = c.reference(level_aware=False)
        assert int(blind[4][0]) == 9                                   # an NMS that ignores the level keeps one

    add(Case("level_nms", o, d, [same, same], [(32, 32), (32, 32)], (96, 96), 18, 40, check=check_level_nms))

    # ---- sweep edges on chain grids
    def chain_case(name, N, grids, pre, post, seeds, check=None):
        lv = [chain_level(N, h, w, s) for (h, w), s in zip(grids, seeds)]
        return Case(name, [o for o, _ in lv], [d for _, d in lv], [CHAIN_BASE] * len(grids), [CHAIN_STRIDE] * len(grids),
                    chain_image(grids), pre, post, check=check)

    def check_chain(c, r):
        total = 0
        for l in range(c.L):
            want = chain_keep(c, l)[:c.post]
            total += len(want)
            if total <= c.post:                                        # every level's list survives the merge whole
                assert np.array_equal(np.sort(_kept_of_level(r, l)), np.sort(want)), (c.name, l)
        assert int(r[4][0]) == min(total, c.post)

    add(chain_case("sweep_63_64_65", 1, [(1, 63), (1, 64), (1, 65)], 100, 4096, [11, 12, 13], check_chain))
    add(chain_case("sweep_2047_2048", 1, [(1, 2047), (2, 1024)], 2048, 4096, [21, 22], check_chain))

    def check_edge(c, r):
        check_chain(c, r)
        assert np.array_equal(chain_keep(c, 0), np.arange(0, 130, 2))  # the chain runs over the edges at 64 and 128

    add(chain_case("chain_over_block_edge", 1, [(1, 130)], 200, 4096, [None], check_edge))

    def check_last(c, r):
        k = chain_keep(c, 0)
        assert len(k) == c.post == 33 and k[-1] == 64 and c.grids[0] == (1, 65)   # the post-th kept is the last candidate
        check_chain(c, r)

    add(chain_case("post_is_last_candidate", 1, [(1, 65)], 100, 33, [None], check_last))

    def check_post_one(c, r):
        assert int(r[4][0]) == 1 and int(r[4][1]) == 1 and r[2][0, 0] == 0

    add(chain_case("post_one", 2, [(2, 70), (1, 40)], 64, 1, [31, 32], check_post_one))

    def check_padding(c, r):
        n = int(r[4][0])
        assert 0 < n < c.post
        assert (r[0][0, n:] == 0).all() and np.isneginf(r[1][0, n:]).all() and (r[2][0, n:] == -1).all()
        assert (r[3][0, n:] == -1).all() and (r[5][n:, 0] == -1).all() and (r[5][n:, 1:] == 0).all()

    add(chain_case("post_above_everything", 1, [(3, 50), (2, 30)], 90, 300, [41, 42], check_padding))

    # ---- the select branch: its edge (A = 2049), one score for all, heavy ties, a larger random level
    def check_branch(c, r):
        assert "select" in c.branches and int(r[4].min()) > 0

    add(chain_case("select_edge_2049", 1, [(1, 2049), (1, 2048)], 2048, 4096, [51, 52], check_branch))
    o = [torch.full((1, 1, 1, 2049), 0.25), torch.full((1, 1, 1, 2048), 0.25)]
    d = [torch.zeros(1, 4, 1, 2049), torch.zeros(1, 4, 1, 2048)]

    def check_one_score(c, r):
        check_branch(c, r)
        assert np.array_equal(_kept_of_level(r, 0), np.arange(0, 100, 2))          # the first pre by index, every other kept
        assert np.array_equal(_kept_of_level(r, 1), np.arange(0, 100, 2))

    add(Case("select_one_score", o, d, [CHAIN_BASE] * 2, [CHAIN_STRIDE] * 2, chain_image([(1, 2049)]), 100, 4096,
             check=check_one_score))
    oq = (torch.randint(-6, 7, (2, 3, 40, 50), generator=g).to(F32) / 2)
    oq.view(-1)[::5] = -0.0
    dq = torch.randn(2, 12, 40, 50, generator=g) * 0.3
    o2, d2 = random_level(g, 2, 3, 20, 25)
    b3 = ops.pyramid_anchor_bases(((32,), (64,)), ((0.5, 1.0, 2.0),) * 2)

    def check_ties_large(c, r):
        check_branch(c, r)
        s = torch.sort(c.flat(0)[0], descending=True, stable=True).values
        assert s[c.pre - 1] == s[c.pre] and c.branches == ("select", "sort")

    add(Case("select_heavy_ties", [oq, o2], [dq, d2], b3, [(8, 8), (16, 16)], (320, 400), 1000, 600,
             check=check_ties_large))
    o1, d1 = random_level(g, 1, 3, 64, 80)
    o1 = torch.randn(1, 3, 64, 80, generator=g)                          # 15,360 logits, float ties only by chance
    o2, d2 = random_level(g, 1, 3, 32, 40)
    add(Case("select_large", [o1, o2], [d1, d2], b3, [(8, 8), (16, 16)], (512, 640), 2000, 2000, check=check_branch))

    # ---- empty results: nothing survives in image 1, beside a full image 0
    lv = [random_level(g, 2, 2, h, w) for h, w in ((4, 5), (2, 3))]
    o, d = [t for t, _ in lv], [t for _, t in lv]
    o[0][1] = nanp
    d[1][1, 2::4] = float("-inf")                                       # zero width

    def check_empty(c, r):
        assert int(r[4][0]) > 0 and int(r[4][1]) == 0
        assert (r[5][c.post:, 0] == -1).all() and np.isneginf(r[1][1]).all()

    add(Case("empty_image", o, d, [two * 4, two * 8], [(8, 8), (16, 16)], (64, 64), 30, 50, check=check_empty))
    return cases


def transposed(case, kind):
    """A copy of ``case`` whose inputs are laid out under a swapped convention: "hw" (the maps'
    memory read as [W, H]), "kc" (the deltas' channel as c*K + k), "yx" (the strides swapped)."""
    o, d, st = case.objectness, case.deltas, case.strides
    if kind == "hw":
        o = [t.transpose(2, 3).contiguous().view(t.shape) for t in o]
        d = [t.transpose(2, 3).contiguous().view(t.shape) for t in d]
    elif kind == "kc":
        K = case.K
        d = [t.view(t.shape[0], K, 4, *t.shape[2:]).transpose(1, 2).contiguous().view(t.shape) for t in d]
    elif kind == "yx":
        st = [(b, a) for a, b in st]
    else:
        raise KeyError(kind)
    return Case(case.name + "_" + kind, o, d, case.bases, st, case.image_sizes, case.pre, case.post,
                nms_thresh=case.nms_thresh, score_thresh=case.score_thresh, min_size=case.min_size)


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
NAMES = tuple(BY_NAME)
