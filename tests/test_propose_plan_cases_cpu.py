"""tests/propose_plan_cases.py on the oracle alone: the constants are read from
csrc/proposal.hip (loudly when a line is gone), every case reaches the plan branch it
names under each of its paths (the host's plan restated), the oracle's keep list is the
construction's closed form, and every case can catch what it is for: the ``post``-th
kept box lies in the chunk / stage meant, the truncated block would keep more, every
courier's target is kept without the courier, chains have their length inside a block,
the pinned anchors rank among the first ten, and the `whole` bucket equals the need."""
import numpy as np
import pytest

import propose_plan_cases as ppc
from oracle import ref_numpy as orc
from propose_plan_cases import CASES

CASE = pytest.mark.parametrize("case", CASES, ids=repr)


def group(*names):
    return pytest.mark.parametrize("case", [c for c in CASES if c.group in names], ids=repr)


# ----------------------------------------------------------------- the constants
def test_constants_are_the_ones_the_cases_were_sized_for():
    k = ppc.constants()
    assert (k.kChunk, k.kRun, k.kHistBins, k.kFusedMaxA, k.kMaskGrid, k.kSub) == (1024, 1024, 4096, 24576, 2048, 16)
    assert (k.post_wide, k.auto_n, k.auto_post) == (4096, 4, 1000)
    assert (k.stage0, k.stage1, k.stage_mul) == (48, 64, 2)
    assert (k.first0, k.first_div) == (64, 2)
    assert (k.kpt_a, k.kpt_b, k.kpt_c) == (8, 16, 24)
    assert (k.lds_chunk, k.lds_post, k.fix_rounds) == (28, 20, 65)


@pytest.mark.parametrize("gone", [
    "constexpr int kSub = 16;", "post > 4096", "N >= 4 || post <= 1000", "width = 48", "cb0 == 48 ? 64", "int f = 64;",
    "post + post / 2", "if (kpt <= 8)", "else if (kpt <= 16)", "post) * 20", "it < 65"])
def test_a_missing_source_line_fails_loudly(gone):
    with open(ppc.SOURCE) as f:
        src = f.read()
    assert gone in src
    ppc.read_constants(src)
    doctored = src.replace(gone, "/* moved */", 1) if gone != "it < 65" else src.replace(gone, "it < limit", 1)
    with pytest.raises(AssertionError, match="proposal.hip"):
        ppc.read_constants(doctored)


def test_a_changed_literal_is_read():
    with open(ppc.SOURCE) as f:
        src = f.read()
    k = ppc.read_constants(src.replace("post > 4096", "post > 2048").replace("else if (kpt <= 16) FRCNN_FUSED(16",
                                                                              "else if (kpt <= 12) FRCNN_FUSED(12"))
    assert (k.post_wide, k.kpt_b) == (2048, 12)


# -------------------------------------------------------------- the restated plan
def test_first_chunk_edges():
    for post, first in ppc.FIRST_CHUNK_EDGES:
        assert ppc.first_chunk(post) == first, post
    assert [ppc.first_chunk(p) for p in (1, 683, 4096)] == [64, 1024, 1024]
    assert {ppc.first_chunk(p) for p in range(1, 700)} == {64, 128, 256, 512, 1024}


def test_plan_edges():
    k = ppc.constants()
    assert [ppc.kpt(a) for a in (1, 8192, 8193, 16384, 16385, 24576)] == [8, 8, 16, 16, 24, 24]
    assert [ppc.nr(a) for a in (1024, 1025, 2048, 3000)] == [1, 2, 2, 3]
    assert ppc.stages(15361) == [(0, 48), (48, 112), (112, 240), (240, 241)]
    assert ppc.stages(3072) == [(0, 48)] and ppc.stages(3073) == [(0, 48), (48, 49)]
    for forced in ppc.FUSED:
        assert ppc.use_fused(1, k.kFusedMaxA, 4096, forced) and not ppc.use_fused(1, k.kFusedMaxA + 1, 100, forced)
        assert not ppc.use_fused(8, 5000, 4097, forced)
    assert ppc.use_fused(3, 4096, 1000) and not ppc.use_fused(3, 4096, 1001) and ppc.use_fused(4, 4096, 1001)
    assert not ppc.use_fused(8, 4096, 100, "wide")
    # the largest dynamic LDS request, within a CU's 160 KB
    assert ppc.fused_lds_bytes(4096) == 16384 + 28672 + 81920 <= 160 * 1024
    assert ppc.chunk_rows(1089, 30) == [64, 1024, 1] and ppc.chunk_rows(0, 30) == []


@CASE
def test_case_reaches_its_branch(case):
    assert set(case.want) == set(case.paths)
    for path, want in case.want.items():
        got = ppc.plan(case.N, case.A, case.pre, case.post, path)
        assert {k: got.get(k) for k in want} == want, (path, got)


def test_every_listed_branch_has_a_case():
    by = lambda g: [c for c in CASES if c.group == g]
    plans = {(c.group, p, tuple(sorted(w.items()))) for c in CASES for p, w in c.want.items()}
    assert {c.want["hybrid"].get("kpt") for c in by("ladder")} == {8, 16, 24, None}
    assert {c.A for c in by("ladder")} == {8192, 8193, 16384, 16385, 24576, 24577}
    for first in (64, 128, 256, 512, 1024):
        assert {c.chunk for c in by("first") if c.want["hybrid"].get("first") == first} >= {0, 1}, first
    assert {ppc.BY_NAME[f"first_edge_post{p}"].want["lazy"]["first"] for p in (171, 172)} == {256, 512}
    assert ppc.BY_NAME["post_4096"].want["hybrid"]["route"] == "hybrid"
    assert ppc.BY_NAME["post_4097"].want == {"auto": {"route": "wide"}, "hybrid": {"route": "wide"}}
    for kk in (8, 16):
        cont = [c for c in by("cont") if c.want["lazy"]["kpt"] == kk]
        assert {c.P for c in cont} >= {0, 1, 63, 64, 65, 128, 129, 700, 1089, 1153}
        assert max(c.chunk or 0 for c in cont) == 3
    assert {(c.chunk > 0, c.stage) for c in by("trunc")} == {(False, 0), (True, 0), (True, 1)}
    chains = {(c.chains[0][1], ppc.chunk_of(c.chains[0][0], c.post) > 0, c.stage) for c in by("fixed")}
    assert chains >= {(64, False, 0), (64, True, 0), (64, True, 1), (65, False, 0)}   # length, continuation, stage
    assert {c.P for c in by("stage")} == {3072, 3073, 7168, 7169}
    assert {c.want["wide"]["nr"] for c in by("sort")} == {1, 2, 3}
    assert {w["route"] for c in by("auto") for w in c.want.values()} == {"hybrid", "wide"}
    assert by("mixed")[0].N == 5 and set(by("mixed")[0].paths) == set(ppc.ALL_PATHS)
    assert by("mixed")[1].want["wide"]["stages"] == 3 and by("mixed")[1].stage == 2
    assert plans


# ------------------------------------------------- oracle == closed form, per image
@CASE
def test_oracle_keeps_the_closed_form(case):
    anchors = case.inputs()[0]
    for n, (rois, idx) in enumerate(case.reference()):
        erois, eidx = case.expected(n)
        assert np.array_equal(idx, eidx), n
        assert np.array_equal(rois.view(np.uint32), erois.view(np.uint32)), n
        assert np.array_equal(anchors[idx], rois)            # zero deltas: a decoded box is its anchor


def test_box_rule():
    """The rule closed_form walks, on the boxes: IoU over the threshold exactly for the same
    region at most one position apart."""
    region = np.array([5, 5, 5, 6, 69, ppc.CHAIN0, ppc.CHAIN0, ppc.CHAIN0, ppc.CHAIN0 + 1, ppc.CHAIN0 + 12, 6])   # (6: jittered twins)
    pos = np.array([0, 1, 2, 0, 0, 0, 1, 2, 0, 64, 0])
    jit = np.array([0, 0, 0, 2, 1, 0, 0, 0, 0, 0, 0])
    iou = orc.bbox_iou(*(ppc.boxes_of(region, pos, jit).astype(np.float64),) * 2)
    over = (region[:, None] == region[None]) & (abs(pos[:, None] - pos[None]) <= 1)
    assert np.array_equal(iou > ppc.THR, over)
    assert (iou[~over] < 0.61).all() and (iou[over] > 0.77).all() and (iou[region[:, None] != region[None]] == 0).all()


# ------------------------------------------- what a case must be able to catch
@CASE
def test_candidate_count_and_target(case):
    assert len(case.candidates(0)) == case.P
    keep = case.keep_ranks(case.timg)
    if case.target is None:
        assert case.group in ("cont", "auto") and (case.group == "auto" or len(keep) < case.post)
        return
    assert len(keep) >= case.post and keep[case.post - 1] == case.target
    if case.chunk is not None:
        assert ppc.chunk_of(case.target, case.post) == case.chunk
    if case.stage is not None:
        assert ppc.stage_of(case.target, min(case.pre, case.A)) == case.stage
    if case.rows is not None:
        assert ppc.chunk_rows(case.P, case.post) == case.rows


@group("cont")
def test_continuation_rows(case):
    assert case.rows is None or ppc.chunk_rows(case.P, case.post) == case.rows
    if case.P in (0, 1, 63, 64, 65):
        assert len(case.images[0].order) == case.P < case.pre           # limited by the valid count
    if case.name.startswith("cont_pre_limit"):
        assert len(case.images[0].order) == case.A > case.pre == case.P  # by pre, valid keys behind it


@group("ladder")
def test_ladder_top_ranks(case):
    cand, keep = case.candidates(0), case.keep_ranks(0)
    A = case.A
    assert sorted(case.top.values()) == [A - 1024, A - 2, A - 1]
    for rank, a in case.top.items():
        assert rank < 10 and cand[rank] == a and rank in keep[:case.post]
    assert (A - 1) // 1024 == -(-A // 1024) - 1               # A - 1 sits in the last register slot
    assert len(case.images[0].order) == A                     # every key is valid: the select sees them all


@group("trunc")
def test_truncated_block_would_keep_more(case):
    keep = case.keep_ranks(0)
    block = case.target // 64
    assert (keep[case.post:] // 64 == block).sum() >= 2
    assert (keep[:case.post - 1] // 64 == block).sum() >= 1   # and kept boxes before the post-th as well


@group("fixed")
def test_chain_lengths(case):
    cand, keep = case.candidates(0), case.keep_ranks(0)
    (r0, L), = case.chains
    a = cand[r0:r0 + L]
    assert (case.region[a] == case.region[a[0]]).all() and np.array_equal(case.pos[a], np.arange(L))
    assert np.array_equal(keep[(keep >= r0) & (keep < r0 + L)], np.arange(r0, r0 + L, 2))
    if L == 64:
        assert r0 % 64 == 0                                   # one block, filled exactly
    else:
        assert r0 // 64 != (r0 + L - 1) // 64 and r0 % 64     # across a block edge
    assert case.target > r0 + L                               # all of it lies before the post-th kept box
    if case.chunk:                                            # blocks of a continuation chunk start at its first row
        assert (r0 - ppc.first_chunk(case.post)) % 64 == 0 or L == 65
    if case.stage:
        assert ppc.stage_of(r0, case.pre) == 1


@group("route")
def test_courier_targets(case):
    keep = set(case.keep_ranks(0).tolist())
    for c, targets in case.couriers:
        without = set(case.keep_ranks(0, without=(c,)).tolist())
        assert c in keep
        for t in targets:
            assert c < t < case.target and t not in keep and t in without


def test_routes_lie_where_they_are_meant():
    c = ppc.BY_NAME["route_fused"]
    ch = lambda r: ppc.chunk_of(r, c.post)
    (c1, t1), (c2, t2) = c.couriers
    assert (ch(c1), [ch(t) for t in t1]) == (0, [1, 2]) and (ch(c2), [ch(t) for t in t2]) == (1, [2])
    c = ppc.BY_NAME["route_wide"]
    assert c.pre >= 7169
    sub = lambda r: ppc.substage_of(r, c.pre)
    (a, ta), (b, tb), (l, tl), (g, tg), (s, ts) = c.couriers
    assert sub(a)[0] == 0 and [sub(t)[0] for t in ta] == [1, 2]            # prehit, once and twice removed
    assert sub(b)[0] == 1 and sub(tb[0])[0] == 2                           # prehit from stage 1
    assert sub(l) == (1, 0) and sub(tl[0]) == (1, 2)                       # kept[] in LDS
    assert sub(g) == sub(tg[0]) == (1, 2) and g // 64 < tg[0] // 64        # col[] registers
    assert s // 64 == ts[0] // 64                                          # one block


@group("stage")
def test_stage_edge_keeps_in_the_last_block(case):
    keep = case.keep_ranks(0)
    assert keep[case.post - 1] == case.P - 1 and len(case.images[0].order) == case.P < case.pre
    assert len(case.inputs()[0]) > case.P                                  # invalid keys among them


@group("sort")
def test_sort_cases_have_interleaved_invalid_keys(case):
    valid = np.zeros(case.A, bool)
    valid[case.images[0].order] = True
    assert valid[::2].all() and not valid[1::2].any() and valid.sum() == case.P < case.pre


@group("select")
def test_select_cases(case):
    sc = case.inputs()[1][0]
    bits = np.unique(sc.view(np.uint32))
    if case.whole is None:
        assert len(bits) == 1
    else:       # two values that differ in the first digit; the upper one's count against the first need
        assert len(bits) == 2 and (bits >> 20)[0] != (bits >> 20)[1]
        assert (sc == sc.max()).sum() == case.whole
        assert case.whole - ppc.first_chunk(case.post) == (0 if case.name.endswith("256") else 1)
    assert np.array_equal(case.candidates(0), np.arange(case.P))           # the anchor index decides


def test_mixed_batch_images():
    c = ppc.BY_NAME["mixed_batch"]
    assert (c.N, c.pre, c.post) == (5, 6000, 300)
    P = [len(c.candidates(n)) for n in range(5)]
    kept = [len(c.keep_ranks(n)[:c.post]) for n in range(5)]
    assert P[0] <= 64 and kept[0] < c.post                     # done in its first 64-row block
    assert kept[1] == c.post and ppc.chunk_of(c.target, c.post) == 3 and ppc.stage_of(c.target, c.pre) == 1
    assert (P[2], kept[2]) == (0, 0) and (P[3], kept[3]) == (1, 1)
    assert P[4] == c.pre < len(c.images[4].order) and kept[4] == 200 < c.post


@group("auto")
def test_auto_cases_are_truncated_at_post(case):
    for n in range(case.N):
        assert len(case.keep_ranks(n)) > case.post


@pytest.mark.parametrize("n", ppc.NMS_SIZES)
def test_nms_cases(n):
    boxes, scores, keep = ppc.nms_case(n)
    assert np.array_equal(orc.nms(boxes, scores, ppc.THR), keep)
    order = np.argsort(-scores, kind="stable")
    assert keep[-1] == order[-1] and len(keep) == len(range(0, n, 40)) + ((n - 1) % 40 != 0)   # kept in the last block
    assert (np.diff(keep) < 0).any()                                       # not in index order
    assert len(ppc.stages(n)) == {3072: 1, 3073: 2, 7168: 2, 7169: 3, 15360: 3, 15361: 4}[n]
