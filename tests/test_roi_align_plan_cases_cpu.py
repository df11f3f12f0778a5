"""The RoIAlign launch plan without a GPU (tests/roi_align_plan_cases.py; DESIGN.md §3
"RoIAlign", "Launch-plan branches and the cases that pin them"): every named case reaches
the branch it names; the tiled restatement of the backward and the thread-wise one of the
forward equal the reference bit for bit; every planted structural mistake is told apart by
the cases that claim it, and none is left without a catcher; the numpy port of the host
launch numbers equals ``frcnn_roi_align_plan`` / ``frcnn_roi_align_multi_plan`` over a sweep."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import roi_align_plan_cases as PC  # noqa: E402
import roi_align_ref as ref  # noqa: E402
from replication_faster_rcnn_amd import _lib  # noqa: E402

F = np.float32
CASES = PC.cases()
IDS = [c.name for c in CASES]
HALF = {"f16": torch.float16, "bf16": torch.bfloat16}
_refs = {}


def reference(c):
    """(x, rois, grad, forward, backward) of a case, computed once."""
    if c.name not in _refs:
        x, rois, grad = c.inputs()
        _refs[c.name] = (x, rois, grad, ref.forward(x, rois, c.size, 1.0, c.sampling_ratio, c.aligned),
                         ref.backward(grad, rois, c.shape, 1.0, c.sampling_ratio, c.aligned))
    return _refs[c.name]


def planted(c, mistake):
    """True if the restatement with ``mistake`` planted differs from the reference on ``c``."""
    x, rois, grad, fwd, bwd = reference(c)
    if mistake.startswith("fwd_"):
        return not PC.forward_equals(PC.forward_threads(x, rois, c.size, 1.0, c.sampling_ratio, c.aligned, mistake), fwd)
    return not PC.backward_tiled(grad, rois, c.shape, 1.0, c.sampling_ratio, c.aligned, mistake).equals(bwd)


# ------------------------------------------- every case reaches what it names
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_case_reaches_what_it_names(c):
    c.check()
    assert c.catches, "a case that tells nothing apart"
    q = _lib.roi_align_plan(c.R, c.N, c.C, c.H, c.W, *c.size)
    assert {k: q[k] for k in c.plan()} == c.plan()
    paths = c.paths()
    assert ("guarded",) not in paths and ("empty",) not in paths
    print(c.name, sorted(set(paths)), {k: q[k] for k in ("units", "blocks", "idle", "staged")})


def test_table_pins_what_the_design_names():
    """The properties the table exists for, stated on the table itself."""
    k = PC.consts()
    by = {c.name: c for c in CASES}
    assert (k.RUN, k.TILE, k.STRIDE, k.WAVES, k.STAGE_BINS, k.SCAN, k.LANE) == (8, 8, 65, 5, 49, 16, 64)
    assert by["out14_unstaged"].size == (14, 14) and not PC.staged(14, 14)
    assert by["out5x10_first_unstaged"].size[0] * by["out5x10_first_unstaged"].size[1] == k.STAGE_BINS + 1
    # stride 49 != PHW 48 with all 64 channels: the stage's highest word is the 3135th of its 3136
    c = by["stage48_full"]
    _, rois, grad, _, _ = reference(c)
    t = PC.backward_tiled(grad, rois, c.shape, 1.0, c.sampling_ratio, c.aligned)
    assert PC.stage_stride(*c.size) == 49 and t.max_stage_word == 63 * 49 + 47 == 64 * k.STAGE_BINS - 2
    c = by["stage_even_small"]
    assert PC.stage_stride(*c.size) == 5 and [min(c.C - g * 64, 64) for g in range(2)] == [64, 6]
    assert c.plan()["tiles_x"] != c.plan()["tiles_y"] and c.N != c.plan()["cgroups"] > 1
    assert by["walk72_unstaged"].size[0] * 8 == 72 > k.LANE == by["walk72_unstaged"].size[1] * 8
    g = by["sr10_divide"].geoms()[0]
    assert g.count == 100 and not PC.pow2_count(g.count) and PC.pow2_count(F(64)) and PC.pow2_count(F(1))
    assert by["pw65"].size == (1, k.LANE + 1) and by["pw65"].sampling_ratio == 1
    # sample_on_edge: samples exactly at -1, on the interior tile edges, at y == H and x == W
    c = by["sample_on_edge"]
    ys, xs = PC.edge_positions(c)
    assert {-1.0, 8.0, 16.0, float(c.H)} <= ys and {-1.0, 8.0, 16.0, float(c.W)} <= xs
    assert all(v == int(v) for v in ys | xs)
    # adaptive_mixed: a bisected range ends on an interior tile edge (a == the first sample past it)
    c = by["adaptive_mixed"]
    g = c.geoms()[2]
    a, e = PC.align_range(g.sh + F(3) * g.bh, g.bh, g.gh, 7, 16, False)
    assert 0 < a < e < g.gh and ref.pos(g.sh + F(3) * g.bh, g.bh, g.gh, e - 1) < 16 <= ref.pos(
        g.sh + F(3) * g.bh, g.bh, g.gh, e)
    for name in ("r64", "r65", "r129"):
        assert by[name].R == int(name[1:]) and (np.diff(by[name].rois[:, 0]) != 0).all()   # images interleaved
    # every arm has a named case
    paths = {p for c in CASES for p in c.paths()}
    assert {("lane",)} | {("walk", a, b) for a in ("scan", "bisect") for b in ("scan", "bisect")} == paths
    assert {PC.staged(*c.size) for c in CASES} == {True, False}
    assert {(PC.staged(*c.size), c.paths()[0][0]) for c in CASES} == {(s, p) for s in (True, False)
                                                                      for p in ("lane", "walk")}


# ------------------------------------------ restatements against the reference
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_restatements_equal_the_reference(c):
    x, rois, grad, fwd, bwd = reference(c)
    t = PC.backward_tiled(grad, rois, c.shape, 1.0, c.sampling_ratio, c.aligned)
    assert (t.stores[:t.n] == 1).all(), "a grad_in element is not stored exactly once"
    assert not t.stores[t.n:].any() and t.lost == 0, "a store past grad_in"
    assert t.equals(bwd)
    assert PC.forward_equals(PC.forward_threads(x, rois, c.size, 1.0, c.sampling_ratio, c.aligned), fwd)


@pytest.mark.parametrize("dtype", sorted(HALF))
@pytest.mark.parametrize("c", [c for c in CASES if c.half], ids=[c.name for c in CASES if c.half])
def test_restatements_widen_run_round_once(c, dtype):
    dt = HALF[dtype]
    x, rois, grad = c.inputs()
    x16, g16 = torch.from_numpy(x).to(dt), torch.from_numpy(grad).to(dt)
    xw, gw = x16.float().numpy(), g16.float().numpy()

    def once(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dt).float().numpy()

    t = PC.backward_tiled(gw, rois, c.shape, 1.0, c.sampling_ratio, c.aligned)
    assert (t.stores[:t.n] == 1).all()
    assert ref.same_bits(once(t.grad_in), once(ref.backward(gw, rois, c.shape, 1.0, c.sampling_ratio, c.aligned)))
    out, stores = PC.forward_threads(xw, rois, c.size, 1.0, c.sampling_ratio, c.aligned)
    assert (stores == 1).all()
    assert ref.same_bits(once(out), once(ref.forward(xw, rois, c.size, 1.0, c.sampling_ratio, c.aligned)))


@pytest.mark.parametrize("rc", ref.CASES, ids=[c.name for c in ref.CASES])
def test_tiled_restatement_on_the_older_cases(rc):
    x, rois, grad = rc.inputs()
    t = PC.backward_tiled(grad, rois, x.shape, 1.0, rc.sampling_ratio, rc.aligned)
    assert t.equals(ref.backward(grad, rois, x.shape, 1.0, rc.sampling_ratio, rc.aligned))


# ------------------------------------------------------------ planted mistakes
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_case_tells_its_mistakes_apart(c):
    for mistake in c.catches:
        assert planted(c, mistake), f"{c.name} does not tell {mistake} from the reference"


def test_every_mistake_has_a_catcher():
    """The matrix, printed; a mistake without a catching case fails."""
    old = {rc.name: rc for rc in ref.CASES}
    catchers = {m: [c.name for c in CASES if m in c.catches] for m in PC.MISTAKES}
    for name, m in PC.REF_CATCHERS:
        rc = old[name]
        x, rois, grad = rc.inputs()
        want = ref.backward(grad, rois, x.shape, 1.0, rc.sampling_ratio, rc.aligned)
        assert not PC.backward_tiled(grad, rois, x.shape, 1.0, rc.sampling_ratio, rc.aligned, m).equals(want), (name, m)
        catchers[m].append(name)
    width = max(map(len, PC.MISTAKES))
    for m in PC.MISTAKES:
        print(f"{m:{width}s}  {', '.join(catchers[m]) or '-'}")
    assert not [m for m in PC.MISTAKES if not catchers[m]]


def test_shapes_where_a_mistake_hides():
    """Why the table has the shapes it has: the older cases cannot see these mistakes."""
    old = {rc.name: rc for rc in ref.CASES}
    rc = old["c70"]                                  # 2 x 2 tiles, N == cgroups == 2
    x, rois, grad = rc.inputs()
    want = ref.backward(grad, rois, x.shape, 1.0, rc.sampling_ratio, rc.aligned)
    for m in ("cg_b_swapped", "tile_div_mod_swapped"):
        assert PC.backward_tiled(grad, rois, x.shape, 1.0, rc.sampling_ratio, rc.aligned, m).equals(want), m
    # one chunk only: the order of chunks cannot show; 50 bins with 5 channels: the stage does not overrun
    assert not planted(PC.case("r64"), "chunks_reversed") and not planted(PC.case("r64"), "chunk_tail_dropped")
    c = PC.case("out5x10_first_unstaged")
    x, rois, grad, _, _ = reference(c)
    few = grad[:, :5].copy()
    want = ref.backward(few, rois, (c.N, 5, c.H, c.W), 1.0, c.sampling_ratio, c.aligned)
    assert PC.backward_tiled(few, rois, (c.N, 5, c.H, c.W), 1.0, c.sampling_ratio, c.aligned, "stage_limit_50").equals(want)


# ------------------------------------------------------- the port and the query
def test_query_fields_and_validation():
    lib = _lib.load(require_gpu=False)
    buf = (ctypes.c_int64 * 17)()
    assert lib.frcnn_roi_align_plan(1, 1, 1, 8, 8, 7, 7, None) == -1 and b"null" in lib.frcnn_last_error()
    for args, word in [((1, 1, 1, 8, 8, 0, 7), b"output_size"), ((1, 1, 1, 8, 8, 7, -1), b"output_size"),
                       ((-1, 1, 1, 8, 8, 7, 7), b"shape"), ((1, 1, 1, (1 << 24) + 1, 8, 7, 7), b"2^24")]:
        assert lib.frcnn_roi_align_plan(*args, buf) == -1 and word in lib.frcnn_last_error(), args
    # 2^31 tiles: the backward refuses the map, and so does the query, in the launch's words
    big = 1 << 19
    assert PC.plan(1, 1, 1, big, big, 7, 7) is None
    assert lib.frcnn_roi_align_plan(1, 1, 1, big, big, 7, 7, buf) == -1
    why = lib.frcnn_last_error().split(b": ", 1)[1]
    assert b"map too large" in why
    one = (ctypes.c_float * 8)()
    p = ctypes.addressof(one)
    assert lib.frcnn_roi_align_bwd_t(0, p, p, 1, 1, 1, big, big, 7, 7, 1.0, 2, 0, p, None, 0, None) == -1
    assert lib.frcnn_last_error().split(b": ", 1)[1] == why
    assert PC.plan(1, 1, 1, big, big // 2 - 8, 7, 7)["units"] < 1 << 31
    assert _lib.ROI_ALIGN_PLAN_FIELDS[7:] == tuple(PC.plan(1, 1, 1, 1, 1, 1, 1))
    # the pyramid form
    m = (ctypes.c_int64 * 14)()
    hw = (ctypes.c_int * 2)(8, 8)
    assert lib.frcnn_roi_align_multi_plan(0, hw, hw, 1, 1, 7, 7, m) == -1 and b"n_levels" in lib.frcnn_last_error()
    assert lib.frcnn_roi_align_multi_plan(9, hw, hw, 1, 1, 7, 7, m) == -1
    assert lib.frcnn_roi_align_multi_plan(2, None, hw, 1, 1, 7, 7, m) == -1 and b"null" in lib.frcnn_last_error()
    assert lib.frcnn_roi_align_multi_plan(2, hw, hw, 1, 1, 7, 7, None) == -1


def test_port_equals_query_over_the_sweep():
    """Zero shapes, the tile and channel-group edges, R around the chunk, outputs around the
    staging limit."""
    lib = _lib.load(require_gpu=False)
    buf = (ctypes.c_int64 * 17)()
    n = 0
    seen_idle = set()
    for R in (0, 1, 64, 65, 1000):
        for N in (0, 1, 2, 3):
            for C in (0, 1, 8, 9, 63, 64, 65, 128, 129):
                for H, W in [(0, 0), (0, 5), (5, 0), (1, 1), (8, 8), (8, 9), (9, 8), (16, 17), (17, 16), (7, 203),
                             (203, 7), (64, 80)]:
                    for PH, PW in [(1, 1), (7, 7), (6, 8), (5, 10), (7, 8), (14, 14), (1, 65)]:
                        assert lib.frcnn_roi_align_plan(R, N, C, H, W, PH, PW, buf) == 0, lib.frcnn_last_error()
                        got = dict(zip(_lib.ROI_ALIGN_PLAN_FIELDS, buf))
                        want = PC.plan(R, N, C, H, W, PH, PW)
                        assert {k: got[k] for k in want} == want, (R, N, C, H, W, PH, PW, got)
                        seen_idle.add(got["idle"])
                        n += 1
    assert seen_idle == set(range(5))
    print(f"{n} plans")
    # shapes with nothing to launch
    assert PC.plan(5, 0, 3, 8, 8, 7, 7)["units"] == 0 == PC.plan(5, 0, 3, 8, 8, 7, 7)["fwd_threads"]
    assert PC.plan(5, 2, 0, 8, 8, 7, 7)["blocks"] == 0 and PC.plan(0, 2, 3, 8, 8, 7, 7)["fwd_grid"] == 0
    assert PC.plan(0, 2, 3, 8, 8, 7, 7)["units"] == 2


def test_pyramid_first_equals_query():
    for sizes, N, C in [(PC.STRADDLE["sizes"], 2, 5), (PC.EMPTY_MIDDLE["sizes"], 2, 5), ([(8, 8)], 1, 1),
                        ([(0, 0)], 2, 3), ([(64, 80), (32, 40), (16, 20), (8, 10)], 2, 70),
                        ([(65, 66), (33, 33), (17, 17), (9, 9), (5, 5), (3, 3), (2, 2), (1, 1)], 1, 5),
                        ([(9, 9), (5, 5)], 0, 5), ([(9, 9), (5, 5)], 2, 0)]:
        q = _lib.roi_align_multi_plan(sizes, N, C, 14, 14)
        first = PC.multi_first(sizes, N, C)
        k = PC.consts()
        assert q["first"] == first and q["units"] == first[-1], (sizes, q)
        assert q["blocks"] == (first[-1] + k.WAVES - 1) // k.WAVES and q["idle"] == q["blocks"] * k.WAVES - q["units"]
        assert q["staged"] == 0
    s = PC.STRADDLE
    q = _lib.roi_align_multi_plan(s["sizes"], s["N"], s["C"])
    assert q["first"][:3] == s["first"] and q["units"] == s["units"] and q["idle"] == 2 and q["staged"] == 1
    # workgroup 3 holds the units 15..19 (levels 0 and 1), workgroup 5 the units 25..27 (levels 1 and 2)
    assert 15 < s["first"][1] <= 19 and 25 < s["first"][2] <= 27
    e = _lib.roi_align_multi_plan(PC.EMPTY_MIDDLE["sizes"], 2, 5)
    assert e["first"][1] == e["first"][2] > 0 and e["units"] > e["first"][2]
