"""The preprocessing launch plan without a GPU (tests/preprocess_plan_cases.py;
DESIGN.md §3 "Preprocessing", "Launch-plan branches and the cases that pin
them"): the numpy port of the host plan against ``frcnn_preprocess_plan`` on
the case table, the tile-height ladder and a sweep; the footprint bound the
kernel's clamp would otherwise hide; that every case reaches the plan it
names; the banded reference against the dense one; and that every structural
mistake planted in the tiled restatement is told apart from the reference by
the cases that claim it."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import preprocess_plan_cases as PC  # noqa: E402
import preprocess_ref as R  # noqa: E402
from replication_faster_rcnn_amd import _lib  # noqa: E402

SWEEP_OUT = range(1, 131)
TILE_HEIGHTS = (32, 16, 8, 4, 2, 1)
MARGIN = 3.0      # a mistake is told apart at max |mutant - reference| >= 3 x the case's tolerance


def sweep_max_in(n_out):
    return range(1, PC.MAX_RATIO * n_out + 4)


def query(lib, buf, N, max_hw, out_hw):
    rc = lib.frcnn_preprocess_plan(N, max_hw[0], max_hw[1], out_hw[0], out_hw[1], buf)
    assert rc == 0, (max_hw, out_hw, lib.frcnn_last_error())
    return dict(zip(PC.PLAN_FIELDS, buf))


# --------------------------------------------------------------- plans agree
def test_query_fields_and_validation():
    """The query names its fields as the port does and rejects what
    frcnn_preprocess rejects, with the same reason."""
    assert _lib.PREPROCESS_PLAN_FIELDS == PC.PLAN_FIELDS
    lib = _lib.load(require_gpu=False)
    buf = (ctypes.c_int32 * 8)()
    mean, std = (ctypes.c_float * 3)(*R.MEAN), (ctypes.c_float * 3)(*R.STD)
    for args in [(0, 8, 8, 4, 4), (1025, 8, 8, 4, 4), (1, 0, 8, 4, 4), (1, 8, 16385, 4, 4), (1, 8, 8, 0, 4),
                 (1, 8, 8, 4, 4097)]:
        assert lib.frcnn_preprocess_plan(*args, buf) == -1
        why = lib.frcnn_last_error().split(b": ", 1)[1]
        assert lib.frcnn_preprocess(args[0], None, 0, None, None, *args[1:], mean, std, None, None, None, 0, None) == -1
        assert lib.frcnn_last_error().split(b": ", 1)[1] == why and b" must be in " in why
    assert lib.frcnn_preprocess_plan(1, 8, 8, 4, 4, None) == -1 and b"null" in lib.frcnn_last_error()
    assert lib.frcnn_preprocess_plan(1024, 16384, 16384, 4096, 4096, buf) == 0
    assert _lib.preprocess_plan(3, (8, 8), (4, 4)) == PC.plan(3, (8, 8), (4, 4))


@pytest.mark.parametrize("c", PC.CASES, ids=PC.CASE_IDS)
def test_port_equals_query_on_cases(c):
    for max_hw in (c.in_hw, (min(5 * c.out_hw[0], 16384), min(5 * c.out_hw[1], 16384)), (16384, 16384)):
        for N in (1, 4):
            assert PC.plan(N, max_hw, c.out_hw) == _lib.preprocess_plan(N, max_hw, c.out_hw), max_hw


def test_ladder_takes_five_tile_heights():
    got = []
    for max_hw, th in PC.LADDER:
        p = _lib.preprocess_plan(1, max_hw, PC.LADDER_OUT)
        assert p == PC.plan(1, max_hw, PC.LADDER_OUT) and p["TH"] == th, (max_hw, p)
        assert PC.LADDER_IMAGE[0] <= max_hw[0] and PC.LADDER_IMAGE[1] <= max_hw[1]
        got.append(p["TH"])
    assert got == [32, 16, 8, 4, 2] and PC.LADDER[0][0] == PC.LADDER_IMAGE
    assert PC.axis_radius(PC.LADDER_IMAGE[1], PC.LADDER_OUT[1]) > 0 and PC.LADDER_IMAGE[0] <= PC.LADDER_OUT[0]


def test_port_equals_query_over_the_sweep():
    """out in 1..130, max_in in 1..5*out+3, on each axis beside three settings of
    the other (smallest, ratio 5, the widest accepted), and both axes together at
    their worst (max_in = 5*out+3).  Every plan fits the LDS budget at TH >= 2:
    the TH == 1 rung of the host's loop and its "internal" error are never taken
    (at ratio 5 on both axes TH 2 needs 48,592 B, and span_bound caps the ratio at 5)."""
    lib = _lib.load(require_gpu=False)
    buf = (ctypes.c_int32 * 8)()
    others = [(1, 1), (40, 200), (4096, 16384)]
    seen_th, worst = set(), 0
    n = 0

    def one(max_hw, out_hw):
        nonlocal worst, n
        p = query(lib, buf, 1, max_hw, out_hw)
        assert p == PC.plan(1, max_hw, out_hw), (max_hw, out_hw, p)
        assert p["lds_bytes"] <= PC.LDS_BUDGET and p["TH"] >= 2, (max_hw, out_hw, p)
        seen_th.add(p["TH"])
        worst = max(worst, p["lds_bytes"])
        n += 1

    for out in SWEEP_OUT:
        for max_in in sweep_max_in(out):
            for o_out, o_max in others:
                one((max_in, o_max), (out, o_out))
                one((o_max, max_in), (o_out, out))
    for out_h in SWEEP_OUT:
        for out_w in SWEEP_OUT:
            one((5 * out_h + 3, 5 * out_w + 3), (out_h, out_w))
    print(f"{n} plans, tile heights {sorted(seen_th)}, largest LDS {worst} B")
    assert seen_th == {32, 16, 8, 4, 2}
    # the worst corner, named: ratio 5 on both axes
    p = query(lib, buf, 1, (16384, 16384), (130, 130))
    assert (p["TH"], p["lds_rows"], p["lds_cols"], p["lds_bytes"]) == (2, 23, 333, 48592)
    assert PC.plan(1, (16384, 16384), (130, 130), min_th=32)["lds_bytes"] > PC.LDS_BUDGET


# ------------------------------------------------------ the clamp never bites
def test_footprint_bound_holds_over_the_sweep():
    """For every accepted (n_in, n_out) of the sweep, every tile length the host
    can pick and every tile origin, the rows (columns) the tile reaches are
    <= span_bound at the tightest host bound (max_in = n_in; the bound only
    grows with max_in).  The kernel's ``nrows < lds_rows ? nrows : lds_rows``
    would turn a violation into wrong pixels, not a fault."""
    tight = 0
    for n_out in SWEEP_OUT:
        n_in = np.arange(1, PC.MAX_RATIO * n_out + 1)
        r = np.array([PC.axis_radius(int(n), n_out) for n in n_in])
        start = PC.tap_start(n_in[:, None], n_out, np.arange(n_out)[None, :])
        prev = None
        for L in (PC.TW,) + TILE_HEIGHTS:
            d0 = np.arange(0, n_out, L)
            last = np.minimum(d0 + L, n_out) - 1
            span = (start[:, last] - start[:, d0]).max(1) + 2 + 2 * r
            bound = np.array([PC.span_bound(L, int(n), n_out) for n in n_in])
            bad = np.nonzero(span > bound)[0]
            assert bad.size == 0, (n_out, L, n_in[bad][:4], span[bad][:4], bound[bad][:4])
            tight += int((span == bound).sum())
            # the bound grows with the host's max_in, so max_in = n_in is the tightest
            assert (np.diff(bound) >= 0).all()
            prev = bound
        assert prev is not None
    assert tight > 0, "the bound is reached somewhere: it is not slack everywhere"
    # the vectorised span is the restatement's own
    for n_in, n_out, d0, L in [(60, 12, 10, 2), (161, 70, 64, 64), (2, 1, 0, 32), (650, 130, 128, 64)]:
        last = min(d0 + L, n_out) - 1
        want = int(PC.tap_start(n_in, n_out, last) - PC.tap_start(n_in, n_out, d0)) + 2 + 2 * PC.axis_radius(n_in, n_out)
        assert PC.axis_span(n_in, n_out, d0, L) == want


@pytest.mark.parametrize("c", PC.CASES, ids=PC.CASE_IDS)
def test_footprint_bound_holds_on_cases(c):
    """The footprints the tiled restatement computes, tile by tile, under the
    case's own plan: never above lds_rows x lds_cols, and equal to axis_span."""
    p = PC.plan(1, c.in_hw, c.out_hw)
    trace = []
    PC.tiled(PC.case_image(c), c.out_hw, p, trace=trace)
    assert len(trace) == p["grid_x"] * p["grid_y"]
    for y0, x0, ny, nx, nrows, ncols in trace:
        assert nrows <= p["lds_rows"] and ncols <= p["lds_cols"], (y0, x0, nrows, ncols, p)
        assert nrows == PC.axis_span(c.in_hw[0], c.out_hw[0], y0, p["TH"])
        assert ncols == PC.axis_span(c.in_hw[1], c.out_hw[1], x0, PC.TW)


# ------------------------------------------- every case reaches what it names
@pytest.mark.parametrize("c", PC.CASES, ids=PC.CASE_IDS)
def test_case_reaches_what_it_names(c):
    p = _lib.preprocess_plan(1, c.in_hw, c.out_hw)
    rh, rw = PC.axis_radius(c.in_hw[0], c.out_hw[0]), PC.axis_radius(c.in_hw[1], c.out_hw[1])
    assert (rh, rw) == c.r == (R.sigma_radius(c.in_hw[0], c.out_hw[0])[1], R.sigma_radius(c.in_hw[1], c.out_hw[1])[1])
    assert (R.taps(c.in_hw[0], c.out_hw[0]), R.taps(c.in_hw[1], c.out_hw[1])) == (2 + 2 * rh, 2 + 2 * rw)
    assert p["TH"] == c.TH and (p["lds_rows"], p["lds_cols"], p["lds_bytes"]) == c.lds, p
    assert (p["grid_y"], p["grid_x"]) == c.tiles and p["max_taps"] == 2 + 2 * max(rh, rw)
    last = (c.out_hw[0] - (c.tiles[0] - 1) * c.TH, c.out_hw[1] - (c.tiles[1] - 1) * PC.TW)
    assert last == c.last and 1 <= last[0] <= c.TH and 1 <= last[1] <= PC.TW
    assert c.fast == ((rh | rw) == 0)
    assert set(c.catches) <= set(PC.MISTAKES) and c.catches


def test_table_pins_what_the_design_names():
    """The properties the table exists for, stated on the table itself."""
    by = {c.id: c for c in PC.CASES}
    assert by["down_x_tiles"].tiles == (3, 2) and by["down_x_tiles"].last == (13, 36) and by["down_x_tiles"].TH == 16
    assert by["down_x_tiles"].lds[:2] == (36, 132)
    # ratio 2.3: int(4 s) = 2, int(4 s + 0.5) = 3
    s = (161 / 70 - 1) / 2
    assert by["radius_rounds_up"].r == (3, 3) and int(4 * s) == 2 and int(4 * (46 / 20 - 1) / 2) == 2
    assert by["radius_rounds_up"].last[1] == 6
    assert by["ratio5"].r == (PC.GAUSS // 2,) * 2 and by["ratio5"].TH == 2 and by["ratio5"].lds == (23, 333, 48592)
    assert R.taps(60, 12) == 18 and by["ratio5"].in_hw == (5 * 12, 5 * 12)
    assert by["ratio5_wide"].tiles[1] == 3 and by["ratio5_wide"].last[1] == 2 and by["ratio5_wide"].r[1] == 8
    assert by["down_up"].r == (4, 0) and by["up_down"].r == (0, 4) and not by["down_up"].fast
    assert by["up_down"].TH == 32 and by["up_down"].last[0] == 18
    assert by["w64"].tiles[1] == 1 and by["w64"].last[1] == 64 and by["w65"].tiles[1] == 2 and by["w65"].last[1] == 1
    assert by["h33_slow"].TH == 16 and by["h33_slow"].last[0] == 1 and not by["h33_slow"].fast
    assert by["h33_fast"].TH == 32 and by["h33_fast"].last[0] == 1 and by["h33_fast"].fast
    assert by["h33_th32"].TH == 32 and by["h33_th32"].last[0] == 1 and not by["h33_th32"].fast
    assert by["two_rows"].in_hw[0] == 2 and by["two_rows"].r[0] == 2 and by["two_by_two"].in_hw == (2, 2)
    assert by["one_row"].in_hw[0] == 1 and by["one_row"].r == (0, 2) and by["one_row"].last[1] == 1
    assert by["voc_down"].lds[2] == 62336
    m = by["max_extent"]
    assert m.in_hw[1] == 16384 and m.out_hw[1] == 4096 and m.tiles[1] == 64 and m.last[1] == 64
    assert 2 ** 27 - 2 ** 15 < (2 * (m.out_hw[1] - 1) + 1) * m.in_hw[1] - m.out_hw[1] < 2 ** 27
    assert [c.fast for c in PC.CASES].count(True) == 1
    assert {c.TH for c in PC.CASES} == {32, 16, 2}       # 8 and 4 come from the ladder
    assert {k for c in PC.CASES for k in c.kinds} == {"random", "checker"}
    assert by["ratio5"].kinds == by["two_rows"].kinds == ("random", "checker")


# ------------------------------------------- banded and tiled against the dense
def test_banded_matrix_equals_the_dense_one():
    pairs = {(c.in_hw[a], c.out_hw[a]) for c in PC.CASES if c.id not in PC.BANDED_ONLY for a in (0, 1)}
    pairs |= {(c[1][a], c[2][a]) for c in R.CASES for a in (0, 1)} | {PC.LADDER_IMAGE[1:] + PC.LADDER_OUT[1:]}
    pairs |= {(2, 1), (1, 4), (16, 4), (7, 7)}
    worst = 0.0
    for n_in, n_out in sorted(pairs):
        idx, w = PC.axis_band(n_in, n_out)
        assert idx.shape == w.shape == (n_out, R.taps(n_in, n_out)) and idx.min() >= 0 and idx.max() < n_in
        err = np.abs(PC.band_dense(idx, w, n_in) - R.axis_matrix(n_in, n_out)).max()
        worst = max(worst, err)
        assert err <= 1e-15, (n_in, n_out, err)
    print(f"{len(pairs)} axes, max |banded - dense| = {worst:.3g}")
    # the widest axis: rows sum to 1, indices inside the image
    idx, w = PC.axis_band(16384, 4096)
    assert np.abs(w.sum(1) - 1).max() < 1e-15 and idx.min() >= 0 and idx.max() == 16383


@pytest.mark.parametrize("c", PC.CASES, ids=PC.CASE_IDS)
def test_tiled_restatement_equals_the_reference(c):
    for kind in c.kinds:
        img, ref = PC.case_data(c, kind)
        if c.id not in PC.BANDED_ONLY:
            assert np.abs(PC.preprocess_banded(img, c.out_hw) - ref).max() <= 1e-12
        got = PC.tiled(img, c.out_hw, PC.plan(1, c.in_hw, c.out_hw))
        err = np.abs(got - ref).max()
        print(f"{c.id}/{kind}: max |tiled - reference| = {err:.3g}")
        assert got.shape == ref.shape and err <= 1e-12


def test_tiled_restatement_does_not_depend_on_the_tile_height():
    img, ref = PC.ladder_data()
    for max_hw, _ in PC.LADDER:
        assert np.abs(PC.tiled(img, PC.LADDER_OUT, PC.plan(1, max_hw, PC.LADDER_OUT)) - ref).max() <= 1e-12


# ------------------------------------------------------------ planted mistakes
_margins = {}


def margin(c, mistake):
    """max |mutant - reference| over the case's tolerance; reference against
    mutant only, the device is not involved."""
    key = (c.id, mistake)
    if key not in _margins:
        img, ref = PC.case_data(c)
        got = PC.tiled(img, c.out_hw, PC.plan(1, c.in_hw, c.out_hw), mistake=mistake)
        _margins[key] = float(np.abs(got - ref).max() / R.tolerance(c.in_hw, c.out_hw))
    return _margins[key]


@pytest.mark.parametrize("mistake", PC.MISTAKES)
def test_planted_mistake_is_told_apart(mistake):
    claimed = [c for c in PC.CASES if mistake in c.catches]
    assert claimed, f"no case claims {mistake}"
    for c in claimed:
        m = margin(c, mistake)
        print(f"{mistake} on {c.id}: {m:.3g} x tolerance")
        assert m >= MARGIN, (mistake, c.id, m)


def test_margins_the_design_records():
    """int(4 s) is invisible at every integer ratio, which is why
    radius_rounds_up exists; the other figures of DESIGN.md's table hold at
    3 x at least."""
    for cid in ("down_x_tiles", "ratio5", "down_up", "up_down"):
        assert margin(PC.case(cid), "radius_trunc") < 1e-6, cid
    assert margin(PC.case("radius_rounds_up"), "radius_trunc") >= MARGIN
    for mistake, cid in [("fold_edge_repeat", "w65"), ("fold_edge_repeat", "down_up"), ("drop_last_tap", "ratio5"),
                         ("drop_last_tap", "down_x_tiles")]:
        assert margin(PC.case(cid), mistake) >= MARGIN, (mistake, cid)
    # an edge-repeat fold cannot show at 2 -> 1: the weights are symmetric about position 0.5, so either
    # fold gives each of the two pixels half
    assert margin(PC.case("two_by_two"), "fold_edge_repeat") < 1e-6
