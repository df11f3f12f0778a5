"""tests/pool_plan_cases.py on the oracle alone: every case reaches the plan branch it
names (the host's plan restated over the constants read from csrc/roi_pool.hip, at an
MI355X's 256 CUs) and can catch what it is for -- empty and non-empty bins, a tie that
only first-max breaks rightly, gradients whose bits depend on the summation order, and,
above 64 bins, argmax pixels shared across and within the backward's 64-bin chunks."""
import numpy as np
import pytest

import pool_plan_cases as ppc
from pool_plan_cases import BWD_CASES, CASES

CASE = pytest.mark.parametrize("case", CASES, ids=repr)


def test_constants_are_the_ones_the_cases_were_sized_for():
    """The shapes in the table were worked out for these values; a change here means
    re-deriving them (the plan tests below say which cases moved)."""
    k = ppc.constants()
    assert (k.kLdsPerCu, k.kPlaneBudget, k.kPlaneBudgetRing) == (160 * 1024, 64 * 1024, 144 * 1024)
    assert (k.kBwdXRow, k.kMaxBins, k.kBwdRing, k.kBwdLead) == (80, 1024, 8, 4)


@CASE
def test_case_reaches_its_forward_branch(case):
    for grouped, want in zip((True, False), case.fwd):
        assert ppc.fwd_plan(case.N, case.C, case.H, case.W, *case.size, grouped) == want, grouped


@pytest.mark.parametrize("case", BWD_CASES, ids=repr)
def test_case_reaches_its_backward_branch(case):
    for path, want in case.bwd.items():
        kind, icpw = ppc.bwd_plan(case.R, case.N, case.C, case.H, case.W, *case.size, path)
        assert kind == want, path
        if case.icpw:
            assert icpw == case.icpw[path], path


def test_every_listed_branch_has_a_case():
    fwd = {(c.group, f[0]) for c in CASES for f in c.fwd}
    assert {("bins", "generic"), ("budget", "generic"), ("wide", "generic"), ("tile", "wave"),
            ("tile", "generic")} <= fwd
    assert any(c.group == "bins" and c.fwd[0] == ("generic", False) for c in CASES)     # scalar stores
    bwd = {(c.group, p, k) for c in CASES for p, k in c.bwd.items()}
    assert {("bins", "auto", "plain_lds"), ("global", "plain", "plain_global"),
            ("budget", "auto", "lead"), ("budget", "auto", "pf"), ("budget", "auto", "plain_global"),
            ("partial", "auto", "lead"), ("partial", "ring", "pf"), ("partial", "plain", "plain_lds"),
            ("partial", "plain", "plain_global")} <= bwd
    assert {c.size for c in CASES if c.group == "bins"} >= {(13, 5), (9, 9), (14, 14), (1, 65), (65, 1),
                                                            (3, 341), (32, 32)}
    assert max(c.PHW for c in CASES) == ppc.constants().kMaxBins
    for ph, pw in ppc.REJECTED_SIZES:
        assert not 0 < ph * pw <= ppc.constants().kMaxBins


def test_budget_window_is_tight():
    """The four maps sit on consecutive edges of kPlaneBudgetRing: the leader's LDS need
    crosses it between 190 and 191, the plane itself between 192 x 192 (equal) and 192 x 193."""
    k = ppc.constants()
    lead = lambda h, w: ((h * w + 67) & ~3) * 4 + 2 * k.kBwdXRow * 8
    assert lead(190, 190) <= k.kPlaneBudgetRing < lead(191, 191)
    assert 191 * 191 * 4 < k.kPlaneBudgetRing == 192 * 192 * 4 < 192 * 193 * 4
    assert 130 * 130 * 4 > k.kPlaneBudget and k.kPlaneBudgetRing // (130 * 130 * 4) == 2
    # the 4-channel wave tile: 98 x 103 fills the CU's LDS to the byte, one pixel group more does not
    need = lambda hw: ((hw + 16) & ~15) * 16 + 64 * 16 + k.kWaveScratch + 1024
    assert need(98 * 103) == k.kLdsPerCu < need(99 * 102)


def test_fits_guard_edge():
    s = ppc.FITS_SHAPE
    r = ppc.fits_edge(s["C"], 49)
    assert r * s["C"] * 49 * 4 < 2 ** 31 <= (r + 1) * s["C"] * 49 * 4
    for dt in ppc.ALL:
        assert "roi_pool_bwd_lead_kernel" in ppc.bwd_name(dt, r, s["N"], s["C"], s["H"], s["W"], 7, 7)
        assert "roi_pool_bwd_pf_kernel" in ppc.bwd_name(dt, r + 1, s["N"], s["C"], s["H"], s["W"], 7, 7)


def test_names_of_the_benchmark_shapes():
    """The restated plans give the names tests/test_gpu_pool_half.py::test_name_queries
    pins for the library itself."""
    assert ppc.fwd_name("f32", 8, 256, 38, 63, 7, 7, True, head=True) == \
        "roi_pool_fwd_wave_kernel<1024, 16, 7, true, false, 38400>"
    assert ppc.fwd_name("f32", 1, 512, 50, 84, 7, 7, True, head=True) == "roi_pool_fwd_wave_kernel<1024, 8, 7, true>"
    assert ppc.fwd_name("f16", 8, 256, 38, 63, 7, 7, False) == \
        "roi_pool_fwd_dense_kernel_h<__half, 1024, 16, 7, false, true>"
    assert ppc.bwd_name("f32", 2048, 16, 256, 38, 38, 7, 7) == "roi_pool_bwd_lead_kernel<4, 7, 7>"
    assert ppc.bwd_name("bf16", 2048, 16, 256, 38, 38, 9, 7) == "roi_pool_bwd_lead_kernel_h<__hip_bfloat16, 4, 7, 0>"
    assert ppc.bwd_name("f32", 2048, 16, 256, 38, 38, 5, 5) == "roi_pool_bwd_pf_kernel<8>"
    assert ppc.bwd_name("f16", 2048, 16, 256, 38, 38, 7, 7, "plain") == "roi_pool_bwd_kernel_h<__half, true>"
    assert ppc.bwd_name("f16", 6, 1, 2, 130, 130, 7, 7, "plain") == "roi_pool_bwd_kernel_h<__half, false>"


@CASE
def test_case_inputs(case):
    x, rois, perm = case.inputs()
    assert x.dtype == np.float32 and rois.dtype == np.float32 and rois.shape == (case.R, 5)
    assert sorted(perm) == list(range(case.R))
    if len(np.unique(rois[:, 0])) > 1:
        assert (np.diff(case.rois(False)[:, 0]) < 0).any()      # the ungrouped order is not grouped
    b = rois[:, 0].astype(np.int64)
    per_image = np.bincount(b[(b >= 0) & (b < case.N)], minlength=case.N)
    if case.N >= 3:
        assert 0 in per_image and 1 in per_image
    assert ((b < 0) | (b >= case.N)).any() == case.invalid
    w, h = rois[:, 3] - rois[:, 1], rois[:, 4] - rois[:, 2]
    assert ((w == 0) & (h == 0)).any() and (w < 0).any()                    # zero and negative size
    assert len(np.unique(rois, axis=0)) < len(rois)                         # duplicated RoIs
    assert (rois[:, 3] < 0).any() and (rois[:, 1] < 0).any()                # off / partly off the map
    if case.group == "partial":
        assert case.C > 16 and all(case.C % d for d in range(2, case.C))    # prime
        assert all(case.C % i for i in set(case.icpw.values()))             # a partly filled workgroup
        assert case.N * case.C > 2 * ppc.MI355X_CUS or case.H * case.W * 4 > ppc.constants().kPlaneBudget


@CASE
def test_case_has_empty_and_full_bins_and_a_first_max_tie(case):
    empty, full = ppc.bin_stats(case)
    print(case.name, "empty", empty, "non-empty", full)
    assert empty > 0 and full >= 0.25 * (empty + full)
    assert ppc.first_max_tie(case) is not None


@pytest.mark.parametrize("case", BWD_CASES, ids=repr)
def test_backward_case_depends_on_summation_order(case):
    n = ppc.order_sensitive_pixels(case)
    print(case.name, "order-sensitive pixels", n)
    assert n >= 1


@pytest.mark.parametrize("case", [c for c in CASES if c.PHW > 64], ids=repr)
def test_bins_case_shares_pixels_across_and_within_chunks(case):
    cross, within = ppc.shared_pixels(case)
    print(case.name, "cross-chunk", cross, "within-chunk", within)
    assert cross >= 1 and within >= 1


def test_invalid_rows_pool_to_nothing():
    case = ppc.BY_NAME["bins_9x9"]
    out, am = ppc.forward_ref(case)
    bad = ~ppc.valid_rows(case)
    assert bad.sum() == 4 and (out[bad] == 0).all() and (am[bad] == -1).all()
    og, oa = ppc.forward_ref(case, grouped=False)
    perm = case.inputs()[2]
    assert np.array_equal(og.view(np.uint32), out[perm].view(np.uint32)) and np.array_equal(oa, am[perm])
