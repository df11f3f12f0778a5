"""Every score-ordering case (tests/score_cases.py) still is the case it claims
to be, asserted on the references alone.  CPU only.

1. The oracle's keep list equals the greedy sweep walked in torch's own stable
   descending order: the oracle's comparator is pinned to real torch.
2. Ordering by raw fp32 bits -- the sign-folded bit pattern as an unsigned
   integer, which is how the kernels ordered scores before NaNs and zeros were
   made canonical -- gives another keep list on the cases that exist for
   signed zeros and sign-set NaNs: those cases can fail.
3. Without NaN, numpy's stable ``argsort(-s)`` (orc.propose_one's ranking) and
   torch's sort agree, so the proposal reference differs from the oracle only
   where the documented deviation (NaN last) applies.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import score_cases as sc  # noqa: E402
from oracle import ref_numpy as orc  # noqa: E402


def raw_bits_order(scores):
    """Ordering by raw fp32 bits: flip every bit of a sign-set pattern, set the
    sign bit of the others (ascending unsigned == ascending finite float), walk
    from the largest down, ties by index.  -0.0 comes after +0.0 and a sign-set
    NaN after -inf."""
    u = sc.bits_of(scores).astype(np.int64)
    asc = np.where(u >= 0x80000000, 0xFFFFFFFF - u, u + 0x80000000)
    desc = np.minimum(0xFFFFFFFF - asc, 0xFFFFFFFE)   # the largest value was kept free
    return np.lexsort((np.arange(len(u)), desc))


def test_table_is_complete():
    assert set(sc.NAMES) == {"signed_zero_pair", "signed_zero_blocks", "zeros_among_finite", "nan_signs", "all_nan",
                             "inf_and_extremes", "wide_stage_edge"}
    assert len(sc.CASES["signed_zero_blocks"][1]) == 130 and len(sc.CASES["all_nan"][1]) == 70
    assert len(sc.CASES["wide_stage_edge"][1]) == 2049
    assert all(len(s) <= 200 for n, (_, s, _) in sc.CASES.items() if n != "wide_stage_edge")
    for name, (b, s, _) in sc.CASES.items():
        assert b.dtype == np.float32 and s.dtype == np.float32 and b.shape == (len(s), 4), name


def test_case_contents():
    u = {n: sc.bits_of(s) for n, (_, s, _) in sc.CASES.items()}
    assert set(u["signed_zero_blocks"]) == {0, 0x80000000}
    # across both 64-candidate block edges a -0.0 precedes a +0.0
    assert u["signed_zero_blocks"][[63, 64, 127, 128, 129]].tolist() == [0x80000000, 0, 0, 0x80000000, 0]
    z = sc.CASES["zeros_among_finite"][1]
    assert {0, 0x80000000} <= set(u["zeros_among_finite"]) and (z > 0).any() and (z < 0).any()
    assert set(sc.NAN_BITS) <= set(u["nan_signs"])
    s = sc.CASES["nan_signs"][1]
    assert np.isposinf(s).any() and np.isneginf(s).any() and np.isfinite(s).any()
    assert np.isnan(sc.CASES["all_nan"][1]).all() and set(u["all_nan"]) == set(sc.NAN_BITS)
    fi = np.finfo(np.float32)
    want = [np.inf, -np.inf, fi.max, -fi.max, fi.tiny, -fi.tiny]
    assert set(sc.bits_of(np.array(want, np.float32))) | {1, 0x80000001} <= set(u["inf_and_extremes"])
    assert set(u["wide_stage_edge"]) == {0, 0x80000000, 0x3f000000, 0xffc00000}


def test_issue_examples():
    b, s, thr = sc.CASES["signed_zero_pair"]
    assert orc.nms(b, s, thr).tolist() == [0, 2]
    assert sc.nms_on_order(b, raw_bits_order(s), thr).tolist() == [1, 2]
    s = np.array([1.0, 0.0, 0.5], np.float32)
    s[1] = sc.from_bits([0xffc00000])[0]
    assert orc.nms(b, s, thr).tolist() == [1, 2]
    assert sc.nms_on_order(b, raw_bits_order(s), thr).tolist() == [0, 2]


@pytest.mark.parametrize("name", sc.NAMES)
def test_oracle_is_torch_order(name):
    b, s, thr = sc.CASES[name]
    keep = sc.reference_keep(name)
    assert np.array_equal(keep, sc.nms_on_order(b, sc.torch_order(s), thr))
    assert 0 < len(keep) < len(s), "the sweep both keeps and suppresses"


@pytest.mark.parametrize("name", sc.NAMES)
def test_raw_bits_order(name):
    b, s, thr = sc.CASES[name]
    raw = sc.nms_on_order(b, raw_bits_order(s), thr)
    assert {"signed_zero_pair", "signed_zero_blocks", "nan_signs", "all_nan", "wide_stage_edge"} <= set(sc.RAW_BITS_DIFFER)
    assert np.array_equal(raw, sc.reference_keep(name)) == (name not in sc.RAW_BITS_DIFFER)


@pytest.mark.parametrize("name", [n for n in sc.NAMES if not np.isnan(sc.CASES[n][1]).any()])
def test_numpy_and_torch_rank_alike_without_nan(name):
    s = sc.CASES[name][1]
    assert np.array_equal(np.argsort(-s, kind="stable"), sc.torch_order(s))


@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_propose_variants(variant):
    anchors, s, de = sc.propose_inputs(variant)
    u = sc.bits_of(s)
    args = (anchors, s, de, sc.IMG_W, sc.IMG_H)
    for pre, post in [(3000, 300), (2049, 4000)]:
        rois, idx = sc.propose_ref(*args, pre, post)
        raw = sc.propose_ref(*args, pre, post, order=raw_bits_order)[1]
        assert 0 < len(idx) <= post
        if variant == "ties_pos_zero":
            assert (u == 0).sum() > 100 and not (u == 0x80000000).any()
            assert len(np.unique(s)) <= 9, "heavy ties"
            orois, oidx = orc.propose_one(*args, pre, post)
            assert np.array_equal(idx, oidx) and np.array_equal(rois, orois)
            assert np.array_equal(raw, idx), "no signed zero, no NaN: raw bits order alike"
        elif variant == "ties_signed_zero":
            assert (u == 0).sum() > 50 and (u == 0x80000000).sum() > 50
            orois, oidx = orc.propose_one(*args, pre, post)
            assert np.array_equal(idx, oidx) and np.array_equal(rois, orois)
        else:
            nan = np.isnan(s)
            assert 40 <= nan.sum() <= 60 and (u[nan] >> 31).any() and not (u[nan] >> 31).all()
            assert np.isnan(s[idx[0]]), "NaN scores rank first"
            assert not np.array_equal(raw, idx), "ordering by raw bits differs"
