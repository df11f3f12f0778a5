"""Every target-assignment edge case (tests/target_cases.py) still is the case
it claims to be: its precondition, asserted on the oracle alone.  CPU only."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import target_cases as tc  # noqa: E402


@pytest.mark.parametrize("name", [c.name for c in tc.ALL_CASES])
def test_case_precondition(name, rng_guard):
    case = tc.BY_NAME[name]
    before = np.random.get_state()
    out = tc.oracle(case)
    assert len(out["images"]) == len(case.boxes)
    case.check(case, out)
    after = np.random.get_state()
    assert before[2] == after[2] and np.array_equal(before[1], after[1]), "the oracle run restores the global RNG"


def test_case_table_is_complete():
    names = {c.name.split("-")[0] for c in tc.ANCHOR_CASES}
    assert names == {"dup_anchor_ties", "dup_gt", "no_overlap", "thr_equal", "pad_interleaved", "g_sizes",
                     "a_sizes", "nonfinite", "sampling"}
    assert {c.name.split("-")[0] for c in tc.PROPOSAL_CASES} == {"t_edges", "dup_gt_labels", "thresholds", "rounding"}
    assert sum(c.name.startswith("sampling") for c in tc.ANCHOR_CASES) == 8
    assert sum(c.name.startswith("a_sizes") for c in tc.ANCHOR_CASES) == 11
    assert sum(c.name.startswith("g_sizes") for c in tc.ANCHOR_CASES) == 6
    assert sum(c.name.startswith("rounding") for c in tc.PROPOSAL_CASES) == 7
