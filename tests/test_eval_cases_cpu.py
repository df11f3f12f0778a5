"""The named VOC evaluation cases (tests/eval_cases.py) on the CPU: every case's check holds on
the numpy restatement (tests/eval_ref.py), the port of the plan query equals ``frcnn_eval_plan``,
the query refuses bad arguments, every planted mistake is told apart by the case named for it, and
on every batch case the devkit's sequential loop equals the minimum-claim-key form the kernel uses."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eval_cases as ec  # noqa: E402
import eval_ref  # noqa: E402
from replication_faster_rcnn_amd import _lib  # noqa: E402

U = np.uint64


@pytest.mark.parametrize("case", ec.BATCH_CASES + ec.STATE_CASES, ids=repr)
def test_check_holds_on_the_reference(case):
    case.check(case, case.reference())


def test_case_names_are_unique_and_cover_the_list():
    names = [c.name for c in ec.BATCH_CASES + ec.STATE_CASES]
    assert len(set(names)) == len(names)
    want = ["images_257", "images_1024", "slots_255", "slots_256", "slots_257", "slots_513", "scores_special",
            "best_gt_tie_first", "difficult", "difficult_null", "thresholds", "plus_one_widens", "labels_at_limits",
            "classes_128", "gt_256_last_wins", "exact_fit_then_drop"]
    want += ["sort_n_%d" % n for n in (1, 255, 256, 257, 4095, 4096, 4097, 8192, 8193)]
    want += ["sort_tiles_4", "sort_tiles_5", "sort_one_digit"] + ["sort_byte_%d" % p for p in range(5)]
    want += ["segment_0", "segment_1_tp", "segment_1_fp", "segment_255", "segment_256", "segment_257", "segment_513",
             "segment_257_tp255", "segment_257_tp256", "segment_513_tp255", "segment_513_tp256", "segment_all_ignored",
             "segment_ignored_first", "segment_across_tile", "class_zero_ahead", "classes_mixed", "all_nan",
             "recall_at_tenths", "n_below_held"]
    assert not set(want) - set(names), set(want) - set(names)
    ec.check_scan_shares(ec.STATE_CASES)
    assert all(c.held <= 5 * ec.TILE for c in ec.STATE_CASES)           # every state is tiny
    assert all(b["det_labels"].size <= ec.MAX_N for c in ec.BATCH_CASES for b, _ in c.updates)


# ------------------------------------------------------------------ the plan
def test_plan_port_equals_the_query():
    assert tuple(_lib.EVAL_PLAN_FIELDS) == ec.PLAN_FIELDS
    Ns = (1, 2, 255, 256, 257, 511, 512, 513, 1023, ec.MAX_N)
    Ms = (1, 255, 256, 257, 513, 4096, ec.MAX_M - 1, ec.MAX_M)
    ns = (0, 1, 255, 256, 257, 4095, 4096, 4097, 8192, 8193, 3 * 4096 + 1, 4 * 4096, 4 * 4096 + 1, 100003,
          ec.MAX_CAP - 1, ec.MAX_CAP)
    for N in Ns:
        for M in Ms:
            for n in ns:
                assert _lib.eval_plan(N, M, n) == ec.plan(N, M, n), (N, M, n)
    for c in ec.BATCH_CASES:
        for shape, p in zip(c.shapes(), c.plans):
            assert _lib.eval_plan(*shape) == p, (c, shape)
    for c in ec.STATE_CASES:
        assert _lib.eval_plan(1, 1, c.n_records) == c.plan, c
    # the workspace holds what the plan says the scan covers, next to the two key buffers
    lib = _lib.load(require_gpu=False)
    for n in (1, 4096, 4097, 100003):
        assert lib.frcnn_eval_ap_workspace_size(21, n) >= 2 * 8 * n + 4 * ec.plan(1, 1, n)["scan_len"]


def test_plan_query_refuses_bad_arguments():
    lib = _lib.load(require_gpu=False)
    buf = (ctypes.c_int64 * 10)(*([-7] * 10))
    for (N, M, n), word in [((0, 1, 1), b"N="), ((ec.MAX_N + 1, 1, 1), b"N="), ((-1, 1, 1), b"N="),
                            ((1, 0, 1), b"M="), ((1, ec.MAX_M + 1, 1), b"M="), ((1, 1, -1), b"n_records"),
                            ((1, 1, ec.MAX_CAP + 1), b"n_records")]:
        assert lib.frcnn_eval_plan(N, M, n, buf) == -1, (N, M, n)
        assert word in lib.frcnn_last_error() and b"frcnn_eval_plan" in lib.frcnn_last_error()
        assert list(buf) == [-7] * 10                    # nothing is written on an error
    assert lib.frcnn_eval_plan(1, 1, 1, None) == -1 and b"plan" in lib.frcnn_last_error()
    with pytest.raises(_lib.FrcnnError, match="N="):
        _lib.eval_plan(0, 1, 1)
    assert lib.frcnn_eval_plan(ec.MAX_N, ec.MAX_M, ec.MAX_CAP, buf) == 0 and list(buf) == \
        [ec.plan(ec.MAX_N, ec.MAX_M, ec.MAX_CAP)[k] for k in ec.PLAN_FIELDS]


# -------------------------------------------------------------- the mistakes
def test_every_mistake_has_a_named_case():
    assert set(ec.CAUGHT_BY) == set(eval_ref.MISTAKES)
    assert set(ec.CAUGHT_BY.values()) <= set(ec.BY_NAME)


@pytest.mark.parametrize("mistake", sorted(ec.CAUGHT_BY))
def test_mistake_is_told_apart_by_its_case(mistake):
    case = ec.BY_NAME[ec.CAUGHT_BY[mistake]]
    assert ec.tells_apart(case, mistake), (mistake, case)
    assert not ec.tells_apart(case, None)
    caught = [c.name for c in ec.BATCH_CASES + ec.STATE_CASES if ec.tells_apart(c, mistake)]
    print(mistake, "is told apart by", caught)


def test_walk_direction_of_the_envelope_mistakes():
    """The kernel walks a segment from its last record, so its chunks are counted from there.  A
    257-record segment's far chunk is record 0 alone, whose envelope only an FP can miss: the
    from-the-end mistake shows first at 513 records, with a TP ahead of the last two chunks."""
    m = "envelope_restarts_each_chunk_from_end"
    assert not any(ec.tells_apart(c, m) for c in ec.STATE_CASES if c.held <= ec.CHUNK + 1)
    assert ec.tells_apart(ec.BY_NAME["segment_513_early_tp"], m)
    assert ec.tells_apart(ec.BY_NAME["segment_513_early_tp"], "running_sum_restarts_each_chunk")
    for name in ("segment_257_tp256", "segment_513_tp256"):    # the lone TP just behind a restart
        assert ec.tells_apart(ec.BY_NAME[name], "running_sum_restarts_each_chunk"), name
    for name in ("segment_257_early_tp", "segment_513_tp255", "segment_513_tp256", "segment_513_early_tp"):
        assert ec.tells_apart(ec.BY_NAME[name], "running_sum_restarts_each_chunk_from_end"), name


# ------------------------------------------- sequential loop == minimum claim key
@pytest.mark.parametrize("case", ec.BATCH_CASES, ids=repr)
def test_sequential_loop_equals_minimum_claim_key(case):
    """The devkit loop (eval_ref) against the parallel form the kernel uses: a gt's TP is the
    claimant with the smallest (desc_score_key << 32 | slot)."""
    st = case.reference()
    held, pos, img = 0, 0, 0
    for (b, kw), (N, M, after) in zip(case.updates, case.shapes()):
        ks = np.clip(b["det_count"], 0, M)
        if after == held and ks.sum() > 0:
            continue                                     # a dropped batch: no record, no entry in st.best
        held = after
        for n in range(N):
            k = int(ks[n])
            best, flag = st.best[img], st.rec_flag[pos:pos + k]
            lab = b["det_labels"][n, :k]
            valid = (lab >= 1) & (lab < case.C)
            key = (eval_ref.desc_score_key(b["det_scores"][n, :k]).astype(U) << U(32)) | np.arange(k, dtype=U)
            want = np.where(valid, 0, -1).astype(np.int8)
            for j in range(b["gt_labels"].shape[1]):
                cl = np.nonzero(best == j)[0]
                if len(cl) == 0:
                    continue
                if b["gt_difficult"][n, j] and not kw.get("no_difficult"):
                    want[cl] = -1
                else:
                    want[cl[np.argmin(key[cl])]] = 1
            assert np.array_equal(flag, want), (case, n)
            pos, img = pos + k, img + 1
    assert pos == st.hdr[0] and img == len(st.best)
