"""The named VOC evaluation cases (tests/eval_cases.py) on the HIP path against the numpy
restatement of the contract (tests/eval_ref.py).

Bars, those of test_gpu_eval.py: hdr, rec_key, rec_flag, rec_image, the sorted keys and the
11-point AP (a fixed 11-term order of exactly rounded divisions) are bit-exact.  The area AP is
within n_c * 2^-52 absolute, n_c the class's record count: both sides add the same at most n_c
terms, which sum to at most 1, in different orders, and each addition rounds by at most 2^-53.
map with the area AP: within the largest class's bound.  NaN positions are equal.

Every case first compares ``_lib.eval_plan`` with the plan it carries, and runs twice: into record
arrays filled with zeros and into arrays filled with a sentinel.  The two runs give the same bits,
and nothing at or past hdr[0] is written -- the arrays are views of longer ones, so a write past
the capacity would show too."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import coco_eval_ref  # noqa: E402
import eval_cases as ec  # noqa: E402
import eval_ref  # noqa: E402
from replication_faster_rcnn_amd import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu

U = np.uint64
PAD = 64                                                  # elements behind the capacity that must stay as they were
SENTINEL = {torch.int64: 0x5A5A5A5A5A5A5A5A, torch.int8: 0x5A, torch.int32: 0x5A5A5A5A}
worst = {"diff": 0.0, "bound": 0.0, "case": None}         # the largest area-AP difference seen, and its bound


def make_state(C, cap, sentinel):
    """ops.eval_state's arrays as views of arrays PAD longer, filled with the sentinel or zeros."""
    dev = _lib.device()
    stores = [torch.full((cap + PAD,), SENTINEL[dt] if sentinel else 0, dtype=dt, device=dev)
              for dt in (torch.int64, torch.int8, torch.int32)]
    state = (torch.zeros(4 + C, dtype=torch.int64, device=dev),) + tuple(s[:cap] for s in stores)
    return state, stores


def assert_untouched(stores, n, sentinel):
    for s in stores:
        fill = SENTINEL[s.dtype] if sentinel else 0
        assert bool((s[n:] == fill).all()), "written at or past hdr[0]"


def upload(case):
    out = []
    for b, kw in case.updates:
        t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in eval_ref.args(b)]
        out.append((t, kw))
    return out


def run_updates(state, dev_updates):
    for (db, dl, ds, dc, gb, gl, gd), kw in dev_updates:
        ops.eval_update((db, dl, ds, dc), gb, gl, None if kw.get("no_difficult") else gd, state=state,
                        iou_thresh=kw.get("iou_thresh", 0.5), plus_one=bool(kw.get("plus_one", 1)))


def run_ap(state, n):
    """{use_07: (ap, map, sorted keys)} as device tensors."""
    return {m: ops.eval_ap(state, n, use_07_metric=m, return_sorted=True) for m in (True, False)}


def to_host(out):
    return {m: (ap.cpu().numpy(), float(mean.item()), sk.cpu().numpy().view(np.uint64))
            for m, (ap, mean, sk) in out.items()}


def assert_ap(name, got, want):
    """got: to_host(run_ap(...)); want: {use_07: eval_ref.State.ap(...)}."""
    for use_07 in (True, False):
        ap, mean, sk = got[use_07]
        wap, wmean, wsk, nper = want[use_07]
        assert np.array_equal(sk, wsk), "sorted keys differ"
        assert np.array_equal(np.isnan(ap), np.isnan(wap)), (ap, wap)
        assert np.isnan(mean) == np.isnan(wmean)
        if use_07:
            assert np.array_equal(ap, wap, equal_nan=True), (ap, wap)
            assert mean == wmean or np.isnan(wmean), (mean, wmean)
        else:
            bound = nper * 2.0 ** -52
            diff = np.abs(ap - wap)
            ok = np.isnan(wap) | (diff <= bound)
            if (~np.isnan(diff)).any():
                c = int(np.nanargmax(diff))
                print("%s: largest area AP |diff| %.3g, its bound %.3g" % (name, diff[c], bound[c]))
                if diff[c] > worst["diff"]:
                    worst.update(diff=float(diff[c]), bound=float(bound[c]), case=name)
            assert ok.all(), (ap, wap, bound)
            if not np.isnan(wmean):
                assert abs(mean - wmean) <= bound[~np.isnan(wap)].max(), (mean, wmean)


def same_bits(a, b):
    for m in (True, False):
        for x, y in zip(a[m], b[m]):
            assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)


# ------------------------------------------------------------------- batches
@pytest.mark.parametrize("case", ec.BATCH_CASES, ids=repr)
def test_batch_case(case):
    for shape, p in zip(case.shapes(), case.plans):
        assert _lib.eval_plan(*shape) == p, shape
    ref = case.reference()
    case.check(case, ref)
    n = int(ref.hdr[0])
    want = {m: ref.ap(use_07_metric=m) for m in (True, False)}
    dev = upload(case)
    runs = []
    for sentinel in (False, True):
        state, stores = make_state(case.C, case.cap, sentinel)
        run_updates(state, dev)
        hdr = state[0].cpu().numpy()
        key, flag, image = (s.cpu().numpy() for s in stores)
        assert np.array_equal(hdr, ref.hdr), (hdr, ref.hdr)
        assert np.array_equal(key.view(np.uint64)[:n], ref.rec_key[:n]), "rec_key differs"
        assert np.array_equal(flag[:n], ref.rec_flag[:n]), (flag[:n], ref.rec_flag[:n])
        assert np.array_equal(image[:n], ref.rec_image[:n]), "rec_image differs"
        assert_untouched(stores, n, sentinel)
        got = to_host(run_ap(state, n))
        assert_ap(case.name, got, want)
        assert_untouched(stores, n, sentinel)            # the closing step leaves the state alone
        runs.append((key[:n], flag[:n], image[:n], got))
    for x, y in zip(runs[0][:3], runs[1][:3]):
        assert np.array_equal(x, y)
    same_bits(runs[0][3], runs[1][3])


# -------------------------------------------------------------------- states
def load_state(case, sentinel):
    state, stores = make_state(case.C, case.cap, sentinel)
    ref = case.state()
    state[0].copy_(torch.from_numpy(ref.hdr))
    if case.held:
        state[1][:case.held].copy_(torch.from_numpy(case.keys.view(np.int64)))
        state[2][:case.held].copy_(torch.from_numpy(case.flags))
    return state, stores


@pytest.mark.parametrize("case", ec.STATE_CASES, ids=repr)
def test_state_case(case):
    assert _lib.eval_plan(1, 1, case.n_records) == case.plan
    want = case.reference()
    case.check(case, want)
    runs = []
    for sentinel in (False, True):
        state, stores = load_state(case, sentinel)
        before = [s.clone() for s in stores]
        got = to_host(run_ap(state, case.n_records))
        assert_ap(case.name, got, want)
        assert all(torch.equal(a, b) for a, b in zip(before, stores)), "eval_ap wrote to the state"
        assert_untouched(stores, case.held, sentinel)
        runs.append(got)
    same_bits(runs[0], runs[1])


def test_largest_area_ap_difference():
    """Runs behind the cases above and prints the largest area-AP difference they saw, next to its bound."""
    print("largest area AP |diff| over the named cases: %.3g (bound %.3g, case %s)"
          % (worst["diff"], worst["bound"], worst["case"]))
    assert worst["diff"] <= worst["bound"]


# ---------------------------------------------------- the shared sort entry
def test_coco_evaluator_sorts_the_same_key_sets():
    """eval_coco.hip reaches the same sort through eval_sort_keys: on every sort_* key set, with
    random matched masks and ranks, precision and recall -- which depend on the order of the
    records within a class -- equal the restatement's on np.sort of the keys, bit for bit."""
    for case in ec.SORT_CASES:
        n, C = case.held, case.C
        r = np.random.default_rng(n + C)
        st = coco_eval_ref.State(C, n)
        st.rec_key[:] = case.keys
        st.rec_bits[:, 0] = r.integers(0, 1 << 10, n).astype(U)             # matched at "all", nothing ignored
        st.rec_bits[:, 1] = r.integers(0, 12, n).astype(U) << U(32)         # ranks on both sides of maxDets 1 and 10
        st.hdr[0], st.hdr[1] = n, 1
        st.npig[1:, 0] = n                                                  # tp <= npig; the other ranges have no gt
        want = st.accumulate()
        assert (want["precision"][:, :, 1:, 0, :] > 0).any(), case
        state = ops.coco_eval_state(C, n)
        state[0].copy_(torch.from_numpy(st.hdr))
        state[1].copy_(torch.from_numpy(st.rec_key.view(np.int64)))
        state[2].copy_(torch.from_numpy(st.rec_bits.view(np.int64)))
        precision, recall, _, _ = (t.cpu().numpy() for t in ops.coco_eval_accumulate(state, n))
        assert np.array_equal(precision, want["precision"]), (case, np.argwhere(precision != want["precision"])[:4])
        assert np.array_equal(recall, want["recall"]), case


# ------------------------------------------------------------- no host read
def test_no_host_read_when_n_records_is_given():
    """The whole case set under torch's sync debug mode: with n_records given, neither the updates
    nor the closing step read anything back."""
    batches = [(c, upload(c), make_state(c.C, c.cap, False)[0], c.n_records) for c in ec.BATCH_CASES]
    states = [(c, None, load_state(c, False)[0], c.n_records) for c in ec.STATE_CASES]
    want = {c.name: ({m: c.reference().ap(use_07_metric=m) for m in (True, False)} if dev is not None
                     else c.reference()) for c, dev, _, _ in batches + states}
    torch.cuda.synchronize()
    out = {}
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for c, dev, state, n in batches + states:
            if dev is not None:
                run_updates(state, dev)
            out[c.name] = run_ap(state, n)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for name, got in out.items():
        assert_ap(name, to_host(got), want[name])
