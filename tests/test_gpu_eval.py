"""ops.eval_update / ops.eval_ap / VOCEvaluator against the numpy restatement of
the evaluation contract (tests/eval_ref.py, the devkit's sequential loop).

Bars: hdr, rec_key, rec_flag, rec_image, the sorted keys and the 11-point AP
(a fixed 11-term order of exactly rounded divisions) are bit-exact.  The area AP
is within n_c * 2^-52 absolute, n_c the class's record count: both sides add
the same at most n_c terms, which sum to at most 1, in different orders, and
each addition rounds by at most 2^-53.  map with the area AP: within the
largest class's bound (a mean of the class differences).  NaN positions are
equal.  Each case asserts its precondition on the reference alone."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eval_ref  # noqa: E402
from replication_faster_rcnn_amd import _lib, ops, synth  # noqa: E402
from replication_faster_rcnn_amd.evaluate import VOCEvaluator  # noqa: E402

pytestmark = pytest.mark.gpu

U = np.uint64
_cache = {}


def cases(name):
    """Named batches (a list: one entry per update), generated once, never modified."""
    if name not in _cache:
        mk = eval_ref.make_case
        if name == "mixed":
            c = [mk(3, 64, 8, 5, seed=11)]
        elif name == "voc":
            c = [mk(2, 200, 32, 21, seed=12, max_gt=6)]
        elif name == "shuffled":
            c = [mk(4, 65, 3, 2, seed=13, shuffle=True, counts=[65, 64, 65, 33])]
        elif name == "one":
            c = [mk(1, 1, 1, 2, seed=14, counts=[1])]
        elif name == "one_empty":
            c = [mk(1, 1, 1, 2, seed=14, counts=[0])]
        elif name == "g0":
            c = [mk(2, 20, 0, 3, seed=15)]
        elif name == "g256":
            c = [mk(2, 300, 256, 5, seed=16, counts=[300, 280])]
        elif name == "clamped":
            c = [mk(3, 40, 6, 4, seed=17, counts=[-3, 45, 20])]
        elif name == "chunks":
            c = [mk(1, 2500, 16, 3, seed=18, counts=[2500], max_gt=4)]
        elif name == "sort":
            kw = dict(seed=19, levels=2, gt_classes=(3, 7, 12))
            c = [mk(8, 300, 8, 21, counts=[300] * 8, **kw), mk(16, 300, 8, 21, first_image=8, counts=[300] * 16, **kw),
                 mk(16, 300, 8, 21, first_image=24, counts=[300] * 16, **kw),
                 mk(1, 300, 8, 21, first_image=40, counts=[37], **kw)]
        elif name == "batches":
            c = [mk(2, 64, 8, 5, seed=20), mk(3, 64, 8, 5, seed=20, first_image=2),
                 mk(1, 64, 8, 5, seed=20, first_image=5)]
        _cache[name] = c
    return _cache[name]


def reference(name, C, cap=None, plus_one=1):
    key = ("ref", name, C, cap, plus_one)
    if key not in _cache:
        cs = cases(name)
        st = eval_ref.State(C, cap or sum(c["det_labels"].size for c in cs))
        for c in cs:
            st.update(*eval_ref.args(c), plus_one=plus_one)
        _cache[key] = st
    return _cache[key]


def to_dev(case):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in eval_ref.args(case)]


def update(state, case, **kw):
    db, dl, ds, dc, gb, gl, gd = to_dev(case)
    ops.eval_update((db, dl, ds, dc), gb, gl, gd, state=state, **kw)


def host(state):
    hdr, key, flag, image = (t.cpu().numpy() for t in state)
    return hdr, key.view(np.uint64), flag, image


def assert_state(state, ref):
    hdr, key, flag, image = host(state)
    assert np.array_equal(hdr, ref.hdr), (hdr, ref.hdr)
    n = int(ref.hdr[0])
    assert np.array_equal(key[:n], ref.rec_key[:n]), "rec_key differs"
    assert np.array_equal(flag[:n], ref.rec_flag[:n]), "rec_flag differs"
    assert np.array_equal(image[:n], ref.rec_image[:n]), "rec_image differs"


def assert_ap(state, ref):
    n = int(ref.hdr[0])
    out = {}
    for use_07 in (True, False):
        ap, mean, sk = ops.eval_ap(state, n, use_07_metric=use_07, return_sorted=True)
        ap, mean, sk = ap.cpu().numpy(), float(mean.item()), sk.cpu().numpy().view(np.uint64)
        wap, wmean, wsk, nper = ref.ap(use_07_metric=use_07)
        assert np.array_equal(sk, wsk), "sorted keys differ"
        assert np.array_equal(np.isnan(ap), np.isnan(wap)), (ap, wap)
        assert np.isnan(mean) == np.isnan(wmean)
        if use_07:
            assert np.array_equal(ap, wap, equal_nan=True), (ap, wap)
            assert mean == wmean or np.isnan(wmean), (mean, wmean)
        else:
            bound = nper * 2.0 ** -52
            diff = np.abs(ap - wap)
            print("area AP |diff| / bound per class:", [(float(d), float(b)) for d, b in zip(diff, bound) if d == d])
            ok = np.isnan(wap) | (diff <= bound)
            assert ok.all(), (ap, wap, bound)
            if not np.isnan(wmean):
                assert abs(mean - wmean) <= bound[~np.isnan(wap)].max(), (mean, wmean)
        out[use_07] = (ap, mean)
    return out


def run(name, C, plus_one=1, cap=None):
    ref = reference(name, C, cap, plus_one)
    state = ops.eval_state(C, ref.cap)
    for c in cases(name):
        update(state, c, plus_one=bool(plus_one))
    assert_state(state, ref)
    assert_ap(state, ref)
    return state, ref


def records(name, ref):
    """(case index, image, slot, flag, matched gt) rows of the reference's records."""
    rows, i, pos = [], 0, 0
    for ci, c in enumerate(cases(name)):
        for n in range(len(c["det_count"])):
            best = ref.best[i]
            for s in range(len(best)):
                rows.append((ci, n, s, int(ref.rec_flag[pos]), int(best[s])))
                pos += 1
            i += 1
    assert pos == ref.hdr[0]
    return rows


def claimants(name, ref):
    """(case, image, gt) -> [(slot, score)] of the detections matched to a non-difficult gt."""
    out = {}
    for ci, n, s, flag, j in records(name, ref):
        c = cases(name)[ci]
        if j >= 0 and not c["gt_difficult"][n, j]:
            out.setdefault((ci, n, j), []).append((s, float(c["det_scores"][n, s])))
    return out


def test_mixed():
    ref = reference("mixed", 5)
    flags = ref.rec_flag[:ref.hdr[0]]
    cl = claimants("mixed", ref)
    assert (flags == 1).sum() >= 1 and (flags == -1).sum() >= 1
    assert any(len(v) > 1 for v in cl.values())                                       # an over-threshold FP on a claimed gt
    assert any(len({sc for _, sc in v}) < len(v) for v in cl.values())                # a score tie between two claimants
    print("mixed: TP / FP / ignored", (flags == 1).sum(), (flags == 0).sum(), (flags == -1).sum())
    run("mixed", 5)


def test_mixed_without_plus_one():
    run("mixed", 5, plus_one=0)


def test_voc():
    ref = reference("voc", 21)
    npos = ref.hdr[5:]
    assert (npos == 0).any() and (npos > 0).any()
    run("voc", 21)


def test_shuffled():
    ref = reference("shuffled", 2)
    cl = claimants("shuffled", ref)
    # a gt whose first claimant by score is not its first claimant by slot
    assert any(min(v, key=lambda t: (-t[1], t[0]))[0] != min(s for s, _ in v) for v in cl.values())
    run("shuffled", 2)


@pytest.mark.parametrize("name,nrec", [("one", 1), ("one_empty", 0)])
def test_one(name, nrec):
    ref = reference(name, 2)
    assert ref.hdr[0] == nrec and ref.hdr[1] == 1
    run(name, 2)


def test_no_gt_slots():
    ref = reference("g0", 3)
    assert ref.hdr[0] > 0 and (ref.rec_flag[:ref.hdr[0]] == 0).all() and ref.hdr[4:].sum() == 0
    state, _ = run("g0", 3)
    ap, mean = ops.eval_ap(state)                        # n_records read from the device
    assert np.isnan(ap.cpu().numpy()).all() and np.isnan(mean.item())


def test_256_gt_slots():
    ref = reference("g256", 5)
    assert (cases("g256")[0]["gt_labels"] >= 1).sum(axis=1).max() > 128 and (ref.rec_flag[:ref.hdr[0]] == 1).sum() > 0
    run("g256", 5)


def test_clamped_counts():
    ref = reference("clamped", 4)
    assert cases("clamped")[0]["det_count"].tolist() == [-3, 45, 20] and ref.hdr[0] == 0 + 40 + 20
    run("clamped", 4)


@pytest.mark.parametrize("name", sorted(eval_ref.known_answers()))
def test_known_answers(name):
    case, C, plus_one, flags = eval_ref.known_answers()[name]
    ref = eval_ref.State(C, 16)
    ref.update(*eval_ref.args(case), plus_one=plus_one)
    assert ref.rec_flag[:len(flags)].tolist() == flags
    state = ops.eval_state(C, 16)
    update(state, case, plus_one=bool(plus_one))
    assert_state(state, ref)
    assert host(state)[2][:len(flags)].tolist() == flags
    got = assert_ap(state, ref)
    if name == "tp_fp_tp_fp":
        assert abs(got[False][0][1] - 5.0 / 6.0) <= 4 * 2.0 ** -52 and np.isnan(got[False][0][2])
        assert abs(got[True][0][1] - 28.0 / 33.0) <= 11 * 2.0 ** -53


def test_chunks():
    ref = reference("chunks", 3)
    cl = claimants("chunks", ref)
    assert any(len({s // 256 for s, _ in v}) > 1 for v in cl.values())   # claimants of one gt in different chunks
    run("chunks", 3)


def test_sort():
    ref = reference("sort", 21)
    n = int(ref.hdr[0])
    assert n == 40 * 300 + 37 >= 10000 and ref.hdr[1] == 41
    _, counts = np.unique(ref.rec_key[:n] >> U(24), return_counts=True)
    assert counts.max() > 1000                           # more than a thousand records share one (class, score)
    run("sort", 21)


def test_sort_many_tiles():
    """The closing step alone on a state written by hand: 100,003 records (two dozen sort
    tiles, the last one ragged) of 20 classes and 8 score values, so every (class, score)
    group spans several tiles."""
    C, n = 21, 100003
    r = synth.rng_for(22, 0, 7)
    ref = eval_ref.State(C, n)
    score = (r.integers(0, 8, n) / 8.0).astype(np.float32)
    ref.rec_key[:] = (r.integers(1, C, n).astype(U) << U(56)) | (eval_ref.desc_score_key(score).astype(U) << U(24)) | \
        np.arange(n, dtype=U)
    ref.rec_flag[:] = r.integers(-1, 2, n)
    ref.hdr[0], ref.hdr[1] = n, 1
    ref.hdr[5:] = r.integers(0, 3, C - 1) * 40000        # some classes without positives; tp <= npos is not needed
    _, counts = np.unique(ref.rec_key >> U(24), return_counts=True)
    assert counts.min() > 256 and (ref.hdr[5:] == 0).any() and (ref.hdr[5:] > 0).any()
    state = ops.eval_state(C, n)
    state[0].copy_(torch.from_numpy(ref.hdr))
    state[1].copy_(torch.from_numpy(ref.rec_key.view(np.int64)))
    state[2].copy_(torch.from_numpy(ref.rec_flag))
    assert_ap(state, ref)


def test_batching():
    """Three updates equal one update of the concatenated batch, bit for bit."""
    parts = cases("batches")
    ref = reference("batches", 5)
    whole = eval_ref.State(5, ref.cap)
    whole.update(*eval_ref.args(eval_ref.concat(parts)))
    assert np.array_equal(whole.hdr, ref.hdr) and np.array_equal(whole.rec_key, ref.rec_key)
    a, _ = run("batches", 5)
    b = ops.eval_state(5, ref.cap)
    update(b, eval_ref.concat(parts))
    n = int(ref.hdr[0])
    ha, hb = host(a), host(b)
    assert np.array_equal(ha[0], hb[0])
    for x, y in zip(ha[1:], hb[1:]):
        assert np.array_equal(x[:n], y[:n])
    for use_07 in (True, False):
        pa = ops.eval_ap(a, n, use_07_metric=use_07, return_sorted=True)
        pb = ops.eval_ap(b, n, use_07_metric=use_07, return_sorted=True)
        for x, y in zip(pa, pb):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True)


def test_overflow():
    b1, b2, b3 = cases("batches")
    k1, k2 = (int(np.clip(b["det_count"], 0, 64).sum()) for b in (b1, b2))
    cap = k1 + k2 - 1                                    # one short of the second batch
    ref = eval_ref.State(5, cap)
    for b in (b1, b2, b3):
        ref.update(*eval_ref.args(b))
    without = eval_ref.State(5, cap)
    without.update(*eval_ref.args(b1))
    without.update(*eval_ref.args(b3))
    assert ref.hdr[2] == 1 and ref.hdr[0] == without.hdr[0] > k1 and np.array_equal(ref.hdr[4:], without.hdr[4:])
    ev = VOCEvaluator(n_class=5, capacity=cap)
    for b in (b1, b2, b3):
        ev.update(to_dev(b)[:4], *to_dev(b)[4:])
    assert_state(ev.state, ref)
    hdr = host(ev.state)[0]
    assert hdr[2] == 1 and np.array_equal(np.delete(hdr, 2), np.delete(without.hdr, 2))
    with pytest.raises(_lib.FrcnnError, match="dropped"):
        ev.result()
    ev.reset()
    assert (host(ev.state)[0] == 0).all()
    ev.update(to_dev(b1)[:4], *to_dev(b1)[4:])
    assert ev.result()["n_records"] == k1


def _detect_case():
    """ops.detect's output on synthetic head outputs, with gt from synth.gt_boxes
    plus boxes copied from the detections (one of them difficult)."""
    if "detect" not in _cache:
        H, W, C = 600, 1000, 5
        dev = [torch.from_numpy(a).cuda() for a in synth.head_outputs(2, 77, C, H, W, seed=21)]
        det = ops.detect(*dev, img_h=H, img_w=W, score_thresh=0.05)
        boxes, labels, _, _, count, _ = (t.cpu().numpy() for t in det)
        G = 8
        gb, gl, gd = -np.ones((2, G, 4)), -np.ones((2, G)), np.zeros((2, G), np.uint8)
        for n in range(2):
            b, l = synth.gt_boxes(H, W, 3, 21, n)        # labels in 1..20: those >= C are no gt here
            gb[n, :3], gl[n, :3] = b, l
            picks = [s for s in (0, 5, 10, 15) if s < count[n]]
            for i, s in enumerate(picks):
                gb[n, 4 + i], gl[n, 4 + i] = boxes[n, s].astype(np.float64), labels[n, s]
            gd[n, 5] = 1
        _cache["detect"] = (det, gb, gl, gd, C)
    return _cache["detect"]


def _detect_reference(det, gb, gl, gd, C, cap):
    ref = eval_ref.State(C, cap)
    db, dl, ds, _, dc, _ = (t.cpu().numpy() for t in det)
    ref.update(db, dl, ds, dc, gb, gl.astype(np.int32), gd)
    return ref


def test_voc_evaluator_from_detect():
    det, gb, gl, gd, C = _detect_case()
    ref = _detect_reference(det, gb, gl, gd, C, 4096)
    n = int(ref.hdr[0])
    assert (ref.rec_flag[:n] == 1).sum() >= 1 and ref.hdr[4:].sum() >= 2
    for use_07 in (False, True):
        ev = VOCEvaluator(n_class=C, capacity=4096, use_07_metric=use_07)
        gt = [torch.from_numpy(a).cuda() for a in (gb, gl, gd)]
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")         # update on device inputs contains no host read
        try:
            ev.update(det, *gt)
        finally:
            torch.cuda.set_sync_debug_mode(prev)
        assert_state(ev.state, ref)
        assert_ap(ev.state, ref)
        res = ev.result()
        wap, wmean, _, nper = ref.ap(use_07_metric=use_07)
        assert res["n_records"] == n and res["n_images"] == 2 and np.array_equal(res["npos"], ref.hdr[4:])
        assert res["ap"].shape == (C,) and np.array_equal(np.isnan(res["ap"]), np.isnan(wap))
        assert (np.isnan(wap) | (np.abs(res["ap"] - wap) <= (0 if use_07 else 1) * nper * 2.0 ** -52)).all()
        assert abs(res["map"] - wmean) <= (0 if use_07 else nper.max() * 2.0 ** -52)


def test_fp64_labels_and_numpy_inputs():
    det, gb, gl, gd, C = _detect_case()
    ref = _detect_reference(det, gb, gl, gd, C, 4096)
    assert gl.dtype == np.float64 and (gl == -1).any()
    ev = VOCEvaluator(n_class=C, capacity=4096)
    ev.update(tuple(t.cpu().numpy() for t in det), gb, gl, gd)
    assert_state(ev.state, ref)
    ev2 = VOCEvaluator(n_class=C, capacity=4096)         # CPU tensors, the 4-tuple, no difficult flags
    ev2.update(tuple(det[i].cpu() for i in (0, 1, 2, 4)), torch.from_numpy(gb), torch.from_numpy(gl))
    ref2 = eval_ref.State(C, 4096)
    db, dl, ds, _, dc, _ = (t.cpu().numpy() for t in det)
    ref2.update(db, dl, ds, dc, gb, gl.astype(np.int32), None)
    assert_state(ev2.state, ref2)
    assert ref2.hdr[4:].sum() > ref.hdr[4:].sum()


def test_errors():
    case = cases("mixed")[0]
    db, dl, ds, dc, gb, gl, gd = to_dev(case)
    state = ops.eval_state(5, 1000)
    with pytest.raises(RuntimeError):
        ops.eval_update((db, dl.long(), ds, dc), gb, gl, gd, state=state)
    with pytest.raises(RuntimeError):
        ops.eval_update((db, dl, ds, dc), gb.float(), gl, gd, state=state)
    with pytest.raises(RuntimeError):
        ops.eval_update((db, dl, ds, dc), gb, gl[:, :-1].contiguous(), gd, state=state)
    with pytest.raises(RuntimeError):
        ops.eval_update((db, dl, ds, dc), gb, gl, gd, state=state[:3])
    with pytest.raises(RuntimeError):
        ops.eval_state(1, 100)
    with pytest.raises(RuntimeError):
        ops.eval_state(5, (1 << 24) + 1)
    with pytest.raises(RuntimeError):
        ops.eval_ap(state, 1001)
    assert (host(state)[0] == 0).all()
