"""Named cases of the fused training losses (DESIGN.md "Losses"): sizes at the
kernels' wave / workgroup / tile edges, both label dtypes, the smooth-L1
threshold to the ulp, labels at the ends of and outside the class range,
extreme logits and garbage in unlabelled rows.  Plain numpy, no GPU.

Every case carries its inputs in the ops' shapes (cls [N, L, C], reg [N, L, 4]
or [N, L, 4C] for a head case, reg_t fp64 [N, L, 4], labels int32 / fp64
[N, L]) and a ``check(case, ref)`` that asserts the case's precondition on
``loss_ref.stage``'s output alone, so a change to a generator cannot silently
turn a case into an easy one.  Users: tests/test_loss_cpu.py (loss_ref against
the reference formulas run by torch in fp64) and tests/test_gpu_losses.py (the
HIP path against loss_ref).

Two properties the torch comparison relies on, kept by the generators:
random logits are N(0, 2^2), so no softmax term rounds to exactly 0 or 1 in
fp32 while it does not in fp64; the extreme rows keep a spread of at most 80
(or so large that fp64 underflows too) for the same reason.
"""
from __future__ import annotations

import numpy as np

import loss_ref

F32 = np.float32


class LossCase:
    """clean: for a case with garbage in its unlabelled rows, the same case
    without it (the outputs must be those of the clean inputs)."""

    def __init__(self, name, cls, reg, reg_t, labels, check, sigma=1.0, head=False, clean=None):
        self.name, self.cls, self.reg, self.reg_t, self.labels = name, cls, reg, reg_t, labels
        self.check, self.sigma, self.head, self.clean = check, sigma, head, clean
        N, L, C = cls.shape
        assert cls.dtype == F32 and reg.dtype == F32 and reg_t.dtype == np.float64
        assert labels.dtype in (np.int32, np.float64) and labels.shape == (N, L)
        assert reg.shape == (N, L, 4 * C if head else 4) and reg_t.shape == (N, L, 4)

    @property
    def C(self):
        return self.cls.shape[2]

    @property
    def rows(self):
        return self.cls.shape[0] * self.cls.shape[1]

    def flat(self):
        """The stage's inputs as the kernels see them: (cls [rows, C], reg, reg_t, labels [rows])."""
        r = self.rows
        return (self.cls.reshape(r, self.C), self.reg.reshape(r, self.reg.shape[2]), self.reg_t.reshape(r, 4),
                self.labels.reshape(r))


_cache = {}


def reference(case, g_cls=1.0, g_reg=1.0):
    """loss_ref.stage on the case (on its clean inputs where it has them), computed once."""
    key = (case.name, g_cls, g_reg)
    if key not in _cache:
        src = case.clean if case.clean is not None else case
        _cache[key] = loss_ref.stage(*src.flat(), sigma=src.sigma, head=src.head, g_cls=g_cls, g_reg=g_reg)
    return _cache[key]


# ------------------------------------------------------------------ generators
def _random(name, N, L, C, head, seed, lab_dtype, n_labelled=None, n_pos=None, sigma=1.0, check=None):
    """Random stage: logits N(0, 2^2), predictions N(0, 1), targets = prediction +
    N(0, 1.5^2) as genuine doubles, n_labelled rows labelled of which n_pos positive."""
    r = np.random.RandomState(seed)
    rows = N * L
    cls = (r.randn(rows, C) * 2).astype(F32)
    reg = r.randn(rows, 4 * C if head else 4).astype(F32)
    reg_t = r.randn(rows, 4) * 1.5 + (reg[:, :4].astype(np.float64) if not head else 0.0)
    n_labelled = rows if n_labelled is None else n_labelled
    n_pos = (n_labelled + 1) // 2 if n_pos is None else n_pos
    lab = np.full(rows, -1, np.int64)
    sel = r.permutation(rows)[:n_labelled]
    lab[sel[:n_pos]] = r.randint(1, C, n_pos)
    lab[sel[n_pos:]] = 0
    if head:  # put the targets near the label's own columns, so both branches occur
        for i in np.nonzero(lab > 0)[0]:
            reg_t[i] += reg[i, 4 * lab[i]:4 * lab[i] + 4]
    want = (n_labelled, n_pos, 0)

    def chk(case, ref, want=want, extra=check):
        assert tuple(ref["stats"][:3]) == want, (case.name, ref["stats"])
        if extra:
            extra(case, ref)

    return LossCase(name, cls.reshape(N, L, C), reg.reshape(N, L, -1), reg_t.reshape(N, L, 4),
                    lab.astype(lab_dtype).reshape(N, L), chk, sigma=sigma, head=head)


def _both_branches(case, ref):
    src = case.clean if case.clean is not None else case
    cls, reg, reg_t, lab = src.flat()
    lab = loss_ref.classify_labels(lab, src.C)
    pos = np.nonzero(lab > 0)[0]
    col = (lab[pos] * 4 if src.head else 0 * pos)[:, None] + np.arange(4)
    d = np.abs(reg[pos[:, None], col] - reg_t[pos].astype(F32))
    inv = loss_ref.sigma_consts(src.sigma)[1]
    assert (d < inv).any() and (d >= inv).any(), case.name


def _nan_loss(case, ref):
    assert np.isnan(ref["loss"][0]) and ref["loss"][1] == 0
    assert not ref["dcls"].any() and not ref["dreg"].any()


def _no_positives(case, ref):
    assert ref["loss"][1] == 0 and not ref["dreg"].any() and ref["dcls"].any() and np.isfinite(ref["loss"][0])


def _one_positive(case, ref):
    assert np.count_nonzero(ref["dreg"]) == 4 and ref["dreg"].any(axis=1).sum() == 1


def _threshold_case(name, sigma):
    """One positive row per d in {0, 1/sigma^2 - ulp, 1/sigma^2, 1/sigma^2 + ulp} and sign:
    t = 0, so x - t is exact and d is the chosen value to the bit."""
    inv = loss_ref.sigma_consts(sigma)[1]
    ds = [F32(0.0), np.nextafter(inv, F32(0)), inv, np.nextafter(inv, F32(2))]
    xs = np.array([[d, -d, d, -d] for d in ds] + [[ds[0], ds[1], ds[2], ds[3]], [-ds[3], -ds[2], -ds[1], -ds[0]]], F32)
    rows = len(xs)
    r = np.random.RandomState(11)
    cls = (r.randn(1, rows, 2) * 2).astype(F32)
    lab = np.ones((1, rows), np.int32)

    def chk(case, ref, inv=inv, xs=xs):
        s2 = loss_ref.sigma_consts(case.sigma)[0]
        g = ref["dreg"] * F32(rows)                      # g_reg = 1, n_pos = rows
        assert ref["stats"][1] == rows
        below = np.abs(xs) < inv
        assert below.sum() == 12 and (np.abs(xs) == inv).sum() == 6 and (xs == 0).sum() == 6
        np.testing.assert_allclose(g[~below], np.sign(xs[~below]), rtol=3e-7, atol=0)   # linear from 1/sigma^2 on
        np.testing.assert_allclose(g[below], s2 * xs[below], rtol=3e-7, atol=0)
        assert (ref["dreg"][xs == 0] == 0).all()

    return LossCase(name, cls, xs.reshape(1, rows, 4), np.zeros((1, rows, 4)), lab, chk, sigma=sigma)


def _head_label_ends(name, C):
    """Head rows with label 0 (cross-entropy only) and C-1 (the last four columns)."""
    base = _random(name, 3, 5, C, True, 21 + C, np.float64)
    lab = base.labels.reshape(-1).copy()
    lab[:] = -1.0
    lab[[0, 4, 9]] = 0.0
    lab[[2, 7, 14]] = float(C - 1)
    lab[5] = 1.0

    def chk(case, ref):
        assert tuple(ref["stats"][:3]) == (7, 4, 0)
        nz = np.nonzero(ref["dreg"].reshape(15, C, 4).any(axis=2))
        assert sorted(zip(*nz)) == [(2, C - 1), (5, 1), (7, C - 1), (14, C - 1)]
        assert not ref["dreg"][[0, 4, 9]].any() and ref["dcls"][[0, 4, 9]].any(axis=1).all()

    return LossCase(name, base.cls, base.reg, base.reg_t, lab.reshape(3, 5), chk, head=True)


def _out_of_range(name, head, lab_dtype):
    C = 5 if head else 2
    base = _random(name, 2, 20, C, head, 31, lab_dtype)
    lab = base.labels.reshape(-1).copy()
    bad = [-2, C, C + 7, -100] if lab_dtype == np.int32 else [-2.0, float(C), np.nan, 1e300, -np.inf, -2.5]
    lab[1:1 + len(bad)] = bad
    n_bad = len(bad)

    def chk(case, ref):
        assert ref["stats"][2] == n_bad and ref["stats"][0] == case.rows - n_bad
        assert not ref["dcls"][1:1 + n_bad].any() and not ref["dreg"][1:1 + n_bad].any()
        assert np.isfinite(ref["loss"]).all()

    return LossCase(name, base.cls, base.reg, base.reg_t, lab.reshape(2, 20), chk, head=head)


def _truncating_labels():
    """fp64 labels that are not integers truncate toward zero: -0.5 -> 0, -1.5 -> -1, 2.7 -> 2."""
    base = _random("f64_labels_truncate", 1, 6, 4, True, 41, np.float64)
    lab = np.array([[-0.5, -1.5, 2.7, 3.999, 0.3, -1.0]])

    def chk(case, ref):
        assert tuple(ref["stats"][:3]) == (4, 2, 0)
        nz = np.nonzero(ref["dreg"].reshape(6, 4, 4).any(axis=2))
        assert sorted(zip(*nz)) == [(2, 2), (3, 3)]

    return LossCase("f64_labels_truncate", base.cls, base.reg, base.reg_t, lab, chk, head=True)


def _extreme_logits():
    rows_ = [[80, 0, 0], [0, 80, 0], [-80, 0, 0], [80, 80, 80], [-80, -80, -80], [80, 79, 78.5],
             [1e4, 0, 0], [0, 0, 1e4], [1e4, 1e4, 1e4], [-1e4, 0, 0], [-1e4, -1e4, -1e4], [1e4, -1e4, 0]]
    cls = np.array(rows_, F32).reshape(1, -1, 3)
    n = cls.shape[1]
    lab = (np.arange(n) % 3).astype(np.int32).reshape(1, n)
    r = np.random.RandomState(51)
    reg = r.randn(1, n, 4).astype(F32)

    def chk(case, ref):
        assert np.isfinite(ref["loss"]).all() and np.isfinite(ref["dcls"]).all() and ref["loss"][0] > 100

    return LossCase("extreme_logits", cls, reg, reg.astype(np.float64) + 0.25, lab, chk)


def _garbage(name, base):
    """base with NaN / inf / huge values in cls, reg and reg_t of its unlabelled rows."""
    cls, reg, reg_t = base.cls.copy(), base.reg.copy(), base.reg_t.copy()
    un = np.nonzero(loss_ref.classify_labels(base.labels.reshape(-1), base.C) < 0)[0]
    assert len(un) >= 6
    junk = [np.nan, np.inf, -np.inf, 3e38, -3e38, 1e30]
    for k, i in enumerate(un):
        n, l = divmod(int(i), base.cls.shape[1])
        cls[n, l, k % base.C] = junk[k % 6]
        reg[n, l, k % reg.shape[2]] = junk[(k + 1) % 6]
        reg_t[n, l, k % 4] = [np.nan, np.inf, 1e300, -1e300][k % 4]

    def chk(case, ref):
        base.check(base, ref)
        assert np.isfinite(ref["loss"]).all() and np.isfinite(ref["dcls"]).all() and np.isfinite(ref["dreg"]).all()
        dirty = loss_ref.stage(*case.flat(), sigma=case.sigma, head=case.head)
        for k in ref:
            assert np.array_equal(dirty[k], ref[k]), (case.name, k)     # loss_ref never reads those rows

    return LossCase(name, cls, reg, reg_t, base.labels, chk, sigma=base.sigma, head=base.head, clean=base)


def _empty():
    z = np.zeros
    return LossCase("rows_0", z((2, 0, 2), F32), z((2, 0, 4), F32), z((2, 0, 4)), z((2, 0), np.int32), _nan_loss)


def _build():
    i32, f64 = np.int32, np.float64
    cases = [_empty()]
    for rows in (1, 63, 64, 65, 257):
        cases.append(_random(f"rpn_rows_{rows}", 1, rows, 2, False, rows, i32,
                             check=_both_branches if rows > 1 else None))
    cases.append(_random("rpn_f64_labels_2x100", 2, 100, 2, False, 3, f64, n_labelled=60, n_pos=17,
                         check=_both_branches))
    # several workgroups in the forward and full-size tiles in the backward: train.py's shape at N = 2
    multi = _random("rpn_multi_workgroup", 2, 38 * 38 * 9, 2, False, 5, i32, n_labelled=512, n_pos=200,
                    check=_both_branches)
    cases.append(multi)
    for C in (2, 21, 128):
        cases.append(_random(f"head_3x5_c{C}", 3, 5, C, True, 100 + C, f64))
    cases.append(_random("head_i32_labels_3x5_c21", 3, 5, 21, True, 7, i32, n_labelled=9, n_pos=4))
    cases.append(_random("head_c21_two_tiles", 2, 130, 21, True, 8, f64, check=_both_branches))
    cases.append(_random("head_c128_two_tiles", 2, 40, 128, True, 9, f64, n_labelled=70, n_pos=30))
    cases.append(_random("head_sigma3_2x64_c21", 2, 64, 21, True, 10, f64, sigma=3.0, check=_both_branches))
    cases.append(_random("all_unlabelled", 2, 70, 2, False, 12, i32, n_labelled=0, n_pos=0, check=_nan_loss))
    cases.append(_random("all_unlabelled_head_f64", 3, 5, 21, True, 13, f64, n_labelled=0, n_pos=0, check=_nan_loss))
    cases.append(_random("no_positives", 2, 70, 2, False, 14, i32, n_labelled=50, n_pos=0, check=_no_positives))
    cases.append(_random("single_positive", 2, 70, 2, False, 15, i32, n_labelled=30, n_pos=1, check=_one_positive))
    cases.append(_random("single_positive_head", 3, 5, 21, True, 16, f64, n_labelled=8, n_pos=1, check=_one_positive))
    cases.append(_threshold_case("sl1_threshold_sigma1", 1.0))
    cases.append(_threshold_case("sl1_threshold_sigma3", 3.0))
    cases.append(_head_label_ends("head_label_0_and_last_c21", 21))
    cases.append(_head_label_ends("head_label_0_and_last_c128", 128))
    cases.append(_out_of_range("labels_out_of_range_rpn_i32", False, i32))
    cases.append(_out_of_range("labels_out_of_range_head_f64", True, f64))
    cases.append(_truncating_labels())
    cases.append(_extreme_logits())
    cases.append(_garbage("garbage_unlabelled_rpn", _random("garbage_base_rpn", 2, 100, 2, False, 17, i32,
                                                            n_labelled=40, n_pos=12)))
    cases.append(_garbage("garbage_unlabelled_head", _random("garbage_base_head", 3, 8, 21, True, 18, f64,
                                                             n_labelled=14, n_pos=6)))
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
MULTI_WORKGROUP = "rpn_multi_workgroup"
