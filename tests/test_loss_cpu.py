"""The losses contract without a GPU: tests/loss_ref.py over the case table
(tests/loss_cases.py) against the reference formulas run by torch on the CPU in
fp64 -- train.fast_rcnn_loc_loss, F.cross_entropy(ignore_index=-1), the reg_ind
gather of train.py:112-117 and their autograd gradients --, and the C-ABI's
host-side surface (symbols, argument validation before any HIP call)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_cases
import loss_ref
from replication_faster_rcnn_amd import train

GRADS = [(1.0, 1.0), (2.0, 0.5)]


def torch_reference(case, g_cls, g_reg):
    """(losses [2], dcls [rows, C], dreg [rows, 4P], n_valid, n_pos) in fp64.  Labels outside
    -1..C-1, which torch rejects, are given to it as ignored rows: the contract skips them in
    both terms.  A case with garbage in unlabelled rows is run on its clean inputs (torch's
    dense log-softmax backward would let a NaN through)."""
    src = case.clean if case.clean is not None else case
    N, L, C = src.cls.shape
    cl = loss_ref.classify_labels(src.labels.reshape(-1), C).reshape(N, L)
    lab = torch.from_numpy(np.where(cl == -2, -1, src.labels)).long()        # torch's own truncation
    assert np.array_equal(lab.numpy(), np.where(cl == -2, -1, cl))
    cls = torch.from_numpy(src.cls).double().requires_grad_(True)            # [N, L, C]
    reg = torch.from_numpy(src.reg).double().requires_grad_(True)
    reg_t = torch.from_numpy(src.reg_t)
    ce = F.cross_entropy(cls.permute(0, 2, 1), lab, ignore_index=-1)
    pred = reg
    if src.head:  # train.py:112-117
        reg_ind = lab.clamp(min=0).unsqueeze(-1) * 4
        reg_ind = torch.cat([reg_ind, reg_ind + 1, reg_ind + 2, reg_ind + 3], dim=-1)
        pred = torch.gather(reg, dim=-1, index=reg_ind)
    rl = train.fast_rcnn_loc_loss(pred, reg_t, lab.double(), sigma=src.sigma)
    if N * L:
        (g_cls * ce + g_reg * rl).backward()
    dcls = cls.grad.numpy().reshape(N * L, C) if cls.grad is not None else np.zeros((N * L, C))
    dreg = reg.grad.numpy().reshape(N * L, -1) if reg.grad is not None else np.zeros((N * L, src.reg.shape[2]))
    return (np.array([float(ce.detach()), float(rl.detach())]), dcls, dreg, int((lab >= 0).sum()), int((lab > 0).sum()))


@pytest.mark.parametrize("case", loss_cases.CASES, ids=lambda c: c.name)
def test_case_precondition(case):
    case.check(case, loss_cases.reference(case))


@pytest.mark.parametrize("g", GRADS, ids=lambda g: f"g{g[0]}_{g[1]}")
@pytest.mark.parametrize("case", loss_cases.CASES, ids=lambda c: c.name)
def test_loss_ref_matches_torch_fp64(case, g):
    ref = loss_cases.reference(case, *g)
    loss, dcls, dreg, n_valid, n_pos = torch_reference(case, *g)
    assert (ref["stats"][0], ref["stats"][1]) == (n_valid, n_pos)
    np.testing.assert_allclose(ref["loss"], loss, rtol=1e-5, atol=1e-7, equal_nan=True)
    assert np.array_equal(ref["dcls"] == 0, dcls == 0), "zero pattern of dcls"
    assert np.array_equal(ref["dreg"] == 0, dreg == 0), "zero pattern of dreg"
    np.testing.assert_allclose(ref["dcls"], dcls, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(ref["dreg"], dreg, rtol=1e-5, atol=1e-7)


def test_loss_ref_unused_loss_has_zero_gradient():
    case = loss_cases.BY_NAME["head_3x5_c21"]
    both = loss_ref.stage(*case.flat(), sigma=case.sigma, head=True)
    only_cls = loss_ref.stage(*case.flat(), sigma=case.sigma, head=True, g_reg=None)
    only_reg = loss_ref.stage(*case.flat(), sigma=case.sigma, head=True, g_cls=None)
    assert not only_cls["dreg"].any() and np.array_equal(only_cls["dcls"], both["dcls"])
    assert not only_reg["dcls"].any() and np.array_equal(only_reg["dreg"], both["dreg"])


def test_table_covers_the_sizes_and_dtypes():
    rows = {c.rows for c in loss_cases.CASES}
    assert {0, 1, 63, 64, 65, 257} <= rows and max(rows) > 2 * 256 * 8
    assert max(c.rows for c in loss_cases.CASES if c.name != loss_cases.MULTI_WORKGROUP) <= 400
    heads = {c.C for c in loss_cases.CASES if c.head and c.cls.shape[:2] == (3, 5)}
    assert {2, 21, 128} <= heads
    assert {c.labels.dtype for c in loss_cases.CASES} == {np.dtype(np.int32), np.dtype(np.float64)}
    assert {c.sigma for c in loss_cases.CASES} == {1.0, 3.0}


def test_symbols_declared_and_exported():
    from replication_faster_rcnn_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "frcnn_capi.h")).read(), flags=re.S)
    syms = set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH) if os.path.exists(_lib.LIB_PATH) else None
    assert lib is not None, "libfrcnn_mi355x.so not built (run __graft_entry__.build())"
    for s in ("frcnn_losses_workspace_size", "frcnn_losses_fwd", "frcnn_losses_bwd"):
        assert s in syms and s in _lib.SIGNATURES and hasattr(lib, s), s


def test_argument_validation_without_gpu():
    """Limits are checked on the host before any HIP call: rc = -1 and a message naming the argument."""
    from replication_faster_rcnn_amd import _lib
    lib = _lib.load(require_gpu=False)
    fwd = lambda rows, C, P, sigma=1.0: lib.frcnn_losses_fwd(rows, C, P, None, None, None, None, 0, sigma, None,
                                                              None, None, 0, None)   # noqa: E731
    bwd = lambda rows, C, P, sigma=1.0: lib.frcnn_losses_bwd(rows, C, P, None, None, None, None, 0, sigma, None,
                                                              None, None, None, None, None)   # noqa: E731
    for fn in (fwd, bwd):
        assert fn(10, 1, 1) == -1 and b"C=1" in lib.frcnn_last_error()
        assert fn(10, 129, 1) == -1 and b"C=129" in lib.frcnn_last_error()
        assert fn(-1, 2, 1) == -1 and b"rows=-1" in lib.frcnn_last_error()
        assert fn(1 << 31, 2, 1) == -1 and b"rows=" in lib.frcnn_last_error()
        assert fn(10, 21, 2) == -1 and b"P=2" in lib.frcnn_last_error()
        assert fn(10, 2, 1, 0.0) == -1 and b"sigma" in lib.frcnn_last_error()
        assert fn(10, 2, 1, float("nan")) == -1 and b"sigma" in lib.frcnn_last_error()
    assert fwd(10, 2, 1) == -1 and b"null" in lib.frcnn_last_error()     # valid shape, no buffers: still no launch
    assert bwd(10, 2, 1) == -1 and b"null" in lib.frcnn_last_error()
    assert bwd(0, 2, 1) == 0                                               # no rows: no output elements, no launch
    assert lib.frcnn_losses_workspace_size(10, 1) == 0 and lib.frcnn_losses_workspace_size(-1, 2) == 0
    assert lib.frcnn_losses_workspace_size(0, 2) == 0
    one = lib.frcnn_losses_workspace_size(256, 2)
    assert one >= 32 and lib.frcnn_losses_workspace_size(257, 2) >= 64
    assert lib.frcnn_losses_workspace_size(1 << 30, 128) == lib.frcnn_losses_workspace_size(2048 * 256, 2)
