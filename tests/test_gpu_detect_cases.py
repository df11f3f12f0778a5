"""ops.detect on the named edge cases of tests/detect_cases.py (DESIGN.md §3 "Detection edges and
the cases that pin them") against tests/detect_ref.py: all six outputs compared as bits through
integer views, so a zero's sign counts.  fp32 runs every case and holds the reference to the
case's own precondition (for the chain cases the closed form); float16 and bfloat16 run the
cases listed by name in ``detect_cases.HALF_NAMES`` against the reference on the widened rounded
inputs.  Every case runs twice, the second time into caller-owned outputs filled with 7 and a
workspace of exactly ``frcnn_detect_workspace_size`` bytes, 256-byte aligned, filled with 0xFF."""
import numpy as np
import pytest
import torch

import detect_cases as dc
from replication_faster_rcnn_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
_single = {}        # fp32 outputs of single-image runs, for the batch case


def device_inputs(case, dtype):
    rois, rcount, cls, reg = (torch.tensor(a) for a in case.inputs("f32"))       # a copy: the case's arrays are read-only
    dt = TORCH[dtype]
    return rois.to(DEV), rcount.to(DEV), cls.to(dt).to(DEV), reg.to(dt).to(DEV)       # .to rounds once


def call(case, args, **kw):
    return ops.detect(*args, img_h=case.img_h, img_w=case.img_w, **case.kwargs(), **kw)


def host(out):
    return [t.cpu().numpy() for t in out]


def run_case(case, dtype):
    want = case.reference(dtype)
    if dtype == "f32":
        case.check(case, want)
    else:       # the rounding the reference saw is the device's
        _, _, cls, reg = device_inputs(case, dtype)
        for mine, dev in zip(case.inputs(dtype)[2:], (cls, reg)):
            assert np.array_equal(dc.bits(mine), dc.bits(dev.float().cpu().numpy())), "the reference's rounding"
    args = device_inputs(case, dtype)
    got = host(call(case, args))
    dc.same_bits(got, want, f"{case.name} {dtype}")
    # again: caller-owned outputs (every element must be stored), an exact, aligned, dirty workspace
    N, md = case.N, case.max_det
    outs = (torch.full((N, md, 4), 7.0, device=DEV), torch.full((N, md), 7, dtype=torch.int32, device=DEV),
            torch.full((N, md), 7.0, device=DEV), torch.full((N, md), 7, dtype=torch.int32, device=DEV),
            torch.full((N,), 7, dtype=torch.int32, device=DEV), torch.full((N,), 7, dtype=torch.int32, device=DEV))
    need = int(ops._lib.load().frcnn_detect_workspace_size(N, case.R, case.C))
    assert need > 0
    ws = torch.full((need + 512,), 0xFF, dtype=torch.uint8, device=DEV)
    ws = ws[(-ws.data_ptr()) % 256:][:need]
    assert ws.data_ptr() % 256 == 0 and ws.numel() == need
    again = call(case, args, out=outs, workspace=ws)
    assert all(a is b for a, b in zip(again, outs))
    dc.same_bits(host(again), want, f"{case.name} {dtype} (caller-owned outputs, 0xFF workspace)")
    return got


@pytest.mark.parametrize("case", dc.CASES, ids=repr)
def test_case_f32(case):
    _single[case.name] = run_case(case, "f32")


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("name", dc.HALF_NAMES)
def test_case_16bit(name, dtype):
    run_case(dc.BY_NAME[name], dtype)


@pytest.mark.parametrize("dtype", dc.DTYPES)
def test_batch_image_by_image(dtype):
    """Each image of the batch comes out as its case does when run alone."""
    batch = dc.BY_NAME["batch_three"]
    got = host(call(batch, device_inputs(batch, dtype)))
    for n, part in enumerate(batch.parts):
        alone = _single.get(part.name) if dtype == "f32" else None
        if alone is None:
            alone = host(call(part, device_inputs(part, dtype)))
        dc.same_bits([a[n:n + 1] for a in got], alone, f"image {n} against {part.name} alone, {dtype}")
        dc.same_bits(alone, part.reference(dtype), f"{part.name} alone, {dtype}")
