"""ops.preprocess on the named launch-plan cases (tests/preprocess_plan_cases.py;
DESIGN.md §3 "Preprocessing", "Launch-plan branches and the cases that pin
them").  Needs an MI355X.

Every case first asserts, through the library's own plan query, that its launch
takes the tile height, footprint and grid the case names, and only then
compares values: with the dense numpy fp64 reference (the banded one for
``max_extent``) under the derived bound of preprocess_ref.tolerance, unchanged."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import preprocess_plan_cases as PC  # noqa: E402
import preprocess_ref as R  # noqa: E402
from replication_faster_rcnn_amd import _lib, data, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def run(images, out_hw, max_hw="own"):
    """ops.preprocess of a list of uint8 images -> (numpy [N,3,oh,ow], status list)."""
    pixels, offset, hw, own = data.pack_images(list(images))
    out, status = ops.preprocess(pixels.to(DEV), offset.to(DEV), hw.to(DEV), out_hw,
                                 max_hw=own if max_hw == "own" else max_hw)
    return out.cpu().numpy(), status.tolist()


def max_err(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max())


@pytest.mark.parametrize("c", PC.CASES, ids=PC.CASE_IDS)
def test_case_takes_its_plan_and_matches_the_reference(c):
    p = _lib.preprocess_plan(1, c.in_hw, c.out_hw)
    assert p["TH"] == c.TH and (p["lds_rows"], p["lds_cols"], p["lds_bytes"]) == c.lds, p
    assert (p["grid_y"], p["grid_x"], p["grid_z"]) == c.tiles + (1,)
    assert p == PC.plan(1, c.in_hw, c.out_hw)
    tol = R.tolerance(c.in_hw, c.out_hw)
    for kind in c.kinds:
        img, ref = PC.case_data(c, kind)
        got, status = run([img], c.out_hw)
        err = max_err(got[0], ref)
        print(f"{c.id}/{kind}: TH {p['TH']}, {p['lds_rows']} x {p['lds_cols']}, max |device - reference| = {err:.3g}, "
              f"bound {tol:.3g}")
        assert status == [0] and got.shape == (1, 3) + c.out_hw and got.dtype == np.float32
        assert err <= tol
        # the wrapper's default bounds (5 x out_size) shrink the tiles; the bits stay
        wide, sw = run([img], c.out_hw, max_hw=None)
        assert sw == [0] and np.array_equal(wide, got), f"{c.id}/{kind}: max_hw=None changes the bits"


def test_ladder_of_tile_heights_gives_the_same_bits():
    img, ref = PC.ladder_data()
    outs, ths = [], []
    for max_hw, th in PC.LADDER:
        p = _lib.preprocess_plan(1, max_hw, PC.LADDER_OUT)
        assert p["TH"] == th, (max_hw, p)
        ths.append(p["TH"])
        got, status = run([img], PC.LADDER_OUT, max_hw=max_hw)
        assert status == [0]
        outs.append(got)
    assert ths == [32, 16, 8, 4, 2]
    for th, o in zip(ths[1:], outs[1:]):
        assert np.array_equal(o, outs[0]), f"TH {th} differs from TH 32"
    err, tol = max_err(outs[0][0], ref), R.tolerance(PC.LADDER_IMAGE, PC.LADDER_OUT)
    print(f"ladder: max |device - reference| = {err:.3g}, bound {tol:.3g}")
    assert err <= tol


def test_mixed_batch_of_fast_and_slow_workgroups():
    """The images of down_x_tiles, up_down and ratio5 and an upscaled one in
    one launch to (45, 100): two-tap and Gaussian workgroups side by side.  Each
    image equals itself alone (launched under its own bounds, so under another
    plan) bit for bit, and the reference."""
    out_hw = (45, 100)
    imgs = [PC.case_image(PC.case(cid)) for cid in ("down_x_tiles", "up_down", "ratio5")] + [R.image((30, 80), seed=77)]
    radii = [(PC.axis_radius(im.shape[0], 45), PC.axis_radius(im.shape[1], 100)) for im in imgs]
    assert radii == [(2, 2), (0, 4), (1, 0), (0, 0)]
    pixels, offset, hw, max_hw = data.pack_images(imgs)
    assert max_hw == (90, 300)
    out = torch.full((4, 3) + out_hw, float("nan"), device=DEV)
    got, status = ops.preprocess(pixels.to(DEV), offset.to(DEV), hw.to(DEV), out_hw, max_hw=max_hw, out=out)
    assert got is out and status.tolist() == [0, 0, 0, 0]
    got = got.cpu().numpy()
    assert not np.isnan(got).any()
    batch = _lib.preprocess_plan(4, max_hw, out_hw)
    alone_th = [_lib.preprocess_plan(1, im.shape[:2], out_hw)["TH"] for im in imgs]
    assert batch["grid_z"] == 4 and any(th != batch["TH"] for th in alone_th), (batch, alone_th)
    for i, im in enumerate(imgs):
        alone, s = run([im], out_hw)
        assert s == [0] and np.array_equal(got[i], alone[0]), f"image {i} differs from itself preprocessed alone"
        assert max_err(got[i], R.preprocess(im, out_hw)) <= R.tolerance(im.shape[:2], out_hw)


def test_accepted_and_rejected_limits():
    """h == 5 * out_h and w == max_w are accepted; one more of either is status
    1 and zeros."""
    out_hw, max_hw = (4, 8), (21, 12)
    buf = R.image((21, 13), seed=78)
    pixels = torch.from_numpy(buf.reshape(-1).copy()).to(DEV)
    hw = torch.tensor([[20, 12], [21, 12], [20, 13], [20, 12]], dtype=torch.int32, device=DEV)
    offset = torch.zeros(4, dtype=torch.int64, device=DEV)
    out = torch.full((4, 3) + out_hw, float("nan"), device=DEV)
    got, status = ops.preprocess(pixels, offset, hw, out_hw, max_hw=max_hw, out=out)
    assert status.tolist() == [0, 1, 1, 0]
    got = got.cpu().numpy()
    assert (got[1] == 0).all() and (got[2] == 0).all()
    img = buf.reshape(-1)[:3 * 20 * 12].reshape(20, 12, 3)
    assert PC.axis_radius(20, 4) == 8
    assert max_err(got[0], R.preprocess(img, out_hw)) <= R.tolerance((20, 12), out_hw)
    assert np.array_equal(got[0], got[3])


def test_pixel_offsets_past_2_to_31():
    """A pixel buffer of 2^31 + 4 KiB bytes, zero-filled, with one image at 0
    and the same kind of image ending at the buffer's last byte: both equal the
    same images in a small buffer bit for bit, and one byte further is status 2."""
    c = PC.case("w65")
    h, w = c.in_hw
    nb = 3 * h * w
    a, b = PC.case_image(c), R.image(c.in_hw, seed=79)
    small, s = run([a, b], c.out_hw)
    assert s == [0, 0]
    total = (1 << 31) + 4096
    pixels = torch.zeros(total, dtype=torch.uint8, device=DEV)
    far = total - nb
    assert far >= 1 << 31
    pixels[:nb] = torch.from_numpy(a.reshape(-1).copy()).to(DEV)
    pixels[far:] = torch.from_numpy(b.reshape(-1).copy()).to(DEV)
    hw = torch.tensor([[h, w]] * 3, dtype=torch.int32, device=DEV)
    offset = torch.tensor([0, far, far + 1], dtype=torch.int64, device=DEV)
    got, status = ops.preprocess(pixels, offset, hw, c.out_hw, max_hw=c.in_hw)
    assert status.tolist() == [0, 0, 2]
    got = got.cpu().numpy()
    assert np.array_equal(got[0], small[0]) and np.array_equal(got[1], small[1])
    assert (got[2] == 0).all()
    assert max_err(got[1], R.preprocess(b, c.out_hw)) <= R.tolerance(c.in_hw, c.out_hw)
