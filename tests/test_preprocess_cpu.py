"""The preprocessing contract without a GPU: the numpy reference
(tests/preprocess_ref.py) against the two scipy.ndimage calls that
``skimage.transform.resize`` makes, its own properties, the box reference, and
the C-ABI's argument validation (DESIGN.md §3 "Preprocessing")."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import preprocess_plan_cases as PC  # noqa: E402
import preprocess_ref as R  # noqa: E402
from replication_faster_rcnn_amd import data  # noqa: E402


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_reference_matches_scipy(case):
    """gaussian_filter(mode='mirror') then zoom(order=1, mode='mirror',
    grid_mode=True), as skimage >= 0.19 calls them: 1e-12 or better."""
    ndi = pytest.importorskip("scipy.ndimage")
    _, in_hw, out_hw, _, mean, std = case
    img, ref = R.case_data(case)
    p = img.astype(np.float64) / 255
    sig = [max(0, (i / o - 1) / 2) for i, o in zip(in_hw, out_hw)]
    r = np.empty(tuple(out_hw) + (3,))
    for c in range(3):
        f = ndi.gaussian_filter(p[:, :, c], sig, mode="mirror")
        r[:, :, c] = ndi.zoom(f, (out_hw[0] / in_hw[0], out_hw[1] / in_hw[1]), order=1, mode="mirror",
                              grid_mode=True)
    want = ((r - np.array(mean)) / np.array(std)).transpose(2, 0, 1)
    err = np.abs(ref - want).max()
    print(f"{case[0]}: max |reference - scipy| = {err:.3g}")
    assert ref.shape == (3,) + tuple(out_hw) and err <= 1e-12


def test_case_table_covers_the_contract():
    got = {(c[1], c[2]) for c in R.CASES} | {(c.in_hw, c.out_hw) for c in PC.CASES}
    for pair in [((4, 5), (4, 5)), ((5, 7), (12, 12)), ((2, 3), (8, 8)), ((1, 1), (4, 4)), ((13, 9), (6, 12)),
                 ((20, 31), (6, 7)), ((64, 48), (37, 41)), ((24, 24), (6, 6)), ((4, 4), (1, 1)),
                 ((3, 499), (4, 600)), ((375, 500), (600, 600)),
                 # the launch-plan cases (tests/preprocess_plan_cases.py)
                 ((90, 200), (45, 100)), ((46, 161), (20, 70)), ((60, 60), (12, 12)), ((30, 650), (6, 130)),
                 ((120, 40), (40, 100)), ((20, 300), (50, 100)), ((10, 96), (10, 64)), ((10, 98), (10, 65)),
                 ((66, 20), (33, 16)), ((20, 20), (33, 16)), ((20, 12), (33, 16)), ((2, 40), (1, 20)),
                 ((2, 2), (1, 1)), ((1, 130), (3, 65)), ((500, 375), (200, 150)), ((2, 16384), (1, 4096))]:
        assert pair in got, pair
    kinds = {c[3] for c in R.CASES}
    assert kinds == {"random", "checker", "zeros", "full"}
    assert any(c[4] != R.MEAN and c[5] != R.STD for c in R.CASES)
    # the taps the tolerance is derived from
    assert R.taps(5, 12) == 2 and R.taps(24, 6) == 14 and R.taps(13, 6) == 2 + 2 * int(4 * (13 / 6 - 1) / 2 + 0.5)
    assert R.tolerance((5, 7), (12, 12)) == (4 * 4 + 16) * 2.0 ** -24 / 0.224
    assert R.tolerance((24, 24), (6, 6)) == (4 * 28 + 16) * 2.0 ** -24 / 0.224


def test_fold_is_mirror_without_edge_repeat():
    assert [R.fold(i, 5) for i in range(-5, 11)] == [3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2]
    assert [R.fold(i, 2) for i in range(-3, 5)] == [1, 0, 1, 0, 1, 0, 1, 0]
    assert all(R.fold(i, 1) == 0 for i in range(-7, 8))


def test_reference_properties():
    rng = np.random.default_rng(1)
    # a constant image stays constant, up- and downscaled (every matrix row sums to 1)
    for in_hw, out_hw in [((5, 7), (12, 12)), ((20, 31), (6, 7)), ((13, 9), (6, 12)), ((4, 4), (1, 1))]:
        p = np.full(in_hw + (3,), 0.3)
        assert np.abs(R.resize(p, out_hw) - 0.3).max() < 1e-15
        for n_in, n_out in zip(in_hw, out_hw):
            assert np.abs(R.axis_matrix(n_in, n_out).sum(1) - 1).max() < 1e-15
    # in == out returns p exactly
    p = rng.random((4, 5, 3))
    assert np.array_equal(R.resize(p, (4, 5)), p)
    assert np.array_equal(R.axis_matrix(7, 7), np.eye(7))
    # a 1x1 source: every output is that pixel
    p = rng.random((1, 1, 3))
    assert np.array_equal(R.resize(p, (4, 4)), np.broadcast_to(p, (4, 4, 3)))
    # upscaling has no Gaussian; ratio 4 has sigma 1.5 and radius 6
    assert R.sigma_radius(500, 600) == (0.0, 0) and R.sigma_radius(24, 6) == (1.5, 6)
    # the exact integer position: 499 -> 600, row d at ((2d+1) 499 - 600) / 1200
    b = R.bilinear_matrix(499, 600)
    d = 437
    num = (2 * d + 1) * 499 - 600
    assert b[d, num // 1200] == 1 - (num % 1200) / 1200 and b[d, num // 1200 + 1] == (num % 1200) / 1200


def test_box_reference_is_data_rescale_boxes():
    rng = np.random.default_rng(2)
    boxes = np.around(rng.uniform(0, 400, (3, 32, 4)))
    boxes[:, 20:] = -1
    boxes[1, 3, 1] = -7.0
    hw = np.array([[375, 500], [333, 499], [0, 500]], np.int32)
    got = R.rescale_boxes(boxes, hw, (600, 608))
    for n in range(2):
        assert np.array_equal(got[n], data.rescale_boxes(boxes[n], hw[n], (600, 608)))
    assert (got[2] == -1).all() and got[1, 3, 1] == -1 and (got[:, 20:] == -1).all()


def test_pack_images_layout_and_rejections():
    import torch
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (8, 6, 4), dtype=np.uint8)[:, ::2, :3]     # a strided view
    c = torch.from_numpy(rng.integers(0, 256, (1, 1, 3), dtype=np.uint8))
    pixels, offset, hw, max_hw = data.pack_images([a, b, c])
    assert pixels.dtype == torch.uint8 and offset.dtype == torch.int64 and hw.dtype == torch.int32
    assert offset.tolist() == [0, 105, 105 + 72] and hw.tolist() == [[5, 7], [8, 3], [1, 1]] and max_hw == (8, 7)
    assert pixels.numel() == 105 + 72 + 3
    assert np.array_equal(pixels.numpy()[105:177].reshape(8, 3, 3), b)
    for bad in ([a[:, :, :2]], [a[:, :, 0]], [a.astype(np.float32)], [np.zeros((0, 4, 3), np.uint8)], [], a,
                [np.concatenate([a, a[:, :, :1]], 2)], [c.float()]):
        with pytest.raises(ValueError, match="pack_images"):
            data.pack_images(bad)


def test_argument_validation_without_gpu():
    """Limits are reported before any HIP call: rc -1, a message naming the
    argument, and a workspace size of 0 for the same arguments."""
    from replication_faster_rcnn_amd import _lib
    lib = _lib.load(require_gpu=False)
    mean = (ctypes.c_float * 3)(*R.MEAN)
    std = (ctypes.c_float * 3)(*R.STD)

    def call(N=1, max_h=8, max_w=8, out_h=4, out_w=4, mean=mean, std=std):
        return lib.frcnn_preprocess(N, None, 0, None, None, max_h, max_w, out_h, out_w, mean, std, None, None,
                                    None, 0, None)

    assert lib.frcnn_preprocess_workspace_size(1, 8, 8, 4, 4) > 0
    for kw, name in [(dict(N=0), b"N"), (dict(N=1025), b"N"), (dict(out_h=0), b"out_h"), (dict(out_w=4097), b"out_w"),
                     (dict(max_w=16385), b"max_w"), (dict(max_h=0), b"max_h")]:
        assert call(**kw) == -1 and name + b" must" in lib.frcnn_last_error(), kw
        a = dict(N=1, max_h=8, max_w=8, out_h=4, out_w=4)
        a.update(kw)
        assert lib.frcnn_preprocess_workspace_size(a["N"], a["max_h"], a["max_w"], a["out_h"], a["out_w"]) == 0
    assert call(mean=None) == -1 and b"mean" in lib.frcnn_last_error()
    assert call(std=(ctypes.c_float * 3)(0.2, 0.0, 0.2)) == -1 and b"std" in lib.frcnn_last_error()
    # valid limits, null device pointers: still rejected on the host
    assert call() == -1 and b"null" in lib.frcnn_last_error()
    assert lib.frcnn_rescale_boxes(0, 4, None, None, 600, 600, None, None) == -1
    assert b"N=0" in lib.frcnn_last_error()
    assert lib.frcnn_rescale_boxes(2, 4, None, None, 600, 600, None, None) == -1
    assert b"null" in lib.frcnn_last_error()
