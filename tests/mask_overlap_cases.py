"""Named cases of ops.mask_overlap (DESIGN.md "COCO segm evaluation"): each a tiny hand-built
input, the launch plan it must reach, and for the closed-form ones the values it must give.

CASES: name -> builder of dict(det_masks uint8 [N, D, H, W], gt_masks uint8 [N, G, H, W],
det_labels / det_count / gt_labels (or None), n_class (or None), plan: the fields of
frcnn_mask_overlap_plan that pin the case, expect: {(output, index): value} in closed form,
cells: {(n, d, g): True / False}: whether the pair kernel reads the bits of the pair at all).
"""
import numpy as np

CASES = {}


def case(name):
    def deco(f):
        CASES[name] = f
        return f
    return deco


def pts(H, W, *points, value=1):
    m = np.zeros((H, W), np.uint8)
    for y, x in points:
        m[y, x] = value
    return m


def rect(H, W, y0, x0, y1, x1, value=1):
    m = np.zeros((H, W), np.uint8)
    m[y0:y1, x0:x1] = value
    return m


def pack(det, gt, det_labels=None, det_count=None, gt_labels=None, n_class=None, plan=None, expect=None, cells=None):
    """det / gt: lists (images) of lists of [H, W] masks."""
    dm = np.ascontiguousarray(np.stack([np.stack(d) for d in det]), np.uint8)
    gm = np.ascontiguousarray(np.stack([np.stack(g) for g in gt]), np.uint8)
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)       # noqa: E731
    return dict(det_masks=dm, gt_masks=gm, det_labels=i32(det_labels), det_count=i32(det_count),
                gt_labels=i32(gt_labels), n_class=n_class, plan=plan or {}, expect=expect or {}, cells=cells or {})


def random_masks(seed, N, K, H, W, density=0.5):
    r = np.random.default_rng(seed)
    vals = np.array([1, 2, 128, 255], np.uint8)
    return (r.uniform(size=(N, K, H, W)) < density) * vals[r.integers(0, 4, (N, K, H, W))]


# ---------------------------------------------------------------- row geometry
def _geometry(H, W, seed, **plan):
    def build():
        d, g = random_masks(seed, 2, 3, H, W), random_masks(seed + 1, 2, 2, H, W)
        return pack(list(d), list(g), plan=dict(dict(words=(W + 63) // 64, edges=int(W % 16 != 0), pack_blocks=10,
                                                     pair_blocks=6), **plan))
    return build


for _w, _h in [(1, 5), (15, 5), (16, 5), (17, 5), (63, 5), (64, 5), (65, 5), (128, 5), (600, 5)]:
    CASES["w%d" % _w] = _geometry(_h, _w, 100 + _w)
# an odd width: rows, and masks, start at every byte alignment (37 r mod 16 takes all sixteen values)
CASES["w37_every_alignment"] = _geometry(17, 37, 200, items=4, bands=1)
CASES["h1"] = _geometry(1, 100, 201, bands=1)
CASES["2x4096"] = _geometry(2, 4096, 202, words=64, items=256, band_rows=16, bands=1)
CASES["4096x2"] = _geometry(4096, 2, 203, words=1, items=2, band_rows=2048, bands=2)
# a second band of two rows: 39 patterns per row, 105 rows per band
CASES["two_bands"] = _geometry(107, 600, 204, items=39, band_rows=105, bands=2)


# ------------------------------------------------------------------------ bits
@case("col63_col64_touch")
def _():
    H, W = 3, 130
    return pack([[pts(H, W, (1, 63))]], [[pts(H, W, (1, 64))]], plan=dict(words=3, edges=1),
                expect={("inter", (0, 0, 0)): 0, ("det_area", (0, 0)): 1, ("gt_area", (0, 0)): 1},
                cells={(0, 0, 0): False})                    # word columns 0 and 1: windows that touch


@case("col63_both")
def _():
    H, W = 3, 130
    return pack([[pts(H, W, (1, 63))]], [[pts(H, W, (1, 63))]], plan=dict(words=3, edges=1),
                expect={("inter", (0, 0, 0)): 1}, cells={(0, 0, 0): True})


@case("first_last_bytes")
def _():
    # the first and last byte of a row and of the mask, at a width whose last vector is a tail: a
    # read past W would see the next row's first byte, or the next mask's
    H, W = 4, 67
    a = pts(H, W, (0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))
    b = pts(H, W, (0, W - 1), (1, 0), (H - 1, W - 1))
    c = pts(H, W, (0, 0), (2, 0))
    return pack([[a, b]], [[a, b, c]], plan=dict(words=2, edges=1, items=6),
                expect={("inter", (0, 0, 0)): 4, ("inter", (0, 0, 1)): 2, ("inter", (0, 0, 2)): 1,
                        ("inter", (0, 1, 2)): 0, ("det_area", (0, 0)): 4, ("det_area", (0, 1)): 3,
                        ("gt_area", (0, 2)): 2})


@case("byte_values")
def _():
    H, W = 2, 16
    m = np.zeros((H, W), np.uint8)
    m[0, :4] = [1, 2, 128, 255]
    m[1, 5:9] = [255, 128, 2, 1]
    full = np.full((H, W), 2, np.uint8)
    return pack([[m]], [[full, m]], plan=dict(words=1, edges=0, items=1),
                expect={("inter", (0, 0, 0)): 8, ("inter", (0, 0, 1)): 8, ("det_area", (0, 0)): 8,
                        ("gt_area", (0, 0)): 32})


@case("full_full")
def _():
    H, W = 9, 70
    full = np.full((H, W), 255, np.uint8)
    return pack([[full]], [[full]], expect={("inter", (0, 0, 0)): H * W, ("det_area", (0, 0)): H * W})


# --------------------------------------------------------------------- windows
@case("disjoint_rows")
def _():
    H, W = 8, 70
    return pack([[rect(H, W, 0, 0, 4, W)]], [[rect(H, W, 4, 0, 8, W)]], expect={("inter", (0, 0, 0)): 0},
                cells={(0, 0, 0): False})


@case("disjoint_word_columns")
def _():
    H, W = 8, 200
    return pack([[rect(H, W, 0, 0, 8, 64)]], [[rect(H, W, 0, 64, 8, 200)]], plan=dict(words=4),
                expect={("inter", (0, 0, 0)): 0}, cells={(0, 0, 0): False})


@case("one_word_overlap")
def _():
    # the windows share word column 1 only, and it is the last column of the detection's window
    H, W = 4, 200
    return pack([[rect(H, W, 0, 10, 4, 100)]], [[rect(H, W, 1, 90, 3, 190)]], plan=dict(words=4),
                expect={("inter", (0, 0, 0)): 2 * 10}, cells={(0, 0, 0): True})


@case("empty_det")
def _():
    H, W = 6, 33
    return pack([[np.zeros((H, W), np.uint8), rect(H, W, 0, 0, 6, 33)]], [[rect(H, W, 1, 1, 5, 30)]],
                expect={("inter", (0, 0, 0)): 0, ("det_area", (0, 0)): 0, ("inter", (0, 1, 0)): 4 * 29},
                cells={(0, 0, 0): False})


@case("empty_gt")
def _():
    H, W = 6, 33
    return pack([[rect(H, W, 0, 0, 6, 33)]], [[np.zeros((H, W), np.uint8), rect(H, W, 0, 0, 1, 1)]],
                expect={("inter", (0, 0, 0)): 0, ("gt_area", (0, 0)): 0, ("inter", (0, 0, 1)): 1},
                cells={(0, 0, 0): False})


@case("nested")
def _():
    H, W = 20, 150
    return pack([[rect(H, W, 2, 3, 18, 140), rect(H, W, 5, 70, 9, 80)]],
                [[rect(H, W, 5, 70, 9, 80), rect(H, W, 2, 3, 18, 140)]],
                expect={("inter", (0, 0, 0)): 40, ("inter", (0, 1, 1)): 40, ("inter", (0, 0, 1)): 16 * 137})


# ----------------------------------------------------------------------- pairs
@case("labels_differ")
def _():
    H, W = 5, 20
    full = np.ones((H, W), np.uint8)
    return pack([[full, full]], [[full, full]], det_labels=[[1, 2]], det_count=[2], gt_labels=[[2, 1]], n_class=3,
                expect={("inter", (0, 0, 0)): 0, ("inter", (0, 0, 1)): 100, ("inter", (0, 1, 0)): 100,
                        ("inter", (0, 1, 1)): 0}, cells={(0, 0, 0): False})


@case("labels_outside")
def _():
    H, W = 5, 20
    full = np.ones((H, W), np.uint8)
    # label 0, n_class and beyond, negative: equal on both sides and still no pair; the areas are counted
    return pack([[full] * 5], [[full] * 5], det_labels=[[0, 3, 7, -1, 2]], det_count=[5],
                gt_labels=[[0, 3, 7, -1, 2]], n_class=3,
                expect={**{("inter", (0, d, g)): (100 if d == g == 4 else 0) for d in range(5) for g in range(5)},
                        **{("det_area", (0, d)): 100 for d in range(5)}})


@case("count_zero")
def _():
    H, W = 4, 18
    return pack(list(random_masks(300, 2, 3, H, W)), list(random_masks(301, 2, 2, H, W)), det_count=[0, 3],
                expect={("det_area", (0, 0)): 0, ("inter", (0, 2, 1)): 0})


@case("count_below_d_junk")
def _():
    # the masks at and beyond det_count hold junk; nothing of it may reach an output
    H, W = 6, 40
    d = random_masks(302, 2, 4, H, W)
    d[0, 2:] = 255
    d[1, 1:] = np.random.default_rng(5).integers(1, 256, (3, H, W), dtype=np.uint8)
    return pack(list(d), list(random_masks(303, 2, 3, H, W)), det_count=[2, 1],
                expect={("det_area", (0, 2)): 0, ("det_area", (0, 3)): 0, ("det_area", (1, 1)): 0,
                        ("inter", (0, 2, 0)): 0, ("inter", (1, 3, 2)): 0})


@case("count_outside_range")
def _():
    H, W = 3, 16
    return pack(list(random_masks(304, 2, 3, H, W)), list(random_masks(305, 2, 2, H, W)), det_count=[-4, 9])


@case("g256_one_class")
def _():
    H, W = 8, 8
    g = random_masks(306, 1, 256, H, W)
    return pack(list(random_masks(307, 1, 2, H, W)), list(g), det_labels=[[1, 1]], det_count=[2],
                gt_labels=np.ones((1, 256), np.int32), n_class=2, plan=dict(words=1, edges=1, pack_blocks=258))


@case("d101")
def _():
    H, W = 8, 24
    return pack(list(random_masks(308, 1, 101, H, W)), list(random_masks(309, 1, 3, H, W)),
                plan=dict(pack_blocks=104, pair_blocks=101))


@case("more_gt_than_waves_and_fewer")
def _():
    # a workgroup has four waves: class 1 has nine gt (every wave claims again), class 2 has two
    H, W = 8, 24
    gl = [[1] * 9 + [2] * 2 + [-1]]
    return pack(list(random_masks(310, 1, 3, H, W, 0.8)), list(random_masks(311, 1, 12, H, W, 0.8)),
                det_labels=[[1, 2, 1]], det_count=[3], gt_labels=gl, n_class=3)


@case("labels_omitted_all_pairs")
def _():
    H, W = 8, 24
    full = np.ones((H, W), np.uint8)
    return pack([[full, full], [full, full]], [[full] * 3, [full] * 3], det_count=[2, 1],
                expect={**{("inter", (0, d, g)): 192 for d in range(2) for g in range(3)},
                        ("inter", (1, 0, 0)): 192, ("inter", (1, 1, 0)): 0})


def junk_zeroed(c):
    """The case with the masks at and beyond det_count zeroed."""
    out = dict(c, det_masks=c["det_masks"].copy())
    D = out["det_masks"].shape[1]
    for n, k in enumerate(np.clip(c["det_count"], 0, D)):
        out["det_masks"][n, k:] = 0
    return out
