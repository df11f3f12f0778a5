"""CPU-side checks of the evaluation stage: the C-ABI boundary (no compute, no
GPU), hand-derived known answers for the numpy restatement of the contract
(tests/eval_ref.py), its generator, and the loader's difficult flags."""
import ctypes
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import eval_ref  # noqa: E402
from replication_faster_rcnn_amd import data  # noqa: E402

SYMBOLS = ("frcnn_eval_update", "frcnn_eval_ap_workspace_size", "frcnn_eval_ap")


def test_header_and_library_have_eval():
    from replication_faster_rcnn_amd import _lib
    raw = open(os.path.join(ROOT, "include", "frcnn_capi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES
    # each declaration's comment cites the empty test_eval.py and the contract
    assert raw.count("test_eval.py") >= 3 and raw.count('DESIGN.md "Evaluation"') >= 2


def _update(lib, N=2, M=64, G=8, C=21, cap=1000, null=None, thr=0.5):
    """frcnn_eval_update with dummy non-null pointers: every case here is
    rejected before any pointer is used or any HIP call is made."""
    d = ctypes.c_void_p(0x1000)
    p = dict(det_boxes=d, det_labels=d, det_scores=d, det_count=d, gt_boxes=d, gt_labels=d, gt_difficult=d,
             hdr=d, rec_key=d, rec_flag=d, rec_image=d)
    if null:
        p[null] = None
    return lib.frcnn_eval_update(N, M, G, C, cap, p["det_boxes"], p["det_labels"], p["det_scores"], p["det_count"],
                                 p["gt_boxes"], p["gt_labels"], p["gt_difficult"], thr, 1, p["hdr"], p["rec_key"],
                                 p["rec_flag"], p["rec_image"], None)


def _ap(lib, C=21, n=100, null=None, ws=None, ws_bytes=1 << 40):
    d = ctypes.c_void_p(0x1000)
    p = dict(hdr=d, rec_key=d, rec_flag=d, ap=d, map=d)
    if null:
        p[null] = None
    return lib.frcnn_eval_ap(C, n, p["hdr"], p["rec_key"], p["rec_flag"], 0, p["ap"], p["map"], None,
                             d if ws is None else ws, ws_bytes, None)


def test_eval_argument_validation_without_gpu():
    from replication_faster_rcnn_amd import _lib
    lib = _lib.load(require_gpu=False)
    for kw, word in [(dict(N=0), b"N="), (dict(N=1025), b"N="), (dict(M=0), b"M="), (dict(M=(1 << 20) + 1), b"M="),
                     (dict(G=-1), b"G="), (dict(G=257), b"G="), (dict(C=1), b"C="), (dict(C=129), b"C="),
                     (dict(cap=0), b"cap="), (dict(cap=(1 << 24) + 1), b"cap="), (dict(thr=float("nan")), b"iou_thresh"),
                     (dict(null="det_scores"), b"det_scores"), (dict(null="gt_boxes"), b"gt_boxes"),
                     (dict(null="rec_flag"), b"rec_flag"), (dict(null="hdr"), b"hdr")]:
        assert _update(lib, **kw) == -1, kw
        assert word in lib.frcnn_last_error(), (kw, lib.frcnn_last_error())
    for kw, word in [(dict(C=1), b"C="), (dict(C=129), b"C="), (dict(n=-1), b"n_records"),
                     (dict(n=(1 << 24) + 1), b"n_records"), (dict(null="ap"), b"ap"), (dict(null="hdr"), b"hdr"),
                     (dict(null="rec_key"), b"rec_key")]:
        assert _ap(lib, **kw) == -1, kw
        assert word in lib.frcnn_last_error(), (kw, lib.frcnn_last_error())
    need = lib.frcnn_eval_ap_workspace_size(21, 100)
    assert _ap(lib, ws_bytes=need - 1) == -3 and b"workspace" in lib.frcnn_last_error()
    assert _ap(lib, ws=ctypes.c_void_p(0)) == -3


def test_eval_ap_workspace_size():
    from replication_faster_rcnn_amd import _lib
    lib = _lib.load(require_gpu=False)
    size = lib.frcnn_eval_ap_workspace_size
    for bad in [(1, 100), (129, 100), (21, 0), (21, (1 << 24) + 1)]:
        assert size(*bad) == 0, bad
    assert size(21, 100) >= 2 * 100 * 8                  # the sort's two key buffers
    assert size(21, 1 << 20) >= 2 * (1 << 20) * 8 and size(21, 1 << 24) > size(21, 1 << 20)


# ------------------------------------------------------------- known answers
def _run(name):
    case, C, plus_one, flags = eval_ref.known_answers()[name]
    st = eval_ref.State(C, 16)
    st.update(*eval_ref.args(case), plus_one=plus_one)
    n = int(st.hdr[0])
    assert n == len(flags) and st.hdr[1] == 1 and st.hdr[2] == 0
    assert st.rec_flag[:n].tolist() == flags, name
    return case, st


def test_known_tp_fp_tp_fp():
    _, st = _run("tp_fp_tp_fp")
    assert st.hdr[4:].tolist() == [0, 2, 0]
    ap, mean, sk, _ = st.ap()
    assert abs(ap[1] - 5.0 / 6.0) <= 4 * 2.0 ** -52 and np.isnan(ap[0]) and np.isnan(ap[2])   # class 2: no gt
    assert mean == ap[1]
    assert (sk & np.uint64(0xFFFFFF)).tolist() == [0, 1, 2, 3] and (sk >> np.uint64(56)).tolist() == [1] * 4
    ap07 = st.ap(use_07_metric=True)[0]
    assert abs(ap07[1] - 28.0 / 33.0) <= 11 * 2.0 ** -53 and np.isnan(ap07[2])


def test_known_iou_at_threshold_is_fp():
    case, _ = _run("at_threshold")
    assert eval_ref.iou(case["det_boxes"][0, 0], case["gt_boxes"][0, :1], plus_one=0)[0] == 0.5


def test_known_identical_gt():
    _, st = _run("identical_gt")
    assert st.best[0].tolist() == [0, 0]                 # both matched gt 0; gt 1 is never taken
    assert st.hdr[5] == 2


def test_known_zero_area_is_nan():
    case, _ = _run("zero_area")
    assert np.isnan(eval_ref.iou(case["det_boxes"][0, 0], case["gt_boxes"][0, :1], plus_one=0)[0])


def test_sequential_loop_equals_minimum_claim_key():
    """The devkit loop (eval_ref) against the parallel form the kernel uses: a gt's
    TP is the claimant with the smallest (desc_score_key << 32 | slot)."""
    for seed, shuffle, plus_one in [(1, False, 1), (2, True, 0), (3, True, 1)]:
        c = eval_ref.make_case(3, 64, 8, 5, seed=seed, shuffle=shuffle, levels=4)
        st = eval_ref.State(5, 1000)
        st.update(*eval_ref.args(c), plus_one=plus_one)
        pos = 0
        for n in range(3):
            k = int(c["det_count"][n])
            best, flag = st.best[n], st.rec_flag[pos:pos + k]
            key = (eval_ref.desc_score_key(c["det_scores"][n, :k]).astype(np.uint64) << np.uint64(32)) | \
                np.arange(k, dtype=np.uint64)
            for j in range(8):
                cl = np.nonzero(best == j)[0]
                if len(cl) == 0:
                    continue
                if c["gt_difficult"][n, j]:
                    assert (flag[cl] == -1).all()
                else:
                    want = np.zeros(len(cl), np.int8)
                    want[np.argmin(key[cl])] = 1
                    assert np.array_equal(flag[cl], want)
            assert (flag[best < 0] == 0).all()
            pos += k


def test_generator_shapes_and_garbage():
    c = eval_ref.make_case(2, 40, 6, 4, seed=5, counts=[-3, 45])
    assert c["det_count"].tolist() == [-3, 45]
    assert (c["det_boxes"][0] == np.float32(1e30)).all() and (c["det_scores"][0] == 9).all()
    assert (c["det_labels"][0] == 1).all() and (c["det_scores"][1] <= 1).all()
    assert c["gt_boxes"].dtype == np.float64 and c["gt_labels"].dtype == np.int32 and c["gt_difficult"].dtype == np.uint8
    valid = c["gt_labels"] >= 1
    assert ((c["gt_labels"] == -1) | valid).all() and (c["gt_labels"] < 4).all()
    again = eval_ref.make_case(1, 40, 6, 4, seed=5, first_image=1, counts=[45])
    assert all(np.array_equal(c[k][1:], again[k]) for k in eval_ref.ARGS)


# ---------------------------------------------------------------- the loader
OBJ = "<object><name>%s</name>%s<bndbox><xmin>%s</xmin><ymin>20</ymin><xmax>110</xmax><ymax>220</ymax></bndbox></object>"


def _doc(*objs):
    return data.parse_voc_annotation("<annotation><size><width>500</width></size>%s</annotation>" % "".join(objs))


def test_get_difficult():
    doc = _doc(OBJ % ("dog", "<difficult>0</difficult>", "10"), OBJ % ("cat", "<difficult>1</difficult>", "10"),
               OBJ % ("unicorn", "<difficult>1</difficult>", "10"),      # unknown class: -1 row
               OBJ % ("car", "", "10"),                                 # no difficult tag
               OBJ % ("bus", "<difficult>1</difficult>", "x"))          # unparsable box: -1 row
    d = data.get_difficult(doc)
    labels, _ = data.get_labels(doc, difficult=True)
    assert d.dtype == np.uint8 and d.shape == (32,)
    assert d[:5].tolist() == [0, 1, 0, 0, 0] and d[5:].sum() == 0
    assert (labels[:5] != -1).tolist() == [True, True, False, True, False]
    assert (d[labels == -1] == 0).all()
    assert data.get_difficult(doc, n_obj=2).tolist() == [0, 1]


def test_get_difficult_single_object_quirk():
    doc = _doc(OBJ % ("cat", "<difficult>1</difficult>", "10"))
    labels, _ = data.get_labels(doc, difficult=True)
    assert (labels == -1).all()                          # the reference iterates the dict's keys
    assert data.get_difficult(doc).sum() == 0


def test_load_targets_return_difficult():
    xml = "<annotation>%s%s</annotation>" % (OBJ % ("dog", "<difficult>0</difficult>", "10"),
                                             OBJ % ("cat", "<difficult>1</difficult>", "10"))
    box, label = data.load_targets(xml, (300, 500), difficult=True)
    box3, label3, diff = data.load_targets(xml, (300, 500), difficult=True, return_difficult=True)
    assert np.array_equal(box, box3) and np.array_equal(label, label3)
    assert diff[:2].tolist() == [0, 1] and (label3[:2] != -1).all()
