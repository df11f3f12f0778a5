"""Regenerate tests/golden/detect_small.npz (CPU only): the inputs of
``synth.head_outputs(2, 96, 21, 600, 1000, seed=1)`` and ``detect_ref``'s six
outputs at score thresholds 0.05 and 0.7.  Run from the repository root:
``python tests/golden/make_golden_detect.py``."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import detect_ref  # noqa: E402
from replication_faster_rcnn_amd import synth  # noqa: E402

NAMES = ("boxes", "labels", "scores", "roi", "count", "total")
SHAPE = dict(N=2, R=96, C=21, img_h=600, img_w=1000, seed=1)
THRESHOLDS = {"t005": 0.05, "t07": 0.7}

if __name__ == "__main__":
    rois, rcount, cls, reg = synth.head_outputs(**SHAPE)
    out = dict(rois=rois, rcount=rcount, cls=cls, reg=reg)
    for tag, thr in THRESHOLDS.items():
        res = detect_ref.detect(rois, rcount, cls, reg, SHAPE["img_h"], SHAPE["img_w"], score_thresh=thr)
        for name, a in zip(NAMES, res):
            out[f"{tag}_{name}"] = a
    np.savez_compressed(os.path.join(HERE, "detect_small.npz"), **out)
