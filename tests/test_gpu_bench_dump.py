"""bench.py as a plain run (no --full) with --dump-outputs: --steps sets the
number of timed steps, the record carries the headline and ms_per_step and
nothing that takes a run of its own, and the dumped arrays are what the last
timed step computed -- compared with the oracle's proposal layer -> RoI
transform -> roi_pool on that step's input set (the sampled arrays at the same
seeded flat indices)."""
import json
import sys

import numpy as np
import pytest

import bench
from oracle import ref_numpy as orc
from replication_faster_rcnn_amd import synth

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_last_step(monkeypatch, capsys, tmp_path):
    steps, warmup, n_sets = 3, 2, 2
    out = tmp_path / "dump"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                                      "--input-sets", str(n_sets), "--dump-outputs", str(out)])
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["steps"] == steps and rec["warmup"] == warmup and rec["n_gpus"] == 1
    assert rec["unit"] == "images/sec" and rec["higher_is_better"] is True and rec["dtype"] == "fp32"
    assert rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(rec["config"]["global_batch"] / (rec["ms_per_step"] * 1e-3), rel=1e-9)
    assert rec["roofline"] is None and rec["cpu_baseline"] is None   # --full only

    got = {p.stem: np.load(p) for p in out.iterdir()}
    assert set(got) == {"rois", "anchor_idx", "count", "boxes", "pooled", "argmax"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20

    c = synth.CONFIGS["cfg2"]
    N, post, H, W = c["batch"], c["post_nms"], c["feat_h"], c["feat_w"]
    seed = (warmup + steps - 1) % n_sets            # the last step's input set
    anchors = orc.generate_anchors(orc.generate_anchor_base(anchor_scales=c["scales"]), 16, W, H)
    A = len(anchors)
    o_rois = np.zeros((N, post, 4), np.float32)
    for i in range(N):
        r_i, i_i = orc.propose_one(anchors, synth.rpn_scores(A, seed, i), synth.rpn_deltas(A, seed, i),
                                   c["img_w"], c["img_h"], c["pre_nms"], post)
        assert int(got["count"][i]) == len(i_i), i
        assert np.array_equal(got["anchor_idx"][i, :len(i_i)], i_i.astype(np.float32)), i
        o_rois[i, :len(i_i)] = r_i
    assert np.array_equal(got["rois"], o_rois)
    inds = np.repeat(np.arange(N), post).astype(np.float32)
    ob = orc.roi_transform(o_rois.reshape(-1, 4), inds, c["img_h"], c["img_w"], H, W)
    assert np.array_equal(got["boxes"], ob)
    x = np.stack([synth.features(c["C"], H, W, seed, i) for i in range(N)])
    oo, oa = orc.roi_pool_forward(x, ob, 7)
    assert oo.size > bench.DUMP_ELEMS               # written as the seeded sample
    pick = np.sort(np.random.default_rng(0).integers(0, oo.size, bench.DUMP_ELEMS))
    assert np.array_equal(got["pooled"], oo.reshape(-1)[pick])
    assert np.array_equal(got["argmax"], oa.reshape(-1)[pick].astype(np.float32))
