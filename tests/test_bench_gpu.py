"""bench.py on the GPU at a tiny batch: a plain run does only the timed steps
(no --full fields in its line), --steps sets the number of timed steps, and
--dump-outputs writes the last timed step's tables -- compared here, frame by
frame and pair by pair, with the oracle on the same frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
import plvi
from conftest import ROOT
from plvi import dist as pdist
from plvi import synth

pytestmark = pytest.mark.gpu

B, W, H = 4, 640, 480
FULL_ONLY = ("oracle_check", "cpu_baseline", "roofline", "roofline_pyramid", "roofline_lsd_prep", "roofline_lbd",
             "stage_ms", "part_fps", "side_ms", "batch64", "batch64_in_flight", "single_frame_latency",
             "h2d_overlapped")


def _f64(rec):
    return np.stack([rec[f].astype(np.float64) for f in rec.dtype.names], -1)


def test_plain_run_dumps_the_last_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", str(B), "--dump-outputs", str(tmp_path)], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["n_gpus"] == 1 and out["full"] is False
    assert out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"] == "u8"
    assert out["ms_per_step"] > 0
    # value and ms_per_step describe the same 3 timed steps of B frames
    assert out["value"] == pytest.approx(B / (out["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in out]
    assert out["device_errors"] == {"orb": 0, "lines": 0}

    d = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert sum(a.nbytes for a in d.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert d["frames"].tolist() == [0.0, 1.0, 2.0, 3.0]  # B <= 64: every frame of the batch

    # the dumped step's frames, regenerated as the bench generates them (two
    # windows of B frames for its two batches in flight)
    import torch
    lo = out["dump_outputs"]["first_frame"]
    seq = synth.device_sequence(2 * B, W, H, seed=pdist.shard_seed(0), device="cuda:0")
    frames = seq[lo:lo + B].cpu().numpy()
    torch.cuda.synchronize()
    prev = None
    for f in range(B):
        mono, k, de = ol.orb_extract(frames[f])
        kl, ld, fn = ol.line_extract(frames[f])
        n, nl = len(k), len(kl)
        assert n > 300 and nl > 20
        assert d["orb_count"][f] == n and d["orb_mono_count"][f] == mono and d["line_count"][f] == nl
        np.testing.assert_array_equal(d["orb_keypoints"][f, :n], _f64(k.astype(plvi.KEYPOINT_DTYPE)))
        np.testing.assert_array_equal(d["orb_descriptors"][f, :n], de.astype(np.float32))
        np.testing.assert_array_equal(d["keylines"][f, :nl], _f64(kl.astype(plvi.KEYLINE_DTYPE)))
        np.testing.assert_array_equal(d["line_descriptors"][f, :nl], ld.astype(np.float32))
        np.testing.assert_array_equal(d["line_functions"][f, :nl], fn)
        # rows past a frame's count are written as zeros
        assert not d["orb_keypoints"][f, n:].any() and not d["orb_descriptors"][f, n:].any()
        assert not d["keylines"][f, nl:].any() and not d["line_descriptors"][f, nl:].any()
        if prev is not None:
            for name, e in zip(("orb_knn_idx0", "orb_knn_dist0", "orb_knn_idx1", "orb_knn_dist1"),
                               ol.knn2(de, prev[0])):
                np.testing.assert_array_equal(d[name][f, :n], e.astype(np.float64))
            nm, m12 = ol.match(ld, prev[1], 0.9)
            assert d["line_match_count"][f - 1] == nm
            np.testing.assert_array_equal(d["line_matches"][f, :nl], m12.astype(np.float64))
        prev = (de, ld)
