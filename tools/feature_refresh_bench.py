#!/usr/bin/env python3
"""Timings of plvi_feature_refresh_batch on the GPU (profiles/r24/feature_refresh.txt).

The map is the shape of DESIGN.md section 21, built as tools/cull_bench.py builds it: K resident keyframes along a
trajectory, each with `--kp-cap` keypoint slots of which a quarter hold a MapPoint seen from a handful of keyframes
around the one that created it (lists in ascending slot order); for lines a quarter as many MapLines in 300 slots.
The id lists are one feature, an f24 window's worth (`--window`, 6 800) and the whole pool.

The first call of every configuration is compared with the host restatement (tests/native/feature_refresh_ref.cpp),
every output.  Then HIP events around `--calls` back-to-back calls after a warm-up, `--windows` times.  The
restatement's own time on one host thread (objects built inside it) is printed for context only.

    python tools/feature_refresh_bench.py [--out FILE] [--calls 200] [--windows 5] [--small] [--kinds points,lines]
"""
import argparse
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pl-vi-orbslam3_amd"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

import plvi  # noqa: E402
import test_feature_refresh as tf  # noqa: E402
from cull_bench import pool_of  # noqa: E402
from fuse_bench import Events  # noqa: E402

KINDS = {"points": tf.POINTS, "lines": tf.LINES}
WHAT = {"NORMAL": tf.NORMAL, "DESC": tf.DESC, "NORMAL|DESC": tf.NORMAL | tf.DESC}


def session(rng, K, cap, kind):
    _, info, pool, _ = pool_of(rng, K, cap, K * (cap // 4) // 5)
    n = len(pool["bad"])
    t = np.arange(K, dtype=np.float64)
    ow = np.stack([0.3 * t, 2 * np.sin(t / 40), 0.05 * rng.standard_normal(K)], axis=1).astype(np.float32)
    first = pool["obs_kf"][np.minimum(pool["obs_off"][:-1], len(pool["obs_kf"]) - 1)]
    centre = ow[first].astype(np.float64) + rng.uniform(-6, 6, (n, 3)) + [0, 0, 8]
    kf = dict(bad=(rng.random(K) < 0.02).astype(np.uint8), ow=ow, cnt=np.full(K, cap, np.int32), info=info,
              desc=rng.integers(0, 256, (K, cap, 32), dtype=np.uint8))
    pool.update(ref_kf=first.astype(np.int32), normal=np.full((n, 3), tf.S_NORMAL, np.float32),
                dist=np.full((n, 2), tf.S_DIST, np.float32), desc=np.full((n, 32), tf.S_DESC, np.uint8))
    if kind == tf.LINES:
        pool["sep"] = np.concatenate([centre - 0.4, centre + 0.4], axis=1)
    else:
        pool["pos"] = centre.astype(np.float32)
    scale = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    return kf, pool, scale


def bench(ev, say, name, tabs, n_ids, what, calls, windows):
    kind = KINDS[name]
    n = len(tabs[1]["bad"])
    ids = np.arange(n, dtype=np.int32) if n_ids >= n else \
        (np.arange(n_ids, dtype=np.int32) + (n - n_ids) // 2)        # a contiguous window of the pool, as f24 lists it
    fr = tf.refresher(tabs, kind)
    step, fetch = fr.batch(ids, WHAT[what], fill=tf.FILL, run=False)
    assert step() == 0
    r = fetch()
    sec = []
    want = tf.ref_refresh(tabs, kind, ids, WHAT[what], seconds=sec)
    if not WHAT[what] & tf.DESC:
        want.update(best_pos=r["best_pos"], best_median=r["best_median"])
    tf.same(tf.plain(r), want)
    for _ in range(3):
        step()
    t = [ev.time(step, calls) * 1e3 for _ in range(windows)]
    tf.same(tf.plain(fetch()), want)
    say(f"{name} {what}: {len(ids)} ids of a pool of {n} ({r['n_rows']} rows, {int((r['state'] != 0).sum())} "
        f"refreshed, max_obs {fr.max_obs}): equals the restatement ({sec[0] * 1e6:.0f} us on one host thread, for "
        f"context)")
    say(f"  median {np.median(t):.1f} us, min {min(t):.1f} us, max {max(t):.1f} us per call  "
        f"[{' / '.join(f'{v:.1f}' for v in t)}] ({calls} calls per window)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--kp-cap", type=int, default=1200)
    ap.add_argument("--kl-cap", type=int, default=300)
    ap.add_argument("--window", type=int, default=6800)
    ap.add_argument("--kinds", default="points,lines")
    ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    if plvi.load().plvi_device_count() <= 0:
        sys.exit("feature_refresh_bench: no HIP device (there is no CPU fallback)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ev = Events()
    say(f"library: {plvi.LIB_PATH.parent.name}/{plvi.LIB_PATH.name}")
    for name in a.kinds.split(","):
        K = 100 if a.small else a.keyframes
        cap = (16 if name == "lines" else 64) if a.small else (a.kl_cap if name == "lines" else a.kp_cap)
        tabs = session(np.random.default_rng(5), K, cap, KINDS[name])
        n = len(tabs[1]["bad"])
        say(f"{name}: {K} keyframes x {cap} slots, pool {n}, {tabs[1]['obs_off'][n] / n:.1f} observers a feature")
        for n_ids in sorted({1, min(a.window // (20 if a.small else 1), n), n}):
            for what in WHAT:
                bench(ev, say, name, tabs, n_ids, what, a.calls, a.windows)
    say("")
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
