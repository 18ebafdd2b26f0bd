#!/usr/bin/env python3
"""Timings of plvi_ba_window_batch on the GPU (profiles/r20/ba_window.txt).

The map is the shape of DESIGN.md section 21, built as tools/cull_bench.py builds it: K resident keyframes along a
trajectory, each with `--kp-cap` keypoint slots of which a quarter hold a MapPoint seen from a handful of keyframes
around the one that created it; for PLVI_BA_LINES a quarter as many MapLines in 300 slots.  A query's row is its 100
nearest keyframes; the temporal chain is the slot order.

The first call is compared with the host restatement (tests/native/ba_window_ref.cpp), every query of a batch of up to
two, the first two of a larger one.  Then HIP events around `--calls` back-to-back calls after a warm-up, `--windows`
times.  The restatement's own time for one query on one host thread (objects already built) is printed for context
only.

    python tools/ba_window_bench.py [--out FILE] [--calls 200] [--windows 5] [--small] [--queries 1,64]
                                    [--modes points,lines,inertial]
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
import test_ba_window as tb  # noqa: E402
from cull_bench import N_CAND, pool_of  # noqa: E402
from fuse_bench import Events  # noqa: E402

MODES = {"points": tb.POINTS, "lines": tb.LINES, "inertial": tb.INERTIAL}


def session(rng, K, cap, lines, queries):
    kf = dict(bad=(rng.random(K) < 0.02).astype(np.uint8), init_kf=np.zeros(K, np.uint8),
              kf_id=np.arange(1, K + 1, dtype=np.uint32), prev_kf=np.arange(-1, K - 1, dtype=np.int32))
    tab, info, pool, _ = pool_of(rng, K, cap, K * (cap // 4) // 5)
    info = ((info & 1) << 7).astype(np.uint8)      # about half the observations are stereo
    if lines:
        kf.update(ml=tab, nml=np.full(K, cap, np.int32))
    else:
        kf.update(mp=tab, nmp=np.full(K, cap, np.int32), kp_info=info)
    cand = np.zeros((K, 128), np.int32)
    n_cand = np.zeros(K, np.int32)
    for q in queries:
        near = sorted((s for s in range(max(0, q - 60), min(K, q + 61)) if s != q), key=lambda s: (abs(s - q), s))
        cand[q, :N_CAND] = near[:N_CAND]
        n_cand[q] = N_CAND
        kf["bad"][q] = 0
    kf.update(cand=cand, n_cand=n_cand)
    pool["map_id"] = np.zeros(len(pool["bad"]), np.int32)
    return kf, pool, np.zeros(K, np.int32)


def bench(ev, say, name, K, cap, B, calls, windows):
    mode = MODES[name]
    rng = np.random.default_rng(5)
    queries = np.linspace(100, K - 101, B).astype(int).tolist() if B > 1 else [K // 2]
    tabs = session(rng, K, cap, mode == tb.LINES, queries)
    caps = dict(lkf_cap=128, fkf_cap=K + 2, feat_cap=len(tabs[1]["bad"]), edge_cap=len(tabs[1]["obs_kf"]))
    if B > 1:    # what a window of this map needs, not the whole map per query
        caps.update(feat_cap=min(caps["feat_cap"], 20000), edge_cap=min(caps["edge_cap"], 100000))
    win = tb.window(tabs, mode, max_opt=25)
    step, fetch = win.batch(queries, K, fill=tb.FILL, run=False, **caps)
    assert step() == 0
    r = fetch()
    assert (r["err"] == 0).all(), r["err"]
    host_us = []
    for i, q in enumerate(queries[:2]):
        sec = []
        want = tb.ref_window(tabs, mode, q, K, max_opt=25, caps=caps, seconds=sec)
        assert tb.plain(r, i) == want, q
        host_us.append(sec[0] * 1e6)
    for _ in range(3):
        step()
    t = [ev.time(step, calls) * 1e3 for _ in range(windows)]
    again = fetch()
    assert all(np.array_equal(again[k], r[k]) for k in tb.SCALARS + tuple(tb.LISTS))
    n_edges = r["n_mono"] + r["n_stereo"] + r["n_line"]
    say(f"{name}: {K} keyframes x {cap} slots, pool {len(tabs[1]['bad'])}, {B} quer{'y' if B == 1 else 'ies'}: "
        f"{r['n_local_kf'].mean():.0f} local + {r['n_fixed_kf'].mean():.0f} fixed keyframes, "
        f"{r['n_local_feat'].mean():.0f} features, {n_edges.mean():.0f} edges a query: equals the restatement "
        f"({np.median(host_us):.0f} us a query on one host thread, for context)")
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
    ap.add_argument("--queries", default="1,64")
    ap.add_argument("--modes", default="points,lines,inertial")
    ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    if plvi.load().plvi_device_count() <= 0:
        sys.exit("ba_window_bench: no HIP device (there is no CPU fallback)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ev = Events()
    say(f"library: {plvi.LIB_PATH.parent.name}/{plvi.LIB_PATH.name}")
    for name in a.modes.split(","):
        K = 300 if a.small else a.keyframes
        cap = (16 if name == "lines" else 64) if a.small else (a.kl_cap if name == "lines" else a.kp_cap)
        for B in ([1, 3] if a.small else [int(x) for x in a.queries.split(",")]):
            bench(ev, say, name, K, cap, B, a.calls, a.windows)
    say("")
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
