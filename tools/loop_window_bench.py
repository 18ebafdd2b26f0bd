#!/usr/bin/env python3
"""Timings of plvi_loop_window_batch and plvi_loop_bow_merge_batch on the GPU (profiles/r21/loop_window.txt).

The map is the shape of DESIGN.md section 21, built as tools/cull_bench.py builds it: K resident keyframes along a
trajectory, each with `--kp-cap` keypoint slots of which a quarter hold a MapPoint seen from a handful of keyframes
around the one that created it.  Every keyframe's covisible row is its 10 nearest keyframes, nearest first, so a LAST
window has 31 entries of which about a dozen are distinct.  PROJ and LAST run with all four gathers.  The merge takes
six tables per query in which one entry in eight names a slot of the member's table (SearchByBoW matches a minority of
the keypoints).

The first call is compared with the host restatement (tests/native/loop_window_ref.cpp), every query of a batch of up
to two, the first two of a larger one.  Then HIP events around `--calls` back-to-back calls after a warm-up,
`--windows` times.  The restatement's own time for one query on one host thread (objects already built) is printed for
context only.

    python tools/loop_window_bench.py [--out FILE] [--calls 200] [--windows 5] [--small] [--queries 1,12]
                                      [--kinds bow,proj,last,merge]
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
import test_loop_window as tl  # noqa: E402
from cull_bench import pool_of  # noqa: E402
from fuse_bench import Events  # noqa: E402

KINDS = {"bow": tl.BOW, "proj": tl.PROJ, "last": tl.LAST}
GATHER = ("pos", "normal", "dist", "desc")
N_COV = 10


def session(rng, K, cap):
    tab, _, pool, _ = pool_of(rng, K, cap, K * (cap // 4) // 5)
    n = len(pool["bad"])
    kf = dict(bad=(rng.random(K) < 0.02).astype(np.uint8), mp=tab, nmp=np.full(K, cap, np.int32))
    cand = np.zeros((K, 16), np.int32)
    for s in range(K):
        near = sorted((v for v in range(max(0, s - N_COV), min(K, s + N_COV + 1)) if v != s),
                      key=lambda v: (abs(v - s), v))
        cand[s, :N_COV] = near[:N_COV]
    kf.update(cand=cand, n_cand=np.full(K, N_COV, np.int32))
    points = dict(bad=pool["bad"], pos=rng.normal(size=(n, 3)).astype(np.float32),
                  normal=rng.normal(size=(n, 3)).astype(np.float32), dist=rng.uniform(1, 9, (n, 2)).astype(np.float32),
                  desc=rng.integers(0, 256, (n, 32), dtype=np.uint8))
    return kf, points


def report(say, ev, step, calls, windows):
    for _ in range(3):
        step()
    t = [ev.time(step, calls) * 1e3 for _ in range(windows)]
    say(f"  median {np.median(t):.1f} us, min {min(t):.1f} us, max {max(t):.1f} us per call  "
        f"[{' / '.join(f'{v:.1f}' for v in t)}] ({calls} calls per window)")


def bench(ev, say, name, tabs, B, calls, windows, pt_cap):
    kf, points = tabs
    K, cap = kf["mp"].shape
    rng = np.random.default_rng(7)
    slots = np.linspace(100, K - 101, B).astype(int).tolist() if B > 1 else [K // 2]
    kf["bad"][slots] = 0
    cur = 50
    conn = [[int(v) for v in kf["cand"][cur, :N_COV]]] * B      # far from every candidate: nothing aborts
    lw = plvi.LoopWindow(kf, points)
    what = f"{K} keyframes x {cap} slots, pool {len(points['bad'])}, {B} quer{'y' if B == 1 else 'ies'}"
    if name != "merge":
        kind = KINDS[name]
        gather = GATHER if kind != tl.BOW else ()
        step, fetch = lw.batch([kind] * B, slots, cur, conn, pt_cap=pt_cap, gather=gather, fill=tl.FILL, run=False)
        assert step() == 0
        r = fetch()
        assert (r["err"] == 0).all(), r["err"]
        sec = []
        qs = [tl.query(kind, s, cur, conn[0]) for s in slots[:2]]
        for i, (q, e) in enumerate(zip(qs, tl.ref_run(tabs, qs, pt_cap, seconds=sec))):
            assert tl.plain(r, i, q, pt_cap) == {k: e[k] for k in tl.SCALARS + ("win", "pts", "pts_kf")}, q
            tl.rows_equal_pool(r, i, points, e["n_pts"], pt_cap, gather)
        say(f"{name}: {what}: windows of {r['n_win'].mean():.0f}, {r['n_pts'].mean():.0f} points a query: equals the "
            f"restatement ({np.median(sec) * 1e6:.0f} us a query on one host thread, for context)")
        report(say, ev, step, calls, windows)
        return
    m12 = np.where(rng.random((B, tl.BOW_WIN, cap)) < 0.125, rng.integers(0, cap, (B, tl.BOW_WIN, cap)), -1)
    m12 = m12.astype(np.int32)
    w = lw.batch([tl.BOW] * B, slots, cur, conn, pt_cap=1, gather=(), fill=tl.FILL)
    d = w["dev"]
    n1 = np.full(B, cap, np.int32)
    step, fetch = lw.merge_batch(d["win"], d["n_win"], d["abort_at"], m12, n1, fill=tl.FILL, run=False)
    assert step() == 0
    r = fetch()
    sec = []
    qs = [tl.query(tl.BOW, s, cur, conn[0], m12[i], cap) for i, s in enumerate(slots[:2])]
    for i, e in enumerate(tl.ref_run(tabs, qs, 1, seconds=sec)):
        assert int(r["num"][i]) == e["num"]
        assert r["matched_mp"][i].tolist() == e["matched_mp"] and r["matched_kf"][i].tolist() == e["matched_kf"]
    say(f"merge: {what}: 6 tables of {cap}, {r['num'].mean():.0f} distinct points a query: equals the restatement "
        f"({np.median(sec) * 1e6:.0f} us a query on one host thread with its window, for context)")
    report(say, ev, step, calls, windows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--kp-cap", type=int, default=1200)
    ap.add_argument("--queries", default="1,12")
    ap.add_argument("--kinds", default="bow,proj,last,merge")
    ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    if plvi.load().plvi_device_count() <= 0:
        sys.exit("loop_window_bench: no HIP device (there is no CPU fallback)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ev = Events()
    say(f"library: {plvi.LIB_PATH.parent.name}/{plvi.LIB_PATH.name}")
    K, cap = (300, 64) if a.small else (a.keyframes, a.kp_cap)
    tabs = session(np.random.default_rng(5), K, cap)
    for name in a.kinds.split(","):
        for B in ([1, 3] if a.small else [int(x) for x in a.queries.split(",")]):
            bench(ev, say, name, tabs, B, a.calls, a.windows, pt_cap=8192)
    say("")
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
