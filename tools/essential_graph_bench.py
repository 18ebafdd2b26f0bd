#!/usr/bin/env python3
"""Timings of plvi_loop_correct_device, plvi_loop_connections_device and plvi_essential_graph_device on the GPU
(profiles/r23/essential_graph.txt).

The map is the shape of DESIGN.md section 21, built as tools/cull_bench.py builds it: K resident keyframes along a
trajectory, each with `--kp-cap` keypoint slots of which a quarter hold a MapPoint seen from a handful of keyframes
around the one that created it.  For A and C every keyframe's row is its 10 nearest keyframes (weights 300 down to
30, so about a third pass minFeat), the current keyframe's its 30 nearest: a window of 31; every window member has two
loop connections near the loop keyframe, 62 in all, at weights 120 and 99.  Parents, the prev / next chain and a loop
edge every 97 keyframes complete the graph.  B runs on a plvi.Covisibility graph built from the observation lists of
the same map by one update of every keyframe, with the same window.

The first call of each is compared with the host restatement (tests/native/essential_graph_ref.cpp).  Then HIP events
around `--calls` back-to-back calls after a warm-up, `--windows` times.  The restatement's own time for one call on
one host thread (objects already built) is printed for context only.

    python tools/essential_graph_bench.py [--out FILE] [--calls 200] [--windows 5] [--small]
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
import test_essential_graph as te  # noqa: E402
from cull_bench import pool_of  # noqa: E402
from fuse_bench import Events  # noqa: E402

N_COV, N_WIN = 10, 30


def session(rng, K, cap):
    tab, _, pool, _ = pool_of(rng, K, cap, K * (cap // 4) // 5)
    n = len(pool["bad"])
    T = te.make_map(K, kp_cap=cap, kl_cap=0, C=32, n_pts=n, n_lns=0)
    T["mp"][:], T["nmp"][:] = tab, cap
    T["points"]["bad"][:] = pool["bad"]
    T["points"]["ref_kf"][:] = rng.integers(0, K, n)
    cur, loop = K - 60, 40
    for s in range(K):
        m = N_WIN if s == cur else N_COV
        near = sorted((v for v in range(max(0, s - m), min(K, s + m + 1)) if v != s), key=lambda v: (abs(v - s), v))
        for r, v in enumerate(near[:m]):
            te.connect(T, s, v, max(300 - 30 * r, 20), both=False)
    T["parent"][1:] = np.arange(K - 1)
    T["prev_kf"][1:], T["next_kf"][:-1] = np.arange(K - 1), np.arange(1, K)
    for s in range(1, K):
        T["children"][s - 1].append(s)
    for s in range(97, K, 97):
        T["loops"][s].append(s - 90)
        T["loops"][s - 90].append(s)
    T["imu"][:] = 1
    T["init_kf"][0] = 1
    te.finish(T)
    win = np.append(T["cand"][cur, :T["n_cand"][cur]], cur).astype(np.int32)
    lc_kf = np.full((len(win), 8), -1, np.int32)
    n_lc = np.full(len(win), 2, np.int32)
    for p, s in enumerate(win):
        a, b = loop + 2 * p, loop + 2 * p + 1
        te.connect(T, int(s), a, 120, both=False)
        te.connect(T, int(s), b, 99, both=False)
        lc_kf[p, :2] = (a, b)
    lc_kf[len(win) - 1, 0] = loop
    te.finish(T)
    return T, pool, cur, loop, win, lc_kf, n_lc


def report(say, ev, step, calls, windows):
    for _ in range(3):
        step()
    t = [ev.time(step, calls) * 1e3 for _ in range(windows)]
    say(f"  median {np.median(t):.1f} us, min {min(t):.1f} us, max {max(t):.1f} us per call  "
        f"[{' / '.join(f'{v:.1f}' for v in t)}] ({calls} calls per window)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--kp-cap", type=int, default=1200)
    ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    if plvi.load().plvi_device_count() <= 0:
        sys.exit("essential_graph_bench: no HIP device (there is no CPU fallback)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ev = Events()
    say(f"library: {plvi.LIB_PATH.parent.name}/{plvi.LIB_PATH.name}")
    K, cap = (300, 64) if a.small else (a.keyframes, a.kp_cap)
    T, pool, cur, loop, win, lc_kf, n_lc = session(np.random.default_rng(5), K, cap)
    what = f"{K} keyframes x {cap} slots, pool {len(pool['bad'])}, a window of {len(win)}"

    # ---- A: the stamps are reset by nobody, so every call after the first finds its points stamped; the timed
    # calls therefore run on a table without stamps (each call lists every point)
    sec = []
    drop = ("corr_by", "corr_ref")
    exp = te.ref_correct(T, cur, lines=False, drop=drop, seconds=sec)
    g = te.eg_of(T, lines=False, drop=drop)
    step, fetch = g.correct_device(cur, fill=te.FILL, run=False)
    assert step() == 0
    te.assert_same(fetch(), exp, te.CORRECT_KEYS, "A")
    say(f"correct: {what}, {int(exp['n_pts'][0])} points listed: equals the restatement ({sec[0] * 1e6:.0f} us on one "
        "host thread, for context)")
    report(say, ev, step, a.calls, a.windows)

    # ---- C
    g = te.eg_of(T, lines=False)
    for name, mode in (("7DOF", te.D7), ("4DOF", te.D4)):
        sec = []
        exp = te.ref_graph(T, cur, loop, mode, win, lc_kf, n_lc, lines=False, seconds=sec, edge_cap=8 * K)
        step, fetch = g.graph_device(cur, loop, mode, win, None, lc_kf, n_lc, edge_cap=8 * K, fill=te.FILL, run=False)
        assert step() == 0
        te.assert_same(fetch(), exp, te.GRAPH_KEYS, "C " + name)
        say(f"graph {name}: {what}, {int(n_lc.sum())} loop connections: {int(exp['n_vert'][0])} vertices, edges by kind "
            f"{exp['n_edges'].tolist()}: equals the restatement ({sec[0] * 1e6:.0f} us on one host thread, for context)")
        report(say, ev, step, a.calls, a.windows)

    # ---- B
    kf = dict(bad=T["bad"], order=T["order"], mp=T["mp"], nmp=T["nmp"], first_conn=np.zeros(K, np.uint8),
              parent=np.full(K, -1, np.int32))
    pts = dict(bad=pool["bad"], obs_off=pool["obs_off"], obs_kf=pool["obs_kf"])
    cov = plvi.Covisibility(K, 64).set_tables(kf, pts)
    assert cov.update_batch(np.arange(K))["rc"] == 0
    sec = []
    exp = te.ref_connections(kf, pts, [(np.arange(K), None)], win, 32, K, seconds=sec)
    te.ref_lib().covis_ref_destroy(exp.pop("h"))
    step, fetch = plvi.EssentialGraph.connections_device(cov, win, 32, fill=te.FILL, run=False)
    assert step() == 0
    te.assert_same(fetch(), exp, ("lc_kf", "n_lc", "lc_err", "n_counted", "n_conn"), "B")
    say(f"connections: {what}, conn_cap 64, rows of {exp['n_lc'][:len(win)].mean():.1f} on average: equals the "
        f"restatement ({sec[0] * 1e6:.0f} us on one host thread, for context)")
    report(say, ev, step, max(a.calls // 10, 1), a.windows)
    say("")
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
