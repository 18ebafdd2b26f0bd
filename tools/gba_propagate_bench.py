#!/usr/bin/env python3
"""Timings of plvi_gba_walk_device and plvi_gba_correct_device on the GPU (profiles/r25/gba_propagate.txt).

The map is the size of DESIGN.md section 21: 2000 keyframes, 120 000 MapPoints, 30 000 MapLines.  Three spanning
trees: a pure chain (the walk's worst case: one dependent step per keyframe), the chain with a side branch of three
keyframes at every tenth keyframe, and a random recursive tree.  The solver has seen every fourth keyframe and 40 % of
the features; a feature's reference keyframe is drawn uniformly.

The first call of every configuration is compared with the host restatement (tests/native/gba_propagate_ref.cpp),
every output.  Then HIP events around `--calls` back-to-back calls after a warm-up, `--windows` times.  Repeated walks
find every child stamped: the same loads, scans and atomics, only the stamp store is missing.  The restatement's own
time on one host thread is printed beside the walk's.

    python tools/gba_propagate_bench.py [--out FILE] [--calls 100] [--windows 5] [--small]
"""
import argparse
import collections
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pl-vi-orbslam3_amd"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

import plvi  # noqa: E402
import test_gba_propagate as tg  # noqa: E402
from fuse_bench import Events  # noqa: E402

HBM_GBS = 8000.0  # MI355X peak, GB/s


def trees(K, rng):
    stamped = range(0, K, 4)
    order = rng.permutation(K)
    yield "chain", tg.forest(K, {s: [s + 1] for s in range(K - 1)}, stamped=stamped, order=order)
    main = [s for s in range(K) if s % 13 < 10]          # ten on the trunk, then a branch of three off the tenth
    ch = collections.defaultdict(list)
    for a, b in zip(main, main[1:]):
        ch[a].append(b)
    for s in range(K):
        if s % 13 >= 10:
            ch[s - 1].append(s)
    yield "chain with a side branch every tenth keyframe", tg.forest(K, ch, stamped=stamped, order=order)
    yield "random recursive tree", tg.random_tree(K, 9, stamped=stamped, order=order)


def stats(say, t, calls):
    say(f"  median {np.median(t):.1f} us, min {min(t):.1f} us, max {max(t):.1f} us per call  "
        f"[{' / '.join(f'{v:.1f}' for v in t)}] ({calls} calls per window)")


def bench_walk(ev, say, name, kf, calls, windows):
    K = len(kf["bad"])
    g = tg.propagation(kf)
    step, fetch = g.walk.batch([0], tg.LOOP, fill=tg.FILL, run=False)
    assert step() == 0
    sec = []
    want = tg.ref_walk(kf, [0], seconds=sec)
    r = fetch()
    tg.same_walk(r, want)
    for _ in range(3):
        step()
    t = [ev.time(step, calls) * 1e3 for _ in range(windows)]
    depth = np.zeros(K, np.int64)
    for s, p in zip(want["walk"][:K], want["walk_parent"][:K]):
        depth[s] = depth[p] + 1 if p >= 0 else 0
    say(f"walk, {name}: {K} keyframes, {want['n_walk']} walked, {want['n_new']} new, depth {int(depth.max())}, widest "
        f"row {int(np.diff(kf['child_off']).max())}: equals the restatement ({sec[0] * 1e6:.0f} us on one host thread)")
    stats(say, t, calls)


def bench_correct(ev, say, kind, n, K, calls, windows):
    name = "lines" if kind == tg.LINES else "points"
    m = tg.feature_map(kind, n, K=K, seed=12)
    m["poses"]["kf_ba_for"][:] = tg.LOOP
    m["poses"]["kf_ba_for"][np.arange(K) % 50 == 7] = tg.OLD
    m["poses"]["has_bef"][:] = 1
    kf = dict(bad=m["kf_bad"], kf_ba_for=m["poses"]["kf_ba_for"])
    for compat in (0, tg.FMA):
        g = tg.propagation(kf, m)
        step, fetch = g.correct.batch(kind, tg.LOOP, m["poses"], map=m["map"], compat=compat, fill=tg.FILL, run=False)
        assert step() == 0
        sec = []
        want = tg.ref_correct(m, compat, seconds=sec)
        tg.same_correct(fetch(), want, tg.col_of(m))
        for _ in range(3):
            step()
        t = [ev.time(step, calls) * 1e3 for _ in range(windows)]
        c = want["counts"]
        row = 48 if kind == tg.LINES else 12
        # per feature: bad, map_id, the stamp and state; a row in and a row out where written; ref_kf, the keyframe's
        # stamp and flag where the reference keyframe decides.  The 96 bytes of the two poses come out of the cache.
        moved = n * (1 + 4 + 4 + 1) + int(c[1]) * 2 * row + (n - int(c[1])) * (4 + 4 + 1) + int(c[2]) * 2 * row
        say(f"correct, {name}, compat {compat}: pool {n}, states {c.tolist()}: equals the restatement "
            f"({sec[0] * 1e6:.0f} us on one host thread, for context)")
        stats(say, t, calls)
        gbs = moved / (np.median(t) * 1e-6) / 1e9
        say(f"  {moved / n:.1f} bytes a feature, {gbs:.0f} GB/s: {100 * gbs / HBM_GBS:.1f} % of {HBM_GBS:.0f} GB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--lines", type=int, default=30000)
    ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    if plvi.load().plvi_device_count() <= 0:
        sys.exit("gba_propagate_bench: no HIP device (there is no CPU fallback)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ev = Events()
    say(f"library: {plvi.LIB_PATH.parent.name}/{plvi.LIB_PATH.name}")
    K = 130 if a.small else a.keyframes
    for name, kf in trees(K, np.random.default_rng(5)):
        bench_walk(ev, say, name, kf, a.calls, a.windows)
    bench_correct(ev, say, tg.POINTS, 1200 if a.small else a.points, K, a.calls, a.windows)
    bench_correct(ev, say, tg.LINES, 300 if a.small else a.lines, K, a.calls, a.windows)
    say("")
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
