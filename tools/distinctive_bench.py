#!/usr/bin/env python3
"""Timings of plvi_distinctive_descriptors_batch on the GPU (profiles/r12/distinctive.txt).

Per shape: seeded lists (tests/test_distinctive.seeded: per feature a base descriptor with every bit flipped with
probability 0.12), uploaded once; a warm-up; then HIP events around `--calls` back-to-back launches, `--windows`
times, the variants of one shape alternating inside every window.  The whole batch is compared with the host
restatement (tests/native/distinctive_ref.cpp) in the same run, and the restatement's own time on the host is
printed for context only.  A launch is what one call enqueues: the segment kernel alone when max_obs <= 64, else a
memset node, the LDS kernel and the segment kernel.

The lanes a short list occupies follow max_obs (8, 16, 32 or 64 lanes per feature), so the same lists timed with a
larger max_obs than they need give the A/B of shared waves against one wave per feature.

    python tools/distinctive_bench.py [--out FILE] [--calls 200] [--windows 5] [--only-long] [--small]

PLVI_LIB=... selects a variant of the library (tools/build_variant.sh) for an A/B of the long-list shapes.
"""
import argparse
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pl-vi-orbslam3_amd"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

import plvi  # noqa: E402
import test_distinctive as td  # noqa: E402
from fuse_bench import Events  # noqa: E402


def bench(ev, say, title, counts, seed, variants, calls, windows):
    """variants: (label, max_obs) pairs, all at least the longest list, so every one computes the same answer."""
    pool, off, rows = td.seeded(seed, counts)
    t0 = time.perf_counter()
    _, bp, bm, out = td.ref(pool, off, rows)
    host_ms = (time.perf_counter() - t0) * 1e3
    b = td.Batch(pool, off, rows)
    runs = []
    for label, max_obs in variants:
        run = lambda m=max_obs: b.call(m)  # noqa: E731
        b.fill()
        for _ in range(3):
            run()
        gbp, gbm, gout = b.read()
        assert np.array_equal(gbp, bp) and np.array_equal(gbm, bm) and np.array_equal(gout, out), (title, label)
        runs.append((label, run))
    times = {label: [] for label, _ in runs}
    for _ in range(windows):
        for label, run in runs:
            times[label].append(ev.time(run, calls) * 1e3)
    n = np.asarray(counts)
    say(f"{title}: {len(n)} features, {int(n.sum())} observations, N {int(n.min())}..{int(n.max())}; "
        f"host restatement {host_ms:.2f} ms (one thread, for context); every variant equals it")
    for label, _ in runs:
        t = times[label]
        say(f"  {label}: median {np.median(t):.1f} us, min {min(t):.1f} us per launch  "
            f"[{' / '.join(f'{v:.1f}' for v in t)}] ({calls} launches per window)")
    say("")
    return {label: float(np.median(times[label])) for label, _ in runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--only-long", action="store_true", help="only the shapes with a long list (A/B of library variants)")
    ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    lib = plvi.load()
    if lib.plvi_device_count() <= 0:
        sys.exit("distinctive_bench: no HIP device (there is no CPU fallback)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ev = Events()
    rng = np.random.default_rng(2024)
    k = 20 if a.small else 1
    shared = [("max_obs 30, 32 lanes per feature (two features share a wave)", 30),
              ("max_obs 64, one wave per feature", 64)]
    if not a.only_long:
        short_shapes(ev, say, rng, k, shared, a)
    long_shapes(ev, say, k, a)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text("\n".join(lines) + "\n")


def short_shapes(ev, say, rng, k, shared, a):
    bench(ev, say, "keyframe points after SearchInNeighbors", rng.integers(2, 31, 1000 // k), 1, shared, a.calls,
          a.windows)
    bench(ev, say, "keyframe lines", rng.integers(2, 21, 200 // k), 2,
          [("max_obs 20, 32 lanes per feature", 20), ("max_obs 64, one wave per feature", 64)], a.calls, a.windows)
    bench(ev, say, "loop closing / map initialization refresh", rng.integers(2, 31, 8000 // k), 3, shared, a.calls,
          a.windows)
    bench(ev, say, "very short lists (segment sizes)", rng.integers(2, 9, 8000 // k), 4,
          [(f"max_obs {m}, {max(m, 8)} lanes per feature", m) for m in (8, 16, 32, 64)], a.calls, a.windows)


def long_shapes(ev, say, k, a):
    """The imbalance case: what one long list costs a launch of short ones."""
    say(f"library: {plvi.LIB_PATH.parent.name}/{plvi.LIB_PATH.name}")
    long_n = 200 if a.small else 1448
    short = np.full(1000 // k, 10)
    t_short = bench(ev, say, "1000 features of N = 10", short, 5,
                    [("max_obs 10, 16 lanes per feature", 10), ("max_obs 64, one wave per feature", 64),
                     (f"max_obs {long_n}: memset + LDS kernel (every workgroup exits) + segment kernel", long_n)],
                    a.calls, a.windows)
    t_both = bench(ev, say, f"1000 features of N = 10 plus one of N = {long_n}", np.append(short, long_n), 5,
                   [(f"max_obs {long_n}", long_n)], max(a.calls // 4, 5), a.windows)
    t_long = bench(ev, say, f"one feature of N = {long_n} alone", np.array([long_n]), 6,
                   [(f"max_obs {long_n}", long_n)], max(a.calls // 4, 5), a.windows)
    ts = list(t_short.values())
    say(f"imbalance: short lists alone {ts[0]:.1f} us (their own max_obs) / {ts[2]:.1f} us (max_obs {long_n}); "
        f"with the long list {list(t_both.values())[0]:.1f} us; the long list alone {list(t_long.values())[0]:.1f} us")
    bench(ev, say, "one feature of N = 300 alone", np.array([300 // k]), 7, [("max_obs = N", 300 // k)],
          max(a.calls // 4, 5), a.windows)


if __name__ == "__main__":
    main()
