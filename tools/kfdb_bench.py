#!/usr/bin/env python3
"""Timings of plvi_kfdb_query_batch on the GPU (profiles/r13/kfdb.txt).

Per shape: a synthetic trajectory of K keyframes of ~900 words each -- two thirds of a keyframe's words come from a
window of a ring of "scene" words that slides along the trajectory (so neighbours in time share a hundred words or
more, as revisited places do), the rest from the whole vocabulary --, a covisibility table of the ten nearest
keyframes in time, and queries that are perturbed copies of keyframes (a revisit).  The database is filled once;
the first two calls of every variant are compared with the host restatement (tests/native/kfdb_ref.cpp, which
carries the score members from one call to the next as the handle does): word counts, double scores bit for bit,
list order and candidates.  Then HIP events around `--calls` back-to-back calls, `--windows` times.  One call is
what plvi_kfdb_query_batch enqueues: two memsets, (mode 1) the connected-marking kernel, the count, score, carry
and select kernels.  The restatement's own time on one host thread is printed for context only.

    python tools/kfdb_bench.py [--out FILE] [--calls 50] [--windows 5] [--small] [--shapes 500,2000,8000]

PLVI_LIB=... selects a variant of the library (tools/build_variant.sh) for the A/Bs: -DPLVI_KFDB_SINGLE_PASS=1,
-DPLVI_KFDB_LANE_PER_SLOT=1, -DPLVI_KFDB_LANE0_SUM=1, -DPLVI_KFDB_SLOTS_PER_GROUP=n.
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
import test_kfdb as tk  # noqa: E402
from fuse_bench import Events, Tables  # noqa: E402

N_WORDS = 1000000
WORDS = 900


def trajectory(rng, K, n_local=600, window=3000, step=40):
    """K BowVectors (sorted unique words, L1-normalised values) and their 3 maps."""
    ring = max(K * step, window)
    scene = rng.permutation(N_WORDS)[:ring]
    bows = []
    for i in range(K):
        local = scene[(i * step + rng.integers(0, window, n_local)) % ring]
        w = np.unique(np.concatenate([local, rng.integers(0, N_WORDS, WORDS - n_local)])).astype(np.uint32)
        v = rng.random(len(w)) + 0.05
        bows.append((w, v / v.sum()))
    return bows


def perturbed(rng, b, keep=0.7):
    w, _ = b
    kept = w[rng.random(len(w)) < keep]
    w2 = np.unique(np.concatenate([kept, rng.integers(0, N_WORDS, len(w) - len(kept))])).astype(np.uint32)
    v = rng.random(len(w2)) + 0.05
    return w2, v / v.sum()


def bench(ev, say, K, Q, mode, calls, windows, seed=7):
    rng = np.random.default_rng(seed)
    bows = trajectory(rng, K)
    maps = (np.arange(K) * 3 // K).astype(np.int32)
    cap = max(len(b[0]) for b in bows)
    covis = np.full((K, 10), -1, np.int32)
    for s in range(K):
        near = [s + d for d in (1, -1, 2, -2, 3, -3, 4, -4, 5, -5) if 0 <= s + d < K]
        covis[s, :len(near)] = near
    src = rng.integers(0, K, Q)
    queries = [perturbed(rng, bows[int(s)]) for s in src]
    qmaps = [int(maps[s]) for s in src]
    conn = [set(range(max(int(s) - 8, 0), min(int(s) + 9, K))) for s in src] if mode == 1 else None
    bad = [0, 0, 0]

    # the restatement: the first two calls (the second reads the members the first left)
    ref = tk.Case(N_WORDS, K, cap)
    ref.add(*[(s, bows[s], int(maps[s])) for s in range(K)])
    for _ in range(2):
        ref.query(queries, qmaps, mode, n_best=3, connected=conn, covis=covis, bad=bad)
    t0 = time.perf_counter()
    exp, _ = tk.run_host(ref, tk.RefDB)
    host_ms = (time.perf_counter() - t0) * 1e3  # includes the K adds

    db = plvi.KeyFrameDatabase(N_WORDS, K, cap)
    assert db.add_many(list(range(K)), bows, maps) == 0
    t = Tables()
    qw, qv, qn = plvi.pack_bow(queries, cap)
    d_w, d_v, d_n, d_m = t.up(qw), t.up(qv), t.up(qn), t.up(np.array(qmaps, np.int32))
    d_cov, d_bad = t.up(covis), t.up(np.array(bad, np.uint8))
    off = np.zeros(Q + 1, np.int32)
    cs = np.zeros(1, np.int32)
    if conn:
        off[1:] = np.cumsum([len(c) for c in conn])
        cs = np.array([s for c in conn for s in sorted(c)], np.int32)
    d_off, d_cs = t.up(off), t.up(cs)
    o = {k: t.out(4 * Q * n) for k, n in (("words", K), ("order", K), ("norder", 1), ("cand", K), ("ncand", 1),
                                           ("loop", 3), ("nloop", 1), ("merge", 3), ("nmerge", 1))}
    o["score"] = t.out(8 * Q * K)

    def run(stages=True):
        g = lambda k: o[k].ptr if stages else 0  # noqa: E731
        plvi.kfdb_query_batch(db, Q, d_w.ptr, d_v.ptr, d_n.ptr, cap, d_m.ptr, mode, 3, d_off.ptr if conn else 0,
                              d_cs.ptr if conn else 0, d_cov.ptr, d_bad.ptr, 3, g("words"), g("score"), g("order"),
                              g("norder"), o["cand"].ptr, K, o["ncand"].ptr, o["loop"].ptr, o["nloop"].ptr,
                              o["merge"].ptr, o["nmerge"].ptr)

    n_scored = 0
    for call in range(2):
        o["score"].upload(np.full((Q, K), np.nan))
        run()
        plvi.load().plvi_device_synchronize()
        words = o["words"].download(np.zeros((Q, K), np.int32))
        score = o["score"].download(np.zeros((Q, K), np.float64))
        order = o["order"].download(np.zeros((Q, K), np.int32))
        norder = o["norder"].download(np.zeros(Q, np.int32))
        a = o["cand" if mode == 0 else "loop"].download(np.zeros((Q, K if mode == 0 else 3), np.int32))
        na = o["ncand" if mode == 0 else "nloop"].download(np.zeros(Q, np.int32))
        b = o["merge"].download(np.zeros((Q, 3), np.int32))
        nb = o["nmerge"].download(np.zeros(Q, np.int32))
        for q in range(Q):
            e = exp[call * Q + q]
            assert np.array_equal(words[q], e["words"]) and score[q].tobytes() == e["score"].tobytes(), (call, q)
            assert order[q][:norder[q]].tolist() == e["order"], (call, q)
            assert a[q][:na[q]].tolist() == e["a"], (call, q)
            if mode == 1:
                assert b[q][:nb[q]].tolist() == e["b"], (call, q)
            n_scored += int(np.isfinite(e["score"]).sum()) if call == 0 else 0
    for _ in range(3):
        run(False)
    times = [ev.time(lambda: run(False), calls) * 1e3 for _ in range(windows)]
    shared = np.mean([len(e["order"]) for e in exp[:Q]])
    say(f"{K} keyframes x {np.mean([len(b[0]) for b in bows]):.0f} words, {Q} quer{'y' if Q == 1 else 'ies'}, mode "
        f"{mode}: {shared:.0f} sharing and {n_scored / Q:.1f} scored keyframes per query, "
        f"{np.mean([len(e['a']) + len(e['b']) for e in exp[:Q]]):.1f} candidates; equals the restatement "
        f"(two calls: {host_ms:.0f} ms on one host thread with its {K} adds, for context)")
    say(f"  median {np.median(times):.1f} us, min {min(times):.1f} us per call  "
        f"[{' / '.join(f'{v:.1f}' for v in times)}] ({calls} calls per window)")
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--shapes", default="500,2000,8000")
    ap.add_argument("--queries", default="1,64")
    ap.add_argument("--modes", default="0,1")
    ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    lib = plvi.load()
    if lib.plvi_device_count() <= 0:
        sys.exit("kfdb_bench: no HIP device (there is no CPU fallback)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ev = Events()
    say(f"library: {plvi.LIB_PATH.parent.name}/{plvi.LIB_PATH.name}")
    shapes = [60, 150] if a.small else [int(x) for x in a.shapes.split(",")]
    for K in shapes:
        for Q in ([1, 4] if a.small else [int(x) for x in a.queries.split(",")]):
            for mode in [int(x) for x in a.modes.split(",")]:
                bench(ev, say, K, Q, mode, a.calls, a.windows)
        say("")
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
