#!/usr/bin/env python3
"""Timings of plvi_keyframe_culling_batch on the GPU (profiles/r17/cull.txt).

The map is the shape of DESIGN.md section 21: K resident keyframes along a trajectory, each with `--kp-cap` keypoint
slots of which a quarter hold a MapPoint seen from a handful of keyframes around the one that created it (with
--lines a quarter as many MapLines in 300 slots).  A query walks its 100 nearest keyframes.  Left alone no keyframe
of such a map is redundant; `--culls` n makes the candidates at positions 10, 40, 70, ... of every query's list
redundant (their entries with fewer than eight observers are marked "left out by depth", the others get the coarsest
octave), so a pass erases about n keyframes: the candidates after the first of them are recounted by the walk.

The first call is compared with the host restatement (tests/native/cull_ref.cpp) -- every query of a batch of up to
four, the first four of a larger one.  Then HIP events around `--calls` back-to-back calls after a warm-up,
`--windows` times.  The restatement's own time for one walk on one host thread (objects already built) is printed for
context only.

    python tools/cull_bench.py [--out FILE] [--calls 200] [--windows 5] [--small] [--queries 1,64] [--culls 0,1,3]
                               [--lines]

PLVI_LIB=... selects a variant of the library (tools/build_variant.sh NAME "-DPLVI_CULL_SPECULATE=0" is the walk
kernel alone, everything counted in order).
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
import test_cull as tc  # noqa: E402
from fuse_bench import Events  # noqa: E402

N_CAND = 100


def pool_of(rng, K, cap, n):
    """n features, each seen from 1 + geometric keyframes within 12 of its centre, at scattered table indices.
    Returns (table, info, pool dict, observers per feature)."""
    tab = np.full((K, cap), -1, np.int32)
    info = np.zeros((K, cap), np.uint8)
    slots = [rng.permutation(cap) for _ in range(K)]
    used = np.zeros(K, np.int64)
    centre = np.sort(rng.integers(0, K, n))
    off, okf, oidx = np.zeros(n + 1, np.int32), [], []
    for i in range(n):
        kfs = np.unique(np.clip(centre[i] + rng.integers(-12, 13, 1 + rng.geometric(0.2)), 0, K - 1))
        base = int(rng.integers(0, 5))
        for s in kfs:
            if used[s] < cap:
                j = slots[s][used[s]]
                used[s] += 1
                tab[s, j] = i
                info[s, j] = base + int(rng.integers(0, 3))
                okf.append(s)
                oidx.append(j)
        off[i + 1] = len(okf)
    pool = dict(bad=(rng.random(n) < 0.02).astype(np.uint8), obs_off=off, obs_kf=np.array(okf, np.int32),
                obs_idx=np.array(oidx, np.int32))
    return tab, info, pool, np.diff(off)


def make_redundant(tab, info, n_obs, slot):
    """Every counted entry of `slot` is seen by at least seven others at an octave at or below its own + 1."""
    ids = tab[slot]
    few = (ids >= 0) & (n_obs[np.maximum(ids, 0)] < 8)
    info[slot, few] |= tc.DEPTH
    info[slot, ~few] = 63


def session(rng, K, kp_cap, kl_cap, queries, n_culls):
    kf = dict(bad=(rng.random(K) < 0.02).astype(np.uint8), nmp=np.full(K, kp_cap, np.int32))
    kf["mp"], kf["kp_info"], mp, n_obs = pool_of(rng, K, kp_cap, K * (kp_cap // 4) // 5)
    ml = None
    if kl_cap:
        kf["ml"], kf["kl_info"], ml, l_obs = pool_of(rng, K, kl_cap, K * (kl_cap // 4) // 5)
        kf["nml"] = np.full(K, kl_cap, np.int32)
    cand = np.zeros((K, 128), np.int32)
    n_cand = np.zeros(K, np.int32)
    for q in queries:
        near = sorted((s for s in range(max(0, q - 60), min(K, q + 61)) if s != q), key=lambda s: (abs(s - q), s))
        cand[q, :N_CAND] = near[:N_CAND]
        n_cand[q] = N_CAND
        kf["bad"][q] = 0
        for pos in range(10, 10 + 30 * n_culls, 30):
            s = int(cand[q, pos])
            kf["bad"][s] = 0
            make_redundant(kf["mp"], kf["kp_info"], n_obs, s)
            if kl_cap:
                make_redundant(kf["ml"], kf["kl_info"], l_obs, s)
    kf.update(cand=cand, n_cand=n_cand)
    return kf, mp, ml


def bench(ev, say, K, kp_cap, kl_cap, B, n_culls, calls, windows):
    rng = np.random.default_rng(5)
    queries = np.linspace(100, K - 101, B).astype(int).tolist() if B > 1 else [K // 2]
    tabs = session(rng, K, kp_cap, kl_cap, queries, n_culls)
    P = tc.params(0.9, monocular=0)
    c = plvi.KeyFrameCulling(*tabs, **P)
    step, fetch = c.cull_batch(queries, n_kf_in_map=K, out_cap=128, changed_cap=128, run=False)
    assert step() == 0
    r = fetch()
    assert (r["err"] == 0).all() and (r["stop"] == tc.END).all()
    host_us = []
    for i, q in enumerate(queries[:4]):
        extra = {}
        want = tc.ref_walk(tabs, P, tc.query(q, n_kf_in_map=K), 128, 128, extra)
        assert tc.plain({k: r[k][i] for k in tc.PER_Q + tc.PER_C + tc.PER_CH}) == want, q
        host_us.append(extra["seconds"] * 1e6)
    for _ in range(3):
        step()
    t = [ev.time(step, calls) * 1e3 for _ in range(windows)]
    again = fetch()
    assert all(np.array_equal(again[k], r[k]) for k in tc.PER_Q + tc.PER_C + tc.PER_CH)
    say(f"{K} keyframes x {kp_cap} slots" + (f" + {kl_cap} line slots" if kl_cap else "") +
        f", pools {len(tabs[1]['bad'])} points" + (f" / {len(tabs[2]['bad'])} lines" if kl_cap else "") +
        f", {B} quer{'y' if B == 1 else 'ies'} x {N_CAND} candidates, {r['n_changed'].mean():.1f} culls a pass, "
        f"{r['n_mps'][:, :N_CAND].clip(0).mean():.0f} points counted a candidate: equals the restatement "
        f"({np.median(host_us):.0f} us a walk on one host thread, for context)")
    say(f"  median {np.median(t):.1f} us, min {min(t):.1f} us per call  [{' / '.join(f'{v:.1f}' for v in t)}] "
        f"({calls} calls per window)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--kp-cap", type=int, default=1200)
    ap.add_argument("--queries", default="1,64")
    ap.add_argument("--culls", default="0,1,3")
    ap.add_argument("--lines", action="store_true", help="KeyFrameCullingWithLines: 300 keyline slots a keyframe")
    ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    if plvi.load().plvi_device_count() <= 0:
        sys.exit("cull_bench: no HIP device (there is no CPU fallback)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ev = Events()
    say(f"library: {plvi.LIB_PATH.parent.name}/{plvi.LIB_PATH.name}")
    K, kp_cap = (300, 64) if a.small else (a.keyframes, a.kp_cap)
    kl_cap = (16 if a.small else 300) if a.lines else 0
    for B in ([1, 3] if a.small else [int(x) for x in a.queries.split(",")]):
        for n_culls in [int(x) for x in a.culls.split(",")]:
            bench(ev, say, K, kp_cap, kl_cap, B, n_culls, a.calls, a.windows)
    say("")
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
