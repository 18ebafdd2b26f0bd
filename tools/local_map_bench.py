#!/usr/bin/env python3
"""Timings of plvi_local_map_batch on the GPU (profiles/r15/local_map.txt).

The shape is a tracking session's: K resident keyframes along a trajectory, each with `--kp-cap` keypoint slots
of which about a quarter hold a MapPoint; a MapPoint is seen from a handful of keyframes around the one that
created it; every keyframe has its ten nearest in time as covisibles, its predecessor as parent and mPrevKF.  A
frame votes with about `--votes` MapPoints seen around its place on the trajectory, which gives about 80 local
keyframes and a few thousand local points.  The first call is compared with the host restatement
(tests/native/local_map_ref.cpp) output for output; then HIP events around `--calls` back-to-back calls,
`--windows` times.  One call is what plvi_local_map_batch enqueues: two fills and four kernels.  The restatement's
own time for its two Update functions on one host thread (object graph already built) is printed for context only.

    python tools/local_map_bench.py [--out FILE] [--calls 50] [--windows 5] [--small] [--frames 1,64] [--lines]

PLVI_LIB=... selects a variant of the library (tools/build_variant.sh).  The map builder and the restatement are
those of tests/test_local_map.py (tl.Map, tl.ref_frame); the session's shape is set here, by `session`.
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
import test_local_map as tl  # noqa: E402
from fuse_bench import Events  # noqa: E402


def session(rng, K, kp_cap, per_kf, kl_cap, lines_per_kf):
    """A tl.Map of K keyframes; about per_kf MapPoints (lines_per_kf MapLines) in every keyframe's table."""
    n_mp = K * per_kf // 5            # a point is seen from ~5 keyframes
    n_ml = K * lines_per_kf // 5 if kl_cap else 0
    m = tl.Map(K, kp_cap, n_mp, kl_cap, n_ml, imu=True)
    m.order = rng.permutation(K).tolist()
    m.bad[:] = rng.random(K) < 0.02
    for s in range(K):
        near = [s + d for d in (1, -1, 2, -2, 3, -3, 4, -4, 5, -5) if 0 <= s + d < K]
        m.covis[s, :len(near)] = near
        if s:
            m.tree(s - 1, s)
    m.prev[1:] = np.arange(K - 1)
    for n, obs, tab, cnt, cap, bad in ((n_mp, m.mp_obs, m.kf_mp, m.nmp, kp_cap, m.mp_bad),
                                       (n_ml, m.ml_obs, m.kf_ml, m.nml, kl_cap, m.ml_bad)):
        if not n:
            continue
        bad[:] = rng.random(n) < 0.02
        slots = [rng.permutation(cap) for _ in range(K)]   # a keyframe's features sit at scattered indices
        used = np.zeros(K, np.int64)
        centre = np.sort(rng.integers(0, K, n))
        for i in range(n):
            kfs = np.unique(np.clip(centre[i] + rng.integers(-12, 13, 1 + rng.geometric(0.2)), 0, K - 1))
            obs[i] = kfs.tolist()
            for s in kfs:
                if used[s] < cap:
                    tab[s, slots[s][used[s]]] = i
                    used[s] += 1
        cnt[:] = cap
    m.next_mp, m.next_ml = n_mp, n_ml
    return m


def frames_of(rng, m, B, votes, line_votes):
    by_kf = [[] for _ in range(m.K)]
    for i, o in enumerate(m.mp_obs):
        for s in o:
            by_kf[s].append(i)
    lby = [[] for _ in range(m.K)]
    for i, o in enumerate(m.ml_obs):
        for s in o:
            lby[s].append(i)
    frames = []
    for _ in range(B):
        c = int(rng.integers(20, m.K - 20))
        pick = lambda tabs, n: rng.permutation(np.unique(np.concatenate(  # noqa: E731
            [np.array(tabs[s], np.int64) for s in range(c - 12, c + 13)])))[:n].tolist()
        frames.append(tl.frame(pick(by_kf, votes) + [-1] * 50, vote_ml=pick(lby, line_votes) if m.kl_cap else None,
                               last_kf=c))
    return frames


def bench(ev, say, m, lm, B, votes, line_votes, calls, windows, seed=11):
    rng = np.random.default_rng(seed + B)
    frames = frames_of(rng, m, B, votes, line_votes)
    check = frames[:min(B, 3)]
    refs, host = [], []
    for fr in check:
        refs.append(tl.ref_frame(m, fr))
        host.append(tl.ref_lib().local_map_ref_seconds() * 1e6)
    args = tl.gpu_args(frames)
    n_mp, n_ml = len(m.mp_bad), len(m.ml_bad)
    caps = [256, 8192, 4096 if m.kl_cap else 0]
    step, fetch = lm.update_batch(**args, lkf_cap=caps[0], lmp_cap=caps[1], lml_cap=caps[2], fill=tl.FILL, run=False)
    assert step() == 0
    got = fetch()
    e = tl.expected(lm, m, check, refs, caps)
    for k, want in e.items():
        assert np.array_equal(got[k][:len(check)], want), k
    assert (got["err"] == 0).all(), got["err"]
    for _ in range(3):
        step()
    times = [ev.time(step, calls) * 1e3 for _ in range(windows)]
    say(f"{m.K} keyframes x {m.kp_cap} slots, pools {n_mp} points / {n_ml} lines, B = {B}: "
        f"{np.mean([len(fr['vote_mp']) - 50 for fr in frames]):.0f} voting points"
        f"{'' if not m.kl_cap else ' + %.0f lines' % np.mean([len(fr['vote_ml']) for fr in frames])}, "
        f"{got['n_local_kf'].mean():.0f} local keyframes, {got['n_local_mp'].mean():.0f} local points"
        f"{'' if not m.kl_cap else ', %.0f local lines' % got['n_local_ml'].mean()}; equals the restatement "
        f"({np.mean(host):.0f} us a frame on one host thread, for context)")
    say(f"  median {np.median(times):.1f} us, min {min(times):.1f} us per call  "
        f"[{' / '.join(f'{v:.1f}' for v in times)}] ({calls} calls per window)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--kp-cap", type=int, default=1200)
    ap.add_argument("--votes", type=int, default=1000)
    ap.add_argument("--frames", default="1,64")
    ap.add_argument("--lines", action="store_true", help="the points-and-lines form: 300 keyline slots a keyframe")
    ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    if plvi.load().plvi_device_count() <= 0:
        sys.exit("local_map_bench: no HIP device (there is no CPU fallback)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ev = Events()
    say(f"library: {plvi.LIB_PATH.parent.name}/{plvi.LIB_PATH.name}")
    K, kp_cap, votes = (120, 64, 60) if a.small else (a.keyframes, a.kp_cap, a.votes)
    kl_cap = (16 if a.small else 300) if a.lines else 0
    m = session(np.random.default_rng(5), K, kp_cap, kp_cap // 4, kl_cap, kl_cap // 4)
    lm = plvi.LocalMap(*m.tables())
    for B in ([1, 3] if a.small else [int(x) for x in a.frames.split(",")]):
        bench(ev, say, m, lm, B, votes, votes // 5, a.calls, a.windows)
    say("")
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
