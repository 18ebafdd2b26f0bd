#!/usr/bin/env python3
"""Timings of plvi_covis_update_batch on the GPU (profiles/r16/covis.txt).

The map is the tracking session of tools/local_map_bench.py: K resident keyframes along a trajectory, each with
`--kp-cap` keypoint slots of which a quarter hold a MapPoint seen from a handful of keyframes around the one that
created it, so a keyframe shares points with the twenty-odd keyframes around it.  The queries are keyframes spread
over the trajectory.  The first call on a fresh graph is compared with the host restatement
(tests/native/covis_ref.cpp): per-query outputs, first_conn, parent, the covis table and the state of a sample of
slots.  Then HIP events around `--calls` back-to-back calls, `--windows` times, of two things:

  steady   plvi_covis_update_batch again on the connected graph: every AddConnection finds its weight unchanged
           and no neighbour is re-sorted (CorrectLoop re-running UpdateConnections over a neighbourhood);
  fresh    plvi_covis_erase_batch of the queries followed by plvi_covis_update_batch: every listed neighbour gets
           the query appended and is re-sorted (a new keyframe); the pair is timed, the erase is part of the figure.

The steady call is also captured into a HIP graph and replayed (one launch a call): the difference to the plain
figure is what the host's six enqueues cost.

The restatement's own time for the UpdateConnections calls of the batch on one host thread (object graph already
built) is printed for context only.

    python tools/covis_bench.py [--out FILE] [--calls 1000] [--windows 5] [--small] [--queries 1,64] [--lines]

PLVI_LIB=... selects a variant of the library (tools/build_variant.sh).
"""
import argparse
import ctypes
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pl-vi-orbslam3_amd"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

import plvi  # noqa: E402
import test_covis as tc  # noqa: E402
from fuse_bench import Events  # noqa: E402
from local_map_bench import session  # noqa: E402


def as_cmap(m, conn_cap):
    """The session's tl.Map as the tc.CMap the runners of tests/test_covis.py take."""
    m.__class__ = tc.CMap
    m.map_id = None
    m.init = np.zeros(m.K, np.uint8)
    m.init[m.order[0]] = 1
    m.first = np.ones(m.K, np.uint8)
    m.conn_cap = conn_cap
    return m


def time_on(ev, stream, fn, calls):
    """Milliseconds per call of `calls` back-to-back calls, events recorded on `stream`."""
    ms = ctypes.c_float()
    assert ev.hip.hipEventRecord(ev.a, stream) == 0
    for _ in range(calls):
        fn()
    assert ev.hip.hipEventRecord(ev.b, stream) == 0
    assert ev.hip.hipEventSynchronize(ev.b) == 0
    assert ev.hip.hipEventElapsedTime(ctypes.byref(ms), ev.a, ev.b) == 0
    return ms.value / calls


def bench(ev, say, m, B, calls, windows):
    q = np.linspace(20, m.K - 21, B).astype(np.int32).tolist()
    m.slots = sorted(set(q[:4] + [s + d for s in q[:4] for d in (-3, 1, 7)]))
    ref = tc.RefRunner(m)
    want = ref.run([("update", q)])
    host_us = ref.seconds * 1e6
    g = tc.GpuRunner(m)
    tc.same(g.run([("update", q)]), want)
    step, fetch = g.cov.update_batch(q, run=False)

    def fresh():
        assert g.cov.erase(q) == 0
        assert step() == 0
    for _ in range(3):
        step()
    steady = [ev.time(step, calls) * 1e3 for _ in range(windows)]
    fresh()
    pair = [ev.time(fresh, calls) * 1e3 for _ in range(windows)]
    assert step() == 0
    # the steady call captured once and replayed: one launch a call, so the host's enqueues are off the clock
    lib = plvi.load()
    st = ctypes.c_void_p()
    assert lib.plvi_stream_create(ctypes.byref(st)) == 0
    graph = plvi.StepGraph(lambda s: step(s), st.value)
    for _ in range(3):
        graph.launch()
    replay = [time_on(ev, st, graph.launch, calls) * 1e3 for _ in range(windows)]
    assert lib.plvi_stream_synchronize(st) == 0
    r = fetch()
    assert r["n_counted"].tolist() == want[0]["n_counted"] and (r["err"] == 0).all()
    say(f"{m.K} keyframes x {m.kp_cap} slots, pools {len(m.mp_bad)} points / {len(m.ml_bad)} lines, "
        f"{B} quer{'y' if B == 1 else 'ies'}: counters of {np.mean(want[0]['n_counted']):.0f}, lists of "
        f"{np.mean(want[0]['n_conn']):.0f}; equals the restatement ({host_us:.0f} us for the batch on one host "
        f"thread, for context)")
    del graph
    assert lib.plvi_stream_destroy(st) == 0
    for name, t in (("steady", steady), ("steady, graph replay", replay), ("fresh (erase + update)", pair)):
        say(f"  {name}: median {np.median(t):.1f} us, min {min(t):.1f} us per call  "
            f"[{' / '.join(f'{v:.1f}' for v in t)}] ({calls} calls per window)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=1000, help="calls per window: a call is tens of microseconds")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--kp-cap", type=int, default=1200)
    ap.add_argument("--queries", default="1,64")
    ap.add_argument("--lines", action="store_true", help="UpdateConnectionsWithLines: 300 keyline slots a keyframe")
    ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    if plvi.load().plvi_device_count() <= 0:
        sys.exit("covis_bench: no HIP device (there is no CPU fallback)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ev = Events()
    say(f"library: {plvi.LIB_PATH.parent.name}/{plvi.LIB_PATH.name}")
    K, kp_cap = (120, 64) if a.small else (a.keyframes, a.kp_cap)
    kl_cap = (16 if a.small else 300) if a.lines else 0
    m = as_cmap(session(np.random.default_rng(5), K, kp_cap, kp_cap // 4, kl_cap, kl_cap // 4), 256)
    for B in ([1, 3] if a.small else [int(x) for x in a.queries.split(",")]):
        bench(ev, say, m, B, a.calls, a.windows)
    say("")
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
