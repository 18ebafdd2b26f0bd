#!/usr/bin/env python3
"""Timings of plvi_fuse_points_batch / plvi_fuse_lines_batch on the GPU (profiles/r11/fuse.txt).

Per shape: seeded tables (tests/util.reloc_case per pair for the points, tests/test_fuse.lines_general for the
lines), uploaded once; the grid from plvi_assign_grid_batch; a warm-up; then HIP events around `--calls`
back-to-back launches, `--windows` times.  The first pairs of every shape are compared with the host
restatement (tests/native/fuse_ref.cpp) in the same run.  Beside every point shape search_sim3_proj_kernel
(plvi_search_sim3_projection_batch) runs on the same tables: the only existing kernel with comparable per-point
work.  The time of a launch includes the memset node of nfused.

    python tools/fuse_bench.py [--out FILE] [--calls 50] [--windows 3] [--small]
"""
import argparse
import ctypes
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pl-vi-orbslam3_amd"))
sys.path.insert(0, str(ROOT / "tests"))

import plvi  # noqa: E402
import util  # noqa: E402
import test_fuse as tf  # noqa: E402

f32 = np.float32


class Events:
    """hipEvent timing through the runtime the library is bound to."""

    def __init__(self):
        try:
            self.hip = ctypes.CDLL("libamdhip64.so.7")
        except OSError:
            self.hip = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so")
        self.a, self.b = ctypes.c_void_p(), ctypes.c_void_p()
        for e in (self.a, self.b):
            assert self.hip.hipEventCreate(ctypes.byref(e)) == 0

    def time(self, fn, calls):
        """Milliseconds per call of `calls` back-to-back calls on the null stream."""
        assert self.hip.hipEventRecord(self.a, None) == 0
        for _ in range(calls):
            fn()
        assert self.hip.hipEventRecord(self.b, None) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        ms = ctypes.c_float()
        assert self.hip.hipEventElapsedTime(ctypes.byref(ms), self.a, self.b) == 0
        return ms.value / calls


class Tables:
    def __init__(self):
        self.bufs = []

    def up(self, arr):
        arr = np.ascontiguousarray(arr)
        b = plvi.DeviceBuffer(max(arr.nbytes, 4))
        b.upload(arr)
        self.bufs.append(b)
        return b

    def out(self, nbytes):
        b = plvi.DeviceBuffer(nbytes)
        self.bufs.append(b)
        return b


def point_pair(seed, n_kp, n_pt):
    c = util.reloc_case(seed, n_cur=n_kp, n_kf=n_pt, pre_blocked=0.0)
    rng = np.random.default_rng(seed + 7)
    ur = c["cur_kps"]["x"] - f32(40.0) / rng.uniform(1.0, 20.0, n_kp).astype(f32)
    ur[rng.random(n_kp) < 0.5] = -1.0
    return {"kps": c["cur_kps"], "desc": c["cur_desc"], "grid": c["grid"], "scale_factors": c["scale_factors"],
            "camera": c["camera"], "x3dc": c["x3dc"], "dist": c["dist"], "level": c["level"], "flags": c["kf_flags"],
            "mp_desc": c["mp_desc"], "dot": c["dist"][:, 0].astype(np.float64) * rng.uniform(0.45, 1.0, n_pt),
            "bf": f32(40.0), "inv_sigma2": tf.inv_level_sigma2(c["scale_factors"]), "uright": ur.astype(f32)}


def bench_points(ev, say, P, n_kp, n_pt, calls, windows):
    cases = [point_pair(1000 + p, n_kp, n_pt) for p in range(P)]
    t = Tables()
    stack = lambda k: np.stack([c[k] for c in cases])  # noqa: E731
    dk, dd, du = t.up(stack("kps")), t.up(stack("desc")), t.up(stack("uright"))
    dn, dpn = t.up(np.full(P, n_kp, np.int32)), t.up(np.full(P, n_pt, np.int32))
    co, ci = t.out(4 * 3073 * P), t.out(4 * n_kp * P)
    g = cases[0]["grid"]
    plvi.assign_grid_batch(dk.ptr, dn.ptr, n_kp, P, plvi.GridParams(g[0], g[2], g[4], g[5]), co.ptr, ci.ptr)
    pts = [t.up(stack(k)).ptr for k in tf.PT_KEYS] + [dpn.ptr]
    oi, od, nf = t.out(4 * n_pt * P), t.out(4 * n_pt * P), t.out(4 * P)
    om, nm = t.out(4 * n_kp * P), t.out(4 * P)
    kf = [dk.ptr, dd.ptr, dn.ptr, du.ptr, co.ptr, ci.ptr]
    lib = plvi.load()
    say(f"points: {P} pairs x {n_kp} keypoints x {n_pt} points  "
        f"(grid {P * ((n_pt + plvi.FUSE_CHUNK - 1) // plvi.FUSE_CHUNK)} x {plvi.FUSE_CHUNK}, no LDS)")
    for mode, th in ((0, 3.0), (1, 4.0)):
        prm = tf.fuse_params(cases[0], mode, th)
        run = lambda: plvi.fuse_points_batch(P, prm, kf, n_kp, pts, n_pt, oi.ptr, od.ptr, nf.ptr)  # noqa: E731
        for _ in range(3):
            run()
        lib.plvi_device_synchronize()
        got_i = oi.download(np.empty((P, n_pt), np.int32))
        got_d = od.download(np.empty((P, n_pt), np.int32))
        got_n = nf.download(np.empty(P, np.int32))
        for p in range(min(P, 2)):
            ne, ie, de, _ = tf.ref_points(cases[p], mode, th)
            assert got_n[p] == ne and np.array_equal(got_i[p], ie) and np.array_equal(got_d[p], de), (mode, p)
        ms = [ev.time(run, calls) for _ in range(windows)]
        say(f"  fuse_points_kernel mode {mode} th {th}: " + " / ".join(f"{m * 1000:.1f}" for m in ms) +
            f" us per launch ({calls} launches per window), {int(got_n.sum())} fused "
            f"({got_n.sum() / P:.0f} per pair), first pairs equal the restatement")
        sp = plvi.Sim3ProjParams()
        for k in ("fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y", "inv_w", "inv_h", "nlevels"):
            setattr(sp, k, getattr(prm, k))
        sp.th, sp.ratio_hamming, sp.projection = int(th), 1.0, 0
        for i in range(16):
            sp.scale_factors[i] = prm.scale_factors[i]
        skf = [dk.ptr, dd.ptr, dn.ptr, 0, co.ptr, ci.ptr]
        srun = lambda: plvi.search_sim3_projection_batch(P, sp, skf, n_kp, pts, n_pt, om.ptr, nm.ptr)  # noqa: E731
        for _ in range(3):
            srun()
        lib.plvi_device_synchronize()
        got_nm = nm.download(np.empty(P, np.int32))
        ms = [ev.time(srun, max(calls // 5, 5)) for _ in range(windows)]
        say(f"  search_sim3_proj_kernel th {int(th)} ratio 1.0, same tables: " +
            " / ".join(f"{m * 1000:.1f}" for m in ms) + f" us per launch, {int(got_nm.sum())} matches")
    say("")


def bench_lines(ev, say, P, n_kl, n_ml, calls, windows):
    cases = [tf.lines_general(2000 + p, n_kl, n_ml) for p in range(P)]
    t = Tables()
    stack = lambda k: np.stack([c[k] for c in cases])  # noqa: E731
    kf = [t.up(stack("kl")).ptr, t.up(stack("kl_desc")).ptr, t.up(np.full(P, n_kl, np.int32)).ptr]
    mls = [t.up(stack(k)).ptr for k in tf.ML_KEYS] + [t.up(np.full(P, n_ml, np.int32)).ptr]
    oi, od, nf = t.out(4 * n_ml * P), t.out(4 * n_ml * P), t.out(4 * P)
    prm = tf.line_params(cases[0], 3.0)
    run = lambda: plvi.fuse_lines_batch(P, prm, kf, n_kl, mls, n_ml, oi.ptr, od.ptr, nf.ptr)  # noqa: E731
    for _ in range(3):
        run()
    plvi.load().plvi_device_synchronize()
    got_i = oi.download(np.empty((P, n_ml), np.int32))
    got_n = nf.download(np.empty(P, np.int32))
    for p in range(min(P, 2)):
        ne, ie, _, _ = tf.ref_lines(cases[p], 3.0)
        assert got_n[p] == ne and np.array_equal(got_i[p], ie), p
    ms = [ev.time(run, calls) for _ in range(windows)]
    say(f"lines: {P} pairs x {n_kl} keylines x {n_ml} MapLines  "
        f"(grid {P * ((n_ml + plvi.FUSE_CHUNK - 1) // plvi.FUSE_CHUNK)} x {plvi.FUSE_CHUNK}, {48 * n_kl} B LDS)")
    say("  fuse_lines_kernel th 3.0: " + " / ".join(f"{m * 1000:.1f}" for m in ms) +
        f" us per launch ({calls} launches per window), {int(got_n.sum())} fused, first pairs equal the restatement")
    say("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    lib = plvi.load()
    if lib.plvi_device_count() <= 0:
        sys.exit("fuse_bench: no HIP device (there is no CPU fallback)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ev = Events()
    shapes = [(1, 200, 300), (3, 100, 100)] if a.small else [(1, 2000, 8000), (30, 2000, 2000), (64, 1000, 2000)]
    for P, n_kp, n_pt in shapes:
        bench_points(ev, say, P, n_kp, n_pt, a.calls, a.windows)
    bench_lines(ev, say, *((2, 50, 70) if a.small else (30, 300, 300)), a.calls, a.windows)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
