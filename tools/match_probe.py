#!/usr/bin/env python3
"""The matching stage alone (profiles/r14): plvi_hamming_knn2_batch over P pairs of n x n ORB-sized tables and
plvi_line_match_batch over P pairs of nl x nl line tables (capacity lcap), random descriptors with 60 %
near-duplicates (about 6 % of the bits flipped), uploaded once; a warm-up, then HIP events around `--calls` back-to-back launches, `--windows`
times.  PLVI_MATCH_MFMA=0 in the environment times the VALU kernel and the three-launch line matcher on the
same tables; the first pair's tables are compared with a numpy brute-force scan in every run.  Also the
workload of the counter passes (one rocprofv3 --pmc pass per counter over `--calls 2 --windows 1`).

    python tools/match_probe.py [--pairs 3071] [--n 1000] [--nl 200] [--lcap 200] [--calls 10] [--windows 3]
"""
import argparse
import ctypes
import os
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pl-vi-orbslam3_amd"))
sys.path.insert(0, str(ROOT / "tests"))

import plvi  # noqa: E402
import batch_pack as bp  # noqa: E402
from fuse_bench import Events  # noqa: E402


def tables(rng, P, n, cap):
    """[P][cap][32] query and train tables: pair p's queries are 60 % its train rows with ~6 % flipped bits."""
    t = rng.integers(0, 256, (P, cap, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (P, cap, 32), dtype=np.uint8)
    k = int(0.6 * n)
    src = rng.integers(0, n, (P, k))
    noise = rng.integers(0, 256, (P, k, 32), dtype=np.uint8)
    for _ in range(3):  # a bit survives four draws with probability 1 / 16
        noise &= rng.integers(0, 256, (P, k, 32), dtype=np.uint8)
    q[:, :k] = np.take_along_axis(t, src[:, :, None], axis=1) ^ noise
    return q, t


def brute_knn2(q, t):
    d = bp.hamming(q, t)
    order = np.argsort(d, axis=1, kind="stable")[:, :2]
    return order[:, 0], np.take_along_axis(d, order[:, :1], 1)[:, 0], order[:, 1], np.take_along_axis(d, order[:, 1:], 1)[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3071)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--nl", type=int, default=200)
    ap.add_argument("--lcap", type=int, default=200)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=3)
    a = ap.parse_args()
    lib = plvi.load()
    if lib.plvi_device_count() <= 0:
        sys.exit("match_probe: no HIP device (there is no CPU fallback)")
    P, n, nl, lcap = a.pairs, a.n, a.nl, a.lcap
    rng = np.random.default_rng(14)
    bufs = []

    def up(arr):
        arr = np.ascontiguousarray(arr)
        b = plvi.DeviceBuffer(max(arr.nbytes, 4))
        b.upload(arr)
        bufs.append(b)
        return ctypes.c_void_p(b.ptr)

    def out(nbytes):
        bufs.append(plvi.DeviceBuffer(nbytes))
        return ctypes.c_void_p(bufs[-1].ptr)

    q, t = tables(rng, P, n, n)
    lq, lt = tables(rng, P, nl, lcap)
    dq, dt, dn = up(q), up(t), up(np.full(P, n, np.int32))
    dlq, dlt, dln = up(lq), up(lt), up(np.full(P, nl, np.int32))
    o = [out(4 * P * n) for _ in range(4)]
    scratch, m12, nm = out(4 * 4 * P * 2 * lcap), out(4 * P * lcap), out(4 * P)

    def knn():
        assert lib.plvi_hamming_knn2_batch(dq, dn, n, dt, dn, n, P, *o, None) == 0

    def lines():
        assert lib.plvi_line_match_batch(dlq, dln, lcap, dlt, dln, lcap, P, 0.9, scratch, m12, nm, None) == 0

    for _ in range(2):
        knn()
        lines()
    lib.plvi_device_synchronize()
    got = [bufs[6 + k].download(np.empty((P, n), np.int32))[0] for k in range(4)]
    for g, e in zip(got, brute_knn2(q[0, :n], t[0, :n])):
        assert np.array_equal(g, e)
    mode = "VALU kernel, three-launch line matcher (PLVI_MATCH_MFMA=0)" \
        if os.environ.get("PLVI_MATCH_MFMA", "1") == "0" else "matrix-core kernels"
    ev = Events()
    print(f"{mode}: {P} pairs; first pair equals the brute-force scan")
    ms = [ev.time(knn, a.calls) for _ in range(a.windows)]
    print(f"  kNN-2 {n} x {n}: " + " / ".join(f"{m:.3f}" for m in ms) + f" ms per launch ({a.calls} per window)")
    ms = [ev.time(lines, a.calls) for _ in range(a.windows)]
    print(f"  line match {nl} x {nl} (cap {lcap}): " + " / ".join(f"{m:.3f}" for m in ms) +
          f" ms per call ({a.calls} per window)")


if __name__ == "__main__":
    main()
