#!/usr/bin/env python3
"""Host time of 1000 back-to-back calls of plvi_assign_grid_batch and plvi_search_by_bow_batch on the smallest valid
shapes (cap 1, one frame / pair, every count 0), a device synchronise at the end of each window: what the per-call
hipFuncSetAttribute of launch_lds (csrc/plvi_common.h) costs where the attribute used to be set once per process
(profiles/r18/launch_overhead.txt).  Where the window is bounded by the kernel and not by the host (see the figures
there), the number says that much and no more.

    python tools/launch_overhead.py

PLVI_LIB=... selects another build of the library (the parent commit's, for the comparison).
"""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pl-vi-orbslam3_amd"))
import plvi  # noqa: E402
from plvi import _abi  # noqa: E402

lib = plvi.load()
CALLS, WINDOWS = 1000, 9


def zeros(nbytes=1 << 16):
    b = _abi.DeviceBuffer(nbytes)
    b.upload(np.zeros(nbytes, np.uint8))
    return b


bufs = [zeros() for _ in range(18)]
P = [b.ptr for b in bufs]
gp = plvi.GridParams(0.0, 0.0, 0.1, 0.1)


def assign():
    return lib.plvi_assign_grid_batch(P[0], P[1], 1, 1, ctypes.byref(gp), P[2], P[3], None)


def bow():
    return lib.plvi_search_by_bow_batch(1, ctypes.c_float(0.75), 1, 1, 1, 1, P[0], P[1], P[2], P[3], P[4], P[5], P[6],
                                        P[7], P[8], P[9], P[10], P[11], P[12], P[13], P[14], P[15], None)


print("library:", "PLVI_LIB" if os.environ.get("PLVI_LIB") else "lib/libplvi_frontend.so")
for name, fn in (("plvi_assign_grid_batch", assign), ("plvi_search_by_bow_batch", bow)):
    for _ in range(CALLS):
        assert fn() == 0
    lib.plvi_device_synchronize()
    ws = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        lib.plvi_device_synchronize()
        ws.append((time.perf_counter() - t0) * 1e3)
    s = sorted(ws)
    print(f"  {name}: {CALLS} calls + sync, ms per window: median {s[len(s) // 2]:.2f}, min {s[0]:.2f}  ["
          + " / ".join(f"{w:.2f}" for w in ws) + "]")
