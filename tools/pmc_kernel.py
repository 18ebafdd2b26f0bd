"""FETCH_SIZE / WRITE_SIZE per launch of the kernels whose name contains one of
the given substrings, from the pass directories tools/gpu_traffic.sh writes
(pmc_FETCH_SIZE, pmc_WRITE_SIZE), calibrated like tools/pmc_traffic.py by
the 1 GiB streaming kernels of tools/calib.

usage: python tools/pmc_kernel.py PASS_DIR [substring ...]   (default: lsd_rect lsd_grow)
"""
import pathlib
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
from pmc_traffic import per_kernel  # noqa: E402

d = pathlib.Path(sys.argv[1])
subs = sys.argv[2:] or ["lsd_rect", "lsd_grow"]
cal = 1 << 30
fe = per_kernel(next(d.glob("pmc_FETCH_SIZE/**/*counter_collection.csv")), "FETCH_SIZE")
wr = per_kernel(next(d.glob("pmc_WRITE_SIZE/**/*counter_collection.csv")), "WRITE_SIZE")
mean = lambda v: sum(v) / len(v)  # noqa: E731
f_rd = cal / mean(fe["calib_dword_read"])
f_wr8 = cal / mean(wr["calib_dwordx2_store"])
print(f"calibration: true bytes per counted byte: read {f_rd:.4f}  write(dwordx2) {f_wr8:.4f}")
for k in sorted(set(fe) & set(wr)):
    if any(s in k for s in subs):
        print(f"{k}: launches {len(fe[k])}  fetched/launch raw {mean(fe[k]) / 1e9:.3f} GB calibrated "
              f"{mean(fe[k]) * f_rd / 1e9:.3f} GB  written/launch raw {mean(wr[k]) / 1e9:.3f} GB calibrated "
              f"{mean(wr[k]) * f_wr8 / 1e9:.3f} GB")
