"""LBD describe (lbd_describe_kernel) alone at several batch sizes (DESIGN.md
§26): a lines-only batch with nothing beside it, the kernel's time per batch
from the extractor's own event pairs (kernel_timing kind 4) next to the whole
line chain per batch.  Select an A/B build with PLVI_LIB=... (see
tools/build_variant.sh).

usage: python tools/lbd_probe.py [B,B,...]
"""
import sys
import time
import pathlib

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pl-vi-orbslam3_amd"))
import torch  # noqa: E402
import plvi  # noqa: E402
from plvi import synth  # noqa: E402

Bs = [int(b) for b in (sys.argv[1] if len(sys.argv) > 1 else "1,64,3072").split(",")]
W, H = 640, 480
seq = synth.device_sequence(max(Bs), W, H, seed=1, device="cuda:0", run=256)
s = torch.cuda.Stream()
for B in Bs:
    lx = plvi.Lineextractor(200, 0, 0.8, 2, 2.0, 0, W, H, max_batch=B)
    N = 5 if B >= 1024 else 20
    for _ in range(3):
        lx.extract_batch(seq.data_ptr(), B, W * H, W, stream=s.cuda_stream)
    torch.cuda.synchronize()
    lx.kernel_timing(True)
    t0 = time.perf_counter()
    for _ in range(N):
        lx.extract_batch(seq.data_ptr(), B, W * H, W, stream=s.cuda_stream)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / N * 1e3
    dt_, dn = lx.kernel_timing_read(4)
    lx.kernel_timing(False)
    assert lx.errors() == 0
    print(f"B={B:5d} lbd_describe {dt_ / N:8.4f} ms/batch ({dn // N} launches)  line chain {dt:8.3f} ms/batch",
          flush=True)
    lx.close()
