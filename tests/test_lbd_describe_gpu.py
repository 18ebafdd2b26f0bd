"""lbd_describe_kernel (BinaryDescriptor::computeLBD + binaryConversion): the
multi-line waves, the 16-sample gather step and the 21-step band sums give
the oracle's descriptors bit for bit at the inputs where that loop structure
can go wrong: line lengths of every residue mod 16 and shorter than a step,
frames with fewer lines than the capacity or none, a grid far larger than the
count, an odd plane width, a reused handle, and a captured schedule.  Every
case asserts from the oracle's output that the input has the property it is
there for, then compares bitwise with oracle_lib.line_extract."""
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
import plvi
from plvi import synth
from util import assert_lines_same, real_frames

pytestmark = pytest.mark.gpu

CW, CH = 170, 130


def _crop(seed):
    return np.ascontiguousarray(synth.frame(seed)[:CH, :CW])


@pytest.fixture(scope="module")
def crop1():
    img = _crop(1)
    return img, ol.line_extract(img)


def _batch_out(lx, frames):
    n = len(frames)
    h, w = frames[0].shape
    arr = np.ascontiguousarray(np.stack(frames))
    buf = plvi.DeviceBuffer(arr.nbytes)
    buf.upload(arr)
    lx.extract_batch(buf.ptr, n, w * h, w)
    plvi.load().plvi_device_synchronize()
    klp, dep, fnp, cop, cap = lx.outputs()
    cnt = plvi.download(cop, np.zeros(n, np.int32))
    kl = plvi.download(klp, np.zeros(n * cap, plvi.KEYLINE_DTYPE))
    de = plvi.download(dep, np.zeros((n * cap, 32), np.uint8))
    fn = plvi.download(fnp, np.zeros((n * cap, 3), np.float64))
    return cnt, [(kl[f * cap:f * cap + cnt[f]], de[f * cap:f * cap + cnt[f]], fn[f * cap:f * cap + cnt[f]])
                 for f in range(n)], de.reshape(n, cap, 32)


def test_small_crop_every_length_residue(plvi_lib, crop1):
    img, exp = crop1
    npx = exp[0]["numOfPixels"]
    assert len(set(int(v) % 16 for v in npx)) == 16 and npx.min() < 8
    assert set(int(o) for o in exp[0]["octave"]) == {0, 1} and len(npx) < 200
    lx = plvi.Lineextractor(200, 0, 0.8, 2, 2.0, 0, CW, CH)
    assert_lines_same(lx(img), exp, "crop170x130")
    assert lx.errors() == 0


def test_batch_with_empty_frame_forward_and_reversed(plvi_lib, crop1):
    flat = np.full((CH, CW), 90, np.uint8)
    frames = [crop1[0], flat, _crop(9)]
    exps = [crop1[1], ol.line_extract(flat), ol.line_extract(frames[2])]
    assert len(exps[1][0]) == 0 and len(exps[0][0]) > 0 and len(exps[2][0]) > 0
    lx = plvi.Lineextractor(200, 0, 0.8, 2, 2.0, 0, CW, CH, max_batch=3)
    _, dep, _, _, cap = lx.outputs()
    junk = np.full(3 * cap * 32, 0xA5, np.uint8)
    assert plvi.load().plvi_memcpy(dep, junk.ctypes.data, junk.nbytes, 1) == 0
    cnt, got, de = _batch_out(lx, frames)
    assert cnt.tolist() == [len(e[0]) for e in exps]
    for f in range(3):
        assert_lines_same(got[f], exps[f], f"forward frame {f}")
    assert (de[1] == 0xA5).all(), "the empty frame's descriptor rows were written"
    # the same handle, frames in reverse order: nothing of the first run may survive
    cnt, got, _ = _batch_out(lx, frames[::-1])
    assert cnt.tolist() == [len(e[0]) for e in exps[::-1]]
    for f in range(3):
        assert_lines_same(got[f], exps[2 - f], f"reversed frame {f}")
    assert lx.errors() == 0


def test_keep_all_grid_far_larger_than_count(plvi_lib):
    img = synth.frame(1)
    exp = ol.line_extract(img, nfeatures=0)
    lx = plvi.Lineextractor(0, 0, 0.8, 2, 2.0, 0, 640, 480)
    cap = lx.outputs()[4]
    assert 200 < len(exp[0]) < cap // 4 and exp[0]["numOfPixels"].max() > 200
    assert_lines_same(lx(img), exp, "keep-all")
    assert lx.errors() == 0


def test_odd_plane_width(plvi_lib):
    fr = real_frames()
    big = np.concatenate([fr["euroc1"], fr["euroc1"][:, :40]], axis=1)  # 792 x 480
    img = np.ascontiguousarray(big[:482, 3:645])
    # the crop of tests/test_lbd_sobel_gpu.py (the frame has 480 rows): octave 1 is
    # 321 wide, so imageWidth = realWidth - 1 is even and rows start at odd offsets
    h, w = img.shape
    assert w == 642 and (w // 2) % 2 == 1
    exp = ol.line_extract(img)
    assert len(exp[0]) > 0 and set(int(o) for o in exp[0]["octave"]) == {0, 1}
    lx = plvi.Lineextractor(200, 0, 0.8, 2, 2.0, 0, w, h)
    assert_lines_same(lx(img), exp, "crop642")


def test_timing_kind_4_one_launch_per_batch(plvi_lib, crop1):
    lx = plvi.Lineextractor(200, 0, 0.8, 2, 2.0, 0, CW, CH, max_batch=3)
    frames = [crop1[0], _crop(9), crop1[0]]
    _batch_out(lx, frames)
    lx.kernel_timing(True)
    runs = 3
    for _ in range(runs):
        _batch_out(lx, frames)
    t4, n4 = lx.kernel_timing_read(4)
    assert n4 == runs and t4 > 0
    # kinds 0-3 keep their meaning: one Sobel launch per octave and batch;
    # lsd_prep and region2rect one or two launches per batch (per octave / stream)
    assert lx.kernel_timing_read(1)[1] == runs and lx.kernel_timing_read(2)[1] == runs
    assert lx.kernel_timing_read(0)[1] in (runs, 2 * runs) and lx.kernel_timing_read(3)[1] in (runs, 2 * runs)
    for k in range(4):
        assert lx.kernel_timing_read(k)[0] > 0
    with pytest.raises(plvi.PlviError):
        lx.kernel_timing_read(5)
    lx.kernel_timing(False)


def test_frame_schedule_two_frames_vs_oracle(plvi_lib):
    n = 2
    frames = synth.batch(n, seed0=5)
    buf = plvi.DeviceBuffer(frames.nbytes)
    buf.upload(frames)
    orb = plvi.ORBextractor(1000, 1.2, 8, 20, 7, 640, 480, max_batch=n)
    lx = plvi.Lineextractor(200, 0, 0.8, 2, 2.0, 0, 640, 480, max_batch=n)
    plvi.frame_extract_batch(orb, lx, buf.ptr, n, 640 * 480, 640)
    plvi.load().plvi_device_synchronize()
    klp, dep, fnp, cop, cap = lx.outputs()
    cnt = plvi.download(cop, np.zeros(n, np.int32))
    de = plvi.download(dep, np.zeros((n * cap, 32), np.uint8))
    for f in range(n):
        ekl, ede, _ = ol.line_extract(frames[f])
        assert cnt[f] == len(ekl) > 0
        np.testing.assert_array_equal(de[f * cap:f * cap + cnt[f]], ede)
    assert lx.errors() == 0


def test_frame_schedule_two_frames_graph_replay():
    """The same two frames (tools/graph_probe.py's seed) captured and replayed:
    every table equal to the step issued call by call, LBD descriptors among
    them; a child process on the system runtime, as tests/test_frame_gpu.py."""
    from conftest import ROOT
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "graph_probe.py"), "frame", "2"], capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0 and "frame replay equal" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
