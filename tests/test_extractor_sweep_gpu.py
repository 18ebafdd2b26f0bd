"""Extractor parity away from the default configuration and frame size.

Every other GPU test builds ORBextractor(1000 | 5000, 1.2, 8, 20, 7) and
Lineextractor(200 | 0 | 100, 0, 0.8 | 1.0, 2, 2.0, 0) at 640x480, 752x480 or
641x479.  The geometry- and parameter-dependent code (cell grid, octree
roots, blur + FAST strip planner, packed resize tables, LSD prep strips and
row bands, min_reg_size, list / node capacities, threshold clamps) is swept
here over small and odd shapes, other scale factors, level counts, quotas
and thresholds, bit-exactly against the CPU oracle with the comparison of
test_orb_gpu.py / test_lines_gpu.py (util.assert_orb_same /
assert_lines_same): every KeyPoint / KeyLine field, descriptors, monoIndex
and the f64 line functions.  Nothing has a tolerance.

Each size gets one batch of five frames (one more than the streaming pyramid
kernel's four frames per workgroup, so its last block is partial).  The
oracle's side of every case is computed once per module and shared."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
import plvi
from plvi import synth
from util import assert_lines_same, assert_orb_same, structured_frames

pytestmark = pytest.mark.gpu

FRAMES = ("synth", "noise", "checker", "binary_noise", "flat")
SYNTH, NOISE, FLAT = 0, 1, 4


@functools.lru_cache(maxsize=None)
def frames(w, h):
    s = structured_frames(w, h)
    out = (synth.frame(7, w, h), np.random.default_rng(2).integers(0, 256, (h, w), dtype=np.uint8),
           s["checker"], s["binary_noise"], np.full((h, w), 128, np.uint8))
    for a in out:
        a.setflags(write=False)
    return out


def upload(imgs, pad):
    """The frames as one device batch with `pad` extra bytes per row: (buffer, frame stride, row stride)."""
    h, w = imgs[0].shape
    stride = w + pad
    host = np.zeros((len(imgs), h, stride), np.uint8)
    for k, im in enumerate(imgs):
        host[k, :, :w] = im
    buf = plvi.DeviceBuffer(host.nbytes)
    buf.upload(host)
    return buf, h * stride, stride


# ------------------------------------------------------------------- ORB
# (w, h, nfeatures, scale, nlevels, ini, min)
ORB_CASES = [
    (62, 62, 1000, 1.2, 1, 20, 7),      # smallest legal level: one cell, one root, narrower than a strip, no resize table
    (63, 94, 1000, 1.2, 1, 20, 7),      # portrait: nIni = 1 from a ratio below 1, odd width with packed rows
    (120, 200, 1000, 1.2, 1, 20, 7),
    (330, 70, 1000, 1.2, 1, 20, 7),     # nIni = 8 = kOrbMaxRoots, one cell row
    (96, 64, 50, 1.2, 1, 20, 7),        # small quota
    (129, 97, 300, 1.2, 2, 20, 7),      # width = 1 mod 4
    (160, 120, 1000, 1.2, 3, 20, 7),
    (160, 120, 0, 1.2, 3, 20, 7),       # quota 0: the roots are still emitted
    (160, 120, 1, 1.2, 3, 20, 7),
    (200, 150, 1000, 1.5, 3, 20, 7),    # top level 89 x 67
    (257, 193, 1000, 1.1, 5, 20, 7),    # five dense levels
    (322, 240, 1000, 2.0, 2, 20, 7),    # INTER_AREA fast path, 161-wide level with one tail column
    (200, 160, 1000, 2.0, 2, 20, 7),    # area path with 4 tail columns
    (322, 241, 1000, 2.0, 2, 20, 7),    # 241 / 2 rounds to 120: the y scale is not 2, the level is bilinear
    (320, 240, 1000, 1.2, 8, 20, 7),
    (320, 240, 1000, 1.2, 8, 40, 12),
    (320, 240, 1000, 1.2, 8, 7, 20),    # ini < min
    (320, 240, 1000, 1.2, 8, 255, 0),
    (320, 240, 1000, 1.2, 8, 300, -5),  # clamped to (255, 0)
    (160, 120, 1000, 1.2, 3, 0, 0),     # every pixel a candidate
    (160, 120, 1000, 1.2, 3, 255, 255),  # none
]


def orb_id(c):
    return "{}x{}-n{}-s{}-L{}-t{}_{}".format(*c)


@functools.lru_cache(maxsize=None)
def orb_expected(case):
    """The oracle's (mono, keypoints, descriptors) of the five frames, checked not to be vacuous."""
    w, h, nf, sc, nl, ini, mn = case
    exp = [ol.orb_extract(im, nf, sc, nl, ini, mn) for im in frames(w, h)]
    for k, (mono, kps, desc) in enumerate(exp):
        assert mono >= 0, f"{FRAMES[k]}: oracle refused {case}"
        per_level = [int((kps["octave"] == l).sum()) for l in range(nl)]
        if (ini, mn) == (255, 255) or k == FLAT:
            assert per_level == [0] * nl, f"{FRAMES[k]}: {per_level}"
        elif k in (SYNTH, NOISE):
            assert min(per_level) >= 1, f"{FRAMES[k]}: a level without keypoints {per_level}"
    return exp


@functools.lru_cache(maxsize=None)
def orb_pyramids(w, h, sc, nl):
    """mvImagePyramid of the five frames (thresholds and quotas do not enter it)."""
    return [[ol.orb_stage(im, l, 1000, sc, nl, 20, 7, cap=20000)["pyr"] for l in range(nl)] for im in frames(w, h)]


def orb_check_batch(case, pad, tag):
    """(a)-(c): the five-frame batch through extract_batch; pyramid levels first, then the tables."""
    w, h, nf, sc, nl, ini, mn = case
    imgs = frames(w, h)
    exp, pyr = orb_expected(case), orb_pyramids(w, h, sc, nl)
    B = len(imgs)
    buf, fstride, rstride = upload(imgs, pad)
    ext = plvi.ORBextractor(nf, sc, nl, ini, mn, w, h, max_batch=B)
    ext.extract_batch(buf.ptr, B, fstride, rstride)
    assert plvi.load().plvi_device_synchronize() == 0
    assert ext.errors() == 0
    p0, fs0, w0, h0 = ext.pyramid_device(0)
    assert (w0, h0) == (w, h)
    if pad == 0:
        assert (p0, fs0) == (buf.ptr, fstride), "packed frames: level 0 is a view of the batch"
    else:
        assert p0 != buf.ptr and fs0 == w * h
    for k in range(B):
        for l in range(nl):
            got = ext.pyramid_level(l, k)
            assert got.shape == pyr[k][l].shape, f"{tag} {FRAMES[k]} level {l}: {got.shape} != {pyr[k][l].shape}"
            bad = np.argwhere(got != pyr[k][l])
            assert bad.size == 0, (f"{tag} {FRAMES[k]} pyramid level {l}: {len(bad)} pixels differ, first (y, x) "
                                   f"{bad[:5].tolist()} got {got[tuple(bad[0])]} exp {pyr[k][l][tuple(bad[0])]}")
    kp_p, de_p, co_p, mo_p, cap = ext.outputs()
    cnt = plvi.download(co_p, np.zeros(B, np.int32))
    mono = plvi.download(mo_p, np.zeros(B, np.int32))
    kps = plvi.download(kp_p, np.zeros(B * cap, plvi.KEYPOINT_DTYPE))
    desc = plvi.download(de_p, np.zeros((B * cap, 32), np.uint8))
    for k in range(B):
        assert 0 <= cnt[k] <= cap, f"{tag} {FRAMES[k]}: count {cnt[k]} of {cap}"
        s = slice(k * cap, k * cap + cnt[k])
        assert_orb_same((int(mono[k]), kps[s], desc[s]), exp[k], f"{tag} {FRAMES[k]}")
    ext.close()


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("mode", ["0", "100000"])
@pytest.mark.parametrize("case", ORB_CASES, ids=orb_id)
def test_orb_sweep_batch(plvi_lib, monkeypatch, case, mode, pad):
    """The five-frame batch, packed (level 0 a view of the frames) and row-padded (pad 3: level 0
    copied), through the streaming pyramid kernel (PLVI_PYR_LEVELWISE=0) and the level-by-level
    launches (100000): every pyramid level of every frame, then keypoints, descriptors and monoIndex."""
    monkeypatch.setenv("PLVI_PYR_LEVELWISE", mode)
    orb_check_batch(case, pad, f"{orb_id(case)} levelwise {mode} pad {pad}")


@pytest.mark.parametrize("case", ORB_CASES, ids=orb_id)
def test_orb_sweep_single_frame(plvi_lib, case):
    """One operator() call on the synth frame."""
    w, h, nf, sc, nl, ini, mn = case
    ext = plvi.ORBextractor(nf, sc, nl, ini, mn, w, h)
    assert_orb_same(ext(frames(w, h)[SYNTH], None, (0, 0)), orb_expected(case)[SYNTH], orb_id(case))
    ext.close()


@pytest.mark.parametrize("case", [ORB_CASES[6], ORB_CASES[10]], ids=orb_id)
def test_orb_sweep_octree_memory_path(plvi_lib, monkeypatch, case):
    """PLVI_ORB_OCT_LDS=0: every level's octree scans its candidate list in memory."""
    assert case[:2] in ((160, 120), (257, 193))
    monkeypatch.setenv("PLVI_ORB_OCT_LDS", "0")
    orb_check_batch(case, 0, f"{orb_id(case)} oct lds 0")


def test_orb_sweep_threshold_clamps_agree():
    """(300, -5) clamps to (255, 0): the oracle gives the same output for both (the GPU side is compared
    with each in test_orb_sweep_batch)."""
    a, b = orb_expected(ORB_CASES[17]), orb_expected(ORB_CASES[18])
    assert ORB_CASES[17][5:] == (255, 0) and ORB_CASES[18][5:] == (300, -5)
    for k in range(len(FRAMES)):
        assert_orb_same(a[k], b[k], FRAMES[k])


# ----------------------------------------------------------------- lines
# (w, h, nfeatures, lsd_scale, nlevels); scale 2.0, refine 0, extractor 0
LINE_CASES = [
    (64, 48, 200, 0.8, 2),    # octave 1 is 32 x 24, its scaled plane 26 x 19: one prep strip, 8 bands of 2-3 rows
    (96, 64, 200, 0.8, 2),    # odd half-widths, scaled widths around one strip
    (130, 98, 200, 0.8, 2),
    (200, 152, 200, 0.8, 2),
    (322, 242, 200, 0.8, 2),
    (300, 64, 200, 0.8, 2),   # extreme aspect ratios
    (64, 300, 200, 0.8, 2),
    (250, 190, 0, 0.8, 2),    # keep all
    (160, 120, 5, 0.8, 2),    # the cut after std::sort
    (160, 120, 200, 1.0, 2),  # no scaling
    (160, 120, 200, 0.9, 2),  # 7 taps like 0.8 and 0.75, another sigma and resize table
    (160, 120, 200, 0.75, 2),
    (161, 121, 200, 0.8, 1),  # one octave, odd size
    (322, 242, 0, 1.0, 1),
]


def line_id(c):
    return "{}x{}-n{}-s{}-L{}".format(*c)


@functools.lru_cache(maxsize=None)
def line_expected(case):
    w, h, nf, ls, nl = case
    exp = [ol.line_extract(im, nf, ls, nl, 2.0) for im in frames(w, h)]
    per_octave = [int((exp[SYNTH][0]["octave"] == o).sum()) for o in range(nl)]
    assert min(per_octave) >= 1, f"synth: an octave without lines {per_octave}"
    return exp


def line_check_batch(case, pad, tag):
    w, h, nf, ls, nl = case
    imgs = frames(w, h)
    exp = line_expected(case)
    B = len(imgs)
    buf, fstride, rstride = upload(imgs, pad)
    lx = plvi.Lineextractor(nf, 0, ls, nl, 2.0, 0, w, h, max_batch=B)
    lx.extract_batch(buf.ptr, B, fstride, rstride)
    assert plvi.load().plvi_device_synchronize() == 0
    assert lx.errors() == 0
    klp, dep, fnp, cop, cap = lx.outputs()
    cnt = plvi.download(cop, np.zeros(B, np.int32))
    kl = plvi.download(klp, np.zeros(B * cap, plvi.KEYLINE_DTYPE))
    de = plvi.download(dep, np.zeros((B * cap, 32), np.uint8))
    fn = plvi.download(fnp, np.zeros((B * cap, 3), np.float64))
    for k in range(B):
        assert 0 <= cnt[k] <= cap, f"{tag} {FRAMES[k]}: count {cnt[k]} of {cap}"
        s = slice(k * cap, k * cap + cnt[k])
        assert_lines_same((kl[s], de[s], fn[s]), exp[k], f"{tag} {FRAMES[k]}")
    lx.close()


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("mw", [None, "0"])
@pytest.mark.parametrize("case", LINE_CASES, ids=line_id)
def test_lines_sweep_batch(plvi_lib, monkeypatch, case, mw, pad):
    """The five-frame batch, packed and row-padded, with the default multi-wave region growing and with
    the sequential kernel (PLVI_GROW_MW=0)."""
    if mw is None:
        monkeypatch.delenv("PLVI_GROW_MW", raising=False)
    else:
        monkeypatch.setenv("PLVI_GROW_MW", mw)
    line_check_batch(case, pad, f"{line_id(case)} mw {mw} pad {pad}")


@pytest.mark.parametrize("case", LINE_CASES, ids=line_id)
def test_lines_sweep_single_frame(plvi_lib, case):
    w, h, nf, ls, nl = case
    lx = plvi.Lineextractor(nf, 0, ls, nl, 2.0, 0, w, h)
    assert_lines_same(lx(frames(w, h)[SYNTH]), line_expected(case)[SYNTH], line_id(case))
    lx.close()


# -------------------------------------------------------------- refusals
@pytest.mark.parametrize("w,h,scale,nlevels,oracle_refuses", [
    (61, 61, 1.2, 1, True),     # nCols is 0
    (100, 80, 2.0, 2, True),    # level 1 (50 x 40) is too small
    (70, 200, 1.2, 1, True),    # nIni is 0
    (400, 70, 1.2, 1, False),   # nIni is 10, above kOrbMaxRoots (a limit of the HIP path alone)
])
def test_orb_create_refuses(plvi_lib, w, h, scale, nlevels, oracle_refuses):
    with pytest.raises(plvi.PlviError) as e:
        plvi.ORBextractor(1000, scale, nlevels, 20, 7, w, h)
    assert e.value.code == plvi.PLVI_E_BADARG
    assert plvi_lib.plvi_device_synchronize() == 0
    if oracle_refuses:
        mono, kps, desc = ol.orb_extract(synth.frame(7, w, h), 1000, scale, nlevels, 20, 7)
        assert mono == -2 and len(kps) == 0


@pytest.mark.parametrize("w,h,lsd_scale,nlevels", [
    (161, 120, 0.8, 2),   # octave 1 is not an exact half
    (160, 120, 0.5, 2),   # needs 9 Gaussian taps
    (160, 120, 1.2, 2),   # outside (0, 1]
])
def test_lines_create_refuses(plvi_lib, w, h, lsd_scale, nlevels):
    with pytest.raises(plvi.PlviError) as e:
        plvi.Lineextractor(200, 0, lsd_scale, nlevels, 2.0, 0, w, h)
    assert e.value.code == plvi.PLVI_E_BADARG
    assert plvi_lib.plvi_device_synchronize() == 0


# ----------------------------------------------------------- re-planning
REPLAN_SIZES = [(160, 120), (200, 152), (96, 64), (160, 120)]


def test_orb_replan_live_handle(plvi_lib):
    """operator() on another frame size re-plans the live handle; a size init refuses raises and leaves
    the old plan intact.  With three levels 96x64 is such a size already (level 2 is 67x44, 12 rows
    between the borders: no cell row; the oracle returns -2), so the sequence holds two refusals."""
    ext = plvi.ORBextractor(1000, 1.2, 3, 20, 7, 160, 120)
    for step, (w, h) in enumerate(REPLAN_SIZES):
        img = synth.frame(7, w, h)
        exp = ol.orb_extract(img, 1000, 1.2, 3, 20, 7)
        if (w, h) == (96, 64):
            assert exp[0] == -2 and len(exp[1]) == 0
            with pytest.raises(plvi.PlviError) as e:
                ext(img, None, (0, 0))
            assert e.value.code == plvi.PLVI_E_BADARG
            continue
        assert all((exp[1]["octave"] == l).any() for l in range(3))
        assert_orb_same(ext(img, None, (0, 0)), exp, f"step {step} {w}x{h}")
        for l in range(3):
            assert np.array_equal(ext.pyramid_level(l), ol.orb_stage(img, l, 1000, 1.2, 3, 20, 7, cap=20000)["pyr"])
    with pytest.raises(plvi.PlviError) as e:
        ext(synth.frame(7, 61, 61), None, (0, 0))
    assert e.value.code == plvi.PLVI_E_BADARG
    img = synth.frame(7, 160, 120)
    assert_orb_same(ext(img, None, (0, 0)), ol.orb_extract(img, 1000, 1.2, 3, 20, 7), "after the refused size")
    ext.close()


def test_lines_replan_live_handle(plvi_lib):
    lx = plvi.Lineextractor(200, 0, 0.8, 2, 2.0, 0, 160, 120)
    for step, (w, h) in enumerate(REPLAN_SIZES):
        img = synth.frame(7, w, h)
        exp = ol.line_extract(img, 200, 0.8, 2, 2.0)
        assert all((exp[0]["octave"] == o).any() for o in range(2))
        assert_lines_same(lx(img), exp, f"step {step} {w}x{h}")
    with pytest.raises(plvi.PlviError) as e:
        lx(synth.frame(7, 161, 121))  # not an exact half for the second octave
    assert e.value.code == plvi.PLVI_E_BADARG
    img = synth.frame(7, 160, 120)
    assert_lines_same(lx(img), ol.line_extract(img, 200, 0.8, 2, 2.0), "after the refused size")
    lx.close()
