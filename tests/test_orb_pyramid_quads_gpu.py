"""The pyramid builders' quad path: four consecutive output pixels per lane.

test_extractor_sweep_gpu.py sweeps small and odd shapes and the scales 1.1 /
1.2 / 1.5 / 2.0 through both builders on five-frame batches.  This file
covers what the quad routine (pyr_quad / pyr_store_quad, orb_kernels.hpp)
adds and that sweep does not reach:

* lane and pass edges: 64 lanes x 4 pixels are 256 columns, a resizer pass is
  two quads per lane (512 columns); level widths of exactly 256, 257, 512 and
  513, all four residues mod 4, a 1024 x 170 frame (level 1 is 853 wide, the
  loader at its width limit) and a last level of the smallest legal width;
* row-end stores: every batch fills max_batch exactly, so the last frame's
  last level ends the pyramid allocation, and every batch holds binary-noise
  (0 / 255) frames, so a stray byte cannot match by accident;
* partial workgroups of the streaming builder (four frames each): 1, 3, 4, 5
  and 9 frames of 320 x 240 with eight levels, every frame different;
* source alignment: row padding 0, 3 and 5 and a packed batch at an odd
  device address;
* scales 1.05, 1.2, 2.0 (the area kernels with 1 and 4 tail columns, and the
  322 x 241 frame whose level is bilinear at x scale 2) and 2.5, where a
  quad's taps no longer fit the 8-byte window and the level is built pixel by
  pixel (kPyrXtabWide);
* the PLVI_COMPAT_RESIZE_V_GENERIC vertical pass.

Every case runs through the streaming kernel (PLVI_PYR_LEVELWISE=0) and the
level-by-level launches (100000).  Everything is exact equality with the CPU
oracle: every pyramid level of every frame, then keypoints, descriptors and
monoIndex of every frame.  The oracle's side is computed once per frame and
configuration and shared."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_lib as ol
import plvi
from plvi import synth
from util import assert_orb_same

pytestmark = pytest.mark.gpu

MODES = ["0", "100000"]


def level_sizes(w, h, scale, nlevels):
    """ComputePyramid's level sizes: cvRound(size * (1.0f / mvScaleFactor[l])), float arithmetic."""
    out, sf = [], np.float32(1.0)
    for l in range(nlevels):
        if l:
            sf = np.float32(sf * np.float32(scale))
        inv = np.float32(1.0) / sf
        out.append((int(np.rint(np.float32(w) * inv)), int(np.rint(np.float32(h) * inv))))
    return out


@functools.lru_cache(maxsize=None)
def frame(k, w, h):
    """Frame k of a batch: every frame differs; k = 1 mod 3 is binary (0 / 255) noise."""
    if k % 3 == 0:
        img = synth.frame(k + 1, w, h)
    elif k % 3 == 1:
        img = (np.random.default_rng(100 + k).integers(0, 2, (h, w)) * 255).astype(np.uint8)
    else:
        img = np.random.default_rng(100 + k).integers(0, 256, (h, w), dtype=np.uint8)
    img = np.ascontiguousarray(img, np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def expected(k, w, h, scale, nlevels, compat):
    """The oracle's pyramid levels and (mono, keypoints, descriptors) of frame k."""
    img = frame(k, w, h)
    with ol.compat(compat):
        pyr = [ol.orb_stage(img, l, 1000, scale, nlevels, 20, 7, cap=20000)["pyr"] for l in range(nlevels)]
        ext = ol.orb_extract(img, 1000, scale, nlevels, 20, 7)
    assert ext[0] >= 0, f"oracle refused {w}x{h} scale {scale} levels {nlevels}"
    return pyr, ext


def check(case, B, mode, monkeypatch, pad=0, odd_address=False, compat=0):
    w, h, scale, nlevels = case
    tag = f"{w}x{h} s{scale} L{nlevels} B{B} levelwise {mode} pad {pad} odd {odd_address} compat {compat}"
    monkeypatch.setenv("PLVI_PYR_LEVELWISE", mode)
    stride = w + pad
    host = np.zeros((B, h, stride), np.uint8)
    for k in range(B):
        host[k, :, :w] = frame(k, w, h)
    off = 1 if odd_address else 0
    buf = plvi.DeviceBuffer(host.nbytes + off)
    lib = plvi.load()
    assert lib.plvi_memcpy(ctypes.c_void_p(buf.ptr + off), ctypes.c_void_p(host.ctypes.data), host.nbytes, 1) == 0
    ext = plvi.ORBextractor(1000, scale, nlevels, 20, 7, w, h, max_batch=B, compat=compat)
    ext.extract_batch(buf.ptr + off, B, h * stride, stride)
    assert lib.plvi_device_synchronize() == 0
    assert ext.errors() == 0
    sizes = level_sizes(w, h, scale, nlevels)
    for l in range(nlevels):
        assert ext.pyramid_device(l)[2:] == sizes[l], f"{tag}: level {l} is {ext.pyramid_device(l)[2:]}"
    for k in range(B):
        pyr = expected(k, w, h, scale, nlevels, compat)[0]
        for l in range(nlevels):
            got = ext.pyramid_level(l, k)
            assert got.shape == pyr[l].shape, f"{tag} frame {k} level {l}: {got.shape} != {pyr[l].shape}"
            bad = np.argwhere(got != pyr[l])
            assert bad.size == 0, (f"{tag} frame {k} level {l}: {len(bad)} pixels differ, first (y, x) "
                                   f"{bad[:5].tolist()} got {got[tuple(bad[0])]} exp {pyr[l][tuple(bad[0])]}")
    kp_p, de_p, co_p, mo_p, cap = ext.outputs()
    cnt = plvi.download(co_p, np.zeros(B, np.int32))
    mono = plvi.download(mo_p, np.zeros(B, np.int32))
    kps = plvi.download(kp_p, np.zeros(B * cap, plvi.KEYPOINT_DTYPE))
    desc = plvi.download(de_p, np.zeros((B * cap, 32), np.uint8))
    for k in range(B):
        assert 0 <= cnt[k] <= cap, f"{tag} frame {k}: count {cnt[k]} of {cap}"
        s = slice(k * cap, k * cap + cnt[k])
        assert_orb_same((int(mono[k]), kps[s], desc[s]), expected(k, w, h, scale, nlevels, compat)[1],
                        f"{tag} frame {k}")
    ext.close()
    del buf


def case_id(c):
    return "{}x{}-s{}-widths_{}".format(c[0], c[1], c[2], "_".join(str(s[0]) for s in level_sizes(*c)))


# (w, h, scale, nlevels): level widths (the ids print them) and their residues mod 4
EDGE_CASES = [
    (307, 100, 1.2, 3),   # 307, 256, 213: one full lane pass; residues 3, 0, 1
    (308, 100, 1.2, 3),   # 308, 257, 214: one quad into the second 256 columns; residues 0, 1, 2
    (614, 110, 1.2, 2),   # 614, 512: exactly one resizer pass of two quads per lane
    (616, 110, 1.2, 2),   # 616, 513: one column into the second pass
    (1024, 170, 1.2, 3),  # 1024, 853, 711: the loader's width limit, two passes per row; residues 0, 1, 3
    (74, 80, 1.2, 2),     # 74, 62: the smallest legal last level; residue 2
]


def test_edge_case_widths():
    """The widths the cases above are chosen for (CPU arithmetic only; the GPU side asserts the same sizes)."""
    widths = [[s[0] for s in level_sizes(*c)] for c in EDGE_CASES]
    assert widths == [[307, 256, 213], [308, 257, 214], [614, 512], [616, 513], [1024, 853, 711], [74, 62]]
    last = {w[-1] % 4 for w in widths}
    assert last == {0, 1, 2, 3}, "the last level (its last row ends the allocation) covers every residue"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", EDGE_CASES, ids=case_id)
def test_lane_and_row_end_edges(plvi_lib, monkeypatch, case, mode):
    """Two frames (synth, binary noise) that fill max_batch: the binary frame's last level ends the
    pyramid allocation, its last quad is partial for three of the four residues."""
    check(case, 2, mode, monkeypatch)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B", [1, 3, 4, 5, 9])
def test_partial_workgroups(plvi_lib, monkeypatch, B, mode):
    """A lone frame, a partial block, a full block, full blocks plus one frame; eight levels."""
    check((320, 240, 1.2, 8), B, mode, monkeypatch)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pad,odd", [(0, False), (3, False), (5, False), (0, True)], ids=["pad0", "pad3", "pad5", "odd_address"])
def test_source_alignment(plvi_lib, monkeypatch, pad, odd, mode):
    check((308, 100, 1.2, 3), 3, mode, monkeypatch, pad=pad, odd_address=odd)


SCALE_CASES = [
    (300, 104, 1.05, 4),  # sy advances by one almost every row
    (322, 240, 2.0, 2),   # area kernels, one tail column
    (200, 160, 2.0, 2),   # area kernels, four tail columns
    (322, 241, 2.0, 2),   # bilinear at x scale 2: a quad's taps span 8 bytes, sy advances by two
    (400, 300, 2.5, 2),   # taps beyond the 8-byte window: the per-pixel path
]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", SCALE_CASES, ids=case_id)
def test_scales(plvi_lib, monkeypatch, case, mode):
    check(case, 2, mode, monkeypatch)


@pytest.mark.parametrize("mode", MODES)
def test_generic_vertical_pass(plvi_lib, monkeypatch, mode):
    """PLVI_COMPAT_RESIZE_V_GENERIC against the oracle under the same switch; it changes the pyramid."""
    case = (320, 240, 1.2, 8)
    a = expected(0, *case, 0)[0][3]
    b = expected(0, *case, plvi.COMPAT_RESIZE_V_GENERIC)[0][3]
    assert a.shape == b.shape and (a != b).any()
    check(case, 3, mode, monkeypatch, compat=plvi.COMPAT_RESIZE_V_GENERIC)


@pytest.mark.parametrize("w,h,scale,nlevels", [
    (1024, 130, 1.2, 3),  # 992 / 98 columns per row of the octree region: 10 roots, above kOrbMaxRoots
    (300, 100, 1.05, 4),  # level 2 is 272 x 91: one cell row of 59 + 6 rows, above kOrbCellMax
])
def test_shapes_the_planner_refuses(plvi_lib, w, h, scale, nlevels):
    """Flatter relatives of the wide cases above are refused by the cell / octree planner, as before
    the quad path; the cases above are the nearest accepted shapes."""
    with pytest.raises(plvi.PlviError) as e:
        plvi.ORBextractor(1000, scale, nlevels, 20, 7, w, h, max_batch=2)
    assert e.value.code == plvi.PLVI_E_BADARG
    assert plvi_lib.plvi_device_synchronize() == 0
