"""region2rect with staged weights (lsd_rect_lanes_kernel): a workgroup first
gathers the modgrad weight of every point of its 256 regions into a weights
array in point order, then lane = region streams them.  Every case compares
the raw segments of each (frame, octave) -- one per region, nothing filtered
-- bitwise with the oracle's flsd output, and the keep-all keylines with the
oracle's extractor; octave 1's oracle runs on the half image the extractor
reports."""
import numpy as np
import pytest

import oracle_lib as ol
import plvi
from plvi import synth
from util import assert_lines_same

pytestmark = pytest.mark.gpu

GRID_LANES = 512  # regions one pass of the two-workgroup grid covers


def checker(w, h, p=16):
    y, x = np.mgrid[0:h, 0:w]
    return np.where(((x // p) + (y // p)) % 2 == 0, 0, 255).astype(np.uint8)


def bars(w, h, p=16):
    """Bars p long and p/2 high on a p-pixel pitch, every other row of bars shifted by one bar."""
    y, x = np.mgrid[0:h, 0:w]
    on = ((y % p) < p // 2) & ((((x + ((y // p) % 2) * p) // p) % 2) == 0)
    return np.where(on, 220, 30).astype(np.uint8)


def long_bar(w=320, h=240):
    img = np.full((h, w), 20, np.uint8)
    img[117:123, 10:310] = 230
    return img


def stripes(w, h, p=2):
    row = np.where((np.arange(w) // p) % 2 == 0, 0, 255).astype(np.uint8)
    return np.tile(row, (h, 1))


class Oracle:
    """Oracle results per distinct image, computed once."""

    def __init__(self):
        self.raw, self.kl = {}, {}

    def lsd_raw(self, img):
        k = (img.shape, img.tobytes())
        if k not in self.raw:
            self.raw[k] = ol.lsd_raw(img)
        return self.raw[k]

    def keylines(self, img):
        k = (img.shape, img.tobytes())
        if k not in self.kl:
            self.kl[k] = ol.line_extract(img, nfeatures=0)
        return self.kl[k]


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def run_and_check(lx, frames, oracle, tag):
    """One batch through lx (keep-all), then every (frame, octave)'s raw
    segments and every frame's keylines against the oracle."""
    frames = np.ascontiguousarray(frames)
    B, h, w = frames.shape
    buf = plvi.DeviceBuffer(frames.nbytes)
    buf.upload(frames)
    lx.extract_batch(buf.ptr, B, w * h, w)
    plvi.load().plvi_device_synchronize()
    assert lx.errors() == 0, tag
    klp, dep, fnp, cop, cap = lx.outputs()
    cnt = plvi.download(cop, np.zeros(lx.max_batch, np.int32))
    kl = plvi.download(klp, np.zeros(lx.max_batch * cap, plvi.KEYLINE_DTYPE))
    de = plvi.download(dep, np.zeros((lx.max_batch * cap, 32), np.uint8))
    fn = plvi.download(fnp, np.zeros((lx.max_batch * cap, 3), np.float64))
    for f in range(B):
        for o in range(2):
            src = frames[f] if o == 0 else lx.pyramid_level(1, frame=f)
            exp = oracle.lsd_raw(src)
            got = lx.debug_raw_lines(o, frame=f)
            assert got.shape == exp.shape, f"{tag} frame {f} octave {o}: {len(got)} segments, oracle {len(exp)}"
            bad = np.flatnonzero((got.view(np.uint32) != exp.view(np.uint32)).any(axis=1))
            assert bad.size == 0, f"{tag} frame {f} octave {o}: segments differ at {bad[:8]}"
        s = slice(f * cap, f * cap + cnt[f])
        assert_lines_same((kl[s], de[s], fn[s]), oracle.keylines(frames[f]), f"{tag} frame {f}")


def variants(img, n):
    """n frames: img and two shifted copies in turn (distinct region lists, few oracle runs)."""
    vs = [img, np.roll(img, (5, 3), (0, 1)), np.roll(img, (11, 7), (0, 1))]
    return np.stack([vs[i % 3] for i in range(n)])


PATTERNS = {"checker": (checker, 320, 240), "bars": (bars, 400, 300)}


@pytest.fixture(scope="module")
def extractors(plvi_lib):
    """One keep-all extractor per (pattern, batch size), made on first use."""
    made = {}

    def get(name, B):
        if (name, B) not in made:
            _, w, h = PATTERNS[name]
            made[name, B] = plvi.Lineextractor(0, 0, 0.8, 2, 2.0, 0, w, h, max_batch=B)
        return made[name, B]

    yield get
    for lx in made.values():
        lx.close()


@pytest.mark.parametrize("B", [1, 17, 64, 65, 300])
@pytest.mark.parametrize("name", ["checker", "bars"])
def test_more_regions_than_one_grid_pass(extractors, oracle, name, B):
    """More than 512 octave-0 regions per frame: the workgroups take a second
    256-region group, with its own staged range.  Batch sizes on both sides of
    the 8- / 2-workgroup grid (16 frames), the two unroll depths (64) and the
    two growth kernels (256)."""
    fn, w, h = PATTERNS[name]
    frames = variants(fn(w, h), B)
    for v in frames[:3]:
        assert len(oracle.lsd_raw(v)) > GRID_LANES
    run_and_check(extractors(name, B), frames, oracle, f"{name} B={B}")


def test_region_longer_than_a_staging_step(plvi_lib, oracle):
    """One bright bar: two regions of several hundred points each and nothing
    else, so a workgroup's range is two regions and 254 lanes have none."""
    img = long_bar()
    exp = oracle.lsd_raw(img)
    assert len(exp) == 2
    assert np.all(np.hypot(exp[:, 2] - exp[:, 0], exp[:, 3] - exp[:, 1]) > 290)
    lx = plvi.Lineextractor(0, 0, 0.8, 2, 2.0, 0, 320, 240, max_batch=2)
    run_and_check(lx, img[None], oracle, "long bar")
    run_and_check(lx, np.stack([img, img[::-1].copy()]), oracle, "long bar x2")


def test_no_regions(plvi_lib, oracle):
    """A flat frame has no region in either octave: alone, and between textured frames."""
    flat = np.full((240, 320), 77, np.uint8)
    assert len(oracle.lsd_raw(flat)) == 0
    lx = plvi.Lineextractor(0, 0, 0.8, 2, 2.0, 0, 320, 240, max_batch=3)
    run_and_check(lx, flat[None], oracle, "flat")
    assert len(lx.debug_raw_lines(0)) == 0 and len(lx.debug_raw_lines(1)) == 0
    run_and_check(lx, np.stack([synth.frame(1, 320, 240), flat, checker(320, 240)]), oracle, "flat in the middle")


@pytest.mark.parametrize("w,h,least", [(330, 250, 256), (96, 64, 64)])
def test_odd_widths(plvi_lib, oracle, w, h, least):
    """Scaled widths (264, 77 and their halves) that are no multiple of a wave, a sector or the staging step."""
    img = synth.frame(3, w, h)
    assert len(oracle.lsd_raw(img)) > least
    lx = plvi.Lineextractor(0, 0, 0.8, 2, 2.0, 0, w, h, max_batch=3)
    run_and_check(lx, img[None], oracle, f"{w}x{h}")
    run_and_check(lx, np.stack([img, synth.frame(4, w, h), img]), oracle, f"{w}x{h} x3")


def test_stale_weights(extractors, oracle):
    """One handle: 65 dense frames, then 3 other frames, then the 65 again.
    A range staged by one batch and read by the next would show here."""
    lx = extractors("checker", 65)
    dense = variants(checker(320, 240), 65)
    other = np.stack([synth.frame(s, 320, 240) for s in (5, 6, 7)])
    run_and_check(lx, dense, oracle, "dense first")
    run_and_check(lx, other, oracle, "other")
    run_and_check(lx, dense, oracle, "dense again")


@pytest.mark.parametrize("B", [1, 65])
def test_more_than_half_the_plane_in_regions(plvi_lib, oracle, B):
    """The weights array holds half a plane of points per (frame, octave); a
    256-region group whose points end beyond that gathers from the modgrad
    plane instead.  2-pixel stripes put the gradient above threshold on 87 %
    of the scaled plane, nearly all of it in full-height regions."""
    img = stripes(320, 240)
    _, ang, _ = ol.lsd_planes(img)
    assert (ang != -1024.0).mean() > 0.8
    lx = plvi.Lineextractor(0, 0, 0.8, 2, 2.0, 0, 320, 240, max_batch=B)
    run_and_check(lx, variants(img, B), oracle, f"stripes B={B}")
