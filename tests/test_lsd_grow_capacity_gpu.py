"""Region growing past its queue, slot and window capacities.

Which path the multi-wave growth kernel (lsd_grow_mw.hpp) takes depends on the
image: how many points a region has (kMwSP = 64 slot points in LDS, kMwGQ =
256 queue entries in LDS, 64 + 2048 = 2112 points a slot holds, 256 + 4096 =
4352 points a grower's queue holds), how far below its seed it reaches (the
kMwRB = 32-row own-mark window) and how many regions a (frame, octave) keeps
(kLsdRawCap = 8192).  The images here are crafted to cross each limit; the
oracle's region census (ol.lsd_regions) proves on the CPU that they do, and
the GPU tests compare every (frame, octave)'s raw segments and every frame's
keylines bit for bit with the oracle, through both growth kernels."""
import ctypes

import numpy as np
import pytest

import oracle_lib as ol
import plvi
from plvi import synth
from util import assert_lines_same, structured_frames

gpu = pytest.mark.gpu

W, H = 320, 240  # the crafted frames: scaled plane 256 x 192, min_reg_size 14

# constants of lsd_grow_mw.hpp / lines_device.h / lines_pipeline.hip the conditions are written against
MW_SP, MW_SLOT_SPILL, MW_GQ, MW_GSPILL, MW_RB = 64, 2048, 256, 4096, 32
MW_WAVES, MW_LOG, MW_MAX_SLOTS, MW_STAT_N = 16, 256, 128, 16
MW_CTL_BYTES = 4 * (12 + MW_STAT_N)          # sizeof(MwCtl)
MW_SLOT_BYTES = 4 * 7 + 4 * MW_SP            # kMwSlotBytes = sizeof(MwSlot) + 4 * kMwSP
LDS_BYTES = 160 * 1024
SLOT_CAP = MW_SP + MW_SLOT_SPILL             # 2112
QUEUE_CAP = MW_GQ + MW_GSPILL                # 4352
RAW_CAP = 8192                               # kLsdRawCap
GROW_ENV = ("PLVI_GROW_MW", "PLVI_GROW_LDS", "PLVI_GROW_RB", "PLVI_GROW_RD", "PLVI_GROW_TPW")


# ----------------------------------------------------------------- crafted images
def ramp_band(y0, y1, x0=100, w=W, h=H):
    """Vertical ramp band clip((x - x0) * 8, 0, 255) on rows y0:y1, 0 elsewhere:
    one region of about 25 points per plane row, as deep as the band."""
    img = np.zeros((h, w), np.uint8)
    img[y0:y1] = np.clip((np.arange(w) - x0) * 8, 0, 255)
    return img


def ramp_rows(x1=W, y0=100, w=W, h=H, lead=False):
    """Horizontal ramp clip((y - y0) * 8, 0, 255) on columns 0:x1, 0 elsewhere:
    one region 25 plane rows deep (inside the own-mark window), about 25
    points per plane column.  lead: a ramp band on rows 0:60 above it, so that
    the walk has a region to resolve first and a grower takes the ramp's."""
    img = np.zeros((h, w), np.uint8)
    img[:, :x1] = np.clip((np.arange(h) - y0) * 8, 0, 255)[:, None]
    if lead:
        img[:60] = ramp_band(0, 60, w=w, h=h)[:60]
    return img


def half_band(y0, hgt, vmax, xe, x0=40, w=W // 2, h=H):
    """A ramp band in a half frame: rows y0:y0+hgt of clip((x - x0) * 8, 0, vmax)
    (its width follows vmax) on columns 0:144, and a partial row below it up to
    column xe."""
    row = np.clip((np.arange(w) - x0) * 8, 0, vmax)
    row[144:] = 0
    img = np.zeros((h, w), np.uint8)
    img[y0:y0 + hgt] = row
    if xe > 0 and y0 + hgt < h:
        img[y0 + hgt, :xe] = row[:xe]
    return img


# (y0, height, vmax, xe) of the left / right half band per threshold T: found by
# a random search on the oracle's census over height, width and the partial
# last row for a region of exactly T / T + 1 points (160 columns = 128 plane
# columns, so the right half resamples as the left one does)
PAIR_PARAMS = {
    64: ((68, 7, 177, 121), (144, 6, 235, 63)),
    256: ((186, 30, 119, 25), (179, 12, 128, 87)),
    2112: ((53, 118, 228, 78), (102, 129, 207, 60)),
    4352: ((7, 221, 250, 66), (7, 231, 238, 35)),
}


def pair_frame(T):
    lo, hi = PAIR_PARAMS[T]
    return np.concatenate([half_band(*lo), half_band(*hi)], axis=1)


def two_giants():
    """Two full-height ramps side by side and a block of synthetic clutter to
    their right: the giants' seeds are in row 0, all the clutter's seeds come
    after them in raster order."""
    x = np.arange(W)
    row = np.where(x >= 92, np.clip((x - 100) * 8, 0, 255), np.clip((x - 20) * 8, 0, 255))
    img = np.tile(row.astype(np.uint8), (H, 1))
    img[:, 190:] = synth.frame(11, W, H)[:, 190:]
    return img


def late_giant():
    """Clutter on the rows above a full-width horizontal ramp: the giant region's
    seed is the last the walk reaches, long after a grower has taken it."""
    img = ramp_rows(y0=150)
    img[:110] = synth.frame(11, W, H)[:110]
    return img


# name -> (image, (size above, size up to), deep?) of the images (a): the largest region of each.  In every
# image a smaller region (the band's upper edge, the lead band) is seeded before it, so the walk is busy
# when the growers start and the large region is grown speculatively.
A_IMAGES = {
    "deep_slot": (lambda: ramp_band(60, 160), (MW_GQ, SLOT_CAP), True),
    "deep_queue": (lambda: ramp_band(40, 200), (SLOT_CAP, QUEUE_CAP), True),
    "deep_giant": (lambda: ramp_band(4, 240), (QUEUE_CAP, 1 << 30), True),
    "shallow_slot": (lambda: ramp_rows(80, lead=True), (MW_GQ, SLOT_CAP), False),
    "shallow_queue": (lambda: ramp_rows(160, lead=True), (SLOT_CAP, QUEUE_CAP), False),
    "shallow_giant": (lambda: ramp_rows(lead=True), (QUEUE_CAP, 1 << 30), False),
}
THRESHOLDS = (MW_SP, MW_GQ, SLOT_CAP, QUEUE_CAP)


def batch_a():
    return np.stack([A_IMAGES[k][0]() for k in A_IMAGES])


def batch_b():
    """The four threshold pairs, then the images (c) and (d) as frames 4 and 5."""
    return np.stack([pair_frame(T) for T in THRESHOLDS] + [two_giants(), late_giant()])


class Oracle:
    """Oracle results per distinct image, computed once and shared by the tests."""

    def __init__(self):
        self.memo = {}

    def _get(self, what, img, fn):
        k = (what, img.shape, img.tobytes())
        if k not in self.memo:
            self.memo[k] = fn(img)
        return self.memo[k]

    def census(self, img):
        return self._get("census", img, ol.lsd_regions)

    def lsd_raw(self, img):
        return self._get("raw", img, lambda i: ol.lsd_raw(i, cap=20000))

    def keylines(self, img):
        return self._get("kl", img, lambda i: ol.line_extract(i, nfeatures=0))


ORACLE = Oracle()


def kept(c):
    return int((c["size"] >= c["min_reg_size"]).sum())


# ----------------------------------------------------------------- CPU: the images meet their conditions
@pytest.mark.parametrize("name", list(A_IMAGES))
def test_census_size_classes(name):
    """Images (a): the largest region lies in its size class, deep (at least 64
    rows below its seed, past the own-mark window) or shallow (inside it)."""
    make, (above, upto), deep = A_IMAGES[name]
    c = ORACLE.census(make())
    assert (c["min_reg_size"] == 14).all()
    i = int(np.argmax(c["size"]))
    r = c[i]
    print(f"{name}: {len(c)} regions, largest {r['size']} points, depth {r['depth']}, "
          f"after regions of {c['size'][:i].tolist()} points")
    assert i > 0 and c["size"][:i].max() > MW_GQ  # a region of some hundred points is resolved before it
    assert above < r["size"] <= upto, r
    assert r["depth"] >= 2 * MW_RB if deep else r["depth"] < MW_RB, r


def threshold_pair(T):
    s = ORACLE.census(pair_frame(T))["size"]
    return int(s[s <= T].max()), int(s[s > T].min())


@pytest.mark.parametrize("T", THRESHOLDS)
def test_census_threshold_pairs(T):
    """Images (b): regions on either side of T, at most 32 points apart (the search aimed at T and T + 1)."""
    lo, hi = threshold_pair(T)
    print(f"threshold {T}: region sizes {lo} and {hi}")
    assert lo <= T < hi and hi - lo <= 32, (T, lo, hi)


def test_census_two_giants():
    """Image (c): two regions beyond a grower's queue with their seeds in the first row, ordinary clutter after."""
    c = ORACLE.census(two_giants())
    g = np.flatnonzero(c["size"] > QUEUE_CAP)
    print(f"two giants: sizes {c['size'][g]}, seeds {c['seed_x'][g]}, {c['seed_y'][g]}; "
          f"{len(c) - g[-1] - 1} regions after them, {kept(c[g[-1] + 1:])} kept")
    assert len(g) == 2 and (c["seed_y"][g] == 0).all()
    after = c[g[-1] + 1:]
    assert len(after) > 500 and kept(after) > 100
    assert after["size"].max() <= SLOT_CAP  # ordinary: every one fits a slot


def test_census_late_giant():
    """Image (d): the region beyond a grower's queue comes after hundreds of others."""
    c = ORACLE.census(late_giant())
    g = np.flatnonzero(c["size"] > QUEUE_CAP)
    print(f"late giant: size {c['size'][g]}, seed row {c['seed_y'][g]}, {g[0]} regions before it, {kept(c[:g[0]])} kept")
    assert len(g) == 1 and g[0] > 500 and kept(c[:g[0]]) > 100
    assert c["seed_y"][g[0]] > 64


def test_census_matches_lsd_raw():
    """The census is flsd's own loop: its kept regions are the raw segments, its seeds come in raster order."""
    for img in (two_giants(), synth.frame(7, W, H)):
        c = ORACLE.census(img)
        assert kept(c) == len(ORACLE.lsd_raw(img))
        pos = c["seed_y"].astype(np.int64) * 4096 + c["seed_x"]
        assert (np.diff(pos) > 0).all()
        assert (c["size"] >= 1).all() and (c["depth"] >= 0).all()


def mw_slots(w, h, lsd_scale=0.8, nlevels=2):
    """LinePipeline::init's sizing of the multi-wave kernel's slot pool (lines_pipeline.hip)."""
    s = float(np.float32(lsd_scale))
    nwords = wpr_max = 0
    for o in range(nlevels):
        sw, sh = int(np.rint((w >> o) * s)), int(np.rint((h >> o) * s))
        wpr = (sw + 31) // 32
        nwords, wpr_max = max(nwords, sh * wpr), max(wpr_max, wpr)
    fixed = MW_CTL_BYTES + 8 * MW_LOG + 4 * (3 * nwords + MW_WAVES * MW_RB * wpr_max + MW_WAVES * MW_GQ)
    return min(MW_MAX_SLOTS, (LDS_BYTES - fixed) // MW_SLOT_BYTES) if fixed < LDS_BYTES else 0


ELIGIBLE, INELIGIBLE = (800, 492), (800, 500)


def test_eligibility_arithmetic():
    """The two frame sizes of the cut-off test lie on either side of mwSlots >= 2 * kMwWaves, the eligible one
    with a pool close to the minimum; the largest frame of the other line tests is far from it."""
    print("slots:", {s: mw_slots(*s) for s in (ELIGIBLE, INELIGIBLE, (752, 480), (W, H))})
    assert mw_slots(*ELIGIBLE) == 34 and mw_slots(*INELIGIBLE) == 29
    assert mw_slots(*INELIGIBLE) < 2 * MW_WAVES <= mw_slots(*ELIGIBLE)
    assert mw_slots(752, 480) == 66 and mw_slots(W, H) == MW_MAX_SLOTS


def dense_checker(w, h, px=10, py=10, ox=0, oy=0):
    y, x = np.mgrid[0:h, 0:w]
    return np.where((((x + ox) // px) + ((y + oy) // py)) % 2 == 0, 0, 255).astype(np.uint8)


# kernel -> (frame size, checker (px, py, ox, oy)): more kept regions in octave 0 than kLsdRawCap.  The
# multi-wave case is the densest of a bounded search (checkers, bricks, bars and diamonds of pitch 8.5 to 12
# in half-pixel steps, two offsets) over the eligible sizes 800 x 492, 752 x 520 and 720 x 544.
CAP_CASES = {"sequential": ((960, 600), (10, 10, 0, 0)), "multi-wave": (ELIGIBLE, (10, 9, 2, 2))}


@pytest.mark.parametrize("kernel", list(CAP_CASES))
def test_census_region_cap(kernel):
    """A dense checkerboard keeps more regions in octave 0 than kLsdRawCap, in a frame only the sequential
    kernel takes and in one the multi-wave kernel takes."""
    (w, h), pat = CAP_CASES[kernel]
    c = ORACLE.census(dense_checker(w, h, *pat))
    print(f"{kernel}: checker {pat} at {w}x{h}: {len(c)} regions, {kept(c)} kept, {mw_slots(w, h)} slots")
    assert kept(c) > RAW_CAP
    assert (mw_slots(w, h) >= 2 * MW_WAVES) == (kernel == "multi-wave")


# ----------------------------------------------------------------- GPU
class Run:
    """One batch through a Lineextractor (keep-all): raw segments per (frame,
    octave), the octave-1 images, keyline tables, error words, stats block."""

    def __init__(self, lx, frames, stats=False):
        frames = np.ascontiguousarray(frames)
        B, h, w = frames.shape
        lib = plvi.load()
        buf = plvi.DeviceBuffer(frames.nbytes)
        buf.upload(frames)
        st = None
        if stats:
            st = plvi.DeviceBuffer(B * 2 * MW_STAT_N * 4)
            st.upload(np.zeros(B * 2 * MW_STAT_N, np.int32))
            lib.plvi_lines_debug_mw_stats(lx._h, ctypes.c_void_p(st.ptr))
        lx.extract_batch(buf.ptr, B, w * h, w)
        lib.plvi_device_synchronize()
        if stats:
            lib.plvi_lines_debug_mw_stats(lx._h, ctypes.c_void_p(0))
            self.stats = plvi.download(st.ptr, np.zeros(B * 2 * MW_STAT_N, np.int32)).reshape(B, 2, MW_STAT_N)
        self.frames = frames
        self.errs = lx.errors(per_frame=True)[:B].copy()
        klp, dep, fnp, cop, cap = lx.outputs()
        cnt = plvi.download(cop, np.zeros(lx.max_batch, np.int32))
        kl = plvi.download(klp, np.zeros(lx.max_batch * cap, plvi.KEYLINE_DTYPE))
        de = plvi.download(dep, np.zeros((lx.max_batch * cap, 32), np.uint8))
        fn = plvi.download(fnp, np.zeros((lx.max_batch * cap, 3), np.float64))
        self.tables = [(kl[f * cap:f * cap + cnt[f]], de[f * cap:f * cap + cnt[f]], fn[f * cap:f * cap + cnt[f]])
                       for f in range(B)]
        self.src = [[frames[f], lx.pyramid_level(1, frame=f)] for f in range(B)]
        self.raw = [[lx.debug_raw_lines(o, frame=f) for o in range(2)] for f in range(B)]

    def check_frame(self, f, tag):
        """Frame f: raw segments of both octaves and the keylines equal the oracle's, no error flag."""
        assert self.errs[f] == 0, f"{tag} frame {f}: error word {self.errs[f]}"
        for o in range(2):
            check_raw(self.raw[f][o], ORACLE.lsd_raw(self.src[f][o]), f"{tag} frame {f} octave {o}")
        assert_lines_same(self.tables[f], ORACLE.keylines(self.frames[f]), f"{tag} frame {f}")

    def check(self, tag):
        for f in range(len(self.frames)):
            self.check_frame(f, tag)

    def check_identity(self, tag):
        """Per (frame, octave): trivial + committed speculative + walker-grown = the
        seeds flsd visits; the walker-grown cover the regrown and the undispatched."""
        for f in range(len(self.frames)):
            for o in range(2):
                s, n = self.stats[f, o], len(ORACLE.census(self.src[f][o]))
                assert s[4] + s[5] + s[12] == n, f"{tag} frame {f} octave {o}: {s[4]} + {s[5]} + {s[12]} != {n}"
                assert s[12] >= s[2] + s[3], f"{tag} frame {f} octave {o}: {s[12]} < {s[2]} + {s[3]}"

    def same_as(self, other, tag):
        for f in range(len(self.frames)):
            for o in range(2):
                assert self.raw[f][o].tobytes() == other.raw[f][o].tobytes(), f"{tag} frame {f} octave {o}"
            for a, b in zip(self.tables[f], other.tables[f]):
                assert a.tobytes() == b.tobytes(), f"{tag} frame {f}"


def check_raw(got, exp, tag):
    assert got.shape == exp.shape, f"{tag}: {len(got)} segments, oracle {len(exp)}"
    bad = np.flatnonzero((got.view(np.uint32) != exp.view(np.uint32)).any(axis=1))
    assert bad.size == 0, f"{tag}: segments differ at {bad[:8]}"


def extractor(monkeypatch, w, h, max_batch, **env):
    """A keep-all extractor made under the given PLVI_GROW_* settings (read when it is made)."""
    for k in GROW_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    return plvi.Lineextractor(0, 0, 0.8, 2, 2.0, 0, w, h, max_batch=max_batch)


def run(monkeypatch, frames, stats=False, **env):
    lx = extractor(monkeypatch, frames.shape[2], frames.shape[1], len(frames), **env)
    try:
        return Run(lx, frames, stats)
    finally:
        lx.close()


@gpu
@pytest.mark.parametrize("which", ["size_classes", "thresholds_and_giants"])
def test_crafted_batch_through_both_kernels(plvi_lib, monkeypatch, which):
    """The crafted frames through the multi-wave kernel, the sequential kernel at
    its default windows and the sequential kernel with a 2-row USED ring (a giant
    region against the smallest ring): each equals the oracle, and the kernels
    each other.  The multi-wave run keeps the accounting identity; over the
    images (c) and (d) the walker regrew at least one region (a giant one
    overflows its grower's queue)."""
    frames = batch_a() if which == "size_classes" else batch_b()
    mw = run(monkeypatch, frames, stats=True, PLVI_GROW_MW=256)
    print("stats [0..5], [12] per (frame, octave):\n", mw.stats[:, :, [0, 1, 2, 3, 4, 5, 12]])
    mw.check("multi-wave")
    mw.check_identity("multi-wave")
    assert mw.stats[:, :, 0].sum() > 0
    seq = run(monkeypatch, frames, PLVI_GROW_MW=0)
    seq.check("sequential")
    ring = run(monkeypatch, frames, PLVI_GROW_MW=0, PLVI_GROW_LDS=6144, PLVI_GROW_RB=2)
    ring.check("sequential, 2-row ring")
    mw.same_as(seq, "multi-wave != sequential")
    ring.same_as(seq, "2-row ring != default windows")
    if which == "thresholds_and_giants":
        assert mw.stats[4:6, :, 2].sum() > 0, mw.stats[4:6, :, :6]


@gpu
def test_stale_marks_after_overflowed_growth(plvi_lib, monkeypatch):
    """One extractor, nothing cleared in between: a batch whose regions overflow
    the growers' queues deep below their seeds (their own marks partly in the
    global spill bitmap when the growth stops), then ordinary frames, then the
    giant batch again.  Every launch equals the oracle: each launch left the
    spill bitmaps zero."""
    giants = np.stack([ramp_band(4, 240), two_giants()])
    plain = np.stack([synth.frame(s, W, H) for s in (5, 6)])
    for img in giants:
        c = ORACLE.census(img)
        assert ((c["size"] > QUEUE_CAP) & (c["depth"] >= 2 * MW_RB)).any()
    lx = extractor(monkeypatch, W, H, 2, PLVI_GROW_MW=256)
    try:
        for tag, frames in (("giants", giants), ("plain", plain), ("giants again", giants), ("plain again", plain)):
            r = Run(lx, frames, stats=True)
            r.check(tag)
            r.check_identity(tag)
            assert r.stats[:, :, 0].sum() > 0, tag
    finally:
        lx.close()


@gpu
@pytest.mark.parametrize("size", [ELIGIBLE, INELIGIBLE])
def test_eligibility_cutoff(plvi_lib, monkeypatch, size):
    """Either side of mwSlots >= 2 * kMwWaves: at 800 x 492 the multi-wave kernel
    runs with a pool of 34 slots, which the thousands of regions of the stripes
    frame starve; at 800 x 500 (29 slots) the sequential kernel runs and the
    stats block stays as uploaded."""
    w, h = size
    frames = np.stack([structured_frames(w, h)["stripes"], synth.frame(7, w, h)])
    assert len(ORACLE.census(frames[0])) > 8000
    r = run(monkeypatch, frames, stats=True, PLVI_GROW_MW=256)
    r.check(f"{w}x{h}")
    if mw_slots(w, h) >= 2 * MW_WAVES:
        assert r.stats[:, :, 0].sum() > 0
        r.check_identity(f"{w}x{h}")
    else:
        assert not r.stats.any()


@gpu
@pytest.mark.parametrize("kernel", list(CAP_CASES))
def test_region_cap(plvi_lib, monkeypatch, kernel):
    """More kept regions than kLsdRawCap in one (frame, octave), under either
    growth kernel: that frame alone reports the overflow, its first 8192
    segments are the oracle's first 8192 (commit order is raster seed order in
    both), and the frames on either side of it in the batch are clean and
    exact."""
    (w, h), pat = CAP_CASES[kernel]
    frames = np.stack([synth.frame(3, w, h), dense_checker(w, h, *pat), synth.frame(4, w, h)])
    exp = ORACLE.lsd_raw(frames[1])
    assert len(exp) > RAW_CAP
    mw = kernel == "multi-wave"
    r = run(monkeypatch, frames, stats=mw, PLVI_GROW_MW=256)
    assert r.errs[1] & 4, r.errs
    assert len(r.raw[1][0]) == RAW_CAP
    check_raw(r.raw[1][0], exp[:RAW_CAP], "checker octave 0")
    check_raw(r.raw[1][1], ORACLE.lsd_raw(r.src[1][1])[:RAW_CAP], "checker octave 1")
    for f in (0, 2):
        r.check_frame(f, "beside the overflowing frame")
    if mw:
        assert r.stats[:, :, 0].sum() > 0
        r.check_identity("region cap")
