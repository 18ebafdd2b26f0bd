"""Every branch of the rectified stereo matchers (csrc/stereo.hip) on crafted pairs.

tests/test_stereo.py feeds the matchers extractor output of plvi.synth.stereo_pair only: 640 x 480, keypoints far
from every border, positive integer disparities.  Here the inputs are built by hand (util.StereoScene,
util.StereoLineSet) so that every branch of Frame::ComputeStereoMatches (src/Frame.cc:1228-1406) and
Frame::ComputeStereoMatches_Lines (:1408-1542) is taken, the median select sees more than one SAD distribution,
the launch shapes vary and the dynamic-LDS bound of stereo_orb_kernel is reached.

Every case names the outcome codes it exists to produce.  Its CPU test proves, from the traced pure-Python
restatement alone (util.py_stereo_traced / py_stereo_lines_traced), that each of them occurs, and that the C++
oracle equals the restatement exactly; the GPU test of the same case compares the HIP path with the oracle
exactly.  The out-of-range inputs (the reference's undefined behaviour, error bits 1 and 2 of the kernel) only
assert the documented error return."""
import functools
import math

import numpy as np
import pytest

import oracle_lib
import util
from util import (ST_ACCEPTED, ST_BORDER_SKIP, ST_CLAMPED, ST_DELTA_RANGE, ST_DISPARITY_RANGE, ST_EDGE_MINIMUM,
                  ST_MAXU_NEG, ST_MEDIAN_REJECTED, ST_NAMES, ST_NO_CANDIDATE, ST_NO_ORB_MATCH)

f32 = np.float32
MBF, MB = f32(47.90639384423901), f32(0.11)  # EuRoC-like bf and baseline: maxD = 435 px
LDS_LIMIT = 150 * 1024  # launch_stereo_orb's bound on the dynamic LDS of stereo_orb_kernel


def _mb_for(max_d):
    """A baseline for which maxD = mbf / mb is about max_d pixels."""
    return f32(float(MBF) / max_d)


# ---------------------------------------------------------------------------------------------- ORB cases
# A builder returns (scene, mb, expect, check): expect = {left keypoint: ST_* before the median test} for the
# hand-placed keypoints, check(tables, ur, dp, codes, info) = the case's further preconditions.
def _none(*_):
    pass


def _case_clamp(identical):
    """Zero disparity: both planes are folds with mirror axes at the multiples of 16 and the keypoints sit on
    the axes at the same position on both sides, so the SADs at incR = +-1 are equal, deltaR is exactly 0,
    disparity exactly 0: the clamp to 0.01 (bestuR = uL - 0.01 in double).  identical: right = left exactly,
    every SAD is 0, the median is 0 and nothing is kept."""
    s = util.StereoScene(41, 2, shift=0, noise=0 if identical else 2, fold=16)
    exp = {}
    for yl in (10, 30, 50, 70):
        for xl in range(16, 145, 16):
            exp[s.add_pair(xl, yl, 0)[0]] = ST_CLAMPED
    for yl in (12, 40, 62):
        for xl in range(16, 113, 16):
            exp[s.add_pair(xl, yl, 1)[0]] = ST_CLAMPED

    def check(t, ur, dp, codes, info):
        kL = t[0]
        assert info["clamped"].all() and (kL["octave"][info["clamped"]] == 1).any()
        if identical:
            assert (info["sad"] == 0).all() and (codes == ST_MEDIAN_REJECTED).all() and (ur == -1).all()
        else:
            keep = codes == ST_CLAMPED
            assert keep.sum() > len(codes) // 2 and (info["sad"] > 0).all()
            assert np.array_equal(ur[keep], (kL["x"][keep].astype(np.float64) - 0.01).astype(np.float32))
            assert (dp[keep] == MBF / f32(0.01)).all()
    return s, MB, exp, check


def _case_at_maxd():
    """disparity == maxD exactly: mbf = 48, mb = 1.5 give maxD = 32, the period of the fold, so a right keypoint
    32 px to the left (uR == minU) sees the same symmetric content: deltaR = 0, disparity = 32, which
    `disparity < maxD` refuses; the keypoints at disparity 0 in the other rows are clamped and kept."""
    s = util.StereoScene(49, 1, shift=0, noise=2, fold=16)
    exp = {}
    for xl in range(48, 145, 16):
        x, y = s.level_xy(xl, 20, 0)
        d = s.desc()
        exp[s.add_left(x, y, 0, d)] = ST_DISPARITY_RANGE
        s.add_right(x - f32(32), y, 0, d)
        exp[s.add_pair(xl, 60, 0)[0]] = ST_CLAMPED

    def check(t, ur, dp, codes, info):
        assert f32(f32(48) / f32(1.5)) == 32 and (info["best"] >= 0).all()
    return s, (f32(1.5), f32(48)), exp, check


def _case_wrong_way():
    """Negative refined disparity: the right content lies 1..4 px to the right of the left one and the right
    keypoint is listed at uR = uL, so the SAD minimum is at incR > 0 and disparity < 0 fails `>= minD`.
    Level 1 holds ordinary matches (so the median test has something to keep)."""
    rows = np.repeat([-1, -2, -3, -4], 24)
    s = util.StereoScene(42, 2, shift=[rows, 3])
    exp = {}
    for k, yl in enumerate((12, 36, 60, 84)):
        for xl in (20, 50, 80, 110, 140):
            exp[s.add_pair(xl, yl, 0, e=-(k + 1))[0]] = ST_DISPARITY_RANGE
    for xl in (20, 45, 70, 95):
        for yl in (15, 45, 66):
            exp[s.add_pair(xl, yl, 1)[0]] = ST_ACCEPTED

    def check(t, ur, dp, codes, info):
        kL, kR = t[0], t[2]
        wrong = np.array([i for i, c in exp.items() if c == ST_DISPARITY_RANGE])
        assert np.array_equal(kL["x"][wrong], kR["x"][info["best"][wrong]])  # listed at uR = uL
    return s, MB, exp, check


def _case_above_maxd():
    """maxD = 3 px: content 5 px away with the right keypoint listed inside the search range (uL - 2) refines
    to a disparity >= maxD; content 2 px away is kept."""
    rows = np.repeat([5, 2], 48)
    s = util.StereoScene(43, 1, shift=[rows])
    exp = {}
    for xl in (20, 45, 70, 95, 120):
        exp[s.add_pair(xl, 20, 0, e=3)[0]] = ST_DISPARITY_RANGE
        exp[s.add_pair(xl, 70, 0)[0]] = ST_ACCEPTED
    return s, _mb_for(3.0), exp, _none


def _case_border():
    """Right keypoints whose scaled column is cols - 11 (the border skip `endu >= cols`) and cols - 12 (the
    last column that is evaluated), on two levels; and SAD minima at the ends of the search range."""
    s = util.StereoScene(44, 2, shift=5)  # the left window of column cols - 6 ends at the level edge
    exp, col = {}, {}
    for lv in (0, 1):
        cols = s.sizes[lv][0]
        for yl in (10, 30, 50):
            iL = s.add_pair(cols - 11 + 5, yl, lv)[0]
            exp[iL], col[iL] = ST_BORDER_SKIP, cols - 11
            iL = s.add_pair(cols - 12 + 5, yl + 8, lv)[0]
            exp[iL], col[iL] = ST_ACCEPTED, cols - 12
            exp[s.add_pair(60, yl + 4, lv)[0]] = ST_ACCEPTED
            exp[s.add_pair(30, yl + 4, lv, e=5)[0]] = ST_EDGE_MINIMUM   # bestincR = -L
            exp[s.add_pair(90, yl + 4, lv, e=-5)[0]] = ST_EDGE_MINIMUM  # bestincR = +L
    d = s.desc()  # a right keypoint left of the image: iniu < 0
    iL = s.add_left(20, 72, 0, d)
    s.add_right(-1.0, 72, 0, d)
    exp[iL], col[iL] = ST_BORDER_SKIP, -1

    def check(t, ur, dp, codes, info):
        kR, inv = t[2], t[7]
        for i, c in col.items():
            r = kR[info["best"][i]]
            assert round(float(f32(r["x"] * inv[r["octave"]]))) == c
    return s, MB, exp, check


def _case_search_bounds():
    """maxD = 20 px.  uR == minU and uR == maxU exactly (both inclusive) and one float beyond each; right
    candidates at octaves -2..+2 around the left one with the best descriptor on the +-2 ones (ignored);
    equal best Hamming distances at different x in one row bucket (the lowest index wins); best distances
    74 (kept) and 75 (thOrbDist)."""
    mb = _mb_for(20.0)
    max_d = f32(MBF / mb)
    rows0 = np.repeat([18, 2, 3, 3], 24)
    s = util.StereoScene(45, 5, shift=[rows0, 3, 3, 3, 3])
    exp, best = {}, {}
    # minU (content 18 px away, listed 20 px away -> incR = +2) and maxU (content 2 px away, listed at uL)
    for xl, beyond in ((60, False), (100, True)):
        d = s.desc()
        u_min = f32(f32(xl) - max_d)
        iL = s.add_left(xl, 12, 0, d)
        best[iL] = s.add_right(np.nextafter(u_min, f32(-np.inf)) if beyond else u_min, 12, 0, d)
        exp[iL] = ST_NO_ORB_MATCH if beyond else ST_ACCEPTED
        d = s.desc()
        iL = s.add_left(xl, 36, 0, d)
        best[iL] = s.add_right(np.nextafter(f32(xl), f32(np.inf)) if beyond else xl, 36, 0, d)
        exp[iL] = ST_NO_ORB_MATCH if beyond else ST_ACCEPTED
    # octaves: left on level 2 (level pixel (40, 32)); the true position is listed on octave 1 at distance 10
    d = s.desc()
    x, y = s.level_xy(40, 32, 2)
    xr, _ = s.level_xy(37, 32, 2)
    xj, _ = s.level_xy(27, 32, 2)  # inside [minU, maxU], 10 level pixels from the content
    iL = s.add_left(x, y, 2, d)
    s.add_right(xj, y, 0, d)
    best[iL] = s.add_right(xr, y, 1, util.flip_bits(d, 10, s.rng))
    s.add_right(xj, y, 2, util.flip_bits(d, 20, s.rng))
    s.add_right(xj, y, 3, util.flip_bits(d, 12, s.rng))
    s.add_right(xj, y, 4, d)
    exp[iL] = ST_ACCEPTED
    # ties at distance 6: true position first / junk position first (12 level pixels off)
    for xl, good_first in ((50, True), (110, False)):
        d = s.desc()
        dr = util.flip_bits(d, 6, s.rng)
        iL = s.add_left(xl, 60, 0, d)
        a = s.add_right(xl - 3 if good_first else xl - 15, 60, 0, dr)
        s.add_right(xl - 15 if good_first else xl - 3, 60, 0, dr)
        best[iL] = a
    # thOrbDist
    exp[s.add_pair(50, 84, 0, flips=74)[0]] = ST_ACCEPTED
    exp[s.add_pair(110, 84, 0, flips=75)[0]] = ST_NO_ORB_MATCH

    def check(t, ur, dp, codes, info):
        for i, r in best.items():
            assert info["best"][i] == (r if exp.get(i) != ST_NO_ORB_MATCH else -1), i
    return s, mb, exp, check


def _case_row_bands():
    """vRowIndices: right y for which y +- 2 * scale is an exact integer (octave 0: integer y; octave 1: y =
    7 - 2.4f and 2 + 2.4f, exact in float), left rows at minr, maxr, minr - 1, maxr + 1, bands that touch row 0
    and row nRows - 1 exactly, a left keypoint at y = -0.5 (row 0) and one with x < 0 in a row with candidates
    (maxU < 0: a plain skip).  Level 1 is as large as level 0, so a left keypoint of octave 1 in the last
    rows still has its window."""
    s = util.StereoScene(46, 2, shift=3, sizes=[(160, 96), (160, 96)])
    exp = {}
    two_four = float(f32(2.0) * s.scale[1])

    def band(xl, y_right, oct_right, lefts):
        d = s.desc()
        s.add_right(xl - 3, y_right, oct_right, d)
        for y_left, code in lefts:
            exp[s.add_left(xl, y_left, 0, d)] = code
    band(40, 40.0, 0, [(38.25, ST_ACCEPTED), (42.75, ST_ACCEPTED), (37.75, ST_NO_CANDIDATE), (43.25, ST_NO_CANDIDATE)])
    band(80, 60.5, 0, [(58.25, ST_ACCEPTED), (63.75, ST_ACCEPTED), (57.75, ST_NO_CANDIDATE), (64.25, ST_NO_CANDIDATE)])
    band(120, 7.0 - two_four, 1, [(7.25, ST_ACCEPTED), (8.25, ST_NO_CANDIDATE)])   # band 2..7, maxr exact
    band(60, 2.0 + two_four, 1, [(7.75, ST_ACCEPTED), (8.75, ST_NO_CANDIDATE)])    # band 2..7, minr exact
    band(100, 2.0, 0, [(4.6, ST_ACCEPTED)])                                         # band 0..4
    d = s.desc()
    s.add_right(f32(f32(57) * s.scale[1]), 93.0, 0, d)                               # band 91..95 = nRows - 1
    exp[s.add_left(f32(f32(60) * s.scale[1]), 91.4, 1, d)] = ST_ACCEPTED
    exp[s.add_left(30, -0.5, 0, s.desc())] = ST_NO_ORB_MATCH
    exp[s.add_left(-1.0, 40.25, 0, s.desc())] = ST_MAXU_NEG

    def check(t, ur, dp, codes, info):
        b = {tuple(r) for r in info["band"].tolist()}
        assert b == {(38, 42), (58, 63), (2, 7), (0, 4), (91, 95)}, b
        y = t[2]["y"].astype(np.float64)
        assert y[2] + two_four == 7.0 and y[3] - two_four == 2.0  # exact in float and in double
    return s, MB, exp, check


def _median_scene(seed, n_drop):
    noise = np.repeat([1, 2, 5, 12], 24)
    s = util.StereoScene(seed, 2, shift=4, noise=[noise, 2])
    exp = {}
    cells = [(xl, yl) for yl in (8, 16, 30, 40, 54, 64, 78, 88) for xl in range(20, 141, 15)]
    for xl, yl in cells[:len(cells) - n_drop]:
        exp[s.add_pair(xl, yl, 0)[0]] = ST_ACCEPTED
    return s, exp


def _case_median(n_drop):
    """Median select on SADs from four noise levels: at least 3 distinct high bytes, several values in the
    median's high-byte bucket, a run of equal SADs across the median position (copies of the keypoint that
    holds the median), rejected and kept matches; n_drop makes the count odd or even."""
    s, exp = _median_scene(47, n_drop)
    t = s.tables()
    _, _, _, info = util.py_stereo_traced(*t, MB, MBF)
    order = np.argsort(info["sad"], kind="stable")
    med = int(info["sad_idx"][order[len(order) // 2]])
    for _ in range(4):
        s.add_left(t[0]["x"][med], t[0]["y"][med], 0, t[1][med])

    def check(t, ur, dp, codes, info):
        sad = np.sort(info["sad"])
        k = len(sad) // 2
        assert len(sad) % 2 == n_drop % 2 and len(sad) > 60
        assert len(set(sad >> 8)) >= 3
        assert len(set(sad[(sad >> 8) == (sad[k] >> 8)])) >= 2
        assert sad[k - 1] == sad[k] == sad[k + 1]
        assert any((a >> 8) + 1 == (b >> 8) and b - a < 32 for a, b in zip(sad, sad[1:]))  # e.g. 252 | 262
        assert (codes == ST_MEDIAN_REJECTED).any() and (codes == ST_ACCEPTED).any()
    return s, MB, {}, check


def _case_median_small(n):
    """nacc == 1 and nacc == 2: the median is the only / the larger SAD (vDistIdx[n / 2]) and everything is kept;
    the two SADs differ by more than 2.1, so the smaller one as median would reject the larger."""
    noise = np.repeat([1, 2, 5, 12], 24)
    s = util.StereoScene(48, 1, shift=4, noise=[noise])
    exp = {s.add_pair(40 + 30 * i, 16 + 48 * i, 0)[0]: ST_ACCEPTED for i in range(n)}

    def check(t, ur, dp, codes, info):
        assert len(info["sad"]) == n and (codes == ST_ACCEPTED).all()
        assert n == 1 or info["sad"].max() > 2.2 * info["sad"].min() > 0
    return s, MB, exp, check


def _random_scene(seed, n_rows, n_l, n_r, nlevels, max_oct):
    """n_r right keypoints on random level pixels, the first min(n_l, n_r) left keypoints their partners, the
    rest of either side unrelated."""
    s = util.StereoScene(seed, nlevels, h0=n_rows, shift=3)
    rng = s.rng
    for i in range(max(n_l, n_r)):
        o = int(rng.integers(0, max_oct + 1))
        w, h = s.sizes[o]
        xl, yl = int(rng.integers(14, w - 12)), int(rng.integers(5, h - 5))
        x, y = s.level_xy(xl, yl, o)
        xr, _ = s.level_xy(xl - 3, yl, o)
        d = s.desc()
        if i < n_l:
            s.add_left(x, y, o, d)
        if i < n_r:
            s.add_right(xr, y, o, d)
    return s


def _case_shape(n_rows, n_l, n_r):
    """Launch shapes: the block scan runs over nRows + 1 entries, the per-keypoint loops over nL and nR, the
    SAD stage over more jobs than the four waves."""
    s = _random_scene(50 + n_l, n_rows, n_l, n_r, 3, 2)

    def check(t, ur, dp, codes, info):
        assert t[4][0].shape[0] == n_rows and len(t[0]) == n_l and len(t[2]) == n_r
        assert (codes == ST_ACCEPTED).sum() >= min(n_l, n_r) // 2
        assert n_l <= n_r or (codes == ST_NO_ORB_MATCH).any() or (codes == ST_NO_CANDIDATE).any()
    return s, MB, {}, check


LDS_ROWS, LDS_LEVELS = 300, 8


def lds_limit_count(n_rows=LDS_ROWS, nlevels=LDS_LEVELS):
    """The largest nL = nR whose stereo_orb_kernel launch stays within the 150 KiB bound."""
    n = 1
    while util.stereo_lds_bytes(n_rows, n + 1, n + 1, nlevels) <= LDS_LIMIT:
        n += 1
    return n


def _case_lds_limit():
    """The largest launch launch_stereo_orb accepts at 300 rows and 8 levels (dynamic LDS just under 150 KiB)."""
    n = lds_limit_count()
    s = _random_scene(60, LDS_ROWS, n, n, LDS_LEVELS, 2)

    def check(t, ur, dp, codes, info):
        assert util.stereo_lds_bytes(LDS_ROWS, n, n, LDS_LEVELS) <= LDS_LIMIT < util.stereo_lds_bytes(
            LDS_ROWS, n + 1, n + 1, LDS_LEVELS)
        assert util.stereo_lds_bytes(LDS_ROWS, n, n, LDS_LEVELS) > 64 * 1024
        assert (codes == ST_ACCEPTED).sum() > n // 2
    return s, MB, {}, check


ORB_CASES = {
    "clamp_noise": (lambda: _case_clamp(False), {ST_CLAMPED}),
    "clamp_identical": (lambda: _case_clamp(True), {ST_MEDIAN_REJECTED}),
    "at_maxd": (_case_at_maxd, {ST_DISPARITY_RANGE, ST_CLAMPED}),
    "wrong_way": (_case_wrong_way, {ST_DISPARITY_RANGE, ST_ACCEPTED}),
    "above_maxd": (_case_above_maxd, {ST_DISPARITY_RANGE, ST_ACCEPTED}),
    "border": (_case_border, {ST_BORDER_SKIP, ST_EDGE_MINIMUM, ST_ACCEPTED}),
    "search_bounds": (_case_search_bounds, {ST_NO_ORB_MATCH, ST_ACCEPTED}),
    "row_bands": (_case_row_bands, {ST_NO_CANDIDATE, ST_NO_ORB_MATCH, ST_MAXU_NEG, ST_ACCEPTED}),
    "median_odd": (lambda: _case_median(1), {ST_MEDIAN_REJECTED, ST_ACCEPTED}),
    "median_even": (lambda: _case_median(0), {ST_MEDIAN_REJECTED, ST_ACCEPTED}),
    "median_one": (lambda: _case_median_small(1), {ST_ACCEPTED}),
    "median_two": (lambda: _case_median_small(2), {ST_ACCEPTED}),
    "shape_48_1_1": (lambda: _case_shape(48, 1, 1), {ST_ACCEPTED}),
    "shape_97_63_33": (lambda: _case_shape(97, 63, 33), {ST_ACCEPTED}),
    "shape_97_65_65": (lambda: _case_shape(97, 65, 65), {ST_ACCEPTED}),
    "shape_300_257_255": (lambda: _case_shape(300, 257, 255), {ST_ACCEPTED}),
    "shape_300_700_701": (lambda: _case_shape(300, 700, 701), {ST_ACCEPTED}),
    "lds_limit": (_case_lds_limit, {ST_ACCEPTED}),
}


@functools.lru_cache(maxsize=None)
def orb_case(name):
    """The case's tables, its traced restatement and the oracle's answer, computed once for the CPU and the
    GPU test."""
    build, produces = ORB_CASES[name]
    s, mb, exp, check = build()
    mb, mbf = mb if isinstance(mb, tuple) else (mb, MBF)
    t = s.tables()
    ur, dp, codes, info = util.py_stereo_traced(*t, mb, mbf)
    ref = oracle_lib.stereo_match(*t, mb, mbf)
    return {"t": t, "mb": mb, "mbf": mbf, "exp": exp, "check": check, "produces": produces,
            "py": (ur, dp, codes, info), "ref": ref}


@pytest.mark.parametrize("name", list(ORB_CASES))
def test_orb_case_takes_its_branches_and_oracle_matches_restatement(name):
    c = orb_case(name)
    ur, dp, codes, info = c["py"]
    seen = set(codes.tolist()) | set(info["pre"].tolist())
    missing = [ST_NAMES[k] for k in c["produces"] - seen]
    assert not missing, f"{name}: no left keypoint came out {missing}"
    assert ST_DELTA_RANGE not in seen  # unreachable (see stereo.hip)
    for i, code in c["exp"].items():
        assert info["pre"][i] == code, f"{name}: left keypoint {i} is {ST_NAMES[info['pre'][i]]}, not {ST_NAMES[code]}"
    c["check"](c["t"], ur, dp, codes, info)
    n, our, odp = c["ref"]
    assert n == int((dp > 0).sum())
    assert np.array_equal(our, ur) and np.array_equal(odp, dp)


def test_orb_cases_cover_every_outcome():
    seen = set()
    for name in ORB_CASES:
        _, _, codes, info = orb_case(name)["py"]
        seen |= set(codes.tolist()) | set(info["pre"].tolist())
    assert seen == set(range(len(ST_NAMES))) - {ST_DELTA_RANGE}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ORB_CASES))
def test_orb_case_gpu_matches_oracle(name):
    import plvi
    c = orb_case(name)
    n, ur, dp = c["ref"]
    got = plvi.ComputeStereoMatches(*c["t"], c["mb"], c["mbf"])
    assert got[0] == n
    assert np.array_equal(got[1].view(np.uint32), ur.view(np.uint32))
    assert np.array_equal(got[2].view(np.uint32), dp.view(np.uint32))


@pytest.mark.gpu
def test_orb_one_keypoint_past_the_lds_bound_is_badarg():
    """launch_stereo_orb refuses the launch (no kernel runs) one keypoint per side above the largest case."""
    import plvi
    n = lds_limit_count() + 1
    s = util.StereoScene(61, LDS_LEVELS, h0=LDS_ROWS)
    x, y = s.level_xy(40, 40, 0)
    for _ in range(n):
        s.add_left(x, y, 0, np.zeros(32, np.uint8))
        s.add_right(x, y, 0, np.zeros(32, np.uint8))
    with pytest.raises(plvi.PlviError) as e:
        plvi.ComputeStereoMatches(*s.tables(), MB, MBF)
    assert e.value.code == plvi.PLVI_E_BADARG


# ------------------------------------------------------------------------------- out-of-range ORB inputs
def _oor(kind):
    """One valid pair plus one input the reference handles with undefined behaviour or an assert."""
    s = util.StereoScene(70, 2, shift=3)
    s.add_pair(60, 40, 0)
    d = s.desc()
    if kind == "band_top":        # minr = -1
        s.add_right(50, 1.0, 0, d)
    elif kind == "band_bottom":   # maxr = nRows
        s.add_right(50, 94.0, 0, d)
    elif kind == "left_row_high":  # vRowIndices[nRows]
        s.add_left(50, 96.0, 0, d)
    elif kind == "left_row_negative":  # (size_t)vL of y <= -1
        s.add_left(50, -1.0, 0, d)
    elif kind == "left_window":   # colRange(-2, 9) of the left level
        s.add_left(3, 40, 0, d)
        s.add_right(2, 40, 0, d)
    elif kind == "left_window_right":   # colRange(152, 163) of a 160-column level
        s.add_left(157, 40, 0, d)
        s.add_right(140, 40, 0, d)
    elif kind == "left_window_top":     # rowRange(-2, 9)
        s.add_left(60, 3, 0, d)
        s.add_right(50, 3, 0, d)
    elif kind == "left_window_bottom":  # rowRange(88, 99) of a 96-row level
        s.add_left(60, 93, 0, d)
        s.add_right(50, 93, 0, d)
    elif kind == "right_window":  # colRange(-2, 9) of the right level at incR = -5
        s.add_left(30, 40, 0, d)
        s.add_right(8, 40, 0, d)
    return s.tables()


OOR_KINDS = ("band_top", "band_bottom", "left_row_high", "left_row_negative", "left_window", "left_window_right",
             "left_window_top", "left_window_bottom", "right_window")


@pytest.mark.parametrize("kind", OOR_KINDS)
def test_orb_out_of_range_oracle_gives_up(kind):
    assert oracle_lib.stereo_match(*_oor(kind), MB, MBF)[0] == -1


@pytest.mark.gpu
@pytest.mark.parametrize("kind", OOR_KINDS)
def test_orb_out_of_range_reports_overflow(kind):
    import plvi
    with pytest.raises(plvi.PlviError) as e:
        plvi.ComputeStereoMatches(*_oor(kind), MB, MBF)
    assert e.value.code == plvi.PLVI_E_OVERFLOW


# --------------------------------------------------------------------------------------------- line cases
SL, OV = util.SL_NAMES, util.OV_NAMES
FRAMES = ((640, 480), (752, 480), (1241, 376))


def line_zoo(W, H):
    """One frame of hand-built stereo lines.  Returns (StereoLineSet, {left line: (SL_* code, OV_* arm)}).
    The overlap and disparity pairs are vertical lines 10 px apart (one x slot each, upper half of the frame),
    so only the y extents / the x offsets decide; the horizontal ones lie along the top row and at y = 300."""
    z = util.StereoLineSet(W * 7 + H)
    exp = {}
    slots = iter(range(40, W - 40, 28))

    def vert(ly, ry, code, arm, lx=(10.0, 10.0), rx=(0.0, 0.0), snap=False):
        x = float(next(slots))
        if snap:  # 0.2 cells into its grid column, so that x + 3 px lies in the same column
            x = (math.floor(x * 64 / W) + 0.2) * W / 64
        iL, _ = z.pair((x + lx[0], ly[0], x + lx[1], ly[1]), (x + rx[0], ry[0], x + rx[1], ry[1]))
        exp[iL] = (code, arm)
        return iL
    A, P, C, D, S, N = (util.SL_ACCEPTED, util.OV_PARTIAL, util.OV_CONTAINED, util.OV_DISJOINT,
                        util.OV_SHORT_LENGTH, util.OV_NONE)
    OR, RR, MR = util.SL_OVERLAP_REJECT, util.SL_RATIO_REJECT, util.SL_MIN_DISP_REJECT
    # lineSegmentOverlapStereo arms
    vert((160, 200), (100, 150), OR, D)           # right above left: epn < sln
    vert((100, 140), (150, 200), OR, S)           # right below left: spn > eln, so length < 0 as well
    vert((100, 200), (90, 210), A, C)
    vert((100, 200), (80, 180), OR, P)            # 80 / 120
    vert((100, 200), (120, 230), A, P)            # 80 / 80: overlap == 1
    vert((100, 200), (200 - 0.0101, 260), A, P)   # length just above 0.01f: 1
    vert((100, 200), (200 - 0.0099, 260), OR, S)  # length just below
    hundredth = f32(0.01)
    vert((-0.2, hundredth), (0.0, 0.3), OR, S)                          # length == (double)0.01f: not above
    vert((-0.2, np.nextafter(hundredth, f32(1))), (0.0, 0.3), A, P)     # one float above: overlap 1
    vert((100, 200), (66.666, 200), OR, P)        # 100 / 133.334 < 0.75f
    vert((100, 200), (66.667, 200), A, P)         # 100 / 133.333 > 0.75f
    vert((100, 200), (100, 200), A, P)            # identical extents: 1
    vert((200, 100), (210, 90), A, C)             # both given end before start
    # filterLineSegmentDisparity
    vert((100, 200), (100, 200), MR, P, lx=(0.0, 0.0), rx=(3.0, 3.0), snap=True)  # both disparities negative (-3, -3)
    vert((100, 200), (100, 200), RR, P, lx=(0.0, 6.0), rx=(3.0, 3.0), snap=True)  # mixed sign (-3, +3)
    vert((100, 200), (100, 200), RR, P, lx=(10.0, 6.99))                   # ratio 0.699
    vert((100, 200), (100, 200), A, P, lx=(10.0, 7.01))                    # ratio 0.701
    one = vert((100, 200), (100, 200), A, P, lx=(1.0, 1.0))                # disparity exactly 1.0
    vert((100, 200), (100, 200), MR, P, lx=(0.999, 0.999))
    quirk = vert((100, 200), (200, 100), MR, P)   # spl(1) == epr(1): the updated sp_r makes ep_r 0 / 0
    # horizontal lines: the left |dy| at 0.05, exactly 0.1f, one float above; along the top row
    tenth = f32(0.1)
    HL, HR = util.SL_HORIZONTAL_LEFT, util.SL_HORIZONTAL_RIGHT
    for k, (dy, code) in enumerate(((f32(0.05), HL), (tenth, HL), (np.nextafter(tenth, f32(1)), A))):
        x = 60.0 + k * W / 4
        exp[z.pair((x, 0.0, x + 60, dy), (x - 10, 0.0, x + 50, dy))[0]] = (code, N if code == HL else P)
    # the right line exactly horizontal (division by zero: inf, NaN), within 0.1 of it, and of zero length
    y0 = 300.0
    x = 60.0
    exp[z.pair((x, y0 - 1, x + 60, y0 + 1), (x - 10, y0, x + 50, y0))[0]] = (HR, P)
    x += W / 4
    exp[z.pair((x, y0, x + 60, y0 + 0.5), (x - 10, y0, x + 50, y0))[0]] = (HR, P)
    x += W / 4
    exp[z.pair((x, y0 - 1, x + 60, y0 + 1), (x - 10, y0, x + 50, y0 + 0.05))[0]] = (HR, P)
    zl = z.pair((32.0, y0 + 29, 33.0, y0 + 31), (30.0, y0 + 30, 30.0, y0 + 30))[0]
    exp[zl] = (HR, P)
    # GridStructure: right lines partly and wholly outside the frame, steep, end before start, negative left
    # coordinates (line_2d truncates toward zero), many lines through one cell
    z.pair((-8.0, 232.0, 50.0, 290.0), (-30.0, 220.0, 40.0, 290.0))
    # both left end points in (-10, 0): grid column 0 by truncation (floor would give -1 and an empty window);
    # the right line lies in column 0 only.  Likewise the last grid column and the last grid row.
    # (the short right line is only within reach of the left start point's window)
    exp[z.pair((-8.0, 100.0, -2.0, 160.0), (4.0, 100.0, 4.0, 104.0))[0]] = (MR, P)
    exp[z.pair((W - 6.0, 100.0, W - 2.0, 140.0), (W - 8.0, 100.0, W - 4.0, 140.0))[0]] = (A, P)
    exp[z.pair((W / 2 + 10, H - 6.0, W / 2 + 50, H - 2.0), (W / 2, H - 6.0, W / 2 + 40, H - 2.0))[0]] = (A, P)
    z.pair((100.0, -6.0, 160.0, 40.0), (90.0, -6.0, 150.0, 40.0))
    z.pair((W - 30.0, 250.0, W - 1.0, 340.0), (W - 40.0, 250.0, W + 60.0, 340.0 + 210))
    z.right((W + 20.0, 50.0, W + 90.0, 90.0))
    z.right((-100.0, -50.0, -20.0, -10.0))
    z.right((100.0, H + 10.0, 200.0, H + 60.0))
    z.right((200.0, -40.0, 260.0, -15.0))
    z.pair((W / 2 + 10, 230.0, W / 2 + 40, H - 10.0), (W / 2, 230.0, W / 2 + 30, H - 10.0))      # steep
    z.pair((W / 2 + 110, H - 20.0, W / 2 + 70, 240.0), (W / 2 + 100, H - 20.0, W / 2 + 60, 240.0))  # end first
    cx, cy = 48.5 * W / 64, 37.5 * H / 48  # the middle of grid cell (48, 37)
    for k in range(24):
        a = math.pi * k / 24
        seg = (cx - 60 * math.cos(a), cy - 60 * math.sin(a), cx + 60 * math.cos(a), cy + 60 * math.sin(a))
        if k % 6 == 1:
            z.pair((seg[0] + 10, seg[1], seg[2] + 10, seg[3]), seg)
        else:
            z.right(seg)
    exp[z.left((W / 3, 330.0, W / 3 + 5, 360.0))] = (util.SL_UNMATCHED, N)
    # mvle_l: one degenerate undistorted line (start == end)
    z.un[one] = (77.0, 55.0, 77.0, 55.0)
    return z, exp, {"quirk": quirk, "one": one, "degenerate": one, "zero_length": zl}


@functools.lru_cache(maxsize=None)
def line_case(W, H, hint):
    z, exp, marks = line_zoo(W, H)
    kl, dl, kr, dr, un = z.tables()
    py = util.py_stereo_lines_traced(kl, dl, kr, dr, W, H, MBF, klUn=un, range_hint=hint)
    ref = oracle_lib.stereo_lines(kl, dl, kr, dr, un, W, H, MBF, range_hint=hint)
    return {"t": (kl, dl, kr, dr, un), "exp": exp, "marks": marks, "py": py, "ref": ref}


def _same_f64(a, b):
    """Bitwise equal except that a NaN matches any NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])


@pytest.mark.parametrize("hint", [0, 1])
@pytest.mark.parametrize("W,H", FRAMES)
def test_line_zoo_takes_its_branches_and_oracle_matches_restatement(W, H, hint):
    c = line_case(W, H, hint)
    m12, disp, dep, codes, info = c["py"]
    for i, (code, arm) in c["exp"].items():
        assert (codes[i], info["arm"][i]) == (code, arm), \
            f"left line {i}: {SL[codes[i]]}/{OV[info['arm'][i]]}, not {SL[code]}/{OV[arm]}"
    assert set(codes.tolist()) == set(range(len(SL))) and set(info["arm"].tolist()) == set(range(len(OV)))
    mk = c["marks"]
    assert info["quirk"][mk["quirk"]] and info["quirk"].sum() == 1
    assert tuple(disp[mk["one"]]) == (1.0, 1.0)
    assert info["cells_outside"] > 30 and info["max_cell"] >= 16
    d = info["disp"]
    assert (np.isinf(d).any(1) & (m12 >= 0)).any() and (np.isnan(d).any(1) & (m12 >= 0)).any()
    assert ((d < 0).all(1)).any() and ((d[:, 0] < 0) & (d[:, 1] > 0)).any()
    assert np.isnan(info["le"][mk["degenerate"]]).any()
    assert np.isfinite(np.delete(info["le"], mk["degenerate"], 0)).all()
    kl = c["t"][0]
    assert (kl["startPointX"] < 0).any() and (kl["startPointY"] < 0).any()
    n, om, odisp, odep, ole = c["ref"]
    assert n == int((codes == util.SL_ACCEPTED).sum()) == int((disp[:, 0] >= 0).sum())
    assert np.array_equal(om, m12)
    assert np.array_equal(odisp, disp) and np.array_equal(odep, dep)
    assert _same_f64(ole, info["le"])


@pytest.mark.gpu
@pytest.mark.parametrize("hint", [0, 1])
@pytest.mark.parametrize("W,H", FRAMES)
def test_line_zoo_gpu_matches_oracle(W, H, hint):
    import plvi
    c = line_case(W, H, hint)
    kl, dl, kr, dr, un = c["t"]
    n, m, disp, dep, le = c["ref"]
    got = plvi.ComputeStereoMatches_Lines(kl, dl, kr, dr, un, W, H, MBF, range_hint=hint)
    assert got[0] == n
    assert np.array_equal(got[1], m)
    assert np.array_equal(got[2].view(np.uint32), disp.view(np.uint32))
    assert np.array_equal(got[3].view(np.uint32), dep.view(np.uint32))
    assert _same_f64(got[4], le)


def _small_lines():
    z = util.StereoLineSet(5)
    z.pair((110.0, 100.0, 110.0, 200.0), (100.0, 90.0, 100.0, 210.0))
    z.pair((310.0, 300.0, 380.0, 420.0), (290.0, 300.0, 360.0, 420.0))
    z.left((500.0, 100.0, 520.0, 160.0))
    return z.tables()


@pytest.mark.gpu
@pytest.mark.parametrize("short", [0, 1])
def test_lines_batch_idx_cap_boundary(short):
    """idx_cap equal to the first frame's grid-entry total fits and equals the oracle; one less raises error
    bit 4 for that frame while the second, small frame of the batch still equals the oracle."""
    import plvi
    import batch_pack as bp
    W, H = FRAMES[0]
    big, small = line_case(W, H, 0)["t"], _small_lines()
    total = line_case(W, H, 0)["py"][4]["grid_total"]
    frames = (big, small)
    assert util.py_stereo_lines_traced(*small[:4], W, H, MBF)[4]["grid_total"] < total - 1
    cl, cr = len(big[0]), len(big[2])
    idx_cap = total - short

    def pack(k, cap, dtype, tail=()):
        out = np.zeros((2, cap) + tail, dtype)
        for f, t in enumerate(frames):
            out[f, :len(t[k])] = t[k]
        return out
    dev = bp.Device()
    sb = plvi.stereo_lines_scratch_bytes(2, cl, cr, idx_cap)
    scratch = dev.up(np.zeros(sb, np.uint8))
    m12, get_m = dev.canary(2, cl)
    disp, get_d = dev.canary(2, cl, 2)
    dep, get_z = dev.canary(2, cl, 2)
    le, get_le = dev.canary(2, cl, 6)
    ns, get_n = dev.canary(2)
    err, get_err = dev.table(np.zeros(1, np.int32))
    plvi.stereo_lines_batch(2, dev.up(pack(0, cl, plvi.KEYLINE_DTYPE)).value,
                            dev.up(pack(1, cl, np.uint8, (32,))).value,
                            dev.up(np.array([len(t[0]) for t in frames], np.int32)).value, cl,
                            dev.up(pack(2, cr, plvi.KEYLINE_DTYPE)).value, dev.up(pack(3, cr, np.uint8, (32,))).value,
                            dev.up(np.array([len(t[2]) for t in frames], np.int32)).value, cr,
                            dev.up(pack(4, cl, plvi.KEYLINE_DTYPE)).value, W, H, MBF, 0, idx_cap, scratch.value, sb,
                            m12.value, disp.value, dep.value, le.value, ns.value, err.value)
    assert get_err()[0] == (4 if short else 0)
    gm, gd, gz, gl, gn = get_m(), get_d(), get_z(), get_le(), get_n()
    for f, t in enumerate(frames):
        if short and f == 0:
            continue
        n, m, d, z, l_ = oracle_lib.stereo_lines(t[0], t[1], t[2], t[3], t[4], W, H, MBF)
        k = len(m)
        assert gn[f] == n and np.array_equal(gm[f, :k], m)
        assert np.array_equal(gd[f, :k], d.view(np.int32)) and np.array_equal(gz[f, :k], z.view(np.int32))
        assert _same_f64(np.ascontiguousarray(gl[f, :k]).view(np.float64), l_)
