"""Every branch of the tracking projection matchers (csrc/proj.hip, csrc/grid_search.h) on crafted scenes.

tests/test_projection.py, test_projection_stereo.py and test_local_stereo.py feed the five guided searches of
tracking random scenes only.  Here the inputs are built by hand (util.ProjScene: keypoints in isolated spots,
descriptors with chosen bits flipped, projections exact in float) so that the sequential dependencies the
kernels' three-part schedule has to reproduce really occur -- a point re-scanned because its best was taken, a
chain of them, the second candidate taken, an overwrite of an unblocking point, the stereo partner that
un-blocks a keypoint -- and so that the equality edges of GetFeaturesInArea, the mvuRight test, TH_HIGH, the
float ratio product, the rotation bin and ComputeThreeMaxima are hit exactly.

Every case names the outcome codes (util.PJ_*) it exists to produce.  The CPU tests prove from the traced
pure-Python restatements (util.py_proj_traced / py_local_traced / py_reloc_traced) that each of them occurs, that
the C++ oracle equals the restatement exactly, that all codes / window returns / ComputeThreeMaxima branches are
covered per kernel, and that every mistake of util.PJ_MUTANTS changes the expected answer of at least one case.
The GPU tests compare the HIP path with the oracle exactly, case by case through the host forms and all cases of
a kernel as batches (tests/batch_pack.py: poisoned padding, canary outputs)."""
import ctypes
import functools

import numpy as np
import pytest

import util
from util import (PJ_ACCEPTED, PJ_ACCEPTED_AFTER_RESCAN, PJ_ACCEPTED_BY_LEVEL, PJ_ALL_BLOCKED, PJ_BAD_LEVEL,
                  PJ_BEHIND, PJ_DEPTH_RANGE, PJ_EMPTY_WINDOW, PJ_LOST_AFTER_RESCAN, PJ_MIRRORED, PJ_NAMES,
                  PJ_NOT_SEARCHED, PJ_OUT_OF_BOUNDS, PJ_OVER_THRESHOLD, PJ_OVERWROTE, PJ_RATIO_REJECTED,
                  PJ_ROT_DROPPED, PJ_SIDE_SKIPPED, PJ_UNBLOCKED_PARTNER, PJ_WINDOW_ABOVE, PJ_WINDOW_BELOW,
                  PJ_WINDOW_LEFT, PJ_WINDOW_RIGHT)

f32 = np.float32
KINDS = util.ProjScene.KINDS
F2F, LOCAL, HIST = ("proj", "proj2"), ("local", "local2"), ("proj", "proj2", "reloc")
W, H = 752, 480
RIGHT0 = 400  # the right image's content sits on spots RIGHT0.. (the left image's on 0..): never on one pixel


def call(kind, **kw):
    """The call's parameters: radius 3 (frame-to-frame, relocalization) or 2.5 (local) at level 0."""
    c = {"th": 1.0 if kind in LOCAL else 3.0, "forward": 0, "backward": 0, "ori": 1, "nnratio": 0.9, "orb_dist": 100}
    c.update(kw)
    return c


def radius(kind, L, th=None):
    sf = util.orb_scale_factors()
    if kind in LOCAL:
        r = f32(2.5) if th in (None, 1.0) else f32(f32(2.5) * f32(th))
        return f32(r * sf[L])
    return f32(f32(3.0 if th is None else th) * sf[L])


def spot(k, pitch=16):
    """Spot k of a lattice: keypoints within 2 px of it are out of every other spot's window up to level 7."""
    per_row = 640 // pitch
    return f32(40 + pitch * (k % per_row)), f32(40 + pitch * (k // per_row))


def sides(s):
    return (0, 1) if s.two else (0,)


def aim(s, u, v, side=0, **kw):
    """A point projected at (u, v) of image `side` that sees nothing in the other image: not in view there
    (local2), at a spot without keypoints (proj2, left), through the opener (proj2, right)."""
    if side == 0:
        return s.pt(u, v, **kw)
    if s.kind == "proj2":
        return s.pt(*s.opener(), right=(u, v), **kw)
    L = kw.pop("L", 0)
    return s.pt(0.0, 0.0, on=0, L=L, right=(u, v, L), **kw)


def lone(s, k, side, flips=0, L=0, o=None, dx=0.0, dy=1.0, **kw):
    """One keypoint and one point on spot k, `flips` bits apart."""
    u, v = spot(k)
    D = s.desc()
    i2 = s.kp(u + f32(dx), v + f32(dy), o=L if o is None else o, d=s.flip(D, flips), side=side)
    return i2, aim(s, u, v, side, d=D, L=L, **kw)


# ------------------------------------------------------------------------------------------------ the cases
# A builder(kind) returns (scene, call, expect, check): expect = [(image, point, PJ_* code)] that the trace must
# show, check(n, tables, trace) = the case's further preconditions on the restatement's answer.
def _none(*_):
    pass


def _case_contention(kind):
    """Two points on keypoint A (the second is re-scanned to B); a chain of four re-scans in which every
    fallback was the next point's phase-1 best, ending with nothing left / with a fallback over the threshold."""
    s = util.ProjScene(kind, 11)
    exp, chains = [], []
    for side in sides(s):
        k0 = RIGHT0 * side
        u, v = spot(k0)
        D = s.desc()
        a, b = s.kp(u + 1, v, d=D, side=side), s.kp(u - 1, v + 1, d=s.flip(D, 10), side=side)
        p0, p1 = aim(s, u, v, side, d=D), aim(s, u, v, side, d=D)
        exp += [(side, p0, PJ_ACCEPTED), (side, p1, PJ_ACCEPTED_AFTER_RESCAN)]
        chains.append((side, [(a, p0), (b, p1)]))
        for over, k in ((False, k0 + 2), (True, k0 + 4)):
            u, v = spot(k)
            D = s.desc()
            G = [list(range(40 * j, 40 * j + 40)) for j in range(4)]
            K = [s.kp(u - 2 + j, v + (j % 3) - 1, d=s.flip_at(D, G[j]), side=side) for j in range(4)]
            if over:
                s.kp(u + 2, v, d=s.flip_at(D, range(160, 240)), side=side)  # 110 from the last point
            # point j: 22 from K[j - 1], 58 from K[j], 82 from the others
            P = [aim(s, u, v, side, d=s.flip_at(D, G[0]))]
            P += [aim(s, u, v, side, d=s.flip_at(D, G[j - 1][:30] + G[j][:12])) for j in (1, 2, 3)]
            P.append(aim(s, u, v, side, d=s.flip_at(D, G[3][:30])))
            exp += [(side, P[0], PJ_ACCEPTED)] + [(side, p, PJ_ACCEPTED_AFTER_RESCAN) for p in P[1:4]]
            exp += [(side, P[4], PJ_LOST_AFTER_RESCAN), (side, P[4], PJ_OVER_THRESHOLD if over else PJ_ALL_BLOCKED)]
            chains.append((side, list(zip(K, P[:4]))))

    def check(n, t, tr):
        for side, links in chains:
            for i2, p in links:
                assert t[side][i2] == p
            for (before, _), (_, p) in zip(links, links[1:]):
                assert tr["p1"][side][p][1] == before != tr["fin"][side][p][1]  # re-scanned off the taken keypoint
        assert len(tr["rescans"]) >= 9 * len(sides(s))
    return s, call(kind), exp, check


def _case_overwrite(kind):
    """The first point on A has no observations: A stays open and the second point overwrites it; nmatches
    counts both.  With the rotation check the overwritten entry's bin (9) is dropped while the surviving one's
    (0) is kept: A reads -2 and one match is taken off per dropped entry -- two for B, whose both entries fall
    in dropped bins (10, 11)."""
    s = util.ProjScene(kind, 12)
    rot = kind in F2F
    exp, marks = [], []
    for side in sides(s):
        k0 = RIGHT0 * side
        (a, p0), (b, p2) = lone(s, k0, side, obs=0, angle=270.0), lone(s, k0 + 2, side, obs=0, angle=300.0)
        p1 = aim(s, *spot(k0), side, d=s.P[p0]["d"], angle=0.0)
        p3 = aim(s, *spot(k0 + 2), side, d=s.P[p2]["d"], angle=330.0)
        for j, ang in enumerate((0.0, 0.0, 90.0, 90.0, 180.0, 180.0)):
            lone(s, k0 + 4 + 2 * j, side, angle=ang)
        exp += [(side, p1, PJ_OVERWROTE), (side, p3, PJ_OVERWROTE)]
        if rot:
            exp += [(side, p, PJ_ROT_DROPPED) for p in (p0, p2, p3)]
        marks.append((side, a, b, p1, p3))

    def check(n, t, tr):
        assert n == (10 - (3 if rot else 0)) * len(sides(s))
        for side, a, b, p1, p3 in marks:
            assert (t[side][a], t[side][b]) == ((-2, -2) if rot else (p1, p3))
        if rot:
            assert tr["keep"] == (0, 3, 6) and PJ_ROT_DROPPED not in tr["codes"][0][marks[0][3]]
    return s, call(kind), exp, check


def _case_second_taken(kind):
    """Local searches: the second candidate B is taken meanwhile and the best A stays -- a ratio rejection becomes
    an acceptance (the new second C is looser), becomes an acceptance by level (C is on another level), and an
    acceptance by level becomes a rejection (C is on A's level)."""
    s = util.ProjScene(kind, 13)
    exp, watch = [], []
    # (L, (A flips, octave), (B ...), (C ...), verdict on entry, verdict at its turn)
    variants = ((0, (20, 0), (21, 0), (40, 0), PJ_RATIO_REJECTED, PJ_ACCEPTED),
                (1, (20, 1), (21, 1), (22, 0), PJ_RATIO_REJECTED, PJ_ACCEPTED_BY_LEVEL),
                (1, (20, 1), (21, 0), (22, 1), PJ_ACCEPTED_BY_LEVEL, PJ_RATIO_REJECTED))
    for side in sides(s):
        for j, (L, A, B, C, v1, vf) in enumerate(variants):
            u, v = spot(RIGHT0 * side + 2 * j)
            D = s.desc()
            db = s.flip(D, B[0])
            s.kp(u + 1, v, o=A[1], d=s.flip(D, A[0]), side=side)
            s.kp(u - 1, v, o=B[1], d=db, side=side)
            s.kp(u, v + 1, o=C[1], d=s.flip(D, C[0]), side=side)
            p0, p1 = aim(s, u, v, side, d=db, L=L), aim(s, u, v, side, d=D, L=L)
            exp += [(side, p0, PJ_ACCEPTED), (side, p1, vf)]
            watch.append((side, p1))

    def check(n, t, tr):
        assert {(a, b) for _, _, _, _, a, b in variants} <= tr["verdicts"]
        for side, p in watch:
            a, b = tr["p1"][side][p], tr["fin"][side][p]
            assert a[1] == b[1] and a[3] != b[3]  # the best stays, the second changes
    return s, call(kind), exp, check


def _case_local2_mirror(kind):
    """A right keypoint blocked only through the mirroring of a left match takes a later MapPoint's right best; a
    left ratio failure skips the right search, a left over-threshold does not."""
    s = util.ProjScene(kind, 14)
    D = s.desc()
    la = s.kp(*spot(0), d=D)
    ra, rb = s.kp(*spot(RIGHT0), d=D, side=1), s.kp(spot(RIGHT0)[0] + 1, spot(RIGHT0)[1] + 1, d=s.flip(D, 10), side=1)
    s.link(la, ra)
    m0 = s.pt(*spot(0), d=D)
    m1 = s.pt(0.0, 0.0, on=0, d=D, right=spot(RIGHT0) + (0,))
    D2 = s.desc()
    u, v = spot(2)
    s.kp(u + 1, v, d=s.flip(D2, 10))
    s.kp(u - 1, v, d=s.flip(D2, 10))
    rx = s.kp(*spot(RIGHT0 + 2), d=D2, side=1)
    m2 = s.pt(u, v, d=D2, right=spot(RIGHT0 + 2) + (0,))
    D3 = s.desc()
    s.kp(*spot(4), d=s.flip(D3, 101))
    ry = s.kp(*spot(RIGHT0 + 4), d=D3, side=1)
    m3 = s.pt(*spot(4), d=D3, right=spot(RIGHT0 + 4) + (0,))
    exp = [(0, m0, PJ_MIRRORED), (1, m1, PJ_ACCEPTED_AFTER_RESCAN), (0, m2, PJ_RATIO_REJECTED),
           (1, m2, PJ_SIDE_SKIPPED), (0, m3, PJ_OVER_THRESHOLD), (1, m3, PJ_ACCEPTED)]

    def check(n, t, tr):
        assert n == 4 and t[0][la] == m0 and (t[1][ra], t[1][rb], t[1][rx], t[1][ry]) == (m0, m1, -1, m3)
    return s, call(kind), exp, check


def _case_local2_unblocked(kind):
    """The `unblocked` path: a right keypoint blocked on entry is the stereo partner of a left keypoint that a
    MapPoint without observations takes, so later MapPoints find it -- one whose phase-1 right scan had no
    candidate at all, one whose phase-1 best was another keypoint at a larger distance.  And its mirror image,
    the left side un-blocked from the right."""
    s = util.ProjScene(kind, 15)
    exp, marks = [], []
    for c in (1, 0):  # the image that is un-blocked
        k_un, k_src = (RIGHT0, 0) if c == 1 else (2, RIGHT0 + 2)
        D = s.desc()
        u, v = spot(k_un)
        x = s.kp(u, v, d=s.flip(D, 5), blocked=1, side=c)
        y = s.kp(u + f32(3.5), v, d=s.flip(D, 30), side=c)
        src = s.kp(*spot(k_src), d=D, side=1 - c)
        s.link(*((src, x) if c == 1 else (x, src)))

        def on(side, uv, **kw):
            return s.pt(*uv, d=D, **kw) if side == 0 else s.pt(0.0, 0.0, on=0, d=D, right=tuple(uv) + (0,), **kw)
        m0 = on(1 - c, spot(k_src), obs=0)
        m1 = on(c, (u, v), obs=0)
        m2 = on(c, (u + f32(1.5), v))
        exp += [(1 - c, m0, PJ_UNBLOCKED_PARTNER), (c, m1, PJ_ACCEPTED), (c, m1, PJ_OVERWROTE),
                (c, m2, PJ_ACCEPTED_AFTER_RESCAN)]
        marks.append((c, x, y, m0, m1, m2))

    def check(n, t, tr):
        for c, x, y, m0, m1, m2 in marks:
            assert t[c][x] == m2 and t[c][y] == -1
            assert tr["p1"][c][m1][1] == -1 and tr["fin"][c][m1][1] == x  # no candidate at all on entry
            assert tr["p1"][c][m2][:2] == (30, y) and tr["fin"][c][m2][:2] == (5, x)
        assert n == 12  # every match is mirrored into its stereo partner
    return s, call(kind), exp, check


# projections whose whole window lies outside the grid: one per early return of GetFeaturesInArea
OUTSIDE = (((W + 100, 100), PJ_WINDOW_RIGHT), ((-100, 100), PJ_WINDOW_LEFT), ((100, H + 100), PJ_WINDOW_BELOW),
           ((100, -100), PJ_WINDOW_ABOVE))


def _case_proj2_sides(kind):
    """Two-camera frame-to-frame: an empty left window skips the right image, a left window whose keypoints are
    all blocked does not; right projections outside the image (no bounds test there) reach each early return of
    GetFeaturesInArea, in its order."""
    s = util.ProjScene(kind, 16)
    D = s.desc()
    r0 = s.kp(*spot(RIGHT0), d=D, side=1)
    p0 = s.pt(*spot(0), d=D, right=spot(RIGHT0))
    D = s.desc()
    s.kp(*spot(2), d=D, blocked=1)
    r1 = s.kp(*spot(RIGHT0 + 2), d=D, side=1)
    p1 = s.pt(*spot(2), d=D, right=spot(RIGHT0 + 2))
    exp = [(0, p0, PJ_EMPTY_WINDOW), (1, p0, PJ_SIDE_SKIPPED), (0, p1, PJ_ALL_BLOCKED), (1, p1, PJ_ACCEPTED)]
    for uv, code in OUTSIDE + (((W + 100, -100), PJ_WINDOW_RIGHT), ((-100, H + 100), PJ_WINDOW_LEFT)):
        exp.append((1, s.pt(*s.opener(), right=uv), code))

    def check(n, t, tr):
        assert n == 1 and t[1][r0] == -1 and t[1][r1] == p1 and tr["window_returns"] == {1, 2, 3, 4}
    return s, call(kind), exp, check


def _case_kb8(kind):
    """KannalaBrandt8 projections of both cameras (the other cases are Pinhole): keypoints placed on the
    restated projections, two points on one target per image."""
    cam = util.KB8_TUMVI
    s = util.ProjScene(kind, 17, W=512, H=512, kb8=cam[4:], camera=tuple(cam[:4]) + (f32(0),))
    exp, marks = [], []
    pts = [(0.3, 0.2, 1.0), (-0.6, 0.4, 2.0), (0.9, -0.8, 1.5), (-0.2, -1.1, 3.0), (1.6, 0.1, 1.0), (0.05, 0.02, 4.0)]
    for j, x3 in enumerate(pts):
        x3 = tuple(f32(t) for t in x3)
        x3r = (f32(x3[0] - f32(0.11)), x3[1], f32(x3[2] + f32(0.01)))
        (ul, vl), (ur, vr) = util.pj_project(s.camera, s.kb8, *x3), util.pj_project(s.camera, s.kb8, *x3r)
        D = s.desc()
        a = s.kp(ul + f32(0.5), vl - f32(0.5), d=D)
        b = s.kp(ur - f32(0.5), vr + f32(0.5), d=D, side=1)
        p = s.pt(0, 0, d=D, x3=x3, x3r=x3r)
        exp += [(0, p, PJ_ACCEPTED), (1, p, PJ_ACCEPTED)]
        marks.append((a, b, p))
        if j < 2:
            a2 = s.kp(ul - f32(1.5), vl + f32(1.0), d=s.flip(D, 12))
            b2 = s.kp(ur + f32(1.5), vr - f32(1.0), d=s.flip(D, 12), side=1)
            p2 = s.pt(0, 0, d=D, x3=x3, x3r=x3r)
            exp += [(0, p2, PJ_ACCEPTED_AFTER_RESCAN), (1, p2, PJ_ACCEPTED_AFTER_RESCAN)]
            marks.append((a2, b2, p2))

    def check(n, t, tr):
        assert n == 2 * len(marks)
        for a, b, p in marks:
            assert t[0][a] == p and t[1][b] == p
        c = s.case()
        d = dict(c, kb8=None)
        assert not np.array_equal(util.py_proj_traced(d, 3.0)[1][0], t[0])  # the fisheye model is really used
    return s, call(kind), exp, check


def _on_edge(u, r):
    """(x_on, x_in): x_on - u == r exactly in float, x_in one float nearer."""
    u, r = f32(u), f32(r)
    x_on = f32(u + r)
    x_in = np.nextafter(x_on, u)
    assert f32(x_on - u) == r and f32(x_in - u) < r, (u, r)
    return x_on, x_in


def _case_edges(kind):
    """|dx| == radius and |dy| == radius exactly (excluded: the test is strict) and one float inside (included),
    on both signs, with a radius that is exact in float (level 0) and one that is not (level 3): the point sits 2
    px from the image corner, where x + r has r's exponent and the subtraction is exact."""
    s = util.ProjScene(kind, 18)
    exp = []
    for side in sides(s):
        for L, base in ((0, 100.0), (3, 2.0)):
            r = radius(kind, L)
            assert (float(r) == float(int(r * 2)) / 2) == (L == 0)
            on, inn = _on_edge(base, r)
            # +dx and +dy at both levels; -dx / -dy at level 0 (level 3 sits in the corner)
            probes = [((base, 200.0 + 40 * L), (1, 0)), ((200.0 + 40 * L, base), (0, 1))]
            if L == 0:
                probes += [((base, 300.0), (-1, 0)), ((300.0, base), (0, -1))]
            for (u, v), (sx, sy) in probes:
                for k, (x, code) in enumerate(((on, PJ_EMPTY_WINDOW), (inn, PJ_ACCEPTED))):
                    uu, vv = f32(u + 16 * k * abs(sy)), f32(v + 16 * k * abs(sx))  # the two probes 16 px apart
                    d = f32(x - f32(base))
                    D = s.desc()
                    s.kp(uu + sx * d, vv + sy * d, o=L, d=D, side=side)
                    exp.append((side, aim(s, uu, vv, side, d=D, L=L), code))
    return s, call(kind), exp, _none


def _case_borders(kind):
    """Windows clipped at each of the four image borders; a keypoint PosInGrid leaves out of the grid (x or y
    rounds to column 64 / row 48) lies inside the window and is never a candidate."""
    s = util.ProjScene(kind, 19)
    exp = []
    for side in sides(s):
        for (u, v), (kx, ky), code in (((1.0, 100.0), (0.5, 100.5), PJ_ACCEPTED),
                                       ((100.0, 1.0), (100.5, 0.5), PJ_ACCEPTED),
                                       ((746.5, 100.0), (745.0, 100.0), PJ_ACCEPTED),
                                       ((100.0, 475.5), (100.0, 474.0), PJ_ACCEPTED),
                                       ((751.0, 200.0), (751.8, 200.0), PJ_EMPTY_WINDOW),
                                       ((200.0, 479.0), (200.0, 479.9), PJ_EMPTY_WINDOW)):
            D = s.desc()
            s.kp(kx, ky, d=D, side=side)
            exp.append((side, aim(s, u, v, side, d=D), code))

    def check(n, t, tr):
        g = s.grid
        for side in sides(s):
            for j, clipped in enumerate(("x0", "y0", "x1", "y1")):
                p = [e[1] for e in exp if e[0] == side][j]
                pr = s.P[p]
                u, v = (pr["u"], pr["v"]) if side == 0 or kind == "local" else pr["right"][:2]
                r = radius(kind, 0)
                lo = (f32(f32(u) - r) * g[4], f32(f32(v) - r) * g[5])
                hi = (f32(f32(u) + r) * g[4], f32(f32(v) + r) * g[5])
                assert {"x0": lo[0] < 0, "y0": lo[1] < 0, "x1": hi[0] > 63, "y1": hi[1] > 47}[clipped]
    return s, call(kind), exp, check


def _case_outside(kind):
    """Local searches take the projections as given: windows wholly outside the grid on each side, and outside on
    two sides at once (the reference's order: x before y, low before high)."""
    s = util.ProjScene(kind, 20)
    exp = []
    for side in sides(s):
        lone(s, RIGHT0 * side, side)
        for uv, code in OUTSIDE + (((W + 100, H + 100), PJ_WINDOW_RIGHT), ((-100, -100), PJ_WINDOW_LEFT)):
            exp.append((side, aim(s, *uv, side), code))

    def check(n, t, tr):
        assert tr["window_returns"] == {1, 2, 3, 4} and n == len(sides(s))
    return s, call(kind), exp, check


def _case_levels(kind, mode="default"):
    """The level filter of each search at its ends: a keypoint one octave outside the admitted range holds the
    point's own descriptor and is ignored, the one on the range's end (10 bits off) is matched; a point whose
    octave / level is -1 or nlevels has no candidate."""
    s = util.ProjScene(kind, 21)
    fwd, bwd = mode == "forward", mode == "backward"
    if kind in F2F:
        levels = {"default": (0, 7), "forward": (0, 3), "backward": (3,)}[mode]
        rng_of = (lambda L: (L, 7)) if fwd else (lambda L: (0, L)) if bwd else \
            (lambda L: (max(L - 1, 0), min(L + 1, 7)))
    elif kind == "reloc":
        levels, rng_of = (0, 3, 7), lambda L: (max(L - 1, 0), min(L + 1, 7))
    else:
        levels, rng_of = (0, 7), lambda L: (max(L - 1, 0), L)
    exp, marks = [], []
    for side in sides(s):
        k = RIGHT0 * side
        for L in levels:
            lo, hi = rng_of(L)
            for end, out in ((lo, lo - 1), (hi, hi + 1)):
                u, v = spot(k)
                k += 2
                D = s.desc()
                if 0 <= out <= 7:
                    s.kp(u + 1, v, o=out, d=D, side=side)
                i2 = s.kp(u - 1, v, o=end, d=s.flip(D, 10), side=side)
                p = aim(s, u, v, side, d=D, L=L)
                exp.append((side, p, PJ_ACCEPTED))
                marks.append((side, i2, p))
        for L in (-1, 8):
            i2, p = lone(s, k, side, L=L, o=0)
            k += 2
            if kind == "proj2" and side == 1:
                continue  # the octave is tested before the left window
            exp.append((side, p, PJ_BAD_LEVEL))
    exp.append((0, lone(s, 390, 0, on=0)[1], PJ_NOT_SEARCHED))

    def check(n, t, tr):
        for side, i2, p in marks:
            assert t[side][i2] == p
        assert n == len(marks)
    return s, call(kind, forward=int(fwd), backward=int(bwd)), exp, check


def _case_uright(kind):
    """The mvuRight test (one camera): a keypoint with mvuRight 0 or negative is not tested (the check is > 0),
    er == radius is kept (strict >), one float above is rejected; at level 0 (exact radius) and level 3.  The
    point's right coordinate is 2 (frame-to-frame: ur = u - mbf / z with u = 10, z = 1 and with u = 6, z = 2;
    local: mTrackProjXR = 2), so that 2 + radius is exact."""
    s = util.ProjScene(kind, 22, uright=True)
    exp = []
    j = 0
    for L in (0, 3):
        r = radius(kind, L)
        on, _ = _on_edge(2.0, r)
        for ur, code in ((0.0, PJ_ACCEPTED), (-5.0, PJ_ACCEPTED), (on, PJ_ACCEPTED),
                         (np.nextafter(on, f32(1e9)), PJ_ALL_BLOCKED), (500.0, PJ_ALL_BLOCKED), (2.5, PJ_ACCEPTED)):
            for u, z in ((10.0, 1.0), (6.0, 2.0)):
                v = f32(40 + 16 * j)
                j += 1
                D = s.desc()
                s.kp(u + 1, v, o=L, d=D, ur=ur)
                exp.append((0, s.pt(u, v, L=L, d=D, xr=2.0, z=z), code))
    return s, call(kind), exp, _none


def _case_gates(kind):
    """The projection gates: zc < 0 (frame-to-frame); u and v exactly on min / max of the image bounds are kept,
    one float beyond is skipped.  Relocalization: dist3D exactly on minDistance / maxDistance is kept, just
    outside is skipped, and a point with negative zc whose projection lands on a keypoint is searched and
    matched (that search has no depth test)."""
    s = util.ProjScene(kind, 23)
    exp = []
    L = 7  # radius 10.7: the last grid column / row ends 5.9 / 5 px inside the image
    up, dn = f32(np.inf), f32(-np.inf)
    for (u, v), (kx, ky) in (((0.0, 100.0), (1.0, 100.0)), ((W, 100.0), (745.0, 100.0)), ((200.0, 0.0), (200.0, 1.0)),
                             ((200.0, H), (200.0, 474.0))):
        D = s.desc()
        s.kp(kx, ky, o=L, d=D)
        exp.append((0, s.pt(u, v, L=L, d=D), PJ_ACCEPTED))
        ub = np.nextafter(f32(u), dn if u == 0 else up) if u in (0.0, W) else f32(u)
        vb = np.nextafter(f32(v), dn if v == 0 else up) if v in (0.0, H) else f32(v)
        exp.append((0, s.pt(ub, vb, L=L, d=D), PJ_OUT_OF_BOUNDS))
    i2, p = lone(s, 60, 0, z=-2.0)
    if kind == "reloc":
        exp.append((0, p, PJ_ACCEPTED))
        for j, (dist, code) in enumerate((((2.5, 2.5, 10.0), PJ_ACCEPTED), ((10.0, 2.5, 10.0), PJ_ACCEPTED),
                                          ((np.nextafter(f32(2.5), dn), 2.5, 10.0), PJ_DEPTH_RANGE),
                                          ((np.nextafter(f32(10.0), up), 2.5, 10.0), PJ_DEPTH_RANGE))):
            exp.append((0, lone(s, 62 + 2 * j, 0, dist=dist)[1], code))
    else:
        exp.append((0, p, PJ_BEHIND))
    exp.append((0, lone(s, 80, 0, on=0)[1], PJ_NOT_SEARCHED))
    return s, call(kind), exp, _none


def _case_thresholds(kind, orb_dist=100):
    """bestDist exactly TH_HIGH (ORBdist) is accepted, one more is rejected."""
    s = util.ProjScene(kind, 24)
    exp = []
    for side in sides(s):
        k = RIGHT0 * side
        exp += [(side, lone(s, k, side, flips=orb_dist)[1], PJ_ACCEPTED),
                (side, lone(s, k + 2, side, flips=orb_dist + 1)[1], PJ_OVER_THRESHOLD)]
    return s, call(kind, orb_dist=orb_dist), exp, _none


RATIO_PAIRS = {
    # (best, second, second on another level): verdict.  f32(0.9) * 10 == 9.0f exactly, so (9, 10) passes the
    # float product that the reference computes; in double the product is 8.99999976 and it would fail.
    0.9: (((9, 10, 0), PJ_ACCEPTED), ((18, 20, 0), PJ_ACCEPTED), ((90, 100, 0), PJ_ACCEPTED),
          ((10, 10, 0), PJ_RATIO_REJECTED), ((10, 11, 0), PJ_RATIO_REJECTED), ((8, 10, 0), PJ_ACCEPTED),
          ((9, 10, 1), PJ_ACCEPTED), ((10, 10, 1), PJ_ACCEPTED_BY_LEVEL), ((91, 100, 1), PJ_ACCEPTED_BY_LEVEL),
          ((40, None, 0), PJ_ACCEPTED)),
    0.8: (((8, 10, 0), PJ_ACCEPTED), ((9, 10, 0), PJ_RATIO_REJECTED), ((7, 10, 0), PJ_ACCEPTED),
          ((80, 100, 0), PJ_ACCEPTED), ((81, 100, 0), PJ_RATIO_REJECTED), ((81, 100, 1), PJ_ACCEPTED_BY_LEVEL)),
    0.75: (((75, 100, 0), PJ_ACCEPTED), ((76, 100, 0), PJ_RATIO_REJECTED), ((3, 4, 0), PJ_ACCEPTED),
           ((4, 5, 0), PJ_RATIO_REJECTED), ((31, 40, 1), PJ_ACCEPTED_BY_LEVEL)),
}


def _case_ratio(kind, nnratio):
    """The local searches' ratio test bestDist > mfNNratio * bestDist2, a float product, on pairs on both sides
    of it, with the second on the best's level and on another one, and with a single candidate."""
    s = util.ProjScene(kind, 25)
    exp = []
    for side in sides(s):
        for j, ((b1, b2, other), code) in enumerate(RATIO_PAIRS[nnratio]):
            u, v = spot(RIGHT0 * side + 2 * j)
            D = s.desc()
            s.kp(u + 1, v, o=1, d=s.flip(D, b1), side=side)
            if b2 is not None:
                s.kp(u - 1, v, o=1 - other, d=s.flip(D, b2), side=side)
            exp.append((side, aim(s, u, v, side, d=D, L=1), code))
    return s, call(kind, nnratio=nnratio), exp, _none


def _case_ties(kind):
    """Two candidates tie for best and the lower keypoint index lies in the later grid column: the winner is the
    first in GetFeaturesInArea's order.  Local searches: two candidates tie for second on different levels (which
    one comes first decides between rejection and acceptance by level), and a candidate equal to the best
    arrives later and becomes the second."""
    s = util.ProjScene(kind, 26)
    exp, marks = [], []
    edge = f32(11.75 * 8.5)  # between grid columns 8 and 9 (PosInGrid rounds)
    for side in sides(s):
        D = s.desc()
        late = s.kp(edge + 1, 100.0, o=1, d=s.flip(D, 10), side=side)
        early = s.kp(edge - 1, 100.0, o=0, d=s.flip(D, 10), side=side)
        p = aim(s, edge, 100.0, side, d=D, L=1)
        assert late < early
        marks.append((side, early, p, late))
        exp.append((side, p, PJ_ACCEPTED_BY_LEVEL if kind in LOCAL else PJ_ACCEPTED))
        if kind in LOCAL:
            for j, (first, code) in enumerate(((1, PJ_RATIO_REJECTED), (0, PJ_ACCEPTED_BY_LEVEL))):
                u, v = spot(RIGHT0 * side + 40 + 2 * j)
                D = s.desc()
                s.kp(u, v + 1, o=1, d=s.flip(D, 10), side=side)
                s.kp(u + f32(0.5), v - 1, o=first, d=s.flip(D, 11), side=side)
                s.kp(u - f32(0.5), v - 1, o=1 - first, d=s.flip(D, 11), side=side)
                exp.append((side, aim(s, u, v, side, d=D, L=1), code))
            u, v = spot(RIGHT0 * side + 46)
            D = s.desc()
            s.kp(u, v + 1, d=s.flip(D, 10), side=side)
            s.kp(u, v - 1, d=s.flip(D, 10), side=side)
            exp.append((side, aim(s, u, v, side, d=D), PJ_RATIO_REJECTED))

    def check(n, t, tr):
        for side, early, p, late in marks:
            assert t[side][early] == p and t[side][late] == -1
            k = s.case()["kps" if s.two and side == 0 else "kps_r" if s.two else "cur_kps"]
            g = s.grid
            assert round(float(k["x"][late] * g[4])) == round(float(k["x"][early] * g[4])) + 1
    return s, call(kind), exp, check


HISTS = {
    # name: ({bin: matches}, kept bins, ComputeThreeMaxima branch, rotation check)
    "tie_four": ({2: 2, 5: 2, 8: 2, 11: 2}, (2, 5, 8), "keep_three", 1),   # strict >: the earlier bins stay ahead
    "tie_two": ({2: 3, 5: 3, 8: 1}, (2, 5, 8), "keep_three", 1),
    "ten_pct_10_1": ({0: 10, 4: 1}, (0, 4, -1), "cut_third", 1),           # 0.1f * 10 == 1.0f: max2 is kept
    "ten_pct_20_2": ({0: 20, 4: 2}, (0, 4, -1), "cut_third", 1),
    "ten_pct_11_1": ({0: 11, 4: 1}, (0, -1, -1), "cut_two", 1),
    "third_10_5_1": ({0: 10, 4: 5, 8: 1}, (0, 4, 8), "keep_three", 1),
    "third_11_5_1": ({0: 11, 4: 5, 8: 1}, (0, 4, -1), "cut_third", 1),
    "one_bin": ({7: 3}, (7, -1, -1), "cut_two", 1),
    "ori_off": ({0: 11, 4: 1}, None, None, 0),
}


def _case_hist(kind, name):
    """ComputeThreeMaxima on a histogram built match by match (angle difference 30 * bin degrees)."""
    s = util.ProjScene(kind, 27)
    counts, keep, branch, ori = HISTS[name]
    exp = []
    k = 0
    for b, n in counts.items():
        for _ in range(n):
            side = (k // 2) % 2 if s.two else 0  # both images feed the one histogram
            exp.append((side, lone(s, RIGHT0 * side + k, side, angle=30.0 * b)[1],
                        PJ_ACCEPTED if (not ori or b in keep) else PJ_ROT_DROPPED))
            k += 2

    def check(n, t, tr):
        assert tr["keep"] == keep and (branch is None or branch in tr["three_maxima"])
        assert n == sum(c for b, c in counts.items() if not ori or b in keep)
        if ori:
            assert [tr["hist"][b] for b in counts] == list(counts.values())
    return s, call(kind, ori=ori), exp, check


def _case_no_match(kind):
    """The rotation check on and not one match: every bin is empty."""
    s = util.ProjScene(kind, 28)
    exp = [(0, lone(s, 2 * j, 0, flips=120)[1], PJ_OVER_THRESHOLD) for j in range(3)]

    def check(n, t, tr):
        assert n == 0 and tr["keep"] == (-1, -1, -1) and all((x == -1).all() for x in t)
    return s, call(kind), exp, check


def _case_rot_half(kind):
    """f32(15) * (1.0f / 30) == 0.5f exactly: round() gives bin 1 (rint would give 0).  Three matches at 15
    degrees, three at 0, two at 150 and two at 270: bins {0: 3, 1: 3, 5: 2, 9: 2}, so bin 9 is dropped -- with
    the 15-degree matches in bin 0 nothing would be."""
    s = util.ProjScene(kind, 29)
    exp = []
    for j, ang in enumerate((15.0, 15.0, 15.0, 0.0, 0.0, 0.0, 150.0, 150.0, 270.0, 270.0)):
        exp.append((0, lone(s, 2 * j, 0, angle=ang)[1], PJ_ROT_DROPPED if ang == 270.0 else PJ_ACCEPTED))

    def check(n, t, tr):
        assert f32(15) * (f32(1) / f32(30)) == f32(0.5) and tr["keep"] == (0, 1, 5) and n == 8
    return s, call(kind), exp, check


def _case_angles(kind):
    """Angle differences of exactly 15 + 30 k degrees, exactly 0, negative ones (+ 360) and a small negative one
    whose sum with 360 is 360.0f in float (bin 12): only bins 0..12 are ever populated."""
    s = util.ProjScene(kind, 30)
    pairs = [(15.0 + 30 * k, 0.0) for k in range(12)] + [(0.0, 0.0), (77.0, 77.0), (10.0, 40.0), (0.0, 359.0),
                                                        (0.0, 1e-6), (100.0, 100.00001)]
    for j, (a, b) in enumerate(pairs):
        u, v = spot(2 * j)
        D = s.desc()
        s.kp(u, v + 1, d=D, angle=b)
        s.pt(u, v, d=D, angle=a)

    def check(n, t, tr):
        bins = [util.py_rot_bin(a, b) for a, b in pairs]
        assert bins[:12] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12] and bins[12:16] == [0, 0, 11, 0], bins
        assert f32(f32(0.0) - f32(1e-6)) + f32(360) == f32(360) and bins[16] == 12
        assert {b for b, c in enumerate(tr["hist"]) if c} <= set(range(13)) and tr["hist"][12] >= 2
    return s, call(kind), [], check


def _case_shape(kind, n_pt, n_kp):
    """Launch shape: the phase-1 loops stride by 256 threads.  Every point is accepted (one bin), so the
    histogram entry list is filled to its capacity when the tables are as long as the counts."""
    s = util.ProjScene(kind, 31 + n_pt)
    exp = []
    for j in range(max(n_pt, n_kp)):
        u, v = spot(j)
        D = s.desc()
        if j < n_kp:
            for side in sides(s):
                s.kp(u, v + 1, d=D, side=side)
        if j < n_pt:
            p = s.pt(u, v, d=D, right=(u, v, 0) if s.two else None)
            exp += [(side, p, PJ_ACCEPTED if j < n_kp else PJ_EMPTY_WINDOW) for side in sides(s)
                    if j < n_kp or side == 0 or kind == "local2"]

    def check(n, t, tr):
        assert n == min(n_pt, n_kp) * len(sides(s)) and all(len(x) == n_kp for x in t)
        assert len(s.P) == n_pt
    return s, call(kind), exp, check


# name: (builder, kinds, the codes it exists to produce)
CASES = {
    "contention": (_case_contention, KINDS, {PJ_ACCEPTED_AFTER_RESCAN, PJ_LOST_AFTER_RESCAN, PJ_ALL_BLOCKED,
                                             PJ_OVER_THRESHOLD}),
    "overwrite": (_case_overwrite, F2F + LOCAL, {PJ_OVERWROTE}),
    "second_taken": (_case_second_taken, LOCAL, {PJ_RATIO_REJECTED, PJ_ACCEPTED_BY_LEVEL, PJ_ACCEPTED_AFTER_RESCAN,
                                                 PJ_LOST_AFTER_RESCAN}),
    "local2_mirror": (_case_local2_mirror, ("local2",), {PJ_MIRRORED, PJ_SIDE_SKIPPED, PJ_ACCEPTED_AFTER_RESCAN}),
    "local2_unblocked": (_case_local2_unblocked, ("local2",), {PJ_UNBLOCKED_PARTNER, PJ_OVERWROTE}),
    "proj2_sides": (_case_proj2_sides, ("proj2",), {PJ_SIDE_SKIPPED, PJ_ALL_BLOCKED, PJ_WINDOW_RIGHT, PJ_WINDOW_LEFT,
                                                    PJ_WINDOW_BELOW, PJ_WINDOW_ABOVE}),
    "kb8": (_case_kb8, ("proj2",), {PJ_ACCEPTED, PJ_ACCEPTED_AFTER_RESCAN}),
    "edges": (_case_edges, KINDS, {PJ_EMPTY_WINDOW, PJ_ACCEPTED}),
    "borders": (_case_borders, KINDS, {PJ_EMPTY_WINDOW, PJ_ACCEPTED}),
    "outside": (_case_outside, LOCAL, {PJ_WINDOW_RIGHT, PJ_WINDOW_LEFT, PJ_WINDOW_BELOW, PJ_WINDOW_ABOVE}),
    "levels": (_case_levels, KINDS, {PJ_BAD_LEVEL, PJ_NOT_SEARCHED, PJ_ACCEPTED}),
    "levels_forward": (functools.partial(_case_levels, mode="forward"), F2F, {PJ_BAD_LEVEL, PJ_ACCEPTED}),
    "levels_backward": (functools.partial(_case_levels, mode="backward"), F2F, {PJ_BAD_LEVEL, PJ_ACCEPTED}),
    "uright": (_case_uright, ("proj", "local"), {PJ_ALL_BLOCKED, PJ_ACCEPTED}),
    "gates": (_case_gates, HIST, {PJ_OUT_OF_BOUNDS, PJ_NOT_SEARCHED}),
    "thresholds": (_case_thresholds, KINDS, {PJ_OVER_THRESHOLD, PJ_ACCEPTED}),
    "thresholds_50": (functools.partial(_case_thresholds, orb_dist=50), ("reloc",), {PJ_OVER_THRESHOLD, PJ_ACCEPTED}),
    "ratio_0.9": (functools.partial(_case_ratio, nnratio=0.9), LOCAL, {PJ_RATIO_REJECTED, PJ_ACCEPTED_BY_LEVEL}),
    "ratio_0.8": (functools.partial(_case_ratio, nnratio=0.8), LOCAL, {PJ_RATIO_REJECTED, PJ_ACCEPTED_BY_LEVEL}),
    "ratio_0.75": (functools.partial(_case_ratio, nnratio=0.75), LOCAL, {PJ_RATIO_REJECTED, PJ_ACCEPTED_BY_LEVEL}),
    "ties": (_case_ties, KINDS, {"local": {PJ_ACCEPTED_BY_LEVEL, PJ_RATIO_REJECTED},
                                 "local2": {PJ_ACCEPTED_BY_LEVEL, PJ_RATIO_REJECTED}}),
    "no_match": (_case_no_match, HIST, {PJ_OVER_THRESHOLD}),
    "rot_half": (_case_rot_half, HIST, {PJ_ROT_DROPPED}),
    "angles": (_case_angles, HIST, {PJ_ACCEPTED}),
}
for _name in HISTS:
    CASES["hist_" + _name] = (functools.partial(_case_hist, name=_name), HIST,
                              {PJ_ROT_DROPPED} if _name in ("tie_four", "ten_pct_11_1") else {PJ_ACCEPTED})
for _n_pt, _n_kp in ((0, 1), (1, 1), (256, 257), (257, 257)):
    CASES[f"shape_{_n_pt}_{_n_kp}"] = (functools.partial(_case_shape, n_pt=_n_pt, n_kp=_n_kp), KINDS,
                                       {PJ_ACCEPTED} if _n_pt else set())
PARAMS = [(name, kind) for name, (_, kinds, _) in CASES.items() for kind in kinds]
IDS = [f"{name}-{kind}" for name, kind in PARAMS]


@functools.lru_cache(maxsize=None)
def case(name, kind):
    """The case's tables, its traced restatement and the oracle's answer, computed once for the CPU and the GPU
    tests."""
    build, _, produces = CASES[name]
    if isinstance(produces, dict):
        produces = produces.get(kind, {PJ_ACCEPTED})
    s, prm, exp, check = build(kind)
    c = s.case()
    return {"c": c, "call": prm, "exp": exp, "check": check, "produces": produces, "py": util.pj_restate(c, prm),
            "ref": util.pj_oracle(c, prm)}


def _seen(tr):
    return {code for side in tr["codes"] for cs in side for code in cs}


def _same(a, b):
    return a[0] == b[0] and len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


# ------------------------------------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("name,kind", PARAMS, ids=IDS)
def test_case_takes_its_branches_and_oracle_matches_restatement(name, kind):
    c = case(name, kind)
    n, tables, tr = c["py"]
    missing = [PJ_NAMES[k] for k in c["produces"] - _seen(tr)]
    assert not missing, f"{name}/{kind}: no point came out {missing}"
    for side, p, code in c["exp"]:
        got = tr["codes"][side][p]
        assert code in got, \
            f"{name}/{kind}: image {side} point {p} is {[PJ_NAMES[k] for k in got]}, not {PJ_NAMES[code]}"
    c["check"](n, tables, tr)
    for t, key in zip(tables, ("kps", "kps_r") if "kps" in c["c"] else ("cur_kps",)):
        assert len(t) == len(c["c"][key]) <= 300 or name.startswith("shape")
    rn, rt = c["ref"]
    assert rn == n, f"{name}/{kind}: oracle nmatches {rn}, restatement {n}"
    for side, (a, b) in enumerate(zip(rt, tables)):
        np.testing.assert_array_equal(a, b, err_msg=f"{name}/{kind}: image {side}")


# The codes every kernel must show over its cases (grid_window's early returns cannot happen where the
# projection is tested against the image bounds first: the one-camera frame-to-frame and relocalization searches).
_COMMON = {PJ_NOT_SEARCHED, PJ_BAD_LEVEL, PJ_EMPTY_WINDOW, PJ_ALL_BLOCKED, PJ_OVER_THRESHOLD, PJ_ACCEPTED,
           PJ_ACCEPTED_AFTER_RESCAN, PJ_LOST_AFTER_RESCAN}
_WINDOWS = {PJ_WINDOW_RIGHT, PJ_WINDOW_LEFT, PJ_WINDOW_BELOW, PJ_WINDOW_ABOVE}
_LOCAL = _COMMON | _WINDOWS | {PJ_RATIO_REJECTED, PJ_ACCEPTED_BY_LEVEL, PJ_OVERWROTE}
CENSUS = {
    "proj": _COMMON | {PJ_BEHIND, PJ_OUT_OF_BOUNDS, PJ_OVERWROTE, PJ_ROT_DROPPED},
    "proj2": _COMMON | _WINDOWS | {PJ_BEHIND, PJ_OUT_OF_BOUNDS, PJ_OVERWROTE, PJ_ROT_DROPPED, PJ_SIDE_SKIPPED},
    "reloc": _COMMON | {PJ_OUT_OF_BOUNDS, PJ_DEPTH_RANGE, PJ_ROT_DROPPED},
    "local": _LOCAL,
    "local2": _LOCAL | {PJ_MIRRORED, PJ_UNBLOCKED_PARTNER, PJ_SIDE_SKIPPED},
}


def census(kind):
    codes, returns, branches, bins = set(), set(), set(), set()
    for name, k in PARAMS:
        if k == kind:
            tr = case(name, kind)["py"][2]
            codes |= _seen(tr)
            returns |= tr["window_returns"]
            branches |= tr["three_maxima"]
            bins |= {b for b, c in enumerate(tr["hist"]) if c}
    return codes, returns, branches, bins


@pytest.mark.parametrize("kind", KINDS)
def test_cases_cover_every_outcome_of_the_kernel(kind):
    codes, returns, branches, bins = census(kind)
    assert codes == CENSUS[kind], ([PJ_NAMES[k] for k in CENSUS[kind] - codes],
                                   [PJ_NAMES[k] for k in codes - CENSUS[kind]])
    assert returns == ({1, 2, 3, 4} if kind in ("proj2",) + LOCAL else set())
    if kind in HIST:
        assert branches == set(util.TM_BRANCHES) and bins == set(range(13))


def test_census_names_every_code():
    assert set().union(*CENSUS.values()) == set(range(len(PJ_NAMES)))


# The mistakes a kernel of this schedule could make, and the kinds whose restatement has the switch.
MUTANTS = {"no_rescan": KINDS, "rescan_best_only": LOCAL, "no_unblocked": ("local2",), "low_index_tie": KINDS,
           "le_radius": KINDS, "ge_uright": ("proj", "local"), "ratio_double": LOCAL, "rint_bin": HIST,
           "ge_three_maxima": HIST, "le_ten_percent": HIST, "dec_per_keypoint": F2F, "lt_th_high": KINDS}


def caught_by(mutant, kind):
    """The cases of `kind` whose expected answer changes under the mutant."""
    out = []
    for name, k in PARAMS:
        if k == kind and not name.startswith("shape"):
            c = case(name, kind)
            n, t, _ = util.pj_restate(c["c"], c["call"], mut=(mutant,))
            if not _same((n, t), c["py"][:2]):
                out.append(name)
    return out


@pytest.mark.parametrize("mutant", util.PJ_MUTANTS)
def test_every_mutant_is_told_apart_by_a_case(mutant):
    assert set(MUTANTS) == set(util.PJ_MUTANTS)
    for kind in MUTANTS[mutant]:
        assert caught_by(mutant, kind), f"no {kind} case changes its answer under {mutant}"


def test_walker_matches_the_older_restatement():
    """pj_in_area against _py_in_area of tests/test_local_stereo.py on the crafted keypoints."""
    from test_local_stereo import _py_in_area
    from test_projection import _py_grid
    c = case("edges", "local")["c"]
    k = c["cur_kps"]
    cells = _py_grid(k["x"], k["y"], c["grid"])
    for x, y, _, _ in c["mp_proj"]:
        for r in (f32(2.5), radius("local", 3), f32(40.0)):
            for lo, hi in ((-1, 0), (2, 3), (0, -1)):
                got = util.pj_in_area(cells, k, c["grid"], x, y, r, lo, hi)[0]
                assert got == _py_in_area(cells, k, c["grid"], x, y, r, lo, hi)


# ------------------------------------------------------------------------------------------- GPU tests
def gpu_host(c, prm):
    """The case through the host form the existing tests use -> (nmatches, [tables])."""
    import plvi
    kind = c["kind"]
    mt = plvi.ORBmatcher(prm["nnratio"], bool(prm["ori"]))
    if kind == "proj":
        r = mt.SearchByProjection(util.proj_params(c, prm["th"], prm["forward"], prm["backward"]), c["cur_kps"],
                                  c["cur_desc"], c["x3dc"], c["last_octave"], c["last_angle"], c["mp_desc"], c["flags"],
                                  c["cur_blocked"], c["cur_uright"])
    elif kind == "proj2":
        r = mt.SearchByProjectionStereo(util.proj_params(c, prm["th"], prm["forward"], prm["backward"]), c["kps"],
                                        c["desc"], c["kps_r"], c["desc_r"], c["x3dc"], c["x3dr"], c["last_octave"],
                                        c["last_angle"], c["mp_desc"], c["flags"], c["kb8"], c["blocked"],
                                        c["blocked_r"])
    elif kind == "reloc":
        r = mt.SearchByProjectionKF(util.reloc_params(c, prm["th"], prm["orb_dist"]), c["cur_kps"], c["cur_desc"],
                                    c["kf_flags"], c["x3dc"], c["dist"], c["level"], c["kf_angle"], c["mp_desc"],
                                    c["cur_blocked"])
    elif kind == "local":
        r = mt.SearchByProjectionLocal(util.local_params(c, prm["th"]), c["cur_kps"], c["cur_desc"], c["mp_flags"],
                                       c["mp_proj"], c["mp_level"], c["mp_desc"], c["cur_blocked"], c["cur_uright"])
    else:
        r = mt.SearchByProjectionLocalStereo(util.local_params(c, prm["th"]), c["kps"], c["desc"], c["kps_r"],
                                             c["desc_r"], c["mp_flags"], c["mp_proj"], c["mp_level"], c["mp_proj_r"],
                                             c["mp_level_r"], c["mp_desc"], c["blocked"], c["blocked_r"], c["l2r"],
                                             c["r2l"])
    return r[0], list(r[1:])


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", PARAMS, ids=IDS)
def test_case_gpu_matches_oracle(name, kind):
    c = case(name, kind)
    n, tables = gpu_host(c["c"], c["call"])
    rn, rt = c["ref"]
    for side, (a, b) in enumerate(zip(tables, rt)):
        np.testing.assert_array_equal(a, b, err_msg=f"{name}/{kind}: image {side}")
    assert n == rn and len(tables) == len(rt)


def batch_groups(kind):
    """The kernel's cases grouped by what one batched launch shares: the parameter struct, the grid, the camera
    and whether mvuRight is given."""
    groups = {}
    for name, k in PARAMS:
        if k == kind:
            c = case(name, kind)
            cc = c["c"]
            key = (tuple(sorted(c["call"].items())), tuple(float(t) for t in cc["grid"]),
                   tuple(float(t) for t in cc.get("camera", ())), cc.get("cur_uright") is not None,
                   cc.get("kb8") is not None)
            groups.setdefault(key, []).append(c)
    return [g + [_filler(kind, g[0]["c"], g[0]["call"])] for g in groups.values()]


@pytest.mark.parametrize("kind", KINDS)
def test_batches_pack_every_case_above_its_counts(kind):
    """The batched GPU test's tables: every case of the kernel is in one group, every capacity is above every
    count, and the rows past a case's count differ from zero padding (poison)."""
    groups = batch_groups(kind)
    assert sum(len(g) - 1 for g in groups) == sum(1 for _, k in PARAMS if k == kind)
    assert max(len(g) for g in groups) >= 8
    for cs in groups:
        b, kk, pk, caps, pcap, _ = _pack(kind, cs)
        for c, row in zip(cs, b[pk]):
            assert len(c["c"][pk]) < pcap and row[len(c["c"][pk]):].any()
        for k, cap in zip(kk, caps):
            assert all(len(c["c"][k]) < cap for c in cs) and b[k].shape[:2] == (len(cs) + 1, cap)


def _filler(kind, like, prm):
    """A plain case under the group's call and camera with matched and spare keypoints on both images: the
    source of the poison rows for a group whose crafted cases leave no keypoint free."""
    big = float(like["grid"][1]) > 600
    s = util.ProjScene(kind, 99, W=W if big else 512, H=H if big else 512, uright=like.get("cur_uright") is not None,
                       kb8=like.get("kb8"), camera=like.get("camera"))
    for side in sides(s):
        for j in range(6):
            if s.kb8 is None:
                lone(s, RIGHT0 * side + 2 * j, side, flips=3 * j)
            s.kp(*spot(RIGHT0 * side + 40 + 2 * j), side=side)
    if s.kb8 is not None:
        s.pt(100.0, 100.0)
    c = s.case()
    return {"c": c, "call": prm, "ref": util.pj_oracle(c, prm)}


def _pack(kind, cs):
    """The padded, poisoned tables of one batched launch over the cases cs and their capacities."""
    import batch_pack as bp
    cases = [c["c"] for c in cs]
    c0 = cases[0]
    two = kind in ("proj2", "local2")
    kk, pk = ("kps", "kps_r") if two else ("cur_kps",), {"proj": "flags", "proj2": "flags", "reloc": "kf_flags",
                                                       "local": "mp_flags", "local2": "mp_flags"}[kind]
    caps = [max(len(c[k]) for c in cases) + 13 for k in kk]
    pcap = max(len(c[pk]) for c in cases) + 7
    ur = (not two) and kind != "reloc" and c0["cur_uright"] is not None
    if two:
        left, right = (bp.LOCAL2_LEFT, bp.LOCAL2_RIGHT) if kind == "local2" else (bp.LEFT, bp.RIGHT)
        b = {**bp.pack_keyed(cases, caps[0], left), **bp.pack_keyed(cases, caps[1], right)}
    else:
        b = bp.pack_keyed(cases, caps[0], bp.CUR_U if ur else bp.CUR)
    b.update(bp.pack_keyed(cases, pcap, {"proj": bp.PROJ_LAST, "proj2": bp.PROJ2_LAST, "reloc": bp.RELOC_KF,
                                         "local": bp.LOCAL_MP, "local2": bp.LOCAL2_MP}[kind]))
    return b, kk, pk, caps, pcap, ur


def _launch(kind, dev, cs):
    """One batched launch over the cases cs (every workgroup runs another case); returns the downloaded tables."""
    import batch_pack as bp
    cases, prm = [c["c"] for c in cs], cs[0]["call"]
    P = len(cases)
    c0 = cases[0]
    b, kk, pk, caps, pcap, ur = _pack(kind, cs)
    up = dev.up
    dk = [up(b[k]) for k in kk]
    dn = [up(bp.counts_array([len(c[k]) for c in cases])) for k in kk]
    dnp = up(bp.counts_array([len(c[pk]) for c in cases]))
    grids = [bp.assign_grid(dev, dk[j], dn[j], caps[j], P, c0["grid"], [c[kk[j]] for c in cases])
             for j in range(len(kk))]
    outs = [dev.canary(P + bp.SLACK, cap) for cap in caps]
    cnt, get_n = dev.canary(P + bp.SLACK)
    lib = dev.lib
    if kind in ("proj", "proj2"):
        p = util.proj_params(c0, prm["th"], prm["forward"], prm["backward"])
        p.check_orientation = prm["ori"]
    elif kind == "reloc":
        p = util.reloc_params(c0, prm["th"], prm["orb_dist"])
        p.check_orientation = prm["ori"]
    else:
        p = util.local_params(c0, prm["th"])
        p.nnratio = prm["nnratio"]
    if kind == "proj":
        rc = lib.plvi_search_by_projection_batch(
            P, ctypes.byref(p), dk[0], up(b["cur_desc"]), dn[0], caps[0], up(b["cur_blocked"]),
            up(b["cur_uright"]) if ur else None, *grids[0], up(b["x3dc"]), up(b["last_octave"]), up(b["last_angle"]),
            up(b["mp_desc"]), up(b["flags"]), dnp, pcap, outs[0][0], cnt, None)
    elif kind == "proj2":
        kb = None if c0["kb8"] is None else np.ascontiguousarray(c0["kb8"], np.float32)
        rc = lib.plvi_search_by_projection_stereo_batch(
            P, ctypes.byref(p), None if kb is None else kb.ctypes.data_as(ctypes.c_void_p), dk[0], up(b["desc"]), dn[0],
            caps[0], up(b["blocked"]), *grids[0], dk[1], up(b["desc_r"]), dn[1], caps[1], up(b["blocked_r"]), *grids[1],
            up(b["x3dc"]), up(b["x3dr"]), up(b["last_octave"]), up(b["last_angle"]), up(b["mp_desc"]), up(b["flags"]),
            dnp, pcap, outs[0][0], outs[1][0], cnt, None)
    elif kind == "reloc":
        rc = lib.plvi_search_reloc_batch(
            P, ctypes.byref(p), dk[0], up(b["cur_desc"]), dn[0], caps[0], up(b["cur_blocked"]), *grids[0],
            up(b["kf_flags"]), up(b["x3dc"]), up(b["dist"]), up(b["level"]), up(b["kf_angle"]), up(b["mp_desc"]), dnp,
            pcap, outs[0][0], cnt, None)
    elif kind == "local":
        rc = lib.plvi_search_local_batch(
            P, ctypes.byref(p), dk[0], up(b["cur_desc"]), dn[0], caps[0], up(b["cur_blocked"]),
            up(b["cur_uright"]) if ur else None, *grids[0], up(b["mp_flags"]), up(b["mp_proj"]), up(b["mp_level"]),
            up(b["mp_desc"]), dnp, pcap, outs[0][0], cnt, None)
    else:
        rc = lib.plvi_search_local_stereo_batch(
            P, ctypes.byref(p), dk[0], up(b["desc"]), dn[0], caps[0], up(b["blocked"]), up(b["l2r"]), *grids[0], dk[1],
            up(b["desc_r"]), dn[1], caps[1], up(b["blocked_r"]), up(b["r2l"]), *grids[1], up(b["mp_flags"]),
            up(b["mp_proj"]), up(b["mp_level"]), up(b["mp_proj_r"]), up(b["mp_level_r"]), up(b["mp_desc"]), dnp, pcap,
            outs[0][0], outs[1][0], cnt, None)
    assert rc == 0
    return [get() for _, get in outs], get_n()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_all_cases_of_a_kernel_as_batches(kind):
    """Every crafted case of the kernel in batched launches, one workgroup per case: capacities above the
    counts, poisoned padding rows, canary-filled outputs.  One launch takes one parameter struct, so the cases
    go in one launch per distinct call (th, forward / backward, nnratio, ORBdist, rotation check, camera)."""
    import batch_pack as bp
    dev = bp.Device()
    groups = batch_groups(kind)
    for cs in groups:
        tables, counts = _launch(kind, dev, cs)
        for side, got in enumerate(tables):
            bp.check_rows(got, [c["ref"][1][side] for c in cs], f"{kind} match table {side}")
        bp.check_counts(counts, [c["ref"][0] for c in cs], f"{kind} nmatches")
