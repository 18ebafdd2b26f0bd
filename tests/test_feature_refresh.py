"""plvi_feature_refresh[_batch] -- MapPoint / MapLine::UpdateNormalAndDepth and ComputeDistinctiveDescriptors for
a list of pool ids over resident tables.

Expected values come from tests/native/feature_refresh_ref.cpp (KeyFrame objects, std::map observations,
observations[pRefKF] indexed as the reference does, the OpenCV calls as helpers; DESC through distinctive_ref.cpp),
built here with -ffp-contract=off.  A second, independent pin in numpy (float32 arrays, explicit np.float64 for the
norm, a Python loop for the ordered sum) checks the crafted cases and random maps against it bit for bit on the CPU.
The GPU tests demand exact equality of every output of both forms over sentinel-filled tables."""
import ctypes
import functools
import pathlib
import subprocess

import numpy as np
import pytest

import plvi

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "feature_refresh_ref.cpp"
BUILD = ROOT / "tests" / "native" / "_build"

POINTS, LINES = plvi.REFRESH_POINTS, plvi.REFRESH_LINES
NORMAL, DESC = plvi.REFRESH_NORMAL, plvi.REFRESH_DESC
E_ROWS, E_REF, E_LEVEL, E_KEYPOINT = 1, 2, 4, 8
FMA = 16  # PLVI_COMPAT_SCALEADD_FMA
FILL, FILL8 = -7, -7 & 0x7f
S_NORMAL, S_DIST, S_DESC = np.float32(777.0), np.float32(555.0), 0xAB  # what an untouched row holds
KINDS = (POINTS, LINES)
f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------- maps
class Map:
    """Keyframe tables of one kind and a pool of features, each a list of (slot, index) observations."""

    def __init__(self, kind, kf_cap, cap, n_levels=8, seed=1):
        rng = self.rng = np.random.default_rng(seed)
        self.kind, self.kf_cap, self.cap, self.n_levels = kind, kf_cap, cap, n_levels
        self.kf = dict(bad=np.zeros(kf_cap, np.uint8), ow=rng.uniform(-4, 4, (kf_cap, 3)).astype(f32),
                       cnt=np.full(kf_cap, cap, np.int32),
                       # bits 6 and 7 belong to other readers of kp_info / kl_info
                       info=(rng.integers(0, n_levels, (kf_cap, cap)) | (rng.integers(0, 4, (kf_cap, cap)) << 6))
                       .astype(np.uint8),
                       desc=rng.integers(0, 256, (kf_cap, cap, 32)).astype(np.uint8))
        self.scale = (f32(1.2) ** np.arange(n_levels)).astype(f32)
        self.feats = []

    def add(self, obs, ref, where=None, bad=0):
        if where is None:
            where = self.rng.uniform(-9, 9, 6 if self.kind == LINES else 3)
        self.feats.append(dict(obs=list(obs), ref=ref, where=np.asarray(where, f64), bad=bad))
        return len(self.feats) - 1

    def octave(self, kf, idx, value):
        self.kf["info"][kf, idx] = value | (self.kf["info"][kf, idx] & 0xc0)

    def tables(self):
        n = len(self.feats)
        off = np.zeros(n + 1, np.int32)
        off[1:] = np.cumsum([len(f["obs"]) for f in self.feats])
        obs = [o for f in self.feats for o in f["obs"]]
        feat = dict(bad=np.array([f["bad"] for f in self.feats], np.uint8), obs_off=off,
                    obs_kf=np.array([o[0] for o in obs] + [0], np.int32),
                    obs_idx=np.array([o[1] for o in obs] + [0], np.int32),
                    ref_kf=np.array([f["ref"] for f in self.feats], np.int32),
                    normal=np.full((n, 3), S_NORMAL, f32), dist=np.full((n, 2), S_DIST, f32),
                    desc=np.full((n, 32), S_DESC, np.uint8))
        where = np.array([f["where"] for f in self.feats], f64).reshape(n, -1)
        feat["sep" if self.kind == LINES else "pos"] = where if self.kind == LINES else where.astype(f32)
        return self.kf, feat, self.scale


def max_obs_of(tabs):
    return max(int(np.diff(tabs[1]["obs_off"]).max(initial=1)), 1)


# ---------------------------------------------------------------- the restatement
class RefArgs(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("kind", "what", "fma_form", "n_levels", "max_obs", "row_cap")] + \
               [("scale", ctypes.c_void_p), ("kf_cap", ctypes.c_int), ("cap", ctypes.c_int)] + \
               [(k, ctypes.c_void_p) for k in ("kf_bad", "ow", "cnt", "info", "kf_desc")] + [("n", ctypes.c_int)] + \
               [(k, ctypes.c_void_p) for k in ("bad", "obs_off", "obs_kf", "obs_idx", "pos", "sep", "ref_kf", "ids")] + \
               [("n_ids", ctypes.c_int)] + \
               [(k, ctypes.c_void_p) for k in ("normal", "dist", "desc", "state", "best_pos", "best_median", "n_rows",
                                               "err", "seconds")]


@functools.lru_cache(None)
def ref_lib():
    so = BUILD / "libfeature_refresh_ref.so"
    deps = (SRC, SRC.parent / "distinctive_ref.cpp", ROOT / "include" / "plvi_frontend.h")
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        so.parent.mkdir(parents=True, exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-o",
                        str(so), str(SRC)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.feature_refresh_ref_run.argtypes, lib.feature_refresh_ref_run.restype = [ctypes.c_void_p], None
    return lib


def blank(n_ids):
    return dict(state=np.full(n_ids, FILL8, np.uint8), best_pos=np.full(n_ids, FILL, np.int32),
                best_median=np.full(n_ids, FILL, np.int32), n_rows=FILL, err=FILL)


def ref_refresh(tabs, kind, ids, what=NORMAL | DESC, compat=0, row_cap=None, max_obs=None, seconds=None):
    """The restatement on copies of the three columns.  Outputs that `what` leaves unwritten keep their fill."""
    kf, feat, scale = tabs
    ids = np.ascontiguousarray(ids, np.int32)
    max_obs = max_obs or max_obs_of(tabs)
    res = blank(len(ids))
    res.update({k: feat[k].copy() for k in ("normal", "dist", "desc")})
    n_rows, err, sec = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, f64)
    if not what & DESC:
        bp = bm = None
    else:
        bp, bm = res["best_pos"], res["best_median"]
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    a = RefArgs(kind, what, int(bool(compat & FMA)), len(scale), max_obs, 1 << 30 if row_cap is None else row_cap,
                p(scale), len(kf["bad"]), kf["info"].shape[1], p(kf["bad"]), p(kf["ow"]), p(kf["cnt"]),
                p(kf["info"]), p(kf["desc"]), len(feat["bad"]), p(feat["bad"]), p(feat["obs_off"]),
                p(feat["obs_kf"]), p(feat["obs_idx"]), p(feat.get("pos")), p(feat.get("sep")), p(feat["ref_kf"]),
                p(ids), len(ids), p(res["normal"]), p(res["dist"]), p(res["desc"]), p(res["state"]), p(bp), p(bm),
                p(n_rows), p(err), p(sec))
    ref_lib().feature_refresh_ref_run(ctypes.byref(a))
    res.update(n_rows=int(n_rows[0]), err=int(err[0]))
    if seconds is not None:
        seconds.append(float(sec[0]))
    return res


# ---------------------------------------------------------------- the numpy pin
def np_distinctive(rows):
    """BestIdx / BestMedian of ComputeDistinctiveDescriptors over descriptor rows [N][32]."""
    bits = np.unpackbits(rows, axis=1).astype(np.int32)
    d = (bits[:, None, :] != bits[None, :, :]).sum(axis=2)
    med = np.sort(d, axis=1)[:, (len(rows) - 1) // 2]
    return int(np.argmin(med)), int(med.min())


def np_refresh(tabs, kind, ids, what=NORMAL | DESC, compat=0, row_cap=None, max_obs=None):
    kf, feat, scale = tabs
    K, cap = kf["info"].shape
    n, n_levels = len(feat["bad"]), len(scale)
    max_obs = max_obs or max_obs_of(tabs)
    res = blank(len(ids))
    res.update({k: feat[k].copy() for k in ("normal", "dist", "desc")})
    res["state"][:] = 0
    err = 0

    def entries(i):
        if not 0 <= i < n or feat["bad"][i]:
            return []
        o, ln = feat["obs_off"][i], min(max(feat["obs_off"][i + 1] - feat["obs_off"][i], 0), max_obs)
        return [(int(feat["obs_kf"][o + t]), int(feat["obs_idx"][o + t])) for t in range(ln)]

    def norm(v):
        return np.sqrt(f64(v[0]) * f64(v[0]) + f64(v[1]) * f64(v[1]) + f64(v[2]) * f64(v[2]))

    with np.errstate(all="ignore"):
        for p, i in enumerate(ids):
            seen = [(k, x) for k, x in entries(i) if 0 <= k < K]
            if not what & NORMAL or not seen:
                continue
            if kind == LINES:
                pos = ((feat["sep"][i, :3] + feat["sep"][i, 3:]) * f64(0.5)).astype(f32)
            else:
                pos = feat["pos"][i]
            acc = np.zeros(3, f32)
            for k, _ in seen:
                d = pos - kf["ow"][k]
                alpha = f32(f64(1.0) / norm(d))
                if compat & FMA:  # one rounding: exact in float64 products of float32, then the sum
                    acc = np.array([fma32(d[c], alpha, acc[c]) for c in range(3)], f32)
                else:
                    acc = (d * alpha).astype(f32) + acc
            ref = int(feat["ref_kf"][i])
            if not 0 <= ref < K:
                err |= E_REF
                continue
            level = 0
            if kind == POINTS:
                idx = next((x for k, x in seen if k == ref), 0)
                if not 0 <= idx < min(max(kf["cnt"][ref], 0), cap):
                    err |= E_KEYPOINT
                    continue
                level = int(kf["info"][ref, idx] & 63)
            if level >= n_levels:
                err |= E_LEVEL
                continue
            dist = f32(norm(pos - kf["ow"][ref]))
            dmax = f32(dist * scale[level])
            res["normal"][i] = acc * f32(f64(1.0) / f64(len(seen)))
            res["dist"][i] = (f32(dmax / scale[n_levels - 1]), dmax)
            res["state"][p] |= NORMAL
        if what & DESC:
            lists = [entries(i) for i in ids]
            res["n_rows"] = sum(len(e) for e in lists)
            over = res["n_rows"] > (1 << 30 if row_cap is None else row_cap)
            err |= E_ROWS if over else 0
            for p, (i, e) in enumerate(zip(ids, lists)):
                live = [t for t, (k, x) in enumerate(e) if 0 <= k < K and not kf["bad"][k]
                        and 0 <= x < min(max(kf["cnt"][k], 0), cap)]
                res["best_pos"][p] = res["best_median"][p] = -1
                if over or not live:
                    continue
                b, m = np_distinctive(np.array([kf["desc"][e[t][0], e[t][1]] for t in live]))
                res["best_pos"][p], res["best_median"][p] = live[b], m
                res["desc"][i] = kf["desc"][e[live[b]][0], e[live[b]][1]]
                res["state"][p] |= DESC
        else:
            res["n_rows"] = 0
    res["err"] = err
    return res


def fma32(a, b, c):
    """fmaf(a, b, c): the product of two float32 is exact in float64; the sum is rounded once to float32 through
    round-to-odd in float64 (53 bits are more than 2 * 24 + 2)."""
    p = f64(a) * f64(b)
    s = p + f64(c)
    if not np.isfinite(s):
        return f32(s)
    bb = s - p
    e = (p - (s - bb)) + (f64(c) - bb)  # TwoSum: s + e is the exact sum
    if e != 0:
        u = s.view(np.uint64) if isinstance(s, np.ndarray) else np.array([s], f64).view(np.uint64)[0]
        if not u & np.uint64(1):  # round to odd: step towards e, which sets the low bit
            s = np.nextafter(s, f64(np.inf) if e > 0 else f64(-np.inf))
    return f32(s)


def same(got, exp, nan_rows=()):
    """Bit-for-bit equality of two results; in the rows nan_rows of normal, NaN equals NaN whatever its payload."""
    for k in ("normal", "dist", "desc", "state", "best_pos", "best_median"):
        g, e = np.ascontiguousarray(got[k]), np.ascontiguousarray(exp[k])
        if k == "normal" and len(nan_rows):
            g, e = g.copy(), e.copy()
            for r in nan_rows:
                assert np.array_equal(np.isnan(g[r]), np.isnan(e[r])), (k, r)
                g[r][np.isnan(g[r])] = 0
                e[r][np.isnan(e[r])] = 0
        w = np.uint32 if g.dtype == f32 else g.dtype
        bad = np.nonzero((g.view(w) != e.view(w)).reshape(len(g), -1).any(axis=1))[0]
        assert not len(bad), (k, bad[:8], g[bad[:3]], e[bad[:3]])
    assert (got["n_rows"], got["err"]) == (exp["n_rows"], exp["err"]), (got["n_rows"], got["err"], exp["n_rows"],
                                                                         exp["err"])


# ---------------------------------------------------------------- crafted cases
@functools.lru_cache(None)
def crafted(kind):
    """One map of a kind, cap = 4, with every case a feature (or two).  Returns (tabs, cases, ids, nan_rows):
    cases[name] = (feature ids, check(exp, tabs)) where check asserts what the case is there to show."""
    m = Map(kind, kf_cap=7, cap=4, n_levels=8, seed=11 + kind)
    m.kf["bad"][3] = 1
    m.kf["cnt"][5] = 0
    K = m.kf_cap
    cases = {}
    untouched = lambda e, i: (e["normal"][i] == S_NORMAL).all() and (e["dist"][i] == S_DIST).all()  # noqa: E731

    a = m.add([(1, 2)], 1)

    def one(e, t):
        assert e["state"][ids.index(a)] == NORMAL | DESC and e["best_pos"][ids.index(a)] == 0
        assert abs(float(np.linalg.norm(e["normal"][a].astype(f64))) - 1) < 1e-6  # n = 1: a unit vector
        assert (e["desc"][a] == t[0]["desc"][1, 2]).all()
    cases["list_of_1"] = ([a], one)

    b = m.add([(0, 1), (2, 3)], 2)
    cases["list_of_2"] = ([b], lambda e, t: (e["state"][ids.index(b)] == 3
                                             and float(np.linalg.norm(e["normal"][b])) <= 1) or pytest.fail("list_of_2"))

    where = m.rng.uniform(-9, 9, 6 if kind == LINES else 3)
    c = m.add([(0, 0), (3, 1), (4, 2), (6, 1)], 0, where)   # slot 3 is bad
    c2 = m.add([(0, 0), (4, 2), (6, 1)], 0, where)
    m.kf["desc"][3, 1] = m.kf["desc"][0, 0]                 # were it counted it would pull the median

    def bad_observer(e, t):
        assert e["state"][ids.index(c)] == 3
        assert e["normal"][c].tobytes() != e["normal"][c2].tobytes()   # it moves the normal
        assert e["best_pos"][ids.index(c)] in (0, 2, 3) and (e["desc"][c] == e["desc"][c2]).all()  # not the choice
    cases["bad_observer"] = ([c, c2], bad_observer)

    d = m.add([(-1, 0), (1, 1), (K + 3, 2), (2, 9), (4, 0)], 1, where)   # (2, 9): an index past the row, DESC only
    d2 = m.add([(1, 1), (2, 0), (4, 0)], 1, where)

    def outside(e, t):
        assert e["normal"][d].tobytes() == e["normal"][d2].tobytes() and e["dist"][d].tobytes() == e["dist"][d2].tobytes()
        assert e["best_pos"][ids.index(d)] in (1, 4)   # positions count the ignored entries
    cases["slot_outside"] = ([d, d2], outside)

    if kind == POINTS:
        m.octave(6, 0, 5)
        for x in (1, 2, 3):
            m.octave(6, x, 2)
        m.octave(0, 1, 1), m.octave(2, 2, 1)
        g = m.add([(0, 1), (2, 2)], 6)      # ref_kf 6 is absent: keypoint 0 of slot 6, octave 5

        def absent(e, t):
            assert e["state"][ids.index(g)] & NORMAL
            assert e["dist"][g][1] / e["dist"][g][0] == pytest.approx(float(t[2][7]), rel=1e-6)
            dist = np.sqrt(((t[1]["pos"][g] - t[0]["ow"][6]).astype(f64) ** 2).sum())
            assert e["dist"][g][1] == pytest.approx(dist * float(t[2][5]), rel=1e-6)
        cases["ref_absent"] = ([g], absent)

        q = m.add([(0, 1), (2, 2)], 5)      # absent and cnt[5] == 0: there is no keypoint 0
        cases["ref_absent_no_keypoint"] = ([q], lambda e, t: (untouched(e, q) and e["err"] & E_KEYPOINT
                                                              and e["state"][ids.index(q)] == DESC)
                                           or pytest.fail("cnt 0"))
        m.octave(4, 3, 7), m.octave(4, 1, 8)
        l7 = m.add([(1, 0), (4, 3)], 4)
        l8 = m.add([(1, 0), (4, 1)], 4)

        def levels(e, t):
            assert e["state"][ids.index(l7)] & NORMAL and e["dist"][l7][0] == pytest.approx(
                float(e["dist"][l7][1]) / float(t[2][7]), rel=1e-6)
            assert e["dist"][l7][1] == pytest.approx(float(e["dist"][l7][0]) * float(t[2][7]), rel=1e-6)
            assert untouched(e, l8) and e["err"] & E_LEVEL and e["state"][ids.index(l8)] == DESC
        cases["level_last_and_past"] = ([l7, l8], levels)
    else:
        g = m.add([(0, 1), (2, 2)], 6)      # lines: level 0 whatever the octaves, ref absent or not

        def level0(e, t):
            assert e["dist"][g][1] / e["dist"][g][0] == pytest.approx(float(t[2][7]), rel=1e-6)
            assert e["dist"][g][1].tobytes() == f32(f32(e["dist"][g][1]) * t[2][0]).tobytes()
        cases["line_level_0"] = ([g], level0)
        h = m.add([(0, 0), (1, 1)], 0, [1.0, 2.0, 3.0, 1.0 + 2.0 ** -30, 2.0 + 2.0 ** -29, 3.0 + 2.0 ** -28])

        def midpoint(e, t):
            mid = (t[1]["sep"][h, :3] + t[1]["sep"][h, 3:]) * 0.5
            assert (mid.astype(f32).astype(f64) != mid).all() and e["state"][ids.index(h)] & NORMAL
        cases["midpoint_not_float"] = ([h], midpoint)

    r = m.add([(0, 1), (2, 2)], K)
    r2 = m.add([(0, 1), (2, 2)], -1)
    cases["ref_out_of_range"] = ([r, r2], lambda e, t: (untouched(e, r) and untouched(e, r2) and e["err"] & E_REF
                                                        and e["state"][ids.index(r)] == DESC) or pytest.fail("ref"))
    u = m.add([(0, 1), (2, 2)], 0, bad=1)
    v = m.add([], 0)
    v2 = m.add([(-1, 0), (K, 0)], 0)        # nothing left of the list
    cases["bad_and_empty_untouched"] = ([u, v, v2], lambda e, t: all(
        untouched(e, i) and (e["desc"][i] == S_DESC).all() and e["state"][ids.index(i)] == 0
        and e["best_pos"][ids.index(i)] == -1 for i in (u, v, v2)) or pytest.fail("untouched"))

    ow1 = m.kf["ow"][1].astype(f64)
    z = m.add([(1, 0), (2, 0)], 2, np.concatenate([ow1, ow1]) if kind == LINES else ow1)   # s = 0 at slot 1
    cases["at_camera_centre"] = ([z], lambda e, t: (np.isnan(e["normal"][z]).any() and e["state"][ids.index(z)] & NORMAL
                                                    and np.isfinite(e["dist"][z]).all()) or pytest.fail("nan"))
    dup = m.add([(0, 2), (1, 1), (4, 3)], 1)

    def duplicate(e, t):
        pos = [p for p, i in enumerate(ids) if i == dup]
        assert len(pos) == 2 and (e["state"][pos] == 3).all() and e["best_pos"][pos[0]] == e["best_pos"][pos[1]]
    cases["duplicate_id"] = ([dup], duplicate)

    n = len(m.feats)
    ids = [-1] + list(range(n)) + [n, dup, 1 << 30]
    return m.tables(), cases, ids, (z,)


CASE_IDS = [(kind, name) for kind in KINDS for name in crafted(kind)[1]]


@functools.lru_cache(None)
def crafted_expected(kind, what=NORMAL | DESC, compat=0):
    tabs, _, ids, _ = crafted(kind)
    return ref_refresh(tabs, kind, ids, what, compat)


@pytest.mark.parametrize("kind,name", CASE_IDS)
def test_crafted_case_shows_what_it_is_for(kind, name):
    tabs, cases, ids, _ = crafted(kind)
    exp = crafted_expected(kind)
    cases[name][1](exp, tabs)
    assert exp["state"][0] == 0 and exp["state"][-1] == 0 and exp["state"][-3] == 0   # ids outside the pool


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("compat", (0, FMA))
@pytest.mark.parametrize("what", (NORMAL, DESC, NORMAL | DESC))
def test_crafted_numpy_pin_agrees(kind, compat, what):
    tabs, _, ids, nan_rows = crafted(kind)
    same(np_refresh(tabs, kind, ids, what, compat), crafted_expected(kind, what, compat), nan_rows)


@pytest.mark.parametrize("kind", KINDS)
def test_row_cap_below_at_above(kind):
    tabs, _, ids, nan_rows = crafted(kind)
    full = crafted_expected(kind)
    n_rows = full["n_rows"]
    assert n_rows > 3 and not full["err"] & E_ROWS
    for cap in (n_rows - 1, n_rows, n_rows + 1):
        exp = ref_refresh(tabs, kind, ids, row_cap=cap)
        same(np_refresh(tabs, kind, ids, row_cap=cap), exp, nan_rows)
        assert exp["n_rows"] == n_rows                         # the full length is always reported
        if cap < n_rows:
            assert exp["err"] & E_ROWS and not (exp["state"] & DESC).any() and (exp["best_pos"] == -1).all()
            assert (exp["desc"] == S_DESC).all()
            assert (exp["state"] & NORMAL).tolist() == (full["state"] & NORMAL).tolist()   # NORMAL is unaffected
            assert exp["normal"].tobytes() == full["normal"].tobytes()
        else:
            same(exp, full, nan_rows)


# ---------------------------------------------------------------- random maps
def random_map(kind, seed, kf_cap=40, cap=6, n_feat=200, lens=None, n_bad_kf=3, clean=False):
    """Lists in ascending slot order (the iteration order of the restatement's std::map), each slot once."""
    m = Map(kind, kf_cap, cap, n_levels=8, seed=seed)
    rng = m.rng
    if n_bad_kf:
        m.kf["bad"][rng.choice(kf_cap, min(n_bad_kf, kf_cap), replace=False)] = 1
    m.kf["cnt"][:] = rng.integers(max(cap - 2, 1), cap + 1, kf_cap)
    for f in range(n_feat):
        ln = int(lens[f]) if lens is not None else int(rng.integers(0, min(13, kf_cap + 1)))
        slots = np.sort(rng.choice(kf_cap, ln, replace=False))
        obs = [(int(s), int(rng.integers(0, m.kf["cnt"][s]))) for s in slots]
        if not clean and ln and rng.random() < 0.1:
            obs = [(-2, 0)] + obs + [(kf_cap + 1, 1)]
        if ln and (clean or rng.random() < 0.8):
            ref = obs[int(rng.integers(0, len(obs)))][0]
        else:
            ref = int(rng.integers(0, kf_cap))
        m.add(obs, ref, bad=0 if clean else int(rng.random() < 0.05))
    return m.tables()


@functools.lru_cache(None)
def random_case(kind):
    tabs = random_map(kind, seed=100 + kind)
    rng = np.random.default_rng(5)
    ids = rng.permutation(len(tabs[1]["bad"])).tolist() + [3, 3, -5, 10 ** 6]
    return tabs, ids


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("compat", (0, FMA))
def test_random_maps_restatements_agree_and_cover(kind, compat):
    tabs, ids = random_case(kind)
    exp = ref_refresh(tabs, kind, ids, compat=compat)
    same(np_refresh(tabs, kind, ids, compat=compat), exp)
    st = exp["state"]
    assert (st == 3).sum() > 100 and (st == 0).sum() > 5
    kf, feat, _ = tabs
    absent = sum(1 for i in range(len(feat["bad"])) if feat["ref_kf"][i] not in
                 feat["obs_kf"][feat["obs_off"][i]:feat["obs_off"][i + 1]])
    assert absent > 10                                          # the default-constructed entry is exercised
    assert max_obs_of(tabs) > 8                                 # past the 8-lane groups


def test_the_two_compat_forms_differ_and_where_they_cannot():
    """From the restatement alone: of 200 random features at least 50 change with the contraction (140 when this
    was written), and a feature with one observer cannot (fma(x, a, 0) = x * a)."""
    tabs = random_map(POINTS, seed=77, clean=True, lens=np.random.default_rng(3).integers(2, 13, 200))
    ids = list(range(200))
    a, b = ref_refresh(tabs, POINTS, ids, NORMAL, 0), ref_refresh(tabs, POINTS, ids, NORMAL, FMA)
    assert (a["state"] == NORMAL).all() and (b["state"] == NORMAL).all()
    differ = int((a["normal"].view(np.uint32) != b["normal"].view(np.uint32)).any(axis=1).sum())
    print("features whose normal differs between the forms:", differ)
    assert differ >= 50
    assert a["dist"].tobytes() == b["dist"].tobytes()
    ctabs, _, ids, _ = crafted(POINTS)
    one = crafted(POINTS)[1]["list_of_1"][0][0]
    assert crafted_expected(POINTS, NORMAL | DESC, 0)["normal"][one].tobytes() == \
        crafted_expected(POINTS, NORMAL | DESC, FMA)["normal"][one].tobytes()


# ---------------------------------------------------------------- the device
def refresher(tabs, kind, max_obs=None, compat=0):
    kf, feat, scale = tabs
    return plvi.FeatureRefresh(kf, {k: a.copy() for k, a in feat.items()}, kind, scale, max_obs=max_obs, compat=compat)


def plain(r):
    assert set(np.atleast_1d(r["past"]["state"]).tolist()) <= {FILL8}, "state written past the batch"
    for k in ("best_pos", "best_median"):
        assert r["past"].get(k, FILL) == FILL, f"{k} written past the batch"
    n = len(r["state"])
    out = {k: r[k] for k in ("normal", "dist", "desc", "state", "n_rows", "err")}
    out.update({k: r.get(k, np.full(n, FILL, np.int32)) for k in ("best_pos", "best_median")})
    return out


def both_forms_equal(tabs, kind, ids, what=NORMAL | DESC, compat=0, row_cap=None, nan_rows=(), exp=None, best=True,
                     host=True):
    exp = exp or ref_refresh(tabs, kind, ids, what, compat, row_cap)
    if not best:
        exp = dict(exp, best_pos=np.full(len(ids), FILL, np.int32), best_median=np.full(len(ids), FILL, np.int32))
    got = refresher(tabs, kind).batch(ids, what, row_cap, compat, best=best, fill=FILL)
    assert got["rc"] == 0
    same(plain(got), exp, nan_rows)
    if host:
        got = refresher(tabs, kind).host(ids, what, row_cap, compat, best=best, fill=FILL)
        assert got["rc"] == (plvi.PLVI_E_CAPACITY if exp["err"] else int((exp["state"] & NORMAL).sum()))
        same(plain(got), exp, nan_rows)
    return exp


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("compat", (0, FMA))
@pytest.mark.parametrize("what", (NORMAL, DESC, NORMAL | DESC))
def test_gpu_crafted_cases_one_batch(plvi_lib, kind, compat, what):
    tabs, _, ids, nan_rows = crafted(kind)
    both_forms_equal(tabs, kind, ids, what, compat, nan_rows=nan_rows, exp=crafted_expected(kind, what, compat))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_row_cap_below_at_above_and_null_optionals(plvi_lib, kind):
    tabs, _, ids, nan_rows = crafted(kind)
    n_rows = crafted_expected(kind)["n_rows"]
    for cap in (n_rows - 1, n_rows, n_rows + 1):
        both_forms_equal(tabs, kind, ids, row_cap=cap, nan_rows=nan_rows)
    both_forms_equal(tabs, kind, ids, nan_rows=nan_rows, best=False)
    both_forms_equal(tabs, kind, ids, row_cap=n_rows - 1, nan_rows=nan_rows, best=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("compat", (0, FMA))
def test_gpu_random_maps(plvi_lib, kind, compat):
    tabs, ids = random_case(kind)
    both_forms_equal(tabs, kind, ids, compat=compat)


@functools.lru_cache(None)
def shape_map(kind, kf_cap):
    if kf_cap == 3:
        lens = [0, 1, 2, 3] * 17
    else:
        lens = [0, 1, 2, 31, 32, 33, 63, 64, 65] + list(np.random.default_rng(9).integers(0, 40, 56))
    return random_map(kind, seed=40 + kf_cap, kf_cap=kf_cap, cap=4, n_feat=len(lens), lens=lens, n_bad_kf=kf_cap // 20)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kf_cap", (3, 300))
def test_gpu_list_lengths_and_id_counts(plvi_lib, kind, kf_cap):
    """cap = 4; lists of 0, 1, 2, 31, 32, 33, 63, 64 and 65 entries; 1 and 65 ids, in both compat forms."""
    tabs = shape_map(kind, kf_cap)
    n = len(tabs[1]["bad"])
    assert n == 65 or kf_cap == 3
    both_forms_equal(tabs, kind, list(range(65)), compat=0)
    both_forms_equal(tabs, kind, list(range(65))[::-1], compat=FMA, host=False)
    for i in (2, 8 if kf_cap == 300 else 3):
        both_forms_equal(tabs, kind, [i], compat=FMA, host=False)


@functools.lru_cache(None)
def long_map(kind):
    lens = [2048, 3, 0, 70, 1]
    return random_map(kind, seed=61, kf_cap=2100, cap=4, n_feat=len(lens), lens=lens, n_bad_kf=40, clean=True)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_one_list_of_2048(plvi_lib, kind):
    tabs = long_map(kind)
    assert max_obs_of(tabs) == plvi_lib_max_obs()
    for compat in (0, FMA):
        both_forms_equal(tabs, kind, [1, 0, 3, 2, 4], compat=compat, host=compat == 0)


def plvi_lib_max_obs():
    return 2048  # PLVI_DISTINCTIVE_MAX_OBS


@pytest.mark.gpu
def test_gpu_ids_one_past_the_scan_tile(plvi_lib):
    """4097 ids, one past the 4096-id tile of the CSR kernel; only the last contributes rows."""
    tabs, _, _, _ = crafted(POINTS)
    cases = crafted(POINTS)[1]
    empty, full = cases["bad_and_empty_untouched"][0][1], cases["bad_observer"][0][0]
    ids = [empty] * 4096 + [full]
    exp = both_forms_equal(tabs, POINTS, ids, host=False)
    assert exp["n_rows"] == 4 and exp["state"][-1] == 3 and not exp["state"][:-1].any()


@pytest.mark.gpu
def test_gpu_graph_capture_and_replay(plvi_lib):
    """One call captured into a hipGraph and replayed once: no host read, no allocation, no sync inside."""
    tabs, ids = random_case(POINTS)
    fr = refresher(tabs, POINTS)
    step, fetch = fr.batch(ids, fill=FILL, run=False)
    st = ctypes.c_void_p()
    assert plvi_lib.plvi_stream_create(ctypes.byref(st)) == 0
    rcs = []
    graph = plvi.StepGraph(lambda s: rcs.append(step(s)), st.value)
    assert rcs == [0]
    before = fetch()
    assert (before["state"] == FILL8).all() and (before["normal"] == S_NORMAL).all()   # captured, not run
    graph.launch()
    assert plvi_lib.plvi_stream_synchronize(st) == 0
    same(plain(fetch()), ref_refresh(tabs, POINTS, ids))


@pytest.mark.gpu
def test_gpu_refusals(plvi_lib):
    tabs, _, ids, _ = crafted(POINTS)
    fr = refresher(tabs, POINTS)
    assert fr.batch(ids, what=0)["rc"] == plvi.PLVI_E_BADARG
    assert fr.batch(ids, what=4)["rc"] == plvi.PLVI_E_BADARG
    fr.max_obs = 2049
    assert fr.batch(ids)["rc"] == plvi.PLVI_E_CAPACITY
    fr.max_obs = 4
    r = fr.batch([], fill=FILL)
    assert (r["rc"], r["n_rows"], r["err"]) == (0, 0, 0)
