"""Keyframe culling on the device (csrc/cull.hip, plvi_keyframe_culling[_batch]): the redundancy walk of
LocalMapping::KeyFrameCulling() / KeyFrameCullingWithLines() (src/LocalMapping.cc:1566-1718 / :1720-1964).

Expected values come from tests/native/cull_ref.cpp, a sequential host restatement in the reference's own shape
(KeyFrame / MapPoint / MapLine objects, std::map observations copied per feature, an nObs member, EraseObservation and
SetBadFlag with their cascade, mPrevKF / mNextKF pointers, a table of norm verdicts).  The CPU part pins it against
np_walk below, an independent restatement in the SET formulation the kernel uses -- live nObs and dead features as
functions of the set of erased keyframes, observer counts by bincount -- on every crafted case and on 240 random maps,
and asserts what each crafted case is there to show.  The gpu part demands exact equality with the restatement for
every output, with sentinel-filled tables.

A case is (map, params, query, check): params = redundant_th / monocular / inertial / slam_mode, query = q_slot,
abort_ba, n_kf_in_map, imu_init, inertial_ba2, norm (verdicts by slot, -1 = the walk stops)."""
import ctypes
import functools
import pathlib
import subprocess

import numpy as np
import pytest

import plvi

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "cull_ref.cpp"
BUILD = ROOT / "tests" / "native" / "_build"
FILL, FILL8 = -7, -7 & 0x7f
E_BADARG, E_CAPACITY = -2, -3
(SKIP_INIT, SKIP_BAD, KEEP, KEEP_FEW_KF, KEEP_RECENT, KEEP_NO_CHAIN, KEEP_TIME, KEEP_NORM, CULLED, CULLED_TIME,
 CULLED_NORM, NEEDS_NORM) = range(1, 13)
DEFERRED = 0x80
END, BREAK_ABORT, BREAK_100, STOP_NORM = range(4)
K_POINTS, K_LINES, K_RELINKED, K_DEFERRED = 1, 2, 4, 8
PER_Q = ("n_visited", "stop", "n_kf_in_map", "err", "n_changed")
PER_C = ("outcome", "n_mps", "n_mls", "n_redundant")
PER_CH = ("changed_slot", "changed_kind")
DEPTH, TWO = 0x40, 0x80


# ------------------------------------------------------------------ the map
class CullMap:
    """Keyframe tables and the two pools, built from observations so that the precondition holds: every
    observation (id, K, idx) has table[K][idx] == id."""

    def __init__(self, K, kp_cap=128, kl_cap=0, cand_stride=None):
        self.K, self.cap = K, (kp_cap, kl_cap)
        self.tab = [np.full((K, c), -1, np.int32) for c in self.cap]
        self.ntab = [np.zeros(K, np.int32) for _ in self.cap]
        self.info = [np.zeros((K, c), np.uint8) for c in self.cap]
        self.bad, self.init, self.not_erase = (np.zeros(K, np.uint8) for _ in range(3))
        self.obs = [[], []]       # per kind, per feature: [(kf, idx)]
        self.nobs = [[], []]      # per kind, per feature: Observations() or None = sum of the weights
        self.fbad = [[], []]
        self.null_nobs = [False, False]
        self.cand = [[] for _ in range(K)]
        self.cand_stride = cand_stride
        self.kf_id = np.arange(K, dtype=np.uint32) + 10
        self.ts = np.arange(K, dtype=np.float64)
        self.prev = np.full(K, -1, np.int32)
        self.next = np.full(K, -1, np.int32)

    def put(self, kind, kf, fid, octave=0, flags=0):
        """A table entry alone (no observation); returns its index."""
        i = int(self.ntab[kind][kf])
        assert i < self.cap[kind], "table full"
        self.tab[kind][kf, i] = fid
        self.info[kind][kf, i] = octave | flags
        self.ntab[kind][kf] = i + 1
        return i

    def add(self, kind, observers, nobs=None, bad=0):
        """A feature observed by `observers`: (kf, octave) or (kf, octave, flags).  Returns its id."""
        fid = len(self.obs[kind])
        self.obs[kind].append([(o[0], self.put(kind, o[0], fid, o[1], o[2] if len(o) > 2 else 0)) for o in observers])
        self.nobs[kind].append(nobs)
        self.fbad[kind].append(bad)
        return fid

    def chain(self, slots, t0=0.0, dt=1.0):
        for a, b in zip(slots, slots[1:]):
            self.next[a], self.prev[b] = b, a
        for i, s in enumerate(slots):
            self.ts[s] = t0 + i * dt

    def pool(self, kind):
        obs = self.obs[kind]
        off = np.zeros(len(obs) + 1, np.int32)
        off[1:] = np.cumsum([len(o) for o in obs])
        flat = [e for o in obs for e in o]
        okf = np.array([e[0] for e in flat], np.int32)
        oidx = np.array([e[1] for e in flat], np.int32)
        p = dict(bad=np.array(self.fbad[kind], np.uint8), obs_off=off, obs_kf=okf, obs_idx=oidx)
        if not self.null_nobs[kind]:
            nobs = []
            for o, n in zip(obs, self.nobs[kind]):
                if n is None:   # what AddObservation made of it: 2 for a stereo point, 1 for a line
                    n = sum(2 if kind == 0 and 0 <= k < self.K and 0 <= i < self.cap[0]
                            and self.info[0][k, i] & TWO else 1 for k, i in o)
                nobs.append(n)
            p["nobs"] = np.array(nobs, np.int32)
        return p

    def tables(self):
        stride = self.cand_stride or max(1, max(len(c) for c in self.cand))
        cand = np.full((self.K, stride), -1, np.int32)
        for s, c in enumerate(self.cand):
            cand[s, :len(c)] = c
        kf = dict(bad=self.bad, init_kf=self.init, not_erase=self.not_erase, mp=self.tab[0], nmp=self.ntab[0],
                  kp_info=self.info[0], cand=cand, n_cand=np.array([len(c) for c in self.cand], np.int32),
                  kf_id=self.kf_id, timestamp=self.ts, prev_kf=self.prev, next_kf=self.next)
        if self.cap[1]:
            kf.update(ml=self.tab[1], nml=self.ntab[1], kl_info=self.info[1])
        return kf, self.pool(0), self.pool(1) if self.cap[1] else None


def params(redundant_th=0.9, monocular=1, inertial=0, slam_mode=0):
    return dict(redundant_th=redundant_th, monocular=monocular, inertial=inertial, slam_mode=slam_mode)


def query(q_slot=0, abort_ba=0, n_kf_in_map=50, imu_init=0, inertial_ba2=0, norm=None):
    return dict(q_slot=q_slot, abort_ba=abort_ba, n_kf_in_map=n_kf_in_map, imu_init=imu_init,
                inertial_ba2=inertial_ba2, norm=norm)


def blank(out_cap, changed_cap):
    r = {k: FILL for k in PER_Q}
    r.update({k: np.full(max(out_cap, 1), FILL8 if k == "outcome" else FILL, np.uint8 if k == "outcome" else np.int32)
              for k in PER_C})
    r.update({k: np.full(max(changed_cap, 1), FILL, np.int32) for k in PER_CH})
    return r


def plain(r):
    return {k: (r[k].tolist() if isinstance(r[k], np.ndarray) else int(r[k])) for k in PER_Q + PER_C + PER_CH}


# ------------------------------------------------------- the restatement (C++)
class RefTables(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("kf_cap", "kp_cap", "kl_cap", "cand_stride")] + \
               [(k, ctypes.c_void_p) for k in ("bad", "init_kf", "not_erase", "mp", "nmp", "ml", "nml", "kp_info",
                                               "kl_info", "cand", "n_cand", "kf_id", "timestamp", "prev_kf",
                                               "next_kf")] + \
               [("mp_n", ctypes.c_int)] + \
               [(k, ctypes.c_void_p) for k in ("mp_bad", "mp_obs_off", "mp_obs_kf", "mp_obs_idx", "mp_nobs")] + \
               [("ml_n", ctypes.c_int)] + \
               [(k, ctypes.c_void_p) for k in ("ml_bad", "ml_obs_off", "ml_obs_kf", "ml_obs_idx", "ml_nobs")] + \
               [("redundant_th", ctypes.c_float)] + [(k, ctypes.c_int) for k in ("monocular", "inertial", "slam_mode")]


class RefQuery(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("q_slot", "abort_ba", "n_kf_in_map", "imu_init", "inertial_ba2")] + \
               [("norm_verdict", ctypes.c_void_p), ("out_cap", ctypes.c_int), ("changed_cap", ctypes.c_int)] + \
               [(k, ctypes.c_void_p) for k in ("n_visited", "stop", "n_kf_out", "err", "outcome", "n_mps", "n_mls",
                                               "n_redundant", "n_changed", "changed_slot", "changed_kind", "n_dead",
                                               "seconds")]


@functools.lru_cache(None)
def ref_lib():
    so = BUILD / "libcull_ref.so"
    if not so.exists() or so.stat().st_mtime < SRC.stat().st_mtime:
        so.parent.mkdir(parents=True, exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", str(so), str(SRC)],
                       check=True)
    lib = ctypes.CDLL(str(so))
    lib.cull_ref_run.argtypes, lib.cull_ref_run.restype = [ctypes.c_void_p, ctypes.c_void_p], None
    return lib


def ref_tables(tabs, P):
    """(RefTables, the arrays it points into)."""
    kf, mp, ml = tabs
    shape = lambda k: kf[k].shape[1] if k in kf else 0  # noqa: E731
    t = RefTables(len(kf["bad"]), shape("mp"), shape("ml"), shape("cand"))
    keep = []

    def ptr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return a.ctypes.data
    for k, dt in plvi._CULL_KF.items():
        setattr(t, k, ptr(kf.get(k), dt))
    for g, p in (("mp", mp), ("ml", ml)):
        setattr(t, g + "_n", 0 if p is None else len(p["bad"]))
        for k, dt in plvi._CULL_POOL.items():
            setattr(t, f"{g}_{k}", None if p is None else ptr(p.get(k), dt))
    t.redundant_th, t.monocular, t.inertial, t.slam_mode = (P[k] for k in ("redundant_th", "monocular", "inertial",
                                                                          "slam_mode"))
    return t, keep


def ref_walk(tabs, P, Q, out_cap, changed_cap, extra=None):
    t, keep = ref_tables(tabs, P)
    r = blank(out_cap, changed_cap)
    scal = {k: np.full(1, FILL, np.int32) for k in PER_Q + ("n_dead",)}
    sec = np.zeros(1, np.float64)
    norm = None if Q["norm"] is None else np.ascontiguousarray(Q["norm"], np.int32)
    q = RefQuery(Q["q_slot"], Q["abort_ba"], Q["n_kf_in_map"], Q["imu_init"], Q["inertial_ba2"],
                 None if norm is None else norm.ctypes.data, out_cap, changed_cap)
    for k, f in (("n_visited", "n_visited"), ("stop", "stop"), ("n_kf_in_map", "n_kf_out"), ("err", "err"),
                 ("n_changed", "n_changed"), ("n_dead", "n_dead")):
        setattr(q, f, scal[k].ctypes.data)
    for k in PER_C + PER_CH:
        setattr(q, k, r[k].ctypes.data)
    q.seconds = sec.ctypes.data
    ref_lib().cull_ref_run(ctypes.byref(t), ctypes.byref(q))
    r.update({k: int(scal[k][0]) for k in PER_Q})
    if extra is not None:
        extra.update(n_dead=int(scal["n_dead"][0]), seconds=float(sec[0]))
    return plain(r)


# -------------------------------------------- the set formulation (numpy)
def np_count(tabs, kind, K, erased, monocular, need):
    """(n, n_redundant, n_dead_total) of keyframe K's table of `kind` with the keyframes `erased` gone."""
    kf, mp, ml = tabs
    pool = ml if kind else mp
    tab, ntab, info = (kf[k] for k in (("ml", "nml", "kl_info") if kind else ("mp", "nmp", "kp_info")))
    n_kf, cap, n = tab.shape[0], tab.shape[1], len(pool["bad"])
    if n == 0 or cap == 0:
        return 0, 0, 0
    off, okf, oidx = pool["obs_off"].astype(np.int64), pool["obs_kf"], pool["obs_idx"]
    ent_ok = (okf >= 0) & (okf < n_kf) & (oidx >= 0) & (oidx < cap)
    ent_info = np.zeros(len(okf), np.int64)
    ent_info[ent_ok] = info[okf[ent_ok], oidx[ent_ok]]
    feat = np.repeat(np.arange(n), np.diff(off))
    gone = ent_ok & np.isin(okf, sorted(erased))
    lost = np.bincount(feat[gone], weights=np.where(ent_info[gone] & TWO, 2, 1), minlength=n).astype(np.int64)
    nobs0 = pool["nobs"].astype(np.int64) if "nobs" in pool else np.diff(off)
    live = nobs0 - lost
    dead = (np.bincount(feat[gone], minlength=n) > 0) & (live <= 2)
    m = int(np.clip(ntab[K], 0, cap))
    ids, own = tab[K, :m].astype(np.int64), info[K, :m].astype(np.int64)
    sel = (ids >= 0) & (ids < n)
    ids, own = ids[sel], own[sel]
    sel = (pool["bad"][ids] == 0) & ~dead[ids]
    if not monocular:
        sel &= (own & DEPTH) == 0
    ids, own = ids[sel], own[sel]
    cnt = off[ids + 1] - off[ids]
    e = np.repeat(np.arange(len(ids)), cnt)
    o = np.concatenate([np.arange(off[i], off[i + 1]) for i in ids]).astype(np.int64) if len(ids) else \
        np.zeros(0, np.int64)
    hit = ent_ok[o] & ~gone[o] & (okf[o] != K) & ((ent_info[o] & 63) <= (own[e] & 63) + 1)
    hits = np.bincount(e[hit], minlength=len(ids))
    red = (live[ids] > 3) & (hits >= need)
    return len(ids), int(red.sum()), int(dead.sum())


def np_redundant(tabs, P, K, e_pts, e_lines):
    """(nMPs, nMLs, nRedundant, the test of semantics 4) of candidate K."""
    with_lines = "ml" in tabs[0]
    n_mps, red_p, _ = np_count(tabs, 0, K, e_pts, P["monocular"], 4)
    n_mls, red_l = 0, 0
    if with_lines:
        n_mls, red_l, _ = np_count(tabs, 1, K, e_lines, P["monocular"], 3)
    if not with_lines:
        n_red, n = red_p, n_mps
    elif P["slam_mode"] == 0:
        n_red, n = red_p + red_l, n_mps + n_mls
    else:
        n_red, n = red_l, n_mls
    return n_mps, n_mls, n_red, bool(np.float32(n_red) > np.float32(P["redundant_th"]) * np.float32(n))


def np_walk(tabs, P, Q, out_cap, changed_cap):
    kf = tabs[0]
    n_kf, with_lines = len(kf["bad"]), "ml" in kf
    r = blank(out_cap, changed_cap)
    e_pts, e_lines, changed = set(), set(), []
    prev, nxt = kf["prev_kf"].copy(), kf["next_kf"].copy()
    n_in_map, err, stop = Q["n_kf_in_map"], 0, END
    cur = Q["q_slot"]
    last_id = 0
    if P["inertial"]:
        aux = cur
        for _ in range(21):
            if not 0 <= prev[aux] < n_kf:
                break
            aux = prev[aux]
        last_id = int(kf["kf_id"][aux])
    cand = kf["cand"][cur, :int(np.clip(kf["n_cand"][cur], 0, kf["cand"].shape[1]))]

    def record(pos, code, a=0, b=0, c=0):
        nonlocal err
        if pos < out_cap:
            r["outcome"][pos], r["n_mps"][pos], r["n_mls"][pos], r["n_redundant"][pos] = code, a, b, c
        else:
            err |= 1

    def cull(s, relink, with_l):
        nonlocal n_in_map
        if relink:
            p, n = prev[s], nxt[s]
            prev[n] = p
            nxt[p] = n
            prev[s] = nxt[s] = -1
        if kf["not_erase"][s]:
            changed.append((s, K_DEFERRED | (K_RELINKED if relink else 0)))
            return DEFERRED
        e_pts.add(s)
        if with_l:
            e_lines.add(s)
        n_in_map -= 1
        changed.append((s, K_POINTS | (K_LINES if with_l else 0) | (K_RELINKED if relink else 0)))
        return 0
    count = 0
    for pos, s in enumerate(cand.tolist()):
        count = pos + 1
        if not 0 <= s < n_kf or (not kf["init_kf"][s] and (kf["bad"][s] or s in e_pts)):
            record(pos, SKIP_BAD)
            continue
        if kf["init_kf"][s]:
            record(pos, SKIP_INIT)
            continue
        a, b, c, redundant = np_redundant(tabs, P, s, e_pts, e_lines)
        code, cont = KEEP, False
        if redundant and not P["inertial"]:
            code = CULLED | cull(s, False, with_lines)
        elif redundant:
            if n_in_map <= 21:
                code, cont = KEEP_FEW_KF, True
            elif int(kf["kf_id"][s]) > (int(kf["kf_id"][cur]) - 2) % 2 ** 64:
                code, cont = KEEP_RECENT, True
            elif not (0 <= prev[s] < n_kf and 0 <= nxt[s] < n_kf):
                code = KEEP_NO_CHAIN
            else:
                t = np.float32(kf["timestamp"][nxt[s]] - kf["timestamp"][prev[s]])
                if (Q["imu_init"] and int(kf["kf_id"][s]) < last_id and t < 3) or t < 0.5:
                    code = CULLED_TIME | cull(s, True, False)
                elif Q["inertial_ba2"] or not t < 3:
                    code = KEEP_TIME
                else:
                    v = -1 if Q["norm"] is None else Q["norm"][s]
                    if v < 0:
                        record(pos, NEEDS_NORM, a, b, c)
                        stop = STOP_NORM
                        break
                    code = (CULLED_NORM | cull(s, True, False)) if v else KEEP_NORM
        record(pos, code, a, b, c)
        if cont:
            continue
        if count > 20 and Q["abort_ba"]:
            stop = BREAK_ABORT
            break
        if count > 100:
            stop = BREAK_100
            break
    for i, (s, k) in enumerate(changed):
        if i < changed_cap:
            r["changed_slot"][i], r["changed_kind"][i] = s, k
        else:
            err |= 2
    r.update(n_visited=count, stop=stop, n_kf_in_map=n_in_map, err=err, n_changed=len(changed))
    return plain(r)


# ------------------------------------------------------------ crafted cases
CUR, SUP = 0, (10, 11, 12, 13, 14, 15)


def crafted_map(n_cand=4, K=16, **kw):
    m = CullMap(K, **kw)
    m.cand[CUR] = list(range(1, 1 + n_cand))
    return m


def private(m, kf, n, n_red, kind=0, octave=0, flags=0):
    """n features in kf's table, n_red of them redundant: observed by kf and 4 supports (the rest by kf and 2)."""
    for j in range(n):
        sup = [SUP[(j + i) % len(SUP)] for i in range(4 if j < n_red else 2)]
        m.add(kind, [(kf, octave, flags)] + [(s, octave) for s in sup])


def outcomes(r, n=None):
    return r["outcome"][:r["n_visited"] if n is None else n]


def case_ratios():
    m = crafted_map(4)
    for kf, (n, red) in zip((1, 2, 3, 4), ((10, 9), (10, 10), (20, 18), (11, 10))):
        private(m, kf, n, red)

    def check(r):
        # 0.9f * 10 and 0.9f * 20 round up to 9 and 18: kept, where double would cull; 10 > 9.9 culls
        assert outcomes(r) == [KEEP, CULLED, KEEP, CULLED]
        assert r["n_mps"][:4] == [10, 10, 20, 11] and r["n_redundant"][:4] == [9, 10, 18, 10]
        assert r["changed_slot"][:2] == [2, 4] and r["changed_kind"][:2] == [K_POINTS] * 2 and r["n_changed"] == 2
        assert r["stop"] == END and r["n_kf_in_map"] == 48
    return m, params(), query(), check


def case_three_others():
    """Exactly 3 other observers: the point is not redundant (nObs > thObs), the line is (nObs >= thObs).  The
    keyframe's own observation has the same octave: counted as an observer it would make the point redundant."""
    m = crafted_map(2, kl_cap=16)
    m.add(0, [(1, 0)] + [(s, 0) for s in SUP[:3]])
    m.add(1, [(2, 0)] + [(s, 0) for s in SUP[:3]])

    def check(r):
        assert outcomes(r) == [KEEP, CULLED]
        assert (r["n_mps"][:2], r["n_mls"][:2], r["n_redundant"][:2]) == ([1, 0], [0, 1], [0, 1])
        assert r["changed_kind"][0] == K_POINTS | K_LINES
    return m, params(), query(), check


def case_observations_gate():
    """Observations() exactly 3 fails `> thObs` although four others observe; 4 passes."""
    m = crafted_map(2)
    m.add(0, [(1, 0)] + [(s, 0) for s in SUP[:4]], nobs=3)
    m.add(0, [(2, 0)] + [(s, 0) for s in SUP[:4]], nobs=4)

    def check(r):
        assert outcomes(r) == [KEEP, CULLED] and r["n_redundant"][:2] == [0, 1]
    return m, params(), query(), check


def case_octaves():
    """An observer at octave s + 1 counts, at s + 2 it does not."""
    m = crafted_map(2)
    m.add(0, [(1, 2)] + [(s, 3) for s in SUP[:4]])
    m.add(0, [(2, 2)] + [(s, 3) for s in SUP[:3]] + [(SUP[3], 4)])

    def check(r):
        assert outcomes(r) == [CULLED, KEEP] and r["n_redundant"][:2] == [1, 0]
    return m, params(), query(), check


def case_order(reverse=False, not_erase=False):
    """A and B share ten points that three supports observe too: each is redundant while the other stands."""
    m = crafted_map(2)
    for _ in range(10):
        m.add(0, [(1, 0), (2, 0)] + [(s, 0) for s in SUP[:3]])
    if reverse:
        m.cand[CUR] = [2, 1]
    m.not_erase[m.cand[CUR][0]] = not_erase

    def check(r):
        first = m.cand[CUR][0]
        if not_erase:   # nothing erased: the second candidate is still redundant
            assert outcomes(r) == [CULLED | DEFERRED, CULLED] and r["n_redundant"][:2] == [10, 10]
            assert r["changed_kind"][:2] == [K_DEFERRED, K_POINTS] and r["n_kf_in_map"] == 49
        else:
            assert outcomes(r) == [CULLED, KEEP] and r["n_redundant"][:2] == [10, 0]
            assert r["changed_slot"][:1] == [first] and r["n_changed"] == 1
    return m, params(), query(), check


def case_death(nobs=3, two=False):
    """D (A, C and one support observe it) is C's one point that is not redundant: 9 of 10, kept.  A's cull
    takes D to nObs 2 -- from 3 by one, or from 4 by a stereo erase of two -- D dies and C stands at 9 of 9."""
    m = crafted_map(2)
    private(m, 1, 10, 10)
    m.add(0, [(1, 0, TWO if two else 0), (2, 0), (SUP[0], 0)], nobs=nobs)
    private(m, 2, 9, 9)
    dies = nobs - (2 if two else 1) <= 2

    def check(r):
        assert outcomes(r) == [CULLED, CULLED if dies else KEEP]
        assert r["n_mps"][:2] == [11, 9 if dies else 10] and r["n_redundant"][:2] == [10, 9]
    return m, params(), query(), check


def case_skips():
    m = crafted_map(3)
    for kf in (1, 2, 3):
        private(m, kf, 4, 4)
    m.init[1] = 1
    m.bad[2] = 1

    def check(r):
        assert outcomes(r) == [SKIP_INIT, SKIP_BAD, CULLED] and r["n_mps"][:3] == [0, 0, 4]
    return m, params(), query(), check


def case_break(n_list, bad_at, abort):
    """A long list (slots repeat: every visit is a KEEP) with the candidate at position bad_at bad."""
    m = crafted_map(0, cand_stride=112)
    for kf in range(1, 9):
        private(m, kf, 2, 0)
    m.bad[9] = 1
    m.cand[CUR] = [1 + i % 8 for i in range(n_list)]
    if bad_at is not None:
        m.cand[CUR][bad_at] = 9
    want = (22 if bad_at is not None else 21) if abort else (102 if bad_at is not None else 101)

    def check(r):
        # the skipped candidate `continue`s past the break test: the walk passes 21 / 101
        assert r["n_visited"] == want and r["stop"] == (BREAK_ABORT if abort else BREAK_100)
        assert r["outcome"][want - 1] == KEEP and r["outcome"][want] == FILL8
        if bad_at is not None:
            assert r["outcome"][bad_at] == SKIP_BAD
    return m, params(), query(abort_ba=abort), check


def case_slam(slam):
    m = crafted_map(3, kl_cap=16)
    private(m, 1, 10, 10)
    private(m, 1, 1, 0, kind=1)
    private(m, 2, 10, 0)
    private(m, 2, 1, 1, kind=1)
    private(m, 3, 10, 10)
    private(m, 3, 1, 1, kind=1)

    def check(r):
        if slam:   # points are neither counted as redundant nor in the denominator
            assert outcomes(r) == [KEEP, CULLED, CULLED] and r["n_redundant"][:3] == [0, 1, 1]
        else:
            assert outcomes(r) == [CULLED, KEEP, CULLED] and r["n_redundant"][:3] == [10, 1, 11]
        assert r["n_mps"][:3] == [10, 10, 10] and r["n_mls"][:3] == [1, 1, 1]
    return m, params(slam_mode=slam), query(), check


def case_depth(monocular):
    m = crafted_map(2, kl_cap=16)
    private(m, 1, 9, 9)
    private(m, 1, 1, 0, flags=DEPTH)
    private(m, 2, 9, 9, kind=1)
    private(m, 2, 1, 0, kind=1, flags=DEPTH)

    def check(r):
        assert outcomes(r) == ([KEEP, KEEP] if monocular else [CULLED, CULLED])
        assert [r["n_mps"][0], r["n_mls"][1]] == ([10, 10] if monocular else [9, 9])
    return m, params(monocular=monocular), query(), check


def case_odd_entries():
    """One id twice, -1 entries, ids and observer slots out of range, a count above the capacity."""
    m = crafted_map(3, kp_cap=24)
    private(m, 1, 6, 6)
    m.put(0, 1, 0, 0)           # point 0 again, without an observation: counts twice
    m.put(0, 1, -1)
    m.put(0, 1, 10 ** 6)
    m.put(0, 1, -5)
    p = m.add(0, [(2, 0)] + [(s, 0) for s in SUP[:3]])
    m.obs[0][p] += [(99, 0), (-2, 0), (SUP[4], 10 ** 6), (SUP[5], -1)]   # ignored: 3 observers are left
    m.nobs[0][p] = 9
    private(m, 3, 24, 24)
    m.ntab[0][3] = 24 + 5       # count contract: read as 24

    def check(r):
        assert outcomes(r) == [CULLED, KEEP, CULLED]
        assert r["n_mps"][:3] == [7, 1, 24] and r["n_redundant"][:3] == [7, 0, 24]
    return m, params(), query(), check


def inertial_map(n_cand, chain, dt, **kw):
    """Candidates 1..n_cand, all redundant, on the chain `chain` spaced dt; ids ascend along the chain."""
    m = crafted_map(n_cand, **kw)
    for kf in range(1, 1 + n_cand):
        private(m, kf, 4, 4)
    m.chain(chain, 0.0, dt)
    for i, s in enumerate(chain):
        m.kf_id[s] = 100 + i
    return m


def case_few_keyframes():
    m = inertial_map(3, [9, 1, 2, 3, 8, CUR], 0.1)

    def check(r):
        assert outcomes(r) == [CULLED_TIME, CULLED_TIME, KEEP_FEW_KF] and r["n_kf_in_map"] == 21
        assert r["changed_kind"][:2] == [K_POINTS | K_RELINKED] * 2
    return m, params(inertial=1), query(n_kf_in_map=23), check


def case_recent(cur_id):
    m = inertial_map(1, [9, 1, 8, CUR], 0.1)
    m.kf_id[CUR], m.kf_id[1] = cur_id, 5

    def check(r):   # 5 > 6 - 2 is recent; 1 - 2 wraps in 64 bits and the gate never fires
        assert outcomes(r) == [KEEP_RECENT if cur_id == 6 else CULLED_TIME]
    return m, params(inertial=1), query(), check


def case_last_id(n_chain):
    """last_ID after min(n_chain, 21) prev steps from the current keyframe; the candidate's id lies between the
    21st ancestor's and the chain's first."""
    K = 48
    m = CullMap(K)
    m.cand[CUR] = [1]
    for _ in range(4):
        m.add(0, [(1, 0)] + [(s, 0) for s in (40, 41, 42, 43)])
    anc = list(range(2, 2 + n_chain))           # CUR's ancestors, nearest first
    m.chain(anc[::-1] + [CUR], 0.0, 1.0)
    for i, s in enumerate(anc):
        m.kf_id[s] = 1000 - 10 * (i + 1)        # 990, 980, ...
    m.kf_id[CUR] = 1000
    m.chain([44, 1, 45], 0.0, 1.0)              # t = 2: only the id rule can cull
    m.kf_id[1] = 1000 - 10 * 25 + 5             # 755: below the 21st ancestor's 790, above the 30th's 700
    reached = 1000 - 10 * min(n_chain, 21)

    def check(r):
        assert outcomes(r) == [CULLED_TIME if 755 < reached else KEEP_TIME]
    return m, params(inertial=1), query(imu_init=1, inertial_ba2=1), check


def case_times(gap, imu_init, want):
    m = inertial_map(1, [9, 1, 8], 1.0)
    m.ts[9], m.ts[8] = 0.0, gap
    m.kf_id[CUR] = 500
    m.chain([7, CUR])
    m.kf_id[7] = 400   # last_ID: candidate 101 is below it

    def check(r):
        assert outcomes(r) == [want], (gap, imu_init)
        assert r["stop"] == (STOP_NORM if want == NEEDS_NORM else END)
    return m, params(inertial=1), query(imu_init=imu_init), check


def case_relink(not_erase=False):
    """P - A - B - N at 0, 0.2, 0.4, 0.6: A goes (t = 0.4), which lengthens B's t from 0.4 to 0.6."""
    m = inertial_map(2, [9, 1, 2, 8], 0.2)
    m.kf_id[CUR] = 500
    m.not_erase[1] = not_erase

    def check(r):
        assert outcomes(r) == [CULLED_TIME | (DEFERRED if not_erase else 0), KEEP_TIME]
        assert r["changed_kind"][:1] == [K_RELINKED | (K_DEFERRED if not_erase else K_POINTS)]
        assert r["n_kf_in_map"] == (50 if not_erase else 49) and r["n_changed"] == 1
    return m, params(inertial=1), query(inertial_ba2=1), check


def case_inertial_lines():
    """A and B share ten lines (two supports besides; nObs 4).  A's inertial cull calls SetBadFlag(), so the
    lines keep A as an observer and stay redundant for B; erased, they would fall to nObs 3."""
    m = crafted_map(2, kl_cap=32)
    m.chain([9, 1, 2, 8], 0.0, 0.2)
    m.kf_id[CUR] = 500
    for _ in range(10):
        m.add(1, [(1, 0), (2, 0), (SUP[0], 0), (SUP[1], 0)])
    private(m, 1, 2, 2)

    def check(r):
        assert outcomes(r) == [CULLED_TIME, KEEP_TIME] and r["n_redundant"][:2] == [12, 10]
        assert r["changed_kind"][0] == K_POINTS | K_RELINKED
    return m, params(inertial=1), query(inertial_ba2=1), check


def case_norm(verdicts):
    """Three candidates whose decision hinges on the norm (t = 2, ba2 clear) on one chain."""
    m = inertial_map(3, [9, 1, 2, 3, 8], 1.0)
    m.kf_id[CUR] = 500
    norm = np.full(m.K, -1, np.int32)
    norm[1:1 + len(verdicts)] = verdicts

    def check(r):   # a culled neighbour lengthens the next one's t to 3: the norm is not asked
        want, t = [], 2
        for v in list(verdicts) + [-1] * (3 - len(verdicts)):
            want.append(KEEP_TIME if t >= 3 else NEEDS_NORM if v < 0 else CULLED_NORM if v else KEEP_NORM)
            if want[-1] == NEEDS_NORM:
                break
            t = 3 if want[-1] == CULLED_NORM else 2
        assert outcomes(r) == want and r["stop"] == (STOP_NORM if want[-1] == NEEDS_NORM else END)
        assert r["n_visited"] == len(want)
    return m, params(inertial=1), query(norm=norm), check


CRAFTED = {
    "ratios": case_ratios,
    "three_others": case_three_others,
    "observations_gate": case_observations_gate,
    "octaves": case_octaves,
    "order_ab": case_order,
    "order_ba": lambda: case_order(reverse=True),
    "death_3_to_2": case_death,
    "death_4_to_2_stereo": lambda: case_death(nobs=4, two=True),
    "no_death_4_to_3": lambda: case_death(nobs=4, two=False),
    "not_erase": lambda: case_order(not_erase=True),
    "skips": case_skips,
    "break_100": lambda: case_break(105, None, 0),
    "break_100_skip_101": lambda: case_break(105, 100, 0),
    "break_abort": lambda: case_break(30, None, 1),
    "break_abort_skip_21": lambda: case_break(30, 20, 1),
    "slam_0": lambda: case_slam(0),
    "slam_1": lambda: case_slam(1),
    "depth_mono": lambda: case_depth(1),
    "depth_stereo": lambda: case_depth(0),
    "odd_entries": case_odd_entries,
    "few_keyframes": case_few_keyframes,
    "recent_cur_6": lambda: case_recent(6),
    "recent_cur_1": lambda: case_recent(1),
    "last_id_chain_5": lambda: case_last_id(5),
    "last_id_chain_30": lambda: case_last_id(30),
    "t_half": lambda: case_times(0.5, 0, NEEDS_NORM),
    "t_below_half": lambda: case_times(0.4999999, 0, CULLED_TIME),
    "t_rounds_to_half": lambda: case_times(0.49999999, 0, NEEDS_NORM),
    "t_three": lambda: case_times(3.0, 1, KEEP_TIME),
    "t_below_three": lambda: case_times(2.9999, 1, CULLED_TIME),
    "relink": case_relink,
    "relink_deferred": lambda: case_relink(not_erase=True),
    "inertial_lines": case_inertial_lines,
    "norm_stop": lambda: case_norm([]),
    "norm_0_then_stop": lambda: case_norm([0]),
    "norm_1_then_stop": lambda: case_norm([1]),
    "norm_0_1_0": lambda: case_norm([0, 1, 0]),
    "norm_1_0_1": lambda: case_norm([1, 0, 1]),
    "norm_0_0_1": lambda: case_norm([0, 0, 1]),
}


def caps_of(m):
    return (m.cand_stride or max(1, max(len(c) for c in m.cand))) + 1, 8


# -------------------------------------------------------------- random maps
def random_case(seed):
    """A small dense map: K 6-14 keyframes, tables of 32 (lines 16), a few hundred features, every mode."""
    rng = np.random.default_rng(seed)
    K = int(rng.integers(6, 15))
    lines = seed % 2 == 1
    inertial = seed % 4 >= 2
    monocular = int(rng.integers(0, 2))
    m = CullMap(K, kp_cap=32, kl_cap=16 if lines else 0)
    cur = int(rng.integers(0, K))
    m.cand[cur] = [int(s) for s in rng.permutation(K) if s != cur]
    if rng.random() < 0.2:
        m.cand[cur].insert(int(rng.integers(0, K)), int(rng.choice([-1, K + 2])))
    m.cand_stride = K + 2
    for kind, cap, n_feat in ((0, 32, int(rng.integers(60, 140))), (1, 16, int(rng.integers(30, 70)))):
        if kind and not lines:
            continue
        base = int(rng.integers(0, 3))
        for _ in range(n_feat):
            free = [s for s in range(K) if m.ntab[kind][s] < cap - 2]
            if len(free) < 2:
                break
            n_obs = min(len(free), int(rng.choice([2, 3, 4, 5, 5, 6, 6, 7, 8])))
            who = rng.choice(free, n_obs, replace=False)
            o0 = base + int(rng.integers(0, 2))
            obs = []
            for s in who:
                fl = (TWO if rng.random() < 0.25 else 0) | (DEPTH if rng.random() < 0.1 else 0)
                obs.append((int(s), o0 + int(rng.choice([0, 0, 0, 1, 1, 2, 3])), fl))
            m.add(kind, obs, nobs=None if rng.random() < 0.7 else int(n_obs + rng.integers(0, 3)),
                  bad=int(rng.random() < 0.03))
        for s in range(K):   # entries without an observation, NULLs
            for _ in range(int(rng.integers(0, 3))):
                m.put(kind, s, int(rng.choice([-1, rng.integers(0, len(m.obs[kind]))])), int(rng.integers(0, 4)))
        m.null_nobs[kind] = rng.random() < 0.2
    m.bad[rng.random(K) < 0.05] = 1
    m.bad[cur] = 0
    m.init[int(rng.integers(0, K))] = rng.random() < 0.5
    m.not_erase[rng.random(K) < 0.1] = 1
    order = [int(s) for s in rng.permutation(K)]
    cut = int(rng.integers(0, 3))
    m.chain(order[:K - cut], 0.0, 1.0)
    m.ts[:] = np.cumsum(rng.choice([0.1, 0.2, 0.3, 0.7, 1.4, 2.0], K))[np.argsort(np.argsort(
        [order.index(s) for s in range(K)]))]
    m.kf_id[:] = 20 + np.argsort(np.argsort([order.index(s) for s in range(K)]))
    if rng.random() < 0.1:
        m.kf_id[cur] = 1
    th = 0.9 if (not inertial or monocular) else 0.5
    if rng.random() < 0.5:   # more culls than the reference's threshold gives on so small a map
        th = 0.5
    P = params(np.float32(th), monocular, int(inertial), int(rng.random() < 0.25))
    norm = rng.integers(-1, 2, K).astype(np.int32) if rng.random() < 0.8 else None
    if norm is not None and rng.random() < 0.6:
        norm[norm < 0] = 1
    Q = query(cur, int(rng.integers(0, 2)), int(rng.choice([21, 22, 23, 40])), int(rng.integers(0, 2)),
              int(rng.random() < 0.3), norm)
    return m, P, Q


N_RANDOM = 240
GPU_RANDOM = tuple(range(0, N_RANDOM, 6))


@functools.lru_cache(None)
def random_ref(seed):
    m, P, Q = random_case(seed)
    extra = {}
    oc, cc = caps_of(m)
    return m, P, Q, ref_walk(m.tables(), P, Q, oc, cc, extra), extra


# ---------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("name", list(CRAFTED))
def test_crafted_case_shows_what_it_is_for(name):
    m, P, Q, check = CRAFTED[name]()
    oc, cc = caps_of(m)
    ref = ref_walk(m.tables(), P, Q, oc, cc)
    assert ref == np_walk(m.tables(), P, Q, oc, cc)
    check(ref)
    assert ref["err"] == 0


def test_order_changes_the_decision():
    """The speculative (entry-state) count differs from the final one, in either order."""
    for rev in (False, True):
        m, P, Q, _ = case_order(reverse=rev)
        tabs = m.tables()
        assert [np_redundant(tabs, P, s, set(), set())[3] for s in m.cand[CUR]] == [True, True]
        ref = ref_walk(tabs, P, Q, 3, 8)
        assert ref["changed_slot"][:ref["n_changed"]] == [m.cand[CUR][0]]


def test_float_product_against_double():
    """(float)nRed > th * (float)n with the product in float: 0.9f * 10k rounds up to 9k for every k <= 400,
    where the double product 0.9f * 10k (0.9f > 0.9) lies below it and would cull; 0.5f has no such case."""
    for k in range(1, 401):
        n, red = 10 * k, 9 * k
        assert not np.float32(red) > np.float32(0.9) * np.float32(n)
        assert float(red) > float(np.float32(0.9)) * n           # the double product would cull
        assert np.float32(0.9) * np.float32(n) == np.float32(red)
    for n in range(1, 4001):
        assert float(np.float32(0.5) * np.float32(n)) == 0.5 * n


def test_random_maps_equal_the_set_formulation():
    for seed in range(N_RANDOM):
        m, P, Q, ref, _ = random_ref(seed)
        oc, cc = caps_of(m)
        assert ref == np_walk(m.tables(), P, Q, oc, cc), seed


def test_random_maps_cover_the_sequential_part():
    culls = multi = flipped = dead = 0
    seen = set()
    for seed in range(N_RANDOM):
        m, P, Q, ref, extra = random_ref(seed)
        kinds = ref["changed_kind"][:min(ref["n_changed"], 8)]
        n = sum(1 for k in kinds if k & K_POINTS)
        culls += n
        multi += n >= 2
        dead += extra["n_dead"]
        seen.update(o & 0x7f for o in outcomes(ref))
        seen.update(DEFERRED for o in outcomes(ref) if o & DEFERRED)
        tabs = m.tables()
        th = np.float32(P["redundant_th"])
        for pos, s in enumerate(m.cand[Q["q_slot"]][:ref["n_visited"]]):
            if ref["outcome"][pos] in (SKIP_INIT, SKIP_BAD, FILL8):
                continue
            n_den = ref["n_mps"][pos] if not m.cap[1] else \
                ref["n_mps"][pos] + ref["n_mls"][pos] if P["slam_mode"] == 0 else ref["n_mls"][pos]
            final = bool(np.float32(ref["n_redundant"][pos]) > th * np.float32(n_den))
            flipped += np_redundant(tabs, P, s, set(), set())[3] != final
    assert culls >= 100 and multi >= 30 and flipped >= 30 and dead >= 20, (culls, multi, flipped, dead)
    assert seen >= set(range(1, 13)) | {DEFERRED}, sorted(seen)


def test_header_documents_the_call_and_mirror_matches():
    txt = plvi.HEADER_PATH.read_text()
    assert f"#define PLVI_CULL_MAX_CHANGED {plvi.CULL_MAX_CHANGED}\n" in txt
    sig = plvi.signatures()
    assert f"#define PLVI_CULL_SPEC {plvi.CULL_SPEC} " in txt
    assert len(sig["plvi_keyframe_culling_batch"][0]) == 12 and len(sig["plvi_keyframe_culling"][0]) == 8
    assert sig["plvi_keyframe_culling_scratch_bytes"] == ([ctypes.c_int], ctypes.c_size_t)
    assert plvi.load().plvi_keyframe_culling_scratch_bytes(3) == 256 + 16 * 3 * plvi.CULL_SPEC
    assert plvi.load().plvi_keyframe_culling_scratch_bytes(-1) == 0
    for name in ("plvi_keyframe_culling_batch", "plvi_keyframe_culling"):
        assert getattr(plvi.load(), name).argtypes == sig[name][0]
    for word in ("Precondition", "mp[K][idx] == id", "do not see each other", ":1661", ":1862", ":1713"):
        assert word in txt
    assert ctypes.sizeof(plvi.CullKeyframes) == 16 + 15 * 8 and ctypes.sizeof(plvi.CullOutputs) == 8 + 11 * 8
    assert ctypes.sizeof(plvi.CullQueries) == 7 * 8 + 8 + 3 * 8 and ctypes.sizeof(plvi.CullParams) == 16


def test_refusals_need_no_device():
    """Every refusal is decided on the host before anything is launched."""
    m, P, Q, _ = case_ratios()
    kf, mp, ml = m.tables()
    c = plvi.KeyFrameCulling(kf, mp, None, **P)
    tabs = plvi._named_tables(c.kf, c.pools)
    structs = c._structs(lambda g, k: tabs[(g, k)].ctypes.data)
    par = plvi.CullParams(0.9, 1, 0, 0)
    cell = np.zeros(64, np.int32)
    qs = plvi.CullQueries()
    for k in ("q_slot", "abort_ba", "n_kf_in_map", "imu_init", "inertial_ba2"):
        setattr(qs, k, cell.ctypes.data)
    out = plvi.CullOutputs(0, 0)
    for k in PER_Q:
        setattr(out, k, cell.ctypes.data)

    def batch(n=1, structs=structs, par=par, qs=qs, out=out, scratch=cell.ctypes.data, sb=1 << 20):
        return plvi._status("plvi_keyframe_culling_batch", n, *structs, par, qs, out, scratch, sb, None)

    def host(structs=structs, par=par, qs=qs, out=out):
        return plvi._status("plvi_keyframe_culling", *structs, par, qs, out)
    assert batch(0) == 0 and batch(-1) == E_BADARG and batch(65536) == E_CAPACITY
    assert batch(scratch=None) == E_BADARG and batch(sb=256 + 16 * plvi.CULL_SPEC - 1) == E_BADARG
    for call in (batch, host):
        assert call(par=None) == E_BADARG and call(qs=None) == E_BADARG and call(out=None) == E_BADARG
        assert call(structs=[None] + structs[1:]) == E_BADARG and call(structs=[structs[0], None] + structs[2:]) \
            == E_BADARG
        no_idx = list(structs)
        no_idx[2] = plvi.CullFeatures()
        assert call(structs=no_idx) == E_BADARG                       # obs_idx missing
        neg = plvi.CullKeyframes.from_buffer_copy(structs[0])
        neg.kp_cap = -1
        assert call(structs=[neg] + structs[1:]) == E_BADARG
        no_chain = plvi.CullKeyframes.from_buffer_copy(structs[0])
        no_chain.timestamp = None
        assert call(structs=[no_chain] + structs[1:], par=plvi.CullParams(0.9, 1, 1, 0)) == E_BADARG
        part = plvi.CullQueries.from_buffer_copy(qs)
        part.start = cell.ctypes.data
        assert call(qs=part) == E_BADARG                              # resume fields given in part
        no_q = plvi.CullQueries.from_buffer_copy(qs)
        no_q.imu_init = None
        assert call(qs=no_q) == E_BADARG
        assert call(out=plvi.CullOutputs(4, 0, *[cell.ctypes.data] * 4)) == E_BADARG   # out_cap without its tables
        assert call(out=plvi.CullOutputs(0, 4, *[cell.ctypes.data] * 4 + [None] * 4 + [cell.ctypes.data])) == E_BADARG


# ---------------------------------------------------------------- GPU tests
def gpu_walk(m, P, Q, out_cap, changed_cap, host=False, max_calls=8):
    """The call chain of a caller: a walk that stops for the norm is resumed with the verdict of Q["norm"]."""
    kf, mp, ml = m.tables()
    c = plvi.KeyFrameCulling(kf, mp, ml, **P)
    run = c.cull if host else c.cull_batch
    q = {k: Q[k] for k in ("q_slot", "abort_ba", "n_kf_in_map", "imu_init", "inertial_ba2")}
    r = run(out_cap=out_cap, changed_cap=changed_cap, **q)
    calls = 1
    while int(r["stop"][0]) == STOP_NORM and Q["norm"] is not None and calls < max_calls:
        pos = int(r["n_visited"][0]) - 1
        v = int(Q["norm"][kf["cand"][Q["q_slot"], pos]])
        if v < 0:
            break
        assert r["past"]["stop"] == FILL
        r = run(out_cap=out_cap, changed_cap=changed_cap, prev=r, verdict=v, **q)
        calls += 1
    assert all(np.all(np.asarray(v) == (FILL8 if k == "outcome" else FILL)) for k, v in r["past"].items()), r["past"]
    return plain({k: r[k][0] for k in PER_Q + PER_C + PER_CH}), calls


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CRAFTED))
def test_gpu_crafted(plvi_lib, name):
    m, P, Q, _ = CRAFTED[name]()
    oc, cc = caps_of(m)
    got, _ = gpu_walk(m, P, Q, oc, cc)
    assert got == ref_walk(m.tables(), P, Q, oc, cc)


@pytest.mark.gpu
def test_gpu_random_maps(plvi_lib):
    resumed = 0
    for seed in GPU_RANDOM:
        m, P, Q, ref, _ = random_ref(seed)
        oc, cc = caps_of(m)
        got, calls = gpu_walk(m, P, Q, oc, cc)
        assert got == ref, seed
        resumed += calls > 1
    assert resumed >= 3


@pytest.mark.gpu
def test_gpu_host_form(plvi_lib):
    for name in ("ratios", "slam_0", "norm_1_0_1", "relink_deferred", "odd_entries"):
        m, P, Q, _ = CRAFTED[name]()
        oc, cc = caps_of(m)
        got, _ = gpu_walk(m, P, Q, oc, cc, host=True)
        assert got == ref_walk(m.tables(), P, Q, oc, cc), name


@pytest.mark.gpu
def test_gpu_mixed_batch(plvi_lib):
    """One call: a query without candidates, lists above out_cap and changed_cap (err bits, nothing written
    past either), a query out of range, and a resumed query beside a fresh one on the same map."""
    m = inertial_map(3, [9, 1, 2, 3, 8], 1.0)
    m.kf_id[CUR] = 500
    m.cand[4] = []
    m.cand[5] = [3, 2, 1]
    m.kf_id[5] = 600
    kf, mp, ml = m.tables()
    P = params(inertial=1)
    c = plvi.KeyFrameCulling(kf, mp, ml, **P)
    norm = np.full(m.K, -1, np.int32)
    norm[1] = 1
    first = c.cull_batch([CUR], n_kf_in_map=50, out_cap=2, changed_cap=0)
    assert first["stop"].tolist() == [STOP_NORM] and first["n_visited"].tolist() == [1]
    # queries: resumed CUR (verdict 1) | no candidates | fresh 5 | slot out of range
    prev = {k: np.concatenate([first[k]] + [np.full_like(first[k], 0 if k in PER_Q else FILL8 if k == "outcome"
                                                        else FILL)] * 3) for k in PER_Q + PER_C + PER_CH}
    prev["n_visited"][1:] = 1   # start = n_visited - 1 = 0 for the fresh ones
    r = c.cull_batch([CUR, 4, 5, 99], n_kf_in_map=50, prev=prev, verdict=[1, -1, -1, -1], out_cap=2, changed_cap=0)
    want0 = ref_walk(m.tables(), P, query(CUR, norm=norm), 2, 0)
    # culled by the verdict, the next kept by its lengthened t, the third asks for the norm at position 2 >= out_cap
    assert want0["err"] == 3 and want0["n_changed"] == 1 and want0["n_visited"] == 3 and want0["stop"] == STOP_NORM
    assert plain({k: r[k][0] for k in PER_Q + PER_C + PER_CH}) == want0
    assert [int(r[k][1]) for k in PER_Q] == [0, END, 50, 0, 0]
    assert r["outcome"][1].tolist() == [FILL8] * 2
    want2 = ref_walk(m.tables(), P, query(5), 2, 0)
    assert want2["stop"] == STOP_NORM
    assert plain({k: r[k][2] for k in PER_Q + PER_C + PER_CH}) == want2
    assert (r["err"][3], r["n_visited"][3], r["n_changed"][3]) == (plvi.CULL_ERR_QUERY, 0, 0)
    assert all(np.all(np.asarray(v) == (FILL8 if k == "outcome" else FILL)) for k, v in r["past"].items())


@pytest.mark.gpu
def test_gpu_overlay_is_independent_of_kf_cap(plvi_lib):
    """The erased set is a list behind a 2048-bit filter keyed by slot % 2048: slots 2048 apart share a bit and
    must still be told apart, and a kf_cap far above the filter needs no other path."""
    K = 2 * 2048 + 16
    m = CullMap(K, kp_cap=16)
    a, b, c = 5, 5 + 2048, 5 + 4096
    sup = (100, 101, 102)
    m.cand[CUR] = [a, b, c]
    for _ in range(4):                     # a and b share: a's cull takes b's redundancy
        m.add(0, [(a, 0), (b, 0)] + [(s, 0) for s in sup])
    for _ in range(4):                     # c's points are observed by b (same filter bit as a), not by a
        m.add(0, [(c, 0), (b, 0)] + [(s, 0) for s in sup] + [(103, 0)])
    oc, cc = caps_of(m)
    P, Q = params(), query()
    ref = ref_walk(m.tables(), P, Q, oc, cc)
    assert outcomes(ref) == [CULLED, KEEP, CULLED]
    assert gpu_walk(m, P, Q, oc, cc)[0] == ref


@pytest.mark.gpu
def test_gpu_graph_capture_replayed_once(plvi_lib):
    m, P, Q, _ = case_death()
    oc, cc = caps_of(m)
    kf, mp, ml = m.tables()
    c = plvi.KeyFrameCulling(kf, mp, ml, **P)
    step, fetch = c.cull_batch([CUR], n_kf_in_map=50, out_cap=oc, changed_cap=cc, run=False)
    st = ctypes.c_void_p()
    assert plvi_lib.plvi_stream_create(ctypes.byref(st)) == 0
    rcs = []
    graph = plvi.StepGraph(lambda s: rcs.append(step(s)), st.value)
    assert rcs == [0]
    assert (fetch()["n_visited"] == FILL).all()   # captured, not run
    graph.launch()
    assert plvi_lib.plvi_stream_synchronize(st) == 0
    r = fetch()
    assert plain({k: r[k][0] for k in PER_Q + PER_C + PER_CH}) == ref_walk(m.tables(), P, Q, oc, cc)


@pytest.mark.gpu
def test_gpu_walks_the_graphs_rows_in_place(plvi_lib):
    """plvi_covis_resort_batch -> plvi_covis_rows -> the walk, on the graph's own device tables."""
    m, P, Q, _ = case_order()
    kf, mp, ml = m.tables()
    K = m.K
    g = plvi.Covisibility(K, 8)
    ck = dict(bad=kf["bad"], order=np.arange(K, dtype=np.int32), mp=kf["mp"], nmp=kf["nmp"])
    g.set_tables(ck, {k: mp[k] for k in ("bad", "obs_off", "obs_kf")})
    assert g.update_batch([1])["rc"] == 0      # keyframe 1's list: 2 and the three supports, all at weight 10
    assert g.resort([1]) == 0
    ord_kf, _, ord_n = g.rows()
    lst = g.download(1)
    row = lst["ord_kf"][:lst["n_ord"]].tolist()
    assert 2 in row and len(row) == 4
    m.cand[1] = row
    c = plvi.KeyFrameCulling(kf, mp, ml, rows=(ord_kf, ord_n, 8), **P)
    r = c.cull_batch([1], n_kf_in_map=50, out_cap=8, changed_cap=8)
    assert plain({k: r[k][0] for k in PER_Q + PER_C + PER_CH}) == ref_walk(m.tables(), P, query(1), 8, 8)
    assert CULLED in r["outcome"][0].tolist()
    g.close()


@pytest.mark.gpu
def test_gpu_refusals(plvi_lib):
    m, P, Q, _ = case_ratios()
    kf, mp, ml = m.tables()
    c = plvi.KeyFrameCulling(kf, mp, None, **P)
    dev = c.upload()
    structs = c._structs(lambda g, k: dev[(g, k)].ptr)
    par = plvi.CullParams(0.9, 1, 0, 0)
    buf = plvi.DeviceBuffer(4096)
    qs = plvi.CullQueries()
    for k in ("q_slot", "abort_ba", "n_kf_in_map", "imu_init", "inertial_ba2"):
        setattr(qs, k, buf.ptr)
    out = plvi.CullOutputs(0, 0)
    for k in PER_Q:
        setattr(out, k, buf.ptr)

    sb = plvi_lib.plvi_keyframe_culling_scratch_bytes(1)
    scratch = plvi.DeviceBuffer(sb)

    def call(n=1, structs=structs, par=par, qs=qs, out=out, sb=sb):
        return plvi._status("plvi_keyframe_culling_batch", n, *structs, par, qs, out, scratch.ptr, sb, None)
    assert call(0) == 0 and call(-1) == E_BADARG and call(65536) == E_CAPACITY
    assert call(sb=sb - 1) == E_BADARG                            # scratch too small
    no_idx = list(structs)
    no_idx[2] = plvi.CullFeatures()
    assert call(structs=no_idx) == E_BADARG                       # obs_idx missing
    assert call(par=plvi.CullParams(0.9, 1, 1, 0)) == 0           # inertial with its four tables
    no_chain = plvi.CullKeyframes.from_buffer_copy(structs[0])
    no_chain.timestamp = None
    assert call(structs=[no_chain] + list(structs[1:]), par=plvi.CullParams(0.9, 1, 1, 0)) == E_BADARG
    part = plvi.CullQueries.from_buffer_copy(qs)
    part.start = buf.ptr
    assert call(qs=part) == E_BADARG                              # resume fields given in part
    assert call(out=plvi.CullOutputs(4, 0, *[buf.ptr] * 4)) == E_BADARG   # out_cap without its tables
    plvi._sync()
