"""The local-BA window on the device (csrc/ba_window.hip, plvi_ba_window[_batch]): the set-up and the edge index
logic of Optimizer::LocalBundleAdjustment(pKF, pbStopFlag, pMap, num_fixedKF), LocalBundleAdjustmentOnlyLines (and
its two Angle variants) and LocalInertialBA (src/Optimizer.cc:4851-4960 / :5048-5168, :6181-6233 / :6291-6337,
:9185-9307 / :9521-9640).

Expected values come from tests/native/ba_window_ref.cpp, a sequential host restatement in the reference's own shape
(objects with mnBALocalForKF / mnBAFixedForKF members, std::list and list::remove, std::map observations, the loop
bodies as the reference's text).  The CPU part pins it against np_window below, an independent restatement in the
formulation the kernel uses -- no stamps, "the smallest traversal position wins" by np.unique(return_index) -- on
every crafted case and on the random maps, asserts what each crafted case is there to show, and asserts the coverage
of the random maps.  The gpu part demands exact equality with the restatement for every output of both forms, with
sentinel-filled tables.

Every crafted case of a mode lives in ONE map (a case takes fresh keyframe slots and fresh feature ids, and a query
sees only what its row, tables and observation lists reach), so one batch per mode runs them all; the random maps of
a mode are composed the same way."""
import ctypes
import functools
import pathlib
import subprocess

import numpy as np
import pytest

import plvi

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "ba_window_ref.cpp"
BUILD = ROOT / "tests" / "native" / "_build"
FILL, FILL8 = -7, -7 & 0x7f
POINTS, LINES, INERTIAL = range(3)
MONO, STEREO, LINE = range(3)
E_LKF, E_FKF, E_FEAT, E_EDGE, E_UNDEF, E_QUERY = 1, 2, 4, 8, 16, 32
SCALARS = ("n_local_kf", "n_fixed_kf", "num_fixed", "init_in_local", "non_fixed", "n_local_feat", "n_mono",
           "n_stereo", "n_line", "err")
LISTS = {"local_kf": "lkf_cap", "fixed_kf": "fkf_cap", "local_feat": "feat_cap", "edge_feat": "edge_cap",
         "edge_kf": "edge_cap", "edge_idx": "edge_cap", "edge_cam": "edge_cap", "edge_kind": "edge_cap"}
CAPS = ("lkf_cap", "fkf_cap", "feat_cap", "edge_cap")
TWO = 0x80
OUT = 1 << 20   # a keyframe slot outside every map


# ------------------------------------------------------------------ the map
class BAMap:
    """Keyframe tables and one pool (MapPoints, or MapLines with lines=True), grown case by case.  Observation
    lists are emitted in slot order (they are std::map keys in the reference)."""

    def __init__(self, cap, lines=False):
        self.cap, self.lines = cap, lines
        self.tab, self.info = [], []
        self.bad, self.init, self.kf_id, self.prev, self.kf_map, self.cand = [], [], [], [], [], []
        self.obs, self.fbad, self.fmap = [], [], []

    @property
    def K(self):
        return len(self.bad)

    def kf(self, bad=0, map_id=0, kf_id=None, init=0, prev=-1):
        s = self.K
        self.tab.append([])
        self.info.append([])
        self.bad.append(bad)
        self.init.append(init)
        self.kf_id.append(100000 - s if kf_id is None else kf_id)   # a later keyframe has a lower id
        self.prev.append(prev)
        self.kf_map.append(map_id)
        self.cand.append([])
        return s

    def put(self, kf, fid, flags=0):
        assert len(self.tab[kf]) < self.cap, "table full"
        self.tab[kf].append(fid)
        self.info[kf].append(flags)
        return len(self.tab[kf]) - 1

    def feat(self, observers, bad=0, map_id=0):
        """A feature observed by `observers`: kf, (kf, flags) or (kf, flags, idx) -- idx given = no table entry."""
        fid = len(self.obs)
        lst = []
        for o in observers:
            o = (o, 0) if isinstance(o, int) else o
            if len(o) > 2:
                lst.append((o[0], o[2]))
            elif 0 <= o[0] < self.K:
                lst.append((o[0], self.put(o[0], fid, o[1])))
            else:
                lst.append((o[0], 0))
        self.obs.append(lst)
        self.fbad.append(bad)
        self.fmap.append(map_id)
        return fid

    def tables(self, stride=None, pad_kf=0):
        """(keyframes, pool, kf_map_id) as plvi.LocalBAWindow takes them; pad_kf empty (bad) slots are appended."""
        K = self.K + pad_kf
        stride = stride or max(1, max(len(c) for c in self.cand))
        tab = np.full((K, self.cap), -1, np.int32)
        info = np.zeros((K, self.cap), np.uint8)
        ntab = np.zeros(K, np.int32)
        cand = np.full((K, stride), -1, np.int32)
        n_cand = np.zeros(K, np.int32)
        for s in range(self.K):
            ntab[s] = len(self.tab[s])
            tab[s, :ntab[s]] = self.tab[s]
            info[s, :ntab[s]] = self.info[s]
            n_cand[s] = len(self.cand[s])
            cand[s, :n_cand[s]] = self.cand[s]
        pad = lambda a, v, dt: np.array(list(a) + [v] * pad_kf, dt)  # noqa: E731
        kf = dict(bad=pad(self.bad, 1, np.uint8), init_kf=pad(self.init, 0, np.uint8), cand=cand, n_cand=n_cand,
                  kf_id=pad(self.kf_id, 0, np.uint32), prev_kf=pad(self.prev, -1, np.int32))
        if self.lines:
            kf.update(ml=tab, nml=ntab)
        else:
            kf.update(mp=tab, nmp=ntab, kp_info=info)
        off = np.zeros(len(self.obs) + 1, np.int32)
        off[1:] = np.cumsum([len(o) for o in self.obs])
        flat = [e for o in self.obs for e in sorted(o, key=lambda e: e[0])]
        pool = dict(bad=np.array(self.fbad, np.uint8), obs_off=off,
                    obs_kf=np.array([e[0] for e in flat], np.int32).reshape(-1),
                    obs_idx=np.array([e[1] for e in flat], np.int32).reshape(-1),
                    map_id=np.array(self.fmap, np.int32))
        return kf, pool, pad(self.kf_map, 0, np.int32)


def window(tabs, mode, max_opt=10):
    kf, pool, kf_map = tabs
    return plvi.LocalBAWindow(kf, None if mode == LINES else pool, pool if mode == LINES else None, mode=mode,
                              max_opt=max_opt, kf_map_id=kf_map)


def big_caps(tabs):
    kf, pool, _ = tabs
    return dict(lkf_cap=kf["cand"].shape[1] + 70, fkf_cap=len(kf["bad"]) + 2, feat_cap=max(len(pool["bad"]), 1),
                edge_cap=max(len(pool["obs_kf"]), 1))


def blank(caps):
    r = {k: FILL for k in SCALARS}
    r.update({k: np.full(max(caps[c], 1), FILL8 if k == "edge_kind" else FILL,
                         np.uint8 if k == "edge_kind" else np.int32) for k, c in LISTS.items()})
    return r


def plain(r, q=None):
    """One query's outputs as plain Python values."""
    pick = (lambda a: a) if q is None else (lambda a: a[q])  # noqa: E731
    return {k: (pick(r[k]).tolist() if isinstance(pick(r[k]), np.ndarray) else int(pick(r[k])))
            for k in SCALARS + tuple(LISTS)}


# ------------------------------------------------------- the restatement (C++)
class RefTables(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("kf_cap", "kp_cap", "kl_cap", "cand_stride")] + \
               [(k, ctypes.c_void_p) for k in ("bad", "init_kf", "mp", "nmp", "ml", "nml", "kp_info", "cand", "n_cand",
                                               "kf_id", "prev_kf", "kf_map_id")] + \
               [("mp_n", ctypes.c_int)] + \
               [(k, ctypes.c_void_p) for k in ("mp_bad", "mp_obs_off", "mp_obs_kf", "mp_obs_idx", "mp_map_id")] + \
               [("ml_n", ctypes.c_int)] + \
               [(k, ctypes.c_void_p) for k in ("ml_bad", "ml_obs_off", "ml_obs_kf", "ml_obs_idx", "ml_map_id")] + \
               [("mode", ctypes.c_int), ("max_opt", ctypes.c_int)]


class RefQuery(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("q_slot", "n_kf_in_map") + CAPS] + \
               [(k, ctypes.c_void_p) for k in ("local_kf", "n_local_kf", "fixed_kf", "n_fixed_kf", "num_fixed",
                                               "init_in_local", "non_fixed", "local_feat", "n_local_feat", "edge_feat",
                                               "edge_kf", "edge_idx", "edge_cam", "edge_kind", "n_mono", "n_stereo",
                                               "n_line", "err", "seconds")]


@functools.lru_cache(None)
def ref_lib():
    so = BUILD / "libba_window_ref.so"
    if not so.exists() or so.stat().st_mtime < SRC.stat().st_mtime:
        so.parent.mkdir(parents=True, exist_ok=True)
        # -Wno-sign-compare: `pKFi->mnId < lowerId` stands as the reference writes it
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-sign-compare", "-shared", "-fPIC", "-o",
                        str(so), str(SRC)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.ba_window_ref_run.argtypes, lib.ba_window_ref_run.restype = [ctypes.c_void_p, ctypes.c_void_p], None
    return lib


_KF_DT = dict(bad=np.uint8, init_kf=np.uint8, mp=np.int32, nmp=np.int32, ml=np.int32, nml=np.int32, kp_info=np.uint8,
              cand=np.int32, n_cand=np.int32, kf_id=np.uint32, prev_kf=np.int32)


def ref_tables(tabs, mode, max_opt):
    kf, pool, kf_map = tabs
    shape = lambda k: kf[k].shape[1] if k in kf else 0  # noqa: E731
    t = RefTables(len(kf["bad"]), shape("mp"), shape("ml"), shape("cand"))
    keep = []

    def ptr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return a.ctypes.data
    for k, dt in _KF_DT.items():
        setattr(t, k, ptr(kf.get(k), dt))
    t.kf_map_id = ptr(kf_map, np.int32)
    g = "ml" if mode == LINES else "mp"
    setattr(t, g + "_n", len(pool["bad"]))
    for k, dt in plvi._BA_POOL.items():
        setattr(t, f"{g}_{k}", ptr(pool.get(k), dt))
    t.mode, t.max_opt = mode, max_opt
    return t, keep


def ref_window(tabs, mode, q_slot, n_kf_in_map=50, max_opt=10, caps=None, seconds=None):
    caps = caps or big_caps(tabs)
    t, keep = ref_tables(tabs, mode, max_opt)
    r = blank(caps)
    scal = {k: np.full(1, FILL, np.int32) for k in SCALARS}
    sec = np.zeros(1, np.float64)
    q = RefQuery(q_slot, n_kf_in_map, *(caps[c] for c in CAPS))
    for k in SCALARS:
        setattr(q, k, scal[k].ctypes.data)
    for k in LISTS:
        setattr(q, k, r[k].ctypes.data)
    q.seconds = sec.ctypes.data
    ref_lib().ba_window_ref_run(ctypes.byref(t), ctypes.byref(q))
    r.update({k: int(scal[k][0]) for k in SCALARS})
    if seconds is not None:
        seconds.append(float(sec[0]))
    return plain(r)


# ------------------------------------- the position formulation (numpy)
def first_seen(a):
    """The distinct values of `a` in the order of their first occurrence."""
    a = np.asarray(a, np.int64)
    _, idx = np.unique(a, return_index=True)
    return a[np.sort(idx)]


def np_window(tabs, mode, q_slot, n_kf_in_map=50, max_opt=10, caps=None):
    kf, pool, kf_map = tabs
    caps = caps or big_caps(tabs)
    r = blank(caps)
    K = len(kf["bad"])
    if not 0 <= q_slot < K:
        r.update({k: 0 for k in SCALARS})
        r.update(non_fixed=1, err=E_QUERY)
        return plain(r)
    tab, ntab = (kf["ml"], kf["nml"]) if mode == LINES else (kf["mp"], kf["nmp"])
    cap, n = tab.shape[1], len(pool["bad"])
    bad, M = kf["bad"].astype(bool), int(kf_map[q_slot])
    in_map = np.asarray(kf_map) == M
    off, okf, oidx = pool["obs_off"].astype(np.int64), pool["obs_kf"].astype(np.int64), pool["obs_idx"]
    err = 0

    def features(kfs, map_test):
        ids = np.concatenate([tab[s, :int(np.clip(ntab[s], 0, cap))] for s in kfs] + [np.zeros(0, np.int32)])
        ids = ids[(ids >= 0) & (ids < n)].astype(np.int64)
        ids = ids[pool["bad"][ids] == 0]
        if map_test:
            ids = ids[pool["map_id"][ids] == M]
        return first_seen(ids)

    def observations(feats):
        """(feature position, observation offset) of every observation of the local features, in traversal order."""
        cnt = off[feats + 1] - off[feats]
        j = np.repeat(np.arange(len(feats)), cnt)
        o = np.concatenate([np.arange(off[f], off[f + 1]) for f in feats] + [np.zeros(0, np.int64)]).astype(np.int64)
        ok = (okf[o] >= 0) & (okf[o] < K)
        return j[ok], o[ok]

    if mode != INERTIAL:
        row = kf["cand"][q_slot, :int(np.clip(kf["n_cand"][q_slot], 0, kf["cand"].shape[1]))].astype(np.int64)
        row = row[(row >= 0) & (row < K)]
        stamped = np.zeros(K, bool)
        stamped[row] = True
        stamped[q_slot] = True
        listed = row[~bad[row] & (in_map[row] if mode == POINTS else True)]
        local = [q_slot] + listed.tolist()
        feats = features(first_seen(local).tolist(), True)
        init = int(any(kf["init_kf"][s] for s in local))
        j, o = observations(feats)
        sel = ~stamped[okf[o]]
        fixed = first_seen(okf[o][sel])
        fixed = fixed[~bad[fixed] & in_map[fixed]].tolist()
        num_fixed = len(fixed) + (init if mode == POINTS else 0)
        if mode == POINTS and num_fixed < 2:
            ext = lambda v: int(np.int32(np.uint32(v & 0xffffffff))) & 0xffffffffffffffff  # noqa: E731 (int)x, then 64 bits
            lower = second = ext(int(kf["kf_id"][q_slot]))
            p_lower = p_second = None
            for s in local:
                if s == q_slot or kf["init_kf"][s]:
                    continue
                i = int(kf["kf_id"][s])
                if i < lower:
                    lower, p_lower = ext(i), s
                elif i < second:
                    second, p_second = ext(i), s
            moves = [p_lower] + ([p_second] if num_fixed + 1 < 2 else [])
            num_fixed += len(moves)
            for m in moves:
                if m is None:
                    err |= E_UNDEF
                else:
                    fixed.append(m)
                    local = [s for s in local if s != m]
        stamp_test = None
    else:
        nd = min(n_kf_in_map - 2, max_opt)
        local = [q_slot]
        prev = lambda s: int(kf["prev_kf"][s]) if 0 <= kf["prev_kf"][s] < K else -1  # noqa: E731
        while len(local) < nd and prev(local[-1]) >= 0:
            local.append(prev(local[-1]))
        feats = features(first_seen(local).tolist(), False)
        init = int(any(kf["init_kf"][s] for s in local))
        taken = np.zeros(K, bool)
        taken[local] = True
        if prev(local[-1]) >= 0:
            fixed = [prev(local[-1])]
        else:
            fixed = [local.pop()]
        taken[fixed[0]] = True
        for f in feats:
            ks = okf[off[f]:off[f + 1]]
            ks = ks[(ks >= 0) & (ks < K)]
            ks = ks[~taken[ks] & ~bad[ks]]
            if len(ks):
                taken[ks[0]] = True
                fixed.append(int(ks[0]))
            if len(fixed) >= 200:
                break
        num_fixed = len(fixed)
        j, o = observations(feats)
        stamp_test = taken
    e_ok = ~bad[okf[o]] & in_map[okf[o]] & (oidx[o] >= 0) & (oidx[o] < cap)
    if stamp_test is not None:
        e_ok &= stamp_test[okf[o]]
    j, o = j[e_ok], o[e_ok]
    cam = {}
    for pos, s in enumerate(local + fixed):
        cam.setdefault(s, pos)
    if mode == LINES:
        kind = np.full(len(o), LINE)
    else:
        kind = np.where(kf["kp_info"][okf[o], oidx[o]] & TWO, STEREO, MONO)
    lists = dict(local_kf=local, fixed_kf=fixed, local_feat=feats.tolist(), edge_feat=j.tolist(),
                 edge_kf=okf[o].tolist(), edge_idx=oidx[o].tolist(), edge_cam=[cam.get(int(s), -1) for s in okf[o]],
                 edge_kind=kind.tolist())
    for k, c in LISTS.items():
        m = min(len(lists[k]), caps[c])
        r[k][:m] = lists[k][:m]
    for k, bit in (("local_kf", E_LKF), ("fixed_kf", E_FKF), ("local_feat", E_FEAT), ("edge_feat", E_EDGE)):
        if len(lists[k]) > caps[LISTS[k]]:
            err |= bit
    r.update(n_local_kf=len(local), n_fixed_kf=len(fixed), num_fixed=num_fixed, init_in_local=init,
             non_fixed=int(not fixed), n_local_feat=len(feats), n_mono=int((kind == MONO).sum()),
             n_stereo=int((kind == STEREO).sum()), n_line=int((kind == LINE).sum()), err=err)
    return plain(r)


def lists_of(r):
    """The lists of a plain result cut to their lengths (the caps were large), edges as tuples."""
    ne = r["n_mono"] + r["n_stereo"] + r["n_line"]
    return dict(local=r["local_kf"][:r["n_local_kf"]], fixed=r["fixed_kf"][:r["n_fixed_kf"]],
                feats=r["local_feat"][:r["n_local_feat"]],
                edges=list(zip(*(r[k][:ne] for k in ("edge_feat", "edge_kf", "edge_idx", "edge_cam", "edge_kind")))))


# ---------------------------------------------------------- crafted cases
# A case adds its keyframes and features to the mode's map and returns (q_slot, n_kf_in_map, check); check(res)
# asserts on lists_of(res) + the scalars what the case is there to show.
def visual_cases(m, mode):
    cases = {}

    def case(fn):
        cases[fn.__name__] = fn()
        return fn

    @case
    def bad_and_other_map_covisibles():
        q, a, b, c, d, d2 = m.kf(), m.kf(), m.kf(bad=1), m.kf(map_id=1), m.kf(), m.kf()
        x, y = m.kf(bad=1), m.kf(map_id=1)      # observers outside the row
        m.cand[q] = [a, b, c]
        f = [m.feat([q, a]), m.feat([q, b, x]), m.feat([q, c, y]), m.feat([q, d]), m.feat([q, d2])]

        def check(r, L):
            assert L["local"] == ([q, a] if mode == POINTS else [q, a, c])
            assert L["fixed"] == [d, d2]
            assert not {b, c, x, y} & set(L["fixed"]), "stamped local / bad / other map: never fixed"
            assert L["feats"] == f
            assert {e[1] for e in L["edges"]} == {q, a, d, d2}
            assert all(e[3] >= 0 for e in L["edges"])
        return q, 50, check

    @case
    def id_twice_in_a_table_and_in_a_later_keyframe():
        q, a, d, e = m.kf(), m.kf(), m.kf(), m.kf()
        m.cand[q] = [a]
        g = m.feat([a, d])
        f = m.feat([q, a, e])
        m.put(q, f)

        def check(r, L):
            assert L["feats"] == [f, g]
            assert L["fixed"] == [e, d], "in the order of the local features, not of the slots"
        return q, 50, check

    @case
    def bad_and_other_map_features():
        q, d, e = m.kf(), m.kf(), m.kf()
        fb, fo, f = m.feat([q, d], bad=1), m.feat([q, d], map_id=1), m.feat([q, e])
        m.put(q, -1)
        m.put(q, OUT)

        def check(r, L):
            assert L["feats"] == [f] and d not in L["fixed"] and e in L["fixed"]
        return q, 50, check

    @case
    def observers_bad_out_of_range_and_idx_out_of_range():
        q, a, x, d, e = m.kf(), m.kf(), m.kf(bad=1), m.kf(), m.kf()
        m.cand[q] = [a]
        f = m.feat([q, x, (OUT, 0), (-1, 0), d, (e, 0, m.cap), (a, 0, -1)])

        def check(r, L):
            assert L["feats"] == [f]
            assert L["fixed"] == [d, e], "x is stamped and unlisted; e is a fixed camera without an edge"
            assert [(e_[1], e_[2]) for e_ in L["edges"]] == [(q, 0), (d, 0)]
        return q, 50, check

    @case
    def q_in_its_own_row():
        q, a, d, e = m.kf(), m.kf(), m.kf(), m.kf()
        m.cand[q] = [a, q]
        f = m.feat([q, a, d, e])

        def check(r, L):
            assert L["local"] == [q, a, q] and L["feats"] == [f] and L["fixed"] == [d, e]
            assert [e_[3] for e_ in L["edges"]] == [0, 1, 3, 4], "the first position of q; fixed after 3 locals"
        return q, 50, check

    @case
    def every_list_nonempty():    # the case that runs one over every capacity
        q, a, d, e = m.kf(), m.kf(), m.kf(), m.kf()
        m.cand[q] = [a]
        m.feat([q, a, d])
        m.feat([a, (e, TWO)])

        def check(r, L):
            assert len(L["local"]) == 2 and len(L["fixed"]) == 2 and len(L["feats"]) == 2 and len(L["edges"]) == 5
        return q, 50, check

    if mode == LINES:
        return cases

    @case
    def mono_and_stereo_interleaved():
        q, a, d = m.kf(), m.kf(), m.kf()
        m.cand[q] = [a]
        m.feat([(q, TWO), a, (d, TWO)])
        m.feat([q, (a, TWO), d])

        def check(r, L):
            assert [e[4] for e in L["edges"]] == [STEREO, MONO, STEREO, MONO, STEREO, MONO]
            assert (r["n_mono"], r["n_stereo"], r["n_line"]) == (3, 3, 0)
        return q, 50, check

    @case
    def init_keyframe_no_fixed_camera():
        q, a, b = m.kf(kf_id=90), m.kf(kf_id=10, init=1), m.kf(kf_id=50)
        m.cand[q] = [a, b]
        m.feat([q, a, b])

        def check(r, L):
            assert r["init_in_local"] == 1 and r["num_fixed"] == 2 and r["err"] == 0
            assert L["local"] == [q, a] and L["fixed"] == [b], "one move; the initial keyframe is never a candidate"
        return q, 50, check

    @case
    def init_keyframe_one_fixed_camera():
        q, a, b, d = m.kf(kf_id=90), m.kf(kf_id=10, init=1), m.kf(kf_id=50), m.kf()
        m.cand[q] = [a, b]
        m.feat([q, a, b, d])

        def check(r, L):
            assert r["init_in_local"] == 1 and r["num_fixed"] == 2
            assert L["local"] == [q, a, b] and L["fixed"] == [d], "1 + 1: nothing moves"
        return q, 50, check

    @case
    def two_moves():
        q, a, b, c = m.kf(kf_id=90), m.kf(kf_id=30), m.kf(kf_id=20), m.kf(kf_id=25)
        m.cand[q] = [a, b, c]
        m.feat([q, a, b, c])

        def check(r, L):
            assert r["num_fixed"] == 2 and L["fixed"] == [b, c] and L["local"] == [q, a]
            assert sorted(e[3] for e in L["edges"]) == [0, 1, 2, 3]
        return q, 50, check

    @case
    def one_move():
        q, a, b, d = m.kf(kf_id=90), m.kf(kf_id=30), m.kf(kf_id=20), m.kf(kf_id=5)
        m.cand[q] = [a, b]
        m.feat([q, a, b, d])

        def check(r, L):
            assert r["num_fixed"] == 2 and L["fixed"] == [d, b] and L["local"] == [q, a]
        return q, 50, check

    @case
    def else_if_is_not_the_second_lowest():
        q, a, b, c = m.kf(kf_id=100), m.kf(kf_id=50), m.kf(kf_id=60), m.kf(kf_id=40)
        m.cand[q] = [a, b, c]
        m.feat([q, a, b, c])

        def check(r, L):
            assert L["fixed"] == [c, b], "40, then 60: 50 lost `lowest` to 40 and is not demoted"
            assert L["local"] == [q, a]
        return q, 50, check

    @case
    def second_candidate_is_the_lowest_again():
        q, a = m.kf(kf_id=100), m.kf(kf_id=50)
        m.cand[q] = [a, a]
        m.feat([q, a])

        def check(r, L):
            assert L["local"] == [q] and L["fixed"] == [a, a], "list::remove took both; the second push repeats it"
            assert [e[3] for e in L["edges"]] == [0, 1]
        return q, 50, check

    @case
    def undefined_pointers():
        q = m.kf()
        m.feat([q])

        def check(r, L):
            assert r["err"] == E_UNDEF and r["num_fixed"] == 2 and L["local"] == [q] and L["fixed"] == []
            assert r["non_fixed"] == 1
        return q, 50, check

    @case
    def second_pointer_undefined():
        q, a = m.kf(kf_id=90), m.kf(kf_id=30)
        m.cand[q] = [a]
        m.feat([q, a])

        def check(r, L):
            assert r["err"] == E_UNDEF and r["num_fixed"] == 2 and L["local"] == [q] and L["fixed"] == [a]
        return q, 50, check

    @case
    def lower_id_is_sign_extended():
        q, a = m.kf(kf_id=0x80000005), m.kf(kf_id=0x80000010)
        m.cand[q] = [a]
        m.feat([q, a])

        def check(r, L):
            assert L["fixed"] == [a], "(int)mnId is negative: every 64-bit mnId is below it"
        return q, 50, check
    return cases


def inertial_cases(m):
    cases = {}

    def case(fn):
        cases[fn.__name__] = fn()
        return fn

    @case
    def chain_shorter_than_nd_and_the_pop():
        b = m.kf()
        a = m.kf(prev=b)
        q = m.kf(prev=a)
        f = [m.feat([q]), m.feat([a]), m.feat([b])]

        def check(r, L):
            assert L["local"] == [q, a] and L["fixed"] == [b] and L["feats"] == f, "b's features stay"
            assert [e[3] for e in L["edges"]] == [0, 1, 2]
        return q, 50, check

    @case
    def nd_one():
        p = m.kf()
        q = m.kf(prev=p)
        m.feat([q, p])

        def check(r, L):
            assert L["local"] == [q] and L["fixed"] == [p]
        return q, 3, check

    @case
    def nd_below_one():
        p = m.kf(init=1)
        q = m.kf(prev=p)
        m.feat([q])
        m.feat([p])

        def check(r, L):
            assert L["local"] == [q] and L["fixed"] == [p] and len(L["feats"]) == 1 and r["init_in_local"] == 0
        return q, 1, check

    @case
    def the_only_keyframe_is_popped():
        q = m.kf()
        m.feat([q])

        def check(r, L):
            assert L["local"] == [] and L["fixed"] == [q] and [e[3] for e in L["edges"]] == [0]
        return q, 50, check

    @case
    def break_bad_observer_and_the_stamp_test():
        p = m.kf()
        q = m.kf(prev=p)
        z, x, y, w, o = m.kf(bad=1), m.kf(), m.kf(), m.kf(map_id=1), m.kf()
        f0 = m.feat([q, z, x, y])     # z is passed, x is taken, the break skips y
        f1 = m.feat([q, w, o])        # no map test: w is taken, o is skipped

        def check(r, L):
            assert L["fixed"] == [p, x, w] and L["feats"] == [f0, f1]
            assert [e[1] for e in L["edges"]] == [q, x, q], "y and o are not stamped, w is of another map"
        return q, 50, check

    @case
    def cap_of_200_inside_the_point_list():
        p = m.kf()
        q = m.kf(prev=p)
        obs = [m.kf() for _ in range(210)]
        for x in obs:
            m.feat([q, x])

        def check(r, L):
            assert L["fixed"] == [p] + obs[:199] and r["n_fixed_kf"] == 200
            assert len(L["edges"]) == 210 + 199
        return q, 50, check

    @case
    def every_list_nonempty():
        p = m.kf()
        q = m.kf(prev=p)
        m.feat([q, p, (m.kf(), TWO)])
        m.feat([q])

        def check(r, L):
            assert len(L["local"]) == 1 and len(L["fixed"]) == 2 and len(L["feats"]) == 2 and len(L["edges"]) == 4
        return q, 50, check
    return cases


@functools.lru_cache(None)
def crafted(mode):
    m = BAMap(cap=256 if mode == INERTIAL else 16, lines=mode == LINES)
    cases = inertial_cases(m) if mode == INERTIAL else visual_cases(m, mode)
    return m.tables(), cases


MODES = (POINTS, LINES, INERTIAL)
CASE_IDS = [(mode, name) for mode in MODES for name in crafted(mode)[1]]


@pytest.mark.parametrize("mode,name", CASE_IDS)
def test_crafted_case_shows_what_it_is_for(mode, name):
    tabs, cases = crafted(mode)
    q, n_kf, check = cases[name]
    r = ref_window(tabs, mode, q, n_kf)
    assert r == np_window(tabs, mode, q, n_kf)
    ne = r["n_mono"] + r["n_stereo"] + r["n_line"]
    assert -1 not in r["edge_cam"][:ne], "every edge's keyframe is in one of the two lists"
    check(r, lists_of(r))


def over_caps(tabs, mode):
    """Capacities one below every list of the case every_list_nonempty."""
    q, n_kf, _ = crafted(mode)[1]["every_list_nonempty"]
    r = ref_window(tabs, mode, q, n_kf)
    return dict(lkf_cap=r["n_local_kf"] - 1, fkf_cap=r["n_fixed_kf"] - 1, feat_cap=r["n_local_feat"] - 1,
                edge_cap=r["n_mono"] + r["n_stereo"] + r["n_line"] - 1)


@pytest.mark.parametrize("mode", MODES)
def test_one_over_every_capacity(mode):
    tabs, cases = crafted(mode)
    caps = over_caps(tabs, mode)
    q, n_kf, _ = cases["every_list_nonempty"]
    r = ref_window(tabs, mode, q, n_kf, caps=caps)
    assert r == np_window(tabs, mode, q, n_kf, caps=caps)
    assert r["err"] == E_LKF | E_FKF | E_FEAT | E_EDGE
    for k, c in LISTS.items():
        fill = FILL8 if k == "edge_kind" else FILL
        assert r[k][caps[c]:] == [fill] * (len(r[k]) - caps[c]) and fill not in r[k][:caps[c]]


def test_query_out_of_range():
    tabs, _ = crafted(POINTS)
    for q in (-1, len(tabs[0]["bad"])):
        r = ref_window(tabs, POINTS, q)
        assert r == np_window(tabs, POINTS, q) and r["err"] == E_QUERY and r["local_kf"][0] == FILL


# ------------------------------------------------------------ random maps
N_RANDOM = 60


def random_submap(m, rng, mode, big):
    """One random map appended to m; returns (q_slot, n_kf_in_map).  big: more than 200 eligible observers."""
    K = 260 if big else int(rng.integers(1, 49))
    maps = (2 * (m.K + 1), 2 * (m.K + 1) + 1)
    tiny = not big and rng.random() < 0.25
    ids = rng.permutation(4 * K)[:K] + 1
    slots = [m.kf(bad=int(rng.random() < 0.12), map_id=maps[int(rng.random() < 0.15)], kf_id=int(ids[i]))
             for i in range(K)]
    q = slots[int(rng.integers(K))]
    m.kf_map[q] = maps[0]
    for s in slots:      # one temporal chain through a shuffle of the slots, with gaps
        if rng.random() < 0.8:
            m.prev[s] = slots[int(rng.integers(K))]
    if big:              # a chain of 9, so that several hundred points are local
        chain = [q] + [s for s in rng.permutation(slots).tolist() if s != q][:8]
        for a, b in zip(chain, chain[1:]):
            m.prev[a] = b
    n_row = 0 if tiny else int(rng.integers(0, min(K, 12) + 1))
    row = [slots[int(i)] for i in rng.integers(0, K, n_row)]
    if n_row and rng.random() < 0.3:
        row[int(rng.integers(n_row))] = OUT if rng.random() < 0.5 else q
    m.cand[q] = row
    n_feat = int(rng.integers(0, 8)) if tiny else int(rng.integers(540, 600) if big else rng.integers(0, 120))
    closed = not big and rng.random() < 0.5     # observed by q and its row alone: no fixed camera, step 4 runs
    core = [q] + [s for s in row if 0 <= s < m.K]
    c = q
    for _ in range(0 if closed else 6):
        c = m.prev[c]
        if not 0 <= c < m.K:
            break
        core.append(c)
    if big:
        core = chain
    if rng.random() < 0.6:     # GetInitKFid() names one keyframe
        m.init[core[int(rng.integers(len(core)))] if rng.random() < 0.5 else slots[int(rng.integers(K))]] = 1
    for _ in range(n_feat):
        n_obs = int(rng.integers(1, 3 if tiny else 7))
        near = big or closed or rng.random() < (0.2 if tiny else 0.8)
        pick = set()
        if near:
            pick.add(core[int(rng.integers(len(core)))])
        while len(pick) < min(n_obs, len(set(core)) if closed else K):
            pick.add((core if closed else slots)[int(rng.integers(len(core) if closed else K))])
        obs = []
        for s in pick:
            if len(m.tab[s]) >= m.cap:
                continue
            flags = TWO if rng.random() < 0.3 else 0
            obs.append((s, flags, int(rng.choice([m.cap, -1]))) if rng.random() < 0.03 else (s, flags))
        if rng.random() < 0.05:
            obs.append((OUT, 0))
        m.feat(obs, bad=int(rng.random() < 0.08), map_id=maps[int(rng.random() < 0.1)])
    return q, 40 if big else int(rng.integers(1, 40))


@functools.lru_cache(None)
def random_maps(mode):
    rng = np.random.default_rng(2400 + mode)
    m = BAMap(cap=64, lines=mode == LINES)
    queries = [random_submap(m, rng, mode, big=mode == INERTIAL and i % 4 == 0) for i in range(N_RANDOM)]
    tabs = m.tables()
    caps = big_caps(tabs)
    # four maps run against capacities of 3, for the overflow bits; the last query is out of range
    small = dict(lkf_cap=3, fkf_cap=3, feat_cap=3, edge_cap=3)
    return tabs, queries + [(len(tabs[0]["bad"]), 5)], caps, small


@functools.lru_cache(None)
def random_expected(mode, small=False):
    tabs, queries, caps, small_caps = random_maps(mode)
    return [ref_window(tabs, mode, q, n_kf, max_opt=25 if i % 2 else 10, caps=small_caps if small else caps)
            for i, (q, n_kf) in enumerate(queries)]


@pytest.mark.parametrize("mode", MODES)
def test_random_maps_restatements_agree_and_cover(mode):
    tabs, queries, caps, small_caps = random_maps(mode)
    exp = random_expected(mode)
    K = len(tabs[0]["bad"])
    moved = unlisted = capped = err_bits = 0
    for i, ((q, n_kf), r) in enumerate(zip(queries, exp)):
        assert r == np_window(tabs, mode, q, n_kf, max_opt=25 if i % 2 else 10, caps=caps), (mode, i)
        if r["err"] & E_QUERY:
            err_bits |= r["err"]
            continue
        L = lists_of(r)
        assert all(e[3] >= 0 for e in L["edges"]), "every edge's keyframe is in one of the two lists"
        err_bits |= r["err"]
        if mode == POINTS:
            # a fixed camera of step 3 is never in the row: one that is was moved there by step 4
            moved += any(s in L["fixed"] for s in tabs[0]["cand"][q][:tabs[0]["n_cand"][q]].tolist())
        if mode != INERTIAL:   # a keyframe that is stamped and never listed: bad or of another map
            row = [s for s in tabs[0]["cand"][q][:tabs[0]["n_cand"][q]].tolist() if 0 <= s < K]
            seen = {int(s) for f in L["feats"] for s in tabs[1]["obs_kf"][tabs[1]["obs_off"][f]:tabs[1]["obs_off"][f + 1]]
                    if 0 <= s < K}
            unlisted += bool((set(row) | seen) - set(L["local"]) - set(L["fixed"]))
        else:
            capped += r["n_fixed_kf"] == 200
    for i, (q, n_kf) in enumerate(queries[:4]):
        r = random_expected(mode, True)[i]
        assert r == np_window(tabs, mode, q, n_kf, max_opt=25 if i % 2 else 10, caps=small_caps)
        err_bits |= r["err"]
    if mode == POINTS:
        assert moved >= 10, moved
        assert err_bits == 63, err_bits
    else:
        assert err_bits == 63 - E_UNDEF, err_bits
    if mode != INERTIAL:
        assert unlisted >= 10, unlisted
    else:
        assert capped >= 10, capped


# ---------------------------------------------------------------- the device
def batch_equals(win, tabs, mode, queries, caps, max_opt=10, expected=None, stream_graph=False):
    qs = [q for q, _ in queries]
    nk = [n for _, n in queries]
    got = win.batch(qs, nk, fill=FILL, **caps)
    assert got["rc"] == 0
    for k, v in got["past"].items():
        v = v if isinstance(v, list) else [v]
        assert set(v) <= {FILL, FILL8}, f"{k}: written past the batch"
    for i, (q, n_kf) in enumerate(queries):
        exp = expected[i] if expected else ref_window(tabs, mode, q, n_kf, max_opt=max_opt, caps=caps)
        assert plain(got, i) == exp, (mode, i, q)
    return got


def host_equals(win, tabs, mode, q, n_kf, caps, max_opt=10, exp=None):
    exp = exp or ref_window(tabs, mode, q, n_kf, max_opt=max_opt, caps=caps)
    got = win.host(q, n_kf, fill=FILL, **caps)
    assert plain(got, 0) == exp, (mode, q)
    assert got["rc"] == (plvi.PLVI_E_CAPACITY if exp["err"] & ~E_UNDEF else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_crafted_cases_one_batch(plvi_lib, mode):
    tabs, cases = crafted(mode)
    queries = [(q, n) for q, n, _ in cases.values()] + [(-1, 5), (len(tabs[0]["bad"]), 5)]
    win = window(tabs, mode)
    batch_equals(win, tabs, mode, queries, big_caps(tabs))
    batch_equals(win, tabs, mode, queries, over_caps(tabs, mode))
    for q, n in queries:
        host_equals(win, tabs, mode, q, n, big_caps(tabs))
    q, n, _ = cases["every_list_nonempty"]
    host_equals(win, tabs, mode, q, n, over_caps(tabs, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_random_maps_one_batch(plvi_lib, mode):
    tabs, queries, caps, small_caps = random_maps(mode)
    for max_opt, sel in ((10, slice(0, None, 2)), (25, slice(1, None, 2))):
        win = window(tabs, mode, max_opt)
        batch_equals(win, tabs, mode, queries[sel], caps, expected=random_expected(mode)[sel])
    win = window(tabs, mode, 10)
    batch_equals(win, tabs, mode, queries[:4:2], small_caps, expected=random_expected(mode, True)[:4:2])
    for i in range(0, len(queries), 6):      # the host form on every sixth (it stages the whole map per call)
        host_equals(win, tabs, mode, *queries[i], caps, exp=random_expected(mode)[i])


def shape_map(mode, n_kf=40, cap=256, feats_per_kf=200, pad_kf=0, seed=7):
    """One query whose row has n_kf keyframes: 40 x 256 table entries against the 8192 positions the feature
    compaction takes per block scan, and more than 2048 local features against the 1024 features the edge pass
    takes per block scan."""
    rng = np.random.default_rng(seed)
    m = BAMap(cap=cap, lines=mode == LINES)
    prev = -1
    slots = []
    for i in range(n_kf):
        prev = m.kf(prev=prev, bad=int(i % 11 == 10))
        slots.append(prev)
    q = slots[-1]
    m.cand[q] = [s for s in reversed(slots[:-1])]
    far = [m.kf() for _ in range(30)]
    for _ in range(n_kf * feats_per_kf // 3):
        pick = {int(s) for s in rng.choice(slots, 3, replace=False)} | {int(s) for s in rng.choice(far, 2, replace=False)}
        m.feat([(s, TWO if rng.random() < 0.5 else 0) for s in pick if len(m.tab[s]) < cap])
    return m.tables(pad_kf=pad_kf), q


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_traversals_longer_than_a_tile(plvi_lib, mode):
    tabs, q = shape_map(mode)
    caps = big_caps(tabs)
    exp = ref_window(tabs, mode, q, 50, max_opt=25, caps=caps)
    if mode != INERTIAL:     # the inertial window is the chain's 25 keyframes
        assert exp["n_local_kf"] * 256 > 8192 and exp["n_local_feat"] > 2 * 1024
    else:
        assert exp["n_local_feat"] > 1024
    win = window(tabs, mode, 25)
    batch_equals(win, tabs, mode, [(q, 50)], caps, max_opt=25)               # 1 query
    batch_equals(win, tabs, mode, [(q, 50)] * 64 + [(0, 4)], caps, max_opt=25)   # 65 queries
    host_equals(win, tabs, mode, q, 50, caps, max_opt=25)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (POINTS, LINES))
def test_gpu_kp_cap_4(plvi_lib, mode):
    tabs, q = shape_map(mode, n_kf=12, cap=4, feats_per_kf=4)
    batch_equals(window(tabs, mode), tabs, mode, [(q, 50), (0, 50)], big_caps(tabs))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_scratch_path_above_the_lds_bound(plvi_lib, mode):
    """kf_cap just above PLVI_BA_LDS_KF with slots 0, bound - 1 and bound + 7 occupied."""
    B = plvi.BA_LDS_KF
    m = BAMap(cap=8, lines=mode == LINES)
    for _ in range(B + 8):
        m.kf(bad=1)
    a, b, c = 0, B - 1, B + 7
    for s in (a, b, c):
        m.bad[s] = 0
    m.prev[c] = b
    m.cand[c] = [b]
    m.feat([a, (b, TWO), c])
    m.feat([b])
    tabs = m.tables()
    exp = ref_window(tabs, mode, c, 50)
    assert exp["local_kf"][:2] == ([c] if mode == INERTIAL else [c, b]) + ([FILL] if mode == INERTIAL else [])
    assert a in exp["fixed_kf"][:exp["n_fixed_kf"]]
    batch_equals(window(tabs, mode), tabs, mode, [(c, 50), (a, 50)], big_caps(tabs))


@pytest.mark.gpu
def test_gpu_graph_capture_and_replay(plvi_lib):
    """One batch captured into a hipGraph and replayed once: no host read, no allocation, no sync inside."""
    tabs, cases = crafted(POINTS)
    queries = [(q, n) for q, n, _ in cases.values()]
    win = window(tabs, POINTS)
    caps = big_caps(tabs)
    step, fetch = win.batch([q for q, _ in queries], [n for _, n in queries], fill=FILL, run=False, **caps)
    st = ctypes.c_void_p()
    assert plvi_lib.plvi_stream_create(ctypes.byref(st)) == 0
    rcs = []
    graph = plvi.StepGraph(lambda s: rcs.append(step(s)), st.value)
    assert rcs == [0]
    assert (fetch()["n_local_kf"] == FILL).all()   # captured, not run
    graph.launch()
    assert plvi_lib.plvi_stream_synchronize(st) == 0
    got = fetch()
    for i, (q, n) in enumerate(queries):
        assert plain(got, i) == ref_window(tabs, POINTS, q, n, caps=caps)
