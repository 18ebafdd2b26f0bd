"""The covisibility graph on the device (csrc/covis.hip, plvi_covis_*): KeyFrame::UpdateConnections[WithLines]
(src/KeyFrame.cc:499-622 / :624-769) for a batch of keyframes, AddConnection, UpdateBestCovisibles, EraseConnection,
the connection part of SetBadFlag and the two getters.

Expected values come from tests/native/covis_ref.cpp, a sequential host restatement in the reference's own shape
(KeyFrame objects placed so that ascending address is `order`, std::map<KeyFrame*, int>, vector<pair<int,
KeyFrame*>> + std::sort + push_front, AddConnection with its early return, the queries applied one by one).  The
CPU part pins it against NpRunner below, an independent restatement in the GATHER formulation the kernels use -- a
bincount vote, lexsort on (weight, rank), every query's own map and list first, then the AddConnections with the
position rule (a neighbour that is itself a later query with a counter is skipped), a neighbour re-sorted iff its
map changed -- on every crafted case and on random maps, and checks what each crafted case is there to show.  The
gpu part demands exact equality with the restatement: every slot's downloaded map and ordered list, the per-query
outputs, first_conn, parent, the covis rows and the error bits, with sentinel-filled tables.

A case is (map, script, check): the script is a list of ("update", slots) / ("erase", slots) / ("resort", slots) /
("mut", fn(map)) / ("snap",) steps; every runner returns the outputs of each update and a snapshot of the whole
graph at each snap and at the end."""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import plvi
import test_local_map as tl

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "covis_ref.cpp"
BUILD = ROOT / "tests" / "native" / "_build"
FILL = -7
E_BADARG, E_CAPACITY = -2, -3
NB = 10
OUTS = ("n_counted", "n_conn", "kf_max", "w_max", "new_parent", "err")

_lib = None


def ref_lib():
    global _lib
    if _lib is None:
        so = BUILD / "libcovis_ref.so"
        if not so.exists() or so.stat().st_mtime < SRC.stat().st_mtime:
            so.parent.mkdir(parents=True, exist_ok=True)
            subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", str(so),
                            str(SRC)], check=True)
        _lib = ctypes.CDLL(str(so))
        V, I = ctypes.c_void_p, ctypes.c_int
        _lib.covis_ref_create.argtypes, _lib.covis_ref_create.restype = [I], V
        _lib.covis_ref_destroy.argtypes, _lib.covis_ref_destroy.restype = [V], None
        _lib.covis_ref_update.argtypes = [V, V, V, I, V, V, I, V, V, I, V, V, V, V, I, V, V, V, I, V, V, V, I, V] + [V] * 6
        _lib.covis_ref_update.restype = None
        for fn in (_lib.covis_ref_erase, _lib.covis_ref_resort):
            fn.argtypes, fn.restype = [V, I, V, V, V, I, V], None
        _lib.covis_ref_get.argtypes, _lib.covis_ref_get.restype = [V, I, V, V, V, V, V, V], None
        _lib.covis_ref_by_weight.argtypes, _lib.covis_ref_by_weight.restype = [V, I, I], I
        _lib.covis_ref_weight.argtypes, _lib.covis_ref_weight.restype = [V, I, I], I
        _lib.covis_ref_seconds.argtypes, _lib.covis_ref_seconds.restype = [], ctypes.c_double
    return _lib


class CMap(tl.Map):
    """tl.Map with the tables UpdateConnections reads besides: map ids, the initial keyframe, mbFirstConnection."""

    def __init__(self, K, kp_cap=64, n_mp=1024, kl_cap=0, n_ml=0, conn_cap=None, slots=None):
        super().__init__(K, kp_cap, n_mp, kl_cap, n_ml)
        self.map_id = None
        self.init = np.zeros(K, np.uint8)
        self.first = np.zeros(K, np.uint8)
        self.conn_cap = min(K, 64) if conn_cap is None else conn_cap
        self.slots = list(range(K)) if slots is None else slots   # the slots whose state is compared

    def link(self, a, b, n):
        """n new MapPoints that a and b both hold and that observe both."""
        for _ in range(n):
            p = self.point(a, b)
            self.put(a, p)
            self.put(b, p)

    def see(self, a, b, n):
        """n new MapPoints in a's table that observe a and b; b does not hold them (an asymmetric count)."""
        for _ in range(n):
            self.put(a, self.point(a, b))

    def link_l(self, a, b, n):
        for _ in range(n):
            p = self.line(a, b)
            self.put_line(a, p)
            self.put_line(b, p)

    def see_l(self, a, b, n):
        for _ in range(n):
            self.put_line(a, self.line(a, b))

    def ctables(self):
        """The dicts plvi.Covisibility.set_tables takes, without the in/out tables."""
        kf, mp, ml = self.tables()
        c = {k: kf[k] for k in ("bad", "order", "mp", "nmp")}
        if self.kl_cap:
            c.update(ml=kf["ml"], nml=kf["nml"])
        if self.map_id is not None:
            c["map_id"] = np.asarray(self.map_id, np.int32)
        c["init_kf"] = self.init
        return c, mp, ml


def plain(x):
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return int(x) if isinstance(x, (np.integer,)) else x


class Runner:
    """The steps of a script on one implementation."""

    def __init__(self, m):
        self.m, self.K = m, m.K
        self.first, self.parent = m.first.copy(), m.parent.copy()
        self.covis = np.full((m.K, NB), FILL, np.int32)

    def sync(self):
        pass

    def rows(self, touched):
        """The covis rows of the slots whose list was assigned: rewritten whole."""
        for s in np.nonzero(touched)[0]:
            o = [k for k, _ in self.lists(int(s))[1]][:NB]
            self.covis[s] = o + [-1] * (NB - len(o))

    def snapshot(self):
        st = {s: self.lists(s) for s in self.m.slots}
        return plain(dict(state=st, first=self.first, parent=self.parent, covis=self.covis,
                          err={s: self.err(s) for s in self.m.slots}))

    def err(self, s):
        return 0

    def run(self, script):
        out = []
        for op in script:
            if op[0] == "update":
                out.append(plain(self.update(list(op[1]))))
            elif op[0] == "erase":
                self.erase(list(op[1]))
            elif op[0] == "resort":
                self.resort(list(op[1]))
            elif op[0] == "mut":
                op[1](self.m)
                self.sync()
            elif op[0] == "snap":
                out.append(self.snapshot())
            else:
                raise ValueError(op)
        out.append(self.snapshot())
        return out


class RefRunner(Runner):
    """tests/native/covis_ref.cpp."""

    def __init__(self, m):
        super().__init__(m)
        self.lib = ref_lib()
        self.h = ctypes.c_void_p(self.lib.covis_ref_create(m.K))
        self.seconds = 0.0

    def __del__(self):
        self.lib.covis_ref_destroy(self.h)

    def _kf(self):
        kf, mp, ml = self.m.ctables()
        a = {k: np.ascontiguousarray(v, np.uint8 if k in ("bad", "init_kf") else np.int32) for k, v in kf.items()}
        return a, mp, ml

    def update(self, q):
        a, mp, ml = self._kf()
        p = tl._p
        qa = np.array(q, np.int32)
        o = {k: np.zeros(len(q) + 1, np.int32) for k in OUTS}
        touched = np.zeros(self.K, np.int32)
        pm = {k: np.ascontiguousarray(mp[k]) for k in ("bad", "obs_off", "obs_kf")}
        pl = {k: np.ascontiguousarray(ml[k]) for k in ("bad", "obs_off", "obs_kf")} if ml is not None else {}
        self.lib.covis_ref_update(
            self.h, p(a["bad"]), p(a["order"]), len(a["order"]), p(a["mp"]), p(a["nmp"]), self.m.kp_cap,
            p(a.get("ml")), p(a.get("nml")), self.m.kl_cap, p(a.get("map_id")), p(a["init_kf"]), p(self.first),
            p(self.parent), len(pm["bad"]), p(pm["bad"]), p(pm["obs_off"]), p(pm["obs_kf"]),
            len(pl["bad"]) if pl else 0, p(pl.get("bad")), p(pl.get("obs_off")), p(pl.get("obs_kf")), len(q), p(qa),
            p(o["n_counted"]), p(o["n_conn"]), p(o["kf_max"]), p(o["w_max"]), p(o["new_parent"]), p(touched))
        self.seconds = self.lib.covis_ref_seconds()
        self.rows(touched)
        return {k: v[:len(q)] for k, v in o.items()}

    def _slots(self, fn, slots):
        a, _, _ = self._kf()
        touched = np.zeros(self.K, np.int32)
        fn(self.h, len(slots), tl._p(np.array(slots, np.int32)), tl._p(a["bad"]), tl._p(a["order"]), len(a["order"]),
           tl._p(touched))
        self.rows(touched)

    def erase(self, slots):
        self._slots(self.lib.covis_ref_erase, slots)

    def resort(self, slots):
        self._slots(self.lib.covis_ref_resort, slots)

    def lists(self, s):
        t = [np.zeros(self.K + 1, np.int32) for _ in range(4)]
        n = [ctypes.c_int(), ctypes.c_int()]
        self.lib.covis_ref_get(self.h, s, tl._p(t[0]), tl._p(t[1]), ctypes.byref(n[0]), tl._p(t[2]), tl._p(t[3]),
                               ctypes.byref(n[1]))
        return (list(zip(t[0][:n[0].value].tolist(), t[1][:n[0].value].tolist())),
                list(zip(t[2][:n[1].value].tolist(), t[3][:n[1].value].tolist())))


class NpRunner(Runner):
    """The independent restatement, gather formulation."""

    def __init__(self, m):
        super().__init__(m)
        self.w = [dict() for _ in range(m.K)]
        self.o = [[] for _ in range(m.K)]

    def rank(self):
        r = np.full(self.K, -1, np.int64)
        for i, s in enumerate(self.m.order):
            if 0 <= s < self.K and r[s] < 0:
                r[s] = i
        named = r >= 0
        r[~named] = len(self.m.order) + np.nonzero(~named)[0]
        return r, named

    def sort(self, pairs, rank):
        """Descending by (weight, rank)."""
        if not pairs:
            return []
        k, w = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
        idx = np.lexsort((rank[k], w))[::-1]
        return [(int(k[i]), int(w[i])) for i in idx]

    def resorted(self, s, rank):
        return self.sort([(k, w) for k, w in self.w[s].items() if not self.m.bad[k]], rank)

    def counter(self, q, named):
        m, K = self.m, self.K
        _, mp, ml = m.ctables()
        count = np.zeros(K, np.int64)
        for tab, cnt, cap, pool in ((m.kf_mp, m.nmp, m.kp_cap, mp), (m.kf_ml, m.nml, m.kl_cap, ml)):
            if pool is None or cap == 0:
                continue
            ids = tab[q, :max(min(int(cnt[q]), cap), 0)]
            ids = ids[(ids >= 0) & (ids < len(pool["bad"]))]
            ids = ids[pool["bad"][ids] == 0]
            off, obs = pool["obs_off"], pool["obs_kf"]
            lens = off[ids + 1] - off[ids]
            idx = np.repeat(off[ids], lens) + np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens)
            o = obs[idx]
            count += np.bincount(o[(o >= 0) & (o < K)], minlength=K)
        count[q] = 0
        count[m.bad != 0] = 0
        count[~named] = 0
        if m.map_id is not None:
            count[np.asarray(m.map_id) != m.map_id[q]] = 0
        return count

    def update(self, q):
        m = self.m
        rank, named = self.rank()
        out = {k: [0] * len(q) for k in OUTS}
        touched = np.zeros(self.K, np.int32)
        listed, pos = [], {s: i for i, s in enumerate(q)}
        for i, s in enumerate(q):
            c = self.counter(s, named)
            kfs = np.nonzero(c)[0]
            kfs = kfs[np.argsort(rank[kfs])]                       # the std::map walk
            out["n_counted"][i] = len(kfs)
            out["kf_max"][i], out["new_parent"][i] = -1, -1
            if not len(kfs):
                listed.append(None)
                continue
            kmax = int(kfs[np.argmax(c[kfs])])                     # argmax: the first of the largest
            out["kf_max"][i], out["w_max"][i] = kmax, int(c[kmax])
            pairs = [(int(k), int(c[k])) for k in kfs if c[k] >= 15] or [(kmax, int(c[kmax]))]
            self.w[s] = {int(k): int(c[k]) for k in kfs}
            self.o[s] = self.sort(pairs, rank)
            out["n_conn"][i] = len(pairs)
            touched[s] = 1
            listed.append(pairs)
            if self.first[s] and not m.init[s]:
                self.parent[s] = out["new_parent"][i] = self.o[s][0][0]
                self.first[s] = 0
        dirty = set()
        for i, s in enumerate(q):
            for t, w in listed[i] or ():
                j = pos.get(t)
                if j is not None and j > i and listed[j] is not None:
                    continue                                       # t's own update comes later and overwrites this
                if self.w[t].get(s) != w:
                    self.w[t][s] = w
                    dirty.add(t)
        for t in dirty:
            self.o[t] = self.resorted(t, rank)
            touched[t] = 1
        self.rows(touched)
        return out

    def erase(self, slots):
        rank, _ = self.rank()
        gone, dirty = set(slots), set()
        touched = np.zeros(self.K, np.int32)
        for s in slots:
            for k in self.w[s]:
                if k not in gone and s in self.w[k]:
                    del self.w[k][s]
                    dirty.add(k)
        for k in dirty:
            self.o[k] = self.resorted(k, rank)
            touched[k] = 1
        for s in slots:
            self.w[s], self.o[s] = {}, []
            touched[s] = 1
        self.rows(touched)

    def resort(self, slots):
        rank, _ = self.rank()
        touched = np.zeros(self.K, np.int32)
        for s in slots:
            self.o[s] = self.resorted(s, rank)
            touched[s] = 1
        self.rows(touched)

    def lists(self, s):
        return sorted(self.w[s].items()), list(self.o[s])


class GpuRunner(Runner):
    """plvi.Covisibility: the batch form, or the host form query by query."""

    def __init__(self, m, host_form=False):
        super().__init__(m)
        self.host_form = host_form
        self.cov = plvi.Covisibility(m.K, m.conn_cap)
        kf, mp, ml = m.ctables()
        kf.update(first_conn=self.first, parent=self.parent, covis=self.covis)
        self.cov.set_tables(kf, mp, ml)
        self.first, self.parent, self.covis = (self.cov.kf[k] for k in ("first_conn", "parent", "covis"))
        self.past = []

    def sync(self):
        kf, mp, ml = self.m.ctables()
        for k, a in kf.items():
            self.cov.put("kf", k, a)
        for g, p in (("mp", mp), ("ml", ml)):
            for k in ("bad", "obs_off", "obs_kf") if p is not None else ():
                self.cov.put(g, k, p[k])

    def update(self, q):
        if self.host_form:
            rs = [self.cov.update(s) for s in q]
            assert all(r["rc"] in (0, E_CAPACITY) for r in rs)
            return {k: [r[k] for r in rs] for k in OUTS}
        r = self.cov.update_batch(q, fill=FILL)
        assert r["rc"] == 0
        self.past.append(r["past"])
        return {k: r[k] for k in OUTS}

    def erase(self, slots):
        assert self.cov.erase(slots) == 0

    def resort(self, slots):
        assert self.cov.resort(slots) == 0

    def snapshot(self):
        if not self.host_form:
            self.first, self.parent, self.covis = (self.cov.table(k) for k in ("first_conn", "parent", "covis"))
        self._dl = {s: self.cov.download(s, FILL) for s in self.m.slots}
        for d in self._dl.values():   # nothing past the counts
            assert (d["map_kf"][d["n_map"]:] == FILL).all() and (d["ord_w"][d["n_ord"]:] == FILL).all()
        return super().snapshot()

    def lists(self, s):
        d = self._dl[s]
        return (list(zip(d["map_kf"][:d["n_map"]].tolist(), d["map_w"][:d["n_map"]].tolist())),
                list(zip(d["ord_kf"][:d["n_ord"]].tolist(), d["ord_w"][:d["n_ord"]].tolist())))

    def err(self, s):
        return self._dl[s]["err"]


# ------------------------------------------------------------------ crafted cases
# Each returns (map, script, check) -- check(results of the restatement) lists what the case shows.  S(r) is the final
# graph: S(r)[slot] = (map as sorted (slot, weight) pairs, ordered list).

def S(r, i=-1):
    return {s: tuple(v) for s, v in r[i]["state"].items()}


def case_threshold():
    m = CMap(8)
    m.see(0, 1, 14)
    m.see(0, 2, 15)
    m.see(0, 3, 16)
    return m, [("update", [0])], lambda r: [
        r[0]["n_counted"] == [3], r[0]["n_conn"] == [2], r[0]["kf_max"] == [3], r[0]["w_max"] == [16],
        S(r)[0] == ([[1, 14], [2, 15], [3, 16]], [[3, 16], [2, 15]]),
        S(r)[1] == ([], []), S(r)[2] == ([[0, 15]], [[0, 15]]), S(r)[3] == ([[0, 16]], [[0, 16]]),
        r[-1]["covis"][0] == [3, 2] + [-1] * 8, r[-1]["covis"][1] == [FILL] * NB]


def case_none_at_15_tie(perm=False):
    """Nothing reaches 15 and the largest count is tied at two positions: pKFmax is the first of them in `order`."""
    m = CMap(8)
    for k, n in ((1, 5), (4, 9), (6, 9), (7, 3)):
        m.see(0, k, n)
    if perm:
        m.order = [7, 6, 5, 4, 3, 2, 1, 0]
    k = 6 if perm else 4
    return m, [("update", [0])], lambda r: [
        r[0]["kf_max"] == [k], r[0]["n_conn"] == [1], r[0]["n_counted"] == [4], S(r)[0][1] == [[k, 9]],
        S(r)[k] == ([[0, 9]], [[0, 9]]), S(r)[10 - k] == ([], [])]


def case_empty_counter():
    """An empty counter returns at once (:534): map, list, first_conn, parent and the covis row are left alone."""
    m = CMap(8)
    m.see(1, 0, 20)        # keyframe 0 holds no feature itself; 1's update gives it a map and a list
    m.first[0], m.parent[0] = 1, 5
    return m, [("update", [1]), ("snap",), ("update", [0])], lambda r: [
        r[2] == dict(n_counted=[0], n_conn=[0], kf_max=[-1], w_max=[0], new_parent=[-1], err=[0]),
        S(r)[0] == S(r, 1)[0] == ([[1, 20]], [[1, 20]]), r[-1]["first"][0] == 1, r[-1]["parent"][0] == 5,
        r[-1]["covis"] == r[1]["covis"], r[-1]["covis"][0] == [1] + [-1] * 9]


def case_must_not_count():
    m = CMap(8, kp_cap=200)
    m.order = [0, 1, 2, 3, 4, 6, 7]          # 5 is an empty slot: bad, and not named
    m.bad[5] = 1
    m.map_id = [0, 0, 0, 1, 0, 0, 0, 0]
    m.put(0, *[m.point(0) for _ in range(20)])            # self observations alone
    m.see(0, 2, 30)
    m.bad[2] = 1                              # a bad keyframe holding the most observations
    m.see(0, 3, 25)                           # a keyframe of another map
    m.see(0, 5, 22)                           # an empty slot
    m.put(0, *[m.point(0, 1, 8 + 3, -2, 2 ** 30) for _ in range(16)])   # observation slots outside [0, kf_cap)
    badp = [m.point(0, 4) for _ in range(17)]
    m.mp_bad[badp] = 1
    m.put(0, -1, *badp, -5, len(m.mp_bad), len(m.mp_bad) + 5, 2 ** 30)  # NULL, bad and out-of-range ids
    return m, [("update", [0])], lambda r: [r[0]["n_counted"] == [1], S(r)[0] == ([[1, 16]], [[1, 16]]),
                                            S(r)[1][0] == [[0, 16]], all(S(r)[k] == ([], []) for k in (2, 3, 4, 5))]


def case_id_twice():
    m = CMap(8)
    m.see(0, 1, 13)
    p = m.point(0, 1)
    m.put(0, p, p)
    return m, [("update", [0])], lambda r: [S(r)[0] == ([[1, 15]], [[1, 15]]), S(r)[1][1] == [[0, 15]]]


def case_lines(with_lines=True):
    """Lines count into the same counter: they lift keyframe 1 from 14 to 15 and move pKFmax to keyframe 2."""
    m = CMap(8, kl_cap=8 if with_lines else 0, n_ml=16 if with_lines else 0)
    m.see(0, 1, 14)
    m.see(0, 2, 12)
    if with_lines:
        m.see_l(0, 1, 1)
        m.see_l(0, 2, 5)
        bad = m.line(0, 1)
        m.ml_bad[bad] = 1
        m.put_line(0, bad, -1)
    want = ([[2, 17], [1, 15]], 2) if with_lines else ([[1, 14]], 1)
    return m, [("update", [0])], lambda r: [S(r)[0][1] == want[0], r[0]["kf_max"] == [want[1]]]


def case_equal_weights_by_rank():
    """Equal weights: sort() on pair<int, KeyFrame*> and push_front leave the LATER keyframe of `order` first."""
    m = CMap(8, kp_cap=128)
    for k in range(1, 6):
        m.see(0, k, 15)
    m.order = [3, 0, 5, 1, 7, 4, 2, 6]
    return m, [("update", [0])], lambda r: [S(r)[0][1] == [[k, 15] for k in (2, 4, 1, 5, 3)], r[0]["kf_max"] == [3]]


def case_neighbour_lists():
    """A list built by UpdateConnections (the >= 15 entries, bad ones kept) against one built by UpdateBestCovisibles
    (the whole map, bad ones dropped): keyframe 1's list under an unchanged and under a changed weight."""
    m = CMap(8, kp_cap=128)
    m.link(1, 2, 10)
    m.link(1, 3, 20)
    m.link(1, 4, 18)
    m.link(0, 1, 16)
    own = [[3, 20], [4, 18], [0, 16]]
    return m, [("update", [0]), ("update", [1]), ("snap",),
               ("mut", lambda m: m.bad.__setitem__(4, 1)), ("update", [0]), ("snap",),
               ("mut", lambda m: m.link(0, 1, 1)), ("update", [0])], lambda r: [
        S(r, 2)[1] == ([[0, 16], [2, 10], [3, 20], [4, 18]], own),
        S(r, 4)[1][1] == own,                                    # the weight is unchanged: no re-sort, 4 stays
        S(r)[1][1] == [[3, 20], [0, 17], [2, 10]],               # changed: the entry below 15 appears, the bad one goes
        S(r)[1][0] == [[0, 17], [2, 10], [3, 20], [4, 18]],
        r[-1]["covis"][1] == [3, 0, 2] + [-1] * 7]


def case_batch_pair(order, sym):
    """Queries 0 and 1 see each other; 2 is a third party both add themselves to."""
    m = CMap(8, kp_cap=128)
    if sym:
        m.link(0, 1, 20)
    else:
        m.see(0, 1, 18)
        m.see(1, 0, 25)
    m.link(0, 2, 16)
    m.link(1, 2, 17)
    a, b = order
    wa = 20 if sym else (18 if a == 0 else 25)     # the first query's count of the second

    def check(r):
        first_list = S(r)[a][1]
        # a's own list stands unless b's AddConnection changed a's map: symmetric counts leave it alone
        return [S(r)[2] == ([[0, 16], [1, 17]], [[1, 17], [0, 16]]), len(first_list) == 2,
                (first_list == [[b, wa], [2, 16 + a]]) == sym]
    return m, [("update", order)], check


def case_cycle():
    m = CMap(8, kp_cap=128)
    m.see(0, 1, 15)
    m.see(1, 2, 16)
    m.see(2, 0, 17)
    m.see(1, 0, 3)
    return m, [("update", [0, 1, 2]), ("snap",), ("update", [2, 0, 1])], lambda r: [
        S(r, 1)[0] == ([[1, 15], [2, 17]], [[2, 17], [1, 15]]),   # 0's own map {1: 15}, then 2's AddConnection
        S(r, 1)[2] == ([[0, 17]], [[0, 17]]),                     # 1's AddConnection(2, 16) came before 2's own update
        S(r, 1)[1] == ([[0, 3], [2, 16]], [[2, 16]])]


def case_parent():
    m = CMap(8, kp_cap=128)
    m.link(0, 1, 20)
    m.link(0, 2, 25)
    m.link(1, 2, 15)
    m.see(3, 4, 7)
    m.see(3, 5, 2)
    m.first[:] = [1, 0, 1, 1, 0, 0, 0, 0]
    m.init[2] = 1
    m.parent[1] = 6
    return m, [("update", [0, 1, 2, 3])], lambda r: [
        r[0]["new_parent"] == [2, -1, -1, 4], r[-1]["parent"] == [2, 6, -1, 4, -1, -1, -1, -1],
        r[-1]["first"] == [0, 0, 1, 0, 0, 0, 0, 0]]


def case_capacity(n):
    """conn_cap 4: a counter of n entries, two of them listed."""
    m = CMap(8, kp_cap=128, conn_cap=4)
    m.see(0, 1, 15)
    m.see(0, 2, 16)
    for k in range(3, n + 1):
        m.see(0, k, 2)
    return m, [("update", [0])], lambda r: [r[0]["n_counted"] == [n]]


def case_append_fills_row():
    """conn_cap 4: keyframe 2 holds two entries; queries 0 and 1 of one call append one each."""
    m = CMap(8, kp_cap=128, conn_cap=4)
    m.link(2, 3, 15)
    m.link(2, 4, 3)
    m.see(0, 2, 16)
    m.see(1, 2, 17)
    return m, [("update", [2]), ("update", [0, 1])], lambda r: [
        S(r)[2] == ([[0, 16], [1, 17], [3, 15], [4, 3]], [[1, 17], [0, 16], [3, 15], [4, 3]])]


def case_scratch_histogram():
    """kf_cap one above PLVI_COVIS_LDS_KF: the histogram lives in the scratch block."""
    K = plvi.COVIS_LDS_KF + 1
    occ = [0, 1, 5, 63, 64, 4095, 4096, 8000, 8190, 8191, 8192, 77]
    m = CMap(K, kp_cap=128, conn_cap=16, slots=occ + [2, 8189])
    m.bad[:] = 1
    m.bad[occ] = 0
    m.order = occ[::-1]
    m.see(8192, 0, 15)
    m.see(8192, 8191, 15)
    m.see(8192, 4096, 40)
    m.see(8192, 77, 3)
    m.link(0, 8000, 16)
    return m, [("update", [8192, 0])], lambda r: [
        S(r)[8192] == ([[0, 15], [77, 3], [4096, 40], [8191, 15]], [[4096, 40], [0, 15], [8191, 15]]),
        S(r)[0][1] == [[8000, 16]], S(r)[0][0] == [[8000, 16]], r[0]["kf_max"] == [4096, 8000]]


def case_count_contract():
    """nmp one below, at and one above kp_cap; a negative count."""
    m = CMap(8, kp_cap=16)
    for q, k in ((0, 1), (2, 3), (4, 5), (6, 7)):
        m.see(q, k, 16)
    m.nmp[0], m.nmp[2], m.nmp[4], m.nmp[6] = 15, 16, 17, -3
    return m, [("update", [0, 2, 4, 6])], lambda r: [r[0]["w_max"] == [15, 16, 16, 0],
                                                     r[0]["n_counted"] == [1, 1, 1, 0]]


def case_long_table():
    """A keyframe table longer than one pass of the count kernel's workgroup, and `order` longer than one pass."""
    K = 600
    m = CMap(K, kp_cap=1100, n_mp=1200, conn_cap=8, slots=[0, 1, 2, 598, 599, 300])
    m.see(0, 1, 500)
    m.see(0, 599, 580)
    m.see(0, 598, 14)
    return m, [("update", [0])], lambda r: [S(r)[0][1] == [[599, 580], [1, 500]], r[0]["n_counted"] == [3],
                                            S(r)[599][1] == [[0, 580]]]


def case_erase():
    """A slot with neighbours; two mutually connected slots in one call; a slot that is nobody's neighbour."""
    m = CMap(12, kp_cap=200)
    for a, b, n in ((0, 1, 20), (0, 2, 16), (1, 2, 18), (3, 4, 15), (3, 0, 17), (4, 1, 19), (2, 5, 4)):
        m.link(a, b, n)
    m.see(6, 0, 15)        # 0 knows 6, 6 ... is updated too; 7 is alone
    return m, [("update", [0, 1, 2, 3, 4, 5, 6]), ("snap",), ("erase", [0]), ("snap",), ("erase", [3, 4]), ("snap",),
               ("erase", [7])], lambda r: [
        S(r, 1)[1][1] == [[0, 20], [4, 19], [2, 18]], S(r, 2)[0] == ([], []), S(r, 2)[1][1] == [[4, 19], [2, 18]],
        S(r, 2)[6] == ([], []),
        S(r, 3)[3] == S(r, 3)[4] == ([], []), S(r, 3)[1] == ([[2, 18]], [[2, 18]]), S(r)[7] == ([], []),
        r[-1]["covis"][7] == [-1] * NB, r[-1]["covis"][8] == [FILL] * NB]


def case_resort_clean():
    m = CMap(8, kp_cap=128)
    m.link(0, 1, 20)
    m.link(0, 2, 4)
    m.link(1, 2, 16)
    return m, [("update", [0, 1, 2]), ("snap",), ("resort", [1, 3])], lambda r: [
        S(r)[1] == S(r, 1)[1], S(r)[3] == ([], []), r[-1]["covis"][3] == [-1] * NB, r[1]["covis"][3] == [FILL] * NB]


def random_case(seed, K=None, kp_cap=200, big=False):
    """A general map and script: asymmetric and symmetric counts, bad keyframes and features, a shuffled `order`,
    empty slots, two maps, resident state from earlier updates, mutually neighbouring queries in both orders,
    erasures and bare re-sorts."""
    rng = np.random.default_rng(seed)
    K = K or int(rng.integers(3, 10))
    lines = seed % 2 == 1
    m = CMap(K, kp_cap, n_mp=K * kp_cap, kl_cap=3 * K if lines else 0, n_ml=2 * K * K if lines else 0)
    occ = [s for s in range(K) if rng.random() < 0.9] or [0]
    m.bad[:] = 1
    m.bad[occ] = 0
    m.order = rng.permutation(occ).tolist()
    if seed % 3 == 0:
        m.map_id = (rng.random(K) < 0.15).astype(np.int32).tolist()
    m.init[m.order[0]] = 1
    m.first[:] = rng.random(K) < 0.6
    weights = [1, 3, 14, 15, 16, 22]
    for a in range(K):
        for b in range(a + 1, K):
            mode = rng.integers(0, 4)
            if mode == 1:
                m.link(a, b, int(rng.choice(weights)))
            elif mode == 2:
                m.see(a, b, int(rng.choice(weights)))
                if rng.random() < 0.5:
                    m.see(b, a, int(rng.choice(weights)))
            if lines and rng.random() < 0.3:
                m.link_l(a, b, int(rng.integers(1, 4)))
    m.mp_bad[:m.next_mp] = rng.random(m.next_mp) < 0.03
    script = []
    for _ in range(5):
        k = rng.integers(0, 8)
        some = rng.permutation(K)[:int(rng.integers(1, K + 1))].tolist()
        if k < 4:
            script.append(("update", some))
            if rng.random() < 0.3:
                script.append(("update", some[::-1]))
        elif k == 4:
            script.append(("erase", some[:2]))
        elif k == 5:
            script.append(("resort", some))
        elif k == 6:
            s = int(rng.integers(0, K))
            script.append(("mut", lambda m, s=s: m.bad.__setitem__(s, 1 - m.bad[s])))
        else:
            p = int(rng.integers(0, max(m.next_mp, 1)))
            script.append(("mut", lambda m, p=p: m.mp_bad.__setitem__(p, 1)))
        if rng.random() < 0.4:
            script.append(("snap",))
    return m, script, lambda r: [True]


def big_random_case():
    """300 keyframes in 400 slots, about 8 observations a point, two batches of 64 queries that overlap."""
    rng = np.random.default_rng(77)
    K, n_kf, kp_cap, n_mp = 400, 300, 256, 7500
    m = CMap(K, kp_cap, n_mp, kl_cap=32, n_ml=600, conn_cap=128)
    occ = np.sort(rng.choice(K, n_kf, replace=False))
    m.bad[:] = 1
    m.bad[occ] = 0
    m.bad[occ[rng.choice(n_kf, 10, replace=False)]] = 1          # named keyframes that are bad
    m.order = rng.permutation(occ).tolist()
    m.first[:] = rng.random(K) < 0.5
    m.init[occ[0]] = 1
    for pool_n, obs, put, cnt, cap in ((n_mp, m.mp_obs, m.put, m.nmp, kp_cap), (600, m.ml_obs, m.put_line, m.nml, 32)):
        for i in range(pool_n):
            c = int(rng.integers(0, n_kf))
            kfs = occ[np.unique(np.clip(c + rng.integers(-8, 9, 9), 0, n_kf - 1))].tolist()
            obs[i] = kfs
            for s in kfs:
                if cnt[s] < cap and rng.random() < 0.9:          # an observer that does not hold the point: asymmetric
                    put(s, i)
    m.next_mp, m.next_ml = n_mp, 600
    m.mp_bad[:] = rng.random(n_mp) < 0.03
    q1 = rng.choice(occ, 64, replace=False).tolist()
    q2 = (q1[40:] + [int(s) for s in occ if s not in q1][:40])
    return m, [("update", q1), ("snap",), ("update", q2), ("erase", q1[:5]), ("resort", q2[:7])], lambda r: [
        min(r[0]["n_counted"]) > 5, max(r[0]["n_conn"]) > 8, sum(len(S(r)[s][1]) for s in range(K)) > 2000]


CASES = {
    "threshold": case_threshold, "none_at_15_tie": case_none_at_15_tie,
    "none_at_15_tie_permuted": lambda: case_none_at_15_tie(True), "empty_counter": case_empty_counter,
    "must_not_count": case_must_not_count, "id_twice": case_id_twice, "lines": case_lines,
    "points_only": lambda: case_lines(False), "equal_weights_by_rank": case_equal_weights_by_rank,
    "neighbour_lists": case_neighbour_lists,
    "batch_ab_sym": lambda: case_batch_pair([0, 1], True), "batch_ba_sym": lambda: case_batch_pair([1, 0], True),
    "batch_ab_asym": lambda: case_batch_pair([0, 1], False), "batch_ba_asym": lambda: case_batch_pair([1, 0], False),
    "cycle": case_cycle, "parent": case_parent, "capacity_below": lambda: case_capacity(3),
    "capacity_at": lambda: case_capacity(4), "append_fills_row": case_append_fills_row,
    "scratch_histogram": case_scratch_histogram, "count_contract": case_count_contract, "long_table": case_long_table,
    "erase": case_erase, "resort_clean": case_resort_clean,
    "random_a": lambda: random_case(1000, K=24, kp_cap=400), "random_b": lambda: random_case(1003, K=33, kp_cap=500),
}

_refs = {}


def ref_of(name):
    """The restatement's results of a case, computed once and shared."""
    if name not in _refs:
        m, script, check = (big_random_case if name == "big_random" else CASES[name])()
        _refs[name] = (RefRunner(m).run(script), check)
    return _refs[name]


def fresh(name):
    return (big_random_case if name == "big_random" else CASES[name])()


def same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.keys() == w.keys(), i
        for k in w:
            if k in ("state", "err"):
                for s in w[k]:
                    assert g[k][s] == w[k][s], (i, k, s)
            else:
                assert g[k] == w[k], (i, k)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_against_gather_formulation(name):
    ref, check = ref_of(name)
    m, script, _ = fresh(name)
    same(NpRunner(m).run(script), ref)
    assert all(check(ref)), check(ref)


@pytest.mark.parametrize("block", range(8))
def test_restatement_random_maps(block):
    """240 random maps of 3-9 keyframes."""
    for seed in range(30 * block, 30 * block + 30):
        m, script, _ = random_case(seed)
        ref = RefRunner(m).run(script)
        m, script, _ = random_case(seed)
        same(NpRunner(m).run(script), ref)


def test_restatement_big_random_map():
    ref, check = ref_of("big_random")
    m, script, _ = fresh("big_random")
    same(NpRunner(m).run(script), ref)
    assert all(check(ref)), check(ref)


def test_random_maps_cover_the_batch_rules():
    """What the random maps are there for: asymmetric counts, and mutually neighbouring queries in both orders."""
    asym = both = 0
    for seed in range(60):
        m, script, _ = random_case(seed)
        r = NpRunner(m)
        rank, named = r.rank()
        c = {s: r.counter(s, named) for s in range(m.K)}
        asym += any(c[a][b] != c[b][a] for a in range(m.K) for b in range(m.K))
        for op in script:
            if op[0] == "update":
                q = op[1]
                pairs = [(i, j) for i in range(len(q)) for j in range(len(q)) if i < j and c[q[i]][q[j]] >= 15 and
                         c[q[j]][q[i]] >= 15]
                both += bool(pairs) and any(q[i] > q[j] for i, j in pairs) and any(q[i] < q[j] for i, j in pairs)
    assert asym > 20 and both > 5


# ------------------------------------------------------------------ gpu

@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_equals_restatement(plvi_lib, name):
    """Every crafted case through plvi_covis_update_batch / _erase_batch / _resort_batch: every compared slot's map
    and list, the per-query outputs, first_conn, parent, the whole covis table and the error bits."""
    ref, _ = ref_of(name)
    m, script, _ = fresh(name)
    g = GpuRunner(m)
    same(g.run(script), ref)
    assert all(p == [FILL] * len(OUTS) for p in g.past)   # nothing written past the last query


@pytest.mark.gpu
def test_gpu_big_random_map(plvi_lib):
    ref, _ = ref_of("big_random")
    m, script, _ = fresh("big_random")
    same(GpuRunner(m).run(script), ref)


@pytest.mark.gpu
def test_gpu_capacity_above(plvi_lib):
    """A counter of conn_cap + 1 entries: the error bit of that slot and of that query alone, the outputs whole, the
    rows of the other slots as the restatement has them, nothing written past a row."""
    ref, _ = ref_of("capacity_at")
    m, script, _ = case_capacity(5)
    g = GpuRunner(m)
    got = g.run(script)
    assert got[0] == dict(ref[0], n_counted=[5], err=[1])
    assert got[-1]["err"] == {s: int(s == 0) for s in range(8)}
    for s in (1, 2):
        assert got[-1]["state"][s] == ref[-1]["state"][s]
    # an append beyond the row: two queries add themselves to a full neighbour
    m, script, _ = case_append_fills_row()
    m.see(5, 2, 18)
    g = GpuRunner(m)
    got = g.run([("update", [2]), ("update", [0, 1, 5])])
    assert got[-1]["err"][2] == 1 and got[1]["err"] == [0, 0, 0] and got[-1]["err"][0] == 0
    assert len(got[-1]["state"][2][0]) == 4


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["batch_ba_asym", "lines", "parent", "neighbour_lists", "empty_counter", "cycle"])
def test_gpu_host_form(plvi_lib, name):
    """plvi_covis_update, one keyframe from host tables, query by query."""
    ref, _ = ref_of(name)
    m, script, _ = fresh(name)
    same(GpuRunner(m, host_form=True).run(script), ref)


@pytest.mark.gpu
def test_gpu_getters(plvi_lib):
    ref, _ = ref_of("random_b")
    m, script, _ = fresh("random_b")
    r = RefRunner(m)
    r.run(script)
    m, script, _ = fresh("random_b")
    g = GpuRunner(m)
    g.run(script)
    lib = ref_lib()
    slots, ws = [], []
    for s in range(m.K):
        ow = [w for _, w in ref[-1]["state"][s][1]]
        # below the minimum, at an element's weight, between two, above the maximum; an empty list gets 15
        for w in sorted({15, *[x + d for x in ow for d in (-1, 0, 1)]}):
            slots.append(s)
            ws.append(w)
    assert any(not ref[-1]["state"][s][1] for s in range(m.K)) and len(ws) > 3 * m.K
    want = [lib.covis_ref_by_weight(r.h, s, w) for s, w in zip(slots, ws)]
    assert g.cov.by_weight(slots + [-1, m.K], ws + [0, 0]).tolist() == want + [0, 0]
    assert want == [sum(1 for _, x in ref[-1]["state"][s][1] if x >= w) for s, w in zip(slots, ws)]
    a, b = np.divmod(np.arange(m.K * m.K), m.K)
    want = [lib.covis_ref_weight(r.h, int(x), int(y)) for x, y in zip(a, b)]
    assert sum(1 for x in want if x) > m.K
    assert g.cov.weight(a.tolist() + [-1, 0], b.tolist() + [0, -1]).tolist() == want + [0, 0]
    # plvi_covis_rows: the ordered tables where they live
    kf, w, n = g.cov.rows()
    C = m.conn_cap
    cnt = plvi.download(n, np.zeros(m.K, np.int32))
    tab = plvi.download(kf, np.zeros((m.K, C), np.int32))
    for s in range(m.K):
        assert tab[s, :cnt[s]].tolist() == [k for k, _ in ref[-1]["state"][s][1]]


@pytest.mark.gpu
def test_gpu_graph_capture(plvi_lib):
    """The batch call under plvi_graph_capture_begin / end and one replay."""
    ref, _ = ref_of("batch_ba_asym")
    m, script, _ = fresh("batch_ba_asym")
    g = GpuRunner(m)
    step, fetch = g.cov.update_batch(script[0][1], fill=FILL, run=False)
    st = ctypes.c_void_p()
    assert plvi_lib.plvi_stream_create(ctypes.byref(st)) == 0
    rcs = []
    graph = plvi.StepGraph(lambda s: rcs.append(step(s)), st.value)
    assert rcs == [0]
    assert (fetch()["n_counted"] == FILL).all()   # captured, not run
    graph.launch()
    assert plvi_lib.plvi_stream_synchronize(st) == 0
    r = fetch()
    assert plain({k: r[k] for k in OUTS}) == ref[0]
    same([g.snapshot()], ref[-1:])
    del graph
    assert plvi_lib.plvi_stream_destroy(st) == 0


@pytest.mark.gpu
def test_gpu_refusals(plvi_lib):
    m, script, _ = fresh("lines")
    g = GpuRunner(m)
    cov = g.cov
    kf, mp, ml = cov._structs(lambda grp, k: cov.dev[(grp, k)].ptr)
    buf = plvi.DeviceBuffer(1 << 12)
    out = plvi.CovisOutputs(*[buf.ptr] * 6)
    sb = plvi.covis_scratch_bytes(2, m.K)
    scratch = plvi.DeviceBuffer(sb)
    V = ctypes.c_void_p

    def call(q=(0, 1), h=cov.h, kf=kf, mp=mp, ml=ml, out=out, scratch_ptr=scratch.ptr, bytes_=sb, n=None):
        qa = np.array(q, np.int32)
        r = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731
        return plvi_lib.plvi_covis_update_batch(h, len(qa) if n is None else n, tl._p(qa), r(kf), r(mp), r(ml), r(out),
                                                V(scratch_ptr), bytes_, None)

    def changed(s, **kw):
        c = type(s)()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(s), ctypes.sizeof(s))
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    before = g.snapshot()
    assert call(q=(), scratch_ptr=0, bytes_=0) == 0                    # no launch, nothing needed
    assert call(q=(0, m.K)) == E_BADARG and call(q=(-1,)) == E_BADARG  # a slot outside [0, kf_cap)
    assert call(q=(3, 1, 3)) == E_BADARG                               # a slot named twice
    assert call(n=-1) == E_BADARG and call(h=None) == E_BADARG
    assert call(kf=None) == E_BADARG and call(mp=None) == E_BADARG and call(out=None) == E_BADARG
    for field in ("n_order", "kp_cap", "kl_cap"):
        assert call(kf=changed(kf, **{field: -1})) == E_BADARG, field
    assert call(kf=changed(kf, kf_cap=m.K + 1)) == E_BADARG            # not the graph's
    for field in ("bad", "order", "mp", "nmp", "nml", "parent", "first_conn"):
        assert call(kf=changed(kf, **{field: None})) == E_BADARG, field
    assert call(mp=changed(mp, n=-1)) == E_BADARG and call(mp=changed(mp, obs_off=None)) == E_BADARG
    assert call(ml=changed(ml, bad=None)) == E_BADARG
    for field in OUTS:
        assert call(out=changed(out, **{field: None})) == E_BADARG, field
    assert call(scratch_ptr=0) == E_BADARG and call(bytes_=sb - 1) == E_BADARG
    assert call(q=[0] * 65536, bytes_=1 << 40) == E_CAPACITY
    assert plvi.covis_scratch_bytes(-1, 4) == 0 and plvi.covis_scratch_bytes(4, -1) == 0
    h = V()
    assert plvi_lib.plvi_covis_create(8, plvi.COVIS_MAX_CONN + 1, 0, ctypes.byref(h)) == E_CAPACITY
    assert plvi_lib.plvi_covis_create((1 << 24) + 1, 4, 0, ctypes.byref(h)) == E_CAPACITY
    assert plvi_lib.plvi_covis_create(0, 4, 0, ctypes.byref(h)) == E_BADARG
    assert plvi_lib.plvi_covis_create(8, 0, 0, ctypes.byref(h)) == E_BADARG
    assert plvi_lib.plvi_covis_create(8, 4, 0, None) == E_BADARG and plvi_lib.plvi_covis_destroy(None) == E_BADARG
    assert cov.erase([1, 1]) == E_BADARG and cov.erase([m.K]) == E_BADARG and cov.resort([-1]) == E_BADARG
    assert cov.erase([]) == 0 and cov.resort([]) == 0
    assert plvi_lib.plvi_covis_download(cov.h, m.K, None, None, None, None, None, None, None) == E_BADARG
    assert plvi_lib.plvi_covis_by_weight_batch(cov.h, 1, None, None, None, None) == E_BADARG
    assert plvi_lib.plvi_covis_weight_batch(cov.h, -1, None, None, None, None) == E_BADARG
    # the host form makes the same checks before it reads a table
    tabs = cov._tables()
    hkf, hmp, hml = cov._structs(lambda grp, k: tabs[(grp, k)].ctypes.data)
    z = np.zeros(8, np.int32)
    hout = plvi.CovisOutputs(*[z.ctypes.data] * 6)
    r = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731
    host = lambda slot=0, kf=hkf, mp=hmp, ml=hml, out=hout: plvi_lib.plvi_covis_update(cov.h, slot, r(kf), r(mp), r(ml), r(out))  # noqa: E731
    assert host(slot=m.K) == E_BADARG and host(slot=-1) == E_BADARG and host(kf=None) == E_BADARG
    assert host(kf=changed(hkf, nmp=None)) == E_BADARG and host(mp=changed(hmp, obs_kf=None)) == E_BADARG
    assert host(out=changed(hout, err=None)) == E_BADARG
    # nothing was launched by a refused call: the graph is as it was, and a good call still runs
    same([g.snapshot()], [before])
    assert call() == 0 and plvi_lib.plvi_device_synchronize() == 0
    # every optional table NULL: no parent rule, one map, no initial keyframe, no covis rows
    after = g.snapshot()
    bare = changed(kf, parent=None, first_conn=None, covis=None, init_kf=None, map_id=None)
    assert call(kf=bare) == 0 and plvi_lib.plvi_device_synchronize() == 0
    same([g.snapshot()], [after])            # the same queries again: nothing changes


@pytest.mark.gpu
def test_gpu_chain_to_local_map(plvi_lib):
    """A new keyframe's plvi_covis_update_batch writes covis and parent on the device; plvi_local_map_batch reads
    those same device tables.  Its outputs equal local_map_ref fed the restatement's tables."""
    rng = np.random.default_rng(5)
    K, kp_cap, n_mp = 40, 96, 1200
    m = CMap(K, kp_cap, n_mp, conn_cap=40)
    for i in range(n_mp):
        c = int(rng.integers(0, K))
        kfs = np.unique(np.clip(c + rng.integers(-3, 4, 5), 0, K - 1)).tolist()
        m.mp_obs[i] = kfs
        for s in kfs:
            if m.nmp[s] < kp_cap:
                m.put(s, i)
    m.next_mp = n_mp
    m.order = rng.permutation(K).tolist()
    m.first[:] = 1
    m.init[0] = 1
    m.first[0] = 0
    script = [("update", list(range(K - 1))), ("update", [K - 1])]      # the map, then the new keyframe
    ref = RefRunner(m)
    rr = ref.run(script)
    g = GpuRunner(m)
    same(g.run(script), rr)
    assert rr[1]["new_parent"][0] >= 0 and sum(1 for x in rr[-1]["covis"][K - 1] if x >= 0) > 3

    # the local map of a frame that votes around the new keyframe, from the device tables covis wrote
    kf, mp, _ = m.tables()
    kf.update(covis=np.full((K, NB), -1, np.int32), parent=np.full(K, -1, np.int32))
    lm = plvi.LocalMap(kf, mp)
    lm.upload()
    lm.dev[("kf", "covis")], lm.dev[("kf", "parent")] = g.cov.dev[("kf", "covis")], g.cov.dev[("kf", "parent")]
    frames = [tl.frame(m.kf_mp[K - 1, :m.nmp[K - 1]].tolist()), tl.frame(m.kf_mp[3, :m.nmp[3]].tolist())]
    args = tl.gpu_args(frames)
    got = lm.update_batch(**args, lkf_cap=K, lmp_cap=n_mp, fill=tl.FILL)
    bare = [tl.ref_frame(m, fr)["local_kf"] for fr in frames]
    m.covis[:] = np.array(rr[-1]["covis"], np.int32)
    m.parent[:] = rr[-1]["parent"]
    refs = [tl.ref_frame(m, fr) for fr in frames]
    assert all(r["local_kf"] != b for r, b in zip(refs, bare))   # the two tables decide the expansion
    tl.compare(got, tl.expected(lm, m, frames, refs, [K, n_mp, 0]), frames, refs, args)
