"""Tracking::UpdateLocalMap / UpdateLocalMapWithLines on the device (csrc/local_map.hip, plvi_local_map[_batch]):
UpdateLocalKeyFrames[WithLines] (src/Tracking.cc:5399-5551 / :5553-5745), UpdateLocalPoints[AndLines] (:5325-5352 /
:5354-5397) and the in_flags of the first loop of SearchLocalPoints[AndLines] (:5052-5069 / :5126-5161).

Expected values come from tests/native/local_map_ref.cpp, a sequential host restatement in the reference's own shape
(objects, a std::map<KF*, int> iterated by address, std::set children, a reserved std::vector walked by an end
iterator taken before the loop, the two stamps).  The CPU part pins it against np_frame below, an independent
restatement in the FORWARD formulation -- a bincount vote, an index loop over a copy of K1, np.unique first
occurrences over the flattened reverse walk, np.isin for the seen-set -- on every crafted case and on random maps,
and checks what each crafted case is there to show.  The gpu part demands exact equality with the restatement for
every output: the lists, the full counts, ref_kf, the vote tables written back, every gathered row and err, with
sentinel-filled outputs so that nothing is written past a count or a capacity."""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import plvi

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "local_map_ref.cpp"
BUILD = ROOT / "tests" / "native" / "_build"
FILL = -7
E_BADARG, E_CAPACITY = -2, -3

_lib = None


def ref_lib():
    global _lib
    if _lib is None:
        so = BUILD / "liblocal_map_ref.so"
        if not so.exists() or so.stat().st_mtime < SRC.stat().st_mtime:
            so.parent.mkdir(parents=True, exist_ok=True)
            subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", str(so),
                            str(SRC)], check=True)
        _lib = ctypes.CDLL(str(so))
        V, I = ctypes.c_void_p, ctypes.c_int
        _lib.local_map_ref.argtypes = [I, V, V, I, V, V, V, V, V, V, V, I, V, V, I,
                                       I, V, V, V, I, V, V, V, V, I, V, I, V, I, V, I, I] + [V] * 9
        _lib.local_map_ref.restype = I
        _lib.local_map_ref_seconds.argtypes, _lib.local_map_ref_seconds.restype = [], ctypes.c_double
    return _lib


_EMPTY = np.zeros(1, np.int32)


def _p(a):
    """NULL for None; an empty table is a valid pointer with count 0."""
    return None if a is None else ctypes.c_void_p((a if a.size else _EMPTY).ctypes.data)


def csr(lists):
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in lists])
    return off, np.array([v for x in lists for v in x] + [0], np.int32)


class Map:
    """A small map: keyframes by slot, a MapPoint pool and (kl_cap > 0) a MapLine pool."""

    def __init__(self, K, kp_cap=8, n_mp=64, kl_cap=0, n_ml=0, imu=False):
        self.K, self.kp_cap, self.kl_cap = K, kp_cap, kl_cap
        self.bad = np.zeros(K, np.uint8)
        self.order = list(range(K))
        self.covis = np.full((K, 10), -1, np.int32)
        self.children = [[] for _ in range(K)]
        self.parent = np.full(K, -1, np.int32)
        self.prev = np.full(K, -1, np.int32) if imu else None
        self.kf_mp, self.nmp = np.full((K, kp_cap), -1, np.int32), np.zeros(K, np.int32)
        self.kf_ml, self.nml = np.full((K, kl_cap), -1, np.int32), np.zeros(K, np.int32)
        self.mp_bad, self.mp_obs, self.next_mp = np.zeros(n_mp, np.uint8), [[] for _ in range(n_mp)], 0
        self.ml_bad, self.ml_obs, self.next_ml = np.zeros(n_ml, np.uint8), [[] for _ in range(n_ml)], 0
        self.null_gathers = ()

    def point(self, *kfs):
        """A new MapPoint observed from kfs (observations only)."""
        i = self.next_mp
        self.next_mp += 1
        self.mp_obs[i] = list(kfs)
        return i

    def line(self, *kfs):
        i = self.next_ml
        self.next_ml += 1
        self.ml_obs[i] = list(kfs)
        return i

    def votes(self, counts):
        """Fresh points, counts[kf] of them observing kf alone."""
        return [self.point(kf) for kf, c in counts.items() for _ in range(c)]

    def put(self, kf, *ids):
        """Append ids to the keyframe's GetMapPointMatches()."""
        for i in ids:
            self.kf_mp[kf, self.nmp[kf]] = i
            self.nmp[kf] += 1

    def put_line(self, kf, *ids):
        for i in ids:
            self.kf_ml[kf, self.nml[kf]] = i
            self.nml[kf] += 1

    def tree(self, parent, *children):
        for c in children:
            self.parent[c] = parent
            self.children[parent].append(c)

    def rank(self):
        r = {}
        for s in self.order:
            if 0 <= s < self.K and s not in r:
                r[s] = len(r)
        return r

    def tables(self):
        """The dicts plvi.LocalMap takes.  Children in std::set<KeyFrame*> order = by the rank of `order`."""
        r = self.rank()
        kids = [sorted(c, key=lambda s: r.get(s, len(r) + s)) for c in self.children]
        coff, cidx = csr(kids)
        kf = dict(bad=self.bad, order=np.array(self.order, np.int32), covis=self.covis, child_off=coff, child=cidx,
                  parent=self.parent, prev_kf=self.prev, mp=self.kf_mp, nmp=self.nmp)
        if self.kl_cap:
            kf.update(ml=self.kf_ml, nml=self.nml)

        def pool(bad, obs, lines):
            n = len(bad)
            off, idx = csr(obs)
            i = np.arange(n)
            p = dict(bad=bad, obs_off=off, obs_kf=idx,
                     normal=np.stack([i + 0.25, -i - 0.5, i * 0.125], 1).astype(np.float32),
                     dist=np.stack([i * 0.5 + 1, i * 2.0 + 3], 1).astype(np.float32),
                     desc=((i[:, None] * 7 + np.arange(32)[None] * 3 + lines) % 251).astype(np.uint8))
            if lines:
                p["sep"] = (i[:, None] * 6 + np.arange(6)[None] + 0.001).astype(np.float64)
            else:
                p["pos"] = (i[:, None] * 3 + np.arange(3)[None] + 0.5).astype(np.float32)
            for k in self.null_gathers:
                p.pop(k, None)
            return p
        return kf, pool(self.mp_bad, self.mp_obs, 0), (pool(self.ml_bad, self.ml_obs, 1) if self.kl_cap else None)


def frame(vote_mp=(), vote_ml=None, seen_mp=None, seen_ml=None, last_kf=-1, n_vote_mp=None, n_vote_ml=None,
          n_seen_mp=None, n_seen_ml=None):
    return dict(vote_mp=list(vote_mp), vote_ml=None if vote_ml is None else list(vote_ml),
                seen_mp=None if seen_mp is None else list(seen_mp), seen_ml=None if seen_ml is None else list(seen_ml),
                last_kf=last_kf, n_vote_mp=n_vote_mp, n_vote_ml=n_vote_ml, n_seen_mp=n_seen_mp, n_seen_ml=n_seen_ml)


def clamped(fr, name):
    """The table as the count contract reads it (None stays None)."""
    t = fr[name]
    if t is None:
        return None
    n = len(t) if fr["n_" + name] is None else max(min(fr["n_" + name], len(t)), 0)
    return np.array(t[:n], np.int32)


def ref_frame(m, fr):
    """tests/native/local_map_ref.cpp on one frame."""
    kf, mp, ml = m.tables()
    lines = ml is not None
    K, nm, nl = m.K, len(mp["bad"]), len(ml["bad"]) if lines else 0
    a = {k: (None if v is None else np.ascontiguousarray(v, np.uint8 if k == "bad" else np.int32))
         for k, v in kf.items()}
    pm = {k: np.ascontiguousarray(mp[k]) for k in ("bad", "obs_off", "obs_kf")}
    pl = {k: np.ascontiguousarray(ml[k]) for k in ("bad", "obs_off", "obs_kf")} if lines else {}
    vm, vl = clamped(fr, "vote_mp"), clamped(fr, "vote_ml")
    sm, sl = clamped(fr, "seen_mp"), clamped(fr, "seen_ml")
    lkf, lmp, lml = np.zeros(K + 1, np.int32), np.zeros(nm + 1, np.int32), np.zeros(nl + 1, np.int32)
    fm, fl = np.zeros(nm + 1, np.uint8), np.zeros(nl + 1, np.uint8)
    c = [ctypes.c_int() for _ in range(4)]
    ln = lambda t: 0 if t is None else len(t)  # noqa: E731
    realloc = ref_lib().local_map_ref(
        K, _p(a["bad"]), _p(a["order"]), len(a["order"]), _p(a["covis"]), _p(a["child_off"]), _p(a["child"]),
        _p(a["parent"]), _p(a["prev_kf"]), _p(a["mp"]), _p(a["nmp"]), m.kp_cap, _p(a.get("ml")), _p(a.get("nml")),
        m.kl_cap, nm, _p(pm["bad"]), _p(pm["obs_off"]), _p(pm["obs_kf"]), nl, _p(pl.get("bad")),
        _p(pl.get("obs_off")), _p(pl.get("obs_kf")), _p(vm), ln(vm), _p(vl), ln(vl), _p(sm), ln(sm), _p(sl), ln(sl),
        fr["last_kf"], _p(lkf), ctypes.byref(c[0]), ctypes.byref(c[1]), _p(lmp), ctypes.byref(c[2]), _p(fm), _p(lml),
        ctypes.byref(c[3]), _p(fl))
    assert realloc == 0, "the reserve of :5453 must keep the iterators of :5474 valid"
    nk, ref, npnt, nlin = (x.value for x in c)
    return dict(local_kf=lkf[:nk].tolist(), ref_kf=ref, local_mp=lmp[:npnt].tolist(), mp_flags=fm[:npnt].tolist(),
                local_ml=lml[:nlin].tolist(), ml_flags=fl[:nlin].tolist(), vote_mp=vm, vote_ml=vl)


def np_frame(m, fr):
    """The independent restatement, forward formulation."""
    kf, mp, ml = m.tables()
    lines = ml is not None
    K = m.K
    pools = [(mp, clamped(fr, "vote_mp"), clamped(fr, "seen_mp"), m.kf_mp, m.nmp, m.kp_cap)]
    if lines:
        pools.append((ml, clamped(fr, "vote_ml"), clamped(fr, "seen_ml"), m.kf_ml, m.nml, m.kl_cap))
    count = np.zeros(K, np.int64)
    votes_out = []
    for p, vote, _, _, _, _ in pools:
        if vote is None:
            votes_out.append(None)
            continue
        vote = vote.copy()
        valid = (vote >= 0) & (vote < len(p["bad"]))
        isbad = valid & (p["bad"][np.where(valid, vote, 0)] != 0)
        for i in vote[valid & ~isbad]:
            o = p["obs_kf"][p["obs_off"][i]:p["obs_off"][i + 1]]
            count += np.bincount(o[(o >= 0) & (o < K)], minlength=K)
        vote[isbad] = -1
        votes_out.append(vote)
    order = [s for s in dict.fromkeys(m.order) if 0 <= s < K]
    k1 = [s for s in order if count[s] > 0 and not m.bad[s]]
    ref = k1[int(np.argmax(count[k1]))] if k1 else -1   # argmax: the first of the largest
    local, listed = list(k1), set(k1)
    r = m.rank()
    for i in range(len(k1)):
        if len(local) > 80:
            break
        s = k1[i]
        cov = m.covis[s].tolist()
        cov = cov[:cov.index(-1)] if -1 in cov else cov
        nb = next((c for c in cov if c < K and not m.bad[c] and c not in listed), None)
        if nb is not None:
            local.append(nb)
            listed.add(nb)
        kids = sorted(set(m.children[s]), key=lambda c: r.get(c, len(r) + c))
        ch = next((c for c in kids if not m.bad[c] and c not in listed), None)
        if ch is not None:
            local.append(ch)
            listed.add(ch)
        par = int(m.parent[s])
        if par >= 0 and par not in listed:
            local.append(par)
            listed.add(par)
            break
    if fr["last_kf"] >= 0 and m.prev is not None and len(local) < 80:
        t = fr["last_kf"]
        for _ in range(20):
            if t < 0 or t in listed:
                break
            local.append(t)
            listed.add(t)
            t = int(m.prev[t])
    res = dict(local_kf=local, ref_kf=ref, vote_mp=votes_out[0], vote_ml=votes_out[1] if lines else None,
               local_ml=[], ml_flags=[])
    for (p, vote, seen, tab, cnt, cap), key, vout in zip(pools, ("mp", "ml"), votes_out):
        walk = [tab[s, :max(min(int(cnt[s]), cap), 0)] for s in reversed(local)]
        flat = np.concatenate(walk) if walk else np.zeros(0, np.int32)
        flat = flat[(flat >= 0) & (flat < len(p["bad"]))]
        flat = flat[p["bad"][flat] == 0]
        _, first = np.unique(flat, return_index=True)
        ids = flat[np.sort(first)]
        s = vout if seen is None else seen
        s = np.zeros(0, np.int32) if s is None else s
        s = s[(s >= 0) & (s < len(p["bad"]))]
        s = s[p["bad"][s] == 0]
        unseen = ~np.isin(ids, s)
        has_obs = (p["obs_off"][ids + 1] - p["obs_off"][ids]) > 0
        res["local_" + key] = ids.tolist()
        res[key + "_flags"] = (unseen.astype(int) | has_obs.astype(int) << 1).tolist()
    return res


# ------------------------------------------------------------------ crafted cases
# Each returns (map, frames, check) -- check(results of the restatement, one per frame) asserts what the case shows.

def case_no_votes():
    m = Map(8)
    m.put(0, m.point(0))
    return m, [frame([]), frame([-1, -1])], lambda r: [x["local_kf"] == [] and x["ref_kf"] == -1 and
                                                       x["local_mp"] == [] for x in r]


def case_bad_kf_most_votes():
    m = Map(8)
    v = m.votes({2: 5, 4: 3, 6: 1})
    m.bad[2] = 1   # :5460: skipped although it holds the most votes
    return m, [frame(v)], lambda r: [r[0]["ref_kf"] == 4 and 2 not in r[0]["local_kf"]]


def case_tie_first_in_order(perm=False):
    m = Map(8)
    v = m.votes({1: 3, 5: 3, 6: 2})
    if perm:
        m.order = [7, 6, 5, 4, 3, 2, 1, 0]
    return m, [frame(v)], lambda r: [r[0]["ref_kf"] == (5 if perm else 1),
                                     r[0]["local_kf"] == ([6, 5, 1] if perm else [1, 5, 6])]


def case_k1(n):
    """K1 of n keyframes, every member with an unlisted covisible: the expansion runs while size() <= 80."""
    m = Map(256, kp_cap=2)
    v = [m.point(*range(n))]
    for i in range(n):
        m.covis[i, 0] = 128 + i
    want = {79: 81, 80: 81, 81: 81, 100: 100}[n]
    return m, [frame(v)], lambda r: [len(r[0]["local_kf"]) == want, r[0]["local_kf"][:n] == list(range(n))]


def case_covis_second_taken():
    m = Map(16)
    v = m.votes({0: 2, 1: 1})
    m.bad[9] = 1
    m.covis[0, :3] = [9, 1, 10]    # bad, listed (K1), taken
    m.covis[1, :3] = [10, 0, 11]   # listed by now, listed, taken
    return m, [frame(v)], lambda r: [r[0]["local_kf"] == [0, 1, 10, 11]]


def case_covis_all_listed():
    m = Map(16)
    v = [m.point(*range(11))]
    m.covis[0] = np.arange(1, 11)
    return m, [frame(v)], lambda r: [r[0]["local_kf"] == list(range(11))]


def case_child_set_order():
    m = Map(16)
    v = m.votes({0: 1})
    m.order = [0, 9, 7, 8] + [s for s in range(16) if s not in (0, 7, 8, 9)]
    m.tree(0, 7, 8, 9)     # std::set order is by address: 9 first
    return m, [frame(v)], lambda r: [r[0]["local_kf"] == [0, 9]]


def case_bad_parent_added():
    m = Map(8)
    v = m.votes({3: 1})
    m.tree(5, 3)
    m.bad[5] = 1           # :5514-5523 has no isBad()
    return m, [frame(v)], lambda r: [r[0]["local_kf"] == [3, 5]]


def case_parent_breaks_outer():
    m = Map(32)
    v = m.votes({0: 1, 1: 1, 2: 1, 3: 1, 4: 1})
    for i in range(5):
        m.covis[i, 0] = 10 + i
    m.tree(20, 2)          # the third K1 member has a parent: :5521 leaves the outer loop
    return m, [frame(v)], lambda r: [r[0]["local_kf"] == [0, 1, 2, 3, 4, 10, 11, 12, 20]]


def case_parent_listed_goes_on():
    m = Map(32)
    v = m.votes({0: 1, 1: 1, 2: 1})
    for i in range(3):
        m.covis[i, 0] = 10 + i
    m.tree(0, 1)           # the parent is a K1 member: no break
    return m, [frame(v)], lambda r: [r[0]["local_kf"] == [0, 1, 2, 10, 11, 12]]


def case_temporal_ends():
    m = Map(16, imu=True)
    v = m.votes({0: 1})
    m.prev[5], m.prev[4] = 4, 3
    return m, [frame(v, last_kf=5)], lambda r: [r[0]["local_kf"] == [0, 5, 4, 3]]


def case_temporal_listed_at_once():
    m = Map(16, imu=True)
    v = m.votes({0: 1})
    m.prev[0] = 1
    return m, [frame(v, last_kf=0)], lambda r: [r[0]["local_kf"] == [0]]


def case_temporal_20():
    m = Map(64, imu=True)
    v = m.votes({0: 1})
    for s in range(40, 10, -1):
        m.prev[s] = s - 1
    return m, [frame(v, last_kf=40)], lambda r: [r[0]["local_kf"] == [0] + list(range(40, 20, -1))]


def case_temporal_at(n):
    """The list at n entries when the temporal loop is reached: it runs below 80 only (:5527)."""
    m = Map(256, kp_cap=2, imu=True)
    v = [m.point(*range(n))]
    m.prev[200] = 201
    want = n + 2 if n < 80 else n
    return m, [frame(v, last_kf=200)], lambda r: [len(r[0]["local_kf"]) == want]


def case_point_once_reverse():
    m = Map(8)
    v = m.votes({0: 1, 1: 1, 2: 1})
    a, b, c, d = (m.point(0) for _ in range(4))
    m.put(0, a, b)
    m.put(1, b, c, a)
    m.put(2, d, c)
    # the walk is 2, 1, 0: d c | b a
    return m, [frame(v)], lambda r: [r[0]["local_mp"] == [d, c, b, a]]


def case_bad_point_in_table():
    m = Map(8)
    v = m.votes({0: 1})
    a, b, c = (m.point(0) for _ in range(3))
    m.put(0, a, b, -1, c)
    m.mp_bad[b] = 1
    return m, [frame(v)], lambda r: [r[0]["local_mp"] == [a, c]]


def case_bad_vote_cleared():
    m = Map(8)
    g = m.votes({0: 1, 1: 2})
    b = m.votes({3: 4})
    m.mp_bad[b] = 1
    v = [g[0], b[0], -1, g[1], b[1], g[2], b[2], b[3]]
    return m, [frame(v)], lambda r: [r[0]["ref_kf"] == 1 and r[0]["local_kf"] == [0, 1],
                                     r[0]["vote_mp"].tolist() == [g[0], -1, -1, g[1], -1, g[2], -1, -1]]


def case_seen_distinct():
    m = Map(8)
    v = m.votes({0: 1})
    a, b, c = (m.point(0) for _ in range(3))
    m.put(0, a, b, c, v[0])
    # the vote table is mLastFrame's (:5425); the current frame has seen b only
    return m, [frame(v, seen_mp=[b, -1]), frame(v, seen_mp=v)], lambda r: [r[0]["mp_flags"] == [3, 2, 3, 3],
                                                                  r[1]["mp_flags"] == [3, 3, 3, 2]]


def case_empty_obs_bit1():
    m = Map(8)
    v = m.votes({0: 1})
    a, b = m.point(0), m.point()
    m.put(0, a, b)
    return m, [frame(v)], lambda r: [r[0]["mp_flags"] == [3, 1]]


def case_lines(with_lines=True):
    """Lines vote into the same counter (:5576-5592) and move pKFmax; the point-only form ignores them."""
    m = Map(8, kl_cap=4 if with_lines else 0, n_ml=16 if with_lines else 0)
    v = m.votes({0: 3, 1: 2})
    m.put(0, m.point(0))
    m.put(1, m.point(1))
    lv = None
    if with_lines:
        lv = [m.line(1), m.line(1, 2), -1]
        bad = m.line(0)
        m.ml_bad[bad] = 1
        lv.append(bad)
        la, lb = m.line(1), m.line()
        m.put_line(1, la, lb)
        m.put_line(2, lb, lv[0])
    want = dict(ref_kf=1, local_kf=[0, 1, 2]) if with_lines else dict(ref_kf=0, local_kf=[0, 1])
    return m, [frame(v, vote_ml=lv)], lambda r: [all(r[0][k] == w for k, w in want.items()),
                                                 not with_lines or (r[0]["local_ml"] == [lb, lv[0], la] and
                                                                    r[0]["ml_flags"] == [1, 2, 3] and
                                                                    r[0]["vote_ml"].tolist() == lv[:3] + [-1])]


def case_count_contract():
    """Counts outside [0, cap] are read as clamped; rows past the clamped count are not read (a bad id there stays).
    Every count -- nmp, nml, n_vote_mp, n_vote_ml, n_seen_mp, n_seen_ml -- takes a negative value, one inside and
    one above its capacity; the fourth frame has the negative n_vote_mp: no point votes, its vote table comes back
    untouched (the bad id in it too), and ref_kf / local_kf come from the two line votes alone."""
    m = Map(8, kl_cap=4, n_ml=16)
    v = m.votes({0: 1, 1: 2})
    b = m.votes({2: 9})
    m.mp_bad[b[0]] = 1
    a, c = m.point(0), m.point(1)
    m.put(0, a, c)
    m.put(1, c)
    m.nmp[0], m.nmp[1], m.nmp[2] = 99, 1, -5     # above capacity, inside, negative
    m.kf_mp[0, 2:] = [a, c, b[1], a, a, a][:m.kp_cap - 2]
    x, y, z = [m.line(0) for _ in range(2)], [m.line(1) for _ in range(3)], [m.line(2) for _ in range(4)]
    m.put_line(0, *x)
    m.put_line(1, *y)
    m.put_line(2, *z)
    m.nml[0], m.nml[1], m.nml[2] = -1, 2, 99     # negative, inside (y[2] is not read), above capacity
    lv = [m.line(2), m.line(0)]
    vm, sm, sl = v + [b[0]], [a, c], [y[0], z[1]]
    walk = z + y[:2]                             # keyframes 2, 1, 0 in reverse; keyframe 0's lines are not read
    return m, [frame(vm, n_vote_mp=3, vote_ml=lv, n_vote_ml=7, seen_mp=sm, n_seen_mp=-2, seen_ml=sl, n_seen_ml=-2),
               frame(vm, n_vote_mp=1000, vote_ml=lv, n_vote_ml=-3, seen_mp=sm, n_seen_mp=1, seen_ml=sl, n_seen_ml=1),
               frame(vm, n_vote_mp=2, vote_ml=lv, n_vote_ml=1, seen_mp=sm, n_seen_mp=77, seen_ml=sl, n_seen_ml=50),
               frame(vm, n_vote_mp=-4, vote_ml=lv, n_vote_ml=2, seen_mp=sm, n_seen_mp=2, seen_ml=sl, n_seen_ml=2)], \
        lambda r: [r[0]["vote_mp"].tolist() == v, r[1]["vote_mp"].tolist() == v + [-1],
                   r[2]["vote_mp"].tolist() == v[:2],
                   [len(x["vote_ml"]) for x in r] == [2, 0, 1, 2],
                   r[0]["local_kf"] == [0, 1, 2], r[1]["local_kf"] == [0, 1], r[2]["local_kf"] == [0, 1, 2],
                   r[0]["local_mp"][:2] == [c, a], r[0]["mp_flags"][:2] == [3, 3], r[1]["mp_flags"][:2] == [3, 2],
                   r[2]["mp_flags"][:2] == [2, 2],
                   r[0]["local_ml"] == walk, r[0]["ml_flags"] == [3] * 6,
                   r[1]["local_ml"] == y[:2], r[1]["ml_flags"] == [2, 3],
                   r[2]["local_ml"] == walk, r[2]["ml_flags"] == [3, 2, 3, 3, 2, 3],
                   r[3]["vote_mp"].tolist() == [], r[3]["vote_ml"].tolist() == lv,
                   r[3]["local_kf"] == [0, 2], r[3]["ref_kf"] == 0,
                   r[3]["local_mp"] == [a, c, b[1]], r[3]["mp_flags"] == [2, 2, 3],
                   r[3]["local_ml"] == z, r[3]["ml_flags"] == [3, 2, 3, 3]]


def case_seen_ml_distinct():
    """The line side of seen_distinct: ml_in_flags bit0 follows seen_ml, not vote_ml, where the two differ."""
    m = Map(8, kl_cap=4, n_ml=8)
    v = m.votes({0: 1})
    la, lb, lc = (m.line(0) for _ in range(3))
    m.put_line(0, la, lb, lc)
    m.put(0, v[0])
    return m, [frame(v, vote_ml=[la], seen_ml=[lb, -1]), frame(v, vote_ml=[la], seen_ml=[la])], \
        lambda r: [r[0]["local_ml"] == [la, lb, lc], r[0]["ml_flags"] == [3, 2, 3], r[1]["ml_flags"] == [2, 3, 3],
                   r[0]["mp_flags"] == [2], r[0]["vote_ml"].tolist() == [la]]


def case_order_outside():
    m = Map(8)
    v = m.votes({0: 1, 3: 2})
    m.order = [-4, 3, 99, 0, 8]
    return m, [frame(v)], lambda r: [r[0]["local_kf"] == [3, 0] and r[0]["ref_kf"] == 3]


def random_map(seed, K=96, kp_cap=24, n_mp=700, kl_cap=0, n_ml=0, imu=True):
    """A general map: a spanning tree, covisibles, a temporal chain, bad keyframes and features, NULL entries."""
    rng = np.random.default_rng(seed)
    m = Map(K, kp_cap, n_mp, kl_cap, n_ml, imu)
    m.order = rng.permutation(K).tolist()
    m.bad[:] = rng.random(K) < 0.08
    for s in range(1, K):
        m.tree(int(rng.integers(0, s)), s)
    for s in range(K):
        n = int(rng.integers(0, 11))
        m.covis[s, :n] = rng.choice(K, n, replace=False)
    if imu:
        m.prev[1:] = np.arange(K - 1)
    for pool_n, obs, put, bad in ((n_mp, m.mp_obs, m.put, m.mp_bad), (n_ml, m.ml_obs, m.put_line, m.ml_bad)):
        if not pool_n:
            continue
        bad[:] = rng.random(pool_n) < 0.05
        cnt = m.nmp if put == m.put else m.nml
        cap = kp_cap if put == m.put else kl_cap
        for i in range(pool_n):
            c = int(rng.integers(0, K))
            kfs = np.unique(np.clip(c + rng.integers(-6, 7, int(rng.integers(0, 9))), 0, K - 1)).tolist()
            obs[i] = kfs
            for s in kfs:
                if cnt[s] < cap:
                    put(s, -1 if rng.random() < 0.05 else i)
    m.next_mp, m.next_ml = n_mp, n_ml
    return m, rng


def random_frames(m, rng, B):
    frames = []
    for _ in range(B):
        c = int(rng.integers(0, m.K))
        near = [i for i, o in enumerate(m.mp_obs) if any(abs(s - c) < 5 for s in o)]
        v = rng.choice(near, min(len(near), 60), replace=False).tolist() + [-1, -1]
        lv = None
        if m.kl_cap:
            nearl = [i for i, o in enumerate(m.ml_obs) if any(abs(s - c) < 5 for s in o)]
            lv = rng.choice(nearl, min(len(nearl), 20), replace=False).tolist() + [-1]
        frames.append(frame(v, vote_ml=lv, last_kf=c if rng.random() < 0.7 else -1))
    return frames


def case_random(seed, lines=False):
    m, rng = random_map(seed, kl_cap=8 if lines else 0, n_ml=200 if lines else 0)
    fr = random_frames(m, rng, 3)
    return m, fr, lambda r: [len(x["local_kf"]) > 10 and len(x["local_mp"]) > 50 for x in r] + \
        [sorted(a["local_kf"]) != sorted(b["local_kf"]) for a, b in zip(r, r[1:])]


def case_lds_bound():
    """kf_cap above PLVI_LOCAL_MAP_LDS_KF: the histogram and the listed-set live in global scratch."""
    K = plvi.LOCAL_MAP_LDS_KF + 9
    m = Map(K, kp_cap=2, n_mp=64)
    v = m.votes({K - 1: 2, 5: 1, K - 3: 3})
    m.covis[K - 3, 0] = K - 2
    m.tree(8195, 5)        # the first K1 member has an unlisted parent: added, and the loop ends
    a, b = m.point(K - 1), m.point(5)
    m.put(K - 1, a, b)
    m.put(K - 2, b)
    return m, [frame(v)], lambda r: [r[0]["local_kf"] == [5, K - 3, K - 1, 8195] and r[0]["ref_kf"] == K - 3]


def case_many_groups():
    """kf_cap * kp_cap = 16 workgroups' worth; a point's first occurrence and a later duplicate lie in different
    workgroups of the list passes (the first and the last keyframe of the walk)."""
    K, cap = 256, 128
    m = Map(K, kp_cap=cap, n_mp=4096)
    n = 40
    v = [m.point(*range(n))]
    shared = m.point(0)
    for s in range(n):
        ids = [m.point(s) for _ in range(60)]
        m.put(s, *ids[:30], shared, *ids[30:], ids[3])
    groups = -(-K * cap // plvi.LOCAL_MAP_GROUP_ENTRIES)
    chunk = -(-n * cap // groups)

    def check(r):
        walk_pos = lambda kf: (n - 1 - kf) * cap + 30  # noqa: E731
        return [groups == 16, walk_pos(n - 1) // chunk == 0, walk_pos(0) // chunk == groups - 1,
                r[0]["local_mp"].count(shared) == 1, r[0]["local_mp"].index(shared) == 30,
                len(r[0]["local_mp"]) == n * 60 + 1]
    return m, [frame(v)], check


CASES = {
    "no_votes": case_no_votes, "bad_kf_most_votes": case_bad_kf_most_votes,
    "tie_first_in_order": case_tie_first_in_order, "tie_permuted_order": lambda: case_tie_first_in_order(True),
    "k1_79": lambda: case_k1(79), "k1_80": lambda: case_k1(80), "k1_81": lambda: case_k1(81),
    "k1_100": lambda: case_k1(100), "covis_second_taken": case_covis_second_taken,
    "covis_all_listed": case_covis_all_listed, "child_set_order": case_child_set_order,
    "bad_parent_added": case_bad_parent_added, "parent_breaks_outer": case_parent_breaks_outer,
    "parent_listed_goes_on": case_parent_listed_goes_on, "temporal_ends": case_temporal_ends,
    "temporal_listed_at_once": case_temporal_listed_at_once, "temporal_20": case_temporal_20,
    "temporal_at_79": lambda: case_temporal_at(79), "temporal_at_80": lambda: case_temporal_at(80),
    "point_once_reverse": case_point_once_reverse, "bad_point_in_table": case_bad_point_in_table,
    "bad_vote_cleared": case_bad_vote_cleared, "seen_distinct": case_seen_distinct,
    "empty_obs_bit1": case_empty_obs_bit1, "seen_ml_distinct": case_seen_ml_distinct, "lines": case_lines,
    "points_only": lambda: case_lines(False),
    "count_contract": case_count_contract, "order_outside": case_order_outside,
    "random_points": lambda: case_random(3), "random_lines": lambda: case_random(4, True),
    "lds_bound": case_lds_bound, "many_groups": case_many_groups,
}

_refs = {}


def case_and_ref(name):
    """The case and the restatement's results, computed once and shared."""
    if name not in _refs:
        m, frames, check = CASES[name]()
        _refs[name] = (m, frames, check, [ref_frame(m, fr) for fr in frames])
    return _refs[name]


def same(a, b):
    for k in ("local_kf", "ref_kf", "local_mp", "mp_flags", "local_ml", "ml_flags"):
        assert a[k] == b[k], k
    for k in ("vote_mp", "vote_ml"):
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or np.array_equal(a[k], b[k])), k


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_against_forward_formulation(name):
    m, frames, check, refs = case_and_ref(name)
    for fr, r in zip(frames, refs):
        same(r, np_frame(m, fr))
    assert all(check(refs)), check(refs)


@pytest.mark.parametrize("seed", range(6))
def test_restatement_random_maps(seed):
    m, rng = random_map(100 + seed, K=40 + 30 * seed, kl_cap=6 if seed % 2 else 0, n_ml=150 if seed % 2 else 0,
                        imu=seed != 2)
    for fr in random_frames(m, rng, 4):
        same(ref_frame(m, fr), np_frame(m, fr))


# ------------------------------------------------------------------ gpu

def pack(frames, name):
    """[B][cap] table and counts of one of the four per-frame tables (None when no frame has it)."""
    if all(fr[name] is None for fr in frames):
        return None, None
    cap = max(max(len(fr[name] or ()) for fr in frames), 1)
    t = np.full((len(frames), cap), -3, np.int32)   # padding: an id that is read as NULL if it were read
    n = np.zeros(len(frames), np.int32)
    for f, fr in enumerate(frames):
        row = fr[name] or []
        t[f, :len(row)] = row
        n[f] = len(row) if fr["n_" + name] is None else fr["n_" + name]
    return t, n


def expected(lm, m, frames, refs, caps, gathers=None):
    """The outputs of update_batch as the restatement has them, sentinel-filled like the device buffers."""
    lines = m.kl_cap > 0
    e = lm._outputs(len(frames), caps, lines, FILL, gathers)
    for f, r in enumerate(refs):
        e["ref_kf"][f] = r["ref_kf"]
        err = 0
        for key, cap, bit, pool, g in (("local_kf", caps[0], 1, None, None),
                                       ("local_mp", caps[1], 2, lm.pools[0], "mp"),
                                       ("local_ml", caps[2], 4, lm.pools[1], "ml")):
            if key == "local_ml" and not lines:
                continue
            ids = np.array(r[key], np.int32)
            e["n_" + key][f] = len(ids)
            err |= bit if len(ids) > cap else 0
            w = min(len(ids), cap)
            e[key][f, :w] = ids[:w]
            if pool is None:
                continue
            for k in ("pos", "sep", "normal", "dist", "desc"):
                if f"{g}_{k}" in e:
                    e[f"{g}_{k}"][f, :w] = pool[k][ids[:w]]
            if f"{g}_in_flags" in e:
                e[f"{g}_in_flags"][f, :w] = r[g + "_flags"][:w]
        e["err"][f] = err
    return e


def gpu_args(frames):
    a = {}
    for name in ("vote_mp", "vote_ml", "seen_mp", "seen_ml"):
        a[name], a["n_" + name] = pack(frames, name)
    if a["vote_mp"] is None:
        a["vote_mp"], a["n_vote_mp"] = np.full((len(frames), 1), -1, np.int32), np.zeros(len(frames), np.int32)
    a["last_kf"] = np.array([fr["last_kf"] for fr in frames], np.int32)
    return a


def compare(got, e, frames, refs, args):
    assert got["rc"] == 0
    for k, want in e.items():
        assert np.array_equal(got[k], want), k
    for name in ("vote_mp", "vote_ml"):
        if args[name] is None:
            continue
        want = args[name].copy()
        for f, r in enumerate(refs):
            if r[name] is not None:
                want[f, :len(r[name])] = r[name]
        assert np.array_equal(got[name], want), name   # written back inside the count, untouched past it


def run_and_compare(name, caps=None, gathers=None):
    m, frames, _, refs = case_and_ref(name)
    lm = plvi.LocalMap(*m.tables())
    args = gpu_args(frames)
    n_mp, n_ml = len(m.mp_bad), len(m.ml_bad)
    caps = caps or [m.K, n_mp, n_ml]
    got = lm.update_batch(**args, lkf_cap=caps[0], lmp_cap=caps[1], lml_cap=caps[2], gathers=gathers, fill=FILL)
    compare(got, expected(lm, m, frames, refs, caps, gathers), frames, refs, args)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_equals_restatement(plvi_lib, name):
    """Every crafted case, B = its frames in one launch (random_*: three frames voting in different parts of one
    map), every output compared whole."""
    run_and_compare(name)


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_gpu_capacities(plvi_lib, which, delta):
    """Each capacity one below, at and one above the true list length: the full count, the err bit, and nothing
    written at or past the capacity (the sentinel fill of the expected arrays)."""
    _, _, _, refs = case_and_ref("random_lines")
    true = [len(refs[0][k]) for k in ("local_kf", "local_mp", "local_ml")]
    m = case_and_ref("random_lines")[0]
    caps = [m.K, len(m.mp_bad), len(m.ml_bad)]
    caps[which] = true[which] + delta
    got = run_and_compare("random_lines", caps)
    assert bool(got["err"][0] & (1 << which)) == (delta < 0)


@pytest.mark.gpu
def test_gpu_zero_capacities(plvi_lib):
    got = run_and_compare("random_lines", [0, 0, 0])
    assert (got["err"] == 7).all()


@pytest.mark.gpu
@pytest.mark.parametrize("null", [("pos", "desc"), ("normal", "dist", "sep"), ("pos", "sep", "normal", "dist", "desc")])
def test_gpu_null_gathers(plvi_lib, null):
    """Pool rows that are NULL are not gathered; in_flags and the lists do not depend on them."""
    m, frames, _, refs = case_and_ref("random_lines")
    m.null_gathers = null
    try:
        lm = plvi.LocalMap(*m.tables())
    finally:
        m.null_gathers = ()
    args = gpu_args(frames)
    caps = [m.K, len(m.mp_bad), len(m.ml_bad)]
    got = lm.update_batch(**args, lkf_cap=caps[0], lmp_cap=caps[1], lml_cap=caps[2], fill=FILL)
    assert not any(f"mp_{k}" in got or f"ml_{k}" in got for k in null)
    compare(got, expected(lm, m, frames, refs, caps), frames, refs, args)
    # and output pointers left NULL although the pool has the rows
    lm = plvi.LocalMap(*m.tables())
    got = lm.update_batch(**args, lkf_cap=caps[0], lmp_cap=caps[1], lml_cap=caps[2], gathers=("normal",), fill=FILL)
    assert "mp_in_flags" not in got and "mp_normal" in got
    compare(got, expected(lm, m, frames, refs, caps, ("normal",)), frames, refs, args)


@pytest.mark.gpu
def test_gpu_graph_capture(plvi_lib):
    """The batch form under plvi_graph_capture_begin / end and one replay: the two fills and four kernels."""
    m, frames, _, refs = case_and_ref("random_lines")
    lm = plvi.LocalMap(*m.tables())
    args = gpu_args(frames)
    caps = [m.K, len(m.mp_bad), len(m.ml_bad)]
    step, fetch = lm.update_batch(**args, lkf_cap=caps[0], lmp_cap=caps[1], lml_cap=caps[2], fill=FILL, run=False)
    st = ctypes.c_void_p()
    assert plvi_lib.plvi_stream_create(ctypes.byref(st)) == 0
    rcs = []
    g = plvi.StepGraph(lambda s: rcs.append(step(s)), st.value)
    assert rcs == [0]
    assert (fetch()["n_local_kf"] == FILL).all()   # captured, not run
    g.launch()
    assert plvi_lib.plvi_stream_synchronize(st) == 0
    compare(fetch(), expected(lm, m, frames, refs, caps), frames, refs, args)
    del g
    assert plvi_lib.plvi_stream_destroy(st) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["random_lines", "random_points", "bad_vote_cleared", "seen_distinct",
                                  "seen_ml_distinct", "count_contract", "no_votes"])
def test_gpu_host_form(plvi_lib, name):
    """plvi_local_map, one frame from host memory, through plvi.LocalMap.update."""
    m, frames, _, refs = case_and_ref(name)
    lm = plvi.LocalMap(*m.tables())
    for fr, r in zip(frames, refs):
        vm = np.array(fr["vote_mp"], np.int32)
        vl = None if fr["vote_ml"] is None else np.array(fr["vote_ml"], np.int32)
        sm = None if fr["seen_mp"] is None else np.array(fr["seen_mp"], np.int32)
        sl = None if fr["seen_ml"] is None else np.array(fr["seen_ml"], np.int32)
        counts = {k: fr["n_" + k] for k in ("vote_mp", "vote_ml", "seen_mp", "seen_ml") if fr["n_" + k] is not None}
        vm0, vl0 = vm.copy(), None if vl is None else vl.copy()
        got = lm.update(vm, vl, sm, sl, fr["last_kf"], counts=counts)
        for t, t0, k in ((vm, vm0, "vote_mp"), (vl, vl0, "vote_ml")):   # untouched past the clamped count
            assert t is None or np.array_equal(t[len(r[k]):], t0[len(r[k]):]), k
            if t is not None:
                t.resize(len(r[k]), refcheck=False)
        assert got["err"] == 0 and got["ref_kf"] == r["ref_kf"]
        assert got["local_kf"].tolist() == r["local_kf"] and got["local_mp"].tolist() == r["local_mp"]
        assert got["mp_in_flags"].tolist() == r["mp_flags"] and np.array_equal(vm, r["vote_mp"])
        ids = np.array(r["local_mp"], np.int64)
        for k in ("pos", "normal", "dist", "desc"):
            assert np.array_equal(got["mp_" + k], lm.pools[0][k][ids]), k
        if m.kl_cap:
            assert got["local_ml"].tolist() == r["local_ml"] and got["ml_in_flags"].tolist() == r["ml_flags"]
            assert np.array_equal(vl, r["vote_ml"])
            assert np.array_equal(got["ml_sep"], lm.pools[1]["sep"][np.array(r["local_ml"], np.int64)])
    # a capacity below the list: PLVI_E_CAPACITY is reported through err, the count stays whole
    r = refs[-1]
    if len(r["local_mp"]) > 1:
        got = lm.update(np.array(frames[-1]["vote_mp"], np.int32),
                        None if frames[-1]["vote_ml"] is None else np.array(frames[-1]["vote_ml"], np.int32),
                        None, None, frames[-1]["last_kf"], lmp_cap=len(r["local_mp"]) - 1, counts=counts)
        assert got["err"] == plvi.LOCAL_MAP_ERR_MP and got["n_local_mp"] == len(r["local_mp"])
        assert got["local_mp"].tolist() == r["local_mp"][:-1]


@pytest.mark.gpu
def test_gpu_refusals(plvi_lib):
    m, frames, _, _ = case_and_ref("lines")
    lm = plvi.LocalMap(*m.tables())
    dev = lm.upload()
    kf, mp, ml = lm._structs(lambda g, k: dev[(g, k)].ptr)
    buf = plvi.DeviceBuffer(1 << 16)
    buf.upload(np.zeros(1 << 14, np.int32))
    sb = plvi.local_map_scratch_bytes(2, m.K, mp.n, ml.n)
    scratch = plvi.DeviceBuffer(sb)

    def call(B=2, kf=kf, mp=mp, ml=ml, fr=None, out=None, scratch_ptr=scratch.ptr, bytes_=sb):
        fr = fr or plvi.LocalMapFrames(vote_mp=buf.ptr, n_vote_mp=buf.ptr, vote_mp_cap=4)
        if out is None:
            out = plvi.LocalMapOutputs(4, 4, 4)
            for k, _ in plvi.LocalMapOutputs._fields_[3:]:
                setattr(out, k, buf.ptr)
        return plvi.local_map_batch(B, kf, mp, ml, fr, out, scratch_ptr, bytes_)

    def changed(s, **kw):
        c = type(s)()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(s), ctypes.sizeof(s))
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    assert call(B=0, scratch_ptr=0, bytes_=0) == 0          # no launch, nothing needed
    assert call(B=-1) == E_BADARG
    for field in ("kf_cap", "n_order", "kp_cap", "kl_cap"):
        assert call(kf=changed(kf, **{field: -1})) == E_BADARG, field
    assert call(mp=changed(mp, n=-1)) == E_BADARG and call(ml=changed(ml, n=-1)) == E_BADARG
    for field in ("vote_mp_cap", "vote_ml_cap", "seen_mp_cap", "seen_ml_cap"):
        assert call(fr=plvi.LocalMapFrames(vote_mp=buf.ptr, n_vote_mp=buf.ptr, **{field: -1})) == E_BADARG, field
    out = plvi.LocalMapOutputs(4, 4, 4)
    for k, _ in plvi.LocalMapOutputs._fields_[3:]:
        setattr(out, k, buf.ptr)
    for field in ("lkf_cap", "lmp_cap", "lml_cap"):
        assert call(out=changed(out, **{field: -1})) == E_BADARG, field
    for field in ("n_local_kf", "ref_kf", "err", "n_local_mp", "local_mp", "n_local_ml"):
        assert call(out=changed(out, **{field: None})) == E_BADARG, field
    assert call(ml=None) == E_BADARG                          # keyframes->ml without a line pool
    assert call(mp=changed(mp, pos=None)) == E_BADARG         # a gather without its source rows
    assert call(fr=plvi.LocalMapFrames(vote_mp=buf.ptr)) == E_BADARG   # a table without its counts
    assert call(scratch_ptr=0) == E_BADARG and call(bytes_=sb - 1) == E_BADARG
    assert call(B=65536, bytes_=1 << 62) == E_CAPACITY
    assert call(kf=changed(kf, kf_cap=1 << 20, kp_cap=1 << 12), bytes_=1 << 62) == E_CAPACITY
    # a position of the walk must stay below the fill of the first-occurrence table: one above the limit
    assert 16711423 * 128 == plvi.LOCAL_MAP_MAX_ENTRIES + 1 < 2 ** 31
    assert call(kf=changed(kf, kf_cap=16711423, kp_cap=128, kl_cap=1), bytes_=1 << 62) == E_CAPACITY
    assert call(kf=changed(kf, kf_cap=16711423, kp_cap=1, kl_cap=128), bytes_=1 << 62) == E_CAPACITY
    # the host form makes the same checks before it reads child_off[kf_cap] or obs_off[n]
    tabs = lm._tables()
    hkf, hmp, hml = lm._structs(lambda g, k: tabs[(g, k)].ctypes.data)
    z = np.zeros(64, np.int32)
    hfr = plvi.LocalMapFrames(vote_mp=z.ctypes.data, n_vote_mp=z.ctypes.data, vote_mp_cap=4)
    hout = plvi.LocalMapOutputs(4, 4, 4)
    for k, _ in plvi.LocalMapOutputs._fields_[3:]:
        setattr(hout, k, z.ctypes.data)

    def host(kf=hkf, mp=hmp, ml=hml, fr=hfr, out=hout):
        r = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731
        return plvi_lib.plvi_local_map(r(kf), r(mp), r(ml), r(fr), r(out))
    assert host(kf=changed(hkf, nml=None)) == E_BADARG and host(kf=changed(hkf, bad=None)) == E_BADARG
    assert host(kf=changed(hkf, child=None)) == E_BADARG and host(mp=changed(hmp, obs_off=None)) == E_BADARG
    assert host(ml=None) == E_BADARG and host(kf=None) == E_BADARG and host(out=changed(hout, err=None)) == E_BADARG
    assert host(kf=changed(hkf, kf_cap=-1)) == E_BADARG and host(fr=changed(hfr, seen_ml_cap=-1)) == E_BADARG
    assert host(kf=changed(hkf, kf_cap=16711423, kp_cap=128)) == E_CAPACITY
    assert plvi.local_map_scratch_bytes(-1, 1, 1, 1) == 0
    assert call() == 0 and plvi_lib.plvi_device_synchronize() == 0


@pytest.mark.gpu
def test_gpu_chain_to_local_search(plvi_lib):
    """plvi_local_map_batch -> plvi_frustum_points_batch -> plvi_assign_grid_batch -> plvi_search_local_batch with no
    host step between (the counts and tables go from one call to the next as device pointers), against the same
    three calls fed from the restatement's lists gathered on the host."""
    import util
    B, K, n_mp, kcap = 2, 48, 900, 700
    rng = np.random.default_rng(21)
    prm = [util.frustum_params(60) for _ in range(B)]
    world = util.frustum_case(70, prm[0], n=n_mp)
    m = Map(K, kp_cap=40, n_mp=n_mp, imu=False)
    for i in range(n_mp):
        kfs = np.unique(np.clip(i * K // n_mp + rng.integers(-3, 4, 3), 0, K - 1)).tolist()
        m.mp_obs[i] = kfs
        for s in kfs:
            if m.nmp[s] < m.kp_cap:
                m.put(s, i)
    m.next_mp = n_mp
    m.mp_bad[:] = rng.random(n_mp) < 0.03
    for s in range(K):
        m.covis[s, :2] = [(s + 1) % K, (s + 5) % K]
    kf, mp, _ = m.tables()
    mp.update(pos=world["pos"], normal=world["normal"], dist=world["dist"],
              desc=rng.integers(0, 256, (n_mp, 32), dtype=np.uint8))
    lm = plvi.LocalMap(kf, mp)
    frames = [frame(rng.choice(n_mp // 2, 80, replace=False).tolist()),
              frame((n_mp // 3 + rng.choice(n_mp // 2, 80, replace=False)).tolist())]
    refs = [ref_frame(m, fr) for fr in frames]
    assert min(len(r["local_mp"]) for r in refs) > 300
    cap = 640
    args = gpu_args(frames)
    got = lm.update_batch(**args, lkf_cap=K, lmp_cap=cap, fill=FILL)
    e = expected(lm, m, frames, refs, [K, cap, 0])
    compare(got, e, frames, refs, args)

    bufs = []

    def dev(a):
        a = np.ascontiguousarray(a)
        b = plvi.DeviceBuffer(max(a.nbytes, 4))
        b.upload(a)
        bufs.append(b)
        return ctypes.c_void_p(b.ptr)
    # current-frame keypoints near the projections of frame 0's visible local points
    kk = np.zeros((B, kcap), plvi.KEYPOINT_DTYPE)
    kk["x"], kk["y"] = rng.uniform(0, 752, (B, kcap)), rng.uniform(0, 480, (B, kcap))
    kk["octave"], kk["size"], kk["class_id"] = rng.integers(0, 8, (B, kcap)), 31, -1
    kd = rng.integers(0, 256, (B, kcap, 32), dtype=np.uint8)
    d_prm = dev(np.frombuffer(bytes((plvi.FrustumParams * B)(*prm)), np.uint8))
    g = plvi.grid_geometry(752, 480)
    lp = plvi.LocalParams()
    lp.min_x, lp.min_y, lp.inv_w, lp.inv_h, lp.th, lp.nnratio, lp.nlevels = g[0], g[2], g[4], g[5], 3.0, 0.8, 8
    for i, s in enumerate(util.orb_scale_factors()):
        lp.scale_factors[i] = s
    V = ctypes.c_void_p

    def chain(pos, nrm, dst, fin, desc, n, kpts=None):
        """frustum -> (grid) -> search; returns (flags, proj, level, nvisible, match, nmatches)."""
        z = lambda shape, dt: dev(np.zeros(shape, dt))  # noqa: E731
        d_fl, d_pr, d_lv, d_de = z((B, cap), np.uint8), z((B, cap, 4), np.float32), z((B, cap), np.int32), \
            z((B, cap), np.float32)
        d_nv = z(B, np.int32)
        assert plvi_lib.plvi_frustum_points_batch(B, d_prm, pos, nrm, dst, fin, n, cap, d_fl, d_pr, d_lv, None, None,
                                                  d_de, d_nv, None) == 0
        if kpts is None:
            plvi_lib.plvi_device_synchronize()
            return (plvi.download(d_fl.value, np.zeros((B, cap), np.uint8)),
                    plvi.download(d_pr.value, np.zeros((B, cap, 4), np.float32)),
                    plvi.download(d_lv.value, np.zeros((B, cap), np.int32)))
        d_k, d_kn = dev(kpts), dev(np.full(B, kcap, np.int32))
        off, idx = plvi.DeviceBuffer(B * 3073 * 4), plvi.DeviceBuffer(B * kcap * 4)
        bufs.extend([off, idx])
        plvi.assign_grid_batch(d_k.value, d_kn.value, kcap, B, plvi.GridParams(g[0], g[2], g[4], g[5]), off.ptr,
                               idx.ptr)
        d_match, d_nm = z((B, kcap), np.int32), z(B, np.int32)
        assert plvi_lib.plvi_search_local_batch(B, ctypes.byref(lp), d_k, dev(kd), d_kn, kcap, None, None, V(off.ptr),
                                                V(idx.ptr), d_fl, d_pr, d_lv, desc, n, cap, d_match, d_nm, None) == 0
        plvi_lib.plvi_device_synchronize()
        return (plvi.download(d_fl.value, np.zeros((B, cap), np.uint8)),
                plvi.download(d_nv.value, np.zeros(B, np.int32)),
                plvi.download(d_match.value, np.zeros((B, kcap), np.int32)),
                plvi.download(d_nm.value, np.zeros(B, np.int32)))
    d = got["d"]
    on_device = [V(d[k].ptr) for k in ("mp_pos", "mp_normal", "mp_dist", "mp_in_flags", "mp_desc", "n_local_mp")]
    from_host = [dev(e[k]) for k in ("mp_pos", "mp_normal", "mp_dist", "mp_in_flags", "mp_desc", "n_local_mp")]
    # place the keypoints on the projections the frustum pass predicts (from the host-fed tables)
    fl, pr, lv = chain(*from_host)
    for f in range(B):
        vis = np.nonzero(fl[f, :len(refs[f]["local_mp"])] & 1)[0][:kcap // 2]
        assert len(vis) > 20
        kk["x"][f, :len(vis)], kk["y"][f, :len(vis)] = pr[f, vis, 0] + 0.5, pr[f, vis, 1] - 0.5
        kk["octave"][f, :len(vis)] = np.clip(lv[f, vis], 0, 7)
        kd[f, :len(vis)] = e["mp_desc"][f, vis]
        kd[f, :len(vis), 0] ^= 1
    a, b = chain(*on_device, kpts=kk), chain(*from_host, kpts=kk)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert (a[3] > 20).all() and (a[1] > 20).all()
