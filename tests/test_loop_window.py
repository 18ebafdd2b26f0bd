"""The loop-detection windows on the device (csrc/loop_window.hip, plvi_loop_window[_batch] and
plvi_loop_bow_merge[_batch]): the keyframe windows, the first-come BoW merge and the point clouds of
LoopClosing::DetectCommonRegionsFromBoW and FindMatchesByProjection (src/LoopClosing.cc:797-858, :893-915,
:1162-1199).

Expected values come from tests/native/loop_window_ref.cpp, a sequential host restatement in the reference's own
shape (keyframe objects with an ordered covisible vector, std::set membership, the push_back / [0] = window, whole
vectors appended, the break inside the j loop).  The CPU part pins it against np_query below, an independent
restatement in the formulation the kernel uses -- no sets, "the smallest traversal position wins" by
np.unique(return_index) -- on every crafted case and on the random maps, asserts what each crafted case is there to
show, and asserts the coverage of the random maps.  The gpu part demands exact equality with the restatement for
every output of both forms, with sentinel-filled tables.

Every crafted case lives in ONE map (a case takes fresh keyframe slots and fresh point ids), so one batch runs them
all."""
import ctypes
import functools
import pathlib
import subprocess

import numpy as np
import pytest

import plvi

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "loop_window_ref.cpp"
BUILD = ROOT / "tests" / "native" / "_build"
FILL = -7
BOW, PROJ, LAST = range(3)
E_PTS, E_UNDEF, E_QUERY = 1, 2, 4
WIN_MAX, BOW_WIN = 31, 6
OUT = 1 << 20   # a keyframe slot outside every map
SCALARS = ("n_win", "abort_at", "n_pts", "err")


# ------------------------------------------------------------------ the map
class LoopMap:
    """Keyframe tables, covisible rows and a MapPoint pool, grown case by case."""

    def __init__(self, cap):
        self.cap = cap
        self.tab, self.bad, self.cand, self.pbad = [], [], [], []

    @property
    def K(self):
        return len(self.bad)

    def pt(self, bad=0):
        self.pbad.append(bad)
        return len(self.pbad) - 1

    def kf(self, ids=(), bad=0, cov=()):
        assert len(ids) <= self.cap, "table full"
        self.tab.append(list(ids))
        self.bad.append(bad)
        self.cand.append(list(cov))
        return self.K - 1

    def kfs(self, n, **kw):
        return [self.kf([self.pt()], **kw) for _ in range(n)]

    def tables(self, stride=None, pad_kf=0):
        """(keyframes, points) as plvi.LoopWindow takes them; pad_kf empty (bad) slots are appended."""
        K = self.K + pad_kf
        stride = stride or max(1, max(len(c) for c in self.cand))
        tab = np.full((K, self.cap), -1, np.int32)
        ntab = np.zeros(K, np.int32)
        cand = np.full((K, stride), -1, np.int32)
        n_cand = np.zeros(K, np.int32)
        for s in range(self.K):
            ntab[s] = len(self.tab[s])
            tab[s, :ntab[s]] = self.tab[s]
            n_cand[s] = len(self.cand[s])
            cand[s, :n_cand[s]] = self.cand[s]
        bad = np.array(list(self.bad) + [1] * pad_kf, np.uint8)
        n = len(self.pbad)
        rng = np.random.default_rng(n)
        pool = dict(bad=np.array(self.pbad, np.uint8).reshape(-1), pos=rng.normal(size=(n, 3)).astype(np.float32),
                    normal=rng.normal(size=(n, 3)).astype(np.float32),
                    dist=rng.uniform(1, 9, (n, 2)).astype(np.float32),
                    desc=rng.integers(0, 256, (n, 32), dtype=np.uint8))
        return dict(bad=bad, mp=tab, nmp=ntab, cand=cand, n_cand=n_cand), pool


def query(kind, kf_slot, cur_slot=0, conn=(), m12=None, n1=0):
    """One query.  m12 [6][cap1] (BOW): the six SearchByBoW tables; n1: the current keyframe's N."""
    return dict(kind=kind, kf_slot=kf_slot, cur_slot=cur_slot, conn=list(conn),
                m12=None if m12 is None else np.ascontiguousarray(m12, np.int32), n1=n1)


def match_table(rows, cap1):
    """[6][cap1] from {member j: {k: index}}."""
    m = np.full((BOW_WIN, cap1), -1, np.int32)
    for j, r in rows.items():
        for k, i in r.items():
            m[j, k] = i
    return m


def blank(pt_cap, cap1=None):
    r = {k: FILL for k in SCALARS}
    r.update(win=[FILL] * WIN_MAX, pts=[FILL] * max(pt_cap, 1), pts_kf=[FILL] * max(pt_cap, 1))
    if cap1 is not None:
        r.update(matched_mp=[FILL] * max(cap1, 1), matched_kf=[FILL] * max(cap1, 1), num=FILL)
    return r


# ------------------------------------------------------- the restatement (C++)
class RefTables(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("kf_cap", "kp_cap", "cand_stride")] + \
               [(k, ctypes.c_void_p) for k in ("bad", "mp", "nmp", "cand", "n_cand")] + \
               [("mp_n", ctypes.c_int), ("mp_bad", ctypes.c_void_p)]


class RefQuery(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("kind", "kf_slot", "cur_slot", "n_conn")] + \
               [("conn", ctypes.c_void_p), ("pt_cap", ctypes.c_int), ("matches12", ctypes.c_void_p),
                ("n1", ctypes.c_int), ("cap1", ctypes.c_int)] + \
               [(k, ctypes.c_void_p) for k in ("win", "n_win", "abort_at", "pts", "pts_kf", "n_pts", "err",
                                               "matched_mp", "matched_kf", "num", "seconds")]


@functools.lru_cache(None)
def ref_lib():
    so = BUILD / "libloop_window_ref.so"
    if not so.exists() or so.stat().st_mtime < SRC.stat().st_mtime:
        so.parent.mkdir(parents=True, exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", str(so), str(SRC)],
                       check=True)
    lib = ctypes.CDLL(str(so))
    lib.loop_window_ref_run.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.loop_window_ref_run.restype = None
    return lib


def ref_run(tabs, queries, pt_cap=None, seconds=None):
    """The restatement's outputs of every query, as plain Python values."""
    kf, pool = tabs
    pt_cap = max(len(pool["bad"]), 1) if pt_cap is None else pt_cap
    t = RefTables(len(kf["bad"]), kf["mp"].shape[1], kf["cand"].shape[1], kf["bad"].ctypes.data, kf["mp"].ctypes.data,
                  kf["nmp"].ctypes.data, kf["cand"].ctypes.data, kf["n_cand"].ctypes.data, len(pool["bad"]),
                  pool["bad"].ctypes.data)
    B = len(queries)
    qs = (RefQuery * max(B, 1))()
    keep = []
    for i, q in enumerate(queries):
        cap1 = None if q["m12"] is None else q["m12"].shape[1]
        o = {k: np.full(1, FILL, np.int32) for k in SCALARS + ("num",)}
        o["win"] = np.full(WIN_MAX, FILL, np.int32)
        o["pts"], o["pts_kf"] = (np.full(max(pt_cap, 1), FILL, np.int32) for _ in range(2))
        o["matched_mp"], o["matched_kf"] = (np.full(max(cap1 or 0, 1), FILL, np.int32) for _ in range(2))
        o["seconds"] = np.zeros(1, np.float64)
        conn = np.array(q["conn"], np.int32).reshape(-1)
        keep.append((o, conn))
        r = qs[i]
        r.kind, r.kf_slot, r.cur_slot, r.n_conn, r.conn = q["kind"], q["kf_slot"], q["cur_slot"], len(conn), \
            conn.ctypes.data
        r.pt_cap = pt_cap
        if cap1 is not None:
            r.matches12, r.n1, r.cap1 = q["m12"].ctypes.data, q["n1"], cap1
        for k, a in o.items():
            setattr(r, k, a.ctypes.data)
    ref_lib().loop_window_ref_run(ctypes.byref(t), B, qs)
    res = []
    for q, (o, _) in zip(queries, keep):
        r = {k: int(o[k][0]) for k in SCALARS}
        r.update({k: o[k].tolist() for k in ("win", "pts", "pts_kf")})
        if q["m12"] is not None:
            r.update(matched_mp=o["matched_mp"].tolist(), matched_kf=o["matched_kf"].tolist(), num=int(o["num"][0]))
        if seconds is not None:
            seconds.append(float(o["seconds"][0]))
        res.append(r)
    return res


# ------------------------------------- the position formulation (numpy)
def cov5(kf, s):
    n = min(int(np.clip(kf["n_cand"][s], 0, kf["cand"].shape[1])), 5)
    return [int(v) for v in kf["cand"][s, :n]]


def np_query(tabs, q, pt_cap=None):
    kf, pool = tabs
    K, n, cap = len(kf["bad"]), len(pool["bad"]), kf["mp"].shape[1]
    pt_cap = max(n, 1) if pt_cap is None else pt_cap
    cap1 = None if q["m12"] is None else q["m12"].shape[1]
    r = blank(pt_cap, cap1)
    kind, m = q["kind"], q["kf_slot"]
    n1 = 0 if cap1 is None else int(np.clip(q["n1"], 0, cap1))
    if cap1 is not None:
        r["matched_mp"][:n1] = r["matched_kf"][:n1] = [-1] * n1
        r["num"] = 0
    r.update(n_win=0, abort_at=-1, n_pts=0, err=0)
    if kind not in (BOW, PROJ, LAST) or not 0 <= m < K or (kind == BOW and not 0 <= q["cur_slot"] < K):
        r["err"] = E_QUERY
        return r
    slot = lambda s: 0 <= s < K  # noqa: E731
    if kind == BOW:
        if kf["bad"][m]:
            return r
        c = cov5(kf, m)
        win = [m] + c[1:] + c[:1]
        r["err"] = 0 if c else E_UNDEF
        conn = np.array([s for s in q["conn"] if slot(s)], np.int64)
        hit = np.flatnonzero(np.isin(np.array(win, np.int64), conn))
        r["abort_at"] = int(hit[0]) if len(hit) else -1
        r["n_win"] = len(win)
        r["win"][:len(win)] = win
        if cap1 is None:
            return r
        J = len(win) if r["abort_at"] < 0 else r["abort_at"]
        P = np.full((max(J, 1), max(n1, 1)), -1, np.int64)[:J, :n1]
        for j in range(J):
            s = win[j]
            if not slot(s) or kf["bad"][s]:
                continue
            idx = q["m12"][j, :n1].astype(np.int64)
            ok = (idx >= 0) & (idx < int(np.clip(kf["nmp"][s], 0, cap)))
            p = np.where(ok, kf["mp"][s, np.clip(idx, 0, max(cap - 1, 0))], -1).astype(np.int64)
            ok = (p >= 0) & (p < n)
            ok[ok] = pool["bad"][p[ok]] == 0
            P[j] = np.where(ok, p, -1)
        flat = P.ravel()
        pos = np.flatnonzero(flat >= 0)
        _, first = np.unique(flat[pos], return_index=True)
        winners = np.sort(pos[first])   # ascending position: a later member overwrites its cell
        r["num"] = len(winners)
        for w in winners:
            j, k = divmod(int(w), n1)
            r["matched_mp"][k] = int(flat[w])
            r["matched_kf"][k] = win[j]
        return r
    c = cov5(kf, m)
    win = c + [m]
    if kind == LAST:
        for s in c:
            if slot(s):
                win += cov5(kf, s)
    rows = [s for s in win if slot(s)]
    lens = [int(np.clip(kf["nmp"][s], 0, cap)) for s in rows]
    ids = np.concatenate([kf["mp"][s, :ln] for s, ln in zip(rows, lens)] + [np.zeros(0, np.int32)]).astype(np.int64)
    own = np.repeat(np.array(rows, np.int64), lens)
    ok = (ids >= 0) & (ids < n)
    ok[ok] = pool["bad"][ids[ok]] == 0
    ids, own = ids[ok], own[ok]
    _, first = np.unique(ids, return_index=True)
    first.sort()
    pts, own = ids[first].tolist(), own[first].tolist()
    r["n_win"], r["n_pts"] = len(win), len(pts)
    r["win"][:len(win)] = win
    k = min(len(pts), pt_cap)
    r["pts"][:k] = pts[:k]
    if kind == PROJ:
        r["pts_kf"][:k] = own[:k]
    r["err"] = E_PTS if len(pts) > pt_cap else 0
    return r


# ------------------------------------------------------------ crafted cases
@functools.lru_cache(None)
def crafted():
    """(tables, {name: (query, check(expected))}) -- every crafted case, in one map."""
    m = LoopMap(cap=8)
    cur = m.kf([m.pt()])
    cases = {}

    def add(name, q, check):
        cases[name] = (q, check)

    # ---- the BoW window: covisible lists of 0, 1, 4, 5 and 6 entries, c0 goes last
    for n in (0, 1, 4, 5, 6):
        cs = m.kfs(n)
        i = m.kf([m.pt()], cov=cs)
        exp_win = [i] + cs[1:5] + cs[:1]

        def check(e, exp_win=exp_win, n=n):
            assert e["win"][:e["n_win"]] == exp_win and e["win"][e["n_win"]:] == [FILL] * (WIN_MAX - len(exp_win))
            assert e["err"] == (E_UNDEF if n == 0 else 0) and e["abort_at"] == -1 and e["n_pts"] == 0
        add(f"bow-cov{n}", query(BOW, i, cur), check)
    cs = m.kfs(3)
    i = m.kf([m.pt()], bad=1, cov=cs)
    add("bow-bad-candidate", query(BOW, i, cur, conn=[cs[0]]),
        lambda e: (e["n_win"], e["abort_at"], e["err"], e["win"][0]) == (0, -1, 0, FILL) or pytest.fail(str(e)))

    # ---- abort_at: at 0, in the middle, none; a bad member that is connected aborts
    cs = m.kfs(5)
    i = m.kf([m.pt()], cov=cs)
    add("abort-at-0", query(BOW, i, cur, conn=[cs[2], i]), lambda e: e["abort_at"] == 0 or pytest.fail(str(e)))
    add("abort-middle", query(BOW, i, cur, conn=[cs[0], cs[3], OUT, -1]),   # window i c1 c2 c3 c4 c0: c3 is at 3
        lambda e: e["abort_at"] == 3 or pytest.fail(str(e)))
    add("abort-none", query(BOW, i, cur, conn=[cur, OUT]), lambda e: e["abort_at"] == -1 or pytest.fail(str(e)))
    add("abort-c0-is-last", query(BOW, i, cur, conn=[cs[0]]), lambda e: e["abort_at"] == 5 or pytest.fail(str(e)))
    pa, pb, pc = m.pt(), m.pt(), m.pt()
    badc = m.kf([pa], bad=1)
    good = m.kf([pb, pc])
    i = m.kf([m.pt()], cov=[good, badc, good])   # window i, badc, good, good
    tab = match_table({1: {0: 0}, 2: {1: 0}, 3: {2: 1}}, 4)

    def check(e, pb=pb, good=good):
        # the bad member at 1 aborts; nothing at or past it is merged
        assert e["abort_at"] == 1 and e["num"] == 0 and e["matched_mp"] == [-1] * 4
    add("bad-member-connected-aborts", query(BOW, i, cur, conn=[badc], m12=tab, n1=4), check)

    def check(e, pa=pa, pb=pb, pc=pc, good=good):
        # not connected: the bad member's row contributes nothing, the members after it do
        assert e["abort_at"] == -1 and e["num"] == 2
        assert e["matched_mp"] == [-1, pb, pc, -1] and e["matched_kf"] == [-1, good, good, -1]
    add("bad-member-not-connected", query(BOW, i, cur, m12=tab, n1=4), check)

    # ---- the merge
    p1, p2, p3, p4 = (m.pt() for _ in range(4))
    pbad = m.pt(bad=1)
    a = m.kf([p1, p3, pbad, -1])
    b = m.kf([p2, p3, p4])
    i = m.kf([p1], cov=[a, b])     # window i, b, a
    tab = match_table({0: {0: 0}, 1: {1: 0, 2: 2, 3: 1}, 2: {1: 0, 2: 1, 4: 1, 5: 2, 6: 3, 7: 9}}, 8)

    def check(e, p1=p1, p2=p2, p3=p3, p4=p4, i=i, a=a, b=b):
        # (0,0) p1, (1,1) p2, (1,2) p4, (1,3) p3 are new; member a: (2,1) p1 seen, (2,2) p3 seen, (2,4) p3 seen,
        # (2,5) bad, (2,6) NULL entry, (2,7) outside the table
        assert e["num"] == 4
        assert e["matched_mp"] == [p1, p2, p4, p3, -1, -1, -1, -1]
        assert e["matched_kf"] == [i, b, b, b, -1, -1, -1, -1]
    add("merge-seen-null-bad", query(BOW, i, cur, m12=tab, n1=8), check)
    q1, q2, q3 = (m.pt() for _ in range(3))
    a = m.kf([q1, q3])
    b = m.kf([q2, q3])
    i = m.kf([m.pt()], cov=[a, b])     # window i, b, a
    tab = match_table({1: {0: 0, 1: 1}, 2: {0: 0, 2: 1}}, 3)

    def check(e, q1=q1, q2=q2, q3=q3, a=a, b=b):
        # k = 0: b gives q2, then a gives q1: both count, the cell holds the later one.  q3 is found by b at k = 1
        # and by a at k = 2: only the first cell is written
        assert e["num"] == 3 and e["num"] > sum(v >= 0 for v in e["matched_mp"][:3])
        assert e["matched_mp"][:3] == [q1, q3, -1] and e["matched_kf"][:3] == [a, b, -1]
    add("merge-overwrite-and-first-cell", query(BOW, i, cur, m12=tab, n1=3), check)
    add("merge-n1-above-cap1", query(BOW, i, cur, m12=tab, n1=5), check)   # the count contract

    # ---- PROJ: the owner is the first keyframe in walk order, not m; a bad keyframe is still walked
    s1, s2, s3 = (m.pt() for _ in range(3))
    sb = m.pt(bad=1)
    c0 = m.kf([s1, -1, sb])
    c1 = m.kf([s2, s1], bad=1)
    i = m.kf([s1, s2, s3], cov=[c0, c1])

    def check(e, c0=c0, c1=c1, i=i, s=(s1, s2, s3)):
        assert e["win"][:3] == [c0, c1, i] and e["n_win"] == 3 and e["abort_at"] == -1
        assert e["pts"][:3] == list(s) and e["pts_kf"][:3] == [c0, c1, i] and e["n_pts"] == 3
    add("proj-owner-and-bad-kf", query(PROJ, i), check)
    add("proj-cand-out-of-range", query(PROJ, m.kf([s3, OUT], cov=[OUT, c0, -1])),
        lambda e, c0=c0, s=(s3, s1): (e["win"][:2] == [OUT, c0] and e["win"][2] == -1 and e["n_win"] == 4
                                      and e["pts"][:e["n_pts"]] == [s[1], s[0]]) or pytest.fail(str(e)))
    add("bow-cand-out-of-range", query(BOW, m.kf([s3], cov=[OUT, c0]), cur, conn=[OUT], m12=match_table({1: {0: 0},
                                                                                                     2: {1: 0}}, 2),
                                       n1=2),
        lambda e, c0=c0, s1=s1: (e["win"][1:3] == [c0, OUT] and e["abort_at"] == -1 and e["num"] == 1
                                 and e["matched_mp"] == [s1, -1]) or pytest.fail(str(e)))

    # ---- LAST: repeats, the searched keyframe inside, the dead nInserted rule
    t = [m.pt() for _ in range(6)]
    near = m.kf([t[5]])                 # connected to the current keyframe
    x = m.kf([t[0]])
    y = m.kf([t[1], t[0]])
    i = m.kf([t[2]])
    m.cand[x] = [y, i, near]            # the searched keyframe inside the window, and a connected one
    m.cand[y] = [x, y, x]               # repeats
    m.cand[i] = [x, y]

    def check(e, x=x, y=y, i=i, near=near, t=t):
        assert e["win"][:e["n_win"]] == [x, y, i, y, i, near, x, y, x] and e["abort_at"] == -1
        # honouring :1172-1180 would leave out `near` (connected to the current keyframe) and with it t[5]
        assert e["pts"][:e["n_pts"]] == [t[0], t[1], t[2], t[5]] and e["pts_kf"][0] == FILL
    add("last-repeats-self-dead-rule", query(LAST, i, cur, conn=[near]), check)
    full = m.kfs(5)
    for s in full:
        m.cand[s] = [full[(full.index(s) + d) % 5] for d in range(1, 5)] + [cur, i]
    j = m.kf([m.pt()], cov=full + [x])
    add("last-31", query(LAST, j), lambda e: e["n_win"] == 31 or pytest.fail(str(e)))
    add("last-cand-out-of-range", query(LAST, m.kf([t[3]], cov=[OUT, x])),
        lambda e, x=x, y=y, i=i, near=near: e["win"][:e["n_win"]] == [OUT, x, e["win"][2], y, i, near]
        or pytest.fail(str(e)))

    # ---- queries outside the map
    for name, q in (("query-slot", query(PROJ, OUT)), ("query-negative", query(LAST, -1)),
                    ("query-kind", query(3, cur)), ("query-cur", query(BOW, cur, OUT))):
        add(name, q, lambda e: (e["n_win"], e["abort_at"], e["n_pts"], e["err"]) == (0, -1, 0, E_QUERY)
            or pytest.fail(str(e)))
    return m.tables(pad_kf=2), cases


def test_crafted_cases_show_what_they_are_for():
    tabs, cases = crafted()
    exp = ref_run(tabs, [q for q, _ in cases.values()])
    for (name, (q, check)), e in zip(cases.items(), exp):
        assert e == np_query(tabs, q), name
        check(e)


@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_crafted_cases_at_the_capacity(delta):
    tabs, cases = crafted()
    qs = [q for q, _ in cases.values()]
    longest = max(e["n_pts"] for e in ref_run(tabs, qs))
    exp = ref_run(tabs, qs, pt_cap=longest + delta)
    assert any(e["err"] & E_PTS for e in exp) == (delta < 0)
    for q, e in zip(qs, exp):
        assert e == np_query(tabs, q, longest + delta)


# -------------------------------------------------------------- random maps
def random_map(seed, K=36, cap=10, n=120, stride=7):
    rng = np.random.default_rng(seed)
    m = LoopMap(cap)
    for _ in range(n):
        m.pt(bad=int(rng.uniform() < 0.1))
    for s in range(K):
        ids = rng.integers(-1, n + 1, rng.integers(0, cap + 1))     # -1 and n: NULL and out of range
        ncov = int(rng.choice([0, 1, 3, 5, 6, 7], p=[0.04, 0.04, 0.06, 0.5, 0.2, 0.16]))
        local = seed % 3 == 0     # covisibles from a small neighbourhood: repeats and the keyframe itself
        cov = [int((s + rng.integers(-4, 5)) % K) if local else int(rng.integers(0, K)) for _ in range(ncov)]
        if rng.uniform() < 0.05 and cov:
            cov[int(rng.integers(len(cov)))] = OUT
        m.kf(ids.tolist(), bad=int(rng.uniform() < 0.1), cov=cov)
    tabs = m.tables(stride=stride)
    qs = []
    for _ in range(14):
        kind = int(rng.integers(0, 3))
        slot = int(rng.integers(0, K)) if rng.uniform() < 0.97 else int(rng.choice([-1, K, OUT]))
        conn = rng.integers(0, K, int(rng.integers(0, 4))).tolist() if rng.uniform() < 0.5 else []
        if kind == BOW:
            cap1 = int(rng.integers(1, 13))
            qs.append(query(BOW, slot, int(rng.integers(0, K)), conn,
                            m12=rng.integers(-1, cap + 1, (BOW_WIN, cap1)), n1=int(rng.integers(0, cap1 + 2))))
        else:
            qs.append(query(kind, slot, 0, conn))
    return tabs, qs


SEEDS = range(40)


@functools.lru_cache(None)
def random_expected(seed, pt_cap=None):
    tabs, qs = random_map(seed)
    return tabs, qs, ref_run(tabs, qs, pt_cap)


def random_pt_cap(seed):
    return None if seed % 4 else 25


def test_random_maps_match_the_position_formulation_and_cover():
    cov = dict(last31=0, repeats=0, overwritten=0, num_above=0, err=0)
    for seed in SEEDS:
        pt_cap = random_pt_cap(seed)
        tabs, qs, exp = random_expected(seed, pt_cap)
        for q, e in zip(qs, exp):
            assert e == np_query(tabs, q, pt_cap), (seed, q)
            cov["err"] |= e["err"]
            w = e["win"][:e["n_win"]]
            cov["last31"] += q["kind"] == LAST and e["n_win"] == WIN_MAX
            cov["repeats"] += len(set(w)) < len(w)
            if q["m12"] is not None and e["err"] != E_QUERY:
                n1 = min(max(q["n1"], 0), q["m12"].shape[1])
                cells = sum(v >= 0 for v in e["matched_mp"][:n1])
                cov["num_above"] += e["num"] > cells
                # every winner writes one cell, so num - cells is the number of cells written again
                cov["overwritten"] += e["num"] - cells > 0
    assert cov["err"] == E_PTS | E_UNDEF | E_QUERY, cov
    assert min(cov["last31"], cov["repeats"], cov["overwritten"], cov["num_above"]) >= 20, cov


# ====================================================================== GPU
def plain(r, i, q, pt_cap):
    """Query i of a batch / host result as ref_run gives it."""
    e = {k: int(r[k][i]) for k in SCALARS}
    e["win"] = r["win"][i].tolist()
    e["pts"] = r["pts"][i].tolist()
    e["pts_kf"] = r["pts_kf"][i].tolist() if "pts_kf" in r else [FILL] * max(pt_cap, 1)
    return e


def past_is_clean(r):
    for k, v in r["past"].items():
        a = np.asarray(v)
        assert (a == (FILL & 0x7f if k == "desc" else FILL)).all(), f"{k} written past the batch"


def rows_equal_pool(r, i, pool, n_pts, pt_cap, gather):
    k = min(n_pts, pt_cap)
    ids = r["pts"][i][:k]
    for g in gather:
        assert np.array_equal(r[g][i][:k], pool[g][ids]), g
        fill = FILL & 0x7f if g == "desc" else FILL
        assert (r[g][i][k:] == fill).all(), f"{g} written past the list"


def merge_rows(queries, exp):
    """The BOW queries with match tables, padded to one cap1, as merge_batch takes them."""
    sel = [i for i, q in enumerate(queries) if q["m12"] is not None]
    if not sel:
        return sel, 0, None, None
    cap1 = max(queries[i]["m12"].shape[1] for i in sel)
    m12 = np.full((len(sel), BOW_WIN, cap1), -1, np.int32)
    for r, i in enumerate(sel):
        m12[r, :, :queries[i]["m12"].shape[1]] = queries[i]["m12"]
    n1 = np.array([min(queries[i]["n1"], queries[i]["m12"].shape[1]) for i in sel], np.int32)
    return sel, cap1, m12, n1


def batch_equals(tabs, queries, pt_cap=None, gather=("pos", "normal", "dist", "desc"), host=True, exp=None):
    kf, pool = tabs
    lw = plvi.LoopWindow(kf, pool)
    exp = exp or ref_run(tabs, queries, pt_cap)
    cap = max(len(pool["bad"]), 1) if pt_cap is None else pt_cap
    args = lambda qs: dict(kind=[q["kind"] for q in qs], kf_slot=[q["kf_slot"] for q in qs],  # noqa: E731
                           cur_slot=[q["cur_slot"] for q in qs], connected=[q["conn"] for q in qs])
    got = lw.batch(**args(queries), pt_cap=cap, gather=gather, fill=FILL)
    assert got["rc"] == 0
    past_is_clean(got)
    for i, (q, e) in enumerate(zip(queries, exp)):
        assert plain(got, i, q, cap) == {k: e[k] for k in SCALARS + ("win", "pts", "pts_kf")}, (i, q)
        rows_equal_pool(got, i, pool, e["n_pts"], cap, gather)
    sel, cap1, m12, n1 = merge_rows(queries, exp)
    if sel:
        mg = lw.merge_batch(got["win"][sel], got["n_win"][sel], got["abort_at"][sel], m12, n1, fill=FILL)
        assert mg["rc"] == 0
        past_is_clean(mg)
        for r, i in enumerate(sel):
            c = queries[i]["m12"].shape[1]
            assert int(mg["num"][r]) == exp[i]["num"], (i, queries[i])
            for k in ("matched_mp", "matched_kf"):
                assert mg[k][r][:c].tolist() == exp[i][k][:c] if c else True, (i, k)
                assert (mg[k][r][int(n1[r]):] == FILL).all(), (i, k)
    if not host:
        return
    for i, (q, e) in enumerate(zip(queries, exp)):
        h = lw.host(q["kind"], q["kf_slot"], q["cur_slot"], q["conn"], pt_cap=cap, gather=gather, fill=FILL)
        assert h["rc"] == (plvi.PLVI_E_CAPACITY if e["err"] & (E_PTS | E_QUERY) else 0)
        past_is_clean(h)
        assert plain(h, 0, q, cap) == {k: e[k] for k in SCALARS + ("win", "pts", "pts_kf")}, (i, q)
        rows_equal_pool(h, 0, pool, e["n_pts"], cap, gather)
        if q["m12"] is not None:
            w = np.array(e["win"], np.int32)
            hm = lw.merge_host(w, e["n_win"], e["abort_at"], q["m12"], q["n1"], fill=FILL)
            past_is_clean(hm)
            assert int(hm["num"][0]) == e["num"]
            for k in ("matched_mp", "matched_kf"):
                assert hm[k][0].tolist() == e[k], (i, k)


@pytest.mark.gpu
def test_gpu_crafted_cases_in_one_batch(plvi_lib):
    tabs, cases = crafted()
    batch_equals(tabs, [q for q, _ in cases.values()])


@pytest.mark.gpu
@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_gpu_crafted_cases_at_the_capacity(plvi_lib, delta):
    tabs, cases = crafted()
    qs = [q for q, _ in cases.values()]
    longest = max(e["n_pts"] for e in ref_run(tabs, qs))
    batch_equals(tabs, qs, pt_cap=longest + delta, host=delta < 0)


@pytest.mark.gpu
def test_gpu_kp_cap_4(plvi_lib):
    rng = np.random.default_rng(4)
    m = LoopMap(4)
    for _ in range(30):
        m.pt(bad=int(rng.uniform() < 0.1))
    for s in range(12):
        m.kf(rng.integers(-1, 30, rng.integers(0, 5)).tolist(), cov=rng.integers(0, 12, 6).tolist())
    tabs = m.tables()
    qs = [query(k, s) for s in range(12) for k in (PROJ, LAST)]
    qs += [query(BOW, s, 0, [int(rng.integers(0, 12))], rng.integers(-1, 5, (BOW_WIN, 5)), 5) for s in range(12)]
    batch_equals(tabs, qs, host=False)


@pytest.mark.gpu
def test_gpu_random_maps(plvi_lib):
    for seed in SEEDS:
        tabs, qs, exp = random_expected(seed, random_pt_cap(seed))
        batch_equals(tabs, qs, pt_cap=random_pt_cap(seed), host=seed < 2, exp=exp)


@pytest.mark.gpu
@pytest.mark.parametrize("n_queries", (1, 65))
def test_gpu_batch_sizes(plvi_lib, n_queries):
    tabs, qs, exp = random_expected(1, None)
    if n_queries == 1:
        for i in range(len(qs)):
            batch_equals(tabs, qs[i:i + 1], host=False, exp=exp[i:i + 1])
    else:
        batch_equals(tabs, (qs * 5)[:n_queries], host=False, exp=(exp * 5)[:n_queries])


@pytest.mark.gpu
def test_gpu_rows_cross_a_scan_tile_by_one(plvi_lib):
    """Three rows of 2731 entries laid end to end are 8193 positions: one more than a scan tile of 1024 threads x 8."""
    cap, n = 2731, 6000
    rng = np.random.default_rng(8193)
    m = LoopMap(cap)
    for _ in range(n):
        m.pt(bad=int(rng.uniform() < 0.05))
    a = m.kf(rng.integers(-1, n, cap).tolist())
    b = m.kf(rng.integers(-1, n, cap).tolist())
    last_new = n - 1     # the 8193rd position holds a point seen nowhere else
    m.pbad[last_new] = 0
    ids = rng.integers(-1, n - 1, cap)
    ids[-1] = last_new
    for t in (m.tab[a], m.tab[b]):
        t[:] = [v if v != last_new else -1 for v in t]
    c = m.kf(ids.tolist(), cov=[a, b])
    m.cand[a] = [b, c]
    tabs = m.tables()
    qs = [query(PROJ, c), query(LAST, c)]
    exp = ref_run(tabs, qs)
    assert exp[0]["pts"][exp[0]["n_pts"] - 1] == last_new and exp[0]["pts_kf"][exp[0]["n_pts"] - 1] == c
    batch_equals(tabs, qs, host=False, exp=exp)
    batch_equals(tabs, qs, pt_cap=exp[0]["n_pts"] - 1, gather=("desc",), host=False)


@pytest.mark.gpu
def test_gpu_null_optional_outputs(plvi_lib):
    tabs, cases = crafted()
    kf, pool = tabs
    qs = [q for q, _ in cases.values()]
    exp = ref_run(tabs, [dict(q, conn=[]) for q in qs])
    lw = plvi.LoopWindow(kf, dict(bad=pool["bad"]))       # a pool without rows
    cap = len(pool["bad"])
    got = lw.batch([q["kind"] for q in qs], [q["kf_slot"] for q in qs], cur_slot=None, connected=None, owners=False,
                   gather=(), pt_cap=cap, fill=FILL)
    assert got["rc"] == 0 and "pts_kf" not in got
    for i, (q, e) in enumerate(zip(qs, exp)):
        if q["kind"] == BOW and not 0 <= q["cur_slot"] < len(kf["bad"]):
            continue      # without cur_slot nothing is checked
        assert plain(got, i, q, cap) == dict({k: e[k] for k in SCALARS + ("win", "pts")}, pts_kf=[FILL] * cap), (i, q)
    with pytest.raises(ValueError):      # a gather needs its pool row
        lw.batch(PROJ, 0, gather=("pos",))


@pytest.mark.gpu
def test_gpu_limits_are_refused(plvi_lib):
    tabs, _ = crafted()
    kf, pool = tabs
    lw = plvi.LoopWindow(kf, pool)
    r = lw.batch([PROJ] * 65536, 0, pt_cap=1, gather=(), owners=False)
    assert r["rc"] == plvi.PLVI_E_CAPACITY and (r["n_win"] == FILL).all()
    assert plvi_lib.plvi_loop_window_scratch_bytes(-1, 5) == 0
    assert plvi_lib.plvi_loop_window_scratch_bytes(3, 100) == 256 + 3 * 400


@pytest.mark.gpu
def test_gpu_graph_capture_and_replay(plvi_lib):
    """Windows and merge captured into one hipGraph and replayed once: no host read, no allocation, no sync."""
    tabs, cases = crafted()
    qs = [q for q, _ in cases.values() if q["m12"] is not None]
    exp = ref_run(tabs, qs)
    kf, pool = tabs
    lw = plvi.LoopWindow(kf, pool)
    cap = len(pool["bad"])
    step, fetch = lw.batch([q["kind"] for q in qs], [q["kf_slot"] for q in qs], [q["cur_slot"] for q in qs],
                           [q["conn"] for q in qs], pt_cap=cap, gather=("pos", "desc"), fill=FILL, run=False)
    d = fetch()["dev"]
    sel, cap1, m12, n1 = merge_rows(qs, exp)
    mstep, mfetch = lw.merge_batch(d["win"], d["n_win"], d["abort_at"], m12, n1, fill=FILL, run=False)
    st = ctypes.c_void_p()
    assert plvi_lib.plvi_stream_create(ctypes.byref(st)) == 0
    rcs = []
    graph = plvi.StepGraph(lambda s: rcs.extend([step(s), mstep(s)]), st.value)
    assert rcs == [0, 0]
    assert (fetch()["n_win"] == FILL).all() and (mfetch()["num"] == FILL).all()   # captured, not run
    graph.launch()
    assert plvi_lib.plvi_stream_synchronize(st) == 0
    got, mg = fetch(), mfetch()
    for i, (q, e) in enumerate(zip(qs, exp)):
        assert plain(got, i, q, cap) == {k: e[k] for k in SCALARS + ("win", "pts", "pts_kf")}
        c = q["m12"].shape[1]
        assert int(mg["num"][i]) == e["num"] and mg["matched_mp"][i][:c].tolist() == e["matched_mp"][:c]
        assert mg["matched_kf"][i][:c].tolist() == e["matched_kf"][:c]


def chain_map(seed=11, K=14, cap=48, n=160):
    """Keyframes that observe shared MapPoints with near-equal descriptors: SearchByBoW finds real matches."""
    rng = np.random.default_rng(seed)
    m = LoopMap(cap)
    for _ in range(n):
        m.pt(bad=int(rng.uniform() < 0.05))
    base = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    desc = np.zeros((K, cap, 32), np.uint8)
    for s in range(K):
        ids = rng.permutation(n)[:cap - 4].tolist() + [-1] * 2
        m.kf(ids, bad=int(s == 5), cov=[int(v) for v in rng.permutation(K)[:int(rng.integers(2, 7))] if v != s])
        for i, p in enumerate(ids):
            desc[s, i] = base[p] if p >= 0 else rng.integers(0, 256, 32)
            desc[s, i, rng.integers(0, 32)] ^= 1 << int(rng.integers(0, 8))
    tabs = m.tables()
    kf, pool = tabs
    ids = kf["mp"]
    live = ((ids >= 0) & (pool["bad"][np.clip(ids, 0, n - 1)] == 0)).astype(np.uint8)
    # FeatureVector: node = point id % 16 (the NULL entries in node 16), as CSR per keyframe
    node_cap = 17
    node = np.tile(np.arange(node_cap, dtype=np.int32), (K, 1))
    off = np.zeros((K, node_cap + 1), np.int32)
    idx = np.zeros((K, cap), np.int32)
    for s in range(K):
        key = np.where(ids[s, :kf["nmp"][s]] >= 0, ids[s, :kf["nmp"][s]] % 16, 16)
        order = np.argsort(key, kind="stable")
        idx[s, :len(order)] = order
        off[s, 1:] = np.cumsum(np.bincount(key, minlength=node_cap))
    angle = np.zeros((K, cap), np.float32)
    return tabs, dict(desc=desc, angle=angle, live=live, n=kf["nmp"].copy(), node=node, off=off,
                      nnodes=np.full(K, node_cap, np.int32), idx=idx), node_cap


@pytest.mark.gpu
def test_gpu_chain_windows_bow_search_merge(plvi_lib):
    """windows(BOW) -> plvi_search_by_bow_kf_batch -> merge with nothing leaving the device in between: the pair
    tables are gathered with torch indexing from the window the first call wrote."""
    import torch
    tabs, feat, node_cap = chain_map()
    kf, pool = tabs
    K, cap = kf["mp"].shape
    dev = "cuda:0"
    T = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in feat.items()}
    cur, cands = 0, [3, 5, 7, 9, 11]          # 5 is bad: no window
    B = len(cands)
    conn = [[], [], [int(kf["cand"][7, 1])], [], []]
    lw = plvi.LoopWindow(kf, pool)
    step, fetch = lw.batch([BOW] * B, cands, cur, conn, pt_cap=1, gather=(), fill=FILL, run=False)
    assert step() == 0
    r = fetch()
    d = r["dev"]
    win = torch.zeros((B + 1, WIN_MAX), dtype=torch.int32, device=dev)
    plvi_lib.plvi_memcpy(ctypes.c_void_p(win.data_ptr()), ctypes.c_void_p(d["win"]), win.numel() * 4, 3)
    # pair p = 6 q + j: KF1 = the current keyframe, KF2 = win[q][j] (a slot outside the map reads slot 0: the
    # merge never reads that pair's row)
    slots = win[:B, :BOW_WIN].reshape(-1).long()
    slots = torch.where((slots >= 0) & (slots < K), slots, torch.zeros_like(slots))
    one = torch.full((B * BOW_WIN,), cur, dtype=torch.long, device=dev)
    names = ("desc", "angle", "live", "n", "node", "off", "nnodes", "idx")
    kf1 = [T[k][one].contiguous() for k in names]
    kf2 = [T[k][slots].contiguous() for k in names]
    m12 = torch.full((B + 1, BOW_WIN, cap), FILL, dtype=torch.int32, device=dev)
    nm = torch.zeros(B * BOW_WIN + 1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    plvi.search_by_bow_kf_batch(B * BOW_WIN, 0.75, False, cap, cap, node_cap, [t.data_ptr() for t in kf1],
                                [t.data_ptr() for t in kf2], m12.data_ptr(), nm.data_ptr())
    n1 = torch.full((B,), int(kf["nmp"][cur]), dtype=torch.int32, device=dev)
    mg = lw.merge_batch(d["win"], d["n_win"], d["abort_at"], m12.data_ptr(), n1.data_ptr(), n_queries=B, cap1=cap,
                        fill=FILL)
    assert mg["rc"] == 0
    torch.cuda.synchronize()
    host_m12 = m12.cpu().numpy()
    qs = [query(BOW, c, cur, conn[i], host_m12[i], int(kf["nmp"][cur])) for i, c in enumerate(cands)]
    exp = ref_run(tabs, qs, pt_cap=1)
    assert exp[1]["n_win"] == 0 and exp[2]["abort_at"] >= 0
    assert sum(e["num"] for e in exp) >= 40, [e["num"] for e in exp]     # the searches found real matches
    for i, e in enumerate(exp):
        assert (int(r["n_win"][i]), int(r["abort_at"][i]), r["win"][i].tolist()) == (e["n_win"], e["abort_at"], e["win"])
        assert int(mg["num"][i]) == e["num"]
        assert mg["matched_mp"][i].tolist() == e["matched_mp"] and mg["matched_kf"][i].tolist() == e["matched_kf"]


@pytest.mark.gpu
def test_gpu_chain_proj_gathered_rows(plvi_lib):
    """windows(PROJ) -> gathered rows: they are the pool rows of pts, in f21's layouts."""
    tabs, _, _ = chain_map(seed=12, cap=120, n=900)
    qs = [query(PROJ, s) for s in range(14)]
    qs = [q for q, e in zip(qs, ref_run(tabs, qs)) if e["n_pts"] > 257][:3]
    assert len(qs) == 3                             # more than one chunk of the gather
    qs.append(query(LAST, qs[0]["kf_slot"]))
    exp = ref_run(tabs, qs)
    batch_equals(tabs, qs, host=False, exp=exp)
    batch_equals(tabs, qs, pt_cap=257, host=False)
