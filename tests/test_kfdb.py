"""KeyFrameDatabase (src/KeyFrameDatabase.cc) on the device (csrc/kfdb.hip): plvi_kfdb_add[_batch], _erase,
_clear_map, _clear and the two live detectors, plvi_kfdb_query[_batch] mode 0 = DetectRelocalizationCandidates
(:790-902) and mode 1 = DetectNBestCandidates (:619-787).

Expected values come from tests/native/kfdb_ref.cpp, a sequential host restatement in the reference's own shape (an
inverted file of std::list, stamp / words / score members that persist, std::map BowVectors, L1Scoring::score as
written, std::list::sort(compFirst)).  The CPU part pins it against NpDB below, an independent numpy restatement in
the FORWARD formulation -- set intersections, the (first shared word, add sequence) key, a stable argsort -- so the
two formulations cross-check the encounter-order claim of the header, on every crafted case and on a seeded general
case that must keep exercising what it is there for (the assertions of test_general_case_conditions).  The gpu part
demands exact equality with the restatement: the word counts, the double scores bit for bit (unwritten cells keep
their NaN fill), the list order and the candidate lists, with sentinel-filled outputs so that nothing is written
past a count or a capacity."""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import plvi

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "kfdb_ref.cpp"
BUILD = ROOT / "tests" / "native" / "_build"
FILL = -7
E_BADARG, E_CAPACITY, E_OVERFLOW = -2, -3, -5

_lib = None
_cache = {}


def ref_lib():
    global _lib
    if _lib is None:
        so = BUILD / "libkfdb_ref.so"
        if not so.exists() or so.stat().st_mtime < SRC.stat().st_mtime:
            so.parent.mkdir(parents=True, exist_ok=True)
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                            "-o", str(so), str(SRC)], check=True)
        _lib = ctypes.CDLL(str(so))
        V, I = ctypes.c_void_p, ctypes.c_int
        _lib.kfdb_ref_create.argtypes, _lib.kfdb_ref_create.restype = [I, I], V
        _lib.kfdb_ref_destroy.argtypes, _lib.kfdb_ref_destroy.restype = [V], None
        _lib.kfdb_ref_add.argtypes, _lib.kfdb_ref_add.restype = [V, I, I, V, V, I], I
        _lib.kfdb_ref_erase.argtypes, _lib.kfdb_ref_erase.restype = [V, I], None
        _lib.kfdb_ref_clear_map.argtypes, _lib.kfdb_ref_clear_map.restype = [V, I], None
        _lib.kfdb_ref_clear.argtypes, _lib.kfdb_ref_clear.restype = [V], None
        _lib.kfdb_ref_query.argtypes, _lib.kfdb_ref_query.restype = [V, V, V, I, I, I, I, V, I] + [V] * 2 + [I] + [V] * 13, None
    return _lib


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def bow(words, values=None):
    """(ascending uint32 words, float64 values); the default values are L1-normalised and all different."""
    w = np.array(sorted(words), np.uint32)
    if values is None:
        values = np.arange(1, len(w) + 1, dtype=np.float64) + 0.25
        values /= max(values.sum(), 1)
    return w, np.asarray(values, np.float64)


class RefDB:
    """tests/native/kfdb_ref.cpp."""

    def __init__(self, n_words, slot_cap):
        self.S, self.lib = slot_cap, ref_lib()
        self.h = self.lib.kfdb_ref_create(n_words, slot_cap)

    def __del__(self):
        self.lib.kfdb_ref_destroy(self.h)

    def add(self, slot, b, map_id):
        w, v = b
        return self.lib.kfdb_ref_add(self.h, slot, map_id, _p(w), _p(v), len(w))

    def erase(self, slot):
        self.lib.kfdb_ref_erase(self.h, slot)

    def clear_map(self, m):
        self.lib.kfdb_ref_clear_map(self.h, m)

    def clear(self):
        self.lib.kfdb_ref_clear(self.h)

    def query(self, b, qmap, mode, n_best, conn, covis, bad):
        S = self.S
        w, v = b
        conn = np.array(sorted(conn), np.int32)
        words, score = np.zeros(S, np.int32), np.full(S, np.nan)
        order, a_, b_ = (np.zeros(S + 1, np.int32) for _ in range(3))
        es, eb, ea = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.float32)
        cnt = [ctypes.c_int() for _ in range(4)]
        diag = np.zeros(2, np.int32)
        bad = None if bad is None else np.ascontiguousarray(bad, np.uint8)
        self.lib.kfdb_ref_query(self.h, _p(w), _p(v), len(w), qmap, mode, n_best, _p(conn), len(conn), _p(covis),
                                _p(bad), 0 if bad is None else len(bad), _p(words), _p(score), _p(order),
                                ctypes.byref(cnt[0]), _p(a_), ctypes.byref(cnt[1]), _p(b_), ctypes.byref(cnt[2]),
                                _p(es), _p(ea), _p(eb), ctypes.byref(cnt[3]), _p(diag))
        no, na, nb, ne = (c.value for c in cnt)
        return dict(words=words, score=score, order=order[:no].tolist(), a=a_[:na].tolist(), b=b_[:nb].tolist(),
                    ent_slot=es[:ne].tolist(), ent_acc=ea[:ne].copy(), ent_best=eb[:ne].tolist(), dup=int(diag[0]),
                    stale=int(diag[1]))


class NpDB:
    """The independent restatement, forward formulation: no inverted file, no list."""

    def __init__(self, n_words, slot_cap):
        self.S, self.kf, self.seq = slot_cap, {}, 0
        self.order_sensitive = 0  # scored pairs whose sum differs between ascending and descending word order

    def add(self, slot, b, map_id):
        if not 0 <= slot < self.S or slot in self.kf:
            return E_BADARG
        self.kf[slot] = dict(w=b[0], v=b[1], map=map_id, seq=self.seq, m=[np.float32(0), np.float32(0)])
        self.seq += 1
        return 0

    def erase(self, slot):
        self.kf.pop(slot, None)

    def clear_map(self, m):
        self.kf = {s: k for s, k in self.kf.items() if k["map"] != m}

    def clear(self):
        self.kf = {}

    def query(self, b, qmap, mode, n_best, conn, covis, bad):
        w, v = b
        share = {}
        for s, k in self.kf.items():
            if mode == 1 and s in conn:
                continue
            common, iq, ik = np.intersect1d(w, k["w"], return_indices=True)
            if len(common):
                share[s] = (len(common), int(common[0]), iq, ik)
        words, score = np.full(self.S, -1, np.int32), np.full(self.S, np.nan)
        res = dict(words=words, score=score, order=[], a=[], b=[])
        if not share:
            return res
        slots = np.array(list(share))
        key = np.lexsort(([self.kf[s]["seq"] for s in slots], [share[s][1] for s in slots]))
        order = [int(s) for s in slots[key]]
        res["order"] = order
        for s in order:
            words[s] = share[s][0]
        minc = int(np.float32(max(c[0] for c in share.values())) * np.float32(0.8))
        scored = [s for s in order if share[s][0] > minc]
        for s in scored:
            _, _, iq, ik = share[s]
            terms = [(abs(a - c) - abs(a)) - abs(c) for a, c in zip(v[iq].tolist(), self.kf[s]["v"][ik].tolist())]
            up = down = 0.0
            for t in terms:
                up += t
            for t in reversed(terms):
                down += t
            self.order_sensitive += up != down
            score[s] = -up * 0.5
            self.kf[s]["m"][mode] = np.float32(score[s])
        acc, best = [], []
        for s in scored:
            a = top = self.kf[s]["m"][mode]
            bs = s
            for nb in ([] if covis is None else covis[s].tolist()):
                if nb < 0:
                    break
                if nb not in share:
                    continue
                m = self.kf[nb]["m"][mode]
                a = np.float32(a + m)
                if m > top:
                    bs, top = nb, m
            acc.append(a)
            best.append(bs)
        acc = np.array(acc, np.float32)
        if mode == 0:
            retain = np.float32(0.75) * max(np.float32(0), acc.max())
            for a, bs in zip(acc, best):
                if a > retain and self.kf[bs]["map"] == qmap and bs not in res["a"]:
                    res["a"].append(bs)
            return res
        seen = set()
        for j in np.argsort(-acc, kind="stable"):
            bs = best[j]
            if bs in seen:
                continue
            seen.add(bs)
            m = self.kf[bs]["map"]
            if m == qmap:
                if len(res["a"]) < n_best:
                    res["a"].append(bs)
            elif len(res["b"]) < n_best and not (bad is not None and 0 <= m < len(bad) and bad[m]):
                res["b"].append(bs)
        return res


class Case:
    def __init__(self, n_words, slot_cap, word_cap):
        self.n_words, self.slot_cap, self.word_cap, self.ops = n_words, slot_cap, word_cap, []

    def add(self, *entries):  # (slot, bow, map id), added in this order by one batch call
        self.ops.append(("add", list(entries)))

    def erase(self, *slots):
        self.ops.append(("erase", list(slots)))

    def clear_map(self, m):
        self.ops.append(("clear_map", m))

    def clear(self):
        self.ops.append(("clear",))

    def query(self, bows, maps, mode, n_best=3, connected=None, covis=None, bad=None, cand_cap=None, counts=None):
        self.ops.append(("query", dict(bows=bows, maps=maps, mode=mode, n_best=n_best, connected=connected,
                                       covis=covis, bad=bad, cand_cap=cand_cap, counts=counts)))


def clamped(q):
    """The queries as the count contract reads them."""
    if q["counts"] is None:
        return q["bows"]
    return [(w[:max(min(c, len(w)), 0)], v[:max(min(c, len(w)), 0)]) for (w, v), c in zip(q["bows"], q["counts"])]


def run_host(case, cls):
    """Every query's result, in order, from RefDB or NpDB; returns (results, db)."""
    db, out = cls(case.n_words, case.slot_cap), []
    for op in case.ops:
        if op[0] == "add":
            for slot, b, m in op[1]:
                assert db.add(slot, b, m) == 0
        elif op[0] == "erase":
            for s in op[1]:
                db.erase(s)
        elif op[0] == "clear_map":
            db.clear_map(op[1])
        elif op[0] == "clear":
            db.clear()
        else:
            q = op[1]
            for i, b in enumerate(clamped(q)):
                conn = set(q["connected"][i]) if q["connected"] is not None else set()
                r = db.query(b, q["maps"][i], q["mode"], q["n_best"], conn, q["covis"], q["bad"])
                r["mode"] = q["mode"]
                out.append(r)
    return out, db


def run_gpu(case, split=False):
    """The same through plvi.KeyFrameDatabase; split=True issues every query of a batch as a call of its own."""
    db, out = plvi.KeyFrameDatabase(case.n_words, case.slot_cap, case.word_cap), []
    for op in case.ops:
        if op[0] == "add":
            assert db.add_many([e[0] for e in op[1]], [e[1] for e in op[1]], [e[2] for e in op[1]]) == 0
        elif op[0] == "erase":
            db.erase(op[1])
        elif op[0] == "clear_map":
            db.clearMap(op[1])
        elif op[0] == "clear":
            db.clear()
        else:
            q = op[1]
            n = len(q["bows"])
            for lo, hi in ([(i, i + 1) for i in range(n)] if split else [(0, n)]):
                o = db.query_arrays(q["bows"][lo:hi], q["maps"][lo:hi], q["mode"], n_best=q["n_best"],
                                    connected=None if q["connected"] is None else q["connected"][lo:hi],
                                    covis=q["covis"], map_bad=q["bad"], cand_cap=q["cand_cap"],
                                    q_cap=max(len(b[0]) for b in q["bows"]) or 1,
                                    counts=None if q["counts"] is None else q["counts"][lo:hi], fill=FILL)
                for i in range(hi - lo):
                    r = dict(words=o["words"][i], score=o["score"][i], mode=q["mode"])
                    no = int(o["norder"][i])
                    r["order"], r["order_tail"] = o["order"][i][:no].tolist(), o["order"][i][no:]
                    if q["mode"] == 0:
                        r["na"] = int(o["ncand"][i])
                        w = min(r["na"], o["cand"].shape[1] if q["cand_cap"] is None else q["cand_cap"])
                        r["a"], r["a_tail"], r["b"] = o["cand"][i][:w].tolist(), o["cand"][i][w:], []
                    else:
                        na, nb = int(o["nloop"][i]), int(o["nmerge"][i])
                        r["a"], r["a_tail"] = o["loop"][i][:na].tolist(), o["loop"][i][na:]
                        r["b"], r["b_tail"] = o["merge"][i][:nb].tolist(), o["merge"][i][nb:]
                    out.append(r)
    assert db.errors() == 0
    return out


def same_host(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert np.array_equal(g["words"], e["words"])
        assert g["score"].tobytes() == e["score"].tobytes()
        assert g["order"] == e["order"] and g["a"] == e["a"] and g["b"] == e["b"]


def same_gpu(got, exp, cand_caps=None):
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert np.array_equal(g["words"], e["words"]), i
        assert g["score"].tobytes() == e["score"].tobytes(), i  # bit for bit; unwritten cells keep the NaN fill
        assert g["order"] == e["order"], i
        assert (g["order_tail"] == FILL).all()
        cap = None if cand_caps is None else cand_caps[i]
        if g["mode"] == 0:
            assert g["na"] == len(e["a"]), i  # the full count
            assert g["a"] == (e["a"] if cap is None else e["a"][:cap]), i
        else:
            assert g["a"] == e["a"] and g["b"] == e["b"], i
            assert (g["b_tail"] == FILL).all()
        assert (g["a_tail"] == FILL).all()


# ------------------------------------------------------------------ cases

def general_case(seed=5):
    """About 200 keyframes of 1-180 words over 600, 3 maps, a random 10-neighbour table, 8 queries of 150 words;
    both modes, the queries of a mode as one batch.  Ten keyframes are erased and five slots filled again."""
    if ("general", seed) in _cache:
        return _cache["general", seed]
    rng = np.random.default_rng(seed)
    S, W = 208, 600
    c = Case(W, S, 180)

    def rand_bow(n):
        w = np.sort(rng.choice(W, n, replace=False)).astype(np.uint32)
        v = rng.random(n) + 0.05
        return w, v / v.sum()

    def size():  # 1-180 words, most keyframes near the top as most of a map's keyframes are full ones
        return int(np.clip(180 - rng.exponential(35), 1, 180))

    slots = rng.permutation(S)[:200]
    c.add(*[(int(s), rand_bow(size()), int(rng.integers(0, 3))) for s in slots])
    gone = [int(s) for s in slots[:10]]
    c.erase(*gone)
    c.add(*[(s, rand_bow(int(rng.integers(100, 181))), int(rng.integers(0, 3))) for s in gone[:5]])
    # neighbours: mostly nearby slots, as a covisibility graph's are; short rows end with -1
    covis = np.full((S, 10), -1, np.int32)
    for s in range(S):
        k = int(rng.integers(4, 11))
        near = (s + rng.integers(-12, 13, k)) % S
        far = rng.integers(0, S, k)
        covis[s, :k] = np.where(rng.random(k) < 0.7, near, far)
    queries = [rand_bow(150) for _ in range(8)]
    maps = [int(m) for m in rng.integers(0, 3, 8)]
    c.query(queries, maps, 0, covis=covis)
    conn = [set(int(x) for x in rng.integers(0, S, 6)) for _ in range(8)]
    c.query(queries, maps, 1, n_best=3, connected=conn, covis=covis, bad=[0, 0, 1])
    _cache["general", seed] = c
    return c


def sizes_case(mode):
    """Slots of 0, 1, 63, 64, 65 and word_cap words; an empty query, one sharing nothing, q_cap-full ones, and
    counts outside [0, q_cap]."""
    cap = 130
    c = Case(1000, 8, cap)
    ns = [0, 1, 63, 64, 65, cap]
    c.add(*[(i, bow(range(3 * i, 3 * i + 2 * n, 2)), i % 2) for i, n in enumerate(ns)])
    full = bow(range(0, 2 * cap, 2))
    odd = bow(range(1, 2 * cap, 2))          # shares with slots 1, 3 and 5 only, full with 2 and 4
    nothing = bow(range(600, 600 + cap))
    covis = np.full((8, 10), -1, np.int32)
    covis[5, :3] = [4, 0, 3]
    covis[4, :2] = [7, 5]
    c.query([full, odd, nothing, full, full, odd], [0, 1, 0, 0, 1, 0], mode, covis=covis,
            counts=[cap, cap, cap, -3, cap + 1000, 0])
    c.query([bow([])], [0], mode, covis=covis)
    return c


def threshold_case(mode):
    """maxCommonWords 10, 7 and 5 (minCommonWords 8, 5 and 4): per query a slot at the maximum, one exactly at the
    threshold (not scored) and one just above it (scored)."""
    c = Case(1000, 12, 40)
    ent = []
    for qi, (base, mx, at, above) in enumerate(((0, 10, 8, 9), (100, 7, 5, 6), (200, 5, 4, 5))):
        for j, k in enumerate((at, mx, above)):
            private = range(500 + 40 * (3 * qi + j), 500 + 40 * (3 * qi + j) + 7 + j)
            ent.append((3 * qi + j, bow(list(range(base, base + k)) + list(private)), 0))
    c.add(*ent)
    qs = [bow(range(0, 10)), bow(range(100, 107)), bow(range(200, 205))]
    c.query(qs, [0, 0, 0], mode)
    return c


def order_case():
    """Every slot shares the query's first word and has the same vector, so the list order is the add order: slots
    added in a permuted order, two erased, one added back into a freed slot -- it now comes last."""
    c = Case(100, 10, 8)
    b = bow([5, 9, 12])
    c.add(*[(s, b, 0) for s in (7, 2, 9, 0, 4, 3)])
    c.erase(2, 0)
    c.add((2, b, 0))
    c.query([bow([5, 9, 12, 40])], [0], 0)
    c.query([bow([5, 9, 12, 40])], [0], 1)
    return c, [7, 9, 4, 3, 2]


def clear_case():
    c = Case(100, 9, 8)
    c.add(*[(s, bow([s % 3, 10, 11 + s]), s % 3) for s in range(9)])
    q = [bow([0, 1, 2, 10, 13])]
    c.query(q, [0], 0)
    c.clear_map(1)
    c.query(q, [0], 0)
    c.query(q, [2], 1, n_best=3)
    c.clear()
    c.query(q, [0], 0)
    c.add(*[(s, bow([s % 3, 10, 11 + s]), 0) for s in (4, 1)])
    c.query(q, [0], 0)
    return c


def ties_case():
    """Two slots with identical vectors and no neighbours: equal accScore, list order kept; n_best 1 and 3."""
    c = Case(100, 6, 8)
    same = bow([3, 4, 8])
    c.add((4, same, 0), (1, same, 0), (2, bow([3, 4, 9]), 0), (5, same, 1), (0, same, 1))
    for nb in (1, 3):
        c.query([bow([3, 4, 8, 20])], [0], 1, n_best=nb)
    return c


def stale_case(mode):
    """q0 scores B.  In q1 B shares one word, fails the threshold and is a neighbour of A: A's accScore takes B's
    member as q0 left it."""
    c = Case(200, 4, 16)
    A, B = 1, 3
    c.add((A, bow(range(100, 110)), 0), (B, bow(list(range(0, 10)) + [100]), 0))
    covis = np.full((4, 10), -1, np.int32)
    covis[A, 0] = B
    q0, q1 = bow(range(0, 12)), bow(range(100, 112))
    c.query([q0, q1], [0, 0], mode, covis=covis)
    return c


def mode1_case(n_best):
    """A connected keyframe excluded from the list and skipped as a neighbour, loop full while merge still fills,
    a bad map."""
    c = Case(100, 12, 8)
    ent = []
    for s in range(12):
        # distinct scores: slot s shares 4 words, values differ
        w = [1, 2, 3, 4, 30 + s]
        v = np.array([1 + 0.1 * s, 2, 3, 4, 5 + s], np.float64)
        ent.append((s, (np.array(w, np.uint32), v / v.sum()), [0, 0, 0, 0, 0, 1, 2, 1, 2, 1, 1, 0][s]))
    c.add(*ent)
    covis = np.full((12, 10), -1, np.int32)
    covis[0, :3] = [11, 5, 3]   # 11 is connected: skipped; 5 shares words
    covis[6, :2] = [8, 7]
    covis[2, :1] = [0]
    q = (np.array([1, 2, 3, 4, 50], np.uint32), np.array([0.1, 0.2, 0.3, 0.3, 0.1]))
    c.query([q, q], [0, 1], 1, n_best=n_best, connected=[{11, 4}, {9}], covis=covis, bad=[0, 0, 1])
    return c


def mode0_case():
    """cand_cap below the count, a pBestKF of another map named twice (dropped by the map filter, never added),
    and one of the query's map named twice (added once)."""
    c = Case(100, 10, 8)
    ent = []
    for s in range(10):
        v = np.array([1 + 0.05 * s, 2, 3, 4], np.float64)
        ent.append((s, (np.array([1, 2, 3, 60 + s], np.uint32), v / v.sum()), 1 if s == 9 else 0))
    c.add(*ent)
    covis = np.full((10, 10), -1, np.int32)
    for s in (7, 6):
        covis[s, 0] = 9      # 9 scores best and is of map 1
    for s in (1, 2, 3):
        covis[s, 0] = 8      # 8 scores better than 1-3 and is of map 0
    for s in (4, 5):
        covis[s, 0] = 0      # a neighbour that scores worse: pBestKF stays, accScore is a sum of two like the others
    q = (np.array([1, 2, 3], np.uint32), np.array([0.2, 0.3, 0.5]))
    c.query([q], [0], 0, covis=covis)
    c.query([q], [0], 0, covis=covis, cand_cap=2)
    c.query([q], [0], 0, covis=covis, cand_cap=0)
    return c


def wide_case():
    """slot_cap above 8192: the sharing list is sorted in global scratch, not in LDS; 300 keyframes of 1-4 words
    over 30 in scattered slots, the last slot among them."""
    rng = np.random.default_rng(3)
    S = 8200
    c = Case(30, S, 4)
    slots = [int(s) for s in rng.permutation(S - 1)[:299]] + [S - 1]
    c.add(*[(s, bow(rng.choice(30, int(rng.integers(1, 5)), replace=False)), int(rng.integers(0, 2)))
            for s in slots])
    covis = np.full((S, 10), -1, np.int32)
    for s in slots:
        covis[s, :3] = rng.choice(slots, 3)
    qs = [bow(rng.choice(30, 6, replace=False)) for _ in range(2)]
    c.query(qs, [0, 1], 0, covis=covis)
    c.query(qs, [0, 1], 1, connected=[set(slots[:4]), set()], covis=covis, bad=[0, 0])
    return c


CASES = {
    "sizes0": lambda: sizes_case(0), "sizes1": lambda: sizes_case(1),
    "threshold0": lambda: threshold_case(0), "threshold1": lambda: threshold_case(1),
    "order": lambda: order_case()[0], "clear": clear_case, "ties": ties_case,
    "stale0": lambda: stale_case(0), "stale1": lambda: stale_case(1),
    "mode1_n1": lambda: mode1_case(1), "mode1_n3": lambda: mode1_case(3), "mode0": mode0_case,
    "general": general_case, "wide": wide_case,
}


def expected(name):
    if name not in _cache:
        _cache[name] = run_host(CASES[name](), RefDB)[0]
    return _cache[name]


def cand_caps(case):
    return [op[1]["cand_cap"] for op in case.ops if op[0] == "query" for _ in op[1]["bows"]]


# ------------------------------------------------------------------ CPU part

@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_forward_numpy(name):
    same_host(run_host(CASES[name](), NpDB)[0], expected(name))


def test_general_case_conditions():
    res = expected("general")
    _, npdb = run_host(general_case(), NpDB)
    # the double sum depends on the order of its terms
    assert npdb.order_sensitive >= 50, npdb.order_sensitive
    for r in res:
        n_list, n_pass = len(r["order"]), int(np.isfinite(r["score"]).sum())
        assert n_pass >= 5 and n_list - n_pass >= 5, (n_list, n_pass)
        assert n_pass == len(r["ent_slot"])
    assert sum(b != s for r in res for s, b in zip(r["ent_slot"], r["ent_best"])) >= 10
    assert sum(r["dup"] for r in res) >= 3
    # a stale member changes an accScore: a non-zero member of a neighbour this query did not score was added
    assert sum(r["stale"] for r in res) >= 1
    odd = 0
    for r in res:
        if r["mode"] == 0 and len(r["a"]) >= 3:
            sc = [float(np.float32(r["score"][s])) if np.isfinite(r["score"][s]) else -1.0 for s in r["a"]]
            odd += r["a"] != sorted(r["a"]) and sc != sorted(sc, reverse=True)
    assert odd >= 1


def test_crafted_cases_say_what_they_claim():
    r = expected("threshold0")
    for qi, (at, mx, above) in enumerate(((8, 10, 9), (5, 7, 6), (4, 5, 5))):
        w, sc = r[qi]["words"], r[qi]["score"]
        assert [int(w[3 * qi + j]) for j in range(3)] == [at, mx, above]
        assert [bool(np.isfinite(sc[3 * qi + j])) for j in range(3)] == [False, True, True]
    case, order = order_case()
    r = expected("order")
    assert r[0]["order"] == order and r[0]["a"] == order          # the slot added back comes last
    assert r[1]["a"] == order[:3]                                  # equal accScore: the stable sort keeps list order
    r = expected("ties")
    assert r[0]["a"] == [4] and r[1]["a"] == [4, 1] and r[1]["b"] == [5, 0]
    for name in ("stale0", "stale1"):
        r = expected(name)
        A, B = 1, 3
        assert np.isfinite(r[0]["score"][B]) and r[1]["words"][B] == 1 and np.isnan(r[1]["score"][B])
        assert r[1]["stale"] == 1 and r[1]["ent_best"] == [B if r[0]["score"][B] > r[1]["score"][A] else A]
        assert r[1]["ent_acc"][0] == np.float32(r[1]["score"][A]) + np.float32(r[0]["score"][B])
    r = expected("mode1_n3")
    assert 11 not in r[0]["order"] and 4 not in r[0]["order"] and r[0]["words"][11] == -1
    assert len(r[0]["a"]) == 3 and 0 < len(r[0]["b"]) <= 3          # loop full, merge still fills
    maps = [0, 0, 0, 0, 0, 1, 2, 1, 2, 1, 1, 0]
    assert all(maps[s] == 1 for s in r[0]["b"])                    # map 2 is bad
    assert all(maps[s] == 0 for s in r[1]["b"])                    # the query of map 1 merges with map 0 only
    r = expected("mode1_n1")
    assert len(r[0]["a"]) == 1 and len(r[0]["b"]) == 1
    r = expected("mode0")
    assert 9 in r[0]["ent_best"] and r[0]["ent_best"].count(9) >= 2 and 9 not in r[0]["a"]
    assert r[0]["ent_best"].count(8) >= 3 and r[0]["a"].count(8) == 1 and r[0]["dup"] >= 2
    assert len(r[0]["a"]) > 2
    r = expected("sizes0")
    ns = [0, 1, 63, 64, 65, 130]
    own = [set(range(3 * i, 3 * i + 2 * n, 2)) for i, n in enumerate(ns)]
    for qi, q in ((0, set(range(0, 260, 2))), (1, set(range(1, 260, 2)))):
        common = [len(o & q) for o in own]
        assert [int(x) for x in r[qi]["words"][:6]] == [c if c else -1 for c in common]
    assert r[1]["words"][5] > 64 and r[0]["words"][4] == 65
    assert (r[2]["words"] == -1).all() and (r[3]["words"] == -1).all() and (r[5]["words"] == -1).all()
    assert np.array_equal(r[4]["words"], r[0]["words"])            # a count above q_cap reads as q_cap
    assert (r[6]["words"] == -1).all()


# ------------------------------------------------------------------ gpu part

@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_restatement(plvi_lib, name):
    case = CASES[name]()
    same_gpu(run_gpu(case), expected(name), cand_caps(case))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["stale0", "stale1", "general"])
def test_batch_equals_single_calls(plvi_lib, name):
    case = CASES[name]()
    same_gpu(run_gpu(case, split=True), expected(name), cand_caps(case))


@pytest.mark.gpu
def test_python_mirror_and_synchronous_entry_points(plvi_lib):
    """add / DetectRelocalizationCandidates / DetectNBestCandidates of the mirror go through plvi_kfdb_add and
    plvi_kfdb_query."""
    case = mode1_case(3)
    q = case.ops[1][1]
    exp = expected("mode1_n3")
    db = plvi.KeyFrameDatabase(case.n_words, case.slot_cap, case.word_cap)
    for slot, b, m in case.ops[0][1]:
        db.add(slot, b, m)
    for i in range(2):
        loop, merge = db.DetectNBestCandidates(q["bows"][i], q["maps"][i], q["connected"][i], 3, q["covis"], q["bad"])
        assert loop == exp[i]["a"] and merge == exp[i]["b"]
    case = mode0_case()
    exp = expected("mode0")
    db = plvi.KeyFrameDatabase(case.n_words, case.slot_cap, case.word_cap)
    for slot, b, m in case.ops[0][1]:
        db.add(slot, {int(w): float(v) for w, v in zip(*b)}, m)
    q = case.ops[1][1]
    assert db.DetectRelocalizationCandidates(q["bows"][0], 0, q["covis"]) == exp[0]["a"]
    assert db.DetectRelocalizationCandidates(q["bows"][0], 0, q["covis"], cand_cap=2) == exp[0]["a"][:2]
    assert db.DetectRelocalizationCandidates(q["bows"][0], 0) == run_host_one(case, q["bows"][0])


def run_host_one(case, b):
    c = Case(case.n_words, case.slot_cap, case.word_cap)
    c.ops = [case.ops[0]]
    c.query([b], [0], 0)
    return run_host(c, RefDB)[0][0]["a"]


@pytest.mark.gpu
def test_bad_arguments_and_the_error_word(plvi_lib):
    with pytest.raises(plvi.PlviError) as e:
        plvi.KeyFrameDatabase(100, 4, 8, scoring=1)  # L2_NORM
    assert e.value.code == E_BADARG
    with pytest.raises(plvi.PlviError) as e:
        plvi.KeyFrameDatabase(100, 4, plvi.KFDB_MAX_WORDS + 1)
    assert e.value.code == E_CAPACITY
    db = plvi.KeyFrameDatabase(100, 4, 8)
    db.add(2, bow([1, 2, 3]), 0)
    for slot in (2, 4, -1):  # occupied, out of range
        with pytest.raises(plvi.PlviError) as e:
            db.add(slot, bow([1, 2]), 0)
        assert e.value.code == E_BADARG
    with pytest.raises(plvi.PlviError) as e:
        db.add_many([0, 0], [bow([1]), bow([2])], [0, 0])  # a slot named twice: nothing is added
    assert e.value.code == E_BADARG
    with pytest.raises(plvi.PlviError) as e:
        db.erase([4])
    assert e.value.code == E_BADARG
    db.erase([1])  # an empty slot is left alone
    assert db.DetectRelocalizationCandidates(bow([1, 2, 3]), 0) == [2]
    # a count above word_cap: clamped, and bit 0 of the error word; the slot holds the first word_cap words
    long = bow(range(10, 22))
    assert db.add_many([0], [long], [0]) == 1 and db.errors() == 0
    ref = Case(100, 4, 8)
    ref.add((2, bow([1, 2, 3]), 0), (0, (long[0][:8], long[1][:8]), 0))
    ref.query([bow(range(10, 30))], [0], 0)
    exp = run_host(ref, RefDB)[0][0]
    got = db.query_arrays([bow(range(10, 30))], [0], 0, fill=FILL)
    assert np.array_equal(got["words"][0], exp["words"]) and got["score"][0].tobytes() == exp["score"].tobytes()
    with pytest.raises(plvi.PlviError) as e:
        db.add(1, long, 0)
    assert e.value.code == E_OVERFLOW
    assert db.add_many([3], [bow([99, 100])], [0]) == 2  # a word id >= n_words
