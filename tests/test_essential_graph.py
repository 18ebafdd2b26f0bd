"""The essential graph on the device (csrc/essential_graph.hip): plvi_loop_correct, plvi_loop_connections and
plvi_essential_graph -- the corrected window with the correction owners, LoopConnections, and the vertices, the
ordered edge list and the feature references of LoopClosing::CorrectLoop[WithLines] and
Optimizer::OptimizeEssentialGraph[4DoF].

Expected values come from tests/native/essential_graph_ref.cpp, a sequential restatement in the reference's own
shape.  The CPU part pins it against np_correct / np_graph / np_connections below, an independent formulation in
positions and ranks (np.unique(return_index), np.isin; no sets, no objects), on every crafted case and on random
maps, asserts what each crafted case is there to show, and asserts the coverage of the random maps from the
restatement's own outputs.  The gpu part demands exact equality with the restatement for every output of both forms,
with sentinel-filled tables."""
import ctypes
import functools
import pathlib
import subprocess

import numpy as np
import pytest

import plvi

ROOT = pathlib.Path(__file__).resolve().parent.parent
NATIVE = ROOT / "tests" / "native"
SRC = NATIVE / "essential_graph_ref.cpp"
BUILD = NATIVE / "_build"
FILL = -7
OUT = 1 << 20  # a keyframe slot outside every map
LOOPCONN, TREE, LOOP, COVIS, INERTIAL = range(5)
E_WIN, E_PTS, E_LNS, E_QUERY, E_VERT, E_EDGE, E_NOV, E_LC = (1 << i for i in range(8))
D7, D4 = 0, 1
i32 = np.int32


# ------------------------------------------------------------------ the map
def make_map(K, kp_cap=4, kl_cap=3, C=8, n_pts=0, n_lns=0):
    """Empty tables of K good keyframes in one map, slot order = address order, kf_id ascending with the slot."""
    T = dict(K=K, C=C, bad=np.zeros(K, np.uint8), init_kf=np.zeros(K, np.uint8),
             kf_id=(np.arange(K) * 2 + 10).astype(np.uint32), order=np.arange(K, dtype=i32),
             mp=np.full((K, kp_cap), -1, i32), nmp=np.zeros(K, i32), ml=np.full((K, kl_cap), -1, i32),
             nml=np.zeros(K, i32), parent=np.full(K, -1, i32), prev_kf=np.full(K, -1, i32),
             next_kf=np.full(K, -1, i32), imu=np.zeros(K, np.uint8), map_id=np.zeros(K, i32),
             weights=[dict() for _ in range(K)], children=[[] for _ in range(K)], loops=[[] for _ in range(K)])
    for name, n in (("points", n_pts), ("lines", n_lns)):
        T[name] = dict(bad=np.zeros(n, np.uint8), ref_kf=np.zeros(n, i32), corr_by=np.zeros(n, np.uint32),
                       corr_ref=np.full(n, -1, i32), map_id=np.zeros(n, i32))
    return T


def put(T, slot, ids, lines=False):
    tab, n = (T["ml"], T["nml"]) if lines else (T["mp"], T["nmp"])
    tab[slot, :len(ids)] = ids
    n[slot] = len(ids)


def connect(T, a, b, w, both=True):
    """a's weight map gets b at weight w (and b's gets a); False where a row is full."""
    if len(T["weights"][a]) >= T["C"] and b not in T["weights"][a]:
        return False
    if both and len(T["weights"][b]) >= T["C"] and a not in T["weights"][b]:
        return False
    T["weights"][a][b] = w
    if both:
        T["weights"][b][a] = w
    return True


def slot_rank(T):
    """The address order: a slot's first position in order, n_order + slot for a slot that order does not name."""
    K, order = T["K"], T["order"]
    r = np.arange(K, dtype=np.int64) + len(order)
    pos = np.flatnonzero((order >= 0) & (order < K))
    slots, first = np.unique(order[pos], return_index=True)
    r[slots] = pos[first]
    return r


def finish(T, rng=None):
    """The table forms of the lists: map rows (shuffled), ordered rows (descending weight, then address; bad
    neighbours left out as UpdateBestCovisibles does), CSR rows in address order."""
    K, C = T["K"], T["C"]
    rank = slot_rank(T)
    T["map_kf"], T["map_w"] = np.full((K, C), -1, i32), np.zeros((K, C), i32)
    T["cand"], T["cand_w"] = np.full((K, C), -1, i32), np.zeros((K, C), i32)
    T["map_n"], T["n_cand"] = np.zeros(K, i32), np.zeros(K, i32)
    for s in range(K):
        items = list(T["weights"][s].items())
        if rng is not None:
            items = [items[i] for i in rng.permutation(len(items))]
        T["map_n"][s] = len(items)
        for e, (k, w) in enumerate(items):
            T["map_kf"][s, e], T["map_w"][s, e] = k, w
        live = sorted((it for it in items if not (0 <= it[0] < K) or not T["bad"][it[0]]),
                      key=lambda it: (-it[1], -(rank[it[0]] if 0 <= it[0] < K else 0)))
        T["n_cand"][s] = len(live)
        for e, (k, w) in enumerate(live):
            T["cand"][s, e], T["cand_w"][s, e] = k, w
    for name in ("children", "loops"):
        off, row = np.zeros(K + 1, i32), []
        for s in range(K):
            row += sorted(T[name][s], key=lambda k: rank[k] if 0 <= k < K else 1 << 40)
            off[s + 1] = len(row)
        key = "child" if name == "children" else "loop"
        T[key + "_off"], T[key] = off, np.array(row, i32).reshape(-1)
    return T


KF_KEYS = ("bad", "init_kf", "mp", "nmp", "ml", "nml", "cand", "n_cand", "kf_id", "prev_kf", "next_kf", "order",
           "map_id", "parent", "child_off", "child", "loop_off", "loop", "imu", "cand_w", "map_kf", "map_w", "map_n")


def eg_of(T, lines=True, drop=(), rows=None):
    """plvi.EssentialGraph over copies of the tables (the stamps are in/out)."""
    kf = {k: T[k].copy() for k in KF_KEYS if k not in drop and (lines or k not in ("ml", "nml"))}
    pool = lambda p: {k: a.copy() for k, a in p.items() if k not in drop}  # noqa: E731
    return plvi.EssentialGraph(kf, pool(T["points"]), pool(T["lines"]) if lines else None, rows=rows)


# ------------------------------------------------------- the restatement (C++)
class RefTables(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("kf_cap", "kp_cap", "kl_cap", "cand_stride", "n_order", "map_stride",
                                            "mp_n", "ml_n")] + \
               [(k, ctypes.c_void_p) for k in ("bad", "init_kf", "mp", "nmp", "ml", "nml", "cand", "n_cand", "kf_id",
                                               "prev_kf", "next_kf", "order", "map_id", "parent", "child_off", "child",
                                               "loop_off", "loop", "imu", "cand_w", "map_kf", "map_w", "map_n",
                                               "mp_bad", "mp_ref", "mp_by", "mp_cref", "mp_map",
                                               "ml_bad", "ml_ref", "ml_by", "ml_cref", "ml_map")]


@functools.lru_cache(None)
def ref_lib():
    so = BUILD / "libessential_graph_ref.so"
    newest = max(SRC.stat().st_mtime, (NATIVE / "covis_ref.cpp").stat().st_mtime)
    if not so.exists() or so.stat().st_mtime < newest:
        so.parent.mkdir(parents=True, exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", str(so), str(SRC)],
                       check=True)
    lib = ctypes.CDLL(str(so))
    for f in (lib.eg_ref_correct, lib.eg_ref_graph, lib.eg_ref_connections, lib.covis_ref_update, lib.covis_ref_get,
              lib.covis_ref_destroy):
        f.restype = None
    lib.covis_ref_create.restype = ctypes.c_void_p
    return lib


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def ref_tables(T, stamps, lines=True, drop=()):
    """(RefTables, keep): stamps = {pool: (corr_by, corr_ref)} arrays the restatement updates in place."""
    t = RefTables(T["K"], T["mp"].shape[1], T["ml"].shape[1], T["C"], len(T["order"]), T["C"], len(T["points"]["bad"]),
                  len(T["lines"]["bad"]) if lines else 0)
    for k in KF_KEYS:
        if k not in drop and (lines or k not in ("ml", "nml")):
            setattr(t, k, _p(T[k]))
    for g, name in (("mp", "points"), ("ml", "lines")):
        if name == "lines" and not lines:
            continue
        p = T[name]
        setattr(t, g + "_bad", _p(p["bad"]))
        if "ref_kf" not in drop:
            setattr(t, g + "_ref", _p(p["ref_kf"]))
        if "map_id" not in drop:
            setattr(t, g + "_map", _p(p["map_id"]))
        if "corr_by" not in drop:
            setattr(t, g + "_by", _p(stamps[name][0]))
            setattr(t, g + "_cref", _p(stamps[name][1]))
    return t


def fresh_stamps(T):
    return {n: (T[n]["corr_by"].copy(), T[n]["corr_ref"].copy()) for n in ("points", "lines")}


def correct_caps(T, lines, win_cap=None, pt_cap=None, ln_cap=None):
    return (T["C"] + 1 if win_cap is None else win_cap, max(len(T["points"]["bad"]), 1) if pt_cap is None else pt_cap,
            max(len(T["lines"]["bad"]) if lines else 0, 1) if ln_cap is None else ln_cap)


def add_stamps(r, stamps, lines, drop):
    if "corr_by" not in drop:
        for name, g in (("points", "pt"), ("lines", "ln")):
            if name == "points" or lines:
                r[g + "_corr_by"], r[g + "_corr_ref"] = stamps[name]


def ref_correct(T, cur, lines=True, drop=(), seconds=None, **caps):
    """The restatement's outputs in the layout plvi.EssentialGraph.correct_* returns, plus "against"."""
    wc, pc, lc = correct_caps(T, lines, **caps)
    r = {k: np.full(c + 1, FILL, i32) for k, c in (("win", wc), ("win_sorted", wc), ("pts", pc), ("pts_kf", pc),
                                                   ("lns", lc), ("lns_kf", lc))}
    r.update({k: np.full(1, FILL, i32) for k in ("n_win", "n_sorted", "n_pts", "n_lns", "err", "against")})
    stamps = fresh_stamps(T)
    t = ref_tables(T, stamps, lines, drop)
    sec = ctypes.c_double()
    ref_lib().eg_ref_correct(ctypes.byref(t), cur, wc, pc, lc, *[_p(r[k]) for k in (
        "win", "n_win", "win_sorted", "n_sorted", "pts", "pts_kf", "n_pts", "lns", "lns_kf", "n_lns", "err",
        "against")], ctypes.byref(sec))
    if seconds is not None:
        seconds.append(sec.value)
    add_stamps(r, stamps, lines, drop)
    return r


def graph_caps(T, vert_cap=None, edge_cap=None):
    return max(T["K"], 1) if vert_cap is None else vert_cap, 4 * max(T["K"], 1) if edge_cap is None else edge_cap


def ref_graph(T, cur, loop, mode, win, lc_kf, n_lc, stamps=None, lines=True, drop=(), refs=True, n_win=None,
              seconds=None, **caps):
    vc, ec = graph_caps(T, **caps)
    r = {k: np.full(c + 1, FILL, i32) for k, c in (("vert", vc), ("vert_flags", vc), ("edge_a", ec), ("edge_b", ec),
                                                   ("edge_kind", ec))}
    r.update(n_vert=np.full(1, FILL, i32), n_edges=np.full(5, FILL, i32), err=np.full(1, FILL, i32),
             suppressed=np.full(1, FILL, i32))
    if refs:
        r["pt_ref"] = np.full(len(T["points"]["bad"]) + 1, FILL, i32)
        if lines:
            r["ln_ref"] = np.full(len(T["lines"]["bad"]) + 1, FILL, i32)
    stamps = stamps or fresh_stamps(T)   # kept alive: the struct holds bare addresses
    t = ref_tables(T, stamps, lines, drop)
    win, n_lc = np.ascontiguousarray(win, i32), np.ascontiguousarray(n_lc, i32)
    lc_kf = np.ascontiguousarray(lc_kf, i32)
    n = len(win) if n_win is None else max(0, min(n_win, len(win)))
    sec = ctypes.c_double()
    ref_lib().eg_ref_graph(ctypes.byref(t), cur, loop, mode, _p(win), n, _p(lc_kf), _p(n_lc), lc_kf.shape[1], vc, ec,
                           *[_p(r.get(k)) for k in ("vert", "vert_flags", "n_vert", "edge_a", "edge_b", "edge_kind",
                                                    "n_edges", "pt_ref", "ln_ref", "err", "suppressed")],
                           ctypes.byref(sec))
    if seconds is not None:
        seconds.append(sec.value)
    return r


# ------------------------------------------------ the numpy formulation (A, C)
def np_correct(T, cur, lines=True, drop=(), **caps):
    wc, pc, lc = correct_caps(T, lines, **caps)
    K = T["K"]
    r = {k: np.full(c + 1, FILL, i32) for k, c in (("win", wc), ("win_sorted", wc), ("pts", pc), ("pts_kf", pc),
                                                   ("lns", lc), ("lns_kf", lc))}
    stamps = fresh_stamps(T)
    if not 0 <= cur < K:
        r.update({k: np.zeros(1, i32) for k in ("n_win", "n_sorted", "n_pts", "n_lns")}, err=np.array([E_QUERY], i32))
        add_stamps(r, stamps, lines, drop)
        return r
    rank = slot_rank(T)
    win = np.append(T["cand"][cur, :np.clip(T["n_cand"][cur], 0, T["C"])], cur).astype(i32)
    u = np.unique(win[(win >= 0) & (win < K)])
    ws = u[np.argsort(rank[u])]
    stamp = T["kf_id"][cur]
    n = {}
    for name, tab, ntab, ids_k, own_k, cap in (("points", "mp", "nmp", "pts", "pts_kf", pc),
                                               ("lines", "ml", "nml", "lns", "lns_kf", lc)):
        n[ids_k] = 0
        width = T[tab].shape[1]
        if (name == "lines" and not lines) or width == 0:
            continue
        pool_n = len(T[name]["bad"])
        ids = T[tab][ws].reshape(-1)
        col = np.tile(np.arange(width), len(ws))
        ok = (col < np.repeat(np.clip(T[ntab][ws], 0, width), width)) & (ids >= 0) & (ids < pool_n)
        safe = np.where(ok, ids, 0)
        ok &= T[name]["bad"][safe] == 0 if pool_n else False
        by = None if "corr_by" in drop else stamps[name][0]
        if by is not None and pool_n:
            ok &= by[safe] != stamp
        e = np.flatnonzero(ok)
        _, first = np.unique(ids[e], return_index=True)   # the smallest traversal position wins
        keep = np.sort(e[first])
        got, owner = ids[keep], ws[keep // width]
        r[ids_k][:min(len(got), cap)] = got[:cap]
        r[own_k][:min(len(got), cap)] = owner[:cap]
        n[ids_k] = len(got)
        if by is not None:
            by[got] = stamp
            stamps[name][1][got] = owner
    r["win"][:min(len(win), wc)] = win[:wc]
    r["win_sorted"][:min(len(ws), wc)] = ws[:wc]
    one = lambda v: np.array([v], i32)  # noqa: E731
    r.update(n_win=one(len(win)), n_sorted=one(len(ws)), n_pts=one(n["pts"]), n_lns=one(n["lns"]),
             err=one((E_WIN if len(win) > wc else 0) | (E_PTS if n["pts"] > pc else 0) | (E_LNS if n["lns"] > lc else 0)))
    add_stamps(r, stamps, lines, drop)
    return r


def np_graph(T, cur, loop, mode, win, lc_kf, n_lc, stamps=None, lines=True, drop=(), refs=True, n_win=None, **caps):
    vc, ec = graph_caps(T, **caps)
    K, C = T["K"], T["C"]
    r = {k: np.full(c + 1, FILL, i32) for k, c in (("vert", vc), ("vert_flags", vc), ("edge_a", ec), ("edge_b", ec),
                                                   ("edge_kind", ec))}
    if refs:
        r["pt_ref"] = np.full(len(T["points"]["bad"]) + 1, FILL, i32)
        if lines:
            r["ln_ref"] = np.full(len(T["lines"]["bad"]) + 1, FILL, i32)
    if not (0 <= cur < K and 0 <= loop < K):
        r.update(n_vert=np.zeros(1, i32), n_edges=np.zeros(5, i32), err=np.array([E_QUERY], i32))
        return r
    get = lambda k, d: d if k in drop else T[k]  # noqa: E731
    map_id, parent, imu = get("map_id", np.zeros(K, i32)), get("parent", np.full(K, -1, i32)), get("imu", np.zeros(K))
    rank, n_order, kf_id, bad = slot_rank(T), len(T["order"]), T["kf_id"].astype(np.int64), T["bad"]
    M = map_id[cur]
    member = np.flatnonzero((rank < n_order) & (map_id == M))
    vp = member[np.argsort(rank[member])]
    win = np.asarray(win, i32)[:len(win) if n_win is None else max(0, min(n_win, len(win)))]
    inr = (win >= 0) & (win < K)
    vert = vp[bad[vp] == 0]
    fixed = (vert == loop) if mode == D4 else (T["init_kf"][vert] != 0)
    flags = fixed.astype(i32) | 2 * np.isin(vert, win[inr]).astype(i32)
    is_vert = np.zeros(K, bool)
    is_vert[vert] = True
    r["vert"][:min(len(vert), vc)] = vert[:vc]
    r["vert_flags"][:min(len(vert), vc)] = flags[:vc]

    def weight(i, js):
        mk, mw = T["map_kf"][i, :np.clip(T["map_n"][i], 0, C)], T["map_w"][i, :np.clip(T["map_n"][i], 0, C)]
        hit = js[:, None] == mk[None, :]
        return np.where(hit.any(1), mw[np.argmax(hit, 1)] if len(mk) else 0, 0)

    ea, eb, ek = [], [], []
    keys = np.unique(win[inr])
    keys = keys[np.argsort(rank[keys])]
    pair = []   # the inserted pairs as min * K + max
    for i in keys:
        p = np.flatnonzero(win == i)[-1]
        row = np.asarray(lc_kf[p][:np.clip(n_lc[p], 0, lc_kf.shape[1])], i32)
        row = row[(row >= 0) & (row < K)]
        ok = ((i == cur) & (row == loop)) | (weight(i, row) >= 100)
        js = row[ok]
        ea += [i] * len(js)
        eb += js.tolist()
        ek += [LOOPCONN] * len(js)
        pair += (np.minimum(i, js).astype(np.int64) * K + np.maximum(i, js)).tolist()
    pair = np.array(pair, np.int64)
    four = mode == D4
    for i in vp:
        par = -1 if four else parent[i]
        prev, nxt = T["prev_kf"][i], T["next_kf"][i]
        lrow = T["loop"][T["loop_off"][i]:T["loop_off"][i + 1]] if "loop" not in drop else np.zeros(0, i32)
        crow = T["child"][T["child_off"][i]:T["child_off"][i + 1]] if "child" not in drop else np.zeros(0, i32)
        lrow_in = lrow[(lrow >= 0) & (lrow < K)]
        out = []
        if 0 <= par < K:
            out.append((par, TREE))
        if four and 0 <= prev < K:
            out.append((prev, INERTIAL))
        out += [(l, LOOP) for l in lrow_in[kf_id[lrow_in] < kf_id[i]]]
        nc = np.clip(T["n_cand"][i], 0, C)
        pre = T["cand"][i, :np.count_nonzero(T["cand_w"][i, :nc] >= 100)]   # descending weights: a prefix
        ok = (pre >= 0) & (pre < K) & (pre != par) & ~np.isin(pre, crow) & ~np.isin(pre, lrow)
        if four:
            ok &= (pre != prev) & (pre != nxt)
        safe = np.where(ok, pre, 0)
        ok &= (bad[safe] == 0) & (kf_id[safe] < kf_id[i])
        ok &= ~np.isin(np.minimum(i, safe).astype(np.int64) * K + np.maximum(i, safe), pair)
        out += [(n, COVIS) for n in pre[ok]]
        if not four and imu[i] and 0 <= prev < K:
            out.append((prev, INERTIAL))
        ea += [i] * len(out)
        eb += [o[0] for o in out]
        ek += [o[1] for o in out]
    ea, eb, ek = np.array(ea, i32), np.array(eb, i32), np.array(ek, i32)
    m = min(len(ea), ec)
    r["edge_a"][:m], r["edge_b"][:m], r["edge_kind"][:m] = ea[:ec], eb[:ec], ek[:ec]
    nov = len(ea) and not (is_vert[ea].all() and is_vert[eb].all())
    r.update(n_vert=np.array([len(vert)], i32), n_edges=np.bincount(ek, minlength=5).astype(i32),
             err=np.array([(E_VERT if len(vert) > vc else 0) | (E_EDGE if len(ea) > ec else 0) | (E_NOV if nov else 0)],
                          i32))
    stamps = stamps or fresh_stamps(T)
    for name, key in (("points", "pt_ref"), ("lines", "ln_ref")):
        if key not in r:
            continue
        p = T[name]
        n = len(p["bad"])
        ref = p["ref_kf"].copy()
        if mode == D7 and "corr_by" not in drop:
            hit = stamps[name][0] == T["kf_id"][cur]
            ref[hit] = stamps[name][1][hit]
        fmap = np.zeros(n, i32) if "map_id" in drop else p["map_id"]
        r[key][:n] = np.where((p["bad"] == 0) & (fmap == M), ref, -1)
    return r


GRAPH_KEYS = ("vert", "vert_flags", "n_vert", "edge_a", "edge_b", "edge_kind", "n_edges", "pt_ref", "ln_ref", "err")
CORRECT_KEYS = ("win", "n_win", "win_sorted", "n_sorted", "pts", "pts_kf", "n_pts", "lns", "lns_kf", "n_lns", "err",
                "pt_corr_by", "pt_corr_ref", "ln_corr_by", "ln_corr_ref")


def assert_same(got, exp, keys, tag):
    for k in keys:
        if k in exp:
            assert k in got, f"{tag}: {k} missing"
            assert np.array_equal(got[k], exp[k]), f"{tag}: {k} differs\n got {got[k][:40]}\n exp {exp[k][:40]}"


def edges(r):
    n = int(r["n_edges"].sum())
    return list(zip(r["edge_a"][:n].tolist(), r["edge_b"][:n].tolist(), r["edge_kind"][:n].tolist()))


# ------------------------------------------------------------ crafted cases, A
def case_a_base():
    """cur = 0 with covisibles 3, 1, 2 in that (weight) order, address order 2 < 0 < 3 < 1."""
    T = make_map(6, kp_cap=4, kl_cap=3, C=4, n_pts=12, n_lns=6)
    T["order"] = np.array([2, 0, 3, 1, 4, 5], i32)
    connect(T, 0, 3, 90)
    connect(T, 0, 1, 80)
    connect(T, 0, 2, 70)
    put(T, 0, [0, 1])
    put(T, 1, [2, 5])
    put(T, 2, [3, 2])      # point 2: member 1 is earlier in the window, member 2 at the lower address
    put(T, 3, [4, -1, OUT, 6])
    T["points"]["bad"][6] = 1
    put(T, 1, [0, 1], lines=True)
    put(T, 2, [1, 2], lines=True)
    return finish(T)


def check_a(T, cur, **kw):
    exp, alt = ref_correct(T, cur, **kw), np_correct(T, cur, **kw)
    assert_same(alt, exp, CORRECT_KEYS, "np vs restatement")
    return exp


def test_a_lower_address_owns_not_earlier_window_position():
    T = case_a_base()
    r = check_a(T, 0)
    assert r["win"][:4].tolist() == [3, 1, 2, 0] and r["win_sorted"][:4].tolist() == [2, 0, 3, 1]
    pts = dict(zip(r["pts"][:r["n_pts"][0]].tolist(), r["pts_kf"][:r["n_pts"][0]].tolist()))
    assert pts[2] == 2 and r["against"][0] >= 1          # member 1 comes first in the window and does not own it
    assert r["pts"][:r["n_pts"][0]].tolist() == [3, 2, 0, 1, 4, 5]
    assert r["pt_corr_by"][2] == T["kf_id"][0] and r["pt_corr_ref"][2] == 2
    assert dict(zip(r["lns"][:3].tolist(), r["lns_kf"][:3].tolist())) == {1: 2, 2: 2, 0: 1}


def test_a_stamped_bad_null_and_out_of_range_entries():
    T = case_a_base()
    T["points"]["corr_by"][4] = T["kf_id"][0]     # already corrected by this keyframe
    T["points"]["corr_ref"][4] = 5
    T["points"]["corr_by"][5] = T["kf_id"][1]     # stamped by another closure: corrected again
    r = check_a(T, 0)
    listed = r["pts"][:r["n_pts"][0]].tolist()
    assert 4 not in listed and 6 not in listed and 5 in listed and -1 not in listed and OUT not in listed
    assert r["pt_corr_ref"][4] == 5 and r["pt_corr_by"][6] == 0


def test_a_bad_member_walked_and_cand_entry_out_of_range():
    T = case_a_base()
    T["bad"][3] = 1
    finish(T)
    T["cand"][0, 0], T["n_cand"][0] = 3, 4      # the bad member is still in the stored row ...
    T["cand"][0, 1:4] = [OUT, 1, 2]             # ... and an entry names no slot
    r = check_a(T, 0)
    assert r["win"][:5].tolist() == [3, OUT, 1, 2, 0] and r["n_sorted"][0] == 4
    assert 4 in r["pts"][:r["n_pts"][0]].tolist()         # point 4 lives in the bad member only


def test_a_empty_row_lines_absent_and_no_stamps():
    T = case_a_base()
    r = check_a(T, 4)                                     # no covisibles: the window is cur alone
    assert r["n_win"][0] == 1 and r["win"][0] == 4 and r["n_pts"][0] == 0
    r = check_a(T, 0, lines=False)
    assert r["n_lns"][0] == 0 and r["lns"][0] == FILL and "ln_corr_by" not in r
    r = check_a(T, 0, drop=("corr_by", "corr_ref"))
    assert r["n_pts"][0] == 6 and "pt_corr_by" not in r
    assert check_a(T, OUT)["err"][0] == E_QUERY and check_a(T, -1)["err"][0] == E_QUERY


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_a_capacities_one_below_at_and_above(d):
    T = case_a_base()
    full = check_a(T, 0)
    for key, n, bit in (("win_cap", 4, E_WIN), ("pt_cap", 6, E_PTS), ("ln_cap", 3, E_LNS)):
        r = check_a(T, 0, **{key: n + d})
        assert r["err"][0] == (bit if d < 0 else 0)
        # the stamps are written beyond the capacity too
        assert np.array_equal(r["pt_corr_by"], full["pt_corr_by"]) and np.array_equal(r["ln_corr_ref"], full["ln_corr_ref"])
        assert r["n_pts"][0] == 6 and r["n_lns"][0] == 3 and r["n_win"][0] == 4


# ------------------------------------------------------------ crafted cases, C
def case_c_base():
    """Nine keyframes, address order = slot order, ids ascending.  cur = 8, loop = 1, window {7, 8}."""
    T = make_map(10, C=8, n_pts=6, n_lns=3)
    T["init_kf"][0] = 1
    T["prev_kf"][1:9] = np.arange(0, 8)
    T["next_kf"][0:8] = np.arange(1, 9)
    T["parent"][1:9] = [0, 1, 2, 2, 4, 5, 6, 7]
    for s in range(1, 9):
        T["children"][T["parent"][s]].append(s)
    T["imu"][[2, 3]] = 1
    T["bad"][9] = 1
    T["order"] = np.arange(9, dtype=i32)
    connect(T, 8, 7, 200)
    connect(T, 8, 1, 0, both=False)    # the cur-loop pair is kept at weight 0
    connect(T, 1, 8, 150, both=False)
    connect(T, 7, 2, 100)              # loop connection at the threshold
    connect(T, 7, 3, 99)               # ... and one below
    connect(T, 6, 3, 100)              # plain covisibility at the threshold
    connect(T, 6, 2, 99)
    connect(T, 5, 3, 120)
    connect(T, 4, 2, 130)              # the parent
    connect(T, 2, 3, 140)              # a child (3's parent is 2): seen from 3, the parent
    connect(T, 6, 0, 110)
    T["loops"][6].append(0)            # ... which is a loop edge
    T["loops"][0].append(6)
    T["loops"][5].append(1)
    T["loops"][1].append(5)
    T["points"]["ref_kf"][:] = [0, 1, 2, 3, 4, 5]
    T["lines"]["ref_kf"][:] = [6, 7, 8]
    return finish(T)


C_WIN = np.array([7, 8], i32)
C_LC = np.array([[2, 3, -1], [1, -1, -1]], i32)
C_NLC = np.array([2, 1], i32)


def check_c(T, cur, loop, mode, win=C_WIN, lc_kf=C_LC, n_lc=C_NLC, **kw):
    exp, alt = ref_graph(T, cur, loop, mode, win, lc_kf, n_lc, **kw), np_graph(T, cur, loop, mode, win, lc_kf, n_lc, **kw)
    assert_same(alt, exp, GRAPH_KEYS, "np vs restatement")
    return exp


def test_c_thresholds_exemption_and_order_7dof():
    T = case_c_base()
    r = check_c(T, 8, 1, D7)
    e = edges(r)
    assert e[:2] == [(7, 2, LOOPCONN), (8, 1, LOOPCONN)]          # 99 is left out; cur-loop kept at weight 0
    assert (7, 3, LOOPCONN) not in e
    assert (6, 3, COVIS) in e and (6, 2, COVIS) not in e          # 100 / 99 on the covisible prefix
    assert (4, 2, COVIS) not in e and (4, 2, TREE) in e           # the neighbour is the parent
    assert (3, 2, COVIS) not in e and (2, 3, COVIS) not in e      # parent from one side, child and larger id from the other
    assert (6, 0, COVIS) not in e and (6, 0, LOOP) in e           # the neighbour is a loop edge
    assert (0, 6, LOOP) not in e                                  # kf_id above
    assert (7, 2, COVIS) not in e and r["suppressed"][0] == 1     # inserted, seen from the window member
    assert (5, 3, COVIS) in e
    at = [x for x in e if x[0] == 6]
    assert at == [(6, 5, TREE), (6, 0, LOOP), (6, 3, COVIS)]      # tree, loop, covisibility
    assert [x for x in e if x[0] == 3] == [(3, 2, TREE), (3, 2, INERTIAL)]
    assert r["n_vert"][0] == 9 and r["vert_flags"][:9].tolist() == [1, 0, 0, 0, 0, 0, 0, 2, 2] and r["err"][0] == 0


def test_c_loop_cur_pair_in_the_other_direction_is_not_exempt():
    T = case_c_base()
    r = check_c(T, 8, 1, D7, win=np.array([1, 8], i32), lc_kf=np.array([[8], [2]], i32), n_lc=np.array([1, 1], i32))
    assert (1, 8, LOOPCONN) in edges(r)                           # weight 150 from 1's side
    T["weights"][1][8] = 99
    finish(T)
    r = check_c(T, 8, 1, D7, win=np.array([1, 8], i32), lc_kf=np.array([[8], [2]], i32), n_lc=np.array([1, 1], i32))
    assert (1, 8, LOOPCONN) not in edges(r) and (8, 2, LOOPCONN) not in edges(r)


def test_c_inserted_through_the_other_endpoint():
    T = case_c_base()
    connect(T, 7, 8, 200)
    # 8's row names 7 at weight 200; 7 > ... the covisibility edge (8, 7) is seen from 8 and inserted as (8, 7)
    r = check_c(T, 8, 1, D7, lc_kf=np.array([[2, 3, -1], [1, 7, -1]], i32), n_lc=np.array([2, 2], i32))
    e = edges(r)
    assert (8, 7, LOOPCONN) in e and (8, 7, COVIS) not in e and (8, 7, TREE) in e
    # ... and through the smaller endpoint's row: (7, 2) is inserted by 7, suppressed when 7 walks its prefix
    assert r["suppressed"][0] == 1
    T2 = case_c_base()
    T2["parent"][8] = -1
    T2["children"][7].remove(8)
    finish(T2)
    r2 = check_c(T2, 8, 1, D7, win=np.array([8, 2], i32), lc_kf=np.array([[1, -1], [7, -1]], i32),
                 n_lc=np.array([1, 1], i32))
    e2 = edges(r2)
    assert (2, 7, LOOPCONN) in e2 and (7, 2, COVIS) not in e2 and r2["suppressed"][0] == 1
    assert (8, 7, COVIS) in e2                                    # no longer the parent, not inserted


def test_c_equal_ids_and_bad_neighbour():
    T = case_c_base()
    T["kf_id"][3] = T["kf_id"][5]                                 # equal: no edge either way
    connect(T, 5, 2, 125)
    finish(T)
    assert (5, 2, COVIS) in edges(check_c(T, 8, 1, D7))
    T["bad"][2] = 1                                               # the stored rows still name it
    r = check_c(T, 8, 1, D7)
    e = edges(r)
    assert (5, 3, COVIS) not in e and (3, 5, COVIS) not in e
    assert not [x for x in e if x[1] == 2 and x[2] == COVIS]
    assert [x for x in e if x[0] == 2]                            # the bad keyframe still emits its edges ...
    assert r["err"][0] == E_NOV and 2 not in r["vert"][:r["n_vert"][0]].tolist()   # ... on a null vertex


def test_c_4dof_parent_prev_next_and_inertial_without_imu():
    T = case_c_base()
    connect(T, 6, 4, 160)
    connect(T, 6, 5, 170)              # prev of 6 and its parent
    connect(T, 7, 6, 180)              # seen from 6: next
    finish(T)
    r = check_c(T, 8, 1, D4)
    e = edges(r)
    assert not [x for x in e if x[2] == TREE]
    assert (4, 2, COVIS) in e                                     # the parent is an ordinary covisible here
    assert (6, 5, COVIS) not in e and (7, 6, COVIS) not in e      # prev / next
    assert (6, 4, COVIS) in e
    assert [x for x in e if x[0] == 6] == [(6, 5, INERTIAL), (6, 0, LOOP), (6, 4, COVIS), (6, 3, COVIS)]
    assert (1, 0, INERTIAL) in e and T["imu"][1] == 0             # no bImu test
    assert r["vert_flags"][:9].tolist() == [0, 1, 0, 0, 0, 0, 0, 2, 2]
    r7 = check_c(T, 8, 1, D7)
    assert (6, 5, COVIS) not in edges(r7) and (6, 4, COVIS) in edges(r7)


def test_c_two_maps_order_twice_and_unnamed():
    T = case_c_base()
    T["map_id"][[4, 5]] = 1
    T["order"] = np.array([3, 0, 1, 2, 3, 4, 5, 6, 7, 8, OUT, 0], i32)   # 3 first; 9 not named
    T["points"]["map_id"][2] = 1
    finish(T)
    r = check_c(T, 8, 1, D7)
    assert r["vert"][:r["n_vert"][0]].tolist() == [3, 0, 1, 2, 6, 7, 8]
    assert r["err"][0] == E_NOV                                   # 6's parent 5 is in the other map
    assert not [x for x in edges(r) if x[0] in (4, 5)]
    assert r["pt_ref"][2] == -1
    r = check_c(T, 5, 4, D7, win=np.array([5], i32), lc_kf=np.zeros((1, 1), i32), n_lc=np.zeros(1, i32))
    assert r["vert"][:r["n_vert"][0]].tolist() == [4, 5] and r["pt_ref"][:6].tolist() == [-1, -1, 2, -1, -1, -1]


def test_c_feature_references_in_all_three_branches():
    T = case_c_base()
    T["points"]["corr_by"][1] = T["kf_id"][8]
    T["points"]["corr_ref"][1] = 7
    T["points"]["corr_by"][2] = T["kf_id"][7]     # another keyframe's stamp
    T["points"]["corr_ref"][2] = 6
    T["points"]["bad"][3] = 1
    T["lines"]["corr_by"][0] = T["kf_id"][8]
    T["lines"]["corr_ref"][0] = 8
    r = check_c(T, 8, 1, D7)
    assert r["pt_ref"][:6].tolist() == [0, 7, 2, -1, 4, 5] and r["ln_ref"][:3].tolist() == [8, 7, 8]
    r = check_c(T, 8, 1, D4)
    assert r["pt_ref"][:6].tolist() == [0, 1, 2, -1, 4, 5] and r["ln_ref"][:3].tolist() == [6, 7, 8]
    r = check_c(T, 8, 1, D7, refs=False)
    assert "pt_ref" not in r
    assert check_c(T, 8, OUT, D7)["err"][0] == E_QUERY and check_c(T, -1, 1, D4)["err"][0] == E_QUERY


def test_c_slot_at_two_positions_reads_the_last_row():
    T = case_c_base()
    r = check_c(T, 8, 1, D7, win=np.array([7, 8, 7], i32), lc_kf=np.array([[3, -1], [1, -1], [2, -1]], i32),
                n_lc=np.array([1, 1, 1], i32))
    assert edges(r)[:2] == [(7, 2, LOOPCONN), (8, 1, LOOPCONN)]
    r = check_c(T, 8, 1, D7, win=np.array([7, 8, 7], i32), lc_kf=np.array([[3, -1], [1, -1], [2, -1]], i32),
                n_lc=np.array([1, 1, 1], i32), n_win=2)
    assert edges(r)[:1] == [(8, 1, LOOPCONN)] and r["n_edges"][0] == 1


@pytest.mark.parametrize("mode", [D7, D4])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_c_capacities_one_below_at_and_above(mode, d):
    T = case_c_base()
    full = check_c(T, 8, 1, mode)
    nv, ne = int(full["n_vert"][0]), int(full["n_edges"].sum())
    r = check_c(T, 8, 1, mode, vert_cap=nv + d)
    assert r["err"][0] == (E_VERT if d < 0 else 0) and r["n_vert"][0] == nv
    r = check_c(T, 8, 1, mode, edge_cap=ne + d)
    assert r["err"][0] == (E_EDGE if d < 0 else 0) and np.array_equal(r["n_edges"], full["n_edges"])
    assert r["edge_a"][ne + d] == FILL


# ------------------------------------------------------------------ random maps
def random_map(seed, K=120, kp_cap=4, kl_cap=3, C=32):
    """A map of K slots with everything the three operations read; returns (T, cur, loop, win, lc_kf, n_lc)."""
    rng = np.random.default_rng(seed)
    n_pts, n_lns = K * max(kp_cap // 2, 1), K * max(kl_cap // 2, 1)
    T = make_map(K, kp_cap, kl_cap, C, n_pts, n_lns)
    T["bad"][:] = rng.random(K) < 0.06
    T["map_id"][:] = rng.random(K) < 0.12
    T["kf_id"][:] = rng.permutation(K) * 3 + 5
    T["init_kf"][rng.integers(0, K)] = 1
    named = rng.permutation(K)[:K - 3]
    T["order"] = np.concatenate([named, [named[0], OUT, -1]]).astype(i32)
    T["imu"][:] = rng.random(K) < 0.5
    T["prev_kf"][1:] = np.where(rng.random(K - 1) < 0.8, np.arange(K - 1), -1)
    T["next_kf"][:-1] = np.where(rng.random(K - 1) < 0.8, np.arange(1, K), -1)
    weights = np.array([20, 60, 99, 100, 101, 150, 300])
    for i in range(K):
        for j in np.unique(np.clip(i + rng.integers(-12, 13, 7), 0, K - 1)):
            if j != i:
                connect(T, i, int(j), int(rng.choice(weights)))
    for i in range(1, K):
        near = [j for j in T["weights"][i] if rng.random() < 0.5]
        if near and rng.random() < 0.85:
            T["parent"][i] = near[0]
            T["children"][near[0]].append(i)
        if rng.random() < 0.1 and T["weights"][i]:
            T["children"][i].append(int(rng.choice(list(T["weights"][i]))))
        if rng.random() < 0.35:
            for l in rng.integers(0, K, rng.integers(1, 4)):
                if l != i and l not in T["loops"][i]:
                    T["loops"][i].append(int(l))
                    T["loops"][int(l)].append(i)
    T["loops"][0].append(OUT)
    cur = int(rng.integers(K // 2, K))
    while T["bad"][cur] or len(T["weights"][cur]) < 4:
        cur = (cur + 1) % K
    T["map_id"][cur] = 0
    loop = int(rng.integers(0, K // 4))
    T["map_id"][loop] = 0
    # features: ids near the slot, so neighbours share them; NULL, out-of-range and bad entries; old stamps
    for name, tab, ntab, cap, n in (("points", "mp", "nmp", kp_cap, n_pts), ("lines", "ml", "nml", kl_cap, n_lns)):
        per = n // K
        for s in range(K):
            m = int(rng.integers(0, cap + 1))
            ids = rng.integers(max(0, (s - 6) * per), min(n, (s + 7) * per), m)
            ids = np.where(rng.random(m) < 0.05, -1, ids)
            ids = np.where(rng.random(m) < 0.03, n + 3, ids)
            T[tab][s, :m] = ids
            T[ntab][s] = m if rng.random() > 0.05 else cap + 2      # a count above the capacity is clamped
            if T[ntab][s] > cap:
                T[tab][s, m:] = rng.integers(0, n, cap - m)
        p = T[name]
        p["bad"][:] = rng.random(n) < 0.08
        p["map_id"][:] = rng.random(n) < 0.1
        p["ref_kf"][:] = rng.integers(0, K, n)
        p["corr_by"][:] = np.where(rng.random(n) < 0.1, T["kf_id"][cur], rng.integers(0, 4 * K, n))
        p["corr_ref"][:] = rng.integers(0, K, n)
    finish(T, rng)
    # the window and its loop connections: far keyframes, some over the threshold from either side
    win = np.append(T["cand"][cur, :T["n_cand"][cur]], cur).astype(i32)
    if seed % 3 == 0:
        win = np.append(win, [win[0], OUT]).astype(i32)              # a slot at two positions, an entry out of range
    lc_cap = 6
    rank = slot_rank(T)
    rows = []
    for p, s in enumerate(win):
        far = [int(j) for j in rng.integers(0, K, 5) if 0 <= s < K and j not in win]
        for j in far:
            connect(T, int(s), j, int(rng.choice(weights)), both=rng.random() < 0.7)
        rows.append(sorted(set(far), key=lambda j: rank[j]))
    if cur != loop and loop not in win:
        rows[len(win) - 1 if seed % 3 else len(win) - 3] = sorted(set(rows[-1][:3] + [loop]), key=lambda j: rank[j])
    finish(T, rng)
    lc_kf = np.full((len(win), lc_cap), -1, i32)
    n_lc = np.zeros(len(win), i32)
    for p, row in enumerate(rows):
        lc_kf[p, :len(row)] = row
        n_lc[p] = len(row)
    return T, cur, loop, win, lc_kf, n_lc


RANDOM_SEEDS = tuple(range(12))


@functools.lru_cache(None)
def random_case(seed, kp_cap=4):
    return random_map(seed, K=90 + 17 * seed, kp_cap=kp_cap)


def test_random_maps_agree_and_cover_every_branch():
    against = suppressed = 0
    kinds = {D7: np.zeros(5, np.int64), D4: np.zeros(5, np.int64)}
    errs = 0
    for seed in RANDOM_SEEDS:
        T, cur, loop, win, lc_kf, n_lc = random_case(seed)
        a = check_a(T, cur)
        # A's window is the stored row: the one C is given here may differ (it was taken before the loop connections)
        against += int(a["against"][0])
        errs |= int(check_a(T, cur, win_cap=2, pt_cap=3, ln_cap=1)["err"][0])
        for mode in (D7, D4):
            stamps = {"points": (a["pt_corr_by"].copy(), a["pt_corr_ref"].copy()),
                      "lines": (a["ln_corr_by"].copy(), a["ln_corr_ref"].copy())}
            r = check_c(T, cur, loop, mode, win, lc_kf, n_lc, stamps=stamps)
            kinds[mode] += r["n_edges"]
            suppressed += int(r["suppressed"][0])
            errs |= int(r["err"][0])
            errs |= int(check_c(T, cur, loop, mode, win, lc_kf, n_lc, vert_cap=5, edge_cap=7)["err"][0])
        errs |= int(check_c(T, OUT, loop, D7, win, lc_kf, n_lc)["err"][0])
    assert against >= 20 and suppressed >= 20, (against, suppressed)
    assert (kinds[D7] >= 20).all() and (kinds[D4][[LOOPCONN, LOOP, COVIS, INERTIAL]] >= 20).all(), kinds
    assert kinds[D4][TREE] == 0
    assert errs == E_WIN | E_PTS | E_LNS | E_QUERY | E_VERT | E_EDGE | E_NOV, errs


# --------------------------------------------------------------- B: LoopConnections
def covis_world(seed, K=24, kp_cap=64):
    """Keyframe tables and observation lists for plvi.Covisibility / covis_ref: keyframes share points in groups, so
    weights straddle the threshold of 15."""
    rng = np.random.default_rng(seed)
    n = K * kp_cap // 3
    tab = np.full((K, kp_cap), -1, i32)
    for s in range(K):
        m = int(rng.integers(kp_cap // 2, kp_cap + 1))
        lo = int(rng.integers(0, max(1, n - 3 * kp_cap)))
        tab[s, :m] = rng.choice(np.arange(lo, min(n, lo + 3 * kp_cap)), m, replace=False)
    return covis_tables(tab, n, rng)


def covis_tables(tab, n, rng=None, bad=None, order=None):
    K = len(tab)
    obs = [[] for _ in range(n)]
    for s in range(K):
        for i in tab[s]:
            if i >= 0:
                obs[i].append(s)
    off = np.zeros(n + 1, i32)
    off[1:] = np.cumsum([len(o) for o in obs])
    kf = dict(bad=np.zeros(K, np.uint8) if bad is None else np.asarray(bad, np.uint8),
              order=(np.arange(K) if order is None else np.asarray(order)).astype(i32), mp=tab,
              nmp=(tab >= 0).sum(1).astype(i32), first_conn=np.ones(K, np.uint8), parent=np.full(K, -1, i32))
    for s in range(K):   # the live entries first
        live = tab[s][tab[s] >= 0]
        tab[s] = -1
        tab[s, :len(live)] = live
    pts = dict(bad=np.zeros(n, np.uint8), obs_off=off, obs_kf=np.array([s for o in obs for s in o], i32).reshape(-1))
    return kf, pts


def ref_connections(kf, pts, pre, win, lc_cap, K, seconds=None):
    """eg_ref_connections on a fresh covis_ref graph brought to the state the earlier updates `pre` leave (a list of
    (slots, the bad flags at that time or None));
    returns the outputs in the layout of plvi.EssentialGraph.connections_*, plus one_shot / n_one_shot and the
    graph handle (the caller destroys it)."""
    lib = ref_lib()
    h = ctypes.c_void_p(lib.covis_ref_create(K))
    args = lambda k, p: [_p(k["bad"]), _p(k["order"]), len(k["order"]), _p(k["mp"]), _p(k["nmp"]), k["mp"].shape[1],  # noqa: E731
                         None, None, 0, None, None, _p(k["first_conn"]), _p(k["parent"]), len(p["bad"]), _p(p["bad"]),
                         _p(p["obs_off"]), _p(p["obs_kf"]), 0, None, None, None]
    k2 = dict(kf, first_conn=kf["first_conn"].copy(), parent=kf["parent"].copy())
    for batch, bad in pre:
        q = np.ascontiguousarray(batch, i32)
        o = [np.zeros(len(q), i32) for _ in range(5)]
        lib.covis_ref_update(h, *args(k2 if bad is None else dict(k2, bad=bad), pts), len(q), _p(q),
                             *[_p(a) for a in o], None)
    win = np.ascontiguousarray(win, i32)
    n = len(win)
    r = {k: np.full(n + 1, FILL, i32) for k in ("n_counted", "n_conn", "kf_max", "w_max", "new_parent", "n_lc",
                                                "n_one_shot")}
    r["lc_kf"] = np.full((n + 1, max(lc_cap, 1)), FILL, i32)
    r["one_shot"] = np.full((n + 1, max(lc_cap, 1)), FILL, i32)
    r["lc_err"] = np.full(1, FILL, i32)
    sec = ctypes.c_double()
    lib.eg_ref_connections(h, *args(k2, pts), n, _p(win), *[_p(r[k]) for k in ("n_counted", "n_conn", "kf_max", "w_max",
                                                                                 "new_parent")], lc_cap, _p(r["lc_kf"]),
                           _p(r["n_lc"]), _p(r["lc_err"]), _p(r["one_shot"]), _p(r["n_one_shot"]), ctypes.byref(sec))
    if seconds is not None:
        seconds.append(sec.value)
    r.update(first_conn=k2["first_conn"], parent=k2["parent"], h=h)
    return r


def ref_graph_rows(h, K, s):
    t = [np.zeros(K, i32) for _ in range(4)]
    n = [ctypes.c_int(), ctypes.c_int()]
    ref_lib().covis_ref_get(h, s, _p(t[0]), _p(t[1]), ctypes.byref(n[0]), _p(t[2]), _p(t[3]), ctypes.byref(n[1]))
    return t[0][:n[0].value], t[1][:n[0].value], t[2][:n[1].value], t[3][:n[1].value]


def np_connections(kf, pts, pre, win, lc_cap, K):
    """lc rows from single-query updates of the covis restatement: the snapshot of each position, then the keys of
    the maps as they stand after the LAST update (the argument the device form rests on)."""
    lib = ref_lib()
    h = ctypes.c_void_p(lib.covis_ref_create(K))
    k2 = dict(kf, first_conn=kf["first_conn"].copy(), parent=kf["parent"].copy())

    def update(q, bad=None):
        q = np.ascontiguousarray(q, i32)
        o = [np.zeros(len(q), i32) for _ in range(5)]
        lib.covis_ref_update(h, _p(k2["bad"] if bad is None else bad), _p(k2["order"]), len(k2["order"]), _p(k2["mp"]), _p(k2["nmp"]),
                             k2["mp"].shape[1], None, None, 0, None, None, _p(k2["first_conn"]), _p(k2["parent"]),
                             len(pts["bad"]), _p(pts["bad"]), _p(pts["obs_off"]), _p(pts["obs_kf"]), 0, None, None,
                             None, len(q), _p(q), *[_p(a) for a in o], None)
    for batch, bad in pre:
        update(batch, bad)
    win = np.asarray(win, i32)
    snaps = []
    for s in win:
        ok = 0 <= s < K
        snaps.append(ref_graph_rows(h, K, int(s))[2].copy() if ok else None)
        if ok:
            update([int(s)])
    order = np.asarray(kf["order"])
    rank = slot_rank(dict(K=K, order=order))
    lc = np.full((len(win) + 1, max(lc_cap, 1)), FILL, i32)
    n_lc = np.full(len(win) + 1, FILL, i32)
    for p, s in enumerate(win):
        n_lc[p] = 0
        if snaps[p] is None:
            continue
        keys = ref_graph_rows(h, K, int(s))[0]
        keys = keys[~np.isin(keys, snaps[p]) & ~np.isin(keys, win)]
        keys = keys[np.argsort(rank[keys])]
        lc[p, :min(len(keys), lc_cap)] = keys[:lc_cap]
        n_lc[p] = len(keys)
    lib.covis_ref_destroy(h)
    return lc, n_lc


def check_b(kf, pts, pre, win, lc_cap):
    K = len(kf["bad"])
    r = ref_connections(kf, pts, pre, win, lc_cap, K)
    lc, n_lc = np_connections(kf, pts, pre, win, lc_cap, K)
    assert np.array_equal(r["lc_kf"], lc) and np.array_equal(r["n_lc"], n_lc), (r["lc_kf"], lc, r["n_lc"], n_lc)
    ref_lib().covis_ref_destroy(r.pop("h"))
    return r


def case_b_resort():
    """Members 0 and 1, outsiders 2 and 3.  Keyframe 1 shares 20 points with 0, 5 with 2 and 20 with 3.  It was
    updated while 0 was still bad: its map is {2: 5, 3: 20} and its ordered row [3] -- 2 is below the threshold, a
    key that is not listed.  Returns (tables, pre): pre is that earlier update."""
    K, cap = 4, 64
    tab = np.full((K, cap), -1, i32)
    tab[1, :45] = list(range(0, 45))
    tab[0, :20] = list(range(0, 20))
    tab[2, :5] = list(range(20, 25))
    tab[3, :20] = list(range(25, 45))
    return covis_tables(tab, 50), [([1], np.array([1, 0, 0, 0], np.uint8))]


def test_b_previous_neighbour_resorted_in_by_an_earlier_member():
    """Window [0, 1].  0's update adds 0 to 1's map, and the UpdateBestCovisibles that follows rebuilds 1's row from
    the WHOLE map: [0, 3, 2].  The snapshot of position 1 therefore names 2 and 1's row of LoopConnections is empty; a
    snapshot of every member taken before the first update holds [3] and keeps 2."""
    (kf, pts), pre = case_b_resort()
    r = check_b(kf, pts, pre, [0, 1], 4)
    assert r["n_lc"][:2].tolist() == [0, 0] and r["n_counted"][:2].tolist() == [1, 3]
    assert r["n_one_shot"][1] == 1 and r["one_shot"][1, 0] == 2      # a one-shot snapshot gives a different row
    # a slot at two positions gets two rows
    r = check_b(kf, pts, [], [1, 0, 1], 4)
    assert r["n_lc"][:3].tolist() == [2, 0, 1] and r["lc_kf"][0, :2].tolist() == [2, 3] and r["lc_kf"][2, 0] == 2


def test_b_below_threshold_key_survives_and_late_member():
    """0 shares 5 points with outsider 3 (below 15: a map key, not a listed connection) and 20 with 2."""
    K, cap = 5, 64
    tab = np.full((K, cap), -1, i32)
    tab[0, :45] = list(range(0, 45))
    tab[1, :20] = list(range(25, 45))       # member 1 shares 20 with member 0
    tab[2, :20] = list(range(0, 20))
    tab[3, :5] = list(range(20, 25))
    kf, pts = covis_tables(tab, 50)
    r = check_b(kf, pts, [], [0, 1], 4)
    assert r["lc_kf"][0, :2].tolist() == [2, 3] and r["n_lc"][0] == 2   # 3 at weight 5 stays in LoopConnections
    assert r["n_lc"][1] == 0                  # 1 sees only 0; 1 was added to 0's map after 0's keys were taken
    assert r["n_conn"][0] == 2 and r["n_counted"][0] == 3


def test_b_empty_counter_out_of_range_and_capacity():
    K, cap = 4, 64
    tab = np.full((K, cap), -1, i32)
    tab[0, :40] = list(range(0, 40))
    tab[1, :20] = list(range(0, 20))
    tab[2, :20] = list(range(20, 40))
    kf, pts = covis_tables(tab, 45)
    r = check_b(kf, pts, [], [3, OUT, 0], 1)
    assert r["n_counted"][0] == 0 and r["n_lc"][:3].tolist() == [0, 0, 2]     # 3 observes nothing: :534 returns
    assert r["n_counted"][1] == FILL and r["lc_err"][0] == E_LC and r["lc_kf"][2, 0] == 1
    assert check_b(kf, pts, [], [3, OUT, 0], 2)["lc_err"][0] == 0


def test_b_random_worlds():
    n_rows = 0
    for seed in range(6):
        kf, pts = covis_world(seed)
        K = len(kf["bad"])
        rng = np.random.default_rng(100 + seed)
        kf["order"] = rng.permutation(K).astype(i32)
        pre = [(rng.permutation(K)[:K // 2], None)]
        win = rng.permutation(K)[:7]
        r = check_b(kf, pts, pre, win, 8)
        n_rows += int((r["n_lc"][:7] > 0).sum())
    assert n_rows >= 10


# ------------------------------------------------------------------------- gpu
def run_forms_a(T, cur, lines=True, drop=(), **caps):
    exp = ref_correct(T, cur, lines, drop, **caps)
    got = eg_of(T, lines, drop).correct_device(cur, fill=FILL, **caps)
    assert got["rc"] == 0
    assert_same(got, exp, CORRECT_KEYS, "device form")
    got = eg_of(T, lines, drop).correct_host(cur, fill=FILL, **caps)
    assert got["rc"] == (plvi.PLVI_E_CAPACITY if exp["err"][0] else 0)
    assert_same(got, exp, CORRECT_KEYS, "host form")
    return exp


def run_forms_c(T, cur, loop, mode, win, lc_kf, n_lc, lines=True, drop=(), refs=True, n_win=None, **caps):
    exp = ref_graph(T, cur, loop, mode, win, lc_kf, n_lc, None, lines, drop, refs, n_win, **caps)
    got = eg_of(T, lines, drop).graph_device(cur, loop, mode, win, n_win, lc_kf, n_lc, refs=refs, fill=FILL, **caps)
    assert got["rc"] == 0
    assert_same(got, exp, GRAPH_KEYS, "device form")
    got = eg_of(T, lines, drop).graph_host(cur, loop, mode, win, n_win, lc_kf, n_lc, refs=refs, fill=FILL, **caps)
    assert got["rc"] == (plvi.PLVI_E_CAPACITY if exp["err"][0] & ~E_NOV else 0)
    assert_same(got, exp, GRAPH_KEYS, "host form")
    return exp


@pytest.mark.gpu
def test_gpu_crafted_cases_both_forms():
    T = case_a_base()
    run_forms_a(T, 0)
    run_forms_a(T, 4)
    run_forms_a(T, OUT)
    run_forms_a(T, 0, lines=False)
    run_forms_a(T, 0, drop=("corr_by", "corr_ref"))
    for d in (-1, 0, 1):
        run_forms_a(T, 0, win_cap=4 + d, pt_cap=6 + d, ln_cap=3 + d)
    T = case_c_base()
    T["points"]["corr_by"][1] = T["kf_id"][8]
    T["points"]["corr_ref"][1] = 7
    for mode in (D7, D4):
        full = run_forms_c(T, 8, 1, mode, C_WIN, C_LC, C_NLC)
        nv, ne = int(full["n_vert"][0]), int(full["n_edges"].sum())
        for d in (-1, 0, 1):
            run_forms_c(T, 8, 1, mode, C_WIN, C_LC, C_NLC, vert_cap=nv + d, edge_cap=ne + d)
        run_forms_c(T, 8, OUT, mode, C_WIN, C_LC, C_NLC)
        run_forms_c(T, 8, 1, mode, np.array([7, 8, 7], i32), np.array([[3, -1], [1, -1], [2, -1]], i32),
                    np.array([1, 1, 1], i32))
    # NULL optionals: one map, no parents, no children, no loop edges, no imu, no init_kf, no stamps, no refs
    drop = ("map_id", "parent", "child_off", "child", "loop_off", "loop", "imu", "init_kf", "corr_by", "corr_ref")
    run_forms_c(T, 8, 1, D7, C_WIN, C_LC, C_NLC, drop=drop)
    run_forms_c(T, 8, 1, D4, C_WIN, C_LC, C_NLC, lines=False, drop=drop, refs=False)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,kp_cap", [(0, 4), (3, 4), (7, 64), (11, 4), (12, 64)])
def test_gpu_random_maps_both_forms(seed, kp_cap):
    T, cur, loop, win, lc_kf, n_lc = random_case(seed, kp_cap)
    assert T["K"] <= 300 and T["C"] == 32
    run_forms_a(T, cur)
    run_forms_a(T, cur, win_cap=2, pt_cap=3, ln_cap=1)
    for mode in (D7, D4):
        run_forms_c(T, cur, loop, mode, win, lc_kf, n_lc)
        run_forms_c(T, cur, loop, mode, win, lc_kf, n_lc, vert_cap=5, edge_cap=7)


@pytest.mark.gpu
def test_gpu_one_past_a_scan_tile_and_a_large_table():
    """order one entry longer than the 1024 of a scan tile, only the last keyframe emitting an edge; kf_cap well
    above the window bound kept in LDS (PLVI_EG_MAX_WIN = 2049)."""
    K = 2600
    T = make_map(K, kp_cap=1, kl_cap=1, C=2, n_pts=4, n_lns=1)
    T["order"] = np.arange(1025, dtype=i32)
    T["parent"][1024] = 3
    T["kf_id"][:] = np.arange(K)[::-1] + 7
    connect(T, 2500, 2400, 300)
    put(T, 2500, [1])
    put(T, 2400, [2])
    finish(T)
    for mode, n in ((D7, 1), (D4, 0)):
        r = run_forms_c(T, 1024, 0, mode, np.array([1024], i32), np.zeros((1, 1), i32), np.zeros(1, i32), vert_cap=K,
                        edge_cap=8)
        assert r["n_vert"][0] == 1025 and int(r["n_edges"].sum()) == n
    assert edges(run_forms_c(T, 1024, 0, D7, np.array([1024], i32), np.zeros((1, 1), i32), np.zeros(1, i32),
                             vert_cap=K)) == [(1024, 3, TREE)]
    r = run_forms_a(T, 2500)           # slots the order does not name sort by slot
    assert r["win_sorted"][:2].tolist() == [2400, 2500] and r["pts"][:2].tolist() == [2, 1]


@pytest.mark.gpu
def test_gpu_graph_capture_of_a_and_c_replayed_once():
    T, cur, loop, win, lc_kf, n_lc = random_case(3)
    lib = plvi.load()
    exp_a = ref_correct(T, cur)
    stamps = {"points": (exp_a["pt_corr_by"].copy(), exp_a["pt_corr_ref"].copy()),
              "lines": (exp_a["ln_corr_by"].copy(), exp_a["ln_corr_ref"].copy())}
    exp_c = ref_graph(T, cur, loop, D7, win, lc_kf, n_lc, stamps)
    g = eg_of(T)
    step_a, fetch_a = g.correct_device(cur, fill=FILL, run=False)
    step_c, fetch_c = g.graph_device(cur, loop, D7, win, None, lc_kf, n_lc, fill=FILL, run=False)
    stream, graph = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.plvi_stream_create(ctypes.byref(stream)) == 0
    try:
        assert lib.plvi_graph_capture_begin(stream) == 0
        rcs = (step_a(stream.value), step_c(stream.value))
        assert lib.plvi_graph_capture_end(stream, ctypes.byref(graph)) == 0
        assert rcs == (0, 0)
        assert lib.plvi_graph_launch(graph, stream) == 0
        assert lib.plvi_stream_synchronize(stream) == 0
        assert_same(fetch_a(), exp_a, CORRECT_KEYS, "captured A")
        assert_same(fetch_c(), exp_c, GRAPH_KEYS, "captured C")    # C reads the stamps A wrote in the same replay
    finally:
        if graph:
            lib.plvi_graph_destroy(graph)
        lib.plvi_stream_destroy(stream)


def covis_of(kf, pts, conn_cap=32):
    cov = plvi.Covisibility(len(kf["bad"]), conn_cap)
    return cov.set_tables({k: a.copy() for k, a in kf.items()}, pts)


@pytest.mark.gpu
def test_gpu_loop_connections_both_forms():
    cases = [(*case_b_resort(), [0, 1], 4), (case_b_resort()[0], [], [1, 0, 1], 4)]
    K, cap = 4, 64
    tab = np.full((K, cap), -1, i32)
    tab[0, :40], tab[1, :20], tab[2, :20] = list(range(40)), list(range(20)), list(range(20, 40))
    cases.append((covis_tables(tab, 45), [], [3, OUT, 0], 1))
    for seed in range(3):
        kf, pts = covis_world(seed)
        rng = np.random.default_rng(100 + seed)
        kf["order"] = rng.permutation(len(kf["bad"])).astype(i32)
        cases.append(((kf, pts), [(rng.permutation(len(kf["bad"]))[:12], None)], rng.permutation(len(kf["bad"]))[:7], 8))
    keys = ("n_counted", "n_conn", "kf_max", "w_max", "new_parent", "lc_kf", "n_lc", "lc_err")
    for (kf, pts), pre, win, lc_cap in cases:
        K = len(kf["bad"])
        exp = ref_connections(kf, pts, pre, win, lc_cap, K)
        ref_lib().covis_ref_destroy(exp.pop("h"))
        for form in ("device", "host"):
            cov = covis_of(kf, pts)
            for batch, bad in pre:
                if bad is not None:
                    cov.put("kf", "bad", bad)
                assert cov.update_batch(batch)["rc"] == 0
                cov.put("kf", "bad", kf["bad"])
            if form == "device":
                got = plvi.EssentialGraph.connections_device(cov, win, lc_cap, fill=FILL)
                assert got["rc"] == 0
                got.update(first_conn=cov.table("first_conn"), parent=cov.table("parent"))
            else:
                cov.kf["parent"][:] = cov.table("parent")
                cov.kf["first_conn"][:] = cov.table("first_conn")
                got = plvi.EssentialGraph.connections_host(cov, win, lc_cap, fill=FILL)
                assert got["rc"] == (plvi.PLVI_E_CAPACITY if exp["lc_err"][0] else 0)
                got.update(first_conn=cov.kf["first_conn"], parent=cov.kf["parent"])
            assert_same(got, exp, keys + ("first_conn", "parent"), form)
            cov.close()


@pytest.mark.gpu
def test_gpu_chain_covisibility_to_a_b_c_on_the_device():
    """plvi.Covisibility graph -> A -> B -> C with the graph's rows read in place and A's / B's outputs passed as
    device addresses, against the restatements run on downloaded tables."""
    rng = np.random.default_rng(5)
    K, cap, n = 12, 64, 400
    tab = np.full((K, cap), -1, i32)
    for s in range(K):   # neighbours share about 40 points: the weights straddle 15; 100 is not reached
        tab[s, :56] = rng.choice(np.arange(max(0, 30 * s - 40), min(n, 30 * s + 60)), 56, replace=False)
    kf, pts = covis_tables(tab, n, order=rng.permutation(K))
    kf["first_conn"][:] = 1
    C = 32
    cov = covis_of(kf, pts, C)
    assert cov.update_batch(np.arange(0, K - 1))["rc"] == 0       # the last keyframe's links are the new ones
    rows, maps = cov.rows(), cov.map_rows()

    ref_kf, parent = rng.integers(0, K, n), cov.table("parent")

    def table_rows():
        T = make_map(K, kp_cap=cap, kl_cap=1, C=C, n_pts=n, n_lns=1)
        T.update(order=kf["order"].copy(), mp=kf["mp"].copy(), nmp=kf["nmp"].copy(), parent=parent.copy())
        T["points"]["ref_kf"][:] = ref_kf
        finish(T)
        for s in range(K):
            d = cov.download(s)
            order = np.argsort(-d["map_kf"][:d["n_map"]])          # the restatement takes map rows in any order
            T["map_n"][s], T["n_cand"][s] = d["n_map"], d["n_ord"]
            T["map_kf"][s, :d["n_map"]], T["map_w"][s, :d["n_map"]] = d["map_kf"][:d["n_map"]][order], d["map_w"][:d["n_map"]][order]
            T["cand"][s, :d["n_ord"]], T["cand_w"][s, :d["n_ord"]] = d["ord_kf"][:d["n_ord"]], d["ord_w"][:d["n_ord"]]
        return T
    T = table_rows()
    cur, loop = K - 2, 0
    in_place = dict(cand=rows[0], cand_w=rows[1], n_cand=rows[2], map_kf=maps[0], map_w=maps[1], map_n=maps[2], stride=C)
    g = eg_of(T, lines=False, rows=in_place)
    a = g.correct_device(cur, fill=FILL)
    exp_a = ref_correct(T, cur, lines=False)
    assert_same(a, exp_a, CORRECT_KEYS, "A in place")
    n_win = int(a["n_win"][0])
    assert n_win >= 3
    win = a["win"][:n_win]
    lc_cap = 8
    b = plvi.EssentialGraph.connections_device(cov, win, lc_cap, fill=FILL)
    assert b["rc"] == 0 and b["lc_err"][0] == 0
    # the restatement of B from the same starting graph
    exp_b = ref_connections(kf, pts, [(np.arange(0, K - 1), None)], win, lc_cap, K)
    ref_lib().covis_ref_destroy(exp_b.pop("h"))
    assert_same(b, exp_b, ("lc_kf", "n_lc", "n_counted", "new_parent"), "B in place")
    assert b["n_lc"][:n_win].sum() > 0
    T2 = table_rows()                                               # the graph as B left it
    stamps = {"points": (a["pt_corr_by"].copy(), a["pt_corr_ref"].copy()), "lines": fresh_stamps(T2)["lines"]}
    for mode in (D7, D4):
        c = g.graph_device(cur, loop, mode, a["dev"]["win"], a["dev"]["n_win"], b["dev"]["lc_kf"], b["dev"]["n_lc"],
                           win_cap=C + 1, lc_cap=lc_cap, fill=FILL)
        exp_c = ref_graph(T2, cur, loop, mode, win, b["lc_kf"][:n_win], b["n_lc"][:n_win], stamps, lines=False)
        assert c["rc"] == 0
        assert_same(c, exp_c, GRAPH_KEYS, "C in place")
    cov.close()
