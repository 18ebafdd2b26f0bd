"""plvi_gba_walk[_device] and plvi_gba_correct[_device] -- the spanning-tree walk and the feature correction behind
an accepted global bundle adjustment (the second half of LoopClosing::RunGlobalBundleAdjustment[WithLines]).

Expected values come from tests/native/gba_propagate_ref.cpp (KeyFrame objects at addresses given by `order`,
std::set children, a std::list queue, the feature loops over cv_gemm_pose), built here with -ffp-contract=off.  An
independent model in Python / numpy (a deque over rows sorted by rank; float32 arrays with the double add spelled
out and fma32 for the contracted form) pins it on the CPU, compared through view(np.uint32) / view(np.uint64).  The
GPU tests demand exact equality of every output of both forms over sentinel-filled arrays.

The restatement gives 1046 of the 1396 state-2 points of the 4097-point map different bits in the two compat forms
(asserted below to be at least one)."""
import collections
import ctypes
import functools
import pathlib
import subprocess

import numpy as np
import pytest

import plvi
from test_feature_refresh import fma32

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "gba_propagate_ref.cpp"
BUILD = ROOT / "tests" / "native" / "_build"

POINTS, LINES = plvi.GBA_POINTS, plvi.GBA_LINES
E_ORIGIN, E_CYCLE, E_WALK, E_REF = 1, 2, 4, 8
FMA = 8  # PLVI_COMPAT_GEMM_FMA
FILL, FILL8 = -7, -7 & 0x7f
LOOP, OLD = 41, 17  # nLoopKF, and a stamp of an earlier GBA
i32, u32, u8, f32, f64 = np.int32, np.uint32, np.uint8, np.float32, np.float64


# ---------------------------------------------------------------- the restatement
class WalkArgs(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("kf_cap", "n_order", "n_origins", "walk_cap")] + \
               [("loop_kf", ctypes.c_uint)] + \
               [(k, ctypes.c_void_p) for k in ("bad", "order", "child_off", "child", "origins", "kf_ba_for", "walk",
                                               "walk_parent", "walk_new", "n_walk", "n_new", "err", "visited",
                                               "seconds")]


class CorrectArgs(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("n", "kf_cap", "kind", "fma_form", "map")] + [("loop_kf", ctypes.c_uint)] + \
               [(k, ctypes.c_void_p) for k in ("bad", "map_id", "ref_kf", "feat_ba_for", "kf_ba_for", "has_bef",
                                               "tcw_bef", "twc", "pos_gba", "col", "state", "counts", "err",
                                               "seconds")]


@functools.lru_cache(None)
def ref_lib():
    so = BUILD / "libgba_propagate_ref.so"
    deps = (SRC, ROOT / "include" / "plvi_frontend.h", ROOT / "oracle" / "ref_fma.h")
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        so.parent.mkdir(parents=True, exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-o",
                        str(so), str(SRC)], check=True)
    lib = ctypes.CDLL(str(so))
    for f in (lib.gba_walk_ref_run, lib.gba_correct_ref_run):
        f.argtypes, f.restype = [ctypes.c_void_p], None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data


# ---------------------------------------------------------------- trees
def forest(K, children, bad=(), stamped=(), order=None, descending=False):
    """Keyframe tables of K slots: children = {slot: [child, ...]} stored as given (or in descending slot order)."""
    rows = [list(children.get(s, ())) for s in range(K)]
    if descending:
        rows = [sorted(r, reverse=True) for r in rows]
    off = np.zeros(K + 1, i32)
    off[1:] = np.cumsum([len(r) for r in rows])
    kf = dict(bad=np.zeros(K, u8), kf_ba_for=np.full(K, OLD, u32), child_off=off,
              child=np.array([c for r in rows for c in r], i32),
              order=np.arange(K, dtype=i32) if order is None else np.asarray(order, i32))
    kf["bad"][list(bad)] = 1
    kf["kf_ba_for"][list(stamped)] = LOOP
    return kf


def chain(K):
    return forest(K, {s: [s + 1] for s in range(K - 1)})


def star(n):
    return forest(n + 1, {0: list(range(1, n + 1))})


def random_tree(K, seed, **kw):
    rng = np.random.default_rng(seed)
    ch = collections.defaultdict(list)
    for s in range(1, K):
        ch[int(rng.integers(0, s))].append(s)
    return forest(K, ch, **kw)


def walk_blank(walk_cap, K, visited=True):
    r = dict(walk=np.full(walk_cap + 1, FILL, i32), walk_parent=np.full(walk_cap + 1, FILL, i32),
             walk_new=np.full(walk_cap + 1, FILL8, u8))
    if visited:
        r["visited"] = np.zeros(K, u8)
    return r


def ref_walk(kf, origins, walk_cap=None, visited=True, loop_kf=LOOP, seconds=None):
    K = len(kf["bad"])
    walk_cap = K if walk_cap is None else walk_cap
    origins = np.ascontiguousarray(origins, i32)
    r = walk_blank(walk_cap, K, visited)
    r["kf_ba_for"] = kf["kf_ba_for"].copy()
    n_walk, n_new, err, sec = np.zeros(1, i32), np.zeros(1, i32), np.zeros(1, i32), np.zeros(1, f64)
    a = WalkArgs(K, len(kf["order"]), len(origins), walk_cap, loop_kf, _p(kf["bad"]), _p(kf["order"]),
                 _p(kf["child_off"]), _p(kf["child"]), _p(origins), _p(r["kf_ba_for"]), _p(r["walk"]),
                 _p(r["walk_parent"]), _p(r["walk_new"]), _p(n_walk), _p(n_new), _p(err), _p(r.get("visited")), _p(sec))
    ref_lib().gba_walk_ref_run(ctypes.byref(a))
    r.update(n_walk=int(n_walk[0]), n_new=int(n_new[0]), err=int(err[0]))
    if seconds is not None:
        seconds.append(float(sec[0]))
    return r


def py_walk(kf, origins, walk_cap=None, visited=True, loop_kf=LOOP):
    """The independent model: ranks as a dict, rows sorted by rank, a deque."""
    K = len(kf["bad"])
    walk_cap = K if walk_cap is None else walk_cap
    rank = {}
    for i, s in enumerate(kf["order"].tolist()):
        if 0 <= s < K:
            rank.setdefault(s, i)
    key = lambda s: rank.get(s, len(kf["order"]) + s)  # noqa: E731
    stamp = kf["kf_ba_for"].copy()
    r = walk_blank(walk_cap, K, visited)
    err, out, n_new = 0, [], 0
    q = collections.deque()
    for o in origins:
        if 0 <= o < K:
            q.append((int(o), -1, 0))
        else:
            err |= E_ORIGIN
    queued = len(q)
    while q:
        s = q[0][0]
        row = kf["child"][kf["child_off"][s]:kf["child_off"][s + 1]].tolist()
        for c in sorted({c for c in row if 0 <= c < K}, key=key):
            if kf["bad"][c]:
                continue
            new = int(stamp[c] != loop_kf)
            stamp[c] = loop_kf
            n_new += new
            queued += 1
            if queued > K:
                return dict(err=err | E_CYCLE)
            q.append((c, s, new))
        out.append(q.popleft())
    for i, (s, p, new) in enumerate(out):
        if i < walk_cap:
            r["walk"][i], r["walk_parent"][i], r["walk_new"][i] = s, p, new
        if visited:
            r["visited"][s] = 1
    r.update(kf_ba_for=stamp, n_walk=len(out), n_new=n_new, err=err | (E_WALK if len(out) > walk_cap else 0))
    return r


WALK_KEYS = ("walk", "walk_parent", "walk_new", "visited", "kf_ba_for", "n_walk", "n_new", "err")


def same_walk(got, exp):
    if exp["err"] & E_CYCLE:  # the reference would not return: only the bit is specified
        assert int(np.ravel(got["err"])[0]) & E_CYCLE
        return
    for k in WALK_KEYS:
        if k in exp:
            assert np.array_equal(np.ravel(got[k]), np.ravel(exp[k])), (k, got[k], exp[k])
    assert ("visited" in got) == ("visited" in exp)


# ---------------------------------------------------------------- walk cases
@functools.lru_cache(None)
def walk_cases():
    c = {}
    c["single_origin_no_children"] = (forest(3, {}), [1], {})
    c["chain_3"] = (chain(3), [0], {})
    c["chain_2100"] = (chain(2100), [0], {})
    for n in (63, 64, 65, 1023, 1024, 1025):
        c[f"star_{n}"] = (star(n), [0], {})
    two = {0: list(range(1, 41))}
    two.update({p: list(range(41 + 40 * (p - 1), 41 + 40 * p)) for p in range(1, 41)})
    c["two_levels_40x40"] = (forest(1641, two), [0], {})
    c["two_origins"] = (forest(8, {0: [1, 2], 4: [5, 6], 5: [7]}), [4, 0], {})
    c["origin_twice"] = (forest(8, {0: [1, 2]}), [0, 0], {})
    c["origin_twice_past_the_queue"] = (forest(4, {0: [1, 2]}), [0, 0], {})
    c["bad_origin"] = (forest(5, {2: [0, 4]}, bad=[2]), [2], {})
    c["origin_out_of_range"] = (forest(5, {1: [2]}), [5, 1, -1], {})
    c["bad_child_with_subtree"] = (forest(9, {0: [1, 2], 1: [3, 4], 4: [5], 2: [6]}, bad=[1]), [0], {})
    c["stamped_child_unstamped_grandchild"] = (forest(6, {0: [1], 1: [2, 3]}, stamped=[1, 3]), [0], {})
    rng = np.random.default_rng(3)
    order = rng.permutation(300)
    order = order[order != 123]
    c["descending_rows_permuted_order_300"] = (random_tree(300, 5, order=order, descending=True), [0], {})
    c["child_minus_1_and_kf_cap"] = (forest(300, {0: [7, -1, 3], 3: [300, 9], 9: [11]}), [0], {})
    c["order_names_a_slot_twice_and_junk"] = (forest(6, {0: [1, 2, 3]}, order=[3, 9, -2, 1, 3, 0]), [0], {})
    n_walk = 300
    for d in (-1, 0, 1):
        c[f"walk_cap_{'below at above'.split()[d + 1]}"] = (random_tree(300, 6), [0], dict(walk_cap=n_walk + d))
    c["walk_cap_0"] = (chain(3), [0], dict(walk_cap=0))
    c["visited_null"] = (random_tree(300, 7), [0], dict(visited=None))
    c["no_origins"] = (chain(3), [], {})
    c["two_slot_cycle"] = (forest(5, {0: [1], 1: [0]}), [0], {})
    return c


def test_walk_restatement_equals_the_python_model():
    for name, (kf, origins, kw) in walk_cases().items():
        exp = ref_walk(kf, origins, **kw)
        model = py_walk(kf, origins, **kw)
        if model["err"] & E_CYCLE:
            assert exp["err"] & E_CYCLE, name
            continue
        same_walk(exp, model)
    # what the cases are there to show
    e = lambda n: ref_walk(*walk_cases()[n][:2], **walk_cases()[n][2])  # noqa: E731
    assert e("single_origin_no_children")["n_walk"] == 1 and e("chain_2100")["n_walk"] == 2100
    assert e("star_1025")["n_new"] == 1025 and e("two_levels_40x40")["n_walk"] == 1641
    assert e("two_origins")["walk"][:2].tolist() == [4, 0]
    r = e("origin_twice")
    assert r["err"] == 0 and r["n_walk"] == 6 and r["n_new"] == 2 and r["walk_new"][:6].tolist() == [0, 0, 1, 1, 0, 0]
    assert e("origin_twice_past_the_queue")["err"] & E_CYCLE and e("two_slot_cycle")["err"] & E_CYCLE
    r = e("bad_origin")
    assert r["walk"][:3].tolist() == [2, 0, 4] and r["kf_ba_for"][2] == OLD   # walked, never stamped
    r = e("origin_out_of_range")
    assert r["err"] == E_ORIGIN and r["walk"][:2].tolist() == [1, 2]
    r = e("bad_child_with_subtree")
    assert sorted(r["walk"][:r["n_walk"]].tolist()) == [0, 2, 6] and (r["kf_ba_for"][[1, 3, 4, 5]] == OLD).all()
    r = e("stamped_child_unstamped_grandchild")
    assert r["walk"][:4].tolist() == [0, 1, 2, 3] and r["walk_new"][:4].tolist() == [0, 0, 1, 0]
    r = e("child_minus_1_and_kf_cap")
    assert r["walk"][:r["n_walk"]].tolist() == [0, 3, 7, 9, 11]
    assert e("order_names_a_slot_twice_and_junk")["walk"][:4].tolist() == [0, 3, 1, 2]
    assert e("walk_cap_below")["err"] == E_WALK and e("walk_cap_at")["err"] == 0 and e("walk_cap_above")["err"] == 0
    assert e("walk_cap_below")["walk"][299] == FILL and (e("walk_cap_below")["kf_ba_for"][1:] == LOOP).all()
    r = e("descending_rows_permuted_order_300")
    assert r["n_walk"] == 300 and r["walk"][:300].tolist() != e("walk_cap_at")["walk"][:300].tolist()


# ---------------------------------------------------------------- the correction
def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def pose_tables(K, seed):
    """mTcwBefGBA and GetPoseInverse() after SetPose of K keyframes: poses a few degrees and centimetres apart."""
    rng = np.random.default_rng(seed)
    bef, twc = np.zeros((K, 12), f32), np.zeros((K, 12), f32)
    for s in range(K):
        R, t = rotation(rng), rng.normal(0, 3, 3)
        w = rng.normal(0, 0.03, 3)
        dR = np.eye(3) + np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        R2, t2 = np.linalg.qr(dR @ R)[0], t + rng.normal(0, 0.05, 3)
        R2 = R2 * np.sign(np.diag(R2 @ R.T))  # the factor nearest R
        bef[s] = np.concatenate([R.ravel(), t])
        twc[s] = np.concatenate([R2.T.ravel(), -R2.T @ t2])
    return bef, twc


def feature_map(kind, n, K=7, seed=1):
    """n features over K keyframes with every state present: slot 2 is bad and still corrects, slot 3 has no
    mTcwBefGBA, slot 4 was not part of this GBA."""
    rng = np.random.default_rng(seed + 10 * kind)
    bef, twc = pose_tables(K, seed)
    poses = dict(kf_ba_for=np.full(K, LOOP, u32), has_bef=np.ones(K, u8), tcw_bef=bef, twc=twc)
    poses["has_bef"][3] = 0
    poses["kf_ba_for"][4] = OLD
    w = 6 if kind == LINES else 3
    col = rng.uniform(-9, 9, (n, w))
    gba = col + rng.normal(0, 0.02, (n, w))
    feat = dict(bad=(rng.random(n) < 0.1).astype(u8), ref_kf=rng.integers(0, K, n).astype(i32),
                map_id=np.where(rng.random(n) < 0.1, 5, 2).astype(i32),
                ba_for=np.where(rng.random(n) < 0.4, LOOP, OLD).astype(u32))
    if kind == LINES:
        feat.update(sep=col.astype(f64), pos_gba=gba.astype(f64))
    else:
        feat.update(pos=col.astype(f32), pos_gba=gba.astype(f32))
    kf_bad = np.zeros(K, u8)
    kf_bad[2] = 1
    return dict(kf_bad=kf_bad, poses=poses, feat=feat, kind=kind, map=2)


def crafted_features(kind):
    """n = 65: one feature per case in front of a random tail."""
    m = feature_map(kind, 65, seed=3)
    f, col = m["feat"], "sep" if kind == LINES else "pos"
    f["bad"][:12], f["map_id"][:12], f["ba_for"][:12] = 0, 2, OLD
    f["ref_kf"][:12] = 0
    f["ba_for"][0] = LOOP                         # state 1
    f["ref_kf"][1] = 1                            # state 2
    f["ref_kf"][2] = 7                            # ref_kf == kf_cap
    f["ref_kf"][3] = -1                           # no reference keyframe
    f["ref_kf"][4] = 3                            # has_bef 0
    f["ref_kf"][5] = 2                            # a bad reference keyframe still corrects
    f["map_id"][6] = 5                            # another map
    f["bad"][7] = 1
    f["ref_kf"][8] = 4                            # its keyframe was not in this GBA
    f["ba_for"][9] = LOOP                         # NaN, with a payload, copied bit for bit
    if kind == LINES:
        f["pos_gba"][9] = np.array([0x7ff4000000000123, 0xfff8000000000000, 0x7ff0000000000001, 1, 2, 3],
                                   np.uint64).view(f64)
        # endpoints no float holds
        f[col][10] = [1 + 2.0 ** -30, -2 - 2.0 ** -40, 1e-50, 3 + 2.0 ** -25, 1234.5678901234567, -0.1]
        f[col][1] = [0.1, 0.2, 0.3, 1 / 3, 2 / 3, 1e-3]
    else:
        f["pos_gba"][9] = np.array([0x7fa00123, 0xffc00000, 0x7f800001], u32).view(f32)
    f["ba_for"][11], f["bad"][11] = LOOP, 1       # bad wins over the stamp
    expect = {0: 1, 1: 2, 2: 0, 3: 0, 4: 0, 5: 2, 6: 0, 7: 0, 8: 0, 9: 1, 10: 2, 11: 0}
    return m, expect


def col_of(m):
    return "sep" if m["kind"] == LINES else "pos"


def ref_correct(m, compat=0, column=None, seconds=None):
    f, p, col = m["feat"], m["poses"], col_of(m)
    n, K = len(f["bad"]), len(p["has_bef"])
    out = (f[col] if column is None else column).copy()
    state, counts, err, sec = np.full(n + 1, FILL8, u8), np.zeros(3, i32), np.zeros(1, i32), np.zeros(1, f64)
    a = CorrectArgs(n, K, m["kind"], int(bool(compat & FMA)), m["map"], LOOP, _p(f["bad"]), _p(f.get("map_id")),
                    _p(f["ref_kf"]), _p(f["ba_for"]), _p(p["kf_ba_for"]), _p(p["has_bef"]), _p(p["tcw_bef"]),
                    _p(p["twc"]), _p(f["pos_gba"]), _p(out), _p(state), _p(counts), _p(err), _p(sec))
    if column is not None:  # a separate output: the input rows are read from the pool, the others stay
        src = f[col].copy()
        a.col = _p(src)
        ref_lib().gba_correct_ref_run(ctypes.byref(a))
        wrote = state[:n] != 0
        out[wrote] = src[wrote]
    else:
        ref_lib().gba_correct_ref_run(ctypes.byref(a))
    if seconds is not None:
        seconds.append(float(sec[0]))
    return {col: out, "state": state, "counts": counts, "err": int(err[0])}


def np_pose(T, X, fma):
    """R * X + t of a pose [12] on X [3] float32: the products and sums in float32, the add of t in float64."""
    out = np.zeros(3, f32)
    for r in range(3):
        a = T[3 * r:3 * r + 3]
        if fma:
            s = fma32(a[2], X[2], fma32(a[0], X[0], f32(a[1] * X[1])))
        else:
            s = f32(f32(f32(a[0] * X[0]) + f32(a[1] * X[1])) + f32(a[2] * X[2]))
        out[r] = f32(f64(s) + f64(T[9 + r]))
    return out


def np_correct(m, compat=0):
    f, p, col = m["feat"], m["poses"], col_of(m)
    n, K = len(f["bad"]), len(p["has_bef"])
    out = f[col].copy()
    state, err = np.full(n + 1, FILL8, u8), 0
    state[:n] = 0
    with np.errstate(all="ignore"):
        for i in range(n):
            if f["bad"][i] or f["map_id"][i] != m["map"]:
                continue
            if f["ba_for"][i] == LOOP:
                out[i] = f["pos_gba"][i]
                state[i] = 1
                continue
            r = int(f["ref_kf"][i])
            if not 0 <= r < K:
                err |= E_REF
                continue
            if p["kf_ba_for"][r] != LOOP or not p["has_bef"][r]:
                continue
            for e in range(2 if m["kind"] == LINES else 1):
                X = out[i, 3 * e:3 * e + 3].astype(f32)
                X = np_pose(p["twc"][r], np_pose(p["tcw_bef"][r], X, compat & FMA), compat & FMA)
                out[i, 3 * e:3 * e + 3] = X
            state[i] = 2
    return {col: out, "state": state, "counts": np.bincount(state[:n], minlength=3).astype(i32), "err": err}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def same_correct(got, exp, col):
    for k in (col, "state", "counts"):
        g, e = bits(got[k]), bits(exp[k])
        assert g.shape == e.shape, (k, g.shape, e.shape)
        bad = np.nonzero((g != e).reshape(len(g), -1).any(axis=1))[0]
        assert not len(bad), (k, bad[:8], got[k][bad[:3]], exp[k][bad[:3]])
    assert int(np.ravel(got["err"])[0]) == exp["err"]


@pytest.mark.parametrize("kind", (POINTS, LINES))
@pytest.mark.parametrize("compat", (0, FMA))
def test_correct_restatement_equals_the_numpy_model(kind, compat):
    m, expect = crafted_features(kind)
    exp = ref_correct(m, compat)
    same_correct(exp, np_correct(m, compat), col_of(m))
    assert {i: int(exp["state"][i]) for i in expect} == expect and exp["err"] == E_REF
    col = col_of(m)
    assert bits(exp[col][9]).tolist() == bits(m["feat"]["pos_gba"][9]).tolist()          # the NaN payloads survive
    assert bits(exp[col][5]).tolist() != bits(m["feat"][col][5]).tolist()                # the bad keyframe corrects
    for i in (2, 3, 4, 6, 7, 8, 11):
        assert bits(exp[col][i]).tolist() == bits(m["feat"][col][i]).tolist()
    if kind == LINES:   # the endpoints went through float: every result is a float widened
        assert (exp[col][10].astype(f32).astype(f64) == exp[col][10])[np.isfinite(exp[col][10])].all()
    for n in (1, 4097):
        big = feature_map(kind, n, seed=8)
        if n == 1:
            big["feat"]["bad"][:], big["feat"]["map_id"][:], big["feat"]["ba_for"][:] = 0, 2, OLD
            big["feat"]["ref_kf"][:] = 0
        same_correct(ref_correct(big, compat), np_correct(big, compat), col_of(big))


def test_the_compat_forms_differ_on_state_2_features():
    big = feature_map(POINTS, 4097, seed=8)
    a, b = ref_correct(big, 0), ref_correct(big, FMA)
    assert np.array_equal(a["state"], b["state"]) and set(a["state"][:4097].tolist()) == {0, 1, 2}
    differ = (bits(a["pos"]) != bits(b["pos"])).any(axis=1)
    assert differ.sum() >= 1 and (a["state"][:4097][differ] == 2).all()
    print("state-2 points that differ between the compat forms:", int(differ.sum()), "of", int((a["state"] == 2).sum()))


# ---------------------------------------------------------------- GPU: the walk
def propagation(kf, m=None):
    pools = [None, None]
    if m is not None:
        pools[m["kind"]] = {k: a.copy() for k, a in m["feat"].items()}
    return plvi.GBAPropagation({k: a.copy() for k, a in kf.items()}, *pools)


def walk_both_forms(kf, origins, exp=None, **kw):
    exp = ref_walk(kf, origins, **kw) if exp is None else exp
    for form in ("batch", "host"):
        g = propagation(kf)
        got = getattr(g.walk, form)(origins, LOOP, fill=FILL, **kw)
        want_rc = plvi.PLVI_E_CAPACITY if exp["err"] else exp["n_walk"]
        assert got["rc"] == (want_rc if form == "host" else 0), (form, got["rc"])
        same_walk(got, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(walk_cases()))
def test_gpu_walk_cases(plvi_lib, name):
    kf, origins, kw = walk_cases()[name]
    walk_both_forms(kf, origins, **kw)


@pytest.mark.gpu
def test_gpu_walk_cycle_stays_inside_its_scratch(plvi_lib):
    kf, origins, _ = walk_cases()["two_slot_cycle"]
    sb = plvi_lib.plvi_gba_walk_scratch_bytes(len(kf["bad"]))
    pad = 4096
    block = plvi.DeviceBuffer(sb + pad)
    block.upload(np.full(sb + pad, 0xA5, u8))
    got = propagation(kf).walk.batch(origins, LOOP, scratch=(block.ptr, sb), fill=FILL)
    assert got["rc"] == 0 and got["err"][0] & E_CYCLE
    assert (block.download(np.zeros(sb + pad, u8))[sb:] == 0xA5).all()
    assert got["walk"][-1] == FILL and got["walk_parent"][-1] == FILL and got["walk_new"][-1] == FILL8


@pytest.mark.gpu
def test_gpu_walk_graph_capture_and_replay(plvi_lib):
    """One call captured into a hipGraph and replayed once: no host read, no allocation, no sync inside."""
    kf, origins, _ = walk_cases()["descending_rows_permuted_order_300"]
    step, fetch = propagation(kf).walk.batch(origins, LOOP, fill=FILL, run=False)
    st = ctypes.c_void_p()
    assert plvi_lib.plvi_stream_create(ctypes.byref(st)) == 0
    rcs = []
    graph = plvi.StepGraph(lambda s: rcs.append(step(s)), st.value)
    assert rcs == [0]
    before = fetch()
    assert (before["walk"] == FILL).all() and (before["kf_ba_for"] == OLD).all()   # captured, not run
    graph.launch()
    assert plvi_lib.plvi_stream_synchronize(st) == 0
    same_walk(fetch(), ref_walk(kf, origins))


@pytest.mark.gpu
def test_gpu_walk_refusals(plvi_lib):
    kf, origins, _ = walk_cases()["chain_3"]
    g = propagation(kf)
    sb = plvi_lib.plvi_gba_walk_scratch_bytes(3)
    assert sb == 5 * 256 and plvi_lib.plvi_gba_walk_scratch_bytes(-1) == 0
    dev = g.upload()
    kfs, eg = g.walk._structs(lambda grp, k: dev[(grp, k)].ptr)
    n = plvi.DeviceBuffer(64)
    out = plvi.GbaWalkOutputs(0, None, None, None, n.ptr, n.ptr + 4, n.ptr + 8, None)
    scr = plvi.DeviceBuffer(sb)
    stamps = dev[("kf", "kf_ba_for")].ptr
    call = lambda *a: plvi._status("plvi_gba_walk_device", *a)  # noqa: E731
    assert call(kfs, eg, None, 0, LOOP, stamps, out, scr.ptr, sb, None) == 0          # capacity 0: no lists needed
    assert call(kfs, eg, None, 0, LOOP, stamps, out, scr.ptr, sb - 1, None) == plvi.PLVI_E_BADARG
    assert call(kfs, eg, None, 1, LOOP, stamps, out, scr.ptr, sb, None) == plvi.PLVI_E_BADARG
    assert call(kfs, eg, None, 0, LOOP, None, out, scr.ptr, sb, None) == plvi.PLVI_E_BADARG
    part = plvi.EgKeyframes(eg.n_order, 0, order=eg.order, child_off=eg.child_off)
    assert call(kfs, part, None, 0, LOOP, stamps, out, scr.ptr, sb, None) == plvi.PLVI_E_BADARG
    big = plvi.CullKeyframes((1 << 24) + 1, 0, 0, 0, bad=kfs.bad)
    assert call(big, eg, None, 0, LOOP, stamps, out, scr.ptr, 1 << 40, None) == plvi.PLVI_E_CAPACITY
    plvi_lib.plvi_device_synchronize()


# ---------------------------------------------------------------- GPU: the correction
def correct_both_forms(m, compat=0, column=None):
    exp = ref_correct(m, compat, column)
    col = col_of(m)
    kf = dict(bad=m["kf_bad"], kf_ba_for=m["poses"]["kf_ba_for"])
    for form in ("batch", "host"):
        g = propagation(kf, m)
        got = getattr(g.correct, form)(m["kind"], LOOP, m["poses"], map=m["map"], compat=compat, column=column,
                                       fill=FILL)
        want_rc = plvi.PLVI_E_CAPACITY if exp["err"] else int(exp["counts"][1] + exp["counts"][2])
        assert got["rc"] == (want_rc if form == "host" else 0), (form, got["rc"])
        same_correct(got, exp, col)
        if form == "host" and column is None:
            assert got[col] is g.pools[m["kind"]][col]    # in place
    return exp


@pytest.mark.gpu
@pytest.mark.parametrize("kind", (POINTS, LINES))
@pytest.mark.parametrize("compat", (0, FMA))
def test_gpu_correct_crafted_in_place_and_separate(plvi_lib, kind, compat):
    m, expect = crafted_features(kind)
    exp = correct_both_forms(m, compat)
    assert {i: int(exp["state"][i]) for i in expect} == expect
    sentinel = np.full_like(m["feat"][col_of(m)], 777.0)
    exp = correct_both_forms(m, compat, column=sentinel)
    assert (exp[col_of(m)][[2, 3, 4, 6, 7, 8, 11]] == 777.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", (POINTS, LINES))
@pytest.mark.parametrize("n", (1, 65, 4097))
def test_gpu_correct_sizes_with_every_state(plvi_lib, kind, n):
    m = feature_map(kind, n, seed=8)
    if n == 1:
        for st, (stamp, ref) in enumerate(((OLD, 4), (LOOP, 0), (OLD, 1))):
            m["feat"]["bad"][:], m["feat"]["map_id"][:] = 0, 2
            m["feat"]["ba_for"][:], m["feat"]["ref_kf"][:] = stamp, ref
            assert correct_both_forms(m, FMA)["counts"].tolist() == [int(st == k) for k in range(3)]
        return
    for compat in (0, FMA):
        exp = correct_both_forms(m, compat)
        assert (exp["counts"] > 0).all() and exp["counts"].sum() == n


@pytest.mark.gpu
def test_gpu_compat_forms_differ_on_the_device(plvi_lib):
    m = feature_map(POINTS, 4097, seed=8)
    kf = dict(bad=m["kf_bad"], kf_ba_for=m["poses"]["kf_ba_for"])
    a = propagation(kf, m).correct.batch(POINTS, LOOP, m["poses"], map=2, compat=0)
    b = propagation(kf, m).correct.batch(POINTS, LOOP, m["poses"], map=2, compat=FMA)
    differ = (bits(a["pos"]) != bits(b["pos"])).any(axis=1)
    assert differ.sum() >= 1 and (a["state"][:4097][differ] == 2).all()


@pytest.mark.gpu
def test_gpu_correct_graph_capture_and_refusals(plvi_lib):
    m = feature_map(LINES, 65, seed=9)
    kf = dict(bad=m["kf_bad"], kf_ba_for=m["poses"]["kf_ba_for"])
    g = propagation(kf, m)
    step, fetch = g.correct.batch(LINES, LOOP, m["poses"], map=2, fill=FILL, run=False)
    st = ctypes.c_void_p()
    assert plvi_lib.plvi_stream_create(ctypes.byref(st)) == 0
    rcs = []
    graph = plvi.StepGraph(lambda s: rcs.append(step(s)), st.value)
    assert rcs == [0] and (fetch()["state"] == FILL8).all()
    graph.launch()
    assert plvi_lib.plvi_stream_synchronize(st) == 0
    same_correct(fetch(), ref_correct(m), "sep")
    with pytest.raises(ValueError):
        g.correct.batch(2, LOOP, m["poses"])
    n = plvi.DeviceBuffer(64)
    out = plvi.GbaCorrectOutputs(None, None, None, n.ptr, n.ptr + 16)
    pool, ef = plvi.LocalMapPool(0), plvi.EgFeatures()
    poses = plvi.GbaPoses(7)
    call = lambda *a: plvi._status("plvi_gba_correct_device", *a)  # noqa: E731
    assert call(pool, ef, None, None, poses, plvi.GbaParams(LINES, LOOP, 0, 0), out, None) == 0   # an empty pool
    assert call(pool, ef, None, None, poses, plvi.GbaParams(2, LOOP, 0, 0), out, None) == plvi.PLVI_E_BADARG
    assert call(plvi.LocalMapPool(-1), ef, None, None, poses, plvi.GbaParams(0, LOOP, 0, 0), out,
                None) == plvi.PLVI_E_BADARG
    assert call(plvi.LocalMapPool(3), ef, None, None, poses, plvi.GbaParams(0, LOOP, 0, 0), out,
                None) == plvi.PLVI_E_BADARG
    plvi_lib.plvi_device_synchronize()


# ---------------------------------------------------------------- GPU: the chain
@pytest.mark.gpu
def test_gpu_chain_walk_poses_correct_frustum(plvi_lib):
    """walk -> the caller's pass over the list for the new poses (numpy) -> correct writing the pool's pos in place
    -> plvi_frustum_points_batch reading that column where it lies, against the restatements and
    oracle_frustum_points."""
    import oracle_lib
    import util
    K, n = 40, 3000
    rng = np.random.default_rng(77)
    kf = random_tree(K, 21, stamped=range(0, K, 3))      # the solver saw every third keyframe, the origin among them
    kf["bad"][5] = 1
    prm = util.frustum_params(60)
    world = util.frustum_case(70, prm, n=n)
    feat = dict(bad=(rng.random(n) < 0.05).astype(u8), ref_kf=rng.integers(0, K, n).astype(i32),
                ba_for=np.where(rng.random(n) < 0.3, LOOP, OLD).astype(u32), pos=world["pos"].copy(),
                pos_gba=(world["pos"] + rng.normal(0, 0.02, (n, 3))).astype(f32))
    g = plvi.GBAPropagation({k: a.copy() for k, a in kf.items()}, feat)

    # A: the walk, its stamps left on the device
    w = g.walk.batch([0], LOOP, fill=FILL)
    exp_w = ref_walk(kf, [0])
    same_walk(w, exp_w)
    n_walk = int(w["n_walk"][0])
    assert 10 < n_walk < K and 5 < int(w["n_new"][0]) < n_walk

    # B: the caller's pass.  A parent stands before its children, so one pass gives every new pose.
    def pose(scale):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = rotation(rng), rng.normal(0, scale, 3)
        return T
    Tcw = [pose(3.0) for _ in range(K)]
    small = lambda: np.linalg.qr(np.eye(3) + rng.normal(0, 0.01, (3, 3)))[0]  # noqa: E731
    Tgba = {}
    for s in range(0, K, 3):
        Tgba[s] = Tcw[s].copy()
        q = small()
        Tgba[s][:3, :3] = (q * np.sign(np.diag(q))) @ Tcw[s][:3, :3]
        Tgba[s][:3, 3] += rng.normal(0, 0.03, 3)
    for s, p, new in zip(w["walk"][:n_walk], w["walk_parent"][:n_walk], w["walk_new"][:n_walk]):
        if new:
            Tgba[int(s)] = Tcw[s] @ np.linalg.inv(Tcw[p]) @ Tgba[int(p)]      # Tchildc * pKF->mTcwGBA
    bef, twc = np.zeros((K, 12), f32), np.zeros((K, 12), f32)
    for s in w["walk"][:n_walk]:
        Twc = np.linalg.inv(Tgba[int(s)])
        bef[s] = np.concatenate([Tcw[s][:3, :3].ravel(), Tcw[s][:3, 3]])
        twc[s] = np.concatenate([Twc[:3, :3].ravel(), Twc[:3, 3]])
    poses = dict(has_bef=w["visited"], tcw_bef=bef, twc=twc)

    # C: the correction in place, on the stamps the walk left
    r = g.correct.batch(POINTS, LOOP, poses, compat=FMA, stamps_on_device=True, fill=FILL)
    m = dict(kf_bad=kf["bad"], poses=dict(poses, kf_ba_for=exp_w["kf_ba_for"]), feat=feat, kind=POINTS, map=0)
    exp = ref_correct(m, FMA)
    assert r["rc"] == 0 and (exp["counts"] > 100).all()
    same_correct(r, exp, "pos")
    assert r["dev"]["pos"] == g.dev[("mp", "pos")].ptr

    # D: the frustum test reads the corrected column where it lies
    bufs = []

    def dev(a):
        a = np.ascontiguousarray(a)
        bufs.append(plvi.DeviceBuffer(max(a.nbytes, 4)))
        bufs[-1].upload(a)
        return ctypes.c_void_p(bufs[-1].ptr)
    V = ctypes.c_void_p
    d_fl, d_pr, d_lv, d_de = dev(np.zeros(n, u8)), dev(world["proj"]), dev(world["level"]), dev(world["depth"])
    d_prm = dev(np.frombuffer(bytes(prm), u8))
    assert plvi_lib.plvi_frustum_points_batch(1, d_prm, V(r["dev"]["pos"]), dev(world["normal"]), dev(world["dist"]),
                                              dev(world["in_flags"]), dev(np.array([n], i32)), n, d_fl, d_pr, d_lv,
                                              None, None, d_de, None, None) == 0
    plvi_lib.plvi_device_synchronize()
    want = oracle_lib.frustum_points(prm, dict(world, pos=exp["pos"]))
    assert np.array_equal(plvi.download(d_fl.value, np.zeros(n, u8)), want["flags"])
    assert plvi.download(d_pr.value, np.zeros((n, 4), f32)).tobytes() == want["proj"].tobytes()
    assert np.array_equal(plvi.download(d_lv.value, np.zeros(n, i32)), want["level"])
    assert plvi.download(d_de.value, np.zeros(n, f32)).tobytes() == want["depth"].tobytes()
    stale = oracle_lib.frustum_points(prm, world)
    assert stale["proj"].tobytes() != want["proj"].tobytes()      # and the correction is what decides it
