"""Packing helper for the count / capacity contract of the batched matchers (include/plvi_frontend.h,
"the count contract"): per-pair cases -> padded [P + 1][cap]... tables whose rows at or past each pair's
count hold *attractive poison* (values that change the answer when read: descriptors at distance 0 from the
other side's, real keypoints / lines, set flags, valid CSR indices, real unit directions), outputs pre-filled
with a canary no kernel produces, and one extra pair of slack behind pair P - 1 so that an off-by-one-pair
stride stays inside the allocation, where the checker sees it.

The packers are plain numpy (tests/test_batch_pack.py checks them without a GPU); `Device` and the `check_*`
functions serve the GPU tests (tests/test_batch_contract_gpu.py)."""
import ctypes

import numpy as np

CANARY = -7
SLACK = 1  # extra pairs behind the last one


def pack_rows(tables, cap, poison):
    """[P + SLACK][cap]... from per-pair arrays [n_p]...; rows n_p.. of pair p repeat poison[p] (non-empty,
    same row shape) cyclically; the slack pairs are all poison."""
    P = len(tables)
    first = np.asarray(tables[0])
    out = np.empty((P + SLACK, cap) + first.shape[1:], first.dtype)
    for p in range(P + SLACK):
        t = np.asarray(tables[p]) if p < P else first[:0]
        src = np.asarray(poison[min(p, P - 1)], first.dtype)
        assert len(t) <= cap and len(src) > 0 and src.shape[1:] == first.shape[1:]
        out[p, :len(t)] = t
        out[p, len(t):] = src[np.arange(cap - len(t)) % len(src)]
    return out


def unpack_rows(packed, counts):
    return [packed[p, :n] for p, n in enumerate(counts)]


def counts_array(ns, override=None):
    """Device count array [P + SLACK]: the real counts, `override` {pair: count} for the negative / over-count
    pairs, and CANARY-free garbage (a large count) for the slack pair, which no launch may look at."""
    c = np.array(list(ns) + [1 << 20] * SLACK, np.int32)
    for p, v in (override or {}).items():
        c[p] = v
    return c


def _first_nonempty(arrays):
    for a in arrays:
        if len(a):
            return np.asarray(a)
    raise AssertionError("every case is empty")


def _or(a, *fallbacks):
    for x in (a,) + fallbacks:
        if len(x):
            return x
    raise AssertionError("no poison source")


# ------------------------------------------------------------------ kNN-2 / LineMatcher::match
def pack_knn(cases, q_cap, t_cap):
    """cases: [(q [nq][32], t [nt][32])].  Train padding = that pair's queries, query padding = its train rows:
    either one read past its count finds a distance-0 row."""
    fb = _first_nonempty([c[0] for c in cases] + [c[1] for c in cases])
    q = pack_rows([c[0] for c in cases], q_cap, [_or(c[1], c[0], fb) for c in cases])
    t = pack_rows([c[1] for c in cases], t_cap, [_or(c[0], c[1], fb) for c in cases])
    return {"q": q, "t": t, "nq": [len(c[0]) for c in cases], "nt": [len(c[1]) for c in cases]}


# ------------------------------------------------------------------ SearchByBoW
BOW_POISON_NODE = 1 << 20  # above every NodeId of util.bow_case


def bow_csr(fv):
    nodes = np.array(sorted(fv), np.int32)
    off = np.zeros(len(nodes) + 1, np.int32)
    idx = []
    for i, n in enumerate(nodes):
        idx.extend(fv[int(n)])
        off[i + 1] = len(idx)
    return nodes, off, np.array(idx, np.int32)


def bow_poison_nodes(case, kf_cap, f_cap, node_cap, rot=20.0):
    """The poison FeatureVector nodes of one case: node BOW_POISON_NODE + j, shared by both sides, holds the
    KF padding row kf_n + j (descriptor = F row j's, live, angle = F row j's + rot) and the real F row j.  A
    merge walk that runs past both node counts matches F row j at distance 0 unless it was matched already.
    Returns (n_poison, kf rows (desc, angle, live) to append)."""
    kd, ka, kl, kfv, fd, fa, ffv = case
    nK, nFn = len(kfv), len(ffv)
    nki, nfi = sum(map(len, kfv.values())), sum(map(len, ffv.values()))
    k = max(0, min(node_cap - nK, node_cap - nFn, kf_cap - nki, f_cap - nfi, kf_cap - len(kd), len(fd)))
    desc = np.asarray(fd[:k], np.uint8).reshape(k, 32)
    ang = np.mod(np.asarray(fa[:k], np.float64) + rot, 360).astype(np.float32)
    return k, (desc, ang, np.ones(k, np.uint8))


def bow_poisoned_case(case, kf_cap, f_cap, node_cap):
    """The case as a kernel would see it that ignores both node counts: poison nodes made real."""
    kd, ka, kl, kfv, fd, fa, ffv = case
    k, (pd, pa, pl) = bow_poison_nodes(case, kf_cap, f_cap, node_cap)
    kfv2, ffv2 = dict(kfv), dict(ffv)
    for j in range(k):
        kfv2[BOW_POISON_NODE + j] = [len(kd) + j]
        ffv2[BOW_POISON_NODE + j] = [j]
    return (np.concatenate([kd, pd]), np.concatenate([ka, pa]), np.concatenate([kl, pl]), kfv2, fd, fa, ffv2)


def pack_bow(cases, kf_cap, f_cap, node_cap):
    """cases: util.bow_case tuples.  KF padding rows: first the poison nodes' rows, then live copies of F
    descriptors; F padding rows: copies of KF descriptors; node / offset / index padding: the poison nodes,
    then empty shared nodes and valid indices."""
    fbd = _first_nonempty([c[0] for c in cases] + [c[4] for c in cases])
    one = np.ones(1, np.uint8)
    ang = np.array([20.0], np.float32)
    kdl, kal, kll, fdl, fal = [], [], [], [], []
    P = len(cases)
    kn = np.zeros((P + SLACK, node_cap), np.int32)
    ko = np.zeros((P + SLACK, node_cap + 1), np.int32)
    ki = np.zeros((P + SLACK, kf_cap), np.int32)
    fn, fo, fi = kn.copy(), ko.copy(), np.zeros((P + SLACK, f_cap), np.int32)
    for p, c in enumerate(cases):
        kd, ka, kl, kfv, fd, fa, ffv = c
        k, (pd, pa, pl) = bow_poison_nodes(c, kf_cap, f_cap, node_cap)
        kdl.append(np.concatenate([kd, pd]))
        kal.append(np.concatenate([ka, pa]))
        kll.append(np.concatenate([kl, pl]))
        fdl.append(fd)
        fal.append(fa)
        for (nodes, off, idx), N, O, I, pidx in ((bow_csr(kfv), kn, ko, ki, len(kd) + np.arange(k)),
                                                 (bow_csr(ffv), fn, fo, fi, np.arange(k))):
            nn, ni = len(nodes), len(idx)
            N[p, :nn] = nodes
            N[p, nn:] = BOW_POISON_NODE + np.arange(node_cap - nn)
            O[p, :nn + 1] = off
            O[p, nn + 1:] = ni + np.minimum(np.arange(1, node_cap - nn + 1), k)
            I[p, :ni] = idx
            I[p, ni:ni + k] = pidx
    for s in range(P, P + SLACK):  # slack pair: one shared node over row 0
        kn[s] = fn[s] = BOW_POISON_NODE + np.arange(node_cap)
        ko[s, 1:] = fo[s, 1:] = 1
    out = {"kd": pack_rows(kdl, kf_cap, [_or(c[4], c[0], fbd) for c in cases]),
           "ka": pack_rows(kal, kf_cap, [_or(c[5], ang) for c in cases]),
           "kl": pack_rows(kll, kf_cap, [one] * P),
           "fd": pack_rows(fdl, f_cap, [_or(c[0], c[4], fbd) for c in cases]),
           "fa": pack_rows(fal, f_cap, [_or(c[1], ang) for c in cases]),
           "kn": kn, "ko": ko, "ki": ki, "fn": fn, "fo": fo, "fi": fi,
           "kf_n": [len(c[0]) for c in cases], "f_n": [len(c[4]) for c in cases],
           "kc": [len(c[3]) for c in cases], "fc": [len(c[6]) for c in cases]}
    return out


# ------------------------------------------------------------------ matchGrid
def grid_csr(grid):
    cols, rows = len(grid), len(grid[0])
    off = np.zeros(cols * rows + 1, np.int32)
    idx = []
    for x in range(cols):
        for y in range(rows):
            idx.extend(grid[x][y])
            off[x * rows + y + 1] = len(idx)
    return off, np.array(idx, np.int32)


def pack_csr_grid(grids, idx_cap):
    """cell_off [P + SLACK][ncell + 1], cell_idx [P + SLACK][idx_cap]; index padding = the pair's own indices
    (valid line numbers), the slack pair = an empty grid over index 0."""
    P = len(grids)
    ncell = len(grids[0]) * len(grids[0][0])
    co = np.zeros((P + SLACK, ncell + 1), np.int32)
    ci = np.zeros((P + SLACK, idx_cap), np.int32)
    for p, g in enumerate(grids):
        off, idx = grid_csr(g)
        assert len(idx) <= idx_cap
        co[p] = off
        ci[p, :len(idx)] = idx
        if len(idx):
            ci[p, len(idx):] = idx[np.arange(idx_cap - len(idx)) % len(idx)]
    return co, ci


def grid_poison_left(case):
    """Left-line poison of a stereo_line_case: copies of real left lines whose descriptor is that of a right
    line listed in the cell of the copy's start point -- a later left line at distance 0 from a right line
    takes it from its true match in the mutual check."""
    lines1, desc1, grid, desc2, dirs = case
    if not len(lines1) or not len(desc2):
        return lines1[:0], desc1[:0]
    cols, rows = len(grid), len(grid[0])
    d = np.empty((len(lines1), 32), np.uint8)
    for j, l in enumerate(lines1):
        cell = grid[int(np.clip(l[0], 0, cols - 1))][int(np.clip(l[1], 0, rows - 1))]
        d[j] = desc2[cell[0] if cell else j % len(desc2)]
    return lines1, d


def pack_match_grid(cases, cap1, cap2, idx_cap):
    """cases: util.stereo_line_case tuples (lines1, desc1, grid, desc2, directions2)."""
    fbl = _first_nonempty([c[0] for c in cases])
    fbd = _first_nonempty([c[1] for c in cases])
    fbv = _first_nonempty([c[4] for c in cases])
    pois = [grid_poison_left(c) for c in cases]
    co, ci = pack_csr_grid([c[2] for c in cases], idx_cap)
    return {"lines1": pack_rows([c[0] for c in cases], cap1, [_or(pl, fbl) for pl, _ in pois]),
            "desc1": pack_rows([c[1] for c in cases], cap1, [_or(pd, fbd) for _, pd in pois]),
            "desc2": pack_rows([c[3] for c in cases], cap2, [_or(c[1], fbd) for c in cases]),
            "dirs2": pack_rows([c[4] for c in cases], cap2, [_or(c[4], fbv) for c in cases]),
            "cell_off": co, "cell_idx": ci,
            "n1": [len(c[0]) for c in cases], "n2": [len(c[3]) for c in cases]}


# ------------------------------------------------------------------ LineMatcher::SearchByProjection
LINE_PROJ_CUR = ("cur_angle", "cur_desc", "cur_blocked")
LINE_PROJ_LAST = ("last_flags", "x3dc", "last_octave", "ml_desc")


def pack_line_proj(cases, cur_cap, last_cap, idx_cap):
    """cases: util.line_proj_case dicts.  Last-frame padding = copies of the pair's own last-frame lines with
    flag bits 0 and 1 set (a duplicate re-assigns or blocks its original's current line); current padding =
    real angles, MapLine descriptors (distance 0), unblocked."""
    fb = next(c for c in cases if len(c["cur_angle"]) and len(c["last_flags"]))
    out = {}
    for k in LINE_PROJ_CUR:
        src = "ml_desc" if k == "cur_desc" else k
        out[k] = pack_rows([c[k] for c in cases], cur_cap,
                           [np.zeros(1, np.uint8) if k == "cur_blocked" else _or(c[src], c[k], fb[src]) for c in cases])
    for k in LINE_PROJ_LAST:
        pois = [_or(c[k], fb[k]) for c in cases]
        if k == "last_flags":
            pois = [f | 3 for f in pois]
        out[k] = pack_rows([c[k] for c in cases], last_cap, pois)
    out["cell_off"], out["cell_idx"] = pack_csr_grid([c["grid"] for c in cases], idx_cap)
    out["n_cur"] = [len(c["cur_angle"]) for c in cases]
    out["n_last"] = [len(c["last_flags"]) for c in cases]
    return out


def line_proj_sub(case, n_cur=None, n_last=None, grid=None):
    """A line_proj_case cut to its first n_cur / n_last rows (an emptied side needs an empty grid)."""
    c = dict(case)
    for k in LINE_PROJ_CUR:
        c[k] = case[k][:n_cur]
    for k in LINE_PROJ_LAST:
        c[k] = case[k][:n_last]
    if grid is not None:
        c["grid"] = grid
    return c


def empty_grid(cols, rows):
    return [[[] for _ in range(rows)] for _ in range(cols)]


# ------------------------------------------------------------------ keypoint-grid matchers (proj.hip, init_match.hip)
def own(key):
    """Poison = copies of the pair's own real rows of `key`."""
    return lambda c: c[key]


def const(value, dtype):
    return lambda c: np.array([value], dtype)


def ingrid_mask(c, key, margin=8.0):
    k = c[key]
    min_x, max_x, min_y, max_y = (float(v) for v in c["grid"][:4])
    return (k["x"] > min_x + margin) & (k["x"] < max_x - margin) & (k["y"] > min_y + margin) & \
        (k["y"] < max_y - margin)


def ingrid(key, margin=8.0):
    """Copies of the pair's keypoints that lie well inside the image bounds of c["grid"] (in the grid)."""
    return lambda c: c[key][ingrid_mask(c, key, margin)]


def pack_keyed(cases, cap, spec):
    """{key: [P + SLACK][cap]...} for dict cases; spec = {key: poison(case) -> rows}.  A pair with no poison
    source of its own (an emptied side) borrows the first pair's that has one."""
    out = {}
    for key, poison in spec.items():
        src = [np.asarray(poison(c)) for c in cases]
        fb = _first_nonempty(src)
        out[key] = pack_rows([c[key] for c in cases], cap, [_or(s, fb) for s in src])
    return out


def cut(case, **sides):
    """The dict case with the listed keys cut to n rows: cut(c, cur=(keys, n), ...)."""
    c = dict(case)
    for keys, n in sides.values():
        for k in keys:
            c[k] = case[k][:n]
    return c


_POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b):
    """[len(a)][len(b)] Hamming distances of 32-byte descriptor rows."""
    a, b = np.asarray(a, np.uint8).reshape(-1, 32), np.asarray(b, np.uint8).reshape(-1, 32)
    out = np.empty((len(a), len(b)), np.int32)
    for i in range(0, len(a), 128):
        out[i:i + 128] = _POPCOUNT[a[i:i + 128, None, :] ^ b[None, :, :]].sum(-1)
    return out


def family(builder):
    """key -> poison(case) for specs whose padding rows are built together: builder(case) -> {key: rows}."""
    cache = {}

    def key(k):
        def f(c):
            if id(c) not in cache:
                cache[id(c)] = (c, builder(c))  # the case is kept, so its id stays its own
            return cache[id(c)][1][k]
        return f
    return key


def free_keypoints(c, kps="cur_kps", desc="cur_desc", blocked="cur_blocked", uright=None, th=100):
    """Keypoints that are still free in the true answer whatever it is: in the grid, not blocked on entry,
    without a stereo coordinate, and farther than `th` (TH_HIGH) from every real point's descriptor."""
    k = c[kps]
    if not len(k):
        return np.zeros(0, np.int64)
    keep = ingrid_mask(c, kps) & (np.asarray(c[blocked]) == 0)
    if uright is not None and c.get(uright) is not None:
        keep &= np.asarray(c[uright]) <= 0
    if len(c["mp_desc"]):
        keep &= hamming(c[desc], c["mp_desc"]).min(1) > th
    return np.flatnonzero(keep)


def _aimed(c, kps, desc, idx, z=5.0, unproject=None):
    """Camera-frame points that project exactly onto keypoints idx, with those keypoints' own descriptor,
    octave and angle (+10 degrees: the rotation every generated case has)."""
    k = c[kps][idx]
    fx, fy, cx, cy = (float(v) for v in c["camera"][:4])
    u, v = k["x"].astype(np.float64), k["y"].astype(np.float64)
    rx, ry = unproject(u, v) if unproject else ((u - cx) / fx, (v - cy) / fy)
    return {"x3dc": np.stack([rx * z, ry * z, np.full(len(k), z)], 1).astype(np.float32),
            "octave": k["octave"].astype(np.int32), "angle": np.mod(k["angle"] + 10, 360).astype(np.float32),
            "mp_desc": np.asarray(c[desc])[idx]}


def _proj_poison(c):
    a = _aimed(c, "cur_kps", "cur_desc", free_keypoints(c, uright="cur_uright"))
    return {"x3dc": a["x3dc"], "last_octave": a["octave"], "last_angle": a["angle"], "mp_desc": a["mp_desc"],
            "flags": np.full(len(a["octave"]), 3, np.uint8)}


def _reloc_poison(c):
    a = _aimed(c, "cur_kps", "cur_desc", free_keypoints(c))
    n = len(a["octave"])
    return {"kf_flags": np.ones(n, np.uint8), "x3dc": a["x3dc"], "level": a["octave"], "kf_angle": a["angle"],
            "dist": np.tile(np.array([5.0, 2.5, 10.0], np.float32), (n, 1)), "mp_desc": a["mp_desc"]}


def _local_poison(c):
    idx = free_keypoints(c, uright="cur_uright")
    k = c["cur_kps"][idx]
    n = len(k)
    return {"mp_flags": np.full(n, 3, np.uint8), "mp_level": k["octave"].astype(np.int32),
            "mp_proj": np.stack([k["x"], k["y"], k["x"], np.ones(n, np.float32)], 1).astype(np.float32),
            "mp_desc": np.asarray(c["cur_desc"])[idx]}


def _proj2_poison(c):
    import util
    un = (lambda u, v: util._kb8_unproject(u, v, util.KB8_TUMVI)) if c.get("kb8") is not None else None
    a = _aimed(c, "kps", "desc", free_keypoints(c, "kps", "desc", "blocked"), unproject=un)
    ang = np.deg2rad(2.0)  # the rig of util.projection_stereo_case
    R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    x3r = (a["x3dc"].astype(np.float64) @ R.T + np.array([-0.11, 0.002, 0.001])).astype(np.float32)
    return {"x3dc": a["x3dc"], "x3dr": x3r, "last_octave": a["octave"], "last_angle": a["angle"],
            "mp_desc": a["mp_desc"], "flags": np.full(len(x3r), 3, np.uint8)}


def _local2_poison(c):
    idx = free_keypoints(c, "kps", "desc", "blocked")
    k = c["kps"][idx]
    n = len(k)
    proj = np.stack([k["x"], k["y"], np.zeros(n), np.ones(n)], 1).astype(np.float32)
    return {"mp_flags": np.full(n, 3, np.uint8), "mp_proj": proj, "mp_level": k["octave"].astype(np.int32),
            "mp_proj_r": proj, "mp_level_r": np.full(n, -1, np.int32), "mp_desc": np.asarray(c["desc"])[idx]}


def _spec(builder, keys):
    key = family(builder)
    return {k: key(k) for k in keys}


# One-camera current frame / the tables behind it, by family (keys of the util.*_case dicts).  The padding
# rows of the last-frame / KeyFrame / MapPoint tables aim exactly at a free keypoint of the pair, with that
# keypoint's own descriptor: the first row read past a count takes a keypoint the true answer leaves alone.
CUR = {"cur_kps": ingrid("cur_kps"), "cur_desc": own("mp_desc"), "cur_blocked": const(0, np.uint8)}
CUR_U = dict(CUR, cur_uright=own("cur_uright"))  # stereo-rectified frames: mvuRight as well
PROJ_LAST = _spec(_proj_poison, ("x3dc", "last_octave", "last_angle", "mp_desc", "flags"))
RELOC_KF = _spec(_reloc_poison, ("kf_flags", "x3dc", "dist", "level", "kf_angle", "mp_desc"))
LOCAL_MP = _spec(_local_poison, ("mp_flags", "mp_proj", "mp_level", "mp_desc"))
# two-camera frames
LEFT = {"kps": ingrid("kps"), "desc": own("mp_desc"), "blocked": const(0, np.uint8)}
RIGHT = {"kps_r": ingrid("kps_r"), "desc_r": own("mp_desc"), "blocked_r": const(0, np.uint8)}
PROJ2_LAST = _spec(_proj2_poison, ("x3dc", "x3dr", "last_octave", "last_angle", "mp_desc", "flags"))
LOCAL2_LEFT = dict(LEFT, l2r=const(-1, np.int32))
LOCAL2_RIGHT = dict(RIGHT, r2l=const(-1, np.int32))
LOCAL2_MP = _spec(_local2_poison, ("mp_flags", "mp_proj", "mp_level", "mp_proj_r", "mp_level_r", "mp_desc"))


# The initializer (cases {"k1", "d1", "prev", "k2", "d2"}): F2 padding = a level-0 keypoint at an F1 point's
# vbPrevMatched position with that point's descriptor (the point matches it at distance 0); F1 padding = a copy
# of the F2 keypoint nearest to a real F1 descriptor, with the F2 descriptor (it steals that keypoint).
def _init_k2_poison(c):
    k1 = c["k1"]
    idx = np.flatnonzero(k1["octave"] == 0)
    k = k1[idx].copy()
    k["x"], k["y"] = c["prev"][idx, 0], c["prev"][idx, 1]
    k["angle"] = np.mod(k["angle"] - 10, 360)
    return {"k2": k, "d2": np.asarray(c["d1"])[idx]}


def _init_k1_poison(c):
    k2 = c["k2"]
    if not len(k2) or not len(c["d1"]):
        return {"k1": k2[:0], "d1": np.asarray(c["d2"])[:0], "prev": np.zeros((0, 2), np.float32)}
    d = hamming(c["d2"], c["d1"]).min(1)
    idx = np.flatnonzero((k2["octave"] == 0) & (d > 0))
    idx = idx[np.argsort(d[idx], kind="stable")]
    k = k2[idx].copy()
    k["angle"] = np.mod(k["angle"] + 10, 360)
    return {"k1": k, "d1": np.asarray(c["d2"])[idx], "prev": np.stack([k["x"], k["y"]], 1).astype(np.float32)}


INIT_K1 = _spec(_init_k1_poison, ("k1", "d1", "prev"))
INIT_K2 = _spec(_init_k2_poison, ("k2", "d2"))


# ComputeStereoMatches_Lines (cases {"klL", "dL", "klR", "dR"}): padding = copies of the side's own lines, nearest
# descriptor first, carrying the nearest descriptor of the other side -- a left copy takes its original's right
# line in the mutual check, a right copy is a distance-0 candidate in the same grid cells as its original.
def _nearest_other(c, kl, d_own, d_other):
    if not len(c[kl]) or not len(c[d_other]):
        return {kl: c[kl][:0], d_own: np.asarray(c[d_own])[:0]}
    h = hamming(c[d_own], c[d_other])
    order = np.argsort(h.min(1), kind="stable")
    return {kl: c[kl][order], d_own: np.asarray(c[d_other])[h.argmin(1)[order]]}


STEREO_L = _spec(lambda c: _nearest_other(c, "klL", "dL", "dR"), ("klL", "dL"))
STEREO_R = _spec(lambda c: _nearest_other(c, "klR", "dR", "dL"), ("klR", "dR"))


# ------------------------------------------------------------------ device side (GPU tests only)
class Device:
    """Uploads packed tables and canary-filled outputs; keeps the buffers alive."""

    def __init__(self):
        import plvi
        self.plvi = plvi
        self.lib = plvi.load()
        self._bufs = []

    def up(self, arr):
        arr = np.ascontiguousarray(arr)
        b = self.plvi.DeviceBuffer(max(arr.nbytes, 4))
        b.upload(arr)
        self._bufs.append(b)
        return ctypes.c_void_p(b.ptr)

    def table(self, arr):
        """An in/out or status table: uploads arr, returns (pointer, download())."""
        arr = np.ascontiguousarray(arr)
        ptr = self.up(arr)
        b = self._bufs[-1]

        def get():
            self.lib.plvi_device_synchronize()
            return b.download(np.empty_like(arr))
        return ptr, get

    def canary(self, *shape):
        """int32 output [shape], every word CANARY.  Returns (pointer, download())."""
        return self.table(np.full(shape, CANARY, np.int32))


def assign_grid(dev, d_kps, d_cnt, cap, P, grid, kps_list):
    """plvi_assign_grid_batch into canary-filled tables, checked against the oracle: cell_off is written whole
    for every frame, cell_idx only up to the frame's in-grid count.  grid = (min_x, -, min_y, -, inv_w, inv_h);
    returns the device pointers (cell_off, cell_idx)."""
    import oracle_lib
    co, get_co = dev.canary(P + SLACK, 3073)
    ci, get_ci = dev.canary(P + SLACK, cap)
    dev.plvi.assign_grid_batch(d_kps.value, d_cnt.value, cap, P,
                               dev.plvi.GridParams(grid[0], grid[2], grid[4], grid[5]), co.value, ci.value)
    refs = [oracle_lib.assign_grid(k["x"], k["y"], grid) for k in kps_list]
    check_rows(get_co(), [eo for eo, _ in refs], "assign_grid cell_off")
    check_rows(get_ci(), [ei for _, ei in refs], "assign_grid cell_idx")
    return co, ci


def check_rows(out, refs, what):
    """out [P + SLACK][cap]: rows [0, n_p) of pair p equal refs[p] (n_p = its length, the clamped count); every
    other row of the pair and the whole slack still hold the canary."""
    P = len(refs)
    for p, ref in enumerate(refs):
        n = len(ref)
        np.testing.assert_array_equal(out[p, :n], ref, err_msg=f"{what}: pair {p} rows [0, {n})")
        bad = np.flatnonzero(out[p, n:] != CANARY)
        assert bad.size == 0, f"{what}: pair {p} wrote rows {n + bad[:8]} past its count {n}"
    assert (out[P:] == CANARY).all(), f"{what}: wrote into the slack behind pair {P - 1}"


def check_counts(got, exp, what):
    P = len(exp)
    np.testing.assert_array_equal(got[:P], np.asarray(exp, np.int32), err_msg=f"{what}: per-pair counts")
    assert (got[P:] == CANARY).all(), f"{what}: count written behind pair {P - 1}"
