"""The count / capacity contract of the batched matchers (include/plvi_frontend.h, "the count contract"),
bit-exact against the oracle: every entry point runs one batch that holds a full pair (count == cap), an
empty side (first one, then the other), an over-count pair (count = cap + 3, read as cap), a negative count
(read as 0) and a small pair, with unequal capacities on the two sides.  The tables come from
tests/batch_pack.py: padding rows hold attractive poison, outputs a canary, and one extra pair of slack sits
behind the last pair -- so a read past a count changes the answer, a write past it destroys a canary, and a
wrong per-pair stride does one or the other inside the allocation.

Also here: kNN-2 at its tile edges (256 queries per block, 256 train rows per LDS chunk), the 1024-candidate
limit of the two grid_match.hip kernels with its error report, and the octave-out-of-range report of
plvi_line_search_projection_batch."""
import ctypes

import numpy as np
import pytest

import batch_pack as bp
import oracle_lib as ol
import util

pytestmark = pytest.mark.gpu

V = ctypes.c_void_p
INT_MAX = 2 ** 31 - 1
# Pair roles of every contract batch.  The negative-count pair sits right behind the over-count one: its output
# rows are all canary, so rows written past the over-count pair's capacity cannot hide behind expected values.
FULL, EMPTY_A, OVER, NEG, EMPTY_B, SMALL = range(6)


def _desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


# ------------------------------------------------------------------ kNN-2 / LineMatcher::match
Q_CAP, T_CAP = 300, 260


@pytest.fixture(scope="module")
def knn_batch():
    rng = np.random.default_rng(31)
    big = [util.near_duplicate_descriptors(rng, T_CAP, Q_CAP, p_flip=0.05) for _ in range(2)]
    mid = util.near_duplicate_descriptors(rng, 100, 120, p_flip=0.05)
    small = util.near_duplicate_descriptors(rng, 5, 7, p_flip=0.05)
    none = _desc(rng, 0)
    cases = [big[0], (none, mid[1]), big[1], (none, none), (mid[0], none), small]
    pk = bp.pack_knn(cases, Q_CAP, T_CAP)
    pk["cases"] = cases
    pk["dq"] = bp.counts_array(pk["nq"], {OVER: Q_CAP + 3, NEG: -2})
    pk["dt"] = bp.counts_array(pk["nt"], {OVER: T_CAP + 3, NEG: -5})
    return pk


def test_knn2_batch_contract(plvi_lib, knn_batch):
    b, dev = knn_batch, bp.Device()
    P = len(b["cases"])
    outs = [dev.canary(P + bp.SLACK, Q_CAP) for _ in range(4)]
    rc = plvi_lib.plvi_hamming_knn2_batch(dev.up(b["q"]), dev.up(b["dq"]), Q_CAP, dev.up(b["t"]), dev.up(b["dt"]),
                                          T_CAP, P, *[o[0] for o in outs], None)
    assert rc == 0
    refs = [ol.knn2(q, t) for q, t in b["cases"]]
    for k, name in enumerate(["idx0", "d0", "idx1", "d1"]):
        bp.check_rows(outs[k][1](), [r[k] for r in refs], f"knn2 {name}")
    assert refs[EMPTY_B][0].tolist() == [-1] * 120 and refs[EMPTY_B][1][0] == INT_MAX


def test_line_match_batch_contract(plvi_lib, knn_batch):
    b, dev = knn_batch, bp.Device()
    P = len(b["cases"])
    scratch = dev.up(np.zeros(4 * (P + bp.SLACK) * (Q_CAP + T_CAP), np.int32))
    m12, get_m = dev.canary(P + bp.SLACK, Q_CAP)
    nm, get_n = dev.canary(P + bp.SLACK)
    rc = plvi_lib.plvi_line_match_batch(dev.up(b["q"]), dev.up(b["dq"]), Q_CAP, dev.up(b["t"]), dev.up(b["dt"]), T_CAP,
                                        P, 0.9, scratch, m12, nm, None)
    assert rc == 0
    refs, cnts = [], []
    for q, t in b["cases"]:
        if len(q) >= 2 and len(t) >= 2:
            n, m = ol.match(q, t, 0.9)
        else:  # fewer than 2 rows on a train side: no match (the reference would index matches_[i][1])
            n, m = 0, np.full(len(q), -1, np.int32)
        refs.append(m)
        cnts.append(n)
    assert cnts[FULL] > 50 and cnts[OVER] > 50
    bp.check_rows(get_m(), refs, "line_match matches_12")
    bp.check_counts(get_n(), cnts, "line_match")


# kNN-2 tile edges: kKnnQ = 256 queries per block, kKnnChunk = 256 train rows per LDS chunk (match.hip)
def _run_knn(plvi_lib, cases, q_cap, t_cap):
    pk = bp.pack_knn(cases, q_cap, t_cap)
    dev = bp.Device()
    P = len(cases)
    outs = [dev.canary(P + bp.SLACK, q_cap) for _ in range(4)]
    rc = plvi_lib.plvi_hamming_knn2_batch(dev.up(pk["q"]), dev.up(bp.counts_array(pk["nq"])), q_cap, dev.up(pk["t"]),
                                          dev.up(bp.counts_array(pk["nt"])), t_cap, P, *[o[0] for o in outs], None)
    assert rc == 0
    refs = [ol.knn2(q, t) for q, t in cases]
    got = [o[1]() for o in outs]
    for k, name in enumerate(["idx0", "d0", "idx1", "d1"]):
        bp.check_rows(got[k], [r[k] for r in refs], f"knn2 {name}")
    return got


def test_knn2_query_block_edges(plvi_lib):
    """nq around one and two 256-query blocks under nq_cap = 600 (3 blocks launched per pair): a partly
    active last block, whole blocks past the count, and an empty pair between two full ones."""
    rng = np.random.default_rng(41)
    cases = [util.near_duplicate_descriptors(rng, 100, nq) for nq in (255, 256, 257, 512, 513)]
    _run_knn(plvi_lib, cases, 600, 128)
    full = [util.near_duplicate_descriptors(rng, 64, 600) for _ in range(2)]
    _run_knn(plvi_lib, [full[0], (_desc(rng, 0), full[0][1]), full[1]], 600, 64)


def test_knn2_train_chunk_edges_and_ties(plvi_lib):
    """nt around one and two 256-row LDS chunks under nt_cap = 600, with identical train rows on both sides of
    a chunk edge (255 | 256) and two chunks apart (0, 512): the lower index wins, the other is second."""
    rng = np.random.default_rng(43)
    nts = (1, 2, 255, 256, 257, 511, 512, 513)
    cases = []
    for nt in nts:
        q, t = util.near_duplicate_descriptors(rng, nt, 70)
        if nt >= 257:
            t[256] = t[255]
            q[0] = t[255]
        if nt >= 513:
            t[512] = t[0]
            q[1] = t[0]
        cases.append((q, t))
    idx0, d0, idx1, d1 = _run_knn(plvi_lib, cases, 96, 600)
    for p, nt in enumerate(nts):
        if nt >= 257:
            assert (idx0[p, 0], d0[p, 0], idx1[p, 0], d1[p, 0]) == (255, 0, 256, 0)
        if nt >= 513:
            assert (idx0[p, 1], d0[p, 1], idx1[p, 1], d1[p, 1]) == (0, 0, 512, 0)


# ------------------------------------------------------------------ SearchByBoW
KF_CAP, F_CAP, NODE_CAP = 330, 301, 24  # odd f_cap: the int2 LDS region behind s_mk needs its own alignment


@pytest.fixture(scope="module")
def bow_batch():
    full = util.bow_case(70, n_kf=300, n_f=F_CAP, n_nodes=NODE_CAP, zipf=0.0, dup=0.8)
    over = util.bow_case(71, n_kf=KF_CAP, n_f=F_CAP, n_nodes=NODE_CAP, zipf=0.0, dup=0.8)
    mid = util.bow_case(72, n_kf=200, n_f=220, n_nodes=20)
    small = util.bow_case(73, n_kf=150, n_f=160, n_nodes=20)
    for c in (full, over):  # node counts == node_cap on both sides
        assert len(c[3]) == NODE_CAP and len(c[6]) == NODE_CAP
    kd, ka, kl, kfv, fd, fa, ffv = mid
    no_f = (kd, ka, kl, kfv, fd[:0], fa[:0], {})
    no_kf = (kd[:0], ka[:0], kl[:0], {}, fd, fa, ffv)
    nothing = (kd[:0], ka[:0], kl[:0], {}, fd[:0], fa[:0], {})
    cases = [full, no_f, over, nothing, no_kf, small]
    pk = bp.pack_bow(cases, KF_CAP, F_CAP, NODE_CAP)
    pk["cases"] = cases
    pk["d_fn"] = bp.counts_array(pk["f_n"], {OVER: F_CAP + 3, NEG: -3})
    pk["d_kc"] = bp.counts_array(pk["kc"], {OVER: NODE_CAP + 3, NEG: -1})
    pk["d_fc"] = bp.counts_array(pk["fc"], {OVER: NODE_CAP + 3, NEG: -2})
    return pk


@pytest.mark.parametrize("stereo", [False, True])
def test_search_by_bow_batch_contract(plvi_lib, bow_batch, stereo):
    b, dev = bow_batch, bp.Device()
    P = len(b["cases"])
    nleft = [150, 0, 100, 5, -1, 80]
    out, get_m = dev.canary(P + bp.SLACK, F_CAP)
    cnt, get_n = dev.canary(P + bp.SLACK)
    args = [P, 0.75, 1, KF_CAP, F_CAP, NODE_CAP] + [dev.up(b[k]) for k in ("kd", "ka", "kl", "kn", "ko")] + \
        [dev.up(b["d_kc"]), dev.up(b["ki"]), dev.up(b["fd"]), dev.up(b["fa"]), dev.up(b["d_fn"]), dev.up(b["fn"]),
         dev.up(b["fo"]), dev.up(b["d_fc"]), dev.up(b["fi"])]
    if stereo:
        rc = plvi_lib.plvi_search_by_bow_stereo_batch(*args, dev.up(np.array(nleft + [7] * bp.SLACK, np.int32)), out,
                                                      cnt, None)
    else:
        rc = plvi_lib.plvi_search_by_bow_batch(*args, out, cnt, None)
    assert rc == 0
    refs = [ol.search_by_bow(*c, 0.75, True, f_nleft=nleft[p] if stereo else -1) for p, c in enumerate(b["cases"])]
    assert refs[FULL][0] > 30 and refs[OVER][0] > 30 and refs[SMALL][0] > 10
    bp.check_rows(get_m(), [m for _, m in refs], "search_by_bow match_kf")
    bp.check_counts(get_n(), [n for n, _ in refs], "search_by_bow")


# ------------------------------------------------------------------ matchGrid
G1_CAP, G2_CAP = 198, 220  # stereo_line_case(n) has n right and int(0.9 n) left lines
COLS, ROWS = 64, 48


@pytest.fixture(scope="module")
def grid_batch():
    full, over = util.stereo_line_case(80, n=G2_CAP), util.stereo_line_case(81, n=G2_CAP)
    l1, d1, grid, d2, v2 = util.stereo_line_case(82, n=150)
    small = util.stereo_line_case(83, n=40)
    eg = bp.empty_grid(COLS, ROWS)
    cases = [full, (l1[:0], d1[:0], grid, d2, v2), over, (l1[:0], d1[:0], eg, d2[:0], v2[:0]),
             (l1, d1, eg, d2[:0], v2[:0]), small]
    assert len(full[0]) == G1_CAP
    idx_cap = max(len(bp.grid_csr(c[2])[1]) for c in cases) + 37
    pk = bp.pack_match_grid(cases, G1_CAP, G2_CAP, idx_cap)
    pk.update(cases=cases, idx_cap=idx_cap, d1n=bp.counts_array(pk["n1"], {OVER: G1_CAP + 3, NEG: -2}),
              d2n=bp.counts_array(pk["n2"], {OVER: G2_CAP + 3, NEG: -1}))
    return pk


def _match_grid_batch(plvi_lib, dev, pk, P, cap1, cap2, d1n, d2n, cols, rows, window, hint):
    out, get_m = dev.canary(P + bp.SLACK, cap1)
    cnt, get_n = dev.canary(P + bp.SLACK)
    err, get_err = dev.table(np.zeros(1, np.int32))
    (w0, w1), (h0, h1) = window
    rc = plvi_lib.plvi_line_match_grid_batch(P, dev.up(pk["lines1"]), dev.up(pk["desc1"]), dev.up(d1n), cap1, cols,
                                             rows, dev.up(pk["cell_off"]), dev.up(pk["cell_idx"]),
                                             pk["cell_idx"].shape[1], dev.up(pk["desc2"]), dev.up(pk["dirs2"]),
                                             dev.up(d2n), cap2, w0, w1, h0, h1, hint, out, cnt, err, None)
    assert rc == 0
    m, n = get_m(), get_n()
    return m, n, int(get_err()[0])


@pytest.mark.parametrize("hint", [0, 1])
def test_line_match_grid_batch_contract(plvi_lib, grid_batch, hint):
    b = grid_batch
    P = len(b["cases"])
    m, n, err = _match_grid_batch(plvi_lib, bp.Device(), b, P, G1_CAP, G2_CAP, b["d1n"], b["d2n"], COLS, ROWS,
                                  ((7, 0), (2, 2)), hint)
    refs = [ol.match_grid(*c, range_hint=hint) for c in b["cases"]]
    assert refs[FULL][0] > 30 and refs[OVER][0] > 30 and refs[SMALL][0] > 5
    bp.check_rows(m, [r for _, r in refs], "match_grid matches_12")
    bp.check_counts(n, [c for c, _ in refs], "match_grid")
    assert err == 0


# ------------------------------------------------------------------ LineMatcher::SearchByProjection
LC_CAP, LL_CAP = 200, 181
ANGTH = float(np.float32(np.pi / 8))


@pytest.fixture(scope="module")
def line_proj_batch():
    full = util.line_proj_case(90, n_cur=LC_CAP, n_last=LL_CAP)
    over = util.line_proj_case(91, n_cur=LC_CAP, n_last=LL_CAP)
    mid = util.line_proj_case(92, n_cur=120, n_last=100)
    small = util.line_proj_case(93, n_cur=30, n_last=25)
    eg = bp.empty_grid(COLS, ROWS)
    cases = [full, bp.line_proj_sub(mid, n_cur=0, grid=eg), over,
             bp.line_proj_sub(mid, n_cur=0, n_last=0, grid=eg), bp.line_proj_sub(mid, n_last=0), small]
    idx_cap = max(len(bp.grid_csr(c["grid"])[1]) for c in cases) + 37
    pk = bp.pack_line_proj(cases, LC_CAP, LL_CAP, idx_cap)
    pk.update(cases=cases, dcn=bp.counts_array(pk["n_cur"], {OVER: LC_CAP + 3, NEG: -1}),
              dln=bp.counts_array(pk["n_last"], {OVER: LL_CAP + 3, NEG: -4}))
    return pk


def _line_proj_batch(plvi_lib, dev, pk, P, params, cur_cap, last_cap, dcn, dln, blocked=True):
    out, get_m = dev.canary(P + bp.SLACK, cur_cap)
    cnt, get_n = dev.canary(P + bp.SLACK)
    err, get_err = dev.table(np.zeros(1, np.int32))
    rc = plvi_lib.plvi_line_search_projection_batch(
        P, ctypes.byref(params), dev.up(pk["cur_angle"]), dev.up(pk["cur_desc"]),
        dev.up(pk["cur_blocked"]) if blocked else None, dev.up(dcn), cur_cap, dev.up(pk["cell_off"]),
        dev.up(pk["cell_idx"]), pk["cell_idx"].shape[1], dev.up(pk["last_flags"]), dev.up(pk["x3dc"]),
        dev.up(pk["last_octave"]), dev.up(pk["ml_desc"]), dev.up(dln), last_cap, out, cnt, err, None)
    assert rc == 0
    m, n = get_m(), get_n()
    return m, n, int(get_err()[0])


def _line_params(case, th, hint, cols=COLS, rows=ROWS):
    p = util.line_proj_params(case, th, ANGTH, hint)
    p.grid_cols, p.grid_rows = cols, rows
    return p


@pytest.mark.parametrize("th,hint", [(3.0, 1), (5.0, 0)])
def test_line_search_projection_batch_contract(plvi_lib, line_proj_batch, th, hint):
    b = line_proj_batch
    P = len(b["cases"])
    m, n, err = _line_proj_batch(plvi_lib, bp.Device(), b, P, _line_params(b["cases"][0], th, hint), LC_CAP, LL_CAP,
                                 b["dcn"], b["dln"])
    refs = [ol.line_search_projection(c, th, ANGTH, hint) for c in b["cases"]]
    assert refs[FULL][0] > 30 and refs[OVER][0] > 30 and refs[SMALL][0] > 3
    bp.check_rows(m, [r for _, r in refs], "line_search_projection match")
    bp.check_counts(n, [c for c, _ in refs], "line_search_projection")
    assert err == 0


def test_line_search_projection_octave_out_of_range(plvi_lib):
    """A last-frame line whose octave is outside [0, nlevels) is skipped and reported (*d_err |= 2); every
    other line matches as if it were not there; a batch without such lines reports nothing."""
    cases = [util.line_proj_case(95, n_cur=90, n_last=80), util.line_proj_case(96, n_cur=70, n_last=75)]
    clean = [ol.line_search_projection(c, 3.0, ANGTH, 1) for c in cases]
    hit = np.unique(clean[0][1][clean[0][1] >= 0])[:2]  # two last-frame lines that do get a match
    assert len(hit) == 2
    bad = dict(cases[0])
    bad["last_octave"] = cases[0]["last_octave"].copy()
    bad["last_octave"][hit] = (-1, 2)  # nlevels = 2 (util.line_proj_params)
    without = dict(cases[0])
    without["last_flags"] = cases[0]["last_flags"].copy()
    without["last_flags"][hit] = 0
    ref = ol.line_search_projection(without, 3.0, ANGTH, 1)
    assert not np.array_equal(ref[1], clean[0][1])
    for batch, refs, want in (([bad, cases[1]], [ref, clean[1]], 2), (cases, clean, 0)):
        idx_cap = max(len(bp.grid_csr(c["grid"])[1]) for c in batch) + 5
        pk = bp.pack_line_proj(batch, 100, 90, idx_cap)
        m, n, err = _line_proj_batch(plvi_lib, bp.Device(), pk, 2, _line_params(cases[0], 3.0, 1), 100, 90,
                                     bp.counts_array(pk["n_cur"]), bp.counts_array(pk["n_last"]))
        assert err == want
        bp.check_rows(m, [r for _, r in refs], "line_search_projection match")
        bp.check_counts(n, [c for c, _ in refs], "line_search_projection")


# ------------------------------------------------------------------ the 1024-candidate limit (grid_match.hip)
LIM_COLS, LIM_ROWS = 8, 5


def _limit_grid(K):
    """K right lines spread over the 40 cells of an 8 x 5 grid, a few (K / 40) per cell."""
    grid = bp.empty_grid(LIM_COLS, LIM_ROWS)
    for i in range(K):
        grid[i % LIM_COLS][(i // LIM_COLS) % LIM_ROWS].append(i)
    return grid


def _limit_stereo_case(K, seed):
    """Every left line's two windows (window 7 / 4 on all sides) cover the whole grid, so its candidate set
    holds all K right lines and the second endpoint inserts every one of them again."""
    rng = np.random.default_rng(seed)
    n1 = 6
    desc2 = _desc(rng, K)
    ang = rng.uniform(0, 0.3, K)
    dirs = np.stack([np.cos(ang), np.sin(ang)], 1)
    lines1 = np.array([[0, 0, 7, i % 3] for i in range(n1)], np.int32)
    src = rng.choice(K, n1, replace=False)
    bits = np.unpackbits(desc2[src], axis=1)
    bits ^= (rng.random(bits.shape) < 0.05).astype(np.uint8)
    return lines1, np.packbits(bits, axis=1), _limit_grid(K), desc2, dirs


LIM_WINDOW = ((7, 7), (4, 4))


@pytest.mark.parametrize("hint", [0, 1])
def test_match_grid_candidate_limit(plvi_lib, hint):
    """Exactly 1024 distinct candidates fit (err == 0, exact); 1025 set *d_err |= 1 (PLVI_E_CAPACITY from the
    one-pair wrapper) and leave the other pair of the batch exact."""
    import plvi
    fits, small = _limit_stereo_case(1024, 1), util.stereo_line_case(84, n=40)
    # the 8 x 5 limit grid and the 64 x 48 one of `small` cannot share a launch: `small` is cut to 8 x 5
    small = (np.minimum(small[0], [7, 4, 7, 4]).astype(np.int32), small[1],
             [col[:LIM_ROWS] for col in small[2][:LIM_COLS]], small[3], small[4])
    for big, want in ((fits, 0), (_limit_stereo_case(1025, 2), 1)):
        cases = [big, small]
        pk = bp.pack_match_grid(cases, 40, 1030, 1100)
        m, n, err = _match_grid_batch(plvi_lib, bp.Device(), pk, 2, 40, 1030, bp.counts_array(pk["n1"]),
                                      bp.counts_array(pk["n2"]), LIM_COLS, LIM_ROWS, LIM_WINDOW, hint)
        assert err == want
        refs = [ol.match_grid(*c, window=LIM_WINDOW, range_hint=hint) for c in cases]
        if want:  # the overflowing pair's rows are unspecified: compare the other pair and the canaries behind it
            np.testing.assert_array_equal(m[1, :len(refs[1][1])], refs[1][1])
            assert n[1] == refs[1][0] and (m[1, len(refs[1][1]):] == bp.CANARY).all() and (m[2:] == bp.CANARY).all()
            with pytest.raises(plvi.PlviError) as e:
                plvi.LineMatcher.matchGrid(*big, window=LIM_WINDOW, range_hint=hint)
            assert e.value.code == plvi.PLVI_E_CAPACITY
        else:
            assert refs[0][0] >= 3
            bp.check_rows(m, [r for _, r in refs], "match_grid matches_12")
            bp.check_counts(n, [c for c, _ in refs], "match_grid")
            got = plvi.LineMatcher.matchGrid(*big, window=LIM_WINDOW, range_hint=hint)
            assert got[0] == refs[0][0] and np.array_equal(got[1], refs[0][1])


def _limit_line_proj_case(K, seed):
    """K current lines in the 8 x 5 grid; last-frame lines that project inside the image, whose window (th 10
    cells) covers the whole grid from both endpoints."""
    rng = np.random.default_rng(seed)
    n_last = 6
    W, H = 640.0, 480.0
    fx, fy, cx, cy = np.float32(458.654), np.float32(457.296), np.float32(320.0), np.float32(240.0)
    cur_desc = _desc(rng, K)
    x3 = np.zeros((n_last, 6), np.float32)
    for i in range(n_last):
        for e, (u, v) in enumerate(((100.0 + 20 * i, 200.0), (400.0 + 20 * i, 200.0))):  # horizontal: angle 0
            z = rng.uniform(2.0, 8.0)
            x3[i, 3 * e:3 * e + 3] = ((u - cx) * z / fx, (v - cy) * z / fy, z)
    src = rng.choice(K, n_last, replace=False)
    bits = np.unpackbits(cur_desc[src], axis=1)
    bits ^= (rng.random(bits.shape) < 0.05).astype(np.uint8)
    return {"cur_angle": rng.uniform(-0.2, 0.2, K).astype(np.float32), "cur_desc": cur_desc,
            "cur_blocked": np.zeros(K, np.uint8), "grid": _limit_grid(K),
            "last_flags": np.full(n_last, 3, np.uint8), "x3dc": x3, "last_octave": np.zeros(n_last, np.int32),
            "ml_desc": np.packbits(bits, axis=1), "scale_l": np.array([1, 2, 0, 0, 0, 0, 0, 0], np.float32),
            "camera": (fx, fy, cx, cy), "bounds": (np.float32(0), np.float32(W), np.float32(0), np.float32(H)),
            "inv_w": LIM_COLS / W, "inv_h": LIM_ROWS / H}


def _cut_line_proj_grid(case):
    """A 64 x 48 line_proj_case seen through the 8 x 5 grid geometry of the limit cases (same launch)."""
    c = dict(case)
    g = bp.empty_grid(LIM_COLS, LIM_ROWS)
    for x in range(COLS):
        for y in range(ROWS):
            cell = g[x * LIM_COLS // COLS][y * LIM_ROWS // ROWS]
            cell.extend(i for i in case["grid"][x][y] if i not in cell)
    c["grid"], c["inv_w"], c["inv_h"] = g, LIM_COLS / 640.0, LIM_ROWS / 480.0
    return c


@pytest.mark.parametrize("hint", [0, 1])
def test_line_search_projection_candidate_limit(plvi_lib, hint):
    import plvi
    small = _cut_line_proj_grid(util.line_proj_case(97, n_cur=40, n_last=30))
    th = 10.0
    for K, want in ((1024, 0), (1025, 1)):
        big = _limit_line_proj_case(K, 3 + K)
        cases = [big, small]
        pk = bp.pack_line_proj(cases, 1030, 35, 1100)
        prm = _line_params(big, th, hint, LIM_COLS, LIM_ROWS)
        m, n, err = _line_proj_batch(plvi_lib, bp.Device(), pk, 2, prm, 1030, 35, bp.counts_array(pk["n_cur"]),
                                     bp.counts_array(pk["n_last"]))
        assert err == want
        refs = [ol.line_search_projection(c, th, ANGTH, hint) for c in cases]
        args = (big["cur_angle"], big["cur_desc"], big["grid"], big["last_flags"], big["x3dc"], big["last_octave"],
                big["ml_desc"], big["cur_blocked"])
        if want:
            np.testing.assert_array_equal(m[1, :len(refs[1][1])], refs[1][1])
            assert n[1] == refs[1][0] and (m[1, len(refs[1][1]):] == bp.CANARY).all() and (m[2:] == bp.CANARY).all()
            with pytest.raises(plvi.PlviError) as e:
                plvi.LineMatcher.SearchByProjection(_line_params(big, th, hint, LIM_COLS, LIM_ROWS), *args)
            assert e.value.code == plvi.PLVI_E_CAPACITY
        else:
            assert refs[0][0] >= 3 and refs[1][0] >= 3
            bp.check_rows(m, [r for _, r in refs], "line_search_projection match")
            bp.check_counts(n, [c for c, _ in refs], "line_search_projection")
            got = plvi.LineMatcher.SearchByProjection(_line_params(big, th, hint, LIM_COLS, LIM_ROWS), *args)
            assert got[0] == refs[0][0] and np.array_equal(got[1], refs[0][1])


# ------------------------------------------------------------------ keypoint-grid matchers (proj.hip)
def _six(full, over, mid, small, a_keys, b_keys, fix=lambda c: c):
    """The six pairs of a contract batch from four generated cases: `mid` loses side A, then both sides (the
    rows of the negative-count pair), then side B."""
    return [full, fix(bp.cut(mid, a=(a_keys, 0))), over, fix(bp.cut(mid, a=(a_keys, 0), b=(b_keys, 0))),
            fix(bp.cut(mid, b=(b_keys, 0))), small]


def _blocking_matters(oracle, case, flag_key):
    """The sequential part is reached: with Observations() == 0 everywhere (bit 1 off, nothing blocks) the
    oracle assigns differently."""
    c = dict(case)
    c[flag_key] = case[flag_key] & np.uint8(~2 & 0xFF)
    return not all(np.array_equal(a, b) for a, b in zip(oracle(case)[1:], oracle(c)[1:]))


C_CAP, L_CAP = 320, 280


def _one_camera_batch(gen, seeds, last_spec, last_len_key, cur_spec=bp.CUR):
    full, over = (gen(s, C_CAP, L_CAP) for s in seeds[:2])
    mid, small = gen(seeds[2], 200, 150), gen(seeds[3], 40, 30)
    cases = _six(full, over, mid, small, list(cur_spec), list(last_spec))
    pk = {**bp.pack_keyed(cases, C_CAP, cur_spec), **bp.pack_keyed(cases, L_CAP, last_spec)}
    pk.update(cases=cases,
              dcn=bp.counts_array([len(c["cur_kps"]) for c in cases], {OVER: C_CAP + 3, NEG: -2}),
              dln=bp.counts_array([len(c[last_len_key]) for c in cases], {OVER: L_CAP + 3, NEG: -5}))
    return pk


@pytest.fixture(scope="module")
def proj_batch():
    return _one_camera_batch(lambda s, nc, nl: util.projection_case(s, n_cur=nc, n_last=nl, uright=True, dup=0.15),
                             (110, 111, 112, 113), bp.PROJ_LAST, "flags", bp.CUR_U)


def test_assign_grid_and_search_by_projection_batch_contract(plvi_lib, proj_batch):
    b, dev = proj_batch, bp.Device()
    cases = b["cases"]
    P = len(cases)
    th = 15.0
    d_kps, d_cn = dev.up(b["cur_kps"]), dev.up(b["dcn"])
    co, ci = bp.assign_grid(dev, d_kps, d_cn, C_CAP, P, cases[0]["grid"], [c["cur_kps"] for c in cases])
    prm = util.proj_params(cases[0], th)
    prm.check_orientation = 1
    out, get_m = dev.canary(P + bp.SLACK, C_CAP)
    cnt, get_n = dev.canary(P + bp.SLACK)
    rc = plvi_lib.plvi_search_by_projection_batch(
        P, ctypes.byref(prm), d_kps, dev.up(b["cur_desc"]), d_cn, C_CAP, dev.up(b["cur_blocked"]),
        dev.up(b["cur_uright"]), co, ci, dev.up(b["x3dc"]), dev.up(b["last_octave"]), dev.up(b["last_angle"]),
        dev.up(b["mp_desc"]), dev.up(b["flags"]), dev.up(b["dln"]), L_CAP, out, cnt, None)
    assert rc == 0
    refs = [ol.search_by_projection(c, th) for c in cases]
    assert refs[FULL][0] > 30 and refs[OVER][0] > 30 and refs[SMALL][0] > 3
    assert _blocking_matters(lambda c: ol.search_by_projection(c, th), cases[FULL], "flags")
    bp.check_rows(get_m(), [m for _, m in refs], "search_by_projection match")
    bp.check_counts(get_n(), [n for n, _ in refs], "search_by_projection")


@pytest.fixture(scope="module")
def reloc_batch():
    return _one_camera_batch(lambda s, nc, nl: util.reloc_case(s, n_cur=nc, n_kf=nl, dup=0.15),
                             (120, 121, 122, 123), bp.RELOC_KF, "kf_flags")


def test_search_reloc_batch_contract(plvi_lib, reloc_batch):
    b, dev = reloc_batch, bp.Device()
    cases = b["cases"]
    P = len(cases)
    d_kps, d_cn = dev.up(b["cur_kps"]), dev.up(b["dcn"])
    co, ci = bp.assign_grid(dev, d_kps, d_cn, C_CAP, P, cases[0]["grid"], [c["cur_kps"] for c in cases])
    prm = util.reloc_params(cases[0], 10.0, 100)
    prm.check_orientation = 1
    out, get_m = dev.canary(P + bp.SLACK, C_CAP)
    cnt, get_n = dev.canary(P + bp.SLACK)
    rc = plvi_lib.plvi_search_reloc_batch(
        P, ctypes.byref(prm), d_kps, dev.up(b["cur_desc"]), d_cn, C_CAP, dev.up(b["cur_blocked"]), co, ci,
        dev.up(b["kf_flags"]), dev.up(b["x3dc"]), dev.up(b["dist"]), dev.up(b["level"]), dev.up(b["kf_angle"]),
        dev.up(b["mp_desc"]), dev.up(b["dln"]), L_CAP, out, cnt, None)
    assert rc == 0
    refs = [ol.search_reloc(c, 10.0, 100) for c in cases]
    assert refs[FULL][0] > 20 and refs[OVER][0] > 20 and refs[SMALL][0] > 2
    # the sequential part is reached: a keypoint taken by an earlier KF point is closed to the later ones, so
    # walking the KF points in the opposite order assigns differently
    rev = dict(cases[FULL])
    for k in bp.RELOC_KF:
        rev[k] = cases[FULL][k][::-1].copy()
    mr = ol.search_reloc(rev, 10.0, 100)[1]
    assert not np.array_equal(np.where(mr >= 0, L_CAP - 1 - mr, mr), refs[FULL][1])
    bp.check_rows(get_m(), [m for _, m in refs], "search_reloc match")
    bp.check_counts(get_n(), [n for n, _ in refs], "search_reloc")


@pytest.fixture(scope="module")
def local_batch():
    return _one_camera_batch(lambda s, nc, nl: util.local_case(s, n_cur=nc, n_mp=nl, uright=True, dup=0.2),
                             (130, 131, 132, 133), bp.LOCAL_MP, "mp_flags", bp.CUR_U)


@pytest.mark.parametrize("th", [1.0, 3.0])
def test_search_local_batch_contract(plvi_lib, local_batch, th):
    b, dev = local_batch, bp.Device()
    cases = b["cases"]
    P = len(cases)
    d_kps, d_cn = dev.up(b["cur_kps"]), dev.up(b["dcn"])
    co, ci = bp.assign_grid(dev, d_kps, d_cn, C_CAP, P, cases[0]["grid"], [c["cur_kps"] for c in cases])
    prm = util.local_params(cases[0], th)
    prm.nnratio = 0.8
    out, get_m = dev.canary(P + bp.SLACK, C_CAP)
    cnt, get_n = dev.canary(P + bp.SLACK)
    rc = plvi_lib.plvi_search_local_batch(
        P, ctypes.byref(prm), d_kps, dev.up(b["cur_desc"]), d_cn, C_CAP, dev.up(b["cur_blocked"]),
        dev.up(b["cur_uright"]), co, ci, dev.up(b["mp_flags"]), dev.up(b["mp_proj"]), dev.up(b["mp_level"]),
        dev.up(b["mp_desc"]), dev.up(b["dln"]), L_CAP, out, cnt, None)
    assert rc == 0
    refs = [ol.search_local(c, th, 0.8) for c in cases]
    assert refs[FULL][0] > 30 and refs[OVER][0] > 30 and refs[SMALL][0] > 3
    assert _blocking_matters(lambda c: ol.search_local(c, th, 0.8), cases[FULL], "mp_flags")
    bp.check_rows(get_m(), [m for _, m in refs], "search_local match")
    bp.check_counts(get_n(), [n for n, _ in refs], "search_local")


# two-camera frames: left / right keypoint tables with their own counts and capacities
SL_CAP, SR_CAP, SM_CAP = 300, 270, 290


def _stereo_batch(gen, seeds, left, right, last, last_len_key, fix=lambda c: c):
    """Pairs: full, no left keypoints, over-count, negative counts (all three tables empty), no right
    keypoints, small."""
    full, over = (gen(s, SL_CAP, SR_CAP, SM_CAP) for s in seeds[:2])
    mid, small = gen(seeds[2], 200, 180, 150), gen(seeds[3], 50, 45, 40)
    L, R, M = list(left), list(right), list(last)
    cases = [full, fix(bp.cut(mid, a=(L, 0))), over, fix(bp.cut(mid, a=(L, 0), b=(R, 0), c=(M, 0))),
             fix(bp.cut(mid, b=(R, 0))), small]
    pk = {**bp.pack_keyed(cases, SL_CAP, left), **bp.pack_keyed(cases, SR_CAP, right),
          **bp.pack_keyed(cases, SM_CAP, last)}
    pk.update(cases=cases,
              dnl=bp.counts_array([len(c["kps"]) for c in cases], {OVER: SL_CAP + 3, NEG: -1}),
              dnr=bp.counts_array([len(c["kps_r"]) for c in cases], {OVER: SR_CAP + 3, NEG: -2}),
              dnm=bp.counts_array([len(c[last_len_key]) for c in cases], {OVER: SM_CAP + 3, NEG: -4}))
    return pk


def _stereo_grids(dev, b, P):
    cases = b["cases"]
    d_kl, d_nl, d_kr, d_nr = dev.up(b["kps"]), dev.up(b["dnl"]), dev.up(b["kps_r"]), dev.up(b["dnr"])
    col, cil = bp.assign_grid(dev, d_kl, d_nl, SL_CAP, P, cases[0]["grid"], [c["kps"] for c in cases])
    cor, cir = bp.assign_grid(dev, d_kr, d_nr, SR_CAP, P, cases[0]["grid"], [c["kps_r"] for c in cases])
    return d_kl, d_nl, d_kr, d_nr, col, cil, cor, cir


def _check_stereo(what, refs, get_l, get_r, get_n):
    assert refs[FULL][0] > 30 and refs[OVER][0] > 30 and refs[SMALL][0] > 3
    bp.check_rows(get_l(), [r[1] for r in refs], f"{what} match")
    bp.check_rows(get_r(), [r[2] for r in refs], f"{what} match_r")
    bp.check_counts(get_n(), [r[0] for r in refs], what)


@pytest.fixture(scope="module")
def proj_stereo_batch():
    return _stereo_batch(lambda s, a, r, m: util.projection_stereo_case(s, n_left=a, n_right=r, n_last=m, dup=0.15),
                         (140, 141, 142, 143), bp.LEFT, bp.RIGHT, bp.PROJ2_LAST, "flags")


def test_search_by_projection_stereo_batch_contract(plvi_lib, proj_stereo_batch):
    b, dev = proj_stereo_batch, bp.Device()
    cases = b["cases"]
    P = len(cases)
    th = 7.0
    d_kl, d_nl, d_kr, d_nr, col, cil, cor, cir = _stereo_grids(dev, b, P)
    prm = util.proj_params(cases[0], th)
    prm.check_orientation = 1
    kb = np.ascontiguousarray(cases[0]["kb8"], np.float32)
    ml, get_l = dev.canary(P + bp.SLACK, SL_CAP)
    mr, get_r = dev.canary(P + bp.SLACK, SR_CAP)
    cnt, get_n = dev.canary(P + bp.SLACK)
    rc = plvi_lib.plvi_search_by_projection_stereo_batch(
        P, ctypes.byref(prm), kb.ctypes.data_as(V), d_kl, dev.up(b["desc"]), d_nl, SL_CAP, dev.up(b["blocked"]), col,
        cil, d_kr, dev.up(b["desc_r"]), d_nr, SR_CAP, dev.up(b["blocked_r"]), cor, cir, dev.up(b["x3dc"]),
        dev.up(b["x3dr"]), dev.up(b["last_octave"]), dev.up(b["last_angle"]), dev.up(b["mp_desc"]),
        dev.up(b["flags"]), dev.up(b["dnm"]), SM_CAP, ml, mr, cnt, None)
    assert rc == 0
    refs = [ol.search_by_projection_stereo(c, th) for c in cases]
    assert _blocking_matters(lambda c: ol.search_by_projection_stereo(c, th), cases[FULL], "flags")
    _check_stereo("search_by_projection_stereo", refs, get_l, get_r, get_n)


def _unpair(c):
    """A local_stereo_case whose left or right table was emptied has no stereo partners left."""
    if not len(c["kps"]) or not len(c["kps_r"]):
        c["l2r"] = np.full(len(c["kps"]), -1, np.int32)
        c["r2l"] = np.full(len(c["kps_r"]), -1, np.int32)
    return c


@pytest.fixture(scope="module")
def local_stereo_batch():
    return _stereo_batch(lambda s, a, r, m: util.local_stereo_case(s, n_left=a, n_right=r, n_mp=m, dup=0.2),
                         (150, 151, 152, 153), bp.LOCAL2_LEFT, bp.LOCAL2_RIGHT, bp.LOCAL2_MP, "mp_flags", _unpair)


def test_search_local_stereo_batch_contract(plvi_lib, local_stereo_batch):
    b, dev = local_stereo_batch, bp.Device()
    cases = b["cases"]
    P = len(cases)
    d_kl, d_nl, d_kr, d_nr, col, cil, cor, cir = _stereo_grids(dev, b, P)
    prm = util.local_params(cases[0], 1.0)
    prm.nnratio = 0.8
    ml, get_l = dev.canary(P + bp.SLACK, SL_CAP)
    mr, get_r = dev.canary(P + bp.SLACK, SR_CAP)
    cnt, get_n = dev.canary(P + bp.SLACK)
    rc = plvi_lib.plvi_search_local_stereo_batch(
        P, ctypes.byref(prm), d_kl, dev.up(b["desc"]), d_nl, SL_CAP, dev.up(b["blocked"]), dev.up(b["l2r"]), col, cil,
        d_kr, dev.up(b["desc_r"]), d_nr, SR_CAP, dev.up(b["blocked_r"]), dev.up(b["r2l"]), cor, cir,
        dev.up(b["mp_flags"]), dev.up(b["mp_proj"]), dev.up(b["mp_level"]), dev.up(b["mp_proj_r"]),
        dev.up(b["mp_level_r"]), dev.up(b["mp_desc"]), dev.up(b["dnm"]), SM_CAP, ml, mr, cnt, None)
    assert rc == 0
    refs = [ol.search_local_stereo(c, 1.0) for c in cases]
    assert _blocking_matters(lambda c: ol.search_local_stereo(c, 1.0), cases[FULL], "mp_flags")
    _check_stereo("search_local_stereo", refs, get_l, get_r, get_n)


# ------------------------------------------------------------------ the initializer's matchers (init_match.hip)
I1_CAP, I2_CAP = 310, 280
INIT_GRID = tuple(np.float32(v) for v in (0, 0, 64 / 640, 48 / 480))  # min_x, min_y, inv_w, inv_h
INIT_K1, INIT_K2 = bp.INIT_K1, bp.INIT_K2


def _init_case(seed, n1, n2, W=640, H=480):
    """SearchForInitialization input: F2 keypoints over the image, F1 keypoints = F2 keypoints moved by a few
    pixels (20 % of them aimed at another one's target: steals), level 0 for most, descriptors with ~5 % bit
    flips, a 10-degree rotation; vbPrevMatched = the F1 positions."""
    from plvi import KEYPOINT_DTYPE
    rng = np.random.default_rng(seed)
    k2 = np.zeros(n2, KEYPOINT_DTYPE)
    k2["x"], k2["y"] = rng.uniform(0, W, n2), rng.uniform(0, H, n2)
    k2["octave"] = np.minimum(rng.geometric(0.5, n2) - 1, 7)
    k2["angle"], k2["size"], k2["class_id"] = rng.uniform(0, 360, n2), 31, -1
    d2 = _desc(rng, n2)
    src = rng.integers(0, n2, n1)
    src[-(n1 // 5):] = src[:n1 // 5]
    k1 = np.zeros(n1, KEYPOINT_DTYPE)
    k1["x"] = k2["x"][src] + rng.normal(0, 15, n1)
    k1["y"] = k2["y"][src] + rng.normal(0, 15, n1)
    k1["octave"] = rng.random(n1) < 0.15
    k1["angle"] = np.mod(k2["angle"][src] + 10 + rng.normal(0, 4, n1), 360)
    k1["size"], k1["class_id"] = 31, -1
    bits = np.unpackbits(d2[src], axis=1)
    bits ^= (rng.random(bits.shape) < 0.05).astype(np.uint8)
    return {"k1": k1, "d1": np.packbits(bits, axis=1), "prev": np.stack([k1["x"], k1["y"]], 1).astype(np.float32),
            "k2": k2, "d2": d2, "grid": (0.0, float(W), 0.0, float(H))}


@pytest.fixture(scope="module")
def init_batch():
    full, over = _init_case(160, I1_CAP, I2_CAP), _init_case(161, I1_CAP, I2_CAP)
    mid, small = _init_case(162, 200, 150), _init_case(163, 40, 30)
    cases = _six(full, over, mid, small, list(INIT_K1), list(INIT_K2))
    pk = {**bp.pack_keyed(cases, I1_CAP, INIT_K1), **bp.pack_keyed(cases, I2_CAP, INIT_K2)}
    pk.update(cases=cases, dn1=bp.counts_array([len(c["k1"]) for c in cases], {OVER: I1_CAP + 3, NEG: -2}),
              dn2=bp.counts_array([len(c["k2"]) for c in cases], {OVER: I2_CAP + 3, NEG: -3}))
    return pk


def test_search_for_initialization_batch_contract(plvi_lib, init_batch):
    """Two rounds, as Tracking carries vbPrevMatched from one frame to the next (window 100, then 40): the
    in/out table keeps its padding rows."""
    import plvi
    b, dev = init_batch, bp.Device()
    cases = b["cases"]
    P = len(cases)
    g4 = (INIT_GRID[0], None, INIT_GRID[1], None, INIT_GRID[2], INIT_GRID[3])
    d_k2, d_n2 = dev.up(b["k2"]), dev.up(b["dn2"])
    co, ci = bp.assign_grid(dev, d_k2, d_n2, I2_CAP, P, g4, [c["k2"] for c in cases])
    d_k1, d_d1, d_n1, d_d2 = dev.up(b["k1"]), dev.up(b["d1"]), dev.up(b["dn1"]), dev.up(b["d2"])
    d_pv, get_pv = dev.table(b["prev"])
    prm = plvi.InitParams(*[float(g) for g in INIT_GRID], 100, 0.9, 1)
    prev = [c["prev"] for c in cases]
    for it, win in enumerate((100, 40)):
        prm.window = win
        out, get_m = dev.canary(P + bp.SLACK, I1_CAP)
        cnt, get_n = dev.canary(P + bp.SLACK)
        plvi.search_for_initialization_batch(P, prm, d_k1.value, d_d1.value, d_n1.value, I1_CAP, d_pv.value, d_k2.value,
                                             d_d2.value, d_n2.value, I2_CAP, co.value, ci.value, out.value, cnt.value)
        refs = [ol.search_for_initialization(c["k1"], c["d1"], prev[p], c["k2"], c["d2"], INIT_GRID, window=win)
                for p, c in enumerate(cases)]
        if it == 0:
            assert refs[FULL][0] > 30 and refs[OVER][0] > 30 and refs[SMALL][0] > 3
        bp.check_rows(get_m(), [m for _, m, _ in refs], "search_for_initialization vnMatches12")
        bp.check_counts(get_n(), [n for n, _, _ in refs], "search_for_initialization")
        got_pv = get_pv()
        for p, (_, _, epv) in enumerate(refs):
            np.testing.assert_array_equal(got_pv[p, :len(epv)], epv, err_msg=f"vbPrevMatched of pair {p}")
            np.testing.assert_array_equal(got_pv[p, len(epv):], b["prev"][p, len(epv):],
                                          err_msg=f"vbPrevMatched padding of pair {p}")
        np.testing.assert_array_equal(got_pv[P:], b["prev"][P:])
        prev = [epv for _, _, epv in refs]


def test_line_search_init_batch_contract(plvi_lib, knn_batch):
    """LineMatcher::SerachForInitialize on the kNN-2 contract batch (same descriptor tables and counts)."""
    import plvi
    b, dev = knn_batch, bp.Device()
    P = len(b["cases"])
    scratch = dev.up(np.zeros(4 * (P + bp.SLACK) * Q_CAP, np.int32))
    pairs, get_p = dev.canary(P + bp.SLACK, Q_CAP, 2)
    cnt, get_n = dev.canary(P + bp.SLACK)
    mad, get_mad = dev.canary(P + bp.SLACK, 4)
    plvi.line_search_init_batch(dev.up(b["q"]).value, dev.up(b["dq"]).value, Q_CAP, dev.up(b["t"]).value,
                                dev.up(b["dt"]).value, T_CAP, P, scratch.value, pairs.value, cnt.value, mad.value)
    refs = [ol.line_search_init(q, t) for q, t in b["cases"]]
    assert len(refs[FULL][0]) > 30 and len(refs[OVER][0]) > 30
    bp.check_rows(get_p(), [r for r, _ in refs], "line_search_init pairs")
    bp.check_counts(get_n(), [len(r) for r, _ in refs], "line_search_init")
    gm = get_mad()
    for p, ((q, t), (_, emad)) in enumerate(zip(b["cases"], refs)):
        if len(q) and len(t) >= 2:
            assert tuple(gm[p].view(np.float64)) == emad, f"pair {p}"
    assert (gm[P:] == bp.CANARY).all()


# ------------------------------------------------------------------ Frame::ComputeStereoMatches_Lines (stereo.hip)
STEREO_L, STEREO_R = bp.STEREO_L, bp.STEREO_R
MBF = 47.9


@pytest.fixture(scope="module")
def stereo_lines_batch():
    from plvi import synth
    ext = []
    for seed in (11, 12):
        L, R, _ = synth.stereo_pair(seed)
        (kl, dl, _), (kr, dr, _) = ol.line_extract(L), ol.line_extract(R)
        ext.append({"klL": kl, "dL": dl, "klR": kr, "dR": dr})
    cap_l = min(len(c["klL"]) for c in ext)
    cap_r = min(len(c["klR"]) for c in ext) - 10  # unequal capacities
    full, over = (bp.cut(c, a=(list(STEREO_L), cap_l), b=(list(STEREO_R), cap_r)) for c in ext)
    mid = bp.cut(ext[0], a=(list(STEREO_L), 60), b=(list(STEREO_R), 70))
    small = bp.cut(ext[1], a=(list(STEREO_L), 25), b=(list(STEREO_R), 30))
    cases = _six(full, over, mid, small, list(STEREO_L), list(STEREO_R))
    pk = {**bp.pack_keyed(cases, cap_l, STEREO_L), **bp.pack_keyed(cases, cap_r, STEREO_R)}
    pk.update(cases=cases, cap_l=cap_l, cap_r=cap_r,
              dnl=bp.counts_array([len(c["klL"]) for c in cases], {OVER: cap_l + 3, NEG: -2}),
              dnr=bp.counts_array([len(c["klR"]) for c in cases], {OVER: cap_r + 3, NEG: -1}))
    return pk


@pytest.mark.parametrize("hint", [0, 1])
def test_stereo_lines_batch_contract(plvi_lib, stereo_lines_batch, hint):
    """The three stereo.hip kernels behind plvi_stereo_lines_batch read the caller's counts too.  Floats and
    doubles are compared bit for bit through their int32 words, so the canary words stay visible."""
    import plvi
    b, dev = stereo_lines_batch, bp.Device()
    cases, cl, cr = b["cases"], b["cap_l"], b["cap_r"]
    P = len(cases)
    idx_cap = 32768
    sb = plvi.stereo_lines_scratch_bytes(P, cl, cr, idx_cap)
    scratch = dev.up(np.zeros(sb, np.uint8))
    m12, get_m = dev.canary(P + bp.SLACK, cl)
    disp, get_d = dev.canary(P + bp.SLACK, cl, 2)
    dep, get_z = dev.canary(P + bp.SLACK, cl, 2)
    le, get_le = dev.canary(P + bp.SLACK, cl, 6)
    ns, get_n = dev.canary(P + bp.SLACK)
    err, get_err = dev.table(np.zeros(1, np.int32))
    plvi.stereo_lines_batch(P, dev.up(b["klL"]).value, dev.up(b["dL"]).value, dev.up(b["dnl"]).value, cl,
                            dev.up(b["klR"]).value, dev.up(b["dR"]).value, dev.up(b["dnr"]).value, cr, None, 640, 480,
                            MBF, hint, idx_cap, scratch.value, sb, m12.value, disp.value, dep.value, le.value,
                            ns.value, err.value)
    refs = [ol.stereo_lines(c["klL"], c["dL"], c["klR"], c["dR"], None, 640, 480, MBF, range_hint=hint)
            for c in cases]
    assert refs[FULL][0] > 10 and refs[OVER][0] > 10

    def words(a):  # [n][k] float32 / float64 as [n][int32 words per row]
        return np.ascontiguousarray(a).view(np.int32).reshape(len(a), a.shape[1] * a.itemsize // 4)
    bp.check_rows(get_m(), [r[1] for r in refs], "stereo_lines matches_12")
    bp.check_rows(get_d(), [words(r[2]) for r in refs], "stereo_lines disparity")
    bp.check_rows(get_z(), [words(r[3]) for r in refs], "stereo_lines depth")
    bp.check_rows(get_le(), [words(r[4]) for r in refs], "stereo_lines le")
    bp.check_counts(get_n(), [r[0] for r in refs], "stereo_lines")
    assert get_err()[0] == 0
