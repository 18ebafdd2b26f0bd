"""The matrix-core Hamming matchers (csrc/match.hip: kNN-2 from int8 MFMA distance tiles, LineMatcher::match
as one launch), bit-exact against the oracle: the edges of the 16 x 16 tiles, of the 64 queries a wave keeps
and of the 256-row train chunks; BFMatcher's tie rule with the tied rows in one tile, in two tiles at the
same lane position and in two lane groups; distances 0 and 256; the VALU kernel and the three-launch line
matcher behind PLVI_MATCH_MFMA=0 giving the same tables; and a HIP-graph replay of both entry points.
Tables come from tests/batch_pack.py (poisoned padding rows, canary-filled outputs, a slack pair)."""
import ctypes

import numpy as np
import pytest

import batch_pack as bp
import oracle_lib as ol
import plvi
import util

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1
NAMES = ["idx0", "d0", "idx1", "d1"]
EDGES = [(1, 1), (1, 2), (2, 1), (15, 17), (16, 16), (17, 15), (31, 33), (64, 64), (65, 63), (100, 129), (255, 257)]


def _desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _run_knn(lib, cases, q_cap, t_cap, over_q=None, over_t=None):
    """One packed batch through plvi_hamming_knn2_batch, checked against the oracle row by row."""
    pk, dev = bp.pack_knn(cases, q_cap, t_cap), bp.Device()
    P = len(cases)
    outs = [dev.canary(P + bp.SLACK, q_cap) for _ in range(4)]
    rc = lib.plvi_hamming_knn2_batch(dev.up(pk["q"]), dev.up(bp.counts_array(pk["nq"], over_q)), q_cap,
                                     dev.up(pk["t"]), dev.up(bp.counts_array(pk["nt"], over_t)), t_cap, P,
                                     *[o[0] for o in outs], None)
    assert rc == 0
    refs = [ol.knn2(q, t) for q, t in cases]
    got = [o[1]() for o in outs]
    for k, name in enumerate(NAMES):
        bp.check_rows(got[k], [r[k] for r in refs], f"knn2 {name}")
    return got


@pytest.fixture(scope="module")
def edge_cases():
    rng = np.random.default_rng(1401)
    cases = [util.near_duplicate_descriptors(rng, nt, nq, p_flip=0.05) for nq, nt in EDGES]
    none = _desc(rng, 0)
    full = util.near_duplicate_descriptors(rng, 260, 260, p_flip=0.05)
    mid = util.near_duplicate_descriptors(rng, 40, 50, p_flip=0.05)
    # counts of 0 on either side, an over-count pair (read as the capacity) and a negative pair right behind it
    cases += [(none, mid[1]), (mid[0], none), full, (none, none)]
    return cases


def _edge_overrides(cases):
    P = len(cases)
    return {P - 2: 263, P - 1: -2}, {P - 2: 263, P - 1: -5}


def test_knn2_tile_edges(plvi_lib, edge_cases):
    oq, ot = _edge_overrides(edge_cases)
    _run_knn(plvi_lib, edge_cases, 260, 260, oq, ot)


def test_knn2_missing_neighbours(plvi_lib):
    """Fewer than two train rows: the missing neighbours are (-1, INT_MAX)."""
    rng = np.random.default_rng(1402)
    got = _run_knn(plvi_lib, [(_desc(rng, 20), _desc(rng, 1)), (_desc(rng, 20), _desc(rng, 0))], 20, 16)
    assert (got[2][0] == -1).all() and (got[3][0] == INT_MAX).all() and (got[0][0] == 0).all()
    assert (got[0][1] == -1).all() and (got[1][1] == INT_MAX).all()


@pytest.mark.parametrize("rows", [(3, 10), (3, 19), (3, 7), (3, 19, 35, 39)])
def test_knn2_ties_by_position(plvi_lib, rows):
    """A query equal to several train rows: in one tile (3, 10), in two tiles at the same lane position
    (3, 19), in two lane groups of one tile (3, 7), and four copies: the two lowest indices at distance 0."""
    rng = np.random.default_rng(1403 + sum(rows))
    t = _desc(rng, 64)
    for r in rows[1:]:
        t[r] = t[rows[0]]
    q = np.concatenate([t[[rows[0]]], _desc(rng, 5)])
    got = plvi.hamming_knn2(q, t)
    for g, e, name in zip(got, ol.knn2(q, t), NAMES):
        assert np.array_equal(g, e), name
    assert (got[0][0], got[1][0], got[2][0], got[3][0]) == (rows[0], 0, rows[1], 0)


def test_knn2_identical_rows_and_extreme_distances(plvi_lib):
    """300 identical train rows: indices (0, 1) for every query; the row itself is at distance 0 (dot = +256
    in the +-1 picture), its complement at 256 (dot = -256)."""
    rng = np.random.default_rng(1404)
    row = _desc(rng, 1)[0]
    t = np.tile(row, (300, 1))
    q = np.stack([row, ~row, row ^ 1, np.zeros(32, np.uint8), np.full(32, 255, np.uint8)])
    got = plvi.hamming_knn2(q, t)
    for g, e, name in zip(got, ol.knn2(q, t), NAMES):
        assert np.array_equal(g, e), name
    assert got[0].tolist() == [0] * 5 and got[2].tolist() == [1] * 5
    assert got[1][:3].tolist() == [0, 256, 32] and got[3][:3].tolist() == [0, 256, 32]
    # all-zero against all-one rows: every one of the 256 products has the same sign
    z, o = np.zeros((3, 32), np.uint8), np.full((3, 32), 255, np.uint8)
    assert plvi.hamming_knn2(z, o)[1].tolist() == [256] * 3 and plvi.hamming_knn2(o, o)[1].tolist() == [0] * 3


@pytest.fixture(scope="module")
def large_cases():
    rng = np.random.default_rng(1405)
    return {(nq, nt): util.near_duplicate_descriptors(rng, nt, nq) for nq, nt in [(1000, 1000), (300, 1500)]}


@pytest.mark.parametrize("nq,nt", [(1000, 1000), (300, 1500)])
def test_knn2_large(plvi_lib, large_cases, nq, nt):
    _run_knn(plvi_lib, [large_cases[nq, nt]], nq, nt)


def test_knn2_forced_fallback_identical(plvi_lib, edge_cases, large_cases, monkeypatch):
    """PLVI_MATCH_MFMA=0 sends the same calls to the VALU kernel: the same tables, word for word."""
    oq, ot = _edge_overrides(edge_cases)
    head = _run_knn(plvi_lib, edge_cases, 260, 260, oq, ot)
    head_l = _run_knn(plvi_lib, [large_cases[300, 1500]], 300, 1500)
    monkeypatch.setenv("PLVI_MATCH_MFMA", "0")
    base = _run_knn(plvi_lib, edge_cases, 260, 260, oq, ot)
    base_l = _run_knn(plvi_lib, [large_cases[300, 1500]], 300, 1500)
    for a, b in zip(head + head_l, base + base_l):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------ LineMatcher::match, one launch
LINE_SIZES = [(64, 60), (10, 12), (2, 5), (1, 30), (40, 0), (0, 7), (2, 2), (1, 1), (17, 33), (200, 200)]


@pytest.fixture(scope="module")
def line_cases():
    rng = np.random.default_rng(1406)
    out = []
    for n1, n2 in LINE_SIZES:
        q, t = util.near_duplicate_descriptors(rng, max(n2, 1), max(n1, 1), p_flip=0.05)
        out.append((q[:n1], t[:n2]))
    return out


def _run_line(lib, cases, cap, nnr):
    pk, dev = bp.pack_knn(cases, cap, cap), bp.Device()
    P = len(cases)
    scratch = dev.up(np.zeros(4 * (P + bp.SLACK) * 2 * cap, np.int32))
    m12, get_m = dev.canary(P + bp.SLACK, cap)
    nm, get_n = dev.canary(P + bp.SLACK)
    rc = lib.plvi_line_match_batch(dev.up(pk["q"]), dev.up(bp.counts_array(pk["nq"])), cap, dev.up(pk["t"]),
                                   dev.up(bp.counts_array(pk["nt"])), cap, P, nnr, scratch, m12, nm, None)
    assert rc == 0
    return get_m(), get_n()


@pytest.mark.parametrize("cap", [64, 200])
@pytest.mark.parametrize("nnr", [0.9, 0.75])
def test_line_match_one_launch(plvi_lib, line_cases, monkeypatch, cap, nnr):
    """Against the oracle, and against the three-launch path (PLVI_MATCH_MFMA=0): the same matches_12 rows
    and counts, canaries intact in both."""
    cases = [c for c in line_cases if len(c[0]) <= cap and len(c[1]) <= cap]
    assert len(cases) == (9 if cap == 64 else 10)
    refs, cnts = [], []
    for q, t in cases:
        if len(q) >= 2 and len(t) >= 2:
            n, m = ol.match(q, t, nnr)
        else:
            n, m = 0, np.full(len(q), -1, np.int32)
        refs.append(m)
        cnts.append(n)
    assert sum(cnts) > 20
    m_head, n_head = _run_line(plvi_lib, cases, cap, nnr)
    bp.check_rows(m_head, refs, "line_match matches_12")
    bp.check_counts(n_head, cnts, "line_match")
    monkeypatch.setenv("PLVI_MATCH_MFMA", "0")
    m_base, n_base = _run_line(plvi_lib, cases, cap, nnr)
    assert np.array_equal(m_head, m_base) and np.array_equal(n_head, n_base)


def test_line_match_large_capacity_takes_three_launches(plvi_lib, line_cases):
    """Above 1024 rows of capacity on a side the call keeps the three-launch path: same answer."""
    cases = line_cases[:3]
    cap = 1100
    refs = [ol.match(q, t, 0.9) for q, t in cases]
    m, n = _run_line(plvi_lib, cases, cap, 0.9)
    bp.check_rows(m, [r[1] for r in refs], "line_match matches_12")
    bp.check_counts(n, [r[0] for r in refs], "line_match")


# ------------------------------------------------------------------ HIP graph
def test_matchers_hip_graph_replay(plvi_lib):
    """plvi_hamming_knn2_batch and plvi_line_match_batch at batch 3 captured into a HIP graph on one stream and
    replayed twice: the tables of the direct calls (no allocation, no synchronisation inside)."""
    import torch
    rng = np.random.default_rng(1407)
    P, cap = 3, 70
    cases = [util.near_duplicate_descriptors(rng, nt, nq, p_flip=0.05) for nq, nt in [(70, 65), (33, 70), (17, 2)]]
    pk = bp.pack_knn(cases, cap, cap)
    dev = "cuda:0"
    q = torch.from_numpy(pk["q"]).to(dev)
    t = torch.from_numpy(pk["t"]).to(dev)
    nq = torch.from_numpy(bp.counts_array(pk["nq"])).to(dev)
    nt = torch.from_numpy(bp.counts_array(pk["nt"])).to(dev)
    outs = [torch.full(((P + bp.SLACK) * cap,), bp.CANARY, dtype=torch.int32, device=dev) for _ in range(5)]
    nm = torch.full((P + bp.SLACK,), bp.CANARY, dtype=torch.int32, device=dev)
    scratch = torch.zeros(4 * (P + bp.SLACK) * 2 * cap, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    V = ctypes.c_void_p

    def step(st):
        assert plvi_lib.plvi_hamming_knn2_batch(V(q.data_ptr()), V(nq.data_ptr()), cap, V(t.data_ptr()),
                                                V(nt.data_ptr()), cap, P, *[V(o.data_ptr()) for o in outs[:4]],
                                                V(st)) == 0
        assert plvi_lib.plvi_line_match_batch(V(q.data_ptr()), V(nq.data_ptr()), cap, V(t.data_ptr()),
                                              V(nt.data_ptr()), cap, P, 0.9, V(scratch.data_ptr()),
                                              V(outs[4].data_ptr()), V(nm.data_ptr()), V(st)) == 0

    step(s.cuda_stream)
    torch.cuda.synchronize()
    ref = [o.cpu().numpy().copy() for o in outs + [nm]]
    refs = [ol.knn2(a, b) for a, b in cases]
    for k, name in enumerate(NAMES):
        bp.check_rows(ref[k].reshape(P + bp.SLACK, cap), [r[k] for r in refs], f"knn2 {name}")
    lrefs = [ol.match(a, b, 0.9) for a, b in cases]
    bp.check_rows(ref[4].reshape(P + bp.SLACK, cap), [r[1] for r in lrefs], "line_match matches_12")
    bp.check_counts(ref[5], [r[0] for r in lrefs], "line_match")
    for o in outs + [nm]:
        o.fill_(bp.CANARY)
    g = plvi.StepGraph(step, s.cuda_stream)
    g.launch()
    g.launch()
    torch.cuda.synchronize()
    for a, o in zip(ref, outs + [nm]):
        np.testing.assert_array_equal(a, o.cpu().numpy())
