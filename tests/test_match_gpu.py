"""Hamming matchers: HIP kNN-2 / LineMatcher vs the CPU oracle (BFMatcher
tie rules), including planted ties and duplicate rows."""
import numpy as np
import pytest

import batch_pack as bp
import oracle_lib as ol
import plvi
from util import near_duplicate_descriptors

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nq,nt", [(1, 2), (7, 5), (200, 200), (1000, 1000), (300, 1500)])
def test_knn2_matches_oracle(plvi_lib, nq, nt):
    rng = np.random.default_rng(nq * 7 + nt)
    q, t = near_duplicate_descriptors(rng, nt, nq)
    got = plvi.hamming_knn2(q, t)
    exp = ol.knn2(q, t)
    for g, e, name in zip(got, exp, ["idx0", "d0", "idx1", "d1"]):
        assert np.array_equal(g, e), name


def test_knn2_ties_keep_lower_index(plvi_lib):
    rng = np.random.default_rng(5)
    t = rng.integers(0, 256, size=(64, 32), dtype=np.uint8)
    t[10] = t[3]; t[40] = t[3]; t[41] = t[7]
    q = t[[3, 7, 10, 41]].copy()
    got = plvi.hamming_knn2(q, t)
    exp = ol.knn2(q, t)
    for g, e in zip(got, exp):
        assert np.array_equal(g, e)
    assert got[0][0] == 3 and got[2][0] == 10 and got[1][0] == 0 and got[3][0] == 0


def test_line_match_nnr_and_mutual(plvi_lib):
    rng = np.random.default_rng(9)
    q, t = near_duplicate_descriptors(rng, 180, 200, p_flip=0.05)
    for nnr in (0.9, 0.75):
        assert plvi.LineMatcher.matchNNR(q, t, nnr)[0] == ol.match_nnr(q, t, nnr)[0]
        assert np.array_equal(plvi.LineMatcher.matchNNR(q, t, nnr)[1], ol.match_nnr(q, t, nnr)[1])
        n, m = plvi.LineMatcher.match(q, t, nnr)
        ne, me = ol.match(q, t, nnr)
        assert n == ne and np.array_equal(m, me)


def test_line_match_batch_device(plvi_lib):
    """Poisoned padding rows and canary-filled outputs (tests/batch_pack.py): nothing past a count is read
    or written."""
    rng = np.random.default_rng(21)
    P, cap = 5, 64
    n1 = np.array([64, 10, 2, 1, 40], np.int32)
    n2 = np.array([60, 12, 5, 30, 0], np.int32)
    cases = []
    for p in range(P):
        q, t = near_duplicate_descriptors(rng, max(n2[p], 1), max(n1[p], 1), p_flip=0.05)
        cases.append((q[:n1[p]], t[:n2[p]]))
    pk, dev = bp.pack_knn(cases, cap, cap), bp.Device()
    scratch = dev.up(np.zeros(4 * (P + bp.SLACK) * 2 * cap, np.int32))
    m12, get_m = dev.canary(P + bp.SLACK, cap)
    nm, get_n = dev.canary(P + bp.SLACK)
    rc = plvi.load().plvi_line_match_batch(dev.up(pk["q"]), dev.up(bp.counts_array(n1)), cap, dev.up(pk["t"]),
                                           dev.up(bp.counts_array(n2)), cap, P, 0.9, scratch, m12, nm, None)
    assert rc == 0
    refs, cnts = [], []
    for p, (q, t) in enumerate(cases):
        if n1[p] >= 2 and n2[p] >= 2:
            ne, me = ol.match(q, t, 0.9)
        else:
            ne, me = 0, np.full(n1[p], -1, np.int32)
        refs.append(me)
        cnts.append(ne)
    bp.check_rows(get_m(), refs, "line_match matches_12")
    bp.check_counts(get_n(), cnts, "line_match")


@pytest.mark.parametrize("nq,nt", [(0, 5), (4, 0), (6, 1)])
def test_knn2_degenerate_sizes(plvi_lib, nq, nt):
    # knnMatch with fewer than 2 train rows leaves the missing neighbours at
    # (-1, INT_MAX) in the oracle's BFMatcher restatement; nq == 0 is a no-op
    rng = np.random.default_rng(100 + nq * 3 + nt)
    q = rng.integers(0, 256, size=(nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, size=(nt, 32), dtype=np.uint8)
    got = plvi.hamming_knn2(q, t)
    exp = ol.knn2(q, t)
    for g, e, name in zip(got, exp, ["idx0", "d0", "idx1", "d1"]):
        assert g.shape == (nq,) and np.array_equal(g, e), name


def test_knn2_all_equal_targets_and_max_distance(plvi_lib):
    # every train row identical: all distances tie, first two indices win;
    # query = bitwise complement of the train rows: distance 256 everywhere
    rng = np.random.default_rng(77)
    row = rng.integers(0, 256, size=32, dtype=np.uint8)
    t = np.tile(row, (300, 1))
    q = np.stack([row, ~row, row ^ 1])  # row ^ 1 flips one bit per byte
    got = plvi.hamming_knn2(q, t)
    exp = ol.knn2(q, t)
    for g, e in zip(got, exp):
        assert np.array_equal(g, e)
    assert list(got[0]) == [0, 0, 0] and list(got[2]) == [1, 1, 1]
    assert list(got[1]) == [0, 256, 32] and list(got[3]) == [0, 256, 32]


def test_line_match_nnr_rejects_single_train_row(plvi_lib):
    # LineMatcher::matchNNR reads matches_[idx][1] (LineMatcher.cpp:41-61),
    # undefined with one train row: the C-ABI refuses instead of guessing
    rng = np.random.default_rng(3)
    q = rng.integers(0, 256, size=(4, 32), dtype=np.uint8)
    t = rng.integers(0, 256, size=(1, 32), dtype=np.uint8)
    with pytest.raises(plvi.PlviError):
        plvi.LineMatcher.matchNNR(q, t, 0.9)
