"""MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:330-404) and MapLine::ComputeDistinctiveDescriptors
(src/MapLine.cc:264-331) on the device (csrc/distinctive.hip): plvi_distinctive_descriptors[_batch].

Expected values come from tests/native/distinctive_ref.cpp, a sequential host restatement in the reference's own
shape (float Distances on the heap, std::sort on a vector<int>, the index 0.5*(N-1), a strict < from INT_MAX).  The
CPU part checks the restatement against an independent numpy restatement (np.unpackbits Hamming, np.sort, argmin)
on a seeded general case that must hold at least 50 features whose least median is attained at two or more rows
and at least 50 whose answer is not row 0, and pins what every crafted list claims about itself.  The gpu part
demands exact equality of best_pos, best_median and out_desc (rows with best_pos = -1 keep the sentinel they were
pre-filled with).  There is no float on this path, so nothing is compared within a tolerance."""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import plvi

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "distinctive_ref.cpp"
BUILD = ROOT / "tests" / "native" / "_build"
LIMIT = plvi.DISTINCTIVE_MAX_OBS
SMALL = 64  # the longest list of the wave-segment path; 65 entries take the LDS path
SENTINEL = 0xA5
E_BADARG, E_CAPACITY = -2, -3

_lib = None
_cache = {}


def ref_lib():
    global _lib
    if _lib is None:
        so = BUILD / "libdistinctive_ref.so"
        if not so.exists() or so.stat().st_mtime < SRC.stat().st_mtime:
            so.parent.mkdir(parents=True, exist_ok=True)
            subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", str(so),
                            str(SRC)], check=True)
        _lib = ctypes.CDLL(str(so))
        V, I = ctypes.c_void_p, ctypes.c_int
        _lib.distinctive_ref.argtypes = [I, V, I, V, V, I, V, V, V]
        _lib.distinctive_ref.restype = I
    return _lib


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def as_case(pool, lists):
    """(pool, obs_off, obs_row) of a list of per-feature row lists."""
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    rows = np.array([r for l in lists for r in l], np.int32)
    return np.ascontiguousarray(pool, np.uint8).reshape(-1, 32), off, rows


def ref(pool, off, rows, max_obs=None, n_feat=None):
    """(count, best_pos, best_median, out_desc) of the restatement; out_desc pre-filled with the sentinel."""
    n_feat = len(off) - 1 if n_feat is None else n_feat
    if max_obs is None:
        max_obs = int(np.max(np.diff(off), initial=0))
    bp, bm = np.full(max(n_feat, 1), -7, np.int32), np.full(max(n_feat, 1), -7, np.int32)
    out = np.full((n_feat, 32), SENTINEL, np.uint8)
    rows = np.ascontiguousarray(rows, np.int32)
    n = ref_lib().distinctive_ref(n_feat, _p(pool), len(pool), _p(off), _p(rows), max_obs, _p(bp), _p(bm), _p(out))
    return n, bp[:n_feat], bm[:n_feat], out


def medians(desc):
    """Per row the element floor((N-1)/2) of its sorted Hamming distances (self included): numpy only."""
    bits = np.unpackbits(np.asarray(desc, np.uint8).reshape(-1, 32), axis=1).astype(np.int32)
    dist = bits @ (1 - bits.T) + (1 - bits) @ bits.T
    return np.sort(dist, axis=1)[:, (len(bits) - 1) // 2]


def np_ref(pool, off, rows, max_obs=None):
    """The independent restatement: (best_pos, best_median, number of rows attaining the least median)."""
    n_feat = len(off) - 1
    bp, bm, ties = (np.full(n_feat, -1, np.int32) for _ in range(3))
    for f in range(n_feat):
        ln = max(int(off[f + 1]) - int(off[f]), 0)
        lst = np.asarray(rows[off[f]:off[f] + (ln if max_obs is None else min(ln, max_obs))])
        pos = np.flatnonzero((lst >= 0) & (lst < len(pool)))
        if len(pos):
            med = medians(pool[lst[pos]])
            i = int(np.argmin(med))  # the first minimum
            bp[f], bm[f], ties[f] = pos[i], med[i], int((med == med[i]).sum())
    return bp, bm, ties


def seeded(seed, counts, flip=0.12):
    """Per feature a base descriptor and `count` rows with every bit of it flipped with probability `flip`;
    the pool is the rows of all features, shuffled, so every list is out of order in the pool."""
    rng = np.random.default_rng(seed)
    total = int(np.sum(counts))
    bits = np.empty((total, 256), np.uint8)
    o = 0
    for c in counts:
        base = rng.integers(0, 2, 256, dtype=np.uint8)
        bits[o:o + c] = base ^ (rng.random((c, 256)) < flip)
        o += c
    perm = rng.permutation(total)
    pool = np.empty((total, 32), np.uint8)
    pool[perm] = np.packbits(bits, axis=1)
    off = np.zeros(len(counts) + 1, np.int32)
    off[1:] = np.cumsum(counts)
    return pool, off, perm.astype(np.int32)


def general():
    if "general" not in _cache:
        counts = np.random.default_rng(12).integers(1, 41, 400)
        _cache["general"] = seeded(12, counts)
    return _cache["general"]


def weights_rows(weights):
    """Rows with disjoint bit sets of the given sizes: the distance of two rows is the sum of their weights."""
    assert sum(weights) <= 256
    bits = np.zeros((len(weights), 256), np.uint8)
    o = 0
    for i, w in enumerate(weights):
        bits[i, o:o + w] = 1
        o += w
    return np.packbits(bits, axis=1)


def tie_5_9():
    """12 rows: rows 5 and 9 (all zero) share the least median, row 2 (one bit) is one worse."""
    w = [20, 21, 1, 22, 23, 0, 24, 25, 26, 0, 27, 28]
    return weights_rows(w)


def tie_two(n, a, b):
    """n rows: rows a and b (all zero) share the least median 3; every other row has three bits of its own."""
    return weights_rows([0 if i in (a, b) else 3 for i in range(n)])


def complement_mix(n_a, n_b, seed=3):
    a = np.random.default_rng(seed).integers(0, 256, 32, dtype=np.uint8)
    return np.stack([a] * n_a + [~a] * n_b)


# ====================================================================== CPU
def test_restatement_equals_numpy_on_the_seeded_general_case():
    pool, off, rows = general()
    n, bp, bm, out = ref(pool, off, rows)
    ebp, ebm, ties = np_ref(pool, off, rows)
    assert n == 400 and np.array_equal(bp, ebp) and np.array_equal(bm, ebm)
    assert np.array_equal(out, pool[rows[off[:-1] + bp]])
    # the case must be able to tell a wrong tie rule from the right one
    assert int((ties >= 2).sum()) >= 50, int((ties >= 2).sum())
    assert int((bp != 0).sum()) >= 50, int((bp != 0).sum())
    counts = np.diff(off)
    assert counts.min() == 1 and counts.max() == 40


def test_restatement_list_conventions():
    """Ignored rows are counted in best_pos, the clamp to max_obs, a decreasing offset, an empty list."""
    pool, off, rows = seeded(5, [9, 7, 30])
    lst = list(rows[:9])
    mixed = [-1, lst[0], len(pool), lst[1], lst[2], -5, lst[3], lst[4], lst[5], lst[6], lst[7], lst[8], 1 << 30]
    p, o, r = as_case(pool, [mixed, [], [-1, len(pool)], list(rows[9:16])])
    n, bp, bm, out = ref(p, o, r)
    ebp, ebm, _ = np_ref(p, o, r)
    assert n == 2 and np.array_equal(bp, ebp) and np.array_equal(bm, ebm)
    n0, bp0, bm0, _ = ref(pool, off, rows)
    keep = np.array([1, 3, 4, 6, 7, 8, 9, 10, 11])
    assert bp[0] == keep[bp0[0]] and bm[0] == bm0[0]
    assert bp[1] == bp[2] == -1 and bm[1] == bm[2] == -1 and (out[1:3] == SENTINEL).all()
    assert np.array_equal(out[0], pool[mixed[bp[0]]])
    # max_obs: the third list reads as its first 11 entries
    n, bp, bm, _ = ref(pool, off, rows, max_obs=11)
    ebp, ebm, _ = np_ref(pool, off, rows, max_obs=11)
    assert np.array_equal(bp, ebp) and np.array_equal(bm, ebm) and bp.max() < 11
    # a decreasing offset reads as an empty list
    o2 = np.array([0, 9, 4, 16], np.int32)
    n, bp, bm, _ = ref(pool, o2, rows)
    assert n == 2 and bp[1] == -1 and bp[2] >= 0


def test_crafted_lists_are_what_they_claim():
    m = medians(tie_5_9())
    assert m[5] == m[9] == m.min() and m[2] == m.min() + 1 and (np.delete(m, [2, 5, 9]) > m[2]).all()
    p, o, r = as_case(tie_5_9(), [range(12)])
    assert ref(p, o, r)[1][0] == 5
    p, o, r = as_case(tie_5_9(), [range(11, -1, -1)])
    assert ref(p, o, r)[1][0] == 2  # row 9 comes first in the reversed list
    for n, a, b in ((80, 10, 70), (60, 10, 50)):
        m = medians(tie_two(n, a, b))
        assert m[a] == m[b] == 3 and (np.delete(m, [a, b]) == 6).all()
        p, o, r = as_case(tie_two(n, a, b), [range(n)])
        assert ref(p, o, r)[1][0] == a
    a = complement_mix(1, 1)
    assert medians(a).tolist() == [0, 0] and np.unpackbits(a[0] ^ a[1]).sum() == 256
    assert medians(complement_mix(2, 1)).tolist() == [0, 0, 256]
    assert medians(complement_mix(3, 4)).tolist() == [256] * 3 + [0] * 4
    assert medians(complement_mix(39, 41)).tolist() == [256] * 39 + [0] * 41
    # N = 2: row 0 whatever the rows; N = 4: the lower middle, element 1
    rng = np.random.default_rng(8)
    for _ in range(20):
        d = rng.integers(0, 256, (4, 32), dtype=np.uint8)
        assert ref(*as_case(d[:2], [range(2)]))[1][0] == 0
        bits = np.unpackbits(d, axis=1).astype(int)
        dist = (bits[:, None, :] != bits[None, :, :]).sum(2)
        assert np.array_equal(medians(d), np.sort(dist, axis=1)[:, 1])


# ====================================================================== GPU
def check_host(pool, off, rows):
    """The synchronous host form against the restatement; returns best_pos."""
    n, bp, bm, out = ref(pool, off, rows)
    got = np.full((len(off) - 1, 32), SENTINEL, np.uint8)
    gn, gbp, gbm, gout = plvi.distinctive_descriptors(pool, off, rows, out_desc=got)
    assert gn == n
    assert np.array_equal(gbp, bp), np.flatnonzero(gbp != bp)[:10]
    assert np.array_equal(gbm, bm), np.flatnonzero(gbm != bm)[:10]
    assert np.array_equal(gout, out)
    return bp


class Batch:
    """The device tables of one batch call, outputs pre-filled with sentinels."""

    def __init__(self, pool, off, rows, want_desc=True):
        self.n_feat = len(off) - 1
        self.pool_rows = len(pool)
        mk = lambda a: self._up(np.ascontiguousarray(a))  # noqa: E731
        self.pool, self.off, self.rows = mk(pool), mk(np.asarray(off, np.int32)), mk(np.asarray(rows, np.int32))
        self.want_desc = want_desc
        self.fill()

    @staticmethod
    def _up(a):
        b = plvi.DeviceBuffer(max(a.nbytes, 4))
        if a.nbytes:
            b.upload(a)
        return b

    def fill(self):
        n = max(self.n_feat, 1)
        self.bp, self.bm = self._up(np.full(n, -7, np.int32)), self._up(np.full(n, -7, np.int32))
        self.out = self._up(np.full((n, 32), SENTINEL, np.uint8))

    def call(self, max_obs, stream=None):
        plvi.distinctive_descriptors_batch(self.n_feat, self.pool.ptr, self.pool_rows, self.off.ptr, self.rows.ptr,
                                           max_obs, self.bp.ptr, self.bm.ptr, self.out.ptr if self.want_desc else 0,
                                           stream)

    def read(self):
        plvi.load().plvi_device_synchronize()
        n = self.n_feat
        return (self.bp.download(np.zeros(max(n, 1), np.int32))[:n], self.bm.download(np.zeros(max(n, 1), np.int32))[:n],
                self.out.download(np.zeros((max(n, 1), 32), np.uint8))[:n])


def check_batch(pool, off, rows, max_obs):
    _, bp, bm, out = ref(pool, off, rows, max_obs=max_obs)
    b = Batch(pool, off, rows)
    b.call(max_obs)
    gbp, gbm, gout = b.read()
    assert np.array_equal(gbp, bp) and np.array_equal(gbm, bm) and np.array_equal(gout, out)
    return bp


@pytest.mark.gpu
def test_gpu_general_case(plvi_lib):
    pool, off, rows = general()
    check_host(pool, off, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4])
def test_gpu_small_n(plvi_lib, n):
    rng = np.random.default_rng(40 + n)
    pool = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    for trial in range(4):
        bp = check_host(*as_case(pool, [rng.permutation(6)[:n]]))
        if n <= 2:
            assert bp[0] == (-1 if n == 0 else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [SMALL - 1, SMALL, SMALL + 1])
def test_gpu_path_boundary(plvi_lib, n):
    check_host(*seeded(100 + n, [n]))
    # beside short lists, which then share the launch with the long one
    check_host(*seeded(200 + n, [5, n, 1, n, 17]))


@pytest.mark.gpu
@pytest.mark.parametrize("max_obs", [7, 8, 9, 16, 17, 32, 33])
def test_gpu_segment_sizes(plvi_lib, max_obs):
    """The wave segment grows with max_obs: 8, 16, 32 and 64 lanes per feature, each at both sides of its seam."""
    counts = np.random.default_rng(max_obs).integers(0, max_obs + 1, 150)
    counts[[0, 77, 149]] = max_obs
    pool, off, rows = seeded(300 + max_obs, counts)
    check_batch(pool, off, rows, max_obs)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [300, 1448, LIMIT])
def test_gpu_long_list(plvi_lib, n):
    check_host(*seeded(n, [n]))


@pytest.mark.gpu
def test_gpu_several_long_lists_in_one_launch(plvi_lib):
    """Each long list is divided among several workgroups by list position: all of them must see one layout."""
    pool, off, rows = seeded(78, [65, 700, 3, 129, 0, 512, 40, 333])
    rows = rows.copy()
    rows[5::7] = -1
    for _ in range(3):
        check_host(pool, off, rows)


@pytest.mark.gpu
def test_gpu_long_list_with_ignored_rows(plvi_lib):
    """The LDS path keeps an ignored entry's slot (flagged, counted in no histogram); best_pos counts it."""
    pool, off, rows = seeded(77, [200])
    lst = list(rows)
    for at in (0, 3, 64, 65, 150, 205):
        lst.insert(at, -1 if at % 2 else len(pool))
    bp = check_host(*as_case(pool, [lst, lst[:70], [-1] * 70, lst[60:140]]))
    assert bp[2] == -1 and bp[0] >= 0


@pytest.mark.gpu
def test_gpu_ties(plvi_lib):
    same = np.tile(np.random.default_rng(1).integers(0, 256, (1, 32), dtype=np.uint8), (100, 1))
    for n in (7, 64, 100):
        p, o, r = as_case(same, [range(n)])
        assert check_host(p, o, r)[0] == 0 and ref(p, o, r)[2][0] == 0
    assert check_host(*as_case(tie_5_9(), [range(12)]))[0] == 5
    assert check_host(*as_case(tie_5_9(), [range(11, -1, -1)]))[0] == 2
    # across the waves of the LDS path, and across the lanes of one wave
    assert check_host(*as_case(tie_two(80, 10, 70), [range(80)]))[0] == 10
    assert check_host(*as_case(tie_two(80, 10, 70), [range(79, -1, -1)]))[0] == 9
    assert check_host(*as_case(tie_two(60, 10, 50), [range(60)]))[0] == 10


@pytest.mark.gpu
def test_gpu_distance_256(plvi_lib):
    for n_a, n_b in ((1, 1), (2, 1), (1, 2), (3, 4), (39, 41), (41, 39)):
        d = complement_mix(n_a, n_b)
        check_host(*as_case(d, [range(n_a + n_b)]))


@pytest.mark.gpu
def test_gpu_pool_indirection(plvi_lib):
    pool, _, _ = seeded(9, [40])
    last = len(pool) - 1
    lists = [[30, 2, 17, last, 5], [5, 17, 17, 17, 2, 30, 30], [last], [last, last, 0], [2, 5] * 35]
    check_host(*as_case(pool, lists))


@pytest.mark.gpu
def test_gpu_ignored_entries(plvi_lib):
    pool, _, rows = seeded(10, [12])
    n = len(pool)
    l0, l1, r1, r2 = (int(v) for v in rows[:4])
    lists = [[-1, l0, n, l1, r1, -1, r2, n + 5, int(rows[5]), -(1 << 31), (1 << 31) - 1, int(rows[6])],
             [-1, n, -1], [l0, -1, l1, r1, -1, r2], [-1, -1, l0], [n] * 66 + [l0]]
    bp = check_host(*as_case(pool, lists))
    assert bp[1] == -1 and bp[3] == 2 and bp[4] == 66


@pytest.mark.gpu
def test_gpu_csr_shapes(plvi_lib):
    counts = [0, 3, 0, 0, 9, 1, 0, 70, 0, 2, 0]
    pool, off, rows = seeded(11, counts)
    bp = check_host(pool, off, rows)
    assert bp[0] == bp[-1] == -1
    # a decreasing offset reads as an empty list (batch form only: the host form refuses it)
    off2 = off.copy()
    off2[5] = off2[4] - 2
    bp2 = check_batch(pool, off2, rows, 70)
    assert bp2[4] == -1 and bp2[5] >= 0
    # a list longer than max_obs reads as its first max_obs entries
    for max_obs in (5, 64, 65, 69):
        check_batch(pool, off, rows, max_obs)
    pool, off, rows = seeded(12, [90, 400, 20])
    for max_obs in (64, 96, 97, 128, 129):
        check_batch(pool, off, rows, max_obs)


@pytest.mark.gpu
def test_gpu_thousand_short_features(plvi_lib):
    counts = np.random.default_rng(13).integers(1, 9, 1000)
    pool, off, rows = seeded(13, counts, flip=0.03)  # few bits: many ties
    check_host(pool, off, rows)
    assert (np_ref(pool, off, rows)[2] >= 2).sum() >= 100


@pytest.mark.gpu
def test_gpu_errors_and_null_out_desc(plvi_lib):
    pool, off, rows = seeded(14, [4, 70, 0, 9])
    b = Batch(pool, off, rows, want_desc=False)
    with pytest.raises(plvi.PlviError) as e:
        b.call(LIMIT + 1)
    assert e.value.code == E_CAPACITY
    for bad in (lambda: b.call(-1),
                lambda: plvi.distinctive_descriptors_batch(-1, b.pool.ptr, 1, b.off.ptr, b.rows.ptr, 4, b.bp.ptr,
                                                           b.bm.ptr),
                lambda: plvi.distinctive_descriptors_batch(1, b.pool.ptr, -1, b.off.ptr, b.rows.ptr, 4, b.bp.ptr,
                                                           b.bm.ptr)):
        with pytest.raises(plvi.PlviError) as e:
            bad()
        assert e.value.code == E_BADARG
    gbp, gbm, gout = b.read()
    assert (gbp == -7).all() and (gbm == -7).all()  # nothing was launched
    b.call(70)  # a NULL d_out_desc is accepted
    gbp, gbm, gout = b.read()
    _, bp, bm, _ = ref(pool, off, rows)
    assert np.array_equal(gbp, bp) and np.array_equal(gbm, bm) and (gout == SENTINEL).all()
    lib = plvi.load()
    assert lib.plvi_distinctive_descriptors_batch(0, None, 0, None, None, 0, None, None, None, None) == 0
    assert lib.plvi_distinctive_descriptors(None, 0, None, None, 0, None, None, None) == 0
    with pytest.raises(plvi.PlviError) as e:
        plvi.distinctive_descriptors(pool, np.array([0, 5, 3, 9], np.int32), rows)
    assert e.value.code == E_BADARG
    with pytest.raises(plvi.PlviError) as e:
        plvi.distinctive_descriptors(pool, np.array([-1, 5], np.int32), rows)
    assert e.value.code == E_BADARG
    with pytest.raises(plvi.PlviError) as e:
        plvi.distinctive_descriptors(pool[:1], np.array([0, LIMIT + 1], np.int32), np.zeros(LIMIT + 1, np.int32))
    assert e.value.code == E_CAPACITY


@pytest.mark.gpu
def test_gpu_lbd_rows(plvi_lib):
    """The pool is the LBD table of a fixture frame: nothing assumes ORB, and the distance is
    ORBmatcher::DescriptorDistance, not LineMatcher's halved one."""
    import oracle_lib
    import util
    _, desc, _ = oracle_lib.line_extract(util.real_frames()["rgb1_gray"])
    assert len(desc) >= 50
    rng = np.random.default_rng(15)
    lists = [rng.integers(0, len(desc), rng.integers(1, 25)) for _ in range(120)] + [np.arange(min(len(desc), LIMIT))]
    check_host(*as_case(desc, lists))


@pytest.mark.gpu
def test_gpu_graph_capture(plvi_lib):
    """The batch form under plvi_graph_capture_begin / end, replayed once: short and long lists (the memset
    node, the LDS kernel and the segment kernel in one graph)."""
    pool, off, rows = seeded(16, [6, 100, 0, 31, 64, 65, 2])
    _, bp, bm, out = ref(pool, off, rows)
    b = Batch(pool, off, rows)
    st = ctypes.c_void_p()
    assert plvi_lib.plvi_stream_create(ctypes.byref(st)) == 0
    g = plvi.StepGraph(lambda s: b.call(100, stream=s), st.value)
    gbp, _, _ = b.read()
    assert (gbp == -7).all()  # captured, not run
    g.launch()
    assert plvi_lib.plvi_stream_synchronize(st) == 0
    gbp, gbm, gout = b.read()
    assert np.array_equal(gbp, bp) and np.array_equal(gbm, bm) and np.array_equal(gout, out)
    del g
    assert plvi_lib.plvi_stream_destroy(st) == 0
