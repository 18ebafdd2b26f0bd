"""The staging rules of the synchronous "one item from host memory" entry points, on tiny inputs: what a host
form leaves untouched past the count it reports, what a NULL optional means, an empty second side given as NULL
arrays, and the round trip of an in/out array.  Every case is one call, or two calls compared.

Pinned elsewhere and not repeated here: the untouched out_desc row of a feature without observations
(test_distinctive.py, check_host), the vote table whose bad id comes back as -1 (test_local_map.py,
test_gpu_host_form[bad_vote_cleared]) and the first_conn / parent / covis rows of the slots a covisibility
update does not name (test_covis.py, test_gpu_host_form)."""
import ctypes

import numpy as np
import pytest

import plvi
import test_kfdb as tk
import test_local_map as tl
import test_loop_match as tlm
import test_fuse as tf
import test_triangulation as tt
import test_vocab as tv
import util

pytestmark = pytest.mark.gpu

SEED = 5        # the tiny seeded cases below have 1 to 4 matches with it (checked in each test)
S32, S8 = -77, 0xA5
ANGTH = float(np.float32(np.pi / 8))


def P(a):
    return None if a is None else plvi._ptr(a)


def sentinel(n, dtype=np.int32, width=None):
    fill = S8 if dtype == np.uint8 else S32
    return np.full(n if width is None else (n, width), fill, dtype)


def line_case():
    c = util.line_proj_case(SEED, n_cur=8, n_last=8)
    for k in ("last_flags", "x3dc", "last_octave", "ml_desc"):
        c[k] = c[k][:4]
    return c


# ------------------------------------------------------------------ the five projection searches as (nmatches, match)
def run_proj(c, blocked, uright=None):
    return plvi.ORBmatcher(0.9, True).SearchByProjection(
        util.proj_params(c, 15.0), c["cur_kps"], c["cur_desc"], c["x3dc"], c["last_octave"], c["last_angle"],
        c["mp_desc"], c["flags"], blocked, uright)


def run_reloc(c, blocked):
    return plvi.ORBmatcher(0.9, True).SearchByProjectionKF(
        util.reloc_params(c, 10.0, 100), c["cur_kps"], c["cur_desc"], c["kf_flags"], c["x3dc"], c["dist"], c["level"],
        c["kf_angle"], c["mp_desc"], blocked)


def run_sim3(c, matched):
    return plvi.ORBmatcher().SearchByProjectionSim3(
        tlm.sim3_params(c, 8, 1.5, 1), c["cur_kps"], c["cur_desc"], c["kf_flags"], c["x3dc"], c["dist"], c["dot"],
        c["level"], c["mp_desc"], matched, projection=1)


def run_local(c, blocked, uright=None):
    return plvi.ORBmatcher(0.8, True).SearchByProjectionLocal(
        util.local_params(c, 3.0), c["cur_kps"], c["cur_desc"], c["mp_flags"], c["mp_proj"], c["mp_level"],
        c["mp_desc"], blocked, uright)


def run_line_proj(c, blocked):
    return plvi.LineMatcher.SearchByProjection(
        util.line_proj_params(c, 5.0, ANGTH, 1), c["cur_angle"], c["cur_desc"], c["grid"], c["last_flags"], c["x3dc"],
        c["last_octave"], c["ml_desc"], blocked)


SEARCHES = {
    "projection": (lambda: util.projection_case(SEED, n_cur=8, n_last=4), run_proj),
    "reloc": (lambda: util.reloc_case(SEED, n_cur=8, n_kf=4), run_reloc),
    "sim3": (lambda: tlm.sim3_general(SEED, n_kp=8, n_pt=4), run_sim3),
    "local": (lambda: util.local_case(SEED, n_cur=8, n_mp=4), run_local),
    "line_projection": (line_case, run_line_proj),
}


# ================================================================== 2. a NULL optional is its documented meaning
@pytest.mark.parametrize("name", list(SEARCHES))
def test_null_blocked_is_all_zero(plvi_lib, name):
    make, run = SEARCHES[name]
    c = make()
    n0, m0 = run(c, None)
    n1, m1 = run(c, np.zeros(8, np.uint8))
    assert n0 == n1 >= 1 and np.array_equal(m0, m1)
    # and the array is read: the first matched keypoint blocked loses its match
    b = np.zeros(8, np.uint8)
    b[np.flatnonzero(m0 >= 0)[0]] = 1
    assert not np.array_equal(run(c, b)[1], m0)


def _uright_failing_at(kps_x, i):
    ur = np.full(len(kps_x), -1, np.float32)   # negative: monocular keypoint, no check
    ur[i] = kps_x[i] + 1000.0                   # a right coordinate no projection is near
    return ur


@pytest.mark.parametrize("name", ["projection", "local"])
def test_null_uright_against_given(plvi_lib, name):
    make, run = SEARCHES[name]
    c = make()
    blocked = np.zeros(8, np.uint8)
    n0, m0 = run(c, blocked, None)
    i = int(np.flatnonzero(m0 >= 0)[0])
    n1, m1 = run(c, blocked, np.full(8, -1, np.float32))
    assert n1 == n0 >= 1 and np.array_equal(m1, m0)
    n2, m2 = run(c, blocked, _uright_failing_at(c["cur_kps"]["x"], i))
    assert np.flatnonzero(m2 != m0).tolist() == [i] and m2[i] == -1 and n2 == n0 - 1


def test_null_uright_against_given_fuse(plvi_lib):
    c = tf.points_case([tf.kpt(100, 100), tf.kpt(300, 200)], [tf.PT_DESC, tf.PT_DESC],
                       [tf.pt(100, 100), tf.pt(300, 200)])
    run = lambda ur: plvi.ORBmatcher().Fuse(tf.fuse_params(c, 0, 3.0), c["kps"], c["desc"],  # noqa: E731
                                            *[c[k] for k in tf.PT_KEYS], uright=ur)
    n0, i0, d0 = run(None)
    assert n0 == 2 and i0.tolist() == [0, 1]
    n1, i1, d1 = run(np.full(2, -1, np.float32))
    assert n1 == 2 and np.array_equal(i1, i0) and np.array_equal(d1, d0)
    n2, i2, d2 = run(_uright_failing_at(c["kps"]["x"], 1))   # the stereo chi-square gate fails for keypoint 1
    assert n2 == 1 and i2.tolist() == [0, -1] and d2.tolist() == [d0[0], -1]


def _stereo_lines(klL, dL, klR, dR, klUn, nR=None):
    n = len(klL)
    m, disp, dep = sentinel(n + 2), np.full((n + 2, 2), S32, np.float32), np.full((n + 2, 2), S32, np.float32)
    le = np.full((n + 2, 3), S32, np.float64)
    k = plvi.load().plvi_stereo_lines(P(klL), P(dL), n, P(klR), P(dR), len(klR) if nR is None else nR, P(klUn), 640,
                                      480, 40.0, 1, P(m), P(disp), P(dep), P(le))
    return k, m, disp, dep, le


def stereo_line_pair(n=6):
    """n left lines and the same lines shifted left by a disparity of 20 px, same descriptors."""
    rng = np.random.default_rng(SEED)
    kl = np.zeros(n, plvi.KEYLINE_DTYPE)
    x0, y0 = rng.uniform(100, 500, n), rng.uniform(50, 400, n)
    kl["startPointX"], kl["startPointY"] = x0, y0
    kl["endPointX"], kl["endPointY"] = x0 + rng.uniform(20, 60, n), y0 + rng.uniform(30, 60, n)
    for a, b in (("sPointInOctaveX", "startPointX"), ("sPointInOctaveY", "startPointY"),
                 ("ePointInOctaveX", "endPointX"), ("ePointInOctaveY", "endPointY")):
        kl[a] = kl[b]
    kl["lineLength"] = np.hypot(kl["endPointX"] - kl["startPointX"], kl["endPointY"] - kl["startPointY"])
    kl["angle"] = np.arctan2(kl["endPointY"] - kl["startPointY"], kl["endPointX"] - kl["startPointX"])
    kr = kl.copy()
    for f in ("startPointX", "endPointX", "sPointInOctaveX", "ePointInOctaveX"):
        kr[f] -= 20.0
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return kl, d, kr, d.copy()


def test_null_klun_is_the_left_lines(plvi_lib):
    kl, dl, kr, dr = stereo_line_pair()
    a = _stereo_lines(kl, dl, kr, dr, None)
    b = _stereo_lines(kl, dl, kr, dr, kl)
    assert a[0] == b[0] >= 1
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()
    for out in a[1:]:   # and nothing past the nL rows
        assert (out[len(kl):] == S32).all()


def frustum_line_inputs():
    p = util.frustum_params(51)
    c = util.frustum_line_case(61, p, n=8)   # two of the eight lines are in view
    return p, c


def _frustum_lines(p, c, desc, n_extra=3):
    n = len(c["sep"])
    sp, nr = np.ascontiguousarray(c["sep"], np.float64), np.ascontiguousarray(c["normal"], np.float32)
    ds, fi = np.ascontiguousarray(c["dist"], np.float32), np.ascontiguousarray(c["in_flags"], np.uint8)
    pr, an = np.array(c["proj"], np.float32), np.array(c["angle"], np.float64)
    iv, cp, cd = np.zeros(n, np.uint8), sentinel(n + n_extra), sentinel(n + n_extra, np.uint8, 32)
    nc = plvi.load().plvi_frustum_lines(ctypes.byref(p), P(sp), P(nr), P(ds), P(fi), P(desc), n, P(iv), P(pr), P(an),
                                        P(cp), P(cd))
    return nc, iv, pr, an, cp, cd


def test_frustum_lines_tail_and_null_desc(plvi_lib):
    p, c = frustum_line_inputs()
    desc = np.ascontiguousarray(c["desc"], np.uint8)
    nc, iv, pr, an, cp, cd = _frustum_lines(p, c, desc)
    assert 0 < nc < 8 and iv.sum() == nc              # at least one line in view and one out
    assert cp[:nc].tolist() == np.flatnonzero(iv).tolist() and (cp[nc:] == S32).all()
    assert np.array_equal(cd[:nc], desc[cp[:nc]]) and (cd[nc:] == S8).all()
    nc2, iv2, pr2, an2, cp2, cd2 = _frustum_lines(p, c, None)
    assert nc2 == nc and (cd2 == S8).all()            # no descriptors: compact_desc is not written at all
    for x, y in ((iv, iv2), (pr, pr2), (an, an2), (cp, cp2)):
        assert x.tobytes() == y.tobytes()


def kfdb_small():
    """Four keyframes of map 0 that share three words with the query, with distinct scores: the device database
    and the restatement of test_kfdb.py."""
    db, ref = plvi.KeyFrameDatabase(100, 4, 8), tk.NpDB(100, 4)
    for s in range(4):
        v = np.array([1 + 0.05 * s, 2, 3, 4], np.float64)
        b = (np.array([1, 2, 3, 60 + s], np.uint32), v / v.sum())
        db.add(s, b, 0)
        assert ref.add(s, b, 0) == 0
    q = (np.array([1, 2, 3], np.uint32), np.array([0.2, 0.3, 0.5]))
    return db, ref, q


def _kfdb_query(db, q, mode, covis=None, map_bad=None, cand_cap=7, n_best=2):
    w, v = np.ascontiguousarray(q[0], np.uint32), np.ascontiguousarray(q[1], np.float64)
    cand, loop, merge = sentinel(7), sentinel(7), sentinel(7)
    nl, nm = ctypes.c_int(S32), ctypes.c_int(S32)
    rc = plvi.load().plvi_kfdb_query(db._h, P(w), P(v), len(w), 0, mode, n_best, None, 0, P(covis), P(map_bad),
                                     0 if map_bad is None else len(map_bad), P(cand), cand_cap, P(loop),
                                     ctypes.byref(nl), P(merge), ctypes.byref(nm))
    return rc, cand, loop, nl.value, merge, nm.value


def test_kfdb_query_tails_and_null_tables(plvi_lib):
    db, ref, q = kfdb_small()
    exp = ref.query(q, 0, 0, 2, set(), None, None)["a"]
    n, cand, loop, nl, merge, nm = _kfdb_query(db, q, 0)
    assert 0 < n == len(exp) <= 4 and cand[:n].tolist() == exp and (cand[n:] == S32).all()
    assert (loop == S32).all() and (merge == S32).all() and nl == S32 and nm == S32   # mode 0 writes neither
    n2, cand2, *_ = _kfdb_query(db, q, 0, cand_cap=1)
    assert n2 == n and cand2[0] == cand[0] and (cand2[1:] == S32).all()             # the full count, one entry
    # covis NULL = a table without neighbours
    n3, cand3, *_ = _kfdb_query(db, q, 0, covis=np.full((4, plvi.KFDB_NEIGHBOURS), -1, np.int32))
    assert n3 == n and np.array_equal(cand3, cand)
    exp = ref.query(q, 0, 1, 2, set(), None, None)
    rc, cand, loop, nl, merge, nm = _kfdb_query(db, q, 1)
    assert rc == nl + nm and 0 < nl <= 2 and 0 <= nm <= 2 and (cand == S32).all()
    assert loop[:nl].tolist() == exp["a"] and merge[:nm].tolist() == exp["b"]
    assert (loop[nl:] == S32).all() and (merge[nm:] == S32).all()
    # map_bad NULL = no bad map
    rc2, _, loop2, nl2, merge2, nm2 = _kfdb_query(db, q, 1, map_bad=np.zeros(1, np.uint8))
    assert (rc2, nl2, nm2) == (rc, nl, nm) and np.array_equal(loop2, loop) and np.array_equal(merge2, merge)


def test_vocab_transform_tails(plvi_lib, tmp_path):
    vg = plvi.ORBVocabulary.loadFromTextFile(tv._write(tmp_path, tv.KAT_TEXT), emulate_tail=False)
    f = np.zeros((5, 32), np.uint8)   # the features of test_oracle_transform_known_answers
    f[0, 0], f[1, 0], f[3, 0] = 1, 3, 1
    f[2], f[4] = 255, 254
    bw, fn, fi = np.full(8, 77, np.uint32), np.full(8, 77, np.uint32), np.full(8, 77, np.uint32)
    bv, fo = np.full(8, -7.0, np.float64), sentinel(9)
    nb, nf = ctypes.c_int(S32), ctypes.c_int(S32)
    assert plvi_lib.plvi_vocab_transform(vg._h, P(f), 5, 1, P(bw), P(bv), ctypes.byref(nb), P(fn), P(fo), P(fi),
                                         ctypes.byref(nf)) == 0
    assert (nb.value, nf.value) == (2, 2)
    assert bw.tolist() == [0, 2] + [77] * 6 and np.allclose(bv[:2], [0.2, 0.8]) and (bv[2:] == -7.0).all()
    assert fn.tolist() == [1, 2] + [77] * 6 and fo.tolist() == [0, 2, 4] + [S32] * 6
    assert fi.tolist() == [0, 3, 2, 4] + [77] * 4
    # a caller that wants the BowVector alone: the other lists are optional
    bw2, bv2 = np.full(8, 77, np.uint32), np.full(8, -7.0, np.float64)
    assert plvi_lib.plvi_vocab_transform(vg._h, P(f), 5, 1, P(bw2), P(bv2), ctypes.byref(nb), None, None, None,
                                         ctypes.byref(nf)) == 0
    assert (nb.value, nf.value) == (2, 2) and np.array_equal(bw2, bw) and np.array_equal(bv2, bv)


def test_local_map_tails(plvi_lib):
    """lmp_cap above the list: list, mp_pos, mp_desc, mp_in_flags rows past n_local_mp keep the fill, and
    n_local_ml is not written without lines."""
    m = tl.Map(4, kp_cap=4, n_mp=4)
    p0, p1, p2 = m.point(0), m.point(0, 1), m.point(1)
    m.put(0, p0, p1)
    m.put(1, p1, p2)
    lm = plvi.LocalMap(*m.tables())
    kept = {}
    outputs = lm._outputs
    lm._outputs = lambda *a, **k: kept.setdefault("o", outputs(*a, **k))
    got = lm.update(np.array([0, 1], np.int32), lmp_cap=7)
    o, n = kept["o"], got["n_local_mp"]
    assert 0 < n < 7 and got["err"] == 0
    assert (o["local_mp"][0, :n] >= 0).all() and (o["local_mp"][0, n:] == -1).all()
    assert (o["mp_pos"][0, n:] == -1).all() and (o["mp_desc"][0, n:] == (-1 & 0x7f)).all()
    assert (o["mp_in_flags"][0, n:] == (-1 & 0x7f)).all()
    assert "n_local_ml" not in o
    # the same call with a place for the line count: it stays as the caller left it
    nml = sentinel(1)
    tabs = lm._tables()
    kf, mp, _ = lm._structs(lambda g, k: tabs[(g, k)].ctypes.data)
    vote, nv, last = np.array([0, 1], np.int32), np.array([2], np.int32), np.array([-1], np.int32)
    fr = plvi.LocalMapFrames()
    fr.vote_mp, fr.n_vote_mp, fr.vote_mp_cap, fr.last_kf = vote.ctypes.data, nv.ctypes.data, 2, last.ctypes.data
    res = outputs(1, [4, 7, 0], False, -1)
    out = plvi.LocalMapOutputs(4, 7, 0)
    for k, a in res.items():
        setattr(out, k, a.ctypes.data)
    out.n_local_ml = nml.ctypes.data
    assert plvi_lib.plvi_local_map(ctypes.byref(kf), ctypes.byref(mp), None, ctypes.byref(fr), ctypes.byref(out)) == 0
    assert nml[0] == S32 and res["n_local_mp"][0] == n


# ================================================================== 3. an empty second side, given as NULL arrays
def test_empty_second_side_projection_forms(plvi_lib):
    lib = plvi_lib
    c = util.projection_case(SEED, n_cur=8, n_last=4)
    k, d = np.ascontiguousarray(c["cur_kps"]), np.ascontiguousarray(c["cur_desc"])
    byref = ctypes.byref

    def expect(rc, m, none=-1):
        assert rc == 0 and (m == none).all()

    m = sentinel(8)
    p = util.proj_params(c, 15.0)
    p.check_orientation = 1
    expect(lib.plvi_search_by_projection(byref(p), P(k), P(d), 8, None, None, None, None, None, None, None, 0, P(m)), m)
    m = sentinel(8)
    expect(lib.plvi_search_reloc(byref(util.reloc_params(util.reloc_case(SEED, 8, 4), 10.0, 100)), P(k), P(d), 8,
                                 None, None, None, None, None, None, None, 0, P(m)), m)
    m = sentinel(8)
    s = tlm.sim3_general(SEED, n_kp=8, n_pt=4)
    expect(lib.plvi_search_sim3_projection(byref(tlm.sim3_params(s, 8, 1.5, 1)), P(k), P(d), 8, None, None, None,
                                           None, None, None, None, 0, P(m)), m)
    m = sentinel(8)
    lp = util.local_params(util.local_case(SEED, n_cur=8, n_mp=4), 3.0)
    lp.nnratio = 0.8
    expect(lib.plvi_search_local(byref(lp), P(k), P(d), 8, None, None, None, None, None, None, 0, P(m)), m)


def test_empty_second_side_line_and_stereo_forms(plvi_lib):
    lib = plvi_lib
    lines1, desc1, grid, _, _ = util.stereo_line_case(SEED, n=8, ties=False)
    cols, rows, off, idx = plvi.grid_csr(grid)
    l1, d1 = np.ascontiguousarray(lines1, np.int32), np.ascontiguousarray(desc1, np.uint8)
    n1 = len(l1)
    m = sentinel(n1 + 2)
    assert 0 < n1 <= 8 and lib.plvi_line_match_grid(P(l1), P(d1), n1, cols, rows, P(off), P(idx), None, None, 0, 7, 0,
                                                    2, 2, 1, P(m)) == 0
    assert (m[:n1] == -1).all() and (m[n1:] == S32).all()
    kl, dl, _, _ = stereo_line_pair()
    k, m, disp, dep, le = _stereo_lines(kl, dl, kl[:0], dl[:0], None, nR=0)
    assert k == 0 and (m[:6] == -1).all() and (disp[:6] == -1).all() and (dep[:6] == -1).all()
    # rectified ORB stereo: no right keypoint, every left keypoint without depth
    rng = np.random.default_rng(SEED)
    kps = np.zeros(8, plvi.KEYPOINT_DTYPE)
    kps["x"], kps["y"] = rng.uniform(20, 100, 8), rng.uniform(20, 60, 8)
    img = rng.integers(0, 256, (80, 128), dtype=np.uint8)
    n, ur, dp = plvi.ComputeStereoMatches(kps, rng.integers(0, 256, (8, 32), dtype=np.uint8), kps[:0],
                                          np.zeros((0, 32), np.uint8), [img], [img], [1.0], [1.0], 0.1, 40.0)
    assert n == 0 and (ur == -1).all() and (dp == -1).all()


def test_empty_second_side_triangulation(plvi_lib):
    c = tt.small_case(SEED, 8, 8)
    node, off, idx = plvi.feature_vector_csr(c["fv1"])
    pair = tt.pair_of(c)
    m = sentinel(8)
    assert plvi_lib.plvi_search_for_triangulation(ctypes.byref(pair), P(c["kps1"]), P(c["desc1"]), 8, P(node), P(off),
                                                  len(node), P(idx), P(c["has1"]), P(c["ur1"]), None, None, 0, None,
                                                  None, 0, None, None, None, P(m)) == 0
    assert (m == -1).all()


# ================================================================== 4. the round trip of an in/out array
def test_frustum_points_in_out(plvi_lib):
    p = util.frustum_params(11)
    c = util.frustum_case(21, p, n=8)   # four of the eight points are visible
    c["in_flags"][5] &= 0xFE   # not to be evaluated: the kernel writes its flag alone
    nv, fl, pr, lv, de, _, _ = plvi.frustum_points(p, c["pos"], c["normal"], c["dist"], c["in_flags"], c["proj"],
                                                   c["level"], c["depth"])
    assert 0 < nv < 8
    # a point that is not evaluated keeps the caller's proj / level / depth ...
    assert pr[5].tobytes() == c["proj"][5].tobytes() and lv[5] == c["level"][5] and de[5] == c["depth"][5]
    # ... and so does the level / depth of an evaluated point the frustum rejects (its proj x, y are written)
    rej = [i for i in range(8) if c["in_flags"][i] & 1 and not fl[i] & 1]
    assert rej
    for i in rej:
        assert lv[i] == c["level"][i] and de[i] == c["depth"][i] and pr[i, 3] == c["proj"][i, 3]
