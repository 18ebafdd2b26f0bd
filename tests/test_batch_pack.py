"""tests/batch_pack.py checked without a GPU: un-padding the packed tables returns the cases, and the
poison rows really are attractive -- an oracle fed n + k rows (or the poison FeatureVector nodes) answers
differently on the first n for at least one pair of each family, so a kernel that reads past a count cannot
pass the contract tests (tests/test_batch_contract_gpu.py) by luck."""
import numpy as np

import batch_pack as bp
import oracle_lib as ol
import util

K = 12  # rows read past the count


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_pack_rows_layout():
    t = [np.arange(6, dtype=np.int32).reshape(3, 2), np.zeros((0, 2), np.int32)]
    poison = [np.array([[-1, -2]], np.int32), np.array([[7, 8], [9, 10]], np.int32)]
    out = bp.pack_rows(t, 4, poison)
    assert out.shape == (2 + bp.SLACK, 4, 2) and out.dtype == np.int32
    assert _same(bp.unpack_rows(out, [3, 0]), t)
    assert out[0, 3].tolist() == [-1, -2]
    assert out[1].tolist() == [[7, 8], [9, 10], [7, 8], [9, 10]] and np.array_equal(out[2], out[1])
    c = bp.counts_array([3, 0], {1: -4})
    assert c[:2].tolist() == [3, -4] and len(c) == 2 + bp.SLACK


def test_knn_poison_is_attractive():
    rng = np.random.default_rng(1)
    cases = [util.near_duplicate_descriptors(rng, 30, 40), util.near_duplicate_descriptors(rng, 45, 20)]
    cases.append((cases[0][0][:0], cases[0][1][:10]))
    pk = bp.pack_knn(cases, 64, 60)
    assert _same(bp.unpack_rows(pk["q"], pk["nq"]), [c[0] for c in cases])
    assert _same(bp.unpack_rows(pk["t"], pk["nt"]), [c[1] for c in cases])
    changed_knn = changed_match = 0
    for p, (q, t) in enumerate(cases[:2]):
        changed_knn += not _same(ol.knn2(q, pk["t"][p, :len(t) + K]), ol.knn2(q, t))
        n, m = ol.match(q, t, 0.9)
        n2, m2 = ol.match(pk["q"][p, :len(q) + K], t, 0.9)
        changed_match += not np.array_equal(m2[:len(q)], m)
        n3, m3 = ol.match(q, pk["t"][p, :len(t) + K], 0.9)
        changed_match += not np.array_equal(m3, m)
    assert changed_knn == 2 and changed_match >= 2


def test_bow_poison_is_attractive():
    caps = (200, 181, 32)
    cases = [util.bow_case(3, n_kf=150, n_f=160, n_nodes=20), util.bow_case(4, n_kf=120, n_f=181, n_nodes=25)]
    pk = bp.pack_bow(cases, *caps)
    changed = 0
    for p, c in enumerate(cases):
        kd, ka, kl, kfv, fd, fa, ffv = c
        assert np.array_equal(pk["kd"][p, :len(kd)], kd) and np.array_equal(pk["fd"][p, :len(fd)], fd)
        assert np.array_equal(pk["ka"][p, :len(ka)], ka) and np.array_equal(pk["fa"][p, :len(fa)], fa)
        assert np.array_equal(pk["kl"][p, :len(kl)], kl)
        for fv, N, O, I, cnt in ((kfv, pk["kn"], pk["ko"], pk["ki"], pk["kc"]),
                                 (ffv, pk["fn"], pk["fo"], pk["fi"], pk["fc"])):
            nodes, off, idx = bp.bow_csr(fv)
            assert cnt[p] == len(nodes) and np.array_equal(N[p, :len(nodes)], nodes)
            assert np.array_equal(O[p, :len(off)], off) and np.array_equal(I[p, :len(idx)], idx)
            assert (np.diff(N[p]) > 0).all() and (np.diff(O[p]) >= 0).all()  # still a sorted CSR all the way
        assert pk["ko"][p, -1] <= caps[0] and pk["fo"][p, -1] <= caps[1]
        assert (pk["ki"][p] < caps[0]).all() and (pk["fi"][p] < caps[1]).all()
        # the packed poison nodes are the ones bow_poisoned_case makes real
        pc = bp.bow_poisoned_case(c, *caps)
        nodes, off, idx = bp.bow_csr(pc[3])
        assert np.array_equal(pk["kn"][p, :len(nodes)], nodes) and np.array_equal(pk["ko"][p, :len(off)], off)
        assert np.array_equal(pk["ki"][p, :len(idx)], idx) and np.array_equal(pk["kd"][p, :len(pc[0])], pc[0])
        nodes, off, idx = bp.bow_csr(pc[6])
        assert np.array_equal(pk["fn"][p, :len(nodes)], nodes) and np.array_equal(pk["fo"][p, :len(off)], off)
        assert np.array_equal(pk["fi"][p, :len(idx)], idx)
        n, m = ol.search_by_bow(*c, 0.75, True)
        n2, m2 = ol.search_by_bow(*pc, 0.75, True)
        changed += not np.array_equal(m, m2)
    assert changed >= 1


def test_match_grid_poison_is_attractive():
    cases = [util.stereo_line_case(s, n=60 + 20 * s) for s in range(2)]
    off0, idx0 = bp.grid_csr(cases[0][2])
    pk = bp.pack_match_grid(cases, 100, 90, 2500)
    for k, i in (("lines1", 0), ("desc1", 1), ("desc2", 3), ("dirs2", 4)):
        n = pk["n1"] if i < 2 else pk["n2"]
        assert _same(bp.unpack_rows(pk[k], n), [c[i] for c in cases])
    assert np.array_equal(pk["cell_off"][0], off0) and np.array_equal(pk["cell_idx"][0, :len(idx0)], idx0)
    assert (pk["cell_idx"] >= 0).all() and (pk["cell_idx"][0] < pk["n2"][0]).all()
    assert np.allclose(np.hypot(pk["dirs2"][..., 0], pk["dirs2"][..., 1]), 1.0)
    changed = 0
    for p, c in enumerate(cases):
        n1 = len(c[0])
        for hint in (0, 1):
            n, m = ol.match_grid(*c, range_hint=hint)
            n2, m2 = ol.match_grid(pk["lines1"][p, :n1 + K], pk["desc1"][p, :n1 + K], *c[2:], range_hint=hint)
            changed += not np.array_equal(m, m2[:n1])
    assert changed >= 1


def test_line_proj_poison_is_attractive():
    cases = [util.line_proj_case(s, n_cur=70 + 10 * s, n_last=60 + 5 * s) for s in range(2)]
    pk = bp.pack_line_proj(cases, 100, 90, 2500)
    for k in bp.LINE_PROJ_CUR:
        assert _same(bp.unpack_rows(pk[k], pk["n_cur"]), [c[k] for c in cases])
    for k in bp.LINE_PROJ_LAST:
        assert _same(bp.unpack_rows(pk[k], pk["n_last"]), [c[k] for c in cases])
    assert (pk["last_flags"][0, pk["n_last"][0]:] & 1).all()
    angth = float(np.float32(np.pi / 8))
    changed = 0
    for p, c in enumerate(cases):
        n, m = ol.line_search_projection(c, 3.0, angth, 1)
        c2 = dict(c)
        for k in bp.LINE_PROJ_LAST:
            c2[k] = pk[k][p, :pk["n_last"][p] + K]
        n2, m2 = ol.line_search_projection(c2, 3.0, angth, 1)
        changed += not np.array_equal(m, m2)
    assert changed >= 1
    # cutting a case down keeps the rest
    sub = bp.line_proj_sub(cases[0], n_cur=0, grid=bp.empty_grid(64, 48))
    assert len(sub["cur_desc"]) == 0 and len(sub["ml_desc"]) == len(cases[0]["ml_desc"])
    assert ol.line_search_projection(sub, 3.0, angth, 1)[0] == 0


# ------------------------------------------------------------------ the keyed families (proj.hip, init, stereo lines)
def _unpads(cases, cap, spec):
    pk = bp.pack_keyed(cases, cap, spec)
    for k in spec:
        assert _same(bp.unpack_rows(pk[k], [len(c[k]) for c in cases]), [c[k] for c in cases]), k
    return pk


def _changed(oracle, cases, pk, keys, k_extra):
    """Pairs whose oracle answer on the first n rows changes when it is fed n + k_extra rows of the packed
    tables `keys` (the other tables as they are)."""
    changed = 0
    for p, c in enumerate(cases):
        c2 = dict(c)
        for k in keys:
            c2[k] = pk[k][p, :len(c[k]) + k_extra]
        a, b = oracle(c), oracle(c2)
        changed += not all(np.array_equal(x, y[:len(x)]) for x, y in zip(a, b))
    return changed


ONE_CAMERA = [
    (lambda s: util.projection_case(s, n_cur=200, n_last=150, uright=True), bp.CUR_U, bp.PROJ_LAST,
     lambda c: ol.search_by_projection(c, 15.0)[1:]),
    (lambda s: util.reloc_case(s, n_cur=200, n_kf=150), bp.CUR, bp.RELOC_KF,
     lambda c: ol.search_reloc(c, 10.0, 100)[1:]),
    (lambda s: util.local_case(s, n_cur=200, n_mp=150, uright=True), bp.CUR_U, bp.LOCAL_MP,
     lambda c: ol.search_local(c, 1.0, 0.8)[1:]),
]


def test_one_camera_poison_is_attractive():
    """The very first padding row of the last-frame / KeyFrame / MapPoint table changes every pair's answer:
    it aims at a keypoint no real point can take, with that keypoint's descriptor."""
    for gen, cur, last, oracle in ONE_CAMERA:
        cases = [gen(200 + s) for s in range(2)]
        pk = {**_unpads(cases, 230, cur), **_unpads(cases, 190, last)}
        assert _changed(oracle, cases, pk, list(last), 1) == 2, list(last)
        assert _changed(oracle, cases, pk, list(last), 3) == 2


def test_two_camera_poison_is_attractive():
    cases = [util.projection_stereo_case(210 + s, n_left=200, n_right=180, n_last=150) for s in range(2)]
    pk = {**_unpads(cases, 220, bp.LEFT), **_unpads(cases, 200, bp.RIGHT), **_unpads(cases, 170, bp.PROJ2_LAST)}
    assert _changed(lambda c: ol.search_by_projection_stereo(c, 7.0)[1:], cases, pk, list(bp.PROJ2_LAST), 1) == 2
    pin = [util.projection_stereo_case(214, n_left=200, n_right=180, n_last=150, kb8=False)]
    pk = bp.pack_keyed(pin, 170, bp.PROJ2_LAST)
    assert _changed(lambda c: ol.search_by_projection_stereo(c, 7.0)[1:], pin, pk, list(bp.PROJ2_LAST), 1) == 1
    cases = [util.local_stereo_case(220 + s, n_left=200, n_right=180, n_mp=150) for s in range(2)]
    pk = {**_unpads(cases, 220, bp.LOCAL2_LEFT), **_unpads(cases, 200, bp.LOCAL2_RIGHT),
          **_unpads(cases, 170, bp.LOCAL2_MP)}
    assert _changed(lambda c: ol.search_local_stereo(c, 1.0)[1:], cases, pk, list(bp.LOCAL2_MP), 1) == 2


def _init_case(seed, n1=200, n2=150):
    """F2 keypoints over a 640 x 480 image, F1 = moved F2 keypoints (mostly level 0) with ~5 % flipped bits."""
    from plvi import KEYPOINT_DTYPE
    rng = np.random.default_rng(seed)
    k2 = np.zeros(n2, KEYPOINT_DTYPE)
    k2["x"], k2["y"] = rng.uniform(0, 640, n2), rng.uniform(0, 480, n2)
    k2["octave"] = np.minimum(rng.geometric(0.5, n2) - 1, 7)
    k2["angle"] = rng.uniform(0, 360, n2)
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    src = rng.integers(0, n2, n1)
    k1 = np.zeros(n1, KEYPOINT_DTYPE)
    k1["x"], k1["y"] = k2["x"][src] + rng.normal(0, 15, n1), k2["y"][src] + rng.normal(0, 15, n1)
    k1["octave"] = rng.random(n1) < 0.15
    k1["angle"] = np.mod(k2["angle"][src] + 10 + rng.normal(0, 4, n1), 360)
    bits = np.unpackbits(d2[src], axis=1) ^ (rng.random((n1, 256)) < 0.05).astype(np.uint8)
    return {"k1": k1, "d1": np.packbits(bits, axis=1), "prev": np.stack([k1["x"], k1["y"]], 1).astype(np.float32),
            "k2": k2, "d2": d2}


def test_init_poison_is_attractive():
    grid = tuple(np.float32(v) for v in (0, 0, 64 / 640, 48 / 480))
    cases = [_init_case(230 + s) for s in range(2)]
    pk = {**_unpads(cases, 240, bp.INIT_K1), **_unpads(cases, 190, bp.INIT_K2)}

    def oracle(c):
        return ol.search_for_initialization(c["k1"], c["d1"], c["prev"], c["k2"], c["d2"], grid)[1:]
    # one more F2 keypoint: the F1 point it was made for matches it at distance 0
    assert _changed(oracle, cases, pk, list(bp.INIT_K2), 1) == 2
    # more F1 keypoints: each steals the F2 keypoint it copies from the real point that held it, if one did
    assert _changed(oracle, cases, pk, list(bp.INIT_K1), 3) >= 1
    # LineMatcher::SerachForInitialize runs on the kNN-2 tables (pack_knn)
    rng = np.random.default_rng(5)
    q, t = util.near_duplicate_descriptors(rng, 30, 40)
    kn = bp.pack_knn([(q, t)], 50, 45)
    assert not np.array_equal(ol.line_search_init(q, kn["t"][0, :31])[0], ol.line_search_init(q, t)[0])


def test_stereo_lines_poison_is_attractive():
    from plvi import synth
    cases = []
    for seed in (11, 12):
        L, R, _ = synth.stereo_pair(seed)
        (kl, dl, _), (kr, dr, _) = ol.line_extract(L), ol.line_extract(R)
        cases.append({"klL": kl[:60], "dL": dl[:60], "klR": kr[:70], "dR": dr[:70]})
    pk = {**_unpads(cases, 80, bp.STEREO_L), **_unpads(cases, 90, bp.STEREO_R)}

    def oracle(c):
        return ol.stereo_lines(c["klL"], c["dL"], c["klR"], c["dR"], None, 640, 480, 47.9)[1:]
    assert _changed(oracle, cases, pk, list(bp.STEREO_L), 3) >= 1
    assert _changed(oracle, cases, pk, list(bp.STEREO_R), 3) >= 1
