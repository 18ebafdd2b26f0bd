"""The chain plvi.LocalBAWindow -> local_feat passed on as a device address for d_ids -> plvi_feature_refresh_batch ->
plvi_frustum_points_batch reading the refreshed normal / dist columns in place, with no host step between, against
the same chain through the restatements (tests/native/ba_window_ref.cpp, feature_refresh_ref.cpp) and
oracle_frustum_points."""
import ctypes

import numpy as np
import pytest

import oracle_lib
import plvi
import test_ba_window as tb
import test_feature_refresh as tf
import util


def ascending_lists(pool):
    """The lists of a pool in ascending slot order: the iteration order of the reference's std::map."""
    pool = dict(pool)
    kf, idx = pool["obs_kf"].copy(), pool["obs_idx"].copy()
    off = pool["obs_off"]
    for i in range(len(pool["bad"])):
        o = np.argsort(kf[off[i]:off[i + 1]], kind="stable")
        kf[off[i]:off[i + 1]], idx[off[i]:off[i + 1]] = kf[off[i]:off[i + 1]][o], idx[off[i]:off[i + 1]][o]
    pool.update(obs_kf=kf, obs_idx=idx)
    return pool


@pytest.mark.gpu
def test_gpu_chain_ba_window_refresh_frustum(plvi_lib):
    (kf, pool, kf_map), q = tb.shape_map(tb.POINTS, n_kf=12, cap=64, feats_per_kf=60)
    pool = ascending_lists(pool)
    tabs = (kf, pool, kf_map)
    K, cap, n = len(kf["bad"]), kf["mp"].shape[1], len(pool["bad"])
    rng = np.random.default_rng(31)
    prm = util.frustum_params(60)
    world = util.frustum_case(70, prm, n=n)
    O = np.array(prm.cam[0].O[:], np.float32)

    # A: the window's features, left on the device
    caps = dict(tb.big_caps(tabs), feat_cap=n + 7)
    win = tb.window(tabs, tb.POINTS, 25)
    got = win.batch([q], [50], fill=tb.FILL, **caps)
    assert got["rc"] == 0 and tb.plain(got, 0) == tb.ref_window(tabs, tb.POINTS, q, 50, max_opt=25, caps=caps)
    n_lf, feat_cap = int(got["n_local_feat"][0]), caps["feat_cap"]
    assert 50 < n_lf < feat_cap                    # the cells past the list hold the fill: ids outside the pool
    d_lf = got["keep"][1]["local_feat"].ptr

    # B: refresh those ids in the resident pool
    rkf = dict(bad=kf["bad"], ow=(O + rng.normal(0, 0.7, (K, 3))).astype(np.float32), cnt=kf["nmp"],
               info=(kf["kp_info"] & 0xc0) | rng.integers(0, 8, (K, cap)).astype(np.uint8),
               desc=rng.integers(0, 256, (K, cap, 32), dtype=np.uint8))
    feat = dict(bad=pool["bad"], obs_off=pool["obs_off"], obs_kf=pool["obs_kf"], obs_idx=pool["obs_idx"],
                ref_kf=pool["obs_kf"][np.minimum(pool["obs_off"][:-1], len(pool["obs_kf"]) - 1)].copy(),
                pos=world["pos"], normal=world["normal"].copy(), dist=world["dist"].copy(),
                desc=np.full((n, 32), tf.S_DESC, np.uint8))
    scale = util.orb_scale_factors()[:8]
    rtabs = (rkf, feat, scale)
    fr = plvi.FeatureRefresh(rkf, {k: a.copy() for k, a in feat.items()}, plvi.REFRESH_POINTS, scale)
    r = fr.batch(d_ids=d_lf, n_ids=feat_cap, row_cap=len(pool["obs_kf"]), fill=tf.FILL)
    ids = got["local_feat"][0][:feat_cap]
    exp = tf.ref_refresh(rtabs, tf.POINTS, ids)
    assert r["rc"] == 0
    tf.same(tf.plain(r), exp)
    assert int((exp["state"] == 3).sum()) > 50 and not exp["state"][n_lf:].any()

    # C: the frustum test reads the refreshed columns where they lie
    bufs = []

    def dev(a):
        a = np.ascontiguousarray(a)
        bufs.append(plvi.DeviceBuffer(max(a.nbytes, 4)))
        bufs[-1].upload(a)
        return ctypes.c_void_p(bufs[-1].ptr)
    V = ctypes.c_void_p
    d_fl, d_pr, d_lv, d_de = dev(np.zeros(n, np.uint8)), dev(world["proj"]), dev(world["level"]), dev(world["depth"])
    d_prm = dev(np.frombuffer(bytes(prm), np.uint8))
    assert plvi_lib.plvi_frustum_points_batch(1, d_prm, V(fr.dev[("f", "pos")].ptr), V(r["dev"]["normal"]),
                                              V(r["dev"]["dist"]), dev(world["in_flags"]), dev(np.array([n], np.int32)),
                                              n, d_fl, d_pr, d_lv, None, None, d_de, None, None) == 0
    plvi_lib.plvi_device_synchronize()
    want = oracle_lib.frustum_points(prm, dict(world, normal=exp["normal"], dist=exp["dist"]))
    assert np.array_equal(plvi.download(d_fl.value, np.zeros(n, np.uint8)), want["flags"])
    assert plvi.download(d_pr.value, np.zeros((n, 4), np.float32)).tobytes() == want["proj"].tobytes()
    assert np.array_equal(plvi.download(d_lv.value, np.zeros(n, np.int32)), want["level"])
    assert plvi.download(d_de.value, np.zeros(n, np.float32)).tobytes() == want["depth"].tobytes()
    refreshed = ids[:n_lf][exp["state"][:n_lf] == 3]
    assert int(((want["flags"][refreshed] & 8) != 0).sum()) > 10     # refreshed features pass the test with the new values
    stale = oracle_lib.frustum_points(prm, world)
    assert not np.array_equal(stale["flags"], want["flags"])    # and the refresh is what decides it
