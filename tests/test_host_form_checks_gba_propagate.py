"""plvi.GBAPropagation refuses a companion array of the wrong length, a CSR given in part, a negative size, an unknown
kind and a short scratch block with ValueError before the library is entered (the C staging would read past the end
of host memory), as tests/test_host_form_checks.py demands of the other host forms.

A minimal map: 4 keyframes in a chain, 3 features of each kind.  The wrapper's call functions are replaced: the
untouched tables must reach one (so the refusals are the checks', not a broken fixture), a mutated table must not."""
import numpy as np
import pytest

import plvi
from plvi import _abi

K, N = 4, 3
i32, u32, u8, f32, f64 = np.int32, np.uint32, np.uint8, np.float32, np.float64


class Reached(Exception):
    pass


def tables():
    kf = dict(bad=np.zeros(K, u8), kf_ba_for=np.zeros(K, u32), order=np.arange(K, dtype=i32),
              child_off=np.array([0, 1, 2, 3, 3], i32), child=np.array([1, 2, 3], i32))
    pools = []
    for w, dt in ((3, f32), (6, f64)):
        pools.append(dict(bad=np.zeros(N, u8), ref_kf=np.zeros(N, i32), map_id=np.zeros(N, i32), ba_for=np.zeros(N, u32),
                          pos_gba=np.ones((N, w), dt), **{"pos" if w == 3 else "sep": np.ones((N, w), dt)}))
    poses = dict(has_bef=np.ones(K, u8), tcw_bef=np.zeros((K, 12), f32), twc=np.zeros((K, 12), f32))
    return kf, pools, poses


MUTATIONS = {"short": lambda a: a[:-1], "long": lambda a: np.concatenate([a, a[:1]])}
WALK = ("kf_ba_for", "child_off", "child")
CORRECT = [("feat", k) for k in ("ref_kf", "map_id", "ba_for", "pos_gba", "where")] + \
          [("poses", k) for k in ("has_bef", "tcw_bef", "twc")]


def patch(monkeypatch, entered):
    for mod, attr in ((plvi, "_call"), (plvi, "_status"), (_abi, "call"), (_abi, "status")):
        monkeypatch.setattr(mod, attr, entered)


def run(monkeypatch, fn, valid):
    def entered(entry, *args):
        if valid:
            raise Reached(entry)
        pytest.fail(f"{entry} entered")
    patch(monkeypatch, entered)
    with pytest.raises(Reached if valid else ValueError):
        fn()


@pytest.mark.parametrize("key, how", [(None, None)] + [(k, h) for k in WALK for h in MUTATIONS])
def test_walk_host_form_checks_its_tables(monkeypatch, key, how):
    plvi.load()
    kf, pools, _ = tables()
    if key is not None:
        kf[key] = MUTATIONS[how](kf[key])
    g = plvi.GBAPropagation(kf, *pools)
    run(monkeypatch, lambda: g.walk.host([0], 5), key is None)


@pytest.mark.parametrize("what", ("child_off-alone", "child-alone", "walk_cap-negative", "visited-short",
                                  "no-stamps", "no-keyframes"))
def test_walk_host_form_checks_the_rest(monkeypatch, what):
    plvi.load()
    kf, pools, _ = tables()
    kw = {}
    if what == "child_off-alone":
        del kf["child"]
    if what == "child-alone":
        del kf["child_off"]
    if what == "walk_cap-negative":
        kw["walk_cap"] = -1
    if what == "visited-short":
        kw["visited"] = np.zeros(K - 1, u8)
    if what == "no-stamps":
        del kf["kf_ba_for"]
    if what == "no-keyframes":
        kf = {k: a[:0] for k, a in kf.items()}
    g = plvi.GBAPropagation(kf, *pools)
    run(monkeypatch, lambda: g.walk.host([0], 5, **kw), False)


def test_walk_batch_refuses_a_short_scratch_block(monkeypatch):
    lib = plvi.load()
    kf, pools, _ = tables()
    g = plvi.GBAPropagation(kf, *pools)
    sb = lib.plvi_gba_walk_scratch_bytes(K)
    assert sb > 0
    run(monkeypatch, lambda: g.walk.batch([0], 5, scratch=(0x1000, sb - 1)), False)


def _correct_params():
    for kind in (plvi.GBA_POINTS, plvi.GBA_LINES):
        yield pytest.param(kind, None, None, None, id=f"{kind}-valid")
        for grp, k in CORRECT:
            for how in MUTATIONS:
                yield pytest.param(kind, grp, k, how, id=f"{kind}-{grp}-{k}-{how}")


@pytest.mark.parametrize("kind, group, key, how", _correct_params())
def test_correct_host_form_checks_its_tables(monkeypatch, kind, group, key, how):
    plvi.load()
    kf, pools, poses = tables()
    if group is not None:
        d = poses if group == "poses" else pools[kind]
        key = ("sep" if kind == plvi.GBA_LINES else "pos") if key == "where" else key
        d[key] = MUTATIONS[how](d[key])
    g = plvi.GBAPropagation(kf, *pools)
    run(monkeypatch, lambda: g.correct.host(kind, 5, poses), group is None)


@pytest.mark.parametrize("what", ("kind-2", "kind-negative", "no-pool", "column-short", "poses-lack-twc",
                                  "pose-rows-of-16"))
def test_correct_host_form_checks_the_rest(monkeypatch, what):
    plvi.load()
    kf, pools, poses = tables()
    kind, kw = plvi.GBA_POINTS, {}
    if what == "kind-2":
        kind = 2
    if what == "kind-negative":
        kind = -1
    if what == "no-pool":
        pools[1], kind = None, plvi.GBA_LINES
    if what == "column-short":
        kw["column"] = np.zeros((N - 1, 3), f32)
    if what == "poses-lack-twc":
        del poses["twc"]
    if what == "pose-rows-of-16":
        poses["twc"] = np.zeros((K, 16), f32)
    g = plvi.GBAPropagation(kf, *pools)
    run(monkeypatch, lambda: g.correct.host(kind, 5, poses, **kw), False)
