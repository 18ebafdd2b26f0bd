"""plvi.EssentialGraph.correct_host and .graph_host refuse a companion array of the wrong length with ValueError
before the library is entered (the C staging would read past the end of host memory), as tests/test_host_form_checks.py
demands of the other host forms.

A minimal map: 3 keyframes, 2 points, 2 lines.  The wrapper's call functions are replaced: the untouched tables must
reach one (so the refusals are the checks', not a broken fixture), a mutated table must not."""
import numpy as np
import pytest

import plvi
from plvi import _abi

K, N = 3, 2
i32 = np.int32


class Reached(Exception):
    pass


def tables():
    kf = dict(bad=np.zeros(K, np.uint8), init_kf=np.zeros(K, np.uint8), mp=np.full((K, 4), -1, i32), nmp=np.zeros(K, i32),
              ml=np.full((K, 3), -1, i32), nml=np.zeros(K, i32), cand=np.zeros((K, 2), i32), n_cand=np.zeros(K, i32),
              kf_id=np.arange(K, dtype=np.uint32), prev_kf=np.full(K, -1, i32), next_kf=np.full(K, -1, i32),
              order=np.arange(K, dtype=i32), map_id=np.zeros(K, i32), parent=np.full(K, -1, i32),
              child_off=np.array([0, 1, 1, 1], i32), child=np.array([1], i32), loop_off=np.array([0, 0, 1, 1], i32),
              loop=np.array([0], i32), imu=np.zeros(K, np.uint8), cand_w=np.zeros((K, 2), i32),
              map_kf=np.zeros((K, 2), i32), map_w=np.zeros((K, 2), i32), map_n=np.zeros(K, i32))
    pool = lambda: dict(bad=np.zeros(N, np.uint8), ref_kf=np.zeros(N, i32), corr_by=np.zeros(N, np.uint32),  # noqa: E731
                        corr_ref=np.zeros(N, i32), map_id=np.zeros(N, i32))
    return kf, pool(), pool()


# (group, table): the tables whose length another table fixes
COMPANIONS = [("kf", k) for k in ("init_kf", "mp", "nmp", "ml", "nml", "cand", "n_cand", "kf_id", "prev_kf", "next_kf",
                                  "map_id", "parent", "child_off", "child", "loop_off", "loop", "imu", "cand_w",
                                  "map_kf", "map_w", "map_n")] + \
             [(g, k) for g in ("points", "lines") for k in ("ref_kf", "corr_by", "corr_ref", "map_id")]
MUTATIONS = {"short": lambda a: a[:-1], "long": lambda a: np.concatenate([a, a[:1]])}


def _params():
    for form in ("correct", "graph"):
        yield pytest.param(form, None, None, None, id=f"{form}-valid")
        for g, k in COMPANIONS:
            for how in MUTATIONS:
                yield pytest.param(form, g, k, how, id=f"{form}-{g}-{k}-{how}")


def run(g, form):
    if form == "correct":
        return g.correct_host(0)
    return g.graph_host(0, 1, plvi.EG_7DOF, np.array([1, 0], i32), None, np.zeros((2, 3), i32), np.zeros(2, i32))


def patch(monkeypatch, entered):
    for mod, attr in ((plvi, "_call"), (plvi, "_status"), (_abi, "call"), (_abi, "status")):
        monkeypatch.setattr(mod, attr, entered)


@pytest.mark.parametrize("form, group, key, how", _params())
def test_host_form_checks_its_tables(monkeypatch, form, group, key, how):
    plvi.load()
    kf, points, lines = tables()
    if group is not None:
        d = {"kf": kf, "points": points, "lines": lines}[group]
        d[key] = MUTATIONS[how](d[key])
    g = plvi.EssentialGraph(kf, points, lines)

    def entered(entry, *args):
        if group is None:
            raise Reached(entry)
        pytest.fail(f"{entry} entered with {group}.{key} {how}")
    patch(monkeypatch, entered)
    with pytest.raises(Reached if group is None else ValueError):
        run(g, form)


@pytest.mark.parametrize("what", ("lc_kf-rows", "n_lc", "lc_kf-flat", "stamps-in-part", "csr-in-part"))
def test_host_form_checks_its_per_call_arrays(monkeypatch, what):
    plvi.load()
    kf, points, lines = tables()
    if what == "stamps-in-part":
        del points["corr_ref"]
    if what == "csr-in-part":
        del kf["loop"]
    g = plvi.EssentialGraph(kf, points, lines)

    def entered(entry, *args):
        pytest.fail(f"{entry} entered with a wrong {what}")
    patch(monkeypatch, entered)
    win = np.array([1, 0], i32)
    with pytest.raises(ValueError):
        if what == "lc_kf-rows":
            g.graph_host(0, 1, plvi.EG_4DOF, win, None, np.zeros((3, 3), i32), np.zeros(2, i32))
        elif what == "n_lc":
            g.graph_host(0, 1, plvi.EG_4DOF, win, None, np.zeros((2, 3), i32), np.zeros(3, i32))
        elif what == "lc_kf-flat":
            g.graph_host(0, 1, plvi.EG_4DOF, win, None, np.zeros(6, i32), np.zeros(2, i32))
        else:
            g.correct_host(0)
