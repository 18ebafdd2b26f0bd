"""plvi.LoopWindow.host and .merge_host refuse a companion array of the wrong length with ValueError before the
library is entered (the C staging would read past the end of host memory), as tests/test_host_form_checks.py demands
of the other host forms.

A minimal map: 3 keyframes, 2 points.  The wrapper's call functions are replaced: the untouched tables must reach one
(so the refusals are the checks', not a broken fixture), a mutated table must not."""
import numpy as np
import pytest

import plvi
from plvi import _abi

K, N = 3, 2


class Reached(Exception):
    pass


def tables():
    kf = dict(bad=np.zeros(K, np.uint8), mp=np.full((K, 4), -1, np.int32), nmp=np.zeros(K, np.int32),
              cand=np.zeros((K, 2), np.int32), n_cand=np.zeros(K, np.int32))
    pool = dict(bad=np.zeros(N, np.uint8), pos=np.zeros((N, 3), np.float32), normal=np.zeros((N, 3), np.float32),
                dist=np.zeros((N, 2), np.float32), desc=np.zeros((N, 32), np.uint8))
    return kf, pool


# (group, table): the tables whose length another table fixes
COMPANIONS = [("kf", k) for k in ("mp", "nmp", "cand", "n_cand")] + \
             [("pool", k) for k in ("pos", "normal", "dist", "desc")]
MUTATIONS = {"short": lambda a: a[:-1], "long": lambda a: np.concatenate([a, a[:1]])}


def _params():
    for form in ("window", "merge"):
        yield pytest.param(form, None, None, None, id=f"{form}-valid")
        for g, k in COMPANIONS:
            for how in MUTATIONS:
                yield pytest.param(form, g, k, how, id=f"{form}-{g}-{k}-{how}")


def run(win, form):
    if form == "window":
        return win.host(plvi.LOOP_WIN_PROJ, 0, gather=("pos", "normal", "dist", "desc"))
    return win.merge_host(np.zeros(plvi.LOOP_WIN_MAX, np.int32), 1, -1, np.zeros((plvi.LOOP_BOW_WIN, 4), np.int32), 4)


@pytest.mark.parametrize("form, group, key, how", _params())
def test_host_form_checks_its_tables(monkeypatch, form, group, key, how):
    plvi.load()
    kf, pool = tables()
    if group == "kf":
        kf[key] = MUTATIONS[how](kf[key])
    elif group == "pool":
        pool[key] = MUTATIONS[how](pool[key])
    win = plvi.LoopWindow(kf, pool)

    def entered(entry, *args):
        if group is None:
            raise Reached(entry)
        pytest.fail(f"{entry} entered with {group}.{key} {how}")
    for mod, attr in ((plvi, "_call"), (plvi, "_status"), (_abi, "call"), (_abi, "status")):
        monkeypatch.setattr(mod, attr, entered)
    if group is None:
        with pytest.raises(Reached):
            run(win, form)
        return
    with pytest.raises(ValueError):
        run(win, form)


@pytest.mark.parametrize("what", ("win", "matches12", "connected"))
def test_host_form_checks_its_per_query_arrays(monkeypatch, what):
    plvi.load()
    win = plvi.LoopWindow(*tables())

    def entered(entry, *args):
        pytest.fail(f"{entry} entered with a wrong {what}")
    for mod, attr in ((plvi, "_call"), (plvi, "_status"), (_abi, "call"), (_abi, "status")):
        monkeypatch.setattr(mod, attr, entered)
    m12 = np.zeros((plvi.LOOP_BOW_WIN, 4), np.int32)
    with pytest.raises(ValueError):
        if what == "win":
            win.merge_host(np.zeros(plvi.LOOP_BOW_WIN, np.int32), 1, -1, m12, 4)
        elif what == "matches12":
            win.merge_host(np.zeros(plvi.LOOP_WIN_MAX, np.int32), 1, -1, m12[:5], 4)
        else:
            win.batch([plvi.LOOP_WIN_BOW] * 2, [0, 1], 0, connected=[[1]])
