"""plvi.LocalBAWindow.host refuses a companion array of the wrong length with ValueError before the library is
entered (the C staging would read past the end of host memory), as tests/test_host_form_checks.py demands of the
other host forms.

A minimal map: 3 keyframes, 2 points, 3 observations.  The wrapper's call functions are replaced: the untouched
tables must reach one (so the refusals are the checks', not a broken fixture), a mutated table must not."""
import numpy as np
import pytest

import plvi
from plvi import _abi

K, N, NOBS = 3, 2, 3


class Reached(Exception):
    pass


def tables():
    kf = dict(bad=np.zeros(K, np.uint8), init_kf=np.zeros(K, np.uint8), mp=np.full((K, 4), -1, np.int32),
              nmp=np.zeros(K, np.int32), kp_info=np.zeros((K, 4), np.uint8), cand=np.zeros((K, 2), np.int32),
              n_cand=np.zeros(K, np.int32), kf_id=np.arange(1, K + 1, dtype=np.uint32),
              prev_kf=np.full(K, -1, np.int32))
    pool = dict(bad=np.zeros(N, np.uint8), obs_off=np.array([0, 2, 3], np.int32), obs_kf=np.zeros(NOBS, np.int32),
                obs_idx=np.zeros(NOBS, np.int32), map_id=np.zeros(N, np.int32))
    return kf, pool, np.zeros(K, np.int32)


# (group, table): the tables whose length another table fixes
COMPANIONS = [("kf", k) for k in ("init_kf", "mp", "nmp", "kp_info", "cand", "n_cand", "kf_id", "prev_kf")] + \
             [("kf_map_id", None)] + [("pool", k) for k in ("obs_off", "obs_idx", "map_id")]
MUTATIONS = {"short": lambda a: a[:-1], "long": lambda a: np.concatenate([a, a[:1]])}


LINE_NAMES = {"mp": "ml", "nmp": "nml"}


def _params():
    for mode, name in ((plvi.BA_POINTS, "points"), (plvi.BA_LINES, "lines"), (plvi.BA_INERTIAL, "inertial")):
        yield pytest.param(mode, None, None, None, id=f"{name}-valid")
        for g, k in COMPANIONS:
            if mode == plvi.BA_LINES and k == "kp_info":
                continue     # the lines mode has no such table
            k = LINE_NAMES.get(k, k) if mode == plvi.BA_LINES else k
            for how in MUTATIONS:
                yield pytest.param(mode, g, k, how, id=f"{name}-{g}-{k}-{how}")


@pytest.mark.parametrize("mode, group, key, how", _params())
def test_host_form_checks_its_tables(monkeypatch, mode, group, key, how):
    plvi.load()
    kf, pool, kf_map = tables()
    if mode == plvi.BA_LINES:
        kf["ml"], kf["nml"] = kf.pop("mp"), kf.pop("nmp")
        del kf["kp_info"]
    if group == "kf":
        kf[key] = MUTATIONS[how](kf[key])
    elif group == "kf_map_id":
        kf_map = MUTATIONS[how](kf_map)
    elif group == "pool":
        pool[key] = MUTATIONS[how](pool[key])
    win = plvi.LocalBAWindow(kf, None if mode == plvi.BA_LINES else pool, pool if mode == plvi.BA_LINES else None,
                             mode=mode, kf_map_id=kf_map)

    def entered(entry, *args):
        if group is None:
            raise Reached(entry)
        pytest.fail(f"{entry} entered with {group}.{key} {how}")
    for mod, attr in ((plvi, "_call"), (plvi, "_status"), (_abi, "call"), (_abi, "status")):
        monkeypatch.setattr(mod, attr, entered)
    if group is None:
        with pytest.raises(Reached):
            win.host(0, 5)
        return
    with pytest.raises(ValueError):
        win.host(0, 5)
