"""plvi.FeatureRefresh.host refuses a companion array of the wrong length with ValueError before the library is
entered (the C staging would read past the end of host memory), as tests/test_host_form_checks.py demands of the
other host forms.

A minimal map: 3 keyframes with rows of 4, 2 features.  The wrapper's call functions are replaced: the untouched
tables must reach one (so the refusals are the checks', not a broken fixture), a mutated table must not."""
import numpy as np
import pytest

import plvi
from plvi import _abi

K, CAP, N = 3, 4, 2
i32, f32 = np.int32, np.float32


class Reached(Exception):
    pass


def tables(kind):
    kf = dict(bad=np.zeros(K, np.uint8), ow=np.zeros((K, 3), f32), cnt=np.full(K, CAP, i32),
              info=np.zeros((K, CAP), np.uint8), desc=np.zeros((K, CAP, 32), np.uint8))
    feat = dict(bad=np.zeros(N, np.uint8), obs_off=np.array([0, 2, 3], i32), obs_kf=np.array([0, 1, 2], i32),
                obs_idx=np.array([1, 0, 3], i32), ref_kf=np.zeros(N, i32), normal=np.zeros((N, 3), f32),
                dist=np.zeros((N, 2), f32), desc=np.zeros((N, 32), np.uint8))
    feat["sep" if kind == plvi.REFRESH_LINES else "pos"] = np.ones((N, 6 if kind == plvi.REFRESH_LINES else 3))
    return kf, feat


COMPANIONS = [("kf", k) for k in ("ow", "cnt", "info", "desc")] + \
             [("feat", k) for k in ("obs_off", "obs_idx", "ref_kf", "normal", "dist", "desc", "where")]
MUTATIONS = {"short": lambda a: a[:-1], "long": lambda a: np.concatenate([a, a[:1]])}


def _params():
    for kind in (plvi.REFRESH_POINTS, plvi.REFRESH_LINES):
        yield pytest.param(kind, None, None, None, id=f"{kind}-valid")
        for g, k in COMPANIONS:
            for how in MUTATIONS:
                yield pytest.param(kind, g, k, how, id=f"{kind}-{g}-{k}-{how}")


def patch(monkeypatch, entered):
    for mod, attr in ((plvi, "_call"), (plvi, "_status"), (_abi, "call"), (_abi, "status")):
        monkeypatch.setattr(mod, attr, entered)


@pytest.mark.parametrize("kind, group, key, how", _params())
def test_host_form_checks_its_tables(monkeypatch, kind, group, key, how):
    plvi.load()
    kf, feat = tables(kind)
    if group is not None:
        d = kf if group == "kf" else feat
        key = ("sep" if kind == plvi.REFRESH_LINES else "pos") if key == "where" else key
        d[key] = MUTATIONS[how](d[key])
    fr = plvi.FeatureRefresh(kf, feat, kind, scale=[1.0, 1.2])

    def entered(entry, *args):
        if group is None:
            raise Reached(entry)
        pytest.fail(f"{entry} entered with {group}.{key} {how}")
    patch(monkeypatch, entered)
    with pytest.raises(Reached if group is None else ValueError):
        fr.host([0, 1])


@pytest.mark.parametrize("what", ("obs_kf-short", "info-rows", "no-levels", "too-many-levels"))
def test_host_form_checks_the_rest(monkeypatch, what):
    plvi.load()
    kf, feat = tables(plvi.REFRESH_POINTS)
    scale = [1.0, 1.2]
    if what == "obs_kf-short":
        feat["obs_kf"], feat["obs_idx"] = feat["obs_kf"][:2], feat["obs_idx"][:2]
    if what == "info-rows":
        kf["info"] = np.zeros((K, CAP + 1), np.uint8)
    if what == "no-levels":
        scale = []
    if what == "too-many-levels":
        scale = [1.0] * 65

    def entered(entry, *args):
        pytest.fail(f"{entry} entered with {what}")
    patch(monkeypatch, entered)
    with pytest.raises(ValueError):
        plvi.FeatureRefresh(kf, feat, plvi.REFRESH_POINTS, scale=scale, cap=CAP).host([0, 1])
