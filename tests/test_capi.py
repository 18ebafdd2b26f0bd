"""C-ABI library: loads on a CPU-only host and exports every declared symbol."""
import ctypes
import subprocess

import pytest

import plvi


def test_library_exports_every_header_symbol():
    lib = plvi.load()
    names = plvi.exported_symbols()
    assert "plvi_orb_extract" in names and "plvi_hamming_knn2_batch" in names
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    out = subprocess.run(["nm", "-D", "--defined-only", str(plvi.LIB_PATH)], capture_output=True, text=True).stdout
    for n in names:
        assert f" T {n}" in out, n


def test_signatures_are_the_header():
    """The ctypes signatures are parsed from the header: they cover every declared symbol, are what load() applied,
    and a few are pinned literally so that the parser is checked against something it did not produce."""
    V, I, S, F, C = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float, ctypes.c_char_p
    sig = plvi.signatures()
    assert sorted(sig) == plvi.exported_symbols()
    lib = plvi.load()
    for name, (args, res) in sig.items():
        fn = getattr(lib, name)
        assert (list(fn.argtypes), fn.restype) == (args, res), name
    assert sig["plvi_version"] == ([], C)
    assert sig["plvi_stereo_lines_scratch_bytes"] == ([I, I, I, I], S)
    assert sig["plvi_local_map_scratch_bytes"] == ([I, I, I, I], S)
    assert sig["plvi_orb_extract"] == ([V, V, I, I, S, I, I, V, V, I, V, V], I)
    args, res = sig["plvi_stereo_lines_batch"]
    assert len(args) == 24 and args[12] is F and args[16] is S and res is I
    assert [a for a in args if a not in (V, I)] == [F, S]
    assert sig["plvi_vocab_load_text"] == ([C, I, I, V], I)
    args, res = sig["plvi_kfdb_query_batch"]
    assert len(args) == 26 and set(args) == {V, I} and res is I


def test_signatures_refuse_a_type_outside_the_rule(tmp_path):
    txt = plvi.HEADER_PATH.read_text()
    old = "int plvi_image_bounds(const plvi_camera* cam,"
    assert txt.count(old) == 1
    bad = tmp_path / "plvi_frontend.h"
    bad.write_text(txt.replace(old, "int plvi_image_bounds(plvi_camera cam,"))
    with pytest.raises(RuntimeError, match="plvi_image_bounds"):
        plvi.signatures(bad)
    bad.write_text(txt.replace(old, "int plvi_image_bounds(int (*cam)(int),"))
    with pytest.raises(RuntimeError, match="plvi_image_bounds"):
        plvi.signatures(bad)
    bad.write_text(txt)
    assert plvi.signatures(bad) == plvi.signatures()


def test_library_contains_gfx950_code_only():
    out = subprocess.run(["strings", str(plvi.LIB_PATH)], capture_output=True, text=True).stdout
    assert "gfx950" in out


def test_version_and_no_device_does_not_crash():
    lib = plvi.load()
    assert b"gfx950" in lib.plvi_version()
    assert lib.plvi_device_count() >= 0


def test_keypoint_and_keyline_layouts():
    assert plvi.KEYPOINT_DTYPE.itemsize == 28  # cv::KeyPoint
    assert plvi.KEYLINE_DTYPE.itemsize == 68   # line_descriptor::KeyLine
