"""The BVH refit without a GPU: the new symbols as the library, the ctypes layer, the hosts and the
CLI declare them, and the refusals that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np

import tinypathtracer_amd as T
from tinypathtracer_amd import _lib

from tests.conftest import ROOT, scene_path

EXE = os.path.join(ROOT, "tinypathtracer_amd", "tpt_render")
BOX = scene_path("box")


def test_symbols_exported():
    L = T.lib()
    sigs = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    assert len(sigs["tpt_scene_refit"][1]) == 2 and L.tpt_scene_refit.restype is C.c_int
    assert len(sigs["tpt_scene_read_wide"][1]) == 5 and L.tpt_scene_read_wide.restype is C.c_int
    assert len(sigs["tpt_wide_tree_levels"][1]) == 5 and L.tpt_wide_tree_levels.restype is C.c_int32
    assert [f for f, _ in _lib.RefitStats._fields_] == ["rebuilt", "launches", "slivers", "cull_eps", "ms", "cost",
                                                        "cost_built"]
    assert C.sizeof(_lib.RefitStats) == 40                  # 3 x int32, float, 3 x double
    assert hasattr(T.DeviceScene, "refit") and hasattr(T.DeviceScene, "read_wide")


def test_headers_say_what_exists_and_what_does_not():
    header = open(os.path.join(ROOT, "include", "tpt.h")).read()
    hpp = open(os.path.join(ROOT, "include", "tpt.hpp")).read()
    assert "tpt_scene_refit(" in header and "tpt_scene_read_wide(" in header and "tpt_wide_tree_levels(" in header
    assert "typedef struct tpt_refit_stats" in header
    for field in ("rebuilt", "launches", "slivers", "cull_eps", "cost_built"):
        assert field in header
    assert "a full rebuild, not a" not in header and "rebuild, not a refit" not in header
    flat = " ".join(header.split())
    assert "dirty-subtree" in flat and "re-sorting" in flat and "topology changes" in flat   # what still does not exist
    assert "bit-equal closest t" in flat                   # the documented difference from a rebuild
    assert "stale" in flat                                  # the Morton keys after a refit
    assert "refit(tpt_refit_stats* stats = nullptr)" in hpp and "tpt_scene_refit(" in hpp
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "tpt_scene_refit" in text and "a rebuild, not a refit" not in text, doc


def test_null_scene_fails_cleanly():
    """No device is needed to be refused."""
    L = T.lib()
    st = _lib.RefitStats()
    assert L.tpt_scene_refit(None, C.byref(st)) == 1
    assert b"scene" in L.tpt_last_error()
    assert L.tpt_scene_refit(None, None) == 1
    nm, ne = C.c_int32(-5), C.c_int32(-5)
    buf = np.full(32, -7.0, np.float32)
    assert L.tpt_scene_read_wide(None, buf.ctypes.data, 1, C.byref(nm), C.byref(ne)) == 1
    assert b"scene" in L.tpt_last_error()
    assert (buf == -7.0).all() and nm.value == -5 and ne.value == -5


def test_cli_usage_names_refit():
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 2
    assert "[--refit]" in r.stderr and "--wave OBJ AMP" in r.stderr


def test_cli_refuses_refit_without_motion(tmp_path):
    """--refit with nothing that moves is refused before anything is loaded or rendered."""
    r = subprocess.run([EXE, BOX, "--out", str(tmp_path / "x"), "--frames", "4", "--temporal", "--refit"],
                       capture_output=True, text=True)
    assert r.returncode == 2
    assert "--refit" in r.stderr and "--wave" in r.stderr
    assert not list(tmp_path.iterdir())
