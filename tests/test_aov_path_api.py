"""tpt_render_aov_path's ABI without a GPU: the symbol, the struct layouts as tpt.h,
the ctypes layer and tpt.hpp declare them, and the refusal of a null scene."""
import ctypes as C
import os
import subprocess

import numpy as np

import tinypathtracer_amd as T
from tinypathtracer_amd import _lib

from tests.conftest import ROOT


def test_aov_path_symbol_exported():
    L = T.lib()
    names = [n for n, _, _ in _lib.SIGNATURES]
    assert "tpt_render_aov_path" in names
    assert L.tpt_render_aov_path.restype is C.c_int
    assert T.AOV_PATH_DEFAULTS == {"max_bounces": 8}


def test_aov_path_struct_layouts(tmp_path):
    """ctypes mirrors vs the C compiler's layout; tpt.hpp's static_assert compiles."""
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tpt.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu\\n",'
                    'sizeof(tpt_aov_path_params),sizeof(tpt_aov_path_stats),'
                    'offsetof(tpt_aov_path_params,flags),offsetof(tpt_aov_path_stats,followed),'
                    'offsetof(tpt_aov_path_stats,deepest));return 0;}')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    mine = [C.sizeof(_lib.AovPathParams), C.sizeof(_lib.AovPathStats), _lib.AovPathParams.flags.offset,
            _lib.AovPathStats.followed.offset, _lib.AovPathStats.deepest.offset]
    assert sizes == mine
    assert sizes[:2] == [8, 24]
    hpp = tmp_path / "hpp.cpp"
    hpp.write_text('#include "tpt.hpp"\n'
                   'static_assert(sizeof(tpt_aov_path_params) == 8 && sizeof(tpt_aov_path_stats) == 24, "layout");\n'
                   'int main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(hpp)])


def test_cli_usage_names_aov_path():
    exe = os.path.join(ROOT, "tinypathtracer_amd", "tpt_render")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2
    assert "--aov-path" in r.stderr


def test_aov_path_null_scene_refused_without_device():
    L = T.lib()
    cam = T.Camera(np.eye(4, dtype=np.float32).T.reshape(16), 0.8, 1.5).to_c()
    z = np.full((4, 4), -7.0, np.float32)
    k = np.full((4, 4), -77, np.int32)
    a = _lib.Aov(None, None, z.ctypes.data, None, None)
    p = _lib.AovPathParams(8, 0)
    st = _lib.AovPathStats()
    rc = L.tpt_render_aov_path(None, C.byref(cam), 4, 4, C.byref(p), C.byref(a), k.ctypes.data, C.byref(st))
    assert rc == 1                                         # TPT_ERR_INVALID_ARG
    assert b"scene not built" in L.tpt_last_error()
    assert (z == -7.0).all() and (k == -77).all()


def test_host_checks_the_bounces_plane():
    import pytest
    with pytest.raises(ValueError):
        T._check_plane("bounces", np.zeros((4, 4), np.float32), 4, 4)
    T._check_plane("bounces", np.zeros((3, 5), np.int32), 5, 3)
