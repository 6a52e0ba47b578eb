"""History clipping's ABI without a GPU: the symbols, the struct layouts as tpt.h, the ctypes layer
and tpt.hpp declare them, the CLI's options and the refusal of a null history."""
import ctypes as C
import os
import subprocess

import tinypathtracer_amd as T
from tinypathtracer_amd import _lib

from tests.conftest import ROOT


def test_clip_symbols_exported():
    L = T.lib()
    names = [n for n, _, _ in _lib.SIGNATURES]
    for name in ("tpt_history_set_clip", "tpt_history_clip_stats"):
        assert name in names
        assert getattr(L, name).restype is C.c_int
    assert set(T.CLIP_DEFAULTS) == {"radius", "gamma", "max_history"}
    assert 1 <= T.CLIP_DEFAULTS["radius"] <= 3 and T.CLIP_DEFAULTS["gamma"] > 0 and 1 <= T.CLIP_DEFAULTS["max_history"] <= 65536
    assert "CLIP_DEFAULTS" in T.__all__
    assert callable(T.History.set_clip) and callable(T.History.clip_stats)


def test_clip_struct_layouts(tmp_path):
    """ctypes mirrors vs the C compiler's layout; tpt.hpp compiles, and its defaults are Python's."""
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tpt.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n",'
                    'sizeof(tpt_clip_params),sizeof(tpt_clip_stats),'
                    'offsetof(tpt_clip_params,radius),offsetof(tpt_clip_params,gamma),'
                    'offsetof(tpt_clip_params,max_history),offsetof(tpt_clip_params,flags),'
                    'offsetof(tpt_clip_stats,box_ms),offsetof(tpt_clip_stats,boxed),'
                    'offsetof(tpt_clip_stats,clipped));return 0;}')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P, S = _lib.ClipParams, _lib.ClipStats
    mine = [C.sizeof(P), C.sizeof(S), P.radius.offset, P.gamma.offset, P.max_history.offset, P.flags.offset,
            S.box_ms.offset, S.boxed.offset, S.clipped.offset]
    assert sizes == mine
    assert sizes[:2] == [16, 24]
    # the structs the issue leaves alone keep their layout
    assert [C.sizeof(_lib.TemporalParams), C.sizeof(_lib.TemporalPathParams), C.sizeof(_lib.TemporalStats)] == [20, 24, 16]
    d = T.CLIP_DEFAULTS
    hpp = tmp_path / "hpp.cpp"
    hpp.write_text('#include "tpt.hpp"\n'
                   'static_assert(sizeof(tpt_clip_params) == 16 && sizeof(tpt_clip_stats) == 24, "layout");\n'
                   'static_assert(sizeof(tpt_temporal_params) == 20 && sizeof(tpt_temporal_stats) == 16, "layout");\n'
                   'int main() {\n'
                   '    const tpt_clip_params p = tpt::defaultClip();\n'
                   '    void (tpt::History::*set)(const tpt_clip_params*) = &tpt::History::setClip;\n'
                   '    tpt_clip_stats (tpt::History::*get)() const = &tpt::History::clipStats;\n'
                   '    (void)set; (void)get;\n'
                   f'    return p.radius == {d["radius"]} && p.gamma == {d["gamma"]!r}f && '
                   f'p.max_history == {d["max_history"]} && p.flags == 0 ? 0 : 1;\n'
                   '}\n')
    exe2 = tmp_path / "hpp"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(hpp), "-o", str(exe2),
                           "-L", os.path.join(ROOT, "tinypathtracer_amd"), "-ltpt",
                           "-Wl,-rpath," + os.path.join(ROOT, "tinypathtracer_amd")])
    assert subprocess.call([str(exe2)]) == 0


def test_cli_usage_names_clip_and_refuses_it_without_temporal():
    exe = os.path.join(ROOT, "tinypathtracer_amd", "tpt_render")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2
    for opt in ("--clip [GAMMA]", "--clip-radius R", "--clip-history N"):
        assert opt in r.stderr
    for opts in (["--clip"], ["--clip", "1.5"], ["--clip-radius", "2"], ["--clip-history", "8"]):
        r = subprocess.run([exe, "nothing.gltf"] + opts, capture_output=True, text=True)
        assert r.returncode == 2 and "--temporal" in r.stderr, (opts, r.stderr)


def test_clip_null_history_refused_without_device():
    L = T.lib()
    p = _lib.ClipParams(3, 1.0, 4, 0)
    st = _lib.ClipStats(-1.0, 77, 77)
    assert L.tpt_history_set_clip(None, C.byref(p)) == 1
    assert b"history" in L.tpt_last_error()
    assert L.tpt_history_set_clip(None, None) == 1
    assert L.tpt_history_clip_stats(None, C.byref(st)) == 1
    assert b"history" in L.tpt_last_error()
    assert (st.box_ms, st.boxed, st.clipped) == (-1.0, 77, 77)     # nothing written
