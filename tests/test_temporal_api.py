"""The temporal pass's ABI without a GPU: tpt_history_* / tpt_temporal (include/tpt.h)
as the ctypes layer, the library and the CLI declare them, and the properties of the
numpy restatement the GPU tests compare against (tests/temporal_ref.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

import tinypathtracer_amd as T
from tinypathtracer_amd import _lib

from tests.conftest import ROOT
from tests import temporal_ref as TR

EXE = os.path.join(ROOT, "tinypathtracer_amd", "tpt_render")


def test_temporal_struct_layouts(tmp_path):
    """ctypes mirrors vs the C compiler's layout of the new structs."""
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tpt.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu %zu %d %d\\n",'
                    'sizeof(tpt_temporal_params),sizeof(tpt_temporal_stats),'
                    'offsetof(tpt_temporal_params,normal_min),offsetof(tpt_temporal_params,max_history),'
                    'offsetof(tpt_temporal_params,flags),offsetof(tpt_temporal_stats,reprojected),'
                    'TPT_TEMPORAL_DEMODULATE,TPT_TEMPORAL_TILES);return 0;}')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    mine = [C.sizeof(_lib.TemporalParams), C.sizeof(_lib.TemporalStats), _lib.TemporalParams.normal_min.offset,
            _lib.TemporalParams.max_history.offset, _lib.TemporalParams.flags.offset,
            _lib.TemporalStats.reprojected.offset, _lib.TEMPORAL_DEMODULATE, _lib.TEMPORAL_TILES]
    assert sizes == mine
    assert sizes[:2] == [20, 16]


def test_temporal_symbols_exported():
    L = T.lib()
    sigs = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    for name in ("tpt_history_create", "tpt_history_reset", "tpt_temporal"):
        assert name in sigs
        assert getattr(L, name).restype is C.c_int
    assert "tpt_history_destroy" in sigs and L.tpt_history_destroy.restype is None
    assert len(sigs["tpt_temporal"][1]) == 10


def test_cli_usage_names_the_temporal_pass():
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 2
    assert "--temporal" in r.stderr and "--yaw" in r.stderr


def test_cli_refuses_temporal_with_progressive(tmp_path):
    """Progressive is already the exact accumulation of an unmoving camera."""
    scene = os.path.join(ROOT, "tests", "golden", "scenes", "box.gltf")
    r = subprocess.run([EXE, scene, "--frames", "2", "--temporal", "--progressive", "--out", str(tmp_path / "x")],
                       capture_output=True, text=True)
    assert r.returncode == 2
    assert "--temporal" in r.stderr and "--progressive" in r.stderr
    assert not list(tmp_path.iterdir())                    # nothing was rendered or written


def test_null_handles_fail_cleanly():
    """No device is needed to be refused: every call names what is missing."""
    L = T.lib()
    h = C.c_void_p()
    assert L.tpt_history_create(None, 4, 4, C.byref(h)) == 1           # TPT_ERR_INVALID_ARG
    assert b"scene" in L.tpt_last_error() and not h.value
    assert L.tpt_history_reset(None) == 1
    assert b"history" in L.tpt_last_error()
    L.tpt_history_destroy(None)                            # a no-op, like free
    cam = T.Camera(np.eye(4, dtype=np.float32).reshape(16), 0.8, 1.0).to_c()
    buf = np.full((4, 4, 3), -7.0, np.float32)
    z = np.zeros((4, 4), np.float32)
    m = np.zeros((4, 4), np.int32)
    g = _lib.Aov(buf.ctypes.data, buf.ctypes.data, z.ctypes.data, None, m.ctypes.data)
    p = _lib.TemporalParams(0.1, 0.1, 0.9, 32, _lib.TEMPORAL_DEMODULATE)
    st = _lib.TemporalStats()
    out = np.full((4, 4, 3), -7.0, np.float32)
    assert L.tpt_temporal(None, C.byref(cam), buf.ctypes.data, C.byref(g), C.byref(p), out.ctypes.data, None, None,
                          None, C.byref(st)) == 1
    assert b"history" in L.tpt_last_error()
    assert (out == -7.0).all()


def test_host_defaults_and_yaw():
    assert T.TEMPORAL_DEFAULTS == {"alpha": 0.1, "depth_tol": 0.1, "normal_min": 0.9, "max_history": 32,
                                   "demodulate": True}
    cam = T.Camera(TR.camera(10.0, (1.0, 2.0, 3.0))["c2w"], 0.8, 1.5)
    assert np.array_equal(cam.yawed(0.0).c2w, cam.c2w)
    turned = cam.yawed(5.0)
    # about its own origin and up axis: the same camera as a world yaw of 15 degrees at that origin
    assert np.abs(turned.c2w - TR.camera(15.0, (1.0, 2.0, 3.0))["c2w"]).max() < 1e-6
    assert (turned.vfov, turned.aspect) == (cam.vfov, cam.aspect)


W, H = 37, 29
PARAMS = dict(alpha=0.1, depth_tol=0.1, normal_min=0.9, max_history=32)


def test_reference_properties():
    """The numpy restatement: a first frame is the input with N = 1 and variance 0; a
    static camera keeps the running mean; a disoccluded pixel starts over; history
    never crosses materials."""
    rng = np.random.default_rng(3)
    cam = TR.camera(aspect=W / H)
    aov = TR.synthetic_guides(cam, W, H)
    aov["albedo"] = rng.uniform(0.2, 1.0, (H, W, 3)).astype(np.float32)
    frames = [rng.uniform(0.0, 2.0, (H, W, 3)).astype(np.float32) for _ in range(4)]
    for demodulate in (False, True):
        r = TR.temporal_ref(None, cam, frames[0], aov, demodulate=demodulate, **PARAMS)
        assert np.abs(r["out"] - frames[0]).max() < 1e-12
        assert (r["history_len"] == 1).all() and not r["reprojected"].any() and r["decidable"].all()
        assert np.abs(r["variance"]).max() < 1e-12
    state = None
    for f in frames:
        r = TR.temporal_ref(state, cam, f, aov, alpha=1 / 64, depth_tol=0.1, normal_min=0.9, max_history=64,
                            demodulate=False)
        state = r["state"]
    assert (r["history_len"] == 4).all() and r["decidable"].all()
    assert np.abs(r["out"] - np.mean([f.astype(np.float64) for f in frames], 0)).max() < 1e-12
    lum = np.stack([f.astype(np.float64) @ TR.LUMA for f in frames])
    assert np.abs(r["variance"] - lum.var(0)).max() < 1e-12
    # a moved camera: both branches, and the near strip's history stays on the near strip
    cam2 = TR.camera(0.0, (0.13, 0.05, 0.02), aspect=W / H)
    aov2 = TR.synthetic_guides(cam2, W, H)
    first = TR.temporal_ref(None, cam, frames[0], aov, demodulate=False, **PARAMS)
    other = frames[0].copy()
    other[aov["material"] == 1] += 1.0
    second = TR.temporal_ref(TR.temporal_ref(None, cam, other, aov, demodulate=False, **PARAMS)["state"], cam2,
                             frames[1], aov2, demodulate=False, **PARAMS)
    base = TR.temporal_ref(first["state"], cam2, frames[1], aov2, demodulate=False, **PARAMS)
    assert base["reprojected"].any() and (~base["reprojected"]).any()
    assert np.array_equal(base["out"][~base["reprojected"]], frames[1].astype(np.float64)[~base["reprojected"]])
    rest = aov2["material"] != 1
    assert np.array_equal(base["out"][rest], second["out"][rest])
    assert not np.array_equal(base["out"][~rest], second["out"][~rest])


def test_synthetic_cameras_are_decidable():
    """What the GPU tests rely on: for every camera they move to, at most 1 % of the
    pixels sit on a threshold, some are disoccluded, some reproject with a partial
    footprint, and about a fifth are misses."""
    a = W / H
    cam1 = TR.camera(aspect=a)
    aov1 = TR.synthetic_guides(cam1, W, H)
    assert 0.15 < (aov1["material"] < 0).mean() < 0.25
    assert all((aov1["material"] == k).any() for k in (0, 1, 2))
    rad = np.ones((H, W, 3), np.float32)
    first = TR.temporal_ref(None, cam1, rad, aov1, demodulate=False, **PARAMS)
    move = (0.13, 0.05, 0.02)
    for cam2 in (cam1, TR.camera(0.0, move, aspect=a), TR.camera(1.5, move, aspect=a), TR.camera(2.0, aspect=a)):
        aov2 = TR.synthetic_guides(cam2, W, H)
        r = TR.temporal_ref(first["state"], cam2, rad, aov2, demodulate=False, **PARAMS)
        assert (~r["decidable"]).mean() <= 0.01
        if cam2 is cam1:
            assert r["reprojected"].all()
        else:
            assert 0.01 < (~r["reprojected"]).mean() < 0.05
    third = TR.camera(3.0, (0.26, 0.10, 0.04), aspect=a)
    r3 = TR.temporal_ref(r["state"], third, rad, TR.synthetic_guides(third, W, H), demodulate=False, **PARAMS)
    assert (~r3["decidable"]).mean() <= 0.01
