"""The post-pass ABI without a GPU: tpt_render_aov / tpt_denoise (include/tpt.h) as
the ctypes layer, the library and the CLI declare them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tinypathtracer_amd as T
from tinypathtracer_amd import _lib

from tests.conftest import ROOT
from tests import post_ref as R


def test_post_struct_layouts(tmp_path):
    """ctypes mirrors vs the C compiler's layout of the new structs."""
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tpt.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu %zu %d %d\\n",'
                    'sizeof(tpt_aov),sizeof(tpt_denoise_params),sizeof(tpt_denoise_stats),'
                    'offsetof(tpt_aov,material),offsetof(tpt_denoise_params,flags),'
                    'offsetof(tpt_denoise_stats,resolve_ms),TPT_DENOISE_DEMODULATE,TPT_DENOISE_DIRECT);return 0;}')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    mine = [C.sizeof(_lib.Aov), C.sizeof(_lib.DenoiseParams), C.sizeof(_lib.DenoiseStats), _lib.Aov.material.offset,
            _lib.DenoiseParams.flags.offset, _lib.DenoiseStats.resolve_ms.offset, _lib.DENOISE_DEMODULATE,
            _lib.DENOISE_DIRECT]
    assert sizes == mine
    assert sizes[:3] == [40, 20, 24]


def test_post_symbols_exported():
    L = T.lib()
    names = [n for n, _, _ in _lib.SIGNATURES]
    for name in ("tpt_render_aov", "tpt_denoise"):
        assert name in names
        assert getattr(L, name).restype is C.c_int


def test_cli_usage_names_the_post_pass():
    exe = os.path.join(ROOT, "tinypathtracer_amd", "tpt_render")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2
    assert "--aov" in r.stderr and "--denoise" in r.stderr


def test_post_without_device_fails_cleanly():
    """No scene can exist without a device: both calls return a status and a message."""
    if T.device_count() > 0:
        pytest.skip("a HIP device is visible")
    L = T.lib()
    cam = T.Camera(np.eye(4, dtype=np.float32).T.reshape(16), 0.8, 1.5).to_c()
    buf = np.zeros((4, 4, 3), np.float32)
    z = np.zeros((4, 4), np.float32)
    a = _lib.Aov(buf.ctypes.data, buf.ctypes.data, z.ctypes.data, None, None)
    ms = C.c_double()
    assert L.tpt_render_aov(None, C.byref(cam), 4, 4, C.byref(a), C.byref(ms)) == 1   # TPT_ERR_INVALID_ARG
    assert b"scene not built" in L.tpt_last_error()
    p = _lib.DenoiseParams(1, 1.0, 1.0, 1.0, 0)
    st = _lib.DenoiseStats()
    out = np.zeros_like(buf)
    assert L.tpt_denoise(None, 4, 4, buf.ctypes.data, C.byref(a), C.byref(p), out.ctypes.data, None,
                         C.byref(st)) == 1
    assert b"null scene" in L.tpt_last_error()
    with pytest.raises(T.TPTError) as e:
        T.Scene(os.path.join(ROOT, "tests", "golden", "scenes", "tir.gltf")).copySceneToDevice(0)
    assert e.value.status == 6                             # TPT_ERR_NO_DEVICE


def test_host_checks_buffer_shapes():
    """The Python host refuses buffers of the wrong size or type before the library sees them."""
    with pytest.raises(ValueError):
        T._check_plane("depth", np.zeros((4, 4), np.float64), 4, 4)
    with pytest.raises(ValueError):
        T._check_plane("albedo", np.zeros((4, 4), np.float32), 4, 4)
    T._check_plane("face", np.zeros((3, 5), np.int32), 5, 3)


def test_reference_filter_properties():
    """The numpy restatement the GPU tests compare against: a constant image is a
    fixed point, iterations 0 is the identity, and a miss block filters among itself."""
    rng = np.random.default_rng(3)
    H, W = 12, 17
    n = rng.normal(size=(H, W, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    z = rng.uniform(1, 5, (H, W))
    alb = rng.uniform(0.1, 1, (H, W, 3))
    const = np.full((H, W, 3), 0.7)
    out = R.atrous_ref(const, alb, n, z, 3, 0.6, 0.3, 0.05, False)
    assert np.abs(out - 0.7).max() < 1e-12
    c = rng.uniform(0, 2, (H, W, 3))
    assert np.array_equal(R.atrous_ref(c, alb, n, z, 0, 0.6, 0.3, 0.05, True), c)
    n[:4, :5] = 0
    z[:4, :5] = 0                                          # a block of misses: z differs from every hit by >= 1
    c2 = c.copy()
    c2[4:, :] += 1.0
    c2[:, 5:] += 1.0
    a = R.atrous_ref(c, alb, n, z, 2, 0.6, 0.3, 0.05, False)
    b = R.atrous_ref(c2, alb, n, z, 2, 0.6, 0.3, 0.05, False)
    assert np.array_equal(a[:4, :5], b[:4, :5])            # exp(-1 / (0.05^2 1e-12)) is 0
