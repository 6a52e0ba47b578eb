"""The variance-guided filter's ABI without a GPU: tpt_denoise_svgf (include/tpt.h) as
the ctypes layer, the library, the hosts and the CLI declare it, and the properties of
the numpy restatement the GPU tests compare against (tests/svgf_ref.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tinypathtracer_amd as T
from tinypathtracer_amd import _lib

from tests.conftest import ROOT
from tests import post_ref as R
from tests import svgf_ref as SR

EXE = os.path.join(ROOT, "tinypathtracer_amd", "tpt_render")


def test_svgf_struct_layouts(tmp_path):
    """ctypes mirrors vs the C compiler's layout of the new structs."""
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tpt.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n",'
                    'sizeof(tpt_svgf_params),sizeof(tpt_svgf_stats),'
                    'offsetof(tpt_svgf_params,sigma_lum),offsetof(tpt_svgf_params,min_history),'
                    'offsetof(tpt_svgf_params,flags),offsetof(tpt_svgf_stats,estimate_ms),'
                    'offsetof(tpt_svgf_stats,resolve_ms),offsetof(tpt_svgf_stats,estimated),'
                    'TPT_SVGF_DEMODULATE,TPT_SVGF_DIRECT);return 0;}')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    mine = [C.sizeof(_lib.SvgfParams), C.sizeof(_lib.SvgfStats), _lib.SvgfParams.sigma_lum.offset,
            _lib.SvgfParams.min_history.offset, _lib.SvgfParams.flags.offset, _lib.SvgfStats.estimate_ms.offset,
            _lib.SvgfStats.resolve_ms.offset, _lib.SvgfStats.estimated.offset, _lib.SVGF_DEMODULATE,
            _lib.SVGF_DIRECT]
    assert sizes == mine
    assert sizes[:2] == [24, 40] and sizes[-2:] == [1, 2]


def test_svgf_symbol_exported():
    L = T.lib()
    sigs = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    assert "tpt_denoise_svgf" in sigs
    assert L.tpt_denoise_svgf.restype is C.c_int
    assert len(sigs["tpt_denoise_svgf"][1]) == 12


def test_cli_usage_names_svgf():
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 2
    assert "--svgf" in r.stderr


def test_host_defaults():
    assert T.SVGF_DEFAULTS == {"iterations": 5, "sigma_lum": 0.5, "sigma_normal": 0.3, "sigma_depth": 0.05,
                               "min_history": 4, "demodulate": True}


def _call(L, scene, out):
    buf = np.zeros((4, 4, 3), np.float32)
    z = np.zeros((4, 4), np.float32)
    a = _lib.Aov(buf.ctypes.data, buf.ctypes.data, z.ctypes.data, None, None)
    p = _lib.SvgfParams(1, 4.0, 0.3, 0.05, 4, _lib.SVGF_DEMODULATE)
    st = _lib.SvgfStats()
    return L.tpt_denoise_svgf(scene, 4, 4, buf.ctypes.data, C.byref(a), z.ctypes.data, z.ctypes.data, C.byref(p),
                              out.ctypes.data, None, None, C.byref(st))


def test_null_scene_fails_cleanly():
    """No device is needed to be refused: a status, a message, nothing written."""
    L = T.lib()
    out = np.full((4, 4, 3), -7.0, np.float32)
    assert _call(L, None, out) == 1                        # TPT_ERR_INVALID_ARG
    assert b"null scene" in L.tpt_last_error()
    assert (out == -7.0).all()


def test_svgf_without_device_fails_cleanly():
    """No scene can exist without a device, so the call can only be refused."""
    if T.device_count() > 0:
        pytest.skip("a HIP device is visible")
    with pytest.raises(T.TPTError) as e:
        T.Scene(os.path.join(ROOT, "tests", "golden", "scenes", "tir.gltf")).copySceneToDevice(0)
    assert e.value.status == 6                             # TPT_ERR_NO_DEVICE
    L = T.lib()
    out = np.full((4, 4, 3), -7.0, np.float32)
    assert _call(L, None, out) == 1 and L.tpt_last_error()


class _NoScene:
    handle = None


def test_host_checks_buffers():
    """The Python host refuses buffers of the wrong size or type, and a history length
    without a variance, before the library sees them."""
    w, h = 5, 3
    pt = T.PathTracer("", w, h, 0)
    rad = np.zeros((h, w, 3), np.float32)
    aov = {"albedo": rad.copy(), "normal": rad.copy(), "depth": np.zeros((h, w), np.float32)}
    plane = np.zeros((h, w), np.float32)
    with pytest.raises(ValueError, match="history_len"):
        pt.denoiseSVGF(_NoScene, rad, aov, None, plane)
    with pytest.raises(ValueError, match="variance"):
        pt.denoiseSVGF(_NoScene, rad, aov, np.zeros((h, w), np.float64))
    with pytest.raises(ValueError, match="variance"):
        pt.denoiseSVGF(_NoScene, rad, aov, np.zeros((h, w + 1), np.float32))
    with pytest.raises(ValueError, match="history_len"):
        pt.denoiseSVGF(_NoScene, rad, aov, plane, np.zeros((h, w), np.int32))
    with pytest.raises(ValueError, match="variance"):
        pt.denoiseSVGF(_NoScene, rad, aov, plane, plane, variance_out=np.zeros((h, w, 3), np.float32))
    with pytest.raises(ValueError, match="radiance"):
        pt.denoiseSVGF(_NoScene, np.zeros((h, w), np.float32), aov)
    with pytest.raises(ValueError, match="radiance"):
        pt.denoiseSVGF(_NoScene, rad, aov, out=np.zeros((h, w, 3), np.float64))
    with pytest.raises(ValueError, match="depth"):
        pt.denoiseSVGF(_NoScene, rad, dict(aov, depth=rad), plane)
    with pytest.raises(ValueError, match="framebuffer"):
        pt.denoiseSVGF(_NoScene, rad, aov, framebuffer=np.zeros((h, w, 3), np.uint8))
    with pytest.raises(T.TPTError) as e:                   # well-formed buffers reach the library: null scene
        pt.denoiseSVGF(_NoScene, rad, aov, plane, plane)
    assert e.value.status == 1


def _frame(rng, H, W):
    n = rng.normal(size=(H, W, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    z = rng.uniform(1, 5, (H, W))
    alb = rng.uniform(0.1, 1, (H, W, 3))
    c = rng.uniform(0, 2, (H, W, 3))
    var = rng.uniform(0, 0.5, (H, W)).astype(np.float32)
    hist = rng.integers(1, 9, (H, W)).astype(np.float32)
    return c, alb, n, z, var, hist


def test_reference_constant_image_is_a_fixed_point():
    c, alb, n, z, var, hist = _frame(np.random.default_rng(3), 12, 17)
    const = np.full((12, 17, 3), 0.7)
    r = SR.svgf_ref(const, alb, n, z, var, hist, iterations=3, demodulate=False)
    assert np.abs(r["out"] - 0.7).max() < 1e-12
    assert np.abs(r["v0"][r["short"]]).max() < 1e-12       # a constant window has no variance
    assert 0 < r["estimated"] < 12 * 17


def test_reference_zero_iterations_is_the_identity():
    c, alb, n, z, var, hist = _frame(np.random.default_rng(3), 12, 17)
    for demodulate in (False, True):
        r = SR.svgf_ref(c, alb, n, z, var, hist, iterations=0, demodulate=demodulate)
        assert np.array_equal(r["out"], c)
        assert np.array_equal(r["variance"], r["v0"])
        assert np.array_equal(r["v0"][~r["short"]], var.astype(np.float64)[~r["short"]])
        assert (r["short"] == (hist < 4)).all()
    # the estimate is the weighted variance of L: one normal, one depth -> the plain 7x7 variance, boosted
    flat_n, flat_z = np.zeros((12, 17, 3)) + (0.0, 0.0, 1.0), np.full((12, 17), 2.0)
    r = SR.svgf_ref(c, alb, flat_n, flat_z, None, None, iterations=0, demodulate=False, min_history=4)
    lum = c @ SR.LUM
    assert r["short"].all() and r["estimated"] == 12 * 17
    assert abs(r["v0"][6, 8] - 4.0 * lum[3:10, 5:12].var()) < 1e-12
    assert abs(r["v0"][0, 0] - 4.0 * lum[0:4, 0:4].var()) < 1e-12      # taps outside the frame are skipped


def test_reference_with_infinite_variance_is_the_plain_filter():
    """A variance scaled towards infinity (1e300: an infinite one would meet weights of 0
    in the variance sum) makes the luminance factor 1: what is left is tpt_denoise's
    filter without its colour factor."""
    c, alb, n, z, var, hist = _frame(np.random.default_rng(4), 12, 17)
    inf = np.full((12, 17), 1e300)
    for demodulate in (False, True):
        r = SR.svgf_ref(c, alb, n, z, inf, None, iterations=3, sigma_normal=0.3, sigma_depth=0.05,
                        demodulate=demodulate)
        plain = R.atrous_ref(c, alb, n, z, 3, 1e30, 0.3, 0.05, demodulate)
        assert r["estimated"] == 0
        assert np.abs(r["out"] - plain).max() < 1e-12
        assert np.abs(r["out"] - c).max() > 0.1


def test_reference_miss_block_filters_among_itself():
    c, alb, n, z, var, hist = _frame(np.random.default_rng(3), 12, 17)
    n[:4, :5] = 0
    z[:4, :5] = 0                                          # a block of misses: z differs from every hit by >= 1
    c2 = c.copy()
    c2[4:, :] += 1.0
    c2[:, 5:] += 1.0
    # one iteration on a given variance: no weight crosses the block's edge
    a = SR.svgf_ref(c, alb, n, z, var, None, iterations=1, demodulate=False)
    b = SR.svgf_ref(c2, alb, n, z, var, None, iterations=1, demodulate=False)
    assert np.array_equal(a["out"][:4, :5], b["out"][:4, :5])          # exp(-1 / (0.05^2 1e-12)) is 0
    assert np.array_equal(a["variance"][:4, :5], b["variance"][:4, :5])
    assert not np.array_equal(a["out"][4:, 5:], b["out"][4:, 5:])
    # Beyond that the hits' variance depends on their colours (the spatial estimate; from
    # the second iteration on the weights of the first), and the 3x3 prefilter, which has
    # no edge stop, carries it into the block's border.  No colour crosses: every hit moved
    # by the same amount keeps the variances (to rounding), and the block with them.
    c3 = c + 1.0
    c3[:4, :5] = c[:4, :5]
    for variance, history in ((var, hist), (None, None)):
        a = SR.svgf_ref(c, alb, n, z, variance, history, iterations=2, demodulate=False)
        b = SR.svgf_ref(c3, alb, n, z, variance, history, iterations=2, demodulate=False)
        assert np.abs(a["out"][:4, :5] - b["out"][:4, :5]).max() < 1e-9
        assert np.abs(a["variance"][:4, :5] - b["variance"][:4, :5]).max() < 1e-9
        assert np.abs(a["out"][4:, 5:] + 1.0 - b["out"][4:, 5:]).max() < 1e-9
