"""Scenes and frames of the pruned-unwind tests (tests/test_unwind_prune_cpu.py states
their premises on the CPU, tests/test_gpu_unwind_prune.py runs the device on them).

k_trace's 2-word-record variants start the unwind of a path that ended with L = +0 at
its deepest level that is not clean (common/trace_variant.hpp, "Pruned unwind").  The
rule needs every baseColor component finite, with a clear sign bit and at most 2^27; the
hostile scenes put a colour that breaks one of these on box's floor material, and with
an inf or NaN colour the reference turns the zero paths that touch it into NaN.

The base scenes are box, ball, the synthesised C5 scene and tir.  The shipped tir's lamp
lights no pixel of a 40x24 frame at 1 spp (tests/variant_scenes.py: 0.5 % at a few
samples), so the premise on lit pixels is stated for variant_scenes.tir_lit, the same
scene through a narrower lens with a wider lamp; the device tests run both."""
import copy

import numpy as np

from oracle import oracle as O
from oracle import scene as oscene
from tests import variant_scenes as VS
from tests.conftest import scene_path

F = np.float32
COLOR_CAP = F(2.0 ** 27)          # kPruneColorCap (trace_variant.hpp)
FLOOR_MATERIAL = "whitWall"       # box.gltf: the material of "bottom" (and of the top and back walls)

W, H, SPP, DEPTH = 40, 24, 16, 8  # the families' frame; the hostile scenes render it too

# name -> the floor material's baseColor
HOSTILE = {
    "inf": (0.8, np.inf, 0.8),
    "nan": (np.nan, 0.8, 0.8),
    "negative": (0.8, 0.8, -0.8),
    "negzero": (-0.0, 0.8, 0.8),
    "overcap": (0.8, np.nextafter(COLOR_CAP, F(np.inf)), 0.8),
    "atcap": (0.8, COLOR_CAP, 0.8),
}

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def base(name) -> oscene.OracleScene:
    """box, ball, tir: the shipped scene; c5: the synthesised one; tir_lit: variant_scenes'."""
    if name == "tir_lit":
        return _once(name, VS.tir_lit)
    return _once(name, lambda: oscene.load_gltf(scene_path(name)))


def hostile(name, n_materials=0) -> oscene.OracleScene:
    """box with HOSTILE[name] on its floor material; n_materials > 0: in a table grown to
    that many entries (65: past what the kernel keeps in LDS)."""
    def make():
        s = copy.copy(base("box"))
        s.materials = np.asarray(s.materials, F).reshape(-1, 15).copy()
        s.materials[s.material_names.index(FLOOR_MATERIAL), :3] = np.array(HOSTILE[name], F)
        return VS.with_materials(s, n_materials) if n_materials else s
    return _once(("hostile", name, n_materials), make)


def oracle_render(s, w, h, spp, depth, env=None):
    """(radiance, counters) of the oracle, seed 42; env in image order (rows top-down)."""
    rad, _, cnt = O.render(O.PackedScene(s), w, h, spp, depth, 42, env=env[::-1].copy() if env is not None else None,
                           trig_mode=1)
    rad.setflags(write=False)
    return rad, cnt


def oracle_frame(key, s, w=W, h=H, spp=SPP, depth=DEPTH, env=None):
    """oracle_render, once per process and key."""
    return _once(("frame", key, w, h, spp, depth, env is not None), lambda: oracle_render(s, w, h, spp, depth, env))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_same(rad, orad):
    """Equal NaN masks, equal bits everywhere else; no pixel excluded."""
    n, m = np.isnan(rad), np.isnan(orad)
    assert np.array_equal(n, m), f"NaN masks differ in {(n != m).sum()} words"
    bad = (bits(rad) != bits(orad)) & ~m
    assert not bad.any(), f"{bad.sum()} words differ"
