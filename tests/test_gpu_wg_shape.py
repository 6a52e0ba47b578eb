"""k_trace's workgroup shape (WGW waves per workgroup, trace_dev.hpp): every variant
family at sizes where each tile-edge case occurs, bit for bit against the CPU
oracle, and the shape that ran against the shape the build declares.

A tile is four waves whatever WGW is, so the sizes cut tiles, sub-tiles and bands:
inside the first 8x8 sub-tile, at a multiple of 8 that is no multiple of 16, and
with a short last band.  Every render asserts tpt_stats.wg_waves equals what the
library declares for the family that must have run (tpt_debug_trace_wg_waves), so a
launch that silently took another family's kernel, or the 4-wave shape, fails; and
that the runtime's resident-workgroup answer, which the host prints under
TPT_DEBUG_SHAPE, fills the CU's wave slots.
"""
import re

import numpy as np
import pytest

import tinypathtracer_amd as T
from oracle import oracle as O

from tests.conftest import scene_path

pytestmark = pytest.mark.gpu

LANE, DRAIN, PAIR, IS, QUAD, REF = range(6)   # tpt_debug_trace_wg_waves families
REF_ORDER, ENV_IS = T._lib.FLAG_REF_ORDER, T._lib.FLAG_ENV_IS


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def scenes():
    out = {}

    def get(name):
        if name not in out:
            s = T.Scene(scene_path(name))
            out[name] = (s, s.copySceneToDevice(0).build(), O.load_scene(scene_path(name)))
        return out[name]

    yield get
    for _, d, _ in out.values():
        d.close()


@pytest.fixture(scope="module")
def oracle_box_72x40():
    """box 72x40, 4 spp, depth 4: shared by the banded cases (never written to)."""
    orad, _, oc = O.render(O.load_scene(scene_path("box")), 72, 40, 4, 4, 42, trig_mode=1)
    orad.setflags(write=False)
    return orad, oc


@pytest.fixture
def shape_log(monkeypatch, capfd):
    """Renders with TPT_DEBUG_SHAPE set; returns the shapes the host printed since the last call."""
    monkeypatch.setenv("TPT_DEBUG_SHAPE", "1")

    def read():
        err = capfd.readouterr().err
        return [dict(zip(("wg_waves", "resident_blocks", "need_blocks", "lds_bytes", "stack_slots", "rec_levels"),
                         map(int, m)))
                for m in re.findall(r"tpt trace shape: wg_waves (\d+) resident_blocks (\d+) need_blocks (\d+) "
                                    r"lds_bytes (\d+) stack_slots (\d+) rec_levels (\d+)", err)]
    return read


def check_shape(st, shape_log, family):
    """The family that must have run, from the call's stats, and its declared shape."""
    declared = int(T.lib().tpt_debug_trace_wg_waves(family))
    assert declared in (1, 2, 4)
    ran = {2: PAIR, 4: QUAD}.get(st["lanes_per_pixel"], DRAIN if st["drained"] else LANE)
    if family in (REF, IS):   # these families have variants of both lane modes / launch sizes
        assert ran in (LANE, DRAIN, PAIR)
    else:
        assert ran == family, (ran, family, st)
    assert st["wg_waves"] == declared, (st["wg_waves"], declared, family)
    shapes = shape_log()
    assert shapes, "TPT_DEBUG_SHAPE printed nothing"
    for sh in shapes:
        assert sh["wg_waves"] == declared
        # 4 SIMDs x the variant's waves per SIMD (4 or 5) in workgroups of wg_waves
        assert sh["need_blocks"] in (16 // declared, 20 // declared)
        assert sh["resident_blocks"] >= sh["need_blocks"], sh
        assert sh["lds_bytes"] <= 163840 // sh["need_blocks"], sh


def render(scenes, name, W, H, spp, depth, family, shape_log, env=None, **kw):
    s, d, _ = scenes(name)
    pt = T.PathTracer("", W, H, 0)
    if env is not None:
        pt.envLight = T.EnvLight(env, 0)
    rad = np.zeros((H, W, 3), np.float32)
    st = pt.doTrace(d, s.m_camera, None, spp, seed=42, max_depth=depth, radiance=rad, **kw)
    check_shape(st, shape_log, family)
    return rad, st


def oracle(scenes, name, W, H, spp, depth, env=None, **kw):
    orad, _, oc = O.render(scenes(name)[2], W, H, spp, depth, 42, env=env[::-1].copy() if env is not None else None,
                           trig_mode=1, **kw)
    return orad, oc


@pytest.mark.parametrize("W,H", [(17, 9), (40, 24)])
def test_one_lane_tile_edges(scenes, shape_log, W, H):
    """17x9 ends inside the first 8x8 sub-tile both ways; 40x24 at a multiple of 8 that is no
    multiple of 16 (the right and top half-tiles' waves have no pixel).  Launches this small are
    drained ones: the DRAIN variants."""
    rad, st = render(scenes, "box", W, H, 4, 4, DRAIN, shape_log, lanes_per_pixel=1)
    orad, oc = oracle(scenes, "box", W, H, 4, 4)
    assert np.array_equal(_bits(rad), _bits(orad))
    assert st["traversals"] == oc["traversals"]


def test_one_lane_full_chip(scenes, shape_log):
    """A launch of more pixels than twice the chip's resident lanes (MI355X 655,360) runs the
    one-lane family proper: 1184x560 = 663,040 pixels, 74 x 35 tiles."""
    W, H = 1184, 560
    rad, st = render(scenes, "box", W, H, 1, 4, LANE, shape_log, lanes_per_pixel=1)
    assert st["drained"] == 0 and W * H >= 2 * st["resident_lanes"]
    orad, oc = oracle(scenes, "box", W, H, 1, 4)
    assert np.array_equal(_bits(rad), _bits(orad))
    assert st["traversals"] == oc["traversals"]


def test_one_lane_bands(scenes, shape_log, oracle_box_72x40):
    """72x40 in bands of 16 rows dealt to 3 ranks: every band_index, the last band 8 rows; then
    the same bands as an explicit list with the whole bands reversed (the API wants a short
    last band last)."""
    orad, _ = oracle_box_72x40
    s, d, _ = scenes("box")
    pt = T.PathTracer("", 72, 40, 0)
    rad = np.zeros((40, 72, 3), np.float32)
    for idx in range(3):
        st = pt.doTrace(d, s.m_camera, None, 4, seed=42, max_depth=4, radiance=rad, band=(16, 3, idx),
                        lanes_per_pixel=1)
        check_shape(st, shape_log, DRAIN)
        assert st["pixels"] == 72 * (8 if idx == 2 else 16)
    assert np.array_equal(_bits(rad), _bits(orad))
    listed = np.zeros((40, 72, 3), np.float32)
    st = pt.doTrace(d, s.m_camera, None, 4, seed=42, max_depth=4, radiance=listed, band=(16, 1, 0),
                    band_list=[1, 0, 2], lanes_per_pixel=1)
    check_shape(st, shape_log, DRAIN)
    assert st["pixels"] == 72 * 40
    assert np.array_equal(_bits(listed), _bits(orad))


def test_pair(scenes, shape_log):
    """Pair mode (8x4 pixels per wave) on a delta-light scene, 20x12: tiles cut both ways."""
    rad, st = render(scenes, "square", 20, 12, 4, 4, PAIR, shape_log, lanes_per_pixel=2)
    orad, oc = oracle(scenes, "square", 20, 12, 4, 4)
    assert np.array_equal(_bits(rad), _bits(orad))
    assert st["traversals"] == oc["traversals"]


def test_pair_env_is(scenes, shape_log):
    sky = T.procedural_sky(64, 32)
    rad, st = render(scenes, "ball", 20, 12, 2, 8, IS, shape_log, env=sky, flags=ENV_IS, lanes_per_pixel=2)
    assert st["lanes_per_pixel"] == 2
    orad, oc = oracle(scenes, "ball", 20, 12, 2, 8, env=sky, env_is=True)
    assert np.array_equal(_bits(rad), _bits(orad))
    assert st["traversals"] == oc["traversals"]


def test_quad(scenes, shape_log):
    """Four lanes per pixel (4x4 pixels per wave, 8x8 per tile), 12x12."""
    rad, st = render(scenes, "box", 12, 12, 4, 4, QUAD, shape_log, lanes_per_pixel=4)
    orad, oc = oracle(scenes, "box", 12, 12, 4, 4)
    assert np.array_equal(_bits(rad), _bits(orad))
    assert st["traversals"] == oc["traversals"]


def test_reference_order(scenes, shape_log):
    rad, st = render(scenes, "box", 24, 24, 4, 4, REF, shape_log, flags=REF_ORDER)
    orad, oc = oracle(scenes, "box", 24, 24, 4, 4)
    assert np.array_equal(_bits(rad), _bits(orad))
    assert st["traversals"] == oc["traversals"] and st["wide_visits"] == 0


def test_deep_records(scenes, shape_log):
    """tir at depth 32: the MAXD 64 variants, records past the LDS levels in private memory."""
    rad, st = render(scenes, "tir", 24, 16, 4, 32, DRAIN, shape_log, lanes_per_pixel=1)
    orad, oc = oracle(scenes, "tir", 24, 16, 4, 32)
    assert np.array_equal(_bits(rad), _bits(orad))
    assert st["traversals"] == oc["traversals"]


def test_frame_batch(scenes, shape_log):
    """3 frames in one launch (grid y interleaves them) against one oracle frame per seed."""
    s, d, o = scenes("box")
    W = H = 24
    seeds = [42, 43, 7]
    pt = T.PathTracer("", W, H, 0)
    rads = [np.zeros((H, W, 3), np.float32) for _ in seeds]
    st = pt.doTraceFrames(d, s.m_camera, seeds, None, 4, max_depth=4, radiances=rads, lanes_per_pixel=1)
    check_shape(st, shape_log, DRAIN)
    assert st["pixels"] == W * H * 3
    for f, sd in enumerate(seeds):
        orad, _, _ = O.render(o, W, H, 4, 4, sd, trig_mode=1)
        assert np.array_equal(_bits(rads[f]), _bits(orad)), f


def test_accumulation(scenes, shape_log):
    """TPT_FLAG_ACCUMULATE: 2 + 2 spp in two calls equals 4 spp in one (and the oracle)."""
    s, d, _ = scenes("box")
    W, H = 40, 24
    pt = T.PathTracer("", W, H, 0)
    prog = np.zeros((H, W, 3), np.float32)
    pt.doTrace(d, s.m_camera, None, 2, seed=42, max_depth=4, radiance=prog, lanes_per_pixel=1)
    st = pt.doTrace(d, s.m_camera, None, 2, max_depth=4, radiance=prog, lanes_per_pixel=1, accumulate=True)
    check_shape(st, shape_log, DRAIN)
    assert st["accumulated_spp"] == 4
    one, _ = render(scenes, "box", W, H, 4, 4, DRAIN, shape_log, lanes_per_pixel=1)
    assert np.array_equal(_bits(prog), _bits(one))
    orad, _ = oracle(scenes, "box", W, H, 4, 4)
    assert np.array_equal(_bits(one), _bits(orad))


def test_forced_pipeline(scenes, shape_log):
    """3 band sets on their own streams, 2 chunks each: one set per band of 40x48."""
    rad, st = render(scenes, "box", 40, 48, 4, 4, DRAIN, shape_log, lanes_per_pixel=1, pipe_sets=3, pipe_chunks=2)
    assert st["trace_launches"] > 3   # every set in chunks (set k starts k / 3 of a chunk early)
    orad, oc = oracle(scenes, "box", 40, 48, 4, 4)
    assert np.array_equal(_bits(rad), _bits(orad))
    assert st["traversals"] == oc["traversals"]


def test_xcd_runs(scenes, shape_log):
    """The synthesised C5 scene (131,712 faces > 16,384) at 256x32: 16 tile columns, two per XCD
    and row, so tiles are dealt to the XCDs in runs of 2 -- a permutation of the row's tiles
    for every WGW, or pixels would be rendered twice and others not at all."""
    rad, st = render(scenes, "c5", 256, 32, 2, 8, DRAIN, shape_log, lanes_per_pixel=1)
    orad, oc = oracle(scenes, "c5", 256, 32, 2, 8)
    assert np.array_equal(_bits(rad), _bits(orad))
    assert st["traversals"] == oc["traversals"]
