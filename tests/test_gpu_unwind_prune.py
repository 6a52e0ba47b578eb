"""k_trace's pruned unwind (common/trace_variant.hpp "Pruned unwind")
against the CPU oracle, bit for bit: every family that prunes (one lane per pixel, its
drained form, four lanes per pixel), the depths at which the unwind's start level moves,
an env map (only depth-limited paths are pruned), chunked and progressive schedules,
colours for which the rule does not hold (the kernel must not prune), and the reference
visit order, whose unwind is not pruned, as an independent check on the device.

Where the oracle gives NaN the NaN masks are compared and the bits elsewhere; no pixel
is excluded.  tests/test_unwind_prune_cpu.py proves that the frames hold zero and lit
paths and that the hostile colours reach them."""
import numpy as np
import pytest

import tinypathtracer_amd as T

from tests import prune_scenes as PS
from tests import variant_scenes as VS

pytestmark = pytest.mark.gpu

REF_ORDER = T._lib.FLAG_REF_ORDER
LANES = [0, 1, 4]   # the launch rule's own choice, one lane per pixel, four lanes per pixel


@pytest.fixture(scope="module")
def device():
    """name -> (Scene, DeviceScene), built once; name is a base scene's or ('hostile', name, n)."""
    out = {}

    def get(key):
        if key not in out:
            s = VS.device_scene(PS.base(key) if isinstance(key, str) else PS.hostile(*key[1:]))
            out[key] = (s, s.copySceneToDevice(0).build())
        return out[key]

    yield get
    for _, d in out.values():
        d.close()


def render(device, key, w, h, spp, depth, env=None, **kw):
    s, d = device(key)
    pt = T.PathTracer("", w, h, 0)
    if env is not None:
        pt.envLight = T.EnvLight(env, 0)
    rad = np.zeros((h, w, 3), np.float32)
    st = pt.doTrace(d, s.m_camera, None, spp, seed=42, max_depth=depth, radiance=rad, **kw)
    return rad, st


def check_family(st, lanes):
    if lanes:
        assert st["lanes_per_pixel"] == lanes, st
    assert st["lanes_per_pixel"] in (1, 4), st   # never pair mode: box has no delta light


# ---- families ----
@pytest.mark.parametrize("lanes", LANES)
def test_small_frame(device, lanes):
    """box 40x24 (tiles cut both ways), 16 spp, depth 8: a drained launch."""
    rad, st = render(device, "box", PS.W, PS.H, PS.SPP, PS.DEPTH, lanes_per_pixel=lanes)
    check_family(st, lanes)
    if lanes == 1:
        assert st["drained"] == 1
    orad, oc = PS.oracle_frame("box", PS.base("box"))
    PS.assert_same(rad, orad)
    assert st["traversals"] == oc["traversals"]


@pytest.mark.parametrize("lanes", LANES)
def test_banded_frame(device, lanes):
    """box 72x40 in three bands of 16 rows (the last one 8), one call each."""
    s, d = device("box")
    pt = T.PathTracer("", 72, 40, 0)
    rad = np.zeros((40, 72, 3), np.float32)
    for idx in range(3):
        st = pt.doTrace(d, s.m_camera, None, PS.SPP, seed=42, max_depth=PS.DEPTH, radiance=rad, band=(16, 3, idx),
                        lanes_per_pixel=lanes)
        check_family(st, lanes)
    orad, _ = PS.oracle_frame("box", PS.base("box"), w=72, h=40)
    PS.assert_same(rad, orad)


def test_full_chip_one_lane(device):
    """1184x560 at 2 spp: more pixels than twice the chip's resident lanes, the one-lane
    family proper (the size tests/test_gpu_wg_shape.py uses for it)."""
    w, h = 1184, 560
    rad, st = render(device, "box", w, h, 2, PS.DEPTH, lanes_per_pixel=1)
    assert st["drained"] == 0 and st["lanes_per_pixel"] == 1 and w * h >= 2 * st["resident_lanes"]
    orad, oc = PS.oracle_frame("box", PS.base("box"), w=w, h=h, spp=2)
    PS.assert_same(rad, orad)
    assert st["traversals"] == oc["traversals"]


# ---- depths ----
@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("lanes", [1, 4])
def test_shallow_depths(device, depth, lanes):
    """max_depth 1, 2, 3 (8: test_small_frame): every path is cut at the limit with L = +0."""
    rad, st = render(device, "box", PS.W, PS.H, PS.SPP, depth, lanes_per_pixel=lanes)
    orad, oc = PS.oracle_frame("box", PS.base("box"), depth=depth)
    PS.assert_same(rad, orad)
    assert st["traversals"] == oc["traversals"]


@pytest.mark.parametrize("name", ["tir", "tir_lit"])
def test_deep_records(device, name):
    """tir at depth 32, 8 spp: the MAXD 64 variants, record levels beyond LDS in private memory."""
    rad, st = render(device, name, PS.W, PS.H, 8, 32, lanes_per_pixel=1)
    orad, oc = PS.oracle_frame(name, PS.base(name), spp=8, depth=32)
    PS.assert_same(rad, orad)
    assert st["traversals"] == oc["traversals"]


# ---- env ----
@pytest.mark.parametrize("lanes", [1, 4])
def test_env_map(device, lanes):
    """The procedural sky: every miss ends with L != 0, only depth-limited paths are pruned."""
    sky = T.procedural_sky(64, 32)
    rad, st = render(device, "box", PS.W, PS.H, PS.SPP, PS.DEPTH, env=sky, lanes_per_pixel=lanes)
    orad, oc = PS.oracle_frame("box", PS.base("box"), env=sky)
    PS.assert_same(rad, orad)
    assert st["traversals"] == oc["traversals"]


# ---- schedules ----
def test_forced_pipeline(device):
    """3 band sets on their own streams, 2 chunks each, 40x48."""
    rad, st = render(device, "box", 40, 48, PS.SPP, PS.DEPTH, lanes_per_pixel=1, pipe_sets=3, pipe_chunks=2)
    assert st["trace_launches"] > 3
    orad, oc = PS.oracle_frame("box", PS.base("box"), w=40, h=48)
    PS.assert_same(rad, orad)
    assert st["traversals"] == oc["traversals"]


def test_progressive_accumulation(device):
    """8 + 8 spp in two calls: the second continues every pixel's stream and sum."""
    s, d = device("box")
    pt = T.PathTracer("", PS.W, PS.H, 0)
    rad = np.zeros((PS.H, PS.W, 3), np.float32)
    pt.doTrace(d, s.m_camera, None, 8, seed=42, max_depth=PS.DEPTH, radiance=rad, lanes_per_pixel=1)
    st = pt.doTrace(d, s.m_camera, None, 8, max_depth=PS.DEPTH, radiance=rad, lanes_per_pixel=1, accumulate=True)
    assert st["accumulated_spp"] == 16
    orad, _ = PS.oracle_frame("box", PS.base("box"))
    PS.assert_same(rad, orad)


# ---- hostile materials ----
@pytest.mark.parametrize("lanes", [1, 4])
@pytest.mark.parametrize("name", sorted(PS.HOSTILE))
def test_hostile_colour(device, name, lanes):
    """One colour of box's floor material non-finite, negative, -0, just above the cap or at
    it.  With inf or NaN the reference turns zero paths into NaN: a kernel that pruned
    there would return 0."""
    rad, st = render(device, ("hostile", name, 0), PS.W, PS.H, PS.SPP, PS.DEPTH, lanes_per_pixel=lanes)
    orad, oc = PS.oracle_frame(name, PS.hostile(name))
    PS.assert_same(rad, orad)
    assert st["traversals"] == oc["traversals"]


@pytest.mark.parametrize("name", ["inf", "atcap"])
def test_hostile_colour_global_table(device, name):
    """65 materials: the table is read from global memory, not LDS."""
    rad, st = render(device, ("hostile", name, 65), PS.W, PS.H, PS.SPP, PS.DEPTH, lanes_per_pixel=1)
    orad, oc = PS.oracle_frame(name, PS.hostile(name))   # (the grown table keeps the frame: the CPU test)
    PS.assert_same(rad, orad)
    assert st["traversals"] == oc["traversals"]


# ---- the reference order's unpruned unwind ----
@pytest.mark.parametrize("name,spp,depth", [("box", 16, 8), ("ball", 16, 8), ("tir", 8, 32), ("tir_lit", 8, 32),
                                            ("c5", 2, 8)])
def test_reference_order_agrees(device, name, spp, depth):
    rad, _ = render(device, name, PS.W, PS.H, spp, depth, lanes_per_pixel=1)
    ref, st = render(device, name, PS.W, PS.H, spp, depth, flags=REF_ORDER)
    assert st["wide_visits"] == 0
    assert np.array_equal(PS.bits(rad), PS.bits(ref))
    orad, _ = PS.oracle_frame(name, PS.base(name), spp=spp, depth=depth)
    PS.assert_same(rad, orad)
