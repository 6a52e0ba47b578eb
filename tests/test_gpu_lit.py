"""GPU: delta lights next to emitters, real materials and each other, against the
CPU oracle (DESIGN.md section 4 "Parity").

The shipped scenes with a delta light have one light, no material table and no
emitter, so the oracle-checked renders reach the LIGHTS kernels with one trip of
the light loop, the NOEMIT pair specialisation and the Material() slot only.  The
scenes of tests/lit_scenes.py add lists of lights to box, tir, ball and the
32,769-face box; tests/test_lit_scenes_cpu.py shows on the CPU that every light
lights what it is meant to, that the order of the lights shows in the bits, and
that a device mixing the lights up renders another frame.  Bars as in
tests/test_gpu_variants.py: float bits of radiance and of hit t / uv; BGRA bytes,
hit ids and ray counts equal.  No tolerance anywhere.
"""
import numpy as np
import pytest

import tinypathtracer_amd as T
from oracle import oracle as O
from tests import lit_scenes as L
from tests import variant_scenes as V
from tests.test_gpu_parity import FORCED_WAVEFRONT, assert_parity, image_metrics

pytestmark = pytest.mark.gpu

REF, WF, IS = T._lib.FLAG_REF_ORDER, T._lib.FLAG_WAVEFRONT, T._lib.FLAG_ENV_IS
NAMES = sorted(L.SCENES)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def dev():
    """name -> (Scene, built DeviceScene), each made once; "box" is the shipped scene."""
    cache = {}

    def get(name):
        if name not in cache:
            ts = V.device_scene(V.scene("box") if name == "box" else L.scene(name))
            cache[name] = (ts, ts.copySceneToDevice(0).build())
        return cache[name]

    yield get
    for _, d in cache.values():
        d.close()


_device_frames = {}


def _render(dev, name, flags=0, lanes=0, keep=False, frame=None, **kw):
    """The device's frame of a named scene at its test size (seed 42): (radiance,
    bgra, stats).  keep: cached per arguments, for the frames several cases compare with."""
    key = (name, flags, lanes)
    if keep and key in _device_frames:
        return _device_frames[key]
    ts, d = dev(name)
    W, H, spp, depth, env = frame if frame is not None else L.frame_of("box_l3" if name == "box" else name)
    pt = T.PathTracer("", W, H, 0)
    if env:
        pt.envLight = T.EnvLight(V.sky(), 0)
    rad = np.zeros((H, W, 3), np.float32)
    fb = np.zeros((H, W, 4), np.uint8)
    st = pt.doTrace(d, ts.m_camera, fb, spp, seed=42, max_depth=depth, radiance=rad, flags=flags,
                    lanes_per_pixel=lanes, **kw)
    if keep:
        _device_frames[key] = (rad, fb, st)
    return rad, fb, st


def _equals_oracle(name, rad, fb, st, env_is=False):
    orad, obgra, oc = L.oracle_frame(name, env_is)
    m = image_metrics(rad, orad)
    print(name, m, st["traversals"], oc["traversals"], st["shade_hits"], oc["shade_hits"])
    assert_parity(m)
    assert np.array_equal(_bits(rad), _bits(orad))
    assert np.array_equal(fb[..., :3], obgra[..., :3])
    assert (fb[..., 3] == 0).all()
    assert st["traversals"] == oc["traversals"]
    assert st["shade_hits"] == oc["shade_hits"]


def _same_frames(a, b):
    assert np.array_equal(_bits(a[0]), _bits(b[0]))
    assert np.array_equal(a[1], b[1])
    assert a[2]["traversals"] == b[2]["traversals"] and a[2]["shade_hits"] == b[2]["shade_hits"]


# --------------------------------------------------------------------------
# frames
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_lane_modes_equal_the_oracle(dev, name):
    """k_trace's LIGHTS variants in the ordered walk with one lane per pixel, in pair
    mode (the side lane traces each bounce's shadow rays and hands the direct sum
    back) and with the host's choice, which is pair mode wherever there are delta
    lights: each frame is the oracle's, so the three are each other's.  box_*: the
    pair kernel that is not the NOEMIT specialisation (box has a lamp), with 3, 15
    and 16 trips of the light loop, glass and metal; tir_l2: MAXD = 64;
    box_m64_l3: MTL_LDS = false; ball_l4: NOEMIT with four lights;
    faces_32769_l1: StackT = int."""
    frames = {}
    for lanes in (1, 2, 0):
        rad, fb, st = _render(dev, name, 0, lanes, keep=True)
        _equals_oracle(name, rad, fb, st)
        if not FORCED_WAVEFRONT:
            assert st["lanes_per_pixel"] == (lanes or 2), (lanes, st["lanes_per_pixel"])
            assert st["wg_waves"] > 0
        frames[lanes] = (rad, fb, st)
    _same_frames(frames[1], frames[2])
    _same_frames(frames[1], frames[0])


@pytest.mark.parametrize("lanes", [1, 0])
@pytest.mark.parametrize("name", NAMES)
def test_reference_order_equals_the_oracle(dev, name, lanes):
    """TPT_FLAG_REF_ORDER: the reference's visit order, no culling, no inline
    emitter test, binary nodes only."""
    rad, fb, st = _render(dev, name, REF, lanes)
    _equals_oracle(name, rad, fb, st)
    assert st["local_rays"] == 0
    assert st["wide_visits"] == 0


@pytest.mark.parametrize("name", [n for n in NAMES if n != "faces_32769_l1"])
def test_wavefront_equals_the_oracle(dev, name):
    """TPT_FLAG_WAVEFRONT: wavefront.hip's own light loop."""
    rad, fb, st = _render(dev, name, WF)
    _equals_oracle(name, rad, fb, st)


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("name", L.ENV_IS_SCENES)
def test_env_is_after_the_delta_lights(dev, name, lanes):
    """TPT_FLAG_ENV_IS with more than one delta light (ball_l4: four, NOEMIT) and
    with delta lights and emitters together (box_l3_sky): the delta lights first,
    then the env sample, then the direct probe, in both lane modes, in the
    reference's order and in the wavefront variant."""
    rad, fb, st = _render(dev, name, IS, lanes)
    _equals_oracle(name, rad, fb, st, env_is=True)
    if not FORCED_WAVEFRONT:
        assert st["lanes_per_pixel"] == lanes
    for flags in (IS | REF, IS | WF):
        rad, fb, st = _render(dev, name, flags, lanes)
        _equals_oracle(name, rad, fb, st, env_is=True)


@pytest.mark.parametrize("lanes", [1, 2, 0])
def test_box_dark_is_box_with_more_rays(dev, lanes):
    """Three lights that add nothing (intensity 0, the room outside the cone, every
    shadow ray occluded): the radiance bits and the bytes are the device's own frame
    of box under the same arguments, and every shaded hit traced a ray per light."""
    rad, fb, st = _render(dev, "box_dark", 0, lanes)
    brad, bfb, bst = _render(dev, "box", 0, lanes, keep=True)
    assert np.array_equal(_bits(rad), _bits(brad))
    assert np.array_equal(fb, bfb)
    n_lights = len(L.scene("box_dark").lights)
    assert st["shade_hits"] == bst["shade_hits"]
    assert st["traversals"] == bst["traversals"] + n_lights * bst["shade_hits"]


@pytest.mark.parametrize("lanes", [1, 2])
def test_direct_sum_follows_the_order_of_the_lights(dev, lanes):
    """box_l16 and box_l16r -- the same 16 lights, the list reversed -- are the same
    picture with other last bits (tests/test_lit_scenes_cpu.py: 27 % of the pixels,
    by at most 4.8e-7).  Each frame is its own oracle frame's bits, so the device
    sums `direct` in the order of the list, in the side lane too."""
    a = _render(dev, "box_l16", 0, lanes, keep=True)
    b = _render(dev, "box_l16r", 0, lanes, keep=True)
    _equals_oracle("box_l16", *a)
    _equals_oracle("box_l16r", *b)
    assert not np.array_equal(_bits(a[0]), _bits(b[0]))


@pytest.mark.parametrize("flags,lanes", [(0, 1), (0, 2), (WF, 0)])
def test_material_table_in_global_memory_with_lights(dev, flags, lanes):
    """MTL_LDS = false (64 materials) with lights, emitters and real materials: the
    frame is the oracle's and, bit for bit, the device's frame of box_l3."""
    rad, fb, st = _render(dev, "box_m64_l3", flags, lanes, keep=True)
    _equals_oracle("box_m64_l3", rad, fb, st)
    _same_frames((rad, fb, st), _render(dev, "box_l3", flags, lanes, keep=True))


# --------------------------------------------------------------------------
# refusals
# --------------------------------------------------------------------------
def test_seventeen_lights_are_refused(gpu_available):
    """kMaxLights = 16: tpt_scene_create refuses the 17th light."""
    lights = L.lights_l16()
    s = L.relit("box_l16", lights + lights[:1])
    assert len(s.lights) == 17
    with pytest.raises(T.TPTError, match="too many delta lights"):
        V.device_scene(s).copySceneToDevice(0)


def test_four_lanes_per_pixel_are_refused_with_lights(dev):
    """lanes_per_pixel = 4 runs the one-lane logic on 2-word records: no delta lights.
    (The wavefront variant has no lane modes and renders the frame.)"""
    if FORCED_WAVEFRONT:
        _equals_oracle("box_l3", *_render(dev, "box_l3", 0, 4))
        return
    with pytest.raises(T.TPTError, match="lanes_per_pixel 4"):
        _render(dev, "box_l3", 0, 4)


# --------------------------------------------------------------------------
# schedules
# --------------------------------------------------------------------------
SCHED = (40, 24, 8, 8, None)      # box_l3 at 40 x 24, 8 spp: three 8-row pair-mode tiles


@pytest.fixture(scope="module")
def one_call(dev):
    """box_l3's one-call pair-mode frames at SCHED, seeds 42 and 43 (the first is the oracle's)."""
    ts, d = dev("box_l3")
    W, H, spp, depth, _ = SCHED
    pt = T.PathTracer("", W, H, 0)
    out = {}
    for seed in (42, 43):
        rad = np.zeros((H, W, 3), np.float32)
        fb = np.zeros((H, W, 4), np.uint8)
        pt.doTrace(d, ts.m_camera, fb, spp, seed=seed, max_depth=depth, radiance=rad, lanes_per_pixel=2)
        out[seed] = (rad, fb)
    orad, obgra, _ = O.render(V.oracle_scene(L.scene("box_l3")), W, H, spp, depth, 42, trig_mode=1)
    assert np.array_equal(_bits(out[42][0]), _bits(orad))
    assert np.array_equal(out[42][1][..., :3], obgra[..., :3])
    return pt, out


def test_schedule_bands(dev, one_call):
    """Three interleaved bands of 8 rows."""
    pt, one = one_call
    ts, d = dev("box_l3")
    W, H, spp, depth, _ = SCHED
    banded = np.zeros((H, W, 3), np.float32)
    for idx in range(3):
        pt.doTrace(d, ts.m_camera, None, spp, seed=42, max_depth=depth, radiance=banded, band=(8, 3, idx),
                   lanes_per_pixel=2)
    assert np.array_equal(_bits(banded), _bits(one[42][0]))


@pytest.mark.parametrize("kw", [dict(pipe_sets=2, pipe_chunks=3), dict(spp_per_launch=3)], ids=["pipeline", "chunks"])
def test_schedule_pipeline_and_chunks(dev, one_call, kw):
    """The launch pipeline (2 band sets, 3 chunks) and 3 + 3 + 2 spp in three launches:
    the path records and the side lane's state carry over."""
    pt, one = one_call
    ts, d = dev("box_l3")
    W, H, spp, depth, _ = SCHED
    rad = np.zeros((H, W, 3), np.float32)
    fb = np.zeros((H, W, 4), np.uint8)
    pt.doTrace(d, ts.m_camera, fb, spp, seed=42, max_depth=depth, radiance=rad, lanes_per_pixel=2, **kw)
    assert np.array_equal(_bits(rad), _bits(one[42][0]))
    assert np.array_equal(fb, one[42][1])


def test_schedule_frame_batch(dev, one_call):
    """tpt_render_frames: two frames (seeds 42 and 43) in one launch, each its own one-call frame."""
    pt, one = one_call
    ts, d = dev("box_l3")
    W, H, spp, depth, _ = SCHED
    seeds = [42, 43]
    rads = [np.zeros((H, W, 3), np.float32) for _ in seeds]
    fbs = [np.zeros((H, W, 4), np.uint8) for _ in seeds]
    st = pt.doTraceFrames(d, ts.m_camera, seeds, fbs, spp, max_depth=depth, radiances=rads, lanes_per_pixel=2)
    assert st["pixels"] == W * H * len(seeds)
    for f, seed in enumerate(seeds):
        assert np.array_equal(_bits(rads[f]), _bits(one[seed][0])), seed
        assert np.array_equal(fbs[f], one[seed][1]), seed
    assert not np.array_equal(_bits(rads[0]), _bits(rads[1]))


def test_schedule_accumulate(dev, one_call):
    """TPT_FLAG_ACCUMULATE: 4 + 4 spp continue the same streams and sums as 8."""
    _, one = one_call
    ts, d = dev("box_l3")
    W, H, spp, depth, _ = SCHED
    pt = T.PathTracer("", W, H, 0)
    prog = np.zeros((H, W, 3), np.float32)
    pt.doTrace(d, ts.m_camera, None, 4, seed=42, max_depth=depth, radiance=prog, lanes_per_pixel=2)
    st = pt.doTrace(d, ts.m_camera, None, 4, seed=None, max_depth=depth, radiance=prog, lanes_per_pixel=2,
                    accumulate=True)
    assert st["accumulated_spp"] == spp
    assert np.array_equal(_bits(prog), _bits(one[42][0]))


# --------------------------------------------------------------------------
# shadow rays on their own
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["box_wall", "tir_l2"])
def test_shadow_rays_in_isolation(dev, name):
    """The first bounce's shadow rays through tpt_debug_trace_rays: from the oracle's
    first-hit points of the 32 x 18 pixel-centre rays, the oracle's light_sample
    direction (orc_kat_light) to every light.  The reference's order (mode 0) and
    the render's walk (mode 1, told the face each ray leaves as the render knows it:
    the grazing guard's exempt path) return the oracle's hit ids and, where there
    is a hit, its t / uv bits; any-hit (mode 2) agrees on occlusion.  box_wall: a tenth
    of the rays at least leave a face whose plane contains the light they aim at;
    tir_l2: rays that start on the glass slab, in its plane's upper side."""
    sr = L.shadow_rays(name)
    o, d, face = sr["origins"], sr["dirs"], sr["face"]
    assert 200 <= len(o) <= 4096
    if name == "box_wall":
        assert L.grazing_share(name) >= 0.10
    _, dv = dev(name)
    for mode, ofid in ((0, None), (1, face)):
        h, t, uv = dv.trace_rays(o, d, mode=mode, origin_fid=ofid)
        assert np.array_equal(h, sr["hit"]), (mode, ofid is not None, int((h != sr["hit"]).sum()))
        m = sr["hit"] >= 0
        assert m.sum() >= 20 and (~m).sum() >= 20
        assert np.array_equal(_bits(t[m]), _bits(sr["t"][m])), mode
        assert np.array_equal(_bits(uv[m]), _bits(sr["uv"][m])), mode
    h2, _, _ = dv.trace_rays(o, d, mode=2, origin_fid=face)
    assert np.array_equal(h2 >= 0, sr["hit"] >= 0)
