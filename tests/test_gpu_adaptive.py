"""GPU: tpt_render_adaptive against tests/adaptive_ref.py (DESIGN.md section 5 "Adaptive
sampling").

Exactness has no tolerance: the tiles' sample counts equal the reference's (the schedule on
oracle frames; tests/test_adaptive_cpu.py shows that every stop decision is at least 1e-3
relative away from its target), and every pixel of the radiance and of the BGRA frame equals
the plain tpt_render at its tile's count, bit for bit -- each distinct level is rendered once
and the frame composed from them.  The estimate lies within rtol 1e-4 of the float64
reference: a 256-term float32 sum at 2^-24 per step is about 1.5e-5, and each pixel's term
adds a few ulp (three subtractions, two sums, a correctly rounded sqrt and divide).
min_spp 2 and max_spp 32 throughout; frames of at most nine tiles.
"""
import ctypes as C

import numpy as np
import pytest

import tinypathtracer_amd as T
from tests import adaptive_ref as R
from tests import variant_scenes as V

pytestmark = pytest.mark.gpu

L = T._lib
NAMES = sorted(R.CASES)
GUARD = 64          # sentinel elements on either side of every output
F_SENT, B_SENT, I_SENT = np.float32(-7.0), np.uint8(0x5a), np.int32(-77)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def dev():
    """case name -> (Scene, built DeviceScene, PathTracer), each scene built once."""
    scenes, out = {}, {}

    def get(name):
        if name not in out:
            build, W, H, env, _, _, _ = R.CASES[name]
            s = build()                  # (built once per process: cases of one scene share the device's)
            key = id(s)
            if key not in scenes:
                ts = V.device_scene(s)
                scenes[key] = (ts, ts.copySceneToDevice(0).build())
            pt = T.PathTracer("", W, H, 0)
            if env:
                pt.envLight = T.EnvLight(V.sky(), 0)
            out[name] = scenes[key] + (pt,)
        return out[name]

    yield get
    for _, d in scenes.values():
        d.close()


class Out:
    """The four outputs of a call between sentinels: rad [H, W, 3], fb [H, W, 4] (row 0 = top),
    spp and err [tiles_y, tiles_x]."""

    def __init__(self, W, H):
        tx, ty = R.tiles_of(W, H)
        self._raw = {}
        for k, shape, dtype, sent in (("rad", (H, W, 3), np.float32, F_SENT), ("fb", (H, W, 4), np.uint8, B_SENT),
                                      ("spp", (ty, tx), np.int32, I_SENT), ("err", (ty, tx), np.float32, F_SENT)):
            n = int(np.prod(shape))
            raw = np.full(n + 2 * GUARD, sent, dtype)
            self._raw[k] = (raw, sent)
            setattr(self, k, raw[GUARD:GUARD + n].reshape(shape))

    def guards_intact(self):
        return all((raw[:GUARD] == sent).all() and (raw[-GUARD:] == sent).all() for raw, sent in self._raw.values())

    def untouched(self):
        return all((raw == sent).all() for raw, sent in self._raw.values())

    def same_bytes(self, other):
        return all(np.array_equal(self._raw[k][0].view(np.uint8), other._raw[k][0].view(np.uint8)) for k in self._raw)


def adaptive(dev, name, target=None, lanes=0, min_spp=R.MIN_SPP, max_spp=R.MAX_SPP):
    ts, d, pt = dev(name)
    _, W, H, _, flags, case_target, seed = R.CASES[name]
    o = Out(W, H)
    st = pt.doTraceAdaptive(d, ts.m_camera, o.fb, min_spp=min_spp, max_spp=max_spp,
                            target=case_target if target is None else target, seed=seed, max_depth=R.DEPTH,
                            radiance=o.rad, flags=flags, lanes_per_pixel=lanes, tile_spp=o.spp, tile_error=o.err)
    assert o.guards_intact()
    return o, st


_plain = {}


def plain(dev, name, spp):
    """The plain tpt_render of a case at `spp` samples (its flags and seed): (radiance, bgra), once per process."""
    if (name, spp) not in _plain:
        ts, d, pt = dev(name)
        _, W, H, _, flags, _, seed = R.CASES[name]
        rad = np.zeros((H, W, 3), np.float32)
        fb = np.full((H, W, 4), B_SENT, np.uint8)
        pt.doTrace(d, ts.m_camera, fb, spp, seed=seed, max_depth=R.DEPTH, radiance=rad, flags=flags)
        rad.setflags(write=False)
        fb.setflags(write=False)
        _plain[(name, spp)] = (rad, fb)
    return _plain[(name, spp)]


def assert_composed(dev, name, o):
    """Every pixel equals the plain render at its tile's level, bit for bit; alpha untouched."""
    levels = [int(n) for n in np.unique(o.spp)]
    frames = {n: plain(dev, name, n) for n in levels}
    rad = R.compose(o.spp, {n: f[0] for n, f in frames.items()})
    fb = R.compose(o.spp, {n: f[1][::-1] for n, f in frames.items()})[::-1]
    assert np.array_equal(_bits(o.rad), _bits(rad))
    assert np.array_equal(o.fb, fb)
    assert (o.fb[..., 3] == B_SENT).all()


@pytest.mark.parametrize("name", NAMES)
def test_frame_levels_estimate_and_stats(dev, name):
    """Fails without the feature.  The sample counts are the reference's, the frame is the plain
    renders' composition, the estimate is the float64 one within rtol 1e-4, the stats agree."""
    ref = R.reference(name)
    o, st = adaptive(dev, name)
    print(name, "spp", o.spp.tolist(), "err", o.err.tolist(), "ref", ref["tile_error"].tolist(), st)
    assert np.array_equal(o.spp, ref["tile_spp"])
    assert len(np.unique(o.spp)) >= R.MIN_LEVELS[name]
    assert_composed(dev, name, o)
    assert np.allclose(o.err, ref["tile_error"], rtol=1e-4, atol=0.0)
    assert st["samples"] == ref["samples"]
    assert st["pixels"] == o.rad.shape[0] * o.rad.shape[1]
    assert st["passes"] == ref["passes"] and st["unconverged_tiles"] == ref["unconverged"]
    assert st["traversals"] > 0 and st["trace_ms"] > 0.0 and st["error_ms"] > 0.0


def test_degenerate_targets(dev):
    name = "box_37x29"
    o, st = adaptive(dev, name, target=0.0)
    assert (o.spp == R.MAX_SPP).all() and st["unconverged_tiles"] == o.spp.size
    assert np.array_equal(_bits(o.rad), _bits(plain(dev, name, R.MAX_SPP)[0]))
    assert np.array_equal(o.fb, plain(dev, name, R.MAX_SPP)[1])
    o, st = adaptive(dev, name, target=float("inf"))
    assert (o.spp == R.MIN_SPP).all() and st["unconverged_tiles"] == 0 and st["passes"] == 2
    assert np.array_equal(_bits(o.rad), _bits(plain(dev, name, R.MIN_SPP)[0]))
    assert np.array_equal(o.fb, plain(dev, name, R.MIN_SPP)[1])
    # one level only: min_spp == max_spp
    o, st = adaptive(dev, name, target=0.0, min_spp=4, max_spp=4)
    assert (o.spp == 4).all() and st["passes"] == 2
    assert np.array_equal(_bits(o.rad), _bits(plain(dev, name, 4)[0]))


def test_lane_modes_give_identical_outputs(dev):
    """Listed launches in every lane mode: one lane per pixel (4 / WGW parts per tile), four
    lanes (four 8x8 workgroups per tile), the host's choice; on the lit scene one lane and pair
    mode (two 16x8 workgroups per tile)."""
    base, _ = adaptive(dev, "box_37x29", lanes=1)
    for lanes in (4, 0):
        o, _ = adaptive(dev, "box_37x29", lanes=lanes)
        assert o.same_bytes(base), lanes
    base, _ = adaptive(dev, R.LIT_CASE, lanes=1)
    for lanes in (2, 0):
        o, _ = adaptive(dev, R.LIT_CASE, lanes=lanes)
        assert o.same_bytes(base), lanes


def test_deterministic_and_leaves_the_scene_clean(dev):
    name = "box_37x29"
    ts, d, pt = dev(name)
    _, W, H, _, flags, _, seed = R.CASES[name]
    fresh = plain(dev, name, 4)
    a, _ = adaptive(dev, name)
    b, _ = adaptive(dev, name)
    assert a.same_bytes(b)
    # a tpt_render after an adaptive call equals a fresh one
    rad = np.zeros((H, W, 3), np.float32)
    pt.doTrace(d, ts.m_camera, None, 4, seed=seed, max_depth=R.DEPTH, radiance=rad, flags=flags)
    assert np.array_equal(_bits(rad), _bits(fresh[0]))
    # a progressive render after an adaptive call starts over: the tiles' sums are at different counts
    adaptive(dev, name)
    st = pt.doTrace(d, ts.m_camera, None, 4, seed=seed, max_depth=R.DEPTH, radiance=rad, flags=flags, accumulate=True)
    assert st["accumulated_spp"] == 4
    assert np.array_equal(_bits(rad), _bits(fresh[0]))


def test_optional_outputs_and_device_memory(dev):
    import torch
    name = "box_37x29"
    ts, d, pt = dev(name)
    _, W, H, _, flags, target, seed = R.CASES[name]
    host, _ = adaptive(dev, name)
    cu = torch.device("cuda", 0)
    tx, ty = R.tiles_of(W, H)
    rad = torch.full((H, W, 3), -7.0, device=cu)
    fb = torch.full((H, W, 4), 0x5a, dtype=torch.uint8, device=cu)
    spp = torch.full((ty, tx), -77, dtype=torch.int32, device=cu)
    err = torch.full((ty, tx), -7.0, device=cu)
    kw = dict(min_spp=R.MIN_SPP, max_spp=R.MAX_SPP, target=target, seed=seed, max_depth=R.DEPTH, flags=flags)
    pt.doTraceAdaptive(d, ts.m_camera, fb, radiance=rad, tile_spp=spp, tile_error=err, **kw)
    assert np.array_equal(_bits(rad.cpu().numpy()), _bits(host.rad))
    assert np.array_equal(fb.cpu().numpy(), host.fb)
    assert np.array_equal(spp.cpu().numpy(), host.spp)
    assert np.array_equal(_bits(err.cpu().numpy()), _bits(host.err))
    # the radiance alone, the frame buffer alone
    only = np.zeros((H, W, 3), np.float32)
    pt.doTraceAdaptive(d, ts.m_camera, None, radiance=only, **kw)
    assert np.array_equal(_bits(only), _bits(host.rad))
    only = np.full((H, W, 4), B_SENT, np.uint8)
    pt.doTraceAdaptive(d, ts.m_camera, only, **kw)
    assert np.array_equal(only, host.fb)


def _params(W, H, **kw):
    p = L.Params(W, H, 0, R.DEPTH, 42, 16, 1, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


_BAND_LIST = (C.c_int32 * 1)(0)
_BAND_COST = (C.c_float * 2)(0.0, 0.0)
REFUSALS = {
    "min_spp odd": (dict(), (3, 24, 0.1, 0)),
    "min_spp below 2": (dict(), (0, 32, 0.1, 0)),
    "min_spp negative": (dict(), (-2, 32, 0.1, 0)),
    "max_spp no doubling of min_spp": (dict(), (2, 24, 0.1, 0)),
    "max_spp below min_spp": (dict(), (4, 2, 0.1, 0)),
    "target NaN": (dict(), (2, 32, float("nan"), 0)),
    "target negative": (dict(), (2, 32, -0.5, 0)),
    "adaptive flags": (dict(), (2, 32, 0.1, 1)),
    "wavefront": (dict(flags=L.FLAG_WAVEFRONT), (2, 32, 0.1, 0)),
    "accumulate": (dict(flags=L.FLAG_ACCUMULATE), (2, 32, 0.1, 0)),
    "band_count": (dict(band_count=2), (2, 32, 0.1, 0)),
    "band_index": (dict(band_index=1), (2, 32, 0.1, 0)),
    "band_list": (dict(band_list=C.cast(_BAND_LIST, C.POINTER(C.c_int32)), band_list_len=1), (2, 32, 0.1, 0)),
    "band_cost": (dict(band_cost=C.cast(_BAND_COST, C.POINTER(C.c_float))), (2, 32, 0.1, 0)),
    "no image output": (dict(), (2, 32, 0.1, 0)),
    "width 0": (dict(width=0), (2, 32, 0.1, 0)),
    "max_depth 0": (dict(max_depth=0), (2, 32, 0.1, 0)),
    "max_depth 65": (dict(max_depth=65), (2, 32, 0.1, 0)),
    "lanes_per_pixel 3": (dict(lanes_per_pixel=3), (2, 32, 0.1, 0)),
    "null camera": (dict(), (2, 32, 0.1, 0)),
    "null adaptive params": (dict(), None),
}


@pytest.mark.parametrize("why", sorted(REFUSALS))
def test_refusals_leave_the_outputs_untouched(dev, why):
    ts, d, _ = dev("box_37x29")
    W, H = 37, 29
    pkw, akw = REFUSALS[why]
    p = _params(W, H, **pkw)
    ap = L.AdaptiveParams(*akw) if akw is not None else None
    o = Out(W, H)
    cam = ts.m_camera.to_c()
    images = (None, None) if why == "no image output" else (T._addr(o.rad), T._addr(o.fb))
    rc = T.lib().tpt_render_adaptive(d.handle, None, None if why == "null camera" else C.byref(cam), C.byref(p),
                                     C.byref(ap) if ap is not None else None, images[0], images[1],
                                     T._addr(o.spp), T._addr(o.err), None)
    assert rc == 1, (why, rc)   # TPT_ERR_INVALID_ARG
    assert T.lib().tpt_last_error()
    assert o.untouched()


def test_refusal_lanes_4_on_a_lit_scene(dev):
    """tpt_render's own refusal, reached through the launch planner."""
    ts, d, pt = dev(R.LIT_CASE)
    o = Out(37, 29)
    with pytest.raises(T.TPTError) as e:
        pt.doTraceAdaptive(d, ts.m_camera, o.fb, min_spp=2, max_spp=32, target=0.1, seed=42, radiance=o.rad,
                           lanes_per_pixel=4, tile_spp=o.spp, tile_error=o.err)
    assert e.value.status == 1
    assert o.untouched()
