"""GPU: the env lookup, env importance sampling and getNewDirection on maps other than
the smooth sky, against the CPU oracle.

Known answers, bit for bit: the device functions of trace_dev.hpp / ptrig.hpp through
tpt_debug_env_kat (kat.hip) against the oracle's hooks (orc_kat_env_lookup,
orc_kat_env_is, orc_kat_new_direction, orc_parity_sincos) -- the device compile of the
parity trig and of the double path, the lookup's fast and exact texel indices on sizes
that are no power of two, the sampler on the adversarial maps of tests/env_maps.py
against each env's real device tables (guide tables, partial blocks, flat CDF runs,
x = 1.0), getNewDirection at the TIR boundary and on degenerate frames.  NaN compares
as "both NaN" (x86 and gfx950 produce different default-NaN patterns).  Float64
restatements bound how far both may be from the mathematics.

Frames, bit for bit (radiance, BGRA bytes, ray counts): box at 20 x 12 under every map,
through every kernel family that reads the env.  tests/test_env_maps_cpu.py shows that
each map reaches its branch and that these frames depend on the map.
"""
import numpy as np
import pytest

import tinypathtracer_amd as T
from oracle import oracle as O
from tests import env_maps as E
from tests import trig_inputs as TI
from tests.conftest import scene_path
from tests.test_gpu_parity import FORCED_WAVEFRONT, assert_parity, image_metrics

pytestmark = pytest.mark.gpu

REF, WF, IS = T._lib.FLAG_REF_ORDER, T._lib.FLAG_WAVEFRONT, T._lib.FLAG_ENV_IS


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    """Bit-equal, NaN matching NaN."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return bool(((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))).all())


def _first_diff(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    bad = ~((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want)))
    rows = np.flatnonzero(bad.reshape(len(got), -1).any(1))
    return len(rows), rows[:5]


# --------------------------------------------------------------------------
# known answers
# --------------------------------------------------------------------------
def test_sincos_device_compile_equals_oracle(gpu_available):
    phi = TI.phis(1_000_000)
    got = T.env_kat("sincos", phi)
    s, c = O.parity_sincos(phi)
    assert _same(got[:, 0], s) and _same(got[:, 1], c)
    rs = np.sin(phi.astype(np.float64)).astype(np.float32)
    rc = np.cos(phi.astype(np.float64)).astype(np.float32)
    assert TI.ulps(got[:, 0].copy(), rs).max() <= 1 and TI.ulps(got[:, 1].copy(), rc).max() <= 1


def test_atan2_acos_double_path_on_the_device(gpu_available):
    """(float) of the device's double evaluation is (float32) of numpy's float64 result, on
    tests/test_cpu_math.py's random and axis sets, the zeros of both signs and tiny values."""
    v = TI.atan2_acos_vectors()
    tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-38, -1e-38, 1e-30, -1e-30, 1e-20, 1.0, -1.0, 3e38, -3e38], np.float32)
    ty, tx = (a.ravel() for a in np.meshgrid(tiny, tiny, indexing="ij"))
    y = np.concatenate([v[:, 2], ty])
    x = np.concatenate([v[:, 0], tx])
    got = T.env_kat("atan2", np.stack([y, x], 1))[:, 0]
    want = np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(np.float32)
    assert _same(got, want), _first_diff(got, want)
    yc = np.concatenate([np.clip(v[:, 1], -1.0, 1.0), tiny[np.abs(tiny) <= 1.0],
                         np.nextafter(np.float32(1.0), np.float32(0.0))[None],
                         np.nextafter(np.float32(-1.0), np.float32(0.0))[None]]).astype(np.float32)
    got = T.env_kat("acos", yc)[:, 0]
    want = np.arccos(yc.astype(np.float64)).astype(np.float32)
    assert _same(got, want), _first_diff(got, want)


@pytest.mark.parametrize("w,h", E.LOOKUP_SIZES)
def test_lookup_indices_and_texels(gpu_available, w, h):
    img = E.lookup_map(w, h)
    env = T.EnvLight(img, 0)
    d = E.lookup_dirs(w, h)
    got = T.env_kat("lookup", d, env=env)
    env.close()
    fc, fr, xc, xr = (got[:, k].astype(np.int64) for k in range(4))
    # the fast indices equal the device's own exact ones wherever they decide
    col, row = fc >= 0, fr >= 0
    assert np.array_equal(fc[col], xc[col]), np.flatnonzero(col & (fc != xc))[:5]
    assert np.array_equal(fr[row], xr[row]), np.flatnonzero(row & (fr != xr))[:5]
    # the exact indices and both forms of the lookup are the oracle's
    rgb, ixy = O.kat_env_lookup(np.ascontiguousarray(img[::-1]), d)
    assert np.array_equal(xc, ixy[:, 0]), np.flatnonzero(xc != ixy[:, 0])[:5]
    assert np.array_equal(xr, ixy[:, 1]), np.flatnonzero(xr != ixy[:, 1])[:5]
    assert _same(got[:, 4:7], rgb) and _same(got[:, 7:10], rgb)
    # the fast bounds decide almost every plain random direction
    plain = np.flatnonzero(TI.plain(E.LOOKUP_RANDOM))
    assert col[plain].mean() > 0.99 and row[plain].mean() > 0.99, (col[plain].mean(), row[plain].mean())
    # float64 Vec2UV agrees away from texel edges (the oracle alone: test_env_maps_cpu.py)
    ix, iy, near = E.texel64(d[plain], w, h)
    assert near.mean() <= 0.01, near.mean()
    assert np.array_equal(xc[plain][~near], ix[~near]) and np.array_equal(xr[plain][~near], iy[~near])


@pytest.mark.parametrize("name", E.LIT)
def test_env_is_sample_on_adversarial_maps(gpu_available, name):
    """env_is_sample against the env's real device tables (tpt_env_create's CDFs and guide
    tables) equals the oracle's plain-search sampler in ok, dir and k_le."""
    cases = E.env_is_cases(name)
    env = T.EnvLight(E.env_map(name), 0)
    got = T.env_kat("env_is", cases, env=env)
    env.close()
    ok, d, k = O.kat_env_is(E.bottom_up(name), cases)
    assert np.array_equal(got[:, 0].astype(np.int32), ok), np.flatnonzero(got[:, 0].astype(np.int32) != ok)[:5]
    assert _same(got[:, 1:4], d), _first_diff(got[:, 1:4], d)
    assert _same(got[:, 4:7], k), _first_diff(got[:, 4:7], k)
    norm_err, outside, accepted = E.env_is_sanity(name, cases, got[:, 0], got[:, 1:4])
    print(name, len(cases), accepted, norm_err, outside)
    assert accepted >= 20000
    assert norm_err <= E.DIR_NORM_TOL and outside <= E.BLOCK_SLACK


def test_env_is_sample_refused_without_a_distribution(gpu_available):
    env = T.EnvLight(E.env_map("black"), 0)
    with pytest.raises(T.TPTError):
        T.env_kat("env_is", np.array([[0, 1, 0, 0.5, 0.5]], np.float32), env=env)
    env.close()
    env = T.EnvLight(E.env_map("odd"), 0)
    for bad in (1.5, -0.25, float("nan")):
        with pytest.raises(T.TPTError):
            T.env_kat("env_is", np.array([[0, 1, 0, bad, 0.5]], np.float32), env=env)
    env.close()
    with pytest.raises(T.TPTError):
        T.env_kat("lookup", np.array([[0, 1, 0]], np.float32))


def test_new_direction_on_the_device(gpu_available):
    cases = E.new_direction_cases()
    n = len(cases)
    st = np.zeros((n, 6), np.uint32)
    T._lib.check(T.lib().tpt_debug_rng_init(0, 42, 0, n, st.ctypes.data))
    assert np.array_equal(st, E.oracle_states(n))
    got, after = T.env_kat("new_direction", cases, states=st)
    want, oafter = O.kat_new_direction(cases, st)
    assert _same(got, want), _first_diff(got, want)
    assert np.array_equal(after, oafter)                     # the same number of uniforms consumed
    err, excluded, draws_ok = E.new_direction_error(cases, st, got, after)
    print(n, err, excluded)
    assert draws_ok and err <= E.NEW_DIRECTION_TOL and excluded <= E.NEW_DIRECTION_MAX_EXCLUDED


# --------------------------------------------------------------------------
# frames
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    out = {}
    for scene in ("box", "ball"):
        s = T.Scene(scene_path(scene))
        out[scene] = (s, s.copySceneToDevice(0).build())
    yield out
    for _, d in out.values():
        d.close()


def _render(built, name, flags=0, lanes=0, scene="box"):
    s, d = built[scene]
    F = E.FRAME
    pt = T.PathTracer("", F["W"], F["H"], 0)
    pt.envLight = T.EnvLight(E.env_map(name), 0)
    rad = np.zeros((F["H"], F["W"], 3), np.float32)
    fb = np.zeros((F["H"], F["W"], 4), np.uint8)
    try:
        st = pt.doTrace(d, s.m_camera, fb, F["spp"], seed=F["seed"], max_depth=F["depth"], radiance=rad, flags=flags,
                        lanes_per_pixel=lanes)
    finally:
        pt.envLight.close()
    return rad, fb, st


def _equals_oracle(name, env_is, rad, fb, st, scene="box"):
    orad, obgra, oc = E.oracle_frame(name, env_is, scene)
    assert_parity(image_metrics(rad, orad))
    assert np.array_equal(_bits(rad), _bits(orad))
    assert np.array_equal(fb[..., :3], obgra[..., :3])
    assert (fb[..., 3] == 0).all()
    assert st["traversals"] == oc["traversals"]
    assert st["shade_hits"] == oc["shade_hits"]


@pytest.mark.parametrize("flags,lanes", [(0, 0), (0, 1), (0, 4), (REF, 0), (WF, 0)],
                         ids=["default", "lane1", "lane4", "ref_order", "wavefront"])
@pytest.mark.parametrize("name", E.NAMES)
def test_frame_without_is(built, name, flags, lanes):
    rad, fb, st = _render(built, name, flags, lanes)
    _equals_oracle(name, False, rad, fb, st)
    if lanes and not (flags & WF) and not FORCED_WAVEFRONT:
        assert st["lanes_per_pixel"] == lanes


@pytest.mark.parametrize("flags,lanes", [(0, 1), (0, 2), (REF, 0), (WF, 0)],
                         ids=["lane1", "pair", "ref_order", "wavefront"])
@pytest.mark.parametrize("name", E.NAMES)
def test_frame_with_env_is(built, name, flags, lanes):
    rad, fb, st = _render(built, name, flags | IS, lanes)
    _equals_oracle(name, True, rad, fb, st)
    if lanes and not FORCED_WAVEFRONT:   # (black: no distribution, so no shadow job for a side lane)
        assert st["lanes_per_pixel"] == (1 if name == "black" else lanes)


@pytest.mark.parametrize("name", ["odd", "sun"])
def test_four_lanes_with_env_is_stays_refused(built, name):
    if not FORCED_WAVEFRONT:   # (the wavefront variant has no lane modes)
        with pytest.raises(T.TPTError):
            _render(built, name, IS, 4)


def test_four_lanes_on_black_run_because_is_is_off(built):
    """An all-black map has no distribution: TPT_FLAG_ENV_IS changes nothing, four lanes included."""
    rad, fb, st = _render(built, "black", IS, 4)
    _equals_oracle("black", True, rad, fb, st)


def test_black_with_env_is_is_its_own_frame_without(built):
    a = _render(built, "black", IS, 0)
    b = _render(built, "black", 0, 0)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1])
    for k in ("traversals", "shade_hits", "local_rays"):
        assert a[2][k] == b[2][k], k


@pytest.mark.parametrize("name", ["odd", "halfblack"])
def test_pair_mode_side_lane_carries_delta_and_env_shadow_jobs(built, name):
    """ball has a point light: under TPT_FLAG_ENV_IS in pair mode the side lane traces the
    delta light's shadow ray and the env sample's."""
    rad, fb, st = _render(built, name, IS, 2, scene="ball")
    _equals_oracle(name, True, rad, fb, st, scene="ball")
    if not FORCED_WAVEFRONT:
        assert st["lanes_per_pixel"] == 2
    assert E.differing_share(E.oracle_frame(name, True, "ball")[0], E.oracle_frame(name, False, "ball")[0]) >= 0.10
