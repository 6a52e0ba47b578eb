"""GPU parity: the HIP path (libtpt.so through the C-ABI) against the CPU oracle.

Bars:
  * integer / index work bit-exact: RNG states, Morton keys, BVH topology,
    hit fids, counters, the copyToFB bytes;
  * float work bit-exact too (same op order, no FMA contraction, the shared
    parity trig): world transforms, boxes, hit t/uv, and every pixel's
    radiance against the oracle (trig_mode 1).  The looser image metrics
    (mean|d| <= 1e-3, p99|d| <= 1e-2, 99.5 % within +-1 after 8-bit
    quantisation) are asserted as well, so a failure says how far off it is.
"""
import numpy as np
import pytest

import tinypathtracer_amd as T
from oracle import oracle as O
import os

from tests.conftest import ROOT, scene_path

pytestmark = pytest.mark.gpu

SCENES = ["box", "box1", "box2", "ball", "tir", "light", "square", "c5"]


# TPT_TEST_FORCE_FLAGS (tinypathtracer_amd._forced_flags) runs the suite through a
# variant; the wavefront variant has its own launch schedule, so the assertions
# on k_trace's launch counts do not apply to it (the images still must match)
FORCED_WAVEFRONT = bool(int(os.environ.get("TPT_TEST_FORCE_FLAGS", "0"), 0) & T._lib.FLAG_WAVEFRONT)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def built():
    out = {}
    for name in SCENES:
        s = T.Scene(scene_path(name))
        out[name] = (s, s.copySceneToDevice(0).build(), O.load_scene(scene_path(name)))
    yield out
    for _, d, _ in out.values():
        d.close()


def test_device_visible(gpu_available):
    assert T.device_count() >= 1


def test_rng_init_matches_oracle(gpu_available):
    first, n = 0, 4096
    st = np.zeros((n, 6), np.uint32)
    T._lib.check(T.lib().tpt_debug_rng_init(0, 42, first, n, st.ctypes.data))
    for i in list(range(0, 64)) + [255, 1000, 4095]:
        s = (O.C.c_uint32 * 6)()
        O.lib().orc_xorwow_init(42, i, s)
        assert list(st[i]) == list(s), i
    # large subsequences (1080p / 4K pixel indices)
    for sub in (2_073_599, 8_294_399, 65_535):
        one = np.zeros((1, 6), np.uint32)
        T._lib.check(T.lib().tpt_debug_rng_init(0, 123456789, sub, 1, one.ctypes.data))
        s = (O.C.c_uint32 * 6)()
        O.lib().orc_xorwow_init(123456789, sub, s)
        assert list(one[0]) == list(s)


@pytest.mark.parametrize("name", SCENES)
def test_world_transform_bit_exact(built, name):
    s, d, o = built[name]
    wv, wn = d.read_world()
    ov, on = O.transform(o)
    assert np.array_equal(_bits(wv), _bits(ov))
    assert np.array_equal(_bits(wn), _bits(on))


@pytest.mark.parametrize("name", SCENES)
def test_bvh_bit_exact(built, name):
    s, d, o = built[name]
    nodes, keys = d.read_bvh()
    onodes, okeys, _, _ = O.build_bvh(o)
    assert np.array_equal(keys, okeys)
    assert np.array_equal(nodes["parent"], onodes["parent"])
    assert np.array_equal(nodes["a"], onodes["a"])
    n_int = s.n_faces - 1
    assert np.array_equal(nodes["b"][:n_int], onodes["b"][:n_int])
    assert np.array_equal(_bits(nodes["bmin"]), _bits(onodes["bmin"]))
    assert np.array_equal(_bits(nodes["bmax"]), _bits(onodes["bmax"]))


@pytest.mark.parametrize("name", ["box", "ball", "box2", "tir"])
def test_trace_rays_bit_exact(built, name):
    s, d, o = built[name]
    rng = np.random.default_rng(7)
    n = 20000
    wv, _ = d.read_world()
    lo, hi = wv.min(0), wv.max(0)
    org = (lo + (hi - lo) * rng.uniform(-0.2, 1.2, (n, 3))).astype(np.float32)
    tgt = (lo + (hi - lo) * rng.uniform(0.0, 1.0, (n, 3))).astype(np.float32)
    dirs = (tgt - org).astype(np.float32)
    dirs[:64] = 0.0                               # degenerate: inf/NaN slab paths
    dirs[64:128, 1] = 0.0                         # axis-parallel rays
    hit, t, uv = d.trace_rays(org, dirs)
    onodes, _, owv, _ = O.build_bvh(o)
    nodes_c = (O.Node * len(onodes)).from_buffer_copy(onodes.tobytes())
    oh = np.zeros(n, np.int32)
    ot = np.zeros(n, np.float32)
    ouv = np.zeros((n, 2), np.float32)
    idx = np.ascontiguousarray(o.indices)
    owv = np.ascontiguousarray(owv)
    for i in range(n):
        tt = O.C.c_float()
        uu = (O.C.c_float * 2)()
        oh[i] = O.lib().orc_trace_ray(nodes_c, s.n_faces, O._ptr(owv, O.C.c_float), O._ptr(idx, O.C.c_uint32),
                                      (O.C.c_float * 3)(*org[i]), (O.C.c_float * 3)(*dirs[i]), O.C.byref(tt), uu)
        ot[i] = tt.value
        ouv[i] = uu[:]
    assert np.array_equal(hit, oh)
    m = hit >= 0
    assert m.sum() > n // 10
    assert np.array_equal(_bits(t[m]), _bits(ot[m]))
    assert np.array_equal(_bits(uv[m]), _bits(ouv[m]))


def image_metrics(a, b):
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    qa = np.clip(a * 255.0, 0, 255).astype(np.int32)
    qb = np.clip(b * 255.0, 0, 255).astype(np.int32)
    within1 = (np.abs(qa - qb) <= 1).all(-1).mean()
    bit_same = (a.view(np.uint32) == b.view(np.uint32)).all(-1).mean()
    return dict(mean=float(d.mean()), p99=float(np.percentile(d, 99)), within1=float(within1),
                bit_same=float(bit_same))


def assert_parity(m, bit_min=1.0):
    assert m["mean"] <= 1e-3, m
    assert m["p99"] <= 1e-2, m
    assert m["within1"] >= 0.995, m
    assert m["bit_same"] >= bit_min, m


CASES = [
    # name, W, H, spp, depth, env
    ("box", 64, 36, 16, 8, None),
    ("box", 48, 48, 16, 4, None),
    ("box2", 64, 36, 16, 8, None),
    ("tir", 64, 36, 16, 32, None),
    ("ball", 64, 36, 16, 8, "sky"),
    ("square", 64, 36, 16, 8, None),
    ("light", 64, 36, 8, 8, "sky"),
    ("box1", 40, 24, 8, 8, "sky"),
    ("c5", 96, 54, 8, 8, None),   # 131,712 triangles: 32-bit stack ids, LDS + private stack
    ("c5", 512, 24, 2, 8, None),  # 32 tiles per row, 16 two-tile workgroups: XCD runs of 2 (k_trace prologue)
    ("box", 72, 40, 8, 8, None),  # 5 tiles per row: the last workgroup's pixel pool is empty
    ("tir", 88, 20, 8, 16, None),  # 6 tiles, the last one partial (x 80..87): pool pixels skipped
]


@pytest.mark.parametrize("order", ["ordered", "reference"])
@pytest.mark.parametrize("name,W,H,spp,depth,env", CASES)
def test_render_parity(built, name, W, H, spp, depth, env, order):
    """Default traversal (near-first + t-culling + leaf-position tie-break) and
    the reference's right-first DFS (TPT_FLAG_REF_ORDER) against the oracle."""
    s, d, o = built[name]
    sky = T.procedural_sky(64, 32) if env else None
    pt = T.PathTracer("", W, H, 0)
    if env:
        pt.envLight = T.EnvLight(sky, 0)
    fb = np.zeros((H, W, 4), np.uint8)
    rad = np.zeros((H, W, 3), np.float32)
    flags = T._lib.FLAG_REF_ORDER if order == "reference" else 0
    stats = pt.doTrace(d, s.m_camera, fb, spp, seed=42, max_depth=depth, radiance=rad, flags=flags)
    orad, obgra, oc = O.render(o, W, H, spp, depth, 42, env=sky[::-1].copy() if env else None, trig_mode=1)
    m = image_metrics(rad, orad)
    assert_parity(m)
    # copyToFB layout: flipped rows, B,G,R bytes (exact); alpha untouched
    assert np.array_equal(fb[..., :3], obgra[..., :3])
    assert (fb[..., 3] == 0).all()
    # ray counts are deterministic; equal unless a diverged path took a different branch
    assert abs(stats["traversals"] - oc["traversals"]) <= 0.01 * oc["traversals"]
    # probes resolved in the shading pass (no emitter / inline emitter test) are a subset
    assert 0 <= stats["local_rays"] <= stats["traversals"]
    if order == "reference":
        assert stats["local_rays"] == 0
    elif name in ("box", "box1", "square"):   # box: inline emitter test; box1, square: no emitter
        assert stats["local_rays"] > 0
    if m["bit_same"] == 1.0:
        assert stats["traversals"] == oc["traversals"]
        assert stats["shade_hits"] == oc["shade_hits"]
        if order == "reference":
            assert stats["wide_visits"] == 0   # binary nodes only
        if order == "reference" and not s.lights:   # same visit sequence as the reference DFS
            assert stats["internal_visits"] == oc["internal_visits"]
            assert stats["leaf_tests"] == oc["leaf_tests"]
        else:   # culling / any-hit shadow rays only ever remove visits; a 4-wide node is
            # one even-depth binary node the reference also pops
            assert stats["internal_visits"] + stats["wide_visits"] <= oc["internal_visits"]
            assert stats["leaf_tests"] <= oc["leaf_tests"]


# The BASELINE configurations at their full resolution and a few
# spp: C2 box, C3 ball + sky (2048x1024 procedural equirect), C4 tir at depth
# 32, C5 the 131,712-triangle merge at 3840x2160.  The oracle runs on the
# box's host cores (OpenMP); the GPU renders in the default order, in the
# reference's order and (C2) through a forced launch pipeline.
FULL = [
    # name, W, H, spp, depth, env
    ("box", 1920, 1080, 2, 8, None),
    ("ball", 1920, 1080, 2, 8, "sky"),
    ("tir", 1920, 1080, 2, 32, None),
    ("c5", 3840, 2160, 1, 8, None),
]


@pytest.mark.parametrize("name,W,H,spp,depth,env", FULL)
def test_render_parity_full_resolution(built, name, W, H, spp, depth, env):
    s, d, o = built[name]
    sky = T.procedural_sky(2048, 1024) if env else None
    orad, obgra, oc = O.render(o, W, H, spp, depth, 42, env=sky[::-1].copy() if env else None, trig_mode=1)
    pt = T.PathTracer("", W, H, 0)
    if env:
        pt.envLight = T.EnvLight(sky, 0)
    runs = [("ordered", {}), ("reference", {"flags": T._lib.FLAG_REF_ORDER})]
    if name == "box":   # 3 band sets on 3 streams, 2 chunks each (host/launch_plan.cpp launch pipeline)
        runs.append(("pipeline", {"pipe_sets": 3, "pipe_chunks": 2}))
    if name == "ball":   # delta light: pair mode is the default; one lane per pixel too
        runs.append(("one lane per pixel", {"lanes_per_pixel": 1}))
    for label, kw in runs:
        fb = np.zeros((H, W, 4), np.uint8)
        rad = np.zeros((H, W, 3), np.float32)
        st = pt.doTrace(d, s.m_camera, fb, spp, seed=42, max_depth=depth, radiance=rad, **kw)
        m = image_metrics(rad, orad)
        assert m["bit_same"] == 1.0, (label, m, int((rad.view(np.uint32) != orad.view(np.uint32)).any(-1).sum()))
        assert np.array_equal(fb[..., :3], obgra[..., :3]), label
        assert st["traversals"] == oc["traversals"], label
        assert st["shade_hits"] == oc["shade_hits"], label
        if label == "pipeline" and not FORCED_WAVEFRONT:
            assert st["trace_launches"] > 3


@pytest.mark.parametrize("name,W,H,spp,depth,env", [("ball", 64, 36, 16, 8, "sky"), ("square", 64, 36, 16, 8, None),
                                                    ("ball", 48, 30, 6, 32, "sky"), ("square", 40, 24, 8, 1, None)])
def test_pair_mode_parity(built, name, W, H, spp, depth, env):
    """Pair mode (lanes_per_pixel=2: a side lane per pixel traces the shadow
    rays): bit-identical to one lane per pixel and to the oracle, ray counts
    unchanged; banded and launch-pipelined schedules too."""
    s, d, o = built[name]
    sky = T.procedural_sky(64, 32) if env else None
    pt = T.PathTracer("", W, H, 0)
    if env:
        pt.envLight = T.EnvLight(sky, 0)
    one = np.zeros((H, W, 3), np.float32)
    fb1 = np.zeros((H, W, 4), np.uint8)
    st1 = pt.doTrace(d, s.m_camera, fb1, spp, seed=42, max_depth=depth, radiance=one, lanes_per_pixel=1)
    two = np.zeros((H, W, 3), np.float32)
    fb2 = np.zeros((H, W, 4), np.uint8)
    st2 = pt.doTrace(d, s.m_camera, fb2, spp, seed=42, max_depth=depth, radiance=two, lanes_per_pixel=2)
    assert np.array_equal(_bits(two), _bits(one))
    assert np.array_equal(fb2, fb1)
    assert st2["traversals"] == st1["traversals"] and st2["shade_hits"] == st1["shade_hits"]
    orad, _, oc = O.render(o, W, H, spp, depth, 42, env=sky[::-1].copy() if env else None, trig_mode=1)
    assert np.array_equal(_bits(two), _bits(orad))
    assert st2["traversals"] == oc["traversals"]
    banded = np.zeros((H, W, 3), np.float32)
    for idx in range(3):
        pt.doTrace(d, s.m_camera, None, spp, seed=42, max_depth=depth, radiance=banded, band=(8, 3, idx),
                   lanes_per_pixel=2)
    assert np.array_equal(_bits(banded), _bits(one))
    piped = np.zeros((H, W, 3), np.float32)
    pt.doTrace(d, s.m_camera, None, spp, seed=42, max_depth=depth, radiance=piped, lanes_per_pixel=2,
               pipe_sets=2, pipe_chunks=3)
    assert np.array_equal(_bits(piped), _bits(one))


def test_pair_mode_full_resolution_c3(built):
    """C3 (ball + sky) at 1920x1080, 2 spp, in pair mode: bit-exact vs the oracle."""
    s, d, o = built["ball"]
    W, H, spp = 1920, 1080, 2
    sky = T.procedural_sky(2048, 1024)
    orad, obgra, oc = O.render(o, W, H, spp, 8, 42, env=sky[::-1].copy(), trig_mode=1)
    pt = T.PathTracer("", W, H, 0)
    pt.envLight = T.EnvLight(sky, 0)
    fb = np.zeros((H, W, 4), np.uint8)
    rad = np.zeros((H, W, 3), np.float32)
    st = pt.doTrace(d, s.m_camera, fb, spp, seed=42, radiance=rad, lanes_per_pixel=2)
    assert np.array_equal(_bits(rad), _bits(orad))
    assert np.array_equal(fb[..., :3], obgra[..., :3])
    assert st["traversals"] == oc["traversals"]


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("name", ["ball", "box1", "box", "square"])
def test_env_importance_sampling_parity(built, name, lanes):
    """TPT_FLAG_ENV_IS (A15 re-derived, opt-in): env next-event estimation at
    diffuse hits against the oracle's restatement -- same tables, samples,
    shadow rays and ray counts; and the flag does change the image.  Both lane
    modes: in pair mode the path lane draws the env sample's uniforms in RNG
    order and the side lane evaluates it and traces its shadow ray after the
    bounce's delta-light rays (box1, box: env only; ball, square: a light too)."""
    s, d, o = built[name]
    W, H, spp = 48, 27, 8
    sky = T.procedural_sky(128, 64)
    pt = T.PathTracer("", W, H, 0)
    pt.envLight = T.EnvLight(sky, 0)
    rad = np.zeros((H, W, 3), np.float32)
    stats = pt.doTrace(d, s.m_camera, None, spp, seed=42, radiance=rad, flags=T._lib.FLAG_ENV_IS,
                       lanes_per_pixel=lanes)
    orad, _, oc = O.render(o, W, H, spp, 8, 42, env=sky[::-1].copy(), trig_mode=1, env_is=True)
    m = image_metrics(rad, orad)
    assert_parity(m)
    assert m["bit_same"] == 1.0, m
    assert stats["traversals"] == oc["traversals"]
    plain = np.zeros((H, W, 3), np.float32)
    st2 = pt.doTrace(d, s.m_camera, None, spp, seed=42, radiance=plain)
    assert st2["traversals"] < stats["traversals"]        # one env shadow ray per diffuse hit
    assert not np.array_equal(_bits(plain), _bits(rad))
    ref = np.zeros((H, W, 3), np.float32)                  # the reference's visit order, IS on
    st3 = pt.doTrace(d, s.m_camera, None, spp, seed=42, radiance=ref,
                     flags=T._lib.FLAG_ENV_IS | T._lib.FLAG_REF_ORDER)
    assert np.array_equal(_bits(ref), _bits(rad))
    assert st3["traversals"] == stats["traversals"]


def test_env_importance_sampling_full_resolution_c3(built):
    """C3 with A15 on (BASELINE configs[2] "env-light importance sampling
    path"): ball + the 2048x1024 sky at 1920x1080, 2 spp, bit-exact against the
    oracle's restatement in both lane modes (pair mode is the default)."""
    s, d, o = built["ball"]
    W, H, spp = 1920, 1080, 2
    sky = T.procedural_sky(2048, 1024)
    orad, obgra, oc = O.render(o, W, H, spp, 8, 42, env=sky[::-1].copy(), trig_mode=1, env_is=True)
    pt = T.PathTracer("", W, H, 0)
    pt.envLight = T.EnvLight(sky, 0)
    for lanes in (0, 1, 2):
        fb = np.zeros((H, W, 4), np.uint8)
        rad = np.zeros((H, W, 3), np.float32)
        st = pt.doTrace(d, s.m_camera, fb, spp, seed=42, radiance=rad, flags=T._lib.FLAG_ENV_IS,
                        lanes_per_pixel=lanes)
        m = image_metrics(rad, orad)
        assert m["bit_same"] == 1.0, (lanes, m)
        assert np.array_equal(fb[..., :3], obgra[..., :3]), lanes
        assert st["traversals"] == oc["traversals"], lanes
        assert st["shade_hits"] == oc["shade_hits"], lanes


def test_band_sharding_bit_identical(built):
    s, d, _ = built["box"]
    W, H, spp = 64, 48, 8
    pt = T.PathTracer("", W, H, 0)
    full = np.zeros((H, W, 3), np.float32)
    pt.doTrace(d, s.m_camera, None, spp, seed=42, radiance=full)
    for count in (2, 3, 4):
        acc = np.zeros((H, W, 3), np.float32)
        for idx in range(count):
            pt.doTrace(d, s.m_camera, None, spp, seed=42, radiance=acc, band=(16, count, idx))
        assert np.array_equal(_bits(acc), _bits(full)), count


def test_frame_batch_bit_identical(built):
    """tpt_render_frames: a batch of frames in one launch (grid z), each equal
    bit for bit to a separate doTrace with its seed -- whole frames, banded
    frames (the weak-scaling split), host and torch device outputs, bgra too;
    a progressive continuation of the batch equals one call with the total spp."""
    import torch
    s, d, _ = built["box"]
    W, H, spp = 48, 40, 6
    seeds = [42, 43, 7]
    pt = T.PathTracer("", W, H, 0)
    singles, fbs = [], []
    for sd in seeds:
        r = np.zeros((H, W, 3), np.float32)
        fb = np.zeros((H, W, 4), np.uint8)
        pt.doTrace(d, s.m_camera, fb, spp, seed=sd, radiance=r)
        singles.append(r)
        fbs.append(fb)
    rads = [np.zeros((H, W, 3), np.float32) for _ in seeds]
    fbo = [np.zeros((H, W, 4), np.uint8) for _ in seeds]
    st = pt.doTraceFrames(d, s.m_camera, seeds, fbo, spp, radiances=rads)
    assert (FORCED_WAVEFRONT or st["trace_launches"] == 1) and st["pixels"] == W * H * len(seeds)
    for f in range(len(seeds)):
        assert np.array_equal(_bits(rads[f]), _bits(singles[f])), f
        assert np.array_equal(fbo[f], fbs[f]), f
    # banded: every rank renders its rows of every frame (bench.py weak scaling)
    dev = [torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0") for _ in seeds]
    for idx in range(3):
        pt.doTraceFrames(d, s.m_camera, seeds, None, spp, radiances=dev, band=(16, 3, idx))
    for f in range(len(seeds)):
        assert np.array_equal(_bits(dev[f].cpu().numpy()), _bits(singles[f])), f
    # progressive continuation of the whole batch
    prog = [np.zeros((H, W, 3), np.float32) for _ in seeds]
    pt.doTraceFrames(d, s.m_camera, seeds, None, 2, radiances=prog)
    st = pt.doTraceFrames(d, s.m_camera, seeds, None, 4, radiances=prog, accumulate=True)
    assert st["accumulated_spp"] == spp
    for f in range(len(seeds)):
        assert np.array_equal(_bits(prog[f]), _bits(singles[f])), f


def test_spp_chunking_bit_identical(built):
    s, d, _ = built["box2"]
    W, H, spp = 32, 32, 12
    pt = T.PathTracer("", W, H, 0)
    a = np.zeros((H, W, 3), np.float32)
    b = np.zeros((H, W, 3), np.float32)
    pt.doTrace(d, s.m_camera, None, spp, seed=9, radiance=a, spp_per_launch=spp)
    st = pt.doTrace(d, s.m_camera, None, spp, seed=9, radiance=b, spp_per_launch=5)
    assert FORCED_WAVEFRONT or st["trace_launches"] == 3
    assert np.array_equal(_bits(a), _bits(b))


def test_launch_pipeline_bit_identical(built):
    """The launch pipeline (row band sets on their own streams, spp in offset
    chunks, host/launch_plan.cpp; the default from 1024 spp on, tpt_params.pipe_sets
    forces it from 256) equals one launch bit for bit: 2, 3 and 4 sets, banded
    across ranks, and a frame batch."""
    s, d, _ = built["box"]
    W, H, spp = 96, 80, 256
    pt = T.PathTracer("", W, H, 0)
    one = np.zeros((H, W, 3), np.float32)
    fb1 = np.zeros((H, W, 4), np.uint8)
    st1 = pt.doTrace(d, s.m_camera, fb1, spp, seed=11, radiance=one, pipe_sets=1)
    assert FORCED_WAVEFRONT or st1["trace_launches"] == 1
    seeds = [11, 12]
    batch1 = [np.zeros((H, W, 3), np.float32) for _ in seeds]
    pt.doTraceFrames(d, s.m_camera, seeds, None, spp, radiances=batch1, pipe_sets=1)
    for sets, launches in ((2, 5), (3, 8), (4, 11)):   # chunks of 128 spp, set k k/sets of a chunk ahead
        got = np.zeros((H, W, 3), np.float32)
        fb = np.zeros((H, W, 4), np.uint8)
        st = pt.doTrace(d, s.m_camera, fb, spp, seed=11, radiance=got, pipe_sets=sets)
        assert FORCED_WAVEFRONT or st["trace_launches"] == launches, sets
        assert st["traversals"] == st1["traversals"]
        assert st["trace_kernel_ms"] > 0.0
        assert np.array_equal(_bits(got), _bits(one)), sets
        assert np.array_equal(fb, fb1), sets
    # more chunks per set: 3 sets x 2 chunks of >= 128 spp
    got = np.zeros((H, W, 3), np.float32)
    st = pt.doTrace(d, s.m_camera, None, spp, seed=11, radiance=got, pipe_sets=3, pipe_chunks=2)
    assert np.array_equal(_bits(got), _bits(one))
    banded = np.zeros((H, W, 3), np.float32)
    for idx in range(2):
        pt.doTrace(d, s.m_camera, None, spp, seed=11, radiance=banded, band=(16, 2, idx), pipe_sets=2)
    assert np.array_equal(_bits(banded), _bits(one))
    batch = [np.zeros((H, W, 3), np.float32) for _ in seeds]
    st = pt.doTraceFrames(d, s.m_camera, seeds, None, spp, radiances=batch, pipe_sets=2)
    assert FORCED_WAVEFRONT or st["trace_launches"] > 1
    for f in range(len(seeds)):
        assert np.array_equal(_bits(batch[f]), _bits(batch1[f])), f


def test_progressive_accumulation_bit_identical(built):
    """TPT_FLAG_ACCUMULATE: 4 calls of 4 spp continue the same per-pixel streams
    and sums, so the frame equals one 16-spp call bit for bit; a changed frame
    (other seed) starts afresh."""
    s, d, _ = built["box"]
    W, H = 40, 24
    pt = T.PathTracer("", W, H)
    one = np.zeros((H, W, 3), np.float32)
    pt.doTrace(d, s.m_camera, None, 16, seed=5, radiance=one)
    prog = np.zeros((H, W, 3), np.float32)
    for i in range(4):
        st = pt.doTrace(d, s.m_camera, None, 4, seed=5 if i == 0 else None, radiance=prog, accumulate=i > 0)
        assert st["accumulated_spp"] == 4 * (i + 1)
    assert np.array_equal(_bits(prog), _bits(one))
    fresh = np.zeros((H, W, 3), np.float32)
    st = pt.doTrace(d, s.m_camera, None, 4, seed=6, radiance=fresh, accumulate=True)   # other seed: restart
    assert st["accumulated_spp"] == 4


def test_render_is_deterministic(built):
    s, d, _ = built["box"]
    pt = T.PathTracer("", 32, 32, 0)
    a = np.zeros((32, 32, 3), np.float32)
    b = np.zeros((32, 32, 3), np.float32)
    pt.doTrace(d, s.m_camera, None, 8, seed=5, radiance=a)
    pt.doTrace(d, s.m_camera, None, 8, seed=5, radiance=b)
    assert np.array_equal(_bits(a), _bits(b))
    c = np.zeros((32, 32, 3), np.float32)
    pt.doTrace(d, s.m_camera, None, 8, seed=6, radiance=c)
    assert not np.array_equal(a, c)


def test_errors_are_reported(built):
    s, d, _ = built["box"]
    pt = T.PathTracer("", 16, 16, 0)
    with pytest.raises(T.TPTError):
        pt.doTrace(d, s.m_camera, None, 0, seed=1)          # spp 0
    with pytest.raises(T.TPTError):
        pt.doTrace(d, s.m_camera, None, 4, seed=1, max_depth=65)
    with pytest.raises(T.TPTError):
        pt.doTrace(d, s.m_camera, None, 4, seed=1, band=(16, 2, 5))


def test_torch_device_output(built):
    torch = pytest.importorskip("torch")
    s, d, _ = built["box"]
    W, H = 32, 16
    pt = T.PathTracer("", W, H, 0)
    host = np.zeros((H, W, 3), np.float32)
    pt.doTrace(d, s.m_camera, None, 4, seed=3, radiance=host)
    dev = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    pt.doTrace(d, s.m_camera, None, 4, seed=3, radiance=dev)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(dev.cpu().numpy()), _bits(host))


def test_pathtracer_render_api():
    pt = T.PathTracer("", 32, 18, 0)
    fr = pt.render(scene_path("box"), nSamplesPerPixel=4, seed=1)
    assert fr.bgra.shape == (18, 32, 4) and fr.radiance.shape == (18, 32, 3)
    assert fr.stats["traversals"] > 0 and fr.radiance.mean() > 0.01


@pytest.mark.parametrize("frames", [1, 4])
def test_cpp_cli_matches_python_host(tmp_path, frames):
    """tpt_render (C++ host API, include/tpt.hpp) renders the same frame as the
    Python host mirror through the same C-ABI; 4 progressive frames of 2 spp
    equal one 8-spp frame."""
    import subprocess
    exe = os.path.join(ROOT, "tinypathtracer_amd", "tpt_render")
    W, H, spp = 48, 27, 8
    out = str(tmp_path / "cli")
    extra = ["--frames", str(frames), "--progressive"] if frames > 1 else []
    res = subprocess.run([exe, scene_path("box"), "--width", str(W), "--height", str(H), "--spp",
                          str(spp // frames), "--seed", "42", "--out", out] + extra,
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    with open(out + ".pfm", "rb") as f:
        for _ in range(3):
            f.readline()
        pfm = np.frombuffer(f.read(), np.float32).reshape(H, W, 3)
    s = T.Scene(scene_path("box"))
    d = s.copySceneToDevice(0).build()
    rad = np.zeros((H, W, 3), np.float32)
    T.PathTracer("", W, H, 0).doTrace(d, s.m_camera, None, spp, seed=42, radiance=rad)
    d.close()
    assert np.array_equal(pfm.view(np.uint32), rad.view(np.uint32))


def test_env_from_jpeg_file(built, tmp_path):
    """EnvLight(file) (env_light.cuh:8-18): a JPEG env decoded natively
    (tpt_env_load, C++ CLI --env) renders bit-identically to the same texels
    decoded by libjpeg (PIL) and uploaded as an array; the C++ CLI agrees."""
    import subprocess
    from PIL import Image
    s, d, _ = built["ball"]
    W, H, spp = 40, 24, 4
    sky = T.procedural_sky(256, 128)[..., :3]
    jpg = str(tmp_path / "sky.jpg")
    Image.fromarray(sky).save(jpg, "JPEG", quality=85, progressive=True)
    decoded = np.asarray(Image.open(jpg).convert("RGB"))
    a = T.PathTracer("", W, H, 0)
    a.envLight = T.EnvLight(jpg)                 # native decoder
    assert a.envLight.rgba is None
    b = T.PathTracer("", W, H, 0)
    b.envLight = T.EnvLight(decoded)             # libjpeg's texels as an array
    ra = np.zeros((H, W, 3), np.float32)
    rb = np.zeros((H, W, 3), np.float32)
    a.doTrace(d, s.m_camera, None, spp, seed=3, radiance=ra)
    b.doTrace(d, s.m_camera, None, spp, seed=3, radiance=rb)
    assert ra.max() > 0
    assert np.array_equal(_bits(ra), _bits(rb))
    exe = os.path.join(ROOT, "tinypathtracer_amd", "tpt_render")
    out = str(tmp_path / "cli")
    res = subprocess.run([exe, scene_path("ball"), "--width", str(W), "--height", str(H), "--spp", str(spp),
                          "--seed", "3", "--env", jpg, "--out", out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    with open(out + ".pfm", "rb") as f:
        for _ in range(3):
            f.readline()
        pfm = np.frombuffer(f.read(), np.float32).reshape(H, W, 3)
    assert np.array_equal(pfm.view(np.uint32), _bits(ra))
