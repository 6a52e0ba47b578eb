"""GPU: the trace-kernel variants and size limits the shipped scenes never reach,
against the CPU oracle (DESIGN.md section 4 "Parity", the table of launch decisions).

The shipped scenes and C5 all sit in one corner of the host's launch rules (at most
six materials, LBVHs far shallower than 48, finite boxes, 2 to 1,932 or 131,712
faces).  The scenes of tests/variant_scenes.py cross each rule in turn;
tests/test_variant_scenes_cpu.py shows on the CPU that each is on the far side of
its rule and that a device taking the wrong side renders another frame.  Bars as in
tests/test_gpu_parity.py: float bits of radiance, hit t / uv, world vertices and
boxes; BGRA bytes, hit ids, BVH links, Morton keys and ray counts equal.
"""
import numpy as np
import pytest

import tinypathtracer_amd as T
from tests import post_ref
from tests import variant_scenes as V
from tests.test_gpu_cull import _check_modes
from tests.test_gpu_parity import FORCED_WAVEFRONT, assert_parity, image_metrics

pytestmark = pytest.mark.gpu

REF = T._lib.FLAG_REF_ORDER
ORDERS = {"ordered": 0, "reference": REF}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def dev():
    """name -> (Scene, built DeviceScene), each made once."""
    cache = {}

    def get(name):
        if name not in cache:
            ts = V.device_scene(V.scene(name))
            cache[name] = (ts, ts.copySceneToDevice(0).build())   # tpt_scene_build accepts every scene here
        return cache[name]

    yield get
    for _, d in cache.values():
        d.close()


_device_frames = {}


def _render(dev, name, flags=0, lanes=0, env_is=False, keep=False):
    """The device's frame of a named scene at its test size (seed 42).  keep: cached
    per arguments -- the base scenes' frames, which several cases compare with."""
    key = (name, flags, lanes, env_is)
    if keep and key in _device_frames:
        return _device_frames[key]
    ts, d = dev(name)
    W, H, spp, depth, env = V.frame_of(name)
    pt = T.PathTracer("", W, H, 0)
    if env:
        pt.envLight = T.EnvLight(V.sky(), 0)
    rad = np.zeros((H, W, 3), np.float32)
    fb = np.zeros((H, W, 4), np.uint8)
    st = pt.doTrace(d, ts.m_camera, fb, spp, seed=42, max_depth=depth, radiance=rad,
                    flags=flags | (T._lib.FLAG_ENV_IS if env_is else 0), lanes_per_pixel=lanes)
    if keep:
        _device_frames[key] = (rad, fb, st)
    return rad, fb, st


def _equals_oracle(name, rad, fb, st, env_is=False):
    orad, obgra, oc = V.oracle_frame(name, env_is)
    m = image_metrics(rad, orad)
    print(name, m, st["traversals"], oc["traversals"])
    assert_parity(m)
    assert np.array_equal(_bits(rad), _bits(orad))
    assert np.array_equal(fb[..., :3], obgra[..., :3])
    assert (fb[..., 3] == 0).all()
    assert st["traversals"] == oc["traversals"]
    assert st["shade_hits"] == oc["shade_hits"]


def _equals_base(dev, name, rad, fb, st, **kw):
    """Bit for bit the device's frame of the base scene (its original material
    table, no extra triangle) under the same arguments."""
    brad, bfb, bst = _render(dev, V.base_name(name), keep=True, **kw)
    assert np.array_equal(_bits(rad), _bits(brad))
    assert np.array_equal(fb, bfb)
    assert st["traversals"] == bst["traversals"] and st["shade_hits"] == bst["shade_hits"]


def _bvh_equals_oracle(dev, name):
    ts, d = dev(name)
    _, (onodes, okeys, owv, own) = V.oracle_bvh(name)
    wv, wn = d.read_world()
    assert np.array_equal(_bits(wv), _bits(owv))
    assert np.array_equal(_bits(wn), _bits(own))
    nodes, keys = d.read_bvh()
    n_int = ts.n_faces - 1
    assert len(nodes) == 2 * ts.n_faces - 1
    assert np.array_equal(keys, okeys)
    assert np.array_equal(nodes["parent"], onodes["parent"])
    assert np.array_equal(nodes["a"], onodes["a"])
    assert np.array_equal(nodes["b"][:n_int], onodes["b"][:n_int])
    assert np.array_equal(_bits(nodes["bmin"]), _bits(onodes["bmin"]))
    assert np.array_equal(_bits(nodes["bmax"]), _bits(onodes["bmax"]))


_oracle_hits = {}


def _rays_and_oracle_hits(name, boundary=False):
    """The scene's ray set (at most 4,096 rays) and orc_trace_ray's answers, once."""
    if name not in _oracle_hits:
        s = V.scene(name)
        ps, built = V.oracle_bvh(name)
        W, H = V.frame_of(name)[:2]
        o, d = V.boundary_rays(s, ps, built)[:2] if boundary else V.generic_rays(s, built[2], W, H)
        assert len(o) <= 4096
        _oracle_hits[name] = (o, d) + V.oracle_trace(ps, o, d, built)
    return _oracle_hits[name]


def _trace_equals(got, want, min_hits):
    h, t, uv = got
    oh, ot, ouv = want
    assert np.array_equal(h, oh), int((h != oh).sum())
    m = oh >= 0
    assert m.sum() >= min_hits
    assert np.array_equal(_bits(t[m]), _bits(ot[m]))
    assert np.array_equal(_bits(uv[m]), _bits(ouv[m]))


def _aov_equals_oracle(dev, name, keys):
    ts, d = dev(name)
    W, H = V.frame_of(name)[:2]
    got = T.PathTracer("", W, H, 0).renderAOV(d, ts.m_camera)
    want = post_ref.oracle_aov(V.oracle_bvh(name)[0], W, H)
    assert (want["face"] >= 0).mean() > 0.05
    for k in keys:
        if got[k].dtype == np.float32:
            assert np.array_equal(_bits(got[k]), _bits(want[k])), k
        else:
            assert np.array_equal(got[k], want[k]), k
    return got, want


# --------------------------------------------------------------------------
# material table placement
# --------------------------------------------------------------------------
@pytest.mark.parametrize("order,lanes", [("ordered", 1), ("ordered", 4), ("ordered", 0), ("reference", 1),
                                         ("reference", 0)])
@pytest.mark.parametrize("n", V.MATERIAL_COUNTS)
def test_material_table_in_global_memory(dev, n, order, lanes):
    """k_trace's MTL_LDS = false instantiations (trace.hip launch_trace: the table
    goes to LDS while (n_materials + 1) * 32 <= TPT_MTL_LDS_MAX = 2048, so 63
    materials are the last LDS table and 64, 65 and 200 read a.mtl): box with one
    lane per pixel, four (the QUAD variants; not offered in the reference order) and
    the host's choice, in the ordered walk and the reference's order.  The frame is
    the oracle's, and the frame of box with its own six materials: the real
    materials sit at ids n - 6 .. n - 1 among decoys, so an id wrapped or truncated
    on the way to the table shows."""
    name = f"box_m{n}"
    rad, fb, st = _render(dev, name, ORDERS[order], lanes)
    _equals_oracle(name, rad, fb, st)
    _equals_base(dev, name, rad, fb, st, flags=ORDERS[order], lanes=lanes)
    if lanes and not FORCED_WAVEFRONT:
        assert st["lanes_per_pixel"] == lanes


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("n", V.MATERIAL_COUNTS)
def test_material_table_in_global_memory_delta_light(dev, n, lanes):
    """The LIGHTS = true variants with MTL_LDS = false (TPT_MTL_LDS_MAX), one lane and
    pair mode: square (a spot light; its faces take the Material() slot, id n, the
    entry past the table) -- 5-word records with the id in bits 0-29, in pair mode
    masked with 0x7fff."""
    name = f"square_m{n}"
    rad, fb, st = _render(dev, name, 0, lanes)
    _equals_oracle(name, rad, fb, st)
    _equals_base(dev, name, rad, fb, st, lanes=lanes)
    if not FORCED_WAVEFRONT:
        assert st["lanes_per_pixel"] == lanes


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("n", V.MATERIAL_COUNTS)
def test_material_table_in_global_memory_env_is(dev, n, lanes):
    """The env-IS variants without an LDS material table (TPT_MTL_LDS_MAX; the
    "eight ordered env-IS variants" of trace_dev.hpp): ball under the procedural sky
    with TPT_FLAG_ENV_IS, one lane and pair mode."""
    name = f"ball_m{n}"
    rad, fb, st = _render(dev, name, 0, lanes, env_is=True)
    _equals_oracle(name, rad, fb, st, env_is=True)
    _equals_base(dev, name, rad, fb, st, lanes=lanes, env_is=True)


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("name", ["tir_m64", "box_m64_deep"])
def test_material_table_in_global_memory_at_max_depth_64(dev, name, order):
    """The MAXD = 64 variants with MTL_LDS = false (TPT_MTL_LDS_MAX: 64 materials):
    max_depth 64, so the path records past the LDS levels spill to private memory.
    tir (its lamp widened, variant_scenes.tir_lit) and box, whose closed room
    keeps paths alive past depth 8 (6.1 rays per sample against 4.5)."""
    rad, fb, st = _render(dev, name, ORDERS[order], 1)
    _equals_oracle(name, rad, fb, st)
    _equals_base(dev, name, rad, fb, st, flags=ORDERS[order], lanes=1)


@pytest.mark.parametrize("name", ["box_m200", "square_m64"])
def test_material_table_in_global_memory_wavefront(dev, name):
    """TPT_FLAG_WAVEFRONT (wavefront.hip reads the table from global memory always;
    its records pack ids as k_trace's do): 200 materials on box, 64 and a delta
    light on square -- past TPT_MTL_LDS_MAX either way."""
    rad, fb, st = _render(dev, name, T._lib.FLAG_WAVEFRONT)
    _equals_oracle(name, rad, fb, st)
    _equals_base(dev, name, rad, fb, st, flags=T._lib.FLAG_WAVEFRONT)


def test_material_ids_in_the_feature_buffers(dev):
    """k_aov's material and albedo planes with 200 materials (ids 194..199 among
    decoys, past TPT_MTL_LDS_MAX's 63): equal to tests/post_ref.py's."""
    got, want = _aov_equals_oracle(dev, "box_m200", ("material", "albedo", "face", "depth", "normal"))
    assert got["material"].max() == 199 and got["material"][got["face"] >= 0].min() >= 194


# --------------------------------------------------------------------------
# record words
# --------------------------------------------------------------------------
@pytest.mark.parametrize("order,lanes", [("ordered", 1), ("ordered", 0), ("reference", 1), ("reference", 0)])
@pytest.mark.parametrize("n", V.RECORD_COUNTS)
def test_record_word_boundary(dev, n, order, lanes):
    """rec_words (trace_variant.hpp): the 2-word path records pack the material id in
    bits 0-14 and the probe's material in bits 15-29 with kNoProbe = 0x7fff, so
    from n_materials = 0x7ffe on the records have 5 words.  n = 0x7ffd is the last
    packed table: the emitter is id 0x7ffc and the Material() slot 0x7ffd.
    n = 0x7ffe takes LIGHTS = true with n_lights = 0."""
    name = f"box_m{n}"
    rad, fb, st = _render(dev, name, ORDERS[order], lanes)
    _equals_oracle(name, rad, fb, st)
    _equals_base(dev, name, rad, fb, st, flags=ORDERS[order], lanes=lanes)
    if n == 0x7ffe and not FORCED_WAVEFRONT:
        assert st["lanes_per_pixel"] == 1       # no four-lane variant with 5-word records


def test_record_word_boundary_quad(dev):
    """Four lanes per pixel need the 2-word records: at 0x7ffd materials they run (and
    pack probe id 0x7ffc); at 0x7ffe the host refuses them, as
    test_quad_refused_where_the_one_lane_logic_does_not_apply expects elsewhere."""
    rad, fb, st = _render(dev, "box_m32765", 0, 4)
    _equals_oracle("box_m32765", rad, fb, st)
    if not FORCED_WAVEFRONT:
        assert st["lanes_per_pixel"] == 4
        with pytest.raises(T.TPTError):
            _render(dev, "box_m32766", 0, 4)


@pytest.mark.parametrize("n,ran", [(0x7ffd, 2), (0x7ffe, 1)])
def test_record_word_boundary_delta_light(dev, n, ran):
    """Pair mode packs the material id in 15 bits as well (launch_trace: pair needs
    n_materials + 1 < kNoProbe).  square's faces take the Material() slot, id n:
    0x7ffd is the last id pair mode carries; at 0x7ffe lanes_per_pixel = 2 runs one
    lane per pixel, and the stats say so."""
    name = f"square_m{n}"
    rad, fb, st = _render(dev, name, 0, 2)
    _equals_oracle(name, rad, fb, st)
    _equals_base(dev, name, rad, fb, st, lanes=2)
    if not FORCED_WAVEFRONT:
        assert st["lanes_per_pixel"] == ran


# --------------------------------------------------------------------------
# stack-id width
# --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [32768, 32769])
def test_stack_id_width_build_and_rays(dev, n):
    """launch_trace: 2F - 1 <= 65535 selects uint16_t stack entries.  F = 32,768
    has 65,535 nodes and takes the StackT = uint16_t variants, with node id 65,534
    pushed and popped (it is a ray's closest hit, test_variant_scenes_cpu.py);
    F = 32,769 has 65,537 and takes StackT = int.  The build and single rays
    (k_trace_rays keeps int entries: the ids' width is the render's)."""
    name = f"faces_{n}"
    _bvh_equals_oracle(dev, name)
    o, d, oh, ot, ouv = _rays_and_oracle_hits(name, boundary=True)
    ts, dv = dev(name)
    for mode in (0, 1):
        _trace_equals(dv.trace_rays(o, d, mode=mode), (oh, ot, ouv), 500)
    assert (oh == V.oracle_bvh(name)[1][0]["a"][-1]).sum() >= 1      # the last leaf is hit


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("n", [32768, 32769])
def test_stack_id_width_frames(dev, n, order):
    """F = 32,768: k_trace<..., StackT = uint16_t> (ids up to 65,534 in 16 bits);
    F = 32,769: StackT = int -- 65535 is the bound.  (The reference order always
    runs the int variant.)"""
    name = f"faces_{n}"
    rad, fb, st = _render(dev, name, ORDERS[order], 1)
    _equals_oracle(name, rad, fb, st)


# --------------------------------------------------------------------------
# deep LBVH
# --------------------------------------------------------------------------
CHAINS = ["chain_up", "chain_down", "chain_up_inf", "chain_down_inf"]


@pytest.mark.parametrize("name", CHAINS)
def test_deep_lbvh_build_and_rays(dev, name):
    """LaneStack::deep in k_trace_rays: kRaysLdsSlots = 48 stack slots per lane are
    in LDS, and the chain's walks hold up to 61 entries (test_variant_scenes_cpu.py),
    so put() and get() take their private branch, and inner_visit4_q pushes across
    sp + 3 > nlds.  The LBVH (depth 60; stack_depth = depth + 2 = 62 in the _inf
    scenes, the wide tree's need otherwise, far below the refusal at 160) bit for
    bit; mode 0 against the oracle; modes 1-3 against mode 0."""
    _bvh_equals_oracle(dev, name)
    o, d, oh, ot, ouv = _rays_and_oracle_hits(name)
    ts, dv = dev(name)
    h0, t0, uv0 = dv.trace_rays(o, d, mode=0)
    _trace_equals((h0, t0, uv0), (oh, ot, ouv), 500)
    h1, t1, uv1 = dv.trace_rays(o, d, mode=1)
    _trace_equals((h1, t1, uv1), (h0, t0, uv0), 500)
    _check_modes(ts, dv, o, d, h0, t0, uv0)


@pytest.mark.parametrize("name", CHAINS)
def test_deep_lbvh_feature_buffers(dev, name):
    """k_aov's LaneStack::deep: kAovLdsSlots = 48 (as kRaysLdsSlots) of the chain's
    up to 61 entries are in LDS, the rest private."""
    _aov_equals_oracle(dev, name, ("face", "depth"))


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("name", CHAINS)
def test_deep_lbvh_frames(dev, name, order):
    """k_trace on a depth-60 LBVH: trace_lds_layout sizes the LDS stack from
    stack_depth (kRaysLdsSlots' counterpart in the render), the reference order
    defers a node per level, and in the _inf scenes (boxes_finite == 0) the ordered
    walk is the binary one at full depth."""
    rad, fb, st = _render(dev, name, ORDERS[order], 1)
    _equals_oracle(name, rad, fb, st)


def test_deep_lbvh_wavefront(dev):
    """wavefront.hip's stack on the chain (deeper than kRaysLdsSlots' 48 too)."""
    rad, fb, st = _render(dev, "chain_down", T._lib.FLAG_WAVEFRONT)
    _equals_oracle("chain_down", rad, fb, st)


# --------------------------------------------------------------------------
# non-finite boxes on real content
# --------------------------------------------------------------------------
@pytest.mark.parametrize("order,lanes", [("ordered", 1), ("ordered", 0), ("reference", 1)])
def test_non_finite_boxes_frame(dev, order, lanes):
    """boxes_finite == 0 (build.hip k_pack_inner; api_scene.cpp skips the SAH wide
    tree and the sliver pass): every ordered walk of box takes the binary LBVH path
    (Trav::fin false), with one lane per pixel and with the host's choice of lanes.
    The frame is the oracle's and plain box's: the triangle with the +inf vertex is
    never hit."""
    rad, fb, st = _render(dev, "box_inf", ORDERS[order], lanes)
    _equals_oracle("box_inf", rad, fb, st)
    brad, bfb, _ = _render(dev, "box", ORDERS[order], lanes, keep=True)
    assert np.array_equal(_bits(rad), _bits(brad)) and np.array_equal(fb, bfb)
    if order == "ordered":
        assert st["wide_visits"] == 0                # no 4-wide node was visited


def test_non_finite_boxes_build_rays_and_feature_buffers(dev):
    """boxes_finite == 0: the build (the +inf boxes bit for bit), k_trace_rays mode 1
    and k_aov on the binary path."""
    _bvh_equals_oracle(dev, "box_inf")
    o, d, oh, ot, ouv = _rays_and_oracle_hits("box_inf")
    _trace_equals(dev("box_inf")[1].trace_rays(o, d, mode=1), (oh, ot, ouv), 500)
    _aov_equals_oracle(dev, "box_inf", ("face", "depth", "material", "albedo", "normal"))


# --------------------------------------------------------------------------
# one, two, three triangles
# --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3])
def test_tiny_scene_build_rays_and_feature_buffers(dev, n):
    """nint == 0 (F = 1: the root is a leaf; launch_build, scene_build and the walks
    guard on n > 1, there is no wide tree, emit_root stays -1 and cull_eps 0) and the
    smallest trees with inner nodes (F = 2, 3)."""
    name = f"tiny{n}"
    _bvh_equals_oracle(dev, name)
    ts, dv = dev(name)
    assert len(dv.read_bvh()[0]) == 2 * n - 1
    o, d, oh, ot, ouv = _rays_and_oracle_hits(name)
    h0, t0, uv0 = dv.trace_rays(o, d, mode=0)
    _trace_equals((h0, t0, uv0), (oh, ot, ouv), 150)
    _trace_equals(dv.trace_rays(o, d, mode=1), (h0, t0, uv0), 150)
    _check_modes(ts, dv, o, d, h0, t0, uv0)
    _aov_equals_oracle(dev, name, ("face", "depth", "material", "albedo", "normal"))


@pytest.mark.parametrize("order,lanes", [("ordered", 0), ("ordered", 1), ("reference", 0), ("reference", 1)])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_tiny_scene_frames(dev, n, order, lanes):
    """k_trace with nint == 0 (F = 1) and on two- and three-leaf trees, the host's
    lane choice (four lanes per pixel at this size) and one lane."""
    name = f"tiny{n}"
    rad, fb, st = _render(dev, name, ORDERS[order], lanes)
    _equals_oracle(name, rad, fb, st)
