"""The conditions that keep tests/test_gpu_variants.py from passing vacuously,
asserted with the oracle alone (no GPU).  Each scene of tests/variant_scenes.py is
there to carry a device kernel across one branch; here the scene is shown to be on
the far side of it, and a device that took the wrong side is shown to render
another frame.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import post_ref
from tests import variant_scenes as V


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _render(s, name):
    W, H, spp, depth, env = V.frame_of(name)
    return O.render(V.oracle_scene(s), W, H, spp, depth, 42, env=V.sky()[::-1].copy() if env else None,
                    trig_mode=1)[0]


# what a device that lost bits of a material id would index
REMAPS = {"mod 64": lambda m: m % 64,                       # an LDS table of 64 entries indexed with id & 63
          "14 bits": lambda m: m & 0x3fff,                  # the packed id masked one bit short
          "15 bits, top bit dropped": lambda m: (m & 0x7fff) & ~0x4000}


@pytest.mark.parametrize("name", ["box_m65", "box_m200", "box_m32765", "box_m32766", "tir_m64", "square_m64",
                                  "square_m65", "square_m200", "square_m32765", "square_m32766", "ball_m64",
                                  "ball_m200"])
def test_decoys_show_a_truncated_material_id(name):
    """Every remap that moves an id an object uses changes the oracle's frame in at
    least 10 % of the pixels whose centre ray hits geometry; `mod 64` moves one in
    every scene here with more than 64 materials, the masks in the scenes with ids
    above 0x3fff.  (The real materials sit at the highest ids, so with 64 or fewer
    none of these remaps moves an id: box_m63 and box_m64 are held to the frame of
    plain box instead, test_gpu_variants.py.  tir_m64's objects use ids 61..63;
    the Material() slot, id 64, is what `mod 64` would wrap, and no object takes
    it, so tir_m64 is checked with `mod 32`.)"""
    s = V.scene(name)
    W, H = V.frame_of(name)[:2]
    ref = V.oracle_frame(name)[0]
    hit = post_ref.oracle_aov(V.oracle_scene(s), W, H)["face"] >= 0
    assert hit.sum() >= 40
    used = sorted({int(m) for m in s.lut[:, 1]})
    remaps = dict(REMAPS)
    if name == "tir_m64":
        remaps = {"mod 32": lambda m: m % 32}
    moved = 0
    for label, f in remaps.items():
        if all(f(m) == m for m in used):
            continue
        moved += 1
        rad = _render(V.remap_materials(s, f), name)
        changed = (_bits(rad) != _bits(ref)).any(-1) & hit
        assert changed.sum() >= 0.10 * hit.sum(), (name, label, int(changed.sum()), int(hit.sum()))
    n = len(s.materials)
    assert moved >= (3 if n > 0x3fff else 1), (name, moved)


@pytest.mark.parametrize("base", ["box", "square", "ball", "tir"])
def test_grown_material_table_keeps_the_frame(base):
    """The real materials only move: the oracle's frame of every many-material scene
    equals the frame of its base scene bit for bit, and the decoys differ from every
    real material in colour and in emission."""
    names = [k for k in V.SCENES if k.startswith(base + "_m")]
    assert names
    for name in names:
        s = V.scene(name)
        ref = V.oracle_frame(V.base_name(name))[0]
        assert np.array_equal(_bits(V.oracle_frame(name)[0]), _bits(ref)), name
        real = s.materials[s.meta["real_ids"]] if s.meta["real_ids"] else np.zeros((0, 15), np.float32)
        decoys = np.delete(s.materials, s.meta["real_ids"], axis=0)
        assert len(decoys) == s.meta["n_decoys"] > 0
        every = np.concatenate([real, V.material_row((0.82, 0.67, 0.16))[None]])   # and the Material() slot
        for r in every:
            assert not (decoys[:, :3] == r[:3]).all(1).any() and not (decoys[:, 3] == r[3]).any(), name


def test_emissive_material_takes_the_top_id():
    """n = 0x7ffd: the emitter is material 0x7ffc, the largest probe id the 2-word
    records pack, and the Material() slot is 0x7ffd, below kNoProbe = 0x7fff.
    n = 0x7ffe: one more each, and rec_words switches to 5 words."""
    for n in V.RECORD_COUNTS:
        s = V.scene(f"box_m{n}")
        assert len(s.materials) == n
        emit = np.nonzero(s.materials[:, 3] == 6.0)[0]
        assert emit.tolist() == [n - 1] and n - 1 in s.lut[:, 1]
        assert s.meta["real_ids"] == list(range(n - 6, n))
        # a probe id masked to 14 bits would read a decoy's emission, not the lamp's
        assert s.materials[(n - 1) & 0x3fff, 3] == np.float32(0.375) != s.materials[n - 1, 3]
    assert 0x7ffd - 1 >= 0x7ffc and 0x7ffd < 0x7fff
    sq = V.scene("square_m32766")
    assert (sq.lut[:, 1] == 0x7ffe).all() and len(sq.lights) == 1     # the Material() slot, a delta light


@pytest.mark.parametrize("direction", ["up", "down"])
def test_chain_has_depth_60(direction):
    s = V.scene(f"chain_{direction}")
    assert s.n_faces == 61
    nodes, keys, _, _ = O.build_bvh(V.oracle_scene(s))       # accepted: no duplicate-key cycle
    assert len(set(keys.tolist())) == 61
    assert V.tree_depth(nodes) == V.CHAIN_DEPTH == 60
    assert np.isfinite(nodes["bmin"]).all() and np.isfinite(nodes["bmax"]).all()
    step = np.sort(np.abs(keys - (keys[0] if direction == "up" else keys[-1])))
    assert step.tolist() == [0] + [1 << k for k in range(60)]


def test_chain_fills_more_than_the_lds_stack_slots():
    """48 is kRaysLdsSlots (trace.hip, k_trace_rays) and kAovLdsSlots (post.hip,
    k_aov): a lane's stack entries from the 49th on live in LaneStack::deep.  The
    reference's right-first walk over the oracle's nodes holds at least 49 entries
    for at least 64 of the test's rays in at least one direction (it is "down": the
    lone leaf of every level is the left child and waits)."""
    enough = {}
    for direction in ("up", "down"):
        name = f"chain_{direction}"
        s = V.scene(name)
        nodes = O.build_bvh(V.oracle_scene(s))[0]
        o, d = V.camera_rays(s, *V.frame_of(name)[:2])
        occ = V.dfs_max_occupancy(nodes, s.n_faces, o, d)
        enough[direction] = int((occ >= 49).sum())
        assert occ.max() <= 62                               # stack_depth = tree depth + 2
    assert max(enough.values()) >= 64, enough


def test_dfs_restatement_agrees_with_the_oracle_on_box():
    """The restated walk visits what orc_trace_ray visits: its box test, applied to
    the leaves the oracle's rays hit, passes every one of them."""
    s = V.scene("box")
    ps = V.oracle_scene(s)
    built = O.build_bvh(ps)
    o, d = V.camera_rays(s, 16, 9)
    hit, _, _ = V.oracle_trace(ps, o, d, built)
    leaf_of = np.zeros(s.n_faces, np.int64)
    leaf_of[built[0]["a"][s.n_faces - 1:]] = np.arange(s.n_faces - 1, 2 * s.n_faces - 1)
    passes = V.box_hits(built[0], o, d)
    assert (hit >= 0).sum() > 30
    for r in np.nonzero(hit >= 0)[0]:
        node = leaf_of[hit[r]]
        while True:
            assert passes[r, node]
            if node == 0:
                break
            node = int(built[0]["parent"][node])


@pytest.mark.parametrize("n,n_nodes", [(32768, 65535), (32769, 65537)])
def test_face_counts_at_the_stack_id_width(n, n_nodes):
    """65,535 nodes is the last count whose ids fit uint16_t stack entries."""
    name = f"faces_{n}"
    s = V.scene(name)
    assert s.n_faces == n
    ps = V.oracle_scene(s)
    built = O.build_bvh(ps)                                  # accepted
    assert len(built[0]) == n_nodes == 2 * n - 1
    if n == 32768:
        o, d, last_fid = V.boundary_rays(s, ps, built)
        assert len(o) <= 4096
        hit, _, _ = V.oracle_trace(ps, o, d, built)
        assert built[0]["a"][65534] == last_fid
        assert (hit == last_fid).sum() >= 1                  # node 65,534, the largest 16-bit id pushed, wins a ray
        assert (hit >= 0).mean() > 0.5


@pytest.mark.parametrize("name", sorted(V.SCENES))
def test_frames_are_covered_and_finite(name):
    """At least a quarter of every test frame's pixels carry radiance, so a frame
    comparison compares light.  Two bases were reshaped to get there, not the
    bound: square is seen through a 0.4 x lens (15 % -> 61 %), and tir through the
    same lens with its lamp 4 x as wide and deep, at 8 spp (0.5 % -> 48 %);
    variant_scenes.BASES."""
    rad = V.oracle_frame(name)[0]
    assert np.isfinite(rad).all()
    assert (rad.max(-1) > 0).mean() >= 0.25, float((rad.max(-1) > 0).mean())


@pytest.mark.parametrize("name", ["box_inf", "chain_up_inf", "chain_down_inf"])
def test_inf_scenes_have_a_non_finite_box_and_no_nan(name):
    """boxes_finite == 0 on the device needs a node box that is not finite.  The
    triangle sits in an object of its own rather than in the last object, with a
    matrix without zeros, and its vertex is +inf in all three coordinates: through
    box's own matrices a (+inf, y, z) vertex becomes NaN in two coordinates
    (0 * inf), and NaN's bit pattern is the host's, so the boxes could not be
    compared bit for bit."""
    s = V.scene(name)
    ps = V.oracle_scene(s)
    nodes, _, wv, wn = O.build_bvh(ps)
    assert np.isinf(nodes["bmax"]).any() and np.isinf(nodes["bmax"][0]).all()
    assert not np.isnan(nodes["bmin"]).any() and not np.isnan(nodes["bmax"]).any()
    assert not np.isnan(wv).any() and np.isfinite(wn).all()
    assert np.isinf(wv[-1]).all() and np.isfinite(wv[:-1]).all()


def test_inf_triangle_is_never_hit():
    """box_inf renders plain box's frame bit for bit (mean 0.29683709 at 32 x 18 x 4)."""
    a, b = V.oracle_frame("box_inf")[0], V.oracle_frame("box")[0]
    assert np.array_equal(_bits(a), _bits(b))
    assert abs(float(a.mean()) - 0.29683709) < 1e-7


@pytest.mark.parametrize("n", [1, 2, 3])
def test_tiny_scenes_build(n):
    s = V.scene(f"tiny{n}")
    assert s.n_faces == n
    nodes, keys, _, _ = O.build_bvh(V.oracle_scene(s))
    assert len(nodes) == 2 * n - 1 and len(set(keys.tolist())) == n
    assert s.materials[s.lut[0, 1], 3] > 0                   # the first triangle emits


@pytest.mark.parametrize("base", ["box", "square", "ball", "tir"])
def test_both_hosts_get_the_same_arrays(base):
    """Scene.from_arrays over the oracle's arrays is the scene the native loader
    makes of the file: arrays, lights, camera, and the tpt_scene_desc built from it."""
    import tinypathtracer_amd as T
    from tests.conftest import scene_path
    want = T.Scene(scene_path(base))
    got = V.device_scene(V.base_scene(base))
    for k in ("indices", "vertices", "normals", "lut", "vert_trans", "normal_trans", "materials"):
        a, b = getattr(got, k), getattr(want, k)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    assert [bytes(L) for L in got.lights] == [bytes(L) for L in want.lights]
    assert np.array_equal(_bits(got.m_camera.c2w), _bits(want.m_camera.c2w))
    assert (got.m_camera.vfov, got.m_camera.aspect, got.m_camera.znear) == \
        (want.m_camera.vfov, want.m_camera.aspect, want.m_camera.znear)
    assert got.missing_material == want.missing_material
    d = got.desc()
    assert (d.n_faces, d.n_vertices, d.n_objects, d.n_materials, d.n_lights) == \
        (want.n_faces, len(want.vertices), len(want.lut), len(want.materials), len(want.lights))


def test_from_arrays_refuses_inconsistent_arrays():
    import tinypathtracer_amd as T
    s = V.base_scene("tir")
    args = [s.indices, s.vertices, s.normals, s.lut, s.vert_trans, s.normal_trans, s.materials]
    with pytest.raises(ValueError):
        T.Scene.from_arrays(s.indices[:-1], *args[1:])
    with pytest.raises(ValueError):
        T.Scene.from_arrays(s.indices + np.uint32(len(s.vertices)), *args[1:])
    with pytest.raises(ValueError):
        T.Scene.from_arrays(*args[:4], s.vert_trans[:-1], *args[5:])
