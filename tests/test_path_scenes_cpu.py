"""The premises of tests/test_gpu_aov_path.py, stated with the oracle alone (no GPU):
what the path scenes' materials are, how many pixels are comparable, how many of them
follow a mirror, and how deep the chains between the hall's two mirrors go."""
import numpy as np

from tests import path_ref as P
from tests import path_scenes as S
from tests import variant_scenes as V


def _mirror_pixels(ps, ref):
    mir = P.is_mirror(P.material_table(ps))
    fm = ref["first_material"]
    return (fm >= 0) & mir[np.maximum(fm, 0)]


def test_scene_materials():
    box2 = S.scene("box2")
    hall, tinted, lamp = S.scene("hall"), S.scene("tinted"), S.scene("lamp_mirror")
    for name, colour in (("redWall", (1.0, 0.0, 0.0)), ("blueWall", (0.0, 0.0, 0.8))):
        m = S.material_id(box2, name)
        assert box2.materials[m, S.METALLIC] == 0                       # diffuse as shipped
        assert np.allclose(box2.materials[m, S.BASE_COLOR], colour)
        assert hall.materials[m, S.METALLIC] == 1 and (hall.materials[m, S.BASE_COLOR] == 1).all()
        assert tinted.materials[m, S.METALLIC] == 1
        assert np.array_equal(tinted.materials[m, S.BASE_COLOR], box2.materials[m, S.BASE_COLOR])
    ids = S.emitter_ids(box2)
    assert len(ids) == 1 and box2.materials[ids[0], S.METALLIC] == 0
    assert lamp.materials[ids[0], S.METALLIC] == 1 and lamp.materials[ids[0], S.EMISSION] > 0
    # the emitter is metallic, yet no mirror: it ends the path
    assert not P.is_mirror(P.material_table(V.oracle_scene(lamp)))[ids[0]]
    assert P.is_mirror(P.material_table(V.oracle_scene(lamp)), emitter_terminal=False)[ids[0]]
    assert np.array_equal(box2.indices, hall.indices) and np.array_equal(box2.vertices, tinted.vertices)


def test_hall_premises():
    """128 x 72, max_bounces 3.  Measured: 75.0 % comparable; 1,425 mirror pixels, 492 of
    them comparable; bounces 0 / 1 / 2 / 3: 7,791 / 1,176 / 122 / 127."""
    ps = V.oracle_scene(S.scene("hall"))
    ref = P.oracle_aov_path(ps, 128, 72, 3)
    ok = P.comparable(ref)
    mir = _mirror_pixels(ps, ref)
    hist = np.bincount(ref["bounces"].ravel(), minlength=4)
    print(f"hall: comparable {ok.mean():.3f}; mirror pixels {mir.sum()}, comparable {(mir & ok).sum()}; "
          f"bounces {hist.tolist()}")
    assert ok.mean() >= 0.7
    assert (mir & ok).sum() >= 300
    assert hist[2] >= 50 and hist[3] >= 50 and len(hist) == 4
    assert ((ref["bounces"] > 0) == mir).all()             # every mirror pixel is followed, nothing else is
    capped = ref["bounces"] == 3
    cm = ref["material"][capped]
    assert (cm >= 0).any() and P.is_mirror(P.material_table(ps))[cm[cm >= 0]].any()   # some end on a mirror at the cap


def test_box2_premises():
    """256 x 144, max_bounces 8.  Measured: 86.5 % comparable; 2,397 mirror pixels (its
    cube), 1,395 comparable, 921 of those with a terminal hit; 671 mirror pixels end in a miss."""
    ps = V.oracle_scene(S.scene("box2"))
    ref = P.oracle_aov_path(ps, 256, 144, 8)
    ok = P.comparable(ref)
    mir = _mirror_pixels(ps, ref)
    hit = mir & ok & (ref["face"] >= 0)
    miss = mir & (ref["face"] < 0)
    print(f"box2: comparable {ok.mean():.3f}; mirror pixels {mir.sum()}, comparable {(mir & ok).sum()}, "
          f"with a terminal hit {hit.sum()}; mirror pixels ending in a miss {miss.sum()}")
    assert ok.mean() >= 0.7
    assert (mir & ok).sum() >= 300
    assert hit.sum() >= 300 and (miss & ok).sum() >= 50
    assert (ref["depth"][miss] > 0).all() and (ref["normal"][miss] == 0).all()


def test_lamp_mirror_premises():
    ps = V.oracle_scene(S.scene("lamp_mirror"))
    ref = P.oracle_aov_path(ps, 128, 72, 8)
    lamp = S.emitter_ids(ps.src)[0]
    first = ref["first_material"] == lamp
    print(f"lamp_mirror: {first.sum()} pixels see the emitter first")
    assert first.sum() >= 20
    assert (ref["bounces"][first] == 0).all()
    loose = P.oracle_aov_path(ps, 128, 72, 8, knock="emitter")
    assert (loose["bounces"][first] > 0).all()             # what the rule prevents


def test_box_has_no_comparable_mirror_pixel():
    """box's mirror is a finely tessellated sphere: neighbouring pixels reflect off other
    faces, so the parity tests use box2 and the hall."""
    from oracle import oracle as O
    from tests.conftest import scene_path
    ps = O.load_scene(scene_path("box"))
    ref = P.oracle_aov_path(ps, 96, 54, 8)
    mir = _mirror_pixels(ps, ref)
    print(f"box 96 x 54: mirror pixels {mir.sum()}, comparable {(mir & P.comparable(ref)).sum()}")
    assert mir.sum() >= 100
    assert (mir & P.comparable(ref)).sum() == 0


def test_no_bounce_is_the_first_hit():
    """max_bounces 0 restates post_ref.oracle_aov bit for bit."""
    from tests import post_ref as R
    ps = V.oracle_scene(S.scene("tinted"))
    a = P.oracle_aov_path(ps, 64, 36, 0)
    b = R.oracle_aov(ps, 64, 36)
    for k in ("albedo", "normal", "depth", "face", "material"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert (a["bounces"] == 0).all()


def test_mirror_direction_is_the_reference_s():
    """orc_kat_new_direction (getNewDirection) on a metal returns path_ref.reflect's bits,
    attenuation 1 and probability 1, and draws no random number."""
    from oracle import oracle as O
    rng = np.random.default_rng(5)
    d = P.R.normalize(rng.normal(size=(64, 3)).astype(np.float32))
    n = P.R.normalize(rng.normal(size=(64, 3)).astype(np.float32))
    cases = np.concatenate([d, n, np.zeros((64, 1), np.float32), np.ones((64, 1), np.float32)], 1).astype(np.float32)
    states = np.tile(np.asarray(O.xorwow_stream(1, 0, 6), np.uint32), (64, 1))
    out, after = O.kat_new_direction(cases, states)
    assert np.array_equal(np.ascontiguousarray(out[:, :3]).view(np.uint32), P.reflect(d, n).view(np.uint32))
    assert (out[:, 3:] == 1.0).all() and np.array_equal(after, states)


def test_which_shipped_scenes_have_no_mirror():
    """tir and ball have none, so tpt_render_aov_path must equal tpt_render_aov on them at any
    cap.  box1 has one: its whitWall leaves metallicFactor out, and glTF's default is 1."""
    from oracle import oracle as O
    from tests.conftest import scene_path
    for name, expect in (("tir", False), ("ball", False), ("box1", True)):
        ps = O.load_scene(scene_path(name))
        ref = P.oracle_aov_path(ps, 64, 36, 8)
        hits = (ref["first_face"] >= 0).mean()
        print(f"{name}: bounces {np.bincount(ref['bounces'].ravel()).tolist()}, first hits {hits:.3f}")
        assert (ref["bounces"] > 0).any() == expect and hits > 0.02
    box1 = O.load_scene(scene_path("box1"))
    m = box1.src.material_names.index("whitWall")
    assert box1.src.materials[m][5] == 1.0
