"""The conditions that keep tests/test_gpu_lit.py from passing vacuously, asserted
with the oracle alone (no GPU).  Each scene of tests/lit_scenes.py is there to
carry the device's delta-light code across one rule; here the lights are shown to
light what they are meant to light, the order of the lights to show in the bits,
and a device that mixed the lights up to render another frame.
"""
import numpy as np
import pytest

from tests import lit_scenes as L
from tests import variant_scenes as V

LIT = [n for n in L.SCENES if n != "box_dark"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _changed(a, b):
    """bool [H, W]: the pixels whose radiance bits differ."""
    return (_bits(a) != _bits(b)).any(-1)


@pytest.mark.parametrize("name", LIT)
def test_lit_enough(name):
    """The lights change at least a fifth of the frame's pixels (box's geometry
    covers 47 % of its frame, and all of that changes; ball is seen through a
    0.6 x lens to get there: 20 % -> 56 %)."""
    rad = L.oracle_frame(name)[0]
    assert np.isfinite(rad).all()
    share = _changed(rad, L.unlit_frame(name)[0]).mean()
    assert share >= 0.20, share


@pytest.mark.parametrize("name", ["box_l3", "box_l16", "ball_l4"])
def test_every_light_counts(name):
    """Each added light, rendered alone, changes at least 1 % of the unlit frame's
    pixels: none sits inside a ball, behind a wall or with the room outside its cone."""
    unlit = L.unlit_frame(name)[0]
    keep = L.unlit(name).lights
    added = L.added_lights(name)
    assert len(added) == {"box_l3": 3, "box_l16": 16, "ball_l4": 3}[name]
    for i, light in enumerate(added):
        rad = L.render(L.relit(name, keep + [light]), name)[0]
        share = _changed(rad, unlit).mean()
        assert share >= 0.01, (i, light["type"], share)


def test_light_lists():
    """box_l3 has one light of each type; box_l16 has kMaxLights = 16 of mixed types
    with distinct intensities and colours, box_l16r the same list reversed, box_l15
    the list without its last light; ball_l4 keeps ball's own light first."""
    assert [x["type"] for x in L.scene("box_l3").lights] == [0, 1, 2]
    l16 = L.scene("box_l16").lights
    assert len(l16) == 16 and {x["type"] for x in l16} == {0, 1, 2}
    assert len({float(x["intensity"]) for x in l16}) == 16
    assert len({tuple(float(c) for c in x["color"]) for x in l16}) == 16
    assert L.scene("box_l16r").lights == l16[::-1]
    assert L.scene("box_l15").lights == l16[:15]
    ball = L.scene("ball_l4").lights
    assert len(ball) == 4 and ball[0] == V.base_scene("ball").lights[0]
    assert sorted(x["type"] for x in ball) == [0, 0, 1, 2]
    assert len(L.scene("faces_32769_l1").lights) == 1 and L.scene("faces_32769_l1").lights[0]["type"] == 1
    assert L.scene("box_l3_sky").lights == L.scene("box_l3").lights and L.frame_of("box_l3_sky")[4] == "sky"


def test_last_light_counts():
    """box_l16 against box_l15: a light loop that stopped one short renders another frame."""
    assert _changed(L.oracle_frame("box_l16")[0], L.oracle_frame("box_l15")[0]).sum() >= 1


def test_the_order_of_the_lights_shows():
    """box_l16 and box_l16r are the same picture, and only the order of the fp32
    direct sum tells them apart: other bits in at least 1 % of the pixels (27 %
    here), by less than 1e-5 (4.8e-7 here)."""
    a, b = L.oracle_frame("box_l16")[0], L.oracle_frame("box_l16r")[0]
    share = _changed(a, b).mean()
    assert share >= 0.01, share
    assert np.abs(a.astype(np.float64) - b.astype(np.float64)).max() < 1e-5


def test_every_material_is_lit():
    """box_l3's pixels grouped by the material of their first hit: at least 4 pixels
    of the glass ball (eta 2), of the glossy ball (metallic 1) and of a diffuse wall
    differ from the unlit frame; and at least 4 diffuse ones that differ carry
    radiance in the unlit frame too -- paths that reach the lamp and are lit as well."""
    s = L.scene("box_l3")
    aov = L.first_hits("box_l3")
    mat = aov["material"]
    mats = s.materials
    glass = [m for m in range(len(mats)) if mats[m, 4] >= 1.0]                  # eta
    glossy = [m for m in range(len(mats)) if mats[m, 5] > 0.0]                  # metallic
    diffuse = [m for m in range(len(mats)) if mats[m, 4] == 0.0 and mats[m, 5] == 0.0 and mats[m, 3] == 0.0]
    assert len(glass) == 1 and len(glossy) == 1 and len(diffuse) == 3
    lit, unlit = L.oracle_frame("box_l3")[0], L.unlit_frame("box_l3")[0]
    ch = _changed(lit, unlit)
    assert (ch & np.isin(mat, glass)).sum() >= 4
    assert (ch & np.isin(mat, glossy)).sum() >= 4
    assert (ch & np.isin(mat, diffuse)).sum() >= 4
    assert (ch & np.isin(mat, diffuse) & (unlit.max(-1) > 0)).sum() >= 4
    # an emitter is in the frame too: the lamp is some pixels' first hit
    assert (np.isin(mat, [m for m in range(len(mats)) if mats[m, 3] > 0.0])).sum() >= 1


def test_box_dark_is_the_unlit_frame():
    """Three lights that add nothing: the radiance bits and the BGRA bytes are the
    unlit frame's, and the shadow rays are traced all the same."""
    rad, bgra, cnt = L.oracle_frame("box_dark")
    urad, ubgra, ucnt = L.unlit_frame("box_dark")
    assert np.array_equal(_bits(rad), _bits(urad))
    assert np.array_equal(bgra, ubgra)
    assert cnt["traversals"] > ucnt["traversals"]
    assert (urad.max(-1) > 0).mean() >= 0.25


def test_box_dark_lights_are_dark_for_three_reasons():
    """Of the first bounce's shadow rays: the zero-intensity light's and the averted
    spot light's leave the room unoccluded for a tenth of the rays at least (it is
    the intensity and the cone that keep them dark), and every ray towards the
    light inside the glossy ball is occluded.  The same lights with the intensity
    set, the spot turned round and the third one moved out of the ball do light
    the room."""
    sr = L.shadow_rays("box_dark")
    for li in (0, 1):
        assert (sr["hit"][sr["light"] == li] < 0).mean() >= 0.10, li
    assert (sr["hit"][sr["light"] == 2] >= 0).all()
    dark = L.scene("box_dark").lights
    assert dark[0]["intensity"] == 0 and dark[1]["type"] == 2 and dark[2]["intensity"] > 0
    fixed = [L.point(dark[0]["pos"], 2000.0), L.spot(dark[1]["pos"], (0.0, 1.0, 0.0), 9000.0, 0.42, 0.2),
             L.point((0.3, 1.0, 3.0), 3000.0)]
    urad = L.unlit_frame("box_dark")[0]
    for i, light in enumerate(fixed):
        assert _changed(L.render(L.relit("box_dark", [light]), "box_dark")[0], urad).mean() >= 0.20, i


@pytest.mark.parametrize("name", sorted(L.SCENES))
def test_ray_counts(name):
    """Lights draw no random numbers, so the paths are the unlit ones: shade_hits
    stays, and every shaded hit traces one shadow ray per light."""
    cnt, ucnt = L.oracle_frame(name)[2], L.unlit_frame(name)[2]
    n = len(L.added_lights(name))
    assert n >= 1
    assert cnt["shade_hits"] == ucnt["shade_hits"] > 0
    assert cnt["traversals"] == ucnt["traversals"] + n * ucnt["shade_hits"]


@pytest.mark.parametrize("name", L.ENV_IS_SCENES)
def test_ray_counts_with_env_is(name):
    """The same relation against the unlit env-IS frame; and env IS does change the frame."""
    cnt, ucnt = L.oracle_frame(name, True)[2], L.unlit_frame(name, True)[2]
    n = len(L.added_lights(name))
    assert cnt["shade_hits"] == ucnt["shade_hits"] > 0
    assert cnt["traversals"] == ucnt["traversals"] + n * ucnt["shade_hits"]
    assert cnt["traversals"] > L.oracle_frame(name)[2]["traversals"]
    assert _changed(L.oracle_frame(name, True)[0], L.oracle_frame(name)[0]).mean() >= 0.20


def test_box_wall_lights_lie_in_their_walls_planes():
    """box_wall: at least 10 % of the frame's pixels have their first hit on a face
    whose plane contains one of the two lights (|n . (p - light)| <= 1e-6, the
    face's fp64 unit normal) -- every shadow ray from there to that light leaves
    its face in the face's own plane -- and at least 4 of those pixels differ from
    the unlit frame.  Each light lies in its own wall's plane and in no other face's."""
    s = L.scene("box_wall")
    assert len(s.lights) == 2
    ends = list(s.lut[1:, 0]) + [s.n_faces]
    through = [L.faces_through("box_wall", light) for light in s.lights]
    for light_faces, obj in zip(through, (L.FLOOR_OBJECT, L.BACK_WALL_OBJECT)):
        assert np.flatnonzero(light_faces).tolist() == list(range(s.lut[obj, 0], ends[obj]))
    face = L.first_hits("box_wall")["face"]
    in_plane = (face >= 0) & (through[0] | through[1])[np.maximum(face, 0)]
    assert in_plane.mean() >= 0.10, in_plane.mean()
    ch = _changed(L.oracle_frame("box_wall")[0], L.unlit_frame("box_wall")[0])
    assert (ch & in_plane).sum() >= 4
    for light_faces in through:                                # each wall on its own, too
        assert (ch & (face >= 0) & light_faces[np.maximum(face, 0)]).sum() >= 4


@pytest.mark.parametrize("name", ["box_wall", "tir_l2"])
def test_shadow_ray_sets(name):
    """The rays tests/test_gpu_lit.py traces on their own: at most 4,096, occluded
    and unoccluded ones both; a tenth at least of box_wall's leave a face whose
    plane contains the light they aim at."""
    sr = L.shadow_rays(name)
    n = len(sr["hit"])
    assert 200 <= n <= 4096
    assert (sr["hit"] >= 0).sum() >= 20 and (sr["hit"] < 0).sum() >= 20
    assert np.isfinite(sr["dirs"]).all()
    if name == "box_wall":
        assert L.grazing_share(name) >= 0.10, L.grazing_share(name)


def test_tir_l2_lights_the_glass():
    """tir_l2 (max_depth 64): at least 4 changed pixels have the glass slab (eta 2,
    object 0) as their first hit."""
    s = L.scene("tir_l2")
    assert L.frame_of("tir_l2")[3] == 64
    mat = L.first_hits("tir_l2")["material"]
    glass = int(s.lut[0, 1])
    assert s.materials[glass, 4] == 2.0
    ch = _changed(L.oracle_frame("tir_l2")[0], L.unlit_frame("tir_l2")[0])
    assert (ch & (mat == glass)).sum() >= 4


def test_faces_32769_l1_needs_wide_stack_ids():
    s = L.scene("faces_32769_l1")
    assert s.n_faces == 32769 and 2 * s.n_faces - 1 > 65535


def test_box_m64_l3_is_box_l3():
    """64 materials (past the LDS table) with the real ones at ids 58..63: the
    oracle's frame is box_l3's bit for bit."""
    s = L.scene("box_m64_l3")
    assert len(s.materials) == 64 and s.meta["real_ids"] == list(range(58, 64))
    assert s.lights == L.scene("box_l3").lights
    a, b = L.oracle_frame("box_m64_l3"), L.oracle_frame("box_l3")
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1])
    assert a[2]["traversals"] == b[2]["traversals"]


def test_a_wrong_device_renders_another_frame():
    """Teeth: box_l3 with its lights rotated by one position (the same set, summed
    in another order), and with light 2's type field changed from spot to point,
    are other frames than box_l3's."""
    ref = L.oracle_frame("box_l3")[0]
    lights = L.scene("box_l3").lights
    rotated = L.render(L.relit("box_l3", lights[1:] + lights[:1]), "box_l3")[0]
    assert _changed(rotated, ref).sum() >= 1
    assert np.abs(rotated.astype(np.float64) - ref).max() < 1e-5       # the same picture
    as_point = [dict(x) for x in lights]
    assert as_point[2]["type"] == 2
    as_point[2]["type"] = 0
    retyped = L.render(L.relit("box_l3", as_point), "box_l3")[0]
    assert _changed(retyped, ref).mean() >= 0.01
