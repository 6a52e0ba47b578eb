"""In-memory scenes with delta lights next to emitters, real materials and each
other (tests/test_lit_scenes_cpu.py states their premises with the oracle alone,
tests/test_gpu_lit.py runs the device against the oracle on them; DESIGN.md
section 4 "Parity" lists the rule each one crosses).

The shipped scenes with a delta light (ball: one point light, square: one spot
light) have no material table and no emitter, so every oracle-checked render with
lights takes one trip of the light loop, the NOEMIT pair kernel and the Material()
slot.  The scenes here are shipped scenes with lists of lights added, built on
tests/variant_scenes.py's helpers.

How a light reaches a surface here: the reference's shadow ray has no far end
(path_tracer.cu:265-286, any hit along the whole ray occludes) and the light is
added without a cosine.  box is a room open towards the camera (+z), so a light
counts where the ray towards it leaves through the opening: the lights stand in
front of the room, and a directional light's direction has a negative z.
"""
import copy
import math

import numpy as np

from oracle import oracle as O
from oracle import scene as oscene
from tests import variant_scenes as V

F = np.float32


# --------------------------------------------------------------------------
# lights, as oracle/scene.py load_gltf makes them
# --------------------------------------------------------------------------
def _f3(v):
    return [F(x) for x in v]


def _unit(v):
    v = np.asarray(v, np.float64)
    return _f3(v / np.linalg.norm(v))


def point(pos, lumens, color=(1.0, 1.0, 1.0)):
    return dict(type=oscene.LIGHT_POINT, color=_f3(color), intensity=F(F(lumens) * oscene.WATTS_PER_LUMEN),
                pos=_f3(pos), direction=_f3((0, 0, 0)), cos_outer=F(0), inv_cos_cone_diff=F(0))


def directional(direction, intensity, color=(1.0, 1.0, 1.0)):
    """`direction` is the way the light travels; the shadow ray goes the other way."""
    return dict(type=oscene.LIGHT_DIRECTIONAL, color=_f3(color), intensity=F(intensity), pos=_f3((0, 0, 0)),
                direction=_unit(direction), cos_outer=F(0), inv_cos_cone_diff=F(0))


def spot(pos, target, lumens, outer=0.7853981634, inner=0.0, color=(1.0, 1.0, 1.0)):
    """A spot light at pos looking at target; the cone terms as load_gltf computes them."""
    co = F(math.cos(float(F(outer))))
    ci = F(math.cos(float(F(inner))))
    return dict(type=oscene.LIGHT_SPOT, color=_f3(color), intensity=F(F(lumens) * oscene.WATTS_PER_LUMEN),
                pos=_f3(pos), direction=_unit(np.asarray(target, np.float64) - np.asarray(pos, np.float64)),
                cos_outer=co, inv_cos_cone_diff=F(F(1.0) / F(ci - co)))


def with_lights(base, lights, keep=True):
    """`base` (a scene's name in variant_scenes, or an OracleScene) with `lights`
    after its own (keep) or instead of them."""
    s = copy.copy(V.scene(base) if isinstance(base, str) else base)
    s.lights = copy.deepcopy((list(s.lights) if keep else []) + list(lights))
    return s


# --------------------------------------------------------------------------
# the light lists
# --------------------------------------------------------------------------
def lights_l3():
    """One light of each type, in the order point, directional, spot."""
    return [point((0.9, 1.6, 3.5), 2400.0, (1.0, 0.85, 0.7)),
            directional((0.35, -0.3, -1.0), 0.3, (0.6, 0.8, 1.0)),
            spot((-1.2, 1.0, 4.0), (0.0, 0.7, 0.0), 9000.0, 0.42, 0.2, (0.8, 1.0, 0.75))]


def lights_l16():
    """16 lights in front of the room: types point, spot, directional in turn,
    no two intensities or colours alike."""
    out = []
    for i in range(16):
        a, b, c = (i * 0.6180339887) % 1.0, (i * 0.7548776662) % 1.0, (i * 0.5698402910) % 1.0
        pos = (-1.4 + 2.8 * a, 0.4 + 1.9 * b, 2.6 + 2.0 * c)
        color = (0.35 + 0.65 * c, 0.35 + 0.65 * a, 0.35 + 0.65 * b)
        if i % 3 == 0:
            out.append(point(pos, 500.0 + 70.0 * i, color))
        elif i % 3 == 1:
            out.append(spot(pos, (0.6 * math.sin(i), 0.8, -0.2), 1500.0 + 130.0 * i, 0.45, 0.15, color))
        else:
            out.append(directional((0.5 - pos[0] * 0.4, 0.6 - pos[1] * 0.5, -1.0), 0.03 + 0.004 * i, color))
    return out


GLOSSY_BALL_CENTRE = (-0.45, 0.4, -0.45)   # box's object 5 (metallic 1): x, z -0.85..-0.05, y 0..0.8


def lights_dark():
    """Three lights that add nothing to box, each for another reason: a point light
    of intensity 0 in plain sight (its shadow rays leave the room, it adds 0); a
    spot light in front of the room that looks away from it (the room is outside
    its outer cone: falloff 0); a point light at the centre of the glossy ball,
    which every shadow ray fails to reach unoccluded (a ray towards a point inside
    a closed mesh goes on through the mesh's far side, from any origin -- the
    ball's own faces included).  A light below the floor would not do here: the
    shadow rays of the floor's own points go down and meet nothing, and the
    reference adds a delta light without a cosine."""
    return [point((0.3, 1.2, 3.5), 0.0),
            spot((0.0, 1.0, 4.0), (0.0, 1.0, 9.0), 9000.0, 0.42, 0.2),
            point(GLOSSY_BALL_CENTRE, 3000.0, (1.0, 0.5, 0.25))]


FLOOR_OBJECT, BACK_WALL_OBJECT = 1, 4      # box's objects: y = 0 and z = -1


def lights_wall():
    """A point light in the floor's plane, in front of the room, and one in the back
    wall's plane, beside the room: the plane coordinate is the world vertex's the
    oracle's transform gives for the object's first vertex."""
    s = V.scene("box")
    wv = O.transform(V.oracle_scene(s))[0]
    tri = s.indices.reshape(-1, 3)
    y_floor = float(wv[tri[s.lut[FLOOR_OBJECT, 0], 0], 1])
    z_back = float(wv[tri[s.lut[BACK_WALL_OBJECT, 0], 0], 2])
    return [point((0.2, y_floor, 3.0), 2600.0, (1.0, 0.9, 0.8)),
            point((2.6, 1.2, z_back), 2600.0, (0.7, 0.9, 1.0))]


def lights_tir():
    return [point((1.5, 1.5, 2.0), 2000.0, (1.0, 0.8, 0.6)),
            directional((0.3, -0.5, -0.8), 0.25, (0.7, 0.85, 1.0))]


def lights_ball():
    """On top of ball's own point light: a directional, a spot and a second point light."""
    return [directional((-0.4, -0.8, -0.45), 0.2, (1.0, 0.9, 0.7)),
            spot((2.0, 3.0, 2.0), (0.0, 0.8, 0.0), 12000.0, 0.5, 0.25, (0.7, 0.8, 1.0)),
            point((-2.0, 1.5, 1.5), 2200.0, (0.9, 1.0, 0.8))]


def lights_faces():
    return [directional((0.3, -0.35, -1.0), 0.35, (1.0, 0.9, 0.8))]


# --------------------------------------------------------------------------
# the scenes by name: builder, then the frame both hosts render
# (width, height, samples per pixel, max depth, "sky" for the procedural env)
# --------------------------------------------------------------------------
_BOX = (32, 18, 4, 8, None)        # 18 rows: a partial 8-row pair-mode tile
SCENES = {
    "box_l3": (lambda: with_lights("box", lights_l3()),) + _BOX,
    "box_l16": (lambda: with_lights("box", lights_l16()),) + _BOX,
    "box_l16r": (lambda: with_lights("box", lights_l16()[::-1]),) + _BOX,
    "box_l15": (lambda: with_lights("box", lights_l16()[:-1]),) + _BOX,
    "box_dark": (lambda: with_lights("box", lights_dark()),) + _BOX,
    "box_wall": (lambda: with_lights("box", lights_wall()),) + _BOX,
    "tir_l2": (lambda: with_lights(V.tir_lit(), lights_tir()), 32, 18, 8, 64, None),
    "box_m64_l3": (lambda: V.with_materials(scene("box_l3"), 64),) + _BOX,
    # ball through a 0.6 x lens: at the shipped lens its geometry covers 18 % of a 32 x 18 frame
    "ball_l4": (lambda: with_lights(V.zoomed("ball", 0.6), lights_ball()), 32, 18, 4, 8, "sky"),
    "box_l3_sky": (lambda: scene("box_l3"), 32, 18, 4, 8, "sky"),
    "faces_32769_l1": (lambda: with_lights(V.faces_exactly(32769), lights_faces()),) + _BOX,
}
ENV_IS_SCENES = ("ball_l4", "box_l3_sky")
N_SHIPPED_LIGHTS = {"ball_l4": 1}          # the lights the base scene came with: unlit() keeps them

_built = {}


def scene(name) -> oscene.OracleScene:
    """SCENES[name], built once per process."""
    if name not in _built:
        _built[name] = SCENES[name][0]()
    return _built[name]


def frame_of(name):
    return SCENES[name][1:]


def unlit(name) -> oscene.OracleScene:
    """The scene without the lights added here (ball_l4 keeps ball's own point light)."""
    return relit(name, scene(name).lights[:N_SHIPPED_LIGHTS.get(name, 0)])


def relit(name, lights) -> oscene.OracleScene:
    """The scene with another list of lights."""
    s = copy.copy(scene(name))
    s.lights = copy.deepcopy(list(lights))
    return s


def added_lights(name):
    return scene(name).lights[N_SHIPPED_LIGHTS.get(name, 0):]


def render(s, name, env_is=False):
    """The oracle's frame of scene `s` at `name`'s test size, seed 42: (radiance, bgra, counters)."""
    W, H, spp, depth, env = frame_of(name)
    return O.render(V.oracle_scene(s), W, H, spp, depth, 42, env=V.sky()[::-1].copy() if env else None, trig_mode=1,
                    env_is=env_is)


_frames = {}


def _cached(key, s, name, env_is):
    if key not in _frames:
        rad, bgra, cnt = render(s(), name, env_is)
        rad.setflags(write=False)
        bgra.setflags(write=False)
        _frames[key] = (rad, bgra, cnt)
    return _frames[key]


def oracle_frame(name, env_is=False):
    """The oracle's frame of a named scene, rendered once per process.  Read-only."""
    return _cached((name, env_is), lambda: scene(name), name, env_is)


def unlit_frame(name, env_is=False):
    """The oracle's frame of unlit(name), rendered once per process.  Read-only."""
    return _cached((name, env_is, "unlit"), lambda: unlit(name), name, env_is)


_bvhs = {}


def oracle_bvh(name):
    """(PackedScene, (nodes, keys, world vertices, world normals)) of a named scene, once per process."""
    if name not in _bvhs:
        ps = V.oracle_scene(scene(name))
        _bvhs[name] = (ps, O.build_bvh(ps))
    return _bvhs[name]


_aovs = {}


def first_hits(name):
    """tests/post_ref.py's first-hit buffers of the pixel-centre rays (face, material, depth ...), once."""
    if name not in _aovs:
        from tests import post_ref
        W, H = frame_of(name)[:2]
        _aovs[name] = post_ref.oracle_aov(oracle_bvh(name)[0], W, H)
    return _aovs[name]


# --------------------------------------------------------------------------
# shadow rays on their own
# --------------------------------------------------------------------------
def light_dirs(light, points):
    """The oracle's light_sample direction (orc_kat_light) from every point to one light."""
    L = O.lib()
    C = O.C
    lt = O.Light(int(light["type"]), (C.c_float * 3)(*[float(x) for x in light["color"]]), float(light["intensity"]),
                 (C.c_float * 3)(*[float(x) for x in light["pos"]]),
                 (C.c_float * 3)(*[float(x) for x in light["direction"]]), float(light["cos_outer"]),
                 float(light["inv_cos_cone_diff"]))
    out = np.zeros((len(points), 3), F)
    d3, r3 = (C.c_float * 3)(), (C.c_float * 3)()
    for i, p in enumerate(np.asarray(points, F)):
        L.orc_kat_light(C.byref(lt), (C.c_float * 3)(*[float(x) for x in p]), d3, r3)
        out[i] = d3[:]
    return out


_shadow = {}


def shadow_rays(name):
    """The shadow rays of the first bounce of a named scene's pixel-centre rays, and
    the oracle's answers, once per process: the oracle's first-hit points
    (origin + t * direction in float32, the render's own step), from each the
    light_sample direction to every light of the scene.  Returns a dict: origins,
    dirs [n, 3]; face [n] the face each ray leaves; light [n] the light's index;
    hit, t, uv the oracle's trace of them."""
    if name not in _shadow:
        s = scene(name)
        ps, built = oracle_bvh(name)
        W, H = frame_of(name)[:2]
        o, d = V.camera_rays(s, W, H)
        hit, t, _ = V.oracle_trace(ps, o, d, built)
        m = hit >= 0
        p = (o[m] + t[m, None] * d[m]).astype(F)
        origins = np.concatenate([p] * len(s.lights))
        dirs = np.concatenate([light_dirs(L, p) for L in s.lights])
        face = np.concatenate([hit[m]] * len(s.lights))
        light = np.repeat(np.arange(len(s.lights)), int(m.sum()))
        h2, t2, uv2 = V.oracle_trace(ps, origins, dirs, built)
        _shadow[name] = dict(origins=origins, dirs=dirs, face=face, light=light, hit=h2, t=t2, uv=uv2)
    return _shadow[name]


def grazing_share(name):
    """The share of shadow_rays(name) that leave a face whose plane contains the light they aim at."""
    sr = shadow_rays(name)
    through = np.stack([faces_through(name, light) for light in scene(name).lights])     # [lights, faces]
    return float(through[sr["light"], sr["face"]].mean())


def faces_through(name, light, tol=1e-6):
    """bool per face: the face's plane contains the light's position, |n . (p - light)| <= tol
    with the face's unit normal in float64."""
    s = scene(name)
    wv = oracle_bvh(name)[1][2].astype(np.float64)
    tri = wv[s.indices.reshape(-1, 3).astype(np.int64)]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    pos = np.array([float(x) for x in light["pos"]], np.float64)
    return np.abs(((tri[:, 0] - pos) * n).sum(1)) <= tol
