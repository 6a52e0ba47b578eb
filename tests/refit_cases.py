"""The scenes, poses and ray sets of the refit tests (tests/test_refit_cpu.py shows on the CPU that
the ray sets hold almost no near-ties; tests/test_gpu_refit.py traces them).

Scenes, the smallest at which each step of tpt_scene_refit can go wrong:
  two         two triangles: one LBVH inner node, one 4-wide node
  sheet       tests/deform_scenes.py's 130 triangles: several levels, less than one block
  sheet_emit  the same with an emissive material on the 128 sheet triangles: a multi-level emissive tree
  box         box.gltf, 1,932 faces: several 256-thread blocks; ball1 displaced as tpt_render --wave does
A scene is a dict of the arrays Scene.from_arrays takes, `camera`, `poses`: name -> (vertices,
normals) of the whole scene, and for the sheet `matrices`: name -> vert_trans (a pose by
tpt_scene_set_transforms alone).

A ray set is about 4,000 rays: the pixel-centre rays of a small camera and seeded random origins
and directions through the scene's bounds.  usable() drops the rays a refit may legitimately
answer differently from a rebuild: those whose two nearest hits, found by testing every triangle
in float64, lie within 1e-4 relative of each other."""
import functools

import numpy as np

from tests import deform_scenes as DS
from tests import post_ref as R
from tests import temporal_ref as TR
from tests import variant_scenes as VS
from tests.conftest import scene_path

F = np.float32
BALL1 = 5                       # box.gltf's object "ball1" (tests/test_motion_api.py)
WAVE_AMP = 0.05
CAM_W, CAM_H = 48, 40           # 1,920 pixel-centre rays
N_RANDOM = 2080
T_MIN = 1e-4                    # a hit counts from here on
TIE_REL = 1e-4
SCENES = ("two", "sheet", "sheet_emit", "box")


def _eye(n):
    return np.tile(np.eye(4, dtype=F).reshape(16), (n, 1))


def _two():
    v = np.array([[-1.0, -1.0, -3.0], [1.0, -1.0, -3.0], [0.0, 1.0, -3.0],
                  [-0.6, -0.8, -4.0], [1.2, -0.4, -4.5], [0.2, 1.1, -4.2]], F)
    n = np.tile(np.array([0.0, 0.0, 1.0], F), (6, 1))
    moved = v.copy()
    moved[2] += np.array([0.4, 0.3, 0.5], F)
    moved[3] += np.array([-0.5, 0.0, 0.7], F)
    far = v.copy()
    far[:3] += np.array([0.9, -0.2, -2.5], F)      # the front triangle goes behind the other
    mats = np.stack([VS.material_row((0.8, 0.6, 0.4)), VS.material_row((0.3, 0.5, 0.7), emission=2.0)])
    return dict(indices=np.arange(6, dtype=np.uint32), vertices=v, normals=n, lut=np.array([[0, 0], [1, 1]], np.int32),
                vert_trans=_eye(2), materials=mats, camera=TR.camera(),
                poses={"moved": (moved, n), "far": (far, n)})


SLIVER_QUAD = (3, 3)            # the sheet quad whose first triangle the pose "sliver" flattens


def sliver_pose():
    """The bulged sheet with one vertex moved: corner c of the quad's triangle (a, b, c) goes to
    a + 1.6 (b - a) plus 1e-4 |b - a| sideways, so the sine of the angle at v0 = a drops to
    6e-5, below the 1e-3 of the sliver criterion (trace.hip "Culling").  On the bulge, not at
    rest: there the stretched neighbours would lie in the plane of the triangles they overlap."""
    v, n = DS.deformed(DS.bulge)
    j, i = SLIVER_QUAD
    a = j * (DS.QUADS + 1) + i
    b, c = a + 1, a + DS.QUADS + 2
    v = v.copy()
    e = v[b].astype(np.float64) - v[a]
    side = np.cross(e, [0.0, 0.0, 1.0])
    v[c] = (v[a] + 1.6 * e + 1e-4 * side).astype(F)
    return v, n


def _sheet(emissive):
    idx, v, n, lut = DS.rest()
    mats = np.stack([VS.material_row((0.8, 0.6, 0.4), emission=1.5 if emissive else 0.0),
                     VS.material_row((0.3, 0.5, 0.7), emission=2.0)])
    poses = {"bend": DS.deformed(DS.bend), "half": DS.deformed(DS.half), "bulge": DS.deformed(DS.bulge),
             "sliver": sliver_pose()}
    return dict(indices=idx, vertices=v, normals=n, lut=lut, vert_trans=_eye(2), materials=mats, camera=TR.camera(),
                poses=poses, matrices={"turned": sheet_turned()})


def sheet_turned():
    """A pose by tpt_scene_set_transforms alone: the sheet's object shifted and turned by 5 degrees
    about y through its centre; vert_trans of both objects [2, 16]."""
    from tests import motion_ref as MR
    vt = _eye(2)
    vt[0] = MR.col_major(MR.translation((0.08, 0.05, 0.1)) @ MR.rotation_y(5.0, centre=(0.0, 0.0, DS.Z_SHEET)))
    return vt


def _box():
    import tinypathtracer_amd as T
    s = T.Scene(scene_path("box"))
    v, n = np.asarray(s.vertices, F).reshape(-1, 3), np.asarray(s.normals, F).reshape(-1, 3)
    poses = {}
    for frame in (1, 4):
        first, pv = DS.wave(s, BALL1, WAVE_AMP, frame)
        w = v.copy()
        w[first:first + len(pv)] = pv
        poses[f"wave{frame}"] = (w, n)
    c = s.m_camera
    cam = {"c2w": np.asarray(c.c2w, F).reshape(16), "vfov": float(c.vfov), "aspect": float(c.aspect)}
    return dict(indices=np.asarray(s.indices, np.uint32), vertices=v, normals=n,
                lut=np.asarray(s.lut, np.int32).reshape(-1, 2), vert_trans=np.asarray(s.vert_trans, F).reshape(-1, 16),
                normal_trans=np.asarray(s.normal_trans, F).reshape(-1, 16), materials=np.asarray(s.materials, F),
                camera=cam, poses=poses)


@functools.lru_cache(maxsize=None)
def scene(name):
    return {"two": _two, "sheet": lambda: _sheet(False), "sheet_emit": lambda: _sheet(True), "box": _box}[name]()


def make(name, vertices=None, normals=None):
    """The scene as a tinypathtracer_amd.Scene, at rest or with these arrays."""
    import tinypathtracer_amd as T
    from tests import test_gpu_temporal as G
    sc = scene(name)
    s = T.Scene.from_arrays(sc["indices"], sc["vertices"] if vertices is None else vertices,
                            sc["normals"] if normals is None else normals, sc["lut"], sc["vert_trans"],
                            sc.get("normal_trans", sc["vert_trans"]).copy(), sc["materials"])
    s.m_camera = G._cam(sc["camera"])
    return s


def world(name, vertices, vert_trans=None):
    """World-space corners [F, 3, 3] in float64 (each object's matrix applied to its faces;
    vert_trans None: the scene's own)."""
    sc = scene(name)
    tri = sc["indices"].reshape(-1, 3).astype(np.int64)
    v = np.asarray(vertices, np.float64)
    begin = sc["lut"][:, 0].astype(np.int64)
    obj = np.searchsorted(begin, np.arange(len(tri)), side="right") - 1
    m = np.asarray(sc["vert_trans"] if vert_trans is None else vert_trans).astype(np.float64)
    m = m.reshape(-1, 4, 4).transpose(0, 2, 1)                                         # column-major -> [o, row, col]
    p = v[tri]                                                                         # [F, 3, 3]
    return np.einsum("fij,fcj->fci", m[obj][:, :3, :3], p) + m[obj][:, None, :3, 3]


@functools.lru_cache(maxsize=None)
def rays(name):
    """(origins [n, 3], directions [n, 3]) float32: the same for every pose of a scene."""
    sc = scene(name)
    cam = sc["camera"]
    o, d = R.pixel_centre_rays(cam["c2w"], cam["vfov"], cam["aspect"], CAM_W, CAM_H)
    d = d.reshape(-1, 3)
    o = np.tile(np.asarray(o, F), (len(d), 1))
    corners = np.concatenate([world(name, sc["vertices"]).reshape(-1, 3)] +
                             [world(name, pv).reshape(-1, 3) for pv, _ in sc["poses"].values()] +
                             [world(name, sc["vertices"], vt).reshape(-1, 3) for vt in sc.get("matrices", {}).values()])
    lo, hi = corners.min(0), corners.max(0)
    rng = np.random.default_rng(20 + SCENES.index(name))
    size = (hi - lo).max()
    ro = rng.uniform(lo - 0.25 * size, hi + 0.25 * size, (N_RANDOM, 3))
    # half of them aimed at a point of the bounds, half anywhere
    aim = rng.uniform(lo, hi, (N_RANDOM, 3)) - ro
    free = rng.normal(size=(N_RANDOM, 3))
    rd = np.where((np.arange(N_RANDOM) % 2 == 0)[:, None], aim, free)
    rd /= np.linalg.norm(rd, axis=-1, keepdims=True)
    return np.concatenate([o, ro.astype(F)]), np.concatenate([d, rd.astype(F)])


def two_nearest(corners, o, d):
    """Every triangle against every ray in float64 (rayHitTriangle's test): the two smallest
    accepted t per ray, inf where there is none."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    t1 = np.full(len(o), np.inf)
    t2 = np.full(len(o), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for v0, v1, v2 in corners:
            e1, e2, tv = v1 - v0, v2 - v0, o - v0
            p = np.cross(d, e2)
            q = np.cross(tv, e1)
            den = p @ e1
            u, w, t = (p * tv).sum(-1) / den, (d * q).sum(-1) / den, (q @ e2) / den
            ok = (den != 0) & (u >= 0) & (w >= 0) & (u + w <= 1) & (t > T_MIN)
            t = np.where(ok, t, np.inf)
            t2 = np.where(t < t1, t1, np.minimum(t2, t))
            t1 = np.minimum(t1, t)
    return t1, t2


@functools.lru_cache(maxsize=None)
def nearest(name, pose):
    """two_nearest of rays(name) against the scene under `pose`: None (at rest), a name of its
    `poses` (vertices) or of its `matrices` (the rest vertices under other vert_trans)."""
    sc = scene(name)
    o, d = rays(name)
    if pose in sc.get("matrices", {}):
        return two_nearest(world(name, sc["vertices"], sc["matrices"][pose]), o, d)
    v = sc["vertices"] if pose is None else sc["poses"][pose][0]
    return two_nearest(world(name, v), o, d)


def usable(name, pose):
    """The rays of rays(name) kept for `pose`: a boolean mask."""
    t1, t2 = nearest(name, pose)
    second = np.where(np.isfinite(t2), t2, 0.0)            # (no second hit: no tie)
    first = np.where(np.isfinite(t2), t1, 0.0)
    tie = np.isfinite(t2) & (second - first <= TIE_REL * first)
    return ~tie
