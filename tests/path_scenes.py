"""Scenes for tpt_render_aov_path (tests/test_path_scenes_cpu.py states their premises
on the CPU, tests/test_gpu_aov_path.py runs the device on them): box2 with some of its
materials turned into perfect mirrors, built with tests/variant_scenes.py's builders.

  hall         the red and the blue side wall are white mirrors (metallic 1, base colour
               1): two facing planar mirrors, so chains of reflections reach any cap;
  tinted       the same with the walls' base colours as shipped, (1, 0, 0) and
               (0, 0, 0.8): the albedo product is not the terminal albedo alone;
  lamp_mirror  box2 with its emitter's material also metallic: the path stops there;
  tilted       tinted with the mirror walls' vertex normals tilted off their planes."""
import copy

import numpy as np

from tests import variant_scenes as V

F = np.float32
BASE_COLOR, EMISSION, ETA, METALLIC = slice(0, 3), 3, 4, 5   # columns of a material row
WALLS = ("redWall", "blueWall")


def _box2():
    s = V.base_scene("box2")
    out = copy.copy(s)
    out.materials = np.array(s.materials, F).reshape(-1, 15).copy()
    return out


def material_id(s, name):
    return s.material_names.index(name)


def _hall(white):
    s = _box2()
    for name in WALLS:
        m = material_id(s, name)
        assert s.materials[m, EMISSION] == 0 and not s.materials[m, ETA] > 0
        s.materials[m, METALLIC] = F(1.0)
        if white:
            s.materials[m, BASE_COLOR] = F(1.0)
    return s


def hall():
    return _hall(True)


def tinted():
    return _hall(False)


def emitter_ids(s):
    return [m for m in range(len(s.materials)) if s.materials[m, EMISSION] > 0]


def lamp_mirror():
    s = _box2()
    ids = emitter_ids(s)
    assert ids
    for m in ids:
        s.materials[m, METALLIC] = F(1.0)
    return s


TILT = (0.2, 0.15, 0.3)                                     # parallel to no wall's normal


def tilted():
    """`tinted` with the vertex normals of the two mirror walls pushed by TILT (up to
    0.4 rad off the plane's normal): the walls stay flat, so pixels stay comparable, but
    the shading normal the reflection uses is no longer the geometric one."""
    s = tinted()
    s.normals = np.array(s.normals, F).reshape(-1, 3).copy()
    idx = np.asarray(s.indices).reshape(-1, 3)
    begins = [int(b) for b in s.lut[:, 0]] + [len(idx)]
    for o, m in enumerate(s.lut[:, 1]):
        if 0 <= int(m) < len(s.material_names) and s.material_names[int(m)] in WALLS:
            v = np.unique(idx[begins[o]:begins[o + 1]])
            n = s.normals[v] + np.asarray(TILT, F)
            s.normals[v] = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F)
    return s


SCENES = {"box2": _box2, "hall": hall, "tinted": tinted, "lamp_mirror": lamp_mirror, "tilted": tilted}


def scene(name):
    return SCENES[name]()
