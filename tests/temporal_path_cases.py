"""What tests/test_temporal_path_cpu.py and tests/test_gpu_temporal_path.py share: the
scenes, the translated cameras, the frames and the cases of tpt_temporal_path's tests.

The camera moves by 3 % of the median first-hit depth along x, 0.4 of that along y and 0.2
along z (hall: 6.69 -> (0.2007, 0.0803, 0.0401)): a yaw about the eye leaves every eye ray
where it was, so only a translation shows what first-hit reprojection does to a mirror."""
import numpy as np

from tests import path_ref as P
from tests import path_scenes as S
from tests import temporal_path_ref as TP
from tests import variant_scenes as V

F = np.float32
PARAMS = dict(alpha=0.1, depth_tol=0.1, normal_min=0.9, max_history=32)
POINT_TOL = 1.0                      # pixel footprints
# The device tests' bound on max|gpu - ref| / max|ref|: ten times the largest value measured on
# an MI355X (tests/test_gpu_temporal_path.py's header has the measurements).
GPU_MEASURED_MAX = 5.464e-6           # variance, hall 80 x 45 two frames, demodulated, frame 2
GPU_BOUND = 10 * GPU_MEASURED_MAX
MOVE = np.array([1.0, 0.4, 0.2]) * 0.03
# name -> (builder of the oracle's scene source, cap)
SCENES = {"hall": (lambda: S.scene("hall"), 3), "box2": (lambda: V.base_scene("box2"), 8),
          "tilted": (lambda: S.scene("tilted"), 3), "box": (lambda: V.base_scene("box"), 8),
          "tir": (lambda: V.base_scene("tir"), 8), "tinted": (lambda: S.scene("tinted"), 3)}

_SRC, _PS, _TRACER, _WALK = {}, {}, {}, {}


def source(name):
    if name not in _SRC:
        _SRC[name] = SCENES[name][0]()
    return _SRC[name]


def packed(name):
    if name not in _PS:
        _PS[name] = V.oracle_scene(source(name))
    return _PS[name]


def tracer(name):
    if name not in _TRACER:
        _TRACER[name] = P.Tracer(packed(name))
    return _TRACER[name]


def cap_of(name):
    return SCENES[name][1]


def scene_camera(name, aspect=None):
    s = source(name)
    return {"c2w": np.asarray(s.camera_c2w, F).reshape(16).copy(), "vfov": float(s.vfov),
            "aspect": float(s.aspect if aspect is None else aspect)}


def moved(cam, shift):
    """The camera dict with its origin shifted in world space, in float32 (Camera.moved)."""
    c2w = np.array(cam["c2w"], F).copy()
    c2w[12:15] = c2w[12:15] + np.asarray(shift, F)
    return dict(cam, c2w=c2w)


def walk(name, w, h, cap, cam):
    """oracle_aov_path_points, remembered per (scene, size, cap, camera)."""
    key = (name, w, h, cap, cam["c2w"].tobytes(), cam["vfov"], cam["aspect"])
    if key not in _WALK:
        _WALK[key] = TP.oracle_aov_path_points(packed(name), w, h, cap, cam=cam, tracer=tracer(name))
    return _WALK[key]


def median_depth(name):
    """The median first-hit depth from the scene's camera at 96 x 54."""
    first = walk(name, 96, 54, 0, scene_camera(name))
    return float(np.median(first["depth"][first["material"] >= 0]))


def translation(name):
    return MOVE * median_depth(name)


def mirror_first_hit(name, ref):
    tab = P.material_table(packed(name))
    return (ref["first_material"] >= 0) & P.is_mirror(tab)[np.maximum(ref["first_material"], 0)]


def radiance(seed, aov):
    """Seeded random colours, as tests/test_gpu_temporal.py's frames."""
    h, w = aov["depth"].shape
    return np.random.default_rng(seed).uniform(0.0, 2.0, (h, w, 3)).astype(F)


# The device cases of tests/test_gpu_temporal_path.py: name -> (scene, W, H, cap, the fractions
# of the translation at which its frames stand).  The CPU suite asserts that the reference
# leaves at most 1 % of each case's pixels undecidable at POINT_TOL.
GPU_CASES = {
    "hall_two": ("hall", 80, 45, 3, (0.0, 1.0)),
    "hall_chain": ("hall", 80, 45, 3, (0.0, 1 / 3, 2 / 3)),
    "box2_two": ("box2", 80, 45, 8, (0.0, 1.0)),
    "box2_chain": ("box2", 80, 45, 8, (0.0, 1 / 3, 2 / 3)),
    "tilted_two": ("tilted", 80, 45, 3, (0.0, 1.0)),      # shading normals off the mirrors' planes
    "box_two": ("box", 80, 45, 8, (0.0, 1.0)),            # a curved mirror, and sky reflected in it
    "tir_chain": ("tir", 80, 45, 8, (0.0, 1 / 3, 2 / 3)),  # no mirror: glass is terminal
    "hall_131x9": ("hall", 131, 9, 3, (0.0, 1.0)),
    "hall_16x16": ("hall", 16, 16, 3, (0.0, 1.0)),
    "hall_3x2": ("hall", 3, 2, 3, (0.0, 1.0)),
    "hall_1x1": ("hall", 1, 1, 3, (0.0, 1.0)),
    "hall_257x241_static": ("hall", 257, 241, 3, (0.0, 0.0)),
}


def case_cameras(case):
    name, w, h, _, fractions = GPU_CASES[case]
    cam = scene_camera(name, aspect=w / h)
    t = translation(name)
    return [moved(cam, f * t) if f else cam for f in fractions]


def run_reference(frames, cams, demodulate, point_tol=POINT_TOL, params=PARAMS, without=None):
    """A chain through temporal_path_ref.  frames: (radiance, path buffers) per camera."""
    state, out = None, []
    for cam, (rad, aov) in zip(cams, frames):
        r = TP.temporal_path_ref(state, cam, rad, aov, demodulate=demodulate, point_tol=point_tol, _without=without,
                                 **params)
        state = r["state"]
        out.append(r)
    return out
