"""The cases of the deforming-mesh tests, shared by tests/test_deform_cpu.py,
test_deform_ref_teeth.py (feature buffers computed in numpy, deform_scenes.numpy_guides) and
tests/test_gpu_deform.py (the GPU's own feature and world buffers): which deformation the sheet
of tests/deform_scenes.py is under in which frame, from which camera, with which parameters, and
which rule of the definition the case is there to decide."""
import numpy as np

from tests import deform_ref as DR
from tests import deform_scenes as DS
from tests import temporal_ref as TR

F = np.float32
W, H = 37, 29                       # odd, no multiple of a tile or of a 64-pixel row segment
ASPECT = W / H
PARAMS = dict(alpha=0.1, depth_tol=0.1, normal_min=0.9, max_history=32)
STATIC = TR.camera(aspect=ASPECT)
MOVED = TR.camera(2.0, (0.13, 0.05, 0.02), aspect=ASPECT)
THIRD = TR.camera(3.0, (0.26, 0.10, 0.04), aspect=ASPECT)
PITCH_ROLL = dict(yaw_deg=1.0, pitch_deg=-2.0, roll_deg=3.0, translate=(0.1, -0.07, 0.05))
REST = (None, {})

# The normal rule of case "bend" sets normal_min = 0.999, and the right answer is n' . ne = 1 less the
# float32 rounding of the two normals (1e-7): 1e-3 from the threshold, which motion_ref's margin of 1e-3
# calls undecidable.  What the margin guards against is a float32 evaluation on the other side of the
# threshold; a float32 dot product of unit vectors errs by 4 * 2^-24 = 2.4e-7 and ne's normalisation
# by three ulps more, so 1e-4 is four hundred times what can happen.
BEND_MARGIN = 1e-4

# name -> (frames: (camera, (deformation, its arguments), seed), parameters that differ, the rules the case decides)
CASES = {
    # (a) up to a quarter of the sheet's depth towards the camera; depth_tol 0.02: only the distance of X' passes
    "bulge": ([(STATIC, REST, 101), (STATIC, (DS.bulge, {}), 202)], {"depth_tol": 0.02}, ("X", "current")),
    # (b) in the plane, up to 1.5 px: the static assumption reprojects onto where the point is now
    "swirl": ([(STATIC, REST, 101), (STATIC, (DS.swirl, {}), 202)], {}, ("X", "current")),
    # (c) up to 6 degrees of normal change, normal_min 0.999 > cos 6 deg = 0.9945: only ne passes
    "bend": ([(STATIC, REST, 101), (STATIC, (DS.bend, {}), 202)], {"normal_min": 0.999, "normal_margin": BEND_MARGIN},
             ("ne", "current")),
    # (d) the camera and the sheet both
    "camera_bulge": ([(STATIC, REST, 101), (MOVED, (DS.bulge, {}), 202)], {"depth_tol": 0.02}, ("X",)),
    # (e) static, stretched and translated triangles side by side
    "half": ([(STATIC, REST, 101), (STATIC, (DS.half, {}), 202)], {}, ("X",)),
}
CHAIN = [(STATIC, REST, 101), (MOVED, (DS.swirl, {}), 202), (THIRD, (DS.bulge, {"amp": 0.3}), 303)]
# a tpt_temporal call between two deform calls: (camera, deformation, seed, deform)
ALTERNATION = [(STATIC, REST, 101, True), (STATIC, REST, 202, False), (STATIC, (DS.swirl, {}), 303, True)]
SIZES = ((131, 9), (70, 70))
TINY = ((1, 1), (3, 2), (16, 16))


def colours(aov, seed):
    """Seeded random radiance and albedo for a frame with these guides (albedo 1 on a miss, as
    tpt_render_aov writes it; the middle hit pixel black: demodulation divides by the floor)."""
    h, w = aov["depth"].shape
    rng = np.random.default_rng(seed)
    rad = rng.uniform(0.0, 2.0, (h, w, 3)).astype(F)
    alb = rng.uniform(0.2, 1.0, (h, w, 3)).astype(F)
    alb[aov["material"] < 0] = 1.0
    hits = np.argwhere(aov["material"] >= 0)
    if len(hits):
        black = tuple(hits[len(hits) // 2])
        alb[black] = 0.0
        rad[black] = 0.0
    return rad, alb


def sequence(spec, w=W, h=H):
    """[(camera, world vertices, world normals, radiance, guides, deform)] of a list of (camera,
    deformation, seed[, deform]), the guides computed in numpy (deform_scenes.numpy_guides)."""
    seq = []
    for cam, (fn, kw), seed, *rest in spec:
        wv, wn = DS.deformed(fn, **kw)
        aov = DS.numpy_guides(cam, w, h, wv, wn)
        rad, aov["albedo"] = colours(aov, seed)
        seq.append((cam, wv, wn, rad, aov, rest[0] if rest else True))
    return seq


def reference(seq, params, **kw):
    """One result per frame.  A frame with deform False is a tpt_temporal call (the face guide is not
    read, and kw, the deform reference's knock-out, does not apply); it reports no motion: zero."""
    idx = DS.rest()[0]
    plain = {k: v for k, v in params.items() if k != "normal_margin"}
    refs, state = [], None
    for cam, wv, wn, rad, aov, deform in seq:
        if deform:
            refs.append(DR.temporal_deform_ref(state, cam, rad, aov, idx, wv, wn, **params, **kw))
        else:
            refs.append(dict(TR.temporal_ref(state, cam, rad, aov, **plain), motion=np.zeros(rad.shape[:2] + (2,))))
        state = refs[-1]["state"]
    return refs


def case(name, demodulate=True):
    spec, extra, _ = CASES[name]
    seq = sequence(spec)
    params = dict(PARAMS, **extra, demodulate=demodulate)
    return seq, params, reference(seq, params)


def sized_spec(w, h):
    """Two frames at w x h: the identity camera at rest, then PITCH_ROLL with the sheet swirled."""
    return [(TR.camera(aspect=w / h), REST, 101), (TR.camera(aspect=w / h, **PITCH_ROLL), (DS.swirl, {}), 202)]


def sized(w, h):
    seq = sequence(sized_spec(w, h), w, h)
    params = dict(PARAMS, demodulate=True)
    return seq, params, reference(seq, params)
