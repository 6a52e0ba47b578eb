"""tpt_temporal_motion and tpt_scene_set_transforms: the motion-aware temporal pass against
a float64 numpy restatement of its definition (tests/motion_ref.py; DESIGN.md section 5
"Moving objects") on temporal_ref's three patches, each bound to an object of box2 and
moved with it; the rebuilt scene against a fresh one, bit for bit; real geometry; an
end-to-end run.  tests/test_motion_ref_teeth.py shows on the CPU that the cases' inputs
can see the rules they are named for."""
import ctypes as C

import numpy as np
import pytest

import tinypathtracer_amd as T
from tinypathtracer_amd import _lib

from tests.conftest import scene_path
from tests import motion_ref as MR
from tests import temporal_ref as TR
from tests import test_gpu_temporal as G

pytestmark = pytest.mark.gpu

W, H = G.W, G.H                     # 37 x 29
ASPECT = G.ASPECT
PARAMS = G.PARAMS
ONE = G.ONE
CARRIER = MR.Carrier(T.Scene(scene_path("box2")))          # the lut and the objects; loaded on the host
BACK, CUBE, CUBE1 = MR.PATCH_OBJECTS                        # far wall, near strip, tilted wall
# the reference speaks of the library's flags
assert (_lib.MOTION_TRACKED, _lib.MOTION_IDENTITY, _lib.MOTION_UNTRACKED) == (MR.TRACKED, MR.IDENTITY, MR.UNTRACKED)

# The near strip lies at z = -2.5, where the 37 x 29 frame has 13.7 pixels per world unit
# both ways: (0.08, 0.075) is 1.1 pixels to the right and 1.0 up, 1.5 pixels in all.  The strip
# reaches below the frame, so its bottom row comes from outside the previous frame: disoccluded.
STRIP_STEP = MR.translation((0.08, 0.075, 0.0))
STRIP_BACK = MR.translation((-0.08, 0.15, 0.0))             # against the moving camera: 1.35 pixels up in its frame
STRIP_TURN = MR.rotation_y(4.0, centre=(0.05, 0.0, -2.5))
WALL_IN = MR.translation((0.0, 0.0, 1.0))                  # the tilted wall is 4 to 5 deep: a quarter of it
STATIC = G.CAMERAS["static"]

# name -> (frames: (camera, poses, seed), materials, parameters that differ, the rules the case decides).
# Poses are world motions from the rest pose, per object; an object without one stands still.
MOTION_CASES = {
    # the static assumption reprojects the strip onto where it is now, 1.5 pixels off its history
    "strip_translate": ([(STATIC, {}, 101), (STATIC, {CUBE: STRIP_STEP}, 202)], (0, 1, 2), {}, ("D",)),
    # one material and normal_min 0.999 > cos 4 deg = 0.9976: only the turned normal passes
    "strip_rotate": ([(STATIC, {}, 101), (STATIC, {CUBE: STRIP_TURN}, 202)], ONE, {"normal_min": 0.999}, ("G",)),
    # towards the camera by a quarter of its depth: the distance of X' is the history's, that of X is not
    "wall_approach": ([(STATIC, {}, 101), (STATIC, {CUBE1: WALL_IN}, 202)], ONE, {"depth_tol": 0.02}, ("dist",)),
    "both_move": ([(STATIC, {}, 101), (G.CAMERAS["yaw_translate"], {CUBE: STRIP_BACK}, 202)], (0, 1, 2), {}, ("D",)),
}
MOVED_PATCH = {"strip_translate": MR.STRIP, "strip_rotate": MR.STRIP, "wall_approach": MR.TILTED, "both_move": MR.STRIP}
# A rigid patch that is wholly in view in both frames finds history for every one of its pixels;
# what its motion disoccludes lies on the surface behind it.  In these cases the strip also
# moves up by more than a pixel, so its bottom row comes from below the previous frame.
EDGE_CASES = ("strip_translate", "both_move")
# A turn of 4 degrees about the strip's own centre moves its edges by 0.015 pixels: it uncovers
# no pixel centre, and every pixel of that case finds history -- if the G rule is applied.
NOTHING_UNCOVERED = ("strip_rotate",)
CHAIN = [(STATIC, {}, 101), (G.CAMERAS["yaw_translate"], {CUBE: STRIP_STEP}, 202),
         (G.THIRD, {CUBE: STRIP_TURN @ STRIP_STEP, CUBE1: MR.rotation_y(2.0, centre=(-2.0, 0.0, -3.4))}, 303)]


def frame(cam, seed, poses=None, w=W, h=H, materials=(0, 1, 2)):
    """test_gpu_temporal.frame with the moved patches' guides (black = None)."""
    rng = np.random.default_rng(seed)
    aov = MR.synthetic_guides(cam, w, h, CARRIER, poses, materials)
    rad = rng.uniform(0.0, 2.0, (h, w, 3)).astype(np.float32)
    alb = rng.uniform(0.2, 1.0, (h, w, 3)).astype(np.float32)
    alb[aov["material"] < 0] = 1.0
    hits = np.argwhere(aov["material"] >= 0)
    if len(hits):
        black = tuple(hits[len(hits) // 2])
        alb[black] = 0.0
        rad[black] = 0.0
    aov["albedo"] = alb
    return rad, aov


def sequence(spec, materials=(0, 1, 2), w=W, h=H):
    """[(camera, the scene's matrices, (radiance, guides))] of a list of (camera, poses, seed)."""
    return [(cam, CARRIER.vert_trans(poses), frame(cam, seed, poses, w, h, materials)) for cam, poses, seed in spec]


def reference(seq, params, **kw):
    refs, state = [], None
    for cam, vt, (rad, aov) in seq:
        refs.append(MR.temporal_motion_ref(state, cam, rad, aov, CARRIER, vt, **params, **kw))
        state = refs[-1]["state"]
    return refs


def case(name, demodulate=True):
    spec, materials, extra, _ = MOTION_CASES[name]
    seq = sequence(spec, materials)
    params = dict(PARAMS, **extra, demodulate=demodulate)
    return seq, params, reference(seq, params)


def sized(w, h, materials=(0, 1, 2)):
    """Two frames at w x h: the identity camera, then test_gpu_temporal's PITCH_ROLL with the
    strip moved one step."""
    cams = (TR.camera(aspect=w / h), TR.camera(aspect=w / h, **G.PITCH_ROLL))
    seq = sequence([(cams[0], {}, 101), (cams[1], {CUBE: STRIP_STEP}, 202)], materials, w, h)
    params = dict(PARAMS, demodulate=True)
    return seq, params, reference(seq, params)


# The bound.  tpt_temporal's a-priori ceiling (test_gpu_temporal.py) allows the float32
# reprojected coordinate 2^-14 px of error, which moves each of the four bilinear weights by
# that much, renormalised by wsum >= 1/16: 4 * 16 * 2^-14 = 4e-3 of the value range.  Here the
# coordinate also carries the error of the float32 X' = D X: three products and three sums of
# terms below 8, half an ulp (2^-21) each, and four entries of D a float32 rounding (2^-24,
# relative) away from the reference's, times |X| <= 5: 3 * 2^-21 + 4 * 5 * 2^-24 = 2.6e-6 world
# units, taken as DX = 6 * 2^-21.  A world unit is max(W / sensor_w, H / sensor_h) / z pixels, the
# nearest surface of these frames being Z_MIN = 2 away (the strip at 2.5, the cameras' 0.13
# steps): 17 px at 37 x 29, 41 px at 70 x 70.  So the ceiling is 4 * 16 * (2^-14 + DX * px per
# unit): 7.0e-3 at 37 x 29, 1.2e-2 at 70 x 70, 5.0e-3 at 131 x 9.  MEASURED_MAX is the largest
# max|gpu - ref| / max|ref| over colour, variance and history length of every case below on
# MI355X; the asserted bound is ten times that and must stay under the smallest ceiling.
DX = 6 * 2.0 ** -21
Z_MIN = 2.0


def ceiling(w, h):
    sw, sh, _, _ = (float(v) for v in TR.sensor(0.8, w / h))
    return 4 * 16 * (2.0 ** -14 + DX * max(w / sw, h / sh) / Z_MIN)


# Measured on MI355X, max|gpu - ref| / max|ref| over colour, variance and history length (undecidable
# pixels of the last frame in brackets; every first frame has none and differs by rounding, 1e-16):
#   two-frame cases at 37 x 29, both demodulate settings   6.7e-7 .. 2.72e-6 (both_move, variance) [0]
#   three-frame chains                                     2.79e-6, blended history lengths 3.6e-7 [0]
#   131 x 9, either block shape                            8.54e-6 colour, 6.91e-6 variance [1 of 1,179]
#   70 x 70, either block shape                            4.41e-6 colour, 4.84e-6 variance [8 of 4,900]
#   1 x 1, 3 x 2, 16 x 16                                  0 .. 7.4e-7 [0]
#   untracked strip, faces -1 and 36 (the other pixels)    4.0e-7 [0]
#   box2 80 x 45, Cube moved, the GPU's feature buffers    2.22e-6 colour [0]
#   motion_out, both_move                                  4.3e-6 px of MOTION_PX = 1.2e-4
# These are tpt_temporal's own figures on the same frames (test_gpu_temporal.py: 8.61e-6 at 131 x 9,
# 4.80e-6 at 70 x 70): D X adds nothing that shows, and the largest is a 470th of the smallest ceiling.
MEASURED_MAX = 8.541e-6             # colour, 131 x 9 frame 2
BOUND = 10 * MEASURED_MAX
assert BOUND <= min(ceiling(w, h) for w, h in ((W, H), (131, 9), (70, 70), (1, 1), (3, 2), (16, 16), (80, 45)))
MOTION_PX = 2.0 ** -14 + DX * 41.4 / Z_MIN                  # motion_out against the reference, in pixels


@pytest.fixture(scope="module")
def ctx(gpu_available):
    s = T.Scene(scene_path("box2"))
    d = s.copySceneToDevice(0)                             # tpt_temporal_motion reads its matrices; it need not be built
    yield d
    d.close()


def play(d, seq, params, flags=0, motion=True, with_motion_out=False):
    """A new history through the sequence, the scene's matrices set before every frame.
    Returns per frame (out, variance, history length, stats[, motion_out])."""
    h, w = seq[0][2][0].shape[:2]
    pt = T.PathTracer("", w, h, 0)
    hist = T.History(d, w, h)
    got = []
    for cam, vt, (rad, aov) in seq:
        d.set_transforms(0, vt)
        kw = dict(params, flags=flags)
        mv = None
        if motion:
            kw["motion"] = True
            if with_motion_out:
                mv = kw["motion_out"] = np.full((h, w, 2), -3.0, np.float32)
        r = G.run(pt, hist, cam, rad, aov, **kw)
        got.append(r + (mv,) if with_motion_out else r)
    hist.close()
    return got


@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("name", list(MOTION_CASES))
def test_two_frame_cases_match_numpy_reference(ctx, name, demodulate):
    seq, params, refs = case(name, demodulate)
    got = play(ctx, seq, params)
    for k in range(2):
        G.compare(f"{name} demodulate {demodulate} frame {k + 1}", got[k], refs[k], bound=BOUND)
    on = seq[1][2][1]["face"] == MR.patch_faces(CARRIER)[MOVED_PATCH[name]]
    n = got[1][2]
    assert (n[on] == 2.0).any()                            # the moved patch finds its history
    assert (n == 1.0).any() == (name not in NOTHING_UNCOVERED)         # and its motion uncovers something
    if name in EDGE_CASES:
        assert (n[on] == 1.0).any()                        # and part of the patch itself is new


@pytest.mark.parametrize("materials", [(0, 1, 2), ONE], ids=["three_materials", "one_material"])
def test_three_frame_chain(ctx, materials):
    """A different motion in every step: the camera and the strip, then the camera, the strip
    (turned as well) and the tilted wall."""
    seq = sequence(CHAIN, materials)
    params = dict(PARAMS, demodulate=True)
    refs = reference(seq, params)
    got = play(ctx, seq, params)
    for k in range(3):
        G.compare(f"chain {materials} frame {k + 1}", got[k], refs[k], exact_n=k < 2, bound=BOUND)
    n = got[2][2]
    assert (n == 3.0).any() and (n == 1.0).any()


@pytest.mark.parametrize("w,h", [(131, 9), (70, 70)])
def test_multi_block_frames(ctx, w, h):
    """Several blocks under both block shapes, against the reference and each other."""
    seq, params, refs = sized(w, h)
    rows = play(ctx, seq, params, flags=0, with_motion_out=True)
    tiles = play(ctx, seq, params, flags=_lib.TEMPORAL_TILES, with_motion_out=True)
    for name, got in (("row segments", rows), ("tiles", tiles)):
        for k in range(2):
            G.compare(f"{w} x {h} {name} frame {k + 1}", got[k][:4], refs[k], bound=BOUND)
    for a, b in zip(rows[1][:3] + (rows[1][4],), tiles[1][:3] + (tiles[1][4],)):
        assert np.array_equal(G._bits(a), G._bits(b))
    assert rows[1][3]["reprojected"] == tiles[1][3]["reprojected"]
    n = rows[1][2]
    assert (n == 1.0).any() and (n == 2.0).any()


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (16, 16)])
@pytest.mark.parametrize("flags", [0, _lib.TEMPORAL_TILES], ids=["rows", "tiles"])
def test_tiny_frames(ctx, w, h, flags):
    """Less than a wave, less than a tile, exactly one tile."""
    seq, params, refs = sized(w, h)
    got = play(ctx, seq, params, flags=flags)
    for k in range(2):
        G.compare(f"{w} x {h} flags {flags} frame {k + 1}", got[k], refs[k], bound=BOUND)


def test_motion_out(ctx):
    """(fx - x, fy - y) after the snap wherever the reprojection is in front of the previous
    camera, accepted or not; (0, 0) on the first frame and behind the previous camera."""
    seq, params, refs = case("both_move")
    got = play(ctx, seq, params, with_motion_out=True)
    assert (got[0][4] == 0.0).all()
    mv, ref = got[1][4], refs[1]
    dec = ref["decidable"]
    err = np.abs(mv.astype(np.float64) - ref["motion"])[dec].max()
    print(f"motion_out: max|gpu - ref| = {err:.3e} px (allowed {MOTION_PX:.3e}); largest motion "
          f"{np.abs(ref['motion']).max():.2f} px")
    assert err <= MOTION_PX
    strip = seq[1][2][1]["face"] == MR.patch_faces(CARRIER)[MR.STRIP]
    rejected = strip & ~ref["reprojected"] & dec
    assert rejected.any() and (np.abs(mv[rejected]).sum(-1) > 0).all()    # written whether or not the taps were accepted
    # everything the second camera sees lies behind the first (test_gpu_temporal's turn_180)
    spec = [(STATIC, {}, 101), (TR.camera(180.0, aspect=ASPECT), {CUBE: STRIP_STEP}, 202)]
    seq = sequence(spec, ONE)
    got = play(ctx, seq, params, with_motion_out=True)
    assert (got[1][4] == 0.0).all() and (got[1][2] == 1.0).all()


def test_all_static_is_tpt_temporal(ctx):
    """Nothing moved: the same bits as tpt_temporal, and after a third frame too, which shows
    that the two leave the same state."""
    cams = [STATIC, G.CAMERAS["yaw_translate"], G.THIRD]
    seq = sequence([(c, {}, seed) for c, seed in zip(cams, (101, 202, 303))])
    pt = T.PathTracer("", W, H, 0)
    ctx.set_transforms(0, CARRIER.rest)
    results = {}
    for motion in (False, True):
        hist = T.History(ctx, W, H)
        per_frame = []
        for cam, _, (rad, aov) in seq:
            fb = np.full((H, W, 4), 0x5A, np.uint8)
            kw = dict(PARAMS, demodulate=True, framebuffer=fb)
            if motion:
                kw["motion"] = True
            per_frame.append(G.run(pt, hist, cam, rad, aov, **kw) + (fb,))
        hist.close()
        results[motion] = per_frame
    for a, b in zip(results[False], results[True]):
        for x, y in zip(a[:3], b[:3]):
            assert np.array_equal(G._bits(x), G._bits(y))
        assert np.array_equal(a[4], b[4]) and a[3]["reprojected"] == b[3]["reprojected"]
    assert (results[True][2][2] == 3.0).any()
    # and either entry point records the transforms: a tpt_temporal frame, then a motion frame
    seq = sequence(MOTION_CASES["strip_translate"][0])
    refs = reference(seq, dict(PARAMS, demodulate=True))
    hist = T.History(ctx, W, H)
    ctx.set_transforms(0, seq[0][1])
    G.run(pt, hist, seq[0][0], *seq[0][2], demodulate=True, **PARAMS)
    ctx.set_transforms(0, seq[1][1])
    got = G.run(pt, hist, seq[1][0], *seq[1][2], demodulate=True, motion=True, **PARAMS)
    hist.close()
    G.compare("tpt_temporal, then tpt_temporal_motion", got, refs[1], bound=BOUND)


def test_untracked_object_and_bad_faces(ctx):
    """A singular matrix for the strip's object: its pixels are disoccluded (N = 1, the output
    the input bit for bit), the others match the reference.  The same for hit pixels whose
    face id is -1 or n_faces."""
    seq = sequence(MOTION_CASES["strip_translate"][0])
    flat = MR.mat(CARRIER.rest[CUBE]).copy()
    flat[:3, 1] = 0.0                                      # the y axis scaled to nothing
    seq[1] = (seq[1][0], seq[1][1].copy(), seq[1][2])
    seq[1][1][CUBE] = MR.col_major(flat)
    params = dict(PARAMS, demodulate=True)
    assert MR.motion_matrices_ref(seq[0][1], seq[1][1])[2][CUBE] == MR.UNTRACKED
    refs = reference(seq, params)
    got = play(ctx, seq, params, with_motion_out=True)
    strip = seq[1][2][1]["face"] == MR.patch_faces(CARRIER)[MR.STRIP]
    out, var, n, st, mv = got[1]
    assert strip.sum() > 50 and (n[strip] == 1.0).all() and (mv[strip] == 0.0).all()
    assert np.array_equal(G._bits(out[strip]), G._bits(seq[1][2][0][strip]))
    assert (n[~strip] == 2.0).any()
    G.compare("untracked strip frame 2", got[1][:4], refs[1], bound=BOUND)
    for bad in (-1, CARRIER.n_faces):
        seq = sequence(MOTION_CASES["strip_translate"][0])
        aov = dict(seq[1][2][1])
        strip = aov["face"] == MR.patch_faces(CARRIER)[MR.STRIP]
        aov["face"] = np.where(strip, bad, aov["face"]).astype(np.int32)
        seq[1] = (seq[1][0], seq[1][1], (seq[1][2][0], aov))
        refs = reference(seq, params)
        got = play(ctx, seq, params)
        assert (got[1][2][strip] == 1.0).all()
        assert np.array_equal(G._bits(got[1][0][strip]), G._bits(seq[1][2][0][strip]))
        G.compare(f"face {bad} frame 2", got[1], refs[1], bound=BOUND)


def moved_box2():
    """(scene, the rest matrices, the moved ones): box2's object "Cube" (the scene's object 6)
    turned by 5 degrees about y through its own world position, then translated."""
    s = T.Scene(scene_path("box2"))
    rest = np.asarray(s.vert_trans, np.float32).copy()
    centre = MR.mat(rest[CUBE])[:3, 3]
    move = MR.translation((0.25, 0.0, 0.15)) @ MR.rotation_y(5.0, centre=centre)
    moved = rest.copy()
    moved[CUBE] = MR.col_major(move @ MR.mat(rest[CUBE]))
    return s, rest, moved


def test_real_geometry_box2_moved(gpu_available):
    """box2 at 80 x 45: frame 1 as loaded, frame 2 with Cube moved through set_transforms +
    build, the guides from tpt_render_aov of the rebuilt scene, against the reference fed the
    GPU's own feature buffers."""
    w, h = 80, 45
    s, rest, moved = moved_box2()
    d = s.copySceneToDevice(0).build()
    pt = T.PathTracer("", w, h, 0)
    cam = s.m_camera
    camd = {"c2w": np.asarray(cam.c2w, np.float32), "vfov": cam.vfov, "aspect": cam.aspect}
    carrier = MR.Carrier(s)
    rng = np.random.default_rng(77)
    hist = T.History(d, w, h)
    state = None
    for k, vt in enumerate((rest, moved)):
        if k:
            d.set_transforms(CUBE, vt[CUBE:CUBE + 1]).build()
        aov = pt.renderAOV(d, cam)
        rad = rng.uniform(0.0, 2.0, (h, w, 3)).astype(np.float32)
        var = np.zeros((h, w), np.float32)
        n = np.zeros((h, w), np.float32)
        st = {}
        out = pt.temporal(hist, cam, rad, aov, variance=var, history_len=n, stats=st, demodulate=True, motion=True,
                          **PARAMS)
        ref = MR.temporal_motion_ref(state, camd, rad, aov, carrier, vt, demodulate=True, **PARAMS)
        state = ref["state"]
        G.compare(f"box2 moved {w} x {h} frame {k + 1}", (out, var, n, st), ref, bound=BOUND)
    hist.close()
    d.close()
    lo, hi = carrier.faces_of(CUBE)
    cube = (aov["face"] >= lo) & (aov["face"] < hi)
    # every visible point of the cube was visible before its 5 degrees; what it uncovers is wall and floor
    assert cube.sum() > 100 and (n[cube] == 2.0).mean() > 0.9 and (n[~cube] == 1.0).any()


@pytest.mark.parametrize("asynchronous", [False, True], ids=["build", "build_async"])
def test_rebuild_is_a_fresh_scene(gpu_available, asynchronous):
    """set_transforms + build against a fresh DeviceScene created with the same matrices: the
    world vertices and normals, the BVH and a 64 x 36, 4-spp, seed-7 frame, bit for bit."""
    from oracle import scene as S
    s, rest, moved = moved_box2()
    cols = [[moved[CUBE][4 * c + r] for r in range(4)] for c in range(4)]
    normal = S.flat(S.normal_to_world(cols))               # the loader's operations (tests/test_loader_abi.py)
    pt = T.PathTracer("", 64, 36, 0)

    def snapshot(d):
        rad = np.zeros((36, 64, 3), np.float32)
        pt.doTrace(d, s.m_camera, None, 4, seed=7, radiance=rad)
        return d.read_world() + d.read_bvh() + (rad,)

    d = s.copySceneToDevice(0).build()
    before = snapshot(d)
    d.set_transforms(CUBE, moved[CUBE:CUBE + 1])           # normal_trans computed by the library
    assert not d.built
    d.build(asynchronous=asynchronous)
    rebuilt = snapshot(d)
    d.set_transforms(CUBE, moved[CUBE:CUBE + 1], normal[None]).build(asynchronous=asynchronous)
    explicit = snapshot(d)
    d.close()
    fresh_scene = T.Scene(scene_path("box2"))
    fresh_scene.vert_trans[CUBE] = moved[CUBE]
    fresh_scene.normal_trans[CUBE] = normal
    f = fresh_scene.copySceneToDevice(0).build()
    fresh = snapshot(f)
    f.close()
    for got in (rebuilt, explicit):
        for a, b in zip(got, fresh):
            assert a.tobytes() == b.tobytes()
    assert before[0].tobytes() != fresh[0].tobytes() and before[4].tobytes() != fresh[4].tobytes()


def test_refusals(ctx):
    """A missing face guide and set_transforms' range errors: TPT_ERR_INVALID_ARG, nothing
    written, the history, its snapshot and the scene as they were -- the next valid call gives
    what an undisturbed history gives."""
    L = T.lib()
    seq, params, refs = case("strip_translate")
    pt = T.PathTracer("", W, H, 0)
    hist = T.History(ctx, W, H)
    ctx.set_transforms(0, seq[0][1])
    G.run(pt, hist, seq[0][0], *seq[0][2], motion=True, **params)
    ctx.set_transforms(0, seq[1][1])
    cam2, _, (rad2, aov2) = seq[1]
    out = np.full((H, W, 3), -7.0, np.float32)
    mv = np.full((H, W, 2), -7.0, np.float32)
    cam = G._cam(cam2).to_c()
    p = _lib.TemporalParams(0.1, 0.1, 0.9, 32, 1)

    def call(face, handle=hist.handle):
        g = _lib.Aov(aov2["albedo"].ctypes.data, aov2["normal"].ctypes.data, aov2["depth"].ctypes.data, face,
                     aov2["material"].ctypes.data)
        return L.tpt_temporal_motion(handle, C.byref(cam), rad2.ctypes.data, C.byref(g), C.byref(p), out.ctypes.data,
                                     None, None, mv.ctypes.data, None, None)

    assert call(None) == 1 and b"face" in L.tpt_last_error()
    assert call(aov2["face"].ctypes.data, handle=None) == 1 and b"history" in L.tpt_last_error()
    assert (out == -7.0).all() and (mv == -7.0).all()
    with pytest.raises(ValueError):
        pt.temporal(hist, G._cam(cam2), rad2, aov2, motion_out=mv, **params)       # motion_out without motion
    one = np.ascontiguousarray(seq[1][1][:1])
    n = CARRIER.n_objects
    for first, count, vt in ((0, 0, one), (n, 1, one), (n - 1, 2, np.ascontiguousarray(seq[1][1][:2])),
                             (2 ** 32 - 1, 2, one), (0, 1, None)):
        ptr = None if vt is None else vt.ctypes.data
        assert L.tpt_scene_set_transforms(ctx.handle, first, count, ptr, None) == 1, (first, count)
    assert L.tpt_scene_set_transforms(None, 0, 1, one.ctypes.data, None) == 1
    got = G.run(pt, hist, cam2, rad2, aov2, motion=True, **params)
    hist.close()
    G.compare("after the refusals", got, refs[1], bound=BOUND)


def test_nothing_is_written_past_the_end_and_deterministic(ctx):
    """131 x 9, every output the first rows of a device tensor one row longer: the extra row
    keeps its sentinel.  Two runs and the two block shapes agree bit for bit."""
    import torch
    w, h = 131, 9
    seq, params, refs = sized(w, h)
    dev = torch.device("cuda", 0)
    up = lambda a: {k: torch.from_numpy(v).to(dev) for k, v in a.items()}
    pt = T.PathTracer("", w, h, 0)
    want = play(ctx, seq, params, with_motion_out=True)[1]
    again = play(ctx, seq, params, with_motion_out=True)[1]
    for a, b in zip(want[:3] + (want[4],), again[:3] + (again[4],)):
        assert np.array_equal(G._bits(a), G._bits(b))
    for flags in (0, _lib.TEMPORAL_TILES):
        hist = T.History(ctx, w, h)
        for cam, vt, (rad, aov) in seq:
            ctx.set_transforms(0, vt)
            whole = [torch.full((h + 1, w, 3), -7.0, device=dev), torch.full((h + 1, w), -7.0, device=dev),
                     torch.full((h + 1, w), -7.0, device=dev), torch.full((h + 1, w, 2), -7.0, device=dev)]
            pt.temporal(hist, G._cam(cam), torch.from_numpy(rad).to(dev), up(aov), out=whole[0][:h],
                        variance=whole[1][:h], history_len=whole[2][:h], motion=True, motion_out=whole[3][:h],
                        flags=flags, **params)
        hist.close()
        for t, ref in zip(whole, want[:3] + (want[4],)):
            got = t.cpu().numpy()
            assert (got[h] == -7.0).all()
            assert not (got[:h] == -7.0).any()
            assert np.array_equal(G._bits(got[:h]), G._bits(ref))


# box's object "ball1" (the scene's object 5) sits 7 world units in front of the camera, where
# the 96 x 54 frame has 19 pixels per world unit (96 / (aspect * 2 tan(0.2)) / 7).  The step is
# chosen by two arguments.  Direction: along +x the ball runs behind ball2 and along -x into the
# left wall, so it rises, +y, off the floor it rests on, where nothing comes to hide it.  Size:
# ball1 is a mirror (metallic 1), whose shading -- the reflected light and walls -- slides over
# its surface as it moves; the pass reprojects surface points and does not track that
# (include/tpt.h), and the lag it leaves grows with the square of the step while the noise it
# removes does not, so the test takes the slow end of the 1 to 3 pixels per frame it is to cover:
# 0.055 world units, 1.05 pixels.
BALL1 = 5
BALL_STEP = (0.0, 0.055, 0.0)


def test_end_to_end_follows_the_ball(gpu_available):
    """box at 96 x 54, a static camera, eight frames of 8 spp (seeds 1..8), ball1 one BALL_STEP
    further in every frame.  Over the final pose's ball1 pixels the motion-aware accumulation
    is closer to a 2,048-spp render of that pose than the last 8-spp frame alone.  tpt_temporal
    on the same frames and both passes' mean history length there are printed, not asserted:
    the untextured ball may hide the static assumption's smear."""
    w, h = 96, 54
    s = T.Scene(scene_path("box"))
    rest = np.asarray(s.vert_trans, np.float32).copy()
    d = s.copySceneToDevice(0).build()
    pt = T.PathTracer("", w, h, 0)
    cam = s.m_camera
    hists = {True: T.History(d, w, h), False: T.History(d, w, h)}
    noisy = np.zeros((h, w, 3), np.float32)
    outs, lens, steps = {}, {True: np.zeros((h, w), np.float32), False: np.zeros((h, w), np.float32)}, []
    mv = np.zeros((h, w, 2), np.float32)
    for k in range(8):
        m = MR.col_major(MR.translation(np.multiply(BALL_STEP, k)) @ MR.mat(rest[BALL1]))
        if k:
            d.set_transforms(BALL1, m[None]).build()
        pt.doTrace(d, cam, None, 8, seed=k + 1, radiance=noisy)
        aov = pt.renderAOV(d, cam)
        for motion in (True, False):
            outs[motion] = pt.temporal(hists[motion], cam, noisy, aov, history_len=lens[motion], motion=motion,
                                       motion_out=mv if motion else None)
        lo, hi = MR.Carrier(s).faces_of(BALL1)
        ball = (aov["face"] >= lo) & (aov["face"] < hi)
        if k:
            steps.append(float(np.sqrt((mv[ball] ** 2).sum(-1)).mean()))
    truth = np.zeros((h, w, 3), np.float32)
    pt.doTrace(d, cam, None, 2048, seed=42, radiance=truth)
    for hist in hists.values():
        hist.close()
    d.close()
    mse = lambda a: float(((a.astype(np.float64) - truth)[ball] ** 2).mean())
    print(f"ball1: {int(ball.sum())} pixels, {min(steps):.2f} .. {max(steps):.2f} px per frame; MSE last 8-spp frame "
          f"{mse(noisy):.5f}, tpt_temporal_motion {mse(outs[True]):.5f}, tpt_temporal {mse(outs[False]):.5f}; "
          f"mean history length {lens[True][ball].mean():.2f} / {lens[False][ball].mean():.2f}")
    assert ball.sum() > 50
    assert 1.0 <= min(steps) and max(steps) <= 3.0
    assert mse(outs[True]) < mse(noisy)
    # measured on MI355X: 0.117 against 0.220 for the single frame and 0.758 for tpt_temporal, whose
    # static assumption smears the ball over its path (6.5 times the motion-aware error): a factor 2 is asserted
    assert mse(outs[False]) > 2.0 * mse(outs[True])
