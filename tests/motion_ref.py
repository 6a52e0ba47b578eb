"""CPU reference for the motion-aware temporal pass (tests/test_gpu_motion.py,
tests/test_motion_api.py, tests/test_motion_ref_teeth.py): a float64 numpy restatement of
tpt_temporal_motion as DESIGN.md section 5 "Moving objects" defines it, of
tpt_motion_matrices, and temporal_ref's three synthetic patches bound to objects of a
scene and moved with them.

The definition itself lives in temporal_ref.temporal_core.  temporal_motion_ref adds what
tpt_temporal_motion adds: where each lane's surface was in the previous frame (its object's
D and G applied to X and n, and whether the object is tracked), the reported motion, and
the matrices carried in the state.  Where every object stands still that is X and n
themselves, so it agrees with temporal_ref array for array (test_motion_api.py).  Its
`decidable` mask leaves out pixels within MARGIN of a threshold: 1e-3 less one part in 10^9: a turned normal against normal_min 0.999 gives
n' . n_e = 1 - 1e-16, which float64 places 1e-3 - 1e-16 from the threshold, and what the mask
guards against -- a float32 evaluation on the other side -- is six orders of magnitude wider."""
import numpy as np

from tests import post_ref as R
from tests import temporal_ref as TR

F = np.float32
TRACKED, IDENTITY, UNTRACKED = 0, 1, 2
MARGIN = 1e-3 * (1.0 - 1e-9)


def mat(m16):
    """16 float32 values, column-major -> a float64 4 x 4 matrix."""
    return np.asarray(m16, F).astype(np.float64).reshape(4, 4).T


def col_major(m):
    """A 4 x 4 matrix -> 16 float32 values, column-major (one rounding)."""
    return np.asarray(m, np.float64).T.reshape(16).astype(F)


def translation(t):
    m = np.eye(4)
    m[:3, 3] = t
    return m


def rotation_y(deg, centre=(0.0, 0.0, 0.0), scale=1.0):
    """A turn by `deg` about +y through `centre`, then a uniform scale about it."""
    a = np.deg2rad(deg)
    r = np.eye(4)
    r[0, 0], r[0, 2], r[2, 0], r[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    r[:3, :3] *= scale
    return translation(centre) @ r @ translation(-np.asarray(centre, np.float64))


def motion_matrices_ref(prev, cur):
    """tpt_motion_matrices in numpy float64, each entry rounded to float32 once.
    Returns D [n, 3, 4], G [n, 3, 3] (float32) and flags [n]."""
    prev = np.asarray(prev, F).reshape(-1, 16)
    cur = np.asarray(cur, F).reshape(-1, 16)
    n = len(cur)
    D = np.tile(np.eye(4, dtype=F)[:3], (n, 1, 1))
    G = np.tile(np.eye(3, dtype=F), (n, 1, 1))
    flags = np.zeros(n, np.int32)
    last = np.array([0.0, 0.0, 0.0, 1.0])
    for o in range(n):
        if np.array_equal(prev[o].view(np.uint32), cur[o].view(np.uint32)):
            flags[o] = IDENTITY
            continue
        mp, m = mat(prev[o]), mat(cur[o])
        ok = np.array_equal(mp[3], last) and np.array_equal(m[3], last) and np.linalg.det(m[:3, :3]) != 0.0
        if ok:
            with np.errstate(all="ignore"):
                try:
                    d = mp @ np.linalg.inv(m)
                    g = np.linalg.inv(d[:3, :3]).T
                    d32, g32 = d[:3].astype(F), g.astype(F)
                    ok = bool(np.isfinite(d32).all() and np.isfinite(g32).all())
                except np.linalg.LinAlgError:
                    ok = False
        if not ok:
            flags[o] = UNTRACKED
            continue
        D[o], G[o] = d32, g32
    return D, G, flags


def face_objects(lut, n_faces):
    """The object whose lut interval holds each face."""
    begin = np.asarray(lut, np.int64).reshape(-1, 2)[:, 0]
    return (np.searchsorted(begin, np.arange(n_faces), side="right") - 1).astype(np.int32)


class Carrier:
    """What the reference needs of a scene: its lut and its objects' matrices.  box2's scene
    serves the synthetic tests; it need not be built."""

    def __init__(self, scene):
        self.lut = np.asarray(scene.lut, np.int32).reshape(-1, 2)
        self.n_faces = int(scene.n_faces)
        self.n_objects = len(self.lut)
        self.face_object = face_objects(self.lut, self.n_faces)
        self.rest = np.asarray(scene.vert_trans, F).reshape(-1, 16).copy()

    def faces_of(self, o):
        end = self.lut[o + 1, 0] if o + 1 < self.n_objects else self.n_faces
        return int(self.lut[o, 0]), int(end)

    def vert_trans(self, poses):
        """The scene's matrices with object o's rest matrix moved by poses[o] (a 4 x 4 world
        motion); an object without a pose keeps its rest matrix bit for bit."""
        vt = self.rest.copy()
        for o, a in poses.items():
            if a is not None:
                vt[o] = col_major(np.asarray(a, np.float64) @ mat(self.rest[o]))
        return vt


# temporal_ref's three patches, each bound to an object of box2 (far wall -> back, near strip ->
# Cube, tilted wall -> Cube.001) and given one face of that object: the first, the last, the second
PATCH_OBJECTS = (4, 6, 7)
FAR, STRIP, TILTED = 0, 1, 2


def patch_faces(carrier):
    ends = [carrier.faces_of(o) for o in PATCH_OBJECTS]
    return ends[0][0], ends[1][1] - 1, ends[2][0] + 1


def synthetic_guides(cam, W, H, carrier, poses=None, materials=(0, 1, 2)):
    """temporal_ref.synthetic_guides with a face plane, each patch moved rigidly by the world
    motion poses[its object] (None / absent: where temporal_ref has it, computed with
    temporal_ref's operations, so the guides are then temporal_ref's bit for bit)."""
    poses = poses or {}
    o32, d32 = R.pixel_centre_rays(cam["c2w"], cam["vfov"], cam["aspect"], W, H)
    o, d = o32.astype(np.float64), d32.astype(np.float64)
    patches = [
        ((0.0, 0.0, -4.0), (0.0, 0.0, 1.0), lambda X: X[..., 1] < 1.0, materials[0]),
        ((0.0, 0.0, -2.5), (0.0, 0.0, 1.0), lambda X: (X[..., 0] > -0.4) & (X[..., 0] < 0.5) & (X[..., 1] < 0.6), materials[1]),
        ((-1.2, 0.0, -4.0), (0.6, 0.0, 0.8), lambda X: (X[..., 0] < -1.2) & (X[..., 1] < 1.0), materials[2]),
    ]
    faces = patch_faces(carrier)
    best = np.full((H, W), np.inf)
    normal = np.zeros((H, W, 3), F)
    material = np.full((H, W), -1, np.int32)
    face = np.full((H, W), -1, np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k, (point, nrm, inside, mtl) in enumerate(patches):
            nrm, point = np.asarray(nrm), np.asarray(point)
            a = poses.get(PATCH_OBJECTS[k])
            if a is not None:
                a = np.asarray(a, np.float64)
                lin = a[:3, :3]
                point = lin @ point + a[:3, 3]
                nrm = np.linalg.inv(lin).T @ nrm
                nrm = nrm / np.linalg.norm(nrm)
                back = np.linalg.inv(a)
            t = ((point - o) @ nrm) / (d @ nrm)
            X = o + t[..., None] * d
            rest = X if a is None else X @ back[:3, :3].T + back[:3, 3]
            ok = np.isfinite(t) & (t > 0) & inside(rest) & (t < best)
            best = np.where(ok, t, best)
            normal[ok] = nrm.astype(F)
            material[ok] = mtl
            face[ok] = faces[k]
    depth = np.where(material >= 0, best, 0.0).astype(F)
    return {"normal": normal, "depth": depth, "material": material, "face": face}


def temporal_motion_ref(state, cam, radiance, aov, carrier, vert_trans, alpha, depth_tol, normal_min, max_history,
                        demodulate, clip=None, _without=None):
    """One call of the definition.  carrier: the scene's lut (Carrier); vert_trans: its
    objects' matrices at this call ([n, 16] float32); state: None or what a previous call
    returned under `state` (it holds that call's matrices).  Returns temporal_core's dict with
    `motion` [H, W, 2].

    _without (tests/test_motion_ref_teeth.py only) evaluates a wrong definition, one rule
    knocked out: "D" reprojects X instead of X' (the static assumption), "G" compares the
    unrotated normal, "dist" (temporal_core's) measures the expected depth from X instead of X'."""
    f = np.asarray(aov["face"], np.int64)
    vert_trans = np.asarray(vert_trans, F).reshape(-1, 16).copy()

    def source(state, X, n, hit, o, d32):
        # changes 1 - 3 and 5: the object, its D and G, X' and the previous frame's normal
        D, G, flags = motion_matrices_ref(state["vert_trans"], vert_trans)
        in_range = (f >= 0) & (f < carrier.n_faces)
        obj = carrier.face_object[np.clip(f, 0, carrier.n_faces - 1)]
        tracked = ~hit | (in_range & (flags[obj] != UNTRACKED))
        moved = hit & in_range & (flags[obj] == TRACKED)
        Dp, Gp = D.astype(np.float64)[obj], G.astype(np.float64)[obj]
        Xm, ne = X, n
        if moved.any():
            Xd = np.einsum("hwij,hwj->hwi", Dp[..., :3], X) + Dp[..., 3]
            gn = np.einsum("hwij,hwj->hwi", Gp, n)
            with np.errstate(divide="ignore", invalid="ignore"):
                gn = gn / np.linalg.norm(gn, axis=-1, keepdims=True)
            Xm = np.where(moved[..., None], Xd, X)
            ne = np.where(moved[..., None], gn, n)
        return X if _without == "D" else Xm, n if _without == "G" else ne, tracked

    return TR.temporal_core(state, cam, radiance, aov, alpha, depth_tol, normal_min, max_history, demodulate, clip=clip,
                            source=source, motion=True, extra_state={"vert_trans": vert_trans}, margin=MARGIN,
                            knocks=("D", "G"), _without=_without)
