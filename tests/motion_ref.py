"""CPU reference for the motion-aware temporal pass (tests/test_gpu_motion.py,
tests/test_motion_api.py, tests/test_motion_ref_teeth.py): a float64 numpy restatement of
tpt_temporal_motion as DESIGN.md section 5 "Moving objects" defines it, of
tpt_motion_matrices, and temporal_ref's three synthetic patches bound to objects of a
scene and moved with them.

temporal_motion_ref is temporal_ref.temporal_ref with the numbered changes of the
definition; where every object stands still it performs temporal_ref's operations in
temporal_ref's order, so the two agree array for array (test_motion_api.py).  It carries
the same `decidable` mask: pixels within 1e-3 of a threshold are left out of comparisons.
MARGIN is that 1e-3 less one part in 10^9: a turned normal against normal_min 0.999 gives
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
                        demodulate, _without=None):
    """One call of the definition.  carrier: the scene's lut (Carrier); vert_trans: its
    objects' matrices at this call ([n, 16] float32); state: None or what a previous call
    returned under `state` (it holds that call's matrices).  Returns temporal_ref's dict and
    `motion` [H, W, 2].

    _without (tests/test_motion_ref_teeth.py only) evaluates a wrong definition, one rule
    knocked out: "D" reprojects X instead of X' (the static assumption), "G" compares the
    unrotated normal, "dist" measures the expected depth from X instead of X'."""
    assert _without in (None, "D", "G", "dist")
    n = np.asarray(aov["normal"], np.float64)
    z = np.asarray(aov["depth"], np.float64)
    m = np.asarray(aov["material"], np.int64)
    f = np.asarray(aov["face"], np.int64)
    H, W = z.shape
    a = np.maximum(np.asarray(aov["albedo"], np.float64), TR.ALBEDO_FLOOR) if demodulate else 1.0
    c = np.asarray(radiance, np.float64) / a
    L = c @ TR.LUMA
    hit = m >= 0
    reproj = np.zeros((H, W), bool)
    decidable = np.ones((H, W), bool)
    motion = np.zeros((H, W, 2))
    hC, hN, hM1, hM2 = np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    vert_trans = np.asarray(vert_trans, F).reshape(-1, 16).copy()
    if state is not None:
        o32, d32 = R.pixel_centre_rays(cam["c2w"], cam["vfov"], cam["aspect"], W, H)
        o, d = o32.astype(np.float64), d32.astype(np.float64)
        X = o + z[..., None] * d
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
        Xp = X if _without == "D" else Xm
        if _without == "G":
            ne = n
        pc = state["cam"]
        pm = np.asarray(pc["c2w"], F).astype(np.float64).reshape(4, 4).T
        inv = np.linalg.inv(pm).astype(F).astype(np.float64)          # double, rounded to float32
        po = pm[:3, 3]
        local = np.where(hit[..., None], Xp @ inv[:3, :3].T + inv[:3, 3], d @ inv[:3, :3].T)
        dist = np.linalg.norm((X if _without == "dist" else Xp) - po, axis=-1)
        front = (local[..., 2] < 0) & tracked
        sw, sh, hsw, hsh = (np.float64(v) for v in TR.sensor(pc["vfov"], pc["aspect"]))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            s = -1.0 / local[..., 2]
            fx = (local[..., 0] * s + hsw) / sw * W - 0.5
            fy = (local[..., 1] * s + hsh) / sh * H - 0.5
        finite = front & np.isfinite(fx) & np.isfinite(fy)
        with np.errstate(invalid="ignore"):                             # change 8: after the snap, unclipped
            sx = np.where(np.abs(fx - np.round(fx)) < TR.SNAP, np.round(fx), fx)
            sy = np.where(np.abs(fy - np.round(fy)) < TR.SNAP, np.round(fy), fy)
        xs = np.arange(W, dtype=np.float64)[None, :]
        ys = np.arange(H, dtype=np.float64)[:, None]
        motion[..., 0] = np.where(finite, sx - xs, 0.0)
        motion[..., 1] = np.where(finite, sy - ys, 0.0)
        fx = np.where(front & np.isfinite(fx), fx, -10.0)               # behind: no tap; kept finite
        fy = np.where(front & np.isfinite(fy), fy, -10.0)
        fx, fy = np.clip(fx, -10.0, W + 10.0), np.clip(fy, -10.0, H + 10.0)
        for g in (fx, fy):
            off = np.abs(g - np.round(g))
            decidable &= ~(front & (np.abs(off - TR.SNAP) < 1e-4))
        fx = np.where(np.abs(fx - np.round(fx)) < TR.SNAP, np.round(fx), fx)
        fy = np.where(np.abs(fy - np.round(fy)) < TR.SNAP, np.round(fy), fy)
        x0, y0 = np.floor(fx), np.floor(fy)
        tx, ty = fx - x0, fy - y0
        wsum = np.zeros((H, W))
        for j in (0, 1):
            for i in (0, 1):
                w = (tx if i else 1.0 - tx) * (ty if j else 1.0 - ty)
                qx, qy = (x0 + i).astype(np.int64), (y0 + j).astype(np.int64)
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                match = front & (w > 0) & inside & (state["m"][qyc, qxc] == m)
                with np.errstate(divide="ignore", invalid="ignore"):
                    rel = np.abs(state["z"][qyc, qxc] - dist) / dist
                ndot = (state["n"][qyc, qxc] * ne).sum(-1)
                surf = match & hit
                decidable &= ~(surf & ((np.abs(rel - depth_tol) < MARGIN) | (np.abs(ndot - normal_min) < MARGIN)))
                valid = match & (~hit | ((rel <= depth_tol) & (ndot >= normal_min)))
                wv = np.where(valid, w, 0.0)
                wsum += wv
                hC += wv[..., None] * state["C"][qyc, qxc]
                hN += wv * state["N"][qyc, qxc]
                hM1 += wv * state["M1"][qyc, qxc]
                hM2 += wv * state["M2"][qyc, qxc]
        decidable &= ~(np.abs(wsum - TR.MIN_WSUM) < MARGIN)
        reproj = wsum >= TR.MIN_WSUM
        ws = np.where(reproj, wsum, 1.0)
        hC, hN, hM1, hM2 = hC / ws[..., None], hN / ws, hM1 / ws, hM2 / ws
    N = np.where(reproj, np.minimum(hN + 1.0, float(max_history)), 1.0)
    k = np.maximum(alpha, 1.0 / N)
    C = np.where(reproj[..., None], hC + k[..., None] * (c - hC), c)
    M1 = np.where(reproj, hM1 + k * (L - hM1), L)
    M2 = np.where(reproj, hM2 + k * (L * L - hM2), L * L)
    new = {"cam": cam, "C": C, "N": N, "M1": M1, "M2": M2, "n": n, "z": z, "m": m, "vert_trans": vert_trans}
    return {"out": C * a, "variance": np.maximum(M2 - M1 * M1, 0.0), "history_len": N, "reprojected": reproj,
            "decidable": decidable, "motion": motion, "state": new}
