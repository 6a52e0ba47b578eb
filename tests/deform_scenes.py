"""The deforming-mesh tests' scene (tests/test_deform_cpu.py, test_deform_ref_teeth.py,
test_gpu_deform.py): an 8 x 8-quad sheet (81 vertices, 128 triangles, smooth vertex normals,
material 0) at z = -2.5 that covers the middle of the view of temporal_ref's cameras, in front
of a two-triangle back wall (material 1) at z = -5 that leaves the sky showing at the frame's
edge, so all three kinds of pixel occur: deformable hits, static hits, misses.  Both objects'
matrices are the identity, so the world vertices are the object-space ones.

The deformations act on the sheet's vertices between frames; each returns (vertices, normals or
None for "the stored normals stay").  numpy_guides computes first-hit feature buffers on the CPU
by intersecting the pixel-centre rays with every triangle, for the tests that have no GPU."""
import numpy as np

from tests import post_ref as R

F = np.float32
QUADS = 8
HALF = 0.8                          # the sheet spans [-HALF, HALF]^2
Z_SHEET, Z_WALL = -2.5, -5.0
WALL_HALF = (2.2, 1.7)              # the 37 x 29 frame sees +-2.70 x +-2.11 at z = -5: sky all round
N_SHEET_VERTS = (QUADS + 1) ** 2
N_SHEET_FACES = 2 * QUADS * QUADS
N_FACES = N_SHEET_FACES + 2


def rest():
    """(indices uint32 [3 F], vertices [V, 3], normals [V, 3], lut [2, 2]) of the rest pose."""
    g = np.linspace(-HALF, HALF, QUADS + 1)
    xs, ys = np.meshgrid(g, g)
    sheet = np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, Z_SHEET)], -1)
    wx, wy = WALL_HALF
    wall = np.array([[-wx, -wy, Z_WALL], [wx, -wy, Z_WALL], [wx, wy, Z_WALL], [-wx, wy, Z_WALL]])
    idx = []
    for j in range(QUADS):
        for i in range(QUADS):
            a = j * (QUADS + 1) + i
            b, c, d = a + 1, a + QUADS + 2, a + QUADS + 1
            idx += [a, b, c, a, c, d]                       # counter-clockwise seen from +z
    w0 = N_SHEET_VERTS
    idx += [w0, w0 + 1, w0 + 2, w0, w0 + 2, w0 + 3]
    verts = np.concatenate([sheet, wall]).astype(F)
    norms = np.tile(np.array([0.0, 0.0, 1.0], F), (len(verts), 1))
    lut = np.array([[0, 0], [N_SHEET_FACES, 1]], np.int32)
    return np.array(idx, np.uint32), verts, norms, lut


FACE_MATERIAL = np.array([0] * N_SHEET_FACES + [1, 1], np.int32)


def scene(vertices=None, normals=None):
    """The scene as a tinypathtracer_amd.Scene (Scene.from_arrays), at rest or with these arrays."""
    import tinypathtracer_amd as T
    from tests import variant_scenes as VS
    idx, v, n, lut = rest()
    eye = np.tile(np.eye(4, dtype=F).reshape(16), (2, 1))
    # the wall emits, so that a rendered frame shows the sheet's outline against it
    mats = np.stack([VS.material_row((0.8, 0.6, 0.4)), VS.material_row((0.3, 0.5, 0.7), emission=2.0)])
    return T.Scene.from_arrays(idx, v if vertices is None else vertices, n if normals is None else normals, lut, eye,
                               eye.copy(), mats)


# ---- the deformations: sheet vertices [81, 3] float32 at rest -> (vertices, normals or None) ----

def bulge(v, amp=0.6):
    """(a) Towards the camera by up to amp (0.6: a quarter of the sheet's 2.5 depth), a Gaussian
    of width 0.39 about the centre; the normals stay, so only the distance of X' can tell."""
    out = v.astype(np.float64).copy()
    out[:, 2] += amp * np.exp(-(out[:, 0] ** 2 + out[:, 1] ** 2) / 0.3)
    return out.astype(F), None


def swirl(v, theta0=0.547):
    """(b) In the plane, about the centre, by theta0 (1 - r / HALF) radians: r theta is largest
    at r = HALF / 2, 0.2 theta0 = 0.109 world units = 1.5 px of the 37 x 29 frame (13.7 px per
    unit at z = -2.5)."""
    out = v.astype(np.float64).copy()
    r = np.hypot(out[:, 0], out[:, 1])
    t = theta0 * np.clip(1.0 - r / HALF, 0.0, None)
    x, y = out[:, 0].copy(), out[:, 1].copy()
    out[:, 0] = np.cos(t) * x - np.sin(t) * y
    out[:, 1] = np.sin(t) * x + np.cos(t) * y
    return out.astype(F), None


def bend(v, k=0.131):
    """(c) z = Z_SHEET - k x^2 / 2 with the surface's own normals (k x, 0, 1) normalised:
    atan(k HALF) = 6.0 degrees at the edges, 0.042 deep (1.7 % of the distance)."""
    out = v.astype(np.float64).copy()
    out[:, 2] -= 0.5 * k * out[:, 0] ** 2
    n = np.stack([k * out[:, 0], np.zeros(len(out)), np.ones(len(out))], -1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    return out.astype(F), n.astype(F)


def half(v, step=(0.08, 0.05, 0.0)):
    """(e) The vertices with x > 0 (36 of 81) move by `step`; the triangles left of the column
    x = 0 stay bit for bit, the column's own triangles stretch, the others translate: static and
    deformed triangles inside one wave."""
    out = v.copy()
    out[v[:, 0] > 0] += np.asarray(step, F)
    return out, None


def deformed(fn, **kw):
    """(vertices, normals) of the whole scene with the sheet under `fn` (None: at rest)."""
    _, v, n, _ = rest()
    if fn is None:
        return v, n
    sv, sn = fn(v[:N_SHEET_VERTS], **kw)
    v, n = v.copy(), n.copy()
    v[:N_SHEET_VERTS] = sv
    if sn is not None:
        n[:N_SHEET_VERTS] = sn
    return v, n


def numpy_guides(cam, W, H, wv, wn):
    """First-hit feature buffers of the pixel-centre rays (the kernel's own float32 rays) against
    every triangle, in float64: normal (interpolated, unit length), depth, material, face."""
    idx = rest()[0].reshape(-1, 3).astype(np.int64)
    o32, d32 = R.pixel_centre_rays(cam["c2w"], cam["vfov"], cam["aspect"], W, H)
    o, d = o32.astype(np.float64), d32.astype(np.float64)
    v, nn = np.asarray(wv, np.float64), np.asarray(wn, np.float64)
    best = np.full((H, W), np.inf)
    face = np.full((H, W), -1, np.int32)
    normal = np.zeros((H, W, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        for f, (i0, i1, i2) in enumerate(idx):
            e1, e2, tv = v[i1] - v[i0], v[i2] - v[i0], o - v[i0]
            p = np.cross(d, e2)
            q = np.cross(tv, e1)
            den = p @ e1
            u, w = (p @ tv) / den, (d @ q) / den
            t = (q @ e2) / den
            ok = (den != 0) & (u >= 0) & (w >= 0) & (u + w <= 1) & (t > 1e-4) & (t < best)
            best = np.where(ok, t, best)
            face[ok] = f
            n = (1 - u - w)[..., None] * nn[i0] + u[..., None] * nn[i1] + w[..., None] * nn[i2]
            n = n / np.linalg.norm(n, axis=-1, keepdims=True)
            normal[ok] = n[ok]
    hit = face >= 0
    return {"normal": normal.astype(F), "depth": np.where(hit, best, 0.0).astype(F),
            "material": np.where(hit, FACE_MATERIAL[np.clip(face, 0, None)], -1).astype(np.int32), "face": face}


def wave(scene, obj, amp, frame):
    """tpt_render --wave OBJ AMP on a loaded scene: (first vertex, positions) of object `obj`'s
    vertex range in frame `frame`, every vertex its faces name displaced along its own object-space
    normal by amp sin(6 y_obj + frame); the factor in double, rounded once, the rest in float32."""
    lut = np.asarray(scene.lut, np.int64).reshape(-1, 2)
    begin = int(lut[obj, 0])
    end = int(lut[obj + 1, 0]) if obj + 1 < len(lut) else scene.n_faces
    ids = np.unique(np.asarray(scene.indices, np.int64)[3 * begin:3 * end])
    lo, hi = int(ids.min()), int(ids.max())
    out = np.asarray(scene.vertices, F)[lo:hi + 1].copy()
    k = ids - lo
    s = (amp * np.sin(6.0 * out[k, 1].astype(np.float64) + float(frame))).astype(F)
    out[k] = out[k] + s[:, None] * np.asarray(scene.normals, F)[ids]
    return lo, out
