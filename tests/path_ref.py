"""CPU restatement of tpt_render_aov_path (DESIGN.md section 5 "Post-pass", "Mirror-path
feature buffers"): tpt_render_aov's pixel-centre rays (tests/post_ref.py) continued
through perfect mirrors, one orc_trace_ray per hop over the oracle's BVH, the hit
prelude and the reflection in numpy float32 in the device's order of operations.

`knock` removes one rule of the definition (tests/test_path_ref_teeth.py):
  "no_product"  albedo = the terminal surface's base colour alone;
  "last_depth"  depth = the last hop's distance alone;
  "geo_normal"  reflect about the geometric normal instead of the shading normal;
  "emitter"     an emissive mirror does not end the path;
  "cap"         the cap is max_bounces + 1.
follow_glass=True is the variant DESIGN.md records as a negative (tools/aov_path_quality.py):
dielectrics are followed too, refracted, or reflected on total internal reflection."""
import numpy as np

from oracle import oracle as O

from tests import post_ref as R

F = np.float32
KEYS = ("albedo", "normal", "depth", "face", "material", "bounces")
DEFAULT_BASE = (0.82, 0.67, 0.16)                        # Material() (material.h:88-103)


def dot(a, b):
    """tpt_math.hpp dot: (a.x b.x + a.y b.y) + a.z b.z, float32."""
    return ((a[..., 0] * b[..., 0]).astype(F) + (a[..., 1] * b[..., 1]).astype(F)).astype(F) + \
        (a[..., 2] * b[..., 2]).astype(F)


def reflect(d, n):
    """reflect_dir (trace_dev.hpp; path_tracer.cu:137-141): d - (2 dot(d, n)) n, float32."""
    d, n = np.asarray(d, F), np.asarray(n, F)
    k = (F(2.0) * dot(d, n)).astype(F)
    return (d - (k[..., None] * n).astype(F)).astype(F)


def refract_or_reflect(d, n, eta_m):
    """new_direction's dielectric branch without its coin flip: the refracted direction
    (path_tracer.cu:143-163), the reflected one on total internal reflection."""
    d, n = np.asarray(d, F), np.asarray(n, F)
    cos_i = dot(d, n)
    eta = np.where(cos_i > 0, eta_m, F(1.0) / eta_m).astype(F)
    nn = np.where((cos_i > 0)[:, None], -n, n)
    cos_i = np.abs(cos_i)
    sin2t = eta * eta * (F(1.0) - cos_i * cos_i)
    tir = sin2t >= 1
    cos_t = np.sqrt(np.maximum(F(1.0) - sin2t, F(0.0))).astype(F)
    rf = (eta[:, None] * d + ((cos_i * eta - cos_t)[:, None] * nn)).astype(F)
    return np.where(tir[:, None], reflect(d, n), rf).astype(F)


def material_table(ps):
    """Rows (base colour [3], emission, eta, metallic) with the Material() slot appended."""
    mats = np.asarray(ps.src.materials, F).reshape(-1, 15)
    default = np.array([list(DEFAULT_BASE) + [0.0, 0.0, 0.0]], F)
    return np.concatenate([mats[:, :6], default]) if len(mats) else default


def is_mirror(rows, emitter_terminal=True):
    """new_direction's branch order: not a dielectric, metallic; an emitter ends the path."""
    m = ~(rows[:, 4] > 0) & (rows[:, 5] > 0)
    return m & ~(rows[:, 3] > 0) if emitter_terminal else m


class Tracer:
    """orc_trace_ray over one scene's BVH, built once."""

    def __init__(self, ps):
        self.ps = ps
        nodes, _, wv, wn = O.build_bvh(ps)
        self.nf = len(ps.indices) // 3
        self.nodes_c = (O.Node * len(nodes)).from_buffer_copy(nodes.tobytes())
        self.idx = np.ascontiguousarray(ps.indices)
        self.wv = np.ascontiguousarray(wv)
        self.wn = np.asarray(wn, F)
        self.tri = self.idx.reshape(-1, 3)
        self.face_mtl = R.face_material(ps, self.nf)
        self.mtl = material_table(ps)

    def trace(self, origins, dirs):
        n = len(origins)
        hit = np.full(n, -1, np.int32)
        t = np.zeros(n, F)
        uv = np.zeros((n, 2), F)
        tt = O.C.c_float()
        uu = (O.C.c_float * 2)()
        fn = O.lib().orc_trace_ray
        wv_p, idx_p = O._ptr(self.wv, O.C.c_float), O._ptr(self.idx, O.C.c_uint32)
        f3 = O.C.c_float * 3
        for i in range(n):
            hit[i] = fn(self.nodes_c, self.nf, wv_p, idx_p, f3(*origins[i]), f3(*dirs[i]), O.C.byref(tt), uu)
            if hit[i] >= 0:
                t[i] = tt.value
                uv[i] = uu[:]
        return hit, t, uv

    def shading_normal(self, face, uv):
        tri = self.tri[face]
        n0, n1, n2 = self.wn[tri[:, 0]], self.wn[tri[:, 1]], self.wn[tri[:, 2]]
        u, v = uv[:, 0:1], uv[:, 1:2]
        w = F(1.0) - u - v
        return R.normalize(((w * n0) + (u * n1)) + (v * n2))

    def geometric_normal(self, face):
        tri = self.tri[face]
        v0, v1, v2 = self.wv[tri[:, 0]], self.wv[tri[:, 1]], self.wv[tri[:, 2]]
        g = np.cross((v1 - v0).astype(np.float64), (v2 - v0).astype(np.float64))
        return (g / np.linalg.norm(g, axis=-1, keepdims=True)).astype(F)


def oracle_aov_path(ps, W, H, max_bounces, cam=None, knock=None, tracer=None, follow_glass=False):
    """The definition, hop by hop.  Returns renderAOVPath's dict ([H, W(, 3)], row 0 =
    bottom) plus "first_face" / "first_material": what the primary ray hits (-1: nothing)."""
    assert knock in (None, "no_product", "last_depth", "geo_normal", "emitter", "cap")
    s = ps.src
    tr = tracer or Tracer(ps)
    c2w = cam["c2w"] if cam else s.camera_c2w
    vfov = cam["vfov"] if cam else s.vfov
    aspect = cam["aspect"] if cam else s.aspect
    origin, dirs = R.pixel_centre_rays(c2w, vfov, aspect, W, H)
    n = W * H
    o = np.tile(np.asarray(origin, F), (n, 1))
    d = np.ascontiguousarray(dirs.reshape(n, 3), F)
    cap = max_bounces + 1 if knock == "cap" else max_bounces
    mirror_of = is_mirror(tr.mtl, emitter_terminal=knock != "emitter")
    A = np.ones((n, 3), F)
    D = np.zeros(n, F)
    k = np.zeros(n, np.int32)
    face = np.full(n, -1, np.int32)
    material = np.full(n, -1, np.int32)
    normal = np.zeros((n, 3), F)
    first_face = np.full(n, -1, np.int32)
    first_material = np.full(n, -1, np.int32)
    live = np.arange(n)
    hop = 0
    while len(live):
        hit, t, uv = tr.trace(o[live], d[live])
        got = hit >= 0
        if hop == 0:
            first_face[:] = hit
            first_material[got] = tr.face_mtl[hit[got]]
        miss = live[~got]                                  # the path ends: A and D stand
        face[miss], material[miss], normal[miss] = -1, -1, F(0.0)
        px, f, t, uv = live[got], hit[got], t[got], uv[got]
        nrm = tr.shading_normal(f, uv)
        m = tr.face_mtl[f]
        b = tr.mtl[m, :3]
        D[px] = t if knock == "last_depth" else (D[px] + t).astype(F)
        A[px] = b if knock == "no_product" else (A[px] * b).astype(F)
        face[px], material[px], normal[px] = f, m, nrm
        glass = (tr.mtl[m, 4] > 0) & (~(tr.mtl[m, 3] > 0)) if follow_glass else np.zeros(len(m), bool)
        go = (mirror_of[m] | glass) & (k[px] < cap)
        px, t, nrm, glass, eta = px[go], t[go], nrm[go], glass[go], tr.mtl[m[go], 4]
        if knock == "geo_normal":
            nrm = tr.geometric_normal(f[go])
        o[px] = (o[px] + (t[:, None] * d[px]).astype(F)).astype(F)
        nd = reflect(d[px], nrm)
        if glass.any():
            nd[glass] = refract_or_reflect(d[px][glass], nrm[glass], eta[glass])
        d[px] = nd
        k[px] += 1
        live = px
        hop += 1
    out = {"albedo": A.reshape(H, W, 3), "normal": normal.reshape(H, W, 3), "depth": D.reshape(H, W),
           "face": face.reshape(H, W), "material": material.reshape(H, W), "bounces": k.reshape(H, W),
           "first_face": first_face.reshape(H, W), "first_material": first_material.reshape(H, W)}
    return out


def uniform3x3(img):
    """test_gpu_aov.comparable's rule: the 3x3 neighbourhood (edges replicated) is uniform."""
    p = np.pad(img, 1, mode="edge")
    same = np.ones(img.shape, bool)
    for dy in range(3):
        for dx in range(3):
            same &= p[dy:dy + img.shape[0], dx:dx + img.shape[1]] == img
    return same


def comparable(ref):
    """A pixel whose first-hit face, terminal face and bounce count are each uniform over
    its 3x3 neighbourhood: a last-bit difference in a ray cannot change its path."""
    return uniform3x3(ref["first_face"]) & uniform3x3(ref["face"]) & uniform3x3(ref["bounces"])
