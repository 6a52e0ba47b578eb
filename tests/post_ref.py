"""CPU references for the post-pass tests (tests/test_gpu_aov.py, test_gpu_denoise.py,
tools/denoise_quality.py): the pixel-centre rays of tpt_render_aov in numpy float32,
their first hits through the oracle, and a float64 restatement of the a-trous filter
as DESIGN.md section 5 "Post-pass" defines it."""
import numpy as np

from oracle import oracle as O

F = np.float32


def frsqrt(x):
    """vec.h:25-38: the Quake inverse square root with one Newton step, float32."""
    x = np.asarray(x, F)
    x2 = x * F(0.5)
    y = (np.int32(0x5f3759df) - (x.view(np.int32) >> 1)).view(F)
    return y * (F(1.5) - (x2 * y * y))


def normalize(v):
    v = np.asarray(v, F)
    n2 = v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]
    return frsqrt(n2)[..., None] * v


def pixel_centre_rays(c2w, vfov, aspect, W, H):
    """sampleRays (path_tracer.cu:42-59) with the jitter fixed at (0.5, 0.5), in its
    order of operations, float32 throughout.  Returns (origin [3], dirs [H, W, 3]),
    row 0 = bottom."""
    m = np.asarray(c2w, F).reshape(16)                   # column-major
    tan_half = F(np.tan(np.float64(F(vfov) * F(0.5))))
    sensor_h = F(2.0) * tan_half
    sensor_w = F(aspect) * sensor_h
    half_sw, half_sh = F(0.5) * sensor_w, F(0.5) * sensor_h
    inv_w, inv_h = F(1.0) / F(W), F(1.0) / F(H)
    x = np.arange(W, dtype=F)[None, :] + np.zeros((H, 1), F)
    y = np.arange(H, dtype=F)[:, None] + np.zeros((1, W), F)
    lx = ((F(0.5) + x) * inv_w) * sensor_w
    ly = ((F(0.5) + y) * inv_h) * sensor_h
    v = (lx - half_sw, ly - half_sh, F(-1.0), F(0.0))

    def row(i, vec):                                     # mat.h:37-51: from 0, column by column
        acc = np.zeros((H, W), F)
        for j in range(4):
            acc = acc + m[4 * j + i] * vec[j]
        return acc.astype(F)

    d = np.stack([row(0, v), row(1, v), row(2, v)], -1).astype(F)
    origin = m[12:15].copy()                             # c2w * (0, 0, 0, 1), :57
    return origin, normalize(d)


def face_material(ps, n_faces):
    """The LUT search of every face (mesh.cuh:74-78): object o owns faces
    [begin_o, begin_o+1); out-of-range material ids take the Material() slot."""
    lut = np.asarray(ps.src.lut, np.int64).reshape(-1, 2)
    obj = np.searchsorted(lut[:, 0], np.arange(n_faces), side="right") - 1
    mtl = lut[obj, 1]
    nm = len(ps.src.materials)
    return np.where((mtl < 0) | (mtl >= nm), nm, mtl).astype(np.int32)


def oracle_aov(ps, W, H, cam=None):
    """First hits of the pixel-centre rays through the oracle's traversal
    (orc_trace_ray over the oracle's BVH) and the numpy hit prelude
    (path_tracer.cu:364-374).  Returns a dict like PathTracer.renderAOV's."""
    s = ps.src
    c2w = cam["c2w"] if cam else s.camera_c2w
    vfov = cam["vfov"] if cam else s.vfov
    aspect = cam["aspect"] if cam else s.aspect
    origin, dirs = pixel_centre_rays(c2w, vfov, aspect, W, H)
    nodes, _, wv, wn = O.build_bvh(ps)
    nf = len(ps.indices) // 3
    nodes_c = (O.Node * len(nodes)).from_buffer_copy(nodes.tobytes())
    idx = np.ascontiguousarray(ps.indices)
    wv = np.ascontiguousarray(wv)
    n = W * H
    face = np.full(n, -1, np.int32)
    t = np.zeros(n, F)
    uv = np.zeros((n, 2), F)
    flat = np.ascontiguousarray(dirs.reshape(n, 3))
    o_c = (O.C.c_float * 3)(*origin)
    trace = O.lib().orc_trace_ray
    wv_p, idx_p = O._ptr(wv, O.C.c_float), O._ptr(idx, O.C.c_uint32)
    tt = O.C.c_float()
    uu = (O.C.c_float * 2)()
    for i in range(n):
        face[i] = trace(nodes_c, nf, wv_p, idx_p, o_c, (O.C.c_float * 3)(*flat[i]), O.C.byref(tt), uu)
        if face[i] >= 0:
            t[i] = tt.value
            uv[i] = uu[:]
    hit = face >= 0
    fm = face_material(ps, nf)
    mats = np.asarray(s.materials, F).reshape(-1, 15)
    base = np.concatenate([mats[:, :3], np.array([[0.82, 0.67, 0.16]], F)]) if len(mats) else \
        np.array([[0.82, 0.67, 0.16]], F)               # Material() default (material.h:88-103)
    material = np.where(hit, fm[np.maximum(face, 0)], -1).astype(np.int32)
    albedo = np.where(hit[:, None], base[np.maximum(material, 0)], F(1.0)).astype(F)
    tri = idx.reshape(-1, 3)[np.maximum(face, 0)]
    wn = np.asarray(wn, F)
    n0, n1, n2 = wn[tri[:, 0]], wn[tri[:, 1]], wn[tri[:, 2]]
    u, v = uv[:, 0:1], uv[:, 1:2]
    w = F(1.0) - u - v
    normal = np.where(hit[:, None], normalize(((w * n0) + (u * n1)) + (v * n2)), F(0.0)).astype(F)
    return {"albedo": albedo.reshape(H, W, 3), "normal": normal.reshape(H, W, 3), "depth": t.reshape(H, W),
            "face": face.reshape(H, W), "material": material.reshape(H, W)}


H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float64)


def atrous_ref(radiance, albedo, normal, depth, iterations, sigma_color, sigma_normal, sigma_depth, demodulate):
    """The filter definition, float64 (inputs [H, W, 3] / [H, W]; any row order,
    the filter is symmetric).  iterations 0 returns the input unchanged."""
    if iterations == 0:
        return np.array(radiance, copy=True)
    c = np.asarray(radiance, np.float64)
    a = np.maximum(np.asarray(albedo, np.float64), 1e-3)
    n = np.asarray(normal, np.float64)
    z = np.asarray(depth, np.float64)
    if demodulate:
        c = c / a
    Hh, Ww = z.shape
    kz = 1.0 / (sigma_depth ** 2 * np.maximum(z * z, 1e-12))
    with np.errstate(under="ignore"):
        for i in range(iterations):
            s = 1 << i
            sc2 = (sigma_color * 2.0 ** -i) ** 2
            num = np.zeros_like(c)
            den = np.zeros((Hh, Ww))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = dy * s, dx * s
                    # p ranges over the pixels whose tap q = p + (ox, oy) is inside the frame
                    py = slice(max(0, -oy), min(Hh, Hh - oy))
                    px = slice(max(0, -ox), min(Ww, Ww - ox))
                    if py.start >= py.stop or px.start >= px.stop:
                        continue
                    qy = slice(py.start + oy, py.stop + oy)
                    qx = slice(px.start + ox, px.stop + ox)
                    dc = ((c[py, px] - c[qy, qx]) ** 2).sum(-1)
                    dn = ((n[py, px] - n[qy, qx]) ** 2).sum(-1)
                    dz = (z[py, px] - z[qy, qx]) ** 2
                    w = H5[dx + 2] * H5[dy + 2] * np.exp(-dc / sc2) * np.exp(-dn / sigma_normal ** 2) * \
                        np.exp(-dz * kz[py, px])
                    num[py, px] += w[..., None] * c[qy, qx]
                    den[py, px] += w
            c = num / den[..., None]
    if demodulate:
        c = c * a
    return c
