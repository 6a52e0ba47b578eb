"""CPU references for the temporal pass that follows mirrors (tests/test_gpu_temporal_path.py,
tests/test_temporal_path_cpu.py):

  oracle_aov_path_points  tests/path_ref.oracle_aov_path with tpt_render_aov_path_points'
                          seventh output restated: the terminal world point origin_k + t d_k
                          in float32, formed as the walk advances an origin, or the unit
                          direction d_k of the last ray where the path leaves the scene;
  temporal_path_ref       a float64 numpy restatement of tpt_temporal_path as DESIGN.md
                          section 5 "Temporal accumulation through mirrors" defines it.

temporal_path_ref is tests/temporal_ref.temporal_ref with the rules of the new entry point:
a tap also needs the bounce count k' = k, and a pixel with k > 0 needs the tap's stored
terminal point (a direction where the path left the scene) within point_tol pixel
footprints of its own.  The rays are post_ref.pixel_centre_rays', so they are the kernel's
own float32 rays; everything after them is float64.  Where a float32 and a float64
evaluation could fall on different sides of a threshold the pixel is undecidable
(`decidable` mask): temporal_ref's margins, and a relative 1e-3 around the point and the
direction tolerance.

`_without` knocks one rule out (tests/test_temporal_path_cpu.py shows each one's teeth):
  "k"          the bounce counts are not compared;
  "point"      the terminal points of hit pixels are not compared;
  "direction"  the last directions of reflected sky are not compared;
  "virtual"    a followed hit reprojects its terminal point P itself and not the virtual
               image X = o + D d that the path's length D places behind the mirrors."""
import numpy as np

from tests import path_ref as P
from tests import post_ref as R
from tests.temporal_ref import ALBEDO_FLOOR, LUMA, MIN_WSUM, SNAP, sensor

F = np.float32
KNOCKS = ("k", "point", "direction", "virtual")
POINT_MARGIN = 1e-3


def oracle_aov_path_points(ps, W, H, max_bounces, cam=None, tracer=None):
    """path_ref.oracle_aov_path's walk, keeping each pixel's last ray.  Returns its dict
    plus "points" [H, W, 3] float32."""
    s = ps.src
    tr = tracer or P.Tracer(ps)
    c2w = cam["c2w"] if cam else s.camera_c2w
    vfov = cam["vfov"] if cam else s.vfov
    aspect = cam["aspect"] if cam else s.aspect
    origin, dirs = R.pixel_centre_rays(c2w, vfov, aspect, W, H)
    n = W * H
    o = np.tile(np.asarray(origin, F), (n, 1))
    d = np.ascontiguousarray(dirs.reshape(n, 3), F)
    mirror_of = P.is_mirror(tr.mtl)
    A = np.ones((n, 3), F)
    D = np.zeros(n, F)
    k = np.zeros(n, np.int32)
    face = np.full(n, -1, np.int32)
    material = np.full(n, -1, np.int32)
    normal = np.zeros((n, 3), F)
    points = np.zeros((n, 3), F)
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
        miss = live[~got]
        face[miss], material[miss], normal[miss] = -1, -1, F(0.0)
        points[miss] = d[miss]                                 # the path leaves the scene along d_k
        px, f, t, uv = live[got], hit[got], t[got], uv[got]
        nrm = tr.shading_normal(f, uv)
        m = tr.face_mtl[f]
        D[px] = (D[px] + t).astype(F)
        A[px] = (A[px] * tr.mtl[m, :3]).astype(F)
        face[px], material[px], normal[px] = f, m, nrm
        at = (o[px] + (t[:, None] * d[px]).astype(F)).astype(F)   # the advance: o + t d, no FMA
        points[px] = at
        go = mirror_of[m] & (k[px] < max_bounces)
        px, nrm, at = px[go], nrm[go], at[go]
        o[px] = at
        d[px] = P.reflect(d[px], nrm)
        k[px] += 1
        live = px
        hop += 1
    return {"albedo": A.reshape(H, W, 3), "normal": normal.reshape(H, W, 3), "depth": D.reshape(H, W),
            "face": face.reshape(H, W), "material": material.reshape(H, W), "bounces": k.reshape(H, W),
            "points": points.reshape(H, W, 3), "first_face": first_face.reshape(H, W),
            "first_material": first_material.reshape(H, W)}


def footprint(cam, H):
    """sensor_h / height of a camera dict, as float64 of the library's float32 sensor."""
    return np.float64(sensor(cam["vfov"], cam["aspect"])[1]) / H


def temporal_path_ref(state, cam, radiance, aov, alpha, depth_tol, normal_min, max_history, demodulate, point_tol,
                      _without=None):
    """One call of the definition.  aov: tpt_render_aov_path_points' buffers (normal, depth,
    material, bounces, points; albedo with demodulate).  state: None or the dict a previous
    call returned.  Returns temporal_ref's dict."""
    assert _without is None or _without in KNOCKS
    n = np.asarray(aov["normal"], np.float64)
    z = np.asarray(aov["depth"], np.float64)
    m = np.asarray(aov["material"], np.int64)
    k = np.asarray(aov["bounces"], np.int64)
    Pt = np.asarray(aov["points"], np.float64)
    H, W = z.shape
    a = np.maximum(np.asarray(aov["albedo"], np.float64), ALBEDO_FLOOR) if demodulate else 1.0
    c = np.asarray(radiance, np.float64) / a
    L = c @ LUMA
    hit = m >= 0
    followed = k > 0
    reproj = np.zeros((H, W), bool)
    decidable = np.ones((H, W), bool)
    hC, hN, hM1, hM2 = np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    if state is not None:
        o32, d32 = R.pixel_centre_rays(cam["c2w"], cam["vfov"], cam["aspect"], W, H)
        o, d = o32.astype(np.float64), d32.astype(np.float64)
        X = o + z[..., None] * d                               # k > 0: the virtual image of the terminal point
        if _without == "virtual":
            X = np.where((followed & hit)[..., None], Pt, X)
        pc = state["cam"]
        pm = np.asarray(pc["c2w"], F).astype(np.float64).reshape(4, 4).T
        inv = np.linalg.inv(pm).astype(F).astype(np.float64)   # double, rounded to float32
        po = pm[:3, 3]
        local = np.where(hit[..., None], X @ inv[:3, :3].T + inv[:3, 3], d @ inv[:3, :3].T)
        dist = np.linalg.norm(X - po, axis=-1)
        front = local[..., 2] < 0
        sw, sh, hsw, hsh = (np.float64(v) for v in sensor(pc["vfov"], pc["aspect"]))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            s = -1.0 / local[..., 2]
            fx = (local[..., 0] * s + hsw) / sw * W - 0.5
            fy = (local[..., 1] * s + hsh) / sh * H - 0.5
        fx = np.where(front & np.isfinite(fx), fx, -10.0)
        fy = np.where(front & np.isfinite(fy), fy, -10.0)
        fx, fy = np.clip(fx, -10.0, W + 10.0), np.clip(fy, -10.0, H + 10.0)
        for f in (fx, fy):
            off = np.abs(f - np.round(f))
            decidable &= ~(front & (np.abs(off - SNAP) < 1e-4))
        fx = np.where(np.abs(fx - np.round(fx)) < SNAP, np.round(fx), fx)
        fy = np.where(np.abs(fy - np.round(fy)) < SNAP, np.round(fy), fy)
        x0, y0 = np.floor(fx), np.floor(fy)
        tx, ty = fx - x0, fy - y0
        # the point rule's radius: point_tol footprints of the current camera at the path's
        # length; a direction's at distance 1
        tol = point_tol * footprint(cam, H) * np.where(hit, z, 1.0)
        use_point = followed & (hit if _without != "point" else False) | \
            followed & (~hit if _without != "direction" else False)
        wsum = np.zeros((H, W))
        for j in (0, 1):
            for i in (0, 1):
                w = (tx if i else 1.0 - tx) * (ty if j else 1.0 - ty)
                qx, qy = (x0 + i).astype(np.int64), (y0 + j).astype(np.int64)
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                match = front & (w > 0) & inside & (state["m"][qyc, qxc] == m)
                if _without != "k":
                    match &= state["k"][qyc, qxc] == k
                with np.errstate(divide="ignore", invalid="ignore"):
                    rel = np.abs(state["z"][qyc, qxc] - dist) / dist
                    off = np.linalg.norm(state["P"][qyc, qxc] - Pt, axis=-1) / tol
                ndot = (state["n"][qyc, qxc] * n).sum(-1)
                surf = match & hit
                decidable &= ~(surf & ((np.abs(rel - depth_tol) < 1e-3) | (np.abs(ndot - normal_min) < 1e-3)))
                decidable &= ~(match & use_point & (np.abs(off - 1.0) < POINT_MARGIN))
                valid = match & (~hit | ((rel <= depth_tol) & (ndot >= normal_min))) & (~use_point | (off <= 1.0))
                wv = np.where(valid, w, 0.0)
                wsum += wv
                hC += wv[..., None] * state["C"][qyc, qxc]
                hN += wv * state["N"][qyc, qxc]
                hM1 += wv * state["M1"][qyc, qxc]
                hM2 += wv * state["M2"][qyc, qxc]
        decidable &= ~(np.abs(wsum - MIN_WSUM) < 1e-3)
        reproj = wsum >= MIN_WSUM
        ws = np.where(reproj, wsum, 1.0)
        hC, hN, hM1, hM2 = hC / ws[..., None], hN / ws, hM1 / ws, hM2 / ws
    N = np.where(reproj, np.minimum(hN + 1.0, float(max_history)), 1.0)
    kk = np.maximum(alpha, 1.0 / N)
    Cn = np.where(reproj[..., None], hC + kk[..., None] * (c - hC), c)
    M1 = np.where(reproj, hM1 + kk * (L - hM1), L)
    M2 = np.where(reproj, hM2 + kk * (L * L - hM2), L * L)
    new = {"cam": cam, "C": Cn, "N": N, "M1": M1, "M2": M2, "n": n, "z": z, "m": m, "k": k, "P": Pt}
    return {"out": Cn * a, "variance": np.maximum(M2 - M1 * M1, 0.0), "history_len": N, "reprojected": reproj,
            "decidable": decidable, "state": new}


def first_hit_state(state):
    """The state as it is after a tpt_temporal call: every stored bounce count 0."""
    return dict(state, k=np.zeros_like(state["m"]), P=np.zeros(state["m"].shape + (3,)))
