"""CPU references for the temporal pass that follows mirrors (tests/test_gpu_temporal_path.py,
tests/test_temporal_path_cpu.py):

  oracle_aov_path_points  tests/path_ref.oracle_aov_path with tpt_render_aov_path_points'
                          seventh output restated: the terminal world point origin_k + t d_k
                          in float32, formed as the walk advances an origin, or the unit
                          direction d_k of the last ray where the path leaves the scene;
  temporal_path_ref       a float64 numpy restatement of tpt_temporal_path as DESIGN.md
                          section 5 "Temporal accumulation through mirrors" defines it.

The definition itself lives in tests/temporal_ref.temporal_core.  temporal_path_ref adds
what tpt_temporal_path adds: a further rule on each tap -- it also needs the bounce count
k' = k, and a pixel with k > 0 needs the tap's stored terminal point (a direction where
the path left the scene) within point_tol pixel footprints of its own -- and the state's
k and P.  Where a float32 and a float64 evaluation could fall on different sides of a
threshold the pixel is undecidable (`decidable` mask): temporal_ref's margins, and a
relative POINT_MARGIN around the point and the direction tolerance.

`_without` knocks one rule out (tests/test_temporal_path_cpu.py shows each one's teeth):
  "k"          the bounce counts are not compared;
  "point"      the terminal points of hit pixels are not compared;
  "direction"  the last directions of reflected sky are not compared;
  "virtual"    a followed hit reprojects its terminal point P itself and not the virtual
               image X = o + D d that the path's length D places behind the mirrors."""
import numpy as np

from tests import path_ref as P
from tests import post_ref as R
from tests.temporal_ref import sensor, temporal_core

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
                      clip=None, _without=None):
    """One call of the definition.  aov: tpt_render_aov_path_points' buffers (normal, depth,
    material, bounces, points; albedo with demodulate).  state: None or the dict a previous
    call of any entry point returned (a call without the path rule left k = 0 everywhere and
    no points, which no followed pixel matches).  Returns temporal_core's dict."""
    m = np.asarray(aov["material"], np.int64)
    k = np.asarray(aov["bounces"], np.int64)
    Pt = np.asarray(aov["points"], np.float64)
    hit, followed = m >= 0, k > 0
    # the point rule's radius: point_tol footprints of the current camera at the path's
    # length; a direction's at distance 1
    tol = point_tol * footprint(cam, m.shape[0]) * np.where(hit, np.asarray(aov["depth"], np.float64), 1.0)
    use_point = followed & (hit if _without != "point" else False) | \
        followed & (~hit if _without != "direction" else False)

    def virtual(state, X, n, hit, o, d32):      # knocked out: P itself, not its image behind the mirrors
        return np.where((followed & hit)[..., None], Pt, X), n, np.ones(hit.shape, bool)

    def tap_rule(state, qyc, qxc):
        was = state["P"][qyc, qxc] if "P" in state else 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            off = np.linalg.norm(was - Pt, axis=-1) / tol
        same = True if _without == "k" else state["k"][qyc, qxc] == k
        return same, ~use_point | (off <= 1.0), use_point & (np.abs(off - 1.0) < POINT_MARGIN)

    return temporal_core(state, cam, radiance, aov, alpha, depth_tol, normal_min, max_history, demodulate, clip=clip,
                         source=virtual if _without == "virtual" else None, tap_rule=tap_rule,
                         extra_state={"k": k, "P": Pt}, knocks=KNOCKS, _without=_without)
