"""CPU reference for the temporal pass: the one float64 numpy definition that every GPU test
of the temporal kernels is compared against, the synthetic three-patch scene whose feature
buffers the tests build analytically, and the cameras they move between.

temporal_core restates DESIGN.md section 5 "Post-pass" in the order the kernel text
(temporal_kernel.hpp) takes its steps, each step once: the lane's own pixel, where its
surface was, the projection into the previous camera, the four-tap gather, the optional
history clip, the blend, the new state.  The entry points are what differs between them:
  temporal_ref (here)                  tpt_temporal: nothing added;
  motion_ref.temporal_motion_ref       where the surface was, from the objects' matrices;
  deform_ref.temporal_deform_ref       where the surface was, from the snapshot's corners;
  temporal_path_ref.temporal_path_ref  a further tap rule (bounce count, terminal point);
  clip_ref                             the box that the clip step clamps to.

The state is one dict, as the library's tpt_history is one object: cam, C, N, M1, M2, n, z,
m always; k = 0 after a call without the path rule (the kernel writes 0.0f there); a
deform snapshot (wv, wn) that a call of another entry point keeps but marks invalid;
vert_trans after a motion call only.  Known gap: the library records the scene's
transforms on every call, the reference only on motion calls, which alone are given them.

The rays are post_ref.pixel_centre_rays', so they are the kernel's own float32 rays;
everything after them is float64.  Where a float32 and a float64 evaluation could
fall on different sides of one of the definition's thresholds the pixel is marked
undecidable and left out of comparisons (the `decidable` mask); the tests assert that
such pixels are at most 1 % of the frame.  The margins are each entry point's own."""
import numpy as np

from tests import post_ref as R

F = np.float32
SNAP = 1.0 / 1024.0
MIN_WSUM = 1.0 / 16.0
ALBEDO_FLOOR = 1e-3
LUMA = np.array([0.2126, 0.7152, 0.0722])


def sensor(vfov, aspect):
    """sensor_w, sensor_h, half_sw, half_sh as the library computes them (float32)."""
    tan_half = F(np.tan(np.float64(F(vfov) * F(0.5))))
    sensor_h = F(2.0) * tan_half
    sensor_w = F(aspect) * sensor_h
    return sensor_w, sensor_h, F(0.5) * sensor_w, F(0.5) * sensor_h


def camera(yaw_deg=0.0, translate=(0.0, 0.0, 0.0), vfov=0.8, aspect=1.0, pitch_deg=0.0, roll_deg=0.0):
    """A camera dict: the identity turned by R = R_y(yaw) R_x(pitch) R_z(roll) (roll
    about the viewing axis first, then pitch, then yaw about +y), then moved by
    `translate`.  c2w is 16 float32 values, column-major.  With pitch = roll = 0 the
    yaw matrix is not multiplied by anything, so those cameras are what they were
    before pitch and roll existed, bit for bit."""
    t = np.deg2rad(yaw_deg)
    m = np.eye(4)
    m[0, 0], m[0, 2], m[2, 0], m[2, 2] = np.cos(t), np.sin(t), -np.sin(t), np.cos(t)
    if pitch_deg != 0.0 or roll_deg != 0.0:
        p, r = np.deg2rad(pitch_deg), np.deg2rad(roll_deg)
        rx, rz = np.eye(3), np.eye(3)
        rx[1, 1], rx[1, 2], rx[2, 1], rx[2, 2] = np.cos(p), -np.sin(p), np.sin(p), np.cos(p)
        rz[0, 0], rz[0, 1], rz[1, 0], rz[1, 1] = np.cos(r), -np.sin(r), np.sin(r), np.cos(r)
        m[:3, :3] = m[:3, :3] @ rx @ rz
    m[:3, 3] = translate
    return {"c2w": m.T.reshape(16).astype(F), "vfov": float(vfov), "aspect": float(aspect)}


def synthetic_guides(cam, W, H, materials=(0, 1, 2)):
    """First hits of the pixel-centre rays against three world-space patches, closest
    first; everything else is a miss (normal 0, depth 0, material -1).
      far wall:    z = -4, normal +z, y < 1.0, material materials[0]
      near strip:  z = -2.5, normal +z, -0.4 < x < 0.5, y < 0.6, material materials[1]
      tilted wall: through (-1.2, 0, -4), normal (0.6, 0, 0.8), x < -1.2, y < 1.0, material materials[2]
    materials = (0, 0, 0) is the single-material scene: the same geometry, but only
    the depth and the normal rules can tell the patches apart."""
    o32, d32 = R.pixel_centre_rays(cam["c2w"], cam["vfov"], cam["aspect"], W, H)
    o, d = o32.astype(np.float64), d32.astype(np.float64)
    patches = [
        ((0.0, 0.0, -4.0), (0.0, 0.0, 1.0), lambda X: X[..., 1] < 1.0, materials[0]),
        ((0.0, 0.0, -2.5), (0.0, 0.0, 1.0), lambda X: (X[..., 0] > -0.4) & (X[..., 0] < 0.5) & (X[..., 1] < 0.6), materials[1]),
        ((-1.2, 0.0, -4.0), (0.6, 0.0, 0.8), lambda X: (X[..., 0] < -1.2) & (X[..., 1] < 1.0), materials[2]),
    ]
    best = np.full((H, W), np.inf)
    normal = np.zeros((H, W, 3), F)
    material = np.full((H, W), -1, np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for point, nrm, inside, mtl in patches:
            nrm = np.asarray(nrm)
            t = ((np.asarray(point) - o) @ nrm) / (d @ nrm)
            X = o + t[..., None] * d
            ok = np.isfinite(t) & (t > 0) & inside(X) & (t < best)
            best = np.where(ok, t, best)
            normal[ok] = nrm.astype(F)
            material[ok] = mtl
    depth = np.where(material >= 0, best, 0.0).astype(F)
    return {"normal": normal, "depth": depth, "material": material}


def colour(radiance, aov, demodulate):
    """The colour the temporal kernel accumulates, and the albedo it divides by."""
    a = np.maximum(np.asarray(aov["albedo"], np.float64), ALBEDO_FLOOR) if demodulate else 1.0
    return np.asarray(radiance, np.float64) / a, a


def temporal_core(state, cam, radiance, aov, alpha, depth_tol, normal_min, max_history, demodulate, *, clip=None,
                  source=None, motion=False, tap_rule=None, extra_state=None, margin=1e-3, normal_margin=None,
                  knocks=(), _without=None):
    """One call of the definition on a history.  state: None (after create / reset) or the dict
    a previous call of any entry point returned under `state`.  What an entry point adds:
      source(state, X, n, hit, o, d32) -> (X', ne, tracked): where each lane's surface was in
          the previous frame, the normal it had there, and whether that is known (absent: X, n,
          everywhere); motion: report `motion` [H, W, 2], the snapped, unclipped reprojection;
      tap_rule(state, qyc, qxc) -> (same, ok, near): a further rule on the tap at [qyc, qxc]:
          what must match for the tap to count at all, what a counted tap must pass, and where
          that is undecidable;
      extra_state: members the call adds to the new state;
      margin, normal_margin: the distance from a threshold (the normal rule's: normal_margin,
          margin if None) below which a pixel is undecidable; the snap's is 1e-4 everywhere;
      clip: dict(radius, gamma, max_history) of tpt_history_set_clip, or None;
      knocks: the entry point's own `_without` names, acted on in its hooks.
    Returns a dict: `out`, `variance`, `history_len` (float64), `reprojected`, `decidable`,
    `clipped`, `boxed` (bool masks), `n` (the box's tap count; the last three all-false and 0
    without a clip), `motion` if asked for, and the new state under `state`.  With a clip
    `decidable` also loses the reprojected pixels whose history lies within clip_ref.MARGIN of
    the value range of a box edge.

    _without (the teeth tests only) evaluates a *wrong* definition, one rule knocked out, to
    show that a test's inputs can see that rule: "prev_origin" measures the expected depth to
    the current origin instead of the previous one, "front" drops the local.z < 0 test, "dist"
    measures the expected depth from X instead of X', "cap" leaves a clipped pixel's history
    length alone, "shift" leaves its luminance moments alone; "similarity" and "n4" are
    clip_ref.box_ref's.  (The depth, normal and sensor rules need no switch: depth_tol 1e9,
    normal_min -1, a previous camera with the current sensor.)"""
    from tests import clip_ref as CR                                     # (it imports this module)
    assert _without in (None, "prev_origin", "front", "dist") + CR.KNOCKS + tuple(knocks)
    # 1. the lane's own pixel
    n = np.asarray(aov["normal"], np.float64)
    z = np.asarray(aov["depth"], np.float64)
    m = np.asarray(aov["material"], np.int64)
    H, W = z.shape
    c, a = colour(radiance, aov, demodulate)
    L = c @ LUMA
    hit = m >= 0
    reproj = np.zeros((H, W), bool)
    decidable = np.ones((H, W), bool)
    mv = np.zeros((H, W, 2))
    hC, hN, hM1, hM2 = np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    if state is not None:
        o32, d32 = R.pixel_centre_rays(cam["c2w"], cam["vfov"], cam["aspect"], W, H)
        o, d = o32.astype(np.float64), d32.astype(np.float64)
        X = o + z[..., None] * d
        # 2. where the surface was
        Xp, ne, tracked = source(state, X, n, hit, o, d32) if source else (X, n, np.ones((H, W), bool))
        # 3. into the previous camera
        pc = state["cam"]
        pm = np.asarray(pc["c2w"], F).astype(np.float64).reshape(4, 4).T
        inv = np.linalg.inv(pm).astype(F).astype(np.float64)          # double, rounded to float32
        po = pm[:3, 3]
        local = np.where(hit[..., None], Xp @ inv[:3, :3].T + inv[:3, 3], d @ inv[:3, :3].T)
        dist = np.linalg.norm((X if _without == "dist" else Xp) - po, axis=-1)
        front = (local[..., 2] < 0) & tracked
        if _without == "prev_origin":
            dist = np.linalg.norm(X - o, axis=-1)
        if _without == "front":
            front = np.ones((H, W), bool)
        sw, sh, hsw, hsh = (np.float64(v) for v in sensor(pc["vfov"], pc["aspect"]))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            s = -1.0 / local[..., 2]
            fx = (local[..., 0] * s + hsw) / sw * W - 0.5
            fy = (local[..., 1] * s + hsh) / sh * H - 0.5
        if motion:                                                      # after the snap, unclipped
            finite = front & np.isfinite(fx) & np.isfinite(fy)
            with np.errstate(invalid="ignore"):
                sx = np.where(np.abs(fx - np.round(fx)) < SNAP, np.round(fx), fx)
                sy = np.where(np.abs(fy - np.round(fy)) < SNAP, np.round(fy), fy)
            mv[..., 0] = np.where(finite, sx - np.arange(W, dtype=np.float64)[None, :], 0.0)
            mv[..., 1] = np.where(finite, sy - np.arange(H, dtype=np.float64)[:, None], 0.0)
        fx = np.where(front & np.isfinite(fx), fx, -10.0)               # behind: no tap; kept finite
        fy = np.where(front & np.isfinite(fy), fy, -10.0)
        fx, fy = np.clip(fx, -10.0, W + 10.0), np.clip(fy, -10.0, H + 10.0)
        for f in (fx, fy):
            off = np.abs(f - np.round(f))
            decidable &= ~(front & (np.abs(off - SNAP) < 1e-4))
        fx = np.where(np.abs(fx - np.round(fx)) < SNAP, np.round(fx), fx)
        fy = np.where(np.abs(fy - np.round(fy)) < SNAP, np.round(fy), fy)
        # 4. the gather
        x0, y0 = np.floor(fx), np.floor(fy)
        tx, ty = fx - x0, fy - y0
        wsum = np.zeros((H, W))
        nm = margin if normal_margin is None else normal_margin
        for j in (0, 1):
            for i in (0, 1):
                w = (tx if i else 1.0 - tx) * (ty if j else 1.0 - ty)
                qx, qy = (x0 + i).astype(np.int64), (y0 + j).astype(np.int64)
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                same, ok, near = tap_rule(state, qyc, qxc) if tap_rule else (True, True, False)
                match = front & (w > 0) & inside & (state["m"][qyc, qxc] == m) & same
                with np.errstate(divide="ignore", invalid="ignore"):
                    rel = np.abs(state["z"][qyc, qxc] - dist) / dist
                ndot = (state["n"][qyc, qxc] * ne).sum(-1)
                surf = match & hit
                decidable &= ~(surf & ((np.abs(rel - depth_tol) < margin) | (np.abs(ndot - normal_min) < nm)))
                decidable &= ~(match & near)
                valid = match & (~hit | ((rel <= depth_tol) & (ndot >= normal_min))) & ok
                wv = np.where(valid, w, 0.0)
                wsum += wv
                hC += wv[..., None] * state["C"][qyc, qxc]
                hN += wv * state["N"][qyc, qxc]
                hM1 += wv * state["M1"][qyc, qxc]
                hM2 += wv * state["M2"][qyc, qxc]
        decidable &= ~(np.abs(wsum - MIN_WSUM) < margin)
        reproj = wsum >= MIN_WSUM
        ws = np.where(reproj, wsum, 1.0)
        hC, hN, hM1, hM2 = hC / ws[..., None], hN / ws, hM1 / ws, hM2 / ws
    # 5. the clip: the gathered history clamped to the box of the current frame's colours
    clipped, nbox = np.zeros((H, W), bool), np.zeros((H, W), np.int64)
    if clip is not None:
        lo, hi, nbox = CR.box_ref(radiance, aov, clip["radius"], clip["gamma"], depth_tol, normal_min, demodulate,
                                  bounces=aov.get("bounces"), _without=_without if _without in CR.KNOCKS else None)
        hcl = np.minimum(np.maximum(hC, lo), hi)
        clipped = reproj & (hcl != hC).any(-1)
        span = max(float(np.abs(c).max()), float(np.abs(hC[reproj]).max(initial=0.0)), 1e-30)
        with np.errstate(invalid="ignore"):
            close = (np.abs(hC - lo) < CR.MARGIN * span) | (np.abs(hC - hi) < CR.MARGIN * span)
        decidable &= ~(reproj & close.any(-1))
        v = np.maximum(hM2 - hM1 * hM1, 0.0)
        Lc = hcl @ LUMA
        hC = np.where(clipped[..., None], hcl, hC)
        if _without != "cap":
            hN = np.where(clipped, np.minimum(hN, float(clip["max_history"])), hN)
        if _without != "shift":
            hM1, hM2 = np.where(clipped, Lc, hM1), np.where(clipped, v + Lc * Lc, hM2)
    # 6. the blend
    N = np.where(reproj, np.minimum(hN + 1.0, float(max_history)), 1.0)
    k = np.maximum(alpha, 1.0 / N)
    C = np.where(reproj[..., None], hC + k[..., None] * (c - hC), c)
    M1 = np.where(reproj, hM1 + k * (L - hM1), L)
    M2 = np.where(reproj, hM2 + k * (L * L - hM2), L * L)
    # 7. the new state
    new = {"cam": cam, "C": C, "N": N, "M1": M1, "M2": M2, "n": n, "z": z, "m": m, "k": np.zeros_like(m)}
    if state is not None and "wv" in state:                             # kept, but no longer the previous call's
        new.update(wv=state["wv"], wn=state["wn"], snap_valid=False)
    new.update(extra_state or {})
    res = {"out": C * a, "variance": np.maximum(M2 - M1 * M1, 0.0), "history_len": N, "reprojected": reproj,
           "decidable": decidable, "clipped": clipped, "boxed": nbox >= 4, "n": nbox, "state": new}
    return dict(res, motion=mv) if motion else res


def temporal_ref(state, cam, radiance, aov, alpha, depth_tol, normal_min, max_history, demodulate, clip=None,
                 _without=None):
    """tpt_temporal: temporal_core with nothing added."""
    return temporal_core(state, cam, radiance, aov, alpha, depth_tol, normal_min, max_history, demodulate, clip=clip,
                         _without=_without)
