"""CPU reference for the temporal pass on deforming meshes (tests/test_deform_cpu.py,
test_deform_ref_teeth.py, test_gpu_deform.py): a float64 numpy restatement of
tpt_temporal_deform as DESIGN.md section 5 "Deforming meshes" defines it, built on
temporal_ref / motion_ref.

temporal_deform_ref is motion_ref.temporal_motion_ref with the object's matrices replaced by the
triangle's previous corners; where no triangle is deformed it performs temporal_ref's operations
in temporal_ref's order, so the two agree array for array (test_deform_cpu.py).  It carries the
same `decidable` mask.  Two discrete decisions are taken on float32 bits, as the kernel takes
them, and are therefore always decidable: whether a triangle is static (18 words compared), and
whether its determinant is zero (computed in float32 in the kernel's order of operations)."""
import numpy as np

from tests import motion_ref as MR
from tests import post_ref as R
from tests import temporal_ref as TR

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _cross32(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(F)


def _dot32(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]).astype(F) + a[..., 2] * b[..., 2]).astype(F)


def temporal_deform_ref(state, cam, radiance, aov, indices, wverts, wnorms, alpha, depth_tol, normal_min, max_history,
                        demodulate, deform=True, normal_margin=MR.MARGIN, _without=None):
    """One call on a history.  indices: the scene's [3 F]; wverts, wnorms: its world buffers at
    this call ([V, 3] float32).  state: None or what a previous call returned under `state`.
    deform=False is a call of another entry point (tpt_temporal: the face guide is not read): the
    snapshot it leaves is not the previous call's, so the next deform call disoccludes its hits.
    Returns temporal_ref's dict and `motion` [H, W, 2].

    normal_margin: the distance of n' . ne from normal_min below which the normal rule counts as
    undecidable (motion_ref's by default; a case that sets normal_min within 1e-3 of 1 passes its
    own, with its reasoning).

    _without (tests/test_deform_ref_teeth.py only) evaluates a wrong definition, one rule knocked
    out: "X" reprojects X instead of X' (the static assumption), "ne" compares the current
    normal, "current" applies the barycentrics to the current corners instead of the
    snapshot's, "snapshot" takes the snapshot for valid whatever call came in between."""
    assert _without in (None, "X", "ne", "current", "snapshot")
    n = np.asarray(aov["normal"], np.float64)
    z = np.asarray(aov["depth"], np.float64)
    m = np.asarray(aov["material"], np.int64)
    H, W = z.shape
    a = np.maximum(np.asarray(aov["albedo"], np.float64), TR.ALBEDO_FLOOR) if demodulate else 1.0
    c = np.asarray(radiance, np.float64) / a
    L = c @ TR.LUMA
    hit = m >= 0
    reproj = np.zeros((H, W), bool)
    decidable = np.ones((H, W), bool)
    motion = np.zeros((H, W, 2))
    hC, hN, hM1, hM2 = np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    wv32, wn32 = np.ascontiguousarray(wverts, F).reshape(-1, 3), np.ascontiguousarray(wnorms, F).reshape(-1, 3)
    if state is not None:
        o32, d32 = R.pixel_centre_rays(cam["c2w"], cam["vfov"], cam["aspect"], W, H)
        o, d = o32.astype(np.float64), d32.astype(np.float64)
        X = o + z[..., None] * d
        Xp, ne = X, n
        tracked = np.ones((H, W), bool)
        if deform:
            f = np.asarray(aov["face"], np.int64)
            tri = np.asarray(indices, np.int64).reshape(-1, 3)
            snap_ok = "wv" in state and (state["snap_valid"] or _without == "snapshot")
            in_range = (f >= 0) & (f < len(tri))
            tracked = ~hit | (in_range & bool(snap_ok))
            if snap_ok:
                ids = tri[np.clip(f, 0, len(tri) - 1)]                       # [H, W, 3]
                cv, cn = wv32[ids], wn32[ids]                               # [H, W, 3 corners, 3]
                pv, pn = state["wv"][ids], state["wn"][ids]
                same = (_bits(cv) == _bits(pv)).all((-1, -2)) & (_bits(cn) == _bits(pn)).all((-1, -2))
                moved = hit & in_range & ~same
                # the determinant as the kernel computes it: float32, rayHitTriangle's order
                e1, e2 = cv[..., 1, :] - cv[..., 0, :], cv[..., 2, :] - cv[..., 0, :]
                with np.errstate(all="ignore"):
                    den32 = _dot32(_cross32(d32, e2), e1)
                flat = moved & (den32 == 0)
                cv64, pv64, pn64, cn64 = (x.astype(np.float64) for x in (cv, pv, pn, cn))
                e1, e2, tv = cv64[..., 1, :] - cv64[..., 0, :], cv64[..., 2, :] - cv64[..., 0, :], o - cv64[..., 0, :]
                p, q = np.cross(d, e2), np.cross(tv, e1)
                with np.errstate(all="ignore"):
                    den = (p * e1).sum(-1)
                    u, v = (p * tv).sum(-1) / den, (q * d).sum(-1) / den
                    w = 1.0 - u - v
                    src_v, src_n = (cv64, cn64) if _without == "current" else (pv64, pn64)
                    Xd = (w[..., None] * src_v[..., 0, :] + u[..., None] * src_v[..., 1, :]) + v[..., None] * src_v[..., 2, :]
                    gn = (w[..., None] * src_n[..., 0, :] + u[..., None] * src_n[..., 1, :]) + v[..., None] * src_n[..., 2, :]
                    gn = gn / np.linalg.norm(gn, axis=-1, keepdims=True)
                finite = np.isfinite(u) & np.isfinite(v) & np.isfinite(Xd).all(-1)
                tracked &= ~(moved & (flat | ~finite))
                use = moved & tracked
                if _without != "X":
                    Xp = np.where(use[..., None], Xd, X)
                if _without != "ne":
                    ne = np.where(use[..., None], gn, n)
        pc = state["cam"]
        pm = np.asarray(pc["c2w"], F).astype(np.float64).reshape(4, 4).T
        inv = np.linalg.inv(pm).astype(F).astype(np.float64)          # double, rounded to float32
        po = pm[:3, 3]
        local = np.where(hit[..., None], Xp @ inv[:3, :3].T + inv[:3, 3], d @ inv[:3, :3].T)
        dist = np.linalg.norm(Xp - po, axis=-1)
        front = (local[..., 2] < 0) & tracked
        sw, sh, hsw, hsh = (np.float64(x) for x in TR.sensor(pc["vfov"], pc["aspect"]))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            s = -1.0 / local[..., 2]
            fx = (local[..., 0] * s + hsw) / sw * W - 0.5
            fy = (local[..., 1] * s + hsh) / sh * H - 0.5
        finite = front & np.isfinite(fx) & np.isfinite(fy)
        with np.errstate(invalid="ignore"):                             # tpt_temporal_motion's motion_out
            sx = np.where(np.abs(fx - np.round(fx)) < TR.SNAP, np.round(fx), fx)
            sy = np.where(np.abs(fy - np.round(fy)) < TR.SNAP, np.round(fy), fy)
        xs = np.arange(W, dtype=np.float64)[None, :]
        ys = np.arange(H, dtype=np.float64)[:, None]
        if deform:
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
                wt = (tx if i else 1.0 - tx) * (ty if j else 1.0 - ty)
                qx, qy = (x0 + i).astype(np.int64), (y0 + j).astype(np.int64)
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                match = front & (wt > 0) & inside & (state["m"][qyc, qxc] == m)
                with np.errstate(divide="ignore", invalid="ignore"):
                    rel = np.abs(state["z"][qyc, qxc] - dist) / dist
                ndot = (state["n"][qyc, qxc] * ne).sum(-1)
                surf = match & hit
                decidable &= ~(surf & ((np.abs(rel - depth_tol) < MR.MARGIN) | (np.abs(ndot - normal_min) < normal_margin)))
                valid = match & (~hit | ((rel <= depth_tol) & (ndot >= normal_min)))
                wq = np.where(valid, wt, 0.0)
                wsum += wq
                hC += wq[..., None] * state["C"][qyc, qxc]
                hN += wq * state["N"][qyc, qxc]
                hM1 += wq * state["M1"][qyc, qxc]
                hM2 += wq * state["M2"][qyc, qxc]
        decidable &= ~(np.abs(wsum - TR.MIN_WSUM) < MR.MARGIN)
        reproj = wsum >= TR.MIN_WSUM
        ws = np.where(reproj, wsum, 1.0)
        hC, hN, hM1, hM2 = hC / ws[..., None], hN / ws, hM1 / ws, hM2 / ws
    N = np.where(reproj, np.minimum(hN + 1.0, float(max_history)), 1.0)
    k = np.maximum(alpha, 1.0 / N)
    C = np.where(reproj[..., None], hC + k[..., None] * (c - hC), c)
    M1 = np.where(reproj, hM1 + k * (L - hM1), L)
    M2 = np.where(reproj, hM2 + k * (L * L - hM2), L * L)
    new = {"cam": cam, "C": C, "N": N, "M1": M1, "M2": M2, "n": n, "z": z, "m": m}
    if deform:                                                          # the snapshot, taken at the end of the call
        new.update(wv=wv32.copy(), wn=wn32.copy(), snap_valid=True)
    elif state is not None and "wv" in state:                           # kept, but no longer the previous call's
        new.update(wv=state["wv"], wn=state["wn"], snap_valid=False)
    return {"out": C * a, "variance": np.maximum(M2 - M1 * M1, 0.0), "history_len": N, "reprojected": reproj,
            "decidable": decidable, "motion": motion, "state": new}
