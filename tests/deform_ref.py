"""CPU reference for the temporal pass on deforming meshes (tests/test_deform_cpu.py,
test_deform_ref_teeth.py, test_gpu_deform.py): a float64 numpy restatement of
tpt_temporal_deform as DESIGN.md section 5 "Deforming meshes" defines it.

The definition itself lives in temporal_ref.temporal_core.  temporal_deform_ref adds what
tpt_temporal_deform adds: where each lane's surface was in the previous frame (its barycentrics
applied to the triangle's corners in the snapshot), the reported motion, and the snapshot
carried in the state, which a call of another entry point leaves invalid.  Where no triangle is
deformed that is X and n themselves, so it agrees with temporal_ref array for array
(test_deform_cpu.py).  The margins are motion_ref's.  Two discrete decisions are taken on float32
bits, as the kernel takes them, and are therefore always decidable: whether a triangle is static
(18 words compared), and whether its determinant is zero (computed in float32 in the kernel's
order of operations)."""
import numpy as np

from tests import motion_ref as MR
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
                        demodulate, clip=None, normal_margin=MR.MARGIN, _without=None):
    """One call on a history.  indices: the scene's [3 F]; wverts, wnorms: its world buffers at
    this call ([V, 3] float32).  state: None or what a previous call returned under `state`; after
    a call of another entry point the snapshot it holds is not the previous call's, so this call
    disoccludes its hits.  Returns temporal_core's dict with `motion` [H, W, 2].

    normal_margin: the distance of n' . ne from normal_min below which the normal rule counts as
    undecidable (motion_ref's by default; a case that sets normal_min within 1e-3 of 1 passes its
    own, with its reasoning).

    _without (tests/test_deform_ref_teeth.py only) evaluates a wrong definition, one rule knocked
    out: "X" reprojects X instead of X' (the static assumption), "ne" compares the current
    normal, "current" applies the barycentrics to the current corners instead of the
    snapshot's, "snapshot" takes the snapshot for valid whatever call came in between."""
    f = np.asarray(aov["face"], np.int64)
    tri = np.asarray(indices, np.int64).reshape(-1, 3)
    wv32, wn32 = np.ascontiguousarray(wverts, F).reshape(-1, 3), np.ascontiguousarray(wnorms, F).reshape(-1, 3)

    def source(state, X, n, hit, o, d32):
        d = d32.astype(np.float64)
        Xp, ne = X, n
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
        return Xp, ne, tracked

    snapshot = dict(wv=wv32.copy(), wn=wn32.copy(), snap_valid=True)    # taken at the end of the call
    return TR.temporal_core(state, cam, radiance, aov, alpha, depth_tol, normal_min, max_history, demodulate, clip=clip,
                            source=source, motion=True, extra_state=snapshot, margin=MR.MARGIN,
                            normal_margin=normal_margin, knocks=("X", "ne", "current", "snapshot"), _without=_without)
