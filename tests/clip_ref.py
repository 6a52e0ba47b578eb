"""CPU reference for history clipping (tests/test_gpu_clip.py, tests/test_clip_cpu.py): a float64
numpy restatement of tpt_history_set_clip's two steps as DESIGN.md section 5 "History clipping"
defines them -- the box of the current frame's colours around each pixel (k_clip_box) and the
clamp of the reprojected history to it (the k_temporal*_clip kernels) -- on top of the four
entry points' own references (temporal_ref, motion_ref, deform_ref, temporal_path_ref), none of
which is edited.

The similarity decisions of the box are taken in float32 in the order the definition writes
them, so they are the kernel's bit for bit; the moments and everything after them are float64.

The clamp sits between an entry point's gather and its blend, and the references return only the
blend.  The gather is taken from them all the same: called with alpha = 0 and an unbounded
max_history, a reference blends with k = 1 / N', N' = hN + 1, so that

    hN = N' - 1,   hC = (N' C' - c) / hN,   hM1 = (N' M1' - L) / hN,   hM2 = (N' M2' - L^2) / hN

give back the gathered history (hN >= 1 wherever a pixel is reprojected) to float64 rounding.
One restatement of the clamp and the blend then serves all four entry points."""
import numpy as np

from tests import temporal_ref as TR

F = np.float32
LUMA = TR.LUMA
ALBEDO_FLOOR = TR.ALBEDO_FLOOR
# test_gpu_temporal.BOUND_NEW: ten times the largest float32-against-float64 history difference
# measured at these frame sizes (8.609e-6, 131 x 9); the margin around a box edge inside which the
# float32 kernel and this reference may clamp differently, as a share of the value range
MARGIN = 10 * 8.609e-6
KNOCKS = ("similarity", "n4", "cap", "shift")
SPECK = 7                           # a material id no scene of the tests uses


def speck(aov, count=2):
    """`aov` with the material of `count` hit pixels (spread over the hit pixels in row-major
    order) replaced by SPECK: pixels without a similar neighbour, so n = 1 < 4 and no box.  Put
    into every frame of a sequence at the same places, a static camera reprojects them."""
    out = dict(aov)
    m = np.array(aov["material"], np.int32)
    hits = np.argwhere(m >= 0)
    for k in range(count):
        if len(hits):
            m[tuple(hits[(len(hits) * (2 * k + 1)) // (2 * count + 1)])] = SPECK
    out["material"] = m
    return out


def colour(radiance, aov, demodulate):
    """The colour the temporal kernel accumulates, and the albedo it divides by."""
    a = np.maximum(np.asarray(aov["albedo"], np.float64), ALBEDO_FLOOR) if demodulate else 1.0
    return np.asarray(radiance, np.float64) / a, a


def box_ref(radiance, aov, radius, gamma, depth_tol, normal_min, demodulate, bounces=None, _without=None):
    """k_clip_box: returns lo, hi ([H, W, 3] float64; -inf / +inf where n < 4) and n ([H, W] int).
    bounces: tpt_temporal_path's k, compared as well."""
    assert _without in (None,) + KNOCKS
    c, _ = colour(radiance, aov, demodulate)
    nr = np.asarray(aov["normal"], F)
    z = np.asarray(aov["depth"], F)
    m = np.asarray(aov["material"], np.int64)
    k = None if bounces is None else np.asarray(bounces, np.int64)
    H, W = z.shape
    hit = m >= 0
    ys, xs = np.mgrid[0:H, 0:W]
    n = np.zeros((H, W), np.int64)
    s1, s2 = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    ztol = (F(depth_tol) * z).astype(F)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            qy, qx = ys + dy, xs + dx
            inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
            qyc, qxc = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
            ok = inside & (m[qyc, qxc] == m)
            if k is not None:
                ok &= k[qyc, qxc] == k
            nq = nr[qyc, qxc]
            with np.errstate(invalid="ignore", over="ignore"):
                near = np.abs((z[qyc, qxc] - z).astype(F)) <= ztol                   # float32, as written
                ndot = ((nq[..., 0] * nr[..., 0] + nq[..., 1] * nr[..., 1]).astype(F) + nq[..., 2] * nr[..., 2]).astype(F)
            ok &= ~hit | (near & (ndot >= F(normal_min)))
            if _without == "similarity":
                ok = inside
            if dx == 0 and dy == 0:
                ok = np.ones((H, W), bool)                  # the centre always counts
            d = np.where(ok[..., None], c[qyc, qxc] - c, 0.0)
            n += ok
            s1 += d
            s2 += d * d
    nn = n[..., None].astype(np.float64)
    m1 = s1 / nn
    sigma = np.sqrt(np.maximum(s2 / nn - m1 * m1, 0.0))
    mu = c + m1
    lo, hi = mu - gamma * sigma, mu + gamma * sigma
    if _without != "n4":
        few = (n < 4)[..., None]
        lo, hi = np.where(few, -np.inf, lo), np.where(few, np.inf, hi)
    return lo, hi, n


def clipped_ref(base, state, cam, radiance, aov, *extra, clip, alpha, depth_tol, normal_min, max_history, demodulate,
                _without=None, **kw):
    """One clipped call of the entry point whose reference is `base` (TR.temporal_ref,
    MR.temporal_motion_ref, deform_ref.temporal_deform_ref, temporal_path_ref.temporal_path_ref;
    `extra` and `kw` are what that reference takes between `aov` and `alpha` and after
    `demodulate`).  clip: dict(radius, gamma, max_history), or None: the reference itself.
    Returns what `base` returns plus `clipped` and `boxed` (bool masks) and `n`; `decidable` loses
    the reprojected pixels whose history lies within MARGIN of the value range of a box edge.

    _without (tests/test_clip_cpu.py only) evaluates a wrong definition: "similarity" counts every
    in-frame tap, "n4" boxes a pixel however few taps it has, "cap" leaves a clipped pixel's
    history length alone, "shift" leaves its luminance moments alone."""
    assert _without in (None,) + KNOCKS
    rules = dict(depth_tol=depth_tol, normal_min=normal_min, demodulate=demodulate, **kw)
    if clip is None:
        r = base(state, cam, radiance, aov, *extra, alpha=alpha, max_history=max_history, **rules)
        H, W = r["reprojected"].shape
        return dict(r, clipped=np.zeros((H, W), bool), boxed=np.zeros((H, W), bool), n=np.zeros((H, W), np.int64))
    g = base(state, cam, radiance, aov, *extra, alpha=0.0, max_history=2.0 ** 40, **rules)
    reproj, decidable = g["reprojected"], g["decidable"].copy()
    c, a = colour(radiance, aov, demodulate)
    L = c @ LUMA
    lo, hi, n = box_ref(radiance, aov, clip["radius"], clip["gamma"], depth_tol, normal_min, demodulate,
                        bounces=aov.get("bounces"), _without=_without)
    Ng = g["state"]["N"]
    hN = np.where(reproj, Ng - 1.0, 1.0)
    hC = np.where(reproj[..., None], (Ng[..., None] * g["state"]["C"] - c) / hN[..., None], 0.0)
    hM1 = np.where(reproj, (Ng * g["state"]["M1"] - L) / hN, 0.0)
    hM2 = np.where(reproj, (Ng * g["state"]["M2"] - L * L) / hN, 0.0)
    hcl = np.minimum(np.maximum(hC, lo), hi)
    clipped = reproj & (hcl != hC).any(-1)
    span = max(float(np.abs(c).max()), float(np.abs(hC).max()), 1e-30)
    with np.errstate(invalid="ignore"):
        close = (np.abs(hC - lo) < MARGIN * span) | (np.abs(hC - hi) < MARGIN * span)
    decidable &= ~(reproj & close.any(-1))
    v = np.maximum(hM2 - hM1 * hM1, 0.0)
    Lc = hcl @ LUMA
    hC = np.where(clipped[..., None], hcl, hC)
    if _without != "cap":
        hN = np.where(clipped, np.minimum(hN, float(clip["max_history"])), hN)
    if _without != "shift":
        hM1, hM2 = np.where(clipped, Lc, hM1), np.where(clipped, v + Lc * Lc, hM2)
    N = np.where(reproj, np.minimum(hN + 1.0, float(max_history)), 1.0)
    k = np.maximum(alpha, 1.0 / N)
    C = np.where(reproj[..., None], hC + k[..., None] * (c - hC), c)
    M1 = np.where(reproj, hM1 + k * (L - hM1), L)
    M2 = np.where(reproj, hM2 + k * (L * L - hM2), L * L)
    new = dict(g["state"], C=C, N=N, M1=M1, M2=M2)
    return dict(g, out=C * a, variance=np.maximum(M2 - M1 * M1, 0.0), history_len=N, decidable=decidable, state=new,
                clipped=clipped, boxed=n >= 4, n=n)


def temporal_clip_ref(state, cam, radiance, aov, clip, **params):
    """tpt_temporal with the clip: clipped_ref over temporal_ref."""
    return clipped_ref(TR.temporal_ref, state, cam, radiance, aov, clip=clip, **params)
