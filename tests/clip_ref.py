"""CPU reference for history clipping (tests/test_gpu_clip.py, tests/test_clip_cpu.py): a float64
numpy restatement of the first of tpt_history_set_clip's two steps as DESIGN.md section 5
"History clipping" defines them: the box of the current frame's colours around each pixel
(k_clip_box).  The second, the clamp of the gathered history to that box (the k_temporal*_clip
kernels), sits between the gather and the blend of temporal_ref.temporal_core, which every
entry point's reference reaches with `clip=`.  Here are also the margin around a box edge, the
names of the clip's knock-outs and the speck pixels of the clip tests' frames.

The similarity decisions of the box are taken in float32 in the order the definition writes
them, so they are the kernel's bit for bit; the moments are float64."""
import numpy as np

from tests.temporal_ref import colour

F = np.float32
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
