"""The synthetic inputs of the tpt_upsample tests: one analytic scene over the unit square,
sampled at each size's own pixel centres ((x + 0.5) / w, (y + 0.5) / h), so that the low-size and
the full-size feature buffers describe one scene as two renders of one camera do.  The scene: a
material split at u = 0.55 with a normal of its own on each side, a depth ramp with a step at
v = 0.5, a disc with spherical normals and its own depth, a block of miss pixels, and a vertical
bar 0.03 wide -- thinner than a low pixel of every case, so the low frame often misses it -- whose
albedo is black (demodulation divides by the floor)."""
import numpy as np

# (full size, low size): what each exercises is listed in tests/test_gpu_upsample.py
CASES = [((37, 29), (19, 15)), ((37, 29), (13, 10)), ((37, 29), (24, 17)), ((37, 29), (37, 29)),
         ((131, 9), (33, 3)), ((16, 16), (4, 4)), ((17, 16), (9, 8)), ((5, 3), (1, 1)), ((1, 1), (1, 1))]
CASE_IDS = [f"{W}x{H}-from-{wl}x{hl}" for (W, H), (wl, hl) in CASES]
SIGMA = dict(sigma_normal=0.3, sigma_depth=0.05)

ALBEDO = {0: (0.8, 0.7, 0.6), 1: (0.3, 0.5, 0.9), 2: (0.9, 0.2, 0.2), 3: (0.0, 0.0, 0.0), -1: (1.0, 1.0, 1.0)}
# the material-coded frame: one colour per material id, far apart
CODE = {0: (0.25, 1.5, 0.125), 1: (2.0, 0.5, 0.75), 2: (0.0625, 0.375, 3.0), 3: (4.0, 4.0, 0.5), -1: (1.0, 0.0, 1.0)}


def features(w, h):
    """The scene's feature buffers at w x h: albedo, normal [h, w, 3], depth [h, w] float32,
    material [h, w] int32, row 0 = bottom."""
    u = ((np.arange(w) + 0.5) / w)[None, :] + np.zeros((h, 1))
    v = ((np.arange(h) + 0.5) / h)[:, None] + np.zeros((1, w))
    m = np.where(u < 0.55, 0, 1).astype(np.int32)
    nrm = np.where((u < 0.55)[..., None], (0.0, 0.0, 1.0), (0.6, 0.0, 0.8))
    z = 2.0 + 0.5 * u + np.where(v >= 0.5, 1.5, 0.0)
    du, dv = (u - 0.3) / 0.18, (v - 0.6) / 0.18           # the disc
    d2 = du * du + dv * dv
    disc = d2 < 1.0
    nz = np.sqrt(np.maximum(1.0 - d2, 0.0))
    m = np.where(disc, 2, m)
    nrm = np.where(disc[..., None], np.stack([du, dv, nz], -1), nrm)
    z = np.where(disc, 1.5 - 0.3 * nz, z)
    bar = (u > 0.395) & (u < 0.425) & ~disc               # the bar, behind the disc
    m = np.where(bar, 3, m)
    nrm = np.where(bar[..., None], (0.0, 0.6, 0.8), nrm)
    z = np.where(bar, 1.8, z)
    miss = (u > 0.69) & (u < 0.91) & (v > 0.09) & (v < 0.31)
    m = np.where(miss, -1, m)
    nrm = np.where(miss[..., None], 0.0, nrm)
    z = np.where(miss, 0.0, z)
    alb = np.zeros((h, w, 3))
    for k, a in ALBEDO.items():
        alb = np.where((m == k)[..., None], a, alb)
    alb = alb * np.where((m == 0) | (m == 1), 1.0 - 0.3 * v, 1.0)[..., None]   # (textured walls)
    return {"albedo": alb.astype(np.float32), "normal": nrm.astype(np.float32), "depth": z.astype(np.float32),
            "material": m.astype(np.int32)}


def low_radiance(wl, hl, seed=23):
    """Seeded noise on a smooth ramp, [hl, wl, 3] float32 in [0, 3)."""
    rng = np.random.default_rng(seed + 1000 * wl + hl)
    ramp = np.linspace(0.0, 1.0, wl)[None, :, None] + np.zeros((hl, 1, 3))
    return (ramp + rng.uniform(0.0, 2.0, (hl, wl, 3))).astype(np.float32)


def material_coded(aov):
    """A frame that holds CODE[material] at every pixel of aov."""
    m = aov["material"]
    out = np.zeros(m.shape + (3,), np.float32)
    for k, c in CODE.items():
        out[m == k] = c
    return out


def case_inputs(full, low):
    """(radiance_low, aov_low, aov) of one case."""
    return low_radiance(*low), features(*low), features(*full)
