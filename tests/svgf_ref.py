"""CPU reference of tpt_denoise_svgf (tests/test_gpu_svgf.py, test_svgf_api.py,
test_svgf_ref_teeth.py, tools/svgf_quality.py): a float64 restatement of the
variance-guided a-trous filter as DESIGN.md section 5 "Post-pass" defines it.  What it
shares with the plain filter (the taps h) comes from tests/post_ref.py."""
import numpy as np

from tests.post_ref import H5

G3 = np.array([1 / 4, 1 / 2, 1 / 4], np.float64)
LUM = np.array([0.2126, 0.7152, 0.0722], np.float64)

# the rules test_svgf_ref_teeth.py knocks out (svgf_ref's _without)
RULES = ("per_pixel_variance", "prefilter", "estimate", "boost", "squared")


def _taps(Hh, Ww, radius, step):
    """For every offset of the window: (dy, dx, the slices of p, the slices of q = p +
    step (dx, dy)), p ranging over the pixels whose tap is inside the frame."""
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            oy, ox = dy * step, dx * step
            py = slice(max(0, -oy), min(Hh, Hh - oy))
            px = slice(max(0, -ox), min(Ww, Ww - ox))
            if py.start >= py.stop or px.start >= px.stop:
                continue
            yield dy, dx, (py, px), (slice(py.start + oy, py.stop + oy), slice(px.start + ox, px.stop + ox))


def svgf_ref(radiance, albedo, normal, depth, variance=None, history_len=None, iterations=5, sigma_lum=4.0,
             sigma_normal=0.3, sigma_depth=0.05, min_history=4, demodulate=True, _without=None):
    """The filter definition, float64 (inputs [H, W, 3] / [H, W]; any row order, the
    filter is symmetric).  Returns a dict: `out` [H, W, 3] (iterations 0: the input
    unchanged), `variance` [H, W] (the filtered variance; iterations 0: v0), `v0`,
    `short` (the pixels that took the spatial estimate) and `estimated`, their count.
    _without: one of RULES, knocked out."""
    assert _without is None or _without in RULES
    if history_len is not None and variance is None:
        raise ValueError("history_len needs a variance")
    c = np.asarray(radiance, np.float64)
    a = np.maximum(np.asarray(albedo, np.float64), 1e-3) if demodulate else None
    n = np.asarray(normal, np.float64)
    z = np.asarray(depth, np.float64)
    if demodulate:
        c = c / a
    Hh, Ww = z.shape
    kz = 1.0 / (sigma_depth ** 2 * np.maximum(z * z, 1e-12))

    def w_guide(p, q):
        dn = ((n[p] - n[q]) ** 2).sum(-1)
        dz = (z[p] - z[q]) ** 2
        return np.exp(-dn / sigma_normal ** 2) * np.exp(-dz * kz[p])

    # rule 3: the history length, compared as the caller's float32 value
    if variance is None:
        N = np.ones((Hh, Ww))
        short = np.ones((Hh, Ww), bool)
    elif history_len is None:
        N = np.full((Hh, Ww), np.inf)
        short = np.zeros((Hh, Ww), bool)
    else:
        N = np.maximum(np.asarray(history_len, np.float32), np.float32(1.0)).astype(np.float64)
        short = N < float(min_history)
    if _without == "estimate":
        short = np.zeros((Hh, Ww), bool)
    v_in = np.zeros((Hh, Ww)) if variance is None else np.maximum(np.asarray(variance, np.float64), 0.0)
    lum = c @ LUM
    with np.errstate(under="ignore", invalid="ignore"):
        # rule 4: the spatial estimate over the 7x7 window
        s0, s1, s2 = np.zeros((Hh, Ww)), np.zeros((Hh, Ww)), np.zeros((Hh, Ww))
        for _, _, p, q in _taps(Hh, Ww, 3, 1):
            w = w_guide(p, q)
            s0[p] += w
            s1[p] += w * lum[q]
            s2[p] += w * lum[q] ** 2
        mu1, mu2 = s1 / s0, s2 / s0
        boost = 1.0 if _without == "boost" else float(min_history) / N
        v = np.where(short, np.maximum(mu2 - mu1 * mu1, 0.0) * boost, v_in)
        v0 = v.copy()
        for i in range(iterations):
            s = 1 << i
            if _without == "prefilter":
                vbar = v
            else:
                num, den = np.zeros((Hh, Ww)), np.zeros((Hh, Ww))
                for dy, dx, p, q in _taps(Hh, Ww, 1, 1):
                    g = G3[dx + 1] * G3[dy + 1]
                    num[p] += g * v[q]
                    den[p] += g
                vbar = num / den
            if _without == "per_pixel_variance":
                vbar = np.full((Hh, Ww), vbar.mean())
            kl = 1.0 / (sigma_lum * np.sqrt(vbar + 1e-10))
            lum = c @ LUM
            cnum, vnum, den = np.zeros_like(c), np.zeros((Hh, Ww)), np.zeros((Hh, Ww))
            for dy, dx, p, q in _taps(Hh, Ww, 2, s):
                dl = np.abs(lum[p] - lum[q]) * kl[p]
                w = H5[dx + 2] * H5[dy + 2] * np.exp(-dl) * w_guide(p, q)
                cnum[p] += w[..., None] * c[q]
                vnum[p] += (w if _without == "squared" else w * w) * v[q]
                den[p] += w
            c = cnum / den[..., None]
            v = vnum / (den if _without == "squared" else den * den)
    if iterations == 0:
        out = np.array(radiance, copy=True)
    else:
        out = c * a if demodulate else c
    return {"out": out, "variance": v, "v0": v0, "short": short, "estimated": int(short.sum())}
