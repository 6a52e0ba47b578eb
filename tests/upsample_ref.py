"""Float64 numpy restatement of tpt_upsample's definition (DESIGN.md section 5 "Guided
upsampling"): the checker of tests/test_gpu_upsample.py and the upsampler of
tools/upsample_quality.py.  The footprint (which low pixels are taps) and the fallback decision
are made in Python integers, as the kernel makes them in 64-bit integers: both are exact, so the
two sides hold the same tap set and count the same fallback pixels."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
ALBEDO_FLOOR = 1e-3


def axis_footprint(lo, full):
    """Per full-size coordinate x of one axis: the two taps' clamped low coordinates [2, full],
    the fraction f = r / 2 full as float64, and whether the second tap counts (r != 0).
    n = (2 x + 1) lo - full, x0 = floor(n / 2 full), r = n - 2 full x0: Python integers."""
    q = np.zeros((2, full), np.int64)
    f = np.zeros(full, np.float64)
    two = np.zeros(full, bool)
    for x in range(full):
        n = (2 * x + 1) * lo - full
        x0 = n // (2 * full)
        r = n - 2 * full * x0
        q[0, x] = min(max(x0, 0), lo - 1)
        q[1, x] = min(max(x0 + 1, 0), lo - 1)
        f[x] = r / (2 * full)
        two[x] = r != 0
    return q, f, two


def upsample_ref(radiance_low, aov_low, aov, sigma_normal, sigma_depth, demodulate, *,
                 use_emin=True, use_material=True, details=None):
    """Returns (frame [H, W, 3] float64, fallback mask [H, W] bool).  use_emin / use_material
    False: the definition with that rule deleted, for the teeth tests only.  details: a dict that
    receives `emin` [H, W] (0 at fallback pixels)."""
    rl = np.asarray(radiance_low, np.float64)
    hl, wl = rl.shape[:2]
    H, W = np.asarray(aov["depth"]).shape
    f64 = lambda a: np.asarray(a, np.float64)
    nl, zl, ml = f64(aov_low["normal"]), f64(aov_low["depth"]), np.asarray(aov_low["material"])
    n_p, z_p, m_p = f64(aov["normal"]), f64(aov["depth"]), np.asarray(aov["material"])
    qx, fx, twox = axis_footprint(wl, W)
    qy, fy, twoy = axis_footprint(hl, H)
    kz = np.minimum(1.0 / (sigma_depth ** 2 * np.maximum(z_p * z_p, 1e-12)), FLT_MAX)
    b, ok, e, cq, craw = [], [], [], [], []
    for k in range(4):                                     # (0,0), (1,0), (0,1), (1,1): the kernel's order
        i, j = k & 1, k >> 1
        yy, xx = qy[j][:, None], qx[i][None, :]
        bx = fx if i else 1.0 - fx
        by = fy if j else 1.0 - fy
        tap = (np.ones(W, bool) if i == 0 else twox)[None, :] & (np.ones(H, bool) if j == 0 else twoy)[:, None]
        bk = np.where(tap, bx[None, :] * by[:, None], 0.0)
        dn = nl[yy, xx] - n_p
        dz = zl[yy, xx] - z_p
        ek = np.minimum((dn * dn).sum(-1) / sigma_normal ** 2 + dz * dz * kz, FLT_MAX)
        okk = tap & (bk > 0.0)
        if use_material:
            okk = okk & (ml[yy, xx] == m_p)
        c = rl[yy, xx]
        craw.append(c)
        if demodulate:
            c = c / np.maximum(f64(aov_low["albedo"])[yy, xx], ALBEDO_FLOOR)
        b.append(bk)
        ok.append(okk)
        e.append(ek)
        cq.append(c)
    any_ok = ok[0] | ok[1] | ok[2] | ok[3]
    emin = np.full((H, W), np.inf)
    for k in range(4):
        emin = np.where(ok[k], np.minimum(emin, e[k]), emin)
    emin = np.where(any_ok, emin, 0.0)
    if details is not None:
        details["emin"] = emin

    def mean_about_first(counts, weights, colours):
        """c_r + sum w (c_q - c_r) / sum w, c_r the first tap that counts"""
        cr = np.zeros((H, W, 3))
        have = np.zeros((H, W), bool)
        for k in range(4):
            first = counts[k] & ~have
            cr = np.where(first[..., None], colours[k], cr)
            have |= counts[k]
        sw = np.zeros((H, W))
        acc = np.zeros((H, W, 3))
        for k in range(4):
            w = np.where(counts[k], weights[k], 0.0)
            sw += w
            acc += w[..., None] * np.where(counts[k][..., None], colours[k] - cr, 0.0)
        return cr + acc / np.where(sw > 0.0, sw, 1.0)[..., None]

    with np.errstate(over="ignore", under="ignore"):
        wts = [b[k] * np.exp(-(e[k] - emin)) if use_emin else b[k] * np.exp(-e[k]) for k in range(4)]
    guided = mean_about_first(ok, wts, cq)
    if not use_emin:   # (the deleted rule's failure: every weight underflows, 0 / 0)
        sw = sum(np.where(ok[k], wts[k], 0.0) for k in range(4))
        guided = np.where((any_ok & (sw == 0.0))[..., None], np.nan, guided)
    if demodulate:
        guided = guided * np.maximum(f64(aov["albedo"]), ALBEDO_FLOOR)
    plain = mean_about_first([bk > 0.0 for bk in b], b, craw)   # never demodulated, never re-modulated
    return np.where(any_ok[..., None], guided, plain), ~any_ok


def bilinear_ref(radiance_low, W, H):
    """Plain bilinear upsampling over the same footprint: the fallback rule at every pixel."""
    hl, wl = np.asarray(radiance_low).shape[:2]
    none = {"normal": np.zeros((hl, wl, 3)), "depth": np.zeros((hl, wl)), "material": np.zeros((hl, wl), np.int32)}
    full = {"normal": np.zeros((H, W, 3)), "depth": np.zeros((H, W)), "material": np.ones((H, W), np.int32)}
    out, fb = upsample_ref(radiance_low, none, full, 1.0, 1.0, False)
    assert fb.all()
    return out
