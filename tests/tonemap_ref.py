"""tpt_tonemap's definition (DESIGN.md section 5 "Tone mapping") in numpy: the luminance and the
binning in float32, which is exact (the post-pass is built without FMA contraction), everything
else in float64.  map_frame takes the dtype, so that the float32 restatement of the map is the same
text."""
import numpy as np

OPS = ("linear", "reinhard", "aces")
TRANSFERS = ("none", "srgb", "gamma")
BAYER4 = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]])
DARK, NAN = -1, 256          # lum_bins' codes beside the bins 0..255

# What a device y may differ by from this file's float64 y: ten times the largest difference
# measured on the MI355X (tests/test_gpu_tonemap.py records the measurements), asserted at most
# 1e-5 there.  The bytes are compared where 255 y + 0.5 + d is farther than DELTA from an integer.
BOUND = 2.5e-6
DELTA = 255.0 * BOUND


def lum32(rad):
    """L = (0.2126 r + 0.7152 g) + 0.0722 b in float32, the device's bits."""
    rad = np.asarray(rad, np.float32)
    with np.errstate(all="ignore"):
        return (np.float32(0.2126) * rad[..., 0] + np.float32(0.7152) * rad[..., 1]) + np.float32(0.0722) * rad[..., 2]


def lum_bins(L):
    """The bin of each float32 luminance: 8 (e + 16) + m3 from the float's bits, 255 from 2^16 up
    (+inf too), DARK below 2^-16 (zero and negatives too), NAN for a NaN."""
    L = np.ascontiguousarray(L, np.float32)
    u = L.view(np.uint32).astype(np.int64)
    b = 8 * (((u >> 23) & 0xFF) - 127 + 16) + ((u >> 20) & 7)
    with np.errstate(invalid="ignore"):
        b = np.where(L >= np.float32(2.0 ** 16), 255, b)
        b = np.where(L >= np.float32(2.0 ** -16), b, DARK)
    return np.where(np.isnan(L), NAN, b)


def histogram(rad):
    """(hist[256] uint64, counted, dark, nonfinite) of a frame [H, W, 3]."""
    b = lum_bins(lum32(rad)).ravel()
    hist = np.bincount(b[(b >= 0) & (b < 256)], minlength=256).astype(np.uint64)
    return hist, int(hist.sum()), int((b == DARK).sum()), int((b == NAN).sum())


def bin_rep(k):
    """The log2 of bin k's centre: (k div 8) - 16 + log2(1 + ((k mod 8) + 0.5) / 8)."""
    k = np.asarray(k)
    return (k // 8) - 16 + np.log2(1.0 + ((k % 8) + 0.5) / 8.0)


def f32(v):
    """A parameter as the library holds it: rounded to float32, then widened."""
    return float(np.float32(v))


def measure(hist, *, key=0.18, p_low=0.10, p_high=0.95, min_ev=-16.0, max_ev=16.0, rate=1.0, ev=0.0, state=None):
    """The measurement in float64.  state: s' or None.  Returns (log2_avg, log2_scale, s); s is None
    where there is still no state (no counted pixel and none before)."""
    h = np.asarray(hist, np.float64)
    N = float(h.sum())
    if N == 0:
        s = state
        return 0.0, (0.0 if s is None else s) + f32(ev), s
    a = np.floor(f32(p_low) * N)
    b = max(np.ceil(f32(p_high) * N), a + 1.0)
    C = np.concatenate([[0.0], np.cumsum(h)[:-1]])
    overlap = np.maximum(0.0, np.minimum(C + h, b) - np.maximum(C, a))
    log2_avg = float((overlap * bin_rep(np.arange(256))).sum() / (b - a))
    target = min(max(np.log2(f32(key)) - log2_avg, f32(min_ev)), f32(max_ev))
    s = target if state is None else state + f32(rate) * (target - state)
    return log2_avg, s + f32(ev), s


def map_frame(rad, scale, op="reinhard", transfer="srgb", white=4.0, gamma=2.2, dtype=np.float64):
    """y [H, W, 3] of the frame at this scale, computed in `dtype`."""
    T = dtype
    white, gamma = T(np.float32(white)), T(np.float32(gamma))
    with np.errstate(all="ignore"):
        x = np.asarray(rad, np.float32).astype(T) * T(scale)
        x = np.minimum(np.maximum(np.where(np.isnan(x), T(0), x), T(0)), T(65504))
        if op == "linear":
            y = np.minimum(x, T(1))
        elif op == "reinhard":
            Lx = (T(0.2126) * x[..., 0] + T(0.7152) * x[..., 1]) + T(0.0722) * x[..., 2]
            Ly = Lx * (T(1) + Lx / (white * white)) / (T(1) + Lx)
            y = np.where(Lx[..., None] == 0, T(0), np.minimum(x * (Ly / Lx)[..., None], T(1)))
        elif op == "aces":
            y = np.clip(x * (T(2.51) * x + T(0.03)) / (x * (T(2.43) * x + T(0.59)) + T(0.14)), T(0), T(1))
        else:
            raise ValueError(op)
        if transfer == "srgb":
            y = np.where(y <= T(0.0031308), T(12.92) * y, T(1.055) * np.power(y, T(1) / T(2.4)) - T(0.055))
        elif transfer == "gamma":
            y = np.power(y, T(1) / gamma)
        elif transfer != "none":
            raise ValueError(transfer)
    return y.astype(T)


def byte_args(y, dither=False):
    """255 y + 0.5 + d per channel sample, [H, W, 3] float64 (row 0 = bottom, as y)."""
    y = np.asarray(y, np.float64)
    H, W = y.shape[:2]
    d = np.zeros((H, W))
    if dither:
        d = (BAYER4[np.arange(H)[:, None] & 3, np.arange(W)[None, :] & 3] + 0.5) / 16.0 - 0.5
    return 255.0 * y + 0.5 + d[..., None]


def to_bytes(args):
    """floor(clamp(args, 0, 255)) as the bytes of a framebuffer's B, G, R: [H, W, 3], row 0 = top."""
    b = np.floor(np.clip(args, 0.0, 255.0)).astype(np.uint8)
    return b[::-1, :, ::-1]


def near_boundary(args, delta=DELTA):
    """Which channel samples lie within delta of a rounding boundary, in to_bytes' layout.  The
    boundaries are the integers 1..255: below 1 every argument gives 0, from 255 up 255."""
    a = np.asarray(args, np.float64)
    k = np.round(a)
    near = (np.abs(a - k) <= delta) & (k >= 1) & (k <= 255)
    return near[::-1, :, ::-1]
