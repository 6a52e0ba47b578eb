"""Seeded synthetic frames for tpt_tonemap's tests: [H, W, 3] float32, row 0 = bottom.  Each is
computed once per size and handed out read-only."""
import functools

import numpy as np

# 1x1, one wave, a partial row segment, odd sizes, several workgroups with partial ones, and the
# smallest convenient frame above one sweep of the histogram grid (512 workgroups of 256 lanes =
# 131,072 pixels): as a constant frame it also puts more than 65,535 pixels into one bin.
SIZES = ((1, 1), (16, 16), (17, 16), (37, 29), (131, 9), (363, 362))
SWEEP = 512 * 256
NAMES = ("log_uniform", "planted", "constant", "two_bins")
PLANT_KINDS = ("zero", "negative", "nan", "inf", "tiny")


def _frozen(a):
    a.setflags(write=False)
    return a


def _coloured(L, rng):
    """Pixels of luminance about L with a seeded tint: rgb = L t / lum(t)."""
    t = rng.uniform(0.2, 1.0, L.shape + (3,))
    t /= (0.2126 * t[..., 0] + 0.7152 * t[..., 1] + 0.0722 * t[..., 2])[..., None]
    return (L[..., None] * t).astype(np.float32)


@functools.lru_cache(maxsize=None)
def log_uniform(w, h, seed=1, lo=-10.0, hi=6.0):
    """Luminances log-uniform over 2^lo .. 2^hi."""
    rng = np.random.default_rng([seed, w, h])
    return _frozen(_coloured(np.exp2(rng.uniform(lo, hi, (h, w))), rng))


def plant_counts(w, h):
    """How many pixels of each kind `planted` holds: up to 5, fewer in a frame too small for them."""
    return {kind: min(5 - i % 3, (w * h) // 8) for i, kind in enumerate(PLANT_KINDS)}


@functools.lru_cache(maxsize=None)
def planted(w, h, seed=2):
    """log_uniform with zeros, negatives, NaN, +inf and values below 2^-16 at seeded places."""
    rng = np.random.default_rng([seed, w, h])
    f = log_uniform(w, h, seed).copy().reshape(-1, 3)
    counts = plant_counts(w, h)
    where = rng.permutation(w * h)[:sum(counts.values())]
    values = {"zero": (0.0, 0.0, 0.0), "negative": (-1.0, -0.5, -2.0), "nan": (np.nan, 0.5, 0.5),
              "inf": (np.inf, 1.0, 1.0), "tiny": (1e-6, 1e-6, 1e-6)}
    at = 0
    for kind in PLANT_KINDS:
        f[where[at:at + counts[kind]]] = values[kind]
        at += counts[kind]
    return _frozen(f.reshape(h, w, 3))


@functools.lru_cache(maxsize=None)
def constant(w, h, value=(0.31, 0.62, 0.17)):   # (no channel lands on a rounding boundary under any op)
    return _frozen(np.broadcast_to(np.asarray(value, np.float32), (h, w, 3)).copy())


@functools.lru_cache(maxsize=None)
def two_bins(w, h):
    """Grey pixels in a checkerboard of two luminances 12 octaves apart."""
    y, x = np.mgrid[0:h, 0:w]
    L = np.where((x + y) & 1, np.float32(1.3 * 2.0 ** -8), np.float32(1.3 * 2.0 ** 4)).astype(np.float32)
    return _frozen(np.repeat(L[..., None], 3, axis=2))


@functools.lru_cache(maxsize=None)
def black(w, h):
    return _frozen(np.zeros((h, w, 3), np.float32))


def frame(name, w, h):
    return {"log_uniform": log_uniform, "planted": planted, "constant": constant, "two_bins": two_bins}[name](w, h)
