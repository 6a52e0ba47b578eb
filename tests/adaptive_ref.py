"""The reference of tpt_render_adaptive (tpt.h; DESIGN.md section 5 "Adaptive sampling"):
the schedule and the error estimate in float64 on oracle renders.

A pixel's first n samples are the n-spp render (the per-pixel streams are indexed by
the global pixel and a progressive render is bit-identical to one call), so the oracle
frames at n / 2 and n samples are exactly what the device's estimate at n reads: I =
the n-spp radiance, A = the n / 2-spp radiance,
    e = (|I.r - A.r| + |I.g - A.g| + |I.b - A.b|) / sqrt(max(I.r + I.g + I.b, 1e-4)),
and a tile's error E is the mean of e over its in-frame pixels.  Tiles are 16 x 16
pixels, row 0 at the bottom like the radiance.

CASES are the frames tests/test_adaptive_cpu.py proves the premises on and
tests/test_gpu_adaptive.py renders: min_spp 2 and max_spp 32 throughout, the targets
read off the oracle's tables of estimates (test_adaptive_cpu prints them).
"""
import numpy as np

from oracle import oracle as O
from tests import lit_scenes as L
from tests import variant_scenes as V

TILE = 16
MIN_SPP, MAX_SPP, DEPTH = 2, 32, 8
FLAG_REF_ORDER, FLAG_ENV_IS = 0x2, 0x8

# name -> (scene builder, width, height, "sky" or None, device flags, target, seed).  Each target gives
# the minimum, an intermediate level and max_spp with an unconverged tile, well away from every
# estimate (test_adaptive_cpu); box_17x16 has two tiles, so two levels, and box_35x16 is that row
# with a third tile, ending at three levels (33 wide still shows two, at six seeds).  box_131x9 at seed 42 has no
# such target (its noisy tiles all run to 32 spp at any target that stops the others), seed 16 has.
CASES = {
    "box_37x29": (lambda: V.scene("box"), 37, 29, None, 0, 0.23, 42),        # 3 x 2 tiles, partial both ways
    "tir_37x29": (lambda: V.scene("tir"), 37, 29, None, 0, 0.29, 42),
    "box_131x9": (lambda: V.scene("box"), 131, 9, None, 0, 0.06, 16),        # one partial row of nine tiles
    "box_17x16": (lambda: V.scene("box"), 17, 16, None, 0, 0.2, 42),         # a whole tile and a one-pixel column
    "box_35x16": (lambda: V.scene("box"), 35, 16, None, 0, 0.263, 42),       # the same row with a third tile: three levels
    "box_l3_37x29": (lambda: L.scene("box_l3"), 37, 29, None, 0, 0.18, 42),  # delta lights: pair mode
    "box_l3_sky_is": (lambda: L.scene("box_l3_sky"), 37, 29, "sky", FLAG_ENV_IS, 0.18, 42),
    "box_ref_order": (lambda: V.scene("box"), 37, 29, None, FLAG_REF_ORDER, 0.23, 42),
}
MIN_LEVELS = {name: 2 if name == "box_17x16" else 3 for name in CASES}   # distinct stop levels a case shows
LIT_CASE = "box_l3_37x29"


def tiles_of(W, H):
    return (W + TILE - 1) // TILE, (H + TILE - 1) // TILE


def spp_levels(min_spp=MIN_SPP, max_spp=MAX_SPP):
    """The sample counts a schedule reads a frame at: min_spp / 2, min_spp, 2 min_spp, ..., max_spp."""
    out, n = [min_spp // 2], min_spp
    while n <= max_spp:
        out.append(n)
        n *= 2
    return out


_frames = {}


def oracle_levels(name):
    """spp -> the oracle's radiance of CASES[name] at that many samples, for every level of the
    schedule; rendered once per process, read-only."""
    if name not in _frames:
        build, W, H, env, flags, _, seed = CASES[name]
        ps = V.oracle_scene(build())
        sky = V.sky()[::-1].copy() if env else None
        frames = {}
        for n in spp_levels():
            rad, _, _ = O.render(ps, W, H, n, DEPTH, seed, env=sky, trig_mode=1, env_is=bool(flags & FLAG_ENV_IS))
            rad.setflags(write=False)
            frames[n] = rad
        _frames[name] = frames
    return _frames[name]


def tile_errors(rad_n, rad_half):
    """E per tile (float64, [tiles_y, tiles_x]) from the n-spp and the n / 2-spp radiance."""
    I = np.asarray(rad_n, np.float64)
    A = np.asarray(rad_half, np.float64)
    with np.errstate(invalid="ignore"):   # (a non-finite pixel: inf - inf = NaN, as on the device)
        e = np.abs(I - A).sum(-1) / np.sqrt(np.maximum(I.sum(-1), 1e-4))
    H, W = e.shape
    tx, ty = tiles_of(W, H)
    out = np.zeros((ty, tx))
    for j in range(ty):
        for i in range(tx):
            out[j, i] = e[j * TILE:(j + 1) * TILE, i * TILE:(i + 1) * TILE].mean()
    return out


def schedule(levels, target, min_spp=MIN_SPP, max_spp=MAX_SPP):
    """The schedule on frames `levels` (spp -> radiance).  Returns a dict:
    tile_spp [ty, tx] int32; tile_error [ty, tx] each tile's last estimate; passes (trace
    passes: the two halves of min_spp, then one per doubling); unconverged (tiles not below
    the target at max_spp); samples (sum of in-frame pixels x spp); checkpoints, a list of
    (n, estimates of the tiles active at n)."""
    H, W = levels[min_spp].shape[:2]
    tx, ty = tiles_of(W, H)
    active = np.ones((ty, tx), bool)
    spp = np.zeros((ty, tx), np.int32)
    err = np.zeros((ty, tx))
    n, passes, unconverged, checkpoints = min_spp, 2, 0, []
    while True:
        E = tile_errors(levels[n], levels[n // 2])
        err[active] = E[active]
        checkpoints.append((n, E[active].copy()))
        stop = active & (E < target)          # NaN is below no target
        if n == max_spp:
            unconverged = int((active & ~stop).sum())
            stop = active.copy()
        spp[stop] = n
        active &= ~stop
        if not active.any():
            break
        n *= 2
        passes += 1
    px = np.minimum(TILE, W - TILE * np.arange(tx))[None, :] * np.minimum(TILE, H - TILE * np.arange(ty))[:, None]
    return {"tile_spp": spp, "tile_error": err, "passes": passes, "unconverged": unconverged,
            "samples": int((px * spp).sum()), "checkpoints": checkpoints}


def reference(name, target=None):
    """schedule() of CASES[name] at its own target (or another)."""
    return schedule(oracle_levels(name), CASES[name][5] if target is None else target)


def compose(tile_spp, frames):
    """The frame whose pixels come from frames[spp of their tile] (arrays [H, W, c], row 0 = bottom)."""
    first = next(iter(frames.values()))
    out = np.zeros_like(first)
    H, W = first.shape[:2]
    per_pixel = np.repeat(np.repeat(tile_spp, TILE, 0), TILE, 1)[:H, :W]
    for n, f in frames.items():
        out[per_pixel == n] = f[per_pixel == n]
    return out
