"""Adversarial environment maps and the shared pieces of their tests
(tests/test_env_maps_cpu.py, tests/test_gpu_env_maps.py).

Every other test map is tinypathtracer_amd.procedural_sky: power-of-two sides,
smooth, nowhere black.  The maps here have what the env lookup and the env sampler
(TPT_FLAG_ENV_IS; trace_dev.hpp env_is_sample, lower_bound_guided; api_scene.cpp
build_env_is, build_guide) branch on: sides that are no power of two, flat CDF runs,
zero rows and columns, one texel holding nearly all the weight, partial blocks, one
row, one column, one texel, no light at all.  Generated from a seeded numpy RNG in
image order (row 0 = top), RGBA8; none is committed.

Also here, restated in Python from the sampler's tables (oracle.env_is_tables): the
host's guide tables, the guided search and the plain search, and float64 versions
of Vec2UV (env_light.cuh:72-78) and getNewDirection (path_tracer.cu:187-225).
"""
import functools

import numpy as np

from oracle import oracle as O
from tests.conftest import scene_path

NAMES = ["odd", "sun", "dimsun", "halfblack", "blocks", "poles", "one", "column", "row", "black"]
LIT = [n for n in NAMES if n != "black"]
NORMALS = ([0.0, 1.0, 0.0], [0.6, 0.0, 0.8], [0.0, -1.0, 0.0])
UMIN = np.float32(2.3283064e-10 / 2.0)   # the smallest curand_uniform (x = 0): 2^-33
FRAME = dict(scene="box", W=20, H=12, spp=2, depth=8, seed=42)


def _noise(rng, h, w):
    img = np.zeros((h, w, 4), np.uint8)
    img[..., :3] = rng.integers(1, 256, (h, w, 3), dtype=np.uint8)   # nowhere black by accident
    img[..., 3] = 255
    return img


@functools.lru_cache(maxsize=None)
def env_map(name):
    """The map `name`, image order (row 0 = top), RGBA8, read-only."""
    rng = np.random.default_rng(1000 + NAMES.index(name))
    if name == "odd":            # 19 x 37: no power of two, B = 1
        img = _noise(rng, 19, 37)
    elif name == "sun":          # black but one small bright patch: flat CDFs, zero rows first
        img = np.zeros((48, 96, 4), np.uint8)
        img[9:12, 70:73, :3] = (255, 240, 200)
    elif name == "dimsun":       # tiny weights next to a huge one
        img = np.ones((48, 96, 4), np.uint8)
        img[14, 61, :3] = 255
    elif name == "halfblack":    # bottom half and columns 10..39 black: lo == 0, flat runs inside a row
        img = _noise(rng, 32, 64)
        img[16:, :, :3] = 0
        img[:, 10:40, :3] = 0
    elif name == "blocks":       # 259 x 515: B = 2, partial blocks on both edges
        img = _noise(rng, 259, 515)
    elif name == "poles":        # only the top and bottom rows lit: sin(theta) smallest, pdf largest
        img = np.zeros((32, 64, 4), np.uint8)
        img[0, :, :3] = rng.integers(128, 256, (64, 3), dtype=np.uint8)
        img[31, :, :3] = rng.integers(128, 256, (64, 3), dtype=np.uint8)
    elif name == "one":
        img = np.zeros((1, 1, 4), np.uint8)
        img[0, 0, :3] = (200, 150, 100)
    elif name == "column":
        img = _noise(rng, 64, 1)
    elif name == "row":
        img = _noise(rng, 1, 64)
    elif name == "black":
        img = np.zeros((8, 16, 4), np.uint8)
    else:
        raise KeyError(name)
    img[..., 3] = 255
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def bottom_up(name):
    """The map as the env texture stores it (row 0 = bottom), for the oracle."""
    a = np.ascontiguousarray(env_map(name)[::-1])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def tables(name):
    return O.env_is_tables(bottom_up(name))


# ---------------------------------------------------------------------------
# the two searches, restated (vectorised over x; float32 arithmetic throughout)
# ---------------------------------------------------------------------------
def pow2_at_least(n):
    k = 1
    while k < n and k < (1 << 20):
        k <<= 1
    return k


def guide_sizes(t):
    """(kr, kc) as tpt_env_create chooses them."""
    return pow2_at_least(t["bh"]), pow2_at_least(max(1, t["bw"] // 4))


def build_guide(a, total, K):
    """api_scene.cpp build_guide, statement for statement, in float32."""
    a = np.asarray(a, np.float32)
    n = len(a)
    inv = np.float32(1.0) / np.float32(K)
    g = np.zeros(K + 1, np.int32)
    i = 0
    for k in range(K + 1):
        thr = np.float32(np.float32(np.float32(k) * inv) * np.float32(total))
        while i < n - 1 and a[i] < thr:
            i += 1
        g[k] = i
    return g


def plain_search(a, total, x):
    """The oracle's lower_bound_f of t = x * total: first i with a[i] >= t, n - 1 if none."""
    a = np.asarray(a, np.float32)
    n = len(a)
    t = (np.asarray(x, np.float32) * np.float32(total)).astype(np.float32)
    lo = np.zeros(len(t), np.int64)
    hi = np.full(len(t), n - 1, np.int64)
    while True:
        m = lo < hi
        if not m.any():
            return lo
        mid = (lo + hi) >> 1
        ge = a[mid] >= t
        hi = np.where(m & ge, mid, hi)
        lo = np.where(m & ~ge, mid + 1, lo)


def guided_search(a, total, g, K, x):
    """trace_dev.hpp lower_bound_guided."""
    a = np.asarray(a, np.float32)
    n = len(a)
    x = np.asarray(x, np.float32)
    t = (x * np.float32(total)).astype(np.float32)
    k = np.clip((x * np.float32(K)).astype(np.float32).astype(np.int64), 0, K)   # (int) truncates
    lo = g[k].astype(np.int64)
    hi = np.where(k < K, g[np.minimum(k + 1, K)], n - 1).astype(np.int64)
    hi = np.minimum(hi, n - 1)
    while True:
        m = hi - lo > 8
        if not m.any():
            break
        mid = (lo + hi) >> 1
        ge = a[np.clip(mid, 0, n - 1)] >= t
        hi = np.where(m & ge, mid, hi)
        lo = np.where(m & ~ge, mid + 1, lo)
    cnt = np.zeros(len(t), np.int64)
    for j in range(8):
        i = lo + j
        v = np.where(i < hi, a[np.clip(i, 0, n - 1)], t)
        cnt += v < t
    return lo + cnt


def cdf_ratios(a, total):
    """Each CDF entry over the total as float32, and its two neighbouring floats, kept in
    (0, 1]: the uniforms whose t = x * total lands on, just below or just above an entry."""
    r = (np.asarray(a, np.float32) / np.float32(total)).astype(np.float32)
    x = np.concatenate([r, np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))])
    x = x[np.isfinite(x) & (x > 0.0) & (x <= 1.0)]
    return np.unique(x.astype(np.float32))


def search_inputs(a, total, dense):
    grid = ((np.arange(dense, dtype=np.float64) + 0.5) / dense).astype(np.float32)
    return np.unique(np.concatenate([np.array([1.0, UMIN, 0.5], np.float32), grid, cdf_ratios(a, total)]))


def chosen_blocks(name, x1, x2):
    """(by, bx) of the sampler for uniforms (x1, x2), by the plain search."""
    t = tables(name)
    by = plain_search(t["marg"], t["total"], x1)
    bx = np.zeros(len(by), np.int64)
    x2 = np.asarray(x2, np.float32)
    for r in np.unique(by):
        m = by == r
        bx[m] = plain_search(t["cond"][r], t["row"][r], x2[m])
    return by, bx


def env_is_cases(name, n_random=20000, seed=5):
    """The env sampler's known-answer cases (nf3, x1, x2) on a map: per normal, the corners
    {1, UMIN, 0.5}^2, every marginal CDF ratio (x2 = 0.5), every row's conditional CDF ratios
    with an x1 inside that row's marginal step, and n_random seeded curand uniforms."""
    t = tables(name)
    marg, total = t["marg"], t["total"]
    c = np.array([1.0, UMIN, 0.5], np.float32)
    pairs = [np.stack(np.meshgrid(c, c, indexing="ij"), -1).reshape(-1, 2)]
    r1 = cdf_ratios(marg, total)
    pairs.append(np.stack([r1, np.full(len(r1), 0.5, np.float32)], -1))
    lo = np.concatenate([[np.float32(0.0)], marg[:-1]]).astype(np.float64)
    for by in range(t["bh"]):
        if not t["row"][by] > 0.0:
            continue
        xm = np.float32((lo[by] + float(marg[by])) * 0.5 / float(total))   # inside row by's step
        r2 = cdf_ratios(t["cond"][by], t["row"][by])
        pairs.append(np.stack([np.full(len(r2), xm, np.float32), r2], -1))
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2**32, (n_random, 2), dtype=np.uint64).astype(np.uint32)
    pairs.append((bits.astype(np.float32) * np.float32(2.3283064e-10) + UMIN).astype(np.float32))
    xs = np.concatenate(pairs).astype(np.float32)
    out = []
    for nf in NORMALS:
        out.append(np.concatenate([np.tile(np.asarray(nf, np.float32), (len(xs), 1)), xs], 1))
    return np.ascontiguousarray(np.concatenate(out), np.float32)


# ---------------------------------------------------------------------------
# float64 restatements
# ---------------------------------------------------------------------------
def uv64(d):
    """Vec2UV (env_light.cuh:72-78) in float64: (u, v) of directions [n,3]."""
    d = np.asarray(d, np.float64)
    u = np.arctan2(d[:, 2], d[:, 0]) / (2.0 * np.pi)
    u = np.where(u < 0.0, u + 1.0, u)
    v = 1.0 - np.arccos(np.clip(d[:, 1], -1.0, 1.0)) / np.pi
    return u, v


def texel64(d, w, h, eps=1e-4):
    """The float64 texel of each direction and whether u*w or v*h lies within eps of an
    integer (where the fp32 lookup may legitimately land next door)."""
    u, v = uv64(d)
    fx, fy = u * w, v * h
    ix = np.clip(np.floor(fx), 0, w - 1).astype(np.int64)
    iy = np.clip(np.floor(fy), 0, h - 1).astype(np.int64)
    near = (np.abs(fx - np.rint(fx)) < eps) | (np.abs(fy - np.rint(fy)) < eps)
    return ix, iy, near


LOOKUP_SIZES = [(2048, 1024), (1000, 500), (37, 19), (515, 259), (1, 1), (1, 64), (64, 1)]
LOOKUP_RANDOM = 100_000


def lookup_map(w, h):
    rng = np.random.default_rng(7000 + 3 * w + h)
    return _noise(rng, h, w)   # image order


def lookup_dirs(w, h):
    """trig_inputs.dirs and edge_dirs for the size, (0,0,0), and every sign of zero with an axis."""
    from tests import trig_inputs as TI
    special = [(0.0, 0.0, 0.0)]
    for ax in range(3):
        for s in (1.0, -1.0):
            for z1 in (0.0, -0.0):
                for z2 in (0.0, -0.0):
                    v = [z1, z2]
                    v.insert(ax, s)
                    special.append(tuple(v))
    return np.ascontiguousarray(np.concatenate([TI.dirs(LOOKUP_RANDOM, 7 + w), TI.edge_dirs(w, h, 11 + h),
                                                np.array(special, np.float32)]), np.float32)


# ---------------------------------------------------------------------------
# getNewDirection cases and its float64 restatement
# ---------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def new_direction_cases(seed=9, n_random=10000):
    """(d3, n3, eta, metallic) rows: random unit d and n over the etas; incidences whose
    sin2t is exactly 1.0 and one float either side (the TIR boundary); d.n exactly 0 and
    just above; n.z in {0, -0, denormal}; metal with a dielectric eta; eta <= 0 with
    metallic <= 0 (diffuse)."""
    rng = np.random.default_rng(seed)
    etas = np.array([1.0, 1.5, 1.0 / 1.5, 0.99], np.float32)
    rows = []
    d, n = _unit(rng, n_random), _unit(rng, n_random)
    for k, (eta, met) in enumerate([(e, 0.0) for e in etas] + [(0.0, 0.0), (-1.0, 0.0), (0.0, -0.5), (0.0, 1.0),
                                                               (1.5, 1.0), (0.0, 0.3)]):
        sl = slice(k, None, 10)
        rows.append(np.concatenate([d[sl], n[sl], np.full((len(d[sl]), 1), eta, np.float32),
                                    np.full((len(d[sl]), 1), met, np.float32)], 1))
    # TIR boundary: n = +y, d = (s, c, 0) leaving the dense side (cos_i > 0 -> eta = eta_m), with
    # cos_i scanned over neighbouring floats around the critical angle; the rows whose float32
    # sin2t (the kernel's own operation order) is exactly 1.0, and one step either side, are kept
    edge = []
    for eta in (np.float32(1.5), np.float32(1.0) / np.float32(0.99), np.float32(1.25)):
        cc = np.float32(np.sqrt(1.0 - 1.0 / float(eta) ** 2))
        cs = [cc]
        lo = hi = cc
        for _ in range(4096):
            lo = np.nextafter(lo, np.float32(0.0))
            hi = np.nextafter(hi, np.float32(1.0))
            cs += [lo, hi]
        c = np.sort(np.array(cs, np.float32))
        sin2t = sin2t_f32(c, eta)
        one = np.flatnonzero(sin2t == np.float32(1.0))
        keep = set()
        for i in one:
            keep.update([i - 1, i, i + 1])
        for i in sorted(k for k in keep if 0 <= k < len(c)):
            s = np.float32(np.sqrt(max(0.0, 1.0 - float(c[i]) ** 2)))
            edge.append([s, c[i], 0.0, 0.0, 1.0, 0.0, eta, 0.0])
            edge.append([0.0, c[i], s, 0.0, 1.0, 0.0, eta, 1.0])   # the same with metallic > 0: still dielectric
    rows.append(np.array(edge, np.float32))
    special = []
    den = np.float32(1e-42)
    for eta, met in [(1.5, 0.0), (1.0 / 1.5, 0.0), (0.0, 0.0), (0.0, 1.0)]:
        special.append([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, eta, met])             # d.n exactly 0
        special.append([0.6, 0.0, 0.8, 0.0, 0.0, 1.0, eta, met])             # d.n > 0: leaving
        special.append([0.6, 1e-8, 0.8, 0.0, 1.0, 0.0, eta, met])            # d.n just above 0
        for nz in (0.0, -0.0, den, -den):
            special.append([0.0, -1.0, 0.0, 0.6, 0.8, nz, eta, met])         # n.z zero / denormal
            special.append([0.0, -0.6, 0.8, 1.0, 0.0, nz, eta, met])
    rows.append(np.array(special, np.float32))
    return np.ascontiguousarray(np.concatenate(rows), np.float32)


def sin2t_f32(cos_i, eta):
    """refract's sin2t in the kernel's float32 operation order (eta * eta * (1 - c * c))."""
    c = np.asarray(cos_i, np.float32)
    eta = np.float32(eta)
    sin2i = (np.float32(1.0) - (c * c).astype(np.float32)).astype(np.float32)
    return ((eta * eta).astype(np.float32) * sin2i).astype(np.float32)


def uniforms_of(states, n_draws):
    """The next n_draws curand uniforms of each state (6 words), without advancing them."""
    st = np.array(states, np.uint32).reshape(-1, 6).copy()
    out = np.zeros((len(st), n_draws), np.float32)
    with np.errstate(over="ignore"):
        for k in range(n_draws):
            t = st[:, 0] ^ (st[:, 0] >> np.uint32(2))
            st[:, 0:4] = st[:, 1:5].copy()
            st[:, 4] = (st[:, 4] ^ (st[:, 4] << np.uint32(4))) ^ (t ^ (t << np.uint32(1)))
            st[:, 5] = st[:, 5] + np.uint32(362437)
            x = st[:, 4] + st[:, 5]
            out[:, k] = x.astype(np.float32) * np.float32(2.3283064e-10) + UMIN
    return out, st


def new_direction64(cases, u):
    """getNewDirection (path_tracer.cu:187-225: refract :143-163, shlickFresnel :165-173,
    HemisphereCosine sampler.h:75-96) in float64 on the float32 inputs, fed the uniforms u
    [n,2] the device draws.  Returns next [n,3], atten, pdf, draws consumed, and `edge`:
    the cases within 1e-6 of the TIR test or of the coin flip, where a float32 evaluation
    may legitimately take the other branch."""
    c = np.asarray(cases, np.float64)
    d, n, eta_m, met = c[:, 0:3], c[:, 3:6], c[:, 6], c[:, 7]
    u = np.asarray(u, np.float64)
    N = len(c)
    nxt = np.zeros((N, 3))
    att = np.ones(N)
    pdf = np.ones(N)
    draws = np.zeros(N, np.int64)
    edge = np.zeros(N, bool)
    dn = (d * n).sum(1)
    refl = d - 2.0 * dn[:, None] * n
    diel = eta_m > 0.0
    metal = ~diel & (met > 0.0)
    diff = ~diel & ~metal
    # dielectric
    with np.errstate(divide="ignore", invalid="ignore"):
        eta = np.where(dn > 0.0, eta_m, 1.0 / eta_m)
        nn = np.where((dn > 0.0)[:, None], -n, n)
        ci = np.abs(dn)
        sin2t = eta * eta * (1.0 - ci * ci)
        tir = sin2t >= 1.0
        ct = np.sqrt(np.maximum(0.0, 1.0 - sin2t))
        refr = eta[:, None] * d + (ci * eta - ct)[:, None] * nn
        f0 = ((1.0 - eta) / (1.0 + eta)) ** 2
        m = np.clip(1.0 - ci, 0.0, 1.0)
        fr = np.where(tir, 1.0, f0 + (1.0 - f0) * m ** 5)
    pick_refl = u[:, 0] < fr
    nxt[diel] = np.where(pick_refl[:, None], refl, refr)[diel]
    draws[diel] = 1
    edge |= diel & ((np.abs(sin2t - 1.0) < 1e-6) | (np.abs(u[:, 0] - fr) < 1e-6))
    nxt[metal] = refl[metal]
    # diffuse: cosine hemisphere about the incident-side normal
    sign = np.where(dn > 0.0, -1.0, 1.0)
    nf = sign[:, None] * n
    with np.errstate(divide="ignore", invalid="ignore"):
        xb = np.where((nf[:, 2] == 0.0)[:, None], np.array([0.0, 0.0, 1.0]),
                      np.stack([np.ones(N), np.zeros(N), -nf[:, 0] / nf[:, 2]], -1))
        xb = xb / np.linalg.norm(xb, axis=1, keepdims=True)
    zb = np.cross(xb, nf)
    phi = 2.0 * np.pi * u[:, 0]
    cos_t = np.sqrt(u[:, 1])
    sin_t = np.sqrt(np.maximum(0.0, 1.0 - cos_t * cos_t))
    hd = (np.cos(phi) * sin_t)[:, None] * xb + cos_t[:, None] * nf + (np.sin(phi) * sin_t)[:, None] * zb
    cc = (hd * nf).sum(1)
    nxt[diff] = hd[diff]
    att[diff] = (np.abs(cc) / np.pi)[diff]
    pdf[diff] = np.where(cc > 0.0, cc / np.pi, 0.0)[diff]
    draws[diff] = 2
    return nxt, att, pdf, draws, edge


# ---------------------------------------------------------------------------
# the oracle's frames, rendered once
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene(scene):
    return O.load_scene(scene_path(scene))


@functools.lru_cache(maxsize=None)
def oracle_frame(name, env_is, scene=FRAME["scene"]):
    """The oracle's frame (radiance, bgra, counters) of `scene` under map `name` (None: no
    env) at the test size, trig_mode 1."""
    env = None if name is None else bottom_up(name)
    return O.render(_scene(scene), FRAME["W"], FRAME["H"], FRAME["spp"], FRAME["depth"], FRAME["seed"], env=env,
                    trig_mode=1, env_is=env_is)


def differing_share(a, b):
    return float((np.ascontiguousarray(a, np.float32).view(np.uint32) !=
                  np.ascontiguousarray(b, np.float32).view(np.uint32)).any(-1).mean())


# ---------------------------------------------------------------------------
# float64 sanity figures of known-answer outputs: measured on the oracle, asserted
# on the oracle (tests/test_env_maps_cpu.py) and on the device
# (tests/test_gpu_env_maps.py) with a 4x margin
# ---------------------------------------------------------------------------
# | |dir| - 1 | of an accepted env sample: measured <= 1.01e-7 on every map (0.85 ulp of 1)
DIR_NORM_TOL = 4.0e-7
# how far float64 Vec2UV of an accepted sample's dir lies outside the chosen block, in
# texels: measured <= 8.1e-5 (blocks, 515 texels wide; <= 7e-6 on the other maps)
BLOCK_SLACK = 3.2e-4
# getNewDirection against its float64 restatement, absolute, on next / atten / pdf:
# measured 1.63e-6 (a refraction near the critical angle, where cos_t = sqrt(1 - sin2t) is
# ill-conditioned); 0.43 % of the cases are left out (the TIR-boundary rows by construction)
NEW_DIRECTION_TOL = 6.5e-6
NEW_DIRECTION_MAX_EXCLUDED = 0.01


def oracle_states(n, seed=42):
    """The RNG states of pixels 0..n-1 after setupRandSeed (tpt_debug_rng_init's on the device)."""
    st = np.zeros((n, 6), np.uint32)
    one = (O.C.c_uint32 * 6)()
    for i in range(n):
        O.lib().orc_xorwow_init(seed, i, one)
        st[i] = one[:]
    return st


def env_is_sanity(name, cases, ok, d):
    """Of the accepted samples: the largest | |dir| - 1 |, and the farthest that float64
    Vec2UV of dir lies outside the block the two searches chose, in texels."""
    t = tables(name)
    h, w = env_map(name).shape[:2]
    m = np.asarray(ok).astype(bool)
    by, bx = chosen_blocks(name, cases[m, 3], cases[m, 4])
    dd = np.asarray(d, np.float64)[m]
    norm_err = float(np.abs(np.linalg.norm(dd, axis=1) - 1.0).max())
    u, v = uv64(dd)
    b = t["b"]
    x0, y0 = bx * b, by * b
    x1, y1 = np.minimum(x0 + b, w), np.minimum(y0 + b, h)
    fx, fy = u * w, v * h
    outx = np.maximum(np.maximum(x0 - fx, fx - x1), 0.0)
    outx = np.minimum(outx, np.maximum(np.maximum(x0 - (fx - w), (fx - w) - x1), 0.0))   # u wraps at 0 / 1
    outx = np.minimum(outx, np.maximum(np.maximum(x0 - (fx + w), (fx + w) - x1), 0.0))
    outy = np.maximum(np.maximum(y0 - fy, fy - y1), 0.0)
    return norm_err, float(max(outx.max(), outy.max())), int(m.sum())


def new_direction_error(cases, states, out, states_after):
    """Against new_direction64 fed the same uniforms: the largest absolute error of next,
    atten and pdf over the compared cases, the share left out (within 1e-6 of the TIR test
    or the coin flip, or not finite in float32: n.x / n.z overflows for a denormal n.z), and
    whether every case consumed the restatement's number of uniforms."""
    u, _ = uniforms_of(states, 2)
    nxt, att, pdf, draws, edge = new_direction64(cases, u)
    consumed = np.full(len(cases), -1)
    for k in range(3):
        _, st_k = uniforms_of(states, k)
        consumed[(st_k == np.asarray(states_after, np.uint32)).all(1)] = k
    finite = np.isfinite(out).all(1)
    keep = ~edge & finite
    ref = np.concatenate([nxt, att[:, None], pdf[:, None]], 1)
    err = float(np.abs(np.asarray(out, np.float64)[keep] - ref[keep]).max())
    return err, float(1.0 - keep.mean()), bool((consumed == draws).all())
