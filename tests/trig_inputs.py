"""Input sets of the parity-trig tests, shared by the host compile's checks
(tests/test_cpu_math.py) and the device's (tests/test_gpu_env_maps.py): the same
values go through g++'s and the device compiler's build of ptrig.hpp."""
import numpy as np


def phis(n, seed=1):
    """phi = 2*pi*u over n curand uniforms, and the quadrant edges."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    u = (x.astype(np.float32) * np.float32(2.3283064e-10) + np.float32(2.3283064e-10 / 2.0)).astype(np.float32)
    phi = (np.float32(2.0 * np.float32(3.141592653589793)) * u).astype(np.float32)
    edge = np.array([0.0, 1.4629181e-09, 6.2831855, 1.5707964, 3.1415927, 4.712389, 0.7853982], np.float32)
    return np.concatenate([phi, edge])


def ulps(a, b):
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def atan2_acos_vectors(n=200_000, seed=3):
    """Unit vectors with zeros of both signs on the axes (the atan2 / acos set)."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3)).astype(np.float32)
    v /= np.linalg.norm(v, axis=1, keepdims=True).astype(np.float32)
    v[::7, 0] = 0.0
    v[::11, 2] = -0.0
    return v


def dirs(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3)).astype(np.float32)
    v /= np.linalg.norm(v, axis=1, keepdims=True).astype(np.float32)
    v[::13, 0] = 0.0
    v[::17, 2] = -0.0
    v[::19, 1] = 1.0
    v[::23, 1] = -1.0
    return v


def plain(n):
    """The rows of dirs(n, .) that were not put on an axis."""
    i = np.arange(n)
    return (i % 13 != 0) & (i % 17 != 0) & (i % 19 != 0) & (i % 23 != 0)


def edge_dirs(w, h, seed):
    """Directions whose (u, v) sit on texel edges (and 1 ulp either side)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(0, w + 1, max(1, w // 256)):
        phi = 2.0 * np.pi * k / w
        th = rng.uniform(0.05, np.pi - 0.05)
        out.append((np.sin(th) * np.cos(phi), np.cos(th), np.sin(th) * np.sin(phi)))
    for k in range(0, h + 1, max(1, h // 256)):
        th = np.pi * (1.0 - k / h)
        phi = rng.uniform(0, 2 * np.pi)
        out.append((np.sin(th) * np.cos(phi), np.cos(th), np.sin(th) * np.sin(phi)))
    v = np.array(out, np.float32)
    nb = [v]
    for d in (-1, 1, -2, 2):   # neighbouring floats of every component
        nb.append(np.nextafter(v, np.float32(d * np.inf)).astype(np.float32))
    return np.concatenate(nb)
