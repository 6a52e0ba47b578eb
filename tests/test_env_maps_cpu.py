"""CPU: the premises of tests/test_gpu_env_maps.py, on the oracle alone.

Each adversarial map of tests/env_maps.py is there to reach one branch of the env
lookup or the env sampler.  These tests show on the CPU that it does -- a guide
bucket wider than 8 entries, partial blocks that are sampled, flat CDF runs, an
empty distribution -- that the host's guide tables give the plain search's index
on such CDFs, that the sampler stays unbiased on them, and that the frames the GPU
tests compare really depend on the map: so the GPU tests cannot pass vacuously.
"""
import numpy as np
import pytest

from tests import env_maps as E
from tests import trig_inputs as TI
from tests.test_env_is import _brute_force
from oracle import oracle as O


def _guides(name):
    t = E.tables(name)
    kr, kc = E.guide_sizes(t)
    gr = E.build_guide(t["marg"], t["total"], kr)
    gc = [E.build_guide(t["cond"][by], t["row"][by], kc) for by in range(t["bh"])]
    return t, kr, kc, gr, gc


@pytest.mark.parametrize("name", ["sun", "dimsun"])
def test_a_guide_bucket_spans_more_than_8_entries(name):
    """lower_bound_guided's `while (hi - lo > 8)` bisection only runs for such a bucket."""
    t, kr, kc, gr, gc = _guides(name)
    widest = max(int(np.diff(g).max()) for by, g in enumerate(gc) if t["row"][by] > 0.0)
    assert widest > 8, widest
    if name == "sun":   # zero rows first: the marginal starts flat, and its guide is wide too
        assert t["marg"][0] == 0.0 and int(np.diff(gr).max()) > 8


def test_blocks_has_partial_blocks_and_samples_them():
    t = E.tables("blocks")
    h, w = E.env_map("blocks").shape[:2]
    assert t["b"] == 2 and w % t["b"] != 0 and h % t["b"] != 0
    assert t["bw"] == (w + 1) // 2 and t["bh"] == (h + 1) // 2
    cases = E.env_is_cases("blocks", n_random=200_000, seed=21)
    cases = cases[: len(cases) // 3]                      # one normal: the blocks do not depend on it
    by, bx = E.chosen_blocks("blocks", cases[:, 3], cases[:, 4])
    assert (bx == t["bw"] - 1).sum() >= 20 and (by == t["bh"] - 1).sum() >= 20
    # the oracle's own directions say the same: accepted samples in the last texel column
    # and the last texel row (the one-texel-wide partial blocks)
    ok, d, _ = O.kat_env_is(E.bottom_up("blocks"), cases)
    u, v = E.uv64(d[ok == 1])
    assert (np.floor(u * w) == w - 1).sum() >= 20 and (np.floor(v * h) == h - 1).sum() >= 20


def test_halfblack_starts_at_zero_and_has_flat_runs():
    t = E.tables("halfblack")
    assert t["marg"][0] == 0.0
    longest = 0
    for row in t["cond"]:
        flat = np.flatnonzero(np.diff(row) != 0.0)
        edges = np.concatenate([[-1], flat, [len(row) - 1]])
        longest = max(longest, int(np.diff(edges).max()))
    assert longest >= 20, longest


def test_black_has_an_empty_distribution():
    assert E.tables("black")["total"] == 0.0
    with pytest.raises(ValueError):
        O.kat_env_is(E.bottom_up("black"), np.array([[0, 1, 0, 0.5, 0.5]], np.float32))


@pytest.mark.parametrize("name", E.LIT)
def test_guided_search_returns_the_plain_search_index(name):
    """api_scene.cpp build_guide's claim, on CDFs that are not sky-shaped: for x = 1.0, the
    smallest curand uniform, a dense grid, and every CDF entry over the total with its
    neighbouring floats."""
    t, kr, kc, gr, gc = _guides(name)
    x = E.search_inputs(t["marg"], t["total"], 1 << 16)
    got = E.guided_search(t["marg"], t["total"], gr, kr, x)
    want = E.plain_search(t["marg"], t["total"], x)
    assert np.array_equal(got, want), x[np.flatnonzero(got != want)[:5]]
    for by in range(t["bh"]):
        if not t["row"][by] > 0.0:
            continue   # never chosen: the marginal step of an empty row is 0
        x = E.search_inputs(t["cond"][by], t["row"][by], 1 << 12)
        got = E.guided_search(t["cond"][by], t["row"][by], gc[by], kc, x)
        want = E.plain_search(t["cond"][by], t["row"][by], x)
        assert np.array_equal(got, want), (by, x[np.flatnonzero(got != want)[:5]])


def _upsampled(env, min_h=256, min_w=512):
    """The same radiance field on a finer grid (every texel repeated), so that the
    brute-force sum's texel-centre quadrature resolves the cosine over a 1 x 1 map too."""
    h, w = env.shape[:2]
    return np.repeat(np.repeat(env, -(-min_h // h), axis=0), -(-min_w // w), axis=1)


# test_env_is.py's tolerances; no map needs more.  Measured at the grid below (the test
# prints every figure): the largest relative error is 2.6 % (the blue channel of `column`
# and `row`: a regular grid puts 8 +- 1 points into each of their 64 cells, and blue weighs
# least in the luma that the pdf follows), 0.6 % on every other map.
UNBIASED_RTOL, UNBIASED_ATOL = 0.03, 2e-3
GRID = 512


@pytest.mark.parametrize("name", E.LIT)
def test_env_is_unbiased_on_adversarial_maps(name):
    """The mean of k_le over a stratified GRID x GRID set of (x1, x2) is test_env_is.py's
    brute-force texel sum (of the map upsampled to at least 256 x 512: the same radiance)."""
    env = E.bottom_up(name)
    c = ((np.arange(GRID, dtype=np.float64) + 0.5) / GRID).astype(np.float32)
    xs = np.stack(np.meshgrid(c, c, indexing="ij"), -1).reshape(-1, 2)
    for nf in E.NORMALS:
        cases = np.concatenate([np.tile(np.asarray(nf, np.float32), (len(xs), 1)), xs], 1)
        _, _, k = O.kat_env_is(env, cases)
        est = k.astype(np.float64).mean(0)
        ref = _brute_force(_upsampled(env), nf)
        print(name, nf, est, ref, np.abs(est - ref).max())
        assert np.allclose(est, ref, rtol=UNBIASED_RTOL, atol=UNBIASED_ATOL), (name, nf, est, ref)


@pytest.mark.parametrize("name", E.LIT)
def test_is_frame_depends_on_the_map(name):
    """Teeth of the bit-for-bit frame tests: importance sampling changes >= 10 % of the pixels."""
    share = E.differing_share(E.oracle_frame(name, True)[0], E.oracle_frame(name, False)[0])
    print(name, "IS vs no IS", share)
    assert share >= 0.10, share


@pytest.mark.parametrize("name", [n for n in E.LIT if n not in ("sun", "poles")])
def test_lookup_frame_depends_on_the_map(name):
    """... and so does the miss lookup alone (sun and poles are too dark to show at this
    size: their lookup is covered by the known-answer test)."""
    share = E.differing_share(E.oracle_frame(name, False)[0], E.oracle_frame(None, False)[0])
    print(name, "env vs none", share)
    assert share >= 0.10, share


def test_black_frames_are_the_envless_frame():
    """IS is off on an all-black map (total == 0), and a black miss adds nothing."""
    base = E.oracle_frame(None, False)
    for env_is in (False, True):
        f = E.oracle_frame("black", env_is)
        assert E.differing_share(f[0], base[0]) == 0.0
        assert f[2]["traversals"] == base[2]["traversals"]


@pytest.mark.parametrize("w,h", E.LOOKUP_SIZES)
def test_oracle_lookup_is_the_float64_texel(w, h):
    """The oracle's texel of the plain random directions is float64 Vec2UV's, except where
    u*w or v*h lies within 1e-4 of an integer; at most 1 % are excluded."""
    env = np.ascontiguousarray(E.lookup_map(w, h)[::-1])
    d = E.lookup_dirs(w, h)[: E.LOOKUP_RANDOM][TI.plain(E.LOOKUP_RANDOM)]
    _, ixy = O.kat_env_lookup(env, d)
    ix, iy, near = E.texel64(d, w, h)
    assert near.mean() <= 0.01, near.mean()
    assert np.array_equal(ixy[~near, 0], ix[~near]) and np.array_equal(ixy[~near, 1], iy[~near])


def test_new_direction_cases_reach_the_boundaries():
    c = E.new_direction_cases()
    diel = c[:, 6] > 0.0
    dn = (c[:, 0:3] * c[:, 3:6]).sum(1, dtype=np.float32)
    eta = np.where(dn > 0, c[:, 6], np.float32(1.0) / np.where(diel, c[:, 6], np.float32(1.0)))
    s2 = np.array([E.sin2t_f32(abs(a), e) for a, e in zip(dn, eta)], np.float32)
    exact = diel & (s2 == np.float32(1.0)) & (c[:, 3] == 0) & (c[:, 4] == 1)
    assert exact.sum() >= 2                                 # sin2t exactly 1.0: TIR by `>=`
    assert (diel & (s2 < 1.0) & (s2 > 0.999999)).any() and (diel & (s2 > 1.0) & (s2 < 1.000001)).any()
    assert (dn == 0.0).any() and ((dn > 0.0) & (dn < 1e-6)).any()
    nz = c[:, 5]
    assert (nz == 0.0).sum() >= 2 and np.signbit(nz[nz == 0.0]).any() and ((nz != 0.0) & (np.abs(nz) < 1e-38)).any()
    assert ((c[:, 7] > 0.0) & diel).any() and ((c[:, 6] <= 0.0) & (c[:, 7] <= 0.0)).any()


@pytest.mark.parametrize("name", E.LIT)
def test_oracle_env_samples_are_unit_and_inside_their_block(name):
    """The bounds the device's samples are held to (env_maps.DIR_NORM_TOL, BLOCK_SLACK: 4x
    what the oracle shows here), and that the case set has accepted samples to hold."""
    cases = E.env_is_cases(name)
    ok, d, k = O.kat_env_is(E.bottom_up(name), cases)
    norm_err, outside, accepted = E.env_is_sanity(name, cases, ok, d)
    print(name, len(cases), accepted, norm_err, outside)
    assert accepted >= 20000 and np.isfinite(k).all() and (k >= 0.0).all()
    assert norm_err <= E.DIR_NORM_TOL / 4 * 1.01 and outside <= E.BLOCK_SLACK / 4 * 1.01


def test_oracle_new_direction_is_the_float64_restatement():
    cases = E.new_direction_cases()
    st = E.oracle_states(len(cases))
    out, after = O.kat_new_direction(cases, st)
    err, excluded, draws_ok = E.new_direction_error(cases, st, out, after)
    print(len(cases), err, excluded)
    assert draws_ok                                          # 1 uniform (dielectric), 0 (metal), 2 (diffuse)
    assert err <= E.NEW_DIRECTION_TOL / 4 * 1.01 and excluded <= E.NEW_DIRECTION_MAX_EXCLUDED
