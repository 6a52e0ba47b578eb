"""The premises of tpt_tonemap's device tests, without a GPU: the bin function, the operators' known
values, how few channel samples lie near a rounding boundary, and how far a float32 evaluation of
the map is from the float64 one."""
import numpy as np
import pytest

from tests import tonemap_cases as K
from tests import tonemap_ref as R

W, H = 37, 29
COMBOS = [(op, tr) for op in R.OPS for tr in R.TRANSFERS]


def test_bins_are_monotone_and_follow_the_logarithm():
    L = np.sort(np.concatenate([np.exp2(np.random.default_rng(3).uniform(-16, 16, 20000)),
                                np.exp2(np.arange(-16, 16, 0.125)), [2.0 ** -16, np.nextafter(np.float32(2.0 ** 16), 0)]])
                .astype(np.float32))
    L = L[(L >= np.float32(2.0 ** -16)) & (L < np.float32(2.0 ** 16))]
    b = R.lum_bins(L)
    assert b.min() == 0 and b.max() == 255
    assert (np.diff(b) >= 0).all()
    # a bin is linear in the mantissa inside its octave, so it is floor(8 log2 L) or one more
    ideal = np.floor(8.0 * np.log2(L.astype(np.float64))).astype(int) + 128
    assert (np.abs(b - ideal) <= 1).all()
    # each bin's centre lies inside it
    centres = np.exp2(R.bin_rep(np.arange(256))).astype(np.float32)
    assert (R.lum_bins(centres) == np.arange(256)).all()


def test_bins_of_the_special_values():
    L = np.array([0.0, -0.0, -1.0, -np.inf, 1e-6, np.nextafter(np.float32(2.0 ** -16), 0), 2.0 ** -16, np.nan, np.inf,
                  2.0 ** 16, 3e38, np.nextafter(np.float32(2.0 ** 16), 0)], np.float32)
    assert R.lum_bins(L).tolist() == [R.DARK] * 6 + [0, R.NAN, 255, 255, 255, 255]


@pytest.mark.parametrize("name", K.NAMES)
@pytest.mark.parametrize("size", K.SIZES)
def test_totals_add_up(name, size):
    w, h = size
    hist, counted, dark, nonfinite = R.histogram(K.frame(name, w, h))
    assert counted + dark + nonfinite == w * h
    if name == "planted":
        c = K.plant_counts(w, h)
        assert nonfinite == c["nan"]
        assert dark == c["zero"] + c["negative"] + c["tiny"]
        assert hist[255] == c["inf"]
    if name == "constant":
        assert (hist > 0).sum() == 1 and counted == w * h
    if name == "two_bins" and w * h > 1:
        k = np.flatnonzero(hist)
        assert len(k) == 2 and k[1] - k[0] == 96


def test_the_large_constant_frame_is_past_one_sweep_and_a_16_bit_count():
    w, h = K.SIZES[-1]
    assert w * h > K.SWEEP and w * h > 65535
    assert R.histogram(K.constant(w, h))[0].max() == w * h


def test_measure_on_a_constant_frame_hits_the_key():
    hist = R.histogram(K.constant(W, H))[0]
    log2_avg, log2_scale, s = R.measure(hist, key=0.18)
    k = int(np.flatnonzero(hist)[0])
    assert log2_avg == pytest.approx(R.bin_rep(k), abs=1e-12)
    # (the widest bin, an octave's first, spans log2(9 / 8): no member is farther from its centre)
    assert abs(log2_avg - np.log2(float(R.lum32(K.constant(W, H))[0, 0]))) <= np.log2(9.0 / 8.0)
    assert s == pytest.approx(np.log2(R.f32(0.18)) - log2_avg, abs=1e-12) and log2_scale == s
    # the trim: with the darkest 40 % and the brightest 40 % cut, two_bins' average is within its bins
    h2 = R.histogram(K.two_bins(W, H))[0]
    lo, hi = R.bin_rep(np.flatnonzero(h2))
    assert R.measure(h2, p_low=0.0, p_high=0.4)[0] == pytest.approx(lo, abs=1e-9)
    assert R.measure(h2, p_low=0.6, p_high=1.0)[0] == pytest.approx(hi, abs=1e-9)
    assert R.measure(np.zeros(256), state=None)[1:] == (0.0, None)
    assert R.measure(np.zeros(256), state=1.5, ev=0.5)[1:] == (2.0, 1.5)


def test_operators_known_values():
    grey = lambda v: np.full((1, 1, 3), v, np.float32)   # noqa: E731
    # Reinhard maps Lx == white to 1, and leaves small values nearly alone
    assert R.map_frame(grey(4.0), 1.0, "reinhard", "none", white=4.0)[0, 0, 0] == pytest.approx(1.0, abs=1e-12)
    assert R.map_frame(grey(2.0), 2.0, "reinhard", "none", white=4.0)[0, 0, 0] == pytest.approx(1.0, abs=1e-12)
    assert R.map_frame(grey(1e-4), 1.0, "reinhard", "none")[0, 0, 0] == pytest.approx(1e-4, rel=2e-4)
    assert R.map_frame(grey(0.0), 1.0, "reinhard", "none")[0, 0, 0] == 0.0
    # both curves are monotone
    v = np.exp2(np.linspace(-12, 16, 4000)).astype(np.float32).reshape(-1, 1, 1).repeat(3, axis=2)
    for op in ("reinhard", "aces"):
        y = R.map_frame(v, 1.0, op, "none")[:, 0, 0]
        assert (np.diff(y) >= 0).all() and y[0] < 1e-3 and y[-1] == 1.0
    # the sRGB branches meet at the knee
    knee = 0.0031308
    assert abs(12.92 * knee - (1.055 * knee ** (1 / 2.4) - 0.055)) <= 1e-7
    assert R.map_frame(grey(1.0), 1.0, "linear", "srgb")[0, 0, 0] == pytest.approx(1.0, abs=1e-12)
    assert R.map_frame(grey(0.25), 1.0, "linear", "gamma", gamma=2.0)[0, 0, 0] == pytest.approx(0.5, abs=1e-12)
    # bad values: NaN and negatives to 0, +inf to 1 under every op
    bad = np.array([[[np.nan, -3.0, np.inf]]], np.float32)
    for op in R.OPS:
        assert R.map_frame(bad, 1.0, op, "none")[0, 0].tolist() == [0.0, 0.0, 1.0]


def test_bytes_and_dither():
    y = np.array([[[0.0, 0.5, 1.0]]])
    assert R.to_bytes(R.byte_args(y))[0, 0].tolist() == [255, 128, 0]          # B, G, R; 127.5 + 0.5 = 128
    assert sorted(R.BAYER4.ravel().tolist()) == list(range(16))
    d = R.byte_args(np.zeros((4, 4, 3)), dither=True)[..., 0] - 0.5
    assert d.min() == 0.5 / 16 - 0.5 and d.max() == 15.5 / 16 - 0.5 and abs(d.mean()) < 1e-15
    assert d[1, 0] == (12 + 0.5) / 16 - 0.5                                    # B[y_row][x], row 0 at the bottom


@pytest.mark.parametrize("name", K.NAMES)
@pytest.mark.parametrize("op,transfer", COMBOS)
def test_few_samples_lie_near_a_rounding_boundary(name, op, transfer):
    """What the device tests exclude from the byte comparison is at most 2 % of the samples."""
    y = R.map_frame(K.frame(name, W, H), 1.0, op, transfer)
    for dither in (False, True):
        share = R.near_boundary(R.byte_args(y, dither)).mean()
        assert share <= 0.02, (dither, share)


@pytest.mark.parametrize("op,transfer", COMBOS)
def test_float32_restatement(op, transfer):
    """The map evaluated in float32 stays within 2.6e-7 of the float64 one, a fifteenth of BOUND,
    and gives the same bytes on the log-uniform case."""
    worst = 0.0
    for name in K.NAMES:
        f = K.frame(name, W, H)
        y64 = R.map_frame(f, 1.0, op, transfer)
        y32 = R.map_frame(f, 1.0, op, transfer, dtype=np.float32)
        assert y32.dtype == np.float32 and np.isfinite(y32).all()
        worst = max(worst, float(np.abs(y32.astype(np.float64) - y64).max()))
    assert worst <= 2.6e-7, worst
    f = K.log_uniform(W, H)
    b64 = R.to_bytes(R.byte_args(R.map_frame(f, 1.0, op, transfer)))
    b32 = R.to_bytes(R.byte_args(R.map_frame(f, 1.0, op, transfer, dtype=np.float32).astype(np.float64)))
    assert (b64 == b32).all()


def test_bound_is_within_the_issue_limit():
    assert R.BOUND <= 1e-5 and R.DELTA == 255.0 * R.BOUND
