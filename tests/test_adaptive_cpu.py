"""tpt_render_adaptive on the CPU: the premises of tests/test_gpu_adaptive.py, shown on the
oracle alone with tests/adaptive_ref.py.

For every case the schedule on oracle frames must exercise the stopping rule -- tiles that
stop at min_spp, tiles that stop at a level in between, tiles that reach max_spp, one of them
unconverged -- and no estimate at any checkpoint may lie within 1e-3 relative of the case's
target, so that the device's float32 estimate (rtol 1e-4 of the float64 one) decides every
tile the same way.  box_17x16 has two tiles and therefore two levels.  The tables the targets
were read off are printed."""
import numpy as np
import pytest

from tests import adaptive_ref as R


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_case_exercises_the_stopping_rule(name):
    target = R.CASES[name][5]
    ref = R.reference(name)
    levels = np.unique(ref["tile_spp"])
    for n, E in ref["checkpoints"]:
        print(name, "n", n, np.sort(E).round(4))
    print(name, "target", target, "levels", dict(zip(*np.unique(ref["tile_spp"], return_counts=True))),
          "unconverged", ref["unconverged"], "passes", ref["passes"])
    assert len(levels) >= R.MIN_LEVELS[name]
    assert levels[0] == R.MIN_SPP and levels[-1] == R.MAX_SPP
    if R.MIN_LEVELS[name] >= 3:
        assert any(R.MIN_SPP < n < R.MAX_SPP for n in levels)
    assert ref["unconverged"] >= 1
    assert ref["passes"] == 2 + int(np.log2(R.MAX_SPP // R.MIN_SPP))
    for n, E in ref["checkpoints"]:
        assert np.isfinite(E).all()
        assert (np.abs(E - target) > 1e-3 * target).all(), (n, E)


def test_issue_table_box_37x29():
    """The estimates of box at 37 x 29 (seed 42) at 2 and at 32 samples, as recorded when the
    feature was specified: the reference computes what the specification simulated."""
    lv = R.oracle_levels("box_37x29")
    assert np.allclose(np.sort(R.tile_errors(lv[2], lv[1]).ravel()), [0, 0, 0.268, 0.273, 0.41, 0.484], atol=1e-3)
    assert np.allclose(np.sort(R.tile_errors(lv[32], lv[16]).ravel()), [0, 0, 0.166, 0.182, 0.289, 0.305], atol=1e-3)
    r = R.schedule(lv, 0.3)
    assert sorted(np.unique(r["tile_spp"])) == [2, 32] and r["unconverged"] == 1


def test_schedule_degenerate_targets_and_nan():
    lv = R.oracle_levels("box_37x29")
    r0, rinf = R.schedule(lv, 0.0), R.schedule(lv, np.inf)
    assert (r0["tile_spp"] == R.MAX_SPP).all() and r0["unconverged"] == r0["tile_spp"].size
    assert (rinf["tile_spp"] == R.MIN_SPP).all() and rinf["unconverged"] == 0 and rinf["passes"] == 2
    # a non-finite pixel: its tile's estimate is NaN, below no target, so it runs to max_spp
    bad = {n: f.copy() for n, f in lv.items()}
    for f in bad.values():
        f[0, 0, 0] = np.inf
    rb = R.schedule(bad, np.inf)
    assert rb["tile_spp"][0, 0] == R.MAX_SPP and np.isnan(rb["tile_error"][0, 0]) and rb["unconverged"] == 1
    assert (rb["tile_spp"].ravel()[1:] == R.MIN_SPP).all()


def test_compose_takes_each_pixel_from_its_tiles_frame():
    spp = np.array([[2, 4, 2], [4, 2, 4]], np.int32)
    frames = {2: np.full((29, 37, 3), 2.0, np.float32), 4: np.full((29, 37, 3), 4.0, np.float32)}
    out = R.compose(spp, frames)
    assert (out[:16, :16] == 2).all() and (out[:16, 16:32] == 4).all() and (out[16:, 32:] == 4).all()
    assert (out[16:, 16:32] == 2).all()
