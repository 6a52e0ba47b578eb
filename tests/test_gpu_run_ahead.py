"""Run-ahead across sample chunks (the 8-level variants of k_trace's one-lane full-occupancy
family).

When a set's spp is cut into several launches, a lane that has run a launch's samples while
another lane of its wave still owes some goes on with the pixel's next samples, and the
pixel's credit plane tells the set's next launch how many are already done.  Every pixel's
samples still run in order on its own stream, so every schedule must give the frame of one
launch bit for bit, and the totals of the frame's stats that its samples fix must be those
of one launch.

The one-lane full-occupancy family runs only launches of at least twice the chip's resident
lanes in pixels (host/launch_plan.cpp), so every property is checked at two sizes: the small
frame, where the four-lane or drained variants run (compiled without run-ahead: unchanged)
and the CPU oracle is the reference, and a full-chip frame (FULL, the size
tests/test_gpu_unwind_prune.py and tests/test_gpu_wg_shape.py use for that family), where the
new code runs and one launch of the same library is the reference; the full-chip frame meets
the oracle once, at 2 spp in two launches (the oracle frame test_gpu_unwind_prune.py shares).
Every image comparison is bitwise."""
import numpy as np
import pytest

import tinypathtracer_amd as T
from tests import prune_scenes as PS
from tests.conftest import scene_path

pytestmark = pytest.mark.gpu

FAST = T._lib.FLAG_FAST
FULL = (1184, 560)   # 663,040 pixels: at least twice the resident lanes of an MI355X (2 x 327,680)
# What a frame's samples fix whatever the schedule.  wide_visits and leaf_tests are not among them:
# a lane walks on past a parked leaf with the hit distance it had (speculative leaf postponement),
# and when its wave runs the parked tests depends on the lanes it shares its steps with, so the two
# counts move with the schedule in every family, with or without run-ahead (drained one-lane box
# 40x24, 12 spp: 180,745 wide visits in one launch, 180,796 under 3 sets x 2 chunks, the same two
# figures from the library before run-ahead).  They are printed beside the others.
TOTALS = ("traversals", "local_rays", "shade_hits", "samples")
SCHEDULE_DEPENDENT = ("wide_visits", "leaf_tests")
PIPES = [dict(pipe_sets=3, pipe_chunks=2), dict(pipe_sets=2, pipe_chunks=4)]


def ibits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture(scope="module")
def device():
    out = {}

    def get(name):
        if name not in out:
            s = T.Scene(scene_path(name))
            out[name] = (s, s.copySceneToDevice(0).build())
        return out[name]

    yield get
    for _, d in out.values():
        d.close()


def render(device, name, w, h, spp, depth=8, pt=None, rad=None, **kw):
    s, d = device(name)
    pt = pt or T.PathTracer("", w, h, 0)
    rad = np.zeros((h, w, 3), np.float32) if rad is None else rad
    st = pt.doTrace(d, s.m_camera, None, spp, seed=kw.pop("seed", 42), max_depth=depth, radiance=rad, **kw)
    return rad, st


def one_lane_family(st, w, h):
    """The launch ran the one-lane full-occupancy family, the one compiled with run-ahead."""
    assert st["drained"] == 0 and st["lanes_per_pixel"] == 1 and w * h >= 2 * st["resident_lanes"], st


def same_totals(st, st1):
    print("totals", [(k, st[k], st1[k]) for k in TOTALS + SCHEDULE_DEPENDENT])
    for k in TOTALS:
        assert st[k] == st1[k], (k, st[k], st1[k])


# ---- 1. forced pipelines against one launch and the oracle ----
@pytest.mark.parametrize("spp", [12, 13])
@pytest.mark.parametrize("size", [(40, 24), (72, 40)], ids=["40x24", "72x40"])
def test_forced_pipelines_small(device, size, spp):
    """box, depth 8: 3 sets x 2 chunks and 2 sets x 4 chunks, as the launch rule deals them and with
    one lane per pixel, in bands of 16 rows and of 8 (where a frame this low has rows for every set)."""
    w, h = size
    orad, oc = PS.oracle_frame("box", PS.base("box"), w=w, h=h, spp=spp)
    for lanes in (0, 1):
        one, st1 = render(device, "box", w, h, spp, lanes_per_pixel=lanes, pipe_sets=1)
        assert st1["trace_launches"] == 1
        PS.assert_same(one, orad)
        assert st1["traversals"] == oc["traversals"]
        for pipe in PIPES:
            for rows in (16, 8):
                got, st = render(device, "box", w, h, spp, lanes_per_pixel=lanes, band=(rows, 1, 0), **pipe)
                assert np.array_equal(ibits(got), ibits(one)), (pipe, lanes, rows)
                PS.assert_same(got, orad)
                same_totals(st, st1)
                if h >= pipe["pipe_sets"] * rows:
                    assert st["trace_launches"] > pipe["pipe_sets"], (pipe, rows, st)


@pytest.fixture(scope="module")
def full_one(device):
    """One launch of the full-chip frame per spp: the reference of the schedules below."""
    out = {}

    def get(spp):
        if spp not in out:
            rad, st = render(device, "box", *FULL, spp, pipe_sets=1, spp_per_launch=spp)
            assert st["trace_launches"] == 1
            one_lane_family(st, *FULL)
            rad.setflags(write=False)
            out[spp] = (rad, st)
        return out[spp]

    return get


@pytest.mark.parametrize("spp", [12, 13])
@pytest.mark.parametrize("pipe", PIPES, ids=["3x2", "2x4"])
def test_forced_pipelines_full_chip(device, full_one, pipe, spp):
    one, st1 = full_one(spp)
    got, st = render(device, "box", *FULL, spp, **pipe)
    one_lane_family(st, *FULL)
    assert st["trace_launches"] > pipe["pipe_sets"]
    assert np.array_equal(ibits(got), ibits(one))
    same_totals(st, st1)


def test_full_chip_two_launches_match_the_oracle(device):
    """2 spp in two launches of 1: the first may run the second's sample, the second then has
    lanes with nothing left.  Against the oracle's frame."""
    got, st = render(device, "box", *FULL, 2, spp_per_launch=1)
    one_lane_family(st, *FULL)
    assert st["trace_launches"] == 2
    orad, oc = PS.oracle_frame("box", PS.base("box"), w=FULL[0], h=FULL[1], spp=2)
    PS.assert_same(got, orad)
    assert st["traversals"] == oc["traversals"]


# ---- 2. a last launch smaller than the credit a lane can hold ----
@pytest.mark.parametrize("size", [(17, 9), FULL], ids=["17x9", "full-chip"])
def test_short_last_launch(device, size):
    """spp 12 in launches of 5, 5 and 2: after the first a lane may hold 7 samples of credit, more
    than the second launch's 5 and than the last one's 2; every pixel still ends at exactly 12."""
    w, h = size
    one, st1 = render(device, "box", w, h, 12, spp_per_launch=12)
    got, st = render(device, "box", w, h, 12, spp_per_launch=5)
    assert (st1["trace_launches"], st["trace_launches"]) == (1, 3)
    if size == FULL:
        one_lane_family(st, w, h)
    assert np.array_equal(ibits(got), ibits(one))
    same_totals(st, st1)
    assert st["samples"] == w * h * 12


# ---- 3. tiles that mix miss pixels and object pixels: lanes that enter a launch with remaining < 0 ----
def _banded(device, w, h, spp, expect_family, **pipe):
    """The frame in three interleaved bands of 16 rows, as band = (16, 3, i) and as explicit lists."""
    s, d = device("box")
    pt = T.PathTracer("", w, h, 0)
    one, st1 = render(device, "box", w, h, spp, pt=pt, pipe_sets=1, spp_per_launch=spp)
    n_bands = (h + 15) // 16
    for deal in ("interleaved", "listed"):
        got = np.zeros((h, w, 3), np.float32)
        tot = dict.fromkeys(TOTALS + SCHEDULE_DEPENDENT, 0)
        for i in range(3):
            kw = dict(band=(16, 3, i)) if deal == "interleaved" else dict(band_list=list(range(i, n_bands, 3)))
            _, st = render(device, "box", w, h, spp, pt=pt, rad=got, **kw, **pipe)
            assert st["trace_launches"] > 1, (deal, i, st)
            if expect_family:
                assert st["drained"] == 0 and st["lanes_per_pixel"] == 1, (deal, i, st)
            for k in tot:
                tot[k] += st[k]
        assert np.array_equal(ibits(got), ibits(one)), deal
        same_totals(tot, st1)
    return one


def test_mixed_tiles_banded_small(device):
    """72x40: box's walls end inside the frame, so its edge tiles hold miss pixels (one ray per
    sample) beside object pixels."""
    one = _banded(device, 72, 40, 12, False, spp_per_launch=5)
    orad, _ = PS.oracle_frame("box", PS.base("box"), w=72, h=40, spp=12)
    PS.assert_same(one, orad)
    miss = (ibits(one) == 0).all(-1)
    assert miss.any() and not miss.all()


def test_mixed_tiles_banded_full_chip(device):
    """1920x1080, where each of the three bands' calls is a full-chip launch of its own: chunks of
    5, 5 and 2 on one stream, then two sets of three chunks."""
    _banded(device, 1920, 1080, 12, True, spp_per_launch=5)
    _banded(device, 1920, 1080, 6, True, pipe_sets=2, pipe_chunks=3)


@pytest.mark.parametrize("size", [(72, 40), FULL], ids=["72x40", "full-chip"])
def test_frame_batch(device, size):
    """Three frames in one call: each frame has a credit plane of its own."""
    w, h = size
    s, d = device("box")
    pt = T.PathTracer("", w, h, 0)
    seeds = [42, 43, 44]
    ones = [np.zeros((h, w, 3), np.float32) for _ in seeds]
    st1 = pt.doTraceFrames(d, s.m_camera, seeds, None, 12, radiances=ones, pipe_sets=1, spp_per_launch=12)
    assert st1["trace_launches"] == 1
    rows = 8 if h < 48 else 16   # (bands of 8 rows give a frame this low rows for three sets)
    for kw in (dict(pipe_sets=3, pipe_chunks=2, band=(rows, 1, 0)), dict(spp_per_launch=5)):
        got = [np.zeros((h, w, 3), np.float32) for _ in seeds]
        st = pt.doTraceFrames(d, s.m_camera, seeds, None, 12, radiances=got, **kw)
        assert st["trace_launches"] >= 3
        if size == FULL:
            assert st["drained"] == 0 and st["lanes_per_pixel"] == 1
        for f in range(len(seeds)):
            assert np.array_equal(ibits(got[f]), ibits(ones[f])), (kw, f)
        same_totals(st, st1)
    assert not np.array_equal(ibits(ones[0]), ibits(ones[1]))
    if size != FULL:
        orad, _ = PS.oracle_frame("box", PS.base("box"), w=w, h=h, spp=12)
        PS.assert_same(ones[0], orad)


# ---- 4. progressive accumulation ----
@pytest.mark.parametrize("size", [(40, 24), FULL], ids=["40x24", "full-chip"])
def test_progressive(device, size):
    """4 + 4 spp under a forced 3 x 2 pipeline equals 8 spp in one call: the credit is zero at the
    end of a call, so the continuation starts every pixel at its next sample."""
    w, h = size
    s, d = device("box")
    pt = T.PathTracer("", w, h, 0)
    one, st1 = render(device, "box", w, h, 8, pt=pt, pipe_sets=1, spp_per_launch=8)
    prog = np.zeros((h, w, 3), np.float32)
    rows = 8 if h < 48 else 16
    _, st_a = render(device, "box", w, h, 4, pt=pt, rad=prog, band=(rows, 1, 0), pipe_sets=3, pipe_chunks=2)
    _, st_b = render(device, "box", w, h, 4, pt=pt, rad=prog, band=(rows, 1, 0), pipe_sets=3, pipe_chunks=2, seed=None,
                     accumulate=True)
    assert st_a["trace_launches"] > 3 and st_b["trace_launches"] > 3
    assert st_b["accumulated_spp"] == 8
    if size == FULL:
        one_lane_family(st_b, w, h)
    assert np.array_equal(ibits(prog), ibits(one))
    for k in TOTALS:
        assert st_a[k] + st_b[k] == st1[k], k


# ---- 5. deep records and a large scene ----
@pytest.mark.parametrize("size", [(40, 24), FULL], ids=["40x24", "full-chip"])
def test_tir_deep_records(device, size):
    """tir at depth 32: the MAXD 64 variants, compiled without run-ahead (it lost at C4, which runs
    them): chunked schedules must give them the same frame as ever."""
    w, h = size
    one, st1 = render(device, "tir", w, h, 8, depth=32, lanes_per_pixel=1, pipe_sets=1, spp_per_launch=8)
    got, st = render(device, "tir", w, h, 8, depth=32, lanes_per_pixel=1, band=(8 if h < 48 else 16, 1, 0), pipe_sets=3,
                     pipe_chunks=2)
    assert st["trace_launches"] > 3
    assert np.array_equal(ibits(got), ibits(one))
    same_totals(st, st1)
    if size == FULL:
        assert st["drained"] == 0 and st["lanes_per_pixel"] == 1
    else:
        orad, oc = PS.oracle_frame("tir", PS.base("tir"), w=w, h=h, spp=8, depth=32)
        PS.assert_same(got, orad)
        assert st["traversals"] == oc["traversals"]


@pytest.mark.parametrize("size", [(256, 32), FULL], ids=["256x32", "full-chip"])
def test_c5_scene(device, size):
    """The synthesised C5 scene (131 K triangles: 32-bit stack ids, XCD runs at the full-chip size)."""
    w, h = size
    spp = 4
    one, st1 = render(device, "c5", w, h, spp, pipe_sets=1, spp_per_launch=spp)
    got, st = render(device, "c5", w, h, spp, pipe_sets=2, pipe_chunks=2)
    assert st["trace_launches"] == 4 + 1   # set 1 starts half a chunk early: 1 + 2 + 1
    assert np.array_equal(ibits(got), ibits(one))
    same_totals(st, st1)
    if size == FULL:
        one_lane_family(st, w, h)
    else:
        orad, oc = PS.oracle_frame("c5", PS.base("c5"), w=w, h=h, spp=spp)
        PS.assert_same(got, orad)
        assert st["traversals"] == oc["traversals"]


# ---- 6. the tolerance build ----
@pytest.mark.parametrize("size", [(72, 40), FULL], ids=["72x40", "full-chip"])
def test_fast_build(device, size):
    """TPT_FLAG_FAST is deterministic too: its pipeline equals its one launch bit for bit."""
    w, h = size
    one, st1 = render(device, "box", w, h, 12, flags=FAST, pipe_sets=1, spp_per_launch=12)
    for kw in (dict(pipe_sets=2, pipe_chunks=4), dict(spp_per_launch=5)):
        got, st = render(device, "box", w, h, 12, flags=FAST, **kw)
        assert st["trace_launches"] >= 3
        if size == FULL:
            one_lane_family(st, w, h)
        assert np.array_equal(ibits(got), ibits(one)), kw
        same_totals(st, st1)
