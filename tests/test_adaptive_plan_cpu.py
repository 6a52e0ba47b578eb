"""The launch planner's rules for listed launches (host/launch_plan.cpp, PlanInput::n_tiles:
the launches of tpt_render_adaptive over a list of 16x16-pixel tiles), without a GPU.

tpt_adaptive_stats carries no lane mode, so which k_trace variant a pass runs shows only here:
the lane mode and the drained-launch rule key on 256 * n_tiles pixels, not on the frame; a
listed launch has one band set on one stream, its spp chunked as for one set; no XCD runs; and
bands, frame batches, band lists and the wavefront variant are refused.

tests/sanitize/plan_tiles_check.cpp, built here with the host compiler (under ASan + UBSan
where the toolchain has them), prints plan_launches' decisions for each case."""
import json
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

HOST = os.path.join(ROOT, "tinypathtracer_amd", "csrc", "host")
SRCS = [os.path.join(ROOT, "tests", "sanitize", "plan_tiles_check.cpp"), os.path.join(HOST, "launch_plan.cpp")]
BOX = "faces=1932"                 # box.gltf: no delta lights, stacks in LDS
RESIDENT = 327680                  # the harness's default, the MI355X's: 1,280 tiles of 256 pixels
HD = "w=1920,h=1080"               # 8,160 tiles, 2,073,600 pixels: neither four lanes nor drained as a frame


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not os.path.exists(SRCS[0]) or shutil.which("g++") is None:
        pytest.skip("sanitizer harness not present (GPU box) or no g++")
    out = str(tmp_path_factory.mktemp("plan") / "plan_tiles_check")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-o", out]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    r = subprocess.run(base + san + SRCS, capture_output=True, text=True)
    if r.returncode != 0:          # a toolchain without the sanitizers' runtimes: the rules still hold
        r = subprocess.run(base + SRCS, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def plan(exe, *cases):
    r = subprocess.run([exe] + list(cases), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(cases), r.stdout
    return [json.loads(ln) for ln in lines]


def test_lane_mode_and_drained_key_on_the_listed_pixels(exe):
    """Four lanes per pixel up to resident_lanes pixels, drained below twice that -- of the list,
    whatever the frame: the same 1080p frame unlisted takes one lane, not drained."""
    frame, = plan(exe, f"{HD},spp=64,{BOX}")
    assert (frame["quad"], frame["drained"], frame["refill"], frame["leaf_kb"]) == (0, 0, 16, 4)
    at, over, below2, at2, every = plan(exe, *(f"{HD},spp=64,{BOX},tiles={n}" for n in (1280, 1281, 2559, 2560, 8160)))
    assert (at["quad"], at["drained"]) == (1, 1)             # 256 * 1280 = resident_lanes: <=
    assert (over["quad"], over["drained"]) == (0, 1)
    assert (below2["quad"], below2["drained"]) == (0, 1)     # 655,104 < 655,360
    assert (at2["quad"], at2["drained"]) == (0, 0)           # drained is strictly below
    assert (every["quad"], every["drained"]) == (0, 0)       # every tile of the frame listed: as the frame
    assert (over["refill"], over["leaf_kb"]) == (4, 2) and (at2["refill"], at2["leaf_kb"]) == (16, 4)
    # the device's figure, not a constant
    small, = plan(exe, f"{HD},spp=64,{BOX},tiles=1280,resident=327679")
    assert small["quad"] == 0
    # a small frame whose list is its every tile: 3 x 2 tiles
    few, = plan(exe, f"w=37,h=29,spp=16,{BOX},tiles=6")
    assert (few["quad"], few["drained"]) == (1, 1)


def test_lane_mode_requests_and_scenes_without_four_lanes(exe):
    """A listed launch takes the lane modes of an unlisted one: explicit 1 / 2 / 4, pair mode on
    lit scenes, and no four lanes with delta lights, env IS, the reference order or stacks
    beyond LDS -- automatic mode falls back, an explicit 4 is refused."""
    one, two, four = plan(exe, *(f"{HD},spp=16,{BOX},tiles=3,lanes={k}" for k in (1, 2, 4)))
    assert (one["quad"], one["pair"]) == (0, 0) and (two["quad"], two["pair"]) == (0, 1)
    assert (four["quad"], four["pair"]) == (1, 0)
    big4, = plan(exe, f"{HD},spp=16,{BOX},tiles=8160,lanes=4")
    assert big4["quad"] == 1                                 # an explicit request holds at any size
    for why in ("lights=1", "env_is=1", "flags=2", "quad_fits=0"):
        auto, forced = plan(exe, f"{HD},spp=16,{BOX},tiles=3,{why}", f"{HD},spp=16,{BOX},tiles=3,lanes=4,{why}")
        assert auto["status"] == 0 and auto["quad"] == 0 and auto["drained"] == 1, why
        assert auto["pair"] == (1 if why in ("lights=1", "env_is=1") else 0), why
        assert forced["status"] == 1 and "lanes_per_pixel 4" in forced["message"], why
    lit, = plan(exe, f"{HD},spp=16,{BOX},tiles=3,lights=1")
    assert lit["pair_kernel"] == 1 and lit["refill"] == 1 and lit["leaf_kb"] == 1


def test_one_set_chunked_as_for_one_set(exe):
    """One band set on one stream, whatever pipe_sets asks and however many spp: the unlisted
    1080p frame at 1,024 spp splits into three sets.  The chunk is one set's, on the listed pixels."""
    frame, listed, forced = plan(exe, f"{HD},spp=1024,{BOX}", f"{HD},spp=1024,{BOX},tiles=8160",
                                 f"{HD},spp=1024,{BOX},tiles=8160,sets=3,chunks=2")
    assert frame["nset"] == 3
    for p in (listed, forced):
        assert p["nset"] == 1 and p["launches"] == [[0, 1024]] and p["chunk"] == 1024
    # floor(4096 * 2,073,600 / (256 * 8160)) = 4065 spp per launch
    long_, = plan(exe, f"{HD},spp=8192,{BOX},tiles=8160")
    assert long_["nset"] == 1 and long_["chunk"] == 4065 and long_["launches"] == [[0, 4065], [0, 4065], [0, 62]]
    # one tile: the quotient is clamped, the chunk is the pass's spp
    tile, = plan(exe, f"{HD},spp=512,{BOX},tiles=1")
    assert tile["launches"] == [[0, 512]]
    # an explicit spp_per_launch keeps its chunked loop
    spl, = plan(exe, f"{HD},spp=12,spl=5,{BOX},tiles=7")
    assert spl["nset"] == 1 and spl["launches"] == [[0, 5], [0, 5], [0, 2]]


def test_no_xcd_runs(exe):
    frame, listed = plan(exe, f"{HD},spp=8,faces=131072", f"{HD},spp=8,faces=131072,tiles=8160")
    assert frame["xcd_run"] == 5 and listed["xcd_run"] == 0


def test_refusals(exe):
    """The whole frame only: bands, a band list, a frame batch, a call that renders part of the
    rows and the wavefront variant are refused with TPT_ERR_INVALID_ARG."""
    ok, = plan(exe, f"w=64,h=64,spp=8,{BOX},tiles=16")
    assert ok["status"] == 0
    for why in ("bc=2", "bc=2,bi=1", "frames=2", "listed=1", "bh=32", "flags=32"):
        bad, = plan(exe, f"w=64,h=64,spp=8,{BOX},tiles=16,{why}")
        assert bad["status"] == 1 and "tile list" in bad["message"], why
        good, = plan(exe, f"w=64,h=64,spp=8,{BOX},{why}" + (",bh=32" if why.startswith("bc=2") else ""))
        assert good["status"] == 0, why                      # the same call unlisted is planned
