"""Host state that threads share, under the sanitizers (tests/sanitize/host_check.cpp,
stand-alone programs with their own main; CPU only, as tests/test_host_sanitize.py).

include/tpt.h lets calls on different scenes run concurrently from different host
threads.  What such threads share on the host:

* the RNG's jump table (host/rng_host.cpp host_jumps), built by the process's first
  tpt_scene_create or tpt_debug_rng_init.  `jumps 8`: eight threads make that first call
  together, and each must see the table a serial xorwow_jump_matrices builds.  (Built as
  "if empty: resize, then fill", the threads that lost the race saw zeros, or the ASan
  build aborted in the doubled resize, and ThreadSanitizer reported the race on the vector.)
* nothing in the parsers, the launch planner or the variant selection.  `parse-threads 8`
  pins that: eight threads load every shipped scene, decode a baseline and a progressive
  JPEG and run the plan and variant cases of tests/test_host_sanitize.py at once, each on
  its own objects, and compare their bytes with the serial run's.

Each mode runs under the ASan + UBSan build and under the ThreadSanitizer build."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT, SCENE_DIR
from tests.test_host_sanitize import BOX, LAYOUT_PINS, SAN, _make

# 64 x 48 seeded noise, saved by PIL at quality 90 (baseline) and at quality 50, progressive
IMAGES = [os.path.join(ROOT, "tests", "golden", "images", f"noise_64x48_{kind}.jpg")
          for kind in ("baseline", "progressive")]

THREADS = 8

# (make target, the runtime's words in a failed link, the options of the run)
BUILDS = {
    "asan": ("host_check", ("asan", "sanitize"),
             {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:allocator_may_return_null=1",
              "UBSAN_OPTIONS": "print_stacktrace=1"}),
    "tsan": ("host_check_tsan", ("tsan", "sanitize"), {"TSAN_OPTIONS": "halt_on_error=1"}),
}

# the cases of tests/test_host_sanitize.py's test_plan_* and test_variant_*
PLAN_CASES = [
    f"w=1920,h=1080,spp=1024,{BOX}",
    *(f"w=96,h=80,spp=256,{BOX},sets={k}" for k in (1, 0, 2, 3, 4)),
    f"w=32,h=32,spp=12,spl=5,{BOX}", f"w=64,h=48,spp=8,sets=3,chunks=2,{BOX}", f"w=96,h=40,spp=1024,sets=3,{BOX}",
    f"w=1920,h=1080,spp=4096,lights=1,{BOX}", f"w=1920,h=1080,spp=4096,lights=1,{BOX},flags=2",
    *(f"w={w},h=64,spp=8,faces={f}" for f in (131072, 16384) for w in (3840, 1920, 640, 256, 100)),
    *(f"w=1920,h=1080,spp=1024,bc={n},bi=0,{BOX}" for n in (8, 4, 2)),
    f"w=96,h=96,spp=8,sets=2,chunks=2,list=5:1:3:0:2,{BOX}",
    f"w=64,h=64,spp=8,lanes=3,{BOX}", f"w=64,h=64,spp=8,lanes=4,lights=1,{BOX}",
    f"w=64,h=1080,rows=1080,frames=65535,spp=8,lanes=1,{BOX}",
]
VARIANT_CASES = ["table"] + ["select=1," + c for c in (
    "pair=0", "drained=1", "pair=1,drained=1,lights=1,mtls=0,faces=5000,emitter=0", "pair=1,lights=1,mtls=0,faces=5000",
    "pair=0,drained=1,lights=1,mtls=0,faces=5000", "pair=1", "env_is=1,drained=1", "env_is=1,pair=1,emitter=0",
    "env_is=1,quad=1", "ref=1,pair=1,quad=1,drained=1,lights=1", "ref=1,env_is=1,pair=1,mtls=0,faces=6,depth=2",
    "quad=1,drained=1", "quad=1,lights=1", "quad=1,mtls=32766", "mtls=32765", "mtls=32766", "mtls=32765,pair=1,lights=1",
    "mtls=32766,pair=1,lights=1", "mtls=32765,pair=1,env_is=1", "mtls=32766,pair=1,env_is=1", "mtls=62", "mtls=63",
    "mtls=64", "faces=32768", "faces=32769", "faces=32768,pair=1,lights=1", "faces=32769,pair=1,lights=1", "depth=1",
    "depth=8", "depth=9", "depth=64")] + ["layout=1," + c for c, _ in LAYOUT_PINS]


@pytest.fixture(scope="module", params=sorted(BUILDS))
def binary(request):
    """(path, environment) of one sanitizer build; the skips of test_wide_tree_pool_under_tsan."""
    target, words, options = BUILDS[request.param]
    if not os.path.isdir(SAN) or shutil.which("g++") is None:
        pytest.skip("sanitizer harness not present (GPU box) or no g++")
    r = _make(target)
    if r.returncode != 0:
        if any(w in r.stderr.lower() for w in words):
            pytest.skip(f"toolchain without the {request.param} runtime")
        raise AssertionError(r.stderr)
    return os.path.join(SAN, target), dict(os.environ, **options)


def _ok(binary, *args):
    exe, env = binary
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_jump_table_first_use_from_many_threads(binary):
    out = _ok(binary, "jumps", THREADS)
    assert f"{THREADS} threads saw the serial table (12800 words)" in out, out


def test_parsers_and_planner_from_many_threads(binary):
    for path, sof in zip(IMAGES, (b"\xff\xc0", b"\xff\xc2")):      # the fixtures are what their names say
        assert sof in open(path, "rb").read()
    scenes = sorted(os.path.join(SCENE_DIR, f) for f in os.listdir(SCENE_DIR) if f.endswith(".gltf"))
    assert len(scenes) >= 7
    out = _ok(binary, "parse-threads", THREADS, "--gltf", *scenes, "--image", *IMAGES, "--plan", *PLAN_CASES,
              "--variant", *VARIANT_CASES)
    assert (f"{THREADS} threads, {len(scenes)} scenes, 2 images, {len(PLAN_CASES)} plans, "
            f"{len(VARIANT_CASES)} variant cases") in out, out
