"""The host-side parsers under AddressSanitizer + UndefinedBehaviorSanitizer
(SURVEY.md section 5): host/gltf.cpp + json_lite.hpp, host/image.cpp (JPEG
baseline / progressive, PPM) and host/wide_bvh.cpp, built for the CPU by
tests/sanitize/Makefile and fed valid and corrupted inputs -- truncated files,
flipped bytes, bad Huffman tables, absurd dimensions and sampling factors,
malformed JSON, negative / huge / out-of-range accessor fields, broken data
URIs.  Every input must end in "ok" or a parse error; a memory error or
undefined behaviour aborts the harness with the sanitizer's report.

The same harness runs the launch planner (host/launch_plan.cpp, the launch rules
of tpt_render_frames): the test_plan_* cases pin the lane mode, the kernel knobs
and the launch schedule it decides, which otherwise show only on a GPU.  The
test_variant_* cases do the same for the k_trace variant space
(common/trace_variant.hpp): the family table, the rule that picks a launch's
variant, its agreement with the planner and the LDS layout.

CPU only (the sanitizer build never travels to the GPU box)."""
import base64
import io
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT, SCENE_DIR

SAN = os.path.join(ROOT, "tests", "sanitize")


def _make(target):
    """make under an exclusive lock: pytest-xdist workers each set the module's
    fixtures up, and two concurrent links of one binary fail ("Text file busy")."""
    import fcntl
    with open(os.path.join(SAN, ".build.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        return subprocess.run(["make", "-C", SAN, target], capture_output=True, text=True)


@pytest.fixture(scope="module")
def host_check():
    if not os.path.isdir(SAN) or shutil.which("g++") is None:
        pytest.skip("sanitizer harness not present (GPU box) or no g++")
    r = _make("host_check")
    if r.returncode != 0:
        if "asan" in r.stderr.lower() or "sanitize" in r.stderr.lower():
            pytest.skip("toolchain without ASan/UBSan runtime")
        raise AssertionError(r.stderr)
    return os.path.join(SAN, "host_check")


def run(exe, mode, files):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:allocator_may_return_null=1",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, mode] + [str(f) for f in files], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(files), r.stdout
    return lines


def test_valid_scenes(host_check):
    files = sorted(os.path.join(SCENE_DIR, f) for f in os.listdir(SCENE_DIR) if f.endswith(".gltf"))
    out = run(host_check, "gltf", files)
    assert all(x.startswith("ok") for x in out), out


def _mutants(model):
    """Malformed variants of a glTF model (dict) with an embedded buffer."""
    m = json.loads(json.dumps(model))
    out = []

    def mut(fn):
        x = json.loads(json.dumps(m))
        fn(x)
        out.append(json.dumps(x))

    acc = m["accessors"]
    for i in range(min(len(acc), 3)):
        for key, val in (("byteOffset", -4), ("byteOffset", 2 ** 62), ("byteOffset", 1e30), ("count", -1),
                         ("count", 2 ** 40), ("count", 1e300), ("count", 2 ** 61 + 7), ("bufferView", 99),
                         ("bufferView", -3), ("componentType", 5130), ("type", "MAT4"), ("count", 0)):
            mut(lambda x, i=i, key=key, val=val: x["accessors"][i].__setitem__(key, val))
    for key, val in (("byteOffset", -8), ("byteOffset", 10 ** 12), ("buffer", 5), ("byteLength", -1)):
        mut(lambda x, key=key, val=val: x["bufferViews"][0].__setitem__(key, val))
    mut(lambda x: x["buffers"][0].__setitem__("uri", x["buffers"][0]["uri"][:-40]))          # short buffer
    mut(lambda x: x["buffers"][0].__setitem__("uri", x["buffers"][0]["uri"][:60] + "!!@@"))  # bad base64
    mut(lambda x: x["buffers"][0].__setitem__("uri", "data:application/octet-stream;base64,"))
    mut(lambda x: x["buffers"][0].__setitem__("uri", "does_not_exist.bin"))
    mut(lambda x: x["meshes"][0]["primitives"][0].__setitem__("indices", 10 ** 9))
    mut(lambda x: x["meshes"][0]["primitives"][0]["attributes"].__setitem__("POSITION", -1))
    mut(lambda x: x["meshes"][0]["primitives"][0].__setitem__("material", 1e99))
    mut(lambda x: x["meshes"][0].__setitem__("primitives", []))
    mut(lambda x: x["nodes"][0].__setitem__("mesh", 2 ** 31))
    mut(lambda x: x["nodes"][0].__setitem__("mesh", -1e308))
    mut(lambda x: x["nodes"][0].__setitem__("rotation", [1, 2]))
    mut(lambda x: x["nodes"][0].__setitem__("scale", "big"))
    mut(lambda x: x.__setitem__("accessors", {}))
    mut(lambda x: x.__setitem__("nodes", 7))
    return out


def test_corrupted_gltf(host_check, tmp_path):
    files = []
    for name in ("box", "square", "ball"):
        text = open(os.path.join(SCENE_DIR, f"{name}.gltf")).read()
        model = json.loads(text)
        for k, t in enumerate(_mutants(model)):
            p = tmp_path / f"{name}_m{k}.gltf"
            p.write_text(t)
            files.append(p)
        for cut in (0, 1, 10, len(text) // 3, len(text) // 2, len(text) - 2):   # truncated JSON
            p = tmp_path / f"{name}_cut{cut}.gltf"
            p.write_text(text[:cut])
            files.append(p)
    rng = np.random.default_rng(3)
    text = open(os.path.join(SCENE_DIR, "box.gltf")).read()
    for k in range(40):                                  # random byte flips
        b = bytearray(text.encode())
        for _ in range(8):
            b[rng.integers(len(b))] = int(rng.integers(32, 127))
        p = tmp_path / f"flip{k}.gltf"
        p.write_bytes(bytes(b))
        files.append(p)
    for k, t in enumerate(["[" * 200000, "{\"a\":" * 100000, "1e400", "-", "\"\\u12", "{\"a\" 1}", "nan", "\0\0\0",
                           "{\"accessors\": [{\"count\": 1e999}]}", "[1,2,3" + ",4" * 100000]):
        p = tmp_path / f"json{k}.gltf"
        p.write_text(t)
        files.append(p)
    out = run(host_check, "gltf", files)
    assert sum(x.startswith("error") for x in out) > len(files) // 2


def _jpeg(arr, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", **kw)
    return buf.getvalue()


def test_corrupted_images(host_check, tmp_path):
    pytest.importorskip("PIL")
    rng = np.random.default_rng(11)
    sky = (rng.uniform(0, 255, (48, 64, 3))).astype(np.uint8)
    goods = [_jpeg(sky, quality=90), _jpeg(sky, quality=50, progressive=True),
             _jpeg(sky, quality=75, subsampling=0), _jpeg(sky, quality=75, subsampling=2)]
    files = []
    for k, g in enumerate(goods):
        p = tmp_path / f"good{k}.jpg"
        p.write_bytes(g)
        files.append(p)
    out = run(host_check, "image", files)
    assert all(x.startswith("ok") for x in out), out
    files = []
    for k, g in enumerate(goods):
        for cut in sorted(set([2, 4, 20, 100, 200, 400, len(g) // 2, len(g) - 10, len(g) - 2]
                              + list(range(3, len(g), 97)))):
            p = tmp_path / f"cut{k}_{cut}.jpg"
            p.write_bytes(g[:cut])
            files.append(p)
        for j in range(250):                             # flipped bytes, headers included
            b = bytearray(g)
            for _ in range(1 + j % 4):
                pos = int(rng.integers(2, min(len(b), 700))) if j % 2 else int(rng.integers(2, len(b)))
                b[pos] = int(rng.integers(0, 256))
            p = tmp_path / f"flip{k}_{j}.jpg"
            p.write_bytes(bytes(b))
            files.append(p)
    g = bytearray(goods[0])
    i = g.find(b"\xff\xc4")                              # DHT: code counts that overflow 256 symbols
    if i > 0:
        b = bytearray(g)
        for q in range(16):
            b[i + 5 + q] = 255
        (tmp_path / "dht.jpg").write_bytes(bytes(b))
        files.append(tmp_path / "dht.jpg")
    i = g.find(b"\xff\xc0")                              # SOF0: absurd dimensions, components, sampling
    if i > 0:
        for k, (off, val) in enumerate(((5, b"\xff\xff\xff\xff"), (5, b"\x00\x00\x00\x00"), (9, b"\x07"),
                                        (11, b"\x00"), (11, b"\x55"), (11, b"\xff"), (12, b"\x09"))):
            b = bytearray(g)
            b[i + off:i + off + len(val)] = val
            p = tmp_path / f"sof{k}.jpg"
            p.write_bytes(bytes(b))
            files.append(p)
    for k, t in enumerate([b"P6\n64 48\n255\n" + bytes(100), b"P6\n-1 48\n255\n", b"P6\n99999 99999\n255\n",
                           b"P6\n4 4\n0\n" + bytes(48), b"P6\n4 4\n65535\n" + bytes(10), b"P6", b"P3\n1 1\n255\n1 2 3",
                           b"P6\n4 4 255 " + bytes(48), b"P6\n#c\n4 4\n255\n" + bytes(48)]):
        p = tmp_path / f"ppm{k}.ppm"
        p.write_bytes(t)
        files.append(p)
    out = run(host_check, "image", files)
    assert sum(x.startswith("error") for x in out) > len(files) // 3


@pytest.mark.parametrize("n,seed,threads", [(2, 1, -1), (3, 2, -1), (33, 3, -1), (1000, 4, -1), (20000, 5, -1),
                                            (20000, 6, 4)])
def test_wide_tree_builder(host_check, n, seed, threads):
    r = subprocess.run([host_check, "wide", str(n), str(seed), str(threads)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr[-3000:]


def _plan(exe, *cases):
    """plan_launches (host/launch_plan.cpp) on each case ("key=value,..." as
    host_check.cpp plan_case reads it): one dict per case."""
    return [json.loads(x) for x in run(exe, "plan", cases)]


def _sets(plan):
    """Each set's launches, in order."""
    return [[n for k, n in plan["launches"] if k == s] for s in range(plan["nset"])]


BOX = "faces=1932"   # box.gltf: 1,932 triangles, no delta lights; resident lanes 327,680, 16 band rows, one frame


def test_plan_default_1080p(host_check):
    """The launch rules of tpt_render_frames, as the code before the planner was
    split out computed them (derived by hand from it): box at 1080p, 1024 spp."""
    p, = _plan(host_check, f"w=1920,h=1080,spp=1024,{BOX}")
    assert (p["pair"], p["pair_kernel"], p["quad"], p["drained"]) == (0, 0, 0, 0)
    assert (p["refill"], p["leaf_kb"], p["xcd_run"], p["wg_rows"]) == (16, 4, 0, 16)
    assert (p["nset"], p["chunk"], len(p["launches"])) == (3, 128, 26)
    assert _sets(p) == [[128] * 8, [86] + [128] * 7 + [42], [43] + [128] * 7 + [85]]
    assert p["set_rows"] == [368, 360, 352]


def test_plan_small_frame_and_forced_sets(host_check):
    """96 x 80 at 256 spp (test_gpu_parity.py test_launch_pipeline_bit_identical
    asserts the same launch counts on the GPU: 1, 5, 8, 11 for pipe_sets 1..4).

    With pipe_sets 0 the frame runs as one set in two launches of 128, not one of
    256: the default three sets cap the chunk at max(128, ceil(256 / 8)) = 128
    before the "only from 1024 spp on" rule takes the sets back to one, and the
    cap stays.  One launch of 256 is what pipe_sets 1 gives, which is the case
    the GPU test pins."""
    one, zero, two, three, four = _plan(host_check, *(f"w=96,h=80,spp=256,{BOX},sets={k}" for k in (1, 0, 2, 3, 4)))
    for p in (one, zero):
        assert (p["quad"], p["drained"]) == (1, 1)   # 7,680 pixels <= resident lanes
        assert (p["refill"], p["leaf_kb"], p["wg_rows"], p["nset"]) == (4, 2, 8, 1)
    assert one["launches"] == [[0, 256]]
    assert zero["launches"] == [[0, 128], [0, 128]]
    assert [len(p["launches"]) for p in (two, three, four)] == [5, 8, 11]
    assert two["launches"] == [[0, 128], [0, 128], [1, 64], [1, 128], [1, 64]]
    assert two["order"] == [0, 2, 3, 1, 4]


def test_plan_chunked_and_exact_schedules(host_check):
    p, q, r = _plan(host_check, f"w=32,h=32,spp=12,spl=5,{BOX}", f"w=64,h=48,spp=8,sets=3,chunks=2,{BOX}",
                    f"w=96,h=40,spp=1024,sets=3,{BOX}")
    assert p["nset"] == 1 and _sets(p) == [[5, 5, 2]]
    assert (q["nset"], q["chunk"], len(q["launches"])) == (3, 4, 8)
    assert _sets(q) == [[4, 4], [3, 4, 1], [2, 4, 2]]
    assert r["nset"] == 1   # 40 rows < 3 sets x 16 band rows


def test_plan_pair_mode(host_check):
    p, q = _plan(host_check, f"w=1920,h=1080,spp=4096,lights=1,{BOX}",
                 f"w=1920,h=1080,spp=4096,lights=1,{BOX},flags=2")   # TPT_FLAG_REF_ORDER
    assert (p["pair"], p["pair_kernel"]) == (1, 1)
    assert (p["refill"], p["leaf_kb"], p["wg_rows"]) == (1, 1, 8)
    assert (p["nset"], p["chunk"], len(p["launches"])) == (3, 256, 50)
    assert _sets(p) == [[256] * 16, [171] + [256] * 15 + [85], [86] + [256] * 15 + [170]]
    assert (q["pair"], q["pair_kernel"]) == (1, 0)
    assert (q["refill"], q["leaf_kb"], q["wg_rows"]) == (16, 4, 16)   # the one-lane rules


def test_plan_xcd_runs(host_check):
    widths = (3840, 1920, 640, 256, 100)
    big = _plan(host_check, *(f"w={w},h=64,spp=8,faces=131072" for w in widths))
    assert [p["xcd_run"] for p in big] == [10, 5, 5, 2, 0]
    small = _plan(host_check, *(f"w={w},h=64,spp=8,faces=16384" for w in widths))
    assert [p["xcd_run"] for p in small] == [0] * 5


def test_plan_lane_mode_per_rank(host_check):
    """1920 wide, one rank's bands of 1080 rows (test_gpu_deal.py asserts the lane
    mode and `drained` per rank on the GPU)."""
    p8, p4, p2 = _plan(host_check, *(f"w=1920,h=1080,spp=1024,bc={n},bi=0,{BOX}" for n in (8, 4, 2)))
    assert [p["bh"] for p in (p8, p4, p2)] == [144, 272, 544]   # 9, 17 and 34 whole bands (an eighth is 135 rows)
    assert (p8["quad"], p8["drained"]) == (1, 1)                  # 276,480 pixels <= 327,680 resident lanes
    assert (p4["quad"], p4["pair"], p4["drained"]) == (0, 0, 1)   # 522,240 < twice the resident lanes
    assert (p2["quad"], p2["pair"], p2["drained"]) == (0, 0, 0)


def test_plan_explicit_deal(host_check):
    p, = _plan(host_check, f"w=96,h=96,spp=8,sets=2,chunks=2,list=5:1:3:0:2,{BOX}")
    assert p["nset"] == 2
    assert p["set_list"] == [[5, 3, 2], [1, 0]]
    assert p["set_rows"] == [48, 32]
    assert p["set_off"] == [5, 8]   # behind the whole list, back to back


def test_plan_argument_errors(host_check):
    a, b, c = _plan(host_check, f"w=64,h=64,spp=8,lanes=3,{BOX}", f"w=64,h=64,spp=8,lanes=4,lights=1,{BOX}",
                    f"w=64,h=1080,rows=1080,frames=65535,spp=8,lanes=1,{BOX}")
    assert a == {"status": 1, "message": "lanes_per_pixel: 0, 1, 2 or 4"}
    assert b == {"status": 1, "message": "lanes_per_pixel 4: scenes without delta lights, no env IS, ordered "
                                         "traversal, stacks in LDS"}
    assert c == {"status": 1, "message": "frame batch too large for one launch"}


def test_plan_invariants_random_sweep(host_check):
    """500 seeded random cases; the harness checks that every set's samples sum to
    spp, inner launches are whole chunks, the issue order is a permutation that
    keeps each set's order, the sets' rows sum to the call's and their shares
    partition an explicit list."""
    r = subprocess.run([host_check, "plan-sweep", "500", "20"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok plan sweep"), r.stdout + r.stderr[-3000:]
    assert int(r.stdout.split()[3]) >= 400   # (a few cases may end in an argument error)


def _variant(exe, *cases):
    """The k_trace variant space (common/trace_variant.hpp) through host_check.cpp
    variant_case: one dict per case."""
    return [json.loads(x) for x in run(exe, "variant", cases)]


def _picked(v):
    return (v["family"], v["deep"], v["lights"], v["mtl_lds"], v["wide_ids"], v["noemit"])


def test_variant_family_table(host_check):
    """What each family fixes, as the kernels were built before the table existed:
    (waves per workgroup, waves per SIMD of the launch bounds, waves per SIMD of the
    LDS budget, lanes per pixel, tile width, tile rows, env IS, ordered).  The first
    six rows are tpt_debug_trace_wg_waves' families in its order.  The reference
    order with env IS is compiled for 4 waves and budgets LDS for 5: recorded, not
    fixed.  82 variants exist per build."""
    t, = _variant(host_check, "table")
    assert t["families"] == [["lane", 1, 5, 5, 1, 16, 16, 0, 1], ["drain", 1, 4, 5, 1, 16, 16, 0, 1],
                             ["pair", 4, 4, 4, 2, 16, 8, 0, 1], ["is", 4, 4, 4, 1, 16, 16, 1, 1],
                             ["quad", 4, 4, 4, 4, 8, 8, 0, 1], ["ref", 4, 5, 5, 1, 16, 16, 0, 0],
                             ["is_pair", 4, 4, 4, 2, 16, 8, 1, 1], ["ref_is", 4, 4, 5, 1, 16, 16, 1, 0]]
    assert (t["public"], t["legal_keys"], t["round_trip"]) == (6, 82, 256)


def test_variant_selection(host_check):
    """select_trace_variant, the one rule launch_trace and the planner share.  A case
    starts box-like (no lights, 5 materials, 1,932 faces, depth 8, an emitter); the
    tuples are (family, deep, 5-word records, materials in LDS, 32-bit ids, NOEMIT)."""
    sel = lambda *cases: _variant(host_check, *("select=1," + c for c in cases))
    box, drained = sel("pair=0", "drained=1")
    assert _picked(box) == ("lane", 0, 0, 1, 0, 0) and _picked(drained) == ("drain", 0, 0, 1, 0, 0)
    assert all(v["legal"] == 1 for v in (box, drained))
    # ball-like: a delta light, no material table, no emitter / an emitter; pair is granted over drained
    noemit, emit, one = sel("pair=1,drained=1,lights=1,mtls=0,faces=5000,emitter=0",
                            "pair=1,lights=1,mtls=0,faces=5000", "pair=0,drained=1,lights=1,mtls=0,faces=5000")
    assert _picked(noemit) == ("pair", 0, 1, 1, 0, 1) and noemit["lanes"] == 2
    assert _picked(emit) == ("pair", 0, 1, 1, 0, 0)
    assert _picked(one) == ("drain", 0, 1, 1, 0, 0)
    # a pair request without shadow rays to hand off falls back to one lane
    assert _picked(sel("pair=1")[0]) == ("lane", 0, 0, 1, 0, 0)
    # env IS: 5-word records without lights, pair by request, never drained, before a quad request
    is1, is2, isq = sel("env_is=1,drained=1", "env_is=1,pair=1,emitter=0", "env_is=1,quad=1")
    assert _picked(is1) == ("is", 0, 1, 1, 0, 0) and (is1["env_is"], is1["lanes"]) == (1, 1)
    assert _picked(is2) == ("is_pair", 0, 1, 1, 0, 1) and (is2["env_is"], is2["lanes"]) == (1, 2)
    assert _picked(isq) == _picked(is1)
    # the reference order: one general variant, whatever else is asked
    ref, ref_is = sel("ref=1,pair=1,quad=1,drained=1,lights=1", "ref=1,env_is=1,pair=1,mtls=0,faces=6,depth=2")
    assert _picked(ref) == ("ref", 1, 1, 0, 1, 0) and _picked(ref_is) == ("ref_is", 1, 1, 0, 1, 0)
    # four lanes: one-lane records only
    quad, quad_lit, quad_m = sel("quad=1,drained=1", "quad=1,lights=1", "quad=1,mtls=32766")
    assert _picked(quad) == ("quad", 0, 0, 1, 0, 0) and quad["lanes"] == 4
    assert quad_lit == quad_m == {"error": "four lanes per pixel need 2-word path records"}
    # n_materials 0x7ffd / 0x7ffe: the packed records' last id; then 5 words and no pair
    m0, m1, p0, p1, i0, i1 = sel("mtls=32765", "mtls=32766", "mtls=32765,pair=1,lights=1", "mtls=32766,pair=1,lights=1",
                                 "mtls=32765,pair=1,env_is=1", "mtls=32766,pair=1,env_is=1")
    assert _picked(m0) == ("lane", 0, 0, 0, 0, 0) and _picked(m1) == ("lane", 0, 1, 0, 0, 0)
    assert _picked(p0) == ("pair", 0, 1, 0, 0, 0) and _picked(p1) == ("lane", 0, 1, 0, 0, 0)
    assert _picked(i0) == ("is_pair", 0, 1, 0, 0, 0) and _picked(i1) == ("is", 0, 1, 0, 0, 0)
    # TPT_MTL_LDS_MAX: 64 entries (n + the Material() slot) fit, 65 do not
    assert [v["mtl_lds"] for v in sel("mtls=62", "mtls=63", "mtls=64")] == [1, 1, 0]
    # 16-bit ids up to 65,535 nodes
    assert [v["wide_ids"] for v in sel("faces=32768", "faces=32769", "faces=32768,pair=1,lights=1",
                                       "faces=32769,pair=1,lights=1")] == [0, 1, 0, 1]
    assert [v["deep"] for v in sel("depth=1", "depth=8", "depth=9", "depth=64")] == [0, 0, 1, 1]


def test_variant_agrees_with_planner_random_sweep(host_check):
    """500 seeded random cases (plan-sweep's, plus four-lane requests, material and
    face counts on both sides of each rule, depths and emitters): for every plan
    that succeeds, pair_kernel says the selected variant runs two lanes per pixel,
    quad that it runs four, and wg_rows is its family's tile rows."""
    r = subprocess.run([host_check, "variant-sweep", "500", "20"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok variant sweep"), r.stdout + r.stderr[-3000:]
    assert int(r.stdout.split()[3]) >= 350
    seen = dict(x.split("=") for x in r.stdout.split("families")[1].split())
    assert all(int(n) > 0 for n in seen.values()), seen   # every family was reached


# (case, (bytes, material offset, stack offset, record offset, LDS stack slots, LDS record levels)): rows of
# the layout the kernels ran with before trace_lds_layout moved out of trace.hip, from a sweep in which the
# two agreed everywhere (stack depth 1..160, max_depth 1..64, 0..200 materials, every variant, 1 / 2 / 4 waves,
# with and without caps)
LAYOUT_PINS = [
    # box at one wave: the share of 5 waves per SIMD less the 512-byte slack; 26 of its 27 slots
    ("family=lane,mtl_lds=1,wgw=1,stack=24,depth=8,mtls=5", (7680, 0, 256, 3584, 26, 8)),
    ("family=lane,mtl_lds=1,wgw=4,stack=24,depth=8,mtls=5", (30976, 0, 256, 14592, 27, 8)),
    ("family=lane,mtl_lds=1,wgw=1,stack=24,depth=64,mtls=5", (7680, 0, 256, 2048, 14, 11)),
    ("family=drain,lights=1,mtl_lds=1,wgw=1,stack=24,depth=8,mtls=5", (7680, 0, 256, 2560, 18, 4)),
    # the 5-word pair layout: records for half the lanes
    ("family=pair,lights=1,mtl_lds=1,wgw=4,stack=31,depth=8,mtls=0", (38016, 0, 128, 17536, 34, 8)),
    ("family=pair,lights=1,mtl_lds=1,wide_ids=1,wgw=4,stack=41,depth=32,mtls=0", (40576, 0, 128, 12416, 12, 11)),
    # a deep tree: the stack's deepest slots spill to private memory
    ("family=lane,mtl_lds=1,wgw=1,stack=120,depth=8,mtls=1", (7552, 0, 128, 3456, 26, 8)),
    ("family=lane,mtl_lds=1,wgw=1,stack=120,depth=64,mtls=1", (7552, 0, 128, 1920, 14, 11)),
    # the reference order with env IS: a fifth of the CU's LDS (32,768 B), though compiled for 4 waves
    ("family=ref_is,lights=1,wide_ids=1,wgw=4,stack=40,depth=64,mtls=5", (32768, 0, 0, 12288, 12, 4)),
    ("family=ref,lights=1,wide_ids=1,wgw=4,stack=40,depth=8,mtls=5", (32768, 0, 0, 12288, 12, 4)),
    ("family=is,lights=1,mtl_lds=1,wgw=4,stack=31,depth=8,mtls=63", (40960, 0, 2048, 10240, 16, 6)),
    ("family=is_pair,lights=1,wgw=4,stack=31,depth=8,mtls=64", (37888, 0, 0, 17408, 34, 8)),
    ("family=quad,mtl_lds=1,wgw=4,stack=24,depth=8,mtls=5", (20224, 0, 256, 3840, 27, 8)),
    ("family=quad,mtl_lds=1,wgw=4,stack=120,depth=64,mtls=5", (39168, 0, 256, 2304, 14, 18)),
    ("family=lane,wide_ids=1,wgw=1,stack=41,depth=8,mtls=200", (7680, 0, 0, 3584, 14, 8)),
    ("family=lane,mtl_lds=1,wgw=2,stack=24,depth=8,mtls=5,max_slots=20,max_levels=3", (8448, 0, 256, 5376, 20, 3)),
]


def test_variant_lds_layout_pinned(host_check):
    got = _variant(host_check, *("layout=1," + c for c, _ in LAYOUT_PINS))
    for (case, want), g in zip(LAYOUT_PINS, got):
        assert (g["bytes"], g["mtl_offset"], g["stack_offset"], g["rec_offset"], g["stack_slots"],
                g["rec_levels"]) == want, case


def test_wide_tree_pool_under_tsan():
    """The builder's task pool (chunked binning and scatter, subtree tasks,
    the parallel breadth-first collapse) under ThreadSanitizer, 4 and 8
    threads, each compared byte for byte with the serial build."""
    if not os.path.isdir(SAN) or shutil.which("g++") is None:
        pytest.skip("sanitizer harness not present (GPU box) or no g++")
    r = _make("host_check_tsan")
    if r.returncode != 0:
        if "tsan" in r.stderr.lower() or "sanitize" in r.stderr.lower():
            pytest.skip("toolchain without the TSan runtime")
        raise AssertionError(r.stderr)
    exe = os.path.join(SAN, "host_check_tsan")
    for threads in (4, 8):
        r = subprocess.run([exe, "wide", "40000", "7", str(threads)], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1"))
        assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr[-4000:]
