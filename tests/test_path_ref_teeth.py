"""Does tests/path_ref.py have teeth?  Each rule of tpt_render_aov_path's definition is
knocked out of the restatement in turn; on the comparable pixels the GPU parity test looks
at, the buffers must then move by far more than that test's bounds (equal bits for face,
material, bounces and albedo; 1e-4 for depth and normal).  CPU only."""
import numpy as np
import pytest

from tests import path_ref as P
from tests import path_scenes as S
from tests import variant_scenes as V

W, H, CAP = 128, 72, 3
BOUND = 1e-4                                               # test_gpu_aov_path's depth and normal bound


@pytest.fixture(scope="module")
def tinted():
    ps = V.oracle_scene(S.scene("tinted"))
    tr = P.Tracer(ps)
    ref = P.oracle_aov_path(ps, W, H, CAP, tracer=tr)
    return ps, tr, ref, P.comparable(ref)


def _rel_depth(a, b, where):
    return np.abs(a["depth"][where].astype(np.float64) - b["depth"][where]) / b["depth"][where]


def test_albedo_is_the_product(tinted):
    ps, tr, ref, ok = tinted
    bad = P.oracle_aov_path(ps, W, H, CAP, knock="no_product", tracer=tr)
    followed = ok & (ref["bounces"] > 0) & (ref["face"] >= 0)   # (after one mirror and a miss the product is its tint alone)
    moved = (bad["albedo"] != ref["albedo"]).any(-1)
    d = np.abs(bad["albedo"][followed] - ref["albedo"][followed]).max()
    print(f"no product: {(moved & followed).sum()} of {followed.sum()} comparable followed pixels with a terminal "
          f"hit move, max {d:.3f}")
    assert (moved & followed).sum() >= 100 and d >= 0.5    # the GPU test asks for equal bits
    assert not (moved & ok & (ref["bounces"] == 0)).any()


def test_depth_is_the_whole_path(tinted):
    ps, tr, ref, ok = tinted
    bad = P.oracle_aov_path(ps, W, H, CAP, knock="last_depth", tracer=tr)
    followed = ok & (ref["bounces"] > 0) & (ref["face"] >= 0)
    rel = _rel_depth(bad, ref, followed)
    print(f"last hop's depth: least relative change {rel.min():.3f} over {followed.sum()} pixels")
    assert followed.sum() >= 300 and rel.min() >= 1000 * BOUND


def test_reflection_uses_the_shading_normal():
    """On `tinted` the walls are flat and their vertex normals the planes', so the two
    normals agree to rounding; `tilted` tilts the walls' vertex normals (same geometry)."""
    ps = V.oracle_scene(S.scene("tilted"))
    tr = P.Tracer(ps)
    ref = P.oracle_aov_path(ps, W, H, CAP, tracer=tr)
    bad = P.oracle_aov_path(ps, W, H, CAP, knock="geo_normal", tracer=tr)
    ok = P.comparable(ref) & (ref["bounces"] > 0)
    hit = ok & (ref["face"] >= 0) & (bad["face"] >= 0)
    face_moved = (bad["face"] != ref["face"]) & ok
    rel = _rel_depth(bad, ref, hit)
    print(f"geometric normal: {face_moved.sum()} of {ok.sum()} comparable followed pixels change face, "
          f"median relative depth change {np.median(rel):.3e}")
    assert ok.sum() >= 300 and np.median(rel) >= 100 * BOUND


def test_emitter_is_terminal():
    ps = V.oracle_scene(S.scene("lamp_mirror"))
    tr = P.Tracer(ps)
    ref = P.oracle_aov_path(ps, W, H, 8, tracer=tr)
    bad = P.oracle_aov_path(ps, W, H, 8, knock="emitter", tracer=tr)
    # (the lamp is seen at a grazing angle: 4 of its 82 pixels have a uniform face around them, 24 a
    # uniform material, which is what decides here)
    first = P.uniform3x3(ref["first_material"]) & (ref["first_material"] == S.emitter_ids(ps.src)[0])
    print(f"emitter not terminal: {first.sum()} emitter pixels with the emitter all around, all followed")
    assert first.sum() >= 10
    assert (ref["bounces"][first] == 0).all() and (bad["bounces"][first] >= 1).all()
    assert (bad["face"][first] != ref["face"][first]).all()


def test_cap_is_exact():
    """Cap 2: 37 comparable pixels end on a mirror at the cap (cap 3: 29 pixels, none comparable)."""
    ps = V.oracle_scene(S.scene("tinted"))
    tr = P.Tracer(ps)
    cap = 2
    ref = P.oracle_aov_path(ps, W, H, cap, tracer=tr)
    bad = P.oracle_aov_path(ps, W, H, cap, knock="cap", tracer=tr)
    assert ref["bounces"].max() == cap and bad["bounces"].max() == cap + 1
    moved = P.comparable(ref) & (bad["bounces"] != ref["bounces"])
    assert (ref["bounces"][moved] == cap).all() and P.is_mirror(tr.mtl)[ref["material"][moved]].all()
    rel = _rel_depth(bad, ref, moved)
    print(f"cap + 1: {moved.sum()} comparable capped pixels go on, least relative depth change {rel.min():.3f}")
    assert moved.sum() >= 20 and rel.min() >= 100 * BOUND
