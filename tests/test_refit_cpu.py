"""tpt_scene_refit without a GPU: the numpy restatement (tests/refit_ref.py) against the host tree
builder's own output, its teeth, tpt_wide_tree_levels, and the ray sets the GPU tests trace
(tests/refit_cases.py): almost none of their rays is a near-tie."""
import ctypes as C

import numpy as np
import pytest

import tinypathtracer_amd as T

from tests import refit_cases as RC
from tests import refit_ref as RR

F = np.float32
SIZES = (2, 3, 5, 130, 2000)


def boxes(n, seed):
    """n random finite leaf boxes [n, 6] (min.xyz, max.xyz) and emitter flags, a third of them set."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-10.0, 10.0, (n, 3))
    h = rng.uniform(0.0, 1.0, (n, 3)) ** 3
    h[rng.uniform(size=(n, 3)) < 0.05] = 0.0              # flat boxes: axis-aligned triangles
    b = np.concatenate([c - h, c + h], -1).astype(F)
    return b, (rng.uniform(size=n) < 0.33).astype(np.uint32)


def build(leaf_box, emit):
    n = len(leaf_box)
    nodes = np.zeros((max(n - 1, 1), 32), F)
    need = C.c_int32(0)
    n4 = T.lib().tpt_wide_tree_build(n, leaf_box.ctypes.data, emit.ctypes.data, nodes.ctypes.data, len(nodes),
                                     C.byref(need), 1)
    assert 0 < n4 <= len(nodes)
    return nodes[:n4].copy()


@pytest.fixture(scope="module", params=SIZES)
def tree(request):
    n = request.param
    b, e = boxes(n, 100 + n)
    return n, b, e, build(b, e)


def same_tree(a, b):
    """Floats with ==, so +0 and -0 agree (min/max operand order differs between SSE and the GPU);
    links bit for bit."""
    return bool((a[:, :24] == b[:, :24]).all() and np.array_equal(RR.links(a), RR.links(b)) and
                np.array_equal(a[:, 28:].view(np.uint32), b[:, 28:].view(np.uint32)))


def check_exact(nodes, leaf_box, leaf_base, id_base=0):
    """Every leaf child box is its leaf's box bit for bit, every inner child box the exact union
    of the child boxes of the node it names.  Returns the number of violations."""
    ids = RR.child_ids(nodes)
    bad = 0
    for i in range(len(nodes)):
        for k in range(4):
            c = ids[i, k]
            if c < 0:
                continue
            got = nodes[i, 6 * k:6 * k + 6]
            if c >= leaf_base:
                bad += not np.array_equal(got.view(np.uint32), leaf_box[c - leaf_base].view(np.uint32))
            else:
                bad += not (got == RR.node_union(nodes[c - id_base], ids[c - id_base])).all()
    return bad


def test_refit_of_the_builders_output_is_the_identity(tree):
    n, b, e, nodes = tree
    assert check_exact(nodes, b, n - 1) == 0               # the builder's inner boxes are exact unions
    assert same_tree(RR.refit_wide(nodes, b, n - 1, 0), nodes)


def perturbed(b, seed):
    rng = np.random.default_rng(seed)
    c = rng.normal(scale=0.7, size=(len(b), 3))
    g = rng.uniform(0.5, 1.5, (len(b), 3))
    mid, half = 0.5 * (b[:, :3] + b[:, 3:]) + c, 0.5 * (b[:, 3:] - b[:, :3]) * g
    return np.concatenate([mid - half, mid + half], -1).astype(F)


def test_refit_with_moved_leaves(tree):
    n, b, e, nodes = tree
    nb = perturbed(b, 7 + n)
    out = RR.refit_wide(nodes, nb, n - 1, 0)
    assert check_exact(out, nb, n - 1) == 0
    assert not same_tree(out, nodes)
    assert np.array_equal(RR.links(out), RR.links(nodes))
    assert check_exact(nodes, nb, n - 1) > 0               # the stale tree is seen


def test_grow_only_refit_fails_the_exact_union_check(tree):
    """Teeth: uniting every box with the one it had keeps a valid (looser) tree, which the check
    must refuse."""
    n, b, e, nodes = tree
    nb = perturbed(b, 7 + n)
    assert check_exact(RR.grow_only(nodes, nb, n - 1, 0), nb, n - 1) > 0


def c_levels(nodes, id_base=0, cap=None):
    cap = len(nodes) + 2 if cap is None else cap
    out = np.full(cap, -7, np.int32)
    lv = T.lib().tpt_wide_tree_levels(nodes.ctypes.data, len(nodes), id_base, out.ctypes.data, cap)
    return lv, out


def test_levels_against_the_reference(tree):
    n, b, e, nodes = tree
    lv, out = c_levels(nodes)
    want = RR.levels(nodes, 0)
    assert lv == len(want) - 1 and list(out[:lv + 1]) == want and (out[lv + 1:] == -7).all()
    begin = out[:lv + 1]
    assert begin[0] == 0 and begin[1] == 1 and begin[-1] == len(nodes) and (np.diff(begin) > 0).all()   # a partition
    ids = RR.child_ids(nodes)
    for l in range(lv):
        kids = ids[begin[l]:begin[l + 1]]
        kids = kids[(kids >= 0) & (kids < len(nodes))]
        if l + 1 < lv:
            assert ((kids >= begin[l + 1]) & (kids < begin[l + 2])).all()
        else:
            assert len(kids) == 0
    if n >= 130:
        assert lv >= 3                                       # several levels


def test_levels_with_an_id_base_and_refusals(tree):
    n, b, e, nodes = tree
    base = 11
    moved = nodes.copy()
    l = RR.links(nodes).copy()
    inner = (l >= 0) & ((l & RR.ID_MASK) < len(nodes))
    leaf = (l >= 0) & ~inner
    l[inner] += base
    l[leaf] += 2 * base                                      # leaf ids stay past the nodes'
    moved[:, 24:28] = l.view(F)
    lv, out = c_levels(moved, base)
    assert lv == len(RR.levels(nodes, 0)) - 1 and list(out[:lv + 1]) == RR.levels(moved, base)
    # too small a buffer: the count comes back, nothing is written
    lv2, small = c_levels(nodes, 0, cap=lv)
    assert lv2 == lv and (small == -7).all()
    assert T.lib().tpt_wide_tree_levels(None, 4, 0, None, 0) == -1
    assert T.lib().tpt_wide_tree_levels(nodes.ctypes.data, 0, 0, None, 0) == -1
    if len(nodes) >= 3:                                      # a link upwards: not numbered level by level
        bad = nodes.copy()
        lb = RR.links(bad).copy()
        k = int(np.flatnonzero(inner[0])[0])
        lb[0, k] = (lb[0, k] & ~RR.ID_MASK) | 0              # the root names itself
        bad[:, 24:28] = lb.view(F)
        assert c_levels(bad)[0] == -1


def test_cost_of_a_two_leaf_tree():
    b = np.array([[0, 0, 0, 1, 1, 1], [2, 0, 0, 3, 2, 1]], F)
    nodes = build(b, np.zeros(2, np.uint32))
    assert len(nodes) == 1
    # areas 6 and 10 over the union's (3 x 2 x 1: 22)
    assert RR.cost(nodes) == pytest.approx(16.0 / 22.0, rel=1e-15)


@pytest.mark.parametrize("name", RC.SCENES)
def test_ray_sets_hold_few_near_ties(name):
    """Brute force in float64: fewer than 1 % of a set's rays have their two nearest hits within
    1e-4 relative of each other, for every scene and pose the GPU tests use; and the sets hit and
    miss."""
    o, d = RC.rays(name)
    assert 3900 <= len(o) <= 4100
    for pose in (None,) + tuple(RC.scene(name)["poses"]) + tuple(RC.scene(name).get("matrices", {})):
        keep = RC.usable(name, pose)
        dropped = 1.0 - keep.mean()
        print(f"{name} {pose}: {len(o)} rays, {100 * dropped:.3f} % dropped")
        assert dropped < 0.01
        t1, _ = RC.nearest(name, pose)
        assert 0.05 < np.isfinite(t1).mean() < 0.999
