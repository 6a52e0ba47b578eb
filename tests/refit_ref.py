"""tpt_scene_refit in numpy (tests/test_refit_cpu.py, test_gpu_refit.py; DESIGN.md section 5 "BVH
refit"): the boxes of a kept topology from new leaf boxes, the tree cost, the level ranges.

Nodes are [n, 32] float32 in the inner4 layout (device_api.hpp): child k's box in columns
6k..6k+5 (min.xyz, max.xyz), the four child links as the int32 bits of columns 24..27 (-1: none;
bit 30: the child's subtree holds an emitter; the rest: an id -- below leaf_base a node's, counted
from id_base for the tree's own first node; from leaf_base on the leaf at position id - leaf_base).
A tree is numbered breadth-first, so a node's inner children have larger ids than it has."""
import numpy as np

F = np.float32
ID_MASK = (1 << 30) - 1


def links(nodes):
    return np.ascontiguousarray(nodes[:, 24:28]).view(np.int32)


def child_ids(nodes):
    """The links' ids, -1 where there is no child."""
    l = links(nodes)
    return np.where(l < 0, -1, l & ID_MASK)


def union(boxes):
    """The exact min/max union of [m, 6] boxes."""
    return np.concatenate([boxes[:, :3].min(0), boxes[:, 3:].max(0)]).astype(F)


def node_union(node, ids):
    """The union of the child boxes a node has."""
    return union(np.stack([node[6 * k:6 * k + 6] for k in range(4) if ids[k] >= 0]))


def refit_wide(nodes, leaf_box, leaf_base, id_base):
    """The tree with every child box recomputed from leaf_box ([positions, 6], by position): a
    leaf child takes its leaf's box bit for bit, an inner child the exact union of the child boxes
    of the node it names; an unused slot, the links and the padding stay.  Bottom-up: in a
    breadth-first numbering that is by descending id."""
    out = np.array(nodes, F, copy=True)
    ids = child_ids(out)
    n = len(out)
    for i in range(n - 1, -1, -1):
        for k in range(4):
            c = ids[i, k]
            if c < 0:
                continue
            if c >= leaf_base:
                out[i, 6 * k:6 * k + 6] = leaf_box[c - leaf_base]
            else:
                j = c - id_base
                assert i < j < n, "not numbered breadth-first"
                out[i, 6 * k:6 * k + 6] = node_union(out[j], ids[j])
    return out


def grow_only(nodes, leaf_box, leaf_base, id_base):
    """What refit_wide must not be: every box united with the one it had (still a valid tree, a
    looser one).  The tests' teeth."""
    new = refit_wide(nodes, leaf_box, leaf_base, id_base)
    old = np.asarray(nodes, F)
    out = new.copy()
    ids = child_ids(old)
    for k in range(4):
        has = ids[:, k] >= 0
        out[has, 6 * k:6 * k + 3] = np.minimum(new[has, 6 * k:6 * k + 3], old[has, 6 * k:6 * k + 3])
        out[has, 6 * k + 3:6 * k + 6] = np.maximum(new[has, 6 * k + 3:6 * k + 6], old[has, 6 * k + 3:6 * k + 6])
    return out


def refit_lbvh(nodes36, leaf_box_by_position):
    """The LBVH's node boxes [2F - 1, 6] from the leaves' (tinypathtracer_amd.NODE_DTYPE nodes as
    tpt_scene_read_bvh returns them: ids below F - 1 are inner nodes with the children a and b,
    id F - 1 + p is the leaf at position p): every inner box the exact union of its two children's."""
    nn = len(nodes36)
    nint = (nn - 1) // 2
    box = np.zeros((nn, 6), F)
    box[nint:] = leaf_box_by_position
    done = np.zeros(nn, bool)
    done[nint:] = True
    lc = nodes36["a"].astype(np.int64)
    rc = nodes36["b"].astype(np.int64)
    todo = list(range(nint))
    while todo:
        rest = []
        for i in todo:
            if done[lc[i]] and done[rc[i]]:
                box[i] = union(np.stack([box[lc[i]], box[rc[i]]]))
                done[i] = True
            else:
                rest.append(i)
        assert len(rest) < len(todo), "the links hold a cycle"
        todo = rest
    return box


def area(box):
    """wide_bvh.cpp Box::area in float64: 0 for an inverted extent."""
    d = box[..., 3:6].astype(np.float64) - box[..., 0:3].astype(np.float64)
    a = 2.0 * (d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0])
    return np.where((d >= 0).all(-1), a, 0.0)


def cost(nodes):
    """tpt_refit_stats.cost: the summed areas of every child box of every node over the area of the
    union of the root's child boxes, in float64."""
    ids = child_ids(nodes)
    total = 0.0
    for k in range(4):
        total += float(area(nodes[:, 6 * k:6 * k + 6])[ids[:, k] >= 0].sum())
    return total / float(area(node_union(nodes[0], ids[0])))


def levels(nodes, id_base):
    """The level ranges: level l is the nodes [begin[l], begin[l + 1]), the root alone in level
    0; found by walking down from the root, one level's inner children making the next."""
    ids = child_ids(nodes)
    n = len(nodes)
    inner = (ids >= id_base) & (ids < id_base + n)
    begin = [0, 1]
    lo, hi = 0, 1
    while True:
        kids = np.sort((ids[lo:hi][inner[lo:hi]] - id_base).ravel())
        if len(kids) == 0:
            break
        assert kids[0] == hi and (np.diff(kids) == 1).all(), "a level is not one run of ids"
        lo, hi = hi, int(kids[-1]) + 1
        begin.append(hi)
    assert hi == n
    return begin
