"""In-memory scenes that put the hosts on the far side of the launch rules the
shipped scenes never cross (tests/test_variant_scenes_cpu.py states the
conditions on the CPU, tests/test_gpu_variants.py runs the device against the
oracle on them; DESIGN.md section 4 "Parity" lists which rule each one is for).

A scene here is one oracle.scene.OracleScene -- one set of numpy arrays, with the
lights as dicts -- and both hosts are made from it: device_scene() the product's
tinypathtracer_amd.Scene, oracle_scene() the oracle's PackedScene.  Every builder
is deterministic and writes no file.

  with_materials(base, n)  a shipped scene with its material table grown to n
                           entries, the real materials at the highest ids;
  with_inf_vertex(base)    plus one unhittable triangle with a +inf vertex;
  chain(direction, inf)    61 triangles whose LBVH is a chain of depth 60;
  faces_exactly(n)         box subdivided twice plus small triangles, n faces;
  tiny(n)                  1, 2 or 3 triangles.
"""
import copy
import os

import numpy as np

from oracle import oracle as O
from oracle import scene as oscene
from tests.conftest import SCENE_DIR

F = np.float32
_IDENTITY = np.eye(4, dtype=F).reshape(16)


def base_scene(name) -> oscene.OracleScene:
    """A shipped scene's packed arrays (the oracle's loader; tests/test_loader_abi.py
    pins the native loader to the same arrays)."""
    return oscene.load_gltf(os.path.join(SCENE_DIR, f"{name}.gltf"))


def device_scene(s: oscene.OracleScene):
    import tinypathtracer_amd as T
    cam = T.Camera(np.asarray(s.camera_c2w, F).copy(), float(s.vfov), float(s.aspect), float(s.znear))
    return T.Scene.from_arrays(s.indices, s.vertices, s.normals, s.lut, s.vert_trans, s.normal_trans, s.materials,
                               s.lights, cam)


def oracle_scene(s: oscene.OracleScene) -> O.PackedScene:
    return O.PackedScene(s)


def _scene(indices, vertices, normals, lut, vert_trans, normal_trans, materials, lights, like=None, camera=None):
    c2w, vfov, aspect, znear = camera if camera is not None else (like.camera_c2w, like.vfov, like.aspect, like.znear)
    materials = np.asarray(materials, F).reshape(-1, 15)
    return oscene.OracleScene(
        indices=np.ascontiguousarray(indices, np.uint32).reshape(-1),
        vertices=np.ascontiguousarray(vertices, F).reshape(-1, 3),
        normals=np.ascontiguousarray(normals, F).reshape(-1, 3),
        lut=np.ascontiguousarray(lut, np.int32).reshape(-1, 2),
        vert_trans=np.ascontiguousarray(vert_trans, F).reshape(-1, 16),
        normal_trans=np.ascontiguousarray(normal_trans, F).reshape(-1, 16),
        materials=materials, material_names=[f"m{i}" for i in range(len(materials))],
        lights=copy.deepcopy(list(lights)), camera_c2w=np.asarray(c2w, F).reshape(16).copy(), vfov=F(vfov),
        aspect=F(aspect), znear=F(znear), missing_material=len(materials) == 0)


def material_row(base_color, emission=0.0, **kw):
    m = dict(oscene.MATERIAL_DEFAULT, base_color=tuple(F(c) for c in base_color), emission_factor=F(emission))
    m.update({k: F(v) for k, v in kw.items()})
    return np.array(list(m["base_color"]) + [m[k] for k in oscene.MATERIAL_FIELDS[1:]], F)


# --------------------------------------------------------------------------
# many materials
# --------------------------------------------------------------------------
def decoy_materials(n):
    """n rows no shipped material equals: saturated colours off the shipped ones'
    grid, and an emission (0.375) no shipped material has (theirs are 0 or 6)."""
    i = np.arange(n, dtype=np.float64)
    rows = np.tile(material_row((0, 0, 0), 0.375), (n, 1))
    rows[:, 0] = (0.031 + 0.937 * ((i * 0.6180339887) % 1.0)).astype(F)
    rows[:, 1] = (0.043 + 0.911 * ((i * 0.7548776662) % 1.0)).astype(F)
    rows[:, 2] = (0.057 + 0.893 * ((i * 0.5698402910) % 1.0)).astype(F)
    return rows.astype(F)


def with_materials(base, n, layout="top"):
    """`base` (a shipped scene's name, or an OracleScene) with a material table of
    n entries.  layout "top": the materials the objects use keep their values and
    move to the highest ids in their old order, except that an emissive one goes
    to the very top (id n - 1: the largest probe id a path record packs); every
    other slot is a decoy (decoy_materials).  An object without a material (it
    takes the Material() slot, id == the table's size) keeps taking it: its id
    becomes n.  The frame must not change by a bit."""
    if layout != "top":
        raise ValueError(layout)
    s = base_scene(base) if isinstance(base, str) else base
    old = np.asarray(s.materials, F).reshape(-1, 15)
    used = sorted({int(m) for m in s.lut[:, 1] if 0 <= int(m) < len(old)})
    order = [m for m in used if old[m, 3] == 0.0] + [m for m in used if old[m, 3] != 0.0]   # emitters last
    if n < len(order):
        raise ValueError(f"{len(order)} materials in use, table of {n}")
    mats = decoy_materials(n)
    for row in mats[:n - len(order)]:
        assert not any(np.array_equal(row[:3], o[:3]) or row[3] == o[3] for o in old), "a decoy equals a real material"
    new_id = {}
    for k, m in enumerate(order):
        new_id[m] = n - len(order) + k
        mats[new_id[m]] = old[m]
    lut = s.lut.copy()
    lut[:, 1] = [new_id.get(int(m), n) for m in s.lut[:, 1]]
    out = _scene(s.indices, s.vertices, s.normals, lut, s.vert_trans, s.normal_trans, mats, s.lights, like=s)
    out.meta = {"real_ids": sorted(new_id.values()), "n_decoys": n - len(order)}
    return out


def remap_materials(s, f):
    """The scene with every object's material id m replaced by f(m): what a device
    that truncated or wrapped the id would render."""
    out = copy.copy(s)
    out.lut = s.lut.copy()
    out.lut[:, 1] = [f(int(m)) for m in s.lut[:, 1]]
    return out


# --------------------------------------------------------------------------
# a non-finite node box
# --------------------------------------------------------------------------
def with_inf_vertex(base):
    """`base` plus one triangle with a vertex at (+inf, +inf, +inf), in an object of
    its own (the last) that shares the last object's material.  Its matrix has no
    zero and no negative entry in its upper 3x3, so the world vertex is +inf in
    every coordinate on either host -- a matrix with a zero there would make it
    NaN (0 * inf), whose sign and payload are the arithmetic unit's.  The leaf box
    and every box above it are non-finite (max = +inf).  No ray can hit it:
    Moller-Trumbore's t for an infinite edge is NaN, and NaN < t_best is false."""
    s = base_scene(base) if isinstance(base, str) else base
    nv = len(s.vertices)
    verts = np.concatenate([s.vertices, np.array([[0.125, 0.25, 0.5], [0.5, 0.125, 0.25], [np.inf] * 3], F)])
    norms = np.concatenate([s.normals, np.tile(np.array([[0.0, 0.0, 1.0]], F), (3, 1))])
    idx = np.concatenate([s.indices, np.array([nv, nv + 1, nv + 2], np.uint32)])
    lut = np.concatenate([s.lut, np.array([[s.n_faces, s.lut[-1, 1]]], np.int32)])
    m = np.array([1, 0.5, 0.25, 0, 0.25, 1, 0.5, 0, 0.5, 0.25, 1, 0, 0.125, 0.125, 0.125, 1], F)
    vt = np.concatenate([s.vert_trans, m[None]])
    nt = np.concatenate([s.normal_trans, _IDENTITY[None]])
    return _scene(idx, verts, norms, lut, vt, nt, s.materials, s.lights, like=s)


# --------------------------------------------------------------------------
# a chain-shaped LBVH
# --------------------------------------------------------------------------
CHAIN_DEPTH = 60
_CHAIN_R = F(256.0)
_CHAIN_B = 2.0 ** -12      # one step of the Morton quantisation (floatTo21Int keeps 2^-12 below 256)


def chain_centres(direction):
    """61 box centres whose Morton keys are K, K + 2^0 .. K + 2^59 ("up") or
    K', K' - 2^0 .. K' - 2^59 ("down"): the base centre b * (1, 1, 1), and one per
    axis and k = 0..19 with that coordinate b * (1 + 2^k); "down" mirrors them
    through the base centre to 0 and -b * 2^k.  A coordinate m * b quantises to
    2^20 - 1 + m, so "up" sets one more bit of 2^20 and "down" clears one bit of
    2^20 - 1, and every inner node of the LBVH splits one leaf off the rest."""
    c = [(1, 1, 1)]
    for k in range(20):
        for ax in range(3):
            m = [1, 1, 1]
            m[ax] = 1 + 2 ** k
            c.append(tuple(m))
    c = np.array(c, np.float64)
    if direction == "down":
        c = -(c - 1.0)
    elif direction != "up":
        raise ValueError(direction)
    return (c * _CHAIN_B).astype(F)


def chain(direction, inf=False):
    """61 triangles whose LBVH has depth 60 (chain_centres).  Triangle i has the
    corners c_i - R and c_i + R (R = 256: both exact, so the box centre is c_i
    exactly, and all 61 boxes share a cube 384 across: [-128, 256]^3 for "up",
    [-256, 128]^3 for "down") and a third vertex
    c_i + R * w_i inside that box, the w_i a fan of 61 directions round the
    diagonal: 61 distinct planes, large well-shaped triangles that cross near the
    diagonal.  Material 1 (every fourth triangle) emits.  A right-first walk
    defers the lone leaf at every level of "down" and the inner child at every
    level of "up".  inf=True: with_inf_vertex's triangle on top, so no wide tree
    exists and every ordered walk is the binary one."""
    c = chain_centres(direction).astype(np.float64)
    n = len(c)
    u = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)
    v = np.array([1.0, 1.0, -2.0]) / np.sqrt(6.0)
    # golden-angle order: neighbours in key order are far apart in the fan
    th = 2.0 * np.pi * ((np.arange(n) * 0.6180339887 + 0.05) % 1.0)
    w = 0.85 * (np.cos(th)[:, None] * u + np.sin(th)[:, None] * v)
    R = float(_CHAIN_R)
    verts = np.stack([c - R, c + R, c + R * w], 1).astype(F)               # [n, 3, 3]
    assert np.array_equal(F(0.5) * (verts[:, 0] + verts[:, 1]), c.astype(F))
    assert (verts[:, 2] > verts[:, 0]).all() and (verts[:, 2] < verts[:, 1]).all()
    nrm = np.cross(verts[:, 1].astype(np.float64) - verts[:, 0], verts[:, 2].astype(np.float64) - verts[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    normals = np.repeat(nrm.astype(F), 3, axis=0)
    idx = np.arange(3 * n, dtype=np.uint32)
    lut = np.array([[i, 1 if i % 4 == 0 else 0] for i in range(n)], np.int32)   # one object per triangle
    mats = np.stack([material_row((0.8, 0.8, 0.8)), material_row((1.0, 1.0, 1.0), 4.0)])
    ident = np.tile(_IDENTITY, (n, 1))
    # the camera looks across the diagonal at the fan's middle: its rays cross the boxes' common region
    eye = np.array([64.0, 64.0, 64.0]) + 400.0 * u
    s = _scene(idx, verts.reshape(-1, 3), normals, lut, ident, ident, mats, [],
               camera=(look_at(eye, (64.0, 64.0, 64.0), v), 1.1, 16.0 / 9.0, 0.1))
    return with_inf_vertex(s) if inf else s


def look_at(eye, target, up):
    """Column-major camera-to-world matrix: the camera looks along its -z."""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    z = eye - target
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
    return m.T.astype(F).reshape(16)   # rows of m.T = columns of the matrix


def tree_depth(nodes):
    """The deepest leaf's distance from the root, from the oracle's parent links."""
    parent = nodes["parent"].astype(np.int64)
    cur = np.arange(len(nodes))
    depth = 0
    while (cur != 0).any():
        cur = np.where(cur != 0, parent[cur], 0)
        depth += 1
        assert depth <= len(nodes), "a parent chain misses the root"
    return depth


def box_hits(nodes, origins, dirs):
    """rayHitBBox (geometry_queries.h:18-46) of every ray against every node's box,
    float32 in the reference's order of operations: bool [rays, nodes]."""
    o = np.asarray(origins, F)[:, None, :]
    with np.errstate(all="ignore"):
        inv = (F(1.0) / np.asarray(dirs, F))[:, None, :]
        a = (nodes["bmin"][None] - o) * inv
        b = (nodes["bmax"][None] - o) * inv
    lo, hi = np.where(a > b, b, a), np.where(a > b, a, b)
    t0 = np.full(lo.shape[:2], -np.finfo(F).max, F)
    t1 = np.full(lo.shape[:2], np.finfo(F).max, F)
    ok = np.ones(lo.shape[:2], bool)
    for k in range(3):
        ok &= ~((t0 > hi[..., k]) | (lo[..., k] > t1))
        t0 = np.where(t0 > lo[..., k], t0, lo[..., k])
        t1 = np.where(t1 < hi[..., k], t1, hi[..., k])
    return ok


def dfs_max_occupancy(nodes, n_faces, origins, dirs):
    """The reference's traverseBVH (path_tracer.cu:61-107) restated for its stack
    alone: pop a node; an inner node pushes its left child, then its right child,
    each if the ray passes its box -- so the right child is visited first and the
    left one waits.  Returns per ray the largest number of entries the stack held."""
    hits = box_hits(nodes, origins, dirs)
    left, right = nodes["a"], nodes["b"]
    out = np.zeros(len(hits), np.int64)
    for r in range(len(hits)):
        h = hits[r]
        stack, most = [0], 1
        while stack:
            cur = stack.pop()
            if cur >= n_faces - 1:
                continue
            for child in (int(left[cur]), int(right[cur])):
                if h[child]:
                    stack.append(child)
            most = max(most, len(stack))
        out[r] = most
    return out


def camera_rays(s, W, H):
    """The pixel-centre rays of the scene's camera (tests/post_ref.py)."""
    from tests import post_ref
    o, d = post_ref.pixel_centre_rays(s.camera_c2w, s.vfov, s.aspect, W, H)
    d = np.ascontiguousarray(d.reshape(-1, 3), F)
    return np.tile(o.astype(F), (len(d), 1)), d


def oracle_trace(ps, origins, dirs, built=None):
    """orc_trace_ray (the reference's traverseBVH) over the oracle's BVH: (hit, t, uv)."""
    nodes, _, wv, _ = built if built is not None else O.build_bvh(ps)
    nodes_c = (O.Node * len(nodes)).from_buffer_copy(nodes.tobytes())
    idx = np.ascontiguousarray(ps.indices)
    wv = np.ascontiguousarray(wv)
    n = len(origins)
    hit = np.zeros(n, np.int32)
    t = np.zeros(n, F)
    uv = np.zeros((n, 2), F)
    tt = O.C.c_float()
    uu = (O.C.c_float * 2)()
    trace = O.lib().orc_trace_ray
    wv_p, idx_p = O._ptr(wv, O.C.c_float), O._ptr(idx, O.C.c_uint32)
    for i in range(n):
        hit[i] = trace(nodes_c, len(idx) // 3, wv_p, idx_p, (O.C.c_float * 3)(*origins[i]),
                       (O.C.c_float * 3)(*dirs[i]), O.C.byref(tt), uu)
        t[i] = tt.value
        uv[i] = uu[:]
    return hit, t, uv


# --------------------------------------------------------------------------
# face counts at the stack-id width
# --------------------------------------------------------------------------
def faces_exactly(n):
    """box subdivided twice (synth.subdivide: 1,932 * 16 = 30,912 faces) plus one
    more object of n - 30,912 small triangles in the free air of the room, on a
    grid 1/64 apart -- 64 Morton steps, so their keys are distinct from each
    other's -- each tilted differently.  n = 32,768 gives 65,535 nodes (the last
    count whose ids fit 16 bits), n = 32,769 gives 65,537."""
    from tinypathtracer_amd import synth
    s = base_scene("box")
    nf = s.n_faces
    ends = list(s.lut[1:, 0]) + [nf]
    pos, nrm, idx, lut, vcount = [], [], [], [], 0
    for o in range(len(s.lut)):
        tri = s.indices.reshape(-1, 3)[s.lut[o, 0]:ends[o]].astype(np.int64)
        lo, hi = int(tri.min()), int(tri.max()) + 1         # the object's own vertices
        p, q, t = s.vertices[lo:hi], s.normals[lo:hi], (tri - lo).astype(np.uint32)
        for _ in range(2):
            p, q, t = synth.subdivide(p, q, t)
        lut.append((sum(len(i) for i in idx) // 3, int(s.lut[o, 1])))
        idx.append((t.reshape(-1) + np.uint32(vcount)).astype(np.uint32))
        pos.append(p)
        nrm.append(q)
        vcount += len(p)
    have = sum(len(i) for i in idx) // 3
    extra = n - have
    if extra <= 0:
        raise ValueError(f"the subdivided box has {have} faces already")
    # a 3-D grid in x -0.5..0.5, y 1.2..1.7, z -0.5..0.5 (world: above the balls, below the lamp)
    k = np.arange(extra)
    gx, gy, gz = k % 32, (k // 32) % 32, k // 1024
    c = np.stack([-0.25 + gx / 64.0, 1.2 + gy / 64.0, -0.25 + gz / 64.0], 1)
    ang = 2.0 * np.pi * ((k * 0.6180339887) % 1.0)
    tilt = 0.3 + 0.4 * ((k * 0.7548776662) % 1.0)
    e1 = np.stack([np.cos(ang), tilt * np.sin(ang), np.sin(ang)], 1) * 0.006
    e2 = np.stack([-np.sin(ang), tilt * np.cos(ang), np.cos(ang)], 1) * 0.006
    tv = np.stack([c - (e1 + e2) / 3.0, c + (2.0 * e1 - e2) / 3.0, c + (2.0 * e2 - e1) / 3.0], 1).astype(F)
    tn = np.cross(tv[:, 1].astype(np.float64) - tv[:, 0], tv[:, 2].astype(np.float64) - tv[:, 0])
    tn /= np.linalg.norm(tn, axis=1, keepdims=True)
    lut.append((have, int(s.lut[0, 1])))
    idx.append(np.arange(3 * extra, dtype=np.uint32) + np.uint32(vcount))
    pos.append(tv.reshape(-1, 3))
    nrm.append(np.repeat(tn.astype(F), 3, axis=0))
    vt = np.concatenate([s.vert_trans, _IDENTITY[None]])
    nt = np.concatenate([s.normal_trans, _IDENTITY[None]])
    return _scene(np.concatenate(idx), np.concatenate(pos), np.concatenate(nrm), lut, vt, nt, s.materials, s.lights,
                  like=s)


def generic_rays(s, wv, W=32, H=18, n_random=1024, seed=11):
    """The camera's W x H pixel-centre rays and n_random chords of the scene's
    (finite) bounds, from origins up to a tenth outside them."""
    o1, d1 = camera_rays(s, W, H)
    rng = np.random.default_rng(seed)
    fin = wv[np.isfinite(wv).all(1)]
    lo, hi = fin.min(0), fin.max(0)
    o2 = (lo + (hi - lo) * rng.uniform(-0.1, 1.1, (n_random, 3))).astype(F)
    d2 = ((lo + (hi - lo) * rng.uniform(0.0, 1.0, (n_random, 3))).astype(F) - o2).astype(F)
    return np.concatenate([o1, o2]), np.concatenate([d1, d2])


def boundary_rays(s, ps, built, n_random=1024, seed=11):
    """The ray set of the stack-id width tests: generic_rays, and short rays onto
    the face of the last leaf (the largest node id) from both sides."""
    nodes, _, wv, _ = built
    o1, d1 = generic_rays(s, wv, 32, 18, n_random, seed)
    rng = np.random.default_rng(seed + 1)
    o2, d2 = o1[:0], d1[:0]
    fid = int(nodes["a"][-1])
    tri = wv[ps.indices.reshape(-1, 3)[fid]].astype(np.float64)
    nn = np.cross(tri[1] - tri[0], tri[2] - tri[0])
    nn /= np.linalg.norm(nn)
    b = rng.dirichlet([2.0, 2.0, 2.0], 32)
    p = b @ tri
    side = np.where(np.arange(32) % 2 == 0, 1.0, -1.0)[:, None]
    o3 = (p + side * nn * 0.004).astype(F)
    d3 = (p - o3.astype(np.float64)).astype(F)
    return np.concatenate([o1, o2, o3]), np.concatenate([d1, d2, d3]), fid


# --------------------------------------------------------------------------
# one, two, three triangles
# --------------------------------------------------------------------------
def tiny(n):
    """n = 1: one emissive triangle facing the camera; n = 2, 3: plus a diffuse
    floor triangle under it, then a diffuse one beside it that it lights."""
    if n not in (1, 2, 3):
        raise ValueError(n)
    tris = [((-2.2, -0.8, -3.0), (2.2, -0.8, -3.0), (0.0, 1.9, -3.0)),           # emitter, normal +z
            ((-2.4, -0.9, -1.2), (2.4, -0.9, -1.2), (0.3, -0.9, -5.0)),          # floor, normal +y
            ((-2.8, -0.8, -1.6), (-2.4, 1.3, -2.9), (-2.6, -0.8, -2.95))][:n]    # left wall, in front of the emitter
    verts = np.array(tris, F).reshape(-1, 3)
    v = verts.reshape(-1, 3, 3).astype(np.float64)
    nn = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    lut = np.array([[i, (1, 0, 2)[i]] for i in range(n)], np.int32)
    mats = np.stack([material_row((0.75, 0.7, 0.6)), material_row((1.0, 1.0, 1.0), 5.0),
                     material_row((0.3, 0.6, 0.8))])
    ident = np.tile(_IDENTITY, (n, 1))
    return _scene(np.arange(3 * n, dtype=np.uint32), verts, np.repeat(nn.astype(F), 3, axis=0), lut, ident, ident, mats,
                  [], camera=(_IDENTITY, 0.9, 16.0 / 9.0, 0.1))


# --------------------------------------------------------------------------
# the scenes of the two test files, by name: builder, then the frame both render
# (width, height, samples per pixel, max depth, "sky" for the procedural env)
# --------------------------------------------------------------------------
MATERIAL_COUNTS = (63, 64, 65, 200)          # TPT_MTL_LDS_MAX: (n + 1) * 32 bytes > 2048 from n = 64 on
RECORD_COUNTS = (0x7ffd, 0x7ffe)             # rec_words: 5-word path records from n = 0x7ffe on

def zoomed(base, factor):
    """A shipped scene seen through a narrower lens (vfov * factor), so that its
    content fills a small test frame."""
    s = copy.copy(base_scene(base) if isinstance(base, str) else base)
    s.vfov = F(F(s.vfov) * F(factor))
    return s


def tir_lit():
    """tir through a 0.4 x lens and with its lamp four times as wide and deep (16
    times the area): at a test frame's few samples the shipped lamp lights 0.5 %
    of the pixels, this one 48 %.  (The lamp's normal matrix stays: a scale along
    x and z leaves the normal of a horizontal quad alone.)"""
    s = zoomed("tir", 0.4)
    s.vert_trans = s.vert_trans.copy()
    m = s.vert_trans[1].reshape(4, 4)          # object 1: the lamp, column-major
    assert s.materials[s.lut[1, 1], 3] > 0
    m[0, :3] *= F(4.0)
    m[2, :3] *= F(4.0)
    return s


# the bases of the many-material scenes: a shipped scene, or one reshaped so that the
# oracle's frame at the test size is lit in a quarter of its pixels (square through a
# 0.4 x lens: 15 % -> 61 %; tir: tir_lit)
BASES = {"box": (lambda: base_scene("box"), 32, 18, 4, 8, None),
         "square": (lambda: zoomed("square", 0.4), 32, 18, 4, 8, None),
         "ball": (lambda: base_scene("ball"), 32, 18, 4, 8, "sky"),
         "tir": (tir_lit, 32, 18, 8, 64, None)}

SCENES = {}
for _n in MATERIAL_COUNTS + RECORD_COUNTS:
    SCENES[f"box_m{_n}"] = (lambda n=_n: with_materials(scene("box"), n),) + BASES["box"][1:]
    SCENES[f"square_m{_n}"] = (lambda n=_n: with_materials(scene("square"), n),) + BASES["square"][1:]
for _n in MATERIAL_COUNTS:
    SCENES[f"ball_m{_n}"] = (lambda n=_n: with_materials(scene("ball"), n),) + BASES["ball"][1:]
SCENES["tir_m64"] = (lambda: with_materials(scene("tir"), 64),) + BASES["tir"][1:]
SCENES["box_m64_deep"] = (lambda: scene("box_m64"), 32, 18, 4, 64, None)   # max_depth 64 in a closed room
SCENES["box_inf"] = (lambda: with_inf_vertex(scene("box")), 32, 18, 4, 8, None)
for _d in ("up", "down"):
    SCENES[f"chain_{_d}"] = (lambda d=_d: chain(d), 48, 27, 4, 8, None)
    SCENES[f"chain_{_d}_inf"] = (lambda d=_d: chain(d, inf=True), 48, 27, 4, 8, None)
for _n in (32768, 32769):
    SCENES[f"faces_{_n}"] = (lambda n=_n: faces_exactly(n), 32, 18, 4, 8, None)
for _n in (1, 2, 3):
    SCENES[f"tiny{_n}"] = (lambda n=_n: tiny(n), 32, 18, 4, 8, None)
BASES["box_deep"] = (lambda: scene("box"), 32, 18, 4, 64, None)



def base_name(name):
    """The BASES entry whose frame SCENES[name] must reproduce bit for bit: a grown
    material table, or the unhittable triangle, changes no radiance bit."""
    if name == "box_m64_deep":
        return "box_deep"
    if name == "box_inf":
        return "box"
    base, _, count = name.partition("_m")
    return base if count.isdigit() and base in BASES else None


_built = {}


def scene(name) -> oscene.OracleScene:
    """SCENES[name] or BASES[name], built once per process."""
    if name not in _built:
        _built[name] = (SCENES[name] if name in SCENES else BASES[name])[0]()
    return _built[name]


def frame_of(name):
    return (SCENES[name] if name in SCENES else BASES[name])[1:]


def sky():
    import tinypathtracer_amd as T
    return T.procedural_sky(64, 32)


_frames = {}


def oracle_frame(name, env_is=False):
    """The oracle's frame of a named scene at its test size, seed 42, rendered once
    per process: (radiance, bgra, counters).  Read-only."""
    key = (name, env_is)
    if key not in _frames:
        W, H, spp, depth, env = frame_of(name)
        rad, bgra, cnt = O.render(oracle_scene(scene(name)), W, H, spp, depth, 42,
                                  env=sky()[::-1].copy() if env else None, trig_mode=1, env_is=env_is)
        rad.setflags(write=False)
        bgra.setflags(write=False)
        _frames[key] = (rad, bgra, cnt)
    return _frames[key]


_bvhs = {}


def oracle_bvh(name):
    """(PackedScene, (nodes, keys, world vertices, world normals)) of a named scene, once per process."""
    if name not in _bvhs:
        ps = oracle_scene(scene(name))
        _bvhs[name] = (ps, O.build_bvh(ps))
    return _bvhs[name]
