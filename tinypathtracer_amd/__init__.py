"""tinypathtracer_amd -- MI355X-native TinyPathTracer hot path, Python host mirror.

Mirrors the reference host API (include/path_tracer.h:16-35,
include/mesh.cuh:98-115, include/bvh.cuh:60-68, include/camera.h) over the
C-ABI in include/tpt.h (libtpt.so, HIP for gfx950):

    pt = PathTracer(env_file)            # PathTracer(const std::string&)
    frame = pt.render("input/box.gltf")  # render(meshFile), headless

Scene/Mesh loading, BVH construction and the trace megakernel all run in the
native library; this module only marshals arrays.
"""
from __future__ import annotations

import ctypes as C
import os
import time
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import TPTError, build_identity, check, lib

__all__ = ["Camera", "Scene", "DeviceScene", "BVH", "EnvLight", "PathTracer", "Frame", "TPTError",
           "procedural_sky", "version", "device_count", "build_identity", "NODE_DTYPE", "DENOISE_DEFAULTS",
           "History", "TEMPORAL_DEFAULTS", "TEMPORAL_PATH_DEFAULTS", "CLIP_DEFAULTS", "motion_matrices", "ADAPTIVE_DEFAULTS",
           "UPSAMPLE_DEFAULTS", "low_size", "Exposure", "TONEMAP_DEFAULTS"]

# BVHNode (include/bvh.cuh:52-58): parent, info{left,right | fid,placeHolder}, box
NODE_DTYPE = np.dtype([("parent", "<u4"), ("a", "<i4"), ("b", "<i4"), ("bmin", "<f4", 3), ("bmax", "<f4", 3)])


def version() -> str:
    return lib().tpt_version().decode()


def device_count() -> int:
    return int(lib().tpt_device_count())


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


@dataclass
class Camera:
    """include/camera.h:9-65 (getters :56-58); c2w = m_transform->localToWorld()."""
    c2w: np.ndarray
    vfov: float
    aspect: float
    znear: float = 0.1

    def getVFov(self):
        return self.vfov

    def getAspRatio(self):
        return self.aspect

    def getNearPlane(self):
        return self.znear

    def yawed(self, deg: float) -> "Camera":
        """This camera turned by `deg` degrees about its own origin and up axis
        (c2w * R_y, as tpt_render --yaw does per frame)."""
        m = np.asarray(self.c2w, np.float32).reshape(4, 4).astype(np.float64)   # rows = columns of c2w
        t = np.deg2rad(float(deg))
        out = m.copy()
        out[0] = np.cos(t) * m[0] - np.sin(t) * m[2]
        out[2] = np.sin(t) * m[0] + np.cos(t) * m[2]
        return Camera(out.astype(np.float32).reshape(16), self.vfov, self.aspect, self.znear)

    def moved(self, dx: float, dy: float, dz: float) -> "Camera":
        """This camera with its origin shifted by (dx, dy, dz) in world space (as tpt_render
        --truck does per frame): c2w's translation column plus the shift, in float32."""
        out = np.array(self.c2w, np.float32).reshape(16).copy()
        out[12:15] = out[12:15] + np.asarray((dx, dy, dz), np.float32)
        return Camera(out, self.vfov, self.aspect, self.znear)

    def to_c(self) -> _lib.Camera:
        c = _lib.Camera()
        c.c2w[:] = [float(v) for v in np.asarray(self.c2w, np.float32).reshape(16)]
        c.vfov, c.aspect, c.znear = float(self.vfov), float(self.aspect), float(self.znear)
        return c


class Scene:
    """Scene(filename, type) (mesh.cu:68-79): host-side glTF scene, loaded by the
    native loader (mesh.cu:80-307 semantics).  Arrays are the packed content of
    copySceneToDevice (mesh.cu:309-397)."""

    def __init__(self, filename: str, type: str = "gltf"):
        if type != "gltf":
            raise RuntimeError("Unsupported file format. Only support .gltf file.")
        h = C.c_void_p()
        check(lib().tpt_gltf_load(os.fsencode(filename), C.byref(h)))
        try:
            d = _lib.SceneDesc()
            cam = _lib.Camera()
            check(lib().tpt_gltf_desc(h, C.byref(d), C.byref(cam)))
            nf, nv = d.n_faces, d.n_vertices
            self.indices = np.ctypeslib.as_array(d.indices, (3 * nf,)).copy()
            self.vertices = np.ctypeslib.as_array(d.vertices, (nv, 3)).copy()
            self.normals = np.ctypeslib.as_array(d.normals, (nv, 3)).copy()
            self.lut = np.array([(d.lut[i].begin, d.lut[i].mtl) for i in range(d.n_objects)], np.int32)
            self.vert_trans = np.ctypeslib.as_array(d.vert_trans, (d.n_objects, 16)).copy()
            self.normal_trans = np.ctypeslib.as_array(d.normal_trans, (d.n_objects, 16)).copy()
            self.materials = np.array([[*d.materials[i].base_color] + [getattr(d.materials[i], f)
                                        for f, _ in _lib.Material._fields_[1:]] for i in range(d.n_materials)],
                                      np.float32).reshape(-1, 15)
            self.lights = [_lib.Light.from_buffer_copy(d.lights[i]) for i in range(d.n_lights)]
            self.missing_material = bool(lib().tpt_gltf_missing_material(h))
            self.m_camera = Camera(np.array(cam.c2w[:], np.float32), cam.vfov, cam.aspect, cam.znear)
        finally:
            lib().tpt_gltf_free(h)
        self.filename = filename

    @classmethod
    def from_arrays(cls, indices, vertices, normals, lut, vert_trans, normal_trans, materials=(), lights=(),
                    camera: "Camera | None" = None) -> "Scene":
        """A scene from packed arrays in the layouts the loader produces (the
        attributes above): indices uint32 [3F], vertices / normals float32 [V, 3],
        lut int32 [O, 2] (first face, material id), vert_trans / normal_trans
        float32 [O, 16] column-major, materials float32 [M, 15].  lights: _lib.Light
        structs, or dicts with their field names.  camera None: Camera() of the
        reference (identity, vfov 60, aspect 1.77778)."""
        s = cls.__new__(cls)
        s.indices = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        s.vertices = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        s.normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        s.lut = np.ascontiguousarray(lut, np.int32).reshape(-1, 2)
        s.vert_trans = np.ascontiguousarray(vert_trans, np.float32).reshape(-1, 16)
        s.normal_trans = np.ascontiguousarray(normal_trans, np.float32).reshape(-1, 16)
        s.materials = np.ascontiguousarray(materials, np.float32).reshape(-1, 15)
        if len(s.indices) % 3 or len(s.normals) != len(s.vertices) or len(s.vert_trans) != len(s.lut) or \
                len(s.normal_trans) != len(s.lut):
            raise ValueError("from_arrays: 3 indices per face, a normal per vertex, two matrices per object")
        if len(s.indices) and int(s.indices.max()) >= len(s.vertices):
            raise ValueError("from_arrays: an index past the vertices")
        s.lights = []
        for L in lights:
            if not isinstance(L, _lib.Light):
                d, L = L, _lib.Light()
                L.type, L.intensity = int(d["type"]), float(d["intensity"])
                L.cos_outer, L.inv_cos_cone_diff = float(d["cos_outer"]), float(d["inv_cos_cone_diff"])
                for k in ("color", "pos", "direction"):
                    getattr(L, k)[:] = [float(v) for v in d[k]]
            s.lights.append(L)
        s.missing_material = len(s.materials) == 0
        s.m_camera = camera if camera is not None else \
            Camera(np.eye(4, dtype=np.float32).reshape(16), 60.0, 1.77778, 0.1)
        s.filename = ""
        return s

    @property
    def n_faces(self):
        return len(self.indices) // 3

    def desc(self):
        """tpt_scene_desc view (keeps buffers alive on self)."""
        self._mats = (_lib.Material * max(len(self.materials), 1))()
        for i, row in enumerate(self.materials):
            m = self._mats[i]
            m.base_color[:] = [float(v) for v in row[:3]]
            for k, (f, _) in enumerate(_lib.Material._fields_[1:]):
                setattr(m, f, float(row[3 + k]))
        self._lights = (_lib.Light * max(len(self.lights), 1))(*self.lights)
        self._lut = (_lib.Interval * len(self.lut))(*[_lib.Interval(int(b), int(m)) for b, m in self.lut])
        self._arr = [np.ascontiguousarray(a) for a in (self.indices, self.vertices, self.normals,
                                                        self.vert_trans, self.normal_trans)]
        ind, ver, nor, vt, nt = self._arr
        return _lib.SceneDesc(
            ind.ctypes.data_as(C.POINTER(C.c_uint32)), self.n_faces,
            ver.ctypes.data_as(C.POINTER(C.c_float)), nor.ctypes.data_as(C.POINTER(C.c_float)), len(ver),
            C.cast(self._lut, C.POINTER(_lib.Interval)), len(self.lut),
            vt.ctypes.data_as(C.POINTER(C.c_float)), nt.ctypes.data_as(C.POINTER(C.c_float)),
            C.cast(self._mats, C.POINTER(_lib.Material)), len(self.materials),
            C.cast(self._lights, C.POINTER(_lib.Light)), len(self.lights))

    def copySceneToDevice(self, device: int = 0) -> "DeviceScene":
        return DeviceScene(self, device)

    def device_buffers(self, device: int = 0) -> dict:
        """The reference's DeviceScene (mesh.cuh:80-96) as torch tensors in HBM of
        `device`, element types and layouts as the reference's thrust
        device_vectors hold them: indices u32, Vec3 vertices/normals, Material
        (15 floats), MtlInterval, column-major Mat4, and DeltaLight
        (delta_light.h:96-130, 52 B: the type, then the light union -- a
        directional light's direction where the others keep pos; bytes a light
        type does not own are NaN here, so a reader of them would show).  These
        are the `trace` kernel's own arguments (path_tracer.cu:297-299);
        DeviceScene(scene, device, buffers=...) hands them to tpt_scene_create
        as device pointers."""
        import torch
        dev = torch.device("cuda", device)
        lights = np.full((max(len(self.lights), 1), 13), np.nan, np.float32)
        for i, L in enumerate(self.lights):
            row = lights[i]
            row[0:1].view(np.int32)[0] = L.type
            row[1:4] = L.color[:]
            row[4] = L.intensity
            if L.type == 1:    # DirectionalLight{color, intensity, direction}
                row[5:8] = L.direction[:]
            else:              # PointLight{color, intensity, pos}; SpotLight{..., pos, direction, cos, invDiff}
                row[5:8] = L.pos[:]
                if L.type == 2:
                    row[8:11] = L.direction[:]
                    row[11] = L.cos_outer
                    row[12] = L.inv_cos_cone_diff
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if len(a) else \
            torch.empty(0, dtype=dt, device=dev)
        bufs = {
            "indices": t(self.indices.astype(np.uint32).view(np.int32), torch.int32),
            "vertices": t(self.vertices.astype(np.float32), torch.float32),
            "normals": t(self.normals.astype(np.float32), torch.float32),
            "materials": t(self.materials.astype(np.float32), torch.float32),
            "materialsLUT": t(self.lut.astype(np.int32), torch.int32),
            "vertTrans": t(self.vert_trans.astype(np.float32), torch.float32),
            "normalTrans": t(self.normal_trans.astype(np.float32), torch.float32),
            "lights": t(lights[:len(self.lights)], torch.float32),
        }
        torch.cuda.synchronize(dev)
        return bufs


class DeviceScene:
    """DeviceScene (mesh.cuh:80-96): scene buffers resident in HBM of `device`."""

    def __init__(self, scene: Scene, device: int = 0, buffers: dict | None = None):
        """buffers: Scene.device_buffers() -- device arrays in the reference's
        layouts, passed to tpt_scene_create as device pointers (the reference's
        doTrace hands over its DeviceScene this way)."""
        self.scene = scene
        self.device = device
        self.handle = C.c_void_p()
        if buffers is None:
            d = scene.desc()
        else:
            b = buffers
            dp = lambda k, ty: C.cast(C.c_void_p(b[k].data_ptr() if b[k].numel() else 0), C.POINTER(ty))
            d = _lib.SceneDesc(
                dp("indices", C.c_uint32), b["indices"].numel() // 3,
                dp("vertices", C.c_float), dp("normals", C.c_float), b["vertices"].numel() // 3,
                dp("materialsLUT", _lib.Interval), b["materialsLUT"].numel() // 2,
                dp("vertTrans", C.c_float), dp("normalTrans", C.c_float),
                dp("materials", _lib.Material), b["materials"].numel() // 15,
                dp("lights", _lib.Light), b["lights"].numel() // 13, _lib.DESC_DELTALIGHT_LAYOUT)
        check(lib().tpt_scene_create(C.byref(d), device, C.byref(self.handle)))
        self.built = False

    def set_build_threads(self, threads: int):
        """Host threads of the traversal-tree build (tpt_scene_set_build_threads):
        < 0 the usable cores, 0/1 serial; the same tree either way."""
        check(lib().tpt_scene_set_build_threads(self.handle, int(threads)))
        return self

    def build(self, asynchronous: bool = False):
        """World transform + LBVH (path_tracer.cu:536-542) on the device, then
        the host SAH traversal trees.  asynchronous=True: the host trees finish
        on a background thread (tpt_scene_build_async) while the next render
        enqueues its RNG initialisation; that render waits for them."""
        check(lib().tpt_scene_build_async(self.handle) if asynchronous else lib().tpt_scene_build(self.handle))
        self.built = True
        return self

    def set_transforms(self, first: int, vert_trans, normal_trans=None):
        """New local-to-world matrices for objects first, first + 1, ... (tpt_scene_set_transforms):
        vert_trans [n, 16] float32, column-major like Scene.vert_trans; normal_trans likewise, or
        None for the loader's inverse transpose.  The vertices stay on the device; the scene
        is unbuilt afterwards, so build() comes next.  A progressive accumulation does not
        survive it."""
        vt = np.ascontiguousarray(vert_trans, np.float32).reshape(-1, 16)
        nt = None if normal_trans is None else np.ascontiguousarray(normal_trans, np.float32).reshape(-1, 16)
        if nt is not None and nt.shape != vt.shape:
            raise ValueError(f"normal_trans: need {vt.shape[0]} matrices, got {nt.shape[0]}")
        check(lib().tpt_scene_set_transforms(self.handle, int(first), len(vt), _ptr(vt), _ptr(nt)))
        self.built = False
        return self

    def set_vertices(self, first: int, vertices, normals=None):
        """New object-space positions for vertices first, first + 1, ... (tpt_scene_set_vertices):
        vertices [n, 3] float32 like Scene.vertices; normals likewise, or None to keep the stored
        ones.  Each a numpy array or a torch CUDA tensor of the scene's device.  Topology,
        materials and matrices stay; the scene is unbuilt afterwards, so build() comes next.  A
        progressive accumulation does not survive it.  self.scene keeps the arrays it was made of."""
        def plane(a):
            if a is None:
                return None
            if not hasattr(a, "data_ptr"):       # numpy, or anything numpy can read
                return np.ascontiguousarray(a, np.float32).reshape(-1, 3)
            if str(a.dtype) != "torch.float32" or not a.is_contiguous() or a.numel() % 3:
                raise ValueError("set_vertices: a contiguous float32 tensor of xyz triples")
            return a
        count = lambda a: a.size // 3 if isinstance(a, np.ndarray) else a.numel() // 3
        v, n = plane(vertices), plane(normals)
        if n is not None and count(n) != count(v):
            raise ValueError(f"normals: need {count(v)} vertices, got {count(n)}")
        check(lib().tpt_scene_set_vertices(self.handle, int(first), count(v), _addr(v), _addr(n)))
        self.built = False
        return self

    def refit(self) -> dict:
        """In place of build() after set_vertices / set_transforms (tpt_scene_refit): the trees'
        topology and the triangle order of the last full build stay, every box is recomputed on
        the device.  Falls back to a full build where it must (never built, no SAH tree, a
        non-finite vertex).  Returns tpt_refit_stats as a dict: rebuilt, launches, slivers,
        cull_eps, ms, cost, cost_built -- cost / cost_built is the caller's signal for a rebuild."""
        st = _lib.RefitStats()
        check(lib().tpt_scene_refit(self.handle, C.byref(st)))
        self.built = True
        return st.as_dict()

    def read_wide(self):
        """The resident 4-wide traversal trees (tpt_scene_read_wide): (main [n_main, 32],
        emissive [n_emit, 32]) float32, as uploaded or refitted; links are the int32 bits of
        columns 24..27."""
        nm, ne = C.c_int32(0), C.c_int32(0)
        check(lib().tpt_scene_read_wide(self.handle, None, 0, C.byref(nm), C.byref(ne)))
        nodes = np.zeros((nm.value + ne.value, 32), np.float32)
        check(lib().tpt_scene_read_wide(self.handle, _ptr(nodes), len(nodes), C.byref(nm), C.byref(ne)))
        return nodes[:nm.value], nodes[nm.value:]

    def read_bvh(self):
        nf = self.scene.n_faces
        nodes = np.zeros(2 * nf - 1, NODE_DTYPE)
        keys = np.zeros(nf, np.int64)
        check(lib().tpt_scene_read_bvh(self.handle, _ptr(nodes), _ptr(keys)))
        return nodes, keys

    def read_world(self):
        nv = len(self.scene.vertices)
        wv = np.zeros((nv, 3), np.float32)
        wn = np.zeros((nv, 3), np.float32)
        check(lib().tpt_scene_read_world(self.handle, _ptr(wv), _ptr(wn)))
        return wv, wn

    def trace_rays(self, origins, dirs, mode=0, origin_fid=None):
        """mode 0: the reference's visit order; 1: the render's ordered culled
        traversal; 2: any hit; 3: two-pass probe (see tpt_debug_trace_rays).
        origin_fid: per ray the face it leaves (-1 none), as the render knows it
        for secondary rays (the grazing test)."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = len(o)
        hit = np.zeros(n, np.int32)
        t = np.zeros(n, np.float32)
        uv = np.zeros((n, 2), np.float32)
        of = None if origin_fid is None else np.ascontiguousarray(origin_fid, np.int32).reshape(n)
        check(lib().tpt_debug_trace_rays(self.handle, n, _ptr(o), _ptr(d), _ptr(of), mode, _ptr(hit), _ptr(t),
                                         _ptr(uv)))
        return hit, t, uv

    def step_latency(self, origins, dirs, mode=0, flags=0):
        """ONE 64-lane wave walks these <= 64 closest-hit rays (tpt_debug_step_latency):
        mode 0 nodes from global memory, 1 the whole 4-wide tree in LDS, 2 four lanes
        per ray (<= 16 rays; steps = node visits, leaf children tested in-node).  Returns
        (steps per lane, wave loop iterations, wave shader cycles, hit fids)."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        out = np.zeros((64, 4), np.uint64)
        check(lib().tpt_debug_step_latency(self.handle, len(o), _ptr(o), _ptr(d), mode, flags, _ptr(out)))
        n = len(o)
        return out[:n, 0].astype(np.int64), int(out[0, 1]), int(out[0, 2]), out[:n, 3].astype(np.int64)

    def close(self):
        if self.handle:
            lib().tpt_scene_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def hot_kat(op, cases, device=0):
    """The trace kernel's own device functions on `cases` (tpt_debug_hot_kat):
    op 0 box (n,12) -> (n,2); 1 triangle (n,15) -> (n,4); 2 light (n,16) -> (n,6);
    3 toUChar (n,3) -> (n,3).  Tests pin them to the reference's headers."""
    nin, nout = {0: (12, 2), 1: (15, 4), 2: (16, 6), 3: (3, 3)}[op]
    a = np.ascontiguousarray(cases, np.float32).reshape(-1, nin)
    out = np.zeros((len(a), nout), np.float32)
    check(lib().tpt_debug_hot_kat(device, op, len(a), _ptr(a), _ptr(out)))
    return out


ENV_KAT_OPS = {"sincos": 0, "atan2": 1, "acos": 2, "lookup": 3, "env_is": 4, "new_direction": 5}
_ENV_KAT_SHAPES = {0: (1, 2), 1: (2, 1), 2: (1, 1), 3: (3, 10), 4: (5, 7), 5: (8, 5)}


def env_kat(op, cases, env=None, states=None, device=0):
    """The device's env paths, parity trig and getNewDirection on `cases`, one per
    lane (tpt_debug_env_kat; op by number or ENV_KAT_OPS name):
    sincos (n,1) x -> (n,2) sin, cos of fsincos_2pi; atan2 (n,2) y, x -> (n,1) and
    acos (n,1) -> (n,1), the double path; lookup (n,3) dir -> (n,10): env_col_fast,
    env_row_fast (-1: undecided), env_col_exact, env_row_exact, the lookup's rgb out
    of line and inlined; env_is (n,5) nf, x1, x2 -> (n,7): ok, dir, k_le against the
    tables of `env` (an EnvLight; lookup and env_is need one); new_direction (n,8)
    d, n, eta, metallic with `states` (n,6) uint32 -> ((n,5) next, atten, pdf; the
    states after).  Tests compare them bit for bit with the oracle's hooks."""
    op = ENV_KAT_OPS.get(op, op)
    nin, nout = _ENV_KAT_SHAPES[op]
    a = np.ascontiguousarray(cases, np.float32).reshape(-1, nin)
    out = np.zeros((len(a), nout), np.float32)
    st = None
    if states is not None:
        st = np.array(states, np.uint32).reshape(-1, 6).copy()
        if len(st) != len(a):
            raise ValueError("one RNG state per case")
    handle = env.handle if env is not None else None
    check(lib().tpt_debug_env_kat(device, handle, op, len(a), _ptr(a), _ptr(st) if st is not None else None,
                                  _ptr(out)))
    return (out, st) if op == 5 else out


class BVH:
    """BVH (bvh.cuh:60-68): BVH(size) + construct(vertices, indices) -> m_nodes, m_keys.
    Construction runs on the device (src/bvh.cu:304-331 semantics)."""

    def __init__(self, size: int = 0):
        self.size = size
        self.m_nodes = np.zeros(max(2 * size - 1, 0), NODE_DTYPE)
        self.m_keys = np.zeros(size, np.int64)

    def construct(self, device_scene: DeviceScene):
        if not device_scene.built:
            device_scene.build()
        self.m_nodes, self.m_keys = device_scene.read_bvh()
        self.size = len(self.m_keys)
        return self


def procedural_sky(width=2048, height=1024):
    """Deterministic equirect RGBA8 stand-in for the missing kloppenheim env
    (SURVEY 8(d) C3).  Returns rows top-down (image order)."""
    v = (np.arange(height, dtype=np.float64) + 0.5) / height          # 0 = top
    u = (np.arange(width, dtype=np.float64) + 0.5) / width
    theta = v * np.pi
    phi = u * 2.0 * np.pi
    elev = np.cos(theta)[:, None]
    sky = np.clip(elev, 0.0, 1.0)
    ground = np.clip(-elev, 0.0, 1.0)
    sun = np.exp(-((theta[:, None] - 0.9) ** 2 + (np.cos(phi[None, :]) - 1.0) ** 2) * 40.0)
    r = 0.45 + 0.25 * sky - 0.25 * ground + 0.5 * sun
    g = 0.55 + 0.25 * sky - 0.30 * ground + 0.45 * sun
    b = 0.75 + 0.20 * sky - 0.45 * ground + 0.30 * sun
    img = np.stack([r + 0 * phi[None, :], g + 0 * phi[None, :], b + 0 * phi[None, :]], -1)
    img = np.clip(img * 255.0, 0, 255).astype(np.uint8)
    alpha = np.full((height, width, 1), 255, np.uint8)
    return np.concatenate([img, alpha], -1)


class EnvLight:
    """EnvLight (env_light.cuh:8-18): equirect radiance, used on miss (A14).
    Accepts an image file or an RGBA/RGB array in image order (row 0 = top);
    stored row 0 = bottom like FreeImage (picture.h:41-43).  JPEG and binary
    PPM files are decoded by the library's native decoder (tpt_env_load, the
    FreeImage/libjpeg arithmetic); other formats go through PIL."""

    def __init__(self, source=None, device: int = 0):
        self.device = device
        self.handle = C.c_void_p()
        if source is None or (isinstance(source, str) and source == ""):
            self.rgba = None
            return
        if isinstance(source, str):
            if self._native(source):
                self.rgba = None
                check(lib().tpt_env_load(source.encode(), device, C.byref(self.handle)))
                return
            img = self._read(source)
        else:
            img = np.asarray(source, np.uint8)
        if img.ndim != 3 or img.shape[2] not in (3, 4):
            raise RuntimeError("Failed to create texture! Choose picture with 3 or 4 channels.")
        if img.shape[2] == 3:
            img = np.concatenate([img, np.full(img.shape[:2] + (1,), 255, np.uint8)], -1)
        self.rgba = np.ascontiguousarray(img[::-1])           # bottom-up
        h, w = self.rgba.shape[:2]
        check(lib().tpt_env_create(_ptr(self.rgba), w, h, device, C.byref(self.handle)))

    @staticmethod
    def _native(path):
        try:
            with open(path, "rb") as f:
                head = f.read(2)
        except OSError as e:
            raise RuntimeError(f"Failed to open file {path}") from e
        return head in (b"\xff\xd8", b"P6")

    @staticmethod
    def _read(path):
        try:
            from PIL import Image
        except ImportError as e:   # pragma: no cover
            raise RuntimeError(f"Failed to open file {path}: no image decoder") from e
        try:
            with Image.open(path) as im:
                return np.asarray(im.convert("RGBA"))
        except OSError as e:
            raise RuntimeError(f"Failed to open file {path}") from e

    def close(self):
        if self.handle:
            lib().tpt_env_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class Frame:
    bgra: np.ndarray            # [H, W, 4] uint8, row 0 = top (copyToFB layout)
    radiance: np.ndarray        # [H, W, 3] float32, row 0 = bottom (color / spp)
    stats: dict = field(default_factory=dict)


# Denoiser defaults of the Python host and the CLI (DESIGN.md section 5 "Post-pass":
# checked against a 2,048-spp render of box at 8 spp)
DENOISE_DEFAULTS = {"iterations": 5, "sigma_color": 4.0, "sigma_normal": 0.3, "sigma_depth": 0.05,
                    "demodulate": True}

# buffer name -> (values per pixel, element type) of tpt_aov's planes, the radiance and the framebuffer
AOV_LAYOUT = {"albedo": (3, "float32"), "normal": (3, "float32"), "depth": (1, "float32"),
              "face": (1, "int32"), "material": (1, "int32")}
_PLANES = dict(AOV_LAYOUT, radiance=(3, "float32"), framebuffer=(4, "uint8"))

# Mirror-path feature buffers (tpt_render_aov_path): the hosts' and the CLI's default cap, the
# render's default max_depth
AOV_PATH_DEFAULTS = {"max_bounces": 8}
# doTraceAdaptive: tiles stop once their error estimate (tpt.h, tpt_render_adaptive) is below the target
ADAPTIVE_DEFAULTS = {"min_spp": 16, "max_spp": 1024, "target": 0.1}
_PLANES.update(bounces=(1, "int32"), points=(3, "float32"))


def _aov_out(out, width, height, extra=()):
    """renderAOV's / renderAOVPath's `out`: the default buffers for None, the unknown-key check."""
    keys = tuple(AOV_LAYOUT) + tuple(extra)
    if out is None:
        return {k: np.zeros((height, width) + ((3,) if _PLANES[k][0] == 3 else ()), _PLANES[k][1]) for k in keys}
    unknown = set(out) - set(keys)
    if unknown:
        raise ValueError(f"unknown feature buffers {sorted(unknown)}")
    return out


def _take_guides(aov, keys, width, height):
    """The feature planes `keys` of aov that are there, checked, as the library's tpt_aov."""
    g = _lib.Aov()
    for k in keys:
        buf = aov.get(k)
        if buf is not None:
            _check_plane(k, buf, width, height)
            setattr(g, k, _addr(buf))
    return g


def _check_plane(name, buf, width, height):
    """The library reads / writes width * height * channels elements behind the
    pointer: refuse a buffer of another size or element type."""
    ch, dt = _PLANES[name]
    if isinstance(buf, int):   # a raw device pointer: the caller's responsibility
        return
    n = buf.size if isinstance(buf, np.ndarray) else buf.numel()
    have = str(buf.dtype).replace("torch.", "")
    if n != width * height * ch or have != dt:
        raise ValueError(f"{name}: need {width * height * ch} {dt} values ({height} x {width} x {ch}), "
                         f"got {n} of {have}")


# Temporal-accumulation defaults of the hosts and the CLI (tpt.hpp defaultTemporal)
TEMPORAL_DEFAULTS = {"alpha": 0.1, "depth_tol": 0.1, "normal_min": 0.9, "max_history": 32, "demodulate": True}
_PLANES.update(variance=(1, "float32"), history_len=(1, "float32"), motion_out=(2, "float32"))


# Accumulation through mirrors (tpt_temporal_path): TEMPORAL_DEFAULTS, and point_tol by the sweep of
# tools/temporal_path_quality.py (DESIGN.md section 5 "Temporal accumulation through mirrors")
TEMPORAL_PATH_DEFAULTS = dict(TEMPORAL_DEFAULTS, point_tol=8.0)


# History clipping (History.set_clip): by the sweep of tools/clip_quality.py (DESIGN.md section 5
# "History clipping")
CLIP_DEFAULTS = {"radius": 1, "gamma": 1.0, "max_history": 4}


def motion_matrices(prev, cur):
    """tpt_motion_matrices: from the objects' local-to-world matrices of the previous frame
    and of this one ([n, 16] float32, column-major) the records tpt_temporal_motion works
    with.  Returns (D [n, 3, 4], G [n, 3, 3] float32, flags [n] int32: _lib.MOTION_*, the
    number of untracked objects)."""
    p = np.ascontiguousarray(prev, np.float32).reshape(-1, 16)
    c = np.ascontiguousarray(cur, np.float32).reshape(-1, 16)
    if p.shape != c.shape:
        raise ValueError(f"{p.shape[0]} previous matrices, {c.shape[0]} current ones")
    out = np.zeros((len(p), 24), np.float32)
    untracked = int(lib().tpt_motion_matrices(len(p), _ptr(p), _ptr(c), _ptr(out)))
    return (out[:, :12].reshape(-1, 3, 4).copy(), out[:, 12:21].reshape(-1, 3, 3).copy(),
            out[:, 21].copy().view(np.int32), untracked)

# Defaults of the variance-guided filter of the hosts and the CLI (tpt.hpp defaultSVGF;
# DESIGN.md section 5 "Post-pass": sigma_lum by the sweep there, not the paper's phi_l = 4, which blurs
# an accumulated frame whose variance_in is the variance of one frame's luminance)
SVGF_DEFAULTS = {"iterations": 5, "sigma_lum": 0.5, "sigma_normal": 0.3, "sigma_depth": 0.05, "min_history": 4,
                 "demodulate": True}


# Guided upsampling (PathTracer.upsample): chosen by the sweep of tools/upsample_quality.py (DESIGN.md
# section 5 "Guided upsampling"), which started from DENOISE_DEFAULTS' sigmas: sigma_depth 0.2 has the
# lower error than 0.05 in 7 of its 8 columns, sigma_normal and demodulation move nothing on box
UPSAMPLE_DEFAULTS = {"sigma_normal": 0.3, "sigma_depth": 0.2, "demodulate": False}


def low_size(width: int, height: int, scale: int):
    """The low frame size of an integer scale: (ceil(width / scale), ceil(height / scale))."""
    width, height, scale = int(width), int(height), int(scale)
    if width <= 0 or height <= 0 or scale <= 0:
        raise ValueError(f"low_size: width, height and scale must be > 0, got {width}, {height}, {scale}")
    return (width + scale - 1) // scale, (height + scale - 1) // scale


class History:
    """tpt_temporal's state across frames (tpt_history): the accumulated colour, the
    history length, the luminance moments and the feature buffers of the previous
    frame, for one frame size.  d_scene supplies the device and the stream; close the
    history before it."""

    def __init__(self, d_scene: DeviceScene, width: int, height: int):
        self.width, self.height = int(width), int(height)
        self.handle = C.c_void_p()
        check(lib().tpt_history_create(d_scene.handle, self.width, self.height, C.byref(self.handle)))
        self._scene = d_scene                   # kept alive: the history is destroyed first

    def reset(self):
        """The next temporal() starts over: every pixel disoccluded."""
        check(lib().tpt_history_reset(self.handle))
        return self

    def set_clip(self, params=True, *, radius: int = CLIP_DEFAULTS["radius"], gamma: float = CLIP_DEFAULTS["gamma"],
                 max_history: int = CLIP_DEFAULTS["max_history"]):
        """History clipping (tpt_history_set_clip): every later temporal call on this history
        clamps its reprojected history colour to mean +- gamma standard deviations of the current
        frame's colours over the similar pixels of a (2 radius + 1)^2 window, and caps a clipped
        pixel's history length at max_history.  set_clip(None) turns it off (the default); the
        setting survives reset()."""
        if params is None:
            check(lib().tpt_history_set_clip(self.handle, None))
        else:
            p = _lib.ClipParams(int(radius), float(gamma), int(max_history), 0)
            check(lib().tpt_history_set_clip(self.handle, C.byref(p)))
        return self

    def clip_stats(self) -> dict:
        """box_ms, boxed, clipped of the last temporal call on this history (zeros with the clip off)."""
        st = _lib.ClipStats()
        check(lib().tpt_history_clip_stats(self.handle, C.byref(st)))
        return st.as_dict()

    def close(self):
        if self.handle:
            lib().tpt_history_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# Tone mapping (PathTracer.tonemap; tpt.hpp defaultTonemap): conventions -- Reinhard's white point of
# 4, the sRGB curve, the photographic key of 0.18 and a 10 % / 95 % trim -- not the result of a sweep
TONEMAP_DEFAULTS = {"op": "reinhard", "transfer": "srgb", "auto": False, "dither": False, "ev": 0.0, "white": 4.0,
                    "gamma": 2.2, "key": 0.18, "p_low": 0.10, "p_high": 0.95, "min_ev": -16.0, "max_ev": 16.0,
                    "rate": 1.0}


class Exposure:
    """tpt_tonemap's adapted exposure across frames (tpt_exposure): the log2 scale the last
    auto-exposed frames settled on and the last measured histogram.  d_scene supplies the device
    and the stream; close the exposure before it."""

    def __init__(self, d_scene: DeviceScene):
        self.handle = C.c_void_p()
        check(lib().tpt_exposure_create(d_scene.handle, C.byref(self.handle)))
        self._scene = d_scene                   # kept alive: the exposure is destroyed first

    def reset(self):
        """The next auto-exposed tonemap() starts at its target."""
        check(lib().tpt_exposure_reset(self.handle))
        return self

    def histogram(self):
        """The 256 bin counts (uint64) of the last auto-exposed tonemap() on this exposure."""
        bins = np.zeros(256, np.uint64)
        check(lib().tpt_exposure_histogram(self.handle, bins.ctypes.data))
        return bins

    def measure_ms(self) -> float:
        """The duration of that call's measurement kernel."""
        ms = C.c_double()
        check(lib().tpt_exposure_measure_ms(self.handle, C.byref(ms)))
        return ms.value

    def close(self):
        if self.handle:
            lib().tpt_exposure_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _tonemap_params(given: dict):
    """TONEMAP_DEFAULTS overridden by `given` as a tpt_tonemap_params: names are checked here, the
    values' ranges by the library."""
    unknown = sorted(set(given) - set(TONEMAP_DEFAULTS))
    if unknown:
        raise TypeError(f"tonemap: unknown parameter {', '.join(unknown)}; there are {', '.join(TONEMAP_DEFAULTS)}")
    v = dict(TONEMAP_DEFAULTS, **given)
    if v["op"] not in _lib.TONEMAP_OPS:
        raise ValueError(f"tonemap: op must be one of {', '.join(_lib.TONEMAP_OPS)}, got {v['op']!r}")
    if v["transfer"] not in _lib.TONEMAP_TRANSFERS:
        raise ValueError(f"tonemap: transfer must be one of {', '.join(_lib.TONEMAP_TRANSFERS)}, got {v['transfer']!r}")
    flags = (_lib.TONEMAP_AUTO if v["auto"] else 0) | (_lib.TONEMAP_DITHER if v["dither"] else 0)
    return _lib.TonemapParams(_lib.TONEMAP_OPS[v["op"]], _lib.TONEMAP_TRANSFERS[v["transfer"]], flags, float(v["ev"]),
                              float(v["white"]), float(v["gamma"]), float(v["key"]), float(v["p_low"]),
                              float(v["p_high"]), float(v["min_ev"]), float(v["max_ev"]), float(v["rate"]))


class PathTracer:
    """PathTracer (include/path_tracer.h:16-35), headless.

    The reference renders into a 1920x1080 Vulkan window forever, reseeding the
    RNG with time() and drawing 64 spp per frame (path_tracer.cu:556-579).  Here
    render() draws `frames` frames and returns the last one; seed=None keeps the
    reference's time() seeding, an integer makes the frame reproducible."""

    def __init__(self, envLightFile: str = "", width: int = 1920, height: int = 1080, device: int = 0):
        self.m_width, self.m_height, self.device = width, height, device
        self.envLight = EnvLight(envLightFile, device) if envLightFile else None

    def doTrace(self, d_scene: DeviceScene, camera: Camera, framebuffer=None, nSamplesPerPixel: int = 64,
                seed=None, max_depth: int = 8, radiance=None, band=(16, 1, 0), spp_per_launch: int = 0,
                flags: int = 0, refill: int = 0, accumulate: bool = False, pipe_sets: int = 0,
                pipe_chunks: int = 0, lanes_per_pixel: int = 0, leaf_batch: int = 0, wf_slots: int = 0,
                wf_refill: int = 0, band_list=None, band_cost=None):
        """One frame (path_tracer.cu:491-554).  framebuffer/radiance: numpy (host)
        or torch CUDA tensors / raw device pointers (device, int).
        accumulate=True: progressive rendering (TPT_FLAG_ACCUMULATE) -- continue
        the previous call's samples of the same frame; with seed None the
        previous seed is kept (the reference re-seeds from time() every frame).
        band = (band_rows, band_count, band_index): the interleaved deal;
        band_list: an explicit deal (ascending global band ids of band_rows
        rows each; band_count/band_index ignored); band_cost: a float32 array of
        ceil(H / band_rows) entries that receives the rendered bands' costs
        (tpt_params.band_cost, shard.cost_deal)."""
        if not d_scene.built:
            d_scene.build()
        W, H = self.m_width, self.m_height
        if accumulate:
            flags |= _lib.FLAG_ACCUMULATE
            if seed is None:
                seed = getattr(self, "_last_seed", None)
        if seed is None:
            seed = int(time.time())
        self._last_seed = seed
        p = _lib.Params(W, H, nSamplesPerPixel, max_depth, seed, band[0], band[1], band[2], spp_per_launch,
                        flags | _forced_flags(), refill, pipe_sets, pipe_chunks, lanes_per_pixel, leaf_batch, wf_slots,
                        wf_refill)
        keep = _deal_params(p, H, band, band_list, band_cost)  # noqa: F841 (alive through the call)
        st = _lib.Stats()
        env = self.envLight.handle if self.envLight is not None else None
        rad_p = _addr(radiance)
        fb_p = _addr(framebuffer)
        cam = camera.to_c()
        check(lib().tpt_render(d_scene.handle, env, C.byref(cam), C.byref(p), rad_p, fb_p, C.byref(st)))
        return st.as_dict()

    def doTraceFrames(self, d_scene: DeviceScene, camera: Camera, seeds, framebuffers=None,
                      nSamplesPerPixel: int = 64, max_depth: int = 8, radiances=None, band=(16, 1, 0),
                      spp_per_launch: int = 0, flags: int = 0, refill: int = 0, accumulate: bool = False,
                      pipe_sets: int = 0, pipe_chunks: int = 0, lanes_per_pixel: int = 0, leaf_batch: int = 0,
                      wf_slots: int = 0, wf_refill: int = 0, band_list=None, band_cost=None):
        """A batch of independent frames in one trace launch (tpt_render_frames):
        frame f is doTrace(..., seed=seeds[f]) bit for bit.  framebuffers /
        radiances: None or one buffer (or None) per frame.  band / band_list /
        band_cost as in doTrace."""
        if not d_scene.built:
            d_scene.build()
        seeds = [int(x) for x in seeds]
        n = len(seeds)
        if n == 0:
            raise ValueError("no frames")
        if accumulate:
            flags |= _lib.FLAG_ACCUMULATE
        W, H = self.m_width, self.m_height
        p = _lib.Params(W, H, nSamplesPerPixel, max_depth, seeds[0], band[0], band[1], band[2], spp_per_launch,
                        flags | _forced_flags(), refill, pipe_sets, pipe_chunks, lanes_per_pixel, leaf_batch, wf_slots,
                        wf_refill)
        keep = _deal_params(p, H, band, band_list, band_cost)  # noqa: F841
        st = _lib.Stats()
        env = self.envLight.handle if self.envLight is not None else None

        def ptrs(bufs):
            if bufs is None:
                return None
            if len(bufs) != n:
                raise ValueError("need one output buffer per frame")
            arr = (C.c_void_p * n)(*[(_addr(b).value if b is not None else None) for b in bufs])
            return C.cast(arr, C.POINTER(C.c_void_p)), arr

        rp, fp = ptrs(radiances), ptrs(framebuffers)
        cs = (C.c_uint64 * n)(*seeds)
        cam = camera.to_c()
        check(lib().tpt_render_frames(d_scene.handle, env, C.byref(cam), C.byref(p), n, cs,
                                      rp[0] if rp else None, fp[0] if fp else None, C.byref(st)))
        return st.as_dict()

    def doTraceAdaptive(self, d_scene: DeviceScene, camera: Camera, framebuffer=None, *,
                        min_spp: int = ADAPTIVE_DEFAULTS["min_spp"], max_spp: int = ADAPTIVE_DEFAULTS["max_spp"],
                        target: float = ADAPTIVE_DEFAULTS["target"], seed=None, max_depth: int = 8, radiance=None,
                        flags: int = 0, refill: int = 0, lanes_per_pixel: int = 0, leaf_batch: int = 0,
                        tile_spp=None, tile_error=None, stats=None):
        """One frame, every 16x16-pixel tile rendered until its error estimate falls
        below `target` (tpt_render_adaptive): min_spp samples first, then doublings
        up to max_spp = min_spp * 2^j.  Every pixel equals doTrace at its tile's
        sample count, bit for bit.  framebuffer / radiance as in doTrace (at least
        one); tile_spp (int32) / tile_error (float32): optional outputs of
        ceil(H / 16) x ceil(W / 16) entries, row 0 = bottom.  stats: a dict that
        receives tpt_adaptive_stats.  Returns the stats."""
        if not d_scene.built:
            d_scene.build()
        W, H = self.m_width, self.m_height
        if seed is None:
            seed = int(time.time())
        self._last_seed = seed
        # (the wavefront variant takes no tile list: a suite forced through it keeps the megakernel here)
        p = _lib.Params(W, H, 0, max_depth, seed, 16, 1, 0, 0, flags | (_forced_flags() & ~_lib.FLAG_WAVEFRONT),
                        refill, 0, 0, lanes_per_pixel, leaf_batch)
        ap = _lib.AdaptiveParams(min_spp, max_spp, target, 0)
        st = _lib.AdaptiveStats()
        env = self.envLight.handle if self.envLight is not None else None
        cam = camera.to_c()
        check(lib().tpt_render_adaptive(d_scene.handle, env, C.byref(cam), C.byref(p), C.byref(ap), _addr(radiance),
                                        _addr(framebuffer), _addr(tile_spp), _addr(tile_error), C.byref(st)))
        if stats is not None:
            stats.update(st.as_dict())
        return st.as_dict()

    def renderAOV(self, d_scene: DeviceScene, camera: Camera, out=None, stats=None):
        """First-hit feature buffers of the frame (tpt_render_aov): one ray per pixel
        centre through the render's own traversal.  Returns a dict of `albedo`
        [H, W, 3], `normal` [H, W, 3], `depth` [H, W] (float32), `face`, `material`
        [H, W] (int32), row 0 = bottom like the radiance; misses hold albedo 1,
        normal 0, depth 0, face / material -1.  out: a dict with any of those keys
        (numpy arrays or torch CUDA tensors): only these are computed, into the
        given buffers; None: all five, as numpy arrays.  stats: a dict that
        receives `trace_ms`."""
        if not d_scene.built:
            d_scene.build()
        W, H = self.m_width, self.m_height
        out = _aov_out(out, W, H)
        a = _take_guides(out, out, W, H)
        ms = C.c_double()
        cam = camera.to_c()
        check(lib().tpt_render_aov(d_scene.handle, C.byref(cam), W, H, C.byref(a), C.byref(ms)))
        if stats is not None:
            stats["trace_ms"] = ms.value
        return out

    def renderAOVPath(self, d_scene: DeviceScene, camera: Camera, max_bounces: int = AOV_PATH_DEFAULTS["max_bounces"],
                      out=None, stats=None, points: bool = False):
        """Mirror-path feature buffers (tpt_render_aov_path, DESIGN.md section 5
        "Post-pass"): renderAOV continued through up to `max_bounces` perfect mirrors.
        The buffers describe the first surface that is no mirror (or the mirror met at
        the cap): its face, material and normal, the product of every base colour met
        as `albedo`, the distance along the whole path as `depth`; a path that leaves
        the scene holds face / material -1, normal 0, the mirrors' tint and the distance
        to the last mirror.  Returns renderAOV's dict plus `bounces` [H, W] (int32), the
        mirrors followed.  out: as renderAOV's, `bounces` included.  stats: a dict that
        receives trace_ms, followed (pixels with bounces > 0) and deepest.  The result
        guides denoise / denoiseSVGF and temporalPath; temporal stays on renderAOV's
        first-hit buffers.
        points=True (tpt_render_aov_path_points), or a `points` key in out: also `points`
        [H, W, 3] float32, where each path ended -- the terminal world point, or the last
        ray's direction where the path leaves the scene -- which temporalPath needs."""
        if not d_scene.built:
            d_scene.build()
        W, H = self.m_width, self.m_height
        points = bool(points) or (out is not None and "points" in out)
        out = _aov_out(out, W, H, extra=("bounces", "points") if points else ("bounces",))
        if points and out.get("points") is None:
            out["points"] = np.zeros((H, W, 3), np.float32)
        a = _take_guides(out, [k for k in out if k not in ("bounces", "points")], W, H)
        bounces, pts = out.get("bounces"), out.get("points")
        if bounces is not None:
            _check_plane("bounces", bounces, W, H)
        if pts is not None:
            _check_plane("points", pts, W, H)
        p = _lib.AovPathParams(int(max_bounces), 0)
        st = _lib.AovPathStats()
        cam = camera.to_c()
        if pts is not None:
            check(lib().tpt_render_aov_path_points(d_scene.handle, C.byref(cam), W, H, C.byref(p), C.byref(a),
                                                   _addr(bounces), _addr(pts), C.byref(st)))
        else:
            check(lib().tpt_render_aov_path(d_scene.handle, C.byref(cam), W, H, C.byref(p), C.byref(a),
                                            _addr(bounces), C.byref(st)))
        if stats is not None:
            stats.update(st.as_dict())
        return out

    def denoise(self, d_scene: DeviceScene, radiance, aov, iterations: int = DENOISE_DEFAULTS["iterations"],
                sigma_color: float = DENOISE_DEFAULTS["sigma_color"],
                sigma_normal: float = DENOISE_DEFAULTS["sigma_normal"],
                sigma_depth: float = DENOISE_DEFAULTS["sigma_depth"],
                demodulate: bool = DENOISE_DEFAULTS["demodulate"], out=None, framebuffer=None, flags: int = 0,
                stats=None):
        """Edge-avoiding a-trous filter (tpt_denoise, DESIGN.md section 5 "Post-pass")
        of `radiance` [H, W, 3] guided by aov["albedo"], aov["normal"] and
        aov["depth"] (renderAOV).  d_scene supplies the device and keeps the scratch
        planes.  out: the filtered radiance's buffer (may be `radiance` itself;
        None: a new numpy array); framebuffer: optional [H, W, 4] uint8, written as
        doTrace writes it (row 0 = top, B, G, R; alpha untouched).  Buffers are numpy
        arrays or torch CUDA tensors.  Returns `out`; stats: a dict that receives
        pack_ms, filter_ms, resolve_ms."""
        W, H = self.m_width, self.m_height
        _check_plane("radiance", radiance, W, H)
        g = _take_guides(aov, ("albedo", "normal", "depth"), W, H)
        if out is None:
            out = np.zeros((H, W, 3), np.float32)
        _check_plane("radiance", out, W, H)
        if framebuffer is not None:
            _check_plane("framebuffer", framebuffer, W, H)
        p = _lib.DenoiseParams(int(iterations), float(sigma_color), float(sigma_normal), float(sigma_depth),
                               int(flags) | (_lib.DENOISE_DEMODULATE if demodulate else 0))
        st = _lib.DenoiseStats()
        check(lib().tpt_denoise(d_scene.handle, W, H, _addr(radiance), C.byref(g), C.byref(p), _addr(out),
                                _addr(framebuffer), C.byref(st)))
        if stats is not None:
            stats.update(st.as_dict())
        return out

    def temporal(self, history: History, camera: Camera, radiance, aov, *,
                 alpha: float = TEMPORAL_DEFAULTS["alpha"], depth_tol: float = TEMPORAL_DEFAULTS["depth_tol"],
                 normal_min: float = TEMPORAL_DEFAULTS["normal_min"],
                 max_history: int = TEMPORAL_DEFAULTS["max_history"],
                 demodulate: bool = TEMPORAL_DEFAULTS["demodulate"], out=None, variance=None, history_len=None,
                 framebuffer=None, flags: int = 0, stats=None, motion: bool = False, motion_out=None,
                 deform: bool = False):
        """Temporal reprojection and accumulation (tpt_temporal, DESIGN.md section 5
        "Post-pass"): this frame's `radiance` [H, W, 3] and its feature buffers
        aov["normal"], aov["depth"], aov["material"] (and aov["albedo"] with
        demodulate) rendered from `camera`, blended with what `history` holds of the
        previous frames where the previous frame saw the same surface.  out: the
        accumulated radiance's buffer (may be `radiance` itself; None: a new numpy
        array); variance / history_len: optional [H, W] float32 buffers for the
        luminance variance and the history length; framebuffer: optional [H, W, 4]
        uint8 as doTrace writes it.  Buffers are numpy arrays or torch CUDA tensors.
        Returns `out`; stats: a dict that receives kernel_ms and reprojected.
        motion=True (tpt_temporal_motion): objects of the history's scene may have moved
        since the previous call (DeviceScene.set_transforms + build, then this frame's
        render and feature buffers); aov["face"] is needed too, and motion_out, an
        optional [H, W, 2] float32 buffer, receives each pixel's reprojected minus its own
        coordinates in pixels.
        deform=True (tpt_temporal_deform): vertices of the history's scene may have moved since
        the previous deform=True call (DeviceScene.set_vertices + build); the scene must be
        built; aov["face"] and motion_out as for motion=True."""
        W, H = self.m_width, self.m_height
        if motion and deform:
            raise ValueError("motion and deform are two entry points: pick one")
        if motion_out is not None and not (motion or deform):
            raise ValueError("motion_out needs motion=True or deform=True")
        if (history.width, history.height) != (W, H):
            raise ValueError(f"the history is {history.width} x {history.height}, the frame {W} x {H}")
        _check_plane("radiance", radiance, W, H)
        g = _take_guides(aov, (("albedo",) if demodulate else ()) + ("normal", "depth", "material") +
                         (("face",) if motion or deform else ()), W, H)
        if out is None:
            out = np.zeros((H, W, 3), np.float32)
        _check_plane("radiance", out, W, H)
        for name, buf in (("variance", variance), ("history_len", history_len), ("framebuffer", framebuffer),
                          ("motion_out", motion_out)):
            if buf is not None:
                _check_plane(name, buf, W, H)
        p = _lib.TemporalParams(float(alpha), float(depth_tol), float(normal_min), int(max_history),
                                int(flags) | (_lib.TEMPORAL_DEMODULATE if demodulate else 0))
        st = _lib.TemporalStats()
        cam = camera.to_c()
        if motion or deform:
            entry = lib().tpt_temporal_motion if motion else lib().tpt_temporal_deform
            check(entry(history.handle, C.byref(cam), _addr(radiance), C.byref(g), C.byref(p),
                        _addr(out), _addr(variance), _addr(history_len), _addr(motion_out),
                        _addr(framebuffer), C.byref(st)))
        else:
            check(lib().tpt_temporal(history.handle, C.byref(cam), _addr(radiance), C.byref(g), C.byref(p), _addr(out),
                                     _addr(variance), _addr(history_len), _addr(framebuffer), C.byref(st)))
        if stats is not None:
            stats.update(st.as_dict())
        return out

    def temporalPath(self, history: History, camera: Camera, radiance, aov, bounces=None, points=None, *,
                     alpha: float = TEMPORAL_PATH_DEFAULTS["alpha"],
                     depth_tol: float = TEMPORAL_PATH_DEFAULTS["depth_tol"],
                     normal_min: float = TEMPORAL_PATH_DEFAULTS["normal_min"],
                     max_history: int = TEMPORAL_PATH_DEFAULTS["max_history"],
                     demodulate: bool = TEMPORAL_PATH_DEFAULTS["demodulate"],
                     point_tol: float = TEMPORAL_PATH_DEFAULTS["point_tol"], out=None, variance=None,
                     history_len=None, framebuffer=None, flags: int = 0, stats=None):
        """temporal on mirror-path guides (tpt_temporal_path, DESIGN.md section 5 "Temporal
        accumulation through mirrors"): reflections in perfect mirrors keep their history while
        the camera moves.  aov: renderAOVPath(..., points=True)'s buffers -- normal, depth (the
        path's length) and material, albedo with demodulate; bounces / points default to
        aov["bounces"] / aov["points"].  A pixel that followed k mirrors accepts a tap only
        where the previous frame followed k mirrors to the same material and its terminal
        world point lies within point_tol pixel footprints; with k = 0 the rules are
        temporal's.  Everything else -- out, variance, history_len, framebuffer, stats, the
        buffers' types -- is temporal's.  The history may alternate between temporal and
        temporalPath: after a temporal call the mirror pixels start over.  Objects that moved
        are not followed: reset the history, or use temporal(motion=True)."""
        W, H = self.m_width, self.m_height
        if (history.width, history.height) != (W, H):
            raise ValueError(f"the history is {history.width} x {history.height}, the frame {W} x {H}")
        _check_plane("radiance", radiance, W, H)
        g = _take_guides(aov, (("albedo",) if demodulate else ()) + ("normal", "depth", "material"), W, H)
        bounces = aov.get("bounces") if bounces is None else bounces
        points = aov.get("points") if points is None else points
        if out is None:
            out = np.zeros((H, W, 3), np.float32)
        _check_plane("radiance", out, W, H)
        for name, buf in (("bounces", bounces), ("points", points), ("variance", variance),
                          ("history_len", history_len), ("framebuffer", framebuffer)):
            if buf is not None:
                _check_plane(name, buf, W, H)
        p = _lib.TemporalPathParams(float(alpha), float(depth_tol), float(normal_min), int(max_history),
                                    int(flags) | (_lib.TEMPORAL_DEMODULATE if demodulate else 0), float(point_tol))
        st = _lib.TemporalStats()
        cam = camera.to_c()
        check(lib().tpt_temporal_path(history.handle, C.byref(cam), _addr(radiance), C.byref(g), _addr(bounces),
                                      _addr(points), C.byref(p), _addr(out), _addr(variance), _addr(history_len),
                                      _addr(framebuffer), C.byref(st)))
        if stats is not None:
            stats.update(st.as_dict())
        return out

    def denoiseSVGF(self, d_scene: DeviceScene, radiance, aov, variance=None, history_len=None, *,
                    iterations: int = SVGF_DEFAULTS["iterations"], sigma_lum: float = SVGF_DEFAULTS["sigma_lum"],
                    sigma_normal: float = SVGF_DEFAULTS["sigma_normal"],
                    sigma_depth: float = SVGF_DEFAULTS["sigma_depth"],
                    min_history: int = SVGF_DEFAULTS["min_history"],
                    demodulate: bool = SVGF_DEFAULTS["demodulate"], out=None, variance_out=None, framebuffer=None,
                    flags: int = 0, stats=None):
        """Variance-guided a-trous filter (tpt_denoise_svgf, DESIGN.md section 5
        "Post-pass") of `radiance` [H, W, 3] guided by aov["normal"], aov["depth"] (and
        aov["albedo"] with demodulate) and by temporal()'s `variance` and `history_len`
        [H, W] float32: a pixel whose history is shorter than min_history takes a spatial
        variance estimate instead.  variance None: every pixel does; history_len None
        with a variance: none does.  Run temporal() and this with the same
        `demodulate`.  out: the filtered radiance's buffer (may be `radiance` itself;
        None: a new numpy array); variance_out: optional [H, W] float32 for the
        filtered variance (may be `variance`); framebuffer: optional [H, W, 4] uint8 as
        doTrace writes it.  Buffers are numpy arrays or torch CUDA tensors.  Returns
        `out`; stats: a dict that receives pack_ms, estimate_ms, filter_ms, resolve_ms
        and estimated."""
        W, H = self.m_width, self.m_height
        if history_len is not None and variance is None:
            raise ValueError("history_len needs a variance")
        _check_plane("radiance", radiance, W, H)
        g = _take_guides(aov, ("albedo", "normal", "depth") if demodulate else ("normal", "depth"), W, H)
        if out is None:
            out = np.zeros((H, W, 3), np.float32)
        _check_plane("radiance", out, W, H)
        for name, buf in (("variance", variance), ("history_len", history_len), ("variance", variance_out),
                          ("framebuffer", framebuffer)):
            if buf is not None:
                _check_plane(name, buf, W, H)
        p = _lib.SvgfParams(int(iterations), float(sigma_lum), float(sigma_normal), float(sigma_depth),
                            int(min_history), int(flags) | (_lib.SVGF_DEMODULATE if demodulate else 0))
        st = _lib.SvgfStats()
        check(lib().tpt_denoise_svgf(d_scene.handle, W, H, _addr(radiance), C.byref(g), _addr(variance),
                                     _addr(history_len), C.byref(p), _addr(out), _addr(variance_out),
                                     _addr(framebuffer), C.byref(st)))
        if stats is not None:
            stats.update(st.as_dict())
        return out

    def upsample(self, d_scene: DeviceScene, radiance_low, aov_low, aov, *,
                 sigma_normal: float = UPSAMPLE_DEFAULTS["sigma_normal"],
                 sigma_depth: float = UPSAMPLE_DEFAULTS["sigma_depth"],
                 demodulate: bool = UPSAMPLE_DEFAULTS["demodulate"], out=None, framebuffer=None, stats=None,
                 low_size=None):
        """Guided upsampling (tpt_upsample, DESIGN.md section 5 "Guided upsampling") of
        `radiance_low` [hl, wl, 3], a render of this tracer's camera at a smaller size, to this
        tracer's frame size: aov_low are the feature buffers at the low size, aov those at the
        full size (renderAOV or renderAOVPath of a tracer of each size) -- normal, depth and
        material, and albedo with demodulate.  The low size is radiance_low's shape; low_size =
        (wl, hl) names it for a raw device pointer.  out: the full-size radiance's buffer (None:
        a new numpy array); framebuffer: optional [H, W, 4] uint8 as doTrace writes it.  Buffers
        are numpy arrays or torch CUDA tensors.  Returns `out`; stats: a dict that receives
        kernel_ms and fallback (the pixels no tap of which holds their material: plain bilinear)."""
        W, H = self.m_width, self.m_height
        if low_size is None:
            shape = tuple(getattr(radiance_low, "shape", ()))
            if len(shape) != 3 or shape[2] != 3:
                raise ValueError(f"radiance_low: need [hl, wl, 3] (or low_size=(wl, hl)), got shape {shape}")
            low_size = (shape[1], shape[0])
        wl, hl = int(low_size[0]), int(low_size[1])
        if not (1 <= wl <= W and 1 <= hl <= H):
            raise ValueError(f"the low size {wl} x {hl} must be within 1 x 1 .. {W} x {H}")
        _check_plane("radiance", radiance_low, wl, hl)
        keys = (("albedo",) if demodulate else ()) + ("normal", "depth", "material")
        gl = _take_guides(aov_low, keys, wl, hl)
        g = _take_guides(aov, keys, W, H)
        if out is None:
            out = np.zeros((H, W, 3), np.float32)
        _check_plane("radiance", out, W, H)
        if framebuffer is not None:
            _check_plane("framebuffer", framebuffer, W, H)
        p = _lib.UpsampleParams(float(sigma_normal), float(sigma_depth),
                                _lib.UPSAMPLE_DEMODULATE if demodulate else 0)
        st = _lib.UpsampleStats()
        check(lib().tpt_upsample(d_scene.handle, wl, hl, _addr(radiance_low), C.byref(gl), W, H, C.byref(g),
                                 C.byref(p), _addr(out), _addr(framebuffer), C.byref(st)))
        if stats is not None:
            stats.update(st.as_dict())
        return out

    def tonemap(self, d_scene: DeviceScene, radiance, *, exposure=None, out=None, bgra=None, stats=None, **params):
        """The display stage (tpt_tonemap, DESIGN.md section 5 "Tone mapping") of `radiance`
        [H, W, 3]: exposure, tone curve, transfer function, and rounding to bytes.  params override
        TONEMAP_DEFAULTS: op "linear" | "reinhard" | "aces", transfer "none" | "srgb" | "gamma",
        auto (measure the frame's exposure; else the scale is 2^ev), dither, ev, white, gamma, key,
        p_low, p_high, min_ev, max_ev, rate.  exposure: an Exposure that carries the adapted value
        across auto-exposed frames (None: each frame stands alone).  out: the buffer of the
        mapped colours in [0, 1], [H, W, 3] float32; it may be `radiance` itself.  bgra: [H, W, 4]
        uint8 as doTrace writes it, alpha untouched.  With neither, a new numpy array is `out`.
        Buffers are numpy arrays or torch CUDA tensors.  Returns `out`, or `bgra` where only that
        was given; stats: a dict that receives hist_ms, map_ms, log2_scale, scale, log2_avg,
        counted, dark and nonfinite."""
        W, H = self.m_width, self.m_height
        p = _tonemap_params(params)
        if exposure is not None and not isinstance(exposure, Exposure):
            raise TypeError(f"exposure: need an Exposure or None, got {type(exposure).__name__}")
        _check_plane("radiance", radiance, W, H)
        if out is None and bgra is None:
            out = np.zeros((H, W, 3), np.float32)
        if out is not None:
            _check_plane("radiance", out, W, H)
        if bgra is not None:
            _check_plane("framebuffer", bgra, W, H)
        st = _lib.TonemapStats()
        check(lib().tpt_tonemap(d_scene.handle, exposure.handle if exposure is not None else None, W, H,
                                _addr(radiance), C.byref(p), _addr(out), _addr(bgra), C.byref(st)))
        if stats is not None:
            stats.update(st.as_dict())
        return out if out is not None else bgra

    def render(self, meshFile: str, nSamplesPerPixel: int = 64, seed=None, max_depth: int = 8, frames: int = 1):
        scene = Scene(meshFile, "gltf")
        d_scene = scene.copySceneToDevice(self.device).build()
        fb = np.zeros((self.m_height, self.m_width, 4), np.uint8)
        fb[..., 3] = 255
        rad = np.zeros((self.m_height, self.m_width, 3), np.float32)
        stats = {}
        for _ in range(frames):
            stats = self.doTrace(d_scene, scene.m_camera, fb, nSamplesPerPixel, seed, max_depth, rad)
        d_scene.close()
        return Frame(fb, rad, stats)


# Test hook: OR-ed into every render's flags, so a whole parity suite can run
# through a variant.  Only tests/conftest.py sets it (from TPT_TEST_FORCE_FLAGS,
# e.g. 32 = TPT_FLAG_WAVEFRONT); the library itself reads no environment.
test_force_flags = 0


def _forced_flags() -> int:
    return int(test_force_flags)


def _deal_params(p, height, band, band_list, band_cost):
    """Fill tpt_params' explicit deal / cost output; returns the ctypes buffers
    that must stay alive through the call."""
    keep = []
    if band_list is not None:
        arr = (C.c_int32 * max(len(band_list), 1))(*[int(b) for b in band_list])
        p.band_list_len = len(band_list)
        p.band_list = C.cast(arr, C.POINTER(C.c_int32))
        keep.append(arr)
    if band_cost is not None:
        nb = (height + band[0] - 1) // band[0]
        if not (isinstance(band_cost, np.ndarray) and band_cost.dtype == np.float32 and band_cost.size == nb
                and band_cost.flags["C_CONTIGUOUS"]):
            raise ValueError(f"band_cost: a contiguous float32 array of {nb} entries")
        p.band_cost = band_cost.ctypes.data_as(C.POINTER(C.c_float))
        keep.append(band_cost)
    return keep


def _addr(buf):
    if buf is None:
        return None
    if isinstance(buf, int):
        return C.c_void_p(buf)
    if isinstance(buf, np.ndarray):
        if not buf.flags["C_CONTIGUOUS"]:
            raise ValueError("output buffers must be contiguous")
        return C.c_void_p(buf.ctypes.data)
    if hasattr(buf, "data_ptr"):             # torch tensor (device memory)
        if not buf.is_contiguous():
            raise ValueError("output tensors must be contiguous")
        if getattr(buf, "is_cuda", False):
            # the library writes device outputs on its own stream (tpt.h): work the
            # caller queued on torch's stream (allocation fill, earlier reads) must be
            # done first
            import torch
            torch.cuda.current_stream(buf.device).synchronize()
        return C.c_void_p(buf.data_ptr())
    raise TypeError(f"unsupported buffer type {type(buf)}")
