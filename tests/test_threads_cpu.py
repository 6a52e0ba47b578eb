"""tpt_last_error() is per thread (include/tpt.h), through the real libtpt.so and without a
device: four threads fail calls that return before any device work -- tpt_gltf_load and
tpt_image_load on missing paths of their own, tpt_env_create without texels -- and each reads
its own status and message back after every call, while a fifth loads and frees tir.gltf.
ctypes releases the GIL in every call, so the calls and the reads of different threads
interleave."""
import ctypes as C
import os
import threading

import numpy as np

import tinypathtracer_amd as T
from tests.conftest import scene_path
from tinypathtracer_amd import _lib

ITERATIONS = 500
LOADS = 100
ERR_INVALID_ARG, ERR_IO = 1, 4
ARRAYS = ("indices", "vertices", "normals", "lut", "vert_trans", "normal_trans", "materials")


def _scene_arrays(scene):
    cam = scene.m_camera
    return [np.asarray(getattr(scene, k)) for k in ARRAYS] + \
        [np.asarray(cam.c2w, np.float32), np.array([cam.vfov, cam.aspect, cam.znear], np.float32)]


def test_last_error_is_per_thread(tmp_path):
    L = T.lib()
    serial = _scene_arrays(T.Scene(scene_path("tir")))
    failures = []          # (thread, iteration, what)
    start = threading.Barrier(5)

    def missing_gltf(name):
        path = os.fsencode(str(tmp_path / name))
        h = C.c_void_p()
        return lambda: L.tpt_gltf_load(path, C.byref(h)), ERR_IO, path.decode()

    def missing_image(name):
        path = os.fsencode(str(tmp_path / name))
        px, w, h = C.POINTER(C.c_uint8)(), C.c_int32(), C.c_int32()
        return lambda: L.tpt_image_load(path, C.byref(px), C.byref(w), C.byref(h)), ERR_IO, path.decode()

    def empty_env():
        h = C.c_void_p()
        return lambda: L.tpt_env_create(None, 0, 0, 0, C.byref(h)), ERR_INVALID_ARG, "bad env arguments"

    def failing(tid, call, status, text):
        try:
            start.wait()
            for it in range(ITERATIONS):
                st = call()
                msg = L.tpt_last_error().decode(errors="replace")
                if st != status or text not in msg:
                    failures.append((tid, it, f"status {st} (want {status}), message {msg!r} (want {text!r} in it)"))
                    return
        except Exception as e:   # a thread's exception would otherwise be lost
            failures.append((tid, -1, repr(e)))

    def loading(tid):
        try:
            start.wait()
            for it in range(LOADS):
                got = _scene_arrays(T.Scene(scene_path("tir")))
                if len(got) != len(serial) or not all(np.array_equal(a, b) and a.dtype == b.dtype
                                                      for a, b in zip(got, serial)):
                    failures.append((tid, it, "tir.gltf loaded differently from the serial load"))
                    return
        except Exception as e:
            failures.append((tid, -1, repr(e)))

    threads = [threading.Thread(daemon=True, target=failing, args=(0, *missing_gltf("missing_scene_0.gltf"))),
               threading.Thread(daemon=True, target=failing, args=(1, *missing_image("missing_image_1.jpg"))),
               threading.Thread(daemon=True, target=failing, args=(2, *missing_gltf("missing_scene_2.gltf"))),
               threading.Thread(daemon=True, target=failing, args=(3, *empty_env())),
               threading.Thread(daemon=True, target=loading, args=(4,))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not any(t.is_alive() for t in threads), "a thread did not finish"
    assert failures == []
    assert _lib.STATUS_NAMES[ERR_IO] == "IO" and _lib.STATUS_NAMES[ERR_INVALID_ARG] == "INVALID_ARG"
