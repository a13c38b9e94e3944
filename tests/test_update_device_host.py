"""rt_scene_update_device without a GPU: the header and the export, what the call refuses before it touches anything
(NULL arguments, a host-only scene, which stays byte for byte what it was), and the per-face flags of host-only
scenes held to a fixture recorded before their arithmetic moved into the RT_HD functions the device update's
kernels share with the host stages (rt_faceflags.h; tools/gen_face_flags_golden.py wrote the fixture)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import update_scenes as U
from conftest import GOLDEN, ROOT

HEADER = os.path.join(ROOT, "include", "rt", "rt_api.h")
RT_OK, RT_ERR_INVALID, RT_ERR_NO_DEVICE = 0, -1, -5
NONE = -2  # RT_DEVICE_NONE


def host_scene(rt, mesh, M=None, **kw):
    return rt.Scene(mesh, device=NONE, shape_model_matrix=M, **kw)


def test_header_declares_and_library_exports(rt):
    text = open(HEADER).read()
    assert re.search(r"^#define RT_HAS_DEVICE_UPDATE 1\b", text, re.M)
    assert re.search(r"^#define RT_API_VERSION 4\b", text, re.M) and rt.lib().rt_version() == 4
    assert re.search(r"typedef struct rt_device_geometry \{", text)
    assert re.search(r"^int\s+rt_scene_update_device\s*\(", text, re.M)
    assert hasattr(rt.lib(), "rt_scene_update_device")
    assert "rt_scene_update_device" in rt.EXPORTS
    assert C.sizeof(rt.DeviceGeometry) == 5 * C.sizeof(C.c_void_p)
    # the codes the refusals below are held to
    assert re.search(r"RT_ERR_INVALID\s*=\s*-1\b", text) and re.search(r"RT_ERR_NO_DEVICE\s*=\s*-5\b", text)


def test_null_arguments_are_invalid(rt):
    L = rt.lib()
    sc = host_scene(rt, U.mesh_of(rt, U.scene_arrays(rt, "cornell")))
    g = rt.DeviceGeometry()
    assert L.rt_scene_update_device(None, C.byref(g), None, None) == RT_ERR_INVALID
    assert L.rt_scene_update_device(sc.h, None, None, None) == RT_ERR_INVALID
    # a NULL array while the count is positive: before the scene's kind is looked at
    assert L.rt_scene_update_device(sc.h, C.byref(g), None, None) == RT_ERR_INVALID
    buf = np.zeros(4, np.float32)
    for missing in ("vertices", "vertex_normals", "face_normals"):
        g = rt.DeviceGeometry()
        for f in ("vertices", "vertex_normals", "face_normals"):
            setattr(g, f, None if f == missing else buf.ctypes.data)
        assert L.rt_scene_update_device(sc.h, C.byref(g), None, None) == RT_ERR_INVALID, missing
        assert "null" in L.rt_last_error().decode()


def test_host_only_scene_is_refused_and_unchanged(rt):
    L = rt.lib()
    arr = U.scene_arrays(rt, "cornell")
    sc = host_scene(rt, U.mesh_of(rt, arr), builder=rt.RT_BUILDER_SAH)
    before = [sc.records(w).copy() for w in range(3)]
    boxes = [a.copy() for a in sc.ref_boxes()]
    flags = sc.face_flags()
    buf = np.zeros(16, np.float32)  # (never read: the refusal comes before the pointers are looked at)
    g = rt.DeviceGeometry()
    g.vertices = g.vertex_normals = g.face_normals = buf.ctypes.data
    st = rt.UpdateStats()
    assert L.rt_scene_update_device(sc.h, C.byref(g), None, C.byref(st)) == RT_ERR_NO_DEVICE
    assert "host-only" in L.rt_last_error().decode()
    for w in range(3):
        assert np.array_equal(sc.records(w), before[w]), w
    for a, b in zip(sc.ref_boxes(), boxes):
        assert np.array_equal(a, b)
    ff, ro = sc.face_flags()
    assert np.array_equal(ff, flags[0]) and ro == flags[1]
    # ... and it still updates on the host
    sc.update(U.mesh_of(rt, arr, U.steps(arr)[0]))
    assert sc.validate_bvh()["ok"]


@pytest.mark.parametrize("name", U.SCENES)
def test_shared_flag_functions_keep_the_host_flags(rt, name):
    """Created and updated host-only scenes carry the flags (and the certificate range) of the build before the
    flag arithmetic was shared with the device."""
    want = np.load(os.path.join(GOLDEN, "face_flags.npz"))
    arr, M, seq = U.scene_steps(rt, name)
    sc = host_scene(rt, U.mesh_of(rt, arr), M, builder=rt.RT_BUILDER_SAH)
    for k, v in enumerate([None] + list(seq)):
        if v is not None:
            sc.update(U.mesh_of(rt, arr, v), model_matrix=M)
        ff, ro = sc.face_flags()
        assert np.array_equal((ff >> 30).astype(np.uint8), want[f"{name}_{k}_flags"]), (name, k)
        assert np.float32(ro) == want[f"{name}_{k}_ro"][0], (name, k)
        if v is not None:  # a freshly created scene agrees (create and update run the same stages)
            fresh = host_scene(rt, U.mesh_of(rt, arr, v), M, builder=rt.RT_BUILDER_SAH)
            assert np.array_equal(fresh.face_flags()[0], ff), (name, k)


def test_the_fixture_exercises_both_bits():
    want = np.load(os.path.join(GOLDEN, "face_flags.npz"))
    seen = np.zeros(4, np.int64)
    for key in want.files:
        if key.endswith("_flags"):
            seen += np.bincount(want[key], minlength=4)[:4]
    assert seen[3] > 0 and seen[2] > 0 and (seen[0] > 0 or seen[1] > 0)  # certified, safe only, not safe
