"""rt_scene_update on host-only scenes (RT_DEVICE_NONE): after every step of a deformation sequence the updated
scene holds what a scene freshly created from the same mesh description holds -- the reference boxes with their
face order, the per-face flags and the certificate range, the ray bounds -- its refit trees are sound, a tree
without clipped leaves returns to its original bytes when the vertices do, and what the call refuses leaves the
scene untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import update_scenes as U
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "rt", "rt_api.h")
RT_OK, RT_ERR_INVALID, RT_ERR_UNSUPPORTED = 0, -1, -6
NONE = -2  # RT_DEVICE_NONE
SYMBOLS = ("rt_scene_update", "rt_debug_scene_records")


def host_scene(rt, mesh, M=None, **kw):
    return rt.Scene(mesh, device=NONE, shape_model_matrix=M, **kw)


def images(sc):
    return [sc.records(which).copy() for which in range(3)]


def test_header_declares_and_library_exports(rt):
    text = open(HEADER).read()
    assert re.search(r"^#define RT_HAS_SCENE_UPDATE 1\b", text, re.M)
    assert re.search(r"^#define RT_API_VERSION 4\b", text, re.M) and rt.lib().rt_version() == 4
    assert re.search(r"typedef struct rt_update_stats \{", text)
    for name in SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(" % name, text, re.M), name
        assert hasattr(rt.lib(), name), name
        assert name in rt.EXPORTS
    # six phase times, the path taken (padded to 8 bytes), the SAH cost
    assert C.sizeof(rt.UpdateStats) == 64 and rt.UpdateStats.sah_cost.offset == 56


@pytest.mark.parametrize("name", U.SCENES)
def test_update_equals_fresh_host_scene(rt, name):
    arr, M, seq = U.scene_steps(rt, name)
    builder = rt.RT_BUILDER_SBVH if name == "bunny" else rt.RT_BUILDER_SAH  # the bunny: spatial splits
    sc = host_scene(rt, U.mesh_of(rt, arr), M, builder=builder)
    prev = sc.ref_boxes()
    changed = []
    for step, v in enumerate(seq):
        if name == "tie":
            assert U.tie_copies_coincide(v)  # the ties survive the rigid shift
        mesh = U.mesh_of(rt, arr, v)
        st = sc.update(mesh, model_matrix=M, stats=True)
        assert st["bounds_on_device"] == 0 and st["total_ms"] > 0
        fresh = host_scene(rt, mesh, M, builder=builder)
        got, want = sc.ref_boxes(), fresh.ref_boxes()
        for a, b in zip(got, want):
            assert np.array_equal(a, b), (name, step)
        changed.append(len(got[0]) != len(prev[0]) or not np.array_equal(got[2], prev[2]))
        prev = got
        (ff, ro), (wf, wro) = sc.face_flags(), fresh.face_flags()
        assert np.array_equal(ff, wf) and ro == wro, (name, step)
        assert np.array_equal(sc.ray_bounds(), fresh.ray_bounds()), (name, step)
        val = sc.validate_bvh()
        assert val["ok"] and val["violations"] == 0, (name, step, val)
        assert val["nodes4"] > 0 and val["covered4"] == val["covered2"]  # the host-built scene's quantised tree
        # the refit tree is the fresh tree's topology only when nothing moved; its cost is reported either way
        assert st["sah_cost"] == pytest.approx(sc.tree_cost()["sah"], rel=0, abs=0)
        assert sc.info()["n_ref_boxes"] == len(got[0])
    if name == "bunny":
        assert any(changed), "no step changed the reference-box partition: the check would be vacuous"


@pytest.mark.parametrize("name", U.SCENES)
def test_away_and_back_restores_the_records(rt, name):
    """RT_BUILDER_SAH keeps every triangle whole in one leaf, so the refit boxes are the builder's own boxes:
    back at the original vertices all three record images are the original bytes."""
    arr, M, seq = U.scene_steps(rt, name)
    sc = host_scene(rt, U.mesh_of(rt, arr), M, builder=rt.RT_BUILDER_SAH)
    first = images(sc)
    moved = False
    for v in seq:
        sc.update(U.mesh_of(rt, arr, v), model_matrix=M)
        now = images(sc)
        moved = moved or not np.array_equal(now[1], first[1])
    assert moved
    for a, b in zip(first, now):
        assert np.array_equal(a, b)


def test_model_matrix_change_and_back(rt):
    """A rotated and stretched model matrix tilts the normals against their world triangles (accept-region bounds,
    no certificates); back at the normalised matrix the certificates return."""
    arr = U.scene_arrays(rt, "cornell")
    mesh = U.mesh_of(rt, arr)
    M0 = mesh.export()["M16"]
    sc = host_scene(rt, mesh, builder=rt.RT_BUILDER_SAH)
    first = images(sc)
    assert sc.face_flags()[1] > 0
    M1 = U.rotated_stretched(M0)
    sc.update(mesh, model_matrix=M1)
    fresh = host_scene(rt, mesh, M1, builder=rt.RT_BUILDER_SAH)
    assert sc.face_flags()[1] == fresh.face_flags()[1] == 0.0
    assert np.array_equal(sc.face_flags()[0], fresh.face_flags()[0])
    assert np.array_equal(sc.ray_bounds(), fresh.ray_bounds())
    assert sc.validate_bvh()["ok"]  # (the validator bounds the accept region where the scene carries one)
    sc.update(mesh, model_matrix=M0)
    for a, b in zip(images(sc), first):
        assert np.array_equal(a, b)


def test_refusals_leave_the_scene_untouched(rt):
    arr = U.scene_arrays(rt, "cornell")
    v, f, mats, groups = arr
    sc = host_scene(rt, U.mesh_of(rt, arr), builder=rt.RT_BUILDER_SAH)
    first = images(sc)
    boxes = sc.ref_boxes()
    L = rt.lib()
    fewer = rt.Mesh.from_arrays(v, f[:-1], mats, groups=[(len(f) - 1, groups[0][1])] if len(groups) == 1 else
                                groups[:-1] + [(groups[-1][0] - 1, groups[-1][1])])
    f2 = f.copy()
    f2[3] = f2[3][[1, 2, 0]]  # the same triangle, another first vertex: one changed face id
    other_face = rt.Mesh.from_arrays(v, f2, mats, groups=groups)
    more_mats = rt.Mesh.from_arrays(v, f, np.concatenate([mats, mats[:1]]), groups=groups)
    for bad in (fewer, other_face, more_mats):
        d = bad.desc()
        assert L.rt_scene_update(sc.h, C.byref(d), None) == RT_ERR_INVALID
        for a, b in zip(images(sc), first):
            assert np.array_equal(a, b)
        for a, b in zip(sc.ref_boxes(), boxes):
            assert np.array_equal(a, b)
    d = U.mesh_of(rt, arr).desc()
    assert L.rt_scene_update(None, C.byref(d), None) == RT_ERR_INVALID
    assert L.rt_scene_update(sc.h, None, None) == RT_ERR_INVALID
    n = C.c_int64(0)
    assert L.rt_debug_scene_records(None, 0, 0, None, C.byref(n)) == RT_ERR_INVALID
    assert L.rt_debug_scene_records(sc.h, 0, 0, None, None) == RT_ERR_INVALID
    assert L.rt_debug_scene_records(sc.h, 3, 0, None, C.byref(n)) == RT_ERR_INVALID
    assert L.rt_debug_scene_records(sc.h, 0, 0, None, C.byref(n)) == RT_OK and n.value == 64 * sc.info()["bvh_nodes"]
    small = np.zeros(16, np.uint8)
    assert L.rt_debug_scene_records(sc.h, 0, 16, small.ctypes.data_as(C.c_void_p), C.byref(n)) == RT_ERR_INVALID
    wide = host_scene(rt, U.mesh_of(rt, arr), wide_tree=1)
    assert L.rt_scene_update(wide.h, C.byref(d), None) == RT_ERR_UNSUPPORTED
    assert "wide_tree" in L.rt_last_error().decode()


def test_nan_coordinate_takes_the_host_path(rt):
    arr = U.scene_arrays(rt, "cornell")
    sc = host_scene(rt, U.mesh_of(rt, arr), builder=rt.RT_BUILDER_SAH)
    v = U.deform(arr[0], U.AMPLITUDES[0])
    v[5, 1] = np.nan
    mesh = U.mesh_of(rt, arr, v)
    M = U.mesh_of(rt, arr).export()["M16"]  # (the loader's normalisation of a NaN extent is no matrix to test with)
    st = sc.update(mesh, model_matrix=M, stats=True)
    assert st["bounds_on_device"] == 0
    fresh = host_scene(rt, mesh, M, builder=rt.RT_BUILDER_SAH)
    for a, b in zip(sc.ref_boxes(), fresh.ref_boxes()):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(sc.face_flags()[0], fresh.face_flags()[0])

    def by_face(s):  # the triangle records (16 words, face id in word 14) in face order, as bytes: NaN patterns compare
        r = s.records(1).view(np.uint32).reshape(-1, 16)
        return r[np.argsort(r[:, 14], kind="stable")]

    assert np.array_equal(by_face(sc), by_face(fresh))


def test_single_leaf_scene_keeps_its_sentinel(rt):
    """Two faces under leaf size 4: the root is one leaf wrapped with a never-hit sentinel child, which a refit
    leaves alone."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]], np.float32)
    f = np.array([[0, 1, 2], [1, 3, 2]], np.uint32)
    mats = np.array([[0.1] * 3 + [0.7] * 3 + [0.2] * 3 + [16.0, 1.0, 1.0]], np.float32)
    arr = (v, f, mats, [(2, 0)])
    sc = host_scene(rt, U.mesh_of(rt, arr), builder=rt.RT_BUILDER_SAH)
    assert sc.info()["bvh_nodes"] == 1
    first = images(sc)
    v2 = v.copy()
    v2[3, 2] = 2.0
    sc.update(U.mesh_of(rt, arr, v2))
    val = sc.validate_bvh()
    assert val["ok"] and val["covered2"] == 2
    now = images(sc)
    assert not np.array_equal(now[0][:24], first[0][:24])  # child 0: the leaf's new box
    assert np.array_equal(now[0][24:], first[0][24:])      # child 1: the sentinel, and the handles
    sc.update(U.mesh_of(rt, arr))
    for a, b in zip(images(sc), first):
        assert np.array_equal(a, b)
