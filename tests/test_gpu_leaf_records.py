"""Leaf records of the fused PRIMARY kernel (MI355X): its binary-only instantiation (scenes without the 4-wide tree)
and its wide instantiation, on tiny frames of meshes whose leaves hold 1..16 records. (Scenes are built without and
with the wide tree, which is what launch_frame chooses the instantiation by; which one ran is not observable through
the API and is not asserted.)

Bar: through rt_render with hit records, face id and t bits equal the CPU oracle's on every pixel and colours are
within test_gpu_parity's tolerance; each frame is byte-identical to the same frame rendered by the two-kernel
PRIMARY (variant 32768 of VB_PRIMARY_UNFUSED, whose trace kernel keeps the plain leaf loop; the product and the
variants library both have it). Frames: 64x64 and 40x24 (partial tiles, inactive lanes). What each fixture's tree
holds is asserted on the host build in tests/test_leaf_records_host.py (leaf histogram, duplicates, last leaf).
"""
import numpy as np
import pytest

import edge_scenes as E
import leaf_scenes as LS
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu
FRAMES = ((64, 64), (40, 24))
SPLIT_PRIMARY = 32768


@pytest.fixture(scope="module", autouse=True)
def need_gpu(rt):
    if rt.device_count() == 0:
        pytest.skip("no GPU")


def fixtures():
    """name -> (mesh arrays, vertex normals or None, camera dz)."""
    normal, vn, _ = E.normal_scene()
    return {"stack": (LS.stack_scene()[0], None, LS.STACK_DZ), "tie": (E.tie_scene()[0], None, 20.0),
            "normals": (normal, vn, 20.0), "one": (LS.one_triangle(), None, 20.0), "empty": (LS.empty(), None, 20.0)}


@pytest.fixture(scope="module")
def reference(orc):
    """The oracle's frames of every fixture, computed once: name -> {(W, H): (rgb, face, t)}."""
    out = {}
    for name, ((v, f, m, g), vn, dz) in fixtures().items():
        if name == "empty":
            continue
        osc = orc.Scene(orc.Mesh.from_arrays(v, f, m, vn3=vn, groups=g))
        out[name] = {(W, H): osc.render(orc.flycam(W, H, 0, 0, dz), orc.DEFAULT_LIGHTS, W, H, full=False) for W, H in FRAMES}
    return out


def check_scene(rt, reference, name, leaf, wide):
    (v, f, m, g), vn, dz = fixtures()[name]
    sc = rt.Scene(rt.Mesh.from_arrays(v, f, m, vn3=vn, groups=g), builder=rt.RT_BUILDER_SBVH, leaf_size=leaf, wide_tree=wide)
    for W, H in FRAMES:
        cam = rt.flycam(W, H, 0, 0, dz)
        got = sc.render(cam, rt.DEFAULT_LIGHTS, W, H, want_hits=True)
        prev = rt.set_variant(SPLIT_PRIMARY)
        try:
            two = sc.render(cam, rt.DEFAULT_LIGHTS, W, H, want_hits=True)
        finally:
            rt.set_variant(prev)
        what = f"{name} leaf {leaf} wide {wide} {W}x{H}"
        for a, b in zip(got[:3], two[:3]):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), f"{what}: fused and two-kernel PRIMARY differ"
        if name == "empty":
            assert (got[1] == -1).all() and np.isinf(got[2]).all(), what
            np.testing.assert_array_equal(got[0], np.float32(0.9))
        else:
            compare(*got[:3], *reference[name][(W, H)], what)
            assert (np.asarray(got[1]) >= 0).any(), what


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("leaf", LS.LEAF_BOUNDS)
def test_leaf_sizes_match_the_oracle(rt, reference, leaf, wide):
    """The stack scene (cells of 1..16 coincident faces: leaves of every count 1..16, odd and even, equal t with the
    rank deciding, and a leaf that ends at the last record of the triangle array, in view) built with leaf bounds
    1, 2, 3, 4 and 16; without and with the 4-wide tree."""
    check_scene(rt, reference, "stack", leaf, wide)


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("name", ["tie", "normals", "one", "empty"])
def test_edge_meshes_match_the_oracle(rt, reference, name, wide):
    """tie: three coincident grids, 335 records duplicated by spatial splits (the same face in two leaves: equal t
    and equal rank) and distinct coincident faces (equal t, the rank decides), leaves of 1..6; normals: zero, NaN
    and odd vertex normals (352 of 520 records without the safe-normal bit: the uncertified-normal branch and its
    shading-record address run); one triangle; the empty scene (n_nodes == 0)."""
    check_scene(rt, reference, name, 0, wide)
