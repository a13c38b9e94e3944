"""What the fixtures of tests/test_gpu_leaf_records.py hold, asserted on host builds (no GPU): the leaf histogram
of every tree, read from the scene cache, the duplicated records, the flags, and that the leaf which ends at the
last record of the triangle array is in view of both test frames (on the oracle's frames)."""
import numpy as np
import pytest

import edge_scenes as E
import leaf_scenes as LS

FRAMES = ((64, 64), (40, 24))


def host_scene(rt, arrs, vn=None, leaf=0, wide=0):
    v, f, m, g = arrs
    return rt.Scene(rt.Mesh.from_arrays(v, f, m, vn3=vn, groups=g), device=rt.RT_DEVICE_NONE, builder=rt.RT_BUILDER_SBVH,
                    leaf_size=leaf, wide_tree=wide)


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("leaf", LS.LEAF_BOUNDS)
def test_stack_scene_has_leaves_of_every_count(rt, orc, leaf, wide):
    """Coincident copies cannot be separated, so whatever the leaf bound the stack scene's binary tree holds leaves
    of every count 1..16 (the bound does not bite on this fixture; the tie scene's leaves of 1..6 come from a
    builder that could split); the tree is sound; and the oracle's frames show a face of the leaf that ends at the
    last triangle record."""
    arrs, copies = LS.stack_scene()
    sc = host_scene(rt, arrs, leaf=leaf, wide=wide)
    assert sc.validate_bvh()["ok"]
    s = LS.tree_summary(sc)
    print(f"stack leaf bound {leaf} wide {wide}: leaf histogram {s['hist']}, {s['n_records']} records, "
          f"{s['duplicates']} duplicates, last leaf of {len(s['last_leaf_faces'])}")
    assert set(s["hist"]) == set(range(1, LS.STACK_MAX + 1)), s["hist"]
    assert s["last_leaf_faces"], "a leaf ends at the last record"
    v, f, m, g = arrs
    osc = orc.Scene(orc.Mesh.from_arrays(v, f, m, groups=g))
    for W, H in FRAMES:
        face = np.asarray(osc.render(orc.flycam(W, H, 0, 0, LS.STACK_DZ), orc.DEFAULT_LIGHTS, W, H, full=False)[1])
        assert set(s["last_leaf_faces"]) & set(face.tolist()), (W, H)
        seen = set(copies[face[face >= 0]].tolist())
        assert seen >= set(range(1, LS.STACK_MAX + 1)), (W, H, sorted(seen))  # every cell size is hit


def test_edge_fixtures_hold_what_they_claim(rt):
    tie = LS.tree_summary(host_scene(rt, E.tie_scene()[0]))
    print(f"tie: leaf histogram {tie['hist']}, {tie['duplicates']} duplicate records")
    assert tie["duplicates"] > 0 and {1, 2, 3, 4} <= set(tie["hist"])
    arrs, vn, _ = E.normal_scene()
    sc = host_scene(rt, arrs, vn)
    records, safe_normal, _ = sc.record_flags()
    print(f"normals: leaf histogram {LS.tree_summary(sc)['hist']}, {records - safe_normal} of {records} records uncertified")
    assert records - safe_normal > 100
    one = LS.tree_summary(host_scene(rt, LS.one_triangle()))
    assert one["n_records"] == 1 and one["n_nodes"] <= 1
    none = LS.tree_summary(host_scene(rt, LS.empty()))
    assert none["n_records"] == 0 and none["n_nodes"] == 0
