"""The deep-tree inputs of tests/deep_scenes.py really reach what they are built for -- asserted on the CPU oracle,
the numpy model of the PLOC rule and host-only scenes, so that the GPU battery (tests/test_gpu_deep_trees.py) cannot
go vacuous. No GPU needed.

Measured values (this oracle build, the generators' fixed seeds) are in the docstrings, after the bound."""
import numpy as np
import pytest

import deep_scenes as D

GENERATORS = {"spine": D.spine, "pairs": D.pair_spine}
# the frames of the GPU battery: test_gpu_edges.FRAME_SIZES and the tile-aligned frame
FRAME_SIZES = [(37, 11), (65, 9), (64, 40), D.FRAME]


class Inputs:
    def __init__(self, orc, name):
        self.arrays = GENERATORS[name]()
        v, f, m, g = self.arrays
        self.mesh = orc.Mesh.from_arrays(v, f, m, groups=g)
        self.export = self.mesh.export()
        self.shell = D.shell_of_face(self.arrays)
        self.n_shells = int(self.shell.max()) + 1
        wb = D.world_boxes(self.export)
        self.face_boxes = wb
        self.shell_boxes = np.stack([np.concatenate([wb[self.shell == s][:, :3].min(0), wb[self.shell == s][:, 3:].max(0)])
                                     for s in range(self.n_shells)])
        self.lists = D.ray_lists(self.export)
        self.scene = {mf: orc.Scene(self.mesh, min_faces=mf) for mf in (8, 300)}


@pytest.fixture(scope="module")
def inputs(orc):
    return {name: Inputs(orc, name) for name in GENERATORS}


def camera_rays(orc, cam, W, H):
    od = [orc.camera_ray(cam, i, j) for j in range(H) for i in range(W)]
    return np.array([a for a, _ in od], np.float32), np.array([b for _, b in od], np.float32)


@pytest.mark.parametrize("name", sorted(GENERATORS))
def test_generators_shape(inputs, name):
    """62 shells of one face, 61 shells of two coincident faces; largest shell first; every face normal (0, 0, 1);
    two materials, one with a non-integer exponent, both reflective; min_faces 8 gives several reference boxes
    [spine 10, pairs 19], 300 one."""
    r = inputs[name]
    v, f, m, g = r.arrays
    assert len(f) <= 200
    assert (r.n_shells, len(f)) == ((D.SPINE_N, D.SPINE_N) if name == "spine" else (D.PAIRS_N, 2 * D.PAIRS_N))
    assert (np.diff(r.shell) <= 0).all() and r.shell[0] == r.n_shells - 1 and r.shell[-1] == 0
    fn = r.export["fn3"]
    assert np.allclose(fn / np.linalg.norm(fn, axis=1, keepdims=True), [0, 0, 1])
    assert len(m) == 2 and sorted(m[:, 9].tolist()) == [2.5, 16.0] and (m[:, 6:9] > 0).all()
    assert set(r.export["fmat"].tolist()) == {0, 1}
    if name == "pairs":
        w = D.world_vertices(r.export)[r.export["fidx"].astype(np.int64)]
        assert np.array_equal(w[0::2], w[1::2])
    assert r.scene[8].box_count() >= 8 and r.scene[300].box_count() == 1


@pytest.mark.parametrize("name", sorted(GENERATORS))
def test_forward_lists_cross_the_whole_spine(inputs, name):
    """Slab test of the rays against the shells' world boxes, no tree: at least 64 rays of the forward list, of its
    reverse and of the 257-ray list cross at least n - 2 shells [forward 3,547 of 4,096; 214 of 257]."""
    r = inputs[name]
    for ln in ("forward", "reversed", "odd"):
        o, d = r.lists[ln]
        assert len(o) == (257 if ln == "odd" else 4096)
        crossed = D.boxes_crossed(r.shell_boxes, o, d)
        deep = int((crossed >= r.n_shells - 2).sum())
        print(f"{name} {ln}: {deep} of {len(o)} rays cross >= {r.n_shells - 2} shells, most {int(crossed.max())}")
        assert deep >= 64
    o, d = r.lists["forward"]
    assert (d[:, 2] < -0.85).all() and (r.lists["reversed"][1][:, 2] > 0.85).all()


@pytest.mark.parametrize("name", sorted(GENERATORS))
def test_lists_are_not_trivial(inputs, name):
    """The oracle's answers: at least 10 distinct winning faces per closest-hit list [forward 61, reversed 18, odd
    51], hits and misses in each [forward 3,941 hits of 4,096], blocked and free shadow segments [2,275 blocked of
    4,096]."""
    r = inputs[name]
    for mf in (8, 300):
        for ln in ("forward", "reversed", "odd"):
            face, t, P = r.scene[mf].closest(*r.lists[ln])
            hit = face >= 0
            distinct = len(set(face[hit].tolist()))
            print(f"{name} min_faces {mf} {ln}: hits {int(hit.sum())} of {len(face)}, distinct faces {distinct}")
            assert distinct >= 10 and hit.any() and (~hit).any()
        b = r.scene[mf].shadow(*r.lists["shadow"])
        print(f"{name} min_faces {mf} shadow: blocked {int(b.sum())} of {len(b)}")
        assert 0.1 < b.mean() < 0.9


@pytest.mark.parametrize("WH", FRAME_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", sorted(GENERATORS))
def test_frames_cross_the_whole_spine(orc, inputs, name, WH):
    """The battery's camera (deep_scenes.camera_args: the eye one unit in front of the apex): every pixel of at least
    one whole 8x8 tile, and the centre pixel, cross at least n - 2 shells' boxes [2 tiles at 37x11 and 65x9, every
    tile at 64x40 and 64x64]; the FULL frame has at least 10 distinct winning faces [35 .. 62], hits and misses."""
    r = inputs[name]
    W, H = WH
    cam = orc.flycam(*D.camera_args(r.export, W, H))
    o, d = camera_rays(orc, cam, W, H)
    ok = (D.boxes_crossed(r.shell_boxes, o, d) >= r.n_shells - 2).reshape(H, W)
    tiles = sum(bool(ok[j:j + 8, i:i + 8].all()) for j in range(0, H - 7, 8) for i in range(0, W - 7, 8))
    rgb, face, t = r.scene[8].render(cam, orc.DEFAULT_LIGHTS, W, H, full=True)
    hit = face >= 0
    distinct = len(set(face[hit].tolist()))
    print(f"{name} {W}x{H}: {int(ok.sum())} of {W * H} pixels cross >= {r.n_shells - 2} shells, whole 8x8 tiles {tiles}, "
          f"hits {int(hit.sum())}, distinct faces {distinct}")
    assert tiles >= 1 and ok[H // 2, W // 2]
    assert distinct >= 10 and hit.any() and (~hit).any()
    assert np.isfinite(rgb[hit]).all(1).sum() >= hit.sum() // 4


def test_ploc_model_chains_both_generators(inputs):
    """The PLOC rule in numpy (Morton order of the box centres, nearest neighbour by merged half area within 4 places,
    mutual pairs merge): one merge per iteration on the spine [61 iterations], on the pairs one iteration that merges
    every pair and then one merge per iteration [61 iterations]; the tree is 62 levels as relayout_dfs counts them,
    and on the spine every interior node has a single face as a child. One shell more is 63 levels (refused); the
    200-shell spine is far deeper [195]."""
    merges, depth, leaf_children = D.ploc_model(inputs["spine"].face_boxes)
    assert merges == [1] * (D.SPINE_N - 1) and depth == D.MAX_DEPTH and min(leaf_children) >= 1
    merges, depth, _ = D.ploc_model(inputs["pairs"].face_boxes)
    assert merges == [D.PAIRS_N] + [1] * (D.PAIRS_N - 1) and depth == D.MAX_DEPTH
    import oracle
    for gen, n, want in ((D.spine, D.SPINE_N + 1, D.MAX_DEPTH + 1), (D.pair_spine, D.PAIRS_N + 1, D.MAX_DEPTH + 1),
                         (D.spine, 200, None)):
        v, f, m, g = gen(n)
        boxes = D.world_boxes(oracle.Mesh.from_arrays(v, f, m, groups=g).export())
        _, depth, _ = D.ploc_model(boxes)
        print(f"{gen.__name__}({n}): modelled PLOC depth {depth}")
        assert depth == want if want else depth > D.MAX_DEPTH + 20


@pytest.mark.parametrize("name", sorted(GENERATORS))
def test_host_builders_stay_shallow(rt, inputs, name):
    """Host-only scenes (SAH and SBVH; leaf 1, 4 and 16; binary and 4-wide): every tree validates and stays under
    depth 40 [9 .. 12; wide 7 .. 9], so the forced-median switch at depth kMaxDepth - 20 is not reached; a device
    builder asked of a host-only scene reports the host SAH builder."""
    v, f, m, g = inputs[name].arrays
    mesh = rt.Mesh.from_arrays(v, f, m, groups=g)
    for builder in (rt.RT_BUILDER_SAH, rt.RT_BUILDER_SBVH):
        for leaf in (1, 4, 16):
            for wide in (0, 1):
                sc = rt.Scene(mesh, device=rt.RT_DEVICE_NONE, builder=builder, leaf_size=leaf, wide_tree=wide)
                info, val = sc.info(), sc.validate_bvh()
                print(f"{name} builder {builder} leaf {leaf} wide {wide}: depth {info['bvh_depth']}, wide depth {info['wide_depth']}")
                assert info["builder"] == builder and val["ok"], (builder, leaf, wide, val)
                assert info["bvh_depth"] < 40
                assert (info["wide_depth"] > 0) == bool(wide)
    for builder in (rt.RT_BUILDER_PLOC_GPU, rt.RT_BUILDER_LBVH_GPU, rt.RT_BUILDER_SAH_GPU):
        sc = rt.Scene(mesh, device=rt.RT_DEVICE_NONE, builder=builder, leaf_size=1)
        assert sc.info()["builder"] == rt.RT_BUILDER_SAH and sc.validate_bvh()["ok"] and sc.info()["bvh_depth"] < 40


def test_chain_stack_demand_on_a_hand_made_chain():
    """chain_stack_demand and tree_shape on node records written by hand: a 5-level chain of unit boxes stacked
    along -z, a leaf beside every link. A ray down the axis needs both children at every level; a ray that passes
    beside the leaves' boxes needs them nowhere; a ray from below meets the same levels."""
    n = 5
    rec = np.zeros(n, D.NODE_DTYPE)
    for k in range(n):
        # child 0: the rest of the chain (z from -n to -(k + 1)), wide in x; child 1: the leaf at z = -k, narrow
        rec["box"][k] = [-2, 2, -1, 1, -float(n), -(k + 1.0), -0.5, 0.5, -1, 1, -(k + 0.5), -(k + 0.25)]
        rec["child"][k] = [(k + 1) * 64 if k + 1 < n else D.LEAF_BIT | 7, D.LEAF_BIT | k]
    nodes = D.parse_nodes(rec.tobytes(), 64)
    assert D.tree_shape(nodes[1]) == (n, 0)
    o = np.array([[0, 0, 1], [1.5, 0, 1], [0, 0, -9]], np.float64)
    d = np.array([[0, 0, -1], [0, 0, -1], [0, 0, 1]], np.float64)
    assert D.chain_stack_demand(nodes, o, d).tolist() == [n, 0, n]
    idx = np.zeros(n, D.NODE_DTYPE)
    idx[:] = rec
    idx["child"][:, 0] = [k + 1 if k + 1 < n else D.LEAF_BIT | 7 for k in range(n)]
    assert D.chain_stack_demand(D.parse_nodes(idx.tobytes(), 1), o, d).tolist() == [n, 0, n]
