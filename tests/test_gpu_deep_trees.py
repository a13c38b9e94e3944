"""Deep-tree parity battery (MI355X): every traversal loop against the CPU oracle on trees as deep as the library
accepts. The scenes of tests/deep_scenes.py chain under the PLOC builder: the 62-shell spine gives bvh_depth 62
(= kMaxDepth + 2, the limit of adopt_tree, rt_scene_create and the cache loader) with a leaf beside every one of its
61 interior levels, so a ray down the axis leaves one entry on the traversal stack per level; one shell more is
refused and built by the host SAH instead. tests/test_deep_inputs.py asserts on the CPU that the inputs reach this.

Every comparison is with the oracle -- face ids equal, t and P bit-identical, blocked equal, colours as in
tests/test_gpu_parity.py (non-finite values at the same positions, finite ones within TOL) -- except where a test
says "against the fresh scene" or "against the host-only scene", which are bit for bit.

Measured on the MI355X: spine(62) PLOC leaf 1 depth 62, 4-wide depth 21; spine(63) and spine(200) fall back to the
host SAH (depth 11 and 15), also at leaf sizes 4 and 16 for spine(200); pair_spine(61) PLOC depth 62, 4-wide depth
31 (3 * 31 + 4 = 97 of the 128 stack entries); LBVH / SAH_GPU / SBVH_GPU stay at depth 11 .. 19; the modelled stack
demand of the forward list reaches 61."""
import numpy as np
import pytest

import deep_scenes as D
import edge_scenes as E
import update_scenes as U
from conftest import PARITY_REPORT
from test_gpu_edges import FRAME_SIZES, PRODUCT_VARIANTS, same_frames
from test_gpu_light_sets import NO_CACHE, with_variant
from test_gpu_parity import compare
from test_gpu_ray_streams import dev
from test_gpu_supersample import in_order_mean, shifted
from test_oracle_pinning import same_bits

pytestmark = pytest.mark.gpu

PRIMARY, FULL, BOXES = 0, 1, 2
Q_CLOSEST, Q_SHADOW = 0, 1
NONE = -2  # RT_DEVICE_NONE
ALL_FRAMES = FRAME_SIZES + [D.FRAME]
GENERATORS = {"spine": D.spine, "pairs": D.pair_spine}


@pytest.fixture(scope="module", autouse=True)
def need_gpu(rt):
    if rt.device_count() == 0:
        pytest.skip("no GPU")


class Mesh:
    """One mesh in the library and in the oracle, its ray lists, and the oracle's answers (computed once, read-only
    afterwards)."""

    def __init__(self, rt, orc, arrays, min_faces=(8, 300)):
        self.rt, self.orcm, self.arrays = rt, orc, arrays
        v, f, m, g = arrays
        self.gpu_mesh = rt.Mesh.from_arrays(v, f, m, groups=g)
        self.orc_mesh = orc.Mesh.from_arrays(v, f, m, groups=g)
        self.export = self.orc_mesh.export()
        self.lists = D.ray_lists(self.export)
        self.orc = {mf: orc.Scene(self.orc_mesh, min_faces=mf) for mf in min_faces}
        self._closest, self._shadow, self._frames = {}, {}, {}

    def closest(self, mf, name):
        if (mf, name) not in self._closest:
            out = self.orc[mf].closest(*self.lists[name])
            for a in out:
                a.setflags(write=False)
            self._closest[(mf, name)] = out
        return self._closest[(mf, name)]

    def shadow(self, mf):
        if mf not in self._shadow:
            out = self.orc[mf].shadow(*self.lists["shadow"])
            out.setflags(write=False)
            self._shadow[mf] = out
        return self._shadow[mf]

    def camera(self, lib, W, H, eye=D.EYE_OBJECT):
        return lib.flycam(*D.camera_args(self.export, W, H, eye))

    def frame(self, mf, W, H, mode, depth=0, lights=None, eye=D.EYE_OBJECT):
        """The oracle's frame (rgb [n,3], face, t); mode PRIMARY / FULL / BOXES, depth 0 = the mode's own."""
        key = (mf, W, H, mode, depth, None if lights is None else len(lights), eye)
        if key not in self._frames:
            orc, sc = self.orcm, self.orc[mf]
            cam = self.camera(orc, W, H, eye)
            L = orc.DEFAULT_LIGHTS if lights is None else lights
            if mode == BOXES:
                out = sc.render(cam, L, W, H, box_colors=orc.box_colors_glibc(sc.box_count()))
            else:
                out = sc.render(cam, L, W, H, full=(mode == FULL), max_depth=depth or None)
            for a in out:
                a.setflags(write=False)
            self._frames[key] = out
        return self._frames[key]


class Ref:
    def __init__(self, rt, orc):
        self.spine = Mesh(rt, orc, D.spine())
        self.pairs = Mesh(rt, orc, D.pair_spine())
        self.demand = None  # the forward list's modelled stack demand on the limit scene


@pytest.fixture(scope="module")
def ref(rt, orc):
    return Ref(rt, orc)


@pytest.fixture(scope="module")
def limit(rt, ref):
    """The limit scene: the spine through PLOC at leaf size 1, per min_faces."""
    out = {mf: rt.Scene(ref.spine.gpu_mesh, builder=rt.RT_BUILDER_PLOC_GPU, leaf_size=1, min_faces=mf) for mf in (8, 300)}
    nodes = D.parse_nodes(out[8].records(0), 64)
    ref.demand = D.chain_stack_demand(nodes, *ref.spine.lists["forward"])
    return out


def report(name, scenes, rays, hits, demand, bad):
    PARITY_REPORT.append(f"deep {name}: scenes {scenes}, rays {rays}, hits {hits}, largest modelled stack demand {demand}, "
                         f"mismatches {bad}")


def list_mismatches(sc, m, mf, names=("forward", "reversed", "odd")):
    """(rays, hits, mismatches) of trace_closest on the named lists and trace_shadow on the shadow list."""
    rays = hits = bad = 0
    for name in names:
        face, t, P = sc.trace_closest(*m.lists[name])
        of, ot, oP = m.closest(mf, name)
        bad += int(((face != of) | ~same_bits(t, ot) | ~same_bits(P, oP).all(1)).sum())
        rays += len(of)
        hits += int((of >= 0).sum())
    ob = m.shadow(mf)
    bad += int((sc.trace_shadow(*m.lists["shadow"]) != ob).sum())
    return rays + len(ob), hits + int(ob.sum()), bad


def gpu_frame(rt, sc, m, W, H, mode, depth=0, eye=D.EYE_OBJECT, **kw):
    rgb, face, t, st = sc.render(m.camera(rt, W, H, eye), rt.DEFAULT_LIGHTS, W, H, mode=mode, want_hits=True,
                                 max_depth=depth, **kw)
    return (rgb, face, t), st


def frame_parity(rt, sc, m, mf, W, H, mode, depth, what):
    """compare() of the GPU frame with the oracle's; returns (pixels, hits)."""
    got, _ = gpu_frame(rt, sc, m, W, H, mode, depth)
    want = m.frame(mf, W, H, mode, depth)
    compare(*got, *want, what)
    if mode == BOXES:
        assert got[0].reshape(-1, 3).tobytes() == want[0].tobytes(), what
    return W * H, int((want[1] >= 0).sum())


def tree_of(sc):
    return D.tree_shape(D.parse_nodes(sc.records(0), 64)[1])


def demand_of(sc, m):
    """The largest modelled stack demand of m's forward list on sc's binary tree."""
    return int(D.chain_stack_demand(D.parse_nodes(sc.records(0), 64), *m.lists["forward"]).max())


# ---- the limit is where the code says ----
def test_limit_scene_is_a_62_level_chain(rt, ref, limit):
    """spine(62) through PLOC at leaf size 1 is adopted at bvh_depth 62; the node records are a chain of 61 interior
    levels with a leaf at every node; the forward list's modelled stack demand reaches at least 60 for at least 64
    rays [61; 3,414 rays]; every list equals the oracle at min_faces 8 and 300."""
    tot = [0, 0, 0]
    for mf, sc in limit.items():
        info, val = sc.info(), sc.validate_bvh()
        assert info["builder"] == rt.RT_BUILDER_PLOC_GPU and info["bvh_depth"] == D.MAX_DEPTH, info
        assert val["ok"] and val["covered2"] == D.SPINE_N, val
        assert info["n_ref_boxes"] == ref.spine.orc[mf].box_count()
        levels, without_leaf = tree_of(sc)
        assert (levels, without_leaf) == (D.MAX_DEPTH - 1, 0)
        for k, x in enumerate(list_mismatches(sc, ref.spine, mf)):
            tot[k] += x
    deep = int((ref.demand >= 60).sum())
    print(f"modelled demand: max {int(ref.demand.max())}, {deep} rays at >= 60")
    assert deep >= 64
    assert tot[2] == 0, f"{tot[2]} rays differ from the oracle"
    report("limit scene lists", 2, tot[0], tot[1], int(ref.demand.max()), tot[2])


@pytest.fixture(scope="module")
def bigger(rt, orc):
    return {n: Mesh(rt, orc, D.spine(n), min_faces=(8,)) for n in (D.SPINE_N + 1, 200)}


@pytest.mark.parametrize("n", [D.SPINE_N + 1, 200])
def test_deeper_chains_fall_back_to_the_host_sah(rt, bigger, n):
    """One shell more (PLOC depth 63) and the 200-shell spine: adopt_tree refuses the device tree and the host SAH
    builds the scene -- the builder reported is RT_BUILDER_SAH, the tree validates at depth < 40 [11, 15], and the
    lists and the 64x64 FULL frame equal the oracle."""
    m = bigger[n]
    sc = rt.Scene(m.gpu_mesh, builder=rt.RT_BUILDER_PLOC_GPU, leaf_size=1, min_faces=8)
    info, val = sc.info(), sc.validate_bvh()
    print(f"spine({n}) asked of PLOC: builder {info['builder']}, depth {info['bvh_depth']}")
    assert info["builder"] == rt.RT_BUILDER_SAH, info
    assert val["ok"] and info["bvh_depth"] < 40
    rays, hits, bad = list_mismatches(sc, m, 8)
    assert bad == 0, f"{bad} rays differ from the oracle"
    px, fh = frame_parity(rt, sc, m, 8, *D.FRAME, FULL, 0, f"spine({n}) fallback")
    report(f"fallback spine({n})", 1, rays + px, hits + fh, demand_of(sc, m), bad)


@pytest.mark.parametrize("builder", ["RT_BUILDER_LBVH_GPU", "RT_BUILDER_SAH_GPU", "RT_BUILDER_SBVH_GPU"])
@pytest.mark.parametrize("n", [D.SPINE_N + 1, 200])
def test_other_device_builders_on_the_spines(rt, bigger, n, builder):
    """The same two sizes through the other device builders: the builder reported is the one asked for, the tree
    validates [depth 11 .. 19], lists and the 64x64 FULL frame equal the oracle."""
    m = bigger[n]
    bid = getattr(rt, builder)
    sc = rt.Scene(m.gpu_mesh, builder=bid, leaf_size=1, min_faces=8)
    info = sc.info()
    print(f"spine({n}) {builder}: depth {info['bvh_depth']}")
    assert info["builder"] == bid and sc.validate_bvh()["ok"] and info["bvh_depth"] <= D.MAX_DEPTH
    rays, hits, bad = list_mismatches(sc, m, 8)
    assert bad == 0, f"{bad} rays differ from the oracle"
    px, fh = frame_parity(rt, sc, m, 8, *D.FRAME, FULL, 0, f"spine({n}) {builder}")
    report(f"spine({n}) {builder}", 1, rays + px, hits + fh, demand_of(sc, m), bad)


@pytest.mark.parametrize("leaf", [4, 16])
def test_ploc_leaf_sizes_at_200_shells(rt, bigger, leaf):
    """spine(200) through PLOC with leaves of up to 4 and 16 triangles: the collapse shortens the chain, but not
    below 62 -- as found on the MI355X both fall back to the host SAH [depth 15] -- with parity either way."""
    m = bigger[200]
    sc = rt.Scene(m.gpu_mesh, builder=rt.RT_BUILDER_PLOC_GPU, leaf_size=leaf, min_faces=8)
    info = sc.info()
    print(f"spine(200) PLOC leaf {leaf}: builder {info['builder']}, depth {info['bvh_depth']}")
    assert info["builder"] == rt.RT_BUILDER_SAH and info["bvh_depth"] < 40 and sc.validate_bvh()["ok"]
    rays, hits, bad = list_mismatches(sc, m, 8)
    assert bad == 0, f"{bad} rays differ from the oracle"
    report(f"spine(200) PLOC leaf {leaf} (fell back)", 1, rays, hits, demand_of(sc, m), bad)


# ---- every stack home at depth 62 ----
def stream(sc, query, a, b, reorder):
    return {k: v.cpu().numpy() for k, v in sc.trace_stream(query, dev(a), dev(b), reorder=reorder).items()}


def test_ray_streams_on_the_limit_scene(rt, ref, limit):
    """rt_trace_stream closest and shadow, in order and with RT_RAYS_REORDER, on every list."""
    m = ref.spine
    rays = hits = bad = 0
    for mf, sc in limit.items():
        for reorder in (False, True):
            for name in ("forward", "reversed", "odd"):
                got = stream(sc, Q_CLOSEST, *m.lists[name], reorder)
                of, ot, oP = m.closest(mf, name)
                bad += int(((got["face"] != of) | ~same_bits(got["t"], ot) | ~same_bits(got["P"], oP).all(1)).sum())
                rays += len(of)
                hits += int((of >= 0).sum())
            got = stream(sc, Q_SHADOW, *m.lists["shadow"], reorder)
            bad += int((got["blocked"] != m.shadow(mf)).sum())
            rays += len(m.shadow(mf))
    assert bad == 0, f"{bad} rays differ from the oracle"
    report("limit scene ray streams", 2, rays, hits, int(ref.demand.max()), bad)


@pytest.mark.parametrize("wavefront", [False, True], ids=["megakernel", "wavefront"])
@pytest.mark.parametrize("mode", [PRIMARY, FULL], ids=["primary", "full"])
def test_stream_color_on_the_limit_scene(rt, ref, limit, mode, wavefront):
    """rt_trace_stream_color at depths 1, 2, 4 and 16 on the 4,096 camera rays of the 64x64 frame (every one crosses
    the whole spine) and on their first 257: colours, faces and t against the oracle's frame."""
    m = ref.spine
    W, H = D.FRAME
    rays = hits = 0
    for mf, sc in limit.items():
        o, d = sc.camera_rays(m.camera(rt, W, H), W, H)
        for depth in (1, 2, 4, 16):
            want = m.frame(mf, W, H, mode, depth)
            for n in (W * H, 257):
                got = sc.trace_stream_color(o[:n].contiguous(), d[:n].contiguous(), rt.DEFAULT_LIGHTS, mode=mode,
                                            max_depth=depth, wavefront=wavefront)
                got = {k: v.cpu().numpy() for k, v in got.items()}
                compare(got["rgb"], got["face"], got["t"], want[0][:n], want[1][:n], want[2][:n],
                        f"stream colour mode {mode} depth {depth} wavefront {wavefront} min_faces {mf} n {n}")
                rays += n
                hits += int((want[1][:n] >= 0).sum())
    report(f"limit scene stream colours mode {mode} wavefront {wavefront}", 2, rays, hits, int(ref.demand.max()), 0)


@pytest.mark.parametrize("WH", ALL_FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frames_on_the_limit_scene(rt, ref, limit, WH):
    """PRIMARY and FULL at the modes' own depth and at max_depth 1..4 and 16, and RT_MODE_BOX_COLORS; counting frames
    (RT_FRAME_STATS, and with RT_FRAME_WAVE_STATS at the modes' own depth) render the plain frame's bits with positive
    counters; shards 0..2 of 3 stitch to the whole frame."""
    m = ref.spine
    W, H = WH
    px = hits = 0
    for mf, sc in limit.items():
        for mode in (PRIMARY, FULL):
            for depth in (0, 1, 2, 3, 4, 16):
                a, b = frame_parity(rt, sc, m, mf, W, H, mode, depth, f"{W}x{H} mode {mode} depth {depth} min_faces {mf}")
                px += a
                hits += b
        a, b = frame_parity(rt, sc, m, mf, W, H, BOXES, 0, f"{W}x{H} box colours min_faces {mf}")
        px += a
        hits += b
        for mode in (PRIMARY, FULL):
            whole, _ = gpu_frame(rt, sc, m, W, H, mode)
            for depth, flags in ((0, rt.RT_FRAME_STATS), (0, rt.RT_FRAME_STATS | rt.RT_FRAME_WAVE_STATS), (4, rt.RT_FRAME_STATS)):
                plain = whole if depth == 0 else gpu_frame(rt, sc, m, W, H, mode, depth)[0]
                got, st = gpu_frame(rt, sc, m, W, H, mode, depth, flags=flags)
                assert same_frames(plain, got), f"{W}x{H} mode {mode} depth {depth} flags {flags}: counting frame differs"
                assert st["primary_rays"] == W * H and st["node_visits"] > 0 and st["tri_tests"] > 0 and st["hits"] > 0, st
                if flags & rt.RT_FRAME_WAVE_STATS:
                    ws = sc.wave_stats().astype(np.int64)
                    assert len(ws) == 4 * ((W + 15) // 16) * ((H + 15) // 16) and ws[:, 0].sum() > 0 and ws[:, 1].sum() > 0
            out = [np.full((H, W, 3), np.nan, np.float32), np.full((H, W), -7, np.int32), np.full((H, W), np.nan, np.float32)]
            cover = np.zeros((H, W), np.int32)
            for k in range(3):
                part, _ = gpu_frame(rt, sc, m, W, H, mode, shard=(k, 3))
                mask = rt.shard_mask(W, H, k, 3)
                cover += mask
                for dst, src in zip(out, part):
                    dst[mask] = src[mask]
            assert (cover == 1).all() and same_frames(whole, out), f"mode {mode}: 3 shards stitched != whole frame"
    report(f"limit scene frames {W}x{H} (pixels as rays)", 2, px, hits, int(ref.demand.max()), 0)


@pytest.mark.parametrize("bits", PRODUCT_VARIANTS)
def test_product_variants_on_the_limit_scene(rt, ref, limit, bits):
    """Every kernel variant the product library serves: the 64x64 and 37x11 frames (PRIMARY, FULL, box colours;
    max_depth 0 and 4) and the ray lists, each against the oracle."""
    m = ref.spine
    px = hits = bad = 0

    def run():
        nonlocal px, hits, bad
        for mf, sc in limit.items():
            for W, H in (D.FRAME, FRAME_SIZES[0]):
                for mode in (PRIMARY, FULL, BOXES):
                    for depth in ((0,) if mode == BOXES else (0, 4)):
                        a, b = frame_parity(rt, sc, m, mf, W, H, mode, depth, f"variant {bits} {W}x{H} mode {mode} depth {depth}")
                        px += a
                        hits += b
            r, h, b = list_mismatches(sc, m, mf)
            px, hits, bad = px + r, hits + h, bad + b
    with_variant(rt, bits, run)
    assert bad == 0, f"variant {bits}: {bad} rays differ from the oracle"
    report(f"limit scene variant {bits}", 2, px, hits, int(ref.demand.max()), bad)


def test_four_frames_in_flight_on_the_limit_scene(rt, ref, limit):
    """Nine FULL frames queued on four slots from four eyes: the last one downloaded equals the oracle's."""
    m = ref.spine
    W, H = D.FRAME
    eyes = [D.EYE_OBJECT, (-0.2, 0.1, 1.0), (0.0, 0.0, 0.5), (0.3, -0.2, 2.0)]
    sc = rt.Scene(m.gpu_mesh, builder=rt.RT_BUILDER_PLOC_GPU, leaf_size=1, min_faces=8, frames_in_flight=4)
    assert sc.info()["bvh_depth"] == D.MAX_DEPTH
    for k in range(9):
        sc.render_async(m.camera(rt, W, H, eyes[k % 4]), rt.DEFAULT_LIGHTS, W, H, mode=rt.RT_MODE_FULL,
                        flags=rt.RT_FRAME_WRITE_HITS)
    sc.synchronize()
    got = sc.download(W, H, want_hits=True)
    want = m.frame(8, W, H, FULL, 0, eye=eyes[8 % 4])
    compare(*got, *want, "frames in flight")
    report("limit scene, four frames in flight", 1, W * H, int((want[1] >= 0).sum()), int(ref.demand.max()), 0)


def test_light_set_on_the_limit_scene(rt, ref, limit):
    """33 lights (a set read from device memory) with and without the wave-level occluder cache, as a frame and as a
    ray list, FULL at the mode's depth and at 4."""
    m = ref.spine
    W, H = D.FRAME
    lights = E.ring_lights(33)
    px = hits = 0
    for mf, sc in limit.items():
        ls = sc.light_set(lights)
        cam = m.camera(rt, W, H)
        o, d = sc.camera_rays(cam, W, H)
        for depth in (0, 4):
            want = m.frame(mf, W, H, FULL, depth, lights=lights)
            for variant in (0, NO_CACHE):
                rgb, face, t, _ = with_variant(rt, variant, lambda: sc.render_lit(cam, ls, W, H, mode=rt.RT_MODE_FULL,
                                                                                  max_depth=depth, want_hits=True))
                compare(rgb, face, t, *want, f"33 lights frame depth {depth} variant {variant} min_faces {mf}")
                got = with_variant(rt, variant, lambda: sc.trace_stream_lit(o, d, ls, mode=rt.RT_MODE_FULL, max_depth=depth))
                got = {k: v.cpu().numpy() for k, v in got.items()}
                compare(got["rgb"], got["face"], got["t"], *want, f"33 lights list depth {depth} variant {variant}")
                px += 2 * W * H
                hits += 2 * int((want[1] >= 0).sum())
    report("limit scene, 33-light set", 2, px, hits, int(ref.demand.max()), 0)


def test_view_batch_and_supersampling_on_the_limit_scene(rt, orc, ref, limit):
    """A batch of 4 cameras (PRIMARY and FULL), and supersampled frames at S = 4 (the packed layout) and S = 3 (the
    loop): every view against the oracle's frame, every supersampled pixel against the in-order mean of the oracle's
    frames of the shifted cameras, face and t sample 0's."""
    m = ref.spine
    W, H = D.FRAME
    eyes = [D.EYE_OBJECT, (-0.2, 0.1, 1.0), (0.0, 0.0, 0.5), (0.3, -0.2, 2.0)]
    sc = limit[8]
    px = hits = 0
    for mode in (PRIMARY, FULL):
        res = sc.render_views([m.camera(rt, W, H, e) for e in eyes], rt.DEFAULT_LIGHTS, W, H, mode=mode, want_hits=True)
        res = {k: v.cpu().numpy() for k, v in res.items()}
        for k, e in enumerate(eyes):
            want = m.frame(8, W, H, mode, 0, eye=e)
            compare(res["rgb"][k], res["face"][k], res["t"][k], *want, f"view {k} mode {mode}")
            px += W * H
            hits += int((want[1] >= 0).sum())
    assert rt.sample_plan(FULL, 0, 4, 4, 1, 4)["layout"] == 1 and rt.sample_plan(FULL, 0, 4, 4, 1, 3)["layout"] == 0
    ocam = m.camera(orc, W, H)
    for grid in ((2, 2), (3, 1)):
        offs = rt.sample_pattern(grid).array()
        frames = [m.orc[8].render(shifted(ocam, ox, oy), orc.DEFAULT_LIGHTS, W, H, full=True) for ox, oy in offs]
        want = in_order_mean([f[0] for f in frames])
        res = sc.render_views([m.camera(rt, W, H)], rt.DEFAULT_LIGHTS, W, H, mode=rt.RT_MODE_FULL, want_hits=True, samples=grid)
        res = {k: v.cpu().numpy()[0] for k, v in res.items()}
        compare(res["rgb"], res["face"], res["t"], want, frames[0][1], frames[0][2], f"supersampling {grid}")
        px += W * H * len(offs)
        hits += sum(int((f[1] >= 0).sum()) for f in frames)
    report("limit scene, view batch and supersampling", 1, px, hits, int(ref.demand.max()), 0)


def test_two_replicas_on_one_gpu(rt, ref, limit):
    m = ref.spine
    W, H = D.FRAME
    sc = rt.Scene(m.gpu_mesh, builder=rt.RT_BUILDER_PLOC_GPU, leaf_size=1, min_faces=8, devices=[0, 0])
    assert sc.info()["bvh_depth"] == D.MAX_DEPTH and sc.info()["builder"] == rt.RT_BUILDER_PLOC_GPU
    px = hits = 0
    for mode in (PRIMARY, FULL):
        a, b = frame_parity(rt, sc, m, 8, W, H, mode, 0, f"two replicas mode {mode}")
        px, hits = px + a, hits + b
    report("limit scene, two replicas on one GPU", 1, px, hits, int(ref.demand.max()), 0)


@pytest.mark.parametrize("wide", [0, 1])
def test_pairs_scene(rt, ref, wide):
    """pair_spine(61): two coincident faces per shell, PLOC depth 62 with a two-leaf subtree beside every chain link;
    with wide_tree=1 the fp32 4-wide tree is 31 levels deep (3 * 31 + 4 = 97 stack entries of 128; the plain spine's
    is 21). Lists and frames against the oracle; every hit is a tie that the reference's rank decides."""
    m = ref.pairs
    px = hits = bad = 0
    for mf in (8, 300):
        sc = rt.Scene(m.gpu_mesh, builder=rt.RT_BUILDER_PLOC_GPU, leaf_size=1, min_faces=mf, wide_tree=wide)
        info, val = sc.info(), sc.validate_bvh()
        print(f"pairs wide_tree {wide} min_faces {mf}: depth {info['bvh_depth']}, wide_depth {info['wide_depth']}")
        assert info["builder"] == rt.RT_BUILDER_PLOC_GPU and info["bvh_depth"] == D.MAX_DEPTH and val["ok"], (info, val)
        assert (info["wide_depth"] > 0) == bool(wide)
        r, h, b = list_mismatches(sc, m, mf)
        px, hits, bad = px + r, hits + h, bad + b
        for W, H in (D.FRAME, FRAME_SIZES[0]):
            for mode, depth in ((PRIMARY, 0), (FULL, 0), (FULL, 4), (BOXES, 0)):
                a, b = frame_parity(rt, sc, m, mf, W, H, mode, depth, f"pairs wide {wide} {W}x{H} mode {mode} depth {depth}")
                px, hits = px + a, hits + b
    assert bad == 0, f"{bad} rays differ from the oracle"
    report(f"pairs scene wide_tree {wide}", 2, px, hits, demand_of(sc, m), bad)


# ---- refit on 61 levels ----
def identical(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), what


@pytest.mark.parametrize("how", ["update", "update_device"])
def test_refit_on_61_levels(rt, ref, tmp_path, how):
    """rt_scene_update / rt_scene_update_device on the limit scene (k_refit_level once per level: 61 launches) with
    the deformations of tests/update_scenes.py -- small, large, back: after every step the frames and the forward
    list equal, bit for bit, a fresh scene of that geometry (built by the default builder: a fresh PLOC build of moved
    geometry may fall back), and the three record images are byte-equal to the host-only scene -- the saved limit
    scene loaded without a device -- updated on the host."""
    from test_gpu_update_device import tensors
    m = ref.spine
    W, H = D.FRAME
    arr = m.arrays
    sc = rt.Scene(m.gpu_mesh, builder=rt.RT_BUILDER_PLOC_GPU, leaf_size=1)
    assert sc.info()["bvh_depth"] == D.MAX_DEPTH
    path = str(tmp_path / "limit.rtscene")
    sc.save(path)
    on_host = rt.Scene.load(path, device=NONE)
    assert on_host.info()["bvh_depth"] == D.MAX_DEPTH
    for which in range(3):
        identical(sc.records(which), on_host.records(which), f"created, records {which}")
    cam = m.camera(rt, W, H)
    o, d = m.lists["forward"]
    rays = hits = 0
    for step, v in enumerate(U.steps(arr)):
        mesh = U.mesh_of(rt, arr, v)
        if how == "update":
            st = sc.update(mesh, stats=True)
        else:
            tv, tvn, tfn = tensors(mesh)
            st = sc.update_device(tv, tvn, tfn, model_matrix=mesh.export()["M16"], stats=True)
        assert st["bounds_on_device"] == 1
        on_host.update(mesh)
        for which in range(3):
            identical(sc.records(which), on_host.records(which), f"{how} step {step}, records {which}")
        val = sc.validate_bvh()
        assert val["ok"] and sc.info()["bvh_depth"] == D.MAX_DEPTH, val
        fresh = rt.Scene(mesh)
        for mode, depth in ((PRIMARY, 0), (FULL, 0), (FULL, 4)):
            a = sc.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=mode, max_depth=depth, want_hits=True)[:3]
            b = fresh.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=mode, max_depth=depth, want_hits=True)[:3]
            assert same_frames(a, b), f"{how} step {step} mode {mode} depth {depth}: differs from the fresh scene"
            assert (b[1] >= 0).any()
            rays += W * H
            hits += int((b[1] >= 0).sum())
        a, b = sc.trace_closest(o, d), fresh.trace_closest(o, d)
        assert same_frames(a, b), f"{how} step {step}: forward list differs from the fresh scene"
        rays += len(o)
        hits += int((b[0] >= 0).sum())
    # back at the original vertices: the oracle's answers again
    assert list_mismatches(sc, m, 300)[2] == 0
    report(f"limit scene refit by {how} (against the fresh scene)", 1, rays, hits, int(D.MAX_DEPTH - 1), 0)


# ---- the cache round trip ----
def test_cache_round_trip_of_the_limit_scene(rt, ref, limit, tmp_path):
    """The saved limit scene loads on the device and on the host at bvh_depth 62 with the same three record images;
    its nodes section is the 61-level chain; the scene loaded on the device passes the list parity."""
    from test_host import NODES, _cache_sections
    m = ref.spine
    path = tmp_path / "limit.rtscene"
    limit[8].save(path)
    levels, without_leaf = D.tree_shape(D.parse_nodes(_cache_sections(path.read_bytes())[NODES], 1)[1])
    assert (levels, without_leaf) == (D.MAX_DEPTH - 1, 0)
    on_dev, on_host = rt.Scene.load(path), rt.Scene.load(path, device=NONE)
    for sc in (on_dev, on_host):
        assert sc.info()["bvh_depth"] == D.MAX_DEPTH and sc.info()["builder"] == rt.RT_BUILDER_PLOC_GPU
        assert sc.validate_bvh()["ok"]
        for which in range(3):
            identical(sc.records(which), limit[8].records(which), f"loaded, records {which}")
    rays, hits, bad = list_mismatches(on_dev, m, 8)
    assert bad == 0, f"{bad} rays differ from the oracle"
    px, fh = frame_parity(rt, on_dev, m, 8, *D.FRAME, FULL, 4, "loaded limit scene")
    report("limit scene from the cache", 1, rays + px, hits + fh, int(ref.demand.max()), bad)
