"""Mesh-edge parity battery (MI355X): the kernels against the CPU oracle on the inputs of tests/edge_scenes.py that
reach calculateDistance's last rejection -- a hit whose interpolated normal has norm exactly 0 is dropped
(flyscene.cpp:467) and the ray goes on to what lies behind -- and on zero-area faces and triangles whose area
arithmetic underflows. The kernels skip that blend for faces carrying the safe-normal flag (TriRec64::box bit 31)
and re-run the reference's arithmetic for the others; a wrong flag or a blend that rounds differently makes a face
opaque where the reference sees through it, or the reverse. Every path that accepts a candidate is held to the
oracle here: closest hit and shadow through every builder, leaf size, tree width and box size; frames in every mode,
depth, product kernel variant, in flight and sharded; 33 lights with and without the occluder cache; ray lists in
order, reordered and wavefront; view batches and supersampled batches; the scene cache.
tests/test_mesh_edges_host.py asserts on the oracle alone that these inputs reach those edges.

Comparisons as everywhere in this suite: face ids equal, t and P bit-identical (NaN equal to NaN), blocked equal;
colours with non-finite positions identical and finite ones within 1e-4; paths documented as bit-identical to
rt_render are compared with rt_render bit for bit. Each test adds a line to the run's parity summary: rays, hits,
through-rays (rays whose answer lies behind a face that rejected them) and mismatches [first run: 504,816 rays and
19,176 through-rays per builder, 0 mismatches everywhere]."""
import numpy as np
import pytest
import torch

import edge_scenes as E
from conftest import PARITY_REPORT
from test_gpu_edges import BUILDERS, FRAME_SIZES, PRODUCT_VARIANTS, same_frames
from test_gpu_light_sets import NO_CACHE, lit_trace, with_variant
from test_gpu_parity import TOL, compare
from test_gpu_ray_streams import Q_CLOSEST, Q_COLOR, Q_SHADOW, assert_same, dev, stream_trace
from test_gpu_supersample import LOOP, PACKED, in_order_mean, layout_variant, shifted
from test_gpu_view_batches import assert_views, collect, sentinel_buffers
from test_oracle_pinning import colour_errors, same_bits

pytestmark = pytest.mark.gpu

SAFE = 0x80000000
NFRONT = 2 * E.NORMAL_N ** 2
CAMERA = (0.0, 0.0, 20.0)  # flycam(W, H, dx, dy, dz): the eye at (0, 0, 1), head-on
PRIMARY, FULL, BOX = 0, 1, 2
COMBOS = [(False, False), (True, False), (False, True), (True, True)]  # (reorder, wavefront)


@pytest.fixture(scope="module", autouse=True)
def need_gpu(rt):
    if rt.device_count() == 0:
        pytest.skip("no GPU")


class Ref:
    """The three scenes' arrays and the oracle's answers, computed once per module and never written to afterwards."""

    def __init__(self, orc):
        self.orc = orc
        (v, f, m, g), vn, self.cls = E.normal_scene()
        v2, f2, vn2, self.added, self.new_id = E.degenerate_faces(v, f, vn)
        self.arrays = {"normal": ((v, f, m, g), vn), "degenerate": ((v2, f2, m, [(len(f2), 0)]), vn2),
                       "micro": (E.micro_fan_scene(), None)}
        # the faces behind the front grid (normal, degenerate) / behind the fan (micro)
        self.behind = {"normal": np.arange(NFRONT, len(f)), "degenerate": self.new_id[NFRONT:],
                       "micro": np.array([len(E.MICRO_EXPONENTS)])}
        self.rays = {"lattice": E.normal_lattice_rays(), "random": E.normal_random_rays(), "shadow": E.normal_shadow_rays(),
                     "micro": E.micro_fan_rays()[:2]}
        self._mesh, self._scene, self._closest, self._shadow, self._frames = {}, {}, {}, {}, {}

    def lists(self, which):
        return ("micro",) if which == "micro" else ("lattice", "random", "shadow")

    def mesh(self, which):
        if which not in self._mesh:
            (v, f, m, g), vn = self.arrays[which]
            self._mesh[which] = self.orc.Mesh.from_arrays(v, f, m, vn3=vn, groups=g)
        return self._mesh[which]

    def scene(self, which, mf=300):
        if (which, mf) not in self._scene:
            self._scene[(which, mf)] = self.orc.Scene(self.mesh(which), min_faces=mf)
        return self._scene[(which, mf)]

    def closest(self, which, mf, rays):
        key = (which, mf, rays)
        if key not in self._closest:
            out = self.scene(which, mf).closest(*self.rays[rays])
            for a in out:
                a.setflags(write=False)
            self._closest[key] = out
        return self._closest[key]

    def shadow(self, which, mf, rays):
        key = (which, mf, rays)
        if key not in self._shadow:
            out = self.scene(which, mf).shadow(*self.rays[rays])
            out.setflags(write=False)
            self._shadow[key] = out
        return self._shadow[key]

    def through(self, which, mf, rays):
        return int(np.isin(self.closest(which, mf, rays)[0], self.behind[which]).sum())

    def frame(self, which, mf, W, H, mode, depth, lights="default"):
        """mode PRIMARY | FULL | BOX; depth 0 = the mode's own; lights "default" or "ring33"."""
        key = (which, mf, W, H, mode, depth, lights)
        if key not in self._frames:
            orc, sc = self.orc, self.scene(which, mf)
            cam = orc.flycam(W, H, *CAMERA)
            ll = orc.DEFAULT_LIGHTS if lights == "default" else E.ring_lights(33)
            if mode == BOX:
                out = sc.render(cam, ll, W, H, box_colors=orc.box_colors_glibc(sc.box_count()))
            else:
                out = sc.render(cam, ll, W, H, full=(mode == FULL), max_depth=depth or None)
            for a in out:
                a.setflags(write=False)
            self._frames[key] = out
        return self._frames[key]


@pytest.fixture(scope="module")
def ref(orc):
    return Ref(orc)


@pytest.fixture(scope="module")
def meshes(rt, ref):
    out = {}
    for which, ((v, f, m, g), vn) in ref.arrays.items():
        out[which] = rt.Mesh.from_arrays(v, f, m, vn3=vn, groups=g)
    return out


@pytest.fixture(scope="module")
def gpu(rt, meshes):
    """The normal scene's default build (device SBVH, device boxes) per min_faces and a host-SBVH build with the
    4-wide tree, as tests/test_gpu_edges.py builds the tie scene; and the degenerate scene's default build."""
    out = {(mf, wide): rt.Scene(meshes["normal"], min_faces=mf, wide_tree=wide,
                                builder=rt.RT_BUILDER_SBVH if wide else rt.RT_BUILDER_SBVH_GPU)
           for mf in (8, 300) for wide in (0, 1)}
    out["degenerate"] = rt.Scene(meshes["degenerate"])
    return out


def report(name, rays, hits, through, bad):
    PARITY_REPORT.append(f"{name}: rays {rays}, hits {hits}, through-rays {through}, mismatches {bad}")


def closest_bad(got, want):
    face, t, P = got
    of, ot, oP = want
    return int(((face != of) | ~same_bits(t, ot) | ~same_bits(P, oP).all(1)).sum())


@pytest.mark.parametrize("builder", sorted(BUILDERS))
def test_closest_and_shadow_match_the_oracle(rt, ref, meshes, builder):
    """trace_closest and trace_shadow of the lattice, random, shadow and micro-fan lists on the normal scene, the
    normal scene with 24 zero-area faces and the micro fan: host SBVH / SAH and device SBVH / SAH / PLOC / LBVH, leaf
    sizes 1, 4 and 16, binary and 4-wide trees, min_faces 8 and 300. Every build reports the builder asked for, the
    oracle's box count, and passes validate_bvh(); face, t and P equal the oracle's bit for bit, blocked equals."""
    bid = getattr(rt, BUILDERS[builder])
    n_rays = n_hits = n_thr = n_bad = n_scenes = 0
    for which in ("normal", "degenerate", "micro"):
        for leaf in (1, 4, 16):
            for wide in (0, 1):
                for mf in (8, 300):
                    what = f"{builder} {which} leaf {leaf} wide {wide} min_faces {mf}"
                    sc = rt.Scene(meshes[which], builder=bid, leaf_size=leaf, wide_tree=wide, min_faces=mf)
                    info = sc.info()
                    assert info["builder"] == bid, f"{what}: built with builder {info['builder']}"
                    assert info["n_ref_boxes"] == ref.scene(which, mf).box_count(), what
                    val = sc.validate_bvh()
                    assert val["ok"], f"{what}: {val}"
                    n_scenes += 1
                    for rays in ref.lists(which):
                        a, b = ref.rays[rays]
                        bad = closest_bad(sc.trace_closest(a, b), ref.closest(which, mf, rays))
                        sbad = int((sc.trace_shadow(a, b) != ref.shadow(which, mf, rays)).sum())
                        n_rays += 2 * len(a)
                        n_hits += int((ref.closest(which, mf, rays)[0] >= 0).sum()) + int(ref.shadow(which, mf, rays).sum())
                        n_thr += ref.through(which, mf, rays)
                        n_bad += bad + sbad
                        assert bad == 0 and sbad == 0, f"{what} {rays}: closest {bad}, shadow {sbad} rays differ"
                    if which == "degenerate":
                        assert not np.isin(sc.trace_closest(*ref.rays["lattice"])[0], ref.added).any(), what
    assert n_thr > 0
    report(f"mesh edges {builder} ({n_scenes} scenes, closest + shadow)", n_rays, n_hits, n_thr, n_bad)


def gpu_frame(rt, sc, W, H, mode, depth=0, shard=(0, 1), lights=None):
    rgb, face, t, _ = sc.render(rt.flycam(W, H, *CAMERA), rt.DEFAULT_LIGHTS if lights is None else lights, W, H, mode=mode,
                                want_hits=True, max_depth=depth, shard=shard)
    return rgb, face, t


def frame_bad(got, want):
    return int(((got[1].reshape(-1) != want[1]) | ~same_bits(got[2].reshape(-1), want[2])).sum())


@pytest.mark.parametrize("WH", FRAME_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frames_match_the_oracle(rt, ref, meshes, gpu, WH):
    """The normal scene head-on in ragged frames: PRIMARY / FULL at max_depth 0, 1 and 3 against the oracle (68 and 2
    reference boxes, binary and 4-wide trees; the degenerate scene's default build too), RT_MODE_BOX_COLORS once; the
    3-shard stitch equals the whole frame; the last of five frames queued with rt_render_async on four slots equals
    rt_render's."""
    W, H = WH
    px = hits = thr = bad = 0
    for key, sc in gpu.items():
        which, mf = ("degenerate", 300) if key == "degenerate" else ("normal", key[0])
        for mode in (PRIMARY, FULL):
            for depth in (0, 1, 3):
                got = gpu_frame(rt, sc, W, H, mode, depth)
                want = ref.frame(which, mf, W, H, mode, depth)
                px += W * H
                hits += int((want[1] >= 0).sum())
                thr += int(np.isin(want[1], ref.behind[which]).sum())
                bad += frame_bad(got, want)
                compare(*got, *want, f"{W}x{H} mode {mode} depth {depth} {key}")
            whole = gpu_frame(rt, sc, W, H, mode)
            out = [np.full((H, W, 3), np.nan, np.float32), np.full((H, W), -7, np.int32), np.full((H, W), np.nan, np.float32)]
            cover = np.zeros((H, W), np.int32)
            for k in range(3):
                part = gpu_frame(rt, sc, W, H, mode, shard=(k, 3))
                mask = rt.shard_mask(W, H, k, 3)
                cover += mask
                for dst, src in zip(out, part):
                    dst[mask] = src[mask]
            assert (cover == 1).all() and same_frames(whole, out), f"{key} mode {mode}: 3 shards stitched != whole frame"
    if (W, H) == (64, 40):
        for mf in (8, 300):
            got = gpu_frame(rt, gpu[(mf, 0)], W, H, BOX)
            want = ref.frame("normal", mf, W, H, BOX, 0)
            compare(*got, *want, f"{W}x{H} boxes min_faces {mf}")
            assert got[0].reshape(-1, 3).tobytes() == want[0].tobytes()
    # frames in flight: four slots, five frames of alternating modes and sizes queued back to back
    fly = rt.Scene(meshes["normal"], frames_in_flight=4)
    cam = rt.flycam(W, H, *CAMERA)
    for mode in (PRIMARY, FULL):
        want = gpu_frame(rt, gpu[(300, 0)], W, H, mode, 3)
        for k in range(4):
            w2, h2 = FRAME_SIZES[k % 3]
            fly.render_async(rt.flycam(w2, h2, *CAMERA), rt.DEFAULT_LIGHTS, w2, h2, mode=(mode + k) % 2, max_depth=k % 3,
                             flags=rt.RT_FRAME_WRITE_HITS)
        fly.render_async(cam, rt.DEFAULT_LIGHTS, W, H, mode=mode, max_depth=3, flags=rt.RT_FRAME_WRITE_HITS)
        fly.synchronize()
        assert same_frames(want, fly.download(W, H, want_hits=True)), f"mode {mode}: the frame in flight differs"
    assert thr > 0
    report(f"mesh edges frames {W}x{H} (pixels as rays)", px, hits, thr, bad)


@pytest.mark.parametrize("bits", PRODUCT_VARIANTS)
def test_product_variants_on_mesh_edges(rt, ref, gpu, bits):
    """Every kernel variant the product library serves renders the normal-scene frames (PRIMARY, FULL; max_depth 0, 1
    and 3; the three frame sizes) and answers the lattice / random / shadow lists with the default kernels' bits --
    which the tests above hold to the oracle."""
    n = 0
    for key, sc in gpu.items():
        rays = {k: ref.rays[k] for k in ("lattice", "random", "shadow")}
        prev = rt.set_variant(0)
        try:
            want_f = {(WH, mode, dep): gpu_frame(rt, sc, *WH, mode, dep) for WH in FRAME_SIZES for mode in (PRIMARY, FULL)
                      for dep in (0, 1, 3)}
            want_r = {k: sc.trace_closest(*r) + (sc.trace_shadow(*r),) for k, r in rays.items()}
            rt.set_variant(bits)
            for k in want_f:
                assert same_frames(want_f[k], gpu_frame(rt, sc, *k[0], k[1], k[2])), (bits, key, k)
                n += k[0][0] * k[0][1]
            for k, r in rays.items():
                assert same_frames(want_r[k], sc.trace_closest(*r) + (sc.trace_shadow(*r),)), (bits, key, k)
                n += 2 * len(r[0])
        finally:
            rt.set_variant(prev)
    # the 64x40 frames of the default build once more against the oracle, under the variant
    thr = bad = 0
    for mode in (PRIMARY, FULL):
        want = ref.frame("normal", 300, 64, 40, mode, 0)
        got = with_variant(rt, bits, lambda: gpu_frame(rt, gpu[(300, 0)], 64, 40, mode))
        compare(*got, *want, f"variant {bits} mode {mode}")
        thr += int((want[1] >= NFRONT).sum())
        bad += frame_bad(got, want)
    report(f"mesh edges variant {bits} vs default kernels and the oracle", n, 0, thr, bad)


def lit_back_pixels(ref, W, H, lights):
    """From the oracle alone: the back-grid pixels of the frame that some light reaches (shadow() per light)."""
    orc, osc = ref.orc, ref.scene("normal")
    ocam = orc.flycam(W, H, *CAMERA)
    od = [orc.camera_ray(ocam, i, j) for j in range(H) for i in range(W)]
    face, t, P = osc.closest(np.array([x[0] for x in od], np.float32), np.array([x[1] for x in od], np.float32))
    Pb = P[face >= NFRONT]
    blocked = np.zeros(len(Pb), np.int64)
    for pos, _ in lights:
        L = -(Pb - np.array(pos, np.float32))
        blocked += osc.shadow(Pb, (L / np.linalg.norm(L, axis=1, keepdims=True)).astype(np.float32))
    return int((blocked < len(lights)).sum())


@pytest.mark.parametrize("WH", FRAME_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_33_lights_with_and_without_the_occluder_cache(rt, ref, gpu, WH):
    """ring_lights(33) -- one more than the kernel-argument path takes, so the memory-lights kernels run -- through a
    light set: rt_render_lit frames (PRIMARY / FULL, max_depth 0 and 3) and rt_trace_stream_lit of the frame's camera
    rays (in order, and reordered + wavefront), with the occluder cache and with the variant bit that turns it off,
    against the oracle; the list equals the frame bit for bit. The cached pre-test must let light through rejected
    faces: the oracle's count of back-grid pixels some light reaches is non-zero [64x40: 150 of 150; 6 of 6 in the
    other two]."""
    W, H = WH
    lights = E.ring_lights(33)
    lit = lit_back_pixels(ref, W, H, lights)
    assert lit > 0
    sc = gpu[(300, 0)]
    cam = rt.flycam(W, H, *CAMERA)
    ls = sc.light_set(lights)
    o, d = sc.camera_rays(cam, W, H)
    px = hits = thr = bad = 0
    for variant in (0, NO_CACHE):
        for mode in (PRIMARY, FULL):
            for depth in (0, 3):
                what = f"{W}x{H} 33 lights mode {mode} depth {depth} variant {variant}"
                want = ref.frame("normal", 300, W, H, mode, depth, "ring33")
                rgb, face, t, _ = with_variant(rt, variant, lambda: sc.render_lit(cam, ls, W, H, mode=mode, max_depth=depth,
                                                                                  want_hits=True))
                compare(rgb, face, t, *want, what + ": render_lit")
                frame = {"rgb": rgb.reshape(-1, 3), "face": face.reshape(-1), "t": t.reshape(-1)}
                for reorder, wavefront in ((False, False), (True, True)):
                    got = with_variant(rt, variant, lambda: lit_trace(sc, o, d, ls, mode, depth, reorder, wavefront))
                    assert_same(got, frame, what + f": trace_stream_lit reorder={reorder} wavefront={wavefront}")
                px += W * H
                hits += int((want[1] >= 0).sum())
                thr += int((want[1] >= NFRONT).sum())
                bad += frame_bad((rgb, face, t), want)
    report(f"mesh edges 33 lights {W}x{H} (lit back-grid pixels {lit})", px, hits, thr, bad)


def normal_restatement(ref, P, face):
    """The reference's interpolated normal at the oracle's hit points of the normal scene, in float32 numpy
    (edge_scenes.blend_normal_f32: held to the oracle's pinned arithmetic in tests/test_mesh_edges_host.py)."""
    (v, f, _, _), vn = ref.arrays["normal"]
    w = v.copy()
    w[:, 2] += np.float32(E.NORMAL_PLANE_Z)
    tri = f[face]
    nn = E.normalized_f32(vn)
    return E.blend_normal_f32(w[tri[:, 0]], w[tri[:, 1]], w[tri[:, 2]], nn[tri[:, 0]], nn[tri[:, 1]], nn[tri[:, 2]], P)


@pytest.mark.parametrize("rays", ["lattice", "random"])
def test_ray_lists_match_the_oracle(rt, ref, gpu, rays):
    """rt_trace_stream, all three queries, in order and reordered, and the host-pointer calls (trace_closest_normal,
    trace_shadow, trace_color) on the lattice and random lists: face, t, P and blocked equal the oracle's bit for
    bit; N is the same bits in every call and, on hits of unflagged faces, the bits of the float32 numpy restatement
    of the reference's blend (NaN equal to NaN); rt_trace_stream_color in PRIMARY and FULL at max_depth 1, 2 and 4,
    in order / reordered / wavefront / both: face and t equal the oracle's closest hit, and rgb, face and t are the
    same bits in every flag combination (and trace_color's, for FULL at depth 2)."""
    a, b = ref.rays[rays]
    n_bad = 0
    for key in ((300, 0), (8, 1)):
        sc, mf = gpu[key], key[0]
        flagged = (sc.face_flags()[0] & SAFE) != 0
        of, ot, oP = ref.closest("normal", mf, rays)
        ob = ref.shadow("normal", mf, rays)
        host = dict(zip(("face", "t", "P", "N"), sc.trace_closest_normal(a, b)))
        n_bad += closest_bad((host["face"], host["t"], host["P"]), (of, ot, oP))
        assert closest_bad((host["face"], host["t"], host["P"]), (of, ot, oP)) == 0, f"{rays} {key}: trace_closest_normal"
        hit = of >= 0
        unfl = hit & ~flagged[np.maximum(of, 0)]
        want_n = normal_restatement(ref, oP[hit], of[hit])
        okn = same_bits(host["N"][hit], want_n).all(1)
        print(f"{rays} {key}: hits {int(hit.sum())}, on unflagged faces {int(unfl.sum())}, N differs on unflagged "
              f"{int((~okn & unfl[hit]).sum())}, on flagged {int((~okn & ~unfl[hit]).sum())}")
        assert unfl.sum() >= 1000 and okn[unfl[hit]].all(), f"{rays} {key}: N differs from the reference's blend"
        for reorder in (False, True):
            what = f"{rays} {key} reorder={reorder}"
            assert_same(stream_trace(rt, sc, Q_CLOSEST, a, b, reorder=reorder), host, what + ": closest")
            got = stream_trace(rt, sc, Q_SHADOW, a, b, reorder=reorder)["blocked"]
            assert (got == ob).all() and (sc.trace_shadow(a, b) == ob).all(), what + ": shadow"
            col = stream_trace(rt, sc, Q_COLOR, a, b, lights=rt.DEFAULT_LIGHTS, reorder=reorder)
            assert_same(col, dict(zip(("rgb", "face", "t"), sc.trace_color(a, b, rt.DEFAULT_LIGHTS))), what + ": colour")
            assert (col["face"] == of).all() and same_bits(col["t"], ot).all(), what + ": colour face / t"
        ta, tb = dev(a), dev(b)
        for mode in (PRIMARY, FULL):
            for depth in (1, 2, 4):
                first = None
                for reorder, wavefront in COMBOS:
                    res = sc.trace_stream_color(ta, tb, rt.DEFAULT_LIGHTS, mode=mode, max_depth=depth, reorder=reorder,
                                                wavefront=wavefront)
                    got = {k: x.cpu().numpy() for k, x in res.items()}
                    what = f"{rays} {key} mode {mode} depth {depth} reorder={reorder} wavefront={wavefront}"
                    assert (got["face"] == of).all() and same_bits(got["t"], ot).all(), what
                    if first is None:
                        first = got
                    assert_same(got, first, what)
                if mode == FULL and depth == 2:
                    assert_same(first, dict(zip(("rgb", "face", "t"), sc.trace_color(a, b, rt.DEFAULT_LIGHTS))), "trace_color")
    report(f"mesh edges ray lists {rays} (streams, colour lists, N)", 2 * len(a), 2 * int((of >= 0).sum()),
           ref.through("normal", 300, rays) + ref.through("normal", 8, rays), n_bad)


def test_camera_ray_lists_match_the_oracle_frames(rt, ref, gpu):
    """The 64x40 frame's camera rays through rt_trace_stream_color (PRIMARY and FULL, max_depth 1, 2 and 4, every
    flag combination) and trace_color: rgb, face and t against the oracle's pixel of the same ray, and the frame's
    bits."""
    W, H = 64, 40
    sc = gpu[(300, 0)]
    o, d = sc.camera_rays(rt.flycam(W, H, *CAMERA), W, H)
    thr = bad = 0
    for mode in (PRIMARY, FULL):
        for depth in (1, 2, 4):
            want = ref.frame("normal", 300, W, H, mode, depth)
            frame = dict(zip(("rgb", "face", "t"), (x.reshape(-1, 3) if x.ndim == 3 else x.reshape(-1)
                                                    for x in gpu_frame(rt, sc, W, H, mode, depth))))
            for reorder, wavefront in COMBOS:
                res = sc.trace_stream_color(o, d, rt.DEFAULT_LIGHTS, mode=mode, max_depth=depth, reorder=reorder,
                                            wavefront=wavefront)
                got = {k: x.cpu().numpy() for k, x in res.items()}
                what = f"camera rays mode {mode} depth {depth} reorder={reorder} wavefront={wavefront}"
                compare(got["rgb"], got["face"], got["t"], *want, what)
                assert_same(got, frame, what + ": list vs frame")
            thr += int((want[1] >= NFRONT).sum())
            bad += frame_bad((frame["rgb"], frame["face"], frame["t"]), want)
    want = ref.frame("normal", 300, W, H, FULL, 0)
    rgb, face, t = sc.trace_color(o.cpu().numpy(), d.cpu().numpy(), rt.DEFAULT_LIGHTS)
    compare(rgb, face, t, *want, "trace_color of the camera rays")
    report("mesh edges camera-ray lists 64x40", 6 * W * H, 6 * int((want[1] >= 0).sum()), thr, bad)


def test_view_batches_and_supersampling(rt, ref, gpu):
    """render_views with three cameras equals rt_render's frames bit for bit (PRIMARY and FULL at depth 3); the
    supersampled batch with the 2x2 grid equals the in-order mean of rt_render's frames of the shifted cameras, in the
    loop layout and in the packed one (S = 4) -- colours bit for bit with NaN equal to NaN, face and t sample 0's."""
    W, H = 64, 40
    sc = gpu[(300, 0)]
    cams = [rt.flycam(W, H, *CAMERA), rt.flycam(W, H, 2.0, -1.0, 20.0), rt.flycam(W, H, -3.0, 2.0, 17.0)]
    offs = rt.sample_pattern((2, 2)).array()
    nan = thr = 0
    for mode, depth in ((PRIMARY, 0), (FULL, 3)):
        frames = [sc.render(c, rt.DEFAULT_LIGHTS, W, H, mode=mode, max_depth=depth, want_hits=True)[:3] for c in cams]
        want = {k: np.stack([f[i] for f in frames]) for i, k in enumerate(("rgb", "face", "t"))}
        nan += int(np.isnan(want["rgb"]).any(-1).sum())
        thr += int((want["face"] >= NFRONT).sum())
        full, out = sentinel_buffers(len(cams), H, W, ("rgb", "face", "t"))
        torch.cuda.synchronize()
        sc.render_views(cams, rt.DEFAULT_LIGHTS, W, H, mode=mode, max_depth=depth, out=out)
        assert_views(collect(full, out), want, f"render_views mode {mode} depth {depth}")
        comp = {"rgb": [], "face": [], "t": []}
        for c in cams:
            fr = [sc.render(shifted(c, ox, oy), rt.DEFAULT_LIGHTS, W, H, mode=mode, max_depth=depth, want_hits=True)[:3]
                  for ox, oy in offs]
            with np.errstate(invalid="ignore"):
                comp["rgb"].append(in_order_mean([f[0] for f in fr]))
            comp["face"].append(fr[0][1])
            comp["t"].append(fr[0][2])
        comp = {k: np.stack(x) for k, x in comp.items()}
        for layout in (LOOP, PACKED):
            v = layout_variant(rt, 4, layout)
            assert v is not None

            def run():
                full, out = sentinel_buffers(len(cams), H, W, ("rgb", "face", "t"))
                torch.cuda.synchronize()
                sc.render_views(cams, rt.DEFAULT_LIGHTS, W, H, mode=mode, max_depth=depth, out=out, samples=(2, 2))
                return collect(full, out)
            got = with_variant(rt, v, run)
            what = f"supersampled mode {mode} depth {depth} layout {layout}"
            assert same_bits(got["rgb"], comp["rgb"]).all(), what + ": rgb"
            assert (got["face"] == comp["face"]).all() and same_bits(got["t"], comp["t"]).all(), what + ": face / t"
    assert nan > 0 and thr > 0
    report("mesh edges view batches (3 views, 2x2 samples, both layouts)", 2 * 3 * W * H, 0, thr, 0)


def test_scene_cache_keeps_flags_and_bits(rt, ref, gpu, tmp_path):
    """The normal scene and the degenerate scene saved and loaded: the same face_flags() and record_flags(), the
    same frame bits (PRIMARY and FULL at depth 3) and the same closest-hit / shadow bits on the lattice list."""
    for key in ((300, 0), (8, 1), "degenerate"):
        orig = gpu[key]
        p = tmp_path / "mesh_edges.rtscene"
        orig.save(p)
        ld = rt.Scene.load(p, wide_tree=0 if key == "degenerate" else key[1])
        assert (orig.face_flags()[0] == ld.face_flags()[0]).all() and orig.face_flags()[1] == ld.face_flags()[1]
        assert orig.record_flags() == ld.record_flags() and 0 < orig.record_flags()[1] < orig.record_flags()[0]
        for mode, depth in ((PRIMARY, 0), (FULL, 3)):
            assert same_frames(gpu_frame(rt, orig, 64, 40, mode, depth), gpu_frame(rt, ld, 64, 40, mode, depth)), (key, mode)
        a, b = ref.rays["lattice"]
        assert same_frames(orig.trace_closest(a, b) + (orig.trace_shadow(a, b),), ld.trace_closest(a, b) + (ld.trace_shadow(a, b),))


def test_flags_on_the_device_builds(rt, ref, gpu, meshes):
    """The flag does not depend on the builder or the device: the default builds carry it on exactly the faces whose
    vertices are all of class P, S or U (and the back grid), none of the zero-area faces, and no micro-fan triangle
    whose A is 0."""
    (v, f, _, _), _ = ref.arrays["normal"]
    want = np.array([all(c in "PSU" for c in ref.cls[tri]) for tri in f[:NFRONT]] + [True] * 8)
    for key in ((8, 0), (300, 0), (8, 1), (300, 1)):
        assert (((gpu[key].face_flags()[0] & SAFE) != 0) == want).all(), key
    dflag = (gpu["degenerate"].face_flags()[0] & SAFE) != 0
    assert not dflag[ref.added].any() and (dflag[ref.new_id] == want).all()
    (mv, mf, _, _), _ = ref.arrays["micro"]
    w = mv.copy()
    w[:, 2] += np.float32(E.MICRO_PLANE_Z)
    A = E.area_f32(w[mf[:, 0]], w[mf[:, 1]], w[mf[:, 2]])
    mflag = (rt.Scene(meshes["micro"]).face_flags()[0] & SAFE) != 0
    assert (A == 0).any() and (mflag == (A > np.float32(1e-30))).all()
    assert TOL == 1e-4 and colour_errors(np.float32([[np.nan, 1, 2]]), np.float32([[0, 1, 2]]))[0] == 1
