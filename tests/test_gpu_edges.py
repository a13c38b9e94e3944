"""Edge-case parity battery (MI355X): the packet kernels against the CPU oracle on the inputs of
tests/edge_scenes.py -- faces at bit-identical t (the tie goes to the reference's box-then-in-box rank),
axis-aligned rays with +0.0 / -0.0 components on reference-box planes (NaN slabs), origins exactly on a face
plane (t = +0 / -0), the shadow offset straddling a plane, d = 0, ray lists of odd lengths, small ragged frames
with shards / repeats / every max_depth, 0 and RT_MAX_LIGHTS lights, non-integer and boundary shininess, faces
without a material -- through every builder, leaf size, tree width and product kernel variant.
tests/test_edge_inputs.py asserts on the oracle alone that these inputs reach those edges.

Every comparison is with the oracle: face ids equal, t and P bit-identical, blocked equal; colours as in
tests/test_gpu_parity.py (non-finite positions identical, finite ones within 1e-4)."""
import ctypes as C

import numpy as np
import pytest

import edge_scenes as E
from conftest import PARITY_REPORT, scene_path
from kernel_variants import VARIANTS
from test_gpu_parity import TOL, compare
from test_oracle_pinning import same_bits

pytestmark = pytest.mark.gpu

PRODUCT_VARIANTS = [VARIANTS[n] for n in ("primary-binary-tree", "coarse-cost-buckets", "generic-depth-kernel", "split-primary",
                                           "dispatch-order", "full-8-waves", "full-small-build")]
FRAME_SIZES = [(37, 11), (65, 9), (64, 40)]
TIE_CAMERA = (3.0, -2.0, 20.0)  # flycam(W, H, dx, dy, dz): the triple plane nearly head-on from z = 1


@pytest.fixture(scope="module", autouse=True)
def need_gpu(rt):
    if rt.device_count() == 0:
        pytest.skip("no GPU")


class Ref:
    """The oracle's answers, computed once per module and never written to afterwards."""

    def __init__(self, orc):
        self.orc = orc
        (v, f, m, g), self.copy = E.tie_scene()
        self.tie_arrays = (v, f, m, g)
        self.tie = {mf: orc.Scene(orc.Mesh.from_arrays(v, f, m, groups=g), min_faces=mf) for mf in (8, 300)}
        self.cube = orc.Scene(orc.Mesh.load_obj(scene_path("cube.obj")))
        self.rays = {"random": E.tie_random_rays(), "lattice": E.tie_lattice_rays()[:2],
                     "cube-lattice": E.cube_lattice_rays()[:2], "on-plane": E.on_plane_rays()[:2],
                     "zero-d": E.zero_direction_rays(), "straddle": E.shadow_straddle_rays()}
        self._closest, self._shadow, self._nan, self._frames = {}, {}, {}, {}

    def scene(self, which):
        return self.cube if which == "cube" else self.tie[which]

    def closest(self, which, rays):
        key = (which, rays)
        if key not in self._closest:
            out = self.scene(which).closest(*self.rays[rays])
            for a in out:
                a.setflags(write=False)
            self._closest[key] = out
        return self._closest[key]

    def shadow(self, which, rays):
        key = (which, rays)
        if key not in self._shadow:
            out = self.scene(which).shadow(*self.rays[rays])
            out.setflags(write=False)
            self._shadow[key] = out
        return self._shadow[key]

    def nan_rays(self, which, rays):
        key = (which, rays)
        if key not in self._nan:
            sc = self.scene(which)
            o, d = self.rays[rays]
            self._nan[key] = int(E.ref_slab_nan(sc.boxes()[0], sc.mesh.export()["M16"], o, d).sum())
        return self._nan[key]

    def frame(self, mf, W, H, mode, depth):
        """mode 'primary' | 'full' | 'boxes'; depth 0 = the mode's own."""
        key = (mf, W, H, mode, depth)
        if key not in self._frames:
            orc, sc = self.orc, self.tie[mf]
            cam = orc.flycam(W, H, *TIE_CAMERA)
            if mode == "boxes":
                out = sc.render(cam, orc.DEFAULT_LIGHTS, W, H, box_colors=orc.box_colors_glibc(sc.box_count()))
            else:
                out = sc.render(cam, orc.DEFAULT_LIGHTS, W, H, full=(mode == "full"), max_depth=depth or None)
            self._frames[key] = out
        return self._frames[key]


@pytest.fixture(scope="module")
def ref(orc):
    return Ref(orc)


@pytest.fixture(scope="module")
def tie_mesh(rt, ref):
    v, f, m, g = ref.tie_arrays
    return rt.Mesh.from_arrays(v, f, m, groups=g)


@pytest.fixture(scope="module")
def tie_gpu(rt, tie_mesh):
    """The default build (device SBVH, device boxes) of the tie scene per min_faces, and a host-SBVH build with
    the 4-wide tree (what variant 2097152 turns off)."""
    return {(mf, wide): rt.Scene(tie_mesh, min_faces=mf, wide_tree=wide,
                                 builder=rt.RT_BUILDER_SBVH if wide else rt.RT_BUILDER_SBVH_GPU)
            for mf in (8, 300) for wide in (0, 1)}


def closest_mismatches(sc, ref, which, rays):
    """rays whose face / t bits / P bits differ from the oracle's (closest hit)"""
    o, d = ref.rays[rays]
    face, t, P = sc.trace_closest(o, d)
    of, ot, oP = ref.closest(which, rays)
    bad = (face != of) | ~same_bits(t, ot) | ~same_bits(P, oP).all(1)
    return int(bad.sum()), int((of >= 0).sum())


def shadow_mismatches(sc, ref, which, rays):
    P, L = ref.rays[rays]
    return int((sc.trace_shadow(P, L) != ref.shadow(which, rays)).sum()), int(ref.shadow(which, rays).sum())


def report(name, rays, hits, nan, bad):
    PARITY_REPORT.append(f"{name}: rays {rays}, hits {hits}, NaN-slab rays {nan}, mismatches {bad}")


BUILDERS = {"sbvh": "RT_BUILDER_SBVH", "sah": "RT_BUILDER_SAH", "sbvhgpu": "RT_BUILDER_SBVH_GPU",
            "sahgpu": "RT_BUILDER_SAH_GPU", "ploc": "RT_BUILDER_PLOC_GPU", "lbvh": "RT_BUILDER_LBVH_GPU"}


@pytest.mark.parametrize("builder", sorted(BUILDERS))
def test_ties_resolve_by_reference_rank(rt, ref, tie_mesh, builder):
    """Three faces at bit-identical t on every ray: the winner is the oracle's (first in reference-box order,
    then in-box order) whatever the tree -- host SBVH / SAH, device SBVH / SAH / PLOC / LBVH, leaf sizes 1, 2
    and 16, binary and 4-wide trees, 68 and 4 reference boxes -- on 4,096 random rays (for 40% of which, with
    min_faces 8, the winner is not the lowest face id) and the 1,976 lattice rays."""
    bid = getattr(rt, BUILDERS[builder])
    n_rays = n_hits = n_bad = n_scenes = 0
    for leaf in (1, 2, 16):
        for wide in (0, 1):
            for mf in (8, 300):
                sc = rt.Scene(tie_mesh, builder=bid, leaf_size=leaf, wide_tree=wide, min_faces=mf)
                assert sc.info()["builder"] == bid and sc.info()["n_ref_boxes"] == ref.tie[mf].box_count()
                n_scenes += 1
                for rays in ("random", "lattice"):
                    bad, hits = closest_mismatches(sc, ref, mf, rays)
                    n_rays += len(ref.rays[rays][0])
                    n_hits += hits
                    n_bad += bad
                    assert bad == 0, f"{builder} leaf {leaf} wide {wide} min_faces {mf} {rays}: {bad} rays differ"
    report(f"edge ties {builder} ({n_scenes} scenes)", n_rays, n_hits,
           ref.nan_rays(8, "lattice") + ref.nan_rays(300, "lattice"), n_bad)


def test_axis_aligned_and_plane_grazing_rays(rt, ref, tie_gpu):
    """d = +-e_k with zero components of both signs, origins on lattice and reference-box plane coordinates
    (0 / 0 in the reference's slabs; in-plane rays along the triple plane; back-facing hits from the far plane),
    on the cube and the tie scene: trace_closest and trace_shadow equal the oracle's; d = (+-0, +-0, +-0) misses."""
    cube = rt.Scene(rt.Mesh.load_obj(scene_path("cube.obj")))
    cases = [(cube, "cube", "cube-lattice")] + [(tie_gpu[(mf, w)], mf, r) for mf in (8, 300) for w in (0, 1)
                                                 for r in ("lattice", "zero-d")]
    tot = [0, 0, 0, 0]
    for sc, which, rays in cases:
        bad, hits = closest_mismatches(sc, ref, which, rays)
        sbad, blocked = shadow_mismatches(sc, ref, which, rays)
        nan = ref.nan_rays(which, rays)
        for k, x in enumerate((len(ref.rays[rays][0]), hits, nan, bad + sbad)):
            tot[k] += x
        assert bad == 0 and sbad == 0, f"{which} {rays}: closest {bad}, shadow {sbad} rays differ"
        if rays == "zero-d":
            assert hits == 0 and blocked == 0
    report("edge axis-aligned", *tot)


def test_origins_on_a_face_plane(rt, ref, tie_gpu):
    """Origins exactly on the triple plane: closest hits with t = +0 and t = -0 (38% / 37% of the rays; sign
    included, t is compared bitwise), in-plane directions missing, and shadow() of the same rays."""
    tot = [0, 0, 0, 0]
    for (mf, w), sc in tie_gpu.items():
        bad, hits = closest_mismatches(sc, ref, mf, "on-plane")
        sbad, _ = shadow_mismatches(sc, ref, mf, "on-plane")
        t = sc.trace_closest(*ref.rays["on-plane"])[1]
        assert (t.view(np.uint32) == 0x80000000).any() and (t.view(np.uint32) == 0).any()
        for k, x in enumerate((len(t), hits, ref.nan_rays(mf, "on-plane"), bad + sbad)):
            tot[k] += x
        assert bad == 0 and sbad == 0, f"min_faces {mf} wide {w}: closest {bad}, shadow {sbad} rays differ"
    report("edge on-plane origins", *tot)


def test_shadow_offset_straddle(rt, ref, tie_gpu):
    """shadow(P, L) with P + 0.003 L just above, about on and just below the triple plane while the box test
    starts at P below it."""
    tot = [0, 0, 0, 0]
    for (mf, w), sc in tie_gpu.items():
        sbad, blocked = shadow_mismatches(sc, ref, mf, "straddle")
        for k, x in enumerate((len(ref.rays["straddle"][0]), blocked, ref.nan_rays(mf, "straddle"), sbad)):
            tot[k] += x
        assert sbad == 0, f"min_faces {mf} wide {w}: {sbad} rays differ"
    report("edge shadow straddle (hits = blocked)", *tot)


SENT_I, SENT_F = -123456789, np.float32(-7.5e33)
CAP = 257 + 31


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_ray_list_lengths(rt, orc, ref, tie_gpu):
    """n in {0, 1, 63, 64, 65, 255, 256, 257} through rt_trace_closest / _closest_normal / _shadow / _color: the
    last wave is padded with inactive copies of its first ray, so every prefix must equal the same prefix of the
    257-ray answer and the oracle's, nothing past n may be written (sentinel-filled outputs), and n = 0 returns
    RT_OK without touching anything."""
    sc = tie_gpu[(8, 0)]
    L = rt.lib()
    sel = np.r_[0:150, 900:1007]  # lattice rays along x and along z
    o, d = (np.ascontiguousarray(a[sel]) for a in ref.rays["lattice"])
    of, ot, oP = ref.tie[8].closest(o, d)
    ob = ref.tie[8].shadow(o, d)
    assert 40 < (of >= 0).sum() < 257 and 20 < ob.sum() < 257
    # traceRay colours: the first 257 pixels' camera rays of the 37x11 frame, against the oracle's FULL frame
    W, H = 37, 11
    ocam = orc.flycam(W, H, *TIE_CAMERA)
    pix = [(k % W, k // W) for k in range(257)]
    rays = [orc.camera_ray(ocam, i, j) for i, j in pix]
    co = np.ascontiguousarray(np.array([a for a, _ in rays], np.float32))
    cd = np.ascontiguousarray(np.array([b for _, b in rays], np.float32))
    crgb, cface, ct = (a[:257] for a in ref.frame(8, W, H, "full", 0))
    lights = sc._lights(rt.DEFAULT_LIGHTS)
    full = None
    n_bad = 0
    for n in (257, 0, 1, 63, 64, 65, 255, 256):
        face = np.full(CAP, SENT_I, np.int32)
        t = np.full(CAP, SENT_F, np.float32)
        P = np.full((CAP, 3), SENT_F, np.float32)
        N = np.full((CAP, 3), SENT_F, np.float32)
        face2, t2, P2 = face.copy(), t.copy(), P.copy()
        blocked = np.full(CAP, SENT_I, np.int32)
        rgb = np.full((CAP, 3), SENT_F, np.float32)
        face3, t3 = face.copy(), t.copy()
        assert L.rt_trace_closest(sc.h, n, _ptr(o), _ptr(d), _ptr(face2), _ptr(t2), _ptr(P2)) == 0
        assert L.rt_trace_closest_normal(sc.h, n, _ptr(o), _ptr(d), _ptr(face), _ptr(t), _ptr(P), _ptr(N)) == 0
        assert L.rt_trace_shadow(sc.h, n, _ptr(o), _ptr(d), _ptr(blocked)) == 0
        assert L.rt_trace_color(sc.h, n, _ptr(co), _ptr(cd), C.cast(lights, C.c_void_p), 1, _ptr(rgb), _ptr(face3),
                                _ptr(t3)) == 0
        for a, s in ((face, SENT_I), (face2, SENT_I), (face3, SENT_I), (blocked, SENT_I), (t, SENT_F), (t2, SENT_F),
                     (t3, SENT_F), (P, SENT_F), (P2, SENT_F), (N, SENT_F), (rgb, SENT_F)):
            assert (a[n:] == s).all(), f"n = {n}: written past the end"
        if n == 257:
            full = (face.copy(), t.copy(), P.copy(), N.copy(), blocked.copy(), rgb.copy(), face3.copy(), t3.copy())
        got = (face, t, P, N, blocked, rgb, face3, t3)
        for a, b in zip(got, full):
            assert a[:n].tobytes() == b[:n].tobytes(), f"n = {n}: differs from the 257-ray answer"
        bad = (face[:n] != of[:n]) | ~same_bits(t[:n], ot[:n]) | ~same_bits(P[:n], oP[:n]).all(1) | \
              (face2[:n] != of[:n]) | ~same_bits(t2[:n], ot[:n]) | ~same_bits(P2[:n], oP[:n]).all(1) | \
              (blocked[:n] != ob[:n])
        n_bad += int(bad.sum())
        assert not bad.any(), f"n = {n}: {int(bad.sum())} rays differ from the oracle"
        if n:
            compare(rgb[:n], face3[:n], t3[:n], crgb[:n], cface[:n], ct[:n], f"trace_color n = {n}")
        hitN = N[:n][face[:n] >= 0]
        assert np.isfinite(hitN).all() and (np.abs(np.linalg.norm(hitN, axis=1) - 1) < 1e-5).all()
    # a null pointer with n = 0 is fine: nothing is read or written
    assert L.rt_trace_closest(sc.h, 0, None, None, None, None, None) == 0
    assert L.rt_trace_shadow(sc.h, 0, None, None, None) == 0
    report("edge ray-list lengths (8 lengths x 4 queries)", 257, int((of >= 0).sum()),
           int(E.ref_slab_nan(ref.tie[8].boxes()[0], ref.tie[8].mesh.export()["M16"], o, d).sum()), n_bad)


def gpu_frame(rt, sc, W, H, mode, depth=0, shard=(0, 1), flags=0):
    m = {"primary": rt.RT_MODE_PRIMARY, "full": rt.RT_MODE_FULL, "boxes": rt.RT_MODE_BOX_COLORS}[mode]
    rgb, face, t, _ = sc.render(rt.flycam(W, H, *TIE_CAMERA), rt.DEFAULT_LIGHTS, W, H, mode=m, want_hits=True,
                                max_depth=depth, shard=shard, flags=flags)
    return rgb, face, t


def same_frames(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("WH", FRAME_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_edge_frames(rt, ref, tie_mesh, tie_gpu, WH):
    """The tie scene nearly head-on (every hit pixel a three-way tie) in ragged frames: PRIMARY / FULL at
    max_depth 0, 1 and 3 and RT_MODE_BOX_COLORS against the oracle (68 and 4 reference boxes, binary and 4-wide
    trees); the 3-shard stitch equals the whole frame; twenty frames on a one-slot scene (longest-first order
    from the second frame, sub-wave split of the costliest waves, whose merge decides rank ties again) render
    the same bits every time."""
    W, H = WH
    px = hits = bad = 0
    for (mf, wide), sc in tie_gpu.items():
        for mode in ("primary", "full", "boxes"):
            for depth in ((0,) if mode == "boxes" else (0, 1, 3)):
                rgb, face, t = gpu_frame(rt, sc, W, H, mode, depth)
                orgb, oface, ot = ref.frame(mf, W, H, mode, depth)
                px += W * H
                hits += int((oface >= 0).sum())
                bad += int(((face.reshape(-1) != oface) | ~same_bits(t.reshape(-1), ot)).sum())
                if mode == "boxes":
                    compare(rgb, face, t, orgb, oface, ot, f"{W}x{H} boxes mf {mf}")
                    assert rgb.reshape(-1, 3).tobytes() == orgb.tobytes()
                else:
                    compare(rgb, face, t, orgb, oface, ot, f"{W}x{H} {mode} depth {depth} mf {mf} wide {wide}")
            whole = gpu_frame(rt, sc, W, H, mode)
            out = [np.full((H, W, 3), np.nan, np.float32), np.full((H, W), -7, np.int32), np.full((H, W), np.nan, np.float32)]
            cover = np.zeros((H, W), np.int32)
            for k in range(3):
                part = gpu_frame(rt, sc, W, H, mode, shard=(k, 3))
                mask = rt.shard_mask(W, H, k, 3)
                cover += mask
                for dst, src in zip(out, part):
                    dst[mask] = src[mask]
            assert (cover == 1).all() and same_frames(whole, out), f"{mode}: 3 shards stitched != whole frame"
    assert hits >= px // 8
    for mf in (8, 300):
        solo = rt.Scene(tie_mesh, min_faces=mf, frames_in_flight=1)
        for mode in ("primary", "full"):
            first = gpu_frame(rt, solo, W, H, mode)
            orgb, oface, ot = ref.frame(mf, W, H, mode, 0)
            compare(*first, orgb, oface, ot, f"{W}x{H} {mode} one slot")
            for k in range(20):
                assert same_frames(first, gpu_frame(rt, solo, W, H, mode)), f"{mode} repeat {k} differs"
    report(f"edge frames {W}x{H} (pixels as rays)", px, hits, 0, bad)


def test_edge_frames_wave_split_engages(rt, tie_mesh):
    """The 64x40 frame has 48 waves (>= 32): lone frames after a slot's first are dispatched longest-first."""
    solo = rt.Scene(tie_mesh, min_faces=8, frames_in_flight=1)
    for k in range(3):
        gpu_frame(rt, solo, 64, 40, "full")
    lpt = solo.lpt_stats()
    assert lpt["frames"] == 3 and lpt["valid"], lpt


def test_materials_and_light_counts(rt, orc):
    """The material scene (Ns 0, 1, 0.5, 2.5, 16, 324, 1023, 1024, 1e4, 100.25 and a group without material) with
    0, 1 and RT_MAX_LIGHTS (32) lights, PRIMARY and FULL: faces and t bit-exact, NaN colours (negative base to a
    non-integer power: 38 .. 74 pixels) at the oracle's positions, finite colours within 1e-4; 33 lights are
    refused."""
    v, f, m, g = E.material_scene()
    sc = rt.Scene(rt.Mesh.from_arrays(v, f, m, groups=g))
    osc = orc.Scene(orc.Mesh.from_arrays(v, f, m, groups=g))
    W, H, dx, dy, dz = E.MATERIAL_CAMERA
    px = hits = nans = 0
    worst = 0.0
    for lights in ([], rt.DEFAULT_LIGHTS, E.ring_lights(32)):
        for full in (False, True):
            rgb, face, t, _ = sc.render(rt.flycam(W, H, dx, dy, dz), lights, W, H,
                                        mode=rt.RT_MODE_FULL if full else rt.RT_MODE_PRIMARY, want_hits=True)
            orgb, oface, ot = osc.render(orc.flycam(W, H, dx, dy, dz), lights, W, H, full=full)
            worst = max(worst, compare(rgb, face, t, orgb, oface, ot, f"materials {len(lights)} lights full {full}"))
            px += W * H
            hits += int((oface >= 0).sum())
            nans += int(np.isnan(orgb).any(1).sum())
            if lights:
                assert np.isnan(rgb).any()
    assert TOL == 1e-4
    with pytest.raises(rt.RTError, match="invalid"):
        sc.render(rt.flycam(W, H, dx, dy, dz), E.ring_lights(33), W, H)
    PARITY_REPORT.append(f"edge materials: pixels {px}, hits {hits}, NaN-colour pixels {nans} (positions identical), "
                         f"mismatches 0, finite colour L_inf {worst:.3g}")


@pytest.mark.parametrize("bits", PRODUCT_VARIANTS)
def test_product_variants_on_edge_inputs(rt, ref, tie_gpu, bits):
    """Every kernel variant the product library serves renders the tie-scene frames (PRIMARY, FULL, box colours;
    max_depth 0 and 3) and answers the lattice / on-plane / straddle ray lists with the default kernels' bits."""
    n = 0
    for (mf, wide), sc in tie_gpu.items():
        rays = {k: ref.rays[k] for k in ("lattice", "on-plane", "straddle")}
        prev = rt.set_variant(0)
        try:
            want_f = {(WH, mode, dep): gpu_frame(rt, sc, *WH, mode, dep) for WH in FRAME_SIZES
                      for mode in ("primary", "full", "boxes") for dep in ((0,) if mode == "boxes" else (0, 3))}
            want_r = {k: sc.trace_closest(*r) + (sc.trace_shadow(*r),) for k, r in rays.items()}
            rt.set_variant(bits)
            for key in want_f:
                assert same_frames(want_f[key], gpu_frame(rt, sc, *key[0], key[1], key[2])), (bits, mf, wide, key)
                n += key[0][0] * key[0][1]
            for k, r in rays.items():
                assert same_frames(want_r[k], sc.trace_closest(*r) + (sc.trace_shadow(*r),)), (bits, mf, wide, k)
                n += 2 * len(r[0])
        finally:
            rt.set_variant(prev)
    report(f"edge variant {bits} vs default kernels", n, 0, 0, 0)
