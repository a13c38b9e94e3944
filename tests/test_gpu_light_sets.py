"""Light sets on the GPU (MI355X): rt_render_lit / rt_trace_stream_lit with small sets against today's calls bit for
bit on both light paths (kernel arguments and device memory), beyond 32 lights against the CPU oracle, ray lists in
every flag combination, shards / frames in flight / multi-device scenes, and the wave-level occluder cache against
the same kernels without it.

Frames are 64x48 (cornell) and 64x40 (the material scene)."""
import numpy as np
import pytest
import torch

import edge_scenes as E
from conftest import scene_path
from test_gpu_ray_streams import PAD, SENT, assert_same, bits, collect

pytestmark = pytest.mark.gpu

TOL = 1e-4  # the suite's colour tolerance against the oracle (tests/test_gpu_ray_depth.py, test_gpu_edges.py)
PRIMARY, FULL, BOX = 0, 1, 2
MEM_LIGHTS, NO_CACHE = 8388608, 16777216
COMBOS = [(False, False), (True, False), (False, True), (True, True)]  # (reorder, wavefront)
# Where the soft light of the cornell frames sits. The penumbra counts below were checked on the CPU with the
# oracle and the real rt_lights_spherical jitter (100 lights: see shadow_census's docstring).
CORNELL_LIGHT = ((0.3, 0.45, 0.2), (1.0, 1.0, 1.0), 0.15)
MATERIAL_LIGHT = ((-0.5, 2.0, 3.0), (1.0, 1.0, 1.0), 0.5)


@pytest.fixture(scope="module", autouse=True)
def need_gpu(rt):
    if rt.device_count() == 0:
        pytest.skip("no GPU")


class Ref:
    def __init__(self, rt, orc, name):
        self.name = name
        if name == "cornell":
            self.W, self.H = 64, 48
            self.gpu = rt.Scene(rt.Mesh.load_obj(scene_path("cornell.obj")))
            self.orc = orc.Scene(orc.Mesh.load_obj(scene_path("cornell.obj")))
            self.cam, self.ocam = rt.flycam(self.W, self.H), orc.flycam(self.W, self.H)
            self.soft = CORNELL_LIGHT
        else:
            v, f, m, g = E.material_scene()
            self.W, self.H = E.MATERIAL_CAMERA[:2]
            self.gpu = rt.Scene(rt.Mesh.from_arrays(v, f, m, groups=g))
            self.orc = orc.Scene(orc.Mesh.from_arrays(v, f, m, groups=g))
            self.cam, self.ocam = rt.flycam(*E.MATERIAL_CAMERA), orc.flycam(*E.MATERIAL_CAMERA)
            self.soft = MATERIAL_LIGHT
        self.o, self.d = self.gpu.camera_rays(self.cam, self.W, self.H)
        self.sh = np.random.default_rng(41).permutation(self.W * self.H)
        tsh = torch.from_numpy(self.sh).cuda()
        self.o_sh, self.d_sh = self.o[tsh].contiguous(), self.d[tsh].contiguous()
        self._soft = {}
        self._plain = {}

    def soft_set(self, rt, n_points):
        """(lights, LightSet) of the scene's spherical light of n_points + 1 lights (a fresh rand() sequence)"""
        if n_points not in self._soft:
            lights = rt.spherical_light(self.soft[0], self.soft[1], self.soft[2], n_points)
            assert len(lights) == n_points + 1
            self._soft[n_points] = (lights, self.gpu.light_set(lights))
        return self._soft[n_points]

    def plain(self, rt, mode, depth):
        """the 100-light frame of the plain rt_render_lit call, rendered once per (mode, depth)"""
        if (mode, depth) not in self._plain:
            rgb, face, t, _ = self.gpu.render_lit(self.cam, self.soft_set(rt, 99)[1], self.W, self.H, mode=mode,
                                                  max_depth=depth, want_hits=True)
            self._plain[(mode, depth)] = frame_dict(rgb, face, t)
        return self._plain[(mode, depth)]


@pytest.fixture(scope="module")
def refs(rt, orc):
    return {name: Ref(rt, orc, name) for name in ("cornell", "material")}


def frame_dict(rgb, face, t):
    return {"rgb": rgb.reshape(-1, 3), "face": face.reshape(-1), "t": t.reshape(-1)}


def lit_trace(sc, a, b, ls, mode, depth, reorder=False, wavefront=False, stats=False):
    """rt_trace_stream_lit into sentinel-filled buffers of n + PAD elements (checked by collect)."""
    n = a.shape[0]
    full, out = {}, {}
    for name, w in (("rgb", 3), ("face", 1), ("t", 1)):
        buf = torch.full((n + PAD, 3) if w == 3 else (n + PAD,), int(SENT), dtype=torch.int32, device="cuda")
        if name != "face":
            buf = buf.view(torch.float32)
        full[name] = buf
        out[name] = buf[:n]
    sc.trace_stream_lit(a, b, ls, mode=mode, max_depth=depth, reorder=reorder, wavefront=wavefront, stats=stats, out=out)
    return collect(full, n)


def with_variant(rt, v, fn):
    prev = rt.set_variant(v)
    try:
        return fn()
    finally:
        rt.set_variant(prev)


# ---- 1. small sets equal today's calls, on both light paths ----
def small_lights(n):
    """ring_lights(n) with three of them turned into directional lights at interleaved positions (their position is
    then the stored vector); n < 4 has no room for three and keeps point lights."""
    lights = [tuple(l) + (0,) for l in E.ring_lights(n)]
    if n >= 4:
        for k in (1, n // 2, n - 2):
            lights[k] = (lights[k][0], lights[k][1], 1)
    return lights


@pytest.mark.parametrize("n", [0, 1, 32])
@pytest.mark.parametrize("name", ["cornell", "material"])
def test_small_sets_equal_the_array_calls_on_both_paths(rt, refs, name, n):
    r = refs[name]
    lights = small_lights(n)
    assert len(lights) == n and sum(l[2] for l in lights) == (3 if n >= 4 else 0)
    ls = r.gpu.light_set(lights)
    assert len(ls) == n
    nans = 0
    for mode in (PRIMARY, FULL):
        for depth in (0, 3):
            what = f"{name} n={n} mode {mode} depth {depth}"
            rgb, face, t, _ = r.gpu.render(r.cam, lights, r.W, r.H, mode=mode, max_depth=depth, want_hits=True)
            want = frame_dict(rgb, face, t)
            nans += int(np.isnan(want["rgb"]).any(1).sum())
            got = frame_dict(*r.gpu.render_lit(r.cam, ls, r.W, r.H, mode=mode, max_depth=depth, want_hits=True)[:3])
            assert_same(got, want, what + ": render_lit")
            mem = with_variant(rt, MEM_LIGHTS, lambda: frame_dict(*r.gpu.render_lit(
                r.cam, ls, r.W, r.H, mode=mode, max_depth=depth, want_hits=True)[:3]))
            assert (np.isnan(mem["rgb"]) == np.isnan(want["rgb"])).all(), what + ": NaN positions"
            assert_same(mem, want, what + ": render_lit, lights from memory")
            mem_nc = with_variant(rt, MEM_LIGHTS | NO_CACHE, lambda: frame_dict(*r.gpu.render_lit(
                r.cam, ls, r.W, r.H, mode=mode, max_depth=depth, want_hits=True)[:3]))
            assert_same(mem_nc, want, what + ": render_lit, lights from memory, no occluder cache")
            res = r.gpu.trace_stream_color(r.o, r.d, lights, mode=mode, max_depth=depth)
            lst = {k: v.cpu().numpy() for k, v in res.items()}
            assert_same(lit_trace(r.gpu, r.o, r.d, ls, mode, depth), lst, what + ": trace_stream_lit")
            for reorder, wavefront in ((False, False), (True, True)):
                got = with_variant(rt, MEM_LIGHTS, lambda: lit_trace(r.gpu, r.o, r.d, ls, mode, depth, reorder, wavefront))
                assert_same(got, lst, what + f": trace_stream_lit from memory, reorder={reorder} wavefront={wavefront}")
            assert_same(lst, want, what + ": list vs frame")
    if name == "material" and n:
        assert nans > 0  # the material scene's NaN-colour pixels are part of the comparison


# ---- 2. beyond 32 lights against the oracle ----
def shadow_census(osc, ocam, W, H, lights):
    """From the oracle alone: closest hits of the camera rays, then shadow() per light and hit pixel. Returns
    (hit pixels, some-but-not-all lights blocked, all blocked, none blocked).
    Checked on the CPU with the real rt_lights_spherical jitter before any GPU run: cornell, 100 lights at
    CORNELL_LIGHT: 635 hits, 555 / 20 / 60 (33 lights: 513 / 20 / 102); the material scene, 100 lights at
    MATERIAL_LIGHT: 350 hits, 137 / 0 / 213, and 50 NaN-colour pixels in the FULL frame."""
    import oracle
    od = [oracle.camera_ray(ocam, i, j) for j in range(H) for i in range(W)]
    o = np.array([x[0] for x in od], np.float32)
    d = np.array([x[1] for x in od], np.float32)
    face, t, P = osc.closest(o, d)
    hit = face >= 0
    Ph = P[hit]
    blocked = np.zeros(len(Ph), np.int64)
    for pos, _ in lights:
        L = -(Ph - np.array(pos, np.float32))
        L = (L / np.linalg.norm(L, axis=1, keepdims=True)).astype(np.float32)
        blocked += osc.shadow(Ph, L)
    n = len(lights)
    return int(hit.sum()), int(((blocked > 0) & (blocked < n)).sum()), int((blocked == n).sum()), int((blocked == 0).sum())


def compare_with_oracle(got, want, what):
    rgb, face, t = want
    assert (got["face"] == face).all(), f"{what}: face"
    assert bits(got["t"]).tobytes() == bits(t).tobytes(), f"{what}: t"
    nan_g, nan_o = np.isnan(got["rgb"]), np.isnan(rgb)
    assert (nan_g == nan_o).all(), f"{what}: NaN positions"
    err = float(np.abs(np.where(nan_o, 0.0, got["rgb"] - rgb)).max())
    print(f"{what}: colour L_inf {err:.3g}, NaN-colour pixels {int(nan_o.any(1).sum())}")
    assert err < TOL, f"{what}: colour L_inf {err}"


def test_the_soft_light_exercises_shadows(rt, refs):
    r = refs["cornell"]
    hits, some, all_, none = shadow_census(r.orc, r.ocam, r.W, r.H, r.soft_set(rt, 99)[0])
    print(f"cornell 100 lights: hits {hits}, penumbra {some}, all blocked {all_}, none blocked {none}")
    assert some >= 100 and all_ >= 5 and none >= 20


@pytest.mark.parametrize("case", ["33", "100", "100+2dir"])
def test_beyond_32_lights_match_the_oracle(rt, refs, case):
    r = refs["cornell"]
    points = r.soft_set(rt, 32 if case == "33" else 99)[0]
    dirs = []
    lights = [tuple(l) + (0,) for l in points]
    if case == "100+2dir":
        dirs = [((0.2, 0.9, 0.4), (0.10, 0.08, 0.06)), ((-0.5, 0.6, 0.7), (0.05, 0.07, 0.09))]
        lights.insert(17, dirs[0] + (1,))  # interleaved among the points; the set puts them after every point
        lights.insert(60, dirs[1] + (1,))
    ls = r.gpu.light_set(lights)
    assert len(ls) == len(points) + len(dirs) > 32
    for mode, depth in ((FULL, 0), (FULL, 3), (PRIMARY, 1)):
        got = frame_dict(*r.gpu.render_lit(r.cam, ls, r.W, r.H, mode=mode, max_depth=depth, want_hits=True)[:3])
        want = r.orc.render(r.ocam, points, r.W, r.H, full=mode == FULL, max_depth=depth if depth else None, dir_lights=dirs)
        compare_with_oracle(got, want, f"cornell {case} mode {mode} depth {depth}")
        assert (got["face"] >= 0).any() and (got["face"] < 0).any()


def test_material_scene_with_100_lights_matches_the_oracle(rt, refs):
    r = refs["material"]
    points, ls = r.soft_set(rt, 99)
    hits, some, all_, none = shadow_census(r.orc, r.ocam, r.W, r.H, points)
    print(f"material 100 lights: hits {hits}, penumbra {some}, all blocked {all_}, none blocked {none}")
    assert some >= 100 and none >= 20  # the cornell frame's rule; its small triangles never block every light
    nans = 0
    for mode, depth in ((FULL, 0), (FULL, 3), (PRIMARY, 1)):
        got = frame_dict(*r.gpu.render_lit(r.cam, ls, r.W, r.H, mode=mode, max_depth=depth, want_hits=True)[:3])
        want = r.orc.render(r.ocam, points, r.W, r.H, full=mode == FULL, max_depth=depth if depth else None)
        compare_with_oracle(got, want, f"material 100 mode {mode} depth {depth}")
        nans += int(np.isnan(want[0]).any(1).sum())
    assert nans > 0


# ---- 3. lists ----
def test_lists_equal_the_frame_in_every_combination(rt, refs):
    r = refs["cornell"]
    ls = r.soft_set(rt, 99)[1]
    frame = r.plain(rt, FULL, 3)
    counts = []
    for name, o, d, want in (("raster", r.o, r.d, frame), ("shuffle", r.o_sh, r.d_sh, {k: v[r.sh] for k, v in frame.items()})):
        for reorder, wavefront in COMBOS:
            got = lit_trace(r.gpu, o, d, ls, FULL, 3, reorder, wavefront, stats=True)
            assert_same(got, want, f"{name}: reorder={reorder} wavefront={wavefront}")
            counts.append(tuple(r.gpu.counters(8)[4:7]))
    assert len(set(counts)) == 1, counts  # RT_RAYS_STATS slots 4 (rays), 5 (primary hits), 6 (all rays)
    assert counts[0][0] == r.W * r.H and counts[0][2] > 100 * counts[0][1] > 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_list_lengths(rt, refs, n):
    r = refs["cornell"]
    ls = r.soft_set(rt, 99)[1]
    frame = r.plain(rt, FULL, 3)
    want = {k: v[r.sh[:n]] for k, v in frame.items()}
    o, d = r.o_sh[:n].contiguous(), r.d_sh[:n].contiguous()
    for reorder, wavefront in COMBOS:
        assert_same(lit_trace(r.gpu, o, d, ls, FULL, 3, reorder, wavefront), want, f"n={n} reorder={reorder} wavefront={wavefront}")


# ---- 4. the other frame paths ----
def test_shards_stitch_to_the_plain_frame(rt, refs):
    r = refs["cornell"]
    ls = r.soft_set(rt, 99)[1]
    want = r.plain(rt, FULL, 0)["rgb"].reshape(r.H, r.W, 3)
    out = np.full((r.H, r.W, 3), np.float32(-7.0))
    for k in range(3):
        rgb, _ = r.gpu.render_lit(r.cam, ls, r.W, r.H, mode=FULL, shard=(k, 3))
        m = rt.shard_mask(r.W, r.H, k, 3)
        out[m] = rgb[m]
    assert bits(out).tobytes() == bits(want).tobytes()


def test_frames_in_flight_and_two_replicas(rt, refs):
    r = refs["cornell"]
    lights, ls = r.soft_set(rt, 99)
    want = r.plain(rt, FULL, 0)
    for _ in range(4):
        r.gpu.render_lit_async(r.cam, ls, r.W, r.H, mode=FULL, flags=rt.RT_FRAME_WRITE_HITS)
    r.gpu.synchronize()
    rgb, face, t = r.gpu.download(r.W, r.H, want_hits=True)
    assert_same(frame_dict(rgb, face, t), want, "render_lit_async x4")
    two = rt.Scene(rt.Mesh.load_obj(scene_path("cornell.obj")), devices=[0, 0])
    assert two.info()["n_devices"] == 2
    ls2 = two.light_set(lights)
    got = frame_dict(*two.render_lit(r.cam, ls2, r.W, r.H, mode=FULL, want_hits=True)[:3])
    assert_same(got, want, "devices=[0, 0]")
    del ls2, two


def test_wave_stats_refused_and_box_colours_ignore_the_set(rt, refs):
    r = refs["cornell"]
    ls = r.soft_set(rt, 99)[1]
    with pytest.raises(rt.RTError, match="error -6"):
        r.gpu.render_lit(r.cam, ls, r.W, r.H, mode=FULL, flags=rt.RT_FRAME_STATS | rt.RT_FRAME_WAVE_STATS)
    box, _ = r.gpu.render_lit(r.cam, ls, r.W, r.H, mode=BOX)
    want, _ = r.gpu.render(r.cam, [], r.W, r.H, mode=BOX)
    assert bits(box).tobytes() == bits(want).tobytes()


# ---- 5. the occluder cache ----
def test_occluder_cache_changes_no_bit_and_saves_node_fetches(rt, refs):
    r = refs["cornell"]
    ls = r.soft_set(rt, 99)[1]
    for depth in (0, 3):
        want = r.plain(rt, FULL, depth)
        off = with_variant(rt, NO_CACHE, lambda: frame_dict(*r.gpu.render_lit(
            r.cam, ls, r.W, r.H, mode=FULL, max_depth=depth, want_hits=True)[:3]))
        assert_same(off, want, f"depth {depth}: cache off vs on")
    st_on = r.gpu.render_lit(r.cam, ls, r.W, r.H, mode=FULL, flags=rt.RT_FRAME_STATS)[1]
    st_off = with_variant(rt, NO_CACHE, lambda: r.gpu.render_lit(r.cam, ls, r.W, r.H, mode=FULL, flags=rt.RT_FRAME_STATS)[1])
    print(f"wave node fetches: cached {st_on['wave_node_fetches']}, uncached {st_off['wave_node_fetches']}; "
          f"wave triangle fetches: cached {st_on['wave_tri_fetches']}, uncached {st_off['wave_tri_fetches']}")
    assert st_on["wave_node_fetches"] < st_off["wave_node_fetches"]
    for k in ("total_rays", "hits", "primary_rays"):
        assert st_on[k] == st_off[k] > 0, k


# ---- 6. the cap of the existing calls stays ----
def test_the_array_calls_keep_their_cap(rt, refs):
    r = refs["cornell"]
    ls = r.gpu.light_set(E.ring_lights(33))
    r.gpu.render_lit(r.cam, ls, r.W, r.H, mode=FULL)
    with pytest.raises(rt.RTError, match="invalid"):
        r.gpu.render(r.cam, E.ring_lights(33), r.W, r.H)
    with pytest.raises(rt.RTError, match="invalid"):
        r.gpu.trace_stream_color(r.o, r.d, E.ring_lights(33))
