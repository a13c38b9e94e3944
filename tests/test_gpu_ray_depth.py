"""rt_trace_stream_color (MI355X): traceRay for device ray lists at any depth and mode, in order, reordered and as
the wavefront path, against the CPU oracle, the frame kernels and each other -- bit for bit wherever two GPU
paths are compared.

Every output buffer holds n + 64 elements filled with a sentinel, as in tests/test_gpu_ray_streams.py."""
import numpy as np
import pytest
import torch

import edge_scenes as E
from conftest import scene_path
from test_gpu_ray_streams import PAD, SENT, aimed_rays, assert_same, bits, collect, dev, stream_trace

pytestmark = pytest.mark.gpu

TOL = 1e-4
PRIMARY, FULL = 0, 1
Q_CLOSEST, Q_COLOR = 0, 2
COMBOS = [(False, False), (True, False), (False, True), (True, True)]  # (reorder, wavefront)


@pytest.fixture(scope="module", autouse=True)
def need_gpu(rt):
    if rt.device_count() == 0:
        pytest.skip("no GPU")


def color_trace(sc, a, b, lights, mode, depth, reorder=False, wavefront=False, stats=False, stream=None, sync=True):
    """rt_trace_stream_color into sentinel-filled buffers of n + PAD elements (checked by collect)."""
    ta = a if torch.is_tensor(a) else dev(np.asarray(a, np.float32).reshape(-1, 3))
    tb = b if torch.is_tensor(b) else dev(np.asarray(b, np.float32).reshape(-1, 3))
    n = ta.shape[0]
    full, out = {}, {}
    for name, w in (("rgb", 3), ("face", 1), ("t", 1)):
        buf = torch.full((n + PAD, 3) if w == 3 else (n + PAD,), int(SENT), dtype=torch.int32, device="cuda")
        if name != "face":
            buf = buf.view(torch.float32)
        full[name] = buf
        out[name] = buf[:n]
    res = sc.trace_stream_color(ta, tb, lights, mode=mode, max_depth=depth, reorder=reorder, wavefront=wavefront,
                                stats=stats, stream=stream, out=out)
    assert set(res) == set(out)
    return collect(full, n) if sync else full


def all_combos_equal(sc, a, b, lights, mode, depth, plain, what):
    for reorder, wavefront in COMBOS[1:]:
        got = color_trace(sc, a, b, lights, mode, depth, reorder=reorder, wavefront=wavefront)
        assert_same(got, plain, f"{what}: reorder={reorder} wavefront={wavefront}")


def check_against_oracle(got, want, what):
    rgb, face, t = want
    assert (got["face"] == face).all(), f"{what}: face"
    assert bits(got["t"]).tobytes() == bits(t).tobytes(), f"{what}: t"
    nan_g, nan_o = np.isnan(got["rgb"]), np.isnan(rgb)
    assert (nan_g == nan_o).all(), f"{what}: NaN positions"
    err = float(np.abs(np.where(nan_o, 0.0, got["rgb"] - rgb)).max())
    print(f"{what}: colour L_inf {err:.3g}")
    assert err < TOL, f"{what}: colour L_inf {err}"


def camera_list_checks(rt, sc, osc, cam, ocam, W, H, lights, mode, depth, rays, what):
    """The assertions of 1. and 2.: the flagless call against the oracle and the frame, every other combination
    against the flagless call on the raster list and on a fixed shuffle of it."""
    o, d, sh, o_sh, d_sh = rays
    plain = color_trace(sc, o, d, lights, mode, depth)
    want = osc.render(ocam, lights, W, H, full=mode == FULL, max_depth=depth if depth else None)
    check_against_oracle(plain, want, what)
    rgb, face, t, _ = sc.render(cam, lights, W, H, mode=mode, max_depth=depth, want_hits=True)
    assert_same(plain, {"rgb": rgb.reshape(-1, 3), "face": face.reshape(-1), "t": t.reshape(-1)}, f"{what}: frame")
    all_combos_equal(sc, o, d, lights, mode, depth, plain, what)
    plain_sh = {k: v[sh] for k, v in plain.items()}
    for reorder, wavefront in COMBOS:
        got = color_trace(sc, o_sh, d_sh, lights, mode, depth, reorder=reorder, wavefront=wavefront)
        assert_same(got, plain_sh, f"{what} shuffled: reorder={reorder} wavefront={wavefront}")
    return plain


def camera_rays(sc, cam, W, H, seed):
    o, d = sc.camera_rays(cam, W, H)
    sh = np.random.default_rng(seed).permutation(W * H)
    tsh = torch.from_numpy(sh).cuda()
    return o, d, sh, o[tsh].contiguous(), d[tsh].contiguous()


# ---- 1. camera lists against the oracle and the frames ----
class CameraRef:
    def __init__(self, rt, orc, name):
        if name == "cornell":
            self.W, self.H = 64, 48
            self.gpu = rt.Scene(rt.Mesh.load_obj(scene_path("cornell.obj")))
            self.orc = orc.Scene(orc.Mesh.load_obj(scene_path("cornell.obj")))
            self.cam, self.ocam = rt.flycam(self.W, self.H), orc.flycam(self.W, self.H)
            self.lights = rt.DEFAULT_LIGHTS
        else:
            v, f, m, g = E.material_scene()
            self.W, self.H = E.MATERIAL_CAMERA[:2]
            self.gpu = rt.Scene(rt.Mesh.from_arrays(v, f, m, groups=g))
            self.orc = orc.Scene(orc.Mesh.from_arrays(v, f, m, groups=g))
            self.cam, self.ocam = rt.flycam(*E.MATERIAL_CAMERA), orc.flycam(*E.MATERIAL_CAMERA)
            self.lights = E.ring_lights(4)
        self.rays = camera_rays(self.gpu, self.cam, self.W, self.H, 41)


@pytest.fixture(scope="module")
def camrefs(rt, orc):
    return {name: CameraRef(rt, orc, name) for name in ("cornell", "material")}


@pytest.mark.parametrize("depth", [0, 1, 2, 3, 6])
@pytest.mark.parametrize("mode", [PRIMARY, FULL])
@pytest.mark.parametrize("name", ["cornell", "material"])
def test_camera_lists_match_oracle_and_frames(rt, camrefs, name, mode, depth):
    r = camrefs[name]
    plain = camera_list_checks(rt, r.gpu, r.orc, r.cam, r.ocam, r.W, r.H, r.lights, mode, depth, r.rays,
                               f"{name} mode {mode} depth {depth}")
    assert (plain["face"] >= 0).any() and (plain["face"] < 0).any()


# ---- 2. sticky material ----
@pytest.fixture(scope="module")
def sticky(rt, orc):
    """cornell with the material of every even face removed, one group per face, in the library and the oracle"""
    ex = rt.Mesh.load_obj(scene_path("cornell.obj")).export()
    v, f, fmat, mats = ex["v4"][:, :3].copy(), ex["fidx"], ex["fmat"], ex["mats"]
    groups = [(1, -1 if i % 2 == 0 else int(fmat[i])) for i in range(len(f))]
    assert any(g[1] >= 0 for g in groups)

    class R:
        pass
    r = R()
    r.W, r.H = 64, 48
    r.gpu = rt.Scene(rt.Mesh.from_arrays(v, f, mats, groups=groups))
    r.orc = orc.Scene(orc.Mesh.from_arrays(v, f, mats, groups=groups))
    r.cam, r.ocam = rt.flycam(r.W, r.H), orc.flycam(r.W, r.H)
    r.lights = rt.DEFAULT_LIGHTS
    r.rays = camera_rays(r.gpu, r.cam, r.W, r.H, 43)
    r.has_mat = np.array([g[1] >= 0 for g in groups])
    return r


def test_sticky_precondition_chains_cross_between_material_and_none(rt, sticky):
    """Selection only: level-1 rays from a CLOSEST query's P and N by a numpy reflection; enough chains go from a
    face with a material to one without, and the other way."""
    o, d = sticky.rays[:2]
    c0 = stream_trace(rt, sticky.gpu, Q_CLOSEST, o, d)
    hit = c0["face"] >= 0
    dn = d.cpu().numpy().astype(np.float64)
    dn /= np.linalg.norm(dn, axis=1, keepdims=True)
    N = c0["N"].astype(np.float64)
    r1 = dn - 2.0 * (dn * N).sum(1, keepdims=True) * N
    o1 = c0["P"].astype(np.float64) + 0.001 * r1
    idx = np.flatnonzero(hit & (np.linalg.norm(r1, axis=1) > 0))
    c1 = stream_trace(rt, sticky.gpu, Q_CLOSEST, o1[idx].astype(np.float32), r1[idx].astype(np.float32))
    both = c1["face"] >= 0
    m0, m1 = sticky.has_mat[c0["face"][idx][both]], sticky.has_mat[c1["face"][both]]
    to_none, to_mat = int((m0 & ~m1).sum()), int((~m0 & m1).sum())
    print(f"chains material -> none {to_none}, none -> material {to_mat}")
    assert to_none >= 32 and to_mat >= 32


@pytest.mark.parametrize("depth", [2, 3, 4])
@pytest.mark.parametrize("mode", [PRIMARY, FULL])
def test_sticky_material_follows_the_chain(rt, sticky, mode, depth):
    r = sticky
    camera_list_checks(rt, r.gpu, r.orc, r.cam, r.ocam, r.W, r.H, r.lights, mode, depth, r.rays,
                       f"sticky mode {mode} depth {depth}")


# ---- 3. packet boundaries ----
@pytest.fixture(scope="module")
def scenes(rt):
    return {name: rt.Scene(rt.Mesh.load_obj(scene_path(name + ".obj"))) for name in ("cornell", "bunny")}


def away_rays(n, seed):
    """Rays that start above the scene and point away from it: every one misses."""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(3.0, 4.0, n)], 1).astype(np.float32)
    d = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), np.ones(n)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4096])
def test_packet_boundaries(rt, scenes, n):
    sc = scenes["cornell"]
    o, d = aimed_rays(n)
    plain = color_trace(sc, o, d, rt.DEFAULT_LIGHTS, FULL, 3)
    all_combos_equal(sc, o, d, rt.DEFAULT_LIGHTS, FULL, 3, plain, f"n={n}")


def test_a_list_of_misses_gives_the_background(rt, scenes):
    sc = scenes["cornell"]
    o, d = away_rays(300, 5)
    W, H = 64, 48
    rgb, face, _, _ = sc.render(rt.flycam(W, H), rt.DEFAULT_LIGHTS, W, H, mode=FULL, max_depth=3, want_hits=True)
    bg = rgb.reshape(-1, 3)[np.flatnonzero(face.reshape(-1) < 0)[0]]
    for reorder, wavefront in COMBOS:
        got = color_trace(sc, o, d, rt.DEFAULT_LIGHTS, FULL, 3, reorder=reorder, wavefront=wavefront)
        assert (got["face"] == -1).all() and np.isposinf(got["t"]).all()
        assert (bits(got["rgb"]) == bits(bg)[None, :]).all()
        if wavefront:
            assert sc.ray_levels().tolist() == [[300, 0], [0, 0], [0, 0]]


@pytest.mark.parametrize("k", [0, 1, 64, 65])
def test_lists_with_exactly_k_hits(rt, scenes, k):
    sc = scenes["cornell"]
    n = 4096
    ao, ad = aimed_rays(n, seed=19)
    hitters = np.flatnonzero(stream_trace(rt, sc, Q_CLOSEST, ao, ad)["face"] >= 0)
    assert len(hitters) >= 65
    o, d = away_rays(n, 6)
    where = np.sort(np.random.default_rng(8).choice(n, k, replace=False))
    o[where], d[where] = ao[hitters[:k]], ad[hitters[:k]]
    plain = color_trace(sc, o, d, rt.DEFAULT_LIGHTS, FULL, 3)
    assert int((plain["face"] >= 0).sum()) == k
    for reorder, wavefront in COMBOS[1:]:
        got = color_trace(sc, o, d, rt.DEFAULT_LIGHTS, FULL, 3, reorder=reorder, wavefront=wavefront)
        assert_same(got, plain, f"k={k}: reorder={reorder} wavefront={wavefront}")
        if wavefront:
            lv = sc.ray_levels()
            assert lv.shape == (3, 2) and lv[0].tolist() == [n, k] and lv[1, 0] == k


# ---- 4. edge lists ----
@pytest.fixture(scope="module")
def tie_gpu(rt):
    (v, f, m, g), _ = E.tie_scene()
    return rt.Scene(rt.Mesh.from_arrays(v, f, m, groups=g), min_faces=8)


@pytest.mark.parametrize("name", ["random", "on-plane", "zero-d"])
def test_edge_lists_pass_through_keys_compaction_and_state(rt, tie_gpu, name):
    a, b = {"random": E.tie_random_rays, "on-plane": lambda: E.on_plane_rays()[:2], "zero-d": E.zero_direction_rays}[name]()
    plain = color_trace(tie_gpu, a, b, rt.DEFAULT_LIGHTS, FULL, 3)
    all_combos_equal(tie_gpu, a, b, rt.DEFAULT_LIGHTS, FULL, 3, plain, name)


# ---- 5. the existing query ----
def test_full_depth_two_is_the_existing_colour_query(rt, scenes):
    sc = scenes["bunny"]
    o, d = aimed_rays(4096)
    want = stream_trace(rt, sc, Q_COLOR, o, d, lights=rt.DEFAULT_LIGHTS)
    assert (want["face"] >= 0).any()
    for depth in (0, 2):
        for reorder, wavefront in COMBOS:
            got = color_trace(sc, o, d, rt.DEFAULT_LIGHTS, FULL, depth, reorder=reorder, wavefront=wavefront)
            assert_same(got, want, f"depth {depth}: reorder={reorder} wavefront={wavefront}")


# ---- 6. levels and counters ----
def test_levels_and_counters(rt, scenes):
    sc = scenes["cornell"]
    W, H, D = 64, 48, 4
    lights = rt.DEFAULT_LIGHTS
    _, _, _, o, d = camera_rays(sc, rt.flycam(W, H), W, H, 17)
    n = W * H
    plain = color_trace(sc, o, d, lights, FULL, D)
    color_trace(sc, o, d, lights, FULL, D, reorder=True)
    order_plain = sc.ray_order()
    in_order = color_trace(sc, o, d, lights, FULL, D, stats=True)
    c_in = sc.counters(8)
    assert_same(in_order, plain, "in-order counting call")
    counted = color_trace(sc, o, d, lights, FULL, D, reorder=True, wavefront=True, stats=True)
    c_wf = sc.counters(8)
    lv = sc.ray_levels()
    assert_same(counted, plain, "wavefront counting call")
    live, hits = lv[:, 0], lv[:, 1]
    print("levels", lv.tolist(), "counters in-order", c_in, "wavefront", c_wf)
    assert lv.shape == (D, 2) and live[0] == n and hits[0] == int((plain["face"] >= 0).sum()) > 0
    assert (live[1:] == hits[:-1]).all()
    assert c_wf[4] == c_in[4] == n and c_wf[5] == c_in[5] == hits[0]
    assert c_wf[6] == c_in[6] == n + int(hits[:-1].sum()) + len(lights) * int(hits.sum())
    assert (sc.ray_order() == order_plain).all() and len(order_plain) == n
    color_trace(sc, o, d, lights, FULL, D, reorder=True, wavefront=True, stats=True)
    assert sc.counters(8)[:7] == c_wf[:7] and (sc.ray_levels() == lv).all()
    # a wavefront call without the reorder leaves the order's record alone
    color_trace(sc, o[:500].contiguous(), d[:500].contiguous(), lights, FULL, D, wavefront=True)
    assert len(sc.ray_order()) == n


# ---- 7. stream order ----
def test_stream_order_growth_and_cross_stream(rt, scenes):
    sc = scenes["cornell"]
    lights = rt.DEFAULT_LIGHTS
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    base_o, base_d = aimed_rays(70000, seed=13)
    tb_o, tb_d = dev(base_o), dev(base_d)
    torch.cuda.synchronize()
    pending = []
    for stream, n in ((s1, 300), (s1, 70000), (s1, 300), (s2, 5000)):
        with torch.cuda.stream(stream):
            o = (tb_o[:n] * 1.0).contiguous()
            d = torch.nn.functional.normalize(tb_d[:n] + 0.0, dim=1)
            full = color_trace(sc, o, d, lights, FULL, 3, reorder=True, wavefront=True, stream=stream.cuda_stream, sync=False)
            hit_sum = (full["face"][:n] >= 0).sum()
        pending.append((n, o, d, full, hit_sum))
    torch.cuda.synchronize()
    for n, o, d, full, hit_sum in pending:
        got = collect(full, n)
        want = color_trace(sc, o, d, lights, FULL, 3)
        assert_same(got, want, f"n={n}")
        assert int(hit_sum) == int((want["face"] >= 0).sum())
    empty = torch.empty((0, 3), dtype=torch.float32, device="cuda")
    for flags in range(8):
        res = sc.trace_stream_color(empty, empty, lights, mode=FULL, max_depth=3, reorder=bool(flags & 1),
                                    stats=bool(flags & 2), wavefront=bool(flags & 4))
        assert all(v.shape[0] == 0 for v in res.values())


# ---- 8. replicated scene ----
def test_replicated_scene_traces_on_its_first_device(rt, scenes):
    rep = rt.Scene(rt.Mesh.load_obj(scene_path("cornell.obj")), devices=[0, 0])
    o, d = aimed_rays(257, seed=3)
    for mode, depth in ((FULL, 3), (PRIMARY, 2)):
        want = color_trace(scenes["cornell"], o, d, rt.DEFAULT_LIGHTS, mode, depth)
        for reorder, wavefront in COMBOS:
            got = color_trace(rep, o, d, rt.DEFAULT_LIGHTS, mode, depth, reorder=reorder, wavefront=wavefront)
            assert_same(got, want, f"mode {mode}: reorder={reorder} wavefront={wavefront}")
