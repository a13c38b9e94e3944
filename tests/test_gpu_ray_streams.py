"""Ray streams (MI355X): rt_trace_stream / rt_rays_camera on torch tensors against the host-pointer API, the
frame kernels and the CPU oracle, bit for bit; the coherence reorder against the in-order trace on the inputs
where the grouping of rays into waves could matter (tests/edge_scenes.py).

Every output buffer holds n + 64 elements filled with a sentinel: after each call the 64 past the end are
untouched and no sentinel is left in [0, n)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import edge_scenes as E
from conftest import ROOT, scene_path
from test_oracle_pinning import same_bits

pytestmark = pytest.mark.gpu

SENT = np.int32(-559038737)  # 0xDEADBEEF: as a float -6.26e18, a value no query writes
PAD = 64
Q_CLOSEST, Q_SHADOW, Q_COLOR = 0, 1, 2
OUTPUTS = {Q_CLOSEST: (("face", 1), ("t", 1), ("P", 3), ("N", 3)), Q_SHADOW: (("blocked", 1),),
           Q_COLOR: (("rgb", 3), ("face", 1), ("t", 1))}
INT_OUTPUTS = ("face", "blocked")


@pytest.fixture(scope="module", autouse=True)
def need_gpu(rt):
    if rt.device_count() == 0:
        pytest.skip("no GPU")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def stream_trace(rt, sc, query, a, b, lights=None, reorder=False, stats=False, stream=None, sync=True):
    """rt_trace_stream into sentinel-filled buffers of n + PAD elements; checks the padding and that every element
    below n was written; returns {name: numpy array of the n results}. a, b: numpy arrays or device tensors."""
    ta = a if torch.is_tensor(a) else dev(np.asarray(a, np.float32).reshape(-1, 3))
    tb = b if torch.is_tensor(b) else dev(np.asarray(b, np.float32).reshape(-1, 3))
    n = ta.shape[0]
    full, out = {}, {}
    for name, w in OUTPUTS[query]:
        shape = (n + PAD, 3) if w == 3 else (n + PAD,)
        buf = torch.full(shape, int(SENT), dtype=torch.int32, device="cuda")
        if name not in INT_OUTPUTS:
            buf = buf.view(torch.float32)
        full[name] = buf
        out[name] = buf[:n]
    res = sc.trace_stream(query, ta, tb, lights=lights, reorder=reorder, stats=stats, stream=stream, out=out)
    assert set(res) == set(out)
    if not sync:
        return full
    return collect(full, n)


def collect(full, n):
    got = {}
    for name, buf in full.items():
        h = buf.cpu().numpy()
        assert (bits(h[n:]) == SENT).all(), f"{name}: written past n"
        assert not (bits(h[:n]) == SENT).any(), f"{name}: not written below n"
        got[name] = h[:n]
    return got


def host_trace(rt, sc, query, a, b, lights=None):
    if query == Q_CLOSEST:
        return dict(zip(("face", "t", "P", "N"), sc.trace_closest_normal(a, b)))
    if query == Q_SHADOW:
        return {"blocked": sc.trace_shadow(a, b)}
    return dict(zip(("rgb", "face", "t"), sc.trace_color(a, b, lights)))


def assert_same(got, want, what):
    assert set(got) == set(want), what
    for name in want:
        assert bits(got[name]).tobytes() == bits(want[name]).tobytes(), f"{what}: {name} differs"


def aimed_rays(n, seed=7):
    """Rays as tests/test_gpu_parity.py::test_trace_queries_match_oracle draws them."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    tgt = rng.uniform(-0.3, 0.3, (n, 3)).astype(np.float32)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)


@pytest.fixture(scope="module")
def scenes(rt):
    return {name: rt.Scene(rt.Mesh.load_obj(scene_path(name + ".obj"))) for name in ("cube", "cornell", "bunny")}


CASES = [(s, n) for s in ("cube", "cornell") for n in (1, 63, 64, 65, 257, 4096)] + [("bunny", 4096)]


@pytest.mark.parametrize("name,n", CASES)
def test_stream_equals_host_api(rt, scenes, name, n):
    """1. All three queries, in order and reordered, equal the host-pointer API bit for bit."""
    sc = scenes[name]
    o, d = aimed_rays(n)
    for query in (Q_CLOSEST, Q_SHADOW, Q_COLOR):
        lights = rt.DEFAULT_LIGHTS if query == Q_COLOR else None
        want = host_trace(rt, sc, query, o, d, lights)
        for reorder in (False, True):
            got = stream_trace(rt, sc, query, o, d, lights=lights, reorder=reorder)
            assert_same(got, want, f"{name} n={n} query={query} reorder={reorder}")


def test_empty_list_launches_nothing(rt, scenes):
    """n = 0 returns RT_OK for every query and flag and leaves the last reorder record alone."""
    sc = scenes["cube"]
    o, d = aimed_rays(100)
    stream_trace(rt, sc, Q_CLOSEST, o, d, reorder=True)
    before = sc.ray_order()
    empty = torch.empty((0, 3), dtype=torch.float32, device="cuda")
    for query in (Q_CLOSEST, Q_SHADOW, Q_COLOR):
        for reorder in (False, True):
            res = sc.trace_stream(query, empty, empty, lights=rt.DEFAULT_LIGHTS if query == Q_COLOR else None,
                                  reorder=reorder, stats=reorder)
            assert all(v.shape[0] == 0 for v in res.values())
    assert (sc.ray_order() == before).all() and len(before) == 100


# ---- 2. reorder on the inputs where grouping could matter ----
class TieRef:
    """The tie scene on the device and in the oracle, the edge ray lists, and the oracle's answers (computed once,
    read-only afterwards)."""

    def __init__(self, rt, orc):
        (v, f, m, g), _ = E.tie_scene()
        self.gpu = rt.Scene(rt.Mesh.from_arrays(v, f, m, groups=g), min_faces=8)
        self.orc = orc.Scene(orc.Mesh.from_arrays(v, f, m, groups=g), min_faces=8)
        ident_o = np.tile(np.array([[0.11, -0.07, 1.0]], np.float32), (130, 1))
        ident_d = np.tile(np.array([[0.0, 0.0, -1.0]], np.float32), (130, 1))
        self.lists = {"lattice": E.tie_lattice_rays()[:2], "random": E.tie_random_rays(), "on-plane": E.on_plane_rays()[:2],
                      "straddle": E.shadow_straddle_rays(), "zero-d": E.zero_direction_rays(), "identical": (ident_o, ident_d)}
        o, d = (x.copy() for x in E.tie_random_rays(700, seed=31))
        rng = np.random.default_rng(32)
        for k, i in enumerate(rng.choice(700, 90, replace=False)):
            arr = o if k % 2 else d
            arr[i, k % 3] = (np.nan, np.inf, -np.inf)[(k // 6) % 3]
        self.nonfinite = (o, d)
        self._oracle = {}

    def oracle(self, query, name):
        key = (query, name)
        if key not in self._oracle:
            a, b = self.lists[name]
            if query == Q_CLOSEST:
                out = dict(zip(("face", "t", "P"), self.orc.closest(a, b)))
            else:
                out = {"blocked": self.orc.shadow(a, b)}
            for x in out.values():
                x.setflags(write=False)
            self._oracle[key] = out
        return self._oracle[key]


@pytest.fixture(scope="module")
def tie(rt, orc):
    return TieRef(rt, orc)


EDGE_CASES = [(Q_CLOSEST, "lattice"), (Q_CLOSEST, "random"), (Q_CLOSEST, "on-plane"), (Q_CLOSEST, "zero-d"),
              (Q_CLOSEST, "identical"), (Q_SHADOW, "lattice"), (Q_SHADOW, "on-plane"), (Q_SHADOW, "straddle"),
              (Q_SHADOW, "zero-d"), (Q_SHADOW, "identical"), (Q_CLOSEST, "nonfinite"), (Q_SHADOW, "nonfinite"),
              (Q_COLOR, "random"), (Q_COLOR, "nonfinite")]


@pytest.mark.parametrize("query,name", EDGE_CASES)
def test_reorder_cannot_change_a_bit(rt, tie, query, name):
    """2. Reordered, in order, and in order after a fixed shuffle: the same bits per ray; the finite lists also
    equal the oracle's closest / shadow."""
    a, b = tie.nonfinite if name == "nonfinite" else tie.lists[name]
    n = len(a)
    lights = rt.DEFAULT_LIGHTS if query == Q_COLOR else None
    plain = stream_trace(rt, tie.gpu, query, a, b, lights=lights)
    reordered = stream_trace(rt, tie.gpu, query, a, b, lights=lights, reorder=True)
    assert_same(reordered, plain, f"{name}: reordered vs in order")
    if n > 64:
        order = tie.gpu.ray_order()
        assert sorted(order.tolist()) == list(range(n))
        if name not in ("identical", "zero-d"):
            assert (order != np.arange(n)).any(), "the reorder left the list as it was"
    sh = np.random.default_rng(99).permutation(n)
    shuffled = stream_trace(rt, tie.gpu, query, a[sh], b[sh], lights=lights)
    undone = {k: np.empty_like(v) for k, v in shuffled.items()}
    for k, v in shuffled.items():
        undone[k][sh] = v
    assert_same(undone, plain, f"{name}: shuffled vs in order")
    if name != "nonfinite" and query != Q_COLOR:
        want = tie.oracle(query, name)
        for k, v in want.items():
            assert bits(plain[k]).tobytes() == bits(v).tobytes(), f"{name}: {k} differs from the oracle"
    if name == "nonfinite":  # the degenerate rays were traced last
        keys = rt.ray_keys(query, a, b, tie.gpu.ray_bounds())
        nbad = int((keys >> 31).sum())
        assert nbad == 90 and (keys[tie.gpu.ray_order()[-nbad:]] >> 31).all()


@pytest.mark.parametrize("n", [65, 3072])
def test_permutation_is_the_stable_argsort_of_the_host_keys(rt, scenes, n):
    """3. rt_debug_ray_order after a reordered call: a bijection, equal to argsort(host keys, stable)."""
    sc = scenes["cornell"]
    o, d = aimed_rays(n, seed=11)
    o[5], d[5] = o[9], d[9]  # two equal keys: index order decides
    stream_trace(rt, sc, Q_CLOSEST, o, d, reorder=True)
    order = sc.ray_order()
    assert order.dtype == np.uint32 and sorted(order.tolist()) == list(range(n))
    keys = rt.ray_keys(Q_CLOSEST, o, d, sc.ray_bounds())
    assert (order == np.argsort(keys, kind="stable")).all()
    # ... under the other key layout too (A/B variant bit)
    prev = rt.set_variant(4194304)
    try:
        stream_trace(rt, sc, Q_SHADOW, o, d, reorder=True)
        order2 = sc.ray_order()
        keys2 = rt.ray_keys(Q_SHADOW, o, d, sc.ray_bounds())
    finally:
        rt.set_variant(prev)
    assert (order2 == np.argsort(keys2, kind="stable")).all() and (keys2 != keys).any()


# ---- 4. camera rays ----
@pytest.mark.parametrize("WH", [(64, 48), (37, 11)])
@pytest.mark.parametrize("dz", [0.0, 20.0])
def test_camera_rays_match_frames_and_oracle(rt, orc, scenes, WH, dz):
    W, H = WH
    sc = scenes["cornell"]
    cam = rt.flycam(W, H, 0.0, 0.0, dz)
    full_o = torch.full((W * H + PAD, 3), int(SENT), dtype=torch.int32, device="cuda").view(torch.float32)
    full_d = torch.full((W * H + PAD, 3), int(SENT), dtype=torch.int32, device="cuda").view(torch.float32)
    o, d = sc.camera_rays(cam, W, H, out=(full_o[:W * H], full_d[:W * H]))
    rays = collect({"origins": full_o, "dirs": full_d}, W * H)
    # the frame kernels' rays: a PRIMARY frame's hits and a FULL frame's colours
    rgb_p, face, t, _ = sc.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=rt.RT_MODE_PRIMARY, want_hits=True)
    got = stream_trace(rt, sc, Q_CLOSEST, o, d)
    assert (got["face"] == face.reshape(-1)).all() and same_bits(got["t"], t.reshape(-1)).all()
    assert (face >= 0).any()
    rgb_f, _ = sc.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=rt.RT_MODE_FULL)
    col = stream_trace(rt, sc, Q_COLOR, o, d, lights=rt.DEFAULT_LIGHTS, reorder=True)
    assert bits(col["rgb"]).tobytes() == bits(rgb_f.reshape(-1, 3)).tobytes()
    assert (col["face"] == face.reshape(-1)).all()
    # the oracle's camera ray at the corners, the centre and 32 random pixels
    ocam = orc.flycam(W, H, 0.0, 0.0, dz)
    rng = np.random.default_rng(5)
    pix = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2)] + \
        [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(32)]
    for px, py in pix:
        oo, od = orc.camera_ray(ocam, px, py)
        i = py * W + px
        assert same_bits(rays["origins"][i], oo).all() and same_bits(rays["dirs"][i], od).all(), (px, py)


# ---- 5. counting ----
def tile_order(W, H):
    """pixel indices in 8x8-block order (the frame kernels' packets)"""
    idx = np.arange(W * H).reshape(H, W)
    return np.concatenate([idx[y:y + 8, x:x + 8].reshape(-1) for y in range(0, H, 8) for x in range(0, W, 8)])


def test_reorder_lowers_the_wave_node_fetches(rt, scenes):
    """5. 64x48 cornell camera rays under a fixed shuffle: the reordered trace fetches strictly fewer node records
    per wave than the in-order one.

    ST_NODE / ST_TRI (per-ray counts) are not compared: in the binary packet loop (rt_traverse.h traverse) a ray's
    box test is cut off at its current closest hit (tcut = h.t) and the near child is chosen by the wave's
    majority vote, so which nodes a ray still wants depends on the rays sharing its wave. Rays and hits do not."""
    W, H = 64, 48
    sc = scenes["cornell"]
    o, d = sc.camera_rays(rt.flycam(W, H), W, H)
    sh = torch.from_numpy(np.random.default_rng(17).permutation(W * H)).cuda()
    os_, ds = o[sh].contiguous(), d[sh].contiguous()
    counts = {}
    hits = {}
    for label, (a, b, reorder) in {"shuffled": (os_, ds, False), "reordered": (os_, ds, True),
                                   "tiles": (o[torch.from_numpy(tile_order(W, H)).cuda()].contiguous(),
                                             d[torch.from_numpy(tile_order(W, H)).cuda()].contiguous(), False)}.items():
        got = stream_trace(rt, sc, Q_CLOSEST, a, b, reorder=reorder, stats=True)
        counts[label] = sc.counters(8)
        hits[label] = int((got["face"] >= 0).sum())
    print("ST_WNODE shuffled %d, reordered %d, tile order %d (3072 rays, 48 waves)" %
          (counts["shuffled"][2], counts["reordered"][2], counts["tiles"][2]))
    assert counts["reordered"][2] < counts["shuffled"][2]
    for label in counts:
        assert counts[label][4] == W * H and counts[label][5] == hits[label] == hits["shuffled"], label
        assert counts[label][0] > 0 and counts[label][1] > 0 and counts[label][3] > 0
    # the counting kernels give the plain kernels' results
    plain = stream_trace(rt, sc, Q_CLOSEST, os_, ds)
    counted = stream_trace(rt, sc, Q_CLOSEST, os_, ds, stats=True)
    assert_same(counted, plain, "stats vs plain")
    for query in (Q_SHADOW, Q_COLOR):
        lights = rt.DEFAULT_LIGHTS if query == Q_COLOR else None
        assert_same(stream_trace(rt, sc, query, os_, ds, lights=lights, stats=True, reorder=True),
                    stream_trace(rt, sc, query, os_, ds, lights=lights), f"stats query {query}")
        assert sc.counters(8)[4] == W * H


# ---- 6. stream order ----
def test_stream_order_growth_and_cross_stream(rt, scenes):
    """Rays built by torch ops on a side stream, traced on it without a host wait, consumed by a torch op on it;
    one synchronize at the end. n = 300, 70,000, 300 (scratch growth and reuse), then once on a second stream."""
    sc = scenes["cornell"]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    base_o, base_d = aimed_rays(70000, seed=13)
    tb_o, tb_d = dev(base_o), dev(base_d)
    torch.cuda.synchronize()
    pending = []
    for stream, n in ((s1, 300), (s1, 70000), (s1, 300), (s2, 5000)):
        with torch.cuda.stream(stream):
            o = (tb_o[:n] * 1.0).contiguous()  # torch work on this stream feeds the trace
            d = torch.nn.functional.normalize(tb_d[:n] + 0.0, dim=1)
            full = stream_trace(rt, sc, Q_CLOSEST, o, d, reorder=True, stream=stream.cuda_stream, sync=False)
            hit_sum = (full["face"][:n] >= 0).sum()  # consumed on the same stream
        pending.append((n, o, d, full, hit_sum))
    torch.cuda.synchronize()
    for n, o, d, full, hit_sum in pending:
        got = collect(full, n)
        want = stream_trace(rt, sc, Q_CLOSEST, o, d)  # synchronous, in order
        assert_same(got, want, f"n={n}")
        assert int(hit_sum) == int((want["face"] >= 0).sum())


# ---- 7. replicated scene ----
def test_replicated_scene_traces_on_its_first_device(rt, scenes):
    mesh = rt.Mesh.load_obj(scene_path("cornell.obj"))
    rep = rt.Scene(mesh, devices=[0, 0])
    o, d = aimed_rays(257, seed=3)
    for query in (Q_CLOSEST, Q_SHADOW, Q_COLOR):
        lights = rt.DEFAULT_LIGHTS if query == Q_COLOR else None
        for reorder in (False, True):
            assert_same(stream_trace(rt, rep, query, o, d, lights=lights, reorder=reorder),
                        stream_trace(rt, scenes["cornell"], query, o, d, lights=lights), f"query {query}")


# ---- 8. variants library ----
def test_wide4_variant_reads_the_permutation(rt):
    """tests/ray_streams_variant_check.py in a child process with the variants library (one library per process):
    variant 2 (the quantised 4-wide tree's packets) with reorder gives the default kernels' bits on n = 257."""
    lib = os.path.join(ROOT, "ray-tracing-project_amd", "lib", "librtamd_variants.so")
    if not os.path.exists(lib):
        pytest.skip("variants library not built (make variants)")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ray_streams_variant_check.py")],
                       env=dict(os.environ, RTAMD_LIB=lib), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res == {"differing": [], "reordered": True}, res
