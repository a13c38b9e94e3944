"""View batches on the GPU (MI355X): rt_render_views / rt_render_views_lit against rt_render / rt_render_lit bit for
bit (colour, face and t of every view), one batch against the CPU oracle, the optional outputs, stream order, the
refusals and the empty batch.

Frames are tiny: cornell at 40x24 (3x2 tiles; both edges cut a tile and a quarter) and at 16x16 (one tile), the
material scene of tests/edge_scenes.py at its own 64x40. The cameras of a batch all differ -- flycam poses at
different dx / dy / dz and one rotated look-at pose -- so a view written at the wrong index or rendered with a
neighbour's camera shows. Every output lies in a sentinel-filled buffer of n * H * W (* 3) + PAD elements: after each
call the PAD elements past the end are untouched and no sentinel is left below."""
import ctypes as C

import numpy as np
import pytest
import torch

import edge_scenes as E
from conftest import scene_path
from test_gpu_far import look_at
from test_gpu_ray_streams import PAD, SENT, bits

pytestmark = pytest.mark.gpu

TOL = 1e-4  # the suite's colour tolerance against the oracle (tests/test_gpu_light_sets.py, test_gpu_ray_depth.py)
PRIMARY, FULL, BOX = 0, 1, 2
MEM_LIGHTS, NO_CACHE = 8388608, 16777216
RT_OK, RT_ERR_INVALID, RT_ERR_UNSUPPORTED = 0, -1, -6
WIDTH = {"rgb": 3, "face": 1, "t": 1}
# (dx, dy, dz) of the flycam poses, added to the scene's base pose; the ninth camera is the look-at pose
OFFSETS = [(0, 0, 0), (2, 0, 0), (-2, 1, 0), (0, -2, 1), (1, 2, -3), (-1, -1, 2), (3, 0, -1), (0, 3, 3)]
EYE, FOVY = (0.55, 0.4, 1.7), 50.0
POINT = ((-0.5, 2.0, 3.0), (0.8, 0.7, 0.6))
DIRECTIONAL = ((0.3, 0.5, 0.8), (0.3, 0.35, 0.4))
LIGHTS = [POINT + (0,), DIRECTIONAL + (1,)]  # one point light and one directional light, through the array call


@pytest.fixture(scope="module", autouse=True)
def need_gpu(rt):
    if rt.device_count() == 0:
        pytest.skip("no GPU")


class Ref:
    """A scene, its nine cameras and rt_render's frames of them, each rendered once and never changed."""

    def __init__(self, rt, name, W=None, H=None):
        self.rt, self.name = rt, name
        if name == "cornell":
            self.W, self.H, base = W or 40, H or 24, (0.0, 0.0, 0.0)
            self.gpu = rt.Scene(rt.Mesh.load_obj(scene_path("cornell.obj")))
        else:
            self.W, self.H, base = E.MATERIAL_CAMERA[0], E.MATERIAL_CAMERA[1], E.MATERIAL_CAMERA[2:]
            v, f, m, g = E.material_scene()
            self.gpu = rt.Scene(rt.Mesh.from_arrays(v, f, m, groups=g))
        self.poses = [tuple(b + o for b, o in zip(base, off)) for off in OFFSETS]
        self.cams = [rt.flycam(self.W, self.H, *p) for p in self.poses]
        self.cams.append(look_at(rt, self.W, self.H, EYE, (0, 0, 0), (0, 1, 0), FOVY))
        self._frames = {}

    def frame(self, v, lights, mode, depth, key="array"):
        """rt_render (a light list) or rt_render_lit (a LightSet) of camera v with RT_FRAME_WRITE_HITS"""
        k = (v, key, mode, depth)
        if k not in self._frames:
            call = self.gpu.render_lit if isinstance(lights, self.rt.LightSet) else self.gpu.render
            rgb, face, t, _ = call(self.cams[v], lights, self.W, self.H, mode=mode, max_depth=depth, want_hits=True)
            self._frames[k] = {"rgb": rgb, "face": face, "t": t}
        return self._frames[k]

    def frames(self, views, lights, mode, depth, key="array"):
        fs = [self.frame(v, lights, mode, depth, key) for v in views]
        return {name: np.stack([f[name] for f in fs]) for name in WIDTH}


@pytest.fixture(scope="module")
def refs(rt):
    return {name: Ref(rt, name) for name in ("cornell", "material")}


def sentinel_buffers(n, H, W, names):
    """{name: flat sentinel-filled tensor of n H W (3) + PAD elements}, {name: its [n, H, W(, 3)] head}"""
    full, out = {}, {}
    for name in names:
        size = n * H * W * WIDTH[name]
        buf = torch.full((size + PAD,), int(SENT), dtype=torch.int32, device="cuda")
        if name != "face":
            buf = buf.view(torch.float32)
        full[name] = buf
        out[name] = buf[:size].view((n, H, W, 3) if name == "rgb" else (n, H, W))
    return full, out


def collect(full, out):
    """after a synchronise: pad untouched, everything below written; {name: numpy [n, H, W(, 3)]}"""
    got = {}
    for name, buf in full.items():
        h = buf.cpu().numpy()
        size = out[name].numel()
        assert (bits(h[size:]) == SENT).all(), f"{name}: written past n * H * W"
        assert not (bits(h[:size]) == SENT).any(), f"{name}: not written below n * H * W"
        got[name] = h[:size].reshape(tuple(out[name].shape))
    return got


def untouched(full):
    return all((bits(buf.cpu().numpy()) == SENT).all() for buf in full.values())


def batch(r, views, lights, mode, depth, names=("rgb", "face", "t"), stream=None, sync=True):
    """rt_render_views of r's cameras `views` into sentinel buffers; stream: a torch stream (the buffers are filled on
    it) or None (the scene's own stream, synchronous)."""
    cams = [r.cams[v] for v in views]
    if stream is None:
        full, out = sentinel_buffers(len(cams), r.H, r.W, names)
        torch.cuda.synchronize()  # the fills ran on torch's stream
        res = r.gpu.render_views(cams, lights, r.W, r.H, mode=mode, max_depth=depth, out=out)
    else:
        with torch.cuda.stream(stream):
            full, out = sentinel_buffers(len(cams), r.H, r.W, names)
            res = r.gpu.render_views(cams, lights, r.W, r.H, mode=mode, max_depth=depth, out=out, stream=stream)
    assert set(res) == set(names)
    return collect(full, out) if sync and stream is None else (full, out)


def assert_views(got, want, what):
    for name in got:
        for k in range(got[name].shape[0]):
            assert bits(got[name][k]).tobytes() == bits(want[name][k]).tobytes(), f"{what}: {name} of view {k} differs"


def with_variant(rt, v, fn):
    prev = rt.set_variant(v)
    try:
        return fn()
    finally:
        rt.set_variant(prev)


# ---- 1. equal to rt_render, bit for bit ----
VIEWS = {1: [4], 2: [8, 1], 3: [2, 8, 5], 9: [3, 0, 8, 1, 7, 2, 6, 4, 5]}  # 9 blocks-of-views cross the 8-XCD round robin


@pytest.mark.parametrize("mode,depth", [(PRIMARY, 1), (PRIMARY, 3), (FULL, 2), (FULL, 4)])
@pytest.mark.parametrize("n", [1, 2, 3, 9])
@pytest.mark.parametrize("name", ["cornell", "material"])
def test_batch_equals_rt_render(rt, refs, name, n, mode, depth):
    r = refs[name]
    want = r.frames(VIEWS[n], LIGHTS, mode, depth)
    assert all((want["face"][k] >= 0).any() for k in range(n)), "every view sees the scene"
    got = batch(r, VIEWS[n], LIGHTS, mode, depth)
    assert_views(got, want, f"{name} n={n} mode {mode} depth {depth}")
    plan = rt.view_plan(mode, depth, (r.W + 15) // 16, (r.H + 15) // 16, n)
    assert plan["kernel"] == (1 if (mode, depth) == (PRIMARY, 1) else 2) and plan["total_blocks"] == n * plan["units_per_view"]


def test_the_cameras_of_a_batch_all_differ(refs):
    for r in refs.values():
        f = r.frames(range(9), LIGHTS, PRIMARY, 1)
        for a in range(9):
            for b in range(a):
                assert bits(f["t"][a]).tobytes() != bits(f["t"][b]).tobytes(), (r.name, a, b)


@pytest.mark.parametrize("mode,depth", [(PRIMARY, 0), (FULL, 0), (PRIMARY, 2)])
def test_one_tile_frames_and_the_modes_own_depth(rt, mode, depth):
    r = Ref(rt, "cornell", 16, 16)
    got = batch(r, [8, 0, 3], LIGHTS, mode, depth)
    assert_views(got, r.frames([8, 0, 3], LIGHTS, mode, depth), f"16x16 mode {mode} depth {depth}")


# ---- 2. equal to rt_render_lit, bit for bit ----
def ring32():
    lights = [tuple(l) + (0,) for l in E.ring_lights(32)]
    for k in (1, 16, 30):
        lights[k] = (lights[k][0], lights[k][1], 1)
    return lights


@pytest.mark.parametrize("name", ["cornell", "material"])
def test_batch_equals_rt_render_lit(rt, refs, name):
    r = refs[name]
    views = [6, 8, 2]
    ls32 = r.gpu.light_set(ring32())
    soft = rt.spherical_light((0.3, 0.45, 0.9) if name == "cornell" else (-0.5, 2.0, 3.0), (1.0, 1.0, 1.0), 0.3, 32)
    ls33 = r.gpu.light_set(soft)
    assert len(ls32) == 32 and len(ls33) == 33
    for mode, depth in ((PRIMARY, 1), (FULL, 2)):
        want = r.frames(views, ls32, mode, depth, key="ls32")
        assert_views(batch(r, views, ls32, mode, depth), want, f"{name} 32 lights, kernel arguments, mode {mode}")
        mem = with_variant(rt, MEM_LIGHTS, lambda: batch(r, views, ls32, mode, depth))
        assert_views(mem, want, f"{name} 32 lights from memory, mode {mode}")
    want = r.frames(views, ls33, FULL, 2, key="ls33")
    assert_views(batch(r, views, ls33, FULL, 2), want, f"{name} 33 lights, FULL")
    nc = with_variant(rt, NO_CACHE, lambda: batch(r, views, ls33, FULL, 2))
    assert_views(nc, want, f"{name} 33 lights, FULL, no occluder cache")
    assert_views(batch(r, views, ls33, PRIMARY, 1), r.frames(views, ls33, PRIMARY, 1, key="ls33"), f"{name} 33 lights, PRIMARY")


# ---- 3. one batch against the CPU oracle directly ----
def test_batch_against_the_oracle(rt, orc, refs):
    r = refs["cornell"]
    views = [1, 8, 5]
    osc = orc.Scene(orc.Mesh.load_obj(scene_path("cornell.obj")))
    ocams = [orc.flycam(r.W, r.H, *r.poses[v]) if v < 8 else look_at(orc, r.W, r.H, EYE, (0, 0, 0), (0, 1, 0), FOVY)
             for v in views]
    got = batch(r, views, LIGHTS, FULL, 2)
    hits = 0
    for k, ocam in enumerate(ocams):
        orgb, oface, ot = osc.render(ocam, [POINT], r.W, r.H, full=True, dir_lights=[DIRECTIONAL], max_depth=2)
        assert (got["face"][k].reshape(-1) == oface).all(), f"view {k}: face"
        assert bits(got["t"][k].reshape(-1)).tobytes() == bits(ot).tobytes(), f"view {k}: t"
        err = float(np.abs(got["rgb"][k].reshape(-1, 3) - orgb).max())
        print(f"view {k}: colour L_inf {err:.3g}")
        assert err < TOL, f"view {k}: colour L_inf {err}"
        hits += int((oface >= 0).sum())
    assert hits > 100


# ---- 4. optional outputs ----
@pytest.mark.parametrize("mode,depth", [(PRIMARY, 1), (FULL, 2)])
@pytest.mark.parametrize("names", [("rgb",), ("rgb", "face"), ("rgb", "t")])
def test_optional_outputs(rt, refs, names, mode, depth):
    r = refs["cornell"]
    views = [7, 8]
    want = r.frames(views, LIGHTS, mode, depth)
    spare, _ = sentinel_buffers(len(views), r.H, r.W, [k for k in WIDTH if k not in names])
    got = batch(r, views, LIGHTS, mode, depth, names=names)
    assert set(got) == set(names)
    assert_views(got, want, f"outputs {names} mode {mode}")
    torch.cuda.synchronize()
    assert untouched(spare)
    # want_hits allocates all three, without it rgb alone
    res = r.gpu.render_views([r.cams[v] for v in views], LIGHTS, r.W, r.H, mode=mode, max_depth=depth, want_hits=True)
    assert_views({k: x.cpu().numpy() for k, x in res.items()}, want, "allocated outputs")
    assert set(r.gpu.render_views([r.cams[7]], LIGHTS, r.W, r.H)) == {"rgb"}


# ---- 5. streams ----
def test_streams(rt, refs):
    r = refs["cornell"]
    a, b = [0, 8, 4], [5, 2, 8, 6, 1]  # different cameras and different sizes (the second grows nothing back)
    want_a, want_b = r.frames(a, LIGHTS, FULL, 2), r.frames(b, LIGHTS, FULL, 2)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    # two batches back to back on one stream, no synchronisation between them; then the same two on two streams
    pending = [(batch(r, a, LIGHTS, FULL, 2, stream=s1), want_a), (batch(r, b, LIGHTS, FULL, 2, stream=s1), want_b),
               (batch(r, a, LIGHTS, FULL, 2, stream=s1), want_a), (batch(r, b, LIGHTS, FULL, 2, stream=s2), want_b)]
    torch.cuda.synchronize()
    for k, ((full, out), want) in enumerate(pending):
        assert_views(collect(full, out), want, f"stream case {k}")
    # the scene's own stream, synchronous
    assert_views(batch(r, b, LIGHTS, PRIMARY, 1), r.frames(b, LIGHTS, PRIMARY, 1), "stream=None")
    # a batch issued while an rt_render_async frame of the same scene is in flight: both right
    want_f = r.frame(3, LIGHTS, FULL, 2)
    r.gpu.render_async(r.cams[3], LIGHTS, r.W, r.H, mode=FULL, flags=rt.RT_FRAME_WRITE_HITS)
    full, out = batch(r, a, LIGHTS, FULL, 2, stream=s2)
    r.gpu.synchronize()
    rgb, face, t = r.gpu.download(r.W, r.H, want_hits=True)
    torch.cuda.synchronize()
    assert_views(collect(full, out), want_a, "batch beside a frame in flight")
    assert_views({"rgb": rgb[None], "face": face[None], "t": t[None]}, {k: x[None] for k, x in want_f.items()},
                 "frame beside a batch")


# ---- 6. refusals on the device: nothing is written ----
def test_refusals_write_nothing(rt, refs):
    r = refs["cornell"]
    other = refs["material"]
    L = rt.lib()
    n = 2
    cams = (rt.Camera * n)(r.cams[0], r.cams[8])
    full, out = sentinel_buffers(n, r.H, r.W, ("rgb", "face", "t"))
    torch.cuda.synchronize()
    vb = rt.ViewBatch(n, C.cast(cams, C.c_void_p), out["rgb"].data_ptr(), out["face"].data_ptr(), out["t"].data_ptr())
    two = rt.Scene._lights(LIGHTS)
    many = rt.Scene._lights(E.ring_lights(33))
    ok = rt.Frame(r.W, r.H, FULL, 0, 1, 0, 0)

    def call(batch=vb, lights=two, n_lights=2, frame=ok):
        rc = L.rt_render_views(r.gpu.h, C.byref(batch), C.cast(lights, C.c_void_p), n_lights, C.byref(frame), None)
        assert rc == RT_OK or L.rt_last_error()
        return rc

    host_rgb = np.full((n, r.H, r.W, 3), 7.0, np.float32)
    host = rt.ViewBatch(n, C.cast(cams, C.c_void_p), host_rgb.ctypes.data, None, None)
    assert call(batch=host) == RT_ERR_INVALID and (host_rgb == 7.0).all()
    host_t = np.full((n, r.H, r.W), 7.0, np.float32)
    mixed = rt.ViewBatch(n, C.cast(cams, C.c_void_p), out["rgb"].data_ptr(), None, host_t.ctypes.data)
    assert call(batch=mixed) == RT_ERR_INVALID and (host_t == 7.0).all()
    assert call(frame=rt.Frame(r.W, r.H, BOX, 0, 1, 0, 0)) == RT_ERR_UNSUPPORTED
    assert call(frame=rt.Frame(r.W, r.H, FULL, 0, 2, 0, 0)) == RT_ERR_UNSUPPORTED
    assert call(frame=rt.Frame(r.W, r.H, FULL, 1, 2, 0, 0)) == RT_ERR_UNSUPPORTED
    for flags in (rt.RT_FRAME_STATS, rt.RT_FRAME_TIMELINE, rt.RT_FRAME_STATS | rt.RT_FRAME_WAVE_STATS):
        assert call(frame=rt.Frame(r.W, r.H, FULL, 0, 1, flags, 0)) == RT_ERR_UNSUPPORTED
    assert call(lights=many, n_lights=33) == RT_ERR_INVALID
    assert call(frame=rt.Frame(r.W, r.H, FULL, 0, 1, 0, 17)) == RT_ERR_INVALID
    assert call(batch=rt.ViewBatch(rt.RT_MAX_VIEWS + 1, vb.cameras, vb.rgb, vb.face, vb.t)) == RT_ERR_INVALID
    assert call(batch=rt.ViewBatch(n, None, vb.rgb, vb.face, vb.t)) == RT_ERR_INVALID
    assert call(batch=rt.ViewBatch(n, vb.cameras, None, vb.face, vb.t)) == RT_ERR_INVALID
    foreign = other.gpu.light_set(LIGHTS)
    assert L.rt_render_views_lit(r.gpu.h, C.byref(vb), foreign.h, C.byref(ok), None) == RT_ERR_INVALID
    assert "another scene" in L.rt_last_error().decode()
    assert L.rt_render_views_lit(r.gpu.h, C.byref(vb), None, C.byref(ok), None) == RT_ERR_INVALID
    torch.cuda.synchronize()
    assert untouched(full)
    # ... and the same batch is accepted once nothing is wrong with it
    assert call() == RT_OK
    assert_views(collect(full, out), r.frames([0, 8], LIGHTS, FULL, 2), "after the refusals")


# ---- 7. empty batch ----
def test_empty_batch(rt, refs):
    r = refs["cornell"]
    L = rt.lib()
    full, out = sentinel_buffers(1, r.H, r.W, ("rgb", "face", "t"))
    torch.cuda.synchronize()
    two = rt.Scene._lights(LIGHTS)
    ls = r.gpu.light_set(LIGHTS)
    for mode in (PRIMARY, FULL):
        fr = rt.Frame(r.W, r.H, mode, 0, 1, 0, 0)
        for vb in (rt.ViewBatch(0, None, None, None, None),
                   rt.ViewBatch(0, None, out["rgb"].data_ptr(), out["face"].data_ptr(), out["t"].data_ptr())):
            for stream in (None, C.c_void_p(torch.cuda.current_stream().cuda_stream)):
                assert L.rt_render_views(r.gpu.h, C.byref(vb), C.cast(two, C.c_void_p), 2, C.byref(fr), stream) == RT_OK
                assert L.rt_render_views_lit(r.gpu.h, C.byref(vb), ls.h, C.byref(fr), stream) == RT_OK
    res = r.gpu.render_views([], LIGHTS, r.W, r.H, want_hits=True)
    assert tuple(res["rgb"].shape) == (0, r.H, r.W, 3) and tuple(res["t"].shape) == (0, r.H, r.W)
    torch.cuda.synchronize()
    assert untouched(full)
