"""Supersampled views (rt_render_views_ss, rt_render_views_ss_lit, rt_render_ss), the part that needs no GPU: the
ABI additions, the grid and jittered sample patterns bit for bit, the plan of a supersampled batch
(csrc/rt_dispatch.h plan_views through rt_debug_sample_plan) in both layouts with every refusal, and the checks of
the entry points that come before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, scene_path

HEADER = os.path.join(ROOT, "include", "rt", "rt_api.h")
RT_OK, RT_ERR_INVALID, RT_ERR_NO_DEVICE, RT_ERR_UNSUPPORTED = 0, -1, -5, -6
PRIMARY, FULL, BOX = 0, 1, 2
LOOP, PACKED = 0, 1
SAMPLE_LAYOUT, GENERIC_DEPTH, NO_CACHE = 33554432, 65536, 16777216
SYMBOLS = ("rt_sample_pattern_grid", "rt_sample_pattern_jittered", "rt_render_views_ss", "rt_render_views_ss_lit",
           "rt_render_ss", "rt_debug_sample_plan")
RAND_MAX = 2147483647


@pytest.fixture(scope="module")
def host_scene(rt):
    return rt.Scene(rt.Mesh.load_obj(scene_path("cube.obj")), device=rt.RT_DEVICE_NONE)


def last_error(rt):
    return rt.lib().rt_last_error().decode()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_header_and_library_carry_the_new_symbols(rt):
    text = open(HEADER).read()
    assert re.search(r"^#define RT_HAS_SUPERSAMPLING 1\b", text, re.M)
    assert re.search(r"^#define RT_MAX_SAMPLES 64\b", text, re.M) and rt.RT_MAX_SAMPLES == 64
    assert re.search(r"^#define RT_API_VERSION 4\b", text, re.M) and rt.lib().rt_version() == 4
    assert re.search(r"typedef struct rt_sample_pattern \{", text)
    for name in SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(" % name, text, re.M), name
        assert hasattr(rt.lib(), name), name
        assert name in rt.EXPORTS
    # the binding's struct has the header's layout: int32 n_samples, then 64 (ox, oy) pairs
    assert C.sizeof(rt.SamplePattern) == 4 + 512
    assert rt.SamplePattern.n_samples.offset == 0 and rt.SamplePattern.offsets.offset == 4
    assert rt.VARIANT_SAMPLE_LAYOUT == SAMPLE_LAYOUT and str(SAMPLE_LAYOUT) in text


# ---- patterns ----
def grid_offsets(nx, ny, u=None):
    """the documented arithmetic: double, then one rounding to float32; u = per-cell (ux, uy), default the centre"""
    out = []
    for j in range(ny):
        for i in range(nx):
            ux, uy = u[j * nx + i] if u is not None else (0.5, 0.5)
            out.append((np.float32((i + ux) / nx - 0.5), np.float32((j + uy) / ny - 0.5)))
    return np.array(out, np.float32).reshape(-1, 2)


@pytest.mark.parametrize("nx,ny", [(1, 1), (2, 2), (3, 1), (4, 4), (8, 8), (1, 64), (5, 7)])
def test_grid_offsets_bit_exact(rt, nx, ny):
    p = rt.sample_grid(nx, ny)
    assert p.n_samples == nx * ny
    assert bits(p.array()).tobytes() == bits(grid_offsets(nx, ny)).tobytes()
    tail = np.array([[o[0], o[1]] for o in p.offsets[p.n_samples:]], np.float32)
    assert not tail.size or (bits(tail) == 0).all(), "offsets past n_samples are zero"
    if (nx, ny) == (1, 1):
        assert (bits(p.array()) == 0).all(), "1x1 is the offset (+0, +0)"
    if (nx, ny) == (2, 2):
        assert p.array().tolist() == [[-0.25, -0.25], [0.25, -0.25], [-0.25, 0.25], [0.25, 0.25]]


@pytest.mark.parametrize("nx,ny", [(9, 8), (65, 1), (1, 65), (0, 4), (4, 0), (-1, -1), (1 << 20, 1 << 20)])
def test_pattern_refusals(rt, nx, ny):
    p = rt.SamplePattern()
    p.n_samples = -77
    assert rt.lib().rt_sample_pattern_grid(nx, ny, C.byref(p)) == RT_ERR_INVALID and last_error(rt)
    assert rt.lib().rt_sample_pattern_jittered(nx, ny, None, C.byref(p)) == RT_ERR_INVALID and last_error(rt)
    assert p.n_samples == -77
    assert rt.lib().rt_sample_pattern_grid(2, 2, None) == RT_ERR_INVALID
    assert rt.lib().rt_sample_pattern_jittered(2, 2, None, None) == RT_ERR_INVALID


@pytest.mark.parametrize("nx,ny", [(1, 1), (2, 2), (3, 1), (4, 4), (8, 8)])
def test_jittered_offsets(rt, nx, ny):
    rng = rt.Rand(1)
    u = [(rng() / (RAND_MAX + 1.0), rng() / (RAND_MAX + 1.0)) for _ in range(nx * ny)]  # x first, then y, per cell
    want = grid_offsets(nx, ny, u)
    default = rt.sample_jittered(nx, ny)  # rng None: seed 1
    assert default.n_samples == nx * ny
    assert bits(default.array()).tobytes() == bits(want).tobytes()
    assert bits(rt.sample_jittered(nx, ny, rt.Rand(1)).array()).tobytes() == bits(want).tobytes()
    other = rt.sample_jittered(nx, ny, rt.Rand(7)).array()
    assert bits(other).tobytes() != bits(want).tobytes()
    assert bits(rt.sample_jittered(nx, ny, rt.Rand(7)).array()).tobytes() == bits(other).tobytes(), "reproducible"
    # a generator is advanced: the next pattern continues the sequence
    g = rt.Rand(1)
    rt.sample_jittered(nx, ny, g)
    assert g() == rng()
    # every sample inside its own cell (closed below; the rounding to float32 may reach the upper edge)
    for a in (default.array(), other):
        for j in range(ny):
            for i in range(nx):
                ox, oy = a[j * nx + i]
                assert i / nx - 0.5 <= ox <= (i + 1) / nx - 0.5 and j / ny - 0.5 <= oy <= (j + 1) / ny - 0.5, (i, j)


def test_sample_pattern_accepts_what_render_views_does(rt):
    g = rt.sample_grid(3, 1)
    assert rt.sample_pattern(g) is g
    assert bits(rt.sample_pattern((3, 1)).array()).tobytes() == bits(g.array()).tobytes()
    a = np.array([[0.0, 0.0], [0.75, -1.0], [0.125, 0.5]], np.float32)
    p = rt.sample_pattern(a)
    assert p.n_samples == 3 and bits(p.array()).tobytes() == bits(a).tobytes()
    with pytest.raises(ValueError):
        rt.sample_pattern(np.zeros((4, 3), np.float32))


# ---- the plan ----
@pytest.mark.parametrize("mode,depth,mem,variant", [
    (PRIMARY, 0, 0, 0), (PRIMARY, 3, 0, 0), (FULL, 0, 0, 0), (FULL, 4, 0, 0), (PRIMARY, 1, 33, 0), (FULL, 0, 100, NO_CACHE),
    (PRIMARY, 0, 0, GENERIC_DEPTH), (FULL, 2, 0, SAMPLE_LAYOUT),
])
@pytest.mark.parametrize("tx,ty,n", [(1, 1, 1), (3, 2, 9), (120, 68, 1), (3, 2, 0)])
def test_one_sample_is_the_view_plan(rt, mode, depth, mem, variant, tx, ty, n):
    v = rt.view_plan(mode, depth, tx, ty, n, variant=variant, mem_lights=mem)
    s = rt.sample_plan(mode, depth, tx, ty, n, 1, variant=variant, mem_lights=mem)
    assert {k: s[k] for k in rt.VIEW_PLAN_FIELDS} == v
    assert (s["layout"], s["pixels_per_wave"], s["waves_per_tile"]) == (LOOP, 64, 4)


def default_layout(rt, S):
    return rt.sample_plan(FULL, 0, 1, 1, 1, S)["layout"]


# S: (pixels per wave, waves per tile) of the packed layout
PACKED_SHAPE = {2: (32, 8), 4: (16, 16), 8: (8, 32), 16: (4, 64), 32: (2, 128), 64: (1, 256)}


@pytest.mark.parametrize("S", [2, 3, 4, 5, 8, 16, 32, 63, 64])
def test_block_counts_per_layout(rt, S):
    tx, ty, n = 3, 2, 5
    plans = {v: rt.sample_plan(FULL, 0, tx, ty, n, S, variant=v) for v in (0, SAMPLE_LAYOUT)}
    view = rt.view_plan(FULL, 0, tx, ty, n)
    for p in plans.values():
        assert not p["refused"] and p["status"] == RT_OK and p["why"] == ""
        assert (p["kernel"], p["depth"], p["light_source"]) == (view["kernel"], view["depth"], view["light_source"])
    if S not in PACKED_SHAPE:  # not a power of two: the loop, whatever the bit says
        assert plans[0] == plans[SAMPLE_LAYOUT] and plans[0]["layout"] == LOOP
    else:  # the bit selects the other layout
        assert {plans[0]["layout"], plans[SAMPLE_LAYOUT]["layout"]} == {LOOP, PACKED}
    for p in plans.values():
        if p["layout"] == LOOP:
            assert (p["pixels_per_wave"], p["waves_per_tile"]) == (64, 4)
            assert p["units_per_view"] == 4 * tx * ty and p["total_blocks"] == 4 * tx * ty * n
        else:
            assert (p["pixels_per_wave"], p["waves_per_tile"]) == PACKED_SHAPE[S]
            assert p["pixels_per_wave"] * S == 64 and p["waves_per_tile"] * p["pixels_per_wave"] == 256
            assert p["units_per_view"] == 4 * S * tx * ty and p["total_blocks"] == 4 * S * tx * ty * n


@pytest.mark.parametrize("S", [4, 16, 64])
def test_the_block_limit_comes_s_times_sooner_when_packed(rt, S):
    loop_v = 0 if default_layout(rt, S) == LOOP else SAMPLE_LAYOUT
    packed_v = loop_v ^ SAMPLE_LAYOUT
    # loop: rt_render_views' limit, 2^26 - 4 blocks accepted and 2^26 refused
    assert rt.sample_plan(PRIMARY, 0, 1, (1 << 24) - 1, 1, S, variant=loop_v)["total_blocks"] == (1 << 26) - 4
    p = rt.sample_plan(PRIMARY, 0, 1, 1 << 24, 1, S, variant=loop_v)
    assert (p["refused"], p["status"]) == (1, RT_ERR_INVALID) and "2^26" in p["why"] and "8x8-pixel blocks" in p["why"]
    # packed: the same launch limit on S times the blocks
    ty = (1 << 24) // S
    p = rt.sample_plan(PRIMARY, 0, 1, ty - 1, 1, S, variant=packed_v)
    assert not p["refused"] and p["total_blocks"] == (1 << 26) - 4 * S and p["layout"] == PACKED
    p = rt.sample_plan(PRIMARY, 0, 1, ty, 1, S, variant=packed_v)
    assert (p["kernel"], p["refused"], p["status"]) == (0, 1, RT_ERR_INVALID)
    assert "2^26" in p["why"] and "one-wave blocks" in p["why"]
    assert not rt.sample_plan(PRIMARY, 0, 1, ty, 1, S, variant=loop_v)["refused"]
    # saturated far beyond 64 bits
    assert rt.sample_plan(PRIMARY, 0, 1 << 27, 1 << 27, 65536, S, variant=packed_v)["status"] == RT_ERR_INVALID


@pytest.mark.parametrize("kw,status,why", [
    (dict(n_samples=0), RT_ERR_INVALID, "n_samples"), (dict(n_samples=65), RT_ERR_INVALID, "n_samples"),
    (dict(n_samples=-4), RT_ERR_INVALID, "n_samples"),
    (dict(mode=BOX), RT_ERR_UNSUPPORTED, "box colours"),
    (dict(shard_count=2), RT_ERR_UNSUPPORTED, "whole frames"),
    (dict(flags=2), RT_ERR_UNSUPPORTED, "no counters"), (dict(flags=4), RT_ERR_UNSUPPORTED, "no counters"),
    (dict(flags=8), RT_ERR_UNSUPPORTED, "no counters"),
    (dict(n_views=65536 + 1), RT_ERR_INVALID, "n_views"), (dict(n_views=-1), RT_ERR_INVALID, "n_views"),
    (dict(mode=7), RT_ERR_INVALID, "bad mode"), (dict(max_depth=17), RT_ERR_INVALID, "max_depth"),
    (dict(max_depth=-1), RT_ERR_INVALID, "max_depth"), (dict(flags=16), RT_ERR_INVALID, "bad flags"),
    (dict(tiles_x=0), RT_ERR_INVALID, "empty frame"),
    (dict(tiles_x=2048, tiles_y=2048, n_views=4), RT_ERR_INVALID, "2^26"),
])
@pytest.mark.parametrize("variant", [0, SAMPLE_LAYOUT])
def test_plan_refusals_carry_status_and_message(rt, kw, status, why, variant):
    args = dict(mode=FULL, max_depth=0, tiles_x=3, tiles_y=2, n_views=4, n_samples=4, variant=variant)
    ok = rt.sample_plan(**args)
    assert (ok["kernel"], ok["refused"], ok["status"], ok["why"]) == (2, 0, RT_OK, "")
    args.update(kw)
    p = rt.sample_plan(**args)
    assert (p["kernel"], p["refused"], p["status"]) == (0, 1, status), p
    assert why in p["why"] and p["why"].startswith("rt_debug_sample_plan: "), p["why"]


def test_plan_hook_checks_its_own_arguments(rt):
    fn = rt.lib().rt_debug_sample_plan
    good = np.array([FULL, 0, 0, 0, 3, 2, 4, 0, 0, 4], np.int64)
    out = np.full(10, -77, np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert fn(p(good), 10, p(out), 10) == RT_OK and out[0] == 2 and out[8] in (64, 16)
    out[:] = -77
    for n_in, n_out in ((9, 10), (11, 10), (10, 7), (10, 11), (9, 7)):
        assert fn(p(good), n_in, p(out), n_out) == RT_ERR_INVALID and last_error(rt)
    assert fn(None, 10, p(out), 10) == RT_ERR_INVALID and fn(p(good), 10, None, 10) == RT_ERR_INVALID
    for k, v in ((4, 1 << 28), (6, 1 << 40), (9, 1 << 40)):
        bad = good.copy()
        bad[k] = v
        assert fn(p(bad), 10, p(out), 10) == RT_ERR_INVALID, (k, v)
    assert (out == -77).all()
    # rt_debug_view_plan keeps its own lengths
    assert rt.lib().rt_debug_view_plan(p(good), 10, p(out), 7) == RT_ERR_INVALID
    assert rt.lib().rt_debug_view_plan(p(good), 9, p(out), 10) == RT_ERR_INVALID


# ---- entry points ----
def test_entry_points_need_a_device_and_a_scene(rt, host_scene):
    """rt_render_views' order: RT_ERR_INVALID on a NULL scene, then RT_ERR_NO_DEVICE on a host-only scene whatever
    else is passed -- a bad or missing pattern included; both leave a message."""
    L = rt.lib()
    cams = (rt.Camera * 2)(rt.flycam(16, 16), rt.flycam(16, 16, 1.0))
    lights = rt.Scene._lights(rt.DEFAULT_LIGHTS)
    fr = rt.Frame(16, 16, PRIMARY, 0, 1, 0, 0)
    rgb = np.full((2, 16, 16, 3), 7.0, np.float32)
    vb = rt.ViewBatch(2, C.cast(cams, C.c_void_p), rgb.ctypes.data, None, None)
    ls = host_scene.light_set(rt.DEFAULT_LIGHTS)
    empty = rt.ViewBatch(0, None, None, None, None)
    good = rt.sample_grid(2, 2)
    bad = rt.SamplePattern()
    bad.n_samples = 99
    for pat in (C.byref(good), C.byref(bad), None):
        for batch in (vb, empty):
            assert L.rt_render_views_ss(host_scene.h, C.byref(batch), C.cast(lights, C.c_void_p), 1, C.byref(fr), pat, None) == RT_ERR_NO_DEVICE
            assert "host-only" in last_error(rt)
            assert L.rt_render_views_ss_lit(host_scene.h, C.byref(batch), ls.h, C.byref(fr), pat, None) == RT_ERR_NO_DEVICE
            assert "host-only" in last_error(rt)
            assert L.rt_render_views_ss(None, C.byref(batch), C.cast(lights, C.c_void_p), 1, C.byref(fr), pat, None) == RT_ERR_INVALID
            assert last_error(rt)
            assert L.rt_render_views_ss_lit(None, C.byref(batch), ls.h, C.byref(fr), pat, None) == RT_ERR_INVALID
            assert last_error(rt)
        assert L.rt_render_ss(host_scene.h, C.byref(cams[0]), C.cast(lights, C.c_void_p), 1, C.byref(fr), pat, rgb.ctypes.data) == RT_ERR_NO_DEVICE
        assert "host-only" in last_error(rt)
        assert L.rt_render_ss(None, C.byref(cams[0]), C.cast(lights, C.c_void_p), 1, C.byref(fr), pat, rgb.ctypes.data) == RT_ERR_INVALID
        assert last_error(rt)
    # also with nothing else valid
    assert L.rt_render_views_ss(host_scene.h, None, None, 99, None, None, None) == RT_ERR_NO_DEVICE
    assert L.rt_render_views_ss_lit(host_scene.h, None, None, None, None, None) == RT_ERR_NO_DEVICE
    assert L.rt_render_ss(host_scene.h, None, None, 99, None, None, None) == RT_ERR_NO_DEVICE
    assert L.rt_render_views_ss(None, None, None, 0, None, None, None) == RT_ERR_INVALID
    assert L.rt_render_views_ss_lit(None, None, None, None, None, None) == RT_ERR_INVALID
    assert L.rt_render_ss(None, None, None, 0, None, None, None) == RT_ERR_INVALID
    assert (rgb == 7.0).all()
    with pytest.raises(rt.RTError, match="host-only"):
        host_scene.render_views([rt.flycam(16, 16)], rt.DEFAULT_LIGHTS, 16, 16, samples=(2, 2),
                                out={"rgb": _FakeTensor((1, 16, 16, 3))})
    with pytest.raises(rt.RTError, match="host-only"):
        host_scene.render_ss(rt.flycam(16, 16), rt.DEFAULT_LIGHTS, 16, 16, (2, 2))


class _FakeTensor:
    """What Scene.render_views needs of a tensor to reach the library: the call is refused before the pointer is used."""

    def __init__(self, shape):
        self.shape, self.dtype = shape, "float32"

    def data_ptr(self):
        return 64

    def is_contiguous(self):
        return True
