"""View batches (rt_render_views, rt_render_views_lit), the part that needs no GPU: the ABI additions, the plan of a
batch (csrc/rt_dispatch.h plan_views through rt_debug_view_plan) with every refusal and its status, and the
checks of both entry points that come before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, scene_path

HEADER = os.path.join(ROOT, "include", "rt", "rt_api.h")
RT_OK, RT_ERR_INVALID, RT_ERR_NO_DEVICE, RT_ERR_UNSUPPORTED = 0, -1, -5, -6
PRIMARY, FULL, BOX = 0, 1, 2
NONE, K_PRIMARY, K_DEPTH = 0, 1, 2
LS_KERNARG, LS_MEMORY, LS_MEMORY_CACHED = 0, 1, 2
GENERIC_DEPTH, NO_CACHE = 65536, 16777216
SYMBOLS = ("rt_render_views", "rt_render_views_lit", "rt_debug_view_plan")


@pytest.fixture(scope="module")
def host_scene(rt):
    return rt.Scene(rt.Mesh.load_obj(scene_path("cube.obj")), device=rt.RT_DEVICE_NONE)


def last_error(rt):
    return rt.lib().rt_last_error().decode()


def test_header_and_library_carry_the_new_symbols(rt):
    text = open(HEADER).read()
    assert re.search(r"^#define RT_HAS_VIEW_BATCHES 1\b", text, re.M)
    assert re.search(r"^#define RT_MAX_VIEWS 65536\b", text, re.M) and rt.RT_MAX_VIEWS == 65536
    assert re.search(r"^#define RT_API_VERSION 4\b", text, re.M) and rt.lib().rt_version() == 4
    assert re.search(r"typedef struct rt_view_batch \{", text)
    for name in SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(" % name, text, re.M), name
        assert hasattr(rt.lib(), name), name
        assert name in rt.EXPORTS
    # the binding's struct has the header's layout: int32 n_views, then four pointers
    assert C.sizeof(rt.ViewBatch) == 8 + 4 * C.sizeof(C.c_void_p)
    assert rt.ViewBatch.cameras.offset == 8 and rt.ViewBatch.t.offset == 8 + 3 * C.sizeof(C.c_void_p)


@pytest.mark.parametrize("mode,depth,mem,variant,kernel,limit", [
    (PRIMARY, 0, 0, 0, K_PRIMARY, 1), (PRIMARY, 1, 0, 0, K_PRIMARY, 1), (PRIMARY, 3, 0, 0, K_DEPTH, 3),
    (FULL, 0, 0, 0, K_DEPTH, 2), (FULL, 2, 0, 0, K_DEPTH, 2), (FULL, 4, 0, 0, K_DEPTH, 4),
    (PRIMARY, 0, 1, 0, K_DEPTH, 1), (PRIMARY, 1, 33, 0, K_DEPTH, 1), (FULL, 0, 100, 0, K_DEPTH, 2),
    (FULL, 16, 65536, 0, K_DEPTH, 16), (PRIMARY, 0, 0, GENERIC_DEPTH, K_DEPTH, 1),
])
def test_plan_kernel_and_recursion_limit(rt, mode, depth, mem, variant, kernel, limit):
    p = rt.view_plan(mode, depth, 3, 2, 5, variant=variant, mem_lights=mem)
    assert (p["kernel"], p["depth"], p["refused"], p["status"]) == (kernel, limit, 0, RT_OK), p
    assert p["light_source"] == (LS_MEMORY_CACHED if mem else LS_KERNARG)
    if mem:  # ... and without the occluder cache under its variant bit; the kernel-argument path ignores the bit
        assert rt.view_plan(mode, depth, 3, 2, 5, variant=variant | NO_CACHE, mem_lights=mem)["light_source"] == LS_MEMORY
    else:
        assert rt.view_plan(mode, depth, 3, 2, 5, variant=variant | NO_CACHE)["light_source"] == LS_KERNARG


@pytest.mark.parametrize("tx,ty,n", [(1, 1, 1), (3, 2, 9), (120, 68, 1), (4, 4, 65536), (8, 8, 65536 - 1), (1024, 1024, 15)])
def test_plan_units_and_blocks(rt, tx, ty, n):
    for mode in (PRIMARY, FULL):
        p = rt.view_plan(mode, 0, tx, ty, n)
        assert p["units_per_view"] == 4 * tx * ty and p["total_blocks"] == 4 * tx * ty * n and not p["refused"], p
    # flags 0 and RT_FRAME_WRITE_HITS, shard_count 0 and 1 are the same plan
    base = rt.view_plan(FULL, 3, tx, ty, n)
    for flags, sc in ((1, 0), (0, 1), (1, 1)):
        assert rt.view_plan(FULL, 3, tx, ty, n, flags=flags, shard_count=sc) == base


def test_plan_of_an_empty_batch(rt):
    for mode, mem in ((PRIMARY, 0), (FULL, 0), (FULL, 40)):
        p = rt.view_plan(mode, 0, 3, 2, 0, mem_lights=mem)
        assert (p["kernel"], p["total_blocks"], p["refused"], p["status"]) == (NONE, 0, 0, RT_OK), p
        assert p["units_per_view"] == 24


@pytest.mark.parametrize("kw,status", [
    (dict(mode=BOX), RT_ERR_UNSUPPORTED),
    (dict(shard_count=2), RT_ERR_UNSUPPORTED), (dict(shard_count=8), RT_ERR_UNSUPPORTED),
    (dict(flags=2), RT_ERR_UNSUPPORTED), (dict(flags=4), RT_ERR_UNSUPPORTED), (dict(flags=8), RT_ERR_UNSUPPORTED),
    (dict(flags=1 | 2 | 8), RT_ERR_UNSUPPORTED),
    (dict(n_views=65536 + 1), RT_ERR_INVALID), (dict(n_views=-1), RT_ERR_INVALID),
    (dict(tiles_x=8192, tiles_y=8192, n_views=8), RT_ERR_INVALID),  # 4 * 2^26 * 8 = 2^31 blocks
    (dict(tiles_x=1 << 27, tiles_y=1 << 27, n_views=65536), RT_ERR_INVALID),  # far beyond 64 bits unless saturated
    (dict(tiles_x=2048, tiles_y=2048, n_views=4), RT_ERR_INVALID),  # 2^26 blocks: 2^32 work-items, the launch's limit
    (dict(mode=7), RT_ERR_INVALID), (dict(max_depth=17), RT_ERR_INVALID), (dict(max_depth=-1), RT_ERR_INVALID),
    (dict(flags=16), RT_ERR_INVALID),
])
def test_plan_refusals_carry_their_status(rt, kw, status):
    args = dict(mode=FULL, max_depth=0, tiles_x=3, tiles_y=2, n_views=4)
    ok = rt.view_plan(**args)
    assert (ok["kernel"], ok["refused"], ok["status"]) == (K_DEPTH, 0, RT_OK)
    args.update(kw)
    p = rt.view_plan(**args)
    assert (p["kernel"], p["refused"], p["status"]) == (NONE, 1, status), p


def test_plan_limits_sit_where_documented(rt):
    # one block below the launch's limit is accepted: 2^26 - 4 blocks
    p = rt.view_plan(PRIMARY, 0, 2048, 2048, 3)
    assert not p["refused"] and p["total_blocks"] == 3 << 24
    p = rt.view_plan(PRIMARY, 0, 1, (1 << 24) - 1, 1)
    assert not p["refused"] and p["total_blocks"] == (1 << 26) - 4
    assert rt.view_plan(PRIMARY, 0, 1, 1 << 24, 1)["refused"]
    assert not rt.view_plan(PRIMARY, 0, 1, 1, 65536)["refused"]


def test_plan_hook_checks_its_own_arguments(rt):
    fn = rt.lib().rt_debug_view_plan
    good = np.array([FULL, 0, 0, 0, 3, 2, 4, 0, 0], np.int64)
    out = np.full(7, -77, np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert fn(p(good), 9, p(out), 7) == RT_OK and out[0] == K_DEPTH
    out[:] = -77
    for n_in, n_out in ((8, 7), (10, 7), (9, 6), (9, 8)):
        assert fn(p(good), n_in, p(out), n_out) == RT_ERR_INVALID and last_error(rt)
    assert fn(None, 9, p(out), 7) == RT_ERR_INVALID and fn(p(good), 9, None, 7) == RT_ERR_INVALID
    for k, v in ((4, 1 << 28), (6, 1 << 40), (7, -(1 << 40))):
        bad = good.copy()
        bad[k] = v
        assert fn(p(bad), 9, p(out), 7) == RT_ERR_INVALID, (k, v)
    assert (out == -77).all()


def test_entry_points_need_a_device_and_a_scene(rt, host_scene):
    """RT_ERR_NO_DEVICE on a host-only scene whatever else is passed (the device check comes first), RT_ERR_INVALID
    on a NULL scene; both leave a message."""
    L = rt.lib()
    cams = (rt.Camera * 2)(rt.flycam(16, 16), rt.flycam(16, 16, 1.0))
    lights = rt.Scene._lights(rt.DEFAULT_LIGHTS)
    fr = rt.Frame(16, 16, PRIMARY, 0, 1, 0, 0)
    rgb = np.full((2, 16, 16, 3), 7.0, np.float32)
    vb = rt.ViewBatch(2, C.cast(cams, C.c_void_p), rgb.ctypes.data, None, None)
    ls = host_scene.light_set(rt.DEFAULT_LIGHTS)
    empty = rt.ViewBatch(0, None, None, None, None)
    for batch in (vb, empty):
        assert L.rt_render_views(host_scene.h, C.byref(batch), C.cast(lights, C.c_void_p), 1, C.byref(fr), None) == RT_ERR_NO_DEVICE
        assert "host-only" in last_error(rt)
        assert L.rt_render_views_lit(host_scene.h, C.byref(batch), ls.h, C.byref(fr), None) == RT_ERR_NO_DEVICE
        assert "host-only" in last_error(rt)
        assert L.rt_render_views(None, C.byref(batch), C.cast(lights, C.c_void_p), 1, C.byref(fr), None) == RT_ERR_INVALID
        assert last_error(rt)
        assert L.rt_render_views_lit(None, C.byref(batch), ls.h, C.byref(fr), None) == RT_ERR_INVALID
        assert last_error(rt)
    # also with nothing else valid
    assert L.rt_render_views(host_scene.h, None, None, 99, None, None) == RT_ERR_NO_DEVICE
    assert L.rt_render_views_lit(host_scene.h, None, None, None, None) == RT_ERR_NO_DEVICE
    assert L.rt_render_views(None, None, None, 0, None, None) == RT_ERR_INVALID
    assert L.rt_render_views_lit(None, None, None, None, None) == RT_ERR_INVALID
    assert (rgb == 7.0).all()
    with pytest.raises(rt.RTError, match="host-only"):
        host_scene.render_views([rt.flycam(16, 16)], rt.DEFAULT_LIGHTS, 16, 16, out={"rgb": _FakeTensor((1, 16, 16, 3))})


class _FakeTensor:
    """What Scene.render_views needs of a tensor to reach the library: the call is refused before the pointer is used."""

    def __init__(self, shape):
        self.shape, self.dtype = shape, "float32"

    def data_ptr(self):
        return 64

    def is_contiguous(self):
        return True
