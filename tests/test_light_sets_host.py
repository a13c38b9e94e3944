"""Light sets (rt_light_set, rt_render_lit, rt_trace_stream_lit), the part that needs no GPU: the ABI additions, a
set's order and limits on a host-only scene, the argument checks that come before any device work, and the
dispatch plan of a frame whose lights are read from device memory."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, scene_path

HEADER = os.path.join(ROOT, "include", "rt", "rt_api.h")
RT_OK, RT_ERR_INVALID, RT_ERR_NO_DEVICE = 0, -1, -5
PRIMARY, FULL = 0, 1
P, D = 0, 1  # RT_LIGHT_POINT, RT_LIGHT_DIRECTIONAL
GENERIC, FUSED, MEGAKERNEL = 1, 2, 7
SMALL = 5 << 20
SYMBOLS = ("rt_light_set_create", "rt_light_set_destroy", "rt_light_set_get", "rt_render_lit", "rt_render_lit_async",
           "rt_trace_stream_lit")


@pytest.fixture(scope="module")
def host_scene(rt):
    return rt.Scene(rt.Mesh.load_obj(scene_path("cube.obj")), device=rt.RT_DEVICE_NONE)


@pytest.fixture(scope="module")
def other_scene(rt):
    return rt.Scene(rt.Mesh.load_obj(scene_path("plane.obj")), device=rt.RT_DEVICE_NONE)


def last_error(rt):
    return rt.lib().rt_last_error().decode()


def test_header_and_library_carry_the_new_symbols(rt):
    text = open(HEADER).read()
    assert re.search(r"^#define RT_HAS_LIGHT_SETS 1\b", text, re.M)
    assert re.search(r"^#define RT_MAX_LIGHT_SET 65536\b", text, re.M) and rt.RT_MAX_LIGHT_SET == 65536
    assert re.search(r"^#define RT_MAX_LIGHTS 32\b", text, re.M)
    assert re.search(r"^#define RT_API_VERSION 4\b", text, re.M) and rt.lib().rt_version() == 4
    for name in SYMBOLS:
        assert re.search(r"^(int|void)\s+%s\s*\(" % name, text, re.M), name
        assert hasattr(rt.lib(), name), name
        assert name in rt.EXPORTS
    assert "8388608" in text  # the memory-path variant bit is documented beside the others


def seven_lights():
    kinds = [D, P, D, P, P, D, P]
    return [((float(i), 0.5 * i, -1.0 * i), (0.1 * i, 0.2, 0.3), k) for i, k in enumerate(kinds)]


def test_a_set_keeps_calculate_colors_order(rt, host_scene):
    lights = seven_lights()
    ls = host_scene.light_set(lights)
    assert len(ls) == 7
    got = ls.lights()
    assert [g[2] for g in got] == [P, P, P, P, D, D, D]
    want = [l for l in lights if l[2] == P] + [l for l in lights if l[2] == D]
    for g, w in zip(got, want):
        assert np.array_equal(np.array(g[0], np.float32), np.array(w[0], np.float32))
        assert np.array_equal(np.array(g[1], np.float32), np.array(w[1], np.float32))
    # too small a capacity: refused, nothing written
    out = (rt.Light * 7)()
    C.memset(out, 0x5A, C.sizeof(out))
    n = C.c_int32(-7)
    assert rt.lib().rt_light_set_get(ls.h, 6, out, C.byref(n)) == RT_ERR_INVALID
    assert bytes(out) == b"\x5a" * C.sizeof(out) and n.value == -7
    assert rt.lib().rt_light_set_get(None, 7, out, C.byref(n)) == RT_ERR_INVALID
    # any kind that is not directional is a point light
    odd = host_scene.light_set([((1, 2, 3), (1, 1, 1), 7), ((4, 5, 6), (1, 1, 1), D), ((7, 8, 9), (1, 1, 1), -1)])
    assert [g[2] for g in odd.lights()] == [P, P, D] and odd.lights()[1][0] == (7.0, 8.0, 9.0)


def test_set_sizes_and_invalid_arguments(rt, host_scene):
    f = rt.lib().rt_light_set_create
    h = C.c_void_p()
    empty = host_scene.light_set([])
    assert len(empty) == 0 and empty.lights() == []
    big = (rt.Light * 65537)()
    for i in (0, 65535, 65536):
        big[i].position[0] = float(i)
    assert f(host_scene.h, big, 65536, C.byref(h)) == RT_OK and h.value
    n = C.c_int32(0)
    assert rt.lib().rt_light_set_get(h, 0, None, C.byref(n)) == RT_OK and n.value == 65536
    back = (rt.Light * 65536)()
    assert rt.lib().rt_light_set_get(h, 65536, back, None) == RT_OK and back[65535].position[0] == 65535.0
    rt.lib().rt_light_set_destroy(h)
    rt.lib().rt_light_set_destroy(None)  # a no-op
    for args in ((host_scene.h, big, 65537), (host_scene.h, big, -1), (host_scene.h, None, 1), (None, big, 1)):
        h = C.c_void_p(1)
        assert f(args[0], args[1], args[2], C.byref(h)) == RT_ERR_INVALID
        assert h.value is None  # *out is cleared on failure
    assert f(host_scene.h, big, 1, None) == RT_ERR_INVALID
    assert f(host_scene.h, None, 0, C.byref(h)) == RT_OK  # no lights, no array
    rt.lib().rt_light_set_destroy(h)


def good(rt, n=4):
    return rt.RayStream(n, 16, 16, 16, 16, None, None, None, 16)  # never dereferenced


def test_host_only_scene_has_no_device(rt, host_scene):
    ls = host_scene.light_set(seven_lights())
    with pytest.raises(rt.RTError, match="host-only"):
        host_scene.render_lit(rt.flycam(64, 64), ls, 64, 64)
    fr = rt.Frame(64, 64, FULL, 0, 1, 0, 0)
    cam = rt.flycam(64, 64)
    assert rt.lib().rt_render_lit(host_scene.h, C.byref(cam), ls.h, C.byref(fr), None, None) == RT_ERR_NO_DEVICE
    assert rt.lib().rt_render_lit_async(host_scene.h, C.byref(cam), ls.h, C.byref(fr)) == RT_ERR_NO_DEVICE
    rs = good(rt)
    for mode, depth, flags in ((FULL, 0, 0), (FULL, 2, 4), (PRIMARY, 3, 0), (FULL, 16, 7), (PRIMARY, 0, 5)):
        assert rt.lib().rt_trace_stream_lit(host_scene.h, flags, C.byref(rs), ls.h, mode, depth, None) == RT_ERR_NO_DEVICE
        assert "host-only" in last_error(rt)
    assert rt.lib().rt_trace_stream_lit(host_scene.h, 0, C.byref(good(rt, 0)), ls.h, FULL, 0, None) == RT_ERR_NO_DEVICE


def test_a_set_of_another_scene_is_refused(rt, host_scene, other_scene):
    ls = host_scene.light_set(seven_lights())
    fr = rt.Frame(64, 64, FULL, 0, 1, 0, 0)
    cam = rt.flycam(64, 64)
    assert rt.lib().rt_render_lit(other_scene.h, C.byref(cam), ls.h, C.byref(fr), None, None) == RT_ERR_INVALID
    assert "another scene" in last_error(rt)
    assert rt.lib().rt_render_lit_async(other_scene.h, C.byref(cam), ls.h, C.byref(fr)) == RT_ERR_INVALID
    assert rt.lib().rt_trace_stream_lit(other_scene.h, 0, C.byref(good(rt)), ls.h, FULL, 0, None) == RT_ERR_INVALID
    assert "another scene" in last_error(rt)
    # ... and no set at all
    assert rt.lib().rt_render_lit(host_scene.h, C.byref(cam), None, C.byref(fr), None, None) == RT_ERR_INVALID
    assert rt.lib().rt_trace_stream_lit(host_scene.h, 0, C.byref(good(rt)), None, FULL, 0, None) == RT_ERR_INVALID
    assert rt.lib().rt_trace_stream_lit(None, 0, C.byref(good(rt)), ls.h, FULL, 0, None) == RT_ERR_INVALID


def test_list_argument_checks_before_any_device_work(rt, host_scene):
    """The checks and messages of rt_trace_stream_color, in its order: mode, depth, flags, the list."""
    f = rt.lib().rt_trace_stream_lit
    ls = host_scene.light_set(seven_lights())
    h, rs = host_scene.h, good(rt)
    for mode in (2, -1):
        assert f(h, 0, C.byref(rs), ls.h, mode, 0, None) == RT_ERR_INVALID and "bad mode" in last_error(rt)
    for depth in (-1, 17):
        assert f(h, 0, C.byref(rs), ls.h, FULL, depth, None) == RT_ERR_INVALID and "max_depth" in last_error(rt)
    for flags in (8, -1, 15):
        assert f(h, flags, C.byref(rs), ls.h, FULL, 0, None) == RT_ERR_INVALID and "bad flags" in last_error(rt)
    assert f(h, 8, None, ls.h, 2, 17, None) == RT_ERR_INVALID and "bad mode" in last_error(rt)
    assert f(h, 8, None, ls.h, FULL, 17, None) == RT_ERR_INVALID and "max_depth" in last_error(rt)
    assert f(h, 8, None, ls.h, FULL, 3, None) == RT_ERR_INVALID and "bad flags" in last_error(rt)
    for flags in (0, 1, 4, 5, 7):
        assert f(h, flags, None, ls.h, FULL, 3, None) == RT_ERR_INVALID
        assert f(h, flags, C.byref(good(rt, -1)), ls.h, FULL, 3, None) == RT_ERR_INVALID
        no_rgb = rt.RayStream(4, 16, 16, 16, 16, None, None, None, None)
        assert f(h, flags, C.byref(no_rgb), ls.h, PRIMARY, 3, None) == RT_ERR_INVALID and "rgb3" in last_error(rt)
        assert f(h, flags, C.byref(rt.RayStream(4, None, 16, 16, 16, None, None, None, 16)), ls.h, FULL, 0, None) == RT_ERR_INVALID


# ---- the dispatch plan ----
PLAN_INPUTS = [(PRIMARY, 0, 0, 40, 23, 0, 1, 0, SMALL, False, True), (FULL, 0, 0, 40, 23, 0, 1, 0, SMALL, False, True),
               (FULL, 3, 0, 40, 23, 0, 1, 0, SMALL, False, True), (FULL, 0, 2, 120, 68, 0, 8, 0, 150 << 20, True, False),
               (2, 0, 0, 4, 3, 0, 1, 65536, SMALL, False, True)]


def test_eleven_inputs_keep_their_plans(rt):
    want_kernel = [FUSED, MEGAKERNEL, GENERIC, MEGAKERNEL, FUSED]
    for inp, k in zip(PLAN_INPUTS, want_kernel):
        p11 = rt.frame_plan(*inp)
        assert p11["kernel"] == k, inp
        assert rt.frame_plan(*inp, mem_lights=0) == p11, inp  # in[11] = 0 equals the 11-input plan


def test_memory_lights_take_the_generic_kernel(rt):
    for mode, depth, want_depth in ((PRIMARY, 0, 1), (FULL, 0, 2), (FULL, 3, 3)):
        p = rt.frame_plan(mode, depth, 0, 40, 23, 0, 1, 0, SMALL, False, True, mem_lights=100)
        assert p["kernel"] == GENERIC and p["depth"] == want_depth, (mode, depth, p)
        assert p["writes_wave_stats"] == 0  # out slot 8: RT_FRAME_WAVE_STATS is refused on this path
        assert p["lpt"] == 1 and p["needs_variants"] == 0 and p["units"] == 4 * p["grid"]
        # not alone: no longest-first order, as for every other one-wave kernel
        assert rt.frame_plan(mode, depth, 0, 40, 23, 0, 1, 0, SMALL, False, False, mem_lights=100)["lpt"] == 0
    # a box-colours frame has no lights: its kernel stays
    assert rt.frame_plan(2, 0, 0, 40, 23, 0, 1, 0, SMALL, False, True, mem_lights=100)["kernel"] == FUSED


def test_plan_input_counts(rt):
    fn = rt.lib().rt_debug_frame_plan
    out = np.zeros(14, np.int32)
    inp = np.array([FULL, 0, 0, 40, 23, 0, 1, 0, SMALL, 0, 1, 100, 0], np.int64)
    assert fn(inp.ctypes.data, 13, out.ctypes.data, 14) == RT_ERR_INVALID
    assert fn(inp.ctypes.data, 10, out.ctypes.data, 14) == RT_ERR_INVALID
    assert fn(inp.ctypes.data, 12, out.ctypes.data, 14) == RT_OK and out[0] == GENERIC
    assert fn(inp.ctypes.data, 11, out.ctypes.data, 14) == RT_OK and out[0] == MEGAKERNEL
    inp[11] = -1
    assert fn(inp.ctypes.data, 12, out.ctypes.data, 14) == RT_ERR_INVALID
