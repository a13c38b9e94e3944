"""rt_trace_stream_color / rt_debug_ray_levels, the part that needs no GPU: the ABI additions and the argument checks
that come before any device work (a host-only scene, pointers that are never dereferenced)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT, scene_path

HEADER = os.path.join(ROOT, "include", "rt", "rt_api.h")
RT_ERR_INVALID, RT_ERR_NO_DEVICE = -1, -5
PRIMARY, FULL = 0, 1


@pytest.fixture(scope="module")
def host_scene(rt):
    return rt.Scene(rt.Mesh.load_obj(scene_path("cube.obj")), device=rt.RT_DEVICE_NONE)


def last_error(rt):
    return rt.lib().rt_last_error().decode()


def good(rt, n=4):
    return rt.RayStream(n, 16, 16, 16, 16, None, None, None, 16)  # never dereferenced


def test_header_and_library_carry_the_new_symbols(rt):
    text = open(HEADER).read()
    assert re.search(r"^#define RT_HAS_RAY_DEPTH 1\b", text, re.M)
    assert re.search(r"^#define RT_RAYS_WAVEFRONT 4\b", text, re.M) and rt.RT_RAYS_WAVEFRONT == 4
    assert re.search(r"^#define RT_API_VERSION 4\b", text, re.M) and rt.lib().rt_version() == 4
    for name in ("rt_trace_stream_color", "rt_debug_ray_levels"):
        assert re.search(r"^int %s\s*\(" % name, text, re.M), name
        assert hasattr(rt.lib(), name), name
        assert name in rt.EXPORTS
    # rt_ray_stream keeps its layout
    assert C.sizeof(rt.RayStream) == 8 + 8 * C.sizeof(C.c_void_p)


def test_argument_checks_before_any_device_work(rt, host_scene):
    f = rt.lib().rt_trace_stream_color
    h = host_scene.h
    rs = good(rt)
    for mode in (2, -1):
        assert f(h, 0, C.byref(rs), None, 0, mode, 0, None) == RT_ERR_INVALID
        assert "bad mode" in last_error(rt)
    for depth in (-1, 17):
        for mode in (PRIMARY, FULL):
            assert f(h, 0, C.byref(rs), None, 0, mode, depth, None) == RT_ERR_INVALID
            assert "max_depth" in last_error(rt)
    for flags in (8, -1, 15):
        assert f(h, flags, C.byref(rs), None, 0, FULL, 0, None) == RT_ERR_INVALID
        assert "bad flags" in last_error(rt)
    # the order of concern: mode before depth before flags before the list
    assert f(h, 8, None, None, 0, 2, 17, None) == RT_ERR_INVALID and "bad mode" in last_error(rt)
    assert f(h, 8, None, None, 0, FULL, 17, None) == RT_ERR_INVALID and "max_depth" in last_error(rt)
    assert f(h, 8, None, None, 0, FULL, 3, None) == RT_ERR_INVALID and "bad flags" in last_error(rt)
    assert f(None, 0, C.byref(rs), None, 0, FULL, 0, None) == RT_ERR_INVALID
    for flags in (0, 1, 4, 5, 7):
        assert f(h, flags, None, None, 0, FULL, 3, None) == RT_ERR_INVALID
        assert f(h, flags, C.byref(good(rt, -1)), None, 0, FULL, 3, None) == RT_ERR_INVALID
        no_rgb = rt.RayStream(4, 16, 16, 16, 16, None, None, None, None)
        assert f(h, flags, C.byref(no_rgb), None, 0, PRIMARY, 3, None) == RT_ERR_INVALID
        assert "rgb3" in last_error(rt)
        assert f(h, flags, C.byref(rt.RayStream(4, None, 16, 16, 16, None, None, None, 16)), None, 0, FULL, 0, None) == RT_ERR_INVALID
        assert f(h, flags, C.byref(rt.RayStream(4, 16, None, 16, 16, None, None, None, 16)), None, 0, FULL, 0, None) == RT_ERR_INVALID
        assert f(h, flags, C.byref(rs), None, 33, FULL, 3, None) == RT_ERR_INVALID
        assert f(h, flags, C.byref(rs), None, 1, PRIMARY, 0, None) == RT_ERR_INVALID


def test_host_only_scene_has_no_device(rt, host_scene):
    rs = good(rt)
    for mode, depth, flags in ((FULL, 0, 0), (FULL, 2, 4), (PRIMARY, 3, 0), (FULL, 16, 7), (PRIMARY, 0, 5)):
        assert rt.lib().rt_trace_stream_color(host_scene.h, flags, C.byref(rs), None, 0, mode, depth, None) == RT_ERR_NO_DEVICE
        assert "host-only" in last_error(rt)
    # ... for an empty list too, as rt_trace_stream
    assert rt.lib().rt_trace_stream_color(host_scene.h, 0, C.byref(good(rt, 0)), None, 0, FULL, 0, None) == RT_ERR_NO_DEVICE
    n = C.c_int32(0)
    assert rt.lib().rt_debug_ray_levels(host_scene.h, 0, None, C.byref(n)) == RT_ERR_NO_DEVICE
    # the Python wrapper checks its tensors itself
    import numpy as np
    with pytest.raises(TypeError):
        host_scene.trace_stream_color(np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), [])


def test_trace_stream_still_refuses_the_wavefront_flag(rt, host_scene):
    rs = rt.RayStream(4, 16, 16, 16, 16, None, None, 16, 16)
    for q in (rt.RT_RAYS_CLOSEST, rt.RT_RAYS_SHADOW, rt.RT_RAYS_COLOR):
        assert rt.lib().rt_trace_stream(host_scene.h, q, 4, C.byref(rs), None, 0, None) == RT_ERR_INVALID
        assert "bad flags" in last_error(rt)
