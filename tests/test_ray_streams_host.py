"""Ray streams, the part that needs no GPU: the ABI additions, the argument checks that come before any device
work, and the coherence key (csrc/rt_raykey.h through rt_debug_ray_keys)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import edge_scenes as E
from conftest import ROOT, scene_path

HEADER = os.path.join(ROOT, "include", "rt", "rt_api.h")
NEW = ["rt_trace_stream", "rt_rays_camera", "rt_scene_ray_bounds", "rt_debug_ray_keys", "rt_debug_ray_order"]
UNIT = np.array([-0.5, -0.5, -0.5, 0.5, 0.5, 0.5], np.float32)
DEGENERATE = np.uint32(0x80000000)
RT_ERR_INVALID, RT_ERR_NO_DEVICE = -1, -5


@pytest.fixture(scope="module")
def host_scene(rt):
    return rt.Scene(rt.Mesh.load_obj(scene_path("cube.obj")), device=rt.RT_DEVICE_NONE)


def last_error(rt):
    return rt.lib().rt_last_error().decode()


def test_header_and_library_carry_the_new_symbols(rt):
    text = open(HEADER).read()
    assert re.search(r"^#define RT_HAS_RAY_STREAMS 1\b", text, re.M)
    assert re.search(r"^#define RT_API_VERSION 4\b", text, re.M) and rt.lib().rt_version() == 4
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(rt.lib(), name), name
    for name in ("RT_RAYS_CLOSEST = 0", "RT_RAYS_SHADOW = 1", "RT_RAYS_COLOR = 2", "#define RT_RAYS_REORDER 1",
                 "#define RT_RAYS_STATS   2", "typedef struct rt_ray_stream"):
        assert name in text, name
    # the ctypes mirror has the header's nine fields: n, then eight pointers
    assert C.sizeof(rt.RayStream) == 8 + 8 * C.sizeof(C.c_void_p)


def test_host_only_scene_has_no_device(rt, host_scene):
    rs = rt.RayStream(4, 16, 16, 16, 16, None, None, 16, 16)  # never dereferenced: the scene check comes first
    for q in (rt.RT_RAYS_CLOSEST, rt.RT_RAYS_SHADOW, rt.RT_RAYS_COLOR):
        assert rt.lib().rt_trace_stream(host_scene.h, q, 0, C.byref(rs), None, 0, None) == RT_ERR_NO_DEVICE
        assert "host-only" in last_error(rt)
    cam = rt.flycam(8, 8)
    assert rt.lib().rt_rays_camera(host_scene.h, C.byref(cam), 8, 8, 16, 16, None) == RT_ERR_NO_DEVICE
    assert "host-only" in last_error(rt)
    n = C.c_int64(0)
    assert rt.lib().rt_debug_ray_order(host_scene.h, 0, None, C.byref(n)) == RT_ERR_NO_DEVICE


def test_argument_checks_before_any_device_work(rt, host_scene):
    L = rt.lib()
    rs = rt.RayStream(4, 16, 16, 16, 16, None, None, 16, 16)
    for q in (-1, 3, 99):
        assert L.rt_trace_stream(host_scene.h, q, 0, C.byref(rs), None, 0, None) == RT_ERR_INVALID
        assert "bad query" in last_error(rt)
    for fl in (4, 8, -1, 7):
        assert L.rt_trace_stream(host_scene.h, 0, fl, C.byref(rs), None, 0, None) == RT_ERR_INVALID
        assert "bad flags" in last_error(rt)
    assert L.rt_trace_stream(None, 0, 0, C.byref(rs), None, 0, None) == RT_ERR_INVALID
    assert L.rt_trace_stream(host_scene.h, 0, 0, None, None, 0, None) == RT_ERR_INVALID
    neg = rt.RayStream(-1, 16, 16, 16, 16, None, None, 16, 16)
    assert L.rt_trace_stream(host_scene.h, 0, 0, C.byref(neg), None, 0, None) == RT_ERR_INVALID
    # required outputs per query, and the lights of a colour query
    assert L.rt_trace_stream(host_scene.h, 0, 0, C.byref(rt.RayStream(4, 16, 16, None, 16)), None, 0, None) == RT_ERR_INVALID
    assert L.rt_trace_stream(host_scene.h, 0, 0, C.byref(rt.RayStream(4, 16, 16, 16, None)), None, 0, None) == RT_ERR_INVALID
    assert L.rt_trace_stream(host_scene.h, 1, 0, C.byref(rt.RayStream(4, 16, 16)), None, 0, None) == RT_ERR_INVALID
    assert L.rt_trace_stream(host_scene.h, 2, 0, C.byref(rt.RayStream(4, 16, 16)), None, 0, None) == RT_ERR_INVALID
    assert L.rt_trace_stream(host_scene.h, 2, 0, C.byref(rs), None, 33, None) == RT_ERR_INVALID
    assert L.rt_trace_stream(host_scene.h, 2, 0, C.byref(rs), None, 1, None) == RT_ERR_INVALID
    assert L.rt_trace_stream(host_scene.h, 0, 0, C.byref(rt.RayStream(4, None, 16, 16, 16)), None, 0, None) == RT_ERR_INVALID
    cam = rt.flycam(8, 8)
    assert L.rt_rays_camera(host_scene.h, None, 8, 8, 16, 16, None) == RT_ERR_INVALID
    assert L.rt_rays_camera(host_scene.h, C.byref(cam), 0, 8, 16, 16, None) == RT_ERR_INVALID
    assert L.rt_rays_camera(host_scene.h, C.byref(cam), 8, 8, None, 16, None) == RT_ERR_INVALID
    # the Python wrapper checks dtype, shape and contiguity itself
    with pytest.raises(TypeError):
        host_scene.trace_stream(0, np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32))
    # rt_debug_ray_keys: n = 0 is fine, a bad query or missing arrays are not
    assert L.rt_debug_ray_keys(0, 0, None, None, UNIT.ctypes.data, None) == 0
    assert len(rt.ray_keys(0, np.zeros((0, 3)), np.zeros((0, 3)), UNIT)) == 0
    assert L.rt_debug_ray_keys(3, 0, None, None, UNIT.ctypes.data, None) == RT_ERR_INVALID
    assert L.rt_debug_ray_keys(0, 2, None, None, UNIT.ctypes.data, None) == RT_ERR_INVALID
    assert L.rt_debug_ray_keys(0, -1, None, None, UNIT.ctypes.data, None) == RT_ERR_INVALID


def test_scene_bounds_are_the_world_vertices(rt, host_scene):
    b = host_scene.ray_bounds()
    assert b.dtype == np.float32 and (b[:3] < b[3:]).all()
    # the normalised cube spans [-0.5, 0.5]^3
    assert np.allclose(b, UNIT, atol=1e-6)


def random_rays(n, seed):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)


def test_keys_are_deterministic_and_31_bits_for_ordinary_rays(rt):
    o, d = random_rays(5000, 3)
    k = rt.ray_keys(0, o, d, UNIT)
    assert k.dtype == np.uint32 and (k == rt.ray_keys(0, o, d, UNIT)).all()
    assert not (k & DEGENERATE).any()
    assert len(np.unique(k)) > 4000  # the key separates rays
    # one ray at a time gives the same keys (no dependence on the list)
    assert all(rt.ray_keys(0, o[i], d[i], UNIT)[0] == k[i] for i in range(0, 5000, 371))


def test_top_bit_marks_exactly_the_degenerate_rays(rt):
    zo, zd = E.zero_direction_rays()
    assert (rt.ray_keys(0, zo, zd, UNIT) == DEGENERATE).all()
    o, d = random_rays(64, 4)
    bad = np.zeros(64, bool)
    vals = [np.nan, np.inf, -np.inf]
    for i in range(0, 36, 2):  # every component of origin and direction, each non-finite value
        arr, c = (o, i // 2 % 3) if i < 18 else (d, (i - 18) // 2 % 3)
        arr[i, c] = vals[(i // 6) % 3]
        bad[i] = True
    d[40] = [0.0, -0.0, 0.0]
    bad[40] = True
    d[42] = [0.0, 0.0, 1e-30]   # tiny but not zero: an ordinary ray
    d[44] = [3e38, 3e38, 3e38]  # |d| sums to +inf: still an ordinary ray
    o[46] = [1e30, -1e30, 0.0]  # far outside the bounds: clamped
    k = rt.ray_keys(0, o, d, UNIT)
    assert ((k & DEGENERATE) != 0).tolist() == bad.tolist()
    assert (k[bad] == DEGENERATE).all()  # no other bits: they sort last, by index


def test_origins_outside_the_bounds_clamp(rt):
    d = np.array([[0.3, 0.5, 0.8]] * 4, np.float32)
    inside = np.array([[-0.499, -0.499, -0.499], [0.499, 0.499, 0.499]], np.float32)
    outside = np.array([[-7.0, -1e20, -0.6], [0.51, 1e30, 123.0]], np.float32)
    k = rt.ray_keys(0, np.concatenate([inside, outside]), d, UNIT)
    assert k[0] == k[2] and k[1] == k[3] and k[0] != k[1]


def test_signed_zero_components_choose_the_octant(rt):
    o = np.zeros((2, 3), np.float32)
    for c in range(3):
        d = np.array([[0.5, 0.5, 0.5]] * 2, np.float32)
        d[0, c], d[1, c] = 0.0, -0.0
        k = rt.ray_keys(0, o, d, UNIT)
        assert k[0] != k[1], c
        # ... and -0.0 shares its octant with a small negative component
        d[0, c] = -1e-3
        k2 = rt.ray_keys(0, o, d, UNIT)
        assert abs(int(k2[0]) - int(k2[1])) < abs(int(k[0]) - int(k[1])), c


def test_neighbouring_directions_are_closer_than_opposite_octants(rt):
    o = np.array([[0.1, 0.2, 0.3]] * 3, np.float32)
    a = np.array([0.5, 0.6, 0.62], np.float32)
    d = np.stack([a, a + np.float32(0.01), -a]).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for variant in (0, 4194304):  # both key layouts
        prev = rt.set_variant(variant)
        try:
            k = rt.ray_keys(0, o, d, UNIT).astype(np.int64)
        finally:
            rt.set_variant(prev)
        assert abs(k[0] - k[1]) < abs(k[0] - k[2]), (variant, k)


def test_shadow_keys_use_P_and_L(rt):
    P, L = E.shadow_straddle_rays(256)
    assert (rt.ray_keys(1, P, L, UNIT) == rt.ray_keys(0, P, L, UNIT)).all()
    # not the offset origin P + 0.003 L, and not the roles swapped
    assert (rt.ray_keys(1, P, L, UNIT) != rt.ray_keys(1, L, P, UNIT)).any()


def test_degenerate_bounds_give_finite_keys(rt):
    (v, f, m, g), _ = E.tie_scene()
    sc = rt.Scene(rt.Mesh.from_arrays(v, f, m, groups=g), device=rt.RT_DEVICE_NONE, min_faces=8)
    o, d = E.tie_random_rays(512)
    for b in (sc.ray_bounds(), np.array([-0.5, -0.5, 0.375, 0.5, 0.5, 0.375], np.float32), np.zeros(6, np.float32)):
        k = rt.ray_keys(0, o, d, b)
        assert not (k & DEGENERATE).any()
    flat = rt.ray_keys(0, o, d, np.array([-0.5, -0.5, 0.375, 0.5, 0.5, 0.375], np.float32))
    o2 = o.copy()
    o2[:, 2] += np.float32(0.25)  # the flat axis is one cell: z does not enter the key
    assert (rt.ray_keys(0, o2, d, np.array([-0.5, -0.5, 0.375, 0.5, 0.5, 0.375], np.float32)) == flat).all()
