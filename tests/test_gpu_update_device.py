"""rt_scene_update_device on the MI355X: a scene updated from device tensors equals, bit for bit, a scene freshly
created from the same arrays, and its records equal the host path's byte for byte -- every word the update's kernels
compute (normals, plane distances, ranks, box ids, the safe-normal and certificate bits, shading normals, the pad,
the accept-region bounds) against the host stages'. Scenes, amplitudes, the 96x64 frames and the 4096 rays are
tests/update_scenes.py's; every update gets the arrays of U.mesh_of(...).export() as torch tensors, so the host
comparison sees the same bytes."""
import numpy as np
import pytest
import torch

import update_scenes as U
from test_gpu_scene_update import RAYS, Q_CLOSEST, dev, frames, identical, same_frames, same_traces, traces

pytestmark = pytest.mark.gpu
W, H = U.W, U.H
NONE = -2  # RT_DEVICE_NONE


@pytest.fixture(scope="module", autouse=True)
def need_gpu(rt):
    if rt.device_count() == 0:
        pytest.skip("no GPU")


def tensors(mesh):
    """The three device arrays of a mesh (the bytes a host update of `mesh` reads)."""
    ex = mesh.export()
    return dev(ex["v4"].astype(np.float32)), dev(ex["vn3"].astype(np.float32)), dev(ex["fn3"].astype(np.float32))


def update_device(sc, mesh, M=None, **kw):
    v, vn, fn = tensors(mesh)
    return sc.update_device(v, vn, fn, model_matrix=mesh.export()["M16"] if M is None else M, **kw)


def same_host_half(sc, fresh, what):
    for a, b in zip(sc.ref_boxes(), fresh.ref_boxes()):
        assert np.array_equal(a, b), what
    (ff, ro), (wf, wro) = sc.face_flags(), fresh.face_flags()
    assert np.array_equal(ff, wf) and ro == wro, what
    assert np.array_equal(sc.ray_bounds(), fresh.ray_bounds()), what
    val = sc.validate_bvh()
    assert val["ok"] and val["violations"] == 0, (what, val)


# ---- 1. every step matches a fresh scene ----
@pytest.mark.parametrize("name", U.SCENES)
def test_every_step_matches_a_fresh_scene(rt, name):
    arr, M, seq = U.scene_steps(rt, name)
    sc = rt.Scene(U.mesh_of(rt, arr), shape_model_matrix=M)
    first = frames(rt, sc, name)
    first_rays = traces(rt, sc)
    prev = sc.ref_boxes()
    changed = []
    for step, v in enumerate(seq):
        what = f"{name} step {step}"
        mesh = U.mesh_of(rt, arr, v)
        st = update_device(sc, mesh, M, stats=True)
        assert st["bounds_on_device"] == 1 and st["total_ms"] > 0, what
        fresh = rt.Scene(mesh, shape_model_matrix=M)
        got, want = frames(rt, sc, name), frames(rt, fresh, name)
        same_frames(got, want, what)
        hit = float((want["primary"][1] >= 0).mean())
        print(f"{what}: {hit:.3f} of the pixels hit; stats {st}")
        assert hit >= 0.2, what
        got_rays, want_rays = traces(rt, sc), traces(rt, fresh)
        same_traces(got_rays, want_rays, what)
        same_host_half(sc, fresh, what)
        boxes = sc.ref_boxes()
        changed.append(len(boxes[0]) != len(prev[0]) or not np.array_equal(boxes[2], prev[2]))
        prev = boxes
        assert st["sah_cost"] == sc.tree_cost()["sah"]
    same_frames(got, first, f"{name} back at the original")
    same_traces(got_rays, first_rays, f"{name} back at the original")
    if name == "bunny":
        assert any(changed)


# ---- 2. / 3. the records equal the host path's ----
def records_follow_the_host(rt, arr, M, steps, what, **kw):
    mesh0 = U.mesh_of(rt, arr)
    on_dev = rt.Scene(mesh0, shape_model_matrix=M, **kw)
    on_host = rt.Scene(mesh0, device=NONE, shape_model_matrix=M, **kw)
    for step, (v, Ms) in enumerate(steps):
        mesh = U.mesh_of(rt, arr, v)
        Mu = mesh.export()["M16"] if Ms is None else Ms
        assert update_device(on_dev, mesh, Mu, stats=True)["bounds_on_device"] == 1
        assert on_host.update(mesh, model_matrix=Mu, stats=True)["bounds_on_device"] == 0
        for which in range(3):
            a, b = on_dev.records(which), on_host.records(which)
            assert a.shape == b.shape and np.array_equal(a, b), (what, step, which, int((a != b).sum()))
        assert on_dev.validate_bvh() == on_host.validate_bvh(), (what, step)
        assert on_dev.tree_cost() == on_host.tree_cost(), (what, step)
        for a, b in zip(on_dev.ref_boxes(), on_host.ref_boxes()):
            assert np.array_equal(a, b), (what, step)
        assert on_dev.face_flags()[1] == on_host.face_flags()[1]
    return on_dev


@pytest.mark.parametrize("name,builder", [("cornell", 0), ("tie", 0), ("material", 0), ("bunny", 0), ("bunny", 2)])
def test_records_equal_the_host_path(rt, name, builder):
    arr, M, seq = U.scene_steps(rt, name)
    steps = [(v, M) for v in seq]
    if name == "cornell":  # tilted normals: accept-region bounds, certificates off; and back
        M0 = U.mesh_of(rt, arr).export()["M16"]
        steps += [(arr[0], U.rotated_stretched(M0)), (arr[0], M0)]
    records_follow_the_host(rt, arr, M, steps, (name, builder), builder=builder)


@pytest.mark.parametrize("name", ["cornell", "tie"])
def test_many_small_boxes(rt, name):
    """min_faces = 4: many boxes, multi-pass splits, boxes of a handful of faces (the rank and partition stages)."""
    arr, M, seq = U.scene_steps(rt, name)
    on_dev = records_follow_the_host(rt, arr, M, [(v, M) for v in seq[:2]], (name, "min_faces 4"), builder=0, min_faces=4)
    assert on_dev.info()["n_ref_boxes"] > 4
    mesh = U.mesh_of(rt, arr, seq[1])
    fresh = rt.Scene(mesh, shape_model_matrix=M, min_faces=4)
    sc = rt.Scene(U.mesh_of(rt, arr), shape_model_matrix=M, min_faces=4)
    update_device(sc, mesh, M)
    same_frames(frames(rt, sc, name), frames(rt, fresh, name), f"{name} min_faces 4")
    same_traces(traces(rt, sc), traces(rt, fresh), f"{name} min_faces 4")
    same_host_half(sc, fresh, f"{name} min_faces 4")


def test_one_triangle(rt):
    """A single-leaf root with its sentinel child."""
    v = np.array([[-0.5, -0.4, 0.0], [0.6, -0.3, 0.1], [0.0, 0.5, -0.1]], np.float32)
    f = np.array([[0, 1, 2]], np.uint32)
    mats = U.scene_arrays(rt, "cornell")[2][:1]
    arr = (v, f, mats, [(1, 0)])
    mesh0 = U.mesh_of(rt, arr)
    M = mesh0.export()["M16"]
    v1 = (v * np.float32(0.75) + np.float32(0.0625)).astype(np.float32)
    records_follow_the_host(rt, arr, M, [(v1, M), (v, M)], "one triangle", builder=0)
    sc = rt.Scene(mesh0, shape_model_matrix=M)
    mesh1 = U.mesh_of(rt, arr, v1)
    assert update_device(sc, mesh1, M, stats=True)["bounds_on_device"] == 1
    fresh = rt.Scene(mesh1, shape_model_matrix=M)
    cam = rt.flycam(W, H, 0, 0, 20)
    for a, b in zip(sc.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=rt.RT_MODE_FULL, want_hits=True)[:3],
                    fresh.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=rt.RT_MODE_FULL, want_hits=True)[:3]):
        identical(a, b, "one triangle")
    same_host_half(sc, fresh, "one triangle")


# ---- 4. a non-finite vertex ----
def test_nan_vertex_takes_the_host_path(rt):
    arr = U.scene_arrays(rt, "cornell")
    mesh0 = U.mesh_of(rt, arr)
    M = mesh0.export()["M16"]  # (the loader's normalisation of a NaN extent is no matrix to test with)
    sc = rt.Scene(mesh0)
    first = frames(rt, sc, "cornell")
    vnan = U.deform(arr[0], U.AMPLITUDES[0])
    vnan[5, 1] = np.nan
    mesh = U.mesh_of(rt, arr, vnan)
    v, vn, fn = tensors(mesh)
    v[5, 1] = float("nan")  # written into the device tensor (the mesh's own array holds it too)
    assert bool(torch.isnan(v).sum() == 1)
    st = sc.update_device(v, vn, fn, model_matrix=M, stats=True)
    assert st["bounds_on_device"] == 0
    fresh = rt.Scene(mesh, shape_model_matrix=M)
    got = frames(rt, sc, "cornell")
    same_frames(got, frames(rt, fresh, "cornell"), "NaN vertex")
    same_traces(traces(rt, sc), traces(rt, fresh), "NaN vertex")
    for a, b in zip(sc.ref_boxes(), fresh.ref_boxes()):
        assert np.array_equal(a, b)
    assert (got["primary"][1] >= 0).mean() >= 0.2
    assert update_device(sc, mesh0, M, stats=True)["bounds_on_device"] == 1
    same_frames(frames(rt, sc, "cornell"), first, "back from the NaN vertex")


# ---- what the features below are compared against ----
@pytest.fixture(scope="module")
def bunny_pair(rt):
    arr, _, seq = U.scene_steps(rt, "bunny")
    mesh = U.mesh_of(rt, arr, seq[1])
    return arr, mesh, rt.Scene(mesh)


def original_bunny(rt, bunny_pair, **kw):
    return rt.Scene(U.mesh_of(rt, bunny_pair[0]), **kw)


# ---- 5. ordering ----
def test_update_behind_frames_in_flight(rt, bunny_pair):
    sc = original_bunny(rt, bunny_pair, frames_in_flight=4)
    Wb, Hb = 640, 360
    cams = [rt.flycam(Wb, Hb, 0.5 * k, 0, 20) for k in range(4)]
    want_last = sc.render(cams[3], rt.DEFAULT_LIGHTS, Wb, Hb, mode=rt.RT_MODE_FULL)[0]
    for cam in cams:
        sc.render_async(cam, rt.DEFAULT_LIGHTS, Wb, Hb, mode=rt.RT_MODE_FULL)
    update_device(sc, bunny_pair[1])
    identical(sc.download(Wb, Hb), want_last, "the last frame before the update saw the old scene")
    same_frames(frames(rt, sc, "bunny"), frames(rt, bunny_pair[2], "bunny"), "after frames in flight")
    sc.synchronize()


def test_update_behind_a_list_on_a_side_stream(rt, bunny_pair):
    sc = original_bunny(rt, bunny_pair)
    reps = 256  # 1M rays
    o, d = dev(np.tile(RAYS[0], (reps, 1))), dev(np.tile(RAYS[1], (reps, 1)))
    want = {k: v.cpu().numpy() for k, v in sc.trace_stream(Q_CLOSEST, o, d).items()}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got = sc.trace_stream(Q_CLOSEST, o, d, stream=side)
    update_device(sc, bunny_pair[1])
    side.synchronize()
    for k in want:
        identical(got[k].cpu().numpy(), want[k], f"list before the update {k}")
    same_frames(frames(rt, sc, "bunny"), frames(rt, bunny_pair[2], "bunny"), "after the list")


def test_arrays_produced_on_a_side_stream(rt, bunny_pair):
    """The vertices come out of a long elementwise chain on a side stream; stream=side orders the update's reads
    behind it with no synchronise in between."""
    sc = original_bunny(rt, bunny_pair)
    v, vn, fn = tensors(bunny_pair[1])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        big = torch.zeros(1 << 24, device="cuda")
        for _ in range(20):
            big = big + 1.0  # the stream is busy before the chain starts
        x = v.clone()
        for _ in range(400):  # exact in fp32: each pair restores the bits (powers of two, no overflow)
            x = x * 2.0
            x = x * 0.5
    sc.update_device(x, vn, fn, model_matrix=bunny_pair[1].export()["M16"], stream=side)
    same_frames(frames(rt, sc, "bunny"), frames(rt, bunny_pair[2], "bunny"), "arrays from a side stream")


# ---- 6. what lives across an update ----
def test_light_set_made_before(rt, bunny_pair):
    sc, fresh = original_bunny(rt, bunny_pair), bunny_pair[2]
    lights = [((np.cos(k), np.sin(k), 1.0), (0.02, 0.03, 0.025)) for k in range(40)]
    ls = sc.light_set(lights)
    update_device(sc, bunny_pair[1])
    cam = rt.flycam(W, H, 0, 0, 20)
    got = sc.render_lit(cam, ls, W, H, mode=rt.RT_MODE_FULL, want_hits=True)
    want = fresh.render_lit(cam, fresh.light_set(lights), W, H, mode=rt.RT_MODE_FULL, want_hits=True)
    for part, a, b in zip(("rgb", "face", "t"), got[:3], want[:3]):
        identical(a, b, f"light set {part}")


def test_views_supersampling_and_wavefront_after(rt, bunny_pair):
    sc, fresh = original_bunny(rt, bunny_pair), bunny_pair[2]
    cams = [rt.flycam(W, H, dx, 0, 20) for dx in (-2.0, 0.0, 2.0)]
    sc.render_views(cams, rt.DEFAULT_LIGHTS, W, H, mode=rt.RT_MODE_FULL, want_hits=True)
    o, d = dev(RAYS[0]), dev(RAYS[1])
    sc.trace_stream_color(o, d, rt.DEFAULT_LIGHTS, wavefront=True)
    update_device(sc, bunny_pair[1])
    got = sc.render_views(cams, rt.DEFAULT_LIGHTS, W, H, mode=rt.RT_MODE_FULL, want_hits=True)
    want = fresh.render_views(cams, rt.DEFAULT_LIGHTS, W, H, mode=rt.RT_MODE_FULL, want_hits=True)
    for k in want:
        identical(got[k].cpu().numpy(), want[k].cpu().numpy(), f"view batch {k}")
    identical(sc.render_ss(cams[1], rt.DEFAULT_LIGHTS, W, H, (2, 2), mode=rt.RT_MODE_FULL),
              fresh.render_ss(cams[1], rt.DEFAULT_LIGHTS, W, H, (2, 2), mode=rt.RT_MODE_FULL), "supersampled frame")
    for reorder in (False, True):
        a = sc.trace_stream_color(o, d, rt.DEFAULT_LIGHTS, wavefront=True, reorder=reorder, max_depth=3)
        b = fresh.trace_stream_color(o, d, rt.DEFAULT_LIGHTS, wavefront=True, reorder=reorder, max_depth=3)
        for k in b:
            identical(a[k].cpu().numpy(), b[k].cpu().numpy(), f"wavefront colour {k}")


def test_box_colours_after(rt, bunny_pair):
    sc, fresh = original_bunny(rt, bunny_pair), bunny_pair[2]
    cam = rt.flycam(W, H, 0, 0, 20)
    sc.set_box_colors()
    sc.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=rt.RT_MODE_BOX_COLORS)
    n_before = sc.info()["n_ref_boxes"]
    update_device(sc, bunny_pair[1])
    assert sc.info()["n_ref_boxes"] == fresh.info()["n_ref_boxes"] != n_before
    sc.set_box_colors()
    fresh.set_box_colors()
    got = sc.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=rt.RT_MODE_BOX_COLORS, want_hits=True)
    want = fresh.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=rt.RT_MODE_BOX_COLORS, want_hits=True)
    for part, a, b in zip(("rgb", "face", "t"), got[:3], want[:3]):
        identical(a, b, f"box colours {part}")


def test_two_replicas_on_one_gpu(rt, bunny_pair):
    sc, fresh = original_bunny(rt, bunny_pair, devices=[0, 0]), bunny_pair[2]
    frames(rt, sc, "bunny")
    update_device(sc, bunny_pair[1])
    same_frames(frames(rt, sc, "bunny"), frames(rt, fresh, "bunny"), "two replicas")
    assert np.array_equal(sc.ray_bounds(), fresh.ray_bounds())  # (through the scene whose host half the replica shares)
    same_traces(traces(rt, sc), traces(rt, fresh), "two replicas")
    cam = rt.flycam(W, H, 0, 0, 20)
    sc.set_box_colors()
    fresh.set_box_colors()
    got = sc.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=rt.RT_MODE_BOX_COLORS, want_hits=True)
    want = fresh.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=rt.RT_MODE_BOX_COLORS, want_hits=True)
    identical(got[0], want[0], "two replicas, box colours")


def test_save_and_load(rt, bunny_pair, tmp_path):
    sc = original_bunny(rt, bunny_pair)
    update_device(sc, bunny_pair[1])
    path = str(tmp_path / "updated.rtscene")
    sc.save(path)
    loaded = rt.Scene.load(path)
    same_frames(frames(rt, loaded, "bunny"), frames(rt, bunny_pair[2], "bunny"), "saved and loaded")
    assert loaded.validate_bvh()["ok"]
    for a, b in zip(loaded.ref_boxes(), bunny_pair[2].ref_boxes()):
        assert np.array_equal(a, b)


def test_debug_ray(rt, bunny_pair):
    sc, fresh = original_bunny(rt, bunny_pair), bunny_pair[2]
    update_device(sc, bunny_pair[1])
    cam = rt.flycam(W, H, 0, 0, 20)
    got = sc.debug_ray(cam, rt.DEFAULT_LIGHTS, W / 2, H / 2, max_depth=3)
    want = fresh.debug_ray(cam, rt.DEFAULT_LIGHTS, W / 2, H / 2, max_depth=3)
    assert len(got) == len(want) >= 1
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            identical(np.atleast_1d(a), np.atleast_1d(b), "debug ray")


# ---- 7. device, host, device ----
def test_mixed_sequence(rt):
    arr, M, seq = U.scene_steps(rt, "bunny")
    sc = rt.Scene(U.mesh_of(rt, arr))
    for step, (v, on_device) in enumerate(zip(seq, (True, False, True))):
        mesh = U.mesh_of(rt, arr, v)
        if on_device:
            update_device(sc, mesh)
        else:
            sc.update(mesh)
        fresh = rt.Scene(mesh)
        same_frames(frames(rt, sc, "bunny"), frames(rt, fresh, "bunny"), f"mixed step {step}")
        same_host_half(sc, fresh, f"mixed step {step}")


# ---- 8. refusals ----
def test_refusals_leave_the_scene_unchanged(rt):
    arr = U.scene_arrays(rt, "cornell")
    mesh0 = U.mesh_of(rt, arr)
    sc = rt.Scene(mesh0)
    first = frames(rt, sc, "cornell")
    recs = [sc.records(w).copy() for w in range(3)]
    mesh = U.mesh_of(rt, arr, U.steps(arr)[1])
    v, vn, fn = tensors(mesh)
    with pytest.raises(rt.RTError):  # host memory
        sc.update_device(v.cpu(), vn, fn)
    with pytest.raises(rt.RTError):
        sc.update_device(v, vn, fn.cpu())
    with pytest.raises(ValueError):  # a wrong shape
        sc.update_device(v[:, :3].contiguous(), vn, fn)
    with pytest.raises(ValueError):
        sc.update_device(v, vn, fn[:-1])
    wide = rt.Scene(mesh0, wide_tree=1)
    with pytest.raises(rt.RTError):
        wide.update_device(v, vn, fn)
    assert rt.lib().rt_last_error().decode().find("wide_tree") >= 0
    for w in range(3):
        assert np.array_equal(sc.records(w), recs[w]), w
    same_frames(frames(rt, sc, "cornell"), first, "after the refusals")
    # a light set and a view batch made afterwards still work, and so does the update
    ls = sc.light_set([((0.0, 1.0, 1.0), (0.5, 0.5, 0.5))])
    cam = rt.flycam(W, H, 0, 0, 20)
    sc.render_lit(cam, ls, W, H, mode=rt.RT_MODE_FULL)
    sc.render_views([cam], rt.DEFAULT_LIGHTS, W, H)
    update_device(sc, mesh)
    same_frames(frames(rt, sc, "cornell"), frames(rt, rt.Scene(mesh), "cornell"), "after the refusals, updated")
