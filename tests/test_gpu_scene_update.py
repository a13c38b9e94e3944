"""rt_scene_update on the MI355X: after every step of a deformation sequence every query of the updated scene gives,
bit for bit, what a scene freshly created from the same mesh description gives; the refit kernels' records are
byte-equal to the host refit's; and what lives across an update (light sets, frame slots and scratch, replicas,
the scene cache) keeps working. Frames are 96x64 and the ray lists 4096 rays; scenes and amplitudes are
tests/update_scenes.py's."""
import numpy as np
import pytest
import torch

import update_scenes as U
from test_oracle_pinning import same_bits

pytestmark = pytest.mark.gpu
W, H = U.W, U.H
NONE = -2  # RT_DEVICE_NONE
Q_CLOSEST, Q_SHADOW = 0, 1


@pytest.fixture(scope="module", autouse=True)
def need_gpu(rt):
    if rt.device_count() == 0:
        pytest.skip("no GPU")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def identical(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    if a.dtype.kind == "f":
        ok = same_bits(a.reshape(-1), b.reshape(-1))
    else:
        ok = a.reshape(-1) == b.reshape(-1)
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} values differ"


def frames(rt, sc, name):
    """PRIMARY, FULL at depth 2 and FULL at depth 4: {key: (rgb, face, t)}."""
    cam = rt.flycam(W, H, 0, 0, U.CAMERA_DZ[name])
    out = {}
    for key, mode, depth in (("primary", rt.RT_MODE_PRIMARY, 0), ("full2", rt.RT_MODE_FULL, 2), ("full4", rt.RT_MODE_FULL, 4)):
        rgb, face, t, _ = sc.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=mode, want_hits=True, max_depth=depth)
        out[key] = (rgb, face, t)
    return out


def same_frames(got, want, what):
    for key in want:
        for part, a, b in zip(("rgb", "face", "t"), got[key], want[key]):
            identical(a, b, f"{what} {key} {part}")


RAYS = U.rays()


def traces(rt, sc):
    """rt_trace_stream closest and shadow on the seeded rays, in the given order and with RT_RAYS_REORDER."""
    o, d = dev(RAYS[0]), dev(RAYS[1])
    L = dev((RAYS[0] + 3.0 * RAYS[1]).astype(np.float32))  # shadow segments from the origins through the scene
    out = {}
    for reorder in (False, True):
        c = sc.trace_stream(Q_CLOSEST, o, d, reorder=reorder)
        s = sc.trace_stream(Q_SHADOW, o, L, reorder=reorder)
        out[reorder] = {k: v.cpu().numpy() for k, v in c.items()}
        out[reorder]["blocked"] = s["blocked"].cpu().numpy()
    return out


def same_traces(got, want, what):
    for reorder in want:
        for k in want[reorder]:
            identical(got[reorder][k], want[reorder][k], f"{what} rays reorder={reorder} {k}")


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
        if name == "tie":
            assert U.tie_copies_coincide(v)
        mesh = U.mesh_of(rt, arr, v)
        st = sc.update(mesh, model_matrix=M, stats=True)
        assert st["bounds_on_device"] == 1, what
        fresh = rt.Scene(mesh, shape_model_matrix=M)
        got, want = frames(rt, sc, name), frames(rt, fresh, name)
        same_frames(got, want, what)
        hit = float((want["primary"][1] >= 0).mean())
        print(f"{what}: {hit:.3f} of the pixels hit, sah {st['sah_cost']:.2f} (fresh {fresh.tree_cost()['sah']:.2f})")
        assert hit >= 0.2, what
        got_rays, want_rays = traces(rt, sc), traces(rt, fresh)
        same_traces(got_rays, want_rays, what)
        assert 0.05 < (want_rays[False]["face"] >= 0).mean() < 1.0 and 0 < want_rays[False]["blocked"].mean() < 1
        boxes, wboxes = sc.ref_boxes(), fresh.ref_boxes()
        for a, b in zip(boxes, wboxes):
            assert np.array_equal(a, b), what
        changed.append(len(boxes[0]) != len(prev[0]) or not np.array_equal(boxes[2], prev[2]))
        prev = boxes
        assert np.array_equal(sc.face_flags()[0], fresh.face_flags()[0]) and sc.face_flags()[1] == fresh.face_flags()[1]
        assert np.array_equal(sc.ray_bounds(), fresh.ray_bounds())
        val = sc.validate_bvh()  # (through the host mirror, refreshed from the device)
        assert val["ok"] and val["violations"] == 0, (what, val)
    same_frames(got, first, f"{name} back at the original")
    same_traces(got_rays, first_rays, f"{name} back at the original")
    if name == "bunny":
        assert any(changed)


def test_bunny_step_against_the_cpu_oracle(rt, orc):
    from test_gpu_parity import compare
    arr, M, seq = U.scene_steps(rt, "bunny")
    sc = rt.Scene(U.mesh_of(rt, arr))
    sc.update(U.mesh_of(rt, arr, seq[1]))
    osc = orc.Scene(orc.Mesh.from_arrays(seq[1], arr[1], arr[2], groups=arr[3]))
    pix = np.array([(i, j) for j in range(0, H, 2) for i in range(0, W, 2)], np.int32)
    for full in (False, True):
        rgb, face, t, _ = sc.render(rt.flycam(W, H, 0, 0, 20), rt.DEFAULT_LIGHTS, W, H,
                                    mode=rt.RT_MODE_FULL if full else rt.RT_MODE_PRIMARY, want_hits=True)
        orgb, oface, ot = osc.render(orc.flycam(W, H, 0, 0, 20), orc.DEFAULT_LIGHTS, W, H, full=full, pixels=pix, threads=16)
        i, j = pix[:, 0], pix[:, 1]
        compare(rgb[j, i], face[j, i], t[j, i], orgb, oface, ot, f"updated bunny full={full}")
        assert (face >= 0).mean() >= 0.2


def test_model_matrix_change_and_back(rt):
    """cornell under a rotated and stretched model matrix (accept-region bounds, certificates off) and back."""
    arr = U.scene_arrays(rt, "cornell")
    mesh = U.mesh_of(rt, arr)
    M0 = mesh.export()["M16"]
    M1 = U.rotated_stretched(M0)
    sc = rt.Scene(mesh)
    first = frames(rt, sc, "cornell")
    assert sc.face_flags()[1] > 0
    for M in (M1, M0):
        sc.update(mesh, model_matrix=M)
        fresh = rt.Scene(mesh, shape_model_matrix=M)
        got = frames(rt, sc, "cornell")
        same_frames(got, frames(rt, fresh, "cornell"), "cornell model matrix")
        same_traces(traces(rt, sc), traces(rt, fresh), "cornell model matrix")
        assert sc.face_flags()[1] == fresh.face_flags()[1] and (sc.face_flags()[1] > 0) == (M is M0)
        assert (got["primary"][1] >= 0).mean() >= 0.2
        assert sc.validate_bvh()["ok"]
    same_frames(got, first, "cornell back at its matrix")


@pytest.mark.parametrize("name,builder", [("cornell", 0), ("tie", 0), ("material", 0), ("bunny", 0), ("bunny", 2)])
def test_kernel_records_equal_the_host_refit(rt, name, builder):
    """The same host-built tree on the device and in a host-only scene, updated through the same steps: the three
    record images stay byte-equal (binary nodes, triangle records, shading records). Builder 2 (spatial splits):
    clipped leaves and duplicated references."""
    arr, M, seq = U.scene_steps(rt, name)
    mesh0 = U.mesh_of(rt, arr)
    on_dev = rt.Scene(mesh0, shape_model_matrix=M, builder=builder)
    on_host = rt.Scene(mesh0, device=NONE, shape_model_matrix=M, builder=builder)
    steps = [(v, M) for v in seq]
    if name == "cornell":  # the accept-region triangles' path of k_refit_slots, and back
        M0 = mesh0.export()["M16"]
        steps += [(arr[0], U.rotated_stretched(M0)), (arr[0], M0)]
    for which in range(3):
        assert np.array_equal(on_dev.records(which), on_host.records(which)), (name, "created", which)
    for step, (v, Ms) in enumerate(steps):
        mesh = U.mesh_of(rt, arr, v)
        assert on_dev.update(mesh, model_matrix=Ms, stats=True)["bounds_on_device"] == 1
        assert on_host.update(mesh, model_matrix=Ms, stats=True)["bounds_on_device"] == 0
        for which in range(3):
            a, b = on_dev.records(which), on_host.records(which)
            assert a.shape == b.shape and np.array_equal(a, b), (name, step, which, int((a != b).sum()))
        assert on_dev.validate_bvh() == on_host.validate_bvh()
        assert on_dev.tree_cost() == on_host.tree_cost()


@pytest.fixture(scope="module")
def bunny_pair(rt):
    """(arrays, the moved mesh, a fresh scene of it): what the features below are compared against."""
    arr, _, seq = U.scene_steps(rt, "bunny")
    mesh = U.mesh_of(rt, arr, seq[1])
    return arr, mesh, rt.Scene(mesh)


def updated_bunny(rt, bunny_pair, **kw):
    arr, mesh, _ = bunny_pair
    sc = rt.Scene(U.mesh_of(rt, arr), **kw)
    return sc, mesh


def test_light_set_made_before_the_update(rt, bunny_pair):
    sc, mesh = updated_bunny(rt, bunny_pair)
    fresh = bunny_pair[2]
    lights = [((np.cos(k), np.sin(k), 1.0), (0.02, 0.03, 0.025)) for k in range(40)]  # more than the 32 kernel-argument lights
    ls = sc.light_set(lights)
    sc.update(mesh)
    cam = rt.flycam(W, H, 0, 0, 20)
    got = sc.render_lit(cam, ls, W, H, mode=rt.RT_MODE_FULL, want_hits=True)
    want = fresh.render_lit(cam, fresh.light_set(lights), W, H, mode=rt.RT_MODE_FULL, want_hits=True)
    for part, a, b in zip(("rgb", "face", "t"), got[:3], want[:3]):
        identical(a, b, f"light set {part}")


def test_views_supersampling_and_wavefront_after_an_update(rt, bunny_pair):
    sc, mesh = updated_bunny(rt, bunny_pair)
    fresh = bunny_pair[2]
    cams = [rt.flycam(W, H, dx, 0, 20) for dx in (-2.0, 0.0, 2.0)]
    before = sc.render_views(cams, rt.DEFAULT_LIGHTS, W, H, mode=rt.RT_MODE_FULL, want_hits=True)  # the view scratch exists
    sc.render_ss(cams[1], rt.DEFAULT_LIGHTS, W, H, (2, 2))
    o, d = dev(RAYS[0]), dev(RAYS[1])
    sc.trace_stream_color(o, d, rt.DEFAULT_LIGHTS, wavefront=True)
    sc.update(mesh)
    got = sc.render_views(cams, rt.DEFAULT_LIGHTS, W, H, mode=rt.RT_MODE_FULL, want_hits=True)
    want = fresh.render_views(cams, rt.DEFAULT_LIGHTS, W, H, mode=rt.RT_MODE_FULL, want_hits=True)
    for k in want:
        identical(got[k].cpu().numpy(), want[k].cpu().numpy(), f"view batch {k}")
    assert not np.array_equal(before["t"].cpu().numpy(), got["t"].cpu().numpy())
    identical(sc.render_ss(cams[1], rt.DEFAULT_LIGHTS, W, H, (2, 2), mode=rt.RT_MODE_FULL),
              fresh.render_ss(cams[1], rt.DEFAULT_LIGHTS, W, H, (2, 2), mode=rt.RT_MODE_FULL), "supersampled frame")
    for reorder in (False, True):
        a = sc.trace_stream_color(o, d, rt.DEFAULT_LIGHTS, wavefront=True, reorder=reorder, max_depth=3)
        b = fresh.trace_stream_color(o, d, rt.DEFAULT_LIGHTS, wavefront=True, reorder=reorder, max_depth=3)
        for k in b:
            identical(a[k].cpu().numpy(), b[k].cpu().numpy(), f"wavefront colour {k}")


def test_update_behind_frames_in_flight(rt, bunny_pair):
    """Four rt_render_async frames, then the update with no synchronise in between, then a render."""
    sc, mesh = updated_bunny(rt, bunny_pair, frames_in_flight=4)
    fresh = bunny_pair[2]
    Wb, Hb = 640, 360
    for k in range(4):
        sc.render_async(rt.flycam(Wb, Hb, 0.5 * k, 0, 20), rt.DEFAULT_LIGHTS, Wb, Hb, mode=rt.RT_MODE_FULL)
    sc.update(mesh)
    same_frames(frames(rt, sc, "bunny"), frames(rt, fresh, "bunny"), "after frames in flight")
    sc.synchronize()


def test_update_waits_for_lists_on_caller_streams(rt, bunny_pair):
    """Lists enqueued on a caller's stream return at once and read the scene's records until their kernels end: an
    in-order list (no scratch, no scratch event), a reordered one and a wavefront one, each followed by an update
    with nothing in between, give the bits of the scene before the update."""
    arr, mesh, _ = bunny_pair
    sc = rt.Scene(U.mesh_of(rt, arr))
    reps = 256  # 1M rays: the list kernels run for milliseconds
    o, d = dev(np.tile(RAYS[0], (reps, 1))), dev(np.tile(RAYS[1], (reps, 1)))
    side = torch.cuda.Stream()
    cases = [dict(reorder=False), dict(reorder=True), dict(wavefront=True)]
    meshes = [mesh, U.mesh_of(rt, arr), mesh]
    for kw, after in zip(cases, meshes):
        want = {k: v.cpu().numpy() for k, v in sc.trace_stream_color(o, d, rt.DEFAULT_LIGHTS, max_depth=4, **kw).items()}
        want_c = {k: v.cpu().numpy() for k, v in sc.trace_stream(Q_CLOSEST, o, d, reorder=kw.get("reorder", False)).items()}
        torch.cuda.synchronize()
        got = sc.trace_stream_color(o, d, rt.DEFAULT_LIGHTS, max_depth=4, stream=side, **kw)
        got_c = sc.trace_stream(Q_CLOSEST, o, d, reorder=kw.get("reorder", False), stream=side)
        sc.update(after)
        side.synchronize()
        for k in want:
            identical(got[k].cpu().numpy(), want[k], f"list before the update {kw} {k}")
        for k in want_c:
            identical(got_c[k].cpu().numpy(), want_c[k], f"closest list before the update {kw} {k}")


def test_nan_vertex_on_a_device_scene(rt):
    """One NaN coordinate: the host refit, then the three record images uploaded again (no kernel); and back."""
    arr = U.scene_arrays(rt, "cornell")
    mesh0 = U.mesh_of(rt, arr)
    M = mesh0.export()["M16"]  # (the loader's normalisation of a NaN extent is no matrix to test with)
    sc = rt.Scene(mesh0)
    first = frames(rt, sc, "cornell")
    v = U.deform(arr[0], U.AMPLITUDES[0])
    v[5, 1] = np.nan
    mesh = U.mesh_of(rt, arr, v)
    assert sc.update(mesh, model_matrix=M, stats=True)["bounds_on_device"] == 0
    fresh = rt.Scene(mesh, shape_model_matrix=M)
    got = frames(rt, sc, "cornell")
    same_frames(got, frames(rt, fresh, "cornell"), "NaN vertex")
    same_traces(traces(rt, sc), traces(rt, fresh), "NaN vertex")
    assert (got["primary"][1] >= 0).mean() >= 0.2
    assert sc.update(mesh0, stats=True)["bounds_on_device"] == 1
    same_frames(frames(rt, sc, "cornell"), first, "back from the NaN vertex")


def test_box_colours_after_an_update(rt, bunny_pair):
    sc, mesh = updated_bunny(rt, bunny_pair)
    fresh = bunny_pair[2]
    cam = rt.flycam(W, H, 0, 0, 20)
    sc.set_box_colors()
    sc.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=rt.RT_MODE_BOX_COLORS)
    n_before = sc.info()["n_ref_boxes"]
    sc.update(mesh)
    assert sc.info()["n_ref_boxes"] == fresh.info()["n_ref_boxes"] != n_before
    sc.set_box_colors()
    fresh.set_box_colors()
    got = sc.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=rt.RT_MODE_BOX_COLORS, want_hits=True)
    want = fresh.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=rt.RT_MODE_BOX_COLORS, want_hits=True)
    for part, a, b in zip(("rgb", "face", "t"), got[:3], want[:3]):
        identical(a, b, f"box colours {part}")


def test_two_replicas_on_one_gpu(rt, bunny_pair):
    sc, mesh = updated_bunny(rt, bunny_pair, devices=[0, 0])
    fresh = bunny_pair[2]
    frames(rt, sc, "bunny")
    sc.update(mesh)
    same_frames(frames(rt, sc, "bunny"), frames(rt, fresh, "bunny"), "two replicas")
    sc.update(U.mesh_of(rt, bunny_pair[0]))
    same_frames(frames(rt, sc, "bunny"), frames(rt, rt.Scene(U.mesh_of(rt, bunny_pair[0])), "bunny"), "two replicas, back")


def test_save_and_load_an_updated_scene(rt, bunny_pair, tmp_path):
    sc, mesh = updated_bunny(rt, bunny_pair)
    sc.update(mesh)
    path = str(tmp_path / "updated.rtscene")
    sc.save(path)
    loaded = rt.Scene.load(path)
    same_frames(frames(rt, loaded, "bunny"), frames(rt, bunny_pair[2], "bunny"), "saved and loaded")
    assert loaded.validate_bvh()["ok"]
