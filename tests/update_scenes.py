"""Scenes and deformations of the scene-update tests (tests/test_scene_update_host.py, tests/test_gpu_scene_update.py):
every scene as mesh arrays that Mesh.from_arrays re-ingests after its vertices have moved, a seeded smooth
displacement, and the sequence small amplitude -> large amplitude -> back to the original vertices.
tools/scene_update_ab.py measures with the same obj_arrays / deform / mesh_of, so this module imports only numpy at
the top (the test-only helpers import tests/edge_scenes.py and tests/conftest.py where they need them)."""
import numpy as np

F = np.float32

# amplitudes of the deformation sequence, as fractions of the mesh's largest extent. Chosen on host-only scenes
# (the tests assert what they were chosen for): on the bunny both steps change the reference-box partition's
# face order, and at dz = 20 more than 20% of a 96x64 frame's pixels still hit.
AMPLITUDES = (0.02, 0.15)
W, H = 96, 64
# flycam dz per scene: more than 20% of the frame hits at every step (the material scene's small triangles are
# sparse: the camera moves closer; measured with the CPU oracle 0.23-0.25, the bunny 0.33-0.40, cornell 0.77-0.91)
CAMERA_DZ = {"cornell": 20.0, "tie": 20.0, "material": 26.0, "bunny": 20.0}
SCENES = ("cornell", "tie", "material", "bunny")


def scene_steps(rt, name):
    """(arrays, model matrix to keep or None, [vertex arrays of the sequence])."""
    arr = scene_arrays(rt, name)
    if name == "tie":
        return arr, mesh_of(rt, arr).export()["M16"], tie_steps(arr)
    return arr, None, steps(arr)


def obj_arrays(rt, path):
    """The OBJ file at `path` as from_arrays input: (v3, faces, materials12, groups)."""
    ex = rt.Mesh.load_obj(path).export()
    fmat = ex["fmat"]
    cuts = np.flatnonzero(np.diff(fmat)) + 1
    starts = np.concatenate([[0], cuts])
    ends = np.concatenate([cuts, [len(fmat)]])
    groups = [(int(e - s), int(fmat[s])) for s, e in zip(starts, ends)]
    return ex["v4"][:, :3].astype(F), ex["fidx"].astype(np.uint32), ex["mats"], groups


def scene_arrays(rt, name):
    import edge_scenes as E
    from conftest import scene_path
    if name == "tie":
        return E.tie_scene()[0]
    if name == "material":
        return E.material_scene()
    return obj_arrays(rt, scene_path(name + ".obj"))


def deform(v3, amplitude, seed=3):
    """v3 displaced along a seeded direction by a sine along a seeded axis: amplitude * extent * sin(2 pi k x + phase)."""
    if amplitude == 0:
        return v3.copy()
    rng = np.random.default_rng(seed)
    v = v3.astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    ext = float((hi - lo).max())
    axis = int(rng.integers(3))
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    phase = rng.uniform(0, 2 * np.pi)
    s = np.sin(2 * np.pi * 1.5 * (v[:, axis] - lo[axis]) / max(hi[axis] - lo[axis], 1e-30) + phase)
    return (v + amplitude * ext * s[:, None] * d[None, :]).astype(F)


def mesh_of(rt, arrays, v3=None):
    v, f, mats, groups = arrays
    return rt.Mesh.from_arrays(v if v3 is None else v3, f, mats, groups=groups)


def steps(arrays):
    """The deformation sequence's vertex arrays: small, large, back to the original."""
    v = arrays[0]
    return [deform(v, AMPLITUDES[0]), deform(v, AMPLITUDES[1]), v.copy()]


TIE_SHIFTS = ((0.0625, 0.03125, 0.0), (-0.25, 0.125, -0.125))


def tie_steps(arrays):
    """The tie scene's sequence: rigid shifts (the model matrix is kept by the caller), so the three coincident
    copies stay coincident -- the same fp32 sum at every shared lattice position -- and the rank still decides."""
    v = arrays[0]
    return [(v + np.array(s, F)[None, :]).astype(F) for s in TIE_SHIFTS] + [v.copy()]


def tie_copies_coincide(v3):
    """The three copies' vertex blocks ((TIE_N + 1)^2 vertices each, the same lattice order) are bit-equal."""
    import edge_scenes as E
    n = (E.TIE_N + 1) ** 2
    return bool(np.array_equal(v3[:n], v3[n:2 * n]) and np.array_equal(v3[:n], v3[2 * n:3 * n]))


def rotated_stretched(M16):
    """A column-major model matrix rotated (0.5 rad about z, 0.3 about x) and stretched (1.3, 1, 0.8) in world
    space: no similarity, so normals tilt against their world triangles and nothing is certified."""
    M = np.asarray(M16, np.float64).reshape(4, 4).T
    c, s = np.cos(0.5), np.sin(0.5)
    Rz = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    c, s = np.cos(0.3), np.sin(0.3)
    Rx = np.array([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1]])
    A = Rz @ Rx @ np.diag([1.3, 1.0, 0.8, 1.0])
    return (A @ M).T.reshape(16).astype(F)


def rays(n=4096, seed=11):
    """Seeded rays towards the scene: origins on a sphere of radius 2, directions at points near the origin."""
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(n, 3))
    o = 2.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = rng.uniform(-0.45, 0.45, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(F), d.astype(F)
