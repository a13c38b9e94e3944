"""Deterministic edge-case inputs for the packet kernels (tests/test_edge_inputs.py holds, on the CPU oracle
alone, that they reach the edges they are built for; tests/test_gpu_edges.py holds the kernels to the oracle
on them). A plain module: fixed seeds, coordinates that are exact binary fractions where stated, and every
direction component either exactly zero or of magnitude >= 1e-12.

Scene builders return mesh arrays (vertices [nv,3] f32, faces [nf,3] u32, materials [nm,12] f32, groups
[(n_faces, mat)]), the arguments of both rtamd.Mesh.from_arrays and oracle.Mesh.from_arrays; the tie-scene
builders return them with a per-face label array.
"""
import numpy as np

F = np.float32
TIE_N = 12            # quads per side of a tie-scene grid
TIE_SLANT = 3         # cells by which the slanted copies' triangles lean (see _strip)
TIE_PLANE_Z = 0.375   # world z of the triple plane (object z = 0; the loader centres z in [-0.75, 0], scale 1)
MATERIAL = [0.1, 0.1, 0.1, 0.7, 0.7, 0.7, 0.2, 0.2, 0.2, 16.0, 1.0, 1.0]


def lattice(n=TIE_N):
    """The n + 1 grid coordinates k / n - 0.5 in fp32, as the tie scene's vertices compute them."""
    return (np.arange(n + 1, dtype=F) / F(n) - F(0.5)).astype(F)


def _strip(bottom, top, lead):
    """Counter-clockwise triangles of the strip between two parallel lattice lines (vertex ids `bottom`, `top`,
    the top line on the left of the bottom line's direction), one per lattice edge: the walk along the top line
    runs `lead` edges ahead of the bottom one, so lead 0 gives the usual half-quads and lead 3 slanted triangles
    that span up to four cells."""
    n = len(bottom) - 1
    b = t = 0
    out = []
    while b < n or t < n:
        if t < n and (t - b < lead or b == n):
            out.append((bottom[b], top[t + 1], top[t]))
            t += 1
        else:
            out.append((bottom[b], bottom[b + 1], top[t]))
            b += 1
    return out


def _grid(n, z, cut=0):
    """(n+1)^2 lattice vertices in the plane z and 2 n^2 counter-clockwise triangles on them. cut 0: half-quads;
    1: rows of triangles slanted along x; 2: columns of triangles slanted along y."""
    c = lattice(n)
    xx, yy = np.meshgrid(c, c, indexing="xy")
    v = np.stack([xx.reshape(-1), yy.reshape(-1), np.full(xx.size, z, F)], 1).astype(F)
    vid = np.arange((n + 1) ** 2).reshape(n + 1, n + 1)  # [row j (y), column i (x)]
    f = []
    for k in range(n):
        if cut == 2:
            f += _strip(vid[:, k + 1], vid[:, k], TIE_SLANT)
        else:
            f += _strip(vid[k, :], vid[k + 1, :], TIE_SLANT if cut == 1 else 0)
    return v, np.array(f, np.uint32)


def tie_scene(seed=5):
    """Three coincident copies of a 12x12 quad grid (288 triangles each) in the plane z = 0, each with its own
    vertex block, its own face order and its own cut of the lattice into triangles (half-quads, slanted along x,
    slanted along y: coincident faces then have different extents, and the reference's box partition, which
    keeps a face in a box only with all three vertices, puts them into different boxes -- with the same cut in
    every copy coincident faces always share a box, where the in-box order is the face-id order), plus one 2x2 grid at z = -0.75 (a three-dimensional extent: the loader's
    normalisation is then scale 1, centre (0, 0, -0.375), exact in fp32); the whole face list permuted again.
    Every face of the plane has the unit normal (0, 0, 1) exactly, so every ray through the plane meets three
    faces at bit-identical t. Returns the mesh arrays and copy_of_face [nf] (0..2 the copies, 3 the back grid)."""
    rng = np.random.default_rng(seed)
    vs, fs, copy = [], [], []
    base = 0
    for k in range(3):
        v, f = _grid(TIE_N, 0.0, cut=k)
        vs.append(v)
        fs.append(f[rng.permutation(len(f))] + base)
        copy.append(np.full(len(f), k))
        base += len(v)
    v, f = _grid(2, -0.75)
    vs.append(v)
    fs.append(f + base)
    copy.append(np.full(len(f), 3))
    v, f, copy = np.concatenate(vs), np.concatenate(fs), np.concatenate(copy)
    perm = rng.permutation(len(f))
    f, copy = f[perm], copy[perm]
    return (v.astype(F), f.astype(np.uint32), np.array([MATERIAL], F), [(len(f), 0)]), copy


def tie_copy_scene(k, seed=5):
    """The tie scene without the other two copies' faces (all vertices kept, so the normalisation is the
    same): copy k and the back grid, in the tie scene's face order. Returns the mesh arrays and face_id [n],
    the tie scene's id of every face kept."""
    (v, f, mats, _), copy = tie_scene(seed)
    keep = np.flatnonzero((copy == k) | (copy == 3))
    return (v, f[keep], mats, [(len(keep), 0)]), keep


# shininess of the material scene's ten materials: the pow fast path's bounds (0, 1023, 1024), small integers,
# non-integer exponents (the library pow), 324 (the .mtl files' 323.999994 in fp32) and two large ones
MATERIAL_NS = [0.0, 1.0, 0.5, 2.5, 16.0, 324.0, 1023.0, 1024.0, 1e4, 100.25]
MATERIAL_TRIS = 55    # per group; 11 groups
MATERIAL_CAMERA = (64, 40, 0.0, 0.0, 20.0)  # flycam(W, H, dx, dy, dz): the eye at (0, 0, 1)


def material_scene(seed=9):
    """605 small triangles scattered on a sphere of radius 0.4, in 11 groups of 55 that interleave over the
    whole sphere: ten materials (MATERIAL_NS, each with its own colours, all with a specular term) and a last
    group with material id -1 (the frame's default material)."""
    rng = np.random.default_rng(seed)
    ng = len(MATERIAL_NS) + 1
    n = MATERIAL_TRIS * ng
    c = rng.normal(size=(n, 3))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    # two tangents per triangle, edge about 0.07
    a = np.cross(c, rng.normal(size=(n, 3)))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = np.cross(c, a)
    ang = rng.uniform(0, 2 * np.pi, (n, 1))
    r = 0.05
    v = np.empty((n, 3, 3))
    for k in range(3):
        th = ang + 2 * np.pi * k / 3
        p = c + r * (np.cos(th) * a + np.sin(th) * b)
        v[:, k] = 0.4 * p / np.linalg.norm(p, axis=1, keepdims=True)
    v = v.reshape(-1, 3).astype(F)
    f = np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)
    mats = []
    for k, ns in enumerate(MATERIAL_NS):
        ka = [0.05 + 0.01 * k, 0.10, 0.15 - 0.01 * k]
        kd = [0.3 + 0.05 * k, 0.6 - 0.03 * k, 0.4]
        ks = [0.5, 0.3 + 0.02 * k, 0.25]
        mats.append(ka + kd + ks + [ns, 1.0, 1.0])
    groups = [(MATERIAL_TRIS, k) for k in range(len(MATERIAL_NS))] + [(MATERIAL_TRIS, -1)]
    return v, f, np.array(mats, F), groups


def ring_lights(n, colour=0.05):
    """n point lights on two rings around the z axis in front of the scene, colours <= `colour` per channel."""
    out = []
    for k in range(n):
        th = 2 * np.pi * k / max(n, 1)
        rad, z = (2.0, 2.5) if k % 2 == 0 else (0.8, 1.5)
        out.append(((float(F(rad * np.cos(th))), float(F(rad * np.sin(th))), z),
                    (colour, colour * (0.6 + 0.4 * (k % 3) / 2), colour * (1.0 - 0.5 * (k % 4) / 3))))
    return out


def _signed_zero(d):
    """Zero components +0.0 in the even rays and -0.0 in the odd ones."""
    d = d.astype(F).copy()
    odd = (np.arange(len(d)) % 2 == 1)[:, None]
    return np.where((d == 0) & odd, F(-0.0), d).astype(F)


def axis_rays(cu, cv, cw_side, starts):
    """Axis-aligned rays d = +-e_k for every axis k and sign s: origins at -s * start along k for every start in
    `starts[k]` (positive = before the scene, 0.5 = on the near plane of a unit box, negative = past the centre)
    and at every pair of the lattice coordinates in the other two axes -- (cu, cv) for rays along z, and (cu or
    cv, cw_side) for rays along x and y, cw_side being the z coordinates of the side rays. Returns o [n,3],
    d [n,3] (zero components of both signs) and axis_dir [n] = 2 k + (1 if d = -e_k)."""
    os_, ds, ad = [], [], []
    for k in range(3):
        for s in (1.0, -1.0):
            for start in starts[k]:
                if k == 2:
                    u, v = np.meshgrid(cu, cv, indexing="xy")
                    o = np.stack([u.reshape(-1), v.reshape(-1), np.full(u.size, -s * start)], 1)
                else:
                    u, w = np.meshgrid(cu if k == 1 else cv, cw_side, indexing="xy")
                    o = np.empty((u.size, 3))
                    o[:, k] = -s * start
                    o[:, 1 - k] = u.reshape(-1)
                    o[:, 2] = w.reshape(-1)
                d = np.zeros((len(o), 3))
                d[:, k] = s
                os_.append(o)
                ds.append(d)
                ad.append(np.full(len(o), 2 * k + (s < 0)))
    o = np.concatenate(os_).astype(F)
    d = _signed_zero(np.concatenate(ds))
    return o, d, np.concatenate(ad).astype(np.int32)


def tie_lattice_rays():
    """Axis-aligned rays at the tie scene's vertex coordinates (so also on reference-box planes, boxes being
    fitted to vertices): along z through every grid vertex, from outside, from exactly on either grid's plane and
    from between them; along x and y at the world z of the triple plane (in-plane, grazing), of the back grid and
    at two heights between, from outside, from the scene's bounding planes and from the centre."""
    c = lattice()
    side = (1.0, 0.5, 0.0)
    return axis_rays(c, c, np.array([TIE_PLANE_Z, -0.375, 0.0, 0.25], F), (side, side, (1.0, TIE_PLANE_Z, 0.0, -0.375)))


def cube_lattice_rays():
    """Axis-aligned rays on the 11x11 lattice of multiples of 1/8 in [-0.625, 0.625] (the normalised cube spans
    [-0.5, 0.5]^3), 40 of the 121 exactly in a face plane of the cube; each from outside, from exactly on the
    near face's plane, from the centre plane and from exactly on the far face's plane."""
    c = (np.arange(-5, 6, dtype=F) / F(8)).astype(F)
    st = (1.0, 0.5, 0.0, -0.5)
    return axis_rays(c, c, c, (st, st, st))


def tie_random_rays(n=4096, seed=21):
    """Rays from above and below through random points of the triple plane."""
    rng = np.random.default_rng(seed)
    tgt = np.stack([rng.uniform(-0.49, 0.49, n), rng.uniform(-0.49, 0.49, n), np.full(n, TIE_PLANE_Z)], 1)
    o = np.stack([rng.uniform(-0.8, 0.8, n), rng.uniform(-0.8, 0.8, n),
                  np.where(np.arange(n) % 4 == 0, -0.9, 1.0) * rng.uniform(0.8, 1.2, n)], 1)
    # the rays from below start between the two grids
    o[:, 2] = np.where(o[:, 2] < 0, rng.uniform(-0.3, 0.2, n), o[:, 2])
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(F), d.astype(F)


def on_plane_rays(n=2048, seed=22):
    """Origins exactly on the triple plane (world z = 0.375). Directions: random (first half), +-e_z (next
    quarter), in-plane with d_z exactly zero of either sign (last quarter). Returns o, d, kind (0 / 1 / 2)."""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-0.45, 0.45, n), rng.uniform(-0.45, 0.45, n), np.full(n, TIE_PLANE_Z)], 1).astype(F)
    d = rng.normal(size=(n, 3))
    kind = np.zeros(n, np.int32)
    q = n // 4
    kind[2 * q:3 * q] = 1
    kind[3 * q:] = 2
    d[kind == 1] = np.array([0.0, 0.0, 1.0]) * np.where(np.arange(q) % 2 == 0, 1.0, -1.0)[:, None]
    d[kind == 2, 2] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(F)
    small = (d != 0) & (np.abs(d) < 1e-12)
    assert not small.any()
    return o, _signed_zero(d), kind


def shadow_straddle_rays(n=1536, seed=23):
    """shadow(P, L) with L pointing up through the triple plane and P below it by 0.5x, 1x and 1.5x of
    0.003 |L_z|: the reference tests triangles from P + 0.003 L (above, about on, below the plane) while its box
    test still starts at P."""
    rng = np.random.default_rng(seed)
    L = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n), rng.uniform(0.3, 1.0, n)], 1)
    L /= np.linalg.norm(L, axis=1, keepdims=True)
    L = L.astype(F)
    frac = np.array([0.5, 1.0, 1.5], F)[np.arange(n) % 3]
    P = np.stack([rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n), np.zeros(n)], 1).astype(F)
    P[:, 2] = F(TIE_PLANE_Z) - frac * (F(0.003) * np.abs(L[:, 2]))
    return P, L


def zero_direction_rays():
    """d = (0, 0, 0) with zeros of both signs, from origins above, on and below the triple plane."""
    o = np.array([[0.1, 0.2, 1.0], [0.0, 0.0, TIE_PLANE_Z], [-0.25, 0.25, 0.0], [0.3, -0.3, -1.0]] * 2, F)
    d = np.zeros((8, 3), F)
    d[4:] = F(-0.0)
    return o, d


def ref_slab_nan(boxes6, M16, o, d):
    """Per ray: does the reference's intersectBox arithmetic (lo - o2) / d2, (hi - o2) / d2 produce a NaN for any
    box? o2 = M^-1 o, d2 = normalized(M^-1 d) with the exported model matrix (column-major 4x4)."""
    M = np.asarray(M16, np.float64).reshape(4, 4).T
    Mi = np.linalg.inv(M)
    o2 = (np.asarray(o, np.float64) @ Mi[:3, :3].T + Mi[:3, 3]).astype(F)
    d2 = np.asarray(d, np.float64) @ Mi[:3, :3].T
    nrm = np.linalg.norm(d2, axis=1, keepdims=True)
    d2 = np.where(nrm > 0, d2 / np.where(nrm > 0, nrm, 1.0), d2).astype(F)
    b = np.asarray(boxes6, F)
    with np.errstate(all="ignore"):
        lo = (b[None, :, 0:3] - o2[:, None, :]) / d2[:, None, :]
        hi = (b[None, :, 3:6] - o2[:, None, :]) / d2[:, None, :]
    return (np.isnan(lo) | np.isnan(hi)).any(axis=(1, 2))
