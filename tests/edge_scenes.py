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


# ---- mesh edges: odd vertex normals and degenerate faces (tests/test_mesh_edges_host.py holds on the oracle that
# they reach calculateDistance's norm() == 0 rejection; tests/test_gpu_mesh_edges.py holds the kernels to it) ----
NORMAL_N = 16                          # quads per side of the normal scene's front grid
NORMAL_CLASSES = "PPNNZZZTTSSXXUUPP"   # class of a front vertex by its column i = id % 17
NORMAL_PLANE_Z = 0.375                 # world z of the front grid (the back grid at -0.375), as in the tie scene


def _class_normals():
    t, u = np.radians(70.0), np.radians(50.0)
    return {"P": (0.0, 0.0, 1.0), "N": (0.0, 0.0, -1.0), "Z": (0.0, 0.0, 0.0), "T": (np.sin(t), 0.0, np.cos(t)),
            "S": (0.0, 0.0, 3.5), "X": (np.nan, 0.0, 1.0), "U": (0.0, np.sin(u), np.cos(u))}


def normal_scene():
    """A 16x16 quad grid (512 half-quad faces, 17x17 vertices) in the plane z = 0 in front of a 2x2 grid at
    z = -0.75 (normalisation exactly scale 1, translation (0, 0, 0.375)), with explicit vertex normals: the back
    grid's are (0, 0, 1); a front vertex takes its class from its column (NORMAL_CLASSES): P (0,0,1), N (0,0,-1),
    Z the zero vector, T a unit vector 70 degrees from +z towards +x, S (0,0,3.5), X (NaN,0,1), U a unit vector
    50 degrees from +z towards +y. Where a face's interpolated normal is exactly zero (all-Z faces, the P|N faces
    where the weights cancel, the Z|T faces on edges that only Z vertices weigh in) the reference rejects the hit
    and the ray goes on to the back grid. Returns the mesh arrays, vn3 [nv,3] and cls [289] (one character per
    front vertex)."""
    v0, f0 = _grid(NORMAL_N, 0.0)
    v1, f1 = _grid(2, -0.75)
    v = np.concatenate([v0, v1]).astype(F)
    f = np.concatenate([f0, f1 + len(v0)]).astype(np.uint32)
    cls = np.array([NORMAL_CLASSES[i % (NORMAL_N + 1)] for i in range(len(v0))])
    table = _class_normals()
    vn = np.array([table[c] for c in cls] + [table["P"]] * len(v1), np.float64).astype(F)
    return (v, f, np.array([MATERIAL], F), [(len(f), 0)]), vn, cls


def normal_lattice_rays():
    """d = (0, 0, -1) from z = 2 at every pair of the 65 coordinates k / 64 - 0.5 (4,225 rays): hit points exactly
    on the front grid's vertices, edges and cell midlines."""
    c = (np.arange(65, dtype=F) / F(64) - F(0.5)).astype(F)
    x, y = np.meshgrid(c, c, indexing="xy")
    o = np.stack([x.reshape(-1), y.reshape(-1), np.full(x.size, 2.0)], 1).astype(F)
    d = np.zeros_like(o)
    d[:, 2] = -1.0
    return o, d


def normal_random_rays(n=4096, seed=5):
    """Origins uniform in [-0.8, 0.8]^2 x [0.8, 1.5], aimed at uniform points of [-0.49, 0.49]^2 in the front
    grid's plane."""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-0.8, 0.8, n), rng.uniform(-0.8, 0.8, n), rng.uniform(0.8, 1.5, n)], 1)
    tgt = np.stack([rng.uniform(-0.49, 0.49, n), rng.uniform(-0.49, 0.49, n), np.full(n, NORMAL_PLANE_Z)], 1)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(F), d.astype(F)


def normal_shadow_rays(n=2048, seed=5):
    """shadow(P, L) from just above the back grid straight up through the front grid: P uniform in
    [-0.45, 0.45]^2 at z = -0.375 + 1e-3, L = (0, 0, 1)."""
    rng = np.random.default_rng(seed)
    P = np.stack([rng.uniform(-0.45, 0.45, n), rng.uniform(-0.45, 0.45, n), np.full(n, -NORMAL_PLANE_Z + 1e-3)], 1)
    L = np.zeros((n, 3))
    L[:, 2] = 1.0
    return P.astype(F), L.astype(F)


DEGENERATE_PER_KIND = 6


def degenerate_faces(v, f, vn3=None, n=NORMAL_N, seed=7):
    """The mesh (vertices whose first (n+1)^2 rows are a _grid(n, .) lattice, faces, optional vertex normals)
    with 4 x DEGENERATE_PER_KIND zero-area faces spread through the face list (the other faces keep their
    relative order): (a, a, b) and (a, a, a) with a repeated index; three collinear lattice vertices of one
    row; and two coincident vertices, for which a copy of the lattice's first row (with its normals) is appended
    to the vertices. Every one has the face normal (0, 0, 0), cross products that are exactly zero and a box of no
    extent in at least one axis. Returns v, f, vn3 (None if not given), added [24] (the new faces' ids) and
    new_id [len(f)] (where each face of the input went)."""
    rng = np.random.default_rng(seed)
    v = np.asarray(v, F)
    f = np.asarray(f, np.uint32)
    nv, row = len(v), n + 1
    dup = nv + np.arange(row)
    v2 = np.concatenate([v, v[:row]]).astype(F)
    vn2 = None if vn3 is None else np.concatenate([np.asarray(vn3, F), np.asarray(vn3, F)[:row]]).astype(F)
    new = []
    for k in range(DEGENERATE_PER_KIND):
        a, b = (int(x) for x in rng.choice(row * row, 2, replace=False))
        new.append((a, a, b) if k % 2 == 0 else (a, b, b))
        new.append((a, a, a))
        j, i = int(rng.integers(0, row)), int(rng.integers(0, row - 2))
        new.append((j * row + i, j * row + i + 1, j * row + i + 2))
        i = int(rng.integers(0, row - 1))
        new.append((i, int(dup[i]), row + i + 1) if k % 2 == 0 else (int(dup[i]), i + 1, i))
    new = np.array(new, np.uint32)
    total = len(f) + len(new)
    added = np.sort(rng.permutation(total)[:len(new)])
    is_new = np.zeros(total, bool)
    is_new[added] = True
    f2 = np.empty((total, 3), np.uint32)
    f2[is_new] = new
    f2[~is_new] = f
    return v2, f2, vn2, added.astype(np.int64), np.flatnonzero(~is_new)


MICRO_EXPONENTS = tuple(range(8, 45))  # edge lengths 2^-8 .. 2^-44
MICRO_PLANE_Z = 0.25                   # world z of the fan (object z = 0; the backdrop at object z = -0.5)


def micro_fan_scene():
    """37 triangles around the origin, triangle k in its own sector of the plane z = 0 with edges of about
    2^-e, e = 8 .. 44 (O, 2^-e u(phi), 2^-e u(phi + 0.12)), in front of one unit-sized triangle at z = -0.5 (the
    normalisation is scale 1, translation (0, 0, 0.25): x and y are kept exactly, so the small edges survive).
    Below about 2^-37 the squared cross products underflow: the area A, the sub-areas and Eigen's squaredNorm
    become denormal and then zero. The vertex normals are the loader's own. Face e - 8 is the triangle of size
    2^-e; the last face is the backdrop. Returns the mesh arrays."""
    vs, fs = [(0.0, 0.0, 0.0)], []
    for k, e in enumerate(MICRO_EXPONENTS):
        phi = 2 * np.pi * k / len(MICRO_EXPONENTS)
        s = 2.0 ** -e
        vs += [(s * np.cos(phi), s * np.sin(phi), 0.0), (s * np.cos(phi + 0.12), s * np.sin(phi + 0.12), 0.0)]
        fs.append((0, 2 * k + 1, 2 * k + 2))
    b = len(vs)
    vs += [(-0.5, -0.5, -0.5), (0.5, -0.5, -0.5), (0.0, 0.5, -0.5)]
    fs.append((b, b + 1, b + 2))
    f = np.array(fs, np.uint32)
    return np.array(vs, np.float64).astype(F), f, np.array([MATERIAL], F), [(len(f), 0)]


def micro_fan_rays():
    """Rays at every fan triangle's centroid and three edge midpoints (float64 means of the float32 world
    vertices, rounded once): straight down (d = (0, 0, -1)) from distance 1, and along (0.6, 0, -0.8) from 4 edge
    lengths away. Returns o [296,3], d [296,3] and tri [296] (the fan triangle aimed at)."""
    v, f, _, _ = micro_fan_scene()
    w = v.astype(np.float64)
    w[:, 2] += MICRO_PLANE_Z
    os_, ds, tri = [], [], []
    for k, e in enumerate(MICRO_EXPONENTS):
        p = w[f[k]]
        tg = [p.mean(0), (p[0] + p[1]) / 2, (p[1] + p[2]) / 2, (p[2] + p[0]) / 2]
        for dirn, dist in (((0.0, 0.0, -1.0), 1.0), ((0.6, 0.0, -0.8), 4 * 2.0 ** -e)):
            dirn = np.array(dirn)
            for t in tg:
                os_.append(t - dist * dirn)
                ds.append(dirn)
                tri.append(k)
    return np.array(os_).astype(F), np.array(ds).astype(F), np.array(tri, np.int32)


def area_f32(w0, w1, w2):
    """norm(cross(e0, -e2)) / 2 with e0 = w1 - w0, e2 = w0 - w2 in float32, in Eigen's order (cross by
    components, x0 + (x1 + x2) sums): the A of interpolateNormal, of the kernels and of the safe-normal flag."""
    w0, w1, w2 = (np.asarray(x, F) for x in (w0, w1, w2))
    with np.errstate(all="ignore"):
        return (_norm_f32(_cross_f32(w1 - w0, -(w0 - w2))) / F(2)).astype(F)


def _cross_f32(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(F)


def _norm_f32(a):
    return np.sqrt(a[..., 0] * a[..., 0] + (a[..., 1] * a[..., 1] + a[..., 2] * a[..., 2])).astype(F)


def blend_normal_f32(w0, w1, w2, n0, n1, n2, P):
    """interpolateNormal (flyscene.cpp:572-600) in float32 numpy, kernel-independent: the sub-areas of P against
    the world vertices w0..w2 [n,3], (n0 a1 / A + n1 a2 / A) + n2 a0 / A with the normalised vertex normals, and
    Eigen's normalized() (unchanged when the squared norm is not > 0). No inside test: for points that passed it."""
    w0, w1, w2, n0, n1, n2, P = (np.asarray(x, F) for x in (w0, w1, w2, n0, n1, n2, P))
    with np.errstate(all="ignore"):
        e0, e1, e2 = w1 - w0, w2 - w1, w0 - w2
        a0 = _norm_f32(_cross_f32(e0, P - w0)) / F(2)
        a1 = _norm_f32(_cross_f32(e1, P - w1)) / F(2)
        a2 = _norm_f32(_cross_f32(e2, P - w2)) / F(2)
        A = _norm_f32(_cross_f32(e0, -e2)) / F(2)
        s = ((n0 * a1[:, None] / A[:, None] + n1 * a2[:, None] / A[:, None]) + n2 * a0[:, None] / A[:, None]).astype(F)
        z = s[:, 0] * s[:, 0] + (s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2])
        r = np.sqrt(z).astype(F)
        return np.where((z > 0)[:, None], s / r[:, None], s).astype(F)


def normalized_f32(a):
    """Eigen's normalized() per row in float32: a / sqrt(|a|^2), a itself when |a|^2 is not > 0 (zero, NaN)."""
    a = np.asarray(a, F)
    with np.errstate(all="ignore"):
        z = a[:, 0] * a[:, 0] + (a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2])
        return np.where((z > 0)[:, None], a / np.sqrt(z).astype(F)[:, None], a).astype(F)


def soundness_scene(seed):
    """A single 16x16 quad grid in the plane z = 0 (nothing behind it) whose vertex normals are random unit vectors
    at angles uniform in [0, 75] degrees from +z, except a few vertices exactly at the safe-normal flag's boundary
    n . n_k = 0.5: (sqrt(3)/2, 0, 0.5) rounded to float32 and its two float neighbours in z. Returns the mesh
    arrays and vn3."""
    rng = np.random.default_rng(seed)
    v, f = _grid(NORMAL_N, 0.0)
    nv = len(v)
    ang = np.radians(rng.uniform(0.0, 75.0, nv))
    az = rng.uniform(0.0, 2 * np.pi, nv)
    vn = np.stack([np.sin(ang) * np.cos(az), np.sin(ang) * np.sin(az), np.cos(ang)], 1).astype(F)
    edge = np.array([np.sqrt(3.0) / 2, 0.0, 0.5]).astype(F)
    for k, vid in enumerate(rng.choice(nv, 12, replace=False)):
        n = edge.copy()
        if k % 3 == 1:
            n[2] = np.nextafter(F(0.5), F(1.0))
        elif k % 3 == 2:
            n[2] = np.nextafter(F(0.5), F(0.0))
        vn[vid] = n
    return (v, f, np.array([MATERIAL], F), [(len(f), 0)]), vn
