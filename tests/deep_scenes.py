"""Deterministic inputs for the deep-tree battery: meshes whose PLOC tree (rt_build.hip k_ploc_nn / k_ploc_flags) is
a chain as deep as the traversal stacks allow (adopt_tree, rt_layout.cpp: depth <= kMaxDepth + 2 = 62), cameras and
ray lists that descend the whole chain with the far child pushed at every level, a numpy model of the PLOC
clustering rule, and a numpy walk of a built tree that counts the levels at which a ray needs both children.
tests/test_deep_inputs.py holds on the CPU that these inputs reach what they are built for;
tests/test_gpu_deep_trees.py holds the kernels to the oracle on them. A plain module with fixed seeds.

Scene builders return mesh arrays (vertices [nv,3] f32, faces [nf,3] u32, materials [nm,12] f32, groups
[(n_faces, mat)]), the arguments of both rtamd.Mesh.from_arrays and oracle.Mesh.from_arrays.

The spine: shell k is one triangle of size s_k = r^k in the plane z = -s_k / 4, a sliver along a diagonal of the
square |x|, |y| <= 1.5 s_k (corner to the far corner's two neighbours at 1.3 s_k, turned by a quarter per shell, the
whole shell shifted by -0.02 s_k in x and y). Every shell contains the z axis and fills its square's box; the smallest
is nearest a viewer on +z. What makes PLOC chain it, by the rule as the kernels apply it:
  - Morton order. The key is built from the box centre, x the highest bit. The centres (-0.02 s, -0.02 s, -s / 4)
    fall in all three coordinates as s grows, so the Morton order is the size order reversed; the smallest shells
    share a Morton cell and tie to the face slot. Faces are therefore listed from the largest shell to the smallest:
    ties then keep the same order. (With centres that rise in x and y while z falls -- a triangle (-s, -s),
    (2s, -s), (-s, 2s) -- the order interleaves large and small shells and the tree comes out about 18 deep.)
  - Nearest neighbours. Shell k + 1 must prefer the cluster of shells 0..k to shell k + 2. The cluster's box is shell
    k's square with the thickness of everything below it, (s_k - 1) / 4: half area (9 + 6 / 4) s_k^2 at most, against
    (9 r^2 + 6 r (r - 1) / 4) s_k^2 for the pair above -- 10.5 < 11.05 at r = 1.1. With the planes at z = -s_k the
    thickness term is four times as large and the chain breaks at the seventh shell.
Slivers, because the cone of squares is 80 degrees wide: a 60-degree camera near the apex never sees past a square's
edge, but it does see past the slivers, so frames have misses and the nearest sliver under a pixel changes with the
pixel's distance from the centre."""
import numpy as np

F = np.float32
MAX_DEPTH = 62          # kMaxDepth + 2: the deepest tree adopt_tree, rt_scene_create and the cache loader accept
SPINE_R = 1.1
SPINE_N = 62            # the spine whose PLOC chain is MAX_DEPTH deep (61 interior levels + the leaf level)
PAIRS_N = 61            # pairs of coincident shells: 60 chain levels + the pair's node + the leaf level = 62
PLOC_RADIUS = 4         # kPlocRadius (rt_layout.cpp)
FLAT = 0.25             # plane of shell k: z = -FLAT * s_k
SHIFT = 0.02            # every shell shifted by -SHIFT * s_k in x and y
# materials: one with an integer exponent, one with a non-integer one (the library pow); both reflect
MATERIALS = [[0.10, 0.08, 0.06, 0.6, 0.5, 0.4, 0.5, 0.5, 0.5, 16.0, 1.0, 1.0],
             [0.05, 0.07, 0.10, 0.3, 0.5, 0.7, 0.4, 0.3, 0.5, 2.5, 1.0, 1.0]]
MATT = [[0.10, 0.08, 0.06, 0.6, 0.5, 0.4, 0.0, 0.0, 0.0, 16.0, 1.0, 1.0],
        [0.05, 0.07, 0.10, 0.3, 0.5, 0.7, 0.0, 0.0, 0.0, 2.5, 1.0, 1.0]]
# the eye of the chosen frames, in object coordinates (shell 0 has size 1): on the axis side of the apex, in front
EYE_OBJECT = (0.1, 0.05, 1.0)
FRAME = (64, 64)        # the tile-aligned frame: 64 8x8 wave tiles; its 4,096 camera rays are also a ray list
_SLIVER = np.array([(-1.5, -1.5), (1.5, 1.3), (1.3, 1.5)])  # counter-clockwise: the normal is +z


def _shells(n, r, copies):
    """Vertices and faces of shells n-1 .. 0 (largest first), `copies` coincident triangles per shell."""
    v, f = [], []
    for k in range(n - 1, -1, -1):
        s = float(r) ** k
        a = 0.5 * np.pi * (k % 4)
        rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]).round()
        xy = (_SLIVER @ rot.T - SHIFT) * s
        for _ in range(copies):
            b = len(v)
            v += [(x, y, -FLAT * s) for x, y in xy]
            f.append((b, b + 1, b + 2))
    return np.array(v, np.float64).astype(F), np.array(f, np.uint32), len(f)


def spine(n=SPINE_N, r=SPINE_R, reflective=True):
    """n shells, the largest first (face i = shell n - 1 - i, each with its own three vertices), materials
    alternating between the two of MATERIALS (reflective: ks > 0, so FULL frames at depth > 2 keep bouncing
    between the shells) or of MATT."""
    v, f, nf = _shells(n, r, 1)
    return v, f, np.array(MATERIALS if reflective else MATT, F), [(1, i % 2) for i in range(nf)]


def pair_spine(n=PAIRS_N, r=SPINE_R, reflective=True):
    """n shells of two coincident triangles each (faces 2i and 2i + 1; every hit is a tie the reference's rank
    decides). PLOC merges each pair first (the merged box is the triangle's own), then chains the pairs: a
    two-leaf subtree beside every chain link, so the 4-wide collapse absorbs fewer binary levels per wide level
    than on the plain chain."""
    v, f, nf = _shells(n, r, 2)
    return v, f, np.array(MATERIALS if reflective else MATT, F), [(1, (i // 2) % 2) for i in range(nf)]


def shell_of_face(arrays):
    """[nf]: the shell of every face (0 = the smallest)."""
    v, f = arrays[0], arrays[1]
    z = v[f[:, 0], 2].astype(np.float64)
    return np.searchsorted(np.unique(-z), -z)


def world_vertices(export):
    """The mesh's world vertices in float64 from Mesh.export() (v4 and the column-major model matrix)."""
    M = np.asarray(export["M16"], np.float64).reshape(4, 4).T
    return (np.asarray(export["v4"], np.float64) @ M.T)[:, :3]


def world_boxes(export):
    """[nf, 6] lo xyz, hi xyz of every face in world space."""
    w = world_vertices(export)[np.asarray(export["fidx"], np.int64)]
    return np.concatenate([w.min(1), w.max(1)], 1)


def object_point(export, p):
    M = np.asarray(export["M16"], np.float64).reshape(4, 4).T
    return (M @ np.array([p[0], p[1], p[2], 1.0]))[:3]


def camera_args(export, W, H, eye=EYE_OBJECT):
    """flycam(W, H, dx, dy, dz) arguments that put the eye at the world position of the object point `eye`, looking
    down -z (the flycam's eye is (0.05 dx, 0.05 dy, 2 - 0.05 dz))."""
    e = object_point(export, eye)
    return W, H, float(F(e[0] / 0.05)), float(F(e[1] / 0.05)), float(F((2.0 - e[2]) / 0.05))


# ---- ray lists along the spine ----
def forward_rays(export, n=4096, seed=31, half_angle=0.45):
    """Origins in front of the smallest shell (object x, y in [-0.6, 0.6], z in [0, 6]), directions within
    `half_angle` radians of -z: the direction in which, at every chain node, the interior child (the smaller
    shells) is the near one and the leaf is pushed."""
    rng = np.random.default_rng(seed)
    M = np.asarray(export["M16"], np.float64).reshape(4, 4).T
    po = np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n), rng.uniform(0.0, 6.0, n), np.ones(n)], 1)
    o = (po @ M.T)[:, :3]
    th = half_angle * np.sqrt(rng.uniform(0, 1, n))
    ph = rng.uniform(0, 2 * np.pi, n)
    d = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), -np.cos(th)], 1)
    return o.astype(F), d.astype(F)


def reversed_rays(export, o, d):
    """The same lines walked the other way: from behind the largest shell towards +z (the near child is then the
    leaf, nothing stays on the stack)."""
    w = world_vertices(export)
    span = 1.25 * float(w[:, 2].max() - w[:, 2].min()) + 0.05
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    return (o64 + span * d64).astype(F), (-d64).astype(F)


def shadow_segments(export, n=4096, seed=32):
    """shadow(P, L): P just behind shell k (k cycling over the shells) at a point inside the shell's triangle,
    L the unit vector towards a light in front of shell 0 at the object point (0.5, 0.5, 1.5). Segments from
    behind the small shells see little in front of them; from behind the large ones the smaller shells block."""
    rng = np.random.default_rng(seed)
    w = world_vertices(export)[np.asarray(export["fidx"], np.int64)]  # [nf, 3, 3]
    nf = len(w)
    k = np.arange(n) % nf
    bary = rng.dirichlet((1.0, 1.0, 1.0), n)
    P = (w[k] * bary[:, :, None]).sum(1)
    gap = np.abs(np.diff(np.unique(w[:, 0, 2]))).min()
    P[:, 2] -= 0.25 * gap
    light = object_point(export, (0.5, 0.5, 1.5))
    L = light[None, :] - P
    L /= np.linalg.norm(L, axis=1, keepdims=True)
    return P.astype(F), L.astype(F)


def ray_lists(export):
    """{name: (a, b)}: forward (4,096), reversed, shadow (P, L), odd (the first 257 forward rays)."""
    o, d = forward_rays(export)
    return {"forward": (o, d), "reversed": reversed_rays(export, o, d), "shadow": shadow_segments(export),
            "odd": (np.ascontiguousarray(o[:257]), np.ascontiguousarray(d[:257]))}


def boxes_crossed(boxes6, o, d):
    """[n_rays]: how many of the boxes (lo xyz, hi xyz; flat boxes included) the ray o + t d, t >= 0, crosses, by
    the slab test in float64."""
    o = np.asarray(o, np.float64)[:, None, :]
    d = np.asarray(d, np.float64)[:, None, :]
    b = np.asarray(boxes6, np.float64)[None, :, :]
    with np.errstate(all="ignore"):
        inv = 1.0 / d
        t0, t1 = (b[:, :, 0:3] - o) * inv, (b[:, :, 3:6] - o) * inv
    near, far = np.minimum(t0, t1).max(2), np.maximum(t0, t1).min(2)
    return ((near <= far) & (far >= 0)).sum(1)


# ---- the PLOC rule in numpy ----
def _expand10(v):
    v = v & 0x3FF
    v = (v | (v << 16)) & 0x030000FF
    v = (v | (v << 8)) & 0x0300F00F
    v = (v | (v << 4)) & 0x030C30C3
    v = (v | (v << 2)) & 0x09249249
    return v


def _half_area(b):
    e = np.maximum(b[..., 3:6] - b[..., 0:3], 0.0).astype(F)
    return (e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2] + e[..., 2] * e[..., 0]).astype(F)


def ploc_model(boxes6, radius=PLOC_RADIUS):
    """The device PLOC clustering on the faces' world boxes, in float32: Morton order of the box centres (scene box
    quantised to 1024^3, x the highest bit, ties to the face slot), then per iteration every cluster's nearest
    neighbour among the `radius` clusters either side (half surface area of the merged box, the first minimum)
    and a merge of every mutual pair. Returns (merges per iteration, depth of the tree counted as relayout_dfs
    counts it: interior levels + the leaf level, single-leaf children per interior node [n_interior])."""
    b = np.asarray(boxes6, np.float64).astype(F)
    n = len(b)
    lo, hi = b[:, 0:3].min(0), b[:, 3:6].max(0)
    scale = np.where(hi > lo, F(1024.0) / (hi - lo), F(0.0)).astype(F)
    c = (F(0.5) * (b[:, 0:3] + b[:, 3:6])).astype(F)
    q = np.clip(((c - lo) * scale).astype(F), 0.0, 1023.0).astype(np.int64)
    key = (((_expand10(q[:, 0]) << 2) | (_expand10(q[:, 1]) << 1) | _expand10(q[:, 2])) << 32) | np.arange(n)
    order = np.argsort(key, kind="stable")
    single = [True] * n
    boxes = [b[i].copy() for i in order]
    height = [1] * n                                           # levels below and including this cluster's root
    merges, leaf_children = [], []
    while len(boxes) > 1:
        N = len(boxes)
        B = np.stack(boxes)
        nn = np.full(N, -1)
        for i in range(N):
            j0, j1 = max(0, i - radius), min(N - 1, i + radius)
            js = np.array([j for j in range(j0, j1 + 1) if j != i])
            jb = np.concatenate([np.minimum(B[i, 0:3], B[js, 0:3]), np.maximum(B[i, 3:6], B[js, 3:6])], 1)
            nn[i] = js[int(np.argmin(_half_area(jb)))]
        nb, nh, ns, m = [], [], [], 0
        for i in range(N):
            j = nn[i]
            mutual = nn[j] == i
            if mutual and j < i:
                continue
            if mutual:
                nb.append(np.concatenate([np.minimum(boxes[i][0:3], boxes[j][0:3]), np.maximum(boxes[i][3:6], boxes[j][3:6])]))
                nh.append(max(height[i], height[j]) + 1)
                ns.append(False)
                leaf_children.append(int(single[i]) + int(single[j]))
                m += 1
            else:
                nb.append(boxes[i]); nh.append(height[i]); ns.append(single[i])
        boxes, height, single = nb, nh, ns
        merges.append(m)
        assert m > 0
    return merges, height[0], leaf_children


# ---- a built tree, walked in numpy ----
NODE_DTYPE = np.dtype([("box", "<f4", 12), ("child", "<u4", 2), ("pad", "<u4", 2)])
LEAF_BIT = 0x80000000


def parse_nodes(raw, handle_stride):
    """Binary node records (64 bytes each) as a structured array. handle_stride: what an interior child handle
    counts in -- 64 for the device form of rt_debug_scene_records (byte offsets), 1 for the scene cache's nodes
    section (tests/test_host.py NODES: node indices). Returns (boxes [nn, 2, 6] lo xyz hi xyz per child,
    child [nn, 2] node index or -1 for a leaf)."""
    rec = np.frombuffer(bytes(raw), NODE_DTYPE)
    bx = rec["box"].astype(np.float64)
    # child 0: lo.x hi.x lo.y hi.y lo.z hi.z ; child 1 the same, from float 6 (rt_internal.h Node64)
    c0 = np.stack([bx[:, 0], bx[:, 2], bx[:, 4], bx[:, 1], bx[:, 3], bx[:, 5]], 1)
    c1 = np.stack([bx[:, 6], bx[:, 8], bx[:, 10], bx[:, 7], bx[:, 9], bx[:, 11]], 1)
    h = rec["child"].astype(np.int64)
    child = np.where(h & LEAF_BIT, -1, h // handle_stride)
    return np.stack([c0, c1], 1), child


def tree_shape(child):
    """(interior levels of the deepest path from node 0, interior nodes without a leaf child)."""
    depth = {0: 1}
    order = [0]
    for n in order:
        for c in child[n]:
            if c >= 0:
                depth[int(c)] = depth[n] + 1
                order.append(int(c))
    no_leaf = sum(1 for n in order if (child[n] >= 0).all())
    return max(depth.values()), no_leaf


def subtree_levels(child):
    """[nn]: interior levels of the subtree under every node (a node whose children are both leaves: 1)."""
    nn = len(child)
    order = [0]
    for n in order:
        order += [int(c) for c in child[n] if c >= 0]
    lev = np.ones(nn, np.int64)
    for n in reversed(order):
        for c in child[n]:
            if c >= 0:
                lev[n] = max(lev[n], 1 + lev[c])
    return lev


def chain_stack_demand(nodes, o, d):
    """Per ray: the number of tree levels, along one root-to-leaf descent, at which the ray crosses both children's
    boxes (float64 slabs, t >= 0) -- the entries a depth-first walk that takes this path first leaves on its stack.
    The descent continues into the interior child whose box the ray crosses; where it crosses both, into the one
    with more levels below it. A model of demand, not of the kernel's exact order (a kernel visits the nearer child
    first and may pop early once a hit bounds t). nodes: parse_nodes()."""
    boxes, child = nodes
    lev = subtree_levels(child)
    o = np.asarray(o, np.float64)
    d = np.asarray(d, np.float64)
    n = len(o)
    demand = np.zeros(n, np.int64)
    node = np.zeros(n, np.int64)
    alive = np.ones(n, bool)
    with np.errstate(all="ignore"):
        inv = 1.0 / d
    while alive.any():
        idx = np.flatnonzero(alive)
        b = boxes[node[idx]]                                   # [m, 2, 6]
        with np.errstate(all="ignore"):
            t0 = (b[:, :, 0:3] - o[idx, None, :]) * inv[idx, None, :]
            t1 = (b[:, :, 3:6] - o[idx, None, :]) * inv[idx, None, :]
        near, far = np.minimum(t0, t1).max(2), np.maximum(t0, t1).min(2)
        hit = (near <= far) & (far >= 0)                       # [m, 2]
        demand[idx] += hit.all(1)
        ch = child[node[idx]]                                  # [m, 2]
        below = np.where(hit & (ch >= 0), lev[np.maximum(ch, 0)], 0)
        pick = (below[:, 1] > below[:, 0]).astype(np.int64)
        nxt = np.where(below.max(1) > 0, ch[np.arange(len(idx)), pick], -1)
        alive[idx] = nxt >= 0
        node[idx] = np.maximum(nxt, 0)
    return demand
