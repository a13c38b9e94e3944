"""Fixtures of the leaf-record tests (tests/test_gpu_leaf_records.py, tests/test_leaf_records_host.py): tiny meshes
whose binary trees hold leaves of chosen sizes, and the leaf histogram of a built scene read from its scene cache."""
import os
import struct
import tempfile

import numpy as np

import edge_scenes as E

F = np.float32
STACK_N = 8            # cells per side of the stack scene's front grid
STACK_MAX = 16         # most coincident copies in a cell = the leaf handle's largest count
STACK_DZ = 10.0        # flycam(W, H, 0, 0, STACK_DZ): the whole front grid in view, at 64x64 and at 40x24
LEAF_BOUNDS = (1, 2, 3, 4, 16)


def stack_scene(seed=3):
    """An 8x8 grid of cells in the plane z = 0, each cell holding one triangle (its lower-left half-quad) copied
    c times with its own vertices, c running 1..16 over the cells (four cells of every count); plus the tie
    scene's 2x2 back grid at z = -0.75, so that the loader's normalisation is scale 1 exactly. The copies of a
    cell are distinct faces with bit-identical planes: every ray through a cell meets c faces at equal t and the
    rank decides. No builder can separate coincident copies, so each cell stays one leaf of c records whatever
    the leaf bound: the bound does not bite on this fixture, and the trees built with the bounds of LEAF_BOUNDS
    all hold leaves of every count 1..16 (tests/test_leaf_records_host.py asserts it). The face list is permuted. Returns the mesh arrays and
    copies_of_face [nf] (0 for the back grid)."""
    rng = np.random.default_rng(seed)
    c = E.lattice(STACK_N)
    vs, fs, cop = [], [], []
    counts = rng.permutation(np.repeat(np.arange(1, STACK_MAX + 1), STACK_N * STACK_N // STACK_MAX))
    base = 0
    for j in range(STACK_N):
        for i in range(STACK_N):
            k = int(counts[j * STACK_N + i])
            tri = np.array([[c[i], c[j], 0], [c[i + 1], c[j], 0], [c[i], c[j + 1], 0]], F)
            for _ in range(k):
                vs.append(tri)
                fs.append([base, base + 1, base + 2])
                cop.append(k)
                base += 3
    v, f = E._grid(2, -0.75)
    vs.append(v)
    fs += (f + base).tolist()
    cop += [0] * len(f)
    v, f, cop = np.concatenate(vs).astype(F), np.array(fs, np.uint32), np.array(cop)
    perm = rng.permutation(len(f))
    return (v, f[perm], np.array([E.MATERIAL], F), [(len(f), 0)]), cop[perm]


def one_triangle():
    v = np.array([[-0.5, -0.5, 0.0], [0.5, -0.5, 0.0], [0.0, 0.5, -0.25]], F)
    return v, np.array([[0, 1, 2]], np.uint32), np.array([E.MATERIAL], F), [(1, 0)]


def empty():
    return np.zeros((0, 3), F), np.zeros((0, 3), np.uint32), np.array([E.MATERIAL], F), []


def tree_summary(sc):
    """Leaf histogram and record facts of a built scene, from its scene cache (split by test_host._cache_sections,
    the suite's one description of the cache layout): hist[c] = binary-tree leaves of c records (c = 1..16),
    n_records, n_faces, duplicate records (spatial splits), and the face ids of the leaf that ends at the last
    record of the triangle array."""
    from test_host import NODES, _cache_sections
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "s.rtscene")
        sc.save(p)
        with open(p, "rb") as fh:
            sections = _cache_sections(fh.read())
    nodes = np.frombuffer(bytes(sections[NODES]), "<u4").reshape(-1, 16)
    tris = np.frombuffer(bytes(sections[NODES + 2]), "<u4").reshape(-1, 16)
    nn, nt = len(nodes), len(tris)
    ch = nodes[:, 12:14].reshape(-1)  # Node64::child0 / child1
    leaves = ch[(ch >> 31) == 1]      # kLeafBit | (count - 1) << 27 | first
    cnt = ((leaves >> 27) & 15) + 1
    first = leaves & 0x7FFFFFF
    hist = {int(c): int(n) for c, n in enumerate(np.bincount(cnt, minlength=17)) if c and n}
    last = np.flatnonzero(first + cnt == nt)
    last_faces = tris[int(first[last[0]]):nt, 14].tolist() if len(last) else []  # TriRec64::face
    n_faces = int(struct.unpack_from("<8i", bytes(sections[0]), 16)[1])
    return dict(n_nodes=nn, n_records=nt, n_faces=n_faces, hist=hist,
                duplicates=int(nt - len(np.unique(tris[:, 14]))), last_leaf_faces=last_faces)
