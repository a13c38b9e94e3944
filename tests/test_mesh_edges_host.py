"""The mesh-edge inputs of tests/edge_scenes.py (explicit vertex normals that are zero, opposed, NaN, unnormalised or
tilted; zero-area faces; triangles small enough for the area arithmetic to underflow) really reach
calculateDistance's last rejection -- a hit whose interpolated normal has norm exactly 0 is dropped
(flyscene.cpp:467) -- asserted on the CPU oracle alone, so that the GPU battery (tests/test_gpu_mesh_edges.py)
can never go vacuous; and the safe-normal flag (TriRec64::box bit 31, rt_layout.cpp safe_normal), which lets the
kernels skip that rejection, is set exactly where it may be, on host-only scenes. No GPU needed.

Measured values (this oracle build, the generators' fixed seeds) are in the docstrings, after the bound."""
import numpy as np
import pytest

import edge_scenes as E

SAFE = 0x80000000
NFRONT = 2 * E.NORMAL_N ** 2  # faces of the normal scene's front grid; the back grid's follow


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def normal(orc):
    (v, f, m, g), vn, cls = E.normal_scene()
    mesh = orc.Mesh.from_arrays(v, f, m, vn3=vn, groups=g)
    return dict(arrays=(v, f, m, g), vn=vn, cls=cls, mesh=mesh, scene={mf: orc.Scene(mesh, min_faces=mf) for mf in (8, 300)})


def lattice_cell(o):
    """The front grid's cell column (0..15) under each lattice ray; a ray exactly on a column line counts to the
    cell on its right."""
    return np.minimum(np.floor((o[:, 0].astype(np.float64) + 0.5) * E.NORMAL_N).astype(int), E.NORMAL_N - 1)


def test_normal_scene_shape(orc, normal):
    """520 faces (512 + 8), 298 vertices; normalisation exactly scale 1, translation (0, 0, 0.375); the mesh keeps
    the given vertex normals bit for bit (NaN included); every face normal is exactly (0, 0, 1); min_faces 8 -> [68]
    reference boxes, 300 -> [2]."""
    v, f, m, g = normal["arrays"]
    ex = normal["mesh"].export()
    assert len(f) == NFRONT + 8 == 520 and len(v) == 298 and len(normal["cls"]) == 289
    M = np.eye(4, dtype=np.float32)
    M[2, 3] = E.NORMAL_PLANE_Z
    assert ex["M16"].tobytes() == M.T.reshape(-1).tobytes()
    assert ex["vn3"].tobytes() == normal["vn"].tobytes()
    assert (ex["fn3"] == np.float32([0, 0, 1])).all()
    assert "".join(normal["cls"][:17]) == E.NORMAL_CLASSES and set(E.NORMAL_CLASSES) == set("PNZTSXU")
    assert normal["scene"][8].box_count() > 50 and normal["scene"][300].box_count() >= 2


def test_lattice_rays_pass_through_zero_normals(orc, normal):
    """4,225 lattice rays: >= 300 pass through the front grid and hit the back grid [640]: >= 256 in the all-Z
    cells [512], >= 32 in the P|N cell [64, none on a column line: the weights of (0,0,1) and (0,0,-1) cancel
    exactly on the cell's midline, inside a face], >= 32 in the Z|T cell [64, all on the column line between two Z
    vertices, where the T vertex weighs nothing]; none in any other cell column [0]; the same for 68 and 2
    reference boxes. The same geometry with the loader's own normals lets none through [0]."""
    o, d = E.normal_lattice_rays()
    assert len(o) == 4225
    cell = lattice_cell(o)
    pair = np.array([E.NORMAL_CLASSES[c:c + 2] for c in range(E.NORMAL_N)])[cell]
    for mf in (8, 300):
        face, t, _ = normal["scene"][mf].closest(o, d)
        thr = face >= NFRONT
        on_line = (o[:, 0].astype(np.float64) + 0.5) * E.NORMAL_N == cell
        cnt = {p: int((thr & (pair == p)).sum()) for p in sorted(set(pair))}
        print(f"min_faces {mf}: through {int(thr.sum())}, by cell {cnt}, P|N on a line {int((thr & (pair == 'PN') & on_line).sum())}, "
              f"Z|T on a line {int((thr & (pair == 'ZT') & on_line).sum())}, misses {int((face < 0).sum())}")
        assert thr.sum() >= 300 and cnt["ZZ"] >= 256 and cnt["PN"] >= 32 and cnt["ZT"] >= 32
        assert sum(n for p, n in cnt.items() if p not in ("ZZ", "PN", "ZT")) == 0
        assert np.isfinite(t[thr]).all()
    v, f, m, g = normal["arrays"]
    plain = orc.Scene(orc.Mesh.from_arrays(v, f, m, groups=g))
    assert (plain.closest(o, d)[0] >= NFRONT).sum() == 0


def test_random_and_shadow_rays_pass_through(orc, normal):
    """4,096 random rays: >= 68 pass through to the back grid [153]; 2,048 shadow rays from just above the back
    grid: >= 134 unblocked [269], >= 134 blocked [1,779]."""
    o, d = E.normal_random_rays()
    P, L = E.normal_shadow_rays()
    assert len(o) == 4096 and len(P) == 2048
    for mf in (8, 300):
        thr = int((normal["scene"][mf].closest(o, d)[0] >= NFRONT).sum())
        blocked = normal["scene"][mf].shadow(P, L)
        print(f"min_faces {mf}: random through {thr}, shadow unblocked {int((blocked == 0).sum())}")
        assert thr >= 68 and (blocked == 0).sum() >= 134 and (blocked != 0).sum() >= 134


def test_frames_see_the_back_grid_and_nan_colours(orc, normal):
    """flycam(64, 40, 0, 0, 20): >= 75 back-grid pixels [150] and >= 220 pixels with a NaN colour [440] in PRIMARY,
    in FULL and at depth 3 [the same counts in all three; 2,070 hit pixels]."""
    for full, depth in ((False, None), (True, None), (True, 3)):
        rgb, face, t = normal["scene"][300].render(orc.flycam(64, 40, 0, 0, 20), orc.DEFAULT_LIGHTS, 64, 40, full=full,
                                                   max_depth=depth)
        back, nan = int((face >= NFRONT).sum()), int(np.isnan(rgb).any(1).sum())
        print(f"full {full} depth {depth}: back-grid pixels {back}, NaN pixels {nan}, hits {int((face >= 0).sum())}")
        assert back >= 75 and nan >= 220


def test_degenerate_faces_are_never_hit(orc, normal):
    """The generator's 24 zero-area faces ((a, a, b), (a, a, a), three collinear lattice vertices, two coincident
    vertices) spread through the normal scene's face list: the normalisation is unchanged, their face normals are
    exactly (0, 0, 0) and the others' still (0, 0, 1); none is ever hit, by any list at any box size [0]; with one
    reference box (min_faces 100,000: the partition cannot change) every other answer of the lattice, random and
    shadow lists is bit-identical -- face (ids mapped), t, P, blocked [0 differences]; with min_faces 8 and 300 the
    random and shadow lists still are [0], while the lattice list is only printed there: the added faces move the
    partition's split planes (the mean vertex coordinate over a box's faces) [68 -> 83 and 2 -> 3 boxes], and lattice
    rays lie on box planes and on edges shared by faces at equal t [1,045 and 193 rays answer another face, 7 and 1
    another t]."""
    v, f, m, g = normal["arrays"]
    lists = {"lattice": E.normal_lattice_rays(), "random": E.normal_random_rays()}
    P, L = E.normal_shadow_rays()
    v2, f2, vn2, added, new_id = E.degenerate_faces(v, f, normal["vn"])
    assert len(added) == 4 * E.DEGENERATE_PER_KIND and len(f2) == len(f) + len(added)
    assert (f2[new_id] == f).all() and not np.isin(new_id, added).any() and (np.diff(new_id) > 0).all()
    mesh = orc.Mesh.from_arrays(v2, f2, m, vn3=vn2, groups=[(len(f2), 0)])
    ex = mesh.export()
    assert ex["M16"].tobytes() == normal["mesh"].export()["M16"].tobytes()
    assert (ex["fn3"][added] == 0).all() and (ex["fn3"][new_id] == np.float32([0, 0, 1])).all()
    for mf in (8, 300, 100000):
        base = normal["scene"][mf] if mf in normal["scene"] else orc.Scene(normal["mesh"], min_faces=mf)
        deg = orc.Scene(mesh, min_faces=mf)
        for name, (o, d) in lists.items():
            a, b = base.closest(o, d), deg.closest(o, d)
            assert not np.isin(b[0], added).any(), name
            mapped = np.where(a[0] >= 0, new_id[np.maximum(a[0], 0)], -1)
            diff = (mapped != b[0]) | (bits(a[1]) != bits(b[1])) | (bits(a[2]) != bits(b[2])).any(1)
            print(f"min_faces {mf} {name}: boxes {base.box_count()} -> {deg.box_count()}, differ {int(diff.sum())}, "
                  f"t differs {int((bits(a[1]) != bits(b[1])).sum())}")
            if name == "random" or mf == 100000:
                assert not diff.any(), (mf, name)
        assert (base.shadow(P, L) == deg.shadow(P, L)).all()
        if mf == 100000:
            assert base.box_count() == deg.box_count() == 1


def micro_world(orc):
    v, f, m, g = E.micro_fan_scene()
    mesh = orc.Mesh.from_arrays(v, f, m, groups=g)
    w = v.copy()
    w[:, 2] += np.float32(E.MICRO_PLANE_Z)
    return (v, f, m, g), mesh, w


def micro_sqnorm(w, f):
    """Eigen's squaredNorm of cross(e0, -e2) per face in float32: what A = sqrt(.) / 2 is taken from."""
    c = E._cross_f32(w[f[:, 1]] - w[f[:, 0]], -(w[f[:, 0]] - w[f[:, 2]]))
    with np.errstate(all="ignore"):
        return (c[:, 0] * c[:, 0] + (c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])).astype(np.float32)


def test_micro_fan_reaches_the_underflow(orc):
    """37 triangles with edges 2^-8 .. 2^-44 and a unit backdrop; normalisation exactly scale 1, translation
    (0, 0, 0.25), so the world vertices are the given ones. In float32 A = norm(cross(e0, -e2)) / 2 is exactly 0 for
    >= 1 triangle [9: edges 2^-36 and smaller] and is taken from a denormal squared norm for >= 1 [6: edges 2^-30
    .. 2^-35; A itself cannot be denormal here: the square root of the smallest denormal is 2^-74.5, so below
    A = 1.9e-23 only 0 is left, and safe_normal's A > 1e-30 guard decides between those two]. Of the 296 aimed rays
    the oracle hits the aimed triangle for >= 74 [181], another face for >= 18 [70] and nothing for >= 11 [45]."""
    (v, f, m, g), mesh, w = micro_world(orc)
    ex = mesh.export()
    M = np.eye(4, dtype=np.float32)
    M[2, 3] = E.MICRO_PLANE_Z
    assert ex["M16"].tobytes() == M.T.reshape(-1).tobytes() and len(f) == len(E.MICRO_EXPONENTS) + 1 == 38
    A = E.area_f32(w[f[:, 0]], w[f[:, 1]], w[f[:, 2]])
    z = micro_sqnorm(w, f)
    tiny = np.finfo(np.float32).tiny
    zero, den = int((A == 0).sum()), int(((z > 0) & (z < tiny)).sum())
    print(f"A == 0: {zero} triangles, denormal squared norm: {den}, smallest non-zero A {A[A > 0].min():.4g}")
    assert zero >= 1 and den >= 1 and (A[:8] > tiny).all() and A[-1] == 0.5
    o, d, tri = E.micro_fan_rays()
    face, t, _ = orc.Scene(mesh).closest(o, d)
    own, other, miss = int((face == tri).sum()), int(((face >= 0) & (face != tri)).sum()), int((face < 0).sum())
    print(f"{len(o)} rays: aimed triangle {own}, another face {other}, miss {miss}")
    assert len(o) == 296 and own >= 74 and other >= 18 and miss >= 11


# ---- the flag itself, on host-only scenes ----

def host_scene(rt, arrays, vn, builder, **kw):
    v, f, m, g = arrays
    return rt.Scene(rt.Mesh.from_arrays(v, f, m, vn3=vn, groups=g), device=rt.RT_DEVICE_NONE, builder=builder,
                    box_builder=rt.RT_BOXES_HOST, **kw)


def check_record_counts(sc, flagged):
    """record_flags() against the per-face flags: every record of a flagged face carries the bit and no other
    record does, so the count lies between the flagged faces and those plus the extra (split) records, and equals
    the former when no face was split."""
    records, safe, _ = sc.record_flags()
    nf = sc.info()["n_faces"]
    assert records >= nf and int(flagged.sum()) <= safe <= int(flagged.sum()) + (records - nf)
    return records


@pytest.mark.parametrize("builder", ["RT_BUILDER_SBVH", "RT_BUILDER_SAH"])
def test_safe_normal_flag_follows_the_vertex_classes(rt, normal, builder):
    """A face of the normal scene has bit 0x80000000 exactly when its three vertices are of class P, S or U (unit
    after the mesh's normalisation and within 60 degrees of the face normal) [160 front faces and the 8 back-grid
    faces]; no degenerate face has it, and the others keep theirs; host SBVH and SAH, leaf sizes 1 and 16."""
    v, f, m, g = normal["arrays"]
    cls = normal["cls"]
    want = np.array([all(c in "PSU" for c in cls[tri]) for tri in f[:NFRONT]] + [True] * 8)
    for leaf in (1, 16):
        sc = host_scene(rt, normal["arrays"], normal["vn"], getattr(rt, builder), leaf_size=leaf, min_faces=8)
        assert sc.info()["builder"] == getattr(rt, builder) and sc.validate_bvh()["ok"]
        flagged = (sc.face_flags()[0] & SAFE) != 0
        assert (flagged == want).all() and 100 <= want.sum() <= 400
        check_record_counts(sc, flagged)
        v2, f2, vn2, added, new_id = E.degenerate_faces(v, f, normal["vn"])
        deg = host_scene(rt, (v2, f2, m, [(len(f2), 0)]), vn2, getattr(rt, builder), leaf_size=leaf, min_faces=8)
        assert deg.validate_bvh()["ok"], deg.validate_bvh()
        dflag = (deg.face_flags()[0] & SAFE) != 0
        assert not dflag[added].any() and (dflag[new_id] == want).all()
        check_record_counts(deg, dflag)


@pytest.mark.parametrize("builder", ["RT_BUILDER_SBVH", "RT_BUILDER_SAH"])
def test_safe_normal_flag_on_the_micro_fan(rt, orc, builder):
    """No micro-fan triangle whose A is <= 1e-30 or not finite is flagged [9 with A == 0, unflagged]; the ones with
    a normal A and the loader's normals (0, 0, 1) are [28 and the backdrop]."""
    (v, f, m, g), mesh, w = micro_world(orc)
    A = E.area_f32(w[f[:, 0]], w[f[:, 1]], w[f[:, 2]])
    sc = host_scene(rt, (v, f, m, g), None, getattr(rt, builder))
    assert sc.validate_bvh()["ok"], sc.validate_bvh()
    flagged = (sc.face_flags()[0] & SAFE) != 0
    unsafe = ~(A > np.float32(1e-30)) | ~np.isfinite(A)
    print(f"A <= 1e-30: {int(unsafe.sum())}, flagged {int(flagged.sum())}")
    assert unsafe.sum() >= 1 and not flagged[unsafe].any() and (flagged == ~unsafe).all()
    check_record_counts(sc, flagged)


@pytest.mark.parametrize("seed", range(4))
def test_flagged_faces_are_never_rejected_by_the_oracle(rt, orc, seed):
    """Soundness of the flag, judged by the oracle: a 16x16 grid with random unit vertex normals 0 .. 75 degrees
    from the face normal and twelve vertices exactly at the flag's boundary (n . n_k = 0.5 and its float
    neighbours); rays from z = 2 straight at the vertices, edge midpoints, centroid and 1/64 lattice points of
    every flagged face return a finite t -- all but the rays exactly in the planes x = 0.5 and y = 0.5, the outer
    planes of the reference boxes, which the reference's box predicate rejects (0 / 0 in its slabs) before any
    triangle is tested [4,466 .. 6,292 rays per seed, 90 / 138 / 164 / 74 of them in those planes, of which 86 / 130 /
    158 / 70 miss]; for those, and for all the others again, the blend
    itself (blend_normal_f32, held to the oracle's arithmetic below) is finite and not the zero vector at the
    target. >= 100 flagged and >= 100 unflagged faces per seed [flagged 203, 286, 254, 252 of 512]."""
    (v, f, m, g), vn = E.soundness_scene(seed)
    sc = host_scene(rt, (v, f, m, g), vn, rt.RT_BUILDER_SBVH)
    flagged = (sc.face_flags()[0] & SAFE) != 0
    assert flagged.sum() >= 100 and (~flagged).sum() >= 100
    # the flag's own rule, restated: every normalised vertex normal within 60 degrees of (0, 0, 1)
    nn = E.normalized_f32(vn)
    assert (flagged == (nn[f][:, :, 2] >= np.float32(0.5)).all(1)).all()
    w = v[f[flagged]].astype(np.float64)  # [n, 3 vertices, xyz]; z = 0
    tg = [w[:, 0], w[:, 1], w[:, 2], (w[:, 0] + w[:, 1]) / 2, (w[:, 1] + w[:, 2]) / 2, (w[:, 2] + w[:, 0]) / 2, w.mean(1)]
    # the 1/64 lattice points of the face's cell that lie in the triangle (barycentric weights >= 0, exact in float64)
    lo = w.min(1)
    k = np.arange(5) / 64.0
    gx, gy = np.meshgrid(k, k, indexing="xy")
    pts = lo[:, None, :2] + np.stack([gx.reshape(-1), gy.reshape(-1)], 1)[None]  # [n, 25, 2]
    a, b, c = w[:, None, 0, :2], w[:, None, 1, :2], w[:, None, 2, :2]
    cr = lambda p, q, r: (q[..., 0] - p[..., 0]) * (r[..., 1] - p[..., 1]) - (q[..., 1] - p[..., 1]) * (r[..., 0] - p[..., 0])
    inside = (cr(a, b, pts) >= 0) & (cr(b, c, pts) >= 0) & (cr(c, a, pts) >= 0)
    assert (inside.sum(1) == 15).all()
    lat = np.concatenate([pts[inside], np.zeros((int(inside.sum()), 1))], 1)
    tgt = np.concatenate(tg + [lat])
    o = tgt.copy()
    o[:, 2] = 2.0
    d = np.zeros_like(o)
    d[:, 2] = -1.0
    exact = np.ones(len(o), bool)
    exact[6 * len(w):7 * len(w)] = False  # (the centroids round; every other target is a binary fraction)
    assert (o.astype(np.float32) == o)[exact].all()
    face, t, _ = orc.Scene(orc.Mesh.from_arrays(v, f, m, vn3=vn, groups=g)).closest(o, d)
    # rays exactly in the planes x = 0.5 or y = 0.5 mostly never reach a triangle test: there the reference's box
    # predicate divides 0 by 0 (hi - o2 over a zero direction component) and rejects the box, whatever the normals are
    outer = (o[:, 0] == 0.5) | (o[:, 1] == 0.5)
    print(f"seed {seed}: flagged {int(flagged.sum())}, rays {len(o)}, on the outer box planes {int(outer.sum())}, "
          f"infinite t {int((~np.isfinite(t)).sum())}")
    assert np.isfinite(t[~outer]).all() and (face[~outer] >= 0).all()
    # so those are judged by the arithmetic itself (and all the others again): the reference's blend at the target,
    # restated in float32, is not the zero vector for the flagged face aimed at
    fid = np.flatnonzero(flagged)
    aimed = np.concatenate([fid] * 7 + [np.repeat(fid, 15)])
    w32 = v.copy()
    nrm = E.blend_normal_f32(w32[f[aimed, 0]], w32[f[aimed, 1]], w32[f[aimed, 2]], nn[f[aimed, 0]], nn[f[aimed, 1]],
                             nn[f[aimed, 2]], tgt.astype(np.float32))
    assert (E._norm_f32(nrm) != 0).all() and np.isfinite(nrm).all()


def test_blend_restatement_matches_the_oracle_arithmetic(orc, normal):
    """blend_normal_f32 / area_f32 (the float32 numpy restatement the GPU battery holds the kernels' N to) give the
    bits of the oracle's pinned Eigen expressions (known-answer ops NORM 14: norm(a) / 2, NRM_INTERP 13: the
    blend from normals, sub-areas and A) on the normal scene's random-ray hits [3,723 hits, every class of normal]
    and on the micro fan's areas."""
    v, f, m, g = normal["arrays"]
    o, d = E.normal_random_rays()
    face, t, P = normal["scene"][300].closest(o, d)
    hit = face >= 0
    tri, P = f[face[hit]], P[hit]
    w = v.copy()
    w[:, 2] += np.float32(E.NORMAL_PLANE_Z)
    w0, w1, w2 = w[tri[:, 0]], w[tri[:, 1]], w[tri[:, 2]]
    vn = normal["vn"]
    got = E.blend_normal_f32(w0, w1, w2, *(E.normalized_f32(vn[tri[:, k]]) for k in range(3)), P)
    e0, e1, e2 = w1 - w0, w2 - w1, w0 - w2
    cr = [E._cross_f32(e0, P - w0), E._cross_f32(e1, P - w1), E._cross_f32(e2, P - w2), E._cross_f32(e0, -e2)]
    n = len(P)
    areas = [orc.kat(14, c.reshape(-1), n, 1) for c in cr]
    inp = np.concatenate([vn[tri[:, 0]], vn[tri[:, 1]], vn[tri[:, 2]], np.stack(areas, 1)], 1).astype(np.float32)
    want = orc.kat(13, inp.reshape(-1), n, 3).reshape(n, 3)
    same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    print(f"{n} hits, classes {sorted(set(normal['cls'][tri[tri < 289]]))}, NaN normals {int(np.isnan(want).any(1).sum())}")
    assert n >= 2000 and same.all() and np.isnan(want).any() and (bits(areas[3]) == bits(E.area_f32(w0, w1, w2))).all()
    (mv, mf, _, _), _, mw = micro_world(orc)
    c = E._cross_f32(mw[mf[:, 1]] - mw[mf[:, 0]], -(mw[mf[:, 0]] - mw[mf[:, 2]]))
    assert (bits(orc.kat(14, c.reshape(-1), len(mf), 1)) == bits(E.area_f32(mw[mf[:, 0]], mw[mf[:, 1]], mw[mf[:, 2]]))).all()
