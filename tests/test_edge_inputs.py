"""The edge-case inputs of tests/edge_scenes.py really reach the edges they are built for -- asserted on the CPU
oracle alone, so that the GPU battery (tests/test_gpu_edges.py) can never go vacuous -- and the parity helper
of the GPU tests rejects a colour that is NaN or infinite on one side only. No GPU needed.

Measured values (this oracle build, the generators' fixed seeds) are in the docstrings, after the bound."""
import numpy as np
import pytest

import edge_scenes as E
from conftest import scene_path
from test_oracle_pinning import colour_errors

PLUS0, MINUS0 = 0x00000000, 0x80000000


def bits(t):
    return np.asarray(t, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def tie(orc):
    (v, f, m, g), copy = E.tie_scene()
    sc = {mf: orc.Scene(orc.Mesh.from_arrays(v, f, m, groups=g), min_faces=mf) for mf in (8, 300)}
    return sc, copy


def test_tie_scene_shape(orc, tie):
    """872 faces (3 x 288 + 8); normalisation exactly scale 1, translation (0, 0, 0.375); every face normal
    exactly (0, 0, 1); min_faces 8 -> more than 50 reference boxes [68], 300 -> [4]."""
    sc, copy = tie
    ex = sc[8].mesh.export()
    assert len(copy) == 872 and [(copy == k).sum() for k in range(4)] == [288, 288, 288, 8]
    M = np.eye(4, dtype=np.float32)
    M[2, 3] = E.TIE_PLANE_Z
    assert ex["M16"].tobytes() == M.T.reshape(-1).tobytes()
    assert (ex["fn3"] == np.float32([0, 0, 1])).all()
    assert sc[8].box_count() > 50 and 2 <= sc[300].box_count() <= 8


def test_tie_scene_random_rays_tie_and_rank_decides(orc, tie):
    """4,096 rays through the triple plane: all hit; the three coincident candidates (each copy traced alone)
    have the winner's t bit for bit; each copy wins >= 20% [min_faces 8: 41 / 30 / 28 %, 300: 34 / 35 / 31 %]; with
    min_faces 8 the winner is not the lowest face id among the three candidates for >= 25% of the rays [40.1%]
    (with min_faces 300, four boxes, for some [9.3%]): a tie broken by face id, slot or visit order cannot
    reproduce the reference's box-then-in-box order."""
    sc, copy = tie
    o, d = E.tie_random_rays()
    assert len(o) == 4096
    cand, ct = [], []
    for k in range(3):
        (v, f, m, g), ids = E.tie_copy_scene(k)
        fc, t, _ = orc.Scene(orc.Mesh.from_arrays(v, f, m, groups=g)).closest(o, d)
        assert (fc >= 0).all()
        cand.append(ids[fc])
        ct.append(t)
    cand = np.stack(cand, 1)
    assert (copy[cand] == np.arange(3)).all()
    frac = {}
    for mf in (8, 300):
        face, t, _ = sc[mf].closest(o, d)
        assert (face >= 0).all() and (t > 0).all()
        for tk in ct:
            assert (bits(tk) == bits(t)).all()
        assert (cand == face[:, None]).any(1).all()
        share = [(copy[face] == k).mean() for k in range(3)]
        frac[mf] = float((face != cand.min(1)).mean())
        print(f"min_faces {mf}: copies win {share}, winner != lowest id {frac[mf]:.4f}")
        assert min(share) >= 0.20
    assert frac[8] >= 0.25 and frac[300] > 0


def test_tie_scene_lattice_rays_reach_the_nan_slabs(orc, tie):
    """1,976 axis-aligned rays at vertex coordinates: >= 20 have a NaN (0 / 0) in the reference's slab arithmetic
    [min_faces 8: 1,944, 300: 1,272]; >= 5 get another answer when only the box partition changes (min_faces 8 vs
    300) [closest 501, shadow 4]: the box predicate's NaN behaviour decides there."""
    sc, _ = tie
    o, d, _ = E.tie_lattice_rays()
    M16 = sc[8].mesh.export()["M16"]
    res = {}
    for mf in (8, 300):
        nan = E.ref_slab_nan(sc[mf].boxes()[0], M16, o, d)
        face, t, _ = sc[mf].closest(o, d)
        res[mf] = (face, sc[mf].shadow(o, d))
        print(f"min_faces {mf}: {len(o)} rays, NaN-slab rays {int(nan.sum())}, hits {int((face >= 0).sum())}")
        assert nan.sum() >= 20 and (face >= 0).sum() >= 100
    dc, ds = int((res[8][0] != res[300][0]).sum()), int((res[8][1] != res[300][1]).sum())
    print(f"closest differs for {dc} rays, shadow for {ds}")
    assert dc >= 5
    assert ((d == 0) & ~np.signbit(d)).any() and ((d == 0) & np.signbit(d)).any()


def test_cube_lattice_rays_reach_the_nan_slabs(orc):
    """484 rays per axis direction: >= 20 NaN-slab rays each [160]; every direction also returns back-facing
    faces (n . d > 0: the far side's, from origins on the far plane) [+y: faces 4, 5] and hits at t = +0 and
    t = -0 [65 or 66 of each per direction]."""
    mesh = orc.Mesh.load_obj(scene_path("cube.obj"))
    sc = orc.Scene(mesh)
    ex = mesh.export()
    o, d, ad = E.cube_lattice_rays()
    nan = E.ref_slab_nan(sc.boxes()[0], ex["M16"], o, d)
    face, t, _ = sc.closest(o, d)
    for a in range(6):
        s = ad == a
        k, sign = a // 2, 1.0 if a % 2 == 0 else -1.0
        hit = face[s][face[s] >= 0]
        back = sorted({int(x) for x in hit if ex["fn3"][x][k] * sign > 0})
        print(f"direction {a}: rays {int(s.sum())}, NaN-slab rays {int(nan[s].sum())}, hits {len(hit)}, back-facing {back}")
        assert nan[s].sum() >= 20 and back
        assert (bits(t[s]) == PLUS0).sum() >= 20 and (bits(t[s]) == MINUS0).sum() >= 20


def test_on_plane_rays_give_both_zeros(orc, tie):
    """Origins exactly on the triple plane: t = +0 for >= 25% of the 2,048 rays [38.1%], t = -0 for >= 25% [36.9%];
    the in-plane directions (n . d = 0) all miss; shadow() of the same rays is mixed [16.3% blocked]."""
    sc, _ = tie
    o, d, kind = E.on_plane_rays()
    for mf in (8, 300):
        face, t, _ = sc[mf].closest(o, d)
        p0, m0 = (bits(t) == PLUS0).mean(), (bits(t) == MINUS0).mean()
        blocked = sc[mf].shadow(o, d).mean()
        print(f"min_faces {mf}: +0 {p0:.4f}, -0 {m0:.4f}, shadow blocked {blocked:.4f}")
        assert p0 >= 0.25 and m0 >= 0.25
        assert (face[kind == 2] == -1).all() and np.isinf(t[kind == 2]).all()
        assert 0.05 < blocked < 0.95


def test_shadow_straddle_is_mixed(orc, tie):
    """P below the plane by 0.5x / 1x / 1.5x of 0.003 |L_z|: blocked share between 20% and 80% [66.7%: 0%, 100%,
    100% by class -- at 1x the reference's P + 0.003 L rounds onto or below the plane, where t = +-0 counts]."""
    sc, _ = tie
    P, L = E.shadow_straddle_rays()
    for mf in (8, 300):
        b = sc[mf].shadow(P, L)
        print(f"min_faces {mf}: blocked {b.mean():.4f}, by class {[float(b[i::3].mean()) for i in range(3)]}")
        assert 0.2 <= b.mean() <= 0.8


def test_material_scene_covers_every_group(orc):
    """64x40, eye (0, 0, 1): >= 20 hit pixels per group [22 .. 46, 350 in all; the material-less group 33]; NaN
    colours with a light on [1 light: 39 PRIMARY / 38 FULL pixels, 32 lights: 73 / 74]; 0 and 32 lights render
    (0 lights: every hit pixel black, no NaN)."""
    v, f, m, g = E.material_scene()
    assert len(f) == 605 and len(m) == 10 and g[-1][1] == -1
    assert sorted(m[:, 9].tolist()) == sorted(np.float32(E.MATERIAL_NS).tolist())
    sc = orc.Scene(orc.Mesh.from_arrays(v, f, m, groups=g))
    W, H, dx, dy, dz = E.MATERIAL_CAMERA
    gid = np.repeat(np.arange(len(g)), [x[0] for x in g])
    for nl, lights in ((0, []), (1, orc.DEFAULT_LIGHTS), (32, E.ring_lights(32))):
        assert len(lights) == nl and all(max(c) <= 0.05 for _, c in lights if nl == 32)
        for full in (False, True):
            rgb, face, t = sc.render(orc.flycam(W, H, dx, dy, dz), lights, W, H, full=full)
            hit = face >= 0
            cnt = np.bincount(gid[face[hit]], minlength=len(g))
            nanpx = int(np.isnan(rgb).any(1).sum())
            print(f"{nl} lights, full {full}: hits {int(hit.sum())}, per group {cnt.tolist()}, NaN pixels {nanpx}")
            assert cnt.min() >= 20
            if nl == 0:
                assert nanpx == 0 and (rgb[hit] == 0).all()
            else:
                assert nanpx >= 1 and np.isfinite(rgb[hit]).all(1).sum() >= 200


def test_zero_direction_rays_miss(orc, tie):
    """d = (+-0, +-0, +-0): the reference divides by zero in every slab and its triangle test returns -1."""
    sc, _ = tie
    o, d = E.zero_direction_rays()
    face, t, _ = sc[8].closest(o, d)
    assert (face == -1).all() and np.isinf(t).all() and (sc[8].shadow(o, d) == 0).all()


def test_colour_errors_counts_one_sided_nonfinite():
    a = np.float32([[0.1, 0.2, 0.3], [np.nan, 0.5, np.inf], [0.0, -np.inf, 1.0]])
    assert colour_errors(a, a.copy()) == (0, 0.0)
    for pos, val in (((0, 0), np.nan), ((1, 0), 0.5), ((1, 2), -np.inf), ((2, 1), np.inf), ((0, 1), np.inf), ((1, 2), 1.0)):
        b = a.copy()
        b[pos] = val
        assert colour_errors(a, b)[0] == 1 and colour_errors(b, a)[0] == 1, (pos, val)
    b = a.copy()
    b[0, 2] += np.float32(0.25)
    odd, linf = colour_errors(a, b)
    assert odd == 0 and abs(linf - 0.25) < 1e-6


def test_compare_rejects_one_sided_nan():
    """compare() of the GPU parity tests: a colour that is NaN (or infinite) in the GPU frame and finite in the
    oracle's, or the reverse, fails -- it is not dropped from the maximum."""
    from test_gpu_parity import compare
    face = np.int32([0, 1, -1, 2])
    t = np.float32([1.0, 2.0, np.inf, 0.5])
    rgb = np.float32([[0.1, 0.2, 0.3], [np.nan, np.nan, np.nan], [0.9, 0.9, 0.9], [1.0, 0.0, 0.5]])
    assert compare(rgb, face, t, rgb.copy(), face, t, "same") == 0.0
    for pos, val in (((0, 1), np.nan), ((1, 1), 0.25), ((3, 2), np.inf)):
        other = rgb.copy()
        other[pos] = val
        for x, y in ((rgb, other), (other, rgb)):
            with pytest.raises(AssertionError, match="one side only"):
                compare(x, face, t, y, face, t, "one-sided")
    other = rgb.copy()
    other[0, 0] += np.float32(1e-3)
    with pytest.raises(AssertionError, match="L_inf"):
        compare(rgb, face, t, other, face, t, "finite error")
