"""CPU: the mesh voxelisation stage's contract as tests/meshvoxel_ref.py restates it - against the analytic cube and
octahedron, the separating-axis test against exact clipping in fractions, every consequence the contract lists, the planted errors -,
mesh.voxelize, mesh.occupancy_lists and groundTruth.gt_cubes_from_mesh on a stand-in context that is the restatement, the wiring of the new
symbols, and the rules header under the sanitizers (tests/host/meshvoxel_check.cpp). No GPU and no library.

The solids stand meshwinding_ref.SHIFT = 8 whole cells up every axis, in cubes of D = 8 at stride 4: world cells 0 .. 19."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import mesh_refusals as bad
import meshnormals_ref as mn
import meshrender_ref as rr
import meshvoxel_ref as ref
import meshwinding_ref as wr
from test_host_plumbing import CSRC, ROOT, _compile

AXES = (0, 1, 2)
FIX, HALF = ref.FIX, ref.HALF


def _same(a, b, keys=ref.KEYS):
    return ref.same_bytes(a, b, keys) == []


def _cells(r, case, bit):
    return {tuple(c) for c in ref.distinct(r["occ"], case[2], case[4], bit).tolist()}


# ---- the restatement on the solids -----------------------------------------------------------------------------------------------------------------------
def _cube_truth(g):
    """g (…,3) world cells, in the solid's own frame -> (solid, surface) of the cube 0 .. 4: a centre strictly inside or - rule 4's half-open
    fill - on a face that owns it is decided by the restatement, so only centres off the surface are held; a box meets the surface iff it
    meets the closed cube and does not lie inside the open one."""
    inside = ((g > 0) & (g < 4)).all(axis=-1)
    on = ((g >= 0) & (g <= 4)).all(axis=-1) & ~inside
    meets = ((g >= 0) & (g <= 4)).all(axis=-1)                  # g - 1/2 <= 4 and g + 1/2 >= 0, g an integer
    within = ((g >= 1) & (g <= 3)).all(axis=-1)                 # [g - 1/2, g + 1/2] inside (0, 4)
    return inside, on, meets & ~within


def _octahedron_truth(g, r=4):
    a = np.abs(g)
    d = a.sum(axis=-1)
    nearest, farthest = np.maximum(a - 0.5, 0).sum(axis=-1), (a + 0.5).sum(axis=-1)      # the least and the largest |x| + |y| + |z| over the box
    return d < r, d == r, (nearest <= r) & (r <= farthest)


@pytest.mark.parametrize("name,truth", [("cube", _cube_truth), ("octahedron", _octahedron_truth)])
def test_the_solids_against_the_analytic_answer(name, truth):
    v, f, cube, D, stride = ref.CASES[name]()
    assert (D, stride) == (8, 4) and cube.shape == (64, 3)
    g = ref.world_cells(cube, D, stride) - int(wr.SHIFT)
    inside, on, surface = truth(g)
    assert inside.sum() > 100 and on.sum() > 100 and surface.sum() >= on.sum() and (~inside & ~surface).sum() > 10000
    whole = [n for n in range(64) if not surface[n].any()]
    assert any(inside[n].sum() == 0 for n in whole) and len(whole) >= 7      # cubes wholly above, below and beside the mesh
    for axis in AXES:
        r = ref.reference(name, axis)
        assert np.array_equal((r["occ"] & 2) != 0, surface), axis
        assert np.array_equal(((r["occ"] & 1) != 0)[~on], inside[~on]), axis
        assert np.array_equal(r["Y"], ((r["occ"] & 2) != 0).astype(np.float32)[:, None]) and r["Y"].dtype == np.float32
        assert r["per_cube"].sum(axis=0).tolist() == r["counts"][3:5].tolist() == [int((r["occ"] & 1).sum()), int(((r["occ"] >> 1) & 1).sum())]
        assert r["counts"][5] == (r["occ"] == 3).sum() > 0
    assert ref.reference("cube", 0)["counts"][:3].tolist() == [4, 8, 0] and ref.reference("octahedron", 1)["counts"][:3].tolist() == [8, 0, 0]


# ---- the separating-axis test against exact clipping -----------------------------------------------------------------------------------------------------
def _clip_nonempty(tri):
    """tri: three corners of Fractions relative to the box centre -> the closed triangle and the closed box [-1/2, 1/2]^3 have a common
    point: Sutherland-Hodgman against the six closed half spaces; what is left is not empty."""
    poly = [tuple(p) for p in tri]
    h = Fraction(1, 2)
    for d in range(3):
        for sign in (1, -1):
            inside = lambda p: sign * p[d] <= h
            out = []
            for i, p in enumerate(poly):
                q = poly[(i + 1) % len(poly)]
                if inside(p):
                    out.append(p)
                if inside(p) != inside(q):
                    t = (sign * h - p[d]) / (q[d] - p[d])
                    out.append(tuple(p[k] + t * (q[k] - p[k]) for k in range(3)))
            poly = out
            if not poly:
                return False
    return True


def _pairs():
    """(triangle, box) pairs as q (m,3,3) int64 relative to the box centre: corners on a lattice of quarter cells around the box - vertices on
    box faces, edges and corners, edges through box edges and corners, coplanar faces - and corners in general position."""
    rng = np.random.RandomState(5)
    coarse = rng.randint(-4, 5, (2600, 3, 3)).astype(np.int64) * (FIX // 4)
    fine = rng.randint(-2 * FIX, 2 * FIX, (900, 3, 3)).astype(np.int64)
    # small triangles just off the middle of a box face, their planes through the box: only that face's axis parts them from the box
    centre = np.zeros((360, 1, 3))
    centre[np.arange(360), 0, np.arange(360) % 3] = np.where(np.arange(360) % 2, 0.6, -0.6)
    tiny = np.rint((centre + rng.uniform(-0.05, 0.05, (360, 1, 3)) + rng.uniform(-0.12, 0.12, (360, 3, 3))) * FIX).astype(np.int64)
    made = np.asarray([
        [[2, 0, 0], [2, 4, 0], [2, 0, 4]],                      # coplanar with the face x = 1/2
        [[2, 2, 2], [6, 2, 2], [2, 6, 6]],                      # a vertex on the corner
        [[4, 0, -4], [0, 4, -4], [4, 4, 8]],                    # an edge through the box edge x + y = 1 at z ... (x = y = 1/2)
        [[3, -1, 0], [-1, 3, 0], [3, 3, 0]],                    # an edge through the box edge's middle, in the plane z = 0
        [[3, 0, 0], [0, 3, 0], [0, 0, 3]],                      # the plane x + y + z = 3/4: cuts the corner
        [[6, 0, 0], [0, 6, 0], [0, 0, 6]],                      # x + y + z = 3/2: touches the corner
        [[7, 0, 0], [0, 7, 0], [0, 0, 7]],                      # beyond it
        [[8, 8, 1], [-8, 8, 1], [0, -8, 1]]], np.int64) * (FIX // 4)      # a large triangle through the box
    return np.concatenate([coarse, fine, tiny, made])


def test_the_separating_axis_test_against_exact_clipping():
    v = _pairs()
    n = [wr._normal(*(tuple(int(x) for x in c) for c in t), lambda x: x) for t in v]
    keep = np.asarray([x != (0, 0, 0) for x in n])
    v, n = v[keep], [x for x, k in zip(n, keep) if k]
    assert v.shape[0] > 3000
    want = np.asarray([_clip_nonempty([[Fraction(int(x), FIX) for x in c] for c in t]) for t in v])
    got = np.asarray([ref.sat(t[None], x)[0] for t, x in zip(v, n)])
    assert np.array_equal(got, want) and 500 < want.sum() < want.size - 500
    # the same through Python integers
    assert np.array_equal(np.asarray([ref.sat(t[None].astype(object), x)[0] for t, x in zip(v[:400], n[:400])]), want[:400])
    # planted: touching counts as separated - the pairs that only touch are lost
    opened = np.asarray([ref.sat(t[None], x, open_sets=True)[0] for t, x in zip(v, n)])
    assert (opened <= want).all() and (want & ~opened).sum() > 50
    # planted: each of the 13 axes left out gives a hit where the sets are apart - every axis is needed
    for skip in range(13):
        loose = np.asarray([ref.sat(t[None], x, skip=skip)[0] for t, x in zip(v, n)])
        assert (loose >= want).all() and (loose & ~want).any(), skip


# ---- what follows from the contract ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "octahedron", "sliver", "shell_q"])
def test_consequences(name):
    from surfacenet_amd import mesh
    case = ref.CASES[name]()
    v, f, cube, D, stride = case
    want = {axis: ref.reference(name, axis) for axis in AXES}
    rng = np.random.RandomState(3)
    fp, cp = rng.permutation(f.shape[0]), rng.permutation(cube.shape[0])
    world = ref.world_cells(cube, D, stride).reshape(-1, 3)
    _, inverse, n_in = np.unique(world, axis=0, return_inverse=True, return_counts=True)
    inverse = np.asarray(inverse).reshape(-1)
    assert (n_in > 1).any()                                     # the cubes overlap
    for axis in AXES:
        w = want[axis]
        flat = w["occ"].reshape(-1)
        for bit in (1, 2):                                      # two cubes that share a world cell give it the same bits
            per_cell = np.zeros((n_in.size,), np.int64)
            np.add.at(per_cell, inverse, (flat & bit) != 0)
            assert ((per_cell == 0) | (per_cell == n_in)).all(), (axis, bit)
        assert _same(ref.voxelize(v, f[fp], cube, D, stride, axis), w)                      # a permutation of the faces
        r = ref.voxelize(v, f, cube[cp], D, stride, axis)                                   # a permutation of the cubes
        assert all(np.array_equal(r[k], w[k][cp]) for k in ref.KEYS[:3]) and np.array_equal(r["counts"][:6], w["counts"][:6])
        if axis == 2:
            shift = np.asarray([1000, 8, (1 << 19) // stride])
            assert _same(ref.voxelize(v + shift * stride, f, cube + shift.astype(np.int32), D, stride, axis), w)      # whole cells
        if f.shape[1] == 4:
            assert _same(ref.voxelize(v, mesh.triangulate(f), cube, D, stride, axis), w)      # mesh.triangulate changes nothing
        assert _same(ref.voxelize(v, f[:, ::-1], cube, D, stride, axis), w, ("occ", "Y", "per_cube"))      # every face reversed
        assert np.array_equal(w["occ"] & 2, want[0]["occ"] & 2)                             # the surface bit does not depend on the axis
        # a centre on the surface has its surface bit
        cells = np.unique(world, axis=0)
        on = wr.winding(v, f, cells.astype(np.float64), axis)["on_surface"].astype(bool)
        surface = {tuple(c) for c in ref.distinct(w["occ"], cube, stride, 2).tolist()}
        assert all(tuple(c) in surface for c in cells[on].tolist()) and (on.any() or name in ("sliver", "shell_q"))
        # two centres adjacent along the axis that differ in the solid bit: one of them has the surface bit
        solid, surf = np.moveaxis((w["occ"] & 1) != 0, axis + 1, -1), np.moveaxis((w["occ"] & 2) != 0, axis + 1, -1)
        differ = solid[..., 1:] != solid[..., :-1]
        assert (surf[..., 1:] | surf[..., :-1])[differ].all() and (differ.any() or name == "sliver")
    # modes and select: the bits one by one
    w = want[1]
    for modes in (1, 2):
        r = ref.voxelize(v, f, cube, D, stride, 1, modes=modes, select=modes)
        assert np.array_equal(r["occ"], w["occ"] & modes) and np.array_equal(r["Y"][:, 0], (w["occ"] & modes) != 0)
    assert np.array_equal(ref.voxelize(v, f, cube, D, stride, 1, select=3)["Y"][:, 0], w["occ"] != 0)


def _closed_and_consistent(tri):
    e = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    fwd = {(int(a), int(b)) for a, b in e}
    return len(fwd) == len(e) and all((b, a) in fwd for a, b in fwd)


def _sphere():
    v, f = rr.sphere(6)
    return np.rint((v * 4.5 + 10.0) * FIX) / FIX, f


@pytest.mark.parametrize("name", ["cube", "octahedron", "sphere"])
def test_the_volume_lies_within_the_surface_voxels_of_the_solid_count(name):
    """On a closed, consistently turned mesh without self-intersections inside the cubes |volume - #solid| <= #surface over the distinct
    world cells: a box that no triangle touches lies wholly in or wholly out, as its centre does; the volume is mesh_normals' exact one."""
    v, f = _sphere() if name == "sphere" else ref.CASES[name]()[:2]
    cube, D, stride = ref.cube_grid(0, 3, 4), 8, 4
    assert _closed_and_consistent(wr.triangles(f)) and v.min() > 0.5 and v.max() < 18.5
    volume = Fraction(int(mn.normals(v, f)["vol6"]), 6 * FIX ** 3)
    assert volume > 0
    for axis in AXES:
        r = ref.voxelize(v, f, cube, D, stride, axis)
        n_solid, n_surface = (ref.distinct(r["occ"], cube, stride, bit).shape[0] for bit in (1, 2))
        assert abs(volume - n_solid) <= n_surface and n_solid > 20, (axis, float(volume), n_solid, n_surface)


def test_same_way_nested_cubes_winding_two_is_solid():
    v, f, cube, D, stride = ref.CASES["nested_same"]()
    cells = np.unique(ref.world_cells(cube, D, stride).reshape(-1, 3), axis=0)
    w = wr.winding(v, f, cells.astype(np.float64), 2)["winding"]
    assert (w == 2).sum() >= 27
    solid = {tuple(c) for c in ref.distinct(ref.reference("nested_same")["occ"], cube, stride, 1).tolist()}
    assert all(tuple(c) in solid for c in cells[w == 2].tolist())


def test_the_two_ways_to_the_solid_bit_agree():
    for name in ("octahedron", "nested_same", "open_cube", "degenerate"):
        v, f, cube, D, stride = ref.CASES[name]()
        pick = cube[::5]
        for axis in AXES:
            want = (ref.voxelize(v, f, pick, D, stride, axis)["occ"] & 1) != 0
            assert np.array_equal(ref.solid_by_columns(v, f, pick, D, stride, axis), want) and want.any(), (name, axis)


# ---- planted errors: each fails a named case -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plant,name,axis,keys", [("parity", "nested_same", 2, ("occ",)), ("open", "cube", 2, ("occ",)), ("floor_columns", "sliver", 2, ("occ",)),
                                                  ("overlap", "octahedron", 2, ("occ",)), ("axis_z", "open_cube", 0, ("occ",)), ("skip_axis", "sliver_12", 1, ("occ",))])
def test_planted_errors(plant, name, axis, keys):
    v, f, cube, D, stride = ref.CASES[name]()
    want = ref.reference(name, axis)
    assert _same(ref.voxelize(v, f, cube, D, stride, axis), want)
    if plant == "skip_axis":
        wrong = [ref.voxelize(v, f, cube, D, stride, axis, plant=plant, skip=s) for s in range(4, 13)]
        assert any(ref.same_bytes(r, want, keys) == list(keys) for r in wrong)
        return
    r = ref.voxelize(v, f, cube, D, stride, axis, plant=plant)
    assert ref.same_bytes(r, want, keys) == list(keys), plant
    if plant == "overlap":                                      # ... and it is the shared-cell property that sees it
        world = ref.world_cells(cube, D, stride).reshape(-1, 3)
        _, inverse, n_in = np.unique(world, axis=0, return_inverse=True, return_counts=True)
        per_cell = np.zeros((n_in.size,), np.int64)
        np.add.at(per_cell, np.asarray(inverse).reshape(-1), (r["occ"].reshape(-1) & 2) != 0)
        assert not ((per_cell == 0) | (per_cell == n_in)).all()


def test_planted_k_off_by_one():
    v, f, cube, D, stride = ref.CASES["octahedron"]()
    pick = cube[21:23]
    want = (ref.voxelize(v, f, pick, D, stride, 2)["occ"] & 1) != 0
    assert np.array_equal(ref.solid_by_columns(v, f, pick, D, stride, 2), want) and want.any()
    assert not np.array_equal(ref.solid_by_columns(v, f, pick, D, stride, 2, plant="k_off"), want)


# ---- the refusals, in the library's words ----------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_restatement():
    v, f = bad.sheet()
    cube = np.asarray([[0, 0, 0], [1, 2, 3]], np.int32)
    bv, bf, text = bad.bad_index(v, f, 2, 5)
    neg, far = cube.copy(), cube.copy()
    neg[1, 1], far[0, 2] = -1, (2097144 - 8) // 4 + 1
    for args, words in (((bv, bf, cube, 8, 4), text), ((v, f, neg, 8, 4), ref.NEGATIVE_TEXT % 1), ((v, f, far, 8, 4), ref.REACH_TEXT % 0),
                        ((bv, bf, neg, 8, 4), text), ((v, f, cube, 0, 4), "D = 0: 1 .. 64"), ((v, f, cube, 65, 4), "D = 65: 1 .. 64"),
                        ((v, f, cube, 8, 0), "stride_vox = 0 must be >= 1"), ((v, f, np.zeros(((1 << 15) + 1, 3), np.int32), 64, 1), "8590196736 voxels: at most 2^33")):
        with pytest.raises(ValueError) as e:
            ref.voxelize(*args)
        assert str(e.value) == words
    far[0, 2] -= 1                                              # the last cell is 2^21 - 9: legal
    assert ref.voxelize(v, f, far, 8, 4)["occ"].shape == (2, 8, 8, 8)
    for kw, words in ((dict(axis=3), wr.AXIS_TEXT % 3), (dict(modes=0), "modes = 0: 1 (solid), 2 (surface) or 3 (both)"), (dict(select=4), "select = 4: 1 (solid), 2 (surface) or 3 (either)")):
        with pytest.raises(ValueError) as e:
            ref.voxelize(v, f, cube, 8, 4, **kw)
        assert str(e.value) == words
    r = ref.voxelize(v, f, np.zeros((0, 3), np.int32), 8, 4)    # no cube: the mesh is checked and counted
    assert r["occ"].shape == (0, 8, 8, 8) and r["Y"].shape == (0, 1, 8, 8, 8) and r["counts"][:3].sum() == 18 and not r["counts"][3:].any()
    r = ref.voxelize(np.zeros((0, 3)), np.zeros((0, 3), np.int32), cube, 1, 1)
    assert r["occ"].shape == (2, 1, 1, 1) and not r["occ"].any() and not r["counts"].any()


# ---- the Python layers, before the library and on a stand-in ---------------------------------------------------------------------------------------------
class StandIn:
    """A context whose mesh_voxelize is the restatement."""

    def mesh_voxelize(self, verts, faces, cube_ijk, D, stride_vox, axis=2, modes=3, select=2, outputs=ref.KEYS[:3], device=False):
        r = ref.voxelize(verts, faces, cube_ijk, D, stride_vox, axis, modes, select)
        return {k: r[k] for k in tuple(outputs) + ("counts",)}


def _stand_in(monkeypatch):
    from surfacenet_amd import runtime
    ctx = StandIn()
    monkeypatch.setattr(runtime, "any_context", lambda: ctx)


def _no_library(monkeypatch):
    from surfacenet_amd import runtime

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(runtime, "any_context", no_library)


def test_the_python_layers_refuse_in_the_stages_words_before_the_library(monkeypatch):
    from surfacenet_amd import groundTruth, mesh
    _no_library(monkeypatch)
    v, f = bad.sheet()
    cube = np.asarray([[0, 0, 0], [1, 2, 3]], np.int32)
    bv, bf, text = bad.bad_index(v, f, 2, 5)
    cv, cf, ctext = bad.bad_coordinate(v, f, 3, 2097144.0)
    neg, far = cube.copy(), cube.copy()
    neg[1, 1], far[0, 2] = -1, (2097144 - 8) // 4 + 1
    cases = (((bv, bf, cube, 8, 4), text), ((cv, cf, cube, 8, 4), ctext), ((v, f, neg, 8, 4), ref.NEGATIVE_TEXT % 1), ((v, f, far, 8, 4), ref.REACH_TEXT % 0),
             ((v, f, cube, 0, 4), "D = 0: 1 .. 64"), ((v, f, cube, 65, 4), "D = 65: 1 .. 64"), ((v, f, cube, 8, 0), "stride_vox = 0 must be >= 1"),
             ((v, f, cube, 8.5, 4), "cube_D = 8.5 must be an integer"), ((v, f, cube, 8, True), "stride_vox = True must be an integer"),
             ((v, f, cube.astype(np.float64), 8, 4), "cube_ijk must hold integers, not float64"), ((v, f, np.zeros((2, 2), np.int32), 8, 4), "cube_ijk must be (N,3), not (2, 2)"),
             ((v.astype(np.int32), f, cube, 8, 4), "vert_lattice must be float32 or float64, not int32"),
             ((v, f, np.zeros(((1 << 15) + 1, 3), np.int32), 64, 1), "8590196736 voxels: at most 2^33"))
    for fn in (mesh.voxelize, groundTruth.gt_cubes_from_mesh):
        for args, words in cases:
            with pytest.raises(ValueError) as e:
                fn(*args)
            assert str(e.value) == words, (fn, words)
        with pytest.raises(ValueError, match="axis = 5"):
            fn(v, f, cube, 8, 4, axis=5)
    for mode in ("both", (), ("solid", "edge"), 3, None):
        with pytest.raises(ValueError, match="mode = "):
            mesh.voxelize(v, f, cube, 8, 4, mode=mode)
    for select in ("both", 2, None, ()):
        with pytest.raises(ValueError, match="select = "):
            groundTruth.gt_cubes_from_mesh(v, f, cube, 8, 4, select=select)
        with pytest.raises(ValueError, match="select = "):
            mesh.occupancy_lists(np.zeros((1, 2, 2, 2), np.uint8), select)
    with pytest.raises(ValueError, match="occ must be uint8"):
        mesh.occupancy_lists(np.zeros((1, 2, 2, 3), np.uint8))
    # no cube, no face: without the library
    for vv, ff, cc in ((v, f, np.zeros((0, 3), np.int32)), (np.zeros((0, 3)), np.zeros((0, 4), np.int32), cube), (v, np.zeros((0, 3), np.int32), cube)):
        r = mesh.voxelize(vv, ff, cc, 8, 4, axis="x")
        N = cc.shape[0]
        assert r["occ"].shape == (N, 8, 8, 8) and r["occ"].dtype == np.uint8 and r["solid"].dtype == r["surface"].dtype == bool and not r["occ"].any()
        assert r["n_solid"].shape == r["n_surface"].shape == (N,) and [r[k] for k in mesh.VOXEL_COUNTS] == [0] * 8
        Y = groundTruth.gt_cubes_from_mesh(vv, ff, cc, 8, 4)
        assert Y.shape == (N, 1, 8, 8, 8) and Y.dtype == np.float32 and not Y.any()
    assert mesh.VOXEL_COUNTS == ref.COUNTS


def test_the_python_layers_on_the_stand_in(monkeypatch):
    from surfacenet_amd import groundTruth, mesh
    _stand_in(monkeypatch)
    v, f, cube, D, stride = ref.CASES["octahedron"]()
    for axis, name in ((0, "x"), (1, 1), (2, "z")):
        want = ref.reference("octahedron", axis)
        got = mesh.voxelize(v.astype(np.float32), f.astype(np.int64), cube.astype(np.int64), D, stride, axis=name)
        assert np.array_equal(got["occ"], want["occ"]) and np.array_equal(got["solid"], (want["occ"] & 1) != 0) and np.array_equal(got["surface"], (want["occ"] & 2) != 0)
        assert np.array_equal(got["n_solid"], want["per_cube"][:, 0]) and np.array_equal(got["n_surface"], want["per_cube"][:, 1])
        assert [got[k] for k in mesh.VOXEL_COUNTS[:6]] == want["counts"][:6].tolist()
        for mode, bits in (("solid", 1), ("surface", 2), (("surface", "solid"), 3)):
            assert np.array_equal(mesh.voxelize(v, f, cube, D, stride, mode=mode, axis=axis)["occ"], want["occ"] & bits)
        for select, bits in (("surface", 2), ("solid", 1), ("either", 3)):
            Y = groundTruth.gt_cubes_from_mesh(v, f, cube, D, stride, select=select, axis=name)
            assert Y.dtype == np.float32 and np.array_equal(Y, ((want["occ"] & bits) != 0).astype(np.float32)[:, None])
            ijk, mask = mesh.occupancy_lists(want["occ"], select)
            assert len(ijk) == len(mask) == cube.shape[0] and all(a.dtype == np.uint8 and a.shape == (len(m), 3) and m.dtype == bool and m.all() for a, m in zip(ijk, mask))
            for n in (0, 21, 63):
                back = np.zeros((D, D, D), bool)
                back[tuple(ijk[n].T.astype(np.int64))] = True
                assert np.array_equal(back, (want["occ"][n] & bits) != 0) and len(np.unique(ijk[n], axis=0)) == len(ijk[n])
    assert np.array_equal(mesh.voxelize(v, f, cube, D, stride)["occ"], ref.reference("octahedron", 2)["occ"])      # both bits, axis = 2 by default


# ---- the ABI: symbols are only added ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_version_script_binding_and_makefile():
    import ctypes
    import fnmatch
    import re
    from surfacenet_amd import _lib
    new = ("sn_mesh_voxelize", "sn_mesh_voxelize_dev")
    txt = open(os.path.join(ROOT, "include", "surfacenet_hip.h")).read()
    assert "#define SN_ABI_VERSION 2" in txt and "sn_mesh_voxelize_cfg" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    additions = re.search(r"Added since, without a version change.*?\*/", txt, flags=re.S).group(0)
    pattern = re.search(r"global:\s*([^;]+);", open(os.path.join(CSRC, "exports.map")).read()).group(1).strip()
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert re.search(r"\b%s\b" % name, additions), name
        assert fnmatch.fnmatchcase(name, pattern), (name, pattern)
        assert name in _lib.ABI_SYMBOLS, name
    assert re.search(r"typedef struct sn_mesh_voxelize_cfg \{\s*int axis;[^}]*int modes;[^}]*int select;[^}]*int reserved;[^}]*\} sn_mesh_voxelize_cfg;", code)
    assert "sn_meshvoxel.hip" in open(os.path.join(CSRC, "Makefile")).read()
    assert ctypes.sizeof(_lib.MeshVoxelizeCfg) == 16 and [n for n, _ in _lib.MeshVoxelizeCfg._fields_] == ["axis", "modes", "select", "reserved"]
    from surfacenet_amd import Context, groundTruth, mesh
    assert all(callable(getattr(mesh, n)) for n in ("voxelize", "check_voxelize_args", "occupancy_lists")) and callable(Context.mesh_voxelize)
    assert callable(groundTruth.gt_cubes_from_mesh)


def test_the_rules_header_is_hip_free():
    with open(os.path.join(CSRC, "meshvoxel_rules.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes and all("hip/" not in i and i in ("<stdint.h>", '"meshwinding_rules.h"') for i in includes), includes
    with open(os.path.join(CSRC, "meshvoxel.h")) as f:
        txt = f.read()
    assert '#include "meshvoxel_rules.h"' in txt and '#include "meshwinding.h"' in txt
    assert "mxi_pick_level" not in txt and "lt_claim" not in txt      # the grid's level, table and scatter are the winding stage's, not a third copy


# ---- the rules and the argument checks of the C entry, on the CPU ----------------------------------------------------------------------------------------
def test_rules_and_argument_checks_under_sanitizers(tmp_path):
    """tests/host/meshvoxel_check.cpp runs csrc/meshvoxel_rules.h - the columns of an interval, K at the ends of the magnitudes, the solid and
    the surface rule on a triangle across the whole range - and sn_host.h's vox_check_args over every end of every range, compiled
    stand-alone with -fsanitize=address,undefined and run as a child process. (voxel, triangle) rows go in as integers - the triangles of
    the cube, the octahedron, the slivers, the degenerate set and the clipping test's pairs against the first centres of columns - and what
    comes back, s, K and the box test, equals the restatement row by row."""
    rows = []
    for name in ("cube", "octahedron", "sliver", "degenerate"):
        v, f, cube, D, stride = ref.CASES[name]()
        q = np.rint(np.nan_to_num(v) * FIX).astype(np.int64)
        cells = ref.world_cells(cube[[0, 13, 26]], D, stride)[:, :, :, 0].reshape(-1, 3)[::3]
        for n, t in enumerate(wr.triangles(f).tolist()):
            for k, g in enumerate(cells.tolist()):
                axis = (n + k) % 3
                p = [x * FIX for x in g]
                rows.append([axis, 1 + (n * 7 + k) % 64] + p + q[t[0]].tolist() + q[t[1]].tolist() + q[t[2]].tolist())
    for k, t in enumerate(_pairs()[::3].tolist()):
        rows.append([k % 3, 1 + k % 64, 0, 0, 0] + t[0] + t[1] + t[2])
    assert len(rows) > 3000
    want = []
    for row in rows:
        axis, D = row[:2]
        p, a, b, c = (tuple(row[2 + 3 * i:5 + 3 * i]) for i in range(4))
        n = wr._normal(a, b, c, lambda x: x)
        touches = n != (0, 0, 0) and bool(ref.sat(np.asarray([[[x - y for x, y in zip(corner, p)] for corner in (a, b, c)]], object), n)[0])
        x = np.asarray([a, b, c], np.float64) / FIX             # (exact: |q| < 2^38)
        col = np.asarray([p] * D, np.float64) / FIX
        col[:, axis] += np.arange(D)
        w = wr.winding(x, [[0, 1, 2]], col, axis)["winding"]
        K = int((w != 0).sum())
        assert K == 0 or (w[:K] == w[0]).all()                  # a prefix of the column
        want.append("%d %d %d" % (int(w[0]), K, touches))
    assert {w.split()[0] for w in want} == {"-1", "0", "1"} and len({w.split()[1] for w in want}) > 4 and 100 < sum(w.split()[2] == "1" for w in want) < len(want) - 100
    exe = str(tmp_path / "meshvoxel_check")
    _compile(os.path.join(ROOT, "tests", "host", "meshvoxel_check.cpp"), exe)
    text = "".join(" ".join("%d" % x for x in row) + "\n" for row in rows)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "MESHVOXEL-CHECK-OK %d rows" % len(rows) in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    got = p.stdout.splitlines()[:len(rows)]
    for i, line in enumerate(got):
        assert line == want[i], (i, rows[i], line, want[i])
