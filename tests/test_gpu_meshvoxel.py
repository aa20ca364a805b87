"""GPU (-m gpu): the mesh voxelisation stage (surfacenet_amd/csrc/meshvoxel.h) against the restatement
tests/meshvoxel_ref.py, byte for byte - occ, Y, per_cube and the counts but counts[6] and counts[7], the broad phase's own numbers -, in
the host form and the device form and along every axis: the named cases at D = 8 and 12 in overlapping cubes, one cube of D = 64 around the
shell (the LDS maximum, every slab), 8 cubes of D = 32 against Context.mesh_winding on the same centres, the grid level forced in the
test-only twin, colliding keys at a forced level, the edge forms, the refusals, repeated calls on one context, and the Python layers above
the entry. Every launch is a plain bounded kernel."""
import ctypes
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import mesh_refusals as bad
import meshvoxel_ref as ref
import meshwinding_ref as wr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = (0, 1, 2)
DIRECT = tuple(n for n in ref.CASES if n != "late_columns")    # (late_columns is adversarial at its forced level: the child below)


@pytest.fixture(scope="module")
def ctx(gpu_required):
    from surfacenet_amd import runtime
    return runtime.any_context()


def _check(ctx, case, axis, want, **kw):
    for device in (False, True):
        got = ctx.mesh_voxelize(*case, axis=axis, device=device, **kw)
        assert [got[k].dtype for k in ref.KEYS] == [np.uint8, np.float32, np.int64, np.int64]
        assert ref.same_bytes(got, want) == [], (axis, device, ref.same_bytes(got, want), got["counts"].tolist(), want["counts"].tolist())
    return got


def _bits(r):
    return {k: (np.asarray(r[k])[:6] if k == "counts" else np.asarray(r[k])).tobytes() for k in ref.KEYS}


def _centres(cube, D, stride):
    return np.ascontiguousarray(ref.world_cells(cube, D, stride).reshape(-1, 3).astype(np.float64))


@pytest.mark.parametrize("name", DIRECT)
def test_byte_for_byte_against_the_restatement(ctx, name):
    case = ref.CASES[name]()
    v, f, cube, D, stride = case
    assert D in (8, 12) and stride < D                          # the cubes overlap
    for axis in AXES:
        want = ref.reference(name, axis)
        got = _check(ctx, case, axis, want)
        assert got["counts"][6] > 0 and got["counts"][7] > 0
    if name in ("cube", "octahedron"):
        per_cube = ref.reference(name)["per_cube"]
        assert (per_cube.sum(axis=1) == 0).sum() >= 7 and (per_cube[:, 0] > 0).any()      # cubes wholly above, below and beside the mesh
    if name == "nested_same":
        assert (wr.winding(v, f, _centres(cube[21:22], D, stride), 2)["winding"] == 2).any()
    if name == "degenerate":
        assert ref.reference(name)["counts"][:3].tolist() == [4, 9, 4] and np.isnan(v[18, 0])
    if name == "big_and_small":
        assert f.shape[0] == 401
    # the bits one by one, and either bit as the target
    want = ref.reference(name, 1)
    for modes, select in ((1, 1), (2, 2), (3, 3), (3, 1)):
        r = ref.voxelize(v, f, cube, D, stride, 1, modes=modes, select=select)
        assert np.array_equal(r["occ"], want["occ"] & modes)
        _check(ctx, case, 1, r, modes=modes, select=select)


def test_one_cube_of_64_around_the_shell_and_its_volume(ctx):
    """D = 64: the most LDS a workgroup asks for, 22 slabs of which the last is short; D a multiple of 16: the 16-byte stores. Oriented
    outward the shell is closed, consistently turned and free of self-intersections: |volume - #solid| <= #surface."""
    from surfacenet_amd import mesh
    v, q, _ = wr.CASES["shell_q"]()
    o = mesh.orient_mesh(v, q, sign="outward")
    assert o["n_inconsistent"] == 0 and o["n_closed"] == o["n_components"] == 1 and mesh.self_intersections(v, o["faces"])["n_pairs"] == 0
    q = np.ascontiguousarray(o["faces"], np.int32)
    cube, D, stride = np.asarray([[0, 0, 0]], np.int32), 64, 64
    assert v[np.unique(q)].min() > 1 and v[np.unique(q)].max() < 62
    cells = ref.world_cells(cube, D, stride).reshape(-1, 3)
    surf, _ = ref.surface_cells(v, q, cells)
    volume = Fraction(mesh.mesh_normals(v, q)["vol6"], 6 << 48)    # mesh_normals' exact volume, in cells^3
    assert volume > 500
    seen = []
    for axis in AXES:
        inside = ctx.mesh_winding(v, q, cells.astype(np.float64), axis=axis, outputs=("winding",))["winding"] != 0
        occ = (inside.astype(np.uint8) | (surf.astype(np.uint8) << 1)).reshape(1, D, D, D)
        want = dict(occ=occ, Y=((occ & 2) != 0).astype(np.float32).reshape(1, 1, D, D, D), per_cube=np.asarray([[inside.sum(), surf.sum()]], np.int64))
        for faces in (q, mesh.triangulate(q).astype(np.int32)):
            for device in (False, True):
                got = ctx.mesh_voxelize(v, faces, cube, D, stride, axis=axis, device=device)
                assert ref.same_bytes(got, want, ("occ", "Y", "per_cube")) == [], (axis, device)
                assert got["counts"][3:6].tolist() == [int(inside.sum()), int(surf.sum()), int((occ == 3).sum())]
        n_solid, n_surface = int(inside.sum()), int(surf.sum())
        seen.append((n_solid, n_surface))
        print("axis %d: volume %.3f, %d solid, %d surface" % (axis, float(volume), n_solid, n_surface))
        assert abs(volume - n_solid) <= n_surface, (axis, float(volume), n_solid, n_surface)
    assert all(s[1] == seen[0][1] for s in seen) and seen[0][0] > 500
    # the first slabs against the whole restatement, through meshwinding_ref on their centres
    rows = cells.reshape(D, D, D, 3)[:7].reshape(-1, 3)
    w = wr.winding(v, q, rows.astype(np.float64), 2)["winding"] != 0
    assert np.array_equal(ctx.mesh_voxelize(v, q, cube, D, stride, axis=2, outputs=("occ",))["occ"][0, :7].reshape(-1) & 1, w.astype(np.uint8))


def test_eight_cubes_of_32_against_the_winding_stage_on_the_device(ctx):
    v, q, _ = wr.CASES["shell_q"]()
    cube, D, stride = ref.cube_grid(0, 1, 16), 32, 16
    centres = _centres(cube, D, stride)
    cells, inverse = np.unique(ref.world_cells(cube, D, stride).reshape(-1, 3), axis=0, return_inverse=True)
    surf = ref.surface_cells(v, q, cells)[0][np.asarray(inverse).reshape(-1)]
    for axis in AXES:
        w = ctx.mesh_winding(v, q, centres, axis=axis, outputs=("winding", "on_surface"), device=True)
        for device in (False, True):
            got = ctx.mesh_voxelize(v, q, cube, D, stride, axis=axis, device=device)
            assert np.array_equal(got["occ"].reshape(-1) & 1, (w["winding"] != 0).astype(np.uint8)) and (w["winding"] != 0).sum() > 1000
            assert np.array_equal((got["occ"].reshape(-1) >> 1) & 1, surf.astype(np.uint8))
            assert ((got["occ"].reshape(-1) & 2) != 0)[w["on_surface"] != 0].all()
            assert np.array_equal(got["per_cube"], np.stack([(got["occ"] & 1).reshape(8, -1).sum(axis=1), ((got["occ"] >> 1) & 1).reshape(8, -1).sum(axis=1)], axis=1))


@pytest.mark.parametrize("name,levels", [("shell_q", (None, 0, "chosen+3", wr.LEVELS - 1)), ("late_columns", (0,))])
def test_the_result_does_not_depend_on_the_grid_level(gpu_required, tmp_path, name, levels):
    """SN_VOX_LEVEL forces the level in the test-only twin (read once per call; one child process per level): the finest, three above the one
    the stage picks, and the coarsest - every triangle in one cell. late_columns: 200 one-triangle columns whose unit cells' keys are late
    (tests/hash_adversary.py) at level 0."""
    v, f, cube, D, stride = ref.CASES[name]()
    want = ref.reference(name)
    chosen, _ = ref.grid_level(v, f)
    if name == "late_columns":
        assert cube.shape == (wr.LATE_N, 3) and want["counts"][4] > wr.LATE_N and ref.grid_level(v, f, budget=1 << 20)[0] == 0
    tests = []
    for level in levels:
        level = chosen + 3 if level == "chosen+3" else level
        env = dict(os.environ, SURFACENET_HIP_LIB=os.path.join(ROOT, "surfacenet_amd", "libsurfacenet_hip_dbg.so"))      # the switch exists in the twin alone
        env.pop("SN_VOX_LEVEL", None)
        if level is not None:
            env["SN_VOX_LEVEL"] = str(level)
        out = str(tmp_path / ("level_%s.npz" % level))
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "bench_meshvoxel.py"), "--case", name, "--save", out], env=env, cwd=ROOT)
        got = np.load(out)
        assert ref.same_bytes(got, want) == [], (level, ref.same_bytes(got, want), got["counts"].tolist())
        tests.append((int(got["counts"][6]), int(got["counts"][7])))
    if name == "shell_q":
        assert chosen + 3 < wr.LEVELS - 1 and len(set(tests)) == 1      # a (column, triangle) pair is met once at every level: the work is the same
    assert tests[0][0] > 0 and tests[0][1] > 0


def test_edge_forms(ctx):
    v, f, cube, D, stride = ref.CASES["degenerate"]()           # (its vertex 18 is unreferenced and not a number)
    none_f, none_c = np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32)
    for device in (False, True):
        for axis in AXES:
            want = ref.reference("degenerate", axis)
            e = ctx.mesh_voxelize(v, none_f, cube, D, stride, axis=axis, device=device)      # no face: all zeros, the NaN vertex not looked at
            assert ref.same_bytes(e, ref.voxelize(v, none_f, cube, D, stride, axis)) == [] and not e["counts"].any() and not e["occ"].any() and not e["Y"].any()
            e = ctx.mesh_voxelize(np.zeros((0, 3)), np.zeros((0, 4), np.int32), cube, D, stride, axis=axis, device=device)      # no vertex
            assert e["occ"].shape == (27, 8, 8, 8) and not e["occ"].any() and not e["per_cube"].any() and not e["counts"].any()
            e = ctx.mesh_voxelize(v, f, none_c, D, stride, axis=axis, device=device)          # no cube: the mesh is checked and counted
            assert e["occ"].shape == (0, 8, 8, 8) and e["Y"].shape == (0, 1, 8, 8, 8) and e["counts"].tolist() == want["counts"][:3].tolist() + [0] * 5
            # D = 1: a cube is one voxel
            one = ref.world_cells(cube[13:14], D, stride).reshape(-1, 3).astype(np.int32)
            r = ref.voxelize(v, f, one, 1, 1, axis)
            got = ctx.mesh_voxelize(v, f, one, 1, 1, axis=axis, device=device)
            assert ref.same_bytes(got, r) == [] and np.array_equal(got["occ"].reshape(8, 8, 8), want["occ"][13]) and got["occ"].any()
        want = ref.reference("degenerate", 1)
        for outputs in (("Y", "per_cube"), ("occ", "per_cube"), ("occ", "Y"), ()):      # each output NULL in turn, and all of them
            got = ctx.mesh_voxelize(v, f, cube, D, stride, axis=1, outputs=outputs, device=device)
            assert set(got) == set(outputs) | {"counts"} and ref.same_bytes(got, want, outputs + ("counts",)) == []


def test_refusals_leave_the_outputs_and_the_context_alone(ctx):
    from surfacenet_amd import _lib, SurfaceNetHipError
    v, f = bad.sheet(51)
    cube, D, stride = np.asarray([[0, 0, 0], [1, 2, 0], [3, 3, 1]], np.int32), 8, 4
    want = ref.voxelize(v, f, cube, D, stride)
    before = {device: _bits(ctx.mesh_voxelize(v, f, cube, D, stride, device=device)) for device in (False, True)}
    assert before[False] == before[True] == _bits(want) and want["occ"].any()
    bv, bf, text = bad.bad_index(v, f, 257, 280)
    cv, cf, ctext = bad.bad_coordinate(v, f, 257, np.nan)
    neg, far = cube.copy(), cube.copy()
    neg[2, 1], neg[1, 0], far[1, 2] = -1, (2097144 - 8) // 4 + 1, (2097144 - 8) // 4 + 1
    cases = [(bv, bf, cube, text), (cv, cf, cube, ctext), (cv, bad.bad_index(v, f, 280, 280)[1], cube, ctext),      # the smaller face is the one named
             (v, f, neg, ref.REACH_TEXT % 1), (v, f, far, ref.REACH_TEXT % 1), (bv, bf, neg, text)]                  # the first bad cube; the mesh before the cubes
    neg2 = cube.copy()
    neg2[0, 2] = -5
    cases.append((v, f, neg2, ref.NEGATIVE_TEXT % 0))
    for cv_, cf_, cc, words in cases:
        said = set()
        for device in (False, True):
            with pytest.raises(SurfaceNetHipError) as e:
                ctx.mesh_voxelize(cv_, cf_, cc, D, stride, device=device)
            said.add(str(e.value))
            with pytest.raises(ValueError) as r:
                ref.voxelize(cv_, cf_, cc, D, stride)
            assert str(r.value) == words
        assert len(said) == 1 and words in said.pop(), (words, said)
    for kw, words in ((dict(axis=3), "axis = 3: 0 \\(x\\), 1 \\(y\\) or 2 \\(z\\)"), (dict(axis=-1), "axis = -1"), (dict(modes=0), "modes = 0"), (dict(modes=4), "modes = 4"),
                      (dict(select=0), "select = 0"), (dict(select=4), "select = 4")):
        for device in (False, True):
            with pytest.raises(SurfaceNetHipError, match=words):
                ctx.mesh_voxelize(v, f, cube, D, stride, device=device, **kw)
    # the host form, called directly: a refusal writes nothing but zero counts
    lib = _lib.load()
    N = cube.shape[0]
    good_v, bv, bf = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(bv, np.float64), np.ascontiguousarray(bf, np.int32)
    cv = np.ascontiguousarray(cv, np.float64)
    ok = _lib.MeshVoxelizeCfg(2, 3, 2, 0)
    rows = ((ok, bv, bf, cube, D, stride, None, N), (ok, cv, f, cube, D, stride, None, N), (ok, good_v, f, neg, D, stride, None, N), (ok, good_v, f, far, D, stride, None, N),
            (_lib.MeshVoxelizeCfg(3, 3, 2, 0), good_v, f, cube, D, stride, None, N), (_lib.MeshVoxelizeCfg(2, 0, 2, 0), good_v, f, cube, D, stride, None, N),
            (_lib.MeshVoxelizeCfg(2, 3, 4, 0), good_v, f, cube, D, stride, None, N), (None, good_v, f, cube, D, stride, None, N),
            (ok, good_v, f, cube, 0, stride, None, N), (ok, good_v, f, cube, 65, stride, None, N), (ok, good_v, f, cube, D, 0, None, N), (ok, good_v, f, cube, D, stride, None, -1),
            (ok, good_v, f, cube, D, stride, (1 << 26) + 1, N), (ok, good_v, f, cube, 64, stride, None, (1 << 15) + 1))
    for cfg, vv, ff, cc, d, s, F, n_cubes in rows:
        occ, Y, per = np.full((N, D, D, D), 7, np.uint8), np.full((N, 1, D, D, D), 7, np.float32), np.full((N, 2), 7, np.int64)
        counts = (ctypes.c_longlong * 8)(*([9] * 8))
        rc = lib.sn_mesh_voxelize(ctx._h, None if cfg is None else ctypes.byref(cfg), vv.shape[0], _lib.ptr(vv), ff.shape[0] if F is None else F, 3, _lib.ptr(ff), n_cubes,
                                  _lib.ptr(np.ascontiguousarray(cc)), d, s, _lib.ptr(occ), _lib.ptr(Y), _lib.ptr(per), counts)
        assert rc == -1 and list(counts) == [0] * 8 and (occ == 7).all() and (Y == 7).all() and (per == 7).all(), (d, s, F, n_cubes)
    assert "voxels: at most 2^33" in _lib.last_error()
    assert {device: _bits(ctx.mesh_voxelize(v, f, cube, D, stride, device=device)) for device in (False, True)} == before      # the context is usable


def test_run_twice_then_grow_the_workspace_and_come_back(gpu_required):
    import surfacenet_amd
    small = ref.CASES["degenerate"]()
    v, q, _ = wr.CASES["shell_q"]()
    large = (v, q, ref.cube_grid(0, 1, 16), 32, 16)
    fresh = {}
    for name, case in (("small", small), ("large", large)):
        with surfacenet_amd.Context(max_samples=1) as c:
            fresh[name] = _bits(c.mesh_voxelize(*case))
    assert fresh["small"] == _bits(ref.reference("degenerate"))
    with surfacenet_amd.Context(max_samples=1) as c:
        assert _bits(c.mesh_voxelize(*small)) == fresh["small"] and _bits(c.mesh_voxelize(*small)) == fresh["small"]
        assert _bits(c.mesh_voxelize(*large)) == fresh["large"]
        assert _bits(c.mesh_voxelize(*small)) == fresh["small"] and _bits(c.mesh_voxelize(*small, device=True)) == fresh["small"]
        assert _bits(c.mesh_voxelize(*large, device=True)) == fresh["large"]


def test_python_layers_and_the_round_trips(ctx):
    from surfacenet_amd import groundTruth, mesh, normals
    v, q, cube, D, stride = ref.CASES["shell_q"]()
    for axis, name in ((0, "x"), (2, 2)):
        want = ref.reference("shell_q", axis)
        got = mesh.voxelize(v, q.astype(np.int64), cube, D, stride, axis=name)
        assert np.array_equal(got["occ"], want["occ"]) and np.array_equal(got["solid"], (want["occ"] & 1) != 0) and np.array_equal(got["surface"], (want["occ"] & 2) != 0)
        assert np.array_equal(got["n_solid"], want["per_cube"][:, 0]) and np.array_equal(got["n_surface"], want["per_cube"][:, 1])
        assert [got[k] for k in mesh.VOXEL_COUNTS[:6]] == want["counts"][:6].tolist()
        for select, bits in (("surface", 2), ("solid", 1), ("either", 3)):
            Y = groundTruth.gt_cubes_from_mesh(v, q, cube, D, stride, select=select, axis=name)
            assert Y.dtype == np.float32 and np.array_equal(Y, ((want["occ"] & bits) != 0).astype(np.float32)[:, None])
    # occupancy_lists -> unique_voxels: the distinct set cells
    want = ref.reference("shell_q")
    for select, bits in (("surface", 2), ("solid", 1), ("either", 3)):
        ijk, mask = mesh.occupancy_lists(want["occ"], select)
        keep = normals.unique_voxels(cube, ijk, mask, stride)
        kept = np.concatenate([cube[n].astype(np.int64) * stride + a[k].astype(np.int64) for n, (a, k) in enumerate(zip(ijk, keep))])
        assert np.array_equal(np.unique(kept, axis=0), ref.distinct(want["occ"], cube, stride, bits)) and len(kept) == len(np.unique(kept, axis=0)) > 100
        assert sum(len(a) for a in ijk) > len(kept)               # the cubes overlap: some cell was listed twice
    # gt_cubes_from_mesh -> weighted_accuracy against itself
    cube32 = ref.cube_grid(0, 1, 16)
    Y = groundTruth.gt_cubes_from_mesh(v, q, cube32, 32, 16)
    assert Y.shape == (8, 1, 32, 32, 32) and 0 < Y.sum() < Y.size / 4
    assert groundTruth.weighted_accuracy(Y, Y) == 1.0
    assert groundTruth.weighted_accuracy(np.zeros_like(Y), Y) == 0.5
