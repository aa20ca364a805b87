"""GPU (-m gpu): the winding-number stage (surfacenet_amd/csrc/meshwinding.h) against the restatement
tests/meshwinding_ref.py, byte for byte - winding, crossings, on_surface and the counts but counts[4], the broad phase's own number -, in
the host form and the device form and along every axis: the named cases, the grid level forced in the test-only twin, colliding keys at a
forced level, the edge forms, the refusals, repeated calls on one context, and the Python layers above the entry. Every launch is a plain
bounded kernel. The solids stand ref.SHIFT whole cells up every axis (tests/test_meshwinding_cpu.py says why)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_refusals as bad
import meshwinding_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = (0, 1, 2)
DIRECT = tuple(n for n in ref.CASES if n != "late_columns")    # (late_columns is adversarial at its forced level: the child below)


@pytest.fixture(scope="module")
def ctx(gpu_required):
    from surfacenet_amd import runtime
    return runtime.any_context()


def _check(ctx, v, f, pts, axis, want):
    for device in (False, True):
        got = ctx.mesh_winding(v, f, pts, axis=axis, device=device)
        assert [got[k].dtype for k in ref.KEYS] == [np.int32, np.int32, np.uint8, np.int64]
        assert ref.same_bytes(got, want) == [], (axis, device, ref.same_bytes(got, want), got["counts"].tolist(), want["counts"].tolist())
    return got


def _bits(r):
    return {k: (np.delete(np.asarray(r[k]), 4) if k == "counts" else np.asarray(r[k])).tobytes() for k in ref.KEYS}


@pytest.mark.parametrize("name", DIRECT)
def test_byte_for_byte_against_the_restatement(ctx, name):
    v, f, pts = ref.CASES[name]()
    for axis in AXES:
        want = ref.reference(name, axis)
        got = _check(ctx, v, f, pts, axis, want)
        assert got["counts"][4] >= want["crossings"].sum()      # every crossing was a test
    if name in ("cube", "octahedron"):
        assert pts.shape[0] == 2 * 1331
        inside, on = (ref.cube_where if name == "cube" else ref.octahedron_where)(pts - ref.SHIFT)
        assert np.array_equal(got["on_surface"].astype(bool), on) and np.array_equal(got["winding"][~on], inside[~on].astype(np.int32))
    if name == "many":
        assert pts.shape[0] == 531441 > 2048 * 256              # more queries than the lanes of the largest grid: a second trip of the loop
    if name == "degenerate":
        assert want["counts"][:3].tolist() == [4, 9, 4] and np.isnan(v[18, 0])      # axis 2: the sliver is parallel to the rays
        assert ref.reference(name, 0)["counts"][:3].tolist() == [5, 8, 4]
    if name == "big_and_small":
        assert f.shape[0] == 401 and (want["crossings"] == 2).any()
    if name == "far":
        inside, on = ref.cube_where(pts, ref.FAR_LO, ref.FAR_HI)
        assert np.array_equal(got["on_surface"].astype(bool), on) and np.array_equal(got["winding"][~on], inside[~on].astype(np.int32))
    if name == "nested_reversed":
        assert (want["crossings"][want["winding"] == 0] == 2).any()
    if name == "open_cube":
        assert ref.same_bytes(ref.reference(name, 0), want, ("winding",)) == ["winding"]


def test_the_shell_oriented_outward_winds_once_around_its_centre(ctx):
    from surfacenet_amd import mesh
    v, q, pts = ref.CASES["shell_q"]()
    assert mesh.smooth_mesh(v, q, iterations=0)["n_boundary_edges"] == 0
    o = mesh.orient_mesh(v, q, sign="outward")
    assert o["n_inconsistent"] == 0 and o["n_closed"] == o["n_components"] == 1 and o["faces"].shape == q.shape
    centre = pts.shape[0] - 1
    assert pts[centre].tolist() == [20.0, 20.0, 20.0]
    seen = []
    for faces in (o["faces"], mesh.triangulate(o["faces"]).astype(np.int32)):
        for axis in AXES:
            want = ref.winding(v, faces, pts, axis)
            got = _check(ctx, v, faces, pts, axis, want)
            assert got["winding"][centre] == 1 and set(got["winding"].tolist()) == {0, 1}
            seen.append((got["winding"].tobytes(), got["crossings"].tobytes(), got["on_surface"].tobytes()))
    free = np.frombuffer(seen[0][2], np.uint8) == 0
    wind = [np.frombuffer(s[0], np.int32) for s in seen]
    assert all(np.array_equal(w[free], wind[0][free]) for w in wind) and all(s[2] == seen[0][2] for s in seen)      # the axes agree; quads = triangles
    assert seen[:3] == seen[3:]


@pytest.mark.parametrize("name,levels", [("shell_q", (None, 0, "chosen+3", ref.LEVELS - 1)), ("late_columns", (0,))])
def test_the_result_does_not_depend_on_the_grid_level(gpu_required, tmp_path, name, levels):
    """SN_WND_LEVEL forces the level in the test-only twin (read once per call; one child process per level): the finest, three above the one
    the stage picks, and the coarsest - every triangle in one cell. late_columns: 200 one-triangle columns whose cells' keys are late
    (tests/hash_adversary.py) at level 0, where a grid cell is the unit cell, so that every key of the table starts its walk in the table's
    last sixteen slots."""
    v, f, pts = ref.CASES[name]()
    want = ref.reference(name)
    chosen, _ = ref.grid_level(v, f)
    if name == "late_columns":
        import hash_adversary as ha
        cells = ref.late_columns()[3]
        assert cells.shape == (ref.LATE_N, 2) and np.array_equal(np.floor(v[f[:, 0]][:, :2]).astype(np.int64) + ref.CELL_OFFSET, cells)
        keys = ha.lt_key(cells[:, 0], cells[:, 1], np.zeros((ref.LATE_N,), np.int64))
        assert ha.table_cap(ref.BUDGET * f.shape[0], 2, 1024) == 4096 and ha.late_mask(keys, ha.W, 12).all() and np.unique(keys).size == ref.LATE_N
        assert ref.grid_level(v, f) == (0, ref.LATE_N)
        assert want["counts"][3] == 2 * ref.LATE_N and want["counts"][5] == ref.LATE_N
    tests = []
    for level in levels:
        level = chosen + 3 if level == "chosen+3" else level
        env = dict(os.environ, SURFACENET_HIP_LIB=os.path.join(ROOT, "surfacenet_amd", "libsurfacenet_hip_dbg.so"))      # the switch exists in the twin alone
        env.pop("SN_WND_LEVEL", None)
        if level is not None:
            env["SN_WND_LEVEL"] = str(level)
        out = str(tmp_path / ("level_%s.npz" % level))
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "bench_meshwinding.py"), "--case", name, "--save", out], env=env, cwd=ROOT)
        got = np.load(out)
        assert ref.same_bytes(got, want) == [], (level, ref.same_bytes(got, want), got["counts"].tolist())
        tests.append(int(got["counts"][4]))
    if name == "shell_q":
        assert chosen + 3 < ref.LEVELS - 1 and tests[3] == max(tests) and len(set(tests)) > 2      # (the levels were not all one level)
        assert tests[3] == int(want["counts"][:2].sum()) * pts.shape[0]                           # level 21: every triangle in one cell, every query looks at all of them
    else:
        assert tests[0] > 0


def test_edge_forms(ctx):
    v, f, pts = ref.CASES["degenerate"]()                       # (its vertex 18 is unreferenced and not a number)
    none_f, none_p = np.zeros((0, 3), np.int32), np.zeros((0, 3))
    for device in (False, True):
        for axis in AXES:
            want = ref.reference("degenerate", axis)
            e = ctx.mesh_winding(v, none_f, pts, axis=axis, device=device)      # no face: all zeros, the NaN vertex not looked at
            assert ref.same_bytes(e, ref.winding(v, none_f, pts, axis)) == [] and not e["counts"].any() and not e["winding"].any() and not e["on_surface"].any()
            e = ctx.mesh_winding(np.zeros((0, 3)), np.zeros((0, 4), np.int32), pts, axis=axis, device=device)      # no vertex
            assert e["winding"].shape == (pts.shape[0],) and not e["winding"].any() and not e["crossings"].any() and not e["counts"].any()
            e = ctx.mesh_winding(v, f, none_p, axis=axis, device=device)         # no query: the mesh is checked and counted
            assert e["winding"].shape == (0,) and e["on_surface"].shape == (0,) and e["counts"].tolist() == want["counts"][:3].tolist() + [0] * 5
        want = ref.reference("degenerate", 1)
        for outputs in (("crossings", "on_surface"), ("winding", "on_surface"), ("winding", "crossings"), ()):      # each output NULL in turn, and all of them
            got = ctx.mesh_winding(v, f, pts, axis=1, outputs=outputs, device=device)
            assert set(got) == set(outputs) | {"counts"} and ref.same_bytes(got, want, outputs + ("counts",)) == []
        with pytest.raises(ValueError, match="face 0 names a vertex outside"):
            ref.winding(np.zeros((0, 3)), f, none_p)


def test_refusals_leave_the_outputs_and_the_context_alone(ctx):
    from surfacenet_amd import _lib, SurfaceNetHipError
    v, f = bad.sheet(51)
    pts = np.ascontiguousarray(v[::7] + [0.25, 0.25, -1.0])
    before = {device: _bits(ctx.mesh_winding(v, f, pts, device=device)) for device in (False, True)}
    assert before[False] == before[True] == _bits(ref.winding(v, f, pts)) and ref.winding(v, f, pts)["winding"].any()
    bv, bf, text = bad.bad_index(v, f, 257, 280)
    cv, cf, ctext = bad.bad_coordinate(v, f, 257, np.nan)
    hv, hf, htext = bad.bad_coordinate(v, f, 257, 2097144.0)
    outp = pts.copy()
    outp[5, 1], outp[9, 0] = np.nan, -4.5
    lowp = pts.copy()
    lowp[9, 2] = 2097144.0
    cases = [(bv, bf, pts, text), (cv, cf, pts, ctext), (hv, hf, pts, htext), (cv, bad.bad_index(v, f, 280, 280)[1], pts, ctext),      # the smaller face is the one named
             (v, f, outp, ref.POINT_TEXT % 5), (v, f, lowp, ref.POINT_TEXT % 9), (bv, bf, outp, text)]                              # the mesh before the queries
    for cv_, cf_, cp, words in cases:
        said = set()
        for device in (False, True):
            with pytest.raises(SurfaceNetHipError) as e:
                ctx.mesh_winding(cv_, cf_, cp, device=device)
            said.add(str(e.value))
            with pytest.raises(ValueError) as r:
                ref.winding(cv_, cf_, cp)
            assert str(r.value) == words
        assert len(said) == 1 and words in said.pop(), (words, said)
    for axis in (-1, 3):
        for device in (False, True):
            with pytest.raises(SurfaceNetHipError, match="axis = %d: 0 \\(x\\), 1 \\(y\\) or 2 \\(z\\)" % axis):
                ctx.mesh_winding(v, f, pts, axis=axis, device=device)
    # the host form, called directly: a refusal writes nothing but zero counts - bad mesh, bad query, bad axis, null cfg, too many triangles
    lib = _lib.load()
    n = pts.shape[0]
    good_v, bv, bf = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(bv, np.float64), np.ascontiguousarray(bf, np.int32)
    cv = np.ascontiguousarray(cv, np.float64)
    for cfg, vv, ff, pp, F in ((_lib.MeshWindingCfg(2, 0), bv, bf, pts, None), (_lib.MeshWindingCfg(2, 0), cv, f, pts, None), (_lib.MeshWindingCfg(0, 0), good_v, f, outp, None),
                               (_lib.MeshWindingCfg(3, 0), good_v, f, pts, None), (None, good_v, f, pts, None), (_lib.MeshWindingCfg(1, 0), good_v, f, pts, (1 << 26) + 1)):
        wind, cross, on = np.full((n,), 7, np.int32), np.full((n,), 7, np.int32), np.full((n,), 7, np.uint8)
        counts = (ctypes.c_longlong * 8)(*([9] * 8))
        rc = lib.sn_mesh_winding(ctx._h, None if cfg is None else ctypes.byref(cfg), vv.shape[0], _lib.ptr(vv), ff.shape[0] if F is None else F, 3, _lib.ptr(ff), n,
                                 _lib.ptr(pp), _lib.ptr(wind), _lib.ptr(cross), _lib.ptr(on), counts)
        assert rc == -1 and list(counts) == [0] * 8 and (wind == 7).all() and (cross == 7).all() and (on == 7).all()
    assert "triangles: at most 2^26" in _lib.last_error()
    assert {device: _bits(ctx.mesh_winding(v, f, pts, device=device)) for device in (False, True)} == before      # the context is usable


def test_run_twice_then_grow_the_workspace_and_come_back(gpu_required):
    import surfacenet_amd
    small, large = ref.CASES["degenerate"](), ref.CASES["shell_q"]()
    fresh = {}
    for name, case in (("small", small), ("large", large)):
        with surfacenet_amd.Context(max_samples=1) as c:
            fresh[name] = _bits(c.mesh_winding(*case))
    assert fresh["small"] == _bits(ref.reference("degenerate")) and fresh["large"] == _bits(ref.reference("shell_q"))
    with surfacenet_amd.Context(max_samples=1) as c:
        assert _bits(c.mesh_winding(*small)) == fresh["small"] and _bits(c.mesh_winding(*small)) == fresh["small"]
        assert _bits(c.mesh_winding(*large)) == fresh["large"]
        assert _bits(c.mesh_winding(*small)) == fresh["small"] and _bits(c.mesh_winding(*small, device=True)) == fresh["small"]
        assert _bits(c.mesh_winding(*large, device=True)) == fresh["large"]


def test_python_layers(ctx):
    from surfacenet_amd import mesh
    v, q, pts = ref.CASES["shell_q"]()
    for axis, name in ((0, "x"), (2, 2)):
        want = ref.reference("shell_q", axis)
        got = mesh.winding_number(pts, v, q.astype(np.int64), axis=name)
        assert np.array_equal(got["winding"], want["winding"]) and np.array_equal(got["crossings"], want["crossings"]) and np.array_equal(got["inside"], want["winding"] != 0)
        assert np.array_equal(got["on_surface"], want["on_surface"].astype(bool)) and [got[k] for k in mesh.WINDING_COUNTS] == want["counts"][[0, 1, 2, 3, 5]].tolist()
    # signed_distance equals the two restatements composed
    v, f, pts = ref.CASES["cube"]()
    for axis in AXES:
        got = mesh.signed_distance(pts, v, f, max_dist=1.25, axis=axis, resol=0.4)
        want = ref.signed_distance(v, f, pts, 1.25, axis, 0.4)
        assert all(np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes() for k in ("dist", "face", "closest", "winding", "on_surface"))
        inside, on = ref.cube_where(pts - ref.SHIFT)
        assert (got["dist"][on] == 0.0).all() and (got["dist"][inside] < 0).all() and (got["dist"][~inside & ~on] > 0).all()
    v, q, pts = ref.CASES["shell_q"]()
    got, want = mesh.signed_distance(pts, v, q, max_dist=2.5), ref.signed_distance(v, q, pts, 2.5)
    assert all(np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes() for k in ("dist", "face", "closest", "winding", "on_surface"))
    assert (got["dist"] < 0).sum() > 100 and (got["dist"] == 2.5).any()
