"""GPU (-m gpu): the point-to-mesh distance stage (surfacenet_amd/csrc/meshdistance.h) against the restatement
tests/meshdistance_ref.py, bit for bit - d2, face, closest and the counts but counts[4], the broad phase's own number -, in the host form
and the device form: the named cases, the grid level forced in the test-only twin, colliding keys at a forced level, the edge forms,
the refusals, repeated calls on one context, and the Python layers above the entry. Every launch is a plain bounded kernel."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_refusals as bad
import meshdistance_ref as ref
import meshsample_ref as sref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECT = tuple(n for n in ref.CASES if n != "late_cells")      # (late_cells is adversarial at its forced level only: the child below)


@pytest.fixture(scope="module")
def ctx(gpu_required):
    from surfacenet_amd import runtime
    return runtime.any_context()


def _check(ctx, v, f, pts, max_dist, want):
    for device in (False, True):
        got = ctx.mesh_distance(v, f, pts, max_dist, device=device)
        assert [got[k].dtype for k in ref.KEYS] == [np.float64, np.int32, np.float64, np.int64]
        assert ref.same_bits(got, want) == [], (device, ref.same_bits(got, want), got["counts"].tolist(), want["counts"].tolist())
    return got


def _bits(r):
    return {k: (np.delete(np.asarray(r[k]), 4) if k == "counts" else np.asarray(r[k])).tobytes() for k in ref.KEYS}


@pytest.mark.parametrize("name", DIRECT)
def test_bit_for_bit_against_the_restatement(ctx, name):
    v, f, pts, max_dist = ref.CASES[name]()
    want = ref.reference(name)
    got = _check(ctx, v, f, pts, max_dist, want)
    assert got["counts"][4] >= want["counts"][2]                # every answered point met a triangle
    if name in ("shell", "shell_500"):
        V = ref.shell()[0].shape[0]
        assert (got["d2"][:V] == 0.0).all() and got["closest"][:V].tobytes() == np.ascontiguousarray(v).tobytes()      # its own vertices
        share = want["counts"][3] / pts.shape[0]
        assert 0.01 <= share <= 0.10 and pts.shape[0] > 1000     # the restatement alone puts 1 % .. 10 % beyond the cap
        assert got["counts"][4] < want["counts"][4] // 4         # the grid spares most of the brute force's tests
    if name == "many":
        assert pts.shape[0] > 2048 * 256                        # more queries than the lanes of the largest grid: a second trip of the loop
    if name == "far_hit":
        assert want["counts"][2:4].tolist() == [7, 0]
    if name == "far_miss":
        assert want["counts"][2:4].tolist() == [0, 7] and got["counts"][4] == 0      # no triangle was looked at
    if name == "fan":
        assert f.shape[0] == 300 and want["face"][0] == 0 and want["d2"][0] == 0.0      # the hub itself: the tie of all 300 goes to face 0
    if name == "degenerate":
        assert want["counts"][:2].tolist() == [4, 3]


@pytest.mark.parametrize("name,levels", [("shell", (None, 0, "chosen+3", ref.LEVELS - 1)), ("late_cells", (ref.LATE_LEVEL,))])
def test_the_result_does_not_depend_on_the_grid_level(gpu_required, tmp_path, name, levels):
    """SN_MDI_LEVEL forces the level in the test-only twin (read once per call; one child process per level): the finest, three above the one
    the stage picks, and the coarsest - every triangle in one cell. late_cells: tests/hash_adversary.py's late cells at the level where a
    grid cell is the unit cell, so that every key of the table starts its walk in the table's last sixteen slots."""
    v, f, pts, max_dist = ref.CASES[name]()
    want = ref.reference(name)
    chosen, _, _ = ref.grid_level(v, f, max_dist)
    if name == "late_cells":
        import hash_adversary as ha
        forced = ref.grid_level(v, f, max_dist, budget=1)
        assert forced[0] == ref.LATE_LEVEL and forced[2] == 1.0 and chosen != ref.LATE_LEVEL
        cells = np.floor(v[f[:ref.LATE_N, 0]]).astype(np.int64)
        cap = ha.table_cap(ref.BUDGET * f.shape[0], 2, 1024)
        assert np.array_equal(cells, ha.arranged_cells(ref.LATE_N)) and cap == 4096 and ha.late_mask(ha.keys_of_cells(cells), ha.W, 12).all()
    tests = []
    for level in levels:
        level = chosen + 3 if level == "chosen+3" else level
        env = dict(os.environ, SURFACENET_HIP_LIB=os.path.join(ROOT, "surfacenet_amd", "libsurfacenet_hip_dbg.so"))      # the switch exists in the twin alone
        env.pop("SN_MDI_LEVEL", None)
        if level is not None:
            env["SN_MDI_LEVEL"] = str(level)
        out = str(tmp_path / ("level_%s.npz" % level))
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "bench_meshdistance.py"), "--case", name, "--save", out], env=env, cwd=ROOT)
        got = np.load(out)
        assert ref.same_bits(got, want) == [], (level, ref.same_bits(got, want), got["counts"].tolist())
        tests.append(int(got["counts"][4]))
    if name == "shell":
        assert chosen + 3 < ref.LEVELS - 1 and tests[3] == max(tests) and len(set(tests)) > 2      # (the levels were not all one level)


def test_edge_forms(ctx):
    v, f, pts, max_dist = ref.CASES["degenerate"]()             # (its vertex 9 is unreferenced and not a number)
    want = ref.reference("degenerate")
    none_f, none_p = np.zeros((0, 3), np.int32), np.zeros((0, 3))
    for device in (False, True):
        e = ctx.mesh_distance(v, none_f, pts, max_dist, device=device)      # no face: every point beyond the cap, the NaN vertex not looked at
        assert ref.same_bits(e, ref.distance(v, none_f, pts, max_dist)) == [] and e["counts"].tolist() == [0, 0, 0, 9, 0, 0, 0, 0]
        e = ctx.mesh_distance(np.zeros((0, 3)), np.zeros((0, 4), np.int32), pts, max_dist, device=device)
        assert np.isinf(e["d2"]).all() and (e["face"] == -1).all() and np.isnan(e["closest"]).all()
        e = ctx.mesh_distance(v, f, none_p, max_dist, device=device)         # no point: the mesh is checked and counted
        assert e["d2"].shape == (0,) and e["closest"].shape == (0, 3) and e["counts"].tolist() == [4, 3, 0, 0, 0, 0, 0, 0]
        for outputs in (("face", "closest"), ("d2", "closest"), ("d2", "face"), ()):      # each output NULL in turn, and all of them
            got = ctx.mesh_distance(v, f, pts, max_dist, outputs=outputs, device=device)
            assert set(got) == set(outputs) | {"counts"} and ref.same_bits(got, want, outputs + ("counts",)) == []


def test_refusals_leave_the_outputs_and_the_context_alone(ctx):
    from surfacenet_amd import _lib, SurfaceNetHipError
    v, f = bad.sheet(51)
    pts = np.ascontiguousarray(v[::7] + [0.25, 0.25, 1.0])
    before = {device: _bits(ctx.mesh_distance(v, f, pts, 5.0, device=device)) for device in (False, True)}
    assert before[False] == before[True] == _bits(ref.distance(v, f, pts, 5.0))
    bv, bf, text = bad.bad_index(v, f, 257, 280)
    nanv = v.copy()
    nanv[bad.first_used_by(f, 257), 2] = np.inf
    nan_text = "face 257: a coordinate of one of its vertices is not finite"
    nanp = pts.copy()
    nanp[5, 1], nanp[9, 0] = np.nan, np.inf
    cases = [(bv, bf, pts, text), (nanv, f, pts, nan_text), (nanv, bad.bad_index(v, f, 280, 280)[1], pts, nan_text),      # the smaller face is the one named
             (v, f, nanp, "point 5: a coordinate is not finite")]
    for cv, cf, cp, words in cases:
        said = set()
        for device in (False, True):
            with pytest.raises(SurfaceNetHipError) as e:
                ctx.mesh_distance(cv, cf, cp, 5.0, device=device)
            said.add(str(e.value))
        assert len(said) == 1 and words in said.pop(), (words, said)
    for max_dist in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(SurfaceNetHipError, match="max_dist"):
            ctx.mesh_distance(v, f, pts, max_dist)
    # the host form, called directly: a refusal writes nothing but zero counts - bad mesh, bad point, bad cap, null cfg
    lib = _lib.load()
    n = pts.shape[0]
    good_v, bv, bf = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(bv, np.float64), np.ascontiguousarray(bf, np.int32)
    for cfg, vv, ff, pp in ((_lib.MeshDistanceCfg(5.0), bv, bf, pts), (_lib.MeshDistanceCfg(5.0), good_v, f, nanp), (_lib.MeshDistanceCfg(-1.0), good_v, f, pts),
                            (None, good_v, f, pts)):
        d2, face, closest = np.full((n,), 7.0), np.full((n,), 7, np.int32), np.full((n, 3), 7.0)
        counts = (ctypes.c_longlong * 8)(*([9] * 8))
        rc = lib.sn_mesh_distance(ctx._h, None if cfg is None else ctypes.byref(cfg), vv.shape[0], _lib.ptr(vv), ff.shape[0], 3, _lib.ptr(ff), n, _lib.ptr(pp),
                                  _lib.ptr(d2), _lib.ptr(face), _lib.ptr(closest), counts)
        assert rc == -1 and list(counts) == [0] * 8 and (d2 == 7.0).all() and (face == 7).all() and (closest == 7.0).all()
    assert {device: _bits(ctx.mesh_distance(v, f, pts, 5.0, device=device)) for device in (False, True)} == before      # the context is usable


def test_run_twice_then_grow_the_workspace_and_come_back(gpu_required):
    import surfacenet_amd
    small, large = ref.CASES["degenerate"](), ref.CASES["shell"]()
    fresh = {}
    for name, case in (("small", small), ("large", large)):
        with surfacenet_amd.Context(max_samples=1) as c:
            fresh[name] = _bits(c.mesh_distance(*case))
    assert fresh["small"] == _bits(ref.reference("degenerate")) and fresh["large"] == _bits(ref.reference("shell"))
    with surfacenet_amd.Context(max_samples=1) as c:
        assert _bits(c.mesh_distance(*small)) == fresh["small"] and _bits(c.mesh_distance(*small)) == fresh["small"]
        assert _bits(c.mesh_distance(*large)) == fresh["large"]
        assert _bits(c.mesh_distance(*small)) == fresh["small"] and _bits(c.mesh_distance(*small, device=True)) == fresh["small"]
        assert _bits(c.mesh_distance(*large, device=True)) == fresh["large"]


def test_python_layer(ctx):
    from surfacenet_amd import mesh
    v, q, pts, max_dist = ref.CASES["shell"]()
    want = ref.reference("shell")
    got = mesh.point_to_mesh(pts, v, q.astype(np.int64), max_dist=max_dist)
    assert got["dist2"].tobytes() == want["d2"].tobytes() and np.array_equal(got["face"], want["face"]) and got["closest"].tobytes() == want["closest"].tobytes()
    assert np.array_equal(got["dist"], np.minimum(np.sqrt(want["d2"]), max_dist)) and [got[k] for k in mesh.DISTANCE_COUNTS] == want["counts"][:4].tolist()
    # mesh_deviation against the restatement's statistics of the restatement's samples
    vs, fs = sref.sphere_mesh()
    vs, fs = vs[: int(fs[:400].max()) + 1], fs[:400]
    t, dst = 0.25, 0.2
    dev = mesh.mesh_deviation(vs, fs, vs + [t, 0.0, 0.0], fs, dst)
    a, b = sref.sample(vs, fs, dst)[0], sref.sample(vs + [t, 0.0, 0.0], fs, dst)[0]
    for key, p, vv in (("a_to_b", a, vs + [t, 0.0, 0.0]), ("b_to_a", b, vs)):
        d = np.minimum(np.sqrt(ref.distance(vv, fs, p, 60.0)["d2"]), 60.0)
        assert dev[key] == dict(n=p.shape[0], n_beyond=0, max=float(d.max()), mean=float(d.mean()), rms=float(np.sqrt((d * d).mean())))
        assert 0.0 < dev[key]["max"] <= t
    assert dev["hausdorff"] == max(dev["a_to_b"]["max"], dev["b_to_a"]["max"])


MASK = np.ones((30, 30, 30), np.uint8)
BB, RES, PLANE = np.asarray([[-30.0, -30, -30], [28, 28, 28]]), 2, np.asarray([0.0, 0.0, 1.0, 20.0])


def test_completeness_surface_lies_in_the_bracket_of_the_samples(ctx):
    from surfacenet_amd import evaluation
    v, f = sref.sphere_mesh()
    g = ref.lattice_queries((-15.0, -15.0, -15.0), (-9.0, -9.0, -9.0), 9)
    sample_dst = 0.2
    kw = dict(dst=1e-3, sample_dst=sample_dst, max_dist=2.5)   # (a reduction at 1e-3 mm keeps every sample: the bracket is about the samples)
    samples = evaluation.mesh_compare(v, f, g, MASK, BB, RES, PLANE, **kw)
    surface = evaluation.mesh_compare(v, f, g, MASK, BB, RES, PLANE, completeness="surface", **kw)
    assert "completeness" not in samples and surface["completeness"] == "surface"
    for k in samples:
        if k != "Dstl":
            assert np.array_equal(surface[k], samples[k]), k
    assert (samples["Dstl"] - 2.0 / 3.0 * sample_dst <= surface["Dstl"]).all() and (surface["Dstl"] <= samples["Dstl"] * (1.0 + 1e-12)).all()
    assert np.array_equal(surface["Dstl"], np.minimum(np.sqrt(ref.distance(v, f, g, 2.5)["d2"]), 2.5)) and (surface["Dstl"] == 2.5).any()


def _scene():
    import normals_ref as nref
    s = nref.surface_scene((2, 2, 1))
    d = s["lists"]
    out = dict(prediction_list=d["prediction_list"], vxl_ijk_list=d["vxl_ijk_list"], rayPooling_votes_list=d["rayPooling_votes_list"],
               cube_ijk_np=d["cube_ijk_np"], param_np=s["param"], viewPair_np=s["viewPair"], rgb_list=d["rgb_list"])
    return s, d, out


def test_in_a_scene_the_deviation_is_the_stages_called_by_hand(gpu_required, tmp_path):
    import meshchain_util as mc
    from surfacenet_amd import mesh, reconstruct
    s, d, out = _scene()
    kw = dict(tau=0.7, gamma=0.5, N_refine_iter=2, cameraTs_np=s["cameraTs"], mesh=True, mesh_smooth=3)
    dirs = {}
    for tag in ("deviation", "plain"):
        dirs[tag] = tmp_path / tag
        dirs[tag].mkdir()
    got = reconstruct.scene_postpass(out, 32, 26, 2, mesh_deviation=True, mesh_ply_prefix=str(dirs["deviation"] / "s_"), **kw)
    plain = reconstruct.scene_postpass(out, 32, 26, 2, mesh_ply_prefix=str(dirs["plain"] / "s_"), **kw)
    assert set(got) - set(plain) == {"fixThresh_mesh_deviation", "adapt_mesh_deviation"}
    files = sorted(os.listdir(str(dirs["plain"])))
    assert sorted(os.listdir(str(dirs["deviation"]))) == files    # it writes no file, and every other file holds the same bytes
    for fname in files:
        assert open(str(dirs["plain"] / fname), "rb").read() == open(str(dirs["deviation"] / fname), "rb").read()
    for key in plain:
        if key.endswith("_mesh") or "_mesh_" in key:
            mc.same_dict(got[key], plain[key])
    _, resol = mesh.lattice_origin(out["cube_ijk_np"], out["param_np"], 13)
    for name in ("fixThresh", "adapt"):
        m, last = got[name + "_mesh"], got[name + "_mesh_smoothed"]
        by_hand = mesh.mesh_deviation(last["vertices"], last["quads"], m["vertices"], m["quads"], resol)
        assert got[name + "_mesh_deviation"] == by_hand
        assert by_hand["a_to_b"]["n"] > 1000 and by_hand["a_to_b"]["n_beyond"] == 0 and 0.0 < by_hand["hausdorff"] < 3.0 * resol      # smoothing moves the surface by less than a few cells
    wide = reconstruct.scene_postpass(out, 32, 26, 2, mesh_deviation=dict(dst=2.0 * resol, max_dist=1e-3), **kw)
    assert wide["adapt_mesh_deviation"]["a_to_b"]["n"] < got["adapt_mesh_deviation"]["a_to_b"]["n"] and wide["adapt_mesh_deviation"]["hausdorff"] == 1e-3
