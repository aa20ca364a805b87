"""GPU (-m gpu): the mesh self-intersection stage (surfacenet_amd/csrc/meshintersect.h) against the restatement
tests/meshintersect_ref.py, byte for byte - face_hit, face_pairs, the pair list and the counts but counts[2], the broad phase's own number -,
in the host form and the device form: the named cases, the scrambled case mapped back, short pair lists, the grid level forced in the
test-only twin, repeated calls on one context, the empty meshes, the refusals in the other stages' words, mesh.self_intersections' Python
layer, and the check at the end of reconstruct.scene_postpass's chain. Every launch is a plain bounded kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_refusals as bad
import meshintersect_ref as ref

pytestmark = pytest.mark.gpu
CASES = tuple(ref.CASES)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx(gpu_required):
    from surfacenet_amd import runtime
    return runtime.any_context()


def _bytes(r):
    out = {k: np.asarray(r[k]).tobytes() for k in ref.KEYS[:3]}
    out["counts"] = np.delete(np.asarray(r["counts"]), 2).tobytes()
    return out


def _check(ctx, v, f, want, **kw):
    for device in (False, True):
        got = ctx.mesh_intersect(v, f, device=device, **kw)
        assert [got[k].dtype for k in ref.KEYS] == [np.uint8, np.int32, np.int32, np.int64]
        assert ref.same_bytes(got, want) == [], (device, kw, ref.same_bytes(got, want), got["counts"].tolist(), want["counts"].tolist())
    return got


@pytest.mark.parametrize("name", CASES)
def test_bit_for_bit_against_the_restatement(ctx, name):
    v, f = ref.CASES[name]()
    want = ref.reference(name)
    got = _check(ctx, v, f, want)
    assert got["counts"][2] >= want["counts"][3]                # every hit was a candidate somewhere
    if name == "two_spheres_crossing":
        assert f.shape[0] == 2904 and want["counts"][3] > 500   # several workgroups, hundreds of pairs
    if name == "coincident":
        assert want["counts"][3] > f.shape[0]                   # more pairs than faces: the list of the first call is short, the second is exact


def test_the_scrambled_case_maps_back(ctx):
    v, f, perm = ref.scramble()
    got = _check(ctx, v, f, ref.reference("scr"))
    base = ref.reference("two_spheres_crossing")
    assert np.array_equal(got["face_hit"], base["face_hit"][perm]) and np.array_equal(got["face_pairs"], base["face_pairs"][perm])
    back = {tuple(sorted((int(perm[a]), int(perm[b])))) for a, b in got["pairs"].tolist()}
    assert back == {tuple(p) for p in base["all_pairs"].tolist()}


def test_a_short_pair_list_is_truncated_not_refused(ctx):
    v, f = ref.CASES["two_spheres_crossing"]()
    want = ref.reference("two_spheres_crossing")
    P = int(want["counts"][3])
    for cap in (0, P - 1, P):
        got = _check(ctx, v, f, ref.truncated(want, cap), cap_pairs=cap)
        assert got["pairs"].shape == (min(P, cap), 2) and got["counts"][3] == P and got["counts"][7] == min(P, cap)


@pytest.mark.parametrize("name", ["two_spheres_crossing", "big_and_small"])
def test_the_result_does_not_depend_on_the_grid_level(gpu_required, tmp_path, name):
    """SN_MXI_LEVEL forces the level in the test-only twin (read once per call; one child process per level): the finest, three above the
    one the stage picks, and the coarsest - one cell for everything, walked by whole workgroups."""
    want = ref.reference(name)
    chosen, _ = ref.grid_level(*ref.CASES[name]())
    assert chosen == (0 if name == "two_spheres_crossing" else 1)      # big_and_small: above the small triangles' natural level
    candidates = []
    for level in (None, 0, chosen + 3, 21):
        env = dict(os.environ, SURFACENET_HIP_LIB=os.path.join(ROOT, "surfacenet_amd", "libsurfacenet_hip_dbg.so"))      # the switch exists in the twin alone
        env.pop("SN_MXI_LEVEL", None)
        if level is not None:
            env["SN_MXI_LEVEL"] = str(level)
        out = str(tmp_path / ("level_%s.npz" % level))
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "bench_meshintersect.py"), "--case", name, "--save", out], env=env, cwd=ROOT)
        got = np.load(out)
        assert ref.same_bytes(got, want) == [], (level, ref.same_bytes(got, want), got["counts"].tolist())
        candidates.append(int(got["counts"][2]))
    assert len(set(candidates)) == 1, candidates                # (a candidate is a pair of overlapping boxes, met in one cell: the same number at any level)


def test_run_twice_then_grow_the_workspace_and_come_back(ctx):
    small, large = ref.CASES["wall"](), ref.CASES["coincident"]()
    first = _bytes(ctx.mesh_intersect(*small))
    assert _bytes(ctx.mesh_intersect(*small)) == first
    assert ref.same_bytes(ctx.mesh_intersect(*large), ref.reference("coincident")) == []
    assert _bytes(ctx.mesh_intersect(*small)) == first and _bytes(ctx.mesh_intersect(*small, device=True)) == first
    assert ref.same_bytes(ctx.mesh_intersect(*small), ref.reference("wall")) == []


def test_empty_meshes(ctx):
    v = np.asarray([(0, 0, 0), (2, 0, 0), (0, 2, 0), (np.nan, 1, 1)], np.float64)
    for device in (False, True):
        for vv, ff in ((v, np.zeros((0, 3), np.int32)), (np.zeros((0, 3)), np.zeros((0, 4), np.int32))):
            e = ctx.mesh_intersect(vv, ff, device=device)       # F = 0: the NaN vertex is not looked at
            assert e["face_hit"].shape == (0,) and e["pairs"].shape == (0, 2) and not e["counts"].any()
            assert ref.same_bytes(e, ref.intersect(vv, ff)) == []
    f = np.asarray([[0, 1, 2]], np.int32)
    got = _check(ctx, v, f, ref.intersect(v, f))
    assert got["counts"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    f = np.asarray([[0, 1, 1], [0, 1, 2]], np.int32)            # one degenerate face and nothing else to meet
    assert _check(ctx, v, f, ref.intersect(v, f))["counts"][:2].tolist() == [1, 1]


@pytest.mark.parametrize("rows,at,later,coord_at", [(4, 2, 5, 3), (51, 257, 280, 257)])
def test_refusals_in_the_smoothers_words(ctx, rows, at, later, coord_at):
    from surfacenet_amd import _lib, SurfaceNetHipError
    v, f = bad.sheet(rows)
    before = {device: _bytes(ctx.mesh_intersect(v, f, device=device)) for device in (False, True)}
    assert before[False] == before[True] == _bytes(ref.intersect(v, f))
    cases = [bad.bad_index(v, f, at, later)]
    for value in (np.nan, 2097144.0):
        cases.append(bad.bad_coordinate(v, f, coord_at, value))
    far, _, text = bad.bad_coordinate(v, f, coord_at, np.nan)       # ... and a bad index at a later face: the smaller face is the one named
    cases.append((far, bad.bad_index(v, f, later, later)[1], text))
    for bv, bf, text in cases:
        said = set()
        for device in (False, True):
            for run in (lambda: ctx.mesh_intersect(bv, bf, device=device), lambda: ctx.mesh_smooth(bv, bf, 2, device=device)):
                with pytest.raises(SurfaceNetHipError) as e:
                    run()
                said.add(str(e.value))
        assert len(said) == 1 and text in said.pop(), (text, said)
    with pytest.raises(SurfaceNetHipError, match="cap_pairs"):
        ctx.mesh_intersect(v, f, cap_pairs=-1)
    # the host form, called directly: a refusal writes nothing but zero counts - bad mesh, bad cap, null cfg
    lib = _lib.load()
    bv, bf, _ = cases[0]
    bv, bf = np.ascontiguousarray(bv, np.float64), np.ascontiguousarray(bf, np.int32)
    for cfg, vv, ff in ((_lib.MeshIntersectCfg(100), bv, bf), (_lib.MeshIntersectCfg(-1), np.ascontiguousarray(v), f), (None, np.ascontiguousarray(v), f)):
        hit, pairs_per, pairs = np.full((f.shape[0],), 7, np.uint8), np.full((f.shape[0],), 7, np.int32), np.full((100, 2), 7, np.int32)
        counts = (_lib.ctypes.c_longlong * 8)(*([9] * 8))
        rc = lib.sn_mesh_intersect(ctx._h, None if cfg is None else _lib.ctypes.byref(cfg), vv.shape[0], _lib.ptr(vv), ff.shape[0], 3, _lib.ptr(ff),
                                   _lib.ptr(hit), _lib.ptr(pairs_per), _lib.ptr(pairs), counts)
        assert rc == -1 and list(counts) == [0] * 8 and (hit == 7).all() and (pairs_per == 7).all() and (pairs == 7).all()
    assert {device: _bytes(ctx.mesh_intersect(v, f, device=device)) for device in (False, True)} == before      # the context is usable


def test_python_layer(ctx):
    from surfacenet_amd import mesh
    v, f = ref.CASES["two_spheres_crossing"]()
    want = ref.reference("two_spheres_crossing")
    got = mesh.self_intersections(v, f)
    assert [got[k] for k in mesh.INTERSECT_COUNTS] == want["counts"][[0, 1, 3, 4, 5, 6]].tolist() and got["truncated"] is False
    assert np.array_equal(got["pairs"], want["all_pairs"]) and got["face_hit"].dtype == bool and np.array_equal(got["face_pairs"], want["face_pairs"])
    few = mesh.self_intersections(v, f.astype(np.int64), max_pairs=10)
    assert np.array_equal(few["pairs"], want["all_pairs"][:10]) and few["truncated"] is True and few["n_pairs"] == got["n_pairs"]
    co = mesh.self_intersections(*ref.CASES["coincident"]())     # more pairs than faces: the second call, at the count
    assert np.array_equal(co["pairs"], ref.reference("coincident")["all_pairs"]) and co["truncated"] is False and co["n_pairs"] > f.shape[0]
    q = mesh.self_intersections(*ref.CASES["quad_saddle"]())
    assert q["pairs"].tolist() == [[0, 1]] and q["n_degenerate_faces"] == 1 and q["n_triangles"] == 3
    clean = mesh.self_intersections(*ref.CASES["sphere6_q"]())
    assert clean["n_pairs"] == 0 and not clean["face_hit"].any() and clean["pairs"].shape == (0, 2)


def _scene():
    import normals_ref as nref
    s = nref.surface_scene((2, 2, 1))
    d = s["lists"]
    out = dict(prediction_list=d["prediction_list"], vxl_ijk_list=d["vxl_ijk_list"], rayPooling_votes_list=d["rayPooling_votes_list"],
               cube_ijk_np=d["cube_ijk_np"], param_np=s["param"], viewPair_np=s["viewPair"], rgb_list=d["rgb_list"])
    return s, d, out


@pytest.mark.parametrize("chain", [dict(), dict(mesh_fill=16, mesh_smooth=3, mesh_cell=2, mesh_orient="outward")])
def test_in_a_scene_the_check_is_the_stage_on_the_chains_last_mesh(gpu_required, tmp_path, chain):
    import meshchain_util as mc
    from surfacenet_amd import mesh, reconstruct
    s, d, out = _scene()
    kw = dict(tau=0.7, gamma=0.5, N_refine_iter=2, cameraTs_np=s["cameraTs"], mesh=True, **chain)
    dirs = {}
    for tag in ("checked", "plain"):
        dirs[tag] = tmp_path / tag
        dirs[tag].mkdir()
    got = reconstruct.scene_postpass(out, 32, 26, 2, mesh_check=True, mesh_ply_prefix=str(dirs["checked"] / "s_"), **kw)
    plain = reconstruct.scene_postpass(out, 32, 26, 2, mesh_ply_prefix=str(dirs["plain"] / "s_"), **kw)
    assert set(got) - set(plain) == {"fixThresh_mesh_checked", "adapt_mesh_checked"}
    files = sorted(os.listdir(str(dirs["plain"])))
    assert sorted(os.listdir(str(dirs["checked"]))) == files    # the check writes no file, and every other file holds the same bytes
    for fname in files:
        assert open(str(dirs["plain"] / fname), "rb").read() == open(str(dirs["checked"] / fname), "rb").read()
    for key in plain:
        if (key.endswith("_mesh") or "_mesh_" in key) and not key.endswith("_oriented"):
            mc.same_dict(got[key], plain[key])
    for name in ("fixThresh", "adapt"):
        last = got[name + ("_mesh_oriented" if chain else "_mesh")]
        faces = last["faces"] if "faces" in last else last["quads"]
        by_hand = mesh.self_intersections(last["vert_lattice"], faces)
        report = got[name + "_mesh_checked"]
        assert set(report) == set(by_hand) and report["n_triangles"] > 1000
        for k in by_hand:
            assert np.array_equal(report[k], by_hand[k]), k
        want = ref.intersect(last["vert_lattice"], faces)       # and the restatement on the scene's own mesh
        assert np.array_equal(report["pairs"], want["all_pairs"]) and report["n_pairs"] == want["counts"][3]
    few = reconstruct.scene_postpass(out, 32, 26, 2, mesh_check=dict(max_pairs=0), **kw)
    assert few["adapt_mesh_checked"]["pairs"].shape == (0, 2) and few["adapt_mesh_checked"]["n_pairs"] == got["adapt_mesh_checked"]["n_pairs"]
