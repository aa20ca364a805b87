"""GPU (-m gpu): the mesh orientation stage (surfacenet_amd/csrc/meshorient.h) against the restatement
tests/meshorient_ref.py, byte for byte - the oriented faces, the four per-face arrays, the three per-piece arrays and the counts -, in the
host form and the device form and for both signs: the named cases, the thousand tetrahedra with the filter, a permutation of the faces,
repeated calls on one context, the empty meshes, the refusals in the other stages' words, mesh.orient_mesh's Python layer, and the fourth
stage of reconstruct.scene_postpass's chain. Every launch is a plain bounded kernel."""
import os

import numpy as np
import pytest

import mesh_refusals as bad
import meshorient_ref as ref

pytestmark = pytest.mark.gpu
CASES = tuple(ref.CASES)


@pytest.fixture(scope="module")
def ctx(gpu_required):
    from surfacenet_amd import runtime
    return runtime.any_context()


def _bytes(r):
    return {k: np.asarray(r[k]).tobytes() for k in ref.KEYS}


def _check(ctx, v, f, want, *cfg):
    for device in (False, True):
        got = ctx.mesh_orient(v, f, *cfg, device=device)
        assert [got[k].dtype for k in ref.KEYS] == [np.int32, np.uint8, np.int32, np.uint8, np.int32, np.uint8, np.uint64, np.int64]
        assert ref.same_bytes(got, want) == [], (device, cfg, ref.same_bytes(got, want), got["counts"].tolist(), want["counts"].tolist())
    return got


@pytest.mark.parametrize("name", CASES)
def test_bit_for_bit_against_the_restatement(ctx, name):
    v, f = ref.CASES[name]()
    for sign in (ref.MAJORITY, ref.OUTWARD):
        _check(ctx, v, f, ref.reference(name, sign), sign)
    if name == "surface_scr":
        assert f.shape[0] == 4600                               # several workgroups, one piece
    if name == "soup":
        assert ref.reference(name)["counts"][5] == 19834        # the lanes of one wave belong to different pieces


def test_thousand_tetrahedra_with_the_filter(ctx):
    v, f = ref.CASES["tets1000"]()
    for cfg in ((ref.MAJORITY, 5, 1), (ref.OUTWARD, 5, 1), (ref.MAJORITY, 5, 0), (ref.OUTWARD, 4, 0)):
        got = _check(ctx, v, f, ref.reference("tets1000", *cfg), *cfg)
    assert got["counts"][10:].tolist() == [4000, 1000]
    v, f = ref.CASES["two_spheres"]()
    _check(ctx, v, f, ref.reference("two_spheres", ref.OUTWARD, 1453, 1), ref.OUTWARD, 1453, 1)      # both too small: the first is kept


def test_a_permutation_of_the_faces(ctx):
    v, f = ref.CASES["sphere6_t_scr"]()
    want = ref.reference("sphere6_t_scr", ref.MAJORITY, 5, 1)
    perm = np.random.default_rng(13).permutation(f.shape[0])
    got = _check(ctx, v, np.ascontiguousarray(f[perm]), ref.orient(v, f[perm], ref.MAJORITY, 5, 1), ref.MAJORITY, 5, 1)
    assert np.array_equal(got["face_flip"], want["face_flip"][perm]) and np.array_equal(got["face_keep"], want["face_keep"][perm])
    assert np.array_equal(got["faces_out"], want["faces_out"][perm])


def test_run_twice_then_grow_the_workspace_and_come_back(ctx):
    small, large = ref.CASES["sphere6_q_scr"](), ref.CASES["soup"]()
    first = _bytes(ctx.mesh_orient(*small, ref.OUTWARD))
    assert _bytes(ctx.mesh_orient(*small, ref.OUTWARD)) == first
    assert ref.same_bytes(ctx.mesh_orient(*large), ref.reference("soup")) == []
    assert _bytes(ctx.mesh_orient(*small, ref.OUTWARD)) == first and _bytes(ctx.mesh_orient(*small, ref.OUTWARD, device=True)) == first
    assert ref.same_bytes(ctx.mesh_orient(*small, ref.OUTWARD), ref.reference("sphere6_q_scr", ref.OUTWARD)) == []


def test_empty_meshes(ctx):
    v = np.asarray([(0, 0, 0), (2, 0, 0), (0, 2, 0), (np.nan, 1, 1)], np.float64)
    for device in (False, True):
        for vv, ff in ((v, np.zeros((0, 3), np.int32)), (np.zeros((0, 3)), np.zeros((0, 4), np.int32))):
            e = ctx.mesh_orient(vv, ff, device=device)          # F = 0: the NaN vertex is not looked at
            assert e["faces_out"].shape == ff.shape and e["comp_vol6"].shape == (0, 3) and not e["counts"].any()
            assert ref.same_bytes(e, ref.orient(vv, ff)) == []
    f = np.asarray([[0, 1, 2]], np.int32)
    got = _check(ctx, v, f, ref.orient(v, f))
    assert got["counts"].tolist() == [3, 3, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1] and got["comp_flags"].tolist() == [ref.ORIENTABLE | ref.KEPT]


@pytest.mark.parametrize("rows,at,later,coord_at", [(4, 2, 5, 3), (51, 257, 280, 257)])
def test_refusals_in_the_smoothers_words(ctx, rows, at, later, coord_at):
    from surfacenet_amd import SurfaceNetHipError
    v, f = bad.sheet(rows)
    before = {device: _bytes(ctx.mesh_orient(v, f, device=device)) for device in (False, True)}
    assert before[False] == before[True] == _bytes(ref.orient(v, f))
    cases = [bad.bad_index(v, f, at, later)]
    for value in (np.nan, 2097144.0):
        cases.append(bad.bad_coordinate(v, f, coord_at, value))
    far, _, text = bad.bad_coordinate(v, f, coord_at, np.nan)       # ... and a bad index at a later face: the smaller face is the one named
    cases.append((far, bad.bad_index(v, f, later, later)[1], text))
    for bv, bf, text in cases:
        said = set()
        for device in (False, True):
            for run in (lambda: ctx.mesh_orient(bv, bf, ref.OUTWARD, device=device), lambda: ctx.mesh_smooth(bv, bf, 2, device=device)):
                with pytest.raises(SurfaceNetHipError) as e:
                    run()
                said.add(str(e.value))
        assert len(said) == 1 and text in said.pop(), (text, said)
    for cfg, word in (((2, 0, 0), "sign"), ((0, -1, 0), "min_faces"), ((0, 0, 2), "keep_largest")):
        with pytest.raises(SurfaceNetHipError, match=word):
            ctx.mesh_orient(v, f, *cfg)
    assert {device: _bytes(ctx.mesh_orient(v, f, device=device)) for device in (False, True)} == before


def test_python_layer(ctx):
    from surfacenet_amd import mesh
    v, f = ref.CASES["two_spheres"]()
    want = ref.reference("two_spheres", ref.OUTWARD, 0, 0)
    got = mesh.orient_mesh(v, f, sign="outward", resol=0.4)
    assert [got[k] for k in mesh.ORIENT_COUNTS] == want["counts"].tolist()
    c = got["components"]
    assert c["id"].tolist() == [0, 1452] and c["n_faces"].tolist() == [1452, 1452] and c["orientable"].all() and c["closed"].all()
    assert c["flipped"].tolist() == [False, True] and c["kept"].all()
    assert c["vol6"] == [want["vol6"][0], want["vol6"][1452]] and all(type(x) is int for x in c["vol6"])
    assert c["volume"].tolist() == [x / 6 / 2 ** 48 * 0.4 ** 3 for x in c["vol6"]] and abs(c["volume"][0] - 1015.167199 * 0.064) < 1e-6
    assert np.array_equal(got["faces"], want["faces_out"]) and got["face_src"].tolist() == list(range(2904)) and got["face_flip"].dtype == bool
    v, f = ref.CASES["tets1000"]()
    want = ref.reference("tets1000", ref.MAJORITY, 5, 1)
    got = mesh.orient_mesh(v, f, min_faces=5, keep_largest=True)
    keep = want["face_keep"].astype(bool)
    assert np.array_equal(got["faces"], want["faces_out"][keep]) and got["faces"].shape == (4, 3) and got["face_src"].tolist() == [0, 1, 2, 3]
    assert np.array_equal(got["face_keep"], keep) and np.array_equal(got["face_component"], want["face_component"])
    assert got["components"]["kept"].sum() == 1 and got["n_kept_faces"] == 4
    q = mesh.orient_mesh(*ref.CASES["sphere6_q_scr"](), sign="outward")
    assert q["faces"].shape == (726, 4) and np.array_equal(q["faces"], ref.sm.sphere_case(6, True)[1])      # the mesher's quads come back


def _scene():
    import normals_ref as nref
    s = nref.surface_scene((2, 2, 1))
    d = s["lists"]
    out = dict(prediction_list=d["prediction_list"], vxl_ijk_list=d["vxl_ijk_list"], rayPooling_votes_list=d["rayPooling_votes_list"],
               cube_ijk_np=d["cube_ijk_np"], param_np=s["param"], viewPair_np=s["viewPair"], rgb_list=d["rgb_list"])
    return s, d, out


def test_in_a_scene_the_chain_keeps_the_orientation(gpu_required, tmp_path):
    import meshchain_util as mc
    from surfacenet_amd import mesh, reconstruct
    s, d, out = _scene()
    kw = dict(tau=0.7, gamma=0.5, N_refine_iter=2, cameraTs_np=s["cameraTs"], mesh=True, mesh_fill=16, mesh_smooth=3, mesh_cell=2)
    dirs = {}
    for tag in ("oriented", "plain"):
        dirs[tag] = tmp_path / tag
        dirs[tag].mkdir()
    got = reconstruct.scene_postpass(out, 32, 26, 2, mesh_orient="outward", mesh_ply_prefix=str(dirs["oriented"] / "s_"), **kw)
    plain = reconstruct.scene_postpass(out, 32, 26, 2, mesh_ply_prefix=str(dirs["plain"] / "s_"), **kw)
    assert set(got) - set(plain) == {"fixThresh_mesh_oriented", "adapt_mesh_oriented"}
    old = sorted(os.listdir(str(dirs["plain"])))
    assert sorted(os.listdir(str(dirs["oriented"]))) == sorted(old + ["s_fixThresh_mesh_o.ply", "s_adapt_mesh_o.ply"])
    for fname in old:                                           # every other file: the bytes of the call without mesh_orient
        assert open(str(dirs["plain"] / fname), "rb").read() == open(str(dirs["oriented"] / fname), "rb").read()
    for key in plain:
        if key.endswith("_mesh") or "_mesh_" in key:
            mc.same_dict(got[key], plain[key])
    for name in ("fixThresh", "adapt"):
        o, before = got[name + "_mesh_oriented"], plain[name + "_mesh_simplified"]
        assert o["n_inconsistent"] == 0 and o["n_flipped_faces"] == 0      # the chain kept its orientation
        assert o["n_links"] > 1000 and o["n_components"] >= 1 and o["n_kept_faces"] == before["faces"].shape[0]
        assert np.array_equal(o["faces"], before["faces"]) and np.array_equal(o["vertices"], before["vertices"])
        assert np.array_equal(o["vert_src"], before["vert_src"]) and o["components"]["n_faces"].sum() == before["faces"].shape[0]
        mc.check_stage_ply(str(dirs["oriented"] / ("s_%s_mesh_o.ply" % name)), o, got[name + "_normal_list"], d["rgb_list"])
