"""CPU: the restatement of the mesh self-intersection stage (tests/meshintersect_ref.py) on what each named case was
built to show - a positive case whose rule did not fire fails here, not on the GPU -, on the consequences of its rules (rule 8) and on an
error planted in each rule; the argument checks of mesh.self_intersections and the fifth row of the chain, which run before the library is
touched; the new symbols in header, version script and binding; and csrc/meshintersect_rules.h with mxi_check_args of csrc/sn_host.h
compiled alone under the sanitizers and run as a child process."""
import os
import subprocess

import numpy as np
import pytest

import mesh_refusals as bad
import meshchain_util as mc
import meshintersect_ref as ref
from test_host_plumbing import CSRC, ROOT, _compile


def _no_library(monkeypatch):
    from surfacenet_amd import runtime

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(runtime, "any_context", no_library)


def _counts(r):
    return dict(zip(ref.COUNTS, r["counts"].tolist()))


def _pair_set(r):
    return {tuple(p) for p in r["all_pairs"].tolist()}


# ---- what every case was built to show ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.CLEAN)
def test_clean_meshes_have_no_pair(name):
    r = ref.reference(name)
    c = _counts(r)
    assert c["n_pairs"] == 0 and c["n_faces_hit"] == 0 and not r["face_hit"].any() and r["pairs"].shape == (0, 2) and r["pairs"].dtype == np.int32
    assert c["n_candidates"] > 100 and c["n_degenerate_faces"] == 0        # neighbours were looked at and found to share no more than their indices


def test_rules_case_is_the_duplicate_and_the_degenerate_face():
    v, f = ref.CASES["rules"]()
    r = ref.reference("rules")
    assert np.isnan(v[7, 0]) and 7 not in f                     # the unreferenced vertex is not looked at
    assert r["all_pairs"].tolist() == [[0, 1]] and r["k_hits"] == [0, 0, 0, 1]
    assert _counts(r) == dict(n_triangles=5, n_degenerate_faces=1, n_candidates=r["counts"][2], n_pairs=1, n_faces_hit=2, n_disjoint_pairs=0,
                              n_adjacent_pairs=1, n_written=1)
    assert r["face_hit"].tolist() == [1, 1, 0, 0, 0, 0] and r["face_pairs"].tolist() == [1, 1, 0, 0, 0, 0]


def test_positive_cases_fire_the_rule_they_were_built_for():
    two = ref.reference("two_spheres_crossing")
    assert two["k_hits"][0] > 500 and two["k_hits"][1:] == [0, 0, 0] and two["counts"][3] > 500
    first, second = two["all_pairs"][:, 0], two["all_pairs"][:, 1]
    assert (first < 1452).all() and (second >= 1452).all()      # every pair joins the two spheres
    assert len(set((first // 256).tolist())) > 2                # ... from several workgroups of faces
    co = ref.reference("coincident")
    assert co["face_hit"].all() and co["k_hits"][1:] == [0, 0, 0] and {(i, i + 1452) for i in range(1452)} <= _pair_set(co)
    assert co["counts"][3] > 10 * 1452                          # ... and its twin's neighbours
    fold = ref.reference("fold")
    assert fold["k_hits"][1] > 0 and fold["k_hits"][2] > 0 and fold["k_hits"][3] == 0 and fold["bits"] == 0      # coplanar throughout: every 3x3 determinant is 0
    assert fold["counts"][6] > 0
    assert ref.same_bytes(ref.reference("fold_x"), fold) == []  # the same sheet in the plane x = 3
    wall, touch = ref.reference("wall"), ref.reference("wall_touch")
    assert wall["k_hits"] == [wall["k_hits"][0], 0, 0, 0] and wall["k_hits"][0] > 0 and wall["bits"] > 0
    assert all(a < 32 <= b for a, b in wall["all_pairs"].tolist())         # lower sheet against upper sheet only
    assert 0 < touch["counts"][3] < wall["counts"][3] and all(a < 32 <= b for a, b in touch["all_pairs"].tolist())
    v, f = ref.CASES["wall_touch"]()
    lows = {a for a, _ in touch["all_pairs"].tolist()}
    assert len(lows) == 1 and v[25 + 12, 2] == 3.0              # the vertex lies in one triangle of the lower sheet, exactly on it
    tj = ref.reference("tjunction")
    assert tj["all_pairs"].tolist() == [[0, 1], [0, 2]] and tj["k_hits"] == [0, 2, 0, 0] and tj["counts"][5:7].tolist() == [0, 2]
    sad = ref.reference("quad_saddle")
    assert sad["all_pairs"].tolist() == [[0, 1]] and [(a, b) for a, b, _ in sad["tri_hits"]] == [(1, 2)]      # through the quad's second triangle only
    assert sad["counts"][:2].tolist() == [3, 1]                 # the thin quad's second triangle is degenerate; its first is not skipped
    far = ref.reference("far")
    assert far["bits"] > 100 and far["counts"][3] == ref.reference("wall")["counts"][3] + 3
    assert far["all_pairs"][:12].tolist() == ref.reference("wall")["all_pairs"].tolist()       # the translated wall: the same pairs
    big = ref.reference("big_and_small")
    assert big["counts"][0] == 4001 and 50 < big["counts"][3] < 200 and (big["all_pairs"][:, 1] == 4000).all()


# ---- rule 8 ------------------------------------------------------------------------------------------------------------------------------------------
def test_a_permutation_of_the_faces_permutes_the_arrays_and_relabels_the_pairs():
    v, f, perm = ref.scramble()
    base, scr = ref.reference("two_spheres_crossing"), ref.reference("scr")
    assert np.array_equal(scr["face_hit"], base["face_hit"][perm]) and np.array_equal(scr["face_pairs"], base["face_pairs"][perm])
    back = {tuple(sorted((int(perm[a]), int(perm[b])))) for a, b in scr["all_pairs"].tolist()}
    assert back == _pair_set(base) and scr["counts"][[0, 1, 3, 4, 5, 6]].tolist() == base["counts"][[0, 1, 3, 4, 5, 6]].tolist()


@pytest.mark.parametrize("name", ["fold", "wall_touch", "tjunction", "quad_saddle", "wall"])
def test_translation_and_reversal_change_nothing(name):
    v, f = ref.CASES[name]()
    want = ref.reference(name)
    assert ref.same_bytes(ref.intersect(v + np.asarray([7.0, -3.0, 1000.0]), f), want) == []
    rev = f.copy()
    rev[::2] = rev[::2][:, ::-1] if f.shape[1] == 3 else rev[::2][:, [0, 3, 2, 1]]      # (a quad keeps its diagonal)
    assert ref.same_bytes(ref.intersect(v, rev), want) == []


def test_triangulated_quads_give_the_same_pairs():
    from surfacenet_amd import mesh
    v, q = ref.sm.sphere_case(6, True)
    cases = [ref.CASES["quad_saddle"](), (np.concatenate([v, v + [5.0, 0.0, 0.0]]), np.concatenate([q, q + v.shape[0]]).astype(np.int32))]
    for vv, quads in cases:
        as_quads, as_tris = ref.intersect(vv, quads), ref.intersect(vv, mesh.triangulate(quads))
        back = {tuple(sorted((a // 2, b // 2))) for a, b in as_tris["all_pairs"].tolist()}
        assert back == _pair_set(as_quads) and as_quads["counts"][3] > 0
    assert ref.intersect(*cases[1])["counts"][3] > 100


# ---- an error planted in each rule changes a named case ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plant,name", [("open", "wall_touch"), ("no_coplanar", "fold"), ("k1_as_k0", "wall"), ("int64", "far"), ("drop_z", "fold_x")])
def test_a_planted_error_is_seen(plant, name):
    assert plant in ref.PLANTS
    want = ref.reference(name)
    assert ref.same_bytes(ref.intersect(*ref.CASES[name]()), want) == []
    assert ref.same_bytes(ref.intersect(*ref.CASES[name](), plant=plant), want) != []


def test_a_short_list_is_the_head_of_the_long_one():
    v, f = ref.CASES["wall"]()
    want = ref.reference("wall")
    P = int(want["counts"][3])
    for cap in (0, P - 1, P, P + 5):
        r = ref.intersect(v, f, cap_pairs=cap)
        assert ref.same_bytes(r, ref.truncated(want, cap)) == [] and r["pairs"].shape == (min(P, cap), 2) and r["counts"][3] == P


# ---- mesh.self_intersections and the chain before the library ----------------------------------------------------------------------------------------
def test_check_intersect_args():
    from surfacenet_amd import mesh
    assert mesh.check_intersect_args() is None and mesh.check_intersect_args(0) == 0 and mesh.check_intersect_args(17) == 17
    for value, text in ((-1, "max_pairs = -1: an integer number of pairs >= 0, or None for all of them"),
                        (2.5, "max_pairs = 2.5: an integer number of pairs >= 0, or None for all of them"),
                        (True, "max_pairs = True: an integer number of pairs >= 0, or None for all of them"),
                        ("a", "max_pairs = 'a' must be an integer or None")):
        with pytest.raises(ValueError) as e:
            mesh.check_intersect_args(value)
        assert str(e.value) == text


def test_self_intersections_refuses_a_bad_mesh_in_the_stages_words(monkeypatch):
    from surfacenet_amd import mesh
    _no_library(monkeypatch)
    v, f = bad.sheet()
    cases = [bad.bad_index(v, f, 2, 5)] + [bad.bad_coordinate(v, f, 3, value) for value in (np.nan, 2097144.0)]
    cases += [(v.astype(np.int32), f, "vert_lattice must be float32 or float64, not int32"), (v, np.zeros((18, 5), np.int32), "faces must be (F,3) or (F,4), not (18, 5)"),
              (np.zeros((0, 3)), f, "face 0 names a vertex outside [0, 0)")]
    for bv, bf, text in cases:
        for run in (mesh.self_intersections, mesh.smooth_mesh):
            with pytest.raises(ValueError) as e:
                run(bv, bf)
            assert str(e.value) == text
    for bv, bf, text in cases[:3]:
        with pytest.raises(ValueError) as e:
            ref.intersect(bv, bf)
        assert str(e.value) == text
    with pytest.raises(ValueError, match="max_pairs = -2"):
        mesh.self_intersections(v, f, max_pairs=-2)
    for vv, ff in ((v, np.zeros((0, 4), np.int32)), (np.zeros((0, 3)), np.zeros((0, 3), np.int32))):      # no face: without the library
        e = mesh.self_intersections(vv, ff, max_pairs=3)
        assert e["pairs"].shape == (0, 2) and e["pairs"].dtype == np.int32 and e["face_hit"].shape == (0,) and e["face_hit"].dtype == bool
        assert e["face_pairs"].dtype == np.int32 and [e[k] for k in mesh.INTERSECT_COUNTS] == [0] * 6 and e["truncated"] is False
        assert ref.same_bytes(dict(e, face_hit=e["face_hit"].astype(np.uint8), counts=np.zeros((8,), np.int64)), ref.intersect(vv, ff)) == []
    assert mesh.INTERSECT_COUNTS == tuple(ref.COUNTS[i] for i in (0, 1, 3, 4, 5, 6))


def test_the_chains_fifth_row(monkeypatch):
    from surfacenet_amd import mesh, reconstruct
    _no_library(monkeypatch)
    assert mesh.chain_settings(mesh_check=True) == [("checked", dict(max_pairs=None))] == mesh.chain_settings(mesh_check=dict())
    assert mesh.chain_settings(mesh_check=dict(max_pairs=5)) == [("checked", dict(max_pairs=5))]
    assert mesh.chain_settings(mesh_check=None) == [] == mesh.chain_settings(mesh_check=False)
    stages = mesh.chain_settings(mc.FILL, mc.SMOOTH, mc.CELL, "mean", "outward", True)
    assert [k for k, _ in stages] == ["filled", "smoothed", "simplified", "oriented", "checked"]
    assert stages[:4] == mesh.chain_settings(mc.FILL, mc.SMOOTH, mc.CELL, "mean", "outward")
    assert [mesh.stage_tag(k, kw) for k, kw in stages] == ["_f16", "_s2", "_c2", "_o", None]      # the check writes no file
    for value, text in ((5, "mesh_check = 5: True or a dict of max_pairs"), ("yes", "mesh_check = 'yes': True or a dict of max_pairs"),
                        (dict(cell=2), "mesh_check = {'cell': 2}: True or a dict of max_pairs"),
                        (dict(max_pairs=-1), "max_pairs = -1: an integer number of pairs >= 0, or None for all of them")):
        with pytest.raises(ValueError) as e:
            mesh.chain_settings(2, -1, 1, "mean", "up", value)  # the new argument is the first one judged
        assert str(e.value) == text
    with pytest.raises(ValueError, match="sign = 'up'"):        # then the table's order as before
        mesh.chain_settings(2, -1, 1, "mean", "up", True)
    empty = dict(prediction_list=[], vxl_ijk_list=[], rayPooling_votes_list=[], cube_ijk_np=np.zeros((0, 3), np.int64))
    cams = np.zeros((2, 3))
    with pytest.raises(ValueError) as e:
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh_check=True)
    assert str(e.value) == "mesh_check needs mesh=True: it checks the mesh that mesh=True extracts"
    with pytest.raises(ValueError, match="mesh_orient needs mesh=True"):      # the order: ..., orient, render, check
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh_orient="outward", mesh_check=True)
    with pytest.raises(ValueError, match="mesh_check = 3"):
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_check=3)


@pytest.mark.parametrize("combo", mc.COMBOS)
def test_run_chain_on_the_empty_mesh_with_the_check(combo, monkeypatch):
    from surfacenet_amd import mesh, reconstruct
    _no_library(monkeypatch)
    old = mesh.run_chain(mesh.empty_mesh(), mesh.chain_settings(*combo, "mean", "outward"), (0.0, 0.0, 0.0), 1.0)
    got = mesh.run_chain(mesh.empty_mesh(), mesh.chain_settings(*combo, "mean", "outward", True), (0.0, 0.0, 0.0), 1.0)
    assert list(got) == mc.asked(combo) + ["oriented", "checked"]
    for key in old:                                             # the four old stages: unchanged
        if key == "oriented":                                   # (its components are a dict of their own)
            assert set(got[key]) == set(old[key]) and all(np.array_equal(got[key][k], old[key][k]) for k in old[key] if k != "components")
        else:
            mc.same_dict(got[key], old[key])
    e = got["checked"]
    assert set(e) == {"pairs", "face_hit", "face_pairs", "truncated"} | set(mesh.INTERSECT_COUNTS)
    assert e["pairs"].shape == (0, 2) and e["n_pairs"] == 0 and e["truncated"] is False
    empty = dict(prediction_list=[], vxl_ijk_list=[], rayPooling_votes_list=[], cube_ijk_np=np.zeros((0, 3), np.int64))
    fill, smooth, cell = combo
    kw = dict(cameraTs_np=np.zeros((2, 3)), mesh=True, mesh_fill=fill, mesh_smooth=smooth, mesh_cell=cell)
    plain = reconstruct.scene_postpass(empty, 32, 26, 2, **kw)
    for off in (None, False):                                   # the default: no key, the same dicts
        none = reconstruct.scene_postpass(empty, 32, 26, 2, mesh_check=off, **kw)
        assert set(none) == set(plain)
    for normals in ("source", "mesh"):
        post = reconstruct.scene_postpass(empty, 32, 26, 2, mesh_check=True, mesh_normals=normals, mesh_ply_prefix="/nonexistent/x_", **kw)
        assert set(post) - set(plain) == {"fixThresh_mesh_checked", "adapt_mesh_checked"}
        assert set(post["adapt_mesh_checked"]) == set(e)        # a report: no vert_normals are added to it
        if normals == "source":
            for key in plain:
                if key.endswith("_mesh") or "_mesh_" in key:
                    mc.same_dict(post[key], plain[key])


# ---- the ABI: symbols are only added -----------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_version_script_and_binding():
    import fnmatch
    import re
    from surfacenet_amd import _lib
    new = ("sn_mesh_intersect", "sn_mesh_intersect_dev")
    txt = open(os.path.join(ROOT, "include", "surfacenet_hip.h")).read()
    assert "#define SN_ABI_VERSION 2" in txt and "sn_mesh_intersect_cfg" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    pattern = re.search(r"global:\s*([^;]+);", open(os.path.join(CSRC, "exports.map")).read()).group(1).strip()
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert fnmatch.fnmatchcase(name, pattern), (name, pattern)
        assert name in _lib.ABI_SYMBOLS, name
    assert "sn_meshintersect.hip" in open(os.path.join(CSRC, "Makefile")).read()
    assert ctypes_size(_lib.MeshIntersectCfg) == 8


def ctypes_size(struct):
    import ctypes
    return ctypes.sizeof(struct)


def test_the_rules_header_is_hip_free():
    with open(os.path.join(CSRC, "meshintersect_rules.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes and all("hip/" not in i and i in ("<stdint.h>", '"meshnormals_sum.h"') for i in includes), includes


# ---- the rules and the argument checks of the C entry, on the CPU ------------------------------------------------------------------------------------
def test_rules_and_argument_checks_under_sanitizers(tmp_path):
    """tests/host/meshintersect_check.cpp runs csrc/meshintersect_rules.h - the signs at the ends of the coordinate range, every sign
    combination of rule 3, each k of rule 4, the pair key, the grid's arithmetic - and sn_host.h's mxi_check_args over every end of every
    range, compiled stand-alone with -fsanitize=address,undefined and run as a child process."""
    exe = str(tmp_path / "meshintersect_check")
    _compile(os.path.join(ROOT, "tests", "host", "meshintersect_check.cpp"), exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "MESHINTERSECT-CHECK-OK" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
