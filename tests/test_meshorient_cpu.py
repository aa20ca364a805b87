"""CPU: the restatement of the mesh orientation stage (tests/meshorient_ref.py) pinned on hand values of its smallest
cases, checked against an independent breadth-first propagation in plain Python, on the consequences of its rules (rule 10) and on a fault
planted in each rule; the argument checks of mesh.orient_mesh and the fourth row of the chain, which run before the library is touched; the
new symbols in header, version script, binding and library; and csrc/meshorient_rules.h with mor_check_args of csrc/sn_host.h compiled alone
under the sanitizers and run as a child process."""
import collections
import os
import subprocess

import numpy as np
import pytest

import mesh_refusals as bad
import meshchain_util as mc
import meshnormals_ref as mn
import meshorient_ref as ref
from test_host_plumbing import CSRC, ROOT, _compile


def _no_library(monkeypatch):
    from surfacenet_amd import runtime

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(runtime, "any_context", no_library)


def _counts(r):
    return dict(zip(ref.COUNTS, r["counts"].tolist()))


# ---- hand values -----------------------------------------------------------------------------------------------------------------------------------
def test_tetrahedra():
    t = ref.reference("tet")
    assert _counts(t) == dict(n_edges=6, n_boundary_edges=0, n_nonmanifold_edges=0, n_links=6, n_inconsistent=0, n_components=1,
                              n_nonorientable=0, n_closed=1, n_flipped_faces=0, n_flipped_components=0, n_kept_faces=4, n_kept_components=1)
    assert t["vol6"] == {0: 64 << 48} and t["comp_flags"].tolist() == [ref.ORIENTABLE | ref.CLOSED | ref.KEPT, 0, 0, 0]
    assert np.array_equal(t["faces_out"], ref.TET_F) and t["comp_faces"].tolist() == [4, 0, 0, 0]
    one = ref.reference("tet_one")
    assert one["counts"][4] == 3 and one["face_flip"].tolist() == [0, 0, 1, 0] and np.array_equal(one["faces_out"], ref.TET_F)
    assert one["vol6"] == {0: 64 << 48} and not one["comp_flags"][0] & ref.FLIPPED
    inward, turned = ref.reference("tet_inward"), ref.reference("tet_inward", ref.OUTWARD)
    assert inward["counts"][8] == 0 and inward["vol6"] == {0: -(64 << 48)}
    assert turned["counts"][8] == 4 and turned["counts"][9] == 1 and turned["vol6"] == {0: 64 << 48}
    assert np.array_equal(turned["faces_out"], ref.TET_F) and turned["comp_flags"][0] & ref.FLIPPED
    assert np.array_equal(ref.reference("tet_one", ref.OUTWARD)["faces_out"], ref.TET_F)


@pytest.mark.parametrize("name,faces,links", [("moebius_q", 8, 8), ("moebius_t", 16, 16)])
def test_moebius_strip_is_reported_and_left_alone(name, faces, links):
    v, f = ref.CASES[name]()
    for sign in (ref.MAJORITY, ref.OUTWARD):
        r = ref.reference(name, sign)
        c = _counts(r)
        assert f.shape[0] == faces and (c["n_links"], c["n_inconsistent"], c["n_components"], c["n_nonorientable"]) == (links, 1, 1, 1)
        assert c["n_closed"] == 0 and c["n_flipped_faces"] == 0 and c["n_boundary_edges"] == 16
        assert np.array_equal(r["faces_out"], f) and r["comp_flags"][0] == ref.KEPT and not r["rel"].any()
        assert r["vol6"][0] == mn.normals(v, f)["vol6"]         # the sum of its faces as given


def test_checkerboard_is_an_exact_tie():
    v, f = ref.CASES["sheet_checker"]()
    r = ref.reference("sheet_checker")
    assert r["n_rel"] == {0: 32} and f.shape[0] == 64 and r["counts"][4] == r["counts"][3] == 112
    assert r["counts"][8] == 32 and r["counts"][9] == 0 and r["face_flip"][0] == 0
    assert np.array_equal(r["faces_out"], ref.sm.sheet_case(True)[1])


@pytest.mark.parametrize("name,base,faces,links,bad_links,closed", [("sheet_q_scr", "sheet_q", 64, 112, 64, 0), ("sphere6_q_scr", "sphere6_q", 726, 1452, 694, 1),
                                                                   ("sphere6_t_scr", "sphere6_t", 1452, 2178, 1072, 1), ("surface_scr", "surface", 4600, 6802, 3343, 0)])
def test_scrambled_meshes_recover_exactly_the_reversed_faces(name, base, faces, links, bad_links, closed):
    """One piece: the flips are rev ^ rev[0] or its complement by rule 6, and the result is the consistent mesh or its mirror. The inconsistent
    links are those the rule `default_rng(5).random(F) < 0.5` gives: every link whose two faces differ in rev."""
    v, f, rev = ref.scramble(base)
    _, clean = ref.sm.CASES[base]()
    assert not ref.orient(v, clean)["counts"][4]                # the case itself is consistent
    for sign in (ref.MAJORITY, ref.OUTWARD):
        r = ref.reference(name, sign)
        c = _counts(r)
        assert (f.shape[0], c["n_links"], c["n_inconsistent"], c["n_components"], c["n_closed"]) == (faces, links, bad_links, 1, closed)
        flip = r["face_flip"].astype(bool)
        assert np.array_equal(flip, rev ^ rev[0]) or np.array_equal(flip, ~(rev ^ rev[0]))
        assert np.array_equal(r["rel"].astype(bool), rev ^ rev[0])
        mirror = not np.array_equal(flip, rev)
        assert np.array_equal(r["faces_out"], ref.flipped(clean) if mirror else clean)
        if closed and sign == ref.OUTWARD:                      # the mesher's quads are counter-clockwise seen from outside
            assert not mirror and r["vol6"][0] == mn.reference(base)["vol6"] > 0


def test_soup_pieces_and_links():
    r = ref.reference("soup")
    c = _counts(r)
    assert (c["n_components"], c["n_links"], c["n_closed"], c["n_nonorientable"]) == (19834, 166, 0, 0)
    assert collections.Counter(r["comp_faces"][r["comp_faces"] > 0].tolist())[1] > 19000


def test_thousand_tetrahedra_with_the_filter():
    v, f = ref.CASES["tets1000"]()
    out = ref.reference("tets1000", ref.OUTWARD)
    c = _counts(out)
    assert (c["n_components"], c["n_closed"], c["n_inconsistent"], c["n_flipped_components"]) == (1000, 1000, 1002, 500)
    assert all(x == 64 << 48 for x in out["vol6"].values())     # every one outward afterwards
    assert np.array_equal(out["faces_out"], (ref.TET_F[None] + 4 * np.arange(1000)[:, None, None]).reshape(-1, 3))
    few = ref.reference("tets1000", ref.MAJORITY, 5, 1)
    assert few["counts"][10:].tolist() == [4, 1] and few["face_keep"].tolist() == [1] * 4 + [0] * 3996      # all tie at 4 faces: the smallest id
    assert ref.reference("tets1000", ref.MAJORITY, 5, 0)["counts"][10:].tolist() == [0, 0]
    assert ref.reference("tets1000", ref.MAJORITY, 4, 0)["counts"][10:].tolist() == [4000, 1000]


def test_strip_far_cube_fin_and_rules():
    s = _counts(ref.reference("strip3000"))
    assert (s["n_links"], s["n_inconsistent"], s["n_components"], s["n_flipped_faces"]) == (2999, 2999, 1, 1500)
    cube = ref.reference("far_cube_in", ref.OUTWARD)
    side = 2097000 * 65536
    assert cube["vol6"] == {0: 6 * side ** 3} and cube["counts"][8] == 12 and ref.reference("far_cube_in")["vol6"] == {0: -6 * side ** 3}
    q, f, _ = mn.quantise(*ref.CASES["far_cube_in"]())
    terms = [int((q[a] * mn._cross(q[b][None], q[c][None])[0]).sum()) for a, b, c in f.tolist()]
    assert max(abs(t) for t in terms).bit_length() == 111 and min(terms) < 0 < max(terms)      # side^3 each; their sum takes 114 bits
    assert (6 * side ** 3).bit_length() == 114 and cube["comp_vol6"][0].tolist() == mn.limbs(6 * side ** 3) and cube["comp_vol6"][0][1] != 0
    inward = ref.reference("far_cube_in")["comp_vol6"][0].tolist()
    assert inward == mn.limbs(-6 * side ** 3) and inward[2] == 2 ** 64 - 1      # negative: the borrow crosses both limb boundaries
    fin = _counts(ref.reference("fin"))
    assert (fin["n_nonmanifold_edges"], fin["n_links"], fin["n_components"]) == (1, 0, 3)
    v, f = ref.CASES["rules"]()
    r = ref.reference("rules")
    assert np.isnan(v[6, 0]) and 6 not in f
    assert r["face_component"].tolist() == [0, 1, 2, 3, 3] and r["counts"][3:6].tolist() == [1, 1, 4]
    assert r["face_flip"].tolist() == [0, 0, 0, 0, 1] and r["faces_out"][4].tolist() == [1, 3, 2]      # a tie of two: face 3 stays
    assert r["comp_flags"].tolist() == [9, 9, 9, 9, 0] and r["counts"][:3].tolist() == [9, 7, 0]        # (a,b,a): an edge of two sides, no boundary, no link
    rq = ref.reference("rules_q")
    assert rq["counts"][2] == 1 and rq["face_component"].tolist() == [0, 1, 1] and rq["faces_out"][2].tolist() == [1, 4, 5, 2]


def test_two_spheres():
    maj, out = ref.reference("two_spheres"), ref.reference("two_spheres", ref.OUTWARD)
    assert _counts(maj)["n_components"] == _counts(maj)["n_closed"] == 2 and _counts(maj)["n_flipped_components"] == 0
    assert _counts(out)["n_flipped_components"] == 1
    first, second = sorted(out["vol6"])
    assert first == 0 and second == 1452 and out["vol6"][first] == out["vol6"][second] == mn.reference("sphere6_t")["vol6"]
    assert maj["vol6"][second] == -out["vol6"][second]


# ---- an independent statement: breadth-first propagation over face adjacency, plain Python ----------------------------------------------------------
def _bfs(f):
    """-> (comp, rel, nonorientable per face, links, inconsistent)."""
    F, nv = f.shape
    sides = collections.defaultdict(list)
    for i, row in enumerate(f.tolist()):
        for k in range(nv):
            p, r = row[k], row[(k + 1) % nv]
            if p != r:
                sides[(min(p, r), max(p, r))].append((i, p < r))
    nbr = [[] for _ in range(F)]
    links = bad_links = 0
    for s in sides.values():
        if len(s) == 2 and s[0][0] != s[1][0]:
            links += 1
            bad_links += s[0][1] == s[1][1]
            nbr[s[0][0]].append((s[1][0], s[0][1] == s[1][1]))
            nbr[s[1][0]].append((s[0][0], s[0][1] == s[1][1]))
    comp, rel, nonor = [-1] * F, [0] * F, [False] * F
    for start in range(F):
        if comp[start] >= 0:
            continue
        comp[start], members, clash = start, [start], False
        queue = collections.deque([start])
        while queue:
            i = queue.popleft()
            for j, differs in nbr[i]:
                if comp[j] < 0:
                    comp[j], rel[j] = start, rel[i] ^ differs
                    members.append(j)
                    queue.append(j)
                elif rel[j] != rel[i] ^ differs:
                    clash = True
        if clash:
            for j in members:
                rel[j], nonor[j] = 0, True
    return comp, rel, nonor, links, bad_links


@pytest.mark.parametrize("name", [n for n in ref.CASES if n != "soup"])
def test_restatement_against_breadth_first_propagation(name):
    v, f = ref.CASES[name]()
    assert f.shape[0] < 5000
    r = ref.reference(name)
    comp, rel, nonor, links, bad_links = _bfs(np.asarray(f, np.int64))
    assert r["face_component"].tolist() == comp and r["rel"].tolist() == rel
    assert [not r["comp_flags"][c] & ref.ORIENTABLE for c in comp] == nonor
    assert r["counts"][3:5].tolist() == [links, bad_links]


# ---- rule 10 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tet_one", "moebius_q", "sheet_checker", "sphere6_t_scr", "surface_scr", "tets1000", "two_spheres", "rules"])
@pytest.mark.parametrize("sign", [ref.MAJORITY, ref.OUTWARD])
def test_running_it_on_its_own_output_flips_nothing(name, sign):
    v, f = ref.CASES[name]()
    r = ref.reference(name, sign)
    again = ref.orient(v, r["faces_out"], sign)
    assert not again["face_flip"].any() and np.array_equal(again["faces_out"], r["faces_out"])
    assert again["vol6"] == r["vol6"] and np.array_equal(again["face_component"], r["face_component"])
    inside = again["comp_flags"][again["face_component"]] & ref.ORIENTABLE == 0
    assert again["counts"][4] == (1 if name == "moebius_q" else 0) and (again["counts"][4] == 0 or inside.all())


@pytest.mark.parametrize("name,base", [("sphere6_q_scr", "sphere6_q"), ("sphere6_t_scr", "sphere6_t")])
def test_outward_volume_is_the_consistent_meshs(name, base):
    v, clean = ref.sm.CASES[base]()
    r = ref.reference(name, ref.OUTWARD)
    assert r["vol6"][0] == abs(mn.normals(v, clean)["vol6"]) == mn.normals(v, r["faces_out"])["vol6"]
    assert mn.limbs(r["vol6"][0]) == r["comp_vol6"][0].tolist()


def test_reversing_every_face_changes_the_flips_only_through_rule_6():
    for name in ("sphere6_t_scr", "surface_scr", "two_spheres"):
        v, f = ref.CASES[name]()
        r, m = ref.reference(name), ref.orient(v, ref.flipped(f))
        assert np.array_equal(m["rel"], r["rel"]) and np.array_equal(m["face_component"], r["face_component"])
        assert np.array_equal(m["face_flip"], r["face_flip"])  # majority: the same faces are the fewer
        assert np.array_equal(m["faces_out"], ref.flipped(r["faces_out"]))
        o, mo = ref.reference(name, ref.OUTWARD), ref.orient(v, ref.flipped(f), ref.OUTWARD)
        closed = (o["comp_flags"][o["face_component"]] & ref.CLOSED) != 0
        assert np.array_equal(mo["face_flip"][closed], 1 - o["face_flip"][closed])      # outward: the same surface comes out
        assert np.array_equal(mo["faces_out"][closed], o["faces_out"][closed])


def test_a_permutation_of_the_faces_permutes_flip_and_keep():
    v, f = ref.CASES["sphere6_t_scr"]()
    r = ref.reference("sphere6_t_scr", ref.MAJORITY, 5, 1)
    assert 2 * r["n_rel"][0] != f.shape[0]                      # no tie
    perm = np.random.default_rng(13).permutation(f.shape[0])
    p = ref.orient(v, f[perm], ref.MAJORITY, 5, 1)
    assert np.array_equal(p["face_flip"], r["face_flip"][perm]) and np.array_equal(p["face_keep"], r["face_keep"][perm])
    assert np.array_equal(p["faces_out"], r["faces_out"][perm]) and sorted(p["vol6"].values()) == sorted(r["vol6"].values())


# ---- a planted fault in each rule fails the comparison ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plant,name,cfg", [("direction", "tet_one", (0, 0, 0)), ("same_face", "rules", (0, 0, 0)), ("tie", "sheet_checker", (0, 0, 0)),
                                            ("negation", "far_cube_in", (1, 0, 0)), ("largest_tie", "tets1000", (0, 5, 1))])
def test_a_planted_fault_is_seen(plant, name, cfg):
    assert plant in ref.PLANTS
    want = ref.reference(name, *cfg)
    assert ref.same_bytes(ref.orient(*ref.CASES[name](), *cfg), want) == []
    assert ref.same_bytes(ref.orient(*ref.CASES[name](), *cfg, plant=plant), want) != []


# ---- mesh.orient_mesh and the chain before the library ---------------------------------------------------------------------------------------------
def test_check_orient_args():
    from surfacenet_amd import mesh
    assert mesh.check_orient_args("majority", 0, False) == (0, 0, 0) and mesh.check_orient_args("outward", 7, True) == (1, 7, 1)
    for args, text in ((("inward", 0, False), "sign = 'inward': 'majority' or 'outward'"), ((1, 0, False), "sign = 1: 'majority' or 'outward'"),
                       (("outward", -1, False), "min_faces = -1: an integer number of faces >= 0"),
                       (("outward", 2.5, False), "min_faces = 2.5: an integer number of faces >= 0"),
                       (("outward", "a", False), "min_faces = 'a' must be an integer"), (("outward", True, False), "min_faces = True: an integer number of faces >= 0"),
                       (("outward", 0, 1), "keep_largest = 1: True or False"), (("outward", 0, "yes"), "keep_largest = 'yes': True or False")):
        with pytest.raises(ValueError) as e:
            mesh.check_orient_args(*args)
        assert str(e.value) == text


def test_orient_mesh_refuses_a_bad_mesh_in_the_stages_words(monkeypatch):
    from surfacenet_amd import mesh
    _no_library(monkeypatch)
    v, f = bad.sheet()
    cases = [bad.bad_index(v, f, 2, 5)] + [bad.bad_coordinate(v, f, 3, value) for value in (np.nan, 2097144.0)]
    cases += [(v.astype(np.int32), f, "vert_lattice must be float32 or float64, not int32"), (v, np.zeros((18, 5), np.int32), "faces must be (F,3) or (F,4), not (18, 5)"),
              (np.zeros((0, 3)), f, "face 0 names a vertex outside [0, 0)")]
    for bv, bf, text in cases:
        for run in (mesh.orient_mesh, mesh.smooth_mesh):
            with pytest.raises(ValueError) as e:
                run(bv, bf)
            assert str(e.value) == text
    for bv, bf, text in cases[:3]:
        with pytest.raises(ValueError) as e:
            ref.orient(bv, bf)
        assert str(e.value) == text
    with pytest.raises(ValueError, match="sign = 'up'"):
        mesh.orient_mesh(v, f, sign="up")
    with pytest.raises(ValueError, match="resol = 0"):
        mesh.orient_mesh(v, f, resol=0)
    for vv, ff in ((v, np.zeros((0, 4), np.int32)), (np.zeros((0, 3)), np.zeros((0, 3), np.int32))):      # no face: without the library
        e = mesh.orient_mesh(vv, ff, "outward", 3, True)
        assert e["faces"].shape == ff.shape and e["faces"].dtype == np.int32 and e["face_src"].shape == (0,) and e["face_keep"].dtype == bool
        assert [e[k] for k in mesh.ORIENT_COUNTS] == [0] * 12 and e["components"]["vol6"] == [] and e["components"]["id"].shape == (0,)
    assert mesh.ORIENT_COUNTS == ref.COUNTS


def test_the_chains_fourth_row(monkeypatch):
    from surfacenet_amd import mesh, reconstruct
    _no_library(monkeypatch)
    full = dict(sign="outward", min_faces=0, keep_largest=False)
    assert mesh.chain_settings(None, None, None, "mean", "outward") == [("oriented", full)] == mesh.chain_settings(mesh_orient="outward")
    stages = mesh.chain_settings(mc.FILL, mc.SMOOTH, mc.CELL, "mean", dict(min_faces=9, keep_largest=True))
    assert [k for k, _ in stages] == ["filled", "smoothed", "simplified", "oriented"]
    assert stages[3][1] == dict(sign="majority", min_faces=9, keep_largest=True) and stages[:3] == mesh.chain_settings(mc.FILL, mc.SMOOTH, mc.CELL, "mean")
    assert [mesh.stage_tag(k, kw) for k, kw in stages] == ["_f16", "_s2", "_c2", "_o"]
    for value, text in (("up", "sign = 'up': 'majority' or 'outward'"), (3, "sign = 3: 'majority' or 'outward'"),
                        (dict(sign="outward", min_faces=-2), "min_faces = -2: an integer number of faces >= 0"),
                        (dict(cell=2), "mesh_orient = {'cell': 2}: a sign word or a dict of sign, min_faces, keep_largest")):
        with pytest.raises(ValueError) as e:
            mesh.chain_settings(2, -1, 1, "mean", value)        # the new argument is the first one judged
        assert str(e.value) == text
    empty = dict(prediction_list=[], vxl_ijk_list=[], rayPooling_votes_list=[], cube_ijk_np=np.zeros((0, 3), np.int64))
    cams = np.zeros((2, 3))
    with pytest.raises(ValueError) as e:
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh_orient="outward")
    assert str(e.value) == "mesh_orient needs mesh=True: it orients the mesh that mesh=True extracts"
    with pytest.raises(ValueError, match="mesh_fill needs mesh=True"):      # the order: cell, smooth, fill, normals, orient
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh_fill=16, mesh_orient="outward")
    with pytest.raises(ValueError, match="sign = 'up'"):
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_orient="up")


@pytest.mark.parametrize("combo", mc.COMBOS)
def test_run_chain_on_the_empty_mesh_with_the_fourth_stage(combo, monkeypatch):
    from surfacenet_amd import mesh, reconstruct
    _no_library(monkeypatch)
    old = mesh.run_chain(mesh.empty_mesh(), mesh.chain_settings(*combo, "mean"), (0.0, 0.0, 0.0), 1.0)
    got = mesh.run_chain(mesh.empty_mesh(), mesh.chain_settings(*combo, "mean", "outward"), (0.0, 0.0, 0.0), 1.0)
    assert list(got) == mc.asked(combo) + ["oriented"]
    for key in old:                                             # the three old stages: unchanged
        mc.same_dict(got[key], old[key])
    before = old[mc.asked(combo)[-1]] if mc.asked(combo) else mesh.empty_mesh()
    faces = "quads" if combo[0] is None and combo[2] is None else "faces"
    e = got["oriented"]
    carried = set(before) if mc.asked(combo)[-1:] in ([], ["smoothed"]) else set()      # (a new mesh hands on its four keys only)
    assert set(e) == {"vertices", "vert_lattice", "vert_src", faces} | (carried - {"quads", "faces"}) | set(mesh.ORIENT_COUNTS) | {
        "face_src", "face_flip", "face_component", "face_keep", "components"}
    assert e[faces].shape == before[faces].shape and e[faces].dtype == np.int32 and e["n_inconsistent"] == 0 and e["vert_src"].dtype == np.int64
    empty = dict(prediction_list=[], vxl_ijk_list=[], rayPooling_votes_list=[], cube_ijk_np=np.zeros((0, 3), np.int64))
    fill, smooth, cell = combo
    kw = dict(cameraTs_np=np.zeros((2, 3)), mesh=True, mesh_fill=fill, mesh_smooth=smooth, mesh_cell=cell)
    plain, none = reconstruct.scene_postpass(empty, 32, 26, 2, **kw), reconstruct.scene_postpass(empty, 32, 26, 2, mesh_orient=None, **kw)
    post = reconstruct.scene_postpass(empty, 32, 26, 2, mesh_orient="outward", mesh_ply_prefix="/nonexistent/x_", **kw)
    assert set(none) == set(plain) and set(post) - set(plain) == {"fixThresh_mesh_oriented", "adapt_mesh_oriented"}
    for key in plain:
        if key.endswith("_mesh") or "_mesh_" in key:
            mc.same_dict(post[key], plain[key])
            mc.same_dict(none[key], plain[key])
    assert set(post["adapt_mesh_oriented"]) == set(e)


# ---- the ABI: symbols are only added ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_version_script_binding_and_library():
    import fnmatch
    import re
    import __graft_entry__ as g
    g.build()
    from surfacenet_amd import _lib
    new = ("sn_mesh_orient", "sn_mesh_orient_dev")
    txt = open(os.path.join(ROOT, "include", "surfacenet_hip.h")).read()
    assert "#define SN_ABI_VERSION 2" in txt and "sn_mesh_orient_cfg" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    pattern = re.search(r"global:\s*([^;]+);", open(os.path.join(CSRC, "exports.map")).read()).group(1).strip()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode().split()
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert fnmatch.fnmatchcase(name, pattern), (name, pattern)
        assert name in _lib.ABI_SYMBOLS and name in exported, name
    lib = _lib.load()
    assert lib.sn_version() == 2 and all(hasattr(lib, name) for name in new)
    assert "sn_meshorient.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_the_rules_header_is_hip_free():
    with open(os.path.join(CSRC, "meshorient_rules.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes and all("hip/" not in i and i in ("<stdint.h>", '"meshnormals_sum.h"') for i in includes), includes


# ---- the rules and the argument checks of the C entry, on the CPU ----------------------------------------------------------------------------------
def test_rules_and_argument_checks_under_sanitizers(tmp_path):
    """tests/host/meshorient_check.cpp runs csrc/meshorient_rules.h - the side code at the largest face, the link relation, the flipped face,
    the sign and the negation of a three-limb sum across both limb boundaries, rules 6 and 8 with their ties - and sn_host.h's mor_check_args
    over every end of every range, compiled stand-alone with -fsanitize=address,undefined and run as a child process."""
    exe = str(tmp_path / "meshorient_check")
    _compile(os.path.join(ROOT, "tests", "host", "meshorient_check.cpp"), exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "MESHORIENT-CHECK-OK" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
