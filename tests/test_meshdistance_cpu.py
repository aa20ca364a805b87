"""CPU: the restatement of the point-to-mesh distance stage (tests/meshdistance_ref.py) against exact rational
arithmetic, on its degenerate triangles, on the consequences of its rules (rule 7), at the cap's edge and on an error planted in each rule;
the argument checks of mesh.point_to_mesh, the layers above it on a stand-in context that IS the restatement, and the keyword of the scene
post-pass, all before the library is touched; the new symbols in header, version script and binding; and csrc/meshdistance_rules.h with
mdi_check_args of csrc/sn_host.h compiled alone under the sanitizers and run as a child process, its answers compared with the
restatement's bit for bit."""
import os
import struct
import subprocess

import numpy as np
import pytest

import mesh_refusals as bad
import meshchain_util as mc
import meshdistance_ref as ref
import meshsample_ref as sref
import pointeval_ref as pref
from test_host_plumbing import CSRC, ROOT, _compile

# |d - d_exact| <= K_EXACT x the largest coordinate magnitude: 4 x the worst value the cases of test_restatement_against_exact_rationals
# measure (3.3e-16, profiles/meshdistance/README.md): it covers rounding, not a design choice.
K_EXACT = 4 * 3.3e-16
# mesh_deviation of a mesh against itself, in mm on 400 faces of the R = 6 shell at resol 0.4, dst 0.2: 4 x the worst distance the
# restatement measures there (1.8e-15, profiles/meshdistance/README.md)
SELF_DEVIATION = 4 * 1.8e-15


def _no_library(monkeypatch):
    from surfacenet_amd import runtime

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(runtime, "any_context", no_library)


class StandIn(pref.RefContext):
    """A context whose mesh_sample and mesh_distance are the restatements (point_reduce, nn_dist2 and point_flags are pointeval_ref's)."""

    def mesh_sample(self, vertices, faces, dst, cap=None, device=False):
        return sref.sample(vertices, faces, dst)

    def mesh_distance(self, verts, faces, pts, max_dist, outputs=("d2", "face", "closest"), device=False):
        return ref.distance(verts, faces, pts, max_dist)


def _stand_in(monkeypatch):
    from surfacenet_amd import runtime
    ctx = StandIn()
    monkeypatch.setattr(runtime, "any_context", lambda: ctx)


# ---- the restatement itself ------------------------------------------------------------------------------------------------------------------------
def test_restatement_against_exact_rationals():
    worst = 0.0
    for scale in ref.SCALES:
        for offset in ref.OFFSETS:
            v, f, pts, names = ref.single_triangle(scale, offset)
            for p in pts:
                worst = max(worst, ref.exact_error(p, v[0], v[1], v[2]))
            for row in ref.dyadic_triangles(100, scale, offset, seed=11):
                worst = max(worst, ref.exact_error(*row))
    print("worst |d - d_exact| / magnitude = %.3g (bound %.3g)" % (worst, K_EXACT))
    assert worst <= K_EXACT


def test_single_triangle_regions_answer_what_they_were_built_for():
    v, f, pts, names = ref.single_triangle()
    r = ref.distance(v, f, pts, 100.0)
    by = dict(zip(names, zip(r["d2"].tolist(), r["closest"].tolist())))
    assert by["inside_above"] == (2.25, [1.0, 0.75, 0.0]) and by["inside_plane"] == (0.0, [1.0, 0.75, 0.0])
    assert by["edge_ab_plane"][1] == [2.0, 0.0, 0.0] and by["edge_ca_below"][1] == [0.0, 1.5, 0.0]
    assert by["corner_a_above"][1] == [0.0, 0.0, 0.0] and by["corner_b_plane"][1] == [4.0, 0.0, 0.0] and by["corner_c_below"][1] == [0.0, 3.0, 0.0]
    assert by["at_corner_b"] == (0.0, [4.0, 0.0, 0.0]) and by["on_edge_bc"][0] == 0.0 and by["on_edge_ab"] == (0.0, [1.0, 0.0, 0.0])
    assert np.allclose(by["edge_bc_plane"][1], [2.28, 1.29, 0.0], atol=1e-12) and (r["face"] == 0).all()
    assert r["counts"].tolist() == [1, 0, len(names), 0, len(names), 0, 0, 0]


def test_degenerate_triangles_are_their_segments_and_points():
    v, f, pts = ref.degenerate_mesh()
    r = ref.distance(v, f, pts, 100.0)
    assert np.isfinite(r["d2"]).all() and np.isfinite(r["closest"]).all()
    assert r["counts"][:4].tolist() == [4, 3, 9, 0]
    seg = lambda p, a, b: float(ref.segment(ref._xyz(np.asarray(p)), ref._xyz(np.asarray(a)), ref._xyz(np.asarray(b)))[0])
    assert r["face"].tolist() == [1, 1, 1, 2, 2, 2, 3, 3, 0]
    assert r["d2"][:3].tolist() == [seg(p, v[3], v[4]) for p in pts[:3]] == [1.0, 2.0, 2.0]      # the repeated index: segment 3-4
    assert r["d2"][3:6].tolist() == [seg(p, v[5], v[7]) for p in pts[3:6]] == [1.0, 5.0, 2.0]      # collinear: the segment of its ends
    assert r["d2"][6:8].tolist() == [1.0, 3.0] and (r["closest"][6:8] == 9.0).all()                # coincident: its point
    alone = ref.distance(v, f[1:], pts, 100.0)                                                     # no good triangle at all
    assert np.isfinite(alone["d2"]).all() and alone["counts"][:2].tolist() == [3, 3]


def test_rule_7_permutations_triangulation_and_vertices():
    from surfacenet_amd import mesh
    v, q = ref.shell()
    pts = ref.shell_queries()[::4]
    base = ref.distance(v, q, pts, ref.SHELL_MAX_DIST)
    rng = np.random.RandomState(2)
    perm = rng.permutation(q.shape[0])
    scr = ref.distance(v, q[perm], pts, ref.SHELL_MAX_DIST)
    assert ref.same_bits(scr, base, ("d2", "counts")) == []
    ok = base["face"] >= 0
    assert ok.sum() > 100 and (scr["face"][~ok] == -1).all()
    # closest stays - but for a query with two nearest points (the shell is symmetric: a lattice point in a mirror plane has them), where
    # rule 3 takes the smaller triangle index, whichever triangle now has it: the same d2 from the other point
    same = ok & (scr["closest"] == base["closest"]).all(axis=1)
    tie = ok & ~same
    assert tie.sum() <= 3 and (ref._dot(ref._xyz(pts[tie] - scr["closest"][tie]), ref._xyz(pts[tie] - scr["closest"][tie])) == base["d2"][tie]).all()
    # the face is relabelled: the face named now attains the minimum under its old label too (a vertex ties its faces; the index decides)
    for k in np.nonzero(ok)[0][::3]:
        one = ref.distance(v, q[perm[scr["face"][k]]][None], pts[k][None], ref.SHELL_MAX_DIST)
        assert one["d2"][0] == base["d2"][k] and perm[scr["face"][k]] >= base["face"][k]
    untied = ok & (base["d2"] > 0.0) & same
    assert (perm[scr["face"][untied]] == base["face"][untied]).sum() > untied.sum() // 2
    order = rng.permutation(pts.shape[0])
    shuffled = ref.distance(v, q, pts[order], ref.SHELL_MAX_DIST)
    for k in ("d2", "face", "closest"):
        assert shuffled[k].tobytes() == base[k][order].tobytes(), k
    tris = ref.distance(v, mesh.triangulate(q), pts, ref.SHELL_MAX_DIST)
    assert tris["d2"].tobytes() == base["d2"].tobytes() and tris["closest"].tobytes() == base["closest"].tobytes()
    assert np.array_equal(np.where(tris["face"] >= 0, tris["face"] // 2, -1), base["face"])
    own = ref.distance(v, q, v, ref.SHELL_MAX_DIST)
    assert (own["d2"] == 0.0).all() and own["closest"].tobytes() == v.tobytes()


def test_the_shell_case_is_what_the_gpu_test_says_it_is():
    """About 1,000 queries: the shell's own vertices (d2 == 0.0 exactly), lattice points within 3 cells of it, and 5 % of the points chosen
    beyond the cap - the restatement alone puts between 1 % and 10 % there. The other named cases in a line each."""
    v, q, pts, max_dist = ref.CASES["shell"]()
    r = ref.reference("shell")
    assert 1000 <= pts.shape[0] <= 1100 and (r["d2"][:v.shape[0]] == 0.0).all() and r["counts"][0] == 2 * q.shape[0] == 1452
    assert 0.01 <= r["counts"][3] / pts.shape[0] <= 0.10 and r["counts"][2] + r["counts"][3] == pts.shape[0]
    moved = ref.reference("shell_500")
    assert np.array_equal(moved["face"] >= 0, r["face"] >= 0) and np.abs(moved["d2"][r["face"] >= 0] - r["d2"][r["face"] >= 0]).max() < 1e-10      # (at 500 mm rounding breaks the ties its own way: the faces may differ, the distances do not)
    assert ref.reference("far_hit")["counts"][2:4].tolist() == [7, 0] and ref.reference("far_miss")["counts"][2:4].tolist() == [0, 7]
    big = ref.CASES["big_and_small"]()
    assert big[1].shape[0] == 301 and (ref.reference("big_and_small")["face"] == 300).sum() >= 40      # the spanning triangle is many points' nearest
    assert ref.CASES["fan"]()[1].shape[0] == 300 and ref.reference("fan")["d2"][0] == 0.0 and ref.reference("fan")["face"][0] == 0
    lv, lf, lp, ld = ref.CASES["late_cells"]()
    assert ref.grid_level(lv, lf, ld, budget=1)[::2] == (ref.LATE_LEVEL, 1.0) and lf.shape[0] == ref.LATE_N + 2


def test_the_caps_edge():
    v, f = ref.TRI, np.asarray([[0, 1, 2]], np.int32)
    d = 1.5
    at, ulp, past = d, np.nextafter(d, 2.0), d * (1.0 + 2.0 ** -39)
    r = ref.distance(v, f, np.asarray([[1.0, 0.75, at], [1.0, 0.75, ulp], [1.0, 0.75, past]]), d)
    assert r["d2"][0] == d * d and r["face"].tolist() == [0, 0, -1]      # exactly max_dist and one ulp beyond it: answered, within the slack
    assert r["d2"][1] > d * d and np.isinf(r["d2"][2]) and np.isnan(r["closest"][2]).all() and r["counts"][2:4].tolist() == [2, 1]
    assert past * past >= ref.limit(d) > ulp * ulp
    none = ref.distance(v, np.zeros((0, 3), np.int32), np.asarray([[1.0, 0.75, 0.0]]), d)
    assert np.isinf(none["d2"]).all() and none["face"].tolist() == [-1] and np.isnan(none["closest"]).all() and none["counts"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0]


@pytest.mark.parametrize("plant,case,changed", [("open", "neg_zero_corner", ["closest"]), ("no_inside", "outside_case", ["d2", "closest"]),
                                                ("u_plus_e", "u_plus_e_case", ["d2", "closest"]), ("tie_large", "tie_case", ["face"]),
                                                ("half_quad", "quad_case", ["d2", "closest", "counts"])])
def test_a_planted_error_is_seen(plant, case, changed):
    assert plant in ref.PLANTS
    v, f, pts = getattr(ref, case)()
    want = ref.distance(v, f, pts, 100.0)
    assert ref.same_bits(ref.distance(v, f, pts, 100.0), want) == []
    assert ref.same_bits(ref.distance(v, f, pts, 100.0, plant=plant), want) == changed


# ---- mesh.point_to_mesh and the layers above it, before the library ----------------------------------------------------------------------------------
def test_check_distance_args():
    from surfacenet_amd import mesh
    p, d = mesh.check_distance_args(np.zeros((2, 3), np.float32))
    assert p.dtype == np.float64 and p.shape == (2, 3) and d == 60.0
    pts = np.zeros((3, 3))
    nan = pts.copy()
    nan[1, 2] = np.nan
    for points, max_dist, text in ((pts.astype(np.int32), 1.0, "points must be float32 or float64, not int32"), (np.zeros((3, 2)), 1.0, "points must be (n,3), not (3, 2)"),
                                   (pts, 0.0, "max_dist = 0.0 must be finite and > 0"), (pts, -1, "max_dist = -1 must be finite and > 0"),
                                   (pts, np.inf, "max_dist = inf must be finite and > 0"), (pts, "far", "max_dist = 'far' must be a number"),
                                   (pts, True, "max_dist = True must be finite and > 0"), (nan, 1.0, "point 1: a coordinate is not finite")):
        with pytest.raises(ValueError) as e:
            mesh.check_distance_args(points, max_dist)
        assert str(e.value) == text


def test_point_to_mesh_refuses_in_the_stages_words(monkeypatch):
    from surfacenet_amd import mesh
    _no_library(monkeypatch)
    v, f = bad.sheet()
    pts = np.zeros((2, 3))
    bv, bf, text = bad.bad_index(v, f, 2, 5)
    nanv = v.copy()
    nanv[bad.first_used_by(f, 3), 1] = np.inf
    for vv, ff, text in ((bv, bf, text), (nanv, f, "face 3: a coordinate of one of its vertices is not finite"),
                         (v.astype(np.int32), f, "vertices must be float32 or float64, not int32"), (v, np.zeros((18, 5), np.int32), "faces must be (F,3) or (F,4), not (18, 5)"),
                         (np.zeros((0, 3)), f, "face 0 names a vertex outside [0, 0)")):
        with pytest.raises(ValueError) as e:
            mesh.point_to_mesh(pts, vv, ff)
        assert str(e.value) == text
    with pytest.raises(ValueError, match="point 0: a coordinate is not finite"):
        mesh.point_to_mesh(pts + np.nan, v, f)
    with pytest.raises(ValueError, match="max_dist = -2"):
        mesh.point_to_mesh(pts, v, f, max_dist=-2)
    unreferenced = np.concatenate([v, [[np.nan, 0, 0]]])       # an unreferenced vertex may hold anything
    for pp, vv, ff in ((np.zeros((0, 3)), unreferenced, f), (pts, np.zeros((0, 3)), np.zeros((0, 4), np.int32))):      # no point, no vertex: without the library
        r = mesh.point_to_mesh(pp, vv, ff, max_dist=5.0)
        n = pp.shape[0]
        assert r["dist2"].shape == (n,) and np.isinf(r["dist2"]).all() and (r["dist"] == 5.0).all() and r["face"].dtype == np.int32 and (r["face"] == -1).all()
        assert r["closest"].shape == (n, 3) and np.isnan(r["closest"]).all() and [r[k] for k in mesh.DISTANCE_COUNTS] == [0, 0, 0, n]
    assert mesh.DISTANCE_COUNTS == ref.COUNTS[:4]


def test_point_to_mesh_on_the_stand_in(monkeypatch):
    from surfacenet_amd import mesh
    _stand_in(monkeypatch)
    v, q = ref.shell()
    pts = ref.shell_queries()[::5]
    want = ref.distance(v, q, pts, ref.SHELL_MAX_DIST)
    got = mesh.point_to_mesh(pts, v, q.astype(np.int64), max_dist=ref.SHELL_MAX_DIST)
    assert got["dist2"].tobytes() == want["d2"].tobytes() and np.array_equal(got["face"], want["face"]) and got["closest"].tobytes() == want["closest"].tobytes()
    assert np.array_equal(got["dist"], np.minimum(np.sqrt(want["d2"]), ref.SHELL_MAX_DIST)) and got["dist"].max() == ref.SHELL_MAX_DIST
    assert [got[k] for k in mesh.DISTANCE_COUNTS] == want["counts"][:4].tolist() and got["n_beyond"] > 0


def test_mesh_deviation_against_itself_and_a_translated_copy(monkeypatch):
    from surfacenet_amd import mesh
    _stand_in(monkeypatch)
    v, f = sref.sphere_mesh()
    v, f = v[: int(f[:400].max()) + 1], f[:400]                 # a cap of the shell, in mm
    dst = 0.2
    own = mesh.mesh_deviation(v, f, v, f, dst)
    n = sref.sample(v, f, dst)[0].shape[0]
    assert set(own) == {"a_to_b", "b_to_a", "hausdorff"} and set(own["a_to_b"]) == {"n", "n_beyond", "max", "mean", "rms"}
    assert own["a_to_b"] == own["b_to_a"] and own["a_to_b"]["n"] == n > 400 and own["a_to_b"]["n_beyond"] == 0
    print("mesh against itself: max %.3g mean %.3g (bound %.3g)" % (own["hausdorff"], own["a_to_b"]["mean"], SELF_DEVIATION))
    assert 0.0 < own["hausdorff"] == own["a_to_b"]["max"] <= SELF_DEVIATION and own["a_to_b"]["mean"] <= own["a_to_b"]["rms"] <= own["a_to_b"]["max"]
    t = 0.25
    moved = mesh.mesh_deviation(v, f, v + [t, 0.0, 0.0], f, dst)
    for key in ("a_to_b", "b_to_a"):                            # a sample moved by t lies on the other mesh: at most t
        assert 0.0 < moved[key]["mean"] <= moved[key]["rms"] <= moved[key]["max"] <= t and moved[key]["n"] == n
    assert moved["hausdorff"] == max(moved["a_to_b"]["max"], moved["b_to_a"]["max"])
    capped = mesh.mesh_deviation(v, f, v + [5.0, 0.0, 0.0], f, dst, max_dist=1.0)
    assert capped["hausdorff"] == 1.0 and capped["a_to_b"]["n_beyond"] > 0
    empty = mesh.mesh_deviation(v, f, np.zeros((0, 3)), np.zeros((0, 3), np.int32), dst, max_dist=7.0)
    assert empty["a_to_b"] == dict(n=n, n_beyond=n, max=7.0, mean=7.0, rms=7.0) and empty["b_to_a"]["n"] == 0 and empty["hausdorff"] == 7.0
    with pytest.raises(ValueError, match="dst = 0"):
        mesh.mesh_deviation(v, f, v, f, 0)


MASK = np.ones((30, 30, 30), np.uint8)
BB, RES, PLANE = np.asarray([[-30.0, -30, -30], [28, 28, 28]]), 2, np.asarray([0.0, 0.0, 1.0, 20.0])


def test_completeness_surface_lies_in_the_bracket_of_the_samples(monkeypatch):
    """Dstl to the surface against Dstl to the samples, both on the restatement: the nearest surface point is no farther than the nearest
    sample, and every point of the surface has a sample within 2/3 sample_dst, so
    Dstl_samples - 2/3 sample_dst <= Dstl_surface <= Dstl_samples (1 + 1e-12)."""
    from surfacenet_amd import evaluation
    _stand_in(monkeypatch)
    v, f = sref.sphere_mesh()
    g = ref.lattice_queries((-15.0, -15.0, -15.0), (-9.0, -9.0, -9.0), 9)      # a lattice around the shell (centre -12 mm, radius 2.4 mm)
    sample_dst = 0.2
    kw = dict(dst=1e-3, sample_dst=sample_dst, max_dist=2.5)   # (a reduction at 1e-3 mm keeps every sample: the bracket is about the samples)
    samples = evaluation.mesh_compare(v, f, g, MASK, BB, RES, PLANE, **kw)
    surface = evaluation.mesh_compare(v, f, g, MASK, BB, RES, PLANE, completeness="surface", **kw)
    assert "completeness" not in samples and surface["completeness"] == "surface" and set(surface) == set(samples) | {"completeness"}
    assert samples["Qdata"].shape[0] == samples["n_samples"]
    for k in samples:
        if k != "Dstl":
            assert np.array_equal(surface[k], samples[k]), k
    lo, hi = samples["Dstl"] - 2.0 / 3.0 * sample_dst, samples["Dstl"] * (1.0 + 1e-12)
    assert (lo <= surface["Dstl"]).all() and (surface["Dstl"] <= hi).all()
    assert (surface["Dstl"] < samples["Dstl"]).sum() > g.shape[0] // 2 and (surface["Dstl"] == 2.5).any()      # nearer nearly everywhere, and capped somewhere
    with pytest.raises(ValueError) as e:
        evaluation.mesh_compare(v, f, g, MASK, BB, RES, PLANE, completeness="both")
    assert str(e.value) == 'completeness = \'both\': "samples" or "surface"'


# ---- the scene post-pass's keyword -------------------------------------------------------------------------------------------------------------------
def test_check_deviation_setting():
    from surfacenet_amd import mesh
    assert mesh.check_deviation_setting(None) is None and mesh.check_deviation_setting(False) is None
    assert mesh.check_deviation_setting(True) == dict(dst=None, max_dist=60.0) == mesh.check_deviation_setting({})
    assert mesh.check_deviation_setting(dict(dst=0.5)) == dict(dst=0.5, max_dist=60.0)
    assert mesh.check_deviation_setting(dict(max_dist=2, dst=1)) == dict(dst=1.0, max_dist=2.0)
    for value, text in ((5, "mesh_deviation = 5: True or a dict of dst, max_dist"), ("yes", "mesh_deviation = 'yes': True or a dict of dst, max_dist"),
                        (dict(cell=2), "mesh_deviation = {'cell': 2}: True or a dict of dst, max_dist"),
                        (dict(dst=0), "dst = 0 must be finite and > 0"), (dict(dst="a"), "dst = 'a' must be a number"),
                        (dict(max_dist=-1), "max_dist = -1 must be finite and > 0")):
        with pytest.raises(ValueError) as e:
            mesh.check_deviation_setting(value)
        assert str(e.value) == text


def test_the_scene_keyword(monkeypatch):
    from surfacenet_amd import mesh, reconstruct
    _no_library(monkeypatch)
    empty = dict(prediction_list=[], vxl_ijk_list=[], rayPooling_votes_list=[], cube_ijk_np=np.zeros((0, 3), np.int64))
    cams = np.zeros((2, 3))
    with pytest.raises(ValueError) as e:
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh_deviation=True)
    assert str(e.value) == "mesh_deviation needs mesh=True: it measures the chain against the mesh that mesh=True extracts"
    with pytest.raises(ValueError, match="mesh_check needs mesh=True"):      # the order: ..., render, check, deviation
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh_check=True, mesh_deviation=True)
    calls = []
    monkeypatch.setattr(mesh, "extract_mesh", lambda *a, **k: calls.append("extract"))
    monkeypatch.setattr(mesh, "run_chain", lambda *a, **k: calls.append("chain"))
    with pytest.raises(ValueError, match="mesh_deviation = 3: True or a dict of dst, max_dist"):      # refused before any stage runs
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_smooth=2, mesh_deviation=3)
    with pytest.raises(ValueError, match="dst = -1"):
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_deviation=dict(dst=-1))
    assert calls == []


@pytest.mark.parametrize("combo", mc.COMBOS[::3])
def test_the_keyword_on_the_empty_scene(combo, monkeypatch):
    from surfacenet_amd import reconstruct
    _no_library(monkeypatch)
    empty = dict(prediction_list=[], vxl_ijk_list=[], rayPooling_votes_list=[], cube_ijk_np=np.zeros((0, 3), np.int64))
    fill, smooth, cell = combo
    kw = dict(cameraTs_np=np.zeros((2, 3)), mesh=True, mesh_fill=fill, mesh_smooth=smooth, mesh_cell=cell)
    plain = reconstruct.scene_postpass(empty, 32, 26, 2, **kw)
    for off in (None, False):                                   # the default: no key, the same dicts
        none = reconstruct.scene_postpass(empty, 32, 26, 2, mesh_deviation=off, **kw)
        assert set(none) == set(plain)
    post = reconstruct.scene_postpass(empty, 32, 26, 2, mesh_deviation=True, mesh_ply_prefix="/nonexistent/x_", **kw)
    assert set(post) - set(plain) == {"fixThresh_mesh_deviation", "adapt_mesh_deviation"}
    zero = dict(n=0, n_beyond=0, max=0.0, mean=0.0, rms=0.0)
    assert post["adapt_mesh_deviation"] == dict(a_to_b=zero, b_to_a=zero, hausdorff=0.0)
    for key in plain:
        if key.endswith("_mesh") or "_mesh_" in key:
            mc.same_dict(post[key], plain[key])


def test_the_keyword_runs_deviation_of_the_last_mesh_against_the_extracted_one(monkeypatch):
    from surfacenet_amd import mesh, reconstruct
    _no_library(monkeypatch)
    seen = []

    def deviation(va, fa, vb, fb, dst, max_dist=60.0):
        seen.append((va, fa, vb, fb, dst, max_dist))
        return dict(hausdorff=float(len(seen)))
    monkeypatch.setattr(mesh, "mesh_deviation", deviation)
    empty = dict(prediction_list=[], vxl_ijk_list=[], rayPooling_votes_list=[], cube_ijk_np=np.zeros((0, 3), np.int64))
    kw = dict(cameraTs_np=np.zeros((2, 3)), mesh=True)
    post = reconstruct.scene_postpass(empty, 32, 26, 2, mesh_cell=2, mesh_smooth=1, mesh_deviation=dict(dst=0.5, max_dist=9.0), **kw)
    assert post["fixThresh_mesh_deviation"] == dict(hausdorff=1.0) and post["adapt_mesh_deviation"] == dict(hausdorff=2.0)
    va, fa, vb, fb, dst, max_dist = seen[1]
    assert va is post["adapt_mesh_simplified"]["vertices"] and fa is post["adapt_mesh_simplified"]["faces"]      # the LAST mesh of the chain
    assert vb is post["adapt_mesh"]["vertices"] and fb is post["adapt_mesh"]["quads"] and (dst, max_dist) == (0.5, 9.0)
    seen.clear()
    post = reconstruct.scene_postpass(empty, 32, 26, 2, mesh_deviation=True, **kw)      # no chain: the extracted mesh against itself
    va, fa, vb, fb, dst, max_dist = seen[0]
    assert va is vb and fa is fb and (dst, max_dist) == (1.0, 60.0)      # (an empty scene has no lattice: resol 1)


# ---- the ABI: symbols are only added -----------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_version_script_and_binding():
    import ctypes
    import fnmatch
    import re
    from surfacenet_amd import _lib
    new = ("sn_mesh_distance", "sn_mesh_distance_dev")
    txt = open(os.path.join(ROOT, "include", "surfacenet_hip.h")).read()
    assert "#define SN_ABI_VERSION 2" in txt and "sn_mesh_distance_cfg" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    additions = re.search(r"Added since, without a version change.*?\*/", txt, flags=re.S).group(0)
    pattern = re.search(r"global:\s*([^;]+);", open(os.path.join(CSRC, "exports.map")).read()).group(1).strip()
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert re.search(r"\b%s\b" % name, additions), name
        assert fnmatch.fnmatchcase(name, pattern), (name, pattern)
        assert name in _lib.ABI_SYMBOLS, name
    assert "sn_meshdistance.hip" in open(os.path.join(CSRC, "Makefile")).read()
    assert ctypes.sizeof(_lib.MeshDistanceCfg) == 8


def test_the_rules_header_is_hip_free():
    with open(os.path.join(CSRC, "meshdistance_rules.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes and all("hip/" not in i and i in ("<stdint.h>", '"lattice.h"') for i in includes), includes


# ---- the rules and the argument checks of the C entry, on the CPU ------------------------------------------------------------------------------------
def test_rules_and_argument_checks_under_sanitizers(tmp_path):
    """tests/host/meshdistance_check.cpp runs csrc/meshdistance_rules.h - rule 1's branches, rule 2's regions, the degenerate kinds, the grid's
    arithmetic and the walks' bounds - and sn_host.h's mdi_check_args over every end of every range, compiled stand-alone with
    -fsanitize=address,undefined and run as a child process; the region cases at every scale and offset, the degenerate ones, the planted
    errors' cases and the random dyadic triangles go in as bits, and what comes back equals the restatement bit for bit."""
    rows = []
    for scale in ref.SCALES:
        for offset in ref.OFFSETS:
            v, f, pts, _ = ref.single_triangle(scale, offset)
            rows += [np.concatenate([p, v[0], v[1], v[2]]) for p in pts]
            rows += [r.reshape(-1) for r in ref.dyadic_triangles(40, scale, offset, seed=3)]
    for case in (ref.degenerate_mesh, ref.neg_zero_corner, ref.u_plus_e_case, ref.tie_case, ref.outside_case):
        v, f, pts = case()
        rows += [np.concatenate([p, v[t[0]], v[t[1]], v[t[2]]]) for t in f for p in pts]
    rows = np.asarray(rows, np.float64)
    P, A, B, C = (ref._xyz(rows[:, 3 * k:3 * k + 3]) for k in range(4))
    d2, c, degenerate = ref.triangle(P, A, B, C)
    assert degenerate.sum() > 20 and rows.shape[0] > 400
    exe = str(tmp_path / "meshdistance_check")
    _compile(os.path.join(ROOT, "tests", "host", "meshdistance_check.cpp"), exe)
    text = "".join(" ".join("%016x" % struct.unpack("<Q", struct.pack("<d", x))[0] for x in row) + "\n" for row in rows)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "MESHDISTANCE-CHECK-OK %d rows" % rows.shape[0] in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    got = [line.split() for line in p.stdout.splitlines()[:rows.shape[0]]]
    bits = lambda x: "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]
    for i, line in enumerate(got):
        assert line == [bits(d2[i]), bits(c[0][i]), bits(c[1][i]), bits(c[2][i]), "%d" % int(degenerate[i])], (i, rows[i].tolist())
