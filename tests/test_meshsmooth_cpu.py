"""CPU: the numpy restatement of the mesh smoother (tests/meshsmooth_ref.py) pinned on hand-made cases and on the
mesher's own meshes; the argument checks of mesh.smooth_mesh and reconstruct.scene_postpass, which run before the library is touched; and the
rounding helper of the device code (csrc/meshsmooth_round.h) compiled alone under the sanitizers and run as a child process."""
import os
import subprocess

import numpy as np
import pytest

import mesh_ref as mr
import meshsimplify_ref as sref
import meshsmooth_ref as ref
from test_host_plumbing import CSRC, ROOT, _compile

LAM, MU = ref.q16(0.5), ref.q16(-0.53)


# ---- the sheet -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quads,E", [(True, 144), (False, 208)])
def test_sheet(quads, E):
    v, f = ref.sheet_case(quads)
    assert v.shape == (81, 3) and f.shape == ((64, 4) if quads else (128, 3))
    name = "sheet_q" if quads else "sheet_t"
    r = ref.reference(name, 5, LAM, MU, ref.FIXED)
    assert r["counts"].tolist() == [E, 32, 0, 81]
    assert int((r["vert_flags"] & ref.BOUNDARY).astype(bool).sum()) == 32 and (r["vert_flags"] & ref.REFERENCED).all()
    assert np.array_equal(r["q"], r["q0"])                     # a flat regular sheet with its rim fixed does not move at all
    assert np.array_equal(r["vert_lattice"], v) and np.array_equal(r["vertices"], v.astype(np.float32))
    for mode in (ref.CURVE, ref.FREE):
        m = ref.reference(name, 5, LAM, MU, mode)
        assert (m["q"] != m["q0"]).any() and (m["q"][:, 2] == 7 * 65536).all()      # it moves, and stays in its plane exactly
        assert m["counts"].tolist() == r["counts"].tolist() and np.array_equal(m["vert_degree"], r["vert_degree"])
    # mode 1: the rim is a curve - an edge's inner vertices keep their line, a corner moves along the diagonal; mode 2 pulls the rim inwards
    one = ref.smooth(v, f, 1, LAM, 0, ref.CURVE)
    assert np.array_equal(one["q"][4], one["q0"][4]) and one["q"][0].tolist() == [16384, 16384, 7 * 65536]
    free = ref.smooth(v, f, 1, LAM, 0, ref.FREE)
    assert free["q"][4, 0] > free["q0"][4, 0] and (free["q"][4, 1] == free["q0"][4, 1]) == quads      # (a triangle's diagonal pulls sideways too)
    for key, dt in (("vertices", np.float32), ("vert_lattice", np.float64), ("vert_degree", np.int32), ("vert_flags", np.uint8), ("counts", np.int64)):
        assert r[key].dtype == dt, key


# ---- exactness -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sheet_t", "sphere6_q", "surface"])
def test_translation_and_face_permutation_commute_exactly(name):
    v, f = ref.CASES[name]()
    r = ref.reference(name, 10, LAM, MU, ref.CURVE)
    t = ref.smooth(v + np.asarray([3.0, -2.0, 11.0]), f, 10, LAM, MU, ref.CURVE)
    assert np.array_equal(t["q"], r["q"] + np.asarray([3, -2, 11]) * 65536)
    assert np.array_equal(t["vert_lattice"], r["vert_lattice"] + np.asarray([3.0, -2.0, 11.0]))
    p = ref.smooth(v, f[np.random.default_rng(5).permutation(f.shape[0])], 10, LAM, MU, ref.CURVE)
    for key in ref.KEYS:
        assert np.array_equal(p[key], r[key]), key


# ---- sphere shells: Taubin keeps the volume, Laplace does not -------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,V,E", [(6, 728, 1452), (9, 1496, 2988)])
def test_sphere_shells(R, V, E):
    name = "sphere%d_q" % R
    v, f = ref.CASES[name]()
    r0 = ref.reference(name, 0, LAM, MU, ref.FREE)
    assert v.shape == (V, 3) and r0["counts"].tolist() == [E, 0, 0, V] and r0["vert_degree"].max() <= 6
    assert not (r0["vert_flags"] & (ref.BOUNDARY | ref.NONMANIFOLD)).any()
    assert np.array_equal(r0["edges"], mr.edge_counts(f)[0]) and np.array_equal(r0["edge_count"], mr.edge_counts(f)[1])
    vol0, rough0 = mr.signed_volume(r0["vert_lattice"], f), ref.roughness(r0["q0"], r0["edges"])
    ratios = {}
    for it, mu in ((10, MU), (20, MU), (10, 0)):
        r = ref.reference(name, it, LAM, mu, ref.FREE)
        ratios[(it, mu)] = mr.signed_volume(r["vert_lattice"], f) / vol0
        assert r["counts"].tolist() == r0["counts"].tolist()
    rough = ref.roughness(ref.reference(name, 10, LAM, MU, ref.FREE)["q"], r0["edges"])
    print("R = %d: volume ratios %r, roughness %.3f -> %.3f" % (R, ratios, rough0, rough))
    assert 0.98 <= ratios[(10, MU)] <= 1.02
    assert 0.98 <= ratios[(20, MU)] <= 1.02
    assert ratios[(10, 0)] < 0.95
    assert rough < 0.5 * rough0


# ---- the surface scene and its simplification: open boundary, a non-manifold edge -----------------------------------------------------------------
def test_surface_scene():
    v, f = ref.surface_case()
    r = ref.reference("surface", 0)
    assert v.shape == (2398, 3) and r["counts"].tolist() == [6998, 196, 0, 2398]
    e, n = sref.tri_edge_counts(f)
    assert np.array_equal(r["edges"], e) and np.array_equal(r["edge_count"], n)
    assert int((r["vert_flags"] & ref.BOUNDARY).astype(bool).sum()) == np.unique(e[n == 1]).size and not (r["vert_flags"] & ref.NONMANIFOLD).any()
    vs, fs = ref.surface_simplified_case(2)
    s = ref.reference("surface_k2", 0)
    assert vs.shape == (646, 3) and s["counts"].tolist() == [1837, 103, 1, 646] and s["vert_degree"].max() == 11
    e, n = sref.tri_edge_counts(fs)
    assert np.array_equal(np.nonzero(s["vert_flags"] & ref.NONMANIFOLD)[0], np.sort(e[n > 2].reshape(-1)))
    assert np.array_equal((s["vert_flags"] & ref.BOUNDARY) != 0, np.isin(np.arange(646), e[n == 1]))
    assert np.array_equal(s["vert_degree"], np.bincount(e.reshape(-1), minlength=646))
    m = ref.reference("surface_k2", 10)                         # curve mode: the rim stays a rim, nothing leaves the range
    assert (m["q"] != m["q0"]).any() and m["q"].min() >= ref.QMIN


# ---- hand-made rule cases --------------------------------------------------------------------------------------------------------------------------
def test_rules_case_by_hand():
    v, f = ref.rules_case()
    r = ref.smooth(v, f, 0)
    # edges (a < b) and their counts: faces 0 and 1 are the same face (count 2 from them alone); face 2 = (2, 4, 4) gives (2,4) twice and no (4,4)
    assert r["edges"].tolist() == [[0, 1], [0, 2], [0, 5], [1, 2], [1, 3], [1, 5], [1, 6], [2, 3], [2, 4], [3, 6]]
    assert r["edge_count"].tolist() == [3, 2, 1, 3, 2, 1, 1, 1, 2, 1]
    assert r["counts"].tolist() == [10, 5, 2, 7]
    assert r["vert_degree"].tolist() == [3, 5, 4, 3, 1, 2, 2, 0] and r["bdegree"].tolist() == [1, 2, 1, 2, 0, 2, 2, 0]
    assert r["vert_flags"].tolist() == [7, 7, 7, 3, 1, 3, 3, 0]
    # iterations = 0 quantises: the two ends of the range are legal, the unreferenced vertex passes through bit for bit. The last double below
    # 2^21 - 8 lies 2^-32 under it, and rule 2 rounds it to QMAX + 1: quantising does not clamp, only a pass does (limits)
    assert r["q"][5].tolist() == [ref.QMIN] * 3 and v[6, 0] < ref.HI and r["q"][6, 0] == ref.QMAX + 1 and r["vert_lattice"][6, 0] == ref.HI
    assert ref.smooth(np.where(v == v[6, 0], ref.HI - 2.0 ** -16, v), f, 0)["q"][6, 0] == ref.QMAX
    assert r["vert_lattice"][7].tobytes() == v[7].tobytes() and np.isnan(r["vertices"][7, 0])
    assert np.array_equal(r["vert_lattice"][:6], v[:6]) and np.array_equal(r["vert_lattice"][6, 1:], v[6, 1:])
    for mode in (ref.FIXED, ref.CURVE, ref.FREE):
        m = ref.smooth(v, f, 3, LAM, MU, mode)
        assert m["vert_lattice"][7].tobytes() == v[7].tobytes() and m["q"].min() >= ref.QMIN and m["q"].max() <= ref.QMAX + (mode == ref.FIXED)
        assert (m["q"][4] != m["q0"][4]).any()               # vertex 4: its one edge (2,4) has count 2, so it is interior and moves in every mode
    # one pass by hand, free: vertex 4's only neighbour is 2, vertex 0 gathers 1, 2 and 5
    one = ref.smooth(v, f, 1, LAM, 0, ref.FREE)
    assert np.array_equal(one["q"][4], one["q0"][4] + ((LAM * (one["q0"][2] - one["q0"][4]) + 32768) >> 16))
    S = one["q0"][[1, 2, 5]].sum(axis=0)
    mean = (2 * S + 3) // 6
    assert np.array_equal(one["q"][0], one["q0"][0] + ((LAM * (mean - one["q0"][0]) + 32768) >> 16))
    # curve: vertex 0 is a boundary vertex whose one boundary edge leads to 5; vertex 3's lead to 2 and 6
    curve = ref.smooth(v, f, 1, LAM, 0, ref.CURVE)
    assert np.array_equal(curve["q"][0], curve["q0"][0] + ((LAM * (curve["q0"][5] - curve["q0"][0]) + 32768) >> 16))
    S = curve["q0"][[2, 6]].sum(axis=0)
    assert np.array_equal(curve["q"][3], curve["q0"][3] + ((LAM * ((2 * S + 2) // 4 - curve["q0"][3]) + 32768) >> 16))
    fixed = ref.smooth(v, f, 1, LAM, 0, ref.FIXED)
    assert np.array_equal(fixed["q"][[0, 1, 2, 3, 5, 6]], fixed["q0"][[0, 1, 2, 3, 5, 6]]) and (fixed["q"][4] != fixed["q0"][4]).any()


def test_the_clamp_stops_a_runaway_vertex():
    v, f = ref.clamp_case()
    r = ref.smooth(v, f, 60, -65536, -65536, ref.FREE)
    assert r["q"].min() == ref.QMIN and r["q"].max() == ref.QMAX
    assert ((r["q"] == ref.QMIN) | (r["q"] == ref.QMAX)).all()
    assert r["vert_lattice"].min() == -4.0 and r["vert_lattice"].max() == float(ref.QMAX) / 65536 < 2097144.0
    sref.simplify(r["vert_lattice"], f, 2)                      # ... a valid input of the simplifier still
    one = ref.smooth(v, f, 1, -65536, 0, ref.FREE)              # one pass by hand: vertex 1 gathers 0, 2, 3 and 4; w = -1 mirrors it at their mean
    free = 2 * one["q0"][1] - (2 * one["q0"][[0, 2, 3, 4]].sum(axis=0) + 4) // 8
    assert free[1] < ref.QMIN <= free[0] and one["q"][1].tolist() == [free[0], ref.QMIN, free[2]]


def test_fans_and_soup_are_what_the_gpu_tests_say():
    for n in (300, 5000):
        r = ref.reference("fan%d" % n, 0)
        assert r["vert_degree"][0] == n and (r["vert_degree"][1:] == 3).all() and r["counts"].tolist() == [2 * n, n, 0, n + 1]
    s = ref.reference("soup", 0)
    v, f = ref.soup_case()
    assert s["counts"][3] == np.unique(f).size < 5000 and (f[:, 0] == f[:, 1]).any() and s["edge_count"].max() >= 2
    assert s["counts"][0] < 3 * 20000 - int((f[:, 0] == f[:, 1]).sum())


# ---- the restatement's own errors ------------------------------------------------------------------------------------------------------------------
def test_restatement_errors():
    v, f = ref.rules_case()
    bad = f.copy()
    bad[4, 1] = 8
    bad[5, 0] = -1
    with pytest.raises(ValueError, match="face 4 "):
        ref.smooth(v, bad, 1)
    for value in (np.nan, np.inf, 2097144.0, np.nextafter(-4.0, -5.0)):
        far = v.copy()
        far[3, 1] = value
        with pytest.raises(ValueError, match="face 3:"):
            ref.smooth(far, f, 1)
    with pytest.raises(ValueError, match="face 2 "):            # an index error at a smaller face wins over a range error
        far = v.copy()
        far[3, 1] = np.nan
        b2 = f.copy()
        b2[2, 0] = 99
        ref.smooth(far, b2, 1)
    for kw in (dict(iterations=-1), dict(iterations=1001), dict(iterations=2.5), dict(lam_q16=65537), dict(lam_q16=-65537), dict(mu_q16=65537),
               dict(mu_q16=-65537), dict(boundary=3), dict(boundary=-1), dict(resol=0.0), dict(resol=np.inf), dict(resol=np.nan),
               dict(origin=(0.0, np.nan, 0.0)), dict(origin=(np.inf, 0.0, 0.0))):
        with pytest.raises(ValueError):
            ref.smooth(v, f, **kw)
    with pytest.raises(ValueError, match="nv"):
        ref.smooth(v, np.zeros((2, 5), np.int32), 1)
    many = (1 << 28) + 1
    with pytest.raises(ValueError, match="2\\^28"):
        ref.smooth(np.broadcast_to(np.zeros((1, 3)), (many, 3)), f, 1)
    with pytest.raises(ValueError, match="2\\^28"):
        ref.smooth(v, np.broadcast_to(np.zeros((1, 3), np.int32), (many, 3)), 1)
    ref.smooth(v, f, 1000, 65536, -65536, 2)                    # the ends of every range are legal
    e = ref.smooth(v, f[:0], 5)                                 # F = 0: nothing is referenced
    assert e["counts"].tolist() == [0, 0, 0, 0] and e["vert_lattice"].tobytes() == v.tobytes() and not e["vert_flags"].any()


# ---- surfacenet_amd/mesh.py and reconstruct.py: host code ------------------------------------------------------------------------------------------
def _no_library(monkeypatch):
    from surfacenet_amd import runtime

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(runtime, "any_context", no_library)


def test_smooth_mesh_checks_its_arguments_before_the_library(monkeypatch):
    from surfacenet_amd import mesh
    _no_library(monkeypatch)
    v, f = ref.rules_case()
    assert mesh.check_smooth_args(10, 0.5, -0.53, "curve") == (10, 32768, -34734, 1)
    assert mesh.check_smooth_args(0, 1, -1.0, "free") == (0, 65536, -65536, 2) and mesh.check_smooth_args(1000, 0.0, 0, "fixed")[1:] == (0, 0, 0)
    with pytest.raises(AssertionError, match="library was touched"):
        mesh.smooth_mesh(v, f)                                  # well-formed arguments get as far as the library
    with pytest.raises(AssertionError, match="library was touched"):
        mesh.smooth_mesh(v.astype(np.float32), np.asarray([[0, 1, 3, 2]]), iterations=0, lam=1.0, mu=0.0, boundary="fixed", origin=(1, 2, 3), resol=0.4)
    bad = f.copy()
    bad[4, 1] = 8
    with pytest.raises(ValueError, match="face 4 "):
        mesh.smooth_mesh(v, bad)
    bad[2, 2] = -1
    with pytest.raises(ValueError, match="face 2 "):
        mesh.smooth_mesh(v, bad)
    for value in (np.nan, np.inf, 2097144.0, np.nextafter(-4.0, -5)):
        far = v.copy()
        far[3, 1] = value
        with pytest.raises(ValueError, match="face 3:"):
            mesh.smooth_mesh(far, f)
    for it in (-1, 1001, 2.5, "3", None, True):
        with pytest.raises(ValueError, match="iterations"):
            mesh.smooth_mesh(v, f, iterations=it)
    for x in (1.5, -1.0001, np.nan, np.inf, "a", None):
        with pytest.raises(ValueError, match="lam"):
            mesh.smooth_mesh(v, f, lam=x)
        with pytest.raises(ValueError, match="mu"):
            mesh.smooth_mesh(v, f, mu=x)
    for b in (0, 1, "rim", None):
        with pytest.raises(ValueError, match="boundary"):
            mesh.smooth_mesh(v, f, boundary=b)
    for resol in (0.0, -0.4, np.inf, np.nan, "x"):
        with pytest.raises(ValueError, match="resol"):
            mesh.smooth_mesh(v, f, resol=resol)
    for origin in ((0.0, np.nan, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0), "abc"):
        with pytest.raises(ValueError, match="origin"):
            mesh.smooth_mesh(v, f, origin=origin)
    many = (1 << 28) + 1                                        # V and F over the limit: broadcast views, no memory behind them
    with pytest.raises(ValueError, match="2\\^28"):
        mesh.smooth_mesh(np.broadcast_to(np.zeros((1, 3), np.float32), (many, 3)), f)
    with pytest.raises(ValueError, match="2\\^28"):
        mesh.smooth_mesh(v, np.broadcast_to(np.zeros((1, 3), np.int32), (many, 3)))
    for args in ((v[:, :2], f), (np.zeros((8, 3), np.int64), f), (v, f[:, :2]), (v, np.zeros((2, 5), np.int32)), (v, f.astype(np.float64)), (v.reshape(-1), f)):
        with pytest.raises(ValueError):
            mesh.smooth_mesh(*args)
    e = mesh.smooth_mesh(np.zeros((0, 3)), np.zeros((0, 4), np.int32))      # no vertex: the empty result without the library
    assert set(e) == {"vertices", "vert_lattice", "vert_degree", "vert_flags", "n_edges", "n_boundary_edges", "n_nonmanifold_edges", "n_referenced"}
    assert e["vertices"].shape == (0, 3) and e["vert_flags"].dtype == np.uint8 and e["n_edges"] == 0


def test_scene_postpass_checks_mesh_smooth_before_any_stage(monkeypatch):
    from surfacenet_amd import reconstruct
    _no_library(monkeypatch)
    empty = dict(prediction_list=[], vxl_ijk_list=[], rayPooling_votes_list=[], cube_ijk_np=np.zeros((0, 3), np.int64))
    cams = np.zeros((2, 3))
    with pytest.raises(ValueError, match="mesh=True"):
        reconstruct.scene_postpass(empty, 32, 26, 2, mesh_smooth=3)
    with pytest.raises(ValueError, match="mesh=True"):
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh_smooth=dict(iterations=3))
    for it in (-1, 1001, 2.5, "2"):
        with pytest.raises(ValueError, match="iterations"):
            reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_smooth=it)
    with pytest.raises(ValueError, match="boundary"):
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_smooth=dict(iterations=2, boundary="rim"))
    with pytest.raises(ValueError, match="lam"):
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_smooth=dict(lam=2.0))
    with pytest.raises(ValueError, match="mesh_smooth"):
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_smooth=dict(iterations=2, cell=4))
    plain = reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True)
    post = reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_smooth=dict(iterations=4, mu=0.0, boundary="free"))
    assert set(post) - set(plain) == {"fixThresh_mesh_smoothed", "adapt_mesh_smoothed"}
    assert post["adapt_mesh_smoothed"]["quads"].shape == (0, 4) and post["adapt_mesh_smoothed"]["n_edges"] == 0
    both = reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_smooth=2, mesh_cell=2)
    assert set(both) - set(plain) == {"fixThresh_mesh_smoothed", "adapt_mesh_smoothed", "fixThresh_mesh_simplified", "adapt_mesh_simplified"}


# ---- the rounding helper of the device code, on the CPU --------------------------------------------------------------------------------------------
def test_rounding_helper_is_hip_free_and_checks_under_sanitizers(tmp_path):
    """csrc/meshsmooth_round.h includes no HIP header; tests/host/meshsmooth_check.cpp compares its floor division, mean, shifted product and
    clamped step with a hand-made table and runs sn_host.h's msm_check_args over every end of every range, compiled stand-alone with
    -fsanitize=address,undefined and run as a child process."""
    with open(os.path.join(CSRC, "meshsmooth_round.h")) as fh:
        includes = [line.split()[1] for line in fh if line.startswith("#include")]
    assert includes and all(i[0] == "<" and "hip/" not in i for i in includes), includes
    exe = str(tmp_path / "meshsmooth_check")
    _compile(os.path.join(ROOT, "tests", "host", "meshsmooth_check.cpp"), exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "MESHSMOOTH-CHECK-OK" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
