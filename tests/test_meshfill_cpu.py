"""CPU: the numpy restatement of the hole filler (tests/meshfill_ref.py) pinned on facts that can be checked by hand - the
loops of the sheets and sphere shells with faces taken out, the pinch, the fan, the opposed pair -; the argument checks of mesh.fill_holes and
reconstruct.scene_postpass, which run before the library is touched; the new symbols in header, version script, binding and library; and
mfl_check_args of csrc/sn_host.h compiled alone under the sanitizers and run as a child process."""
import os
import subprocess

import numpy as np
import pytest

import meshfill_ref as ref
import meshsmooth_ref as sm
from test_host_plumbing import CSRC, ROOT, _compile


def _loops(r):
    return [(lp["root"], lp["n"], lp["state"], lp["votes"]) for lp in r["loops"]]


def _signed_volume(v, tris):
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


# ---- the figures of the prototype ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sheet_q", "sheet_t"])
def test_whole_sheet_is_one_rim(name):
    r = ref.reference(name)
    assert _loops(r) == [(0, 32, ref.RIM, 0)] and r["zero_votes"] == 0
    assert r["counts"].tolist() == [144 if name == "sheet_q" else 208, 32, 1, 0, 0, 1, 0, 0]
    assert r["new_faces"].shape == (0, 3) and r["new_vert_lattice"].shape == (0, 3)
    assert sorted(set(r["vert_loop"].tolist())) == [ref.NONE, ref.RIM] and int((r["vert_loop"] == ref.RIM).sum()) == 32
    for key, dt in (("new_vertices", np.float32), ("new_vert_lattice", np.float64), ("loop_root", np.int32), ("loop_len", np.int32),
                    ("new_faces", np.int32), ("vert_loop", np.uint8), ("counts", np.int64)):
        assert r[key].dtype == dt, key


@pytest.mark.parametrize("name,E", [("sheet_hole_q", 140), ("sheet_hole_t", 200)])
def test_sheet_with_a_hole(name, E):
    v, f = ref.CASES[name]()
    assert v.shape == (81, 3) and f.shape == ((60, 4) if name.endswith("_q") else (120, 3))
    r = ref.reference(name, origin=(-20.0, -20.0, -20.0), resol=0.4)
    assert _loops(r) == [(0, 32, ref.RIM, 0), (30, 8, ref.FILLED, 8)] and r["zero_votes"] == 0
    assert r["counts"].tolist() == [E, 40, 2, 1, 0, 1, 0, 8]
    assert r["loop_root"].tolist() == [30] and r["loop_len"].tolist() == [8]
    assert r["new_vert_lattice"].tolist() == [[4.0, 4.0, 7.0]]                 # the centre of the sheet, z = 7.0 exactly
    assert r["new_vertices"].tolist() == [[np.float32(-20 + 0.4 * 4), np.float32(-20 + 0.4 * 4), np.float32(-20 + 0.4 * 7)]]
    ring = np.nonzero(r["vert_loop"] == ref.FILLED)[0]
    assert ring.tolist() == [30, 31, 32, 39, 41, 48, 49, 50]                   # the 3 x 3 block around vertex 40 without its centre
    t = r["new_faces"]
    assert t[:, 1].tolist() == ring.tolist() and (t[:, 2] == 81).all()        # ordered by p, all to the one new vertex
    assert sorted(t[:, 0].tolist()) == ring.tolist()                           # p -> r is one cycle through the ring
    # the cap closes the hole and keeps the orientation: the new triangles' normals point where the sheet's do
    vv, tris = ref.filled_mesh(v, f, r)
    n = np.cross(vv[t[:, 1]] - vv[t[:, 0]], vv[t[:, 2]] - vv[t[:, 0]])
    f0 = np.asarray(f[0])
    sheet_n = np.cross(v[f0[1]] - v[f0[0]], v[f0[2]] - v[f0[0]])
    assert (n[:, 2] * sheet_n[2] > 0).all() and (n[:, :2] == 0).all()
    again = sm.smooth(vv, tris, 0)
    assert again["counts"][1] == 32 and again["counts"][2] == 0                # only the rim is left


@pytest.mark.parametrize("name,n,root", [("sphere6_hole_q", 44, 59), ("sphere6_hole_t", 40, 59), ("sphere12_hole_q", 60, 654)])
def test_capped_sphere_is_closed_again(name, n, root):
    v, f = ref.CASES[name]()
    r = ref.reference(name)
    assert _loops(r) == [(root, n, ref.FILLED, n)] and r["zero_votes"] == 0   # all votes hole, none exactly 0
    assert r["counts"][1:].tolist() == [n, 1, 1, 0, 0, 0, n]
    vv, tris = ref.filled_mesh(v, f, r)
    closed = sm.smooth(vv, tris, 0)
    E, boundary, nonman, referenced = closed["counts"].tolist()
    assert boundary == 0 and nonman == 0
    assert referenced - E + tris.shape[0] == 2                                # Euler: a sphere
    assert _signed_volume(vv, tris) > 0
    whole_v, whole_f = sm.sphere_case(int(name[6:].split("_")[0]), name.endswith("_q"))
    assert 0.9 < _signed_volume(vv, tris) / _signed_volume(*ref.filled_mesh(whole_v, whole_f, ref.fill(whole_v, whole_f))) < 1.0      # a flat cap


def test_three_holes_interleave():
    v, f = ref.CASES["sphere12_holes3_q"]()
    r = ref.reference("sphere12_holes3_q")
    assert _loops(r) == [(31, 60, ref.FILLED, 60), (654, 60, ref.FILLED, 60), (868, 60, ref.FILLED, 60)]
    third = r["new_faces"][:, 2] - v.shape[0]
    assert sorted(set(third.tolist())) == [0, 1, 2] and (np.diff(third) != 0).sum() > 2       # the ranks are not three runs
    vv, tris = ref.filled_mesh(v, f, r)
    assert sm.smooth(vv, tris, 0)["counts"][1] == 0


@pytest.mark.parametrize("name", ["single_q", "single_t"])
def test_single_face_is_a_rim_and_any_caps_it(name):
    v, f = ref.CASES[name]()
    n = f.shape[1]
    r = ref.reference(name)
    assert _loops(r) == [(0, n, ref.RIM, 0)] and r["counts"].tolist() == [n, n, 1, 0, 0, 1, 0, 0]
    a = ref.reference(name, 64, ref.ANY)
    assert _loops(a) == [(0, n, ref.FILLED, None)] and a["counts"].tolist() == [n, n, 1, 1, 0, 0, 0, n]
    vv, tris = ref.filled_mesh(v, f, a)
    assert sm.smooth(vv, tris, 0)["counts"][1] == 0
    assert a["new_vert_lattice"].tolist() == ([[6.5, 6.0, 5.0]] if n == 4 else [[480597 / 65536, 349525 / 65536, 5.0]])
    # (the triangle: x = 22/3 cells, floor((2 * 22 * 65536 + 3) / 6) = 480597; y = 16/3, floor((2 * 16 * 65536 + 3) / 6) = 349525)


def test_pinch_fan_and_opposed_pair_are_complex():
    p = ref.reference("pinch")                                  # two one-cell holes that share vertex (3, 3) = 24: one component of 8 half-edges
    assert _loops(p) == [(0, 24, ref.RIM, 0), (16, 8, ref.COMPLEX, None)] and p["counts"].tolist() == [84, 32, 2, 0, 0, 1, 1, 0]
    assert np.nonzero(p["vert_loop"] == ref.COMPLEX)[0].tolist() == [16, 17, 23, 24, 25, 31, 32]
    assert ref.reference("pinch", 64, ref.ANY)["loop_root"].tolist() == [0]    # "any" caps the rim, the pinched pair still not
    t = ref.reference("two_holes")                              # apart, each is a hole of four edges
    assert _loops(t) == [(0, 24, ref.RIM, 0), (8, 4, ref.FILLED, 4), (25, 4, ref.FILLED, 4)]
    assert t["new_vert_lattice"].tolist() == [[3.5, 3.5, 3.0], [6.5, 5.5, 3.0]] and t["counts"].tolist() == [84, 32, 3, 2, 0, 1, 0, 8]
    fan = ref.reference("fan3", 64, ref.ANY)                    # three faces on one edge: its ends are not simple
    assert _loops(fan) == [(0, 6, ref.COMPLEX, None)] and fan["counts"].tolist() == [7, 6, 1, 0, 0, 0, 1, 0]
    assert (fan["vert_loop"] == ref.COMPLEX).all()
    opp = ref.reference("opposed", 64, ref.ANY)                 # two faces that both run 0 -> 1: out = 2 at vertex 1, in = 2 at vertex 0
    assert _loops(opp) == [(0, 4, ref.COMPLEX, None)] and opp["counts"].tolist() == [5, 4, 1, 0, 0, 0, 1, 0]


def test_max_len_decides_at_n():
    for name, n in (("sheet_hole_q", 8), ("sphere6_hole_q", 44)):
        short = ref.reference(name, n - 1)
        assert short["counts"][3] == 0 and short["counts"][4] >= 1 and int((short["vert_loop"] == ref.LONG).sum()) >= n
        assert [lp["state"] for lp in short["loops"] if lp["n"] == n] == [ref.LONG]
        assert ref.reference(name, n)["counts"][3] == 1
    ann = ref.reference("annulus4096", 4096)
    assert _loops(ann) == [(0, 4096, ref.FILLED, 4096), (4096, 4096, ref.RIM, 0)] and ann["zero_votes"] == 0
    assert ann["new_vert_lattice"][0, 2] == 9.0 and ann["new_faces"].shape == (4096, 3)
    assert _loops(ref.reference("annulus4096", 4095)) == [(0, 4096, ref.LONG, None), (4096, 4096, ref.LONG, None)]


# ---- rule 13 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sheet_hole_t", "sphere6_hole_q", "sphere12_holes3_q", "two_holes"])
def test_face_order_translation_and_second_call(name):
    v, f = ref.CASES[name]()
    r = ref.reference(name)
    p = ref.fill(v, f[np.random.default_rng(7).permutation(f.shape[0])])
    for key in ref.KEYS:
        assert np.array_equal(p[key], r[key]), key
    shift = np.asarray([3.0, -2.0, 11.0])
    t = ref.fill(v + shift, f)
    assert np.array_equal(t["new_vert_lattice"], r["new_vert_lattice"] + shift)
    for key in ("loop_root", "loop_len", "new_faces", "vert_loop", "counts"):
        assert np.array_equal(t[key], r[key]), key
    vv, tris = ref.filled_mesh(v, f, r)
    second = ref.fill(vv, tris)
    assert second["counts"][3] == 0 and second["counts"][7] == 0
    assert not second["vert_loop"][:v.shape[0]][r["vert_loop"] == ref.FILLED].any()        # the filled loops' vertices are interior now


def test_closed_and_empty():
    for name in ("sphere6_q", "sphere6_t"):
        r = ref.reference(name)
        assert r["counts"][1:].tolist() == [0] * 7 and not r["vert_loop"].any() and r["loops"] == []
    v, f = sm.rules_case()
    e = ref.fill(v, f[:0])
    assert e["counts"].tolist() == [0] * 8 and e["vert_loop"].shape == (8,) and not e["vert_loop"].any() and e["new_faces"].shape == (0, 3)
    rules = ref.fill(v, f)                                      # the smoother's rule case: the doubled face and the degenerate side count as there
    assert rules["counts"][:2].tolist() == [10, 5]


def test_restatement_errors():
    v, f = ref.CASES["sheet_hole_t"]()
    for bad in (2, 65537, 0, -1, 2.5, True):
        with pytest.raises(ValueError, match="max_len"):
            ref.fill(v, f, bad)
    for bad in (2, -1, "holes"):
        with pytest.raises(ValueError, match="orientation"):
            ref.fill(v, f, 64, bad)
    g = f.copy()
    g[5, 1] = 81
    with pytest.raises(ValueError, match="face 5 "):
        ref.fill(v, g)
    far = v.copy()
    far[f[7, 0], 1] = np.nan
    first = int(np.nonzero((f == f[7, 0]).any(axis=1))[0][0])
    with pytest.raises(ValueError, match="face %d:" % first):
        ref.fill(far, f)
    with pytest.raises(ValueError, match="resol"):
        ref.fill(v, f, resol=0.0)
    with pytest.raises(ValueError, match="origin"):
        ref.fill(v, f, origin=(0.0, np.inf, 0.0))
    with pytest.raises(ValueError, match="nv"):
        ref.fill(v, np.zeros((2, 5), np.int32))
    assert ref.fill(v, f, 3)["counts"][4] == 2 and ref.fill(v, f, 65536)["counts"][3] == 1


# ---- surfacenet_amd/mesh.py and reconstruct.py: host code ------------------------------------------------------------------------------------------
def _no_library(monkeypatch):
    from surfacenet_amd import runtime

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(runtime, "any_context", no_library)


def test_fill_holes_checks_its_arguments_before_the_library(monkeypatch):
    from surfacenet_amd import mesh
    _no_library(monkeypatch)
    v, f = ref.CASES["sheet_hole_t"]()
    assert mesh.check_fill_args(64, "holes") == (64, 0) and mesh.check_fill_args(3, "any") == (3, 1) and mesh.check_fill_args(65536, "holes") == (65536, 0)
    assert mesh.check_fill_args(np.int64(16), "any") == (16, 1)
    with pytest.raises(AssertionError, match="library was touched"):
        mesh.fill_holes(v, f)                                   # well-formed arguments get as far as the library
    with pytest.raises(AssertionError, match="library was touched"):
        mesh.fill_holes(v.astype(np.float32), np.asarray([[0, 1, 10, 9]]), max_len=3, orientation="any", origin=(1, 2, 3), resol=0.4,
                        vert_src=np.arange(81), triangulate=False)
    for bad in (2, 65537, 0, -5, 2.5, "3", None, True):
        with pytest.raises(ValueError, match="max_len"):
            mesh.fill_holes(v, f, max_len=bad)
        with pytest.raises(ValueError, match="max_len"):
            mesh.check_fill_args(bad, "holes")
    for bad in (0, 1, "rims", None, True):
        with pytest.raises(ValueError, match="orientation"):
            mesh.fill_holes(v, f, orientation=bad)
    g = f.copy()
    g[4, 1] = 81
    with pytest.raises(ValueError, match="face 4 "):
        mesh.fill_holes(v, g)
    g[2, 2] = -1
    with pytest.raises(ValueError, match="face 2 "):
        mesh.fill_holes(v, g)
    first = int(np.nonzero((f == 3).any(axis=1))[0][0])
    for value in (np.nan, np.inf, 2097144.0, np.nextafter(-4.0, -5)):
        far = v.copy()
        far[3, 1] = value
        with pytest.raises(ValueError, match="face %d:" % first):
            mesh.fill_holes(far, f)
    for resol in (0.0, -0.4, np.inf, np.nan, "x"):
        with pytest.raises(ValueError, match="resol"):
            mesh.fill_holes(v, f, resol=resol)
    for origin in ((0.0, np.nan, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0), "abc"):
        with pytest.raises(ValueError, match="origin"):
            mesh.fill_holes(v, f, origin=origin)
    with pytest.raises(ValueError, match="vert_src"):
        mesh.fill_holes(v, f, vert_src=np.arange(80))
    many = (1 << 28) + 1                                        # V and F over the limit: broadcast views, no memory behind them
    with pytest.raises(ValueError, match="2\\^28"):
        mesh.fill_holes(np.broadcast_to(np.zeros((1, 3), np.float32), (many, 3)), f)
    with pytest.raises(ValueError, match="2\\^28"):
        mesh.fill_holes(v, np.broadcast_to(np.zeros((1, 3), np.int32), (many, 3)))
    for args in ((v[:, :2], f), (np.zeros((8, 3), np.int64), f), (v, f[:, :2]), (v, np.zeros((2, 5), np.int32)), (v, f.astype(np.float64)), (v.reshape(-1), f)):
        with pytest.raises(ValueError):
            mesh.fill_holes(*args)
    e = mesh.fill_holes(v, np.zeros((0, 4), np.int32), origin=(1.0, 2.0, 3.0), resol=0.5, vert_src=np.arange(81))      # no face: without the library
    assert set(e) == {"vertices", "vert_lattice", "faces", "loop_root", "loop_len", "vert_loop", "vert_src"} | set(mesh.FILL_COUNTS)
    assert e["vertices"].shape == (81, 3) and e["vertices"].dtype == np.float32 and e["faces"].shape == (0, 3) and e["n_filled"] == 0
    assert np.array_equal(e["vertices"], (np.asarray([1.0, 2.0, 3.0]) + 0.5 * v).astype(np.float32)) and not e["vert_loop"].any()
    assert mesh.FILL_COUNTS == ref.COUNT_NAMES


def test_scene_postpass_checks_mesh_fill_before_any_stage(monkeypatch):
    from surfacenet_amd import reconstruct
    _no_library(monkeypatch)
    empty = dict(prediction_list=[], vxl_ijk_list=[], rayPooling_votes_list=[], cube_ijk_np=np.zeros((0, 3), np.int64))
    cams = np.zeros((2, 3))
    with pytest.raises(ValueError, match="mesh=True"):
        reconstruct.scene_postpass(empty, 32, 26, 2, mesh_fill=64)
    with pytest.raises(ValueError, match="mesh=True"):
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh_fill=dict(max_len=16))
    for bad in (2, 65537, 2.5, "64"):
        with pytest.raises(ValueError, match="max_len"):
            reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_fill=bad)
    with pytest.raises(ValueError, match="orientation"):
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_fill=dict(max_len=16, orientation="rims"))
    with pytest.raises(ValueError, match="mesh_fill"):
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_fill=dict(max_len=16, iterations=4))
    plain = reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True)
    post = reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_fill=dict(max_len=16, orientation="any"))
    assert set(post) - set(plain) == {"fixThresh_mesh_filled", "adapt_mesh_filled"}
    assert post["adapt_mesh_filled"]["faces"].shape == (0, 3) and post["adapt_mesh_filled"]["n_filled"] == 0
    all3 = reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_fill=64, mesh_smooth=2, mesh_cell=2)
    assert set(all3) - set(plain) == {"fixThresh_mesh_filled", "adapt_mesh_filled", "fixThresh_mesh_smoothed", "adapt_mesh_smoothed",
                                      "fixThresh_mesh_simplified", "adapt_mesh_simplified"}
    assert all3["adapt_mesh_smoothed"]["faces"].shape == (0, 3) and "quads" not in all3["adapt_mesh_smoothed"]


# ---- the ABI: symbols are only added ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_version_script_binding_and_library():
    import fnmatch
    import re
    import __graft_entry__ as g
    g.build()
    from surfacenet_amd import _lib
    new = ("sn_mesh_fill", "sn_mesh_fill_dev")
    txt = open(os.path.join(ROOT, "include", "surfacenet_hip.h")).read()
    assert "#define SN_ABI_VERSION 2" in txt and "sn_mesh_fill_cfg" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    pattern = re.search(r"global:\s*([^;]+);", open(os.path.join(CSRC, "exports.map")).read()).group(1).strip()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode().split()
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert fnmatch.fnmatchcase(name, pattern), (name, pattern)
        assert name in _lib.ABI_SYMBOLS and name in exported, name
    lib = _lib.load()
    assert lib.sn_version() == 2 and all(hasattr(lib, name) for name in new)
    assert "sn_meshfill.hip" in open(os.path.join(CSRC, "Makefile")).read()
    import ctypes
    assert ctypes.sizeof(_lib.MeshFillCfg) == 40                # int, int, double[3], double


# ---- the argument checks of the C entry, on the CPU ------------------------------------------------------------------------------------------------
def test_argument_checks_under_sanitizers(tmp_path):
    """tests/host/meshfill_check.cpp runs sn_host.h's mfl_check_args over every end of every range and rule 5's centroid at the ends of its range,
    compiled stand-alone with -fsanitize=address,undefined and run as a child process."""
    exe = str(tmp_path / "meshfill_check")
    _compile(os.path.join(ROOT, "tests", "host", "meshfill_check.cpp"), exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "MESHFILL-CHECK-OK" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
