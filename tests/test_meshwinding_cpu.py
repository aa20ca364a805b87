"""CPU: the winding-number stage's contract as tests/meshwinding_ref.py restates it - against the analytic inside / on
/ outside of two solids, the properties of rule 8, nested, overlapping and open meshes, the planted errors -, mesh.winding_number and
mesh.signed_distance on a stand-in context that is the restatement, the wiring of the new symbols, and the rules header under the sanitizers
(tests/host/meshwinding_check.cpp). No GPU and no library.

The issue states the solids about the origin (the cube 0 .. 4, the octahedron of radius 4, queries in [-5, 5]^3) and the range of a query's
coordinates as [-4, 2^21 - 8): the cases stand ref.SHIFT = 8 whole cells up every axis, which rule 8 - tested below - says changes nothing."""
import os
import subprocess

import numpy as np
import pytest

import mesh_refusals as bad
import meshdistance_ref as md
import meshrender_ref as rr
import meshwinding_ref as ref
from test_host_plumbing import CSRC, ROOT, _compile

AXES = (0, 1, 2)


def _same(a, b, keys=ref.KEYS):
    return ref.same_bytes(a, b, keys) == []


def _closed_and_consistent(tri):
    """Every directed edge once, and its reverse once: a closed mesh whose faces turn one way."""
    e = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    fwd = {(int(a), int(b)) for a, b in e}
    return len(fwd) == len(e) and all((b, a) in fwd for a, b in fwd)


def _sphere():
    v, f = rr.sphere(6)
    return np.rint((v * 4.5 + ref.SHIFT) * ref.FIX) / ref.FIX, f      # (on the fixed-point grid: a translation by whole cells is exact)


# ---- the restatement on the solids -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,where", [("cube", ref.cube_where), ("octahedron", ref.octahedron_where)])
def test_the_solids_against_the_analytic_answer(name, where):
    v, f, pts = ref.CASES[name]()
    assert pts.shape == (2 * 1331, 3) and np.array_equal(pts[1331:], pts[:1331] + ref.OFFSET)
    inside, on = where(pts - ref.SHIFT)
    assert inside.sum() > 50 and on[:1331].sum() > 50 and not on[1331:].any() and (~inside & ~on).sum() > 1000
    for axis in AXES:
        r = ref.reference(name, axis)
        assert np.array_equal(r["on_surface"].astype(bool), on), axis
        assert np.array_equal(r["winding"][~on], inside[~on].astype(np.int32)), axis
        assert (r["crossings"][inside] == 1).all() and set(r["crossings"][~inside & ~on].tolist()) == {0, 2}, axis      # a convex solid: out, or in and out
        assert r["counts"][3] == (r["winding"] != 0).sum() and r["counts"][5] == on.sum() and r["counts"][6:].tolist() == [0, 0]
    assert ref.reference("cube", 0)["counts"][:3].tolist() == [4, 8, 0] and ref.reference("octahedron", 1)["counts"][:3].tolist() == [8, 0, 0]


def test_python_integers_and_int64_agree_where_int64_holds():
    v, f, pts = ref.CASES["octahedron"]()
    small = ref.winding(v, f, pts, 1)
    far = ref.winding(v + 2.0 ** 20, f, np.concatenate([pts + 2.0 ** 20, [[3.0, 3.0, 3.0]]]), 1)      # one far query: Python integers throughout
    for k in ("winding", "crossings", "on_surface"):
        assert np.array_equal(far[k][:-1], small[k]) and far[k][-1] == 0


@pytest.mark.parametrize("name", ["cube", "octahedron", "sphere"])
def test_rule_8(name):
    from surfacenet_amd import mesh
    v, f = _sphere() if name == "sphere" else ref.CASES[name]()[:2]
    pts = ref.solid_queries() + ref.SHIFT
    assert _closed_and_consistent(ref.triangles(f))
    want = {axis: ref.winding(v, f, pts, axis) for axis in AXES}
    rng = np.random.RandomState(3)
    fp, pp = rng.permutation(f.shape[0]), rng.permutation(pts.shape[0])
    for axis in AXES:
        w = want[axis]
        assert _same(ref.winding(v, f[fp], pts, axis), w)                                   # a permutation of the faces
        r = ref.winding(v, f, pts[pp], axis)                                                # a permutation of the points
        assert all(np.array_equal(r[k], w[k][pp]) for k in ref.KEYS[:3]) and np.array_equal(r["counts"], w["counts"])
        r = ref.winding(v, f[:, ::-1], pts, axis)                                           # every face reversed
        assert np.array_equal(r["winding"], -w["winding"]) and _same(r, w, ("crossings", "on_surface"))
        assert _same(ref.winding(v + [1000.0, 7.0, 2 ** 20], f, pts + [1000.0, 7.0, 2 ** 20], axis), w)      # whole cells
        free = w["on_surface"] == 0
        assert np.array_equal(w["winding"][free], want[0]["winding"][free])                 # the axes agree off the surface
        assert np.array_equal(w["on_surface"], want[0]["on_surface"])
        assert set(w["winding"][free].tolist()) == {0, 1}
    q = ref.cube(quads=True)[0] + ref.SHIFT, ref.cube(quads=True)[1]
    for axis in AXES:
        assert _same(ref.winding(q[0], mesh.triangulate(q[1]), pts, axis), ref.winding(q[0], q[1], pts, axis))


# ---- nested, overlapping and open meshes ----------------------------------------------------------------------------------------------------------------
def test_nested_and_overlapping_solids():
    pts = ref.CASES["nested_same"]()[2]
    at = lambda x, y, z: int(np.flatnonzero((pts == np.asarray([x, y, z]) + ref.OFFSET + ref.SHIFT).all(axis=1))[0])
    cavity, wall, outside, overlap, single = at(0, 0, 0), at(-3, 0, 0), at(-5, -5, -5), at(0, 0, 0), at(-2, -2, -2)
    for axis in AXES:
        r = ref.reference("nested_reversed", axis)
        assert (r["winding"][cavity], r["crossings"][cavity]) == (0, 2) and r["winding"][wall] == 1 and r["crossings"][wall] in (1, 3)
        assert (r["winding"][outside], r["crossings"][outside]) == (0, 0)
        r = ref.reference("nested_same", axis)
        assert (r["winding"][cavity], r["crossings"][cavity]) == (2, 2) and r["winding"][wall] == 1
        r = ref.reference("overlapping", axis)
        assert (r["winding"][overlap], r["crossings"][overlap]) == (2, 2) and r["winding"][single] == 1 and r["winding"][outside] == 0
        free = r["on_surface"] == 0
        assert np.array_equal(r["winding"][free], ref.reference("overlapping", 0)["winding"][free])
    assert np.array_equal(ref.reference("reversed")["winding"], -ref.reference("cube")["winding"])


def test_an_open_mesh_has_no_winding_number_but_a_surface():
    z, x = ref.reference("open_cube", 2), ref.reference("open_cube", 0)      # the +z face is missing: rays along +z leave through the hole
    free = z["on_surface"] == 0
    assert (z["winding"][free] != x["winding"][free]).any()
    for axis in AXES:
        assert np.array_equal(ref.reference("open_cube", axis)["on_surface"], z["on_surface"])
    assert z["counts"][5] < ref.reference("cube")["counts"][5]


# ---- the planted errors ---------------------------------------------------------------------------------------------------------------------------------------
PLANTED = [("closed", "cube", 2, ["winding", "crossings", "counts"]),      # a ray through an edge of the top face meets both its triangles
           ("above_closed", "cube", 2, ["winding", "crossings"]),           # a query on the top face is crossed by it
           ("no_parallel", "cube", 2, ["on_surface", "counts"]),            # the four faces parallel to the rays hold no query any more
           ("int64", "far", 2, None),
           ("axis_z", "open_cube", 0, None),
           ("non_cyclic", "cube", 1, None),
           ("parity", "nested_same", 2, ["winding", "counts"])]


@pytest.mark.parametrize("plant,name,axis,changed", PLANTED)
def test_a_planted_error_is_seen(plant, name, axis, changed):
    v, f, pts = ref.CASES[name]()
    want = ref.reference(name, axis)
    assert _same(ref.winding(v, f, pts, axis), want)
    got = ref.winding(v, f, pts, axis, plant=plant)
    diff = ref.same_bytes(got, want)
    assert diff and set(changed or ()) <= set(diff), diff
    if plant == "closed":
        i = int(np.flatnonzero((pts == np.asarray([2.0, 2.0, 1.0]) + ref.SHIFT).all(axis=1))[0])      # inside, under the top face's diagonal
        assert (want["winding"][i], want["crossings"][i]) == (1, 1) and (got["winding"][i], got["crossings"][i]) == (2, 2)      # the double count
    if plant == "non_cyclic":
        free = want["on_surface"] == 0
        assert np.array_equal(got["winding"][free], -want["winding"][free])      # the sign
    if plant == "parity":
        assert want["winding"].max() == 2 and got["winding"].max() == 1
    if plant == "int64":
        inside, on = ref.cube_where(pts, ref.FAR_LO, ref.FAR_HI)
        assert np.array_equal(want["on_surface"].astype(bool), on) and np.array_equal(want["winding"][~on], inside[~on].astype(np.int32))
        assert inside.sum() >= 3 and on.sum() >= 2


def test_the_restatement_refuses_in_the_librarys_words():
    v, f = bad.sheet()
    pts = np.zeros((3, 3))
    bv, bf, text = bad.bad_index(v, f, 2, 5)
    cv, cf, ctext = bad.bad_coordinate(v, f, 3, np.nan)
    out = pts.copy()
    out[1, 2], out[2, 0] = -4.5, np.nan
    for vv, ff, pp, axis, words in ((bv, bf, pts, 2, text), (cv, cf, pts, 2, ctext), (cv, bad.bad_index(v, f, 5, 5)[1], out, 2, ctext),
                                    (v, f, out, 0, ref.POINT_TEXT % 1), (v, f, pts, 3, ref.AXIS_TEXT % 3), (bv, bf, out, -1, ref.AXIS_TEXT % -1)):
        with pytest.raises(ValueError) as e:
            ref.winding(vv, ff, pp, axis)
        assert str(e.value) == words
    r = ref.winding(v, f, np.zeros((0, 3)), 1)                  # no query: the mesh is checked and counted
    assert r["winding"].shape == (0,) and r["counts"].tolist() == [0, 18, 0, 0, 0, 0, 0, 0]
    r = ref.winding(np.zeros((0, 3)), np.zeros((0, 4), np.int32), pts, 1)
    assert not r["winding"].any() and not r["counts"].any()


# ---- mesh.winding_number and mesh.signed_distance, before the library and on a stand-in ---------------------------------------------------------------------
class StandIn:
    """A context whose mesh_winding and mesh_distance are the restatements."""

    def mesh_winding(self, verts, faces, pts, axis=2, outputs=ref.KEYS[:3], device=False):
        return ref.winding(verts, faces, pts, axis)

    def mesh_distance(self, verts, faces, pts, max_dist, outputs=("d2", "face", "closest"), device=False):
        return md.distance(verts, faces, pts, max_dist)


def _stand_in(monkeypatch):
    from surfacenet_amd import runtime
    ctx = StandIn()
    monkeypatch.setattr(runtime, "any_context", lambda: ctx)


def _no_library(monkeypatch):
    from surfacenet_amd import runtime

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(runtime, "any_context", no_library)


def test_check_winding_args():
    from surfacenet_amd import mesh
    p, a = mesh.check_winding_args(np.zeros((2, 3), np.float32))
    assert p.dtype == np.float64 and p.shape == (2, 3) and a == 2
    assert [mesh.check_winding_args(p, x)[1] for x in (0, 1, 2, "x", "y", "z", np.int64(1), 2.0)] == [0, 1, 2, 0, 1, 2, 1, 2]
    pts = np.zeros((3, 3))
    out = pts.copy()
    out[1, 2], out[2, 0] = 2097144.0, np.nan
    axis_text = "axis = %r: 0, 1, 2 or one of ['x', 'y', 'z']"
    for points, axis, text in ((pts.astype(np.int32), 2, "points_lattice must be float32 or float64, not int32"), (np.zeros((3, 2)), 2, "points_lattice must be (n,3), not (3, 2)"),
                               (pts, 3, axis_text % 3), (pts, -1, axis_text % -1), (pts, "w", axis_text % "w"), (pts, True, axis_text % True), (pts, 1.5, axis_text % 1.5),
                               (pts, None, axis_text % None), (out, 2, ref.POINT_TEXT % 1), (out, 7, axis_text % 7)):
        with pytest.raises(ValueError) as e:
            mesh.check_winding_args(points, axis)
        assert str(e.value) == text


def test_the_python_layers_refuse_in_the_stages_words_before_the_library(monkeypatch):
    from surfacenet_amd import mesh
    _no_library(monkeypatch)
    v, f = bad.sheet()
    pts = np.zeros((2, 3))
    bv, bf, text = bad.bad_index(v, f, 2, 5)
    cv, cf, ctext = bad.bad_coordinate(v, f, 3, 2097144.0)
    cases = ((bv, bf, pts, text), (cv, cf, pts, ctext), (v.astype(np.int32), f, pts, "vert_lattice must be float32 or float64, not int32"),
             (v, np.zeros((18, 5), np.int32), pts, "faces must be (F,3) or (F,4), not (18, 5)"), (np.zeros((0, 3)), f, pts, "face 0 names a vertex outside [0, 0)"),
             (v, f, pts - 4.5, ref.POINT_TEXT % 0), (bv, bf, pts - 4.5, ref.POINT_TEXT % 0))
    for fn in (mesh.winding_number, mesh.signed_distance):
        for vv, ff, pp, words in cases:
            with pytest.raises(ValueError) as e:
                fn(pp, vv, ff)
            assert str(e.value) == words, fn
        with pytest.raises(ValueError, match="axis = 5"):
            fn(pts, v, f, axis=5)
    for kw, words in ((dict(max_dist=-2), "max_dist = -2"), (dict(resol=0.0), "resol = 0.0 must be finite and > 0"), (dict(resol="big"), "resol = 'big' must be a number")):
        with pytest.raises(ValueError, match=words):
            mesh.signed_distance(pts, v, f, **kw)
    unreferenced = np.concatenate([v, [[np.nan, 0, 0]]])       # an unreferenced vertex may hold anything
    for pp, vv, ff in ((np.zeros((0, 3)), unreferenced, f), (pts, np.zeros((0, 3)), np.zeros((0, 4), np.int32)), (pts, v, np.zeros((0, 3), np.int32))):      # no point, no face: without the library
        r = mesh.winding_number(pp, vv, ff, axis="x")
        n = pp.shape[0]
        assert [r[k].dtype for k in ("winding", "crossings", "on_surface", "inside")] == [np.int32, np.int32, bool, bool]
        assert all(r[k].shape == (n,) and not r[k].any() for k in ("winding", "crossings", "on_surface", "inside")) and [r[k] for k in mesh.WINDING_COUNTS] == [0] * 5
    assert mesh.WINDING_COUNTS == tuple(ref.COUNTS[i] for i in (0, 1, 2, 3, 5))


def test_winding_number_on_the_stand_in(monkeypatch):
    from surfacenet_amd import mesh
    _stand_in(monkeypatch)
    v, f, pts = ref.CASES["nested_same"]()
    for axis, name in ((0, "x"), (1, 1), (2, "z")):
        want = ref.reference("nested_same", axis)
        got = mesh.winding_number(pts.astype(np.float32), v, f.astype(np.int64), axis=name)      # (these coordinates are float32's own)
        assert np.array_equal(got["winding"], want["winding"]) and np.array_equal(got["crossings"], want["crossings"])
        assert got["on_surface"].dtype == bool and np.array_equal(got["on_surface"], want["on_surface"].astype(bool)) and np.array_equal(got["inside"], want["winding"] != 0)
        assert [got[k] for k in mesh.WINDING_COUNTS] == want["counts"][[0, 1, 2, 3, 5]].tolist() and got["n_inside"] > 0 and got["n_on_surface"] > 0
    assert mesh.winding_number(pts, v, f)["winding"].tobytes() == ref.reference("nested_same", 2)["winding"].tobytes()      # axis = 2 by default


def test_signed_distance_on_the_stand_in(monkeypatch):
    from surfacenet_amd import mesh
    _stand_in(monkeypatch)
    v, f, pts = ref.CASES["cube"]()
    inside, on = ref.cube_where(pts - ref.SHIFT)
    for axis in AXES:
        got = mesh.signed_distance(pts, v, f, max_dist=1.25, axis=axis, resol=0.4)
        want = ref.signed_distance(v, f, pts, 1.25, axis, 0.4)
        assert all(np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes() for k in ("dist", "face", "closest", "winding", "on_surface"))
        d = got["dist"]
        assert (d[on] == 0.0).all() and not np.signbit(d[on]).any() and (d[inside] < 0).all() and (d[~inside & ~on] > 0).all()      # sign and zero
        # scaling and the cap: point_to_mesh's capped distance in cells, times resol
        cells = mesh.signed_distance(pts, v, f, max_dist=1.25, axis=axis)
        assert np.array_equal(d, cells["dist"] * 0.4) and np.array_equal(got["closest"], cells["closest"] * 0.4, equal_nan=True) and d.max() == 1.25 * 0.4 and d.min() == -1.25 * 0.4
        assert np.array_equal(np.abs(cells["dist"]), np.minimum(np.sqrt(md.distance(v, f, pts, 1.25)["d2"]), 1.25) * ~on)
    plain = mesh.signed_distance(pts, v, f)                     # resol = 1, max_dist = 60, axis = 2
    assert np.array_equal(np.abs(plain["dist"]), np.minimum(np.sqrt(md.distance(v, f, pts, 60.0)["d2"]), 60.0))


# ---- the ABI: symbols are only added -----------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_version_script_binding_and_makefile():
    import ctypes
    import fnmatch
    import re
    from surfacenet_amd import _lib
    new = ("sn_mesh_winding", "sn_mesh_winding_dev")
    txt = open(os.path.join(ROOT, "include", "surfacenet_hip.h")).read()
    assert "#define SN_ABI_VERSION 2" in txt and "sn_mesh_winding_cfg" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    additions = re.search(r"Added since, without a version change.*?\*/", txt, flags=re.S).group(0)
    pattern = re.search(r"global:\s*([^;]+);", open(os.path.join(CSRC, "exports.map")).read()).group(1).strip()
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert re.search(r"\b%s\b" % name, additions), name
        assert fnmatch.fnmatchcase(name, pattern), (name, pattern)
        assert name in _lib.ABI_SYMBOLS, name
    assert re.search(r"typedef struct sn_mesh_winding_cfg \{\s*int axis;[^}]*int reserved;[^}]*\} sn_mesh_winding_cfg;", code)
    assert "sn_meshwinding.hip" in open(os.path.join(CSRC, "Makefile")).read()
    assert ctypes.sizeof(_lib.MeshWindingCfg) == 8 and [n for n, _ in _lib.MeshWindingCfg._fields_] == ["axis", "reserved"]
    from surfacenet_amd import Context, mesh
    assert all(callable(getattr(mesh, n)) for n in ("winding_number", "check_winding_args", "signed_distance")) and callable(Context.mesh_winding)


def test_the_rules_header_is_hip_free():
    with open(os.path.join(CSRC, "meshwinding_rules.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes and all("hip/" not in i and i in ("<stdint.h>", '"meshintersect_rules.h"', '"meshrender_rules.h"') for i in includes), includes
    with open(os.path.join(CSRC, "meshwinding.h")) as f:
        assert '#include "meshwinding_rules.h"' in f.read()


# ---- the rules and the argument checks of the C entry, on the CPU ------------------------------------------------------------------------------------
def test_rules_and_argument_checks_under_sanitizers(tmp_path):
    """tests/host/meshwinding_check.cpp runs csrc/meshwinding_rules.h - the axes, the quantisation, the class, rules 3 and 4 at the ends of the
    range - and sn_host.h's wnd_check_args over every end of every range, compiled stand-alone with -fsanitize=address,undefined and run as
    a child process. (point, triangle) rows go in as integers - the cube's and the octahedron's triangles against queries through their
    vertices, along their edges and inside ray-parallel faces, the degenerate set, the far cube - and what comes back equals the
    restatement, row by row."""
    rows = []
    lattice = ref.lattice_queries(-4, 4) + ref.SHIFT
    for name, pts in (("cube", lattice[::9]), ("octahedron", np.concatenate([lattice[::7], lattice[::11] + ref.OFFSET])), ("far", ref.far_queries()),
                      ("degenerate", ref.degenerate_case()[2][-5:])):
        v, f, _ = ref.CASES[name]()
        q = np.rint(np.nan_to_num(v) * ref.FIX).astype(np.int64)
        for n, t in enumerate(ref.triangles(f).tolist()):
            for k, p in enumerate(np.rint(pts * ref.FIX).astype(np.int64).tolist()):
                rows.append([(n + k) % 3] + p + q[t[0]].tolist() + q[t[1]].tolist() + q[t[2]].tolist())
    assert len(rows) > 400
    want = []
    for row in rows:
        x = np.asarray(row[1:], np.float64).reshape(4, 3) / ref.FIX      # (exact: |q| < 2^38)
        r = ref.winding(x[1:], [[0, 1, 2]], x[:1], row[0])
        want.append("%d %d %d" % (r["counts"][:3].tolist().index(1), r["on_surface"][0], r["winding"][0]))
    assert {w.split()[0] for w in want} == {"0", "1", "2"} and {w.split()[2] for w in want} == {"-1", "0", "1"} and sum(w.split()[1] == "1" for w in want) > 20
    exe = str(tmp_path / "meshwinding_check")
    _compile(os.path.join(ROOT, "tests", "host", "meshwinding_check.cpp"), exe)
    text = "".join(" ".join("%d" % x for x in row) + "\n" for row in rows)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "MESHWINDING-CHECK-OK %d rows" % len(rows) in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    got = p.stdout.splitlines()[:len(rows)]
    for i, line in enumerate(got):
        assert line == want[i], (i, rows[i], line, want[i])
