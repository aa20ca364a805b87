"""GPU (-m gpu): the hole filler (surfacenet_amd/csrc/meshfill.h) through the C ABI against the numpy restatement tests/meshfill_ref.py (DESIGN.md
section 4.17). Everything that decides or positions is an integer or one fixed-order fp64 expression, so new_verts_lattice, every integer output
and the counts are compared with array_equal; new_verts_mm as tests/test_gpu_mesh.py compares its own: within one float32 ulp."""
import ctypes

import numpy as np
import pytest

import meshfill_ref as ref
import meshsmooth_ref as sm
import normals_ref as nref

pytestmark = pytest.mark.gpu
ORIGIN, RESOL = (-20.0, -20.0, -20.0), 0.4
OUT = ("new_verts_mm", "new_verts_lattice", "loop_root", "loop_len", "new_faces", "vert_loop")


@pytest.fixture(scope="module")
def ctx(gpu_required):
    from surfacenet_amd import runtime
    return runtime.any_context()


def _compare(got, want):
    """got: Context.mesh_fill's dict; want: the restatement's."""
    assert got["new_verts_mm"].dtype == np.float32 and got["new_verts_lattice"].dtype == np.float64 and got["vert_loop"].dtype == np.uint8
    assert all(got[k].dtype == np.int32 for k in ("loop_root", "loop_len", "new_faces"))
    assert got["counts"].tolist() == want["counts"].tolist()
    for a, b in (("loop_root", "loop_root"), ("loop_len", "loop_len"), ("new_faces", "new_faces"), ("vert_loop", "vert_loop"),
                 ("new_verts_lattice", "new_vert_lattice")):
        assert got[a].shape == want[b].shape and np.array_equal(got[a], want[b]), a
    a, b = got["new_verts_mm"], want["new_vertices"]
    assert a.shape == b.shape and np.isfinite(a).all()
    ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)))
    assert (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= ulp.astype(np.float64)).all()


def _check(ctx, name, max_len=64, orientation=ref.HOLES, **kw):
    v, f = ref.CASES[name]()
    got = ctx.mesh_fill(v, f, max_len, orientation, origin=ORIGIN, resol=RESOL, **kw)
    _compare(got, ref.reference(name, max_len, orientation, ORIGIN, RESOL))
    return got


def _both_forms(ctx, name, max_len=64, orientation=ref.HOLES):
    a = _check(ctx, name, max_len, orientation)
    d = _check(ctx, name, max_len, orientation, device=True)
    for key in OUT + ("counts",):
        assert a[key].tobytes() == d[key].tobytes(), key       # sn_mesh_fill_dev = sn_mesh_fill bit for bit
    return a


# ---- the sheets: 81 vertices, one partial wave; quads and triangles, both orientations ------------------------------------------------------------
@pytest.mark.parametrize("name", ["sheet_q", "sheet_t", "sheet_hole_q", "sheet_hole_t"])
def test_sheets(ctx, name):
    holes = _both_forms(ctx, name)
    any_ = _both_forms(ctx, name, 64, ref.ANY)
    hole = 1 if "hole" in name else 0
    assert holes["counts"][3] == hole and any_["counts"][3] == hole + 1      # "any" caps the rim too
    if hole:
        assert holes["new_verts_lattice"].tolist() == [[4.0, 4.0, 7.0]] and holes["loop_root"].tolist() == [30]
        _check(ctx, name, 7)                                    # the hole is long, the rim stays a rim
        _check(ctx, name, 8, ref.ANY)                           # the rim is long, the hole is filled


# ---- sphere shells: R = 12 has 2,720 vertices, several workgroups and the scan's second level -----------------------------------------------------
@pytest.mark.parametrize("name,n", [("sphere6_hole_q", 44), ("sphere6_hole_t", 40), ("sphere12_hole_q", 60), ("sphere12_holes3_q", 60),
                                    ("sphere6_q", 0), ("sphere12_t", 0)])
def test_sphere_shells(ctx, name, n):
    got = _both_forms(ctx, name)
    _check(ctx, name, 64, ref.ANY)
    if n == 0:
        assert got["counts"][1:].tolist() == [0] * 7 and not got["vert_loop"].any()      # a closed mesh: H = T = 0
        return
    assert set(got["loop_len"].tolist()) == {n}
    assert _check(ctx, name, n - 1)["counts"][3:5].tolist() == [0, got["counts"][3]]      # max_len = n - 1 leaves the holes, state 2
    _check(ctx, name, n)
    # the second GPU stage: the capped sphere is closed
    v, f = ref.CASES[name]()
    vv, tris = ref.filled_mesh(v, f, dict(new_vert_lattice=got["new_verts_lattice"], new_faces=got["new_faces"]))
    assert ctx.mesh_smooth(vv, tris, 0)["counts"][1:3].tolist() == [0, 0]
    again = ctx.mesh_fill(vv, tris, 64, ref.HOLES)
    assert again["counts"][3] == 0 and again["counts"][7] == 0 and not again["vert_loop"].any()


def test_three_holes_interleave(ctx):
    got = _check(ctx, "sphere12_holes3_q")
    assert got["loop_root"].tolist() == [31, 654, 868]
    third = got["new_faces"][:, 2] - 2720
    assert (np.diff(third) != 0).sum() > 2 and (np.diff(got["new_faces"][:, 1]) > 0).all()


# ---- pinch, fan, opposed orientation; single faces; two holes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pinch", "two_holes", "fan3", "opposed", "single_q", "single_t", "rules", "surface", "soup"])
def test_hand_cases(ctx, name):
    for orientation in (ref.HOLES, ref.ANY):
        _both_forms(ctx, name, 64, orientation)
    _check(ctx, name, 3)


def test_face_order_and_translation(ctx):
    v, f = ref.CASES["sphere12_holes3_q"]()
    base = ctx.mesh_fill(v, f, 64, 0, origin=ORIGIN, resol=RESOL)
    perm = ctx.mesh_fill(v, f[np.random.default_rng(11).permutation(f.shape[0])], 64, 0, origin=ORIGIN, resol=RESOL)
    for key in OUT + ("counts",):
        assert base[key].tobytes() == perm[key].tobytes(), key
    shift = np.asarray([3.0, -2.0, 11.0])
    moved = ctx.mesh_fill(v + shift, f, 64, 0)
    assert np.array_equal(moved["new_verts_lattice"], base["new_verts_lattice"] + shift)
    for key in ("loop_root", "loop_len", "new_faces", "vert_loop", "counts"):
        assert np.array_equal(moved[key], base[key]), key


# ---- one long loop: 4,096 adders on the root's sums and votes ------------------------------------------------------------------------------------
def test_long_loop(ctx):
    got = _both_forms(ctx, "annulus4096", 4096)
    assert got["loop_len"].tolist() == [4096] and got["counts"].tolist() == [12288, 8192, 2, 1, 0, 1, 0, 4096]
    _check(ctx, "annulus4096", 4095)
    _check(ctx, "annulus4096", 65536, ref.ANY)


def test_two_runs_give_equal_bytes_and_workspace_reuse(ctx):
    v, f = ref.CASES["sphere12_holes3_q"]()
    a = ctx.mesh_fill(v, f, 64, 0, origin=ORIGIN, resol=RESOL)
    _check(ctx, "two_holes")                                    # a small call after a larger one: the workspace is reused, its tables are stale
    _check(ctx, "annulus4096", 4096)
    b = ctx.mesh_fill(v, f, 64, 0, origin=ORIGIN, resol=RESOL)
    for key in OUT + ("counts",):
        assert a[key].tobytes() == b[key].tobytes(), key
    _compare(a, ref.reference("sphere12_holes3_q", 64, 0, ORIGIN, RESOL))


# ---- empty, optional outputs, caps, errors -------------------------------------------------------------------------------------------------------
def _raw(ctx, v, f, max_len=64, orientation=0, origin=ORIGIN, resol=RESOL, nv=None, V=None, F=None, caps=None, outputs=True, dev=False):
    """sn_mesh_fill itself: -> (status, counts, arrays in OUT order), the arrays pre-filled with a pattern."""
    from surfacenet_amd import _lib
    v, f = np.ascontiguousarray(v, np.float64).reshape(-1, 3), np.ascontiguousarray(f, np.int32)
    cfg = _lib.MeshFillCfg(max_len, orientation)
    cfg.origin[:] = list(origin)
    cfg.resol = resol
    n, room = v.shape[0], max(f.size, 4)
    arrs = [np.full((room, 3), 7, np.float32), np.full((room, 3), 7, np.float64), np.full((room,), 7, np.int32), np.full((room,), 7, np.int32),
            np.full((room, 3), 7, np.int32), np.full((n,), 7, np.uint8)]
    counts = (ctypes.c_longlong * 8)(*([-5] * 8))
    cv, cf = (room, room) if caps is None else caps
    if not dev:
        rc = ctx._lib.sn_mesh_fill(ctx._h, ctypes.byref(cfg), n if V is None else V, _lib.ptr(v), f.shape[0] if F is None else F,
                                   f.shape[1] if nv is None else nv, _lib.ptr(f), cv, cf, *[_lib.ptr(a) if outputs else None for a in arrs], counts)
        return rc, list(counts), arrs
    with ctx._on_device((v, f)) as src, ctx._on_device(arrs) as dst:
        rc = ctx._lib.sn_mesh_fill_dev(ctx._h, ctypes.byref(cfg), n if V is None else V, src[0], f.shape[0] if F is None else F,
                                       f.shape[1] if nv is None else nv, src[1], cv, cf, *[d if outputs else None for d in dst], counts)
        for a, d in zip(arrs, dst):
            if a.nbytes:
                ctx.d2h(a, d)
    return rc, list(counts), arrs


def test_no_faces_and_optional_outputs(ctx):
    v, f = ref.CASES["two_holes"]()
    for dev in (False, True):
        rc, counts, arrs = _raw(ctx, v, f[:0], dev=dev)
        assert rc == 0 and counts == [0] * 8 and all((a == 7).all() for a in arrs)       # F = 0: all counts 0, nothing written
        rc, counts, arrs = _raw(ctx, v, f, outputs=False, dev=dev)
        assert rc == 0 and counts == ref.reference("two_holes")["counts"].tolist() and all((a == 7).all() for a in arrs)
    got = ctx.mesh_fill(v, f[:0])
    assert got["counts"].tolist() == [0] * 8 and got["new_faces"].shape == (0, 3) and not got["vert_loop"].any()


def test_short_cap_returns_the_counts_and_writes_nothing(ctx):
    from surfacenet_amd import _lib
    v, f = ref.CASES["two_holes"]()
    want = ref.reference("two_holes", 64, 0, ORIGIN, RESOL)
    for dev in (False, True):
        for caps in ((1, 8), (2, 7), (0, 0)):
            rc, counts, arrs = _raw(ctx, v, f, caps=caps, dev=dev)
            assert rc == -1 and counts == want["counts"].tolist() and "are needed" in _lib.last_error()
            assert all((a == 7).all() for a in arrs)
        rc, counts, arrs = _raw(ctx, v, f, caps=(2, 8), dev=dev)      # the exact caps
        assert rc == 0 and counts == want["counts"].tolist()
        assert np.array_equal(arrs[4][:8], want["new_faces"]) and (arrs[4][8:] == 7).all() and np.array_equal(arrs[5], want["vert_loop"])
        assert np.array_equal(arrs[1][:2], want["new_vert_lattice"]) and (arrs[1][2:] == 7).all()
    _compare(ctx.mesh_fill(v, f, origin=ORIGIN, resol=RESOL, cap=(0, 3)), want)          # Context.mesh_fill: one retry at the counts


def test_errors_name_the_face_the_smoother_names(ctx):
    from surfacenet_amd import SurfaceNetHipError, _lib
    v, f = sm.soup_case()
    v, f = v.copy(), f.copy()

    def refused(v, f, match, same_as_smooth=False, **kw):
        for device in (False, True):
            with pytest.raises(SurfaceNetHipError, match=match) as e:
                ctx.mesh_fill(v, f, kw.get("max_len", 64), kw.get("orientation", 0), origin=kw.get("origin", ORIGIN), resol=kw.get("resol", RESOL),
                              device=device)
            if same_as_smooth:
                with pytest.raises(SurfaceNetHipError) as s:
                    ctx.mesh_smooth(v, f, 0, origin=kw.get("origin", ORIGIN), resol=kw.get("resol", RESOL), device=device)
                assert str(e.value) == str(s.value)
        rc, counts, arrs = _raw(ctx, v, f, **kw)
        assert rc == -1 and counts == [0] * 8 and all((a == 7).all() for a in arrs)
        _check(ctx, "two_holes")                                # the context still works

    bad = f.copy()
    bad[15000, 2] = v.shape[0]
    bad[15100, 0] = -1
    refused(v, bad, "face 15000 ", True)
    first = int(np.nonzero((f == f[1234, 1]).any(axis=1))[0][0])
    for value in (np.nan, 2097144.0, np.nextafter(-4.0, -5.0)):
        far = v.copy()
        far[f[1234, 1], 2] = value
        refused(far, f, "face %d[ :]" % first, True)
    far = v.copy()
    far[f[1234, 1], 2] = np.nan
    mixed = f.copy()
    mixed[first + 1, 0] = -7                                    # the range error sits at the smaller face: it is the one named
    refused(far, mixed, "face %d[ :]" % first, True)
    for max_len in (2, 65537, -1):
        refused(v, f, "max_len", max_len=max_len)
    for orientation in (2, -1):
        refused(v, f, "orientation", orientation=orientation)
    for resol in (0.0, float("nan")):
        refused(v, f, "resol", True, resol=resol)
    refused(v, f, "origin", True, origin=(0.0, float("nan"), 0.0))
    for kw, word in ((dict(nv=5), "nv"), (dict(V=(1 << 28) + 1), "n_verts"), (dict(F=(1 << 28) + 1), "n_verts"), (dict(V=-1), "n_verts"),
                     (dict(caps=(-1, 4)), "cap_verts")):
        for dev in (False, True):
            rc, counts, arrs = _raw(ctx, v[:1], f[:1], dev=dev, **kw)
            assert rc == -1 and counts == [0] * 8 and word in _lib.last_error() and all((a == 7).all() for a in arrs)
    _check(ctx, "soup")


# ---- through the pipeline --------------------------------------------------------------------------------------------------------------------------
def test_fill_holes_and_scene_postpass(ctx, tmp_path):
    import mesh_ref as mr
    from surfacenet_amd import mesh, reconstruct
    # mesh.fill_holes: float32 positions, quads, both values of triangulate
    v, f = ref.CASES["sheet_hole_q"]()
    want = ref.reference("sheet_hole_q", 64, 0, ORIGIN, RESOL)
    got = mesh.fill_holes(v.astype(np.float32), f.astype(np.int64), origin=ORIGIN, resol=RESOL, vert_src=np.arange(81) * 3)
    assert np.array_equal(got["faces"], np.concatenate([mesh.triangulate(f), want["new_faces"]])) and got["faces"].dtype == np.int32
    assert np.array_equal(got["vert_lattice"], np.concatenate([v, want["new_vert_lattice"]])) and got["vertices"].shape == (82, 3)
    assert got["vert_src"].tolist() == (np.arange(81) * 3).tolist() + [90] and got["n_filled"] == 1 and got["n_new_faces"] == 8
    keep = mesh.fill_holes(v, f, origin=ORIGIN, resol=RESOL, triangulate=False)
    assert np.array_equal(keep["faces"], f) and np.array_equal(keep["new_faces"], want["new_faces"])
    assert mesh.smooth_mesh(got["vert_lattice"], got["faces"], 0)["n_boundary_edges"] == 32
    # the small scene of tests/test_gpu_meshsmooth.py
    s = nref.surface_scene((2, 2, 1))
    d = s["lists"]
    out = dict(prediction_list=d["prediction_list"], vxl_ijk_list=d["vxl_ijk_list"], rayPooling_votes_list=d["rayPooling_votes_list"],
               cube_ijk_np=d["cube_ijk_np"], param_np=s["param"], viewPair_np=s["viewPair"], rgb_list=d["rgb_list"])
    kw = dict(tau=0.7, gamma=0.5, N_refine_iter=2, cameraTs_np=s["cameraTs"], mesh=True)
    prefix = str(tmp_path / "scene_")
    post = reconstruct.scene_postpass(out, 32, 26, 2, mesh_fill=dict(max_len=16, orientation="any"), mesh_ply_prefix=prefix, **kw)
    plain = reconstruct.scene_postpass(out, 32, 26, 2, **kw)
    assert set(post) - set(plain) == {"fixThresh_mesh_filled", "adapt_mesh_filled"}
    origin, resol = mesh.lattice_origin(d["cube_ijk_np"], s["param"], 13)
    for key in plain:                                           # every other key is what it was
        a, b = post[key], plain[key]
        if isinstance(a, dict):
            assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a), key
        elif isinstance(a, list):
            assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), key
        else:
            assert np.array_equal(a, b), key
    for name in ("fixThresh", "adapt"):
        full, got = post[name + "_mesh"], post[name + "_mesh_filled"]
        want = mesh.fill_holes(full["vert_lattice"], full["quads"], 16, "any", origin=origin, resol=resol, vert_src=full["vert_src"])
        assert set(got) == set(want) and all(np.array_equal(got[k], want[k]) for k in want)
        r = ref.fill(full["vert_lattice"], full["quads"], 16, ref.ANY, origin, resol)
        assert np.array_equal(got["faces"][2 * full["quads"].shape[0]:], r["new_faces"]) and np.array_equal(got["vert_loop"], r["vert_loop"])
        assert [got[k] for k in mesh.FILL_COUNTS] == r["counts"].tolist()
        header, verts, faces = mr.parse_ply("%s%s_mesh_f16.ply" % (prefix, name))
        assert np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), got["vertices"]) and np.array_equal(np.asarray(faces), got["faces"])
        nl = np.concatenate(post[name + "_normal_list"])
        assert np.array_equal(np.stack([verts["nx"], verts["ny"], verts["nz"]], 1), nl[got["vert_src"]])
        assert np.array_equal(np.stack([verts["red"], verts["green"], verts["blue"]], 1), np.concatenate(d["rgb_list"])[got["vert_src"]])
    all3 = reconstruct.scene_postpass(out, 32, 26, 2, mesh_fill=dict(max_len=16, orientation="any"), mesh_smooth=2, mesh_cell=2, **kw)
    for name in ("fixThresh", "adapt"):                         # fill, smooth, decimate
        fm, smd = all3[name + "_mesh_filled"], all3[name + "_mesh_smoothed"]
        assert np.array_equal(fm["faces"], post[name + "_mesh_filled"]["faces"]) and np.array_equal(smd["faces"], fm["faces"])
        want = mesh.smooth_mesh(fm["vert_lattice"], fm["faces"], 2, origin=origin, resol=resol)
        assert np.array_equal(smd["vert_lattice"], want["vert_lattice"]) and smd["n_boundary_edges"] == want["n_boundary_edges"]
        dec = mesh.simplify_mesh(smd["vert_lattice"], smd["faces"], 2, origin=origin, resol=resol, vert_src=smd["vert_src"])
        assert all(np.array_equal(all3[name + "_mesh_simplified"][k], dec[k]) for k in dec)
