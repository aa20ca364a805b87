"""GPU (-m gpu): the mesh simplifier (surfacenet_amd/csrc/meshsimplify.h) through the C ABI against the numpy restatement
tests/meshsimplify_ref.py. Every decision is an exact integer and the sums are integer atomics, so every integer
output and vert_lattice are compared with array_equal; vertices as tests/test_gpu_mesh.py compares its verts_mm: within one float32 ulp."""
import ctypes

import numpy as np
import pytest

import meshsimplify_ref as ref
import mesh_ref as mr
import normals_ref as nref

pytestmark = pytest.mark.gpu
ORIGIN, RESOL = (-20.0, -20.0, -20.0), 0.4
OUT = ("verts_mm", "verts_lattice", "vert_rep", "vert_count", "faces", "face_src", "vert_cluster")


@pytest.fixture(scope="module")
def ctx(gpu_required):
    from surfacenet_amd import runtime
    return runtime.any_context()


def _compare(got, want):
    """got: Context.mesh_simplify's dict (or mesh.simplify_mesh's, which names two arrays differently); want: the restatement's."""
    mm = got["verts_mm"] if "verts_mm" in got else got["vertices"]
    lat = got["verts_lattice"] if "verts_lattice" in got else got["vert_lattice"]
    assert mm.dtype == np.float32 and lat.dtype == np.float64
    for key in ("vert_rep", "vert_count", "faces", "face_src", "vert_cluster"):
        assert got[key].dtype == np.int32 and got[key].shape == want[key].shape, (key, got[key].shape, want[key].shape)
        assert np.array_equal(got[key], want[key]), key
    assert lat.shape == want["vert_lattice"].shape and np.array_equal(lat, want["vert_lattice"])
    assert mm.shape == want["vertices"].shape
    ulp = np.spacing(np.maximum(np.abs(mm), np.abs(want["vertices"])))
    err = np.abs(mm.astype(np.float64) - want["vertices"].astype(np.float64))
    assert (err <= ulp.astype(np.float64)).all()


def _check(ctx, name, cell, placement=0, **kw):
    v, f = ref.CASES[name]()
    _compare(ctx.mesh_simplify(v, f, cell, placement, origin=ORIGIN, resol=RESOL, **kw), ref.reference(name, cell, placement, ORIGIN, RESOL))


# ---- the two hand cases: fewer than 64 (81) vertices, one partial wave -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sheet", "rules"])
def test_hand_cases(ctx, name):
    from surfacenet_amd import mesh
    v, f = ref.CASES[name]()
    for placement, word in ((0, "mean"), (1, "member")):
        want = ref.reference(name, 4, placement, ORIGIN, RESOL)
        _check(ctx, name, 4, placement)
        _check(ctx, name, 4, placement, device=True)
        got = mesh.simplify_mesh(v, f, 4, placement=word, origin=ORIGIN, resol=RESOL, vert_src=np.arange(v.shape[0]) * 3)
        _compare(got, want)
        assert np.array_equal(got["vert_src"], want["vert_rep"].astype(np.int64) * 3)
    if name == "sheet":
        got = ctx.mesh_simplify(v, f, 4)
        assert got["verts_lattice"].tolist() == [[x, y, 7.0] for x in (1.5, 5.5, 8.0) for y in (1.5, 5.5, 8.0)]
        assert got["face_src"].tolist() == [54, 55, 62, 63, 118, 119, 126, 127]
        quads = f.reshape(-1, 2, 3)[:, :, [0, 1, 2]]
        quads = np.concatenate([quads[:, 0], quads[:, 1, 2:]], axis=1)     # (F,4) quads go through triangulate
        _compare(mesh.simplify_mesh(v.astype(np.float32), quads, 4, origin=ORIGIN, resol=RESOL), ref.reference(name, 4, 0, ORIGIN, RESOL))
    else:
        spare = v.copy()
        spare[4] = np.nan                                       # an unreferenced vertex is not looked at
        _compare(ctx.mesh_simplify(spare, f, 4, origin=ORIGIN, resol=RESOL), ref.reference(name, 4, 0, ORIGIN, RESOL))


# ---- sphere shells: 2,720 vertices and 5,436 faces cross workgroups and the scan's second level ----------------------------------------------------
@pytest.mark.parametrize("R", [6, 9, 12])
def test_sphere_shells(ctx, R):
    for cell in (2, 4):
        for placement in (0, 1):
            _check(ctx, "sphere%d" % R, cell, placement)
    _check(ctx, "sphere%d" % R, 3, device=True)


# ---- the surface scene: negative coordinates, runs of one cluster that cross waves ---------------------------------------------------------------
@pytest.mark.parametrize("cell", [2, 3, 4, 8])
def test_surface_scene(ctx, cell):
    _check(ctx, "surface", cell)
    _check(ctx, "surface", cell, 1, device=True)


# ---- the soup: one cluster fed from many workgroups, duplicate faces owned elsewhere, the empty result --------------------------------------------
@pytest.mark.parametrize("cell", [2, 8, 16, 64])
def test_soup(ctx, cell):
    _check(ctx, "soup", cell)
    _check(ctx, "soup", cell, 1)
    if cell == 64:
        got = ctx.mesh_simplify(*ref.soup_case(), 64)
        assert got["faces"].shape == (0, 3) and got["verts_lattice"].shape == (0, 3) and (got["vert_cluster"] == -1).all()


def test_two_runs_give_equal_bytes_and_workspace_reuse(ctx):
    v, f = ref.soup_case()
    a = ctx.mesh_simplify(v, f, 16, origin=ORIGIN, resol=RESOL)
    _check(ctx, "rules", 4)                                     # a small call after a larger one: the workspace is reused, its tables are stale
    _check(ctx, "sphere6", 2)
    b = ctx.mesh_simplify(v, f, 16, origin=ORIGIN, resol=RESOL)
    d = ctx.mesh_simplify(v, f, 16, origin=ORIGIN, resol=RESOL, device=True)
    for key in OUT:
        assert a[key].tobytes() == b[key].tobytes(), key
        assert a[key].tobytes() == d[key].tobytes(), key        # sn_mesh_simplify_dev = sn_mesh_simplify bit for bit
    _compare(a, ref.reference("soup", 16, 0, ORIGIN, RESOL))


# ---- empty and short -----------------------------------------------------------------------------------------------------------------------------
def _raw(ctx, v, f, cell, cap_v, cap_f, placement=0, origin=ORIGIN, resol=RESOL):
    """sn_mesh_simplify itself: -> (status, n_verts, n_faces, arrays in OUT order), the arrays pre-filled with a pattern."""
    from surfacenet_amd import _lib
    v, f = np.ascontiguousarray(v, np.float64).reshape(-1, 3), np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    cfg = _lib.MeshSimplifyCfg(cell, placement)
    cfg.origin[:] = list(origin)
    cfg.resol = resol
    arrs = [np.full((cap_v, 3), 7, np.float32), np.full((cap_v, 3), 7, np.float64), np.full((cap_v,), 7, np.int32), np.full((cap_v,), 7, np.int32),
            np.full((cap_f, 3), 7, np.int32), np.full((cap_f,), 7, np.int32), np.full((v.shape[0],), 7, np.int32)]
    nv, nf = ctypes.c_longlong(-5), ctypes.c_longlong(-5)
    rc = ctx._lib.sn_mesh_simplify(ctx._h, ctypes.byref(cfg), v.shape[0], _lib.ptr(v), f.shape[0], _lib.ptr(f), cap_v, cap_f,
                                   *[_lib.ptr(a) for a in arrs], ctypes.byref(nv), ctypes.byref(nf))
    return rc, nv.value, nf.value, arrs


def test_no_faces(ctx):
    v, f = ref.sphere_case(6)
    for device in (False, True):
        got = ctx.mesh_simplify(v, f[:0], 4, device=device)
        assert got["faces"].shape == (0, 3) and got["verts_mm"].shape == (0, 3) and got["vert_cluster"].shape == (v.shape[0],)
        assert (got["vert_cluster"] == -1).all() and got["vert_cluster"].dtype == np.int32
    got = ctx.mesh_simplify(np.zeros((0, 3)), f[:0], 4)
    assert got["vert_cluster"].shape == (0,) and got["face_src"].shape == (0,)


def test_short_caps_report_the_counts_and_write_nothing(ctx):
    v, f = ref.sphere_case(6)
    want = ref.reference("sphere6", 2, 0, ORIGIN, RESOL)
    C, G = want["vert_rep"].shape[0], want["faces"].shape[0]
    for cap_v, cap_f in ((C - 1, G), (C, G - 1), (0, 0)):
        rc, nv, nf, arrs = _raw(ctx, v, f, 2, cap_v, cap_f)
        assert rc == -1 and (nv, nf) == (C, G)
        assert all((a == 7).all() for a in arrs)
    rc, nv, nf, arrs = _raw(ctx, v, f, 2, C + 3, G + 2)
    assert rc == 0 and (nv, nf) == (C, G)
    assert all((a[n:] == 7).all() for a, n in zip(arrs[:6], (C, C, C, C, G, G)))
    _compare(dict(zip(OUT, [a[:n] for a, n in zip(arrs, (C, C, C, C, G, G, v.shape[0]))])), want)
    # Context.mesh_simplify retries once with the exact counts
    _compare(ctx.mesh_simplify(v, f, 2, origin=ORIGIN, resol=RESOL, cap=(1, 1)), want)
    _compare(ctx.mesh_simplify(v, f, 2, origin=ORIGIN, resol=RESOL, cap=(C, 1), device=True), want)
    # every output is optional
    from surfacenet_amd import _lib
    cfg = _lib.MeshSimplifyCfg(2, 0)
    cfg.resol = 1.0
    nv, nf = ctypes.c_longlong(-5), ctypes.c_longlong(-5)
    f32 = np.ascontiguousarray(f, np.int32)
    rc = ctx._lib.sn_mesh_simplify(ctx._h, ctypes.byref(cfg), v.shape[0], _lib.ptr(v), f32.shape[0], _lib.ptr(f32), 0, 0, *([None] * 7),
                                   ctypes.byref(nv), ctypes.byref(nf))
    assert rc == -1 and (nv.value, nf.value) == (C, G)
    rc = ctx._lib.sn_mesh_simplify(ctx._h, ctypes.byref(cfg), v.shape[0], _lib.ptr(v), f32.shape[0], _lib.ptr(f32), C, G, *([None] * 7),
                                   ctypes.byref(nv), ctypes.byref(nf))
    assert rc == 0 and (nv.value, nf.value) == (C, G)


# ---- errors --------------------------------------------------------------------------------------------------------------------------------------
def test_errors_name_the_face_and_leave_the_context_usable(ctx):
    from surfacenet_amd import SurfaceNetHipError
    v, f = ref.soup_case()
    v, f = v.copy(), f.copy()

    def refused(v, f, match, cell=4, placement=0, origin=ORIGIN, resol=RESOL):
        for device in (False, True):
            with pytest.raises(SurfaceNetHipError, match=match):
                ctx.mesh_simplify(v, f, cell, placement, origin=origin, resol=resol, device=device)
        rc, nv, nf, arrs = _raw(ctx, v, f, cell, 16, 16, placement, origin, resol)
        assert rc == -1 and (nv, nf) == (0, 0) and all((a == 7).all() for a in arrs)
        _check(ctx, "rules", 4)                                 # the context still works

    bad = f.copy()
    bad[15000, 2] = v.shape[0]
    bad[15100, 0] = -1
    refused(v, bad, "face 15000 ")
    for value in (np.nan, np.inf, 2097144.0, np.nextafter(-4.0, -5.0)):
        far = v.copy()
        far[f[1234, 1], 2] = value
        first = int(np.nonzero((f == f[1234, 1]).any(axis=1))[0][0])
        refused(far, f, "face %d[ :]" % first)
    far = v.copy()
    far[f[1234, 1], 2] = np.nan
    mixed = f.copy()
    mixed[first + 1, 0] = -7                                    # the range error sits at the smaller face: it is the one named
    refused(far, mixed, "face %d[ :]" % first)
    mixed[max(first - 1, 0), 0] = 1 << 20
    refused(far, mixed, "face %d " % max(first - 1, 0))
    spare = np.concatenate([v, [[np.nan, 0.0, 0.0]]])           # a vertex no face names is not looked at
    _compare(ctx.mesh_simplify(spare, f, 8, origin=ORIGIN, resol=RESOL),
             dict(ref.reference("soup", 8, 0, ORIGIN, RESOL), vert_cluster=np.append(ref.reference("soup", 8, 0, ORIGIN, RESOL)["vert_cluster"], -1).astype(np.int32)))
    edge = v.copy()
    edge[f[0, 0]] = [-4.0, np.nextafter(2097144.0, 0.0), 0.0]   # both ends of the range are legal
    _compare(ctx.mesh_simplify(edge, f, 64, origin=ORIGIN, resol=RESOL), ref.simplify(edge, f, 64, 0, ORIGIN, RESOL))
    for cell in (1, 65, 0, -2):
        refused(v, f, "cell", cell=cell)
    for placement in (2, -1):
        refused(v, f, "placement", placement=placement)
    for resol in (0.0, -0.4, float("inf"), float("nan")):
        refused(v, f, "resol", resol=resol)
    refused(v, f, "origin", origin=(0.0, float("nan"), 0.0))
    refused(v, f, "origin", origin=(float("inf"), 0.0, 0.0))


def test_limits_are_refused_before_any_array_is_read(ctx):
    """n_verts, n_faces over 2^28: refused from the arguments alone (the arrays behind them are one row)."""
    from surfacenet_amd import _lib
    cfg = _lib.MeshSimplifyCfg(4, 0)
    cfg.resol = 1.0
    v, f = np.zeros((1, 3), np.float64), np.zeros((1, 3), np.int32)
    nv, nf = ctypes.c_longlong(-5), ctypes.c_longlong(-5)
    for V, F in (((1 << 28) + 1, 1), (1, (1 << 28) + 1), (-1, 1)):
        for fn in (ctx._lib.sn_mesh_simplify, ctx._lib.sn_mesh_simplify_dev):
            rc = fn(ctx._h, ctypes.byref(cfg), V, _lib.ptr(v), F, _lib.ptr(f), 0, 0, *([None] * 7), ctypes.byref(nv), ctypes.byref(nf))
            assert rc == -1 and (nv.value, nf.value) == (0, 0) and "n_verts" in _lib.last_error()


def test_too_many_clusters_are_refused(ctx):
    """P >= 2^21: a 128^3 grid of vertices two cells apart, every one its own cluster at cell = 2; cell = 4 gives 64^3 clusters and runs."""
    from surfacenet_amd import SurfaceNetHipError
    g = np.arange(128, dtype=np.float64) * 2
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    strip = np.minimum(np.arange(1 << 21, dtype=np.int32).reshape(-1, 1) + np.asarray([[0, 1, 2]], np.int32), (1 << 21) - 1)
    with pytest.raises(SurfaceNetHipError, match="larger cell"):
        ctx.mesh_simplify(grid, strip, 2)
    got = ctx.mesh_simplify(grid, strip, 4)
    assert got["vert_count"].sum() <= 1 << 21 and (got["vert_count"] <= 8).all() and got["verts_lattice"].shape[0] <= 1 << 18
    assert (got["vert_cluster"][got["vert_rep"]] == np.arange(got["vert_rep"].shape[0])).all()


# ---- through the pipeline ------------------------------------------------------------------------------------------------------------------------
def test_scene_postpass_mesh_cell_and_ply(ctx, tmp_path):
    from surfacenet_amd import evaluation, mesh, reconstruct
    s = nref.surface_scene((2, 2, 1))
    d = s["lists"]
    out = dict(prediction_list=d["prediction_list"], vxl_ijk_list=d["vxl_ijk_list"], rayPooling_votes_list=d["rayPooling_votes_list"],
               cube_ijk_np=d["cube_ijk_np"], param_np=s["param"], viewPair_np=s["viewPair"], rgb_list=d["rgb_list"])
    kw = dict(tau=0.7, gamma=0.5, N_refine_iter=2, cameraTs_np=s["cameraTs"], mesh=True)
    prefix = str(tmp_path / "scene_")
    post = reconstruct.scene_postpass(out, 32, 26, 2, mesh_cell=2, mesh_ply_prefix=prefix, **kw)
    plain = reconstruct.scene_postpass(out, 32, 26, 2, **kw)
    assert set(post) - set(plain) == {"fixThresh_mesh_simplified", "adapt_mesh_simplified"}
    origin, resol = mesh.lattice_origin(d["cube_ijk_np"], s["param"], 13)
    for name in ("fixThresh", "adapt"):
        full, got = post[name + "_mesh"], post[name + "_mesh_simplified"]
        for k in full:
            assert np.array_equal(full[k], plain[name + "_mesh"][k]), (name, k)
        want = mesh.simplify_mesh(full["vert_lattice"], full["quads"], 2, origin=origin, resol=resol, vert_src=full["vert_src"])
        assert set(got) == {"vertices", "faces", "vert_lattice", "vert_rep", "vert_count", "face_src", "vert_cluster", "vert_src"}
        for k in want:
            assert np.array_equal(got[k], want[k]), (name, k)
        _compare(got, ref.simplify(full["vert_lattice"], mesh.triangulate(full["quads"]), 2, 0, origin, resol))
        assert 0 < got["faces"].shape[0] < full["quads"].shape[0] and np.array_equal(got["vert_src"], full["vert_src"][got["vert_rep"]])
        path = "%s%s_mesh_c2.ply" % (prefix, name)
        pv, pf = evaluation.read_ply_mesh(path)
        assert np.array_equal(pv, got["vertices"]) and np.array_equal(pf, got["faces"])
        header, verts, _ = mr.parse_ply(path)
        nl = np.concatenate(post[name + "_normal_list"])
        assert np.array_equal(np.stack([verts["nx"], verts["ny"], verts["nz"]], 1), nl[got["vert_src"]])
        assert np.array_equal(np.stack([verts["red"], verts["green"], verts["blue"]], 1), np.concatenate(d["rgb_list"])[got["vert_src"]])
    member = reconstruct.scene_postpass(out, 32, 26, 2, mesh_cell=4, mesh_placement="member", **kw)["adapt_mesh_simplified"]
    assert np.array_equal(member["vert_lattice"], post["adapt_mesh"]["vert_lattice"][member["vert_rep"]])
