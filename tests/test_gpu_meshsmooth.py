"""GPU (-m gpu): the mesh smoother (surfacenet_amd/csrc/meshsmooth.h) through the C ABI against the numpy restatement tests/meshsmooth_ref.py
(DESIGN.md section 4.16). Every value is an exact integer and the sums do not depend on the order of arrival, so verts_lattice, vert_degree,
vert_flags and the counts are compared with array_equal; verts_mm as tests/test_gpu_mesh.py compares its own: within one float32 ulp."""
import ctypes

import numpy as np
import pytest

import mesh_ref as mr
import meshsmooth_ref as ref
import normals_ref as nref

pytestmark = pytest.mark.gpu
ORIGIN, RESOL = (-20.0, -20.0, -20.0), 0.4
LAM, MU = ref.q16(0.5), ref.q16(-0.53)
OUT = ("verts_mm", "verts_lattice", "vert_degree", "vert_flags")


@pytest.fixture(scope="module")
def ctx(gpu_required):
    from surfacenet_amd import runtime
    return runtime.any_context()


def _compare(got, want):
    """got: Context.mesh_smooth's dict (or mesh.smooth_mesh's, which names its arrays differently); want: the restatement's."""
    mm = got["verts_mm"] if "verts_mm" in got else got["vertices"]
    lat = got["verts_lattice"] if "verts_lattice" in got else got["vert_lattice"]
    counts = got["counts"] if "counts" in got else [got[k] for k in ("n_edges", "n_boundary_edges", "n_nonmanifold_edges", "n_referenced")]
    assert mm.dtype == np.float32 and lat.dtype == np.float64 and got["vert_degree"].dtype == np.int32 and got["vert_flags"].dtype == np.uint8
    assert list(counts) == want["counts"].tolist()
    assert np.array_equal(got["vert_degree"], want["vert_degree"]) and np.array_equal(got["vert_flags"], want["vert_flags"])
    assert lat.shape == want["vert_lattice"].shape and lat.tobytes() == want["vert_lattice"].tobytes()      # (an unreferenced NaN: bit for bit)
    assert mm.shape == want["vertices"].shape
    nan = np.isnan(want["vertices"])
    assert np.array_equal(np.isnan(mm), nan) and not nan[(want["vert_flags"] & ref.REFERENCED) != 0].any()
    a, b = np.where(nan, np.float32(0), mm), np.where(nan, np.float32(0), want["vertices"])
    fin = np.isfinite(b)
    assert np.array_equal(a[~fin], b[~fin])
    ulp = np.spacing(np.maximum(np.abs(a[fin]), np.abs(b[fin])))
    assert (np.abs(a[fin].astype(np.float64) - b[fin].astype(np.float64)) <= ulp.astype(np.float64)).all()


def _check(ctx, name, iterations, lam=LAM, mu=MU, boundary=ref.CURVE, **kw):
    v, f = ref.CASES[name]()
    _compare(ctx.mesh_smooth(v, f, iterations, lam, mu, boundary, origin=ORIGIN, resol=RESOL, **kw),
             ref.reference(name, iterations, lam, mu, boundary, ORIGIN, RESOL))


# ---- the sheet: 81 vertices, one partial wave; quads and triangles, every mode -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sheet_q", "sheet_t"])
def test_sheet(ctx, name):
    v, f = ref.CASES[name]()
    for boundary in (ref.FIXED, ref.CURVE, ref.FREE):
        for iterations in (0, 1, 5):
            _check(ctx, name, iterations, boundary=boundary)
    _check(ctx, name, 5, device=True)
    fixed = ctx.mesh_smooth(v, f, 5, LAM, MU, ref.FIXED)
    assert np.array_equal(fixed["verts_lattice"], v) and fixed["counts"].tolist() == [144 if name == "sheet_q" else 208, 32, 0, 81]
    free = ctx.mesh_smooth(v, f, 5, LAM, MU, ref.FREE)
    assert (free["verts_lattice"] != v).any() and (free["verts_lattice"][:, 2] == 7.0).all()


# ---- sphere shells: R = 12 has 2,720 vertices, several workgroups and the scan's second level -----------------------------------------------------
@pytest.mark.parametrize("name", ["sphere6_q", "sphere6_t", "sphere12_q", "sphere12_t"])
def test_sphere_shells(ctx, name):
    _check(ctx, name, 10, boundary=ref.FREE)
    _check(ctx, name, 10, mu=0, boundary=ref.FREE)
    _check(ctx, name, 10, device=True)
    v, f = ref.CASES[name]()
    if name.endswith("_q"):
        got = ctx.mesh_smooth(v, f, 10, LAM, MU, ref.FREE)
        assert got["counts"][1] == 0 and got["counts"][2] == 0 and got["vert_degree"].max() <= 6
        assert 0.98 <= mr.signed_volume(got["verts_lattice"], f) / mr.signed_volume(v, f) <= 1.02


# ---- the surface scene and its simplifications: an open boundary, non-manifold edges, degrees up to 11 --------------------------------------------
@pytest.mark.parametrize("name", ["surface", "surface_k2", "surface_k8"])
def test_surface_scene(ctx, name):
    for iterations in (0, 4):
        _check(ctx, name, iterations, boundary=ref.CURVE)
    _check(ctx, name, 4, boundary=ref.CURVE, device=True)
    if name != "surface":
        assert ref.reference(name, 0, LAM, MU, ref.CURVE, ORIGIN, RESOL)["counts"][2] > 0


# ---- the soup: repeated edges, degenerate sides, unreferenced vertices, degrees of several dozen --------------------------------------------------
@pytest.mark.parametrize("boundary", [ref.FIXED, ref.CURVE, ref.FREE])
def test_soup(ctx, boundary):
    _check(ctx, "soup", 3, boundary=boundary)
    _check(ctx, "soup", 3, boundary=boundary, device=True)
    v, f = ref.soup_case()
    quads = np.concatenate([f, f[::-1, :1]], axis=1)           # ... and as 20,000 random quads
    _compare(ctx.mesh_smooth(v, quads, 3, LAM, MU, boundary, origin=ORIGIN, resol=RESOL), ref.smooth(v, quads, 3, LAM, MU, boundary, ORIGIN, RESOL))


# ---- fans: rows far longer than a wave -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [300, 5000])
def test_fan(ctx, n):
    for boundary in (ref.CURVE, ref.FREE):
        _check(ctx, "fan%d" % n, 3, boundary=boundary)
    got = ctx.mesh_smooth(*ref.fan_case(n), 0)
    assert got["vert_degree"][0] == n and got["counts"].tolist() == [2 * n, n, 0, n + 1]


# ---- the hand-made rule cases ----------------------------------------------------------------------------------------------------------------------
def test_rule_cases(ctx):
    from surfacenet_amd import mesh
    v, f = ref.rules_case()
    for boundary, word in ((ref.FIXED, "fixed"), (ref.CURVE, "curve"), (ref.FREE, "free")):
        for iterations in (0, 1, 3):
            _check(ctx, "rules", iterations, boundary=boundary)
        got = mesh.smooth_mesh(v, f, 3, boundary=word, origin=ORIGIN, resol=RESOL)
        _compare(got, ref.reference("rules", 3, LAM, MU, boundary, ORIGIN, RESOL))
        assert got["vert_lattice"][7].tobytes() == v[7].tobytes()      # the unreferenced NaN vertex: bit for bit
    got = ctx.mesh_smooth(v, f, 0)
    assert got["counts"].tolist() == [10, 5, 2, 7] and got["vert_flags"].tolist() == [7, 7, 7, 3, 1, 3, 3, 0]
    assert got["verts_lattice"][5].tolist() == [-4.0] * 3
    # the clamp: lam = mu = -1 throws every vertex out until the ends of the range hold it
    _check(ctx, "clamp", 60, lam=-65536, mu=-65536, boundary=ref.FREE)
    c = ctx.mesh_smooth(*ref.clamp_case(), 60, -65536, -65536, ref.FREE)
    assert c["verts_lattice"].min() == -4.0 and c["verts_lattice"].max() == ref.QMAX / 65536.0
    for w in (65536, -65536, 1, -1, 0):
        _check(ctx, "sphere6_q", 2, lam=w, mu=-w, boundary=ref.FREE)
    # float32 positions and (F,4) quads through mesh.smooth_mesh
    vq, fq = ref.sheet_case(True)
    _compare(mesh.smooth_mesh(vq.astype(np.float32), fq.astype(np.int64), 5, boundary="free", origin=ORIGIN, resol=RESOL),
             ref.reference("sheet_q", 5, LAM, MU, ref.FREE, ORIGIN, RESOL))


def test_two_runs_give_equal_bytes_host_equals_device_and_workspace_reuse(ctx):
    v, f = ref.soup_case()
    a = ctx.mesh_smooth(v, f, 3, origin=ORIGIN, resol=RESOL)
    _check(ctx, "rules", 3)                                     # a small call after a larger one: the workspace is reused, its tables are stale
    _check(ctx, "sphere6_q", 2)
    b = ctx.mesh_smooth(v, f, 3, origin=ORIGIN, resol=RESOL)
    d = ctx.mesh_smooth(v, f, 3, origin=ORIGIN, resol=RESOL, device=True)
    for key in OUT + ("counts",):
        assert a[key].tobytes() == b[key].tobytes(), key
        assert a[key].tobytes() == d[key].tobytes(), key        # sn_mesh_smooth_dev = sn_mesh_smooth bit for bit
    _compare(a, ref.reference("soup", 3, LAM, MU, ref.CURVE, ORIGIN, RESOL))


# ---- empty, optional outputs, errors ---------------------------------------------------------------------------------------------------------------
def _raw(ctx, v, f, iterations=2, lam=LAM, mu=MU, boundary=1, origin=ORIGIN, resol=RESOL, nv=None, V=None, F=None, outputs=True, dev=False):
    """sn_mesh_smooth itself: -> (status, counts, arrays in OUT order), the arrays pre-filled with a pattern."""
    from surfacenet_amd import _lib
    v, f = np.ascontiguousarray(v, np.float64).reshape(-1, 3), np.ascontiguousarray(f, np.int32)
    cfg = _lib.MeshSmoothCfg(iterations, lam, mu, boundary)
    cfg.origin[:] = list(origin)
    cfg.resol = resol
    n = v.shape[0]
    arrs = [np.full((n, 3), 7, np.float32), np.full((n, 3), 7, np.float64), np.full((n,), 7, np.int32), np.full((n,), 7, np.uint8)]
    counts = (ctypes.c_longlong * 4)(-5, -5, -5, -5)
    fn = ctx._lib.sn_mesh_smooth_dev if dev else ctx._lib.sn_mesh_smooth
    rc = fn(ctx._h, ctypes.byref(cfg), n if V is None else V, _lib.ptr(v), f.shape[0] if F is None else F, f.shape[1] if nv is None else nv,
            _lib.ptr(f), *[_lib.ptr(a) if outputs else None for a in arrs], counts)
    return rc, list(counts), arrs


def test_no_faces(ctx):
    v, f = ref.rules_case()
    for device in (False, True):
        got = ctx.mesh_smooth(v, f[:0], 5, origin=ORIGIN, resol=RESOL, device=device)
        _compare(got, ref.smooth(v, f[:0], 5, LAM, MU, ref.CURVE, ORIGIN, RESOL))
        assert got["counts"].tolist() == [0, 0, 0, 0] and got["verts_lattice"].tobytes() == v.tobytes() and not got["vert_flags"].any()
    got = ctx.mesh_smooth(np.zeros((0, 3)), np.zeros((0, 4), np.int32), 5)
    assert got["verts_lattice"].shape == (0, 3) and got["counts"].tolist() == [0, 0, 0, 0]


def test_every_output_is_optional(ctx):
    v, f = ref.sphere_case(6)
    want = ref.reference("sphere6_q", 0, LAM, MU, ref.CURVE, ORIGIN, RESOL)
    rc, counts, arrs = _raw(ctx, v, f, iterations=0, outputs=False)
    assert rc == 0 and counts == want["counts"].tolist() and all((a == 7).all() for a in arrs)


def test_errors_name_the_face_and_leave_the_context_usable(ctx):
    from surfacenet_amd import SurfaceNetHipError, _lib
    v, f = ref.soup_case()
    v, f = v.copy(), f.copy()

    def refused(v, f, match, **kw):
        for device in (False, True):
            with pytest.raises(SurfaceNetHipError, match=match):
                ctx.mesh_smooth(v, f, kw.get("iterations", 2), kw.get("lam", LAM), kw.get("mu", MU), kw.get("boundary", 1),
                                origin=kw.get("origin", ORIGIN), resol=kw.get("resol", RESOL), device=device)
        rc, counts, arrs = _raw(ctx, v, f, **kw)
        assert rc == -1 and counts == [0, 0, 0, 0] and all((a == 7).all() for a in arrs)
        _check(ctx, "rules", 3)                                 # the context still works

    bad = f.copy()
    bad[15000, 2] = v.shape[0]
    bad[15100, 0] = -1
    refused(v, bad, "face 15000 ")
    first = int(np.nonzero((f == f[1234, 1]).any(axis=1))[0][0])
    for value in (np.nan, np.inf, 2097144.0, np.nextafter(-4.0, -5.0)):
        far = v.copy()
        far[f[1234, 1], 2] = value
        refused(far, f, "face %d[ :]" % first)
    far = v.copy()
    far[f[1234, 1], 2] = np.nan
    mixed = f.copy()
    mixed[first + 1, 0] = -7                                    # the range error sits at the smaller face: it is the one named
    refused(far, mixed, "face %d[ :]" % first)
    mixed[max(first - 1, 0), 0] = 1 << 20
    refused(far, mixed, "face %d " % max(first - 1, 0))
    for iterations in (-1, 1001):
        refused(v, f, "iterations", iterations=iterations)
    for w in (65537, -65537):
        refused(v, f, "lam_q16", lam=w)
        refused(v, f, "mu_q16", mu=w)
    for boundary in (3, -1):
        refused(v, f, "boundary", boundary=boundary)
    for resol in (0.0, -0.4, float("inf"), float("nan")):
        refused(v, f, "resol", resol=resol)
    refused(v, f, "origin", origin=(0.0, float("nan"), 0.0))
    refused(v, f, "origin", origin=(float("inf"), 0.0, 0.0))
    # nv, and V or F over the limit: refused from the arguments alone, in both forms
    for kw, word in ((dict(nv=5), "nv"), (dict(nv=2), "nv"), (dict(V=(1 << 28) + 1), "n_verts"), (dict(F=(1 << 28) + 1), "n_verts"), (dict(V=-1), "n_verts")):
        for dev in (False, True):
            rc, counts, arrs = _raw(ctx, v[:1], f[:1], dev=dev, **kw)
            assert rc == -1 and counts == [0, 0, 0, 0] and word in _lib.last_error() and all((a == 7).all() for a in arrs)
    _check(ctx, "soup", 3)


# ---- through the pipeline --------------------------------------------------------------------------------------------------------------------------
def test_scene_postpass_mesh_smooth_and_ply(ctx, tmp_path):
    from surfacenet_amd import mesh, reconstruct
    s = nref.surface_scene((2, 2, 1))
    d = s["lists"]
    out = dict(prediction_list=d["prediction_list"], vxl_ijk_list=d["vxl_ijk_list"], rayPooling_votes_list=d["rayPooling_votes_list"],
               cube_ijk_np=d["cube_ijk_np"], param_np=s["param"], viewPair_np=s["viewPair"], rgb_list=d["rgb_list"])
    kw = dict(tau=0.7, gamma=0.5, N_refine_iter=2, cameraTs_np=s["cameraTs"], mesh=True)
    prefix = str(tmp_path / "scene_")
    post = reconstruct.scene_postpass(out, 32, 26, 2, mesh_smooth=3, mesh_ply_prefix=prefix, **kw)
    plain = reconstruct.scene_postpass(out, 32, 26, 2, **kw)
    assert set(post) - set(plain) == {"fixThresh_mesh_smoothed", "adapt_mesh_smoothed"}
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
        full, got = post[name + "_mesh"], post[name + "_mesh_smoothed"]
        want = ref.smooth(full["vert_lattice"], full["quads"], 3, LAM, MU, ref.CURVE, origin, resol)
        _compare(got, want)
        assert np.array_equal(got["quads"], full["quads"]) and np.array_equal(got["vert_src"], full["vert_src"])
        assert (got["vert_lattice"] != full["vert_lattice"]).any()
        path = "%s%s_mesh_s3.ply" % (prefix, name)
        header, verts, faces = mr.parse_ply(path)
        assert np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), got["vertices"]) and np.array_equal(np.asarray(faces), full["quads"])
        nl = np.concatenate(post[name + "_normal_list"])
        assert np.array_equal(np.stack([verts["nx"], verts["ny"], verts["nz"]], 1), nl[full["vert_src"]])
        assert np.array_equal(np.stack([verts["red"], verts["green"], verts["blue"]], 1), np.concatenate(d["rgb_list"])[full["vert_src"]])
    both = reconstruct.scene_postpass(out, 32, 26, 2, mesh_smooth=dict(iterations=3), mesh_cell=2, **kw)
    for name in ("fixThresh", "adapt"):                         # smooth, then decimate
        sm = both[name + "_mesh_smoothed"]
        assert np.array_equal(sm["vert_lattice"], post[name + "_mesh_smoothed"]["vert_lattice"])
        want = mesh.simplify_mesh(sm["vert_lattice"], sm["quads"], 2, origin=origin, resol=resol, vert_src=sm["vert_src"])
        assert set(both[name + "_mesh_simplified"]) == set(want)
        for k in want:
            assert np.array_equal(both[name + "_mesh_simplified"][k], want[k]), (name, k)
        assert not np.array_equal(want["vert_lattice"], plain_simplified(mesh, post[name + "_mesh"], origin, resol)["vert_lattice"])


def plain_simplified(mesh, m, origin, resol):
    return mesh.simplify_mesh(m["vert_lattice"], m["quads"], 2, origin=origin, resol=resol)
