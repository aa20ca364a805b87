"""GPU (-m gpu): the mesh sampler (surfacenet_amd/csrc/meshsample.h) through the C ABI against the numpy restatement tests/meshsample_ref.py
(DESIGN.md section 4.13). Subdivision counts and sample positions hang on exact integers and the float arithmetic is one fp64 rounding per
operation on both sides, so points and tri are compared with array_equal: no tolerance. Then the evaluation of a mesh built on it."""
import ctypes

import numpy as np
import pytest

import meshsample_ref as ref
import pointeval_ref as pref

pytestmark = pytest.mark.gpu
DST = 0.2


@pytest.fixture(scope="module")
def ctx(gpu_required):
    from surfacenet_amd import runtime
    return runtime.any_context()


def _same(got, want):
    assert got[0].dtype == np.float64 and got[1].dtype == np.int32
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, (got[0].shape, want[0].shape)
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0], want[0])


# ---- (a) single triangles ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dst", [("RIGHT", 0.2), ("HALF", 0.25), ("HALF", 0.2), ("SCALENE", 0.2), ("NEEDLE", 0.2), ("QUAD", 0.2), ("DEGENERATE", 0.2)])
def test_single_triangles(ctx, name, dst):
    from surfacenet_amd import mesh
    v, f = getattr(ref, name)
    want = ref.sample(v, f, dst)
    _same(ctx.mesh_sample(v, f, dst), want)
    _same(mesh.sample_surface(v, f, dst), want)
    if name == "RIGHT":
        assert want[0].shape[0] == 64 and want[0][0].tolist() == [1.0 / 24.0, 1.0 / 24.0, 0.0]


def test_float32_vertices_and_quads(ctx):
    from surfacenet_amd import mesh
    v32 = ref.SCALENE[0].astype(np.float32)
    _same(mesh.sample_surface(v32, ref.SCALENE[1], DST), ref.sample(v32.astype(np.float64), ref.SCALENE[1], DST))
    v, f = ref.QUAD
    p, tri = mesh.sample_surface(v.astype(np.float32), np.asarray([[0, 1, 2, 3]]), DST)
    _same((p, tri), ref.sample(v.astype(np.float32).astype(np.float64), f, DST))
    assert (tri // 2 == 0).all() and p.shape[0] == 18


# ---- (b) the sphere mesh ---------------------------------------------------------------------------------------------------------------------
def test_sphere_mesh(ctx):
    v, f = ref.sphere_mesh()
    assert f.shape == (1452, 3)
    _same(ctx.mesh_sample(v, f, DST), ref.sphere_samples(DST))


# ---- (c) mixed sizes: many faces per workgroup, many workgroups per face -----------------------------------------------------------------------
def test_mixed_sizes(ctx):
    v, f = ref.mixed_mesh()
    want = ref.sample(v, f, DST)
    assert f.shape[0] == 5002 and want[0].shape[0] > 90000 + 5000
    got = ctx.mesh_sample(v, f, DST)
    _same(got, want)
    _same(ctx.mesh_sample(v, f, DST, device=True), want)       # (e) sn_mesh_sample_dev = sn_mesh_sample


# ---- (d) empty and short -------------------------------------------------------------------------------------------------------------------------
def _raw(ctx, v, f, dst, cap):
    """sn_mesh_sample itself: -> (status, n_points, points, tri), the arrays pre-filled with a pattern."""
    from surfacenet_amd import _lib
    v, f = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.int32)
    points, tri = np.full((cap, 3), 7.0, np.float64), np.full((cap,), 7, np.int32)
    m = ctypes.c_longlong(-5)
    rc = ctx._lib.sn_mesh_sample(ctx._h, v.shape[0], _lib.ptr(v), f.shape[0], _lib.ptr(f), dst, cap, _lib.ptr(points), _lib.ptr(tri), ctypes.byref(m))
    return rc, m.value, points, tri


def test_empty_and_short_cap(ctx):
    v, f = ref.sphere_mesh()
    want = ref.sphere_samples(DST)
    M = want[0].shape[0]
    for device in (False, True):
        p, tri = ctx.mesh_sample(v, f[:0], DST, device=device)
        assert p.shape == (0, 3) and p.dtype == np.float64 and tri.shape == (0,) and tri.dtype == np.int32
        _same(ctx.mesh_sample(v, f, DST, cap=1, device=device), want)
        _same(ctx.mesh_sample(v, f, DST, cap=M, device=device), want)
    p, tri = ctx.mesh_sample(np.zeros((0, 3)), f[:0], DST)
    assert p.shape == (0, 3) and tri.shape == (0,)
    for cap in (M - 1, 0):
        rc, m, points, tri = _raw(ctx, v, f, DST, cap)
        assert rc == -1 and m == M and (points == 7.0).all() and (tri == 7).all()
    rc, m, points, tri = _raw(ctx, v, f, DST, M + 3)
    assert rc == 0 and m == M and (points[M:] == 7.0).all() and (tri[M:] == 7).all()
    _same((points[:M], tri[:M]), want)


# ---- (e) device form -----------------------------------------------------------------------------------------------------------------------------
def test_device_form_equals_host_form(ctx):
    v, f = ref.sphere_mesh()
    a, b = ctx.mesh_sample(v, f, DST), ctx.mesh_sample(v, f, DST, device=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- (f) errors ------------------------------------------------------------------------------------------------------------------------------------
def test_errors_name_the_face_and_leave_the_context_usable(ctx):
    from surfacenet_amd import SurfaceNetHipError, _lib
    v, f = ref.mixed_mesh()
    v, f = v.copy(), f.copy()
    good = (ref.QUAD, ref.sample(*ref.QUAD, DST))

    def refused(v, f, match, dst=DST):
        for device in (False, True):
            with pytest.raises(SurfaceNetHipError, match=match):
                ctx.mesh_sample(v, f, dst, device=device)
        rc, m, points, tri = _raw(ctx, v, f, dst, 16)
        assert rc == -1 and (points == 7.0).all() and (tri == 7).all()
        _same(ctx.mesh_sample(*good[0], DST), good[1])          # the context still works

    bad = f.copy()
    bad[4000, 2] = v.shape[0]
    bad[4100, 0] = -1
    refused(v, bad, "face 4000 ")
    nan = v.copy()
    nan[f[1234, 1], 2] = np.nan
    nan[f[3000, 0], 0] = np.inf
    refused(nan, f, "face 1234[ :]")
    spare = np.concatenate([v, [[np.nan, 0.0, 0.0]]])           # a vertex no face names is not looked at
    _same(ctx.mesh_sample(spare, f, DST), ref.sample(v, f, DST))
    far = np.asarray([[0.0, 0, 0], [7000.0, 0, 0], [0, 1.0, 0]])
    refused(np.concatenate([ref.QUAD[0], far]), np.asarray([[0, 1, 2], [4, 5, 6], [0, 2, 3]]), "face 1 ")
    limit = np.asarray([[0.0, 0, 0], [32768 * 0.25, 0, 0], [1.0, 0, 0]])          # n = 32768 exactly is the last one allowed: only counted here
    rc, m, _, _ = _raw(ctx, limit, ref.RIGHT[1], 0.25, 0)
    assert rc == -1 and m == 1 << 30
    for dst in (0.0, -0.2, float("inf"), float("nan")):
        refused(*ref.QUAD, "dst", dst=dst)
    rc, m, _, _ = _raw(ctx, np.concatenate([limit, limit]), np.asarray([[0, 1, 2], [3, 4, 5]]), 0.25, 0)
    assert rc == -1 and m == 0 and "face 1" in _lib.last_error()       # M = 2^31 > 2^31 - 1: face 1 takes it there


# ---- (g) evaluation --------------------------------------------------------------------------------------------------------------------------------
MASK = np.ones((30, 30, 30), np.uint8)
BB, RES, PLANE = np.asarray([[-30.0, -30, -30], [28, 28, 28]]), 2, np.asarray([0.0, 0.0, 1.0, 20.0])


def test_mesh_compare_equals_point_compare_on_the_restatement_samples(ctx):
    from surfacenet_amd import evaluation
    v, f = ref.sphere_mesh()
    samples, _ = ref.sphere_samples(DST)
    stl = samples + [0.0, 0.0, 1.0]
    got = evaluation.mesh_compare(v, f, stl, MASK, BB, RES, PLANE, dst=DST, cSet=3)
    want = evaluation.point_compare(samples, stl, MASK, BB, RES, PLANE, dst=DST, cSet=3)
    assert set(got) == set(want) | {"n_samples", "n_faces"}
    assert got["n_samples"] == samples.shape[0] and got["n_faces"] == 1452
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert got["Qdata"].shape[0] < samples.shape[0] and got["DataInMask"].all()
    coarse = evaluation.mesh_compare(v, f, stl, MASK, BB, RES, PLANE, dst=DST, sample_dst=0.4)
    assert coarse["n_samples"] < got["n_samples"] and coarse["dst"] == DST


def test_flat_sheet_against_its_lifted_samples(ctx):
    from surfacenet_amd import evaluation
    v = np.asarray([[0.0, 0, 0], [8, 0, 0], [8, 8, 0], [0, 8, 0]])
    f = np.asarray([[0, 1, 2, 3]])
    samples, tri = ref.sample(v, np.asarray([[0, 1, 2], [0, 2, 3]]), DST)
    assert (samples[:, 2] == 0.0).all()
    base = evaluation.mesh_compare(v, f, samples + [0.0, 0.0, 1.0], MASK, BB, RES, PLANE, dst=DST)
    assert base["n_samples"] == samples.shape[0] and base["n_faces"] == 1 and 0 < base["Qdata"].shape[0] < samples.shape[0]
    assert (base["Ddata"] == 1.0).all()
    assert (base["Dstl"] >= 1.0).all() and (base["Dstl"] <= np.sqrt(1.0 + DST * DST)).all()


# ---- (h) eval_mesh_ply on a synthetic DTU folder ---------------------------------------------------------------------------------------------------
def test_eval_mesh_ply_end_to_end(ctx, tmp_path):
    sio = pytest.importorskip("scipy.io")
    from surfacenet_amd import evaluation, mesh
    v, f = ref.sphere_mesh()
    v32 = v.astype(np.float32)                                  # (exact: the vertices are float32 values)
    samples, _ = ref.sphere_samples(DST)
    stl = (samples + [0.0, 0.0, 1.0]).astype(np.float32)
    folder = pref.make_dtu_folder(str(tmp_path / "dtu"), 9, stl, dims=(31, 31, 31), bb_min=(-30, -30, -30), plane=(0.01, -0.02, 1.0, 20.0))
    mesh.save_mesh_2ply(str(tmp_path / "mesh.ply"), v32, f)
    got = evaluation.eval_mesh_ply(9, str(tmp_path / "mesh.ply"), str(tmp_path / "eval.mat"), str(tmp_path / "dtu"))
    base = evaluation.mesh_compare(v32, f, stl, folder["mask"], folder["BB"], folder["Res"], folder["plane"], dst=DST)
    assert np.array_equal(got, evaluation.eval_acc_compl(base)) and got.shape == (4,) and (got[[0, 2]] > 0).all()
    want = pref.point_compare(samples, stl, folder["mask"], folder["BB"], folder["Res"], folder["plane"])
    assert np.array_equal(got, pref.eval_acc_compl(want))
    be = sio.loadmat(str(tmp_path / "eval.mat"))["BaseEval"][0, 0]
    assert np.array_equal(be["Qdata"], base["Qdata"].T) and np.array_equal(be["Ddata"].reshape(-1), base["Ddata"])
    assert np.array_equal(be["Dstl"].reshape(-1), base["Dstl"]) and be["n_samples"].item() == samples.shape[0] and be["n_faces"].item() == 1452
