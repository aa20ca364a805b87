"""GPU (-m gpu): the surface-nets mesher (surfacenet_amd/csrc/mesh.h) through the C ABI against the numpy restatement tests/mesh_ref.py
(DESIGN.md section 4.12). The field is an exact integer, so quads, vert_cell and vert_src are compared with array_equal. vert_lattice: within 1e-9
(one float64 ulp at 2^21 is 4.7e-10; the offsets inside a dual cube agree to about 1e-15). verts_mm: within one float32 ulp of the restatement's
value (the same float64 expression rounded once; a lattice value that differs in its last bit may round to the neighbouring float32)."""
import ctypes

import numpy as np
import pytest

import mesh_ref as mr
import normals_ref as nref

pytestmark = pytest.mark.gpu
ORIGIN, RESOL = (-20.0, -20.0, -20.0), 0.4


@pytest.fixture(scope="module")
def ctx(gpu_required):
    from surfacenet_amd import runtime
    return runtime.any_context()


def _run(ctx, s, radius=2, reach=0, origin=ORIGIN, resol=RESOL, **kw):
    return ctx.mesh(*mr.scene_args(s), radius=radius, reach=reach, origin=origin, resol=resol, **kw)


def _compare(got, want):
    assert got["quads"].dtype == np.int32 and got["vert_cell"].dtype == np.int32 and got["vert_src"].dtype == np.int64
    assert got["verts_lattice"].dtype == np.float64 and got["verts_mm"].dtype == np.float32
    assert got["quads"].shape == want["quads"].shape and got["vert_cell"].shape == want["vert_cell"].shape, (got["quads"].shape, want["quads"].shape,
                                                                                                            got["vert_cell"].shape, want["vert_cell"].shape)
    assert np.array_equal(got["vert_cell"], want["vert_cell"])
    assert np.array_equal(got["quads"], want["quads"])
    assert np.array_equal(got["vert_src"], want["vert_src"])
    V = want["vert_cell"].shape[0]
    err = float(np.abs(got["verts_lattice"] - want["vert_lattice"]).max()) if V else 0.0
    ulp = np.spacing(np.maximum(np.abs(got["verts_mm"]), np.abs(want["verts_mm"])))
    mm = np.abs(got["verts_mm"].astype(np.float64) - want["verts_mm"].astype(np.float64))
    print("%d vertices, %d quads: max lattice error %.3g, max mm error %.3g" % (V, want["quads"].shape[0], err, float(mm.max()) if V else 0.0))
    assert err <= 1e-9
    assert (mm <= ulp.astype(np.float64)).all()


def _check(ctx, s, radius=2, reach=0, origin=ORIGIN, resol=RESOL, want=None):
    want = mr.mesh_ref(*mr.scene_args(s), radius=radius, reach=reach, origin=origin, resol=resol) if want is None else want
    got = _run(ctx, s, radius, reach, origin, resol)
    _compare(got, want)
    return got


# ---- small hand-built scenes ---------------------------------------------------------------------------------------------------------------------
def test_sheet_by_hand(ctx):
    s = mr.sheet_scene(z=7)
    m = _check(ctx, s, origin=(0.0, 0.0, 0.0), resol=1.0)
    assert m["quads"].shape == (25, 4) and m["verts_lattice"].shape == (36, 3)
    assert (m["verts_lattice"][:, 2] == 7.0).all() and sorted(set(m["verts_lattice"][:, 0].tolist())) == [9.5, 10.5, 11.5, 12.5, 13.5, 14.5]
    assert (mr.quad_normals(m["verts_lattice"], m["quads"])[:, 2] > 0).all()
    assert np.array_equal(m["verts_mm"], m["verts_lattice"].astype(np.float32))
    for reach, quads in ((1, 49), (2, 81)):
        assert _check(ctx, s, reach=reach)["quads"].shape[0] == quads
    for radius in (1, 3):
        _check(ctx, s, radius=radius, reach=radius)


def test_tilted_sheet_across_the_seam(ctx):
    m = _check(ctx, mr.tilted_scene())
    assert m["quads"].shape[0] == 204


def test_the_owners_normal_decides(ctx):
    cells0 = np.asarray([(x, y, 13) for x in range(4, 9) for y in range(4, 9)], np.uint8)
    cells1 = np.asarray([(x, y, 0) for x in range(4, 9) for y in range(4, 9)], np.uint8)
    up = np.tile(np.asarray([0, 0, 1], np.float32), (25, 1))
    off, ijk = nref.pack([cells0, cells1])
    a = dict(offsets=off, ijk=ijk, cube_ijk=np.asarray([[0, 0, 0], [0, 0, 1]]), mask=np.ones(50, bool), stride_vox=13, normals=np.concatenate([up, -up]))
    b = dict(a, cube_ijk=np.asarray([[0, 0, 1], [0, 0, 0]]), ijk=np.concatenate([cells1, cells0]), normals=np.concatenate([-up, up]))
    ma, mb = _check(ctx, a), _check(ctx, b)
    assert (mr.quad_normals(ma["verts_lattice"], ma["quads"])[:, 2] > 0).all() and (mr.quad_normals(mb["verts_lattice"], mb["quads"])[:, 2] < 0).all()
    assert ma["vert_src"].max() < 25 and mb["vert_src"].max() < 25
    # an unmasked first listing does not own the cell
    c = dict(a, mask=np.concatenate([np.zeros(25, bool), np.ones(25, bool)]))
    mc = _check(ctx, c)
    assert mc["vert_src"].min() >= 25 and (mr.quad_normals(mc["verts_lattice"], mc["quads"])[:, 2] < 0).all()


def test_half_full_tables_at_the_minimum_capacity(ctx):
    """32 masked voxels in 32 distinct world cells of 32 distinct 4^3 bricks (the bias of one brick keeps 7|8 and 15|16 across brick
    boundaries): the cell table and the brick table have their minimum capacity of 64 slots and are half full, the fullest the capacity rule
    allows (probes walk past taken slots, also from the last slot on to slot 0). Two cubes, so the owner search runs as well."""
    ax = (3, 4, 11, 12)
    vox = np.asarray([(i, j, k) for i in ax for j in ax for k in (3, 4)], np.uint8)
    off, ijk = nref.pack([vox[:16], vox[16:] - np.asarray([8, 0, 0], np.uint8)])                  # x = 11, 12 from a cube 8 cells along x
    up = np.tile(np.asarray([0, 0, 1], np.float32), (32, 1))
    s = dict(offsets=off, ijk=ijk, cube_ijk=np.asarray([[0, 0, 0], [1, 0, 0]], np.int64), mask=np.ones(32, bool), stride_vox=8, normals=up)
    cells = mr.oriented_cells(*mr.scene_args(s))[0]
    assert np.unique(cells, axis=0).shape[0] == 32 and np.unique((cells + 4) >> 2, axis=0).shape[0] == 32
    for radius, reach in ((1, 0), (2, 1), (3, 3)):
        assert _check(ctx, s, radius, reach)["quads"].shape[0] > 0


@pytest.mark.parametrize("place", ["split", "zero", "top"])
def test_sphere_placements(ctx, place):
    if place == "split":                                        # dealt to 4^3 cubes of stride 13: straddles cube and brick boundaries
        s = mr.sphere_scene(6, split=True)
    elif place == "zero":                                       # the shell of centre 6 is cut by the block's faces: cells at 0, samples down to -3
        s = mr.sphere_scene(6, centre=6)
        assert mr.oriented_cells(*mr.scene_args(s))[0].min() == 0
    else:                                                       # the largest cell coordinate is 2^21 - 9, the last one allowed
        s = mr.sphere_scene(6, cube_shift=(699039, 699039, 699039), stride_vox=3)
        assert mr.oriented_cells(*mr.scene_args(s))[0].max() == (1 << 21) - 9
    m = _check(ctx, s, radius=3 if place != "split" else 2, reach=1 if place != "split" else 0)
    if place == "split":
        _, count = mr.edge_counts(m["quads"])
        assert (count == 2).all() and m["quads"].shape[0] == 726 and mr.signed_volume(m["verts_lattice"], m["quads"]) > 0


# ---- the synthetic surface -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice,radius,reach", [((2, 2, 1), 1, 0), ((2, 2, 1), 1, 1), ((2, 2, 1), 2, 0), ((2, 2, 1), 2, 1), ((2, 2, 1), 3, 0),
                                                  ((2, 2, 1), 3, 1), ((3, 3, 2), 2, 0), ((6, 6, 2), 2, 0)])
def test_surface_against_restatement(ctx, lattice, radius, reach):
    s = mr.surface_mesh_scene(lattice)
    want = mr.surface_mesh_reference(lattice, radius, reach)
    m = _check(ctx, s, radius, reach, want=want)
    assert m["quads"].shape[0] > 1000
    if lattice == (2, 2, 1) and radius == 2 and reach == 0:
        assert want["n_cells"] == 2935


def test_nothing_to_mesh(ctx):
    s = mr.sheet_scene()
    for scene in (dict(s, normals=np.zeros((25, 3), np.float32)), dict(s, mask=np.zeros(25, bool)),
                  dict(s, offsets=np.zeros(2, np.int64), ijk=np.zeros((0, 3), np.uint8), mask=np.zeros(0, bool), normals=np.zeros((0, 3), np.float32)),
                  dict(offsets=np.zeros(1, np.int64), ijk=np.zeros((0, 3), np.uint8), cube_ijk=np.zeros((0, 3), np.int64), mask=np.zeros(0, bool),
                       stride_vox=13, normals=np.zeros((0, 3), np.float32))):
        for device in (False, True):
            m = _run(ctx, scene, device=device)
            assert m["quads"].shape == (0, 4) and m["verts_mm"].shape == (0, 3) and m["vert_src"].shape == (0,)
    # a speck (masked, zero normal) beside the sheet takes no part; an unmasked voxel with a NaN normal neither
    ijk = np.concatenate([s["ijk"], np.asarray([[12, 12, 8], [12, 12, 9]], np.uint8)])
    nrm = np.concatenate([s["normals"], np.zeros((1, 3), np.float32), np.full((1, 3), np.nan, np.float32)])
    extra = dict(s, offsets=np.asarray([0, 27], np.int64), ijk=ijk, mask=np.concatenate([np.ones(26, bool), [False]]), normals=nrm)
    _compare(_run(ctx, extra), mr.mesh_ref(*mr.scene_args(s), origin=ORIGIN, resol=RESOL))


def _raw(ctx, s, cap_v, cap_q, radius=2, reach=0):
    """sn_mesh itself: -> (status, n_verts, n_quads, arrays), the arrays pre-filled with a pattern."""
    from surfacenet_amd import _lib
    off = np.ascontiguousarray(s["offsets"], np.int64)
    ijk, cube = np.ascontiguousarray(s["ijk"], np.uint8), np.ascontiguousarray(s["cube_ijk"], np.uint32)
    mask, nrm = np.ascontiguousarray(s["mask"], bool).view(np.uint8), np.ascontiguousarray(s["normals"], np.float32)
    cfg = _lib.MeshCfg(radius, reach, int(s["stride_vox"]))
    cfg.origin[:] = list(ORIGIN)
    cfg.resol = RESOL
    arrs = [np.full((cap_v, 3), 7, np.float32), np.full((cap_v, 3), 7, np.float64), np.full((cap_v, 3), 7, np.int32), np.full((cap_v,), 7, np.int64),
            np.full((cap_q, 4), 7, np.int32)]
    nv, nq = ctypes.c_longlong(-5), ctypes.c_longlong(-5)
    rc = ctx._lib.sn_mesh(ctx._h, off.size - 1, ctypes.byref(cfg), _lib.ptr(off), _lib.ptr(ijk), _lib.ptr(cube), _lib.ptr(mask), _lib.ptr(nrm), cap_v, cap_q,
                          *[_lib.ptr(a) for a in arrs], ctypes.byref(nv), ctypes.byref(nq))
    return rc, nv.value, nq.value, arrs


def test_short_cap_reports_the_counts_and_writes_nothing(ctx):
    s = mr.tilted_scene()
    want = mr.mesh_ref(*mr.scene_args(s), origin=ORIGIN, resol=RESOL)
    V, Q = want["vert_cell"].shape[0], want["quads"].shape[0]
    for cap_v, cap_q in ((V - 1, Q), (V, Q - 1), (0, 0)):
        rc, nv, nq, arrs = _raw(ctx, s, cap_v, cap_q)
        assert rc == -1 and (nv, nq) == (V, Q)
        assert all((a == 7).all() for a in arrs)
    rc, nv, nq, arrs = _raw(ctx, s, V, Q)
    assert rc == 0 and (nv, nq) == (V, Q)
    _compare(dict(zip(("verts_mm", "verts_lattice", "vert_cell", "vert_src", "quads"), arrs)), want)
    # Context.mesh retries once with the exact counts
    _compare(_run(ctx, s, cap=(1, 1)), want)
    _compare(_run(ctx, s, cap=(1, 1), device=True), want)


def test_errors_leave_the_context_usable(ctx):
    from surfacenet_amd import SurfaceNetHipError
    s = mr.sheet_scene()
    want = mr.mesh_ref(*mr.scene_args(s), origin=ORIGIN, resol=RESOL)

    def refused(scene, match, **kw):
        for device in (False, True):
            with pytest.raises(SurfaceNetHipError, match=match):
                _run(ctx, scene, device=device, **kw)
        _compare(_run(ctx, s), want)                            # the context still works

    refused(s, "radius", radius=0)
    refused(s, "radius", radius=4)
    refused(s, "reach", radius=2, reach=3)
    refused(dict(s, stride_vox=0), "stride_vox")
    top = (1 << 21) - 8                                         # the sheet's z = 7 lands on cell 2^21 - 8: cell + 8 = 2^21
    refused(dict(s, cube_ijk=np.asarray([[0, 0, top - 7]]), stride_vox=1), "2\\^21")
    _check(ctx, dict(s, cube_ijk=np.asarray([[0, 0, top - 8]]), stride_vox=1))      # one cell lower is the last one allowed
    bad = s["normals"].copy()
    bad[3, 1] = np.nan
    refused(dict(s, normals=bad), "normal")
    bad[3, 1] = 2.5
    refused(dict(s, normals=bad), "normal")
    with pytest.raises(SurfaceNetHipError, match="offsets"):     # the device form checks the table in a kernel
        _run(ctx, dict(s, offsets=np.asarray([1, 25], np.int64)), device=True)
    with pytest.raises(SurfaceNetHipError, match="offsets"):
        _run(ctx, dict(s, offsets=np.asarray([1, 25], np.int64)))
    two = dict(s, offsets=np.asarray([0, 30, 25], np.int64), cube_ijk=np.zeros((2, 3), np.int64))      # decreases
    for device in (False, True):
        with pytest.raises(SurfaceNetHipError, match="offsets"):
            _run(ctx, two, device=device)
    _compare(_run(ctx, s), want)


def test_runs_repeat_device_form_and_workspace_growth(ctx):
    small, large = mr.tilted_scene(), mr.surface_mesh_scene((3, 3, 2))
    want_small = mr.mesh_ref(*mr.scene_args(small), origin=ORIGIN, resol=RESOL)
    want_large = mr.surface_mesh_reference((3, 3, 2), 2, 0)
    a = _run(ctx, small)
    b = _run(ctx, large)
    c = _run(ctx, small)                                        # small, large, small in one context: the workspaces grow and are reused
    _compare(a, want_small)
    _compare(b, want_large)
    b2, bd = _run(ctx, large), _run(ctx, large, device=True)
    for k in ("verts_mm", "verts_lattice", "vert_cell", "vert_src", "quads"):
        assert a[k].tobytes() == c[k].tobytes(), k
        assert b[k].tobytes() == b2[k].tobytes(), k             # two runs are bit-identical
        assert b[k].tobytes() == bd[k].tobytes(), k             # sn_mesh_dev = sn_mesh bit for bit


# ---- through the pipeline ------------------------------------------------------------------------------------------------------------------------
def test_scene_postpass_mesh_and_ply(ctx, tmp_path):
    from surfacenet_amd import mesh, reconstruct
    s = nref.surface_scene((2, 2, 1))
    d = s["lists"]
    out = dict(prediction_list=d["prediction_list"], vxl_ijk_list=d["vxl_ijk_list"], rayPooling_votes_list=d["rayPooling_votes_list"],
               cube_ijk_np=d["cube_ijk_np"], param_np=s["param"], viewPair_np=s["viewPair"], rgb_list=d["rgb_list"])
    cams = s["cameraTs"]
    kw = dict(tau=0.7, gamma=0.5, N_refine_iter=2, cameraTs_np=cams)
    prefix = str(tmp_path / "scene_")
    post = reconstruct.scene_postpass(out, 32, 26, 2, mesh=True, mesh_ply_prefix=prefix, **kw)
    plain = reconstruct.scene_postpass(out, 32, 26, 2, **kw)
    assert set(post) - set(plain) == {"fixThresh_mesh", "adapt_mesh"}
    with pytest.raises(ValueError, match="cameraTs_np"):
        reconstruct.scene_postpass(out, 32, 26, 2, mesh=True)
    off, ijk = nref.pack(d["vxl_ijk_list"])
    for name in ("fixThresh", "adapt"):
        masks, nl = post[name + "_denoised_list"], post[name + "_normal_list"]
        assert all(np.array_equal(a, b) for a, b in zip(masks, plain[name + "_denoised_list"]))
        want = mesh.extract_mesh(d["cube_ijk_np"], d["vxl_ijk_list"], masks, nl, s["param"], 13)
        got = post[name + "_mesh"]
        assert set(got) == {"vertices", "quads", "vert_src", "vert_lattice"} and got["quads"].shape[0] > 1000
        for k in want:
            assert np.array_equal(got[k], want[k]), (name, k)
        origin, resol = mesh.lattice_origin(d["cube_ijk_np"], s["param"], 13)
        r = mr.mesh_ref(off, ijk, d["cube_ijk_np"], np.concatenate(masks), 13, np.concatenate(nl), origin=origin, resol=resol)
        _compare(dict(verts_mm=got["vertices"], verts_lattice=got["vert_lattice"], vert_cell=r["vert_cell"], vert_src=got["vert_src"], quads=got["quads"]), r)
        header, verts, faces = mr.parse_ply(prefix + name + "_mesh.ply")
        assert "element vertex %d" % got["vertices"].shape[0] in header and "element face %d" % got["quads"].shape[0] in header
        assert np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), got["vertices"])
        assert np.array_equal(np.stack([verts["nx"], verts["ny"], verts["nz"]], 1), np.concatenate(nl)[got["vert_src"]])
        assert np.array_equal(np.stack([verts["red"], verts["green"], verts["blue"]], 1), np.concatenate(d["rgb_list"])[got["vert_src"]])
        assert np.array_equal(np.asarray(faces), got["quads"])
    # reach 1: faces beyond the oriented cells; a vertex with no oriented cell beside it is written without normal and colour
    far = reconstruct.scene_postpass(out, 32, 26, 2, mesh=True, mesh_reach=1, mesh_ply_prefix=str(tmp_path / "far_"), **kw)["adapt_mesh"]
    assert far["quads"].shape[0] > post["adapt_mesh"]["quads"].shape[0]
    header, verts, faces = mr.parse_ply(str(tmp_path / "far_adapt_mesh.ply"))
    none = far["vert_src"] < 0
    want_n = np.where(none[:, None], 0, np.concatenate(post["adapt_normal_list"])[far["vert_src"]])
    want_c = np.where(none[:, None], 0, np.concatenate(d["rgb_list"])[far["vert_src"]])
    assert np.array_equal(np.stack([verts["nx"], verts["ny"], verts["nz"]], 1), want_n.astype(np.float32))
    assert np.array_equal(np.stack([verts["red"], verts["green"], verts["blue"]], 1), want_c.astype(np.uint8))
    assert np.array_equal(np.asarray(faces), far["quads"])
