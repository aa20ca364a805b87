"""GPU (-m gpu): oriented normals and de-duplication of the output cloud (surfacenet_amd/csrc/normals.h) through the C ABI, against the numpy
restatement tests/normals_ref.py: window moments and unique owners bit for bit, normals within one float32 rounding.

Tolerance of a normal's component: 2e-7. One float32 rounding of a component below 1 is at most 2^-25 = 3e-8 and a float64 eigen-solve adds about
1e-15 over the relative eigen-gap (>= 1e-3 on the compared voxels); a solver carried in float32 would miss by at least 6e-8 / 0.064 = 9e-7 at the
smallest gap of these scenes."""
import numpy as np
import pytest

import normals_ref as ref

pytestmark = pytest.mark.gpu
TOL = 2e-7


@pytest.fixture(scope="module")
def ctx(gpu_required):
    from surfacenet_amd import runtime
    return runtime.any_context()


def _run(ctx, s, radius=2, min_neighbours=6):
    return ctx.normals(*ref.scene_args(s), radius=radius, min_neighbours=min_neighbours, return_moments=True)


def _unique(ctx, s):
    return ctx.unique_voxels(s["offsets"], s["ijk"], s["cube_ijk"], s["mask"], s["stride_vox"])


def _check(ctx, s, r, radius=2, min_neighbours=6, min_compared=0.0):
    """Everything the contract promises, against the restatement's result r."""
    nrm, mom = _run(ctx, s, radius, min_neighbours)
    assert mom.dtype == np.int32 and np.array_equal(mom, r["moments"])
    assert nrm.dtype == np.float32 and nrm.shape == (s["mask"].size, 3) and np.isfinite(nrm).all()
    cmp_ = r["comparable"]
    n_masked = int(s["mask"].sum())
    frac = cmp_.sum() / max(n_masked, 1)
    err = float(np.abs(nrm[cmp_].astype(np.float64) - r["normals"][cmp_].astype(np.float64)).max()) if cmp_.any() else 0.0
    min_cos = float(np.abs(r["cos"][cmp_]).min()) if cmp_.any() else 1.0
    length = np.sqrt((nrm.astype(np.float64) ** 2).sum(1))
    len_err = float(np.abs(length[r["solved"]] - 1).max()) if r["solved"].any() else 0.0
    print("radius %d: %d masked, compared %.4f, max component error %.3g, min |cos| %.3g, max | |n| - 1 | %.3g"
          % (radius, n_masked, frac, err, min_cos, len_err))
    assert frac >= min_compared
    assert min_cos >= 1e-6                                     # no compared voxel sees its cameras edge-on: the sign is decided
    assert err <= TOL
    assert len_err <= TOL
    assert not nrm[~r["solved"]].any()                         # unmasked, or fewer than min_neighbours cells: exactly zero
    return nrm, mom


# ---- small hand-built scenes ---------------------------------------------------------------------------------------------------------------------
def test_one_cube_sheet_is_exact(ctx):
    s = ref.hand_scene([[0, 0, 0]], ref.sheet_5x5(z=7))
    r = ref.normals_ref(*ref.scene_args(s))
    nrm, mom = _check(ctx, s, r, min_compared=1.0)
    assert mom[12].tolist() == [25, 0, 0, 0, 50, 0, 0, 50, 0, 0] and mom[0].tolist() == [9, 9, 9, 0, 15, 9, 0, 15, 0, 0]
    assert np.array_equal(nrm, np.tile(np.asarray([0, 0, 1], np.float32), (25, 1)))
    assert _unique(ctx, s).all()
    for radius in (1, 3):
        _check(ctx, s, ref.normals_ref(*ref.scene_args(s), radius=radius), radius=radius)
    # moments alone need neither cameras nor cube geometry
    only = ctx.normals(s["offsets"], s["ijk"], s["cube_ijk"], s["mask"], s["stride_vox"], return_normals=False, return_moments=True)
    assert np.array_equal(only, mom)


def test_tilted_sheet_across_the_seam(ctx):
    cube_ijk, lists = ref.tilted_sheet_two_cubes()
    s = ref.hand_scene(cube_ijk, lists)
    r = ref.normals_ref(*ref.scene_args(s))
    nrm, mom = _check(ctx, s, r, min_compared=1.0)
    assert np.abs(nrm - (np.asarray([1.0, 0.0, 1.0]) / np.sqrt(2.0))).max() <= TOL
    n0 = int(s["offsets"][1])
    own = ref.moments_ref(s["offsets"][:2], s["ijk"][:n0], cube_ijk[:1], s["mask"][:n0], 13, 2)
    rim = np.nonzero(s["ijk"][:n0, 0] == 17)[0]
    assert (mom[rim, 0] > own[rim, 0]).all()                   # the rim's windows hold the other cube's voxels
    assert _unique(ctx, s).all()


def test_repeated_voxels_count_once_and_unique_keeps_the_first(ctx):
    sheet = [(i, j, 3) for i in range(11, 16) for j in range(1, 6)]
    # (14,3,3) of cube 0 is listed twice more; cube (1,0,0) lists the same world cells again (local x = x - 13, for x >= 13)
    lists = [np.asarray(sheet + [(14, 3, 3), (14, 3, 3)], np.uint8), np.asarray([(i - 13, j, k) for i, j, k in sheet if i >= 13], np.uint8)]
    s = ref.hand_scene([[0, 0, 0], [1, 0, 0]], lists)
    r = ref.normals_ref(*ref.scene_args(s))
    nrm, mom = _check(ctx, s, r, min_compared=1.0)
    centre = sheet.index((13, 3, 3))
    assert mom[centre, 0] == 25                                # 25 cells, though 42 voxels are listed
    keep = _unique(ctx, s)
    assert np.array_equal(keep, ref.unique_ref(s["offsets"], s["ijk"], s["cube_ijk"], s["mask"], 13))
    assert keep[:25].all() and not keep[25:].any()
    m = s["mask"].copy()
    m[sheet.index((14, 3, 3))] = False                         # its first listing unmasked: the next listing of the cell owns it
    s2 = dict(s, mask=m)
    keep2 = _unique(ctx, s2)
    assert np.array_equal(keep2, ref.unique_ref(s["offsets"], s["ijk"], s["cube_ijk"], m, 13)) and keep2[25] and not keep2[26]
    _check(ctx, s2, ref.normals_ref(*ref.scene_args(s2)), min_compared=1.0)


@pytest.mark.parametrize("cubes", [1, 2])
def test_half_full_tables_at_the_minimum_capacity(ctx, cubes):
    """32 masked voxels in 32 distinct world cells of 32 distinct 4^3 bricks: the brick table (normals) and the cell table (unique voxels)
    have their minimum capacity of 64 slots and are half full, the fullest the capacity rule allows (probes walk past taken slots, also from
    the last slot on to slot 0). Coordinates 3|4 and 11|12 are neighbours across a brick boundary, so the windows are not empty."""
    ax = (3, 4, 11, 12)
    vox = np.asarray([(i, j, k) for i in ax for j in ax for k in (3, 4)], np.uint8)
    lists = [vox] if cubes == 1 else [vox[:16], vox[16:] - np.asarray([8, 0, 0], np.uint8)]      # x = 11, 12 from a cube 8 cells along x
    s = ref.hand_scene([[0, 0, 0], [1, 0, 0]][:cubes], lists, stride_vox=8)
    g = ref.world_cells(s["offsets"], s["ijk"], s["cube_ijk"], 8)
    assert s["mask"].all() and np.unique(g, axis=0).shape[0] == 32 and np.unique(g >> 2, axis=0).shape[0] == 32
    for radius in (1, 2, 3):
        r = ref.normals_ref(*ref.scene_args(s), radius=radius, min_neighbours=4)
        nrm, mom = _run(ctx, s, radius, 4)
        assert np.array_equal(mom, r["moments"]) and mom[:, 0].min() >= 4
        assert np.abs(nrm[r["comparable"]].astype(np.float64) - r["normals"][r["comparable"]].astype(np.float64)).max(initial=0.0) <= TOL
        assert not nrm[~r["solved"]].any()
    assert np.array_equal(_unique(ctx, s), ref.unique_ref(s["offsets"], s["ijk"], s["cube_ijk"], s["mask"], 8)) and _unique(ctx, s).all()


def test_speck_empty_cube_unmasked_cube_and_no_voxels(ctx):
    lists = ref.sheet_5x5(z=7) + [np.zeros((0, 3), np.uint8), np.asarray([(20, 20, 20)], np.uint8), ref.sheet_5x5(z=9)[0]]
    s = ref.hand_scene([[0, 0, 0], [1, 1, 0], [4, 4, 4], [0, 0, 1]], lists)
    s["mask"][s["offsets"][3]:] = False                        # the last cube has no masked voxel
    r = ref.normals_ref(*ref.scene_args(s))
    nrm, mom = _check(ctx, s, r)
    speck = int(s["offsets"][2])
    assert mom[speck].tolist() == [1] + [0] * 9 and not nrm[speck].any()
    assert not mom[s["offsets"][3]:].any()
    keep = _unique(ctx, s)
    assert np.array_equal(keep, s["mask"])
    # no voxel at all, and no cube at all
    e = ref.hand_scene([[0, 0, 0], [1, 0, 0]], [np.zeros((0, 3), np.uint8)] * 2)
    nrm, mom = _run(ctx, e)
    assert nrm.shape == (0, 3) and mom.shape == (0, 10) and _unique(ctx, e).shape == (0,)
    z = ref.hand_scene(np.zeros((0, 3)), [])
    nrm, mom = _run(ctx, z)
    assert nrm.shape == (0, 3) and mom.shape == (0, 10) and _unique(ctx, z).shape == (0,)


def _far_scene(radius, x_far):
    """One voxel at world cell (0,0,0), one at (x_far,0,0), in two cubes."""
    cx = x_far // 13 - 1
    lists = [np.asarray([(0, 0, 0)], np.uint8), np.asarray([(x_far - 13 * cx, 0, 0)], np.uint8)]
    s = ref.hand_scene([[0, 0, 0], [cx, 0, 0]], lists)
    assert ref.world_cells(s["offsets"], s["ijk"], s["cube_ijk"], 13)[:, 0].tolist() == [0, x_far]
    return s


@pytest.mark.parametrize("radius", [1, 2])
def test_both_ends_of_the_key_range(ctx, radius):
    """Cell 0 and cell 2^21 - 1 - r on one axis, the two ends of what the keys hold, are not neighbours: windows that reach below zero miss."""
    s = _far_scene(radius, 2 ** 21 - 1 - radius)
    nrm, mom = _run(ctx, s, radius=radius, min_neighbours=1)
    assert mom.tolist() == [[1] + [0] * 9] * 2
    assert np.array_equal(mom, ref.moments_ref(s["offsets"], s["ijk"], s["cube_ijk"], s["mask"], 13, radius))
    assert np.isfinite(nrm).all() and np.allclose((nrm.astype(np.float64) ** 2).sum(1), 1.0, atol=4e-7, rtol=0)      # degenerate: any unit vector
    assert _unique(ctx, s).all()


def test_bad_cells_and_view_indices_are_rejected(ctx):
    import surfacenet_amd
    s = _far_scene(2, 2 ** 21 - 2)                             # g + radius = 2^21
    with pytest.raises(surfacenet_amd.SurfaceNetHipError, match="2\\^21"):
        _run(ctx, s, radius=2)
    assert _run(ctx, s, radius=1)[1].tolist() == [[1] + [0] * 9] * 2      # g + 1 = 2^21 - 1: the last cell the keys hold
    s = _far_scene(2, 2 ** 21)
    with pytest.raises(surfacenet_amd.SurfaceNetHipError, match="2\\^21"):
        _unique(ctx, s)
    unmasked = dict(s, mask=np.asarray([True, False]))         # a cell past the range that no masked voxel occupies is no cell
    assert _unique(ctx, unmasked).tolist() == [True, False]
    good = ref.hand_scene([[0, 0, 0]], ref.sheet_5x5())
    bad = dict(good, view_idx=good["view_idx"].copy())
    bad["view_idx"][0, 2] = good["cameraTs"].shape[0]          # == V
    with pytest.raises(surfacenet_amd.SurfaceNetHipError, match="view index"):
        _run(ctx, bad)
    bad["view_idx"][0, 2] = -1
    with pytest.raises(surfacenet_amd.SurfaceNetHipError, match="view index"):
        _run(ctx, bad)
    for radius in (0, 4):
        with pytest.raises(surfacenet_amd.SurfaceNetHipError, match="radius"):
            _run(ctx, good, radius=radius)
    with pytest.raises(surfacenet_amd.SurfaceNetHipError, match="stride_vox"):
        ctx.unique_voxels(good["offsets"], good["ijk"], good["cube_ijk"], good["mask"], 0)
    two = ref.hand_scene([[0, 0, 0], [1, 0, 0]], ref.sheet_5x5() * 2)
    two["cube_resol"][1] = 0.8
    with pytest.raises(surfacenet_amd.SurfaceNetHipError, match="resol"):
        _run(ctx, two)
    _check(ctx, good, ref.normals_ref(*ref.scene_args(good)), min_compared=1.0)       # the context still works


def test_cameras_below_flip_every_sign_and_nothing_else(ctx):
    cube_ijk, lists = ref.tilted_sheet_two_cubes()
    s = ref.hand_scene(cube_ijk, lists)
    up, mom_up = _run(ctx, s)
    down, mom_down = _run(ctx, dict(s, cameraTs=ref.cameras_above(4, sign=-1.0)))
    assert np.array_equal(mom_up, mom_down) and np.array_equal(down, -up) and (up[:, 2] > 0).all()


def test_per_cube_views_orient_a_shared_cell_per_cube(ctx):
    sheet = ref.sheet_5x5(z=7)[0]
    s = ref.hand_scene([[0, 0, 0], [0, 0, 0]], [sheet, sheet])                  # the same cells, listed by two cubes
    s["cameraTs"] = np.concatenate([ref.cameras_above(2), ref.cameras_above(2, sign=-1.0)])
    s["view_idx"] = np.asarray([[0, 1, 0, 1], [2, 3, 3, 2]], np.int32)           # cube 0 was seen from above, cube 1 from below
    nrm, mom = _check(ctx, s, ref.normals_ref(*ref.scene_args(s)), min_compared=1.0)
    assert np.array_equal(mom[:25], mom[25:]) and (nrm[:25, 2] == 1).all() and (nrm[25:, 2] == -1).all()
    keep = _unique(ctx, s)
    assert keep[:25].all() and not keep[25:].any()


# ---- synthetic.sparse_surface -----------------------------------------------------------------------------------------------------------------------
SURFACES = [((2, 2, 1), 26, (0, 0, 0), "above", 1), ((2, 2, 1), 26, (0, 0, 0), "above", 2), ((2, 2, 1), 26, (0, 0, 0), "above", 3),
            ((3, 3, 2), 26, (0, 0, 0), "above", 1), ((3, 3, 2), 26, (0, 0, 0), "above", 2), ((3, 3, 2), 26, (0, 0, 0), "above", 3),
            ((2, 1, 1), 52, (0, 0, 0), "above", 2),
            ((2, 2, 1), 26, (70000, 3, 150000), "above", 2),                    # keys near the top of the range
            ((6, 6, 2), 26, (0, 0, 0), "above", 2),                              # 99,131 voxels: several hundred workgroups
            ((2, 2, 1), 26, (0, 0, 0), "side", 2), ((3, 3, 2), 26, (0, 0, 0), "side", 2)]


@pytest.mark.parametrize("lattice,Dc,shift,cams,radius", SURFACES)
def test_surface_against_restatement(ctx, lattice, Dc, shift, cams, radius):
    """Moments and unique owners bit for bit, normals within TOL on the voxels with a decided eigenvector (at least 95 % of the masked ones), unit
    length wherever a normal is due, zero elsewhere. The (3,3,2) lattice is the one whose moments need voxels of other cubes in most windows."""
    s = ref.surface_scene(lattice, Dc, shift, cams)
    r = ref.surface_reference(lattice, Dc, shift, cams, radius)
    _check(ctx, s, r, radius=radius, min_compared=0.95)
    keep = _unique(ctx, s)
    assert np.array_equal(keep, r["unique"])
    cells = ref.world_cells(s["offsets"], s["ijk"], s["cube_ijk"], s["stride_vox"])[s["mask"]]
    assert int(keep.sum()) == np.unique(cells, axis=0).shape[0] < int(s["mask"].sum())


def test_min_neighbours_is_an_integer_threshold(ctx):
    s = ref.surface_scene((2, 2, 1))
    r = ref.normals_ref(*ref.scene_args(s), min_neighbours=12, mom=ref.surface_reference((2, 2, 1))["moments"])
    assert r["solved"].sum() < ref.surface_reference((2, 2, 1))["solved"].sum()
    _check(ctx, s, r, min_neighbours=12)


# ---- through the pipeline ----------------------------------------------------------------------------------------------------------------------------
def test_scene_postpass_lists_ply_and_device_entry(ctx, tmp_path):
    import ctypes
    from surfacenet_amd import _lib, normals, reconstruct, sparseCubes
    s = ref.surface_scene((3, 3, 2))
    d = s["lists"]
    out = dict(prediction_list=d["prediction_list"], vxl_ijk_list=d["vxl_ijk_list"], rayPooling_votes_list=d["rayPooling_votes_list"],
               cube_ijk_np=d["cube_ijk_np"], param_np=s["param"], viewPair_np=s["viewPair"])
    cams = s["cameraTs"]
    post = reconstruct.scene_postpass(out, 32, 26, 2, tau=0.7, gamma=0.5, N_refine_iter=2, cameraTs_np=cams, unique=True)
    plain = reconstruct.scene_postpass(out, 32, 26, 2, tau=0.7, gamma=0.5, N_refine_iter=2)
    assert set(post) - set(plain) == {"fixThresh_normal_list", "adapt_normal_list", "fixThresh_unique_list", "adapt_unique_list"}
    n = len(d["vxl_ijk_list"])
    for name in ("fixThresh", "adapt"):
        masks = post[name + "_denoised_list"]
        assert all(np.array_equal(a, b) for a, b in zip(masks, plain[name + "_denoised_list"]))
        nl, ul = post[name + "_normal_list"], post[name + "_unique_list"]
        assert len(nl) == len(ul) == n
        want_n = normals.estimate_normals(d["cube_ijk_np"], d["vxl_ijk_list"], masks, s["param"], s["viewPair"], cams, 13)
        want_u = normals.unique_voxels(d["cube_ijk_np"], d["vxl_ijk_list"], masks, 13)
        for i in range(n):
            assert nl[i].dtype == np.float32 and nl[i].shape == (len(d["vxl_ijk_list"][i]), 3) and np.array_equal(nl[i], want_n[i]), i
            assert ul[i].dtype == bool and ul[i].shape == masks[i].shape and np.array_equal(ul[i], want_u[i]), i
            assert not (ul[i] & ~masks[i]).any()
    # the PLY of the de-duplicated cloud with normals
    masks, nl, ul = post["adapt_denoised_list"], post["adapt_normal_list"], post["adapt_unique_list"]
    path = str(tmp_path / "cloud.ply")
    sparseCubes.save_sparseCubes_2ply(ul, d["vxl_ijk_list"], d["rgb_list"], s["param"], path, normal_list=nl)
    blob = open(path, "rb").read()
    header = blob[:blob.index(b"end_header\n")].decode("ascii").splitlines()
    off, ijk = ref.pack(d["vxl_ijk_list"])
    flat = np.concatenate(masks)
    n_cells = np.unique(ref.world_cells(off, ijk, d["cube_ijk_np"], 13)[flat], axis=0).shape[0]
    assert "element vertex %d" % n_cells in header and 0 < n_cells < int(flat.sum())
    assert [h for h in header if h.startswith("property")] == ["property float x", "property float y", "property float z", "property float nx",
                                                              "property float ny", "property float nz", "property uchar red",
                                                              "property uchar green", "property uchar blue"]
    body = np.frombuffer(blob[blob.index(b"end_header\n") + 11:], dtype=np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)]))
    assert body.shape == (n_cells,) and np.array_equal(body["n"], np.concatenate(nl)[np.concatenate(ul)])
    # sn_normals_dev / sn_unique_voxels_dev on device arrays = the host entries, bit for bit; a second run too
    host_n, host_m = _run(ctx, s)
    again_n, again_m = _run(ctx, s)
    assert np.array_equal(host_n.view(np.uint32), again_n.view(np.uint32)) and np.array_equal(host_m, again_m)
    host_u = _unique(ctx, s)
    assert np.array_equal(host_u, _unique(ctx, s))
    T, K, V = int(s["offsets"][-1]), s["view_idx"].shape[1], cams.shape[0]
    bufs = []

    def up(a):
        a = np.ascontiguousarray(a)
        p = ctx.dev_alloc(max(a.nbytes, 1))
        bufs.append(p)
        ctx.h2d(p, a)
        return p
    try:
        d_in = [up(s["offsets"]), up(s["ijk"]), up(s["cube_ijk"].astype(np.uint32)), up(s["mask"].view(np.uint8))]
        d_geo = [up(s["cube_xyz"]), up(s["cube_resol"]), up(s["view_idx"]), up(cams)]
        d_n, d_m, d_u = up(np.full((T, 3), 7, np.float32)), up(np.full((T, 10), 7, np.int32)), up(np.full(T, 7, np.uint8))
        cfg = _lib.NormalsCfg(2, 6, 13, V, K)
        for _ in range(2):
            _lib.check(ctx._lib.sn_normals_dev(ctx._h, len(s["cube_ijk"]), ctypes.byref(cfg), T, *(d_in + d_geo + [d_n, d_m])))
            got_n, got_m = np.empty((T, 3), np.float32), np.empty((T, 10), np.int32)
            ctx.d2h(got_n, d_n)
            ctx.d2h(got_m, d_m)
            assert np.array_equal(got_n.view(np.uint32), host_n.view(np.uint32)) and np.array_equal(got_m, host_m)
        _lib.check(ctx._lib.sn_unique_voxels_dev(ctx._h, len(s["cube_ijk"]), 13, T, *(d_in + [d_u])))
        got_u = np.empty(T, np.uint8)
        ctx.d2h(got_u, d_u)
        assert np.array_equal(got_u.view(bool), host_u)
        bad = s["offsets"].copy()
        bad[-1] += 1                                               # the table promises one voxel more than `total`
        d_bad = up(bad)
        assert ctx._lib.sn_unique_voxels_dev(ctx._h, len(s["cube_ijk"]), 13, T, d_bad, *(d_in[1:] + [d_u])) == -1
        assert "offsets table" in _lib.last_error()
    finally:
        for p in bufs:
            ctx.dev_free(p)
