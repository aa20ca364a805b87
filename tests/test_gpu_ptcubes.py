"""GPU (-m gpu): the point-seeded cube list (surfacenet_amd/csrc/ptcubes.h) through surfacenet_amd.scene: bit-identical to goldens recorded
from the reference's scene.quantizePts2Cubes (tests/golden/ptcubes_cases.npz), to the numpy restatement (tests/ptcubes_ref.py) on clouds
too large to commit, on both forms of the cell set (occupancy bitmap / hash set + sort), host and device entries, the fused sparse-list
entry, the index limit, and a seeded cube set through reconstruct_scene and scene_postpass. Every comparison is array_equal."""
import functools

import numpy as np
import pytest

import ptcubes_ref as ref

pytestmark = pytest.mark.gpu
CASES = ref.golden_cases()
RESOL = np.float32(0.4)                                    # params.py:168 gives the resolution as float32


@pytest.fixture(scope="module")
def sn(gpu_required):
    from surfacenet_amd import runtime, scene, sparseCubes, synthetic
    yield dict(runtime=runtime, scene=scene, sparseCubes=sparseCubes, synthetic=synthetic)
    runtime.reset()


def _same(got, want):
    (cubes, side), (wcubes, wside) = got, want
    assert cubes.dtype == ref.CUBE_DTYPE and cubes.shape == wcubes.shape
    assert np.array_equal(cubes["ijk"], wcubes["ijk"])                                        # also the row order
    assert np.array_equal(cubes["xyz"], wcubes["xyz"]) and np.array_equal(cubes["resol"], wcubes["resol"])
    assert type(side) is type(wside) and side == wside


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_equals_reference_goldens(sn, case):
    name, kw, ijk, xyz, dmm = case
    cubes, side = sn["scene"].quantizePts2Cubes(**kw)
    assert cubes.dtype == ref.CUBE_DTYPE
    assert np.array_equal(cubes["ijk"], ijk) and np.array_equal(cubes["xyz"], xyz)
    assert np.all(cubes["resol"] == np.float32(kw["resol"]))
    assert np.asarray(side).dtype == dmm.dtype and np.asarray(side) == dmm


@functools.lru_cache(maxsize=4)
def _cloud(n, spatial):
    return ref.wavy_cloud(n, seed=n % 97, spatial=spatial)


@pytest.mark.parametrize("spatial", [True, False], ids=["spatial", "permuted"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [100000, 3000000])
def test_equals_restatement_at_scale(sn, n, dtype, spatial):
    pts = _cloud(n, spatial).astype(dtype)
    kw = dict(resol=RESOL, cube_D=32, cube_Dcenter=26, cube_overlapping_ratio=0.5, BB=ref.SCAN9_BB)
    _same(sn["scene"].quantizePts2Cubes(pts, **kw), ref.quantizePts2Cubes(pts, **kw))


def _two_sheets(dtype):
    """Two copies of a sheet 4000 mm apart on every axis: about 770 strides per axis, more cells than the occupancy bitmap is used for, and
    enough distinct cells for the sort to leave its in-LDS tiles."""
    a = _cloud(100000, True)
    return np.concatenate([a, a + 4000.0]).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_cell_extents_beyond_the_dense_form(sn, dtype):
    pts = _two_sheets(dtype)
    kw = dict(resol=RESOL, cube_D=32, cube_Dcenter=26, cube_overlapping_ratio=0.5)
    want = ref.quantizePts2Cubes(pts, **kw)
    ext = want[0]["ijk"].max(axis=0).astype(np.int64) + 1
    assert ext.prod() > (1 << 27) and want[0].shape[0] > 2048
    _same(sn["scene"].quantizePts2Cubes(pts, **kw), want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_hash_set_half_full_at_its_smallest(sn, dtype):
    """512 points whose cells and diagonal cells are all distinct, too far apart for the occupancy bitmap: 1,024 keys in the hash set's minimum
    of 2,048 slots, the fullest the capacity rule allows (probes walk past taken slots, also from the last slot on to slot 0)."""
    kw = dict(resol=RESOL, cube_D=32, cube_Dcenter=26, cube_overlapping_ratio=0.5)
    stride = float(sn["scene"]._plan(np.dtype(dtype), RESOL, 32, 26, 0.5, None)["stride_q"])
    i = np.arange(512, dtype=np.float64)
    along = np.where(i == 0, 0.0, (3 * i + 0.5) * stride)                                      # cell 3 i of the space diagonal (the first point is the shift)
    pts = np.repeat(along[np.random.RandomState(5).permutation(512), None], 3, axis=1).astype(dtype)
    want = ref.quantizePts2Cubes(pts, **kw)
    ext = want[0]["ijk"].max(axis=0).astype(np.int64) + 1
    assert ext.prod() > (1 << 27) and want[0].shape[0] == 1024
    _same(sn["scene"].quantizePts2Cubes(pts, **kw), want)


@pytest.mark.parametrize("far", [False, True], ids=["dense", "hashed"])
def test_dev_entry_and_short_outputs_equal_host_entry(sn, far):
    scene = sn["scene"]
    ctx = sn["runtime"].any_context()
    pts = _two_sheets(np.float32) if far else _cloud(100000, False).astype(np.float32)
    p = scene._plan(pts.dtype, RESOL, 32, 26, 0.5, ref.SCAN9_BB if not far else None)
    args = (p["stride_q"], p["stride_xyz"], p["half"], p["compute_f64"])
    ijk, xyz = ctx.ptcubes(pts, *args, box=p["box"])
    assert ijk.shape[0] > 1000
    d = ctx.upload(pts)
    try:
        ijk_d, xyz_d = ctx.ptcubes_dev(pts.shape[0], d, False, *args, box=p["box"])
        ijk_r, xyz_r = ctx.ptcubes_dev(pts.shape[0], d, False, *args, box=p["box"], cap=7)      # too short: the needed length comes back, one retry
    finally:
        ctx.dev_free(d)
    ijk_s, xyz_s = ctx.ptcubes(pts, *args, box=p["box"], cap=0)
    for a, b in ((ijk_d, xyz_d), (ijk_r, xyz_r), (ijk_s, xyz_s)):
        assert np.array_equal(a, ijk) and np.array_equal(b, xyz)


@pytest.mark.parametrize("with_bb", [False, True], ids=["noBB", "BB"])
@pytest.mark.parametrize("resol", [0.2, np.float32(0.2), np.float64(0.2)], ids=["py", "f32", "f64"])
def test_cubes_from_sparse_equals_quantize_of_sparse_xyz(sn, resol, with_bb):
    scene, sc = sn["scene"], sn["sparseCubes"]
    s = sn["synthetic"].sparse_surface(lattice=(5, 4, 3), Dc=26, seed=4)
    masks = [p >= np.float16(0.75) for p in s["prediction_list"]]
    masks[3][:] = False                                                                    # a cube with nothing masked
    pts = sc.sparse_xyz(masks, s["vxl_ijk_list"], s["param_np"])
    assert pts.dtype == np.float32 and 1000 < pts.shape[0] < sum(len(m) for m in masks)
    BB = np.array([[-18.0, -2.0], [-19.0, 0.5], [-16.0, -6.0]]) if with_bb else None
    kw = dict(resol=resol, cube_D=32, cube_Dcenter=26, cube_overlapping_ratio=0.5, BB=BB)
    want = scene.quantizePts2Cubes(pts, **kw)
    _same(want, ref.quantizePts2Cubes(pts, **kw))
    _same(scene.cubes_from_sparse(masks, s["vxl_ijk_list"], s["param_np"], **kw), want)
    if with_bb:
        assert want[0].shape[0] < scene.quantizePts2Cubes(pts, **dict(kw, BB=None))[0].shape[0]


def test_index_limit_and_empty_box(sn):
    from surfacenet_amd import SurfaceNetHipError
    scene = sn["scene"]
    pts = np.array([[0.0, 0.0, 0.0], [1.0e5, 3.0, 3.0]])
    with pytest.raises(SurfaceNetHipError, match=r"2\^21"):                                 # 1e5 / 0.04 = 2.5e6 strides
        scene.quantizePts2Cubes(pts, 0.04, 4, 2, 0.5)
    with pytest.raises(SurfaceNetHipError, match=r"status -1"):
        scene.quantizePts2Cubes(pts.astype(np.float32), np.float32(0.04), 4, 2, 0.5)
    # 2^21 - 2 is the last floor index that fits (its diagonal neighbour is 2^21 - 1); one stride further does not
    edge = np.array([[0.0, 0.0, 0.0], [float((1 << 21) - 2), 0.0, 0.0]])
    cubes, _ = scene.quantizePts2Cubes(edge, 1, 4, 2, 0.5)
    assert cubes["ijk"][:, 0].tolist() == [0, 1, (1 << 21) - 2, (1 << 21) - 1]
    edge[1, 0] += 1.0
    with pytest.raises(SurfaceNetHipError, match=r"2\^21"):
        scene.quantizePts2Cubes(edge, 1, 4, 2, 0.5)
    with pytest.raises(ValueError):                                                        # the box leaves no point
        scene.quantizePts2Cubes(pts, 0.4, 32, 26, 0.5, BB=np.array([[500, 600], [500, 600], [500, 600]]))
    # the context is still usable
    _same(scene.quantizePts2Cubes(pts[:1], 0.4, 32, 26, 0.5), ref.quantizePts2Cubes(pts[:1], 0.4, 32, 26, 0.5))


def test_seeded_cubes_through_reconstruct_scene_and_postpass(sn):
    """A point-seeded cube set - two separate clumps, not a box - is a valid cubes_param_np: the scene runs, the cross-cube passes find their
    neighbours through the ijk map, and every cube that comes back is one of the seeded cells."""
    import test_gpu_pipeline as P
    from surfacenet_amd import reconstruct
    inp = P._pipeline_inputs()
    rs = np.random.RandomState(8)
    pts = np.concatenate([rs.rand(3, 3) * [14, 14, 8] + [-30, -25, 600], rs.rand(3, 3) * [14, 14, 8] + [10, 5, 612]]).astype(np.float32)
    resol = inp["cubes"]["resol"][0]
    cubes, cube_D_mm = sn["scene"].quantizePts2Cubes(pts, resol, inp["cube_D"], inp["Dc"], 0.5)
    _same((cubes, cube_D_mm), ref.quantizePts2Cubes(pts, resol, inp["cube_D"], inp["Dc"], 0.5))
    ext = cubes["ijk"].max(axis=0).astype(np.int64) + 1
    assert 8 <= cubes.shape[0] < ext.prod() and cube_D_mm == inp["cube_D_mm"]              # fewer cubes than the box around them
    inp["cubes"] = cubes
    out = P._run_scene(inp, sharded=False)
    assert len(out["vxl_ijk_list"]) > 0 and sum(len(a) for a in out["vxl_ijk_list"]) > 0
    post = reconstruct.scene_postpass(out, inp["cube_D"], inp["Dc"], inp["N_vp"], tau=0.6, gamma=0.5, beta=6, N_refine_iter=2)
    assert len(post["adapt_denoised_list"]) == len(out["vxl_ijk_list"])
    seeded = set(map(tuple, cubes["ijk"].tolist()))
    assert out["cube_ijk_np"].shape[0] > 0 and all(tuple(r) in seeded for r in out["cube_ijk_np"].tolist())
