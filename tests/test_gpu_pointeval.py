"""GPU (-m gpu): the DTU point-cloud evaluation (surfacenet_amd/csrc/pointeval.h through surfacenet_amd.evaluation) bit-identical to the CPU
restatement (tests/pointeval_ref.py): nearest-neighbour distances, the reduced index set, the mask / plane flags, eval_ply end to end on a
synthetic DTU folder, and a scene's masks evaluated in memory equal to the PLY path."""
import numpy as np
import pytest

import pointeval_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ev(gpu_required):
    from surfacenet_amd import evaluation, runtime
    return evaluation, runtime.any_context()


def _mixed_clouds(rs, n=20000):
    stl = ref.wavy_surface(n - 2000, rs)
    clusters = np.repeat(rs.uniform([0, 0, 3], [40, 30, 7], (100, 3)), 10, axis=0) + rs.normal(0, 0.02, (1000, 3))
    to = np.concatenate([stl, clusters, stl[rs.randint(0, stl.shape[0], 1000)]])          # exact duplicates
    frm = np.concatenate([ref.data_cloud(stl, rs, outliers=0.0)[:n - 400 - 300], to[rs.randint(0, to.shape[0], 300)],   # points ON the cloud
                          rs.uniform([-30, -30, -30], [70, 60, 40], (400, 3))])             # 2 % far outliers, some beyond max_dist
    return to[rs.permutation(to.shape[0])], frm[rs.permutation(frm.shape[0])]


def _check_d2(got, to, frm, max_dist):
    want = ref.nn_d2(to, frm)
    lim = max_dist * max_dist * (1.0 + 2.0 ** -40)
    below = want < lim
    assert np.array_equal(got[below], want[below])
    assert np.all(got[~below] == np.inf)
    assert np.array_equal(ref.capped(got, max_dist), ref.capped(want, max_dist))


@pytest.mark.parametrize("max_dist", [60.0, 1.0, 0.05])
def test_nn_dist2_mixed_clouds(ev, max_dist):
    _, ctx = ev
    to, frm = _mixed_clouds(np.random.RandomState(10))
    _check_d2(ctx.nn_dist2(to, frm, max_dist), to, frm, max_dist)


def test_nn_dist2_edge_cases(ev):
    evaluation, ctx = ev
    rs = np.random.RandomState(11)
    frm = rs.uniform(-5, 5, (777, 3))
    assert np.all(ctx.nn_dist2(np.zeros((0, 3)), frm, 60.0) == np.inf)
    assert np.all(evaluation.max_dist_cp(np.zeros((0, 3)), frm, 60.0) == 60.0)
    assert ctx.nn_dist2(frm, np.zeros((0, 3)), 60.0).shape == (0,)
    one = np.asarray([[0.5, -0.25, 1.0]])
    _check_d2(ctx.nn_dist2(one, frm, 60.0), one, frm, 60.0)
    _check_d2(ctx.nn_dist2(frm, one, 60.0), frm, one, 60.0)
    same = np.repeat(one, 50, axis=0)                                   # every point in one cell, queries far and near
    _check_d2(ctx.nn_dist2(same, frm, 3.0), same, frm, 3.0)
    far = frm + [1e4, 0, 0]                                             # every query beyond max_dist
    assert np.all(ctx.nn_dist2(frm, far, 60.0) == np.inf)
    _check_d2(ctx.nn_dist2(frm, far, np.inf), frm, far, np.inf)


@pytest.mark.parametrize("n,dst", [(20000, 0.25), (20000, 0.2), (20000, 0.0), (200000, 0.2), (1000000, 0.2)])
def test_reduce_index_set(ev, n, dst):
    evaluation, ctx = ev
    rs = np.random.RandomState(n % 997)
    base = rs.randint(0, 1024, (n // 8, 3)) / 64.0
    parts = [base, base + [0.25, 0, 0], base + [0, 0, -0.25],                          # pairs at exactly 0.25
             np.repeat(base[: n // 16], 2, axis=0),                                     # coincident points
             np.repeat(rs.uniform(0, 16, (n // 400, 3)), 50, axis=0) + rs.normal(0, 0.03, (n // 400 * 50, 3))]   # dense clusters
    p = np.concatenate(parts)
    p = np.concatenate([p, rs.uniform(0, 16, (n - p.shape[0], 3))])
    order = rs.permutation(n)
    want = ref.reduce_rounds(p, order, dst)
    got, idx = evaluation.reduce_points(p, dst=dst, order=order, return_index=True)
    assert np.array_equal(idx, np.nonzero(want)[0])
    assert np.array_equal(got, p[want])


def test_reduce_default_order_and_rounds(ev):
    evaluation, ctx = ev
    rs = np.random.RandomState(12)
    p = ref.data_cloud(ref.wavy_surface(20000, rs), rs)
    want = ref.reduce_rounds(p, np.random.RandomState(0).permutation(p.shape[0]), 0.2)
    assert np.array_equal(evaluation.reduce_points(p), p[want])
    small = p[:3000]
    order = rs.permutation(3000)
    rank = np.empty(3000, np.int64)
    rank[order] = np.arange(3000)
    keep, rounds = ctx.point_reduce(small, rank, 0.2)
    assert np.array_equal(keep, ref.reduce_sequential(small, order, 0.2)) and 1 <= rounds < 100


def test_one_point_per_cell_fills_half_of_the_smallest_table(ev):
    """512 points in 512 distinct cells: the grid's hash table has its minimum capacity of 1,024 slots and is half full, the fullest the
    capacity rule allows (probes walk past taken slots, also from the last slot on to slot 0)."""
    evaluation, ctx = ev
    ijk = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
    p = ijk + 0.03 * (ijk.sum(1, keepdims=True) % 2)           # neighbours along an axis lie 0.971 or 1.031 apart
    dst = 0.98
    cells = np.floor((p - p.min(0)) / (dst * (1.0 + 1e-6)))    # the reduction's grid: cells a little larger than dst
    assert np.unique(cells, axis=0).shape[0] == 512
    order = np.random.RandomState(13).permutation(512)
    want = ref.reduce_rounds(p, order, dst)
    assert 0 < want.sum() < 512
    got, idx = evaluation.reduce_points(p, dst=dst, order=order, return_index=True)
    assert np.array_equal(idx, np.nonzero(want)[0]) and np.array_equal(got, p[want])
    # nearest neighbours: the first bucketing of the 512 points, at their mean spacing, puts one point in every cell as well
    frm = np.concatenate([p + [0.25, -0.125, 0.5], p[::7]])
    _check_d2(ctx.nn_dist2(p, frm, 60.0), p, frm, 60.0)
    _check_d2(ctx.nn_dist2(p, frm, 0.5), p, frm, 0.5)


def test_flags_at_boundaries(ev):
    _, ctx = ev
    rs = np.random.RandomState(13)
    mask = (rs.uniform(0, 1, (23, 17, 9)) < 0.6).astype(np.uint8)
    bb, res = np.asarray([-20.0, -7.0, 3.0]), 2.0
    # voxel half-boundaries (k + 0.5 voxels, and the doubles either side), the mask's faces, outside, negative coordinates
    k = np.arange(-3, 27)[:, None] + np.asarray([0.5, 0.0, -0.5])[None, :]
    t = (k.reshape(-1)[:, None] * res + bb[None, :])
    q = np.concatenate([t, np.nextafter(t, np.inf), np.nextafter(t, -np.inf), bb[None, :] + [[-0.49999999999999994 * res, 0, 0]],
                        rs.uniform(-60, 60, (20000, 3)), [bb + res * (np.asarray(mask.shape) - 1), bb + res * (np.asarray(mask.shape) - 0.5)]])
    q = np.concatenate([q, q[:, [1, 2, 0]], q[:, [2, 0, 1]]])
    plane = np.asarray([0.3, -0.7, 0.2, 1.5])
    in_mask, above = ctx.point_flags(q, mask=mask, bb_min=bb, res=res, plane=plane)
    assert np.array_equal(in_mask, ref.in_mask(q, mask, bb, res)) and in_mask.any() and not in_mask.all()
    assert np.array_equal(above, ref.above_plane(q, plane)) and above.any() and not above.all()
    a2, b2 = ctx.point_flags(q, plane=plane)
    assert a2 is None and np.array_equal(b2, above)
    on = np.asarray([[1.0, 1.0, 1.0], [2.0, 0.0, 0.0]])
    assert ctx.point_flags(on, plane=[1.0, 1.0, 1.0, -3.0])[1].tolist() == [False, False]


def test_eval_ply_end_to_end(ev, tmp_path):
    sio = pytest.importorskip("scipy.io")
    evaluation, _ = ev
    from surfacenet_amd import sparseCubes
    rs = np.random.RandomState(14)
    stl = ref.wavy_surface(20000, rs).astype(np.float32)
    data = ref.data_cloud(stl.astype(np.float64), rs).astype(np.float32)
    folder = ref.make_dtu_folder(str(tmp_path / "dtu"), 9, stl)
    sparseCubes.save2ply(str(tmp_path / "data.ply"), data)
    got = evaluation.eval_ply(9, str(tmp_path / "data.ply"), str(tmp_path / "eval.mat"), str(tmp_path / "dtu"))
    base = ref.point_compare(data, stl, folder["mask"], folder["BB"], folder["Res"], folder["plane"])
    assert np.array_equal(got, ref.eval_acc_compl(base))
    be = sio.loadmat(str(tmp_path / "eval.mat"))["BaseEval"][0, 0]
    assert np.array_equal(be["Qdata"], base["Qdata"].T) and np.array_equal(be["Ddata"].reshape(-1), base["Ddata"])
    assert np.array_equal(be["Dstl"].reshape(-1), base["Dstl"])


def test_scene_points_in_memory_equal_the_ply_path(ev, tmp_path):
    evaluation, _ = ev
    from surfacenet_amd import sparseCubes, synthetic
    d = synthetic.sparse_surface((6, 6, 3), 26, thickness=2, amplitude=6.0, seed=5)
    masks = [p >= 0.7 for p in d["prediction_list"]]
    path = str(tmp_path / "scene.ply")
    sparseCubes.save_sparseCubes_2ply(masks, d["vxl_ijk_list"], d["rgb_list"], d["param_np"], ply_filePath=path)
    from_ply = evaluation.read_ply_xyz(path)
    in_memory = sparseCubes.sparse_xyz(masks, d["vxl_ijk_list"], d["param_np"])
    assert in_memory.dtype == np.float32 and np.array_equal(in_memory, from_ply)
    stl = from_ply[::3].astype(np.float64) + [0.05, -0.05, 0.1]
    mask = np.ones((9, 11, 13), np.uint8)
    BB, res, plane = np.asarray([[-22, -22, -22], [0, 0, 0]]), 2, np.asarray([0.0, 0.0, 1.0, 10.0])
    a = evaluation.eval_acc_compl(evaluation.point_compare(from_ply, stl, mask, BB, res, plane))
    b = evaluation.eval_acc_compl(evaluation.point_compare(in_memory, stl, mask, BB, res, plane))
    base = ref.point_compare(from_ply, stl, mask, BB, res, plane)
    assert np.array_equal(a, b) and np.array_equal(a, ref.eval_acc_compl(base))
