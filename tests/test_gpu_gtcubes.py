"""GPU (-m gpu): the ground-truth mode (surfacenet_amd/csrc/gtcubes.h) against the numpy restatement
(tests/gtcubes_ref.py): occupancy cubes from a bound cloud - edge cases at the smallest cube sizes, a 200k-point cloud through the host and
device entries, the error paths - the weighted-accuracy counts, and the drop-ins built on them (SurfaceNet_inference(with_groundTruth=True),
the val_fn of SurfaceNet_fn_trainVal, reconstruct.hot_loop(gt=), SparseLoop(gt=)). Every comparison is array_equal or integer equality."""
import functools

import numpy as np
import pytest

import gtcubes_ref as ref
import ptcubes_ref

pytestmark = pytest.mark.gpu
R04, R08 = np.float32(0.4), np.float32(0.8)


@pytest.fixture(scope="module")
def ctxs(gpu_required):
    import surfacenet_amd
    made = {}

    def get(s):
        if s not in made:
            made[s] = surfacenet_amd.Context(cube_D=s, max_samples=4)
        return made[s]
    yield get
    for c in made.values():
        c.close()


@functools.lru_cache(maxsize=None)
def _edge_inputs(s):
    """A cloud and a cube list that put points on every kind of boundary of a cube of s voxels of 0.4 (side = 0.4 s)."""
    rs = np.random.RandomState(100 + s)
    x0 = np.array([-3.0, 2.0, 640.0], np.float32)
    xn = np.array([-20.5, -7.25, -0.1 - 0.4 * s], np.float32)                        # a cube in negative coordinates, across z = 0
    side = R04 * np.float32(s)
    pts = [x0 + (rs.rand(300, 3) * s).astype(np.float32) * R04,                      # inside the base cube
           xn + (rs.rand(120, 3) * s).astype(np.float32) * R04,
           x0 + rs.randint(0, s + 1, (60, 3)).astype(np.float32) * R04,              # exactly on voxel boundaries (some on the max faces)
           x0 + rs.randint(0, 2 * s + 1, (40, 3)).astype(np.float32) * (R04 / 2),
           x0[None, :].copy(), xn[None, :].copy()]                                   # p == xyz: the min corner
    face = x0 + (rs.rand(30, 3) * s).astype(np.float32) * R04
    face[:10, 0], face[10:20, 1], face[20:, 2] = x0[0], x0[1], x0[2]                 # on the three min faces
    top = x0 + (rs.rand(30, 3) * s).astype(np.float32) * R04
    top[:10, 0], top[10:20, 1], top[20:, 2] = x0[0] + side, x0[1] + side, x0[2] + side      # on the three max faces: outside
    pts += [face, top, np.array([[-0.0, 0.0, 0.0], [0.0, -0.0, 1e-30]], np.float32)]
    pts = np.concatenate(pts)
    lo = pts.min(axis=0).astype(np.float64)
    cell = float(side) / 4.0
    on_cells = (lo[None, :] + rs.randint(0, 12, (40, 3)) * cell).astype(np.float32)   # on the boundaries of the grid cells of the default bind
    pts = np.concatenate([pts, on_cells, pts[:50], pts[300:320]])                    # + duplicate points
    pts = np.ascontiguousarray(pts[rs.permutation(len(pts))])
    offs = np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], np.float32)
    xyz = [x0[None, :], x0[None, :], xn[None, :],                                    # duplicate cubes
           x0[None, :] + np.float32(1000.0),                                          # far from the cloud
           x0[None, :] + offs * (np.float32(0.4) * side),                             # overlapping at stride 0.4 of the side: a point lands in up to 27
           x0[None, :] - side / 2, xn[None, :] - side / 2,                            # resol 0.8 cubes around the two clumps
           np.zeros((1, 3), np.float32) - side / 2]
    xyz = np.concatenate(xyz).astype(np.float32)
    resol = np.full((xyz.shape[0],), R04, np.float32)
    resol[-3:] = R08                                                                  # resolutions differ within one call
    return pts, xyz, resol, float(side)


@pytest.mark.parametrize("cell", ["quarter", "larger_than_cube", "smaller_than_voxel"])
@pytest.mark.parametrize("s", [8, 12, 32])
def test_edge_cases_equal_restatement(ctxs, s, cell):
    ctx = ctxs(s)
    pts, xyz, resol, side = _edge_inputs(s)
    want = _edge_ref(s)
    assert want[0].sum() > 50 and want[3].sum() == 0 and np.array_equal(want[0], want[1]) and want[-2].sum() > 0
    assert ctx.gt_bind(pts, {"quarter": side / 4, "larger_than_cube": 2.5 * side, "smaller_than_voxel": 0.19}[cell]) == len(pts)
    got = ctx.gt_cubes((xyz, resol))
    assert got.dtype == np.float32 and got.shape == (len(xyz), 1, s, s, s)
    assert np.array_equal(got, want)
    assert np.array_equal(ctx.gt_cubes((xyz[::-1], resol[::-1])), want[::-1])
    if cell == "quarter":
        bound = ctx.bind_points(pts[::-1].astype(np.float64), side)                   # the Python surface: float64 in, any order
        assert bound.n_points == len(pts) and np.array_equal(ctx.gt_cubes((xyz, resol)), want)
        cubes = np.zeros(len(xyz), dtype=ptcubes_ref.CUBE_DTYPE)
        cubes["xyz"], cubes["resol"] = xyz, resol
        assert np.array_equal(ctx.gt_cubes(cubes), want)                              # the reference's cubes_param_np


@functools.lru_cache(maxsize=None)
def _edge_ref(s):
    pts, xyz, resol, _ = _edge_inputs(s)
    want = ref.gt_cubes(pts, xyz, resol, s)
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("s", [8, 12])
def test_one_point_and_no_points(ctxs, s):
    ctx = ctxs(s)
    _, xyz, resol, side = _edge_inputs(s)
    one = np.array([[-2.9, 2.3, 641.0]], np.float32)
    ctx.gt_bind(one, side / 4)
    want = ref.gt_cubes(one, xyz, resol, s)
    assert want[0].sum() == 1 and np.array_equal(ctx.gt_cubes((xyz, resol)), want)
    assert ctx.gt_bind(np.zeros((0, 3), np.float32), side / 4) == 0
    got = ctx.gt_cubes((xyz, resol))
    assert got.shape == want.shape and not got.any()
    assert ctx.gt_cubes((xyz[:0], resol[:0])).shape == (0, 1, s, s, s)


def test_one_point_per_cell_fills_half_of_the_smallest_table(ctxs):
    """512 points in 512 distinct cells: the bound grid's hash table has its minimum capacity of 1,024 slots and is half full, the fullest
    the capacity rule allows (probes walk past taken slots, also from the last slot on to slot 0)."""
    s, cell = 8, 0.8
    ctx = ctxs(s)
    x0 = np.array([-3.0, 2.0, 640.0], np.float32)
    side = R04 * np.float32(s)                                                        # four cells
    f = np.arange(8) + np.where(np.arange(8) == 0, 0.0, 0.5)                          # the grid's origin itself, then the middle of every further cell
    pts = x0 + (np.stack(np.meshgrid(f, f, f, indexing="ij"), -1).reshape(-1, 3) * cell).astype(np.float32)
    assert pts.dtype == np.float32
    cells = np.floor((pts.astype(np.float64) - pts.min(axis=0).astype(np.float64)) / cell)
    assert np.unique(cells, axis=0).shape[0] == 512
    offs = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.float32)
    xyz = np.concatenate([x0[None, :] + offs * side, x0[None, :] + side / 2, x0[None, :] - side / 4]).astype(np.float32)
    resol = np.full((len(xyz),), R04, np.float32)
    want = ref.gt_cubes(pts, xyz, resol, s)
    assert want.sum() > 512                                                           # every point in a lattice cube, some in the two others too
    assert ctx.gt_bind(pts, cell) == 512
    assert np.array_equal(ctx.gt_cubes((xyz, resol)), want)


SCALE_STEP, BATCH = 37, 64


@functools.lru_cache(maxsize=None)
def _scale():
    """ptcubes_ref.wavy_cloud(200000) as float32 and the cubes quantizePts2Cubes seeds from it with the scan9 settings - every 37th of its
    12340, so that the restatement's side of the comparison stays within a second: 334 cubes, five calls of 64 and one of 14."""
    pts = ptcubes_ref.wavy_cloud(200000).astype(np.float32)
    cubes, side = ptcubes_ref.quantizePts2Cubes(pts, BB=ptcubes_ref.SCAN9_BB, **ptcubes_ref.SCAN9)
    cubes = cubes[::SCALE_STEP]
    assert cubes.shape[0] > 4 * BATCH and cubes.shape[0] % BATCH != 0
    want = ref.gt_cubes(pts, cubes["xyz"], cubes["resol"], 32, sorted_x=ref.presort(pts))
    want.setflags(write=False)
    assert (want.reshape(len(cubes), -1).sum(axis=1) > 0).mean() > 0.9 and want.sum() > 20000
    return pts, cubes, float(side), want


@pytest.mark.parametrize("order", ["raster", "permuted"])
def test_scale_host_and_dev_entries_equal_restatement(ctxs, order):
    ctx = ctxs(32)
    pts, cubes, side, want = _scale()
    if order == "permuted":
        pts = pts[np.random.RandomState(5).permutation(len(pts))]
    n, s = len(cubes), 32
    bound = ctx.bind_points(pts, side)
    host = np.concatenate([ctx.gt_cubes(cubes[i:i + BATCH]) for i in range(0, n, BATCH)])
    assert np.array_equal(host, want)
    d_pts, d_xyz, d_resol = ctx.upload(pts), ctx.upload(np.ascontiguousarray(cubes["xyz"])), ctx.upload(np.ascontiguousarray(cubes["resol"]))
    d_Y = ctx.dev_alloc(BATCH * s ** 3 * 4)
    try:
        ctx.gt_bind_dev(len(pts), d_pts, side / 4)
        with pytest.raises(ValueError):
            bound.check()                                                             # the context holds another binding now
        dev = np.empty_like(host)
        for i in range(0, n, BATCH):
            m = min(BATCH, n - i)
            ctx.gt_cubes_dev(m, d_xyz + 12 * i, d_resol + 4 * i, d_Y)
            ctx.d2h(dev[i:i + m], d_Y)
        ctx.synchronize()
        assert np.array_equal(dev, host)
        ctx.gt_cubes_dev(3, d_xyz + 12, d_resol + 4, d_Y + 4)                         # a Y that is not 16-byte aligned: the scalar stores
        odd = np.empty((3, 1, s, s, s), np.float32)
        ctx.d2h(odd, d_Y + 4)
        assert np.array_equal(odd, want[1:4])
    finally:
        for p in (d_pts, d_xyz, d_resol, d_Y):
            ctx.dev_free(p)


def test_rebinding_replaces_the_cloud(ctxs):
    ctx = ctxs(32)
    pts, cubes, side, want = _scale()
    sub = cubes[:BATCH]
    ctx.bind_points(pts, side)
    assert np.array_equal(ctx.gt_cubes(sub), want[:BATCH])
    other = (pts[::7] + np.float32(3.0)).astype(np.float32)                           # fewer points, moved: a smaller table in the same workspace
    ctx.bind_points(other, side)
    got = ctx.gt_cubes(sub)
    assert np.array_equal(got, ref.gt_cubes(other, sub["xyz"], sub["resol"], 32)) and not np.array_equal(got, want[:BATCH])


def test_errors_leave_the_context_usable(gpu_required):
    import surfacenet_amd
    from surfacenet_amd import SurfaceNetHipError
    s = 8
    pts, xyz, resol, side = _edge_inputs(s)
    want = _edge_ref(s)
    with surfacenet_amd.Context(cube_D=s, max_samples=2) as ctx:
        with pytest.raises(SurfaceNetHipError, match=r"no ground-truth cloud is bound.*status -2"):
            ctx.gt_cubes((xyz, resol))
        d = ctx.dev_alloc(len(xyz) * s ** 3 * 4)
        try:
            with pytest.raises(SurfaceNetHipError, match=r"status -2"):
                ctx.gt_cubes_dev(1, d, d, d)
            for bad_value in (np.nan, np.inf, -np.inf):
                bad = pts.copy()
                bad[len(bad) // 2, 1] = bad_value
                with pytest.raises(SurfaceNetHipError, match=r"not finite.*status -1"):
                    ctx.gt_bind(bad, side / 4)
            with pytest.raises(SurfaceNetHipError, match=r"status -2"):             # a failed bind leaves no cloud
                ctx.gt_cubes((xyz, resol))
            ctx.gt_bind(pts, side / 4)
            assert np.array_equal(ctx.gt_cubes((xyz, resol)), want)
            far = np.array([[0.0, 0.0, 0.0], [1.0e5, 3.0, 3.0]], np.float32)
            with pytest.raises(SurfaceNetHipError, match=r"2\^21.*status -1"):       # 1e5 / 0.04 = 2.5e6 cells
                ctx.gt_bind(far, 0.04)
            for cell in (0.0, -1.0, np.nan, np.inf):
                with pytest.raises(SurfaceNetHipError, match=r"cell.*status -1"):
                    ctx.gt_bind(pts, cell)
            ctx.gt_bind(pts, side / 4)
            for bad_resol in (0.0, -0.4, np.nan, np.inf):
                r = resol.copy()
                r[2] = bad_resol
                with pytest.raises(SurfaceNetHipError, match=r"cube 2: resol.*status -1"):
                    ctx.gt_cubes((xyz, r))
            x = xyz.copy()
            x[1, 2] = np.nan
            with pytest.raises(SurfaceNetHipError, match=r"cube 1: xyz.*status -1"):
                ctx.gt_cubes((x, resol))
            # the device form is asynchronous: it zeroes such a cube and reports at the next synchronize
            r = resol.copy()
            r[2] = 0.0
            d_xyz, d_r = ctx.upload(xyz), ctx.upload(r)
            try:
                ctx.gt_cubes_dev(len(xyz), d_xyz, d_r, d)
                with pytest.raises(SurfaceNetHipError, match=r"sn_gt_cubes_dev.*status -1"):
                    ctx.synchronize()
                got = np.empty_like(want)
                ctx.d2h(got, d)
                keep = np.arange(len(xyz)) != 2
                assert np.array_equal(got[keep], want[keep]) and not got[2].any()
                ctx.synchronize()                                                     # reported once
            finally:
                ctx.dev_free(d_xyz); ctx.dev_free(d_r)
            assert np.array_equal(ctx.gt_cubes((xyz, resol)), want)
            with pytest.raises(TypeError):
                ctx.weighted_accuracy_counts(want.astype(np.float64), want)
            with pytest.raises(TypeError):
                ctx.weighted_accuracy_counts(want, want[:-1])
        finally:
            ctx.dev_free(d)


def _accuracy_inputs(s):
    rs = np.random.RandomState(200 + s)
    n = 6
    pred = rs.rand(n, 1, s, s, s).astype(np.float32)
    Y = (rs.rand(n, 1, s, s, s) < 0.2).astype(np.float32)
    p, y = pred.reshape(n, -1), Y.reshape(n, -1)
    below = np.nextafter(np.float32(0.5), np.float32(0))
    p[0, :8] = [0.5, 0.5, below, below, np.nan, np.nan, 1.0, 0.0]
    y[0, :8] = [1, 0, 1, 0, 1, 0, 1, 0]
    p[1, ::5] = 0.5
    p[1, 1::7] = below
    y[2, :40] = 0.7                                                                   # soft targets: positives no prediction can hit
    y[2, 40:60] = -1.0                                                                # negative targets: in neither class
    y[2, 60:70] = np.nan
    p[2, 65:75] = np.nan
    y[3] = 0.0                                                                        # an empty cube
    y[4] = 1.0                                                                        # a full cube
    p[5, -3:] = [np.inf, -np.inf, -0.0]
    y[5, -3:] = [1, 0, -0.0]
    return pred, Y


@pytest.mark.parametrize("s", [8, 12, 32])
def test_accuracy_counts_equal_restatement(ctxs, s):
    from surfacenet_amd import groundTruth
    ctx = ctxs(s)
    pred, Y = _accuracy_inputs(s)
    n = pred.shape[0]
    want = ref.accuracy_counts(pred, Y)
    assert want[3, 0] == 0 and want[4, 1] == 0 and want[2, 0] >= 40 and want[2, :2].sum() == s ** 3 - 30
    got = ctx.weighted_accuracy_counts(pred, Y)
    assert got.dtype == np.int64 and got.shape == (n, 4) and np.array_equal(got, want)
    acc, per_cube = ctx.weighted_accuracy(pred, Y, per_cube=True)
    assert type(acc) is np.float64 and acc == ref.weighted_accuracy(pred, Y) and np.array_equal(per_cube, want)
    assert per_cube.sum(axis=0).tolist() == ref.accuracy_counts(pred.reshape(1, -1), Y.reshape(1, -1))[0].tolist()     # per-cube counts sum to the batch's
    for thr in (0.3, float(np.nextafter(np.float32(0.5), np.float32(1)))):
        assert np.array_equal(ctx.weighted_accuracy_counts(pred, Y, thr), ref.accuracy_counts(pred, Y, thr))
    # single cubes: no positives -> acc_pos = acc_neg; no negatives -> NaN
    a3, a4 = ctx.weighted_accuracy(pred[3:4], Y[3:4]), ctx.weighted_accuracy(pred[4:5], Y[4:5])
    assert a3 == groundTruth.accuracy_from_counts(want[3:4]) == want[3, 3] / want[3, 1] and np.isnan(a4)
    d_p, d_y, d_c = ctx.upload(pred), ctx.upload(Y), ctx.dev_alloc(n * 32 + 32)
    try:
        dev = np.full((n, 4), -1, np.int64)
        ctx.weighted_accuracy_dev(n, d_p, d_y, d_c)
        ctx.d2h(dev, d_c)
        assert np.array_equal(dev, want)
        ctx.weighted_accuracy_dev(n - 1, d_p + 4 * s ** 3, d_y + 4 * s ** 3, d_c + 32)        # a later cube first, into a later row
        ctx.d2h(dev[1:], d_c + 32)
        assert np.array_equal(dev[1:], want[1:])
    finally:
        for p in (d_p, d_y, d_c):
            ctx.dev_free(p)


@pytest.fixture()
def dropin(gpu_required):
    from surfacenet_amd import SurfaceNet, groundTruth, runtime
    runtime.reset()
    yield SurfaceNet, groundTruth, runtime
    runtime.reset()


def test_dropin_with_groundTruth_and_val_fn(dropin):
    SurfaceNet, groundTruth, runtime = dropin
    import surfacenet_amd
    import synth
    from surfacenet_amd import weights
    s, n, n_vp = 8, 3, 2
    values = weights.synthetic_param_values(0)
    X = synth.random_cvc(n * n_vp, s, 7)
    rs = np.random.RandomState(7)
    w = (rs.rand(n, n_vp) + 0.1).astype(np.float32)
    w /= w.sum(axis=1, keepdims=True)
    # targets from a cloud, through the module-level surface: points in the three cubes, one cube left half empty
    xyz = np.array([[0.0, 0.0, 0.0], [1.6, 1.6, 0.0], [-40.0, 3.0, 7.0]], np.float32)
    pts = np.concatenate([xyz[c] + (rs.rand(60 + 40 * c, 3) * [s, s, s // (1 + c % 2)]).astype(np.float32) * R04 for c in range(n)])
    runtime.prefer_cube_D(s)
    bound = groundTruth.bind_points(pts, float(R04) * s)
    assert bound.ctx is runtime.context_for(s) and bound.n_points == len(pts)
    Y = groundTruth.gt_cubes((xyz, R04), s)
    assert np.array_equal(Y, ref.gt_cubes(pts, xyz, R04, s)) and Y.sum() > 100
    assert np.array_equal(groundTruth.gt_cubes_from_points(pts[::-1], (xyz, R04), s), Y)

    relw_fn, fn = SurfaceNet.SurfaceNet_inference(n_vp, None, param_values=values)
    f0, u0 = fn(X, w)
    _, fn_gt = SurfaceNet.SurfaceNet_inference(n_vp, None, param_values=values, with_groundTruth=True)
    out = fn_gt(X, w, Y)
    assert isinstance(out, list) and len(out) == 3
    acc, fused, unfused = out
    assert np.array_equal(fused, f0) and np.array_equal(unfused, u0)
    assert type(acc) is np.float64 and acc == ref.weighted_accuracy(fused, Y) and 0.0 <= acc <= 1.0
    assert acc == groundTruth.weighted_accuracy(fused, Y)
    acc2, fused2, _ = fn_gt(X, w, Y, n_vp)                                           # n_samples_perGroup after Y (nets/SurfaceNet.py:365-372)
    assert acc2 == acc and np.array_equal(fused2, f0)
    acc3 = fn_gt(X, w, Y, n_samples_perGroup=n_vp)[0]
    assert acc3 == acc
    for bad in (Y.astype(np.float64), Y[:, 0], Y[:-1], np.zeros((n, 1, s, s, s + 1), np.float32), Y.tolist()):
        with pytest.raises(TypeError):
            fn_gt(X, w, bad)
    with pytest.raises(TypeError):
        fn_gt(X, w)                                                                  # Y is missing

    # N_viewPairs4inference == 1: (X, Y)
    _, fn1 = SurfaceNet.SurfaceNet_inference(1, None, param_values=values)
    _, fn1_gt = SurfaceNet.SurfaceNet_inference(1, None, param_values=values, with_groundTruth=True)
    g0 = fn1(X[:n])[0]
    acc1, g1, g1u = fn1_gt(X[:n], Y)
    assert np.array_equal(g1, g0) and np.array_equal(g1u, g0) and acc1 == ref.weighted_accuracy(g1, Y)
    with pytest.raises(TypeError):
        fn1_gt(X[:n], w[:, :1], Y)

    # val_fn(X, similFeature, Y) = relative_weights, then the drop-in
    feat = rs.rand(n * n_vp, 258).astype(np.float32)
    net, train_fn, val_fn = SurfaceNet.SurfaceNet_fn_trainVal(n_vp, param_values=values)
    assert net is None and train_fn is None
    va, vf = val_fn(X, feat, Y)
    wa, wf, _ = fn_gt(X, relw_fn(feat), Y)
    assert va == wa and np.array_equal(vf, wf) and type(va) is np.float64
    with pytest.raises(NotImplementedError):
        SurfaceNet.SurfaceNet_fn_trainVal(n_vp, param_values=values, return_train_fn=True)

    # more samples than the context holds at once: the chunks of sn_forward
    with surfacenet_amd.Context(cube_D=s, max_samples=4) as ctx:
        ctx.load_param_values(values)
        cf, cu = ctx.forward(X, w, n_vp=n_vp)
        gf, gu, counts = ctx.forward_gt(X, w, Y, n_vp=n_vp)
        assert np.array_equal(gf, cf) and np.array_equal(gu, cu) and np.array_equal(counts, ref.accuracy_counts(cf, Y))


def test_hot_loop_and_sparse_loop_count_on_the_device(gpu_required):
    import surfacenet_amd
    import golden_util
    from surfacenet_amd import reconstruct, weights
    s, n_all, n_vp = 16, 7, 2
    validCubes = np.array([1, 1, 0, 1, 1, 0, 1], dtype=bool)                          # 5 valid cubes, batches of 2
    sc = golden_util.synthetic_scene(n_all, n_vp, s=s, seed=6, hw=(600, 800))
    cubes_param_np = np.zeros(n_all, dtype=ptcubes_ref.CUBE_DTYPE)
    cubes_param_np["xyz"], cubes_param_np["resol"] = sc["xyz"], sc["resol"]
    vp4, w4 = sc["pairs"][validCubes], sc["w"][validCubes]
    rs = np.random.RandomState(6)
    side = float(sc["resol"][0]) * s
    pts = np.concatenate([sc["xyz"][c] + (rs.rand(150, 3) * [s, s, 2]).astype(np.float32) * sc["resol"][c] + np.float32([0, 0, 0.4 * c])
                          for c in range(n_all) if c != 3]).astype(np.float32)        # a sheet in every cube but one
    values = weights.synthetic_param_values(0)
    with surfacenet_amd.Context(cube_D=s, max_samples=8) as ctx:
        ctx.load_param_values(values); ctx.set_cameras(sc["cams"]); ctx.set_images(sc["imgs"])
        plain = list(reconstruct.hot_loop(ctx, validCubes, vp4, w4, cubes_param_np, batch_size=2))
        gt = ctx.bind_points(pts, side)
        with_gt = list(reconstruct.hot_loop(ctx, validCubes, vp4, w4, cubes_param_np, batch_size=2, gt=gt))
        assert len(plain) == len(with_gt) == 3 and all(len(a) == 4 and len(b) == 5 for a, b in zip(plain, with_gt))
        Y = ctx.gt_cubes(cubes_param_np[validCubes])
        assert np.array_equal(Y, ref.gt_cubes(pts, sc["xyz"][validCubes], sc["resol"][validCubes], s)) and all(Y[c].any() for c in (0, 1, 3, 4))
        table = np.concatenate([b[4] for b in with_gt])
        fused_all = np.concatenate([a[1] for a in plain])
        for a, b in zip(plain, with_gt):
            for k in range(4):
                assert np.array_equal(a[k], b[k])                                     # the other outputs: bit-identical
        assert table.shape == (5, 4) and table.dtype == np.int64
        assert np.array_equal(table, ctx.weighted_accuracy_counts(fused_all, Y))      # per-cube counts from the host path
        assert np.array_equal(table, ref.accuracy_counts(fused_all, Y))
        # one batch larger than the context holds at once (chunked as sn_cvc_forward chunks), without the CVC tensor
        big = list(reconstruct.hot_loop(ctx, validCubes, vp4, w4, cubes_param_np, batch_size=5, return_cvc=False, gt=gt))
        want_big = ctx.cvc_forward(vp4, sc["xyz"][validCubes], sc["resol"][validCubes], w4)
        assert len(big) == 1 and big[0][3] is None and np.array_equal(big[0][1], want_big[0]) and np.array_equal(big[0][2], want_big[1])
        assert np.array_equal(big[0][4], ref.accuracy_counts(want_big[0], Y))
        # the device-resident loop body: its own outputs unchanged, the same table
        kw = dict(max_cubes=2, min_prob=0.5, cube_Dcenter=12)
        loop = reconstruct.SparseLoop(ctx, n_vp, **kw)
        want_many = loop.run_many(vp4, sc["xyz"][validCubes], sc["resol"][validCubes], w4)
        want_one = loop.run(vp4[:2], sc["xyz"][validCubes][:2], sc["resol"][validCubes][:2], w4[:2])
        loop.close()
        loop = reconstruct.SparseLoop(ctx, n_vp, gt=gt, **kw)
        got_many = loop.run_many(vp4, sc["xyz"][validCubes], sc["resol"][validCubes], w4)
        got_one = loop.run(vp4[:2], sc["xyz"][validCubes][:2], sc["resol"][validCubes][:2], w4[:2])
        loop.close()
        assert len(want_many) == len(want_one) == 6 and len(got_many) == len(got_one) == 7
        for want, got in ((want_many, got_many), (want_one, got_one)):
            assert got[0] == want[0] and np.array_equal(got[5], want[5])
            for k in (1, 2, 3, 4):
                assert len(got[k]) == len(want[k]) and all(np.array_equal(a, b) for a, b in zip(got[k], want[k]))
        assert np.array_equal(got_many[6], table) and np.array_equal(got_one[6], table[:2])
        other = surfacenet_amd.Context(cube_D=s, max_samples=2)
        try:
            with pytest.raises(ValueError):
                list(reconstruct.hot_loop(other, validCubes, vp4, w4, cubes_param_np, batch_size=2, gt=gt))     # bound to another context
        finally:
            other.close()
