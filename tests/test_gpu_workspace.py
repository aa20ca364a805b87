"""GPU (-m gpu): the context's device workspaces (sn_internal.h DevBuf / dev_reserve) through the entries that carve them. One context, and
per entry three calls, small -> large -> small: the first allocates the workspace, the second has to grow it, the third runs in a buffer
larger than it needs. Every result equals the entry's restatement (bit for bit, or within the tolerance the entry's own test module uses),
and the third equals the first bit for bit. The packed-list entries also take a call without cubes and one without voxels in between. The
host forms share two more buffers, the host mirror's (sn_internal.h HostMirror): the geometry stages and the post-pass entries run in turn
on one scene per size, so that each call finds those buffers as another entry left them."""
import os

import numpy as np
import pytest

import components_ref
import golden_util
import gtcubes_ref
import mesh_ref
import meshsample_ref
import meshsimplify_ref
import normals_ref
import pointeval_ref
import postpass_ref
import ptcubes_ref
from oracle import post_oracle, simil_oracle

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
P_DTU = np.load(os.path.join(GOLD, "cameras.npz"))["P_dtu"]
SIMIL = np.load(os.path.join(GOLD, "simil_cases.npz"))
MEAN_BGR = np.asarray([103.939, 116.779, 123.68]).astype(np.float32)
S = 8                      # the smallest cube edge a context takes
TOL_NORMAL = 2e-7          # tests/test_gpu_normals.py TOL
TOL_EMB = 2e-5             # tests/test_gpu_simil.py TOL_EMB_X3


@pytest.fixture(scope="module")
def ctx(gpu_required):
    import surfacenet_amd
    from surfacenet_amd import weights
    H, W = (int(v) for v in SIMIL["sc_hw"])
    with surfacenet_amd.Context(cube_D=S, max_samples=2) as c:
        c.set_cameras(P_DTU)
        c.set_images([golden_util.synth_image(int(sd), H, W) for sd in SIMIL["sc_seeds"]])
        c.load_simil_param_values(weights.synthetic_simil_param_values(1))      # the weights tests/test_gpu_simil.py sets against the oracle
        yield c


def _same(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(a, b)) and len(a) == len(b)


# ---- normals and unique voxels: one workspace ------------------------------------------------------------------------------------------------
def _stepped_sheet(nx, ny):
    """nx x ny cubes of 8^3 voxels at a stride of 4 (neighbours overlap by half): each lists its part of the one-voxel sheet z = (x + y) // 10."""
    cubes, lists = [], []
    for cx in range(nx):
        for cy in range(ny):
            cubes.append([cx, cy, 0])
            lists.append(np.asarray([(i, j, (4 * cx + i + 4 * cy + j) // 10) for i in range(8) for j in range(8)], np.uint8))
    return normals_ref.hand_scene(cubes, lists, stride_vox=4)


def _normals_and_unique(ctx, s):
    nrm, mom = ctx.normals(*normals_ref.scene_args(s), return_moments=True)
    keep = ctx.unique_voxels(s["offsets"], s["ijk"], s["cube_ijk"], s["mask"], s["stride_vox"])      # between two normals calls: the same workspace
    r = normals_ref.normals_ref(*normals_ref.scene_args(s))
    assert np.array_equal(mom, r["moments"])
    assert np.array_equal(keep, normals_ref.unique_ref(s["offsets"], s["ijk"], s["cube_ijk"], s["mask"], s["stride_vox"]))
    assert r["comparable"].any() and np.abs(nrm[r["comparable"]].astype(np.float64) - r["normals"][r["comparable"]]).max() <= TOL_NORMAL
    assert not nrm[~r["solved"]].any()
    return nrm, mom, keep


def _empty_packed_calls(ctx):
    none = normals_ref.hand_scene(np.zeros((0, 3)), [], stride_vox=4)                                  # n = 0
    bare = normals_ref.hand_scene([[0, 0, 0], [1, 0, 0]], [np.zeros((0, 3), np.uint8)] * 2, stride_vox=4)   # total = 0
    for e in (none, bare):
        nrm, mom = ctx.normals(*normals_ref.scene_args(e), return_moments=True)
        assert nrm.shape == (0, 3) and mom.shape == (0, 10)
        assert ctx.unique_voxels(e["offsets"], e["ijk"], e["cube_ijk"], e["mask"], 4).shape == (0,)


def test_normals_and_unique_share_a_growing_workspace(ctx):
    small, large = _stepped_sheet(2, 1), _stepped_sheet(8, 5)
    assert len(small["cube_ijk"]) == 2 and len(large["cube_ijk"]) == 40
    first = _normals_and_unique(ctx, small)
    _empty_packed_calls(ctx)
    _normals_and_unique(ctx, large)
    _empty_packed_calls(ctx)
    third = _normals_and_unique(ctx, small)
    assert _same(first, third)
    assert not first[2].all() and first[2].any()               # the overlap: some cells are listed by both cubes


# ---- the host mirror: every host form stages in the same two buffers -----------------------------------------------------------------------------
ORIGIN, RESOL = (-20.0, -20.0, -20.0), 0.4     # tests/test_gpu_mesh.py


def _one_ulp(got, want):
    """tests/test_gpu_mesh.py's bound on verts_mm: within one float32 ulp of the restatement's value."""
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(want))).astype(np.float64)
    return got.dtype == np.float32 and got.shape == want.shape and bool((np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all())


def _geometry(ctx, s):
    """normals, unique_voxels, components, mesh, mesh_sample and mesh_simplify in turn on one scene, each against its restatement as its own
    test module compares them, and against its device=True form bit for bit."""
    nrm, mom, keep = _normals_and_unique(ctx, s)
    args = components_ref.scene_args(s)
    comp = ctx.components(*args, connectivity=6, min_cells=2)
    components_ref.compare(comp, components_ref.components_ref(*args, connectivity=6, min_cells=2))
    assert _same(comp[:3], ctx.components(*args, connectivity=6, min_cells=2, device=True)[:3])
    # the mesh of the normals just computed (tests/test_gpu_mesh.py _compare)
    m = ctx.mesh(*args, nrm, origin=ORIGIN, resol=RESOL)
    want = mesh_ref.mesh_ref(*args, nrm, origin=ORIGIN, resol=RESOL)
    assert want["quads"].shape[0] > 0
    for k in ("vert_cell", "quads", "vert_src"):
        assert m[k].dtype == want[k].dtype and np.array_equal(m[k], want[k]), k
    assert np.abs(m["verts_lattice"] - want["vert_lattice"]).max() <= 1e-9 and _one_ulp(m["verts_mm"], want["verts_mm"])
    names = sorted(m)
    T = s["ijk"].shape[0]
    for kw in (dict(device=True), dict(cap=(4 * T + 1000, 4 * T + 1000)), dict(cap=(1, 1))):      # cap=None is (2 T + 64, 2 T + 64); (1, 1): the retry
        other = ctx.mesh(*args, nrm, origin=ORIGIN, resol=RESOL, **kw)
        assert _same([m[k] for k in names], [other[k] for k in names]), kw
    # samples of that mesh, and the mesh made smaller (tests/test_gpu_meshsample.py _same, tests/test_gpu_meshsimplify.py _compare)
    tris = meshsimplify_ref.triangulate(m["quads"]).astype(np.int32)
    smp = ctx.mesh_sample(m["verts_lattice"], tris, 0.4)
    assert _same(smp, meshsample_ref.sample(m["verts_lattice"], tris, 0.4)) and smp[0].shape[0] > tris.shape[0]
    assert _same(smp, ctx.mesh_sample(m["verts_lattice"], tris, 0.4, device=True))
    sim = ctx.mesh_simplify(m["verts_lattice"], tris, 2, origin=ORIGIN, resol=RESOL)
    want = meshsimplify_ref.simplify(m["verts_lattice"], tris, 2, origin=ORIGIN, resol=RESOL)
    for k in ("vert_rep", "vert_count", "faces", "face_src", "vert_cluster"):
        assert sim[k].dtype == np.int32 and np.array_equal(sim[k], want[k]), k
    assert np.array_equal(sim["verts_lattice"], want["vert_lattice"]) and _one_ulp(sim["verts_mm"], want["vertices"])
    assert 0 < sim["faces"].shape[0] < tris.shape[0]
    other = ctx.mesh_simplify(m["verts_lattice"], tris, 2, origin=ORIGIN, resol=RESOL, device=True)
    assert _same([sim[k] for k in sorted(sim)], [other[k] for k in sorted(sim)])
    return (nrm, mom, keep) + tuple(comp[:3]) + tuple(m[k] for k in names) + tuple(smp) + tuple(sim[k] for k in sorted(sim))


def test_geometry_stages_share_the_host_mirror(ctx):
    small, large = _stepped_sheet(2, 1), _stepped_sheet(8, 5)
    first = _geometry(ctx, small)
    _empty_packed_calls(ctx)
    _geometry(ctx, large)
    _empty_packed_calls(ctx)
    assert _same(first, _geometry(ctx, small))


def _postpass(ctx, s):
    """denoise, adapthresh, ptcubes and gt_cubes / weighted_accuracy in turn on one scene: bit for bit their restatements (tests/test_gpu_postpass.py,
    test_gpu_ptcubes.py, test_gpu_gtcubes.py)."""
    off, ijk, cube = s["offsets"], s["ijk"], s["cube_ijk"]
    n, T = len(cube), ijk.shape[0]
    rs = np.random.RandomState(T)
    split = lambda flat: postpass_ref.split(flat, off)
    pred = (0.35 + 0.6 * rs.rand(T)).astype(np.float16)
    votes = rs.randint(2, 7, T).astype(np.uint8)
    mask = rs.rand(T) < 0.8
    den = ctx.denoise(off, ijk, cube, mask, 8, 8)
    assert np.array_equal(den, np.concatenate(postpass_ref.denoise_ref(cube, split(ijk), split(mask), 8, 8))) and den.any()
    at = ctx.adapthresh(off, ijk, pred, votes, cube, 8, 2, 0.5, 0.9, 4, 2, 8)
    want = postpass_ref.adapthresh_ref(split(pred), split(ijk), split(votes), cube, 2, 8, 0.5, 0.9, 4, 2, 8)
    assert np.array_equal(at["init_denoised"], np.concatenate(want["init_denoised"]))
    assert at["thresh"].dtype == np.float64 and np.array_equal(at["thresh"], want["thresh"]) and np.array_equal(at["choice"], want["choice"])
    for k in range(2):
        assert np.array_equal(at["masks"][k], np.concatenate(want["masks"][k])) and np.array_equal(at["denoised"][k], np.concatenate(want["denoised"][k]))
    # the cubes around the voxels' points, as scene.quantizePts2Cubes asks for them
    pts = normals_ref.voxel_points(off, ijk, s["cube_xyz"], s["cube_resol"]).astype(np.float32)
    kw = dict(resol=np.float32(0.4), cube_D=8, cube_Dcenter=6, cube_overlapping_ratio=0.5)
    from surfacenet_amd import scene
    p = scene._plan(pts.dtype, BB=None, **kw)
    cells = ctx.ptcubes(pts, p["stride_q"], p["stride_xyz"], p["half"], p["compute_f64"])
    cubes = ptcubes_ref.quantizePts2Cubes(pts, **kw)[0]
    assert np.array_equal(cells[0], cubes["ijk"]) and np.array_equal(cells[1], cubes["xyz"]) and len(cubes) > 1
    assert _same(cells, ctx.ptcubes(pts, p["stride_q"], p["stride_xyz"], p["half"], p["compute_f64"], cap=1))      # the retry
    # the occupancy of those cubes by those points, and a prediction's counts against it
    assert ctx.gt_bind(pts, 0.8) == T
    Y = ctx.gt_cubes(cubes)
    assert np.array_equal(Y, gtcubes_ref.gt_cubes(pts, cubes["xyz"], cubes["resol"], S)) and Y.any()
    guess = np.clip(0.6 * Y + 0.55 * rs.rand(*Y.shape), 0, 1).astype(np.float32)
    counts = ctx.weighted_accuracy_counts(guess, Y)
    assert np.array_equal(counts, gtcubes_ref.accuracy_counts(guess, Y))
    return den, at["init_denoised"], at["thresh"], at["masks"], at["denoised"], at["choice"], cells[0], cells[1], Y, counts


def test_postpass_entries_share_the_host_mirror(ctx):
    small, large = _stepped_sheet(2, 1), _stepped_sheet(8, 5)
    first = _postpass(ctx, small)
    for e in (normals_ref.hand_scene(np.zeros((0, 3)), [], stride_vox=4), normals_ref.hand_scene([[0, 0, 0], [1, 0, 0]], [np.zeros((0, 3), np.uint8)] * 2, 4)):
        assert ctx.denoise(e["offsets"], e["ijk"], e["cube_ijk"], e["mask"], 8, 8).shape == (0,)
        assert ctx.adapthresh(e["offsets"], e["ijk"], np.zeros(0, np.float16), None, e["cube_ijk"], 8, 2, 0.5, 0.9, 0, 2, 8)["thresh"].shape == (2, len(e["cube_ijk"]))
    _postpass(ctx, large)
    assert _same(first, _postpass(ctx, small))


# ---- point-cloud evaluation --------------------------------------------------------------------------------------------------------------------
def _cloud(n, seed):
    rs = np.random.RandomState(seed)
    p = np.concatenate([rs.uniform(0, 4, (n - n // 5, 3)), np.repeat(rs.uniform(0, 4, (n // 10, 3)), 2, axis=0)])      # a tenth of them twice
    return p[rs.permutation(n)], rs.permutation(n)


def _reduce_and_nn(ctx, n):
    p, order = _cloud(n, n)
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    keep, rounds = ctx.point_reduce(p, rank, 0.2)
    assert np.array_equal(keep, pointeval_ref.reduce_sequential(p, order, 0.2)) and rounds >= 1 and not keep.all()
    to, frm = p[: n // 2], p[n // 2:] + 0.01
    d2 = ctx.nn_dist2(to, frm, 0.5)
    want = pointeval_ref.nn_d2(to, frm)
    below = want < 0.25 * (1.0 + 2.0 ** -40)
    assert below.any() and np.array_equal(d2[below], want[below]) and np.all(d2[~below] == np.inf)
    return keep, d2


def test_point_reduce_and_nn_dist2_small_large_small(ctx):
    first = _reduce_and_nn(ctx, 50)
    _reduce_and_nn(ctx, 5000)
    assert _same(first, _reduce_and_nn(ctx, 50))


# ---- ray pooling and dense2sparse ---------------------------------------------------------------------------------------------------------------
def _cubes(n):
    rs = np.random.RandomState(40 + n)
    g = np.indices((S, S, S)).astype(np.float32) / S
    pred = np.stack([np.clip(np.exp(-((g[i % 3] - 0.5) * 4) ** 2) * 0.9 + 0.08 * rs.rand(S, S, S), 0, 0.9999) for i in range(n)]).astype(np.float32)
    pairs = rs.randint(0, 4, (n, 2, 2))
    xyz = (rs.rand(n, 3) * [60, 60, 40] + [-30, -30, 590]).astype(np.float32)
    resol = np.full(n, 0.4, np.float32)
    rgb = rs.randint(0, 256, (n, 3, S, S, S)).astype(np.uint8)
    return pred, pairs, xyz, resol, rgb


def _ray_pool(ctx, n):
    pred, pairs, xyz, resol, _ = _cubes(n)
    votes = ctx.ray_pool(pairs, xyz, resol, pred, 0.5)
    p16 = pred.astype(np.float16)
    for i in range(n):
        assert np.array_equal(votes[i], post_oracle.ray_pool_1cube(P_DTU, p16[i], pairs[i], xyz[i], resol[i], 0.5).astype(np.uint8)), i
    assert votes.any()
    return (votes,)


def test_ray_pool_small_large_small(ctx):
    first = _ray_pool(ctx, 1)
    _ray_pool(ctx, 4)
    assert _same(first, _ray_pool(ctx, 1))


def _dense2sparse(ctx, n):
    pred, pairs, xyz, resol, rgb = _cubes(n)
    off, ijk, p16, rgb_out, votes = ctx.dense2sparse(pred, rgb, pairs, xyz, resol, min_prob=0.5, rayPool_thresh=0, enable_rayPooling=True)
    want = post_oracle.dense2sparse(pred.astype(np.float16), np.ascontiguousarray(np.transpose(rgb, (0, 2, 3, 4, 1))), xyz, resol, pairs, min_prob=0.5,
                                    rayPool_thresh=0, enable_rayPooling=True, cameraPOs=P_DTU)
    counts = np.diff(off)
    assert off[0] == 0 and np.nonzero(counts)[0].tolist() == list(want[0]) and counts.sum() > 0
    assert np.array_equal(ijk, np.concatenate(want[1])) and np.array_equal(p16.view(np.uint16), np.concatenate(want[2]).view(np.uint16))
    assert np.array_equal(rgb_out, np.concatenate(want[3])) and np.array_equal(votes, np.concatenate(want[4]))
    return off, ijk, p16, rgb_out, votes


def test_dense2sparse_small_large_small(ctx):
    first = _dense2sparse(ctx, 1)
    _dense2sparse(ctx, 4)
    assert _same(first, _dense2sparse(ctx, 1))


# ---- the host mirror returns what was staged, and no more ---------------------------------------------------------------------------------------
SENTINEL = 0x5C


def _sentinels(spec):
    """One array per (rows, width, dtype) of spec, every byte SENTINEL."""
    outs = [np.empty((rows, width) if width > 1 else (rows,), dtype) for rows, width, dtype in spec]
    for o in outs:
        o.view(np.uint8)[...] = SENTINEL
    return outs


def _host_and_device(ctx, ins, spec, call):
    """call(form, input pointers, output pointers) -> status on sentinel-filled outputs, through ctypes: the host form on the arrays themselves,
    the device form on copies staged here and read back whole. -> (host outputs, device outputs)."""
    from surfacenet_amd import _lib
    host, dev = _sentinels(spec), _sentinels(spec)
    assert call(False, [_lib.ptr(a) for a in ins], [_lib.ptr(o) for o in host]) == 0, _lib.last_error()
    with ctx._on_device([a for a in ins if a is not None]) as src, ctx._on_device(dev) as dst:
        src = iter(src)
        assert call(True, [None if a is None else next(src) for a in ins], dst) == 0, _lib.last_error()
        for o, d in zip(dev, dst):
            ctx.d2h(o, d)
    return host, dev


def _rows_then_sentinel(host, dev, rows):
    """Rows [0, rows[k]) of host output k equal the device form's byte for byte, and every byte beyond them is still the sentinel."""
    for k, (h, d, r) in enumerate(zip(host, dev, rows)):
        assert 0 < r <= h.shape[0], k
        assert np.array_equal(h[:r].view(np.uint8), d[:r].view(np.uint8)), k
        assert (h[r:].view(np.uint8) == SENTINEL).all(), k
    assert any(r < h.shape[0] for h, r in zip(host, rows))      # the tail exists


def test_mesh_simplify_host_form_returns_the_counted_rows_only(ctx):
    """Outputs that hold 9 vertices and 8 faces, of which the simplified 2 x 2 sheet needs fewer: the host form writes what the device form
    writes, and nothing behind it."""
    import ctypes
    from surfacenet_amd import _lib
    v = np.asarray([(i, j, 0) for i in range(3) for j in range(3)], np.float64)
    quads = np.asarray([(3 * i + j, 3 * (i + 1) + j, 3 * (i + 1) + j + 1, 3 * i + j + 1) for i in range(2) for j in range(2)])
    f = np.ascontiguousarray(meshsimplify_ref.triangulate(quads), np.int32)
    want = meshsimplify_ref.simplify(v, f, 2)
    C, G = want["vertices"].shape[0], want["faces"].shape[0]
    assert v.shape[0] == 9 and f.shape[0] == 8 and 0 < C < 9 and 0 < G < 8
    cfg = ctx._on_lattice(_lib.MeshSimplifyCfg(2, 0), (0.0, 0.0, 0.0), 1.0)
    spec = ((9, 3, np.float32), (9, 3, np.float64), (9, 1, np.int32), (9, 1, np.int32), (8, 3, np.int32), (8, 1, np.int32), (9, 1, np.int32))
    counts = []

    def call(device, ins, outs):
        nv, nf = ctypes.c_longlong(-1), ctypes.c_longlong(-1)
        fn = ctx._lib.sn_mesh_simplify_dev if device else ctx._lib.sn_mesh_simplify
        rc = fn(ctx._h, ctypes.byref(cfg), 9, ins[0], 8, ins[1], 9, 8, *outs, ctypes.byref(nv), ctypes.byref(nf))
        counts.append((nv.value, nf.value))
        return rc

    host, dev = _host_and_device(ctx, [v, f], spec, call)
    assert counts == [(C, G), (C, G)]
    _rows_then_sentinel(host, dev, [C, C, C, C, G, G, 9])
    assert np.array_equal(host[4][:G], want["faces"]) and np.array_equal(host[6], want["vert_cluster"])


@pytest.mark.parametrize("pooling", [False, True])
def test_dense2sparse_host_form_returns_the_listed_rows_only(ctx, pooling):
    """sn_dense2sparse stages its lists at their upper bound, n s^3 rows, and returns the T rows its offsets table counts: those equal the
    device form's, and rows [T, n s^3) of the caller's arrays are not written."""
    import ctypes
    from surfacenet_amd import _lib
    n, n_vp, cap = 2, 2, 2 * S ** 3
    rs = np.random.RandomState(7)
    pred = np.full((n, S, S, S), 0.125, np.float32)
    for i, kept in enumerate((5, 7)):                           # a handful of voxels per cube above min_prob, each value a float16
        at = rs.choice(S ** 3, kept, replace=False)
        pred[i].reshape(-1)[at] = (0.6 + 0.3 * rs.rand(kept)).astype(np.float16)
    pairs = np.ascontiguousarray(rs.randint(0, 4, (n, n_vp, 2)), np.int64)
    xyz = (rs.rand(n, 3) * [60, 60, 40] + [-30, -30, 590]).astype(np.float32)
    resol = np.full(n, 0.4, np.float32)
    rgb = rs.randint(0, 256, (n, 3, S, S, S)).astype(np.uint8)
    cfg = _lib.SparseCfg(0.5, 0, 0, S, int(pooling))
    spec = ((n + 1, 1, np.int64), (cap, 3, np.uint8), (cap, 1, np.uint16), (cap, 3, np.uint8)) + (((cap, 1, np.uint8),) if pooling else ())
    ins = [pairs, xyz, resol, pred, rgb] if pooling else [None, None, None, pred, rgb]

    def call(device, ins, outs):
        outs = list(outs) + [None] * (5 - len(outs))
        if not device:
            return ctx._lib.sn_dense2sparse(ctx._h, n, n_vp, *ins, ctypes.byref(cfg), *outs)
        return ctx._lib.sn_dense2sparse_dev(ctx._h, n, n_vp, *ins, ctypes.byref(cfg), votes_ws[0] if pooling else None, *outs)

    with ctx._on_device([np.zeros(n * S ** 3, np.uint8)]) as votes_ws:      # the device form's scratch: every voxel's votes
        host, dev = _host_and_device(ctx, ins, spec, call)
    off = host[0]
    T = int(off[n])
    assert off.tolist() == [0, 5, 12] and T < cap
    _rows_then_sentinel(host, dev, [n + 1] + [T] * (len(spec) - 1))
    assert np.array_equal(np.sort(host[2][:T].view(np.float16)), np.sort(pred[pred >= 0.5].astype(np.float16)))


# ---- similarityNet: the chunk workspace and the per-call buffer ---------------------------------------------------------------------------------------
def _centres(n):
    rs = np.random.RandomState(n)
    H, W = (int(v) for v in SIMIL["sc_hw"])
    return rs.uniform(40, H - 40, n), rs.uniform(40, W - 40, n)


def test_crop_embed_small_large_small(ctx):
    from surfacenet_amd import weights
    H, W = (int(v) for v in SIMIL["sc_hw"])
    (h3, w3), (h40, w40) = _centres(3), _centres(40)
    # the oracle once, for the 43 patches of both sizes
    raw = simil_oracle.crop_patches(golden_util.synth_image(int(SIMIL["sc_seeds"][0]), H, W), np.concatenate([h3, h40]), np.concatenate([w3, w40]))
    want = simil_oracle.embedding_torch(simil_oracle.preprocess(raw, MEAN_BGR), weights.synthetic_simil_param_values(1))
    first = ctx.crop_embed(0, h3, w3, MEAN_BGR)
    large = ctx.crop_embed(0, h40, w40, MEAN_BGR)
    third = ctx.crop_embed(0, h3, w3, MEAN_BGR)
    assert first.shape == (3, 128) and large.shape == (40, 128)
    assert np.abs(first - want[:3]).max() < TOL_EMB and np.abs(large - want[3:]).max() < TOL_EMB
    assert _same((first,), (third,))
