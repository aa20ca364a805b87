"""GPU (-m gpu): the colliding-key cases of tests/hash_adversary.py through every stage that keeps its data in a lattice hash table
(surfacenet_amd/csrc/lattice_table.h; the hand-rolled walks of gtcubes.h and crosscube.h). The keys of a case all start their walk in the last
sixteen slots of whatever table the stage sizes, so the claims race along one run hundreds of slots long that walks off slot `mask` on to
slot 0, duplicates of one key among them - the walks no random or geometric input of the suite reaches (tests/test_hash_adversary_cpu.py
shows both halves of that on a model). Every stage runs through the entry its own GPU test uses and is held to the same restatement by the
same comparison, twice (equal bytes), in the host-array form and, where there is one, the device form. Nothing here is at workload size.

Ray pooling's pixel and cell tables (in LDS, where the four arrays lie back to back and may be 83 % full, and in global memory), the mesher's
brick table and the self-intersection grid get keys that are late at the one capacity their sizing rule gives them (hash_adversary.TARGETED)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import components_ref as cr
import gtcubes_ref
import hash_adversary as ha
import mesh_ref as mr
import meshfill_ref as fref
import meshintersect_ref as xref
import meshorient_ref as oref
import meshsimplify_ref as simref
import meshsmooth_ref as smref
import normals_ref as nref
import pointeval_ref
import postpass_cases as cases
import postpass_ref
import ptcubes_ref

pytestmark = pytest.mark.gpu
ORIGIN, RESOL = (-20.0, -20.0, -20.0), 0.4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(name):
    return ha.BUILDERS[name]() if name in ha.BUILDERS else ha.targeted(name)[0]


@pytest.fixture(scope="module")
def ctx(gpu_required):
    from surfacenet_amd import runtime
    return runtime.any_context()


def _bytes(x):
    if isinstance(x, dict):
        return {k: _bytes(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_bytes(v) for v in x]
    return np.asarray(x).tobytes()


def _twice(run):
    """Two runs with equal bytes -> the first result."""
    a, b = run(), run()
    assert _bytes(a) == _bytes(b)
    return a


class _Staged(object):
    """Device copies of host arrays, freed on exit."""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.ctx.dev_alloc(max(a.nbytes, 1))
        self.bufs.append(p)
        self.ctx.h2d(p, a)
        return p

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.bufs:
            self.ctx.dev_free(p)


def _packed_dev(st, s):
    return [st.up(s["offsets"]), st.up(s["ijk"]), st.up(np.asarray(s["cube_ijk"]).astype(np.uint32)), st.up(np.asarray(s["mask"]).view(np.uint8))]


# ---- packed world cells: unique voxels, components, the mesher; 4^3 bricks: normals -----------------------------------------------------------------------
def _unique(ctx, name):
    from surfacenet_amd import _lib
    s = ha.BUILDERS[name]()
    want = nref.unique_ref(s["offsets"], s["ijk"], s["cube_ijk"], s["mask"], s["stride_vox"])
    got = _twice(lambda: ctx.unique_voxels(s["offsets"], s["ijk"], s["cube_ijk"], s["mask"], s["stride_vox"]))
    assert got.dtype == np.bool_ and np.array_equal(got, want)
    g = nref.world_cells(s["offsets"], s["ijk"], s["cube_ijk"], s["stride_vox"])[s["mask"]]
    assert int(got.sum()) == np.unique(g, axis=0).shape[0]
    T = int(s["offsets"][-1])
    with _Staged(ctx) as st:
        d_in, d_u = _packed_dev(st, s), st.up(np.full(T, 7, np.uint8))
        for _ in range(2):
            _lib.check(ctx._lib.sn_unique_voxels_dev(ctx._h, len(s["cube_ijk"]), int(s["stride_vox"]), T, *(d_in + [d_u])))
            dev = np.empty(T, np.uint8)
            ctx.d2h(dev, d_u)
            assert np.array_equal(dev.view(bool), want)


def _components(ctx, name):
    s = ha.BUILDERS[name]()
    for connectivity, min_cells in ((26, 1), (6, 2)):
        want = cr.components_ref(*cr.scene_args(s), connectivity=connectivity, min_cells=min_cells)
        host = _twice(lambda: ctx.components(*cr.scene_args(s), connectivity=connectivity, min_cells=min_cells))
        cr.compare(host, want)
        dev = ctx.components(*cr.scene_args(s), connectivity=connectivity, min_cells=min_cells, device=True)
        cr.compare(dev, want)
        assert _bytes(dev[:3]) == _bytes(host[:3])
    assert want[3] > s["n_late"] // 2                          # the late cells are scattered: nearly one component each


def _normals(ctx, name):
    import test_gpu_normals as tn
    from surfacenet_amd import _lib
    s = ha.BUILDERS[name]()
    min_nb = 3                                                  # a late brick holds three cells
    r = nref.normals_ref(*nref.scene_args(s), radius=2, min_neighbours=min_nb)
    assert r["solved"].sum() > s["n_late"]
    nrm, mom = tn._check(ctx, s, r, radius=2, min_neighbours=min_nb)
    again = tn._run(ctx, s, 2, min_nb)
    assert _bytes(again) == _bytes((nrm, mom))
    T, K, V = int(s["offsets"][-1]), s["view_idx"].shape[1], s["cameraTs"].shape[0]
    with _Staged(ctx) as st:
        d_in = _packed_dev(st, s)
        d_geo = [st.up(s["cube_xyz"]), st.up(s["cube_resol"]), st.up(s["view_idx"]), st.up(s["cameraTs"])]
        d_n, d_m = st.up(np.full((T, 3), 7, np.float32)), st.up(np.full((T, 10), 7, np.int32))
        cfg = _lib.NormalsCfg(2, min_nb, int(s["stride_vox"]), V, K)
        _lib.check(ctx._lib.sn_normals_dev(ctx._h, len(s["cube_ijk"]), ctypes.byref(cfg), T, *(d_in + d_geo + [d_n, d_m])))
        got_n, got_m = np.empty((T, 3), np.float32), np.empty((T, 10), np.int32)
        ctx.d2h(got_n, d_n)
        ctx.d2h(got_m, d_m)
        assert _bytes((got_n, got_m)) == _bytes((nrm, mom))


def _mesh(ctx, name):
    import test_gpu_mesh as tm
    s = _case(name)
    want = mr.mesh_ref(*mr.scene_args(s), radius=2, reach=0, origin=ORIGIN, resol=RESOL)
    assert want["quads"].shape[0] > 0 and want["n_cells"] >= s["n_late"]
    host = _twice(lambda: tm._run(ctx, s))
    tm._compare(host, want)
    dev = tm._run(ctx, s, device=True)
    tm._compare(dev, want)
    assert _bytes(dev) == _bytes(host)


# ---- the cube map ------------------------------------------------------------------------------------------------------------------------------------------
def _denoise(ctx, name):
    from surfacenet_amd import _lib, denoising
    c = ha.BUILDERS[name]()
    d = c["d"]
    want = postpass_ref.denoise_ref(d["cube_ijk_np"], d["vxl_ijk_list"], c["masks"], c["D_cube"])
    assert not want[c["repeated"]].any() and want[-1].any()     # the repeated ijk: the larger index is in the map
    got = _twice(lambda: denoising.denoise_crossCubes(d["cube_ijk_np"], d["vxl_ijk_list"], c["masks"], c["D_cube"]))
    assert cases.list_differences(got, want) == []
    off, ijk = nref.pack(d["vxl_ijk_list"])
    T, n = ijk.shape[0], len(d["vxl_ijk_list"])
    with _Staged(ctx) as st:
        d_off, d_ijk, d_cube = st.up(off), st.up(ijk), st.up(np.asarray(d["cube_ijk_np"]).astype(np.uint32))
        d_mask, d_out = st.up(np.concatenate(c["masks"]).view(np.uint8)), st.up(np.full(T, 7, np.uint8))
        _lib.check(ctx._lib.sn_denoise_dev(ctx._h, n, c["Dc"], c["D_cube"], T, d_off, d_ijk, d_cube, d_mask, d_out))
        out = np.empty(T, np.uint8)
        ctx.d2h(out, d_out)
        ctx.synchronize()
        assert np.array_equal(out.view(bool), np.concatenate(want))


def _adapthresh(ctx, name):
    from surfacenet_amd import adapthresh
    c = ha.BUILDERS[name]()
    args = cases.at_args(c["d"], c["D_cube"])
    want = cases.packed(postpass_ref.adapthresh_ref(*args))
    got = _twice(lambda: {k: v for k, v in adapthresh.adapthresh_lists(*args).items() if k in want})
    assert cases.adapthresh_differences(got, want) == []
    assert want["denoised"][-1].any() and (want["choice"] >= 0).sum() == want["choice"].size - 2      # every cube but the repeated one is in the map


# ---- edge keys: smooth, fill, orient -------------------------------------------------------------------------------------------------------------------------
def _smooth(ctx, name):
    import test_gpu_meshsmooth as ts
    c = ha.BUILDERS[name]()
    v, f = c["verts"], c["faces"]
    for iterations, boundary in ((0, smref.CURVE), (3, smref.CURVE), (3, smref.FREE)):
        want = smref.smooth(v, f, iterations, ts.LAM, ts.MU, boundary, ORIGIN, RESOL)
        host = _twice(lambda: ctx.mesh_smooth(v, f, iterations, ts.LAM, ts.MU, boundary, origin=ORIGIN, resol=RESOL))
        ts._compare(host, want)
        dev = ctx.mesh_smooth(v, f, iterations, ts.LAM, ts.MU, boundary, origin=ORIGIN, resol=RESOL, device=True)
        assert _bytes({k: dev[k] for k in ts.OUT + ("counts",)}) == _bytes({k: host[k] for k in ts.OUT + ("counts",)})
    assert want["counts"][1] > 100 and want["counts"][2] > 100 and (want["vert_lattice"] != v).any()


def _fill(ctx, name):
    import test_gpu_meshfill as tf
    c = ha.BUILDERS[name]()
    v, f = c["verts"], c["faces"]
    for orientation in (fref.HOLES, fref.ANY):
        want = fref.fill(v, f, 64, orientation, ORIGIN, RESOL)
        host = _twice(lambda: ctx.mesh_fill(v, f, 64, orientation, origin=ORIGIN, resol=RESOL))
        tf._compare(host, want)
        dev = ctx.mesh_fill(v, f, 64, orientation, origin=ORIGIN, resol=RESOL, device=True)
        assert _bytes({k: dev[k] for k in tf.OUT + ("counts",)}) == _bytes({k: host[k] for k in tf.OUT + ("counts",)})


def _orient(ctx, name):
    c = ha.BUILDERS[name]()
    v, f = c["verts"], c["faces"]
    for sign in (oref.MAJORITY, oref.OUTWARD):
        want = oref.orient(v, f, sign)
        for device in (False, True):
            got = _twice(lambda: ctx.mesh_orient(v, f, sign, device=device))
            assert oref.same_bytes(got, want) == [], (sign, device, oref.same_bytes(got, want))
    assert want["counts"][0] > 2000 and want["counts"][5] < f.shape[0]      # faces joined into pieces across the late sides


# ---- the simplifier's two tables ---------------------------------------------------------------------------------------------------------------------------------
def _simplify(ctx, name):
    import test_gpu_meshsimplify as tsim
    c = ha.BUILDERS[name]()
    v, f = c["verts"], c["faces"]
    for placement in (0, 1):
        want = simref.simplify(v, f, c["cell"], placement, ORIGIN, RESOL)
        assert want["clusters"] == c["n_late"] and want["duplicates"] == c["n_late_faces"] // 4
        host = _twice(lambda: ctx.mesh_simplify(v, f, c["cell"], placement, origin=ORIGIN, resol=RESOL))
        tsim._compare(host, want)
        dev = ctx.mesh_simplify(v, f, c["cell"], placement, origin=ORIGIN, resol=RESOL, device=True)
        assert _bytes({k: dev[k] for k in tsim.OUT}) == _bytes({k: host[k] for k in tsim.OUT})


# ---- the cell grid -----------------------------------------------------------------------------------------------------------------------------------------------
def _point_reduce(ctx, name):
    from surfacenet_amd import evaluation
    c = ha.BUILDERS[name]()
    per_cell = len(c["xyz"]) // c["n_late"]
    p = c["xyz"]
    want = pointeval_ref.reduce_rounds(p, c["order"], c["dst"])
    keep, rounds = _twice(lambda: ctx.point_reduce(p, c["rank"], c["dst"]))
    assert np.array_equal(keep, want) and 1 <= rounds < 100
    got, idx = evaluation.reduce_points(p, dst=c["dst"], order=c["order"], return_index=True)
    assert np.array_equal(idx, np.nonzero(want)[0]) and np.array_equal(got, p[want])
    assert want.all() if per_cell == 1 else 0 < want.sum() < len(p)


def _nn_dist2(ctx, name):
    import test_gpu_pointeval as tp
    c = ha.BUILDERS[name]()
    to, frm = c["to"], c["frm"]
    for max_dist in (np.inf, 60.0, 25.0 * c["h"]):
        tp._check_d2(_twice(lambda: ctx.nn_dist2(to, frm, max_dist)), to, frm, max_dist)
    # and the other way round: the late cloud searched
    tp._check_d2(ctx.nn_dist2(frm, to, np.inf), frm, to, np.inf)


def _gt_cubes(_, name):
    import surfacenet_amd
    c = ha.BUILDERS[name]()
    pts, xyz, resol, s = c["pts"], c["xyz"], c["resol"], c["s"]
    want = gtcubes_ref.gt_cubes(pts, xyz, resol, s)
    assert (want.reshape(len(xyz), -1).sum(axis=1) >= 1).all()
    ctx = surfacenet_amd.Context(cube_D=s, max_samples=4)
    try:
        assert ctx.gt_bind(pts, c["cell"]) == len(pts)
        got = _twice(lambda: ctx.gt_cubes((xyz, resol)))
        assert got.dtype == np.float32 and np.array_equal(got, want)
        with _Staged(ctx) as st:
            d_pts, d_xyz, d_resol = st.up(pts), st.up(xyz), st.up(resol)
            d_Y = st.up(np.full(want.shape, 7, np.float32))
            ctx.gt_bind_dev(len(pts), d_pts, c["cell"])
            ctx.gt_cubes_dev(len(xyz), d_xyz, d_resol, d_Y)
            dev = np.empty_like(want)
            ctx.d2h(dev, d_Y)
            ctx.synchronize()
            assert np.array_equal(dev, want)
    finally:
        ctx.close()


# ---- quantizePts2Cubes, the hash-set form ---------------------------------------------------------------------------------------------------------------------
def _ptcubes(ctx, name):
    import test_gpu_ptcubes as tpc
    from surfacenet_amd import scene
    c = ha.BUILDERS[name]()
    pts = c["pts"]
    dtype = str(pts.dtype)
    want = ptcubes_ref.quantizePts2Cubes(pts, **ha.PT_ARGS)
    got = scene.quantizePts2Cubes(pts, **ha.PT_ARGS)
    tpc._same(got, want)
    again = scene.quantizePts2Cubes(pts, **ha.PT_ARGS)
    assert got[0].tobytes() == again[0].tobytes()
    p = scene._plan(pts.dtype, ha.PT_ARGS["resol"], 32, 26, 0.5, None)
    args = (p["stride_q"], p["stride_xyz"], p["half"], p["compute_f64"])
    ijk, xyz = ctx.ptcubes(pts, *args, box=p["box"])
    d = ctx.upload(pts)
    try:
        ijk_d, xyz_d = ctx.ptcubes_dev(pts.shape[0], d, dtype == "float64", *args, box=p["box"])
    finally:
        ctx.dev_free(d)
    assert np.array_equal(ijk_d, ijk) and np.array_equal(xyz_d, xyz) and np.array_equal(ijk, want[0]["ijk"])


# ---- ray pooling: the pixel table and the cell table, in LDS and in global memory ------------------------------------------------------------------------------
def _ray_pool(_, name):
    import surfacenet_amd
    c = _case(name)
    want = ha.rp_want(name)
    D = c["D"]
    n, n_vp = c["pairs"].shape[:2]
    assert want.any() and want.max() <= 2 * n_vp
    with surfacenet_amd.Context(cube_D=D, max_samples=4) as ctx:
        ctx.set_cameras(c["cameras"])
        got = _twice(lambda: ctx.ray_pool(c["pairs"], c["xyz"], c["resol"], c["pred"], c["thresh"]))
        assert got.dtype == np.uint8 and got.shape == (1, D, D, D) and got.tobytes() == want.tobytes()
        with _Staged(ctx) as st:
            d_in = [st.up(c["pairs"].astype(np.int64)), st.up(c["xyz"]), st.up(c["resol"]), st.up(c["pred"])]
            d_votes = st.up(np.full(D ** 3, 7, np.uint8))
            for _ in range(2):
                ctx.ray_pool_dev(n, n_vp, *(d_in + [d_votes]), prediction_thresh=c["thresh"])
                dev = np.empty(D ** 3, np.uint8)
                ctx.d2h(dev, d_votes)
                assert dev.tobytes() == want.tobytes()


# ---- the self-intersection grid ------------------------------------------------------------------------------------------------------------------------------
def _intersect(ctx, name):
    c = _case(name)
    v, f = c["verts"], c["faces"]
    want = xref.intersect(v, f)
    assert xref.grid_level(v, f)[0] == 0 and want["counts"][3] > 200
    for device in (False, True):
        got = _twice(lambda: ctx.mesh_intersect(v, f, device=device))
        assert xref.same_bytes(got, want) == [], (device, xref.same_bytes(got, want), got["counts"].tolist(), want["counts"].tolist())


_CHILD = """import sys
import numpy as np
sys.path[:0] = [%r, %r]
import hash_adversary as ha
from surfacenet_amd import runtime
c = ha.intersect_case(8)
ctx = runtime.any_context()
out = {}
for device in (False, True):
    for run in (0, 1):
        got = ctx.mesh_intersect(c["verts"], c["faces"], device=device)
        out.update({"%%s_%%d_%%d" %% (k, device, run): got[k] for k in ("face_hit", "face_pairs", "pairs", "counts")})
np.savez(sys.argv[1], **out)
"""


def test_late_grid_cells_at_a_forced_level(gpu_required, tmp_path):
    """The mesh with (v + 4) scaled by 8 presents the same late keys at level 3, which SN_MXI_LEVEL forces in the test-only twin (one child
    process, as in tests/test_gpu_meshintersect.py): the restatement on the scaled mesh, host and device form, twice."""
    c = ha.intersect_case(8)
    want = xref.intersect(c["verts"], c["faces"])
    assert xref.same_bytes(want, xref.intersect(*[_case("intersect")[k] for k in ("verts", "faces")])) == []
    env = dict(os.environ, SURFACENET_HIP_LIB=os.path.join(ROOT, "surfacenet_amd", "libsurfacenet_hip_dbg.so"), SN_MXI_LEVEL=str(c["level"]))
    script, out = tmp_path / "child.py", str(tmp_path / "forced.npz")
    script.write_text(_CHILD % (ROOT, os.path.join(ROOT, "tests")))
    subprocess.check_call([sys.executable, str(script), out], env=env, cwd=ROOT)
    got = np.load(out)
    for device in (0, 1):
        for run in (0, 1):
            r = {k: got["%s_%d_%d" % (k, device, run)] for k in xref.KEYS}
            assert xref.same_bytes(r, want) == [], (device, run, xref.same_bytes(r, want), r["counts"].tolist(), want["counts"].tolist())


# ---- one test per stage and case -------------------------------------------------------------------------------------------------------------------------------
STAGES = [(_unique, ("cells32", "cells512", "cells1500", "bricks")), (_components, ("cells32", "cells512", "cells1500", "bricks")),
          (_normals, ("bricks", "cells1500")), (_mesh, ("cells32b", "cells512b", "cells1500b", "bricks_mesh")), (_denoise, ("cubemap",)), (_adapthresh, ("cubemap",)),
          (_smooth, ("edges3", "edges4")), (_fill, ("edges3", "edges4")), (_orient, ("edges3", "edges4")), (_simplify, ("simplify",)),
          (_point_reduce, ("reduce1", "reduce3")), (_nn_dist2, ("nn",)), (_gt_cubes, ("gt",)), (_ptcubes, ("ptcubes_f64", "ptcubes_f32")),
          (_ray_pool, ha.RAY_POOL + tuple(ha.FULL)), (_intersect, ("intersect",))]
RUNS = [(fn, name) for fn, names in STAGES for name in names]


@pytest.mark.parametrize("stage,name", RUNS, ids=["%s-%s" % (fn.__name__[1:], name) for fn, name in RUNS])
def test_late_keys(ctx, stage, name):
    stage(ctx, name)
