"""Ground-truth mode: what the reference's `__SurfaceNet_fn_inference__(with_groundTruth=True)` (nets/SurfaceNet.py:359-378) and the `val_fn`
of `SurfaceNet_fn_trainVal` (nets/SurfaceNet.py:253-264) compare the network against, on the MI355X.

* `bind_points(pts_xyz, cube_D_mm)`          binds a ground-truth cloud (a DTU `stlXXX_total.ply`, the output of a finer pass ...)
* `gt_cubes(cubes, cube_D)`                  the target tensor `Y` (n,1,s,s,s) float32 of a batch of cubes: the occupancy of the bound cloud
* `gt_cubes_from_points(pts, cubes, cube_D)` both in one call
* `gt_cubes_from_mesh(vert_lattice, faces, cube_ijk, cube_D, stride_vox)` the same tensor from a mesh in lattice cells
* `weighted_accuracy(pred, Y)`               `__weighted_accuracy__` (nets/SurfaceNet.py:203-224) of a batch
* `accuracy_from_counts(counts)`             the same from the (n,4) integer counts the GPU returns (host arithmetic, float64)

Occupancy: with q = np.floor((p - xyz_c) / resol_c) per axis in float32, Y[c, 0, q0, q1, q2] = 1.0 iff some point has 0 <= q < s on all three
axes; every other voxel is 0.0. tests/gtcubes_ref.py restates it (and the counts) in numpy; the GPU results equal it bit for bit."""
import numpy as np

from . import runtime

_cloud = None        # what bind_points registered: (float32 points, cube_D_mm); bound lazily into the context of the cube size asked for


class BoundCloud(object):
    """A ground-truth cloud bound to one Context (`ctx.bind_points`): what `reconstruct.hot_loop(gt=)` / `SparseLoop(gt=)` take. A context
    holds one cloud: binding another one there makes this handle stale (`check()` raises)."""

    def __init__(self, ctx, pts_xyz, cube_D_mm):
        cube_D_mm = float(cube_D_mm)
        if not cube_D_mm > 0:
            raise ValueError("cube_D_mm must be > 0")
        self.ctx, self.cube_D_mm = ctx, cube_D_mm
        self.n_points = ctx.gt_bind(pts_xyz, cube_D_mm / 4.0)     # a quarter of the cube side: a cube's box overlaps 5..6 cells per axis
        self._serial = ctx._gt_serial

    def check(self, ctx=None):
        if ctx is not None and ctx is not self.ctx:
            raise ValueError("the ground-truth cloud is bound to another Context")
        if getattr(self.ctx, "_gt_serial", 0) != self._serial:
            raise ValueError("another cloud has been bound to the Context since this one")
        return self


def bind_points(pts_xyz, cube_D_mm):
    """Binds the ground-truth cloud pts_xyz (n,3) - converted with np.asarray(pts, np.float32); n = 0 is legal - for cubes of side cube_D_mm
    (= resol * cube_D; it only sizes the grid the points are sorted into). Replaces the cloud bound before. Returns the BoundCloud of
    `runtime.any_context()`; `gt_cubes` binds the same points into the context of another cube size on demand."""
    global _cloud
    pts = np.ascontiguousarray(np.asarray(pts_xyz, np.float32).reshape(-1, 3))
    bound = BoundCloud(runtime.any_context(), pts, cube_D_mm)
    _cloud = (pts, float(cube_D_mm), {id(bound.ctx): bound})
    return bound


def _bound_in(ctx):
    if _cloud is None:
        raise RuntimeError("groundTruth.bind_points has not been called")
    pts, cube_D_mm, handles = _cloud
    b = handles.get(id(ctx))
    if b is None or b.ctx is not ctx or getattr(ctx, "_gt_serial", 0) != b._serial:
        b = handles[id(ctx)] = BoundCloud(ctx, pts, cube_D_mm)
    return b


def gt_cubes(cubes, cube_D):
    """Y (n,1,cube_D,cube_D,cube_D) float32 of `cubes` - the reference's cubes_param_np (fields 'xyz', 'resol') or a pair (xyz (n,3), resol (n,)
    or a scalar) - from the cloud of `bind_points`. Per-cube resolutions may differ within one call."""
    ctx = runtime.context_for(int(cube_D))
    _bound_in(ctx)
    return ctx.gt_cubes(cubes)


def gt_cubes_from_points(pts, cubes, cube_D):
    """bind_points + gt_cubes in one call; the cube side that sizes the grid is taken from the first cube's resolution."""
    xyz, resol = runtime.Context._cube_params(cubes)
    side = float(resol[0]) * int(cube_D) if resol.size else 1.0
    ctx = runtime.context_for(int(cube_D))
    global _cloud
    p = np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 3))
    bound = BoundCloud(ctx, p, side)
    _cloud = (p, side, {id(ctx): bound})
    return ctx.gt_cubes((xyz, resol))


def gt_cubes_from_mesh(vert_lattice, faces, cube_ijk, cube_D, stride_vox, select="surface", axis=2):
    """The target tensor Y (n,1,cube_D,cube_D,cube_D) float32 from a MESH in lattice cells (mesh.voxelize states the
    voxels): 1.0 where a voxel has one of the selected bits - "surface": its closed box meets a triangle, "solid": its centre is inside,
    "either" -, else 0.0. `weighted_accuracy(pred, Y)` takes it as it is. No cloud is bound or needed."""
    from . import mesh
    v, f = mesh._mesh_arrays(vert_lattice, faces)
    if select is None:
        raise ValueError("select = None: of %s" % sorted(mesh.VOXEL_SELECTS))
    cube, D, stride, _, a, sel = mesh.check_voxelize_args(cube_ijk, cube_D, stride_vox, axis=axis, select=select)
    mesh._mesh_args(v, f, (0.0, 0.0, 0.0), 1.0, None, "faces")
    if f.shape[0] * (f.shape[1] - 2) > mesh.MAX_DISTANCE_TRIANGLES:
        raise ValueError("%d triangles: at most 2^26" % (f.shape[0] * (f.shape[1] - 2)))
    if cube.shape[0] == 0 or f.shape[0] == 0:
        return np.zeros((cube.shape[0], 1, D, D, D), np.float32)
    return runtime.any_context().mesh_voxelize(v.astype(np.float64), f.astype(np.int32), cube, D, stride, axis=a, modes=sel, select=sel,
                                               outputs=("Y",))["Y"]


def accuracy_from_counts(counts):
    """`__weighted_accuracy__` (nets/SurfaceNet.py:203-224) from counts (..., 4) = n_pos, n_neg, hit_pos, hit_neg, summed over all leading axes:
        acc_neg = hit_neg / n_neg;  acc_pos = hit_pos / n_pos, or acc_neg when n_pos == 0 (the reference's ifelse);  (acc_pos + acc_neg) / 2
    in float64. n_neg == 0 gives NaN, as the mean of an empty selection does.
    Two deliberate points: (1) the dtype Theano would return for this expression cannot be pinned without Theano at hand; np.float64 is
    returned. (2) the reference computes ONE accuracy over the whole batch tensor - the summed counts give exactly that; the per-cube counts
    are an extra the reference does not have."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 4).sum(axis=0)
    n_pos, n_neg, hit_pos, hit_neg = (np.float64(v) for v in c)
    with np.errstate(divide="ignore", invalid="ignore"):
        acc_neg = hit_neg / n_neg
        acc_pos = hit_pos / n_pos if n_pos != 0 else acc_neg
        return np.float64((acc_pos + acc_neg) / 2.0)


def weighted_accuracy(pred, Y, threshold=0.5, per_cube=False):
    """`__weighted_accuracy__(pred, Y)` counted on the GPU: pred, Y float32 (n,1,s,s,s). Positive is Y > 0, negative Y == 0 (a negative or NaN
    target is neither), a hit is float(pred >= threshold) == Y (lasagne's binary_accuracy: `ge`, threshold 0.5; a NaN prediction compares
    false). Returns np.float64 (see `accuracy_from_counts` for the dtype and the whole-batch definition); with per_cube also the (n,4) int64
    counts n_pos, n_neg, hit_pos, hit_neg of every cube, which sum to the batch's."""
    if not isinstance(pred, np.ndarray) or pred.dtype != np.float32 or pred.ndim != 5:
        raise TypeError("pred must be a float32 5-D ndarray")
    return runtime.context_for(pred.shape[2]).weighted_accuracy(pred, Y, threshold, per_cube)
