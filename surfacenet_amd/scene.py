"""Drop-in for the reference's `utils/scene.py`: where a reconstruction's cubes come from.

    initializeCubes      utils/scene.py:7-61    the full grid over a bounding box (= synthetic.cube_grid)
    quantizePts2Cubes    utils/scene.py:63-108  cubes only around an initial point cloud (main_reconstruct.py:52-60, initialPtsNamePattern)
    readPointCloud_xyz   utils/scene.py:111-114
    readBB_fromModel     utils/scene.py:116-119
    cubes_from_sparse    the coarse-to-fine step: quantizePts2Cubes of a finished scene's masked voxels, the points never leaving the GPU

Same names, arguments and outputs. The cell list of quantizePts2Cubes is built on the GPU (surfacenet_amd/csrc/ptcubes.h) and equals, bit
for bit, what the reference's function returns under numpy 2 - including its quirk that a point contributes its
floor cell and the DIAGONALLY next one, not all eight around it.
"""
import numpy as np

from . import evaluation, runtime
from .synthetic import CUBE_DTYPE, cube_grid

initializeCubes = cube_grid


def _plan(pts_dtype, resol, cube_D, cube_Dcenter, cube_overlapping_ratio, BB):
    """The host scalars of quantizePts2Cubes in the caller's scalar types (utils/scene.py:87-92), and how numpy 2 promotes
    (pts - shift) // stride: float32 when the points are float32 and the stride is a Python scalar or float32, else float64."""
    side, core = resol * cube_D, resol * cube_Dcenter
    stride = core * cube_overlapping_ratio
    half = side / 2
    compute = np.result_type(pts_dtype, stride.dtype) if isinstance(stride, np.generic) else np.dtype(pts_dtype)
    box = None
    if BB is not None:
        BB = np.asarray(BB)
        box = np.array([[BB[ax, 0] - half for ax in range(3)], [BB[ax, 1] + half for ax in range(3)]], dtype=np.float64)
    # the cell index divides by the stride as the promoted type holds it; xyz multiplies uint32 indices by the stride in float64
    return dict(side=side, stride_q=float(compute.type(stride)), stride_xyz=float(np.float64(stride)), half=float(np.float64(half)),
                compute_f64=compute == np.float64, box=box)


def _cubes(ijk, xyz, resol):
    if ijk.shape[0] == 0:
        raise ValueError("no point to place cubes around (none given, or none inside the bounding box)")
    cubes = np.empty((ijk.shape[0],), dtype=CUBE_DTYPE)
    cubes["ijk"], cubes["xyz"], cubes["resol"] = ijk, xyz, resol
    return cubes


def quantizePts2Cubes(pts_xyz, resol, cube_D, cube_Dcenter, cube_overlapping_ratio, BB=None):
    """Overlapping cubes covering a point cloud: pts_xyz (N,3) float32 or float64 (other dtypes are converted to float64), BB (3,2) or None
    keeps the points within cube_D_mm / 2 of the box. Returns (cubes (N_cubes,) CUBE_DTYPE in ascending ijk, cube_D_mm)."""
    pts = np.asarray(pts_xyz)
    if pts.dtype not in (np.float32, np.float64):
        pts = pts.astype(np.float64)
    pts = pts.reshape(-1, 3)
    if not np.isfinite(pts).all():
        raise ValueError("pts_xyz holds a non-finite coordinate")
    if pts.shape[0] == 0:
        raise ValueError("no point to place cubes around")
    p = _plan(pts.dtype, resol, cube_D, cube_Dcenter, cube_overlapping_ratio, BB)
    ijk, xyz = runtime.any_context().ptcubes(pts, p["stride_q"], p["stride_xyz"], p["half"], p["compute_f64"], box=p["box"])
    return _cubes(ijk, xyz, resol), p["side"]


def cubes_from_sparse(vxl_mask_list, vxl_ijk_list, param_np, resol, cube_D, cube_Dcenter, cube_overlapping_ratio, BB=None):
    """quantizePts2Cubes(sparseCubes.sparse_xyz(vxl_mask_list, vxl_ijk_list, param_np), ...) - the cubes of a finer pass around the surface a
    coarser pass found - with the voxels' points formed on the GPU."""
    offsets = np.zeros((len(vxl_mask_list) + 1,), np.int64)
    offsets[1:] = np.cumsum([len(m) for m in vxl_mask_list])
    mask = np.concatenate(vxl_mask_list, axis=0) if len(vxl_mask_list) else np.zeros((0,), bool)
    ijk = np.vstack(vxl_ijk_list) if len(vxl_ijk_list) else np.zeros((0, 3), np.uint8)
    p = _plan(np.float32, resol, cube_D, cube_Dcenter, cube_overlapping_ratio, BB)
    cells, xyz = runtime.any_context().ptcubes_sparse(offsets, ijk, mask, param_np["xyz"], param_np["resol"], p["stride_q"], p["stride_xyz"],
                                                      p["half"], p["compute_f64"], box=p["box"])
    return _cubes(cells, xyz, resol), p["side"]


def readPointCloud_xyz(pointCloudFile='xx/xx.ply'):
    """(N,3) float32 x, y, z of a PLY's vertices."""
    return np.ascontiguousarray(evaluation.read_ply_xyz(pointCloudFile), dtype=np.float32)


def readBB_fromModel(objFile='xx/xx.obj'):
    """(3,2) [[x_min, x_max], ...] over the `v` lines of a Wavefront OBJ."""
    v = []
    with open(objFile) as f:
        for line in f:
            t = line.split()
            if len(t) >= 4 and t[0] == "v":
                v.append([float(t[1]), float(t[2]), float(t[3])])
    if not v:
        raise ValueError("%s holds no vertex" % objFile)
    v = np.asarray(v, dtype=np.float64)
    return np.c_[v.min(axis=0), v.max(axis=0)]
