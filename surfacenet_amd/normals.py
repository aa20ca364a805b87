"""Oriented normals and de-duplication of the output cloud on the MI355X, on the reference's per-cube list conventions.

    estimate_normals   one (n_i,3) float32 array per cube: the normal_list that sparseCubes.save_sparseCubes_2ply(normal_list=) writes
    unique_voxels      a mask list that keeps one voxel per world cell (overlapping cubes predict the same cell several times)

The reference accepts normals in its PLY writers (utils/sparseCubes.py:246-327) but has nothing that produces them. Both functions look at the
scene on the world voxel lattice - cell = cube_ijk * stride_vox + vxl_ijk - across cubes, in one GPU call each (surfacenet_amd/csrc/normals.h).
Every argument check runs before the library is touched.
"""
import numpy as np

from . import runtime
from .denoising import pack_lists, split_lists


def stride_voxels(cube_Dcenter, cube_overlapping_ratio):
    """The cube stride in voxels, cube_Dcenter * cube_overlapping_ratio (13 for 26 x 0.5); ValueError unless it is a positive integer."""
    s = float(cube_Dcenter) * float(cube_overlapping_ratio)
    if not (s >= 1 and s == int(s)):
        raise ValueError("cube_Dcenter * cube_overlapping_ratio = %r is not a positive integer number of voxels" % (s,))
    return int(s)


def _stride(stride_vox):
    s = float(stride_vox)
    if not (s >= 1 and s == int(s)):
        raise ValueError("stride_vox = %r must be a positive integer (cube_Dcenter * cube_overlapping_ratio)" % (stride_vox,))
    return int(s)


def _pack(cube_ijk_np, vxl_ijk_list, vxl_mask_list):
    n = len(vxl_ijk_list)
    if len(vxl_mask_list) != n or len(cube_ijk_np) != n:
        raise ValueError("%d voxel lists, %d mask lists, %d cube ijk rows" % (n, len(vxl_mask_list), len(cube_ijk_np)))
    for i, (a, m) in enumerate(zip(vxl_ijk_list, vxl_mask_list)):
        if len(a) != np.asarray(m).size:
            raise ValueError("cube %d: %d voxels, %d mask entries" % (i, len(a), np.asarray(m).size))
    offsets, ijk, _ = pack_lists(vxl_ijk_list)
    mask = np.concatenate([np.asarray(m, dtype=bool).reshape(-1) for m in vxl_mask_list]) if n else np.zeros((0,), bool)
    return offsets, ijk, mask


def estimate_normals(cube_ijk_np, vxl_ijk_list, vxl_mask_list, param_np, viewPair_np, cameraTs_np, stride_vox, radius=2, min_neighbours=6,
                     return_moments=False):
    """cube_ijk_np (N,3), vxl_ijk_list[i] (iN,3) uint8, vxl_mask_list[i] (iN,) bool, param_np the cube table ('xyz', 'resol'), viewPair_np
    (N,N_vp,2) the views each cube selected, cameraTs_np (V,3) the camera centres, stride_vox = cube_Dcenter * cube_overlapping_ratio.
    -> normal_list, [(iN,3) float32, ...]: for a masked voxel with at least min_neighbours occupied cells in its (2*radius+1)^3 window the unit
    normal of the plane through them, pointing toward the mean centre of its cube's views; zero otherwise. With return_moments also the list of
    (iN,10) int32 window moments (count, sum d, sum d d^T)."""
    stride = _stride(stride_vox)
    if int(radius) != radius or not 1 <= int(radius) <= 3:
        raise ValueError("radius = %r: the window radius is 1, 2 or 3 cells" % (radius,))
    if int(min_neighbours) < 1:
        raise ValueError("min_neighbours must be >= 1")
    offsets, ijk, mask = _pack(cube_ijk_np, vxl_ijk_list, vxl_mask_list)
    n = len(vxl_ijk_list)
    if len(param_np) != n or len(viewPair_np) != n:
        raise ValueError("%d cubes: %d parameter rows, %d view-pair rows" % (n, len(param_np), len(viewPair_np)))
    resol = np.asarray(param_np['resol'], dtype=np.float32).reshape(-1)
    if n and not np.all(resol == resol[0]):
        raise ValueError("cubes of different resol: a cell-space normal is a direction in mm only on an isotropic lattice")
    cams = np.asarray(cameraTs_np, dtype=np.float64)
    if cams.ndim != 2 or cams.shape[1] != 3:
        raise ValueError("cameraTs_np must be (V,3)")
    if n == 0:
        return ([], []) if return_moments else []
    view_idx = np.asarray(viewPair_np).reshape(n, -1).astype(np.int32)
    if view_idx.shape[1] == 0:
        raise ValueError("viewPair_np names no view")
    res = runtime.any_context().normals(offsets, ijk, cube_ijk_np, mask, stride, param_np['xyz'], resol, view_idx, cams, radius=int(radius),
                                        min_neighbours=int(min_neighbours), return_moments=bool(return_moments))
    if return_moments:
        return tuple([a.copy() for a in split_lists(flat, offsets)] for flat in res)
    return [a.copy() for a in split_lists(res, offsets)]


def unique_voxels(cube_ijk_np, vxl_ijk_list, vxl_mask_list, stride_vox):
    """-> [(iN,) bool, ...]: vxl_mask_list with every world cell kept once, in the first cube (and at the first position) that lists it."""
    stride = _stride(stride_vox)
    offsets, ijk, mask = _pack(cube_ijk_np, vxl_ijk_list, vxl_mask_list)
    if len(vxl_ijk_list) == 0:
        return []
    keep = runtime.any_context().unique_voxels(offsets, ijk, cube_ijk_np, mask, stride)
    return [a.copy() for a in split_lists(keep, offsets)]
