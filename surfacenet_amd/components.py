"""Connected components of the output cloud on the MI355X - removing the floaters - on the reference's per-cube list conventions (DESIGN.md
section 4.14).

    label_components   one (n_i,) int32 label array per cube plus the components' sizes in cells
    remove_floaters    a mask list without the small detached blobs

The reference judges a cluster inside one cube only (utils/denoising.py __cluster_inCube__, scipy.ndimage.label) and keeps it when it touches a
voxel of a neighbour cube, so a blob that straddles a seam survives denoise_crossCubes. Both functions here look at the scene on the world voxel
lattice - cell = cube_ijk * stride_vox + vxl_ijk - across cubes, in one GPU call (surfacenet_amd/csrc/components.h). Adjacency is
scipy.ndimage.generate_binary_structure(3, 1 | 2 | 3) for connectivity 6 | 18 | 26, the reference's neighbor_dist. A cell that several cubes list
counts once. Every argument check runs before the library is touched.
"""
import numpy as np

from . import runtime
from .denoising import split_lists
from .normals import _pack, _stride, stride_voxels      # noqa: F401  (stride_voxels: the callers' way to stride_vox)


def _count(v, what):
    if v is None:
        return None
    if isinstance(v, bool) or float(v) != int(v) or int(v) < 1:
        raise ValueError("%s = %r must be a positive integer" % (what, v))
    return int(v)


def check_args(min_cells, keep_largest, connectivity):
    """-> (min_cells, keep_largest, connectivity) as ints / None; ValueError for what remove_floaters refuses."""
    if connectivity not in (6, 18, 26):
        raise ValueError("connectivity = %r: 6, 18 or 26" % (connectivity,))
    return _count(min_cells, "min_cells"), _count(keep_largest, "keep_largest"), int(connectivity)


def kept_components(sizes, min_cells=None, keep_largest=None):
    """(C,) bool: the components that pass. min_cells: at least that many cells; keep_largest=k: among the k with the most cells, ties going to
    the lower number; with both, both."""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    ok = np.ones(sizes.shape, bool)
    if min_cells is not None:
        ok &= sizes >= min_cells
    if keep_largest is not None:
        top = np.zeros(sizes.shape, bool)
        top[np.argsort(-sizes, kind="stable")[:keep_largest]] = True
        ok &= top
    return ok


def _sizes(label, cells, C):
    sizes = np.zeros((C,), np.int32)
    m = label >= 0
    sizes[label[m]] = cells[m]
    return sizes


def label_components(cube_ijk_np, vxl_ijk_list, vxl_mask_list, stride_vox, connectivity=26):
    """cube_ijk_np (N,3), vxl_ijk_list[i] (iN,3) uint8, vxl_mask_list[i] (iN,) bool, stride_vox = cube_Dcenter * cube_overlapping_ratio.
    -> (label_list, sizes): label_list[i] (iN,) int32 the component of each voxel's world cell (-1 unmasked), numbered by the first voxel - in
    cube order, then list order - that lies in it; sizes (C,) int32 in distinct cells."""
    stride = _stride(stride_vox)
    _, _, connectivity = check_args(None, None, connectivity)
    offsets, ijk, mask = _pack(cube_ijk_np, vxl_ijk_list, vxl_mask_list)
    if len(vxl_ijk_list) == 0:
        return [], np.zeros((0,), np.int32)
    label, cells, _, C = runtime.any_context().components(offsets, ijk, cube_ijk_np, mask, stride, connectivity=connectivity)
    return [a.copy() for a in split_lists(label, offsets)], _sizes(label, cells, C)


def remove_floaters(cube_ijk_np, vxl_ijk_list, vxl_mask_list, stride_vox, min_cells=None, keep_largest=None, connectivity=26):
    """-> [(iN,) bool, ...]: vxl_mask_list without the voxels of the components that fail: fewer than min_cells cells, or not among the
    keep_largest largest (ties to the lower number); with both given a component must pass both. ValueError with neither."""
    stride = _stride(stride_vox)
    min_cells, keep_largest, connectivity = check_args(min_cells, keep_largest, connectivity)
    if min_cells is None and keep_largest is None:
        raise ValueError("remove_floaters needs min_cells, keep_largest or both")
    offsets, ijk, mask = _pack(cube_ijk_np, vxl_ijk_list, vxl_mask_list)
    if len(vxl_ijk_list) == 0:
        return []
    label, cells, keep, C = runtime.any_context().components(offsets, ijk, cube_ijk_np, mask, stride, connectivity=connectivity,
                                                             min_cells=1 if min_cells is None else min(min_cells, 2 ** 31 - 1))
    if keep_largest is not None:                     # decided on the host: C integers
        ok = kept_components(_sizes(label, cells, C), min_cells, keep_largest)
        keep = (label >= 0) & ok[np.maximum(label, 0)] if C else np.zeros(label.shape, bool)
    return [a.copy() for a in split_lists(keep, offsets)]
