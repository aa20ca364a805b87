"""Drop-in for the reference's `utils/denoising.py` on the MI355X (call sites main_reconstruct.py:175, utils/adapthresh.py:108,170).

    denoise_crossCubes   utils/denoising.py:150-184

Same name, arguments and result: a list with one bool array per cube. A voxel is kept iff it is masked and its 26-connected component inside
its cube holds a voxel that coincides with a masked voxel of one of the 26 neighbouring cubes (v == u + (D_cube // 2) * shift). The
components, the cube map and the neighbour tests run in one GPU call (surfacenet_amd/csrc/crosscube.h); D_cube is taken as given.
"""
import numpy as np

from . import runtime


def pack_lists(vxl_ijk_list):
    """Per-cube voxel lists -> (offsets (n+1,) int64, ijk (T,3) uint8, Dc): the packed form of dense2sparse's output. Dc is the bit-row width
    the lists need (largest index + 1)."""
    counts = np.asarray([len(a) for a in vxl_ijk_list], dtype=np.int64)
    offsets = np.zeros((counts.size + 1,), dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    ijk = (np.concatenate([np.asarray(a).reshape(-1, 3) for a in vxl_ijk_list], axis=0) if counts.size else np.zeros((0, 3))).astype(np.uint8)
    Dc = int(ijk.max()) + 1 if ijk.size else 1
    return offsets, ijk, Dc


def split_lists(flat, offsets):
    """(T,...) array + offsets -> one array per cube."""
    return [flat[offsets[i]:offsets[i + 1]] for i in range(offsets.size - 1)]


def denoise_crossCubes(cube_ijk_np, vxl_ijk_list, vxl_mask_list, D_cube):
    """cube_ijk_np (N,3), vxl_ijk_list[i] (iN,3) uint8, vxl_mask_list[i] (iN,) bool -> [(iN,) bool, ...]."""
    offsets, ijk, Dc = pack_lists(vxl_ijk_list)
    mask = np.concatenate([np.asarray(m, dtype=bool).reshape(-1) for m in vxl_mask_list]) if len(vxl_mask_list) else np.zeros((0,), bool)
    if mask.size != ijk.shape[0]:
        raise ValueError("vxl_mask_list and vxl_ijk_list differ in length")
    out = runtime.any_context().denoise(offsets, ijk, cube_ijk_np, mask, D_cube, Dc)
    return [a.copy() for a in split_lists(out, offsets)]
