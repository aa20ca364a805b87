"""CPU restatement of the output cloud's normals and de-duplication, independent of the device code: a dense bool grid over
the occupied cells' bounding box, an einsum for the window moments, np.linalg.eigh for the eigenvector, np.unique for the owners. Also the scenes
tests/test_normals_cpu.py and tests/test_gpu_normals.py share."""
import functools
import itertools

import numpy as np


def pack(vxl_ijk_list):
    counts = np.asarray([len(a) for a in vxl_ijk_list], dtype=np.int64)
    offsets = np.zeros((counts.size + 1,), np.int64)
    np.cumsum(counts, out=offsets[1:])
    ijk = np.concatenate([np.asarray(a, np.uint8).reshape(-1, 3) for a in vxl_ijk_list]) if counts.size else np.zeros((0, 3), np.uint8)
    return offsets, ijk


def cube_of(offsets):
    return np.repeat(np.arange(offsets.size - 1), np.diff(offsets))


def world_cells(offsets, ijk, cube_ijk, stride_vox):
    """g = int64(cube_ijk) * stride_vox + int64(vxl_ijk), (T,3)."""
    return np.asarray(cube_ijk, np.int64).reshape(-1, 3)[cube_of(offsets)] * int(stride_vox) + np.asarray(ijk, np.int64)


def window(radius):
    return np.asarray(list(itertools.product(range(-radius, radius + 1), repeat=3)), np.int64)      # (W,3), d = 0 included


def moments_ref(offsets, ijk, cube_ijk, mask, stride_vox, radius):
    """(T,10) int32: |N|, sum d, sum d d^T (xx xy xz yy yz zz) over the occupied cells of the (2r+1)^3 window; zeros for unmasked voxels."""
    mask = np.asarray(mask, bool)
    out = np.zeros((mask.size, 10), np.int32)
    if not mask.any():
        return out
    g = world_cells(offsets, ijk, cube_ijk, stride_vox)[mask]
    lo = g.min(0)
    p = g - lo + radius                                        # padded by the radius: lookups beside the occupied box miss
    grid = np.zeros(tuple(g.max(0) - lo + 1 + 2 * radius), bool)
    grid[p[:, 0], p[:, 1], p[:, 2]] = True
    # cells with a negative coordinate do not exist; they are unoccupied in the grid anyway (nothing maps there)
    D = window(radius)
    occ = np.stack([grid[p[:, 0] + d[0], p[:, 1] + d[1], p[:, 2] + d[2]] for d in D], axis=1).astype(np.int64)      # (M,W)
    q = np.einsum("mw,wa,wb->mab", occ, D, D)
    m = np.concatenate([occ.sum(1)[:, None], occ @ D, q[:, 0, 0:3], q[:, 1, 1:3], q[:, 2, 2:3]], axis=1)
    out[mask] = m.astype(np.int32)
    return out


def scatter_matrix(mom):
    """C = n*q - s*s^T as (T,3,3) int64 from (T,10) moments."""
    m = np.asarray(mom, np.int64)
    n, s = m[:, 0], m[:, 1:4]
    q = np.empty((m.shape[0], 3, 3), np.int64)
    q[:, 0, 0], q[:, 0, 1], q[:, 0, 2], q[:, 1, 1], q[:, 1, 2], q[:, 2, 2] = m[:, 4], m[:, 5], m[:, 6], m[:, 7], m[:, 8], m[:, 9]
    q[:, 1, 0], q[:, 2, 0], q[:, 2, 1] = q[:, 0, 1], q[:, 0, 2], q[:, 1, 2]
    return n[:, None, None] * q - s[:, :, None] * s[:, None, :]


def voxel_points(offsets, ijk, cube_xyz, cube_resol):
    """The float32 points sparseCubes.sparse_xyz writes, for every voxel."""
    c = cube_of(offsets)
    return np.asarray(ijk, np.uint8) * np.asarray(cube_resol, np.float32)[c][:, None] + np.asarray(cube_xyz, np.float32)[c]


def mean_camera(view_idx, cameraTs):
    view_idx = np.asarray(view_idx)
    cams = np.asarray(cameraTs, np.float64)
    s = np.zeros((view_idx.shape[0], 3), np.float64)
    for k in range(view_idx.shape[1]):                         # summed in index order
        s = s + cams[view_idx[:, k]]
    return s / float(view_idx.shape[1])


def normals_ref(offsets, ijk, cube_ijk, mask, stride_vox, cube_xyz, cube_resol, view_idx, cameraTs, radius=2, min_neighbours=6, mom=None):
    """-> dict(normals (T,3) float32, moments (T,10) int32, solved (T,) bool: n >= min_neighbours, comparable (T,) bool: solved and
    (l1 - l0) >= 1e-3 * l2, gap (T,) float64: (l1 - l0) / l2 where solved, cos (T,) float64: cos(n, cbar - x) where solved)."""
    mask = np.asarray(mask, bool)
    T = mask.size
    mom = moments_ref(offsets, ijk, cube_ijk, mask, stride_vox, radius) if mom is None else mom
    solved = mask & (mom[:, 0] >= min_neighbours)
    res = dict(normals=np.zeros((T, 3), np.float32), moments=mom, solved=solved, comparable=np.zeros(T, bool), gap=np.zeros(T), cos=np.zeros(T))
    if not solved.any():
        return res
    C = scatter_matrix(mom[solved]).astype(np.float64)
    lam, vec = np.linalg.eigh(C)
    v = vec[:, :, 0]
    x = voxel_points(offsets, ijk, cube_xyz, cube_resol)[solved].astype(np.float64)
    d = mean_camera(view_idx, cameraTs)[cube_of(offsets)[solved]] - x
    dot = (v[:, 0] * d[:, 0] + v[:, 1] * d[:, 1]) + v[:, 2] * d[:, 2]
    v = np.where((dot < 0)[:, None], -v, v)
    res["normals"][solved] = v.astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.where(lam[:, 2] > 0, (lam[:, 1] - lam[:, 0]) / lam[:, 2], 0.0)
    res["gap"][solved] = gap
    res["comparable"][solved] = (lam[:, 1] - lam[:, 0]) >= 1e-3 * lam[:, 2]
    res["cos"][solved] = dot / np.sqrt((d * d).sum(1))
    return res


def unique_ref(offsets, ijk, cube_ijk, mask, stride_vox):
    """keep[t] = mask[t] and t is the smallest packed index among the masked voxels of its world cell."""
    mask = np.asarray(mask, bool)
    keep = np.zeros(mask.size, bool)
    idx = np.nonzero(mask)[0]
    if idx.size:
        _, first = np.unique(world_cells(offsets, ijk, cube_ijk, stride_vox)[idx], axis=0, return_index=True)       # first occurrence: idx is ascending
        keep[idx[first]] = True
    return keep


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------------
def hand_scene(cube_ijk, ijk_lists, stride_vox=13, resol=0.4, n_views=4):
    """A scene from hand-written voxel lists: every voxel masked (callers edit the mask). Cameras: `n_views` about 600 mm above (+z)."""
    cube_ijk = np.asarray(cube_ijk, np.int64).reshape(-1, 3)
    n = cube_ijk.shape[0]
    offsets, ijk = pack(ijk_lists)
    xyz = (cube_ijk * stride_vox * resol).astype(np.float32) + np.float32(-20.0)
    return dict(offsets=offsets, ijk=ijk, cube_ijk=cube_ijk, mask=np.ones(ijk.shape[0], bool), stride_vox=stride_vox, cube_xyz=xyz,
                cube_resol=np.full(n, resol, np.float32), view_idx=np.tile(np.arange(n_views, dtype=np.int32), (n, 1)), cameraTs=cameras_above(n_views))


def cameras_above(n_views=4, height=600.0, sign=1.0):
    a = np.arange(n_views) * (2 * np.pi / n_views) + 0.3
    return np.stack([60.0 * np.cos(a), 60.0 * np.sin(a), np.full(n_views, sign * height)], axis=1).astype(np.float64)


def cameras_side(n_views=4, dist=600.0):
    a = np.arange(n_views) * (2 * np.pi / n_views) + 0.3
    return np.stack([np.full(n_views, dist), 60.0 * np.cos(a) + 7.3, 60.0 * np.sin(a) - 11.7], axis=1).astype(np.float64)


@functools.lru_cache(maxsize=None)
def surface_scene(lattice=(2, 2, 1), Dc=26, shift=(0, 0, 0), cams="above", views_per_cube=4):
    """synthetic.sparse_surface(thickness=2, amplitude=6.0, seed=0) with masks pred >= float16(0.5), as packed arrays plus the lists; per-cube view
    indices drawn from 6 cameras (4 of `cams` + 2 of the other set, so that cubes differ in what they average). Do not modify the result."""
    from surfacenet_amd import synthetic
    d = synthetic.sparse_surface(tuple(lattice), Dc, thickness=2, amplitude=6.0, seed=0)
    n = len(d["vxl_ijk_list"])
    mask_list = [p >= np.float16(0.5) for p in d["prediction_list"]]
    offsets, ijk = pack(d["vxl_ijk_list"])
    cube_ijk = d["cube_ijk_np"].astype(np.int64) + np.asarray(shift, np.int64)
    main, other = (cameras_above(4), cameras_side(2)) if cams == "above" else (cameras_side(4), cameras_above(2))
    # the lattice's centre under / beside the cameras
    st = Dc // 2
    centre = np.asarray([(m + 1) * st * 0.4 / 2 - 20.0 for m in lattice])
    cameraTs = np.concatenate([main, other]) + np.asarray([centre[0], centre[1], 0.0] if cams == "above" else [0.0, centre[1], centre[2]])
    rs = np.random.RandomState(7)
    view_idx = np.concatenate([rs.randint(0, 4, (n, views_per_cube - 1)), rs.randint(0, 6, (n, 1))], axis=1).astype(np.int32)
    param = d["param_np"].copy()
    param["ijk"] = cube_ijk
    return dict(offsets=offsets, ijk=ijk, cube_ijk=cube_ijk, mask=np.concatenate(mask_list), stride_vox=st, cube_xyz=param["xyz"].copy(),
                cube_resol=param["resol"].copy(), view_idx=view_idx, cameraTs=cameraTs, lists=d, mask_list=mask_list, param=param,
                viewPair=view_idx.reshape(n, -1, 2).astype(np.uint16))


def scene_args(s):
    """The positional arguments of normals_ref / Context.normals up to cameraTs."""
    return (s["offsets"], s["ijk"], s["cube_ijk"], s["mask"], s["stride_vox"], s["cube_xyz"], s["cube_resol"], s["view_idx"], s["cameraTs"])


@functools.lru_cache(maxsize=None)
def surface_reference(lattice=(2, 2, 1), Dc=26, shift=(0, 0, 0), cams="above", radius=2, min_neighbours=6):
    """normals_ref + unique_ref of surface_scene, computed once per configuration and shared (read-only) among the tests."""
    s = surface_scene(lattice, Dc, shift, cams)
    r = normals_ref(*scene_args(s), radius=radius, min_neighbours=min_neighbours)
    r["unique"] = unique_ref(s["offsets"], s["ijk"], s["cube_ijk"], s["mask"], s["stride_vox"])
    return r


def sheet_5x5(z=7):
    """One cube, a 5x5 axis-aligned sheet at z, voxels (10..14, 10..14, z) in ascending order."""
    return [np.asarray([(i, j, z) for i in range(10, 15) for j in range(10, 15)], np.uint8)]


def tilted_sheet_two_cubes(stride_vox=13, Dc=26):
    """The sheet x + z = 20 over world x in 4..34, y in 8..13, split between cubes (0,0,0) and (1,0,0): world x <= 17 goes to cube 0 only, the rest
    to cube 1 only (local x = world x - 13), so every window at the seam needs the other cube's voxels."""
    a, b = [], []
    for x in range(4, 35):
        z = 20 - x
        if not 0 <= z < Dc:
            continue
        for y in range(8, 14):
            (a if x <= 17 else b).append((x, y, z) if x <= 17 else (x - stride_vox, y, z))
    return np.asarray([[0, 0, 0], [1, 0, 0]]), [np.asarray(a, np.uint8), np.asarray(b, np.uint8)]
