"""CPU restatement of the output cloud's connected components (include/surfacenet_hip.h, sn_components), independent of
the device code: the distinct world cells as sorted keys, neighbour look-ups with searchsorted, labels by hooking every edge's larger label
below the smaller one and pointer jumping until nothing changes. It is the definition the GPU is held to. Also the scenes and the comparison
helper that tests/test_components_cpu.py and tests/test_gpu_components.py share.

Contract: world cell g = cube_ijk * stride_vox + ijk; O = the distinct cells of the masked voxels; two distinct cells are adjacent iff
max |d| <= 1 and sum |d| <= 1, 2, 3 for connectivity 6, 18, 26; a component is a class of the transitive closure; first(K) = the smallest packed
index among the masked voxels whose cell lies in K; components are numbered by ascending first(K). label (T,) int32, -1 unmasked; cells (T,)
int32 = |K| in distinct cells, 0 unmasked; keep = mask and cells >= min_cells; C."""
import itertools

import numpy as np

from normals_ref import cube_of, pack, world_cells  # noqa: F401  (pack, cube_of: for the tests)

AXIS_BITS = 21


def offsets_before(connectivity):
    """The 3 / 9 / 13 neighbour offsets that precede (0, 0, 0) in (dx, dy, dz) order: every adjacent pair once."""
    max_sum = {6: 1, 18: 2, 26: 3}[connectivity]
    return [d for d in itertools.product((-1, 0, 1), repeat=3) if d < (0, 0, 0) and sum(abs(x) for x in d) <= max_sum]


def cell_keys(g):
    g = np.asarray(g, np.int64)
    return (g[:, 0] << (2 * AXIS_BITS)) | (g[:, 1] << AXIS_BITS) | g[:, 2]


def components_ref(offsets, ijk, cube_ijk, mask, stride_vox, connectivity=26, min_cells=1):
    """-> (label (T,) int32, cells (T,) int32, keep (T,) bool, C)."""
    mask = np.asarray(mask, bool).reshape(-1)
    T = mask.size
    label, cells = np.full((T,), -1, np.int32), np.zeros((T,), np.int32)
    idx = np.nonzero(mask)[0]
    if idx.size == 0:
        return label, cells, np.zeros((T,), bool), 0
    g = world_cells(offsets, ijk, cube_ijk, stride_vox)[idx]
    assert g.min() >= 0 and g.max() + 1 < (1 << AXIS_BITS)
    keys, first, inv = np.unique(cell_keys(g), return_index=True, return_inverse=True)      # first occurrence: idx is ascending
    inv = inv.reshape(-1)
    M = keys.size
    # cells renamed by the rank of their first packed index: the smallest name in a component is the cell of first(K)
    rank = np.empty((M,), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(M)
    gu = g[first]
    ea, eb = [], []
    for d in offsets_before(connectivity):
        q = gu + np.asarray(d, np.int64)
        ok = (q >= 0).all(1)                         # cells with a negative coordinate do not exist
        kq = cell_keys(q[ok])
        pos = np.minimum(np.searchsorted(keys, kq), M - 1)
        hit = keys[pos] == kq
        ea.append(rank[np.nonzero(ok)[0][hit]])
        eb.append(rank[pos[hit]])
    ea, eb = np.concatenate(ea), np.concatenate(eb)
    parent = np.arange(M)
    while True:
        pa, pb = parent[ea], parent[eb]
        if np.array_equal(pa, pb):
            break
        lo = np.minimum(pa, pb)
        np.minimum.at(parent, np.maximum(pa, pb), lo)
        np.minimum.at(parent, ea, lo)
        np.minimum.at(parent, eb, lo)
        while True:                                  # pointer jumping
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    roots = np.nonzero(parent == np.arange(M))[0]    # ascending: by first(K)
    number = np.full((M,), -1, np.int64)
    number[roots] = np.arange(roots.size)
    size = np.bincount(parent, minlength=M)          # distinct cells per root
    of_voxel = parent[rank[inv]]
    label[idx] = number[of_voxel]
    cells[idx] = size[of_voxel]
    return label, cells, mask & (cells >= min_cells), int(roots.size)


def sizes_of(label, cells, C):
    """(C,) int32: the size of every component, from a result."""
    sizes = np.zeros((C,), np.int32)
    m = label >= 0
    sizes[label[m]] = cells[m]
    return sizes


def compare(got, want):
    """Exact equality of (label, cells, keep, C), dtypes included: what the GPU tests assert."""
    names = ("label", "cells", "keep")
    assert int(got[3]) == int(want[3]), "C: %d, expected %d" % (got[3], want[3])
    for name, a, b, dt in zip(names, got[:3], want[:3], (np.int32, np.int32, np.bool_)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == dt and a.shape == b.shape, (name, a.dtype, a.shape, b.shape)
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, "%s differs at %d voxels, first %d: %r, expected %r" % (name, bad.size, bad[0], a[bad[0]], b[bad[0]])


def same_partition(a, b):
    """Two label arrays (any numbering, the same entries < 0) describe the same partition."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    if not np.array_equal(a < 0, b < 0):
        return False
    m = a >= 0
    pairs = np.unique(np.stack([a[m], b[m]], 1), axis=0)
    return np.unique(pairs[:, 0]).size == pairs.shape[0] and np.unique(pairs[:, 1]).size == pairs.shape[0]


# ---- scenes: dict(offsets, ijk, cube_ijk, mask, stride_vox) ---------------------------------------------------------------------------------------
def scene(cube_ijk, ijk_lists, stride_vox, mask=None):
    offsets, ijk = pack(ijk_lists)
    return dict(offsets=offsets, ijk=ijk, cube_ijk=np.asarray(cube_ijk, np.int64).reshape(-1, 3),
                mask=np.ones(ijk.shape[0], bool) if mask is None else np.asarray(mask, bool), stride_vox=stride_vox)


def scene_args(s):
    return s["offsets"], s["ijk"], s["cube_ijk"], s["mask"], s["stride_vox"]


def dense_to_list(vol):
    return np.stack(np.nonzero(vol), 1).astype(np.uint8)


def random_cube(D=8, fill=0.3, seed=3):
    """One cube, every cell occupied with probability `fill`, the voxels in a shuffled order."""
    rs = np.random.RandomState(seed)
    vol = rs.rand(D, D, D) < fill
    lst = dense_to_list(vol)
    return scene([[2, 1, 3]], [lst[rs.permutation(len(lst))]], 4), vol


def seam_scene(n_cubes=2, D=8, stride=4, seed=5, shuffle=True):
    """2 (along x) or 8 (2x2x2) overlapping cubes: a sheet z = 5 (world) crossing every seam, a second sheet two cells above it in the first
    cube only, and random blobs; every cube lists every occupied world cell inside it (cells in the overlaps up to eight times); the first
    voxels of every cube repeated at its end; a fifth of the entries unmasked (often on top of masked cells of another cube). Cubes shuffled."""
    rs = np.random.RandomState(seed)
    cubes = [(x, 0, 0) for x in range(2)] if n_cubes == 2 else list(itertools.product(range(2), repeat=3))
    ext = np.asarray(cubes).max(0) * stride + D
    world = rs.rand(*ext) < 0.06
    world[:, :, 5] = True
    world[:D, :D, 7] = rs.rand(D, D) < 0.5
    lists, masks = [], []
    for c in cubes:
        o = np.asarray(c) * stride
        lst = dense_to_list(world[o[0]:o[0] + D, o[1]:o[1] + D, o[2]:o[2] + D])
        lst = lst[rs.permutation(len(lst))]
        lst = np.concatenate([lst, lst[:5]])
        lists.append(lst)
        masks.append(rs.rand(len(lst)) >= 0.2)
    order = rs.permutation(len(cubes)) if shuffle else np.arange(len(cubes))
    return scene(np.asarray(cubes)[order] + 1, [lists[i] for i in order], stride, np.concatenate([masks[i] for i in order]))


def snake_scene(D=16, stride=16, layers=16, n_cubes=(2, 2, 1)):
    """A one-cell-wide path winding through the cubes, listed in REVERSE order along the path: a boustrophedon over every second row (x, y even)
    of every second layer (z even), the turns through the cells between. -> (scene, path length)."""
    X, Y = n_cubes[0] * D, n_cubes[1] * D
    path = []
    for zi, z in enumerate(range(0, layers, 2)):
        rows = list(range(0, Y, 2))
        if zi % 2:
            rows = rows[::-1]
        layer = []
        for yi, y in enumerate(rows):
            xs = list(range(X)) if yi % 2 == 0 else list(range(X - 1, -1, -1))
            if layer:                                            # the turn: one cell between the rows
                layer.append((layer[-1][0], (layer[-1][1] + y) // 2, z))
            layer.extend((x, y, z) for x in xs)
        if path:
            path.append((path[-1][0], path[-1][1], z - 1))
            if layer[0][:2] != path[-1][:2]:
                layer = layer[::-1]
            assert layer[0][:2] == path[-1][:2]
        path.extend(layer)
    path = np.asarray(path, np.int64)[::-1]
    cube = path // D
    cubes = sorted(set(map(tuple, cube)))
    lists = [(path[(cube == np.asarray(c)).all(1)] - np.asarray(c) * D).astype(np.uint8) for c in cubes]
    return scene(cubes, lists, stride), len(path)


def block_scene(D=24, gap=None):
    """Every cell of one D^3 cube, in (i, j, k) order; gap = x: the plane i == x left out."""
    vol = np.ones((D, D, D), bool)
    if gap is not None:
        vol[gap] = False
    return scene([[0, 0, 0]], [dense_to_list(vol)], D)


def checkerboard_scene(count, extra_unmasked=0, D=128):
    """The first `count` cells with i + j + k even of one D^3 cube, in (i, j, k) order: no two are 6-adjacent. Then `extra_unmasked` entries."""
    i, j, k = np.meshgrid(np.arange(D, dtype=np.uint8), np.arange(D, dtype=np.uint8), np.arange(D, dtype=np.uint8), indexing="ij")
    even = ((i.astype(np.int32) + j + k) & 1) == 0
    lst = np.stack([i[even], j[even], k[even]], 1)[:count]
    assert len(lst) == count
    lst = np.concatenate([lst, lst[:extra_unmasked]])
    return scene([[0, 0, 0]], [lst], D, np.arange(len(lst)) < count)
