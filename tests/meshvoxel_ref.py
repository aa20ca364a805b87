"""The contract of the mesh voxelisation stage (surfacenet_amd/csrc/meshvoxel.h), restated with Python integers for
tests/test_meshvoxel_cpu.py and tests/test_gpu_meshvoxel.py, and the named cases both share.

    cells    voxel (n; i,j,k) is the world cell g = cube_ijk[n] * stride_vox + (i,j,k); its centre is the lattice point g, p = g * 65536 in
             the stages' fixed point; its box is the closed [p - 32768, p + 32768]^3. Vertices are q = rint(v * 65536).
    solid    bit 0: winding(p) != 0 under section 4.25's rules along `axis` - through meshwinding_ref.winding on the centres.
    surface  bit 1: some triangle with n != 0 has a point in common with the closed box: the separating-axis test on 13 axes - the
             triangle's normal, the 3 box axes, the 9 products of a box axis and an edge - in exact integers; separated iff on some axis
             the triangle's interval lies STRICTLY beyond the box's.
    outputs  occ (N,D,D,D) uint8 the bits, Y (N,1,D,D,D) float32 = 1.0 iff occ & select, per_cube (N,2) int64, counts (8,) int64.

Both bits are computed once per distinct world cell and handed to every cube that holds it. `plant` is one of PLANTS, a deliberate error for
tests/test_meshvoxel_cpu.py. solid_by_columns is the kernel's own way to the solid bit - per (triangle, column) the number K of centres
strictly below the triangle, +s at 0 and -s at K, a prefix sum - restated beside the first: the two agree."""
import functools

import numpy as np

import meshnormals_ref as mn
import meshwinding_ref as wr

FIX, HALF = 65536, 32768
HI_CELL = 2097144
MAX_D, MAX_VOXELS = 64, 1 << 33
SOLID, SURFACE = 1, 2
KEYS = ("occ", "Y", "per_cube", "counts")
COUNTS = ("n_triangles", "n_parallel", "n_degenerate", "n_solid_voxels", "n_surface_voxels", "n_both_voxels", "n_pairs", "n_tests")
PLANTS = ("parity", "open", "k_off", "skip_axis", "floor_columns", "overlap", "axis_z")
NEGATIVE_TEXT = "cube %d: a negative ijk"
REACH_TEXT = "cube %d: its last cell reaches 2^21 - 8 lattice cells"


def first(mn_q):
    """The first voxel column (or layer) whose closed box reaches the coordinate mn_q: ceil(mn / 65536 - 1/2)."""
    return -((-(mn_q - HALF)) // FIX)


def last(mx_q):
    return (mx_q + HALF) // FIX


def check_args(cube_ijk, D, stride_vox, axis=2, modes=3, select=2):
    """The refusals of the settings and the cubes, in the library's words -> cube (N,3) int64."""
    for name, value, lo, hi, text in (("D", D, 1, MAX_D, "D = %d: 1 .. 64"), ("stride_vox", stride_vox, 1, None, "stride_vox = %d must be >= 1"),
                                      ("axis", axis, 0, 2, wr.AXIS_TEXT), ("modes", modes, 1, 3, "modes = %d: 1 (solid), 2 (surface) or 3 (both)"),
                                      ("select", select, 1, 3, "select = %d: 1 (solid), 2 (surface) or 3 (either)")):
        if value < lo or (hi is not None and value > hi):
            raise ValueError(text % value)
    cube = np.asarray(cube_ijk, np.int64).reshape(-1, 3)
    if cube.shape[0] * D ** 3 > MAX_VOXELS:
        raise ValueError("%d voxels: at most 2^33" % (cube.shape[0] * D ** 3))
    return cube


def check_cubes(cube, D, stride_vox):
    negative, reach = (cube < 0).any(axis=1), (cube * stride_vox + D - 1 >= HI_CELL).any(axis=1)
    bad = negative | reach
    if bad.any():
        n = int(np.argmax(bad))
        raise ValueError((NEGATIVE_TEXT if negative[n] else REACH_TEXT) % n)


def world_cells(cube_ijk, D, stride_vox):
    """-> (N,D,D,D,3) int64: the world cell of every voxel."""
    cube = np.asarray(cube_ijk, np.int64).reshape(-1, 3)
    a = np.arange(D, dtype=np.int64)
    local = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1)
    return cube[:, None, None, None, :] * stride_vox + local[None]


def sat(v, n, skip=None, open_sets=False):
    """v (m,3,3): corner j of the triangle minus the voxel's centre (int64 or object), n (3,) the triangle's normal, Python ints -> (m,) bool:
    the closed box [-HALF, HALF]^3 and the closed triangle have a point in common. skip: an axis 0..12 left out (a plant); open_sets: touching
    counts as separated (a plant)."""
    beyond = (lambda a, b: a >= b) if open_sets else (lambda a, b: a > b)
    m = v.shape[0]
    sep = np.zeros((m,), bool)
    if skip != 0:
        dist = (n[0] * v[:, 0, 0] + n[1] * v[:, 0, 1]) + n[2] * v[:, 0, 2]
        sep |= np.asarray(beyond(abs(dist), HALF * (abs(n[0]) + abs(n[1]) + abs(n[2]))), bool)
    for d in range(3):
        if skip == 1 + d:
            continue
        lo, hi = np.minimum(np.minimum(v[:, 0, d], v[:, 1, d]), v[:, 2, d]), np.maximum(np.maximum(v[:, 0, d], v[:, 1, d]), v[:, 2, d])
        sep |= np.asarray(beyond(lo, HALF), bool) | np.asarray(beyond(-hi, HALF), bool)
    for e in range(3):
        e1, o = (e + 1) % 3, (e + 2) % 3
        f = v[:, e1, :] - v[:, e, :]
        for d in range(3):
            if skip == 4 + 3 * e + d:
                continue
            d1, d2 = (d + 1) % 3, (d + 2) % 3
            pe = f[:, d1] * v[:, e, d2] - f[:, d2] * v[:, e, d1]
            po = f[:, d1] * v[:, o, d2] - f[:, d2] * v[:, o, d1]
            r = HALF * (abs(f[:, d1]) + abs(f[:, d2]))
            sep |= np.asarray(beyond(np.minimum(pe, po), r), bool) | np.asarray(beyond(-np.maximum(pe, po), r), bool)
    return ~sep


def _tris(verts, faces):
    """-> [(a, b, c, n)] of the triangles with n != 0 (tuples of Python ints), and the number of the others."""
    q, f, _ = mn.quantise(verts, faces)
    out, degenerate = [], 0
    for row in wr.triangles(f).tolist():
        a, b, c = (tuple(int(x) for x in q[i]) for i in row)
        n = wr._normal(a, b, c, lambda x: x)
        if n == (0, 0, 0):
            degenerate += 1
        else:
            out.append((a, b, c, n))
    return out, degenerate


def surface_cells(verts, faces, cells, plant=None, skip=None):
    """cells (M,3) int64 distinct world cells -> ((M,) bool the surface bit, box tests run): every triangle against the cells of its box of
    columns and layers."""
    M = cells.shape[0]
    surf, tests = np.zeros((M,), bool), 0
    tris, _ = _tris(verts, faces)
    if M == 0 or not tris:
        return surf, tests
    lo, hi = cells.min(axis=0), cells.max(axis=0)
    index = None
    if int(np.prod((hi - lo + 1).astype(object))) <= 1 << 25:   # the cells' bounding box is small: a dense index; else every cell is asked
        index = np.full(tuple((hi - lo + 1).tolist()), -1, np.int64)
        index[tuple((cells - lo).T)] = np.arange(M)
    for a, b, c, n in tris:
        rng, inside = [], np.ones((M,), bool)
        for d in range(3):
            mnq, mxq = min(a[d], b[d], c[d]), max(a[d], b[d], c[d])
            f0, l0 = (mnq // FIX, mxq // FIX) if plant == "floor_columns" else (first(mnq), last(mxq))
            rng.append(slice(max(f0 - int(lo[d]), 0), max(min(l0, int(hi[d])) - int(lo[d]) + 1, 0)))
            if index is None:
                inside &= (cells[:, d] >= f0) & (cells[:, d] <= l0)
        ids = np.flatnonzero(inside) if index is None else index[tuple(rng)].reshape(-1)
        ids = ids[ids >= 0]
        if ids.size == 0:
            continue
        tests += ids.size
        p = cells[ids] * FIX
        v = np.asarray([a, b, c], np.int64)[None, :, :] - p[:, None, :]      # (|q| < 2^38: exact)
        if int(np.abs(v).max()) >= 1 << 19:                     # beyond 8 cells (|n| < 2^41, |n . v| < 3 * 2^60) int64 may not hold n . v: Python integers
            v = v.astype(object)
        hit = sat(v, n, skip=skip, open_sets=plant == "open")
        surf[ids[hit]] = True
    return surf, tests


def solid_by_columns(verts, faces, cube_ijk, D, stride_vox, axis=2, plant=None):
    """The kernel's way to the solid bit, per cube: for every triangle with s != 0 and every column of the cube that rule 4 covers, K = the
    centres of the column strictly below the triangle, +s at 0 and -s at K; the prefix sum along the ray axis is the winding number.
    -> (N,D,D,D) bool."""
    cube = np.asarray(cube_ijk, np.int64).reshape(-1, 3)
    w = axis
    u, v = wr.axes(w)
    tris, _ = _tris(verts, faces)
    out = np.zeros((cube.shape[0], D, D, D), bool)
    for n_cube, c in enumerate((cube * stride_vox).tolist()):
        delta = np.zeros((D, D, D + 1), np.int64)                   # [column u][column v][k]
        for a, b, cc, n in tris:
            s = (n[w] > 0) - (n[w] < 0)
            if not s:
                continue
            for gu in range(max(first(min(a[u], b[u], cc[u])), c[u]), min(last(max(a[u], b[u], cc[u])), c[u] + D - 1) + 1):
                for gv in range(max(first(min(a[v], b[v], cc[v])), c[v]), min(last(max(a[v], b[v], cc[v])), c[v] + D - 1) + 1):
                    pu, pv = gu * FIX, gv * FIX
                    covered = True
                    for x, y in ((a, b), (b, cc), (cc, a)):
                        dx, dy = s * (y[u] - x[u]), s * (y[v] - x[v])
                        e = dx * (pv - x[v]) - dy * (pu - x[u])
                        covered = covered and (e > 0 or (e == 0 and (dy > 0 or (dy == 0 and dx > 0))))
                    if not covered:
                        continue
                    p = [0, 0, 0]
                    K = 0
                    for k in range(D):
                        p[u], p[v], p[w] = pu, pv, (c[w] + k) * FIX
                        K += (sum(n[d] * (p[d] - a[d]) for d in range(3)) * s) < 0
                    if plant == "k_off" and K:
                        K = min(K + 1, D)
                    if K:
                        delta[gu - c[u], gv - c[v], 0] += s
                        delta[gu - c[u], gv - c[v], K] -= s
        wind = np.cumsum(delta[:, :, :D], axis=2) != 0            # [u][v][w]
        out[n_cube] = np.moveaxis(wind, (0, 1, 2), (u, v, w))
    return out


def voxelize(verts, faces, cube_ijk, D, stride_vox, axis=2, modes=3, select=2, plant=None, skip=None):
    """verts (V,3) float64 in lattice cells, faces (F,3) or (F,4) integers, cube_ijk (N,3), D 1..64, stride_vox >= 1 -> dict: occ (N,D,D,D)
    uint8, Y (N,1,D,D,D) float32, per_cube (N,2) int64, counts (8,) int64 (counts[6], counts[7]: THIS broad phase's, not held). ValueError
    in the library's words: the settings, then the first offending face, then the first offending cube."""
    assert plant is None or plant in PLANTS
    cube = check_args(cube_ijk, D, stride_vox, axis, modes, select)
    f = np.asarray(faces)
    if f.ndim == 2 and f.shape[0] * (f.shape[1] - 2) > wr.MAX_TRIANGLES:
        raise ValueError("%d triangles: at most 2^26" % (f.shape[0] * (f.shape[1] - 2)))
    mn.quantise(verts, faces)
    check_cubes(cube, D, stride_vox)
    N = cube.shape[0]
    world = world_cells(cube, D, stride_vox).reshape(-1, 3)
    cells, inverse = np.unique(world, axis=0, return_inverse=True) if world.size else (np.zeros((0, 3), np.int64), np.zeros((0,), np.int64))
    inverse = np.asarray(inverse).reshape(-1)
    w = wr.winding(verts, faces, cells.astype(np.float64), axis, plant=plant if plant in ("parity", "axis_z") else None)
    bits = np.zeros((cells.shape[0],), np.uint8)
    pairs = tests = 0
    if modes & SOLID:
        bits |= (w["winding"] != 0).astype(np.uint8) * SOLID
        pairs = int(w["counts"][4])
    if modes & SURFACE:
        surf, tests = surface_cells(verts, faces, cells, plant, skip if plant == "skip_axis" else None)
        bits |= surf.astype(np.uint8) * SURFACE
    occ = bits[inverse].reshape(N, D, D, D)
    if plant == "overlap" and N > 1:                            # every cube but the first forgets the surface bit of its first layer
        occ = occ.copy()
        occ[1:, 0] &= ~np.uint8(SURFACE)
    Y = ((occ & select) != 0).astype(np.float32).reshape(N, 1, D, D, D)
    per_cube = np.stack([((occ & SOLID) != 0).reshape(N, D ** 3).sum(axis=1), ((occ & SURFACE) != 0).reshape(N, D ** 3).sum(axis=1)], axis=1).astype(np.int64)
    counts = np.asarray(w["counts"][:3].tolist() + [int(per_cube[:, 0].sum()), int(per_cube[:, 1].sum()), int((occ == 3).sum()), pairs, tests], np.int64)
    return dict(occ=np.ascontiguousarray(occ), Y=Y, per_cube=per_cube.reshape(N, 2), counts=counts)


def same_bytes(got, want, keys=KEYS):
    """The keys whose bytes differ; counts[6] and counts[7], the broad phase's cost, are not held."""
    diff = []
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if k == "counts":
            g, w = g.copy(), w.copy()
            g[6:] = w[6:] = 0
        if g.dtype != w.dtype or g.shape != w.shape or g.tobytes() != w.tobytes():
            diff.append(k)
    return diff


def grid_level(verts, faces, axis=2, budget=wr.BUDGET):
    """The broad phase's choice, restated (no part of the contract; the tests force other levels to show that): meshwinding_ref.grid_level
    with the box of the voxel columns, first(min) .. last(max) on the kept axes. -> (level, entries at that level)."""
    u, v = wr.axes(axis)
    tris, _ = _tris(verts, faces)
    b = np.asarray([[[first(min(a[d], b_[d], c[d])) for d in (u, v)], [last(max(a[d], b_[d], c[d])) for d in (u, v)]] for a, b_, c, _ in tris],
                   np.int64).reshape(-1, 2, 2) + wr.CELL_OFFSET
    for s in range(wr.LEVELS):
        total = int(np.prod((b[:, 1] >> s) - (b[:, 0] >> s) + 1, axis=1).sum()) if len(tris) else 0
        if total <= budget * len(tris) or s == wr.LEVELS - 1:
            return s, total


def late_columns_case(axis=2):
    """meshwinding_ref.late_columns' one-triangle columns, whose unit cells have late keys at level 0, each in a cube of D = 8 at stride 1
    around it."""
    v, f, _, cells = wr.late_columns(axis)
    u, w = wr.axes(axis)
    cube = np.zeros((cells.shape[0], 3), np.int64)
    cube[:, u], cube[:, w], cube[:, axis] = cells[:, 0] - wr.CELL_OFFSET - 3, cells[:, 1] - wr.CELL_OFFSET - 3, 3
    return v, f, np.ascontiguousarray(np.maximum(cube, 0).astype(np.int32)), 8, 1


def distinct(occ, cube_ijk, stride_vox, bit):
    """The distinct world cells with `bit` set -> (m,3) int64, sorted."""
    occ = np.asarray(occ)
    world = world_cells(cube_ijk, occ.shape[1], stride_vox)
    return np.unique(world[(occ & bit) != 0].reshape(-1, 3), axis=0)


# ---- the named cases: name -> (verts, faces, cube_ijk, D, stride_vox); every axis is asked of each ------------------------------------------------
def cube_grid(lo, hi, stride):
    """cube_ijk of every cube lo .. hi (inclusive) per axis."""
    a = np.arange(lo, hi + 1, dtype=np.int32)
    return np.ascontiguousarray(np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3))


def sliver_case():
    """Small triangles between the lattice points: none holds a voxel centre, each touches the boxes of the voxels around it; one lies in a
    box face (x = 12.5), one has a corner on a box corner (11.5, 11.5, 11.5)."""
    v = np.asarray([[9.6, 9.7, 9.8], [9.9, 9.7, 9.8], [9.6, 9.9, 9.9],
                    [12.5, 10.0, 10.0], [12.5, 11.0, 10.0], [12.5, 10.0, 11.0],
                    [11.5, 11.5, 11.5], [11.75, 11.5, 11.5], [11.5, 11.75, 11.75],
                    [14.25, 8.0, 9.5], [14.75, 16.0, 9.5], [14.5, 12.0, 13.25]], np.float64)
    return v, np.arange(12, dtype=np.int32).reshape(-1, 3)


def _solid(mesh):
    v, f = mesh
    return np.asarray(v, np.float64) + wr.SHIFT, f


# the cubes of D = 8 at stride 4 around the solids placed 8 cells up: world cells 0 .. 19 per axis; the outer ones lie wholly above, below
# and beside the mesh
CASES = dict(
    cube=lambda: _solid(wr.cube()) + (cube_grid(0, 3, 4), 8, 4),
    cube_quads=lambda: _solid(wr.cube(quads=True)) + (cube_grid(0, 3, 4), 8, 4),
    octahedron=lambda: _solid(wr.octahedron()) + (cube_grid(0, 3, 4), 8, 4),
    nested_same=lambda: _solid(wr.join(wr.cube(-4.0, 4.0), wr.cube(-2.0, 2.0))) + (cube_grid(0, 3, 4), 8, 4),
    open_cube=lambda: _solid(wr.cube(skip=1)) + (cube_grid(0, 3, 4), 8, 4),
    octahedron_12=lambda: _solid(wr.octahedron()) + (cube_grid(0, 2, 5), 12, 5),
    sliver=lambda: sliver_case() + (cube_grid(1, 3, 4), 8, 4),
    sliver_12=lambda: sliver_case() + (cube_grid(0, 1, 7), 12, 7),
    degenerate=lambda: wr.degenerate_case()[:2] + (cube_grid(1, 3, 5), 8, 5),
    big_and_small=lambda: wr.big_and_small_case()[:2] + (np.asarray([[0, 0, 1], [1, 1, 1], [2, 1, 3], [5, 5, 2], [9, 9, 9]], np.int32), 12, 7),
    shell_q=lambda: wr.shell(True)[:2] + (np.asarray([[1, 1, 1], [2, 2, 2], [1, 2, 3]], np.int32), 12, 8),
    late_columns=late_columns_case,
)


@functools.lru_cache(maxsize=None)
def reference(name, axis=2):
    """The restatement's result for a named case and axis, computed once. Do not modify."""
    v, f, cube, D, stride = CASES[name]()
    r = voxelize(v, f, cube, D, stride, axis)
    for a in r.values():
        a.setflags(write=False)
    return r
