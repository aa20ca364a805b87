"""The contract of the winding-number stage (surfacenet_amd/csrc/meshwinding.h), restated with Python integers for
tests/test_meshwinding_cpu.py and tests/test_gpu_meshwinding.py, and the named cases both share.

    1 axes      the ray runs along +w, w = axis; the kept axes are (u, v) = (w + 1, w + 2) mod 3.
    2 triangle  n = (b - a) x (c - a), A2 = n_w, s = sign(A2), D = n . (p - a); q = rint(v * 65536) for vertices and queries alike.
    3 surface   a triangle with n != 0 holds p iff D = 0 and, along the triangle's own drop axis, the orient2 signs of p against ab, bc, ca
                hold no positive beside a negative.
    4 crossing  a triangle with s != 0 is crossed iff every edge x -> y has e = s ((y_u - x_u)(p_v - x_v) - (y_v - x_v)(p_u - x_u)) > 0, or
                e = 0 and the edge owns its line (s dy > 0, or s dy = 0 and s dx > 0), and D s < 0.
    5 outputs   winding = the sum of s over the crossed triangles, crossings their number, on_surface; counts.

Brute force over the triangles, every triangle against the queries inside the closed box of its (u, v) projection - a query outside it is
neither on the triangle nor under it. The integers are Python's (numpy object arrays) wherever a product could leave int64: a mesh and queries
within 16 cells of each other keep every value below 6 * 2^60 and are done in int64, the same values. `plant` is one of PLANTS, a deliberate
error for tests/test_meshwinding_cpu.py."""
import functools
import itertools

import numpy as np

import meshnormals_ref as mn

FIX = 65536
LO, HI = -4.0, 2097144.0
LEVELS, BUDGET, CELL_OFFSET = 22, 8, 4
MAX_TRIANGLES = 1 << 26
KEYS = ("winding", "crossings", "on_surface", "counts")
COUNTS = ("n_triangles", "n_parallel", "n_degenerate", "n_inside", "n_tests", "n_on_surface", "reserved6", "reserved7")
PLANTS = ("closed", "above_closed", "no_parallel", "int64", "axis_z", "non_cyclic", "parity")
POINT_TEXT = "point %d: a coordinate is outside [-4, 2^21 - 8) lattice cells"      # (the library adds "(or not a number)")
AXIS_TEXT = "axis = %d: 0 (x), 1 (y) or 2 (z)"


def _wrap64(x):
    return ((x + (1 << 63)) & ((1 << 64) - 1)) - (1 << 63)


def _sgn(x):
    """The signs of an int64 or object array, int64."""
    return np.asarray(x > 0, bool).astype(np.int64) - np.asarray(x < 0, bool).astype(np.int64)


def triangles(faces):
    """faces (F,nv) -> tri (T,3) int64: a quad (a,b,c,d) is (a,b,c) then (a,c,d), in face order."""
    f = np.asarray(faces, np.int64)
    if f.shape[1] == 3:
        return f.copy()
    return np.stack([f[:, [0, 1, 2]], f[:, [0, 2, 3]]], axis=1).reshape(-1, 3)


def quantise_points(pts):
    """The check of rule 7 on the queries, then q (n,3) int64."""
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        ok = ((p >= LO) & (p < HI)).all(axis=1)                 # (NaN fails)
    if not ok.all():
        raise ValueError(POINT_TEXT % int(np.argmin(ok)))
    return np.rint(p * float(FIX)).astype(np.int64)            # ties to even, exact


def axes(w):
    return (w + 1) % 3, (w + 2) % 3


def _drop_axis(n):
    m, axis = abs(n[0]), 0
    if abs(n[1]) > m:
        m, axis = abs(n[1]), 1
    if abs(n[2]) > m:
        axis = 2
    return axis


def _normal(a, b, c, W):
    u, v = [b[k] - a[k] for k in range(3)], [c[k] - a[k] for k in range(3)]
    return (W(W(u[1] * v[2]) - W(u[2] * v[1])), W(W(u[2] * v[0]) - W(u[0] * v[2])), W(W(u[0] * v[1]) - W(u[1] * v[0])))


def winding(verts, faces, pts, axis=2, plant=None):
    """verts (V,3) float64 in lattice cells, faces (F,3) or (F,4) integers, pts (n,3) float64 in lattice cells, axis 0..2 -> dict: winding
    (n,) int32, crossings (n,) int32, on_surface (n,) uint8, counts (8,) int64 (counts[4]: the tests of THIS broad phase, not held).
    ValueError in the library's words: the settings, then the first offending face, then the first offending query."""
    assert plant is None or plant in PLANTS
    if axis not in (0, 1, 2):
        raise ValueError(AXIS_TEXT % axis)
    f = np.asarray(faces)
    if f.ndim == 2 and f.shape[0] * (f.shape[1] - 2) > MAX_TRIANGLES:
        raise ValueError("%d triangles: at most 2^26" % (f.shape[0] * (f.shape[1] - 2)))
    q, f, referenced = mn.quantise(verts, faces)
    p = quantise_points(pts)
    n_pts = p.shape[0]
    tri = triangles(f)
    w = 2 if plant == "axis_z" else axis
    u, v = axes(w)
    wind, cross, on = np.zeros((n_pts,), np.int64), np.zeros((n_pts,), np.int64), np.zeros((n_pts,), bool)
    classes, tests = [0, 0, 0], 0
    span = 0
    if referenced.any() and n_pts:
        used = np.asarray(q[referenced].tolist(), np.int64)
        span = int(max(used.max(), p.max()) - min(used.min(), p.min()))
    small = plant == "int64" or span <= 1 << 20                 # int64 holds every value (or the plant asks for its wrap)
    W = _wrap64 if plant == "int64" else (lambda x: x)
    pa = p if small else p.astype(object)
    with np.errstate(over="ignore"):
        for row in tri.tolist():
            a, b, c = (tuple(int(x) for x in q[i]) for i in row)
            n = _normal(a, b, c, W)
            if n == (0, 0, 0):
                classes[2] += 1
                continue
            s = (n[w] > 0) - (n[w] < 0)
            classes[0 if s else 1] += 1
            # the queries inside the closed box of the (u, v) projection
            lo_u, hi_u, lo_v, hi_v = min(a[u], b[u], c[u]), max(a[u], b[u], c[u]), min(a[v], b[v], c[v]), max(a[v], b[v], c[v])
            ids = np.flatnonzero((p[:, u] >= lo_u) & (p[:, u] <= hi_u) & (p[:, v] >= lo_v) & (p[:, v] <= hi_v))
            if ids.size == 0:
                continue
            tests += ids.size
            P = pa[ids]
            D = (n[0] * (P[:, 0] - a[0]) + n[1] * (P[:, 1] - a[1])) + n[2] * (P[:, 2] - a[2])
            sd = _sgn(D)
            # rule 3
            if s or plant != "no_parallel":
                drop = _drop_axis(n)
                i, j = (1 if drop == 0 else 0), (1 if drop == 2 else 2)
                pos, neg = np.zeros((ids.size,), bool), np.zeros((ids.size,), bool)
                for x, y in ((a, b), (b, c), (c, a)):
                    o = _sgn((y[i] - x[i]) * (P[:, j] - x[j]) - (y[j] - x[j]) * (P[:, i] - x[i]))
                    pos |= o > 0
                    neg |= o < 0
                on[ids[(sd == 0) & ~(pos & neg)]] = True
            # rule 4
            if not s:
                continue
            cu, cv, sa = u, v, s
            if plant == "non_cyclic":                           # the kept axes swapped: the projected area changes its sign
                cu, cv, sa = v, u, -s
            covered = np.ones((ids.size,), bool)
            for x, y in ((a, b), (b, c), (c, a)):
                dx, dy = sa * (y[cu] - x[cu]), sa * (y[cv] - x[cv])
                e = dx * (P[:, cv] - x[cv]) - dy * (P[:, cu] - x[cu])
                owns = dy > 0 or (dy == 0 and dx > 0)
                covered &= (e > 0) | ((e == 0) & (owns or plant == "closed"))
            above = sd * s <= 0 if plant == "above_closed" else sd * s < 0
            hit = ids[covered & above]
            wind[hit] += sa
            cross[hit] += 1
    if plant == "parity":
        wind = cross % 2
    counts = np.asarray(classes + [int((wind != 0).sum()), tests, int(on.sum()), 0, 0], np.int64)
    return dict(winding=wind.astype(np.int32), crossings=cross.astype(np.int32), on_surface=on.astype(np.uint8), counts=counts)


def same_bytes(got, want, keys=KEYS):
    """The keys whose bytes differ; counts[4], the broad phase's tests, is not held."""
    diff = []
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if k == "counts":
            g, w = g.copy(), w.copy()
            g[4] = w[4] = 0
        if g.dtype != w.dtype or g.shape != w.shape or g.tobytes() != w.tobytes():
            diff.append(k)
    return diff


def grid_level(verts, faces, axis=2, budget=BUDGET):
    """The broad phase's choice, restated (it is no part of the contract; the tests force other levels to show that): a triangle with n != 0
    has the box floor(q / 65536) + 4 of its (u, v) extremes; at level s it overlaps prod((hi >> s) - (lo >> s) + 1) grid cells; the level is
    the smallest whose total is at most budget * T (21 at the latest). -> (level, entries at that level)."""
    q, f, _ = mn.quantise(verts, faces)
    u, v = axes(axis)
    boxes = []
    for row in triangles(f).tolist():
        a, b, c = (tuple(int(x) for x in q[i]) for i in row)
        if _normal(a, b, c, lambda x: x) != (0, 0, 0):
            boxes.append([[min(a[d], b[d], c[d]) >> 16 for d in (u, v)], [max(a[d], b[d], c[d]) >> 16 for d in (u, v)]])
    b = np.asarray(boxes, np.int64).reshape(-1, 2, 2) + CELL_OFFSET
    for s in range(LEVELS):
        total = int(np.prod((b[:, 1] >> s) - (b[:, 0] >> s) + 1, axis=1).sum()) if len(boxes) else 0
        if total <= budget * len(boxes) or s == LEVELS - 1:
            return s, total


def signed_distance(verts, faces, pts, max_dist=60.0, axis=2, resol=1.0):
    """mesh.signed_distance as the two restatements composed: meshdistance_ref.distance on the positions as given, winding for the sign."""
    import meshdistance_ref as md
    d = md.distance(np.asarray(verts, np.float64), np.asarray(faces, np.int32), np.asarray(pts, np.float64), max_dist)
    w = winding(verts, faces, pts, axis)
    dist = np.minimum(np.sqrt(d["d2"]), max_dist) * resol
    dist = np.where(w["winding"] != 0, -dist, dist)
    dist[(w["on_surface"] != 0) | (d["d2"] == 0.0)] = 0.0
    return dict(dist=dist, face=d["face"], closest=d["closest"] * resol, winding=w["winding"], on_surface=w["on_surface"].astype(bool))


# ---- the solids ---------------------------------------------------------------------------------------------------------------------------------------
_CUBE_QUADS = ((0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5))      # outward: -z, +z, -y, +y, -x, +x


def cube(lo=0.0, hi=4.0, reverse=False, quads=False, skip=None):
    """The cube [lo, hi]^3, vertex 4 k + 2 j + i at (i, j, k), outward faces (reverse: inward), as 6 quads or 12 triangles; skip: a face of
    _CUBE_QUADS that is left out. -> (verts (8,3) float64, faces int32)."""
    lo, hi = np.broadcast_to(np.asarray(lo, np.float64), (3,)), np.broadcast_to(np.asarray(hi, np.float64), (3,))
    v = np.asarray([[(lo[0], hi[0])[i], (lo[1], hi[1])[j], (lo[2], hi[2])[k]] for k in (0, 1) for j in (0, 1) for i in (0, 1)], np.float64)
    q = np.asarray([row for n, row in enumerate(_CUBE_QUADS) if n != skip], np.int32)
    if reverse:
        q = q[:, ::-1]
    return v, np.ascontiguousarray(q if quads else triangles(q).astype(np.int32))


def octahedron(r=4.0, centre=(0.0, 0.0, 0.0)):
    """The octahedron |x| + |y| + |z| <= r about centre, 8 outward triangles."""
    v = np.asarray([[r, 0, 0], [-r, 0, 0], [0, r, 0], [0, -r, 0], [0, 0, r], [0, 0, -r]], np.float64) + np.asarray(centre, np.float64)
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    return v, np.asarray(f, np.int32)


def join(*meshes):
    verts, faces, base = [], [], 0
    for v, f in meshes:
        verts.append(np.asarray(v, np.float64))
        faces.append(np.asarray(f, np.int32) + base)
        base += len(v)
    return np.concatenate(verts), np.concatenate(faces)


OFFSET = np.asarray([0.5, 0.25, 0.125])
# The solids are stated about the origin - the cube 0 .. 4, the octahedron of radius 4, queries in [-5, 5]^3 - and a query's coordinates
# start at -4 (rule 7): a case places mesh and queries SHIFT whole cells up every axis, which by rule 8 changes nothing.
SHIFT = 8.0


def placed(mesh, pts, shift=SHIFT):
    """(verts, faces), queries in the solids' own frame -> (verts + shift, faces, pts + shift)."""
    v, f = mesh
    return np.asarray(v, np.float64) + shift, f, np.asarray(pts, np.float64) + shift


@functools.lru_cache(maxsize=None)
def lattice_queries(lo=-5, hi=5, step=1.0):
    """Every point of the lattice lo .. hi at `step` - (n,3) float64 -, read-only."""
    a = np.arange(lo, hi + step / 2, step, dtype=np.float64)
    g = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    g.setflags(write=False)
    return g


def solid_queries():
    """In the solids' own frame: the 1,331 lattice points of [-5, 5]^3 and the same points plus (0.5, 0.25, 0.125): rays through vertices, along edges and inside
    ray-parallel faces, then rays in general position."""
    g = lattice_queries()
    return np.concatenate([g, g + OFFSET])


def cube_where(pts, lo=0.0, hi=4.0):
    """-> (inside, on) of the closed cube, analytically."""
    p = np.asarray(pts, np.float64)
    inside = ((p > lo) & (p < hi)).all(axis=1)
    return inside, ((p >= lo) & (p <= hi)).all(axis=1) & ~inside


def octahedron_where(pts, r=4.0):
    d = np.abs(np.asarray(pts, np.float64)).sum(axis=1)
    return d < r, d == r


# ---- the named cases: name -> (verts, faces, pts); every axis is asked of each ------------------------------------------------------------------------
FAR_LO, FAR_HI = float((1 << 20) - 16), float((1 << 21) - 16)   # a cube of 2^20-cell sides just below the range's end 2^21 - 8


def far_queries():
    mid = (FAR_LO + FAR_HI) / 2
    return np.asarray([[mid, mid, mid], [FAR_LO, mid, mid], [FAR_HI, FAR_HI, FAR_HI], [FAR_LO - 1, mid, mid], [mid, mid, FAR_HI + 7.5],
                       [mid + 0.5, FAR_LO + 1.0 / 65536, FAR_HI - 1.0 / 65536], [3.0, 3.0, 3.0], [FAR_HI - 0.25, FAR_HI - 0.25, FAR_LO + 0.25],
                       [mid, mid, FAR_LO - 2.0], [FAR_LO + 1.0 / 65536, FAR_LO + 2.0 / 65536, FAR_LO + 3.0 / 65536]], np.float64)


def degenerate_case():
    """A cube about (10, 10, 10) with, beside it, a triangle of a repeated index, one of collinear corners, one of coincident corners and a
    sliver parallel to the z axis; vertex 18 is unreferenced and not a number."""
    v, f = cube(8.0, 12.0)
    extra = np.asarray([[14, 14, 14], [15, 14, 14], [16, 14, 14], [14, 16, 14], [14, 16, 14], [20, 9, 9], [20, 9, 12], [20, 9.0000153, 9], [1, 1, 1], [2, 3, 4],
                        [np.nan, 0, 0]], np.float64)
    v = np.concatenate([v, extra])
    f = np.concatenate([f, np.asarray([[8, 9, 8], [8, 9, 10], [8, 11, 12], [13, 14, 15], [16, 17, 16]], np.int32)])
    pts = np.concatenate([lattice_queries(7, 13), [[15.0, 14, 14], [14.5, 14, 13], [20.0, 9, 10], [20.0, 9, 8], [20.0, 9.0000153, 9]]])
    return v, f, pts


def big_and_small_case():
    """One triangle across the whole box, high above 400 small ones in a 20 x 20 sheet of cells, each with its own three vertices."""
    v = [[2.0, 2.0, 30.0], [60.0, 2.0, 30.0], [2.0, 60.0, 30.0]]
    f = [[0, 1, 2]]
    for i, j in itertools.product(range(20), repeat=2):
        x, y, z, b = 5.0 + i, 5.0 + j, 10.0 + ((i * 7 + j * 3) % 5) * 0.25, len(v)
        v += [[x + 0.125, y + 0.125, z], [x + 0.875, y + 0.125, z], [x + 0.125, y + 0.875, z + 0.5]]
        f.append([b, b + 1, b + 2] if (i + j) % 2 else [b, b + 2, b + 1])
    rng = np.random.RandomState(11)
    pts = np.concatenate([rng.uniform(4.0, 26.0, (600, 3)), np.rint(rng.uniform(4.0, 26.0, (300, 3)) * 8) / 8, [[5.125, 5.125, 10.0], [5.5, 5.5, 2.0]]])
    return np.asarray(v, np.float64), np.asarray(f, np.int32), pts


def shell(quads=True):
    """The R = 6 sphere shell from the mesher (its restatement), as quads or triangulated, with the lattice points of [12, 28]^3, the same
    plus OFFSET, and the shell's centre."""
    import meshdistance_ref as md
    v, q = md.shell()
    g = lattice_queries(12, 28)
    return v, (q if quads else triangles(q).astype(np.int32)), np.concatenate([g, g + OFFSET, [[20.0, 20.0, 20.0]]])


LATE_N, LATE_SPAN = 200, 1 << 11


@functools.lru_cache(maxsize=None)
def late_columns(axis=2):
    """LATE_N one-triangle columns whose grid cell at level 0 - (cu, cv, 0), the unit cell - has a late key (tests/hash_adversary.py: its walk
    starts in the last sixteen slots of every table of 2^5 .. 2^16 slots), in hash_adversary.arrange's order; the queries lie under, on and
    over every triangle. -> (verts, faces, pts, cells (LATE_N,2))."""
    import hash_adversary as ha
    a = np.arange(CELL_OFFSET, LATE_SPAN, dtype=np.int64)
    cu, cv = (x.reshape(-1) for x in np.meshgrid(a, a, indexing="ij"))
    keys = ha.lt_key(cu, cv, np.zeros_like(cu))
    late = ha.late_mask(keys)
    cu, cv, keys = cu[late], cv[late], keys[late]
    order = ha.arrange(keys, LATE_N)
    cells = np.stack([cu[order], cv[order]], axis=1)
    u, v = axes(axis)
    verts, pts = [], []
    for n, (x, y) in enumerate(cells.tolist()):
        z = 5.0 + n % 7
        for du, dv, dz in ((0.125, 0.125, 0.0), (0.875, 0.125, 0.0), (0.125, 0.875, 0.25)):
            row = [0.0, 0.0, 0.0]
            row[u], row[v], row[axis] = x - CELL_OFFSET + du, y - CELL_OFFSET + dv, z + dz
            verts.append(row)
        for du, dv, dz in ((0.25, 0.25, -1.0), (0.25, 0.25, 2.0), (0.125, 0.125, 0.0), (0.75, 0.75, -1.0), (0.5, 0.125, -0.5)):
            row = [0.0, 0.0, 0.0]
            row[u], row[v], row[axis] = x - CELL_OFFSET + du, y - CELL_OFFSET + dv, z + dz
            pts.append(row)
    f = np.arange(3 * LATE_N, dtype=np.int32).reshape(-1, 3)
    return np.asarray(verts, np.float64), f, np.asarray(pts, np.float64), cells


CASES = dict(
    cube=lambda: placed(cube(), solid_queries()),
    cube_quads=lambda: placed(cube(quads=True), solid_queries()),
    octahedron=lambda: placed(octahedron(), solid_queries()),
    nested_reversed=lambda: placed(join(cube(-4.0, 4.0), cube(-2.0, 2.0, reverse=True)), solid_queries()),
    nested_same=lambda: placed(join(cube(-4.0, 4.0), cube(-2.0, 2.0)), solid_queries()),
    overlapping=lambda: placed(join(cube(-3.0, 2.0), cube(-1.0, 4.0)), solid_queries()),
    reversed=lambda: placed(cube(reverse=True), solid_queries()),
    open_cube=lambda: placed(cube(skip=1), solid_queries()),
    shell_q=lambda: shell(True),
    shell_t=lambda: shell(False),
    degenerate=degenerate_case,
    big_and_small=big_and_small_case,
    far=lambda: cube(FAR_LO, FAR_HI) + (far_queries(),),
    many=lambda: placed(octahedron(), lattice_queries(-5, 5, 0.125)),
    late_columns=lambda: late_columns()[:3],
)


@functools.lru_cache(maxsize=None)
def reference(name, axis=2):
    """The restatement's result for a named case and axis, computed once. Do not modify."""
    v, f, pts = CASES[name]()
    r = winding(v, f, pts, axis)
    for a in r.values():
        a.setflags(write=False)
    return r
