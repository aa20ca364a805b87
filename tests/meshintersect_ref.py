"""CPU restatement of the mesh self-intersection stage (include/surfacenet_hip.h states the contract), independent of
the device code: Python integers for every determinant (no width to overflow), candidates from a brute-force numpy box-overlap prefilter over
all triangle pairs (fine to about 5,000 triangles). tests/test_gpu_meshintersect.py compares bytes - every output but counts[2], the broad
phase's own number -, tests/test_meshintersect_cpu.py checks the restatement itself, and the named cases live here.

The contract, restated:
  inputs   sn_mesh_smooth's: verts (V,3) float64 in lattice cells, faces (F,nv) integers, nv 3 or 4; the checks of section 4.18 in its words;
           q = int64(rint(v * 65536)) of the referenced vertices; cap_pairs >= 0.
  1  a triangle face is one triangle, a quad (a,b,c,d) is (a,b,c) then (a,c,d). A triangle is degenerate iff two of its indices are equal or
     (q_b - q_a) x (q_c - q_a) = 0: skipped, its face counted once in n_degenerate_faces.
  2  orient3(a,b,c,d) = sign(((b-a) x (c-a)) . (d-a)); the drop axis of a triangle is the axis of its normal's largest magnitude, the lowest
     among equals; orient2 is the sign of the 2x2 determinant in the two kept axes, in their order.
  3  closed segment pq against closed non-degenerate triangle abc: sp = orient3(a,b,c,p), sq = orient3(a,b,c,q); sp * sq > 0: no; both 0: in
     the projection, yes iff p or q is in the triangle (three orient2 signs without both a positive and a negative) or pq meets one of the
     three edges (four-sign test, collinear endpoints by the closed bounding box); otherwise yes iff orient3(p,q,a,b), orient3(p,q,b,c),
     orient3(p,q,c,a) do not hold both a positive and a negative.
  4  two non-degenerate triangles of different faces, k = shared vertex INDICES: k = 0 the six edge-against-triangle tests; k = 1 the edge
     opposite the shared index in one against the other triangle, either way round; k = 2 (shared edge u < v, apexes a, b) orient3(u,v,a,b) = 0
     and (v-u) x (a-u), (v-u) x (b-u) of one sign in the first one's drop axis; k = 3 they intersect.
  5  faces f < g are a pair iff some triangle of f and some triangle of g intersect; one quad's two triangles are never tested.
  6  face_hit (F) uint8, face_pairs (F) int32 saturating at 2^31 - 1, pairs the first min(P, cap_pairs) pairs in ascending (f, g) order,
     counts[8] = T, degenerate faces, candidates (not held), P, faces hit, pairs with a k = 0 hit, pairs with k >= 1 hits only, pairs written.
"""
import functools

import numpy as np

import meshnormals_ref as mn
import meshsmooth_ref as sm

KEYS = ("face_hit", "face_pairs", "pairs", "counts")
COUNTS = ("n_triangles", "n_degenerate_faces", "n_candidates", "n_pairs", "n_faces_hit", "n_disjoint_pairs", "n_adjacent_pairs", "n_written")
PLANTS = ("open", "no_coplanar", "k1_as_k0", "int64", "drop_z")
_KEPT = ((1, 2), (0, 2), (0, 1))                              # the axes a drop axis keeps, in their order


def _sign(x):
    return (x > 0) - (x < 0)


def _wrap64(x):
    return ((x + (1 << 63)) & ((1 << 64) - 1)) - (1 << 63)


class _Rules:
    """Rules 2 to 4 on tuples of Python ints. plant: one of PLANTS, a deliberate error (tests/test_meshintersect_cpu.py)."""

    def __init__(self, plant=None):
        assert plant is None or plant in PLANTS
        self.plant = plant
        self.w = _wrap64 if plant == "int64" else (lambda x: x)
        self.bits = 0                                           # the widest determinant met

    def normal(self, a, b, c):
        w = self.w
        u = (b[0] - a[0], b[1] - a[1], b[2] - a[2])
        v = (c[0] - a[0], c[1] - a[1], c[2] - a[2])
        return (w(w(u[1] * v[2]) - w(u[2] * v[1])), w(w(u[2] * v[0]) - w(u[0] * v[2])), w(w(u[0] * v[1]) - w(u[1] * v[0])))

    def orient3(self, a, b, c, d):
        w = self.w
        n = self.normal(a, b, c)
        det = w(w(w(n[0] * (d[0] - a[0])) + w(n[1] * (d[1] - a[1]))) + w(n[2] * (d[2] - a[2])))
        self.bits = max(self.bits, abs(det).bit_length())
        return _sign(det)

    def drop_axis(self, n):
        if self.plant == "drop_z":
            return 2
        m = [abs(x) for x in n]
        return 0 if m[0] >= m[1] and m[0] >= m[2] else (1 if m[1] >= m[2] else 2)

    def orient2(self, p, q, r, drop):
        i, j = _KEPT[drop]
        w = self.w
        return _sign(w(w((q[i] - p[i]) * (r[j] - p[j])) - w((q[j] - p[j]) * (r[i] - p[i]))))

    @staticmethod
    def mixed(*s):
        return max(s) > 0 and min(s) < 0

    def point_in_tri2(self, x, a, b, c, drop):
        s = (self.orient2(a, b, x, drop), self.orient2(b, c, x, drop), self.orient2(c, a, x, drop))
        if self.plant == "open":
            return 0 not in s and not self.mixed(*s)
        return not self.mixed(*s)

    @staticmethod
    def on_box2(p, q, x, drop):
        return all(min(p[k], q[k]) <= x[k] <= max(p[k], q[k]) for k in _KEPT[drop])

    def seg_seg2(self, p, q, r, s, drop):
        d1, d2, d3, d4 = self.orient2(p, q, r, drop), self.orient2(p, q, s, drop), self.orient2(r, s, p, drop), self.orient2(r, s, q, drop)
        if d1 * d2 < 0 and d3 * d4 < 0:
            return True
        if self.plant == "open":
            return False
        return ((d1 == 0 and self.on_box2(p, q, r, drop)) or (d2 == 0 and self.on_box2(p, q, s, drop)) or
                (d3 == 0 and self.on_box2(r, s, p, drop)) or (d4 == 0 and self.on_box2(r, s, q, drop)))

    def seg_tri(self, p, q, a, b, c):
        sp, sq = self.orient3(a, b, c, p), self.orient3(a, b, c, q)
        if sp * sq > 0:
            return False
        if sp == 0 and sq == 0:
            if self.plant == "no_coplanar":
                return False
            drop = self.drop_axis(self.normal(a, b, c))
            return (self.point_in_tri2(p, a, b, c, drop) or self.point_in_tri2(q, a, b, c, drop) or self.seg_seg2(p, q, a, b, drop) or
                    self.seg_seg2(p, q, b, c, drop) or self.seg_seg2(p, q, c, a, drop))
        s = (self.orient3(p, q, a, b), self.orient3(p, q, b, c), self.orient3(p, q, c, a))
        if self.plant == "open":
            return sp * sq < 0 and 0 not in s and not self.mixed(*s)
        return not self.mixed(*s)

    def tri_tri(self, ia, A, ib, B):
        """-> (hit, k): rule 4 of two non-degenerate triangles, ia / ib their indices, A / B their corners."""
        shared = [(i, j) for i in range(3) for j in range(3) if ia[i] == ib[j]]
        k = len(shared)
        if k == 0 or (k == 1 and self.plant == "k1_as_k0"):
            for e in range(3):
                n = (e + 1) % 3
                if self.seg_tri(A[e], A[n], *B) or self.seg_tri(B[e], B[n], *A):
                    return True, k
            return False, k
        if k == 1:
            va, vb = shared[0]
            return (self.seg_tri(A[(va + 1) % 3], A[(va + 2) % 3], *B) or self.seg_tri(B[(vb + 1) % 3], B[(vb + 2) % 3], *A)), k
        if k == 2:
            pa = ({0, 1, 2} - {i for i, _ in shared}).pop()
            pb = ({0, 1, 2} - {j for _, j in shared}).pop()
            u, v = sorted(((pa + 1) % 3, (pa + 2) % 3), key=lambda i: ia[i])
            if self.orient3(A[u], A[v], A[pa], B[pb]) != 0:
                return False, k
            na, nb = self.normal(A[u], A[v], A[pa]), self.normal(A[u], A[v], B[pb])
            drop = self.drop_axis(na)
            return _sign(na[drop]) * _sign(nb[drop]) > 0, k
        return True, k


def triangles(faces):
    """faces (F,nv) -> (tri (T',3) int64, tri_face (T',) int64): rule 1's triangles in face order, degenerate ones included."""
    f = np.asarray(faces, np.int64)
    if f.shape[1] == 3:
        return f.copy(), np.arange(f.shape[0])
    return np.stack([f[:, [0, 1, 2]], f[:, [0, 2, 3]]], axis=1).reshape(-1, 3), np.repeat(np.arange(f.shape[0]), 2)


def intersect(verts, faces, cap_pairs=None, plant=None):
    """verts (V,3) float64 in lattice cells, faces (F,3) or (F,4) integers, cap_pairs (None: every pair) -> dict: face_hit (F,) uint8,
    face_pairs (F,) int32, pairs (min(P, cap_pairs),2) int32, counts (8,) int64, and what the tests look at beside them: all_pairs (P,2),
    k_hits [hits of triangle pairs with k = 0, 1, 2, 3], tri_hits the hit triangle pairs as (triangle, triangle, k), bits the widest
    determinant met. ValueError names the first offending face."""
    q, f, _ = mn.quantise(verts, faces)
    if cap_pairs is not None and cap_pairs < 0:
        raise ValueError("cap_pairs = %d must be >= 0" % cap_pairs)
    F = f.shape[0]
    rules = _Rules(plant)
    tri, tri_face = triangles(f)
    P = [[tuple(int(x) for x in q[i]) for i in row] for row in tri.tolist()]
    live = np.zeros((tri.shape[0],), bool)
    for t, (row, p) in enumerate(zip(tri.tolist(), P)):
        live[t] = len(set(row)) == 3 and _Rules().normal(*p) != (0, 0, 0)
    degenerate = np.zeros((F,), bool)
    degenerate[tri_face[~live]] = True
    # the prefilter: closed boxes of the quantised corners, brute force over the pairs of live triangles of different faces
    ids = np.flatnonzero(live)
    corners = np.asarray([P[t] for t in ids], np.int64).reshape(-1, 3, 3)
    lo, hi = corners.min(axis=1), corners.max(axis=1)
    cand = []
    for s in range(0, ids.size, 256):
        over = ((lo[s:s + 256, None, :] <= hi[None, :, :]) & (lo[None, :, :] <= hi[s:s + 256, None, :])).all(axis=2)
        i, j = np.nonzero(over)
        i += s
        keep = (i < j) & (tri_face[ids[i]] != tri_face[ids[j]])
        cand.append(np.stack([ids[i[keep]], ids[j[keep]]], axis=1))
    cand = np.concatenate(cand) if cand else np.zeros((0, 2), np.int64)
    kind = {}                                                   # (f, g) -> True iff some hit of theirs has k = 0
    k_hits, tri_hits = [0, 0, 0, 0], []
    tl = tri.tolist()
    for ta, tb in cand.tolist():
        hit, k = rules.tri_tri(tl[ta], P[ta], tl[tb], P[tb])
        if hit:
            k_hits[k] += 1
            tri_hits.append((ta, tb, k))
            key = tuple(sorted((int(tri_face[ta]), int(tri_face[tb]))))
            kind[key] = kind.get(key, False) or k == 0
    all_pairs = np.asarray(sorted(kind), np.int32).reshape(-1, 2)
    n_pairs = all_pairs.shape[0]
    face_pairs = np.bincount(all_pairs.reshape(-1), minlength=F).astype(np.int64)
    written = n_pairs if cap_pairs is None else min(n_pairs, int(cap_pairs))
    disjoint = sum(1 for v in kind.values() if v)
    counts = np.asarray([int(live.sum()), int(degenerate.sum()), cand.shape[0], n_pairs, int((face_pairs > 0).sum()), disjoint, n_pairs - disjoint,
                         written], np.int64)
    return dict(face_hit=(face_pairs > 0).astype(np.uint8), face_pairs=np.minimum(face_pairs, 2 ** 31 - 1).astype(np.int32),
                pairs=np.ascontiguousarray(all_pairs[:written]), counts=counts, all_pairs=all_pairs, k_hits=k_hits, tri_hits=tri_hits,
                bits=rules.bits)


def grid_level(verts, faces, budget=8):
    """The broad phase's choice, restated (it is no part of the contract; the tests force other levels to show that): a live triangle's box
    in lattice cells is floor(q / 65536) of its corners' extremes; at level s it overlaps prod((hi >> s) - (lo >> s) + 1) grid cells; the
    level is the smallest whose total over the live triangles is at most budget * T (21 at the latest). -> (level, entries at that level)."""
    q, f, _ = mn.quantise(verts, faces)
    tri, _ = triangles(f)
    boxes = []
    for row in tri.tolist():
        p = [tuple(int(x) for x in q[i]) for i in row]
        if len(set(row)) == 3 and _Rules().normal(*p) != (0, 0, 0):
            boxes.append([[min(c[d] for c in p) >> 16 for d in range(3)], [max(c[d] for c in p) >> 16 for d in range(3)]])
    b = np.asarray(boxes, np.int64).reshape(-1, 2, 3) + 4
    for s in range(22):
        total = int(np.prod((b[:, 1] >> s) - (b[:, 0] >> s) + 1, axis=1).astype(object).sum()) if len(boxes) else 0
        if total <= budget * len(boxes) or s == 21:
            return s, total


def same_bytes(got, want):
    """The keys of KEYS whose bytes differ; counts[2], the broad phase's candidates, is not held."""
    diff = []
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if k == "counts":
            g, w = g.copy(), w.copy()
            g[2] = w[2] = 0
        if g.dtype != w.dtype or g.shape != w.shape or g.tobytes() != w.tobytes():
            diff.append(k)
    return diff


# ---- named cases: (verts, faces). Do not modify the results. -------------------------------------------------------------------------------------
def _grid(nx, ny, z=3.0, x0=8.0, y0=8.0, step=1.0):
    """A flat sheet of (nx + 1) x (ny + 1) vertices, each cell cut into two triangles: vertex (i, j) = i * (ny + 1) + j."""
    i, j = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    v = np.stack([x0 + step * i, y0 + step * j, np.full(i.shape, z)], axis=-1).reshape(-1, 3).astype(np.float64)
    a = (i * (ny + 1) + j)[:-1, :-1].reshape(-1)
    b, c, d = a + (ny + 1), a + (ny + 1) + 1, a + 1
    f = np.stack([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)], axis=1).reshape(-1, 3)
    return v, f.astype(np.int32)


def _join(*meshes):
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(np.asarray(v, np.float64))
        fs.append(np.asarray(f, np.int32) + base)
        base += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


@functools.lru_cache(maxsize=None)
def two_spheres_case(shift=5.0):
    v, f = sm.sphere_case(6, False)
    return _join((v, f), (v + np.asarray([shift, 0.0, 0.0]), f))


@functools.lru_cache(maxsize=None)
def fold_case():
    """A flat 4 x 4 sheet whose centre vertex is moved, in the plane, across the edge of its neighbours: coplanar hits among triangles that
    share one and two indices."""
    v, f = _grid(4, 4)
    v = v.copy()
    v[2 * 5 + 2] += [1.25, 0.25, 0.0]
    return v, f


@functools.lru_cache(maxsize=None)
def fold_x_case():
    """fold in the plane x = 3: its triangles' drop axis is x."""
    v, f = fold_case()
    return np.ascontiguousarray(v[:, [2, 0, 1]]), f


def _wall(z_vertex):
    low, up = _grid(4, 4, z=3.0), _grid(4, 4, z=3.5, x0=8.3, y0=8.2)
    v = up[0].copy()
    v[2 * 5 + 2, 2] = z_vertex
    return _join(low, (v, up[1]))


@functools.lru_cache(maxsize=None)
def wall_case():
    """Two parallel sheets half a cell apart, the upper's centre vertex pushed one cell down through the lower."""
    return _wall(2.5)


@functools.lru_cache(maxsize=None)
def wall_touch_case():
    """... with that vertex EXACTLY on the lower sheet: a touch, sp = 0."""
    return _wall(3.0)


@functools.lru_cache(maxsize=None)
def tjunction_case():
    """Triangle 0 has the edge 0-1; on its other side that edge is split at its midpoint 3, a vertex triangle 0 does not name."""
    v = np.asarray([(8, 8, 8), (12, 8, 8), (10, 12, 9), (10, 8, 8), (10, 4, 7)], np.float64)
    return v, np.asarray([[0, 1, 2], [0, 4, 3], [3, 4, 1]], np.int32)


@functools.lru_cache(maxsize=None)
def quad_saddle_case():
    """A non-planar quad and a thin triangle (a quad with a repeated corner) through its second triangle (a,c,d) only."""
    v = np.asarray([(8, 8, 8), (12, 8, 8), (12, 12, 10), (8, 12, 8), (9, 11, 7), (9.25, 11, 10), (8.75, 11.25, 10)], np.float64)
    return v, np.asarray([[0, 1, 2, 3], [4, 5, 6, 6]], np.int32)


@functools.lru_cache(maxsize=None)
def far_case():
    """The wall near the top of the range on every axis, and triangles that span the whole range: a pair that crosses, a pair that misses by
    2^-16 cell, a pair that touches. Their determinants need more than 100 bits."""
    v, f = wall_case()
    wall = (v + 2097122.0, f)
    top = 2097143.0
    eps = 1.0 / 65536
    big = np.asarray([(-4, -4, -4), (top, -4, -3), (-4, top, -3),                              # a huge, nearly flat triangle
                      (100, 100, -4), (100.5, 100, top), (100, 100.5, top),                     # crosses it
                      (top, top, -3 + eps), (top - 9, top, 5), (top, top - 9, 5),               # above its far corner region: misses the plane's triangle
                      (-4, -4, top), (top, -4, top), (-4, top, top - eps),                      # a huge lid ...
                      (1000, 1000, top), (1001, 1000, top - 7), (1000, 1001, top - 7)],         # ... touched from below at one vertex? (Python decides)
                     np.float64)
    return _join(wall, (big, np.arange(15).reshape(5, 3)))


@functools.lru_cache(maxsize=None)
def big_and_small_case():
    """4,000 small triangles in a sheet and one triangle that spans all of it, tilted through it: its box is most of the grid's entries at
    the small ones' natural level."""
    v, f = _grid(40, 50, z=5.0)
    big = np.asarray([(7.5, 7.5, -3.0), (49.5, 7.75, 13.0), (7.75, 59.5, 13.0)], np.float64)
    return _join((v, f), (big, [[0, 1, 2]]))


@functools.lru_cache(maxsize=None)
def scramble():
    """two_spheres_crossing with its faces permuted and some reversed -> (verts, faces, perm): face i of it is face perm[i] of the case."""
    v, f = two_spheres_case()
    rng = np.random.default_rng(23)
    perm = rng.permutation(f.shape[0])
    g = f[perm].copy()
    rev = rng.random(g.shape[0]) < 0.5
    g[rev] = g[rev][:, ::-1]
    return v, np.ascontiguousarray(g), perm


CLEAN = ("sphere6_q", "sphere6_t", "sheet_q", "fan300")
CASES = dict({name: sm.CASES[name] for name in CLEAN}, rules=sm.rules_case, two_spheres_crossing=two_spheres_case,
             coincident=lambda: two_spheres_case(0.0), fold=fold_case, fold_x=fold_x_case, wall=wall_case, wall_touch=wall_touch_case, tjunction=tjunction_case,
             quad_saddle=quad_saddle_case, far=far_case, big_and_small=big_and_small_case, scr=lambda: scramble()[:2])


@functools.lru_cache(maxsize=None)
def reference(name):
    """intersect of a named case with every pair, computed once and shared (read-only) among the tests."""
    return intersect(*CASES[name]())


def truncated(want, cap):
    """reference()'s result as a call with cap_pairs = cap returns it."""
    written = min(int(want["counts"][3]), cap)
    counts = want["counts"].copy()
    counts[7] = written
    return dict(want, pairs=np.ascontiguousarray(want["all_pairs"][:written]), counts=counts)
