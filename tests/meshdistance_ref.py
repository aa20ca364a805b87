"""CPU restatement of the point-to-mesh distance stage (include/surfacenet_hip.h states the contract), independent of
the device code: every point against every triangle, brute force, in elementwise numpy float64 - no np.dot, einsum or sum over the three
components, so every product and sum is rounded where the contract rounds it. tests/test_gpu_meshdistance.py compares bits - every output
but counts[4], the broad phase's own number -, tests/test_meshdistance_cpu.py checks the restatement itself against exact rationals, and the
named cases live here.

The contract, restated:
  inputs   verts (V,3) float64 in world coordinates, faces (F,nv) integers, nv 3 or 4 - a quad (a,b,c,d) is (a,b,c) then (a,c,d), triangle
           t = f for nv = 3 and 2 f + half for nv = 4 -, pts (n,3) float64 finite, max_dist finite and > 0.
           dot(a,b) = (a0*b0 + a1*b1) + a2*b2; cross(a,b) = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0).
  1  P against closed segment UV: e = V - U, w = P - U, ee = dot(e,e), we = dot(w,e); ee == 0 or we <= 0: c = U; else we >= ee: c = V itself;
     else t = we / ee, c = U + e*t. d2 = dot(P - c, P - c).
  2  P against ABC: e1 = B - A, e2 = C - A, n = cross(e1,e2), nn = dot(n,n); nn > 0: w = P - A, nb = dot(cross(w,e2), n), ng =
     dot(cross(e1,w), n), and nb > 0, ng > 0, nb + ng < nn give the face candidate c = A + (e1*(nb/nn) + e2*(ng/nn)). The first of face, AB,
     BC, CA with the least d2. nn == 0: degenerate, the three segments.
  3  the least d2 over all triangles, the smallest triangle index among those that attain it.
  4  reported when d2 < max_dist^2 (1 + 2^-40); else d2 = +inf, face = -1, closest = NaN. The same for F = 0.
  5  counts[8] = triangles, degenerate triangles, answered, beyond, tests (not held), 0, 0, 0.
"""
import functools
import itertools

import numpy as np

KEYS = ("d2", "face", "closest", "counts")
COUNTS = ("n_triangles", "n_degenerate", "n_answered", "n_beyond", "n_tests")
PLANTS = ("open", "no_inside", "u_plus_e", "tie_large", "half_quad")


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _xyz(a):
    """(..., 3) -> the three component arrays"""
    return (a[..., 0], a[..., 1], a[..., 2])


def segment(P, U, V, plant=None):
    """Rule 1 on tuples of component arrays (broadcast against each other) -> (d2, c)."""
    e, w = _sub(V, U), _sub(P, U)
    ee, we = _dot(e, e), _dot(w, e)
    at_u = (ee == 0.0) | ((we < 0.0) if plant == "open" else (we <= 0.0))
    at_v = ~at_u & (we >= ee)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = we / np.where(ee == 0.0, 1.0, ee)
    end = tuple(U[k] + e[k] * 1.0 for k in range(3)) if plant == "u_plus_e" else V
    c = tuple(np.where(at_u, U[k], np.where(at_v, end[k], U[k] + e[k] * t)) for k in range(3))
    return _dot(_sub(P, c), _sub(P, c)), c


def triangle(P, A, B, C, plant=None):
    """Rule 2 on tuples of component arrays -> (d2, c, degenerate)."""
    e1, e2 = _sub(B, A), _sub(C, A)
    n = _cross(e1, e2)
    nn = _dot(n, n)
    w = _sub(P, A)
    nb, ng = _dot(_cross(w, e2), n), _dot(_cross(e1, w), n)
    inside = (nn > 0.0) & (nb > 0.0) & (ng > 0.0) & (nb + ng < nn)
    if plant == "no_inside":
        inside = (nn > 0.0) & np.ones_like(inside)
    safe = np.where(nn > 0.0, nn, 1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        u, v = nb / safe, ng / safe
        c = tuple(A[k] + (e1[k] * u + e2[k] * v) for k in range(3))
        best = np.where(inside, _dot(_sub(P, c), _sub(P, c)), np.inf)
    for U, V in ((A, B), (B, C), (C, A)):
        d, s = segment(P, U, V, plant)
        take = d < best
        best = np.where(take, d, best)
        c = tuple(np.where(take, s[k], c[k]) for k in range(3))
    return best, c, ~(nn > 0.0)


def triangles(faces):
    """(F,3) or (F,4) -> (T,3): rule "a quad (a,b,c,d) is (a,b,c), (a,c,d)"."""
    f = np.asarray(faces)
    if f.shape[1] == 3:
        return f.reshape(-1, 3)
    return np.stack([f[:, [0, 1, 2]], f[:, [0, 2, 3]]], axis=1).reshape(-1, 3)


def limit(max_dist):
    return float(max_dist) * float(max_dist) * (1.0 + 2.0 ** -40)


def distance(verts, faces, pts, max_dist, plant=None, cells=2_000_000):
    """The contract on arrays -> dict of KEYS. plant: one of PLANTS, a deliberate error (tests/test_meshdistance_cpu.py)."""
    assert plant is None or plant in PLANTS
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces)
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    n, nv = p.shape[0], f.shape[1]
    tri = triangles(f)
    if plant == "half_quad" and nv == 4:
        tri = tri[0::2]
    T = tri.shape[0]
    d2 = np.full((n,), np.inf)
    best_t = np.zeros((n,), np.int64)
    closest = np.full((n, 3), np.nan)
    counts = np.zeros((8,), np.int64)
    counts[0] = T
    if T:
        A, B, C = (tuple(v[tri[:, k], a][None, :] for a in range(3)) for k in range(3))
        A1, B1, C1 = (tuple(x[0] for x in X) for X in (A, B, C))
        counts[1] = int(triangle(A1, A1, B1, C1)[2].sum())        # (nn depends on the triangle alone)
        step = max(1, cells // T)
        for i0 in range(0, n, step):
            q = p[i0:i0 + step]
            P = tuple(q[:, a][:, None] for a in range(3))
            d, _, _ = triangle(P, A, B, C, plant)
            if plant == "tie_large":
                t = T - 1 - np.argmin(d[:, ::-1], axis=1)
            else:
                t = np.argmin(d, axis=1)                         # (the first of the least: the smallest triangle index)
            # the chosen pairs once more, for their closest points: the same arithmetic, so the same bits
            dd, c, _ = triangle(_xyz(q), _xyz(v[tri[t, 0]]), _xyz(v[tri[t, 1]]), _xyz(v[tri[t, 2]]), plant)
            assert np.array_equal(dd, d[np.arange(q.shape[0]), t])
            d2[i0:i0 + step], best_t[i0:i0 + step] = dd, t
            closest[i0:i0 + step] = np.stack(c, axis=1)
        counts[4] = n * T
    ok = d2 < limit(max_dist)
    if plant == "half_quad" and nv == 4:
        face = best_t
    else:
        face = best_t >> (nv - 3)
    counts[2], counts[3] = int(ok.sum()), int(n - ok.sum())
    return dict(d2=np.where(ok, d2, np.inf), face=np.where(ok, face, -1).astype(np.int32), closest=np.where(ok[:, None], closest, np.nan), counts=counts)


def same_bits(got, want, keys=KEYS):
    """The keys whose arrays differ in dtype, shape or bits (counts: all but counts[4])."""
    bad = []
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if k == "counts":
            a, b = np.delete(a, 4), np.delete(b, 4)
        if a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
            bad.append(k)
    return bad


# ---- named cases ---------------------------------------------------------------------------------------------------------------------------------
TRI = np.asarray([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 3.0, 0.0]])
# the seven regions of the triangle's plane (inside, beyond each edge, beyond each corner), above the plane and in it; then the points the
# contract names: in the plane inside, a corner, on an edge
REGION_UV = dict(inside=(0.25, 0.25), edge_ab=(0.5, -0.5), edge_bc=(0.75, 0.75), edge_ca=(-0.5, 0.5), corner_a=(-0.5, -0.5), corner_b=(1.75, -0.5),
                 corner_c=(-0.5, 1.75))


def region_queries():
    """(names, (n,3) points) around TRI at unit scale."""
    names, pts = [], []
    for name, (u, v) in REGION_UV.items():
        base = TRI[0] + u * (TRI[1] - TRI[0]) + v * (TRI[2] - TRI[0])
        for tag, z in (("above", 1.5), ("plane", 0.0), ("below", -0.75)):
            names.append(name + "_" + tag)
            pts.append(base + [0.0, 0.0, z])
    names += ["at_corner_b", "on_edge_bc", "on_edge_ab"]
    pts += [TRI[1].copy(), 0.5 * (TRI[1] + TRI[2]), np.asarray([1.0, 0.0, 0.0])]
    return names, np.asarray(pts)


def single_triangle(scale=1.0, offset=0.0):
    """TRI and its region queries at a scale and an offset along (1,1,1): (verts, faces, pts, names)."""
    names, pts = region_queries()
    return TRI * scale + offset, np.asarray([[0, 1, 2]], np.int32), pts * scale + offset, names


SCALES, OFFSETS = (0.01, 1.0, 300.0), (0.0, 500.0)


def degenerate_mesh():
    """Degenerate triangles of all three kinds beside one good one: a repeated index, collinear corners, coincident corners (three indices, one
    position). Vertex 9 is unreferenced and not a number. -> (verts, faces, pts)"""
    v = np.asarray([[0.0, 0, 0], [2, 0, 0], [0, 2, 0],            # 0 1 2: the good triangle
                    [5, 0, 0], [7, 0, 0],                         # 3 4: a segment, as (3,4,4)
                    [0, 5, 0], [0, 6, 0], [0, 8, 0],              # 5 6 7: collinear
                    [9, 9, 9], [np.nan, 0, 0], [9, 9, 9], [9, 9, 9]], np.float64)      # 8 10 11: one point
    f = np.asarray([[0, 1, 2], [3, 4, 4], [5, 6, 7], [8, 10, 11]], np.int32)
    pts = np.asarray([[6.0, 1, 0], [4, 0, 1], [8, -1, 0], [1, 7, 0], [0, 9, 2], [-1, 4, 0], [9, 9, 10], [8, 8, 8], [0.5, 0.5, 3]])
    return v, f, pts


def neg_zero_corner():
    """A corner at -0.0 and a query whose foot on AB is exactly that corner (we == 0): the closest point is the corner itself, -0.0, not
    U + e*0 = +0.0. The triangle is a segment twice over, so no other candidate comes first."""
    v = np.asarray([[-0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    return v, np.asarray([[0, 1, 1]], np.int32), np.asarray([[0.0, 1.0, 0.0]])


def u_plus_e_case():
    """A query beyond V of a segment whose U + (V - U) is not V in float64, on the side where the wrong point is the nearer one (V is also
    the U of the next segment, which would otherwise win with the right point)."""
    v = np.asarray([[0.2, 0.3, 0.2], [0.9, 0.9, 0.9]])
    e = v[1] - v[0]
    assert ((v[0] + e * 1.0) != v[1]).any()
    return v, np.asarray([[0, 1, 1]], np.int32), np.asarray([[0.5, 1.5, 1.5]])


def tie_case():
    """Two triangles that share an edge, the query above the middle of that edge: both attain the minimum."""
    v = np.asarray([[0.0, 0, 0], [2, 0, 0], [1, 2, 0], [1, -2, 0]])
    return v, np.asarray([[0, 1, 2], [1, 0, 3]], np.int32), np.asarray([[1.0, 0.0, 1.0]])


def quad_case():
    """One quad, the query above the middle of its second triangle."""
    v = np.asarray([[0.0, 0, 0], [4, 0, 0], [4, 4, 0], [0, 4, 0]])
    return v, np.asarray([[0, 1, 2, 3]], np.int32), np.asarray([[1.0, 3.0, 0.5]])


def outside_case():
    """One triangle, the query beyond edge BC in the triangle's plane: its projection is nearer than any point of the triangle."""
    return TRI.copy(), np.asarray([[0, 1, 2]], np.int32), np.asarray([[4.0, 3.0, 0.0]])


@functools.lru_cache(maxsize=None)
def shell(R=6):
    """The quad mesh of the R shell (tests/mesh_ref.py sphere_scene through the mesher's restatement). Do not modify."""
    import meshsmooth_ref as sm
    v, q = sm.sphere_case(R, True)
    return np.ascontiguousarray(v, np.float64), np.ascontiguousarray(q, np.int32)


SHELL_MAX_DIST = 2.5


@functools.lru_cache(maxsize=None)
def shell_queries(R=6, beyond=0.05, seed=5):
    """About 1,000 queries of the shell: its own vertices, lattice points within 3 cells of it, and `beyond` of them farther than
    SHELL_MAX_DIST (lattice points 4 to 6 cells off the sphere). Do not modify."""
    v, _ = shell(R)
    g = np.asarray(list(itertools.product(range(8, 33), repeat=3)), np.float64)
    rad = np.sqrt(((g - 20.0) ** 2).sum(1))
    near, far = g[np.abs(rad - R) <= 3.0], g[(rad - R >= 4.0) & (rad - R <= 6.0)]
    rng = np.random.RandomState(seed)
    n_near = 1000 - v.shape[0] if v.shape[0] < 900 else 300
    n_far = int(round(beyond * (v.shape[0] + n_near) / (1.0 - beyond)))
    near = near[rng.choice(near.shape[0], n_near, replace=False)]
    far = far[rng.choice(far.shape[0], n_far, replace=False)]
    return np.ascontiguousarray(np.concatenate([v, near + 0.25, far]))


@functools.lru_cache(maxsize=None)
def big_and_small(n=300, seed=7):
    """One triangle that spans the whole box among n small ones. -> (verts, faces, pts). Do not modify."""
    rng = np.random.RandomState(seed)
    c = rng.uniform(2.0, 62.0, (n, 3))
    small = (c[:, None, :] + rng.uniform(-0.4, 0.4, (n, 3, 3))).reshape(-1, 3)
    v = np.concatenate([small, [[0.0, 0.0, 0.0], [64.0, 0.0, 64.0], [0.0, 64.0, 64.0]]])
    f = np.concatenate([np.arange(3 * n).reshape(n, 3), [[3 * n, 3 * n + 1, 3 * n + 2]]]).astype(np.int32)
    pts = np.concatenate([c + 0.3, rng.uniform(0.0, 64.0, (300, 3)), rng.uniform(-30.0, 94.0, (60, 3))])
    return v, f, np.ascontiguousarray(pts)


@functools.lru_cache(maxsize=None)
def fan(n=300):
    """n triangles through one point, crowding its cell. -> (verts, faces, pts). Do not modify."""
    t = 2 * np.pi * np.arange(n) / n
    rim = np.stack([16 + 10 * np.cos(t), 16 + 10 * np.sin(t), 14 + 3 * np.cos(7 * t)], axis=1)
    v = np.concatenate([[[16.0, 16.0, 16.0]], rim])
    i = np.arange(n)
    f = np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], axis=1).astype(np.int32)
    rng = np.random.RandomState(3)
    pts = np.concatenate([[[16.0, 16.0, 16.0], [16.0, 16.0, 18.0]], rng.uniform(4.0, 28.0, (200, 3)), v[1::7] + [0.0, 0.0, 0.5]])
    return v, f, np.ascontiguousarray(pts)


def far_queries(verts, cell=1.0, cells=40):
    """Queries `cells` cells outside the mesh's box on each of its six sides and at a corner."""
    lo, hi = verts.min(0), verts.max(0)
    mid = 0.5 * (lo + hi)
    pts = []
    for a in range(3):
        for side, edge in ((-1.0, lo), (1.0, hi)):
            q = mid.copy()
            q[a] = edge[a] + side * cells * cell
            pts.append(q)
    pts.append(hi + cells * cell)
    return np.asarray(pts)


def lattice_queries(lo, hi, n_axis):
    """n_axis^3 lattice points of the box lo .. hi."""
    ax = [np.linspace(lo[a], hi[a], n_axis) for a in range(3)]
    return np.ascontiguousarray(np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3))


def small_mesh():
    """An octahedron: the small mesh of the query-count case."""
    v = np.asarray([[1.0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]) * 3.0 + 10.0
    f = np.asarray([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


# ---- exact rationals -----------------------------------------------------------------------------------------------------------------------------
def exact_d2(P, A, B, C):
    """The squared distance from P to triangle ABC in exact rational arithmetic (fractions): the minimum over the face's foot, if it lies in the
    closed triangle, and the three closed segments."""
    from fractions import Fraction as Fr
    P, A, B, C = ([Fr(float(x)) for x in p] for p in (P, A, B, C))
    sub = lambda a, b: [a[k] - b[k] for k in range(3)]
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    def seg(U, V):
        e, w = sub(V, U), sub(P, U)
        ee, we = dot(e, e), dot(w, e)
        t = Fr(0) if ee == 0 else min(max(we / ee, Fr(0)), Fr(1))
        c = [U[k] + e[k] * t for k in range(3)]
        return dot(sub(P, c), sub(P, c))
    best = min(seg(A, B), seg(B, C), seg(C, A))
    e1, e2 = sub(B, A), sub(C, A)
    n = cross(e1, e2)
    nn = dot(n, n)
    if nn > 0:
        w = sub(P, A)
        nb, ng = dot(cross(w, e2), n), dot(cross(e1, w), n)
        if nb >= 0 and ng >= 0 and nb + ng <= nn:
            h = dot(w, n)
            best = min(best, h * h / nn)
    return best


def exact_error(P, A, B, C):
    """|d - d_exact| / the largest coordinate magnitude, d the restatement's distance."""
    import math
    from fractions import Fraction as Fr
    d2, _, _ = triangle(*(tuple(np.float64(x) for x in p) for p in (P, A, B, C)))
    ex = exact_d2(P, A, B, C)
    # sqrt of the exact rational to well beyond float64: integer square root of the scaled value
    scale = 1 << 200
    root = Fr(math.isqrt(int(ex * scale * scale)), scale)
    mag = max(abs(float(x)) for p in (P, A, B, C) for x in p)
    return float(abs(Fr(float(np.sqrt(d2))) - root)) / mag


def dyadic_triangles(n, scale, offset, seed):
    """n random triangles and queries whose coordinates are multiples of scale / 1024 near offset, every eighth one degenerate."""
    rng = np.random.RandomState(seed)
    q = rng.randint(-1024, 1025, (n, 4, 3)).astype(np.float64)
    q[0::8, 2] = q[0::8, 1]                                     # B = A: a repeated corner
    q[4::16, 3] = 2 * q[4::16, 2] - q[4::16, 1]                 # C = 2 B - A: collinear
    return q * (scale / 1024.0) + offset


# ---- the cases the GPU is held to, by name -----------------------------------------------------------------------------------------------------------
def _shell_case(shift=0.0):
    v, q = shell()
    return v + shift, q, shell_queries() + shift, SHELL_MAX_DIST


def _far_case(max_dist):
    v, q = shell()
    return v, q, far_queries(v), max_dist


MANY_AXIS = 81                                                  # 81^3 = 531,441 queries: more than the 2048 x 256 lanes of one grid-stride trip


def _many_case():
    v, f = small_mesh()
    return v, f, lattice_queries((2.0, 2.0, 2.0), (18.0, 18.0, 18.0), MANY_AXIS), 4.0


def _plain(case, max_dist=100.0):
    return lambda: case() + (max_dist,)


CASES = {"single_%g_%g" % (s, o): (lambda s=s, o=o: single_triangle(s, o)[:3] + (1e4 * s,)) for s in SCALES for o in OFFSETS}
CASES.update(degenerate=_plain(degenerate_mesh), neg_zero_corner=_plain(neg_zero_corner), u_plus_e=_plain(u_plus_e_case), tie=_plain(tie_case),
             quad=_plain(quad_case), outside=_plain(outside_case), shell=_shell_case, shell_500=lambda: _shell_case(500.0),
             big_and_small=_plain(big_and_small, 20.0), fan=_plain(fan, 6.0), far_hit=lambda: _far_case(80.0), far_miss=lambda: _far_case(30.0),
             many=_many_case)


LATE_LEVEL, LATE_N = 2, 200


@functools.lru_cache(maxsize=None)
def late_cells_case():
    """Colliding keys: 200 small triangles, one in each of tests/hash_adversary.py's late cells of [0, 128)^3 - the cells whose lt_key starts
    its probe walk in the last sixteen slots of every table of 2^5 .. 2^16 slots - in arrange()'s order, and two anchors that pin the box
    to [0, 127.75]: the top cell is 128, a finest cell 0.25, and at the FORCED level 2 a grid cell is the unit cell floor(x). The table
    of 2 * 8 * 202 -> 4,096 slots sees every key arrive at its end and wrap around. Queries: beside every triangle and between them."""
    import hash_adversary as ha
    cells = np.asarray(ha.arranged_cells(LATE_N), np.float64)
    corner = np.asarray([[0.25, 0.25, 0.25], [0.5, 0.25, 0.25], [0.25, 0.5, 0.25]])
    anchors = np.asarray([[[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.5, 0.0]], [[127.75, 127.75, 127.75], [127.25, 127.75, 127.75], [127.75, 127.25, 127.75]]])
    v = np.concatenate([(cells[:, None, :] + corner[None]).reshape(-1, 3), anchors.reshape(-1, 3)])
    f = np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3)
    rng = np.random.RandomState(9)
    pts = np.concatenate([cells + 0.4 + rng.uniform(-0.3, 0.3, cells.shape), cells + [1.5, -0.5, 0.75], rng.uniform(0.0, 128.0, (200, 3))])
    v.setflags(write=False)
    return v, f, np.ascontiguousarray(pts), 12.0


CASES["late_cells"] = late_cells_case


@functools.lru_cache(maxsize=None)
def reference(name):
    """distance() of a named case, computed once and shared among the tests. Do not modify."""
    v, f, pts, max_dist = CASES[name]()
    return distance(v, f, pts, max_dist)


LEVELS, BUDGET = 10, 8


def grid_level(verts, faces, max_dist, budget=BUDGET):
    """The broad phase's level and its entries, restated (csrc/meshdistance_rules.h): the top cell is the power of two above the larger of
    the box's largest extent and max_dist * 2^-20, a finest cell top / 2^9, the level the finest whose entries are at most budget per
    triangle. -> (level, entries, cell size of the level)"""
    import math
    v = np.asarray(verts, np.float64)
    tri = triangles(faces)
    c = v[tri]                                                  # (T,3,3)
    used = v[np.unique(tri)]
    o, extent = used.min(axis=0), float((used.max(axis=0) - used.min(axis=0)).max())
    top = 2.0 ** math.frexp(max(extent, max_dist * 2.0 ** -20))[1]       # (frexp gives m in [0.5, 1): 2^e is above an exact power of two too)
    inv = 2.0 ** (LEVELS - 1) / top
    cell = lambda x: np.clip(np.floor((x - o) * inv), 0, 2 ** (LEVELS - 1) - 1).astype(np.int64)
    lo, hi = cell(c.min(axis=1)), cell(c.max(axis=1))
    for s in range(LEVELS):
        total = int(np.prod((hi >> s) - (lo >> s) + 1, axis=1).sum())
        if total <= budget * tri.shape[0] or s == LEVELS - 1:
            return s, total, top / 2.0 ** (LEVELS - 1 - s)
