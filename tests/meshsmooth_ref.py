"""CPU restatement of the mesh smoother (Taubin lambda|mu smoothing with the uniform umbrella operator, in fixed point),
independent of the device code: dense int64 numpy, np.unique for the undirected edges and their face counts, np.add.at for the neighbour sums,
`//` and `>>` for the rounding. Every value is an exact integer, so tests/test_gpu_meshsmooth.py compares with array_equal. It is the checker of
tests/test_meshsmooth_cpu.py too, and holds the named cases of both."""
import functools

import numpy as np

import mesh_ref as mr
import meshsimplify_ref as sref

FIX = 65536                                                     # fixed point: q = rint(v * 65536)
LO, HI = -4.0, 2097144.0                                        # the range of a referenced coordinate: -4 <= v < 2^21 - 8
QMIN, QMAX = -4 * FIX, (2 ** 21 - 8) * FIX - 1
MAX_ITEMS = 1 << 28
MAX_DEGREE = 1 << 24
MAX_ITERATIONS = 1000
FIXED, CURVE, FREE = 0, 1, 2
REFERENCED, BOUNDARY, NONMANIFOLD = 1, 2, 4                     # bits of vert_flags
KEYS = ("vertices", "vert_lattice", "vert_degree", "vert_flags", "counts")


def q16(x):
    """A factor as mesh.smooth_mesh converts it."""
    return int(np.rint(float(x) * 65536.0))


def edge_table(faces, V):
    """faces (F,nv) with valid indices -> (edges (E,2) int64 with a < b, count (E,) int64): rule 3."""
    f = np.asarray(faces, np.int64)
    s = np.stack([f, np.roll(f, -1, axis=1)], axis=2).reshape(-1, 2)
    s = s[s[:, 0] != s[:, 1]]                                   # a side with equal ends is ignored
    key, count = np.unique((s.min(axis=1) << 28) | s.max(axis=1), return_counts=True)
    return np.stack([key >> 28, key & ((1 << 28) - 1)], axis=1), count.astype(np.int64)


def _pass(q, w, a, b, d, moves):
    """One Jacobi pass with factor w over the directed pairs a -> b (a gathers b), d = pairs per vertex, moves = who may move: rule 6."""
    S = np.zeros_like(q)
    np.add.at(S, a, q[b])
    dd = np.maximum(d, 1)[:, None]
    mean = (2 * S + dd) // (2 * dd)                             # floor division
    step = (w * (mean - q) + 32768) >> 16                       # arithmetic shift
    return np.where(moves[:, None], np.clip(q + step, QMIN, QMAX), q)


def _means(q, a, b, d):
    S = np.zeros_like(q)
    np.add.at(S, a, q[b])
    dd = np.maximum(d, 1)[:, None]
    return (2 * S + dd) // (2 * dd)


def smooth(verts, faces, iterations=10, lam_q16=32768, mu_q16=-34734, boundary=CURVE, origin=(0.0, 0.0, 0.0), resol=1.0):
    """verts (V,3) float64 in lattice cells, faces (F,3) or (F,4) integers -> dict: vertices (V,3) float32, vert_lattice (V,3) float64,
    vert_degree (V,) int32, vert_flags (V,) uint8, counts (4,) int64 = E, boundary edges, non-manifold edges, referenced vertices; and what the
    tests look at beside them: q (V,3) int64 (0 where unreferenced), q0 the same before smoothing, bdegree (V,) int32, edges, edge_count.
    ValueError names the first offending face or the vertex."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError("verts must be (V,3)")
    if f.ndim != 2 or f.shape[1] not in (3, 4):
        raise ValueError("nv: faces must be (F,3) or (F,4)")
    f = f.astype(np.int64)
    V, F = v.shape[0], f.shape[0]
    origin = np.asarray(origin, np.float64).reshape(3)
    resol = float(resol)
    if int(iterations) != iterations or not 0 <= int(iterations) <= MAX_ITERATIONS:
        raise ValueError("iterations = %r: an integer in 0 .. 1000" % (iterations,))
    for name, w in (("lam_q16", lam_q16), ("mu_q16", mu_q16)):
        if int(w) != w or not -65536 <= int(w) <= 65536:
            raise ValueError("%s = %r: an integer in -65536 .. 65536" % (name, w))
    if boundary not in (FIXED, CURVE, FREE):
        raise ValueError("boundary = %r: 0 (fixed), 1 (curve) or 2 (free)" % (boundary,))
    if not (np.isfinite(resol) and resol > 0):
        raise ValueError("resol = %r must be finite and > 0" % (resol,))
    if not np.isfinite(origin).all():
        raise ValueError("origin is not finite")
    if V > MAX_ITEMS or F > MAX_ITEMS:
        raise ValueError("at most 2^28 vertices and faces")
    iterations, lam_q16, mu_q16 = int(iterations), int(lam_q16), int(mu_q16)
    bad_index = ((f < 0) | (f >= V)).any(axis=1)
    referenced = np.zeros((V,), bool)
    referenced[f[~bad_index].reshape(-1)] = True
    with np.errstate(invalid="ignore"):
        in_range = ((v >= LO) & (v < HI)).all(axis=1)           # (NaN fails)
    bad_range = np.zeros((F,), bool)
    bad_range[~bad_index] = (~in_range[f[~bad_index]]).any(axis=1)
    code = np.where(bad_index, 1, np.where(bad_range, 2, 0))
    if code.any():
        first = int(np.nonzero(code)[0][0])
        raise ValueError("face %d names a vertex outside [0, %d)" % (first, V) if code[first] == 1 else
                         "face %d: a coordinate of one of its vertices is outside [-4, 2^21 - 8)" % first)
    q = np.zeros((V, 3), np.int64)
    q[referenced] = np.rint(v[referenced] * float(FIX)).astype(np.int64)       # ties to even, exact
    q0 = q.copy()
    edges, count = edge_table(f, V)
    E = edges.shape[0]
    a = np.concatenate([edges[:, 0], edges[:, 1]])
    b = np.concatenate([edges[:, 1], edges[:, 0]])
    on_b = np.concatenate([count == 1, count == 1])
    degree = np.bincount(a, minlength=V).astype(np.int64)
    bdegree = np.bincount(a[on_b], minlength=V).astype(np.int64)
    if degree.max(initial=0) >= MAX_DEGREE:
        raise ValueError("vertex %d has %d edges: at most 2^24 - 1" % (int(np.argmax(degree >= MAX_DEGREE)), int(degree.max())))
    is_b = bdegree > 0
    flags = referenced.astype(np.uint8) * REFERENCED | is_b.astype(np.uint8) * BOUNDARY
    nm = np.zeros((V,), bool)
    nm[edges[count > 2].reshape(-1)] = True
    flags |= nm.astype(np.uint8) * NONMANIFOLD
    # rule 5
    if boundary == CURVE:
        use = ~is_b[a] | on_b                                   # a boundary vertex gathers across boundary edges only
        a, b = a[use], b[use]
        d = np.where(is_b, bdegree, degree)
    else:
        d = degree
    moves = d > 0
    if boundary == FIXED:
        moves &= ~is_b
    for _ in range(iterations):
        q = _pass(q, lam_q16, a, b, d, moves)
        if mu_q16 != 0:
            q = _pass(q, mu_q16, a, b, d, moves)
    lattice = v.copy()
    lattice[referenced] = q[referenced].astype(np.float64) / float(FIX)
    with np.errstate(invalid="ignore"):
        mm = (origin + resol * lattice).astype(np.float32)
    return dict(vertices=mm, vert_lattice=lattice, vert_degree=degree.astype(np.int32), vert_flags=flags,
                counts=np.asarray([E, int((count == 1).sum()), int((count > 2).sum()), int(referenced.sum())], np.int64),
                q=q, q0=q0, bdegree=bdegree.astype(np.int32), edges=edges, edge_count=count)


# ---- properties ----------------------------------------------------------------------------------------------------------------------------------
def roughness(q, edges):
    """Sum over the vertices with an edge of |mean - q|^2 in cells^2, mean = rule 6's over all edge neighbours."""
    a = np.concatenate([edges[:, 0], edges[:, 1]])
    b = np.concatenate([edges[:, 1], edges[:, 0]])
    d = np.bincount(a, minlength=q.shape[0]).astype(np.int64)
    diff = (_means(q, a, b, d) - q)[d > 0].astype(np.float64) / FIX
    return float((diff * diff).sum())


# ---- named cases: (verts, faces). Do not modify the results. -------------------------------------------------------------------------------------
def quads_of(tris):
    """The (Q,4) quads a triangulate() of them gave: triangles (0,1,2), (0,2,3) in quad order."""
    t = np.asarray(tris).reshape(-1, 2, 3)
    return np.concatenate([t[:, 0], t[:, 1, 2:]], axis=1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def sheet_case(quads=True):
    v, t = sref.sheet_case()
    return v, (quads_of(t) if quads else t)


@functools.lru_cache(maxsize=None)
def sphere_case(R, quads=True):
    m = mr.mesh_ref(*mr.scene_args(mr.sphere_scene(R)))
    return m["vert_lattice"], (m["quads"].astype(np.int32) if quads else sref.triangulate(m["quads"]).astype(np.int32))


def surface_case():
    return sref.surface_case()


@functools.lru_cache(maxsize=None)
def surface_simplified_case(k):
    r = sref.reference("surface", k)
    return r["vert_lattice"], r["faces"]


def soup_case():
    return sref.soup_case()


@functools.lru_cache(maxsize=None)
def fan_case(n):
    """One hub (vertex 0) at (16, 16, 16) with n triangles around it: rim vertex i on a circle that wobbles in z, closed."""
    t = 2 * np.pi * np.arange(n) / n
    rim = np.stack([16 + 10 * np.cos(t), 16 + 10 * np.sin(t), 14 + 3 * np.cos(7 * t)], axis=1)
    v = np.concatenate([[[16.0, 16.0, 16.0]], rim])
    i = np.arange(n)
    return v, np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], axis=1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def rules_case():
    """8 vertices and 6 triangles: face 0 = face 1 (count 2 on their edges), face 2 has a side with equal ends (4, 4), vertex 7 is unreferenced
    and not a number, vertex 5 sits at exactly -4 and vertex 6 just under 2^21 - 8."""
    v = np.asarray([(1, 1, 1), (5, 1, 1.25), (1, 5, 1.5), (5, 5, 2), (3, 9, 1), (-4, -4, -4), (np.nextafter(HI, 0), 3, 3), (np.nan, 0, np.inf)],
                   np.float64)
    f = np.asarray([[0, 1, 2], [0, 1, 2], [2, 4, 4], [1, 3, 2], [0, 5, 1], [3, 6, 1]], np.int32)
    return v, f


@functools.lru_cache(maxsize=None)
def clamp_case():
    """A triangle fan whose hub lies near the range's lower end: lam = mu = -1 throws it outwards until the clamp holds it."""
    v = np.asarray([(-3, -3, -3), (-2, -3.5, -3), (-3.5, -2, -3), (-3, -3, -1.5), (-1, -1, -1)], np.float64)
    f = np.asarray([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 4, 2], [2, 4, 3], [3, 4, 1]], np.int32)
    return v, f


CASES = dict(sheet_q=lambda: sheet_case(True), sheet_t=lambda: sheet_case(False),
             sphere6_q=lambda: sphere_case(6, True), sphere6_t=lambda: sphere_case(6, False), sphere9_q=lambda: sphere_case(9, True),
             sphere12_q=lambda: sphere_case(12, True), sphere12_t=lambda: sphere_case(12, False),
             surface=surface_case, surface_k2=lambda: surface_simplified_case(2), surface_k8=lambda: surface_simplified_case(8),
             soup=soup_case, fan300=lambda: fan_case(300), fan5000=lambda: fan_case(5000), rules=rules_case, clamp=clamp_case)


@functools.lru_cache(maxsize=None)
def reference(name, iterations=10, lam_q16=32768, mu_q16=-34734, boundary=CURVE, origin=(0.0, 0.0, 0.0), resol=1.0):
    """smooth of a named case, computed once per configuration and shared (read-only) among the tests."""
    v, f = CASES[name]()
    return smooth(v, f, iterations, lam_q16, mu_q16, boundary, origin, resol)
