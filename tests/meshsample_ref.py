"""numpy restatement of the surface sampling of a triangle mesh (rules 1-4): the checker of sn_mesh_sample. Dense
arrays, np.repeat / np.cumsum; sqrt only estimates the two integers a decision hangs on (the subdivision count n, the row t of a sample), an
integer predicate corrects each by +-1. All float arithmetic is float64, one rounding per operation."""
import functools

import numpy as np

MAX_N = 32768


def len2(e):
    return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]


def _first(bad, text):
    if bad.any():
        raise ValueError("face %d %s" % (int(np.nonzero(bad)[0][0]), text))


def subdivisions(verts, faces, dst):
    """(F,) int64 n_f. ValueError (rule 4) naming the first offending face, or for a bad dst."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    dst = float(dst)
    if not (np.isfinite(dst) and dst > 0):
        raise ValueError("dst must be finite and > 0")
    bad_index = ((f < 0) | (f >= v.shape[0])).any(axis=1)
    safe = np.where(bad_index[:, None], 0, f)
    bad_finite = ~bad_index & (~np.isfinite(v[safe].reshape(-1, 9)).all(axis=1) if v.shape[0] else False)
    A, B, C = (np.where((bad_index | bad_finite)[:, None], 0.0, v[safe[:, i]]) if v.shape[0] else np.zeros((f.shape[0], 3)) for i in range(3))
    with np.errstate(all="ignore"):
        L2 = np.maximum(np.maximum(len2(B - A), len2(C - A)), len2(C - B))
        q = L2 / (dst * dst)
        bad_n = ~bad_index & ~bad_finite & ~(q <= float(MAX_N) * float(MAX_N))
        q = np.where(bad_n, 1.0, q)
        n = np.maximum(np.ceil(np.sqrt(q)).astype(np.int64), 1)
    down = (n > 1) & (((n - 1) * (n - 1)).astype(np.float64) >= q)
    up = ~down & ((n * n).astype(np.float64) < q)
    n = n - down + up
    bad = bad_index | bad_finite | bad_n
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        _first(bad_index[:i + 1], "names a vertex outside [0, %d)" % v.shape[0])
        _first(bad_finite[:i + 1], "has a vertex with a coordinate that is not finite")
        _first(bad_n[:i + 1], "needs more than %d subdivisions" % MAX_N)
    assert ((n * n).astype(np.float64) >= q).all() and ((n == 1) | (((n - 1) * (n - 1)).astype(np.float64) < q)).all()
    return n


def isqrt(k):
    """t with t*t <= k < (t+1)*(t+1), elementwise on int64 k >= 0."""
    t = np.floor(np.sqrt(k.astype(np.float64))).astype(np.int64)
    t = t - (t * t > k)
    t = t + ((t + 1) * (t + 1) <= k)
    assert ((t * t <= k) & (k < (t + 1) * (t + 1))).all()
    return t


def offsets(n):
    """(F + 1,) int64 exclusive offsets of the faces' n*n samples; ValueError when the total exceeds 2^31 - 1."""
    off = np.zeros(n.size + 1, np.int64)
    np.cumsum(n * n, out=off[1:])
    over = off[1:] > (1 << 31) - 1
    if over.any():
        raise ValueError("face %d takes the samples past 2^31 - 1" % int(np.nonzero(over)[0][0]))
    return off


def sample(verts, faces, dst):
    """-> (points (M,3) float64, tri (M,) int32): samples in face order, then k."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    n = subdivisions(v, f, dst)
    off = offsets(n)
    M = int(off[-1])
    tri = np.repeat(np.arange(f.shape[0], dtype=np.int64), n * n)
    if M == 0:
        return np.zeros((0, 3), np.float64), np.zeros((0,), np.int32)
    k = np.arange(M, dtype=np.int64) - off[tri]
    t = isqrt(k)
    w = k - t * t
    c = w >> 1
    odd = (w & 1) == 1
    beta = 3 * t - 3 * c + np.where(odd, -1, 1)
    gamma = 3 * c + np.where(odd, 2, 1)
    den = (3 * n[tri]).astype(np.float64)
    u, vv = beta.astype(np.float64) / den, gamma.astype(np.float64) / den
    A, B, C = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    AB, AC = B - A, C - A
    points = A[tri] + (AB[tri] * u[:, None] + AC[tri] * vv[:, None])
    return points, tri.astype(np.int32)


# ---- meshes the tests share ---------------------------------------------------------------------------------------------------------------------
RIGHT = (np.asarray([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.asarray([[0, 1, 2]], np.int32))
HALF = (np.asarray([[0.0, 0, 0], [1, 0, 0], [0, 0.5, 0]]), np.asarray([[0, 1, 2]], np.int32))
SCALENE = (np.asarray([[0.3, -0.2, 0.1], [1.7, 0.4, 0.5], [0.6, 1.1, -0.4]]), np.asarray([[0, 1, 2]], np.int32))
NEEDLE = (np.asarray([[0.0, 0, 0], [5, 0, 0], [0, 0.01, 0]]), np.asarray([[0, 1, 2]], np.int32))
QUAD = (np.asarray([[0.0, 0, 0], [0.4, 0, 0], [0.4, 0.4, 0], [0, 0.4, 0]]), np.asarray([[0, 1, 2], [0, 2, 3]], np.int32))
DEGENERATE = (np.asarray([[0.25, -1.5, 3.0]] * 3), np.asarray([[0, 1, 2]], np.int32))


def surface_points(verts, face, count, rs):
    """count uniform random points of one triangle."""
    a, b = rs.uniform(0, 1, (2, count))
    flip = a + b > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    A, B, C = (np.asarray(verts, np.float64)[i] for i in face)
    return A + a[:, None] * (B - A) + b[:, None] * (C - A)


def worst_gap(points, samples, chunk=512):
    """max over points of the distance to the nearest sample."""
    worst = 0.0
    for i in range(0, points.shape[0], chunk):
        d = points[i:i + chunk, None, :] - samples[None, :, :]
        worst = max(worst, float(np.sqrt((d * d).sum(2).min(1)).max()))
    return worst


@functools.lru_cache(maxsize=None)
def sphere_mesh():
    """The sphere shell R = 6 of mesh_ref at resol 0.4, origin (-20, -20, -20), triangulated: (vertices (V,3) float64 from the float32 mm
    positions, triangles (1452,3) int32). Do not modify."""
    import mesh_ref as mr
    m = mr.mesh_ref(*mr.scene_args(mr.sphere_scene(6, split=True)), origin=(-20.0, -20.0, -20.0), resol=0.4)
    q = np.asarray(m["quads"]).reshape(-1, 4)
    tris = np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], axis=1).reshape(-1, 3).astype(np.int32)
    return np.asarray(m["verts_mm"], np.float32).astype(np.float64), tris


@functools.lru_cache(maxsize=None)
def sphere_samples(dst=0.2):
    """sample() of sphere_mesh, computed once and shared. Do not modify."""
    return sample(*sphere_mesh(), dst)


@functools.lru_cache(maxsize=None)
def mixed_mesh(seed=7):
    """5,000 faces with n = 1 or 2 at dst 0.2, one face with n = 300 in the middle followed by a degenerate face; vertices from a seeded
    RandomState. -> (vertices, faces). Do not modify."""
    rs = np.random.RandomState(seed)
    F = 5000
    base = rs.uniform(-50, 50, (F, 3))
    size = np.where(rs.uniform(0, 1, F) < 0.5, 0.09, 0.19)           # two edges of this length, the third below twice it: n = 1 or 2
    e1, e2 = rs.normal(0, 1, (2, F, 3))
    e1 /= np.sqrt((e1 * e1).sum(1))[:, None]
    e2 /= np.sqrt((e2 * e2).sum(1))[:, None]
    v = np.stack([base, base + e1 * size[:, None], base + e2 * size[:, None]], axis=1).reshape(-1, 3)
    f = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    big = np.asarray([[10.0, 10, 10], [10 + 59.9, 10, 10], [10 + 20.0, 10 + 30.0, 12]])      # longest edge 59.9 = 299.5 dst: n = 300
    dot = np.asarray([[1.0, 2, 3]] * 3)
    v = np.concatenate([v, big, dot])
    extra = np.asarray([[3 * F, 3 * F + 1, 3 * F + 2], [3 * F + 3, 3 * F + 4, 3 * F + 5]], np.int32)
    f = np.concatenate([f[:F // 2], extra, f[F // 2:]])
    return v, f
