"""CPU restatement of the mesh simplifier (vertex clustering on a lattice of `cell` lattice cells per axis), independent
of the device code: dense numpy, np.unique for the clusters and the duplicate faces, np.add.at / np.minimum.at for the sums and the
representative member. Every decision is an exact integer, so tests/test_gpu_meshsimplify.py compares with array_equal. It is the checker of
tests/test_meshsimplify_cpu.py too, and holds the named cases of both."""
import functools

import numpy as np

import mesh_ref as mr

FIX = 256                                                       # fixed point: q = rint(v * 256)
BIAS = 4 * FIX                                                  # 4 cells: the mesher's vertices go down to about -1
LO, HI = -4.0, 2097144.0                                        # the range of a referenced coordinate: -4 <= v < 2^21 - 8
MAX_CLUSTERS = 1 << 21                                          # a face key packs three cluster numbers of 21 bits
MAX_ITEMS = 1 << 28
KEYS = ("vertices", "vert_lattice", "vert_rep", "vert_count", "faces", "face_src", "vert_cluster")


def _key(t):
    t = np.asarray(t, np.int64)
    return (t[:, 0] << 42) | (t[:, 1] << 21) | t[:, 2]


def simplify(verts, faces, cell, placement=0, origin=(0.0, 0.0, 0.0), resol=1.0):
    """verts (V,3) float64 in lattice cells, faces (F,3) integers, cell 2..64, placement 0 (mean) / 1 (member) -> dict: vertices (C,3) float32,
    vert_lattice (C,3) float64, vert_rep (C,) int32, vert_count (C,) int32, faces (G,3) int32, face_src (G,) int32, vert_cluster (V,) int32, and
    the figures the tests pin: clusters (P), collapsed, duplicates, largest (members of the largest cluster). ValueError names the first
    offending face."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V, F = v.shape[0], f.shape[0]
    k = int(cell)
    origin = np.asarray(origin, np.float64).reshape(3)
    resol = float(resol)
    if k != cell or not 2 <= k <= 64:
        raise ValueError("cell = %r: an integer in 2 .. 64" % (cell,))
    if placement not in (0, 1):
        raise ValueError("placement = %r: 0 (mean) or 1 (member)" % (placement,))
    if not (np.isfinite(resol) and resol > 0):
        raise ValueError("resol = %r must be finite and > 0" % (resol,))
    if not np.isfinite(origin).all():
        raise ValueError("origin is not finite")
    if V > MAX_ITEMS or F > MAX_ITEMS:
        raise ValueError("at most 2^28 vertices and faces")
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
    out = dict(vertices=np.zeros((0, 3), np.float32), vert_lattice=np.zeros((0, 3), np.float64), vert_rep=np.zeros((0,), np.int32),
               vert_count=np.zeros((0,), np.int32), faces=np.zeros((0, 3), np.int32), face_src=np.zeros((0,), np.int32),
               vert_cluster=np.full((V,), -1, np.int32), clusters=0, collapsed=0, duplicates=0, largest=0)
    if F == 0:
        return out
    # clusters of the referenced vertices, numbered by ascending owner (= smallest member)
    idx = np.nonzero(referenced)[0]
    side = FIX * k
    q = np.rint(v[idx] * float(FIX)).astype(np.int64)
    c = np.floor_divide(q + BIAS, side)
    assert c.min() >= 0 and c.max() < (1 << 21)
    _, first, inv = np.unique(_key(c), return_index=True, return_inverse=True)     # idx ascends: the first occurrence is the smallest index
    inv = np.asarray(inv).reshape(-1)
    owner = idx[first]
    rank = np.empty((owner.size,), np.int64)
    rank[np.argsort(owner)] = np.arange(owner.size)
    pnum = rank[inv]
    P = int(owner.size)
    if P >= MAX_CLUSTERS:
        raise ValueError("%d clusters: at most 2^21 - 1, choose a larger cell" % P)
    S = np.zeros((P, 3), np.int64)
    np.add.at(S, pnum, q)
    n = np.bincount(pnum, minlength=P).astype(np.int64)
    e = 2 * (q - (c * side - BIAS)) - side
    d = (e * e).sum(axis=1)
    assert d.max() < 3 << 28
    best = np.full((P,), np.iinfo(np.int64).max, np.int64)
    np.minimum.at(best, pnum, (d << 32) | idx)
    rep = best & 0xffffffff
    vnum = np.full((V,), -1, np.int64)
    vnum[idx] = pnum
    # faces
    t = vnum[f]
    alive = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    src = np.nonzero(alive)[0]
    ta = t[alive]
    rot = np.take_along_axis(ta, (np.argmin(ta, axis=1)[:, None] + np.arange(3)) % 3, axis=1) if ta.size else ta
    _, ffirst = np.unique(_key(rot), return_index=True)         # src ascends: the first occurrence is the smallest input index
    keep = np.sort(ffirst)
    rot, face_src = rot[keep], src[keep]
    used = np.zeros((P,), bool)
    used[rot.reshape(-1)] = True
    cnum = np.cumsum(used) - 1
    sel = np.nonzero(used)[0]
    if placement == 0:
        lattice = (S[sel].astype(np.float64) / n[sel].astype(np.float64)[:, None]) / float(FIX)
    else:
        lattice = v[rep[sel]].copy()
    out.update(vertices=(origin + resol * lattice).astype(np.float32), vert_lattice=lattice, vert_rep=rep[sel].astype(np.int32),
               vert_count=n[sel].astype(np.int32), faces=cnum[rot].astype(np.int32).reshape(-1, 3), face_src=face_src.astype(np.int32),
               vert_cluster=np.where((vnum >= 0) & used[np.maximum(vnum, 0)], cnum[np.maximum(vnum, 0)], -1).astype(np.int32),
               clusters=P, collapsed=int(F - src.size), duplicates=int(src.size - keep.size), largest=int(n.max()))
    return out


# ---- properties ----------------------------------------------------------------------------------------------------------------------------------
def tri_edge_counts(faces):
    """-> (undirected edges (E,2), number of triangles on each)."""
    t = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.stack([t, np.roll(t, -1, axis=1)], axis=2).reshape(-1, 2)
    return np.unique(np.sort(e, axis=1), axis=0, return_counts=True)


def tri_volume(verts, faces):
    v, t = np.asarray(verts, np.float64), np.asarray(faces, np.int64).reshape(-1, 3)
    return float(np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0)


def max_move(verts, r):
    """The largest distance, in cells, from an input vertex with a cluster to its cluster's output vertex."""
    vc = r["vert_cluster"]
    m = vc >= 0
    if not m.any():
        return 0.0
    return float(np.sqrt(((np.asarray(verts, np.float64)[m] - r["vert_lattice"][vc[m]]) ** 2).sum(axis=1)).max())


def check_invariants(verts, faces, r):
    """What holds of every output: three distinct indices per face, no two equal rows, face_src ascending, vert_cluster consistent with vert_rep
    and vert_count, every output vertex used."""
    C, G = r["vert_lattice"].shape[0], r["faces"].shape[0]
    t = r["faces"].astype(np.int64)
    assert r["vertices"].shape == (C, 3) and r["vert_rep"].shape == (C,) and r["vert_count"].shape == (C,) and r["face_src"].shape == (G,)
    if G:
        assert t.min() >= 0 and t.max() < C
        assert (t[:, 0] != t[:, 1]).all() and (t[:, 1] != t[:, 2]).all() and (t[:, 0] != t[:, 2]).all()
        assert (t[:, 0] < t[:, 1]).all() and (t[:, 0] < t[:, 2]).all()      # rotated: the smallest number first
        assert np.unique(t, axis=0).shape[0] == G
        assert (np.diff(r["face_src"]) > 0).all() and r["face_src"][0] >= 0 and r["face_src"][-1] < np.asarray(faces).reshape(-1, 3).shape[0]
    assert np.array_equal(np.unique(t), np.arange(C))
    vc = r["vert_cluster"]
    assert vc.shape == (np.asarray(verts).reshape(-1, 3).shape[0],) and vc.max(initial=-1) < C
    assert np.array_equal(np.bincount(vc[vc >= 0], minlength=C), r["vert_count"])
    assert np.array_equal(vc[r["vert_rep"]], np.arange(C))
    # the output face is the input face under the vertex map, rotated
    if G:
        m = vc[np.asarray(faces, np.int64).reshape(-1, 3)[r["face_src"]]]
        assert np.array_equal(np.sort(m, axis=1), np.sort(t, axis=1))
        assert np.array_equal(np.take_along_axis(m, (np.argmin(m, axis=1)[:, None] + np.arange(3)) % 3, axis=1), t)


# ---- named cases: (verts, faces). Do not modify the results. -------------------------------------------------------------------------------------
def triangulate(quads):
    q = np.asarray(quads).reshape(-1, 4)
    return np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], axis=1).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def sheet_case():
    """The 9 x 9 sheet at z = 7: vertex 9 i + j at (i, j, 7), 64 quads in (i, j) order, triangulated."""
    i, j = np.meshgrid(np.arange(9), np.arange(9), indexing="ij")
    v = np.stack([i.reshape(-1), j.reshape(-1), np.full(81, 7)], axis=1).astype(np.float64)
    a, b = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    a, b = a.reshape(-1), b.reshape(-1)
    quads = np.stack([9 * a + b, 9 * (a + 1) + b, 9 * (a + 1) + b + 1, 9 * a + b + 1], axis=1)
    return v, triangulate(quads).astype(np.int32)


@functools.lru_cache(maxsize=None)
def rules_case():
    """11 vertices and 8 faces in which every rule of the contract decides something (tests/test_meshsimplify_cpu.py says which)."""
    v = np.asarray([(0.25, 0.25, 0.25), (0.75, 0.5, 0.5), (4.5, 0.5, 0.5), (0.5, 4.5, 0.5), (9, 9, 9), (20.125, 20.125, 20.125),
                    (20.5, 20.25, 20.125), (20.25, 20.5, 20.25), (-0.5, 4.5, 0.5), (3, 1, 2), (1, 3, 2)], np.float64)
    f = np.asarray([[0, 2, 3], [2, 3, 1], [0, 3, 2], [0, 1, 2], [3, 1, 2], [5, 6, 7], [8, 0, 2], [9, 10, 2]], np.int32)
    return v, f


@functools.lru_cache(maxsize=None)
def sphere_case(R):
    m = mr.mesh_ref(*mr.scene_args(mr.sphere_scene(R)))
    return m["vert_lattice"], triangulate(m["quads"]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def surface_case():
    m = mr.surface_mesh_reference((2, 2, 1))
    return m["vert_lattice"], triangulate(m["quads"]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def soup_case():
    rng = np.random.default_rng(2024)
    v = rng.random((5000, 3)) * 36 - 3.5
    f = rng.integers(0, 4990, (20000, 3))
    return v, f.astype(np.int32)


CASES = dict(sheet=sheet_case, rules=rules_case, sphere6=lambda: sphere_case(6), sphere9=lambda: sphere_case(9), sphere12=lambda: sphere_case(12),
             surface=surface_case, soup=soup_case)


@functools.lru_cache(maxsize=None)
def reference(name, cell, placement=0, origin=(0.0, 0.0, 0.0), resol=1.0):
    """simplify of a named case, computed once per configuration and shared (read-only) among the tests."""
    v, f = CASES[name]()
    return simplify(v, f, cell, placement, origin, resol)
