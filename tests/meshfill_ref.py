"""CPU restatement of the hole filler (the closed boundary loops of a triangle or quad mesh, each decided - hole or rim -
and every hole within max_len capped by a fan of triangles around its centroid), independent of the device code: the edges and their counts from
meshsmooth_ref.edge_table, the boundary components by repeated minimum over the boundary edges, int64 numpy for the sums and the floor
division, the vote's fp64 expression written out component by component. Every value is an exact integer or one fixed-order fp64 expression, so
tests/test_gpu_meshfill.py compares with array_equal. It is the checker of tests/test_meshfill_cpu.py too, and holds the named cases of both."""
import functools

import numpy as np

import meshsmooth_ref as sm

FIX = sm.FIX
NONE, FILLED, LONG, RIM, COMPLEX = 0, 1, 2, 3, 4                # vert_loop
HOLES, ANY = 0, 1                                              # orientation
MAX_LEN_LO, MAX_LEN_HI = 3, 65536
COUNT_NAMES = ("n_edges", "n_boundary_edges", "n_boundary_components", "n_filled", "n_long", "n_rims", "n_complex", "n_new_faces")
KEYS = ("new_vertices", "new_vert_lattice", "loop_root", "loop_len", "new_faces", "vert_loop", "counts")


def _cross(a, b):
    """Rule 6's cross product, per component."""
    return (a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0])


def vote_dot(qp, qr, qs, c):
    """(n,3) int64 each -> (n,) float64: dot = (a.x*b.x + a.y*b.y) + a.z*b.z with a = d1 x d2, b = d1 x d3."""
    d1, d2, d3 = (qr - qp).astype(np.float64), (qs - qp).astype(np.float64), (c - qp).astype(np.float64)
    ax, ay, az = _cross(d1, d2)
    bx, by, bz = _cross(d1, d3)
    return (ax * bx + ay * by) + az * bz


def fill(verts, faces, max_len=64, orientation=HOLES, origin=(0.0, 0.0, 0.0), resol=1.0):
    """verts (V,3) float64 in lattice cells, faces (F,3) or (F,4) integers -> dict: new_vertices (H,3) float32, new_vert_lattice (H,3) float64,
    loop_root (H,) int32, loop_len (H,) int32, new_faces (T,3) int32, vert_loop (V,) uint8, counts (8,) int64 = E, boundary edges, boundary
    components, filled loops, long loops, rims, complex components, new triangles; and what the tests look at beside them: loops - a list of
    dicts (root, n, state, votes or None) by ascending root - and zero_votes, the number of votes that were exactly 0. ValueError as
    meshsmooth_ref.smooth raises it for the shared arguments."""
    if isinstance(max_len, bool) or int(max_len) != max_len or not MAX_LEN_LO <= int(max_len) <= MAX_LEN_HI:
        raise ValueError("max_len = %r: an integer in 3 .. 65536" % (max_len,))
    if orientation not in (HOLES, ANY):
        raise ValueError("orientation = %r: 0 (holes) or 1 (any)" % (orientation,))
    max_len = int(max_len)
    base = sm.smooth(verts, faces, 0, 0, 0, sm.CURVE, origin, resol)       # rules 1 to 4 of section 4.16 and its refusals
    origin = np.asarray(origin, np.float64).reshape(3)
    resol = float(resol)
    f = np.asarray(faces).astype(np.int64)
    V, (F, nv) = np.asarray(verts).shape[0], f.shape
    q, edges, count = base["q"], base["edges"], base["edge_count"]
    vert_loop = np.zeros((V,), np.uint8)
    empty = dict(new_vertices=np.zeros((0, 3), np.float32), new_vert_lattice=np.zeros((0, 3), np.float64), loop_root=np.zeros((0,), np.int32),
                 loop_len=np.zeros((0,), np.int32), new_faces=np.zeros((0, 3), np.int32), vert_loop=vert_loop, loops=[], zero_votes=0)
    if F == 0:
        return dict(empty, counts=np.zeros((8,), np.int64))
    # rule 1: the sides on edges of count 1, in their face's direction, each with its third vertex
    p, r, s = (np.stack([f[:, (k + j) % nv] for k in range(nv)], axis=1).reshape(-1) for j in (0, 1, 2))
    keep = p != r
    p, r, s = p[keep], r[keep], s[keep]
    key = (np.minimum(p, r) << 28) | np.maximum(p, r)
    edge_key = (edges[:, 0] << 28) | edges[:, 1]
    on_b = count[np.searchsorted(edge_key, key)] == 1
    p, r, s = p[on_b], r[on_b], s[on_b]
    out, inn = np.bincount(p, minlength=V), np.bincount(r, minlength=V)
    nonman = (base["vert_flags"] & sm.NONMANIFOLD) != 0
    on_boundary = (base["vert_flags"] & sm.BOUNDARY) != 0
    simple = (out == 1) & (inn == 1) & ~nonman
    # rule 3: components by their smallest vertex
    label = np.arange(V)
    while True:
        new = label.copy()
        np.minimum.at(new, p, label[r])
        np.minimum.at(new, r, label[p])
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    roots = np.unique(label[on_boundary])
    length = np.bincount(label[p], minlength=V)                 # half-edges per component, at its root
    complex_ = np.zeros((V,), bool)
    complex_[label[on_boundary & ~simple]] = True
    nxt, third = np.zeros((V,), np.int64), np.zeros((V,), np.int64)
    nxt[p], third[p] = r, s                                     # read only where out = 1
    # rules 4 to 6 for the vertices of the simple loops within max_len (on such a loop every vertex has out = 1: n is also their number)
    candidate = np.zeros((V,), bool)
    candidate[roots] = ~complex_[roots] & (length[roots] <= max_len)
    cv = np.nonzero(on_boundary & candidate[label])[0]
    S = np.zeros((V, 3), np.int64)
    np.add.at(S, label[cv], q[cv])
    n_ = np.maximum(length, 1)[:, None]
    cent = (2 * S + n_) // (2 * n_)                             # floor division: rule 5
    votes, zero_votes = np.zeros((V,), np.int64), 0
    if orientation == HOLES:
        dot = vote_dot(q[cv], q[nxt[cv]], q[third[cv]], cent[label[cv]])
        votes = np.bincount(label[cv][dot < 0], minlength=V)
        zero_votes = int((dot == 0).sum())
    state = np.zeros((V,), np.uint8)                            # per root
    state[roots] = np.where(complex_[roots], COMPLEX, np.where(length[roots] > max_len, LONG, FILLED))
    if orientation == HOLES:
        state[roots[(state[roots] == FILLED) & ~(2 * votes[roots] > length[roots])]] = RIM
    vert_loop[on_boundary] = state[label[on_boundary]]
    loops = [dict(root=int(x), n=int(length[x]), state=int(state[x]), votes=int(votes[x]) if orientation == HOLES and candidate[x] else None)
             for x in roots.tolist()]
    filled = roots[state[roots] == FILLED]
    H = filled.size
    rank = np.zeros((V,), np.int64)
    rank[filled] = np.arange(H)
    lattice = cent[filled].astype(np.float64) / float(FIX)
    on_filled = np.nonzero(vert_loop == FILLED)[0]              # ascending p
    new_faces = np.stack([nxt[on_filled], on_filled, V + rank[label[on_filled]]], axis=1)
    states = [lp["state"] for lp in loops]
    counts = np.asarray([edges.shape[0], int((count == 1).sum()), len(loops), H, states.count(LONG), states.count(RIM), states.count(COMPLEX),
                         new_faces.shape[0]], np.int64)
    return dict(new_vertices=(origin + resol * lattice).astype(np.float32), new_vert_lattice=lattice, loop_root=filled.astype(np.int32),
                loop_len=length[filled].astype(np.int32), new_faces=new_faces.astype(np.int32), vert_loop=vert_loop,
                counts=counts, loops=loops, zero_votes=zero_votes)


def filled_mesh(verts, faces, r):
    """-> (verts (V + H,3) float64, triangles int32): the input, its quads triangulated, with fill's result r appended."""
    f = np.asarray(faces)
    tris = f if f.shape[1] == 3 else np.stack([f[:, [0, 1, 2]], f[:, [0, 2, 3]]], axis=1).reshape(-1, 3)
    return np.concatenate([np.asarray(verts, np.float64), r["new_vert_lattice"]]), np.concatenate([tris, r["new_faces"]]).astype(np.int32)


# ---- named cases: (verts, faces). Do not modify the results. -------------------------------------------------------------------------------------
def _without(v, f, drop):
    return v, np.ascontiguousarray(f[~drop])


@functools.lru_cache(maxsize=None)
def sheet_hole_case(quads=True):
    """The sheet without the faces whose centroid is within 1.0 cell of the sheet's centre in x and y."""
    v, f = sm.sheet_case(quads)
    centre = (v[:, :2].min(axis=0) + v[:, :2].max(axis=0)) / 2
    return _without(v, f, (np.abs(v[f].mean(axis=1)[:, :2] - centre) <= 1.0).all(axis=1))


def _cap(v, f, axis, sign, depth=2.5):
    """faces whose corners all lie beyond extreme - depth along sign * axis"""
    x = sign * v[:, axis]
    return (x[f] > x.max() - depth).all(axis=1)


@functools.lru_cache(maxsize=None)
def sphere_hole_case(R, quads=True):
    """A sphere shell without the faces whose corners all have z > z_max - 2.5."""
    v, f = sm.sphere_case(R, quads)
    return _without(v, f, _cap(v, f, 2, 1))


@functools.lru_cache(maxsize=None)
def sphere_three_holes_case():
    """The R = 12 quad shell with three caps removed, along +z, -x and +y: ranks and triangle places interleave."""
    v, f = sm.sphere_case(12, True)
    return _without(v, f, _cap(v, f, 2, 1) | _cap(v, f, 0, -1) | _cap(v, f, 1, 1))


def _grid(nx, ny):
    """(nx + 1) * (ny + 1) vertices at z = 3 and the nx * ny quads between them, counter-clockwise seen from +z; vertex (i, j) = j * (nx + 1) + i."""
    i, j = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1))
    v = np.stack([i.reshape(-1) + 2.0, j.reshape(-1) + 2.0, np.full((i.size,), 3.0)], axis=1)
    a = (np.arange(ny)[:, None] * (nx + 1) + np.arange(nx)[None, :]).reshape(-1)
    return v, np.stack([a, a + 1, a + nx + 2, a + nx + 1], axis=1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def pinch_case():
    """A 6 x 6 grid of quads without the cells (2, 2) and (3, 3): two one-cell holes that share the vertex (3, 3)."""
    v, f = _grid(6, 6)
    cell = np.arange(36)
    return _without(v, f, (cell == 2 * 6 + 2) | (cell == 3 * 6 + 3))


@functools.lru_cache(maxsize=None)
def two_holes_case():
    """The same grid without the cells (1, 1) and (4, 3): two separate one-cell holes."""
    v, f = _grid(6, 6)
    cell = np.arange(36)
    return _without(v, f, (cell == 1 * 6 + 1) | (cell == 3 * 6 + 4))


@functools.lru_cache(maxsize=None)
def fan3_case():
    """Three triangles on the edge (0, 1): it is non-manifold, and the six other edges form one boundary component through 0 and 1."""
    v = np.asarray([(4, 4, 4), (8, 4, 4), (6, 8, 4), (6, 2, 7), (6, 2, 1)], np.float64)
    return v, np.asarray([[0, 1, 2], [0, 1, 3], [0, 1, 4]], np.int32)


@functools.lru_cache(maxsize=None)
def opposed_case():
    """Two triangles on the edge (0, 1) that both run 0 -> 1: an interior edge between faces of opposed orientation; vertex 1 has out = 2."""
    v = np.asarray([(4, 4, 4), (8, 4, 4), (6, 8, 4), (6, 1, 4)], np.float64)
    return v, np.asarray([[0, 1, 2], [0, 1, 3]], np.int32)


@functools.lru_cache(maxsize=None)
def single_case(quad=True):
    v = np.asarray([(4, 4, 5), (9, 4, 5), (9, 8, 5), (4, 8, 5)], np.float64)
    return (v, np.asarray([[0, 1, 2, 3]], np.int32)) if quad else (v[:3], np.asarray([[0, 1, 2]], np.int32))


@functools.lru_cache(maxsize=None)
def annulus_case(n=4096):
    """A strip of n quads between an inner circle (vertices 0 .. n-1, radius 700) and an outer one (n .. 2n-1, radius 704), counter-clockwise seen
    from +z: the inner loop is a hole of n edges, the outer one a rim of n edges."""
    t = 2 * np.pi * np.arange(n) / n
    ring = lambda rad: np.stack([1000 + rad * np.cos(t), 1000 + rad * np.sin(t), np.full((n,), 9.0)], axis=1)
    i = np.arange(n)
    j = (i + 1) % n
    return np.concatenate([ring(700.0), ring(704.0)]), np.stack([i, n + i, n + j, j], axis=1).astype(np.int32)


CASES = dict(sm.CASES)
CASES.update(sheet_hole_q=lambda: sheet_hole_case(True), sheet_hole_t=lambda: sheet_hole_case(False),
             sphere6_hole_q=lambda: sphere_hole_case(6, True), sphere6_hole_t=lambda: sphere_hole_case(6, False),
             sphere12_hole_q=lambda: sphere_hole_case(12, True), sphere12_holes3_q=sphere_three_holes_case,
             pinch=pinch_case, two_holes=two_holes_case, fan3=fan3_case, opposed=opposed_case,
             single_q=lambda: single_case(True), single_t=lambda: single_case(False), annulus4096=annulus_case)


@functools.lru_cache(maxsize=None)
def reference(name, max_len=64, orientation=HOLES, origin=(0.0, 0.0, 0.0), resol=1.0):
    """fill of a named case, computed once per configuration and shared (read-only) among the tests."""
    v, f = CASES[name]()
    return fill(v, f, max_len, orientation, origin, resol)
