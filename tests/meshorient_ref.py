"""CPU restatement of the mesh orientation stage, independent of the device code: np.unique for the edges and their
side counts, scipy.sparse.csgraph.connected_components on the double cover, np.minimum.at for the roots, Python integers for the volumes.
Every value is an exact integer, so tests/test_gpu_meshorient.py compares bytes. It is the checker of tests/test_meshorient_cpu.py too, and
holds the cases the smoother's list (tests/meshsmooth_ref.CASES) lacks. `plant` names a fault planted in one rule: the comparison has to see
each of them."""
import functools

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import meshnormals_ref as mn
import meshsmooth_ref as sm

MAJORITY, OUTWARD = 0, 1
ORIENTABLE, CLOSED, FLIPPED, KEPT = 1, 2, 4, 8                  # bits of comp_flags
KEYS = ("faces_out", "face_flip", "face_component", "face_keep", "comp_faces", "comp_flags", "comp_vol6", "counts")
COUNTS = ("n_edges", "n_boundary_edges", "n_nonmanifold_edges", "n_links", "n_inconsistent", "n_components", "n_nonorientable", "n_closed",
          "n_flipped_faces", "n_flipped_components", "n_kept_faces", "n_kept_components")
PLANTS = ("direction", "same_face", "tie", "negation", "largest_tie")


def links_of(f, plant=None):
    """faces (F,nv) int64 with valid indices -> (lf, lg, r, on_link, edge counts): the links f < g with r = inconsistent, per face and corner
    whether the corner starts a side that lies on a link, and the side count of every edge: rules 1 and 2."""
    F, nv = f.shape
    p, r = f, np.roll(f, -1, axis=1)
    side = p != r                                               # p == r is no side
    face = np.repeat(np.arange(F, dtype=np.int64), nv).reshape(F, nv)
    d = (p < r).astype(np.int64)
    key = (np.minimum(p, r) << 28) | np.maximum(p, r)
    flat = np.flatnonzero(side.reshape(-1))
    k, fa, da = key.reshape(-1)[flat], face.reshape(-1)[flat], d.reshape(-1)[flat]
    order = np.argsort(k, kind="stable")
    k, fa, da, flat = k[order], fa[order], da[order], flat[order]
    uniq, start, count = np.unique(k, return_index=True, return_counts=True)
    two = start[count == 2]
    f1, f2, d1, d2 = fa[two], fa[two + 1], da[two], da[two + 1]
    is_link = (f1 != f2) | (plant == "same_face")
    on_link = np.zeros((F * nv,), bool)
    on_link[flat[two[is_link]]] = True
    on_link[flat[two[is_link] + 1]] = True
    f1, f2, d1, d2 = f1[is_link], f2[is_link], d1[is_link], d2[is_link]
    bad = (d1 == d2) if plant != "direction" else (d1 != d2)
    return np.minimum(f1, f2), np.maximum(f1, f2), bad.astype(np.int64), on_link.reshape(F, nv), count


def flipped(f):
    """Rule 7: (a,b,c) -> (a,c,b), (a,b,c,d) -> (a,d,c,b)."""
    return np.concatenate([f[:, :1], f[:, :0:-1]], axis=1)


def orient(verts, faces, sign=MAJORITY, min_faces=0, keep_largest=0, plant=None):
    """verts (V,3) float64 in lattice cells, faces (F,3) or (F,4) integers -> dict of KEYS as sn_mesh_orient writes them - faces_out (F,nv)
    int32, face_flip, face_keep (F,) uint8, face_component (F,) int32, comp_faces (F,) int32, comp_flags (F,) uint8, comp_vol6 (F,3) uint64,
    counts (12,) int64 - and what the tests look at beside them: rel, vol6 {piece: Python int}, n_rel {piece: int}. ValueError names the
    first offending face."""
    if sign not in (MAJORITY, OUTWARD):
        raise ValueError("sign = %r: 0 (majority) or 1 (outward)" % (sign,))
    if int(min_faces) != min_faces or min_faces < 0:
        raise ValueError("min_faces = %r must be >= 0" % (min_faces,))
    if keep_largest not in (0, 1):
        raise ValueError("keep_largest = %r: 0 or 1" % (keep_largest,))
    q, f, _ = mn.quantise(verts, faces)
    F, nv = f.shape
    out = dict(faces_out=np.zeros((F, nv), np.int32), face_flip=np.zeros((F,), np.uint8), face_component=np.zeros((F,), np.int32),
               face_keep=np.zeros((F,), np.uint8), comp_faces=np.zeros((F,), np.int32), comp_flags=np.zeros((F,), np.uint8),
               comp_vol6=np.zeros((F, 3), np.uint64), counts=np.zeros((12,), np.int64), rel=np.zeros((F,), np.int64), vol6={}, n_rel={})
    if F == 0:
        return out
    lf, lg, r, on_link, count = links_of(f, plant)
    # rule 3: the double cover
    a = np.concatenate([2 * lf, 2 * lf + 1])
    b = np.concatenate([2 * lg + r, 2 * lg + 1 - r])
    _, label = connected_components(coo_matrix((np.ones(a.shape[0], np.int8), (a, b)), shape=(2 * F, 2 * F)), directed=False)
    smallest = np.full((label.max() + 1,), 2 * F, np.int64)
    np.minimum.at(smallest, label, np.arange(2 * F, dtype=np.int64))
    root = smallest[label]
    # rule 4
    comp, rel = root[0::2] >> 1, root[0::2] & 1
    nonor = root[0::2] == root[1::2]
    assert (comp <= np.arange(F)).all() and (comp[comp] == comp).all()      # the smallest face of the piece
    assert not rel[nonor].any() and np.array_equal(nonor, nonor[comp])
    ids = np.flatnonzero(comp == np.arange(F))
    # rule 5
    n_faces = np.bincount(comp, minlength=F)
    n_rel = np.bincount(comp, weights=rel, minlength=F).astype(np.int64)
    open_ = np.zeros((F,), bool)
    open_[comp[~on_link.all(axis=1)]] = True
    closed = ~nonor & ~open_
    c = [q[f[:, k]] for k in range(nv)]
    t = (c[0] * mn._cross(c[1], c[2]).reshape(F, 3)).sum(axis=1)
    if nv == 4:
        t = t + (c[0] * mn._cross(c[2], c[3]).reshape(F, 3)).sum(axis=1)
    vol = {int(i): 0 for i in ids}
    for i, x, s in zip(comp.tolist(), t.tolist(), rel.tolist()):
        vol[i] += -x if s else x
    # rules 6 and 8
    flipc = np.zeros((F,), bool)
    for i in ids.tolist():
        if nonor[i]:
            continue
        if sign == OUTWARD and closed[i] and vol[i] != 0:
            flipc[i] = vol[i] < 0
        elif plant == "tie":
            flipc[i] = n_rel[i] >= n_faces[i] - n_rel[i]
        else:
            flipc[i] = n_rel[i] > n_faces[i] - n_rel[i]
        if flipc[i]:
            vol[i] = -vol[i] - (1 if plant == "negation" else 0)
    kept = n_faces >= min_faces
    if keep_largest:
        most = n_faces[ids].max()
        kept[ids[n_faces[ids] == most][-1 if plant == "largest_tie" else 0]] = True
    flip = (rel ^ flipc[comp]).astype(bool)
    out["faces_out"] = np.where(flip[:, None], flipped(f), f).astype(np.int32)
    out["face_flip"] = flip.astype(np.uint8)
    out["face_component"] = comp.astype(np.int32)
    out["face_keep"] = kept[comp].astype(np.uint8)
    out["comp_faces"][ids] = n_faces[ids]
    out["comp_flags"][ids] = (~nonor[ids] * ORIENTABLE + closed[ids] * CLOSED + flipc[ids] * FLIPPED + kept[ids] * KEPT).astype(np.uint8)
    out["comp_vol6"][ids] = np.asarray([mn.limbs(vol[i]) for i in ids.tolist()], np.uint64).reshape(-1, 3)
    out["counts"][:] = [count.shape[0], int((count == 1).sum()), int((count > 2).sum()), lf.shape[0], int(r.sum()), ids.shape[0],
                        int(nonor[ids].sum()), int(closed[ids].sum()), int(flip.sum()), int(flipc[ids].sum()), int(kept[comp].sum()),
                        int(kept[ids].sum())]
    out.update(rel=rel, vol6=vol, n_rel={int(i): int(n_rel[i]) for i in ids})
    return out


def same_bytes(got, want):
    """The keys of KEYS on which a result differs from the restatement, byte for byte ([]: none)."""
    return [k for k in KEYS if np.asarray(got[k]).tobytes() != np.asarray(want[k]).tobytes() or np.asarray(got[k]).shape != np.asarray(want[k]).shape]


# ---- named cases: (verts, faces). Do not modify the results. --------------------------------------------------------------------------------------
def reversed_where(f, rev):
    """faces with the rows of rev turned as rule 7 turns them."""
    return np.where(np.asarray(rev, bool)[:, None], flipped(f), f).astype(np.int32)


def scramble(name, seed=5):
    """A case of the smoother's list with faces reversed where default_rng(seed).random(F) < 0.5 -> (verts, faces, rev)."""
    v, f = sm.CASES[name]()
    rev = np.random.default_rng(seed).random(f.shape[0]) < 0.5
    return v, reversed_where(f, rev), rev


TET_V = np.asarray([(10, 10, 10), (14, 10, 10), (10, 14, 10), (10, 10, 14)], np.float64)
TET_F = np.asarray([(0, 2, 1), (0, 1, 3), (1, 2, 3), (0, 3, 2)], np.int32)      # outward: volume 64 / 6 cells^3


def tet_case(kind=""):
    if kind == "one":
        return TET_V, reversed_where(TET_F, [False, False, True, False])
    return TET_V, (reversed_where(TET_F, [True] * 4) if kind == "inward" else TET_F)


@functools.lru_cache(maxsize=None)
def moebius_case(quads=True, n=8):
    """A band of n quads between the rails i and n + i whose last quad joins the rails crosswise: a Moebius strip."""
    t = 2 * np.pi * np.arange(n) / n
    mid = np.stack([20 + 8 * np.cos(t), 20 + 8 * np.sin(t), np.full(n, 20.0)], axis=1)
    w = np.stack([np.cos(t / 2) * np.cos(t), np.cos(t / 2) * np.sin(t), np.sin(t / 2)], axis=1)
    v = np.floor(256.0 * np.concatenate([mid - 2 * w, mid + 2 * w])) / 256.0
    i = np.arange(n - 1)
    q = np.concatenate([np.stack([i, i + 1, n + i + 1, n + i], axis=1), [[n - 1, n, 0, 2 * n - 1]]]).astype(np.int32)
    return v, (q if quads else sm.sref.triangulate(q).astype(np.int32))


@functools.lru_cache(maxsize=None)
def sheet_checker_case():
    v, f = sm.sheet_case(True)
    i = np.arange(f.shape[0])
    return v, reversed_where(f, (i // 8 + i % 8) % 2 == 1)


@functools.lru_cache(maxsize=None)
def tets_case(n=1000):
    """n disjoint tetrahedra on a 10 x 10 x 10 grid of 6 cells: every other one inward, every third with one face reversed."""
    i = np.arange(n)
    shift = np.stack([i % 10, i // 10 % 10, i // 100], axis=1) * 6.0
    v = (TET_V[None] + shift[:, None]).reshape(-1, 3)
    f = (TET_F[None] + 4 * i[:, None, None]).reshape(-1, 3)
    rev = np.repeat(i % 2 == 1, 4)
    rev[4 * i[i % 3 == 0] + 2] ^= True
    return v, reversed_where(f, rev)


@functools.lru_cache(maxsize=None)
def strip_case(n=3000):
    """A triangle strip in index order, triangle i on the vertices i, i + 1, i + 2, consistent, with alternate faces reversed."""
    j = np.arange(n + 2)
    v = np.stack([10.0 + j // 2 * 0.5, 10.0 + (j % 2) * 1.0, np.full(n + 2, 5.0)], axis=1)
    i = np.arange(n)
    f = np.where((i % 2 == 0)[:, None], np.stack([i, i + 1, i + 2], axis=1), np.stack([i + 1, i, i + 2], axis=1))
    return v, reversed_where(f, i % 2 == 1)


@functools.lru_cache(maxsize=None)
def far_cube_case():
    """A cube of side 2,097,000 cells with a corner at (100, 100, 100), 12 triangles, inward: terms near 2^113 in both signs."""
    s = 2097000.0
    v = 100.0 + s * np.asarray([(x, y, z) for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.float64)
    quads = np.asarray([(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)], np.int32)      # outward
    return v, reversed_where(sm.sref.triangulate(quads).astype(np.int32), [True] * 12)


def fin_case():
    """Three triangles on the edge 0 - 1: pieces end at the non-manifold edge."""
    v = np.asarray([(10, 10, 10), (14, 10, 10), (12, 14, 10), (12, 6, 10), (12, 10, 14)], np.float64)
    return v, np.asarray([(0, 1, 2), (1, 0, 3), (0, 1, 4)], np.int32)


def rules_case():
    """(a,b,a) - its edge has two sides, both its own: no link -, (a,a,a), a face that is its own piece, an unreferenced NaN vertex; two
    triangles across one link, the second reversed."""
    v = np.asarray([(1, 1, 1), (5, 1, 1.25), (1, 5, 1.5), (5, 5, 2), (3, 9, 1), (9, 9, 9), (np.nan, 0, np.inf), (8, 2, 3), (7, 7, 2), (2, 2, 8),
                    (3, 4, 8)], np.float64)
    return v, np.asarray([(9, 10, 9), (4, 4, 4), (5, 7, 8), (0, 1, 2), (1, 2, 3)], np.int32)


def rules_quad_case():
    """The quad (a,b,a,b) - its edge has four sides - beside two quads across one link."""
    v = np.asarray([(1, 1, 1), (5, 1, 1), (5, 5, 1), (1, 5, 1), (9, 1, 2), (9, 5, 2), (np.nan, 0, 0)], np.float64)
    return v, np.asarray([(0, 1, 0, 1), (0, 1, 2, 3), (1, 2, 5, 4)], np.int32)


@functools.lru_cache(maxsize=None)
def two_spheres_case():
    """The R = 6 shell outward and a copy shifted by 20 cells, inward, with a quarter of its faces reversed."""
    v, f = sm.sphere_case(6, False)
    rev = np.random.default_rng(9).random(f.shape[0]) < 0.25
    g = reversed_where(reversed_where(f + v.shape[0], [True] * f.shape[0]), rev)
    return np.concatenate([v, v + np.asarray([20.0, 0.0, 0.0])]), np.concatenate([f.astype(np.int32), g])


CASES = dict(tet=lambda: tet_case(), tet_one=lambda: tet_case("one"), tet_inward=lambda: tet_case("inward"),
             moebius_q=lambda: moebius_case(True), moebius_t=lambda: moebius_case(False), sheet_checker=sheet_checker_case,
             sheet_q_scr=lambda: scramble("sheet_q")[:2], sphere6_q_scr=lambda: scramble("sphere6_q")[:2],
             sphere6_t_scr=lambda: scramble("sphere6_t")[:2], surface_scr=lambda: scramble("surface")[:2], soup=sm.soup_case,
             tets1000=tets_case, strip3000=strip_case, far_cube_in=far_cube_case, fin=fin_case, rules=rules_case, rules_q=rules_quad_case,
             two_spheres=two_spheres_case)


@functools.lru_cache(maxsize=None)
def reference(name, sign=MAJORITY, min_faces=0, keep_largest=0):
    """orient of a named case, computed once per configuration and shared (read-only) among the tests."""
    return orient(*CASES[name](), sign, min_faces, keep_largest)
