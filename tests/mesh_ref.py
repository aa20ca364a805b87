"""CPU restatement of the surface-nets mesher, independent of the device code: dense int64 grids of the field F and the
weight W over the bounding box of the oriented cells, boolean grids for the edges, np.lexsort for the canonical order. It is the checker of
tests/test_mesh_cpu.py and tests/test_gpu_mesh.py; the scenes come from tests/normals_ref.py plus the sphere shell below."""
import functools
import itertools

import numpy as np

import normals_ref as nref

QSCALE = 16384
BIAS = 4                                                        # one brick: samples down to -4 keep non-negative keys
AXIS_MAX = 1 << 21


def quantise(normals):
    """nq = int(rint(float64(n) * 16384)), ties to even."""
    return np.rint(np.asarray(normals, np.float32).astype(np.float64) * float(QSCALE)).astype(np.int64)


def oriented_cells(offsets, ijk, cube_ijk, mask, stride_vox, normals):
    """-> (cells (M,3) int64, owner (M,) int64 packed indices, nq (M,3) int64): the world cells whose owner - the smallest packed index among
    the cell's masked voxels - has a normal with a non-zero component."""
    mask = np.asarray(mask, bool).reshape(-1)
    normals = np.asarray(normals, np.float32).reshape(-1, 3)
    idx = np.nonzero(mask)[0]
    if idx.size == 0:
        return np.zeros((0, 3), np.int64), np.zeros((0,), np.int64), np.zeros((0, 3), np.int64)
    bad = ~np.isfinite(normals[idx]) | (np.abs(normals[idx]) > 2)
    if bad.any():
        raise ValueError("a masked voxel's normal is not finite or exceeds 2 in magnitude")
    g = nref.world_cells(offsets, ijk, cube_ijk, stride_vox)[idx]
    if (g + 8 >= AXIS_MAX).any():
        raise ValueError("a masked voxel's world cell plus 8 reaches 2^21")
    _, first = np.unique(g, axis=0, return_index=True)          # idx ascending: the first occurrence is the smallest packed index
    owner = idx[first]
    cells = g[first]
    keep = (normals[owner] != 0).any(axis=1)
    return cells[keep], owner[keep].astype(np.int64), quantise(normals[owner[keep]])


def _order_key(p):
    """Columns for np.lexsort, least significant first, of biased lattice points p (K,3): ascending (brick x, brick y, brick z, local)."""
    q = p + BIAS
    local = (q[:, 0] & 3) * 16 + (q[:, 1] & 3) * 4 + (q[:, 2] & 3)
    return [local, q[:, 2] >> 2, q[:, 1] >> 2, q[:, 0] >> 2]


def mesh_ref(offsets, ijk, cube_ijk, mask, stride_vox, normals, radius=2, reach=0, origin=(0.0, 0.0, 0.0), resol=1.0):
    """-> dict(quads (Q,4) int32, vert_cell (V,3) int32, vert_lattice (V,3) float64, verts_mm (V,3) float32, vert_src (V,) int64, n_cells)."""
    r, reach = int(radius), int(reach)
    if not 1 <= r <= 3 or not 0 <= reach <= r or int(stride_vox) < 1:
        raise ValueError("radius in 1..3, reach in 0..radius, stride_vox >= 1")
    cells, owner, nq = oriented_cells(offsets, ijk, cube_ijk, mask, stride_vox, normals)
    empty = dict(quads=np.zeros((0, 4), np.int32), vert_cell=np.zeros((0, 3), np.int32), vert_lattice=np.zeros((0, 3), np.float64),
                 verts_mm=np.zeros((0, 3), np.float32), vert_src=np.zeros((0,), np.int64), n_cells=int(cells.shape[0]))
    if cells.shape[0] == 0:
        return empty
    pad = r + 3
    lo = cells.min(0) - pad
    dims = tuple(int(v) for v in (cells.max(0) - cells.min(0) + 2 * pad + 1))
    p = cells - lo
    F = np.zeros(dims, np.int64)
    W = np.zeros(dims, np.int64)
    own = np.full(dims, -1, np.int64)
    own[p[:, 0], p[:, 1], p[:, 2]] = owner
    for d in itertools.product(range(-r, r + 1), repeat=3):
        w = (r + 1 - abs(d[0])) * (r + 1 - abs(d[1])) * (r + 1 - abs(d[2]))
        c = p + np.asarray(d)                                   # the cells are distinct: so are the samples of one offset
        F[c[:, 0], c[:, 1], c[:, 2]] += w * (nq[:, 0] * d[0] + nq[:, 1] * d[1] + nq[:, 2] * d[2])
        W[c[:, 0], c[:, 1], c[:, 2]] += w
    defined, inside, inP = W > 0, F < 0, own >= 0
    near = inP.copy()
    for _ in range(reach):                                      # Chebyshev dilation by one cell (the border is `pad` cells of nothing)
        for ax in range(3):
            m = near.copy()
            sl_a, sl_b = [slice(None)] * 3, [slice(None)] * 3
            sl_a[ax], sl_b[ax] = slice(1, None), slice(None, -1)
            m[tuple(sl_a)] |= near[tuple(sl_b)]
            m[tuple(sl_b)] |= near[tuple(sl_a)]
            near = m

    def shifted(A, ax):                                         # A at c + e_ax (False / 0 past the end)
        out = np.zeros_like(A)
        sl_a, sl_b = [slice(None)] * 3, [slice(None)] * 3
        sl_a[ax], sl_b[ax] = slice(None, -1), slice(1, None)
        out[tuple(sl_a)] = A[tuple(sl_b)]
        return out

    active = [defined & shifted(defined, a) & (inside != shifted(inside, a)) for a in range(3)]
    emit = [active[a] & (near | shifted(near, a)) for a in range(3)]
    ec = [np.argwhere(emit[a]) for a in range(3)]
    c_all = np.concatenate(ec)
    a_all = np.concatenate([np.full(len(ec[a]), a, np.int64) for a in range(3)])
    if c_all.shape[0] == 0:
        return empty
    order = np.lexsort([a_all] + _order_key(c_all + lo))
    c_all, a_all = c_all[order], a_all[order]
    Q = c_all.shape[0]
    corners = np.zeros((Q, 4, 3), np.int64)
    eye = np.eye(3, dtype=np.int64)
    for k, (u, v) in enumerate([(1, 1), (0, 1), (0, 0), (1, 0)]):
        corners[:, k] = c_all - u * eye[(a_all + 1) % 3] - v * eye[(a_all + 2) % 3]
    c_inside = inside[c_all[:, 0], c_all[:, 1], c_all[:, 2]]
    corners[~c_inside] = corners[~c_inside][:, ::-1]            # c + e_a is the inside end: reversed
    m_all, inv = np.unique(corners.reshape(-1, 3), axis=0, return_inverse=True)
    vorder = np.lexsort(_order_key(m_all + lo))
    pos = np.empty(vorder.size, np.int64)
    pos[vorder] = np.arange(vorder.size)
    quads = pos[np.asarray(inv).reshape(-1)].reshape(Q, 4).astype(np.int32)
    m = m_all[vorder]
    V = m.shape[0]
    # positions: the 12 edges in the contract's order, every active one counted
    s = np.zeros((V, 3), np.float64)
    cnt = np.zeros((V,), np.int64)
    for a in range(3):
        o0, o1 = [x for x in range(3) if x != a]
        for u, v in [(0, 0), (0, 1), (1, 0), (1, 1)]:
            off = np.zeros(3, np.int64)
            off[o0], off[o1] = u, v
            c = m + off
            c1 = c + eye[a]
            act = active[a][c[:, 0], c[:, 1], c[:, 2]]
            F0 = F[c[:, 0], c[:, 1], c[:, 2]].astype(np.float64)
            F1 = F[c1[:, 0], c1[:, 1], c1[:, 2]].astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                t = F0 / (F0 - F1)
            pt = np.tile(off.astype(np.float64), (V, 1))
            pt[:, a] = t
            s[act] = s[act] + pt[act]
            cnt += act
    assert (cnt > 0).all()
    offset = s / cnt[:, None].astype(np.float64)
    vert_cell = m + lo
    vert_lattice = vert_cell.astype(np.float64) + offset
    verts_mm = (np.asarray(origin, np.float64).reshape(3) + float(resol) * vert_lattice).astype(np.float32)
    # vert_src: the nearest oriented cell of m + {-1,0,1,2}^3 to the dual cube's centre, ties to the smallest (x,y,z)
    best = np.full((V,), 1 << 30, np.int64)
    src = np.full((V,), -1, np.int64)
    for d in itertools.product(range(-1, 3), repeat=3):
        c = m + np.asarray(d)
        o = own[c[:, 0], c[:, 1], c[:, 2]]
        dist = sum((2 * x - 1) ** 2 for x in d)
        better = (o >= 0) & (dist < best)
        best[better], src[better] = dist, o[better]
    return dict(quads=quads, vert_cell=vert_cell.astype(np.int32), vert_lattice=vert_lattice, verts_mm=verts_mm, vert_src=src,
                n_cells=int(cells.shape[0]))


# ---- mesh properties -----------------------------------------------------------------------------------------------------------------------------
def edge_counts(quads):
    """-> (undirected edges (E,2), number of quads on each)."""
    q = np.asarray(quads, np.int64)
    e = np.stack([q, np.roll(q, -1, axis=1)], axis=2).reshape(-1, 2)
    return np.unique(np.sort(e, axis=1), axis=0, return_counts=True)


def signed_volume(verts, quads):
    """Of the triangulation (0,1,2), (0,2,3): positive when the faces' normals point outward."""
    v = np.asarray(verts, np.float64)
    q = np.asarray(quads, np.int64)
    tri = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]])
    a, b, c = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def quad_normals(verts, quads):
    v = np.asarray(verts, np.float64)
    q = np.asarray(quads, np.int64)
    return np.cross(v[q[:, 2]] - v[q[:, 0]], v[q[:, 3]] - v[q[:, 1]])


def parse_ply(path):
    """A binary little-endian PLY of float / uchar vertex properties and one face list -> (header lines, vertex records, list of faces)."""
    blob = open(path, "rb").read()
    cut = blob.index(b"end_header\n") + 11
    header = blob[:cut].decode("ascii").splitlines()
    nv = int([h for h in header if h.startswith("element vertex")][0].split()[-1])
    nf = int([h for h in header if h.startswith("element face")][0].split()[-1])
    props = [h.split()[1:] for h in header if h.startswith("property") and "list" not in h]
    dt = np.dtype([(name, {"float": "<f4", "uchar": "u1"}[typ]) for typ, name in props])
    verts = np.frombuffer(blob[cut:cut + nv * dt.itemsize], dtype=dt)
    faces, pos = [], cut + nv * dt.itemsize
    for _ in range(nf):
        k = blob[pos]
        faces.append(np.frombuffer(blob[pos + 1:pos + 1 + 4 * k], dtype="<i4"))
        pos += 1 + 4 * k
    assert pos == len(blob)
    return header, verts, faces


# ---- scenes --------------------------------------------------------------------------------------------------------------------------------------
def one_cube_scene(cells, normals, cube_ijk=(0, 0, 0), stride_vox=13):
    """Packed lists of one cube whose voxels are `cells` (local, < 256), all masked."""
    ijk = np.asarray(cells, np.uint8).reshape(-1, 3)
    return dict(offsets=np.asarray([0, ijk.shape[0]], np.int64), ijk=ijk, cube_ijk=np.asarray([cube_ijk], np.int64), mask=np.ones(ijk.shape[0], bool),
                stride_vox=stride_vox, normals=np.asarray(normals, np.float32).reshape(-1, 3))


def sheet_scene(z=7):
    ijk = nref.sheet_5x5(z)[0]
    return one_cube_scene(ijk, np.tile(np.asarray([0, 0, 1], np.float32), (ijk.shape[0], 1)))


def tilted_scene():
    """normals_ref.tilted_sheet_two_cubes with the plane's normal (1,0,1)/sqrt(2) on every voxel."""
    cube_ijk, lists = nref.tilted_sheet_two_cubes()
    offsets, ijk = nref.pack(lists)
    n = np.tile((np.asarray([1.0, 0.0, 1.0]) / np.sqrt(2.0)).astype(np.float32), (ijk.shape[0], 1))
    return dict(offsets=offsets, ijk=ijk, cube_ijk=np.asarray(cube_ijk, np.int64), mask=np.ones(ijk.shape[0], bool), stride_vox=13, normals=n)


@functools.lru_cache(maxsize=None)
def sphere_scene(R=6, centre=20, cube_shift=(0, 0, 0), stride_vox=13, split=False):
    """The shell | |g - centre| - R | < 1 of a 40^3 block with analytic radial normals rounded to float32. split: every cell goes to cube
    g // stride_vox (the last cube takes the rest), so the shell straddles cube boundaries; otherwise one cube at cube_shift holds it all.
    Do not modify the result."""
    g = np.asarray(list(itertools.product(range(40), repeat=3)), np.int64)
    d = (g - centre).astype(np.float64)
    rad = np.sqrt((d * d).sum(1))
    sel = np.abs(rad - R) < 1
    g, n = g[sel], (d[sel] / rad[sel][:, None]).astype(np.float32)
    if not split:
        s = one_cube_scene(g, n, cube_shift, stride_vox)
        return s
    cube = np.minimum(g // stride_vox, (40 - 1) // stride_vox)
    local = g - cube * stride_vox
    keys, inv = np.unique(cube, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    order = np.argsort(inv, kind="stable")
    counts = np.bincount(inv, minlength=len(keys))
    offsets = np.zeros(len(keys) + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    return dict(offsets=offsets, ijk=local[order].astype(np.uint8), cube_ijk=keys + np.asarray(cube_shift, np.int64), mask=np.ones(g.shape[0], bool),
                stride_vox=stride_vox, normals=n[order])


@functools.lru_cache(maxsize=None)
def surface_normals(lattice=(2, 2, 1), radius=2):
    """The float32 normals normals_ref computes for surface_scene(lattice): the mesher's input in the surface tests. Do not modify."""
    return nref.surface_reference(tuple(lattice), radius=radius)["normals"]


def surface_mesh_scene(lattice=(2, 2, 1)):
    s = nref.surface_scene(tuple(lattice))
    return dict(offsets=s["offsets"], ijk=s["ijk"], cube_ijk=s["cube_ijk"], mask=s["mask"], stride_vox=s["stride_vox"], normals=surface_normals(tuple(lattice)))


def scene_args(s):
    return (s["offsets"], s["ijk"], s["cube_ijk"], s["mask"], s["stride_vox"], s["normals"])


@functools.lru_cache(maxsize=None)
def surface_mesh_reference(lattice=(2, 2, 1), radius=2, reach=0):
    """mesh_ref of surface_mesh_scene, computed once per configuration and shared (read-only) among the tests."""
    return mesh_ref(*scene_args(surface_mesh_scene(lattice)), radius=radius, reach=reach, origin=(-20.0, -20.0, -20.0), resol=0.4)
