"""Colliding keys for the lattice hash tables (surfacenet_amd/csrc/lattice_table.h; the hand-rolled walks of gtcubes.h and crosscube.h), built from
Python and fed through the stages' ordinary entry points by tests/test_hash_adversary_cpu.py and tests/test_gpu_hash_adversary.py.

The hash is public (lattice.h: lt_mix64, murmur3's finaliser; crosscube.h: cc_hash mixes three multiplies before it). A key whose hash has bits
[w, top) all set starts its walk in the last 2^w slots of EVERY table of 2^c slots, w < c <= top: a set of such keys ("late" keys) is one long
run that walks off slot `mask` on to slot 0, whatever capacity the stage's sizing rule picks. These inputs are legal: every table still holds
at least twice its keys, every walk ends at a free slot.

    mix64, lt_key, cc_hash      the hash, numpy uint64
    late_mask, late_keys        the late candidates
    probe_model                 sequential linear probing: slot, walk length, wrap per key; the keys a planted fault loses
    table_cap                   sn_host.h's capacity rule (only to know which capacity a case WILL meet; the key sets do not depend on it)
    *_case                      one builder per key form: the stage's ordinary arguments plus the key multiset each of its tables receives

A case is a dict: `tables` maps a table's name to dict(keys (uint64, in insertion order: what the model hashes), cap); everything else is the
stage's input. Do not modify a case: they are cached and shared."""
import functools

import numpy as np

import normals_ref as nref

U64 = np.uint64
W, TOP = 4, 16
FAULTS = ("no_wrap", "limit", "lost_race")
LIMIT = 64


# ---- the hash --------------------------------------------------------------------------------------------------------------------------------------
def mix64(keys):
    """lt_mix64 on a uint64 array (wrapping multiplies)."""
    k = np.asarray(keys).astype(U64)
    with np.errstate(over="ignore"):
        k = k ^ (k >> U64(33))
        k = k * U64(0xff51afd7ed558ccd)
        k = k ^ (k >> U64(33))
        k = k * U64(0xc4ceb9fe1a85ec53)
        k = k ^ (k >> U64(33))
    return k


# the four low words tests/host/lattice_check.cpp pins
assert [int(h) & 0xffffffff for h in mix64(np.asarray([0x0000040000400003, 1, 0x0123456789abcdef, 0x7fffffffffffffff], U64))] == \
    [0x21d38bd8, 0x34c2cb2c, 0x89022cea, 0xa930edea]


def lt_key(x, y, z):
    """lattice.h's key of cell (x, y, z), 21 bits per axis."""
    x, y, z = (np.asarray(a).astype(U64) for a in (x, y, z))
    return (x << U64(42)) | (y << U64(21)) | z


def cc_hash(i, j, k):
    """The value crosscube.h's cc_hash hands to lt_mix64 for cube (i, j, k)."""
    i, j, k = (np.asarray(a).astype(U64) for a in (i, j, k))
    with np.errstate(over="ignore"):
        return (i * U64(0x9E3779B97F4A7C15)) ^ ((j + U64(0x632BE59BD9B4E019)) * U64(0xC2B2AE3D27D4EB4F)) ^ (k * U64(0x165667B19E3779F9))


def late_mask(keys, w=W, top=TOP):
    """True where mix64(key) has bits [w, top) all set."""
    bits = U64(((1 << top) - 1) & ~((1 << w) - 1))
    return (mix64(keys) & bits) == bits


def late_keys(candidates, w=W, top=TOP):
    """The candidates that start their walk in the last 2^w slots of every table of 2^c slots, w < c <= top."""
    c = np.asarray(candidates).astype(U64)
    return c[late_mask(c, w, top)]


def table_cap(n, factor, min_cap):
    """sn_host.h: the smallest power of two >= factor * n, at least min_cap."""
    cap = int(min_cap)
    while cap < factor * int(n):
        cap *= 2
    return cap


# ---- the reference model ----------------------------------------------------------------------------------------------------------------------------
def probe_model(keys, cap, fault=None):
    """Sequential linear probing of `keys` (in order; a repeated key finds its slot) into `cap` slots from mix64(key) & (cap - 1).
    -> dict(slot, walk, wrapped: per DISTINCT key in order of first appearance (slot -1: lost); keys: those distinct keys; lost: the keys the
    fault loses; taken: occupied slots). fault: "no_wrap" the walk ends at slot `mask`; "limit" the walk gives up after 64 steps; "lost_race" a key
    that finds its first slot taken by another key is dropped."""
    assert cap & (cap - 1) == 0 and fault in (None,) + FAULTS
    keys = np.asarray(keys).astype(U64)
    _, first = np.unique(keys, return_index=True)
    distinct = keys[np.sort(first)]
    assert fault is not None or 2 * distinct.size <= cap, "a table holds at least twice its keys"
    start = (mix64(distinct) & U64(cap - 1)).astype(np.int64).tolist()
    nxt = list(range(cap + 1))                               # nxt[s]: the first free slot >= s (cap: none), with path compression

    def free_from(s):
        r = s
        while nxt[r] != r:
            r = nxt[r]
        while nxt[s] != r:
            nxt[s], s = r, nxt[s]
        return r
    slot, walk, wrapped, lost = [], [], [], []
    for key, h in zip(distinct.tolist(), start):
        s = free_from(h)
        wrap = s == cap
        if wrap:
            s = free_from(0)
        steps = (s - h) % cap
        gone = (fault == "no_wrap" and wrap) or (fault == "limit" and steps >= LIMIT) or (fault == "lost_race" and steps > 0)
        if gone:
            lost.append(key)
            slot.append(-1)
        else:
            nxt[s] = s + 1
            slot.append(s)
        walk.append(steps)
        wrapped.append(wrap)
    return dict(keys=distinct, slot=np.asarray(slot, np.int64), walk=np.asarray(walk, np.int64), wrapped=np.asarray(wrapped, bool),
                lost=np.asarray(lost, U64), taken=int(distinct.size - len(lost)))


def first_distinct(keys, count):
    """The prefix of `keys` that holds its first `count` distinct keys (all of it when there are fewer)."""
    keys = np.asarray(keys).astype(U64)
    _, first = np.unique(keys, return_index=True)
    first = np.sort(first)
    return keys if first.size <= count else keys[:first[count]]


def _table(keys, n, factor, min_cap):
    keys = np.ascontiguousarray(np.asarray(keys).astype(U64))
    keys.setflags(write=False)
    return dict(keys=keys, cap=table_cap(n, factor, min_cap))


def _freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, (list, tuple)):
        for y in x:
            _freeze(y)
    elif isinstance(x, dict):
        for y in x.values():
            _freeze(y)
    return x


# ---- late cells of a 128^3 block ----------------------------------------------------------------------------------------------------------------------
BLOCK = 128


@functools.lru_cache(maxsize=None)
def late_cells(w=W, top=TOP, lo=0):
    """The cells of [lo, lo + 128)^3 whose lt_key is late, in key order: (L,3) int64."""
    a = np.arange(lo, lo + BLOCK, dtype=np.int64)
    g = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    g = g[late_mask(lt_key(g[:, 0], g[:, 1], g[:, 2]), w, top)]
    g.setflags(write=False)
    return g


def keys_of_cells(g):
    g = np.asarray(g, np.int64).reshape(-1, 3)
    return lt_key(g[:, 0], g[:, 1], g[:, 2])


# Where a case's late keys stand in list order. All late keys share bits [4, 16) of the hash, so at every capacity of 2^5 .. 2^16 slots a key
# starts at slot cap - 16 + (hash & 15). Sixteen keys of one offset (14; 15 or 13 where there are too few) come first: the second of them already walks off slot `mask`, and the k-th
# walks k slots, however few of them a small table takes. The others follow by descending offset: each class loses one key to the free slot
# below the run and sends the rest to the run's end, so the last key of ANY prefix walks nearly the whole run before it.
LEAD_OFFSETS, LEAD = (14, 15, 13), 16


def arrange(keys, n=None):
    """Indices of `n` of the late `keys` (all by default) in the order described above; within a class in the order given."""
    off = (mix64(keys) & U64(15)).astype(np.int64)
    lead = [np.nonzero(off == o)[0][:LEAD] for o in LEAD_OFFSETS]
    lead = [l for l in lead if len(l) == LEAD][0]              # the first of the offsets that sixteen keys share
    rest = np.setdiff1d(np.arange(len(off)), lead)
    rest = rest[np.argsort(-off[rest], kind="stable")]
    out = np.concatenate([lead, rest]).astype(np.int64)
    return out if n is None else out[:n]


@functools.lru_cache(maxsize=None)
def arranged_cells(n=None, lo=0):
    """`n` late cells of [lo, lo + 128)^3 in arrange()'s order."""
    c = late_cells(lo=lo)
    c = c[arrange(keys_of_cells(c), n)]
    c.setflags(write=False)
    return c


# ---- packed world cells: unique voxels, components, the mesher's cell table (bias 4); 4^3 bricks: normals --------------------------------------------
STRIDE = 64                                                     # cubes of 128 cells at stride 64: neighbours overlap by half
CAMERA_SHIFT = np.asarray([7.3, -11.7, 0.0])                    # the mean camera centre off the voxel lattice: no voxel is seen exactly edge-on


def _sheet(count, z=65):
    """`count` cells of a sheet at z, none of them late: the filler of the small cases."""
    out = []
    for x in range(60, 60 + 40):
        for y in range(60, 60 + 16):
            out.append((x, y, z))
    out = np.asarray(out, np.int64)
    out = out[~late_mask(keys_of_cells(out)) & ~late_mask(keys_of_cells(out + 4))][:count]
    assert len(out) == count
    return out


def _shell(R=6, centre=(40, 44, 48)):
    """The shell | |g - centre| - R | < 1 and its radial normals."""
    a = np.arange(-R - 1, R + 2)
    d = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    rad = np.sqrt((d * d).sum(1).astype(np.float64))
    sel = np.abs(rad - R) < 1
    return d[sel] + np.asarray(centre, np.int64), (d[sel] / rad[sel][:, None]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cells_case(total, bias=0):
    """Late cells of the block under lt_key(g + bias) as packed lists (bias 4: the mesher's table). total 32 / 512: `total` voxels in `total`
    distinct cells, all masked - the cell table of 2 * total slots is exactly half full; three quarters of them late, the rest a sheet. Any other
    total: every late cell, every fourth of them listed a second time from the overlapping cube that holds it and a third time from a repeat of
    the first cube (every eighth of these listings unmasked), and a sphere shell of radius 6. Late cells come first in packed order."""
    up = np.asarray([0, 0, 1], np.float32)
    late = arranged_cells(3 * total // 4 if total in (32, 512) else None, bias) - bias
    if total in (32, 512):
        n_late = len(late)
        fill = _sheet(total - n_late)
        cubes, lists = [[0, 0, 0]], [np.concatenate([late, fill])]
        normals = np.tile(up, (total, 1))
        mask = np.ones(total, bool)
    else:
        fill, fill_n = _shell()
        dup = late[::4]
        c2 = np.zeros_like(dup)
        for i, g in enumerate(dup):                              # the first axis along which the overlapping neighbour holds the cell
            ax = np.nonzero(g >= STRIDE)[0]
            if ax.size:
                c2[i, ax[0]] = 1
        second = sorted(set(map(tuple, c2.tolist())))
        cubes = [[0, 0, 0]] + [list(c) for c in second] + [[0, 0, 0]]
        lists = [np.concatenate([late, fill])]
        for c in second:
            m = (c2 == np.asarray(c)).all(1)
            lists.append(dup[m] - np.asarray(c) * STRIDE)
        lists.append(dup)
        n_first = len(lists[0])
        n_dup = sum(len(l) for l in lists[1:])
        normals = np.concatenate([np.tile(up, (len(late), 1)), fill_n, np.tile(-up, (n_dup, 1))])
        mask = np.ones(n_first + n_dup, bool)
        mask[n_first::8] = False
    for l in lists:
        assert l.min() >= 0 and l.max() < BLOCK
    s = nref.hand_scene(cubes, [l.astype(np.uint8) for l in lists], stride_vox=STRIDE)
    s["mask"], s["normals"], s["cameraTs"] = mask, normals, nref.cameras_above(4) + CAMERA_SHIFT
    g = nref.world_cells(s["offsets"], s["ijk"], s["cube_ijk"], STRIDE)
    T = mask.size
    s.update(name="cells%d%s" % (total, "b" if bias else ""), bias=bias, n_late=len(late),
             tables=dict(cell=_table(keys_of_cells(g[mask] + bias), T, 2, 64)))
    return _freeze(s)


@functools.lru_cache(maxsize=None)
def bricks_case():
    """Late 4^3 bricks (normals.h's table: key of g >> 2): three cells in every late brick of [0, 128)^3 bricks, i.e. world cells below 512 in
    cubes of 128 cells at stride 64 - one entry of the cube list per brick, so the bricks keep their order -, plus the shell. Every fourth brick
    has a cell listed again by the overlapping cube."""
    b = arranged_cells()
    inside = np.asarray([(1, 1, 1), (2, 1, 1), (1, 2, 2)], np.int64)
    g = 4 * b[:, None, :] + inside[None, :, :]                 # (L,3,3)
    cube = np.minimum(g[:, 0] // STRIDE, 6)                    # local index 0 .. 127
    cubes, lists = cube.tolist(), [x - c * STRIDE for x, c in zip(g, cube)]
    fill, _ = _shell()
    cubes.append([0, 0, 0])
    lists.append(fill)
    for x, c in zip(g[::4], cube[::4]):                        # the first cell of every fourth brick again, from the neighbour cube below along x
        below = np.asarray([x[0, 0] // STRIDE - 1, c[1], c[2]])
        if below[0] >= 0:
            cubes.append(below.tolist())
            lists.append(x[:1] - below * STRIDE)
    for l in lists:
        assert l.min() >= 0 and l.max() < BLOCK
    s = nref.hand_scene(cubes, [l.astype(np.uint8) for l in lists], stride_vox=STRIDE)
    s["cameraTs"] = nref.cameras_above(4) + CAMERA_SHIFT
    w = nref.world_cells(s["offsets"], s["ijk"], s["cube_ijk"], STRIDE)
    assert np.array_equal(w[:3 * len(b)], g.reshape(-1, 3))
    T = s["mask"].size
    s.update(name="bricks", n_late=len(b), tables=dict(brick=_table(keys_of_cells(w >> 2), T, 2, 64), cell=_table(keys_of_cells(w), T, 2, 64)))
    return _freeze(s)


def without_cells(s, lost):
    """The scene with every voxel whose (biased) cell key is in `lost` unmasked: what a table that lost those keys holds."""
    g = nref.world_cells(s["offsets"], s["ijk"], s["cube_ijk"], s["stride_vox"]) + s.get("bias", 0)
    return dict(s, mask=np.asarray(s["mask"]) & ~np.isin(keys_of_cells(g), lost))


def scene_keys(s):
    """The cell keys an existing packed scene (components_ref / normals_ref) enters, and its table's capacity."""
    g = nref.world_cells(s["offsets"], s["ijk"], s["cube_ijk"], s["stride_vox"])[np.asarray(s["mask"], bool)]
    return _table(keys_of_cells(g), np.asarray(s["mask"]).size, 2, 64)


# ---- the cube map of the cross-cube post-pass ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cubemap_case(n_late=200):
    """`n_late` cubes whose cc_hash is late, then the +x neighbour of each (never late itself), Dc = D_cube = 8: late cube i's voxels
    (5, 1 + j, 1), (5, 2 + j, 1), (6, 2 + j, 2) form one component that coincides with the neighbour's (1, 1 + j, 1); (1, 6, 6) touches nothing.
    The ijk of the middle late cube comes again as the last cube (the map keeps the largest index). Seeded predictions and votes for adapthresh."""
    a = np.arange(1, 1 + BLOCK, dtype=np.int64)
    c = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    late = late_mask(cc_hash(c[:, 0], c[:, 1], c[:, 2]))
    lateset = set(map(tuple, c[late].tolist()))
    pick = np.asarray([t for t in c[late].tolist() if (t[0] + 1, t[1], t[2]) not in lateset and (t[0] - 1, t[1], t[2]) not in lateset], np.int64)
    pick = pick[arrange(cc_hash(pick[:, 0], pick[:, 1], pick[:, 2]), n_late)]
    rs = np.random.RandomState(23)
    rep = n_late // 2
    cubes = pick.tolist() + (pick + [1, 0, 0]).tolist() + [pick[rep].tolist()]
    lists = [np.asarray([(5, 1 + i % 3, 1), (5, 2 + i % 3, 1), (6, 2 + i % 3, 2), (1, 6, 6), (7, 7, 7)], np.uint8) for i in range(n_late)]
    lists += [np.asarray([(1, 1 + i % 3, 1), (1, 2 + i % 3, 1), (0, 6, 6), (7, 7, 7)], np.uint8) for i in range(n_late)]
    lists.append(lists[rep][:3].copy())
    pred = [np.where(np.arange(len(l)) < 2, 0.95, rs.uniform(0.46, 1.0, len(l))).astype(np.float16) for l in lists]
    votes = [np.where(np.arange(len(l)) < 2, 6, np.where(rs.rand(len(l)) < 0.8, 6, 2)).astype(np.uint8) for l in lists]
    d = dict(vxl_ijk_list=lists, prediction_list=pred, rayPooling_votes_list=votes, rgb_list=[np.zeros((len(l), 3), np.uint8) for l in lists],
             cube_ijk_np=np.asarray(cubes, np.uint32))
    masks = [(p >= np.float16(0.7)) & (v >= 4) for p, v in zip(pred, votes)]
    cu = np.asarray(cubes, np.int64)
    return _freeze(dict(name="cubemap", d=d, masks=masks, D_cube=8, Dc=8, repeated=rep, n_late=n_late,
                        tables=dict(map=_table(cc_hash(cu[:, 0], cu[:, 1], cu[:, 2]), len(cubes), 2, 64))))


def without_cubes(c, lost):
    """The denoise masks with every cube whose cc_hash is in `lost` emptied: such a cube is not in the map."""
    cu = np.asarray(c["d"]["cube_ijk_np"], np.int64)
    gone = np.isin(cc_hash(cu[:, 0], cu[:, 1], cu[:, 2]), lost)
    return [np.zeros_like(m) if g else m for m, g in zip(c["masks"], gone)]


# ---- edge keys of smooth, fill and orient ------------------------------------------------------------------------------------------------------------------
INDEX_BITS = 28


def edge_keys(faces):
    """The keys (lo << 28) | hi of the faces' sides in (face, side) order, sides with equal ends left out: what the edge table's build inserts."""
    f = np.asarray(faces, np.int64)
    s = np.stack([f, np.roll(f, -1, axis=1)], axis=2).reshape(-1, 2)
    s = s[s[:, 0] != s[:, 1]]
    return (s.min(axis=1).astype(U64) << U64(INDEX_BITS)) | s.max(axis=1).astype(U64)


@functools.lru_cache(maxsize=None)
def late_pairs(V=2048):
    """The vertex pairs lo < hi < V whose edge key is late, in key order: (L,2) int64."""
    lo, hi = np.nonzero(np.triu(np.ones((V, V), bool), 1))
    m = late_mask((lo.astype(U64) << U64(INDEX_BITS)) | hi.astype(U64))
    return np.stack([lo[m], hi[m]], 1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def edges_case(nv, V=2048):
    """A mesh of V vertices on distinct lattice points whose late vertex pairs are sides of triangles (nv 3) or quads (nv 4): pair i = (lo, hi)
    carries the face (lo, hi, free ...), and, unless i % 4 == 1 (a boundary side), the face (hi, lo, free ...) against it; with i % 4 == 3 a
    third face as well (a non-manifold side). The late sides come first in face order; a shared side is inserted two or three times."""
    i = np.arange(V, dtype=np.int64)
    verts = np.stack([i % 16, (i // 16) % 16, i // 256], 1).astype(np.float64) * 2.0 + 3.0 + 0.125 * ((i[:, None] * np.asarray([3, 5, 7])) % 5)
    pairs = late_pairs(V)
    pairs = pairs[arrange((pairs[:, 0].astype(U64) << U64(INDEX_BITS)) | pairs[:, 1].astype(U64))]

    def free(lo, hi, salt, taken=()):
        t = (lo * 7 + hi * 13 + salt) % V
        while t in (lo, hi) + tuple(taken):
            t = (t + 1) % V
        return int(t)
    first, rest = [], []
    for n, (lo, hi) in enumerate(pairs.tolist()):
        a = free(lo, hi, 1)
        b = free(lo, hi, 2, (a,))
        first.append([lo, hi, a] + ([b] if nv == 4 else []))
        if n % 4 != 1:
            c = free(lo, hi, 3)
            d = free(lo, hi, 4, (c,))
            rest.append([hi, lo, c] + ([d] if nv == 4 else []))
        if n % 4 == 3:
            e = free(lo, hi, 5)
            g = free(lo, hi, 6, (e,))
            rest.append([lo, hi, e] + ([g] if nv == 4 else []))
    faces = np.asarray(first + rest, np.int32)
    return _freeze(dict(name="edges%d" % nv, verts=verts, faces=faces, nv=nv, n_late=len(pairs), pairs=pairs,
                        tables=dict(edge=_table(edge_keys(faces), nv * faces.shape[0], 2, 64))))


def without_edges(faces, lost):
    """The faces none of whose sides is in `lost`."""
    f = np.asarray(faces, np.int64)
    a, b = f, np.roll(f, -1, axis=1)
    key = (np.minimum(a, b).astype(U64) << U64(INDEX_BITS)) | np.maximum(a, b).astype(U64)
    return np.asarray(faces)[~np.isin(key, lost).any(axis=1)]


def mesh_edge_table(faces):
    """The edge table an existing mesh case enters."""
    f = np.asarray(faces)
    return _table(edge_keys(f), f.shape[1] * f.shape[0], 2, 64)


# ---- the simplifier's cluster cells and face keys -----------------------------------------------------------------------------------------------------------
SIMPLIFY_CELL = 2


def simplify_cells(verts, cell=SIMPLIFY_CELL):
    """c = (rint(256 v) + 1024) // (256 cell): the cluster cell of a vertex (meshsimplify_ref's expression)."""
    q = np.rint(np.asarray(verts, np.float64) * 256.0).astype(np.int64)
    return np.floor_divide(q + 1024, 256 * int(cell))


def _rot_key(t):
    t = np.asarray(t, np.int64).reshape(-1, 3)
    r = np.take_along_axis(t, (np.argmin(t, axis=1)[:, None] + np.arange(3)) % 3, axis=1)
    return lt_key(r[:, 0], r[:, 1], r[:, 2])


@functools.lru_cache(maxsize=None)
def simplify_case(n_faces=512):
    """Vertex k < P at the centre of late cell k (arrange()'s order; cluster k = vertex k once every vertex is referenced); every fourth cluster has
    a second member, vertex P + k / 4, a quarter of a lattice cell away. Faces: `n_faces` triples of clusters whose lt_key(r0, r1, r2), smallest
    first, is late; every fourth of them again, rotated and through the second members where there are any (the same face key: a duplicate);
    a face per second member that collapses (two corners in one cluster); a plain face for every vertex no late face names."""
    cell = SIMPLIFY_CELL
    c = arranged_cells()
    P = len(c)
    v0 = c.astype(np.float64) * cell + cell / 2.0 - 4.0
    second = np.arange(0, P, 4)
    verts = np.concatenate([v0, v0[second] + np.asarray([0.25, 0.0, -0.25])])
    member2 = np.full(P, -1, np.int64)
    member2[second] = P + np.arange(len(second))
    found = []
    r2 = np.arange(P, dtype=np.int64)
    for r0 in range(P - 2):
        r1 = np.arange(r0 + 1, min(P, r0 + 65), dtype=np.int64)
        a, b = np.meshgrid(r1, r2[r0 + 1:], indexing="ij")
        a, b = a.reshape(-1), b.reshape(-1)
        ok = (a != b) & late_mask(lt_key(np.full_like(a, r0), a, b))
        found += [(r0, int(x), int(y)) for x, y in zip(a[ok], b[ok])]
    seen, late = np.zeros(P, bool), []
    for t in found:                                              # first the faces that name a cluster nobody has named
        if not seen[list(t)].all():
            late.append(t)
            seen[list(t)] = True
    chosen = set(late)
    late = (late + [t for t in found if t not in chosen])[:n_faces]
    assert len(late) == n_faces
    late = [late[i] for i in arrange(_rot_key(late))]
    seen[:] = False
    seen[np.asarray(late).reshape(-1)] = True
    plain = [(k, (k + 1) % P, (k + 2) % P) for k in np.nonzero(~seen)[0].tolist()]
    m = lambda k: int(member2[k]) if member2[k] >= 0 else int(k)
    again = [(m(t[1]), m(t[2]), m(t[0])) for t in late[::4]]
    collapsed = [(int(k), int(member2[k]), int((k + 1) % P)) for k in second.tolist()]
    faces = np.asarray(late + plain + again + collapsed, np.int32)
    cluster = np.concatenate([np.arange(P), second])            # of every vertex
    t = cluster[faces]
    alive = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    V, F = verts.shape[0], faces.shape[0]
    referenced = np.zeros(V, bool)
    referenced[faces.reshape(-1)] = True
    assert referenced[:P].all()
    cc = np.concatenate([c, c[second]])
    return _freeze(dict(name="simplify", verts=verts, faces=faces, cell=cell, cells=cc, n_late=P, n_late_faces=n_faces,
                        tables=dict(vertex=_table(keys_of_cells(cc[referenced]), V, 2, 64), face=_table(_rot_key(t[alive]), F, 2, 64))))


# ---- the cell grid: point reduction, nearest neighbours (its query grid), ground-truth cubes ---------------------------------------------------------------
PE_COARSE = 8


def _grid_points(h, per_cell, dtype=np.float64):
    """Points at the centres of the late cells of a grid of origin 0 and cell size h: the min-corner point (0, 0, 0) and the max-corner point, the
    centre of cell (127, 127, 127), fix the origin and the extent. per_cell 3: two more points a quarter of a cell either side along x."""
    c = arranged_cells()
    corner = np.asarray([[0, 0, 0], [BLOCK - 1] * 3], np.int64)
    cells = np.concatenate([c] * per_cell + [corner])
    off = np.zeros((len(cells), 3))
    off[-2] = -0.5                                               # the min corner itself
    if per_cell == 3:
        off[len(c):2 * len(c), 0], off[2 * len(c):3 * len(c), 0] = 0.25, -0.25
    p = ((cells + 0.5 + off) * h).astype(dtype)
    return p, cells


@functools.lru_cache(maxsize=None)
def reduce_case(per_cell=1, dst=0.75):
    """sn_point_reduce's grid has cells of dst (1 + 1e-6) from the cloud's min corner. Three points per cell lie within dst of each other."""
    h = dst * (1.0 + 1e-6)
    p, cells = _grid_points(h, per_cell)
    n = len(p)
    order = np.random.RandomState(31).permutation(n)
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    return _freeze(dict(name="reduce%d" % per_cell, xyz=p, cells=cells, h=h, dst=dst, order=order, rank=rank, n_late=len(late_cells()),
                        tables=dict(grid=_table(keys_of_cells(cells), n, 2, 1024))))


def nn_query_cell(to):
    """The cell size of sn_nn_dist2's query grid as its host code derives it from the `to` cloud: the first bucketing at the mean spacing h0
    counts the occupied cells, the fine size scales h0 towards six points per cell, the coarse and the query grids have eight times that."""
    to = np.asarray(to, np.float64)
    lo, hi = to.min(0), to.max(0)
    E = float((hi - lo).max())
    vol = 1.0
    for d in range(3):
        vol *= (hi[d] - lo[d]) + E / 64.0
    h0 = float(np.cbrt(vol / to.shape[0]))
    occ = np.unique(np.floor((to - lo) / h0), axis=0).shape[0]
    m0 = to.shape[0] / max(occ, 1)
    h = h0 * np.sqrt(6.0 / m0) if m0 > 6.0 else h0 * np.cbrt(6.0 / m0)
    return PE_COARSE * float(h), occ


@functools.lru_cache(maxsize=None)
def nn_case():
    """sn_nn_dist2 sizes the grids of the `to` cloud from that cloud's own density, so a few thousand points cannot spread over 128^3 of its cells;
    the grid of the QUERIES has the coarse cell size and the queries' own min corner, and they are free: `to` is an 8^3 lattice in the middle of the
    block, the queries sit at the centres of the late cells of their grid (and on top of a few `to` points)."""
    a = np.arange(8, dtype=np.float64)
    to = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    hq, occ = nn_query_cell(to)
    assert occ == 512
    to = to + 64.0 * hq
    frm, cells = _grid_points(hq, 1)
    near = to[::26] + np.asarray([0.25, -0.125, 0.5])          # twenty queries beside `to` points, before the two corner points
    frm = np.concatenate([frm[:-2], near, frm[-2:]])
    cells = np.concatenate([cells[:-2], np.floor(near / hq).astype(np.int64), cells[-2:]])
    return _freeze(dict(name="nn", to=to, frm=frm, cells=cells, h=hq, n_late=len(late_cells()),
                        tables=dict(query=_table(keys_of_cells(cells), len(frm), 2, 1024))))


@functools.lru_cache(maxsize=None)
def gt_case(s=8):
    """Ground-truth cubes over a float32 cloud bound with cell 1.0: three points in every late cell (exact in float32). A cube of 8 voxels of 0.4
    around every fourth late cell, shifted by a few voxels: its candidate box holds at most 6^3 cells, fewer than there are points, so the
    kernel walks the table itself (gtcubes.h's branch nc <= n)."""
    pts, cells = _grid_points(1.0, 3, np.float32)
    c = arranged_cells()[::4].astype(np.float64)
    shift = (np.arange(len(c))[:, None] * np.asarray([1, 3, 5]) % 7) * 0.4
    xyz = (c + 0.5 - 2.8 + shift).astype(np.float32)
    resol = np.full(len(xyz), 0.4, np.float32)
    return _freeze(dict(name="gt", pts=pts, cells=cells, cell=1.0, xyz=xyz, resol=resol, s=s, n_late=len(late_cells()),
                        tables=dict(grid=_table(keys_of_cells(cells), len(pts), 2, 1024))))


# ---- quantizePts2Cubes, the hash-set form ---------------------------------------------------------------------------------------------------------------------
PT_ARGS = dict(resol=np.float32(0.4), cube_D=32, cube_Dcenter=26, cube_overlapping_ratio=0.5)
PT_TOP = 1023                                                   # the max-corner point's cell: 1025^3 cells, more than the bitmap form takes (2^27)


@functools.lru_cache(maxsize=None)
def ptcubes_case(dtype="float64"):
    """Points in the middle of the late floor cells q of the block (the diagonal cell q + 1 is whatever it is), the min-corner point (the shift)
    and a max-corner point in cell 1023 on every axis."""
    stride = float(PT_ARGS["resol"] * PT_ARGS["cube_Dcenter"] * PT_ARGS["cube_overlapping_ratio"])
    q = np.concatenate([arranged_cells(), [[0, 0, 0], [PT_TOP] * 3]])
    off = np.full((len(q), 1), 0.5)
    off[-2] = 0.0
    pts = ((q + off) * stride).astype(dtype)
    keys = np.stack([keys_of_cells(q), keys_of_cells(q + 1)], 1).reshape(-1)
    return _freeze(dict(name="ptcubes_" + dtype, pts=pts, cells=q, n_late=len(late_cells()), tables=dict(set=_table(keys, len(pts), 4, 2048))))


# ---- every case, by the name the tests print ------------------------------------------------------------------------------------------------------------------
BUILDERS = {
    "cells32": lambda: cells_case(32), "cells512": lambda: cells_case(512), "cells1500": lambda: cells_case(1500),
    "cells32b": lambda: cells_case(32, 4), "cells512b": lambda: cells_case(512, 4), "cells1500b": lambda: cells_case(1500, 4),
    "bricks": bricks_case, "cubemap": cubemap_case, "edges3": lambda: edges_case(3), "edges4": lambda: edges_case(4),
    "simplify": simplify_case, "reduce1": lambda: reduce_case(1), "reduce3": lambda: reduce_case(3), "nn": nn_case, "gt": gt_case,
    "ptcubes_f64": lambda: ptcubes_case("float64"), "ptcubes_f32": lambda: ptcubes_case("float32"),
}
# the table of each case that the late keys fill (the other tables of a case are along for the ride)
ADVERSARIAL = {"cells32": "cell", "cells512": "cell", "cells1500": "cell", "cells32b": "cell", "cells512b": "cell", "cells1500b": "cell",
               "bricks": "brick", "cubemap": "map", "edges3": "edge", "edges4": "edge", "simplify": ("vertex", "face"), "reduce1": "grid",
               "reduce3": "grid", "nn": "query", "gt": "grid", "ptcubes_f64": "set", "ptcubes_f32": "set"}
HALF_FULL = ("cells32", "cells512", "cells32b", "cells512b")


def tables_of(name):
    """[(table name, table)] of the case's adversarial tables."""
    t = ADVERSARIAL[name]
    case = BUILDERS[name]()
    return [(k, case["tables"][k]) for k in ((t,) if isinstance(t, str) else t)]
