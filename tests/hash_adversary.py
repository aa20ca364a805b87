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
    late_at, TARGETED           key forms with too few candidates for that (ray pooling's pixels and cells, the mesher's bricks) are late at the ONE
                                capacity their stage's sizing rule - restated here, pinned to the headers by the CPU test - gives them; the
                                self-intersection grid's cells are late everywhere and stand with them

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


def late_at(candidates, cap, w=W):
    """The candidates that start their walk in the last 2^w slots of a table of `cap` slots (bits [w, log2 cap) of the hash all set): late at
    THAT capacity, whatever they do at another. A key form with too few candidates for late_keys has enough of these."""
    assert cap & (cap - 1) == 0 and cap > 1 << w
    c = np.asarray(candidates).astype(U64)
    return c[late_mask(c, w, cap.bit_length() - 1)]


def table_cap(n, factor, min_cap):
    """sn_host.h: the smallest power of two >= factor * n, at least min_cap."""
    cap = int(min_cap)
    while cap < factor * int(n):
        cap *= 2
    return cap


# The sizing rules of the stages whose cases are late at ONE capacity, restated once (tests/test_hash_adversary_cpu.py reads the constants out of
# postpass.h and meshintersect.h and holds every such case to the rule: a targeted case is adversarial only while the rule here is the kernel's).
RP_LIST, RP_LDS_M, RP_LDS_CAP, MXI_BIG = 8192, 3400, 4096, 64
LDS_FILL = (5, 6)                                               # RP_LDS_M selected voxels in RP_LDS_CAP slots: 83 %, at most 5/6


def ray_pool_rule(m):
    """ray_pool_kernel's tables for m selected voxels of a (cube, view) -> dict(cap, lds, listed): the smallest power of two >= 2 m, at least
    64; m <= RP_LDS_M caps it at RP_LDS_CAP and puts the tables into LDS; the voxels are listed iff m <= RP_LIST."""
    cap = table_cap(m, 2, 64)
    lds = m <= RP_LDS_M
    return dict(cap=min(cap, RP_LDS_CAP) if lds else cap, lds=lds, listed=m <= RP_LIST)


def brick_cap(total):
    """The mesher's brick table has the cell table's own mask: table_cap(total, 2, 64) for `total` packed voxels."""
    return table_cap(total, 2, 64)


def intersect_cap(n_tris, budget=8):
    """The intersection grid's cell table: twice the entries a level may have, max(budget, 8) per triangle, at least 1,024 slots."""
    return table_cap(max(budget, 8) * int(n_tris), 2, 1024)


# ---- the reference model ----------------------------------------------------------------------------------------------------------------------------
def probe_model(keys, cap, fault=None, fill=(1, 2)):
    """Sequential linear probing of `keys` (in order; a repeated key finds its slot) into `cap` slots from mix64(key) & (cap - 1).
    -> dict(slot, walk, wrapped: per DISTINCT key in order of first appearance (slot -1: lost); keys: those distinct keys; lost: the keys the
    fault loses; taken: occupied slots). fault: "no_wrap" the walk ends at slot `mask`; "limit" the walk gives up after 64 steps; "lost_race" a key
    that finds its first slot taken by another key is dropped. fill: the fullest the table may be, (1, 2) half; ray pooling's LDS tables: LDS_FILL."""
    assert cap & (cap - 1) == 0 and fault in (None,) + FAULTS
    keys = np.asarray(keys).astype(U64)
    _, first = np.unique(keys, return_index=True)
    distinct = keys[np.sort(first)]
    assert fault is not None or fill[1] * distinct.size <= fill[0] * cap, "a table holds at least twice its keys (LDS tables: 6/5 of them)"
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


# ---- the mesher's brick table: late at the capacity the stage gives it -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bricks_mesh_case(total=512, bias=4):
    """cells512b's shape for the mesher's brick table (mesh.h: key of (g + 4) >> 2): `total` masked voxels with normals in `total` distinct
    cells of one cube, so the cell table and the brick table get 2 * total slots. Three quarters of them sit one per brick, at local cell
    (1, 2, 3) - (k % 2, 0, 0), in the bricks of [1, 33)^3 whose key is late AT THAT CAPACITY (the block has 32,768 bricks: a few hundred of those, a
    handful late at every capacity), in arrange()'s order; the rest are the sheet, whose bricks are not late."""
    cap = brick_cap(total)
    a = np.arange(1, 1 + BLOCK // 4, dtype=np.int64)
    b = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    bkeys = keys_of_cells(b)
    b = b[np.isin(bkeys, late_at(bkeys, cap))]
    b = b[arrange(keys_of_cells(b), 3 * total // 4)]
    assert len(b) == 3 * total // 4
    late = 4 * b + np.asarray([1, 2, 3]) - (np.arange(len(b)) % 2)[:, None] * np.asarray([1, 0, 0]) - bias      # world cells
    sheet = np.asarray([(x, y, 65) for x in range(60, 100) for y in range(60, 76)], np.int64)
    sheet = sheet[~late_mask(keys_of_cells((sheet + bias) >> 2), W, cap.bit_length() - 1)][:total - len(late)]
    cells = np.concatenate([late, sheet])
    assert len(cells) == total and np.unique(cells, axis=0).shape[0] == total and cells.min() >= 0 and cells.max() < BLOCK
    s = nref.hand_scene([[0, 0, 0]], [cells.astype(np.uint8)], stride_vox=STRIDE)
    s["mask"], s["normals"], s["cameraTs"] = np.ones(total, bool), np.tile(np.asarray([0, 0, 1], np.float32), (total, 1)), nref.cameras_above(4) + CAMERA_SHIFT
    g = nref.world_cells(s["offsets"], s["ijk"], s["cube_ijk"], STRIDE) + bias
    s.update(name="bricks_mesh", bias=bias, n_late=len(late), rule_n=total,
             tables=dict(brick=_table(keys_of_cells(g >> 2), total, 2, 64), cell=_table(keys_of_cells(g), total, 2, 64)))
    return _freeze(s)


def without_bricks(s, lost):
    """The scene with every voxel whose (biased) brick key is in `lost` unmasked: what a brick table that lost those keys holds."""
    g = nref.world_cells(s["offsets"], s["ijk"], s["cube_ijk"], s["stride_vox"]) + s["bias"]
    return dict(s, mask=np.asarray(s["mask"]) & ~np.isin(keys_of_cells(g >> 2), lost))


# ---- the self-intersection grid ----------------------------------------------------------------------------------------------------------------------------
MXI_OFFSET = 4                                                  # meshintersect_rules.h: grid cell at level 0 = floor(v) + 4
# a grid cell's contents, in sixteenths of the cell from its min corner: (corners, faces)
_MXI_A = [(3, 3, 4), (13, 3, 4), (8, 13, 12)]                   # a tilted triangle
_MXI_CONTENTS = (
    (_MXI_A + [(8, 6, 3), (8, 6, 13), (8, 10, 8)], [(0, 1, 2), (3, 4, 5)]),                  # a second one through it: a hit
    (_MXI_A + [(4, 11, 5), (5, 12, 5), (4, 12, 6)], [(0, 1, 2), (3, 4, 5)]),                 # a small one in a corner of its box: a candidate only
    (_MXI_A, [(0, 1, 2)]),                                                                  # alone
    ([(4, 4, 8), (12, 4, 8), (8, 12, 8), (8, 2, 12)], [(0, 1, 2), (1, 0, 3)]),               # two that share an edge and fold away: adjacent, no hit
)


def _mxi_big():
    """More than MXI_BIG triangles for one cell: 64 level ones at 64 heights, not one box overlapping another, and three upright ones through most
    of them."""
    v = []
    for i in range(MXI_BIG):
        z = (20 + 3 * i) / 16.0                                 # heights 20/256 .. 209/256 of the cell
        v += [(3, 3, z), (13, 3, z), (8, 13, z)]
    for x in (7, 8, 9):
        v += [(x, 6, 1.5), (x, 6, 14.5), (x, 10, 8)]
    return np.asarray(v, np.float64), [(3 * t, 3 * t + 1, 3 * t + 2) for t in range(MXI_BIG + 3)]


@functools.lru_cache(maxsize=None)
def intersect_case(scale=1):
    """Small triangles strictly inside the late grid cells of level 0 (arranged_cells(): late at every capacity; the grid of under 1,024
    triangles has 16,384 slots). mxi_tris_kernel boxes floor(v) + 4, so cell c holds the points of [c - 4, c - 3)^3. The cells take the four
    contents of _MXI_CONTENTS in turn, several triangles of one cell racing for one key; the LAST cell of the order - the longest walk - holds
    _mxi_big()'s 67 triangles, a cell for the big-cell list. scale 8: the same mesh with (v + 4) scaled by 8, which presents the same keys at
    level 3."""
    cells = arranged_cells()
    verts, faces, tri_cell = [], [], []
    for n, c in enumerate(cells.tolist()):
        if n == len(cells) - 1:
            local, f = _mxi_big()
            local = local / 16.0
        else:
            p, f = _MXI_CONTENTS[n % len(_MXI_CONTENTS)]
            local = np.asarray(p, np.float64) / 16.0
        base = sum(len(v) for v in verts)
        verts.append(local + np.asarray(c, np.float64) - MXI_OFFSET)
        faces += [[base + i for i in t] for t in f]
        tri_cell += [c] * len(f)
    v = np.concatenate(verts)
    if scale != 1:
        v = (v + MXI_OFFSET) * float(scale) - MXI_OFFSET
    f = np.asarray(faces, np.int32)
    tri_cell = np.asarray(tri_cell, np.int64)
    return _freeze(dict(name="intersect" if scale == 1 else "intersect_x%d" % scale, verts=v, faces=f, tri_cell=tri_cell, cells=cells, n_late=len(cells),
                        scale=scale, level=int(scale).bit_length() - 1, rule_n=len(f),
                        tables=dict(grid=dict(keys=_ro(keys_of_cells(tri_cell)), cap=intersect_cap(len(f))))))


def without_grid_cells(c, lost):
    """The faces of an intersect case whose grid cell's key is not in `lost`."""
    return np.asarray(c["faces"])[~np.isin(keys_of_cells(c["tri_cell"]), lost)]


# ---- ray pooling's pixel and cell tables ---------------------------------------------------------------------------------------------------------------------
RP_THRESH = 0.5
RP_PAIRS = np.asarray([[[0, 1], [0, 2]]], np.int64)             # view 0, the adversarial one, twice (the multiplicity path); views 1 and 2 once
# views 1 and 2: every entry a small integer, so their projections are exact too; view 2 is a perspective one with 4 + i depth bins
_RP_SIDE = [[[1, 0, 0, -3], [0, 1, 0, 0], [0, 0, 0, 1]], [[0, 64, 0, 0], [0, 0, 64, 0], [1, 0, 0, 4]]]


def pixel_key(w, h):
    """postpass.h's pixel key: (w, h) as two int32 with the sign bits flipped - (-1, -1) would otherwise be the empty sentinel."""
    w, h = ((np.asarray(a, np.int64) & 0xffffffff).astype(U64) ^ U64(0x80000000) for a in (w, h))
    return (w << U64(32)) | h


def rp_cell_key(slot, d):
    """postpass.h's cell key: the pixel's slot and the depth bin as int32 bits."""
    return (np.asarray(slot).astype(U64) << U64(32)) | (np.asarray(d, np.int64) & 0xffffffff).astype(U64)


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _project(cam, D):
    """(w, h, d) of every voxel of a D^3 cube at xyz 0, resol 1 under `cam`, in float64 as the kernel and post_oracle compute them (the entries
    are integers below 2^53 and so is every product and sum: the FMA chain is exact, the divisions round once)."""
    i, j, k = (x.reshape(-1).astype(np.float64) for x in np.indices((D, D, D)))
    q = [cam[r][0] * i + cam[r][1] * j + cam[r][2] * k + cam[r][3] for r in range(3)]
    return [np.rint(x).astype(np.int64) for x in (q[0] / q[2], q[1] / q[2], q[2] / 1.0)]


def _rp_case(name, table, D, cam0, sel, voxel_keys, pred16, cap, n_late, **more):
    m = len(sel)
    pred = np.full(D ** 3, 0.125, np.float32)
    pred[sel] = pred16.astype(np.float32) / 2048.0              # multiples of 2^-11 in [0.5, 1): exact in fp16
    assert int((pred.astype(np.float16) > np.float16(RP_THRESH)).sum()) == m and np.array_equal(pred.astype(np.float16).astype(np.float32), pred)
    rule = ray_pool_rule(m)
    assert rule["cap"] == cap
    cams = np.asarray([cam0] + _RP_SIDE, np.float64)
    return _freeze(dict(name=name, D=D, cameras=cams, pairs=RP_PAIRS.copy(), xyz=np.zeros((1, 3), np.float32), resol=np.ones(1, np.float32),
                        pred=pred.reshape(1, D, D, D), thresh=RP_THRESH, view=0, selected=sel, voxel_keys=voxel_keys, rule=rule, rule_n=m, n_late=n_late,
                        fill=LDS_FILL if rule["lds"] else (1, 2), tables={table: dict(keys=_ro(voxel_keys.copy()), cap=cap)}, **more))


@functools.lru_cache(maxsize=None)
def rp_pixels_case(m, D=32):
    """Ray pooling's PIXEL table under view 0, an affine camera (third row 0 0 0 1): voxel `flat` of a D^3 cube at xyz 0, resol 1 lands on pixel
    w = flat - 1000, h = -1 - 7 (i - i0) + 3 (j - j0) - 11 (k - k0), (i0, j0, k0) the voxel of flat index 999: pairwise distinct pixels, one
    cell each (d = 1), most of them negative or far outside any image, and voxel 999 on (-1, -1), the pixel whose plain key is the empty
    sentinel. Selected: that voxel, the voxels whose pixel key is late at the capacity ray_pool_rule(m) gives (at most 3 m / 4 of them, the
    first in flat order) and seeded others up to m. Keys in flat order (the kernel's own order is whatever the atomics give)."""
    cap = ray_pool_rule(m)["cap"]
    flat = np.arange(D ** 3, dtype=np.int64)
    i, j, k = np.unravel_index(flat, (D, D, D))
    i0, j0, k0 = np.unravel_index(999, (D, D, D))
    cam0 = [[D * D, D, 1, -1000], [-7, 3, -11, -1 + 7 * i0 - 3 * j0 + 11 * k0], [0, 0, 0, 1]]
    w, h, d = _project(cam0, D)
    assert np.array_equal(w, flat - 1000) and np.array_equal(h, -1 - 7 * (i - i0) + 3 * (j - j0) - 11 * (k - k0)) and (d == 1).all()
    assert (w[999], h[999]) == (-1, -1)
    keys = pixel_key(w, h)
    late = late_mask(keys, W, cap.bit_length() - 1)
    late[999] = False
    rs = np.random.RandomState(m)
    late_idx = np.nonzero(late)[0][:3 * m // 4]
    rest = np.nonzero(~late)[0]
    rest = rest[rest != 999]
    sel = np.sort(np.concatenate([late_idx, [999], rs.choice(rest, m - 1 - len(late_idx), replace=False)]))
    return _rp_case("pixels%d" % m, "pixel", D, cam0, sel, keys[sel], 1229 + rs.randint(0, 600, m), cap, len(late_idx))


@functools.lru_cache(maxsize=None)
def rp_cells_case(m, D=32, w=W):
    """Ray pooling's CELL table under view 0: depth bin d = 2^20 + D j + k (third row 0 D 1 2^20), h = H (second row H times the third) and
    w = rint(G 2^20 (i - D / 2) / d) = G (i - D / 2), off by less than G / 64 before the rint: D pixels, one per i, half of them at negative w,
    D^2 cells each. The cell key is (pixel slot << 32) | d; (G, H) is the first pair for which the D pixels' home slots are pairwise distinct,
    so every pixel gets its home slot whoever inserts first. Selected: the voxels whose cell key starts in the last 2^w slots of the capacity
    ray_pool_rule(m) gives, and seeded others up to m. The late cells carry the largest predictions of their pixels, larger the further the
    model walks them (a pixel's winner is the key a fault loses first); the two best late cells of the pixel with the most of them carry the
    SAME prediction: the tie goes to the smaller d."""
    cap = ray_pool_rule(m)["cap"]
    S = 1 << 20
    assert D == 32
    for G, H in ((g, h) for g in range(1, 32) for h in range(-9, 10)):
        pw = G * (np.arange(D, dtype=np.int64) - D // 2)
        home = (mix64(pixel_key(pw, np.full(D, H))) & U64(cap - 1)).astype(np.int64)
        if np.unique(home).size == D:
            break
    cam0 = [[G * S, 0, 0, -G * S * (D // 2)], [0, H * D, H, H * S], [0, D, 1, S]]
    pix_w, pix_h, d = _project(cam0, D)
    flat = np.arange(D ** 3, dtype=np.int64)
    i, j, k = np.unravel_index(flat, (D, D, D))
    assert np.array_equal(pix_w, pw[i]) and (pix_h == H).all() and np.array_equal(d, S + D * j + k)
    keys = rp_cell_key(home[i], d)
    late = late_mask(keys, w, cap.bit_length() - 1)
    rs = np.random.RandomState(m + 1)
    late_idx = np.nonzero(late)[0]
    sel = np.sort(np.concatenate([late_idx, rs.choice(np.nonzero(~late)[0], m - len(late_idx), replace=False)]))
    is_late = late[sel]
    model = probe_model(keys[sel], cap, fill=LDS_FILL if m <= RP_LDS_M else (1, 2))
    pred16 = 1229 + rs.randint(0, 400, m)
    order = np.argsort(model["walk"][is_late], kind="stable")
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    pred16[is_late] = 1847 + rank * 190 // len(order)
    per_pixel = np.bincount(i[sel][is_late], minlength=D)
    tied = np.nonzero(is_late & (i[sel] == int(np.argmax(per_pixel))))[0]
    tied = tied[np.argsort(pred16[tied], kind="stable")[-2:]]
    pred16[tied] = 2047
    return _rp_case("rp_cells%d" % m, "cell", D, cam0, sel, keys[sel], pred16, cap, len(late_idx), pixel_slots=home, tied=sel[tied], w=w)


@functools.lru_cache(maxsize=None)
def rp_zeros_case(D=12, G=2, H=-3, S=1049629):
    """The one way to lt_find<LtKeys, true> on the LDS tables: a voxel whose stored prediction is 0 asks for its pixel's cell at the view's
    minimum depth bin, and a 0 is selected only without a threshold, when EVERY voxel is: D^3 <= RP_LDS_M and D a multiple of 4 means D = 12 at
    the most, 1,728 keys in the 4,096 slots. rp_cells_case's view 0 (a pixel per i, bin d = S + D j + k, so every pixel has its cell at the
    minimum bin S, voxel (i, 0, 0)). (G, H, S) were searched for (H in -3 .. 3, G in 1 .. 31, S from 2^20 up: the first with distinct pixel home
    slots, 19 cell keys that start in the table's last sixteen slots, and a minimum-bin key of a pixel i >= 1 among them); the CPU test holds
    what they were searched for. The slices of those pixels and two more hold zeros only, so each of their 143 other voxels looks that key up
    (found: no vote; missed: a vote for voxel 0, which nothing else in view 0 elects - slice 0 is not all zero and voxel 0 holds a 0). The
    other slices hold eighths, a zero among them now and then."""
    m = D ** 3
    rule = ray_pool_rule(m)
    cap, half = rule["cap"], D // 2
    assert rule["lds"] and D % 4 == 0 and (D + 4) ** 3 > RP_LDS_M      # the largest cube edge the library takes whose every voxel fits the LDS tables
    pw = G * (np.arange(D, dtype=np.int64) - half)
    home = (mix64(pixel_key(pw, np.full(D, H))) & U64(cap - 1)).astype(np.int64)
    late = late_mask(rp_cell_key(home, S), W, cap.bit_length() - 1)
    late[0] = False
    cam0 = [[G * S, 0, 0, -G * S * half], [0, H * D, H, H * S], [0, D, 1, S]]
    pix_w, pix_h, d = _project(cam0, D)
    i, j, k = np.unravel_index(np.arange(m), (D, D, D))
    assert np.array_equal(pix_w, pw[i]) and (pix_h == H).all() and np.array_equal(d, S + D * j + k)
    zero = late.copy()
    zero[[n for n in range(1, D) if not late[n]][:2]] = True
    rs = np.random.RandomState(D)
    pred = (rs.randint(0, 8, m) / 8.0).astype(np.float32)
    pred[zero[i]] = 0
    pred[0] = 0
    pred[1] = 0.5                                                # slice 0 is not all zero, whatever the seed
    keys = rp_cell_key(home[i], d)
    cams = np.asarray([cam0] + _RP_SIDE, np.float64)
    return _freeze(dict(name="zeros_lds", D=D, cameras=cams, pairs=RP_PAIRS.copy(), xyz=np.zeros((1, 3), np.float32), resol=np.ones(1, np.float32),
                        pred=pred.reshape(1, D, D, D), thresh=None, view=0, selected=np.arange(m), voxel_keys=keys, rule=rule, rule_n=m,
                        n_late=int(late_mask(keys, W, cap.bit_length() - 1).sum()), fill=(1, 2), pixel_slots=home, zero_pixels=np.nonzero(zero)[0],
                        late_pixels=np.nonzero(late)[0], dmin=S, tables=dict(cell=dict(keys=_ro(keys.copy()), cap=cap))))


def without_voxels(c, lost):
    """A ray-pooling case's predictions with every selected voxel whose key is in `lost` below the threshold: what a table that lost those
    keys has pooled."""
    pred = np.array(c["pred"]).reshape(-1)
    pred[c["selected"][np.isin(c["voxel_keys"], lost)]] = 0.125
    return pred.reshape(c["pred"].shape)


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


# The cases whose keys are late at the ONE capacity their stage's sizing rule gives them (late_at): (builder, its adversarial table). They are
# no part of BUILDERS, whose cases are held at every capacity.
TARGETED = {
    "pixels_lds32": (lambda: rp_pixels_case(32), "pixel"), "pixels_lds2048": (lambda: rp_pixels_case(2048), "pixel"),
    "pixels_lds3400": (lambda: rp_pixels_case(RP_LDS_M), "pixel"), "pixels_global": (lambda: rp_pixels_case(4096), "pixel"),
    "pixels_unlisted": (lambda: rp_pixels_case(RP_LIST + 1, 64), "pixel"),
    "cells_lds2048": (lambda: rp_cells_case(2048), "cell"), "cells_lds3400": (lambda: rp_cells_case(RP_LDS_M), "cell"),
    "cells_global": (lambda: rp_cells_case(4096), "cell"),
    "bricks_mesh": (bricks_mesh_case, "brick"), "intersect": (intersect_case, "grid"),
}
RAY_POOL = tuple(n for n in TARGETED if n.startswith(("pixels", "cells")))
# ... and the only way to the COHERENT probe of the LDS tables: every voxel selected, zeros among them
FULL = {"zeros_lds": (rp_zeros_case, "cell")}


def targeted(name):
    """-> (case, its adversarial table)"""
    build, table = (TARGETED if name in TARGETED else FULL)[name]
    case = build()
    return case, case["tables"][table]


def rp_votes(c, pred=None, pairs=None):
    """post_oracle.ray_pool_1cube on a ray-pooling case (or on other predictions or another pair list for it): (D, D, D) uint8."""
    from oracle import post_oracle
    p16 = np.asarray(c["pred"] if pred is None else pred)[0].astype(np.float16)
    pairs = c["pairs"][0] if pairs is None else np.asarray(pairs)
    return post_oracle.ray_pool_1cube(c["cameras"], p16, pairs, c["xyz"][0], c["resol"][0], c["thresh"]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def rp_want(name):
    """The votes of a ray-pooling case, computed once and shared (read-only) among the tests."""
    return _ro(rp_votes(targeted(name)[0]))


def tables_of(name):
    """[(table name, table)] of the case's adversarial tables."""
    t = ADVERSARIAL[name]
    case = BUILDERS[name]()
    return [(k, case["tables"][k]) for k in ((t,) if isinstance(t, str) else t)]
