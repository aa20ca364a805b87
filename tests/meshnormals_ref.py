"""CPU restatement of the mesh's own normals, area and volume, independent of the device code: Python integers in
object-dtype numpy arrays for the face and vertex vectors (no width to overflow), np.add.at for the corner sums, int.bit_length, `>>`,
math.sqrt and `/` for the unit rule. Every sum is an exact integer and the unit rule is one fixed float64 expression, so
tests/test_gpu_meshnormals.py compares bytes. It is the checker of tests/test_meshnormals_cpu.py too, and holds the cases the smoother's
list (tests/meshsmooth_ref.CASES) lacks."""
import functools
import math

import numpy as np

import mesh_refusals as bad
import meshsmooth_ref as sm

FIX = sm.FIX
MANT = 52
KEYS = ("face_normals", "vert_normals", "counts", "sums")


def _cross(u, v):
    """(n,3) x (n,3) of Python integers."""
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)


def unit(X, Y, Z):
    """Rule 3 of one integer triple -> ((x/l, y/l, z/l) as float32, rint(l) << s as an int)."""
    m = max(abs(X), abs(Y), abs(Z))
    if m == 0:
        return (np.float32(0), np.float32(0), np.float32(0)), 0
    s = max(0, m.bit_length() - MANT)
    x, y, z = float(X >> s), float(Y >> s), float(Z >> s)      # floor; exact: at most 52 bits and a sign
    l = math.sqrt((x * x + y * y) + z * z)
    return (np.float32(x / l), np.float32(y / l), np.float32(z / l)), int(np.rint(l)) << s


def _units(N):
    out = np.zeros((N.shape[0], 3), np.float32)
    twice = [0] * N.shape[0]
    for i, (X, Y, Z) in enumerate(N.tolist()):
        out[i], twice[i] = unit(X, Y, Z)
    return out, twice


def limbs(x):
    """A Python int as three 64-bit limbs, least significant first, two's complement."""
    x &= (1 << 192) - 1
    return [(x >> (64 * k)) & ((1 << 64) - 1) for k in range(3)]


def quantise(verts, faces):
    """The checks of section 4.18 in its words, then q (V,3) of Python ints (0 where unreferenced) and the referenced flags."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError("verts must be (V,3)")
    if f.ndim != 2 or f.shape[1] not in (3, 4):
        raise ValueError("nv: faces must be (F,3) or (F,4)")
    f = f.astype(np.int64)
    V, F = v.shape[0], f.shape[0]
    if V > sm.MAX_ITEMS or F > sm.MAX_ITEMS:
        raise ValueError("at most 2^28 vertices and faces")
    bad_index = ((f < 0) | (f >= V)).any(axis=1)
    referenced = np.zeros((V,), bool)
    referenced[f[~bad_index].reshape(-1)] = True
    with np.errstate(invalid="ignore"):
        in_range = ((v >= sm.LO) & (v < sm.HI)).all(axis=1)     # (NaN fails)
    bad_range = np.zeros((F,), bool)
    bad_range[~bad_index] = (~in_range[f[~bad_index]]).any(axis=1)
    code = np.where(bad_index, 1, np.where(bad_range, 2, 0))
    if code.any():
        first = int(np.nonzero(code)[0][0])
        raise ValueError(bad.INDEX_TEXT % (first, V) if code[first] == 1 else bad.RANGE_TEXT % first)
    q = np.zeros((V, 3), object)
    q[:] = 0
    q[referenced] = np.rint(v[referenced] * float(FIX)).astype(np.int64).astype(object)      # ties to even, exact
    return q, f, referenced


def normals(verts, faces):
    """verts (V,3) float64 in lattice cells, faces (F,3) or (F,4) integers -> dict: face_normals (F,3) float32, vert_normals (V,3) float32,
    counts (4,) int64, sums (6,) uint64, and what the tests look at beside them: N_f (F,3) and N_v (V,3) of Python ints, area2, vol6 as
    Python ints, referenced. ValueError names the first offending face."""
    q, f, referenced = quantise(verts, faces)
    V, (F, nv) = q.shape[0], f.shape
    c = [q[f[:, k]] for k in range(nv)]
    if nv == 3:
        N_f = _cross(c[1] - c[0], c[2] - c[0])
        tris = [(c[0], c[1], c[2])]
    else:
        N_f = _cross(c[2] - c[0], c[3] - c[1])
        tris = [(c[0], c[1], c[2]), (c[0], c[2], c[3])]
    N_f = N_f.reshape(F, 3)
    N_v = np.zeros((V, 3), object)
    N_v[:] = 0
    for k in range(nv):
        np.add.at(N_v, f[:, k], N_f)                            # once per corner
    face_normals, twice = _units(N_f)
    vert_normals, _ = _units(N_v)
    vol6 = 0
    for a, b, cc in tris:
        vol6 += int((a * _cross(b, cc).reshape(F, 3)).sum()) if F else 0
    area2 = sum(twice)
    zero_f = int(sum(1 for row in N_f.tolist() if row == [0, 0, 0]))
    zero_v = int(sum(1 for row, r in zip(N_v.tolist(), referenced) if r and row == [0, 0, 0]))
    counts = np.asarray([zero_f, zero_v, int(referenced.sum()), F * (nv - 2)], np.int64)
    return dict(face_normals=face_normals, vert_normals=vert_normals, counts=counts, sums=np.asarray(limbs(area2) + limbs(vol6), np.uint64),
                N_f=N_f, N_v=N_v, area2=area2, vol6=vol6, referenced=referenced)


def same_bytes(got, want):
    """The keys of KEYS on which a result differs from the restatement, byte for byte ([]: none)."""
    return [k for k in KEYS if np.asarray(got[k]).tobytes() != np.asarray(want[k]).tobytes() or np.asarray(got[k]).shape != np.asarray(want[k]).shape]


# ---- named cases beside the smoother's: (verts, faces). Do not modify the results. ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bigfan_case(n=300):
    """A fan that fills the range: the hub (vertex 0) at (-4,-4,-4), rim vertex i at floor(64 (1e6 + 9e5 (cos t, sin t, cos 7t))) / 64,
    t = 2 pi i / n, triangles (0, 1 + i, 1 + (i + 1) % n). Face components reach 70 bits and the hub's sums 75: the low words of the hub carry
    well over a hundred times, with addends of both signs."""
    t = 2 * np.pi * np.arange(n) / n
    rim = np.floor(64.0 * (1e6 + 9e5 * np.stack([np.cos(t), np.sin(t), np.cos(7 * t)], axis=1))) / 64.0
    v = np.concatenate([[[-4.0, -4.0, -4.0]], rim])
    i = np.arange(n)
    return v, np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], axis=1).astype(np.int32)


def rules_case():
    """The smoother's rules case: vertex 7 is unreferenced and not a number."""
    return sm.rules_case()


CASES = dict(sm.CASES, bigfan300=lambda: bigfan_case(300), rules=rules_case)


@functools.lru_cache(maxsize=None)
def reference(name):
    """normals of a named case, computed once and shared (read-only) among the tests."""
    return normals(*CASES[name]())
