"""numpy restatement of scene.quantizePts2Cubes (utils/scene.py:63-108) for tests and tools/bench_ptcubes.py: the CPU test checks it against
goldens produced by the reference itself (tests/golden/ptcubes_cases.npz), the GPU tests check the library against it on clouds too large to
commit. Same arithmetic as the reference under numpy 2 - the caller's scalar types, the subtraction in the points' type, numpy's own
floor_divide in the promoted type, uint32 * stride in float64 - but the distinct cells come from one integer key per cell instead of a
row-wise np.unique over a structured view, so three million points take a second, not a quarter of a minute.

Also the seeded clouds the goldens, the GPU tests and the bench share (`wavy_cloud`), and the goldens' case reader (`golden_cases`)."""
import os

import numpy as np

CUBE_DTYPE = np.dtype([("xyz", np.float32, (3,)), ("ijk", np.uint32, (3,)), ("resol", np.float32)])
AXIS_BITS = 21
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ptcubes_cases.npz")
SCAN9 = dict(resol=0.4, cube_D=32, cube_Dcenter=26, cube_overlapping_ratio=0.5)             # params.py:107,114,168
SCAN9_BB = np.array([[-73, 129], [-197, 183], [472, 810]], dtype=np.int16)                  # ObsMask9_10.mat, as scene_cases.npz holds it


def as_points(pts_xyz):
    pts = np.asarray(pts_xyz)
    if pts.dtype not in (np.float32, np.float64):
        pts = pts.astype(np.float64)
    return pts.reshape(-1, 3)


def promoted(pts_dtype, stride):
    """dtype of (pts - shift) // stride under numpy 2: a Python scalar does not widen the array's type, a numpy scalar promotes by its dtype."""
    return np.result_type(pts_dtype, stride.dtype) if isinstance(stride, np.generic) else np.dtype(pts_dtype)


def quantizePts2Cubes(pts_xyz, resol, cube_D, cube_Dcenter, cube_overlapping_ratio, BB=None):
    pts = as_points(pts_xyz)
    if not np.isfinite(pts).all():
        raise ValueError("non-finite coordinate")
    side = resol * cube_D
    stride = resol * cube_Dcenter * cube_overlapping_ratio
    half = side / 2
    if BB is not None:
        BB = np.asarray(BB)
        keep = np.ones((pts.shape[0],), bool)
        for ax in range(3):
            keep &= (pts[:, ax] >= (BB[ax, 0] - half)) & (pts[:, ax] <= (BB[ax, 1] + half))
        pts = pts[keep]
    if pts.shape[0] == 0:
        raise ValueError("no point left")
    shift = pts.min(axis=0)
    T = promoted(pts.dtype, stride)
    q = np.floor_divide((pts - shift[None, :]).astype(T), T.type(stride)).astype(np.int64)
    if q.min() < 0 or q.max() + 1 >= (1 << AXIS_BITS):
        raise ValueError("cell index beyond 2^%d" % AXIS_BITS)
    key = (q[:, 0] << (2 * AXIS_BITS)) | (q[:, 1] << AXIS_BITS) | q[:, 2]
    diag = (1 << (2 * AXIS_BITS)) | (1 << AXIS_BITS) | 1
    key = np.unique(key)
    keys = np.unique(np.concatenate([key, key + diag]))                                    # floor corner and diagonal corner: the reference's two
    m = (1 << AXIS_BITS) - 1
    cubes = np.empty((keys.size,), dtype=CUBE_DTYPE)
    cubes["ijk"] = np.stack([keys >> (2 * AXIS_BITS), (keys >> AXIS_BITS) & m, keys & m], axis=1)
    centre = cubes["ijk"].astype(np.float64) * np.float64(stride) + shift[None, :].astype(np.float64)
    cubes["xyz"] = centre - np.float64(half)
    cubes["resol"] = resol
    return cubes, side


def wavy_cloud(n, BB=SCAN9_BB, seed=0, dtype=np.float64, spatial=True):
    """n points of a noisy wavy sheet spanning BB's x and y around the middle of its z range. spatial: raster order (x slow, y fast), as a
    reconstruction or a scanner writes a cloud; else a seeded permutation of it."""
    BB = np.asarray(BB, dtype=np.float64)
    rs = np.random.RandomState(seed)
    nx = max(1, int(np.sqrt(n * (BB[0, 1] - BB[0, 0]) / (BB[1, 1] - BB[1, 0]))))
    ny = -(-n // nx)
    i = np.arange(n)
    x = BB[0, 0] + ((i // ny) + rs.rand(n)) * ((BB[0, 1] - BB[0, 0]) / nx)
    y = BB[1, 0] + ((i % ny) + rs.rand(n)) * ((BB[1, 1] - BB[1, 0]) / ny)
    ext = BB[:, 1] - BB[:, 0]
    z = BB[2].mean() + 0.2 * ext[2] * np.sin(x * (9.0 / ext[0]) + 1.0) * np.cos(y * (7.0 / ext[1]) + 2.0) + rs.normal(0, 0.002 * ext[2], n)
    pts = np.stack([x, y, z], axis=1)
    if not spatial:
        pts = pts[rs.permutation(n)]
    return np.ascontiguousarray(pts.astype(dtype))


_RESOL_KINDS = {0: float, 1: np.float32, 2: np.float64, 3: int}


def golden_cases(path=GOLDEN):
    """[(name, kwargs of quantizePts2Cubes, expected ijk, xyz, cube_D_mm)] of the goldens. Points shared by several cases are stored once
    (`base_*`, float64) and cast per case; `extra` rows - points placed exactly on and just outside the widened box - follow them."""
    g = np.load(path)
    out = []
    for name in [str(s) for s in g["names"]]:
        k = lambda f: g[name + "_" + f]
        pts = g[str(k("pts_of"))] if (name + "_pts_of") in g.files else k("pts")
        dt = np.dtype(str(k("dtype")))
        pts = pts.astype(dt)
        if (name + "_extra") in g.files:
            pts = np.concatenate([pts, k("extra").astype(dt)])
        resol = _RESOL_KINDS[int(k("resol_kind"))](k("resol"))
        D, Dc = [int(v) for v in k("cube")]
        kw = dict(pts_xyz=pts, resol=resol, cube_D=D, cube_Dcenter=Dc, cube_overlapping_ratio=float(k("ratio")),
                  BB=(k("BB") if (name + "_BB") in g.files else None))
        out.append((name, kw, k("ijk"), k("xyz"), k("cube_D_mm")))
    return out
