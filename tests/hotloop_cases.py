"""Inputs of tests/test_hotloop_cpu.py and tests/test_gpu_hotloop.py: the small kernels around the network (the CVC warp, the two fusions, dense2sparse, ray
pooling, the point projection) at cube sizes 12 and 20 - s^3 = 1728 and 8000, no multiple of 256 or 1024, so the last workgroup of every launch is ragged -
and on the edges no golden reaches: views of unequal image size, half-pixel ties, the plane q2 == 0, voxels behind the camera, pixels beyond 2^31, weights
over sixty decades, voxels without weight, sums on an integer boundary, predictions one fp16 step either side of the threshold, empty cubes at both ends of a
batch. Seeded numpy only; nothing here touches the library. test_hotloop_cpu.py asserts, with the restatements of oracle/ alone, that every class named
here is present in the inputs; test_gpu_hotloop.py compares the kernels with the same restatements."""
import functools

import numpy as np

import golden_util
from oracle import post_oracle

SIZES = (12, 20)
MEAN6 = golden_util.MEAN6


def _ro(a):
    a.setflags(write=False)          # the cases are shared between tests: nobody edits them in place
    return a


def grid(xyz, resol, s):
    """(s^3, 3) float64 voxel centres in flat order i s^2 + j s + k, with the reference's arithmetic: double(i) * double(resol_f32) + double(min_f32)."""
    r = float(np.float32(resol))
    ax = [np.arange(s, dtype=np.float64) * r + float(np.float32(v)) for v in xyz]
    return np.stack([g.reshape(-1) for g in np.meshgrid(*ax, indexing="ij")], axis=1)


def numerators(P, pts):
    """(3, n) float64 q0, q1, q2 = P . [X Y Z 1] with the oracle's FMA chain."""
    pts = np.asarray(pts, np.float64)
    return post_oracle._numerators(np.asarray(P, np.float64), pts[:, 0], pts[:, 1], pts[:, 2])


# ---------------------------------------------------------------------------------------------------------------------- 1. the CVC warp
IMG_HW = ((9, 14), (1, 1), (37, 5), (1200, 1600), (2, 3))          # (H, W) of views 0 .. 4, bound in this order
V_TIE, V_FAR, V_PIN, V_DTU, V_NEG = range(5)
CVC_N, CVC_NVP = 3, 3
CVC_MAX_SAMPLES = 7                                               # 7 // 3 = 2 cubes per chunk: 3 cubes go as 2 + 1
CUBE_INT, CUBE_FRONT, CUBE_DTU = range(3)


@functools.lru_cache(maxsize=None)
def cvc_images():
    """Random colours in 1 .. 255: a voxel is 0 in the raw warp if and only if it is out of scope, so the premises can count shares in the oracle's output."""
    rs = np.random.RandomState(77)
    return tuple(_ro(rs.randint(1, 256, (h, w, 3)).astype(np.uint8)) for h, w in IMG_HW)


@functools.lru_cache(maxsize=None)
def cvc_cameras():
    P = np.zeros((5, 3, 4))
    P[V_TIE] = [[1, 0, 0, 0.5], [0, 1, 0, 0], [0, 0, 0, 1]]                    # u = X + 0.5, v = Y, q2 = 1: integer X is an exact tie
    P[V_FAR] = [[2.0 ** 32, 0, 0, -2.0 ** 32], [0, 1, 0, -2], [0, 0, 0, 1]]    # u = 2^32 (X - 1), v = Y - 2: |u| >= 2^31 wherever X != 1
    P[V_PIN] = [[4, 0, 2, 0], [0, 4, 0, 0], [0, 0, 1, 0]]                      # pinhole at the origin, q2 = Z
    P[V_NEG] = P[V_PIN] * np.asarray([[1.0], [1.0], [-1.0]])                   # its third row negated: q2 = -Z
    P[V_DTU] = golden_util.cameras()["P_dtu"][0]
    return _ro(P)


@functools.lru_cache(maxsize=None)
def cvc_case(s):
    """Three cubes: the integer lattice from (-3, -2, -5) (ties under V_TIE; its plane k = 5 is Z = 0 under V_PIN and V_NEG), a half-step lattice wholly in
    Z > 0 (in front of V_PIN, behind V_NEG), and a cube across the corner of the DTU frame."""
    assert s in SIZES
    xyz = np.asarray([[-3, -2, -5], [-3, -2, 2], [-164, -173, 638]], np.float32)
    resol = np.asarray([1.0, 0.5, 0.4], np.float32)
    pairs = np.asarray([[[V_TIE, V_PIN], [V_FAR, V_TIE], [-1, -5]],           # -1 = V_NEG, -5 = V_TIE
                        [[V_PIN, V_NEG], [V_NEG, V_NEG], [-3, -4]],           # -3 = V_PIN, -4 = V_FAR; (V_NEG, V_NEG): every voxel behind the camera
                        [[V_DTU, V_DTU], [V_DTU, -2], [-2, V_DTU]]], np.int64)    # -2 = V_DTU: one view six times
    return dict(s=s, pairs=_ro(pairs), xyz=_ro(xyz), resol=_ro(resol), cams=cvc_cameras(), imgs=cvc_images(),
                tie=(0, 0), zero_plane=(0, 1), behind=4)                      # (sample, side) of the designated slots; behind: a sample, both sides


def cvc_views(case):
    """(n * n_vp, 2) view of every (sample, side), negative ids wrapped."""
    p = case["pairs"].reshape(-1, 2)
    return np.where(p < 0, p + len(IMG_HW), p)


# ---------------------------------------------------------------------------------------------------------------------- 2. the fusion
FUSE_CASES = ((12, 2), (12, 3), (12, 5), (12, 6), (20, 3))         # (s, n_vp), n = 3
FUSE_N = 3


def fuse_weights(n_vp):
    """Row 0 spans 1e-30 .. 1e30, row 1 has a zero entry, row 2 has equal weights. Every row is non-decreasing, which fuse_bound relies on."""
    w = np.empty((FUSE_N, n_vp), np.float32)
    w[0] = np.logspace(-30, 30, n_vp)
    w[1] = np.sort(np.random.RandomState(n_vp).rand(n_vp) + 0.1)
    w[1, 0] = 0
    w[2] = 0.3
    return w


def fuse_restatement(unfused, w):
    """fuse_kernel (csrc/elementwise.h) in float32, operation for operation: wsum = ((w_0 + w_1) + ...) from 0, then from 0 the sum over p = 0 .. n_vp - 1 of
    unfused_p * (w_p / wsum) - one division per term, the product rounded, then the addition rounded (the library is built without contraction)."""
    unfused, w = np.asarray(unfused), np.asarray(w)
    assert unfused.dtype == np.float32 and w.dtype == np.float32
    n, n_vp = w.shape
    out = np.empty((n, 1) + unfused.shape[2:], np.float32)
    for c in range(n):
        wsum = np.float32(0)
        for p in range(n_vp):
            wsum = np.float32(wsum + w[c, p])
        acc = np.zeros(unfused.shape[2:], np.float32)
        for p in range(n_vp):
            acc = acc + unfused[c, p] * np.float32(w[c, p] / wsum)
        out[c, 0] = acc
    return out


def fuse_float64(unfused, w):
    u, w = np.asarray(unfused, np.float64), np.asarray(w, np.float64)
    return (u * w[:, :, None, None, None]).sum(axis=1, keepdims=True) / w.sum(axis=1)[:, None, None, None, None]


def fuse_bound(unfused, n_vp):
    """|float32 fusion - float64 fusion| <= (n_vp + 3) 2^-24 max|unfused| for weight rows that are >= 0 and non-decreasing. With u = 2^-24, U = max|unfused|,
    n = n_vp and c_p = w_p / wsum (>= 0, summing to 1), to first order in u:
      the division and the product of a term each move it by u |term|, together                                                2 u U  over the sum;
      wsum: adding to 0 is exact, the k-th partial sum s_k (k = 2 .. n) is rounded by at most u s_k, and s_k <= (k / n) wsum because it holds the k
      smallest weights: relative error of wsum, hence of every c_p, at most u sum_k k / n = u ((n + 1) / 2 - 1 / n);
      the terms: the same count, their k-th partial sum being at most U (c_0 + .. + c_{k-1}) <= U k / n:                 u U ((n + 1) / 2 - 1 / n).
    Sum: (n + 3 - 2 / n) u U. The 2 / n u U left over covers the second-order terms (< 4 n^2 u^2 U) and the underflow of a product (< 2^-149 each)."""
    return (n_vp + 3) * 2.0 ** -24 * float(np.abs(unfused).max())


# ---------------------------------------------------------------------------------------------------------------------- 3. the colour fusion
COLOR_S, COLOR_N = 12, 3
COLOR_NVP = (1, 3, 5)
COLOR_CLASSES = ("no_weight", "one_pair", "half", "full")


@functools.lru_cache(maxsize=None)
def color_case(n_vp):
    """Colours (n n_vp, 6, s, s, s) uint8, predictions (n, n_vp, s, s, s), weights (n, n_vp) and, per class, a (n, s, s, s) mask:
      no_weight  prediction 0 in every pair: 0 / 0 = NaN -> colour 0
      one_pair   prediction 0 in every pair but one: that pair's weight is x / x = 1 and the colour its own mean, truncated
      half       the float32 sum is exactly k + 0.5: one pair with an odd a + b; with n_vp >= 2 also two pairs of weight exactly 1/2 with means k and k + 1
      full       the float32 sum is exactly 255: one pair, both views 255
    Everywhere else predictions are random, a tenth of them 0, and in one x-slab every colour is 255, where the sum of the rounded weights decides 254 | 255."""
    s, n = COLOR_S, COLOR_N
    rs = np.random.RandomState(300 + n_vp)
    col = rs.randint(0, 256, (n, n_vp, 2, 3, s, s, s)).astype(np.uint8)
    pred = rs.rand(n, n_vp, s, s, s).astype(np.float32)
    pred[rs.rand(n, n_vp, s, s, s) < 0.1] = 0
    w = (rs.rand(n, n_vp) + 0.1).astype(np.float32)
    if n_vp >= 2:
        w[:, 1] = w[:, 0]                                          # pairs 0 and 1 weigh the same: equal predictions give the weights 1/2, 1/2
    col[:, :, :, :, s - 1] = 255                                   # the slab i = s - 1
    masks = {k: np.zeros((n, s, s, s), bool) for k in COLOR_CLASSES}
    free = rs.permutation(n * (s - 1) * s * s)                     # distinct voxels outside that slab
    at = lambda lo, hi: np.unravel_index(free[lo:hi], (n, s - 1, s, s))
    for name, (lo, hi) in zip(COLOR_CLASSES, ((0, 40), (40, 80), (80, 140), (140, 180))):
        c, i, j, k = at(lo, hi)
        masks[name][c, i, j, k] = True
        pred[c, :, i, j, k] = 0
        if name == "no_weight":
            continue
        p = rs.randint(0, n_vp, c.size)
        pred[c, p, i, j, k] = (rs.rand(c.size) * 0.9 + 0.05).astype(np.float32)
        if name == "half":
            two = (np.arange(c.size) % 2 == 1) & (n_vp >= 2)
            a = rs.randint(0, 255, (c.size, 3)).astype(np.uint8)
            for ch in range(3):
                col[c, p, 0, ch, i, j, k] = a[:, ch]
                col[c, p, 1, ch, i, j, k] = a[:, ch] + 1           # a + b odd: the pair's mean is a + 0.5
            c2, i2, j2, k2, a2 = c[two], i[two], j[two], k[two], a[two]
            pred[c2, :, i2, j2, k2] = 0
            for q in (0, 1) if n_vp >= 2 else ():                  # two pairs, equal weights and predictions, means a and a + 1
                pred[c2, q, i2, j2, k2] = np.float32(0.5)
                for ch in range(3):
                    col[c2, q, 0, ch, i2, j2, k2] = a2[:, ch] + q
                    col[c2, q, 1, ch, i2, j2, k2] = a2[:, ch] + q
        if name == "full":
            for ch in range(3):
                col[c, p, 0, ch, i, j, k] = 255
                col[c, p, 1, ch, i, j, k] = 255
    col = col.reshape(n * n_vp, 6, s, s, s)
    X = col.astype(np.float32) - MEAN6[None, :, None, None, None]
    return dict(n_vp=n_vp, col=_ro(col), X=_ro(X), pred=_ro(pred), w=_ro(w), masks=masks)


# ---------------------------------------------------------------------------------------------------------------------- 4. dense2sparse
D2S_GEOMETRY = ((12, None), (12, 7), (12, 1), (20, 13))           # (D, cube_Dcenter)
D2S_N, D2S_NVP = 5, 2
D2S_MIN_PROB = 0.7                                                 # no fp16 value: fp16(0.7) = 0x399A = 0.7001953125
D2S_EMPTY_FIRST, D2S_MIXED, D2S_WHOLE, D2S_ONE, D2S_EMPTY_LAST = range(5)
H07 = np.float16(D2S_MIN_PROB)
_h = lambda bits: np.asarray([bits], np.uint16).view(np.float16)[0]
H07_UP, H07_DOWN = _h(int(H07.view(np.uint16)) + 1), _h(int(H07.view(np.uint16)) - 1)
# float32 predictions and whether the reference keeps them (fp16(pred) > fp16(min_prob), sparseCubes.py:62 on the float16 cast of :136)
D2S_CLASSES = {
    "at": ([np.float32(H07)], False),
    "step_above": ([np.float32(H07_UP)], True),
    "step_below": ([np.float32(H07_DOWN)], False),
    # float32 values below fp16(0.7) that round up to it: float32(0.7) itself, and the midpoint to the value below (a tie: 0x399A is even)
    "rounds_up": ([np.float32(0.7), (np.float32(H07) + np.float32(H07_DOWN)) / np.float32(2)], False),
    # ... and above it that round down to it, the midpoint to the value above included: kept by a float32 comparison, not by the reference's
    "rounds_down": ([np.float32(0.7003), (np.float32(H07) + np.float32(H07_UP)) / np.float32(2)], False),
    "nan": ([np.float32(np.nan)], False),
    "zero": ([np.float32(0)], False),
}
D2S_PLANTED = 8                                                    # voxels per class in the mixed cube and in each empty cube, all inside the crop
# (rgb, enable_rayPooling, rayPool_thresh): the threshold rule without and with votes, and the vote rule at 1 and at 2 n_vp
D2S_CONFIGS = tuple((rgb, on, thr) for rgb in (True, False) for on, thr in ((False, 0), (True, 0), (True, 1), (True, 2 * D2S_NVP)))


def d2s_crop(D, dcenter):
    """-> (lo, dc) of sparseCubes.py:43-48."""
    return (0, D) if dcenter is None else ((D - dcenter) // 2, dcenter)


@functools.lru_cache(maxsize=None)
def d2s_case(D, dcenter):
    """Five cubes of float32 predictions: [empty, mixed, whole, one, empty]. `whole` keeps every voxel, `one` keeps only the last voxel of the crop;
    `mixed` carries D2S_PLANTED voxels of every class of D2S_CLASSES inside the crop and the empty cubes those of every class that is not kept (a 1-voxel
    crop has no room: there the classes lie around it). Cube `whole` sees one view four times, so its winners collect 2 n_vp votes."""
    lo, dc = d2s_crop(D, dcenter)
    hi = lo + dc
    n = D2S_N
    rs = np.random.RandomState(1000 * D + dc)
    pred = (rs.rand(n, D, D, D) * 0.69).astype(np.float32)                      # nothing kept yet
    mixed = rs.rand(D, D, D)
    pred[D2S_MIXED] = np.where(mixed < 0.4, 0.71 + 0.28 * rs.rand(D, D, D), pred[D2S_MIXED]).astype(np.float32)
    pred[D2S_WHOLE] = (0.71 + 0.28 * rs.rand(D, D, D)).astype(np.float32)
    pred[D2S_ONE, hi - 1, hi - 1, hi - 1] = np.float32(0.9)
    planted = {}
    plo, phi = (lo, hi) if dc >= 6 else (max(lo - 3, 0), min(hi + 3, D))        # room for the classes
    box = phi - plo
    for cube in (D2S_EMPTY_FIRST, D2S_MIXED, D2S_EMPTY_LAST):
        cells = [c for c in rs.permutation(box ** 3) if dc >= 6 or not all(lo <= plo + v < hi for v in np.unravel_index(c, (box,) * 3))]
        at = 0
        for name, (values, kept) in D2S_CLASSES.items():
            if kept and cube != D2S_MIXED:
                continue                                           # an empty cube stays empty
            i, j, k = (plo + v for v in np.unravel_index(cells[at:at + D2S_PLANTED], (box,) * 3))
            at += D2S_PLANTED
            pred[cube, i, j, k] = np.resize(np.asarray(values, np.float32), D2S_PLANTED)
            planted[(cube, name)] = (i, j, k)
    rgb = rs.randint(0, 256, (n, 3, D, D, D)).astype(np.uint8)
    pairs = rs.randint(0, 4, (n, D2S_NVP, 2)).astype(np.int64)
    pairs[D2S_WHOLE] = 1
    xyz = (rs.rand(n, 3) * [60, 60, 40] + [-30, -30, 590]).astype(np.float32)
    resol = np.full(n, 0.4, np.float32)
    return dict(D=D, dcenter=dcenter, lo=lo, dc=dc, pred=_ro(pred), rgb=_ro(rgb), pairs=_ro(pairs), xyz=_ro(xyz), resol=_ro(resol),
                cams=_ro(np.array(golden_util.cameras()["P_dtu"])), planted=planted)


@functools.lru_cache(maxsize=None)
def d2s_want(D, dcenter, pooling, thresh):
    """The oracle's dense2sparse of d2s_case, packed as the library returns it: offsets (n + 1,) int64, ijk (T, 3) u8, pred (T,) f16, rgb (T, 3) u8, votes
    (T,) u8 | None."""
    c = d2s_case(D, dcenter)
    p16 = c["pred"].astype(np.float16)
    rgb8 = np.ascontiguousarray(np.transpose(c["rgb"], (0, 2, 3, 4, 1)))
    with np.errstate(invalid="ignore"):
        ne, ijk, p, rgb, votes, _ = post_oracle.dense2sparse(p16, rgb8, c["xyz"], c["resol"], c["pairs"], min_prob=D2S_MIN_PROB, rayPool_thresh=thresh,
                                                             enable_centerCrop=dcenter is not None, cube_Dcenter=dcenter, enable_rayPooling=pooling,
                                                             cameraPOs=c["cams"])
    counts = np.zeros(D2S_N, np.int64)
    counts[ne] = [len(x) for x in p]
    cat = lambda lst, shape, dt: np.concatenate(lst) if lst else np.zeros(shape, dt)
    return dict(offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), ijk=cat(ijk, (0, 3), np.uint8), pred=cat(p, (0,), np.float16),
                rgb=cat(rgb, (0, 3), np.uint8), votes=cat(votes, (0,), np.uint8) if pooling else None)


# ---------------------------------------------------------------------------------------------------------------------- 5. ray pooling
RP_N, RP_NVP = 3, 2
RP_CASES = tuple((D, thr) for D in SIZES for thr in (0.5, None))


@functools.lru_cache(maxsize=None)
def rp_case(D, thresh):
    """A wavy surface of probabilities in eighths (equal values along a ray: the argmax ties), a fifth of them 0 when nothing is thresholded (pixels whose
    stored values are all 0). One cube sees one view four times, and one pair list holds negative ids."""
    n = RP_N
    rs = np.random.RandomState(10 * D + (0 if thresh is None else 1))
    g = np.indices((D, D, D)).astype(np.float32) / D
    pred = np.empty((n, D, D, D), np.float32)
    for i in range(n):
        dist = g[i % 3] - (0.5 + 0.2 * np.sin(5 * g[(i + 1) % 3] + i) * np.cos(4 * g[(i + 2) % 3]))
        p = np.exp(-(dist * D / 2.0) ** 2) * 0.9 + 0.08 * rs.rand(D, D, D)
        p = np.round(p * 8) / 8
        if thresh is None:
            p[rs.rand(D, D, D) < 0.2] = 0
        pred[i] = np.clip(p, 0, 0.9999)
    pairs = np.asarray([[[1, 1], [1, 1]], [[0, 3], [2, 0]], [[-1, 2], [-4, 1]]], np.int64)
    xyz = (rs.rand(n, 3) * [60, 60, 40] + [-30, -30, 590]).astype(np.float32)
    resol = np.asarray([0.4, 0.2, 0.8], np.float32)
    return dict(D=D, thresh=thresh, pred=_ro(pred), pairs=_ro(pairs), xyz=_ro(xyz), resol=_ro(resol), cams=_ro(np.array(golden_util.cameras()["P_dtu"])))


@functools.lru_cache(maxsize=None)
def rp_want(D, thresh):
    c = rp_case(D, thresh)
    p16 = c["pred"].astype(np.float16)
    return _ro(np.stack([post_oracle.ray_pool_1cube(c["cams"], p16[i], c["pairs"][i], c["xyz"][i], c["resol"][i], thresh) for i in range(RP_N)]).astype(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------- 6. the projection
PROJ_N = (1, 255, 256, 257, 1000)
PROJ_V = (1, 5)


def proj_cameras(V):
    """V = 5: the pinhole, the tie camera, the DTU camera, the negated pinhole, the far camera; V = 1: the pinhole alone (q2 = Z)."""
    P = cvc_cameras()
    return np.ascontiguousarray(P[[V_PIN, V_TIE, V_DTU, V_NEG, V_FAR][:V]])


@functools.lru_cache(maxsize=None)
def proj_points(n):
    """Point t: t % 4 == 0 an integer point with Z a power of two (u = X + 0.5 under the tie camera; 4 X / Z + 2 is a tie under the pinhole whenever
    4 X / Z is an odd multiple of 1/2), t % 4 == 1 a point of the plane Z = 0 (q2 == 0 under both pinholes: +-inf, and 0 / 0 = NaN on the axes), else a point
    of the DTU scene."""
    rs = np.random.RandomState(n)
    pts = rs.rand(n, 3) * [60, 60, 40] + [-30, -30, 590]
    t = np.arange(n)
    a, b = t % 4 == 0, t % 4 == 1
    pts[a] = np.stack([rs.randint(-9, 10, n), rs.randint(-9, 10, n), 2.0 ** rs.randint(0, 5, n)], axis=1)[a]
    pts[b] = np.stack([rs.randint(-2, 3, n), rs.randint(-2, 3, n), np.zeros(n)], axis=1)[b]
    return _ro(np.ascontiguousarray(pts, np.float64))
