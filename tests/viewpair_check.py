"""The checker of the view-pair stage: the kernels between the similarityNet and the 3-D net that decide which cubes are reconstructed and which
view pairs reach the CNN with which weights (csrc/elementwise.h relw_mlp_kernel, relw_mlp_pairs_kernel, relw_softmax_kernel; csrc/simil.h
pair_simil_all_kernel). No GPU here: numpy, oracle/ and surfacenet_amd.viewPairSelection only.

    features                          the (n_cubes*P, 258) rows of viewPairSelection.viewPairSelection, in combinations order
    restate32_weights / _simil        float32 numpy restatements IN THE KERNELS' OWN ORDER. They are the yardstick of the tolerance (what float32
                                      arithmetic of this shape costs against fp64) and the carrier of the planted faults of
                                      tests/test_viewpair_cpu.py. They are never the reference: that is oracle/net_oracle.py, simil_oracle.py (fp64).
    restate32_rows                    the feature rows as relw_mlp_pairs_kernel gathers them from (embeddings, pair table, d, theta)
    check_weights / check_simil / check_selection

The weights' bound is RELATIVE, |got - ref| / ref, because the weights of a softmax over P pairs are about 1/P (8.5e-4 at DTU's 1,176 pairs): per
case, err32 = the restatement's worst relative error against the oracle, and the device gets max(4 * err32, 2**-21). The factor 4 is for what the
restatement cannot copy - FMA contraction of the 258-term sum, the device's expf, its division; 2**-21 (four ulps) is the floor for cases in
which err32 comes out freakishly small (P = 1: exactly 0)."""
import collections

import numpy as np

from oracle import net_oracle, simil_oracle
from surfacenet_amd import viewPairSelection as vps

F32 = np.float32
D_EMB, D_FEATURE, N_HIDDEN = 128, 258, 100
FACTOR, FLOOR = 4.0, 2.0 ** -21
SIMIL_ATOL = 1e-6            # the project's absolute bound of the pair similarity (tests/test_gpu_simil.py)
SHAPES = [(2, 5), (3, 129), (5, 130), (16, 40), (49, 12), (4, 1)]        # (n_views, n_cubes)
ROW_FAULTS = ("pairs_ji", "swap_cols", "pairs_jmajor", "cube_stride_P")
SIMIL_FAULTS = ("no_sqrt", "last_lane_dropped", "pairs_jmajor", "cube_stride_P")


def pair_table(n_views, fault=None):
    """(P, 2) int: all 2-combinations in combinations order - what both host wrappers upload. fault "pairs_jmajor": ordered by the second view."""
    pairs = vps.k_combination_np(range(n_views), k=2).reshape(-1, 2)
    if fault == "pairs_jmajor":
        pairs = np.asarray([(i, j) for j in range(n_views) for i in range(j)]).reshape(-1, 2)
    return pairs


def draw(n_views, n_cubes, seed):
    """Seeded inputs of one case: embeddings randn * 0.3, dissimilarities rand, cube centres rand * 100 + [-50, -50, 580], camera centres
    rand * 400 - 200 -> e (n, V, 128), d (n, P), theta (n, P) float32 (theta by viewPairSelection.viewPairAngles_wrt_pts)."""
    rs = np.random.RandomState(seed)
    P = n_views * (n_views - 1) // 2
    e = (rs.randn(n_cubes, n_views, D_EMB) * 0.3).astype(F32)
    d = rs.rand(n_cubes, P).astype(F32)
    centers = (rs.rand(n_cubes, 3) * 100 + [-50, -50, 580]).astype(F32)
    Ts = (rs.rand(n_views, 3) * 400 - 200).astype(F32)
    theta = vps.viewPairAngles_wrt_pts(Ts, centers).astype(F32)
    return dict(e=e, d=d, theta=theta, centers=centers, Ts=Ts, n_views=n_views, n_cubes=n_cubes, P=P)


def draw_near(n_views, n_cubes, seed):
    """Embeddings for the similarity's working range: draw()'s are 4.8 apart (128 components of randn * 0.3 each), where sigmoid(3 * dist - 2.5) is
    within 1e-5 of 1 and says little. Here the views of a cube are one randn * 0.3 vector plus randn * 0.3 * s, s = 0.3 * rand**2 per (cube, view) times
    1.5 * rand**3 per cube: distances of 0 .. 2, dissimilarities on both sides of the 0.1 and 0.5 of earlyRejection.selectFromSimilarity, cubes
    with every pair below 0.1 (rejected) and a different count of accepted pairs from cube to cube. Two edges are planted: cube 0's views 0 and 1
    are IDENTICAL (distance exactly 0), and the last cube's last view is multiplied by 100 (|w * dist + b| > 100: the logistic unit saturates to
    exactly 0 or 1). -> (n_cubes, n_views, 128) float32."""
    rs = np.random.RandomState(seed)
    base = rs.randn(n_cubes, 1, D_EMB) * 0.3
    s = 0.3 * rs.rand(n_cubes, n_views, 1) ** 2 * (1.5 * rs.rand(n_cubes, 1, 1) ** 3)
    e = (base + rs.randn(n_cubes, n_views, D_EMB) * 0.3 * s).astype(F32)
    e[0, 1] = e[0, 0]
    e[-1, -1] *= F32(100)
    return e


def features(e, d, theta):
    """(n_cubes*P, 258) float32 rows [emb[c,i] | emb[c,j] | d[c,p] | theta[c,p]] exactly as viewPairSelection.viewPairSelection assembles them
    (utils/viewPairSelection.py:69-74), pairs in combinations order."""
    e = np.asarray(e)
    n, V, D = e.shape
    viewPairs = pair_table(V)
    P = viewPairs.shape[0]
    ee = e[:, viewPairs.flatten()].reshape((n, P, 2 * D))
    return np.concatenate([ee, np.asarray(d).reshape(n, P, 1), np.asarray(theta).reshape(n, P, 1)], axis=-1).astype(F32).reshape((n * P, 2 * D + 2))


def restate32_rows(e, d, theta, fault=None):
    """The rows relw_mlp_pairs_kernel assembles in LDS: e1 = emb + (cube * n_views + pairs[2p]) * 128, e2 likewise with pairs[2p + 1], f[256] = d[row],
    f[257] = theta[row]. Equal to features() without a fault. Faults: "pairs_ji" (e1 and e2 exchanged), "swap_cols" (f[256] and f[257] exchanged),
    "pairs_jmajor" (the uploaded table ordered by the second view), "cube_stride_P" (cube * P instead of cube * n_views; a row index past the
    buffer wraps around it - a stand-in for whatever memory the device would read there)."""
    e = np.ascontiguousarray(e, dtype=F32)
    n, V, D = e.shape
    pairs = pair_table(V, fault)
    P = pairs.shape[0]
    flat = e.reshape(n * V, D)
    cube = np.repeat(np.arange(n), P)
    stride = P if fault == "cube_stride_P" else V
    i1, i2 = (1, 0) if fault == "pairs_ji" else (0, 1)
    r1 = (cube * stride + np.tile(pairs[:, i1], n)) % (n * V)
    r2 = (cube * stride + np.tile(pairs[:, i2], n)) % (n * V)
    c256, c257 = np.asarray(d, dtype=F32).reshape(-1, 1), np.asarray(theta, dtype=F32).reshape(-1, 1)
    if fault == "swap_cols":
        c256, c257 = c257, c256
    return np.concatenate([flat[r1], flat[r2], c256, c257], axis=1)


def _mlp_params(values):
    P = net_oracle.params_to_dict(values)
    fc, lin = P["feature_fc1"], P["feature_linear1"]
    f = lambda a: np.asarray(a, dtype=F32)
    scale = f(fc["gamma"]) * f(fc["inv_std"])                         # folded on the host by sn_load_weights, in float32
    shift = f(fc["beta"]) - f(fc["mean"]) * scale
    return f(fc["W"]), scale, shift, f(lin["W"]).reshape(-1), F32(np.asarray(lin["b"]).reshape(-1)[0])


def restate32_logits(features, values):
    """relw_mlp_kernel in float32, operation by operation: acc += f[k] * W1[k][j] for k = 0 .. 257 in turn (product and sum rounded separately),
    acc * scale + shift, 1 / (1 + exp(-x)), * w2[j], the halving tree over red[128] (hidden units 100 .. 127 hold zeros), + b2."""
    f = np.ascontiguousarray(features, dtype=F32)
    W1, scale, shift, w2, b2 = _mlp_params(values)
    acc = np.zeros((f.shape[0], N_HIDDEN), dtype=F32)
    for k in range(D_FEATURE):
        acc += f[:, k:k + 1] * W1[k]
    with np.errstate(over="ignore"):
        hv = F32(1) / (F32(1) + np.exp(-(acc * scale + shift))) * w2
    red = np.zeros((f.shape[0], 128), dtype=F32)
    red[:, :N_HIDDEN] = hv
    st = 64
    while st > 0:
        red[:, :st] = red[:, :st] + red[:, st:2 * st]
        st >>= 1
    return red[:, 0] + b2


def restate32_softmax(z, n_vp, fault=None):
    """relw_softmax_kernel: the row's maximum, the sum of expf(z - max) over p = 0 .. n_vp - 1 in turn, expf(z - max) / sum.
    fault "group_shift": group g starts at row g * n_vp + 1 (the row past the end wraps to row 0)."""
    z = np.asarray(z, dtype=F32).reshape(-1)
    if fault == "group_shift":
        z = np.roll(z, -1)
    z = z.reshape(-1, n_vp)
    ex = np.exp(z - z.max(axis=1, keepdims=True))
    total = np.cumsum(ex, axis=1, dtype=F32)[:, -1:]                 # cumsum: sequential, each partial sum rounded to float32
    return ex / total


def restate32_weights(features, values, n_vp, fault=None):
    """(n*n_vp, 258) -> (n, n_vp) float32: sn_relative_weights restated (restate32_logits, restate32_softmax)."""
    return restate32_softmax(restate32_logits(features, values), n_vp, fault)


def restate32_simil(emb, values, fault=None):
    """pair_simil_all_kernel in float32: emb (n_cubes, n_views, 128) -> (n_cubes, P). Lane l of the wave sums the squares of components l and l + 64,
    the 64 partial sums meet in the xor-butterfly (offsets 32, 16, .. 1), lane 0 stores 1 / (1 + expf(-(w * sqrtf(ss) + b))).
    Faults: "no_sqrt", "last_lane_dropped" (lane 63's two terms), "pairs_jmajor", "cube_stride_P" (as in restate32_rows)."""
    e = np.ascontiguousarray(emb, dtype=F32)
    n, V, D = e.shape
    pairs = pair_table(V, fault)
    P = pairs.shape[0]
    flat = e.reshape(n * V, D)
    cube = np.repeat(np.arange(n), P)
    stride = P if fault == "cube_stride_P" else V
    e1 = flat[(cube * stride + np.tile(pairs[:, 0], n)) % (n * V)]
    e2 = flat[(cube * stride + np.tile(pairs[:, 1], n)) % (n * V)]
    dd = np.abs(e1 - e2)
    sq = dd * dd
    v = sq[:, :64] + sq[:, 64:]                                       # ss = 0 + d0*d0 + d1*d1 per lane
    if fault == "last_lane_dropped":
        v[:, 63] = 0
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    ss = v[:, 0]
    w, b = F32(np.asarray(values[28]).reshape(())), F32(np.asarray(values[29]).reshape(()))
    dist = ss if fault == "no_sqrt" else np.sqrt(ss)
    with np.errstate(over="ignore"):
        out = F32(1) / (F32(1) + np.exp(-(w * dist + b)))
    return out.reshape(n, P)


WeightCheck = collections.namedtuple("WeightCheck", "ok err where err32 bound sum_err")


def weight_bound(r32, ref):
    """(err32, bound): the restatement's worst relative error against the fp64 oracle, and what the device gets for it."""
    err32 = float((np.abs(r32.astype(np.float64) - ref) / ref).max())
    return err32, max(FACTOR * err32, FLOOR)


def check_weights(got, features, values, n_vp, r32=None, ref=None):
    """got (n, n_vp) against net_oracle.relative_weights (fp64) by the RELATIVE error |got - ref| / ref, bound max(4 * err32, 2**-21); every row's sum
    against the sum of the restatement's row within the same bound (relative to that sum, which is 1 up to float32 rounding). Returns
    WeightCheck(ok, err = the worst relative error, where = its (row, column), err32, bound, sum_err). `r32`: restate32_weights(features, values,
    n_vp) and `ref`: the oracle's weights, if the caller has them already."""
    if ref is None:
        ref = net_oracle.relative_weights(features, values, n_vp)
    if r32 is None:
        r32 = restate32_weights(features, values, n_vp)
    err32, bound = weight_bound(r32, ref)
    got = np.asarray(got)
    if got.shape != ref.shape or got.dtype != F32:
        return WeightCheck(False, np.inf, None, err32, bound, np.inf)
    g = got.astype(np.float64)
    rel = np.abs(g - ref) / ref
    rel[~np.isfinite(rel)] = np.inf
    where = tuple(int(i) for i in np.unravel_index(int(np.argmax(rel)), rel.shape))
    err = float(rel[where])
    s32 = r32.astype(np.float64).sum(axis=1)
    sum_err = np.abs(g.sum(axis=1) - s32) / s32
    sum_err = float(np.where(np.isfinite(sum_err), sum_err, np.inf).max())
    return WeightCheck(bool(err <= bound and sum_err <= bound), err, where, err32, bound, sum_err)


SimilCheck = collections.namedtuple("SimilCheck", "ok err where err32")


def gather_pairs(emb):
    """(n_cubes, n_views, 128) -> (2 * n_cubes * P, 128): rows 2i, 2i + 1 = pair i, cube-major, in combinations order: what
    earlyRejection.embeddingPairs2simil hands to embeddingPair2simil_fn."""
    e = np.asarray(emb)
    pairs = pair_table(e.shape[1])
    return np.ascontiguousarray(e[:, pairs.flatten()].reshape(-1, e.shape[2]))


def simil_reference(emb, values):
    """fp64 oracle of every 2-combination: (n_cubes, P)."""
    e = np.asarray(emb)
    with np.errstate(over="ignore"):
        return simil_oracle.pair_similarity(gather_pairs(e), values).reshape(e.shape[0], -1)


def check_simil(got, emb, values):
    """got (n_cubes, P) against simil_oracle.pair_similarity (fp64) at the project's absolute 1e-6 ->
    SimilCheck(ok, err, where, err32 = the restatement's error, for the record)."""
    ref = simil_reference(emb, values)
    err32 = float(np.abs(restate32_simil(emb, values).astype(np.float64) - ref).max())
    got = np.asarray(got)
    if got.shape != ref.shape or got.dtype != F32:
        return SimilCheck(False, np.inf, None, err32)
    dif = np.abs(got.astype(np.float64) - ref)
    dif[~np.isfinite(dif)] = np.inf
    where = tuple(int(i) for i in np.unravel_index(int(np.argmax(dif)), dif.shape))
    return SimilCheck(bool(dif[where] < SIMIL_ATOL), float(dif[where]), where, err32)


def check_selection(pairs, w, ref_w_all, viewPairs, N, rtol):
    """The selection a device made, judged on the ORACLE's weights, with no exemption for near ties: pairs (n, N, 2) and w (n, N) as
    __argmaxN_viewPairs__ returns them (ascending), ref_w_all (n, P) the oracle's weights of every pair of viewPairs (P, 2).
      - every selected pair is a row of viewPairs, and the N pairs of a cube are distinct;
      - every selected pair's oracle weight is at least the oracle's N-th largest of that cube times (1 - 2 rtol): a device that is within rtol of
        the oracle can prefer a pair to another only if the oracle's weights of the two are that close;
      - the oracle's weights, read in the device's order, do not decrease by more than the same factor;
      - the device's own weights are within rtol of the oracle's.
    Returns the list of violations (empty: passes)."""
    pairs, w, ref_w_all, viewPairs = np.asarray(pairs), np.asarray(w), np.asarray(ref_w_all, dtype=np.float64), np.asarray(viewPairs)
    n, P = ref_w_all.shape
    bad = []
    if pairs.shape != (n, N, 2) or w.shape != (n, N):
        return ["shapes %s %s, expected (%d, %d, 2) and (%d, %d)" % (pairs.shape, w.shape, n, N, n, N)]
    V = int(max(viewPairs.max(), pairs.max())) + 1
    index = np.full((V * V,), -1, dtype=np.int64)
    index[viewPairs[:, 0] * V + viewPairs[:, 1]] = np.arange(P)
    idx = index[pairs[..., 0] * V + pairs[..., 1]] if pairs.min() >= 0 else np.full((n, N), -1)
    slack = 1.0 - 2.0 * rtol
    for c in range(n):
        if (idx[c] < 0).any():
            bad.append("cube %d: a selected pair is not in viewPairs" % c)
            continue
        if np.unique(idx[c]).size != N:
            bad.append("cube %d: pairs not distinct" % c)
        ref = ref_w_all[c, idx[c]]
        nth = np.sort(ref_w_all[c])[P - N]
        if (ref < nth * slack).any():
            bad.append("cube %d: selected oracle weight %.9g below the N-th largest %.9g" % (c, ref.min(), nth))
        if (ref[1:] < ref[:-1] * slack).any():
            bad.append("cube %d: oracle weights in the device's order decrease: %s" % (c, ref))
        if not (np.abs(w[c].astype(np.float64) - ref) <= rtol * ref).all():
            bad.append("cube %d: weights off by %.3e relative" % (c, float((np.abs(w[c] - ref) / ref).max())))
    return bad
