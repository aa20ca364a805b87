"""CPU restatement of the DTU point-cloud evaluation (surfacenet_amd/evaluation.py runs it on the GPU): numpy, float64,
d^2 = (dx*dx + dy*dy) + dz*dz. Candidate searches (grid buckets, KD-trees) only propose pairs; the exact predicate decides.

    nn_d2              min_j d^2 by chunked brute force
    capped             min(sqrt(d2), max_dist)
    reduce_sequential  reducePts_haa as the literal greedy loop
    reduce_rounds      the same result round by round (vectorised; checked against the loop, used at larger sizes)
    round_half_away, in_mask, above_plane, point_compare, eval_acc_compl
    RefContext         the three Context entries of the evaluation, restated (drives evaluation.py's host code on a CPU)
    make_dtu_folder    a synthetic DTU folder (stl PLY, ObsMask / Plane .mat with the real files' names and dtypes)
"""
import os

import numpy as np


def d2_rows(a, b):
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def nn_d2(to, frm, chunk=256):
    to, frm = np.asarray(to, np.float64).reshape(-1, 3), np.asarray(frm, np.float64).reshape(-1, 3)
    out = np.full((frm.shape[0],), np.inf)
    if to.shape[0] == 0:
        return out
    for s in range(0, frm.shape[0], chunk):
        out[s:s + chunk] = d2_rows(frm[s:s + chunk, None, :], to[None, :, :]).min(axis=1)
    return out


def capped(d2, max_dist):
    return np.minimum(np.sqrt(d2), float(max_dist))


def reduce_sequential(p, order, dst):
    p = np.asarray(p, np.float64).reshape(-1, 3)
    alive = np.ones((p.shape[0],), bool)
    for i in order:
        if alive[i]:
            near = d2_rows(p[i][None, :], p) <= dst * dst
            near[i] = False
            alive[near] = False
    return alive


def neighbour_pairs(p, dst):
    """Every ordered pair i != j with d^2 <= dst^2 (grid candidates on cells a little larger than dst, then the exact predicate)."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    n = p.shape[0]
    h = dst * (1.0 + 1e-6) if dst > 0 else 1.0
    c = np.floor((p - p.min(axis=0)) / h).astype(np.int64) + 1
    dims = c.max(axis=0) + 2
    key = lambda cc: (cc[:, 0] * dims[1] + cc[:, 1]) * dims[2] + cc[:, 2]
    order = np.argsort(key(c), kind="stable")
    ks = key(c)[order]
    I_all, J_all = [], []
    for off in np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), -1).reshape(-1, 3):
        nk = key(c + off)
        lo, hi = np.searchsorted(ks, nk, "left"), np.searchsorted(ks, nk, "right")
        cnt = hi - lo
        tot = int(cnt.sum())
        if tot == 0:
            continue
        I = np.repeat(np.arange(n), cnt)
        J = order[np.arange(tot) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)]
        ok = (I != J) & (d2_rows(p[I], p[J]) <= dst * dst)
        I_all.append(I[ok]); J_all.append(J[ok])
    if not I_all:
        return np.zeros((0,), np.int64), np.zeros((0,), np.int64)
    return np.concatenate(I_all), np.concatenate(J_all)


def reduce_rounds(p, order, dst, return_rounds=False):
    """The parallel greedy MIS: a round makes IN every undecided point whose smaller-rank neighbours are all OUT, then OUT every undecided
    point with an IN neighbour."""
    n = np.asarray(p).reshape(-1, 3).shape[0]
    rank = np.empty((n,), np.int64)
    rank[np.asarray(order)] = np.arange(n)
    I, J = neighbour_pairs(p, dst)
    UND, IN, OUT = 0, 1, 2
    st = np.zeros((n,), np.int8)
    rounds = 0
    while (st == UND).any():
        blocked = np.zeros((n,), bool)
        m = (st[I] == UND) & (rank[J] < rank[I]) & (st[J] != OUT)
        blocked[I[m]] = True
        st[(st == UND) & ~blocked] = IN
        m = (st[I] == UND) & (st[J] == IN)
        st[I[m]] = OUT
        rounds += 1
    return (st == IN, rounds) if return_rounds else st == IN


def round_half_away(x):
    """MATLAB's / C's round: half away from zero (x - trunc(x) is exact)."""
    t = np.trunc(x)
    return t + np.where(np.abs(x - t) >= 0.5, np.sign(x), 0.0)


def in_mask(q, mask, bb_min, res):
    q = np.asarray(q, np.float64).reshape(-1, 3)
    v = round_half_away((q - np.asarray(bb_min, np.float64).reshape(1, 3)) / float(res))
    dims = np.asarray(mask.shape)
    ok = np.all((v >= 0) & (v < dims), axis=1)
    out = np.zeros((q.shape[0],), bool)
    vi = v[ok].astype(np.int64)
    out[ok] = mask[vi[:, 0], vi[:, 1], vi[:, 2]] != 0
    return out


def above_plane(q, P):
    q, P = np.asarray(q, np.float64).reshape(-1, 3), np.asarray(P, np.float64).reshape(4)
    return ((P[0] * q[:, 0] + P[1] * q[:, 1]) + P[2] * q[:, 2]) + P[3] > 0


def eval_acc_compl(base):
    acc = np.asarray(base["Ddata"], np.float64) * np.asarray(base["DataInMask"], np.float64)
    compl = np.asarray(base["Dstl"], np.float64) * np.asarray(base["StlAbovePlane"], np.float64)
    return np.asarray([np.mean(acc), np.median(acc), np.mean(compl), np.median(compl)])


def point_compare(Qdata, Qstl, obs_mask, BB, Res, plane, dst=0.2, max_dist=60.0, seed=0):
    Qdata = np.asarray(Qdata, np.float64).reshape(-1, 3)
    keep = reduce_rounds(Qdata, np.random.RandomState(seed).permutation(Qdata.shape[0]), dst)
    Qd, Qs = Qdata[keep], np.asarray(Qstl, np.float64).reshape(-1, 3)
    BB = np.asarray(BB, np.float64).reshape(2, 3)
    return dict(Qdata=Qd, Qstl=Qs, Ddata=capped(nn_d2(Qs, Qd), max_dist), Dstl=capped(nn_d2(Qd, Qs), max_dist),
                DataInMask=in_mask(Qd, obs_mask, BB[0], float(np.asarray(Res).reshape(-1)[0])), StlAbovePlane=above_plane(Qs, plane))


class RefContext(object):
    """Context.point_reduce / nn_dist2 / point_flags, restated."""

    def point_reduce(self, xyz, rank, dst):
        order = np.argsort(np.asarray(rank))
        keep, rounds = reduce_rounds(xyz, order, dst, return_rounds=True)
        return keep, rounds

    def nn_dist2(self, to, frm, max_dist):
        d2 = nn_d2(to, frm)
        d2[d2 >= max_dist * max_dist * (1.0 + 2.0 ** -40)] = np.inf
        return d2

    def point_flags(self, xyz, mask=None, bb_min=None, res=None, plane=None):
        return (None if mask is None else in_mask(xyz, mask, bb_min, res)), (None if plane is None else above_plane(xyz, plane))


# ---- synthetic inputs ---------------------------------------------------------------------------------------------------------------------
def wavy_surface(n, rs, extent=(40.0, 30.0), z0=5.0, amp=2.0):
    xy = rs.uniform(0, 1, (n, 2)) * np.asarray(extent)
    z = z0 + amp * np.sin(xy[:, 0] / 7.0) * np.cos(xy[:, 1] / 5.0)
    return np.c_[xy, z]


def data_cloud(stl, rs, noise=0.15, dup=0.3, outliers=0.02, box=None):
    """A reconstruction-like cloud near `stl`: jittered points, exact duplicates (overlapping cubes) and uniform outliers in `box`."""
    d = stl[rs.randint(0, stl.shape[0], stl.shape[0] // 2)] + rs.normal(0, noise, (stl.shape[0] // 2, 3))
    d = np.concatenate([d, d[rs.randint(0, d.shape[0], int(dup * d.shape[0]))]])
    lo, hi = (stl.min(0) - 5, stl.max(0) + 5) if box is None else box
    d = np.concatenate([d, rs.uniform(lo, hi, (int(outliers * d.shape[0]), 3))])
    return d[rs.permutation(d.shape[0])]


def make_dtu_folder(root, cSet, stl, dims=(41, 33, 17), res=2, bb_min=(-10, -12, -4), plane=(0.01, -0.02, 1.0, -3.0), seed=0):
    """dataPath/Points/stl/stl{cSet:03d}_total.ply and dataPath/ObsMask/{ObsMask{cSet}_10, Plane{cSet}}.mat, with the real files' names and
    dtypes: cSet, Res, Margin uint8 (1,1); BB int16 (2,3); ObsMask uint8 (X,Y,Z) of odd dimensions; P (4,1) float64."""
    import scipy.io as sio
    from surfacenet_amd import sparseCubes
    rs = np.random.RandomState(seed)
    sparseCubes.save2ply(os.path.join(root, "Points", "stl", "stl%03d_total.ply" % cSet), np.asarray(stl, np.float32))
    mask = (rs.uniform(0, 1, dims) < 0.8).astype(np.uint8)
    bb = np.asarray([bb_min, np.asarray(bb_min) + res * (np.asarray(dims) - 1)], dtype=np.int16)
    os.makedirs(os.path.join(root, "ObsMask"), exist_ok=True)
    sio.savemat(os.path.join(root, "ObsMask", "ObsMask%d_10.mat" % cSet),
                dict(cSet=np.uint8([[cSet]]), Res=np.uint8([[res]]), Margin=np.uint8([[10]]), BB=bb, ObsMask=mask))
    sio.savemat(os.path.join(root, "ObsMask", "Plane%d.mat" % cSet), dict(P=np.asarray(plane, np.float64).reshape(4, 1)))
    return dict(mask=mask, BB=bb, Res=res, plane=np.asarray(plane, np.float64))
