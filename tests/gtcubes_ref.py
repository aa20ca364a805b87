"""numpy restatement of the ground-truth mode for tests and tools/bench_gtcubes.py: the occupancy tensor Y of a
batch of cubes from a point cloud, the per-cube counts of __weighted_accuracy__ (nets/SurfaceNet.py:203-224) and the accuracy formed from them.
The CPU test checks it against brute-force loops and the reference's own doctest; the GPU tests check the library against it, bit for bit.

Occupancy: q = np.floor((p - xyz_c) / resol_c) per axis in float32 (one subtraction, one division); Y[c, 0, q0, q1, q2] = 1.0 iff some point
has 0 <= q < s on all three axes. Whatever numpy decides for an edge case (a point on a face, -0.0) is the definition."""
import numpy as np


def as_cloud(pts):
    return np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 3))


def as_cubes(xyz, resol):
    xyz = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3))
    resol = np.ascontiguousarray(np.broadcast_to(np.asarray(resol, np.float32).reshape(-1), (xyz.shape[0],)))
    return xyz, resol


def voxel_index(pts, xyz_c, resol_c):
    """The float32 expression that alone decides membership: (P,3) float32 voxel indices (not yet range-checked)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.floor((pts - xyz_c[None, :]) / resol_c)


def gt_cubes(pts, xyz, resol, s, sorted_x=None):
    """Y (n,1,s,s,s) float32. sorted_x = (order, x of the points in that order) from `presort`: only the points of a slab of x around the cube
    (widened by two voxels and a relative 1e-4) are handed to the membership expression - which decides alone, as without it; the scale tests
    need it to stay quick, and tests/test_gtcubes_cpu.py checks that it changes nothing."""
    pts = as_cloud(pts)
    xyz, resol = as_cubes(xyz, resol)
    Y = np.zeros((xyz.shape[0], 1, s, s, s), np.float32)
    for c in range(xyz.shape[0]):
        cand = pts
        if sorted_x is not None:
            order, xs = sorted_x
            x0, r = float(xyz[c, 0]), float(resol[c])
            m = 2 * r + 1e-4 * (abs(x0) + s * r)
            cand = pts[order[np.searchsorted(xs, x0 - m, "left"):np.searchsorted(xs, x0 + s * r + m, "right")]]
        q = voxel_index(cand, xyz[c], resol[c])
        ok = ((0 <= q) & (q < s)).all(axis=1)
        qi = q[ok].astype(np.int64)
        Y[c, 0, qi[:, 0], qi[:, 1], qi[:, 2]] = 1.0
    return Y


def presort(pts):
    pts = as_cloud(pts)
    order = np.argsort(pts[:, 0], kind="stable")
    return order, pts[order, 0].astype(np.float64)


def accuracy_counts(pred, Y, threshold=0.5):
    """(n,4) int64 per leading index: n_pos (Y > 0), n_neg (Y == 0), hit_pos, hit_neg with hit = (float32(pred >= threshold) == Y)."""
    pred, Y = np.asarray(pred, np.float32), np.asarray(Y, np.float32)
    n = pred.shape[0]
    p, y = pred.reshape(n, -1), Y.reshape(n, -1)
    with np.errstate(invalid="ignore"):
        pos, neg = y > 0, y == 0
        hit = (p >= np.float32(threshold)).astype(np.float32) == y
    return np.stack([pos.sum(1), neg.sum(1), (pos & hit).sum(1), (neg & hit).sum(1)], axis=1).astype(np.int64)


def accuracy_from_counts(counts):
    """(acc_pos + acc_neg) / 2 in float64 from the summed counts; acc_pos = acc_neg when there is no positive; NaN when there is no negative."""
    n_pos, n_neg, hit_pos, hit_neg = (np.float64(v) for v in np.asarray(counts, np.int64).reshape(-1, 4).sum(axis=0))
    with np.errstate(divide="ignore", invalid="ignore"):
        acc_neg = hit_neg / n_neg
        acc_pos = hit_pos / n_pos if n_pos != 0 else acc_neg
        return np.float64((acc_pos + acc_neg) / 2.0)


def weighted_accuracy(pred, Y, threshold=0.5):
    """__weighted_accuracy__(pred, Y) of the whole tensors (any shape): one accuracy, as the reference computes it."""
    pred, Y = np.asarray(pred, np.float32), np.asarray(Y, np.float32)
    return accuracy_from_counts(accuracy_counts(pred.reshape(1, -1), Y.reshape(1, -1), threshold))


def weighted_accuracy_direct(pred, Y, threshold=0.5):
    """The reference's expression read literally (selections, binary_accuracy, means), for the CPU test to hold the count form against."""
    pred, Y = np.asarray(pred, np.float32).reshape(-1), np.asarray(Y, np.float32).reshape(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        binary_accuracy = lambda p, t: ((p >= np.float32(threshold)).astype(np.float32) == t).astype(np.float64)
        pos, neg = np.nonzero(Y > 0)[0], np.nonzero(Y == 0)[0]
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)                # mean of an empty selection: NaN
            acc_neg = np.mean(binary_accuracy(pred[neg], Y[neg]))
            acc_pos = acc_neg if (Y > 0).sum() == 0 else np.mean(binary_accuracy(pred[pos], Y[pos]))
        return np.float64((acc_pos + acc_neg) / 2.0)
