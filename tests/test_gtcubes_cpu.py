"""CPU: the numpy restatement of the ground-truth mode (tests/gtcubes_ref.py) against brute-force loops and the reference's own doctest
(nets/SurfaceNet.py:203-224), and the host arithmetic of the package (surfacenet_amd.groundTruth.accuracy_from_counts) against it. The GPU
tests (tests/test_gpu_gtcubes.py) hold the library to this restatement."""
import math

import numpy as np
import pytest

import gtcubes_ref as ref
from surfacenet_amd import groundTruth, SurfaceNet


def _brute_cubes(pts, xyz, resol, s):
    Y = np.zeros((len(xyz), 1, s, s, s), np.float32)
    for c in range(len(xyz)):
        for p in pts:
            q = []
            for d in range(3):
                v = np.floor(np.float32(np.float32(p[d]) - np.float32(xyz[c][d])) / np.float32(resol[c]))
                q.append(v)
            if all(0 <= v < s for v in q):
                Y[c, 0, int(q[0]), int(q[1]), int(q[2])] = 1.0
    return Y


def _brute_counts(pred, Y, thr):
    out = np.zeros((pred.shape[0], 4), np.int64)
    for c in range(pred.shape[0]):
        for p, y in zip(pred[c].reshape(-1), Y[c].reshape(-1)):
            hit = (np.float32(1.0) if p >= np.float32(thr) else np.float32(0.0)) == y
            if y > 0:
                out[c, 0] += 1
                out[c, 2] += int(hit)
            elif y == 0:
                out[c, 1] += 1
                out[c, 3] += int(hit)
    return out


def test_occupancy_equals_the_triple_loop():
    rs = np.random.RandomState(0)
    s = 4
    xyz = np.array([[0.0, 0.0, 0.0], [-1.3, 0.2, 0.5], [0.8, 0.8, 0.8], [50.0, 50.0, 50.0]], np.float32)
    resol = np.array([0.5, 0.4, 0.8, 0.5], np.float32)
    pts = (rs.rand(60, 3) * 4 - 1.5).astype(np.float32)
    edge = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.5, 1.0, 1.5], [-0.0, 0.5, 0.5], [np.nextafter(np.float32(2.0), np.float32(0)), 1.9, 1.9],
                     [-1.3, 0.2, 0.5], [-1.3 + 1.6, 0.2, 0.5]], np.float32)           # faces, voxel boundaries, -0.0, a max face
    pts = np.concatenate([pts, edge, pts[:5]])
    want = _brute_cubes(pts, xyz, resol, s)
    got = ref.gt_cubes(pts, xyz, resol, s)
    assert got.dtype == np.float32 and got.shape == (4, 1, s, s, s)
    assert np.array_equal(got, want) and 0 < want[:3].sum() and want[3].sum() == 0
    assert set(np.unique(got)) <= {0.0, 1.0}
    assert np.array_equal(ref.gt_cubes(pts, xyz, resol, s, sorted_x=ref.presort(pts)), want)          # the slab prefilter changes nothing
    assert np.array_equal(ref.gt_cubes(pts[::-1], xyz, resol, s), want)                              # nor does the order
    assert got[0, 0, 0, 0, 0] == 1.0 and got[0, 0, 0, 1, 1] == 1.0                                   # the min face is inside, -0.0 is voxel 0
    assert ref.gt_cubes(np.array([[2.0, 0.0, 0.0]]), xyz[:1], resol[:1], s).sum() == 0               # the max face is outside
    assert ref.gt_cubes(np.zeros((0, 3)), xyz, resol, s).sum() == 0                                  # no points


def test_voxel_centres_reproduce_the_mask():
    rs = np.random.RandomState(1)
    for s, resol, origin in ((8, 0.4, (-3.0, 2.0, 640.0)), (12, 0.8, (17.5, -102.0, 0.25)), (5, 0.5, (0.0, 0.0, 0.0))):
        mask = rs.rand(s, s, s) < 0.3
        ijk = np.argwhere(mask)
        xyz = np.asarray(origin, np.float32)
        pts = (ijk + 0.5) * np.float32(resol) + xyz[None, :].astype(np.float64)
        Y = ref.gt_cubes(rs.permutation(pts), xyz[None, :], np.float32(resol), s)
        assert np.array_equal(Y[0, 0], mask.astype(np.float32))


def test_known_answer_of_the_reference_doctest():
    pred = np.array([[0.1, 0], [0.9, 1]], np.float32)
    gt = np.zeros((2, 2), np.float32)
    assert ref.weighted_accuracy(pred, gt) == 0.5                                    # two of four negatives are right, no positives
    assert ref.weighted_accuracy_direct(pred, gt) == 0.5
    counts = ref.accuracy_counts(pred.reshape(1, -1), gt.reshape(1, -1))
    assert counts.tolist() == [[0, 4, 0, 2]]
    acc = groundTruth.accuracy_from_counts(counts)
    assert acc == 0.5 and type(acc) is np.float64


def test_counts_equal_the_loop_and_the_literal_expression():
    rs = np.random.RandomState(2)
    pred = rs.rand(3, 1, 3, 3, 3).astype(np.float32)
    Y = (rs.rand(3, 1, 3, 3, 3) < 0.4).astype(np.float32)
    pred.reshape(-1)[:6] = [0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nan, 0.5, np.nan, 1.0]
    Y.reshape(-1)[:9] = [1, 1, 1, 0, 0, 0.7, -1.0, np.nan, 0.7]                      # soft, negative and NaN targets
    counts = ref.accuracy_counts(pred, Y)
    assert np.array_equal(counts, _brute_counts(pred, Y, 0.5))
    # a soft target is a positive that can never be hit; a negative or NaN target is in neither class
    assert counts[:, :2].sum() == Y.size - 2
    c0 = ref.accuracy_counts(np.array([[0.9, 0.9, 0.1, 0.9]], np.float32), np.array([[0.7, -1.0, 0.7, np.nan]], np.float32))
    assert c0.tolist() == [[2, 0, 0, 0]]
    assert ref.weighted_accuracy(pred, Y) == ref.weighted_accuracy_direct(pred, Y)
    assert groundTruth.accuracy_from_counts(counts) == ref.weighted_accuracy(pred, Y)
    assert counts.sum(axis=0).tolist() == ref.accuracy_counts(pred.reshape(1, -1), Y.reshape(1, -1))[0].tolist()
    for thr in (0.25, 0.75):
        assert np.array_equal(ref.accuracy_counts(pred, Y, thr), _brute_counts(pred, Y, thr))


def test_no_positive_and_no_negative():
    pred = np.array([[0.2, 0.6, 0.7, 0.1]], np.float32)
    empty = np.zeros((1, 4), np.float32)
    assert ref.accuracy_counts(pred, empty).tolist() == [[0, 4, 0, 2]]
    for f in (ref.accuracy_from_counts, groundTruth.accuracy_from_counts):
        assert f([[0, 4, 0, 2]]) == 0.5                                              # acc_pos = acc_neg = 0.5
        assert f([[2, 4, 2, 1]]) == (1.0 + 0.25) / 2
        assert math.isnan(f([[4, 0, 3, 0]]))                                         # no negative: the mean of an empty selection
        assert math.isnan(f(np.zeros((0, 4), np.int64)))
        assert f([[1, 1, 1, 0], [1, 3, 0, 2]]) == (0.5 + 0.5) / 2                    # rows are summed before the ratios: one accuracy per batch
    full = np.ones((1, 4), np.float32)
    assert math.isnan(ref.weighted_accuracy(pred, full)) and math.isnan(ref.weighted_accuracy_direct(pred, full))


def test_trainval_refuses_training_without_a_device():
    with pytest.raises(NotImplementedError):
        SurfaceNet.SurfaceNet_fn_trainVal(2, return_train_fn=True)
    assert SurfaceNet.SurfaceNet_fn_trainVal(2, return_train_fn=False, return_val_fn=False) == (None, None, None)
