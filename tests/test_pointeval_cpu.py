"""CPU: the DTU evaluation's checker (tests/pointeval_ref.py) against itself, the PLY reader, and eval_ply's files driven by the restated
context (no GPU: surfacenet_amd.evaluation's host code with pointeval_ref.RefContext in place of the library)."""
import ctypes
import ctypes.util

import numpy as np
import pytest

import pointeval_ref as ref
from surfacenet_amd import evaluation, sparseCubes


def _clouds(rs):
    """Coincident points, pairs at exactly dst = 0.25 (on a 1/64 grid, so every difference is exact), dense clusters, uniform points."""
    base = rs.randint(0, 64, (300, 3)) / 64.0
    pairs = np.concatenate([base, base + [0.25, 0, 0], base + [0, 0.25, 0], base + [0, 0, -0.25]])
    clusters = np.repeat(rs.uniform(0, 3, (20, 3)), 20, axis=0) + rs.normal(0, 0.05, (400, 3))
    coincident = np.repeat(rs.uniform(0, 3, (50, 3)), 4, axis=0)
    return np.concatenate([pairs, clusters, coincident, rs.uniform(-1, 4, (400, 3))])


@pytest.mark.parametrize("dst", [0.25, 0.2, 0.0])
def test_reduce_rounds_equals_sequential_loop(dst):
    rs = np.random.RandomState(1)
    p = _clouds(rs)
    for order in (rs.permutation(p.shape[0]), np.arange(p.shape[0])):
        want = ref.reduce_sequential(p, order, dst)
        got, rounds = ref.reduce_rounds(p, order, dst, return_rounds=True)
        assert np.array_equal(got, want) and rounds >= 1
    # the survivors are independent and maximal
    I, J = ref.neighbour_pairs(p, dst)
    assert not (want[I] & want[J]).any()
    assert np.all(want | np.bincount(I[want[J]], minlength=p.shape[0]).astype(bool))


def test_neighbour_pairs_exact_at_dst():
    p = np.asarray([[0, 0, 0], [0.25, 0, 0], [0.5 + 2 ** -52, 0, 0], [0.25, 0.25, 0]], np.float64)
    I, J = ref.neighbour_pairs(p, 0.25)
    assert sorted(zip(I.tolist(), J.tolist())) == [(0, 1), (1, 0), (1, 3), (3, 1)]


def test_nn_brute_force_equals_kdtree():
    spatial = pytest.importorskip("scipy.spatial")
    rs = np.random.RandomState(2)
    to = np.concatenate([ref.wavy_surface(3000, rs), ref.wavy_surface(50, rs)[:10].repeat(3, axis=0)])
    frm = ref.data_cloud(to, rs)
    d2 = ref.nn_d2(to, frm)
    dist, _ = spatial.cKDTree(to).query(frm)
    assert np.allclose(np.sqrt(d2), dist, rtol=1e-12, atol=0)
    # the tree proposes every point within its own distance (+ a margin); the exact predicate decides
    cand = spatial.cKDTree(to).query_ball_point(frm, dist * (1 + 1e-9) + 1e-12)
    exact = np.asarray([ref.d2_rows(f[None, :], to[c]).min() for f, c in zip(frm, cand)])
    assert np.array_equal(exact, d2)
    assert np.all(ref.nn_d2(np.zeros((0, 3)), frm) == np.inf)


def test_round_half_away_from_zero():
    x = np.asarray([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999999999999994, -0.49999999999999994, 2.4999999999999996, 1e16 + 2, -3.0, 0.0])
    want = np.asarray([1, 2, 3, -1, -2, -3, 0, 0, 2, 1e16 + 2, -3, 0], np.float64)
    assert np.array_equal(ref.round_half_away(x), want)
    assert not np.array_equal(np.round(x), want)                               # numpy's is half to even
    assert np.floor(0.49999999999999994 + 0.5) == 1.0                            # floor(x + 0.5) is wrong there
    name = ctypes.util.find_library("m")
    if name:
        libm = ctypes.CDLL(name)
        libm.round.restype, libm.round.argtypes = ctypes.c_double, [ctypes.c_double]
        assert [libm.round(float(v)) for v in x] == want.tolist()


def test_mask_and_plane_flags():
    mask = np.zeros((5, 4, 3), np.uint8)
    mask[0, 0, 0] = mask[4, 3, 2] = mask[2, 1, 1] = 1
    bb, res = np.asarray([-2.0, -3.0, 1.0]), 2.0
    q = np.asarray([[-2.0, -3.0, 1.0], [-3.0, -3.0, 1.0], [-3.0 + 1e-15, -3.0, 1.0], [6.0, 3.0, 5.0], [7.0, 3.0, 5.0], [2.0, -1.0, 3.0],
                    [2.999, -0.001, 3.999], [1.0, -2.0, 2.0], [-100.0, 0.0, 0.0]])
    assert ref.in_mask(q, mask, bb, res).tolist() == [True, False, True, True, False, True, True, True, False]
    assert ref.above_plane(q, [0, 0, 1, -3]).tolist() == [False, False, False, True, True, False, True, False, False]


def _write_ply(path, fmt, verts, vdtype, pre=None, face=False):
    """A PLY with vertex properties x y z (+ an int tag), optional fixed-size element before, optional face list element after."""
    types = {"f4": "float", "f8": "double", "i4": "int", "u1": "uchar", "i2": "short"}
    end = "<" if fmt == "binary_little_endian" else ">"
    lines = ["ply", "format %s 1.0" % fmt, "comment written by a test"]
    if pre is not None:
        lines += ["element camera %d" % len(pre), "property short a", "property uchar b"]
    lines += ["element vertex %d" % len(verts)] + ["property %s %s" % (types[vdtype], k) for k in ("x", "y", "z")] + ["property int tag"]
    if face:
        lines += ["element face 1", "property list uchar int vertex_indices"]
    lines.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(lines) + "\n").encode("ascii"))
        if fmt == "ascii":
            if pre is not None:
                f.write("".join("%d %d\n" % tuple(r) for r in pre).encode())
            f.write("".join("%r %r %r %d\n" % (float(v[0]), float(v[1]), float(v[2]), i) for i, v in enumerate(verts)).encode())
            if face:
                f.write(b"3 0 1 2\n")
        else:
            if pre is not None:
                a = np.zeros(len(pre), np.dtype([("a", end + "i2"), ("b", "u1")]))
                a["a"], a["b"] = pre[:, 0], pre[:, 1]
                f.write(a.tobytes())
            v = np.zeros(len(verts), np.dtype([(k, end + vdtype) for k in ("x", "y", "z")] + [("tag", end + "i4")]))
            v["x"], v["y"], v["z"], v["tag"] = verts[:, 0], verts[:, 1], verts[:, 2], np.arange(len(verts))
            f.write(v.tobytes())
            if face:
                f.write(np.asarray([3], np.uint8).tobytes() + np.asarray([0, 1, 2], end + "i4").tobytes())


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
@pytest.mark.parametrize("vdtype", ["f4", "f8"])
def test_read_ply_xyz_formats(tmp_path, fmt, vdtype):
    rs = np.random.RandomState(3)
    verts = rs.uniform(-500, 500, (257, 3)).astype(vdtype)
    p = str(tmp_path / "a.ply")
    _write_ply(p, fmt, verts, vdtype, pre=np.asarray([[-7, 200], [3, 4]]), face=True)
    got = evaluation.read_ply_xyz(p)
    assert got.dtype == np.dtype(vdtype) and np.array_equal(got, verts)


def test_read_ply_xyz_of_save2ply(tmp_path):
    rs = np.random.RandomState(4)
    xyz = rs.uniform(-100, 100, (1000, 3)).astype(np.float32)
    p = str(tmp_path / "s.ply")
    sparseCubes.save2ply(p, xyz, rs.randint(0, 255, (1000, 3)).astype(np.uint8))
    assert np.array_equal(evaluation.read_ply_xyz(p), xyz)
    sparseCubes.save2ply(p, xyz[:0])
    assert evaluation.read_ply_xyz(p).shape == (0, 3)


@pytest.fixture
def ref_context(monkeypatch):
    from surfacenet_amd import runtime
    monkeypatch.setattr(runtime, "any_context", lambda: ref.RefContext())


def test_eval_ply_files_with_restated_context(tmp_path, ref_context):
    sio = pytest.importorskip("scipy.io")
    rs = np.random.RandomState(5)
    stl = ref.wavy_surface(4000, rs).astype(np.float32)
    data = ref.data_cloud(stl.astype(np.float64), rs).astype(np.float32)
    folder = ref.make_dtu_folder(str(tmp_path / "dtu"), 9, stl)
    m = sio.loadmat(str(tmp_path / "dtu" / "ObsMask" / "ObsMask9_10.mat"))
    assert m["BB"].dtype == np.int16 and m["BB"].shape == (2, 3) and m["ObsMask"].dtype == np.uint8
    assert all(m[k].dtype == np.uint8 for k in ("cSet", "Res", "Margin")) and all(s % 2 for s in m["ObsMask"].shape)
    sparseCubes.save2ply(str(tmp_path / "data.ply"), data)
    out = str(tmp_path / "eval.mat")
    got = evaluation.eval_ply(9, str(tmp_path / "data.ply"), out, str(tmp_path / "dtu"))
    base = ref.point_compare(data, stl, folder["mask"], folder["BB"], folder["Res"], folder["plane"])
    assert np.array_equal(got, ref.eval_acc_compl(base))
    assert 0 < got[0] < 1 and got[2] > 0
    be = sio.loadmat(out)["BaseEval"][0, 0]
    assert be["Qdata"].shape == (3, base["Qdata"].shape[0]) and np.array_equal(be["Qdata"], base["Qdata"].T)
    assert be["Qstl"].shape == (3, stl.shape[0]) and np.array_equal(be["Qstl"], stl.T.astype(np.float64))
    for k in ("Ddata", "Dstl", "DataInMask", "StlAbovePlane"):
        assert np.array_equal(be[k].reshape(-1), np.asarray(base[k]).astype(be[k].dtype)), k
    assert be["dst"].item() == 0.2 and be["cSet"].item() == 9 and be["Margin"].item() == 10
    assert np.array_equal(be["GroundPlane"].reshape(-1), folder["plane"])


def test_eval_acc_compl_multiplies_over_all_points():
    base = dict(Ddata=np.asarray([1.0, 2.0, 3.0, 4.0]), DataInMask=np.asarray([True, False, True, False]), Dstl=np.asarray([0.5, 60.0, 1.5]),
                StlAbovePlane=np.asarray([True, True, False]))
    assert evaluation.eval_acc_compl(base).tolist() == [1.0, 0.5, 60.5 / 3, 0.5]
