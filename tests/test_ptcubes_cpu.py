"""CPU: the point-seeded cube list's checker (tests/ptcubes_ref.py) against goldens recorded from the reference's scene.quantizePts2Cubes
(tests/golden/ptcubes_cases.npz, tools/gen_golden_ptcubes.py), and the host side of surfacenet_amd.scene: the readers, initializeCubes, and
the errors raised before any GPU work."""
import numpy as np
import pytest

import ptcubes_ref as ref
from surfacenet_amd import scene, sparseCubes

CASES = ref.golden_cases()


def test_golden_file_holds_the_cases_the_contract_names():
    names = [c[0] for c in CASES]
    assert len(names) == len(set(names)) == 19
    for dt in ("float32", "float64"):
        for kind in ("py", "f32", "f64"):
            assert "wavy_%s_%s" % (dt, kind) in names and "wavy_%s_%s_bb" % (dt, kind) in names
    assert {"doc", "lattice_float32", "lattice_float64", "far_clusters", "dino", "single_point", "identical_points"} <= set(names)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_reference(case):
    name, kw, ijk, xyz, dmm = case
    cubes, side = ref.quantizePts2Cubes(**kw)
    assert cubes["ijk"].dtype == np.uint32 and np.array_equal(cubes["ijk"], ijk)              # also the row order
    assert cubes["xyz"].dtype == np.float32 and np.array_equal(cubes["xyz"], xyz)
    assert np.asarray(side).dtype == dmm.dtype and np.asarray(side) == dmm
    assert np.all(cubes["resol"] == np.float32(kw["resol"]))
    if name.endswith("_bb"):                                                                   # the box really cuts, and the points on it count
        assert ijk.shape[0] < dict((c[0], c[2]) for c in CASES)[name[:-3]].shape[0]


def test_floor_divide_is_not_floor_of_the_quotient():
    """1.0 // 0.1 is 9.0 in numpy (fmod-based), floor(1.0 / 0.1) is 10: the lattice goldens hold points where the two differ, and a point at
    exactly 1.0 with stride 0.1 lands in cell 9 (and its diagonal neighbour 10)."""
    assert np.floor_divide(np.float64(1.0), np.float64(0.1)) == 9.0 and np.floor(1.0 / 0.1) == 10.0
    cubes, _ = ref.quantizePts2Cubes(np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]), 0.1, 4, 2, 0.5)
    assert cubes["ijk"][:, 0].tolist() == [0, 1, 9, 10]
    lat = dict((c[0], c) for c in CASES)["lattice_float64"]
    x = np.unique(lat[1]["pts_xyz"][:, 0])
    assert np.any(np.floor_divide(x, 0.1) != np.floor(x / 0.1))


def test_two_corners_not_eight():
    """A point contributes its floor cell and the diagonally next one (the reference's vstack of floor and floor + 1 rows)."""
    name, kw, ijk, _, _ = dict((c[0], c) for c in CASES)["single_point"]
    assert ijk.tolist() == [[0, 0, 0], [1, 1, 1]]


def test_initializeCubes_is_the_reference_grid():
    g = np.load(ref.GOLDEN.replace("ptcubes_cases", "scene_cases"))
    cubes, side = scene.initializeCubes(resol=1, cube_D=22, cube_Dcenter=10, cube_overlapping_ratio=0.5, BB=g["doc_BB"])
    idx = g["doc_idx"]
    assert side == g["doc_cube_D_mm"] and cubes.shape[0] == int(g["doc_n"])
    assert np.array_equal(cubes["xyz"][idx], g["doc_xyz"]) and np.array_equal(cubes["ijk"][idx], g["doc_ijk"]) and np.array_equal(cubes["resol"][idx], g["doc_resol"])
    from surfacenet_amd import synthetic
    assert scene.initializeCubes is synthetic.cube_grid


def test_readers_round_trip(tmp_path):
    rs = np.random.RandomState(0)
    xyz = rs.normal(0, 50, (37, 3)).astype(np.float32)
    ply = str(tmp_path / "cloud.ply")
    sparseCubes.save2ply(ply, xyz, rgb_np=rs.randint(0, 255, (37, 3)).astype(np.uint8))
    got = scene.readPointCloud_xyz(ply)
    assert got.dtype == np.float32 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, xyz)
    v = rs.normal(0, 3, (25, 3))
    obj = str(tmp_path / "model.obj")
    with open(obj, "w") as f:
        f.write("# a comment\nmtllib none.mtl\n")
        for i, p in enumerate(v):
            f.write("v %r %r %r\n" % tuple(float(c) for c in p))
            if i % 5 == 0:
                f.write("vn 0 0 1\nvt 0.5 0.5\n")
        f.write("f 1 2 3\n")
    BB = scene.readBB_fromModel(obj)
    assert BB.shape == (3, 2) and np.array_equal(BB, np.c_[v.min(axis=0), v.max(axis=0)])


def test_errors_raised_on_the_host():
    pts = np.zeros((4, 3), np.float32)
    pts[2, 1] = np.nan
    with pytest.raises(ValueError):
        scene.quantizePts2Cubes(pts, 0.4, 32, 26, 0.5)
    pts[2, 1] = np.inf
    with pytest.raises(ValueError):
        scene.quantizePts2Cubes(pts.astype(np.float64), 0.4, 32, 26, 0.5)
    with pytest.raises(ValueError):                       # nothing to take a minimum of
        scene.quantizePts2Cubes(np.zeros((0, 3), np.float32), 0.4, 32, 26, 0.5)
    with pytest.raises(ValueError):                       # the checker agrees, also when the box leaves nothing
        ref.quantizePts2Cubes(pts, 0.4, 32, 26, 0.5)
    with pytest.raises(ValueError):
        ref.quantizePts2Cubes(np.zeros((3, 3)), 0.4, 32, 26, 0.5, BB=np.array([[100, 200], [100, 200], [100, 200]]))


def test_promotion_plan():
    """Which type the cell index divides in, and which stride values the library is handed (scene._plan), for every combination the contract names."""
    for pdt in (np.float32, np.float64):
        for resol in (0.4, np.float32(0.4), np.float64(0.4)):
            p = scene._plan(np.dtype(pdt), resol, 32, 26, 0.5, ref.SCAN9_BB)
            stride = resol * 26 * 0.5
            want64 = not (pdt == np.float32 and not isinstance(resol, np.float64))
            assert p["compute_f64"] == want64
            assert p["stride_q"] == float((np.float64 if want64 else np.float32)(stride)) and p["stride_xyz"] == float(stride)
            assert p["half"] == float(resol * 32 / 2) and type(p["side"]) is type(resol * 32)
            assert np.array_equal(p["box"], [[float(ref.SCAN9_BB[a, 0] - resol * 32 / 2) for a in range(3)], [float(ref.SCAN9_BB[a, 1] + resol * 32 / 2) for a in range(3)]])
