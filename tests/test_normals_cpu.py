"""CPU: the contract of the output cloud's normals on hand-made sheets through the numpy restatement
(tests/normals_ref.py), the argument checks of surfacenet_amd.normals - all of which run before the library is touched - and scene_postpass's
unchanged result without the new arguments."""
import inspect

import numpy as np
import pytest

import normals_ref as ref
from surfacenet_amd import normals, reconstruct


def test_axis_aligned_sheet_moments_by_hand_and_exact_normal():
    s = ref.hand_scene([[0, 0, 0]], ref.sheet_5x5(z=7))
    r = ref.normals_ref(*ref.scene_args(s), radius=2, min_neighbours=6)
    mom = r["moments"]
    # centre voxel (12,12,7), packed index 12: the whole 5x5 sheet lies in its window
    assert mom[12].tolist() == [25, 0, 0, 0, 50, 0, 0, 50, 0, 0]
    # corner voxel (10,10,7), index 0: d in {0,1,2}^2 x {0}: n = 9, sum dx = sum dy = 9, sum dx^2 = sum dy^2 = 15, sum dx dy = 9
    assert mom[0].tolist() == [9, 9, 9, 0, 15, 9, 0, 15, 0, 0]
    # edge voxel (10,12,7), index 2: dx in {0,1,2}, dy in {-2..2}: n = 15, sum dx = 15, sum dy = 0, sum dx^2 = 25, sum dy^2 = 30
    assert mom[2].tolist() == [15, 15, 0, 0, 25, 0, 0, 30, 0, 0]
    assert r["solved"].all()
    assert np.array_equal(r["normals"], np.tile(np.asarray([0, 0, 1], np.float32), (25, 1)))          # cameras above: +z, exactly
    below = dict(s, cameraTs=ref.cameras_above(4, sign=-1.0))
    assert np.array_equal(ref.normals_ref(*ref.scene_args(below))["normals"], -r["normals"])
    # radius 1 at the corner: 4 cells < min_neighbours = 6 -> zero normal there, and only at the corners
    r1 = ref.normals_ref(*ref.scene_args(s), radius=1, min_neighbours=6)
    assert r1["moments"][0].tolist() == [4, 2, 2, 0, 2, 1, 0, 2, 0, 0]
    zero = np.all(r1["normals"] == 0, axis=1)
    assert np.nonzero(zero)[0].tolist() == [0, 4, 20, 24]


def test_tilted_sheet_across_two_cubes():
    cube_ijk, lists = ref.tilted_sheet_two_cubes()
    s = ref.hand_scene(cube_ijk, lists)
    r = ref.normals_ref(*ref.scene_args(s))
    assert r["solved"].all()
    want = np.asarray([1.0, 0.0, 1.0]) / np.sqrt(2.0)
    assert np.abs(r["normals"].astype(np.float64) - want).max() <= 1e-12 + 2.0 ** -25          # float32 rounding of 1/sqrt(2) on top of the 1e-12
    # in float64, before the rounding: within 1e-12
    C = ref.scatter_matrix(r["moments"]).astype(np.float64)
    v = np.linalg.eigh(C)[1][:, :, 0]
    v = v * np.sign(v[:, 2:3])
    assert np.abs(v - want).max() <= 1e-12
    # the seam: the last voxel row of cube 0 (world x = 17) sees cube 1's cells; gathered inside its own cube alone it would count fewer
    own = ref.moments_ref(s["offsets"][:2], s["ijk"][:s["offsets"][1]], cube_ijk[:1], s["mask"][:s["offsets"][1]], 13, 2)
    last_row = np.nonzero(s["ijk"][:s["offsets"][1], 0] == 17)[0]
    assert (r["moments"][last_row, 0] > own[last_row, 0]).all()
    # unique: nothing is shared between the two cubes here
    assert ref.unique_ref(s["offsets"], s["ijk"], s["cube_ijk"], s["mask"], 13).all()


def test_unique_ref_keeps_the_first_packed_index():
    # voxel (14,3,3) of cube 0 twice, and the same world cell as (1,3,3) of cube (1,0,0)
    lists = [np.asarray([(14, 3, 3), (2, 2, 2), (14, 3, 3)], np.uint8), np.asarray([(1, 3, 3), (5, 5, 5)], np.uint8)]
    s = ref.hand_scene([[0, 0, 0], [1, 0, 0]], lists)
    assert ref.unique_ref(s["offsets"], s["ijk"], s["cube_ijk"], s["mask"], 13).tolist() == [True, True, False, False, True]
    m = s["mask"].copy()
    m[0] = False
    assert ref.unique_ref(s["offsets"], s["ijk"], s["cube_ijk"], m, 13).tolist() == [False, True, True, False, True]


def _lists():
    s = ref.surface_scene((2, 2, 1))
    return s, (s["cube_ijk"], s["lists"]["vxl_ijk_list"], s["mask_list"], s["param"], s["viewPair"], s["cameraTs"])


def test_wrapper_argument_checks_run_without_a_gpu(monkeypatch):
    from surfacenet_amd import runtime

    def no_library(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(runtime, "any_context", no_library)
    s, args = _lists()
    with pytest.raises(ValueError, match="stride"):
        normals.estimate_normals(*args, stride_vox=6.5)
    with pytest.raises(ValueError, match="stride"):
        normals.unique_voxels(*args[:3], stride_vox=0)
    with pytest.raises(ValueError, match="integer"):
        normals.stride_voxels(26, 0.3)
    assert normals.stride_voxels(26, 0.5) == 13 and normals.stride_voxels(52, 0.5) == 26
    for radius in (0, 4):
        with pytest.raises(ValueError, match="radius"):
            normals.estimate_normals(*args, stride_vox=13, radius=radius)
    mixed = s["param"].copy()
    mixed["resol"][1] = 0.8
    with pytest.raises(ValueError, match="resol"):
        normals.estimate_normals(args[0], args[1], args[2], mixed, args[4], args[5], stride_vox=13)
    with pytest.raises(ValueError, match="mask lists"):
        normals.estimate_normals(args[0], args[1], args[2][:-1], *args[3:], stride_vox=13)
    with pytest.raises(ValueError, match="mask lists"):
        normals.unique_voxels(args[0], args[1], args[2][:-1], stride_vox=13)
    short = list(args[2])
    short[0] = short[0][:-1]
    with pytest.raises(ValueError, match="mask entries"):
        normals.estimate_normals(args[0], args[1], short, *args[3:], stride_vox=13)
    with pytest.raises(ValueError, match="view-pair rows"):
        normals.estimate_normals(args[0], args[1], args[2], args[3], args[4][:-1], args[5], stride_vox=13)
    with pytest.raises(ValueError, match="integer"):
        reconstruct.scene_postpass(dict(prediction_list=[], vxl_ijk_list=[], rayPooling_votes_list=[]), 32, 26, 5, unique=True, cube_overlapping_ratio=0.3)
    # nothing to do: no library either
    assert normals.estimate_normals(np.zeros((0, 3)), [], [], s["param"][:0], s["viewPair"][:0], s["cameraTs"], 13) == []
    assert normals.unique_voxels(np.zeros((0, 3)), [], [], 13) == []


def test_scene_postpass_without_the_new_arguments_returns_todays_keys():
    empty = dict(prediction_list=[], vxl_ijk_list=[], rayPooling_votes_list=[])
    today = {"fixThresh_mask_list", "fixThresh_denoised_list", "adapt_init_denoised_list", "adapt_thresh", "adapt_mask_list", "adapt_denoised_list"}
    assert set(reconstruct.scene_postpass(empty, 32, 26, 5)) == today
    assert set(reconstruct.scene_postpass(empty, 32, 26, 5, keep_iterations=True)) == today | {"adapt_iterations"}
    assert set(reconstruct.scene_postpass(empty, 32, 26, 5, cameraTs_np=np.zeros((2, 3)))) == today | {"fixThresh_normal_list", "adapt_normal_list"}
    assert set(reconstruct.scene_postpass(empty, 32, 26, 5, unique=True)) == today | {"fixThresh_unique_list", "adapt_unique_list"}
    p = inspect.signature(reconstruct.scene_postpass).parameters
    assert p["cameraTs_np"].default is None and p["cube_overlapping_ratio"].default == 0.5 and p["unique"].default is False
