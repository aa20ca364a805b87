"""No GPU: the numpy restatement of the connected components (tests/components_ref.py) against scipy.ndimage.label on
the dense array, the planted faults the comparison helper of the GPU tests must catch, and the host logic and argument checks of
surfacenet_amd.components - all of which run before the library is touched."""
import inspect

import numpy as np
import pytest

import components_ref as cr
from surfacenet_amd import components, reconstruct

CONNECTIVITIES = ((6, 1), (18, 2), (26, 3))


def _dense_labels(s, rank):
    """scipy's labels of the scene's masked world cells, per voxel (-1 unmasked)."""
    ndi = pytest.importorskip("scipy.ndimage")
    g = cr.world_cells(*cr.scene_args(s)[:3], s["stride_vox"])
    vol = np.zeros(tuple(g.max(0) + 1), bool)
    gm = g[s["mask"]]
    vol[gm[:, 0], gm[:, 1], gm[:, 2]] = True
    lab, count = ndi.label(vol, structure=ndi.generate_binary_structure(3, rank))
    per_voxel = np.where(s["mask"], lab[g[:, 0], g[:, 1], g[:, 2]] - 1, -1)
    return per_voxel, count, np.bincount(lab[vol] - 1, minlength=count)


def _check_numbering(s, label, cells, C):
    """Components are numbered by ascending first packed index; cells counts distinct cells."""
    idx = np.nonzero(label >= 0)[0]
    firsts = np.full((C,), label.size, np.int64)
    np.minimum.at(firsts, label[idx], idx)
    assert (np.diff(firsts) > 0).all() and (C == 0 or firsts[0] == idx[0])
    keys = cr.cell_keys(cr.world_cells(*cr.scene_args(s)[:3], s["stride_vox"]))
    distinct = np.unique(np.stack([label[idx], keys[idx]], 1), axis=0)
    assert np.array_equal(cr.sizes_of(label, cells, C), np.bincount(distinct[:, 0], minlength=C))
    assert not cells[label < 0].any()


@pytest.mark.parametrize("connectivity,rank", CONNECTIVITIES)
@pytest.mark.parametrize("which", ["random", "seam2"])
def test_restatement_equals_scipy_label(which, connectivity, rank):
    s = cr.random_cube(seed=7)[0] if which == "random" else cr.seam_scene(2)
    label, cells, keep, C = cr.components_ref(*cr.scene_args(s), connectivity=connectivity)
    want, count, sizes = _dense_labels(s, rank)
    assert C == count
    assert cr.same_partition(label, want)
    assert sorted(cr.sizes_of(label, cells, C)) == sorted(sizes)
    _check_numbering(s, label, cells, C)
    assert np.array_equal(keep, s["mask"])


def test_random_scene_separates_the_three_connectivities():
    s = cr.random_cube(seed=7)[0]
    counts = [cr.components_ref(*cr.scene_args(s), connectivity=c)[3] for c in (6, 18, 26)]
    assert counts[0] > counts[1] > counts[2] >= 1


def test_hand_made_cases():
    # two cells that touch by a corner only, listed twice, the second copy first
    s = cr.scene([[0, 0, 0]], [np.asarray([(1, 1, 1), (0, 0, 0), (1, 1, 1), (5, 5, 5)], np.uint8)], 8)
    for c, want in ((6, [0, 1, 0, 2]), (18, [0, 1, 0, 2]), (26, [0, 0, 0, 1])):
        label, cells, keep, C = cr.components_ref(*cr.scene_args(s), connectivity=c)
        assert label.tolist() == want and C == max(want) + 1
    assert cells.tolist() == [2, 2, 2, 1]            # the repeated cell counts once
    s["mask"][1] = False
    label, cells, keep, C = cr.components_ref(*cr.scene_args(s), connectivity=26, min_cells=2)
    assert label.tolist() == [0, -1, 0, 1] and cells.tolist() == [1, 0, 1, 1] and not keep.any() and C == 2
    # empty inputs
    e = cr.scene(np.zeros((0, 3)), [], 4)
    assert cr.components_ref(*cr.scene_args(e))[3] == 0
    s["mask"][:] = False
    label, cells, keep, C = cr.components_ref(*cr.scene_args(s))
    assert (label == -1).all() and not cells.any() and not keep.any() and C == 0
    # the snake: one component named by the last cell of the path
    snake, length = cr.snake_scene()
    label, cells, keep, C = cr.components_ref(*cr.scene_args(snake), connectivity=6)
    assert 3500 <= length <= 4500 and C == 1 and (cells == length).all() and not label.any()


# ---- planted faults: each must fail the comparison helper the GPU tests use ---------------------------------------------------------------------
def _fails(got, want):
    with pytest.raises(AssertionError):
        cr.compare(got, want)


def test_compare_accepts_the_restatement_itself():
    s = cr.seam_scene(8)
    cr.compare(cr.components_ref(*cr.scene_args(s)), cr.components_ref(*cr.scene_args(s)))


def test_planted_connectivity_18_computed_as_26():
    s = cr.random_cube(seed=7)[0]
    _fails(cr.components_ref(*cr.scene_args(s), connectivity=26), cr.components_ref(*cr.scene_args(s), connectivity=18))


def test_planted_component_not_joined_across_a_seam():
    s = cr.seam_scene(2)
    apart = dict(s, cube_ijk=s["cube_ijk"] * 100)    # the cubes moved apart: every cube labelled on its own
    _fails(cr.components_ref(*cr.scene_args(apart)), cr.components_ref(*cr.scene_args(s)))


def test_planted_shared_cell_counted_twice():
    s = cr.seam_scene(8)
    label, cells, keep, C = cr.components_ref(*cr.scene_args(s))
    per_voxel = np.bincount(label[label >= 0], minlength=C).astype(np.int32)      # masked voxels, not distinct cells
    twice = np.where(label >= 0, per_voxel[np.maximum(label, 0)], 0).astype(np.int32)
    _fails((label, twice, keep, C), (label, cells, keep, C))


def test_planted_numbering_by_cell_key():
    s = cr.seam_scene(8)
    label, cells, keep, C = cr.components_ref(*cr.scene_args(s))
    keys = cr.cell_keys(cr.world_cells(*cr.scene_args(s)[:3], s["stride_vox"]))
    low = np.full((C,), np.iinfo(np.int64).max)
    m = label >= 0
    np.minimum.at(low, label[m], keys[m])
    renum = np.empty((C,), np.int32)
    renum[np.argsort(low)] = np.arange(C, dtype=np.int32)
    by_key = np.where(m, renum[np.maximum(label, 0)], -1).astype(np.int32)
    assert cr.same_partition(by_key, label)
    _fails((by_key, cells, keep, C), (label, cells, keep, C))


def test_planted_keep_as_strictly_greater():
    s = cr.random_cube(seed=7)[0]
    label, cells, keep, C = cr.components_ref(*cr.scene_args(s), connectivity=6, min_cells=2)
    assert (cells == 2).any()
    _fails((label, cells, s["mask"] & (cells > 2), C), (label, cells, keep, C))


# ---- host logic of the drop-ins ---------------------------------------------------------------------------------------------------------------------
def test_kept_components_ties_and_both_conditions():
    sizes = np.asarray([5, 9, 5, 1, 9, 5], np.int32)
    kept = lambda **kw: np.nonzero(components.kept_components(sizes, **kw))[0].tolist()
    assert kept(min_cells=5) == [0, 1, 2, 4, 5]
    assert kept(keep_largest=1) == [1]               # ties go to the lower number
    assert kept(keep_largest=3) == [0, 1, 4]
    assert kept(keep_largest=4) == [0, 1, 2, 4]
    assert kept(keep_largest=100) == [0, 1, 2, 3, 4, 5]
    assert kept(min_cells=6, keep_largest=4) == [1, 4]
    assert kept(min_cells=10, keep_largest=2) == []
    assert components.kept_components(np.zeros((0,), np.int32), keep_largest=2).size == 0


def test_argument_checks_run_before_the_library(monkeypatch):
    from surfacenet_amd import runtime

    def no_library(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(runtime, "any_context", no_library)
    s = cr.seam_scene(2)
    lists = [s["ijk"][a:b] for a, b in zip(s["offsets"][:-1], s["offsets"][1:])]
    masks = [s["mask"][a:b] for a, b in zip(s["offsets"][:-1], s["offsets"][1:])]
    with pytest.raises(ValueError, match="min_cells, keep_largest or both"):
        components.remove_floaters(s["cube_ijk"], lists, masks, 4)
    for kw in (dict(min_cells=0), dict(min_cells=2.5), dict(keep_largest=0), dict(min_cells=True)):
        with pytest.raises(ValueError, match="positive integer"):
            components.remove_floaters(s["cube_ijk"], lists, masks, 4, **kw)
    with pytest.raises(ValueError, match="connectivity"):
        components.remove_floaters(s["cube_ijk"], lists, masks, 4, min_cells=2, connectivity=8)
    with pytest.raises(ValueError, match="connectivity"):
        components.label_components(s["cube_ijk"], lists, masks, 4, connectivity=4)
    with pytest.raises(ValueError, match="stride_vox"):
        components.label_components(s["cube_ijk"], lists, masks, 0)
    with pytest.raises(ValueError, match="mask lists"):
        components.label_components(s["cube_ijk"], lists, masks[:-1], 4)
    with pytest.raises(ValueError, match="mask entries"):
        components.remove_floaters(s["cube_ijk"], lists, [masks[0][:-1]] + masks[1:], 4, min_cells=2)
    # nothing to do: no library either
    label_list, sizes = components.label_components(np.zeros((0, 3)), [], [], 4)
    assert label_list == [] and sizes.shape == (0,) and sizes.dtype == np.int32
    assert components.remove_floaters(np.zeros((0, 3)), [], [], 4, keep_largest=1) == []
    # scene_postpass: every check of the new arguments fails before any stage runs
    empty = dict(prediction_list=[], vxl_ijk_list=[], rayPooling_votes_list=[])
    with pytest.raises(ValueError, match="positive integer"):
        reconstruct.scene_postpass(empty, 32, 26, 5, min_component=0)
    with pytest.raises(ValueError, match="connectivity"):
        reconstruct.scene_postpass(empty, 32, 26, 5, min_component=10, component_connectivity=27)
    with pytest.raises(ValueError, match="integer"):
        reconstruct.scene_postpass(empty, 32, 26, 5, min_component=10, cube_overlapping_ratio=0.3)


def test_scene_postpass_keys_with_and_without_min_component():
    empty = dict(prediction_list=[], vxl_ijk_list=[], rayPooling_votes_list=[])
    today = {"fixThresh_mask_list", "fixThresh_denoised_list", "adapt_init_denoised_list", "adapt_thresh", "adapt_mask_list", "adapt_denoised_list"}
    assert set(reconstruct.scene_postpass(empty, 32, 26, 5)) == today
    assert set(reconstruct.scene_postpass(empty, 32, 26, 5, min_component=10)) == today | {"fixThresh_clean_list", "adapt_clean_list"}
    p = inspect.signature(reconstruct.scene_postpass).parameters
    assert p["min_component"].default is None and p["component_connectivity"].default == 26
