"""GPU (-m gpu): connected components of the output cloud (surfacenet_amd/csrc/components.h) through the C ABI and the drop-ins, against the
numpy restatement tests/components_ref.py. Every comparison is exact: label, cells, keep and C."""
import ctypes

import numpy as np
import pytest

import components_ref as cr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_required):
    from surfacenet_amd import runtime
    return runtime.any_context()


def _run(ctx, s, **kw):
    return ctx.components(*cr.scene_args(s), **kw)


def _check(ctx, s, **kw):
    got, want = _run(ctx, s, **kw), cr.components_ref(*cr.scene_args(s), **kw)
    cr.compare(got, want)
    return got


def _lists(s):
    cut = lambda a: [a[i:j] for i, j in zip(s["offsets"][:-1], s["offsets"][1:])]
    return cut(s["ijk"]), cut(s["mask"])


def _raw(ctx, s, connectivity=26, min_cells=1, label=None, cells=None, keep=None, offsets=None):
    """sn_components itself: any subset of the outputs, the status returned."""
    from surfacenet_amd import _lib
    offsets_, n, ijk, cube = ctx._packed(s["offsets"] if offsets is None else offsets, s["ijk"], s["cube_ijk"])
    m = np.ascontiguousarray(s["mask"], dtype=bool).view(np.uint8)
    cfg = _lib.ComponentsCfg(int(s["stride_vox"]), connectivity, min_cells)
    C = ctypes.c_longlong(-7)
    rc = ctx._lib.sn_components(ctx._h, n, ctypes.byref(cfg), _lib.ptr(offsets_), _lib.ptr(ijk), _lib.ptr(cube), _lib.ptr(m), _lib.ptr(label),
                                _lib.ptr(cells), _lib.ptr(keep), ctypes.byref(C))
    return rc, C.value


# ---- random fill -----------------------------------------------------------------------------------------------------------------------------------
def test_random_fill_at_the_three_connectivities(ctx):
    s = cr.random_cube(D=8, fill=0.3, seed=7)[0]
    counts = [_check(ctx, s, connectivity=c)[3] for c in (6, 18, 26)]
    assert len(set(counts)) == 3                              # a connectivity mix-up cannot pass


def test_min_cells_on_the_random_scene(ctx):
    s = cr.random_cube(D=8, fill=0.3, seed=7)[0]
    want = cr.components_ref(*cr.scene_args(s), connectivity=6)
    largest = int(want[1].max())
    assert np.array_equal(_check(ctx, s, connectivity=6, min_cells=1)[2], s["mask"])
    two = _check(ctx, s, connectivity=6, min_cells=2)[2]
    assert two.any() and not two.all()
    assert not _check(ctx, s, connectivity=6, min_cells=largest + 1)[2].any()
    assert _check(ctx, s, connectivity=6, min_cells=largest)[2].sum() >= largest


# ---- seams, repeats, unmasked entries, shuffled cubes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cubes", [2, 8])
@pytest.mark.parametrize("connectivity", [6, 26])
def test_sheet_across_every_seam(ctx, n_cubes, connectivity):
    s = cr.seam_scene(n_cubes)                                # shuffled cubes: the restatement runs on the shuffled input
    label, cells, keep, C = _check(ctx, s, connectivity=connectivity, min_cells=3)
    big = np.argmax(np.bincount(label[label >= 0]))
    cubes = cr.cube_of(s["offsets"])[label == big]
    assert np.unique(cubes).size == n_cubes                   # the sheet is one component through all the cubes


def test_snake_listed_backwards(ctx):
    s, length = cr.snake_scene()
    for c in (6, 26):
        label, cells, keep, C = _check(ctx, s, connectivity=c)
        assert C == 1 and (cells == length).all() and not label.any()
    # first(K) is the last cell of the path: packed index 0
    assert _run(ctx, s, min_cells=length)[2].all() and not _run(ctx, s, min_cells=length + 1)[2].any()


def test_solid_block_and_gap_plane(ctx):
    s = cr.block_scene(24)
    label, cells, keep, C = _check(ctx, s)
    assert C == 1 and (cells == 24 ** 3).all()
    for c in (6, 26):
        label, cells, keep, C = _check(ctx, cr.block_scene(24, gap=11), connectivity=c, min_cells=24 * 24 * 12)
        assert C == 2 and sorted(set(cells.tolist())) == [24 * 24 * 11, 24 * 24 * 12] and keep.sum() == 24 * 24 * 12


@pytest.mark.parametrize("count,extra", [(3000, 0), ((1 << 20), 5)])
def test_isolated_voxels_number_in_packed_order(ctx, count, extra):
    """A checkerboard at connectivity 6: every voxel its own component, so the scan numbers 0 .. count-1 - over two levels of 1024-element
    blocks at 3,000 voxels, over three at 1,048,576 + 5 (the five extra entries are unmasked)."""
    s = cr.checkerboard_scene(count, extra)
    label, cells, keep, C = _run(ctx, s, connectivity=6)
    assert C == count and np.array_equal(label[:count], np.arange(count, dtype=np.int32)) and (label[count:] == -1).all()
    assert (cells[:count] == 1).all() and not cells[count:].any() and np.array_equal(keep, s["mask"])
    cr.compare((label, cells, keep, C), cr.components_ref(*cr.scene_args(s), connectivity=6))


# ---- edges of the lattice ------------------------------------------------------------------------------------------------------------------------------
def test_lattice_edges(ctx):
    corner = np.asarray([(0, 0, 0), (1, 1, 1), (0, 1, 0), (3, 3, 3)], np.uint8)
    s = cr.scene([[0, 0, 0]], [corner], 4)                    # the neighbour probes of cell (0, 0, 0) go negative
    for c in (6, 18, 26):
        _check(ctx, s, connectivity=c)
    top = (1 << 21) - 2                                       # the last legal coordinate
    base = top - 3
    s = cr.scene([[base] * 3, [0, base, 0]], [corner, corner], 1)
    assert cr.world_cells(*cr.scene_args(s)[:3], 1).max() == top
    for c in (6, 26):
        _check(ctx, s, connectivity=c)
    # one cell further: refused, the outputs as they were
    over = cr.scene([[base] * 3], [np.asarray([(0, 0, 0), (3, 4, 3)], np.uint8)], 1)
    label, cells, keep = np.full(2, 77, np.int32), np.full(2, 77, np.int32), np.full(2, 77, np.uint8)
    rc, C = _raw(ctx, over, label=label, cells=cells, keep=keep)
    from surfacenet_amd import _lib
    assert rc == -1 and "2^21" in _lib.last_error() and C == -7
    assert (label == 77).all() and (cells == 77).all() and (keep == 77).all()
    over["mask"][1] = False                                   # the cell past the range unmasked: legal again
    _check(ctx, over)


# ---- degenerate and refused inputs -------------------------------------------------------------------------------------------------------------------
def test_degenerate_inputs(ctx):
    s = cr.seam_scene(2)
    s["mask"] = np.zeros_like(s["mask"])
    label, cells, keep, C = _check(ctx, s)
    assert C == 0 and (label == -1).all() and not cells.any() and not keep.any()
    e = cr.scene(np.zeros((0, 3)), [], 4)
    label, cells, keep, C = _run(ctx, e)
    assert C == 0 and label.shape == (0,) and cells.shape == (0,) and keep.shape == (0,)
    assert _run(ctx, e, device=True)[3] == 0
    one = cr.scene([[1, 1, 1], [2, 1, 1]], [np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.uint8)], 4)      # cubes without voxels: total == 0
    assert _run(ctx, one)[3] == 0
    a = np.asarray([(0, 0, 3), (1, 0, 3)], np.uint8)
    mid = cr.scene([[1, 1, 1], [9, 9, 9], [2, 1, 1]], [a, np.zeros((0, 3), np.uint8), a], 2)                 # an empty cube in the middle
    label, cells, keep, C = _check(ctx, mid)
    assert C == 1 and (cells == 4).all()


def test_refused_inputs(ctx):
    from surfacenet_amd import _lib
    s = cr.seam_scene(2)
    T = s["mask"].size
    for kw, text in ((dict(connectivity=8), "connectivity"), (dict(min_cells=0), "min_cells")):
        label = np.full(T, 77, np.int32)
        rc, C = _raw(ctx, s, label=label, **kw)
        assert rc == -1 and text in _lib.last_error() and C == -7 and (label == 77).all()
        with pytest.raises(_lib.SurfaceNetHipError, match=text):
            _run(ctx, s, **kw)
        with pytest.raises(_lib.SurfaceNetHipError, match=text):
            _run(ctx, s, device=True, **kw)
    with pytest.raises(_lib.SurfaceNetHipError, match="stride_vox"):
        ctx.components(s["offsets"], s["ijk"], s["cube_ijk"], s["mask"], 0)
    bad = s["offsets"].copy()
    bad[1] = bad[2] + 1                                       # a decreasing table (still ending at T)
    label = np.full(T, 77, np.int32)
    rc, C = _raw(ctx, s, label=label, offsets=bad)
    assert rc == -1 and "offsets" in _lib.last_error() and C == -7 and (label == 77).all()
    with pytest.raises(_lib.SurfaceNetHipError, match="offsets"):
        ctx.components(bad, s["ijk"], s["cube_ijk"], s["mask"], s["stride_vox"], device=True)      # the device form checks it in a kernel


# ---- forms and outputs ---------------------------------------------------------------------------------------------------------------------------------
def test_forms_outputs_and_repeatability(ctx):
    s = cr.seam_scene(8)
    a = _check(ctx, s, min_cells=4)
    b = _run(ctx, s, min_cells=4)
    d = _run(ctx, s, min_cells=4, device=True)
    for x, y, z in zip(a[:3], b[:3], d[:3]):
        assert x.tobytes() == y.tobytes() == z.tobytes()       # two runs, and sn_components_dev = sn_components, bit for bit
    assert a[3] == b[3] == d[3]
    T = s["mask"].size
    for name, dt, want in (("label", np.int32, a[0]), ("cells", np.int32, a[1]), ("keep", np.uint8, a[2].view(np.uint8))):
        out = np.full(T, 99, dt)
        rc, C = _raw(ctx, s, min_cells=4, **{name: out})       # each output alone
        assert rc == 0 and C == a[3] and np.array_equal(out, want), name
    assert _raw(ctx, s) == (0, a[3])                           # no output array at all: C alone
    big = cr.block_scene(24)
    _check(ctx, big)                                           # the workspace grows
    cr.compare(_run(ctx, s, min_cells=4), a)                   # ... and is reused


# ---- drop-ins --------------------------------------------------------------------------------------------------------------------------------------------
def test_list_drop_ins(ctx):
    from surfacenet_amd import components
    s = cr.seam_scene(8)
    ijk_l, mask_l = _lists(s)
    want = cr.components_ref(*cr.scene_args(s), connectivity=18)
    sizes_want = cr.sizes_of(want[0], want[1], want[3])
    label_l, sizes = components.label_components(s["cube_ijk"], ijk_l, mask_l, 4, connectivity=18)
    assert sizes.dtype == np.int32 and np.array_equal(sizes, sizes_want)
    assert len(label_l) == len(ijk_l) and all(a.dtype == np.int32 for a in label_l) and np.array_equal(np.concatenate(label_l), want[0])
    cut = lambda flat: [flat[i:j] for i, j in zip(s["offsets"][:-1], s["offsets"][1:])]
    same = lambda got, flat: len(got) == len(ijk_l) and all(g.dtype == np.bool_ and np.array_equal(g, w) for g, w in zip(got, cut(flat)))
    k3 = cr.components_ref(*cr.scene_args(s), connectivity=18, min_cells=3)[2]
    assert same(components.remove_floaters(s["cube_ijk"], ijk_l, mask_l, 4, min_cells=3, connectivity=18), k3)
    top = components.kept_components(sizes_want, keep_largest=2)
    assert same(components.remove_floaters(s["cube_ijk"], ijk_l, mask_l, 4, keep_largest=2, connectivity=18), (want[0] >= 0) & top[np.maximum(want[0], 0)])
    both = components.kept_components(sizes_want, min_cells=3, keep_largest=4)
    assert same(components.remove_floaters(s["cube_ijk"], ijk_l, mask_l, 4, min_cells=3, keep_largest=4, connectivity=18),
                (want[0] >= 0) & both[np.maximum(want[0], 0)])


def _with_seam_floater(s, D_cube=32):
    """The lists of normals_ref.surface_scene((2, 2, 1)) plus a floater that denoise_crossCubes keeps: one voxel v in cube (0,0,0) and one voxel
    u = v - (D_cube // 2, 0, 0) in cube (1,0,0) - the reference's coincidence rule between neighbour cubes - each at least three cells away from
    every listed voxel. On the world lattice (stride 13) they are two single cells three apart. -> (lists, [(cube, position), ...])."""
    import normals_ref as nref
    d = s["lists"]
    cube_ijk = np.asarray(d["cube_ijk_np"])
    c0, c1 = [int(np.nonzero((cube_ijk == c).all(1))[0][0]) for c in ((0, 0, 0), (1, 0, 0))]
    off, ijk = nref.pack(d["vxl_ijk_list"])
    g = nref.world_cells(off, ijk, cube_ijk, 13)
    near = np.zeros((39 + 6, 39 + 6, 26 + 6), bool)               # index = cell + 3
    for dx in range(7):
        for dy in range(7):
            for dz in range(7):
                near[g[:, 0] + dx, g[:, 1] + dy, g[:, 2] + dz] = True      # within 3 cells of a listed voxel
    h, shift = D_cube // 2, D_cube // 2 - 13
    free = ~near[3:-3, 3:-3, 3:-3]
    both = free[h:26, :13, :] & free[h - shift:26 - shift, :13, :]      # v in cube (0,0,0) alone (y < 13), its partner's world cell v - shift
    v = np.stack(np.nonzero(both), 1)[0] + (h, 0, 0)
    lists = {k: list(d[k]) for k in ("prediction_list", "rgb_list", "vxl_ijk_list", "rayPooling_votes_list")}
    where = []
    for c, local in ((c0, v), (c1, v - (h, 0, 0))):
        where.append((c, len(lists["vxl_ijk_list"][c])))
        lists["vxl_ijk_list"][c] = np.concatenate([lists["vxl_ijk_list"][c], np.asarray([local], np.uint8)])
        lists["prediction_list"][c] = np.concatenate([lists["prediction_list"][c], np.asarray([1.0], np.float16)])
        lists["rayPooling_votes_list"][c] = np.concatenate([lists["rayPooling_votes_list"][c], np.asarray([255], np.uint8)])
        lists["rgb_list"][c] = np.concatenate([lists["rgb_list"][c], np.zeros((1, 3), np.uint8)])
    return lists, where


def test_scene_postpass_removes_floaters_before_the_extras(ctx):
    import normals_ref as nref
    from surfacenet_amd import components, mesh, normals, reconstruct
    s = nref.surface_scene((2, 2, 1))
    d, floater = _with_seam_floater(s)
    cube_ijk, ijk_l = s["lists"]["cube_ijk_np"], d["vxl_ijk_list"]
    out = dict(prediction_list=d["prediction_list"], vxl_ijk_list=ijk_l, rayPooling_votes_list=d["rayPooling_votes_list"],
               cube_ijk_np=cube_ijk, param_np=s["param"], viewPair_np=s["viewPair"], rgb_list=d["rgb_list"])
    kw = dict(tau=0.7, gamma=0.5, N_refine_iter=2)
    k = 10
    plain = reconstruct.scene_postpass(out, 32, 26, 2, **kw)
    assert set(plain) == {"fixThresh_mask_list", "fixThresh_denoised_list", "adapt_init_denoised_list", "adapt_thresh", "adapt_mask_list",
                          "adapt_denoised_list"}                # exactly the keys of a call without the argument
    post = reconstruct.scene_postpass(out, 32, 26, 2, min_component=k, cameraTs_np=s["cameraTs"], unique=True, mesh=True, **kw)
    assert set(post) - set(plain) == {"fixThresh_clean_list", "adapt_clean_list", "fixThresh_normal_list", "adapt_normal_list", "fixThresh_unique_list",
                                      "adapt_unique_list", "fixThresh_mesh", "adapt_mesh"}
    for key in plain:
        same = np.array_equal(post[key], plain[key]) if isinstance(plain[key], np.ndarray) else all(np.array_equal(a, b) for a, b in zip(post[key], plain[key]))
        assert same, key                                        # what was there stays as it was, the denoised lists included
    # the per-cube denoising keeps the floater (it coincides with a neighbour cube's voxel), the scene-wide components drop it
    for c, i in floater:
        assert post["fixThresh_denoised_list"][c][i] and not post["fixThresh_clean_list"][c][i]
    off, ijk = nref.pack(ijk_l)
    for name in ("fixThresh", "adapt"):
        den, clean = post[name + "_denoised_list"], post[name + "_clean_list"]
        want = components.remove_floaters(cube_ijk, ijk_l, den, 13, min_cells=k)
        assert all(a.dtype == np.bool_ and np.array_equal(a, b) for a, b in zip(clean, want))
        assert np.array_equal(np.concatenate(clean), cr.components_ref(off, ijk, cube_ijk, np.concatenate(den), 13, min_cells=k)[2])
        nl = post[name + "_normal_list"]
        assert not np.concatenate(nl)[~np.concatenate(clean)].any()                                  # no normal on a removed voxel
        assert all(np.array_equal(a, b) for a, b in zip(nl, normals.estimate_normals(cube_ijk, ijk_l, clean, s["param"], s["viewPair"], s["cameraTs"], 13)))
        assert all(np.array_equal(a, b) for a, b in zip(post[name + "_unique_list"], normals.unique_voxels(cube_ijk, ijk_l, clean, 13)))
        want_mesh = mesh.extract_mesh(cube_ijk, ijk_l, clean, nl, s["param"], 13)
        for key in want_mesh:
            assert np.array_equal(post[name + "_mesh"][key], want_mesh[key]), (name, key)
        print("%s: min_component = %d removes %d of %d voxels" % (name, k, int(np.concatenate(den).sum() - np.concatenate(clean).sum()), int(np.concatenate(den).sum())))
