"""GPU (-m gpu): the cross-cube post-pass (surfacenet_amd/csrc/crosscube.h) through the drop-ins denoising.denoise_crossCubes and
adapthresh.adapthresh and the in-memory reconstruct.scene_postpass: bit-identical to the goldens recorded from the reference
(tests/golden/postpass_cases.npz, postpass_edge_cases.npz), to the CPU restatement (tests/postpass_ref.py) at scale and at every cube width
where the kernels take another path (tests/postpass_cases.py), and to the drop-ins called one by one."""
import os

import numpy as np
import pytest

import postpass_cases as cases
import postpass_ref as ref

pytestmark = pytest.mark.gpu
DN, AT = ref.load_cases()


@pytest.fixture(scope="module")
def sn(gpu_required):
    from surfacenet_amd import adapthresh, denoising, runtime, sparseCubes
    return dict(adapthresh=adapthresh, denoising=denoising, runtime=runtime, sparseCubes=sparseCubes)


def _same_lists(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == bool and a.shape == b.shape and np.array_equal(a, b), i


@pytest.mark.parametrize("name", sorted(DN))
def test_denoise_bit_identical_to_reference(sn, name):
    c = DN[name]
    got = sn["denoising"].denoise_crossCubes(c["cube_ijk"], c["ijk_list"], c["mask_list"], D_cube=c["D_cube"])
    _same_lists(got, c["out_list"])


def _at_lists(sn, c, keep=("thresh", "masks", "denoised", "choice")):
    return sn["adapthresh"].adapthresh_lists(c["pred_list"], c["ijk_list"], c["votes_list"], c["cube_ijk"], c["N_refine_iter"], c["D_cube"],
                                             c["init_probThresh"], c["max_probThresh"], c["rayPool_thresh"], c["beta"], keep=keep)


@pytest.mark.parametrize("name", sorted(AT))
def test_adapthresh_every_iteration_bit_identical_to_reference(sn, name):
    c = AT[name]
    r = _at_lists(sn, c)
    assert np.array_equal(r["init_denoised"], c["init_denoised"])
    assert r["thresh"].dtype == np.float64 and np.array_equal(r["thresh"], c["thresh"])          # exact float64 thresholds
    assert np.array_equal(r["choice"], c["choice"])
    assert np.array_equal(r["masks"], c["masks"]) and np.array_equal(r["denoised"], c["denoised"])


def _expected_ply(sn, path, masks_flat, c, rgb):
    sn["sparseCubes"].save_sparseCubes_2ply(ref.split(masks_flat, c["offsets"]), c["ijk_list"], rgb, c["param"], ply_filePath=path)
    return open(path, "rb").read()


@pytest.mark.parametrize("name", ["s32", "s64"])
def test_adapthresh_dropin_files_and_return_value(sn, tmp_path, name):
    c = AT[name]
    rs = np.random.RandomState(5)
    rgb = [rs.randint(0, 255, (len(a), 3)).astype(np.uint8) for a in c["ijk_list"]]
    npz = str(tmp_path / "model.npz")
    sn["sparseCubes"].save_sparseCubes(npz, c["pred_list"], rgb, c["ijk_list"], c["votes_list"], c["cube_ijk"], c["param"],
                                       np.zeros((len(rgb), 1, 2), np.uint16))
    N = c["N_refine_iter"]
    last = sn["adapthresh"].adapthresh(str(tmp_path), N, c["D_cube"], c["init_probThresh"], c["min_probThresh"], c["max_probThresh"],
                                       c["rayPool_thresh"], c["beta"], c["gamma"], npz, RGB_visual_ply=True)
    fld = os.path.join(str(tmp_path), "adapThresh_gamma{:.3}_beta{}".format(c["gamma"], c["beta"]))
    assert last == os.path.join(fld, "iter%d.ply" % (N - 1))
    want = ["initialization.ply"] + ["iter%d.ply" % k for k in range(N)] + ["iter%d_tmprgb4debug.ply" % k for k in range(N)]
    assert sorted(os.listdir(fld)) == sorted(want)
    scratch = str(tmp_path / "expected.ply")
    assert open(os.path.join(fld, "initialization.ply"), "rb").read() == _expected_ply(sn, scratch, c["init_denoised"], c, rgb)
    for k in range(N):
        assert open(os.path.join(fld, "iter%d.ply" % k), "rb").read() == _expected_ply(sn, scratch, c["denoised"][k], c, rgb), k
        tmp_rgb = [r.copy() for r in rgb]
        for i in np.nonzero(c["choice"][k] >= 0)[0]:
            tmp_rgb[i][:, c["choice"][k][i]] = 255
        assert open(os.path.join(fld, "iter%d_tmprgb4debug.ply" % k), "rb").read() == _expected_ply(sn, scratch, c["masks"][k], c, tmp_rgb), k


def test_bad_arguments_are_rejected(sn):
    import surfacenet_amd
    ctx = sn["runtime"].any_context()
    c = DN["doc_denoise"]
    off = c["offsets"]
    ijk = np.concatenate(c["ijk_list"])
    mask = np.concatenate(c["mask_list"])
    with pytest.raises(surfacenet_amd.SurfaceNetHipError, match="Dc"):
        ctx.denoise(off, ijk, c["cube_ijk"], mask, 4, 65)
    with pytest.raises(surfacenet_amd.SurfaceNetHipError, match="D_cube"):
        ctx.denoise(off, ijk, c["cube_ijk"], mask, 1, 4)
    bad = off.copy()
    bad[2] = bad[3] + 1
    with pytest.raises(surfacenet_amd.SurfaceNetHipError, match="offsets"):
        ctx.denoise(bad, ijk, c["cube_ijk"], mask, 4, 4)
    with pytest.raises(surfacenet_amd.SurfaceNetHipError, match="Dc"):
        ctx.denoise(off, ijk, c["cube_ijk"], mask, 4, 3)            # an ijk of 3 in a 3-wide cube
    with pytest.raises(surfacenet_amd.SurfaceNetHipError, match="Dc"):
        ctx.adapthresh(off, ijk, np.ones(len(ijk), np.float16), None, c["cube_ijk"], 4, 1, 0.5, 0.9, 0, 6, 65)
    assert np.array_equal(ctx.denoise(off, ijk, c["cube_ijk"], mask, 4, 4), np.concatenate(c["out_list"]))       # the context still works


def test_dev_entries_equal_host_entries(sn):
    """sn_denoise_dev / sn_adapthresh_dev on device arrays give the host forms' results; a bad offsets table reaches sn_synchronize"""
    import ctypes
    from surfacenet_amd import _lib
    ctx = sn["runtime"].any_context()
    c = AT["s32"]
    off, ijk = c["offsets"], np.concatenate(c["ijk_list"])
    p16, votes = np.concatenate(c["pred_list"]).view(np.uint16), np.concatenate(c["votes_list"])
    T, n, N = ijk.shape[0], len(c["ijk_list"]), c["N_refine_iter"]
    host = _at_lists(sn, c)
    bufs = []

    def up(a):
        a = np.ascontiguousarray(a)
        p = ctx.dev_alloc(max(a.nbytes, 1))
        bufs.append(p)
        ctx.h2d(p, a)
        return p

    def alloc(nbytes):
        p = ctx.dev_alloc(nbytes)
        bufs.append(p)
        return p
    try:
        d_off, d_ijk, d_p, d_v, d_cube = up(off), up(ijk), up(p16), up(votes), up(c["cube_ijk"].astype(np.uint32))
        d_init, d_thr, d_m, d_den, d_ch = alloc(T), alloc(8 * N * n), alloc(N * T), alloc(N * T), alloc(N * n)
        cfg = _lib.AdapthreshCfg(N, c["D_cube"], c["init_probThresh"], c["max_probThresh"], float(c["rayPool_thresh"]), float(c["beta"]))
        _lib.check(ctx._lib.sn_adapthresh_dev(ctx._h, n, 26, ctypes.byref(cfg), T, d_off, d_ijk, d_p, d_v, d_cube, d_init, d_thr, d_m, d_den, d_ch))
        ctx.synchronize()
        got = dict(init_denoised=np.empty(T, np.uint8), thresh=np.empty((N, n)), masks=np.empty((N, T), np.uint8), denoised=np.empty((N, T), np.uint8),
                   choice=np.empty((N, n), np.int8))
        for k, p in (("init_denoised", d_init), ("thresh", d_thr), ("masks", d_m), ("denoised", d_den), ("choice", d_ch)):
            ctx.d2h(got[k], p)
            assert np.array_equal(got[k].view(host[k].dtype) if host[k].dtype == bool else got[k], host[k]), k
        d_mask, d_out = up(host["masks"][0].view(np.uint8)), alloc(T)
        _lib.check(ctx._lib.sn_denoise_dev(ctx._h, n, 26, c["D_cube"], T, d_off, d_ijk, d_cube, d_mask, d_out))
        out = np.empty(T, np.uint8)
        ctx.d2h(out, d_out)
        assert np.array_equal(out.view(bool), host["denoised"][0])
        bad = off.copy()
        bad[-1] += 1                                                  # the table promises one voxel more than `total`
        d_bad = up(bad)
        _lib.check(ctx._lib.sn_denoise_dev(ctx._h, n, 26, c["D_cube"], T, d_bad, d_ijk, d_cube, d_mask, d_out))
        with pytest.raises(_lib.SurfaceNetHipError, match="offsets table"):
            ctx.synchronize()
        ctx.synchronize()                                             # reported once
    finally:
        for p in bufs:
            ctx.dev_free(p)


@pytest.mark.parametrize("Dc,cube_D,lattice", [(26, 32, (16, 16, 8)), (52, 64, (6, 6, 3))])
def test_scale_against_restatement(sn, Dc, cube_D, lattice):
    """>= 2,000 cubes (s = 32) against the CPU restatement: denoise with D_cube = Dc and cube_D, two adapthresh iterations"""
    from surfacenet_amd import synthetic
    d = synthetic.sparse_surface(lattice, Dc, thickness=3, amplitude=10.0, seed=11)
    n = len(d["vxl_ijk_list"])
    assert n >= (2000 if Dc == 26 else 100)
    masks = [(p >= 0.7) & (v >= 4) for p, v in zip(d["prediction_list"], d["rayPooling_votes_list"])]
    for D in (Dc, cube_D):
        got = sn["denoising"].denoise_crossCubes(d["cube_ijk_np"], d["vxl_ijk_list"], masks, D)
        _same_lists(got, ref.denoise_ref(d["cube_ijk_np"], d["vxl_ijk_list"], masks, D))
    args = (d["prediction_list"], d["vxl_ijk_list"], d["rayPooling_votes_list"], d["cube_ijk_np"], 2, Dc, 0.5, 0.9, 4, 2)
    got, want = sn["adapthresh"].adapthresh_lists(*args), ref.adapthresh_ref(*args)
    assert np.array_equal(got["thresh"], want["thresh"]) and np.array_equal(got["choice"], want["choice"])
    assert (want["choice"] == 1).any() and (Dc != 26 or (want["choice"] == 0).any())
    for k in range(2):
        assert np.array_equal(got["masks"][k], np.concatenate(want["masks"][k]))
        assert np.array_equal(got["denoised"][k], np.concatenate(want["denoised"][k]))


def test_scene_postpass_equals_dropins_one_by_one(sn, tmp_path):
    """reconstruct.scene_postpass on a small reconstruct_scene output = main_reconstruct.py:172-176 and main.py:37-43 written out with the
    drop-ins (fixed-threshold denoise; npz; adapthresh through its files)"""
    import test_gpu_pipeline as P
    from surfacenet_amd import reconstruct
    inp = P._pipeline_inputs()
    inp["cubes"]["ijk"] = np.stack(np.meshgrid(np.arange(3), np.arange(2), np.arange(2), indexing="ij"), -1).reshape(-1, 3)   # neighbours
    out = P._run_scene(inp, sharded=False)
    cube_D, Dc, N_vp, tau, gamma, beta, N = inp["cube_D"], inp["Dc"], inp["N_vp"], 0.6, 0.5, 6, 3
    assert sum(len(a) for a in out["vxl_ijk_list"]) > 0
    post = reconstruct.scene_postpass(out, cube_D, Dc, N_vp, tau=tau, gamma=gamma, beta=beta, N_refine_iter=N, keep_iterations=True)
    sc, dn, at = sn["sparseCubes"], sn["denoising"], sn["adapthresh"]
    # main_reconstruct.py:172-176
    m = sc.filter_voxels(vxl_mask_list=[], prediction_list=out["prediction_list"], prob_thresh=tau, rayPooling_votes_list=out["rayPooling_votes_list"],
                         rayPool_thresh=gamma * N_vp * 2)
    _same_lists(post["fixThresh_mask_list"], m)
    _same_lists(post["fixThresh_denoised_list"], dn.denoise_crossCubes(out["cube_ijk_np"], out["vxl_ijk_list"], vxl_mask_list=m, D_cube=cube_D))
    npz = str(tmp_path / "model.npz")
    sc.save_sparseCubes(npz, out["prediction_list"], out["rgb_list"], out["vxl_ijk_list"], out["rayPooling_votes_list"], out["cube_ijk_np"],
                        out["param_np"], out["viewPair_np"])
    # main.py:37-43
    kwargs = {'init_probThresh': 0.5, 'min_probThresh': 0.5, 'max_probThresh': 0.9, 'D_cube': Dc, 'N_refine_iter': N, 'save_result_fld': str(tmp_path),
              'rayPool_thresh': int(round(gamma * N_vp * 2)), 'beta': beta, 'gamma': gamma, 'RGB_visual_ply': False, 'npz_file': npz}
    last = at.adapthresh(**kwargs)
    fld = os.path.dirname(last)
    scratch = str(tmp_path / "expected.ply")

    def ply(masks):
        sc.save_sparseCubes_2ply(masks, out["vxl_ijk_list"], out["rgb_list"], out["param_np"], ply_filePath=scratch)
        return open(scratch, "rb").read()
    assert open(os.path.join(fld, "initialization.ply"), "rb").read() == ply(post["adapt_init_denoised_list"])
    for k in range(N):
        assert open(os.path.join(fld, "iter%d.ply" % k), "rb").read() == ply(post["adapt_iterations"]["denoised_lists"][k]), k
    _same_lists(post["adapt_denoised_list"], post["adapt_iterations"]["denoised_lists"][-1])
    _same_lists(post["adapt_mask_list"], post["adapt_iterations"]["mask_lists"][-1])
    assert np.array_equal(post["adapt_thresh"], post["adapt_iterations"]["thresh"][-1])
    sn["runtime"].reset()


# ---- the kernel paths that depend on the cube width Dc, and D_cube != Dc (tests/postpass_cases.py) ------------------------------------------
def _check_case(sn, c):
    """denoise at the case's D_cube and every result of adapthresh against the restatement, np.array_equal throughout"""
    d = c["d"]
    got = sn["denoising"].denoise_crossCubes(d["cube_ijk_np"], d["vxl_ijk_list"], c["masks"], c["D_cube"])
    assert cases.list_differences(got, c["dn_ref"]) == []
    r = sn["adapthresh"].adapthresh_lists(*cases.at_args(d, c["D_cube"]))
    assert cases.adapthresh_differences(r, cases.packed(c["at_ref"])) == []


@pytest.mark.parametrize("name", sorted(cases.TABLE))
def test_edge_case_equals_restatement(sn, name):
    c = cases.case(name)
    assert sn["denoising"].pack_lists(c["d"]["vxl_ijk_list"])[2] == c["Dc"]
    _check_case(sn, c)


@pytest.mark.parametrize("name", ["w53", "w64"])
def test_grid_passes_change_within_one_context(sn, name):
    """two and three passes of cc_grid_kernel before and after a one-pass call (Dc = 26) in the same context: the work buffers are carved anew"""
    c, small = cases.case(name), AT["s32"]
    _check_case(sn, c)
    r = _at_lists(sn, small)
    assert np.array_equal(r["thresh"], small["thresh"]) and np.array_equal(r["masks"], small["masks"]) and np.array_equal(r["denoised"], small["denoised"])
    _check_case(sn, c)


def test_many_cubes_second_cube_per_workgroup(sn):
    """577 cubes on 512 workgroups of cc_denoise_global_kernel, unmapped cubes on either trip; the same bytes from a second call"""
    c = cases.many_cubes()
    d = c["d"]
    want = ref.denoise_ref(d["cube_ijk_np"], d["vxl_ijk_list"], c["masks"], c["D_cube"])
    got = sn["denoising"].denoise_crossCubes(d["cube_ijk_np"], d["vxl_ijk_list"], c["masks"], c["D_cube"])
    assert cases.list_differences(got, want) == []
    assert np.concatenate(want).any() and not any(want[e].any() for e in c["emptied"] + (c["repeated"],))
    again = sn["denoising"].denoise_crossCubes(d["cube_ijk_np"], d["vxl_ijk_list"], c["masks"], c["D_cube"])
    assert np.concatenate(again).tobytes() == np.concatenate(got).tobytes()


def test_extreme_cube_ijk_does_not_wrap(sn):
    c = cases.extreme_ijk()
    d = c["d"]
    got = sn["denoising"].denoise_crossCubes(d["cube_ijk_np"], d["vxl_ijk_list"], c["masks"], c["D_cube"])
    assert cases.list_differences(got, ref.denoise_ref(d["cube_ijk_np"], d["vxl_ijk_list"], c["masks"], c["D_cube"])) == []
    args = cases.at_args(d, c["D_cube"], 1)
    assert cases.adapthresh_differences(sn["adapthresh"].adapthresh_lists(*args), cases.packed(ref.adapthresh_ref(*args))) == []


def test_w64_dev_entries_equal_host_entries(sn):
    """sn_adapthresh_dev / sn_denoise_dev at Dc = 64 (three grid passes, bit 63) on device arrays give the host forms' results"""
    import ctypes
    from surfacenet_amd import _lib
    ctx = sn["runtime"].any_context()
    c = cases.case("w64")
    d = c["d"]
    host = sn["adapthresh"].adapthresh_lists(*cases.at_args(d, c["D_cube"]))
    assert cases.adapthresh_differences(host, cases.packed(c["at_ref"])) == []
    off, ijk, Dc = sn["denoising"].pack_lists(d["vxl_ijk_list"])
    p16, votes = np.concatenate(d["prediction_list"]).view(np.uint16), np.concatenate(d["rayPooling_votes_list"])
    T, n, N = ijk.shape[0], len(d["vxl_ijk_list"]), cases.ARGS["N_refine_iter"]
    assert Dc == 64
    bufs = []

    def up(a):
        a = np.ascontiguousarray(a)
        p = ctx.dev_alloc(max(a.nbytes, 1))
        bufs.append(p)
        ctx.h2d(p, a)
        return p

    def alloc(nbytes):
        p = ctx.dev_alloc(nbytes)
        bufs.append(p)
        return p
    try:
        d_off, d_ijk, d_p, d_v, d_cube = up(off), up(ijk), up(p16), up(votes), up(d["cube_ijk_np"].astype(np.uint32))
        d_init, d_thr, d_m, d_den, d_ch = alloc(T), alloc(8 * N * n), alloc(N * T), alloc(N * T), alloc(N * n)
        a = cases.ARGS
        cfg = _lib.AdapthreshCfg(N, c["D_cube"], a["init_probThresh"], a["max_probThresh"], float(a["rayPool_thresh"]), float(a["beta"]))
        _lib.check(ctx._lib.sn_adapthresh_dev(ctx._h, n, Dc, ctypes.byref(cfg), T, d_off, d_ijk, d_p, d_v, d_cube, d_init, d_thr, d_m, d_den, d_ch))
        ctx.synchronize()
        got = dict(init_denoised=np.empty(T, np.uint8), thresh=np.empty((N, n)), masks=np.empty((N, T), np.uint8), denoised=np.empty((N, T), np.uint8),
                   choice=np.empty((N, n), np.int8))
        for k, p in (("init_denoised", d_init), ("thresh", d_thr), ("masks", d_m), ("denoised", d_den), ("choice", d_ch)):
            ctx.d2h(got[k], p)
            assert np.array_equal(got[k].view(host[k].dtype) if host[k].dtype == bool else got[k], host[k]), k
        d_mask, d_out = up(np.concatenate(c["masks"]).view(np.uint8)), alloc(T)
        _lib.check(ctx._lib.sn_denoise_dev(ctx._h, n, Dc, c["D_cube"], T, d_off, d_ijk, d_cube, d_mask, d_out))
        out = np.empty(T, np.uint8)
        ctx.d2h(out, d_out)
        assert np.array_equal(out.view(bool), np.concatenate(c["dn_ref"]))
    finally:
        for p in bufs:
            ctx.dev_free(p)
