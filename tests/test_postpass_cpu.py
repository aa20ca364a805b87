"""CPU: the cross-cube post-pass's checker and host I/O - the restatement (tests/postpass_ref.py) against the goldens recorded from the
reference (tests/golden/postpass_cases.npz, postpass_edge_cases.npz), the PLY byte layout, the npz round trip with the reference's keys, and
that the cases of tests/postpass_cases.py can tell a wrong kernel path from a right one (conditions on the restatement, planted faults)."""
import os
import struct

import numpy as np
import pytest

import postpass_cases as cases
import postpass_ref as ref

DN, AT = ref.load_cases()


def test_golden_covers_the_contract():
    assert {"doc_cluster", "doc_mark", "doc_denoise", "s32_D26", "s32_D32", "s64_D52", "s64_D64"} <= set(DN)
    assert {"s32", "s32_f16", "s32_thick", "s64"} <= set(AT)
    c = DN["s32_D26"]
    assert any(len(a) == 0 for a in c["ijk_list"]), "an empty cube"
    assert any(len(m) and not m.any() for m in c["mask_list"]), "a cube whose voxels are all masked out"
    keys = [tuple(k) for k in c["cube_ijk"].tolist()]
    assert len(set(keys)) < len(keys), "a repeated ijk"
    assert (c["cube_ijk"] == 0).all(axis=1).any(), "a cube at ijk 0"


@pytest.mark.parametrize("name", sorted(DN))
def test_denoise_restatement_matches_reference(name):
    c = DN[name]
    got = ref.denoise_ref(c["cube_ijk"], c["ijk_list"], c["mask_list"], c["D_cube"])
    assert len(got) == len(c["out_list"])
    for a, b in zip(got, c["out_list"]):
        assert a.dtype == bool and np.array_equal(a, b)


@pytest.mark.parametrize("name", sorted(AT))
def test_adapthresh_restatement_matches_reference(name):
    c = AT[name]
    r = ref.adapthresh_ref(c["pred_list"], c["ijk_list"], c["votes_list"], c["cube_ijk"], c["N_refine_iter"], c["D_cube"], c["init_probThresh"],
                           c["max_probThresh"], c["rayPool_thresh"], c["beta"])
    assert np.array_equal(np.concatenate(r["init_denoised"]), c["init_denoised"])
    assert r["thresh"].dtype == np.float64 and np.array_equal(r["thresh"], c["thresh"])        # exact, float64
    assert np.array_equal(r["choice"], c["choice"])
    for k in range(c["N_refine_iter"]):
        assert np.array_equal(np.concatenate(r["masks"][k]), c["masks"][k])
        assert np.array_equal(np.concatenate(r["denoised"][k]), c["denoised"][k])


def test_float16_cost_decides_and_overflows_in_the_goldens():
    """s32_f16: the float16 accumulation picks another argmin than exact integers would; s32_thick: costs overflow to inf."""
    for name, want in (("s32_f16", "rounding"), ("s32_thick", "inf")):
        c = AT[name]
        args = (c["pred_list"], c["ijk_list"], c["votes_list"], c["cube_ijk"], 1, c["D_cube"], c["init_probThresh"], c["max_probThresh"],
                c["rayPool_thresh"], c["beta"])
        f16, exact = ref.adapthresh_ref(*args), ref.adapthresh_ref(*args, exact_cost=True)
        if want == "rounding":
            assert (f16["choice"] != exact["choice"]).any()
        else:
            assert np.isinf(f16["cost"]).any()


def test_numpy2_float16_accumulation():
    """the semantics DESIGN.md section 4.6 records: the Python int is rounded to float16 first (NEP 50)"""
    c = np.array([-2045, 0, 0]).astype(np.float16)
    c[0] += 4099
    assert c[0] == 2056
    with np.errstate(over="ignore"):
        c[1] += 70000
    assert np.isinf(c[1]) and np.argmin(np.array([np.inf, np.inf, 5], np.float16)) == 2


def test_ply_byte_layout(tmp_path):
    from surfacenet_amd import sparseCubes
    xyz = np.array([[1.5, -2.25, 3.0], [0.1, 0.2, 0.3]], np.float32)
    rgb = np.array([[1, 2, 3], [250, 128, 0]], np.uint8)
    p = str(tmp_path / "sub" / "a.ply")
    sparseCubes.save2ply(p, xyz, rgb)
    head = b"ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n" \
           b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n"
    body = b"".join(struct.pack("<fffBBB", *x.tolist(), *c.tolist()) for x, c in zip(xyz, rgb))
    assert open(p, "rb").read() == head + body
    nrm = np.ones((2, 3), np.float32)
    sparseCubes.save2ply(p, xyz, rgb, nrm)
    data = open(p, "rb").read()
    assert b"property float nx\nproperty float ny\nproperty float nz\nproperty uchar red" in data and len(data.split(b"end_header\n")[1]) == 2 * 27


def test_save_sparseCubes_2ply_coordinates(tmp_path):
    """xyz = ijk * resol + xyz_min in float32, the masked voxels cube after cube (utils/sparseCubes.py:321-322)"""
    from surfacenet_amd import sparseCubes, synthetic
    c = AT["s64"]
    masks = [m.astype(bool) for m in ref.split(c["denoised"][0], c["offsets"])]
    rgb = [np.full((len(a), 3), 7, np.uint8) for a in c["ijk_list"]]
    p = str(tmp_path / "x.ply")
    sparseCubes.save_sparseCubes_2ply(masks, c["ijk_list"], rgb, c["param"], ply_filePath=p)
    xyz = np.vstack([c["ijk_list"][i][m] * c["param"][i]["resol"] + c["param"][i]["xyz"][None, :] for i, m in enumerate(masks)])
    data = open(p, "rb").read()
    head, body = data.split(b"end_header\n")
    assert b"element vertex %d\n" % xyz.shape[0] in head
    rec = np.frombuffer(body, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")]))
    assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], -1), xyz.astype(np.float32)) and (rec["red"] == 7).all()
    assert synthetic.CUBE_DTYPE == c["param"].dtype


def test_npz_round_trip_with_reference_keys(tmp_path):
    from surfacenet_amd import sparseCubes
    c = AT["s32"]
    rgb = [np.arange(3 * len(a), dtype=np.uint8).reshape(-1, 3) for a in c["ijk_list"]]
    vp = np.arange(len(c["ijk_list"]) * 2, dtype=np.uint16).reshape(-1, 1, 2)
    p = str(tmp_path / "m.npz")
    sparseCubes.save_sparseCubes(p, c["pred_list"], rgb, c["ijk_list"], c["votes_list"], c["cube_ijk"], c["param"], vp)
    with np.load(p) as z:
        assert sorted(z.files) == sorted(["cube_1st_vxlIndx_np", "prediction_np", "rgb_np", "vxl_ijk_np", "rayPooling_votes_np", "cube_ijk_np",
                                          "param_np", "viewPair_np"])
        assert z["cube_1st_vxlIndx_np"].dtype == np.uint32 and np.array_equal(z["cube_1st_vxlIndx_np"], c["offsets"])
    back = sparseCubes.load_sparseCubes(p)
    for got, want in zip(back[:4], (c["pred_list"], rgb, c["ijk_list"], c["votes_list"])):
        assert len(got) == len(want) and all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want))
    assert np.array_equal(back[4], c["cube_ijk"]) and np.array_equal(back[5], c["param"]) and np.array_equal(back[6], vp)
    # a file without votes (ray pooling off) loads to empty per-cube vote arrays, as the reference's does
    sparseCubes.save_sparseCubes(p, c["pred_list"], rgb, c["ijk_list"], [], c["cube_ijk"], c["param"], vp)
    assert all(v.size == 0 for v in sparseCubes.load_sparseCubes(p)[3])


# ---- the cases of tests/postpass_cases.py: each one can tell a kernel that takes the wrong path from one that does not ------------------------
DISCRIMINATING = ["w27", "w53", "w63", "w64", "crop32", "crop64", "tiny"]


def test_edge_fixture_holds_the_cases_of_the_table():
    """tests/golden/postpass_edge_cases.npz is the reference's run on cases.build()'s lists (the wide cases on GOLDEN_LATTICE)"""
    assert set(cases.TABLE) <= set(DN) and set(cases.TABLE) <= set(AT)
    for name in cases.TABLE:
        d, D_cube, Dc = cases.build(name, cases.GOLDEN_LATTICE.get(name))
        for c in (DN[name], AT[name]):
            assert c["D_cube"] == D_cube and np.array_equal(c["cube_ijk"], d["cube_ijk_np"])
            assert len(c["ijk_list"]) == len(d["vxl_ijk_list"]) and all(np.array_equal(a, b) for a, b in zip(c["ijk_list"], d["vxl_ijk_list"]))
        assert all(np.array_equal(a, b) for a, b in zip(DN[name]["mask_list"], cases.denoise_masks(d)))
        assert all(np.array_equal(a, b) for a, b in zip(AT[name]["pred_list"], d["prediction_list"]))
        assert all(np.array_equal(a, b) for a, b in zip(AT[name]["votes_list"], d["rayPooling_votes_list"]))
        assert (AT[name]["N_refine_iter"], AT[name]["beta"]) == (cases.ARGS["N_refine_iter"], cases.ARGS["beta"])


@pytest.mark.parametrize("name", DISCRIMINATING)
def test_edge_case_has_competing_choices_removed_voxels_and_repeats(name):
    c = cases.case(name)
    first = c["at_ref"]["choice"][0]
    assert (first == 0).any() and (first == 1).any()
    masked, kept = np.concatenate(c["masks"]), np.concatenate(c["dn_ref"])
    assert (masked & ~kept).any() and kept.any()
    assert any(len(np.unique(a, axis=0)) < len(a) for a in c["d"]["vxl_ijk_list"]), "no cube repeats a voxel"


@pytest.mark.parametrize("k0", [63, 32])
def test_w64_upper_bits_decide_verdicts_below_them(k0):
    """without the voxels of k >= k0 some voxel of k < k0 gets another verdict: bit 63 of a row (k0 = 63) and the bits a shift by h = 32 moves
    (k0 = 32) carry components and coincidences, so a kernel that drops them gives another result"""
    c = cases.case("w64")
    d = c["d"]
    below = [a[:, 2] < k0 for a in d["vxl_ijk_list"]]
    assert any((m & ~b).any() for m, b in zip(c["masks"], below))
    got = ref.denoise_ref(d["cube_ijk_np"], d["vxl_ijk_list"], [m & b for m, b in zip(c["masks"], below)], c["D_cube"], Dc=64)
    assert any(((g != w) & b).any() for g, w, b in zip(got, c["dn_ref"], below))


@pytest.mark.parametrize("name", ["crop32", "crop64"])
def test_crop_cases_depend_on_D_cube(name):
    c = cases.case(name)
    assert c["D_cube"] > c["Dc"]
    other = ref.adapthresh_ref(*cases.at_args(c["d"], c["Dc"]))
    diff = cases.adapthresh_differences(cases.packed(other), cases.packed(c["at_ref"]))
    assert "thresh" in diff or "masks" in diff


def test_far_case_has_no_coincidence_and_no_overlap():
    """h = D_cube // 2 >= Dc: denoise keeps nothing, and every face's AND is 0, so the exact cost is the sum of the half counts nA + nB. With
    h = Dc a cube's voxels all lie in its three lower halves and in none of the upper ones."""
    c = cases.case("far")
    d = c["d"]
    assert c["D_cube"] // 2 >= c["Dc"]
    assert not np.concatenate(c["dn_ref"]).any()
    assert not np.concatenate(c["at_ref"]["init_denoised"]).any() and not any(np.concatenate(m).any() for m in c["at_ref"]["denoised"])
    r = ref.adapthresh_ref(*cases.at_args(d, c["D_cube"], 1), exact_cost=True)
    init = [(p >= cases.ARGS["init_probThresh"]) & (v >= cases.ARGS["rayPool_thresh"]) for p, v in zip(d["prediction_list"], d["rayPooling_votes_list"])]
    mp = ref.cube_map(d["cube_ijk_np"], init)
    assert len(mp) > 1
    for key, n in mp.items():
        nB = sum(int(init[mp[nb]].sum()) for nb in ((key[0] + 1, key[1], key[2]), (key[0], key[1] + 1, key[2]), (key[0], key[1], key[2] + 1)) if nb in mp)
        for g in range(3):
            nA = int((init[n] & (d["prediction_list"][n] >= cases.ARGS["init_probThresh"] + ref.THRESH_PERTURB[g])).sum())
            assert r["cost"][0, n, g] == 3 * nA + nB, (n, g)


def test_many_cubes_pairs_mapped_and_unmapped_cubes_512_apart():
    c = cases.many_cubes()
    d = c["d"]
    n = len(d["vxl_ijk_list"])
    assert n > 512 and len(c["masks"]) == n and len(d["cube_ijk_np"]) == n
    assert 300000 < sum(len(a) for a in d["vxl_ijk_list"]) < 400000
    mp = ref.cube_map(d["cube_ijk_np"], c["masks"])
    mapped = np.zeros(n, bool)
    mapped[list(mp.values())] = True
    lo = np.arange(n - 512)
    assert (mapped[lo] & ~mapped[lo + 512]).any() and (~mapped[lo] & mapped[lo + 512]).any()
    assert min(c["emptied"]) < 512 <= max(c["emptied"]) and not mapped[list(c["emptied"])].any()
    assert c["masks"][c["repeated"]].any() and not mapped[c["repeated"]] and mapped[n - 1]          # the later cube of the same ijk wins


def test_extreme_ijk_third_cube_is_nobodys_neighbour():
    """at x = 2**32 - 1 the third cube neighbours nobody; were the cube arithmetic 32 bits wide it would be cube 0's lower neighbour, and the
    same scene at x = 1, 2, 0 shows that this changes verdicts in cube 0 and cube 2"""
    c = cases.extreme_ijk()
    d = c["d"]
    assert d["cube_ijk_np"].dtype == np.uint32 and d["cube_ijk_np"][2, 0] == 2 ** 32 - 1
    got = ref.denoise_ref(d["cube_ijk_np"], d["vxl_ijk_list"], c["masks"], c["D_cube"])
    assert got[0].any() and got[1].any() and c["masks"][2].any() and not got[2].any()
    wrapped = ref.denoise_ref(c["wrapped"], d["vxl_ijk_list"], c["masks"], c["D_cube"])
    assert wrapped[2].any() and (wrapped[0] & ~got[0]).any()
    r = ref.adapthresh_ref(*cases.at_args(d, c["D_cube"], 1))
    w = ref.adapthresh_ref(*cases.at_args(dict(d, cube_ijk_np=c["wrapped"]), c["D_cube"], 1))
    assert not np.array_equal(r["cost"], w["cost"])


# ---- planted faults: the comparison the GPU tests use fails on a result with one slip of the kind these cases are for ------------------------
@pytest.mark.parametrize("name,g,g_from", [("w53", 2, None), ("w64", 2, None), ("w53", 1, 0), ("w64", 1, 0)])
def test_a_planted_pass_slip_fails_the_comparison(name, g, g_from):
    """One cube's grid g left empty (a pass of cc_grid_kernel's g0 loop that never wrote) or built with another grid's threshold (a pass that
    indexes the thresholds from its own start): some cube shows it in thresh, choice or masks."""
    c = cases.case(name)
    want = cases.packed(c["at_ref"])
    assert cases.adapthresh_differences(cases.packed(c["at_ref"]), want) == []
    shown = None
    for cube in range(len(c["d"]["vxl_ijk_list"])):
        got = cases.packed(ref.adapthresh_ref(*cases.at_args(c["d"], c["D_cube"]), fault=(cube, g, g_from)))
        if cases.adapthresh_differences(got, want):
            shown = cube
            break
    assert shown is not None


def test_grid_2_from_grid_1s_threshold_cannot_show():
    """The slip the w53 / w64 cases were first meant to catch is invisible in any result, by the algorithm and not by the choice of case: a
    cube's mask already holds pred >= t (the initial mask is cut at init_probThresh = the first t, and every iteration ends with
    mask &= pred >= t), so grid 2 (mask & pred >= t - 0.1) IS grid 1 (mask & pred >= t), cost[2] == cost[1], and np.argmin never returns 2.
    What a wrong grid 2 can show is covered above: an empty or stale one."""
    for name in ("w53", "w64"):
        c = cases.case(name)
        assert not (c["at_ref"]["choice"] == 2).any()
        assert np.array_equal(c["at_ref"]["cost"][..., 2], c["at_ref"]["cost"][..., 1])
        got = ref.adapthresh_ref(*cases.at_args(c["d"], c["D_cube"]), fault=(0, 2, 1))
        assert cases.adapthresh_differences(cases.packed(got), cases.packed(c["at_ref"])) == []


def test_a_dropped_bit_63_fails_the_comparison():
    c = cases.case("w64")
    d = c["d"]
    assert cases.list_differences(c["dn_ref"], c["dn_ref"]) == []
    cube, v = next((n, np.nonzero(k & (a[:, 2] == 63))[0][0]) for n, (k, a) in enumerate(zip(c["dn_ref"], d["vxl_ijk_list"])) if (k & (a[:, 2] == 63)).any())
    i, j, k = d["vxl_ijk_list"][cube][v].tolist()
    got = ref.denoise_ref(d["cube_ijk_np"], d["vxl_ijk_list"], c["masks"], c["D_cube"], fault=(cube, i, j, k))
    assert cube in cases.list_differences(got, c["dn_ref"])
