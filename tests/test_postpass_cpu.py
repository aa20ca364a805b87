"""CPU: the cross-cube post-pass's checker and host I/O - the restatement (tests/postpass_ref.py) against the goldens recorded from the
reference (tests/golden/postpass_cases.npz), the PLY byte layout, and the npz round trip with the reference's keys."""
import os
import struct

import numpy as np
import pytest

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
