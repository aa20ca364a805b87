"""GPU (-m gpu): the chain that follows extract_mesh in reconstruct.scene_postpass - fill, smooth, decimate (surfacenet_amd/mesh.py run_chain;
DESIGN.md section 4.19) - in every on / off combination on the small scene of the mesh tests, with mesh_reach 0, 1 and 2: each stage's dict
is that of the stages called by hand on the result before it, and each PLY file holds its stage's mesh with normals and colours gathered
through the stage's vert_src, zero where it is -1. On this scene reach 1 leaves no vertex without a source voxel (2678 and 2695 vertices, none
at -1); reach 2 does (214 of 2893 and 238 of 2933), so it is the case in which -1 meets the gathers of fill and decimate."""
import os

import numpy as np
import pytest

import meshchain_util as mc
import normals_ref as nref

pytestmark = pytest.mark.gpu
FILES = dict(filled="_mesh_f16.ply", smoothed="_mesh_s2.ply", simplified="_mesh_c2.ply")


@pytest.mark.parametrize("combo", mc.COMBOS)
@pytest.mark.parametrize("reach", [0, 1, 2])
def test_scene_postpass_chain_equals_the_stages_by_hand(gpu_required, tmp_path, reach, combo):
    from surfacenet_amd import mesh, reconstruct
    s = nref.surface_scene((2, 2, 1))
    d = s["lists"]
    out = dict(prediction_list=d["prediction_list"], vxl_ijk_list=d["vxl_ijk_list"], rayPooling_votes_list=d["rayPooling_votes_list"],
               cube_ijk_np=d["cube_ijk_np"], param_np=s["param"], viewPair_np=s["viewPair"], rgb_list=d["rgb_list"])
    fill, smooth, cell = combo
    prefix = str(tmp_path / "scene_")
    post = reconstruct.scene_postpass(out, 32, 26, 2, tau=0.7, gamma=0.5, N_refine_iter=2, cameraTs_np=s["cameraTs"], mesh=True, mesh_reach=reach,
                                      mesh_fill=fill, mesh_smooth=smooth, mesh_cell=cell, mesh_ply_prefix=prefix)
    origin, resol = mesh.lattice_origin(d["cube_ijk_np"], s["param"], 13)
    keys = mc.asked(combo)
    assert {k for k in post if "_mesh" in k} == {name + "_mesh" + end for name in ("fixThresh", "adapt") for end in [""] + ["_" + k for k in keys]}
    assert sorted(os.listdir(str(tmp_path))) == sorted("scene_" + name + f for name in ("fixThresh", "adapt")
                                                       for f in ["_mesh.ply"] + [FILES[k] for k in keys])
    for name in ("fixThresh", "adapt"):
        m, nl = post[name + "_mesh"], post[name + "_normal_list"]
        none = int((m["vert_src"] < 0).sum())
        print("%s reach %d: %d vertices, %d without a source voxel" % (name, reach, len(m["vert_src"]), none))
        assert set(m) == {"vertices", "quads", "vert_src", "vert_lattice"}
        assert none > 0 or reach < 2                            # (what reach 2 is here for; on this scene reach 1 leaves no such vertex)
        mc.check_stage_ply(prefix + name + "_mesh.ply", m, nl, d["rgb_list"])
        want = mc.by_hand(mesh, m, combo, origin, resol)
        assert list(want) == keys
        for key in keys:
            got = post["%s_mesh_%s" % (name, key)]
            mc.same_dict(got, want[key])
            assert got["vertices"].shape[0] > 100 and ("quads" in got) == (key == "smoothed" and fill is None)
            if reach == 2 and key != "smoothed":                     # the gathers of fill and decimate meet a vertex without a source voxel
                assert (got["vert_src"] < 0).any() and (got["vert_src"] >= 0).any()
            mc.check_stage_ply(prefix + name + FILES[key], got, nl, d["rgb_list"])
