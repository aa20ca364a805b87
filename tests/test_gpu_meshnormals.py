"""GPU (-m gpu): the mesh's own normals, area and volume (surfacenet_amd/csrc/meshnormals.h) against the restatement
tests/meshnormals_ref.py, byte for byte - both normal arrays, the counts and the limbs of the two sums -, in the host form and the device form:
the named cases, the fan whose hub sums carry out of their low words well over a hundred times, a permutation of its faces, repeated calls on
one context, the empty meshes, the refusals in the other stages' words, and the opt-in of reconstruct.scene_postpass."""
import os

import numpy as np
import pytest

import mesh_refusals as bad
import meshnormals_ref as ref

pytestmark = pytest.mark.gpu
CASES = ("sheet_q", "sheet_t", "sphere6_q", "sphere6_t", "rules", "soup", "fan5000", "surface")


@pytest.fixture(scope="module")
def ctx(gpu_required):
    from surfacenet_amd import runtime
    return runtime.any_context()


def _bytes(r):
    return {k: np.asarray(r[k]).tobytes() for k in ref.KEYS}


def _check(ctx, v, f, want):
    for device in (False, True):
        got = ctx.mesh_normals(v, f, device=device)
        assert got["face_normals"].dtype == np.float32 and got["vert_normals"].dtype == np.float32
        assert got["counts"].dtype == np.int64 and got["sums"].dtype == np.uint64
        assert ref.same_bytes(got, want) == [], (device, ref.same_bytes(got, want))
    return got


@pytest.mark.parametrize("name", CASES)
def test_bit_for_bit_against_the_restatement(ctx, name):
    v, f = ref.CASES[name]()
    want = ref.reference(name)
    _check(ctx, v, f, want)
    if name == "surface":
        assert f.shape[0] == 4600                              # several workgroups
    if name == "rules":
        assert np.isnan(v[7, 0]) and want["counts"].tolist() == [1, 1, 7, 6]


def test_the_wide_carry_in_any_order(ctx):
    v, f = ref.CASES["bigfan300"]()
    want = ref.reference("bigfan300")
    assert want["N_v"][0][2] == 21857123061572827086848
    _check(ctx, v, f, want)
    perm = np.random.default_rng(11).permutation(f.shape[0])
    shuffled = dict(want, face_normals=want["face_normals"][perm])
    _check(ctx, v, np.ascontiguousarray(f[perm]), shuffled)


def test_python_layer_assembles_the_limbs(ctx):
    from surfacenet_amd import mesh
    for name, resol in (("bigfan300", 0.4), ("sphere6_q", 0.25)):
        v, f = ref.CASES[name]()
        want = ref.reference(name)
        got = mesh.mesh_normals(v, f, resol=resol)
        assert got["area2"] == want["area2"] and got["vol6"] == want["vol6"]
        assert [got[k] for k in mesh.NORMAL_COUNTS] == want["counts"].tolist()
        assert got["area"] == want["area2"] / 2 / 2 ** 32 * resol ** 2 and got["volume"] == want["vol6"] / 6 / 2 ** 48 * resol ** 3
        assert got["vert_normals"].tobytes() == want["vert_normals"].tobytes() and got["face_normals"].tobytes() == want["face_normals"].tobytes()
    assert abs(mesh.mesh_normals(*ref.CASES["sphere6_t"]())["volume"] - 1015.167199) < 1e-6


def test_run_twice_then_grow_the_workspace_and_come_back(ctx):
    small, large = ref.CASES["sphere6_q"](), ref.CASES["soup"]()
    first = _bytes(ctx.mesh_normals(*small))
    assert _bytes(ctx.mesh_normals(*small)) == first
    assert ref.same_bytes(ctx.mesh_normals(*large), ref.reference("soup")) == []
    assert _bytes(ctx.mesh_normals(*small)) == first and _bytes(ctx.mesh_normals(*small, device=True)) == first


def test_empty_meshes_and_one_face(ctx):
    v = np.asarray([(0, 0, 0), (2, 0, 0), (0, 2, 0), (np.nan, 1, 1)], np.float64)
    for device in (False, True):
        e = ctx.mesh_normals(v, np.zeros((0, 3), np.int32), device=device)      # F = 0: zero rows, the NaN vertex is not looked at
        assert e["vert_normals"].shape == (4, 3) and not e["vert_normals"].any() and e["face_normals"].shape == (0, 3)
        assert not e["counts"].any() and not e["sums"].any()
        e = ctx.mesh_normals(np.zeros((0, 3)), np.zeros((0, 4), np.int32), device=device)      # V = 0
        assert e["vert_normals"].shape == (0, 3) and e["face_normals"].shape == (0, 3) and not e["counts"].any() and not e["sums"].any()
    f = np.asarray([[0, 1, 2]], np.int32)
    want = ref.normals(v, f)
    got = _check(ctx, v, f, want)
    assert got["face_normals"].tolist() == [[0.0, 0.0, 1.0]] and got["vert_normals"].tolist() == [[0.0, 0.0, 1.0]] * 3 + [[0.0, 0.0, 0.0]]
    assert got["counts"].tolist() == [0, 0, 3, 1] and got["sums"].tolist() == [4 << 32, 0, 0, 0, 0, 0]      # area 2 cells^2; the origin is a corner


@pytest.mark.parametrize("rows,at,later,coord_at", [(4, 2, 5, 3), (51, 257, 280, 257)])
def test_refusals_in_the_smoothers_words(ctx, rows, at, later, coord_at):
    from surfacenet_amd import SurfaceNetHipError
    v, f = bad.sheet(rows)
    assert f.shape == (6 * (rows - 1), 3)
    before = {device: _bytes(ctx.mesh_normals(v, f, device=device)) for device in (False, True)}
    assert before[False] == before[True] == _bytes(ref.normals(v, f))
    cases = [bad.bad_index(v, f, at, later)]
    for value in (np.nan, 2097144.0):
        cases.append(bad.bad_coordinate(v, f, coord_at, value))
    far, _, text = bad.bad_coordinate(v, f, coord_at, np.nan)       # ... and a bad index at a later face: the smaller face is the one named
    cases.append((far, bad.bad_index(v, f, later, later)[1], text))
    for bv, bf, text in cases:
        said = set()
        for device in (False, True):
            for run in (lambda: ctx.mesh_normals(bv, bf, device=device), lambda: ctx.mesh_smooth(bv, bf, 2, device=device)):
                with pytest.raises(SurfaceNetHipError) as e:
                    run()
                said.add(str(e.value))
        assert len(said) == 1 and text in said.pop(), (text, said)
    assert {device: _bytes(ctx.mesh_normals(v, f, device=device)) for device in (False, True)} == before


def _scene():
    import normals_ref as nref
    s = nref.surface_scene((2, 2, 1))
    d = s["lists"]
    out = dict(prediction_list=d["prediction_list"], vxl_ijk_list=d["vxl_ijk_list"], rayPooling_votes_list=d["rayPooling_votes_list"],
               cube_ijk_np=d["cube_ijk_np"], param_np=s["param"], viewPair_np=s["viewPair"], rgb_list=d["rgb_list"])
    return s, d, out


def test_in_a_scene(gpu_required, tmp_path):
    import mesh_ref as mr
    import meshchain_util as mc
    from surfacenet_amd import mesh, reconstruct
    s, d, out = _scene()
    kw = dict(tau=0.7, gamma=0.5, N_refine_iter=2, cameraTs_np=s["cameraTs"], mesh=True, mesh_fill=16, mesh_smooth=3, mesh_cell=2)
    dirs = {}
    for tag in ("own", "plain", "source"):
        dirs[tag] = tmp_path / tag
        dirs[tag].mkdir()
    own = reconstruct.scene_postpass(out, 32, 26, 2, mesh_normals="mesh", mesh_ply_prefix=str(dirs["own"] / "s_"), **kw)
    plain = reconstruct.scene_postpass(out, 32, 26, 2, mesh_ply_prefix=str(dirs["plain"] / "s_"), **kw)
    source = reconstruct.scene_postpass(out, 32, 26, 2, mesh_normals="source", mesh_ply_prefix=str(dirs["source"] / "s_"), **kw)
    _, resol = mesh.lattice_origin(d["cube_ijk_np"], s["param"], 13)
    files = {"": "_mesh.ply", "_filled": "_mesh_f16.ply", "_smoothed": "_mesh_s3.ply", "_simplified": "_mesh_c2.ply"}
    assert sorted(os.listdir(str(dirs["own"]))) == sorted("s_" + name + f for name in ("fixThresh", "adapt") for f in files.values())
    for name in ("fixThresh", "adapt"):
        for end, fname in files.items():
            key = name + "_mesh" + end
            got, base = own[key], plain[key]
            assert set(got) - set(base) == {"vert_normals", "area", "volume"}
            mc.same_dict({k: got[k] for k in base}, base)
            faces = got["faces"] if "faces" in got else got["quads"]
            want = mesh.mesh_normals(got["vert_lattice"], faces, resol=resol)
            assert got["vert_normals"].tobytes() == want["vert_normals"].tobytes() and got["vert_normals"].shape[0] > 100
            assert got["area"] == want["area"] > 0 and got["volume"] == want["volume"]
            _, verts, _ = mr.parse_ply(str(dirs["own"] / ("s_" + name + fname)))
            assert np.stack([verts["nx"], verts["ny"], verts["nz"]], 1).astype(np.float32).tobytes() == want["vert_normals"].tobytes()
            assert np.array_equal(np.stack([verts["red"], verts["green"], verts["blue"]], 1), mc.gathered(d["rgb_list"], got["vert_src"], np.uint8))
            mc.same_dict(source[key], base)                    # the default keyword: the dicts and the files of the call without it
            for tag in ("plain", "source"):
                mc.check_stage_ply(str(dirs[tag] / ("s_" + name + fname)), base, plain[name + "_normal_list"], d["rgb_list"])
            assert open(str(dirs["plain"] / ("s_" + name + fname)), "rb").read() == open(str(dirs["source"] / ("s_" + name + fname)), "rb").read()
