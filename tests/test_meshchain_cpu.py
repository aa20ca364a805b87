"""CPU: the chain that follows extract_mesh in a scene, stated once in surfacenet_amd/mesh.py - chain_settings, run_chain
on the empty mesh, save_stage_2ply - and reconstruct.scene_postpass's use of it on an empty scene. Nothing here touches the library."""
import numpy as np
import pytest

import meshchain_util as mc


@pytest.fixture(autouse=True)
def _no_library(monkeypatch):
    from surfacenet_amd import runtime

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(runtime, "any_context", no_library)


FILL_KW = dict(max_len=16, orientation="any")
SMOOTH_KW = dict(iterations=2, lam=0.5, mu=-0.53, boundary="curve")
CELL_KW = dict(cell=2, placement="mean")


@pytest.mark.parametrize("combo", mc.COMBOS)
def test_chain_settings_gives_the_stages_asked_for_in_the_chains_order(combo):
    from surfacenet_amd import mesh
    stages = mesh.chain_settings(*combo, "mean")
    assert [key for key, _ in stages] == mc.asked(combo)
    assert dict(stages) == {key: kw for key, kw in zip(mc.KEYS, (FILL_KW, SMOOTH_KW, CELL_KW)) if key in mc.asked(combo)}
    assert [mesh.stage_tag(key, kw) for key, kw in stages] == [dict(filled="_f16", smoothed="_s2", simplified="_c2")[key] for key in mc.asked(combo)]


def test_chain_settings_fills_in_the_defaults():
    from surfacenet_amd import mesh
    assert mesh.chain_settings(None, None, None, "member") == []
    assert mesh.chain_settings(64, dict(mu=0.0, boundary="free"), 3, "member") == [
        ("filled", dict(max_len=64, orientation="holes")), ("smoothed", dict(iterations=10, lam=0.5, mu=0.0, boundary="free")),
        ("simplified", dict(cell=3, placement="member"))]
    assert mesh.chain_settings(dict(orientation="any"), None, None, "mean") == [("filled", dict(max_len=64, orientation="any"))]


BAD = (      # (mesh_fill, mesh_smooth, mesh_cell, mesh_placement) with one bad setting -> the refusal, word for word
    ((2, None, None, "mean"), "max_len = 2: an integer number of edges in 3 .. 65536"),
    (("64", None, None, "mean"), "max_len = '64': an integer number of edges in 3 .. 65536"),
    ((dict(max_len=[1]), None, None, "mean"), "max_len = [1] must be an integer"),
    ((dict(max_len=16, orientation="rims"), None, None, "mean"), "orientation = 'rims': 'holes' or 'any'"),
    ((dict(max_len=16, iterations=4), None, None, "mean"),
     "mesh_fill = {'max_len': 16, 'iterations': 4}: a largest loop length or a dict of max_len, orientation"),
    ((None, -1, None, "mean"), "iterations = -1: an integer in 0 .. 1000"),
    ((None, 2.5, None, "mean"), "iterations = 2.5: an integer in 0 .. 1000"),
    ((None, dict(lam=2.0), None, "mean"), "lam = 2.0: a factor in -1 .. 1"),
    ((None, dict(mu="a"), None, "mean"), "mu = 'a' must be a number"),
    ((None, dict(iterations=2, boundary="rim"), None, "mean"), "boundary = 'rim': 'fixed', 'curve' or 'free'"),
    ((None, dict(iterations=2, cell=4), None, "mean"),
     "mesh_smooth = {'iterations': 2, 'cell': 4}: a number of iterations or a dict of iterations, lam, mu, boundary"),
    ((None, None, 1, "mean"), "cell = 1: an integer number of lattice cells in 2 .. 64"),
    ((None, None, 2.5, "mean"), "cell = 2.5: an integer number of lattice cells in 2 .. 64"),
    ((None, None, dict(cell=2), "mean"), "cell = {'cell': 2} must be an integer"),
    ((None, None, 2, "median"), "placement = 'median': 'mean' or 'member'"),
)


@pytest.mark.parametrize("args,text", BAD)
def test_a_bad_setting_is_refused_in_the_words_scene_postpass_has_always_used(args, text):
    from surfacenet_amd import mesh, reconstruct
    with pytest.raises(ValueError) as e:
        mesh.chain_settings(*args)
    assert str(e.value) == text
    empty = dict(prediction_list=[], vxl_ijk_list=[], rayPooling_votes_list=[], cube_ijk_np=np.zeros((0, 3), np.int64))
    fill, smooth, cell, placement = args
    with pytest.raises(ValueError) as e:
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=np.zeros((2, 3)), mesh=True, mesh_fill=fill, mesh_smooth=smooth, mesh_cell=cell,
                                   mesh_placement=placement)
    assert str(e.value) == text


def test_two_bad_arguments_name_the_earlier_one_mesh_cell_then_mesh_smooth_then_mesh_fill():
    from surfacenet_amd import mesh, reconstruct
    for args, word in (((2, -1, 1, "mean"), "cell = 1"), ((2, -1, 2, "median"), "placement"), ((2, -1, 2, "mean"), "iterations = -1"),
                       ((2, dict(cell=4), None, "mean"), "mesh_smooth = "), ((dict(cell=4), 2, 2, "mean"), "mesh_fill = "),
                       ((dict(max_len=2, cell=4), None, None, "mean"), "mesh_fill = "), ((2, None, 2, "mean"), "max_len = 2")):
        with pytest.raises(ValueError) as e:
            mesh.chain_settings(*args)
        assert str(e.value).startswith(word), (args, str(e.value))
    # without mesh=True the first argument given, in that order, is the one refused - however bad the others are
    empty = dict(prediction_list=[], vxl_ijk_list=[], rayPooling_votes_list=[], cube_ijk_np=np.zeros((0, 3), np.int64))
    for kw, text in ((dict(mesh_cell=1, mesh_smooth=-1, mesh_fill=2), "mesh_cell needs mesh=True: it simplifies the mesh that mesh=True extracts"),
                     (dict(mesh_smooth=-1, mesh_fill=2), "mesh_smooth needs mesh=True: it smooths the mesh that mesh=True extracts"),
                     (dict(mesh_fill=2), "mesh_fill needs mesh=True: it fills the holes of the mesh that mesh=True extracts")):
        with pytest.raises(ValueError) as e:
            reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=np.zeros((2, 3)), **kw)
        assert str(e.value) == text
    with pytest.raises(ValueError, match="mesh=True needs cameraTs_np"):
        reconstruct.scene_postpass(empty, 32, 26, 2, mesh=True, mesh_cell=1)


def _check_empty_chain(mesh, got, combo):
    """run_chain's result on the empty mesh: the key sets, shapes and dtypes of the three stages."""
    fill, smooth, cell = combo
    assert list(got) == mc.asked(combo)
    if fill is not None:
        e = got["filled"]
        assert set(e) == {"vertices", "vert_lattice", "faces", "loop_root", "loop_len", "vert_loop", "vert_src"} | set(mesh.FILL_COUNTS)
        assert e["vertices"].shape == (0, 3) and e["vertices"].dtype == np.float32 and e["vert_lattice"].dtype == np.float64
        assert e["faces"].shape == (0, 3) and e["faces"].dtype == np.int32 and e["vert_src"].shape == (0,) and e["vert_src"].dtype == np.int64
        assert e["vert_loop"].shape == (0,) and e["vert_loop"].dtype == np.uint8 and all(e[k] == 0 and type(e[k]) is int for k in mesh.FILL_COUNTS)
    if smooth is not None:
        e = got["smoothed"]
        faces = "quads" if fill is None else "faces"
        assert set(e) == {"vertices", "vert_lattice", "vert_src", faces} | mc.SMOOTH_STATS
        assert e[faces].shape == (0, 4 if fill is None else 3) and e[faces].dtype == np.int32
        assert e["vertices"].shape == (0, 3) and e["vertices"].dtype == np.float32 and e["vert_lattice"].shape == (0, 3)
        assert e["vert_flags"].dtype == np.uint8 and e["vert_degree"].dtype == np.int32 and e["n_edges"] == 0 and e["vert_src"].dtype == np.int64
    if cell is not None:
        e = got["simplified"]
        assert set(e) == mc.SIMPLIFIED_KEYS
        assert e["faces"].shape == (0, 3) and e["faces"].dtype == np.int32 and e["vert_src"].shape == (0,) and e["vert_src"].dtype == np.int64
        assert e["vertices"].shape == (0, 3) and e["vertices"].dtype == np.float32 and e["vert_cluster"].shape == (0,) and e["vert_cluster"].dtype == np.int32


@pytest.mark.parametrize("combo", mc.COMBOS)
def test_run_chain_on_the_empty_mesh_and_the_empty_scene(combo):
    from surfacenet_amd import mesh, reconstruct
    got = mesh.run_chain(mesh.empty_mesh(), mesh.chain_settings(*combo, "mean"), (0.0, 0.0, 0.0), 1.0)
    _check_empty_chain(mesh, got, combo)
    want = mc.by_hand(mesh, mesh.empty_mesh(), combo, (0.0, 0.0, 0.0), 1.0)
    assert list(got) == list(want)
    for key in want:
        mc.same_dict(got[key], want[key])
    # the empty scene: its dict lacks param_np, viewPair_np and rgb_list; the same dicts under <name>_mesh_<key>, and no file
    empty = dict(prediction_list=[], vxl_ijk_list=[], rayPooling_votes_list=[], cube_ijk_np=np.zeros((0, 3), np.int64))
    fill, smooth, cell = combo
    kw = dict(cameraTs_np=np.zeros((2, 3)), mesh=True, unique=True, min_component=4)
    plain = reconstruct.scene_postpass(empty, 32, 26, 2, **kw)
    post = reconstruct.scene_postpass(empty, 32, 26, 2, mesh_fill=fill, mesh_smooth=smooth, mesh_cell=cell, mesh_ply_prefix="/nonexistent/x_", **kw)
    assert set(post) - set(plain) == {"%s_mesh_%s" % (name, key) for name in ("fixThresh", "adapt") for key in want}
    for name in ("fixThresh", "adapt"):
        mc.same_dict(post[name + "_mesh"], mesh.empty_mesh())
        assert all(post[name + end] == [] for end in ("_normal_list", "_unique_list", "_clean_list", "_denoised_list"))
        for key in want:
            mc.same_dict(post["%s_mesh_%s" % (name, key)], want[key])


def test_save_stage_2ply_gathers_normals_and_colours_through_vert_src(tmp_path):
    from surfacenet_amd import mesh
    import mesh_ref as mr
    rs = np.random.RandomState(3)
    normal_list = [rs.randn(3, 3).astype(np.float32), np.zeros((0, 3), np.float32), rs.randn(4, 3).astype(np.float32)]
    rgb_list = [rs.randint(1, 256, (3, 3)).astype(np.uint8), np.zeros((0, 3), np.uint8), rs.randint(1, 256, (4, 3)).astype(np.uint8)]
    src = np.asarray([5, -1, 0, 6], np.int64)
    verts = np.asarray([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    quad = dict(vertices=verts, quads=np.asarray([[0, 1, 2, 3]], np.int32), vert_src=src)
    tris = dict(vertices=verts, faces=np.asarray([[0, 1, 2], [0, 2, 3]], np.int32), vert_src=src, quads="not read when there are faces")
    flat_n, flat_c = np.concatenate(normal_list), np.concatenate(rgb_list)
    for m, k in ((quad, 4), (tris, 3)):
        path = str(tmp_path / ("m%d.ply" % k))
        mesh.save_stage_2ply(path, m, normal_list, rgb_list)
        header, v, faces = mr.parse_ply(path)
        nrm, rgb = np.stack([v["nx"], v["ny"], v["nz"]], 1), np.stack([v["red"], v["green"], v["blue"]], 1)
        assert np.array_equal(nrm[[0, 2, 3]], flat_n[[5, 0, 6]]) and not nrm[1].any() and nrm.dtype == np.float32
        assert np.array_equal(rgb[[0, 2, 3]], flat_c[[5, 0, 6]]) and not rgb[1].any() and rgb[[0, 2, 3]].all()
        assert all(len(f) == k for f in faces) and np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), verts)
        mc.check_stage_ply(path, m, normal_list, rgb_list)
        want = open(path, "rb").read()
        mesh.save_mesh_2ply(path, verts, m["faces" if k == 3 else "quads"], normal_np=nrm, rgb_np=rgb)
        assert open(path, "rb").read() == want                  # the writer underneath, given the same arrays
        for no_rgb in (None, []):
            mesh.save_stage_2ply(path, m, normal_list, no_rgb)
            header, v, _ = mr.parse_ply(path)
            assert v.dtype.names == ("x", "y", "z", "nx", "ny", "nz")
            mc.check_stage_ply(path, m, normal_list, None)
    assert src.tolist() == [5, -1, 0, 6]                        # (the gather leaves its inputs alone)
