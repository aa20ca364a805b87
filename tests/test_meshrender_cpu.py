"""CPU: the restatement of the mesh renderer (tests/meshrender_ref.py) pinned on the figures of its smallest cases -
the watertight sphere, pixel centres on edges and vertices, a physical anchor against the ray-plane depth, the vertex visibility of four
spheres, the colour rounding - and on a fault planted in each rule; the argument checks of mesh.render_mesh, mesh.colour_vertices and
reconstruct.scene_postpass(mesh_render=), which run before the library is touched; the new symbols in header, version script, binding and
library; and csrc/meshrender_rules.h with mrd_check_args of csrc/sn_host.h compiled alone under the sanitizers and run as a child process."""
import os
import subprocess

import numpy as np
import pytest

import meshrender_ref as ref
from test_host_plumbing import CSRC, ROOT, _compile

H, W = ref.SPHERE_HW


def _no_library(monkeypatch):
    from surfacenet_amd import runtime

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(runtime, "any_context", no_library)


def _render(P, v, f, shape, **kw):
    return ref.render(*ref.project(np.asarray(P).reshape(-1, 3, 4), v), f, shape[0], shape[1], **kw)


@pytest.fixture(scope="module")
def sphere12():
    v, f = ref.sphere(12)
    return v, f, _render(ref.CAM, v, f, (H, W))


# ---- the pinned figures ----------------------------------------------------------------------------------------------------------------------------
def test_watertight_sphere(sphere12):
    v, f, r = sphere12
    assert f.shape == (528, 3) and v.shape == (266, 3)
    assert set(np.unique(r["cover"]).tolist()) == {0, 2}        # every covered pixel exactly twice: front and back, no crack, no overlap
    assert dict(zip(ref.COUNTS, r["counts"].tolist())) == dict(n_triangles=528, n_clipped=0, n_degenerate=0, n_rasterised=528, n_pairs=2578,
                                                                n_pixels=1289, n_visible=143, reserved=0)
    hit = r["face"][0] >= 0
    assert hit.sum() == 1289 and (r["depth"][0][~hit] == 0).all() and (r["depth"][0][hit] >= 4.0).all() and (r["depth"][0][hit] < 5.0).all()
    assert r["face_pixels"].sum() == 1289 and np.array_equal(np.bincount(r["face"][0][hit], minlength=528), r["face_pixels"][0])
    assert (v[f[r["face"][0][hit]]].mean(axis=1)[:, 2] < 0).all()        # the winners are the faces towards the camera
    mirror, behind = _render(ref.CAM_MIRROR, v, f, (H, W)), _render(ref.CAM_BEHIND, v, f, (H, W))
    assert np.linalg.det(ref.CAM_MIRROR[:, :3]) < 0 and np.array_equal(mirror["cover"][0], r["cover"][0][:, ::-1][:, np.r_[95, 0:95]])
    assert behind["counts"].tolist() == [528, 528, 0, 0, 0, 0, 0, 0] and not behind["depth"].any() and (behind["face"] == -1).all()


@pytest.mark.parametrize("quads", [False, True])
def test_pixel_centres_on_edges_and_vertices(quads):
    v, f = ref.grid(quads)
    r, back = _render(ref.AFFINE, v, f, (16, 16)), _render(ref.AFFINE, *ref.grid(quads, reverse=True), (16, 16))
    want = np.zeros((16, 16), np.int32)
    want[1:13, 2:14] = 1                                        # the block is half open: rows 1 .. 12, columns 2 .. 13
    assert r["counts"][4] == 144 and np.array_equal(r["cover"][0], want) and np.array_equal(back["cover"][0], want)
    assert np.array_equal(back["depth"], r["depth"]) and (r["depth"][0][want == 1] == 1.0).all()
    assert r["face_pixels"].shape == (1, 36 if quads else 72) and r["face_pixels"].sum() == 144
    if quads:                                                   # a quad's face id is the quad's: t >> 1, four pixels each
        assert (r["face_pixels"] == 4).all() and r["face"][0][1, 2] == 0 and r["face"][0][12, 13] == 35 and r["face"][0].max() == 35
    assert r["vert_visible"].all()


def test_physical_anchor_ray_plane_depth():
    """Triangles in the plane n . X = d of the camera frame whose corners project exactly onto the 1/256 grid: zpix of every covered pixel is
    the depth at which the pixel centre's ray meets the plane."""
    n, d = np.asarray([0.3, -0.2, 1.0]), 6.0
    ray = lambda hh, ww: np.stack([(ww - 48.0) / 100.0, (hh - 32.0) / 100.0, np.ones_like(ww)], axis=-1)
    corners = np.asarray([(3 + 5 / 256, 4 + 1 / 256), (60 + 200 / 256, 20.0), (30.5, 90 + 3 / 256), (5.0, 70 + 128 / 256)])     # (h, w)
    z = d / (ray(corners[:, 0], corners[:, 1]) @ n)
    verts = ray(corners[:, 0], corners[:, 1]) * z[:, None] - np.asarray([0, 0, 5.0])
    f = np.asarray([[0, 1, 2], [0, 2, 3]], np.int32)
    h, w, zz = ref.project(ref.CAM[None], verts)
    assert np.array_equal(np.rint(h[0] * 256), corners[:, 0] * 256) and np.abs(h[0] - corners[:, 0]).max() < 1e-12
    r = ref.render(h, w, zz, f, H, W)
    hit = r["face"][0] >= 0
    ii, jj = np.nonzero(hit)
    want = d / (ray(ii.astype(np.float64), jj.astype(np.float64)) @ n)
    assert hit.sum() > 1500 and np.abs(r["depth"][0][hit] / want - 1).max() < 1e-12
    assert set(np.unique(r["cover"]).tolist()) == {0, 1}        # the shared diagonal belongs to one of the two
    flat = ref.render(h, w, zz, f, H, W, plant="affine")
    assert np.abs(flat["depth"][0][hit] / want - 1).max() > 1e-3      # interpolating z itself is not perspective-correct


@pytest.mark.parametrize("stacks,visible,facing", [(6, 37, 25), (12, 143, 121), (24, 567, 481), (48, 2271, 1921)])
def test_vertex_visibility_misses_no_front_vertex(stacks, visible, facing):
    v, f = ref.sphere(stacks)
    r = _render(ref.CAM, v, f, (H, W))                          # tol = 0
    front = np.einsum("ij,ij->i", v, v - np.asarray([0, 0, -5.0])) < 0      # the normal of a unit sphere is the vertex itself
    vis = r["vert_visible"][0].astype(bool)
    assert (vis.sum(), front.sum()) == (visible, facing) and not (front & ~vis).any()
    assert r["counts"][6] == visible and (v[vis & ~front][:, 2] < 0.35).all()      # the others sit next to the silhouette


def test_ties_and_clipping_by_hand():
    v = np.asarray([(2, 2, 0), (10, 2, 0), (2, 10, 0), (10, 10, 0), (np.nan, 0, 0), (6, 6, 0)], np.float64)
    f = np.asarray([[3, 1, 2], [0, 1, 2], [0, 1, 2], [0, 1, 1], [0, 1, 4], [0, 5, 3]], np.int32)
    r = _render(ref.AFFINE, v, f, (12, 12))
    assert r["counts"][:4].tolist() == [6, 1, 2, 3]             # (0,1,4) clipped; (0,1,1) and the collinear (0,5,3) degenerate
    assert set(np.unique(r["face"]).tolist()) == {-1, 0, 1} and r["face_pixels"][0].tolist()[:3] == [28, 36, 0]      # face 2 never wins its tie
    assert r["vert_visible"][0].tolist() == [1, 1, 1, 1, 0, 1]
    last = _render(ref.AFFINE, v, f, (12, 12), plant="tie_last")
    assert last["face_pixels"][0].tolist()[:3] == [28, 0, 36]


# ---- a planted fault in each rule fails a named case --------------------------------------------------------------------------------------------------
def _case(name):
    if name == "sphere12":
        return (ref.CAM,) + ref.sphere(12) + ((H, W),)
    if name == "sphere12_mirror":
        return (ref.CAM_MIRROR,) + ref.sphere(12) + ((H, W),)
    if name == "grid":
        return (ref.AFFINE,) + ref.grid() + ((16, 16),)
    if name == "grid_quads":
        return (ref.AFFINE,) + ref.grid(True) + ((16, 16),)
    v = np.asarray([(2, 2, 0), (10, 2, 0), (2, 10, 0)], np.float64)
    return ref.AFFINE, v, np.asarray([[0, 1, 2], [0, 1, 2]], np.int32), (12, 12)


@pytest.mark.parametrize("plant,name,keys", [("own_flip", "grid", ("depth", "face")), ("affine", "sphere12", ("depth",)),
                                             ("tie_last", "twice", ("face", "face_pixels")), ("floor_snap", "sphere12", ("depth",)),
                                             ("swap", "sphere12", ("depth",)), ("quad_id", "grid_quads", ("face",)),
                                             ("bracket", "sphere12", ("vert_visible", "counts"))])
def test_a_planted_fault_is_seen(plant, name, keys):
    assert plant in ref.PLANTS
    P, v, f, shape = _case(name)
    want, got = _render(P, v, f, shape), _render(P, v, f, shape, plant=plant)
    assert ref.same_bytes(_render(P, v, f, shape), want) == []
    assert set(keys) <= set(ref.same_bytes(got, want)), (plant, ref.same_bytes(got, want))
    if plant == "swap":                                         # only bits of S change: the same pixels, depths within an ulp or two
        assert np.array_equal(got["face"], want["face"]) and np.abs(got["depth"] - want["depth"]).max() < 1e-14


def test_every_plant_has_a_case():
    assert set(ref.PLANTS) == {"own_flip", "affine", "tie_last", "floor_snap", "swap", "quad_id", "bracket"}


# ---- colours ------------------------------------------------------------------------------------------------------------------------------------------
def test_colour_rounding_half_up():
    V = 3
    img = np.zeros((V, 2, 2, 3), np.uint8)
    img[0, 0, 0], img[1, 0, 0], img[2, 0, 0] = (1, 2, 7), (2, 5, 7), (2, 255, 8)
    h = np.zeros((V, 4))
    w = np.zeros((V, 4))
    z = np.ones((V, 4))
    h[:, 3] = 5.0                                               # vertex 3 projects outside every image
    vis = np.asarray([[1, 1, 1, 1], [0, 1, 1, 1], [0, 0, 1, 1]], np.uint8)
    c = ref.colours(h, w, z, vis, img)
    assert c["vert_views"].tolist() == [1, 2, 3, 0]
    assert c["vert_rgb"].tolist() == [[1, 2, 7], [2, 4, 7], [2, 87, 7], [0, 0, 0]]      # 3/2 -> 2, 7/2 -> 4; 5/3 -> 2, 262/3 = 87.33, 22/3 = 7.33
    assert c["counts"].tolist() == [3, 6]
    vis[1, 0] = 7                                               # any non-zero byte is "visible"
    z[2, 2] = np.nan
    c = ref.colours(h, w, z, vis, img)
    assert c["vert_views"].tolist() == [2, 2, 2, 0] and c["vert_rgb"][0].tolist() == [2, 4, 7]


# ---- the Python layer before the library -----------------------------------------------------------------------------------------------------------
def test_check_render_args():
    from surfacenet_amd import mesh
    P = np.stack([ref.CAM, ref.CAM_MIRROR, ref.CAM_BEHIND])
    got = mesh.check_render_args(P, (64, 96))
    assert got[0].shape == (3, 3, 4) and got[1:] == ((64, 96), 0.0, 0.0, [0, 1, 2])
    got = mesh.check_render_args(P, (1, 16384), 0.5, 2, views=[2, 0])
    assert np.array_equal(got[0], P[[2, 0]]) and got[1:] == ((1, 16384), 0.5, 2.0, [2, 0])
    nanP = P.copy()
    nanP[1, 2, 3] = np.inf
    assert mesh.check_render_args(nanP, (4, 4), views=[0, 2])[4] == [0, 2]      # a camera that is not rendered is not judged
    for args, text in (((P[0], (4, 4)), "cameraPOs must have shape (V, 3, 4) with V >= 1, got (3, 4)"),
                       ((P[:0], (4, 4)), "cameraPOs must have shape (V, 3, 4) with V >= 1, got (0, 3, 4)"),
                       ((P, (0, 4)), "shape = (0, 4): (H, W), integers in 1 .. 16384"), ((P, (4, 16385)), "shape = (4, 16385): (H, W), integers in 1 .. 16384"),
                       ((P, (4.5, 4)), "shape = (4.5, 4): (H, W), integers in 1 .. 16384"), ((P, 7), "shape = 7 must be two integers (H, W)"),
                       ((P, (4, 4), -1.0), "near = -1.0 must be finite and >= 0"), ((P, (4, 4), 0, np.nan), "tol = nan must be finite and >= 0"),
                       ((P, (4, 4), "a"), "near = 'a' must be a number"), ((P, (4, 4), 0, 0, [3]), "views = [3]: at least one index, each in [0, 3)"),
                       ((P, (4, 4), 0, 0, []), "views = []: at least one index, each in [0, 3)"), ((nanP, (4, 4)), "cameraPOs of view 1 is not finite")):
        with pytest.raises(ValueError) as e:
            mesh.check_render_args(*args)
        assert str(e.value) == text


def test_render_mesh_and_colour_vertices_refuse_before_the_library(monkeypatch):
    from surfacenet_amd import mesh
    _no_library(monkeypatch)
    v, f = ref.sphere(6)
    P = ref.CAM[None]
    bad_f = f.copy()
    bad_f[9, 1] = len(v)
    bad_f[4, 2] = -1
    bad_v = v.copy()
    bad_v[f[7, 0], 1] = np.nan
    first = int(np.argmax((f == f[7, 0]).any(axis=1)))
    imgs = [np.zeros((H, W, 3), np.uint8)]
    for run in (lambda vv, ff: mesh.render_mesh(vv, ff, P, (H, W)), lambda vv, ff: mesh.colour_vertices(vv, ff, P, imgs)):
        for vv, ff, text in ((v, bad_f, "face 4 names a vertex outside [0, 62)"), (bad_v, f, "face %d: a coordinate of one of its vertices is not finite" % first),
                             (v.astype(np.int32), f, "vertices must be float32 or float64, not int32"), (v, f[:, :2], "faces must be (F,3) or (F,4), not (120, 2)")):
            with pytest.raises(ValueError) as e:
                run(vv, ff)
            assert str(e.value) == text
    with pytest.raises(ValueError, match="near = -2"):
        mesh.render_mesh(v, f, P, (H, W), near=-2)
    for images, text in (([np.zeros((H, W, 3), np.float32)], "images must be"), ([], "images must be"), (imgs * 2, "2 images for 1 cameras"),
                         ([np.zeros((H, W, 4), np.uint8)], "images must be")):
        with pytest.raises(ValueError, match=text):
            mesh.colour_vertices(v, f, P, images)
    with pytest.raises(ValueError, match=r"vert_visible must have shape \(1, 62\)"):
        mesh.colour_vertices(v, f, P, imgs, vert_visible=np.ones((2, 62), bool))
    # no vertex: without the library
    e = mesh.render_mesh(np.zeros((0, 3)), np.zeros((0, 4), np.int32), np.stack([ref.CAM] * 2), (3, 5), views=[1])
    assert e["depth"].shape == (1, 3, 5) and e["depth"].dtype == np.float64 and not e["depth"].any() and (e["face"] == -1).all() and e["face"].dtype == np.int32
    assert e["face_pixels"].shape == (1, 0) and e["vert_visible"].shape == (1, 0) and e["vert_visible"].dtype == bool and e["views"] == [1]
    assert [e[k] for k in mesh.RENDER_COUNTS] == [0] * 7 and mesh.RENDER_COUNTS == ref.COUNTS[:7]
    c = mesh.colour_vertices(np.zeros((0, 3)), np.zeros((0, 3), np.int32), P, imgs)
    assert c["vert_rgb"].shape == (0, 3) and c["vert_rgb"].dtype == np.uint8 and c["vert_views"].shape == (0,) and c["n_coloured"] == 0


def test_scene_postpass_checks_mesh_render_first_and_passes_the_empty_scene(monkeypatch, tmp_path):
    from surfacenet_amd import mesh, reconstruct
    _no_library(monkeypatch)
    empty = dict(prediction_list=[], vxl_ijk_list=[], rayPooling_votes_list=[], cube_ijk_np=np.zeros((0, 3), np.int64))
    cams = np.zeros((2, 3))
    P = np.stack([ref.CAM, ref.CAM_MIRROR])
    setting = dict(cameraPOs=P, shape=(6, 9))
    with pytest.raises(ValueError) as e:
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh_render=setting)
    assert str(e.value) == "mesh_render needs mesh=True: it renders the mesh that mesh=True extracts"
    with pytest.raises(ValueError, match="mesh_orient needs mesh=True"):      # the order: cell, smooth, fill, normals, orient, render
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh_orient="outward", mesh_render=setting)
    for value, text in ((7, "mesh_render = 7: a dict of cameraPOs, shape"), (dict(shape=(6, 9)), r"mesh_render = \['shape'\]: a dict of"),
                        (dict(setting, cell=2), "mesh_render = .*'cell'.*: a dict of"), (dict(setting, shape=(0, 9)), r"shape = \(0, 9\)"),
                        (dict(setting, tol=-1), "tol = -1"), (dict(setting, views=[2]), r"views = \[2\]"),
                        (dict(setting, images=[np.zeros((6, 9, 3), np.uint8)]), "images must be one"),
                        (dict(setting, images=[np.zeros((6, 8, 3), np.uint8)] * 2), r"one \(6, 9, 3\) uint8 array per camera")):
        with pytest.raises(ValueError, match=text):
            reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_render=value)
    kw = dict(cameraTs_np=cams, mesh=True, mesh_smooth=2)
    plain, none = reconstruct.scene_postpass(empty, 32, 26, 2, **kw), reconstruct.scene_postpass(empty, 32, 26, 2, mesh_render=None, **kw)
    imgs = [np.full((6, 9, 3), 9, np.uint8)] * 2
    post = reconstruct.scene_postpass(empty, 32, 26, 2, mesh_render=dict(setting, views=[1], images=imgs), mesh_ply_prefix=str(tmp_path / "x_"), **kw)
    assert set(none) == set(plain) and set(post) - set(plain) == {"fixThresh_mesh_render", "adapt_mesh_render"}
    assert os.listdir(str(tmp_path)) == []                      # an empty scene writes no file
    r = post["adapt_mesh_render"]
    assert set(r) == {"depth", "face", "face_pixels", "vert_visible", "views", "vert_rgb", "vert_views"} | set(mesh.RENDER_COUNTS)
    assert r["depth"].shape == (1, 6, 9) and r["views"] == [1] and r["vert_rgb"].shape == (0, 3) and r["face_pixels"].shape == (1, 0)
    assert set(reconstruct.scene_postpass(empty, 32, 26, 2, mesh_render=setting, **kw)["fixThresh_mesh_render"]) == set(r) - {"vert_rgb", "vert_views"}


def test_save_stage_2ply_takes_the_view_colours(tmp_path):
    import mesh_ref as mr
    from surfacenet_amd import mesh
    v, f = ref.sphere(6)
    m = dict(vertices=v.astype(np.float32), faces=f, vert_src=np.arange(len(v)) % 5 - 1, vert_lattice=v)
    nrm, rgb = [np.ones((5, 3), np.float32)], [np.full((5, 3), 200, np.uint8)]
    own = (np.arange(3 * len(v)) % 251).astype(np.uint8).reshape(-1, 3)
    mesh.save_stage_2ply(str(tmp_path / "a.ply"), m, nrm, rgb)
    mesh.save_stage_2ply(str(tmp_path / "b.ply"), m, nrm, rgb, rgb_np=None)
    mesh.save_stage_2ply(str(tmp_path / "c.ply"), m, nrm, rgb, rgb_np=own)
    mesh.save_stage_2ply(str(tmp_path / "d.ply"), m, nrm, rgb_np=own)
    a, b, c, d = (open(str(tmp_path / n), "rb").read() for n in ("a.ply", "b.ply", "c.ply", "d.ply"))
    assert a == b and c == d and len(a) == len(c) and a != c
    _, verts, _ = mr.parse_ply(str(tmp_path / "c.ply"))
    assert np.array_equal(np.stack([verts["red"], verts["green"], verts["blue"]], 1), own)


# ---- the ABI: symbols are only added ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_version_script_binding_and_library():
    import fnmatch
    import re
    import __graft_entry__ as g
    g.build()
    from surfacenet_amd import _lib
    new = ("sn_mesh_render", "sn_mesh_render_dev", "sn_mesh_vertex_colors", "sn_mesh_vertex_colors_dev")
    txt = open(os.path.join(ROOT, "include", "surfacenet_hip.h")).read()
    assert "#define SN_ABI_VERSION 2" in txt and "sn_mesh_render_cfg" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    pattern = re.search(r"global:\s*([^;]+);", open(os.path.join(CSRC, "exports.map")).read()).group(1).strip()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode().split()
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert fnmatch.fnmatchcase(name, pattern), (name, pattern)
        assert name in _lib.ABI_SYMBOLS and name in exported, name
    lib = _lib.load()
    assert lib.sn_version() == 2 and all(hasattr(lib, name) for name in new)
    assert "sn_meshrender.hip" in open(os.path.join(CSRC, "Makefile")).read()
    import ctypes
    assert ctypes.sizeof(_lib.MeshRenderCfg) == 24


def test_the_rules_header_is_hip_free():
    with open(os.path.join(CSRC, "meshrender_rules.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes and all("hip/" not in i and i in ("<math.h>", "<stdint.h>", '"meshsmooth_round.h"') for i in includes), includes
    with open(os.path.join(CSRC, "meshrender.h")) as f:         # the kernels read the rules from that one place
        text = f.read()
    assert '#include "meshrender_rules.h"' in text and "rint(" not in text.split("namespace sn {", 1)[1]


# ---- the rules and the argument checks of the C entries, on the CPU --------------------------------------------------------------------------------
def test_rules_and_argument_checks_under_sanitizers(tmp_path):
    """tests/host/meshrender_check.cpp runs csrc/meshrender_rules.h - the snap at the guard band and on the half, the edge function at the
    guard's corners, the ownership of all eight directions, the depth expression and the order of its sum, the clamped span, the vertex tests,
    the colour mean - and sn_host.h's mrd_check_args over every end of every range, compiled stand-alone with
    -fsanitize=address,undefined and run as a child process."""
    exe = str(tmp_path / "meshrender_check")
    _compile(os.path.join(ROOT, "tests", "host", "meshrender_check.cpp"), exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "MESHRENDER-CHECK-OK" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
