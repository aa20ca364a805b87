"""GPU (-m gpu): the mesh renderer and the vertex colours (surfacenet_amd/csrc/meshrender.h) against the restatement
tests/meshrender_ref.py, byte for byte - depth, face, face_pixels, vert_visible and the counts -, in the host form and the device form. The
restatement is fed the (h, w, z) that sn_project_points returns for the same inputs. The named cases are the smallest shapes at which a
kernel path can go wrong: both raster paths and the box size between them, ties, borders, slivers, several workgroups; then a permutation
of the faces, repeated calls on one context, the empty meshes, every refusal with nothing written, the colours, mesh.render_mesh and
mesh.colour_vertices, and reconstruct.scene_postpass(mesh_render=). Every launch is a plain bounded kernel."""
import ctypes
import os

import numpy as np
import pytest

import meshrender_ref as ref

pytestmark = pytest.mark.gpu
RENDER_DTYPES = [np.float64, np.int32, np.int32, np.uint8, np.int64]


@pytest.fixture(scope="module")
def ctx(gpu_required):
    from surfacenet_amd import runtime
    return runtime.any_context()


def _project(ctx, P, v):
    if len(v) == 0:
        return tuple(np.zeros((len(P), 0)) for _ in range(3))
    return ctx.project(v, np.asarray(P, np.float64), return_int_hw=False, return_depth=True)


def _want(ctx, P, v, f, shape, near=0.0, tol=0.0):
    return ref.render(*_project(ctx, P, v), f, shape[0], shape[1], near, tol)


def _check(ctx, P, v, f, shape, near=0.0, tol=0.0, want=None):
    want = _want(ctx, P, v, f, shape, near, tol) if want is None else want
    for device in (False, True):
        got = ctx.mesh_render(v, f, P, shape, near, tol, device=device)
        assert [got[k].dtype for k in ref.KEYS] == RENDER_DTYPES
        assert ref.same_bytes(got, want) == [], (device, ref.same_bytes(got, want), got["counts"].tolist(), want["counts"].tolist())
    return got


def _bytes(r):
    return {k: np.asarray(r[k]).tobytes() for k in ref.KEYS}


# ---- the named cases -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(ref.CASES))
def test_bit_for_bit_against_the_restatement(ctx, name):
    P, v, f, shape, near, tol = ref.CASES[name]()
    got = _check(ctx, P, v, f, shape, near, tol)
    c = dict(zip(ref.COUNTS, got["counts"].tolist()))
    if name == "sphere12":                                      # that camera, the mirrored one, the one behind the object
        assert (c["n_triangles"], c["n_clipped"], c["n_pairs"], c["n_pixels"]) == (3 * 528, 528, 2 * 2578, 2 * 1289)
        assert not got["depth"][2].any() and (got["face"][2] == -1).all() and not got["vert_visible"][2].any()
        assert (got["face"][0] >= 0).sum() == 1289 and got["vert_visible"][0].sum() == 143
    if name == "grid_on_centres":
        assert c["n_pairs"] == c["n_pixels"] == 144 and (got["face"][0][1:13, 2:14] >= 0).all()
    if name == "grid_quads":                                    # face id = t >> 1
        assert (got["face_pixels"][0][:36] == 4).all() and got["face"][0][12, 13] == 35 and got["face_pixels"][0][36] > 0
    if name == "ties":
        assert got["face_pixels"][0].tolist() == [36, 7, 19, 0, 0] and got["face"][0][1:8, 6].tolist() == [0] * 7
    if name == "big_and_small":                                 # both raster paths, the box sizes 240, 256, 272 around the constant
        assert (c["n_clipped"], c["n_degenerate"], c["n_pixels"]) == (2, 1, 96 * 128) and ref.SMALL_BOX == 256
        assert got["face_pixels"][0][0] > 5000 and (got["face_pixels"][0][2001:2007] > 0).all() and not got["vert_visible"][0][-1]
    if name == "slivers":
        assert (got["face_pixels"][0] == 0).sum() > 20 and c["n_pixels"] > 500
    if name == "one_pixel":
        assert got["depth"].shape == (1, 1, 1) and c["n_pixels"] == 1
    if name == "off_screen":
        assert c["n_rasterised"] == 2 and c["n_pairs"] == 0 and not got["depth"].any()
    if name == "many_workgroups":
        assert f.shape[0] == 4600 and got["depth"].shape == (2, 200, 300) and c["n_pixels"] > 25000


def test_a_permutation_of_the_faces(ctx):
    P, v, f, shape, near, tol = ref.CASES["many_workgroups"]()  # no two faces tie in depth at a pixel
    base = ctx.mesh_render(v, f, P, shape)
    perm = np.random.default_rng(13).permutation(f.shape[0])
    inv = np.empty_like(perm)
    inv[perm] = np.arange(f.shape[0])
    for device in (False, True):
        got = ctx.mesh_render(v, np.ascontiguousarray(f[perm]), P, shape, device=device)
        assert ref.same_bytes(got, base, ("depth", "vert_visible", "counts")) == []
        assert np.array_equal(got["face"], np.where(base["face"] >= 0, inv[base["face"]], -1))
        assert np.array_equal(got["face_pixels"], base["face_pixels"][:, perm])


def test_run_twice_then_grow_the_workspace_and_come_back(ctx):
    small, large = ref.CASES["grid_quads"](), ref.CASES["many_workgroups"]()
    args = lambda case: (case[1], case[2], case[0], case[3])   # Context.mesh_render takes the mesh first
    first = _bytes(ctx.mesh_render(*args(small)))
    assert _bytes(ctx.mesh_render(*args(small))) == first
    assert ref.same_bytes(ctx.mesh_render(*args(large)), _want(ctx, *large[:4])) == []
    assert _bytes(ctx.mesh_render(*args(small))) == first and _bytes(ctx.mesh_render(*args(small), device=True)) == first
    assert ref.same_bytes(ctx.mesh_render(*args(small)), _want(ctx, *small[:4])) == []
    only = ctx.mesh_render(*args(small), outputs=("depth",))   # the optional outputs: without the id pass, the same depth
    assert set(only) == {"depth", "counts"} and only["depth"].tobytes() == first["depth"] and only["counts"].tobytes() == first["counts"]
    assert _bytes(dict(ctx.mesh_render(*args(small), outputs=("face_pixels", "vert_visible", "face")), depth=only["depth"])) == first


def test_empty_meshes(ctx):
    P = np.stack([ref.PINHOLE, ref.CAM])
    v = ref.at([(3.2, 4.7, 1.0), (30.0, 4.0, 2.0), (3.0, 60.0, 1.0), (-1.0, 2.0, 1.0), (3.0, 4.0, -1.0)])
    v = np.concatenate([v, [(np.nan, 0.0, 1.0)]])
    for vv, ff in ((v, np.zeros((0, 3), np.int32)), (v, np.zeros((0, 4), np.int32)), (np.zeros((0, 3)), np.zeros((0, 3), np.int32))):
        got = _check(ctx, P, vv, ff, (37, 53), 0.5, 0.0)
        assert got["depth"].shape == (2, 37, 53) and not got["depth"].any() and (got["face"] == -1).all()
        assert got["face_pixels"].shape == (2, 0) and got["vert_visible"].shape == (2, len(vv))
        if len(vv):                                             # rule 8 with every pixel empty: in front of near, nearest pixel in the image
            assert got["vert_visible"][0].tolist() == [1, 1, 0, 0, 0, 0] and got["counts"].tolist()[:6] == [0] * 6


# ---- refusals: SN_ERR_ARG / SN_ERR_STATE, nothing written except counts ----------------------------------------------------------------------------------
def _raw(ctx, v, f, P, shape, near=0.0, tol=0.0, V=None, device=False, nv=None, counts=True, lib_ctx=None):
    """sn_mesh_render[_dev] on sentinel-filled outputs -> (status, text, the four outputs, counts)."""
    from surfacenet_amd import _lib
    c = lib_ctx or ctx
    v, f = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.int32)
    P = None if P is None else np.ascontiguousarray(P, np.float64)
    V = (len(P) if P is not None else 1) if V is None else V
    n, F, H, W = len(v), len(f), max(shape[0], 1), max(shape[1], 1)
    nvv = f.shape[1] if nv is None else nv
    Vn = max(V, 1)
    outs = [np.full((Vn, min(H, 64), min(W, 64)), 7.5), np.full((Vn, min(H, 64), min(W, 64)), 77, np.int32), np.full((Vn, F), 77, np.int32), np.full((Vn, n), 77, np.uint8)]
    cnt = (ctypes.c_longlong * 8)(*([55] * 8))
    cfg = _lib.MeshRenderCfg(int(shape[0]), int(shape[1]), float(near), float(tol))
    args = lambda ins, dst: (c._h, ctypes.byref(cfg), n, ins[0], F, nvv, ins[1], V, ins[2] if P is not None else None, *dst, cnt if counts else None)
    if not device:
        rc = c._lib.sn_mesh_render(*args([_lib.ptr(v), _lib.ptr(f), _lib.ptr(P)], [_lib.ptr(o) for o in outs]))
    else:
        with c._on_device([v, f] + ([P] if P is not None else [])) as src, c._on_device(outs) as dst:
            rc = c._lib.sn_mesh_render_dev(*args(list(src) + [None], dst))
            for o, d in zip(outs, dst):
                if o.nbytes:
                    c.d2h(o, d)
    return rc, _lib.last_error(), outs, list(cnt)


def _untouched(outs):
    return (outs[0] == 7.5).all() and all((o == 77).all() for o in outs[1:])


def test_refusals_write_nothing_but_the_counts(ctx):
    import mesh_refusals as bad
    P, v, f, shape, _, _ = ref.CASES["borders"]()
    assert shape == (37, 53)
    index = f.copy()
    index[9, 1] = len(v)
    index[4, 2] = -1
    coord = v.copy()
    coord[f[7, 0], 1] = np.nan                                  # (a soup: vertex f[7, 0] belongs to face 7 alone)
    inf = v.copy()
    inf[f[11, 2], 0] = np.inf
    both = index.copy()
    both[2, 0] = f[7, 0]                                        # face 2 now names the bad coordinate, face 4 the bad index: the smaller face is named
    nanP = np.stack([ref.PINHOLE, ref.PINHOLE])
    nanP[1, 2, 1] = np.nan
    ARG = -1
    cases = [(dict(f=index), ARG, bad.INDEX_TEXT % (4, len(v))), (dict(v=coord), ARG, "face 7: a coordinate of one of its vertices is not finite"),
             (dict(v=inf), ARG, "face 11: a coordinate of one of its vertices is not finite"),
             (dict(v=coord, f=both), ARG, "face 2: a coordinate of one of its vertices is not finite"),
             (dict(nv=2), ARG, "nv = 2"), (dict(nv=5), ARG, "nv = 5"), (dict(shape=(0, 53)), ARG, "H = 0"), (dict(shape=(37, 16385)), ARG, "W = 16385"),
             (dict(V=0), ARG, "V = 0"), (dict(V=-2), ARG, "V = -2"), (dict(near=-1.0), ARG, "near"), (dict(near=np.inf), ARG, "near"),
             (dict(tol=-0.5), ARG, "tol"), (dict(tol=np.nan), ARG, "tol"), (dict(P=nanP), ARG, "P: entry 9 of view 1 is not finite")]
    for kw, status, text in cases:
        said = set()
        for device in (False, True):
            rc, msg, outs, cnt = _raw(ctx, kw.get("v", v), kw.get("f", f), kw.get("P", P), kw.get("shape", shape), kw.get("near", 0.0), kw.get("tol", 0.0),
                                      V=kw.get("V"), device=device, nv=kw.get("nv"))
            assert rc == status and text in msg and _untouched(outs) and cnt == [0] * 8, (kw.keys(), device, rc, msg, cnt)
            said.add(msg)
        assert len(said) == 1
    rc, msg, outs, cnt = _raw(ctx, v, f, P, shape, counts=False)
    assert rc == ARG and "counts" in msg and _untouched(outs)
    rc, msg, outs, cnt = _raw(ctx, v, f, P, shape)              # and the same arrays go through when nothing is wrong
    assert rc == 0 and cnt[0] == 20 and not _untouched(outs)


def test_too_many_items_and_cameras_that_were_never_set(ctx):
    import surfacenet_amd
    from surfacenet_amd import _lib
    cfg = _lib.MeshRenderCfg(4, 4, 0.0, 0.0)
    cnt = (ctypes.c_longlong * 8)(*([55] * 8))
    one = np.zeros((4, 3))
    for n, F, word in (((1 << 28) + 1, 0, "n_verts"), (1, (1 << 28) + 1, "n_faces")):      # judged before any array is read
        for fn in (ctx._lib.sn_mesh_render, ctx._lib.sn_mesh_render_dev):
            assert fn(ctx._h, ctypes.byref(cfg), n, _lib.ptr(one), F, 3, _lib.ptr(one), 1, _lib.ptr(one), None, None, None, None, cnt) == -1
            assert word in _lib.last_error() and "2^28" in _lib.last_error() and list(cnt) == [0] * 8
    fresh = surfacenet_amd.Context(32, 1)                       # no sn_set_cameras, no sn_set_images on this one
    P, v, f, shape, _, _ = ref.CASES["off_screen"]()
    for device in (False, True):
        rc, msg, outs, cnt = _raw(ctx, v, f, None, shape, V=1, device=device, lib_ctx=fresh)
        assert rc == -2, rc                                  # SN_ERR_STATE
        assert "sn_set_cameras" in msg and _untouched(outs) and cnt == [0] * 8
    with pytest.raises(surfacenet_amd.SurfaceNetHipError, match=r"sn_set_images.*status -2"):
        fresh.mesh_vertex_colors(v, f, P, shape, np.ones((1, len(v)), np.uint8))
    fresh.set_cameras(np.stack([ref.PINHOLE, ref.CAM]))         # P = NULL: the context's cameras, and their count
    got = fresh.mesh_render(v, f, None, shape)
    assert got["depth"].shape == (2, 37, 53) and ref.same_bytes(got, _want(fresh, np.stack([ref.PINHOLE, ref.CAM]), v, f, shape)) == []


# ---- colours ---------------------------------------------------------------------------------------------------------------------------------------------
def test_colours_against_the_restatement(ctx):
    import surfacenet_amd
    P1, v, f, shape, near, tol = ref.CASES["borders"]()
    v = np.concatenate([v, ref.at([(3.5, 4.5, 1.0), (36.4, 52.4, 2.0), (-0.4, 0.2, 1.0), (40.0, 3.0, 1.0), (5.0, 5.0, -1.0)]), [(np.nan, 1.0, 1.0)]])
    P = np.stack([P1[0], ref.look_at(v, shape, 2), ref.look_at(v, shape, 0)])
    rng = np.random.default_rng(5)
    images = rng.integers(0, 256, (3,) + shape + (3,), dtype=np.uint8)
    ctx.set_images(list(images))
    hwz = _project(ctx, P, v)
    vis = ctx.mesh_render(v, f, P, shape, near, tol)["vert_visible"]
    ones = np.ones_like(vis)
    odd = (rng.integers(0, 3, vis.shape) * 100).astype(np.uint8)        # any non-zero byte counts
    for given in (vis, ones, odd):
        want = ref.colours(*hwz, given, images)
        for device in (False, True):
            got = ctx.mesh_vertex_colors(v, f, P, shape, given, device=device)
            assert [got[k].dtype for k in ("vert_views", "vert_rgb", "counts")] == [np.int32, np.uint8, np.int64]
            assert ref.same_bytes(got, want, ("vert_views", "vert_rgb", "counts")) == [], (device, got["counts"], want["counts"])
    assert want["vert_views"].max() == 3 and (want["vert_views"] == 0).any() and (ref.colours(*hwz, ones, images)["vert_views"][-6:-1] > 0).all()
    # images of the wrong count or shape; a bad mesh in the render's words
    ARG = "status -1"
    with pytest.raises(surfacenet_amd.SurfaceNetHipError, match="3 images are set for 2 views.*" + ARG):
        ctx.mesh_vertex_colors(v, f, P[:2], shape, vis[:2])
    with pytest.raises(surfacenet_amd.SurfaceNetHipError, match="image 0 is 37 x 53, not H x W = 53 x 37.*" + ARG):
        ctx.mesh_vertex_colors(v, f, P, shape[::-1], vis)
    ctx.set_images([images[0], images[1], images[2][:, :40]])
    with pytest.raises(surfacenet_amd.SurfaceNetHipError, match="image 2 is 37 x 40.*" + ARG):
        ctx.mesh_vertex_colors(v, f, P, shape, vis)
    ctx.set_images(list(images))
    index = f.copy()
    index[3, 0] = len(v)
    for device in (False, True):
        with pytest.raises(surfacenet_amd.SurfaceNetHipError, match=r"face 3 names a vertex outside \[0, %d\)" % len(v)):
            ctx.mesh_vertex_colors(v, index, P, shape, vis, device=device)
        with pytest.raises(surfacenet_amd.SurfaceNetHipError, match="tol"):
            ctx.mesh_vertex_colors(v, f, P, shape, vis, tol=-1.0, device=device)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------------------
def test_python_layer(ctx):
    from surfacenet_amd import mesh
    P, v, f, shape, near, tol = ref.CASES["sphere12"]()
    want = _want(ctx, P, v, f, shape)
    got = mesh.render_mesh(v, f, P, shape)
    assert ref.same_bytes(dict(got, vert_visible=got["vert_visible"].astype(np.uint8), counts=want["counts"]), want) == []
    assert got["vert_visible"].dtype == bool and got["views"] == [0, 1, 2] and [got[k] for k in mesh.RENDER_COUNTS] == want["counts"][:7].tolist()
    two = mesh.render_mesh(v, f, P, shape, views=[1, 0])
    assert np.array_equal(two["depth"], want["depth"][[1, 0]]) and two["views"] == [1, 0] and two["n_pixels"] == 2 * 1289
    q = mesh.render_mesh(*ref.CASES["grid_quads"]()[1:3], ref.GRID_CAM[None], (16, 16))
    assert q["face_pixels"].shape == (1, 37) and q["n_triangles"] == 74
    rng = np.random.default_rng(9)
    images = list(rng.integers(0, 256, (3,) + shape + (3,), dtype=np.uint8))
    hwz = _project(ctx, P, v)
    col = mesh.colour_vertices(v, f, P, images)                 # renders first
    ref_col = ref.colours(*hwz, want["vert_visible"], np.stack(images))
    assert np.array_equal(col["vert_rgb"], ref_col["vert_rgb"]) and np.array_equal(col["vert_views"], ref_col["vert_views"])
    assert col["n_coloured"] == ref_col["counts"][0] == 266 - (ref_col["vert_views"] == 0).sum() and col["vert_views"].max() == 2
    given = mesh.colour_vertices(v, f, P, images, vert_visible=np.ones((2, 266), bool), views=[2, 0])
    ref_given = ref.colours(*(a[[2, 0]] for a in hwz), np.ones((2, 266), np.uint8), np.stack(images)[[2, 0]])
    assert np.array_equal(given["vert_rgb"], ref_given["vert_rgb"]) and np.array_equal(given["vert_views"], ref_given["vert_views"])


def _scene():
    import normals_ref as nref
    s = nref.surface_scene((2, 2, 1))
    d = s["lists"]
    out = dict(prediction_list=d["prediction_list"], vxl_ijk_list=d["vxl_ijk_list"], rayPooling_votes_list=d["rayPooling_votes_list"],
               cube_ijk_np=d["cube_ijk_np"], param_np=s["param"], viewPair_np=s["viewPair"], rgb_list=d["rgb_list"])
    return s, d, out


def test_in_a_scene_the_last_mesh_of_the_chain_is_rendered(gpu_required, tmp_path):
    import meshchain_util as mc
    import mesh_ref as mr
    from surfacenet_amd import evaluation, mesh, reconstruct
    s, d, out = _scene()
    kw = dict(tau=0.7, gamma=0.5, N_refine_iter=2, cameraTs_np=s["cameraTs"], mesh=True, mesh_fill=16, mesh_cell=2)
    dirs = {}
    for tag in ("rendered", "plain", "bare"):
        dirs[tag] = tmp_path / tag
        dirs[tag].mkdir()
    plain = reconstruct.scene_postpass(out, 32, 26, 2, mesh_ply_prefix=str(dirs["plain"] / "s_"), **kw)
    none = reconstruct.scene_postpass(out, 32, 26, 2, mesh_ply_prefix=str(dirs["bare"] / "s_"), mesh_render=None, **kw)
    shape = (60, 80)
    verts = plain["adapt_mesh_simplified"]["vertices"]
    P = np.stack([ref.look_at(verts, shape, 2), ref.look_at(verts, shape, 0), ref.look_at(verts, shape, 1)])
    rng = np.random.default_rng(21)
    images = list(rng.integers(0, 256, (3,) + shape + (3,), dtype=np.uint8))
    setting = dict(cameraPOs=P, shape=shape, views=[0, 2], images=images)
    got = reconstruct.scene_postpass(out, 32, 26, 2, mesh_ply_prefix=str(dirs["rendered"] / "s_"), mesh_render=setting, **kw)
    assert set(none) == set(plain) and set(got) - set(plain) == {"fixThresh_mesh_render", "adapt_mesh_render"}
    old = sorted(os.listdir(str(dirs["plain"])))
    assert sorted(os.listdir(str(dirs["bare"]))) == old
    assert sorted(os.listdir(str(dirs["rendered"]))) == sorted(old + ["s_fixThresh_mesh_v.ply", "s_adapt_mesh_v.ply"])
    for fname in old:                                           # every other file: the bytes of the call without mesh_render
        assert open(str(dirs["plain"] / fname), "rb").read() == open(str(dirs["rendered"] / fname), "rb").read() == open(str(dirs["bare"] / fname), "rb").read()
    for key in plain:
        if key.endswith("_mesh") or "_mesh_" in key:
            mc.same_dict(got[key], plain[key])
    resol = float(np.float64(np.asarray(s["param"]["resol"], np.float32)[0]))
    for name in ("fixThresh", "adapt"):
        r, last = got[name + "_mesh_render"], got[name + "_mesh_simplified"]
        by_hand = mesh.render_mesh(last["vertices"], last["faces"], P, shape, 0.0, 0.5 * resol, views=[0, 2])      # tol=None: half the lattice's resol
        assert set(r) == set(by_hand) | {"vert_rgb", "vert_views"}
        for k in by_hand:
            assert np.array_equal(r[k], by_hand[k]) if isinstance(by_hand[k], np.ndarray) else r[k] == by_hand[k], k
        assert r["depth"].shape == (2,) + shape and r["n_pixels"] > 1000 and r["vert_visible"].any() and r["n_clipped"] == 0
        col = mesh.colour_vertices(last["vertices"], last["faces"], P, images, vert_visible=r["vert_visible"], views=[0, 2])
        assert np.array_equal(r["vert_rgb"], col["vert_rgb"]) and np.array_equal(r["vert_views"], col["vert_views"]) and (r["vert_views"] > 0).any()
        path = str(dirs["rendered"] / ("s_%s_mesh_v.ply" % name))
        pv, pf = evaluation.read_ply_mesh(path)                 # the round trip
        assert np.array_equal(pv, last["vertices"]) and np.array_equal(pf, last["faces"])
        _, rec, _ = mr.parse_ply(path)
        assert np.array_equal(np.stack([rec["red"], rec["green"], rec["blue"]], 1), r["vert_rgb"])
