"""CPU: the numpy restatement of the mesh simplifier (tests/meshsimplify_ref.py) pinned on hand-made cases and on the
mesher's own meshes, and the argument checks of mesh.simplify_mesh and reconstruct.scene_postpass, which run before the library is touched."""
import numpy as np
import pytest

import meshsimplify_ref as ref


def _bound(k):
    return np.sqrt(3.0) * k + 1.0 / 256.0                       # contract 14: a member and its output vertex lie in one cell of side k


# ---- the sheet, by hand --------------------------------------------------------------------------------------------------------------------------
def test_sheet_by_hand():
    v, f = ref.sheet_case()
    assert v.shape == (81, 3) and f.shape == (128, 3) and v[9 * 3 + 5].tolist() == [3.0, 5.0, 7.0]
    r = ref.simplify(v, f, 4)
    grid = [1.5, 5.5, 8.0]
    assert r["vert_lattice"].tolist() == [[x, y, 7.0] for x in grid for y in grid]
    assert r["vert_count"].tolist() == [16, 16, 4, 16, 16, 4, 4, 4, 1]
    assert r["vert_rep"].tolist() == [20, 24, 26, 56, 60, 62, 74, 78, 80]
    assert r["collapsed"] == 120 and r["duplicates"] == 0
    assert r["faces"].tolist() == [[0, 3, 4], [0, 4, 1], [1, 4, 5], [1, 5, 2], [3, 6, 7], [3, 7, 4], [4, 7, 8], [4, 8, 5]]
    assert r["face_src"].tolist() == [54, 55, 62, 63, 118, 119, 126, 127]
    assert np.array_equal(r["vertices"], r["vert_lattice"].astype(np.float32))
    ref.check_invariants(v, f, r)
    m = ref.simplify(v, f, 4, placement=1, origin=(1.0, 2.0, 3.0), resol=0.5)
    assert np.array_equal(m["vert_lattice"], v[r["vert_rep"]])
    assert np.array_equal(m["vertices"], (np.asarray([1.0, 2.0, 3.0]) + 0.5 * v[r["vert_rep"]]).astype(np.float32))
    for key in ("vert_rep", "vert_count", "faces", "face_src", "vert_cluster"):
        assert np.array_equal(m[key], r[key]), key
    for key in ref.KEYS:
        assert r[key].dtype == dict(vertices=np.float32, vert_lattice=np.float64).get(key, np.int32), key


# ---- every rule decides something ----------------------------------------------------------------------------------------------------------------
def test_every_rule_decides_something():
    v, f = ref.rules_case()
    r = ref.simplify(v, f, 4)
    assert r["vert_lattice"].tolist() == [[1.25, 1.1875, 1.1875], [4.5, 0.5, 0.5], [0.5, 4.5, 0.5], [-0.5, 4.5, 0.5]]
    assert r["vert_count"].tolist() == [4, 1, 1, 1]
    assert r["vert_rep"].tolist() == [9, 2, 3, 8]               # 9 and 10 tie on d: the smaller index
    assert r["faces"].tolist() == [[0, 1, 2], [0, 2, 1], [0, 1, 3]]
    assert r["face_src"].tolist() == [0, 2, 6]                  # 1 and 4 are 0 under rotation, 3 and 7 collapse; the opposite orientation stays
    assert r["collapsed"] == 3 and r["duplicates"] == 2 and r["clusters"] == 5
    assert r["vert_cluster"].tolist() == [0, 0, 1, 2, -1, -1, -1, -1, 3, 0, 0]      # 4 unreferenced; the speck 5, 6, 7 dropped; 4 -> 3
    assert v[8, 0] < 0 and np.floor_divide(np.int64(np.rint(v[8, 0] * 256)) + 1024, 1024) == 0      # a negative x lands in cell 0
    spare = v.copy()
    spare[4] = np.nan                                           # an unreferenced vertex is not looked at
    s = ref.simplify(spare, f, 4)
    for key in ref.KEYS:
        assert np.array_equal(s[key], r[key]), key
    ref.check_invariants(v, f, r)


# ---- sphere shells: closed manifolds stay closed -------------------------------------------------------------------------------------------------
SPHERES = {6: (728, 1452, {2: (176, 348), 3: (80, 156), 4: (56, 108)}),
           9: (1496, 2988, {2: (416, 828), 3: (152, 300), 4: (128, 252)}),
           12: (2720, 5436, {2: (656, 1308), 3: (272, 540), 4: (152, 300)})}


@pytest.mark.parametrize("R", [6, 9, 12])
def test_sphere_shells(R):
    v, f = ref.sphere_case(R)
    V, F, counts = SPHERES[R]
    assert v.shape == (V, 3) and f.shape == (F, 3)
    for k, (C, G) in counts.items():
        for placement in (0, 1):
            r = ref.reference("sphere%d" % R, k, placement)
            assert (r["vert_lattice"].shape[0], r["faces"].shape[0]) == (C, G), (R, k)
            edges, on = ref.tri_edge_counts(r["faces"])
            assert (on == 2).all()
            assert C - edges.shape[0] + G == 2
            assert ref.tri_volume(r["vert_lattice"], r["faces"]) > 0
            assert r["duplicates"] == 0 and r["clusters"] == C and (r["vert_cluster"] >= 0).all()
            assert ref.max_move(v, r) <= _bound(k)
            ref.check_invariants(v, f, r)


# ---- the surface scene: negative coordinates, open boundary --------------------------------------------------------------------------------------
def test_surface_scene():
    v, f = ref.surface_case()
    assert v.shape == (2398, 3) and f.shape == (4600, 3) and -0.98 < v.min() < -0.96
    for k, (C, G) in {2: (646, 1191), 3: (288, 514), 4: (179, 308), 8: (51, 76)}.items():
        r = ref.reference("surface", k)
        assert (r["vert_lattice"].shape[0], r["faces"].shape[0]) == (C, G), k
        assert r["duplicates"] == 0 and ref.max_move(v, r) <= _bound(k)
        assert ref.max_move(v, ref.reference("surface", k, 1)) <= _bound(k)
        ref.check_invariants(v, f, r)
    assert ref.reference("surface", 8)["largest"] == 107


# ---- the soup: duplicates, big clusters, the empty result ---------------------------------------------------------------------------------------
def test_soup():
    v, f = ref.soup_case()
    assert v.shape == (5000, 3) and f.shape == (20000, 3) and v.min() >= -3.5 and v.max() < 32.5
    r8, r16, r64 = ref.reference("soup", 8), ref.reference("soup", 16), ref.reference("soup", 64)
    assert r8["duplicates"] > 0 and r8["collapsed"] > 0
    assert r16["largest"] > 256 and r16["duplicates"] > r16["faces"].shape[0]
    assert r64["vert_lattice"].shape[0] == 0 and r64["faces"].shape[0] == 0 and (r64["vert_cluster"] == -1).all() and r64["clusters"] == 1
    # what this numpy's stream gave the session that wrote the contract (a change of the stream changes these, not the conditions above)
    print("soup:", [(k, r["vert_lattice"].shape[0], r["faces"].shape[0], r["duplicates"], r["collapsed"], r["largest"]) for k, r in
                    ((8, r8), (16, r16))])
    for k in (2, 8, 16, 64):
        for placement in (0, 1):
            r = ref.reference("soup", k, placement)
            ref.check_invariants(v, f, r)
            assert ref.max_move(v, r) <= _bound(k)
    spare = np.concatenate([v, [[np.nan, 0.0, 0.0]]])
    assert np.array_equal(ref.simplify(spare, f, 8)["faces"], r8["faces"])


# ---- the restatement's own errors name the first offending face ----------------------------------------------------------------------------------
def test_restatement_errors():
    v, f = ref.rules_case()
    bad = f.copy()
    bad[5, 1] = 11
    bad[6, 0] = -1
    with pytest.raises(ValueError, match="face 5 "):
        ref.simplify(v, bad, 4)
    far = v.copy()
    far[2, 1] = 2097144.0
    with pytest.raises(ValueError, match="face 0:"):
        ref.simplify(far, f, 4)
    far[2, 1] = np.nextafter(2097144.0, 0)
    far[7, 2] = np.nextafter(-4.0, -5)
    with pytest.raises(ValueError, match="face 5:"):
        ref.simplify(far, f, 4)
    far[7, 2] = -4.0
    assert ref.simplify(far, f, 4)["faces"].shape[0] > 0         # both ends of the range are legal
    with pytest.raises(ValueError, match="face 3 "):            # an index error at a smaller face wins over a range error
        nan = v.copy()
        nan[5, 0] = np.nan
        b2 = f.copy()
        b2[3, 0] = 99
        ref.simplify(nan, b2, 4)
    for kw in (dict(cell=1), dict(cell=65), dict(cell=2.5), dict(cell=4, placement=2), dict(cell=4, resol=0.0), dict(cell=4, resol=np.inf),
               dict(cell=4, origin=(0.0, np.nan, 0.0))):
        with pytest.raises(ValueError):
            ref.simplify(v, f, **kw)
    e = ref.simplify(v, f[:0], 4)
    assert e["faces"].shape == (0, 3) and e["vert_lattice"].shape == (0, 3) and (e["vert_cluster"] == -1).all()


# ---- surfacenet_amd/mesh.py and reconstruct.py: host code ----------------------------------------------------------------------------------------
def _no_library(monkeypatch):
    from surfacenet_amd import runtime

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(runtime, "any_context", no_library)


def test_simplify_mesh_checks_its_arguments_before_the_library(monkeypatch):
    from surfacenet_amd import mesh
    _no_library(monkeypatch)
    v, f = ref.rules_case()
    with pytest.raises(AssertionError, match="library was touched"):
        mesh.simplify_mesh(v, f, 4)                             # well-formed arguments get as far as the library
    with pytest.raises(AssertionError, match="library was touched"):
        mesh.simplify_mesh(v.astype(np.float32), np.asarray([[0, 2, 3, 8]]), 64, placement="member", origin=(1, 2, 3), resol=0.4, vert_src=np.arange(11))
    # contract 11, in its order
    bad = f.copy()
    bad[5, 1] = 11
    with pytest.raises(ValueError, match="face 5 "):
        mesh.simplify_mesh(v, bad, 4)
    bad[2, 2] = -1
    with pytest.raises(ValueError, match="face 2 "):
        mesh.simplify_mesh(v, bad, 4)
    for value in (np.nan, np.inf, 2097144.0, np.nextafter(-4.0, -5)):
        far = v.copy()
        far[7, 1] = value
        with pytest.raises(ValueError, match="face 5:"):
            mesh.simplify_mesh(far, f, 4)
        far[4], far[7] = far[7], v[7]                           # ... of an unreferenced vertex: not looked at
        with pytest.raises(AssertionError, match="library was touched"):
            mesh.simplify_mesh(far, f, 4)
    for cell in (1, 65, 0, -4, 2.5, "4", None, True):
        with pytest.raises(ValueError, match="cell"):
            mesh.simplify_mesh(v, f, cell)
    for placement in (0, 1, "median", None):
        with pytest.raises(ValueError, match="placement"):
            mesh.simplify_mesh(v, f, 4, placement=placement)
    for resol in (0.0, -0.4, np.inf, np.nan, "x"):
        with pytest.raises(ValueError, match="resol"):
            mesh.simplify_mesh(v, f, 4, resol=resol)
    for origin in ((0.0, np.nan, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0), "abc"):
        with pytest.raises(ValueError, match="origin"):
            mesh.simplify_mesh(v, f, 4, origin=origin)
    many = (1 << 28) + 1                                        # V and F over the limit: broadcast views, no memory behind them
    with pytest.raises(ValueError, match="2\\^28"):
        mesh.simplify_mesh(np.broadcast_to(np.zeros((1, 3), np.float32), (many, 3)), f, 4)
    with pytest.raises(ValueError, match="2\\^28"):
        mesh.simplify_mesh(v, np.broadcast_to(np.zeros((1, 3), np.int32), (many, 3)), 4)
    # P >= 2^21: a 128^3 grid of vertices two cells apart, every one its own cluster at cell = 2
    g = np.arange(128, dtype=np.float32) * 2
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    strip = np.arange(1 << 21, dtype=np.int32).reshape(-1, 1) + np.asarray([[0, 1, 2]], np.int32)
    strip = np.minimum(strip, (1 << 21) - 1)
    with pytest.raises(ValueError, match="larger cell"):
        mesh.simplify_mesh(grid, strip, 2)
    with pytest.raises(AssertionError, match="library was touched"):
        mesh.simplify_mesh(grid, strip, 4)                      # 64^3 clusters
    # shapes and dtypes
    for args in ((v[:, :2], f), (v.astype(np.int64), f), (v, f[:, :2]), (v, f.astype(np.float64)), (v.reshape(-1), f)):
        with pytest.raises(ValueError):
            mesh.simplify_mesh(*args, 4)
    with pytest.raises(ValueError, match="vert_src"):
        mesh.simplify_mesh(v, f, 4, vert_src=np.arange(10))
    # no face: the empty result without the library (contract 12)
    e = mesh.simplify_mesh(v, f[:0], 4, vert_src=np.arange(11))
    assert set(e) == {"vertices", "faces", "vert_lattice", "vert_rep", "vert_count", "face_src", "vert_cluster", "vert_src"}
    assert e["vertices"].shape == (0, 3) and e["faces"].shape == (0, 3) and e["vert_src"].shape == (0,) and e["vert_cluster"].tolist() == [-1] * 11


def test_scene_postpass_checks_mesh_cell_before_any_stage(monkeypatch):
    from surfacenet_amd import reconstruct
    _no_library(monkeypatch)
    empty = dict(prediction_list=[], vxl_ijk_list=[], rayPooling_votes_list=[], cube_ijk_np=np.zeros((0, 3), np.int64))
    cams = np.zeros((2, 3))
    with pytest.raises(ValueError, match="mesh=True"):
        reconstruct.scene_postpass(empty, 32, 26, 2, mesh_cell=2)
    with pytest.raises(ValueError, match="mesh=True"):
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh_cell=2)
    for cell in (1, 65, 2.5, "2"):
        with pytest.raises(ValueError, match="cell"):
            reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_cell=cell)
    with pytest.raises(ValueError, match="placement"):
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_cell=2, mesh_placement="median")
    plain = reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True)
    post = reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_cell=2, mesh_placement="member")
    assert set(post) - set(plain) == {"fixThresh_mesh_simplified", "adapt_mesh_simplified"}
    assert post["adapt_mesh_simplified"]["faces"].shape == (0, 3) and post["adapt_mesh_simplified"]["vert_src"].shape == (0,)
