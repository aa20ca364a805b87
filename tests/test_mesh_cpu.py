"""CPU: the numpy restatement of the surface-nets mesher (tests/mesh_ref.py) on scenes whose answer is known - a flat
sheet by hand, closed sphere shells by their topology - plus the host code of surfacenet_amd/mesh.py: the PLY writer, triangulate, and the
argument checks of extract_mesh, which raise before any library call."""
import numpy as np
import pytest

import mesh_ref as mr
import normals_ref as nref


def _mesh(s, **kw):
    return mr.mesh_ref(*mr.scene_args(s), **kw)


def test_sheet_by_hand():
    s = mr.sheet_scene(z=7)
    m = _mesh(s, radius=2, reach=0)
    assert m["quads"].shape == (25, 4) and m["vert_lattice"].shape == (36, 3) and m["n_cells"] == 25
    assert (m["vert_lattice"][:, 2] == 7.0).all()
    half = [9.5, 10.5, 11.5, 12.5, 13.5, 14.5]
    assert sorted(set(m["vert_lattice"][:, 0].tolist())) == half and sorted(set(m["vert_lattice"][:, 1].tolist())) == half
    nrm = mr.quad_normals(m["vert_lattice"], m["quads"])
    assert (nrm[:, 2] > 0).all() and not nrm[:, :2].any()
    assert m["quads"].dtype == np.int32 and m["vert_cell"].dtype == np.int32 and m["vert_src"].dtype == np.int64 and m["verts_mm"].dtype == np.float32
    # every vertex takes the voxel of the nearest sheet cell (ties to the smallest x, then y): the corner vertex (9.5, 9.5) the first voxel
    assert m["vert_src"].min() == 0 and m["vert_src"].max() == 24 and m["vert_src"][0] == 0
    assert len(_mesh(s, radius=2, reach=1)["quads"]) == 49 and len(_mesh(s, radius=2, reach=2)["quads"]) == 81
    # verts_mm = float32(origin + resol * lattice)
    mm = _mesh(s, origin=(-20.0, 3.0, 0.5), resol=0.4)
    assert np.array_equal(mm["verts_mm"], (np.asarray([-20.0, 3.0, 0.5]) + 0.4 * m["vert_lattice"]).astype(np.float32))


@pytest.mark.parametrize("R", [6, 9, 12])
def test_sphere_shell_is_closed_and_outward(R):
    s = mr.sphere_scene(R)
    m = _mesh(s)
    edges, count = mr.edge_counts(m["quads"])
    print("R = %d: %d cells, %d quads, %d vertices" % (R, m["n_cells"], len(m["quads"]), len(m["vert_cell"])))
    assert (m["n_cells"], len(m["quads"])) == {6: (850, 726), 9: (2030, 1494), 12: (3518, 2718)}[R]
    assert (count == 2).all()                                  # closed: every edge between exactly two quads
    assert len(m["vert_cell"]) - len(edges) + len(m["quads"]) == 2
    assert mr.signed_volume(m["vert_lattice"], m["quads"]) > 0
    flipped = dict(s, normals=-s["normals"])
    f = _mesh(flipped)
    assert np.array_equal(f["quads"], m["quads"][:, ::-1])      # the negated field: every quad reversed ...
    for k in ("vert_cell", "vert_lattice", "verts_mm", "vert_src"):
        assert np.array_equal(f[k], m[k]), k                    # ... and nothing else
    # the same shell dealt to the cubes of a stride-13 lattice: the same mesh, vert_src aside (it indexes the packed lists)
    sp = _mesh(mr.sphere_scene(R, split=True))
    for k in ("quads", "vert_cell", "vert_lattice"):
        assert np.array_equal(sp[k], m[k]), k


def test_tilted_sheet_has_no_seam():
    s = mr.tilted_scene()
    m = _mesh(s)
    assert len(m["quads"]) == 204
    edges, count = mr.edge_counts(m["quads"])
    assert count.max() == 2
    # the sheet covers world x 4..20, y 8..13: boundary edges (one quad) lie on its rim, half a cell out, none in the interior - in particular
    # none along the cube seam between x = 17 and x = 18
    v = m["vert_lattice"]
    mid = (v[edges[:, 0]] + v[edges[:, 1]]) / 2
    interior = (mid[:, 0] > 4) & (mid[:, 0] < 20) & (mid[:, 1] > 8) & (mid[:, 1] < 13)
    assert (count[interior] == 2).all() and ((mid[interior, 0] > 17) & (mid[interior, 0] < 18)).sum() >= 5
    assert (count[~interior] == 1).sum() == (count == 1).sum() > 0


def test_surface_scene_is_manifold_where_it_is_a_surface():
    m = mr.surface_mesh_reference((2, 2, 1))
    _, count = mr.edge_counts(m["quads"])
    print("%d cells of P, %d quads, %d vertices" % (m["n_cells"], len(m["quads"]), len(m["vert_cell"])))
    assert count.max() <= 2
    assert m["n_cells"] == 2935 and len(m["quads"]) == 2300 and len(m["vert_cell"]) == 2398
    assert (m["vert_src"] >= 0).all()                           # reach 0: an end of every emitting edge is a cell of P, inside m + {0,1}^3


def test_owner_decides_and_bad_input_is_refused():
    # one cell listed by two cubes (stride 13: local 13 of cube 0 = local 0 of cube 1) with opposite normals
    cells0 = [(x, y, 13) for x in range(4, 9) for y in range(4, 9)]
    cells1 = [(x, y, 0) for x in range(4, 9) for y in range(4, 9)]
    off, ijk = nref.pack([np.asarray(cells0, np.uint8), np.asarray(cells1, np.uint8)])
    up = np.tile(np.asarray([0, 0, 1], np.float32), (25, 1))
    args = dict(offsets=off, ijk=ijk, mask=np.ones(50, bool), stride_vox=13, normals=np.concatenate([up, -up]))
    a = _mesh(dict(args, cube_ijk=np.asarray([[0, 0, 0], [0, 0, 1]])))
    # the cubes swapped, every voxel keeping its normal: now the downward normals own the cells
    b = _mesh(dict(args, cube_ijk=np.asarray([[0, 0, 1], [0, 0, 0]]), ijk=np.concatenate([ijk[25:], ijk[:25]]), normals=np.concatenate([-up, up])))
    assert a["n_cells"] == b["n_cells"] == 25 and len(a["quads"]) == len(b["quads"]) == 25
    assert (mr.quad_normals(a["vert_lattice"], a["quads"])[:, 2] > 0).all() and (mr.quad_normals(b["vert_lattice"], b["quads"])[:, 2] < 0).all()
    assert (a["vert_lattice"][:, 2] == 13.0).all() and (b["vert_lattice"][:, 2] == 13.0).all()
    assert a["vert_src"].max() < 25 and b["vert_src"].max() < 25
    s = mr.sheet_scene()
    with pytest.raises(ValueError):
        _mesh(dict(s, normals=np.full((25, 3), np.nan, np.float32)))
    with pytest.raises(ValueError):
        _mesh(dict(s, cube_ijk=np.asarray([[0, 0, ((1 << 21) - 8 - 7 + 12) // 13 + 1]])))
    with pytest.raises(ValueError):
        _mesh(s, radius=4)
    assert len(_mesh(dict(s, normals=np.zeros((25, 3), np.float32)))["quads"]) == 0


# ---- surfacenet_amd/mesh.py: host code -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tri", [False, True])
def test_ply_round_trip(tmp_path, tri):
    from surfacenet_amd import mesh
    m = _mesh(mr.sheet_scene(), origin=(1.0, 2.0, 3.0), resol=0.4)
    faces = mesh.triangulate(m["quads"]) if tri else m["quads"]
    if tri:
        assert faces.shape == (50, 3) and faces[0].tolist() == m["quads"][0, [0, 1, 2]].tolist() and faces[1].tolist() == m["quads"][0, [0, 2, 3]].tolist()
    rs = np.random.RandomState(0)
    nrm, rgb = rs.randn(36, 3).astype(np.float32), rs.randint(0, 256, (36, 3)).astype(np.uint8)
    path = str(tmp_path / "m.ply")
    mesh.save_mesh_2ply(path, m["verts_mm"], faces, normal_np=nrm, rgb_np=rgb)
    header, verts, got = mr.parse_ply(path)
    assert header == ["ply", "format binary_little_endian 1.0", "element vertex 36", "property float x", "property float y", "property float z",
                      "property float nx", "property float ny", "property float nz", "property uchar red", "property uchar green",
                      "property uchar blue", "element face %d" % len(faces), "property list uchar int vertex_indices", "end_header"]
    assert np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), m["verts_mm"])
    assert np.array_equal(np.stack([verts["nx"], verts["ny"], verts["nz"]], 1), nrm)
    assert np.array_equal(np.stack([verts["red"], verts["green"], verts["blue"]], 1), rgb)
    assert len(got) == len(faces) and all(np.array_equal(a, b) for a, b in zip(got, faces))
    mesh.save_mesh_2ply(path, m["verts_mm"], faces)             # positions only
    header, verts, got = mr.parse_ply(path)
    assert [h for h in header if h.startswith("property")] == ["property float x", "property float y", "property float z",
                                                              "property list uchar int vertex_indices"] and len(got) == len(faces)
    with pytest.raises(ValueError):
        mesh.save_mesh_2ply(path, m["verts_mm"], faces + 36)
    with pytest.raises(ValueError):
        mesh.save_mesh_2ply(path, m["verts_mm"], faces[:, :2])


def test_extract_mesh_checks_its_arguments_before_the_library(monkeypatch):
    from surfacenet_amd import mesh, runtime

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(runtime, "any_context", no_library)
    s = nref.surface_scene((2, 2, 1))
    d, param = s["lists"], s["param"]
    cube, ijk_l, masks = d["cube_ijk_np"], d["vxl_ijk_list"], s["mask_list"]
    nl = [np.zeros((len(a), 3), np.float32) for a in ijk_l]
    good = (cube, ijk_l, masks, nl, param, 13)
    with pytest.raises(AssertionError, match="library was touched"):
        mesh.extract_mesh(*good)                                # well-formed arguments get as far as the library
    for kw in (dict(radius=0), dict(radius=4), dict(radius=1.5), dict(reach=-1), dict(radius=2, reach=3), dict(reach=0.5)):
        with pytest.raises(ValueError):
            mesh.extract_mesh(*good, **kw)
    for stride in (0, 6.5):
        with pytest.raises(ValueError):
            mesh.extract_mesh(cube, ijk_l, masks, nl, param, stride)
    with pytest.raises(ValueError):
        mesh.extract_mesh(cube, ijk_l, masks, nl[:-1], param, 13)
    with pytest.raises(ValueError):
        mesh.extract_mesh(cube, ijk_l, masks, [nl[0][:-1]] + nl[1:], param, 13)
    with pytest.raises(ValueError):
        mesh.extract_mesh(cube, ijk_l, masks[:-1], nl, param, 13)
    bad = [a.copy() for a in nl]
    bad[0][np.nonzero(masks[0])[0][0], 1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        mesh.extract_mesh(cube, ijk_l, masks, bad, param, 13)
    bad[0][np.nonzero(masks[0])[0][0], 1] = 2.5
    with pytest.raises(ValueError):
        mesh.extract_mesh(cube, ijk_l, masks, bad, param, 13)
    p2 = param.copy()
    p2["resol"][1] *= 2
    with pytest.raises(ValueError, match="resol"):
        mesh.extract_mesh(cube, ijk_l, masks, nl, p2, 13)
    p3 = param.copy()
    p3["xyz"][1, 0] += np.float32(0.06 * float(param["resol"][0]))
    with pytest.raises(ValueError, match="lattice"):
        mesh.extract_mesh(cube, ijk_l, masks, nl, p3, 13)
    p4 = param.copy()
    p4["xyz"][1, 0] += np.float32(0.01 * float(param["resol"][0]))      # float32 noise of the mm coordinates is tolerated
    with pytest.raises(AssertionError, match="library was touched"):
        mesh.extract_mesh(cube, ijk_l, masks, nl, p4, 13)
    far = cube.astype(np.int64) + np.asarray([0, 0, (1 << 21) // 13])
    with pytest.raises(ValueError, match="2\\^21"):
        mesh.extract_mesh(far, ijk_l, masks, nl, param, 13)
    # no cubes: an empty mesh, no library
    e = mesh.extract_mesh(np.zeros((0, 3), np.int64), [], [], [], param[:0], 13)
    assert e["vertices"].shape == (0, 3) and e["quads"].shape == (0, 4) and e["vert_src"].shape == (0,) and e["vert_lattice"].shape == (0, 3)
    o, r = mesh.lattice_origin(cube, param, 13)
    assert r == float(np.float64(param["resol"][0])) and np.array_equal(o, param["xyz"][0].astype(np.float64) - (cube[0].astype(np.int64) * 13) * r)
