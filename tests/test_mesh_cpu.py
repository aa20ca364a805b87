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


def test_the_three_mesh_stages_refuse_a_bad_mesh_in_the_same_words(monkeypatch):
    """One table of bad arguments through simplify_mesh, smooth_mesh and fill_holes (surfacenet_amd/mesh.py _mesh_arrays, _mesh_args): the
    same exception text from all three - up to the noun of the 2^28 limit -, raised before the library is touched. The texts are written
    out as the three said them when each had its own copy of the checks."""
    import mesh_refusals as bad
    from surfacenet_amd import mesh, runtime

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(runtime, "any_context", no_library)
    v, f = bad.sheet()
    v = np.concatenate([v, [[0.0, 0.0, 0.0]]])                  # vertex 16: no face names it
    assert v.shape == (17, 3) and f.shape == (18, 3)
    stages = dict(simplify=lambda v, f, **kw: mesh.simplify_mesh(v, f, 2, **kw), smooth=lambda v, f, **kw: mesh.smooth_mesh(v, f, **kw),
                  fill=lambda v, f, **kw: mesh.fill_holes(v, f, **kw))
    nouns = dict(simplify="triangles", smooth="faces", fill="faces")

    def refused(text, v, f, only=stages, **kw):
        for name in only:
            with pytest.raises(ValueError) as e:
                stages[name](v, f, **kw)
            assert str(e.value) == text.replace("NOUN", nouns[name]), name

    def accepted(v, f, **kw):
        for name, run in stages.items():
            with pytest.raises(AssertionError, match="library was touched"):
                run(v, f, **kw)

    accepted(v, f)
    accepted(v.astype(np.float32), f.astype(np.int64), origin=(-20.0, 3.0, 0.5), resol=0.4)
    refused("vert_lattice must be float32 or float64, not int32", v.astype(np.int32), f)
    refused("vert_lattice must be (V,3), not (17, 2)", v[:, :2], f)
    refused("faces must be (F,3) or (F,4), not (18, 5)", v, np.zeros((18, 5), np.int32))
    refused("faces must hold integers, not float64", v, f.astype(np.float64))
    refused("face 2 names a vertex outside [0, 17)", *bad.bad_index(v, f, 2, 5)[:2])
    assert bad.bad_index(v, f, 2, 5)[2] == "face 2 names a vertex outside [0, 17)"
    for value in (np.nan, 2097144.0):
        far, _, text = bad.bad_coordinate(v, f, 3, value)
        assert text == "face 3: a coordinate of one of its vertices is outside [-4, 2^21 - 8) lattice cells" and not np.array_equal(far[6], v[6])
        refused(text, far, f)
        far = v.copy()
        far[16] = value                                         # the same on the unreferenced vertex: not looked at
        accepted(far, f)
    both = bad.bad_coordinate(*bad.bad_index(v, f, 4, 5)[:2], 3, np.nan)[0]
    refused("face 4 names a vertex outside [0, 17)", both, bad.bad_index(v, f, 4, 5)[1])      # a bad index anywhere comes before the coordinates
    refused("origin = (0.0, nan, 0.0) must be three finite numbers", v, f, origin=(0.0, float("nan"), 0.0))
    refused("origin = (0.0, 1.0) must be three finite numbers", v, f, origin=(0.0, 1.0))
    refused("resol = 0 must be finite and > 0", v, f, resol=0)
    refused("origin = 'here', resol = 1.0 must be numbers", v, f, origin="here")
    refused("17 vertices, 5 entries of vert_src", v, f, only=("simplify", "fill"), vert_src=np.arange(5))
    many = np.broadcast_to(np.zeros((1, 3), np.int32), ((1 << 28) + 1, 3))      # (no memory behind it: it is refused by its shape)
    refused("17 vertices, 268435457 NOUN: at most 2^28 of either", v, many)
    # which refusal wins: the arrays, then the stage's own settings, then origin / resol, then the counts, vert_src, the faces
    refused("resol = 0 must be finite and > 0", v, many, resol=0)
    refused("17 vertices, 268435457 NOUN: at most 2^28 of either", v, many, only=("simplify", "fill"), vert_src=np.arange(5))
    refused("17 vertices, 5 entries of vert_src", *bad.bad_index(v, f, 2, 5)[:2], only=("simplify", "fill"), vert_src=np.arange(5))
    with pytest.raises(ValueError, match="cell = 1"):
        mesh.simplify_mesh(v, f, 1, resol=0)
    with pytest.raises(ValueError, match="iterations"):
        mesh.smooth_mesh(v, f, iterations=-1, resol=0)
    with pytest.raises(ValueError, match="max_len"):
        mesh.fill_holes(v, f, max_len=2, resol=0)
    with pytest.raises(ValueError, match="faces must hold integers"):
        mesh.simplify_mesh(v, f.astype(np.float64), 1)


def _offline_context():
    """A Context that was never opened: the library is loaded, the handle is null, and "device memory" is host memory - enough to follow a
    Context.mesh_* call through _host_or_device and _sized_outputs up to the entry's first check, with every argument converted."""
    import contextlib
    import ctypes
    from surfacenet_amd import _lib
    from surfacenet_amd.context import Context
    ctx = Context.__new__(Context)
    ctx._lib, ctx._h, ctx._closed = _lib.load(), None, True
    keep = []

    @contextlib.contextmanager
    def on_device(arrays, upload=True):
        keep.append([np.ascontiguousarray(a) for a in arrays])
        yield [ctypes.c_void_p(a.ctypes.data) for a in keep[-1]]
    ctx._on_device = on_device
    ctx.d2h = lambda dst, src: ctypes.memmove(dst.ctypes.data, src, dst.nbytes)
    return ctx


def test_context_mesh_wrappers_reach_their_entries_in_both_forms():
    """Context.mesh_sample, mesh_simplify, mesh_smooth and mesh_fill, host form and device form, convert every argument and call their entry:
    with a null context handle each entry refuses at its first check, and says so."""
    import mesh_refusals as bad
    from surfacenet_amd import SurfaceNetHipError
    ctx = _offline_context()
    v, f = bad.sheet()
    calls = (lambda d: ctx.mesh_sample(v, f, 0.5, device=d), lambda d: ctx.mesh_simplify(v, f, 2, device=d),
             lambda d: ctx.mesh_smooth(v, f, 2, device=d), lambda d: ctx.mesh_fill(v, f, device=d), lambda d: ctx.mesh_fill(v, f[:, [0, 1, 2, 2]], device=d))
    for call in calls:
        for device in (False, True):
            with pytest.raises(SurfaceNetHipError, match="null context"):
                call(device)
    with pytest.raises(ValueError, match="faces must be"):
        ctx.mesh_smooth(v, f.reshape(-1))


def test_context_mesh_reaches_its_entry_in_both_forms_and_only_the_device_form_takes_T():
    """Context.mesh on packed lists, host form and device form: every argument is converted and the entry - sn_mesh, sn_mesh_dev - refuses the
    null context handle at its first check. The two calls differ in one argument: the device form has T, the number of voxels, after cfg."""
    import ctypes
    from surfacenet_amd import SurfaceNetHipError
    ctx = _offline_context()
    real, calls = ctx._lib, []

    class Spy:
        def __getattr__(self, name):
            def entry(*args):
                calls.append((name, args))
                return getattr(real, name)(*args)
            return entry
    ctx._lib = Spy()
    s = mr.sheet_scene()
    T = len(s["ijk"])
    for device in (False, True):
        with pytest.raises(SurfaceNetHipError, match="null context"):
            ctx.mesh(*mr.scene_args(s), radius=2, reach=1, origin=(1.0, 2.0, 3.0), resol=0.4, cap=(7, 9), device=device)
    (host_name, host), (dev_name, dev) = calls
    assert (host_name, dev_name) == ("sn_mesh", "sn_mesh_dev") and len(host) == 17 and len(dev) == 18
    assert dev[3] == T == 25 and dev[:2] == host[:2] == (None, 1)      # handle, n cubes, cfg; then T in the device form alone
    for cfg in (host[2]._obj, dev[2]._obj):
        assert (cfg.radius, cfg.reach, cfg.stride_vox, list(cfg.origin), cfg.resol) == (2, 1, 13, [1.0, 2.0, 3.0], 0.4)
    assert host[8:10] == dev[9:11] == (7, 9)                    # the caps, after the five inputs
    for a, b in ((host[3:8], dev[4:9]), (host[10:15], dev[11:16])):      # five inputs, five outputs: pointers in both forms
        assert all(isinstance(p, ctypes.c_void_p) and p.value for p in a + b)
    assert all(isinstance(p, ctypes.POINTER(ctypes.c_longlong)) for p in host[15:] + dev[16:])


def test_sized_outputs_retries_once_copies_back_and_trims():
    """Context._sized_outputs against an entry played in Python: caps that suffice, a short cap (one retry at the counts), separate count words
    and one array of them, the host form and the device form, an entry without caps, a refusal."""
    import ctypes
    from surfacenet_amd import SurfaceNetHipError
    ctx = _offline_context()
    spec = (("a", 3, np.float32), ("b", 1, np.int32), ("whole", 1, np.uint8))
    rows = lambda name, sizes: 5 if name == "whole" else sizes[0 if name == "a" else 1]
    log = []

    def entry(words, na, nb):
        def run(caps, src, outs, counts):
            log.append(caps)
            if words:
                counts[0][1], counts[0][2] = na, nb
            else:
                counts[0][0], counts[1][0] = na, nb
            if na > caps[0] or nb > caps[1]:
                return -1
            for p, arr in zip(outs, (np.arange(3 * na, dtype=np.float32), np.arange(nb, dtype=np.int32) + 7, np.full((5,), 9, np.uint8))):
                ctypes.memmove(p, arr.ctypes.data, arr.nbytes)
            return 0
        return run
    for words, kw in ((0, {}), (4, dict(words=4, sized=(1, 2)))):
        for src in (None, ()):
            for caps, tries in (((6, 8), 1), ((4, 3), 1), ((3, 3), 2), ((0, 0), 2)):
                del log[:]
                got = ctx._sized_outputs(entry(words, 4, 3), spec, rows, caps, src, **kw)
                assert log == [caps, (4, 3)][:tries] and set(got) == {"a", "b", "whole"} | ({"counts"} if words else set())
                assert np.array_equal(got["a"], np.arange(12, dtype=np.float32).reshape(4, 3)) and got["b"].tolist() == [7, 8, 9]
                assert got["whole"].tolist() == [9] * 5 and all(a.flags["OWNDATA"] or a.base.shape == a.shape for a in got.values())
                if words:
                    assert got["counts"].tolist() == [0, 4, 3, 0] and got["counts"].dtype == np.int64
    got = ctx._sized_outputs(lambda caps, src, outs, counts: 0, spec[2:], rows, (), words=2)      # no caps: nothing to retry; unwritten is 0
    assert got["whole"].tolist() == [0] * 5 and got["counts"].tolist() == [0, 0]
    with pytest.raises(SurfaceNetHipError):
        ctx._sized_outputs(lambda caps, src, outs, counts: -1, spec, rows, (6, 8))                # SN_ERR_ARG that no count explains
    assert len(log) <= 2
