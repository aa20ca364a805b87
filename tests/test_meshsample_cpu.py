"""CPU: the numpy restatement of the mesh sampler (tests/meshsample_ref.py) and the host code around it:
evaluation.read_ply_mesh against mesh.save_mesh_2ply, and the argument checks of mesh.sample_surface, which run before the library is
touched."""
import numpy as np
import pytest

import meshsample_ref as ref

DST = 0.2


def _n(mesh, dst):
    return ref.subdivisions(mesh[0], mesh[1], dst).tolist()


def test_the_numbers_of_the_contract():
    assert _n(ref.RIGHT, 0.2) == [8]
    p, tri = ref.sample(*ref.RIGHT, 0.2)
    assert p.shape == (64, 3) and p.dtype == np.float64 and tri.dtype == np.int32 and (tri == 0).all()
    assert p[0].tolist() == [1.0 / 24.0, 1.0 / 24.0, 0.0]
    assert p[-1].tolist() == [1.0 / 24.0, 22.0 / 24.0, 0.0]
    assert _n(ref.HALF, 0.25) == [5] and _n(ref.HALF, 0.2) == [6]
    assert _n(ref.QUAD, 0.2) == [3, 3]
    p, tri = ref.sample(*ref.QUAD, 0.2)
    assert p.shape == (18, 3) and tri.tolist() == [0] * 9 + [1] * 9


def test_a_degenerate_triangle_gives_one_sample_at_A():
    p, tri = ref.sample(*ref.DEGENERATE, 0.2)
    assert p.tolist() == [[0.25, -1.5, 3.0]] and tri.tolist() == [0]


def test_an_exact_square_is_not_rounded_up():
    v = np.asarray([[0.0, 0, 0], [2.0, 0, 0], [1.0, 0, 0]])
    assert _n((v, ref.RIGHT[1]), 0.5) == [4]                  # q = 16 exactly
    assert _n((v, ref.RIGHT[1]), np.nextafter(0.5, 0)) == [5]
    k = np.asarray([0, 1, 3, 4, 8, 9, (1 << 30) - 1, 1 << 30, 32767 * 32767 - 1, 32767 * 32767], np.int64)
    assert ref.isqrt(k).tolist() == [0, 1, 1, 2, 2, 3, 32767, 32768, 32766, 32767]


@pytest.mark.parametrize("mesh", [ref.RIGHT, ref.SCALENE, ref.NEEDLE, ref.QUAD], ids=["right", "scalene", "needle", "quad"])
def test_samples_are_distinct_and_average_to_the_centroid(mesh):
    v, f = mesh
    p, tri = ref.sample(v, f, DST)
    assert np.unique(p, axis=0).shape[0] == p.shape[0]
    for i in range(f.shape[0]):
        assert np.abs(p[tri == i].mean(axis=0) - v[f[i]].mean(axis=0)).max() <= 1e-12


@pytest.mark.parametrize("mesh", [ref.RIGHT, ref.SCALENE, ref.NEEDLE], ids=["right", "scalene", "needle"])
def test_every_surface_point_is_within_two_thirds_dst_of_a_sample(mesh):
    v, f = mesh
    p, _ = ref.sample(v, f, DST)
    q = ref.surface_points(v, f[0], 20000, np.random.RandomState(5))
    gap = ref.worst_gap(q, p) / DST
    print("worst gap %.3f dst over %d samples" % (gap, p.shape[0]))
    assert gap <= 2.0 / 3.0


def test_tri_and_offsets_agree_with_the_counts():
    v, f = ref.mixed_mesh()
    n = ref.subdivisions(v, f, DST)
    assert set(n.tolist()) == {1, 2, 300} and (n == 1).sum() > 1000 and (n == 2).sum() > 1000
    assert n[2500] == 300 and n[2501] == 1
    off = ref.offsets(n)
    p, tri = ref.sample(v, f, DST)
    assert off[0] == 0 and off[-1] == p.shape[0] == int((n * n).sum()) and tri.dtype == np.int32
    assert np.array_equal(np.bincount(tri, minlength=f.shape[0]), n * n)
    assert (np.diff(tri) >= 0).all() and np.array_equal(np.searchsorted(tri, np.arange(f.shape[0])), off[:-1])
    assert p[off[2501]].tolist() == [1.0, 2.0, 3.0]


def test_the_restatement_names_the_first_bad_face():
    v, f = ref.QUAD
    with pytest.raises(ValueError, match="face 1 names"):
        ref.sample(v, np.asarray([[0, 1, 2], [0, 2, 4]]), DST)
    with pytest.raises(ValueError, match="face 0 names"):
        ref.sample(v, np.asarray([[0, -1, 2], [0, 2, 9]]), DST)
    bad = v.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="face 1 has"):
        ref.sample(bad, f, DST)
    assert ref.sample(bad, f[:1], DST)[0].shape == (9, 3)     # an unreferenced vertex is not looked at
    far = v.copy()
    far[1, 0] = 7000.0
    with pytest.raises(ValueError, match="face 0 needs"):
        ref.sample(far, f, DST)
    for dst in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="dst"):
            ref.sample(v, f, dst)
    assert ref.sample(v, np.zeros((0, 3), np.int32), DST)[0].shape == (0, 3)
    with pytest.raises(ValueError, match="face 2 takes"):
        ref.offsets(np.asarray([32768, 32767, 256, 1], np.int64))      # 2^30 + (2^30 - 65535) + 65536 = 2^31 + 1
    assert ref.offsets(np.asarray([32768, 32767, 255, 22, 5], np.int64))[-1] == (1 << 31) - 1


# ---- host code: PLY meshes ---------------------------------------------------------------------------------------------------------------------
def _mesh(quads):
    rs = np.random.RandomState(3)
    v = rs.uniform(-5, 5, (7, 3)).astype(np.float32)
    f = rs.randint(0, 7, (5, 4 if quads else 3)).astype(np.int32)
    return v, f, rs.normal(0, 1, (7, 3)).astype(np.float32), rs.randint(0, 256, (7, 3)).astype(np.uint8)


@pytest.mark.parametrize("quads", [False, True])
@pytest.mark.parametrize("normals,colours", [(False, False), (True, False), (False, True), (True, True)])
def test_read_ply_mesh_reads_what_save_mesh_2ply_writes(tmp_path, quads, normals, colours):
    from surfacenet_amd import evaluation, mesh
    v, f, nrm, rgb = _mesh(quads)
    path = str(tmp_path / "m.ply")
    mesh.save_mesh_2ply(path, v, f, normal_np=nrm if normals else None, rgb_np=rgb if colours else None)
    gv, gf = evaluation.read_ply_mesh(path)
    assert gv.dtype == np.float32 and gf.dtype == np.int32 and np.array_equal(gv, v) and np.array_equal(gf, f)
    assert np.array_equal(evaluation.read_ply_xyz(path), v)
    mesh.save_mesh_2ply(path, v, f[:0])
    gv, gf = evaluation.read_ply_mesh(path)
    assert np.array_equal(gv, v) and gf.shape == (0, 3) and gf.dtype == np.int32


def _write(path, fmt, v, faces, extra=False):
    """A PLY written by hand: double vertices with a uchar property between them, `ushort int` face lists (+ a scalar face property)."""
    end = {"binary_little_endian": "<", "binary_big_endian": ">"}.get(fmt)
    head = ["ply", "format %s 1.0" % fmt, "comment by hand", "element vertex %d" % len(v), "property double x", "property uchar flag",
            "property double y", "property double z", "element face %d" % len(faces)]
    head += (["property uchar kind"] if extra else []) + ["property list ushort int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        if end is None:
            for row in v:
                fh.write(("%r 7 %r %r\n" % tuple(float(x) for x in row)).encode("ascii"))
            for face in faces:
                fh.write(((("3 " if extra else "") + "%d " % len(face)) + " ".join(str(i) for i in face) + "\n").encode("ascii"))
        else:
            rec = np.zeros(len(v), dtype=[("x", end + "f8"), ("flag", "u1"), ("y", end + "f8"), ("z", end + "f8")])
            rec["x"], rec["flag"], rec["y"], rec["z"] = v[:, 0], 7, v[:, 1], v[:, 2]
            fh.write(rec.tobytes())
            for face in faces:
                fh.write((b"\x03" if extra else b"") + np.asarray([len(face)], end + "u2").tobytes() + np.asarray(face, end + "i4").tobytes())


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
@pytest.mark.parametrize("extra", [False, True])
def test_read_ply_mesh_formats_and_mixed_faces(tmp_path, fmt, extra):
    from surfacenet_amd import evaluation
    v = np.random.RandomState(4).uniform(-3, 3, (6, 3))
    path = str(tmp_path / "hand.ply")
    for faces in ([[0, 1, 2], [2, 3, 5], [5, 4, 0]], [[0, 1, 2, 3], [2, 3, 4, 5]]):
        _write(path, fmt, v, faces, extra)
        gv, gf = evaluation.read_ply_mesh(path)
        assert gv.dtype == np.float64 and np.array_equal(gv, v) and gf.dtype == np.int32 and np.array_equal(gf, np.asarray(faces))
    for faces in ([[0, 1, 2], [2, 3, 4, 5]], [[0, 1, 2, 3], [2, 3, 4]], [[0, 1, 2], [1, 2, 3], [2, 3, 4, 5]]):
        _write(path, fmt, v, faces, extra)
        with pytest.raises(ValueError, match="mixed size"):
            evaluation.read_ply_mesh(path)
    _write(path, fmt, v, [[0, 1], [2, 3]], extra)
    with pytest.raises(ValueError, match="triangles and quads"):
        evaluation.read_ply_mesh(path)


def test_read_ply_mesh_needs_vertices_and_faces(tmp_path):
    from surfacenet_amd import evaluation, sparseCubes
    path = str(tmp_path / "cloud.ply")
    sparseCubes.save2ply(path, np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError, match="face element"):
        evaluation.read_ply_mesh(path)


# ---- host code: argument checks before the library -----------------------------------------------------------------------------------------------
def test_sample_surface_refuses_bad_arguments_without_a_library(monkeypatch):
    from surfacenet_amd import mesh, runtime

    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(runtime, "any_context", no_library)
    v, f = ref.QUAD
    for bad_v in (v[:, :2], v.reshape(-1), v.astype(np.int64), v.astype(np.float16)):
        with pytest.raises(ValueError, match="vertices"):
            mesh.sample_surface(bad_v, f)
    for bad_f in (f[:, :2], f.reshape(-1), f.astype(np.float64), np.zeros((2, 5), np.int32)):
        with pytest.raises(ValueError, match="faces"):
            mesh.sample_surface(v, bad_f)
    with pytest.raises(ValueError, match="int32"):
        mesh.sample_surface(v, np.asarray([[0, 1, 1 << 31]], np.int64))
    for dst in (0.0, -0.2, np.inf, np.nan, "dense", None):
        with pytest.raises(ValueError, match="dst"):
            mesh.sample_surface(v, f, dst)
    with pytest.raises(AssertionError, match="touched"):      # good arguments do reach the library
        mesh.sample_surface(v.astype(np.float32), f)
