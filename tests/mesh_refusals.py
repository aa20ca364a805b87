"""The bad meshes every mesh stage refuses in the same words (surfacenet_amd/csrc/mesh_input.h), for
tests/test_mesh_cpu.py (mesh.simplify_mesh, smooth_mesh and fill_holes, no library) and tests/test_gpu_mesh_refusals.py (the Context.mesh_*
entries, host and device form). The texts are written out: they are what the three stages said before they shared one front end."""
import numpy as np

INDEX_TEXT = "face %d names a vertex outside [0, %d)"
RANGE_TEXT = "face %d: a coordinate of one of its vertices is outside [-4, 2^21 - 8) lattice cells"      # (the library adds "(or not a number)")


def sheet(rows=4):
    """A flat sheet of rows x 4 vertices at z = 7, vertex 4 r + c at (10 + r, 10 + c, 7), each cell cut into the triangles (a, b, e) and
    (b, d, e) - a, b the cell's corners in row r, e, d those in row r + 1: 6 (rows - 1) faces; rows = 4: 16 vertices, 18 faces; rows = 51:
    204 vertices, 300 faces. Vertex (r + 1, c + 1) is first used by face 6 r + 2 c + 1. -> (verts (V,3) float64, faces (F,3) int32)."""
    r, c = np.meshgrid(np.arange(rows), np.arange(4), indexing="ij")
    v = np.stack([10.0 + r, 10.0 + c, np.full(r.shape, 7.0)], axis=-1).reshape(-1, 3)
    a = (4 * r + c)[:-1, :-1].reshape(-1)
    b, e, d = a + 1, a + 4, a + 5
    f = np.stack([np.stack([a, b, e], axis=1), np.stack([b, d, e], axis=1)], axis=1).reshape(-1, 3)
    return v, f.astype(np.int32)


def first_used_by(faces, face):
    """A vertex that face `face` names and no earlier face does."""
    seen = set(faces[:face].reshape(-1).tolist())
    fresh = [int(i) for i in faces[face] if int(i) not in seen]
    assert fresh, "face %d brings no new vertex" % face
    return fresh[0]


def bad_index(verts, faces, at, later):
    """-> (verts, faces, text): the index V at face `later` together with -1 at face `at` < later - face `at` is the one named."""
    f = faces.copy()
    f[later, 1] = verts.shape[0]
    f[at, 2] = -1
    return verts, f, INDEX_TEXT % (at, verts.shape[0])


def bad_coordinate(verts, faces, at, value):
    """-> (verts, faces, text): `value` (NaN, 2097144.0) as the y of a vertex first used by face `at`."""
    v = verts.copy()
    v[first_used_by(faces, at), 1] = value
    return v, faces, RANGE_TEXT % at
