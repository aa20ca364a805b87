"""Shared by tests/test_meshchain_cpu.py and tests/test_gpu_meshchain.py: the eight on / off combinations of the chain that follows
extract_mesh in reconstruct.scene_postpass (fill, smooth, decimate), the chain called by hand, and the check of a
stage's PLY file."""
import itertools

import numpy as np

FILL, SMOOTH, CELL = dict(max_len=16, orientation="any"), 2, 2
# (mesh_fill, mesh_smooth, mesh_cell) of scene_postpass: every subset of the three
COMBOS = [tuple(v if on else None for v, on in zip((FILL, SMOOTH, CELL), bits)) for bits in itertools.product((False, True), repeat=3)]
KEYS = ("filled", "smoothed", "simplified")                    # the chain's order, the endings of scene_postpass's <name>_mesh_<key>
SMOOTH_STATS = {"vert_degree", "vert_flags", "n_edges", "n_boundary_edges", "n_nonmanifold_edges", "n_referenced"}
SIMPLIFIED_KEYS = {"vertices", "faces", "vert_lattice", "vert_rep", "vert_count", "face_src", "vert_cluster", "vert_src"}


def asked(combo):
    """The keys of the stages a combination asks for, in the chain's order."""
    return [key for key, value in zip(KEYS, combo) if value is not None]


def by_hand(mesh, m, combo, origin, resol):
    """{key: what scene_postpass puts under <name>_mesh_<key>} for extract_mesh's dict m: fill_holes -> smooth_mesh -> simplify_mesh called
    one by one, each on the result of the one before it."""
    fill, smooth, cell = combo
    want, faces = {}, "quads"
    if fill is not None:
        want["filled"] = mesh.fill_holes(m["vert_lattice"], m["quads"], origin=origin, resol=resol, vert_src=m["vert_src"], **fill)
        m, faces = {k: want["filled"][k] for k in ("vertices", "vert_lattice", "faces", "vert_src")}, "faces"
    if smooth is not None:
        s = mesh.smooth_mesh(m["vert_lattice"], m[faces], smooth, origin=origin, resol=resol)
        m = want["smoothed"] = dict(m, **s)
    if cell is not None:
        want["simplified"] = mesh.simplify_mesh(m["vert_lattice"], m[faces], cell, "mean", origin=origin, resol=resol, vert_src=m["vert_src"])
    return want


def same_dict(got, want):
    """The same keys; arrays equal in dtype, shape and value, scalars equal."""
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k, b in want.items():
        a = got[k]
        if isinstance(b, np.ndarray):
            assert isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=b.dtype.kind == "f"), k
        else:
            assert type(a) is type(b) and a == b, k


def gathered(lists, vert_src, dtype):
    """Row vert_src of the concatenated per-voxel lists, zero where vert_src < 0."""
    flat = np.concatenate([np.asarray(a, dtype).reshape(-1, 3) for a in lists])
    out = flat[np.maximum(vert_src, 0)]
    out[vert_src < 0] = 0
    return out


def check_stage_ply(path, m, normal_list, rgb_list):
    """The PLY file at path holds the stage's vertices and faces, and normals / colours gathered through its vert_src (rgb_list None: no
    colours in the file)."""
    import mesh_ref as mr
    header, verts, faces = mr.parse_ply(path)
    want_faces = m["faces"] if "faces" in m else m["quads"]
    assert np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), m["vertices"])
    assert len(faces) == len(want_faces) and np.array_equal(np.asarray(faces).reshape(want_faces.shape), want_faces)
    assert np.array_equal(np.stack([verts["nx"], verts["ny"], verts["nz"]], 1), gathered(normal_list, m["vert_src"], np.float32))
    if rgb_list is None:
        assert not any("red" in h for h in header)
    else:
        assert np.array_equal(np.stack([verts["red"], verts["green"], verts["blue"]], 1), gathered(rgb_list, m["vert_src"], np.uint8))
