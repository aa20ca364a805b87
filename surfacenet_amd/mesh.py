"""Surface mesh of the oriented output cloud on the MI355X: surface nets on the world voxel lattice.

    extract_mesh       vertices, quads and per-vertex source voxels from the per-cube lists plus normals.estimate_normals' normal_list
    triangulate        quads -> triangles
    sample_surface     surface samples of a mesh at the evaluation density (evaluation.mesh_compare scores them)
    simplify_mesh      the mesh made smaller by vertex clustering on a coarser lattice
    smooth_mesh        the mesh without its staircase: Taubin smoothing in fixed point, and its edge statistics
    fill_holes         the mesh with its small holes capped: boundary loops and centroid fans
    mesh_normals       the normals of a mesh from the mesh itself, area-weighted, with its exact area and volume
    orient_mesh        the faces of a mesh made to turn one way, its pieces with their exact volumes, small pieces removed
    self_intersections the pairs of faces of a mesh that cross or touch each other, exactly
    winding_number     inside, outside or on the surface: how many times the mesh winds around a point, exactly
    signed_distance    point_to_mesh's distance with winding_number's sign
    render_mesh        the mesh back in its views: depth maps, face ids, the pixels of every face, the visible vertices
    colour_vertices    the colour of every vertex from the views that see it
    chain_settings     the checked keywords of the stages that follow extract_mesh in a scene: fill, smooth, decimate, orient, check (DESIGN.md
                       section 4.19)
    run_chain          those stages, each on the result of the one before it
    save_mesh_2ply     binary little-endian PLY of a quad or triangle mesh
    save_stage_2ply    the same of a stage's mesh, normals and colours gathered through its vert_src (stage_tag: the file's tag), or with
                       the mesh's own normals

The reference ends in a point cloud: its utils/mesh_util.py only reads and writes OBJ files. The mesher looks at the scene on the world voxel
lattice - cell = cube_ijk * stride_vox + vxl_ijk - across cubes, in one GPU call (surfacenet_amd/csrc/mesh.h). Every argument check runs before
the library is touched.
"""
import collections

import numpy as np

from . import runtime
from .normals import _pack, _stride


def lattice_origin(cube_ijk_np, param_np, stride_vox):
    """-> (origin (3,) float64, resol float): the mm position of world cell (0,0,0), float64(xyz[0]) - float64(cube_ijk[0] * stride_vox) *
    float64(resol[0]). ValueError when the cubes' resol differ or a cube's own origin lies more than 0.05 * resol from it."""
    resol32 = np.asarray(param_np['resol'], dtype=np.float32).reshape(-1)
    if not np.all(resol32 == resol32[0]):
        raise ValueError("cubes of different resol do not share one voxel lattice")
    resol = float(np.float64(resol32[0]))
    if not (np.isfinite(resol) and resol > 0):
        raise ValueError("resol = %r must be finite and > 0" % (resol,))
    cube = np.asarray(cube_ijk_np, dtype=np.int64).reshape(-1, 3)
    origins = np.asarray(param_np['xyz'], dtype=np.float32).reshape(-1, 3).astype(np.float64) - (cube * int(stride_vox)).astype(np.float64) * resol
    if not np.isfinite(origins).all():
        raise ValueError("a cube's xyz is not finite")
    dev = np.abs(origins - origins[0]).max()
    if dev > 0.05 * resol:
        raise ValueError("the cubes do not share one voxel lattice: their origins differ by up to %g mm (resol %g)" % (dev, resol))
    return origins[0].copy(), resol


def empty_mesh():
    """extract_mesh's result for a scene without cubes."""
    return dict(vertices=np.zeros((0, 3), np.float32), quads=np.zeros((0, 4), np.int32), vert_src=np.zeros((0,), np.int64),
                vert_lattice=np.zeros((0, 3), np.float64))


def extract_mesh(cube_ijk_np, vxl_ijk_list, vxl_mask_list, normal_list, param_np, stride_vox, radius=2, reach=0):
    """cube_ijk_np (N,3), vxl_ijk_list[i] (iN,3) uint8, vxl_mask_list[i] (iN,) bool, normal_list[i] (iN,3) float32 as normals.estimate_normals
    returns it (zero = no normal), param_np the cube table ('xyz', 'resol'), stride_vox = cube_Dcenter * cube_overlapping_ratio; radius 1..3 the
    window of the implicit function, reach 0..radius how far from an oriented cell a face may lie.
    -> dict: vertices (V,3) float32 in mm, quads (Q,4) int32 (counter-clockwise seen from outside), vert_src (V,) int64 index into the
    concatenated voxel lists of the voxel whose colour / normal a vertex takes (-1: none), vert_lattice (V,3) float64 in cells."""
    stride = _stride(stride_vox)
    if int(radius) != radius or not 1 <= int(radius) <= 3:
        raise ValueError("radius = %r: the window radius is 1, 2 or 3 cells" % (radius,))
    if int(reach) != reach or not 0 <= int(reach) <= int(radius):
        raise ValueError("reach = %r must be an integer in 0 .. radius = %d" % (reach, int(radius)))
    offsets, ijk, mask = _pack(cube_ijk_np, vxl_ijk_list, vxl_mask_list)
    n = len(vxl_ijk_list)
    if len(normal_list) != n or len(param_np) != n:
        raise ValueError("%d cubes: %d normal lists, %d parameter rows" % (n, len(normal_list), len(param_np)))
    for i, (a, nrm) in enumerate(zip(vxl_ijk_list, normal_list)):
        if np.asarray(nrm).shape != (len(a), 3):
            raise ValueError("cube %d: %d voxels, normals of shape %r" % (i, len(a), np.asarray(nrm).shape))
    if n == 0:
        return empty_mesh()
    normals = np.concatenate([np.asarray(a, dtype=np.float32).reshape(-1, 3) for a in normal_list])
    sel = normals[mask]
    if not np.isfinite(sel).all() or (np.abs(sel) > 2).any():
        raise ValueError("a masked voxel's normal is not finite or has a component beyond 2 in magnitude")
    cube = np.asarray(cube_ijk_np, dtype=np.int64).reshape(n, 3)
    if cube.min() < 0:
        raise ValueError("cube ijk must be >= 0")
    if mask.any():
        top = (cube[np.repeat(np.arange(n), np.diff(offsets))[mask]] * stride + ijk[mask].astype(np.int64)).max()
        if top + 8 >= 1 << 21:
            raise ValueError("a masked voxel's world cell plus 8 reaches 2^21")
    origin, resol = lattice_origin(cube, param_np, stride)
    r = runtime.any_context().mesh(offsets, ijk, cube, mask, stride, normals, radius=int(radius), reach=int(reach), origin=origin, resol=resol)
    return dict(vertices=r["verts_mm"], quads=r["quads"], vert_src=r["vert_src"], vert_lattice=r["verts_lattice"])


def triangulate(quads):
    """(Q,4) -> (2Q,3): triangles (0,1,2) and (0,2,3) of every quad, in quad order."""
    q = np.asarray(quads).reshape(-1, 4)
    return np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], axis=1).reshape(-1, 3)


def _mesh_arrays(vertices, faces, name="vert_lattice"):
    """-> (vertices, faces) as arrays, as given, or ValueError: `name` must be float32 or float64 (V,3), faces integers (F,3) or (F,4)."""
    v = np.asarray(vertices)
    if v.dtype not in (np.float32, np.float64):
        raise ValueError("%s must be float32 or float64, not %s" % (name, v.dtype))
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError("%s must be (V,3), not %r" % (name, v.shape))
    f = np.asarray(faces)
    if f.ndim != 2 or f.shape[1] not in (3, 4):
        raise ValueError("faces must be (F,3) or (F,4), not %r" % (f.shape,))
    if f.dtype.kind not in "iu":
        raise ValueError("faces must hold integers, not %s" % f.dtype)
    return v, f


def _mesh_args(v, f, origin, resol, vert_src, noun):
    """What simplify_mesh, smooth_mesh and fill_holes ask of a mesh beyond _mesh_arrays, in the order the three refuse in (their own settings
    come between the two): origin three finite numbers, resol finite and > 0, at most 2^28 vertices and `noun` ("faces" / "triangles"),
    vert_src (or None) one entry per vertex, every face index in [0, V), every coordinate of a referenced vertex in [-4, 2^21 - 8) - the
    first offending face is named, as the library names it. -> (origin (3,) float64, resol, V, F, vert_src as an array or None, referenced
    (V,) bool - None without faces), or ValueError."""
    try:
        o = np.asarray(origin, dtype=np.float64).reshape(-1)
        r = float(resol)
    except (TypeError, ValueError):
        raise ValueError("origin = %r, resol = %r must be numbers" % (origin, resol))
    if o.shape != (3,) or not np.isfinite(o).all():
        raise ValueError("origin = %r must be three finite numbers" % (origin,))
    if not (np.isfinite(r) and r > 0):
        raise ValueError("resol = %r must be finite and > 0" % (resol,))
    V, F = v.shape[0], f.shape[0]
    if V > 1 << 28 or F > 1 << 28:
        raise ValueError("%d vertices, %d %s: at most 2^28 of either" % (V, F, noun))
    src = None
    if vert_src is not None:
        src = np.asarray(vert_src).reshape(-1)
        if src.shape[0] != V:
            raise ValueError("%d vertices, %d entries of vert_src" % (V, src.shape[0]))
    referenced = None
    if F:
        bad = ((f < 0) | (f >= V)).any(axis=1)
        if bad.any():
            raise ValueError("face %d names a vertex outside [0, %d)" % (int(np.argmax(bad)), V))
        referenced = np.zeros((V,), bool)
        referenced[f.reshape(-1)] = True
        with np.errstate(invalid="ignore"):
            out_of_range = referenced & ~((v >= -4.0) & (v < 2097144.0)).all(axis=1)      # (NaN fails)
        if out_of_range.any():
            first = int(np.argmax(out_of_range[f].any(axis=1)))
            raise ValueError("face %d: a coordinate of one of its vertices is outside [-4, 2^21 - 8) lattice cells" % first)
    return o, r, V, F, src, referenced


def sample_surface(vertices, faces, dst=0.2):
    """Surface samples of a mesh at density dst: vertices (V,3) float32 or float64 (converted to float64 exactly),
    faces (F,3) triangles or (F,4) quads, which go through triangulate first. -> (points (M,3) float64, tri (M,) int32): every point of a
    triangle lies within 2/3 dst of one of its samples; tri is the triangle a sample came from (tri // 2 the quad), so the colour or normal
    of a sample is a gather by the caller. ValueError on bad shapes, dtypes or dst before the library is touched."""
    v, f = _mesh_arrays(vertices, faces, "vertices")
    if f.size and (f.min() < -(1 << 31) or f.max() >= 1 << 31):
        raise ValueError("a face index does not fit int32")
    try:
        d = float(dst)
    except (TypeError, ValueError):
        raise ValueError("dst = %r must be a number" % (dst,))
    if not (np.isfinite(d) and d > 0):
        raise ValueError("dst = %r must be finite and > 0" % (dst,))
    if f.shape[1] == 4:
        f = triangulate(f)
    return runtime.any_context().mesh_sample(v.astype(np.float64), f.astype(np.int32), d)


PLACEMENTS = {"mean": 0, "member": 1}


def check_simplify_args(cell, placement):
    """-> (cell, placement code) of simplify_mesh's two settings, or ValueError."""
    try:
        k = int(cell)
    except (TypeError, ValueError):
        raise ValueError("cell = %r must be an integer" % (cell,))
    if isinstance(cell, bool) or k != cell or not 2 <= k <= 64:
        raise ValueError("cell = %r: an integer number of lattice cells in 2 .. 64" % (cell,))
    if not isinstance(placement, str) or placement not in PLACEMENTS:
        raise ValueError("placement = %r: 'mean' or 'member'" % (placement,))
    return k, PLACEMENTS[placement]


def simplify_mesh(vert_lattice, faces, cell, placement="mean", origin=(0.0, 0.0, 0.0), resol=1.0, vert_src=None):
    """A mesh made smaller by vertex clustering on a lattice of `cell` lattice cells per axis: vert_lattice (V,3)
    float32 or float64 in lattice cells as extract_mesh returns it, faces (F,3) triangles or (F,4) quads, which go through triangulate first;
    placement "mean" (the mean of a cluster's members) or "member" (the member nearest the cluster cell's centre); origin / resol as
    lattice_origin returns them. -> dict: vertices (C,3) float32 in mm, faces (G,3) int32, vert_lattice (C,3) float64, vert_rep (C,) int32 the
    input vertex an output vertex stands for (colour and normal are a gather by the caller), vert_count (C,) int32, face_src (G,) int32 the
    input triangle (face_src // 2 the quad), vert_cluster (V,) int32 the output vertex of an input vertex (-1: none); with vert_src (V,) also
    vert_src = vert_src[vert_rep]. Every input vertex with a cluster lies within sqrt(3) cell + 1/256 cells of its output vertex. ValueError
    on bad shapes, dtypes, settings, face indices or coordinates before the library is touched."""
    v, f = _mesh_arrays(vert_lattice, faces)
    k, code = check_simplify_args(cell, placement)
    if f.shape[1] == 4:
        f = triangulate(f)
    o, r, V, F, src, referenced = _mesh_args(v, f, origin, resol, vert_src, "triangles")
    if F and int(referenced.sum()) >= 1 << 21:                  # only then can there be 2^21 clusters: count them (a sort of the cell keys)
        c = (np.rint(v[referenced].astype(np.float64) * 256.0).astype(np.int64) + 1024) // (256 * k)
        clusters = np.unique((c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]).size
        if clusters >= 1 << 21:
            raise ValueError("cell = %d gives %d clusters, at most 2^21 - 1: choose a larger cell" % (k, clusters))
    if F == 0:                                                  # no face, no referenced vertex: nothing for the library to do
        m = dict(verts_mm=np.zeros((0, 3), np.float32), faces=np.zeros((0, 3), np.int32), verts_lattice=np.zeros((0, 3), np.float64),
                 vert_rep=np.zeros((0,), np.int32), vert_count=np.zeros((0,), np.int32), face_src=np.zeros((0,), np.int32),
                 vert_cluster=np.full((V,), -1, np.int32))
    else:
        m = runtime.any_context().mesh_simplify(v.astype(np.float64), f.astype(np.int32), k, code, origin=o, resol=r)
    res = dict(vertices=m["verts_mm"], faces=m["faces"], vert_lattice=m["verts_lattice"], vert_rep=m["vert_rep"], vert_count=m["vert_count"],
               face_src=m["face_src"], vert_cluster=m["vert_cluster"])
    if src is not None:
        res["vert_src"] = src[m["vert_rep"]]
    return res


BOUNDARIES = {"fixed": 0, "curve": 1, "free": 2}


def check_smooth_args(iterations, lam, mu, boundary):
    """-> (iterations, lam_q16, mu_q16, boundary code) of smooth_mesh's four settings, or ValueError. A factor becomes int(rint(x * 65536))."""
    try:
        n = int(iterations)
    except (TypeError, ValueError):
        raise ValueError("iterations = %r must be an integer" % (iterations,))
    if isinstance(iterations, bool) or n != iterations or not 0 <= n <= 1000:
        raise ValueError("iterations = %r: an integer in 0 .. 1000" % (iterations,))
    q = []
    for name, x in (("lam", lam), ("mu", mu)):
        try:
            w = float(x)
        except (TypeError, ValueError):
            raise ValueError("%s = %r must be a number" % (name, x))
        if isinstance(x, bool) or not np.isfinite(w) or not -1.0 <= w <= 1.0:
            raise ValueError("%s = %r: a factor in -1 .. 1" % (name, x))
        q.append(int(np.rint(w * 65536.0)))
    if not isinstance(boundary, str) or boundary not in BOUNDARIES:
        raise ValueError("boundary = %r: 'fixed', 'curve' or 'free'" % (boundary,))
    return n, q[0], q[1], BOUNDARIES[boundary]


def smooth_mesh(vert_lattice, faces, iterations=10, lam=0.5, mu=-0.53, boundary="curve", origin=(0.0, 0.0, 0.0), resol=1.0):
    """Taubin lambda|mu smoothing of a mesh with the uniform umbrella operator, in fixed point: vert_lattice (V,3)
    float32 or float64 in lattice cells as extract_mesh or simplify_mesh return it, faces (F,3) triangles or (F,4) quads - quads stay quads,
    their four sides are the edges; `iterations` times a pass with factor lam, then one with mu (mu = 0: plain Laplacian smoothing, which
    shrinks); boundary "fixed" (boundary vertices stay), "curve" (they smooth along the boundary curve) or "free"; origin / resol as
    lattice_origin returns them. -> dict: vertices (V,3) float32 in mm, vert_lattice (V,3) float64, vert_degree (V,) int32, vert_flags (V,)
    uint8 (1 referenced, 2 boundary vertex, 4 end of a non-manifold edge), n_edges, n_boundary_edges, n_nonmanifold_edges, n_referenced.
    Indices do not change: faces, colours, normals and vert_src carry over. iterations = 0 only reports the topology (n_boundary_edges = 0:
    the mesh is closed). ValueError on bad shapes, dtypes, settings, face indices or coordinates before the library is touched."""
    v, f = _mesh_arrays(vert_lattice, faces)
    n, lam_q16, mu_q16, code = check_smooth_args(iterations, lam, mu, boundary)
    o, r, V, F, _, _ = _mesh_args(v, f, origin, resol, None, "faces")
    if V == 0:
        m = dict(verts_mm=np.zeros((0, 3), np.float32), verts_lattice=np.zeros((0, 3), np.float64), vert_degree=np.zeros((0,), np.int32),
                 vert_flags=np.zeros((0,), np.uint8), counts=np.zeros((4,), np.int64))
    else:
        m = runtime.any_context().mesh_smooth(v.astype(np.float64), f.astype(np.int32), n, lam_q16, mu_q16, code, origin=o, resol=r)
    c = [int(x) for x in m["counts"]]
    return dict(vertices=m["verts_mm"], vert_lattice=m["verts_lattice"], vert_degree=m["vert_degree"], vert_flags=m["vert_flags"],
                n_edges=c[0], n_boundary_edges=c[1], n_nonmanifold_edges=c[2], n_referenced=c[3])


_triangles_of = triangulate                                   # (fill_holes has an argument of that name)
ORIENTATIONS = {"holes": 0, "any": 1}
FILL_COUNTS = ("n_edges", "n_boundary_edges", "n_boundary_components", "n_filled", "n_long", "n_rims", "n_complex", "n_new_faces")


def check_fill_args(max_len, orientation):
    """-> (max_len, orientation code) of fill_holes' two settings, or ValueError."""
    try:
        n = int(max_len)
    except (TypeError, ValueError):
        raise ValueError("max_len = %r must be an integer" % (max_len,))
    if isinstance(max_len, bool) or n != max_len or not 3 <= n <= 65536:
        raise ValueError("max_len = %r: an integer number of edges in 3 .. 65536" % (max_len,))
    if not isinstance(orientation, str) or orientation not in ORIENTATIONS:
        raise ValueError("orientation = %r: 'holes' or 'any'" % (orientation,))
    return n, ORIENTATIONS[orientation]


def fill_holes(vert_lattice, faces, max_len=64, orientation="holes", origin=(0.0, 0.0, 0.0), resol=1.0, vert_src=None, triangulate=True):
    """The small holes of a mesh, capped: vert_lattice (V,3) float32 or float64 in lattice cells as extract_mesh,
    smooth_mesh or simplify_mesh return it, faces (F,3) triangles or (F,4) quads, whose four sides are the edges. A closed loop of boundary
    edges whose vertices each have one boundary edge in and one out is a simple loop; one of at most max_len edges is capped by a fan of
    triangles around one new vertex at its centroid - with orientation "holes" only when the faces around it say it is a hole and not the rim
    of an open piece, with "any" always. origin / resol as lattice_origin returns them. -> dict of the concatenated mesh: vertices (V + H,3)
    float32 in mm (the old ones float32(origin + resol * vert_lattice)), vert_lattice (V + H,3) float64, faces - the old faces, triangulated
    when they are quads and triangulate is True, followed by the new triangles; with triangulate=False on quads, faces are the untouched quads
    and new_faces (T,3) stands beside them -, loop_root (H,) int32 the old vertex a new vertex takes colour and normal from, loop_len (H,)
    int32, vert_loop (V,) uint8 (0 not on a boundary edge, 1 on a filled loop, 2 on a long loop, 3 on a rim, 4 on a complex component),
    n_edges, n_boundary_edges, n_boundary_components, n_filled, n_long, n_rims, n_complex, n_new_faces; with vert_src (V,) also vert_src
    extended by vert_src[loop_root]. ValueError on bad shapes, dtypes, settings, face indices or coordinates before the library is touched."""
    v, f = _mesh_arrays(vert_lattice, faces)
    n, code = check_fill_args(max_len, orientation)
    o, r, V, F, src, _ = _mesh_args(v, f, origin, resol, vert_src, "faces")
    v64 = v.astype(np.float64)
    if F == 0:                                                  # no face: no loop, nothing for the library to do
        m = dict(new_verts_mm=np.zeros((0, 3), np.float32), new_verts_lattice=np.zeros((0, 3), np.float64), loop_root=np.zeros((0,), np.int32),
                 loop_len=np.zeros((0,), np.int32), new_faces=np.zeros((0, 3), np.int32), vert_loop=np.zeros((V,), np.uint8),
                 counts=np.zeros((8,), np.int64))
    else:
        m = runtime.any_context().mesh_fill(v64, f.astype(np.int32), n, code, origin=o, resol=r)
    with np.errstate(invalid="ignore"):
        old_mm = (o + r * v64).astype(np.float32)               # (an unreferenced vertex may be anything)
    res = dict(vertices=np.concatenate([old_mm, m["new_verts_mm"]]), vert_lattice=np.concatenate([v64, m["new_verts_lattice"]]))
    old = f.astype(np.int32)
    if f.shape[1] == 4 and not triangulate:
        res.update(faces=old, new_faces=m["new_faces"])
    else:
        res["faces"] = np.concatenate([_triangles_of(old).astype(np.int32) if f.shape[1] == 4 else old, m["new_faces"]])
    res.update(loop_root=m["loop_root"], loop_len=m["loop_len"], vert_loop=m["vert_loop"])
    if src is not None:
        res["vert_src"] = np.concatenate([src, src[m["loop_root"]]])
    res.update({k: int(c) for k, c in zip(FILL_COUNTS, m["counts"])})
    return res


NORMAL_COUNTS = ("n_zero_faces", "n_zero_vertices", "n_referenced", "n_triangles")
NORMAL_SOURCES = ("source", "mesh")


def check_normals_arg(normals, name="normals"):
    """-> normals, one of "source" (a vertex takes its source voxel's normal) or "mesh" (mesh_normals' vert_normals), or ValueError."""
    if not isinstance(normals, str) or normals not in NORMAL_SOURCES:
        raise ValueError("%s = %r: 'source' or 'mesh'" % (name, normals))
    return normals


def _limbs(words):
    """Three 64-bit limbs, least significant first, two's complement -> the Python int."""
    x = sum(int(w) << (64 * k) for k, w in enumerate(words))
    return x - (1 << 192) if x >> 191 else x


def mesh_normals(vert_lattice, faces, resol=1.0):
    """The normals of a mesh from the mesh itself, with its exact area and volume: vert_lattice (V,3) float32 or
    float64 in lattice cells as any stage returns it, faces (F,3) triangles or (F,4) quads - a quad's vector is the sum of its two
    triangles'. A vertex's normal is the unit vector of the sum of its faces' vectors, once per corner: area weights. -> dict: vert_normals
    (V,3) float32 (zero for an unreferenced vertex and where the sum is zero), face_normals (F,3) float32, n_zero_faces, n_zero_vertices,
    n_referenced, n_triangles, area2 and vol6 as Python ints (twice the area in 2^-32 cell^2, six times the signed volume in 2^-48 cell^3:
    exact, the same for any order of the faces), area = area2 / 2 / 2^32 * resol^2 and volume = vol6 / 6 / 2^48 * resol^3 as floats.
    ValueError on bad shapes, dtypes, resol, face indices or coordinates before the library is touched."""
    v, f = _mesh_arrays(vert_lattice, faces)
    _, r, V, F, _, _ = _mesh_args(v, f, (0.0, 0.0, 0.0), resol, None, "faces")
    if V == 0 or F == 0:                                        # nothing is referenced: nothing for the library to do
        m = dict(vert_normals=np.zeros((V, 3), np.float32), face_normals=np.zeros((F, 3), np.float32), counts=np.zeros((4,), np.int64),
                 sums=np.zeros((6,), np.uint64))
    else:
        m = runtime.any_context().mesh_normals(v.astype(np.float64), f.astype(np.int32))
    res = dict(vert_normals=m["vert_normals"], face_normals=m["face_normals"])
    res.update({k: int(c) for k, c in zip(NORMAL_COUNTS, m["counts"])})
    res.update(area2=_limbs(m["sums"][:3]), vol6=_limbs(m["sums"][3:]))
    res.update(area=res["area2"] / 2 / 2 ** 32 * r ** 2, volume=res["vol6"] / 6 / 2 ** 48 * r ** 3)
    return res


SIGNS = {"majority": 0, "outward": 1}
ORIENT_COUNTS = ("n_edges", "n_boundary_edges", "n_nonmanifold_edges", "n_links", "n_inconsistent", "n_components", "n_nonorientable", "n_closed",
                 "n_flipped_faces", "n_flipped_components", "n_kept_faces", "n_kept_components")


def check_orient_args(sign, min_faces, keep_largest):
    """-> (sign code, min_faces, keep_largest as 0 / 1) of orient_mesh's three settings, or ValueError."""
    if not isinstance(sign, str) or sign not in SIGNS:
        raise ValueError("sign = %r: 'majority' or 'outward'" % (sign,))
    try:
        n = int(min_faces)
    except (TypeError, ValueError):
        raise ValueError("min_faces = %r must be an integer" % (min_faces,))
    if isinstance(min_faces, bool) or n != min_faces or not 0 <= n < 1 << 31:
        raise ValueError("min_faces = %r: an integer number of faces >= 0" % (min_faces,))
    if not isinstance(keep_largest, (bool, np.bool_)):
        raise ValueError("keep_largest = %r: True or False" % (keep_largest,))
    return SIGNS[sign], n, int(keep_largest)


def orient_mesh(vert_lattice, faces, sign="majority", min_faces=0, keep_largest=False, resol=1.0):
    """The faces of a mesh made to turn one way, piece by piece, its pieces, and the mesh without its small pieces:
    vert_lattice (V,3) float32 or float64 in lattice cells as any stage returns it, faces (F,3) triangles or (F,4) quads - quads stay
    quads. Two faces across an edge that exactly the two of them share belong to one piece; within a piece every face is brought to the
    orientation of the piece's smallest face, then the piece as a whole turns by `sign`: "majority" - the fewer faces turn - or "outward" -
    a closed piece turns iff its volume is negative (an open one: the majority rule). A non-orientable piece is reported and left alone. A
    piece of fewer than min_faces faces is dropped, with keep_largest never the one with the most faces. -> dict: faces (G,nv) int32 the
    kept, oriented faces in input order, face_src (G,) int32 their input faces, and over all F input faces face_flip (F,) bool,
    face_component (F,) int32 (the smallest face of the face's piece), face_keep (F,) bool; n_edges, n_boundary_edges,
    n_nonmanifold_edges, n_links, n_inconsistent, n_components, n_nonorientable, n_closed, n_flipped_faces, n_flipped_components,
    n_kept_faces, n_kept_components; components, a dict of arrays over the pieces in ascending id: id, n_faces, orientable, closed,
    flipped, kept, and vol6 a list of Python ints (six times the signed volume in 2^-48 cell^3 after the turn, exact), volume = vol6 / 6 /
    2^48 * resol^3 as floats. Vertices are untouched: positions, vert_src, colours carry over. ValueError on bad shapes, dtypes, settings,
    face indices or coordinates before the library is touched."""
    v, f = _mesh_arrays(vert_lattice, faces)
    code, n, largest = check_orient_args(sign, min_faces, keep_largest)
    _, r, V, F, _, _ = _mesh_args(v, f, (0.0, 0.0, 0.0), resol, None, "faces")
    nv = f.shape[1]
    if V == 0 or F == 0:                                        # no face (V = 0 with faces was refused): nothing for the library to do
        m = dict(faces_out=np.zeros((F, nv), np.int32), face_flip=np.zeros((F,), np.uint8), face_component=np.zeros((F,), np.int32),
                 face_keep=np.zeros((F,), np.uint8), comp_faces=np.zeros((F,), np.int32), comp_flags=np.zeros((F,), np.uint8),
                 comp_vol6=np.zeros((F, 3), np.uint64), counts=np.zeros((12,), np.int64))
    else:
        m = runtime.any_context().mesh_orient(v.astype(np.float64), f.astype(np.int32), code, n, largest)
    keep = m["face_keep"].astype(bool)
    res = dict(faces=m["faces_out"][keep], face_src=np.flatnonzero(keep).astype(np.int32), face_flip=m["face_flip"].astype(bool),
               face_component=m["face_component"], face_keep=keep)
    res.update({k: int(c) for k, c in zip(ORIENT_COUNTS, m["counts"])})
    ids = np.flatnonzero(m["comp_faces"] > 0)
    fl = m["comp_flags"][ids]
    vol6 = [_limbs(row) for row in m["comp_vol6"][ids]]
    res["components"] = dict(id=ids.astype(np.int32), n_faces=m["comp_faces"][ids], orientable=(fl & 1) != 0, closed=(fl & 2) != 0,
                             flipped=(fl & 4) != 0, kept=(fl & 8) != 0, vol6=vol6,
                             volume=np.asarray([x / 6 / 2 ** 48 * r ** 3 for x in vol6], np.float64))
    return res


INTERSECT_COUNTS = ("n_triangles", "n_degenerate_faces", "n_pairs", "n_faces_hit", "n_disjoint_pairs", "n_adjacent_pairs")
_INTERSECT_WORDS = (0, 1, 3, 4, 5, 6)                         # their places in the library's counts (2: the broad phase's candidates, 7: written)


def check_intersect_args(max_pairs=None):
    """-> max_pairs of self_intersections (None: every pair), or ValueError."""
    if max_pairs is None:
        return None
    try:
        n = int(max_pairs)
    except (TypeError, ValueError):
        raise ValueError("max_pairs = %r must be an integer or None" % (max_pairs,))
    if isinstance(max_pairs, (bool, np.bool_)) or n != max_pairs or not 0 <= n < 1 << 62:
        raise ValueError("max_pairs = %r: an integer number of pairs >= 0, or None for all of them" % (max_pairs,))
    return n


def self_intersections(vert_lattice, faces, max_pairs=None):
    """The pairs of faces of a mesh that have a point in common beyond what their shared vertices explain, exactly:
    vert_lattice (V,3) float32 or float64 in lattice cells as any stage returns it, faces (F,3) triangles or (F,4) quads - a quad is its
    triangles (a,b,c), (a,c,d), pairs name the quads. Positions are the stages' fixed point, q = rint(v * 65536), and every test is a sign
    of an exact integer. Closed sets: two faces that only touch - a T-junction, a seam of coincident but distinct vertices, a duplicate -
    intersect; two faces that share one or two vertex indices intersect only where they have more than those in common (a fold). A
    degenerate triangle is skipped. -> dict: pairs (P',2) int32 the first max_pairs (None: all) pairs f < g in ascending order, face_hit (F,)
    bool, face_pairs (F,) int32 the pairs a face is in, n_triangles, n_degenerate_faces, n_pairs, n_faces_hit, n_disjoint_pairs (a hit of
    two triangles without a common index), n_adjacent_pairs (the others), truncated = n_pairs > len(pairs). There is no repair. ValueError
    on bad shapes, dtypes, max_pairs, face indices or coordinates before the library is touched."""
    v, f = _mesh_arrays(vert_lattice, faces)
    cap = check_intersect_args(max_pairs)
    _, _, V, F, _, _ = _mesh_args(v, f, (0.0, 0.0, 0.0), 1.0, None, "faces")
    if V == 0 or F == 0:                                        # no face (V = 0 with faces was refused): nothing for the library to do
        m = dict(pairs=np.zeros((0, 2), np.int32), face_hit=np.zeros((F,), np.uint8), face_pairs=np.zeros((F,), np.int32),
                 counts=np.zeros((8,), np.int64))
    else:
        m = runtime.any_context().mesh_intersect(v.astype(np.float64), f.astype(np.int32), cap_pairs=cap)
    res = dict(pairs=m["pairs"], face_hit=m["face_hit"].astype(bool), face_pairs=m["face_pairs"])
    res.update({k: int(m["counts"][i]) for k, i in zip(INTERSECT_COUNTS, _INTERSECT_WORDS)})
    res["truncated"] = res["n_pairs"] > res["pairs"].shape[0]
    return res


DISTANCE_COUNTS = ("n_triangles", "n_degenerate", "n_answered", "n_beyond")
MAX_QUERY_POINTS = 1 << 29
MAX_DISTANCE_TRIANGLES = 1 << 26


def check_distance_args(points, max_dist=60.0):
    """-> (points (n,3) float64, max_dist) of point_to_mesh, or ValueError: points float32 or float64 (n,3), at most 2^29 of them, finite - the
    first that is not is named, as the library names it -, max_dist finite and > 0."""
    p = np.asarray(points)
    if p.dtype not in (np.float32, np.float64):
        raise ValueError("points must be float32 or float64, not %s" % p.dtype)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("points must be (n,3), not %r" % (p.shape,))
    if p.shape[0] > MAX_QUERY_POINTS:
        raise ValueError("%d points: at most 2^29" % p.shape[0])
    try:
        d = float(max_dist)
    except (TypeError, ValueError):
        raise ValueError("max_dist = %r must be a number" % (max_dist,))
    if isinstance(max_dist, (bool, np.bool_)) or not (np.isfinite(d) and d > 0):
        raise ValueError("max_dist = %r must be finite and > 0" % (max_dist,))
    bad = ~np.isfinite(p).all(axis=1)
    if bad.any():
        raise ValueError("point %d: a coordinate is not finite" % int(np.argmax(bad)))
    return p.astype(np.float64), d


def point_to_mesh(points, vertices, faces, max_dist=60.0):
    """For every point the nearest point of a mesh, exactly over all its triangles: points (n,3) float32 or float64,
    vertices (V,3) in the same WORLD coordinates, faces (F,3) triangles or (F,4) quads - a quad is its triangles (a,b,c), (a,c,d), `face`
    names the quad. A degenerate triangle is its three segments. -> dict: dist2 (n,) float64 the squared distance (+inf where it is not
    below max_dist^2 (1 + 2^-40)), dist (n,) float64 = min(sqrt(dist2), max_dist) as the DTU protocol caps it, face (n,) int32 (-1 beyond
    the cap), closest (n,3) float64 (NaN there), n_triangles, n_degenerate, n_answered, n_beyond. The distance is unsigned. ValueError on
    bad shapes, dtypes, max_dist, face indices or coordinates before the library is touched."""
    v, f = _world_mesh(vertices, faces)
    p, d = check_distance_args(points, max_dist)
    n, T = p.shape[0], f.shape[0] * (f.shape[1] - 2)
    if T > MAX_DISTANCE_TRIANGLES:
        raise ValueError("%d triangles: at most 2^26" % T)
    if n == 0 or v.shape[0] == 0:                               # no point, or no vertex and so no face: nothing for the library to do
        m = dict(d2=np.full((n,), np.inf), face=np.full((n,), -1, np.int32), closest=np.full((n, 3), np.nan), counts=np.array([0, 0, 0, n, 0, 0, 0, 0], np.int64))
    else:
        m = runtime.any_context().mesh_distance(v, f, p, d)
    res = dict(dist2=m["d2"], dist=np.minimum(np.sqrt(m["d2"]), d), face=m["face"], closest=m["closest"])
    res.update({k: int(c) for k, c in zip(DISTANCE_COUNTS, m["counts"])})
    return res


def _deviation(dist, n_beyond):
    """The statistics of one direction of mesh_deviation: host numpy on the capped distances, float64."""
    d = np.asarray(dist, np.float64)
    if d.size == 0:
        return dict(n=0, n_beyond=0, max=0.0, mean=0.0, rms=0.0)
    return dict(n=int(d.size), n_beyond=int(n_beyond), max=float(d.max()), mean=float(d.mean()), rms=float(np.sqrt((d * d).mean())))


def check_deviation_setting(value):
    """reconstruct.scene_postpass's mesh_deviation -> None (None or False: not asked for) or dict(dst=, max_dist=) with both checked - dst
    None stays None: the lattice's resol -, or ValueError. The library is not touched."""
    if value is None or value is False:
        return None
    if value is not True and (not isinstance(value, dict) or set(value) - {"dst", "max_dist"}):
        raise ValueError("mesh_deviation = %r: True or a dict of dst, max_dist" % (value,))
    kw = dict(dict(dst=None, max_dist=60.0), **({} if value is True else value))
    _, kw["max_dist"] = check_distance_args(np.zeros((0, 3)), kw["max_dist"])
    if kw["dst"] is not None:
        try:
            d = float(kw["dst"])
        except (TypeError, ValueError):
            raise ValueError("dst = %r must be a number" % (kw["dst"],))
        if isinstance(kw["dst"], (bool, np.bool_)) or not (np.isfinite(d) and d > 0):
            raise ValueError("dst = %r must be finite and > 0" % (kw["dst"],))
        kw["dst"] = d
    return kw


def mesh_deviation(vertices_a, faces_a, vertices_b, faces_b, dst, max_dist=60.0):
    """How far two meshes in the same world coordinates are from each other: the surface samples of a at density dst
    (sample_surface) against the surface of b (point_to_mesh), and the reverse. -> dict: a_to_b and b_to_a, each a dict of n the samples,
    n_beyond those farther than max_dist, and max, mean, rms of their distances capped at max_dist; hausdorff, the larger max. It is a
    SAMPLED Hausdorff distance: a lower bound of the true one and, every point of a triangle lying within 2/3 dst of a sample, within
    2/3 dst of it (below the cap). ValueError before the library is touched."""
    va, fa = _world_mesh(vertices_a, faces_a)
    vb, fb = _world_mesh(vertices_b, faces_b)
    check_distance_args(np.zeros((0, 3)), max_dist)
    res = {}
    for key, (v0, f0), (v1, f1) in (("a_to_b", (va, fa), (vb, fb)), ("b_to_a", (vb, fb), (va, fa))):
        pts = sample_surface(v0, f0, dst)[0] if f0.shape[0] else np.zeros((0, 3))
        r = point_to_mesh(pts, v1, f1, max_dist)
        res[key] = _deviation(r["dist"], r["n_beyond"])
    res["hausdorff"] = max(res["a_to_b"]["max"], res["b_to_a"]["max"])
    return res


WINDING_COUNTS = ("n_triangles", "n_parallel", "n_degenerate", "n_inside", "n_on_surface")
_WINDING_WORDS = (0, 1, 2, 3, 5)                                # their places in the library's counts (4: the broad phase's tests)
AXES = {"x": 0, "y": 1, "z": 2}


def check_winding_args(points, axis=2):
    """-> (points (n,3) float64, axis 0..2) of winding_number, or ValueError: points float32 or float64 (n,3) in lattice cells, at most 2^29
    of them, every coordinate in [-4, 2^21 - 8) - the first that is not is named, as the library names it -, axis 0, 1, 2 or "x", "y", "z"."""
    p = np.asarray(points)
    if p.dtype not in (np.float32, np.float64):
        raise ValueError("points_lattice must be float32 or float64, not %s" % p.dtype)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("points_lattice must be (n,3), not %r" % (p.shape,))
    if p.shape[0] > MAX_QUERY_POINTS:
        raise ValueError("%d points: at most 2^29" % p.shape[0])
    if isinstance(axis, str):
        if axis not in AXES:
            raise ValueError("axis = %r: 0, 1, 2 or one of %s" % (axis, sorted(AXES)))
        a = AXES[axis]
    else:
        try:
            a = int(axis)
        except (TypeError, ValueError):
            raise ValueError("axis = %r: 0, 1, 2 or one of %s" % (axis, sorted(AXES)))
        if isinstance(axis, (bool, np.bool_)) or a != axis or not 0 <= a <= 2:
            raise ValueError("axis = %r: 0, 1, 2 or one of %s" % (axis, sorted(AXES)))
    with np.errstate(invalid="ignore"):
        bad = ~((p >= -4.0) & (p < 2097144.0)).all(axis=1)      # (NaN fails)
    if bad.any():
        raise ValueError("point %d: a coordinate is outside [-4, 2^21 - 8) lattice cells" % int(np.argmax(bad)))
    return p.astype(np.float64), a


def winding_number(points_lattice, vert_lattice, faces, axis=2):
    """For every point how many times a mesh winds around it, exactly: points_lattice (n,3) float32 or float64 and
    vert_lattice (V,3) in lattice cells as any stage returns them, faces (F,3) triangles or (F,4) quads - a quad is its triangles (a,b,c),
    (a,c,d) -, axis the axis the rays run along. Positions are the stages' fixed point, q = rint(v * 65536), and every test is a sign of an
    exact integer; a ray through a vertex or along an edge counts each crossing once (the renderer's fill rule). -> dict: winding (n,) int32
    the signed crossings - a closed mesh turned outward (orient_mesh(sign="outward")) gives +1 inside and 0 outside -, crossings (n,) int32
    their number, on_surface (n,) bool the point lies on a triangle (closed, the same for every axis), inside (n,) bool = winding != 0,
    n_triangles (those a ray can cross), n_parallel (parallel to the rays), n_degenerate, n_inside, n_on_surface. On an open or
    inconsistently turned mesh the winding number depends on the axis. ValueError on bad shapes, dtypes, axis, face indices or coordinates
    before the library is touched."""
    v, f = _mesh_arrays(vert_lattice, faces)
    p, a = check_winding_args(points_lattice, axis)
    _, _, V, F, _, _ = _mesh_args(v, f, (0.0, 0.0, 0.0), 1.0, None, "faces")
    n, T = p.shape[0], F * (f.shape[1] - 2)
    if T > MAX_DISTANCE_TRIANGLES:
        raise ValueError("%d triangles: at most 2^26" % T)
    if n == 0 or F == 0:                                        # no point, or no face: nothing for the library to do
        m = dict(winding=np.zeros((n,), np.int32), crossings=np.zeros((n,), np.int32), on_surface=np.zeros((n,), np.uint8),
                 counts=np.zeros((8,), np.int64))
    else:
        m = runtime.any_context().mesh_winding(v.astype(np.float64), f.astype(np.int32), p, axis=a)
    res = dict(winding=m["winding"], crossings=m["crossings"], on_surface=m["on_surface"].astype(bool), inside=m["winding"] != 0)
    res.update({k: int(m["counts"][i]) for k, i in zip(WINDING_COUNTS, _WINDING_WORDS)})
    return res


def signed_distance(points_lattice, vert_lattice, faces, max_dist=60.0, axis=2, resol=1.0):
    """The signed distance of points to a closed mesh, host code over point_to_mesh - with the lattice positions
    as its world - and winding_number: points_lattice (n,3) and vert_lattice (V,3) in lattice cells, max_dist in lattice cells, resol the
    cell size the distances are scaled by. -> dict: dist (n,) float64 = point_to_mesh's capped distance * resol, negative where the point
    is inside (winding != 0) and exactly 0.0 where it lies on the surface or its squared distance is 0; face (n,) int32, closest (n,3)
    float64 (scaled by resol), winding (n,) int32, on_surface (n,) bool. The distance uses the float64 positions as given and the sign the
    quantised ones: they can disagree only within 2^-17 cell of the surface. ValueError before the library is touched."""
    try:
        r = float(resol)
    except (TypeError, ValueError):
        raise ValueError("resol = %r must be a number" % (resol,))
    if isinstance(resol, (bool, np.bool_)) or not (np.isfinite(r) and r > 0):
        raise ValueError("resol = %r must be finite and > 0" % (resol,))
    v, f = _mesh_arrays(vert_lattice, faces)
    p, a = check_winding_args(points_lattice, axis)
    check_distance_args(p, max_dist)
    _mesh_args(v, f, (0.0, 0.0, 0.0), 1.0, None, "faces")
    w = winding_number(p, v, f, axis=a)
    d = point_to_mesh(p, v, f, max_dist=max_dist)
    dist = d["dist"] * r
    dist = np.where(w["inside"], -dist, dist)
    dist[w["on_surface"] | (d["dist2"] == 0.0)] = 0.0
    return dict(dist=dist, face=d["face"], closest=d["closest"] * r, winding=w["winding"], on_surface=w["on_surface"])


VOXEL_MODES = {"solid": 1, "surface": 2}
VOXEL_SELECTS = {"solid": 1, "surface": 2, "either": 3}
VOXEL_COUNTS = ("n_triangles", "n_parallel", "n_degenerate", "n_solid_voxels", "n_surface_voxels", "n_both_voxels", "n_pairs", "n_tests")
MAX_CUBE_D = 64
MAX_VOXELS = 1 << 33


def _voxel_bits(value, table, name):
    """A name of `table`, or a sequence of them, as its bits."""
    names = (value,) if isinstance(value, str) else value
    try:
        names = tuple(names)
        if not names or not all(isinstance(n, str) and n in table for n in names):
            raise TypeError
    except TypeError:
        raise ValueError("%s = %r: of %s" % (name, value, sorted(table)))
    bits = 0
    for n in names:
        bits |= table[n]
    return bits


def check_voxelize_args(cube_ijk, cube_D, stride_vox, mode=("solid", "surface"), axis=2, select=None):
    """-> (cube_ijk (N,3) int32, D, stride, modes bits, axis 0..2, select bits or None) of voxelize, or ValueError in the library's words:
    cube_ijk integers (N,3), cube_D an integer in 1..64, stride_vox an integer >= 1, mode "solid", "surface" or both, axis as winding_number
    takes it, select "solid", "surface" or "either"; at most 2^33 voxels; the first cube with a negative ijk, then the first whose last cell
    cube_ijk * stride_vox + cube_D - 1 reaches 2^21 - 8."""
    c = np.asarray(cube_ijk)
    if c.dtype.kind not in "iu":
        raise ValueError("cube_ijk must hold integers, not %s" % c.dtype)
    if c.ndim != 2 or c.shape[1] != 3:
        raise ValueError("cube_ijk must be (N,3), not %r" % (c.shape,))
    for name, value in (("cube_D", cube_D), ("stride_vox", stride_vox)):
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
            raise ValueError("%s = %r must be an integer" % (name, value))
    D, stride = int(cube_D), int(stride_vox)
    if not 1 <= D <= MAX_CUBE_D:
        raise ValueError("D = %d: 1 .. 64" % D)
    if stride < 1 or stride >= 1 << 31:
        raise ValueError("stride_vox = %d must be >= 1" % stride)
    modes = _voxel_bits(mode, VOXEL_MODES, "mode")
    sel = None if select is None else _voxel_bits(select, VOXEL_SELECTS, "select")
    _, a = check_winding_args(np.zeros((0, 3)), axis)
    if c.shape[0] * D ** 3 > MAX_VOXELS:
        raise ValueError("%d voxels: at most 2^33" % (c.shape[0] * D ** 3))
    c64 = c.astype(np.int64)
    if c.shape[0] and (np.abs(c64) >= 1 << 31).any():
        raise ValueError("cube_ijk must fit int32")
    negative, reach = (c64 < 0).any(axis=1), (c64 * stride + D - 1 >= 2097144).any(axis=1)
    bad = negative | reach
    if bad.any():
        n = int(np.argmax(bad))
        raise ValueError("cube %d: a negative ijk" % n if negative[n] else "cube %d: its last cell reaches 2^21 - 8 lattice cells" % n)
    return np.ascontiguousarray(c64.astype(np.int32)), D, stride, modes, a, sel


def voxelize(vert_lattice, faces, cube_ijk, cube_D, stride_vox, mode=("solid", "surface"), axis=2):
    """A mesh back into cubes of voxels, exactly: vert_lattice (V,3) in lattice cells as any stage returns them,
    faces (F,3) triangles or (F,4) quads, cube_ijk (N,3), cube_D and stride_vox as extract_mesh takes them - voxel (n; i,j,k) is the world
    cell cube_ijk[n] * stride_vox + (i,j,k) and its centre that lattice point -, mode "solid", "surface" or both, axis the axis the solid
    bit's rays run along. solid: the winding number of the voxel's centre is not zero (winding_number's `inside`, byte for byte); surface:
    the voxel's closed box meets a triangle (touching counts; the same for every axis). -> dict: occ (N,D,D,D) uint8 the bits (1 solid, 2
    surface), solid and surface (N,D,D,D) bool, n_solid and n_surface (N,) int64 per cube, and the counts n_triangles, n_parallel,
    n_degenerate, n_solid_voxels, n_surface_voxels, n_both_voxels, n_pairs, n_tests (the last two: the broad phase's cost). Cubes may
    overlap; a shared cell has the same bits in each. ValueError on bad arguments before the library is touched."""
    v, f = _mesh_arrays(vert_lattice, faces)
    cube, D, stride, modes, a, _ = check_voxelize_args(cube_ijk, cube_D, stride_vox, mode, axis)
    _, _, V, F, _, _ = _mesh_args(v, f, (0.0, 0.0, 0.0), 1.0, None, "faces")
    if F * (f.shape[1] - 2) > MAX_DISTANCE_TRIANGLES:
        raise ValueError("%d triangles: at most 2^26" % (F * (f.shape[1] - 2)))
    N = cube.shape[0]
    if N == 0 or F == 0:                                        # no cube, or no face: nothing for the library to do
        m = dict(occ=np.zeros((N, D, D, D), np.uint8), per_cube=np.zeros((N, 2), np.int64), counts=np.zeros((8,), np.int64))
    else:
        m = runtime.any_context().mesh_voxelize(v.astype(np.float64), f.astype(np.int32), cube, D, stride, axis=a, modes=modes, select=modes,
                                                outputs=("occ", "per_cube"))
    res = dict(occ=m["occ"], solid=(m["occ"] & 1).view(bool), surface=((m["occ"] >> 1) & 1).view(bool), n_solid=m["per_cube"][:, 0].copy(),
               n_surface=m["per_cube"][:, 1].copy())
    res.update({k: int(x) for k, x in zip(VOXEL_COUNTS, m["counts"])})
    return res


def occupancy_lists(occ, select="surface"):
    """voxelize's occ (N,D,D,D) uint8 as sparse cubes: (vxl_ijk_list, vxl_mask_list) - per cube the (n,3) uint8 ijk of its voxels with one
    of the selected bits ("surface", "solid" or "either"), in [i,j,k] order, and an all-True mask -, the form extract_mesh,
    normals.estimate_normals, the components pass, sparseCubes.unique_voxels and the PLY writers take."""
    o = np.asarray(occ)
    if o.dtype != np.uint8 or o.ndim != 4 or not o.shape[1] == o.shape[2] == o.shape[3]:
        raise ValueError("occ must be uint8 (N,D,D,D), not %s %r" % (o.dtype, o.shape))
    bits = _voxel_bits(select, VOXEL_SELECTS, "select")
    ijk_list = [np.argwhere(cube & bits).astype(np.uint8).reshape(-1, 3) for cube in o]
    return ijk_list, [np.ones((len(a),), bool) for a in ijk_list]


RENDER_COUNTS = ("n_triangles", "n_clipped", "n_degenerate", "n_rasterised", "n_pairs", "n_pixels", "n_visible")
MAX_IMAGE_DIM = 16384


def check_render_args(cameraPOs, shape, near=0.0, tol=0.0, views=None):
    """-> (P (V',3,4) float64 - the cameras of `views`, all of them for None -, (H, W), near, tol, the views as a list) of render_mesh's
    settings, or ValueError: cameraPOs (V,3,4) finite numbers, shape two integers in 1 .. 16384, near and tol finite and >= 0, views
    distinct or not, each in [0, V), at least one."""
    try:
        P = np.asarray(cameraPOs, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("cameraPOs must be numbers of shape (V, 3, 4)")
    if P.ndim != 3 or P.shape[1:] != (3, 4) or P.shape[0] < 1:
        raise ValueError("cameraPOs must have shape (V, 3, 4) with V >= 1, got %r" % (P.shape,))
    try:
        H, W = shape
        hw = (int(H), int(W))
    except (TypeError, ValueError):
        raise ValueError("shape = %r must be two integers (H, W)" % (shape,))
    if isinstance(H, bool) or isinstance(W, bool) or hw != (H, W) or not (1 <= hw[0] <= MAX_IMAGE_DIM and 1 <= hw[1] <= MAX_IMAGE_DIM):
        raise ValueError("shape = %r: (H, W), integers in 1 .. %d" % (shape, MAX_IMAGE_DIM))
    out = []
    for name, x in (("near", near), ("tol", tol)):
        try:
            val = float(x)
        except (TypeError, ValueError):
            raise ValueError("%s = %r must be a number" % (name, x))
        if isinstance(x, bool) or not np.isfinite(val) or val < 0:
            raise ValueError("%s = %r must be finite and >= 0" % (name, x))
        out.append(val)
    if views is None:
        sel = list(range(P.shape[0]))
    else:
        try:
            sel = [int(v) for v in views]
        except (TypeError, ValueError):
            raise ValueError("views = %r must be a sequence of view indices" % (views,))
        if not sel or any(int(v) != v or isinstance(v, bool) or not 0 <= int(v) < P.shape[0] for v in views):
            raise ValueError("views = %r: at least one index, each in [0, %d)" % (views, P.shape[0]))
    P = np.ascontiguousarray(P[sel])
    if not np.isfinite(P).all():
        raise ValueError("cameraPOs of view %d is not finite" % sel[int(np.argmax(~np.isfinite(P).all(axis=(1, 2))))])
    return P, hw, out[0], out[1], sel


_RENDER_SETTING = dict(cameraPOs=None, shape=None, views=None, near=0.0, tol=None, images=None)


def check_render_setting(value):
    """reconstruct.scene_postpass's mesh_render -> all of its keywords, checked (check_render_args; tol None stays None: half the lattice's
    resol; images: one (H,W,3) uint8 array of `shape` per camera), or ValueError. The library is not touched."""
    words = "mesh_render = %r: a dict of cameraPOs, shape and optionally views, near, tol, images"
    if not isinstance(value, dict) or set(value) - set(_RENDER_SETTING) or "cameraPOs" not in value or "shape" not in value:
        raise ValueError(words % (value if not isinstance(value, dict) else sorted(value),))
    kw = dict(_RENDER_SETTING, **value)
    _, hw, _, _, _ = check_render_args(kw["cameraPOs"], kw["shape"], kw["near"], 0.0 if kw["tol"] is None else kw["tol"], kw["views"])
    if kw["images"] is not None:
        imgs = [np.asarray(im) for im in kw["images"]]
        if len(imgs) != np.asarray(kw["cameraPOs"]).shape[0] or any(im.shape != hw + (3,) or im.dtype != np.uint8 for im in imgs):
            raise ValueError("mesh_render: images must be one (%d, %d, 3) uint8 array per camera" % hw)
    return kw


def _world_mesh(vertices, faces):
    """What render_mesh and colour_vertices ask of a mesh in world coordinates: _mesh_arrays, at most 2^28 of either, every face index in
    [0, V), every coordinate of a referenced vertex finite - the first offending face is named, as the library names it."""
    v, f = _mesh_arrays(vertices, faces, "vertices")
    V, F = v.shape[0], f.shape[0]
    if V > 1 << 28 or F > 1 << 28:
        raise ValueError("%d vertices, %d faces: at most 2^28 of either" % (V, F))
    if F:
        bad = ((f < 0) | (f >= V)).any(axis=1)
        if bad.any():
            raise ValueError("face %d names a vertex outside [0, %d)" % (int(np.argmax(bad)), V))
        bad = ~np.isfinite(v).all(axis=1)[f].all(axis=1)
        if bad.any():
            raise ValueError("face %d: a coordinate of one of its vertices is not finite" % int(np.argmax(bad)))
    return v.astype(np.float64), f.astype(np.int32)


def render_mesh(vertices, faces, cameraPOs, shape, near=0.0, tol=0.0, views=None):
    """A mesh rendered back into the views it came from: vertices (n,3) float32 or float64 in WORLD coordinates (a
    stage's "vertices", in mm), faces (F,3) triangles or (F,4) quads - a quad is its two triangles, face ids stay the quads' -, cameraPOs
    (V,3,4), shape = (H, W) the one size of all views, near >= 0 (a triangle with a corner at z <= near vanishes whole), tol >= 0 the depth
    tolerance of the vertex test (about half a voxel for concave detail), views the indices of the cameras to render (None: all). An
    integer rasteriser with a watertight fill rule, perspective-correct depth in fp64: the result is the same on every run. -> dict: depth
    (V',H,W) float64 (0.0 where no face is), face (V',H,W) int32 (-1 there), face_pixels (V',F) int32 the pixels a face wins, vert_visible
    (V',n) bool, views the list of rendered views, and n_triangles, n_clipped, n_degenerate, n_rasterised, n_pairs, n_pixels, n_visible
    summed over them. Limits: no clipping at the camera plane, one image size, vertices next to the silhouette count as visible, no
    anti-aliasing. ValueError on bad shapes, dtypes, settings, face indices or coordinates before the library is touched."""
    v, f = _world_mesh(vertices, faces)
    P, (H, W), near, tol, sel = check_render_args(cameraPOs, shape, near, tol, views)
    V = P.shape[0]
    if v.shape[0] == 0:                                         # no vertex, so no face: nothing for the library to do
        m = dict(depth=np.zeros((V, H, W), np.float64), face=np.full((V, H, W), -1, np.int32), face_pixels=np.zeros((V, f.shape[0]), np.int32),
                 vert_visible=np.zeros((V, 0), np.uint8), counts=np.zeros((8,), np.int64))
    else:
        m = runtime.any_context().mesh_render(v, f, P, (H, W), near, tol)
    res = dict(depth=m["depth"], face=m["face"], face_pixels=m["face_pixels"], vert_visible=m["vert_visible"].astype(bool), views=sel)
    res.update({k: int(c) for k, c in zip(RENDER_COUNTS, m["counts"])})
    return res


def colour_vertices(vertices, faces, cameraPOs, images, vert_visible=None, near=0.0, tol=0.0, views=None):
    """The colour of every vertex from the views that see it: the mesh and cameras of render_mesh, images a
    sequence of V (H,W,3) uint8 RGB images of one size, one per camera, vert_visible (V',n) - render_mesh's for the same views, or any other
    array; None renders first with near and tol. A view contributes the pixel nearest the vertex's projection when the vertex is visible in
    it: equal weights, rounded mean. -> dict: vert_rgb (n,3) uint8 ((0,0,0) without a view), vert_views (n,) int32, n_coloured. The images
    of `views` become the shared context's (Context.set_images). ValueError before the library is touched."""
    v, f = _world_mesh(vertices, faces)
    imgs = [np.asarray(im) for im in images]
    if not imgs or any(im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8 or im.shape != imgs[0].shape for im in imgs):
        raise ValueError("images must be (H, W, 3) uint8 RGB arrays of one size")
    P, (H, W), near, tol, sel = check_render_args(cameraPOs, imgs[0].shape[:2], near, tol, views)
    if len(imgs) != np.asarray(cameraPOs).shape[0]:
        raise ValueError("%d images for %d cameras" % (len(imgs), np.asarray(cameraPOs).shape[0]))
    n = v.shape[0]
    if vert_visible is not None:
        vis = np.asarray(vert_visible)
        if vis.shape != (len(sel), n):
            raise ValueError("vert_visible must have shape (%d, %d), not %r" % (len(sel), n, vis.shape))
    if n == 0:
        return dict(vert_rgb=np.zeros((0, 3), np.uint8), vert_views=np.zeros((0,), np.int32), n_coloured=0)
    ctx = runtime.any_context()
    if vert_visible is None:
        vis = ctx.mesh_render(v, f, P, (H, W), near, tol, outputs=("vert_visible",))["vert_visible"]
    ctx.set_images([imgs[k] for k in sel])
    m = ctx.mesh_vertex_colors(v, f, P, (H, W), vis != 0, near, tol)
    return dict(vert_rgb=m["vert_rgb"], vert_views=m["vert_views"], n_coloured=int(m["counts"][0]))


# The chain that follows extract_mesh, in its order. A row: the key of the stage's result, reconstruct.scene_postpass's
# argument, the keyword a bare value stands for (a number, or orient's sign word), the defaults (their keys are the allowed ones), what a
# refusal says the argument is, the check of the keywords, the stage, the letter of its PLY file's tag, and what the stage keeps of the mesh
# that goes in: None - nothing, its result is a new mesh with its own vert_src -, "faces" - it moves the vertices -, "vertices" - it
# replaces the faces under the key they came in -, "mesh" - all of it: the stage reports on the mesh and the next one reads the same mesh; it
# has no letter, so no file. mesh_cell is a number only: its second keyword is mesh_placement; mesh_check's bare value is True: the defaults.
_Stage = collections.namedtuple("_Stage", "key arg first defaults words check run letter keeps")
_CHAIN = (
    _Stage("filled", "mesh_fill", "max_len", dict(max_len=64, orientation="holes"), "a largest loop length or a dict of max_len, orientation",
           check_fill_args, fill_holes, "f", None),
    _Stage("smoothed", "mesh_smooth", "iterations", dict(iterations=10, lam=0.5, mu=-0.53, boundary="curve"),
           "a number of iterations or a dict of iterations, lam, mu, boundary", check_smooth_args, smooth_mesh, "s", "faces"),
    _Stage("simplified", "mesh_cell", "cell", None, None, check_simplify_args, simplify_mesh, "c", None),
    _Stage("oriented", "mesh_orient", "sign", dict(sign="majority", min_faces=0, keep_largest=False),
           "a sign word or a dict of sign, min_faces, keep_largest", check_orient_args, orient_mesh, "o", "vertices"),
    _Stage("checked", "mesh_check", "max_pairs", dict(max_pairs=None), "True or a dict of max_pairs", check_intersect_args, self_intersections,
           None, "mesh"),
)
_STAGES = {row.key: row for row in _CHAIN}


def _stage_keywords(row, value):
    """A stage's argument - a number (the row's first keyword) or a dict of keywords - as all of its keywords, or ValueError."""
    kw = dict(value) if isinstance(value, dict) else ({} if row.keeps == "mesh" and value is True else {row.first: value})
    if set(kw) - set(row.defaults) or (row.keeps == "mesh" and not isinstance(value, dict) and value is not True):
        raise ValueError("%s = %r: %s" % (row.arg, value, row.words))
    return dict(row.defaults, **kw)


def chain_settings(mesh_fill=None, mesh_smooth=None, mesh_cell=None, mesh_placement="mean", mesh_orient=None, mesh_check=None):
    """scene_postpass's mesh_fill, mesh_smooth, mesh_cell / mesh_placement, mesh_orient and mesh_check -> [(key, keywords), ...]: the stages
    asked for (not None; mesh_check=False asks for nothing either) in the chain's order - "filled", "smoothed", "simplified", "oriented",
    "checked" - each with the checked keywords of fill_holes, smooth_mesh, simplify_mesh, orient_mesh, self_intersections. ValueError for
    the first bad argument in the order mesh_check, mesh_orient, mesh_cell, mesh_smooth, mesh_fill; the library is not touched."""
    given = dict(mesh_fill=mesh_fill, mesh_smooth=mesh_smooth, mesh_cell=mesh_cell, mesh_orient=mesh_orient,
                 mesh_check=None if mesh_check is False else mesh_check)
    stages = []
    for row in reversed(_CHAIN):
        value = given[row.arg]
        if value is not None:
            kw = dict(cell=value, placement=mesh_placement) if row.defaults is None else _stage_keywords(row, value)
            row.check(**kw)
            stages.insert(0, (row.key, kw))
    return stages


def stage_tag(key, kw):
    """The tag of a chain stage's PLY file, <prefix><name>_mesh<tag>.ply: "_f<max_len>", "_s<iterations>", "_c<cell>", and "_o" - the letter
    alone where the stage's first keyword is a word; None for a stage that writes no file (the check)."""
    if _STAGES[key].letter is None:
        return None
    first = kw[_STAGES[key].first]
    return "_" + _STAGES[key].letter + ("" if isinstance(first, str) else "%d" % int(first))


def _faces(m):
    """A stage's faces: triangles under "faces", or extract_mesh's "quads"."""
    return m["faces"] if "faces" in m else m["quads"]


def run_chain(m, stages, origin, resol):
    """extract_mesh's dict m (empty_mesh() too) through chain_settings' stages, each on the result of the one before it: fill, smooth,
    decimate, orient; origin / resol as lattice_origin returns them. -> {key: the stage's result}: fill_holes' and simplify_mesh's dicts as
    they are, both with vert_src; "smoothed" the mesh that went in - m, or vertices, vert_lattice, faces, vert_src of the filled one - with
    smooth_mesh's positions and statistics, so it holds quads without a fill and faces after one; "oriented" the mesh that went in with
    orient_mesh's kept, oriented faces under the key its faces came in (quads or faces) and the rest of orient_mesh's dict beside them;
    "checked" self_intersections' report on the mesh that went in, which goes on as it is."""
    res = {}
    for key, kw in stages:
        run, keeps = _STAGES[key].run, _STAGES[key].keeps
        if keeps == "mesh":                                     # a report: the mesh goes on as it is
            res[key] = run(m["vert_lattice"], _faces(m), **kw)
        elif keeps == "faces":                                    # indices stay: the mesh's other keys carry over
            m = res[key] = dict(m, **run(m["vert_lattice"], _faces(m), origin=origin, resol=resol, **kw))
        elif keeps == "vertices":                               # vertices stay: the new faces take the place of the old
            r = run(m["vert_lattice"], _faces(m), resol=resol, **kw)
            r["faces" if "faces" in m else "quads"] = r.pop("faces")
            m = res[key] = dict(m, **r)
        else:                                                   # a new mesh: the next stage reads these four of it
            res[key] = run(m["vert_lattice"], _faces(m), origin=origin, resol=resol, vert_src=m["vert_src"], **kw)
            m = {k: res[key][k] for k in ("vertices", "vert_lattice", "faces", "vert_src")}
    return res


def save_mesh_2ply(path, vertices, faces, normal_np=None, rgb_np=None):
    """Binary little-endian PLY: vertices (V,3) float32 x y z [+ nx ny nz float32] [+ red green blue uchar], faces (F,3) or (F,4) as
    `property list uchar int vertex_indices`."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces)
    if f.ndim != 2 or f.shape[1] not in (3, 4):
        raise ValueError("faces must be (F,3) or (F,4)")
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError("a face names a vertex outside [0, %d)" % v.shape[0])
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % v.shape[0], "property float x", "property float y", "property float z"]
    if normal_np is not None:
        nrm = np.asarray(normal_np, dtype=np.float32).reshape(-1, 3)
        if nrm.shape[0] != v.shape[0]:
            raise ValueError("%d vertices, %d normals" % (v.shape[0], nrm.shape[0]))
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        header += ["property float nx", "property float ny", "property float nz"]
    if rgb_np is not None:
        rgb = np.asarray(rgb_np, dtype=np.uint8).reshape(-1, 3)
        if rgb.shape[0] != v.shape[0]:
            raise ValueError("%d vertices, %d colours" % (v.shape[0], rgb.shape[0]))
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += ["element face %d" % f.shape[0], "property list uchar int vertex_indices", "end_header"]
    rec = np.zeros((v.shape[0],), dtype=fields)
    rec["x"], rec["y"], rec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if normal_np is not None:
        rec["nx"], rec["ny"], rec["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    if rgb_np is not None:
        rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    k = f.shape[1]
    frec = np.zeros((f.shape[0],), dtype=[("n", "u1"), ("v", "<i4", (k,))])
    frec["n"], frec["v"] = k, f.astype(np.int32)
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(rec.tobytes())
        fh.write(frec.tobytes())


def save_stage_2ply(path, m, normal_list, rgb_list=None, normals="source", rgb_np=None):
    """save_mesh_2ply of a stage's mesh m - extract_mesh's dict or one of run_chain's - with the attributes of its vertices: every stage keeps
    vert_src, so a vertex's normal and colour are row vert_src of the concatenated per-voxel normal_list / rgb_list (None or empty: no
    colours), and zero where vert_src < 0 (mesh_reach > 0: a vertex with no oriented cell beside it). normals="mesh" writes the mesh's own
    normals in their place: mesh_normals of the stage's vert_lattice and faces, zero where that is zero; the
    colours stay gathered. ValueError for any other value before a file is opened. rgb_np (V,3) uint8 - colour_vertices' vert_rgb - is
    written as the vertices' colours in the place of the gathered ones; None: as before."""
    check_normals_arg(normals)
    src = m["vert_src"]

    def gather(lists, dtype):
        a = np.concatenate([np.asarray(x, dtype).reshape(-1, 3) for x in lists])[src]
        a[src < 0] = 0
        return a
    nrm = mesh_normals(m["vert_lattice"], _faces(m))["vert_normals"] if normals == "mesh" else gather(normal_list, np.float32)
    save_mesh_2ply(path, m["vertices"], _faces(m), normal_np=nrm, rgb_np=rgb_np if rgb_np is not None else (gather(rgb_list, np.uint8) if rgb_list else None))
