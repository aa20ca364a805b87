"""The DTU accuracy / completeness protocol of the reference (experiments/DTU/eval_ply.m, which calls PointCompareMain of the DTU kit), on the
MI355X. DESIGN.md section 4.7 states the contract and what of the kit (not part of the reference) is a documented choice here.

    read_ply_xyz     a PLY's vertex x, y, z (ascii, binary little / big endian; also the reference's scene.readPointCloud_xyz)
    reduce_points    reducePts_haa: greedy density reduction of the data cloud (minimum distance dst)
    max_dist_cp      MaxDistCP: nearest-neighbour distance from every point of one cloud to another, capped at max_dist
    point_compare    PointCompareMain: the BaseEval fields
    eval_acc_compl   eval_ply.m's four numbers from a BaseEval
    eval_ply         the drop-in for eval_ply.m: the DTU folder's files in, BaseEval .mat out, the four numbers back
    read_ply_mesh    a PLY mesh's vertices and faces (what mesh.save_mesh_2ply writes)
    mesh_compare     point_compare for a mesh: its surface sampled at the evaluation density first
    eval_mesh_ply    eval_ply for a mesh PLY

The reduction, the distances and the mask / plane flags run on the GPU (surfacenet_amd/csrc/pointeval.h); the statistics are numpy on the
host. A scene is evaluated in memory with sparseCubes.sparse_xyz (the points save_sparseCubes_2ply would write). Only the .mat I/O of
eval_ply needs scipy (imported there).
"""
import os

import numpy as np

from . import runtime

_PLY_SCALARS = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
                "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def _ply_header(f, lists=None):
    """-> (format, [(element, count, [(property, numpy type or None for a list)])]); the (count type, item type) of every list property are
    appended to `lists`, in file order, when it is given."""
    if f.readline().strip() != b"ply":
        raise ValueError("not a PLY file")
    fmt, elements = None, []
    while True:
        line = f.readline()
        if not line:
            raise ValueError("PLY header without end_header")
        tok = line.decode("ascii", "replace").split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "end_header":
            return fmt, elements
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if tok[1] == "list":
                elements[-1][2].append((tok[4], None))
                if lists is not None:
                    lists.append((_PLY_SCALARS[tok[2]], _PLY_SCALARS[tok[3]]))
            else:
                elements[-1][2].append((tok[2], _PLY_SCALARS[tok[1]]))


def read_ply_xyz(path):
    """(N,3) array of the vertex element's x, y, z (dtype as stored, promoted across the three). The vertex element may be preceded only by
    elements of fixed size (no list properties)."""
    with open(path, "rb") as f:
        fmt, elements = _ply_header(f)
        body = f.read()
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise ValueError("unknown PLY format %r" % fmt)
    skip = 0
    for name, count, props in elements:
        if name == "vertex":
            break
        if any(t is None for _, t in props):
            raise ValueError("element %r before the vertices has list properties: unsupported" % name)
        skip += count * (1 if fmt == "ascii" else sum(np.dtype(t).itemsize for _, t in props))
    else:
        raise ValueError("PLY file without a vertex element")
    if any(t is None for _, t in props):
        raise ValueError("vertex element with list properties: unsupported")
    names = [p for p, _ in props]
    if fmt == "ascii":
        lines = body.decode("ascii").splitlines()
        lines = [ln for ln in lines if ln.strip()][skip:skip + count]
        vals = np.asarray([ln.split() for ln in lines], dtype=object).reshape(count, len(props))
        cols = [vals[:, names.index(k)].astype(np.float64).astype(dict(props)[k]) for k in ("x", "y", "z")]
    else:
        end = "<" if fmt == "binary_little_endian" else ">"
        dt = np.dtype([(p, end + t) for p, t in props])
        v = np.frombuffer(body, dtype=dt, count=count, offset=skip)
        cols = [v[k].astype(v[k].dtype.newbyteorder("=")) for k in ("x", "y", "z")]
    return np.stack(cols, axis=1) if count else np.zeros((0, 3), np.result_type(*cols))


def read_ply_mesh(path):
    """-> (vertices (V,3), faces (F,3) or (F,4) int32) of a PLY mesh: the vertex element's x, y, z (dtype as stored) and the one list property
    of the face element, in ascii and both binary byte orders; what mesh.save_mesh_2ply writes. Scalar properties beside them are skipped.
    ValueError for faces of mixed size, faces that are neither triangles nor quads, or a list property anywhere else before the faces."""
    lists = []
    with open(path, "rb") as f:
        fmt, elements = _ply_header(f, lists)
        body = f.read()
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise ValueError("unknown PLY format %r" % fmt)
    ascii_ = fmt == "ascii"
    end = "<" if fmt == "binary_little_endian" else ">"
    if ascii_:
        body = [ln.split() for ln in body.decode("ascii").splitlines() if ln.strip()]
    pos, verts, faces = 0, None, None                        # pos: bytes (binary) or lines (ascii) consumed
    for name, count, props in elements:
        n_lists = sum(t is None for _, t in props)
        if name == "face" and n_lists == 1:
            ct, it = lists[0]
            at = [t is None for _, t in props].index(True)   # scalar properties before the list
            if count == 0:
                faces = np.zeros((0, 3), np.int32)
            elif ascii_:
                rows = body[pos:pos + count]
                if len(rows) != count:
                    raise ValueError("PLY file ends inside the faces")
                k = int(rows[0][at])
                if any(len(r) != len(props) + k or int(r[at]) != k for r in rows):
                    raise ValueError("faces of mixed size")
                faces = np.asarray([r[at + 1:at + 1 + k] for r in rows], dtype=np.int64)
            else:
                head = sum(np.dtype(t).itemsize for _, t in props[:at])
                if len(body) < pos + head + np.dtype(ct).itemsize:
                    raise ValueError("PLY file ends inside the faces")
                k = int(np.frombuffer(body, dtype=end + ct, count=1, offset=pos + head)[0])
                dt = np.dtype([(p, end + t) if t else (p, [("n", end + ct), ("v", end + it, (k,))]) for p, t in props])
                if len(body) < pos + count * dt.itemsize:
                    raise ValueError("faces of mixed size, or a file that ends inside them")
                rec = np.frombuffer(body, dtype=dt, count=count, offset=pos)[props[at][0]]
                if (rec["n"] != k).any():
                    raise ValueError("faces of mixed size")
                faces = rec["v"].astype(np.int64)
                pos += count * dt.itemsize
            if count and faces.shape[1] not in (3, 4):
                raise ValueError("faces of %d vertices: triangles and quads only" % faces.shape[1])
            if count and (faces.min() < -(1 << 31) or faces.max() >= 1 << 31):
                raise ValueError("a face index does not fit int32")
            faces = np.ascontiguousarray(faces, dtype=np.int32)
            if ascii_:
                pos += count
        elif n_lists:
            if verts is not None and faces is not None:
                break
            raise ValueError("element %r has list properties: unsupported" % name)
        else:
            names = [p for p, _ in props]
            if name == "vertex":
                if ascii_:
                    rows = body[pos:pos + count]
                    if len(rows) != count:
                        raise ValueError("PLY file ends inside the vertices")
                    vals = np.asarray(rows, dtype=object).reshape(count, len(props))
                    cols = [vals[:, names.index(c)].astype(np.float64).astype(dict(props)[c]) for c in ("x", "y", "z")]
                else:
                    dt = np.dtype([(p, end + t) for p, t in props])
                    v = np.frombuffer(body, dtype=dt, count=count, offset=pos)
                    cols = [v[c].astype(v[c].dtype.newbyteorder("=")) for c in ("x", "y", "z")]
                verts = np.stack(cols, axis=1) if count else np.zeros((0, 3), np.result_type(*cols))
            pos += count * (1 if ascii_ else sum(np.dtype(t).itemsize for _, t in props))
        lists = lists[n_lists:]
    if verts is None:
        raise ValueError("PLY file without a vertex element")
    if faces is None:
        raise ValueError("PLY file without a face element that holds one list property")
    return verts, faces


def _points(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 3))


def reduce_points(pts, dst=0.2, seed=0, order=None, return_index=False):
    """reducePts_haa(Qdata, dst): visit the points in `order` (default np.random.RandomState(seed).permutation(n); the kit's MATLAB randperm
    cannot be reproduced); a point still alive removes every other point within d^2 <= dst^2. Returns the survivors in ascending index order
    (and their indices)."""
    p = _points(pts)
    n = p.shape[0]
    order = np.random.RandomState(seed).permutation(n) if order is None else np.asarray(order, dtype=np.int64).reshape(-1)
    if order.size != n or not np.array_equal(np.sort(order), np.arange(n)):
        raise ValueError("order must be a permutation of range(%d)" % n)
    rank = np.empty((n,), np.int64)
    rank[order] = np.arange(n)
    keep, _ = runtime.any_context().point_reduce(p, rank, dst)
    idx = np.nonzero(keep)[0]
    return (p[idx], idx) if return_index else p[idx]


def max_dist_cp(Qto, Qfrom, max_dist=60.0):
    """MaxDistCP(Qto, Qfrom, BB, MaxDist): for every point of Qfrom, min(sqrt(min_j d^2), max_dist), and max_dist when Qto is empty. Exact at
    every distance. The kit's answer beyond max_dist depends on its block tiling (BB), which is not known; here it is max_dist, and BB plays
    no part in the distances."""
    d2 = runtime.any_context().nn_dist2(_points(Qto), _points(Qfrom), max_dist)
    return np.minimum(np.sqrt(d2), float(max_dist))


def point_compare(Qdata, Qstl, obs_mask, BB, Res, plane, dst=0.2, max_dist=60.0, seed=0, order=None, cSet=None, Margin=None):
    """PointCompareMain(cSet, Qdata, dst, dataPath) on arrays: Qdata, Qstl (N,3); obs_mask (X,Y,Z) uint8, BB (2,3) and Res of the ObsMask file;
    plane (4,) of the Plane file. Returns the BaseEval fields: cSet, Margin, dst, Qdata (the reduced data cloud), Ddata, Qstl, Dstl,
    DataInMask, GroundPlane, StlAbovePlane (points (N,3), per-point arrays (N,))."""
    ctx = runtime.any_context()
    Qd = reduce_points(Qdata, dst, seed, order)
    Qs = _points(Qstl)
    BB = np.asarray(BB, dtype=np.float64).reshape(2, 3)
    plane = np.asarray(plane, dtype=np.float64).reshape(4)
    in_mask, _ = ctx.point_flags(Qd, mask=obs_mask, bb_min=BB[0], res=float(np.asarray(Res, dtype=np.float64).reshape(-1)[0]))
    _, above = ctx.point_flags(Qs, plane=plane)
    return dict(cSet=cSet, Margin=Margin, dst=float(dst), Qdata=Qd, Ddata=max_dist_cp(Qs, Qd, max_dist), Qstl=Qs, Dstl=max_dist_cp(Qd, Qs, max_dist),
                DataInMask=in_mask, GroundPlane=plane, StlAbovePlane=above)


def eval_acc_compl(base):
    """eval_ply.m's result: [mean, median] of Ddata .* DataInMask, then of Dstl .* StlAbovePlane - products over ALL points (points outside the
    mask / below the plane count as 0), as eval_ply.m computes them. float64."""
    acc = np.asarray(base["Ddata"], dtype=np.float64) * np.asarray(base["DataInMask"], dtype=np.float64)
    compl = np.asarray(base["Dstl"], dtype=np.float64) * np.asarray(base["StlAbovePlane"], dtype=np.float64)
    return np.asarray([np.mean(acc), np.median(acc), np.mean(compl), np.median(compl)], dtype=np.float64)


def eval_ply(cSet, DataInName, EvalName, dataPath, dst=0.2, max_dist=60.0, seed=0):
    """eval_ply.m (getPaths' dataPath passed in): reads DataInName (PLY), dataPath/Points/stl/stl{cSet:03d}_total.ply,
    dataPath/ObsMask/ObsMask{cSet}_10.mat (BB, Res, Margin, ObsMask) and dataPath/ObsMask/Plane{cSet}.mat (P); writes EvalName (.mat, variable
    BaseEval, point arrays 3 x N as MATLAB holds them); returns the four numbers of eval_acc_compl."""
    Qdata = read_ply_xyz(DataInName)
    Qstl, m, P = _dtu_files(cSet, dataPath)
    base = point_compare(Qdata, Qstl, m["ObsMask"], m["BB"], m["Res"], P, dst=dst, max_dist=max_dist, seed=seed, cSet=cSet,
                         Margin=m["Margin"] if "Margin" in m else None)
    _save_base_eval(EvalName, base, cSet)
    return eval_acc_compl(base)


def _dtu_files(cSet, dataPath):
    """The DTU folder's files of scan cSet -> (Qstl, the ObsMask file's variables, P)."""
    import scipy.io as sio
    Qstl = read_ply_xyz(os.path.join(dataPath, "Points", "stl", "stl%03d_total.ply" % cSet))
    m = sio.loadmat(os.path.join(dataPath, "ObsMask", "ObsMask%d_10.mat" % cSet))
    P = sio.loadmat(os.path.join(dataPath, "ObsMask", "Plane%d.mat" % cSet))["P"]
    return Qstl, m, P


def _save_base_eval(EvalName, base, cSet):
    import scipy.io as sio
    mat = dict(base)
    mat.update(cSet=float(cSet), Qdata=base["Qdata"].T, Qstl=base["Qstl"].T, GroundPlane=base["GroundPlane"].reshape(4, 1))
    if mat["Margin"] is None:
        del mat["Margin"]
    sio.savemat(EvalName, {"BaseEval": mat})


def mesh_compare(vertices, faces, Qstl, obs_mask, BB, Res, plane, dst=0.2, sample_dst=None, max_dist=60.0, seed=0, order=None, cSet=None,
                 Margin=None, completeness="samples"):
    """The DTU practice for a mesh: sample its surface at sample_dst (default dst; mesh.sample_surface), then
    point_compare on the samples, which reduces them at dst. vertices (V,3), faces (F,3) or (F,4). Returns point_compare's BaseEval fields plus
    n_samples and n_faces. completeness="samples" (the default) measures Dstl, the distance from every point of Qstl to the reconstruction,
    to the reduced samples: up to 2/3 sample_dst too large. completeness="surface" measures it to the mesh's surface itself
    (mesh.point_to_mesh), capped at max_dist as the protocol caps it, and says so under the key "completeness" -
    a dict without that key was measured to the samples. Ddata comes from the samples either way."""
    from . import mesh
    if completeness not in ("samples", "surface"):
        raise ValueError("completeness = %r: \"samples\" or \"surface\"" % (completeness,))
    points, _ = mesh.sample_surface(vertices, faces, dst if sample_dst is None else sample_dst)
    base = point_compare(points, Qstl, obs_mask, BB, Res, plane, dst=dst, max_dist=max_dist, seed=seed, order=order, cSet=cSet, Margin=Margin)
    base.update(n_samples=int(points.shape[0]), n_faces=int(np.asarray(faces).shape[0]))
    if completeness == "surface":
        base.update(Dstl=mesh.point_to_mesh(base["Qstl"], vertices, faces, max_dist)["dist"], completeness="surface")
    return base


def eval_mesh_ply(cSet, MeshInName, EvalName, dataPath, dst=0.2, sample_dst=None, max_dist=60.0, seed=0, completeness="samples"):
    """eval_ply for a mesh PLY (read_ply_mesh): the same DTU files in, the same BaseEval .mat out (plus n_samples and n_faces), the four numbers
    of eval_acc_compl back. completeness as mesh_compare takes it."""
    vertices, faces = read_ply_mesh(MeshInName)
    Qstl, m, P = _dtu_files(cSet, dataPath)
    base = mesh_compare(vertices, faces, Qstl, m["ObsMask"], m["BB"], m["Res"], P, dst=dst, sample_dst=sample_dst, max_dist=max_dist, seed=seed,
                        cSet=cSet, Margin=m["Margin"] if "Margin" in m else None, completeness=completeness)
    _save_base_eval(EvalName, base, cSet)
    return eval_acc_compl(base)
