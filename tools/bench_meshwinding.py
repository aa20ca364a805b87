"""Times the winding-number stage at DTU scale, next to the only per-point mesh query the project had before it -
the point-to-mesh distance (sn_mesh_distance, section 4.24) - on the same queries in the same run.

    python tools/bench_meshwinding.py [--out profiles/meshwinding/bench_meshwinding.json] [--reps 5]

Scene: the "dtu" scene of tools/bench_postpass.py as tools/bench_meshsimplify.py sets it up, meshed by sn_mesh and triangulated, in lattice
cells; the stage runs on the mesh as extracted and after mesh.simplify_mesh(cell=2). Queries: the mesh's own mesh.sample_surface(dst = 1
cell) samples displaced by half a cell along the normal of their face's three vertex normals (mesh.mesh_normals), outwards and inwards in
turn, and uniform points in the mesh's box. The restatement (tests/meshwinding_ref.py) is brute force over all triangles: it is compared,
byte for byte, on a crop of the 3,000 triangles nearest the mesh's centre with 2,000 of the queries, host and device form and every axis; on
the whole mesh the host form and the device form are compared with each other. Every time is the median of --reps runs after one warm-up:
  packed_ms / device_ms   Context.mesh_winding on host arrays (upload, kernels, readback) / with mesh and points staged in device memory
  stages_ms               the kernels alone (the context's HIP-event profile): wnd_points, wnd_tris, wnd_grid, wnd_query, wnd_emit
  level, entries          the grid level the broad phase picks and its (cell, triangle) entries, restated in numpy
  tests_per_query         counts[4] / queries
  distance_ms             Context.mesh_distance on the same queries (max_dist 60 mm in cells), host arrays; distance_kernel_ms its kernels
No time is aimed at: the numbers are written down.

    python tools/bench_meshwinding.py --case NAME --axis A --save OUT.npz      (the tests' child: a named case of tests/meshwinding_ref.py,
                                                                                its outputs saved as they came back)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_mesh import _median_time  # noqa: E402  (tools/ is on the path when this file is run as a script)
from bench_meshnormals import _median_stages  # noqa: E402
from bench_meshsimplify import _scene  # noqa: E402

MAX_DIST_MM = 60.0
UNIFORM = 200000


def _meshes(ctx):
    from surfacenet_amd import mesh
    _, m, origin, resol, counts = _scene(ctx)
    lat = np.ascontiguousarray(m["verts_lattice"], dtype=np.float64)
    tris = np.ascontiguousarray(mesh.triangulate(m["quads"]), dtype=np.int32)
    simple = mesh.simplify_mesh(lat, tris, 2, origin=origin, resol=resol)
    meshes = dict(extracted=(lat, tris), simplified_2=(np.ascontiguousarray(simple["vert_lattice"], dtype=np.float64),
                                                       np.ascontiguousarray(simple["faces"], dtype=np.int32)))
    return meshes, resol, counts


def _crop(v, f, n=3000):
    centre = v[np.unique(f)].mean(axis=0)
    d = np.linalg.norm(v[f].mean(axis=1) - centre, axis=1)
    return np.ascontiguousarray(f[np.sort(np.argsort(d, kind="stable")[:n])])


def _displaced(v, f):
    """The surface samples at one per cell, half a cell off the surface along their face's summed vertex normals, out and in in turn."""
    from surfacenet_amd import mesh
    samples, tri = mesh.sample_surface(v, f, 1.0)
    vn = np.asarray(mesh.mesh_normals(v, f)["vert_normals"], np.float64)
    n = vn[f[tri]].sum(axis=1)
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
    sign = np.where(np.arange(samples.shape[0]) % 2 == 0, 0.5, -0.5)[:, None]
    return np.ascontiguousarray(np.clip(samples + sign * n, -4.0, 2097143.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshwinding", "bench_meshwinding.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", help="run a named case of tests/meshwinding_ref.py (the tests' child)")
    ap.add_argument("--axis", type=int, default=2)
    ap.add_argument("--save", help="... and save its outputs here")
    args = ap.parse_args()
    import meshwinding_ref as ref
    from surfacenet_amd import runtime
    ctx = runtime.any_context()
    if args.case:
        v, f, pts = ref.CASES[args.case]()
        got = ctx.mesh_winding(v, f, pts, axis=args.axis)
        np.savez(args.save, **{k: got[k] for k in ref.KEYS})
        return
    meshes, resol, counts = _meshes(ctx)
    max_dist = MAX_DIST_MM / resol
    res = dict(tool="tools/bench_meshwinding.py", resol=resol, max_dist_cells=max_dist, reps=args.reps, meshes={}, **counts)
    try:
        res["box_probe"] = ctx.mfma_probe()
    except Exception as e:             # noqa: BLE001 - the probe only labels the box
        res["box_probe"] = "unavailable: %s" % e

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, default=float)

    rs = np.random.RandomState(5)
    for name, (v, f) in meshes.items():
        row = res["meshes"][name] = dict(faces=int(f.shape[0]), vertices=int(v.shape[0]), queries={})
        level, entries = ref.grid_level(v, f)
        row.update(level=level, entries=entries, entries_per_triangle=entries / max(f.shape[0], 1))
        lo, hi = v[np.unique(f)].min(axis=0), v[np.unique(f)].max(axis=0)
        crop = _crop(v, f)
        for qname, pts in (("displaced_samples", _displaced(v, f)), ("uniform", np.ascontiguousarray(rs.uniform(lo, hi, (UNIFORM, 3))))):
            q = row["queries"][qname] = dict(points=int(pts.shape[0]))
            run = lambda **kw: ctx.mesh_winding(v, f, pts, **kw)
            got, dev = run(), run(device=True)
            differs = [k for k in ref.KEYS if got[k].tobytes() != dev[k].tobytes()]
            if differs:
                raise SystemExit("%s/%s: the host form and the device form differ on %s" % (name, qname, differs))
            q.update(forms_equal=True, tests_per_query=int(got["counts"][4]) / max(pts.shape[0], 1), **dict(zip(ref.COUNTS[:6], (int(x) for x in got["counts"][:6]))))
            hist = np.bincount(np.clip(got["winding"].astype(np.int64) + 2, 0, 4), minlength=5)
            q["winding_histogram"] = dict(zip(("<=-2", "-1", "0", "1", ">=2"), (int(x) for x in hist)))
            sub = np.ascontiguousarray(pts[rs.choice(pts.shape[0], min(2000, pts.shape[0]), replace=False)])
            q["crop"] = dict(faces=int(crop.shape[0]), points=int(sub.shape[0]))
            for axis in (0, 1, 2):
                t = time.perf_counter()
                want = ref.winding(v, crop, sub, axis)
                q["crop"]["restatement_ms_axis%d" % axis] = 1e3 * (time.perf_counter() - t)
                bad = ref.same_bytes(ctx.mesh_winding(v, crop, sub, axis=axis), want) + ref.same_bytes(ctx.mesh_winding(v, crop, sub, axis=axis, device=True), want)
                if bad:
                    raise SystemExit("%s/%s: the GPU result differs from the restatement on the crop's %s (axis %d)" % (name, qname, bad, axis))
            q["crop"]["gpu_equal"] = True
            q["packed_ms"] = _median_time(run, args.reps)
            q["device_ms"] = _median_time(lambda: run(device=True), args.reps)
            stages = _median_stages(ctx, run, args.reps, "wnd_")
            q.update(kernel_ms=float(sum(stages.values())), stages_ms=stages)
            # the per-point mesh query the project had before: the distance to the same mesh from the same queries
            dist = lambda: ctx.mesh_distance(v, f, pts, max_dist)
            q["distance_ms"] = _median_time(dist, args.reps)
            ds = _median_stages(ctx, dist, args.reps, "mdi_")
            q.update(distance_kernel_ms=float(sum(ds.values())), distance_stages_ms=ds)
            save()
    print(json.dumps(res["meshes"], default=float))


if __name__ == "__main__":
    main()
