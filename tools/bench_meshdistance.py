"""Times the point-to-mesh distance stage at DTU scale, next to the way the same quantity is obtained today - the
capped nearest-neighbour distance to the mesh's surface samples (sn_nn_dist2, section 4.7) - from the same queries in the same run.

    python tools/bench_meshdistance.py [--out profiles/meshdistance/bench_meshdistance.json] [--reps 5]

Scene: the "dtu" scene of tools/bench_postpass.py as tools/bench_meshsimplify.py sets it up, meshed by sn_mesh and triangulated, in world
mm; the stage runs on the mesh as extracted and after mesh.simplify_mesh(cell=2). Queries: the mesh's own mesh.sample_surface(dst = resol)
samples, and those samples with 2 % uniform outliers in the mesh's box (section 4.7's outlier case). The restatement
(tests/meshdistance_ref.py) is brute force over all triangles and cannot run at a million of them: it is compared, bit for bit, on a crop
of the 3,000 triangles nearest the mesh's centre with 2,000 of the queries, host and device form; on the whole mesh the host form and the
device form are compared with each other. Every time is the median of --reps runs after one warm-up:
  packed_ms / device_ms   Context.mesh_distance on host arrays (upload, kernels, readback) / with mesh and points staged in device memory
  stages_ms               the kernels alone (the context's HIP-event profile): mdi_points, mdi_tris, mdi_grid, mdi_near, mdi_far, mdi_emit
  level, entries          the grid level the broad phase picks and its (cell, triangle) entries, restated in numpy
  tests_per_query         counts[4] / queries
  nn_dist2_ms             Context.nn_dist2 from the same queries to mesh.sample_surface(mesh, dst): today's way to the same quantity
No time is aimed at: the numbers are written down.

    python tools/bench_meshdistance.py --case NAME --save OUT.npz      (the tests' child: a named case of tests/meshdistance_ref.py, its
                                                                        outputs saved as they came back)
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

MAX_DIST = 60.0


def _meshes(ctx):
    from surfacenet_amd import mesh
    _, m, origin, resol, counts = _scene(ctx)
    lat = np.ascontiguousarray(m["verts_lattice"], dtype=np.float64)
    tris = np.ascontiguousarray(mesh.triangulate(m["quads"]), dtype=np.int32)
    simple = mesh.simplify_mesh(lat, tris, 2, origin=origin, resol=resol)
    world = lambda x: np.ascontiguousarray(np.asarray(x, np.float64))
    meshes = dict(extracted=(world(m["verts_mm"]), tris), simplified_2=(world(simple["vertices"]), np.ascontiguousarray(simple["faces"], dtype=np.int32)))
    return meshes, resol, counts


def _crop(v, f, n=3000):
    centre = v[np.unique(f)].mean(axis=0)
    d = np.linalg.norm(v[f].mean(axis=1) - centre, axis=1)
    return np.ascontiguousarray(f[np.sort(np.argsort(d, kind="stable")[:n])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshdistance", "bench_meshdistance.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", help="run a named case of tests/meshdistance_ref.py (the tests' child)")
    ap.add_argument("--save", help="... and save its outputs here")
    args = ap.parse_args()
    import meshdistance_ref as ref
    from surfacenet_amd import mesh, runtime
    ctx = runtime.any_context()
    if args.case:
        v, f, pts, max_dist = ref.CASES[args.case]()
        got = ctx.mesh_distance(v, f, pts, max_dist)
        np.savez(args.save, **{k: got[k] for k in ref.KEYS})
        return
    meshes, resol, counts = _meshes(ctx)
    res = dict(tool="tools/bench_meshdistance.py", resol=resol, max_dist=MAX_DIST, reps=args.reps, meshes={}, **counts)
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
        level, entries, cell = ref.grid_level(v, f, MAX_DIST)
        row.update(level=level, entries=entries, entries_per_triangle=entries / max(f.shape[0], 1), cell_mm=cell)
        samples, _ = mesh.sample_surface(v, f, resol)
        lo, hi = v[np.unique(f)].min(axis=0), v[np.unique(f)].max(axis=0)
        outliers = rs.uniform(lo, hi, (samples.shape[0] // 50, 3))
        crop = _crop(v, f)
        for qname, pts in (("samples", samples), ("samples_outliers", np.ascontiguousarray(np.concatenate([samples, outliers])))):
            q = row["queries"][qname] = dict(points=int(pts.shape[0]))
            run = lambda **kw: ctx.mesh_distance(v, f, pts, MAX_DIST, **kw)
            got, dev = run(), run(device=True)
            differs = [k for k in ref.KEYS if got[k].tobytes() != dev[k].tobytes()]
            if differs:
                raise SystemExit("%s/%s: the host form and the device form differ on %s" % (name, qname, differs))
            q.update(forms_equal=True, tests_per_query=int(got["counts"][4]) / max(pts.shape[0], 1), **dict(zip(ref.COUNTS, (int(x) for x in got["counts"]))))
            d = np.sqrt(got["d2"][np.isfinite(got["d2"])])
            q.update(dist_max=float(d.max()), dist_mean=float(d.mean()))
            sub = np.ascontiguousarray(pts[rs.choice(pts.shape[0], min(2000, pts.shape[0]), replace=False)])
            t = time.perf_counter()
            want = ref.distance(v, crop, sub, MAX_DIST)
            q["crop"] = dict(faces=int(crop.shape[0]), points=int(sub.shape[0]), restatement_ms=1e3 * (time.perf_counter() - t))
            bad = ref.same_bits(ctx.mesh_distance(v, crop, sub, MAX_DIST), want) + ref.same_bits(ctx.mesh_distance(v, crop, sub, MAX_DIST, device=True), want)
            if bad:
                raise SystemExit("%s/%s: the GPU result differs from the restatement on the crop's %s" % (name, qname, bad))
            q["crop"]["gpu_equal"] = True
            q["packed_ms"] = _median_time(run, args.reps)
            q["device_ms"] = _median_time(lambda: run(device=True), args.reps)
            stages = _median_stages(ctx, run, args.reps, "mdi_")
            q.update(kernel_ms=float(sum(stages.values())), stages_ms=stages)
            # today's way: the capped nearest-neighbour distance from the same queries to the mesh's samples
            q["nn_dist2_ms"] = _median_time(lambda: ctx.nn_dist2(samples, pts, MAX_DIST), args.reps)
            nn = _median_stages(ctx, lambda: ctx.nn_dist2(samples, pts, MAX_DIST), args.reps, "pe_")
            q["nn_dist2_stages_ms"] = nn
            q["nn_dist2_kernel_ms"] = float(sum(nn.values()))
            near = np.minimum(np.sqrt(ctx.nn_dist2(samples, pts, MAX_DIST)), MAX_DIST)
            q["nn_minus_surface_max"] = float((near - np.minimum(np.sqrt(got["d2"]), MAX_DIST)).max())
            save()
    print(json.dumps(res["meshes"], default=float))


if __name__ == "__main__":
    main()
