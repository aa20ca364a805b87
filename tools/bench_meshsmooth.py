"""Times the mesh smoother at DTU scale, next to sn_mesh on the same scene in the same run.

    python tools/bench_meshsmooth.py [--out profiles/meshsmooth/bench_meshsmooth.json] [--reps 5] [--iterations 10]

Scene: the "dtu" scene of tools/bench_postpass.py as tools/bench_meshsimplify.py sets it up, meshed by sn_mesh; the smoother runs on its quads
and on their triangulation. Before anything is reported the GPU result (3 iterations, curve mode) is compared with the restatement
(tests/meshsmooth_ref.py) on the whole mesh. Every time is the median of --reps runs after one warm-up:
  packed_ms / device_ms   Context.mesh_smooth at --iterations on host arrays (upload, kernels, readback) / with the mesh staged in device
                          memory by the caller
  kernel_ms, stages_ms    the kernels alone (the context's HIP-event profile) and their split; build_ms = mark + edges + degree + rows, the
                          adjacency; pass_ms = one launch of the pass kernel; topology_ms = the kernels of an iterations = 0 call
  pass_bytes              what one pass must move: per referenced vertex its own record and one write, per directed edge one neighbour record
                          and one row word; pass_GBps = that over pass_ms, pass_share_of_hbm = that over the 6.3 TB/s a float4 copy achieves on
                          this part. The positions of this scene fit the last-level cache, so the share is not bounded by 1
  mesh_*                  sn_mesh the same ways in the same run
No time is aimed at: the numbers are written down.
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

from bench_mesh import _kernel_ms, _median_time  # noqa: E402  (tools/ is on the path when this file is run as a script)
from bench_meshsimplify import _scene  # noqa: E402

HBM_ACHIEVABLE = 6.3e12        # bytes / s, float4 copy (as tools/bench_relwtrain.py takes it)
RECORD = 24                     # bytes of a position record in the product library
BUILD = ("msm_mark", "msm_edges", "msm_degree", "msm_rows")


def _median_stages(ctx, fn, reps):
    """-> {stage: median over reps of its time in one call}, and the launches of msm_pass in one call."""
    fn()
    runs = []
    for _ in range(reps):
        ctx.profile_enable(True)
        ctx.profile_reset()
        fn()
        prof = ctx.profile()
        ctx.profile_enable(False)
        ctx.profile_reset()
        runs.append({k: (v["ms"], v["launches"]) for k, v in prof.items() if k.startswith("msm_")})
    stages = {k: float(np.median([r[k][0] for r in runs])) for k in runs[0]}
    passes = int(runs[0].get("msm_pass", (0, 0))[1])
    return stages, passes


def _summary(stages, passes):
    out = dict(kernel_ms=float(sum(stages.values())), stages_ms=stages, build_ms=float(sum(stages.get(k, 0.0) for k in BUILD)), passes=passes)
    if passes:
        out["pass_ms"] = stages["msm_pass"] / passes
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshsmooth", "bench_meshsmooth.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=10)
    args = ap.parse_args()
    import meshsmooth_ref
    from surfacenet_amd import mesh, runtime
    ctx = runtime.any_context()
    run_m, m, origin, resol, counts = _scene(ctx)
    lat = np.ascontiguousarray(m["verts_lattice"], dtype=np.float64)
    faces = dict(quads=np.ascontiguousarray(m["quads"], dtype=np.int32), triangles=np.ascontiguousarray(mesh.triangulate(m["quads"]), dtype=np.int32))
    lam, mu = meshsmooth_ref.q16(0.5), meshsmooth_ref.q16(-0.53)
    run = lambda f, n=args.iterations, **kw: ctx.mesh_smooth(lat, f, n, lam, mu, 1, origin=origin, resol=resol, **kw)
    res = dict(tool="tools/bench_meshsmooth.py", resol=resol, reps=args.reps, iterations=args.iterations, lam_q16=lam, mu_q16=mu, boundary="curve",
               vertices=int(lat.shape[0]), hbm_achievable_TBps=HBM_ACHIEVABLE / 1e12, record_bytes=RECORD, meshes={}, **counts)
    try:
        res["box_probe"] = ctx.mfma_probe()
    except Exception as e:             # noqa: BLE001 - the probe only labels the box
        res["box_probe"] = "unavailable: %s" % e

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, default=float)

    for name, f in faces.items():
        row = res["meshes"][name] = dict(faces=int(f.shape[0]))
        t = time.perf_counter()
        want = meshsmooth_ref.smooth(lat, f, 3, lam, mu, 1, origin, resol)
        row["restatement_3_iterations_ms"] = 1e3 * (time.perf_counter() - t)
        got = run(f, 3)
        equal = all(np.array_equal(got[a], want[b]) for a, b in (("verts_lattice", "vert_lattice"), ("verts_mm", "vertices"), ("vert_degree", "vert_degree"),
                                                                 ("vert_flags", "vert_flags"), ("counts", "counts")))
        if not equal:
            raise SystemExit("%s: the GPU result differs from the restatement" % name)
        E, B, N, R = (int(x) for x in want["counts"])
        row.update(gpu_equal=True, edges=E, boundary_edges=B, nonmanifold_edges=N, referenced=R, max_degree=int(want["vert_degree"].max()),
                   moved_cells_max=float(np.abs(got["verts_lattice"] - lat).max()))
        del got, want
        row["packed_ms"] = _median_time(lambda: run(f), args.reps)
        row["device_ms"] = _median_time(lambda: run(f, device=True), args.reps)
        row.update(_summary(*_median_stages(ctx, lambda: run(f), args.reps)))
        topo = _summary(*_median_stages(ctx, lambda: run(f, 0), args.reps))
        row.update(topology_ms=topo["kernel_ms"], topology_packed_ms=_median_time(lambda: run(f, 0), args.reps))
        row["pass_bytes"] = R * 2 * RECORD + 2 * E * (RECORD + 4)
        row["pass_GBps"] = row["pass_bytes"] / (row["pass_ms"] * 1e-3) / 1e9
        row["pass_share_of_hbm"] = row["pass_bytes"] / (row["pass_ms"] * 1e-3) / HBM_ACHIEVABLE
    res["mesh_packed_ms"] = _median_time(run_m, args.reps)
    res["mesh_kernel_ms"], res["mesh_stages_ms"] = _kernel_ms(ctx, run_m, args.reps, ("ms_", "pc_sort"))
    for row in res["meshes"].values():
        row["ratio_to_mesh_kernel"] = row["kernel_ms"] / res["mesh_kernel_ms"]
        row["ratio_to_mesh_packed"] = row["packed_ms"] / res["mesh_packed_ms"]
    save()
    print(json.dumps(dict(mesh_kernel_ms=res["mesh_kernel_ms"], vertices=res["vertices"],
                          meshes={k: {a: b for a, b in row.items() if a in ("faces", "edges", "packed_ms", "device_ms", "kernel_ms", "build_ms", "pass_ms",
                                                                            "topology_ms", "pass_GBps", "pass_share_of_hbm", "ratio_to_mesh_kernel")}
                                  for k, row in res["meshes"].items()}), default=float))


if __name__ == "__main__":
    main()
