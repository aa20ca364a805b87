"""Times the hole filler at DTU scale, next to the smoother's topology query and sn_mesh on the same scene in the same run.

    python tools/bench_meshfill.py [--out profiles/meshfill/bench_meshfill.json] [--reps 5]

Scene: the "dtu" scene of tools/bench_postpass.py as tools/bench_meshsimplify.py sets it up, meshed by sn_mesh; the filler runs on its quads and
on their triangulation at max_len 16, 64 and 1024, orientation 0. Before anything is reported the GPU result at every max_len is compared with
the restatement (tests/meshfill_ref.py) on the whole mesh. Every time is the median of --reps runs after one warm-up:
  packed_ms               Context.mesh_fill on host arrays (upload, kernels, readback)
  kernel_ms, stages_ms    the kernels alone (the context's HIP-event profile) and their split; build_ms = the smoother's edge table
                          (msm_mark + msm_edges + msm_degree), fill_ms = the filler's own kernels (mfl_*)
  topology_*              sn_mesh_smooth(iterations = 0), which builds the same edge table, the same ways in the same run
  mesh_*                  sn_mesh the same ways in the same run
  ratio_to_*              kernel_ms over the other call's kernels
  loops                   the restatement's histogram of the simple loops' lengths (powers of two), and the share of the boundary edges that lie on
                          filled loops
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

BUILD = ("msm_mark", "msm_edges", "msm_degree")
MAX_LENS = (16, 64, 1024)


def _median_stages(ctx, fn, reps):
    """-> {stage: median over reps of its time in one call}."""
    fn()
    runs = []
    for _ in range(reps):
        ctx.profile_enable(True)
        ctx.profile_reset()
        fn()
        prof = ctx.profile()
        ctx.profile_enable(False)
        ctx.profile_reset()
        runs.append({k: v["ms"] for k, v in prof.items() if k.startswith(("msm_", "mfl_"))})
    return {k: float(np.median([r[k] for r in runs])) for k in runs[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshfill", "bench_meshfill.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import meshfill_ref
    from surfacenet_amd import mesh, runtime
    ctx = runtime.any_context()
    run_m, m, origin, resol, counts = _scene(ctx)
    lat = np.ascontiguousarray(m["verts_lattice"], dtype=np.float64)
    faces = dict(quads=np.ascontiguousarray(m["quads"], dtype=np.int32), triangles=np.ascontiguousarray(mesh.triangulate(m["quads"]), dtype=np.int32))
    res = dict(tool="tools/bench_meshfill.py", resol=resol, reps=args.reps, orientation="holes", vertices=int(lat.shape[0]), meshes={}, **counts)
    try:
        res["box_probe"] = ctx.mfma_probe()
    except Exception as e:             # noqa: BLE001 - the probe only labels the box
        res["box_probe"] = "unavailable: %s" % e

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, default=float)

    for name, f in faces.items():
        row = res["meshes"][name] = dict(faces=int(f.shape[0]), max_len={})
        topo = _median_stages(ctx, lambda: ctx.mesh_smooth(lat, f, 0, origin=origin, resol=resol), args.reps)
        row.update(topology_kernel_ms=float(sum(topo.values())), topology_stages_ms=topo,
                   topology_packed_ms=_median_time(lambda: ctx.mesh_smooth(lat, f, 0, origin=origin, resol=resol), args.reps))
        for max_len in MAX_LENS:
            run = lambda: ctx.mesh_fill(lat, f, max_len, 0, origin=origin, resol=resol)
            t = time.perf_counter()
            want = meshfill_ref.fill(lat, f, max_len, 0, origin, resol)
            cell = row["max_len"][str(max_len)] = dict(restatement_ms=1e3 * (time.perf_counter() - t))
            got = run()
            equal = all(np.array_equal(got[a], want[b]) for a, b in (("new_verts_lattice", "new_vert_lattice"), ("loop_root", "loop_root"),
                                                                     ("loop_len", "loop_len"), ("new_faces", "new_faces"),
                                                                     ("vert_loop", "vert_loop"), ("counts", "counts")))
            cell["mm_equal"] = bool(np.array_equal(got["new_verts_mm"], want["new_vertices"]))
            if not equal:
                raise SystemExit("%s, max_len %d: the GPU result differs from the restatement" % (name, max_len))
            c = [int(x) for x in want["counts"]]
            cell.update(gpu_equal=True, counts=dict(zip(meshfill_ref.COUNT_NAMES, c)), zero_votes=int(want["zero_votes"]),
                        boundary_edges_on_filled_loops=int(want["loop_len"].sum()),
                        share_of_boundary_edges_filled=float(want["loop_len"].sum()) / max(c[1], 1))
            if max_len == MAX_LENS[-1]:
                simple = np.asarray([lp["n"] for lp in want["loops"] if lp["state"] != meshfill_ref.COMPLEX], np.int64)
                edges = [3, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 1 << 62]
                row["loops"] = dict(simple_loops=int(simple.size), length_histogram={"%d..%d" % (a, b - 1) if b < 1 << 62 else ">=%d" % a: int(((simple >= a) & (simple < b)).sum())
                                                                                      for a, b in zip(edges[:-1], edges[1:])},
                                    longest_simple_loop=int(simple.max(initial=0)), complex_components=c[6])
            del got, want
            cell["packed_ms"] = _median_time(run, args.reps)
            stages = _median_stages(ctx, run, args.reps)
            cell.update(kernel_ms=float(sum(stages.values())), stages_ms=stages, build_ms=float(sum(stages.get(k, 0.0) for k in BUILD)),
                        fill_ms=float(sum(v for k, v in stages.items() if k.startswith("mfl_"))))
            cell["ratio_to_topology_kernel"] = cell["kernel_ms"] / row["topology_kernel_ms"]
            save()
    res["mesh_packed_ms"] = _median_time(run_m, args.reps)
    res["mesh_kernel_ms"], res["mesh_stages_ms"] = _kernel_ms(ctx, run_m, args.reps, ("ms_", "pc_sort"))
    for row in res["meshes"].values():
        for cell in row["max_len"].values():
            cell["ratio_to_mesh_kernel"] = cell["kernel_ms"] / res["mesh_kernel_ms"]
            cell["ratio_to_mesh_packed"] = cell["packed_ms"] / res["mesh_packed_ms"]
    save()
    print(json.dumps(dict(mesh_kernel_ms=res["mesh_kernel_ms"], vertices=res["vertices"],
                          meshes={k: dict(topology_kernel_ms=row["topology_kernel_ms"], loops=row.get("loops"),
                                          max_len={n: {a: b for a, b in cell.items() if a in ("packed_ms", "kernel_ms", "build_ms", "fill_ms", "counts",
                                                                                             "ratio_to_topology_kernel", "ratio_to_mesh_kernel",
                                                                                             "share_of_boundary_edges_filled")}
                                                   for n, cell in row["max_len"].items()})
                                  for k, row in res["meshes"].items()}), default=float))


if __name__ == "__main__":
    main()
