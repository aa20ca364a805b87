"""Times the mesh simplifier at DTU scale, next to sn_mesh and sn_mesh_sample on the same scene in the same run, and
records what simplification costs in accuracy and completeness on that scene.

    python tools/bench_meshsimplify.py [--out profiles/meshsimplify/bench_meshsimplify.json] [--reps 5] [--dst 0.2] [--no-score] [--no-ab]

Scene: the "dtu" scene of tools/bench_postpass.py as tools/bench_mesh.py sets it up (synthetic.sparse_surface: 40 x 40 x 14 overlapping cubes of
Dc = 26, fixed-threshold masks, normals from sn_normals), meshed by sn_mesh and triangulated. For cell = 2, 4, 8 and both placements the GPU
result is compared with the restatement (tests/meshsimplify_ref.py) on the whole mesh before anything is reported. Times are medians of --reps
after one warm-up:
  packed_ms / device_ms   Context.mesh_simplify on host arrays (upload, kernels, readback) / with the mesh staged in device memory by the caller
  kernel_ms, stages_ms    the kernels alone (the context's HIP-event profile) and their split
  mesh_*, sample_*        sn_mesh and sn_mesh_sample the same ways in the same run
  cluster_no_agg_ms       msim_cluster with one set of atomics per vertex instead of one per run of a wave (the test-only twin library with
                          SN_MSIM_NO_AGG set, in a child process), next to the product's msim_cluster
  score                   evaluation.mesh_compare of the full mesh and of the simplified meshes (cell 2 and 4, mean placement) against the samples
                          of the full mesh, everything in the mask and above the plane: [mean, median] accuracy and completeness in mm
No time is aimed at and no score is asserted: the numbers are written down.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_mesh import _kernel_ms, _median_time  # noqa: E402  (tools/ is on the path when this file is run as a script)

CELLS = (2, 4, 8)


def _scene(ctx):
    """-> (run_mesh, its result, origin, resol, the scene's counts)."""
    from surfacenet_amd import denoising, mesh, synthetic
    Dc, stride, N_vp, V = 26, 13, 5, 49
    d = synthetic.sparse_surface((40, 40, 14), Dc, speck_rate=0.0005, seed=1, thickness=1, amplitude=60.0)
    n = len(d["vxl_ijk_list"])
    fix = [(p >= 0.7) & (v >= 4) for p, v in zip(d["prediction_list"], d["rayPooling_votes_list"])]
    rs = np.random.RandomState(3)
    cams = np.stack([rs.uniform(-100, 300, V), rs.uniform(-100, 300, V), rs.uniform(500, 700, V)], axis=1)
    view_idx = rs.randint(0, V, (n, N_vp, 2)).astype(np.uint16).reshape(n, -1).astype(np.int32)
    param, cube_ijk = d["param_np"], d["cube_ijk_np"]
    offsets, ijk, _ = denoising.pack_lists(d["vxl_ijk_list"])
    mask = np.concatenate(fix)
    origin, resol = mesh.lattice_origin(cube_ijk, param, stride)
    normals = ctx.normals(offsets, ijk, cube_ijk, mask, stride, param["xyz"], param["resol"], view_idx, cams, radius=2)
    run_m = lambda: ctx.mesh(offsets, ijk, cube_ijk, mask, stride, normals, radius=2, reach=0, origin=origin, resol=resol)
    return run_m, run_m(), origin, resol, dict(cubes=n, voxels=int(offsets[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshsimplify", "bench_meshsimplify.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dst", type=float, default=0.2)
    ap.add_argument("--no-score", action="store_true")
    ap.add_argument("--no-ab", action="store_true")
    ap.add_argument("--cluster-only", action="store_true", help="print the msim_cluster time per cell as one JSON line and exit (the A/B child)")
    args = ap.parse_args()
    import meshsimplify_ref
    from surfacenet_amd import evaluation, mesh, runtime
    ctx = runtime.any_context()
    run_m, m, origin, resol, counts = _scene(ctx)
    lat = np.ascontiguousarray(m["verts_lattice"], dtype=np.float64)
    tris = np.ascontiguousarray(mesh.triangulate(m["quads"]), dtype=np.int32)
    run = lambda k, p=0, **kw: ctx.mesh_simplify(lat, tris, k, p, origin=origin, resol=resol, **kw)
    if args.cluster_only:
        print(json.dumps({str(k): _kernel_ms(ctx, lambda: run(k), args.reps, ("msim_cluster",))[0] for k in CELLS}))
        return
    res = dict(tool="tools/bench_meshsimplify.py", resol=resol, dst=args.dst, reps=args.reps, vertices=int(lat.shape[0]),
               triangles=int(tris.shape[0]), cells={}, **counts)
    try:
        res["box_probe"] = ctx.mfma_probe()
    except Exception as e:             # noqa: BLE001 - the probe only labels the box
        res["box_probe"] = "unavailable: %s" % e

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, default=float)

    simplified = {}
    for k in CELLS:
        row = res["cells"][str(k)] = {}
        for p, word in ((0, "mean"), (1, "member")):
            t = time.perf_counter()
            want = meshsimplify_ref.simplify(lat, tris, k, p, origin, resol)
            row["restatement_%s_ms" % word] = 1e3 * (time.perf_counter() - t)
            got = run(k, p)
            equal = all(np.array_equal(got[a], want[b]) for a, b in (("verts_lattice", "vert_lattice"), ("verts_mm", "vertices"), ("vert_rep", "vert_rep"),
                                                                     ("vert_count", "vert_count"), ("faces", "faces"), ("face_src", "face_src"),
                                                                     ("vert_cluster", "vert_cluster")))
            if not equal:
                raise SystemExit("cell %d, placement %s: the GPU result differs from the restatement" % (k, word))
            if p == 0:
                simplified[k] = (got["verts_mm"], got["faces"])
                C, G = int(got["vert_rep"].shape[0]), int(got["faces"].shape[0])
                row.update(C=C, G=G, clusters=want["clusters"], collapsed=want["collapsed"], duplicates=want["duplicates"], largest_cluster=want["largest"],
                           dropped_vertices=int((got["vert_cluster"] < 0).sum()), max_move_cells=meshsimplify_ref.max_move(lat, want))
            del got, want
        row["gpu_equal"] = True
        cap = (row["C"], row["G"])                               # the exact caps: no retry inside the timing
        row["packed_ms"] = _median_time(lambda: run(k, cap=cap), args.reps)
        row["device_ms"] = _median_time(lambda: run(k, cap=cap, device=True), args.reps)
        row["kernel_ms"], row["stages_ms"] = _kernel_ms(ctx, lambda: run(k, cap=cap), args.reps, ("msim_",))
        row["kernel_member_ms"] = _kernel_ms(ctx, lambda: run(k, 1, cap=cap), args.reps, ("msim_",))[0]
    verts_mm = np.ascontiguousarray(m["verts_mm"], dtype=np.float64)
    M = int(ctx.mesh_sample(verts_mm, tris, args.dst)[0].shape[0])
    run_s = lambda: ctx.mesh_sample(verts_mm, tris, args.dst, cap=M)
    res["samples"] = M
    res["mesh_packed_ms"] = _median_time(run_m, args.reps)
    res["sample_packed_ms"] = _median_time(run_s, args.reps)
    res["mesh_kernel_ms"], res["mesh_stages_ms"] = _kernel_ms(ctx, run_m, args.reps, ("ms_", "pc_sort"))
    res["sample_kernel_ms"], res["sample_stages_ms"] = _kernel_ms(ctx, run_s, args.reps, ("msmp_",))
    for k in CELLS:
        row = res["cells"][str(k)]
        row["ratio_to_mesh_kernel"] = row["kernel_ms"] / res["mesh_kernel_ms"]
        row["ratio_to_mesh_packed"] = row["packed_ms"] / res["mesh_packed_ms"]
    save()
    if not args.no_ab:
        dbg = os.path.join(ROOT, "surfacenet_amd", "libsurfacenet_hip_dbg.so")
        env = dict(os.environ, SURFACENET_HIP_LIB=dbg, SN_MSIM_NO_AGG="1")
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--cluster-only", "--reps", str(args.reps)], env=env, capture_output=True,
                             text=True, timeout=300)
        if out.returncode != 0:
            res["cluster_no_agg_ms"] = "failed: %s" % out.stderr[-300:]
        else:
            res["cluster_no_agg_ms"] = json.loads(out.stdout.strip().splitlines()[-1])
        res["cluster_agg_ms"] = {str(k): res["cells"][str(k)]["stages_ms"].get("msim_cluster") for k in CELLS}
        save()
    if not args.no_score:
        # the samples of the full mesh stand for the ground truth; one mask voxel holds everything, the plane lies below everything
        t = time.perf_counter()
        stl, _ = mesh.sample_surface(m["verts_mm"], tris, args.dst)
        lo, hi = stl.min(axis=0) - 1.0, stl.max(axis=0) + 1.0
        obs, BB, Res, plane = np.ones((1, 1, 1), np.uint8), np.stack([lo, hi]), 1e9, np.asarray([0.0, 0.0, 1.0, 1e6])
        res["score"] = dict(columns=["accuracy_mean", "accuracy_median", "completeness_mean", "completeness_median"], reference_samples=int(stl.shape[0]))
        for name, (v, f) in [("full", (m["verts_mm"], tris))] + [("cell_%d" % k, simplified[k]) for k in (2, 4)]:
            base = evaluation.mesh_compare(v, f, stl, obs, BB, Res, plane, dst=args.dst)
            res["score"][name] = dict(mm=evaluation.eval_acc_compl(base).tolist(), n_samples=base["n_samples"], n_faces=base["n_faces"],
                                      reduced_points=int(base["Qdata"].shape[0]))
            assert base["DataInMask"].all() and base["StlAbovePlane"].all()
        res["score"]["wall_s"] = time.perf_counter() - t
        save()
    print(json.dumps(dict(mesh_kernel_ms=res["mesh_kernel_ms"], sample_kernel_ms=res["sample_kernel_ms"],
                          cells={k: {a: b for a, b in row.items() if a in ("C", "G", "packed_ms", "device_ms", "kernel_ms", "ratio_to_mesh_kernel")}
                                 for k, row in res["cells"].items()},
                          cluster_no_agg_ms=res.get("cluster_no_agg_ms"), score={k: v["mm"] for k, v in res.get("score", {}).items() if isinstance(v, dict)}),
                     default=float))


if __name__ == "__main__":
    main()
