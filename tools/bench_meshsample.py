"""Times the mesh sampler at DTU scale, next to sn_mesh on the same scene in the same run and to the numpy restatement.

    python tools/bench_meshsample.py [--out profiles/meshsample/bench_meshsample.json] [--reps 5] [--dst 0.2]

Scene: the "dtu" scene of tools/bench_postpass.py as tools/bench_mesh.py sets it up (synthetic.sparse_surface: 40 x 40 x 14 overlapping cubes of
Dc = 26, fixed-threshold masks, normals from sn_normals), meshed by sn_mesh, triangulated, sampled at --dst mm. The GPU samples are compared with
the restatement (tests/meshsample_ref.py) on the whole mesh before anything is reported. Wall times are medians of --reps after one warm-up:
  sample_packed_ms   Context.mesh_sample on host arrays: upload, kernels, readback of 28 B per sample
  sample_kernel_ms   the kernels alone (the context's HIP-event profile), with the per-stage split in sample_stages_ms
  mesh_*_ms          sn_mesh the same two ways, restatement_ms the numpy restatement on the host
No time is aimed at: samples per second and the written GB/s of msmp_emit (28 B per sample) are what gets written down.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshsample", "bench_meshsample.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dst", type=float, default=0.2)
    args = ap.parse_args()
    import meshsample_ref
    from surfacenet_amd import denoising, mesh, runtime, synthetic
    ctx = runtime.any_context()
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
    m = run_m()
    verts = np.ascontiguousarray(m["verts_mm"], dtype=np.float64)
    tris = np.ascontiguousarray(mesh.triangulate(m["quads"]), dtype=np.int32)
    res = dict(tool="tools/bench_meshsample.py", cubes=n, voxels=int(offsets[-1]), resol=resol, dst=args.dst, reps=args.reps,
               vertices=int(verts.shape[0]), quads=int(m["quads"].shape[0]), triangles=int(tris.shape[0]))
    try:
        res["box_probe"] = ctx.mfma_probe()
    except Exception as e:             # noqa: BLE001 - the probe only labels the box
        res["box_probe"] = "unavailable: %s" % e

    t = time.perf_counter()
    want = meshsample_ref.sample(verts, tris, args.dst)
    res["restatement_ms"] = 1e3 * (time.perf_counter() - t)
    got = ctx.mesh_sample(verts, tris, args.dst)
    M = int(want[0].shape[0])
    res.update(samples=M, samples_per_triangle=M / max(tris.shape[0], 1), gpu_equal=bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])))
    if not res["gpu_equal"]:
        raise SystemExit("the GPU samples differ from the restatement: %s" % json.dumps(res, default=float))
    del got, want

    run_s = lambda: ctx.mesh_sample(verts, tris, args.dst, cap=M)      # the exact cap: no retry inside the timing
    res["sample_packed_ms"] = _median_time(run_s, args.reps)
    res["sample_device_ms"] = _median_time(lambda: ctx.mesh_sample(verts, tris, args.dst, cap=M, device=True), args.reps)
    res["mesh_packed_ms"] = _median_time(run_m, args.reps)
    res["sample_kernel_ms"], res["sample_stages_ms"] = _kernel_ms(ctx, run_s, args.reps, ("msmp_",))
    res["mesh_kernel_ms"], res["mesh_stages_ms"] = _kernel_ms(ctx, run_m, args.reps, ("ms_", "pc_sort"))
    emit = res["sample_stages_ms"].get("msmp_emit", 0.0)
    res["emit_written_GBps"] = 28.0 * M / (emit * 1e-3) / 1e9 if emit > 0 else None
    res["samples_per_s_kernels"] = M / (res["sample_kernel_ms"] * 1e-3)
    res["samples_per_s_packed"] = M / (res["sample_packed_ms"] * 1e-3)
    res["ratio_sample_to_mesh_kernel"] = res["sample_kernel_ms"] / res["mesh_kernel_ms"]
    res["ratio_sample_to_mesh_packed"] = res["sample_packed_ms"] / res["mesh_packed_ms"]
    res["speedup_over_restatement_packed"] = res["restatement_ms"] / res["sample_packed_ms"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, default=float)
    print(json.dumps({k: res[k] for k in res if k.endswith("_ms") and not k.endswith("stages_ms") or k.startswith(("ratio", "samples", "emit", "speedup"))
                      or k in ("triangles",)}, default=float))


if __name__ == "__main__":
    main()
