"""Times the surface-nets mesher at DTU scale, next to sn_normals and sn_denoise on the same scene in the same run.

    python tools/bench_mesh.py [--out profiles/mesh/bench_mesh.json] [--reps 5] [--radius 2] [--reach 0]

Scene: the "dtu" scene of tools/bench_postpass.py (synthetic.sparse_surface: 40 x 40 x 14 overlapping cubes of Dc = 26, ~22k non-empty cubes,
~2.4 M voxels), fixed-threshold masks (pred >= 0.7, votes >= 4), 49 cameras above the sheet, 5 view pairs per cube; the mesher's input normals are
sn_normals' own. Wall times are medians of --reps after one warm-up:
  *_packed_ms   the Context methods on packed arrays: host arrays in and out (upload and readback included)
  *_kernel_ms   the kernels alone (the context's HIP-event profile), with the per-stage split in *_stages_ms
  mesh_lists_ms mesh.extract_mesh: per-cube lists in, arrays out
No time is aimed at: ratio_* = mesh / normals on this box is what gets written down. The restatement (tests/mesh_ref.py) runs on the first
6 x 6 x 14 block of cubes; the GPU result on that block is compared with it before anything is reported.
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


def _median_time(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return 1e3 * float(np.median(ts))


def _kernel_ms(ctx, fn, reps, prefixes):
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(reps):
        fn()
    prof = ctx.profile()
    ctx.profile_enable(False)
    ctx.profile_reset()
    stages = {k: v["ms"] / reps for k, v in prof.items() if k.startswith(prefixes)}
    return float(sum(stages.values())), stages


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh", "bench_mesh.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--reach", type=int, default=0)
    args = ap.parse_args()
    import mesh_ref
    import normals_ref as ref
    from surfacenet_amd import denoising, mesh, runtime, synthetic
    ctx = runtime.any_context()
    cube_D, Dc, stride, N_vp, V = 32, 26, 13, 5, 49
    d = synthetic.sparse_surface((40, 40, 14), Dc, speck_rate=0.0005, seed=1, thickness=1, amplitude=60.0)
    n = len(d["vxl_ijk_list"])
    fix = [(p >= 0.7) & (v >= 4) for p, v in zip(d["prediction_list"], d["rayPooling_votes_list"])]
    rs = np.random.RandomState(3)
    cams = np.stack([rs.uniform(-100, 300, V), rs.uniform(-100, 300, V), rs.uniform(500, 700, V)], axis=1)
    viewPair = rs.randint(0, V, (n, N_vp, 2)).astype(np.uint16)
    param, cube_ijk = d["param_np"], d["cube_ijk_np"]
    offsets, ijk, _ = denoising.pack_lists(d["vxl_ijk_list"])
    mask = np.concatenate(fix)
    view_idx = viewPair.reshape(n, -1).astype(np.int32)
    origin, resol = mesh.lattice_origin(cube_ijk, param, stride)
    res = dict(tool="tools/bench_mesh.py", cubes=n, voxels=int(offsets[-1]), masked_voxels=int(mask.sum()), Dc=Dc, cube_D=cube_D, stride_vox=stride,
               radius=args.radius, reach=args.reach, reps=args.reps)
    try:
        res["box_probe"] = ctx.mfma_probe()
    except Exception as e:             # noqa: BLE001 - the probe only labels the box
        res["box_probe"] = "unavailable: %s" % e
    run_n = lambda: ctx.normals(offsets, ijk, cube_ijk, mask, stride, param["xyz"], param["resol"], view_idx, cams, radius=2)
    normals = run_n()
    run_m = lambda: ctx.mesh(offsets, ijk, cube_ijk, mask, stride, normals, radius=args.radius, reach=args.reach, origin=origin, resol=resol)
    run_d = lambda: ctx.denoise(offsets, ijk, cube_ijk, mask, cube_D, Dc)

    # the restatement on a sub-scene, and the GPU against it
    keep = np.nonzero(np.all(np.asarray(cube_ijk) < np.asarray((6, 6, 14)), axis=1))[0]
    sub_off, sub_ijk = ref.pack([d["vxl_ijk_list"][i] for i in keep])
    sub_nrm = np.concatenate([normals[offsets[i]:offsets[i + 1]] for i in keep])
    sub = (sub_off, sub_ijk, cube_ijk[keep], np.concatenate([fix[i] for i in keep]), stride, sub_nrm)
    t = time.perf_counter()
    r = mesh_ref.mesh_ref(*sub, radius=args.radius, reach=args.reach, origin=origin, resol=resol)
    t_ref = time.perf_counter() - t
    g = ctx.mesh(*sub, radius=args.radius, reach=args.reach, origin=origin, resol=resol)
    equal = bool(np.array_equal(g["quads"], r["quads"]) and np.array_equal(g["vert_cell"], r["vert_cell"]) and np.array_equal(g["vert_src"], r["vert_src"])
                 and np.abs(g["verts_lattice"] - r["vert_lattice"]).max() <= 1e-9)
    res["cpu_restatement"] = dict(subsample_cubes=int(keep.size), subsample_voxels=int(sub_off[-1]), mesh_s=t_ref, scaled_mesh_s=t_ref * n / keep.size,
                                  gpu_equal=equal, quads=int(r["quads"].shape[0]), vertices=int(r["vert_cell"].shape[0]))
    if not equal:
        raise SystemExit("the GPU result differs from the restatement on the sub-scene: %s" % json.dumps(res["cpu_restatement"]))

    m = run_m()
    res.update(vertices=int(m["verts_mm"].shape[0]), quads=int(m["quads"].shape[0]), voxels_with_normal=int(np.any(normals != 0, axis=1).sum()))
    nl = [normals[offsets[i]:offsets[i + 1]] for i in range(n)]
    res["mesh_lists_ms"] = _median_time(lambda: mesh.extract_mesh(cube_ijk, d["vxl_ijk_list"], fix, nl, param, stride, args.radius, args.reach), args.reps)
    res["mesh_packed_ms"] = _median_time(run_m, args.reps)
    res["normals_packed_ms"] = _median_time(run_n, args.reps)
    res["denoise_packed_ms"] = _median_time(run_d, args.reps)
    res["mesh_kernel_ms"], res["mesh_stages_ms"] = _kernel_ms(ctx, run_m, args.reps, ("ms_", "pc_sort"))
    res["normals_kernel_ms"], res["normals_stages_ms"] = _kernel_ms(ctx, run_n, args.reps, ("nm_",))
    res["denoise_kernel_ms"], res["denoise_stages_ms"] = _kernel_ms(ctx, run_d, args.reps, ("cc_",))
    for k in ("packed", "kernel"):
        res["ratio_mesh_to_normals_" + k] = res["mesh_%s_ms" % k] / res["normals_%s_ms" % k]
        res["ratio_mesh_to_denoise_" + k] = res["mesh_%s_ms" % k] / res["denoise_%s_ms" % k]
    res["speedup_over_restatement"] = res["cpu_restatement"]["scaled_mesh_s"] / (res["mesh_packed_ms"] / 1e3)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, default=float)
    print(json.dumps({k: res[k] for k in res if k.endswith("_ms") and not k.endswith("stages_ms") or k.startswith("ratio") or k in ("vertices", "quads")}))


if __name__ == "__main__":
    main()
