"""Times the output cloud's oriented normals and de-duplication at DTU scale, next to sn_denoise on the same scene in the
same run, and the numpy restatement (tests/normals_ref.py) on a sub-scene.

    python tools/bench_normals.py [--out profiles/normals/bench_normals.json] [--reps 5] [--radius 2]

Scene: the "dtu" scene of tools/bench_postpass.py (synthetic.sparse_surface: 40 x 40 x 14 overlapping cubes of Dc = 26, ~22k non-empty cubes,
~2.4 M voxels), fixed-threshold masks (pred >= 0.7, votes >= 4), 49 cameras above the sheet, 5 view pairs per cube. Wall times are medians of
--reps after one warm-up:
  *_lists_ms    the list drop-ins (denoising.denoise_crossCubes, normals.estimate_normals, normals.unique_voxels): per-cube lists in and out,
                as tools/bench_postpass.py times the denoise
  *_packed_ms   the Context methods on packed arrays: host arrays in and out (upload and readback included)
  *_kernel_ms   the kernels alone (the context's HIP-event profile)
ratio_*: (normals + unique) / denoise, the aim being <= 2. The restatement runs on the first 6 x 6 x 14 block of cubes and is scaled by the
cube count; the GPU result on that block is compared with it before anything is reported.
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


def _kernel_ms(ctx, fn, reps, prefix):
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(reps):
        fn()
    prof = ctx.profile()
    ctx.profile_enable(False)
    ctx.profile_reset()
    stages = {k: v["ms"] / reps for k, v in prof.items() if k.startswith(prefix)}
    return float(sum(stages.values())), stages


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals", "bench_normals.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--radius", type=int, default=2)
    args = ap.parse_args()
    import normals_ref as ref
    from surfacenet_amd import denoising, normals, runtime, synthetic
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
    res = dict(tool="tools/bench_normals.py", cubes=n, voxels=int(offsets[-1]), masked_voxels=int(mask.sum()), Dc=Dc, cube_D=cube_D, stride_vox=stride,
               radius=args.radius, min_neighbours=6, views_per_cube=2 * N_vp, reps=args.reps)
    try:
        res["box_probe"] = ctx.mfma_probe()
    except Exception as e:             # noqa: BLE001 - the probe only labels the box
        res["box_probe"] = "unavailable: %s" % e

    # the restatement on a sub-scene, and the GPU against it
    keep = np.nonzero(np.all(np.asarray(cube_ijk) < np.asarray((6, 6, 14)), axis=1))[0]
    sub_off, sub_ijk = ref.pack([d["vxl_ijk_list"][i] for i in keep])
    sub = (sub_off, sub_ijk, cube_ijk[keep], np.concatenate([fix[i] for i in keep]), stride, param["xyz"][keep], param["resol"][keep], view_idx[keep], cams)
    t = time.perf_counter()
    r = ref.normals_ref(*sub, radius=args.radius)
    t_n = time.perf_counter() - t
    t = time.perf_counter()
    u = ref.unique_ref(*sub[:5])
    t_u = time.perf_counter() - t
    g_n, g_m = ctx.normals(*sub, radius=args.radius, return_moments=True)
    cmp_ = r["comparable"]
    err = float(np.abs(g_n[cmp_].astype(np.float64) - r["normals"][cmp_]).max())
    equal = bool(np.array_equal(g_m, r["moments"]) and np.array_equal(ctx.unique_voxels(*sub[:5]), u) and err <= 2e-7)
    res["cpu_restatement"] = dict(subsample_cubes=int(keep.size), subsample_voxels=int(sub_off[-1]), normals_s=t_n, unique_s=t_u,
                                  scaled_normals_s=t_n * n / keep.size, scaled_unique_s=t_u * n / keep.size, gpu_equal=equal, max_component_error=err)
    if not equal:
        raise SystemExit("the GPU result differs from the restatement on the sub-scene: %s" % json.dumps(res["cpu_restatement"]))

    run_n = lambda: ctx.normals(offsets, ijk, cube_ijk, mask, stride, param["xyz"], param["resol"], view_idx, cams, radius=args.radius)
    run_u = lambda: ctx.unique_voxels(offsets, ijk, cube_ijk, mask, stride)
    run_d = lambda: ctx.denoise(offsets, ijk, cube_ijk, mask, cube_D, Dc)
    res["denoise_lists_ms"] = _median_time(lambda: denoising.denoise_crossCubes(cube_ijk, d["vxl_ijk_list"], fix, cube_D), args.reps)
    res["normals_lists_ms"] = _median_time(lambda: normals.estimate_normals(cube_ijk, d["vxl_ijk_list"], fix, param, viewPair, cams, stride, radius=args.radius),
                                           args.reps)
    res["unique_lists_ms"] = _median_time(lambda: normals.unique_voxels(cube_ijk, d["vxl_ijk_list"], fix, stride), args.reps)
    res["denoise_packed_ms"] = _median_time(run_d, args.reps)
    res["normals_packed_ms"] = _median_time(run_n, args.reps)
    res["unique_packed_ms"] = _median_time(run_u, args.reps)
    res["denoise_kernel_ms"], res["denoise_stages_ms"] = _kernel_ms(ctx, run_d, args.reps, "cc_")
    res["normals_kernel_ms"], res["normals_stages_ms"] = _kernel_ms(ctx, run_n, args.reps, "nm_")
    res["unique_kernel_ms"], res["unique_stages_ms"] = _kernel_ms(ctx, run_u, args.reps, "nm_")
    for k in ("lists", "packed", "kernel"):
        res["ratio_" + k] = (res["normals_%s_ms" % k] + res["unique_%s_ms" % k]) / res["denoise_%s_ms" % k]
    keep_mask = run_u()
    nrm = run_n()
    res["distinct_cells"] = int(keep_mask.sum())
    res["duplicate_fraction"] = 1.0 - res["distinct_cells"] / max(res["masked_voxels"], 1)
    res["voxels_with_normal"] = int(np.any(nrm != 0, axis=1).sum())
    res["speedup_normals"] = res["cpu_restatement"]["scaled_normals_s"] / (res["normals_packed_ms"] / 1e3)
    res["speedup_unique"] = res["cpu_restatement"]["scaled_unique_s"] / (res["unique_packed_ms"] / 1e3)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, default=float)
    print(json.dumps({k: res[k] for k in res if k.endswith("_ms") and not k.endswith("stages_ms") or k.startswith("ratio")}))


if __name__ == "__main__":
    main()
