"""Times the connected components of the output cloud at DTU scale, next to sn_unique_voxels and sn_denoise on the
same scene in the same run, and the numpy restatement (tests/components_ref.py) on a sub-scene.

    python tools/bench_components.py [--out profiles/components/bench_components.json] [--reps 5] [--connectivity 26]

Scene: the "dtu" scene of tools/bench_postpass.py (synthetic.sparse_surface: 40 x 40 x 14 overlapping cubes of Dc = 26, ~22k non-empty cubes,
~2.4 M voxels), fixed-threshold masks (pred >= 0.7, votes >= 4). The tool runs two steps, each ONCE, each a child process under its own time
limit, the second only after the first has succeeded:
  check   the GPU result on the first 6 x 6 x 14 block of cubes (504) equals the restatement exactly, at the three connectivities; the
          restatement's time there, scaled by the cube count
  time    medians of --reps after one warm-up:
            *_lists_ms    the list drop-ins (components.remove_floaters, normals.unique_voxels, denoising.denoise_crossCubes)
            *_packed_ms   the Context methods on packed host arrays (upload and readback included)
            *_kernel_ms   the kernels alone, per stage (the context's HIP-event profile)
          ratio_to_unique_*, ratio_to_denoise_*: components / the yardstick. sn_unique_voxels is the same table build plus one probe per
          voxel; sn_denoise is the project's usual yardstick of a post-pass stage. Also the size histogram of the scene's components and the
          voxels that min_component = 10 / 100 / 1000 removes.
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

STEP_LIMIT_S = dict(check=240, time=420)


def _median_time(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return 1e3 * float(np.median(ts))


def _kernel_ms(ctx, fn, reps, prefixes):
    fn()
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(reps):
        fn()
    prof = ctx.profile()
    ctx.profile_enable(False)
    ctx.profile_reset()
    stages = {k: v["ms"] / reps for k, v in prof.items() if k.startswith(prefixes)}
    return float(sum(stages.values())), stages


def _scene():
    from surfacenet_amd import denoising, synthetic
    Dc = 26
    d = synthetic.sparse_surface((40, 40, 14), Dc, speck_rate=0.0005, seed=1, thickness=1, amplitude=60.0)
    fix = [(p >= 0.7) & (v >= 4) for p, v in zip(d["prediction_list"], d["rayPooling_votes_list"])]
    offsets, ijk, _ = denoising.pack_lists(d["vxl_ijk_list"])
    return d, fix, offsets, ijk, np.concatenate(fix)


def step_check(args):
    import components_ref as ref
    import normals_ref
    from surfacenet_amd import runtime
    ctx = runtime.any_context()
    d, fix, offsets, ijk, mask = _scene()
    cube_ijk, n = d["cube_ijk_np"], len(d["vxl_ijk_list"])
    keep = np.nonzero(np.all(np.asarray(cube_ijk) < np.asarray((6, 6, 14)), axis=1))[0]
    sub_off, sub_ijk = normals_ref.pack([d["vxl_ijk_list"][i] for i in keep])
    sub = (sub_off, sub_ijk, cube_ijk[keep], np.concatenate([fix[i] for i in keep]), 13)
    res = dict(subsample_cubes=int(keep.size), subsample_voxels=int(sub_off[-1]), components={})
    for c in (6, 18, 26):
        t = time.perf_counter()
        want = ref.components_ref(*sub, connectivity=c, min_cells=10)
        dt = time.perf_counter() - t
        ref.compare(ctx.components(*sub, connectivity=c, min_cells=10), want)      # raises: the step fails, nothing is timed
        res["components"][str(c)] = want[3]
        if c == args.connectivity:
            res.update(restatement_s=dt, scaled_restatement_s=dt * n / keep.size)
    res["gpu_equal"] = True
    return res


def step_time(args):
    from surfacenet_amd import components, denoising, normals, runtime
    ctx = runtime.any_context()
    d, fix, offsets, ijk, mask = _scene()
    cube_ijk, n = d["cube_ijk_np"], len(d["vxl_ijk_list"])
    cube_D, Dc, stride, conn = 32, 26, 13, args.connectivity
    res = dict(cubes=n, voxels=int(offsets[-1]), masked_voxels=int(mask.sum()), Dc=Dc, cube_D=cube_D, stride_vox=stride, connectivity=conn, reps=args.reps)
    try:
        res["box_probe"] = ctx.mfma_probe()
    except Exception as e:             # noqa: BLE001 - the probe only labels the box
        res["box_probe"] = "unavailable: %s" % e
    run_c = lambda: ctx.components(offsets, ijk, cube_ijk, mask, stride, connectivity=conn, min_cells=10)
    run_u = lambda: ctx.unique_voxels(offsets, ijk, cube_ijk, mask, stride)
    run_d = lambda: ctx.denoise(offsets, ijk, cube_ijk, mask, cube_D, Dc)
    res["components_lists_ms"] = _median_time(lambda: components.remove_floaters(cube_ijk, d["vxl_ijk_list"], fix, stride, min_cells=10, connectivity=conn),
                                              args.reps)
    res["unique_lists_ms"] = _median_time(lambda: normals.unique_voxels(cube_ijk, d["vxl_ijk_list"], fix, stride), args.reps)
    res["denoise_lists_ms"] = _median_time(lambda: denoising.denoise_crossCubes(cube_ijk, d["vxl_ijk_list"], fix, cube_D), args.reps)
    res["components_packed_ms"] = _median_time(run_c, args.reps)
    res["unique_packed_ms"] = _median_time(run_u, args.reps)
    res["denoise_packed_ms"] = _median_time(run_d, args.reps)
    res["components_kernel_ms"], res["components_stages_ms"] = _kernel_ms(ctx, run_c, args.reps, ("cp_",))
    res["unique_kernel_ms"], res["unique_stages_ms"] = _kernel_ms(ctx, run_u, args.reps, ("nm_",))
    res["denoise_kernel_ms"], res["denoise_stages_ms"] = _kernel_ms(ctx, run_d, args.reps, ("cc_",))
    for k in ("lists", "packed", "kernel"):
        res["ratio_to_unique_" + k] = res["components_%s_ms" % k] / res["unique_%s_ms" % k]
        res["ratio_to_denoise_" + k] = res["components_%s_ms" % k] / res["denoise_%s_ms" % k]
    res["kernel_ms_by_connectivity"] = {str(c): _kernel_ms(ctx, lambda: ctx.components(offsets, ijk, cube_ijk, mask, stride, connectivity=c), args.reps, ("cp_",))[0]
                                        for c in (6, 18, 26)}
    label, cells, keep, C = run_c()
    sizes = np.zeros((C,), np.int64)
    sizes[label[label >= 0]] = cells[label >= 0]
    edges = [1, 2, 3, 5, 10, 100, 1000, 10000, 100000, 1 << 31]
    res["n_components"] = C
    res["distinct_cells"] = int(sizes.sum())
    res["largest_components"] = np.sort(sizes)[::-1][:5].tolist()
    res["size_histogram"] = {"%d..%d" % (a, b - 1) if b < (1 << 31) else "%d.." % a: int(((sizes >= a) & (sizes < b)).sum()) for a, b in zip(edges[:-1], edges[1:])}
    res["removed_voxels"] = {str(k): int((mask & (cells < k)).sum()) for k in (10, 100, 1000)}
    res["removed_cells"] = {str(k): int(sizes[sizes < k].sum()) for k in (10, 100, 1000)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components", "bench_components.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--connectivity", type=int, default=26, choices=(6, 18, 26))
    ap.add_argument("--step", choices=("check", "time"), help="(internal) run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        print("STEP_RESULT " + json.dumps(dict(check=step_check, time=step_time)[args.step](args), default=float))
        return
    res = dict(tool="tools/bench_components.py")
    for step in ("check", "time"):                   # each once, under its own limit; a failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps), "--connectivity", str(args.connectivity)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT_S[step])
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("STEP_RESULT ")]
        if p.returncode != 0 or not line:
            raise SystemExit("step %s failed with status %d; nothing further was run" % (step, p.returncode))
        part = json.loads(line[-1][len("STEP_RESULT "):])
        if step == "check":
            res["cpu_restatement"] = part
        else:
            res.update(part)
    res["speedup_packed"] = res["cpu_restatement"]["scaled_restatement_s"] / (res["components_packed_ms"] / 1e3)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, default=float)
    print(json.dumps({k: res[k] for k in res if k.endswith("_ms") and not k.endswith("stages_ms") or k.startswith("ratio")}))


if __name__ == "__main__":
    main()
