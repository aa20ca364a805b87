"""Times the cross-cube post-pass on the GPU at DTU scale and sets it against the CPU restatement (tests/postpass_ref.py) on a subsample.

    python tools/bench_postpass.py [--out profiles/postpass/bench_postpass.json] [--iters 8] [--reps 3]

Scenes (surfacenet_amd.synthetic.sparse_surface): "dtu" - 40 x 40 x 14 overlapping cubes of Dc = 26 (s = 32) around a wavy surface,
~22k non-empty cubes and ~2.4 M voxels, the size of DTU scan9's full bounding box (23,347 cubes, 2.2 M voxels); "thick" - the same
lattice with a 12-voxel-thick surface (large, overflowing float16 costs). Per scene, wall times of the host-array entry points (upload and
readback included; median of --reps after one warm-up):
  denoise_ms          denoise_crossCubes with D_cube = cube_D (32), the fixed-threshold pass of main_reconstruct.py:175
  adapt_memory_ms     --iters adapthresh iterations in memory (adapthresh_lists: every iteration's masks and denoised masks come back)
  adapt_files_s       --iters iterations through the drop-in adapthresh.adapthresh: npz in, initialization.ply + iter{k}.ply out
and the CPU restatement's time for a subsample of cubes, scaled to the whole scene by the cube count (an estimate of the Python cost).
"""
import argparse
import json
import os
import sys
import tempfile
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
    return float(np.median(ts))


def bench_scene(name, d, iters, reps, cube_D=32, Dc=26, sub=(6, 6, 14)):
    from surfacenet_amd import adapthresh, denoising, sparseCubes
    import postpass_ref
    n = len(d["vxl_ijk_list"])
    T = int(sum(len(a) for a in d["vxl_ijk_list"]))
    fix = [(p >= 0.7) & (v >= 4) for p, v in zip(d["prediction_list"], d["rayPooling_votes_list"])]
    res = dict(cubes=n, nonempty_cubes=int(sum(len(a) > 0 for a in d["vxl_ijk_list"])), voxels=T, Dc=Dc, cube_D=cube_D, iters=iters)
    res["denoise_ms"] = 1e3 * _median_time(lambda: denoising.denoise_crossCubes(d["cube_ijk_np"], d["vxl_ijk_list"], fix, cube_D), reps)
    args = (d["prediction_list"], d["vxl_ijk_list"], d["rayPooling_votes_list"], d["cube_ijk_np"], iters, Dc, 0.5, 0.9, 4, 6)
    res["adapt_memory_ms"] = 1e3 * _median_time(lambda: adapthresh.adapthresh_lists(*args), reps)
    r = adapthresh.adapthresh_lists(*args)
    res["choices_per_iteration"] = [np.bincount(c[c >= 0], minlength=3).tolist() for c in r["choice"]]
    with tempfile.TemporaryDirectory() as tmp:
        npz = os.path.join(tmp, "model.npz")
        sparseCubes.save_sparseCubes(npz, d["prediction_list"], d["rgb_list"], d["vxl_ijk_list"], d["rayPooling_votes_list"], d["cube_ijk_np"],
                                     d["param_np"], d["viewPair_np"])
        t = time.perf_counter()
        adapthresh.adapthresh(tmp, iters, Dc, 0.5, 0.5, 0.9, 4, 6, 0.8, npz, RGB_visual_ply=False)
        res["adapt_files_s"] = time.perf_counter() - t
        ply_bytes = sum(os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(tmp) for f in fs if f.endswith(".ply"))
        res["ply_mb_written"] = ply_bytes / 1e6
    # CPU restatement on a sub-lattice of the cubes (the first sub[0] x sub[1] x sub[2] block), scaled by the cube count
    lat = np.asarray(d["cube_ijk_np"])
    keep = np.nonzero(np.all(lat < np.asarray(sub), axis=1))[0]
    pick = lambda key: [d[key][i] for i in keep]
    t = time.perf_counter()
    postpass_ref.denoise_ref(lat[keep], pick("vxl_ijk_list"), [fix[i] for i in keep], cube_D, Dc=Dc)
    t_dn = time.perf_counter() - t
    t = time.perf_counter()
    postpass_ref.adapthresh_ref(pick("prediction_list"), pick("vxl_ijk_list"), pick("rayPooling_votes_list"), lat[keep], 1, Dc, 0.5, 0.9, 4, 6, Dc=Dc)
    t_it = time.perf_counter() - t
    res["cpu_restatement"] = dict(subsample_cubes=int(keep.size), denoise_s=t_dn, one_iteration_s=t_it,
                                  scaled_denoise_s=t_dn * n / keep.size, scaled_adapt_s=t_dn * n / keep.size + iters * t_it * n / keep.size)
    res["speedup_denoise"] = res["cpu_restatement"]["scaled_denoise_s"] / (res["denoise_ms"] / 1e3)
    res["speedup_adapt_memory"] = res["cpu_restatement"]["scaled_adapt_s"] / (res["adapt_memory_ms"] / 1e3)
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "postpass", "bench_postpass.json"))
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from surfacenet_amd import runtime, synthetic
    out = dict(tool="tools/bench_postpass.py", iters=args.iters, scenes={})
    ctx = runtime.any_context()
    try:
        tf = ctx.mfma_probe() if hasattr(ctx, "mfma_probe") else None
        out["box_probe"] = tf
    except Exception as e:             # noqa: BLE001 - the probe only labels the box
        out["box_probe"] = "unavailable: %s" % e
    scenes = dict(dtu=dict(thickness=1, amplitude=60.0), thick=dict(thickness=12, amplitude=60.0))
    for name, kw in scenes.items():
        d = synthetic.sparse_surface((40, 40, 14), 26, speck_rate=0.0005, seed=1, **kw)
        out["scenes"][name] = bench_scene(name, d, args.iters, args.reps)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, default=float)
    print(json.dumps({k: {kk: v[kk] for kk in ("cubes", "voxels", "denoise_ms", "adapt_memory_ms", "adapt_files_s")} for k, v in out["scenes"].items()}))


if __name__ == "__main__":
    main()
