"""Times the point-seeded cube list (surfacenet_amd.scene.quantizePts2Cubes, GPU) beside its numpy restatement (tests/ptcubes_ref.py) on the
same box.

    python tools/bench_ptcubes.py [--out profiles/ptcubes/bench_ptcubes.json] [--reps 5] [--sizes 300000 3000000 10000000]

Input (seeded): tests/ptcubes_ref.py::wavy_cloud - a noisy wavy sheet across DTU scan9's bounding box, in raster order - with scan9's
parameters (resol float32 0.4, cube 32 / 26, overlap 1/2, its BB). Per size and point dtype: the median wall time of the GPU call from host
arrays (upload and readback included), of the same call on points already in HBM, the kernels' stage times (HIP events), the restatement's
time (one run; numpy, single thread), the cube count and, for comparison, the count of the full-box grid over the same BB. The two results
are compared (equal: true) before anything is reported. Prints one JSON line.
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


def median_time(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ptcubes", "bench_ptcubes.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[300000, 3000000, 10000000])
    a = ap.parse_args()
    import ptcubes_ref as ref
    from surfacenet_amd import runtime, scene
    ctx = runtime.any_context()
    kw = dict(resol=np.float32(0.4), cube_D=32, cube_Dcenter=26, cube_overlapping_ratio=0.5, BB=ref.SCAN9_BB)
    full_grid = int(scene.initializeCubes(**kw)[0].shape[0])
    res = dict(params=dict(resol="float32(0.4)", cube_D=32, cube_Dcenter=26, overlap=0.5, BB=ref.SCAN9_BB.tolist()), order="raster",
               full_grid_cubes=full_grid, runs=[])
    for n in a.sizes:
        base = ref.wavy_cloud(n, seed=1, spatial=True)
        for dt in (np.float32, np.float64):
            pts = base.astype(dt)
            scene.quantizePts2Cubes(pts, **kw)                                            # warm-up (code objects)
            gpu_s = median_time(lambda: scene.quantizePts2Cubes(pts, **kw), a.reps)
            p = scene._plan(pts.dtype, kw["resol"], 32, 26, 0.5, kw["BB"])
            d = ctx.upload(pts)
            call = lambda: ctx.ptcubes_dev(n, d, dt == np.float64, p["stride_q"], p["stride_xyz"], p["half"], p["compute_f64"], box=p["box"])
            call()
            gpu_dev_s = median_time(call, a.reps)
            ctx.profile_reset()
            ctx.profile_enable(True)
            call()
            prof = ctx.profile()
            ctx.profile_enable(False)
            ctx.dev_free(d)
            got, _ = scene.quantizePts2Cubes(pts, **kw)
            t = time.perf_counter()
            want, _ = ref.quantizePts2Cubes(pts, **kw)
            cpu_s = time.perf_counter() - t
            run = dict(n_points=int(n), dtype=np.dtype(dt).name, cubes=int(got.shape[0]), equal=bool(np.array_equal(got, want)),
                       gpu_host_arrays_s=gpu_s, gpu_device_points_s=gpu_dev_s, cpu_restatement_s=cpu_s,
                       stage_ms={k: round(float(v["ms"]), 3) for k, v in prof.items() if k.startswith("pc_")})
            res["runs"].append(run)
            print(json.dumps(run), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
