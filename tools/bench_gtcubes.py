"""Times the ground-truth mode on one MI355X, beside the forward pass of the same batch and the numpy restatement
(tests/gtcubes_ref.py) on the same box's host.

    python tools/bench_gtcubes.py [--out profiles/gtcubes/bench_gtcubes.json] [--reps 5] [--calls 50] [--sizes 200000 3000000]

Input (seeded): tests/ptcubes_ref.py::wavy_cloud as float32 - a noisy wavy sheet across DTU scan9's bounding box - and 64 of the cubes
scene.quantizePts2Cubes seeds from it with scan9's parameters (evenly spaced through its list), cube_D 32, 2 view pairs per cube (128 samples:
what a context of this cube size holds). Per cloud size:
  bind_ms               sn_gt_bind_dev, points already in HBM: median wall time of `reps` calls (the call returns when the cloud is sorted)
  gt_cubes_ms           sn_gt_cubes_dev per call of 64 cubes: wall time of `calls` calls ended by one synchronise, median of `reps` windows
  accuracy_ms, GB/s     sn_weighted_accuracy_dev the same way, on the fused tensor of the forward pass and the Y of gt_cubes; the rate is
                        the 8 bytes per voxel it must read over that time
  forward_ms            sn_cvc_forward_dev (CVC warp, network, fusion) of the same batch, the same way
  gt_share_of_step      (gt_cubes_ms + accuracy_ms) / forward_ms
  kernel_ms             the library's HIP-event times of the gt_* stages for one call of each, taken in a pass of its own
  restatement_s         tests/gtcubes_ref.py for the same 64 cubes, one run (numpy, one thread; context only) - and the GPU result is compared
                        with it (equal: true) before anything is reported
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def window_ms(ctx, fn, calls, reps):
    """ms per call: `calls` enqueues ended by one synchronise, median of `reps` such windows (after a warm-up window)"""
    out = []
    for r in range(reps + 1):
        ctx.synchronize()
        t = time.perf_counter()
        for _ in range(calls):
            fn()
        ctx.synchronize()
        out.append((time.perf_counter() - t) * 1e3 / calls)
    return float(np.median(out[1:])), [round(v, 4) for v in out[1:]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gtcubes", "bench_gtcubes.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--sizes", type=int, nargs="+", default=[200000, 3000000])
    a = ap.parse_args()
    import gtcubes_ref as ref
    import ptcubes_ref
    import surfacenet_amd
    from surfacenet_amd import synthetic, weights
    s, n, n_vp = 32, 64, 2
    v = s ** 3
    sc = synthetic.synthetic_scene(n, n_vp, s=s, seed=0)
    res = dict(cube_D=s, cubes_per_call=n, view_pairs=n_vp, reps=a.reps, calls_per_window=a.calls, bytes_per_voxel=8, runs=[])
    with surfacenet_amd.Context(cube_D=s, max_samples=n * n_vp) as ctx:
        ctx.load_param_values(weights.synthetic_param_values(0))
        ctx.set_cameras(sc["cams"])
        ctx.set_images(sc["imgs"])
        d = dict(pairs=ctx.upload(sc["pairs"]), w=ctx.upload(sc["w"]), fused=ctx.dev_alloc(n * v * 4), Y=ctx.dev_alloc(n * v * 4),
                 counts=ctx.dev_alloc(n * 32))
        for n_pts in a.sizes:
            pts = ptcubes_ref.wavy_cloud(n_pts).astype(np.float32)
            cubes, side = ptcubes_ref.quantizePts2Cubes(pts, BB=ptcubes_ref.SCAN9_BB, **ptcubes_ref.SCAN9)
            cubes = cubes[np.linspace(0, len(cubes) - 1, n).astype(int)]
            xyz, resol = np.ascontiguousarray(cubes["xyz"]), np.ascontiguousarray(cubes["resol"])
            cell = float(side) / 4
            d_pts, d_xyz, d_resol = ctx.upload(pts), ctx.upload(xyz), ctx.upload(resol)
            try:
                ctx.gt_bind_dev(n_pts, d_pts, cell)                                    # warm-up (code objects, workspace)
                binds = []
                for _ in range(a.reps):
                    t = time.perf_counter()
                    ctx.gt_bind_dev(n_pts, d_pts, cell)
                    binds.append((time.perf_counter() - t) * 1e3)
                forward = lambda: ctx.cvc_forward_dev(n, n_vp, d["pairs"], d_xyz, d_resol, d["w"], d["fused"])
                cubes_fn = lambda: ctx.gt_cubes_dev(n, d_xyz, d_resol, d["Y"])
                acc_fn = lambda: ctx.weighted_accuracy_dev(n, d["fused"], d["Y"], d["counts"])
                forward(); cubes_fn(); acc_fn()
                ctx.synchronize()
                Y, fused, counts = np.empty((n, 1, s, s, s), np.float32), np.empty((n, 1, s, s, s), np.float32), np.empty((n, 4), np.int64)
                ctx.d2h(Y, d["Y"]); ctx.d2h(fused, d["fused"]); ctx.d2h(counts, d["counts"])
                t = time.perf_counter()
                want = ref.gt_cubes(pts, xyz, resol, s)
                want_counts = ref.accuracy_counts(fused, want)
                cpu_s = time.perf_counter() - t
                equal = bool(np.array_equal(Y, want) and np.array_equal(counts, want_counts))
                fwd_ms, fwd_all = window_ms(ctx, forward, max(1, a.calls // 10), a.reps)
                gt_ms, gt_all = window_ms(ctx, cubes_fn, a.calls, a.reps)
                acc_ms, acc_all = window_ms(ctx, acc_fn, a.calls, a.reps)
                ctx.profile_reset()
                ctx.profile_enable(True)
                ctx.gt_bind_dev(n_pts, d_pts, cell); cubes_fn(); acc_fn()
                ctx.synchronize()
                prof = ctx.profile()
                ctx.profile_enable(False)
                run = dict(n_points=int(n_pts), grid_cell_mm=cell, occupied_voxels_per_cube=float(want.sum() / n), equal=equal,
                           bind_ms=float(np.median(binds)), bind_ms_all=[round(b, 3) for b in binds],
                           gt_cubes_ms=gt_ms, gt_cubes_ms_all=gt_all, accuracy_ms=acc_ms, accuracy_ms_all=acc_all,
                           accuracy_GBps=n * v * 8 / (acc_ms * 1e-3) / 1e9, forward_ms=fwd_ms, forward_ms_all=fwd_all,
                           gt_share_of_step=(gt_ms + acc_ms) / fwd_ms, accuracy_of_batch=float(ref.accuracy_from_counts(counts)),
                           kernel_ms={k: round(float(p["ms"]), 4) for k, p in prof.items() if k.startswith("gt_")}, restatement_s=cpu_s)
                res["runs"].append(run)
                print(json.dumps(run), file=sys.stderr, flush=True)
            finally:
                for p in (d_pts, d_xyz, d_resol):
                    ctx.dev_free(p)
        for p in d.values():
            ctx.dev_free(p)
    if not all(r["equal"] for r in res["runs"]):
        raise SystemExit("the GPU result differs from the restatement: nothing is reported")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
