"""Times one training step of the view-pair weighting net on one MI355X, and its voxel pass alone.

    python tools/bench_relwtrain.py [--out profiles/relwtrain/bench_relwtrain.json] [--reps 5] [--calls 200] [--cubes 64 1024]

Input (seeded): tests/relwtrain_ref.py::make_inputs at cube_D 32 - unfused predictions uniform in (0.02, 0.98), Bernoulli(0.1) targets, unit-norm
feature halves - with the synthetic weights, 2 and 5 view pairs per cube, all tensors resident in HBM (sn_relw_train_step_dev). Per case:
  step_ms               one Nesterov step with every optional result (fused, weights, counts): wall time of `calls` enqueues ended by one
                        synchronise, median of `reps` windows after a warm-up window
  kernel_ms             the library's HIP-event time per launch of each stage (relwtrain_forward / _voxel / _backward / _update, gt_accuracy),
                        from a pass of its own (`calls` steps with profiling on; the events slow the host, so step_ms is not taken there)
  voxel_GBps            what the voxel pass must move - n (n_vp + 1) V 4 bytes read plus n V 4 bytes of f written - over its kernel time, and
  voxel_share_of_hbm    that rate over the 6.3 TB/s a float4 copy achieves on this part (MI355X_MICROARCH.md: 8.0 TB/s on the data sheet).
                        At 64 cubes the tensors (25 - 50 MB) fit the 256 MB Infinity Cache and the launch itself is a large part of the
                        time: the 1024-cube case (0.4 - 0.8 GB per call) is the one that streams from HBM
  equal                 the step's loss, at update 'none', against the float64 restatement (tests/relwtrain_ref.py) within the bound of
                        tests/test_gpu_relwtrain.py - checked for the 64-cube cases before anything is reported
Prints one JSON line."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_ACHIEVABLE = 6.3e12        # bytes / s, float4 copy (MI355X_MICROARCH.md)
HBM_SPEC = 8.0e12


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relwtrain", "bench_relwtrain.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--cubes", type=int, nargs="+", default=[64, 1024])
    a = ap.parse_args()
    import relwtrain_ref as ref
    import surfacenet_amd
    from surfacenet_amd import weights
    s = 32
    v = s ** 3
    values = weights.synthetic_param_values(0)
    res = dict(cube_D=s, reps=a.reps, calls_per_window=a.calls, hbm_achievable_TBps=HBM_ACHIEVABLE / 1e12, hbm_spec_TBps=HBM_SPEC / 1e12, runs=[])
    with surfacenet_amd.Context(cube_D=s, max_samples=2) as ctx:
        for n in a.cubes:
            for n_vp in (2, 5):
                U, F, Y = ref.make_inputs(min(n, 64), n_vp, s, seed=n_vp)
                reps_of_64 = (n + 63) // 64
                if n > 64:                                   # larger batches repeat the 64 cubes (the work does not depend on the values)
                    U, Y = np.tile(U, (reps_of_64, 1, 1, 1, 1))[:n], np.tile(Y, (reps_of_64, 1, 1, 1, 1))[:n]
                    F = np.tile(F.reshape(64, n_vp, -1), (reps_of_64, 1, 1))[:n].reshape(n * n_vp, -1)
                    F = np.ascontiguousarray(F)
                d = dict(U=ctx.upload(U), F=ctx.upload(F), Y=ctx.upload(Y), f=ctx.dev_alloc(n * v * 4), w=ctx.dev_alloc(n * n_vp * 4),
                         c=ctx.dev_alloc(n * 32))
                try:
                    ctx.load_param_values(values)
                    equal = None
                    if n <= 64:
                        ctx.relw_train_begin(0.1, update="none")
                        loss = ctx.relw_train_step_dev(n, n_vp, d["U"], d["F"], d["Y"], d["f"], d["w"], d["c"], want_loss=True)
                        ctx.relw_train_end()
                        L64 = float(ref.step(ref.params_from_values(values, np.float64), U, F, Y, np.float64, ref.cfg())["loss"])
                        equal = bool(abs(loss - L64) <= 4 * 2.0 ** -24 * (math.log2(n * v) + 4) * L64)
                    ctx.relw_train_begin(1e-3, update="nesterov_momentum")
                    step = lambda: ctx.relw_train_step_dev(n, n_vp, d["U"], d["F"], d["Y"], d["f"], d["w"], d["c"])
                    calls = a.calls if n <= 64 else max(10, a.calls // 10)
                    step_ms, step_all = window_ms(ctx, step, calls, a.reps)
                    ctx.profile_reset()
                    ctx.profile_enable(True)
                    for _ in range(calls):
                        step()
                    ctx.synchronize()
                    prof = ctx.profile()
                    ctx.profile_enable(False)
                    ctx.relw_train_end()
                    kernel_ms = {k: p["ms"] / p["launches"] for k, p in prof.items() if k.startswith("relwtrain_") or k == "gt_accuracy"}
                    vox_bytes = n * (n_vp + 1) * v * 4 + n * v * 4
                    vox_rate = vox_bytes / (kernel_ms["relwtrain_voxel"] * 1e-3)
                    run = dict(cubes=n, view_pairs=n_vp, rows=n * n_vp, equal=equal, step_ms=step_ms, step_ms_all=step_all,
                               kernel_ms={k: round(x, 5) for k, x in kernel_ms.items()}, kernel_ms_sum=round(sum(kernel_ms.values()), 5),
                               voxel_bytes=vox_bytes, voxel_GBps=vox_rate / 1e9, voxel_share_of_hbm=vox_rate / HBM_ACHIEVABLE,
                               voxel_share_of_hbm_spec=vox_rate / HBM_SPEC)
                    res["runs"].append(run)
                    print(json.dumps(run), file=sys.stderr, flush=True)
                finally:
                    for p in d.values():
                        ctx.dev_free(p)
    if not all(r["equal"] in (True, None) for r in res["runs"]):
        raise SystemExit("the GPU loss differs from the restatement: nothing is reported")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
