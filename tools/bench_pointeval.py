"""Times the DTU point-cloud evaluation (surfacenet_amd.evaluation.point_compare) on the GPU at DTU scale, beside scipy's cKDTree on the same host.

    python tools/bench_pointeval.py [--out profiles/pointeval/bench_pointeval.json] [--reps 3] [--no-cpu]

Inputs (seeded): "stl" - 3 M points on a smooth wavy surface over 400 x 300 mm (about 0.2 mm spacing) inside a scan9-sized box; "data" -
a SurfaceNet-like cloud: the surface's voxels on a 0.4 mm lattice, two voxels thick, jittered by 0.05 mm, with 30 % exact duplicates
(overlapping cubes). Two runs: "clean", and "outliers" with 2 % of the data points uniform in the box. Per run: the median wall time of
point_compare (dst 0.2, max_dist 60; host arrays in and out), the per-stage GPU time of its kernels (HIP events), the reduction's rounds, and
the cKDTree time (workers=16, build included) of the two nearest-neighbour queries it replaces.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOX = np.asarray([[-60.0, -40.0, 480.0], [460.0, 340.0, 760.0]])


def surface_z(x, y):
    return 600.0 + 40.0 * np.sin(x / 60.0) * np.cos(y / 45.0) + 10.0 * np.sin(x / 17.0 + y / 23.0)


def make_inputs(seed=0, n_stl=3000000):
    rs = np.random.RandomState(seed)
    xy = rs.uniform(0, 1, (n_stl, 2)) * [400.0, 300.0]
    stl = np.c_[xy, surface_z(xy[:, 0], xy[:, 1])].astype(np.float32).astype(np.float64)
    X, Y = np.meshgrid(np.arange(0, 400, 0.4), np.arange(0, 300, 0.4), indexing="ij")
    Z = np.floor(surface_z(X, Y) / 0.4)[..., None] + np.arange(2)
    data = np.stack(np.broadcast_arrays(X[..., None], Y[..., None], Z * 0.4), -1).reshape(-1, 3)
    data = data + rs.normal(0, 0.05, data.shape)
    data = np.concatenate([data, data[rs.randint(0, data.shape[0], int(0.3 * data.shape[0]))]])
    data = data[rs.permutation(data.shape[0])].astype(np.float32).astype(np.float64)
    out = rs.uniform(BOX[0], BOX[1], (int(0.02 * data.shape[0]), 3))
    return stl, data, np.concatenate([data, out])[rs.permutation(data.shape[0] + out.shape[0])]


def run(ctx, evaluation, data, stl, reps, cpu):
    mask = np.ones((261, 191, 141), np.uint8)
    BB, res, plane = np.asarray([[-60, -40, 480], [460, 340, 760]]), 2, np.asarray([0.0, 0.0, 1.0, -500.0])
    evaluation.point_compare(data, stl, mask, BB, res, plane)             # warm-up (code objects, workspace)
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        base = evaluation.point_compare(data, stl, mask, BB, res, plane)
        ts.append(time.perf_counter() - t)
    ctx.profile_reset()
    ctx.profile_enable(True)
    evaluation.point_compare(data, stl, mask, BB, res, plane)
    prof = ctx.profile()
    ctx.profile_enable(False)
    rank = np.empty(data.shape[0], np.int64)
    rank[np.random.RandomState(0).permutation(data.shape[0])] = np.arange(data.shape[0])
    _, rounds = ctx.point_reduce(data, rank, 0.2)
    res_ = dict(n_data=int(data.shape[0]), n_reduced=int(base["Qdata"].shape[0]), n_stl=int(stl.shape[0]), rounds=int(rounds),
                total_s=float(np.median(ts)), total_s_all=[float(t) for t in ts],
                stage_ms={k: round(float(v["ms"]), 3) for k, v in prof.items() if k.startswith("pe_")},
                launches={k: int(v["launches"]) for k, v in prof.items() if k.startswith("pe_")},
                acc_compl=[float(x) for x in evaluation.eval_acc_compl(base)])
    if cpu:
        from scipy.spatial import cKDTree
        Qd = base["Qdata"]
        t = time.perf_counter()
        dd, _ = cKDTree(stl).query(Qd, workers=16, distance_upper_bound=60.0)
        res_["ckdtree_data_to_stl_s"] = time.perf_counter() - t
        t = time.perf_counter()
        ds, _ = cKDTree(Qd).query(stl, workers=16, distance_upper_bound=60.0)
        res_["ckdtree_stl_to_data_s"] = time.perf_counter() - t
        res_["ckdtree_max_abs_diff_mm"] = float(max(np.abs(np.minimum(dd, 60.0) - base["Ddata"]).max(), np.abs(np.minimum(ds, 60.0) - base["Dstl"]).max()))
    return res_


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointeval", "bench_pointeval.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true", help="skip the cKDTree baseline")
    a = ap.parse_args()
    from surfacenet_amd import evaluation, runtime
    ctx = runtime.any_context()
    stl, data, data_out = make_inputs()
    res = dict(box_mm=BOX.tolist(), dst=0.2, max_dist=60.0)
    for name, d in (("clean", data), ("outliers", data_out)):
        res[name] = run(ctx, evaluation, d, stl, a.reps, not a.no_cpu)
        print(name, json.dumps(res[name]), flush=True)
    res["outliers_over_clean"] = res["outliers"]["total_s"] / res["clean"]["total_s"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(dict(clean_s=res["clean"]["total_s"], outliers_s=res["outliers"]["total_s"])))


if __name__ == "__main__":
    main()
