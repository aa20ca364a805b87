#!/usr/bin/env python3
"""bench.py — headline measurement of the MI355X SurfaceNet hot path (BASELINE.json metric).

One "step" = one pass of the hot path (CVC warp -> 3D-CNN -> view-pair fusion) over one batch of synthetic cubes,
inputs (images, cameras, cube parameters, weights) already resident in HBM, outputs left in HBM.
Workload = BASELINE.json configs[1]: synthetic 2-view 1600x1200, s=32, 64 cubes per GPU, N_viewpair=2.
N>1: one process per GPU (torch.distributed / RCCL), cubes sharded per rank (weak scaling), one all-gather of the
per-cube fused surface probabilities per step (north_star's exchange step).

    python bench.py --gpus 1 --steps 10 --warmup 3
    python bench.py --gpus 1 --steps 10 --warmup 3 --full
    python bench.py --gpus 1 --steps 10 --warmup 3 --dump-outputs bench_outputs
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Prints ONE JSON line on rank 0 (metric, value, unit, higher_is_better, dtype, ms_per_step = milliseconds of one timed step). A plain run
sets up, warms up, times exactly K steps (no per-kernel events) and prints the line. --full adds everything else: `box` (sn_mfma_probe),
`roofline` / `kernels_ms_per_step` (dominant kernel, HIP-event timed in a second loop of the same K steps right after the timed region), and
at N=1 the extra legs (f16x3p / f16 modes, s=64, post pass, similarityNet, scene samples, `cpu_baseline`: oracle timed on the host cores,
bounded sample); --no-* skips single legs of --full. --dump-outputs DIR writes what the last timed step computed (the fused surface
probabilities, all ranks' cubes on rank 0) as DIR/fused.npy, float32; the inputs are seeded, so two builds compare output for output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

NATIVE_COMM_DEADLINE_S = 180      # --gpus N: the library's own RCCL communicator must be up (and verified) within this, else torch.distributed carries the exchange

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from surfacenet_amd import synthetic          # noqa: E402  (synthetic inputs of SURVEY §8d; nothing here imports tests/)
MEAN6 = synthetic.MEAN6

DTYPE = {"f16m8": "f16 main term + 6-bit (fp6 e2m3, MX-scaled MFMA) correction terms in every layer, f32 accumulate (L_inf 1e-4 .. 4e-4); CVC warp f64",
         "f16x3": "f16x3 (each operand = hi+lo fp16 pair, 3 MFMAs per product, f32 accumulate: fp32-class results; the two correction terms of a product run on one MX-scaled MFMA in the two merge layers (fp6 e2m3 codes) and in the three dilated layers conv4_x (fp8 e4m3 codes); L_inf vs fp64 oracle 3e-5 .. 1.7e-4, asserted < 2e-4, bar 1e-3); CVC warp f64",
         "f16x3p": "f16x3 pure (each operand = hi+lo fp16 pair, 3 fp16 MFMAs per product in every layer, f32 accumulate); CVC warp f64",
         "f16": "f16 (MFMA, f32 accumulate); CVC warp f64"}
MFMA_F16_DENSE_PEAK_TFLOPS = 2500.0      # /opt/skills/guides/MI355X_MICROARCH.md: BF16/FP16 MFMA dense peak
CNN_FLOPS_PER_SAMPLE_S32 = 44511690752   # learned-conv FLOPs per cube-view-pair at s=32


DUMP_MAX_BYTES = 64 * 10 ** 6        # --dump-outputs: a larger output (many ranks) is written as a seeded sample of its cubes


def dump_outputs(dirname, fused):
    """--dump-outputs: the fused surface probabilities (cubes, 1, s, s, s) of the last timed step as DIR/fused.npy (float32); above
    DUMP_MAX_BYTES a fixed, seeded sample of whole cubes in index order as DIR/fused_sample.npy."""
    os.makedirs(dirname, exist_ok=True)
    name = "fused"
    if fused.nbytes > DUMP_MAX_BYTES:
        k = DUMP_MAX_BYTES // (fused.nbytes // fused.shape[0])
        fused, name = fused[np.sort(np.random.RandomState(0).choice(fused.shape[0], k, replace=False))], "fused_sample"
    np.save(os.path.join(dirname, name + ".npy"), np.ascontiguousarray(fused, dtype=np.float32))


KERNEL_SOURCES = ["conv3d_mfma.h", "mx_format.h", "cvc_warp.h", "elementwise.h", "sn_internal.h", "sn_api.hip"]


def _strip_comments(text):
    """C++ source without comments and with whitespace runs collapsed: what the compiler sees (string literals kept as they are)."""
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if c == '"' or c == "'":
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == "\\" else 1
            out.append(text[i:j + 1]); i = j + 1
        elif text.startswith("//", i):
            j = text.find("\n", i)
            i = n if j < 0 else j
        elif text.startswith("/*", i):
            j = text.find("*/", i + 2)
            i = n if j < 0 else j + 2
        else:
            out.append(c); i += 1
    return " ".join("".join(out).split())


def kernel_src_sha16():
    """sha256[:16] over the sources the hot-path kernels are built from, COMMENTS AND WHITESPACE STRIPPED: stamps profiles/pmc_traffic.json (tools/pmc_traffic.py).
    A comment-only edit keeps the stamp (the kernels are the same); any change of code drops the traffic figure until the counters are collected again."""
    import hashlib
    h = hashlib.sha256()
    for f in KERNEL_SOURCES:
        h.update(_strip_comments(open(os.path.join(ROOT, "surfacenet_amd", "csrc", f), "r", encoding="utf-8", errors="replace").read()).encode("utf-8"))
    return h.hexdigest()[:16]


def cpu_baseline(scene, values, s, n_vp):
    """Times the oracle (CPU restatement of the reference path) on a bounded sample of the same workload."""
    import torch
    from oracle import cvc_oracle, net_oracle
    n_cvc, n_cnn = 64, 32          # ~10 s of host work in total
    sub = lambda k: {kk: (v[:k] if kk in ("xyz", "resol", "pairs", "w") else v) for kk, v in scene.items()}
    a = sub(n_cvc)
    t0 = time.time()
    X = cvc_oracle.gen_coloredCubes(a["pairs"], a["xyz"], a["resol"], a["cams"], a["imgs"], s, mean6=MEAN6)
    t_cvc = (time.time() - t0) / n_cvc
    b = sub(n_cnn)
    Xb = X[: n_cnn * n_vp]
    net_oracle.forward_torch(Xb[:1], values, w=None, n_vp=1, dtype="float32")   # warm-up (thread pool, allocations)
    t0 = time.time()
    net_oracle.forward_torch(Xb, values, w=b["w"], n_vp=n_vp, dtype="float32")
    t_cnn = (time.time() - t0) / n_cnn
    return {"value": round(1.0 / (t_cvc + t_cnn), 3), "unit": "cubes/s", "cores": int(torch.get_num_threads()),
            "kind": "port",
            "sample": "oracle CVC (C, 1 thread) on %d cubes + oracle CNN (torch CPU conv3d fp32, %d threads of %d host cores) on %d cubes; "
                      "cvc %.4f s/cube, cnn %.3f s/cube" % (n_cvc, torch.get_num_threads(), os.cpu_count(), n_cnn, t_cvc, t_cnn)}


def fast_mode(surfacenet_amd, scene, values, s, n, n_vp, device, steps, precision="f16", note=None):
    """Extra, non-headline measurements of the same workload in another arithmetic: the opt-in f16 mode (fails the 1e-3 parity bar; see DESIGN.md
    §Numerics) and `f16x3p` (three fp16 MFMAs per product in EVERY layer: fp32-class everywhere, L_inf ~1e-5 - the number that survives the strictest
    reading of "not narrower than the reference's fp32")."""
    ctx = surfacenet_amd.Context(cube_D=s, max_samples=n * n_vp, device=device, precision=precision)
    ctx.load_param_values(values)
    ctx.set_cameras(scene["cams"]); ctx.set_images(scene["imgs"])
    d = [ctx.upload(scene[k]) for k in ("pairs", "xyz", "resol", "w")]
    d_fused = ctx.dev_alloc(n * s ** 3 * 4)
    for _ in range(2):
        ctx.cvc_forward_dev(n, n_vp, d[0], d[1], d[2], d[3], d_fused)
    ctx.synchronize()
    ctx.profile_reset(); ctx.profile_enable(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        ctx.cvc_forward_dev(n, n_vp, d[0], d[1], d[2], d[3], d_fused)
    ctx.synchronize()
    el = time.perf_counter() - t0
    prof = ctx.profile()
    ctx.close()
    dom = max((k for k in prof if prof[k]["flops"] > 0), key=lambda k: prof[k]["ms"])
    ach = prof[dom]["flops"] / (prof[dom]["ms"] * 1e-3) / 1e12
    conv_ms = sum(v["ms"] for v in prof.values() if v["flops"] > 0)
    conv_fl = sum(v["flops"] for v in prof.values())
    return {"value": round(n * steps / el, 2), "unit": "cubes/s", "ms_per_step": round(el / steps * 1e3, 3), "steps": steps,
            "roofline": {"bound": "mfma", "kernel": "conv3d_f16_mfma<%s>" % dom, "achieved": round(ach, 1), "peak": MFMA_F16_DENSE_PEAK_TFLOPS,
                         "unit": "TFLOP/s", "frac": round(ach / MFMA_F16_DENSE_PEAK_TFLOPS, 4), "avg_launch_ms": round(prof[dom]["ms"] / prof[dom]["launches"], 4)},
            "cnn_all_convs_tflops": round(conv_fl / (conv_ms * 1e-3) / 1e12, 1),
            "note": note or "operands rounded to fp16: L_inf vs fp64 oracle 1e-3..4e-3 on BN-calibrated nets (above the 1e-3 bar) - not the headline"}


def s64_mode(surfacenet_amd, values, n_vp, device, steps, precision, n=32):
    """Extra, non-headline measurement: one GPU's shard of BASELINE.json configs[3] - s=64 (params.py:65 __cube_D = 64), batch 256 over 8 GPUs =
    32 cubes x n_vp view pairs per step and GPU (4x the voxel count of the headline step; 21 GB of activation workspace)."""
    s = 64
    scene = synthetic.synthetic_scene(n, n_vp, s=s, seed=0)
    ctx = surfacenet_amd.Context(cube_D=s, max_samples=n * n_vp, device=device, precision=precision)
    ctx.load_param_values(values)
    ctx.set_cameras(scene["cams"]); ctx.set_images(scene["imgs"])
    d = [ctx.upload(scene[k]) for k in ("pairs", "xyz", "resol", "w")]
    d_fused = ctx.dev_alloc(n * s ** 3 * 4)
    for _ in range(2):
        ctx.cvc_forward_dev(n, n_vp, d[0], d[1], d[2], d[3], d_fused)
    ctx.synchronize()
    ctx.profile_reset(); ctx.profile_enable(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        ctx.cvc_forward_dev(n, n_vp, d[0], d[1], d[2], d[3], d_fused)
    ctx.synchronize()
    el = time.perf_counter() - t0
    prof = ctx.profile()
    ctx.close()
    dom = max((k for k in prof if prof[k]["flops"] > 0), key=lambda k: prof[k]["ms"])
    ach = prof[dom]["flops"] / (prof[dom]["ms"] * 1e-3) / 1e12
    return {"value": round(n * steps / el, 2), "unit": "cubes/s (s=64)", "ms_per_step": round(el / steps * 1e3, 3), "cubes_per_step": n, "n_vp": n_vp,
            "workload": "one GPU's shard of BASELINE.json configs[3]: s=64, 256 cubes over 8 GPUs = %d cubes x %d view pairs per step" % (n, n_vp),
            "equivalent_s32_cubes_per_s": round(8 * n * steps / el, 1),
            "roofline": {"bound": "mfma", "kernel": "conv3d_f16_mfma<%s>" % dom, "achieved": round(ach, 1), "peak": MFMA_F16_DENSE_PEAK_TFLOPS,
                         "unit": "TFLOP/s", "frac": round(ach / MFMA_F16_DENSE_PEAK_TFLOPS, 4), "avg_launch_ms": round(prof[dom]["ms"] / prof[dom]["launches"], 4),
                         "launches": prof[dom]["launches"]}}


def post_pass(surfacenet_amd, ctx, scene, s, n, n_vp, steps, keep_frac=0.1):
    """Extra, non-headline measurement: the whole loop body of main_reconstruct.py:134-160 --
    hot path + voxel colours + ray pooling + dense2sparse -- device-resident (reconstruct.SparseLoop), packed sparse
    lists copied to the host every step. min_prob is set at the (1-keep_frac) quantile of the synthetic net's outputs
    so that keep_frac of the voxels survive (random weights have no surfaces; ~10% is a thick one)."""
    from surfacenet_amd import reconstruct
    from oracle import post_oracle
    fused, _, _ = ctx.cvc_forward(scene["pairs"][:4], scene["xyz"][:4], scene["resol"][:4], scene["w"][:4], return_unfused=False)
    p16 = fused.astype(np.float16)[:, 0]
    dc = {32: 26, 64: 52}.get(s, s)                       # params.py: __cube_Dcenter = {32:26, 64:52}
    lo = (s - dc) // 2
    core = p16[:, lo:lo + dc, lo:lo + dc, lo:lo + dc]     # the centre crop is what dense2sparse keeps
    vals, cnt = np.unique(core, return_counts=True)                # float16 outputs have few distinct values: pick the one whose
    above = 1.0 - np.cumsum(cnt) / float(core.size)               # strict ">" keeps closest to keep_frac of the voxels
    thr = float(vals[int(np.argmin(np.abs(above - keep_frac)))])
    loop = reconstruct.SparseLoop(ctx, n_vp, max_cubes=n, min_prob=thr, rayPool_thresh=0, enable_centerCrop=True, cube_Dcenter=dc,
                                  enable_rayPooling=True)
    reps = 16                                              # 16 batches of n cubes per call: run_many pipelines them (a scene has thousands)
    args = tuple(np.concatenate([scene[k]] * reps) for k in ("pairs", "xyz", "resol", "w"))
    res = loop.run_many(*args)
    ctx.synchronize()
    steps = max(2, steps // 4)
    t0 = time.perf_counter()
    for _ in range(steps):
        res = loop.run_many(*args)
    ctx.synchronize()
    dt = (time.perf_counter() - t0) / (steps * reps)
    ctx.profile_reset(); ctx.profile_enable(True)           # per-kernel times from a separate pass (events around every launch)
    loop.run_many(*args)
    ctx.synchronize()
    prof = ctx.profile(); ctx.profile_enable(False); ctx.profile_reset()
    loop.close()
    steps = reps
    kept = int(sum(len(x) for x in res[2])) // reps
    t0 = time.perf_counter()                              # CPU: the oracle's ray pooling on the same first cubes
    for i in range(4):
        post_oracle.ray_pool_1cube(scene["cams"], p16[i], scene["pairs"][i], scene["xyz"][i], scene["resol"][i], thr)
    t_cpu = (time.perf_counter() - t0) / 4
    rp, d2 = prof.get("ray_pool"), prof.get("dense2sparse")
    out = {"value": round(n / dt, 2), "unit": "cubes/s", "what": "CVC+CNN+fusion+colour fusion+ray pooling+dense2sparse, sparse lists to host each step (16 batches per call, pipelined: SparseLoop.run_many)",
           "ms_per_step": round(dt * 1e3, 3), "min_prob": round(thr, 4), "kept_voxels_per_cube": round(kept / float(n), 1),
           "kernels_ms_per_step": {k: round(v["ms"] / steps, 3) for k, v in prof.items() if k in ("ray_pool", "dense2sparse", "color_fuse")},
           "cpu_ray_pool_ms_per_cube": round(t_cpu * 1e3, 2)}
    if rp:
        out["ray_pool_GBps"] = round(rp["bytes"] / (rp["ms"] * 1e-3) / 1e9, 1)
    if d2:
        out["dense2sparse_GBps"] = round(d2["bytes"] / (d2["ms"] * 1e-3) / 1e9, 1)
    return out


def simil_net(surfacenet_amd, ctx, scene, steps, n=2040):        # = one internal chunk of the library (sn_simil.hip kSimChunk)
    """Extra, non-headline measurement: earlyRejection.patch2embedding's inner loop for one view --
    crop n 64x64 patches around projected cube centres, preprocess, similarityNet embedding -- without leaving HBM
    (sn_crop_embed); embeddings (n,128) copied to the host every step."""
    from surfacenet_amd import weights
    from oracle import simil_oracle
    values = weights.synthetic_simil_param_values(0)
    ctx.load_simil_param_values(values)
    mean = np.asarray([103.939, 116.779, 123.68], dtype=np.float32)           # params.py:130
    rs = np.random.RandomState(1)
    H, W = scene["imgs"][0].shape[:2]
    ch, cw = rs.uniform(0, H, n), rs.uniform(0, W, n)
    ctx.crop_embed(0, ch, cw, mean)
    ctx.profile_reset(); ctx.profile_enable(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        emb = ctx.crop_embed(0, ch, cw, mean)
    dt = (time.perf_counter() - t0) / steps
    prof = ctx.profile(); ctx.profile_enable(False); ctx.profile_reset()
    # the same through ONE call for 16 chunks (a DTU view holds ~126,000 in-scope cube centres = 62 chunks per call: sn_crop_embed runs them back to back, centres up and
    # embeddings down once): what the early-rejection stage of a scene sees, without the per-step synchronisation of the 2,040-patch steps above
    nb = 16 * n
    chb, cwb = rs.uniform(0, H, nb), rs.uniform(0, W, nb)
    t0 = time.perf_counter()
    ctx.crop_embed(0, chb, cwb, mean)
    dt_big = time.perf_counter() - t0
    flops_patch = sum(2.0 * (64 >> st) ** 2 * 9 * ci * co for (_, ci, co), st in zip(weights.SIMIL_CONVS, [0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4]))
    conv = {k: v for k, v in prof.items() if k.startswith("s_conv")}
    conv_ms = sum(v["ms"] for v in conv.values()) / steps
    dom = max(conv, key=lambda k: conv[k]["ms"])
    d = conv[dom]
    raw = simil_oracle.crop_patches(scene["imgs"][0], ch[:4], cw[:4])
    X = simil_oracle.preprocess(raw, mean)
    simil_oracle.embedding_torch(X[:1], values, dtype="float32")
    t0 = time.perf_counter()
    ref = simil_oracle.embedding_torch(X, values, dtype="float32")
    t_cpu = (time.perf_counter() - t0) / 4
    return {"value": round(n / dt, 1), "unit": "patches/s", "what": "crop + preprocess + similarityNet embedding, %d patches of one view per step, embeddings to host" % n,
            "ms_per_step": round(dt * 1e3, 3), "one_call_of_16_chunks_patches_per_s": round(nb / dt_big, 1), "gflop_per_patch": round(flops_patch / 1e9, 3),
            "convs_tflops": round(flops_patch * n / (conv_ms * 1e-3) / 1e12, 1), "convs_ms_per_step": round(conv_ms, 3),
            "dominant": {"kernel": "conv3d_f16_mfma<K2D %s>" % dom, "avg_launch_ms": round(d["ms"] / d["launches"], 4),
                         "achieved_tflops": round(d["flops"] / (d["ms"] * 1e-3) / 1e12, 1), "frac_of_f16_mfma_peak": round(d["flops"] / (d["ms"] * 1e-3) / 1e12 / MFMA_F16_DENSE_PEAK_TFLOPS, 4)},
            "kernels_ms_per_step": {k: round(v["ms"] / steps, 3) for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"]) if v["launches"]},
            "cpu_oracle_patches_per_s": round(1.0 / t_cpu, 2), "check_Linf_vs_oracle_f32": float(np.abs(emb[:4] - ref).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cube-d", type=int, default=32)
    ap.add_argument("--cubes", type=int, default=64, help="cubes per GPU per step")
    ap.add_argument("--n-vp", type=int, default=2)
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "f16x3p", "f16m8", "f16"],
                    help="f16x3 (default): hi/lo split fp16 operands, fp32-class results (parity grade); f16: fast mode, L_inf ~2e-3")
    ap.add_argument("--torch-comm", action="store_true", help="N>1: all-gather through torch.distributed instead of the library's own RCCL binding (the default: "
                    "sn_comm_init / sn_allgather_f32_dev_overlap on the context's communication stream, overlapping the next step's kernels; torch.distributed "
                    "still carries the 128-byte id and the barriers). The native path is checked against torch's result before the timed region and the "
                    "bench falls back to torch.distributed - saying so in its JSON line - if it cannot be set up")
    ap.add_argument("--native-comm", action="store_true", help=argparse.SUPPRESS)      # (the default since round 4; kept for old command lines)
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="process-group backend. nccl (= RCCL, default): what the driver's N>1 runs use. gloo: control plane and fall-back all-gather over "
                         "host memory (the fused probabilities are staged through the host every step) - lets N ranks SHARE one GPU, so that the N>1 decision "
                         "logic (any rank fails => all ranks fall back, MIN all-reduce, MAX-over-ranks timing, rank-seeded shards) runs with a real peer on a "
                         "one-GPU box (tests/test_gpu_bench.py); not a performance mode")
    ap.add_argument("--native-deadline", type=float, default=NATIVE_COMM_DEADLINE_S, help="seconds the library's own RCCL communicator has to come up (and its probe all-gather to verify) before torch.distributed carries the exchange")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the fused surface probabilities of the last timed step as DIR/fused.npy (float32)")
    ap.add_argument("--full", action="store_true", help="also the non-headline measurements: box probe, per-kernel / roofline loop and, at N=1, the extra "
                    "legs below (other precisions, s=64, post pass, similarityNet, scenes, CPU baseline); the --no-* options skip single legs")
    ap.add_argument("--no-fast-mode", action="store_true", help="skip the extra f16 fast-mode measurement")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-s64", action="store_true", help="skip the extra s=64 measurement")
    ap.add_argument("--no-simil", action="store_true", help="skip the extra similarityNet (early rejection) measurement")
    ap.add_argument("--no-post-pass", action="store_true", help="skip the extra whole-loop-body (ray pooling / dense2sparse) measurement")
    ap.add_argument("--no-scenes", action="store_true", help="skip the extra end-to-end scene samples (BASELINE configs[2] and [4] on their dataset calibration)")
    ap.add_argument("--scene-cubes", type=int, default=4000, help="cubes sampled evenly from each scene's grid for the scene samples (0 = the whole grid: 195,360 / 15,456)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus %d needs `python -m torch.distributed.run --nproc-per-node %d bench.py ...`" % (args.gpus, args.gpus))
        raise SystemExit("WORLD_SIZE=%d does not match --gpus %d" % (world, args.gpus))

    import surfacenet_amd
    from surfacenet_amd import weights

    s, n, n_vp = args.cube_d, args.cubes, args.n_vp
    s3 = s ** 3
    dist = None
    torch = None
    use_dist = world > 1 or bool(os.environ.get("BENCH_FORCE_DIST"))
    if use_dist:
        import torch
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if local_rank >= torch.cuda.device_count():      # launcher restricted the visible devices to one per rank
            local_rank = 0
        if os.environ.get("BENCH_TEST_SHARE_GPU0"):      # tests only (tests/test_gpu_bench.py): every rank on device 0, whatever the box holds - the shared-GPU scenario
            local_rank = 0
        torch.cuda.set_device(local_rank)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if args.dist_backend == "nccl":
            dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    ctl_dev = "cuda" if args.dist_backend == "nccl" else "cpu"      # where the control-plane tensors (id broadcast, flags, timings) live
    deadline = float(args.native_deadline)

    scene = synthetic.synthetic_scene(n, n_vp, s=s, seed=rank)   # each rank owns a different shard of cubes
    values = weights.synthetic_param_values(0)
    if os.environ.get("BENCH_ZERO_DATA"):   # DVFS experiment only: all-zero operands draw less power
        values = [np.zeros_like(v) if (v.ndim == 5 and v.shape[2] == 3 and v.shape[0] != 1) else v for v in values]
        scene["imgs"] = [np.zeros_like(im) for im in scene["imgs"]]
    def make_ctx():
        c = surfacenet_amd.Context(cube_D=s, max_samples=n * n_vp, device=local_rank, precision=args.precision)
        c.load_param_values(values)
        c.set_cameras(scene["cams"])
        c.set_images(scene["imgs"])
        return (c,) + tuple(c.upload(scene[k]) for k in ("pairs", "xyz", "resol", "w"))
    ctx, d_pairs, d_xyz, d_resol, d_w = make_ctx()
    # what THIS box sustains on a pure fp16 MFMA stream, measured right before the timed region (boxes of the pool fall into speed classes 5-8 % apart;
    # every absolute number below moves with it). ~10 ms launches, outside the timed region. --full only.
    box = None
    if args.full:
        try:
            tf, ghz = ctx.mfma_probe(10.0)
            box = {"sustained_f16_tflops": round(tf, 1), "effective_clock_ghz": round(ghz, 3), "frac_of_nominal_peak": round(tf / MFMA_F16_DENSE_PEAK_TFLOPS, 4),
                   "what": "pure v_mfma_f32_16x16x32_f16 stream, all CUs, one wave per SIMD, random operands, last of four ~10 ms launches (sn_mfma_probe)"}
        except Exception as e:      # noqa: BLE001 - a measurement aid must not cost the bench line
            box = {"error": "%s: %s" % (type(e).__name__, e)}
    native = use_dist and not (args.torch_comm or bool(os.environ.get("BENCH_TORCH_COMM")))
    comm_note, native_hung, rccl_info = None, False, None
    if native:
        # the C ABI's own exchange: rank 0 draws the RCCL unique id, torch.distributed ships its 128 bytes, every rank joins (sn_comm_init_deadline:
        # the library bounds the wait itself); then one small all-gather through the library is checked against known data. Any failure on any
        # rank -> every rank falls back to torch. The probe all-gather runs in a helper thread with the same deadline: a collective that never
        # completes (the binding has only ever met a one-rank group on the builder's boxes) must cost a note in the JSON line, not the scaling
        # run - and a context whose helper thread is still inside the library is ABANDONED (a fresh one carries the torch path).
        import threading
        state = {"ok": 0, "why": "native all-gather probe did not finish within %g s" % deadline}
        uid = torch.zeros(128, dtype=torch.uint8, device=ctl_dev)
        if rank == 0:
            try:
                uid.copy_(torch.frombuffer(bytearray(surfacenet_amd.Context.comm_unique_id()), dtype=torch.uint8))
            except Exception as e:      # noqa: BLE001
                state["why"] = "%s: %s" % (type(e).__name__, e)
        dist.broadcast(uid, src=0)
        uid_bytes = bytes(uid.cpu().numpy().tobytes())
        try:
            rccl_info = surfacenet_amd.Context.comm_info()
        except Exception as e:      # noqa: BLE001
            rccl_info = ("unavailable: %s" % e, 0)
        joined = False
        late = float(os.environ.get("BENCH_TEST_LATE_RANK1_S", "0") or 0)      # tests only: rank 1 arrives at the communicator set-up this much late
        if late > 0 and rank == 1:
            time.sleep(late)
        try:
            ctx.comm_init(world, rank, uid_bytes, timeout_s=deadline)
            joined = True
        except Exception as e:      # noqa: BLE001 - whatever went wrong, the scaling run must still produce a number
            state["why"] = "%s: %s" % (type(e).__name__, e)

        def _native_probe(c):
            try:
                torch.cuda.set_device(local_rank)
                probe = (np.arange(4096, dtype=np.float32) + 10000.0 * rank)
                d_p, d_pg = c.upload(probe), c.dev_alloc(world * probe.nbytes)
                c.allgather_f32_dev_overlap(d_p, probe.size, d_pg, 7)
                c.synchronize()
                got = np.empty((world * probe.size,), np.float32)
                c.d2h(got, d_pg)
                want = np.concatenate([np.arange(4096, dtype=np.float32) + 10000.0 * r for r in range(world)])
                c.dev_free(d_p); c.dev_free(d_pg)
                if np.array_equal(got, want):
                    state["ok"] = 1
                else:
                    state["why"] = "native all-gather returned wrong data"
            except Exception as e:      # noqa: BLE001
                state["why"] = "%s: %s" % (type(e).__name__, e)

        if joined:
            th = threading.Thread(target=_native_probe, args=(ctx,), daemon=True)
            th.start()
            th.join(deadline)
            native_hung = th.is_alive()
        ok, why = (0 if native_hung else state["ok"]), state["why"]
        flag = torch.tensor([ok], dtype=torch.int32, device=ctl_dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) == 0:
            native, comm_note = False, "native RCCL binding unavailable (%s): torch.distributed all-gather instead" % (why or "another rank failed")
            if native_hung:
                ctx, d_pairs, d_xyz, d_resol, d_w = make_ctx()     # the old context belongs to the stuck thread now: never touched again
    if native:
        d_fused = [ctx.dev_alloc(n * s3 * 4) for _ in range(2)]
        d_all = [ctx.dev_alloc(world * n * s3 * 4) for _ in range(2)]
    elif use_dist and args.dist_backend == "gloo":
        # host-staged exchange (tests on a shared GPU; see --dist-backend): device -> host, gloo all-gather, nothing overlaps
        d_fused = [ctx.dev_alloc(n * s3 * 4) for _ in range(2)]
        h_fused = np.empty((n * s3,), np.float32)
        t_all_host = torch.empty(world * n * s3, dtype=torch.float32)
    elif use_dist:
        # Double-buffered and host-sync free: the all-gather of step i (torch's stream) overlaps the kernels of step i+1 (the
        # context's stream); the two streams are ordered against each other with events only.
        t_fused = [torch.empty(n * s3, dtype=torch.float32, device="cuda") for _ in range(2)]
        t_all = [torch.empty(world * n * s3, dtype=torch.float32, device="cuda") for _ in range(2)]
        gathered = [None, None]
        d_fused = [t.data_ptr() for t in t_fused]
        sn_stream = torch.cuda.ExternalStream(ctx.stream_handle(), device=torch.device("cuda", local_rank))
        comm_stream = torch.cuda.current_stream()
    else:
        d_fused = [ctx.dev_alloc(n * s3 * 4)] * 2
    step_no = [0]

    def step():
        b = step_no[0] & 1
        step_no[0] += 1
        if native:
            ctx.comm_wait(b)                                               # the all-gather that read this buffer pair two steps ago
            ctx.cvc_forward_dev(n, n_vp, d_pairs, d_xyz, d_resol, d_w, d_fused[b])
            ctx.allgather_f32_dev_overlap(d_fused[b], n * s3, d_all[b], b)   # RCCL on the context's communication stream: overlaps the next step's kernels
            return
        if use_dist and args.dist_backend == "gloo":
            ctx.cvc_forward_dev(n, n_vp, d_pairs, d_xyz, d_resol, d_w, d_fused[b])
            ctx.d2h(h_fused, d_fused[b])
            dist.all_gather_into_tensor(t_all_host, torch.from_numpy(h_fused))
            return
        if use_dist and gathered[b] is not None:
            sn_stream.wait_event(gathered[b])      # the all-gather that read this buffer two steps ago must be done first
        ctx.cvc_forward_dev(n, n_vp, d_pairs, d_xyz, d_resol, d_w, d_fused[b])
        if use_dist:
            comm_stream.wait_event(sn_stream.record_event())   # fused probabilities of this step are complete
            dist.all_gather_into_tensor(t_all[b], t_fused[b])
            gathered[b] = comm_stream.record_event()

    def barrier_sync():
        ctx.synchronize()
        if use_dist:
            if args.dist_backend == "nccl":
                torch.cuda.synchronize()
            dist.barrier()
            if args.dist_backend == "nccl":
                torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier_sync()
    # ---- the timed region: exactly K steps, per-kernel event profiling OFF ------------------------------------------
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier_sync()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        # what a caller of the timed path receives: the fused probabilities of the last step (N>1: the all-gathered ones of every rank)
        b = (step_no[0] - 1) & 1
        fused = np.empty((world * n if use_dist else n, 1, s, s, s), np.float32)
        if native:
            ctx.d2h(fused, d_all[b])
        elif use_dist and args.dist_backend == "gloo":
            fused[:] = t_all_host.numpy().reshape(fused.shape)
        elif use_dist:
            fused[:] = t_all[b].cpu().numpy().reshape(fused.shape)
        else:
            ctx.d2h(fused, d_fused[b])
        dump_outputs(args.dump_outputs, fused)
    if args.full:
        # ---- a second loop of the same K steps with HIP events around every kernel launch (on the stream they are launched on):
        # the roofline / per-kernel numbers come from here, the headline from the loop above
        ctx.profile_reset()
        ctx.profile_enable(True)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        barrier_sync()
        elapsed_prof = time.perf_counter() - t0
        prof = ctx.profile()
        ctx.profile_enable(False)

    if use_dist:
        own_elapsed = elapsed
        t = torch.tensor([elapsed], dtype=torch.float64, device=ctl_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        tl = [torch.zeros(1, dtype=torch.float64, device=ctl_dev) for _ in range(world)]
        dist.all_gather(tl, torch.tensor([own_elapsed], dtype=torch.float64, device=ctl_dev))
        per_rank_s = [round(float(x.item()), 6) for x in tl]

    if rank == 0:
        cubes_per_s = world * n * args.steps / elapsed
        out = {
            "metric": "voxel-cubes/sec (CVC warp + 3D CNN fwd) at s=%d, N_viewpair=%d" % (s, n_vp),
            "value": round(cubes_per_s, 2), "unit": "cubes/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": DTYPE[args.precision], "data": "synthetic",
            "config": {"workload": "synthetic 2-view 1600x1200, s=%d, batch=%d cubes/GPU, N_viewpair=%d (%s)" % (
                s, n, n_vp, "BASELINE.json configs[1]" if (s, n, n_vp) == (32, 64, 2) else ("one GPU's shard of BASELINE.json configs[3]: s=64, 256 cubes over 8 GPUs" if (s, n) == (64, 32) else "non-default workload")),
                       "cubes_per_gpu": n, "samples_per_step": n * n_vp * world, "parallelism": "cube-sharded x%d%s" % (world, ((", RCCL all-gather of fused probabilities" + (" (native sn_allgather_f32_dev_overlap)" if native else " (torch.distributed)")) if (native or args.dist_backend == "nccl") else ", all-gather of fused probabilities over host memory (torch.distributed gloo: shared-GPU test mode)") if world > 1 else ""),
                       **({"comm_note": comm_note} if comm_note else {}),
                       **({"dist_backend": args.dist_backend, "elapsed_s_per_rank": per_rank_s} if use_dist else {}),
                       **({"rccl": {"file": rccl_info[0], "version_code": rccl_info[1]}} if rccl_info else {})},
            "end_to_end_tflops": round(cubes_per_s / world * n_vp * CNN_FLOPS_PER_SAMPLE_S32 * (s / 32.0) ** 3 / 1e12, 2),
        }
    if rank == 0 and args.full:
        dom = max((k for k in prof if prof[k]["flops"] > 0), key=lambda k: prof[k]["ms"])
        d = prof[dom]
        ach = d["flops"] / (d["ms"] * 1e-3) / 1e12
        conv_ms = sum(v["ms"] for v in prof.values() if v["flops"] > 0)
        conv_fl = sum(v["flops"] for v in prof.values())
        cvc = prof.get("cvc_warp")
        out["roofline"] = {"bound": "mfma", "kernel": "conv3d_f16_mfma<%s>" % dom, "achieved": round(ach, 2), "peak": MFMA_F16_DENSE_PEAK_TFLOPS,
                           "unit": "TFLOP/s", "frac": round(ach / MFMA_F16_DENSE_PEAK_TFLOPS, 4), "traffic": None,
                           "avg_launch_ms": round(d["ms"] / d["launches"], 4), "launches": d["launches"],
                           "algorithmic_flops_per_launch": d["flops"] / d["launches"]}
        out["cnn_all_convs"] = {"achieved_tflops": round(conv_fl / (conv_ms * 1e-3) / 1e12, 2), "ms_per_step": round(conv_ms / args.steps, 3)}
        out["box"] = box
        if box and "sustained_f16_tflops" in box:
            out["roofline"]["frac_of_box_sustained"] = round(ach / box["sustained_f16_tflops"], 4)
        if cvc:
            # 2 views x s^3 x 3 B gathered + 6 x s^3 x 4 B of planar fp32 written per cube-view-pair = 983,040 B at s = 32. The launch
            # measured here is the FUSED form (writes conv1_1's fp16 hi/lo input instead of the planar tensor): its own traffic is `bytes_per_launch_fused_form`
            survey_bytes = (2 * 3 + 6 * 4) * s3 * n * n_vp
            t_cvc = cvc["ms"] / cvc["launches"] * 1e-3
            out["cvc_warp"] = {"bound": "hbm", "achieved_GBps": round(survey_bytes / t_cvc / 1e9, 1), "peak_GBps": 8000.0, "frac": round(survey_bytes / t_cvc / 8e12, 4),
                               "bytes_per_launch": survey_bytes, "bytes_basis": "SURVEY 8(d): 983,040 B per cube-view-pair at s=32 (planar fp32 form)",
                               "achieved_GBps_fused_form": round(cvc["bytes"] / (cvc["ms"] * 1e-3) / 1e9, 1), "bytes_per_launch_fused_form": cvc["bytes"] / cvc["launches"],
                               "avg_launch_ms": round(cvc["ms"] / cvc["launches"], 4)}
        out["kernels_ms_per_step"] = {k: round(v["ms"] / args.steps, 3) for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])}
        out["profiled_loop_ms_per_step"] = round(elapsed_prof / args.steps * 1e3, 3)     # same K steps with the per-kernel events on
        try:   # HBM-side bytes per launch measured with rocprofv3 PMC passes on this workload (tools/pmc_summary.py, tools/pmc_traffic.py);
            # the file carries the hash of the kernel sources it was measured on and is ignored when they have changed since
            pt = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
            if pt.get("kernel_src_sha16") != kernel_src_sha16():
                out["roofline"]["traffic_note"] = "profiles/pmc_traffic.json was measured on other kernel sources (sha %s != %s): dropped" % (pt.get("kernel_src_sha16"), kernel_src_sha16())
            elif pt["config"] == {"cube_D": s, "samples": n * n_vp, "precision": args.precision} and dom in pt:
                out["roofline"]["traffic"] = pt[dom]["read_bytes"] + pt[dom]["write_bytes"]
                out["roofline"]["traffic_note"] = "bytes/launch, FETCH_SIZE x2 (gfx950) + WRITE_SIZE, Infinity-Cache hits included; L2 hit rate %.2f; profiles/pmc_traffic.json" % pt[dom].get("l2_hit_rate", float("nan"))
                if cvc and "cvc_warp" in pt:
                    out["cvc_warp"]["traffic"] = pt["cvc_warp"]["read_bytes"] + pt["cvc_warp"]["write_bytes"]
        except Exception:
            pass
        out["roofline"]["note"] = ("achieved = ALGORITHMIC conv FLOPs / kernel time; the f16x3 mode issues 3 MFMA FLOPs per algorithmic "
                                   "FLOP (1.5 in the two merge layers, whose correction terms run on the MX-scaled fp6 MFMA at twice the fp16 rate; 2 in conv4_x, fp8 codes), so its ceiling is frac = 1/3 .. 2/3; peak = the nominal 2.5 PF at 2.4 GHz - a pure 16x16x32 MFMA stream sustains "
                                   "1,950-1,980 TF at 1.87 GHz on this chip (tools/probe/power_probe.hip, profiles/r4/power_probe_r4.txt)" if args.precision.startswith("f16x3") else "achieved = algorithmic conv FLOPs / kernel time")
        if world == 1 and args.precision == "f16x3" and not args.no_fast_mode:
            out["f16x3p"] = fast_mode(surfacenet_amd, scene, values, s, n, n_vp, local_rank, max(3, args.steps // 2), precision="f16x3p",
                                      note="every product on three fp16 MFMAs in every layer, f32 accumulate (no MX correction step anywhere): fp32-class "
                                           "in all 19 conv layers, L_inf vs the fp64 oracle 1e-6 .. 1e-5 (asserted < 5e-5) - same workload, same timed-loop structure; not the headline")
            out["fast_mode_f16"] = fast_mode(surfacenet_amd, scene, values, s, n, n_vp, local_rank, max(3, args.steps // 2))
        if world == 1 and s == 32 and not args.no_s64:
            out["s64"] = s64_mode(surfacenet_amd, values, n_vp, local_rank, max(3, args.steps // 2), args.precision)
        if world == 1 and not args.no_post_pass:
            out["loop_body_with_post_pass"] = post_pass(surfacenet_amd, ctx, scene, s, n, n_vp, max(3, args.steps // 2))
            # the regime of a trained net: ~1 % of the centre crop selected (a thin surface) - ray pooling then keeps its hash tables in LDS
            out["loop_body_with_post_pass_thin_surface"] = post_pass(surfacenet_amd, ctx, scene, s, n, n_vp, max(3, args.steps // 2), keep_frac=0.01)
        if world == 1 and not args.no_simil:
            out["similarity_net"] = simil_net(surfacenet_amd, ctx, scene, max(2, args.steps // 3))
        if world == 1 and s == 32 and not args.no_scenes:
            # Extra, non-headline: reconstruct_scene end to end (early rejection -> view-pair selection -> cube loop -> sparse lists) on the
            # calibration and cube grid of DTU scan9 (49 views, N_vp = 5) and Middlebury dino (16 views, 16 view pairs); synthetic views and
            # weights; a bounded even sample of each grid by default. Whole-grid runs: profiles/r2/scene_*.json (tools/bench_scene.py).
            ctx.close()
            ctx = None
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import bench_scene
            lim = ["--max-cubes", str(args.scene_cubes)] if args.scene_cubes else []
            out["scene_dtu_scan9"] = bench_scene.run(["--config", "dtu_scan9"] + lim)
            out["scene_dino"] = bench_scene.run(["--config", "dino"] + lim)
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(scene, values, s, n_vp)
    if rank == 0:
        try:   # RCCL's banner sits in the C stdio buffer: push it out first so that the JSON line is the last line of stdout
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.destroy_process_group()
    if native_hung:             # a helper thread is still stuck inside the RCCL set-up: do not wait for it at interpreter exit
        sys.stdout.flush()
        os._exit(0)
    if ctx is not None:
        ctx.close()


if __name__ == "__main__":
    main()
