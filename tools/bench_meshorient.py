"""Times the mesh orientation stage at DTU scale, next to the smoother's adjacency build on the same mesh in the same run.

    python tools/bench_meshorient.py [--out profiles/meshorient/bench_meshorient.json] [--reps 5]

Scene: the "dtu" scene of tools/bench_postpass.py as tools/bench_meshsimplify.py sets it up, meshed by sn_mesh and triangulated; the stage runs
on the mesh untouched and with half its faces reversed (default_rng(5).random(F) < 0.5), sign "outward" - and, because that mesh falls into tens
of thousands of pieces, on a flat sheet of as many triangles in ONE piece, half its faces reversed the same way. Before anything is reported the GPU
result is compared with the restatement (tests/meshorient_ref.py) on the whole mesh, byte for byte, host and device form. Every time is the
median of --reps runs after one warm-up:
  packed_ms / device_ms   Context.mesh_orient on host arrays (upload, kernels, readback) / with the mesh staged in device memory by the caller
  kernel_ms, stages_ms    the kernels alone (the context's HIP-event profile) and their split: the smoother's build (msm_mark, msm_edges,
                          msm_degree) and the stage's own mor_sides, mor_links, mor_faces, mor_pieces, mor_emit; own_ms is the sum of the mor_*
  restatement_ms          tests/meshorient_ref.py on the same mesh
  smooth_build_ms         the smoother's adjacency build (msm_mark + msm_edges + msm_degree + msm_rows of a 1-iteration call): the yardstick
  reduce_ab               stages_ms with the workgroup's LDS reduction of a one-piece workgroup (the product's) and with every lane sending
                          its own atomics, both from the test-only twin library in child processes (SN_MOR_NO_REDUCE switches it)
No time is aimed at: the numbers are written down.
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

from bench_mesh import _median_time  # noqa: E402  (tools/ is on the path when this file is run as a script)
from bench_meshnormals import BUILD, _median_stages  # noqa: E402
from bench_meshsimplify import _scene  # noqa: E402

OUTWARD = 1


def _meshes(ctx):
    import meshorient_ref
    from surfacenet_amd import mesh
    _, m, origin, resol, counts = _scene(ctx)
    lat = np.ascontiguousarray(m["verts_lattice"], dtype=np.float64)
    tris = np.ascontiguousarray(mesh.triangulate(m["quads"]), dtype=np.int32)
    rev = np.random.default_rng(5).random(tris.shape[0]) < 0.5
    meshes = dict(untouched=(lat, tris), half_reversed=(lat, np.ascontiguousarray(meshorient_ref.reversed_where(tris, rev))))
    # the scene's mesh falls into tens of thousands of pieces: the one giant piece, of the same size, is a flat sheet of n x n cells
    n = int(np.sqrt(tris.shape[0] / 2))
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    sheet = np.stack([10.0 + i, 10.0 + j, 7.0 + 0.25 * ((i + j) % 3)], axis=-1).reshape(-1, 3)
    a = ((n + 1) * i + j)[:-1, :-1].reshape(-1)
    quads = np.stack([a, a + 1, a + n + 2, a + n + 1], axis=1)
    st = np.ascontiguousarray(mesh.triangulate(quads), dtype=np.int32)
    rev = np.random.default_rng(5).random(st.shape[0]) < 0.5
    meshes["one_piece_half_reversed"] = (sheet, np.ascontiguousarray(meshorient_ref.reversed_where(st, rev)))
    return meshes, origin, resol, counts


def _stages(ctx, lat, f, reps):
    stages = _median_stages(ctx, lambda: ctx.mesh_orient(lat, f, OUTWARD), reps, "m")
    return {k: v for k, v in stages.items() if k.startswith("mor_") or k.startswith("msm_")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshorient", "bench_meshorient.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stages-only", action="store_true", help="print the stages' times of both meshes as one JSON line and stop (the A/B's child)")
    ap.add_argument("--no-ab", action="store_true")
    args = ap.parse_args()
    import meshorient_ref
    import meshsmooth_ref
    from surfacenet_amd import runtime
    ctx = runtime.any_context()
    meshes, origin, resol, counts = _meshes(ctx)
    if args.stages_only:
        print(json.dumps({name: _stages(ctx, lat, f, args.reps) for name, (lat, f) in meshes.items()}))
        return
    lam, mu = meshsmooth_ref.q16(0.5), meshsmooth_ref.q16(-0.53)
    res = dict(tool="tools/bench_meshorient.py", resol=resol, reps=args.reps, vertices=int(meshes["untouched"][0].shape[0]), sign="outward", meshes={}, **counts)
    try:
        res["box_probe"] = ctx.mfma_probe()
    except Exception as e:             # noqa: BLE001 - the probe only labels the box
        res["box_probe"] = "unavailable: %s" % e

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, default=float)

    for name, (lat, f) in meshes.items():
        row = res["meshes"][name] = dict(faces=int(f.shape[0]), vertices=int(lat.shape[0]))
        run = lambda **kw: ctx.mesh_orient(lat, f, OUTWARD, **kw)
        t = time.perf_counter()
        want = meshorient_ref.orient(lat, f, OUTWARD)
        row["restatement_ms"] = 1e3 * (time.perf_counter() - t)
        differs = meshorient_ref.same_bytes(run(), want) + meshorient_ref.same_bytes(run(device=True), want)
        if differs:
            raise SystemExit("%s: the GPU result differs from the restatement on %s" % (name, differs))
        row.update(gpu_equal=True, **dict(zip(meshorient_ref.COUNTS, (int(x) for x in want["counts"]))))
        sizes = np.sort(want["comp_faces"][want["comp_faces"] > 0])[::-1]
        row.update(largest_pieces=[int(x) for x in sizes[:5]], closed_volume_mm3=[
            want["vol6"][int(i)] / 6 / 2 ** 48 * resol ** 3 for i in np.flatnonzero(want["comp_flags"] & meshorient_ref.CLOSED)[:5]])
        del want
        row["packed_ms"] = _median_time(run, args.reps)
        row["device_ms"] = _median_time(lambda: run(device=True), args.reps)
        stages = _stages(ctx, lat, f, args.reps)
        row.update(kernel_ms=float(sum(stages.values())), own_ms=float(sum(v for k, v in stages.items() if k.startswith("mor_"))), stages_ms=stages)
        smooth = _median_stages(ctx, lambda: ctx.mesh_smooth(lat, f, 1, lam, mu, 1, origin=origin, resol=resol), args.reps, "msm_")
        row.update(smooth_build_ms=float(sum(smooth.get(k, 0.0) for k in BUILD)), smooth_stages_ms=smooth)
        row["ratio_to_smooth_build"] = row["kernel_ms"] / row["smooth_build_ms"]
        row["own_ratio_to_smooth_build"] = row["own_ms"] / row["smooth_build_ms"]
        save()
    if not args.no_ab:
        dbg = os.path.join(ROOT, "surfacenet_amd", "libsurfacenet_hip_dbg.so")
        res["reduce_ab"] = {}
        for label, extra in (("lds_reduce", {}), ("per_lane", {"SN_MOR_NO_REDUCE": "1"})):
            env = {k: v for k, v in os.environ.items() if k != "SN_MOR_NO_REDUCE"}
            env.update(SURFACENET_HIP_LIB=dbg, **extra)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--stages-only", "--reps", str(args.reps)], env=env, capture_output=True,
                                 text=True, timeout=300)
            res["reduce_ab"][label] = json.loads(out.stdout.strip().splitlines()[-1]) if out.returncode == 0 else "failed: %s" % out.stderr[-300:]
        save()
    print(json.dumps(dict(vertices=res["vertices"], reduce_ab=res.get("reduce_ab"),
                          meshes={k: {a: b for a, b in row.items() if a not in ("smooth_stages_ms",)} for k, row in res["meshes"].items()}), default=float))


if __name__ == "__main__":
    main()
