"""Times the mesh self-intersection stage at DTU scale, next to the smoother's build and the orientation stage's own
kernels on the same meshes in the same run, and answers whether the default chain's meshes cross themselves.

    python tools/bench_meshintersect.py [--out profiles/meshintersect/bench_meshintersect.json] [--reps 5] [--no-ab]

Scene: the "dtu" scene of tools/bench_postpass.py as tools/bench_meshsimplify.py sets it up, meshed by sn_mesh and triangulated; the stage
runs on the mesh as extracted, after mesh.smooth_mesh(iterations=10) and after mesh.simplify_mesh(cell=2). The restatement
(tests/meshintersect_ref.py) takes its candidates from a brute-force prefilter over all triangle pairs and cannot run at a million triangles:
it is compared, byte for byte, on a crop of the 5,000 triangles nearest the mesh's centre, host and device form; on the whole mesh the host
form and the device form are compared with each other. Every time is the median of --reps runs after one warm-up:
  packed_ms / device_ms   Context.mesh_intersect on host arrays (upload, kernels, readback) / with the mesh staged in device memory by the caller
  stages_ms               the kernels alone (the context's HIP-event profile): the smoother's build (msm_*) and the stage's own mxi_tris,
                          mxi_grid, mxi_pairs, mxi_sort, mxi_count, mxi_emit; own_ms is the sum of the mxi_*
  orient_stages_ms        the orientation stage's kernels on the same mesh: the yardstick this stage is read against
  level, entries          the grid level the broad phase picks and its (cell, triangle) entries, restated in numpy
  budget_ab               stages_ms with 4, 8 (the product's) and 16 entries per triangle allowed, from the test-only twin library in child
                          processes (SN_MXI_BUDGET switches it)
No time is aimed at: the numbers are written down.

    python tools/bench_meshintersect.py --case NAME --save OUT.npz      (the tests' child: a named case of tests/meshintersect_ref.py, its
                                                                         outputs saved as they came back)
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
from bench_meshnormals import _median_stages  # noqa: E402
from bench_meshsimplify import _scene  # noqa: E402

BUDGETS = (4, 8, 16)


def _meshes(ctx):
    from surfacenet_amd import mesh
    _, m, origin, resol, counts = _scene(ctx)
    lat = np.ascontiguousarray(m["verts_lattice"], dtype=np.float64)
    quads = np.ascontiguousarray(m["quads"], dtype=np.int32)
    tris = np.ascontiguousarray(mesh.triangulate(quads), dtype=np.int32)
    smooth = mesh.smooth_mesh(lat, quads, iterations=10, origin=origin, resol=resol)
    simple = mesh.simplify_mesh(lat, tris, 2, origin=origin, resol=resol)
    meshes = dict(extracted=(lat, tris), smoothed_10=(np.ascontiguousarray(smooth["vert_lattice"]), tris),
                  simplified_2=(np.ascontiguousarray(simple["vert_lattice"]), np.ascontiguousarray(simple["faces"], dtype=np.int32)))
    return meshes, resol, counts


def _level(lat, f, budget=8):
    """The broad phase's level and entries, in numpy (tests/meshintersect_ref.grid_level states it triangle by triangle)."""
    q = np.rint(lat * 65536.0).astype(np.int64)
    c = q[f]                                                    # (F,3,3)
    n = np.cross((c[:, 1] - c[:, 0]).astype(np.float64), (c[:, 2] - c[:, 0]).astype(np.float64))
    live = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2]) & (n != 0).any(axis=1)
    lo, hi = (c.min(axis=1)[live] >> 16) + 4, (c.max(axis=1)[live] >> 16) + 4
    for s in range(22):
        total = int(np.prod(((hi >> s) - (lo >> s) + 1).astype(np.float64), axis=1).sum())
        if total <= budget * int(live.sum()) or s == 21:
            return s, total, int(live.sum())


def _own(ctx, lat, f, reps):
    stages = _median_stages(ctx, lambda: ctx.mesh_intersect(lat, f), reps, "m")
    return {k: v for k, v in stages.items() if k.startswith("mxi_") or k.startswith("msm_")}


def _crop(lat, f, n=5000):
    centre = lat[np.unique(f)].mean(axis=0)
    d = np.linalg.norm(lat[f].mean(axis=1) - centre, axis=1)
    return np.ascontiguousarray(f[np.sort(np.argsort(d, kind="stable")[:n])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshintersect", "bench_meshintersect.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stages-only", action="store_true", help="print the stages' times of the three meshes as one JSON line and stop (the A/B's child)")
    ap.add_argument("--no-ab", action="store_true")
    ap.add_argument("--case", help="run a named case of tests/meshintersect_ref.py (the tests' child)")
    ap.add_argument("--save", help="... and save its outputs here")
    args = ap.parse_args()
    import meshintersect_ref as ref
    from surfacenet_amd import runtime
    ctx = runtime.any_context()
    if args.case:
        got = ctx.mesh_intersect(*ref.CASES[args.case]())
        np.savez(args.save, **{k: got[k] for k in ref.KEYS})
        return
    meshes, resol, counts = _meshes(ctx)
    if args.stages_only:
        print(json.dumps({name: _own(ctx, lat, f, args.reps) for name, (lat, f) in meshes.items()}))
        return
    res = dict(tool="tools/bench_meshintersect.py", resol=resol, reps=args.reps, meshes={}, **counts)
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
        level, entries, live = _level(lat, f)
        row.update(level=level, entries=entries, entries_per_triangle=entries / max(live, 1))
        run = lambda **kw: ctx.mesh_intersect(lat, f, **kw)
        got, dev = run(), run(device=True)
        differs = [k for k in ref.KEYS if got[k].tobytes() != dev[k].tobytes()]
        if differs:
            raise SystemExit("%s: the host form and the device form differ on %s" % (name, differs))
        row.update(forms_equal=True, **dict(zip(ref.COUNTS, (int(x) for x in got["counts"]))))
        row["first_pairs"] = got["pairs"][:8].tolist()
        if got["pairs"].shape[0]:                               # where: the lattice cells of the hit faces' centroids, their bounding box
            cen = lat[f[np.flatnonzero(got["face_hit"])]].mean(axis=1)
            row["hit_box_cells"] = [cen.min(axis=0).tolist(), cen.max(axis=0).tolist()]
        crop = _crop(lat, f)
        t = time.perf_counter()
        want = ref.intersect(lat, crop)
        row["crop"] = dict(faces=int(crop.shape[0]), restatement_ms=1e3 * (time.perf_counter() - t), pairs=int(want["counts"][3]))
        bad = ref.same_bytes(ctx.mesh_intersect(lat, crop), want) + ref.same_bytes(ctx.mesh_intersect(lat, crop, device=True), want)
        if bad:
            raise SystemExit("%s: the GPU result differs from the restatement on the crop's %s" % (name, bad))
        row["crop"]["gpu_equal"] = True
        row["crop"]["gpu_packed_ms"] = _median_time(lambda: ctx.mesh_intersect(lat, crop), args.reps)
        row["restatement"] = "cannot run at this size: its prefilter is brute force over all triangle pairs; compared on the crop"
        row["packed_ms"] = _median_time(run, args.reps)
        row["device_ms"] = _median_time(lambda: run(device=True), args.reps)
        stages = _own(ctx, lat, f, args.reps)
        row.update(kernel_ms=float(sum(stages.values())), own_ms=float(sum(v for k, v in stages.items() if k.startswith("mxi_"))), stages_ms=stages)
        orient = _median_stages(ctx, lambda: ctx.mesh_orient(lat, f, 1), args.reps, "m")
        row["orient_stages_ms"] = {k: v for k, v in orient.items() if k.startswith("mor_") or k.startswith("msm_")}
        row["orient_own_ms"] = float(sum(v for k, v in orient.items() if k.startswith("mor_")))
        row["build_ms"] = float(sum(v for k, v in stages.items() if k.startswith("msm_")))
        save()
    if not args.no_ab:
        dbg = os.path.join(ROOT, "surfacenet_amd", "libsurfacenet_hip_dbg.so")
        res["budget_ab"] = {}
        for budget in BUDGETS:
            env = dict(os.environ, SURFACENET_HIP_LIB=dbg, SN_MXI_BUDGET=str(budget))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--stages-only", "--reps", str(args.reps)], env=env, capture_output=True,
                                 text=True, timeout=600)
            res["budget_ab"][str(budget)] = json.loads(out.stdout.strip().splitlines()[-1]) if out.returncode == 0 else "failed: %s" % out.stderr[-300:]
            res["budget_ab"]["levels_%d" % budget] = {name: _level(lat, f, budget)[:2] for name, (lat, f) in meshes.items()}
        save()
    print(json.dumps(dict(budget_ab=res.get("budget_ab"), meshes=res["meshes"]), default=float))


if __name__ == "__main__":
    main()
