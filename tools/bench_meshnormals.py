"""Times the mesh's own normals, area and volume at DTU scale, next to the smoother's adjacency build on the same mesh in
the same run.

    python tools/bench_meshnormals.py [--out profiles/meshnormals/bench_meshnormals.json] [--reps 5]

Scene: the "dtu" scene of tools/bench_postpass.py as tools/bench_meshsimplify.py sets it up, meshed by sn_mesh; the stage runs on its quads and
on their triangulation. Before anything is reported the GPU result is compared with the restatement (tests/meshnormals_ref.py) on the whole
mesh, byte for byte. Every time is the median of --reps runs after one warm-up:
  packed_ms / device_ms   Context.mesh_normals on host arrays (upload, kernels, readback) / with the mesh staged in device memory by the caller
  kernel_ms, stages_ms    the kernels alone (the context's HIP-event profile) and their split: mnr_faces (clear the sums, the face kernel),
                          mnr_verts
  restatement_ms          tests/meshnormals_ref.py on the same mesh (Python integers)
  smooth_build_ms         the smoother's adjacency build (msm_mark + msm_edges + msm_degree + msm_rows of a 1-iteration call): its face kernel
                          is bound by atomics too
  atomics                 per corner and axis the face kernel sends a low-word atomic unless the addend is 0, and a high-word atomic unless the
                          high addend with the carry is 0. In a given order of arrival the high word is needed exactly when the vertex's
                          running sum changes sign (sums below 2^63 in magnitude, as here): counted for the FACE order from the restatement's
                          face vectors. The device's order of arrival differs from run to run; the count of carries per word does not
No time is aimed at: the numbers are written down.
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

from bench_mesh import _median_time  # noqa: E402  (tools/ is on the path when this file is run as a script)
from bench_meshsimplify import _scene  # noqa: E402

BUILD = ("msm_mark", "msm_edges", "msm_degree", "msm_rows")


def _median_stages(ctx, fn, reps, prefix):
    """-> {stage: median over reps of its time in one call}."""
    fn()
    runs = []
    for _ in range(reps):
        ctx.profile_enable(True)
        ctx.profile_reset()
        fn()
        prof = ctx.profile()
        ctx.profile_enable(False)
        ctx.profile_reset()
        runs.append({k: v["ms"] for k, v in prof.items() if k.startswith(prefix)})
    return {k: float(np.median([r[k] for r in runs])) for k in runs[0]}


def _atomics_in_face_order(N_f, faces):
    """The face kernel's atomics when the corners arrive in face order: N_f (F,3) Python ints, faces (F,nv)."""
    nv = faces.shape[1]
    assert max(abs(x) for row in N_f.tolist() for x in row).bit_length() < 50      # (sums of at most 2^12 of them stay inside int64)
    n = np.repeat(N_f.astype(np.int64), nv, axis=0)                                # one row per corner, in face order
    vert = faces.reshape(-1).astype(np.int64)
    order = np.argsort(vert, kind="stable")
    vert, n = vert[order], n[order]
    after = np.cumsum(n, axis=0)
    first = np.r_[True, vert[1:] != vert[:-1]]
    start = np.flatnonzero(first)
    carried = np.r_[np.zeros((1, 3), np.int64), after[start[1:] - 1]]      # what the vertices before each one added up to
    after = after - carried[np.cumsum(first) - 1]                           # the running sum of each vertex
    before = after - n
    nonzero = n != 0
    high = nonzero & ((before < 0) != (after < 0))
    corners = int(n.size)
    return dict(corner_axis_pairs=corners, zero_addends_no_atomic=int(corners - nonzero.sum()), low_word_atomics=int(nonzero.sum()),
                high_word_atomics=int(high.sum()), high_word_atomics_skipped=int(nonzero.sum() - high.sum()),
                share_of_high_word_atomics_skipped=float(1.0 - high.sum() / max(int(nonzero.sum()), 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshnormals", "bench_meshnormals.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import meshnormals_ref
    import meshsmooth_ref
    from surfacenet_amd import mesh, runtime
    ctx = runtime.any_context()
    _, m, origin, resol, counts = _scene(ctx)
    lat = np.ascontiguousarray(m["verts_lattice"], dtype=np.float64)
    faces = dict(quads=np.ascontiguousarray(m["quads"], dtype=np.int32), triangles=np.ascontiguousarray(mesh.triangulate(m["quads"]), dtype=np.int32))
    lam, mu = meshsmooth_ref.q16(0.5), meshsmooth_ref.q16(-0.53)
    res = dict(tool="tools/bench_meshnormals.py", resol=resol, reps=args.reps, vertices=int(lat.shape[0]), meshes={}, **counts)
    try:
        res["box_probe"] = ctx.mfma_probe()
    except Exception as e:             # noqa: BLE001 - the probe only labels the box
        res["box_probe"] = "unavailable: %s" % e

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, default=float)

    for name, f in faces.items():
        row = res["meshes"][name] = dict(faces=int(f.shape[0]))
        run = lambda **kw: ctx.mesh_normals(lat, f, **kw)
        t = time.perf_counter()
        want = meshnormals_ref.normals(lat, f)
        row["restatement_ms"] = 1e3 * (time.perf_counter() - t)
        differs = meshnormals_ref.same_bytes(run(), want) + meshnormals_ref.same_bytes(run(device=True), want)
        if differs:
            raise SystemExit("%s: the GPU result differs from the restatement on %s" % (name, differs))
        c = [int(x) for x in want["counts"]]
        row.update(gpu_equal=True, zero_faces=c[0], zero_vertices=c[1], referenced=c[2], triangles=c[3], area2=str(want["area2"]), vol6=str(want["vol6"]),
                   area_mm2=want["area2"] / 2 / 2 ** 32 * resol ** 2, volume_mm3=want["vol6"] / 6 / 2 ** 48 * resol ** 3,
                   face_vector_bits=max(abs(x) for r in want["N_f"].tolist() for x in r).bit_length(),
                   atomics_face_order=_atomics_in_face_order(want["N_f"], f))
        del want
        row["packed_ms"] = _median_time(run, args.reps)
        row["device_ms"] = _median_time(lambda: run(device=True), args.reps)
        stages = _median_stages(ctx, run, args.reps, "mnr_")
        row.update(kernel_ms=float(sum(stages.values())), stages_ms=stages)
        smooth = _median_stages(ctx, lambda: ctx.mesh_smooth(lat, f, 1, lam, mu, 1, origin=origin, resol=resol), args.reps, "msm_")
        row.update(smooth_build_ms=float(sum(smooth.get(k, 0.0) for k in BUILD)), smooth_stages_ms=smooth)
        row["ratio_to_smooth_build"] = row["kernel_ms"] / row["smooth_build_ms"]
        save()
    print(json.dumps(dict(vertices=res["vertices"],
                          meshes={k: {a: b for a, b in row.items() if a in ("faces", "packed_ms", "device_ms", "kernel_ms", "stages_ms", "restatement_ms",
                                                                            "smooth_build_ms", "ratio_to_smooth_build", "atomics_face_order")}
                                  for k, row in res["meshes"].items()}), default=float))


if __name__ == "__main__":
    main()
