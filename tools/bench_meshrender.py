"""Times the mesh renderer at DTU scale: the synthetic shell mesh of tools/bench_meshorient.py into 1200 x 1600 for
1, 8 and 49 views, without and with one image-filling triangle added.

    python tools/bench_meshrender.py [--out profiles/meshrender/bench_meshrender.json] [--reps 3] [--no-restatement]

Scene: the "dtu" scene of tools/bench_postpass.py as tools/bench_meshsimplify.py sets it up, meshed by sn_mesh and triangulated, in world
mm; 49 cameras at the positions that scene's normals were oriented with, each looking at the mesh's centre with a focal length that holds
the mesh in the image. The filler is one triangle under the whole scene, far larger than any view's frustum: every pixel of every view it
adds is covered by it, through the path of the big triangles. Before anything is reported the GPU result of view 0, host form and device
form, is compared with the restatement (tests/meshrender_ref.py, fed sn_project_points' h, w, z) byte for byte. Every time is the median of
--reps calls after one warm-up, from the context's HIP-event profile, divided by the number of views:
  stages_ms_per_view   mrd_clear (the memsets), mrd_project, mrd_setup, mrd_raster_small, mrd_raster_big, mrd_ids_small, mrd_ids_big,
                       mrd_resolve, mrd_visible
  hbm                  the bytes a view's z-buffer clear, resolve and outputs must move - 12 per pixel cleared, 12 read and 12 written by the
                       resolve, 4 per face of face_pixels - over the time of mrd_clear + mrd_resolve: the figure to judge the resolve by
  pairs_per_s          covering (triangle, pixel) pairs per second of the two depth passes (the id passes walk the same pairs again)
  restatement_ms       tests/meshrender_ref.py for ONE view on the same input: the CPU baseline
  filler_ratio         kernel time per view with the filler over the time without it, per number of views; above 2 the tool names the stage
                       that took the difference
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

from bench_meshnormals import _median_stages  # noqa: E402  (tools/ is on the path when this file is run as a script)
from bench_meshsimplify import _scene  # noqa: E402

SHAPE = (1200, 1600)
VIEWS = (1, 8, 49)


def _cameras(verts, n_views, shape):
    """n_views pinhole cameras at the scene's camera positions (bench_meshsimplify._scene draws them the same way), each looking at the
    mesh's centre, the mesh's bounding sphere inside the shorter image side."""
    rs = np.random.RandomState(3)
    pos = np.stack([rs.uniform(-100, 300, n_views), rs.uniform(-100, 300, n_views), rs.uniform(500, 700, n_views)], axis=1)
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    centre, radius = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2
    P = []
    for c in pos:
        fwd = (centre - c) / np.linalg.norm(centre - c)
        right = np.cross(fwd, [0.0, 1.0, 0.0])
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd])
        foc = 0.5 * min(shape) * np.linalg.norm(centre - c) / radius
        K = np.asarray([[foc, 0, (shape[1] - 1) / 2], [0, foc, (shape[0] - 1) / 2], [0, 0, 1.0]])
        P.append(K @ np.concatenate([R, (-R @ c)[:, None]], axis=1))
    return np.ascontiguousarray(np.stack(P))


def _with_filler(verts, faces, P):
    """The mesh plus one triangle under the whole scene (smaller z: the cameras look down from z = 500 .. 700) whose inscribed circle is 2.5
    bounding spheres wide: it holds every view's footprint. Nothing is clipped at the camera plane, so its corners must lie in front of every
    camera: checked here."""
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    c, R = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2
    z = lo[2] - 0.1 * R
    extra = np.asarray([(c[0] + 5 * R * np.cos(a), c[1] + 5 * R * np.sin(a), z) for a in np.deg2rad([90.0, 210.0, 330.0])])
    depth = np.einsum("vj,nj->vn", P[:, 2, :3], extra) + P[:, 2, 3:4]
    if depth.min() <= 0:
        raise SystemExit("the filler has a corner behind a camera (depth %g): it would be clipped whole" % depth.min())
    n = verts.shape[0]
    return np.concatenate([verts, extra]), np.ascontiguousarray(np.concatenate([faces, [[n, n + 1, n + 2]]]).astype(np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshrender", "bench_meshrender.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-restatement", action="store_true", help="skip the numpy baseline and the comparison with it (minutes at this size)")
    args = ap.parse_args()
    import meshrender_ref as ref
    from surfacenet_amd import mesh, runtime
    ctx = runtime.any_context()
    _, m, origin, resol, counts = _scene(ctx)
    verts = np.ascontiguousarray(m["verts_mm"], dtype=np.float64)
    tris = np.ascontiguousarray(mesh.triangulate(m["quads"]), dtype=np.int32)
    P = _cameras(verts, max(VIEWS), SHAPE)
    meshes = dict(shell=(verts, tris), shell_with_filler=_with_filler(verts, tris, P))
    H, W = SHAPE
    tol = 0.5 * resol
    res = dict(tool="tools/bench_meshrender.py", shape=list(SHAPE), resol=resol, tol=tol, reps=args.reps, small_box=ref.SMALL_BOX, meshes={}, **counts)
    try:
        res["box_probe"] = ctx.mfma_probe()
    except Exception as e:             # noqa: BLE001 - the probe only labels the box
        res["box_probe"] = "unavailable: %s" % e

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, default=float)

    for name, (v, f) in meshes.items():
        row = res["meshes"][name] = dict(faces=int(f.shape[0]), vertices=int(v.shape[0]), views={})
        if not args.no_restatement:
            h, w, z = ctx.project(v, P[:1], return_int_hw=False, return_depth=True)
            print("%s: the restatement of one view of %d triangles ..." % (name, f.shape[0]), flush=True)
            t = time.perf_counter()
            want = ref.render(h, w, z, f, H, W, 0.0, tol)
            row["restatement_ms"] = 1e3 * (time.perf_counter() - t)
            differs = ref.same_bytes(ctx.mesh_render(v, f, P[:1], SHAPE, 0.0, tol), want) + ref.same_bytes(ctx.mesh_render(v, f, P[:1], SHAPE, 0.0, tol, device=True), want)
            if differs:
                raise SystemExit("%s: the GPU result differs from the restatement on %s" % (name, differs))
            row.update(gpu_equal=True, view0=dict(zip(ref.COUNTS[:7], (int(x) for x in want["counts"][:7]))), view0_max_cover=int(want["cover"].max()))
            del want
        for V in VIEWS:
            print("%s: %d views ..." % (name, V), flush=True)
            got = ctx.mesh_render(v, f, P[:V], SHAPE, 0.0, tol, device=True)
            c = dict(zip(ref.COUNTS[:7], (int(x) for x in got["counts"][:7])))
            del got
            stages = _median_stages(ctx, lambda: ctx.mesh_render(v, f, P[:V], SHAPE, 0.0, tol, device=True), args.reps, "mrd_")
            per_view = {k: ms / V for k, ms in stages.items() if k != "mrd_check"}
            kernel = float(sum(per_view.values()))
            moved = H * W * (12.0 + 12.0 + 12.0) + 4.0 * f.shape[0]
            hbm_ms = per_view["mrd_clear"] + per_view["mrd_resolve"]
            depth_ms = per_view.get("mrd_raster_small", 0.0) + per_view.get("mrd_raster_big", 0.0)
            row["views"][str(V)] = dict(counts=c, stages_ms_per_view=per_view, check_ms=stages.get("mrd_check", 0.0), kernel_ms_per_view=kernel,
                                        hbm=dict(bytes_per_view=moved, ms=hbm_ms, GB_per_s=moved / hbm_ms / 1e6),
                                        pairs_per_view=c["n_pairs"] / V, pairs_per_s=c["n_pairs"] / V / (depth_ms * 1e-3))
            save()
    ratio = res["filler_ratio"] = {}
    for V in VIEWS:
        a, b = res["meshes"]["shell"]["views"][str(V)], res["meshes"]["shell_with_filler"]["views"][str(V)]
        r = ratio[str(V)] = dict(ratio=b["kernel_ms_per_view"] / a["kernel_ms_per_view"])
        if r["ratio"] > 2:
            diff = {k: b["stages_ms_per_view"][k] - a["stages_ms_per_view"].get(k, 0.0) for k in b["stages_ms_per_view"]}
            r["stage_that_took_the_time"] = max(diff, key=diff.get)
            r["its_ms_per_view"] = diff[r["stage_that_took_the_time"]]
    save()
    print(json.dumps(dict(filler_ratio=ratio, meshes={k: dict(faces=row["faces"], restatement_ms=row.get("restatement_ms"), gpu_equal=row.get("gpu_equal"),
                                                              views={V: dict(kernel_ms_per_view=x["kernel_ms_per_view"], stages_ms_per_view=x["stages_ms_per_view"],
                                                                             hbm_GB_per_s=x["hbm"]["GB_per_s"], pairs_per_s=x["pairs_per_s"], counts=x["counts"])
                                                                     for V, x in row["views"].items()}) for k, row in res["meshes"].items()}), default=float))


if __name__ == "__main__":
    main()
