"""Times the mesh voxelisation stage on the tools/bench_postpass.py scene, next to what a user had before it, in the
same run.

    python tools/bench_meshvoxel.py [--out profiles/meshvoxel/bench_meshvoxel.json] [--reps 5] [--cubes 1024]

Scene: the "dtu" scene of tools/bench_postpass.py as tools/bench_meshsimplify.py sets it up, meshed by sn_mesh, in lattice cells; the stage
runs on the mesh as extracted (quads) and after the chain fill 64, smooth 10, orient outward, into the scene's own cubes (the first --cubes
of them that a triangle's box reaches: the comparison's centres are held in host memory). Every time is the median of --reps runs after one
warm-up:
  device_ms / stages_ms   Context.mesh_voxelize with mesh and cubes staged in device memory (occ and Y) / the kernels alone (the context's
                          HIP-event profile): vox_check, vox_tris, vox_grid, vox_cubes, vox_emit; solid_only and surface_only the same with
                          modes 1 and 2
  pairs, tests            counts[6], counts[7]: (column, triangle) pairs covered, (voxel, triangle) box tests run
  winding_ms              what gave the solid bit before: Context.mesh_winding(device=True) on all N D^3 centres, winding only; its kernels
                          in winding_stages_ms. The solid bit must equal winding != 0 byte for byte, or the tool fails
  surface_target          what gave a surface target before: mesh.sample_surface(dst 0.5 cell) + groundTruth.gt_cubes_from_points, beside
                          the stage's surface mode, both into cubes of 32 voxels at the same corners (the ground-truth mode runs at a
                          context's own cube side). The semantics differ - a voxel is set when a SAMPLE falls into it - so both
                          occupancies are written down, not compared
No time is aimed at: the numbers are written down.

    python tools/bench_meshvoxel.py --case NAME --axis A --save OUT.npz      (the tests' child: a named case of tests/meshvoxel_ref.py, its
                                                                              outputs saved as they came back)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_mesh import _median_time  # noqa: E402  (tools/ is on the path when this file is run as a script)
from bench_meshnormals import _median_stages  # noqa: E402
from bench_meshsimplify import _scene  # noqa: E402

DC, STRIDE = 26, 13                                              # the scene's cube side and stride (tools/bench_meshsimplify.py _scene)
GT_D = 32                                                        # the cube side of the surface-target comparison: a context's own


def _meshes(ctx):
    from surfacenet_amd import mesh, synthetic
    _, m, origin, resol, counts = _scene(ctx)
    m = dict(vertices=m["verts_mm"], quads=m["quads"], vert_src=m["vert_src"], vert_lattice=m["verts_lattice"])
    chain = mesh.run_chain(m, mesh.chain_settings(mesh_fill=64, mesh_smooth=10, mesh_orient="outward"), origin, resol)
    last = chain["oriented"]
    cube_ijk = synthetic.sparse_surface((40, 40, 14), DC, speck_rate=0.0005, seed=1, thickness=1, amplitude=60.0)["cube_ijk_np"]
    meshes = dict(extracted=(np.ascontiguousarray(m["vert_lattice"], np.float64), np.ascontiguousarray(m["quads"], np.int32)),
                  chain=(np.ascontiguousarray(last["vert_lattice"], np.float64), np.ascontiguousarray(mesh._faces(last), np.int32)))
    return meshes, np.ascontiguousarray(cube_ijk, np.int32), origin, resol, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshvoxel", "bench_meshvoxel.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cubes", type=int, default=1024)
    ap.add_argument("--case", help="run a named case of tests/meshvoxel_ref.py (the tests' child)")
    ap.add_argument("--axis", type=int, default=2)
    ap.add_argument("--save", help="... and save its outputs here")
    args = ap.parse_args()
    import meshvoxel_ref as ref
    from surfacenet_amd import groundTruth, mesh, runtime
    ctx = runtime.any_context()
    if args.case:
        v, f, cube, D, stride = ref.CASES[args.case]()
        got = ctx.mesh_voxelize(v, f, cube, D, stride, axis=args.axis)
        np.savez(args.save, **{k: got[k] for k in ref.KEYS})
        return
    meshes, cube_all, origin, resol, counts = _meshes(ctx)
    res = dict(tool="tools/bench_meshvoxel.py", resol=resol, reps=args.reps, D=DC, stride=STRIDE, meshes={}, **counts)
    try:
        res["box_probe"] = ctx.mfma_probe()
    except Exception as e:             # noqa: BLE001 - the probe only labels the box
        res["box_probe"] = "unavailable: %s" % e

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, default=float)

    for name, (v, f) in meshes.items():
        row = res["meshes"][name] = dict(faces=int(f.shape[0]), nv=int(f.shape[1]), vertices=int(v.shape[0]))
        used = v[np.unique(f)]
        lo, hi = np.floor(used.min(axis=0)) - 1, np.ceil(used.max(axis=0)) + 1
        near = ((cube_all * STRIDE + DC - 1 >= lo) & (cube_all * STRIDE <= hi)).all(axis=1)
        cube = np.ascontiguousarray(cube_all[near][:args.cubes])
        N = cube.shape[0]
        row.update(cubes=N, voxels=N * DC ** 3)
        run = lambda **kw: ctx.mesh_voxelize(v, f, cube, DC, STRIDE, device=True, **kw)
        got, host = run(), ctx.mesh_voxelize(v, f, cube, DC, STRIDE)
        differs = ref.same_bytes(got, host) + [k for k in ("counts",) if got[k].tobytes() != host[k].tobytes()]
        if differs:
            raise SystemExit("%s: the host form and the device form differ on %s" % (name, differs))
        row.update(forms_equal=True, **dict(zip(ref.COUNTS, (int(x) for x in got["counts"]))))
        row["device_ms"] = _median_time(lambda: run(outputs=("occ", "Y")), args.reps)
        stages = _median_stages(ctx, lambda: run(outputs=("occ", "Y")), args.reps, "vox_")
        row.update(kernel_ms=float(sum(stages.values())), stages_ms=stages)
        for key, modes in (("solid_only", 1), ("surface_only", 2)):
            st = _median_stages(ctx, lambda: run(modes=modes, select=modes, outputs=("occ",)), args.reps, "vox_")
            row[key] = dict(kernel_ms=float(sum(st.values())), stages_ms=st)
        # what gave the solid bit before: the winding number of every centre
        a = np.arange(DC, dtype=np.float64)
        local = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(1, -1, 3)
        centres = np.ascontiguousarray((cube.astype(np.float64)[:, None, :] * STRIDE + local).reshape(-1, 3))
        wnd = lambda: ctx.mesh_winding(v, f, centres, outputs=("winding",), device=True)
        inside = (wnd()["winding"] != 0).astype(np.uint8).reshape(N, DC, DC, DC)
        if inside.tobytes() != (got["occ"] & 1).tobytes():
            raise SystemExit("%s: the solid bit differs from winding != 0 on %d voxels" % (name, int((inside != (got["occ"] & 1)).sum())))
        row["solid_equals_winding"] = True
        row["winding_ms"] = _median_time(wnd, args.reps)
        ws = _median_stages(ctx, wnd, args.reps, "wnd_")
        row.update(winding_kernel_ms=float(sum(ws.values())), winding_stages_ms=ws)
        # what gave a surface target before: samples of the mesh into gt_cubes. The ground-truth mode runs at a context's own cube side,
        # so this comparison is made in cubes of GT_D voxels at the same corners
        tris = np.ascontiguousarray(mesh.triangulate(f) if f.shape[1] == 4 else f, np.int32)
        xyz = (np.asarray(origin, np.float64) + (cube.astype(np.float64) * STRIDE - 0.5) * resol).astype(np.float32)      # a voxel's box starts half a cell before its centre
        params = (xyz, np.full((N,), resol, np.float32))

        def sample_gt():
            pts, _ = mesh.sample_surface(v, tris, 0.5)
            return groundTruth.gt_cubes_from_points(np.asarray(origin, np.float64) + pts * resol, params, GT_D)
        surface = lambda: ctx.mesh_voxelize(v, f, cube, GT_D, STRIDE, modes=2, select=2, outputs=("Y",), device=True)
        Y, Ys = sample_gt(), surface()["Y"]
        st = _median_stages(ctx, surface, args.reps, "vox_")
        row["surface_target"] = dict(D=GT_D, voxels=N * GT_D ** 3, sample_gt_ms=_median_time(sample_gt, args.reps), voxelize_ms=_median_time(surface, args.reps),
                                     voxelize_kernel_ms=float(sum(st.values())), surface_voxels=int((Ys > 0).sum()), sampled_voxels=int((Y > 0).sum()),
                                     sampled_and_surface=int(((Y > 0) & (Ys > 0)).sum()))
        save()
    print(json.dumps(res["meshes"], default=float))


if __name__ == "__main__":
    main()
