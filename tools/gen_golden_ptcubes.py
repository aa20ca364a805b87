#!/usr/bin/env python3
"""tools/gen_golden_ptcubes.py — TEST INFRASTRUCTURE. Writes tests/golden/ptcubes_cases.npz by EXECUTING THE REFERENCE's
scene.quantizePts2Cubes (utils/scene.py:63-108) under the installed numpy (2.x: the promotion rules the contract names).

Needs the reference tree (loaded as oracle/gen_golden_scene.py loads it: stand-in plyfile / mesh_util modules, doctest tail cut, source
unmodified otherwise). Only arrays are written: inputs, the reference's outputs, no reference text. tests/ptcubes_ref.py::golden_cases reads
the file back.

Usage:  python tools/gen_golden_ptcubes.py   (from the repo root)
"""
import contextlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ptcubes_ref as R                                   # noqa: E402  (the seeded clouds and the case layout only)
from oracle.gen_golden_scene import load_reference_modules   # noqa: E402

KINDS = {float: 0, np.float32: 1, np.float64: 2, int: 3}


def fitted_box(target_lo, target_hi, half):
    """A BB (3,2) float64 whose widened box BB -+ half, evaluated in numpy's scalar arithmetic, is exactly [target_lo, target_hi] per axis."""
    BB = np.zeros((3, 2), np.float64)
    for ax in range(3):
        for side, (t, sgn) in enumerate(((target_lo[ax], 1), (target_hi[ax], -1))):
            v = np.float64(t) + sgn * np.float64(half)
            for _ in range(64):
                got = (v - half) if side == 0 else (v + half)
                if got == t:
                    break
                v = np.nextafter(v, np.inf if got < t else -np.inf)
            else:
                raise RuntimeError("no BB value reproduces the bound %r" % (t,))
            BB[ax, side] = v
    return BB


def main():
    _, scene = load_reference_modules()
    out, names = {}, []

    def case(name, pts, resol, cube_D, cube_Dcenter, ratio, BB=None, pts_of=None, extra=None):
        full = pts if extra is None else np.concatenate([pts, extra.astype(pts.dtype)])
        with contextlib.redirect_stdout(io.StringIO()):
            cubes, dmm = scene.quantizePts2Cubes(full, resol, cube_D, cube_Dcenter, ratio, BB=BB)
        names.append(name)
        if pts_of is None:
            out[name + "_pts"] = pts
        else:
            out[name + "_pts_of"] = np.array(pts_of)
        if extra is not None:
            out[name + "_extra"] = extra
        if BB is not None:
            out[name + "_BB"] = BB
        out[name + "_dtype"] = np.array(pts.dtype.str)
        out[name + "_resol_kind"] = np.int64(KINDS[type(resol)])
        out[name + "_resol"] = np.asarray(resol)
        out[name + "_cube"] = np.array([cube_D, cube_Dcenter], np.int64)
        out[name + "_ratio"] = np.float64(ratio)
        out[name + "_ijk"], out[name + "_xyz"] = np.ascontiguousarray(cubes["ijk"]), np.ascontiguousarray(cubes["xyz"])
        out[name + "_cube_D_mm"] = np.asarray(dmm)
        assert np.all(cubes["resol"] == np.float32(resol))
        print("%-28s %8d pts -> %6d cubes" % (name, full.shape[0], cubes.shape[0]))

    # the doctest input of scene.py:83-84
    doc = np.array([[-1, 2, 0], [0, 2, 0], [1, 2, 0], [0, 1, 0], [0, 0, 0], [1, 0, 0], [2.1, 0, 0]])
    case("doc", doc, 2, 3, 2, 0.5)

    # a wavy surface with scan9's parameters: both point dtypes x three resol types x (no BB, a BB that cuts points off)
    base = R.wavy_cloud(20000, seed=11, spatial=False)
    out["base_wavy"] = base
    lo_t, hi_t = np.array([-40.5, -120.25, 600.0]), np.array([90.75, 100.5, 700.125])        # float32-representable bounds inside the cloud
    for dt in (np.float64, np.float32):
        for resol in (0.4, np.float32(0.4), np.float64(0.4)):
            tag = "wavy_%s_%s" % (np.dtype(dt).name, {float: "py", np.float32: "f32", np.float64: "f64"}[type(resol)])
            case(tag, base.astype(dt), resol, 32, 26, 0.5, pts_of="base_wavy")
            half = resol * 32 / 2
            BB = fitted_box(lo_t, hi_t, half)
            mid = (lo_t + hi_t) / 2
            extra = []
            for ax in range(3):                                   # exactly on each bound (kept), one step outside it (dropped)
                for b, away in ((lo_t[ax], -np.inf), (hi_t[ax], np.inf)):
                    for v in (b, np.nextafter(dt(b), dt(away))):
                        p = mid.copy()
                        p[ax] = v
                        extra.append(p)
            extra = np.asarray(extra, np.float64)
            case(tag + "_bb", base.astype(dt), resol, 32, 26, 0.5, BB=BB, pts_of="base_wavy", extra=extra)
            n_in = sum(int(np.all((extra[i] >= lo_t) & (extra[i] <= hi_t))) for i in range(len(extra)))
            assert n_in == 6, n_in

    # a lattice exactly at k/10 with stride 0.1 (resol 0.1, Dcenter 2, overlap 0.5): floor_divide and floor(a / b) disagree at 1.0 and elsewhere
    k = np.arange(0, 31)
    lat = np.stack(np.meshgrid(k / 10.0, k[:7] / 10.0, k[:3] / 10.0, indexing="ij"), -1).reshape(-1, 3)
    a = lat[:, 0]
    assert np.any(np.floor_divide(a, 0.1) != np.floor(a / 0.1)) and 1.0 // 0.1 == 9.0
    for dt in (np.float64, np.float32):
        case("lattice_%s" % np.dtype(dt).name, lat.astype(dt), 0.1, 4, 2, 0.5)

    # two small clusters 1e5 mm apart on every axis, stride 0.05: about 2e6 cells per axis - no bitmap over the cells is possible
    rs = np.random.RandomState(5)
    far = np.concatenate([rs.rand(300, 3) * 2.0, 1.0e5 + rs.rand(300, 3) * 2.0])
    case("far_clusters", far, 0.05, 4, 2, 0.5)

    # Middlebury dino scale (params.py:176-182)
    BBd = np.array([(-0.061897, 0.010897), (-0.018874, 0.068227), (-0.057845, 0.015495)], dtype=np.float32)
    dino = R.wavy_cloud(5000, BB=BBd, seed=3, dtype=np.float32, spatial=True)
    case("dino", dino, np.float32(0.00025), 32, 26, 0.5, BB=BBd)

    one = np.array([[12.5, -3.25, 640.0]])
    case("single_point", one, 0.4, 32, 26, 0.5)
    case("identical_points", np.repeat(one.astype(np.float32), 50, axis=0), np.float32(0.4), 32, 26, 0.5)

    out["names"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "ptcubes_cases.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d bytes" % (path, len(names), os.path.getsize(path)))


if __name__ == "__main__":
    main()
