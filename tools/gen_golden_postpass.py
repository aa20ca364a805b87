"""Records tests/golden/postpass_cases.npz and tests/golden/postpass_edge_cases.npz (the cases of tests/postpass_cases.py) from the REFERENCE's
own cross-cube post-pass (utils/denoising.py, utils/adapthresh.py, utils/sparseCubes.py of mjiUST/SurfaceNet), run under Python 3 / numpy 2 in
memory:

    python tools/gen_golden_postpass.py --reference /path/to/SurfaceNet [--out tests/golden/postpass_cases.npz] [--out-edge ...]

The three modules are read as text and executed with these Python-2 accommodations, nothing else changed: `d.has_key(k)` -> `(k) in d`,
integer `/` -> `//` (denoising.py:104,127, adapthresh.py:42, sparseCubes.py:53), print statements -> print(), load_sparseCubes opens its
file in binary mode (sparseCubes.py:384), the module-level doctest.testmod() is dropped, and the modules it imports but the post-pass does not
use (cPickle, rayPooling, camera, plyfile) are stubs. save_sparseCubes_2ply is replaced by a recorder of the masks (and rgb) it is given.

Only numbers are recorded: inputs (packed lists) and the reference's outputs. adapthresh's thresholds are not returned by the reference;
they are rebuilt from its debug PLY colours (rgb column argmin set to 255, utils/adapthresh.py:165-166) with the reference's own arithmetic,
min(t + [0.1, 0, -0.1][argmin], max_probThresh), on all-zero input colours.
"""
import argparse
import os
import re
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from surfacenet_amd import synthetic  # noqa: E402
import postpass_cases  # noqa: E402
import postpass_ref  # noqa: E402
from postpass_cases import mixed_votes  # noqa: E402


def _has_key(src):
    out, pat = [], re.compile(r"([A-Za-z_][\w\.]*)\.has_key\(")
    pos = 0
    for m in pat.finditer(src):
        if m.start() < pos:
            continue
        depth, j = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0)
            j += 1
        out.append(src[pos:m.start()] + "((%s) in %s)" % (src[m.end():j - 1], m.group(1)))
        pos = j
    return "".join(out) + src[pos:]


def _py3(src, fixes):
    for a, b in fixes:
        assert a in src, a
        src = src.replace(a, b)
    src = _has_key(src)
    src = re.sub(r"^(\s*)print (?!\()(.+)$", r"\1print(\2)", src, flags=re.M)
    src = "\n".join(line for line in src.split("\n") if line.strip() not in ("import doctest", "doctest.testmod()"))
    return src


def load_reference(ref_root):
    utils = os.path.join(ref_root, "utils")
    for name in ("cPickle", "rayPooling", "camera"):
        sys.modules[name] = types.ModuleType(name)
    ply = types.ModuleType("plyfile")
    ply.PlyData = ply.PlyElement = object
    sys.modules["plyfile"] = ply
    fixes = {
        "sparseCubes": [("(D_orig-cube_Dcenter)/2, (D_orig-cube_Dcenter)/2", "(D_orig-cube_Dcenter)//2, (D_orig-cube_Dcenter)//2"),
                        ("    with open(filePath) as f:\n        npz = np.load(f)", "    with open(filePath, 'rb') as f:\n        npz = np.load(f)")],
        "denoising": [("3**3/2", "3**3//2"), ("(D_cube / 2)", "(D_cube // 2)")],
        "adapthresh": [("D_mid = D_cube / 2", "D_mid = D_cube // 2")],
    }
    mods = {}
    for name in ("sparseCubes", "denoising", "adapthresh"):
        mod = types.ModuleType(name)
        mod.__file__ = os.path.join(utils, name + ".py")
        sys.modules[name] = mod
        exec(compile(_py3(open(mod.__file__).read(), fixes[name]), mod.__file__, "exec"), mod.__dict__)
        mods[name] = mod
    calls = []

    def recorder(vxl_mask_list, vxl_ijk_list, rgb_list, param, ply_filePath, normal_list=None):
        calls.append((os.path.basename(ply_filePath), [np.array(m, bool) for m in vxl_mask_list], [np.array(r) for r in rgb_list]))
        return 1
    mods["sparseCubes"].save_sparseCubes_2ply = recorder
    return mods, calls


def encode_ijk(ijk, Dc):
    """(T,3) uint8 -> int32 differences of the flat index (i*Dc + j)*Dc + k: the lists are sorted within each cube, so this compresses to
    almost nothing (tests/test_postpass_cpu.py decode_ijk inverts it)"""
    flat = (ijk[:, 0].astype(np.int64) * Dc + ijk[:, 1]) * Dc + ijk[:, 2]
    return np.diff(flat, prepend=0).astype(np.int32)


def pack(lists):
    counts = [len(a) for a in lists]
    off = np.zeros((len(lists) + 1,), np.int64)
    off[1:] = np.cumsum(counts)
    return off, (np.concatenate([np.asarray(a) for a in lists]) if counts else np.zeros((0,)))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def docstring_cases():
    """the inputs of the three docstring examples of utils/denoising.py (the first one has no cube ijk: a 2x2 block is assigned)"""
    u8 = lambda a: np.asarray(a, np.uint8)
    b = lambda a: np.asarray(a, bool)
    cluster = ([u8([[1, 0, 0], [2, 2, 2], [3, 3, 3], [1, 0, 1], [2, 3, 3], [0, 3, 3], [1, 2, 2]]), u8([[0, 2, 3], [0, 1, 0], [0, 0, 0], [0, 3, 3]]),
                u8([[0, 2, 3], [0, 1, 0], [0, 2, 3]]), u8([[0, 2, 3], [0, 1, 3], [0, 0, 0], [0, 3, 3], [3, 3, 3]])],
               [b([1, 0, 1, 1, 1, 1, 1]), b([1, 1, 0, 1]), b([0, 0, 0]), b([1, 1, 1, 1, 1])])
    mark = ([u8([[1, 0, 0], [2, 2, 2], [3, 2, 3], [3, 3, 3], [1, 0, 1], [2, 3, 3], [3, 0, 3]]), u8([[0, 2, 3], [0, 1, 3], [0, 0, 0], [0, 3, 3], [1, 0, 3], [3, 3, 0]]),
             u8([[0, 2, 3], [0, 1, 3], [0, 0, 0], [0, 3, 3]]), u8([[0, 2, 3], [0, 1, 3], [0, 0, 0], [0, 3, 3], [3, 3, 3]])],
            [b([1, 0, 0, 1, 1, 1, 1]), b([1, 1, 0, 1, 1, 1]), b([0, 0, 0, 0]), b([1, 1, 1, 1, 1])])
    den = ([u8([[1, 0, 0], [2, 2, 2], [3, 3, 3], [1, 0, 1], [2, 3, 3]]), u8([[0, 2, 3], [0, 1, 3], [0, 0, 0], [0, 3, 3], [3, 3, 0]]),
            u8([[0, 2, 3], [0, 1, 3], [0, 0, 0], [0, 3, 3]]), u8([[0, 2, 3], [0, 1, 3], [0, 0, 0], [0, 3, 3], [3, 3, 3]])],
           [b([1, 0, 1, 1, 1]), b([1, 1, 0, 1, 1]), b([0, 0, 0, 0]), b([1, 1, 1, 1, 1])])
    doc_cubes = np.asarray([[1, 6, 8], [2, 6, 8], [2, 7, 8], [2, 5, 8]], np.uint32)
    return [("doc_cluster", np.asarray([[0, 0, 0], [1, 0, 0], [0, 0, 1], [1, 1, 1]], np.uint32), cluster[0], cluster[1], 4),
            ("doc_mark", doc_cubes, mark[0], mark[1], 4), ("doc_denoise", doc_cubes, den[0], den[1], 4)]


def edge_scene(lattice, Dc, seed, thickness=2, amplitude=6.0):
    """sparse_surface + the edge cases: an empty cube, a cube whose voxels all fail the thresholds, cubes at ijk 0 (the lattice starts there),
    a repeated ijk whose later copy wins, a repeated ijk whose later copy is empty, and components that touch only at a corner"""
    d = synthetic.sparse_surface(lattice, Dc, thickness=thickness, amplitude=amplitude, seed=seed)
    rs = np.random.RandomState(seed + 100)
    P, I, V, R = d["prediction_list"], d["vxl_ijk_list"], d["rayPooling_votes_list"], d["rgb_list"]
    cubes, param = list(d["cube_ijk_np"]), list(d["param_np"])

    def add(ijk, pred, vox, votes, like):
        cubes.append(np.asarray(ijk, np.uint32)); param.append(param[like]); P.append(np.asarray(pred, np.float16))
        I.append(np.asarray(vox, np.uint8).reshape(-1, 3)); V.append(np.asarray(votes, np.uint8)); R.append(np.zeros((len(pred), 3), np.uint8))

    # corner-touching chains: a diagonal chain off the surface voxel 0 of cube 1, and an isolated diagonal pair in cube 2
    for c, start, attach in ((1, None, True), (2, (2, 2, 2), False)):
        base = I[c][0].astype(int) if attach else np.asarray(start)
        chain = [base + t * np.array([1, 1, -1 if base[2] > Dc // 2 else 1]) for t in (1, 2, 3)]
        chain = [p for p in chain if np.all((p >= 0) & (p < Dc))]
        extra = np.asarray(chain, np.uint8).reshape(-1, 3)
        I[c] = np.concatenate([I[c], extra]); P[c] = np.concatenate([P[c], np.full(len(extra), 0.97, np.float16)])
        V[c] = np.concatenate([V[c], np.full(len(extra), 9, np.uint8)]); R[c] = np.concatenate([R[c], np.zeros((len(extra), 3), np.uint8)])
    far = [lattice[0] + 3, 0, 0]
    add(far, [], np.zeros((0, 3)), [], 0)                                                    # empty cube
    add([lattice[0], 0, 0], np.full(len(I[0]), 0.3), I[0], np.zeros(len(I[0])), 0)          # every voxel below the thresholds
    rep = len(cubes) // 3
    sub = rs.rand(len(I[rep])) < 0.7
    add(cubes[rep], P[rep][sub], I[rep][sub], V[rep][sub], rep)                              # repeated ijk, the later copy wins
    add(cubes[rep + 1], np.full(3, 0.2), I[rep + 1][:3], np.zeros(3), rep + 1)                # repeated ijk, later copy empty after thresholds
    return dict(prediction_list=P, vxl_ijk_list=I, rayPooling_votes_list=V, rgb_list=R, cube_ijk_np=np.asarray(cubes, np.uint32),
                param_np=np.asarray(param, dtype=synthetic.CUBE_DTYPE), viewPair_np=np.zeros((len(cubes), 1, 2), np.uint16))


# ---- recording ------------------------------------------------------------------------------------------------------------------------------
def record_denoise(mods, out, name, cube_ijk, ijk_list, mask_list, D_cube):
    res = mods["denoising"].denoise_crossCubes(cube_ijk, [np.asarray(a) for a in ijk_list], [np.asarray(m, bool) for m in mask_list], D_cube=D_cube)
    off, ijk = pack(ijk_list)
    ijk = ijk.astype(np.uint8).reshape(-1, 3)
    Dc = int(ijk.max()) + 1
    key = [k for k in out if k.endswith("/ijk_delta") and k.startswith("dn/") and np.array_equal(out[k], encode_ijk(ijk, Dc))
           and np.array_equal(out[k.replace("ijk_delta", "mask")], pack(mask_list)[1].astype(np.uint8))]
    if key:                                   # the same lists with another D_cube: stored once
        out["dn/%s/inputs_of" % name] = np.asarray(key[0].split("/")[1])
    else:
        out["dn/%s/offsets" % name], out["dn/%s/ijk_delta" % name], out["dn/%s/Dc" % name] = off, encode_ijk(ijk, Dc), np.asarray(Dc, np.int64)
        out["dn/%s/cube_ijk" % name] = np.asarray(cube_ijk, np.uint32)
        out["dn/%s/mask" % name] = pack(mask_list)[1].astype(np.uint8)
    out["dn/%s/D_cube" % name] = np.asarray(D_cube, np.int64)
    out["dn/%s/out" % name] = pack(res)[1].astype(np.uint8)
    ref = postpass_ref.denoise_ref(cube_ijk, ijk_list, mask_list, D_cube)
    assert all(np.array_equal(a, b) for a, b in zip(ref, res)), name
    print("dn/%s: %d cubes, %d voxels, %d kept" % (name, len(ijk_list), ijk.shape[0], out["dn/%s/out" % name].sum()))


def record_adapthresh(mods, calls, out, name, d, N_iter, D_cube, init=0.5, min_t=0.5, max_t=0.9, rayPool=4, beta=6, gamma=0.8):
    d = dict(d)
    d["rgb_list"] = [np.zeros((len(a), 3), np.uint8) for a in d["vxl_ijk_list"]]
    with tempfile.TemporaryDirectory() as tmp:
        npz = os.path.join(tmp, "lists.npz")
        mods["sparseCubes"].save_sparseCubes(npz, d["prediction_list"], d["rgb_list"], d["vxl_ijk_list"], d["rayPooling_votes_list"],
                                             d["cube_ijk_np"], d["param_np"], d["viewPair_np"])
        del calls[:]
        last = mods["adapthresh"].adapthresh(tmp, N_iter, D_cube, init, min_t, max_t, rayPool, beta, gamma, npz, RGB_visual_ply=True)
        assert os.path.basename(last) == "iter%d.ply" % (N_iter - 1)
    names = [c[0] for c in calls]
    assert names == ["initialization.ply"] + sum([["iter%d.ply" % k, "iter%d_tmprgb4debug.ply" % k] for k in range(N_iter)], []), names
    n = len(d["vxl_ijk_list"])
    init_mask = [(np.asarray(p) >= init) & (np.asarray(v) >= rayPool) for p, v in zip(d["prediction_list"], d["rayPooling_votes_list"])]
    mp = postpass_ref.cube_map(d["cube_ijk_np"], init_mask)
    active = np.zeros(n, bool)
    active[list(mp.values())] = True
    t = [init] * n
    thresh, choice = [], []
    for k in range(N_iter):
        rgb = calls[2 + 2 * k][2]
        ch = np.full(n, -1, np.int8)
        for c in np.nonzero(active)[0]:
            cols = np.nonzero((rgb[c] == 255).all(axis=0))[0]
            assert len(cols) == 1, (name, k, c, cols)
            ch[c] = cols[0]
            t[c] = min(t[c] + [0.1, 0, -0.1][cols[0]], max_t)
        thresh.append(np.asarray(t, np.float64)); choice.append(ch)
    p = "at/%s/" % name
    off, ijk = pack(d["vxl_ijk_list"])
    Dc = int(ijk.max()) + 1
    out[p + "offsets"], out[p + "ijk_delta"], out[p + "Dc"], out[p + "cube_ijk"] = off, encode_ijk(ijk.astype(np.uint8).reshape(-1, 3), Dc), \
        np.asarray(Dc, np.int64), d["cube_ijk_np"]
    out[p + "pred16"], out[p + "votes"] = pack(d["prediction_list"])[1].astype(np.float16), pack(d["rayPooling_votes_list"])[1].astype(np.uint8)
    out[p + "param"] = d["param_np"]
    out[p + "args"] = np.asarray([N_iter, D_cube, init, min_t, max_t, rayPool, beta, gamma], np.float64)
    out[p + "init_denoised"] = pack(calls[0][1])[1].astype(np.uint8)
    out[p + "denoised"] = np.stack([pack(calls[1 + 2 * k][1])[1] for k in range(N_iter)]).astype(np.uint8)
    out[p + "masks"] = np.stack([pack(calls[2 + 2 * k][1])[1] for k in range(N_iter)]).astype(np.uint8)
    out[p + "thresh"], out[p + "choice"] = np.asarray(thresh), np.asarray(choice, np.int8)
    ref = postpass_ref.adapthresh_ref(d["prediction_list"], d["vxl_ijk_list"], d["rayPooling_votes_list"], d["cube_ijk_np"], N_iter, D_cube, init, max_t,
                                      rayPool, beta)
    assert np.array_equal(ref["thresh"], out[p + "thresh"]) and np.array_equal(ref["choice"], out[p + "choice"]), name
    exact = postpass_ref.adapthresh_ref(d["prediction_list"], d["vxl_ijk_list"], d["rayPooling_votes_list"], d["cube_ijk_np"], N_iter, D_cube, init,
                                        max_t, rayPool, beta, exact_cost=True)
    f16_decides = int((exact["choice"][:1] != ref["choice"][:1]).sum())
    n_inf = int(np.isinf(ref["cost"]).sum())
    print("at/%s: %d cubes, %d voxels, %d active, choices per iteration %s, first iteration's argmin differs from the exact-integer one in %d "
          "cubes, %d infinite costs" % (name, n, ijk.shape[0], active.sum(), [np.bincount(c[c >= 0], minlength=3).tolist() for c in choice],
                                        f16_decides, n_inf))
    return f16_decides, n_inf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a mjiUST/SurfaceNet checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "postpass_cases.npz"))
    ap.add_argument("--out-edge", default=os.path.join(ROOT, "tests", "golden", "postpass_edge_cases.npz"))
    args = ap.parse_args()
    mods, calls = load_reference(args.reference)
    out = {}
    for name, cubes, ijk_l, mask_l, D in docstring_cases():
        record_denoise(mods, out, name, cubes, ijk_l, mask_l, D)
    for Dc, cube_D, lattice, seed in ((26, 32, (3, 3, 2), 1), (52, 64, (2, 2, 2), 2)):
        d = edge_scene(lattice, Dc, seed)
        rs = np.random.RandomState(seed)
        masks = [(np.asarray(p) >= 0.7) & (np.asarray(v) >= 4) for p, v in zip(d["prediction_list"], d["rayPooling_votes_list"])]
        masks[len(masks) // 2 - 1][:] = False                       # a cube with voxels, every one masked out
        masks = [m & (rs.rand(m.size) < 0.97) for m in masks]
        for D in (Dc, cube_D):
            record_denoise(mods, out, "s%d_D%d" % (cube_D, D), d["cube_ijk_np"], d["vxl_ijk_list"], masks, D)
    record_adapthresh(mods, calls, out, "s32", mixed_votes(edge_scene((3, 2, 2), 26, 3, thickness=4, amplitude=3.0), 3), 4, 26, beta=2)
    f16, _ = record_adapthresh(mods, calls, out, "s32_f16", mixed_votes(edge_scene((3, 2, 2), 26, 22, thickness=12, amplitude=3.0), 22), 3, 26,
                               beta=1.5)
    assert f16 > 0, "no cube whose argmin the float16 rounding decides"
    _, n_inf = record_adapthresh(mods, calls, out, "s32_thick", edge_scene((2, 1, 2), 26, 7, thickness=16, amplitude=1.0), 2, 26, beta=12)
    assert n_inf > 0, "no infinite cost"
    record_adapthresh(mods, calls, out, "s64", mixed_votes(edge_scene((2, 2, 1), 52, 9, thickness=3), 9), 2, 52, beta=2)
    np.savez_compressed(args.out, **out)
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))
    # the cases of tests/postpass_cases.py TABLE: the kernel paths that depend on the cube width, and D_cube != Dc
    edge = {}
    for name in postpass_cases.TABLE:
        d, D_cube, _ = postpass_cases.build(name, postpass_cases.GOLDEN_LATTICE.get(name))
        record_denoise(mods, edge, name, d["cube_ijk_np"], d["vxl_ijk_list"], postpass_cases.denoise_masks(d), D_cube)
        a = postpass_cases.ARGS
        record_adapthresh(mods, calls, edge, name, d, a["N_refine_iter"], D_cube, init=a["init_probThresh"], max_t=a["max_probThresh"],
                          rayPool=a["rayPool_thresh"], beta=a["beta"])
    np.savez_compressed(args.out_edge, **edge)
    print("wrote %s (%d bytes)" % (args.out_edge, os.path.getsize(args.out_edge)))
    assert os.path.getsize(args.out_edge) < 700 * 1000


if __name__ == "__main__":
    main()
