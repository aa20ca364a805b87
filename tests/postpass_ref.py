"""CPU restatement of the cross-cube post-pass (numpy / scipy) - a CHECKER for tests/, never the product path.

    denoise_ref      utils/denoising.py:150-184   denoise_crossCubes
    adapthresh_ref   utils/adapthresh.py:91-178   adapthresh's computation (no file I/O)

Written from the contract in DESIGN.md section 4.6 on dense boolean cubes; tests/test_postpass_cpu.py holds it to the goldens recorded from the
reference itself (tests/golden/postpass_cases.npz), the GPU tests hold the HIP kernels to it at scale. `exact_cost=True` accumulates the cost
in Python integers instead of float16 (used to show that a golden case depends on the float16 rounding).
"""
import os

import numpy as np
import scipy.ndimage as ndi

SHIFTS26 = [s for s in (np.indices((3, 3, 3)).reshape(3, -1).T - 1).tolist() if s != [0, 0, 0]]
FACES = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]]
THRESH_PERTURB = [0.1, 0, -0.1]


def _dc(vxl_ijk_list):
    m = [int(np.asarray(a).max()) for a in vxl_ijk_list if len(a)]
    return max(m) + 1 if m else 1


def _dense(ijk, Dc):
    occ = np.zeros((Dc, Dc, Dc), bool)
    ijk = np.asarray(ijk).reshape(-1, 3).astype(np.int64)
    occ[ijk[:, 0], ijk[:, 1], ijk[:, 2]] = True
    return occ


def _shifted(occ, d):
    """S[v] = occ[v - d] where defined, else False."""
    Dc = occ.shape[0]
    out = np.zeros_like(occ)
    src, dst = [], []
    for x in d:
        if abs(x) >= Dc:
            return out
        src.append(slice(max(0, -x), Dc - max(0, x)))
        dst.append(slice(max(0, x), Dc + min(0, x)))
    out[tuple(dst)] = occ[tuple(src)]
    return out


def cube_map(cube_ijk_np, vxl_mask_list):
    """ijk tuple -> cube index over the cubes with a non-empty mask; the last one wins."""
    m = {}
    for n, ijk in enumerate(np.asarray(cube_ijk_np).reshape(-1, 3).tolist()):
        if np.asarray(vxl_mask_list[n]).sum() > 0:
            m[tuple(ijk)] = n
    return m


def denoise_ref(cube_ijk_np, vxl_ijk_list, vxl_mask_list, D_cube, Dc=None, fault=None):
    """fault = (c, i, j, k) plants a kernel's slip for tests/test_postpass_cpu.py: cube c's bit row (i, j) loses bit k."""
    Dc = Dc or _dc(vxl_ijk_list)
    mp = cube_map(cube_ijk_np, vxl_mask_list)
    keys = [tuple(k) for k in np.asarray(cube_ijk_np).reshape(-1, 3).tolist()]
    occ = {c: _dense(np.asarray(vxl_ijk_list[c])[np.asarray(vxl_mask_list[c], bool)], Dc) for c in set(mp.values())}
    if fault is not None:
        occ[fault[0]][fault[1], fault[2], fault[3]] = False
    h = D_cube // 2
    out = []
    for c, key in enumerate(keys):
        mask = np.asarray(vxl_mask_list[c], bool)
        res = np.zeros(mask.shape, bool)
        if mp.get(key) == c:
            labels, _ = ndi.label(occ[c], np.ones((3, 3, 3), bool))
            touched = np.zeros_like(occ[c])
            for s in SHIFTS26:
                nb = mp.get((key[0] + s[0], key[1] + s[1], key[2] + s[2]))
                if nb is not None:
                    touched |= occ[c] & _shifted(occ[nb], [h * x for x in s])
            good = np.unique(labels[touched])
            v = np.asarray(vxl_ijk_list[c])[mask].astype(np.int64)
            res[mask] = np.isin(labels[v[:, 0], v[:, 1], v[:, 2]], good)
        out.append(res)
    return out


def _half(occ, s, D_cube):
    """access_partial_Occupancy_ijk on a dense cube: the half selected by shift s, translated, as a (D_cube,)*3 dense array."""
    Dc, h = occ.shape[0], D_cube // 2
    H = np.zeros((D_cube,) * 3, bool)
    src, dst = [], []
    for x in s:
        lo, hi = (0, h) if x == -1 else (0, D_cube) if x == 0 else (h, D_cube)
        hi = min(hi, Dc)
        if hi <= lo:
            return H
        t = h if x == 1 else 0
        src.append(slice(lo, hi))
        dst.append(slice(lo - t, hi - t))
    H[tuple(dst)] = occ[tuple(src)]
    return H


def _half_count(ijk, s, D_cube):
    """number of list rows (duplicates included, as .shape[0]) in the half selected by shift s"""
    ijk = np.asarray(ijk).reshape(-1, 3).astype(np.int64)
    h, sel = D_cube // 2, np.ones(ijk.shape[0], bool)
    for d, x in enumerate(s):
        lo, hi = (0, h) if x == -1 else (0, D_cube) if x == 0 else (h, D_cube)
        sel &= (ijk[:, d] >= lo) & (ijk[:, d] < hi)
    return int(sel.sum())


def adapthresh_ref(prediction_list, vxl_ijk_list, rayPooling_votes_list, cube_ijk_np, N_refine_iter, D_cube, init_probThresh, max_probThresh,
                   rayPool_thresh, beta, Dc=None, exact_cost=False, fault=None):
    """-> dict(init_denoised, thresh (N,n), masks, denoised (lists per iteration), choice (N,n) int8, cost (N,n,3))
    fault = (c, g, g_from) plants a kernel's slip for tests/test_postpass_cpu.py: cube c's grid g is built with the threshold of grid g_from,
    or stays empty (g_from None: a pass that never ran)."""
    Dc = Dc or _dc(vxl_ijk_list)
    n = len(vxl_ijk_list)
    keys = [tuple(k) for k in np.asarray(cube_ijk_np).reshape(-1, 3).tolist()]
    masks = [(np.asarray(p) >= init_probThresh) & (np.asarray(v) >= rayPool_thresh) for p, v in zip(prediction_list, rayPooling_votes_list)]
    out = dict(init_denoised=denoise_ref(cube_ijk_np, vxl_ijk_list, masks, D_cube, Dc), thresh=[], masks=[], denoised=[], choice=[], cost=[])
    mp = cube_map(cube_ijk_np, masks)
    t = [init_probThresh] * n
    for _ in range(N_refine_iter):
        sel = {}

        def occupied(c, g):
            if (c, g) not in sel:
                m = masks[c] & (np.asarray(prediction_list[c]) >= t[c] + THRESH_PERTURB[g])
                if fault is not None and (c, g) == tuple(fault[:2]):
                    m = m & False if fault[2] is None else masks[c] & (np.asarray(prediction_list[c]) >= t[c] + THRESH_PERTURB[fault[2]])
                ijk = np.asarray(vxl_ijk_list[c])[m]
                sel[(c, g)] = (ijk, _dense(ijk, Dc))
            return sel[(c, g)]

        t_new, choice, costs = list(t), np.full((n,), -1, np.int8), np.zeros((n, 3))
        for c in sorted(set(mp.values())):
            key = keys[c]
            cost = [0, 0, 0] if exact_cost else np.zeros((3,), np.float16)
            for s in FACES:
                nb = mp.get((key[0] + s[0], key[1] + s[1], key[2] + s[2]))
                if nb is not None:
                    ijk_b, occ_b = occupied(nb, 1)
                    nB, HB = _half_count(ijk_b, [-x for x in s], D_cube), _half(occ_b, [-x for x in s], D_cube)
                else:
                    nB, HB = 0, None
                for g in range(3):
                    ijk_a, occ_a = occupied(c, g)
                    nA = _half_count(ijk_a, s, D_cube)
                    AND = 0 if HB is None else int((_half(occ_a, s, D_cube) & HB).sum())
                    cost[g] += nA + nB - AND * 2
                    if nA >= 6 and nB >= 6:
                        cost[g] -= beta * AND
            best = int(np.argmin(cost))
            t_new[c] = min(t[c] + THRESH_PERTURB[best], max_probThresh)
            choice[c], costs[c] = best, np.asarray(cost, np.float64)
        t = t_new
        masks = [m & (np.asarray(p) >= t[c]) for c, (m, p) in enumerate(zip(masks, prediction_list))]
        out["thresh"].append(np.asarray(t, np.float64))
        out["masks"].append([m.copy() for m in masks])
        out["denoised"].append(denoise_ref(cube_ijk_np, vxl_ijk_list, masks, D_cube, Dc))
        out["choice"].append(choice)
        out["cost"].append(costs)
    out["thresh"] = np.asarray(out["thresh"]).reshape(N_refine_iter, n)
    out["choice"] = np.asarray(out["choice"], np.int8).reshape(N_refine_iter, n)
    out["cost"] = np.asarray(out["cost"]).reshape(N_refine_iter, n, 3)
    return out


# ---- tests/golden/postpass_cases.npz, postpass_edge_cases.npz (tools/gen_golden_postpass.py) ------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "postpass_cases.npz")
GOLDEN_EDGE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "postpass_edge_cases.npz")


def decode_ijk(delta, Dc):
    flat = np.cumsum(delta.astype(np.int64))
    return np.stack([flat // (Dc * Dc), (flat // Dc) % Dc, flat % Dc], -1).astype(np.uint8)


def split(flat, offsets):
    return [flat[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]


def load_cases():
    """-> (denoise cases {name: dict(cube_ijk, ijk_list, mask_list, D_cube, out_list)}, adapthresh cases {name: dict(...)}) of both files"""
    dn, at = {}, {}
    for path in (GOLDEN, GOLDEN_EDGE):
        d, a = _load(path)
        assert not (set(d) & set(dn)) and not (set(a) & set(at)), "a case name in both golden files"
        dn.update(d); at.update(a)
    return dn, at


def _load(path):
    z = np.load(path)
    dn, at = {}, {}
    names = sorted({k.split("/")[1] for k in z.files if k.startswith("dn/")})
    for nm in names:
        src = str(z["dn/%s/inputs_of" % nm]) if "dn/%s/inputs_of" % nm in z.files else nm
        p, q = "dn/%s/" % src, "dn/%s/" % nm
        off = z[p + "offsets"]
        dn[nm] = dict(cube_ijk=z[p + "cube_ijk"], ijk_list=split(decode_ijk(z[p + "ijk_delta"], int(z[p + "Dc"])), off),
                      mask_list=[m.astype(bool) for m in split(z[p + "mask"], off)], D_cube=int(z[q + "D_cube"]),
                      out_list=[m.astype(bool) for m in split(z[q + "out"], off)], offsets=off)
    for nm in sorted({k.split("/")[1] for k in z.files if k.startswith("at/")}):
        p = "at/%s/" % nm
        off = z[p + "offsets"]
        a = z[p + "args"]
        at[nm] = dict(offsets=off, cube_ijk=z[p + "cube_ijk"], ijk_list=split(decode_ijk(z[p + "ijk_delta"], int(z[p + "Dc"])), off),
                      pred_list=split(z[p + "pred16"], off), votes_list=split(z[p + "votes"], off), param=z[p + "param"],
                      N_refine_iter=int(a[0]), D_cube=int(a[1]), init_probThresh=float(a[2]), min_probThresh=float(a[3]), max_probThresh=float(a[4]),
                      rayPool_thresh=int(a[5]), beta=float(a[6]) if a[6] != int(a[6]) else int(a[6]), gamma=float(a[7]),
                      init_denoised=z[p + "init_denoised"].astype(bool), thresh=z[p + "thresh"], masks=z[p + "masks"].astype(bool),
                      denoised=z[p + "denoised"].astype(bool), choice=z[p + "choice"])
    return dn, at
