"""Drop-in for the reference's `utils/adapthresh.py` on the MI355X (call site main.py:37-43).

    adapthresh   utils/adapthresh.py:91-178

Same name, arguments, output folder, file names and return value (the path of the last iter{k}.ply). The initial mask, its denoised form
and all N_refine_iter refinement iterations run in one device-resident GPU call (surfacenet_amd/csrc/crosscube.h); only the masks the PLY
files need come back. The float16 cost follows numpy 2. min_probThresh is accepted and ignored, as in the reference.
"""
import os

import numpy as np

from . import denoising, runtime, sparseCubes

THRESH_PERTURB = [0.1, 0, -0.1]          # utils/adapthresh.py:113, in this order (index = the argmin of the cost)


def adapthresh_lists(prediction_list, vxl_ijk_list, rayPooling_votes_list, cube_ijk_np, N_refine_iter, D_cube, init_probThresh, max_probThresh,
                     rayPool_thresh, beta, keep=("thresh", "masks", "denoised", "choice")):
    """The computation of `adapthresh` on in-memory lists, no file I/O. Returns the packed results (see Context.adapthresh) plus `offsets`."""
    offsets, ijk, Dc = denoising.pack_lists(vxl_ijk_list)
    T = ijk.shape[0]
    pred = np.concatenate([np.asarray(p, np.float16).reshape(-1) for p in prediction_list]) if len(prediction_list) else np.zeros((0,), np.float16)
    votes = None
    if rayPooling_votes_list is not None:
        votes = np.concatenate([np.asarray(v, np.uint8).reshape(-1) for v in rayPooling_votes_list]) if len(rayPooling_votes_list) else np.zeros((0,), np.uint8)
        if votes.size != T:
            raise ValueError("rayPooling_votes_list holds %d votes for %d voxels" % (votes.size, T))
    if pred.size != T:
        raise ValueError("prediction_list holds %d values for %d voxels" % (pred.size, T))
    res = runtime.any_context().adapthresh(offsets, ijk, pred, votes, cube_ijk_np, D_cube, N_refine_iter, init_probThresh, max_probThresh,
                                           rayPool_thresh, beta, Dc, keep=keep)
    res["offsets"] = offsets
    return res


def adapthresh(save_result_fld, N_refine_iter, D_cube, init_probThresh, min_probThresh, max_probThresh, rayPool_thresh, beta, gamma, npz_file,
               RGB_visual_ply=True):
    data = sparseCubes.load_sparseCubes(npz_file)
    prediction_list, rgb_list, vxl_ijk_list, rayPooling_votes_list, cube_ijk_np, param_np, viewPair_np = data
    save_result_fld = os.path.join(save_result_fld, "adapThresh_gamma{:.3}_beta{}".format(gamma, beta))
    if not os.path.exists(save_result_fld):
        os.makedirs(save_result_fld)
    keep = ("denoised", "masks", "choice") if RGB_visual_ply else ("denoised",)
    res = adapthresh_lists(prediction_list, vxl_ijk_list, rayPooling_votes_list, cube_ijk_np, N_refine_iter, D_cube, init_probThresh, max_probThresh,
                           rayPool_thresh, beta, keep=keep)
    off = res["offsets"]
    sparseCubes.save_sparseCubes_2ply(denoising.split_lists(res["init_denoised"], off), vxl_ijk_list, rgb_list, param_np,
                                      ply_filePath=os.path.join(save_result_fld, 'initialization.ply'), normal_list=None)
    for _iter in range(N_refine_iter):
        ply_filePath = os.path.join(save_result_fld, 'iter{}.ply'.format(_iter))
        sparseCubes.save_sparseCubes_2ply(denoising.split_lists(res["denoised"][_iter], off), vxl_ijk_list, rgb_list, param_np,
                                          ply_filePath=ply_filePath, normal_list=None)
        if RGB_visual_ply:
            tmp_rgb_list = [np.array(r, copy=True) for r in rgb_list]
            for c in np.nonzero(res["choice"][_iter] >= 0)[0]:
                tmp_rgb_list[c][:, res["choice"][_iter][c]] = 255      # R/G/B <- the chosen perturbation +0.1 / 0 / -0.1
            sparseCubes.save_sparseCubes_2ply(denoising.split_lists(res["masks"][_iter], off), vxl_ijk_list, tmp_rgb_list, param_np,
                                              ply_filePath=os.path.join(save_result_fld, 'iter{}_tmprgb4debug.ply'.format(_iter)), normal_list=None)
    return ply_filePath
