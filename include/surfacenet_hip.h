/*
 * surfacenet_hip.h — C ABI of libsurfacenet_hip.so (MI355X / gfx950).
 *
 * The reference (mjiUST/SurfaceNet) has no FFI: its hot path is three Python callables used in
 * main_reconstruct.py:134-146. This header is what a ctypes binding of those callables needs; each
 * entry point cites the reference interface it replaces (paths relative to the reference root).
 * The Python side that presents the reference's own signatures on top of this ABI lives in
 * surfacenet_amd/CVC.py and surfacenet_amd/SurfaceNet.py.
 *
 * Conventions: plain C; every pointer is caller-owned HOST memory unless the parameter name ends in
 * `_dev` (device memory of the context's GPU); functions returning int give 0 on success and a
 * negative sn_status on failure, with a human-readable message from sn_last_error() (thread-local).
 * One sn_ctx per GPU per host thread; a context is not thread-safe, the library has no global state.
 * All work of a context is issued on one HIP stream owned by the context; host-pointer entry points
 * are synchronous, `_dev` entry points are asynchronous until sn_synchronize().
 */
#ifndef SURFACENET_HIP_H
#define SURFACENET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SN_ABI_VERSION 2   /* 2 (round 6): + sn_mfma_probe, sn_set_conv4_fp8; sn_calibrate_dev refuses the all-MX mode with SN_ERR_STATE (since round 5) */
/* Added since, without a version change (additions only): sn_ptcubes, sn_ptcubes_dev, sn_ptcubes_sparse_dev and sn_ptcubes_cfg - the
 * point-seeded cube list; sn_normals, sn_normals_dev, sn_unique_voxels, sn_unique_voxels_dev and sn_normals_cfg - oriented normals and
 * de-duplication of the output cloud; sn_gt_bind, sn_gt_bind_dev, sn_gt_cubes, sn_gt_cubes_dev, sn_weighted_accuracy and
 * sn_weighted_accuracy_dev - the ground-truth mode; sn_mesh, sn_mesh_dev and sn_mesh_cfg - the surface-nets mesh of the oriented cloud;
 * sn_mesh_sample and sn_mesh_sample_dev - surface samples of a triangle mesh; sn_components, sn_components_dev and sn_components_cfg - connected
 * components of the output cloud; sn_mesh_simplify, sn_mesh_simplify_dev and sn_mesh_simplify_cfg - a triangle mesh made smaller by vertex
 * clustering; sn_mesh_smooth, sn_mesh_smooth_dev and sn_mesh_smooth_cfg - Taubin smoothing of a triangle or quad mesh in fixed point, with
 * the mesh's edge and boundary counts; sn_mesh_fill, sn_mesh_fill_dev and sn_mesh_fill_cfg - the mesh's small holes capped by centroid fans;
 * sn_mesh_normals and sn_mesh_normals_dev - a mesh's own area-weighted normals with its exact area and volume;
 * sn_mesh_orient, sn_mesh_orient_dev and sn_mesh_orient_cfg - a mesh's faces made to turn one way, its pieces and their exact volumes;
 * sn_mesh_render, sn_mesh_render_dev, sn_mesh_vertex_colors, sn_mesh_vertex_colors_dev and sn_mesh_render_cfg - a mesh rendered back into its
 * views: depth maps, face ids, visibility, vertex colours; sn_mesh_intersect, sn_mesh_intersect_dev and sn_mesh_intersect_cfg - the pairs of
 * faces of a mesh that cross or touch each other, exactly; sn_mesh_distance, sn_mesh_distance_dev and sn_mesh_distance_cfg - for every
 * point of a set the nearest point of a mesh: its squared distance, its face, the point itself; sn_mesh_winding, sn_mesh_winding_dev and
 * sn_mesh_winding_cfg - for every point of a set how many times a mesh winds around it, exactly: inside, outside or on the surface;
 * sn_mesh_voxelize, sn_mesh_voxelize_dev and sn_mesh_voxelize_cfg - a mesh voxelised into cubes: exact solid and surface occupancy. */

/* The library is built with -fvisibility=hidden: the functions below are its WHOLE dynamic symbol table
 * (tests/test_abi.py compares `nm -D` with this header). */
#define SN_API __attribute__((visibility("default")))

typedef struct sn_ctx sn_ctx;

enum sn_status {
    SN_OK = 0,
    SN_ERR_ARG = -1,     /* bad argument (shape, null pointer, view id out of range ...) */
    SN_ERR_STATE = -2,   /* call order: weights / images / cameras not set                */
    SN_ERR_HIP = -3,     /* HIP runtime error; text carries hipGetErrorString             */
    SN_ERR_NOMEM = -4,
    SN_ERR_COMM = -5,
    SN_ERR_RANGE = -6    /* a conv layer stored a non-finite value or one beyond the fp16 range of its storage format */
};

/* One parameter array inside the weight blob (reference pickle = flat list of arrays,
 * nets/SurfaceNet.py:397-400; order documented in SURVEY.md App. B / DESIGN.md). */
typedef struct {
    int64_t offset;   /* in floats, into `blob` */
    int32_t ndim;
    int32_t shape[5];
} sn_param_desc;

/* ---- lifetime -------------------------------------------------------------------------------- */
/* cube_D = s of the s^3 colored voxel cube (params.py:65, 32 or 64; any multiple of 4 in [8,96]
 * except 36 and 68 is accepted); max_samples = largest n*n_vp processed per internal pass (activation
 * workspace is sized for it; larger calls are chunked). Returns NULL on failure (sn_last_error). */
SN_API sn_ctx *sn_create(int device_id, int cube_D, int max_samples);
SN_API void sn_destroy(sn_ctx *ctx);
SN_API const char *sn_last_error(void);
SN_API int sn_version(void);
SN_API int sn_synchronize(sn_ctx *ctx);

/* Arithmetic of the 3D-CNN (the CVC warp is always the reference's fp64/int arithmetic):
 *   SN_PRECISION_F16X3 (default): operands carried as hi+lo pairs of fp16 (22 significant bits), three
 *       MFMAs per product term, fp32 accumulate -> fp32-class results. The two LAST 3x3x3 layers (merge_conv_a,
 *       merge_conv_b: 56 % of a step) compute their two correction terms on one MX-scaled MFMA with 6-bit
 *       (fp6 e2m3) operands, which issues at twice the fp16 rate: 1.5 MFMA units per product instead of 3;
 *       the three dilated layers conv4_1 .. conv4_3 (round 5) compute theirs on one MX-scaled MFMA with fp8 e4m3
 *       operands: 2 units (fp8, not fp6: their activations need the exponent range).
 *       L_inf vs the fp64 oracle 3e-5 .. 1.7e-4 (asserted 2e-4, bar 1e-3);
 *   SN_PRECISION_F16X3_PURE: all three MFMAs in fp16 in every layer (L_inf ~1e-5);
 *   SN_PRECISION_F16: operands rounded to fp16, fp32 accumulate -> 3x faster, L_inf ~2e-3 on BN-normalised
 *       nets, i.e. above the 1e-3 parity bar; opt-in fast mode.
 * Call before sn_load_weights (weights are packed for the selected mode). */
#define SN_PRECISION_F16 0
#define SN_PRECISION_F16X3 1
/*   SN_PRECISION_F16M8 (experimental; the default dominates it in speed and accuracy): EVERY layer with the main term
 *       on the f16 MFMA and the two 2^-11 correction terms on one MX-scaled 6-bit MFMA
 *       (v_mfma_scale_f32_16x16x128_f8f6f4); L_inf 1e-4 .. 4e-4 (bar 1e-3). */
#define SN_PRECISION_F16M8 2
#define SN_PRECISION_F16X3_PURE 3
SN_API int sn_set_precision(sn_ctx *ctx, int mode);
SN_API int sn_get_precision(sn_ctx *ctx);
/* SN_PRECISION_F16X3 only: which layers of the dilated chain conv4_1 .. conv4_3 (nets/layers.py:200-253) compute their correction terms on the fp8 MX
 * MFMA (2 MFMA units per product) instead of three fp16 MFMAs. on = 1 (default): all three - worst observed L_inf 1.83e-4 over the 202-input survey
 * of round 6, conv4_x 1.15 ms per 128 samples; on = 2: conv4_2 and conv4_3 only (conv4_1 on three fp16 MFMAs: <= 1.54e-4 on the survey's worst
 * inputs, +0.07 ms); on = 0: none - the round-4 arithmetic (<= 9.5e-5 on the same inputs, conv4_x 1.5 ms). The merge layers keep their 6-bit
 * correction step in every setting. Call after sn_set_precision (which resets it to 1) and before sn_load_weights (a change discards packed
 * weights: SN_ERR_STATE from the forward calls until they are loaded again). */
SN_API int sn_set_conv4_fp8(sn_ctx *ctx, int on);

/* ---- one-time setup -------------------------------------------------------------------------- */
/* Replaces lasagne.layers.set_all_param_values(...) in SurfaceNet_inference
 * (nets/SurfaceNet.py:385-402). `descs` lists the 105 arrays of the reference pickle in its order
 * (98 for the network alone: the relative-weight MLP arrays may be omitted). BN folding and the
 * fp16 MFMA-fragment packing happen inside. */
SN_API int sn_load_weights(sn_ctx *ctx, const float *blob, size_t n_floats, const sn_param_desc *descs, int n_params);
/* models_img of CVC.gen_coloredCubes (utils/CVC.py:56): V images, (H[v], W[v], 3) uint8 RGB. */
SN_API int sn_set_images(sn_ctx *ctx, int V, const uint8_t *const *imgs, const int *H, const int *W);
/* cameraPOs of CVC.gen_coloredCubes: (V,3,4) float64 row-major projection matrices. */
SN_API int sn_set_cameras(sn_ctx *ctx, int V, const double *P);

/* ---- hot path, host buffers ------------------------------------------------------------------ */
/* CVC.gen_coloredCubes (utils/CVC.py:56-104) [+ CVC.preprocess_augmentation, utils/CVC.py:108-111,
 * when mean6 != NULL]. view_pairs (n, n_vp, 2) int64 indices into the image/camera lists;
 * xyz (n,3) float32 cube min corners; resol (n,) float32; out (n*n_vp, 6, s,s,s) float32. */
SN_API int sn_cvc(sn_ctx *ctx, int n, int n_vp, const int64_t *view_pairs, const float *xyz, const float *resol,
           const float *mean6, float *out);
/* nViewPair_SurfaceNet_fn (nets/SurfaceNet.py:365-382; call at main_reconstruct.py:145-146).
 * X (n*n_vp, 6, s,s,s) float32 mean-subtracted; w (n, n_vp) float32 (NULL iff n_vp == 1);
 * fused (n,1,s,s,s); unfused (n,n_vp,s,s,s) or NULL. */
SN_API int sn_forward(sn_ctx *ctx, int n, int n_vp, const float *X, const float *w, float *fused, float *unfused);
/* The loop body main_reconstruct.py:134-146 in one call: CVC warp -> mean subtraction -> CNN ->
 * fusion, nothing but the cube parameters crossing PCIe. cvc_out (optional) receives the
 * mean-subtracted CVC tensor the reference keeps for colour fusion (main_reconstruct.py:150). */
SN_API int sn_cvc_forward(sn_ctx *ctx, int n, int n_vp, const int64_t *view_pairs, const float *xyz, const float *resol,
                   const float *mean6, const float *w, float *fused, float *unfused, float *cvc_out);
/* viewPair_relativeImpt_fn (nets/SurfaceNet.py:334-338; used at utils/viewPairSelection.py:77):
 * features (n*n_vp, 258) float32 -> softmax weights (n, n_vp). */
SN_API int sn_relative_weights(sn_ctx *ctx, int n, int n_vp, const float *features, float *weights);

/* The weight computation of viewPairSelection.viewPairSelection (utils/viewPairSelection.py:63-77) for every 2-combination of
 * views (itertools.combinations order) in one call: embeddings (n_cubes,n_views,128), dissimilarity and theta (n_cubes,P)
 * float32 -> softmax weights (n_cubes,P). Bit-identical to building the (n_cubes*P,258) feature rows and calling
 * sn_relative_weights with n_vp = P. */
SN_API int sn_viewpair_weights(sn_ctx *ctx, int n_cubes, int n_views, const float *embeddings, const float *dissimilarity,
                        const float *theta, float *weights);

/* utils.generate_voxelLevelWeighted_coloredCubes (utils/utils.py:8-42; call at main_reconstruct.py:150-152), float32 op for
 * op: cvc (n*n_vp,6,s,s,s) is the MEAN-SUBTRACTED tensor of sn_cvc_forward (the caller's `X += mean` is applied inside);
 * unfused (n,n_vp,s,s,s), w (n,n_vp) -> rgb (n,3,s,s,s) uint8. */
SN_API int sn_color_fuse(sn_ctx *ctx, int n, int n_vp, const float *cvc, const float *mean6, const float *unfused, const float *w,
                  unsigned char *rgb);
SN_API int sn_color_fuse_dev(sn_ctx *ctx, int n, int n_vp, const float *cvc_dev, const float *mean6, const float *unfused_dev,
                      const float *w_dev, unsigned char *rgb_dev);

/* ---- hot path, device-resident (asynchronous on the context's stream) ------------------------- */
SN_API void *sn_dev_alloc(sn_ctx *ctx, size_t bytes);
SN_API int sn_dev_free(sn_ctx *ctx, void *p_dev);
SN_API int sn_memcpy_h2d(sn_ctx *ctx, void *dst_dev, const void *src, size_t bytes);
SN_API int sn_memcpy_d2h(sn_ctx *ctx, void *dst, const void *src_dev, size_t bytes);
/* Pipelined readback for loops that enqueue the next batch before they fetch the previous one (the reference's hot loop collects a
 * sparse list per cube and batch, main_reconstruct.py:126-160): sn_mark records point `slot` (0..7) on the context's stream;
 * sn_memcpy_d2h_after copies on a second stream as soon as that point has been reached and returns when the copy is done - work
 * enqueued on the context's stream AFTER the mark keeps running meanwhile (sn_memcpy_d2h would wait for all of it). */
SN_API int sn_mark(sn_ctx *ctx, int slot);
SN_API int sn_memcpy_d2h_after(sn_ctx *ctx, int slot, void *dst, const void *src_dev, size_t bytes);
/* The HIP stream (hipStream_t) every asynchronous entry point of this context is ordered on, for interop: record / wait
 * events on it, or wrap it (e.g. torch.cuda.ExternalStream) to order collectives against the kernels without host syncs. */
SN_API void *sn_stream(sn_ctx *ctx);
/* Same as sn_cvc_forward with every array already in HBM. n*n_vp <= max_samples. mean6 is host. */
SN_API int sn_cvc_forward_dev(sn_ctx *ctx, int n, int n_vp, const int64_t *view_pairs_dev, const float *xyz_dev,
                       const float *resol_dev, const float *mean6, const float *w_dev, float *fused_dev,
                       float *unfused_dev, float *cvc_out_dev);
SN_API int sn_cvc_dev(sn_ctx *ctx, int n, int n_vp, const int64_t *view_pairs_dev, const float *xyz_dev,
               const float *resol_dev, const float *mean6, float *out_dev);
SN_API int sn_forward_dev(sn_ctx *ctx, int n, int n_vp, const float *X_dev, const float *w_dev, float *fused_dev,
                   float *unfused_dev);

/* ---- post-pass of the loop body (main_reconstruct.py:153-160) ------------------- */
/* rayPooling.rayPooling_1cube_numpy (utils/rayPooling.py:143-260) for n cubes at once: pred (n,s,s,s) float32
 * probabilities >= 0 (rounded to float16 inside, as append_dense_2sparseList does at utils/sparseCubes.py:136 before
 * the call), view_pairs (n,n_vp,2) -> votes (n,s,s,s) uint8 (max 2*n_vp). use_thresh = 0 is prediction_thresh=None;
 * otherwise voxels with fp16(pred) > fp16(min_prob) take part. Needs sn_set_cameras only. SN_ERR_ARG if a projected
 * pixel / depth bin falls outside the int32 range (a cube on the camera plane; the reference has no such limit). */
SN_API int sn_ray_pool(sn_ctx *ctx, int n, int n_vp, const int64_t *view_pairs, const float *xyz, const float *resol,
                const float *pred, int use_thresh, float min_prob, unsigned char *votes);
/* Device-resident, asynchronous; the range error is reported by the next sn_synchronize. votes_dev (and votes_ws_dev of
 * sn_dense2sparse_dev) must be 4-byte aligned: the votes are added a 32-bit word at a time (s^3 is a multiple of 4, so
 * every cube's votes then start on a word). pred_dev may have any float alignment; 16-byte aligned cubes are read faster. */
SN_API int sn_ray_pool_dev(sn_ctx *ctx, int n, int n_vp, const int64_t *view_pairs_dev, const float *xyz_dev,
                    const float *resol_dev, const float *pred_dev, int use_thresh, float min_prob,
                    unsigned char *votes_dev);

/* sparseCubes.dense2sparse (utils/sparseCubes.py:9-77) keyword arguments. */
typedef struct sn_sparse_cfg {
    float min_prob;          /* compared in float16, as numpy does for a float16 array */
    int rayPool_thresh;
    int enable_centerCrop;
    int cube_Dcenter;        /* used when enable_centerCrop != 0; (s - cube_Dcenter) / 2 voxels are cut on each side */
    int enable_rayPooling;
} sn_sparse_cfg;
/* pred (n,s,s,s) float32 fused probabilities, rgb (n,3,s,s,s) uint8 (sn_color_fuse's output; may be NULL) ->
 * packed voxel lists of all cubes, cube after cube, voxels in ascending flat index of the (cropped) cube:
 *   offsets (n+1) int64: cube i owns [offsets[i], offsets[i+1]); empty cubes have zero length (the reference skips them)
 *   ijk (total,3) uint8 | pred16 (total) float16 bits | rgb_out (total,3) uint8 | votes_out (total) uint8
 * Output arrays must hold n*Dc^3 entries (Dc = cube_Dcenter when cropping, else s); rgb_out / votes_out may be NULL.
 * votes_out is filled only when enable_rayPooling. The caller shifts xyz by resol*(s-Dc)/2 (sparseCubes.py:55). */
SN_API int sn_dense2sparse(sn_ctx *ctx, int n, int n_vp, const int64_t *view_pairs, const float *xyz, const float *resol,
                    const float *pred, const unsigned char *rgb, const sn_sparse_cfg *cfg, int64_t *offsets,
                    unsigned char *ijk, uint16_t *pred16, unsigned char *rgb_out, unsigned char *votes_out);
/* Same with every array in HBM (offsets too); asynchronous. votes_ws_dev (n,s,s,s) uint8 scratch is required when
 * enable_rayPooling. */
SN_API int sn_dense2sparse_dev(sn_ctx *ctx, int n, int n_vp, const int64_t *view_pairs_dev, const float *xyz_dev,
                        const float *resol_dev, const float *pred_dev, const unsigned char *rgb_dev,
                        const sn_sparse_cfg *cfg, unsigned char *votes_ws_dev, int64_t *offsets_dev,
                        unsigned char *ijk_dev, uint16_t *pred16_dev, unsigned char *rgb_out_dev,
                        unsigned char *votes_out_dev);

/* ---- cross-cube post-pass (main_reconstruct.py:172-176, main.py:37-43) ---------------------------------------------------------------------
 * Both work on the packed voxel lists sn_dense2sparse produces: offsets (n+1) int64 (cube i owns voxels [offsets[i], offsets[i+1]); offsets[0] = 0,
 * non-decreasing), ijk (total,3) uint8 voxel indices inside the cube, each < Dc (the bit-row width, 1..64: cube_Dcenter for dense2sparse's lists),
 * cube_ijk (n,3) uint32 cube indices. Host forms validate the table and the ijk; _dev forms take total = offsets[n] and report a bad table or ijk
 * through the next sn_synchronize (the cubes concerned are skipped). Both forms return when the work is done.
 *
 * denoising.denoise_crossCubes (utils/denoising.py:150-184): mask (total) uint8 0/1 -> out (total) uint8 0/1. A voxel is kept iff it is masked and
 * its 26-connected component inside its cube holds a voxel v that coincides with a masked voxel u of a neighbouring cube, v == u + (D_cube/2)*shift.
 * Only cubes with a masked voxel enter the ijk -> cube map; for a repeated ijk the last such cube wins; every other cube keeps nothing.
 * D_cube (>= 2) is taken as given: main_reconstruct.py:175 passes cube_D, adapthresh cube_Dcenter. */
SN_API int sn_denoise(sn_ctx *ctx, int n, int Dc, int D_cube, const int64_t *offsets, const unsigned char *ijk, const uint32_t *cube_ijk,
                      const unsigned char *mask, unsigned char *out);
SN_API int sn_denoise_dev(sn_ctx *ctx, int n, int Dc, int D_cube, long long total, const int64_t *offsets_dev, const unsigned char *ijk_dev,
                          const uint32_t *cube_ijk_dev, const unsigned char *mask_dev, unsigned char *out_dev);

/* adapthresh.adapthresh's numeric arguments (utils/adapthresh.py:91-94; min_probThresh is accepted and ignored there, so it is absent here). */
typedef struct sn_adapthresh_cfg {
    int N_refine_iter;
    int D_cube;                /* cube_Dcenter at main.py:39: the half-cube selections are [D_cube/2, D_cube) and [0, D_cube/2) */
    double init_probThresh;    /* initial mask: float16(pred) >= float16(init_probThresh) AND votes >= rayPool_thresh */
    double max_probThresh;
    double rayPool_thresh;
    double beta;
} sn_adapthresh_cfg;
/* The whole refinement device-resident: initial mask, its denoised form, then N_refine_iter Jacobi iterations (every cube reads the thresholds and
 * masks of the previous one; float16 cost accumulated in the reference's order as numpy 2 rounds it). pred16 (total) float16
 * bits; votes (total) uint8 or NULL (no vote filter). Outputs, each optional (NULL): init_denoised (total), thresh (N_refine_iter, n) float64 -
 * every cube's threshold after each iteration, masks (N_refine_iter, total) - the cumulative masks, denoised (N_refine_iter, total) - their
 * denoised form (the iter{k}.ply content), choice (N_refine_iter, n) int8 - the argmin of each active cube's cost (0: +0.1, 1: 0, 2: -0.1), -1 for
 * the cubes outside the active set (empty initial mask, or not their ijk's map entry). */
SN_API int sn_adapthresh(sn_ctx *ctx, int n, int Dc, const sn_adapthresh_cfg *cfg, const int64_t *offsets, const unsigned char *ijk,
                         const uint16_t *pred16, const unsigned char *votes, const uint32_t *cube_ijk, unsigned char *init_denoised,
                         double *thresh, unsigned char *masks, unsigned char *denoised, signed char *choice);
SN_API int sn_adapthresh_dev(sn_ctx *ctx, int n, int Dc, const sn_adapthresh_cfg *cfg, long long total, const int64_t *offsets_dev,
                             const unsigned char *ijk_dev, const uint16_t *pred16_dev, const unsigned char *votes_dev,
                             const uint32_t *cube_ijk_dev, unsigned char *init_denoised_dev, double *thresh_dev, unsigned char *masks_dev,
                             unsigned char *denoised_dev, signed char *choice_dev);

/* ---- oriented normals and de-duplication of the output cloud ---------------------------------------------------------
 * On the packed sparse lists of the cross-cube post-pass (offsets, ijk, cube_ijk, mask as sn_denoise takes them). World cell of a voxel:
 * g = cube_ijk * stride_vox + ijk per axis (stride_vox = cube_Dcenter * cube_overlapping_ratio, the cube stride in voxels, >= 1); the occupied set O
 * holds the distinct cells of the masked voxels of all cubes. Masked cells must satisfy g + radius < 2^21 per axis (SN_ERR_ARG otherwise); cells with
 * a negative coordinate do not exist: windows at the lattice's edge simply miss there.
 *
 * sn_normals: for every masked voxel, N = { d in [-radius, radius]^3 : g + d in O } (d = 0 included), radius 1, 2 or 3.
 *   moments (total,10) int32, optional: |N|, sum d (x y z), sum d d^T (xx xy xz yy yz zz) - exact; ten zeros for an unmasked voxel.
 *   normals (total,3) float32, optional: (0,0,0) when |N| < min_neighbours or the voxel is unmasked; else the unit eigenvector of the smallest
 *   eigenvalue of |N| * sum d d^T - (sum d)(sum d)^T, solved in float64, oriented toward c = (sum_k cameraTs[view_idx[cube][k]]) / views_per_cube
 *   (float64, summed in index order): with x = float64(float32(ijk) * resol + xyz) of the voxel's cube, the normal is negated when
 *   (nx*dx + ny*dy) + nz*dz < 0, d = c - x; rounded to float32 once, after that. Where the two smallest eigenvalues coincide the direction is
 *   unspecified (finite, unit length). cube_xyz (n,3) / cube_resol (n) float32, view_idx (n, views_per_cube) int32 each in [0, n_views)
 *   (SN_ERR_ARG otherwise), cameraTs (n_views,3) float64: read only when normals is given. All cube_resol must be equal: the host form checks it
 *   (SN_ERR_ARG), the device form takes it on trust.
 * sn_unique_voxels: keep (total) uint8 = 1 iff the voxel is masked and has the smallest packed index among the masked voxels of its world cell.
 * Both are deterministic. The workspace belongs to the context (grown on demand); a bad offsets table is SN_ERR_ARG in both forms; all four
 * return when the work is done. total <= 2^28. */
typedef struct sn_normals_cfg {
    int radius;                /* 1, 2 or 3 */
    int min_neighbours;        /* >= 1; below it the normal is zero */
    int stride_vox;            /* cube stride in voxels */
    int n_views;               /* rows of cameraTs */
    int views_per_cube;        /* columns of view_idx: 2 * N_viewPairs4inference for viewPair_np */
} sn_normals_cfg;
SN_API int sn_normals(sn_ctx *ctx, int n, const sn_normals_cfg *cfg, const int64_t *offsets, const unsigned char *ijk, const uint32_t *cube_ijk,
                      const unsigned char *mask, const float *cube_xyz, const float *cube_resol, const int32_t *view_idx, const double *cameraTs,
                      float *normals, int32_t *moments);
SN_API int sn_normals_dev(sn_ctx *ctx, int n, const sn_normals_cfg *cfg, long long total, const int64_t *offsets_dev, const unsigned char *ijk_dev,
                          const uint32_t *cube_ijk_dev, const unsigned char *mask_dev, const float *cube_xyz_dev, const float *cube_resol_dev,
                          const int32_t *view_idx_dev, const double *cameraTs_dev, float *normals_dev, int32_t *moments_dev);
SN_API int sn_unique_voxels(sn_ctx *ctx, int n, int stride_vox, const int64_t *offsets, const unsigned char *ijk, const uint32_t *cube_ijk,
                            const unsigned char *mask, unsigned char *keep);
SN_API int sn_unique_voxels_dev(sn_ctx *ctx, int n, int stride_vox, long long total, const int64_t *offsets_dev, const unsigned char *ijk_dev,
                                const uint32_t *cube_ijk_dev, const unsigned char *mask_dev, unsigned char *keep_dev);

/* ---- connected components of the output cloud: removing floaters ----------------------------------------------------
 * On the packed sparse lists exactly as sn_unique_voxels takes them. World cell of a voxel: g = cube_ijk * stride_vox + ijk per axis; O holds the
 * distinct cells of the masked voxels of all cubes. Two distinct cells are adjacent iff max |d| <= 1 per axis and sum |d| <= 1, 2 or 3 for
 * connectivity 6, 18 or 26 (scipy.ndimage.generate_binary_structure(3, 1 | 2 | 3)); a component K is a class of the transitive closure on O -
 * across cubes. first(K) = the smallest packed index among the masked voxels whose cell lies in K; the components are numbered 0 .. C-1 by
 * ascending first(K).
 *   label (total) int32: the component number of the voxel's cell, -1 for an unmasked voxel.
 *   cells (total) int32: |K| counted in DISTINCT cells (a cell listed by several cubes, or twice in one cube, counts once); 0 for an unmasked voxel.
 *   keep  (total) uint8: mask && cells >= min_cells.
 *   n_components (required): C. label, cells and keep are each optional (NULL).
 * SN_ERR_ARG, nothing written: a bad offsets table, connectivity not 6 / 18 / 26, min_cells < 1, stride_vox < 1, a masked cell with
 * g + 1 >= 2^21 on an axis, total > 2^28. Cells with a negative coordinate do not exist: a neighbour probe there misses. n == 0, total == 0 or an
 * all-false mask give C = 0. The result is a function of the partition only, so it is bit-identical from run to run. The workspace belongs to
 * the context (grown on demand); both forms return when the work is done. */
typedef struct sn_components_cfg {
    int stride_vox;            /* cube stride in voxels */
    int connectivity;          /* 6, 18 or 26 */
    int min_cells;             /* >= 1: keep = the component has at least this many cells */
} sn_components_cfg;
SN_API int sn_components(sn_ctx *ctx, int n, const sn_components_cfg *cfg, const int64_t *offsets, const unsigned char *ijk, const uint32_t *cube_ijk,
                         const unsigned char *mask, int32_t *label, int32_t *cells, unsigned char *keep, long long *n_components);
SN_API int sn_components_dev(sn_ctx *ctx, int n, const sn_components_cfg *cfg, long long total, const int64_t *offsets_dev, const unsigned char *ijk_dev,
                             const uint32_t *cube_ijk_dev, const unsigned char *mask_dev, int32_t *label_dev, int32_t *cells_dev,
                             unsigned char *keep_dev, long long *n_components);

/* ---- surface mesh of the oriented output cloud: surface nets on the world lattice -------------------------------------
 * On the packed sparse lists (offsets, ijk, cube_ijk, mask as the two entries above take them) plus normals (total,3) float32 as the normals entry
 * writes them: zero = no normal. The oriented cells P are the world cells whose owner - the smallest packed index among the cell's masked
 * voxels - has a normal with a non-zero component; nq = rint(float64(n) * 16384) per component. At a lattice point c,
 * F(c) = sum over p in P, d = c - p in [-radius, radius]^3, of w(d) * (nq_p . d) and W(c) = sum of w(d), w(d) = prod (radius + 1 - |d_k|), both
 * int64 and exact; c is defined iff W > 0 and inside iff F < 0. A lattice edge (c, c + e_a) is active iff both ends are defined and exactly one is
 * inside; it emits a quad iff a cell of P lies within Chebyshev distance `reach` of an end. One vertex per 2x2x2 group of lattice points (dual
 * cube m) that an emitted quad uses, at the float64 mean of the crossings t = F0 / (F0 - F1) of all its active edges. The order of vertices and
 * quads, the winding (face normals point from inside to outside) and vert_src are canonical: the result equals the numpy restatement
 * tests/mesh_ref.py, the integers exactly. Masked voxels: every normal component finite and |.| <= 2, cell + 8 < 2^21 per axis (SN_ERR_ARG).
 *   verts_mm (V,3) float32 = float32(origin + resol * verts_lattice); verts_lattice (V,3) float64; vert_cell (V,3) int32 = m;
 *   vert_src (V) int64: packed index of the owner of the cell of P nearest the dual cube's centre (-1: none within m + {-1..2}^3);
 *   quads (Q,4) int32 vertex indices. Every output is optional (NULL). The caller sizes them: they hold cap_verts vertices and cap_quads quads;
 *   n_verts / n_quads (required) receive V and Q. When a cap is short nothing is written, the counts say what is needed and the status is
 *   SN_ERR_ARG. Vertex and quad indices are int32. The counts are kept below 2^31 by a limit on the scene, not on the counts themselves: the
 *   oriented cells and their 26 neighbours may occupy at most 2^23 bricks of 4^3 lattice points (64 vertices and 192 quads a brick at most),
 *   beyond that SN_ERR_ARG - a sufficient condition, so a scene past it is refused even if its mesh would have fitted.
 *   Deterministic; the workspace belongs to the context (grown on demand); both forms return when the work is done. total <= 2^28. */
typedef struct sn_mesh_cfg {
    int radius;                /* window radius of the field: 1, 2 or 3 */
    int reach;                 /* 0 .. radius: how far from a cell of P an active edge may lie and still emit its quad */
    int stride_vox;            /* cube stride in voxels */
    double origin[3];          /* mm position of lattice point (0,0,0) */
    double resol;              /* mm per cell */
} sn_mesh_cfg;
SN_API int sn_mesh(sn_ctx *ctx, int n, const sn_mesh_cfg *cfg, const int64_t *offsets, const unsigned char *ijk, const uint32_t *cube_ijk,
                   const unsigned char *mask, const float *normals, long long cap_verts, long long cap_quads, float *verts_mm, double *verts_lattice,
                   int32_t *vert_cell, int64_t *vert_src, int32_t *quads, long long *n_verts, long long *n_quads);
SN_API int sn_mesh_dev(sn_ctx *ctx, int n, const sn_mesh_cfg *cfg, long long total, const int64_t *offsets_dev, const unsigned char *ijk_dev,
                       const uint32_t *cube_ijk_dev, const unsigned char *mask_dev, const float *normals_dev, long long cap_verts, long long cap_quads,
                       float *verts_mm_dev, double *verts_lattice_dev, int32_t *vert_cell_dev, int64_t *vert_src_dev, int32_t *quads_dev,
                       long long *n_verts, long long *n_quads);

/* ---- surface samples of a triangle mesh at the evaluation density ----------------------------------------------------
 * The first step of the DTU protocol for a mesh (sample, reduce, PointCompare). verts (n_verts,3) float64, faces (n_faces,3) int32, dst finite
 * and > 0. Float arithmetic is fp64 without contraction; the squared length of an edge e is (ex*ex + ey*ey) + ez*ez. For face f with corners A,
 * B, C in face order: L2 = the largest squared length of B-A, C-A, C-B; q = L2 / (dst*dst); n_f = the smallest integer >= 1 with
 * float64(n*n) >= q. The face yields n_f^2 samples, the centroids of its n_f^2 congruent sub-triangles: for k in [0, n^2), t = isqrt(k),
 * w = k - t^2, c = w >> 1; w even: beta = 3t - 3c + 1, gamma = 3c + 1; w odd: beta = 3t - 3c - 1, gamma = 3c + 2; u = float64(beta) /
 * float64(3n), v = float64(gamma) / float64(3n); per component p = A + ((B-A)*u + (C-A)*v). Every point of the face lies within 2/3 dst of
 * a sample. Samples come in face order, then k: points (M,3) float64, tri (M) int32 the face of each sample, M = sum n_f^2; either output may
 * be NULL. The result equals the numpy restatement tests/meshsample_ref.py bit for bit.
 *   SN_ERR_ARG, nothing written, the error text naming the first offending face: a face index outside [0, n_verts); a non-finite coordinate
 *   of a referenced vertex; n_f > 32768; M > 2^31 - 1; also dst not finite or not > 0. A degenerate face is legal (n = 1, one sample at A);
 *   n_faces = 0 gives M = 0. The outputs hold cap_points samples; *n_points (required) receives M. When cap_points < M nothing is written,
 *   *n_points = M and the status is SN_ERR_ARG. Deterministic; the workspace belongs to the context; both forms return when the work is done. */
SN_API int sn_mesh_sample(sn_ctx *ctx, int n_verts, const double *verts, int n_faces, const int32_t *faces, double dst, long long cap_points,
                          double *points, int32_t *tri, long long *n_points);
SN_API int sn_mesh_sample_dev(sn_ctx *ctx, int n_verts, const double *verts_dev, int n_faces, const int32_t *faces_dev, double dst,
                              long long cap_points, double *points_dev, int32_t *tri_dev, long long *n_points);

/* ---- a triangle mesh made smaller: vertex clustering on a coarser lattice ---------------------------------------------
 * verts (n_verts,3) float64 in lattice cells (sn_mesh's verts_lattice), faces (n_faces,3) int32; cfg->cell = k in 2..64 lattice cells per
 * cluster cell and axis. A vertex is referenced iff a face names it; an unreferenced vertex is not looked at. Per component of a referenced
 * vertex q = int64(rint(v * 256)) (requires -4 <= v < 2^21 - 8) and the cluster cell c = floor((q + 1024) / (256 k)). A cluster is the set of
 * referenced vertices of one cell, its owner its smallest vertex index; clusters are numbered by ascending owner (P of them; P >= 2^21 is
 * refused). Per cluster: S = the int64 sums of q, n = its size, rep = the member with the smallest (d, index), d = sum over the axes of
 * (2 (q - o) - 256 k)^2 with o = c * 256 k - 1024: the member nearest the cell's centre. A face whose three cluster numbers are not distinct
 * collapses; a surviving face is rotated to its smallest number first (orientation kept); of the faces with one rotated triple the smallest
 * input index survives (the same clusters in the opposite orientation are another face). The output vertices are the clusters a surviving
 * face uses, in number order; the output faces the surviving faces in input order:
 *   verts_lattice (C,3) float64: placement 0 (float64(S) / float64(n)) / 256, placement 1 verts[rep] bit for bit;
 *   verts_mm (C,3) float32 = float32(origin + resol * verts_lattice) in float64 without contraction; vert_rep (C) int32 = rep: colour,
 *   normal and source voxel of an output vertex are a gather by the caller; vert_count (C) int32 = n; faces_out (G,3) int32; face_src (G)
 *   int32 the input face; vert_cluster (n_verts) int32 the output vertex of an input vertex's cluster, -1 when it is unreferenced or its
 *   cluster is used by no surviving face. Every member lies within sqrt(3) k + 1/256 cells of its output vertex.
 * Every output is optional (NULL) except the two counts. The outputs hold cap_verts vertices and cap_faces faces; when one is short nothing is
 * written, the counts say what is needed and the status is SN_ERR_ARG. SN_ERR_ARG too, nothing written, the text naming the first offending
 * face: a face index outside [0, n_verts); a referenced coordinate outside the range (or not a number); also cell, placement, resol (finite,
 * > 0), origin (finite), n_verts or n_faces > 2^28, P >= 2^21 (choose a larger cell). n_faces = 0 gives C = G = 0 and vert_cluster all -1.
 * All sums are integers: the result equals the numpy restatement tests/meshsimplify_ref.py bit for bit, on every run. The workspace belongs to
 * the context (grown on demand); both forms return when the work is done. */
typedef struct sn_mesh_simplify_cfg {
    int cell;                  /* k: lattice cells per cluster cell and axis, 2 .. 64 */
    int placement;             /* 0: the mean of the members; 1: the member nearest the cell's centre */
    double origin[3];          /* mm position of lattice point (0,0,0) */
    double resol;              /* mm per cell */
} sn_mesh_simplify_cfg;
SN_API int sn_mesh_simplify(sn_ctx *ctx, const sn_mesh_simplify_cfg *cfg, int n_verts, const double *verts, int n_faces, const int32_t *faces,
                            long long cap_verts, long long cap_faces, float *verts_mm, double *verts_lattice, int32_t *vert_rep,
                            int32_t *vert_count, int32_t *faces_out, int32_t *face_src, int32_t *vert_cluster, long long *n_out_verts,
                            long long *n_out_faces);
SN_API int sn_mesh_simplify_dev(sn_ctx *ctx, const sn_mesh_simplify_cfg *cfg, int n_verts, const double *verts_dev, int n_faces,
                                const int32_t *faces_dev, long long cap_verts, long long cap_faces, float *verts_mm_dev,
                                double *verts_lattice_dev, int32_t *vert_rep_dev, int32_t *vert_count_dev, int32_t *faces_out_dev,
                                int32_t *face_src_dev, int32_t *vert_cluster_dev, long long *n_out_verts, long long *n_out_faces);

/* ---- a mesh made smooth: Taubin lambda|mu smoothing with the uniform umbrella operator, in fixed point ----------------
 * verts (n_verts,3) float64 in lattice cells (sn_mesh's or sn_mesh_simplify's verts_lattice), faces (n_faces,nv) int32 with nv = 3 or 4; a quad's
 * four sides are its edges, no diagonal is invented. A vertex is referenced iff a face names it; an unreferenced vertex is not looked at (it may
 * be NaN). Per component of a referenced vertex q = int64(rint(v * 65536)) (requires -4 <= v < 2^21 - 8); QMIN = -4 * 65536, QMAX =
 * (2^21 - 8) * 65536 - 1. Every face gives the sides (f[i], f[(i + 1) % nv]); a side with equal ends is ignored; an edge is an unordered pair
 * {a, b}, its count the number of sides on it in either direction; E edges; a boundary edge has count 1, a non-manifold one count > 2. Per
 * vertex: degree = its edges, bdegree = its boundary edges, a boundary vertex has bdegree > 0. The neighbours N(i) of a vertex: boundary 2
 * (free) all edge neighbours; 0 (fixed) the same, but a boundary vertex does not move; 1 (curve) a boundary vertex only its neighbours across
 * boundary edges (d = bdegree), every other vertex all of them: the rim of an open sheet smooths as a curve. A vertex with d = 0 does not move.
 * One pass with factor w is Jacobi - every vertex reads the positions of before the pass - and per axis, S = the sum of q over N(i):
 *   mean = floor((2 S + d) / (2 d)),   q' = min(max(q + ((w * (mean - q) + 32768) >> 16), QMIN), QMAX)      (int64, arithmetic shift).
 * One iteration is a pass with lam_q16, then one with mu_q16 unless that is 0 (plain Laplacian smoothing). Indices do not change: faces,
 * colours and normals carry over. Outputs, each optional (NULL) except counts:
 *   verts_lattice (n_verts,3) float64 = float64(q) / 65536 of a referenced vertex, the input's bits of an unreferenced one;
 *   verts_mm (n_verts,3) float32 = float32(origin + resol * verts_lattice) in float64 without contraction; vert_degree (n_verts) int32;
 *   vert_flags (n_verts) uint8: bit 0 referenced, bit 1 boundary vertex, bit 2 end of a non-manifold edge;
 *   counts[4]: E, boundary edges, non-manifold edges, referenced vertices.
 * iterations = 0 quantises and reports the topology. SN_ERR_ARG, nothing written but counts (zeros): a face index outside [0, n_verts) or a
 * referenced coordinate outside the range (or not a number), the text naming the first offending face; iterations outside 0 .. 1000, a factor
 * outside [-65536, 65536], boundary not 0 / 1 / 2, nv not 3 or 4, resol (finite, > 0), origin (finite), n_verts or n_faces > 2^28; a vertex
 * of 2^24 or more edges (named; it keeps 2 S + d inside int64); 2^30 or more edges. n_faces = 0: nothing is referenced, verts_lattice is the
 * input, the counts are 0. All sums are integers: the result equals the numpy restatement tests/meshsmooth_ref.py bit for bit, on every run.
 * The workspace belongs to the context (grown on demand); both forms return when the work is done. */
typedef struct sn_mesh_smooth_cfg {
    int iterations;            /* 0 .. 1000 */
    int lam_q16, mu_q16;       /* the two factors times 65536, each in [-65536, 65536]; mu_q16 = 0: no second pass */
    int boundary;              /* 0: boundary vertices fixed; 1: they smooth along the boundary curve; 2: free */
    double origin[3];          /* mm position of lattice point (0,0,0) */
    double resol;              /* mm per cell */
} sn_mesh_smooth_cfg;
SN_API int sn_mesh_smooth(sn_ctx *ctx, const sn_mesh_smooth_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv, const int32_t *faces,
                          float *verts_mm, double *verts_lattice, int32_t *vert_degree, unsigned char *vert_flags, long long *counts);
SN_API int sn_mesh_smooth_dev(sn_ctx *ctx, const sn_mesh_smooth_cfg *cfg, int n_verts, const double *verts_dev, int n_faces, int nv,
                              const int32_t *faces_dev, float *verts_mm_dev, double *verts_lattice_dev, int32_t *vert_degree_dev,
                              unsigned char *vert_flags_dev, long long *counts);

/* ---- a mesh's small holes filled: closed boundary loops, each capped by a fan around its centroid ------------------------
 * The inputs are sn_mesh_smooth's: verts (n_verts,3) float64 in lattice cells, faces (n_faces,nv) int32 with nv = 3 or 4, a quad's four sides
 * its edges; referenced vertices, q = int64(rint(v * 65536)) and its range, sides, edges, counts, boundary (count 1) and non-manifold (count
 * > 2) edges as there. A boundary half-edge is the one side (p -> r) on a boundary edge, in its face's direction; its third vertex s is the
 * face's next corner after r (f[(k + 2) % nv] for side k). Per vertex out / in = the boundary half-edges leaving / entering it; a vertex is
 * simple iff out = 1, in = 1 and it is no end of a non-manifold edge. A boundary component is a maximal set of vertices joined by boundary
 * edges, its root its smallest vertex, its length n its number of boundary half-edges. It is a simple loop iff all its vertices are simple
 * (then p -> r is one directed cycle of n vertices), else complex and left alone; a simple loop with n > max_len is long and left alone. Per
 * axis the centroid c = floor((2 S + n) / (2 n)), S the int64 sum of q over the loop. With orientation 0 every half-edge of the loop votes:
 * d1 = float64(q[r] - q[p]), d2 = float64(q[s] - q[p]), d3 = float64(c - q[p]), a = d1 x d2, b = d1 x d3 (x = y*z' - z*y', y = z*x' - x*z',
 * z = x*y' - y*x'), dot = (a.x*b.x + a.y*b.y) + a.z*b.z in float64 without contraction; the vote is "hole" iff dot < 0 (the centroid lies
 * across the edge from the face); the loop is a hole iff 2 * votes > n, else a rim and left alone. With orientation 1 every simple loop within
 * max_len is filled. The filled loops, ranked by ascending root, give H new vertices n_verts + rank at c / 65536, and one triangle
 * (r, p, n_verts + rank) per half-edge p -> r, ordered by ascending p (T of them). Outputs, each optional (NULL) except counts:
 *   new_verts_lattice (H,3) float64; new_verts_mm (H,3) float32 = float32(origin + resol * lattice) in float64 without contraction;
 *   loop_root (H) int32, loop_len (H) int32: colour, normal and source voxel of a new vertex are taken from its root by the caller;
 *   new_faces (T,3) int32 into the concatenation [verts; new_verts]; the old vertices and faces are neither touched nor returned;
 *   vert_loop (n_verts) uint8: 0 not on a boundary edge, 1 on a filled loop, 2 on a long loop, 3 on a rim, 4 on a complex component;
 *   counts[8]: E, boundary edges, boundary components, filled loops H, long loops, rims, complex components, new triangles T.
 * The outputs hold cap_verts new vertices and cap_faces new triangles (T <= nv * n_faces and H <= T / 3 always suffice); when one is short
 * nothing is written, the counts say what is needed and the status is SN_ERR_ARG. SN_ERR_ARG too, nothing written but counts (zeros), in
 * sn_mesh_smooth's words: a face index outside [0, n_verts) or a referenced coordinate outside the range (or not a number), the text naming
 * the first offending face; nv not 3 or 4, resol, origin, n_verts or n_faces > 2^28, 2^30 or more edges; and max_len outside 3 .. 65536,
 * orientation not 0 or 1, a negative cap. n_faces = 0: all counts 0, nothing written. Integers and one fixed-order float64 expression: the
 * result equals the numpy restatement tests/meshfill_ref.py bit for bit, on every run. The workspace belongs to the context (grown on demand);
 * both forms return when the work is done. */
typedef struct sn_mesh_fill_cfg {
    int max_len;               /* the longest loop that is filled, in edges: 3 .. 65536 */
    int orientation;           /* 0: holes only (the vote); 1: any simple loop */
    double origin[3];          /* mm position of lattice point (0,0,0) */
    double resol;              /* mm per cell */
} sn_mesh_fill_cfg;
SN_API int sn_mesh_fill(sn_ctx *ctx, const sn_mesh_fill_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv, const int32_t *faces,
                        long long cap_verts, long long cap_faces, float *new_verts_mm, double *new_verts_lattice, int32_t *loop_root,
                        int32_t *loop_len, int32_t *new_faces, unsigned char *vert_loop, long long *counts);
SN_API int sn_mesh_fill_dev(sn_ctx *ctx, const sn_mesh_fill_cfg *cfg, int n_verts, const double *verts_dev, int n_faces, int nv,
                            const int32_t *faces_dev, long long cap_verts, long long cap_faces, float *new_verts_mm_dev,
                            double *new_verts_lattice_dev, int32_t *loop_root_dev, int32_t *loop_len_dev, int32_t *new_faces_dev,
                            unsigned char *vert_loop_dev, long long *counts);

/* ---- a mesh's own normals, area-weighted, with its exact area and volume --------------------------------------------------
 * The inputs are sn_mesh_smooth's: verts (n_verts,3) float64 in lattice cells, faces (n_faces,nv) int32 with nv = 3 or 4; referenced vertices and
 * q = int64(rint(v * 65536)) with its range as there. No origin or cell size: unit normals do not depend on them, and the caller scales the two
 * measures. Face vector N_f, exact integers below 2^78: a triangle's (q_b - q_a) x (q_c - q_a), a quad's (q_c - q_a) x (q_d - q_b) - the sum of
 * the vectors of the triangles (a,b,c), (a,c,d). Vertex vector N_v = the sum of N_f over every corner that names the vertex (a face that names
 * it twice adds twice): area weights, exact. The unit rule, for faces and vertices alike, of an integer triple: m = the largest magnitude; m = 0
 * gives (0,0,0); else s = max(0, bitlength(m) - 52), the components shifted right by s (floor) are exact float64 x, y, z,
 * l = sqrt((x*x + y*y) + z*z) in this order without contraction, the normal is float32(x / l), float32(y / l), float32(z / l).
 * area2 = the sum over the faces of int(rint(l_f)) << s_f, twice the area in units of 2^-32 cell^2, an integer by rule: the sum does not depend
 * on the order. vol6 = the sum of q_a . (q_b x q_c) over the triangles, a quad's being (a,b,c) and (a,c,d): six times the signed volume in
 * units of 2^-48 cell^3. Outputs, the two arrays optional (NULL):
 *   face_normals (n_faces,3) float32; vert_normals (n_verts,3) float32, zero rows for unreferenced vertices;
 *   counts[4]: faces with N_f = 0, referenced vertices with N_v = 0, referenced vertices, triangles n_faces * (nv - 2);
 *   sums[6]: area2, then vol6, each three 64-bit limbs, least significant first, two's complement.
 * n_faces = 0: counts and sums 0, vert_normals all zero, nothing else written. SN_ERR_ARG, nothing written but counts and sums (zeros), in
 * sn_mesh_smooth's words: a face index outside [0, n_verts) or a referenced coordinate outside the range (or not a number), the text naming the
 * first offending face; nv not 3 or 4, n_verts or n_faces > 2^28. Every sum is an integer: the result equals the restatement
 * tests/meshnormals_ref.py bit for bit, on every run. The workspace belongs to the context (grown on demand); both forms return when the work is
 * done. */
SN_API int sn_mesh_normals(sn_ctx *ctx, int n_verts, const double *verts, int n_faces, int nv, const int32_t *faces, float *face_normals,
                           float *vert_normals, long long *counts, unsigned long long *sums);
SN_API int sn_mesh_normals_dev(sn_ctx *ctx, int n_verts, const double *verts_dev, int n_faces, int nv, const int32_t *faces_dev,
                               float *face_normals_dev, float *vert_normals_dev, long long *counts, unsigned long long *sums);

/* ---- a mesh's faces made to turn one way, its pieces, their exact volumes, small pieces removed ---------------------------
 * The inputs are sn_mesh_smooth's: verts (n_verts,3) float64 in lattice cells, faces (n_faces,nv) int32 with nv = 3 or 4; referenced vertices,
 * q = int64(rint(v * 65536)) and its range, sides, edges and side counts as there. Side k of a face is p -> r = f[k] -> f[(k + 1) % nv]
 * (p = r: no side), its direction bit d = (p < r), its code 2 * face + d. A link is an edge with exactly two sides that belong to two
 * different faces f < g; it is inconsistent iff the two direction bits are equal. Boundary edges, edges with more than two sides and an edge
 * whose two sides are one face's are no links: pieces end there. Double cover: face f is the two nodes 2f (as given) and 2f + 1 (reversed);
 * every link with r = inconsistent unites (2f, 2g + r) and (2f + 1, 2g + 1 - r); root = the smallest node of a class. Per face comp =
 * root(2f) >> 1, the smallest face of its piece, rel = root(2f) & 1; the piece is non-orientable iff root(2f) = root(2f + 1) (then rel = 0
 * throughout and no face of it is flipped). Per piece: n_faces; n_rel = its faces with rel = 1; closed iff orientable and every one of the nv
 * corners of every face starts a side that lies on a link; vol6' = the sum over its faces of s * t, t = q_a . (q_b x q_c) of a triangle, of
 * (a,b,c) plus (a,c,d) for a quad, s = -1 iff rel: an exact integer. Sign of an orientable piece: sign 0 (majority) flipc = (n_rel >
 * n_faces - n_rel) - the fewer faces turn, a tie leaves the smallest face as it is; sign 1 (outward) flipc = (vol6' < 0) on a closed piece
 * with vol6' != 0, the majority rule on every other. flip(f) = rel ^ flipc. A flipped face keeps its first corner and reverses the rest,
 * (a,b,c) -> (a,c,b), (a,b,c,d) -> (a,d,c,b); an unflipped face is copied; face order and vertices are untouched. A piece is kept iff n_faces
 * >= min_faces; with keep_largest the piece with the most faces (the smallest id among equals) is kept as well. Outputs, each optional (NULL)
 * except counts:
 *   faces_out (n_faces,nv) int32; face_flip (n_faces) uint8; face_component (n_faces) int32; face_keep (n_faces) uint8;
 *   per piece at row comp, zero in the rows that are no piece's id: comp_faces (n_faces) int32; comp_flags (n_faces) uint8: 1 orientable,
 *   2 closed, 4 flipped, 8 kept; comp_vol6 (n_faces,3) uint64: vol6' negated iff flipc (a non-orientable piece: the sum of its faces as
 *   given), three 64-bit limbs, least significant first, two's complement, six times the signed volume in units of 2^-48 cell^3;
 *   counts[12]: E, boundary edges, non-manifold edges, links, inconsistent links, pieces, non-orientable pieces, closed pieces, flipped
 *   faces, flipped pieces, kept faces, kept pieces.
 * n_faces = 0: counts 0, nothing written. SN_ERR_ARG, nothing written but counts (zeros), in sn_mesh_smooth's words: a face index outside
 * [0, n_verts) or a referenced coordinate outside the range (or not a number), the text naming the first offending face; nv not 3 or 4,
 * n_verts or n_faces > 2^28, 2^30 or more edges; and sign not 0 or 1, min_faces < 0, keep_largest not 0 or 1. Non-manifold edges are not
 * split or paired, non-orientable pieces are reported and left alone, an open piece has no outward test, vertices that lose all their faces
 * stay, and self-intersections are sn_mesh_intersect's to find. Everything is an integer: the result equals the numpy restatement tests/meshorient_ref.py
 * byte for byte, on every run. The workspace belongs to the context (grown on demand); both forms return when the work is done. */
typedef struct sn_mesh_orient_cfg {
    int sign;                  /* 0: majority - the fewer faces of a piece turn; 1: outward - a closed piece turns iff its volume is negative */
    int min_faces;             /* >= 0: a piece of fewer faces is not kept */
    int keep_largest;          /* 0 / 1: the piece with the most faces is kept whatever min_faces says */
} sn_mesh_orient_cfg;
SN_API int sn_mesh_orient(sn_ctx *ctx, const sn_mesh_orient_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv, const int32_t *faces,
                          int32_t *faces_out, unsigned char *face_flip, int32_t *face_component, unsigned char *face_keep, int32_t *comp_faces,
                          unsigned char *comp_flags, unsigned long long *comp_vol6, long long *counts);
SN_API int sn_mesh_orient_dev(sn_ctx *ctx, const sn_mesh_orient_cfg *cfg, int n_verts, const double *verts_dev, int n_faces, int nv,
                              const int32_t *faces_dev, int32_t *faces_out_dev, unsigned char *face_flip_dev, int32_t *face_component_dev,
                              unsigned char *face_keep_dev, int32_t *comp_faces_dev, unsigned char *comp_flags_dev,
                              unsigned long long *comp_vol6_dev, long long *counts);

/* ---- a mesh's self-intersections, exactly -----------------------------------------------------------------------------------
 * The inputs are sn_mesh_smooth's: verts (n_verts,3) float64 in lattice cells, faces (n_faces,nv) int32 with nv = 3 or 4; referenced vertices,
 * q = int64(rint(v * 65536)) and its range -4 <= v < 2^21 - 8 as there. Every difference of two q is below 2^38 and every 3x3 determinant of
 * differences below 2^117: all arithmetic is exact in 128-bit integers, and only signs are used.
 *   1 triangles  a triangle face is one triangle, a quad (a,b,c,d) is (a,b,c) then (a,c,d). A triangle is DEGENERATE iff two of its indices
 *                are equal or (q_b - q_a) x (q_c - q_a) = 0: it is skipped, and its face is counted once among the degenerate faces.
 *   2 signs      orient3(a,b,c,d) = sign(((b - a) x (c - a)) . (d - a)). The drop axis of a triangle is the axis of its normal's largest
 *                magnitude, the lowest axis among equals; orient2 is the sign of the 2x2 determinant in the two kept axes, in their order.
 *   3 segment    closed segment pq against closed non-degenerate triangle abc: sp = orient3(a,b,c,p), sq = orient3(a,b,c,q). sp * sq > 0: no.
 *                Both 0: in the triangle's projection, yes iff p is in the triangle, or q is, or pq meets one of the three edges - a point is
 *                in the triangle iff its three orient2 signs do not hold both a positive and a negative; segment against segment is the
 *                four-sign test, collinear endpoints decided by the closed bounding box. Otherwise: yes iff orient3(p,q,a,b),
 *                orient3(p,q,b,c), orient3(p,q,c,a) do not hold both a positive and a negative.
 *   4 triangles  two non-degenerate triangles of different faces, k = the vertex INDICES they share. k = 0: they intersect iff one of the six
 *                edge-against-triangle tests says yes. k = 1: iff the edge opposite the shared index in one meets the other triangle, either
 *                way round. k = 2, shared edge u < v, apexes a, b: iff orient3(q_u,q_v,q_a,q_b) = 0 and (q_v - q_u) x (q_a - q_u), (q_v - q_u)
 *                x (q_b - q_u) have the same sign in the first one's drop axis - coplanar and folded over. k = 3: they intersect. Vertices
 *                that coincide in position but not in index are k = 0 contact: closed sets, so T-junctions and coincident seams intersect.
 *   5 pairs      faces f < g are an intersecting pair iff some triangle of f and some triangle of g intersect; the two triangles of one quad
 *                are never tested against each other.
 * Outputs, each optional (NULL) except counts:
 *   face_hit (n_faces) uint8: 1 iff the face is in some pair; face_pairs (n_faces) int32: the pairs it is in, saturating at 2^31 - 1;
 *   pairs (cap_pairs,2) int32: the first min(P, cap_pairs) pairs in ascending (f, g) order, nothing beyond them;
 *   counts[8]: non-degenerate triangles, degenerate faces, candidate triangle pairs tested exactly (this one depends on the broad phase and
 *   is no part of the contract), intersecting pairs P, faces hit, pairs with a k = 0 hit, pairs with a k >= 1 hit and no k = 0 hit, pairs
 *   written.
 * A short cap_pairs is no refusal: the list is truncated and counts[3] says what a second call needs. n_faces = 0: counts 0, nothing written.
 * SN_ERR_ARG, nothing written but counts (zeros), in sn_mesh_smooth's words: a face index outside [0, n_verts) or a referenced coordinate
 * outside the range (or not a number), the text naming the first offending face; nv not 3 or 4, n_verts or n_faces > 2^28; and cap_pairs < 0,
 * a null cfg, more than 2^26 triangles, 2^30 or more intersecting triangle pairs. There is no repair, and the work is quadratic in the triangles
 * that crowd one grid cell. Everything is an integer: the result equals the restatement tests/meshintersect_ref.py byte for byte (but
 * counts[2]), on every run. The workspace belongs to the context (grown on demand); both forms return when the work is done. */
typedef struct sn_mesh_intersect_cfg {
    long long cap_pairs;       /* >= 0: rows of `pairs` */
} sn_mesh_intersect_cfg;
SN_API int sn_mesh_intersect(sn_ctx *ctx, const sn_mesh_intersect_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv,
                             const int32_t *faces, unsigned char *face_hit, int32_t *face_pairs, int32_t *pairs, long long *counts);
SN_API int sn_mesh_intersect_dev(sn_ctx *ctx, const sn_mesh_intersect_cfg *cfg, int n_verts, const double *verts_dev, int n_faces, int nv,
                                 const int32_t *faces_dev, unsigned char *face_hit_dev, int32_t *face_pairs_dev, int32_t *pairs_dev,
                                 long long *counts);

/* ---- distance from points to a mesh: the exact nearest triangle ------------------------------------------------------
 * sn_mesh_distance gives, for each of n_pts points, the nearest point of a mesh: verts (n_verts,3) float64 in WORLD coordinates (as
 * sn_mesh_render's), faces (n_faces,nv) int32, nv = 3 or 4 - a quad (a,b,c,d) is the triangles (a,b,c), (a,c,d), triangle t = f for nv = 3
 * and t = 2 f + half for nv = 4 -, pts (n_pts,3) float64, finite. All float arithmetic is fp64 with + - * / and comparisons only, without
 * contraction, in fixed orders: dot(a,b) = (a0*b0 + a1*b1) + a2*b2, cross(a,b) = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0).
 *   1 segment    P against closed segment UV: e = V - U, w = P - U, ee = dot(e,e), we = dot(w,e). ee == 0 or we <= 0: the closest point c is
 *                U; else we >= ee: c is V itself; else t = we / ee, c = U + e*t per component. d2 = dot(P - c, P - c).
 *   2 triangle   P against ABC, corners in face order: e1 = B - A, e2 = C - A, n = cross(e1,e2), nn = dot(n,n). If nn > 0: w = P - A,
 *                nb = dot(cross(w,e2), n), ng = dot(cross(e1,w), n), and if nb > 0, ng > 0 and nb + ng < nn the face candidate is c = A +
 *                (e1*(nb/nn) + e2*(ng/nn)). The answer is the first, in the order face, AB, BC, CA, of the candidates with the least d2. A
 *                DEGENERATE triangle (nn == 0: a repeated index, collinear or coincident corners) is its three segments.
 *   3 mesh       the least d2 over all triangles and, among those that attain it, the smallest triangle index: face is that triangle's
 *                face, closest its c. The answer depends on no traversal order and not on the grid.
 *   4 cap        the answer is reported when the minimum d2 is below max_dist*max_dist * (1 + 2^-40) (sn_nn_dist2's cap); otherwise d2 =
 *                +inf, face = -1, closest = three NaNs. The same for n_faces = 0.
 * Outputs, each optional (NULL) except counts: d2 (n_pts) float64, face (n_pts) int32, closest (n_pts,3) float64; counts[8] = triangles,
 * degenerate triangles, points answered, points beyond the cap, (point, triangle) tests run (this one belongs to the broad phase and is no
 * part of the contract), 0, 0, 0. n_pts = 0 is legal: the mesh is checked and counted.
 * SN_ERR_ARG, nothing written but counts (zeros): a face index outside [0, n_verts) or a non-finite coordinate of a referenced vertex (the
 * text names the first offending face, in sn_mesh_sample's words; unreferenced vertices may hold anything); a non-finite point (the text
 * names the first); nv not 3 or 4, n_verts or n_faces > 2^28, n_pts > 2^29, max_dist not finite or not > 0, a null cfg, more than 2^26
 * triangles (the grid's tables). Limits: the distance is unsigned; no barycentric coordinates come out; a uniform grid, no hierarchy: the
 * work is quadratic in the triangles that crowd one grid cell; coordinates whose squares overflow fp64 give what rule 2's arithmetic
 * gives. The result equals the restatement tests/meshdistance_ref.py bit for bit (but counts[4]), on every run. The workspace belongs to
 * the context (grown on demand); both forms return when the work is done. */
typedef struct sn_mesh_distance_cfg {
    double max_dist;           /* finite, > 0: rule 4's cap */
} sn_mesh_distance_cfg;
SN_API int sn_mesh_distance(sn_ctx *ctx, const sn_mesh_distance_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv,
                            const int32_t *faces, long long n_pts, const double *pts, double *d2, int32_t *face, double *closest,
                            long long *counts);
SN_API int sn_mesh_distance_dev(sn_ctx *ctx, const sn_mesh_distance_cfg *cfg, int n_verts, const double *verts_dev, int n_faces, int nv,
                                const int32_t *faces_dev, long long n_pts, const double *pts_dev, double *d2_dev, int32_t *face_dev,
                                double *closest_dev, long long *counts);

/* ---- inside or outside: the exact winding number of points against a mesh ---------------------------------------------
 * sn_mesh_winding counts, for each of n_pts points, the signed crossings of the point's ray along +axis with a mesh. The mesh is
 * sn_mesh_smooth's: verts (n_verts,3) float64 in lattice cells, faces (n_faces,nv) int32, nv = 3 or 4 - a quad (a,b,c,d) is the triangles
 * (a,b,c), (a,c,d) -, referenced coordinates in -4 <= v < 2^21 - 8; pts (n_pts,3) float64 in lattice cells, every coordinate in the same
 * range. Vertex and query positions become q = int64(rint(v * 65536)). Everything is an integer and exact in 128 bits; only signs are used.
 *   1 axes      the ray runs along +w, w = axis; the kept axes are (u, v) = (w + 1, w + 2) mod 3, a cyclic permutation.
 *   2 triangle  n = (b - a) x (c - a); A2 = n_w, the doubled signed area of the (u, v) projection, s = sign(A2); D = n . (p - a).
 *   3 surface   a triangle with n != 0 HOLDS p iff D = 0 and, in the projection along the triangle's own drop axis (sn_mesh_intersect's rule
 *               2), the three orient2 signs of p against ab, bc, ca do not hold both a positive and a negative (closed). It does not depend
 *               on axis. on_surface[i] = 1 iff some triangle holds p_i.
 *   4 crossing  a triangle with s != 0 is CROSSED by the ray of p iff it is covered, half open - for each edge x -> y of ab, bc, ca, with
 *               e = s ((y_u - x_u)(p_v - x_v) - (y_v - x_v)(p_u - x_u)) and (dx, dy) = s (y_u - x_u, y_v - x_v): e > 0, or e = 0 and dy > 0,
 *               or e = 0, dy = 0 and dx > 0 (sn_mesh_render's rule 4) - and lies strictly above p: D s < 0. A triangle with s = 0 is never
 *               crossed.
 *   5 outputs   winding[i] = the sum of s over the crossed triangles, crossings[i] their number. A face whose normal points along +w adds
 *               +1: a closed mesh turned outward gives +1 inside and 0 outside.
 * Outputs, each optional (NULL) except counts: winding (n_pts) int32, crossings (n_pts) int32, on_surface (n_pts) uint8; counts[8] =
 * triangles with s != 0, triangles with s = 0 but n != 0, triangles with n = 0, points with winding != 0, (point, triangle) entries looked at
 * (this one belongs to the broad phase and is no part of the contract), points on the surface, 0, 0. n_pts = 0 is legal: the mesh is checked and
 * counted. n_faces = 0: all zeros.
 * SN_ERR_ARG, nothing written but counts (zeros), in sn_mesh_smooth's words: a face index outside [0, n_verts) or a referenced coordinate
 * outside the range (or not a number), the text naming the first offending face, an index before a coordinate; then the first point with a
 * coordinate outside the range (or not a number); nv not 3 or 4, n_verts or n_faces > 2^28, n_pts > 2^29, axis outside 0 .. 2, a null cfg,
 * more than 2^26 triangles. Limits: the winding number of an open or inconsistently turned mesh depends on the axis (on_surface does not);
 * there is no fractional winding number; a uniform 2-D grid, no hierarchy: a query looks at every triangle of its column's cell. The result
 * equals the restatement tests/meshwinding_ref.py byte for byte (but counts[4]), on every run. The workspace belongs to the context (grown on
 * demand); both forms return when the work is done. */
typedef struct sn_mesh_winding_cfg {
    int axis;                  /* 0, 1 or 2: the ray runs along +axis */
    int reserved;              /* 0 */
} sn_mesh_winding_cfg;
SN_API int sn_mesh_winding(sn_ctx *ctx, const sn_mesh_winding_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv,
                           const int32_t *faces, long long n_pts, const double *pts, int32_t *winding, int32_t *crossings,
                           unsigned char *on_surface, long long *counts);
SN_API int sn_mesh_winding_dev(sn_ctx *ctx, const sn_mesh_winding_cfg *cfg, int n_verts, const double *verts_dev, int n_faces, int nv,
                               const int32_t *faces_dev, long long n_pts, const double *pts_dev, int32_t *winding_dev, int32_t *crossings_dev,
                               unsigned char *on_surface_dev, long long *counts);

/* ---- a mesh back into cubes of voxels: exact solid and surface occupancy ------------------------------------------------
 * sn_mesh_voxelize gives every voxel of n_cubes cubes of D^3 voxels two bits against a mesh. The mesh is sn_mesh_winding's: verts
 * (n_verts,3) float64 in lattice cells, faces (n_faces,nv) int32, nv = 3 or 4 - a quad (a,b,c,d) is the triangles (a,b,c), (a,c,d) -,
 * referenced coordinates in -4 <= v < 2^21 - 8, q = int64(rint(v * 65536)). cube_ijk (n_cubes,3) int32, stride_vox >= 1, D in 1 .. 64.
 *   1 cells     voxel (n; i,j,k) is the world cell g = cube_ijk[n] * stride_vox + (i,j,k); its centre is the lattice point g, p = g * 65536
 *               in the fixed point; its box is the closed [p - 32768, p + 32768]^3. Cubes may overlap: a shared cell gets the same bits.
 *   2 solid     bit 0: the winding number of p is not zero under sn_mesh_winding's rules 1, 2, 4, 5 along cfg.axis, unchanged - the bit
 *               equals (sn_mesh_winding(centres).winding != 0) byte for byte, on any mesh.
 *   3 surface   bit 1: some triangle with n != 0 has a point in common with the voxel's closed box, decided by the separating-axis test
 *               in exact integers on 13 axes - the 3 box axes, the triangle's normal, the 9 products of a box axis and an edge. They
 *               are separated iff on some axis the triangle's interval lies strictly beyond the box's: touching is a hit. The bit does
 *               not depend on cfg.axis. Degenerate triangles (n = 0) take no part in either bit; they are counted.
 * cfg.modes says which bits are computed (bit 0 solid, bit 1 surface, 1 .. 3; the other bit is 0), cfg.select (1 .. 3) which make Y.
 * Outputs, each optional (NULL) except counts: occ (n_cubes,D,D,D) uint8 in [n,i,j,k] order, the bits; Y (n_cubes,1,D,D,D) float32, 1.0
 * iff occ & select, else 0.0 - the tensor sn_gt_cubes writes; per_cube (n_cubes,2) int64 solid, surface voxels; counts[8] = triangles
 * with s != 0, triangles with s = 0 but n != 0, triangles with n = 0, solid voxels, surface voxels, voxels with both bits, (column,
 * triangle) pairs covered, (voxel, triangle) box tests run - the last two belong to the broad phase and are no part of the contract.
 * n_cubes = 0 is legal: the mesh is checked and counted. n_faces = 0: all zeros.
 * SN_ERR_ARG, nothing written but counts (zeros), in sn_mesh_smooth's words: a face index outside [0, n_verts) or a referenced coordinate
 * outside the range (or not a number), the text naming the first offending face; then the first cube with a negative ijk or whose last
 * cell cube_ijk * stride_vox + D - 1 reaches 2^21 - 8; nv not 3 or 4, n_verts or n_faces > 2^28, more than 2^26 triangles, n_cubes < 0, D
 * outside 1 .. 64, stride_vox < 1, axis outside 0 .. 2, modes or select outside 1 .. 3, n_cubes * D^3 > 2^33, a null cfg. Limits: no
 * world-mm input, no signed-distance field, no hierarchy - a huge triangle over many cubes costs its box of columns in every cube it
 * covers. The result equals the restatement tests/meshvoxel_ref.py byte for byte (but counts[6], counts[7]), on every run. The
 * workspace belongs to the context (grown on demand); both forms return when the work is done. */
typedef struct sn_mesh_voxelize_cfg {
    int axis;                  /* 0, 1 or 2: the rays of the solid bit run along +axis */
    int modes;                 /* bit 0 solid, bit 1 surface: 1 .. 3 */
    int select;                /* 1 .. 3: the bits of occ that make Y */
    int reserved;              /* 0 */
} sn_mesh_voxelize_cfg;
SN_API int sn_mesh_voxelize(sn_ctx *ctx, const sn_mesh_voxelize_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv,
                            const int32_t *faces, int n_cubes, const int32_t *cube_ijk, int D, int stride_vox, unsigned char *occ, float *Y,
                            long long *per_cube, long long *counts);
SN_API int sn_mesh_voxelize_dev(sn_ctx *ctx, const sn_mesh_voxelize_cfg *cfg, int n_verts, const double *verts_dev, int n_faces, int nv,
                                const int32_t *faces_dev, int n_cubes, const int32_t *cube_ijk_dev, int D, int stride_vox,
                                unsigned char *occ_dev, float *Y_dev, long long *per_cube_dev, long long *counts);

/* ---- the mesh back in its views: depth maps, face ids, visibility, colours --------------------------------------------
 * sn_mesh_render rasterises a mesh into V views of one size: verts (n_verts,3) float64 in WORLD coordinates (as sn_mesh_sample's), faces
 * (n_faces,nv) int32, nv = 3 or 4 - a quad (a,b,c,d) is the triangles (a,b,c), (a,c,d) in that order, triangle t = f for nv = 3 and t = 2 f +
 * half for nv = 4 -, P (V,3,4) float64 or NULL for the cameras of sn_set_cameras (V is then theirs). Pixel (i, j) has its centre at h = i,
 * w = j. All float arithmetic is fp64 without contraction; everything that is summed or compared across lanes is an integer.
 *   1 projection  per view and vertex (h, w, z) are what sn_project_points returns as img_h, img_w, depth (round_int = 0).
 *   2 snap        X = int64(rint(w * 256)), Y = int64(rint(h * 256)). A triangle is CLIPPED when one of its corners has a non-finite h, w or z,
 *                 z <= near, or |X| or |Y| >= 2^25: it is dropped whole and counted. Nothing is clipped against the camera plane.
 *   3 edges       corners 0, 1, 2 in face order; E_k belongs to the edge from corner (k+1)%3 to corner (k+2)%3; for a -> b E(p) = (bx-ax) *
 *                 (py-ay) - (by-ay) * (px-ax), exact in int64. A2 = E_0(corner 0); A2 = 0: DEGENERATE, dropped and counted. s = sign(A2);
 *                 every E_k and every edge direction (dx, dy) is multiplied by s (negated, the corners are not swapped).
 *   4 coverage    pixel (i, j), sampled at (256 j, 256 i), is covered iff for every k: s E_k > 0, or s E_k = 0 and edge k owns its line: s dy >
 *                 0, or s dy = 0 and s dx > 0. Of two triangles that share an edge exactly one owns a centre on it.
 *   5 depth       r_k = 1.0 / z_k; S = (double(s E_0) * r_0 + double(s E_1) * r_1) + double(s E_2) * r_2; zpix = double(s A2) / S: finite, > 0.
 *   6 resolve     depth[v,i,j] = the least zpix over the covering triangles, face[v,i,j] = the face (t for nv = 3, t >> 1 for nv = 4) of the
 *                 smallest triangle index among those that attain it; an empty pixel has depth 0.0 and face -1.
 *   7 face_pixels (V,n_faces) int32: the pixels the face wins in view v.
 *   8 vert_visible (V,n_verts) uint8, for every vertex, referenced or not: 1 iff h, w, z are finite, z > near, |h|, |w| < 2^25; the nearest
 *                 pixel (rint(h), rint(w)) lies in the image; and of the four pixels (floor(h) + {0,1}, floor(w) + {0,1}) at least one is empty
 *                 or outside the image, or z - tol <= the largest of their four depths.
 *   9 counts[8]   summed over the views: triangles, clipped, degenerate, rasterised, covering (triangle, pixel) pairs, non-empty pixels, visible
 *                 (view, vertex) pairs, 0.
 * Outputs, each optional (NULL) except counts: depth (V,H,W) float64, face (V,H,W) int32, face_pixels, vert_visible. n_faces = 0: depth 0.0,
 * face -1, vert_visible by rule 8 with every pixel empty. SN_ERR_ARG with nothing written but counts (zeros): a face index outside [0,
 * n_verts) or a non-finite coordinate of a referenced vertex (the text names the first offending face, in sn_mesh_sample's words), nv not 3 or
 * 4, n_verts or n_faces > 2^28, H or W outside 1 .. 16384, V < 1, near or tol negative or not finite, a non-finite entry of P; SN_ERR_STATE:
 * P = NULL before sn_set_cameras. Limits: no clipping at the camera plane (a triangle with a corner at z <= near vanishes whole), one image
 * size per call, vertices next to the silhouette count as visible, no anti-aliasing. The workspace belongs to the context and holds ONE
 * view's z-buffer whatever V is; the host form copies each view out as it is done. The result equals tests/meshrender_ref.py byte for byte.
 *
 * sn_mesh_vertex_colors: the same mesh, cameras and size, vert_visible (V,n_verts) uint8 as INPUT (the render's, or any other), and the
 * images of sn_set_images, which must be exactly V images of H x W (none set: SN_ERR_STATE; another count or size: SN_ERR_ARG). View v
 * contributes to vertex a iff vert_visible[v,a] != 0, (h, w, z) are finite and the nearest pixel (rint(h), rint(w)) lies in the image.
 * vert_views (n_verts) int32 = the number n of contributing views; vert_rgb (n_verts,3) uint8 = (2 sum + n) / (2 n), rounded down, of those
 * pixels' RGB per channel, (0,0,0) for n = 0: nearest pixel, equal weights. counts[2] = vertices with n > 0, contributing (view, vertex)
 * pairs. cfg's near and tol are checked and otherwise unused. */
typedef struct sn_mesh_render_cfg {
    int H, W;                  /* 1 .. 16384: the one image size of all views */
    double near;               /* >= 0, finite: a corner at z <= near clips its triangle; a vertex at z <= near is not visible */
    double tol;                /* >= 0, finite: rule 8's depth tolerance, in the units of z (about half a voxel for concave detail) */
} sn_mesh_render_cfg;
SN_API int sn_mesh_render(sn_ctx *ctx, const sn_mesh_render_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv, const int32_t *faces,
                          int V, const double *P, double *depth, int32_t *face, int32_t *face_pixels, unsigned char *vert_visible,
                          long long *counts);
SN_API int sn_mesh_render_dev(sn_ctx *ctx, const sn_mesh_render_cfg *cfg, int n_verts, const double *verts_dev, int n_faces, int nv,
                              const int32_t *faces_dev, int V, const double *P_dev, double *depth_dev, int32_t *face_dev,
                              int32_t *face_pixels_dev, unsigned char *vert_visible_dev, long long *counts);
SN_API int sn_mesh_vertex_colors(sn_ctx *ctx, const sn_mesh_render_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv,
                                 const int32_t *faces, int V, const double *P, const unsigned char *vert_visible, int32_t *vert_views,
                                 unsigned char *vert_rgb, long long *counts);
SN_API int sn_mesh_vertex_colors_dev(sn_ctx *ctx, const sn_mesh_render_cfg *cfg, int n_verts, const double *verts_dev, int n_faces, int nv,
                                     const int32_t *faces_dev, int V, const double *P_dev, const unsigned char *vert_visible_dev,
                                     int32_t *vert_views_dev, unsigned char *vert_rgb_dev, long long *counts);

/* ---- DTU point-cloud evaluation (experiments/DTU/eval_ply.m -> PointCompareMain of the DTU kit) ----------------------
 * Points are (n,3) float64, row-major, finite. d^2 = (dx*dx + dy*dy) + dz*dz in float64 without contraction: the results are those of the numpy
 * restatement bit for bit. Host arrays in and out; the device workspace belongs to the context (grown on demand). Synchronous. n <= 2^29.
 *
 * sn_point_reduce (reducePts_haa): visit the points in ascending rank (rank: a permutation of 0..n-1); a point still alive removes every other
 * point within d^2 <= dst^2. keep (n) receives 1 for the survivors - the greedy maximal independent set of that order - and rounds (optional) the
 * number of parallel rounds it took; SN_ERR_STATE past 65536 rounds (orders that chain the points, not random ones). */
SN_API int sn_point_reduce(sn_ctx *ctx, long long n, const double *xyz, const long long *rank, double dst, unsigned char *keep, int *rounds);
/* sn_nn_dist2 (MaxDistCP): d2[i] = min_j d^2(from_i, to_j) when that minimum is below max_dist^2 * (1 + 2^-40), else +inf (also for an empty
 * "to" cloud): min(sqrt(d2), max_dist) is the capped distance. */
SN_API int sn_nn_dist2(sn_ctx *ctx, long long n_to, const double *to, long long n_from, const double *from, double max_dist, double *d2);
/* sn_point_flags: in_mask[i] (DataInMask) = 1 iff v = round((xyz_i - bb_min) / res) per axis (half away from zero) lies in [0, dims) and
 * mask[v0][v1][v2] != 0 (mask: dims[0] x dims[1] x dims[2] bytes, C order); above[i] (StlAbovePlane) = 1 iff
 * ((plane[0]*x + plane[1]*y) + plane[2]*z) + plane[3] > 0. Either output may be NULL (its inputs are then not read). */
SN_API int sn_point_flags(sn_ctx *ctx, long long n, const double *xyz, const unsigned char *mask, const int *dims, const double *bb_min, double res,
                          const double *plane, unsigned char *in_mask, unsigned char *above);

/* ---- point-seeded cube list (scene.quantizePts2Cubes, utils/scene.py:63-108; the initialPtsNamePattern branch of main_reconstruct.py:52-60;
 * DESIGN.md section 4.8) -------------------------------------------------------------------------------------------------------------------
 * The cubes around a point cloud: a point is kept when lo <= p <= hi on every axis (has_box; compared in float64), shift = the per-axis minimum of
 * the kept points, q = (p - shift) // stride_q per axis with numpy's floor_divide - the subtraction in the points' type, the division in float32
 * (compute_f64 = 0: float32 points only; stride_q is then rounded to float32) or float64 - and every kept point contributes the two cells q and
 * q + 1 (the floor corner and the diagonal corner: what the reference's vstack + row-wise unique yields). The result is the set of distinct cells in
 * ascending (i, j, k): ijk (n_cells,3) uint32 and xyz (n_cells,3) float32 = float32((double(ijk) * stride_xyz + double(shift)) - half).
 * Variable-length result, as sn_dense2sparse's lists: the caller's arrays hold `cap` cells (2 n always suffices), *n_cells receives the number
 * produced. When more than cap are needed nothing is written, *n_cells holds the number needed and SN_ERR_ARG is returned. SN_ERR_ARG too for a
 * non-finite coordinate and for a cloud spanning 2^21 or more strides on an axis (cell indices are below 2^21). No kept point: *n_cells = 0.
 * n <= 2^27. All three forms return when the work is done. */
typedef struct sn_ptcubes_cfg {
    int pts_f64;             /* points are float64 (else float32) */
    int compute_f64;         /* the type numpy promotes (pts - shift) // stride to; float64 points require 1 */
    double stride_q;         /* the stride the cell index divides by */
    double stride_xyz;       /* the stride as float64, for xyz */
    double half;             /* cube_D_mm / 2 */
    int has_box;
    double lo[3], hi[3];     /* BB_min - cube_D_mm / 2, BB_max + cube_D_mm / 2 */
} sn_ptcubes_cfg;
SN_API int sn_ptcubes(sn_ctx *ctx, long long n, const void *pts, const sn_ptcubes_cfg *cfg, long long cap, uint32_t *ijk, float *xyz,
                      long long *n_cells);
SN_API int sn_ptcubes_dev(sn_ctx *ctx, long long n, const void *pts_dev, const sn_ptcubes_cfg *cfg, long long cap, uint32_t *ijk_dev,
                          float *xyz_dev, long long *n_cells);
/* The same for the masked voxels of a scene's packed sparse lists (offsets (n_cubes+1) int64, vxl_ijk (total,3) uint8, mask (total) uint8, per-cube
 * xyz (n_cubes,3) and resol (n_cubes) float32), the points never leaving HBM: p = float32(vxl_ijk) * resol + xyz of the voxel's cube, in float32,
 * as sparseCubes.sparse_xyz forms them (cfg->pts_f64 = 0). */
SN_API int sn_ptcubes_sparse_dev(sn_ctx *ctx, int n_cubes, long long total, const int64_t *offsets_dev, const unsigned char *vxl_ijk_dev,
                                 const unsigned char *mask_dev, const float *cube_xyz_dev, const float *cube_resol_dev, const sn_ptcubes_cfg *cfg,
                                 long long cap, uint32_t *ijk_dev, float *xyz_dev, long long *n_cells);

/* ---- ground-truth mode (__SurfaceNet_fn_inference__(with_groundTruth=True), nets/SurfaceNet.py:359-378; the val_fn of SurfaceNet_fn_trainVal,
 * nets/SurfaceNet.py:253-264; __weighted_accuracy__, nets/SurfaceNet.py:203-224) -----------------------------------------
 * The target tensor Y of those functions from a ground-truth point cloud, and the counts their accuracy is formed from.
 * sn_gt_bind: binds n float32 points (n,3) to the context, sorted into a uniform grid of edge `cell` > 0 (a quarter of a cube's side is a good
 *   choice; it decides speed only). Rebinding replaces the cloud; n = 0 is legal (every Y is then zero). SN_ERR_ARG for a non-finite coordinate and
 *   for a cloud spanning 2^21 or more cells on an axis; a failed bind leaves no cloud bound. n <= 2^27. Needs no weights, images or cameras.
 *   Both forms return when the cloud is sorted (the caller's array is not read afterwards).
 * sn_gt_cubes: Y (n,1,s,s,s) float32 for n cubes (xyz (n,3), resol (n) float32; s = cube_D): with q = floor((p - xyz_c) / resol_c) per axis in
 *   float32 - one subtraction, one correctly rounded division - Y[c,0,q0,q1,q2] = 1 iff some bound point has 0 <= q < s on all three axes (q = -0
 *   counts as 0), every other voxel 0. Independent of the order of the points and of `cell`. SN_ERR_STATE when no cloud is bound; SN_ERR_ARG for a
 *   non-finite xyz and for a resol that is not finite and > 0: the host form checks before it starts, the device form - asynchronous on the
 *   context's stream - leaves such a cube's Y zero and reports at the next sn_synchronize.
 * sn_weighted_accuracy: counts (n,4) int64 = per cube n_pos, n_neg, hit_pos, hit_neg of pred and Y (both (n,1,s,s,s) float32): positive is Y > 0,
 *   negative Y == 0 (a negative or NaN target is neither), a hit is float(pred >= threshold) == Y (lasagne's binary_accuracy: ge; a NaN prediction
 *   compares false). Integer arithmetic: exact. n <= 65535. The reference's accuracy of the whole batch tensor follows from the column sums
 *   S in float64: acc_neg = S[3] / S[1], acc_pos = S[2] / S[0] (acc_neg when S[0] = 0, the reference's ifelse), (acc_pos + acc_neg) / 2. The device
 *   form is asynchronous on the context's stream. */
SN_API int sn_gt_bind(sn_ctx *ctx, long long n, const float *pts, double cell);
SN_API int sn_gt_bind_dev(sn_ctx *ctx, long long n, const float *pts_dev, double cell);
SN_API int sn_gt_cubes(sn_ctx *ctx, int n, const float *xyz, const float *resol, float *Y);
SN_API int sn_gt_cubes_dev(sn_ctx *ctx, int n, const float *xyz_dev, const float *resol_dev, float *Y_dev);
SN_API int sn_weighted_accuracy(sn_ctx *ctx, int n, const float *pred, const float *Y, float threshold, int64_t *counts);
SN_API int sn_weighted_accuracy_dev(sn_ctx *ctx, int n, const float *pred_dev, const float *Y_dev, float threshold, int64_t *counts_dev);

/* ---- training the view-pair weighting net with SurfaceNet frozen ("train the softmaxWeight with(out) finetuning the SurfaceNet",
 * nets/SurfaceNet.py:266-294; the 258 -> 100 -> 1 MLP of __relativeWeight_net__, nets/SurfaceNet.py:84-100) ------------
 * Trainable: feature_fc1.W / beta / gamma and feature_linear1.W / b; feature_fc1.mean / inv_std follow as running statistics. The 3-D network
 * is not touched: a step takes its unfused predictions U (n, n_vp, s,s,s), the features F (n * n_vp, 258) and the target Y (n,1,s,s,s), all float32.
 * Forward in training mode (batch statistics, biased variance, bn_eps), w = softmax over each cube's n_vp rows, f = sum_p w_p U_p,
 * loss = mean of -(w_for_1 Y log f' + (1 - w_for_1)(1 - Y) log(1 - f')) with f' = clamp(f, clip, 1 - clip), + l2 (sum W1^2 + sum w2^2); backward in
 * closed form; then the update. fp32 throughout, every sum in a fixed order: the same inputs give the same bits on every run.
 * sn_relw_train_begin: starts a session from the loaded weights (master copies, zero velocities). update: 0 = gradients only (nothing changes),
 *   1 = sgd (p -= lr g), 2 = Nesterov momentum as lasagne.updates.nesterov_momentum (t = lr g; v = momentum v - t; p = (p - t) + momentum v); with
 *   1 and 2 the running statistics move by bn_alpha (mean = (1 - bn_alpha) mean + bn_alpha mu, inv_std alike). SN_ERR_STATE when only the 98
 *   network arrays were loaded. Beginning again restarts from the weights as trained so far; sn_load_weights ends the session.
 * sn_relw_train_step(_dev): one step on n cubes (1 <= n <= 65535) of 2 <= n_vp <= 16 pairs each. Optional results (null: not wanted): fused f
 *   (n,1,s,s,s), weights w (n, n_vp), counts (n,4) int64 of f against Y as sn_weighted_accuracy (threshold 0.5), *loss (host). The device form is
 *   asynchronous on the context's stream unless loss is given. After a step with update != 0, sn_relative_weights and sn_viewpair_weights use
 *   the trained weights (running statistics). SN_ERR_STATE before sn_relw_train_begin, SN_ERR_ARG for a null argument or n / n_vp out of range.
 * sn_relw_train_grads: the last step's gradients W1 (258,100) | beta | gamma | w2 (100 each) | b2 (1), then its batch statistics mu | istd
 *   (100 each): 26301 floats. sn_relw_train_velocities: the velocities, laid out as the gradients (26101 floats). sn_relw_train_dw: the last
 *   step's d loss / d w (n * n_vp floats). SN_ERR_STATE when no step has run.
 * sn_relw_get_params: the seven arrays in weight-file order W1 | beta | gamma | mean | inv_std | w2 | b2 (26301 floats), from the session
 *   when one is open, else as loaded or as the last session left them.
 * sn_relw_train_end: closes the session; the trained weights stay in force for the inference entries. */
typedef struct sn_relw_train_cfg {
    float lr, momentum, w_for_1, l2, bn_alpha, bn_eps, clip;     /* the reference: 0.9, 0.96, 0, 0.1 (Lasagne alpha), 1e-4, 1e-7 */
    int update;
} sn_relw_train_cfg;
SN_API int sn_relw_train_begin(sn_ctx *ctx, const sn_relw_train_cfg *cfg);
SN_API int sn_relw_train_end(sn_ctx *ctx);
SN_API int sn_relw_train_step(sn_ctx *ctx, int n, int n_vp, const float *unfused, const float *features, const float *Y, float *fused,
                              float *weights, int64_t *counts, double *loss);
SN_API int sn_relw_train_step_dev(sn_ctx *ctx, int n, int n_vp, const float *unfused_dev, const float *features_dev, const float *Y_dev,
                                  float *fused_dev, float *weights_dev, int64_t *counts_dev, double *loss);
SN_API int sn_relw_train_grads(sn_ctx *ctx, float *out);
SN_API int sn_relw_train_velocities(sn_ctx *ctx, float *out);
SN_API int sn_relw_train_dw(sn_ctx *ctx, float *out);
SN_API int sn_relw_get_params(sn_ctx *ctx, float *out);

/* ---- similarityNet / early rejection (main_reconstruct.py:76-97) ---------------- */
/* pickle.load + set_all_param_values([embedding layer, similarity layer]) of similarityNet_inference
 * (nets/similarityNet.py:229-244): 30 arrays in order — 13 x (conv W (Cout,Cin,3,3), b (Cout,)) for conv1_1 .. conv5_3
 * (cross-correlation, as Conv2DDNNLayer), embedding W (5888,128), b (128,), similarity W (1,1), b (1,). */
SN_API int sn_simil_load_weights(sn_ctx *ctx, const float *blob, size_t n_floats, const sn_param_desc *descs, int n_params);
/* image.cropImgPatches(img = view's image, pyramidRate = 1, cubeCenter_hw = (center_h, center_w)) (utils/image.py:92-183, as
 * called at utils/earlyRejection.py:50): n patches (n,64,64,3) uint8 RGB around the truncated centre projections,
 * coordinates clamped to the image. center_h / center_w: float64 (n,). Needs sn_set_images. */
SN_API int sn_crop_patches(sn_ctx *ctx, int view, int n, const double *center_h, const double *center_w, unsigned char *patches);
/* patch2embedding_fn (nets/similarityNet.py:219-221): preprocessed patches (n,3,64,64) float32 (BGR - mean) -> (n,128). */
SN_API int sn_patch2embedding(sn_ctx *ctx, int n, const float *patches, float *embeddings);
/* The inner loop of earlyRejection.patch2embedding (utils/earlyRejection.py:50-53) without leaving HBM: crop +
 * image.preprocess_patches (utils/image.py:9-36, mean_bgr[3]) + patch2embedding_fn for n cube centres of one view. */
SN_API int sn_crop_embed(sn_ctx *ctx, int view, int n, const double *center_h, const double *center_w, const float *mean_bgr,
                  float *embeddings);
/* embeddingPair2simil_fn (nets/similarityNet.py:223-226): rows 2i, 2i+1 of emb_pairs (2*n_pairs,128) -> (n_pairs,1)
 * sigmoid(w * ||e1 - e2||_2 + b). */
SN_API int sn_embeddingpair2simil(sn_ctx *ctx, int n_pairs, const float *emb_pairs, float *similarity);
/* earlyRejection.embeddingPairs2simil (utils/earlyRejection.py:59-90) in one call: embeddings (n_cubes, n_views, 128) ->
 * similarity (n_cubes, n_views*(n_views-1)/2), pairs in itertools.combinations order; bit-identical to feeding the same pairs
 * through sn_embeddingpair2simil, without shipping every embedding once per pair across PCIe. */
SN_API int sn_embeddings2simil(sn_ctx *ctx, int n_cubes, int n_views, const float *embeddings, float *similarity);

/* camera.perspectiveProj (utils/camera.py:123-184; calls at main_reconstruct.py:62-65 through perspectiveProj_cubesCorner):
 * V cameras x n points in one launch. P (V,3,4) float64 row-major, or NULL = the cameras of sn_set_cameras (V ignored);
 * xyz (n,3) float64 -> img_h, img_w (V,n) float64 (row v = camera v), depth (V,n) or NULL. Same arithmetic as the CVC
 * warp's projection (fp64 FMA chain over k, IEEE divide); round_int != 0 applies numpy's .round() (half-to-even) - the
 * caller casts to int64. */
SN_API int sn_project_points(sn_ctx *ctx, int V, const double *P, int n, const double *xyz, int round_int, double *img_h,
                      double *img_w, double *depth);

/* ---- numerics of the default mode's 6-bit code planes ------------------------------------------------------------
 * The two merge layers read their inputs as fp16 + 6-bit e2m3 codes scaled by a per-tensor premultiplier 2^s ("cat": the concat buffer of
 * sigmoid side outputs; "act": merge_conv_a's ReLU output). (The dilated layers conv4_1 .. conv4_3 run the same two-term correction on fp8 e4m3
 * codes since round 5: those have the exponent range, there is nothing to calibrate.) s is static - sized from the layers' BatchNorm parameters, which trained nets obey
 * (nets/SurfaceNet.py:33-74, every batch_norm) - unless the caller calibrates it on data:
 *   sn_calibrate_dev looks at the activations the LAST forward call left in the workspace (n_samples of them, <= 0: all that call ran; run
 *   sn_forward / sn_cvc_forward on a representative batch first - SN_ERR_STATE when none has run since the weights / the mode were set, or when it
 *   ran fewer samples; default precision mode only), and sets each tensor's s to the largest value whose saturated fraction (|v| * 2^s > 7.5) stays <= max_sat_fraction.
 *   The new exponents apply to every later call of this context; sn_load_weights / sn_set_precision restore the static ones. A negative
 *   max_sat_fraction only MEASURES: the report holds the saturated fractions under the exponents in force (s_* = s_*_before), nothing changes.
 * A value beyond the code range loses (only) its own correction term; it is not an error. sn_numeric_status reports - and clears - the WARNING bits:
 * which layers stored such values since the last call (names: comma-separated layer names, bit i = the i-th). */
typedef struct sn_calibration {
    int s_act_before, s_cat_before, s_act, s_cat;                /* premultiplier exponents before / after */
    double sat_act_before, sat_cat_before, sat_act, sat_cat;     /* saturated fraction of the non-zero values under them */
    float max_act, max_cat;                                      /* largest stored magnitude */
} sn_calibration;
SN_API int sn_calibrate_dev(sn_ctx *ctx, int n_samples, double max_sat_fraction, sn_calibration *out);
SN_API int sn_numeric_status(sn_ctx *ctx, unsigned *saturated_bits, char *names, int names_cap);

/* ---- multi-GPU (one process per GPU): the path's only exchange is an all-gather of the per-cube fused probabilities
 * (the reference is single-GPU, no counterpart). RCCL over xGMI; librccl is dlopen'ed on first use.
 * Rank 0 calls sn_comm_unique_id and ships the 128 bytes to the other ranks by any means; every rank then calls
 * sn_comm_init (collective). sn_allgather_f32_dev is asynchronous on the context's stream. */
SN_API int sn_comm_unique_id(char *id128);
SN_API int sn_comm_init(sn_ctx *ctx, int world, int rank, const char *id128);
/* The same with a bound on the wait (ncclCommInitRank blocks until EVERY rank has called it): after timeout_s seconds the call returns
 * SN_ERR_COMM, the context stays without a communicator and remains usable for everything but the exchange (the helper thread that is still
 * inside RCCL is abandoned). timeout_s <= 0: no deadline (= sn_comm_init; the caller vouches that all ranks arrive). */
SN_API int sn_comm_init_deadline(sn_ctx *ctx, int world, int rank, const char *id128, double timeout_s);
/* Which RCCL the entry points are bound to: file name + whether the host process had it mapped already (then that copy is used: a process
 * must not run two RCCL copies) and the ncclGetVersion code. Loads librccl if nothing has yet. */
SN_API int sn_comm_info(char *file, int file_cap, int *version_code);
SN_API int sn_allgather_f32_dev(sn_ctx *ctx, const float *local_dev, size_t n_local, float *global_dev);
/* The same on the context's own communication stream, ordered behind everything submitted to the kernel stream so far: the all-gather of
 * batch i overlaps the kernels of batch i + 1. slot (0..7) names its completion; sn_comm_wait(ctx, slot) makes the kernel stream wait for it
 * (call it before local_dev / global_dev are written again). sn_synchronize waits for both streams. */
SN_API int sn_allgather_f32_dev_overlap(sn_ctx *ctx, const float *local_dev, size_t n_local, float *global_dev, int slot);
SN_API int sn_comm_wait(sn_ctx *ctx, int slot);
/* Variable-length all-gather of bytes - the exchange of the packed sparse voxel lists of a sharded scene (SURVEY §8e "counts then
 * all-gather-v"; utils/sparseCubes.py:9-77 produces the lists, main_reconstruct.py:153-160 accumulates them): every rank contributes
 * n_local bytes of device memory (0 allowed, different per rank); global_dev receives the contributions back to back in rank order and
 * counts[r] (host, `world` entries) their sizes. Synchronous. Every rank issues the same collectives whatever its own arguments are (counts; one
 * 8-byte status word per rank - a rank that cannot allocate its staging buffer says so there and EVERY rank returns the error without entering
 * the payload step; payloads): a destination that cannot hold the total is reported AFTER the payload all-gather (SN_ERR_ARG, counts[] filled in)
 * and must NOT be answered by a retry of this rank alone. Size the destination first with sn_allgatherv_counts (collective: the 8-byte counts all-gather alone). */
SN_API int sn_allgatherv_counts(sn_ctx *ctx, size_t n_local, unsigned long long *counts);
SN_API int sn_allgatherv_bytes_dev(sn_ctx *ctx, const void *local_dev, size_t n_local, void *global_dev, size_t global_cap,
                                   unsigned long long *counts);

/* ---- measurement ------------------------------------------------------------------------------ */
/* Per-kernel HIP-event timing on the context's stream. While enabled every kernel launch is
 * bracketed by events; sn_profile_get drains them. idx enumerates kernel tags (layer names);
 * returns 1 past the last. flops / bytes are the ALGORITHMIC work of the recorded launches. */
SN_API int sn_profile_enable(sn_ctx *ctx, int on);
SN_API int sn_profile_count(sn_ctx *ctx);
SN_API int sn_profile_get(sn_ctx *ctx, int idx, char *name, int name_cap, double *ms_total, int64_t *launches,
                   double *flops, double *bytes);
SN_API int sn_profile_reset(sn_ctx *ctx);
/* What THIS box sustains on a pure stream of v_mfma_f32_16x16x32_f16 (all CUs, one wave per SIMD, random fp16 operands in registers): boxes of
 * the same SKU fall into speed classes 5-8 % apart (power / clock management), and every absolute number of a run - cubes/s, kernel times,
 * `roofline.frac` against the nominal 2.5 PF - moves with it. Runs a few launches of ~target_ms (<= 0: 10 ms) on the context's stream (DVFS settles
 * within the first), returns the last one's rate in dense fp16 TFLOP/s and the shader clock it ran at (cycle counter / event time). Synchronous.
 * No reference counterpart: measurement infrastructure (bench.py -> "box"). */
SN_API int sn_mfma_probe(sn_ctx *ctx, double target_ms, double *tflops, double *ghz);

#ifdef __cplusplus
}
#endif
#endif /* SURFACENET_HIP_H */
