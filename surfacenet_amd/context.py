"""`Context`: one GPU's SurfaceNet inference state (images, cameras, weights, workspace) over the C ABI."""
import contextlib
import ctypes

import numpy as np

from . import _lib, weights as _weights

MEAN_CVC_RGBRGB = np.asarray([123.68, 116.779, 103.939, 123.68, 116.779, 103.939]).astype(np.float32)  # params.py:129


def allgatherv_two_step(n_local, counts_fn, payload_fn):
    """The rank-uniform protocol of `Context.allgatherv_bytes`, separated from the C calls so that the multi-rank CPU tests can drive it over gloo:
    `counts_fn(n_local)` -> the per-rank byte counts (one collective), `payload_fn(n_local, total)` -> (counts, the `total` gathered bytes) (the
    collectives of sn_allgatherv_bytes_dev). Every rank calls the two in this order exactly once: the total is the same number everywhere, so the
    sizing of the destination can never send one rank back into a collective its peers have left."""
    counts = counts_fn(n_local)
    total = int(sum(counts))
    counts2, out = payload_fn(n_local, total)
    if list(counts2) != list(counts):
        raise _lib.SurfaceNetHipError("allgatherv: the ranks' counts changed between the two steps (%r -> %r): mismatched collectives" % (counts, counts2))
    ends = np.cumsum(counts)
    return [out[e - c: e] for c, e in zip(counts, ends)]


class NumericsGuard(object):
    """The numerics safety net of the default mode for ONE caller (a drop-in callable, a cube loop, a scene): the two merge layers read their inputs
    as fp16 + 6-bit codes under per-tensor premultipliers that are static - sized from the BatchNorm parameters a trained net obeys. A net that does
    not obey them saturates codes (each such value loses its own correction term); the library raises a WARNING word for that (`numeric_status`) and
    can derive the premultipliers from data instead (`calibrate`). `check()` - called by the caller right after its first batch, then once per
    scene / per call - reads the word; when more than `trigger_fraction` of a code plane's values saturate it calibrates on the batch that was just run, emits ONE `RuntimeWarning`
    naming the layers and the exponents chosen, and returns the calibration report: the caller then REDOES that batch (nets/SurfaceNet.py:385-402
    is where the only weights that will ever matter are loaded; main_reconstruct.py:145-146 is the call this protects). Afterwards the word is still
    read (and cleared) but a calibrated context reports nothing more: the calibration itself tolerates `max_sat_fraction` of saturated values.

    What the guard KNOWS lives on the Context, next to the exponents it describes (`Context._numerics`): contexts are cached and shared
    (runtime._contexts), `load_param_values` resets the exponents to the static ones - and with them this state, so a reused loop / callable watches
    new weights afresh; two callers of one context see one calibration (a caller with auto_calibrate=False does not calibrate, but runs under whatever
    exponents another caller of the same context set - `ctx.calibration_report()` says which). Cost: while the net stays clean the word is zero and a
    check is one 8-byte read-back; a net that saturates a few per mille of its codes (every uncalibrated random net does) raises the word on every
    batch, so after `BACKOFF_AFTER` measure-only probes below the trigger in a row the guard re-probes only every `BACKOFF_EVERY`-th check."""
    FP8_PLANES = frozenset(("conv3_3", "conv4_1", "conv4_2"))      # tensors of the conv4 chain: fp8 e4m3 code planes (hi codes to 448 * 2^-s, lo codes safe to 256 * 2^-s: where the warning starts; nothing to calibrate)
    BACKOFF_AFTER, BACKOFF_EVERY = 3, 64

    def __init__(self, ctx, enabled=True, max_sat_fraction=1e-3, trigger_fraction=1e-2):
        self.ctx, self.enabled, self.max_sat_fraction, self.trigger_fraction = ctx, bool(enabled), float(max_sat_fraction), float(trigger_fraction)
        self.checks = 0

    # (state shared by every guard of the context; reset by Context.load_param_values)
    @property
    def _st(self):
        st = getattr(self.ctx, "_numerics", None)
        if st is None:
            st = self.ctx._numerics = Context._fresh_numerics()
        return st

    @property
    def calibrated(self):
        return self._st["calibrated"]

    @property
    def report(self):
        return self._st["report"]

    def check(self, where="forward"):
        if not self.enabled:
            return None
        self.checks += 1
        st = self._st
        names = self.ctx.numeric_status()
        if not names or st["calibrated"]:
            return None
        import warnings
        fp8 = [n for n in names if n in self.FP8_PLANES]
        if fp8 and not st["fp8_warned"]:
            st["fp8_warned"] = True
            warnings.warn("surfacenet_amd (%s): stored activations of %s exceed 256 * 2^-s: the fp8 correction codes of the dilated chain conv4_1 .. conv4_3 "
                          "saturate for those values (each loses its own correction term; nothing to calibrate - fp8 has the range, the values are outliers of "
                          "the net's BatchNorm statistics). Context(conv4_fp8=False) keeps the chain on three fp16 MFMAs." % (where, ", ".join(fp8)),
                          RuntimeWarning, stacklevel=3)
        names = [n for n in names if n not in self.FP8_PLANES]
        if not names:
            return None
        if self.ctx.precision != "f16x3":
            if not st["mode_warned"]:
                st["mode_warned"] = True
                warnings.warn("surfacenet_amd (%s): stored activations of %s exceed the range of their 6-bit code planes; precision mode %r has no "
                              "data-driven premultipliers - accuracy degrades towards plain fp16 for those values" % (where, ", ".join(names), self.ctx.precision),
                              RuntimeWarning, stacklevel=3)
            return None
        # The warning word fires at the FIRST saturated value. Nets that roughly obey their BatchNorm statistics saturate a few per mille of
        # merge_conv_a's outputs (measured: 0.1 .. 0.3 % on uncalibrated random nets, 0.22 % on the worst structured input - L_inf unchanged at 5e-5);
        # the guard acts when more than `trigger_fraction` (1 %) of a plane's non-zero values saturate (x3.2 stress net: 5 %, L_inf 2e-4).
        if st["clean_probes"] >= self.BACKOFF_AFTER:
            st["skipped"] += 1
            if st["skipped"] % self.BACKOFF_EVERY:
                return None
        probe = self.ctx.calibrate(0, -1.0)
        st["probes"] += 1
        if max(probe["sat_act_before"], probe["sat_cat_before"]) < self.trigger_fraction:
            st["clean_probes"] += 1              # nothing to redo, nothing to report - the watch goes on (more and more sparsely)
            return None
        st["clean_probes"] = 0
        cal = self.ctx.calibrate(0, self.max_sat_fraction)
        st["calibrated"], st["report"] = True, cal        # one calibration, one warning per set of weights
        warnings.warn("surfacenet_amd (%s): stored activations of %s exceeded the range of their 6-bit code planes (%.2f %% of merge_conv_a's non-zero "
                      "outputs, %.2f %% of the concat buffer; the network's BatchNorm statistics under-estimate their spread). Premultipliers "
                      "recalibrated on this batch: s_act %d -> %d, s_cat %d -> %d (saturated fraction now %.3f %% / %.3f %%); the batch is recomputed. "
                      "Pass auto_calibrate=False to keep the static exponents."
                      % (where, ", ".join(names), 100 * cal["sat_act_before"], 100 * cal["sat_cat_before"], cal["s_act_before"], cal["s_act"],
                         cal["s_cat_before"], cal["s_cat"], 100 * cal["sat_act"], 100 * cal["sat_cat"]), RuntimeWarning, stacklevel=3)
        return cal


RELW_MAX_VP = 16            # relwtrain.h RT_MAX_VP


def check_train_args(s, first, features, Y, n_vp, first_is_X):
    """The dtype / ndim / shape rules of Context.forward_gt for the arguments of a training step on cubes of s^3 - (unfused | X, similFeature, Y) -
    as TypeErrors, with no device call. -> n, the number of cubes."""
    s, n_vp = int(s), int(n_vp)
    if not 2 <= n_vp <= RELW_MAX_VP:
        raise TypeError("training needs 2 <= n_vp <= %d view pairs per cube, got %d" % (RELW_MAX_VP, n_vp))
    what = "X" if first_is_X else "unfused"
    if not isinstance(first, np.ndarray) or first.dtype != np.float32 or first.ndim != 5:
        raise TypeError("%s must be a float32 5-D ndarray" % what)
    if first_is_X:
        if first.shape[1:] != (6, s, s, s) or first.shape[0] % n_vp or first.shape[0] == 0:
            raise TypeError("X must have shape (n*%d, 6, %d, %d, %d), got %s" % (n_vp, s, s, s, first.shape))
        n = first.shape[0] // n_vp
    else:
        if first.shape[1:] != (n_vp, s, s, s) or first.shape[0] == 0:
            raise TypeError("unfused must have shape (n, %d, %d, %d, %d), got %s" % (n_vp, s, s, s, first.shape))
        n = first.shape[0]
    if not isinstance(features, np.ndarray) or features.dtype != np.float32 or features.ndim != 2:
        raise TypeError("similFeature must be a float32 matrix")
    if features.shape != (n * n_vp, _weights.D_VIEWPAIR_FEATURE):
        raise TypeError("similFeature must have shape (%d, %d), got %s" % (n * n_vp, _weights.D_VIEWPAIR_FEATURE, features.shape))
    if not isinstance(Y, np.ndarray) or Y.dtype != np.float32 or Y.ndim != 5:
        raise TypeError("Y must be a float32 5-D ndarray")
    if Y.shape != (n, 1, s, s, s):
        raise TypeError("Y must have shape (%d, 1, %d, %d, %d), got %s" % (n, s, s, s, Y.shape))
    return n


class Context(object):
    PRECISIONS = {"f16": 0, "f16x3": 1, "f16m8": 2, "f16x3p": 3}      # f16x3p: f16x3 without the MX tail (see surfacenet_hip.h)

    def __init__(self, cube_D=32, max_samples=64, device=0, precision="f16x3", conv4_fp8=True):
        """precision: "f16x3" (default; fp32-class results, operands as hi+lo fp16 pairs, 3 MFMAs per term) or
        "f16" (3x faster, L_inf ~2e-3 vs the fp64 oracle on BN-normalised nets: above the 1e-3 parity bar).
        conv4_fp8 (default mode only; sn_set_conv4_fp8): True / 1 = conv4_1 .. conv4_3 with their correction terms on the fp8 MX MFMA (default),
        2 = conv4_2 and conv4_3 only, False / 0 = the whole chain back on three fp16 MFMAs."""
        if precision not in self.PRECISIONS:
            raise ValueError("precision must be one of %s" % sorted(self.PRECISIONS))
        self._lib = _lib.load()
        self.cube_D, self.max_samples, self.device = int(cube_D), int(max_samples), int(device)
        self._h = self._lib.sn_create(self.device, self.cube_D, self.max_samples)
        if not self._h:
            raise _lib.SurfaceNetHipError("sn_create failed: %s" % _lib.last_error())
        self.precision = precision
        _lib.check(self._lib.sn_set_precision(self._h, self.PRECISIONS[precision]))
        if int(conv4_fp8) != 1 and precision == "f16x3":
            _lib.check(self._lib.sn_set_conv4_fp8(self._h, int(conv4_fp8)))
        self.n_views = 0
        self.n_cameras = 0
        self._numerics = self._fresh_numerics()

    @staticmethod
    def _fresh_numerics():
        """What the NumericsGuards of this context know about the exponents in force (they are the static ones after every load_param_values)."""
        return {"calibrated": False, "report": None, "clean_probes": 0, "skipped": 0, "probes": 0, "fp8_warned": False, "mode_warned": False}

    def calibration_report(self):
        """The report of the calibration the context runs under (None: the static premultipliers)."""
        return self._numerics["report"]

    # ---- lifetime ---------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.sn_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def stream_handle(self):
        """hipStream_t of this context as an integer (e.g. for torch.cuda.ExternalStream)."""
        return int(self._lib.sn_stream(self._h) or 0)

    def synchronize(self):
        _lib.check(self._lib.sn_synchronize(self._h))

    # ---- setup ------------------------------------------------------------------------------------
    def load_param_values(self, values):
        """values: the reference weight file's list of arrays (98 or 105, weights.PARAM_LAYOUT order)."""
        blob, descs = _weights.to_blob(values)
        _lib.check(self._lib.sn_load_weights(self._h, _lib.ptr(blob), blob.size, descs, len(values)))
        self._numerics = self._fresh_numerics()          # sn_load_weights restored the static premultipliers: every guard of this context starts over

    def set_images(self, models_img):
        imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in models_img]
        for im in imgs:
            if im.ndim != 3 or im.shape[2] != 3:
                raise ValueError("images must be (H, W, 3) uint8 RGB, got %s" % (im.shape,))
        V = len(imgs)
        ptrs = (ctypes.c_void_p * V)(*[im.ctypes.data for im in imgs])
        H = (ctypes.c_int * V)(*[im.shape[0] for im in imgs])
        W = (ctypes.c_int * V)(*[im.shape[1] for im in imgs])
        _lib.check(self._lib.sn_set_images(self._h, V, ptrs, H, W))
        self.n_views = V

    def set_cameras(self, cameraPOs):
        P = np.ascontiguousarray(cameraPOs, dtype=np.float64)
        if P.ndim != 3 or P.shape[1:] != (3, 4):
            raise ValueError("cameraPOs must have shape (V, 3, 4), got %s" % (P.shape,))
        _lib.check(self._lib.sn_set_cameras(self._h, P.shape[0], _lib.ptr(P)))
        self.n_cameras = P.shape[0]

    # ---- hot path, host arrays --------------------------------------------------------------------
    def _batch_args(self, selected_viewPairs, xyz, resol):
        pairs = np.ascontiguousarray(selected_viewPairs, dtype=np.int64)
        if pairs.ndim != 3 or pairs.shape[2] != 2:
            raise ValueError("selected_viewPairs must have shape (N_cubes, N_viewPairs, 2), got %s" % (pairs.shape,))
        n, n_vp = pairs.shape[:2]
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(n, 3)
        resol = np.ascontiguousarray(resol, dtype=np.float32).reshape(n)
        return pairs, xyz, resol, n, n_vp

    def cvc(self, selected_viewPairs, xyz, resol, mean=None):
        pairs, xyz, resol, n, n_vp = self._batch_args(selected_viewPairs, xyz, resol)
        s = self.cube_D
        out = np.empty((n * n_vp, 6, s, s, s), dtype=np.float32)
        m = None if mean is None else np.ascontiguousarray(mean, dtype=np.float32).reshape(6)
        _lib.check(self._lib.sn_cvc(self._h, n, n_vp, _lib.ptr(pairs), _lib.ptr(xyz), _lib.ptr(resol), _lib.ptr(m), _lib.ptr(out)))
        return out

    def forward(self, X, w=None, n_vp=1, return_unfused=True):
        s = self.cube_D
        if not isinstance(X, np.ndarray) or X.dtype != np.float32:
            raise TypeError("X must be a float32 ndarray (the reference's Theano function rejects other dtypes)")
        if X.ndim != 5 or X.shape[1:] != (6, s, s, s):
            raise TypeError("X must have shape (N*n_vp, 6, %d, %d, %d), got %s" % (s, s, s, X.shape))
        if X.shape[0] % n_vp:
            raise ValueError("X.shape[0]=%d is not a multiple of n_vp=%d" % (X.shape[0], n_vp))
        n = X.shape[0] // n_vp
        X = np.ascontiguousarray(X)
        if n_vp > 1:
            if not isinstance(w, np.ndarray) or w.dtype != np.float32 or w.shape != (n, n_vp):
                raise TypeError("w must be a float32 ndarray of shape (%d, %d)" % (n, n_vp))
            w = np.ascontiguousarray(w)
        else:
            w = None
        fused = np.empty((n, 1, s, s, s), dtype=np.float32)
        unfused = np.empty((n, n_vp, s, s, s), dtype=np.float32) if return_unfused else None
        _lib.check(self._lib.sn_forward(self._h, n, n_vp, _lib.ptr(X), _lib.ptr(w), _lib.ptr(fused), _lib.ptr(unfused)))
        return fused, unfused

    def cvc_forward(self, selected_viewPairs, xyz, resol, w=None, mean=MEAN_CVC_RGBRGB, return_unfused=True, return_cvc=False):
        pairs, xyz, resol, n, n_vp = self._batch_args(selected_viewPairs, xyz, resol)
        s = self.cube_D
        if n_vp > 1:
            if w is None:
                raise TypeError("cvc_forward: w (n, n_vp) float32 is required when a cube has more than one view pair (the reference passes 1/N_vp per pair "
                                "when weighted fusion is off, main_reconstruct.py:114-115)")
            w = np.ascontiguousarray(w, dtype=np.float32)
            if w.size != n * n_vp:
                raise TypeError("cvc_forward: w must have shape (%d, %d), got %s" % (n, n_vp, w.shape))
            w = w.reshape(n, n_vp)
        else:
            w = None
        m = np.ascontiguousarray(mean, dtype=np.float32).reshape(6)
        fused = np.empty((n, 1, s, s, s), dtype=np.float32)
        unfused = np.empty((n, n_vp, s, s, s), dtype=np.float32) if return_unfused else None
        cvc = np.empty((n * n_vp, 6, s, s, s), dtype=np.float32) if return_cvc else None
        _lib.check(self._lib.sn_cvc_forward(self._h, n, n_vp, _lib.ptr(pairs), _lib.ptr(xyz), _lib.ptr(resol), _lib.ptr(m),
                                            _lib.ptr(w), _lib.ptr(fused), _lib.ptr(unfused), _lib.ptr(cvc)))
        return fused, unfused, cvc

    def relative_weights(self, features, n_vp):
        f = np.ascontiguousarray(features, dtype=np.float32)
        if f.ndim != 2 or f.shape[1] != _weights.D_VIEWPAIR_FEATURE or f.shape[0] % n_vp:
            raise TypeError("features must have shape (n*n_vp, %d)" % _weights.D_VIEWPAIR_FEATURE)
        n = f.shape[0] // n_vp
        out = np.empty((n, n_vp), dtype=np.float32)
        _lib.check(self._lib.sn_relative_weights(self._h, n, n_vp, _lib.ptr(f), _lib.ptr(out)))
        return out

    def viewpair_weights(self, embeddings, dissimilarity, theta):
        """(n_cubes,n_views,128), (n_cubes,P), (n_cubes,P) float32 -> (n_cubes,P) softmax weights over all 2-combinations."""
        e = np.ascontiguousarray(embeddings, dtype=np.float32)
        n, V = e.shape[:2]
        P = V * (V - 1) // 2
        d = np.ascontiguousarray(dissimilarity, dtype=np.float32).reshape(n, P)
        t = np.ascontiguousarray(theta, dtype=np.float32).reshape(n, P)
        out = np.empty((n, P), dtype=np.float32)
        _lib.check(self._lib.sn_viewpair_weights(self._h, n, V, _lib.ptr(e), _lib.ptr(d), _lib.ptr(t), _lib.ptr(out)))
        return out

    def color_fuse(self, cvc_minus_mean, unfused, w, mean=MEAN_CVC_RGBRGB):
        """utils.generate_voxelLevelWeighted_coloredCubes (utils/utils.py:8-42): (n,3,s,s,s) uint8 fused colours from the
        mean-subtracted CVC tensor (n*n_vp,6,s,s,s), the unfused predictions (n,n_vp,s,s,s) and the pair weights (n,n_vp)."""
        s = self.cube_D
        unfused = np.ascontiguousarray(unfused, dtype=np.float32)
        n, n_vp = unfused.shape[:2]
        cvc = np.ascontiguousarray(cvc_minus_mean, dtype=np.float32).reshape(n * n_vp, 6, s, s, s)
        w = np.ascontiguousarray(w, dtype=np.float32).reshape(n, n_vp)
        m = np.ascontiguousarray(mean, dtype=np.float32).reshape(6)
        rgb = np.empty((n, 3, s, s, s), dtype=np.uint8)
        _lib.check(self._lib.sn_color_fuse(self._h, n, n_vp, _lib.ptr(cvc), _lib.ptr(m), _lib.ptr(unfused), _lib.ptr(w), _lib.ptr(rgb)))
        return rgb

    # ---- hot path, device-resident ------------------------------------------------------------------
    # ---- similarityNet / early rejection -------------------------------------------
    def load_simil_param_values(self, values):
        """values: the similarityNet weight file's 30 arrays (weights.SIMIL_PARAM_SHAPES order)."""
        blob, descs = _weights.simil_to_blob(values)
        _lib.check(self._lib.sn_simil_load_weights(self._h, _lib.ptr(blob), blob.size, descs, len(values)))

    def crop_patches(self, view, center_h, center_w):
        """image.cropImgPatches(img=images[view], pyramidRate=1, cubeCenter_hw=(center_h, center_w)) -> (n,64,64,3) uint8."""
        ch = np.ascontiguousarray(center_h, dtype=np.float64).reshape(-1)
        cw = np.ascontiguousarray(center_w, dtype=np.float64).reshape(-1)
        out = np.empty((ch.size, 64, 64, 3), dtype=np.uint8)
        _lib.check(self._lib.sn_crop_patches(self._h, int(view), ch.size, _lib.ptr(ch), _lib.ptr(cw), _lib.ptr(out)))
        return out

    def patch2embedding(self, patches):
        """patch2embedding_fn: preprocessed (n,3,64,64) float32 patches -> (n,128) float32 embeddings."""
        if not isinstance(patches, np.ndarray) or patches.dtype != np.float32 or patches.ndim != 4 or patches.shape[1:] != (3, 64, 64):
            raise TypeError("patches must be a float32 ndarray of shape (n, 3, 64, 64)")
        x = np.ascontiguousarray(patches)
        out = np.empty((x.shape[0], _weights.D_EMBEDDING), dtype=np.float32)
        _lib.check(self._lib.sn_patch2embedding(self._h, x.shape[0], _lib.ptr(x), _lib.ptr(out)))
        return out

    def crop_embed(self, view, center_h, center_w, mean_bgr):
        """crop + preprocess + embedding of n cube centres of one view without leaving HBM -> (n,128)."""
        ch = np.ascontiguousarray(center_h, dtype=np.float64).reshape(-1)
        cw = np.ascontiguousarray(center_w, dtype=np.float64).reshape(-1)
        m = np.ascontiguousarray(mean_bgr, dtype=np.float32).reshape(3)
        out = np.empty((ch.size, _weights.D_EMBEDDING), dtype=np.float32)
        _lib.check(self._lib.sn_crop_embed(self._h, int(view), ch.size, _lib.ptr(ch), _lib.ptr(cw), _lib.ptr(m), _lib.ptr(out)))
        return out

    def embeddingpair2simil(self, emb_pairs):
        """embeddingPair2simil_fn: (2n,128) float32 (rows 2i, 2i+1 = pair i) -> (n,1) float32."""
        if not isinstance(emb_pairs, np.ndarray) or emb_pairs.dtype != np.float32 or emb_pairs.ndim != 2 or emb_pairs.shape[1] != _weights.D_EMBEDDING \
                or emb_pairs.shape[0] % 2:
            raise TypeError("embeddingPair must be a float32 matrix (2n, %d)" % _weights.D_EMBEDDING)
        e = np.ascontiguousarray(emb_pairs)
        out = np.empty((e.shape[0] // 2, 1), dtype=np.float32)
        _lib.check(self._lib.sn_embeddingpair2simil(self._h, e.shape[0] // 2, _lib.ptr(e), _lib.ptr(out)))
        return out

    def embeddings2simil(self, embeddings):
        """(n_cubes, n_views, 128) float32 -> (n_cubes, n_views*(n_views-1)/2) float32, all 2-combinations of views."""
        e = np.ascontiguousarray(embeddings, dtype=np.float32)
        if e.ndim != 3 or e.shape[2] != _weights.D_EMBEDDING or e.shape[1] < 2:
            raise TypeError("embeddings must have shape (n_cubes, n_views >= 2, %d)" % _weights.D_EMBEDDING)
        out = np.empty((e.shape[0], e.shape[1] * (e.shape[1] - 1) // 2), dtype=np.float32)
        _lib.check(self._lib.sn_embeddings2simil(self._h, e.shape[0], e.shape[1], _lib.ptr(e), _lib.ptr(out)))
        return out

    def project(self, xyz_3D, projection_M=None, return_int_hw=True, return_depth=False):
        """camera.perspectiveProj (utils/camera.py:123-184) of (n,3) points through V cameras in one launch: projection_M
        (V,3,4) float64, or None = the cameras of set_cameras -> img_h, img_w [, depth], each (V, n); int64 when
        return_int_hw (numpy's .round().astype(int64)), else float64."""
        pts = np.ascontiguousarray(xyz_3D, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError("points must have shape (n, 3), got %s" % (pts.shape,))
        M = None if projection_M is None else np.ascontiguousarray(projection_M, dtype=np.float64)
        if M is not None and (M.ndim != 3 or M.shape[1:] != (3, 4)):
            raise ValueError("projection_M must have shape (V, 3, 4), got %s" % (M.shape,))
        n, V = pts.shape[0], (self.n_cameras if M is None else M.shape[0])
        h = np.empty((V, n), dtype=np.float64)
        w = np.empty((V, n), dtype=np.float64)
        d = np.empty((V, n), dtype=np.float64) if return_depth else None
        _lib.check(self._lib.sn_project_points(self._h, V, _lib.ptr(M), n, _lib.ptr(pts), 1 if return_int_hw else 0, _lib.ptr(h), _lib.ptr(w),
                                               _lib.ptr(d)))
        if return_int_hw:
            h, w = h.astype(np.int64), w.astype(np.int64)
        return (h, w, d) if return_depth else (h, w)

    # ---- post-pass ----------------------------------------------------------------
    def ray_pool(self, selected_viewPairs, xyz, resol, prediction, prediction_thresh=None):
        """rayPooling.rayPooling_1cube_numpy (utils/rayPooling.py:143-260) for n cubes: prediction (n,s,s,s) (or
        (n,1,s,s,s)) probabilities >= 0, compared as float16 -> votes (n,s,s,s) uint8."""
        pairs, xyz, resol, n, n_vp = self._batch_args(selected_viewPairs, xyz, resol)
        s = self.cube_D
        pred = np.ascontiguousarray(np.asarray(prediction).astype(np.float16).astype(np.float32).reshape(n, s, s, s))
        votes = np.empty((n, s, s, s), dtype=np.uint8)
        use = 0 if prediction_thresh is None else 1
        thr = 0.0 if prediction_thresh is None else float(np.float16(prediction_thresh))
        _lib.check(self._lib.sn_ray_pool(self._h, n, n_vp, _lib.ptr(pairs), _lib.ptr(xyz), _lib.ptr(resol), _lib.ptr(pred), use, thr,
                                         _lib.ptr(votes)))
        return votes

    def dense2sparse(self, prediction, rgb, selected_viewPairs, xyz, resol, min_prob=0.5, rayPool_thresh=0, enable_centerCrop=False,
                     cube_Dcenter=None, enable_rayPooling=False):
        """sparseCubes.dense2sparse (utils/sparseCubes.py:9-77) on the GPU. prediction (n,s,s,s) or (n,1,s,s,s) float;
        rgb (n,3,s,s,s) uint8 or None. Returns (offsets (n+1,) int64, ijk (T,3) u8, pred (T,) f16, rgb (T,3) u8 | None,
        votes (T,) u8 | None): cube i owns rows offsets[i]:offsets[i+1]."""
        pairs, xyz, resol, n, n_vp = self._batch_args(selected_viewPairs, xyz, resol)
        s = self.cube_D
        pred = np.ascontiguousarray(np.asarray(prediction).astype(np.float16).astype(np.float32).reshape(n, s, s, s))
        dc = int(cube_Dcenter) if enable_centerCrop else s
        cap = n * dc ** 3
        cfg = _lib.SparseCfg(float(np.float16(min_prob)), int(rayPool_thresh), int(bool(enable_centerCrop)), dc, int(bool(enable_rayPooling)))
        rgb_in = None if rgb is None else np.ascontiguousarray(rgb, dtype=np.uint8).reshape(n, 3, s, s, s)
        offsets = np.zeros((n + 1,), dtype=np.int64)
        ijk = np.empty((cap, 3), dtype=np.uint8)
        p16 = np.empty((cap,), dtype=np.float16)
        rgb_out = None if rgb is None else np.empty((cap, 3), dtype=np.uint8)
        votes = np.empty((cap,), dtype=np.uint8) if enable_rayPooling else None
        _lib.check(self._lib.sn_dense2sparse(self._h, n, n_vp, _lib.ptr(pairs), _lib.ptr(xyz), _lib.ptr(resol), _lib.ptr(pred), _lib.ptr(rgb_in),
                                             ctypes.byref(cfg), _lib.ptr(offsets), _lib.ptr(ijk), _lib.ptr(p16), _lib.ptr(rgb_out),
                                             _lib.ptr(votes)))
        T = int(offsets[-1])
        return offsets, ijk[:T], p16[:T], (None if rgb_out is None else rgb_out[:T]), (None if votes is None else votes[:T])

    @staticmethod
    def _packed(offsets, ijk, cube_ijk):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        n = offsets.size - 1
        ijk = np.ascontiguousarray(ijk, dtype=np.uint8).reshape(-1, 3)
        cube = np.asarray(cube_ijk).reshape(n, 3)
        if cube.size and (cube.min() < 0 or cube.max() > 0xFFFFFFFF):
            raise ValueError("cube ijk must lie in [0, 2^32)")
        return offsets, n, ijk, np.ascontiguousarray(cube, dtype=np.uint32)

    @staticmethod
    def _masked(offsets, ijk, mask, normals=None):
        """(mask as (T,) uint8, T = offsets[-1]) of packed lists whose ijk, mask (and normals, when given) all have T rows."""
        m = np.ascontiguousarray(mask, dtype=bool).reshape(-1).view(np.uint8)
        T = int(offsets[-1])
        rows = [(ijk.shape[0], "ijk rows"), (m.size, "mask entries")] + ([] if normals is None else [(normals.shape[0], "normals")])
        if any(r != T for r, _ in rows):
            raise ValueError("offsets end at %d voxels: %s" % (T, ", ".join("%d %s" % row for row in rows)))
        return m, T

    @contextlib.contextmanager
    def _on_device(self, arrays, upload=True):
        """The numpy arrays in device memory for the length of a `with` block: yields their device pointers (16 bytes at least each; upload=False:
        room only, for outputs) and frees them on the way out."""
        bufs = []
        try:
            for a in arrays:
                bufs.append(self.dev_alloc(max(a.nbytes, 16)))
                if upload and a.nbytes:
                    self.h2d(bufs[-1], a)
            yield bufs
        finally:
            for b in bufs:
                self.dev_free(b)

    def _sized_outputs(self, run, spec, rows, caps, src=None, words=0, sized=()):
        """An entry with sized outputs, in its host form (src None) or its device form (src: the inputs' device pointers): spec = (name, width,
        dtype) of each output in the entry's order, rows(name, sizes) its number of rows when the sizes are caps or counts, run(caps, srcs,
        outs, counts) -> status the C call. The outputs hold caps (a tuple) items and the entry writes what it needs to counts: one c_longlong
        per cap, or (words = N) one array of N of which the words `sized` are those, in the caps' order, and which comes back as "counts" (N,)
        int64. Outputs that are too short come back as SN_ERR_ARG with the counts needed: one retry at exactly those. An entry without caps
        (caps = sized = ()) has every row known up front. Returns {name: the array at its exact rows}; what the entry leaves unwritten is 0."""
        out = {}
        counts = (ctypes.c_longlong * (words or len(caps)))()
        need = lambda: tuple(counts[i] for i in (sized if words else range(len(caps))))
        ptrs = [counts] if words else [ctypes.pointer(ctypes.c_longlong.from_buffer(counts, 8 * i)) for i in range(len(caps))]

        def call(caps):
            for name, w, dt in spec:
                out[name] = np.zeros((rows(name, caps), w) if w > 1 else (rows(name, caps),), dt)
            if src is None:
                return run(caps, (), [_lib.ptr(out[name]) for name, _, _ in spec], ptrs)
            with self._on_device(out.values(), upload=False) as dst:
                rc = run(caps, src, dst, ptrs)
                for (name, _, _), b in zip(spec, dst):
                    r = rows(name, need())
                    if rc == 0 and r:
                        self.d2h(out[name][:r], b)
                return rc

        rc = call(caps)
        if rc == -1 and any(n > cap for n, cap in zip(need(), caps)):
            rc = call(need())
        _lib.check(rc)
        for name, _, _ in spec:                      # one by one: each cap-sized array is released before the next copy is made
            r = rows(name, need())
            out[name] = out[name] if r == out[name].shape[0] else out[name][:r].copy()
        if words:
            out["counts"] = np.asarray(list(counts), np.int64)
        return out

    def _host_or_device(self, entry, device, arrays, run, spec, rows, caps, **counts):
        """An entry with sized outputs on its input arrays (a mesh's verts and faces, packed voxel lists): its host form <entry> or, device=True,
        <entry>_dev on copies staged in device memory here - the same result. run(fn, caps, ins, outs, counts) -> status calls fn, one of the
        two, on the inputs' pointers; the rest as _sized_outputs takes it."""
        fn = getattr(self._lib, entry + "_dev" if device else entry)
        if not device:
            ins = [_lib.ptr(a) for a in arrays]
            return self._sized_outputs(lambda caps, _, outs, n: run(fn, caps, ins, outs, n), spec, rows, caps, **counts)
        with self._on_device(arrays) as src:
            return self._sized_outputs(lambda caps, ins, outs, n: run(fn, caps, ins, outs, n), spec, rows, caps, src, **counts)

    @staticmethod
    def _mesh_arrays(verts, faces, nv=None):
        """-> (verts (V,3) float64, faces (F,nv) int32; nv None: (F,3) or (F,4) as given), both contiguous."""
        v = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
        f = np.ascontiguousarray(faces, dtype=np.int32)
        if nv is not None:
            f = f.reshape(-1, nv)
        elif f.ndim != 2:
            raise ValueError("faces must be (F,3) or (F,4), not %r" % (f.shape,))
        return v, f

    @staticmethod
    def _on_lattice(cfg, origin, resol):
        """cfg with its origin[3] / resol filled: the mm position of lattice point 0 and the cell size."""
        cfg.origin[:] = [float(x) for x in np.asarray(origin, dtype=np.float64).reshape(3)]
        cfg.resol = float(resol)
        return cfg

    def denoise(self, offsets, ijk, cube_ijk, mask, D_cube, Dc):
        """denoising.denoise_crossCubes (utils/denoising.py:150-184) on packed voxel lists: offsets (n+1,) int64, ijk (T,3) uint8 (each < Dc),
        cube_ijk (n,3), mask (T,) bool -> (T,) bool."""
        offsets, n, ijk, cube = self._packed(offsets, ijk, cube_ijk)
        m = np.ascontiguousarray(mask, dtype=bool).reshape(-1).view(np.uint8)
        out = np.zeros((m.size,), dtype=np.uint8)
        _lib.check(self._lib.sn_denoise(self._h, n, int(Dc), int(D_cube), _lib.ptr(offsets), _lib.ptr(ijk), _lib.ptr(cube), _lib.ptr(m), _lib.ptr(out)))
        return out.view(bool)

    def adapthresh(self, offsets, ijk, pred16, votes, cube_ijk, D_cube, N_refine_iter, init_probThresh, max_probThresh, rayPool_thresh, beta, Dc,
                   keep=("thresh", "masks", "denoised", "choice")):
        """adapthresh.adapthresh's computation (utils/adapthresh.py:91-178) on packed voxel lists, every iteration on the GPU. pred16 (T,) float16,
        votes (T,) uint8 or None. Returns a dict: init_denoised (T,) bool and, as listed in `keep`, thresh (N_iter, n) float64, masks /
        denoised (N_iter, T) bool, choice (N_iter, n) int8 (argmin of each active cube's cost, -1 outside the active set)."""
        offsets, n, ijk, cube = self._packed(offsets, ijk, cube_ijk)
        T, it = int(offsets[-1]), int(N_refine_iter)
        p16 = np.ascontiguousarray(pred16, dtype=np.float16).reshape(-1).view(np.uint16)
        v = None if votes is None else np.ascontiguousarray(votes, dtype=np.uint8).reshape(-1)
        cfg = _lib.AdapthreshCfg(it, int(D_cube), float(init_probThresh), float(max_probThresh), float(rayPool_thresh), float(beta))
        out = dict(init_denoised=np.zeros((T,), np.uint8))
        shapes = dict(thresh=((it, n), np.float64), masks=((it, T), np.uint8), denoised=((it, T), np.uint8), choice=((it, n), np.int8))
        for k in keep:
            out[k] = np.zeros(*shapes[k])
        _lib.check(self._lib.sn_adapthresh(self._h, n, int(Dc), ctypes.byref(cfg), _lib.ptr(offsets), _lib.ptr(ijk), _lib.ptr(p16), _lib.ptr(v),
                                           _lib.ptr(cube), _lib.ptr(out["init_denoised"]), _lib.ptr(out.get("thresh")), _lib.ptr(out.get("masks")),
                                           _lib.ptr(out.get("denoised")), _lib.ptr(out.get("choice"))))
        for k in ("init_denoised", "masks", "denoised"):
            if k in out:
                out[k] = out[k].view(bool)
        return out

    def normals(self, offsets, ijk, cube_ijk, mask, stride_vox, cube_xyz=None, cube_resol=None, view_idx=None, cameraTs=None, radius=2,
                min_neighbours=6, return_normals=True, return_moments=False):
        """Oriented normals of the masked voxels of packed voxel lists (sn_normals): offsets (n+1,) int64, ijk (T,3) uint8,
        cube_ijk (n,3), mask (T,) bool, stride_vox the cube stride in voxels; cube_xyz (n,3) / cube_resol (n,) float32, view_idx (n,K) int32 and
        cameraTs (V,3) float64 orient them (needed with return_normals). Returns normals (T,3) float32, moments (T,10) int32, or both as a tuple."""
        offsets, n, ijk, cube = self._packed(offsets, ijk, cube_ijk)
        m, T = self._masked(offsets, ijk, mask)
        cx = cr = vi = cam = nrm = mom = None
        K = V = 0
        if return_normals:
            cx = np.ascontiguousarray(cube_xyz, dtype=np.float32).reshape(n, 3)
            cr = np.ascontiguousarray(cube_resol, dtype=np.float32).reshape(n)
            vi = np.ascontiguousarray(np.asarray(view_idx).reshape(n, -1) if n else np.zeros((0, 1)), dtype=np.int32)
            cam = np.ascontiguousarray(cameraTs, dtype=np.float64).reshape(-1, 3)
            K, V = vi.shape[1], cam.shape[0]
            nrm = np.zeros((T, 3), np.float32)
        if return_moments:
            mom = np.zeros((T, 10), np.int32)
        cfg = _lib.NormalsCfg(int(radius), int(min_neighbours), int(stride_vox), V, K)
        _lib.check(self._lib.sn_normals(self._h, n, ctypes.byref(cfg), _lib.ptr(offsets), _lib.ptr(ijk), _lib.ptr(cube), _lib.ptr(m), _lib.ptr(cx),
                                        _lib.ptr(cr), _lib.ptr(vi), _lib.ptr(cam), _lib.ptr(nrm), _lib.ptr(mom)))
        if return_normals and return_moments:
            return nrm, mom
        return nrm if return_normals else mom

    def unique_voxels(self, offsets, ijk, cube_ijk, mask, stride_vox):
        """One voxel per world cell (sn_unique_voxels): (T,) bool, True for a masked voxel with the smallest packed index among the masked voxels
        that share its cell cube_ijk * stride_vox + ijk."""
        offsets, n, ijk, cube = self._packed(offsets, ijk, cube_ijk)
        m, T = self._masked(offsets, ijk, mask)
        keep = np.zeros((T,), np.uint8)
        _lib.check(self._lib.sn_unique_voxels(self._h, n, int(stride_vox), _lib.ptr(offsets), _lib.ptr(ijk), _lib.ptr(cube), _lib.ptr(m), _lib.ptr(keep)))
        return keep.view(bool)

    def components(self, offsets, ijk, cube_ijk, mask, stride_vox, connectivity=26, min_cells=1, device=False):
        """Connected components of the masked voxels' world cells, across cubes (sn_components), on the packed lists
        unique_voxels takes. Returns (label (T,) int32 - the component of the voxel's cell, numbered by the smallest packed index it holds, -1
        unmasked; cells (T,) int32 - the component's size in distinct cells; keep (T,) bool - masked and cells >= min_cells; C). device=True
        stages the lists in device memory here and runs sn_components_dev on them: the same result."""
        offsets, n, ijk, cube = self._packed(offsets, ijk, cube_ijk)
        m, T = self._masked(offsets, ijk, mask)
        cfg = _lib.ComponentsCfg(int(stride_vox), int(connectivity), int(min_cells))
        label, cells, keep = np.full((T,), -1, np.int32), np.zeros((T,), np.int32), np.zeros((T,), np.uint8)
        C = ctypes.c_longlong(0)
        if not device:
            _lib.check(self._lib.sn_components(self._h, n, ctypes.byref(cfg), _lib.ptr(offsets), _lib.ptr(ijk), _lib.ptr(cube), _lib.ptr(m),
                                               _lib.ptr(label), _lib.ptr(cells), _lib.ptr(keep), ctypes.byref(C)))
            return label, cells, keep.view(bool), int(C.value)
        with self._on_device((offsets, ijk, cube, m, label, cells, keep)) as staged:
            _lib.check(self._lib.sn_components_dev(self._h, n, ctypes.byref(cfg), T, *staged, ctypes.byref(C)))
            for a, b in zip((label, cells, keep), staged[4:]):
                if a.nbytes:
                    self.d2h(a, b)
        return label, cells, keep.view(bool), int(C.value)

    def mesh(self, offsets, ijk, cube_ijk, mask, stride_vox, normals, radius=2, reach=0, origin=(0.0, 0.0, 0.0), resol=1.0, cap=None, device=False):
        """Surface-nets mesh of the oriented cloud (sn_mesh): the packed lists unique_voxels takes plus normals (T,3)
        float32 (zero = no normal), origin (3,) / resol the mm position of lattice point 0 and the cell size. Returns a dict: verts_mm (V,3)
        float32, verts_lattice (V,3) float64, vert_cell (V,3) int32, vert_src (V,) int64, quads (Q,4) int32. cap = (vertices, quads) the first
        call's arrays hold (a guess from the voxel count when None); a short guess costs one retry with the exact counts. device=True stages the
        lists in device memory here and runs sn_mesh_dev on them: the same result."""
        offsets, n, ijk, cube = self._packed(offsets, ijk, cube_ijk)
        nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        m, T = self._masked(offsets, ijk, mask, nrm)
        cfg = self._on_lattice(_lib.MeshCfg(int(radius), int(reach), int(stride_vox)), origin, resol)
        caps = (2 * T + 64, 2 * T + 64) if cap is None else (int(cap[0]), int(cap[1]))
        spec = (("verts_mm", 3, np.float32), ("verts_lattice", 3, np.float64), ("vert_cell", 3, np.int32), ("vert_src", 1, np.int64), ("quads", 4, np.int32))
        rows = lambda name, sizes: sizes[1] if name == "quads" else sizes[0]
        size = (T,) if device else ()                           # (the device form takes the number of voxels after cfg)
        run = lambda fn, caps, ins, outs, counts: fn(self._h, n, ctypes.byref(cfg), *size, *ins, caps[0], caps[1], *outs, *counts)
        return self._host_or_device("sn_mesh", device, (offsets, ijk, cube, m, nrm), run, spec, rows, caps)

    def mesh_sample(self, vertices, faces, dst, cap=None, device=False):
        """Surface samples of a triangle mesh (sn_mesh_sample): vertices (V,3) float64, faces (F,3) int32, dst the
        sampling density -> (points (M,3) float64, tri (M,) int32 the face of each sample). cap = the samples the first call's arrays hold (a
        guess from the face count when None); a short guess costs one retry with the exact count. device=True stages the mesh in device memory
        here and runs sn_mesh_sample_dev on it: the same result."""
        v, f = self._mesh_arrays(vertices, faces, 3)
        V, F = v.shape[0], f.shape[0]
        run = lambda fn, caps, ins, outs, counts: fn(self._h, V, ins[0], F, ins[1], float(dst), caps[0], *outs, *counts)
        out = self._host_or_device("sn_mesh_sample", device, (v, f), run, (("points", 3, np.float64), ("tri", 1, np.int32)),
                               lambda name, sizes: sizes[0], (16 * F + 64 if cap is None else int(cap),))
        return out["points"], out["tri"]

    def mesh_simplify(self, verts, faces, cell, placement=0, origin=(0.0, 0.0, 0.0), resol=1.0, cap=None, device=False):
        """A triangle mesh made smaller by vertex clustering (sn_mesh_simplify): verts (V,3) float64 in lattice cells,
        faces (F,3) int32, cell = lattice cells per cluster cell and axis (2..64), placement 0 (mean) / 1 (member), origin (3,) / resol as
        Context.mesh takes them. Returns a dict: verts_mm (C,3) float32, verts_lattice (C,3) float64, vert_rep (C,) int32, vert_count (C,) int32,
        faces (G,3) int32, face_src (G,) int32, vert_cluster (V,) int32. cap = (vertices, faces) the first call's arrays hold (the input's
        counts when None, which always suffice); a short cap costs one retry with the exact counts. device=True stages the mesh in device
        memory here and runs sn_mesh_simplify_dev on it: the same result."""
        v, f = self._mesh_arrays(verts, faces, 3)
        V, F = v.shape[0], f.shape[0]
        cfg = self._on_lattice(_lib.MeshSimplifyCfg(int(cell), int(placement)), origin, resol)
        caps = (min(V, 3 * F), F) if cap is None else (int(cap[0]), int(cap[1]))
        spec = (("verts_mm", 3, np.float32), ("verts_lattice", 3, np.float64), ("vert_rep", 1, np.int32), ("vert_count", 1, np.int32),
                ("faces", 3, np.int32), ("face_src", 1, np.int32), ("vert_cluster", 1, np.int32))
        rows = lambda name, sizes: V if name == "vert_cluster" else (sizes[1] if name in ("faces", "face_src") else sizes[0])
        run = lambda fn, caps, ins, outs, counts: fn(self._h, ctypes.byref(cfg), V, ins[0], F, ins[1], caps[0], caps[1], *outs, *counts)
        return self._host_or_device("sn_mesh_simplify", device, (v, f), run, spec, rows, caps)

    def mesh_smooth(self, verts, faces, iterations=10, lam_q16=32768, mu_q16=-34734, boundary=1, origin=(0.0, 0.0, 0.0), resol=1.0, device=False):
        """Taubin smoothing of a mesh in fixed point (sn_mesh_smooth): verts (V,3) float64 in lattice cells, faces (F,3)
        or (F,4) int32, iterations 0..1000, the two factors times 65536, boundary 0 (fixed) / 1 (curve) / 2 (free), origin (3,) / resol as
        Context.mesh takes them. Returns a dict: verts_mm (V,3) float32, verts_lattice (V,3) float64, vert_degree (V,) int32, vert_flags (V,)
        uint8 (1 referenced, 2 boundary vertex, 4 end of a non-manifold edge), counts (4,) int64 = edges, boundary edges, non-manifold edges,
        referenced vertices. device=True stages the mesh in device memory here and runs sn_mesh_smooth_dev on it: the same result."""
        v, f = self._mesh_arrays(verts, faces)
        V, (F, nv) = v.shape[0], f.shape
        cfg = self._on_lattice(_lib.MeshSmoothCfg(int(iterations), int(lam_q16), int(mu_q16), int(boundary)), origin, resol)
        spec = (("verts_mm", 3, np.float32), ("verts_lattice", 3, np.float64), ("vert_degree", 1, np.int32), ("vert_flags", 1, np.uint8))
        run = lambda fn, _, ins, outs, counts: fn(self._h, ctypes.byref(cfg), V, ins[0], F, nv, ins[1], *outs, *counts)
        return self._host_or_device("sn_mesh_smooth", device, (v, f), run, spec, lambda name, sizes: V, (), words=4)

    def mesh_fill(self, verts, faces, max_len=64, orientation=0, origin=(0.0, 0.0, 0.0), resol=1.0, cap=None, device=False):
        """The small holes of a mesh capped by centroid fans (sn_mesh_fill): verts (V,3) float64 in lattice cells, faces
        (F,3) or (F,4) int32, max_len 3..65536 the longest loop that is filled, orientation 0 (holes only) / 1 (any simple loop), origin (3,) /
        resol as Context.mesh takes them. Returns a dict: new_verts_mm (H,3) float32, new_verts_lattice (H,3) float64, loop_root (H,) int32,
        loop_len (H,) int32, new_faces (T,3) int32 into [verts; new_verts], vert_loop (V,) uint8 (0 none, 1 filled, 2 long, 3 rim, 4 complex),
        counts (8,) int64 = edges, boundary edges, boundary components, filled loops, long loops, rims, complex components, new triangles.
        cap = (new vertices, new triangles) the first call's arrays hold (nv * F // 3 and nv * F when None, which always suffice); a short cap
        costs one retry with the exact counts. device=True stages the mesh in device memory here and runs sn_mesh_fill_dev on it: the same
        result."""
        v, f = self._mesh_arrays(verts, faces)
        V, (F, nv) = v.shape[0], f.shape
        cfg = self._on_lattice(_lib.MeshFillCfg(int(max_len), int(orientation)), origin, resol)
        caps = (nv * F // 3, nv * F) if cap is None else (int(cap[0]), int(cap[1]))
        spec = (("new_verts_mm", 3, np.float32), ("new_verts_lattice", 3, np.float64), ("loop_root", 1, np.int32), ("loop_len", 1, np.int32),
                ("new_faces", 3, np.int32), ("vert_loop", 1, np.uint8))
        rows = lambda name, sizes: V if name == "vert_loop" else (sizes[1] if name == "new_faces" else sizes[0])
        run = lambda fn, caps, ins, outs, counts: fn(self._h, ctypes.byref(cfg), V, ins[0], F, nv, ins[1], caps[0], caps[1], *outs, *counts)
        # (no face: either form returns at once and writes nothing, so there is nothing to stage or to copy back)
        return self._host_or_device("sn_mesh_fill", device and F > 0, (v, f), run, spec, rows, caps, words=8, sized=(3, 7))

    def mesh_normals(self, verts, faces, device=False):
        """A mesh's own area-weighted normals with its exact area and volume (sn_mesh_normals): verts (V,3) float64 in
        lattice cells, faces (F,3) or (F,4) int32. Returns a dict: face_normals (F,3) float32, vert_normals (V,3) float32 (zero rows for
        unreferenced vertices), counts (4,) int64 = faces with a zero vector, referenced vertices with a zero vector, referenced vertices,
        triangles, sums (6,) uint64 = the limbs of area2, then of vol6, least significant first. device=True stages the mesh in device memory
        here and runs sn_mesh_normals_dev on it: the same result."""
        v, f = self._mesh_arrays(verts, faces)
        V, (F, nv) = v.shape[0], f.shape
        sums = (ctypes.c_ulonglong * 6)()
        spec = (("face_normals", 3, np.float32), ("vert_normals", 3, np.float32))
        run = lambda fn, _, ins, outs, counts: fn(self._h, V, ins[0], F, nv, ins[1], *outs, *counts, sums)
        out = self._host_or_device("sn_mesh_normals", device, (v, f), run, spec, lambda name, sizes: F if name == "face_normals" else V, (), words=4)
        out["sums"] = np.asarray(list(sums), np.uint64)
        return out

    def mesh_orient(self, verts, faces, sign=0, min_faces=0, keep_largest=False, device=False):
        """A mesh's faces made to turn one way, its pieces and their exact volumes (sn_mesh_orient): verts (V,3) float64
        in lattice cells, faces (F,3) or (F,4) int32, sign 0 (majority) / 1 (outward), min_faces >= 0 the smallest piece that is kept,
        keep_largest the piece with the most faces is kept as well. Returns a dict: faces_out (F,nv) int32, face_flip (F,) uint8,
        face_component (F,) int32 the smallest face of the face's piece, face_keep (F,) uint8, and per piece at the row of its id (zero
        elsewhere) comp_faces (F,) int32, comp_flags (F,) uint8 (1 orientable, 2 closed, 4 flipped, 8 kept), comp_vol6 (F,3) uint64 limbs,
        least significant first; counts (12,) int64 = edges, boundary edges, non-manifold edges, links, inconsistent links, pieces,
        non-orientable, closed, flipped faces, flipped pieces, kept faces, kept pieces. device=True stages the mesh in device memory here and
        runs sn_mesh_orient_dev on it: the same result."""
        v, f = self._mesh_arrays(verts, faces)
        V, (F, nv) = v.shape[0], f.shape
        cfg = _lib.MeshOrientCfg(int(sign), int(min_faces), int(keep_largest))
        spec = (("faces_out", nv, np.int32), ("face_flip", 1, np.uint8), ("face_component", 1, np.int32), ("face_keep", 1, np.uint8),
                ("comp_faces", 1, np.int32), ("comp_flags", 1, np.uint8), ("comp_vol6", 3, np.uint64))
        run = lambda fn, _, ins, outs, counts: fn(self._h, ctypes.byref(cfg), V, ins[0], F, nv, ins[1], *outs, *counts)
        # (no face: either form returns at once and writes nothing, so there is nothing to stage or to copy back)
        return self._host_or_device("sn_mesh_orient", device and F > 0, (v, f), run, spec, lambda name, sizes: F, (), words=12)

    def mesh_intersect(self, verts, faces, cap_pairs=None, device=False):
        """A mesh's self-intersections, exactly (sn_mesh_intersect): verts (V,3) float64 in lattice cells, faces (F,3)
        or (F,4) int32, cap_pairs >= 0 the rows the pair list may hold - a shorter list is truncated, not refused; None: F rows first and, when
        there are more pairs, one more call at exactly their number. Returns a dict: face_hit (F,) uint8, face_pairs (F,) int32, pairs
        (min(P, cap_pairs),2) int32 in ascending (f, g) order, counts (8,) int64 = non-degenerate triangles, degenerate faces, candidate
        triangle pairs tested exactly (depends on the broad phase), intersecting pairs P, faces hit, pairs with a k = 0 hit, pairs with a
        k >= 1 hit only, pairs written. device=True stages the mesh in device memory here and runs sn_mesh_intersect_dev on it: the same
        result."""
        v, f = self._mesh_arrays(verts, faces)
        V, (F, nv) = v.shape[0], f.shape
        spec = (("face_hit", 1, np.uint8), ("face_pairs", 1, np.int32), ("pairs", 2, np.int32))

        def call(cap):
            cfg = _lib.MeshIntersectCfg(cap)
            rows = lambda name, sizes: min(max(sizes[0], 0), max(cap, 0)) if name == "pairs" else F
            run = lambda fn, _, ins, outs, counts: fn(self._h, ctypes.byref(cfg), V, ins[0], F, nv, ins[1], *outs, *counts)
            # (no face: either form returns at once and writes nothing, so there is nothing to stage or to copy back)
            return self._host_or_device("sn_mesh_intersect", device and F > 0, (v, f), run, spec, rows, (cap,), words=8, sized=(3,))

        out = call(F if cap_pairs is None else int(cap_pairs))
        if cap_pairs is None and int(out["counts"][3]) > F:
            out = call(int(out["counts"][3]))
        return out

    DISTANCE_OUTPUTS = ("d2", "face", "closest")

    def mesh_distance(self, verts, faces, pts, max_dist, outputs=DISTANCE_OUTPUTS, device=False):
        """For every point the nearest point of a mesh (sn_mesh_distance): verts (V,3) float64 in world coordinates,
        faces (F,3) or (F,4) int32, pts (n,3) float64, max_dist > 0 the cap. Returns a dict of those of `outputs` that were asked for - d2
        (n,) float64 (+inf beyond the cap), face (n,) int32 (-1 there), closest (n,3) float64 (NaN there) - and counts (8,) int64 =
        triangles, degenerate triangles, points answered, points beyond the cap, (point, triangle) tests run (the broad phase's own
        number), 0, 0, 0. device=True stages the mesh and the points in device memory here and runs sn_mesh_distance_dev on them: the same
        result."""
        v, f = self._mesh_arrays(verts, faces)
        p = self._points(pts)
        V, (F, nv), n = v.shape[0], f.shape, p.shape[0]
        if set(outputs) - set(self.DISTANCE_OUTPUTS):
            raise ValueError("outputs = %r: of %r" % (outputs, self.DISTANCE_OUTPUTS))
        cfg = _lib.MeshDistanceCfg(float(max_dist))
        widths = dict(d2=(1, np.float64), face=(1, np.int32), closest=(3, np.float64))
        spec = tuple((name,) + widths[name] for name in self.DISTANCE_OUTPUTS if name in outputs)

        def run(fn, _, ins, outs, counts):
            given = dict(zip([name for name, _, _ in spec], outs))
            return fn(self._h, ctypes.byref(cfg), V, ins[0], F, nv, ins[1], n, ins[2], *[given.get(name) for name in self.DISTANCE_OUTPUTS], *counts)
        out = self._host_or_device("sn_mesh_distance", device, (v, f, p), run, spec, lambda name, sizes: n, (), words=8)
        if "closest" in out:
            out["closest"] = out["closest"].reshape(n, 3)
        return out

    WINDING_OUTPUTS = ("winding", "crossings", "on_surface")

    def mesh_winding(self, verts, faces, pts, axis=2, outputs=WINDING_OUTPUTS, device=False):
        """For every point how many times a mesh winds around it, exactly (sn_mesh_winding): verts (V,3) float64 in
        lattice cells, faces (F,3) or (F,4) int32, pts (n,3) float64 in lattice cells, axis 0, 1 or 2 the axis the rays run along. Returns a
        dict of those of `outputs` that were asked for - winding (n,) int32 the signed crossings, crossings (n,) int32 their number,
        on_surface (n,) uint8 - and counts (8,) int64 = triangles that can be crossed, triangles parallel to the rays, degenerate triangles,
        points with winding != 0, (point, triangle) entries looked at (the broad phase's own number), points on the surface, 0, 0. device=True stages
        the mesh and the points in device memory here and runs sn_mesh_winding_dev on them: the same result."""
        v, f = self._mesh_arrays(verts, faces)
        p = self._points(pts)
        V, (F, nv), n = v.shape[0], f.shape, p.shape[0]
        if set(outputs) - set(self.WINDING_OUTPUTS):
            raise ValueError("outputs = %r: of %r" % (outputs, self.WINDING_OUTPUTS))
        cfg = _lib.MeshWindingCfg(int(axis), 0)
        widths = dict(winding=(1, np.int32), crossings=(1, np.int32), on_surface=(1, np.uint8))
        spec = tuple((name,) + widths[name] for name in self.WINDING_OUTPUTS if name in outputs)

        def run(fn, _, ins, outs, counts):
            given = dict(zip([name for name, _, _ in spec], outs))
            return fn(self._h, ctypes.byref(cfg), V, ins[0], F, nv, ins[1], n, ins[2], *[given.get(name) for name in self.WINDING_OUTPUTS], *counts)
        return self._host_or_device("sn_mesh_winding", device, (v, f, p), run, spec, lambda name, sizes: n, (), words=8)

    VOXELIZE_OUTPUTS = ("occ", "Y", "per_cube")

    def mesh_voxelize(self, verts, faces, cube_ijk, D, stride_vox, axis=2, modes=3, select=2, outputs=VOXELIZE_OUTPUTS, device=False):
        """A mesh voxelised into cubes, exactly (sn_mesh_voxelize): verts (V,3) float64 in lattice cells, faces (F,3)
        or (F,4) int32, cube_ijk (N,3) int32, D 1..64 the cube side in voxels, stride_vox >= 1 - voxel (n; i,j,k) is the world cell cube_ijk[n]
        * stride_vox + (i,j,k), its centre that lattice point -, axis 0, 1 or 2 the axis the solid bit's rays run along, modes the bits that
        are computed (1 solid, 2 surface, 3 both), select the bits that make Y. Returns a dict of those of `outputs` that were asked for -
        occ (N,D,D,D) uint8 the bits, Y (N,1,D,D,D) float32, per_cube (N,2) int64 solid and surface voxels - and counts (8,) int64 =
        triangles that can be crossed, triangles parallel to the rays, degenerate triangles, solid voxels, surface voxels, voxels with both
        bits, (column, triangle) pairs covered, (voxel, triangle) box tests run (the last two are the broad phase's own numbers).
        device=True stages the mesh and the cubes in device memory here and runs sn_mesh_voxelize_dev on them: the same result."""
        v, f = self._mesh_arrays(verts, faces)
        cube = np.ascontiguousarray(cube_ijk, dtype=np.int32).reshape(-1, 3)
        V, (F, nv), N, D = v.shape[0], f.shape, cube.shape[0], int(D)
        if set(outputs) - set(self.VOXELIZE_OUTPUTS):
            raise ValueError("outputs = %r: of %r" % (outputs, self.VOXELIZE_OUTPUTS))
        cfg = _lib.MeshVoxelizeCfg(int(axis), int(modes), int(select), 0)
        vox = N * D ** 3 if 1 <= D <= 64 else 0                 # (a refused D writes nothing)
        widths = dict(occ=(1, np.uint8), Y=(1, np.float32), per_cube=(2, np.int64))
        spec = tuple((name,) + widths[name] for name in self.VOXELIZE_OUTPUTS if name in outputs)

        def run(fn, _, ins, outs, counts):
            given = dict(zip([name for name, _, _ in spec], outs))
            return fn(self._h, ctypes.byref(cfg), V, ins[0], F, nv, ins[1], N, ins[2], D, int(stride_vox),
                      *[given.get(name) for name in self.VOXELIZE_OUTPUTS], *counts)
        out = self._host_or_device("sn_mesh_voxelize", device, (v, f, cube), run, spec, lambda name, sizes: N if name == "per_cube" else vox, (), words=8)
        if "occ" in out:
            out["occ"] = out["occ"].reshape(N, D, D, D)
        if "Y" in out:
            out["Y"] = out["Y"].reshape(N, 1, D, D, D)
        return out

    def _render_args(self, verts, faces, cameraPOs, shape, near, tol):
        """-> (verts, faces, P or None, V, cfg) of mesh_render and mesh_vertex_colors: cameraPOs (V,3,4), None = the cameras of set_cameras."""
        v, f = self._mesh_arrays(verts, faces)
        P = None if cameraPOs is None else np.ascontiguousarray(cameraPOs, dtype=np.float64)
        if P is not None and (P.ndim != 3 or P.shape[1:] != (3, 4)):
            raise ValueError("cameraPOs must have shape (V, 3, 4), got %s" % (P.shape,))
        V = getattr(self, "n_cameras", 0) if P is None else P.shape[0]
        return v, f, P, V, _lib.MeshRenderCfg(int(shape[0]), int(shape[1]), float(near), float(tol))

    RENDER_OUTPUTS = ("depth", "face", "face_pixels", "vert_visible")

    def mesh_render(self, verts, faces, cameraPOs, shape, near=0.0, tol=0.0, outputs=RENDER_OUTPUTS, device=False):
        """A mesh rendered into V views of one size (sn_mesh_render): verts (n,3) float64 in world coordinates, faces
        (F,3) or (F,4) int32, cameraPOs (V,3,4) float64 or None for the cameras of set_cameras, shape = (H, W), near >= 0, tol >= 0. Returns a
        dict of those of `outputs` that were asked for - depth (V,H,W) float64 (0.0: empty), face (V,H,W) int32 (-1: empty), face_pixels (V,F)
        int32, vert_visible (V,n) uint8 - and counts (8,) int64 = triangles, clipped, degenerate, rasterised, covering pairs, non-empty
        pixels, visible (view, vertex) pairs, 0, summed over the views. device=True stages the mesh and the cameras in device memory here and
        runs sn_mesh_render_dev on them: the same result."""
        v, f, P, V, cfg = self._render_args(verts, faces, cameraPOs, shape, near, tol)
        n, (F, nv), (H, W) = v.shape[0], f.shape, (cfg.H, cfg.W)
        if set(outputs) - set(self.RENDER_OUTPUTS):
            raise ValueError("outputs = %r: of %r" % (outputs, self.RENDER_OUTPUTS))
        size = dict(depth=max(V, 0) * max(H, 0) * max(W, 0), face=max(V, 0) * max(H, 0) * max(W, 0), face_pixels=max(V, 0) * F, vert_visible=max(V, 0) * n)
        shapes = dict(depth=(V, H, W), face=(V, H, W), face_pixels=(V, F), vert_visible=(V, n))
        dtypes = dict(depth=np.float64, face=np.int32, face_pixels=np.int32, vert_visible=np.uint8)
        spec = tuple((name, 1, dtypes[name]) for name in self.RENDER_OUTPUTS if name in outputs)

        def run(fn, _, ins, outs, counts):
            given = dict(zip([name for name, _, _ in spec], outs))
            return fn(self._h, ctypes.byref(cfg), n, ins[0], F, nv, ins[1], V, ins[2] if P is not None else None,
                      *[given.get(name) for name in self.RENDER_OUTPUTS], *counts)
        out = self._host_or_device("sn_mesh_render", device, (v, f) + (() if P is None else (P,)), run, spec, lambda name, sizes: size[name], (), words=8)
        for name, _, _ in spec:
            out[name] = out[name].reshape(shapes[name])
        return out

    def mesh_vertex_colors(self, verts, faces, cameraPOs, shape, vert_visible, near=0.0, tol=0.0, device=False):
        """The colour of every vertex from the views that see it (sn_mesh_vertex_colors): the mesh, cameras and shape
        of mesh_render, vert_visible (V,n) - mesh_render's, or any other -, the images of set_images, which must be V images of H x W.
        Returns a dict: vert_views (n,) int32 the contributing views, vert_rgb (n,3) uint8 the rounded mean of their nearest pixels ((0,0,0)
        without a view), counts (2,) int64 = coloured vertices, contributing (view, vertex) pairs. device=True: sn_mesh_vertex_colors_dev."""
        v, f, P, V, cfg = self._render_args(verts, faces, cameraPOs, shape, near, tol)
        n, (F, nv) = v.shape[0], f.shape
        vis = np.ascontiguousarray(vert_visible, dtype=np.uint8)
        if vis.shape != (V, n):
            raise ValueError("vert_visible must have shape (V, n_verts) = (%d, %d), got %s" % (V, n, vis.shape))
        spec = (("vert_views", 1, np.int32), ("vert_rgb", 3, np.uint8))
        k = 2 if P is None else 3

        def run(fn, _, ins, outs, counts):
            return fn(self._h, ctypes.byref(cfg), n, ins[0], F, nv, ins[1], V, ins[2] if P is not None else None, ins[k], *outs, *counts)
        out = self._host_or_device("sn_mesh_vertex_colors", device, (v, f) + (() if P is None else (P,)) + (vis,), run, spec, lambda name, sizes: n, (), words=2)
        out["vert_rgb"] = out["vert_rgb"].reshape(n, 3)
        return out

    @staticmethod
    def _points(xyz):
        return np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3))

    def point_reduce(self, xyz, rank, dst):
        """reducePts_haa of the DTU kit: xyz (n,3), rank (n,) a permutation of 0..n-1 (the visiting order's inverse) -> (keep (n,) bool, rounds):
        the greedy maximal independent set under d^2 <= dst^2, visiting the points in ascending rank."""
        p = self._points(xyz)
        r = np.ascontiguousarray(rank, dtype=np.int64).reshape(-1)
        if r.size != p.shape[0]:
            raise ValueError("rank has %d entries for %d points" % (r.size, p.shape[0]))
        keep = np.zeros((p.shape[0],), np.uint8)
        rounds = ctypes.c_int(0)
        _lib.check(self._lib.sn_point_reduce(self._h, p.shape[0], _lib.ptr(p), _lib.ptr(r), float(dst), _lib.ptr(keep), ctypes.byref(rounds)))
        return keep.view(bool), rounds.value

    def nn_dist2(self, to, frm, max_dist):
        """MaxDistCP's search: (n_from,) float64 min_j d^2(frm_i, to_j), exact when below max_dist^2 (1 + 2^-40), else +inf."""
        t, f = self._points(to), self._points(frm)
        d2 = np.zeros((f.shape[0],), np.float64)
        _lib.check(self._lib.sn_nn_dist2(self._h, t.shape[0], _lib.ptr(t), f.shape[0], _lib.ptr(f), float(max_dist), _lib.ptr(d2)))
        return d2

    def point_flags(self, xyz, mask=None, bb_min=None, res=None, plane=None):
        """DataInMask (mask (X,Y,Z) uint8, bb_min (3,), res; None: not computed) and StlAbovePlane (plane (4,); None: not computed) of xyz (n,3)
        -> (in_mask, above), (n,) bool arrays or None."""
        p = self._points(xyz)
        n = p.shape[0]
        in_mask = above = m = dims = bb = pl = None
        if mask is not None:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            if m.ndim != 3:
                raise ValueError("mask must be 3-D")
            dims = np.asarray(m.shape, dtype=np.int32)
            bb = np.ascontiguousarray(bb_min, dtype=np.float64).reshape(3)
            in_mask = np.zeros((n,), np.uint8)
        if plane is not None:
            pl = np.ascontiguousarray(plane, dtype=np.float64).reshape(4)
            above = np.zeros((n,), np.uint8)
        _lib.check(self._lib.sn_point_flags(self._h, n, _lib.ptr(p), _lib.ptr(m), _lib.ptr(dims), _lib.ptr(bb), float(res) if mask is not None else 0.0,
                                            _lib.ptr(pl), _lib.ptr(in_mask), _lib.ptr(above)))
        return (None if in_mask is None else in_mask.view(bool)), (None if above is None else above.view(bool))

    @staticmethod
    def _ptcubes_cfg(pts_f64, compute_f64, stride_q, stride_xyz, half, box):
        cfg = _lib.PtCubesCfg(int(bool(pts_f64)), int(bool(compute_f64)), float(stride_q), float(stride_xyz), float(half), int(box is not None))
        if box is not None:
            b = np.asarray(box, dtype=np.float64).reshape(2, 3)
            cfg.lo[:], cfg.hi[:] = b[0].tolist(), b[1].tolist()
        return cfg

    _PTCUBES_OUT = (("ijk", 3, np.uint32), ("xyz", 3, np.float32))

    def ptcubes(self, pts, stride_q, stride_xyz, half, compute_f64, box=None, cap=None):
        """The cell list of scene.quantizePts2Cubes (sn_ptcubes): pts (n,3) float32 or float64; stride_q the stride of the cell index (in the
        type compute_f64 names), stride_xyz the stride as float64, half = cube_D_mm / 2, box (2,3) = [lo, hi] or None. Returns (ijk (m,3) uint32,
        xyz (m,3) float32), cells in ascending (i, j, k); m = 0 when no point is kept."""
        p = np.asarray(pts)
        if p.dtype not in (np.float32, np.float64):
            p = p.astype(np.float64)
        p = np.ascontiguousarray(p.reshape(-1, 3))
        n = p.shape[0]
        cfg = self._ptcubes_cfg(p.dtype == np.float64, compute_f64, stride_q, stride_xyz, half, box)
        run = lambda caps, _, outs, counts: self._lib.sn_ptcubes(self._h, n, _lib.ptr(p), ctypes.byref(cfg), caps[0], *outs, *counts)
        out = self._sized_outputs(run, self._PTCUBES_OUT, lambda name, sizes: sizes[0], (min(2 * n, 1 << 22) if cap is None else int(cap),))
        return out["ijk"], out["xyz"]

    def _ptcubes_dev_sized(self, run, cap):
        """The device-output forms: run(cap, ijk_dev, xyz_dev, n_cells) -> status. Returns the arrays on the host."""
        call = lambda caps, _, outs, counts: run(caps[0], outs[0], outs[1], counts[0])
        out = self._sized_outputs(call, self._PTCUBES_OUT, lambda name, sizes: sizes[0], (cap,), src=())
        return out["ijk"], out["xyz"]

    def ptcubes_dev(self, n, pts_dev, pts_f64, stride_q, stride_xyz, half, compute_f64, box=None, cap=None):
        """ptcubes for n points already in HBM (sn_ptcubes_dev); the cell list is built in device memory and returned on the host."""
        cfg = self._ptcubes_cfg(pts_f64, compute_f64, stride_q, stride_xyz, half, box)
        run = lambda cap, ijk_dev, xyz_dev, n_cells: self._lib.sn_ptcubes_dev(self._h, int(n), pts_dev, ctypes.byref(cfg), cap, ijk_dev, xyz_dev,
                                                                              n_cells)
        return self._ptcubes_dev_sized(run, min(2 * int(n), 1 << 22) if cap is None else int(cap))

    def ptcubes_sparse(self, offsets, vxl_ijk, mask, cube_xyz, cube_resol, stride_q, stride_xyz, half, compute_f64, box=None, cap=None):
        """The cell list around the masked voxels of packed sparse lists (sn_ptcubes_sparse_dev): offsets (n+1,) int64, vxl_ijk (T,3) uint8, mask
        (T,) bool, cube_xyz (n,3) / cube_resol (n,) float32. The voxels' points - float32(ijk) * resol + xyz of their cube - are formed on the
        GPU and never reach the host."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        n = offsets.size - 1
        ijk = np.ascontiguousarray(vxl_ijk, dtype=np.uint8).reshape(-1, 3)
        m, T = self._masked(offsets, ijk, mask)
        cx = np.ascontiguousarray(cube_xyz, dtype=np.float32).reshape(n, 3)
        cr = np.ascontiguousarray(cube_resol, dtype=np.float32).reshape(n)
        cfg = self._ptcubes_cfg(False, compute_f64, stride_q, stride_xyz, half, box)
        dev = [self.upload(a) for a in (offsets, ijk, m, cx, cr)]
        try:
            run = lambda cap, ijk_dev, xyz_dev, n_cells: self._lib.sn_ptcubes_sparse_dev(self._h, n, T, dev[0], dev[1], dev[2], dev[3], dev[4],
                                                                                         ctypes.byref(cfg), cap, ijk_dev, xyz_dev, n_cells)
            return self._ptcubes_dev_sized(run, min(2 * T, 1 << 22) if cap is None else int(cap))
        finally:
            for d in dev:
                self.dev_free(d)

    # ---- ground-truth mode (surfacenet_amd/groundTruth.py) -------------------------
    def gt_bind(self, pts_xyz, cell):
        """Binds a ground-truth cloud (sn_gt_bind): pts_xyz (n,3), converted with np.asarray(pts, np.float32); cell > 0 the edge of the grid the
        points are sorted into (speed only). Rebinding replaces the cloud. Returns the number of points."""
        p = np.ascontiguousarray(np.asarray(pts_xyz, np.float32).reshape(-1, 3))
        self._gt_serial = getattr(self, "_gt_serial", 0) + 1
        _lib.check(self._lib.sn_gt_bind(self._h, p.shape[0], _lib.ptr(p), float(cell)))
        return p.shape[0]

    def gt_bind_dev(self, n, pts_dev, cell):
        """gt_bind for n float32 points already in HBM (sn_gt_bind_dev)."""
        self._gt_serial = getattr(self, "_gt_serial", 0) + 1
        _lib.check(self._lib.sn_gt_bind_dev(self._h, int(n), pts_dev, float(cell)))

    def bind_points(self, pts_xyz, cube_D_mm):
        """groundTruth.bind_points in this context: the grid cell is a quarter of the cube side. Returns the bound cloud (groundTruth.BoundCloud)."""
        from . import groundTruth
        return groundTruth.BoundCloud(self, pts_xyz, cube_D_mm)

    @staticmethod
    def _cube_params(cubes):
        """cubes_param_np (a structured array with 'xyz' and 'resol') or a pair (xyz (n,3), resol (n,) or scalar) -> float32 (n,3), (n,)."""
        if isinstance(cubes, np.ndarray) and cubes.dtype.names:
            xyz, resol = cubes["xyz"], cubes["resol"]
        else:
            xyz, resol = cubes
        xyz = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3))
        resol = np.ascontiguousarray(np.broadcast_to(np.asarray(resol, np.float32).reshape(-1), (xyz.shape[0],)))
        return xyz, resol

    def gt_cubes(self, cubes):
        """The occupancy tensors of cubes (cubes_param_np or (xyz, resol)) from the bound cloud (sn_gt_cubes): Y (n,1,s,s,s) float32,
        Y[c,0,q] = 1 iff some point has floor((p - xyz_c) / resol_c) == q in float32."""
        xyz, resol = self._cube_params(cubes)
        s, n = self.cube_D, xyz.shape[0]
        Y = np.zeros((n, 1, s, s, s), np.float32)
        _lib.check(self._lib.sn_gt_cubes(self._h, n, _lib.ptr(xyz), _lib.ptr(resol), _lib.ptr(Y)))
        return Y

    def gt_cubes_dev(self, n, xyz_dev, resol_dev, Y_dev):
        _lib.check(self._lib.sn_gt_cubes_dev(self._h, int(n), xyz_dev, resol_dev, Y_dev))

    def _check_target(self, Y, n, what="Y"):
        s = self.cube_D
        if not isinstance(Y, np.ndarray) or Y.dtype != np.float32 or Y.ndim != 5:
            raise TypeError("%s must be a float32 5-D ndarray" % what)
        if Y.shape != (n, 1, s, s, s):
            raise TypeError("%s must have shape (%d, 1, %d, %d, %d), got %s" % (what, n, s, s, s, Y.shape))
        return np.ascontiguousarray(Y)

    def weighted_accuracy_counts(self, pred, Y, threshold=0.5):
        """(n,4) int64: per cube n_pos, n_neg, hit_pos, hit_neg of pred against Y, both (n,1,s,s,s) float32 (sn_weighted_accuracy)."""
        if not isinstance(pred, np.ndarray) or pred.ndim != 5:
            raise TypeError("pred must be a float32 5-D ndarray")
        pred = self._check_target(pred, pred.shape[0], "pred")
        Y = self._check_target(Y, pred.shape[0])
        counts = np.zeros((pred.shape[0], 4), np.int64)
        _lib.check(self._lib.sn_weighted_accuracy(self._h, pred.shape[0], _lib.ptr(pred), _lib.ptr(Y), float(threshold), _lib.ptr(counts)))
        return counts

    def weighted_accuracy_dev(self, n, pred_dev, Y_dev, counts_dev, threshold=0.5):
        _lib.check(self._lib.sn_weighted_accuracy_dev(self._h, int(n), pred_dev, Y_dev, float(threshold), counts_dev))

    def weighted_accuracy(self, pred, Y, threshold=0.5, per_cube=False):
        """groundTruth.weighted_accuracy in this context: np.float64 accuracy of the whole batch [, (n,4) per-cube counts]."""
        from . import groundTruth
        counts = self.weighted_accuracy_counts(pred, Y, threshold)
        acc = groundTruth.accuracy_from_counts(counts)
        return (acc, counts) if per_cube else acc

    def forward_gt(self, X, w, Y, n_vp=1, threshold=0.5):
        """`forward` in ground-truth mode: -> (fused, unfused, counts (n,4) int64). The counts are taken on the device from the fused tensor
        before it is copied back (sn_forward_dev, sn_weighted_accuracy_dev); Y goes up, it never comes down. Same argument checks as `forward`."""
        s = self.cube_D
        if not isinstance(X, np.ndarray) or X.dtype != np.float32:
            raise TypeError("X must be a float32 ndarray (the reference's Theano function rejects other dtypes)")
        if X.ndim != 5 or X.shape[1:] != (6, s, s, s):
            raise TypeError("X must have shape (N*n_vp, 6, %d, %d, %d), got %s" % (s, s, s, X.shape))
        if X.shape[0] % n_vp:
            raise ValueError("X.shape[0]=%d is not a multiple of n_vp=%d" % (X.shape[0], n_vp))
        n = X.shape[0] // n_vp
        X = np.ascontiguousarray(X)
        if n_vp > 1:
            if not isinstance(w, np.ndarray) or w.dtype != np.float32 or w.shape != (n, n_vp):
                raise TypeError("w must be a float32 ndarray of shape (%d, %d)" % (n, n_vp))
            w = np.ascontiguousarray(w)
        else:
            w = None
        Y = self._check_target(Y, n)
        if n_vp > self.max_samples:
            raise ValueError("n_vp exceeds the context's max_samples")
        fused = np.empty((n, 1, s, s, s), dtype=np.float32)
        unfused = np.empty((n, n_vp, s, s, s), dtype=np.float32)
        counts = np.zeros((n, 4), np.int64)
        step = self.max_samples // n_vp                  # the chunks of sn_forward
        m0, v = min(step, n), s ** 3
        if n == 0:
            return fused, unfused, counts
        d = [self.dev_alloc(m0 * n_vp * 6 * v * 4), self.dev_alloc(m0 * n_vp * 4), self.dev_alloc(m0 * v * 4), self.dev_alloc(m0 * v * 4),
             self.dev_alloc(m0 * n_vp * v * 4), self.dev_alloc(m0 * 32)]
        dX, dw, dY, dF, dU, dC = d
        try:
            for i0 in range(0, n, step):
                i1 = min(n, i0 + step)
                m = i1 - i0
                self.h2d(dX, X[i0 * n_vp:i1 * n_vp])
                if w is not None:
                    self.h2d(dw, w[i0:i1])
                self.h2d(dY, Y[i0:i1])
                _lib.check(self._lib.sn_forward_dev(self._h, m, n_vp, dX, dw if w is not None else None, dF, dU))
                self.weighted_accuracy_dev(m, dF, dY, dC, threshold)
                self.d2h(fused[i0:i1], dF)
                self.d2h(unfused[i0:i1], dU)
                self.d2h(counts[i0:i1], dC)
                self.synchronize()
        finally:
            for p in d:
                self.dev_free(p)
        return fused, unfused, counts

    # ---- training the view-pair weighting net, SurfaceNet frozen (training.py) ----------------------------------
    RELW_UPDATES = {"none": 0, "sgd": 1, "nesterov_momentum": 2}
    # offsets of sn_relw_train_grads / sn_relw_train_velocities (W1 | beta | gamma | w2 | b2 [| mu | istd]) and of sn_relw_get_params
    _RELW_G = (("W1", 25800, (258, 100)), ("beta", 100, (100,)), ("gamma", 100, (100,)), ("w2", 100, (100,)), ("b2", 1, (1,)),
               ("mu", 100, (100,)), ("istd", 100, (100,)))
    _RELW_P = ((25800, (258, 100)), (100, (100,)), (100, (100,)), (100, (100,)), (100, (100,)), (100, (100, 1)), (1, (1,)))

    def relw_train_begin(self, lr, momentum=0.9, update="nesterov_momentum", w_for_1=0.96, l2=0.0, bn_alpha=0.1, bn_eps=1e-4, clip=1e-7):
        """Starts a training session from the loaded weights (sn_relw_train_begin). update: 'none' (gradients only), 'sgd', 'nesterov_momentum'."""
        if update not in self.RELW_UPDATES:
            raise ValueError("update must be one of %s" % sorted(self.RELW_UPDATES))
        cfg = _lib.RelwTrainCfg(float(lr), float(momentum), float(w_for_1), float(l2), float(bn_alpha), float(bn_eps), float(clip),
                                self.RELW_UPDATES[update])
        _lib.check(self._lib.sn_relw_train_begin(self._h, ctypes.byref(cfg)))

    def relw_train_end(self):
        _lib.check(self._lib.sn_relw_train_end(self._h))

    def _check_train_args(self, first, features, Y, n_vp, first_is_X):
        return check_train_args(self.cube_D, first, features, Y, n_vp, first_is_X)

    def relw_train_step(self, unfused, features, Y, n_vp):
        """One step on cached predictions (sn_relw_train_step): unfused (n,n_vp,s,s,s), features (n*n_vp,258), Y (n,1,s,s,s), all float32.
        -> (loss float, counts (n,4) int64, fused (n,1,s,s,s), w (n,n_vp))."""
        n = self._check_train_args(unfused, features, Y, n_vp, False)
        s = self.cube_D
        U, F, Yc = np.ascontiguousarray(unfused), np.ascontiguousarray(features), np.ascontiguousarray(Y)
        fused, w, counts = np.empty((n, 1, s, s, s), np.float32), np.empty((n, n_vp), np.float32), np.zeros((n, 4), np.int64)
        loss = ctypes.c_double(0.0)
        _lib.check(self._lib.sn_relw_train_step(self._h, n, int(n_vp), _lib.ptr(U), _lib.ptr(F), _lib.ptr(Yc), _lib.ptr(fused), _lib.ptr(w),
                                                _lib.ptr(counts), ctypes.byref(loss)))
        return loss.value, counts, fused, w

    def relw_train_step_dev(self, n, n_vp, unfused_dev, features_dev, Y_dev, fused_dev=None, weights_dev=None, counts_dev=None, want_loss=False):
        """sn_relw_train_step_dev on device arrays; asynchronous on the context's stream unless want_loss (then the loss is returned)."""
        loss = ctypes.c_double(0.0)
        _lib.check(self._lib.sn_relw_train_step_dev(self._h, int(n), int(n_vp), unfused_dev, features_dev, Y_dev, fused_dev, weights_dev, counts_dev,
                                                    ctypes.byref(loss) if want_loss else None))
        return loss.value if want_loss else None

    def relw_train_fn(self, X, features, Y, n_vp):
        """The same step from the colored cubes X (n*n_vp,6,s,s,s): the frozen SurfaceNet runs first (sn_forward_dev, BN folded, as in inference)
        and its unfused predictions go to the step without leaving the device. The batch statistics span the whole batch, so it is one step:
        n * n_vp <= max_samples. -> (loss, counts, fused, w) as relw_train_step."""
        n = self._check_train_args(X, features, Y, n_vp, True)
        s, S = self.cube_D, n * int(n_vp)
        if S > self.max_samples:
            raise ValueError("a training step is one batch: n * n_vp = %d exceeds the context's max_samples = %d" % (S, self.max_samples))
        v = s ** 3
        fused, w, counts = np.empty((n, 1, s, s, s), np.float32), np.empty((n, n_vp), np.float32), np.zeros((n, 4), np.int64)
        d = [self.dev_alloc(S * 6 * v * 4), self.dev_alloc(S * v * 4), self.dev_alloc(S * v * 4), self.dev_alloc(S * _weights.D_VIEWPAIR_FEATURE * 4),
             self.dev_alloc(n * v * 4), self.dev_alloc(S * 4), self.dev_alloc(n * 32)]
        dX, dU, dF1, dF, dY, dW, dC = d
        try:
            self.h2d(dX, X)
            self.h2d(dF, features)
            self.h2d(dY, Y)
            # the S samples as S one-pair cubes: the fused tensor of that call (dF1) is the unfused one again, and no weights are needed
            _lib.check(self._lib.sn_forward_dev(self._h, S, 1, dX, None, dF1, dU))
            loss = self.relw_train_step_dev(n, n_vp, dU, dF, dY, dF1, dW, dC, want_loss=True)
            self.d2h(fused, dF1)
            self.d2h(w, dW)
            self.d2h(counts, dC)
            self.synchronize()
        finally:
            for p in d:
                self.dev_free(p)
        return loss, counts, fused, w

    def _relw_split(self, flat, names):
        out, off = {}, 0
        for name, size, shape in self._RELW_G:
            if name in names:
                out[name] = flat[off:off + size].reshape(shape).copy()
                off += size
        return out

    def relw_train_grads(self):
        """The last step's gradients {'W1','beta','gamma','w2','b2'} and its batch statistics {'mu','istd'} (sn_relw_train_grads)."""
        flat = np.empty(26301, np.float32)
        _lib.check(self._lib.sn_relw_train_grads(self._h, _lib.ptr(flat)))
        return self._relw_split(flat, ("W1", "beta", "gamma", "w2", "b2", "mu", "istd"))

    def relw_train_velocities(self):
        flat = np.empty(26101, np.float32)
        _lib.check(self._lib.sn_relw_train_velocities(self._h, _lib.ptr(flat)))
        return self._relw_split(flat, ("W1", "beta", "gamma", "w2", "b2"))

    def relw_train_dw(self, n, n_vp):
        """d loss / d w of the last step, which ran on n cubes of n_vp pairs (sn_relw_train_dw)."""
        out = np.empty((int(n), int(n_vp)), np.float32)
        _lib.check(self._lib.sn_relw_train_dw(self._h, _lib.ptr(out)))
        return out

    def relw_get_params(self):
        """The seven arrays of feature_fc1 / feature_linear1 in weight-file order (W, beta, gamma, mean, inv_std, W, b) as the device holds them."""
        flat = np.empty(26301, np.float32)
        _lib.check(self._lib.sn_relw_get_params(self._h, _lib.ptr(flat)))
        out, off = [], 0
        for size, shape in self._RELW_P:
            out.append(flat[off:off + size].reshape(shape).copy())
            off += size
        return out

    def dev_alloc(self, nbytes):
        p = self._lib.sn_dev_alloc(self._h, int(nbytes))
        if not p:
            raise _lib.SurfaceNetHipError("sn_dev_alloc failed: %s" % _lib.last_error())
        return p

    def dev_free(self, p):
        _lib.check(self._lib.sn_dev_free(self._h, p))

    def h2d(self, dst_dev, arr):
        arr = np.ascontiguousarray(arr)
        _lib.check(self._lib.sn_memcpy_h2d(self._h, dst_dev, _lib.ptr(arr), arr.nbytes))

    def d2h(self, arr, src_dev):
        assert arr.flags["C_CONTIGUOUS"]
        _lib.check(self._lib.sn_memcpy_d2h(self._h, _lib.ptr(arr), src_dev, arr.nbytes))

    def mark(self, slot):
        """Records point `slot` (0..7) on the context's stream for d2h_after."""
        _lib.check(self._lib.sn_mark(self._h, int(slot)))

    def d2h_after(self, slot, arr, src_dev):
        """d2h that waits only for the work enqueued BEFORE mark(slot), not for what was enqueued since."""
        assert arr.flags["C_CONTIGUOUS"]
        _lib.check(self._lib.sn_memcpy_d2h_after(self._h, int(slot), _lib.ptr(arr), src_dev, arr.nbytes))

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.dev_alloc(max(arr.nbytes, 16))
        self.h2d(p, arr)
        return p

    def cvc_forward_dev(self, n, n_vp, pairs_dev, xyz_dev, resol_dev, w_dev, fused_dev, unfused_dev=None, cvc_out_dev=None,
                        mean=MEAN_CVC_RGBRGB):
        m = np.ascontiguousarray(mean, dtype=np.float32).reshape(6)
        _lib.check(self._lib.sn_cvc_forward_dev(self._h, n, n_vp, pairs_dev, xyz_dev, resol_dev, _lib.ptr(m), w_dev, fused_dev,
                                                unfused_dev, cvc_out_dev))

    def color_fuse_dev(self, n, n_vp, cvc_dev, unfused_dev, w_dev, rgb_dev, mean=MEAN_CVC_RGBRGB):
        m = np.ascontiguousarray(mean, dtype=np.float32).reshape(6)
        _lib.check(self._lib.sn_color_fuse_dev(self._h, n, n_vp, cvc_dev, _lib.ptr(m), unfused_dev, w_dev, rgb_dev))

    def ray_pool_dev(self, n, n_vp, pairs_dev, xyz_dev, resol_dev, pred_dev, votes_dev, prediction_thresh=None):
        use = 0 if prediction_thresh is None else 1
        thr = 0.0 if prediction_thresh is None else float(np.float16(prediction_thresh))
        _lib.check(self._lib.sn_ray_pool_dev(self._h, n, n_vp, pairs_dev, xyz_dev, resol_dev, pred_dev, use, thr, votes_dev))

    def dense2sparse_dev(self, n, n_vp, pairs_dev, xyz_dev, resol_dev, pred_dev, rgb_dev, votes_ws_dev, offsets_dev, ijk_dev, pred16_dev,
                         rgb_out_dev, votes_out_dev, min_prob=0.5, rayPool_thresh=0, enable_centerCrop=False, cube_Dcenter=None,
                         enable_rayPooling=False):
        dc = int(cube_Dcenter) if enable_centerCrop else self.cube_D
        cfg = _lib.SparseCfg(float(np.float16(min_prob)), int(rayPool_thresh), int(bool(enable_centerCrop)), dc, int(bool(enable_rayPooling)))
        _lib.check(self._lib.sn_dense2sparse_dev(self._h, n, n_vp, pairs_dev, xyz_dev, resol_dev, pred_dev, rgb_dev, ctypes.byref(cfg),
                                                 votes_ws_dev, offsets_dev, ijk_dev, pred16_dev, rgb_out_dev, votes_out_dev))

    # ---- numerics of the 6-bit code planes (default mode) ---------------------------------------------------
    def calibrate(self, n_samples=0, max_sat_fraction=1e-3):
        """Data-driven premultipliers of the two code planes (sn_calibrate_dev): looks at the activations the LAST forward call left in the
        workspace (`n_samples` of them, 0 = all that call ran - run `forward` / `cvc_forward` on a representative batch first) and sets each plane's exponent to the
        largest one that saturates at most `max_sat_fraction` of the values. Returns a dict (exponents and saturated fractions before / after,
        largest magnitudes). The setting holds until the next load_param_values / precision change."""
        cal = _lib.Calibration()
        _lib.check(self._lib.sn_calibrate_dev(self._h, int(n_samples), float(max_sat_fraction), ctypes.byref(cal)))
        out = {k: getattr(cal, k) for k, _ in _lib.Calibration._fields_}
        if max_sat_fraction >= 0:                        # (a negative bound only measures)
            self._numerics["calibrated"], self._numerics["report"] = True, out
        return out

    def numeric_status(self):
        """Warning-level numeric status: names of the layers whose stored outputs exceeded the range of their 6-bit code plane since the last
        call (such a value loses its own correction term only; not an error). Clears the warning bits."""
        bits = ctypes.c_uint(0)
        names = ctypes.create_string_buffer(2048)
        _lib.check(self._lib.sn_numeric_status(self._h, ctypes.byref(bits), names, 2048))
        nm = [x for x in names.value.decode().split(",") if x]
        return [nm[i] if i < len(nm) else "layer %d" % i for i in range(32) if bits.value & (1 << i)]

    # ---- multi-GPU exchange (RCCL, native; torch.distributed is not required) ---------------------------
    @staticmethod
    def comm_unique_id():
        buf = ctypes.create_string_buffer(128)
        _lib.check(_lib.load().sn_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, world, rank, unique_id, timeout_s=None):
        """Joins the RCCL communicator (collective: every rank calls it with rank 0's unique id). timeout_s: bound on the wait for the other ranks
        (sn_comm_init_deadline: SurfaceNetHipError when it expires, the context stays usable without a communicator); None = wait for ever."""
        self.comm_world = self.comm_rank = 0
        _lib.check(self._lib.sn_comm_init_deadline(self._h, int(world), int(rank), ctypes.c_char_p(bytes(unique_id)), float(timeout_s or 0.0)))
        self.comm_world, self.comm_rank = int(world), int(rank)

    @staticmethod
    def comm_info():
        """-> (file the RCCL entry points are bound to [+ whether the process had it mapped already], ncclGetVersion code)."""
        buf, ver = ctypes.create_string_buffer(1024), ctypes.c_int(0)
        _lib.check(_lib.load().sn_comm_info(buf, 1024, ctypes.byref(ver)))
        return buf.value.decode("utf-8", "replace"), int(ver.value)

    def allgather_f32_dev(self, local_dev, n_local, global_dev):
        _lib.check(self._lib.sn_allgather_f32_dev(self._h, local_dev, int(n_local), global_dev))

    def allgather_f32_dev_overlap(self, local_dev, n_local, global_dev, slot):
        """The all-gather on the context's communication stream, behind the kernels submitted so far and overlapping the ones submitted next;
        `comm_wait(slot)` orders the kernel stream behind it again (before the two buffers are reused)."""
        _lib.check(self._lib.sn_allgather_f32_dev_overlap(self._h, local_dev, int(n_local), global_dev, int(slot)))

    def comm_wait(self, slot):
        _lib.check(self._lib.sn_comm_wait(self._h, int(slot)))

    def allgatherv_bytes(self, blob):
        """Variable-length all-gather of one byte string per rank through the library's RCCL binding: `blob` (np.uint8, any length incl. 0) -> list
        of `world` np.uint8 arrays in rank order. The payloads travel device to device over xGMI; only this rank's blob goes up and the gathered
        bytes come down. Collective sequence, identical on every rank whatever the blob sizes are (`allgatherv_two_step`): the counts
        (sn_allgatherv_counts), then counts + payloads into a buffer sized from them (sn_allgatherv_bytes_dev) - no rank ever retries on its own."""
        world = getattr(self, "comm_world", 0)
        if not world:
            raise _lib.SurfaceNetHipError("allgatherv_bytes: comm_init has not been called on this context")
        blob = np.ascontiguousarray(np.asarray(blob, dtype=np.uint8).reshape(-1))
        d_local = self.upload(blob) if blob.size else None

        def counts_fn(n_local):
            counts = (ctypes.c_ulonglong * world)()
            _lib.check(self._lib.sn_allgatherv_counts(self._h, int(n_local), counts))
            return [int(c) for c in counts]

        def payload_fn(n_local, total):
            counts = (ctypes.c_ulonglong * world)()
            try:
                d_all, alloc_err = self.dev_alloc(max(total, 16)), None
            except _lib.SurfaceNetHipError as e:
                # a rank that cannot hold the result must STILL run the call's collectives (its peers are entering them): with no destination the
                # library runs them all and reports "too small" afterwards; the allocation failure is raised then
                d_all, alloc_err = None, e
            try:
                rc = self._lib.sn_allgatherv_bytes_dev(self._h, d_local, int(n_local), d_all, int(total) if d_all else 0, counts)
                if alloc_err is not None:
                    raise alloc_err
                _lib.check(rc)
                out = np.empty((total,), dtype=np.uint8)
                if total:
                    self.d2h(out, d_all)
            finally:
                if d_all:
                    self.dev_free(d_all)
            return [int(c) for c in counts], out
        try:
            return allgatherv_two_step(int(blob.size), counts_fn, payload_fn)
        finally:
            if d_local is not None:
                self.dev_free(d_local)

    # ---- measurement --------------------------------------------------------------------------------
    def mfma_probe(self, target_ms=10.0):
        """What this box sustains on a pure fp16 MFMA stream (sn_mfma_probe) -> (dense fp16 TFLOP/s, shader clock in GHz)."""
        tf, ghz = ctypes.c_double(), ctypes.c_double()
        _lib.check(self._lib.sn_mfma_probe(self._h, float(target_ms), ctypes.byref(tf), ctypes.byref(ghz)))
        return tf.value, ghz.value

    def profile_enable(self, on=True):
        _lib.check(self._lib.sn_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        _lib.check(self._lib.sn_profile_reset(self._h))

    def profile(self):
        """-> {kernel tag: dict(ms, launches, flops, bytes)} accumulated since the last reset."""
        n = self._lib.sn_profile_count(self._h)
        if n < 0:
            _lib.check(n)
        out = {}
        name = ctypes.create_string_buffer(64)
        ms, fl, by = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        cnt = ctypes.c_int64()
        for i in range(n):
            _lib.check(self._lib.sn_profile_get(self._h, i, name, 64, ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(fl), ctypes.byref(by)))
            out[name.value.decode()] = dict(ms=ms.value, launches=cnt.value, flops=fl.value, bytes=by.value)
        return out
