"""Drop-in for the inference entry point of the reference's `nets/SurfaceNet.py`, executed on the MI355X.

`SurfaceNet_inference(N_viewPairs4inference, model_file, layerNameList_2_load)` (nets/SurfaceNet.py:385-402)
returns `(viewPair_relativeImpt_fn, nViewPair_SurfaceNet_fn)` with the calling conventions of the two compiled
Theano functions (nets/SurfaceNet.py:337-338, 365-382):
    viewPair_relativeImpt_fn(features (n*P,258) f32 [, n_samples_perGroup=P]) -> (n, P) f32 softmax weights
    nViewPair_SurfaceNet_fn(X [, w][, n_samples_perGroup])  -> [fused (n,1,s,s,s) f32, unfused (n,N_vp,s,s,s) f32]
X is float32 (n*N_vp, 6, s,s,s), mean-subtracted; w is float32 (n, N_vp). TypeError on dtype/ndim mismatch, as Theano.

Ground-truth mode: `SurfaceNet_inference(..., with_groundTruth=True)` is `__SurfaceNet_fn_inference__(with_groundTruth=True,
return_unfused_predict=True)` (nets/SurfaceNet.py:359-378):
    nViewPair_SurfaceNet_fn(X [, w], Y [, n_samples_perGroup]) -> [accuracy, fused, unfused]
and `SurfaceNet_fn_trainVal(..., return_train_fn=False)` gives the `val_fn` of nets/SurfaceNet.py:253-264:
    val_fn(X, similFeature, Y) -> [accuracy, fused]
Y is float32 (n, 1, s,s,s) (groundTruth.gt_cubes makes one from a point cloud); accuracy is `__weighted_accuracy__` (nets/SurfaceNet.py:203-224),
np.float64 (groundTruth.accuracy_from_counts).
"""
import numpy as np

from . import groundTruth, runtime, weights
from .context import NumericsGuard


def SurfaceNet_inference(N_viewPairs4inference, model_file, layerNameList_2_load=None, cube_D=None, param_values=None, auto_calibrate=True,
                         with_groundTruth=False):
    """model_file: the reference's `*.model` pickle. `param_values` (list of arrays in weight-file order) may be given
    instead, e.g. weights.synthetic_param_values(seed). cube_D = None (default): inferred from X.shape at every call of
    nViewPair_SurfaceNet_fn (the reference fixes it at compile time from params.__cube_D, params.py:65: 64, or 32), so the
    drop-in accepts whichever of the two the caller's params selects; an int pins it (any other X then raises TypeError).
    auto_calibrate (default on): after every call `nViewPair_SurfaceNet_fn` reads the library's saturation warning (context.NumericsGuard); the
    first time the loaded weights push stored activations past the range of the default mode's 6-bit code planes it derives the premultipliers
    from that batch, recomputes the batch and emits one RuntimeWarning with the layer names and the exponents chosen.
    with_groundTruth (default off: the callable is exactly the one described above): nViewPair_SurfaceNet_fn takes the target tensor Y after
    w (after X when N_viewPairs4inference == 1) - the argument order of nets/SurfaceNet.py:365-372 - and returns [accuracy, fused, unfused]. Y must
    be a float32 5-D array of shape (n, 1, s, s, s), TypeError otherwise. The accuracy is counted on the device from the fused tensor before that
    tensor is copied back; a batch redone after a recalibration is recounted."""
    values = param_values if param_values is not None else weights.load_lasagne_pickle(model_file)
    runtime.set_param_values(values)
    if cube_D is not None:
        runtime.prefer_cube_D(cube_D)
    N_vp = int(N_viewPairs4inference)
    guards = {}                                  # one NumericsGuard per context (cube size) this callable has run on

    def viewPair_relativeImpt_fn(similFeature, n_samples_perGroup=N_vp):
        f = np.asarray(similFeature)
        if f.dtype != np.float32 or f.ndim != 2:
            raise TypeError("similFeature must be a float32 matrix")
        ctx = runtime.any_context() if cube_D is None else runtime.context_for(cube_D, n_samples=1)
        return ctx.relative_weights(f, int(n_samples_perGroup))

    def nViewPair_SurfaceNet_fn(X, *args, **kwargs):
        n_per = int(kwargs.pop("n_samples_perGroup", N_vp))
        if kwargs:
            raise TypeError("unexpected keyword arguments %s" % sorted(kwargs))
        Y = None
        if with_groundTruth:
            # nets/SurfaceNet.py:365-372: [X, similWeight (N_vp >= 2)] + [Y] + [n_samples_perGroup (N_vp >= 2)]
            at = 0 if N_vp == 1 else 1
            if len(args) <= at:
                raise TypeError("expected (X, Y)" if N_vp == 1 else "expected (X, similWeight, Y[, n_samples_perGroup])")
            Y = args[at]
            args = args[:at] + args[at + 1:]
        if N_vp == 1:
            if len(args) > 0:
                raise TypeError("the N_viewPairs4inference == 1 function takes %s only (nets/SurfaceNet.py:354-357)" % ("X, Y" if with_groundTruth else "X"))
            w = None
            n_per = 1
        else:
            if len(args) < 1 or len(args) > 2:
                raise TypeError("expected (X, similWeight[, n_samples_perGroup])")
            w = args[0]
            if len(args) == 2:
                n_per = int(args[1])
        if not isinstance(X, np.ndarray) or X.dtype != np.float32 or X.ndim != 5:
            raise TypeError("X must be a float32 5-D ndarray")
        if X.shape[1] != 6 or X.shape[2] != X.shape[3] or X.shape[3] != X.shape[4]:
            raise TypeError("X must have shape (N*n_vp, 6, s, s, s), got %s" % (X.shape,))
        ctx = runtime.context_for(X.shape[2] if cube_D is None else cube_D, n_samples=X.shape[0])
        if with_groundTruth:
            if not isinstance(Y, np.ndarray) or Y.dtype != np.float32 or Y.ndim != 5:
                raise TypeError("Y must be a float32 5-D ndarray")
            run = lambda: ctx.forward_gt(X, w, Y, n_vp=n_per)
        else:
            run = lambda: ctx.forward(X, w, n_vp=n_per, return_unfused=True)
        out = run()
        guard = guards.get(id(ctx))
        if guard is None:
            guard = guards[id(ctx)] = NumericsGuard(ctx, enabled=auto_calibrate)
        if guard.check("nViewPair_SurfaceNet_fn") is not None:
            out = run()                # premultipliers recalibrated on this batch: redo it (in ground-truth mode it is recounted too)
            ctx.numeric_status()       # (clears what the calibration's own tolerance leaves)
        fused, unfused = out[0], out[1]
        res = [fused, fused] if N_vp == 1 else [fused, unfused]      # one tensor twice in the reference when N_vp == 1 (SurfaceNet.py:355-357)
        if with_groundTruth:
            res.insert(0, groundTruth.accuracy_from_counts(out[2]))
        return res

    viewPair_relativeImpt_fn.sn_gpu = True     # lets viewPairSelection.viewPairSelection skip the (N*P, 258) feature matrix
    viewPair_relativeImpt_fn.sn_cube_D = cube_D
    return viewPair_relativeImpt_fn, nViewPair_SurfaceNet_fn


def SurfaceNet_fn_trainVal(N_viewPairs4inference, default_lr=None, input_cube_size=None, D_viewPairFeature=None, num_hidden_units=None,
                           CHANNEL_MEAN=None, return_train_fn=False, return_val_fn=True, with_weight=True, param_values=None, model_file=None,
                           auto_calibrate=True):
    """The validation half of the reference's SurfaceNet_fn_trainVal (nets/SurfaceNet.py:227-294): returns (None, None, val_fn) - the
    reference returns (net, train_fn, val_fn); there is no Lasagne net here, and the train_fn is training.SurfaceNet_fn_train's (return_train_fn=True
    raises NotImplementedError and says so).
        val_fn(X, similFeature, Y) -> [accuracy, fused]          (with_weight; nets/SurfaceNet.py:260-264)
        val_fn(X, Y)               -> [accuracy, fused]          (with_weight=False and one view pair)
    similFeature is the float32 (n*N_vp, 258) matrix of viewPair_relativeImpt_fn: the weights are relative_weights(similFeature), then the
    forward pass, then the count - `SurfaceNet_inference(with_groundTruth=True)` fed with those weights. with_weight=False with N_vp >= 2 is the
    reference's ChannelPool_max fusion, which is not built. input_cube_size pins the cube size (None: taken from X); default_lr,
    D_viewPairFeature, num_hidden_units and CHANNEL_MEAN are accepted for the reference's signature and not used (the weight file fixes the
    layer sizes; X comes mean-subtracted). Weights: param_values (list in weight-file order) or model_file."""
    if return_train_fn:
        raise NotImplementedError("SurfaceNet_fn_trainVal builds the val_fn only; the view-pair weighting net is trained, with SurfaceNet frozen, by "
                                  "training.SurfaceNet_fn_train")
    if not return_val_fn:
        return None, None, None
    N_vp = int(N_viewPairs4inference)
    if not with_weight and N_vp > 1:
        raise NotImplementedError("with_weight=False fuses N_vp >= 2 pairs with ChannelPool_max, which is not built")
    if param_values is None and model_file is None:
        raise TypeError("SurfaceNet_fn_trainVal needs param_values or model_file")
    relw_fn, net_fn = SurfaceNet_inference(N_vp, model_file, cube_D=input_cube_size, param_values=param_values, auto_calibrate=auto_calibrate,
                                           with_groundTruth=True)

    def val_fn(X, *args):
        if N_vp == 1:
            if len(args) != (2 if with_weight else 1):
                raise TypeError("expected (X, similFeature, Y)" if with_weight else "expected (X, Y)")
            acc, fused, _ = net_fn(X, args[-1])          # one pair: its weight is 1 whatever the features say
            return [acc, fused]
        if len(args) != 2:
            raise TypeError("expected (X, similFeature, Y)")
        acc, fused, _ = net_fn(X, relw_fn(args[0]), args[1])
        return [acc, fused]

    return None, None, val_fn
