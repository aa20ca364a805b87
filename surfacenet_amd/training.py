"""Training the view-pair weighting net on the MI355X with SurfaceNet frozen: the second regime of the reference's `SurfaceNet_fn_trainVal`
("train the softmaxWeight with(out) finetuning the SurfaceNet", nets/SurfaceNet.py:266-294), i.e. refitting the 258 -> 100 -> 1 MLP of
`__relativeWeight_net__` (nets/SurfaceNet.py:84-100) on a new dataset's cubes. DESIGN.md section 4.11 states the step.

    trainer, train_fn, val_fn = SurfaceNet_fn_train(N_viewPairs4inference, default_lr, param_values=values)
    loss, acc, fused, w = train_fn(X, similFeature, Y)           # the reference's argument order (nets/SurfaceNet.py:288-293)
    loss, acc, fused, w = trainer.step(unfused, similFeature, Y) # on predictions computed once: many epochs over one cache
    trainer.save("refit.model")                                  # a pickle weights.load_lasagne_pickle reads back

Seven arrays are trained: feature_fc1.W / beta / gamma and feature_linear1.W / b by the optimiser, feature_fc1.mean / inv_std as running
statistics. The 3-D network runs exactly as in inference (BN folded). Three deliberate differences from the reference's (non-working) train_fn:
the loss comes back as its scalar mean (the reference returns the per-voxel tensor), the frozen net does not switch to batch statistics,
and the fused tensor is not divided by the sum of the softmax weights (it is 1). tests/relwtrain_ref.py restates the step in numpy."""
import pickle

import numpy as np

from . import groundTruth, runtime, weights
from .context import RELW_MAX_VP, check_train_args

UPDATE_ALGORITHMS = ("nesterov_momentum", "sgd", "none")
_FIRST = weights.N_NET_PARAMS          # index of feature_fc1.W in weights.PARAM_LAYOUT


class RelativeWeightTrainer(object):
    """A training session of the relative-weight MLP in the context of one cube size. While it is open the context's inference entries
    (viewPair_relativeImpt_fn, val_fn) see the weights as trained so far, in deterministic mode (running statistics)."""

    def __init__(self, N_viewPairs4inference, default_lr, input_cube_size=None, param_values=None, model_file=None, momentum=0.9,
                 update_algorithm="nesterov_momentum", w_for_1=0.96, l2=0.0):
        N_vp = int(N_viewPairs4inference)
        if not 2 <= N_vp <= RELW_MAX_VP:
            raise TypeError("training needs 2 <= N_viewPairs4inference <= %d (the relative weight of a single view pair is 1), got %d" % (RELW_MAX_VP, N_vp))
        if update_algorithm not in UPDATE_ALGORITHMS:
            raise TypeError("update_algorithm must be one of %s" % (UPDATE_ALGORITHMS,))
        if param_values is None and model_file is None:
            raise TypeError("RelativeWeightTrainer needs param_values or model_file")
        values = list(param_values) if param_values is not None else weights.load_lasagne_pickle(model_file)
        if len(values) != len(weights.PARAM_LAYOUT):
            raise TypeError("training needs all %d arrays (the %d network arrays + the relative-weight MLP), got %d"
                            % (len(weights.PARAM_LAYOUT), weights.N_NET_PARAMS, len(values)))
        weights.validate(values)
        self.N_vp, self.lr, self.momentum, self.update_algorithm = N_vp, float(default_lr), float(momentum), update_algorithm
        self.w_for_1, self.l2 = float(w_for_1), float(l2)
        self.cube_D = None if input_cube_size is None else int(input_cube_size)
        self._values = values
        self._ctx = None

    # ---- the session ---------------------------------------------------------------------------------------------------------------------
    def _context(self, s):
        """The context of cube size s with the session open in it (opened at the first step, from the weights given to the trainer)."""
        if self.cube_D is not None and int(s) != self.cube_D:
            raise TypeError("the trainer is pinned to cubes of %d^3, got %d^3" % (self.cube_D, s))
        if self._ctx is not None:
            if self._ctx.cube_D != int(s):
                raise TypeError("the session runs on cubes of %d^3, got %d^3" % (self._ctx.cube_D, s))
            return self._ctx
        runtime.set_param_values(self._values)
        ctx = runtime.context_for(int(s))
        ctx.relw_train_begin(self.lr, self.momentum, self.update_algorithm, self.w_for_1, self.l2)
        self._ctx = ctx
        return ctx

    def close(self):
        if self._ctx is not None:
            self._values = self.param_values()
            self._ctx.relw_train_end()
            self._ctx = None

    @staticmethod
    def _cube_size(a):
        if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim != 5:
            raise TypeError("the first argument must be a float32 5-D ndarray")
        if a.shape[2] != a.shape[3] or a.shape[3] != a.shape[4]:
            raise TypeError("the first argument must end in (s, s, s), got %s" % (a.shape,))
        return a.shape[2]

    def _precheck(self, first, similFeature, Y, first_is_X):
        """forward_gt's dtype / ndim / shape rules, applied before a context exists: no device call is made for a bad argument."""
        s = self._cube_size(first)
        if self.cube_D is not None and s != self.cube_D:
            raise TypeError("the trainer is pinned to cubes of %d^3, got %d^3" % (self.cube_D, s))
        check_train_args(s, first, similFeature, Y, self.N_vp, first_is_X)
        return s

    @staticmethod
    def _result(out):
        loss, counts, fused, w = out
        return [np.float64(loss), groundTruth.accuracy_from_counts(counts), fused, w]

    def step(self, unfused, similFeature, Y):
        """One step on cached predictions: unfused (n,N_vp,s,s,s), similFeature (n*N_vp,258), Y (n,1,s,s,s), float32.
        -> [loss (np.float64 scalar), accuracy (__weighted_accuracy__ of fused against Y), fused (n,1,s,s,s), softmaxWeights (n,N_vp)]."""
        s = self._precheck(unfused, similFeature, Y, False)
        return self._result(self._context(s).relw_train_step(unfused, similFeature, Y, self.N_vp))

    def train_fn(self, X, similFeature, Y):
        """The reference's train_fn(X, similFeature, Y) (nets/SurfaceNet.py:288-293): X (n*N_vp,6,s,s,s) float32, mean-subtracted. The frozen
        SurfaceNet runs on the device and its unfused predictions feed the step without coming back. Same results as `step`."""
        s = self._precheck(X, similFeature, Y, True)
        return self._result(self._context(s).relw_train_fn(X, similFeature, Y, self.N_vp))

    def viewPair_relativeImpt_fn(self, similFeature, n_samples_perGroup=None):
        """The inference MLP (running statistics) with the weights as trained so far: SurfaceNet_inference's viewPair_relativeImpt_fn in the
        session's context. -> (n, n_samples_perGroup) float32 softmax weights."""
        f = np.asarray(similFeature)
        if f.dtype != np.float32 or f.ndim != 2:
            raise TypeError("similFeature must be a float32 matrix")
        if self._ctx is None:
            raise RuntimeError("no step has run: the weights are the ones the trainer was given")
        return self._ctx.relative_weights(f, int(self.N_vp if n_samples_perGroup is None else n_samples_perGroup))

    # ---- state -----------------------------------------------------------------------------------------------------------------------------
    def gradients(self):
        """The last step's gradients {'W1','beta','gamma','w2','b2'} and batch statistics {'mu','istd'}."""
        if self._ctx is None:
            raise RuntimeError("no step has run")
        return self._ctx.relw_train_grads()

    def param_values(self):
        """The full list in weights.PARAM_LAYOUT order with the seven arrays of the MLP replaced by the trained ones."""
        if self._ctx is None:
            return list(self._values)
        return list(self._values[:_FIRST]) + self._ctx.relw_get_params()

    def save(self, path):
        """Writes the list of `param_values()` as a pickle (protocol 2: what a Python-2 reader of the reference's `*.model` files and
        weights.load_lasagne_pickle both read)."""
        values = [np.ascontiguousarray(v, dtype=np.float32) for v in self.param_values()]
        with open(path, "wb") as f:
            pickle.dump(values, f, protocol=2)


def SurfaceNet_fn_train(N_viewPairs4inference, default_lr, input_cube_size=None, param_values=None, model_file=None, momentum=0.9,
                        update_algorithm="nesterov_momentum", w_for_1=0.96, l2=0.0, auto_calibrate=True):
    """-> (trainer, train_fn, val_fn): the shape of the reference's (net, train_fn, val_fn) (nets/SurfaceNet.py:294).
        train_fn(X, similFeature, Y) -> [loss, accuracy, fused, softmaxWeights]
        val_fn(X, similFeature, Y)   -> [accuracy, fused]         (SurfaceNet.SurfaceNet_fn_trainVal's, in deterministic mode)
    val_fn sees the weights as trained so far."""
    from . import SurfaceNet
    trainer = RelativeWeightTrainer(N_viewPairs4inference, default_lr, input_cube_size=input_cube_size, param_values=param_values,
                                    model_file=model_file, momentum=momentum, update_algorithm=update_algorithm, w_for_1=w_for_1, l2=l2)
    _, _, val_fn = SurfaceNet.SurfaceNet_fn_trainVal(trainer.N_vp, default_lr, input_cube_size=input_cube_size, return_val_fn=True,
                                                     param_values=trainer._values, auto_calibrate=auto_calibrate)
    return trainer, trainer.train_fn, val_fn
