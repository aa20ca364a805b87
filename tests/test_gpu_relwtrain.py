"""GPU (-m gpu): one training step of the view-pair weighting net with SurfaceNet frozen (surfacenet_amd/csrc/relwtrain.h)
against the numpy restatement (tests/relwtrain_ref.py) in float64, with the float32 restatement as the measure of what the number format costs:
fusion and update bit for bit, loss / dw / gradients within summation bounds, determinism, the refreshed inference weights, train_fn against
step, the error codes, and thirty steps that learn which view pair to trust.

Measured on an MI355X (err_dev / e32 per array, worst over the five shapes; loss trajectory ratio): see profiles/relwtrain/README.md."""
import ctypes
import functools
import math

import numpy as np
import pytest

import relwtrain_ref as ref

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
# (n, N_vp, s, device pointers of U / Y / fused offset by 4 bytes)
SHAPES = [(3, 2, 8, False),      # R = 6, below any workgroup size
          (4, 5, 12, False),     # V = 1728: a partial last chunk
          (40, 4, 8, False),     # R = 160: more rows than one workgroup
          (2, 3, 8, True),       # unaligned tensors: the scalar path of the voxel pass
          (2, 2, 16, False)]     # V = 4096: two chunks per cube, added in order
GRAD_KEYS = ("W1", "beta", "gamma", "w2", "mu", "istd")


@functools.lru_cache(maxsize=None)
def _values():
    from surfacenet_amd import weights
    return weights.synthetic_param_values(0)


class _Ctxs(object):
    """One context per cube size; `session` reloads the weights first when an earlier session of that context has updated them."""

    def __init__(self):
        self.made, self.dirty = {}, {}

    def get(self, s):
        import surfacenet_amd
        if s not in self.made:
            self.made[s] = surfacenet_amd.Context(cube_D=s, max_samples=8)
            self.made[s].load_param_values(_values())
            self.dirty[s] = False
        return self.made[s]

    def session(self, s, **kw):
        ctx = self.get(s)
        if self.dirty[s]:
            ctx.load_param_values(_values())
        ctx.relw_train_begin(kw.pop("lr", 0.1), update=kw.pop("update", "none"), **kw)
        self.dirty[s] = True
        return ctx

    def clean(self, s):
        self.dirty[s] = False                             # (the session that just ran changed nothing: update = 'none')


@pytest.fixture(scope="module")
def ctxs(gpu_required):
    c = _Ctxs()
    yield c
    for ctx in c.made.values():
        ctx.close()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs and the two restatements of a shape at the synthetic weights, computed once."""
    n, n_vp, s, _ = shape
    U, F, Y = ref.make_inputs(n, n_vp, s, seed=100 + n * n_vp + s)
    c = ref.cfg()
    r64 = ref.step(ref.params_from_values(_values(), np.float64), U, F, Y, np.float64, c)
    r32 = ref.step(ref.params_from_values(_values(), np.float32), U, F, Y, np.float32, c)
    return U, F, Y, r64, r32


def _device_step(ctx, U, F, Y, offset):
    """A step through the device form, the tensors at 4 bytes past an allocation when `offset`. -> (loss, counts, fused, w)"""
    n, n_vp, s = U.shape[0], U.shape[1], U.shape[2]
    o = 4 if offset else 0
    bufs = [ctx.dev_alloc(a.nbytes + 16) for a in (U, F, Y)] + [ctx.dev_alloc(Y.nbytes + 16), ctx.dev_alloc(n * n_vp * 4), ctx.dev_alloc(n * 32)]
    dU, dF, dY, dfu, dw, dc = bufs
    try:
        ctx.h2d(dU + o, U)
        ctx.h2d(dF, F)
        ctx.h2d(dY + o, Y)
        loss = ctx.relw_train_step_dev(n, n_vp, dU + o, dF, dY + o, dfu + o, dw, dc, want_loss=True)
        fused, w, counts = np.empty((n, 1, s, s, s), np.float32), np.empty((n, n_vp), np.float32), np.zeros((n, 4), np.int64)
        ctx.d2h(fused, dfu + o)
        ctx.d2h(w, dw)
        ctx.d2h(counts, dc)
        ctx.synchronize()
    finally:
        for p in bufs:
            ctx.dev_free(p)
    return loss, counts, fused, w


def _err(a, b):
    return float(np.abs(np.asarray(a, np.float64).reshape(-1) - np.asarray(b, np.float64).reshape(-1)).max())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda sh: "n%d_vp%d_s%d%s" % (sh[0], sh[1], sh[2], "_unaligned" if sh[3] else ""))
def test_step_against_the_restatement(ctxs, shape):
    n, n_vp, s, offset = shape
    U, F, Y, r64, r32 = _case(shape)
    V = s ** 3
    ctx = ctxs.session(s, update="none")
    if offset:
        loss, counts, fused, w = _device_step(ctx, U, F, Y, True)
    else:
        loss, counts, fused, w = ctx.relw_train_step(U, F, Y, n_vp)
    G, dw = ctx.relw_train_grads(), ctx.relw_train_dw(n, n_vp)
    relw = ctx.relative_weights(F, n_vp)
    ctx.relw_train_end()
    ctxs.clean(s)
    # 1. the fusion, bit for bit, from the device's own weights
    assert np.array_equal(fused.reshape(n, V), ref.fuse(w, U, np.float32))
    import gtcubes_ref
    assert np.array_equal(counts, gtcubes_ref.accuracy_counts(fused, np.asarray(Y), 0.5))
    # 2. batch statistics, not the running ones; the float64 restatement's weights
    assert np.abs(w - relw).max() > 1e-4
    e32 = _err(r32["w"], r64["w"])
    print("%s w: err_dev %.3e e32 %.3e" % (shape, _err(w, r64["w"]), e32))
    assert _err(w, r64["w"]) <= 16 * max(e32, 2.0 ** -22 * np.abs(r64["w"]).max())
    # 3. the loss: a mean of n V non-negative terms
    L64 = float(r64["loss"])
    print("%s loss: dev %.9g f64 %.9g |diff| / bound %.3f" % (shape, loss, L64, abs(loss - L64) / (4 * EPS * (math.log2(n * V) + 4) * L64)))
    assert abs(loss - L64) <= 4 * EPS * (math.log2(n * V) + 4) * L64
    # 4. dw: the tree-summation bound, two roundings per term
    bound = 8 * EPS * math.log2(V) * r64["abs_gU"]
    print("%s dw: worst |diff| / bound %.3f" % (shape, float((np.abs(dw - r64["dw"]) / bound).max())))
    assert (np.abs(dw - r64["dw"]) <= bound).all()
    # 5. gradients and batch statistics against float64, by what float32 numpy loses on the same inputs
    for k in GRAD_KEYS:
        e32, scale = _err(r32[k], r64[k]), float(np.abs(r64[k]).max())
        err = _err(G[k], r64[k])
        print("%s %s: err_dev %.3e e32 %.3e ratio %.2f (e32 / max %.1e)" % (shape, k, err, e32, err / e32 if e32 else float("inf"), e32 / scale))
        assert err <= 16 * max(e32, 2.0 ** -22 * scale), k
    assert abs(float(G["b2"][0])) <= 16 * EPS * float(np.abs(r64["dz"]).sum())


def _as_ref_params(plist):
    return ref.params_from_values(plist, np.float32)


def test_update_is_the_restatements_bit_for_bit(ctxs):
    """Two Nesterov steps (the second with non-zero velocities) and one sgd step: parameters, velocities and running statistics equal the float32
    restatement's update applied to the gradients the device reports."""
    shape = SHAPES[0]
    n, n_vp, s, _ = shape
    U, F, Y = _case(shape)[:3]
    for update, steps in (("nesterov_momentum", 2), ("sgd", 1)):
        c = ref.cfg(lr=0.5, update=update)
        ctx = ctxs.session(s, lr=0.5, update=update)
        P, Vel = _as_ref_params(ctx.relw_get_params()), ref.zero_velocities(np.float32)
        assert all(np.array_equal(a, np.asarray(b).reshape(a.shape)) for a, b in zip(ctx.relw_get_params(), _values()[-7:]))
        for _ in range(steps):
            ctx.relw_train_step(U, F, Y, n_vp)
            P, Vel = ref.update(P, Vel, ctx.relw_train_grads(), np.float32, c)
            got, vel = _as_ref_params(ctx.relw_get_params()), ctx.relw_train_velocities()
            for k in P:
                assert np.array_equal(got[k], P[k]), (update, k)
            for k in ref.TRAINABLE:
                assert np.array_equal(vel[k].reshape(Vel[k].shape), Vel[k]), (update, k)
        assert update == "sgd" or np.abs(Vel["W1"]).max() > 0
        last = ctx.relw_get_params()
        ctx.relw_train_end()
        assert all(np.array_equal(a, b) for a, b in zip(ctx.relw_get_params(), last))      # the closed session's weights stay


def test_same_start_gives_the_same_bits(ctxs):
    shape = SHAPES[2]
    n, n_vp, s, _ = shape
    U, F, Y = _case(shape)[:3]
    runs = []
    for _ in range(2):
        ctx = ctxs.session(s, lr=0.5, update="nesterov_momentum")
        losses = [ctx.relw_train_step(U, F, Y, n_vp)[0] for _ in range(2)]
        runs.append((losses, ctx.relw_train_dw(n, n_vp), ctx.relw_get_params(), ctx.relw_train_grads()))
        ctx.relw_train_end()
    (l0, dw0, p0, g0), (l1, dw1, p1, g1) = runs
    assert l0 == l1 and dw0.tobytes() == dw1.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(p0, p1)) and all(g0[k].tobytes() == g1[k].tobytes() for k in g0)


def test_error_codes_and_a_valid_call_afterwards(ctxs):
    from surfacenet_amd import _lib
    shape = SHAPES[0]
    n, n_vp, s, _ = shape
    U, F, Y = [np.ascontiguousarray(a) for a in _case(shape)[:3]]
    ctx = ctxs.get(s)
    lib, h, P = ctx._lib, ctx._h, _lib.ptr
    ARG, STATE = -1, -2
    loss = ctypes.c_double(0)
    step = lambda n_, vp_, u, f, y: lib.sn_relw_train_step(h, n_, vp_, u, f, y, None, None, None, ctypes.byref(loss))
    out = np.zeros(26301, np.float32)
    if ctxs.dirty[s]:
        ctx.load_param_values(_values())
        ctxs.dirty[s] = False
    assert step(n, n_vp, P(U), P(F), P(Y)) == STATE                       # before sn_relw_train_begin
    assert lib.sn_relw_train_grads(h, P(out)) == STATE and lib.sn_relw_train_dw(h, P(out)) == STATE and lib.sn_relw_train_end(h) == STATE
    assert lib.sn_relw_train_begin(h, None) == ARG and lib.sn_relw_train_begin(None, ctypes.byref(_lib.RelwTrainCfg())) == ARG
    ctx.relw_train_begin(0.1, update="none")
    assert lib.sn_relw_train_grads(h, P(out)) == STATE                   # no step yet
    for bad_vp in (1, 0, 17):
        assert step(n, bad_vp, P(U), P(F), P(Y)) == ARG
    assert step(0, n_vp, P(U), P(F), P(Y)) == ARG and step(-1, n_vp, P(U), P(F), P(Y)) == ARG          # R < 2
    assert step(n, n_vp, None, P(F), P(Y)) == ARG and step(n, n_vp, P(U), None, P(Y)) == ARG and step(n, n_vp, P(U), P(F), None) == ARG
    assert lib.sn_relw_train_step_dev(h, n, n_vp, None, None, None, None, None, None, None) == ARG
    assert lib.sn_relw_train_grads(h, None) == ARG and lib.sn_relw_get_params(h, None) == ARG
    got = ctx.relw_train_step(U, F, Y, n_vp)                             # a valid call still works
    assert abs(got[0] - float(_case(shape)[3]["loss"])) < 1e-5
    assert step(n, n_vp, P(U), P(F), P(Y)) == 0 and loss.value == got[0]  # all optional results left out
    ctx.relw_train_end()
    import surfacenet_amd
    with surfacenet_amd.Context(cube_D=8, max_samples=2) as c98:
        c98.load_param_values(_values()[:98])
        with pytest.raises(surfacenet_amd.SurfaceNetHipError, match="status -2"):
            c98.relw_train_begin(0.1)


@pytest.fixture()
def fresh_runtime(gpu_required):
    from surfacenet_amd import runtime
    runtime.reset()
    yield runtime
    runtime.reset()


def test_trained_weights_reach_the_inference_entries_and_train_fn_equals_step(fresh_runtime):
    from oracle import net_oracle
    from surfacenet_amd import training
    n, n_vp, s = 3, 2, 8
    U, F, Y = _case(SHAPES[0])[:3]
    rs = np.random.RandomState(5)
    X = (rs.randn(n * n_vp, 6, s, s, s) * 60).astype(np.float32)
    # train_fn(X, F, Y) == step(unfused(X), F, Y), bit for bit (update 'none': both see the same parameters)
    tr, train_fn, val_fn = training.SurfaceNet_fn_train(n_vp, 0.5, input_cube_size=s, param_values=_values(), update_algorithm="none",
                                                           auto_calibrate=False)
    a = train_fn(X, F, Y)
    ctx = fresh_runtime.context_for(s)
    unfused = ctx.forward(X, np.full((n, n_vp), 0.5, np.float32), n_vp=n_vp)[1]
    b = tr.step(unfused, F, Y)
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert np.array_equal(a[2].reshape(n, -1), ref.fuse(a[3], unfused, np.float32))
    tr.close()
    # after a Nesterov step the inference MLP runs on the trained weights, running statistics included
    tr, train_fn, val_fn = training.SurfaceNet_fn_train(n_vp, 0.5, input_cube_size=s, param_values=_values(), auto_calibrate=False)
    before = net_oracle.relative_weights(F, _values(), n_vp)
    tr.step(U, F, Y)
    trained = tr.param_values()
    assert len(trained) == 105 and all(np.array_equal(x, y) for x, y in zip(trained[:98], _values()[:98]))
    assert all(not np.array_equal(x, y) for x, y in zip(trained[98:104], _values()[98:104]))      # (db2 is zero up to rounding: b2 may stay)
    got, want = tr.viewPair_relativeImpt_fn(F), net_oracle.relative_weights(F, trained, n_vp)
    assert np.abs(got - want).max() < 1e-5 and np.abs(got - before).max() > 1e-3
    acc, fused = val_fn(X, F, Y)                          # the val_fn made with the trainer fuses with those weights
    assert np.abs(fused.reshape(n, -1) - ref.fuse(got, unfused, np.float32)).max() < 1e-6
    tr.close()
    assert np.abs(ctx.relative_weights(F, n_vp) - want).max() < 1e-5      # they stay in force after the session


def test_thirty_steps_learn_which_pair_to_trust(fresh_runtime):
    from surfacenet_amd import training
    U, F, Y, good = ref.make_learning_case()
    c = ref.cfg(lr=0.5)
    l64 = ref.train(ref.params_from_values(_values(), np.float64), U, F, Y, np.float64, c, 30)[2]
    l32 = ref.train(ref.params_from_values(_values(), np.float32), U, F, Y, np.float32, c, 30)[2]
    tr = training.RelativeWeightTrainer(U.shape[1], 0.5, input_cube_size=U.shape[2], param_values=_values())
    losses, w = [], None
    for _ in range(30):
        loss, acc, fused, w = tr.step(U, F, Y)
        losses.append(float(loss))
    tr.close()
    ratios = [abs(a - b) / max(16 * abs(x - b), 1e-5 * b) for a, b, x in zip(losses, l64, l32)]
    print("loss %.4f -> %.4f (step 10) -> %.4f; good-pair weight mean %.3f min %.3f; worst |L_dev - L_64| / bound %.3f"
          % (losses[0], losses[10], losses[-1], w[np.arange(len(good)), good].mean(), w[np.arange(len(good)), good].min(), max(ratios)))
    assert losses[-1] <= 0.2 * losses[0]
    assert w[np.arange(len(good)), good].mean() >= 0.9
    assert max(ratios) <= 1.0
