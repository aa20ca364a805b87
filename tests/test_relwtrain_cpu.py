"""CPU: the numpy restatement of a training step of the view-pair weighting net (tests/relwtrain_ref.py) against torch float64 autograd and
a literal transcription of Lasagne's nesterov_momentum; the argument checks, the weight-file round trip and the C ABI of
surfacenet_amd.training. The GPU tests (tests/test_gpu_relwtrain.py) hold the library to this restatement."""
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

import relwtrain_ref as ref
from surfacenet_amd import weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 2, 8), (4, 5, 12), (40, 4, 8)]
NEW_SYMBOLS = ["sn_relw_train_begin", "sn_relw_train_end", "sn_relw_train_step", "sn_relw_train_step_dev", "sn_relw_train_grads",
               "sn_relw_train_velocities", "sn_relw_train_dw", "sn_relw_get_params"]


def _autograd(P, U, F, Y, c):
    """The step of DESIGN.md section 4.11 written with torch float64 ops; gradients by autograd."""
    import torch
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)
    n, n_vp = U.shape[:2]
    p = {k: t(P[k]).requires_grad_(k in ref.TRAINABLE) for k in P}
    Ut, Yt, Ft = t(U.reshape(n, n_vp, -1)), t(Y.reshape(n, 1, -1)), t(F)
    a = Ft @ p["W1"]
    mu = a.mean(0)
    var = ((a - mu) ** 2).mean(0)
    xh = (a - mu) / torch.sqrt(var + c["bn_eps"])
    h = torch.sigmoid(p["gamma"] * xh + p["beta"])
    z = (h @ p["w2"] + p["b2"]).reshape(n, n_vp)
    w = torch.softmax(z, dim=1)
    w.retain_grad()
    f = (w[:, :, None] * Ut).sum(1, keepdim=True)
    fc = torch.clamp(f, c["clip"], 1.0 - c["clip"])
    a1 = c["w_for_1"]
    loss = (-(a1 * Yt * torch.log(fc) + (1 - a1) * (1 - Yt) * torch.log(1 - fc))).mean()
    loss = loss + c["l2"] * ((p["W1"] ** 2).sum() + (p["w2"] ** 2).sum())
    loss.backward()
    out = {k: p[k].grad.numpy() for k in ref.TRAINABLE}
    out["dw"], out["loss"] = w.grad.numpy(), float(loss.detach())
    return out


@pytest.mark.parametrize("l2", [0.0, 1e-3])
@pytest.mark.parametrize("shape", SHAPES)
def test_fp64_restatement_equals_autograd(shape, l2):
    n, n_vp, s = shape
    U, F, Y = ref.make_inputs(n, n_vp, s, seed=7)
    P = ref.params_from_values(weights.synthetic_param_values(0), np.float64)
    c = ref.cfg(l2=l2)
    got, want = ref.step(P, U, F, Y, np.float64, c), _autograd(P, U, F, Y, c)
    assert abs(float(got["loss"]) - want["loss"]) <= 1e-13 * want["loss"]
    for k in ref.TRAINABLE + ("dw",):
        if k == "b2":
            continue
        scale = np.abs(want[k]).max()
        assert scale > 0 and np.abs(got[k].reshape(want[k].shape) - want[k]).max() <= 1e-10 * scale, k
    # db2 is zero in exact arithmetic (a softmax ignores a shift of its group): an absolute quantity
    bound = 1e-12 * np.abs(got["dz"]).sum()
    assert abs(float(got["b2"][0])) <= bound and abs(float(want["b2"][0])) <= bound


def test_gradient_is_zero_where_the_clamp_acts():
    n, n_vp, s = 2, 2, 4
    U, F, Y = ref.make_inputs(n, n_vp, s, seed=3)
    U[0, :, 0, 0, :2] = [0.0, 1.0]                        # f = 0 and f = 1 whatever the weights: clamped voxels
    P = ref.params_from_values(weights.synthetic_param_values(0), np.float64)
    got, want = ref.step(P, U, F, Y, np.float64, ref.cfg()), _autograd(P, U, F, Y, ref.cfg())
    assert np.isfinite(got["loss"]) and np.abs(got["dw"] - want["dw"]).max() <= 1e-10 * np.abs(want["dw"]).max()


def _lasagne_nesterov(params, grads, velocities, lr, momentum):
    """lasagne.updates.nesterov_momentum = apply_nesterov_momentum(sgd(...)), transcribed:
        updates[param] = param - learning_rate * grad                                   (sgd)
        x = momentum * velocity + updates[param] - param;  updates[velocity] = x;  updates[param] = momentum * x + updates[param]"""
    new_p, new_v = {}, {}
    for k in params:
        upd = params[k] - lr * grads[k]
        x = momentum * velocities[k] + upd - params[k]
        new_v[k] = x
        new_p[k] = momentum * x + upd
    return new_p, new_v


def test_nesterov_three_steps_equal_lasagnes_rule():
    n, n_vp, s = 3, 2, 8
    U, F, Y = ref.make_inputs(n, n_vp, s, seed=11)
    c = ref.cfg(lr=0.5)
    P = ref.params_from_values(weights.synthetic_param_values(0), np.float64)
    Vel = ref.zero_velocities(np.float64)
    Pl = {k: P[k].copy() for k in ref.TRAINABLE}
    Vl = {k: Vel[k].copy() for k in ref.TRAINABLE}
    for _ in range(3):
        G = ref.step(P, U, F, Y, np.float64, c)
        mean_before, istd_before = P["mean"], P["inv_std"]
        P, Vel = ref.update(P, Vel, G, np.float64, c)
        Pl, Vl = _lasagne_nesterov(Pl, {k: G[k] for k in ref.TRAINABLE}, Vl, c["lr"], c["momentum"])
        for k in ref.TRAINABLE:
            assert np.abs(P[k] - Pl[k]).max() <= 1e-14 * max(1.0, np.abs(Pl[k]).max()), k
            assert np.abs(Vel[k] - Vl[k]).max() <= 1e-14 * max(1.0, np.abs(Vl[k]).max()), k
            Pl[k] = P[k].copy()                           # (the next gradient is taken at the restatement's parameters)
        assert np.allclose(P["mean"], 0.9 * mean_before + 0.1 * G["mu"], rtol=1e-15, atol=0)
        assert np.allclose(P["inv_std"], 0.9 * istd_before + 0.1 * G["istd"], rtol=1e-15, atol=0)
    Ps, Vs = ref.update(P, Vel, G, np.float64, ref.cfg(lr=0.5, update="sgd"))
    assert all(np.array_equal(Ps[k], P[k] - 0.5 * G[k]) and np.array_equal(Vs[k], Vel[k]) for k in ref.TRAINABLE)


def test_learning_case_learns_in_the_restatement():
    """The figures of the end-to-end GPU test, from the restatement alone (float64): the loss falls at every step, to under a fifth."""
    U, F, Y, good = ref.make_learning_case()
    P = ref.params_from_values(weights.synthetic_param_values(0), np.float64)
    _, _, losses, out = ref.train(P, U, F, Y, np.float64, ref.cfg(lr=0.5), 30)
    assert all(b < a for a, b in zip(losses, losses[1:])) and losses[-1] <= 0.2 * losses[0]
    assert out["w"][np.arange(len(good)), good].mean() >= 0.9


# ---- the package --------------------------------------------------------------------------------------------------------------------------------
def test_training_type_errors_come_before_any_device_call():
    from surfacenet_amd import training
    values = weights.synthetic_param_values(0)
    with pytest.raises(TypeError):
        training.RelativeWeightTrainer(1, 0.1, param_values=values)                  # a single pair has nothing to train
    with pytest.raises(TypeError):
        training.RelativeWeightTrainer(17, 0.1, param_values=values)
    with pytest.raises(TypeError):
        training.RelativeWeightTrainer(2, 0.1)                                        # no weights
    with pytest.raises(TypeError):
        training.RelativeWeightTrainer(2, 0.1, param_values=values[:weights.N_NET_PARAMS])
    with pytest.raises(TypeError):
        training.RelativeWeightTrainer(2, 0.1, param_values=values, update_algorithm="adam")
    tr = training.RelativeWeightTrainer(2, 0.1, param_values=values)
    U, F, Y = ref.make_inputs(3, 2, 8, seed=1)
    X = np.zeros((6, 6, 8, 8, 8), np.float32)
    bad = [(U.astype(np.float64), F, Y), (U[0], F, Y), (U[:, :1], F, Y), (U[:, :, :, :, :4], F, Y), (U, F.astype(np.float64), Y), (U, F[:, :200], Y),
           (U, F[:4], Y), (U, F.reshape(-1), Y), (U, F, Y.astype(np.float64)), (U, F, Y[:, 0]), (U, F, Y[:2]), (U, F, np.zeros((3, 1, 4, 4, 4), np.float32)),
           (U.tolist(), F, Y)]
    for args in bad:
        with pytest.raises(TypeError):
            tr.step(*args)
    for args in [(X.astype(np.float64), F, Y), (X[:, :5], F, Y), (X[:5], F, Y), (X, F[:4], Y), (X, F, Y[:2])]:
        with pytest.raises(TypeError):
            tr.train_fn(*args)
    pinned = training.RelativeWeightTrainer(2, 0.1, input_cube_size=16, param_values=values)
    with pytest.raises(TypeError):
        pinned.step(U, F, Y)
    assert tr._ctx is None and pinned._ctx is None                                    # nothing reached the device


def test_save_round_trips_through_load_lasagne_pickle(tmp_path):
    from surfacenet_amd import training
    values = weights.synthetic_param_values(3)
    tr = training.RelativeWeightTrainer(3, 0.1, param_values=values)
    path = str(tmp_path / "refit.model")
    tr.save(path)
    back = weights.load_lasagne_pickle(path)
    assert len(back) == len(weights.PARAM_LAYOUT) == len(tr.param_values())
    assert all(a.dtype == np.float32 and np.array_equal(a, b) for a, b in zip(back, values))


def test_trainval_points_at_the_trainer():
    from surfacenet_amd import SurfaceNet
    with pytest.raises(NotImplementedError, match="training.SurfaceNet_fn_train"):
        SurfaceNet.SurfaceNet_fn_trainVal(2, return_train_fn=True)


def test_new_symbols_in_header_exports_binding_and_library():
    import __graft_entry__ as g
    g.build()
    from surfacenet_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "surfacenet_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sn_[a-z0-9_]+)\s*\(", hdr))
    assert "sn_relw_train_cfg" in hdr
    emap = open(os.path.join(ROOT, "surfacenet_amd", "csrc", "exports.map")).read()
    emap = re.sub(r"/\*.*?\*/", "", emap, flags=re.S)
    patterns = [p.strip() for p in re.search(r"global:(.*?);", emap, flags=re.S).group(1).split()]
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.ABI_SYMBOLS and name in exported and hasattr(lib, name), name
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), name
    assert lib.sn_version() == 2                          # symbols were added, none changed
    assert "sn_relwtrain.hip" in open(os.path.join(ROOT, "surfacenet_amd", "csrc", "Makefile")).read()
