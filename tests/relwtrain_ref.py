"""Numpy restatement of one training step of the view-pair weighting net with SurfaceNet frozen (surfacenet_amd/csrc/
relwtrain.h), with the dtype as a parameter: float64 is the reference of the tests, float32 shows what the number format alone costs. Forward in
training mode, closed-form backward, the sgd / Nesterov update and the running statistics. Nothing here is used by the product."""
import numpy as np

D, H = 258, 100
TRAINABLE = ("W1", "beta", "gamma", "w2", "b2")
DEFAULT_CFG = dict(lr=0.1, momentum=0.9, w_for_1=0.96, l2=0.0, bn_alpha=0.1, bn_eps=1e-4, clip=1e-7, update="nesterov_momentum")


def cfg(**kw):
    c = dict(DEFAULT_CFG)
    c.update(kw)
    return c


def params_from_values(values, dtype):
    """The seven arrays at the end of a weight list (weights.PARAM_LAYOUT order) as the dict the restatement works on."""
    W1, beta, gamma, mean, inv_std, w2, b2 = [np.asarray(v) for v in values[-7:]]
    return dict(W1=W1.astype(dtype), beta=beta.astype(dtype), gamma=gamma.astype(dtype), mean=mean.astype(dtype), inv_std=inv_std.astype(dtype),
                w2=w2.reshape(H).astype(dtype), b2=b2.reshape(1).astype(dtype))


def zero_velocities(dtype):
    return dict(W1=np.zeros((D, H), dtype), beta=np.zeros(H, dtype), gamma=np.zeros(H, dtype), w2=np.zeros(H, dtype), b2=np.zeros(1, dtype))


def make_inputs(n, n_vp, s, seed):
    """U uniform in (0.02, 0.98) - the clamp never acts -, Y Bernoulli(0.1), F: two unit-norm 128-vectors and two values in (0, 1) per row."""
    rs = np.random.RandomState(seed)
    U = rs.uniform(0.02, 0.98, (n, n_vp, s, s, s)).astype(np.float32)
    Y = (rs.uniform(size=(n, 1, s, s, s)) < 0.1).astype(np.float32)
    F = np.empty((n * n_vp, D), np.float32)
    for half in (0, 1):
        e = rs.randn(n * n_vp, 128)
        F[:, 128 * half:128 * (half + 1)] = e / np.linalg.norm(e, axis=1, keepdims=True)
    F[:, 256:] = rs.uniform(0.0, 1.0, (n * n_vp, 2))
    return U, F, Y


def make_learning_case(seed=0, n=16, n_vp=4, s=8):
    """One informative pair per cube (a noisy copy of Y, small F[:,256]) among uninformative ones (uniform noise, large F[:,256])."""
    rs = np.random.RandomState(seed)
    Y = (rs.uniform(size=(n, 1, s, s, s)) < 0.08).astype(np.float32)
    U = rs.uniform(0.02, 0.6, (n, n_vp, s, s, s)).astype(np.float32)
    _, F, _ = make_inputs(n, n_vp, s, seed + 1)
    F = F.reshape(n, n_vp, D)
    F[:, :, 256] = rs.uniform(0.5, 1.0, (n, n_vp))
    good = rs.randint(0, n_vp, n)
    for c in range(n):
        U[c, good[c]] = np.clip(0.9 * Y[c, 0] + 0.05 + rs.normal(0.0, 0.02, (s, s, s)), 0.01, 0.99)
        F[c, good[c], 256] = rs.uniform(0.0, 0.2)
    return U, np.ascontiguousarray(F.reshape(n * n_vp, D)), Y, good


def fuse(w, U, dtype=np.float32):
    """f_cv = sum_p w_cp U_cpv, elementwise, added in the order p = 0 .. n_vp-1."""
    n, n_vp = w.shape
    Uf = U.reshape(n, n_vp, -1).astype(dtype)
    w = w.astype(dtype)
    f = w[:, 0, None] * Uf[:, 0]
    for p in range(1, n_vp):
        f = f + w[:, p, None] * Uf[:, p]
    return f


def step(P, U, F, Y, dtype, c):
    """Forward and backward of one step at parameters P (dict of dtype arrays). Returns a dict: loss, f, w, dw, dz, mu, istd, the gradients
    under their parameter names, and abs_gU = sum_v |g U| (the summation bound of dw)."""
    T = dtype
    n, n_vp = U.shape[:2]
    R = n * n_vp
    Uf, Yf, Ff = U.reshape(n, n_vp, -1).astype(T), Y.reshape(n, -1).astype(T), F.astype(T)
    V = Uf.shape[2]
    one, a1, clip, eps, l2 = T(1), T(c["w_for_1"]), T(c["clip"]), T(c["bn_eps"]), T(c["l2"])
    a = Ff @ P["W1"]
    mu = a.sum(0) / T(R)
    var = ((a - mu) ** 2).sum(0) / T(R)
    istd = one / np.sqrt(var + eps)
    xh = (a - mu) * istd
    h = one / (one + np.exp(-(P["gamma"] * xh + P["beta"])))
    z = (h @ P["w2"] + P["b2"][0]).reshape(n, n_vp)
    e = np.exp(z - z.max(1, keepdims=True))
    w = e / e.sum(1, keepdims=True)
    f = fuse(w, Uf, T)
    lo, hi = clip, one - clip
    fc = np.minimum(np.maximum(f, lo), hi)
    wy, wn = a1 * Yf, (one - a1) * (one - Yf)
    nV = T(n * V)
    loss = (-(wy * np.log(fc) + wn * np.log(one - fc))).sum() / nV
    if c["l2"] != 0:
        loss = loss + l2 * ((P["W1"] ** 2).sum() + (P["w2"] ** 2).sum())
    g = np.where((f < lo) | (f > hi), T(0), -wy / fc + wn / (one - fc)) / nV
    gU = g[:, None, :] * Uf
    dw = gU.sum(2)
    dz = w * (dw - (w * dw).sum(1, keepdims=True))
    dzf = dz.reshape(R)
    dy = dzf[:, None] * P["w2"][None, :] * h * (one - h)
    dxh = dy * P["gamma"]
    da = istd / T(R) * (T(R) * dxh - dxh.sum(0) - xh * (dxh * xh).sum(0))
    out = dict(loss=loss, f=f, w=w, dw=dw, dz=dz, mu=mu, istd=istd, abs_gU=np.abs(gU).sum(2),
               W1=Ff.T @ da, beta=dy.sum(0), gamma=(dy * xh).sum(0), w2=h.T @ dzf, b2=np.array([dzf.sum()], T))
    if c["l2"] != 0:
        out["W1"] = out["W1"] + T(2) * l2 * P["W1"]
        out["w2"] = out["w2"] + T(2) * l2 * P["w2"]
    return out


def update(P, Vel, G, dtype, c):
    """The update of DESIGN.md section 4.11 in this operation order: t = lr g; v' = m v - t; p' = (p - t) + m v' (nesterov_momentum), p' = p - t
    (sgd); running statistics mean <- (1 - alpha) mean + alpha mu, inv_std alike. G holds the gradients and mu, istd. -> (P', Vel')"""
    T = dtype
    lr, m, alpha, one = T(c["lr"]), T(c["momentum"]), T(c["bn_alpha"]), T(1)
    P2, V2 = dict(P), dict(Vel)
    if c["update"] == "none":
        return P2, V2
    for k in TRAINABLE:
        t = lr * G[k].astype(T)
        if c["update"] == "nesterov_momentum":
            V2[k] = m * Vel[k] - t
            P2[k] = (P[k] - t) + m * V2[k]
        else:
            P2[k] = P[k] - t
    P2["mean"] = (one - alpha) * P["mean"] + alpha * G["mu"].astype(T)
    P2["inv_std"] = (one - alpha) * P["inv_std"] + alpha * G["istd"].astype(T)
    return P2, V2


def train(P, U, F, Y, dtype, c, steps):
    """`steps` steps on one batch from zero velocities. -> (P, Vel, [loss per step], last step's dict)"""
    Vel = zero_velocities(dtype)
    losses, out = [], None
    for _ in range(steps):
        out = step(P, U, F, Y, dtype, c)
        losses.append(float(out["loss"]))
        P, Vel = update(P, Vel, out, dtype, c)
    return P, Vel, losses, out


def inference_weights(P, F, n_vp, dtype=np.float64):
    """The deterministic MLP (running statistics) the inference entries evaluate: softmax over each cube's n_vp rows."""
    T = dtype
    a = F.astype(T) @ P["W1"].astype(T)
    sc = P["gamma"].astype(T) * P["inv_std"].astype(T)
    hh = 1.0 / (1.0 + np.exp(-(a * sc + (P["beta"].astype(T) - P["mean"].astype(T) * sc))))
    z = (hh @ P["w2"].reshape(H).astype(T) + P["b2"].reshape(1)[0].astype(T)).reshape(-1, n_vp)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)
