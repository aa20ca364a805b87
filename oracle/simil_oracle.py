"""oracle/simil_oracle.py — TEST INFRASTRUCTURE (checker only; never imported by the product).

CPU restatement of the similarityNet / early-rejection stage:

    crop_patches      utils/image.py:92-183 cropImgPatches at pyramidRate = 1 (the call form of utils/earlyRejection.py:50)
    preprocess        utils/image.py:9-36   preprocess_patches
    embedding_torch   nets/similarityNet.py:23-58  __input_var_TO_embedding_layer__ (torch CPU conv2d, float64 by default)
    embedding_numpy   the same network in plain numpy (independent formulation, small batches)
    pair_similarity   nets/similarityNet.py:71-77  DistanceLayer(Lp=2) + DenseLayer(1, sigmoid)

PARITY of the numpy/indexing parts is PINNED: tests/golden/simil_cases.npz holds outputs of the reference's own
cropImgPatches / preprocess_patches / img_hw_cubesCorner_inScopeCheck / perspectiveProj_cubesCorner / patch2embedding /
embeddingPairs2simil / selectFromSimilarity executed in the build container (oracle/gen_golden_simil.py).
PARITY of the NETWORK is UNPINNED: its arithmetic lives in Theano/Lasagne/cuDNN (absent), the reference has neither a
test nor weights for it. Layer semantics restated from the call sites:
  * ConvLayer = lasagne.layers.dnn.Conv2DDNNLayer when cuDNN is present (similarityNet.py:6-9): W (Cout,Cin,3,3), pad=1,
    CROSS-CORRELATION (flip_filters=False is that layer's default), + b, rectify (Lasagne's default nonlinearity).
  * Pool2DLayer(2): max, stride 2. CropFeatureMapCenterLayer(r=1): rows/cols [H/2-1, H/2+1), flattened (c,h,w)
    (nets/layers.py:73-78). ConcatLayer order: pool5 flatten, crops of pool1, pool2, pool3, pool4 (similarityNet.py:49-55).
  * L2NormLayer: x / sqrt(sum x^2) per row (layers.py:38-42). embedding = DenseLayer(128, nonlinearity=None): x.W + b.
  * pair similarity: sigmoid(W * ((sum |e1-e2|^2) ** 0.5) + b) (layers.py:130-138, similarityNet.py:76).
"""
import numpy as np

CONVS = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
         (512, 512), (512, 512), (512, 512)]
POOL_AFTER = {1, 3, 6, 9, 12}          # index of the last conv of each block


def crop_patches(img, center_h, center_w, patchSize=64):
    """(n, patchSize, patchSize, c) patches of img (h,w,c): top-left = trunc(centre) - patchSize/2, coordinates clamped."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    r = patchSize // 2
    h0 = np.asarray(center_h, dtype=np.float64).astype(np.int64) - r
    w0 = np.asarray(center_w, dtype=np.float64).astype(np.int64) - r
    hh = np.clip(h0[:, None] + np.arange(patchSize)[None, :], 0, H - 1)
    ww = np.clip(w0[:, None] + np.arange(patchSize)[None, :], 0, W - 1)
    return img[hh[:, :, None], ww[:, None, :], :]


def preprocess(patches, mean_BGR):
    """(n,h,w,3) RGB any dtype -> (n,3,h,w) float32 BGR - mean."""
    x = np.asarray(patches).astype(np.float32)
    x = np.transpose(x, (0, 3, 1, 2))[:, ::-1]
    return np.ascontiguousarray(x - np.asarray(mean_BGR, dtype=np.float32)[None, :, None, None])


def _features(pools):
    """pools: list of 5 arrays (n,C,H,H) -> (n,5888) concat in the reference's order."""
    n = pools[0].shape[0]
    crop = lambda p: p[:, :, p.shape[2] // 2 - 1: p.shape[2] // 2 + 1, p.shape[3] // 2 - 1: p.shape[3] // 2 + 1].reshape(n, -1)
    return np.concatenate([pools[4].reshape(n, -1), crop(pools[0]), crop(pools[1]), crop(pools[2]), crop(pools[3])], axis=1)


def _quantizer(torch, quant, td):
    """Storage rounding of an arithmetic class: None exact; "fp16" one half; "x3" an unevaluated sum hi + lo of two halfs (the operand and
    storage format of the device's f16x3 arithmetic)."""
    def q(t):
        if quant == "x3":
            h = t.to(torch.float16).to(td)
            return h + (t - h).to(torch.float16).to(td)
        return t.to(torch.float16).to(td) if quant == "fp16" else t
    return q


def _layer(torch, F, values, i, x, ax, td, q, quant):
    """Layer i on x: -> (y, A) AFTER ReLU and, for i in POOL_AFTER, the 2x2 max-pool; y not yet rounded for storage. The bias is added in
    float32 where the class's epilogue is float32 (quant "fp16", dtype float32), as the device's is. ax: |x| (None: no error scale wanted)."""
    W = q(torch.from_numpy(np.asarray(values[2 * i])).to(td))
    b = np.asarray(values[2 * i + 1])
    bt = torch.float32 if (quant == "fp16" or td == torch.float32) else td
    y = F.conv2d(x, W, None, padding=1).to(bt) + torch.from_numpy(b).to(bt).view(1, -1, 1, 1)
    y = torch.relu(y).to(td)
    a = None
    if ax is not None:
        a = F.conv2d(ax, W.abs(), None, padding=1) + torch.from_numpy(np.abs(b)).to(td).view(1, -1, 1, 1)
    if i in POOL_AFTER:
        y = F.max_pool2d(y, 2)
        a = F.max_pool2d(a, 2) if a is not None else None      # |max a - max b| <= max |a - b|
    return y, a


def embedding_torch(X, values, dtype="float64", return_pools=False, quant=None, return_intermediates=False):
    """quant / dtype: the arithmetic class, as net_oracle.forward_torch / step_torch - None exact; "x3" weights, input and every stored
    map as hi + lo pairs of halfs (use dtype float32: the class reference of the f16x3 arithmetic); "fp16" weights, input and stored maps as
    halfs, wide accumulation, float32 bias (the class reference of the f16 mode). With a quant, feat and emb are evaluated in float32
    from the class's stored pools (feat_step / emb_step); without one in float64, whatever the convolutions' dtype.
    return_intermediates: -> (emb, inter), inter = {"p0": the input as stored, layer name: its post-ReLU (post-pool) map, "feat", "emb"}."""
    import torch
    import torch.nn.functional as F
    dt = getattr(torch, dtype)
    q = _quantizer(torch, quant, dt)
    x = q(torch.from_numpy(np.ascontiguousarray(X)).to(dt))
    pools, inter = [], {"p0": x.to(torch.float64).numpy()}
    with torch.no_grad():
        for i in range(13):
            x = q(_layer(torch, F, values, i, x, None, dt, q, quant)[0])
            inter[LAYER_NAMES[i]] = x.to(torch.float64).numpy()
            if i in POOL_AFTER:
                pools.append(x.numpy().copy())
    fd = "float64" if quant is None else "float32"
    f = feat_step(pools, dtype=fd)
    emb = emb_step(values, f, dtype=fd)
    if not return_intermediates and not return_pools:
        return emb
    inter["feat"], inter["emb"] = np.asarray(f, dtype=np.float64), np.asarray(emb, dtype=np.float64)
    return (emb, inter) if return_intermediates else (emb, pools)


LAYER_NAMES = ["s_conv1_1", "s_conv1_2", "s_conv2_1", "s_conv2_2", "s_conv3_1", "s_conv3_2", "s_conv3_3", "s_conv4_1", "s_conv4_2", "s_conv4_3",
               "s_conv5_1", "s_conv5_2", "s_conv5_3"]


def step(values, i, x, dtype="float64", quant=None):
    """One launch of the device's plan applied to a given input x (n, Cin, H, H), e.g. the device's own decoded stored tensor: layer i's
    conv + bias + ReLU, + the 2x2 max-pool if i in POOL_AFTER, stored in the class's format (dtype / quant as embedding_torch; quant also
    rounds the weights and the input). Returns (y, A): A, the forward-error scale of the element - the magnitude an error of relative
    size eps in every product and in the bias can reach: |W| (*) |x| + |b| before ReLU (1-Lipschitz) and pooling; a pooled element takes the
    maximum of A over its window."""
    import torch
    import torch.nn.functional as F
    td = getattr(torch, dtype)
    q = _quantizer(torch, quant, td)
    with torch.no_grad():
        xt = q(torch.from_numpy(np.ascontiguousarray(x)).to(td))
        y, a = _layer(torch, F, values, i, xt, xt.abs(), td, q, quant)
        return q(y).to(torch.float64).numpy(), a.to(torch.float64).numpy()


def _seq_sum(a, dtype):
    """Sum over the last axis; in float32 the textbook left-to-right sum (numpy's pairwise / BLAS's blocked orders are properties of a
    library, not of the number format)."""
    if dtype == "float64":
        return a.sum(axis=-1)
    return np.cumsum(a, axis=-1, dtype=np.float32)[..., -1]


def feat_step(pools, dtype="float64"):
    """pool1 .. pool5 (n, C, H, H) -> the (n, 5888) L2-normalised feature rows (gather of _features, x * (1 / sqrt(sum x^2)))."""
    dt = np.dtype(dtype)
    f = _features([np.asarray(p) for p in pools]).astype(dt)
    inv = dt.type(1) / np.sqrt(_seq_sum(f * f, dtype))
    return f * inv[:, None]


def emb_step(values, feat, dtype="float64", with_scale=False):
    """feat (n, 5888) -> emb (n, 128) = feat . W + b; with_scale: also A = |feat| . |W| + |b|."""
    dt = np.dtype(dtype)
    f, W, b = np.asarray(feat).astype(dt), np.asarray(values[26]).astype(dt), np.asarray(values[27]).astype(dt)
    if dtype == "float64":
        emb = f @ W + b
    else:
        acc = np.zeros((f.shape[0], W.shape[1]), dtype=dt)
        for k in range(W.shape[0]):
            acc += f[:, k, None] * W[k][None, :]
        emb = acc + b
    if with_scale:
        return emb, np.abs(np.asarray(feat, dtype=np.float64)) @ np.abs(W.astype(np.float64)) + np.abs(b.astype(np.float64))
    return emb


def embedding_numpy(X, values):
    """Independent formulation: 3x3 cross-correlation as 9 shifted tensordots, float64."""
    x = np.asarray(X, dtype=np.float64)
    pools = []
    for i in range(13):
        W = np.asarray(values[2 * i], dtype=np.float64)
        b = np.asarray(values[2 * i + 1], dtype=np.float64)
        n, c, H, Wd = x.shape
        xp = np.zeros((n, c, H + 2, Wd + 2))
        xp[:, :, 1:-1, 1:-1] = x
        y = np.zeros((n, W.shape[0], H, Wd))
        for dy in range(3):
            for dx in range(3):
                y += np.einsum("nchw,oc->nohw", xp[:, :, dy:dy + H, dx:dx + Wd], W[:, :, dy, dx], optimize=True)
        x = np.maximum(y + b[None, :, None, None], 0)
        if i in POOL_AFTER:
            n, c, H, Wd = x.shape
            x = x.reshape(n, c, H // 2, 2, Wd // 2, 2).max(axis=(3, 5))
            pools.append(x)
    f = _features(pools)
    f = f / np.sqrt((f ** 2).sum(axis=1))[:, None]
    return f @ np.asarray(values[26], dtype=np.float64) + np.asarray(values[27], dtype=np.float64)


def pair_similarity(emb_pairs, values):
    e = np.asarray(emb_pairs, dtype=np.float64).reshape(-1, 2, emb_pairs.shape[-1])
    d = np.sqrt((np.abs(e[:, 0] - e[:, 1]) ** 2).sum(axis=1, keepdims=True))
    w, b = float(np.asarray(values[28]).reshape(())), float(np.asarray(values[29]).reshape(()))
    return 1.0 / (1.0 + np.exp(-(w * d + b)))
