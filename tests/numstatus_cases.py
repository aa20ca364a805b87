"""The nets of tests/test_gpu_numstatus.py, built from parameters alone (no device), so that tests/test_numstatus_cpu.py can hold each case's
preconditions to the fp64 oracle. Planting uses what sn_load_weights does with a layer's BatchNorm (sn_api.hip, sn_pack.h pack_conv_host):
the stored value of ReLU layer channel o is ReLU(acc * scale + shift) with scale = gamma * inv_std * 2^(oe - row), shift = (beta - mean * gamma *
inv_std) * 2^oe, oe = -ilogb(max(|gamma|, |beta|)) and row = -ilogb(max |W[o]|). gamma and beta alone therefore cannot move a stored value
out of [1, 2) x the normalised pre-activation - the renormalisation undoes them - but mean and inv_std do not enter oe:

  * dead(layer, ch, v): W[ch] = 0, gamma = 1, beta = 0, inv_std = 1, mean = -v: acc = 0, oe = 0, shift = v: the channel stores fp16(v) at
    every voxel of every sample, exactly.
  * probe(layer, c, producer channel j storing p > 0 everywhere, B): W[c] = 0 but the centre tap on j = -K (K a power of two, K p > B),
    gamma = 1, beta = 0, inv_std = 1, mean = -B: inside the volume the centre tap always reads p, the pre-activation is B - K p < 0 and the
    channel stores 0; on an all-zero input (what a lane outside the volume is fed) it would store B.

Channels 0 and last of every stored ReLU layer (and concat channel 15) are cut from their consumers in the base net, so that whatever is
planted THERE changes no other tensor: the base net's tensors are the tensors of every planted case, but for the planted channel."""
import numpy as np

import synth
from oracle import net_oracle

CONSUMERS = {"conv1_1": ["conv1_2"], "conv1_2": ["conv1_3"], "conv2_1": ["conv2_2"], "conv2_2": ["conv2_3"], "conv3_1": ["conv3_2"], "conv3_2": ["conv3_3"],
             "conv3_3": ["side_op3", "conv4_1"], "conv4_1": ["conv4_2"], "conv4_2": ["conv4_3"], "conv4_3": ["side_op4"], "merge_conv_a": ["merge_conv_b"]}
CIN_FIRST = {"conv4_1", "conv4_2", "conv4_3", "side_op4"}           # the dilated layers store W as (C_in, C_out, k, k, k)
COUT = {name: cout for name, _, _, cout, _ in net_oracle.LAYERS}
IX = {(layer, p): i for i, (layer, p, _) in enumerate(net_oracle.PARAM_LAYOUT)}
PRODUCER = {"conv1_2": "conv1_1", "conv2_2": "conv2_1", "conv4_2": "conv4_1", "merge_conv_a": "side_op1"}
PROBE_K = float(2 ** 18)
TAME = 0.25          # the base net's ReLU layers see a quarter of their calibrated spread: stored values stay far below every limit


def _cin_view(values, layer):
    """W of `layer` as (C_out, C_in, k, k, k), a view."""
    W = values[IX[(layer, "W")]]
    return W.transpose(1, 0, 2, 3, 4) if layer in CIN_FIRST else W


def base_values(seed=1):
    values = [np.array(v) for v in synth.calibrated_params(seed)]
    for layer, cons in CONSUMERS.items():
        values[IX[(layer, "inv_std")]] *= np.float32(TAME)
        for c in cons:
            _cin_view(values, c)[:, [0, COUT[layer] - 1]] = 0.0
    _cin_view(values, "merge_conv_a")[:, 15] = 0.0
    return values


def dead(values, layer, ch, v):
    _cin_view(values, layer)[ch] = 0.0
    for p, x in (("gamma", 1.0), ("beta", 0.0), ("inv_std", 1.0), ("mean", -float(v))):
        values[IX[(layer, p)]][ch] = np.float32(x)
    assert float(np.float32(v)) == float(v)
    return values


def probe(values, layer, c, B):
    """-> p, the constant the producer channel stores. B = 0: the same net with nothing to tell."""
    prod = PRODUCER[layer]
    if prod == "side_op1":                    # concat channel 15 = side_op1's channel 15: gamma = beta = 0 -> sigmoid(0) = 0.5 everywhere
        j, p = 15, 0.5
        for q in ("gamma", "beta"):
            values[IX[(prod, q)]][j] = 0.0
    else:
        j, p = COUT[prod] - 1, 1.0
        dead(values, prod, j, p)
    W = _cin_view(values, layer)
    W[c] = 0.0
    W[c, j, 1, 1, 1] = -PROBE_K
    for q, x in (("gamma", 1.0), ("beta", 0.0), ("inv_std", 1.0), ("mean", -float(B))):
        values[IX[(layer, q)]][c] = np.float32(x)
    assert PROBE_K * p > B
    return p


def next_f16(v, k=1):
    """The k-th fp16 above the fp16 value v (> 0)."""
    b = np.asarray(v, dtype=np.float16).view(np.uint16)
    assert float(np.asarray(v, dtype=np.float16)) == float(v)
    return float((b + np.uint16(k)).view(np.float16))


def spike_net(values):
    """conv1_1 channel 31 reads input plane 0 through its centre tap alone: gamma = 1, beta = 0, mean = 0, inv_std = 1, W = 1: stores
    ReLU(x[0]) exactly (for x[0] a half)."""
    W = _cin_view(values, "conv1_1")
    W[31] = 0.0
    W[31, 0, 1, 1, 1] = 1.0
    for q, x in (("gamma", 1.0), ("beta", 0.0), ("inv_std", 1.0), ("mean", 0.0)):
        values[IX[("conv1_1", q)]][31] = np.float32(x)
    return values


def stored_oracle(values, X):
    """layer -> the fp64 oracle's output of every stored ReLU layer in STORED units (x 2^oe), (S, C, D, D, D)."""
    from oracle import net_emulation
    P = net_oracle.params_to_dict(values)
    _, _, inter = net_oracle.forward_torch(X, values, return_intermediates=True)
    name = {"merge_conv_a": "merge_a"}
    return {layer: np.ldexp(inter[name.get(layer, layer)], net_emulation.renorm_exponents(P[layer]).astype(np.int64)[None, :, None, None, None])
            for layer in CONSUMERS}
