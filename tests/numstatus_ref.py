"""Restatement of the numeric status words and of the calibration scan as exact integer functions of the bits the device stored (numpy only,
no device): the error word (SN_ERR_RANGE), the warning word (sn_numeric_status) and the report of sn_calibrate_dev, from the raw buffers and
Layouts that test_gpu_layers.read_back returns (tests/act_decode.py), the plan's storage table (tests/layer_check.py storage) and the number
of samples the call ran. Every constant is read off the code, none off a run:

  * warning limit (surfacenet_amd/csrc/sn_internal.h, the conv launcher): a layer has one iff its kernel is a store kernel (EPI_STORE: not the
    fused conv1_3 / conv2_3, not merge_conv_b), its output format carries a code plane (output format >= 2) and it ends in a ReLU; the limit is
    fp16(min(60000, ldexp(base, e8 - 127))), base 255.875 for fp8 planes and 7.5 (SN_MX_FMT 2, e2m3; 28 for SN_MX_FMT 3, e3m2: mx_format.h /
    sn_consts.h) for 6-bit planes; the warning bit is raised iff a stored hi half's bit pattern is GREATER than the limit's
    (conv3d_mfma.h: sn_tracked_max_bits(trk_h) > a.mx_sat_bits).
  * error word (conv3d_mfma.h sn_tracked_bad): a stored hi half of +inf (bits >= 0x7c00), or a non-finite accumulator.
  * calibration (elementwise.h mx_scan_kernel, sn_api.hip sn_calibrate_dev): thirteen counts of |v| > fp16(lim * 2^-(j - 6)), j = 0 .. 12, the
    count of non-zero values and the largest magnitude over the first n_samples samples of the hi planes of merge_conv_a's output ("act") and
    of the concat buffer ("cat"); then the host rule."""
import numpy as np

import act_decode as ad

SN_MX_FMT = 2                                        # sn_consts.h (the shipped 6-bit form: fp6 e2m3)
BASE6 = {2: 7.5, 3: 28.0}[SN_MX_FMT]                 # sn_internal.h / sn_api.hip: SN_MX_FMT == 2 ? 7.5f : 28.f
BASE8 = 255.875                                      # sn_internal.h: OS >= 3 ? 255.875f
LIMIT_CAP = 60000.0
SCAN_BINS = 13                                       # elementwise.h kMxScanBins: premultiplier exponents s = -6 .. +6
INF_BITS = 0x7c00

# ReLU layers launched on a store kernel -> the buffer they write (sn_api.hip build_plan_t). conv3_1's and conv4_1's tensors do not survive a pass
# (conv3_3 / conv4_3 overwrite a3 / a4): SURVIVES says whose bits a read-back after the pass holds.
STORE_LAYERS = {"conv1_1": "a1", "conv1_2": "b1", "conv2_1": "a2", "conv2_2": "b2", "conv3_1": "a3", "conv3_2": "b3", "conv3_3": "a3",
                "conv4_1": "a4", "conv4_2": "b4", "conv4_3": "a4", "merge_conv_a": "ma"}
SURVIVES = {"conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_2", "conv3_3", "conv4_2", "conv4_3", "merge_conv_a"}
REAL_CHANNELS = {"a1": 32, "b1": 32, "a2": 80, "b2": 80, "a3": 160, "b3": 160, "a4": 300, "b4": 300, "ma": 100, "cat": 64}


def f16_bits(v):
    """Bit pattern of the fp16 nearest to v (round to nearest even, as the (_Float16) casts of the launcher and of the scan kernel)."""
    with np.errstate(over="ignore"):                 # (beyond 65504: inf, as the device's conversion)
        return int(np.asarray(v, dtype=np.float64).astype(np.float16).view(np.uint16))


def bits_f16(b):
    return float(np.asarray(b, dtype=np.uint16).view(np.float16))


def layer_formats(precision, conv4_fp8, buffer_fmt):
    """layer -> act_decode.FMT_* of the tensor THAT LAYER writes. buffer_fmt: layer_check.storage(...)[0], the format of each buffer's last
    write; the two layers whose tensor is overwritten later in the pass are stated here (build_plan_t): conv3_1 writes the operand mode's
    format; conv4_1 writes hi + fp8 slots when conv4_fp8 is 1 or 2 (f16x3), the operand mode's format otherwise."""
    c4 = (1 if precision == "f16x3" else 0) if conv4_fp8 is None else int(conv4_fp8)
    mode_fmt = {"f16": ad.FMT_F16, "f16x3p": ad.FMT_HILO, "f16x3": ad.FMT_HILO, "f16m8": ad.FMT_M6}[precision]
    out = {layer: buffer_fmt[buf] for layer, buf in STORE_LAYERS.items()}
    out["conv3_1"] = mode_fmt
    out["conv4_1"] = ad.FMT_M8 if (precision == "f16x3" and c4 in (1, 2)) else mode_fmt
    return out


def limited_layers(precision, conv4_fp8, buffer_fmt):
    """layer -> base of its warning limit, for the layers the launcher gives one."""
    out = {}
    for layer, fmt in layer_formats(precision, conv4_fp8, buffer_fmt).items():
        if fmt == ad.FMT_M6:
            out[layer] = BASE6
        elif fmt in (ad.FMT_M8, ad.FMT_HILO_M8):
            out[layer] = BASE8
    return out


def limit_bits(base, e8):
    """fp16 bits of min(60000, ldexp(base, e8 - 127)) - the launcher computes it in float and casts."""
    return f16_bits(np.float32(min(LIMIT_CAP, float(np.ldexp(np.float32(base), int(e8) - 127)))))


def hi_bits(raw, lay, n_run, channels):
    """|hi plane| as bit patterns: (n_run, channels, D, D, D) uint16 with the sign bit cleared (every tracker and the scan clear it)."""
    D, G, M = lay.extent, lay.cs // 8, lay.max_samples()
    assert 0 < n_run <= M and 0 < channels <= lay.cs
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    h = np.frombuffer(raw, dtype=np.uint16, count=M * G * D ** 3 * 8, offset=0).reshape(M, G, D, D, D, 8)[:n_run]
    h = h.transpose(0, 1, 5, 2, 3, 4).reshape(n_run, G * 8, D, D, D)[:, :channels]
    return h & np.uint16(0x7fff)


def stored_max_bits(raw, lay, n_run, channels):
    """-> (largest fp16 bit pattern of the hi plane over the real channels and samples 0 .. n_run - 1, its (sample, channel, x, y, z))."""
    b = hi_bits(raw, lay, n_run, channels)
    k = int(np.argmax(b))
    return int(b.reshape(-1)[k]), tuple(int(i) for i in np.unravel_index(k, b.shape))


def warning_names(raws, lays, n_run, precision, conv4_fp8, buffer_fmt, gone=None):
    """The set sn_numeric_status must name after a pass of n_run samples. A limited layer whose tensor survives the pass is in the set iff
    stored_max_bits > bits(limit). gone: layer -> bool for the limited layers whose tensor is overwritten (conv3_1, conv4_1) - the caller's
    verdict from what it planted there; a missing verdict for such a layer is an error, never a guess."""
    names = set()
    for layer, base in limited_layers(precision, conv4_fp8, buffer_fmt).items():
        buf = STORE_LAYERS[layer]
        if layer not in SURVIVES:
            assert gone is not None and layer in gone, "no stored bits for %s: the caller has to say" % layer
            if gone[layer]:
                names.add(layer)
            continue
        mx, _ = stored_max_bits(raws[buf], lays[buf], n_run, REAL_CHANNELS[buf])
        if mx > limit_bits(base, lays[buf].e8):
            names.add(layer)
    return names


def error_expected(raws, lays, n_run):
    """Layers of STORE_LAYERS that stored an inf (hi bits >= 0x7c00) in a real channel of samples 0 .. n_run - 1 of a tensor that survives. For
    nets whose pre-activations are all finite the converse holds: no such value, no error."""
    return {layer for layer, buf in STORE_LAYERS.items() if layer in SURVIVES
            and stored_max_bits(raws[buf], lays[buf], n_run, REAL_CHANNELS[buf])[0] >= INF_BITS}


def scan(bits):
    """bits: |hi| bit patterns of the values scanned -> (13 counts of bits > thr[j], non-zero count, largest bit pattern); thr[j] =
    bits(fp16(lim * 2^-(j - 6))) (non-negative fp16 values order like their bit patterns)."""
    b = np.asarray(bits, dtype=np.uint16).reshape(-1)
    thr = [f16_bits(np.float32(np.ldexp(np.float32(BASE6), -(j - SCAN_BINS // 2)))) for j in range(SCAN_BINS)]
    counts = [int(np.count_nonzero(b > t)) for t in thr]
    return counts, int(np.count_nonzero(b)), int(b.max()) if b.size else 0


def host_rule(counts, nz, mx, max_sat_fraction, s_old):
    """sn_calibrate_dev's rule for one tensor -> (s_new, sat_before, sat_after, max)."""
    half = SCAN_BINS // 2
    if nz == 0:
        return s_old, 0.0, 0.0, bits_f16(mx)

    def frac(s):
        return float(counts[max(0, min(SCAN_BINS - 1, s + half))]) / float(nz)

    s_new = -half
    for cand in range(half, -half - 1, -1):
        if frac(cand) <= max_sat_fraction:
            s_new = cand
            break
    if max_sat_fraction < 0.0:
        s_new = s_old
    return s_new, frac(max(-half, min(half, s_old))), frac(s_new), bits_f16(mx)


def calibration(raw_ma, lay_ma, raw_cat, lay_cat, n_samples, max_sat_fraction, s_old):
    """The report sn_calibrate_dev must return (the fields of sn_calibration). s_old: (s_act, s_cat) in force before the call."""
    out = {}
    for key, raw, lay, C, so in (("act", raw_ma, lay_ma, REAL_CHANNELS["ma"], s_old[0]), ("cat", raw_cat, lay_cat, REAL_CHANNELS["cat"], s_old[1])):
        counts, nz, mx = scan(hi_bits(raw, lay, n_samples, C))
        s_new, before, after, m = host_rule(counts, nz, mx, max_sat_fraction, int(so))
        out["s_%s_before" % key], out["s_%s" % key] = int(so), int(s_new)
        out["sat_%s_before" % key], out["sat_%s" % key], out["max_%s" % key] = before, after, m
    return out
