"""No GPU: (1) tests/numstatus_ref.py can tell. A numpy stand-in for the device - a scan with 256-thread workgroups of 8-half vectors, a block
tail and a grid-stride loop; a tile walk whose fragments have lanes outside the volume and padded channel lanes - runs the cases of
tests/test_gpu_numstatus.py on synthetic stored tensors. Unfaulted it agrees with the restatement on every case; with each planted fault it
disagrees on the case named for it. (2) The preconditions of the GPU cases, on the fp64 oracle (oracle/net_oracle.py): what the base net
stores stays below half of every limit, a planted channel stores exactly what was planted and changes no other tensor, a probe channel
stores zeros over the whole volume while its zero-input value is the intended one."""
import numpy as np
import pytest

import act_decode as ad
import layer_check as lc
import numstatus_cases as nc
import numstatus_ref as ref
import synth

LIM6 = ref.limit_bits(ref.BASE6, 127)


# ------------------------------------------------------------------------------------------------
# the stand-in scan (elementwise.h mx_scan_kernel) and its planted faults
# ------------------------------------------------------------------------------------------------
def layout(s, cs, M):
    return ad.Layout(s, cs, 1, -1, -1, 127, M * s ** 3 * cs * 2, ad.FMT_F16)


def sim_scan(raw, lay, n_samples, C, fault=None):
    """The device's walk over the raw hi plane [M][cs / 8][voxel][8]: vector i of 8 halfs belongs to thread i mod 256 of workgroup
    (i / 256) mod grid, pass i / (256 grid), grid = min(2048, ceil(vectors / 256))."""
    M, G, vox = lay.max_samples(), lay.cs // 8, lay.extent ** 3
    n = M if fault == "samples beyond n_samples scanned" else n_samples
    b = np.frombuffer(raw, dtype=np.uint16, count=M * G * vox * 8).reshape(M * G * vox, 8) & np.uint16(0x7fff)
    vectors = n * G * vox
    grid = min(2048, -(-vectors // 256))
    scanned = vectors
    if fault == "dropped tail block":
        scanned = (vectors // 256) * 256
    if fault == "dropped second stride pass":
        scanned = min(vectors, grid * 256)
    v = b[:scanned]
    thr = [ref.f16_bits(np.ldexp(ref.BASE6, -(j - 6))) for j in range(13)]
    counts = [int(np.count_nonzero(v >= t if fault == ">= in place of >" else v > t)) for t in thr]
    nz = int(np.count_nonzero(v))
    if fault == "padded channels counted as non-zero":
        group = (np.arange(scanned) // vox) % G
        nz += int(np.count_nonzero(group == G - 1)) * (lay.cs - C)
    return counts, nz, int(v.max()) if v.size else 0


def sim_report(raws, lays, n, bound, s_old, fault=None):
    out = {}
    for key, buf, so in (("act", "ma", s_old[0]), ("cat", "cat", s_old[1])):
        counts, nz, mx = sim_scan(raws[buf], lays[buf], n, ref.REAL_CHANNELS[buf], fault)
        s_new, before, after, m = ref.host_rule(counts, nz, mx, bound, so)
        out.update({"s_%s_before" % key: so, "s_%s" % key: s_new, "sat_%s_before" % key: before, "sat_%s" % key: after, "max_%s" % key: m})
    return out


def stored_like(s, M, C, cs, seed, scale):
    """A ReLU tensor as the device would leave it: half zeros, values spread over the thresholds, zero pads; every sample and the last voxels
    of the last channel group hold values of their own (what a dropped tail, pass or sample would miss); the maximum grows with the sample."""
    rs = np.random.RandomState(seed)
    v = np.maximum(rs.standard_normal((M, C, s, s, s)) * scale, 0.0) * (1.0 + np.arange(M))[:, None, None, None, None]
    v[:, C - 1, s - 1, s - 1, s - 4:] = [0.12, 0.9, 7.6, 31.0]
    return ad.encode(v, layout(s, cs, M), M=M)


def scan_case(s, M, seed, scale_ma=2.5):
    lays = {"ma": layout(s, 104, M), "cat": layout(s, 64, M)}
    raws = {"ma": stored_like(s, M, 100, 104, seed, scale_ma), "cat": stored_like(s, M, 64, 64, seed + 1, 0.4)}
    return raws, lays


def threshold_case():
    s, M = 8, 2
    lays = {"ma": layout(s, 104, M), "cat": layout(s, 64, M)}
    v = np.maximum(np.random.RandomState(3).standard_normal((M, 100, s, s, s)), 0.0)
    for k in range(13):
        v[:, k] = np.ldexp(ref.BASE6, k - 6)
        v[:, 13 + k] = nc.next_f16(float(np.ldexp(ref.BASE6, k - 6)))
    return {"ma": ad.encode(v, lays["ma"], M=M), "cat": stored_like(s, M, 64, 64, 4, 0.4)}, lays


def zero_case():
    raws, lays = scan_case(8, 2, 9)
    raws["ma"][:] = 0
    return raws, lays


# (name, tensors, samples scanned, bound, exponents in force): the calls of test_gpu_numstatus.py's calibration tests
def scan_cases():
    c8, c12, c32 = scan_case(8, 4, 1), scan_case(12, 1, 2), scan_case(32, 2, 5)
    return [("8x4 scan 4", c8, 4, 1e-3, (0, 2)), ("8x4 scan 2", c8, 2, 1e-3, (0, 2)), ("8x4 bound 0", c8, 2, 0.0, (-1, 2)), ("8x4 measure only", c8, 4, -1.0, (-2, 1)),
            ("12x1 tail", c12, 1, 1e-3, (0, 2)), ("32x2 second pass", c32, 2, 1e-3, (0, 2)),
            ("thresholds", threshold_case(), 2, 0.3, (0, 2)), ("thresholds measure only", threshold_case(), 2, -1.0, (0, 2)),
            ("merge_conv_a all dead", zero_case(), 2, 1e-3, (0, 2))]


SCAN_FAULTS = {">= in place of >": "thresholds", "dropped tail block": "12x1 tail", "dropped second stride pass": "32x2 second pass",
               "padded channels counted as non-zero": "thresholds", "samples beyond n_samples scanned": "8x4 scan 2"}


@pytest.fixture(scope="module")
def scans():
    return scan_cases()


def test_scan_shapes_reach_the_tail_and_the_second_pass():
    assert (12 ** 3 * 104 // 8) % 256 != 0
    assert 2048 * 256 < 2 * 32 ** 3 * 104 // 8 < 2 * 2048 * 256
    assert 4 * 8 ** 3 * 104 // 8 < 2048 * 256 and (4 * 8 ** 3 * 104 // 8) % 256 == 0


def test_stand_in_scan_agrees_with_the_restatement_on_every_case(scans):
    for name, (raws, lays), n, bound, s_old in scans:
        want = ref.calibration(raws["ma"], lays["ma"], raws["cat"], lays["cat"], n, bound, s_old)
        assert sim_report(raws, lays, n, bound, s_old) == want, name
        assert bound >= 0 or (want["s_act"], want["s_cat"]) == s_old
    zero = [c for c in scans if c[0] == "merge_conv_a all dead"][0]
    want = ref.calibration(zero[1][0]["ma"], zero[1][1]["ma"], zero[1][0]["cat"], zero[1][1]["cat"], 2, 1e-3, (0, 2))
    assert (want["s_act"], want["sat_act"], want["sat_act_before"], want["max_act"]) == (0, 0.0, 0.0, 0.0)


@pytest.mark.parametrize("fault", sorted(SCAN_FAULTS))
def test_each_planted_scan_fault_fails_the_case_named_for_it(scans, fault):
    failed = []
    for name, (raws, lays), n, bound, s_old in scans:
        want = ref.calibration(raws["ma"], lays["ma"], raws["cat"], lays["cat"], n, bound, s_old)
        if sim_report(raws, lays, n, bound, s_old, fault) != want:
            failed.append(name)
    assert SCAN_FAULTS[fault] in failed, (fault, failed)


def test_host_rule_picks_the_largest_exponent_within_the_bound():
    counts = [0, 0, 0, 1, 2, 5, 10, 40, 100, 300, 500, 800, 1000]      # j = s + 6
    assert ref.host_rule(counts, 1000, 0x4000, 1e-3, 0) == (-3, 0.01, 0.001, 2.0)
    assert ref.host_rule(counts, 1000, 0x4000, 0.0, 0) == (-4, 0.01, 0.0, 2.0)
    assert ref.host_rule(counts, 1000, 0x4000, 0.005, 0)[0] == -1 and ref.host_rule(counts, 1000, 0x4000, 0.0049, 0)[0] == -2
    assert ref.host_rule(counts, 1000, 0x4000, 1.0 - 1e-9, 3)[0] == 5 and ref.host_rule([7] * 13, 10, 0x4000, 0.5, 0)[0] == -6
    assert ref.host_rule(counts, 1000, 0x4000, -1.0, 3) == (3, 0.3, 0.3, 2.0)
    assert ref.host_rule(counts, 0, 0, 1e-3, 2) == (2, 0.0, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------
# the stand-in tile walk (conv3d_mfma.h store epilogues) and its planted faults
# ------------------------------------------------------------------------------------------------
def sim_tracked_max(bits, zero_input, lanes, fault=None, T=8):
    """bits (S, C, D, D, D): what the lanes that store hold. Every tile of T^3 voxels x `lanes` channel lanes is walked whole: a lane whose voxel
    lies outside the volume holds its channel's zero-input value, a padded channel lane (>= C) holds channel (lane mod 4)'s - the constants the
    store kernels without an LDS table fetched for it. Returns the largest bit pattern the trackers saw."""
    S, C, D = bits.shape[:3]
    b = bits.copy()
    if fault == "last real channel untracked":
        b[:, C - 1] = 0
    if fault == "last sample untracked":
        b[S - 1] = 0
    if fault == "far-corner voxel untracked":
        b[:, :, D - 1, D - 1, D - 1] = 0
    mx = int(b.max())
    if fault == "invalid-voxel lanes tracked" and D % T:
        mx = max(mx, int(np.max(zero_input[:C])))
    if fault == "padded-channel lanes tracked with channel 0's constants" and lanes > C:
        mx = max(mx, int(np.max(zero_input[:4])))
    return mx


WORD_FAULTS = {"last real channel untracked": "dead last channel above", "last sample untracked": "spike", "far-corner voxel untracked": "spike",
               "invalid-voxel lanes tracked": "probe last channel", "padded-channel lanes tracked with channel 0's constants": "probe channel 0, full tile"}


def zero_input_bits(values, layer):
    """fp16 bits of what each channel of `layer` stores on all-zero input: ReLU(shift) in stored units (sn_pack.h)."""
    from oracle import net_emulation, net_oracle
    p = net_oracle.params_to_dict(values)[layer]
    g, b, m, i = (p[k].astype(np.float64) for k in ("gamma", "beta", "mean", "inv_std"))
    shift = np.ldexp(b - m * g * i, net_emulation.renorm_exponents(p).astype(np.int64))
    with np.errstate(over="ignore"):                 # (beyond 65504: inf)
        return np.minimum(np.maximum(shift, 0.0), 7e4).astype(np.float16).view(np.uint16).astype(np.int64)


@pytest.fixture(scope="module")
def word_cases():
    """name -> (layer, stored bits of that layer by the oracle (S, C, D, D, D), zero-input bits, channel lanes, limit bits, intended verdict)."""
    s, n = 12, 2
    X = synth.random_cvc(n, s, 40 + s)
    out = {}

    def add(name, values, layer, lanes, named, Xc=X, extent=None):
        st = nc.stored_oracle(values, Xc)[layer]
        lay = layout(st.shape[-1], -(-st.shape[1] // 8) * 8, st.shape[0])
        raw = ad.encode(st, lay, M=st.shape[0])
        assert ref.stored_max_bits(raw, lay, st.shape[0], st.shape[1])[0] == int(ref.hi_bits(raw, lay, st.shape[0], st.shape[1]).max())
        out[name] = (layer, ref.hi_bits(raw, lay, st.shape[0], st.shape[1]).astype(np.int64), zero_input_bits(values, layer), lanes, LIM6, named, raw, lay)

    v = ref.bits_f16(LIM6 + 1)
    add("tame", nc.base_values(), "merge_conv_a", 112, False)
    add("dead last channel above", nc.dead(nc.base_values(), "merge_conv_a", 99, v), "merge_conv_a", 112, True)
    add("dead last channel below", nc.dead(nc.base_values(), "merge_conv_a", 99, v / 2), "merge_conv_a", 112, False)
    Xs = X.copy()
    Xs[:, 0] = 0.0
    Xs[n - 1, 0, s - 1, s - 1, s - 1] = v
    add("spike", nc.spike_net(nc.base_values()), "conv1_1", 32, True, Xc=Xs)
    for name, c, size in (("probe last channel", 99, 12), ("probe channel 0", 0, 12), ("probe channel 0, full tile", 0, 8)):
        values = nc.base_values()
        nc.probe(values, "merge_conv_a", c, 4 * ref.BASE6)
        add(name, values, "merge_conv_a", 112, False, Xc=synth.random_cvc(1, size, 3) if size != 12 else X)
    return out


def test_stand_in_walk_agrees_with_the_restatement_on_every_case(word_cases):
    for name, (layer, bits, zi, lanes, lim, named, raw, lay) in word_cases.items():
        want = ref.stored_max_bits(raw, lay, bits.shape[0], bits.shape[1])[0] > lim
        assert (sim_tracked_max(bits, zi, lanes) > lim) == want == named, name


@pytest.mark.parametrize("fault", sorted(WORD_FAULTS))
def test_each_planted_walk_fault_fails_the_case_named_for_it(word_cases, fault):
    failed = [name for name, (layer, bits, zi, lanes, lim, named, raw, lay) in word_cases.items() if (sim_tracked_max(bits, zi, lanes, fault) > lim) != named]
    assert WORD_FAULTS[fault] in failed, (fault, failed)


# ------------------------------------------------------------------------------------------------
# preconditions of the GPU cases, on the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [12, 16])
def test_base_net_stores_less_than_half_of_every_limit(s):
    """Every stored ReLU tensor of the base net, in stored units, stays below 7.5 / 2 (and so below 255.875 / 2): the tame set is empty with a
    factor two to spare against the device's own arithmetic, also for conv3_1 and conv4_1, whose tensors no read-back holds."""
    st = nc.stored_oracle(nc.base_values(), synth.random_cvc(2, s, 40 + s))
    for layer, t in st.items():
        assert float(t.max()) < ref.BASE6 / 2, (layer, float(t.max()))
    st = nc.stored_oracle(nc.base_values(), synth.random_cvc(4, 12, 61)[:1])
    assert max(float(t.max()) for t in st.values()) < ref.BASE6 / 2


def test_a_planted_channel_stores_the_planted_value_and_changes_nothing_else():
    s = 12
    X = synth.random_cvc(2, s, 40 + s)
    base = nc.stored_oracle(nc.base_values(), X)
    fmt = lc.storage("f16m8")[0]
    for layer, lim in sorted(ref.limited_layers("f16m8", None, fmt).items()):
        ch = nc.COUT[layer] - 1
        v = ref.bits_f16(ref.limit_bits(lim, 127) + 1)
        got = nc.stored_oracle(nc.dead(nc.base_values(), layer, ch, v), X)
        for other, t in got.items():
            if other == layer:
                assert (t[:, ch] == v).all() and np.array_equal(np.delete(t, ch, axis=1), np.delete(base[layer], ch, axis=1)), layer
            else:
                assert np.array_equal(t, base[other]), (layer, other)
    assert ref.bits_f16(ref.limit_bits(ref.BASE8, 127) + 1) == 256.0 and ref.bits_f16(LIM6 + 1) == 7.50390625
    assert set(ref.limited_layers("f16x3", None, lc.storage("f16x3")[0])) == {"conv3_3", "conv4_1", "conv4_2", "merge_conv_a"}
    assert set(ref.limited_layers("f16x3", 2, lc.storage("f16x3", 2)[0])) == {"conv4_1", "conv4_2", "merge_conv_a"}
    assert set(ref.limited_layers("f16x3", 0, lc.storage("f16x3", 0)[0])) == {"merge_conv_a"}
    assert set(ref.limited_layers("f16m8", None, fmt)) == set(ref.STORE_LAYERS) and not ref.limited_layers("f16x3p", None, lc.storage("f16x3p")[0])


@pytest.mark.parametrize("layer", ["conv1_2", "conv2_2", "conv4_2", "merge_conv_a"])
def test_a_probe_channel_stores_zeros_and_would_store_B_on_zero_input(layer):
    s = 12
    X = synth.random_cvc(2, s, 40 + s)
    for c in (0, nc.COUT[layer] - 1):
        for B in (0.0, 4 * ref.BASE6, 4 * ref.BASE8, 1e5):
            values = nc.base_values()
            p = nc.probe(values, layer, c, B)
            st = nc.stored_oracle(values, X)
            assert not st[layer][:, c].any(), (layer, c, B)
            assert zero_input_bits(values, layer)[c] == ref.f16_bits(min(B, 7e4)), (layer, c, B)
            if layer != "merge_conv_a":
                assert (st[nc.PRODUCER[layer]][:, nc.COUT[nc.PRODUCER[layer]] - 1] == p).all()
            assert max(float(t.max()) for t in st.values()) < ref.BASE6 / 2


def test_the_spike_is_the_only_value_above_the_limit():
    s, n = 12, 2
    for k, above in ((1, 1), (0, 0)):
        v = ref.bits_f16(LIM6 + k)
        X = synth.random_cvc(n, s, 40 + s)
        X[:, 0] = 0.0
        X[n - 1, 0, s - 1, s - 1, s - 1] = v
        st = nc.stored_oracle(nc.spike_net(nc.base_values()), X)
        assert sum(int(np.count_nonzero(t > ref.BASE6)) for t in st.values()) == above
        assert st["conv1_1"][n - 1, 31, s - 1, s - 1, s - 1] == v and np.count_nonzero(st["conv1_1"][:, 31]) == 1
