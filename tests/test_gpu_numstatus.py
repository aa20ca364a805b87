"""GPU (-m gpu): the safety net of the parity claim - the error word (SN_ERR_RANGE), the warning word (sn_numeric_status) and the report of
sn_calibrate_dev - held to tests/numstatus_ref.py, the exact restatement of all three as integer functions of the bits the device itself
stored (read back through the test-only twin library, as tests/test_gpu_layers.py does). No tolerance anywhere: every verdict is `==`.
Every test first asserts that what it planted really landed (read back, exact), then judges the words. Nets: tests/numstatus_cases.py;
their preconditions are held to the fp64 oracle by tests/test_numstatus_cpu.py. Figures of the first run: profiles/numstatus/README.md.

Shapes: cube_D 12 (every conv tile partial along every axis, quarter extent 3), 16 (full 8-tiles, a full 16-wide conv1_x tile), 8 / 12 / 32
for the scan (12: the last workgroup of the scan has a tail; 32 with two samples: 6.8 M halfs, past the 2048 x 256 x 8 of one grid-stride pass)."""
import ctypes
import os

import numpy as np
import pytest

import act_decode as ad
import layer_check as lc
import numstatus_cases as nc
import numstatus_ref as ref
import synth

pytestmark = pytest.mark.gpu

PLANS = [("f16x3", None), ("f16x3", 0), ("f16x3", 2), ("f16m8", None)]
PLAN_IDS = ["f16x3", "f16x3-conv4_fp8_0", "f16x3-conv4_fp8_2", "f16m8"]


@pytest.fixture(scope="module")
def sn(gpu_required):
    import surfacenet_amd
    return surfacenet_amd


@pytest.fixture(scope="module")
def dbg(sn):
    from surfacenet_amd import _lib
    lib = ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libsurfacenet_hip_dbg.so"))
    lib.sn_debug_tensor.restype = lib.sn_debug_tensor_info.restype = ctypes.c_int
    lib.sn_debug_tensor.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t]
    lib.sn_debug_tensor_info.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p]
    lib.sn_last_error.restype = ctypes.c_char_p
    return lib


def read_back(ctx, dbg, bufs=None):
    raws, lays = {}, {}
    for buf in (lc.BUFFERS if bufs is None else bufs):
        info = np.zeros(8, dtype=np.int64)
        assert dbg.sn_debug_tensor_info(ctx._h, buf.encode(), info.ctypes.data_as(ctypes.c_void_p)) == 0, dbg.sn_last_error()
        lay = ad.Layout.from_info(info)
        raw = np.empty(lay.nbytes, dtype=np.uint8)
        assert dbg.sn_debug_tensor(ctx._h, buf.encode(), raw.ctypes.data_as(ctypes.c_void_p), raw.nbytes) == 0, dbg.sn_last_error()
        raws[buf], lays[buf] = raw, lay
    return raws, lays


def context(sn, s, max_samples, precision="f16x3", conv4_fp8=None):
    return sn.Context(cube_D=s, max_samples=max_samples, precision=precision, **({} if conv4_fp8 is None else dict(conv4_fp8=conv4_fp8)))


def planes_of(raw, lay, n):
    """The first n samples of every plane of one buffer: the bytes a call of n samples may write."""
    M = lay.max_samples()
    per = lay.extent ** 3 * lay.cs * 2
    offs = [0] + [2 * o for o in (lay.lo, lay.code) if o > 0]
    return [raw[o: o + M * per].reshape(M, per)[:n] for o in offs]


def same_tensors(rawA, rawB, lays, n, what):
    for buf, lay in lays.items():
        for k, (a, b) in enumerate(zip(planes_of(rawA[buf], lay, n), planes_of(rawB[buf], lay, n))):
            assert np.array_equal(a, b), (what, buf, "plane %d" % k)


def channel_bits(raws, lays, layer, n, ch):
    buf = ref.STORE_LAYERS[layer]
    return ref.hi_bits(raws[buf], lays[buf], n, ref.REAL_CHANNELS[buf])[:, ch]


def words(ctx, X, n_vp=1):
    """One forward pass -> (error message or None, warning names as a set, (fused, unfused) or None)."""
    import surfacenet_amd as sn_
    try:
        out = ctx.forward(X, None, n_vp=n_vp)
        err = None
    except sn_.SurfaceNetHipError as e:
        out, err = None, str(e)
    return err, set(ctx.numeric_status()), out


# ------------------------------------------------------------------------------------------------
# calibration, exact
# ------------------------------------------------------------------------------------------------
def check_report(cal, raws, lays, n, frac, s_old, what):
    want = ref.calibration(raws["ma"], lays["ma"], raws["cat"], lays["cat"], n, frac, s_old)
    print("   %-44s device %s" % (what, {k: cal[k] for k in sorted(cal)}))
    assert set(cal) == set(want)
    for k in want:
        assert cal[k] == want[k], (what, k, cal[k], want[k])
    return (cal["s_act"], cal["s_cat"])


CAL_CASES = [(8, 4, [(4, -1.0), (4, 1e-3), (2, 1e-3), (2, 0.0), (4, -1.0)]), (12, 1, [(1, 1e-3), (1, 0.0), (1, -1.0)]), (32, 2, [(2, 1e-3)])]


@pytest.mark.parametrize("s,n,calls", CAL_CASES, ids=["8x4", "12x1-tail", "32x2-second-pass"])
def test_calibration_report_is_the_scan_of_the_stored_bits(sn, dbg, s, n, calls):
    """The x3.2 stress form of test_gpu_numerics (merge_conv_a's inv_std x 3.2: a few % of its outputs beyond 7.5). Every report equals the
    restatement on the read-back, field for field; the exponents in force carry from one call to the next (a negative bound changes none)."""
    values = [np.array(v) for v in synth.calibrated_params(1)]      # (the net every other test of this file starts from: computed once)
    values[nc.IX[("merge_conv_a", "inv_std")]] *= np.float32(3.2)
    X = synth.random_cvc(n, s, 31)
    vec = n * s ** 3 * 104 // 8
    if s == 12:
        assert vec % 256 != 0                        # the last workgroup has a tail
    if s == 32:
        assert 2048 * 256 < vec < 2 * 2048 * 256     # a second, partial pass of the grid-stride loop
    with context(sn, s, n) as ctx:
        ctx.load_param_values(values)
        ctx.forward(X, None, n_vp=1)
        raws, lays = read_back(ctx, dbg, ("ma", "cat"))
        s_old = (0, 2)                               # sn_consts.h SN_MX_S_ACT, SN_MX_S_CAT
        assert (127 - lays["ma"].e8, 127 - lays["cat"].e8) == s_old
        for k, frac in calls:
            cal = ctx.calibrate(k, max_sat_fraction=frac)
            s_new = check_report(cal, raws, lays, k, frac, s_old, "cube_D %d, %d of %d samples, bound %g" % (s, k, n, frac))
            assert frac >= 0 or s_new == s_old
            s_old = s_new


def test_calibration_thresholds_are_strict_and_an_all_zero_tensor_says_nothing(sn, dbg):
    """Thirteen dead channels of merge_conv_a store exactly lim * 2^k, k = -6 .. 6, thirteen more the next fp16 above each: whether bin j counts
    a whole channel hangs on its `>`. Then merge_conv_a all dead: exponent kept, fractions and maximum 0.0."""
    s, n = 8, 2
    X = synth.random_cvc(n, s, 33)
    values = nc.base_values()
    lim = [float(np.ldexp(ref.BASE6, k)) for k in range(-6, 7)]
    for i, v in enumerate(lim):
        nc.dead(values, "merge_conv_a", i, v)
        nc.dead(values, "merge_conv_a", 13 + i, nc.next_f16(v))
    with context(sn, s, n) as ctx:
        ctx.load_param_values(values)
        err, warn, _ = words(ctx, X)
        raws, lays = read_back(ctx, dbg)
        for i, v in enumerate(lim):
            assert (channel_bits(raws, lays, "merge_conv_a", n, i) == ref.f16_bits(v)).all()
            assert (channel_bits(raws, lays, "merge_conv_a", n, 13 + i) == ref.f16_bits(v) + 1).all()
        assert err is None and warn == ref.warning_names(raws, lays, n, "f16x3", None, lc.storage("f16x3")[0], gone={"conv4_1": False}) == {"merge_conv_a"}
        counts, nz, mx = ref.scan(ref.hi_bits(raws["ma"], lays["ma"], n, 100))
        vox = n * s ** 3
        # thr[j] = lim * 2^(6 - j): j of the channels at a threshold store more than it, j + 1 of those one fp16 above; the 74 tame channels stay
        # below 7.5 = thr[6] (test_numstatus_cpu.py), so down to there the count is the planted channels' alone
        for j in range(13):
            assert counts[j] >= vox * (2 * j + 1) and (j > 6 or counts[j] == vox * (2 * j + 1)), (j, counts[j])
        s_old = check_report(ctx.calibrate(n, -1.0), raws, lays, n, -1.0, (0, 2), "threshold case, measure only")
        check_report(ctx.calibrate(n, 0.3), raws, lays, n, 0.3, s_old, "threshold case, bound 0.3")
        for ch in range(100):
            nc.dead(values, "merge_conv_a", ch, 0.0)
        ctx.load_param_values(values)
        err, warn, _ = words(ctx, X)
        raws, lays = read_back(ctx, dbg)
        assert err is None and warn == set() and not raws["ma"][: n * s ** 3 * 104 * 2].any()
        cal = ctx.calibrate(n, 1e-3)
        check_report(cal, raws, lays, n, 1e-3, (0, 2), "merge_conv_a all dead")
        assert (cal["s_act"], cal["sat_act"], cal["sat_act_before"], cal["max_act"]) == (0, 0.0, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------
# warning word, exact, at partial tiles
# ------------------------------------------------------------------------------------------------
def _limited(precision, conv4_fp8):
    return ref.limited_layers(precision, conv4_fp8, lc.storage(precision, conv4_fp8)[0])


# (cube_D, precision, conv4_fp8, layer): every layer the plan's launcher gives a limit, in turn; layer None: the tame net
WARN_CASES = [(s, p, c4, layer) for (p, c4) in PLANS for s in (12, 16) for layer in [None] + sorted(_limited(p, c4))]


@pytest.mark.parametrize("s,precision,conv4_fp8,layer", WARN_CASES, ids=["%d-%s-%s" % (c[0], PLAN_IDS[PLANS.index(c[1:3])], c[3] or "tame") for c in WARN_CASES])
def test_warning_word_names_exactly_the_layers_whose_stored_bits_exceed_their_limit(sn, dbg, s, precision, conv4_fp8, layer):
    """The tame net (empty set); per limited layer, its last real channel (99 of merge_conv_a, 299 of the conv4 chain, ...) dead at the first
    fp16 above the limit - the layer, and it alone, must be named - and at half that: it must not. The last real channel shares its
    16-channel fragment with padded lanes wherever the layer has any. Two samples: the planted channel also fills the last one."""
    n = 2
    X = synth.random_cvc(n, s, 40 + s)
    fmt = lc.storage(precision, conv4_fp8)[0]
    limited = _limited(precision, conv4_fp8)
    quiet = {k: False for k in limited if k not in ref.SURVIVES}
    bufs = sorted({ref.STORE_LAYERS[k] for k in ref.SURVIVES})
    plan = PLAN_IDS[PLANS.index((precision, conv4_fp8))]
    with context(sn, s, n, precision, conv4_fp8) as ctx:
        def run(values, gone, what):
            ctx.load_param_values(values)
            assert ctx.numeric_status() == []
            err, warn, _ = words(ctx, X)
            raws, lays = read_back(ctx, dbg, bufs)
            want = ref.warning_names(raws, lays, n, precision, conv4_fp8, fmt, gone=gone)
            print("   cube_D %d %s: %-40s device %s restatement %s" % (s, plan, what, sorted(warn), sorted(want)))
            assert err is None and ref.error_expected(raws, lays, n) == set(), (what, err)
            assert warn == want, (what, warn, want)
            return raws, lays, warn

        if layer is None:
            assert run(nc.base_values(), quiet, "tame")[2] == set()
            return
        buf = ref.STORE_LAYERS[layer]
        ch = nc.COUT[layer] - 1
        for named in (True, False):
            lb = ref.limit_bits(limited[layer], lc.storage(precision, conv4_fp8)[1][buf])
            v = ref.bits_f16(lb + 1) * (1.0 if named else 0.5)
            raws, lays, warn = run(nc.dead(nc.base_values(), layer, ch, v), dict(quiet, **({layer: named} if layer in quiet else {})),
                                   "%s channel %d = %r" % (layer, ch, v))
            assert lb == ref.limit_bits(limited[layer], lays[buf].e8)          # (the exponent the library reports is the documented one)
            if layer in ref.SURVIVES:
                assert (channel_bits(raws, lays, layer, n, ch) == ref.f16_bits(v)).all(), (layer, v)
                assert ref.stored_max_bits(raws[buf], lays[buf], n, ref.REAL_CHANNELS[buf])[0] == ref.f16_bits(v) or not named
            assert warn == ({layer} if named else set()), (layer, v, warn)


@pytest.mark.parametrize("s", [12, 16])
def test_one_value_in_the_far_corner_of_the_last_sample(sn, dbg, s):
    """f16m8: conv1_1's channel 31 copies input plane 0 through its centre tap; the plane is zero but for voxel (s-1, s-1, s-1) of the LAST
    sample, the first fp16 above 7.5. Exactly one stored value of the whole pass exceeds a limit, in the far corner of a partial tile (12)
    / of the last tile (16); one fp16 lower, none does."""
    n = 2
    values = nc.spike_net(nc.base_values())
    fmt = lc.storage("f16m8")[0]
    quiet = {"conv3_1": False, "conv4_1": False}
    with context(sn, s, n, "f16m8") as ctx:
        ctx.load_param_values(values)
        for k, named in ((1, True), (0, False)):
            v = ref.bits_f16(ref.limit_bits(ref.BASE6, 127) + k)
            X = synth.random_cvc(n, s, 40 + s)
            X[:, 0] = 0.0
            X[n - 1, 0, s - 1, s - 1, s - 1] = v
            err, warn, _ = words(ctx, X)
            raws, lays = read_back(ctx, dbg)
            b = channel_bits(raws, lays, "conv1_1", n, 31)
            assert int(np.count_nonzero(b)) == 1 and int(b[n - 1, s - 1, s - 1, s - 1]) == ref.f16_bits(v)
            mx, where = ref.stored_max_bits(raws["a1"], lays["a1"], n, 32)
            assert (mx, where) == (ref.f16_bits(v), (n - 1, 31, s - 1, s - 1, s - 1))
            above = int(np.count_nonzero(ref.hi_bits(raws["a1"], lays["a1"], n, 32) > ref.limit_bits(ref.BASE6, 127)))
            assert above == (1 if named else 0)
            want = ref.warning_names(raws, lays, n, "f16m8", None, fmt, gone=quiet)
            print("   cube_D %d: spike %r at the far corner of sample %d: device %s restatement %s" % (s, v, n - 1, sorted(warn), sorted(want)))
            assert err is None and warn == want == ({"conv1_1"} if named else set())


# ------------------------------------------------------------------------------------------------
# words that speak of nothing stored
# ------------------------------------------------------------------------------------------------
PROBES = [(12, p, layer, c) for p in ("f16x3", "f16m8") for layer in ("conv1_2", "conv2_2", "conv4_2", "merge_conv_a") for c in (0, nc.COUT[layer] - 1)]
# cube_D 32, one sample: conv4_2's one tile (extent 8) is full, so the only lanes without a store are its padded channels' (300 of 320) - the
# padded-lane case on its own, in the f16m8 plan's conv4 kernel (no LDS constant table) and in the default plan's
PROBES += [(32, p, "conv4_2", 0) for p in ("f16x3", "f16m8")]


@pytest.mark.parametrize("s,precision,layer,c", PROBES, ids=["%d-%s-%s-ch%d" % p for p in PROBES])
def test_lanes_that_store_nothing_raise_no_word(sn, dbg, s, precision, layer, c):
    """cube_D 12: every tile of every layer is partial (extents 12, 6, 3), so every tile has fragment lanes whose voxel lies outside the volume;
    conv4_2 (300 of 320 lanes) and merge_conv_a (100 of 112) have padded channel lanes besides, which read channel 0's constants in the store
    kernels without an LDS constant table. The probe channel stores 0 at every voxel and would store B on all-zero input: B = 4 x the layer's
    warning limit must leave the warning word empty, B = 1e5 (an fp16 inf if it were stored) must leave the call valid, and in both cases every
    stored tensor and the output equal those of the same net with B = 0, bit for bit."""
    n = 2 if s == 12 else 1
    X = synth.random_cvc(n, s, 40 + s)
    fmt = lc.storage(precision)[0]
    limited = ref.limited_layers(precision, None, fmt)
    quiet = {k: False for k in limited if k not in ref.SURVIVES}
    Bs = [0.0] + ([4.0 * limited[layer]] if layer in limited else []) + [1e5]
    first = None
    with context(sn, s, n, precision) as ctx:
        for B in Bs:
            values = nc.base_values()
            p = nc.probe(values, layer, c, B)
            ctx.load_param_values(values)
            err, warn, out = words(ctx, X)
            raws, lays = read_back(ctx, dbg)
            print("   cube_D %d %s %s channel %d, zero-input value %g: error %s, warning %s" % (s, precision, layer, c, B, err, sorted(warn)))
            # what was planted landed: the producer channel is the constant, the probe channel stores nothing but zeros
            if layer == "merge_conv_a":
                cat = ref.hi_bits(raws["cat"], lays["cat"], n, 64)[:, 15]
                assert (cat == ref.f16_bits(p)).all()
            elif nc.PRODUCER[layer] in ref.SURVIVES:      # (conv4_1's tensor is overwritten by conv4_3: were its constant missing, the probe channel would store B)
                assert (channel_bits(raws, lays, nc.PRODUCER[layer], n, nc.COUT[nc.PRODUCER[layer]] - 1) == ref.f16_bits(p)).all()
            assert not channel_bits(raws, lays, layer, n, c).any()
            assert ref.error_expected(raws, lays, n) == set()
            assert err is None, "a valid call failed on a value no lane stored: %s" % err
            assert warn == ref.warning_names(raws, lays, n, precision, None, fmt, gone=quiet) == set(), (B, warn)
            if first is None:
                first = (raws, out)
            else:
                same_tensors(first[0], raws, lays, n, "B = %g against B = 0" % B)
                assert np.array_equal(first[1][1], out[1])


# ------------------------------------------------------------------------------------------------
# after a flagged call
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x3", "f16m8"])
def test_a_smaller_batch_after_a_flagged_call_reads_no_stale_inf(sn, dbg, precision):
    """cube_D 12, max_samples 4: a 4-sample batch whose last sample is 1e6 everywhere fails, naming conv1_1, and leaves inf in the workspace. The
    next call - one tame sample - returns, with clean words, the output and the stored tensors of a fresh context, bit for bit; twice (the
    second time with samples 1 .. 3 all huge)."""
    s, M = 12, 4
    values = nc.base_values()
    X = synth.random_cvc(M, s, 61)
    bad = X.copy()
    bad[M - 1] = 1e6
    fmt = lc.storage(precision)[0]
    quiet = {k: False for k in ref.limited_layers(precision, None, fmt) if k not in ref.SURVIVES}
    with context(sn, s, M, precision) as ctx:
        ctx.load_param_values(values)
        err, _, out0 = words(ctx, X[:1])
        fresh, lays = read_back(ctx, dbg)
        assert err is None
    with context(sn, s, M, precision) as ctx:
        ctx.load_param_values(values)
        for turn in range(2):
            if turn == 1:
                bad[1:] = 1e6                        # (second turn: the samples next to the one the small batch rewrites hold the stale values too)
            err, _, _ = words(ctx, bad)
            assert err is not None and "conv1_1" in err, err
            raws, _ = read_back(ctx, dbg)
            assert all(layer in err for layer in ref.error_expected(raws, lays, M))
            x0 = ref.hi_bits(raws["x0"], lays["x0"], M, 6)
            assert (x0[M - 1] == ref.INF_BITS).all() and not (x0[0] >= ref.INF_BITS).any()      # the workspace does hold inf, not in sample 0
            err, warn, out = words(ctx, X[:1])
            raws, _ = read_back(ctx, dbg)
            print("   %s, turn %d after the flagged batch: error %s, warning %s" % (precision, turn, err, sorted(warn)))
            assert err is None, err
            assert warn == ref.warning_names(raws, lays, 1, precision, None, fmt, gone=quiet) == set()
            same_tensors(fresh, raws, lays, 1, "after a flagged call")
            assert np.array_equal(out[1], out0[1]) and np.array_equal(out[0], out0[0])


def test_similaritynet_after_a_flagged_call(sn):
    """The 2-D form of the same kernels, where the x axis of a tile is the patch index (no halo along it: a lane beyond the last patch reads
    what an earlier batch left there): 9 float patches with one huge fail at the next sn_synchronize (the float-patch entry reports the error
    word there), naming the first layer; the next call, 1 patch, passes its synchronize with clean words and returns the embedding of a
    fresh context, bit for bit; twice."""
    from surfacenet_amd import weights
    values = weights.synthetic_simil_param_values(1)
    rs = np.random.RandomState(5)
    P = (rs.rand(9, 3, 64, 64).astype(np.float32) - 0.5) * 200.0
    bad = P.copy()
    bad[8] = 1e30
    with context(sn, 8, 2) as ctx:
        ctx.load_simil_param_values(values)
        e1 = ctx.patch2embedding(P[:1])
        e9 = ctx.patch2embedding(P)
    assert np.isfinite(e9).all() and np.array_equal(e9[:1], e1)
    with context(sn, 8, 2) as ctx:
        ctx.load_simil_param_values(values)
        for turn in range(2):
            ctx.patch2embedding(bad)
            with pytest.raises(sn.SurfaceNetHipError, match="s_conv1_1"):
                ctx.synchronize()
            got = ctx.patch2embedding(P[:1])
            ctx.synchronize()                        # (raises if the one-patch run flagged anything)
            assert np.array_equal(got, e1), "turn %d" % turn
            assert ctx.numeric_status() == []


SIMIL_PROBES = [(i, n, c) for i in (0, 12) for n in (1, 9) for c in ("first", "last")]


@pytest.mark.parametrize("i,n,c", SIMIL_PROBES, ids=["%s-n%d-%s" % (("s_conv1_1", "s_conv5_3")[p[0] > 0], p[1], p[2]) for p in SIMIL_PROBES])
def test_similaritynet_lanes_beyond_the_last_patch_raise_no_word(sn, i, n, c):
    """The probe channel in the similarityNet's first (s_conv1_1: store epilogue, 8 patches per tile) and last convolution (s_conv5_3: pooled
    store epilogue, 16 images per tile) at 1 and 9 patches - a partial tile along the patch axis either way. conv + bias + ReLU: the
    producer channel stores 1 (s_conv1_1: input plane 0 is 1), the probe channel has the centre tap -2^18 on it and bias 1e5: it stores 0
    at every pixel of every patch and would store 1e5 - an fp16 inf - on all-zero input. The call and its synchronize must pass, the
    embedding equal that of the same net with bias 0, bit for bit."""
    from surfacenet_amd import weights
    rs = np.random.RandomState(7)
    P = (rs.rand(n, 3, 64, 64).astype(np.float32) - 0.5) * 200.0
    P[:, 0] = 1.0
    emb = []
    with context(sn, 8, 2) as ctx:
        for B in (0.0, 1e5):
            values = [np.array(v) for v in weights.synthetic_simil_param_values(1)]
            j = 0
            if i > 0:                                # the producer channel: the last one of the layer in front, W = 0, bias 1
                j = values[2 * (i - 1)].shape[0] - 1
                values[2 * (i - 1)][j] = 0.0
                values[2 * (i - 1) + 1][j] = 1.0
            ch = 0 if c == "first" else values[2 * i].shape[0] - 1
            values[2 * i][ch] = 0.0
            values[2 * i][ch, j, 1, 1] = -nc.PROBE_K
            values[2 * i + 1][ch] = B
            ctx.load_simil_param_values(values)
            emb.append(ctx.patch2embedding(P))
            ctx.synchronize()                        # SN_ERR_RANGE, if a lane that stores nothing raised the error word
            assert ctx.numeric_status() == []
    assert np.isfinite(emb[0]).all() and np.array_equal(emb[0], emb[1])
