"""Test-side plumbing of tests/test_gpu_simil_layers.py that needs no GPU: the names and shapes of what a similarityNet pass leaves in its
workspace, the references and bounds of the global and the local check, and the two tables - the 2-D counterpart of tests/layer_check.py,
with the same metrics, factors and printing. Everything here works on DECODED tensors (tests/simil_decode.py), so the same functions judge
the device and, in tests/test_simil_layers_cpu.py, a CPU stand-in with planted faults."""
import time

import numpy as np

import simil_decode as sd
from oracle import simil_oracle as so

LAYERS = so.LAYER_NAMES
CHANNELS = dict(zip(LAYERS, (co for _, co in so.CONVS)))
STORED = ["p0"] + LAYERS                              # maps; "feat" and "emb" are plain fp32 rows
POOLS = [LAYERS[i] for i in sorted(so.POOL_AFTER)]    # pool1 .. pool5 under their producers' names
NAMES = LAYERS + ["feat", "emb"]                      # the 15 launches (feat: gather + L2 norm; emb: dense + reduce)
GLOBAL_FACTOR, LOCAL_FACTOR = 4.0, 3.0                # tests/layer_check.py: float32 / fp16-storage class, global; every class, local


def extent(name):
    """Extent of the stored map: 64 >> block, halved again where the block's last layer stores its pooled output."""
    i = LAYERS.index(name)
    st = sum(1 for p in so.POOL_AFTER if p < i)
    return (sd.PATCH >> st) >> (1 if i in so.POOL_AFTER else 0)


def buffer_of(name):
    """The workspace buffer (simil_decode.layout's names) a stored tensor lives in: a block's layers take its ping-pong buffers in turn, its
    last layer writes the pooled map."""
    if name == "p0":
        return "p0"
    i = LAYERS.index(name)
    st = sum(1 for p in so.POOL_AFTER if p < i)
    first = 0 if st == 0 else sorted(so.POOL_AFTER)[st - 1] + 1
    return "pool%d" % (st + 1) if i in so.POOL_AFTER else "a%d%d" % (st, i - first)


def quant_of(precision):
    """The arithmetic class that judges a precision mode: every mode but f16 runs this network in f16x3 (sn_simil.hip simil_mode)."""
    return "fp16" if precision == "f16" else "x3"


def references(X, values, precision):
    """-> (exact, ref): the fp64 oracle's tensors and those of the mode's class reference on the same input (x3: weights, input and stored
    maps as hi + lo pairs of halfs, float32 convolutions; fp16: halfs, wide accumulation), name -> fp64 array."""
    _, exact = so.embedding_torch(X, values, return_intermediates=True)
    q = quant_of(precision)
    _, ref = so.embedding_torch(X, values, dtype="float32" if q == "x3" else "float64", quant=q, return_intermediates=True)
    return exact, ref


def check_p0(value, pad, X, precision):
    """The stored network input against the float32 patches it was made from: channels 0..2 are fp16(x) exactly in f16, and within one
    rounding of the hi + lo pair otherwise (hi + lo carries at least 21 significant bits: |x - (hi + lo)| <= 2^-22 |x|, and nothing below
    the smallest fp16 subnormal's half, 2^-25, is lost to lo's underflow); channels 3..7 are exact zeros in every plane."""
    X64 = np.asarray(X, dtype=np.float64)
    assert value.shape == X64.shape, (value.shape, X64.shape)
    assert pad.shape[2] == 5 and not pad.any(), "p0: padded channels 3..7 are not exact zeros"
    if precision == "f16":
        assert np.array_equal(value, np.asarray(X, dtype=np.float32).astype(np.float16).astype(np.float64)), "p0 is not fp16(x)"
    else:
        err = np.abs(value - X64)
        assert (err <= np.ldexp(np.abs(X64), -22) + 2.0 ** -25).all(), float((err / np.maximum(np.abs(X64), 1e-30)).max())
        assert np.array_equal(value, sd.hilo(X)), "p0 is not the hi + lo pair of x"


def global_table(dec, exact, ref, title, sample_of=None):
    """e_T = max|t - exact| / max|exact| per stored tensor, for the device (dec) and for the class reference; bound = 4 x the reference's.
    sample_of: workspace patch -> input patch (default: identity). Prints the table, returns rows (name, e_dev, e_ref, bound)."""
    rows = []
    print("\n%s\n  %-12s %11s %11s %11s" % (title, "tensor", "e_T device", "reference", "bound"))
    for name in NAMES:
        d = dec[name]
        idx = list(range(d.shape[0])) if sample_of is None else list(sample_of)
        ex, rf = exact[name][idx], ref[name][idx]
        assert d.shape == ex.shape, (name, d.shape, ex.shape)
        den = np.abs(ex).max()
        e_dev, e_ref = np.abs(d - ex).max() / den, np.abs(rf - ex).max() / den
        rows.append((name, float(e_dev), float(e_ref), float(GLOBAL_FACTOR * e_ref)))
        print("  %-12s %11.3e %11.3e %11.3e%s" % (name, e_dev, e_ref, GLOBAL_FACTOR * e_ref, "" if e_dev <= GLOBAL_FACTOR * e_ref else "   <-- FAILS"))
    return rows


def _metric(t, exact, den):
    err = np.abs(t - exact)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(den > 0, err / den, np.where(err > 0, np.inf, 0.0)).max())


def local_table(dec, values, precision, title, only=None):
    """The local check: per launch, the fp64 step applied to the DEVICE's decoded input is the exact answer for what that launch was given;
    metric max |t - exact| / (A + |exact|), A the forward-error scale of the element; bound = 3 x the same metric of the class reference ON
    THE SAME INPUT:
      * the 13 convolutions: simil_oracle.step - A = |W| (*) |x| + |b|, a pooled element the maximum of A over its window; reference: the x3
        class (weights and stored result as hi + lo pairs of halfs, float32 convolution; tests/layer_check.py local_table says why the
        weights cannot stay float32) for every mode but f16, the fp16 class (fp16 weights and stored result, wide accumulation) for f16.
        The weights are rounded as they come, as in net_oracle.step_torch. The packer first scales each output row by a power of two so
        that its largest weight lies in [1, 2); the reference does not, so the lo halves of its weights are fp16 subnormals (|w| < 1/8 for
        every layer here, |w| < 0.007 in s_conv1_1) and ITS error is mostly theirs: about 1.2e-7 per launch, 5e-6 .. 7e-6 in s_conv1_1 -
        where the device measures 6e-8 .. 1.8e-7 - and 3e-6 .. 6e-6 on every GLOBAL row behind it. With the row scaling modelled, the
        float32 convolution alone sits at 9e-8 (s_conv1_2) down to 3e-8 (s_conv5_x) per launch on two patches, below the device's
        1.2e-7 .. 2.6e-7 (three fp16 MFMA chains per product into one fp32 accumulator): a class reference that models the accumulation as well as the operands is the
        follow-up that would sharpen these rows (profiles/simil_layers/README.md);
      * feat (gather of the five stored pools + L2 norm): every element is one product x * (1 / |x|_2), so A = |exact|; reference: the same
        step in float32 on the device's stored pools;
      * emb (dense layer on the device's stored feat): A = |feat| . |W| + |b|; reference: float32.
      The float32 sums of the last two are textbook left-to-right sums (simil_oracle._seq_sum): 5888 terms in one chain, where the device
      adds 8 chains of 736 (dense) resp. 256 threads' partial sums (norm) - the order a library happens to use is no property of float32.
    only: the launches to judge (default: all 15). Prints the table, returns rows (launch, e_dev, e_ref, bound, seconds)."""
    rows = []
    q = quant_of(precision)
    print("\n%s\n  %-12s %11s %11s %11s %6s" % (title, "launch", "device", "reference", "bound", "s"))
    for k, name in enumerate(NAMES):
        if only is not None and name not in only:
            continue
        t0 = time.time()
        if k < 13:
            x = dec["p0"] if k == 0 else dec[LAYERS[k - 1]]
            exact, A = so.step(values, k, x)
            rf = so.step(values, k, x, dtype="float32" if q == "x3" else "float64", quant=q)[0]
        elif name == "feat":
            pools = [dec[p] for p in POOLS]
            exact = so.feat_step(pools)
            A = np.abs(exact)
            rf = so.feat_step(pools, dtype="float32").astype(np.float64)
        else:
            exact, A = so.emb_step(values, dec["feat"], with_scale=True)
            rf = so.emb_step(values, dec["feat"], dtype="float32").astype(np.float64)
        den = A + np.abs(exact)
        e_dev, e_ref = _metric(dec[name], exact, den), _metric(rf, exact, den)
        rows.append((name, e_dev, e_ref, LOCAL_FACTOR * e_ref, time.time() - t0))
        print("  %-12s %11.3e %11.3e %11.3e %6.1f%s" % (name, e_dev, e_ref, LOCAL_FACTOR * e_ref, time.time() - t0, "" if e_dev <= LOCAL_FACTOR * e_ref else "   <-- FAILS"))
    return rows


def failing(g, loc):
    """-> (failing GLOBAL rows, failing LOCAL rows) as printable tuples."""
    return ([(r[0], "%.3e > %.3e" % (r[1], r[3])) for r in g if not r[1] <= r[3]],
            [(r[0], "%.3e > %.3e" % (r[1], r[3])) for r in loc if not r[1] <= r[3]])
