"""Test-side plumbing of tests/test_gpu_layers.py that needs no GPU: which oracle tensor each workspace buffer holds after a forward pass
of the (fused) plan, the references and bounds of the global and the local check, and the two tables. Everything here works on DECODED
tensors (tests/act_decode.py), so the same functions judge the device and, as a sanity check of the harness, the CPU model itself."""
import time

import numpy as np

import act_decode as ad
from oracle import net_emulation, net_oracle

# buffer -> (oracle tensor it holds after a pass of the fused plan, real channels, the ReLU layer whose renormalisation exponents it carries)
# (a1 / a3 / a4 are written twice in a pass: what survives is the LAST write - conv1_1 (conv1_3's output is never stored), conv3_3, conv4_3)
BUFFERS = {
    "x0": ("x", 6, None), "a1": ("conv1_1", 32, "conv1_1"), "b1": ("conv1_2", 32, "conv1_2"), "cat": ("cat", 64, None),
    "p1": ("pool1", 32, "conv1_3"), "a2": ("conv2_1", 80, "conv2_1"), "b2": ("conv2_2", 80, "conv2_2"), "s2": ("side2_pre", 16, None),
    "p2": ("pool2", 80, "conv2_3"), "a3": ("conv3_3", 160, "conv3_3"), "b3": ("conv3_2", 160, "conv3_2"), "a4": ("conv4_3", 300, "conv4_3"),
    "b4": ("conv4_2", 300, "conv4_2"), "s3": ("side3_pre", 16, None), "s4": ("side4_pre", 16, None), "ma": ("merge_a", 100, "merge_conv_a"),
}
PADDED = ("x0", "a4", "b4", "ma")          # channel stride > channels: 6 -> 8, 300 -> 304, 100 -> 104
# Default mode: the outputs whose step runs an MX product or that are stored with a code plane - their reference is the CPU model; the others
# (hi + lo operands, three fp16 MFMAs, hi + lo storage) are judged against a float32 convolution.
MX_OUTPUTS = {"side1", "conv3_3", "conv4_2", "conv4_3", "cat48", "merge_a", "out"}

def decode_all(raws, lays, values, S, unfused):
    """raws / lays: buffer -> raw bytes / act_decode.Layout. Returns (dec, pads): dec oracle name -> (S, C, D, D, D) fp64 as the readers
    see it ("conv3_3": what conv4_1 reads, "conv3_3_x3": what side_op3 reads; "side1" / "cat48": the two halves of the concat buffer;
    "out": the unfused probabilities), pads buffer -> its padded channels."""
    P = net_oracle.params_to_dict(values)
    dec, pads, extras = {}, {}, {}
    for buf, (name, C, relu) in BUFFERS.items():
        oe = net_emulation.renorm_exponents(P[relu]) if relu else None
        v, pad, extra = ad.decode(raws[buf], lays[buf], S, C, oe=oe, view="code" if buf == "a3" else None)
        dec[name], pads[buf], extras[buf] = v, pad, extra
        if buf == "a3":
            dec["conv3_3_x3"] = ad.decode(raws[buf], lays[buf], S, C, oe=oe, view="lo")[0] if lays[buf].fmt == ad.FMT_HILO_M8 else v
    dec["side1"], dec["cat48"] = dec["cat"][:, :16], dec["cat"][:, 16:]
    s = unfused.shape[-1]
    dec["out"] = np.asarray(unfused, dtype=np.float64).reshape(-1, 1, s, s, s)[:S]
    return dec, pads, extras


def references(X, values, precision):
    """-> (exact, ref, factor): the fp64 oracle's tensors, the tensors of the reference of the precision mode's arithmetic class on the same
    input (the CPU model for the MX-assisted modes, the float32 oracle for f16x3p, the fp16-storage oracle for f16), and the factor on that
    reference's own error that bounds the device's."""
    s = X.shape[-1]
    _, u64, exact = net_oracle.forward_torch(X, values, return_intermediates=True)
    if precision in ("f16x3", "f16m8"):
        _, u, ref = net_emulation.forward_emulated(X, values, mode=precision, return_intermediates=True)
        factor = 3.0
    else:
        kw = dict(dtype="float32") if precision == "f16x3p" else dict(quant="fp16")
        _, u, ref = net_oracle.forward_torch(X, values, return_intermediates=True, **kw)
        ref = {k: np.asarray(v, dtype=np.float64) for k, v in ref.items()}
        # (the network input is not computed: its reference is the class's storage of X - hi + lo halfs resp. one half)
        hi = X.astype(np.float16).astype(np.float32)
        ref["x"] = (hi.astype(np.float64) + (X - hi).astype(np.float16).astype(np.float64)) if precision == "f16x3p" else hi.astype(np.float64)
        ref["conv3_3_x3"] = ref["conv3_3"]
        factor = 4.0
    for d, u_ in ((exact, u64), (ref, u)):
        d["x"] = d.get("x", np.asarray(X, dtype=np.float64))
        d["conv3_3_x3"] = d.get("conv3_3_x3", d["conv3_3"])
        d["out"] = np.asarray(u_, dtype=np.float64).reshape(-1, 1, s, s, s)
    return exact, ref, factor


GLOBAL_NAMES = [v[0] for v in BUFFERS.values()] + ["conv3_3_x3", "out"]


def global_table(dec, exact, ref, factor, title, sample_of=None):
    """e_T = max|t - exact| / max|exact| per stored tensor, for the device (dec) and for the reference; bound = factor * the reference's.
    sample_of: workspace sample -> input sample (default: identity). Prints the table, returns the rows (name, e_dev, e_ref, bound)."""
    rows = []
    print("\n%s\n  %-12s %11s %11s %11s" % (title, "tensor", "e_T device", "reference", "bound"))
    for name in GLOBAL_NAMES:
        d = dec[name]
        idx = list(range(d.shape[0])) if sample_of is None else list(sample_of)
        ex, rf = exact[name][idx], ref[name][idx]
        assert d.shape == ex.shape, (name, d.shape, ex.shape)
        den = np.abs(ex).max()
        e_dev, e_ref = np.abs(d - ex).max() / den, np.abs(rf - ex).max() / den
        rows.append((name, float(e_dev), float(e_ref), float(factor * e_ref)))
        print("  %-12s %11.3e %11.3e %11.3e%s" % (name, e_dev, e_ref, factor * e_ref, "" if e_dev <= factor * e_ref else "   <-- FAILS"))
    return rows


def _metric(t, exact, den):
    err = np.abs(t - exact)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(den > 0, err / den, np.where(err > 0, np.inf, 0.0)).max())


def local_table(dec, values, precision, title, steps=None):
    """The local check: per step of net_oracle.STEPS, the fp64 oracle's step applied to the DEVICE's decoded input is the exact answer for what
    that one launch (or fused group) was given; metric max |t - exact| / (A + |exact|) with A the forward-error scale of the element
    (net_oracle.step_torch); the same metric of the arithmetic class's reference ON THE SAME INPUT, times 3, is the bound:
      * an output whose step multiplies on an MX MFMA or that is stored with a code plane (MX_OUTPUTS in the default mode, everything in
        f16m8): the CPU model's per-layer step (net_emulation.layer_step);
      * an x3 output (hi + lo operands, hi + lo storage): a float32 torch convolution of the class's operands - weights and stored results as
        hi + lo pairs of halfs. (With the weights left in float32 the bound is not one ANY implementation of the design can meet: the design
        represents a weight and a stored value to 2^-22, float32 to 2^-24, and the design's own CPU model - exact accumulation - already sits
        at 2.8 .. 6 times the plain float32 figure: conv1_2 1.9e-7 vs 6.8e-8, conv2_2 1.8e-7 vs 4.4e-8, conv3_1+conv3_2 5.3e-9 vs 8.8e-10, s = 8.)
      * f16: the fp16-storage oracle's step (fp16 weights and stored results, wide accumulation).
    Prints the table, returns rows (step, output, e_dev, e_ref, bound, seconds)."""
    rows = []
    print("\n%s\n  %-26s %-11s %11s %11s %11s %6s" % (title, "step", "output", "device", "reference", "bound", "s"))
    for step, (ins, outs) in net_oracle.STEPS.items():
        if steps is not None and step not in steps:
            continue
        t0 = time.time()
        xin = [dec[n] for n in ins]
        exact, A = net_oracle.step_torch(values, step, xin)
        want_emu = precision == "f16m8" or (precision == "f16x3" and any(o in MX_OUTPUTS for o in outs))
        want_f32 = precision == "f16x3p" or (precision == "f16x3" and any(o not in MX_OUTPUTS for o in outs))
        emu = net_emulation.layer_step(values, step, xin, mode=precision) if want_emu else None
        f32 = net_oracle.step_torch(values, step, xin, dtype="float32", quant="x3")[0] if want_f32 else None
        f16 = net_oracle.step_torch(values, step, xin, quant="fp16")[0] if precision == "f16" else None
        for k, o in enumerate(outs):
            den = A[k] + np.abs(exact[k])
            rf = f16[k] if precision == "f16" else (emu[k] if (precision == "f16m8" or (precision == "f16x3" and o in MX_OUTPUTS)) else f32[k])
            e_dev, e_ref = _metric(dec[o], exact[k], den), _metric(rf, exact[k], den)
            rows.append((step, o, e_dev, e_ref, 3.0 * e_ref, time.time() - t0))
            print("  %-26s %-11s %11.3e %11.3e %11.3e %6.1f%s" % (step, o, e_dev, e_ref, 3.0 * e_ref, time.time() - t0, "" if e_dev <= 3.0 * e_ref else "   <-- FAILS"))
    return rows
