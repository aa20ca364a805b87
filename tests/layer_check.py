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
# The six SurfaceNet plans build_plan_t (surfacenet_amd/csrc/sn_api.hip) can select, as (precision, conv4_fp8) - the keys of tests/golden/conv_plan.json.
# conv4_fp8 is a setting of f16x3 alone (1: conv4_1 .. conv4_3 on the fp8 MX step, the default; 2: conv4_2 and conv4_3 only; 0: none).
PLANS = (("f16x3", 1), ("f16x3", 0), ("f16x3", 2), ("f16x3p", 0), ("f16m8", 0), ("f16", 0))


def plan_key(precision, conv4_fp8=None):
    """(precision, conv4_fp8) as conv_plan.json names the plan: None = the mode's default (1 in f16x3, 0 elsewhere), True / False as Context takes them."""
    c4 = (1 if precision == "f16x3" else 0) if conv4_fp8 is None else int(conv4_fp8)
    assert (precision, c4) in PLANS, (precision, conv4_fp8)
    return precision, c4


def mx_outputs(precision, conv4_fp8=None):
    """The outputs of net_oracle.STEPS whose step multiplies on an MX MFMA or that are stored with a code plane in that plan - their reference
    is the CPU model; the others of f16x3 (hi + lo operands, three fp16 MFMAs, hi + lo storage) are judged against a float32 convolution.
    DESIGN.md section 5 / build_plan_t: in every f16x3 plan the concat buffer (side1, cat48) and merge_conv_a's output are stored with 6-bit
    code slots and merge_conv_a / merge_conv_b multiply on the MX step; conv4_fp8 = 2 adds conv4_2 and conv4_3 (fp8 step; conv4_1, x3
    arithmetic, stores hi + codes inside the step conv4_1+conv4_2); conv4_fp8 = 1 adds conv4_1, hence conv3_3 stored with a code plane.
    f16m8: every output. f16x3p / f16: none (no MX step, no code plane)."""
    precision, c4 = plan_key(precision, conv4_fp8)
    if precision == "f16m8":
        return {o for _, outs in net_oracle.STEPS.values() for o in outs}
    if precision != "f16x3":
        return set()
    tail = {"side1", "cat48", "merge_a", "out"}
    return tail | {0: set(), 1: {"conv3_3", "conv4_2", "conv4_3"}, 2: {"conv4_2", "conv4_3"}}[c4]


def format_table(precision, conv4_fp8=None):
    """The CPU model's per-layer correction-format table of that plan (net_emulation._model's `table`; None: the mode's own)."""
    precision, c4 = plan_key(precision, conv4_fp8)
    if precision != "f16x3" or c4 == 1:
        return None
    return dict(net_emulation.LAYER_FORMATS_R4) if c4 == 0 else dict(net_emulation.LAYER_FORMATS_DEFAULT, conv4_1="x3")


def storage(precision, conv4_fp8=None):
    """-> (fmt, e8): buffer -> storage format of its LAST write in a pass (act_decode.FMT_*), buffer -> E8M0 exponent 127 - s its tensor-table
    row carries - what the plan is documented to store (DESIGN.md sections 3 and 5, build_plan_t), not what a device reports.
      f16 / f16x3p / f16m8: every buffer in the operand mode's format (one half | hi + lo | hi + 6-bit slots).
      f16x3: hi + lo, except the concat buffer and merge_conv_a's output (6-bit slots: the merge layers' MX step reads them) and, by conv4_fp8:
        1: a3 = conv3_3 with hi, lo AND fp8 slots (side_op3 / conv4_1), b4 = conv4_2 hi + fp8 slots, a4 = conv4_3 hi + lo (side_op4 reads it);
        2: b4 as under 1; a3 = conv3_3 plain hi + lo (conv4_1 reads x3); a4 is written hi + fp8 slots by conv4_1 and LAST hi + lo by conv4_3;
        0: a3, a4, b4 hi + lo.
    Exponents (mx_format.h: s = 0 activations, 2 concat buffer, -5 network input, 0 the conv4 chain's fp8 planes): cat 125, x0 132, every other
    127 - a3 / a4 / b4 whether their row names the chain's exponent (conv4_fp8 = 1, 2) or the activations' (0: `e8 = MX_C4` is skipped)."""
    precision, c4 = plan_key(precision, conv4_fp8)
    if precision != "f16x3":
        fmt = dict.fromkeys(BUFFERS, {"f16": ad.FMT_F16, "f16x3p": ad.FMT_HILO, "f16m8": ad.FMT_M6}[precision])
    else:
        fmt = dict(dict.fromkeys(BUFFERS, ad.FMT_HILO), cat=ad.FMT_M6, ma=ad.FMT_M6)
        fmt.update({0: {}, 1: dict(a3=ad.FMT_HILO_M8, b4=ad.FMT_M8), 2: dict(b4=ad.FMT_M8)}[c4])
    e8 = dict(dict.fromkeys(BUFFERS, 127), cat=125, x0=132)
    return fmt, e8


def tile_classes(extent, T, R):
    """The tile / halo cases ConvKernel::launch meets along one axis of `extent` voxels cut into tiles of T with a halo of radius R - labels:
      "only tile partial"            extent < T: one tile, partial, no neighbour
      "one full tile"                exactly one full tile (T <= extent < 2 T): no seam between two full tiles
      "several full tiles"           extent >= 2 T: a seam with a full tile on either side
      "interior tile"                three tiles or more: a tile with a neighbour on both sides
      "partial behind full, rem == R" / "partial behind full, rem > R"    extent > T, extent % T = rem > 0: the last tile is partial and stages a
                                     full neighbour's rows; rem == R is the smallest the launch accepts (its neighbour's halo is the whole tile)
    Raises ValueError for 0 < rem < R behind a full tile, which ConvKernel::launch (and sn_create, for the dilated layers) refuses."""
    assert extent > 0 and T > 0 and R > 0
    full, rem = divmod(extent, T)
    if full == 0:
        return {"only tile partial"}
    if 0 < rem < R:
        raise ValueError("extent %d: a %d-voxel partial tile behind a full one under a halo of %d" % (extent, rem, R))
    out = {"one full tile" if full == 1 else "several full tiles"}
    if full + (rem > 0) >= 3:
        out.add("interior tile")
    if rem:
        out.add("partial behind full, rem == R" if rem == R else "partial behind full, rem > R")
    return out


def level_axes(s):
    """cube_D s -> [(level, extent, T, R)]: the axes the 3-D net's 3x3x3 kernels tile - levels 0, 1, 2 at s, s/2, s/4 with halo radius 1, 1, 2
    (the dilated chain) in 8-voxel tiles, and level 0 once more in the 16-voxel tiles conv1_x takes along x."""
    return [(0, s, 8, 1), (0, s, 16, 1), (1, s // 2, 8, 1), (2, s // 4, 8, 2)]


def check_padding(pads, extras, lays):
    """The padded channels of every plane are exact zeros. pads / extras: act_decode.decode's second and third result per buffer."""
    for buf, pad in pads.items():
        assert np.isfinite(pad).all(), buf
        assert pad.shape[1] == (lays[buf].cs - BUFFERS[buf][1])
        # their producers write them as exact zeros (zero weight rows, zero folded scale and shift; the CVC warp / upload zero channels 6, 7)
        assert not pad.any(), (buf, float(np.abs(pad).max()))
        C = BUFFERS[buf][1]
        for k in ("hi", "hi_code", "lo_code"):
            if k in extras[buf]:
                assert np.isfinite(extras[buf][k]).all() and not extras[buf][k][:, C:].any(), (buf, k)
    assert set(b for b in pads if pads[b].shape[1]) == set(PADDED)


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


def references(X, values, precision, conv4_fp8=None):
    """-> (exact, ref, factor): the fp64 oracle's tensors, the tensors of the reference of the plan's arithmetic class on the same input (the
    CPU model with the plan's format table for the MX-assisted modes, the float32 oracle for f16x3p, the fp16-storage oracle for f16), and
    the factor on that reference's own error that bounds the device's."""
    s = X.shape[-1]
    _, u64, exact = net_oracle.forward_torch(X, values, return_intermediates=True)
    if precision in ("f16x3", "f16m8"):
        _, u, ref = net_emulation.forward_emulated(X, values, mode=precision, table=format_table(precision, conv4_fp8), return_intermediates=True)
        factor = 3.0
    else:
        plan_key(precision, conv4_fp8)
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


def global_table(dec, exact, ref, factor, title, sample_of=None, names=None):
    """e_T = max|t - exact| / max|exact| per stored tensor, for the device (dec) and for the reference; bound = factor * the reference's.
    sample_of: workspace sample -> input sample (default: identity); names: the tensors to judge (default: all of GLOBAL_NAMES). Prints the
    table, returns the rows (name, e_dev, e_ref, bound)."""
    rows = []
    print("\n%s\n  %-12s %11s %11s %11s" % (title, "tensor", "e_T device", "reference", "bound"))
    for name in (GLOBAL_NAMES if names is None else names):
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


def closest(rows, dev, bound, name):
    """-> (name, device / bound) of the row of a table closest to (or furthest beyond) its bound; dev / bound / name: the columns."""
    ratio = lambda r: r[dev] / r[bound] if r[bound] > 0 else (np.inf if r[dev] > 0 else 0.0)
    r = max(rows, key=ratio)
    return r[name], float(ratio(r))


def class_step(values, step, xin, precision, conv4_fp8=None):
    """One step of net_oracle.STEPS as the plan's arithmetic class computes it from the given decoded inputs -> its outputs, in STEPS' order:
      * an output whose step multiplies on an MX MFMA or that is stored with a code plane (mx_outputs of the plan; everything in f16m8): the
        CPU model's per-layer step (net_emulation.layer_step) under the plan's format table;
      * an x3 output (hi + lo operands, hi + lo storage): a float32 torch convolution of the class's operands - weights and stored results as
        hi + lo pairs of halfs. (With the weights left in float32 the bound is not one ANY implementation of the design can meet: the design
        represents a weight and a stored value to 2^-22, float32 to 2^-24, and the design's own CPU model - exact accumulation - already sits
        at 2.8 .. 6 times the plain float32 figure: conv1_2 1.9e-7 vs 6.8e-8, conv2_2 1.8e-7 vs 4.4e-8, conv3_1+conv3_2 5.3e-9 vs 8.8e-10, s = 8.)
      * f16: the fp16-storage oracle's step (fp16 weights and stored results, wide accumulation)."""
    outs = net_oracle.STEPS[step][1]
    if precision == "f16":
        return net_oracle.step_torch(values, step, xin, quant="fp16")[0]
    mx = mx_outputs(precision, conv4_fp8)
    table = format_table(precision, conv4_fp8)
    emu = net_emulation.layer_step(values, step, xin, mode=precision, **(dict(table=table) if table else {})) if any(o in mx for o in outs) else None
    f32 = net_oracle.step_torch(values, step, xin, dtype="float32", quant="x3")[0] if any(o not in mx for o in outs) else None
    return [emu[k] if o in mx else f32[k] for k, o in enumerate(outs)]


def local_table(dec, values, precision, title, steps=None, conv4_fp8=None):
    """The local check: per step of net_oracle.STEPS, the fp64 oracle's step applied to the DEVICE's decoded input is the exact answer for what
    that one launch (or fused group) was given; metric max |t - exact| / (A + |exact|) with A the forward-error scale of the element
    (net_oracle.step_torch); the same metric of the arithmetic class's reference ON THE SAME INPUT (class_step says which reference judges
    which output of which plan, and why), times 3, is the bound.
    Prints the table, returns rows (step, output, e_dev, e_ref, bound, seconds)."""
    rows = []
    print("\n%s\n  %-26s %-11s %11s %11s %11s %6s" % (title, "step", "output", "device", "reference", "bound", "s"))
    for step, (ins, outs) in net_oracle.STEPS.items():
        if steps is not None and step not in steps:
            continue
        t0 = time.time()
        xin = [dec[n] for n in ins]
        exact, A = net_oracle.step_torch(values, step, xin)
        ref = class_step(values, step, xin, precision, conv4_fp8)
        for k, o in enumerate(outs):
            den = A[k] + np.abs(exact[k])
            e_dev, e_ref = _metric(dec[o], exact[k], den), _metric(ref[k], exact[k], den)
            rows.append((step, o, e_dev, e_ref, 3.0 * e_ref, time.time() - t0))
            print("  %-26s %-11s %11.3e %11.3e %11.3e %6.1f%s" % (step, o, e_dev, e_ref, 3.0 * e_ref, time.time() - t0, "" if e_dev <= 3.0 * e_ref else "   <-- FAILS"))
    return rows
