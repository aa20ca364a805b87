"""CPU: tests/act_decode.py against oracle/net_emulation.py - the model's stored tensors, written into raw planes in the layout
sn_debug_tensor_info describes and decoded again, come back bit for bit, for each of the four storage formats (and the three-plane tensor),
channel counts that are no multiple of 8 included (100 -> 104, 300 -> 304, 6 -> 8). The two implementations are independent: the model
quantises by arithmetic (round(a / step) * step), the decoder reads code tables, the encoder searches them."""
import numpy as np
import pytest

import act_decode as ad
import synth
from oracle import net_emulation, net_oracle

# rows of the plan's tensor table (sn_api.hip kTensors: level, channel stride) with the format and code exponent the default plan / the f16m8
# plan / the f16 plan store them in: model tensor -> (level, channel stride, real channels, format, e8, producing ReLU layer or None)
DEFAULT = {
    "x": (0, 8, 6, ad.FMT_HILO, 132, None), "conv1_1": (0, 32, 32, ad.FMT_HILO, 127, "conv1_1"), "pool1": (1, 32, 32, ad.FMT_HILO, 127, "conv1_3"),
    "conv2_2": (1, 80, 80, ad.FMT_HILO, 127, "conv2_2"), "side2_pre": (1, 16, 16, ad.FMT_HILO, 127, None),
    "conv3_2": (2, 160, 160, ad.FMT_HILO, 127, "conv3_2"), "conv3_3": (2, 160, 160, ad.FMT_HILO_M8, 127, "conv3_3"),
    "conv4_2": (2, 304, 300, ad.FMT_M8, 127, "conv4_2"), "conv4_3": (2, 304, 300, ad.FMT_HILO, 127, "conv4_3"),
    "cat": (0, 64, 64, ad.FMT_M6, 125, None), "merge_a": (0, 104, 100, ad.FMT_M6, 127, "merge_conv_a"),
}
M8 = {
    "x": (0, 8, 6, ad.FMT_M6, 132, None), "conv2_2": (1, 80, 80, ad.FMT_M6, 127, "conv2_2"), "conv4_2": (2, 304, 300, ad.FMT_M6, 127, "conv4_2"),
    "cat": (0, 64, 64, ad.FMT_M6, 125, None), "merge_a": (0, 104, 100, ad.FMT_M6, 127, "merge_conv_a"),
}
MAX_SAMPLES = 2          # one sample decoded out of a two-sample workspace: the lo / code planes start after BOTH samples


def layout(s, level, cs, fmt, e8, M=MAX_SAMPLES):
    D = s >> level
    plane = M * D ** 3 * cs
    lo = plane if fmt in (ad.FMT_HILO, ad.FMT_HILO_M8) else -1
    code = {ad.FMT_M6: plane, ad.FMT_M8: plane, ad.FMT_HILO_M8: 2 * plane}.get(fmt, -1)
    planes = 1 + (lo > 0) + (code > 0)
    return ad.Layout(D, cs, planes, lo, code, e8, 2 * plane * planes, fmt)


@pytest.fixture(scope="module", params=[8, 12])
def model(request):
    s = request.param
    values = list(synth.calibrated_params(1))
    X = synth.random_cvc(1, s, 40 + s)
    out = {}
    for mode in ("f16x3", "f16m8"):
        _, _, inter = net_emulation.forward_emulated(X, values, mode=mode, return_intermediates=True)
        out[mode] = inter
    return s, net_oracle.params_to_dict(values), out


@pytest.mark.parametrize("mode,table", [("f16x3", DEFAULT), ("f16m8", M8)])
def test_round_trip_is_bit_exact_in_every_storage_format(model, mode, table):
    s, P, inter = model
    inter = inter[mode]
    seen = set()
    for name, (level, cs, C, fmt, e8, relu) in table.items():
        lay = layout(s, level, cs, fmt, e8)
        assert lay.max_samples() == MAX_SAMPLES
        oe = net_emulation.renorm_exponents(P[relu]) if relu else None
        y = inter["unrounded"][name]
        assert y.shape == (1, C, lay.extent, lay.extent, lay.extent)
        raw = ad.encode(y, lay, oe=oe)
        views = [("lo", name + "_x3"), ("code", name)] if fmt == ad.FMT_HILO_M8 else [(None, name)]
        for view, ref in views:
            v, pad, extra = ad.decode(raw, lay, 1, C, oe=oe, view=view)
            assert v.dtype == np.float64 and np.array_equal(v, inter[ref]), (name, view, np.abs(v - inter[ref]).max())
            assert pad.shape[1] == cs - C and not pad.any()
        # the second sample of the workspace was left alone, and the planes do not overlap: decoding it gives zeros
        v2, _, _ = ad.decode(raw, lay, 2, C, oe=oe)
        assert not v2[1].any()
        seen.add(fmt)
        assert np.abs(y).max() > 0 and np.abs(v - y).max() <= np.abs(y).max() * 2.0 ** -10      # (not vacuous: a real tensor, decoded to storage accuracy)
    want = {ad.FMT_HILO, ad.FMT_M6, ad.FMT_M8, ad.FMT_HILO_M8} if mode == "f16x3" else {ad.FMT_M6}
    assert seen == want


def test_single_fp16_plane(model):
    """Format 0 (precision "f16"): one plane, value = fp16(y * 2^e) / 2^e."""
    s, P, inter = model
    y = inter["f16x3"]["unrounded"]["merge_a"]
    oe = net_emulation.renorm_exponents(P["merge_conv_a"])
    lay = layout(s, 0, 104, ad.FMT_F16, 127)
    v, pad, _ = ad.decode(ad.encode(y, lay, oe=oe), lay, 1, 100, oe=oe)
    sc = np.ldexp(1.0, oe.astype(np.int64))[None, :, None, None, None]
    assert np.array_equal(v, (y * sc).astype(np.float16).astype(np.float64) / sc) and not pad.any()


def test_code_tables_and_slot_order():
    """Known answers: the two code tables' landmarks, and one hand-built slot of each kind."""
    assert ad.E2M3[0b011111] == 7.5 and ad.E2M3[0b000001] == 0.125 and ad.E2M3[0b001000] == 1.0 and ad.E2M3[0b100001] == -0.125
    assert ad.E4M3[0x7e] == 448.0 and ad.E4M3[0x01] == 2.0 ** -9 and ad.E4M3[0x38] == 1.0 and np.isnan(ad.E4M3[0x7f])
    lay = layout(8, 3, 8, ad.FMT_M8, 127, M=1)          # one voxel, one group
    raw = np.zeros(lay.nbytes, np.uint8)
    raw[:16].view(np.float16)[:] = np.arange(1, 9)
    raw[16:24] = 0x38                                    # hi codes 1.0
    raw[24:32] = [0x38, 0xb8, 0x40, 0, 0, 0, 0, 0x30]    # lo codes 1, -1, 2, 0 ..., 0.5
    v, _, extra = ad.decode(raw, lay, 1, 8)
    assert np.array_equal(v.ravel(), np.arange(1, 9) + np.array([1, -1, 2, 0, 0, 0, 0, 0.5]) / 4096)
    lay = layout(8, 3, 8, ad.FMT_M6, 125, M=1)           # s = 2
    raw = np.zeros(lay.nbytes, np.uint8)
    raw[:16].view(np.float16)[:] = 0.5
    codes = [0] * 16
    codes[4], codes[7], codes[12] = 0b001000, 0b100001, 0b011111      # lo of channels 0, 3, 4: 1, -0.125, 7.5
    word = sum(c << (6 * p) for p, c in enumerate(codes))
    raw[16:28] = np.frombuffer(word.to_bytes(12, "little"), np.uint8)
    v, _, _ = ad.decode(raw, lay, 1, 8)
    assert np.array_equal(v.ravel(), 0.5 + np.array([1, 0, 0, -0.125, 7.5, 0, 0, 0]) / 2.0 ** 13)


def test_single_steps_reproduce_the_whole_pass(model):
    """net_oracle.step_torch and net_emulation.layer_step, fed the stored tensors of their own full pass, return that pass's next stored
    tensors: the fp64 oracle exactly (the same convolutions on the same arrays), the model to one step of a stored lo code, at most 2^-13 of the
    tensor's maximum (a decoded value hi + lo is split again, and where lo is exactly half an ulp the halves come out differently: the same
    value, but another code of it enters the MX products, and the last fp32 bit of a result decides a 4-bit lo code of 2^-11 of its value)."""
    s, P, inter = model
    values = list(synth.calibrated_params(1))
    X = synth.random_cvc(1, s, 40 + s)
    _, u64, exact = net_oracle.forward_torch(X, values, return_intermediates=True)
    exact.update(x=X.astype(np.float64), out=u64.reshape(1, 1, s, s, s), cat48=exact["cat"][:, 16:], conv3_3_x3=exact["conv3_3"])
    for step, (ins, outs) in net_oracle.STEPS.items():
        got, scale = net_oracle.step_torch(values, step, [exact[n] for n in ins])
        for o, g, a in zip(outs, got, scale):
            assert g.shape == exact[o].shape == a.shape and np.abs(g - exact[o]).max() <= 1e-13 * np.abs(exact[o]).max(), (step, o)
            assert (a >= 0).all() and np.isfinite(a).all(), (step, o)
    for mode in ("f16x3", "f16m8"):
        _, ue, emu = net_emulation.forward_emulated(X, values, mode=mode, return_intermediates=True)
        emu.update(out=ue.reshape(1, 1, s, s, s), cat48=emu["cat"][:, 16:])
        for step, (ins, outs) in net_oracle.STEPS.items():
            got = net_emulation.layer_step(values, step, [emu[n] for n in ins], mode=mode)
            for o, g in zip(outs, got):
                assert np.abs(g - emu[o]).max() <= 2.0 ** -13 * np.abs(emu[o]).max(), (mode, step, o, np.abs(g - emu[o]).max() / np.abs(emu[o]).max())
