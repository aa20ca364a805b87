"""Test-side decoder (and, for the round-trip test, encoder) of the activation tensors the HIP path keeps in its workspace: raw planes as
sn_debug_tensor copies them -> fp64 (S, C, D, D, D) arrays in the network's original units. Plain numpy; knows the formats, not the plan:
the layout of one tensor comes from sn_debug_tensor_info (Layout.from_info), the renormalisation exponents from the layer's BatchNorm
parameters exactly as oracle/net_emulation.py computes them.

Layout: every plane is [max_samples][channel stride / 8][D][D][D][8 channels]; a plane of code slots has the same
shape with a 16-byte slot in place of the 8 halfs. Formats (conv3d_mfma.h OSPLIT, surfacenet_amd/csrc/mx_format.h), with s = 127 - e8:
  0  fp16                        value = hi
  1  hi + fp16 lo                value = hi + lo
  2  hi + 6-bit e2m3 slots       value = hi + code_lo / 2^(11 + s); slot = 16 six-bit codes [hi c0..3 | lo c0..3 | hi c4..7 | lo c4..7],
                                 code p at bits [6p, 6p + 6) of the slot's first 12 bytes; hi codes = q6(hi * 2^s)
  3  hi + fp8 e4m3 slots         value = hi + code_lo / 2^(12 + s); slot = bytes [hi c0..7 | lo c0..7]; hi codes = q8(hi * 2^s)
  4  hi + fp16 lo + fp8 slots    both of the above (conv3_3's output: side_op3 reads hi + lo, conv4_1 hi + codes)
"""
import numpy as np

FMT_F16, FMT_HILO, FMT_M6, FMT_M8, FMT_HILO_M8 = 0, 1, 2, 3, 4
LO_EXP6, LO_EXP8 = 11, 12


def _table(ebits, mbits, bias):
    """Values of the sign-magnitude minifloat codes 0 .. 2^(1 + ebits + mbits) - 1 (no inf; subnormals at exponent field 0)."""
    n = 1 << (ebits + mbits)
    c = np.arange(n)
    e, m = c >> mbits, c & ((1 << mbits) - 1)
    mag = np.where(e == 0, np.ldexp(m / float(1 << mbits), 1 - bias), np.ldexp(1.0 + m / float(1 << mbits), e - bias))
    return np.concatenate([mag, -mag])


E2M3 = _table(2, 3, 1)          # 64 codes, |max| 7.5, subnormal step 0.125
E4M3 = _table(4, 3, 7)          # 256 codes (OCP e4m3fn), |max| 448 at 0x7e; 0x7f / 0xff are NaN
E4M3[[0x7f, 0xff]] = np.nan


class Layout:
    """One tensor as sn_debug_tensor_info describes it: extent, channel stride, planes, lo / code plane offsets in halfs (-1: none), the
    E8M0 exponent of its code plane (127 - s), total bytes, format."""
    def __init__(self, extent, cs, planes, lo, code, e8, nbytes, fmt):
        self.extent, self.cs, self.planes, self.lo, self.code, self.e8, self.nbytes, self.fmt = (int(v) for v in (extent, cs, planes, lo, code, e8, nbytes, fmt))

    @classmethod
    def from_info(cls, info):
        return cls(*[int(v) for v in info[:8]])

    @property
    def s(self):
        return 127 - self.e8

    def max_samples(self):
        per_plane = self.extent ** 3 * self.cs * 2
        n_planes = {FMT_F16: 1, FMT_HILO: 2, FMT_M6: 2, FMT_M8: 2, FMT_HILO_M8: 3}[self.fmt]
        assert self.nbytes % (per_plane * n_planes) == 0, (self.nbytes, per_plane, n_planes)
        return self.nbytes // (per_plane * n_planes)


def _plane16(raw, lay, off, S):
    """halfs [off, off + plane) of the raw bytes -> (S, cs, D, D, D) float64."""
    D, G, M = lay.extent, lay.cs // 8, lay.max_samples()
    h = np.frombuffer(raw, dtype=np.float16, count=M * G * D ** 3 * 8, offset=2 * off).reshape(M, G, D, D, D, 8)[:S]
    return h.transpose(0, 1, 5, 2, 3, 4).reshape(S, G * 8, D, D, D).astype(np.float64)


def _slots(raw, lay, off, S):
    D, G, M = lay.extent, lay.cs // 8, lay.max_samples()
    return np.frombuffer(raw, dtype=np.uint8, count=M * G * D ** 3 * 16, offset=2 * off).reshape(M, G, D, D, D, 16)[:S]


def _codes_to_channels(v, S, lay):
    """(S, G, D, D, D, 8) per-slot values -> (S, cs, D, D, D)."""
    D, G = lay.extent, lay.cs // 8
    return v.transpose(0, 1, 5, 2, 3, 4).reshape(S, G * 8, D, D, D)


def _decode_slots(raw, lay, off, S, fmt):
    """-> (hi code values, lo code values), each (S, cs, D, D, D), still premultiplied (as stored)."""
    sl = _slots(raw, lay, off, S)
    if fmt == FMT_M6:
        bits = np.unpackbits(sl[..., :12], axis=-1, bitorder="little").reshape(sl.shape[:-1] + (16, 6))
        code = (bits * (1 << np.arange(6, dtype=np.uint8))).sum(axis=-1)
        val = E2M3[code]                                             # (..., 16): hi c0..3 | lo c0..3 | hi c4..7 | lo c4..7
        hi = np.concatenate([val[..., 0:4], val[..., 8:12]], axis=-1)
        lo = np.concatenate([val[..., 4:8], val[..., 12:16]], axis=-1)
        unused = sl[..., 12:]
    else:
        val = E4M3[sl]
        hi, lo = val[..., :8], val[..., 8:]
        unused = None
    return _codes_to_channels(hi, S, lay), _codes_to_channels(lo, S, lay), unused


def decode(raw, lay, S, C, oe=None, view=None):
    """raw: the tensor's bytes (sn_debug_tensor; every plane); lay: its Layout; S: samples to decode (<= max_samples); C: real channels;
    oe: per-channel renormalisation exponents (stored = value * 2^oe; None: zeros); view: for format 4 "lo" (default) or "code".
    Returns (value, pad, extra): value (S, C, D, D, D) fp64 in original units as the readers of that view see it; pad (S, cs - C, D, D, D)
    the padded channels as stored (planes summed the same way, no exponent); extra: dict with "hi" (the fp16 plane alone, stored units,
    all cs channels) and, for code formats, "hi_code" / "lo_code" (code values / 2^s resp. / 2^(LO_EXP + s), stored units)."""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    assert raw.size == lay.nbytes, (raw.size, lay.nbytes)
    assert 0 < C <= lay.cs and lay.cs % 8 == 0 and S <= lay.max_samples()
    hi = _plane16(raw, lay, 0, S)
    extra = {"hi": hi}
    fmt = lay.fmt
    if fmt == FMT_HILO_M8:
        fmt = FMT_M8 if view == "code" else FMT_HILO
    if fmt == FMT_F16:
        stored = hi
    elif fmt == FMT_HILO:
        assert lay.lo > 0
        stored = hi + _plane16(raw, lay, lay.lo, S)
    else:
        assert lay.code > 0
        hc, lc, unused = _decode_slots(raw, lay, lay.code, S, fmt)
        le = LO_EXP6 if fmt == FMT_M6 else LO_EXP8
        extra["hi_code"], extra["lo_code"] = np.ldexp(hc, -lay.s), np.ldexp(lc, -(le + lay.s))
        if unused is not None:
            extra["unused_bytes"] = unused
        stored = hi + extra["lo_code"]
    e = np.zeros(C) if oe is None else np.asarray(oe, dtype=np.float64)
    assert e.shape == (C,)
    value = np.ldexp(stored[:, :C], -e.astype(np.int64)[None, :, None, None, None])
    return value, stored[:, C:], extra


# ------------------------------------------------------------------------------------------------
# encoder: the same formats written from unrounded values (the CPU round-trip test; never used on device data)
# ------------------------------------------------------------------------------------------------
def _nearest_code(v, table):
    """Round-to-nearest-even, saturating: index into `table` of the code nearest to v (ties to the even code; NaN entries never chosen)."""
    half = table.size // 2
    mag = table[:half]
    ok = ~np.isnan(mag)
    grid = mag[ok]                                                   # ascending
    a = np.minimum(np.abs(v), grid[-1])
    i = np.clip(np.searchsorted(grid, a, side="left"), 1, grid.size - 1)
    lo, up = grid[i - 1], grid[i]
    pick_up = (a - lo > up - a) | ((a - lo == up - a) & (i % 2 == 0))     # tie: the even code (codes of non-NaN magnitudes are 0 .. n-1 in order)
    idx = np.where(pick_up, i, i - 1)
    return (idx + np.where(np.signbit(v), half, 0)).astype(np.uint8)


def encode(value, lay, M=None, oe=None):
    """value: (S, C, D, D, D) unrounded values in original units -> the raw bytes (uint8, lay.nbytes) a producer would store: channels padded
    with zeros, samples beyond S zero."""
    S, C, D = value.shape[0], value.shape[1], lay.extent
    M = lay.max_samples() if M is None else M
    G = lay.cs // 8
    e = np.zeros(C) if oe is None else np.asarray(oe, dtype=np.float64)
    r = np.zeros((M, lay.cs, D, D, D))
    r[:S, :C] = np.ldexp(np.asarray(value, dtype=np.float64), e.astype(np.int64)[None, :, None, None, None])
    hi = r.astype(np.float16)
    res = r - hi.astype(np.float64)

    def grouped(a):                                                  # (M, cs, D, D, D) -> (M, G, D, D, D, 8)
        return np.ascontiguousarray(a.reshape(M, G, 8, D, D, D).transpose(0, 1, 3, 4, 5, 2))

    raw = np.zeros(lay.nbytes, dtype=np.uint8)

    def put(off, arr):
        b = arr.reshape(-1).view(np.uint8)
        raw[2 * off: 2 * off + b.size] = b

    put(0, grouped(hi))
    if lay.fmt in (FMT_HILO, FMT_HILO_M8):
        put(lay.lo, grouped(res.astype(np.float16)))
    if lay.fmt == FMT_M6:
        hc = grouped(_nearest_code(np.ldexp(hi.astype(np.float64), lay.s), E2M3))
        lc = grouped(_nearest_code(np.ldexp(res, LO_EXP6 + lay.s), E2M3))
        codes = np.concatenate([hc[..., :4], lc[..., :4], hc[..., 4:], lc[..., 4:]], axis=-1)      # (..., 16) six-bit codes
        bits = ((codes[..., None] >> np.arange(6, dtype=np.uint8)) & 1).astype(np.uint8).reshape(codes.shape[:-1] + (96,))
        slot = np.zeros(codes.shape[:-1] + (16,), dtype=np.uint8)
        slot[..., :12] = np.packbits(bits, axis=-1, bitorder="little")
        put(lay.code, slot)
    if lay.fmt in (FMT_M8, FMT_HILO_M8):
        hc = grouped(_nearest_code(np.ldexp(hi.astype(np.float64), lay.s), E4M3))
        lc = grouped(_nearest_code(np.ldexp(res, LO_EXP8 + lay.s), E4M3))
        put(lay.code, np.concatenate([hc, lc], axis=-1))
    return raw
