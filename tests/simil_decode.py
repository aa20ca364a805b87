"""Test-side decoder (and, for the CPU round-trip test, encoder) of the similarityNet's stored tensors as the test-only hook
sn_debug_simil_tensor hands them out: patches [first, first + count) of a map, packed [planes][C/8][count][H][H][8] halfs -> fp64
(count, C, H, H). Plain numpy. Formats: 0 one fp16 plane (f16), value = hi; 1 two planes (every other mode), value = hi + lo.

On the DEVICE the same tensor is a plane [C/8][n][H][H][8] whose group stride is the run's patch count n, with the lo plane at the offset
the workspace's capacity gave it (layout(): that arithmetic restated from simil_carve, so a CPU test can pin what the hook reports)."""
import numpy as np

FMT_F16, FMT_HILO = 0, 1
# the workspace's maps in simil_carve's order: p0, then per block two ping-pong buffers and the pooled map (channels, extent)
STAGE_C = (64, 128, 256, 512, 512)
PATCH, FEAT, EMB, DENSE_KS, CHUNK = 64, 5888, 128, 8, 2040


class Info:
    """sn_debug_simil_info's seven numbers: map extent, channel stride, planes, lo-plane offset in halfs (-1: none), patches of the last run,
    patch capacity of the workspace, bytes of the n patches as the hook packs them."""
    def __init__(self, H, cs, planes, lo, n, cap, nbytes):
        self.H, self.cs, self.planes, self.lo, self.n, self.cap, self.nbytes = (int(v) for v in (H, cs, planes, lo, n, cap, nbytes))

    @classmethod
    def from_info(cls, info):
        return cls(*[int(v) for v in info[:7]])

    @property
    def fmt(self):
        return FMT_HILO if self.planes == 2 else FMT_F16

    def bytes_of(self, count):
        return self.planes * self.cs * count * self.H * self.H * 2


def planes(raw, info, count):
    """-> (planes, count, cs, H, H) float16: the stored halfs, channels unpacked from their 8-groups."""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    assert raw.size == info.bytes_of(count), (raw.size, info.bytes_of(count))
    H, G = info.H, info.cs // 8
    h = raw.view(np.float16).reshape(info.planes, G, count, H, H, 8)
    return np.ascontiguousarray(h.transpose(0, 2, 1, 5, 3, 4)).reshape(info.planes, count, G * 8, H, H)


def decode(raw, info, count, C):
    """raw: what sn_debug_simil_tensor wrote for `count` patches; C: real channels (<= channel stride). Returns (value, pad, halfs): value
    (count, C, H, H) fp64; pad (planes, count, cs - C, H, H) the padded channels of every plane as stored (p0: 3 -> 8); halfs: all planes."""
    assert 0 < C <= info.cs and info.cs % 8 == 0 and info.planes in (1, 2)
    h = planes(raw, info, count)
    v = h[0].astype(np.float64)
    if info.planes == 2:
        v = v + h[1].astype(np.float64)
    return v[:, :C], h[:, :, C:], h


def encode(value, info):
    """value (count, C, H, H), unrounded -> the bytes the hook would hand out for a producer that stores fp16 (format 0) or hi + lo
    (format 1); channels padded with zeros up to the channel stride."""
    count, C, H = value.shape[0], value.shape[1], info.H
    r = np.zeros((count, info.cs, H, H))
    r[:, :C] = np.asarray(value, dtype=np.float64)
    hi = r.astype(np.float16)
    pl = [hi] if info.planes == 1 else [hi, (r - hi.astype(np.float64)).astype(np.float16)]
    G = info.cs // 8
    out = np.stack([p.reshape(count, G, 8, H, H).transpose(1, 0, 3, 4, 2) for p in pl])      # (planes, G, count, H, H, 8)
    return np.ascontiguousarray(out).reshape(-1).view(np.uint8)


def hilo(x):
    """fp64 value of the hi + lo pair of halfs a float32 is stored as (elementwise.h sn_store8: lo = fp16(x - float(hi)) in fp32)."""
    x = np.asarray(x, dtype=np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64) + lo.astype(np.float64)


# ------------------------------------------------------------------------------------------------
# the workspace arithmetic of sn_simil.hip (simil_workspace / simil_carve), restated from the constants
# ------------------------------------------------------------------------------------------------
def _align(off, a=256):
    return (off + a - 1) // a * a


def layout(n, planes_):
    """The similarityNet workspace of a context that has only ever run n patches (n <= CHUNK) in a mode with `planes_` planes:
    -> (cap, total bytes, maps), maps: name -> (byte offset of the hi plane, lo-plane offset in halfs, channels, extent), names "p0",
    "a<st><k>" (block st's ping-pong buffer k), "pool<st + 1>", and "feat" / "emb" -> (byte offset, -1, row length, 0). Every array starts
    256-byte aligned (sn_host.h Carve)."""
    cap = min(max(n, 8), CHUNK)
    off, maps = 0, {}

    def act(name, ch, H):
        nonlocal off
        halfs = ch * H * H * cap
        off = _align(off)
        maps[name] = (off, halfs if planes_ == 2 else -1, ch, H)
        off += halfs * planes_ * 2

    act("p0", 8, PATCH)
    for st, ch in enumerate(STAGE_C):
        H = PATCH >> st
        act("a%d0" % st, ch, H); act("a%d1" % st, ch, H); act("pool%d" % (st + 1), ch, H // 2)
    for name, count, size in (("feat", cap * FEAT, 4), ("emb", cap * EMB, 4), ("part", cap * EMB * DENSE_KS, 4), ("centers", cap * 2, 8),
                              ("patches", cap * PATCH * PATCH * 3, 1)):
        off = _align(off)
        maps[name] = (off, -1, {"feat": FEAT, "emb": EMB}.get(name, 0), 0)
        off += count * size
    return cap, off, maps
