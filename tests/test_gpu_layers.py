"""GPU (-m gpu): every activation tensor the forward pass leaves in the workspace, read back through the test-only twin library
(sn_debug_tensor / sn_debug_tensor_info), decoded (tests/act_decode.py) and compared with the fp64 oracle - layer by layer.

  * GLOBAL: e_T = max|device - fp64| / max|fp64| per stored tensor, bounded by the same figure of the arithmetic class's reference on the same
    input (the CPU model oracle/net_emulation.py in the MX-assisted modes, times 3; the float32 / fp16-storage oracle for f16x3p / f16,
    times 4). The bounds are computed at test time from the references, never from the device.
  * LOCAL: per launch (or fused group of launches), the fp64 oracle's step applied to the DEVICE's own stored input is the exact answer for
    what that kernel was given: |device - exact| <= bound (A + |exact|) per element, A = (|W| (*) |x|) |scale|; bound = 3 x the same metric of
    the class's reference on the same input (tests/layer_check.py local_table says which reference judges which output, and why). Needs no
    upstream agreement: a kernel that mishandles one halo row fails its own row of the table and no other.
  * PADDING: the padded channels (6 -> 8, 300 -> 304, 100 -> 104) are exact zeros in every plane; workspace samples beyond the batch are
    untouched.

Shapes: the smallest cube sizes that reach each tile / halo case of ConvKernel::launch, for EVERY plan build_plan_t can select (precision,
conv4_fp8; tests/golden/conv_plan.json): cube_D 8 and 12 (every tile partial), 20 (extents 20 / 10 / 5: a partial tile behind a full one at
levels 0 and 1, two full 8-tiles and one full 16-tile at level 0), 40 (interior full tiles at level 0; quarter extent 10 = 8 + R, the smallest
multi-tile extent the dilated kernels accept) and 44 (22 / 11: a partial tile at every level at once), one sample; the default plan also at
24 and 28 (quarter extents 6 and 7). tests/test_layers_cpu.py holds CASES to the tile classes (layer_check.tile_classes) each plan can reach.
Measured figures: profiles/layers/README.md."""
import ctypes
import os
import time

import numpy as np
import pytest

import act_decode as ad
import layer_check as lc
import synth

pytestmark = pytest.mark.gpu

ALL = ("f16x3", "f16x3p", "f16m8", "f16")
# (cube_D, precision, conv4_fp8); conv4_fp8 None: the mode's own (sn.Context is given none) - 1 in f16x3
CASES = [(s, p, None) for s in (8, 12) for p in ALL] + [(s, "f16x3", None) for s in (20, 28, 24, 40)] + [(40, "f16x3p", None), (44, "f16x3", None)]
CASES += [(s, p, None) for p in ("f16m8", "f16") for s in (20, 40, 44)] + [(20, "f16x3p", None), (44, "f16x3p", None)]
# conv4_fp8 = 2 (conv4_1 on three fp16 MFMAs storing hi + fp8 codes: an instantiation no other plan has) and 0 (the public opt-out). 20 is there
# because the tile classes of a plan are counted over the plan's own cases (test_layers_cpu.py): extents 16 .. 31 are the only ones with exactly
# one full 16-wide conv1_x tile, and a 40 of the opt-out plan is its only quarter extent of 8 + R.
CASES += [(s, "f16x3", 2) for s in (12, 20, 40, 44)] + [(s, "f16x3", 0) for s in (12, 20, 40, 44)]


def case_id(c):
    return "%d-%s" % c[:2] + ("" if c[2] is None else "-conv4_fp8_%d" % c[2])


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


def read_back(ctx, dbg):
    """-> (raws, lays): every buffer of the plan's tensor table as raw bytes, and its layout as the library describes it."""
    raws, lays = {}, {}
    for buf in lc.BUFFERS:
        info = np.zeros(8, dtype=np.int64)
        assert dbg.sn_debug_tensor_info(ctx._h, buf.encode(), info.ctypes.data_as(ctypes.c_void_p)) == 0, dbg.sn_last_error()
        lay = ad.Layout.from_info(info)
        raw = np.empty(lay.nbytes, dtype=np.uint8)
        assert dbg.sn_debug_tensor(ctx._h, buf.encode(), raw.ctypes.data_as(ctypes.c_void_p), raw.nbytes) == 0, dbg.sn_last_error()
        raws[buf], lays[buf] = raw, lay
    return raws, lays


def check_layouts(lays, s, max_samples, precision, conv4_fp8=None):
    """What sn_debug_tensor_info says against what the plan is documented to store (layer_check.storage: DESIGN.md sections 3 and 5, build_plan_t)."""
    fmt, e8 = lc.storage(precision, conv4_fp8)
    assert set(lays) == set(fmt)
    for buf, lay in lays.items():
        assert lay.fmt == fmt[buf], (buf, lay.fmt, fmt[buf])
        assert lay.e8 == e8[buf], (buf, lay.e8, e8[buf])
        assert lay.max_samples() == max_samples and s % lay.extent == 0 and lay.extent in (s, s // 2, s // 4) and lay.cs % 8 == 0
        assert lay.cs - lc.BUFFERS[buf][1] in (0, 2, 4)


check_padding = lc.check_padding


@pytest.mark.parametrize("s,precision,conv4_fp8", CASES, ids=[case_id(c) for c in CASES])
def test_every_stored_tensor_and_every_launch(sn, dbg, s, precision, conv4_fp8):
    t0 = time.time()
    values = list(synth.calibrated_params(1))
    X = synth.random_cvc(1, s, 40 + s)
    plan = "%s%s" % (precision, "" if conv4_fp8 is None else ", conv4_fp8 = %d" % conv4_fp8)
    with sn.Context(cube_D=s, max_samples=1, precision=precision, **({} if conv4_fp8 is None else dict(conv4_fp8=conv4_fp8))) as ctx:
        ctx.load_param_values(values)
        _, unfused = ctx.forward(X, None, n_vp=1)
        raws, lays = read_back(ctx, dbg)
    t_gpu = time.time() - t0
    check_layouts(lays, s, 1, precision, conv4_fp8)
    dec, pads, extras = lc.decode_all(raws, lays, values, 1, unfused)
    check_padding(pads, extras, lays)
    exact, ref, factor = lc.references(X, values, precision, conv4_fp8)
    g = lc.global_table(dec, exact, ref, factor, "cube_D %d, %s: stored tensors against the fp64 oracle" % (s, plan))
    t_glob = time.time() - t0
    loc = lc.local_table(dec, values, precision, "cube_D %d, %s: each launch against the fp64 step on its own stored input" % (s, plan), conv4_fp8=conv4_fp8)
    print("  wall time: device + read-back %.1f s, global check %.1f s, local check %.1f s" % (t_gpu, t_glob - t_gpu, time.time() - t0 - t_glob))
    bad_g = [(r[0], "%.3e > %.3e" % (r[1], r[3])) for r in g if not r[1] <= r[3]]
    bad_l = [(r[0], r[1], "%.3e > %.3e" % (r[2], r[4])) for r in loc if not r[2] <= r[4]]
    print("  closest to its bound (device / bound): global %s %.2f, local %s %.2f" % (lc.closest(g, 1, 3, 0) + lc.closest(loc, 2, 4, 1)))
    assert not bad_g and not bad_l, (bad_g, bad_l)


def _planes(raw, lay):
    """The planes of one buffer as (max_samples, bytes per sample) views."""
    M = lay.max_samples()
    per = lay.extent ** 3 * lay.cs * 2
    offs = [0] + [2 * o for o in (lay.lo, lay.code) if o > 0]
    return [raw[o: o + M * per].reshape(M, per) for o in offs]


def test_chunked_batch_leaves_the_other_samples_alone(sn, dbg):
    """5 samples through a 4-sample workspace (cube_D 16): the last chunk holds one sample. What it leaves in the workspace is, bit for bit,
    what a one-sample call leaves - samples 1 .. 3 of every plane of every buffer still hold the first chunk's tensors - and all four
    workspace samples pass the global check against the oracle tensors of the inputs they belong to."""
    s, M = 16, 4
    values = list(synth.calibrated_params(1))
    X = synth.random_cvc(5, s, 77)
    with sn.Context(cube_D=s, max_samples=M) as ctx:
        ctx.load_param_values(values)
        _, uA = ctx.forward(X[:4], None, n_vp=1)
        rawA, lays = read_back(ctx, dbg)
        _, uB = ctx.forward(X[4:], None, n_vp=1)
        rawB, _ = read_back(ctx, dbg)
        _, uC = ctx.forward(X, None, n_vp=1)
        rawC, _ = read_back(ctx, dbg)
    check_layouts(lays, s, M, "f16x3")
    for buf, lay in lays.items():
        for k, (a, b, c) in enumerate(zip(_planes(rawA[buf], lay), _planes(rawB[buf], lay), _planes(rawC[buf], lay))):
            assert np.array_equal(a[1:], b[1:]), (buf, k, "a one-sample run touched samples beyond the first")
            assert not np.array_equal(a[0], b[0]), (buf, k)
            assert np.array_equal(b, c), (buf, k, "the chunked call left something else than its two chunks")
    assert np.array_equal(uC[:4], uA) and np.array_equal(uC[4:], uB)
    dec, pads, extras = lc.decode_all(rawC, lays, values, M, np.concatenate([uB, uA[1:]]))
    check_padding(pads, extras, lays)
    exact, ref, factor = lc.references(X, values, "f16x3")
    g = lc.global_table(dec, exact, ref, factor, "cube_D 16, 5 samples through max_samples = 4: workspace samples 0 .. 3 hold inputs 4, 1, 2, 3",
                        sample_of=[4, 1, 2, 3])
    bad = [(r[0], "%.3e > %.3e" % (r[1], r[3])) for r in g if not r[1] <= r[3]]
    assert not bad, bad


def test_debug_tensor_hook_refuses_what_it_cannot_serve(sn, dbg):
    buf = np.zeros(64, np.uint8)
    info = np.zeros(8, np.int64)
    with sn.Context(cube_D=8, max_samples=1) as ctx:
        assert dbg.sn_debug_tensor_info(ctx._h, b"a1", info.ctypes.data_as(ctypes.c_void_p)) != 0 and b"no plan" in dbg.sn_last_error()
        ctx.load_param_values(list(synth.calibrated_params(1)))
        assert dbg.sn_debug_tensor_info(ctx._h, b"zz", info.ctypes.data_as(ctypes.c_void_p)) != 0 and b"unknown tensor" in dbg.sn_last_error()
        ctx.forward(synth.random_cvc(1, 8, 1), None, n_vp=1)
        assert dbg.sn_debug_tensor_info(ctx._h, b"a1", info.ctypes.data_as(ctypes.c_void_p)) == 0
        assert dbg.sn_debug_tensor(ctx._h, b"a1", buf.ctypes.data_as(ctypes.c_void_p), int(info[6]) + 2) != 0 and b"asked for" in dbg.sn_last_error()
        # a3c alone: one plane of 16-byte slots, the same bytes as the third plane of "a3"
        assert dbg.sn_debug_tensor_info(ctx._h, b"a3c", info.ctypes.data_as(ctypes.c_void_p)) == 0 and list(info[:5]) == [2, 160, 1, -1, 0]
        a3c = np.empty(int(info[6]), np.uint8)
        assert dbg.sn_debug_tensor(ctx._h, b"a3c", a3c.ctypes.data_as(ctypes.c_void_p), a3c.nbytes) == 0
        raws, lays = read_back(ctx, dbg)
        assert np.array_equal(raws["a3"][2 * lays["a3"].code:], a3c) and a3c.any()
