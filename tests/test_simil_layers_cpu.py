"""CPU: the per-layer check of the similarityNet (tests/simil_layer_check.py, tests/simil_decode.py) can fail. A stand-in "device" - the x3
class reference run launch by launch, its tensors encoded in the byte layout of the test-only hook sn_debug_simil_tensor and decoded again -
passes every row of both tables; with one fault planted in one stored tensor (and carried through every later launch, as a device would),
the planted launch's LOCAL row fails and no other, and the GLOBAL rows fail from that tensor on. Also: the workspace arithmetic the hook's
info is checked against on the GPU (simil_decode.layout) for the patch counts 1, 9 and 2040 in both modes."""
import numpy as np
import pytest

import simil_decode as sd
import simil_layer_check as slc
from oracle import simil_oracle as so

MEAN_BGR = np.asarray([103.939, 116.779, 123.68]).astype(np.float32)
N = 2


def _info(name, count, planes):
    if name in ("feat", "emb"):
        L = sd.FEAT if name == "feat" else sd.EMB
        return sd.Info(0, L, 1, -1, count, 8, count * L * 4)
    H, cs = (sd.PATCH, 8) if name == "p0" else (slc.extent(name), slc.CHANNELS[name])
    return sd.Info(H, cs, planes, cs * H * H * 8 if planes == 2 else -1, count, 8, planes * cs * count * H * H * 2)


def through_the_hook_layout(t, planes=2):
    """name -> unrounded tensor => name -> what the decoder makes of the bytes the hook would hand out for it (+ the round trip's proof)."""
    dec = {}
    for name, v in t.items():
        if name in ("feat", "emb"):
            dec[name] = np.asarray(v, dtype=np.float32).astype(np.float64)
            continue
        info = _info(name, v.shape[0], planes)
        C = 3 if name == "p0" else slc.CHANNELS[name]
        raw = sd.encode(v[:, :C], info)
        assert raw.size == info.nbytes
        val, pad, halfs = sd.decode(raw, info, v.shape[0], C)
        assert not pad.any() and np.array_equal(sd.encode(val, info), raw), name       # bit-exact round trip
        dec[name] = val
    return dec


def _unpooled_x3(values, i, x):
    """Layer i's conv + bias + ReLU in the x3 class (float32, hi + lo weights), NOT pooled, not yet rounded for storage."""
    import torch
    import torch.nn.functional as F
    W = torch.from_numpy(sd.hilo(values[2 * i]).astype(np.float32))
    b = torch.from_numpy(np.asarray(values[2 * i + 1], dtype=np.float32))
    return F.relu(F.conv2d(torch.from_numpy(np.asarray(x, dtype=np.float32)), W, b, padding=1))


def run_stand_in(values, X, fault=None):
    """The x3 class reference, launch by launch on its own stored tensors, with `fault` (layer name) planted in that layer's stored output."""
    import torch
    import torch.nn.functional as F
    t = {"p0": sd.hilo(X)}
    x = t["p0"]
    for i, name in enumerate(slc.LAYERS):
        y = so.step(values, i, x, dtype="float32", quant="x3")[0]
        if name == fault == "s_conv2_1":
            # patch 1, row 0 without its halo: the image's row 0 has no input row above it, so the one neighbouring row its 3-row windows reach
            # is row 1 - what a kernel that failed to stage that row would store is the result with row 1 read as zeros
            x0 = x.copy()
            x0[:, :, 1, :] = 0
            y[1, :, 0, :] = so.step(values, i, x0, dtype="float32", quant="x3")[0][1, :, 0, :]
        elif name == fault == "s_conv5_2":
            y = y[[1, 0]].copy()                                   # patches 0 and 1 swapped
        elif name == fault == "s_conv3_3":
            u = F.pad(_unpooled_x3(values, i, x)[:, :, 1:, 1:], (0, 1, 0, 1))      # pooled over the 2x2 windows that start at odd rows / columns
            y = sd.hilo(F.max_pool2d(u, 2).numpy())
        t[name] = x = y
    t["feat"] = so.feat_step([t[p] for p in slc.POOLS], dtype="float32")
    t["emb"] = so.emb_step(values, t["feat"], dtype="float32")
    return t


@pytest.fixture(scope="module")
def case():
    from surfacenet_amd import weights
    values = weights.synthetic_simil_param_values(1)
    raw = np.random.RandomState(2).randint(0, 256, (N, 64, 64, 3)).astype(np.uint8)
    raw[1] = (np.indices((64, 64)).sum(0)[:, :, None] * [1, 2, 3] % 256).astype(np.uint8)
    X = so.preprocess(raw, MEAN_BGR)
    exact, ref = slc.references(X, values, "f16x3")
    clean = through_the_hook_layout(run_stand_in(values, X))
    loc = slc.local_table(clean, values, "f16x3", "stand-in device (x3 class reference), no fault: each launch on its own stored input")
    return values, X, exact, ref, clean, loc


def test_round_trip_is_bit_exact_in_both_formats_and_the_stand_in_passes_every_row(case):
    values, X, exact, ref, clean, loc = case
    # format 0 (one fp16 plane) on a map with padded channels and on a pooled map; format 1 is proved inside through_the_hook_layout
    one = through_the_hook_layout({"p0": np.asarray(X, dtype=np.float64), "s_conv5_3": exact["s_conv5_3"]}, planes=1)
    assert np.array_equal(one["p0"], X.astype(np.float16).astype(np.float64))
    assert np.array_equal(one["s_conv5_3"], exact["s_conv5_3"].astype(np.float16).astype(np.float64))
    slc.check_p0(clean["p0"], np.zeros((2, N, 5, 64, 64), np.float16), X, "f16x3")
    slc.check_p0(one["p0"], np.zeros((1, N, 5, 64, 64), np.float16), X, "f16")
    # (the stand-in IS the class reference run the same way: device column == reference column, so every row passes with equality to spare)
    g = slc.global_table(clean, exact, ref, "stand-in device, no fault: stored tensors against the fp64 oracle")
    assert slc.failing(g, loc) == ([], [])
    assert all(r[2] > 0 for r in g) and all(r[2] > 0 for r in loc), "a reference that never errs bounds nothing"
    for name in slc.NAMES:
        assert np.array_equal(clean[name], ref[name]), name


@pytest.mark.parametrize("fault", ["s_conv2_1", "s_conv5_2", "s_conv3_3"])
def test_a_planted_fault_fails_its_own_local_row_and_the_global_rows_from_there_on(case, fault):
    values, X, exact, ref, clean, loc_clean = case
    dec = through_the_hook_layout(run_stand_in(values, X, fault=fault))
    k = slc.NAMES.index(fault)
    for name in slc.NAMES[:k]:
        assert np.array_equal(dec[name], clean[name]), name         # launches before the fault: the clean run's rows stand
    loc = slc.local_table(dec, values, "f16x3", "fault planted in %s: each launch on its own stored input" % fault, only=slc.NAMES[k:])
    bad_l = [r[0] for r in loc if not r[1] <= r[3]]
    assert bad_l == [fault], bad_l                                   # LOCAL: the planted launch and no other - later launches are right about
    #                                                                  the (wrong) input they were given
    g = slc.global_table(dec, exact, ref, "fault planted in %s: stored tensors against the fp64 oracle" % fault)
    bad_g = [r[0] for r in g if not r[1] <= r[3]]
    # GLOBAL: every tensor from the planted one on. Each fault is an O(1) error of the stored map (a third of a window's taps, another
    # patch's map, another window's maximum); it reaches pool5 through every later block's growing windows (conv2_1's row 0 spreads to rows
    # 0 .. 4 of conv4_3's 8 and all of conv5_x's 4), feat through pool5's 2048 entries and emb through the dense layer, and nothing on the way contracts it by the
    # six orders of magnitude that separate it from 4 x the float32 class's error.
    assert bad_g == slc.NAMES[k:], bad_g


@pytest.mark.parametrize("n", [1, 9, 2040])
@pytest.mark.parametrize("planes", [1, 2])
def test_workspace_arithmetic_behind_the_hooks_info(n, planes):
    """What sn_debug_simil_info must report for a fresh context's run of n patches, from simil_carve's arithmetic restated in
    simil_decode.layout: capacity max(n, 8); a map's hi plane of the run ([C/8][n][H][H][8], group stride n) ends at or before its lo plane,
    which sits at the CAPACITY's offset - strictly before it when n < cap; maps do not overlap; the two 64x64 group planes of a slab stay
    below the 2^28 - 16 byte offset field of the conv kernel's halo addressing at the largest chunk."""
    cap, total, maps = sd.layout(n, planes)
    assert cap == max(n, 8) and cap <= sd.CHUNK
    order = sorted(maps.items(), key=lambda kv: kv[1][0])
    for (name, (off, lo, C, H)), nxt in zip(order, order[1:] + [("end", (total, 0, 0, 0))]):
        assert off % 256 == 0
        if H == 0:
            continue
        run_plane = C * n * H * H * 2                                # bytes of one plane of the run
        assert (lo == C * H * H * cap) if planes == 2 else (lo == -1)
        end = off + (2 * lo + run_plane if planes == 2 else run_plane)
        assert end <= nxt[1][0], (name, end, nxt)
        if planes == 2:
            assert run_plane <= 2 * lo and (run_plane < 2 * lo) == (n < cap)
    for name in slc.STORED:                                          # the tensor a layer leaves, in the buffer run_simil's walk gives it
        off, lo, C, H = maps[slc.buffer_of(name)]
        info = _info(name, n, planes)
        assert (info.H, info.cs) == (H, C) and info.nbytes == planes * C * n * H * H * 2 == info.bytes_of(n), name
    assert 2 * 8 * n * 64 * 64 * 2 + 4 * 10 * 10 * 8 * 16 < (1 << 28) - 16 - (1 << 16)
