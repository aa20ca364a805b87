"""GPU (-m gpu): every tensor a similarityNet pass leaves in its workspace - the network input p0, the 13 stored maps (a block's last layer
stores its pooled output), the feature rows and the embeddings - read back through the test-only twin library (sn_debug_simil_info /
sn_debug_simil_tensor, sn_simil.hip), decoded (tests/simil_decode.py) and judged launch by launch (tests/simil_layer_check.py):

  * GLOBAL: e_T = max|device - fp64| / max|fp64| per stored tensor <= 4 x the same figure of the arithmetic class's reference on the same
    input (x3: hi + lo halfs, float32 convolutions - every mode but f16; fp16: halfs, wide accumulation - f16).
  * LOCAL: per launch, the fp64 step on the DEVICE's own stored input is the exact answer; max |device - exact| / (A + |exact|) <= 3 x the
    same metric of the class reference on that input. A wrong halo row fails its own launch's row and no other.
  * p0: channels 0..2 are the stored form of the float32 input, channels 3..7 exact zeros in every plane.
  Every bound is computed at test time from the references, never from the device.

The map extents 64 .. 4 are whole tiles (8x8 pixels; 4x4 = one image per MFMA fragment under conv5_x), so the only partial dimension is the
patch count n - the x axis of the 2-D form of conv3d_f16_mfma, 8 patches per tile (16 images under conv5_x), no halo along it:
  n = 1     a partial tile only; workspace capacity 8 > n, so the planes' group stride (n) differs from the lo plane's offset (capacity)
  n = 9     a full 8-patch tile + a one-patch tile; a partial 16-image conv5 tile
  n = 17    a full 16-image conv5 tile + a one-image tile
  n = 1033  = 129 x 8 + 1 = 64 x 16 + 9: more tiles than resident workgroups in EVERY layer (asserted from the plan rows and the CU count),
            so the persistent workgroups walk to a second tile and the next-tile halo prefetch runs
Measured figures of the first run: profiles/simil_layers/README.md."""
import ctypes
import functools
import os
import time

import numpy as np
import pytest

import golden_util
import simil_decode as sd
import simil_layer_check as slc
from oracle import simil_oracle as so

pytestmark = pytest.mark.gpu

MEAN_BGR = np.asarray([103.939, 116.779, 123.68]).astype(np.float32)
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "simil_cases.npz"))
ALL = ["p0"] + slc.NAMES
MODE = {"f16": 0, "f16x3": 1, "f16m8": 2, "f16x3p": 3}


@pytest.fixture(scope="module")
def sn(gpu_required):
    import surfacenet_amd
    return surfacenet_amd


@pytest.fixture(scope="module")
def dbg(sn):
    from surfacenet_amd import _lib
    lib = ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libsurfacenet_hip_dbg.so"))
    lib.sn_debug_simil_info.restype = lib.sn_debug_simil_tensor.restype = lib.sn_debug_plan.restype = ctypes.c_int
    lib.sn_debug_simil_info.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p]
    lib.sn_debug_simil_tensor.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
    lib.sn_debug_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    lib.sn_last_error.restype = ctypes.c_char_p
    return lib


@functools.lru_cache(maxsize=None)
def values():
    from surfacenet_amd import weights
    return weights.synthetic_simil_param_values(1)


@functools.lru_cache(maxsize=None)
def patches(n):
    """As test_patch2embedding_vs_oracle: random u8 patches, one all-black, one smooth; preprocessed. Shared: nobody writes to it."""
    raw = np.random.RandomState(100 + n).randint(0, 256, (n, 64, 64, 3)).astype(np.uint8)
    raw[0] = 0
    if n > 1:
        raw[1] = (np.indices((64, 64)).sum(0)[:, :, None] * [1, 2, 3] % 256).astype(np.uint8)
    return so.preprocess(raw, MEAN_BGR)


@functools.lru_cache(maxsize=None)
def references(n, quant):
    """(exact, ref) of patches(n), computed once per patch count and arithmetic class and shared by the tests that need them."""
    return slc.references(patches(n), values(), "f16" if quant == "fp16" else "f16x3")


def info_of(ctx, dbg, name):
    out = np.zeros(8, dtype=np.int64)
    assert dbg.sn_debug_simil_info(ctx._h, name.encode(), out.ctypes.data_as(ctypes.c_void_p)) == 0, dbg.sn_last_error()
    return sd.Info.from_info(out)


def read_back(ctx, dbg, names=ALL, first=0, count=None):
    """-> name -> (raw bytes of patches [first, first + count), Info); feat / emb: raw is the (count, L) float32 array."""
    out = {}
    for name in names:
        info = info_of(ctx, dbg, name)
        cnt = info.n - first if count is None else count
        if name in ("feat", "emb"):
            raw = np.empty((cnt, info.cs), dtype=np.float32)
        else:
            raw = np.empty(info.bytes_of(cnt), dtype=np.uint8)
        assert dbg.sn_debug_simil_tensor(ctx._h, name.encode(), first, cnt, raw.ctypes.data_as(ctypes.c_void_p), raw.nbytes) == 0, dbg.sn_last_error()
        out[name] = (raw, info)
    return out


def check_infos(rb, n, cap, precision):
    """What sn_debug_simil_info says against simil_carve's arithmetic restated in simil_decode.layout."""
    planes = 1 if precision == "f16" else 2
    _, _, maps = sd.layout(cap, planes)
    for name, (_, info) in rb.items():
        assert (info.n, info.cap) == (n, cap), (name, info.n, info.cap)
        if name in ("feat", "emb"):
            assert (info.H, info.cs, info.planes, info.lo, info.nbytes) == (0, sd.FEAT if name == "feat" else sd.EMB, 1, -1, n * info.cs * 4), name
            continue
        _, lo, C, H = maps[slc.buffer_of(name)]
        assert (info.H, info.cs, info.planes, info.lo, info.nbytes) == (H, C, planes, lo, planes * C * n * H * H * 2), name


def decode_all(rb, X, precision):
    """-> (dec, halfs): name -> fp64 tensor of the patches read; name -> the stored halfs / float32 rows themselves (bit comparisons).
    Judges p0 on the way."""
    dec, halfs = {}, {}
    for name, (raw, info) in rb.items():
        if name in ("feat", "emb"):
            dec[name], halfs[name] = raw.astype(np.float64), raw
            continue
        count = raw.size // info.bytes_of(1)
        C = 3 if name == "p0" else slc.CHANNELS[name]
        dec[name], pad, halfs[name] = sd.decode(raw, info, count, C)
        assert np.isfinite(halfs[name].astype(np.float32)).all(), name
        if name == "p0":
            slc.check_p0(dec[name], pad, X, precision)
    return dec, halfs


def tables(dec, exact, ref, precision, title, sample_of=None):
    g = slc.global_table(dec, exact, ref, title + ": stored tensors against the fp64 oracle", sample_of=sample_of)
    loc = slc.local_table(dec, values(), precision, title + ": each launch against the fp64 step on its own stored input")
    return slc.failing(g, loc)


def same_bits(a, b, what):
    for name in a:
        x, y = a[name], b[name]
        assert x.shape == y.shape and np.array_equal(x.view(np.uint16 if x.dtype == np.float16 else np.uint32),
                                                     y.view(np.uint16 if y.dtype == np.float16 else np.uint32)), (what, name)


def per_patch(h, order):
    """stored halfs (planes, count, cs, H, H) / rows (count, L) re-ordered along the patch axis."""
    return np.ascontiguousarray(h[order] if h.ndim == 2 else h[:, order])


@pytest.mark.parametrize("precision", ["f16x3", "f16"])
@pytest.mark.parametrize("n", [1, 9, 17])
def test_every_stored_tensor_and_every_launch(sn, dbg, n, precision):
    t0 = time.time()
    X = patches(n)
    with sn.Context(cube_D=8, max_samples=2, precision=precision) as ctx:
        ctx.load_simil_param_values(values())
        got = ctx.patch2embedding(X)
        rb = read_back(ctx, dbg)
        if n > 1:
            ctx.patch2embedding(np.ascontiguousarray(X[::-1]))
            rb_rev = read_back(ctx, dbg)
    t_gpu = time.time() - t0
    check_infos(rb, n, max(n, 8), precision)
    dec, halfs = decode_all(rb, X, precision)
    assert np.array_equal(halfs["emb"], got)
    if n > 1:
        # no halo along x, whatever the tile: a patch's tensors do not depend on its neighbours nor on its place in the batch
        _, halfs_rev = decode_all(rb_rev, X[::-1], precision)
        order = np.arange(n)[::-1]
        same_bits(halfs, {k: per_patch(v, order) for k, v in halfs_rev.items()}, "batch reversed")
    exact, ref = references(n, slc.quant_of(precision))
    bad = tables(dec, exact, ref, precision, "n %d, %s" % (n, precision))
    print("  wall time: device + read-back %.2f s, oracle %.1f s" % (t_gpu, time.time() - t0 - t_gpu))
    assert bad == ([], []), bad


def test_every_mode_but_f16_runs_this_network_in_f16x3(sn, dbg):
    """f16m8 and f16x3p contexts (simil_mode): every stored tensor bit-identical to the f16x3 context's, n = 9."""
    t0 = time.time()
    X = patches(9)
    got = {}
    for precision in ("f16x3", "f16m8", "f16x3p"):
        with sn.Context(cube_D=8, max_samples=2, precision=precision) as ctx:
            ctx.load_simil_param_values(values())
            ctx.patch2embedding(X)
            rb = read_back(ctx, dbg)
        check_infos(rb, 9, 9, precision)
        got[precision] = decode_all(rb, X, precision)[1]
    same_bits(got["f16x3"], got["f16m8"], "f16m8")
    same_bits(got["f16x3"], got["f16x3p"], "f16x3p")
    print("  wall time: device + read-back %.2f s, oracle 0 s" % (time.time() - t0))


def assert_every_layer_walks(dbg, precision, n):
    """The tile walk's precondition, from the plan rows (sn_debug_plan: name cin cout ks dil k2d nf nsplit ...) and the device's CU count:
    B * tiles_x * tiles_y * tiles_z > resident = num_cus * WG_PER_CU / nsplit for every layer. Tile shapes (conv3d_mfma.h ConvCfg): the
    similarityNet's kernels are 8-wave workgroups (WG_PER_CU = 1) of 8 patches x 8 x 8 pixels; those of the 4x4 maps (K2D = 2) 16 images x 4 x 4."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    buf = ctypes.create_string_buffer(8192)
    assert dbg.sn_debug_plan(1, MODE[precision], -1, buf, len(buf)) == 0, dbg.sn_last_error()
    rows = [r.split() for r in buf.value.decode().strip().split("\n")]
    assert [r[0] for r in rows] == slc.LAYERS
    for i, r in enumerate(rows):
        nsplit = int(r[7])
        H = 64 >> sum(1 for p in so.POOL_AFTER if p < i)
        tx, t = (16, 4) if H == 4 else (8, 8)
        tiles = -(-n // tx) * (H // t) ** 2
        resident = max(1, cus // nsplit)
        assert tiles > resident, "%s: %d tiles do not exceed the %d resident workgroups of this %d-CU device: n = %d walks no second tile" % (r[0], tiles, resident, cus, n)


@pytest.mark.parametrize("precision", ["f16x3", "f16"])
def test_tile_walk_against_the_oracle(sn, dbg, precision):
    """n = 1033 patches made of 13 distinct ones (13 is coprime with 8 and 16: every content lands in every tile position).
    (a) patches 0..12, read back with the range form of the hook, pass both tables; (b) pool1 .. pool5, feat and emb of ALL patches: patch i
    is bit-identical to patch i mod 13."""
    n, k = 1033, 13
    assert_every_layer_walks(dbg, precision, n)
    t0 = time.time()
    X13 = patches(k)
    idx = np.arange(n) % k
    X = np.ascontiguousarray(X13[idx])
    with sn.Context(cube_D=8, max_samples=2, precision=precision) as ctx:
        ctx.load_simil_param_values(values())
        got = ctx.patch2embedding(X)
        t_dev = time.time() - t0
        rb = read_back(ctx, dbg, count=k)
        t1 = time.time()
        full = read_back(ctx, dbg, names=slc.POOLS + ["feat", "emb"])
        t_full = time.time() - t1
    t_gpu = time.time() - t0
    check_infos(rb, n, n, precision)
    assert np.array_equal(full["emb"][0], got)
    for name, (raw, info) in full.items():
        if name in ("feat", "emb"):
            r = raw.view(np.uint32)
            assert r.shape[0] == n and np.array_equal(r, r[idx]), name
        else:
            r = raw.view(np.uint16).reshape(info.planes, info.cs // 8, n, -1)      # as the hook packs them: [planes][C/8][n][H][H][8]
            assert np.array_equal(r, r[:, :, idx]), name
            # (the range form and the whole-tensor form of the hook hand out the same bytes for patches 0..12 - the ones the tables judge)
            assert np.array_equal(r[:, :, :k], rb[name][0].view(np.uint16).reshape(info.planes, info.cs // 8, k, -1)), name
    dec, _ = decode_all(rb, X13, precision)
    exact, ref = references(k, slc.quant_of(precision))
    bad = tables(dec, exact, ref, precision, "n %d (13 distinct patches), %s, patches 0..12" % (n, precision))
    print("  wall time: upload + device %.2f s, read-back %.2f s (of which all %d patches of pool1..5, feat, emb: %.2f s, %.0f MB), oracle %.1f s"
          % (t_dev, t_gpu - t_dev, n, t_full, sum(v[0].nbytes for v in full.values()) / 1e6, time.time() - t0 - t_gpu))
    assert bad == ([], []), bad


def test_crop_route_leaves_the_same_tensors_as_crop_then_embed(sn, dbg):
    """sn_crop_embed (patch_crop_kernel writes p0; the embeddings go to the call's own buffer, which is where the hook reads "emb" from)
    against patch2embedding(preprocess(crop_patches(...))) on the same 9 centres, some outside the image: every stored tensor bit-identical."""
    t0 = time.time()
    H, W = (int(v) for v in G["sc_hw"])
    imgs = [golden_util.synth_image(int(s), H, W) for s in G["sc_seeds"]]
    rs = np.random.RandomState(4)
    ch, cw = rs.uniform(-20, H + 20, 9), rs.uniform(-20, W + 20, 9)
    ch[:3], cw[:3] = [-15.0, H + 10.0, H / 2], [W / 2, -3.5, W + 19.0]
    with sn.Context(cube_D=8, max_samples=2) as ctx:
        ctx.set_images(imgs)
        ctx.load_simil_param_values(values())
        emb_a = ctx.crop_embed(0, ch, cw, MEAN_BGR)
        rb_a = read_back(ctx, dbg)
        X = so.preprocess(ctx.crop_patches(0, ch, cw), MEAN_BGR)
        emb_b = ctx.patch2embedding(X)
        rb_b = read_back(ctx, dbg)
    check_infos(rb_a, 9, 9, "f16x3")
    a, b = decode_all(rb_a, X, "f16x3")[1], decode_all(rb_b, X, "f16x3")[1]
    same_bits(a, b, "crop route")
    assert np.array_equal(a["emb"], emb_a) and np.array_equal(b["emb"], emb_b)
    assert np.array_equal(X, so.preprocess(so.crop_patches(imgs[0], ch, cw), MEAN_BGR))
    print("  wall time: device + read-back %.2f s, oracle 0 s" % (time.time() - t0))


def test_stale_workspace_after_a_larger_run(sn, dbg):
    """n = 9 after n = 1033 in the same context: the workspace is kept (capacity 1033), the planes' group stride is now 9. Same tables as a
    fresh context, tensors bit-identical to the fresh run's."""
    t0 = time.time()
    X = patches(9)
    with sn.Context(cube_D=8, max_samples=2) as ctx:
        ctx.load_simil_param_values(values())
        ctx.patch2embedding(np.ascontiguousarray(patches(13)[np.arange(1033) % 13]))
        ctx.patch2embedding(X)
        rb = read_back(ctx, dbg)
    with sn.Context(cube_D=8, max_samples=2) as ctx:
        ctx.load_simil_param_values(values())
        ctx.patch2embedding(X)
        rb_fresh = read_back(ctx, dbg)
    t_gpu = time.time() - t0
    check_infos(rb, 9, 1033, "f16x3")
    check_infos(rb_fresh, 9, 9, "f16x3")
    dec, halfs = decode_all(rb, X, "f16x3")
    same_bits(halfs, decode_all(rb_fresh, X, "f16x3")[1], "stale workspace")
    exact, ref = references(9, "x3")
    bad = tables(dec, exact, ref, "f16x3", "n 9 after n 1033 in the same context, f16x3")
    print("  wall time: device + read-back %.2f s, oracle %.1f s" % (t_gpu, time.time() - t0 - t_gpu))
    assert bad == ([], []), bad


def test_debug_simil_hook_refuses_what_it_cannot_serve(sn, dbg):
    t0 = time.time()
    out = np.zeros(8, np.int64)
    buf = np.zeros(1 << 20, np.uint8)
    info = lambda ctx, name: dbg.sn_debug_simil_info(ctx._h, name, out.ctypes.data_as(ctypes.c_void_p))
    tensor = lambda ctx, name, first, count, nbytes: dbg.sn_debug_simil_tensor(ctx._h, name, first, count, buf.ctypes.data_as(ctypes.c_void_p), nbytes)
    H, W = (int(v) for v in G["sc_hw"])
    with sn.Context(cube_D=8, max_samples=2) as ctx:
        ctx.load_simil_param_values(values())
        assert info(ctx, b"p0") != 0 and b"no similarityNet run" in dbg.sn_last_error()
        ctx.patch2embedding(patches(2))
        assert info(ctx, b"s_conv6_1") != 0 and b"unknown tensor" in dbg.sn_last_error()
        assert info(ctx, b"s_conv5_3") == 0 and list(out[:7]) == [2, 512, 2, 512 * 2 * 2 * 8, 2, 8, 2 * 512 * 2 * 2 * 2 * 2]
        per = 2 * 512 * 2 * 2 * 2
        assert tensor(ctx, b"s_conv5_3", 1, 1, per) == 0
        assert tensor(ctx, b"s_conv5_3", 1, 2, 2 * per) != 0 and b"beyond" in dbg.sn_last_error()
        assert tensor(ctx, b"s_conv5_3", -1, 1, per) != 0 and b"beyond" in dbg.sn_last_error()
        assert tensor(ctx, b"s_conv5_3", 0, 2, 2 * per + 2) != 0 and b"asked for" in dbg.sn_last_error()
        assert tensor(ctx, b"emb", 0, 2, 2 * 128 * 4 - 4) != 0 and b"asked for" in dbg.sn_last_error()
        # the workspace re-made for another mode without a run in it: what the last run left is gone
        ctx.set_images([golden_util.synth_image(1, H, W)])
        assert ctx._lib.sn_set_precision(ctx._h, 0) == 0
        ctx.crop_patches(0, np.asarray([H / 2.0]), np.asarray([W / 2.0]))
        assert info(ctx, b"p0") != 0 and b"re-made" in dbg.sn_last_error()
        ctx.patch2embedding(patches(2))
        assert info(ctx, b"s_conv5_3") == 0 and list(out[:7]) == [2, 512, 1, -1, 2, 8, 512 * 2 * 2 * 2 * 2]
    print("  wall time: device + read-back %.2f s, oracle 0 s" % (time.time() - t0))
