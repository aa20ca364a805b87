"""GPU (-m gpu): the small kernels around the network - cvc_warp_kernel, fuse_kernel, color_fuse_kernel, d2s_count / d2s_write, ray_pool_kernel's listing
loops, project_points_kernel - against the restatements of oracle/ on the inputs of tests/hotloop_cases.py: cube sizes 12 and 20 (s^3 no multiple of a
workgroup, so every launch ends in a ragged one) and the edges tests/test_hotloop_cpu.py asserts present. Bit for bit (the fusion also within its derived
bound of float64; the projection with NaN equal to NaN where q2 == 0), every result computed twice with equal bytes, host-array form and device form."""
import numpy as np
import pytest

import hotloop_cases as hc
from oracle import cvc_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sn(gpu_required):
    import surfacenet_amd
    return surfacenet_amd


def _bytes(r):
    return tuple(None if a is None else np.ascontiguousarray(a).tobytes() for a in (r if isinstance(r, (tuple, list)) else (r,)))


def _twice(run):
    """Two runs with equal bytes -> the first result."""
    a, b = run(), run()
    assert _bytes(a) == _bytes(b)
    return a


class _Staged(object):
    """Device buffers, freed on exit: up() copies a host array, room() only allocates, down() fetches."""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def room(self, nbytes):
        self.bufs.append(self.ctx.dev_alloc(max(int(nbytes), 16)))
        return self.bufs[-1]

    def up(self, a, offset=0):
        a = np.ascontiguousarray(a)
        p = self.room(a.nbytes + offset) + offset
        self.ctx.h2d(p, a)
        return p

    def down(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        if out.nbytes:
            self.ctx.d2h(out, p)
        else:
            self.ctx.synchronize()
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.bufs:
            self.ctx.dev_free(p)


@pytest.fixture(scope="module")
def net_values():
    import synth
    return list(synth.calibrated_params(1))


# ---------------------------------------------------------------------------------------------------------------------- 1. the CVC warp
@pytest.mark.parametrize("s", hc.SIZES)
def test_cvc_warp_mixed_views_ties_and_planes(sn, net_values, s):
    from surfacenet_amd import _lib
    c = hc.cvc_case(s)
    n, n_vp = c["pairs"].shape[:2]
    args = (c["pairs"], c["xyz"], c["resol"])
    want_raw = cvc_oracle.gen_coloredCubes(*args, c["cams"], c["imgs"], s)
    want_pre = cvc_oracle.gen_coloredCubes(*args, c["cams"], c["imgs"], s, mean6=hc.MEAN6)
    assert want_raw.shape == (n * n_vp, 6, s, s, s)
    with sn.Context(cube_D=s, max_samples=16) as ctx:
        ctx.set_cameras(c["cams"]); ctx.set_images(list(c["imgs"]))
        assert _twice(lambda: ctx.cvc(*args)).tobytes() == want_raw.tobytes()
        assert _twice(lambda: ctx.cvc(*args, mean=hc.MEAN6)).tobytes() == want_pre.tobytes()
        with _Staged(ctx) as st:                                  # device form: the negative view ids reach the kernel as they are
            d_in = [st.up(a) for a in args]
            d_out = st.room(want_raw.nbytes)
            for mean, want in ((None, want_raw), (hc.MEAN6, want_pre)):
                def run():
                    ctx.h2d(d_out, np.full(want.shape, 7, np.float32))
                    _lib.check(ctx._lib.sn_cvc_dev(ctx._h, n, n_vp, *d_in, _lib.ptr(mean), d_out))
                    return st.down(d_out, want.shape, np.float32)
                assert _twice(run).tobytes() == want.tobytes()
    w = np.full((n, n_vp), 1.0 / n_vp, np.float32)
    with sn.Context(cube_D=s, max_samples=hc.CVC_MAX_SAMPLES) as ctx:       # 3 cubes of 3 samples through a 7-sample workspace: chunks of 2 cubes and 1
        ctx.set_cameras(c["cams"]); ctx.set_images(list(c["imgs"])); ctx.load_param_values(net_values)
        assert _twice(lambda: ctx.cvc(*args)).tobytes() == want_raw.tobytes()
        assert _twice(lambda: ctx.cvc(*args, mean=hc.MEAN6)).tobytes() == want_pre.tobytes()
        fused, unfused, cvc = _twice(lambda: ctx.cvc_forward(*args, w, mean=hc.MEAN6, return_cvc=True))
    assert cvc.tobytes() == want_pre.tobytes()
    assert np.isfinite(unfused).all() and fused.shape == (n, 1, s, s, s)


# ---------------------------------------------------------------------------------------------------------------------- 2. the fusion
@pytest.mark.parametrize("s,n_vp", hc.FUSE_CASES)
def test_fusion_equals_its_float32_restatement(sn, net_values, s, n_vp):
    """fused == the float32 restatement of fuse_kernel applied to the unfused probabilities the same call returned, and within hc.fuse_bound of their float64
    weighted mean (the figures are printed; profiles/hotloop/README.md records them)."""
    import synth
    from surfacenet_amd import _lib
    n = hc.FUSE_N
    X = synth.random_cvc(n * n_vp, s, 40 + n_vp)
    w = hc.fuse_weights(n_vp)
    with sn.Context(cube_D=s, max_samples=n * n_vp) as ctx:
        ctx.load_param_values(net_values)
        fused, unfused = _twice(lambda: ctx.forward(X, w, n_vp=n_vp))
        with _Staged(ctx) as st:
            d_X, d_w, d_f, d_u = st.up(X), st.up(w), st.room(fused.nbytes), st.room(unfused.nbytes)

            def run():
                _lib.check(ctx._lib.sn_forward_dev(ctx._h, n, n_vp, d_X, d_w, d_f, d_u))
                return st.down(d_f, fused.shape, np.float32), st.down(d_u, unfused.shape, np.float32)
            fused_dev, unfused_dev = _twice(run)
    with sn.Context(cube_D=s, max_samples=n_vp + 1) as ctx:       # one cube per chunk
        ctx.load_param_values(net_values)
        fused_1, unfused_1 = ctx.forward(X, w, n_vp=n_vp)
    assert unfused.shape == (n, n_vp, s, s, s) and 0 < unfused.min() and unfused.max() < 1 and unfused.max() - unfused.min() > 0.01
    assert fused.tobytes() == hc.fuse_restatement(unfused, w).tobytes()
    assert unfused_dev.tobytes() == unfused.tobytes() and fused_dev.tobytes() == fused.tobytes()
    assert unfused_1.tobytes() == unfused.tobytes() and fused_1.tobytes() == fused.tobytes()
    dev, bound = float(np.abs(fused.astype(np.float64) - hc.fuse_float64(unfused, w)).max()), hc.fuse_bound(unfused, n_vp)
    print("fusion vs float64, s %d n_vp %d: %.3e, bound %.3e (%.2f of it)" % (s, n_vp, dev, bound, dev / bound))
    assert dev <= bound


@pytest.mark.parametrize("s", hc.SIZES)
def test_fusion_of_one_pair_is_a_copy(sn, net_values, s):
    import synth
    X = synth.random_cvc(3, s, 5)
    with sn.Context(cube_D=s, max_samples=4) as ctx:
        ctx.load_param_values(net_values)
        for w in (None, np.zeros((3, 1), np.float32), np.full((3, 1), np.nan, np.float32), np.full((3, 1), 1e30, np.float32)):
            fused, unfused = _twice(lambda: ctx.forward(X, w, n_vp=1))
            assert fused.tobytes() == unfused.tobytes() and np.isfinite(fused).all()


# ---------------------------------------------------------------------------------------------------------------------- 3. the colour fusion
@pytest.mark.parametrize("n_vp", hc.COLOR_NVP)
def test_color_fusion_classes(sn, n_vp):
    c = hc.color_case(n_vp)
    s, n = hc.COLOR_S, hc.COLOR_N
    want = cvc_oracle.color_fuse(c["X"] + hc.MEAN6[None, :, None, None, None], c["pred"], c["w"])
    with sn.Context(cube_D=s, max_samples=4) as ctx:
        got = _twice(lambda: ctx.color_fuse(c["X"], c["pred"], c["w"], mean=hc.MEAN6))
        with _Staged(ctx) as st:
            d_in = [st.up(c["X"]), st.up(c["pred"]), st.up(c["w"])]
            d_rgb = st.up(np.full(want.shape, 7, np.uint8))

            def run():
                ctx.color_fuse_dev(n, n_vp, *d_in, d_rgb, mean=hc.MEAN6)
                return st.down(d_rgb, want.shape, np.uint8)
            dev = _twice(run)
    assert got.dtype == np.uint8 and got.shape == (n, 3, s, s, s)
    assert got.tobytes() == want.tobytes() and dev.tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------------------------------- 4. dense2sparse
def _d2s_equal(got, want, rgb, pooling):
    off, ijk, p16, rgb_out, votes = got
    assert np.array_equal(off, want["offsets"])
    assert ijk.tobytes() == want["ijk"].tobytes() and np.asarray(p16).view(np.uint16).tobytes() == want["pred"].view(np.uint16).tobytes()
    assert (rgb_out is None) if not rgb else rgb_out.tobytes() == want["rgb"].tobytes()
    assert (votes is None) if not pooling else votes.tobytes() == want["votes"].tobytes()


@pytest.mark.parametrize("D,dcenter", hc.D2S_GEOMETRY)
def test_dense2sparse_threshold_edges_and_empty_ends(sn, D, dcenter):
    c = hc.d2s_case(D, dcenter)
    n, n_vp, dc = hc.D2S_N, hc.D2S_NVP, c["dc"]
    cap = n * dc ** 3
    with sn.Context(cube_D=D, max_samples=4) as ctx:
        ctx.set_cameras(c["cams"])
        with _Staged(ctx) as st:
            d_pairs, d_xyz, d_resol, d_pred, d_rgb = (st.up(c[k]) for k in ("pairs", "xyz", "resol", "pred", "rgb"))       # pred: float32, not yet fp16
            d_vws = st.room(n * D ** 3)
            d_off, d_ijk, d_p16, d_rgbo, d_votes = st.room((n + 1) * 8), st.room(cap * 3), st.room(cap * 2), st.room(cap * 3), st.room(cap)
            for rgb, pooling, thresh in hc.D2S_CONFIGS:
                want = hc.d2s_want(D, dcenter, pooling, thresh)
                kw = dict(min_prob=hc.D2S_MIN_PROB, rayPool_thresh=thresh, enable_centerCrop=dcenter is not None, cube_Dcenter=dcenter,
                          enable_rayPooling=pooling)
                host = _twice(lambda: ctx.dense2sparse(c["pred"], c["rgb"] if rgb else None, c["pairs"], c["xyz"], c["resol"], **kw))
                _d2s_equal(host, want, rgb, pooling)

                def run():
                    ctx.dense2sparse_dev(n, n_vp, d_pairs, d_xyz, d_resol, d_pred, d_rgb, d_vws, d_off, d_ijk, d_p16, d_rgbo if rgb else None,
                                         d_votes if pooling else None, **kw)
                    off = st.down(d_off, (n + 1,), np.int64)
                    T = int(off[-1])
                    assert 0 <= T <= cap
                    return (off, st.down(d_ijk, (T, 3), np.uint8), st.down(d_p16, (T,), np.uint16), st.down(d_rgbo, (T, 3), np.uint8) if rgb else None,
                            st.down(d_votes, (T,), np.uint8) if pooling else None)
                _d2s_equal(_twice(run), want, rgb, pooling)


# ---------------------------------------------------------------------------------------------------------------------- 5. ray pooling
@pytest.mark.parametrize("D,thresh", hc.RP_CASES)
def test_ray_pool_listing_loops(sn, D, thresh):
    """The 16-byte listing loop on a cube shorter than one trip of it, and the scalar loop, which runs when the predictions are not 16-byte aligned. The
    votes stay 4-byte aligned: rp_vote adds whole words (include/surfacenet_hip.h)."""
    c = hc.rp_case(D, thresh)
    want = hc.rp_want(D, thresh)
    n, n_vp = hc.RP_N, hc.RP_NVP
    args = (c["pairs"], c["xyz"], c["resol"])
    with sn.Context(cube_D=D, max_samples=4) as ctx:
        ctx.set_cameras(c["cams"])
        host = _twice(lambda: ctx.ray_pool(*args, c["pred"], thresh))
        assert host.dtype == np.uint8 and host.tobytes() == want.tobytes()
        with _Staged(ctx) as st:
            d_in = [st.up(a) for a in args]
            d_votes = st.room(want.nbytes)
            got = {}
            for offset in (0, 4):
                d_pred = st.up(c["pred"], offset=offset)
                assert d_pred % 16 == offset and d_votes % 4 == 0

                def run():
                    ctx.h2d(d_votes, np.full(want.shape, 7, np.uint8))
                    ctx.ray_pool_dev(n, n_vp, *d_in, d_pred, d_votes, prediction_thresh=thresh)
                    return st.down(d_votes, want.shape, np.uint8)
                got[offset] = _twice(run)
                assert got[offset].tobytes() == want.tobytes(), offset
            assert got[0].tobytes() == got[4].tobytes()


# ---------------------------------------------------------------------------------------------------------------------- 6. the projection
@pytest.mark.parametrize("V", hc.PROJ_V)
@pytest.mark.parametrize("n", hc.PROJ_N)
def test_project_points_sizes_ties_and_the_plane_q2_0(sn, n, V):
    from surfacenet_amd import _lib
    P, pts = hc.proj_cameras(V), hc.proj_points(n)
    h, w = cvc_oracle.perspectiveProj(P, pts, return_int_hw=False)
    q2 = np.stack([hc.numerators(P[v], pts)[2] for v in range(V)])
    assert np.array_equal(np.isnan(h) | np.isnan(w) | np.isinf(h) | np.isinf(w), q2 == 0)      # the only places NaN is compared with NaN
    same = lambda a, b: a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)

    def c_entry(ctx, M, round_int, depth):
        out = [np.full((V, n), 7.0), np.full((V, n), 7.0), np.full((V, n), 7.0) if depth else None]
        _lib.check(ctx._lib.sn_project_points(ctx._h, V if M is not None else 0, _lib.ptr(M), n, _lib.ptr(pts), round_int, *(_lib.ptr(o) for o in out)))
        return tuple(out)

    def check(ctx, M):
        for depth in (False, True):
            got = _twice(lambda: ctx.project(pts, M, return_int_hw=False, return_depth=depth))
            assert same(got[0], h) and same(got[1], w) and (not depth or same(got[2], q2))
            for round_int, (eh, ew) in ((0, (h, w)), (1, (np.rint(h), np.rint(w)))):
                got = _twice(lambda: c_entry(ctx, M, round_int, depth))
                assert same(got[0], eh) and same(got[1], ew) and (got[2] is None if not depth else same(got[2], q2))

    with sn.Context(cube_D=8, max_samples=1) as ctx:
        ctx.set_cameras(np.zeros((2, 3, 4)))                       # bound, but not the cameras in use when P is given
        check(ctx, P)
        ctx.set_cameras(P)                                         # P = None: the cameras of sn_set_cameras
        check(ctx, None)
