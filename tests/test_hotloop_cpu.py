"""CPU: the premises of tests/test_gpu_hotloop.py, checked with the restatements of oracle/ alone. Every edge class tests/hotloop_cases.py names is asserted
present in its inputs here, so a case that lost its edge fails here instead of passing vacuously on the GPU."""
import numpy as np
import pytest

import hotloop_cases as hc
from oracle import cvc_oracle, post_oracle


# ---------------------------------------------------------------------------------------------------------------------- 1. the CVC warp
@pytest.fixture(scope="module", params=hc.SIZES)
def cvc(request):
    c = hc.cvc_case(request.param)
    raw = cvc_oracle.gen_coloredCubes(c["pairs"], c["xyz"], c["resol"], c["cams"], c["imgs"], c["s"])
    return c, raw


def _slot(c, sample, side):
    """(q (3, s^3), u, v) of one (sample, side): the numerators and the unrounded pixel of every voxel."""
    cube, view = sample // hc.CVC_NVP, hc.cvc_views(c)[sample, side]
    pts = hc.grid(c["xyz"][cube], c["resol"][cube], c["s"])
    q = hc.numerators(c["cams"][view], pts)
    v, u = cvc_oracle.perspectiveProj(c["cams"][view], pts, return_int_hw=False)
    return q, u[0], v[0]


def test_cvc_shapes_are_ragged_and_views_differ(cvc):
    c, raw = cvc
    s = c["s"]
    assert (s ** 3) % 256 != 0 and (s ** 3) % 1024 != 0 and s ** 3 > 256
    assert [im.shape for im in c["imgs"]] == [(h, w, 3) for h, w in hc.IMG_HW] == [(9, 14, 3), (1, 1, 3), (37, 5, 3), (1200, 1600, 3), (2, 3, 3)]
    assert all(im.min() >= 1 for im in c["imgs"])                         # in scope <=> coloured, for the shares below
    assert c["pairs"].shape == (hc.CVC_N, hc.CVC_NVP, 2) == (3, 3, 2) and len(c["cams"]) >= 5
    assert set(c["pairs"][c["pairs"] < 0]) == set(range(-5, 0))           # -1 .. -V
    assert any(a == b for a, b in c["pairs"].reshape(-1, 2))              # a pair (a, a)
    assert np.bincount(hc.cvc_views(c).reshape(-1)).max() >= 3            # a repeated view
    assert set(hc.cvc_views(c).reshape(-1)) == set(range(5))              # every image size is read
    assert np.array_equal(c["cams"][hc.V_DTU], hc.golden_util.cameras()["P_dtu"][0])
    n_all = hc.CVC_N * hc.CVC_NVP
    assert hc.CVC_MAX_SAMPLES < n_all and 0 < n_all % (hc.CVC_MAX_SAMPLES // hc.CVC_NVP * hc.CVC_NVP) < n_all     # chunked, the last chunk short


def test_cvc_tie_plane(cvc):
    c, raw = cvc
    s = c["s"]
    q, u, v = _slot(c, *c["tie"])
    assert hc.cvc_views(c)[c["tie"]] == hc.V_TIE and np.all(q[2] == 1)
    ties = np.modf(np.abs(u))[0] == 0.5
    assert ties.sum() >= s * s
    even = np.rint(u[ties])
    assert np.all(even % 2 == 0) and len(set(even)) > 3                   # half-to-even, downwards as well as upwards
    inside = ties & (np.rint(u) >= 0) & (np.rint(u) < 14) & (v >= 0) & (v < 9)
    assert inside.sum() >= s and (u[inside] < 0).any()                    # -0.5 -> -0 is column 0
    got = raw[c["tie"][0], 3 * c["tie"][1]].reshape(-1)
    assert np.array_equal(got[inside], c["imgs"][hc.V_TIE][v[inside].astype(int), np.rint(u[inside]).astype(int), 0])
    up = np.floor(u + 0.5)                                                # rounding half up instead reads other pixels: the comparison can fail
    both = inside & (up >= 0) & (up < 14)
    assert (c["imgs"][hc.V_TIE][v[both].astype(int), up[both].astype(int), 0] != got[both]).sum() >= s


def test_cvc_zero_plane_and_behind_the_camera(cvc):
    c, raw = cvc
    s = c["s"]
    sample, side = c["zero_plane"]
    q, u, v = _slot(c, sample, side)
    plane = q[2] == 0
    assert plane.sum() == s * s and (q[2] < 0).any() and (q[2] > 0).any()
    assert not np.isfinite(u[plane]).any()
    assert not raw[sample, 3 * side:3 * side + 3].reshape(3, -1)[:, plane].any()
    for side in (0, 1):                                                   # (V_NEG, V_NEG) on the cube in Z > 0
        q, u, v = _slot(c, c["behind"], side)
        assert hc.cvc_views(c)[c["behind"], side] == hc.V_NEG and np.all(q[2] < 0)
        coloured = raw[c["behind"], 3 * side].reshape(-1) != 0
        assert 0 < coloured.sum() < s ** 3


def test_cvc_pixels_beyond_int32(cvc):
    c, raw = cvc
    far = [(sa, si) for sa in range(9) for si in (0, 1) if hc.cvc_views(c)[sa, si] == hc.V_FAR]
    assert far
    for sa, si in far:
        q, u, v = _slot(c, sa, si)
        assert (u > 2.0 ** 31).any() and (u < -2.0 ** 31).any()
        assert not raw[sa, 3 * si].reshape(-1)[np.abs(u) > 2.0 ** 31].any()


def test_cvc_every_slot_is_partly_in_scope(cvc):
    c, raw = cvc
    share = (raw.reshape(9, 2, 3, -1)[:, :, 0] != 0).mean(axis=2)         # no slot is exempt: the designated ones are partly in scope as well
    assert np.all(share > 0) and np.all(share < 1), share


def test_cvc_numpy_restatement_agrees(cvc):
    c, raw = cvc
    with np.errstate(all="ignore"):
        ref = cvc_oracle.gen_coloredCubes_numpy(c["pairs"], c["xyz"], c["resol"], c["cams"], c["imgs"], c["s"])
    assert np.array_equal(ref, raw)


def test_mean_round_trip_is_exact():
    u = np.arange(256, dtype=np.float32)[:, None]
    m = hc.MEAN6[None, :]
    assert np.array_equal((u - m) + m, np.broadcast_to(u, (256, 6)))


# ---------------------------------------------------------------------------------------------------------------------- 2. the fusion
@pytest.mark.parametrize("s,n_vp", hc.FUSE_CASES)
def test_fuse_weight_rows_and_bound(s, n_vp):
    assert sorted(hc.FUSE_CASES) == sorted([(12, v) for v in (2, 3, 5, 6)] + [(20, 3)])
    w = hc.fuse_weights(n_vp)
    assert w.dtype == np.float32 and w.shape == (3, n_vp) and np.all(np.diff(w, axis=1) >= 0) and np.all(w >= 0)
    assert w[0, 0] == np.float32(1e-30) and w[0, -1] == np.float32(1e30) and (w[1] == 0).sum() == 1 and len(set(w[2])) == 1
    unfused = np.random.RandomState(n_vp).rand(3, n_vp, s, s, s).astype(np.float32)     # stand-in probabilities
    got = hc.fuse_restatement(unfused, w)
    assert got.dtype == np.float32 and got.shape == (3, 1, s, s, s)
    dev = float(np.abs(got.astype(np.float64) - hc.fuse_float64(unfused, w)).max())
    print("fusion restatement vs float64, s %d n_vp %d: %.3e, bound %.3e" % (s, n_vp, dev, hc.fuse_bound(unfused, n_vp)))
    assert 0 < dev <= hc.fuse_bound(unfused, n_vp)
    # the order matters to the bits: summing the other way round is a different function
    assert n_vp == 2 or not np.array_equal(got, hc.fuse_restatement(unfused[:, ::-1], w[:, ::-1]))
    # ... and so does the contraction the library is built without
    fma = np.zeros((s, s, s))
    for p in range(n_vp):
        fma = (fma + unfused[2, p].astype(np.float64) * np.float64(np.float32(w[2, p] / np.float32(w[2].sum(dtype=np.float32))))).astype(np.float32).astype(np.float64)
    if n_vp > 2:
        assert not np.array_equal(fma.astype(np.float32), got[2, 0])


def test_fuse_single_pair_is_a_copy():
    u = np.random.RandomState(1).rand(2, 1, 4, 4, 4).astype(np.float32)
    assert np.array_equal(hc.fuse_restatement(u, np.ones((2, 1), np.float32)), u)


# ---------------------------------------------------------------------------------------------------------------------- 3. the colour fusion
@pytest.mark.parametrize("n_vp", hc.COLOR_NVP)
def test_color_classes(n_vp):
    c = hc.color_case(n_vp)
    s, n = hc.COLOR_S, hc.COLOR_N
    assert (s, n, hc.COLOR_NVP) == (12, 3, (1, 3, 5)) and (n * s ** 3) % 256 != 0
    assert np.array_equal(c["X"] + hc.MEAN6[None, :, None, None, None], c["col"].astype(np.float32))
    colours = c["X"] + hc.MEAN6[None, :, None, None, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        f = cvc_oracle.color_fuse_float(colours, c["pred"], c["w"])
    out = cvc_oracle.color_fuse(colours, c["pred"], c["w"])
    assert len(np.unique(out)) > 100
    m = c["masks"]
    assert all(v.sum() >= 8 for v in m.values()) and sum(v.sum() for v in m.values()) == np.logical_or.reduce(list(m.values())).sum()
    pick = lambda a, k: np.moveaxis(a, 1, -1)[m[k]]                       # (voxels, channels | pairs)
    assert np.all(pick(c["pred"], "no_weight") == 0) and np.isnan(pick(f, "no_weight")).all() and np.all(pick(out, "no_weight") == 0)
    assert np.all((pick(c["pred"], "one_pair") != 0).sum(axis=1) == 1) and np.isfinite(pick(f, "one_pair")).all()
    half = pick(f, "half")
    assert np.all(np.modf(half)[0] == 0.5) and np.array_equal(pick(out, "half"), np.floor(half))
    pairs_used = (pick(c["pred"], "half") != 0).sum(axis=1)
    assert set(pairs_used) <= {1, 2} and (pairs_used == 1).sum() >= 8 and (n_vp == 1 or (pairs_used == 2).sum() >= 8)
    assert np.all(pick(f, "full") == 255) and np.all(pick(out, "full") == 255)
    slab = out[:, :, s - 1]                                               # every colour 255: the rounded weights decide
    assert set(np.unique(slab)) >= {254, 255} or n_vp == 1
    assert np.isnan(f).sum() >= 3 * 8 and np.all(out[np.isnan(f)] == 0)


# ---------------------------------------------------------------------------------------------------------------------- 4. dense2sparse
@pytest.mark.parametrize("D,dcenter", hc.D2S_GEOMETRY)
def test_d2s_classes_and_counts(D, dcenter):
    assert hc.D2S_GEOMETRY == ((12, None), (12, 7), (12, 1), (20, 13))
    c = hc.d2s_case(D, dcenter)
    lo, dc = c["lo"], c["dc"]
    T = dc ** 3
    assert (D, dcenter, lo, T) in ((12, None, 0, 1728), (12, 7, 2, 343), (12, 1, 5, 1), (20, 13, 3, 2197))
    assert np.float32(hc.D2S_MIN_PROB) != np.float32(hc.H07) and hc.H07_DOWN < hc.H07 < hc.H07_UP
    p16 = c["pred"].astype(np.float16)
    thr = p16.dtype.type(hc.D2S_MIN_PROB)
    for name, (values, kept) in hc.D2S_CLASSES.items():
        v16 = np.asarray(values, np.float32).astype(np.float16)
        with np.errstate(invalid="ignore"):
            assert np.all((v16 > thr) == kept), name
        if name in ("rounds_up", "rounds_down"):
            assert np.all(v16 == hc.H07) and all((np.float32(v) < np.float32(hc.H07)) == (name == "rounds_up") for v in values)
            assert any((np.float32(v) > np.float32(hc.D2S_MIN_PROB)) for v in hc.D2S_CLASSES["rounds_down"][0])    # a float32 comparison keeps these
        for cube in (hc.D2S_EMPTY_FIRST, hc.D2S_MIXED, hc.D2S_EMPTY_LAST):
            if kept and cube != hc.D2S_MIXED:
                continue
            i, j, k = c["planted"][(cube, name)]
            assert len(i) >= 8 and len(set(zip(i, j, k))) == len(i)
            got = c["pred"][cube, i, j, k]
            assert np.array_equal(got.view(np.uint32), np.resize(np.asarray(values, np.float32), len(i)).view(np.uint32))
            inside = np.all([(lo <= a) & (a < lo + dc) for a in (i, j, k)], axis=0)
            assert inside.all() if dc >= 6 else not inside.any()           # (a 1-voxel crop has no room: its classes lie around it)
    want = hc.d2s_want(D, dcenter, False, 0)
    counts = np.diff(want["offsets"])
    assert counts[hc.D2S_EMPTY_FIRST] == 0 and counts[hc.D2S_WHOLE] == T and counts[hc.D2S_ONE] == 1 and counts[hc.D2S_EMPTY_LAST] == 0
    assert dc == 1 or 8 <= counts[hc.D2S_MIXED] < T
    one = want["ijk"][want["offsets"][hc.D2S_ONE]]
    assert np.array_equal(one, [dc - 1] * 3)                               # the last voxel of the crop
    assert np.isnan(c["pred"]).sum() >= 3 * 8
    crop = c["pred"][:, lo:lo + dc, lo:lo + dc, lo:lo + dc].reshape(hc.D2S_N, -1)
    with np.errstate(invalid="ignore"):                                   # a float32 comparison keeps other voxels: the comparison can fail
        assert dc == 1 or (crop > np.float32(hc.H07)).sum(axis=1)[hc.D2S_MIXED] > counts[hc.D2S_MIXED]
        assert dc == 1 or (crop > np.float32(hc.D2S_MIN_PROB)).sum(axis=1)[hc.D2S_EMPTY_FIRST] > 0
    # the vote rule keeps other voxels than the threshold rule, and fewer the higher it is
    n1, n4 = (np.diff(hc.d2s_want(D, dcenter, True, t)["offsets"]) for t in (1, 2 * hc.D2S_NVP))
    assert np.array_equal(np.diff(hc.d2s_want(D, dcenter, True, 0)["offsets"]), counts)
    assert n1[0] == n1[-1] == n4[0] == n4[-1] == 0 and np.all(n4 <= n1) and np.all(n1 <= counts)
    if dc >= 7:
        assert 0 < n4.sum() < n1.sum() < counts.sum()
    votes = hc.d2s_want(D, dcenter, True, 0)["votes"]
    assert votes.max() == 2 * hc.D2S_NVP and len(votes) == counts.sum()


def test_d2s_configs():
    assert sorted(hc.D2S_CONFIGS) == sorted((rgb, on, thr) for rgb in (False, True) for on, thr in ((False, 0), (True, 0), (True, 1), (True, 4)))


# ---------------------------------------------------------------------------------------------------------------------- 5. ray pooling
@pytest.mark.parametrize("D,thresh", hc.RP_CASES)
def test_rp_selection_and_votes(D, thresh):
    c = hc.rp_case(D, thresh)
    want = hc.rp_want(D, thresh)
    assert (hc.RP_N, hc.RP_NVP) == (3, 2) and sorted(set(d for d, _ in hc.RP_CASES)) == [12, 20] and {t for _, t in hc.RP_CASES} == {0.5, None}
    assert want.shape == (3, D, D, D) and want.any() and want.max() == 2 * hc.RP_NVP
    assert all(w.any() for w in want)
    p16 = c["pred"].astype(np.float16)
    assert c["pred"].dtype == np.float32 and c["pred"].min() >= 0 and not np.array_equal(p16.astype(np.float32), c["pred"])   # the kernel rounds to fp16 itself
    if thresh is None:
        assert (p16 == 0).mean() > 0.1 and D ** 3 <= 8192                 # every voxel is listed, zeros among them
    else:
        sel = (p16 > np.float16(thresh)).reshape(3, -1).sum(axis=1)
        assert np.all(sel > 0) and np.all(sel < D ** 3)
        assert not want[p16 <= np.float16(thresh)].any()
    assert (D ** 3) % 4 == 0 and D ** 3 < 8 * 4 * 1024 and (D ** 3) % (4 * 1024) != 0     # less than one trip of the 16-byte listing loop, ragged end


# ---------------------------------------------------------------------------------------------------------------------- 6. the projection
@pytest.mark.parametrize("V", hc.PROJ_V)
def test_proj_edges(V):
    assert hc.PROJ_N == (1, 255, 256, 257, 1000) and hc.PROJ_V == (1, 5)
    P = hc.proj_cameras(V)
    pts = hc.proj_points(1000)
    assert P.shape == (V, 3, 4)
    h, w = cvc_oracle.perspectiveProj(P, pts, return_int_hw=False)
    q2 = np.stack([hc.numerators(P[v], pts)[2] for v in range(V)])
    assert (q2 == 0).sum() >= 100 and np.array_equal(~np.isfinite(h), q2 == 0) and np.array_equal(~np.isfinite(w), q2 == 0)
    assert np.isnan(h).sum() >= 8 and np.isnan(w).sum() >= 8 and np.isinf(h).sum() >= 8 and np.isinf(w).sum() >= 8
    fin = np.isfinite(w)
    assert (np.modf(np.abs(w[fin]))[0] == 0.5).sum() >= 8 and (np.modf(np.abs(h[fin]))[0] == 0.5).sum() >= (8 if V == 1 else 0)
    for n in hc.PROJ_N:
        assert hc.proj_points(n).shape == (n, 3)
