"""CPU: the checker of the view-pair stage (tests/viewpair_check.py) can fail. The float32 restatements of relw_mlp_kernel / relw_mlp_pairs_kernel /
relw_softmax_kernel / pair_simil_all_kernel pass it at every shape tests/test_gpu_viewpair.py runs on the device; with one fault planted - a
transposed pair, swapped feature columns, a pair table in the other order, the wrong cube stride, a softmax group off by one row, one weight of
1,176 off by half a percent, a missing square root, a lane's terms dropped - they fail it, at DTU's 49 views and at a small shape. The
reference's own viewPairSelection run (tests/golden/vps_cases.npz) passes check_selection and fails it with one cube's pairs exchanged."""
import os

import numpy as np
import pytest

import viewpair_cases as cases
import viewpair_check as vc
from oracle import net_oracle

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FAULT_SHAPES = [(49, 12), (5, 130)]       # DTU's pair count, and the smallest shape at which every fault shows (at 3 views P == n_views and
#                                           the j-major table is the i-major one)


net_values, simil_values, case = cases.net_values, cases.simil_values, cases.case


@pytest.mark.parametrize("shape", vc.SHAPES)
def test_the_unfaulted_restatements_pass_the_checker(shape):
    c = case(*shape)
    assert c["f"].shape == (c["n_cubes"] * c["P"], 258) and c["f"].dtype == np.float32
    assert np.array_equal(vc.restate32_rows(c["e"], c["d"], c["theta"]), c["f"])        # the kernel's gather == the host's feature rows
    r = vc.check_weights(c["r32"], c["f"], net_values(), c["P"], r32=c["r32"], ref=c["ref"])
    print("%2d views x %3d cubes (P = %4d): restatement vs fp64 oracle err32 %.3e, bound %.3e, row sums %.3e" % (shape + (c["P"], r.err32, r.bound, r.sum_err)))
    assert r.ok and r.err == r.err32 and r.sum_err == 0.0
    assert r.err32 < 2e-6          # float32 arithmetic of this size: the issue measured 1.05e-6 at 1,176 pairs
    if c["P"] == 1:
        assert np.array_equal(c["r32"], np.ones((c["n_cubes"], 1), np.float32)) and r.bound == 2.0 ** -21
    for e in (c["e"], c["e_near"]):
        for sign in (1, -1):
            with np.errstate(over="ignore"):
                s = vc.check_simil(vc.restate32_simil(e, simil_values(sign)), e, simil_values(sign))
            assert s.ok and s.err == s.err32, s


@pytest.mark.parametrize("shape", FAULT_SHAPES)
@pytest.mark.parametrize("fault", vc.ROW_FAULTS + ("group_shift",))
def test_a_planted_fault_in_the_weights_fails_the_checker(shape, fault):
    c = case(*shape)
    if fault == "group_shift":
        got = vc.restate32_weights(c["f"], net_values(), c["P"], fault=fault)
    else:
        rows = vc.restate32_rows(c["e"], c["d"], c["theta"], fault=fault)
        assert rows.shape == c["f"].shape and not np.array_equal(rows, c["f"])
        got = vc.restate32_weights(rows, net_values(), c["P"])
    assert np.isfinite(got).all() and np.abs(got.sum(axis=1) - 1).max() < 1e-5       # still a softmax: only the comparison can tell
    r = vc.check_weights(got, c["f"], net_values(), c["P"], r32=c["r32"], ref=c["ref"])
    print("%s at %s: relative error %.3e at %s, bound %.3e" % (fault, shape, r.err, r.where, r.bound))
    assert not r.ok and r.err > r.bound


@pytest.mark.parametrize("shape", FAULT_SHAPES)
def test_one_weight_off_by_half_a_percent_fails_where_the_old_absolute_bound_passed(shape):
    c = case(*shape)
    ref = c["ref"]
    got = c["r32"].copy()
    got[c["n_cubes"] // 2, 7] *= np.float32(1.005)
    r = vc.check_weights(got, c["f"], net_values(), c["P"], r32=c["r32"], ref=c["ref"])
    assert not r.ok and r.where == (c["n_cubes"] // 2, 7) and 4.9e-3 < r.err < 5.1e-3
    if c["P"] == 1176:      # the assertion of test_relative_weight_mlp_vs_oracle lets it through: weights of 8.5e-4, absolute 1e-5
        assert np.abs(got - ref).max() < 1e-5 and np.allclose(got.sum(axis=1), 1.0, atol=1e-5)


@pytest.mark.parametrize("shape", FAULT_SHAPES)
@pytest.mark.parametrize("fault", vc.SIMIL_FAULTS)
@pytest.mark.parametrize("draw", ["e", "e_near"])
def test_a_planted_fault_in_the_similarity_fails_the_checker(shape, fault, draw):
    """On draw()'s embeddings the logistic unit is nearly saturated (all values within 1e-5 of 1) and a fault still shows at 1e-4; on
    draw_near()'s, in the unit's working range, it shows at 1e-2 and more."""
    c = case(*shape)
    got = vc.restate32_simil(c[draw], simil_values(), fault=fault)
    assert got.dtype == np.float32 and np.isfinite(got).all()
    s = vc.check_simil(got, c[draw], simil_values())
    print("%s at %s, %s: |error| %.3e at %s (restatement %.3e)" % (fault, shape, draw, s.err, s.where, s.err32))
    assert not s.ok and s.err >= (1e-2 if draw == "e_near" else 10 * vc.SIMIL_ATOL)


def test_wrong_shape_dtype_and_non_finite_values_fail():
    c = case(5, 130)
    assert not vc.check_weights(c["r32"].astype(np.float64), c["f"], net_values(), c["P"], r32=c["r32"], ref=c["ref"]).ok
    assert not vc.check_weights(c["r32"].reshape(-1), c["f"], net_values(), c["P"], r32=c["r32"], ref=c["ref"]).ok
    bad = c["r32"].copy(); bad[3, 3] = np.nan
    assert not vc.check_weights(bad, c["f"], net_values(), c["P"], r32=c["r32"], ref=c["ref"]).ok
    s = vc.restate32_simil(c["e"], simil_values()).copy(); s[0, 0] = np.nan
    assert not vc.check_simil(s, c["e"], simil_values()).ok


def golden_selection():
    """The reference's viewPairSelection run of tests/golden/vps_cases.npz: its inputs as feature rows, the oracle's and the restatement's weights."""
    from surfacenet_amd import viewPairSelection as vps
    from surfacenet_amd import weights
    v = np.load(os.path.join(GOLD, "vps_cases.npz"))
    values = weights.synthetic_param_values(int(v["sel_seed"]))
    valid = v["sel_valid"].astype(bool)
    theta = vps.viewPairAngles_wrt_pts(v["sel_Ts"], v["sel_centers"][valid])
    f = vc.features(v["sel_e"][valid], v["sel_d"][valid], theta)
    P = v["sel_viewPairs"].shape[0]
    assert np.array_equal(v["sel_viewPairs"], vc.pair_table(v["sel_e"].shape[1]))
    ref = net_oracle.relative_weights(f, values, P)
    r32 = vc.restate32_weights(f, values, P)
    return v, values, f, ref, r32


def test_golden_selection_passes_check_selection_and_a_wrong_row_fails():
    from surfacenet_amd import viewPairSelection as vps
    v, values, f, ref, r32 = golden_selection()
    N, viewPairs = int(v["sel_N"]), v["sel_viewPairs"]
    err32, rtol = vc.weight_bound(r32, ref)
    pairs, w = vps.__argmaxN_viewPairs__(viewPairs, r32, N)
    assert np.array_equal(pairs, v["sel_pairs"])                      # the restatement selects what the reference selected
    assert vc.check_selection(v["sel_pairs"], w, ref, viewPairs, N, rtol) == []
    assert (np.abs(w.astype(np.float64) - v["sel_w"]) <= rtol * v["sel_w"]).all()
    # one cube's pairs replaced by its N lowest-weight pairs (with their own, correct, weights)
    low = np.argsort(ref[2])[:N]
    p2, w2 = pairs.copy(), w.copy()
    p2[2], w2[2] = viewPairs[low], r32[2, low]
    bad = vc.check_selection(p2, w2, ref, viewPairs, N, rtol)
    assert len(bad) == 1 and bad[0].startswith("cube 2: selected oracle weight")
    # the other conditions fire too: a repeated pair, descending order, a pair that is no 2-combination, weights of other pairs
    p3 = pairs.copy(); p3[1, 0] = p3[1, 1]
    assert any("not distinct" in b for b in vc.check_selection(p3, w, ref, viewPairs, N, rtol))
    assert any("decrease" in b for b in vc.check_selection(pairs[:, ::-1], w[:, ::-1], ref, viewPairs, N, rtol))
    assert any("not in viewPairs" in b for b in vc.check_selection(pairs[:, :, ::-1], w, ref, viewPairs, N, rtol))
    assert any("weights off" in b for b in vc.check_selection(pairs, w[::-1], ref, viewPairs, N, rtol))
