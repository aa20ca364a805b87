"""CPU: what tests/test_gpu_layers.py rests on, checked without a GPU.

  a. COVERAGE. For every SurfaceNet plan of tests/golden/conv_plan.json and every tiled axis (layer_check.level_axes), the cube sizes of the
     plan's own CASES reach every tile / halo class (layer_check.tile_classes) that any cube size sn_create accepts up to 44 can reach. A plan
     without cases, or a new case taken away, fails it.
  b. THE CHECK CAN FAIL. A stand-in "device" - the plan's arithmetic class reference run launch by launch on its own stored tensors
     (layer_check.class_step: the CPU model for the MX-judged outputs, the x3 float32 step for the others) - passes both tables; with one
     fault planted in one step's stored output and carried through every later launch, as a device would carry it, the planted step's LOCAL
     row fails and no other, and the GLOBAL table flags that tensor. The faults are the kind the GPU cases hunt: one output voxel row computed
     with the input beyond a tile seam read as zero (a halo row that was not staged), a tensor stored without its lo or code plane, a
     non-zero value in a padded channel. The whole net runs at cube_D 20 (seam 15 | 16: a partial tile behind a full one); the dilated chain
     at quarter extent 10 = 8 + R runs alone, from a conv3_3 tensor of a cube_D 40 pass of the float32 oracle (seam 7 | 8, halo radius 2).
     The dropped plane is not planted in f16m8, where the bound cannot promise to see it (WHOLE_FAULTS says why, with the figures)."""
import json
import os

import numpy as np
import pytest

import act_decode as ad
import layer_check as lc
import synth
import test_gpu_layers as tgl
from oracle import net_emulation, net_oracle

# ------------------------------------------------------------------------------------------------ a. coverage
# (what sn_create accepts: a multiple of 4 from 8 on whose quarter extent leaves no 1-voxel partial tile under the dilation-2 layers - test_abi.py pins 36)
ACCEPTED = [s for s in range(8, 45, 4) if not (s // 4 > 8 and (s // 4) % 8 == 1)]
NEW_CASES = ([(s, p, None) for p in ("f16m8", "f16") for s in (20, 40, 44)] + [(20, "f16x3p", None), (44, "f16x3p", None)]
             + [(s, "f16x3", 2) for s in (12, 20, 40, 44)] + [(s, "f16x3", 0) for s in (12, 20, 40, 44)])


def golden_plans():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan.json")) as f:
        return [(g["mode"], g["conv4_fp8"]) for g in json.load(f)["plans"] if g["net"] == "surfacenet"]


def missing(plans, cases):
    """-> [(plan, (level, T, R), classes no case of that plan reaches)] - empty when the cases cover every plan."""
    out = []
    for plan in plans:
        sizes = [s for s, p, c4 in cases if lc.plan_key(p, c4) == plan] if plan in lc.PLANS else []
        for k, (level, _, T, R) in enumerate(lc.level_axes(8)):
            reach = set().union(*(lc.tile_classes(lc.level_axes(s)[k][1], T, R) for s in ACCEPTED))
            got = set().union(*(lc.tile_classes(lc.level_axes(s)[k][1], T, R) for s in sizes))
            if reach - got:
                out.append((plan, (level, T, R), sorted(reach - got)))
    return out


def test_tile_classes():
    tc = lc.tile_classes
    assert tc(5, 8, 2) == {"only tile partial"} and tc(8, 8, 1) == {"one full tile"} and tc(16, 8, 1) == {"several full tiles"}
    assert tc(10, 8, 2) == {"one full tile", "partial behind full, rem == R"} and tc(11, 8, 2) == {"one full tile", "partial behind full, rem > R"}
    assert tc(10, 8, 1) == {"one full tile", "partial behind full, rem > R"} and tc(12, 16, 1) == {"only tile partial"}
    assert tc(20, 8, 1) == {"several full tiles", "interior tile", "partial behind full, rem > R"}
    assert tc(24, 8, 1) == {"several full tiles", "interior tile"} and tc(40, 16, 1) == {"several full tiles", "interior tile", "partial behind full, rem > R"}
    assert tc(17, 8, 1) == {"several full tiles", "interior tile", "partial behind full, rem == R"}
    with pytest.raises(ValueError):
        tc(9, 8, 2)                                                  # cube_D 36: what sn_create refuses
    assert 36 not in ACCEPTED and ACCEPTED == [8, 12, 16, 20, 24, 28, 32, 40, 44]


def test_the_cases_reach_every_tile_class_of_every_plan():
    plans = golden_plans()
    assert sorted(plans) == sorted(lc.PLANS), plans                  # the harness knows the references and the storage of exactly these
    assert set(NEW_CASES) <= set(tgl.CASES) and len(set(tgl.CASES)) == len(tgl.CASES)
    assert all(s in ACCEPTED for s, _, _ in tgl.CASES)
    assert missing(plans, tgl.CASES) == []
    # the multi-tile classes of the dilated chain are really asked for: both remainders behind a full tile at level 2
    need = {"partial behind full, rem == R", "partial behind full, rem > R"}
    assert need <= set().union(*(lc.tile_classes(s // 4, 8, 2) for s in ACCEPTED))


def test_a_plan_without_cases_fails_the_coverage():
    gaps = missing(golden_plans() + [("f16x3", 3)], tgl.CASES)
    assert gaps and {g[0] for g in gaps} == {("f16x3", 3)} and len(gaps) == 4


@pytest.mark.parametrize("case", NEW_CASES, ids=tgl.case_id)
def test_no_new_case_can_be_taken_away(case):
    gaps = missing(golden_plans(), [c for c in tgl.CASES if c != case])
    assert gaps and {g[0] for g in gaps} == {lc.plan_key(case[1], case[2])}, gaps


# ------------------------------------------------------------------------------------------------ b. the check can fail
BUF_OF = {v[0]: k for k, v in lc.BUFFERS.items()}
N_PLANES = {ad.FMT_F16: 1, ad.FMT_HILO: 2, ad.FMT_M6: 2, ad.FMT_M8: 2, ad.FMT_HILO_M8: 3}


def layout_of(buf, extent, plan):
    """The act_decode.Layout sn_debug_tensor_info would report for that buffer of a one-sample context."""
    fmt, e8 = lc.storage(*plan)
    f, cs = fmt[buf], (lc.BUFFERS[buf][1] + 7) // 8 * 8
    plane = extent ** 3 * cs
    lo = plane if f in (ad.FMT_HILO, ad.FMT_HILO_M8) else -1
    code = plane if f in (ad.FMT_M6, ad.FMT_M8) else (2 * plane if f == ad.FMT_HILO_M8 else -1)
    return ad.Layout(extent, cs, N_PLANES[f], lo, code, e8[buf], 2 * plane * N_PLANES[f], f)


def through_layout(v, name, values, plan, drop=None, view=None):
    """A tensor (oracle name, original units) -> (raw bytes as its producer stores them, Layout, what the reader decodes); drop "lo" / "code":
    with that plane zeroed, as a kernel that never wrote it leaves a fresh workspace."""
    buf = BUF_OF[name]
    _, C, relu = lc.BUFFERS[buf]
    oe = net_emulation.renorm_exponents(net_oracle.params_to_dict(values)[relu]) if relu else None
    lay = layout_of(buf, v.shape[-1], plan)
    raw = ad.encode(v, lay, oe=oe)
    if drop:
        off = 2 * {"lo": lay.lo, "code": lay.code}[drop]
        assert off > 0
        raw[off: off + 2 * v.shape[-1] ** 3 * lay.cs] = 0
    return raw, lay, ad.decode(raw, lay, 1, C, oe=oe, view=view)


def missing_halo(values, plan, lo, hi, row):
    """Fault (i): the step's outputs on the one voxel row `row` (z, y; every channel, every x) are those of the step with the input's planes
    z in [lo, hi) - the rows beyond the tile seam at hi that the tile behind it stages as its halo - read as zero."""
    def fault(step, xin, outs):
        x0 = [a.copy() for a in xin]
        x0[0][:, :, lo:hi] = 0
        bad = lc.class_step(values, step, x0, *plan)
        outs = [o.copy() for o in outs]
        for o, b in zip(outs, bad):
            assert not np.array_equal(o[:, :, row[0], row[1]], b[:, :, row[0], row[1]])
            o[:, :, row[0], row[1]] = b[:, :, row[0], row[1]]
        return outs
    return fault


def dropped_plane(values, plan, drop):
    """Fault (ii): the step's (single) stored output without its lo or code plane."""
    def fault(step, xin, outs):
        name, = set(net_oracle.STEPS[step][1])
        return [through_layout(outs[0], name, values, plan, drop=drop)[2][0]]
    return fault


def run_stand_in(values, dec, plan, steps, fault_at=None, fault=None):
    """The plan's class reference, launch by launch on its own stored tensors: `steps` of net_oracle.STEPS in order, from the tensors already
    in dec (not modified) -> the completed dict."""
    dec = dict(dec)
    for step in steps:
        ins, outs = net_oracle.STEPS[step]
        xin = [dec[n] for n in ins]
        res = lc.class_step(values, step, xin, *plan)
        if step == fault_at:
            res = fault(step, xin, res)
        dec.update(zip(outs, res))
        if step == "upsample":
            dec["cat"] = np.concatenate([dec["side1"], dec["cat48"]], axis=1)
    return dec


def failing(g, loc):
    return [r[0] for r in g if not r[1] <= r[3]], [(r[0], r[1]) for r in loc if not r[2] <= r[4]]


ALL_STEPS = list(net_oracle.STEPS)
WHOLE = [("f16x3", 1), ("f16m8", 0), ("f16x3p", 0)]                  # the default plan, the all-MX mode, the plain x3 mode


@pytest.fixture(scope="module")
def values():
    return list(synth.calibrated_params(1))


@pytest.fixture(scope="module")
def whole(values):
    """plan -> cube_D 20: the references of the GPU test, and the clean stand-in with both of its tables (computed once per plan)."""
    made = {}

    def of(plan):
        if plan not in made:
            X = synth.random_cvc(1, 20, 60)
            exact, ref, factor = lc.references(X, values, *plan)
            clean = run_stand_in(values, {"x": ref["x"]}, plan, ALL_STEPS)
            title = "stand-in device (%s, conv4_fp8 %d), cube_D 20, no fault" % plan
            g = lc.global_table(clean, exact, ref, factor, title)
            loc = lc.local_table(clean, values, plan[0], title, conv4_fp8=plan[1])
            made[plan] = (exact, ref, factor, clean, g, loc)
        return made[plan]
    return of


PLAN_ID = lambda p: "%s-%d" % p if isinstance(p, tuple) else p


@pytest.mark.parametrize("plan", WHOLE, ids=PLAN_ID)
def test_the_stand_in_passes_every_row(whole, plan):
    exact, ref, factor, clean, g, loc = whole(plan)
    assert failing(g, loc) == ([], [])
    assert [r[0] for r in g] == lc.GLOBAL_NAMES and [r[0] for r in loc] == [s for s, (_, o) in net_oracle.STEPS.items() for _ in o]
    assert all(r[2] > 0 for r in g) and all(r[3] > 0 for r in loc), "a reference that never errs bounds nothing"
    # (the stand-in IS the class reference on its own input: the device column of the local table equals the reference column)
    assert all(r[2] == r[3] for r in loc)


# (step, fault, the plans it is planted in): a level-0 halo row behind the seam 15 | 16 in an x3-judged launch (16x8x8 tiles) and in the loosest
# MX-judged one (merge_conv_a: bound 3 x the 6-bit model's error), and one tensor of each storage format without its second plane
def _whole_faults(values, plan):
    f = {"halo-conv1_2": ("conv1_2", missing_halo(values, plan, 15, 16, (16, 5))),
         "halo-merge_conv_a": ("merge_conv_a", missing_halo(values, plan, 15, 16, (16, 11)))}
    fmt = lc.storage(*plan)[0]
    f["plane-conv2_2"] = ("conv2_2", dropped_plane(values, plan, "lo" if fmt["b2"] == ad.FMT_HILO else "code"))
    f["plane-merge_a"] = ("merge_conv_a", dropped_plane(values, plan, "lo" if fmt["ma"] == ad.FMT_HILO else "code"))
    return f


# Fault (ii) is planted where the dropped plane carries precision the plan's arithmetic keeps: a value without its second plane is off by up to
# half an fp16 ulp, 2^-12 of itself, against the 2^-22 of an x3 tensor and the ~2^-16 of a 6-bit / fp8 code plane read by an x3-accurate main
# term. NOT in f16m8: there every product already carries the 6-bit codes' own error (2^-4 of a 2^-11 correction term, twice, per product),
# within the factor 3 of the dropped plane's - measured on this stand-in, conv4_2 without its code plane at quarter extent 10 reads 9.1e-7
# against a local bound of 1.3e-6, and merge_a at cube_D 20 3.9e-4 against a global bound of 4.2e-4 (its local row does fail, 8.4e-5 against
# 1.1e-5). In f16m8 "3 x the reference's own error" therefore does not promise to notice a missing code plane; a missing halo row it does.
WHOLE_FAULTS = ([(p, w) for p in WHOLE for w in ("halo-conv1_2", "halo-merge_conv_a")]
                + [(p, w) for p in (("f16x3", 1), ("f16x3p", 0)) for w in ("plane-conv2_2", "plane-merge_a")])


@pytest.mark.parametrize("plan,which", WHOLE_FAULTS, ids=lambda v: PLAN_ID(v))
def test_a_planted_fault_fails_its_own_local_row_and_its_tensor(whole, values, plan, which):
    exact, ref, factor, clean, g0, loc0 = whole(plan)
    step, fault = _whole_faults(values, plan)[which]
    k = ALL_STEPS.index(step)
    dec = run_stand_in(values, clean, plan, ALL_STEPS[k:], fault_at=step, fault=fault)
    out, = set(net_oracle.STEPS[step][1])
    assert not np.array_equal(dec[out], clean[out])
    title = "%s planted in the stand-in (%s, conv4_fp8 %d), cube_D 20" % ((which,) + plan)
    loc = lc.local_table(dec, values, plan[0], title, steps=ALL_STEPS[k:], conv4_fp8=plan[1])
    g = lc.global_table(dec, exact, ref, factor, title)
    bad_g, bad_l = failing(g, loc)
    assert bad_l == [(step, out)], bad_l                             # LOCAL: the planted launch and no other - later launches are right about
    #                                                                  the (wrong) input they were given; earlier rows are the clean run's
    assert out in bad_g, bad_g                                       # GLOBAL: that tensor (what lies downstream may or may not follow)
    assert not set(bad_g) & {n for s in ALL_STEPS[:k] for n in net_oracle.STEPS[s][1]}


# ---- the dilated chain alone, at quarter extent 10 = 8 + R
CHAIN = ["conv4_1+conv4_2", "conv4_3", "side_op4"]
CHAIN_NAMES = ["conv4_2", "conv4_3", "side4_pre"]
QUARTER = [("f16x3", 1), ("f16x3", 2), ("f16m8", 0), ("f16x3p", 0)]  # (conv4_fp8 = 2: conv4_1 on x3 arithmetic storing hi + fp8 codes, the instantiation no other plan has)


@pytest.fixture(scope="module")
def conv3_3_of_40(values):
    X = synth.random_cvc(1, 40, 80)
    return net_oracle.forward_torch(X, values, dtype="float32", return_intermediates=True)[2]["conv3_3"].astype(np.float64)


@pytest.fixture(scope="module")
def chain(values, conv3_3_of_40):
    """plan -> the stored conv3_3 of a cube_D 40 pass as conv4_1 reads it in that plan, the fp64 chain and the clean stand-in chain from it."""
    made = {}

    def of(plan):
        if plan not in made:
            assert conv3_3_of_40.shape[-1] == 10
            x = through_layout(conv3_3_of_40, "conv3_3", values, plan, view="code")[2][0]
            exact = {"conv3_3": x}
            for step, name in zip(CHAIN, CHAIN_NAMES):
                exact[name] = net_oracle.step_torch(values, step, [exact[net_oracle.STEPS[step][0][0]]])[0][0]
            made[plan] = (exact, run_stand_in(values, {"conv3_3": x}, plan, CHAIN))
        return made[plan]
    return of


@pytest.mark.parametrize("plan,which", [(p, w) for p in QUARTER for w in ("none", "halo", "plane") if (p[0], w) != ("f16m8", "plane")], ids=lambda v: PLAN_ID(v))
def test_the_dilated_chain_at_quarter_extent_10(chain, values, plan, which):
    """No fault: every row passes. halo: conv4_1+conv4_2's output row (8, 4), the first behind the seam 7 | 8, computed with the input planes 6
    and 7 - the two-voxel halo its tile stages from the full tile before it - read as zero. plane: conv4_2 stored without its second plane.
    (Not in f16m8: see WHOLE_FAULTS.) Global reference: the clean stand-in itself (the class reference chained from the same stored conv3_3),
    factor as in layer_check.references."""
    exact, clean = chain(plan)
    factor = 3.0 if plan[0] in ("f16x3", "f16m8") else 4.0
    drop = "lo" if lc.storage(*plan)[0]["b4"] == ad.FMT_HILO else "code"
    fault = {"none": None, "halo": missing_halo(values, plan, 6, 8, (8, 4)), "plane": dropped_plane(values, plan, drop)}[which]
    dec = clean if fault is None else run_stand_in(values, clean, plan, CHAIN, fault_at=CHAIN[0], fault=fault)
    title = "stand-in dilated chain (%s, conv4_fp8 %d), quarter extent 10, fault: %s" % (plan + (which,))
    loc = lc.local_table(dec, values, plan[0], title, steps=CHAIN, conv4_fp8=plan[1])
    g = lc.global_table(dec, exact, clean, factor, title, names=CHAIN_NAMES)
    bad_g, bad_l = failing(g, loc)
    assert all(r[2] > 0 for r in g) and all(r[3] > 0 for r in loc)
    if fault is None:
        assert (bad_g, bad_l) == ([], [])
    else:
        assert bad_l == [(CHAIN[0], "conv4_2")], bad_l
        assert "conv4_2" in bad_g, bad_g


# ---- (iii) padded channels
@pytest.mark.parametrize("plan", [("f16x3", 1), ("f16x3", 0), ("f16m8", 0), ("f16", 0)], ids=lambda p: "%s-%d" % p)
def test_a_non_zero_padded_channel_is_caught(values, plan):
    """The four padded buffers (6 -> 8, 300 -> 304, 100 -> 104 channels) in the plan's byte layout pass check_padding; one non-zero half in a
    padded channel of a hi plane, or one non-zero code in a padded channel of a code plane, does not."""
    rs = np.random.RandomState(5)
    t = {"x": rs.randn(1, 6, 8, 8, 8) * 50, "conv4_3": np.abs(rs.randn(1, 300, 2, 2, 2)), "conv4_2": np.abs(rs.randn(1, 300, 2, 2, 2)),
         "merge_a": np.abs(rs.randn(1, 100, 8, 8, 8))}
    raws, lays = {}, {}
    for name, v in t.items():
        raws[BUF_OF[name]], lays[BUF_OF[name]], _ = through_layout(v, name, values, plan)

    def check(raws):
        pads, extras = {}, {}
        for buf, raw in raws.items():
            _, pads[buf], extras[buf] = ad.decode(raw, lays[buf], 1, lc.BUFFERS[buf][1])
        lc.check_padding(pads, extras, lays)

    check(raws)
    pokes = [("x0", 2 * (123 * 8 + 6), 0x01)]                        # hi plane [D^3][8 halfs]: channel 6 of voxel 123, the smallest subnormal
    lay = lays["ma"]
    if lay.fmt == ad.FMT_M6:                                         # code plane [13 groups][D^3][16 bytes]: the last group's lo code of its channel 7 = 103
        pokes.append(("ma", 2 * lay.code + (12 * 512 + 77) * 16 + 11, 0x04))
    elif lay.fmt == ad.FMT_HILO:
        pokes.append(("ma", 2 * lay.lo + 2 * ((12 * 512 + 77) * 8 + 7), 0x01))
    lay = lays["b4"]
    if lay.fmt == ad.FMT_M8:                                         # fp8 slots [hi c0..7 | lo c0..7]: lo code of channel 5 of group 37 = 301
        pokes.append(("b4", 2 * lay.code + (37 * 8 + 3) * 16 + 8 + 5, 0x01))
    for buf, at, byte in pokes:
        bad = dict(raws)
        bad[buf] = raws[buf].copy()
        assert bad[buf][at] == 0
        bad[buf][at] = byte
        with pytest.raises(AssertionError):
            check(bad)
