"""CPU: the restatement of the mesh's own normals, area and volume (tests/meshnormals_ref.py) pinned on facts that were
computed with Python integers - the closed shells' vector sum, their area2 and volume, the angle to the radial direction - and on the
properties of rule 7; the argument checks of mesh.mesh_normals, mesh.save_stage_2ply and reconstruct.scene_postpass, which run before the
library is touched; the new symbols in header, version script, binding and library; and the arithmetic of csrc/meshnormals_sum.h with
mnr_check_args of csrc/sn_host.h compiled alone under the sanitizers and run as a child process."""
import os
import subprocess

import numpy as np
import pytest

import mesh_refusals as bad
import meshnormals_ref as ref
from test_host_plumbing import CSRC, ROOT, _compile

SHELLS = ("sphere6_q", "sphere6_t", "sphere12_q")
AREA2 = dict(sphere6_q=4205798461176, sphere6_t=4210868105196, sphere12_q=15907349099136)


def _no_library(monkeypatch):
    from surfacenet_amd import runtime

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(runtime, "any_context", no_library)


def _column_sums(N):
    return [sum(col) for col in zip(*N.tolist())]


# ---- anchors ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHELLS)
def test_closed_shell_sums_to_zero_and_has_the_anchored_area(name):
    r = ref.reference(name)
    assert _column_sums(r["N_f"]) == [0, 0, 0]                  # closed and consistently oriented: exactly
    assert r["area2"] == AREA2[name]
    assert r["counts"][0] == 0 and r["counts"][1] == 0 and r["counts"][2] == r["referenced"].sum() == r["vert_normals"].shape[0]
    assert np.array_equal(r["sums"], np.asarray(ref.limbs(r["area2"]) + ref.limbs(r["vol6"]), np.uint64))
    lengths = np.linalg.norm(r["vert_normals"].astype(np.float64), axis=1)
    assert np.abs(lengths - 1).max() < 2e-7                     # three float32 roundings of a unit vector


def test_volume_of_the_r6_shell_is_the_same_integer_in_both_forms():
    q, t = ref.reference("sphere6_q"), ref.reference("sphere6_t")
    assert q["vol6"] == t["vol6"] and abs(q["vol6"] / 6 / 2 ** 48 - 1015.167199) < 1e-6
    assert q["vol6"] > 0                                        # counter-clockwise seen from outside: positive


@pytest.mark.parametrize("name,R,degrees", [("sphere6_q", 6, 4.0), ("sphere12_q", 12, 6.0)])
def test_vertex_normals_point_radially(name, R, degrees):
    """The quad shells, on which the figures were taken (R = 6: 3.64 degrees at most, R = 12: 5.58). The triangulated R = 6 shell weights each
    quad's two halves separately and reaches 5.97 degrees: its normals are held by the properties below and by the anchors above."""
    v, _ = ref.CASES[name]()
    r = ref.reference(name)
    radial = v - 20.0
    radial /= np.linalg.norm(radial, axis=1)[:, None]
    angle = np.degrees(np.arccos(np.clip((r["vert_normals"].astype(np.float64) * radial).sum(axis=1), -1.0, 1.0)))
    print("%s: %.2f degrees at most, %.2f in the mean" % (name, angle.max(), angle.mean()))
    assert angle.max() < degrees and np.abs(np.linalg.norm(v - 20.0, axis=1) - R).max() < 1.5


# ---- rule 7 ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHELLS)
def test_permutation_shift_and_reversal(name):
    v, f = ref.CASES[name]()
    r = ref.reference(name)
    perm = np.random.default_rng(7).permutation(f.shape[0])
    p = ref.normals(v, f[perm])
    assert p["face_normals"].tobytes() == r["face_normals"][perm].tobytes()
    assert all(p[k].tobytes() == r[k].tobytes() for k in ("vert_normals", "counts", "sums"))
    s = ref.normals(v + np.asarray([3.0, -2.0, 11.0]), f)       # whole cells; the shell is closed: vol6 stays too
    assert ref.same_bytes(s, r) == [] and s["vol6"] == r["vol6"]
    b = ref.normals(v, f[:, ::-1])
    assert b["area2"] == r["area2"] and b["vol6"] == -r["vol6"]
    assert np.array_equal(b["face_normals"], -r["face_normals"]) and np.array_equal(b["vert_normals"], -r["vert_normals"])


def test_shift_of_an_open_mesh_changes_the_volume_only():
    v, f = ref.CASES["sheet_t"]()
    r, s = ref.reference("sheet_t"), ref.normals(v + np.asarray([1.0, 2.0, 3.0]), f)
    assert all(s[k].tobytes() == r[k].tobytes() for k in ("face_normals", "vert_normals", "counts")) and s["area2"] == r["area2"]
    assert s["vol6"] != r["vol6"] and _column_sums(r["N_f"]) != [0, 0, 0]


def test_a_quad_and_its_triangulation_agree_per_face():
    from surfacenet_amd import mesh
    v, quads = ref.CASES["sphere6_q"]()
    q = ref.reference("sphere6_q")
    t = ref.normals(v, mesh.triangulate(quads))
    assert np.array_equal(t["N_f"][0::2] + t["N_f"][1::2], q["N_f"])
    assert t["counts"][3] == q["counts"][3] == 2 * quads.shape[0]


# ---- the named cases with degenerate parts ---------------------------------------------------------------------------------------------------------
def test_rules_case():
    """Face 2 = (2, 4, 4) has no area and is all that names vertex 4: one zero face, one referenced vertex with a zero sum; vertex 7 is not a
    number and unreferenced: a second zero row. Faces 0 and 1 are equal: vertex 0 receives the vector twice. Face 5 reaches from 1 to just
    under 2^21 - 8: its components take 55 bits."""
    v, f = ref.CASES["rules"]()
    assert np.isnan(v[7, 0]) and 7 not in f
    r = ref.reference("rules")
    assert r["counts"].tolist() == [1, 1, 7, 6]
    assert np.flatnonzero(~r["vert_normals"].any(axis=1)).tolist() == [4, 7] and not r["face_normals"][2].any()
    assert np.isfinite(r["vert_normals"]).all()
    assert max(abs(x) for x in r["N_f"][5].tolist()).bit_length() == 55
    assert r["N_f"][0].tolist() == r["N_f"][1].tolist() and r["N_v"][0].tolist() == (2 * r["N_f"][0] + r["N_f"][4]).tolist()


def test_soup_case():
    """14 of the 20,000 random triangles name a vertex twice; 10 of the 5,000 vertices are named by no face."""
    r = ref.reference("soup")
    assert r["counts"].tolist() == [14, 0, 4990, 20000]
    assert int((~r["vert_normals"].any(axis=1)).sum()) == 10 and int((~r["face_normals"].any(axis=1)).sum()) == 14


def test_bigfan_needs_more_than_64_bits():
    r = ref.reference("bigfan300")
    assert max(abs(x) for row in r["N_f"].tolist() for x in row).bit_length() == 70
    assert r["N_v"][0][2] == 21857123061572827086848 and int(r["N_v"][0][2]).bit_length() == 75
    lo, carries = [0, 0, 0], [0, 0, 0]                          # the hub's low words, in face order
    for row in r["N_f"].tolist():
        for d in range(3):
            lo[d] += row[d] & (2 ** 64 - 1)
            carries[d] += lo[d] >> 64
            lo[d] &= 2 ** 64 - 1
    negative = sum(1 for row in r["N_f"].tolist() for x in row if x < 0)
    assert carries == [145, 149, 151] and 300 < negative < 600      # of 900 addends: both signs meet the carry


def test_unit_rule_at_its_ends():
    one = np.float32(1)
    assert ref.unit(2 ** 52 - 1, 0, 0) == ((one, 0, 0), 2 ** 52 - 1)
    assert ref.unit(2 ** 52, 0, 0) == ((one, 0, 0), 2 ** 52)
    assert ref.unit(-2 ** 52, 0, 0) == ((-one, 0, 0), 2 ** 52)
    assert ref.unit(-(2 ** 52 + 1), 0, 0) == ((-one, 0, 0), 2 ** 52 + 2)      # floor of a negative
    assert ref.unit(0, 0, 0) == ((0, 0, 0), 0)
    assert ref.unit(3, 0, -4) == ((np.float32(0.6), 0, np.float32(-0.8)), 5)
    assert ref.limbs(-1) == [2 ** 64 - 1] * 3 and ref.limbs(2 ** 64) == [0, 1, 0]


# ---- mesh.mesh_normals, save_stage_2ply and scene_postpass before the library ----------------------------------------------------------------------
def test_mesh_normals_refuses_a_bad_mesh_in_the_stages_words(monkeypatch):
    from surfacenet_amd import mesh
    _no_library(monkeypatch)
    v, f = bad.sheet()

    def refused(text, *args, **kw):
        with pytest.raises(ValueError) as e:
            mesh.mesh_normals(*args, **kw)
        assert str(e.value) == text
        if not kw and np.asarray(args[0]).ndim == 2 and np.asarray(args[0]).shape[1] == 3 and np.asarray(args[0]).dtype.kind == "f":
            with pytest.raises(ValueError) as e2:               # the smoother says the same
                mesh.smooth_mesh(*args)
            assert str(e2.value) == text
    bv, bf, text = bad.bad_index(v, f, 2, 5)
    assert text == "face 2 names a vertex outside [0, 16)"
    refused(text, bv, bf)
    for value in (np.nan, 2097144.0):
        bv, bf, text = bad.bad_coordinate(v, f, 3, value)
        refused(text, bv, bf)
        with pytest.raises(ValueError) as e:                    # ... and so does the restatement
            ref.normals(bv, bf)
        assert str(e.value) == text
    with pytest.raises(ValueError) as e:
        ref.normals(*bad.bad_index(v, f, 2, 5)[:2])
    assert str(e.value) == "face 2 names a vertex outside [0, 16)"
    refused("vert_lattice must be float32 or float64, not int32", v.astype(np.int32), f)
    refused("faces must be (F,3) or (F,4), not (18, 5)", v, np.zeros((18, 5), np.int32))
    refused("faces must hold integers, not float64", v, f.astype(np.float64))
    refused("resol = 0 must be finite and > 0", v, f, resol=0)
    refused("face 0 names a vertex outside [0, 0)", np.zeros((0, 3)), f)
    e = mesh.mesh_normals(v, np.zeros((0, 4), np.int32), resol=0.4)      # no face: without the library
    assert e["vert_normals"].shape == (16, 3) and e["vert_normals"].dtype == np.float32 and not e["vert_normals"].any()
    assert e["face_normals"].shape == (0, 3) and (e["area2"], e["vol6"], e["area"], e["volume"]) == (0, 0, 0.0, 0.0)
    assert [e[k] for k in mesh.NORMAL_COUNTS] == [0, 0, 0, 0]
    e = mesh.mesh_normals(np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    assert e["vert_normals"].shape == (0, 3) and e["area2"] == 0
    assert mesh._limbs(ref.limbs(-12345678901234567890123456789)) == -12345678901234567890123456789 and mesh._limbs(ref.limbs(2 ** 150)) == 2 ** 150


def test_save_stage_2ply_source_is_todays_bytes_and_a_bad_value_opens_no_file(tmp_path, monkeypatch):
    from surfacenet_amd import mesh
    _no_library(monkeypatch)
    v, f = bad.sheet()
    m = dict(vertices=v.astype(np.float32), faces=f, vert_lattice=v, vert_src=np.arange(16, dtype=np.int64) % 5 - 1)
    normal_list = [np.random.default_rng(3).normal(size=(4, 3)).astype(np.float32)]
    rgb_list = [np.arange(12, dtype=np.uint8).reshape(4, 3)]
    a, b, c = (str(tmp_path / n) for n in ("a.ply", "b.ply", "c.ply"))
    mesh.save_stage_2ply(a, m, normal_list, rgb_list)
    mesh.save_stage_2ply(b, m, normal_list, rgb_list, normals="source")
    assert open(a, "rb").read() == open(b, "rb").read() and os.path.getsize(a) > 16 * 27
    for value in ("face", "Mesh", None, 1):
        with pytest.raises(ValueError, match="normals"):
            mesh.save_stage_2ply(c, m, normal_list, rgb_list, normals=value)
    assert not os.path.exists(c)


def test_scene_postpass_checks_mesh_normals_before_any_stage(monkeypatch):
    from surfacenet_amd import reconstruct
    _no_library(monkeypatch)
    empty = dict(prediction_list=[], vxl_ijk_list=[], rayPooling_votes_list=[], cube_ijk_np=np.zeros((0, 3), np.int64))
    cams = np.zeros((2, 3))
    with pytest.raises(ValueError) as e:
        reconstruct.scene_postpass(empty, 32, 26, 2, mesh_normals="mesh")
    assert str(e.value) == "mesh_normals needs mesh=True: it takes its normals from the mesh that mesh=True extracts"
    with pytest.raises(ValueError, match="mesh_normals needs mesh=True"):
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh_normals="mesh")
    with pytest.raises(ValueError, match="mesh_fill needs mesh=True"):      # the order: cell, smooth, fill, normals
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh_fill=16, mesh_normals="mesh")
    with pytest.raises(ValueError, match="mesh_normals needs mesh=True"):   # (needs mesh=True comes before the value)
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh_normals="face")
    with pytest.raises(ValueError, match="max_len"):                        # the stages' settings come before the value too
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_fill=2, mesh_normals="face")
    with pytest.raises(ValueError) as e:
        reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_normals="face")
    assert str(e.value) == "mesh_normals = 'face': 'source' or 'mesh'"
    with pytest.raises(ValueError, match="mesh=True needs cameraTs_np"):
        reconstruct.scene_postpass(empty, 32, 26, 2, mesh=True, mesh_normals="mesh")
    plain = reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_fill=16)
    same = reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_fill=16, mesh_normals="source")
    own = reconstruct.scene_postpass(empty, 32, 26, 2, cameraTs_np=cams, mesh=True, mesh_fill=16, mesh_normals="mesh")
    assert set(same) == set(plain) == set(own)
    for key in ("adapt_mesh", "fixThresh_mesh_filled"):
        assert set(same[key]) == set(plain[key]) and set(own[key]) - set(plain[key]) == {"vert_normals", "area", "volume"}
        assert own[key]["vert_normals"].shape == (0, 3) and own[key]["area"] == 0.0 and own[key]["volume"] == 0.0


# ---- the ABI: symbols are only added ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_version_script_binding_and_library():
    import fnmatch
    import re
    import __graft_entry__ as g
    g.build()
    from surfacenet_amd import _lib
    new = ("sn_mesh_normals", "sn_mesh_normals_dev")
    txt = open(os.path.join(ROOT, "include", "surfacenet_hip.h")).read()
    assert "#define SN_ABI_VERSION 2" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    pattern = re.search(r"global:\s*([^;]+);", open(os.path.join(CSRC, "exports.map")).read()).group(1).strip()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode().split()
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert fnmatch.fnmatchcase(name, pattern), (name, pattern)
        assert name in _lib.ABI_SYMBOLS and name in exported, name
    lib = _lib.load()
    assert lib.sn_version() == 2 and all(hasattr(lib, name) for name in new)
    assert "sn_meshnormals.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_the_arithmetic_header_is_hip_free():
    with open(os.path.join(CSRC, "meshnormals_sum.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes and all("hip/" not in i and i in ("<math.h>", "<stdint.h>", '"meshsmooth_round.h"') for i in includes), includes


# ---- the arithmetic and the argument checks of the C entry, on the CPU -----------------------------------------------------------------------------
def test_arithmetic_and_argument_checks_under_sanitizers(tmp_path):
    """tests/host/meshnormals_check.cpp runs csrc/meshnormals_sum.h - the 128-bit cross product at the ends of the range, the limb sum across
    both carries with negative addends, the unit rule at 2^52 - 1, 2^52, -2^52, 2^77 and with a zero component - and sn_host.h's
    mnr_check_args over every end of every range, compiled stand-alone with -fsanitize=address,undefined and run as a child process."""
    exe = str(tmp_path / "meshnormals_check")
    _compile(os.path.join(ROOT, "tests", "host", "meshnormals_check.cpp"), exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "MESHNORMALS-CHECK-OK" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
