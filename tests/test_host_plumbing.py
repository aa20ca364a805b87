"""CPU: csrc/sn_host.h — the entry points' host plumbing that needs no device (Carve, the host mirror's plan, table_cap, the packed-list checks) — csrc/sn_pack.h —
the host half of weight packing — and csrc/lattice.h — the keys, codes and table predicates of the lattice stages — each compiled alone by a plain host C++17 compiler, with no hip/ include on its path, under the address and
undefined-behaviour sanitizers, and run as a child process (tests/host/sn_host_check.cpp, sn_pack_check.cpp and lattice_check.cpp hold the checks). Nothing is
loaded into this interpreter."""
import json
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surfacenet_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "sn_host_check.cpp")


def _clangxx():
    for cand in (shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++"):
        if cand and os.path.exists(cand):
            return cand
    raise AssertionError("no clang++ on this machine")


def _compile(src, exe):
    cmd = [_clangxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, src]
    c = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-3000:]


def test_sn_host_header_is_hip_free():
    """sn_host.h, sn_pack.h, sn_consts.h, lattice.h and mesh_input.h include no HIP header and none of the project's headers that do."""
    hip_free = ("sn_host.h", "sn_pack.h", "sn_consts.h", "lattice.h", "mesh_input.h")
    for name in hip_free:
        with open(os.path.join(CSRC, name)) as f:
            includes = [line.split()[1] for line in f if line.startswith("#include")]
        assert name == "sn_consts.h" or includes, name
        for i in includes:
            assert "hip/" not in i and (i[0] == "<" or os.path.basename(i.strip('"')) in hip_free + ("surfacenet_hip.h",)), (name, i)


def test_sn_host_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sn_host_check")
    _compile(SRC, exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "SN-HOST-CHECK-OK" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])


def test_lattice_check_under_sanitizers(tmp_path):
    """lattice.h alone: key round trip and order, lt_cube_of against a linear scan, the offsets predicate, the ordered codes, and lt_mix64
    against the values the hashes it replaced gave (tests/host/lattice_check.cpp)."""
    exe = str(tmp_path / "lattice_check")
    _compile(os.path.join(ROOT, "tests", "host", "lattice_check.cpp"), exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "LATTICE-CHECK-OK" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])


def test_sn_pack_check_under_sanitizers(tmp_path):
    """The weight packer against an independent reader of its stream, for every distinct layer row of every recorded plan, and against the byte
    checksums recorded before the packer moved out of sn_api.hip (tests/host/sn_pack_check.cpp; tools/gen_golden_pack.py)."""
    golden = os.path.join(ROOT, "tests", "golden")
    plan = json.load(open(os.path.join(golden, "conv_plan.json")))
    sums = json.load(open(os.path.join(golden, "pack_checksums.json")))
    key = sums["columns"][:10]
    assert key == ["cin", "cout", "ks", "dil", "k2d", "nf", "nsplit", "cs8max", "split", "bridge_requested"]
    idx = [plan["columns"].index(c) for c in key]
    rows = sorted({tuple(r[i] for i in idx) for g in plan["plans"] for r in g["rows"]})
    recorded = {tuple(r[:10]): r[10:] for r in sums["rows"]}
    assert len(rows) > 40 and sorted(recorded) == rows                      # one checksum per distinct plan row, no others
    exe = str(tmp_path / "sn_pack_check")
    _compile(os.path.join(ROOT, "tests", "host", "sn_pack_check.cpp"), exe)
    text = "".join(" ".join(str(v) for v in row + tuple(recorded[row])) + "\n" for row in rows)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "SN-PACK-CHECK-OK %d rows" % len(rows) in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
