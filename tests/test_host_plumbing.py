"""CPU: csrc/sn_host.h — the entry points' host plumbing that needs no device (Carve, table_cap, the packed-list checks) — compiled alone
by a plain host C++17 compiler, with no hip/ include on its path, under the address and undefined-behaviour sanitizers, and run as a child
process (tests/host/sn_host_check.cpp holds the checks). Nothing is loaded into this interpreter."""
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


def test_sn_host_header_is_hip_free():
    with open(os.path.join(CSRC, "sn_host.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes and not [i for i in includes if "hip/" in i or i.strip('"<>') in ("sn_internal.h", "conv3d_mfma.h")], includes


def test_sn_host_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sn_host_check")
    cmd = [_clangxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, SRC]
    c = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "SN-HOST-CHECK-OK" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
