#!/usr/bin/env python3
"""tools/gen_golden_pack.py — record tests/golden/pack_checksums.json: for every distinct layer row of tests/golden/conv_plan.json, the three
array sizes and the byte checksum that sn_debug_pack_host (the test-only twin library; no GPU needed) returns for the recipe weights below.
tests/host/sn_pack_check.cpp rebuilds the same weights in C++, packs them with sn_pack.h and compares: the packed stream is pinned byte for byte.
    python tools/gen_golden_pack.py [path/to/libsurfacenet_hip_dbg.so]
Recorded from the packer as it stood inside sn_api.hip, before it moved to sn_pack.h; re-record only when the packed layout is meant to change.

The recipe (integers only, so numpy and C++ agree bit for bit; sn_pack_check.cpp recipe_weights / recipe_bn restate it):
  s_0 = 0x9E3779B9, s_{i+1} = (1664525 s_i + 1013904223) mod 2^32; element i = (o * cin + ci) * taps + t of the (cout, cin, taps) tensor uses s = s_{i+1}:
  w = k * 2^(e_o - 16 - sh), k = ((s >> 8) & 0x1FFFF) - 65536 (17 bits: more than fp16 holds), sh = s >> 29, e_o = (5 o) mod 33 - 16 (rows spread over
  33 binades); output row 1 is all zero; row 2 is zero over input channels 0..15 (an all-zero 32-element MX block).
  gamma = (4 + o mod 7) / 8, inv_std = (4 + o mod 5) / 4, beta = (1 + o mod 3) / 4, mean = (1 + o mod 11) / 16."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = ["cin", "cout", "ks", "dil", "k2d", "nf", "nsplit", "cs8max", "split", "bridge_requested"]


def lcg_states(n):
    """s_1 .. s_n, by doubling: s_{i+m} = A_m s_i + C_m."""
    s = np.empty(max(n, 1), np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    A, C = np.uint64(1664525), np.uint64(1013904223)
    s[0] = (A * np.uint64(0x9E3779B9) + C) & m32
    m = 1
    while m < n:
        k = min(m, n - m)
        s[m:m + k] = (A * s[:k] + C) & m32
        A, C = (A * A) & m32, (A * C + C) & m32
        m *= 2
    return s[:n]


def recipe_weights(cin, cout, taps):
    s = lcg_states(cout * cin * taps).reshape(cout, cin, taps)
    k = ((s >> np.uint64(8)) & np.uint64(0x1FFFF)).astype(np.int64) - 65536
    sh = (s >> np.uint64(29)).astype(np.int64)
    e = (5 * np.arange(cout)) % 33 - 16
    w = np.ldexp(k.astype(np.float32), (e[:, None, None] - 16 - sh).astype(np.int32)).astype(np.float32)
    if cout > 1:
        w[1] = 0
    if cout > 2:
        w[2, :16] = 0
    return np.ascontiguousarray(w)


def recipe_bn(cout):
    o = np.arange(cout)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return f((1 + o % 3) / 4), f((4 + o % 7) / 8), f((1 + o % 11) / 16), f((4 + o % 5) / 4)      # beta, gamma, mean, inv_std


def distinct_rows():
    plan = json.load(open(os.path.join(ROOT, "tests", "golden", "conv_plan.json")))
    idx = [plan["columns"].index(c) for c in KEY]
    return sorted({tuple(r[i] for i in idx) for g in plan["plans"] for r in g["rows"]})


def main():
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "surfacenet_amd", "libsurfacenet_hip_dbg.so")
    pack = ctypes.CDLL(lib).sn_debug_pack_host
    pack.restype = ctypes.c_int
    pack.argtypes = [ctypes.c_int] * 9 + [ctypes.c_void_p] * 6
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rows = []
    for row in distinct_rows():
        cin, cout, ks, dil, k2d, nf, nsplit, cs8, split, _ = row
        W = recipe_weights(cin, cout, ks * ks * (1 if k2d else ks))
        beta, gamma, mean, inv_std = recipe_bn(cout)
        out = (ctypes.c_ulonglong * 4)()
        assert pack(cin, cout, ks, dil, k2d, nf, nsplit, cs8, split, P(W), P(beta), P(gamma), P(mean), P(inv_std), out) == 0, row
        rows.append(list(row) + [int(out[0]), int(out[1]), int(out[2]), "%016x" % out[3]])
    doc = {"columns": KEY + ["h_halfs", "scale_floats", "shift_floats", "checksum_hex"], "rows": rows}
    with open(os.path.join(ROOT, "tests", "golden", "pack_checksums.json"), "w") as f:
        f.write("{\n \"columns\": %s,\n \"rows\": [\n%s\n ]\n}\n" % (json.dumps(doc["columns"]), ",\n".join("  " + json.dumps(r) for r in rows)))
    print("%d rows" % len(rows))


if __name__ == "__main__":
    main()
