// mesh_input.h — what every mesh stage (meshsample.h, meshsimplify.h, meshedges.h, meshnormals.h, meshrender.h) asks of a mesh it is given, stated once
// (DESIGN.md section 4.18): the limits, the two predicates their kernels test with, and how a kernel reports the first bad face. Plain C++17,
// no hip/ include: sn_host.h checks the counts and words the refusal from the same constants, and the host checks compile it alone.
//   - at most MESH_MAX_ITEMS vertices and as many faces;
//   - every index of a face lies in [0, V): MESH_ERR_INDEX;
//   - every coordinate of a referenced vertex lies in [MESH_LO, MESH_HI) lattice cells, the mesher's own range (a NaN does not): MESH_ERR_RANGE.
//     The sampler has no lattice: it asks for finite coordinates and has its own kinds beside MESH_ERR_INDEX;
//   - a kernel that meets a bad face sends atomicMin(first_bad, mesh_first_bad(face, kind)) to a word preset to MESH_NO_BAD, and writes no
//     other error word: the host reads the smallest bad face, whatever the order of arrival (sn_host.h mesh_report_bad).
// Each kernel keeps its own loop over a face's corners around mesh_index_ok: a loader that returns one verdict for the face makes the
// compiler merge the corners' branches, and the kernels' code is to stay what it was.
#pragma once
#include <stdint.h>

namespace sn {

constexpr int MESH_MAX_ITEMS = 1 << 28;                   // a table of >= 2 n slots stays within 2^29, n + 1 fits the scan's int, an edge key 56 bits
constexpr double MESH_LO = -4.0, MESH_HI = 2097144.0;     // a referenced coordinate: -4 <= v < 2^21 - 8
constexpr unsigned MESH_ERR_INDEX = 1, MESH_ERR_RANGE = 2;      // error kinds: the low 3 bits of first_bad
constexpr unsigned long long MESH_NO_BAD = ~0ull;         // (0xff bytes: a memset presets it)

constexpr unsigned long long mesh_first_bad(long long face, unsigned kind) { return (unsigned long long)face * 8ull + kind; }

// (constexpr: callable from kernels and from host code alike)
constexpr bool mesh_index_ok(int32_t i, int V) { return i >= 0 && i < V; }

constexpr bool mesh_coord_ok(double p) { return p >= MESH_LO && p < MESH_HI; }      // (NaN fails)

}  // namespace sn
