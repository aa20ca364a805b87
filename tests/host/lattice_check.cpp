// lattice_check.cpp — stand-alone check of surfacenet_amd/csrc/lattice.h, the hip-free helpers of the lattice stages: the cell key, the owner
// of a packed voxel, the offsets-table predicate, the ordered float codes and the hash finaliser. tests/test_host_plumbing.py compiles it with
// a plain host compiler under the address and undefined-behaviour sanitizers and runs it; it prints LATTICE-CHECK-OK, or the first failed
// check and exits 1.
#include "lattice.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

using namespace sn;

#define CHECK(cond)                                                                                     \
    do {                                                                                                \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static void check_key()
{
    const long long edge[3] = {0, 1, LT_AXIS_MAX - 1};
    unsigned long long prev = 0;
    bool first = true;
    for (long long x : edge)
        for (long long y : edge)
            for (long long z : edge) {             // ascending (x, y, z)
                const unsigned long long key = lt_key(x, y, z);
                long long b[3];
                lt_unkey(key, b);
                CHECK(b[0] == x && b[1] == y && b[2] == z);
                CHECK(key < (1ull << 63));
                CHECK(first || key > prev);          // key order is lexicographic order
                prev = key; first = false;
            }
    CHECK(lt_key(0, 0, LT_AXIS_MAX - 1) < lt_key(0, 1, 0) && lt_key(0, LT_AXIS_MAX - 1, LT_AXIS_MAX - 1) < lt_key(1, 0, 0));
}

// offsets from per-cube counts; every t in [0, total) has exactly one cube with off[c] <= t < off[c + 1], which the linear scan finds
static void check_cube_of(const std::vector<int> &counts)
{
    const int n = (int)counts.size();
    std::vector<int64_t> off(n + 1, 0);
    for (int c = 0; c < n; ++c) off[c + 1] = off[c] + counts[c];
    const long long total = off[n];
    CHECK(total > 0);
    for (long long t = 0; t < total; ++t) {
        int ref = -1;
        for (int c = 0; c < n; ++c)
            if (off[c] <= t && t < off[c + 1]) { CHECK(ref < 0); ref = c; }
        CHECK(ref >= 0);
        CHECK(lt_cube_of(off.data(), n, t) == ref);
    }
    CHECK(lt_cube_of(off.data(), n, total - 1) < n);
    for (long long t : {-1ll, total, total + 5}) {  // outside the lists: still an index in [0, n)
        const int c = lt_cube_of(off.data(), n, t);
        CHECK(c >= 0 && c < n);
    }
}

static int count_bad(const std::vector<int64_t> &off, long long total)
{
    const int n = (int)off.size() - 1;
    int bad = 0;
    for (long long c = 0; c <= n; ++c) bad += lt_offsets_bad(off.data(), c, n, total) ? 1 : 0;
    return bad;
}

static void check_offsets_bad()
{
    CHECK(count_bad({0, 2, 2, 5}, 5) == 0 && count_bad({0}, 0) == 0 && count_bad({0, 0, 0}, 0) == 0);
    const std::vector<int64_t> shifted = {1, 2, 2, 5}, falling = {0, 3, 2, 5}, good = {0, 2, 2, 5}, none_bad = {4};
    CHECK(count_bad(shifted, 5) == 1 && lt_offsets_bad(shifted.data(), 0, 3, 5));        // does not start at 0
    CHECK(count_bad(falling, 5) == 1 && lt_offsets_bad(falling.data(), 2, 3, 5));        // decreases
    CHECK(count_bad(good, 6) == 1 && lt_offsets_bad(good.data(), 3, 3, 6));              // does not end at total
    CHECK(count_bad(none_bad, 4) == 1 && count_bad(none_bad, 0) == 1);                   // n = 0: entry 0 is first and last
}

template <typename F, typename K>
static void check_code(F denorm)
{
    const F inf = std::numeric_limits<F>::infinity();
    const F v[7] = {-inf, (F)-1, (F)-0.0, (F)0.0, denorm, (F)1, inf};
    CHECK(denorm > 0 && std::fpclassify(denorm) == FP_SUBNORMAL);
    for (int i = 0; i < 7; ++i) {
        const K c = lt_code(v[i]);
        if (i > 0) CHECK(c > lt_code(v[i - 1]));    // strictly monotone, -0 < +0
        const F back = lt_decode(c);
        CHECK(memcmp(&back, &v[i], sizeof(F)) == 0);
    }
}

int main()
{
    check_key();
    check_cube_of({3});                                // n = 1
    check_cube_of({0, 0, 4, 1});                       // empty cubes at the front
    check_cube_of({2, 0, 0, 3, 0, 1});                 // in the middle
    check_cube_of({1, 5, 0, 0});                       // at the end
    check_cube_of({0, 2, 0, 1, 0});                    // everywhere
    check_offsets_bad();
    check_code<float, unsigned>(std::numeric_limits<float>::denorm_min());
    check_code<double, unsigned long long>(std::numeric_limits<double>::denorm_min());
    // the low words the five hashes this replaced gave (recorded from their text before the move: k ^= k >> 33, the two multiplies, full mask)
    CHECK((unsigned)lt_mix64(0x0000040000400003ull) == 0x21d38bd8u && (unsigned)lt_mix64(1ull) == 0x34c2cb2cu);
    CHECK((unsigned)lt_mix64(0x0123456789abcdefull) == 0x89022ceau && (unsigned)lt_mix64(0x7fffffffffffffffull) == 0xa930edeau);
    printf("LATTICE-CHECK-OK\n");
    return 0;
}
