// sn_host_check.cpp — stand-alone check of surfacenet_amd/csrc/sn_host.h, the part of the entry points' host plumbing that needs no device:
// Carve, table_cap and the packed-list checks. tests/test_host_plumbing.py compiles it with a plain host compiler under the address and
// undefined-behaviour sanitizers and runs it; it prints SN-HOST-CHECK-OK, or the first failed check and exits 1.
#include "sn_host.h"

#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#define CHECK(cond)                                                                                     \
    do {                                                                                                \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s  (g_err = \"%s\")\n", __FILE__, __LINE__, #cond, g_err.c_str()); exit(1); } \
    } while (0)

// ---- Carve ------------------------------------------------------------------------------------------------------------------------------------
struct Region { size_t off, bytes; };

// a Carve that also records what each get() handed out
struct Rec {
    Carve cv;
    std::vector<Region> r;
    template <typename T> T *get(size_t n)
    {
        T *p = cv.get<T>(n);
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        r.push_back(Region{cv.off - bytes, bytes});
        if (cv.base) CHECK(reinterpret_cast<unsigned char *>(p) == cv.base + r.back().off);
        else CHECK(p == nullptr);
        return p;
    }
};

// the host form of sn_normals with normals and moments (sn_normals.hip nm_layout, with every array staged): n cubes, T voxels, K views per cube of V cameras
static void normals_layout(Rec &w, size_t n)
{
    const size_t T = 7 * n, K = 5, V = 9, cap = table_cap(T, 2, 64);
    w.get<int64_t>(n + 1); w.get<uint32_t>(3 * n); w.get<uint8_t>(3 * T); w.get<uint8_t>(T);
    w.get<float>(3 * n); w.get<float>(n); w.get<int32_t>(n * K); w.get<double>(3 * V);
    w.get<float>(3 * T); w.get<int32_t>(10 * T);
    w.get<int>(1); w.get<int>(T); w.get<double>(3 * n); w.get<unsigned long long>(2 * cap);
}

// one cell grid of the point evaluation with ranks (cellgrid.h grid_layout; the scan's block sums: one per 1024 slots, + 1)
static void grid_layout(Rec &w, size_t n)
{
    const size_t cap = table_cap(n, 2, 1024);
    w.get<unsigned long long>(cap); w.get<int>(cap); w.get<int>(cap); w.get<int>(cap / 1024 + 1);
    w.get<int>(n); w.get<int>(n); w.get<int>(n); w.get<double>(3 * n); w.get<int>(n);
}

static void check_carve(const std::function<void(Rec &, size_t)> &layout, size_t n)
{
    Rec measure;
    layout(measure, n);
    std::vector<unsigned char> buf(measure.cv.off + 256);
    Rec place;
    place.cv.base = buf.data() + (256 - reinterpret_cast<uintptr_t>(buf.data()) % 256) % 256;      // a 256-byte aligned base, as hipMalloc gives
    layout(place, n);
    CHECK(place.cv.off == measure.cv.off);                       // the final off is the measured size
    CHECK(place.r.size() == measure.r.size());
    size_t end = 0;
    for (size_t i = 0; i < place.r.size(); ++i) {
        CHECK(place.r[i].off == measure.r[i].off && place.r[i].bytes == measure.r[i].bytes);
        CHECK(place.r[i].off % 256 == 0);
        CHECK(reinterpret_cast<uintptr_t>(place.cv.base + place.r[i].off) % 256 == 0);
        CHECK(place.r[i].off >= end);                            // regions come in ascending order and do not overlap
        CHECK(place.r[i].bytes > 0);
        end = place.r[i].off + place.r[i].bytes;
        memset(place.cv.base + place.r[i].off, 0xa5, place.r[i].bytes);      // (the sanitizer sees every byte handed out)
    }
    CHECK(end == measure.cv.off);
}

static void check_carve_empty_get()
{
    Carve cv;
    cv.get<double>(0);
    CHECK(cv.off == sizeof(double));                             // get(0) still advances by one element
    cv.get<unsigned char>(0);
    CHECK(cv.off == 257);
    cv.get<int>(3);
    CHECK(cv.off == 512 + 12);
}

// ---- table_cap: the five loops it replaced, as they stood -------------------------------------------------------------------------------------
static unsigned long long loop_crosscube(int n) { unsigned cap = 64; while (cap < 2u * (unsigned)n) cap <<= 1; return cap; }
static unsigned long long loop_normals(long long total) { unsigned cap = 64; while (cap < 2ull * (unsigned long long)total) cap <<= 1; return cap; }
static unsigned long long loop_pointeval(long long n) { unsigned cap = 1024; while (cap < 2 * (unsigned long long)n) cap <<= 1; return cap; }
static unsigned long long loop_ptcubes(long long n) { unsigned tcap = 2048; while (tcap < 4ull * (unsigned long long)n) tcap <<= 1; return tcap; }
static unsigned long long loop_raypool(size_t s3) { size_t cap = 64; while (cap < 2 * s3) cap <<= 1; return cap; }

static void check_table_cap()
{
    struct Case { unsigned factor; size_t min_cap; std::function<unsigned long long(unsigned long long)> loop; };
    const Case cases[5] = {
        {2, 64, [](unsigned long long n) { return loop_crosscube((int)n); }},
        {2, 64, [](unsigned long long n) { return loop_normals((long long)n); }},
        {2, 1024, [](unsigned long long n) { return loop_pointeval((long long)n); }},
        {4, 2048, [](unsigned long long n) { return loop_ptcubes((long long)n); }},
        {2, 64, [](unsigned long long n) { return loop_raypool((size_t)n); }},
    };
    for (const Case &k : cases) {
        const unsigned long long edge = k.min_cap / k.factor;
        for (unsigned long long n : {0ull, 1ull, edge, edge + 1, (1ull << 20) + 1}) {
            const size_t cap = table_cap(n, k.factor, k.min_cap);
            CHECK(cap == k.loop(n));
            CHECK((cap & (cap - 1)) == 0 && cap >= k.min_cap && cap >= k.factor * n);
        }
    }
}

// ---- packed-list checks -----------------------------------------------------------------------------------------------------------------------
static bool err_is(const char *text) { return g_err == text; }

static void check_packed_lists()
{
    const int64_t good[4] = {0, 2, 2, 5}, shifted[4] = {1, 2, 2, 5}, falling[4] = {0, 3, 2, 5}, none[1] = {0}, none_bad[1] = {4};
    const unsigned char ijk[15] = {0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3, 4, 5, 7};
    g_err = "untouched";
    CHECK(pl_check_counts(3, 5) == SN_OK && pl_check_counts(3, 0) == SN_OK && pl_check_counts(0, 0) == SN_OK);
    CHECK(pl_check_host_offsets(3, good) == SN_OK && pl_check_host_offsets(0, none) == SN_OK);
    CHECK(pl_check_host_ijk(5, ijk, 8) == SN_OK && pl_check_host_ijk(0, nullptr, 8) == SN_OK);
    CHECK(err_is("untouched"));                                  // an accepted list leaves the error text alone

    CHECK(pl_check_host_offsets(3, shifted) == SN_ERR_ARG && err_is("offsets[0] = 1, must be 0"));
    CHECK(pl_check_host_offsets(0, none_bad) == SN_ERR_ARG && err_is("offsets[0] = 4, must be 0"));
    CHECK(pl_check_host_offsets(3, falling) == SN_ERR_ARG && err_is("offsets table decreases at cube 1"));
    CHECK(pl_check_counts(0, 5) == SN_ERR_ARG && err_is("offsets table of 0 cubes holds 5 voxels"));
    CHECK(pl_check_counts(3, -1) == SN_ERR_ARG && err_is("total must be >= 0"));
    CHECK(pl_check_counts(0, -1) == SN_ERR_ARG && err_is("total must be >= 0"));      // the order the entries test in
    CHECK(pl_check_host_ijk(5, ijk, 7) == SN_ERR_ARG && err_is("voxel 2: ijk component 7 >= Dc = 7"));      // a component == Dc
}

int main()
{
    for (size_t n : {(size_t)0, (size_t)1, (size_t)1000}) {
        check_carve(normals_layout, n);
        check_carve(grid_layout, n);
    }
    check_carve_empty_get();
    check_table_cap();
    check_packed_lists();
    CHECK(round_up(0, 8) == 0 && round_up(1, 8) == 8 && round_up(8, 8) == 8 && round_up(9, 8) == 16);
    CHECK(fail(SN_ERR_STATE, "%s %d", "text", 3) == SN_ERR_STATE && err_is("text 3"));
    printf("SN-HOST-CHECK-OK\n");
    return 0;
}
