// sn_host_check.cpp — stand-alone check of surfacenet_amd/csrc/sn_host.h, the part of the entry points' host plumbing that needs no device:
// Carve, MirrorPlan, table_cap, the packed-list checks and the mesh stages' shared checks (mesh_check_common, mesh_check_caps, mesh_report_bad,
// the simplifier's msim_check_args). tests/test_host_plumbing.py compiles it with a plain host compiler under the address and
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

// a workspace of fourteen arrays of the sizes sn_normals handles: n cubes, T voxels, K views per cube of V cameras
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

// ---- MirrorPlan: a host buffer as the "device", memcpy as the copy -----------------------------------------------------------------------------
// What sn_internal.h's HostMirror does with a plan, without a device: one buffer per layout (measured, then placed), the recorded inputs
// copied in, an output's first `count` elements copied back early (back), every output not yet returned copied back at its staged size
// (finish). `copies` lists what went to the caller's arrays, in order.
struct HostExec {
    struct Copy { const void *host; size_t bytes; };
    std::vector<Copy> copies;
    MirrorPlan plan;
    std::vector<unsigned char> buf[2];                           // the inputs' and the outputs' buffer
    unsigned char *base[2] = {nullptr, nullptr};
    size_t size[2] = {0, 0};
    size_t scratch_off = 0, scratch_bytes = 0;                   // a scratch region taken between the arrays of the first layout
    void carve(int which, const std::function<void(Carve &)> &layout)
    {
        Carve measure;
        const size_t before = plan.recs.size();
        layout(measure);
        CHECK(plan.recs.size() == before);                       // the measuring pass records nothing
        size[which] = measure.off;
        buf[which].assign(measure.off + 512, 0xee);
        base[which] = buf[which].data() + (256 - reinterpret_cast<uintptr_t>(buf[which].data()) % 256) % 256;
        Carve place{base[which]};
        layout(place);
        CHECK(place.off == measure.off);                         // the two passes agree
        if (which == 0)
            for (const MirrorPlan::Rec &r : plan.recs)
                if (r.input && r.bytes) memcpy(r.dev, r.host, r.bytes);
    }
    template <typename T> void back(const T *dev, size_t count)
    {
        if (!plan.on || !dev) return;
        const MirrorPlan::Rec *r = plan.note_back(dev, count * sizeof(T));
        CHECK(r && !r->input && count * sizeof(T) <= r->bytes);
        if (count) to_host(r->host, dev, count * sizeof(T));
    }
    void finish()
    {
        CHECK(plan.each_pending([&](void *host, const void *dev, size_t bytes) { return to_host(host, dev, bytes); }));
    }
    bool to_host(void *host, const void *dev, size_t bytes)
    {
        memcpy(host, dev, bytes);
        copies.push_back(Copy{host, bytes});
        return true;
    }
    // every recorded region: aligned, inside its buffer, apart from every other and from the scratch
    void check_regions() const
    {
        for (size_t i = 0; i < plan.recs.size(); ++i) {
            const MirrorPlan::Rec &r = plan.recs[i];
            const int which = r.input ? 0 : 1;
            const unsigned char *d = static_cast<const unsigned char *>(r.dev);
            const size_t room = std::max<size_t>(r.bytes, 1);
            CHECK(reinterpret_cast<uintptr_t>(d) % 256 == 0);
            CHECK(d >= base[which] && d + room <= base[which] + size[which]);
            if (r.input && scratch_bytes) CHECK(d + room <= base[0] + scratch_off || d >= base[0] + scratch_off + scratch_bytes);
            for (size_t j = 0; j < i; ++j) {
                const unsigned char *e = static_cast<const unsigned char *>(plan.recs[j].dev);
                CHECK(d + room <= e || e + std::max<size_t>(plan.recs[j].bytes, 1) <= d);
            }
            CHECK(plan.find(r.dev) == &r);
        }
    }
};

template <typename T> static std::vector<T> pattern(size_t count, unsigned seed)
{
    std::vector<T> v(count + 1);                                 // (+ 1: data() of an empty array is still a pointer that was "given")
    unsigned char *b = reinterpret_cast<unsigned char *>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) b[i] = (unsigned char)(seed * 131u + i * 7u + (i >> 8));
    return v;
}

template <typename T> static void check_arrived(const HostExec &x, const T *dev, const std::vector<T> &host, size_t count)
{
    const MirrorPlan::Rec *r = x.plan.find(dev);
    CHECK(r && r->input && r->host == host.data() && r->bytes == count * sizeof(T));
    CHECK(count == 0 || memcmp(dev, host.data(), count * sizeof(T)) == 0);
}

// an output of `count` staged elements: the kernels "write" a pattern, back(m) copies the first m, the rest of the caller's array keeps its sentinel
template <typename T> static void check_back(HostExec &x, T *dev, std::vector<T> &host, size_t count)
{
    const std::vector<T> wrote = pattern<T>(count, 77);
    if (count) memcpy(dev, wrote.data(), count * sizeof(T));
    for (size_t m : {(size_t)0, count / 2, count}) {
        memset(host.data(), 0x5c, host.size() * sizeof(T));
        x.back(dev, m);
        const unsigned char *h = reinterpret_cast<const unsigned char *>(host.data());
        CHECK(m == 0 || memcmp(h, wrote.data(), m * sizeof(T)) == 0);
        for (size_t i = m * sizeof(T); i < host.size() * sizeof(T); ++i) CHECK(h[i] == 0x5c);
    }
}

// ---- finish(): what goes back without being asked for ------------------------------------------------------------------------------------
// A caller's array of count + 1 elements and what the plan made of it: `dev` is the swapped pointer (the array itself with the mirror off).
struct Arr { unsigned char *host; size_t host_bytes; unsigned char *dev; size_t bytes, elem; };
template <typename T> static Arr arr(std::vector<T> &host, const T *dev, size_t count)
{
    return Arr{reinterpret_cast<unsigned char *>(host.data()), host.size() * sizeof(T), reinterpret_cast<unsigned char *>(const_cast<T *>(dev)),
               count * sizeof(T), sizeof(T)};
}
static void scribble(unsigned char *p, size_t bytes, unsigned seed)
{
    for (size_t i = 0; i < bytes; ++i) p[i] = (unsigned char)(seed * 131u + i * 7u + (i >> 8));
}
static bool scribbled(const unsigned char *p, size_t bytes, unsigned seed)
{
    for (size_t i = 0; i < bytes; ++i)
        if (p[i] != (unsigned char)(seed * 131u + i * 7u + (i >> 8))) return false;
    return true;
}

// The call ends with finish() and names no output again. early: each output's first half is returned by back() before the kernels "write" a
// second pattern, so whatever finish() copied of it would show. The inputs' device copies are overwritten too: none of that may come back.
static void check_finish(HostExec &x, const std::vector<Arr> &ins, const std::vector<Arr> &outs, bool early)
{
    std::vector<std::vector<unsigned char>> in_before;
    for (const Arr &a : ins) in_before.emplace_back(a.host, a.host + a.host_bytes);
    for (const Arr &a : outs) memset(a.host, 0x5c, a.host_bytes);
    if (!x.plan.on) {                                            // a device form: nothing is copied, by back() or by finish()
        for (const Arr &a : outs) { CHECK(a.dev == a.host); x.back(a.dev, a.bytes / 2); }
        x.finish();
        CHECK(x.copies.empty());
        for (const Arr &a : outs)
            for (size_t i = 0; i < a.host_bytes; ++i) CHECK(a.host[i] == 0x5c);
        for (size_t k = 0; k < ins.size(); ++k) CHECK(memcmp(ins[k].host, in_before[k].data(), ins[k].host_bytes) == 0);
        return;
    }
    x.copies.clear();
    for (const Arr &a : outs) scribble(a.dev, a.bytes, 21);
    std::vector<size_t> expect;                                  // bytes of each output that arrive
    for (const Arr &a : outs) expect.push_back(early ? a.bytes / a.elem / 2 * a.elem : a.bytes);
    if (early) {
        for (size_t k = 0; k < outs.size(); ++k) x.back(outs[k].dev, expect[k]);
        for (const Arr &a : outs) scribble(a.dev, a.bytes, 22);
    }
    for (const Arr &a : ins) scribble(a.dev, a.bytes, 23);
    x.finish();
    size_t n_copies = 0;
    for (size_t k = 0; k < outs.size(); ++k) {
        const Arr &a = outs[k];
        CHECK(scribbled(a.host, expect[k], 21));                 // the first pattern, at exactly the expected size
        for (size_t i = expect[k]; i < a.host_bytes; ++i) CHECK(a.host[i] == 0x5c);
        if (!expect[k]) continue;
        CHECK(n_copies < x.copies.size() && x.copies[n_copies].host == a.host && x.copies[n_copies].bytes == expect[k]);      // once, in order
        ++n_copies;
    }
    CHECK(x.copies.size() == n_copies);                          // nothing else: no input, no output twice, none at its staged size after back()
    for (size_t k = 0; k < ins.size(); ++k) CHECK(memcmp(ins[k].host, in_before[k].data(), ins[k].host_bytes) == 0);
    x.finish();
    CHECK(x.copies.size() == n_copies);                          // a second finish() has nothing left to return
}

enum Ending { ENDS_BACK, ENDS_FINISH, ENDS_EARLY_FINISH };       // explicit back() of every output | finish() alone | back() of a half, then finish()

// sn_normals' arrays (sn_normals.hip nm_call): n cubes, T voxels, K views per cube of V cameras; the moments are not asked for (a null output)
static void check_mirror_normals(size_t n, bool on, Ending ending)
{
    const size_t T = 7 * n, K = 5, V = 9;
    std::vector<int64_t> off = pattern<int64_t>(n + 1, 1);
    std::vector<uint32_t> cube = pattern<uint32_t>(3 * n, 2);
    std::vector<uint8_t> ijk = pattern<uint8_t>(3 * T, 3), mask = pattern<uint8_t>(T, 4);
    std::vector<float> xyz = pattern<float>(3 * n, 5), resol = pattern<float>(n, 6), normals(3 * T + 1);
    std::vector<int32_t> view = pattern<int32_t>(n * K, 7);
    std::vector<double> cams = pattern<double>(3 * V, 8);
    const int64_t *p_off = off.data(); const uint32_t *p_cube = cube.data(); const uint8_t *p_ijk = ijk.data(), *p_mask = mask.data();
    const float *p_xyz = xyz.data(), *p_resol = resol.data(); const int32_t *p_view = view.data(); const double *p_cams = cams.data();
    float *p_normals = normals.data(); int32_t *p_moments = nullptr;
    HostExec x;
    x.plan.on = on;
    float *scratch = nullptr;
    x.carve(0, [&](Carve &w) {
        x.plan.in(w, p_off, n + 1); x.plan.in(w, p_cube, 3 * n); x.plan.in(w, p_ijk, 3 * T); x.plan.in(w, p_mask, T);
        scratch = w.get<float>(n);                               // scratch between the arrays, as the weight entries take their logits
        if (w.base) { x.scratch_off = (size_t)(reinterpret_cast<unsigned char *>(scratch) - w.base); x.scratch_bytes = std::max<size_t>(n, 1) * sizeof(float); }
        x.plan.in(w, p_xyz, 3 * n); x.plan.in(w, p_resol, n); x.plan.in(w, p_view, n * K); x.plan.in(w, p_cams, 3 * V);
    });
    x.carve(1, [&](Carve &w) { x.plan.out(w, p_normals, 3 * T); x.plan.out(w, p_moments, 10 * T); });
    CHECK(p_moments == nullptr);                                 // a null array takes no region and stays null
    const std::vector<Arr> ins = {arr(off, p_off, n + 1), arr(cube, p_cube, 3 * n), arr(ijk, p_ijk, 3 * T), arr(mask, p_mask, T),
                                  arr(xyz, p_xyz, 3 * n), arr(resol, p_resol, n), arr(view, p_view, n * K), arr(cams, p_cams, 3 * V)};
    const std::vector<Arr> outs = {arr(normals, p_normals, 3 * T)};
    if (!on) {                                                   // a device form: no pointer changes, no region is taken
        CHECK(x.plan.recs.empty() && p_off == off.data() && p_cams == cams.data() && p_normals == normals.data());
        CHECK(x.size[0] == std::max<size_t>(n, 1) * sizeof(float) && x.size[1] == 0);      // (the scratch alone)
        x.back(p_normals, 3 * T);
        if (ending != ENDS_BACK) check_finish(x, ins, outs, ending == ENDS_EARLY_FINISH);
        return;
    }
    CHECK(x.plan.recs.size() == 9);
    x.check_regions();
    check_arrived(x, p_off, off, n + 1); check_arrived(x, p_cube, cube, 3 * n); check_arrived(x, p_ijk, ijk, 3 * T); check_arrived(x, p_mask, mask, T);
    check_arrived(x, p_xyz, xyz, 3 * n); check_arrived(x, p_resol, resol, n); check_arrived(x, p_view, view, n * K); check_arrived(x, p_cams, cams, 3 * V);
    CHECK(x.plan.find(scratch) == nullptr && x.plan.find(normals.data()) == nullptr);
    if (ending == ENDS_BACK) check_back(x, p_normals, normals, 3 * T);
    else check_finish(x, ins, outs, ending == ENDS_EARLY_FINISH);
}

// sn_mesh's arrays (sn_mesh.hip ms_call / ms_run): the outputs are staged at the counts the kernels found, nv vertices and nq quads
static void check_mirror_mesh(size_t n, bool on, Ending ending)
{
    const size_t T = 7 * n, nv = 3 * n, nq = 2 * n;
    std::vector<int64_t> off = pattern<int64_t>(n + 1, 11), vsrc(nv + 1);
    std::vector<uint32_t> cube = pattern<uint32_t>(3 * n, 12);
    std::vector<uint8_t> ijk = pattern<uint8_t>(3 * T, 13), mask = pattern<uint8_t>(T, 14);
    std::vector<float> nrm = pattern<float>(3 * T, 15), vmm(3 * nv + 1);
    std::vector<double> vlat(3 * nv + 1);
    std::vector<int32_t> quads(4 * nq + 1);
    const int64_t *p_off = off.data(); const uint32_t *p_cube = cube.data(); const uint8_t *p_ijk = ijk.data(), *p_mask = mask.data();
    const float *p_nrm = nrm.data();
    float *p_vmm = vmm.data(); double *p_vlat = vlat.data(); int32_t *p_vcell = nullptr, *p_quads = quads.data(); int64_t *p_vsrc = vsrc.data();
    HostExec x;
    x.plan.on = on;
    x.carve(0, [&](Carve &w) { x.plan.in(w, p_off, n + 1); x.plan.in(w, p_cube, 3 * n); x.plan.in(w, p_ijk, 3 * T); x.plan.in(w, p_mask, T); x.plan.in(w, p_nrm, 3 * T); });
    x.carve(1, [&](Carve &w) {
        x.plan.out(w, p_vmm, 3 * nv); x.plan.out(w, p_vlat, 3 * nv); x.plan.out(w, p_vcell, 3 * nv); x.plan.out(w, p_vsrc, nv); x.plan.out(w, p_quads, 4 * nq);
    });
    CHECK(p_vcell == nullptr);
    const std::vector<Arr> ins = {arr(off, p_off, n + 1), arr(cube, p_cube, 3 * n), arr(ijk, p_ijk, 3 * T), arr(mask, p_mask, T), arr(nrm, p_nrm, 3 * T)};
    const std::vector<Arr> outs = {arr(vmm, p_vmm, 3 * nv), arr(vlat, p_vlat, 3 * nv), arr(vsrc, p_vsrc, nv), arr(quads, p_quads, 4 * nq)};
    if (!on) {
        CHECK(x.plan.recs.empty() && x.size[0] == 0 && x.size[1] == 0);
        CHECK(p_off == off.data() && p_nrm == nrm.data() && p_vmm == vmm.data() && p_quads == quads.data());
        if (ending != ENDS_BACK) check_finish(x, ins, outs, ending == ENDS_EARLY_FINISH);
        return;
    }
    CHECK(x.plan.recs.size() == 9);
    x.check_regions();
    check_arrived(x, p_off, off, n + 1); check_arrived(x, p_cube, cube, 3 * n); check_arrived(x, p_ijk, ijk, 3 * T); check_arrived(x, p_mask, mask, T);
    check_arrived(x, p_nrm, nrm, 3 * T);
    if (ending != ENDS_BACK) return check_finish(x, ins, outs, ending == ENDS_EARLY_FINISH);
    check_back(x, p_vmm, vmm, 3 * nv); check_back(x, p_vlat, vlat, 3 * nv); check_back(x, p_vsrc, vsrc, nv); check_back(x, p_quads, quads, 4 * nq);
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

// ---- the mesh stages' shared checks --------------------------------------------------------------------------------------------------------------
static void check_mesh_stages()
{
    using namespace sn;
    static_assert(MESH_MAX_ITEMS == 1 << 28 && MESH_LO == -4.0 && MESH_HI == 2097144.0 && MESH_ERR_INDEX == 1 && MESH_ERR_RANGE == 2 &&
                  MESH_NO_BAD == ~0ull && mesh_first_bad(5, MESH_ERR_RANGE) == 42, "the shared input contract");
    const double origin[3] = {0.0, -20.0, 3.5};
    g_err = "untouched";
    CHECK(mesh_check_common(100, 50, 3, origin, 0.4) == SN_OK && mesh_check_common(1 << 28, 1 << 28, 4, origin, 0.4) == SN_OK);
    CHECK(mesh_check_common(0, 0, 3, origin, 0.4) == SN_OK && mesh_check_caps(0, 0) == SN_OK && mesh_check_caps(1ll << 40, 7) == SN_OK);
    CHECK(mesh_report_bad(MESH_NO_BAD, 16) == SN_OK);           // the sentinel: no bad face
    CHECK(err_is("untouched"));
    CHECK(mesh_check_common(-1, 1, 3, origin, 0.4) == SN_ERR_ARG && err_is("n_verts and n_faces must be >= 0"));
    CHECK(mesh_check_common((1 << 28) + 1, 1, 3, origin, 0.4) == SN_ERR_ARG && err_is("n_verts = 268435457, n_faces = 1: at most 2^28 of either"));
    CHECK(mesh_check_common(1, 1, 5, origin, 0.4) == SN_ERR_ARG && err_is("nv = 5: faces are triangles (3) or quads (4)"));
    CHECK(mesh_check_common(1, 1, 3, origin, 0.0) == SN_ERR_ARG && err_is("resol = 0 must be finite and > 0"));
    const double bad_origin[3] = {0.0, NAN, 3.5};
    CHECK(mesh_check_common(1, 1, 3, bad_origin, 0.4) == SN_ERR_ARG && err_is("origin[1] = nan is not finite"));
    CHECK(mesh_check_common(-1, 1, 5, bad_origin, 0.0) == SN_ERR_ARG && err_is("n_verts and n_faces must be >= 0"));      // the order
    CHECK(mesh_check_caps(-1, 1) == SN_ERR_ARG && err_is("cap_verts and cap_faces must be >= 0"));
    CHECK(mesh_check_caps(1, -1) == SN_ERR_ARG && err_is("cap_verts and cap_faces must be >= 0"));
    long long counts[8] = {5, 5, 5, 5, 5, 5, 5, 5};
    CHECK(mesh_check_counts(nullptr, counts, 8) == SN_ERR_ARG && err_is("null context") && counts[0] == 5);
    CHECK(mesh_check_counts(counts, nullptr, 8) == SN_ERR_ARG && err_is("counts is required"));
    CHECK(mesh_check_counts(counts, counts, 4) == SN_OK && counts[0] == 0 && counts[3] == 0 && counts[4] == 5);
    static_assert(mesh_index_ok(0, 1) && !mesh_index_ok(1, 1) && !mesh_index_ok(-1, 1) && !mesh_index_ok(0, 0), "an index lies in [0, V)");
    static_assert(mesh_coord_ok(-4.0) && !mesh_coord_ok(-4.000001) && mesh_coord_ok(2097143.999) && !mesh_coord_ok(2097144.0) && !mesh_coord_ok(NAN),
                  "a coordinate lies in [-4, 2^21 - 8)");

    // the first bad face a kernel reported: both kinds, the largest face there can be, and the smaller face winning the minimum
    CHECK(mesh_report_bad(mesh_first_bad(5, MESH_ERR_INDEX), 16) == SN_ERR_ARG && err_is("face 5 names a vertex outside [0, 16)"));
    CHECK(mesh_report_bad(mesh_first_bad(3, MESH_ERR_RANGE), 16) == SN_ERR_ARG &&
          err_is("face 3: a coordinate of one of its vertices is outside [-4, 2^21 - 8) lattice cells (or not a number)"));
    CHECK(mesh_report_bad(mesh_first_bad((1 << 28) - 1, MESH_ERR_INDEX), 1 << 28) == SN_ERR_ARG &&
          err_is("face 268435455 names a vertex outside [0, 268435456)"));
    CHECK(mesh_report_bad(mesh_first_bad((1 << 28) - 1, MESH_ERR_RANGE), 1 << 28) == SN_ERR_ARG &&
          err_is("face 268435455: a coordinate of one of its vertices is outside [-4, 2^21 - 8) lattice cells (or not a number)"));
    CHECK(mesh_first_bad(2, MESH_ERR_RANGE) < mesh_first_bad(5, MESH_ERR_INDEX) && mesh_first_bad((1 << 28) - 1, 7) < MESH_NO_BAD);

    // the simplifier's arguments: every end of every range is legal, one step beyond is SN_ERR_ARG and names the argument
    const sn_mesh_simplify_cfg ok = {8, 0, {0.0, -20.0, 3.5}, 0.4};
    CHECK(msim_check_args(&ok, 100, 50, 100, 50) == SN_OK && msim_check_args(&ok, 1 << 28, 1 << 28, 0, 0) == SN_OK);
    CHECK(msim_check_args(&ok, 0, 0, 0, 0) == SN_OK);
    CHECK(msim_check_args(nullptr, 1, 1, 1, 1) == SN_ERR_ARG && err_is("null cfg"));
    auto refused = [&](sn_mesh_simplify_cfg c, int V, int F, long long cv, long long cf, const char *word) {
        CHECK(msim_check_args(&c, V, F, cv, cf) == SN_ERR_ARG && g_err.find(word) != std::string::npos);
    };
    refused(ok, (1 << 28) + 1, 1, 1, 1, "n_verts"); refused(ok, 1, (1 << 28) + 1, 1, 1, "n_faces");
    refused(ok, -1, 1, 1, 1, "n_verts"); refused(ok, 1, -1, 1, 1, "n_faces");
    refused(ok, 1, 1, -1, 1, "cap_verts"); refused(ok, 1, 1, 1, -1, "cap_faces");
    sn_mesh_simplify_cfg c = ok;
    c.cell = 2; CHECK(msim_check_args(&c, 8, 4, 8, 4) == SN_OK); c.cell = 64; CHECK(msim_check_args(&c, 8, 4, 8, 4) == SN_OK);
    c.cell = 1; refused(c, 8, 4, 8, 4, "cell"); c.cell = 65; refused(c, 8, 4, 8, 4, "cell"); c.cell = -8; refused(c, 8, 4, 8, 4, "cell");
    c = ok; c.placement = 1; CHECK(msim_check_args(&c, 8, 4, 8, 4) == SN_OK);
    c.placement = 2; refused(c, 8, 4, 8, 4, "placement"); c.placement = -1; refused(c, 8, 4, 8, 4, "placement");
    c = ok; c.resol = 0.0; refused(c, 8, 4, 8, 4, "resol"); c.resol = -0.4; refused(c, 8, 4, 8, 4, "resol");
    c.resol = INFINITY; refused(c, 8, 4, 8, 4, "resol"); c.resol = NAN; refused(c, 8, 4, 8, 4, "resol");
    c = ok; c.origin[1] = NAN; refused(c, 8, 4, 8, 4, "origin[1]"); c = ok; c.origin[2] = -INFINITY; refused(c, 8, 4, 8, 4, "origin[2]");
    // the shared refusals read as the smoother's and the filler's do
    const sn_mesh_smooth_cfg s = {1, 0, 0, 1, {0.0, 0.0, 0.0}, 1.0};
    const sn_mesh_fill_cfg f = {64, 0, {0.0, 0.0, 0.0}, 1.0};
    CHECK(msm_check_args(&s, (1 << 28) + 1, 1, 3) == SN_ERR_ARG);
    const std::string words = g_err;
    CHECK(mfl_check_args(&f, (1 << 28) + 1, 1, 3, 1, 1) == SN_ERR_ARG && g_err == words);
    CHECK(msim_check_args(&ok, (1 << 28) + 1, 1, 1, 1) == SN_ERR_ARG && g_err == words);
}

int main()
{
    for (size_t n : {(size_t)0, (size_t)1, (size_t)1000}) {
        check_carve(normals_layout, n);
        check_carve(grid_layout, n);
        for (bool on : {true, false}) {
            check_mirror_normals(n, on, ENDS_BACK);
            check_mirror_mesh(n, on, ENDS_BACK);
        }
    }
    for (size_t n : {(size_t)0, (size_t)1, (size_t)5})
        for (bool on : {true, false})
            for (Ending ending : {ENDS_FINISH, ENDS_EARLY_FINISH}) {
                check_mirror_normals(n, on, ending);
                check_mirror_mesh(n, on, ending);
            }
    check_carve_empty_get();
    check_table_cap();
    check_packed_lists();
    check_mesh_stages();
    CHECK(round_up(0, 8) == 0 && round_up(1, 8) == 8 && round_up(8, 8) == 8 && round_up(9, 8) == 16);
    CHECK(fail(SN_ERR_STATE, "%s %d", "text", 3) == SN_ERR_STATE && err_is("text 3"));
    printf("SN-HOST-CHECK-OK\n");
    return 0;
}
