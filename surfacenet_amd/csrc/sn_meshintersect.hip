// sn_meshintersect.hip — C ABI of the mesh self-intersection stage (meshintersect.h). The device form works on the
// caller's device arrays; the host form is the same computation on the host mirror's device copies of its arrays (sn_internal.h HostMirror).
// The quantised positions are the edge table's, and the sequence around its build is sn_meshedges.h's (MsmStage); everything after it is plain
// launches on the context's stream. The host reads the status block once before any output is touched - the first bad face, the hits - and,
// when something was hit, the counts once more after the sort; a clean mesh costs the one read.
#include "sn_meshedges.h"
#include "bitonic.h"
#include "meshintersect.h"
#include "scan.h"

namespace {

constexpr long long MXI_MAX_KEYS = 1ll << 30;          // hits of triangle pairs: the sorted list's scan is an int's

// the caller's outputs: device arrays in the device form, host arrays in the host form
struct MxiOut { unsigned char *face_hit; int32_t *face_pairs; int32_t *pairs; };

int mxi_check(sn_ctx *c, const sn_mesh_intersect_cfg *cfg, int n_verts, int n_faces, int nv, long long *counts)
{
    const int rc = mesh_check_counts(c, counts, 8);
    return rc != SN_OK ? rc : mxi_check_args(cfg, n_verts, n_faces, nv);
}

// a test-only switch's integer in [lo, hi], or `none`
int mxi_switch(const char *name, int lo, int hi, int none)
{
    const char *v = sn_ab_switch(name);
    if (!v || !*v) return none;
    const int x = atoi(v);
    return x < lo || x > hi ? none : x;
}

// the broad phase's narrow half: the candidates of every cell, tested exactly; the hits' keys as far as the list goes
int mxi_pairs(sn_ctx *c, const MsmEdges &a, const MxiArgs &b)
{
    const unsigned lb = loop_blocks(c);
    ProfScope ps(c, "mxi_pairs", 0, (double)b.ecap * 8.0 + (double)b.n_tris * (24.0 + 12.0 + 72.0));
    HIPCHK(dev_fill(c, &b.st->w[MXI_W_COUNTS + 2], 0, 1));
    HIPCHK(dev_fill(c, &b.st->w[MXI_W_KEYS], 0, 2));           // the hits, the listed cells
    LAUNCH(mxi_pairs_kernel, dim3(std::min(blocks(b.ecap, MXI_NT), lb)), dim3(MXI_NT), a, b);
    LAUNCH(mxi_pairs_big_kernel, dim3(lb), dim3(MXI_NT), a, b);
    return SN_OK;
}

// What both forms do once their arguments are checked.
int mxi_run(sn_ctx *c, bool host, const sn_mesh_intersect_cfg *cfg, int V, const double *verts, int F, int nv, const int32_t *faces, MxiOut d,
            long long *counts)
{
    MsmStage s(c, host);
    const size_t n = (size_t)F;
    const double origin[3] = {0.0, 0.0, 0.0};
    MxiArgs b;
    memset(&b, 0, sizeof b);
    b.tshift = nv - 3;
    b.n_tris = (long long)F << b.tshift;
    b.cap_pairs = cfg->cap_pairs;
    // The grid level: the smallest whose entries number at most 8 per triangle (tools/bench_meshintersect.py, profiles/meshintersect/). The
    // test-only twin reads SN_MXI_LEVEL to force one and SN_MXI_BUDGET for the A/B of the budget. The results are the same bytes.
    b.force_level = mxi_switch("SN_MXI_LEVEL", 0, MXI_LEVELS - 1, -1);
    b.budget = mxi_switch("SN_MXI_BUDGET", 1, 64, 8);
    b.ecap = std::max(b.budget, 8) * b.n_tris;                  // (level 21: at most 8 cells per triangle)
    int rc = s.build(c->mxi_ws, V, verts, F, nv, faces, origin, 1.0, b.st, [&](Carve &w) {
        b.box = w.get<int>(6 * (size_t)b.n_tris);
        b.fpairs = w.get<unsigned>(n);
    });
    if (rc != SN_OK || s.empty) return rc;                      // no face: all counts 0, nothing written
    const MsmEdges &a = s.e;
    HostMirror &m = s.m;
    const unsigned fb = blocks(F, MXI_NT), tb = blocks(b.n_tris, MXI_NT);
    {
        // per face: its indices and flags, its corners' records, a box per triangle
        ProfScope ps(c, "mxi_tris", 0, (double)F * nv * (4.0 + 4.0 + 24.0) + (double)b.n_tris * 24.0);
        LAUNCH(mxi_tris_kernel, dim3(fb), dim3(MXI_NT), a, b);
    }
    MxiStat st;
    if (b.force_level >= 0) {                                   // (twin only) a forced level's entries are whatever they are: size by them
        if ((rc = s.status(&st, b.st)) != SN_OK) return rc;
        const unsigned long long e = st.w[MXI_W_TOTALS + b.force_level];
        if (e > (1ull << 28)) return fail(SN_ERR_ARG, "SN_MXI_LEVEL = %d: %llu entries, at most 2^28", b.force_level, e);
        b.ecap = std::max<long long>(b.ecap, (long long)e);
    }
    const size_t gcap = table_cap((unsigned long long)b.ecap, 2, 1024);
    b.mask = (unsigned)(gcap - 1);
    b.bcap = b.ecap / (MXI_BIG + 1) + 1;
    int *sums = nullptr;
    auto grid = [&](Carve &w) {
        b.cells = w.get<unsigned long long>(gcap);
        b.count = w.get<int>(gcap);
        b.start = w.get<int>(gcap);
        b.cursor = w.get<int>(gcap);
        sums = w.get<int>(scan_sums(gcap));
        b.ent = w.get<unsigned>((size_t)b.ecap);
        b.ent_slot = w.get<unsigned>((size_t)b.ecap);
        b.big = w.get<unsigned>((size_t)b.bcap);
    };
    if ((rc = dev_carve(c, c->mxi_grid, grid, 256)) != SN_OK) return rc;
    // the key list: a key per face at least, or what an earlier call on this context needed; a mesh that hits more often grows it and walks
    // the pairs again
    int *head_sums = nullptr;
    auto pow2 = [](long long x) { long long p = PC_TILE; while (p < x) p <<= 1; return p; };
    b.kcap = std::max(pow2(F), c->mxi_kcap);
    auto keys_layout = [&](Carve &w) {
        b.keys = w.get<unsigned long long>((size_t)b.kcap);    // (a power of two >= PC_TILE: the sort pads within it)
        b.pos = w.get<int>((size_t)b.kcap);
        head_sums = w.get<int>(scan_sums((size_t)b.kcap));
    };
    if ((rc = dev_carve(c, c->mxi_keys, keys_layout)) != SN_OK) return rc;
    {
        ProfScope ps(c, "mxi_grid", 0, (double)gcap * 28.0 + (double)b.n_tris * 24.0 * 2 + (double)b.ecap * 16.0);
        LAUNCH(mxi_pick_kernel, dim3(1), dim3(64), b);
        HIPCHK(dev_fill(c, b.cells, 0xff, gcap));
        HIPCHK(dev_fill(c, b.count, 0, gcap));
        HIPCHK(dev_fill(c, b.cursor, 0, gcap));
        LAUNCH(mxi_cells_kernel<false>, dim3(tb), dim3(MXI_NT), b);
        if ((rc = scan_exclusive(c, b.count, b.start, (int)gcap, sums)) != SN_OK) return rc;
        LAUNCH(mxi_cells_kernel<true>, dim3(tb), dim3(MXI_NT), b);
    }
    if ((rc = mxi_pairs(c, a, b)) != SN_OK) return rc;
    // the one read before any output is touched: the first bad face, the level and its entries, the hits
    if ((rc = s.status(&st, b.st)) != SN_OK) return rc;
    if (st.w[MXI_W_ENTRIES] > (unsigned long long)b.ecap) return fail(SN_ERR_STATE, "%llu grid entries for room of %lld", st.w[MXI_W_ENTRIES], b.ecap);
    if ((long long)st.w[MXI_W_KEYS] >= MXI_MAX_KEYS) return fail(SN_ERR_ARG, "%llu intersecting triangle pairs: at most 2^30 - 1", st.w[MXI_W_KEYS]);
    if ((long long)st.w[MXI_W_KEYS] > b.kcap) {                 // count first, grow, walk again
        b.kcap = c->mxi_kcap = pow2((long long)st.w[MXI_W_KEYS]);
        if ((rc = dev_carve(c, c->mxi_keys, keys_layout)) != SN_OK) return rc;
        if ((rc = mxi_pairs(c, a, b)) != SN_OK) return rc;
        HIPCHK(read_status(c, &st, b.st));
        if ((long long)st.w[MXI_W_KEYS] > b.kcap) return fail(SN_ERR_STATE, "the second walk hit %llu pairs, the first %lld", st.w[MXI_W_KEYS], b.kcap);
    }
    b.n_keys = (long long)st.w[MXI_W_KEYS];
    HIPCHK(dev_fill(c, b.fpairs, 0, n));
    if (b.n_keys > 0) {
        const long long padded = pow2(b.n_keys);
        {
            ProfScope ps(c, "mxi_sort", 0, (double)padded * 16.0);
            if (padded > b.n_keys) LAUNCH(pc_pad_kernel, dim3(blocks(padded - b.n_keys, PC_NT)), dim3(PC_NT), b.keys, b.n_keys, padded);
            if ((rc = pc_sort(c, b.keys, padded)) != SN_OK) return rc;
        }
        ProfScope ps(c, "mxi_count", 0, (double)b.n_keys * 28.0 + (double)F * 4.0);
        const unsigned kb = blocks(b.n_keys, MXI_NT);
        LAUNCH(mxi_heads_kernel, dim3(kb), dim3(MXI_NT), b);
        if ((rc = scan_exclusive(c, b.pos, b.pos, (int)b.n_keys, head_sums)) != SN_OK) return rc;
        LAUNCH(mxi_count_kernel, dim3(kb), dim3(MXI_NT), b);
        LAUNCH(mxi_faces_kernel, dim3(fb), dim3(MXI_NT), b, (long long)F);
        HIPCHK(read_status(c, &st, b.st));                      // the counts: how many rows of the pair list there are
    }
    const long long P = (long long)st.w[MXI_W_COUNTS + 3], written = std::min(P, b.cap_pairs);
    rc = m.outputs([&](Carve &w) { m.out(w, d.face_hit, n); m.out(w, d.face_pairs, n); m.out(w, d.pairs, 2 * (size_t)written); });
    if (rc != SN_OK) return rc;
    b.face_hit = d.face_hit; b.face_pairs = d.face_pairs; b.pairs = d.pairs;
    {
        ProfScope ps(c, "mxi_emit", 0, (double)F * 9.0 + (double)written * 8.0 + (double)b.n_keys * 12.0);
        if (b.pairs && written > 0) {
            b.cap_pairs = written;
            LAUNCH(mxi_emit_pairs_kernel, dim3(blocks(b.n_keys, MXI_NT)), dim3(MXI_NT), b);
        }
        if (b.face_hit || b.face_pairs) LAUNCH(mxi_emit_faces_kernel, dim3(fb), dim3(MXI_NT), b, (long long)F);
    }
    if ((rc = m.finish()) != SN_OK) return rc;
    for (int k = 0; k < 7; ++k) counts[k] = (long long)st.w[MXI_W_COUNTS + k];
    counts[7] = d.pairs ? written : 0;
    return SN_OK;
}

}  // namespace

extern "C" int sn_mesh_intersect_dev(sn_ctx *c, const sn_mesh_intersect_cfg *cfg, int n_verts, const double *verts_dev, int n_faces, int nv,
                                     const int32_t *faces_dev, unsigned char *face_hit_dev, int32_t *face_pairs_dev, int32_t *pairs_dev,
                                     long long *counts)
{
    int rc;
    if ((rc = mxi_check(c, cfg, n_verts, n_faces, nv, counts)) != SN_OK) return rc;
    const MxiOut o = {face_hit_dev, face_pairs_dev, pairs_dev};
    return mxi_run(c, false, cfg, n_verts, verts_dev, n_faces, nv, faces_dev, o, counts);
}

extern "C" int sn_mesh_intersect(sn_ctx *c, const sn_mesh_intersect_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv,
                                 const int32_t *faces, unsigned char *face_hit, int32_t *face_pairs, int32_t *pairs, long long *counts)
{
    int rc;
    if ((rc = mxi_check(c, cfg, n_verts, n_faces, nv, counts)) != SN_OK) return rc;
    const MxiOut o = {face_hit, face_pairs, pairs};
    return mxi_run(c, true, cfg, n_verts, verts, n_faces, nv, faces, o, counts);
}
