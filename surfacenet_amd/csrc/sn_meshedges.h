// sn_meshedges.h — the host side of the edge table (meshedges.h): what a stage that stands on it does before its own launches and at its one
// read, written once. sn_meshedges.hip defines the build's kernels and the members that are no templates.
//   MsmStage s(c, host);
//   rc = s.build(c->xyz_ws, V, verts, F, nv, faces, origin, resol, b.st, [&](Carve &w) { b.parent = w.get<unsigned>(n); ... });
//   if (rc != SN_OK || s.empty) return rc;
//   ... the stage's kernels on s.e ...
//   if ((rc = s.status(&st, b.st)) != SN_OK) return rc;          the one read, and the refusal the build's block asks for
//   rc = s.m.outputs(...); ... the kernels that write them ...; return s.m.finish();
#pragma once
#include "sn_internal.h"
#include "meshedges.h"

// the build's block within a stage's status block: the block itself, or its first member `msm`
inline MsmStat *msm_head(MsmStat *s) { return s; }
template <typename T> MsmStat *msm_head(T *s) { return s ? &s->msm : nullptr; }

struct MsmStage {
    sn_ctx *c;
    HostMirror m;                       // of verts and faces, and of whatever outputs the stage names later
    MsmEdges e;                         // the table, once build() has returned
    bool empty = false;                 // build() met a mesh of no face: nothing was built, all counts are 0 and nothing is written
    MsmStage(sn_ctx *ctx, bool host) : c(ctx), m(ctx, host) {}

    // Mirrors verts and faces, sizes the table, places [status block T | the build's arrays | what extra(w) adds] in ws, zeroes the block and
    // runs the build on the context's stream. any_mesh: the caller has checked its arrays itself and takes a mesh of no face too (the
    // smoother); otherwise no face sets `empty` and a missing array is refused here.
    template <typename T, typename Extra>
    int build(DevBuf &ws, int V, const double *verts, int F, int nv, const int32_t *faces, const double *origin, double resol, T *&st,
              Extra &&extra, bool any_mesh = false)
    {
        int rc = open(V, verts, F, nv, faces, origin, resol, any_mesh);
        if (rc != SN_OK || empty) return rc;
        auto layout = [&](Carve &w) {
            st = w.get<T>(1);
            e.st = msm_head(st);                                // the build writes into the head of the one block the host reads
            carve(w);
            extra(w);
        };
        if ((rc = dev_carve(c, ws, layout, 256)) != SN_OK) return rc;
        HIPCHK(dev_fill(c, st, 0, 1));
        return run();
    }

    // The stage's status block on the host, and what the build's part says of the input, in the words every stage refuses with (SN_OK:
    // nothing). degree_limit: a vertex of 2^24 or more edges is refused too (the smoother's sums).
    template <typename T>
    int status(T *host_st, const T *st, bool degree_limit = false)
    {
        HIPCHK(read_status(c, host_st, st));
        return report(*msm_head(host_st), degree_limit);
    }

    size_t cap() const { return (size_t)e.mask + 1; }           // slots of the table

private:
    int open(int V, const double *verts, int F, int nv, const int32_t *faces, const double *origin, double resol, bool any_mesh);
    void carve(Carve &w);
    int run();
    int report(const MsmStat &st, bool degree_limit) const;
};
