// sn_meshsample.hip — C ABI of the surface sampling of a triangle mesh (meshsample.h). The device form works on the
// caller's device arrays; the host form is the same computation on the host mirror's device copies of its arrays (sn_internal.h HostMirror).
#include "sn_internal.h"
#include "meshsample.h"
#include "scan.h"

namespace {

int msmp_check_args(sn_ctx *c, int n_verts, int n_faces, double dst, long long cap_points, long long *n_points)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    if (!n_points) return fail(SN_ERR_ARG, "null argument");
    *n_points = 0;
    if (n_verts < 0 || n_faces < 0) return fail(SN_ERR_ARG, "n_verts and n_faces must be >= 0");
    if (n_faces == INT32_MAX) return fail(SN_ERR_ARG, "n_faces = %d: at most 2^31 - 2 faces", n_faces);
    if (!std::isfinite(dst) || !(dst > 0)) return fail(SN_ERR_ARG, "dst = %g must be finite and > 0", dst);
    if (cap_points < 0) return fail(SN_ERR_ARG, "cap_points must be >= 0");
    return SN_OK;
}

// What both forms do once their arguments are checked: the whole computation on device-resident verts and faces. host: the arrays are the
// caller's host arrays, and the mirror gives them their device copies (points / tri once the count is known).
int msmp_run(sn_ctx *c, bool host, int V, const double *verts, int F, const int32_t *faces, double dst, long long cap_points, double *points,
             int32_t *tri, long long *n_points)
{
    HIPCHK(hipSetDevice(c->device));
    HostMirror m(c, host);
    int rc = m.inputs([&](Carve &w) { m.in(w, verts, 3 * (size_t)V); m.in(w, faces, 3 * (size_t)F); });
    if (rc != SN_OK) return rc;
    MsmpStat *d_st = nullptr;
    int *off = nullptr, *sums = nullptr;
    auto layout = [&](Carve &w) {
        d_st = w.get<MsmpStat>(1);
        off = w.get<int>((size_t)F + 1);
        sums = w.get<int>(scan_sums((size_t)F + 1));
    };
    if ((rc = dev_carve(c, c->msmp_ws, layout, 256)) != SN_OK) return rc;
    MsmpIn in;
    memset(&in, 0, sizeof in);
    in.verts = verts; in.faces = faces; in.V = V; in.F = F; in.dst2 = dst * dst;
    MsmpStat st;
    HIPCHK(dev_fill(c, d_st, 0, 1));
    HIPCHK(dev_fill(c, &d_st->first_bad, 0xff, 1));
    HIPCHK(dev_fill(c, off + F, 0, 1));
    {
        ProfScope ps(c, "msmp_count", 0, (double)F * 16.0);
        LAUNCH(msmp_count_kernel, dim3((unsigned)(((long long)F + MSMP_NT * MSMP_FACES - 1) / (MSMP_NT * MSMP_FACES))), dim3(MSMP_NT), in, off, d_st);
    }
    HIPCHK(read_status(c, &st, d_st));
    if (st.first_bad != MESH_NO_BAD) {
        const long long f = (long long)(st.first_bad >> 3);
        const unsigned kind = (unsigned)(st.first_bad & 7);
        if (kind == MESH_ERR_INDEX) return mesh_report_bad(st.first_bad, V);
        if (kind == MSMP_ERR_FINITE) return fail(SN_ERR_ARG, "face %lld: a coordinate of one of its vertices is not finite", f);
        return fail(SN_ERR_ARG, "face %lld needs more than %d subdivisions at dst = %g", f, MSMP_MAX_N, dst);
    }
    if (st.total > (unsigned long long)INT32_MAX) {      // error path: walk the counts on the host for the face that crosses the limit
        std::vector<int> cnt((size_t)F);
        HIPCHK(hipMemcpy(cnt.data(), off, sizeof(int) * (size_t)F, hipMemcpyDeviceToHost));
        long long run = 0, f = 0;
        for (; f < F; ++f)
            if ((run += cnt[(size_t)f]) > INT32_MAX) break;
        return fail(SN_ERR_ARG, "%llu samples: at most 2^31 - 1 (reached at face %lld)", st.total, f);
    }
    const int M = (int)st.total;
    *n_points = M;
    if (M > cap_points) return fail(SN_ERR_ARG, "the outputs hold %lld samples, %d are needed", cap_points, M);
    if (M == 0 || (!points && !tri)) return SN_OK;
    {
        ProfScope ps(c, "msmp_scan", 0, (double)F * 12.0);
        if ((rc = scan_exclusive(c, off, off, F + 1, sums)) != SN_OK) return rc;      // off[F] = M
    }
    if ((rc = m.outputs([&](Carve &w) { m.out(w, points, 3 * (size_t)M); m.out(w, tri, (size_t)M); })) != SN_OK) return rc;
    {
        ProfScope ps(c, "msmp_emit", 0, (double)M * ((points ? 24.0 : 0.0) + (tri ? 4.0 : 0.0)));
        LAUNCH(msmp_emit_kernel, dim3((unsigned)(((long long)M + MSMP_RUN - 1) / MSMP_RUN)), dim3(MSMP_NT), in,
               (const int *)off, M, points, tri);
    }
    return m.finish();
}

}  // namespace

extern "C" int sn_mesh_sample_dev(sn_ctx *c, int n_verts, const double *verts_dev, int n_faces, const int32_t *faces_dev, double dst,
                                  long long cap_points, double *points_dev, int32_t *tri_dev, long long *n_points)
{
    int rc;
    if ((rc = msmp_check_args(c, n_verts, n_faces, dst, cap_points, n_points)) != SN_OK || n_faces == 0) return rc;
    if (!faces_dev || (n_verts > 0 && !verts_dev)) return fail(SN_ERR_ARG, "null argument");
    return msmp_run(c, false, n_verts, verts_dev, n_faces, faces_dev, dst, cap_points, points_dev, tri_dev, n_points);
}

extern "C" int sn_mesh_sample(sn_ctx *c, int n_verts, const double *verts, int n_faces, const int32_t *faces, double dst, long long cap_points,
                              double *points, int32_t *tri, long long *n_points)
{
    int rc;
    if ((rc = msmp_check_args(c, n_verts, n_faces, dst, cap_points, n_points)) != SN_OK || n_faces == 0) return rc;
    if (!faces || (n_verts > 0 && !verts)) return fail(SN_ERR_ARG, "null argument");
    return msmp_run(c, true, n_verts, verts, n_faces, faces, dst, cap_points, points, tri, n_points);
}
