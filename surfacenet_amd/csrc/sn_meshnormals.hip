// sn_meshnormals.hip — C ABI of the mesh's own normals, area and volume (meshnormals.h). The device form works on the
// caller's device arrays; the host form is the same computation on the host mirror's device copies of its arrays (sn_internal.h HostMirror).
// Two plain launches on the context's stream, one read of the status block, then the normals leave the workspace.
#include "sn_internal.h"
#include "meshnormals.h"

namespace {

int mnr_check(sn_ctx *c, int n_verts, int n_faces, int nv, long long *counts, unsigned long long *sums)
{
    const int rc = mesh_check_counts(c, counts, 4);
    if (rc != SN_OK) return rc;
    if (!sums) return fail(SN_ERR_ARG, "sums is required");
    std::fill(sums, sums + 6, 0ull);
    return mnr_check_args(n_verts, n_faces, nv);
}

// What both forms do once their arguments are checked, F > 0.
int mnr_run(sn_ctx *c, bool host, int V, const double *verts, int F, int nv, const int32_t *faces, float *face_normals, float *vert_normals,
            long long *counts, unsigned long long *sums)
{
    HostMirror m(c, host);
    int rc = m.inputs([&](Carve &w) { m.in(w, verts, 3 * (size_t)V); m.in(w, faces, (size_t)nv * (size_t)F); });
    if (rc != SN_OK) return rc;
    MnrArgs a;
    memset(&a, 0, sizeof a);
    a.verts = verts; a.faces = faces; a.V = V; a.F = F; a.nv = nv;
    auto layout = [&](Carve &w) {
        a.st = w.get<MnrStat>(1);
        a.ref = w.get<unsigned char>((size_t)V);
        a.acc = w.get<unsigned long long>(6 * (size_t)V);
        a.fn = w.get<float>(3 * (size_t)F);
        a.vn = w.get<float>(3 * (size_t)V);
    };
    if ((rc = dev_carve(c, c->mnr_ws, layout, 256)) != SN_OK) return rc;
    HIPCHK(dev_fill(c, a.st, 0, 1));
    HIPCHK(dev_fill(c, &a.st->first_bad, 0xff, 1));      // MESH_NO_BAD
    {
        // per face: its indices, its corners' coordinates, its normal; per corner and axis up to two atomics on 16 bytes
        ProfScope ps(c, "mnr_faces", 0, (double)F * (nv * (4.0 + 24.0 + 48.0) + 12.0) + (double)V * 49.0);
        HIPCHK(dev_fill(c, a.ref, 0, std::max<size_t>((size_t)V, 1)));
        HIPCHK(dev_fill(c, a.acc, 0, 6 * std::max<size_t>((size_t)V, 1)));
        LAUNCH(mnr_faces_kernel, dim3(std::min(blocks(F, MNR_NT), loop_blocks(c))), dim3(MNR_NT), a);
    }
    if (V > 0) {
        ProfScope ps(c, "mnr_verts", 0, (double)V * (1.0 + 48.0 + 12.0));
        LAUNCH(mnr_verts_kernel, dim3(std::min(blocks(V, MNR_NT), loop_blocks(c))), dim3(MNR_NT), a);
    }
    // the one read, before any output is touched: the first bad face, the counts, the sums
    MnrStat st;
    HIPCHK(read_status(c, &st, a.st));
    if ((rc = mesh_report_bad(st.first_bad, V)) != SN_OK) return rc;
    rc = m.outputs([&](Carve &w) { m.out(w, face_normals, 3 * (size_t)F); m.out(w, vert_normals, 3 * (size_t)V); });
    if (rc != SN_OK) return rc;
    if (face_normals) HIPCHK(hipMemcpyAsync(face_normals, a.fn, sizeof(float) * 3 * (size_t)F, hipMemcpyDeviceToDevice, c->stream));
    if (vert_normals && V > 0)
        HIPCHK(hipMemcpyAsync(vert_normals, a.vn, sizeof(float) * 3 * (size_t)V, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = m.finish()) != SN_OK) return rc;
    for (int k = 0; k < 3; ++k) counts[k] = (long long)st.counts[k];
    counts[3] = (long long)F * (nv - 2);
    for (int k = 0; k < 6; ++k) sums[k] = st.sums[k];
    return SN_OK;
}

int mnr_dispatch(sn_ctx *c, bool host, int V, const double *verts, int F, int nv, const int32_t *faces, float *face_normals, float *vert_normals,
                 long long *counts, unsigned long long *sums)
{
    if (F > 0 && (!faces || (V > 0 && !verts))) return fail(SN_ERR_ARG, "null argument");
    if (F == 0) {                                               // nothing is referenced: zero rows, zero counts and sums
        if (V == 0 || !vert_normals) return SN_OK;
        const size_t bytes = sizeof(float) * 3 * (size_t)V;
        if (host) {
            memset(vert_normals, 0, bytes);
            return SN_OK;
        }
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipMemsetAsync(vert_normals, 0, bytes, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return SN_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    return mnr_run(c, host, V, verts, F, nv, faces, face_normals, vert_normals, counts, sums);
}

}  // namespace

extern "C" int sn_mesh_normals_dev(sn_ctx *c, int n_verts, const double *verts_dev, int n_faces, int nv, const int32_t *faces_dev,
                                   float *face_normals_dev, float *vert_normals_dev, long long *counts, unsigned long long *sums)
{
    int rc;
    if ((rc = mnr_check(c, n_verts, n_faces, nv, counts, sums)) != SN_OK) return rc;
    return mnr_dispatch(c, false, n_verts, verts_dev, n_faces, nv, faces_dev, face_normals_dev, vert_normals_dev, counts, sums);
}

extern "C" int sn_mesh_normals(sn_ctx *c, int n_verts, const double *verts, int n_faces, int nv, const int32_t *faces, float *face_normals,
                               float *vert_normals, long long *counts, unsigned long long *sums)
{
    int rc;
    if ((rc = mnr_check(c, n_verts, n_faces, nv, counts, sums)) != SN_OK) return rc;
    return mnr_dispatch(c, true, n_verts, verts, n_faces, nv, faces, face_normals, vert_normals, counts, sums);
}
