// sn_meshorient.hip — C ABI of the mesh orientation stage (meshorient.h). The device form works on the caller's device
// arrays; the host form is the same computation on the host mirror's device copies of its arrays (sn_internal.h HostMirror). The edge table
// and the sequence around it are sn_meshedges.h's (MsmStage); everything after the build is plain launches on the context's stream, one read
// of the status block, then the kernel that writes the outputs.
#include "sn_meshedges.h"
#include "meshorient.h"

namespace {

// the caller's outputs: device arrays in the device form, host arrays in the host form
struct MorOut {
    int32_t *faces_out; unsigned char *face_flip; int32_t *face_component; unsigned char *face_keep;
    int32_t *comp_faces; unsigned char *comp_flags; unsigned long long *comp_vol6;
};

int mor_check(sn_ctx *c, const sn_mesh_orient_cfg *cfg, int n_verts, int n_faces, int nv, long long *counts)
{
    const int rc = mesh_check_counts(c, counts, 12);
    return rc != SN_OK ? rc : mor_check_args(cfg, n_verts, n_faces, nv);
}

// What both forms do once their arguments are checked.
int mor_run(sn_ctx *c, bool host, const sn_mesh_orient_cfg *cfg, int V, const double *verts, int F, int nv, const int32_t *faces, MorOut d,
            long long *counts)
{
    MsmStage s(c, host);
    const size_t n = (size_t)F;
    const double origin[3] = {0.0, 0.0, 0.0};
    MorArgs b;
    memset(&b, 0, sizeof b);
    b.sign = cfg->sign; b.min_faces = cfg->min_faces; b.keep_largest = cfg->keep_largest;
    // One giant piece is the common case: a workgroup whose faces name one piece sums in LDS and sends one set of atomics. The faster of the
    // two on an MI355X (tools/bench_meshorient.py, profiles/meshorient/); the test-only twin reads SN_MOR_NO_REDUCE to send per lane for the
    // A/B. The results are the same bits.
    b.reduce = sn_ab_switch("SN_MOR_NO_REDUCE") ? 0 : 1;
    int rc = s.build(c->mor_ws, V, verts, F, nv, faces, origin, 1.0, b.st, [&](Carve &w) {
        b.slot_lo = w.get<unsigned>(s.cap());
        b.slot_hi = w.get<unsigned>(s.cap());
        b.parent = w.get<unsigned>(2 * n);
        b.linked = w.get<unsigned>(n);
        b.root = w.get<unsigned>(n);
        b.rec_faces = w.get<unsigned>(n);
        b.rec_rel = w.get<unsigned>(n);
        b.rec_bits = w.get<unsigned>(n);
        b.rec_vol = w.get<unsigned long long>(3 * n);
        b.flags = w.get<unsigned char>(n);
    });
    if (rc != SN_OK || s.empty) return rc;                      // no face: all counts 0, nothing written
    const MsmEdges &a = s.e;
    HostMirror &m = s.m;
    const size_t cap = s.cap();
    const unsigned fb = blocks(F, MOR_NT), sb = blocks((long long)cap, MOR_NT), lb = loop_blocks(c);
    {
        // per side: its face's indices, a probe, the slot's count, two atomics
        ProfScope ps(c, "mor_sides", 0, (double)F * (nv * (4.0 + 4.0 + 16.0 + 4.0 + 8.0) + 8.0) + (double)cap * 8.0);
        HIPCHK(dev_fill(c, b.slot_lo, 0xff, cap));
        HIPCHK(dev_fill(c, b.slot_hi, 0, cap));
        LAUNCH(mor_sides_kernel, dim3(fb), dim3(MOR_NT), a, b);
    }
    {
        ProfScope ps(c, "mor_links", 0, (double)cap * 20.0 + (double)F * nv * 0.5 * (8.0 + 32.0) + (double)F * 4.0);
        HIPCHK(dev_fill(c, b.linked, 0, n));
        LAUNCH(mor_links_kernel, dim3(std::min(sb, lb)), dim3(MOR_NT), a, b);
    }
    {
        // per face: two walks to the root, its indices, its corners' records, the piece's record
        ProfScope ps(c, "mor_faces", 0, (double)F * (16.0 + 4.0 + nv * (4.0 + 4.0 + 24.0) + 8.0 + 36.0));
        HIPCHK(dev_fill(c, b.rec_faces, 0, n));
        HIPCHK(dev_fill(c, b.rec_rel, 0, n));
        HIPCHK(dev_fill(c, b.rec_bits, 0, n));
        HIPCHK(dev_fill(c, b.rec_vol, 0, 3 * n));
        LAUNCH(mor_faces_kernel, dim3(fb), dim3(MOR_NT), a, b);
    }
    {
        ProfScope ps(c, "mor_pieces", 0, (double)F * 8.0);
        LAUNCH(mor_pieces_kernel, dim3(std::min(fb, lb)), dim3(MOR_NT), a, b);
        LAUNCH(mor_keep_kernel, dim3(std::min(fb, lb)), dim3(MOR_NT), a, b);
    }
    // the one read, before any output is touched: the first bad face, the edge limit, the counts
    MorStat st;
    if ((rc = s.status(&st, b.st)) != SN_OK) return rc;
    rc = m.outputs([&](Carve &w) {
        m.out(w, d.faces_out, (size_t)nv * n); m.out(w, d.face_flip, n); m.out(w, d.face_component, n); m.out(w, d.face_keep, n);
        m.out(w, d.comp_faces, n); m.out(w, d.comp_flags, n); m.out(w, d.comp_vol6, 3 * n);
    });
    if (rc != SN_OK) return rc;
    b.faces_out = d.faces_out; b.face_flip = d.face_flip; b.face_component = d.face_component; b.face_keep = d.face_keep;
    b.comp_faces = d.comp_faces; b.comp_flags = d.comp_flags; b.comp_vol6 = d.comp_vol6;
    if (b.faces_out || b.face_flip || b.face_component || b.face_keep || b.comp_faces || b.comp_flags || b.comp_vol6) {
        ProfScope ps(c, "mor_emit", 0, (double)F * (8.0 + nv * 8.0 + 6.0 + 5.0 + 24.0));
        LAUNCH(mor_emit_kernel, dim3(fb), dim3(MOR_NT), a, b);
    }
    if ((rc = m.finish()) != SN_OK) return rc;
    for (int k = 0; k < 3; ++k) counts[k] = (long long)st.msm.counts[k];
    for (int k = 0; k < 9; ++k) counts[3 + k] = (long long)st.counts[k];
    return SN_OK;
}

}  // namespace

extern "C" int sn_mesh_orient_dev(sn_ctx *c, const sn_mesh_orient_cfg *cfg, int n_verts, const double *verts_dev, int n_faces, int nv,
                                  const int32_t *faces_dev, int32_t *faces_out_dev, unsigned char *face_flip_dev, int32_t *face_component_dev,
                                  unsigned char *face_keep_dev, int32_t *comp_faces_dev, unsigned char *comp_flags_dev,
                                  unsigned long long *comp_vol6_dev, long long *counts)
{
    int rc;
    if ((rc = mor_check(c, cfg, n_verts, n_faces, nv, counts)) != SN_OK) return rc;
    const MorOut o = {faces_out_dev, face_flip_dev, face_component_dev, face_keep_dev, comp_faces_dev, comp_flags_dev, comp_vol6_dev};
    return mor_run(c, false, cfg, n_verts, verts_dev, n_faces, nv, faces_dev, o, counts);
}

extern "C" int sn_mesh_orient(sn_ctx *c, const sn_mesh_orient_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv, const int32_t *faces,
                              int32_t *faces_out, unsigned char *face_flip, int32_t *face_component, unsigned char *face_keep, int32_t *comp_faces,
                              unsigned char *comp_flags, unsigned long long *comp_vol6, long long *counts)
{
    int rc;
    if ((rc = mor_check(c, cfg, n_verts, n_faces, nv, counts)) != SN_OK) return rc;
    const MorOut o = {faces_out, face_flip, face_component, face_keep, comp_faces, comp_flags, comp_vol6};
    return mor_run(c, true, cfg, n_verts, verts, n_faces, nv, faces, o, counts);
}
