// meshorient.h — the orientation of a triangle or quad mesh: faces made to turn one way piece by piece, the sign of every piece, the pieces
// themselves with their face counts, closedness and exact volumes, and the removal of small pieces. DESIGN.md section 4.21 states the
// contract; tests/meshorient_ref.py restates it in numpy. The kernels run after the build of the edge table (meshedges.h: mark, quantise,
// edges, degree) on the table, its side counts and its quantised positions.
//   sides    per face: both nodes of its double cover become their own parents; every side with distinct ends finds its edge's slot
//            (lt_find) and, on a slot of two sides, sends its code (meshorient_rules.h) to the slot's two words with atomicMin / atomicMax
//   links    per slot (grid-stride): a slot of two sides of two different faces f < g is a link, r = its two direction bits are equal; the
//            two unions (2f, 2g + r), (2f + 1, 2g + 1 - r) of the double cover (unionfind.h), one more linked side for f and for g; a wave
//            counts its links and its inconsistent links in registers, a workgroup sends one atomic of each at its end
//   faces    per face: root(2f) and root(2f + 1) once - the piece, the face's bit against the piece's smallest face, non-orientable -, its
//            triple product on the quantised corners, then the piece's record: faces, reversed faces, the open and non-orientable bits, the
//            three limbs of s * t. When every face of the workgroup names one piece - the common case, one giant piece - the workgroup sums
//            in LDS and sends one set of atomics; otherwise every lane sends its own
//   pieces   per piece root (grid-stride): rule 6 and the piece's own verdict of rule 8, its volume negated when it turns, the packed
//            maximum that finds the largest piece; the counts as in links
//   keep     per piece root (grid-stride): the largest piece is kept as well; the kept pieces and their faces are counted
//   emit     (after the host has read the status block) per face: flip, copy, keep; row f of the per-piece arrays
// Everything that is summed is an integer: the same bits on every run, whatever the order of the atomics. No lane waits for another lane's
// progress: no flag to spin on, no lock, no cooperative launch, no grid barrier, no captured graph. The only data-dependent loops are
// lt_find's probe walk in a table at most half full, which ends at the side's own key (the build inserted it) or at a free slot, and cc_find /
// cc_union over the 2 F nodes of the double cover within the bounds unionfind.h states: links point to smaller nodes, so a chain has at most
// 2 F steps, and a failed CAS means another lane linked that root, which happens at most 2 F times in all.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blocksum.h"
#include "meshedges.h"
#include "meshnormals.h"
#include "meshorient_rules.h"
#include "unionfind.h"

namespace sn {

constexpr int MOR_NT = 256;
constexpr unsigned MOR_R_OPEN = 1, MOR_R_NONOR = 2;             // bits of a piece's record while it is summed

// What the host reads once, after the keep kernel and before any output is touched: 136 bytes.
struct MorStat {
    MsmStat msm;                        // the build's: the first bad face, the edge counts
    unsigned long long largest;         // max over the pieces of mor_pack_largest(n_faces, id)
    unsigned long long counts[9];       // links, inconsistent links, pieces, non-orientable, closed, flipped faces, flipped pieces, kept faces, kept pieces
};

struct MorArgs {
    int sign, min_faces, keep_largest, reduce;
    // work
    MorStat *st;
    unsigned *slot_lo, *slot_hi;        // [mask + 1] the smallest and the largest side code on a slot of two sides (preset ~0 and 0)
    unsigned *parent;                   // [2 F] the double cover's union-find
    unsigned *linked;                   // [F] sides of the face that lie on a link
    unsigned *root;                     // [F] root(2f)
    unsigned *rec_faces, *rec_rel, *rec_bits;      // [F] at a piece's id: its faces, its reversed faces, MOR_R_*
    unsigned long long *rec_vol;        // [F][3] ... the limbs of its volume
    unsigned char *flags;               // [F] ... its comp_flags
    // outputs (each optional)
    int32_t *faces_out; unsigned char *face_flip; int32_t *face_component; unsigned char *face_keep;
    int32_t *comp_faces; unsigned char *comp_flags; unsigned long long *comp_vol6;
};

// the corners of face f, or false: a face the build refused (an index outside [0, V), a referenced coordinate out of range)
__device__ __forceinline__ bool mor_corners(const MsmEdges &a, long long f, int idx[4])
{
    bool ok = true;
    for (int k = 0; k < a.nv; ++k) {
        idx[k] = a.faces[(size_t)a.nv * f + k];
        if (!mesh_index_ok(idx[k], a.V)) ok = false;
    }
    if (ok)
        for (int k = 0; k < a.nv; ++k)
            if (a.vfl[idx[k]] & MSM_BAD) ok = false;
    return ok;
}

static __global__ void __launch_bounds__(MOR_NT) mor_sides_kernel(MsmEdges a, MorArgs b)
{
    const long long f = (long long)blockIdx.x * MOR_NT + threadIdx.x;
    if (f >= a.F) return;
    cc_st(b.parent + 2 * (size_t)f, 2u * (unsigned)f);
    cc_st(b.parent + 2 * (size_t)f + 1, 2u * (unsigned)f + 1u);
    int idx[4];
    if (!mor_corners(a, f, idx)) return;                        // (the build reported it: its sides are not in the table)
    for (int k = 0; k < a.nv; ++k) {
        const unsigned p = (unsigned)idx[k], r = (unsigned)idx[k + 1 == a.nv ? 0 : k + 1];
        if (p == r) continue;                                   // rule 1: no side
        const unsigned lo = p < r ? p : r, hi = p < r ? r : p;
        const int h = lt_find<LtPairs>(a.tab, a.mask, ((unsigned long long)lo << MSM_INDEX_BITS) | hi);
        if (h < 0 || a.sides[h] != 2u) continue;
        const unsigned code = mor_side_code((unsigned)f, p, r);
        atomicMin(b.slot_lo + h, code);
        atomicMax(b.slot_hi + h, code);
    }
}

// Grid-stride over the slots, the bound the same for a whole wave: the ballots count for all of it.
static __global__ void __launch_bounds__(MOR_NT) mor_links_kernel(MsmEdges a, MorArgs b)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * MOR_NT;
    const unsigned lane = threadIdx.x & 63;
    unsigned long long links = 0, bad = 0;
    for (unsigned long long h = (unsigned long long)blockIdx.x * MOR_NT + threadIdx.x; h - lane <= a.mask; h += stride) {
        unsigned lo = 0, hi = 0, n = 0;
        bool link = msm_slot(a, h, lo, hi, n) && n == 2u;
        unsigned r = 0;
        if (link) {
            lo = b.slot_lo[h]; hi = b.slot_hi[h];
            link = lo < hi && mor_is_link(lo, hi);              // (lo > hi: the presets, no side wrote)
        }
        if (link) {
            const unsigned f = lo >> 1, g = hi >> 1;            // f < g: the codes are ordered as their faces are
            r = mor_inconsistent(lo, hi);
            cc_union(b.parent, 2u * f, 2u * g + r);
            cc_union(b.parent, 2u * f + 1u, 2u * g + 1u - r);
            atomicAdd(b.linked + f, 1u);
            atomicAdd(b.linked + g, 1u);
        }
        links += (unsigned long long)__popcll(__ballot(link));
        bad += (unsigned long long)__popcll(__ballot(link && r));
    }
    const unsigned long long sums[2] = {links, bad};
    block_add<MOR_NT>(&b.st->counts[0], sums);
}

// One face per lane. red: per lane the three limbs, the reversed faces, the record bits and the faces of the workgroup's tree.
static __global__ void __launch_bounds__(MOR_NT) mor_faces_kernel(MsmEdges a, MorArgs b)
{
    __shared__ unsigned long long red[MOR_NT][6];
    __shared__ unsigned first, differ;
    const int t = threadIdx.x;
    const long long f = (long long)blockIdx.x * MOR_NT + t;
    const bool live = f < a.F;
    unsigned c = 0, rel = 0, bits = 0;
    MnrLimbs vol = {{0, 0, 0}};
    if (live) {
        const unsigned r0 = cc_find(b.parent, 2u * (unsigned)f), r1 = cc_find(b.parent, 2u * (unsigned)f + 1u);
        b.root[f] = r0;
        c = r0 >> 1;
        rel = r0 & 1u;
        bits = (r0 == r1 ? MOR_R_NONOR : 0u) | (b.linked[f] != (unsigned)a.nv ? MOR_R_OPEN : 0u);
        int idx[4];
        if (mor_corners(a, f, idx)) {
            long long q[4][3];
            for (int k = 0; k < a.nv; ++k) msm_load(a.pos, (size_t)idx[k], q[k]);
            mnr_i128 six = mnr_triple(q[0], q[1], q[2]);
            if (a.nv == 4) six += mnr_triple(q[0], q[2], q[3]);
            vol = mnr_limbs_of(rel ? -six : six);               // rule 5: s = -1 iff rel
        }
    }
    if (t == 0) { first = c; differ = 0; }                      // (lane 0 of a launched workgroup is a face)
    __syncthreads();
    if (live && c != first) differ = 1;                         // every writer stores the same value
    __syncthreads();
    if (differ || !b.reduce) {                                  // the same for the whole workgroup
        if (!live) return;
        atomicAdd(b.rec_faces + c, 1u);
        if (rel) atomicAdd(b.rec_rel + c, 1u);
        if (bits) atomicOr(b.rec_bits + c, bits);
        mnr_atomic_add_limbs(b.rec_vol + 3 * (size_t)c, vol);
        return;
    }
    // one piece: a tree in LDS, limb sums with carry
    unsigned long long n_rel = rel, n_faces = live ? 1 : 0, all = bits;
    for (int k = 0; k < 3; ++k) red[t][k] = vol.w[k];
    red[t][3] = n_rel; red[t][4] = all; red[t][5] = n_faces;
    __syncthreads();
    for (int h = MOR_NT / 2; h > 0; h >>= 1) {
        if (t < h) {
            MnrLimbs other;
            for (int k = 0; k < 3; ++k) other.w[k] = red[t + h][k];
            mnr_limbs_add(vol, other);
            n_rel += red[t + h][3]; all |= red[t + h][4]; n_faces += red[t + h][5];
            for (int k = 0; k < 3; ++k) red[t][k] = vol.w[k];
            red[t][3] = n_rel; red[t][4] = all; red[t][5] = n_faces;
        }
        __syncthreads();
    }
    if (t == 0) {
        atomicAdd(b.rec_faces + c, (unsigned)n_faces);
        if (n_rel) atomicAdd(b.rec_rel + c, (unsigned)n_rel);
        if (all) atomicOr(b.rec_bits + c, (unsigned)all);
        mnr_atomic_add_limbs(b.rec_vol + 3 * (size_t)c, vol);
    }
}

// Grid-stride over the face indices, a piece's id among them: root(2c) = 2c. After the faces kernel a piece's record is its root's own.
static __global__ void __launch_bounds__(MOR_NT) mor_pieces_kernel(MsmEdges a, MorArgs b)
{
    const long long stride = (long long)gridDim.x * MOR_NT;
    const int lane = threadIdx.x & 63;
    unsigned long long pieces = 0, nonor = 0, closed = 0, turned = 0, turned_faces = 0;
    for (long long c = (long long)blockIdx.x * MOR_NT + threadIdx.x; c - lane < a.F; c += stride) {
        const bool piece = c < a.F && b.root[c] == 2u * (unsigned)c;
        bool orientable = false, shut = false, flipc = false;
        if (piece) {
            const unsigned bits = b.rec_bits[c], n_faces = b.rec_faces[c], n_rel = b.rec_rel[c];
            orientable = !(bits & MOR_R_NONOR);
            shut = orientable && !(bits & MOR_R_OPEN);
            MnrLimbs vol;
            for (int k = 0; k < 3; ++k) vol.w[k] = b.rec_vol[3 * (size_t)c + k];
            flipc = mor_flipc(b.sign, orientable, shut, n_faces, n_rel, vol);
            if (flipc) {
                vol = mor_limbs_neg(vol);
                for (int k = 0; k < 3; ++k) b.rec_vol[3 * (size_t)c + k] = vol.w[k];
                turned_faces += n_faces - n_rel;
            } else turned_faces += n_rel;
            b.flags[c] = (unsigned char)((orientable ? MOR_ORIENTABLE : 0u) | (shut ? MOR_CLOSED : 0u) | (flipc ? MOR_FLIPPED : 0u) |
                                         (mor_kept(n_faces, b.min_faces) ? MOR_KEPT : 0u));
            if (b.keep_largest) atomicMax(&b.st->largest, mor_pack_largest(n_faces, (unsigned)c));
        }
        pieces += (unsigned long long)__popcll(__ballot(piece));
        nonor += (unsigned long long)__popcll(__ballot(piece && !orientable));
        closed += (unsigned long long)__popcll(__ballot(shut));
        turned += (unsigned long long)__popcll(__ballot(flipc));
    }
    const unsigned long long sums[5] = {pieces, nonor, closed, wave_sum(turned_faces), turned};
    block_add<MOR_NT>(&b.st->counts[2], sums);
}

static __global__ void __launch_bounds__(MOR_NT) mor_keep_kernel(MsmEdges a, MorArgs b)
{
    const long long stride = (long long)gridDim.x * MOR_NT;
    const int lane = threadIdx.x & 63;
    const unsigned long long largest = b.st->largest;           // (the pieces kernel is done)
    unsigned long long kept = 0, kept_faces = 0;
    for (long long c = (long long)blockIdx.x * MOR_NT + threadIdx.x; c - lane < a.F; c += stride) {
        bool keep = false;
        if (c < a.F && b.root[c] == 2u * (unsigned)c) {
            unsigned fl = b.flags[c];
            if (b.keep_largest && mor_largest_id(largest) == (unsigned)c) b.flags[c] = (unsigned char)(fl |= MOR_KEPT);
            keep = (fl & MOR_KEPT) != 0;
            if (keep) kept_faces += b.rec_faces[c];
        }
        kept += (unsigned long long)__popcll(__ballot(keep));
    }
    const unsigned long long sums[2] = {wave_sum(kept_faces), kept};
    block_add<MOR_NT>(&b.st->counts[7], sums);
}

static __global__ void __launch_bounds__(MOR_NT) mor_emit_kernel(MsmEdges a, MorArgs b)
{
    const long long f = (long long)blockIdx.x * MOR_NT + threadIdx.x;
    if (f >= a.F) return;
    const unsigned r0 = b.root[f], c = r0 >> 1;
    const unsigned fl = b.flags[c];
    const unsigned flip = (r0 & 1u) ^ ((fl & MOR_FLIPPED) ? 1u : 0u);      // rule 6 (a non-orientable piece: both are 0)
    if (b.faces_out)
        for (int k = 0; k < a.nv; ++k) b.faces_out[(size_t)a.nv * f + k] = a.faces[(size_t)a.nv * f + (flip ? mor_flipped_corner(k, a.nv) : k)];
    if (b.face_flip) b.face_flip[f] = (unsigned char)flip;
    if (b.face_component) b.face_component[f] = (int32_t)c;
    if (b.face_keep) b.face_keep[f] = (fl & MOR_KEPT) ? 1 : 0;
    const bool piece = c == (unsigned)f;                        // row f of the per-piece arrays: zero where f is no piece's id
    if (b.comp_faces) b.comp_faces[f] = piece ? (int32_t)b.rec_faces[f] : 0;
    if (b.comp_flags) b.comp_flags[f] = piece ? (unsigned char)fl : 0;
    if (b.comp_vol6)
        for (int k = 0; k < 3; ++k) b.comp_vol6[3 * (size_t)f + k] = piece ? b.rec_vol[3 * (size_t)f + k] : 0ull;
}

}  // namespace sn
