// meshorient_rules.h — the rules of the mesh orientation stage that host and device share: the code of a side and the
// relation of the two sides of a link (rules 1, 2), the corner a flipped face reads (rule 7), the sign and the negation of a three-limb sum,
// the sign of a piece (rule 6), its verdict and the packed word that finds the largest piece (rule 8). The device code (meshorient.h) and the
// CPU check (tests/host/meshorient_check.cpp) read the same lines. Plain C++17 with no hip/ include.
#pragma once
#include <stdint.h>

#include "meshnormals_sum.h"

namespace sn {

constexpr unsigned MOR_ORIENTABLE = 1, MOR_CLOSED = 2, MOR_FLIPPED = 4, MOR_KEPT = 8;      // comp_flags

// rule 1: the code of side p -> r of a face, p != r: 2 * face + (p < r); face < 2^28, so a code is below 2^29
MSM_HD inline unsigned mor_side_code(unsigned face, unsigned p, unsigned r) { return 2u * face + (p < r ? 1u : 0u); }

// rule 2, of the two codes of an edge with exactly two sides: a link joins two different faces; it is inconsistent iff the two direction bits
// are equal (two consistently oriented neighbours cross their common edge in opposite directions)
MSM_HD inline bool mor_is_link(unsigned lo, unsigned hi) { return (lo >> 1) != (hi >> 1); }
MSM_HD inline unsigned mor_inconsistent(unsigned lo, unsigned hi) { return ((lo ^ hi) & 1u) ^ 1u; }

// rule 7: corner k of a flipped face of nv corners is corner mor_flipped_corner(k, nv) of the face as given: (a,b,c) -> (a,c,b),
// (a,b,c,d) -> (a,d,c,b)
MSM_HD inline int mor_flipped_corner(int k, int nv) { return k == 0 ? 0 : nv - k; }

// -1, 0, 1: the sign of a two's-complement three-limb sum
MSM_HD inline int mor_limbs_sign(const MnrLimbs &s)
{
    if (s.w[2] >> 63) return -1;
    return (s.w[0] | s.w[1] | s.w[2]) ? 1 : 0;
}

// -s modulo 2^192: the complement plus one, the carry walking up
MSM_HD inline MnrLimbs mor_limbs_neg(const MnrLimbs &s)
{
    MnrLimbs r;
    unsigned long long carry = 1;
    for (int k = 0; k < 3; ++k) {
        r.w[k] = ~s.w[k] + carry;
        carry = (carry && r.w[k] == 0) ? 1 : 0;
    }
    return r;
}

// rule 6: does an orientable piece of n_faces faces, n_rel of them reversed against its smallest face, turn? sign 0: the fewer faces turn,
// a tie leaves the smallest face as it is; sign 1: a closed piece with a volume turns iff that is negative, every other piece as sign 0.
// A non-orientable piece never turns.
MSM_HD inline bool mor_flipc(int sign, bool orientable, bool closed, long long n_faces, long long n_rel, const MnrLimbs &vol)
{
    if (!orientable) return false;
    const int s = mor_limbs_sign(vol);
    if (sign == 1 && closed && s != 0) return s < 0;
    return n_rel > n_faces - n_rel;
}

// rule 8: a piece's own verdict ...
MSM_HD inline bool mor_kept(long long n_faces, int min_faces) { return n_faces >= (long long)min_faces; }

// ... and the word whose maximum names the piece with the most faces, the smallest id among equals: faces above, the id's complement below
MSM_HD inline unsigned long long mor_pack_largest(unsigned n_faces, unsigned id) { return ((unsigned long long)n_faces << 32) | (0xffffffffu - id); }
MSM_HD inline unsigned mor_largest_id(unsigned long long packed) { return 0xffffffffu - (unsigned)packed; }

}  // namespace sn
