// The paired null distance of one bin, sign(sum nd) * sum nd^2 over the states in numpy's float32 pairwise order: shared by
// k_pair_fused_s1 (epg_s2.hip) and k_null_dist_draws (epg_nulldraws.hip), so that the two give the same bits.
#pragma once
#include "epg_common.h"

namespace epg {

// d * d as numpy computes it -- rounded to float32 BEFORE it is added.  `__fmul_rn` + `__fadd_rn` are ordinary multiplies and adds to
// the optimiser (hipcc's default -ffp-contract=fast comes with the header they are inlined from, not with this function's pragma):
// in the loops unrolled for a compile-time S it fused them into v_fma_f32 and STEP 4's distance lost its last bit.  The empty asm is
// opaque: the product exists as a register value before anything can be added to it.
__device__ __forceinline__ float sq_nofma(float d) {
    float p = d * d;
    asm volatile("" : "+v"(p));
    return p;
}

// nd(s) = the difference of the two null groups' scores of state s.  numpy's order (k_pair_finish): a plain loop below eight
// elements, else eight partial sums over whole blocks of eight, their pairwise total, then the tail.
template <typename F>
__device__ __forceinline__ float null_dist_pairwise(int S, F&& nd) {
#pragma clang fp contract(off)   // numpy squares, rounds, then adds: no fused multiply-add anywhere in here
    float nsd, nsq;
    if (S < 8) {
        nsd = 0.f;
        nsq = 0.f;
        for (int s = 0; s < S; ++s) {
            const float d = nd(s);
            nsd += d;
            nsq += sq_nofma(d);
        }
    } else {
        float rd[8], rq[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float d = nd(k);
            rd[k] = d;
            rq[k] = sq_nofma(d);
        }
        int i = 8;
        for (; i < S - (S % 8); i += 8) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float d = nd(i + k);
                rd[k] += d;
                rq[k] += sq_nofma(d);
            }
        }
        nsd = ((rd[0] + rd[1]) + (rd[2] + rd[3])) + ((rd[4] + rd[5]) + (rd[6] + rd[7]));
        nsq = ((rq[0] + rq[1]) + (rq[2] + rq[3])) + ((rq[4] + rq[5]) + (rq[6] + rq[7]));
        for (; i < S; ++i) {
            const float d = nd(i);
            nsd += d;
            nsq += sq_nofma(d);
        }
    }
    const float nsg = nsd > 0.f ? 1.f : (nsd < 0.f ? -1.f : nsd);
    return nsq * nsg;
}

}  // namespace epg
