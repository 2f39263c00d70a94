// The pieces every radix select of the trims (pcp.h I3, I3b, I5b) is built from, written once: the
// digits of the most-significant-digit-first select over a key's high word, the wave's count of one
// key into an LDS histogram, the rank of the wanted order statistic and the cut derived from it.
// icp_trim.hip (one select over all keys, global histograms) and icp_batch_trim.hip (one select per
// segment, one workgroup each, the state in LDS) compile this text, so "the same selection" and
// "the same cut" are the same code.
#pragma once
#include "icp_pair.hpp"

namespace pcp {

constexpr int kPeel = 4;
constexpr int kTBins = 2048;  // bins of the widest digit

// digits of 11 / 11 / 10 bits, most significant first
__host__ __device__ constexpr int digit_bits(int p) { return p == 2 ? 10 : 11; }
__host__ __device__ constexpr int digit_shift(int p) { return p == 0 ? 21 : p == 1 ? 10 : 0; }

// Count one key's digit of pass P into the block's LDS histogram h (called by whole waves: every
// lane of the wave reaches it, a lane without a key passes kNoKey).  A key counts when it is not
// kNoKey and, after the first pass, its higher digits equal prefix.
//
// ICP distances sit in a handful of exponents, so in the leading digit almost every lane of a wave
// lands in the same few bins, and 64 same-address LDS atomics serialise.  Each wave therefore peels
// up to kPeel groups first: the lanes that share the first active lane's digit are counted with a
// ballot and added by one lane.  What is still active after kPeel rounds (digits spread over many
// bins, where collisions are rare) adds one by one.
template <int P>
__device__ __forceinline__ void count_digit(uint32_t* h, uint64_t key, uint32_t prefix) {
    constexpr int shift = digit_shift(P), bits = digit_bits(P);
    const uint32_t b = key_d2_bits(key);
    bool act = key != kNoKey;
    if constexpr (P > 0) act = act && (b >> (shift + bits)) == prefix;
    const uint32_t d = (b >> shift) & ((1u << bits) - 1u);
    const int lane = threadIdx.x & 63;
    uint64_t todo = __ballot(act);
#pragma unroll
    for (int r = 0; r < kPeel; r++) {
        if (todo == 0) break;  // wave-uniform
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t dl = (uint32_t)__builtin_amdgcn_readlane((int)d, leader);
        const bool mine = act && d == dl;
        const uint64_t same = __ballot(mine);
        if (lane == leader) atomicAdd(&h[dl], (uint32_t)__popcll(same));
        if (mine) act = false;
        todo &= ~same;
    }
    if (act) atomicAdd(&h[d], 1u);
}

// the contract's r for m valid keys (0 when there is none): fp64 on the device
__device__ __forceinline__ uint64_t trim_rank(float frac, uint64_t m) {
    return m ? (uint64_t)floor((double)frac * (double)(m - 1)) : 0;
}

// the bits of the contract's cut for the selected pattern: fp32 steps, f2 when c is NaN
__device__ __forceinline__ uint32_t trim_cut_bits(uint32_t sel, float mult, float d_floor) {
    const float m2 = mult * mult;
    const float cc = m2 * __uint_as_float(sel);
    const float f2 = d_floor * d_floor;
    const float cut = (cc > f2) ? cc : f2;  // f2 when cc is NaN
    return __float_as_uint(cut);
}

}  // namespace pcp
