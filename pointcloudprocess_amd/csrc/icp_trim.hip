// Trimmed correspondences (include/pcp.h, I3): an exact order statistic of the d2 words of the
// pcp_icp_keys_dev keys, and a filter that rewrites the keys above the cut derived from it to
// INT64_MAX, the "no pair" key every accumulator already skips.
//
// The selection is a most-significant-digit-first radix select on the high word b = key >> 32,
// digits of 11 / 11 / 10 bits: three histogram passes over the keys (per-block LDS histograms
// merged into one global histogram with integer atomics) and, after each, one block that finds
// the digit holding the wanted rank and the rank left inside it.  The filter is the fourth and
// last read.  Everything is integer counting, so the result is the same bit for bit on every run.
//
// Same-address LDS atomics of a wave are peeled by count_digit (icp_trim.hpp), which the per-segment
// select of icp_batch_trim.hip shares with the rank and the cut.
//
// Owned here: the select and the one filter kernel, for both trims: the point trim ranks the keys
// themselves, the trim by plane residual (icp_plane.hip) ranks its residual keys and filters the
// caller's keys by them.  The key's layout and the block count are icp_pair.hpp's.
#include <algorithm>
#include <cmath>

#include "icp_trim.hpp"

namespace pcp {
namespace {

constexpr int kTB = kPairBlock;
constexpr int kTPer = 4;             // keys per thread and block iteration of the histogram passes
constexpr int kTHistBlocks = 1024;   // grid cap of the histogram passes (4 blocks of 8 KB LDS per CU)
constexpr int kTFilterBlocks = 2048; // grid cap of the filter

// work memory: hist[3][kTBins] u32, then the state between the passes
struct TrimState {
    uint64_t rank;    // rank left inside the bins chosen so far
    uint64_t m;       // valid keys
    uint32_t prefix;  // the digits chosen so far, most significant first
    uint32_t pad;
};
constexpr size_t kStateWord = 3 * (size_t)kTBins;  // u32 offset of the state (8-byte aligned)

__device__ __forceinline__ TrimState* state_of(uint32_t* work) { return (TrimState*)(work + kStateWord); }

// pass P: histogram of digit P over the valid keys whose higher digits equal the state's prefix
template <int P>
__global__ void __launch_bounds__(kTB) k_trim_hist(const uint64_t* keys, int64_t n, uint32_t* work) {
    constexpr int nb = 1 << digit_bits(P);
    __shared__ uint32_t h[nb];
    for (int b = threadIdx.x; b < nb; b += kTB) h[b] = 0;
    const uint32_t prefix = P > 0 ? state_of(work)->prefix : 0u;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kTB;
    // the trip count is the same for every thread of the block, so the ballots see whole waves
    for (int64_t base = (int64_t)blockIdx.x * kTB; base < n; base += kTPer * stride) {
        uint64_t k[kTPer];
#pragma unroll
        for (int u = 0; u < kTPer; u++) {
            const int64_t i = base + u * stride + threadIdx.x;
            k[u] = i < n ? keys[i] : kNoKey;
        }
#pragma unroll
        for (int u = 0; u < kTPer; u++) count_digit<P>(h, k[u], prefix);
    }
    __syncthreads();
    uint32_t* g = work + (size_t)P * kTBins;
    for (int b = threadIdx.x; b < nb; b += kTB) {
        const uint32_t c = h[b];
        if (c) atomicAdd(&g[b], c);
    }
}

// one block after pass P: the bin holding the rank, the rank left inside it; after the last pass
// the cut and the stats (kept = 0, the filter adds to it)
template <int P>
__global__ void __launch_bounds__(kTB) k_trim_pick(uint32_t* work, float frac, float mult, float d_floor,
                                                   uint64_t* trim) {
    constexpr int bits = digit_bits(P), nb = 1 << bits, per = nb / kTB;
    __shared__ uint32_t part[kTB];
    __shared__ uint64_t rank_s, left_s;
    __shared__ uint32_t old_s, pre_s;
    const int tid = threadIdx.x;
    const uint32_t* g = work + (size_t)P * kTBins;
    TrimState* st = state_of(work);
    uint32_t c[per], s = 0;
#pragma unroll
    for (int j = 0; j < per; j++) {
        c[j] = g[tid * per + j];
        s += c[j];  // a bin, and their total m, is < 2^31
    }
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < kTB; o <<= 1) {
        const uint32_t v = tid >= o ? part[tid - o] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    if (tid == 0) {
        uint64_t rank;
        if (P == 0) {
            const uint64_t m = part[kTB - 1];
            st->m = m;
            rank = trim_rank(frac, m);
            old_s = 0;
        } else {
            rank = st->rank;
            old_s = st->prefix;
        }
        rank_s = left_s = rank;
        pre_s = old_s << bits;  // m == 0: no bin holds the rank and sel stays 0
    }
    __syncthreads();
    const uint64_t rank = rank_s, excl = part[tid] - s;
    if (rank >= excl && rank < excl + s) {  // one thread at most
        uint64_t cum = excl;
#pragma unroll
        for (int j = 0; j < per; j++) {
            if (rank < cum + c[j]) {
                pre_s = (old_s << bits) | (uint32_t)(tid * per + j);
                left_s = rank - cum;
                break;
            }
            cum += c[j];
        }
    }
    __syncthreads();
    if (tid == 0) {
        st->prefix = pre_s;
        st->rank = left_s;
        if (P == 2) {
            const uint32_t sel = pre_s;
            trim[0] = st->m;
            trim[1] = 0;
            trim[2] = sel;
            trim[3] = trim_cut_bits(sel, mult, d_floor);
        }
    }
}

__global__ void k_trim_empty(float d_floor, uint64_t* trim) {
    trim[0] = trim[1] = trim[2] = 0;
    trim[3] = __float_as_uint(d_floor * d_floor);
}

// The filter: pair i is kept iff its ranked key is valid and as_float(its high word) <= cut; the
// kept count is added to trim[1].  RES = false ranks the keys themselves (pcp.h I3); in place only
// the rejected valid keys are stored.  RES = true ranks the residual keys rkeys of icp_plane.hip's
// k_res_keys (I3b) and applies the result to the caller's keys: a kept key is the caller's, all 64
// bits, and in place every key not kept is stored, since a pair without a usable plane record is
// still a pair in keys.
template <bool RES>
__global__ void __launch_bounds__(kTB) k_trim_filter(const uint64_t* keys, const uint64_t* rkeys, int64_t n,
                                                     uint64_t* out, int inplace, uint64_t* trim) {
    const float cut = __uint_as_float((uint32_t)trim[3]);
    uint32_t cnt = 0;
    for (int64_t i = blockIdx.x * (int64_t)kTB + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTB) {
        const uint64_t rk = RES ? rkeys[i] : keys[i];
        const bool valid = rk != kNoKey;
        const bool keep = valid && key_d2(rk) <= cut;
        cnt += keep ? 1u : 0u;
        if (inplace) {
            if (RES ? !keep : valid && !keep) out[i] = kNoKey;
        } else {
            out[i] = keep ? (RES ? keys[i] : rk) : kNoKey;
        }
    }
    const uint32_t t = block_count(cnt);
    if (threadIdx.x == 0 && t) atomicAdd((unsigned long long*)&trim[1], (unsigned long long)t);
}

template <int P>
void launch_pass(pcp_ctx* ctx, const uint64_t* keys, int64_t n, float frac, float mult, float d_floor,
                 uint64_t* trim, uint32_t* work) {
    const unsigned nb = grid_for(n, kTB * kTPer, kTHistBlocks);
    hipLaunchKernelGGL(k_trim_hist<P>, dim3(nb), dim3(kTB), 0, ctx->stream, keys, n, work);
    hipLaunchKernelGGL(k_trim_pick<P>, dim3(1), dim3(kTB), 0, ctx->stream, work, frac, mult, d_floor, trim);
}

}  // namespace

size_t trim_work_bytes() { return kStateWord * sizeof(uint32_t) + sizeof(TrimState); }

bool trim_args_ok(float frac, float mult, float d_floor) {
    return frac >= 0.f && frac <= 1.f && mult >= 0.f && std::isfinite(mult) && d_floor >= 0.f &&
           std::isfinite(d_floor);
}

int trim_select_async(pcp_ctx* ctx, const uint64_t* keys, int64_t n, float frac, float mult, float d_floor,
                      uint64_t* trim, uint32_t* work) {
    if (n == 0) {
        hipLaunchKernelGGL(k_trim_empty, dim3(1), dim3(1), 0, ctx->stream, d_floor, trim);
        PCP_LAUNCH_CHECK(ctx);
        return PCP_OK;
    }
    PCP_HIP(ctx, hipMemsetAsync(work, 0, trim_work_bytes(), ctx->stream));
    launch_pass<0>(ctx, keys, n, frac, mult, d_floor, trim, work);
    launch_pass<1>(ctx, keys, n, frac, mult, d_floor, trim, work);
    launch_pass<2>(ctx, keys, n, frac, mult, d_floor, trim, work);
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

int trim_filter_async(pcp_ctx* ctx, const uint64_t* keys, const uint64_t* rkeys, int64_t n, uint64_t* out,
                      uint64_t* trim) {
    if (n == 0) return PCP_OK;
    const dim3 grid(grid_for(n, kTB, kTFilterBlocks));
    const int inplace = out == keys ? 1 : 0;
    if (rkeys)
        hipLaunchKernelGGL(k_trim_filter<true>, grid, dim3(kTB), 0, ctx->stream, keys, rkeys, n, out, inplace, trim);
    else
        hipLaunchKernelGGL(k_trim_filter<false>, grid, dim3(kTB), 0, ctx->stream, keys, rkeys, n, out, inplace, trim);
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

int trim_keys_async(pcp_ctx* ctx, const uint64_t* keys, int64_t n, float frac, float mult, float d_floor,
                    uint64_t* out, uint64_t* trim, uint32_t* work) {
    PCP_TRY(trim_select_async(ctx, keys, n, frac, mult, d_floor, trim, work));
    return trim_filter_async(ctx, keys, nullptr, n, out, trim);
}

}  // namespace pcp

using namespace pcp;

extern "C" {

// the argument checks read nothing through ctx: a rejected call never touches the context
int pcp_icp_trim_keys(pcp_ctx* ctx, const uint64_t* keys_dev, int64_t n, float frac, float mult, float d_floor,
                      uint64_t* keys_out_dev, uint64_t* trim_dev) {
    if (!ctx || !trim_dev || n < 0 || n >= (int64_t)1 << 31 || (n > 0 && (!keys_dev || !keys_out_dev)) ||
        !trim_args_ok(frac, mult, d_floor))
        return PCP_ERR_ARG;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    Tmp tmp(ctx);
    uint32_t* work = nullptr;
    PCP_TRY(tmp.get(&work, trim_work_bytes() / sizeof(uint32_t)));
    return trim_keys_async(ctx, keys_dev, n, frac, mult, d_floor, keys_out_dev, trim_dev, work);
}

}  // extern "C"
