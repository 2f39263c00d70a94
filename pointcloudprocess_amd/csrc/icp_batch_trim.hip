// Per-segment trims of a batch (include/pcp.h, I5b): for every segment of a pcp_icp_batch the exact
// order statistic, cut and key filter of pcp_icp_trim_keys (I3) or pcp_icp_trim_keys_plane (I3b) over
// that segment's pairs alone, and the two device loops that put the trim between the keys and the
// accumulation of a batch iteration.  Three launches whatever the number of segments is:
//
//   k_bt_stat     one chunk per wave (k_batch_acc's grid): slot d of the padded layout gets the key
//                 the select ranks, skeys[d] = (b << 32 | low word of the pair's key) for a valid
//                 (point trim) or usable (plane trim) pair, kNoKey for a pad slot or any other pair.
//                 b is the key's high word, or the bits of rho from pose32 / xform / plane_pair /
//                 plane_residual of icp_pair.hpp, the text k_res_keys (icp_plane.hip) calls.
//   k_bt_select   one workgroup per segment: the 11 / 11 / 10-bit radix select of icp_trim.hip over
//                 the segment's own slots, contiguous in skeys.  Histogram, rank and prefix stay in
//                 LDS and the pick runs between the passes in the same block: global histograms would
//                 be nseg x 2048 counters per pass.  Writes the segment's row {m, 0, sel, bits of cut}.
//   k_bt_filter   one chunk per wave: keeps or rejects keys[original index] by skeys[d] against the
//                 segment's cut and adds the chunk's kept count to the row (an integer atomic).
//
// The digits, the wave's histogram count, the rank and the cut are icp_trim.hpp's, shared with the
// single select.  Everything is integer counting, so a run repeats bit for bit.
//
// Barriers and ballots: every loop around one has a block-uniform trip count with the load guarded
// inside; the block of an empty segment leaves, as a whole, before the first barrier.
#include "icp_batch.hpp"
#include "icp_trim.hpp"

namespace pcp {
namespace {

constexpr int kSB = 1024;  // k_bt_select: 16 waves keep a workgroup's walk over a long segment fed
constexpr int kSPer = 4;   // keys per thread and block iteration of its histogram passes

// ---- the ranked key of every slot
template <bool PLANE>
__global__ void __launch_bounds__(kBB) k_bt_stat(const float4* qrec, const int32_t* chunk_seg, int64_t nch,
                                                 const double* T, const uint64_t* keys, const float4* rec,
                                                 uint64_t nrec, uint64_t* skeys) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * kBW + (threadIdx.x >> 6);
    if (c >= nch) return;
    const float4 v = qrec[c * 64 + lane];
    const int oi = __float_as_int(v.w);
    uint64_t out = kNoKey;
    if constexpr (PLANE) {
        const int s = __builtin_amdgcn_readfirstlane(chunk_seg[c]);
        const Pose32 P = pose32(T + 16 * (int64_t)s);  // T is wave-uniform
        if (oi >= 0) {
            const uint64_t key = keys[oi];
            PlanePair pr;
            if (plane_pair(key, rec, nrec, pr)) {
                float x, y, z;
                xform(P, v, x, y, z);
                const double r = plane_residual(x, y, z, pr);
                const float rho = (float)(r * r);
                if (rho == rho) out = key_make(rho, key_index(key));
            }
        }
    } else {
        if (oi >= 0) out = keys[oi];
    }
    skeys[c * 64 + lane] = out;
}

// ---- one pass of a segment's select: the histogram of digit P over the n slots at sk whose higher
// digits equal prefix, then the bin holding rank; prefix and rank are block-uniform in and out.
// P == 0 also finds m and the rank itself.
struct SegSelect {
    uint32_t h[kTBins];
    uint32_t part[kSB];
    uint64_t rank;
    uint32_t prefix;
};

template <int P>
__device__ __forceinline__ void seg_pass(SegSelect& S, const uint64_t* sk, int64_t n, float frac, uint64_t& m,
                                         uint64_t& rank, uint32_t& prefix) {
    constexpr int bits = digit_bits(P), nb = 1 << bits, per = nb / kSB;
    static_assert(per >= 1, "one bin per thread at least");
    const int tid = threadIdx.x;
    for (int b = tid; b < nb; b += kSB) S.h[b] = 0;
    __syncthreads();
    // n is the same for every thread of the block, so the ballots of count_digit see whole waves
    for (int64_t base = 0; base < n; base += (int64_t)kSB * kSPer) {
        uint64_t k[kSPer];
#pragma unroll
        for (int u = 0; u < kSPer; u++) {
            const int64_t i = base + u * kSB + tid;
            k[u] = i < n ? sk[i] : kNoKey;
        }
#pragma unroll
        for (int u = 0; u < kSPer; u++) count_digit<P>(S.h, k[u], prefix);
    }
    __syncthreads();
    uint32_t c[per], s = 0;
#pragma unroll
    for (int j = 0; j < per; j++) {
        c[j] = S.h[tid * per + j];
        s += c[j];  // a bin, and their total m, is < 2^31
    }
    S.part[tid] = s;
    __syncthreads();
    for (int o = 1; o < kSB; o <<= 1) {
        const uint32_t v = tid >= o ? S.part[tid - o] : 0u;
        __syncthreads();
        S.part[tid] += v;
        __syncthreads();
    }
    if (P == 0) {
        m = S.part[kSB - 1];
        rank = trim_rank(frac, m);
    }
    if (tid == 0) {  // m == 0: no bin holds the rank and sel stays 0
        S.prefix = prefix << bits;
        S.rank = rank;
    }
    __syncthreads();
    const uint64_t excl = S.part[tid] - s;
    if (rank >= excl && rank < excl + s) {  // one thread at most
        uint64_t cum = excl;
#pragma unroll
        for (int j = 0; j < per; j++) {
            if (rank < cum + c[j]) {
                S.prefix = (prefix << bits) | (uint32_t)(tid * per + j);
                S.rank = rank - cum;
                break;
            }
            cum += c[j];
        }
    }
    __syncthreads();
    prefix = S.prefix;
    rank = S.rank;
    // the next pass writes S.prefix / S.rank only after its own barriers
}

__global__ void __launch_bounds__(kSB) k_bt_select(const uint64_t* skeys, const int32_t* seg_chunk, float frac,
                                                   float mult, float d_floor, uint64_t* trim) {
    __shared__ SegSelect S;
    const int s = blockIdx.x;
    const int64_t c0 = seg_chunk[s], c1 = seg_chunk[s + 1];
    uint64_t* row = trim + 4 * (int64_t)s;
    if (c0 == c1) {  // an empty segment: the whole block leaves before the first barrier
        if (threadIdx.x == 0) {
            row[0] = row[1] = row[2] = 0;
            row[3] = __float_as_uint(d_floor * d_floor);
        }
        return;
    }
    const uint64_t* sk = skeys + 64 * c0;
    const int64_t n = 64 * (c1 - c0);
    uint64_t m = 0, rank = 0;
    uint32_t prefix = 0;
    seg_pass<0>(S, sk, n, frac, m, rank, prefix);
    seg_pass<1>(S, sk, n, frac, m, rank, prefix);
    seg_pass<2>(S, sk, n, frac, m, rank, prefix);
    if (threadIdx.x == 0) {
        row[0] = m;
        row[1] = 0;  // k_bt_filter adds to it
        row[2] = prefix;
        row[3] = trim_cut_bits(prefix, mult, d_floor);
    }
}

// ---- the filter: the pair of slot d is kept iff its ranked key is valid and as_float(its high word)
// <= its segment's cut.  A kept key is the caller's, all 64 bits.  In place the point trim stores
// only rejected valid keys, the plane trim every key not kept (a pair without a usable plane record
// is still a pair in keys); out of place every key of a query is written.
template <bool PLANE>
__global__ void __launch_bounds__(kBB) k_bt_filter(const float4* qrec, const int32_t* chunk_seg, int64_t nch,
                                                   const uint64_t* keys, const uint64_t* skeys, uint64_t* out,
                                                   int inplace, uint64_t* trim) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * kBW + (threadIdx.x >> 6);
    if (c >= nch) return;  // whole waves
    const int s = __builtin_amdgcn_readfirstlane(chunk_seg[c]);
    uint64_t* row = trim + 4 * (int64_t)s;
    const float cut = __uint_as_float((uint32_t)row[3]);
    const int oi = __float_as_int(qrec[c * 64 + lane].w);
    const uint64_t rk = skeys[c * 64 + lane];  // kNoKey in a pad slot
    const bool valid = rk != kNoKey;
    const bool keep = valid && key_d2(rk) <= cut;
    if (oi >= 0) {
        if (inplace) {
            if (PLANE ? !keep : valid && !keep) out[oi] = kNoKey;
        } else {
            out[oi] = keep ? (PLANE ? keys[oi] : rk) : kNoKey;
        }
    }
    const uint32_t cnt = (uint32_t)__popcll(__ballot(keep));
    if (lane == 0 && cnt) atomicAdd((unsigned long long*)&row[1], (unsigned long long)cnt);
}

}  // namespace

// the trim of every segment on ctx's stream: skeys is 64 * nch keys of the caller's guard memory;
// planes == nullptr ranks the keys' own high words (declared in icp_batch.hpp: the point-to-point
// trimmed loop of icp_batch_p2p.hip runs it too)
void launch_trim(pcp_ctx* ctx, const pcp_icp_batch* b, const double* T_dev, const uint64_t* keys,
                 const pcp_icp_planes* planes, float frac, float mult, float d_floor, uint64_t* out, uint64_t* trim,
                 uint64_t* skeys) {
    const dim3 grid(chunk_grid(b->nch)), block(kBB);
    const float4* qrec = (const float4*)b->rec;
    const int32_t* chunk_seg = (const int32_t*)b->chunk_seg;
    const int inplace = out == keys ? 1 : 0;
    if (b->nch > 0) {
        if (planes)
            hipLaunchKernelGGL(k_bt_stat<true>, grid, block, 0, ctx->stream, qrec, chunk_seg, b->nch, T_dev, keys,
                               (const float4*)planes->rec, (uint64_t)planes->n, skeys);
        else
            hipLaunchKernelGGL(k_bt_stat<false>, grid, block, 0, ctx->stream, qrec, chunk_seg, b->nch, T_dev, keys,
                               (const float4*)nullptr, (uint64_t)0, skeys);
    }
    hipLaunchKernelGGL(k_bt_select, dim3(b->nseg), dim3(kSB), 0, ctx->stream, (const uint64_t*)skeys,
                       (const int32_t*)b->seg_chunk, frac, mult, d_floor, trim);
    if (b->nch > 0) {
        if (planes)
            hipLaunchKernelGGL(k_bt_filter<true>, grid, block, 0, ctx->stream, qrec, chunk_seg, b->nch, keys,
                               (const uint64_t*)skeys, out, inplace, trim);
        else
            hipLaunchKernelGGL(k_bt_filter<false>, grid, block, 0, ctx->stream, qrec, chunk_seg, b->nch, keys,
                               (const uint64_t*)skeys, out, inplace, trim);
    }
}

namespace {

// the argument rules the two trims share; planes and T_dev are checked by the plane trim's caller
bool trim_call_ok(const pcp_ctx* ctx, const pcp_icp_batch* b, const uint64_t* keys, float frac, float mult,
                  float d_floor, const uint64_t* out, const uint64_t* trim) {
    return ctx && b && !(b->nseg > 0 && !trim) && !(b->nq > 0 && (!keys || !out)) && trim_args_ok(frac, mult, d_floor);
}

// iters x (keys, trim in place by the point distance or, with by_plane, the plane residual at the
// iteration's poses, accumulate, sum + solve): six launches per iteration, none of them sized by a
// host read, and no allocation inside the loop
int run_trimmed(pcp_ctx* ctx, const char* who, pcp_icp_batch* b, const pcp_icp_planes* planes, double* T_dev,
                float rmax, float frac, float mult, float d_floor, bool by_plane, int iters, double* stats_dev,
                uint64_t* trim_dev) {
    if (!ctx || !b || iters < 0 || !(rmax >= 0.f) || !trim_args_ok(frac, mult, d_floor) ||
        (b->nseg > 0 && (!planes || !T_dev || !stats_dev || !trim_dev)))
        return PCP_ERR_ARG;
    if (planes && planes->n != b->target->n_in)
        return set_error(ctx, PCP_ERR_ARG, "%s: %lld plane records for a target of %lld points", who,
                         (long long)planes->n, (long long)b->target->n_in);
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    if (b->nseg == 0) return PCP_OK;
    Tmp tmp(ctx);
    uint64_t *keys = nullptr, *skeys = nullptr;
    double* part = nullptr;
    PCP_TRY(tmp.get(&keys, (size_t)b->nq));
    PCP_TRY(tmp.get(&skeys, (size_t)b->nch * 64));
    PCP_TRY(tmp.get(&part, (size_t)b->nch * kPAcc));
    for (int it = 0; it < iters; it++) {
        if (b->nch > 0) batch_launch_search(ctx, b, T_dev, rmax, keys);
        launch_trim(ctx, b, T_dev, keys, by_plane ? planes : nullptr, frac, mult, d_floor, keys, trim_dev, skeys);
        if (b->nch > 0) batch_launch_acc(ctx, b, T_dev, keys, planes, part);
        batch_launch_sum_solve(ctx, b, part, nullptr, T_dev, stats_dev);
    }
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

}  // namespace
}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_icp_batch_trim_keys(pcp_ctx* ctx, pcp_icp_batch* b, const uint64_t* keys_dev, float frac, float mult,
                            float d_floor, uint64_t* keys_out_dev, uint64_t* trim_dev) {
    if (!trim_call_ok(ctx, b, keys_dev, frac, mult, d_floor, keys_out_dev, trim_dev)) return PCP_ERR_ARG;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    if (b->nseg == 0) return PCP_OK;
    Tmp tmp(ctx);
    uint64_t* skeys = nullptr;
    PCP_TRY(tmp.get(&skeys, (size_t)b->nch * 64));
    launch_trim(ctx, b, nullptr, keys_dev, nullptr, frac, mult, d_floor, keys_out_dev, trim_dev, skeys);
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

int pcp_icp_batch_trim_keys_plane(pcp_ctx* ctx, pcp_icp_batch* b, const double* T_dev, const uint64_t* keys_dev,
                                  const pcp_icp_planes* planes, float frac, float mult, float d_floor,
                                  uint64_t* keys_out_dev, uint64_t* trim_dev) {
    if (!trim_call_ok(ctx, b, keys_dev, frac, mult, d_floor, keys_out_dev, trim_dev) ||
        (b->nseg > 0 && (!T_dev || !planes)))
        return PCP_ERR_ARG;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    if (b->nseg == 0) return PCP_OK;
    Tmp tmp(ctx);
    uint64_t* skeys = nullptr;
    PCP_TRY(tmp.get(&skeys, (size_t)b->nch * 64));
    launch_trim(ctx, b, T_dev, keys_dev, planes, frac, mult, d_floor, keys_out_dev, trim_dev, skeys);
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

int pcp_icp_batch_run_plane_trimmed_dev(pcp_ctx* ctx, pcp_icp_batch* b, const pcp_icp_planes* planes, double* T_dev,
                                        float rmax, float frac, float mult, float d_floor, int iters,
                                        double* stats_dev, uint64_t* trim_dev) {
    return run_trimmed(ctx, "pcp_icp_batch_run_plane_trimmed_dev", b, planes, T_dev, rmax, frac, mult, d_floor, false,
                       iters, stats_dev, trim_dev);
}

int pcp_icp_batch_run_plane_rtrimmed_dev(pcp_ctx* ctx, pcp_icp_batch* b, const pcp_icp_planes* planes,
                                         double* T_dev, float rmax, float frac, float mult, float d_floor, int iters,
                                         double* stats_dev, uint64_t* trim_dev) {
    return run_trimmed(ctx, "pcp_icp_batch_run_plane_rtrimmed_dev", b, planes, T_dev, rmax, frac, mult, d_floor, true,
                       iters, stats_dev, trim_dev);
}

}  // extern "C"
