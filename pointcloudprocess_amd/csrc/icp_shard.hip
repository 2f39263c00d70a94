// Target-sharded ICP: what is done with the per-query keys once the ranks have
// exchanged them.  None of it looks at a handle's search state.
//
// Owned here: the key loops k_acc_keys, k_sum_partials, k_keys_owner, k_acc_owned, k_slab_guard and
// their entry points.  The keys themselves are made by icp.hip (k_make_keys); the key's layout, the
// pose cast, the Kabsch terms of a pair and the block reductions are icp_pair.hpp's.
#include "icp_handle.hpp"

namespace pcp {
namespace {

// accumulators over the queries whose global winner lies in [lo, hi) (this rank's shard);
// float products are exact in fp64, so only the summation order differs from the oracle
__global__ void __launch_bounds__(kPairBlock) k_acc_keys(const QXyz* q, const int32_t* qidx, int64_t n,
                                                         const uint64_t* keys, uint64_t lo, uint64_t hi,
                                                         const float* shard, size_t stride_f, Pose32 P,
                                                         double* partials) {
    double acc[kAcc - 1];
#pragma unroll
    for (int k = 0; k < kAcc - 1; k++) acc[k] = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 qq = make_float4(q[i].x, q[i].y, q[i].z, 0.f);
        const uint64_t key = keys[qidx[i]];
        if (key == kNoKey) continue;
        const uint64_t g = key_index(key);
        if (g < lo || g >= hi) continue;
        const float* p = shard + (size_t)(g - lo) * stride_f;
        float x, y, z;
        xform(P, qq, x, y, z);
        const double qv[3] = {x, y, z}, pv[3] = {p[0], p[1], p[2]};
        kabsch_terms(qv, pv, key, acc);
    }
    block_partials<kAcc - 1, kAcc>(acc, partials + (int64_t)blockIdx.x * kAcc);
}

__global__ void __launch_bounds__(kPairBlock) k_sum_partials(const double* part, int nb, double* out) {
    sum_partials<kAcc>(part, nb, out);
}

// Target-sharded mode, device-resident form: after a ReduceScatter(MIN) of
// the per-query keys, each rank knows the global winners of its slice of the queries; the shard
// that owns each winner (by its global target index) is all-gathered as one byte per query, and
// every rank accumulates exactly the queries whose winner lies in its own shard, reading the
// winner from its LOCAL shard -- no rank ever holds the full target.  A SUM over ranks gives the
// accumulators of every query.
// owner[i] = s with bounds[s] <= global index < bounds[s + 1], or 255 (no correspondence)
__global__ void k_keys_owner(const uint64_t* keys, int64_t n, const int64_t* bounds, int nshards, uint8_t* owner) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = keys[i];
        uint8_t o = 255;
        if (k != kNoKey) {
            const int64_t g = (int64_t)key_index(k);
            int lo = 0, hi = nshards;  // the last s with bounds[s] <= g
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (bounds[mid] <= g) lo = mid;
                else hi = mid;
            }
            o = (uint8_t)lo;
        }
        owner[i] = o;
    }
}

// accumulators of the queries (original order, q) whose winner this rank owns: the winner is
// the rank's local key's target (its global index less lo) -- for an owned query the local key
// IS the global MIN.  The pose is pose32 of the device 4x4, the image xform's and the terms
// kabsch_terms' (icp_pair.hpp), so only the summation order differs from the oracle.
__global__ void __launch_bounds__(kPairBlock) k_acc_owned(const double* T, const float* q, size_t qs, int64_t n,
                                                          const uint64_t* keys, const uint8_t* owner, int rank,
                                                          int64_t lo, int64_t hi, const float* shard, size_t ss,
                                                          double* partials) {
    const Pose32 P = pose32(T);
    double acc[kAcc - 1];
#pragma unroll
    for (int k = 0; k < kAcc - 1; k++) acc[k] = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (owner[i] != (uint8_t)rank) continue;
        const uint64_t key = keys[i];
        const int64_t g = (int64_t)key_index(key);
        if (key == kNoKey || g < lo || g >= hi) continue;
        const float* p = shard + (size_t)(g - lo) * ss;
        float x, y, z;
        xform(P, q + (size_t)i * qs, x, y, z);
        const double qv[3] = {x, y, z}, pv[3] = {p[0], p[1], p[2]};
        kabsch_terms(qv, pv, key, acc);
    }
    block_partials<kAcc - 1, kAcc>(acc, partials + (int64_t)blockIdx.x * kAcc);
}

// co-partitioned slab guard (one thread): the owned queries' box [b0..b5] = {x0,x1,y0,y1,z0,z1}
// under the device pose must keep x within [lo, hi] (the slab core widened by the target halo
// less rmax); the x-extreme of an affine image of a box is at a corner.  Latches flag = 1.
__global__ void k_slab_guard(const double* T, double b0, double b1, double b2, double b3, double b4, double b5,
                             double lo, double hi, int* flag) {
    const double bx[2] = {b0, b1}, by[2] = {b2, b3}, bz[2] = {b4, b5};
    double mn = INFINITY, mx = -INFINITY;
    for (int c = 0; c < 8; c++) {
        const double x = T[0] * bx[c & 1] + T[1] * by[(c >> 1) & 1] + T[2] * bz[c >> 2] + T[3];
        mn = fmin(mn, x);
        mx = fmax(mx, x);
    }
    if (!(mn >= lo && mx <= hi)) *flag = 1;
}

}  // namespace
}  // namespace pcp

extern "C" {

int pcp_keys_owner(pcp_ctx* ctx, const uint64_t* keys_dev, int64_t n, const int64_t* bounds_dev, int nshards,
                   uint8_t* owner_dev) {
    if (!ctx || n < 0 || (n > 0 && (!keys_dev || !owner_dev)) || !bounds_dev || nshards < 1 || nshards > 255)
        return PCP_ERR_ARG;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return PCP_OK;
    hipLaunchKernelGGL(pcp::k_keys_owner, dim3(pcp::grid_for(n, 256, 8192)), dim3(256), 0, ctx->stream, keys_dev, n,
                       bounds_dev, nshards, owner_dev);
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

int pcp_icp_accumulate_owned(pcp_ctx* ctx, const double* T_dev, const float* q_dev, size_t q_stride, int64_t nq,
                             const uint64_t* keys_dev, const uint8_t* owner_dev, int rank, int64_t lo, int64_t hi,
                             const float* shard_xyz_dev, size_t shard_stride, double* acc_dev) {
    if (!ctx || !T_dev || nq < 0 || (nq > 0 && (!q_dev || !keys_dev || !owner_dev)) || !acc_dev || rank < 0 ||
        rank > 254 || lo < 0 || hi < lo || (hi > lo && !shard_xyz_dev))
        return PCP_ERR_ARG;
    if (q_stride == 0) q_stride = 3 * sizeof(float);
    if (shard_stride == 0) shard_stride = 3 * sizeof(float);
    if (q_stride % sizeof(float) || shard_stride % sizeof(float))
        return pcp::set_error(ctx, PCP_ERR_ARG, "strides must be whole floats");
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    const int nb = (int)std::min<int64_t>(std::max<int64_t>(1, (nq + 255) / 256), 2048);
    pcp::Tmp tmp(ctx);
    double* part = nullptr;
    PCP_TRY(tmp.get(&part, (size_t)nb * pcp::kAcc));
    const dim3 block(pcp::kPairBlock);
    hipLaunchKernelGGL(pcp::k_acc_owned, dim3(nb), block, 0, ctx->stream, T_dev, q_dev, q_stride / sizeof(float), nq,
                       keys_dev, owner_dev, rank, lo, hi, shard_xyz_dev, shard_stride / sizeof(float), part);
    hipLaunchKernelGGL(pcp::k_sum_partials, dim3(1), block, 0, ctx->stream, (const double*)part, nb, acc_dev);
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

int pcp_slab_guard(pcp_ctx* ctx, const double* T_dev, const double box[6], double lo, double hi, int* flag_dev) {
    if (!ctx || !T_dev || !box || !flag_dev) return PCP_ERR_ARG;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(pcp::k_slab_guard, dim3(1), dim3(1), 0, ctx->stream, T_dev, box[0], box[1], box[2], box[3],
                       box[4], box[5], lo, hi, flag_dev);
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

int pcp_icp_accumulate_keys(pcp_ctx* ctx, pcp_icp* icp, const double T[16], const uint64_t* keys_dev,
                            int64_t lo, int64_t hi, const float* shard_xyz_dev, size_t shard_stride_bytes,
                            double* acc_dev) {
    if (!ctx || !icp || !T || !keys_dev || !acc_dev || lo < 0 || hi < lo || (hi > lo && !shard_xyz_dev))
        return PCP_ERR_ARG;
    if (shard_stride_bytes == 0) shard_stride_bytes = 3 * sizeof(float);
    if (shard_stride_bytes % sizeof(float)) return pcp::set_error(ctx, PCP_ERR_ARG, "shard stride must be whole floats");
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    const int nb = (int)std::min<int64_t>(std::max<int64_t>(1, (icp->nq + 255) / 256), icp->nb_fast + icp->nb_ring);
    const dim3 block(pcp::kPairBlock);
    hipLaunchKernelGGL(pcp::k_acc_keys, dim3(nb), block, 0, ctx->stream, icp->q, icp->qidx, icp->nq, keys_dev,
                       (uint64_t)lo, (uint64_t)hi, shard_xyz_dev, shard_stride_bytes / sizeof(float), pcp::pose32(T),
                       icp->partials);
    hipLaunchKernelGGL(pcp::k_sum_partials, dim3(1), block, 0, ctx->stream, (const double*)icp->partials, nb, acc_dev);
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

}  // extern "C"
