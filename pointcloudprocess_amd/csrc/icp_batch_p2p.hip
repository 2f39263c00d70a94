// Point-to-point registration over a batch (include/pcp.h, I5c): per segment the 24 Kabsch
// accumulators of pcp_icp_solve and its 3x3 solve, in the batch's launch shape -- an iteration is
// keys, accumulate, sum + solve (three launches whatever the number of segments is), or six with
// the per-segment point trim of I5b between the keys and the accumulation.  Nothing is fused: the
// loops are the entries in turn, bit for bit.
//
//   k_batch_acc_kabsch        one chunk per wave (k_batch_acc's shape): the 23 sums of the chunk's
//                             pairs by a butterfly -> partials[chunk], 24 doubles with [23] = 0
//   k_batch_sum_solve_kabsch  one block per segment: its chunks' partials in k_batch_sum_solve's
//                             order (8 interleaved groups, then the groups in order); row s when
//                             asked; thread 0 runs kabsch_apply when T is given
//   k_batch_solve_kabsch      thread s: kabsch_apply on row s
//
// Owned here: those three loops and the four entries.  The search is k_batch_search
// (icp_batch.hip), the trim launch_trim (icp_batch_trim.hip); the pose cast, the image and the 23
// terms are icp_pair.hpp's (pose32, xform, kabsch_terms: the text of pcp_icp_accumulate_owned), the
// solve icp_solve.hpp's.
#include "icp_batch.hpp"
#include "icp_solve.hpp"

namespace pcp {
namespace {

constexpr int kSumGroups = 8;  // chunk c of a segment is summed by group c % 8, as k_batch_sum_solve

// one thread: k_icp_solve_dev's step (icp_pose.hpp) on one segment's accumulators, pose and stats.
// A refused solve latches stats[0] = -1 and freezes T; the fallback count still adds.
__device__ inline void kabsch_apply(const double* a, int do_scale, double* T, double* stats) {
    if (stats[0] < 0) return;
    double dT[16], Tn[16];
    stats[2] += a[23];
    if (icp_solve(a, do_scale, dT) != PCP_OK) {
        stats[0] = -1.0;
        return;
    }
    stats[1] = sqrt(a[22] / a[0]);
    stats[3] += 1.0;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double v = 0;
            for (int k = 0; k < 4; k++) v += dT[4 * i + k] * T[4 * k + j];
            Tn[4 * i + j] = v;
        }
    for (int k = 0; k < 16; k++) T[k] = Tn[k];
}

// ---- accumulate: a pad slot, "no pair" or a target index at or past nt contributes zeros (and
// reads no target); the 23 terms of the chunk's 64 lanes are added by a butterfly, the same tree on
// every run.  tgt is the caller's cloud at caller index, ts floats apart.
__global__ void __launch_bounds__(kBB) k_batch_acc_kabsch(const float4* qrec, const int32_t* chunk_seg, int64_t nch,
                                                          const double* T, const uint64_t* keys, const float* tgt,
                                                          size_t ts, uint64_t nt, double* partials) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * kBW + (threadIdx.x >> 6);
    if (c >= nch) return;
    const int s = __builtin_amdgcn_readfirstlane(chunk_seg[c]);
    const Pose32 P = pose32(T + 16 * (int64_t)s);  // T is wave-uniform
    const float4 v = qrec[c * 64 + lane];
    const int oi = __float_as_int(v.w);
    double term[kAcc - 1];
#pragma unroll
    for (int k = 0; k < kAcc - 1; k++) term[k] = 0.0;
    if (oi >= 0) {
        const uint64_t key = keys[oi];
        const uint64_t j = key_index(key);
        if (key != kNoKey && j < nt) {
            const float* p = tgt + (size_t)j * ts;
            float x, y, z;
            xform(P, v, x, y, z);
            const double qv[3] = {x, y, z}, pv[3] = {p[0], p[1], p[2]};
            kabsch_terms(qv, pv, key, term);
        }
    }
    double mine = 0.0;  // lane k keeps sum k; lane 23 keeps the 0 of [23]
#pragma unroll
    for (int k = 0; k < kAcc - 1; k++) {
        double t = term[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
        mine = lane == k ? t : mine;
    }
    if (lane < kAcc) partials[c * kAcc + lane] = mine;
}

// ---- one block per segment: group g = 0..7 adds chunks g, g + 8, .. in chunk order, then the
// groups are added in order; row s of acc_out when given; thread 0 solves when T is given.  A
// segment without chunks reads nothing of part and sums to 24 zeros.
__global__ void __launch_bounds__(kBB) k_batch_sum_solve_kabsch(const double* part, const int32_t* seg_chunk,
                                                                double* acc_out, int do_scale, double* T,
                                                                double* stats) {
    __shared__ double sg[kSumGroups][kAcc];
    __shared__ double acc[kAcc];
    const int s = blockIdx.x, t = threadIdx.x;
    const int64_t c0 = seg_chunk[s], c1 = seg_chunk[s + 1];
    if (t < kSumGroups * kAcc) {
        const int k = t % kAcc, grp = t / kAcc;
        double v = 0.0;
        for (int64_t c = c0 + grp; c < c1; c += kSumGroups) v += part[c * kAcc + k];
        sg[grp][k] = v;
    }
    __syncthreads();
    if (t < kAcc) {
        double v = 0.0;
        for (int grp = 0; grp < kSumGroups; grp++) v += sg[grp][t];
        acc[t] = v;
        if (acc_out) acc_out[(int64_t)s * kAcc + t] = v;
    }
    __syncthreads();
    if (T && t == 0) {
        double a[kAcc];
        for (int k = 0; k < kAcc; k++) a[k] = acc[k];
        kabsch_apply(a, do_scale, T + 16 * (int64_t)s, stats + 4 * (int64_t)s);
    }
}

// thread s: kabsch_apply on row s
__global__ void __launch_bounds__(64) k_batch_solve_kabsch(const double* acc, int nseg, int do_scale, double* T,
                                                           double* stats) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= nseg) return;
    double a[kAcc];
    for (int k = 0; k < kAcc; k++) a[k] = acc[(int64_t)s * kAcc + k];
    kabsch_apply(a, do_scale, T + 16 * (int64_t)s, stats + 4 * (int64_t)s);
}

// the target cloud's rules, shared by the accumulate entry and the loops; the stride comes back in
// bytes with 0 replaced
int check_target(pcp_ctx* ctx, const float* target_xyz, size_t* t_stride, int64_t n_target) {
    if (n_target < 0 || (n_target > 0 && !target_xyz)) return PCP_ERR_ARG;
    return check_stride(ctx, t_stride);
}

// iters x (keys, the point trim in place when trim_dev is given, accumulate, sum + solve): three or
// six launches per iteration, none of them sized by a host read, and no allocation inside the loop
int run_p2p(pcp_ctx* ctx, const char* who, pcp_icp_batch* b, const float* target_xyz, size_t t_stride,
            int64_t n_target, double* T_dev, float rmax, bool trimmed, float frac, float mult, float d_floor, int iters,
            int do_scale, double* stats_dev, uint64_t* trim_dev) {
    if (!ctx || !b || iters < 0 || !(rmax >= 0.f) || (trimmed && !trim_args_ok(frac, mult, d_floor)) ||
        (b->nseg > 0 && (!T_dev || !stats_dev || (trimmed && !trim_dev))))
        return PCP_ERR_ARG;
    PCP_TRY(check_target(ctx, target_xyz, &t_stride, n_target));
    if (n_target != b->target->n_in)
        return set_error(ctx, PCP_ERR_ARG, "%s: %lld target points for an index of %lld points", who,
                         (long long)n_target, (long long)b->target->n_in);
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    if (b->nseg == 0) return PCP_OK;
    Tmp tmp(ctx);
    uint64_t *keys = nullptr, *skeys = nullptr;
    double* part = nullptr;
    PCP_TRY(tmp.get(&keys, (size_t)b->nq));
    if (trimmed) PCP_TRY(tmp.get(&skeys, (size_t)b->nch * 64));
    PCP_TRY(tmp.get(&part, (size_t)b->nch * kAcc));
    for (int it = 0; it < iters; it++) {
        if (b->nch > 0) batch_launch_search(ctx, b, T_dev, rmax, keys);
        if (trimmed) launch_trim(ctx, b, T_dev, keys, nullptr, frac, mult, d_floor, keys, trim_dev, skeys);
        if (b->nch > 0)
            batch_launch_acc_kabsch(ctx, b, T_dev, keys, target_xyz, t_stride / sizeof(float), n_target, part);
        batch_launch_sum_solve_kabsch(ctx, b, part, nullptr, do_scale, T_dev, stats_dev);
    }
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

}  // namespace

void batch_launch_acc_kabsch(pcp_ctx* ctx, const pcp_icp_batch* b, const double* T_dev, const uint64_t* keys,
                             const float* target_xyz, size_t t_stride_f, int64_t n_target, double* part) {
    hipLaunchKernelGGL(k_batch_acc_kabsch, dim3(chunk_grid(b->nch)), dim3(kBB), 0, ctx->stream,
                       (const float4*)b->rec, (const int32_t*)b->chunk_seg, b->nch, T_dev, keys, target_xyz,
                       t_stride_f, (uint64_t)n_target, part);
}

void batch_launch_sum_solve_kabsch(pcp_ctx* ctx, const pcp_icp_batch* b, const double* part, double* acc_out,
                                   int do_scale, double* T, double* stats) {
    hipLaunchKernelGGL(k_batch_sum_solve_kabsch, dim3(b->nseg), dim3(kBB), 0, ctx->stream, part,
                       (const int32_t*)b->seg_chunk, acc_out, do_scale, T, stats);
}

}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_icp_batch_accumulate(pcp_ctx* ctx, pcp_icp_batch* b, const double* T_dev, const uint64_t* keys_dev,
                             const float* target_xyz_dev, size_t t_stride_bytes, int64_t n_target, double* acc_dev) {
    if (!ctx || !b || (b->nseg > 0 && (!T_dev || !acc_dev)) || (b->nq > 0 && !keys_dev)) return PCP_ERR_ARG;
    PCP_TRY(check_target(ctx, target_xyz_dev, &t_stride_bytes, n_target));
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    if (b->nseg == 0) return PCP_OK;
    Tmp tmp(ctx);
    double* part = nullptr;
    PCP_TRY(tmp.get(&part, (size_t)b->nch * kAcc));
    if (b->nch > 0)
        batch_launch_acc_kabsch(ctx, b, T_dev, keys_dev, target_xyz_dev, t_stride_bytes / sizeof(float), n_target,
                                part);
    batch_launch_sum_solve_kabsch(ctx, b, part, acc_dev, 0, nullptr, nullptr);
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

int pcp_icp_batch_solve_dev(pcp_ctx* ctx, const double* acc_dev, int nseg, int do_scale, double* T_dev,
                            double* stats_dev) {
    if (!ctx || nseg < 0 || nseg > 65535 || (nseg > 0 && (!acc_dev || !T_dev || !stats_dev))) return PCP_ERR_ARG;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    if (nseg == 0) return PCP_OK;
    hipLaunchKernelGGL(k_batch_solve_kabsch, dim3((nseg + 63) / 64), dim3(64), 0, ctx->stream, acc_dev, nseg,
                       do_scale, T_dev, stats_dev);
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

int pcp_icp_batch_run_dev(pcp_ctx* ctx, pcp_icp_batch* b, const float* target_xyz_dev, size_t t_stride_bytes,
                          int64_t n_target, double* T_dev, float rmax, int iters, int do_scale, double* stats_dev) {
    return run_p2p(ctx, "pcp_icp_batch_run_dev", b, target_xyz_dev, t_stride_bytes, n_target, T_dev, rmax, false, 0.f,
                   0.f, 0.f, iters, do_scale, stats_dev, nullptr);
}

int pcp_icp_batch_run_trimmed_dev(pcp_ctx* ctx, pcp_icp_batch* b, const float* target_xyz_dev, size_t t_stride_bytes,
                                  int64_t n_target, double* T_dev, float rmax, float frac, float mult, float d_floor,
                                  int iters, int do_scale, double* stats_dev, uint64_t* trim_dev) {
    return run_p2p(ctx, "pcp_icp_batch_run_trimmed_dev", b, target_xyz_dev, t_stride_bytes, n_target, T_dev, rmax,
                   true, frac, mult, d_floor, iters, do_scale, stats_dev, trim_dev);
}

}  // extern "C"
