// Point-to-plane ICP (include/pcp.h, I2): the build's own contract, not trimesh2's.  The exact
// correspondence search stays in icp.hip; this file takes its per-query winner keys
// (pcp_icp_keys_dev) and does the minimisation: a packed {point, normal} table of the target,
// the 30 accumulators of sum (n . (T q - p))^2 linearised at the pose, the scaled 6x6 LDL^T
// solve, and the device loop around the three (with the trim of icp_trim.hip between the keys and
// the accumulation in its trimmed form, pcp.h I3, or that trim's select over the pairs' squared
// plane residuals between this file's residual pass and that file's filter, I3b).  Owned here: the
// table build, the kernels' loops over the keys, and the host entry points.  The per-pair
// arithmetic and the block reductions are icp_pair.hpp's, the solve icp_plane_solve.hpp's.
//
// The accumulation's cost is its gather: one 32-byte record per pair at a data-dependent index,
// both halves in one 64-byte line (two arrays would cost two lines).  Everything else streams.
#include <algorithm>
#include <cmath>
#include <vector>

#include "icp_pair.hpp"

namespace pcp {
namespace {

constexpr int kPB = kPairBlock;
constexpr int kPBlocks = 2048;  // grid cap of the grid-stride kernels (pcp_icp_accumulate_owned's)

// one record per target point at its caller index; counts[block] = valid records it wrote
__global__ void __launch_bounds__(kPB) k_planes_build(const float* xyz, size_t ts, const float* nrm, size_t ns,
                                                      int64_t n, float4* rec, uint32_t* counts) {
    uint32_t cnt = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float* p = xyz + (size_t)i * ts;
        const float* v = nrm + (size_t)i * ns;
        float4 a = make_float4(p[0], p[1], p[2], 0.f), b = make_float4(v[0], v[1], v[2], 0.f);
        const bool fin = isfinite(a.x) && isfinite(a.y) && isfinite(a.z) && isfinite(b.x) && isfinite(b.y) &&
                         isfinite(b.z);
        if (fin && plane_valid(b.x, b.y, b.z)) {
            cnt++;
        } else {
            if (!fin) a = make_float4(0.f, 0.f, 0.f, 0.f);
            b = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        rec[2 * i] = a;
        rec[2 * i + 1] = b;
    }
    const uint32_t t = block_count(cnt);
    if (threadIdx.x == 0) counts[blockIdx.x] = t;
}

// Block partials of the 30 accumulators (pcp.h): grid-stride over the queries in their original
// order, per-lane fp64 sums of plane_terms (icp_pair.hpp) over the usable pairs (plane_pair) at
// the query's image under pose32 of the device 4x4, then block_partials.
__global__ void __launch_bounds__(kPB) k_acc_plane(const double* T, const float* q, size_t qs, int64_t n,
                                                   const uint64_t* keys, const float4* rec, uint64_t nrec,
                                                   double* partials) {
    const Pose32 P = pose32(T);
    double acc[kPAcc];
#pragma unroll
    for (int k = 0; k < kPAcc; k++) acc[k] = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t key = keys[i];
        PlanePair pr;
        if (!plane_pair(key, rec, nrec, pr)) continue;
        float x, y, z;
        xform(P, q + (size_t)i * qs, x, y, z);
        double term[kPAcc];
        plane_terms(x, y, z, pr, key, term);
#pragma unroll
        for (int k = 0; k < kPAcc; k++) acc[k] += term[k];
    }
    block_partials(acc, partials + (int64_t)blockIdx.x * kPAcc);
}

// Residual pass of the trim by plane residual (pcp.h, I3b): per pair the key the select of
// icp_trim.hip ranks, (bits of (float)(r * r) << 32) | target index for a usable pair and the "no
// pair" key otherwise.  The pose, the image, the usable-pair test and r are pose32, xform,
// plane_pair and plane_residual, which plane_terms squares: r is the value the accumulation
// squares; r -> -r under a negated normal, and r * r is then the same product.
__global__ void __launch_bounds__(kPB) k_res_keys(const double* T, const float* q, size_t qs, int64_t n,
                                                  const uint64_t* keys, const float4* rec, uint64_t nrec,
                                                  uint64_t* rkeys) {
    const Pose32 P = pose32(T);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t key = keys[i];
        uint64_t out = kNoKey;
        PlanePair pr;
        if (plane_pair(key, rec, nrec, pr)) {
            float x, y, z;
            xform(P, q + (size_t)i * qs, x, y, z);
            const double r = plane_residual(x, y, z, pr);
            const float rho = (float)(r * r);
            if (rho == rho) out = key_make(rho, key_index(key));
        }
        rkeys[i] = out;
    }
}

__global__ void __launch_bounds__(kPB) k_plane_sum(const double* part, int nb, double* out) {
    sum_partials<kPAcc>(part, nb, out);
}

__global__ void k_plane_solve_dev(const double* acc, double* T, double* stats) {
    double a[kPAcc];
    for (int k = 0; k < kPAcc; k++) a[k] = acc[k];
    solve_apply(a, T, stats);
}

// the loop's tail in one single-block launch: reduce the block partials, then thread 0 solves
__global__ void __launch_bounds__(kPB) k_plane_sum_solve(const double* part, int nb, double* T, double* stats) {
    __shared__ double acc[kPAcc];
    sum_partials<kPAcc>(part, nb, acc);  // ends with a barrier: acc is visible to thread 0
    if (threadIdx.x == 0) {
        double a[kPAcc];
        for (int k = 0; k < kPAcc; k++) a[k] = acc[k];
        solve_apply(a, T, stats);
    }
}

int acc_blocks(int64_t nq) { return (int)std::min<int64_t>(std::max<int64_t>(1, (nq + kPB - 1) / kPB), kPBlocks); }

void launch_acc(pcp_ctx* ctx, const double* T_dev, const float* q, size_t q_stride, int64_t nq, const uint64_t* keys,
                const pcp_icp_planes* pl, int nb, double* part) {
    hipLaunchKernelGGL(k_acc_plane, dim3(nb), dim3(kPB), 0, ctx->stream, T_dev, q, q_stride / sizeof(float), nq, keys,
                       (const float4*)pl->rec, (uint64_t)pl->n, part);
}

// pcp_icp_trim_keys_plane for callers that have checked the arguments and own the temporaries:
// rkeys (n residual keys) and the select's work memory
int trim_plane_async(pcp_ctx* ctx, const double* T_dev, const float* q, size_t q_stride, int64_t n,
                     const uint64_t* keys, const pcp_icp_planes* pl, float frac, float mult, float d_floor,
                     uint64_t* out, uint64_t* trim, uint64_t* rkeys, uint32_t* work) {
    const int nb = acc_blocks(n);
    if (n > 0)
        hipLaunchKernelGGL(k_res_keys, dim3(nb), dim3(kPB), 0, ctx->stream, T_dev, q, q_stride / sizeof(float), n,
                           keys, (const float4*)pl->rec, (uint64_t)pl->n, rkeys);
    PCP_TRY(trim_select_async(ctx, rkeys, n, frac, mult, d_floor, trim, work));
    return trim_filter_async(ctx, keys, rkeys, n, out, trim);
}

// iters x (keys, [trim in place: trim = {frac, mult, d_floor}, by the point distance (I3) or, with
// by_plane, by the plane residual (I3b); stats of the last one to trim_dev,] accumulate, sum +
// solve) on ctx's stream with no host round trip
int run_plane_loop(pcp_ctx* ctx, const char* who, pcp_icp* icp, const pcp_icp_planes* planes, const float* q_dev,
                   size_t q_stride, int64_t nq, double* T_dev, float rmax, const float* trim, bool by_plane,
                   int iters, double* stats_dev, uint64_t* trim_dev) {
    if (!ctx || !icp || !planes || nq < 0 || (nq > 0 && !q_dev) || !T_dev || !stats_dev || iters < 0 ||
        !(rmax >= 0.f))
        return PCP_ERR_ARG;
    PCP_TRY(check_stride(ctx, &q_stride));
    if (nq != icp_query_count(icp))
        return set_error(ctx, PCP_ERR_ARG, "%s: nq = %lld, the handle has %lld queries", who, (long long)nq,
                         (long long)icp_query_count(icp));
    if (planes->n != icp_target(icp)->n_in)
        return set_error(ctx, PCP_ERR_ARG, "%s: %lld plane records for a target of %lld points", who,
                         (long long)planes->n, (long long)icp_target(icp)->n_in);
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    const int nb = acc_blocks(nq);
    Tmp tmp(ctx);
    uint64_t* keys = nullptr;
    double* part = nullptr;
    uint32_t* work = nullptr;
    PCP_TRY(tmp.get(&keys, (size_t)nq));
    PCP_TRY(tmp.get(&part, (size_t)nb * kPAcc));
    uint64_t* rkeys = nullptr;
    if (trim) PCP_TRY(tmp.get(&work, trim_work_bytes() / sizeof(uint32_t)));
    if (trim && by_plane) PCP_TRY(tmp.get(&rkeys, (size_t)nq));
    for (int it = 0; it < iters; it++) {
        if (nq > 0) PCP_TRY(pcp_icp_keys_dev(ctx, icp, T_dev, rmax, 0, keys));
        if (trim && by_plane)
            PCP_TRY(trim_plane_async(ctx, T_dev, q_dev, q_stride, nq, keys, planes, trim[0], trim[1], trim[2], keys,
                                     trim_dev, rkeys, work));
        else if (trim)
            PCP_TRY(trim_keys_async(ctx, keys, nq, trim[0], trim[1], trim[2], keys, trim_dev, work));
        launch_acc(ctx, T_dev, q_dev, q_stride, nq, keys, planes, nb, part);
        hipLaunchKernelGGL(k_plane_sum_solve, dim3(1), dim3(kPB), 0, ctx->stream, (const double*)part, nb, T_dev,
                           stats_dev);
    }
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

}  // namespace
}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_icp_planes_create(pcp_ctx* ctx, const float* xyz, size_t t_stride, const float* nrm, size_t n_stride,
                          int64_t n, pcp_icp_planes** out) {
    if (!ctx || !out || n < 0 || (n > 0 && (!xyz || !nrm))) return PCP_ERR_ARG;
    *out = nullptr;
    if (n >= (int64_t)1 << 31) return set_error(ctx, PCP_ERR_ARG, "plane table supports < 2^31 points");
    PCP_TRY(check_stride(ctx, &t_stride));
    PCP_TRY(check_stride(ctx, &n_stride));
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    Tmp tmp(ctx);
    float4* rec = nullptr;
    uint32_t* counts = nullptr;
    PCP_TRY(tmp.get(&rec, 2 * (size_t)n));
    const int nb = acc_blocks(n);
    PCP_TRY(tmp.get(&counts, (size_t)nb));
    hipLaunchKernelGGL(k_planes_build, dim3(nb), dim3(kPB), 0, ctx->stream, xyz, t_stride / sizeof(float), nrm,
                       n_stride / sizeof(float), n, rec, counts);
    PCP_LAUNCH_CHECK(ctx);
    std::vector<uint32_t> h((size_t)nb);
    PCP_HIP(ctx, hipMemcpyAsync(h.data(), counts, (size_t)nb * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    PCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pcp_icp_planes* pl = new pcp_icp_planes();
    pl->owner = ctx;
    ctx_retain(ctx);
    pl->n = n;
    for (uint32_t c : h) pl->valid += c;
    pl->rec = tmp.release(rec);
    *out = pl;
    return PCP_OK;
}

int pcp_icp_planes_destroy(pcp_icp_planes* pl) {
    if (!pl) return PCP_ERR_ARG;
    if (pl->owner) (void)hipSetDevice(pl->owner->device);
    dfree(pl->owner, pl->rec);
    pcp_ctx* owner = pl->owner;
    delete pl;
    ctx_release(owner);
    return PCP_OK;
}

int64_t pcp_icp_planes_size(const pcp_icp_planes* pl) { return pl ? pl->n : -1; }
int64_t pcp_icp_planes_valid(const pcp_icp_planes* pl) { return pl ? pl->valid : -1; }

int pcp_icp_accumulate_plane(pcp_ctx* ctx, const double* T_dev, const float* q_dev, size_t q_stride, int64_t nq,
                             const uint64_t* keys_dev, const pcp_icp_planes* planes, double* acc_dev) {
    if (!ctx || !T_dev || nq < 0 || (nq > 0 && (!q_dev || !keys_dev)) || !planes || !acc_dev) return PCP_ERR_ARG;
    PCP_TRY(check_stride(ctx, &q_stride));
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    const int nb = acc_blocks(nq);
    Tmp tmp(ctx);
    double* part = nullptr;
    PCP_TRY(tmp.get(&part, (size_t)nb * kPAcc));
    launch_acc(ctx, T_dev, q_dev, q_stride, nq, keys_dev, planes, nb, part);
    hipLaunchKernelGGL(k_plane_sum, dim3(1), dim3(kPB), 0, ctx->stream, (const double*)part, nb, acc_dev);
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

int pcp_icp_solve_plane(const double acc[30], double dT[16]) {
    if (!acc || !dT) return PCP_ERR_ARG;
    return plane_solve(acc, dT);
}

int pcp_icp_solve_plane_dev(pcp_ctx* ctx, const double* acc_dev, double* T_dev, double* stats_dev) {
    if (!ctx || !acc_dev || !T_dev || !stats_dev) return PCP_ERR_ARG;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_plane_solve_dev, dim3(1), dim3(1), 0, ctx->stream, acc_dev, T_dev, stats_dev);
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

int pcp_icp_run_plane_dev(pcp_ctx* ctx, pcp_icp* icp, const pcp_icp_planes* planes, const float* q_dev,
                          size_t q_stride, int64_t nq, double* T_dev, float rmax, int iters, double* stats_dev) {
    return run_plane_loop(ctx, "pcp_icp_run_plane_dev", icp, planes, q_dev, q_stride, nq, T_dev, rmax, nullptr, false,
                          iters, stats_dev, nullptr);
}

int pcp_icp_run_plane_trimmed_dev(pcp_ctx* ctx, pcp_icp* icp, const pcp_icp_planes* planes, const float* q_dev,
                                  size_t q_stride, int64_t nq, double* T_dev, float rmax, float frac, float mult,
                                  float d_floor, int iters, double* stats_dev, uint64_t* trim_dev) {
    if (!trim_dev || !trim_args_ok(frac, mult, d_floor)) return PCP_ERR_ARG;
    const float trim[3] = {frac, mult, d_floor};
    return run_plane_loop(ctx, "pcp_icp_run_plane_trimmed_dev", icp, planes, q_dev, q_stride, nq, T_dev, rmax, trim,
                          false, iters, stats_dev, trim_dev);
}

// as pcp_icp_trim_keys, the argument checks before the stride's read nothing through ctx
int pcp_icp_trim_keys_plane(pcp_ctx* ctx, const double* T_dev, const float* q_dev, size_t q_stride, int64_t n,
                            const uint64_t* keys_dev, const pcp_icp_planes* planes, float frac, float mult,
                            float d_floor, uint64_t* keys_out_dev, uint64_t* trim_dev) {
    if (!ctx || !trim_dev || !T_dev || !planes || n < 0 || n >= (int64_t)1 << 31 ||
        (n > 0 && (!q_dev || !keys_dev || !keys_out_dev)) || !trim_args_ok(frac, mult, d_floor))
        return PCP_ERR_ARG;
    PCP_TRY(check_stride(ctx, &q_stride));
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    Tmp tmp(ctx);
    uint64_t* rkeys = nullptr;
    uint32_t* work = nullptr;
    PCP_TRY(tmp.get(&rkeys, (size_t)n));
    PCP_TRY(tmp.get(&work, trim_work_bytes() / sizeof(uint32_t)));
    return trim_plane_async(ctx, T_dev, q_dev, q_stride, n, keys_dev, planes, frac, mult, d_floor, keys_out_dev,
                            trim_dev, rkeys, work);
}

int pcp_icp_run_plane_rtrimmed_dev(pcp_ctx* ctx, pcp_icp* icp, const pcp_icp_planes* planes, const float* q_dev,
                                   size_t q_stride, int64_t nq, double* T_dev, float rmax, float frac, float mult,
                                   float d_floor, int iters, double* stats_dev, uint64_t* trim_dev) {
    if (!trim_dev || !trim_args_ok(frac, mult, d_floor)) return PCP_ERR_ARG;
    const float trim[3] = {frac, mult, d_floor};
    return run_plane_loop(ctx, "pcp_icp_run_plane_rtrimmed_dev", icp, planes, q_dev, q_stride, nq, T_dev, rmax, trim,
                          true, iters, stats_dev, trim_dev);
}

}  // extern "C"
