// Batched point-to-plane registration (include/pcp.h, I5): B query segments, B device poses, one
// fp32 target index and one plane table, three launches per iteration whatever B is.
//
// The single-pair handle (icp.hip) keeps one pose in scalar registers and a per-query neighbour
// cache that assumes it.  Here every 64-query chunk of the sorted layout belongs to one segment
// (segments are padded to whole chunks), so a wave reads its segment's pose through scalar loads
// and reduces its accumulators without a segment test per lane.  There is no cache: a query runs
// the exact row search of icp_search.hpp from the bound rmax^2, the arithmetic the single-pair
// kernels use, so the keys are theirs bit for bit.  Owned here: the padded chunk layout, the three
// kernels' loops and the per-segment sum; the pose cast, the key, the usable-pair test and the 30
// terms are icp_pair.hpp's, the solve icp_plane_solve.hpp's.
//
//   k_batch_search      one query per lane: pose chain, box_search, key -> keys[original index]
//   k_batch_acc         one chunk per wave: the 30 sums of the chunk's pairs -> partials[chunk]
//   k_batch_sum_solve   one block per segment: its chunks' partials in a fixed order, then thread
//                       0 runs solve_apply on the segment's pose
#include <vector>

#include "sortcfg.hpp"

#include "icp_batch.hpp"

namespace pcp {
namespace {

constexpr int kSumGroups = 8;     // k_batch_sum_solve: chunk c of a segment is summed by group c % 8

// ---- create: sort key (segment, cell key at the identity) and the caller index as payload
__global__ void __launch_bounds__(kBB) k_batch_sort_keys(GridDesc g, const float* q, size_t stride_f, int64_t n,
                                                         const int64_t* off, int nseg, unsigned cbits,
                                                         uint64_t* key, uint32_t* val) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        // the last segment s with off[s] <= i (empty segments before it share its offset)
        int lo = 0, hi = nseg;  // off[lo] <= i < off[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (off[mid] <= i) lo = mid;
            else hi = mid;
        }
        const float* p = q + (size_t)i * stride_f;
        const float x = p[0], y = p[1], z = p[2];
        const bool fin = isfinite(x) && isfinite(y) && isfinite(z);
        const uint32_t k = fin ? query_cell_key(g, x, y, z) : query_key_end(g);  // non-finite: last of its segment
        key[i] = ((uint64_t)lo << cbits) | k;
        val[i] = (uint32_t)i;
    }
}

// the padded layout: slot d of chunk c = d / 64 (segment s) holds sorted query off[s] + d - 64 *
// seg_chunk[s] when that is still inside the segment, else a pad
__global__ void __launch_bounds__(kBB) k_batch_gather(const float* q, size_t stride_f, const uint32_t* val,
                                                      const int64_t* off, const int32_t* chunk_seg,
                                                      const int32_t* seg_chunk, int64_t nslots, float4* rec) {
    for (int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; d < nslots; d += (int64_t)gridDim.x * blockDim.x) {
        const int s = chunk_seg[d >> 6];
        const int64_t p = off[s] + (d - 64 * (int64_t)seg_chunk[s]);
        float4 r = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
        if (p < off[s + 1]) {
            const uint32_t i = val[p];
            const float* v = q + (size_t)i * stride_f;
            r = make_float4(v[0], v[1], v[2], __int_as_float((int)i));
        }
        rec[d] = r;
    }
}

// ---- keys: wave w of the grid takes chunk w.  The search starts from the bound r2 with no
// winner, so a pair is accepted iff d2 <= r2 (Best::consider takes an equal d2 over "none").
__global__ void __launch_bounds__(kBB) k_batch_search(GridDesc g, const float4* tp, const float4* rec,
                                                      const int32_t* chunk_seg, int64_t nch, const double* T,
                                                      float r2, float mc, uint64_t* keys) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * kBW + (threadIdx.x >> 6);
    if (c >= nch) return;
    const int s = __builtin_amdgcn_readfirstlane(chunk_seg[c]);
    const Pose32 P = pose32(T + 16 * (int64_t)s);  // T is wave-uniform
    const float4 v = rec[c * 64 + lane];
    const int oi = __float_as_int(v.w);
    if (oi < 0) return;  // a pad slot
    uint64_t key = kNoKey;
    float x, y, z;
    xform(P, v, x, y, z);
    // a non-finite query or image has no correspondence (every d2 would be NaN)
    if (isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(x) && isfinite(y) && isfinite(z)) {
        Best b{r2, 0x7fffffff, 0u, 0.f, 0.f, 0.f};
        box_search<1>(g, tp, x, y, z, mc, b);
        if (b.bj != 0x7fffffff) key = key_make(b.bd, (uint32_t)b.bj);
    }
    keys[oi] = key;
}

// ---- accumulate: plane_pair's skip rule and plane_terms (icp_pair.hpp), as every plane consumer;
// the 30 terms of the chunk's 64 lanes are added by a butterfly, the same tree on every run
__global__ void __launch_bounds__(kBB) k_batch_acc(const float4* qrec, const int32_t* chunk_seg, int64_t nch,
                                                   const double* T, const uint64_t* keys, const float4* rec,
                                                   uint64_t nrec, double* partials) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * kBW + (threadIdx.x >> 6);
    if (c >= nch) return;
    const int s = __builtin_amdgcn_readfirstlane(chunk_seg[c]);
    const Pose32 P = pose32(T + 16 * (int64_t)s);  // T is wave-uniform
    const float4 v = qrec[c * 64 + lane];
    const int oi = __float_as_int(v.w);
    double term[kPAcc];
#pragma unroll
    for (int k = 0; k < kPAcc; k++) term[k] = 0.0;
    if (oi >= 0) {
        const uint64_t key = keys[oi];
        PlanePair pr;
        if (plane_pair(key, rec, nrec, pr)) {
            float x, y, z;
            xform(P, v, x, y, z);
            plane_terms(x, y, z, pr, key, term);
        }
    }
    double mine = 0.0;  // lane k keeps sum k
#pragma unroll
    for (int k = 0; k < kPAcc; k++) {
        double t = term[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
        mine = lane == k ? t : mine;
    }
    if (lane < kPAcc) partials[c * kPAcc + lane] = mine;
}

// ---- one block per segment: its chunks' partials summed in a fixed order (group g = 0..7 adds
// chunks g, g + 8, .. in chunk order, then the groups are added in order); row s of acc_out when
// given; thread 0 solves when T is given.  A segment without chunks sums to 30 zeros.
__global__ void __launch_bounds__(kBB) k_batch_sum_solve(const double* part, const int32_t* seg_chunk,
                                                         double* acc_out, double* T, double* stats) {
    __shared__ double sg[kSumGroups][kPAcc];
    __shared__ double acc[kPAcc];
    const int s = blockIdx.x, t = threadIdx.x;
    const int64_t c0 = seg_chunk[s], c1 = seg_chunk[s + 1];
    if (t < kSumGroups * kPAcc) {
        const int k = t % kPAcc, grp = t / kPAcc;
        double v = 0.0;
        for (int64_t c = c0 + grp; c < c1; c += kSumGroups) v += part[c * kPAcc + k];
        sg[grp][k] = v;
    }
    __syncthreads();
    if (t < kPAcc) {
        double v = 0.0;
        for (int grp = 0; grp < kSumGroups; grp++) v += sg[grp][t];
        acc[t] = v;
        if (acc_out) acc_out[(int64_t)s * kPAcc + t] = v;
    }
    __syncthreads();
    if (T && t == 0) {
        double a[kPAcc];
        for (int k = 0; k < kPAcc; k++) a[k] = acc[k];
        solve_apply(a, T + 16 * (int64_t)s, stats + 4 * (int64_t)s);
    }
}

// thread s: solve_apply on row s
__global__ void __launch_bounds__(64) k_batch_solve(const double* acc, int nseg, double* T, double* stats) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= nseg) return;
    double a[kPAcc];
    for (int k = 0; k < kPAcc; k++) a[k] = acc[(int64_t)s * kPAcc + k];
    solve_apply(a, T + 16 * (int64_t)s, stats + 4 * (int64_t)s);
}

}  // namespace

void batch_launch_search(pcp_ctx* ctx, const pcp_icp_batch* b, const double* T_dev, float rmax, uint64_t* keys) {
    const pcp_index* tg = b->target;
    hipLaunchKernelGGL(k_batch_search, dim3(chunk_grid(b->nch)), dim3(kBB), 0, ctx->stream, tg->g,
                       (const float4*)tg->pts, (const float4*)b->rec, (const int32_t*)b->chunk_seg, b->nch, T_dev,
                       rmax * rmax, search_margin(tg->g), keys);
}

void batch_launch_acc(pcp_ctx* ctx, const pcp_icp_batch* b, const double* T_dev, const uint64_t* keys,
                      const pcp_icp_planes* pl, double* part) {
    hipLaunchKernelGGL(k_batch_acc, dim3(chunk_grid(b->nch)), dim3(kBB), 0, ctx->stream, (const float4*)b->rec,
                       (const int32_t*)b->chunk_seg, b->nch, T_dev, keys, (const float4*)pl->rec, (uint64_t)pl->n,
                       part);
}

void batch_launch_sum_solve(pcp_ctx* ctx, const pcp_icp_batch* b, const double* part, double* acc_out, double* T,
                            double* stats) {
    hipLaunchKernelGGL(k_batch_sum_solve, dim3(b->nseg), dim3(kBB), 0, ctx->stream, part,
                       (const int32_t*)b->seg_chunk, acc_out, T, stats);
}

}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_icp_batch_destroy(pcp_icp_batch* b) {
    if (!b) return PCP_ERR_ARG;
    pcp_ctx* owner = b->owner;
    if (owner) (void)hipSetDevice(owner->device);
    dfree(owner, b->rec);
    dfree(owner, b->chunk_seg);
    dfree(owner, b->seg_chunk);
    delete b;
    ctx_release(owner);
    return PCP_OK;
}

int pcp_icp_batch_create(pcp_ctx* ctx, const pcp_index* target, const float* q_dev, size_t q_stride, int64_t nq,
                         const int64_t* seg_offsets, int nseg, pcp_icp_batch** out) {
    if (!ctx || !target || !out || !seg_offsets || nq < 0 || (nq > 0 && !q_dev)) return PCP_ERR_ARG;
    *out = nullptr;
    if (nseg < 0 || nseg > 65535) return set_error(ctx, PCP_ERR_ARG, "pcp_icp_batch_create: 0 <= nseg <= 65535");
    if (nq >= (int64_t)1 << 31) return set_error(ctx, PCP_ERR_ARG, "pcp_icp_batch_create supports < 2^31 queries");
    if (target->is_f64 || target->is_h16)
        return set_error(ctx, PCP_ERR_ARG, "ICP target must be an fp32 index");
    PCP_TRY(check_stride(ctx, &q_stride));
    if (seg_offsets[0] != 0 || seg_offsets[nseg] != nq)
        return set_error(ctx, PCP_ERR_ARG, "pcp_icp_batch_create: segment offsets must start at 0 and end at nq");
    for (int s = 0; s < nseg; s++)
        if (seg_offsets[s + 1] < seg_offsets[s])
            return set_error(ctx, PCP_ERR_ARG, "pcp_icp_batch_create: segment offsets must not decrease");
    const GridDesc& g = target->g;
    if (int rc = pcp_icp_check_sizes(target->n, nq))
        return set_error(ctx, rc, "ICP target must have < 2^28 - 1 points (32-bit record offsets)");
    if (g.nbricks * 64 >= ((int64_t)1 << 32) ||
        qbricks(g, 0) * qbricks(g, 1) * qbricks(g, 2) * kQBrick * kQBrick * kQBrick >= ((int64_t)1 << 32))
        return set_error(ctx, PCP_ERR_UNSUPPORTED, "ICP target grid too large for 32-bit cell keys");
    PCP_HIP(ctx, hipSetDevice(ctx->device));

    // the padded layout, on the host: segment s owns chunks [seg_chunk[s], seg_chunk[s + 1])
    std::vector<int32_t> seg_chunk((size_t)nseg + 1, 0);
    int64_t nch = 0;
    for (int s = 0; s < nseg; s++) {
        seg_chunk[s] = (int32_t)nch;
        nch += (seg_offsets[s + 1] - seg_offsets[s] + 63) / 64;
    }
    seg_chunk[nseg] = (int32_t)nch;
    std::vector<int32_t> chunk_seg((size_t)nch);
    for (int s = 0; s < nseg; s++)
        for (int64_t c = seg_chunk[s]; c < seg_chunk[s + 1]; c++) chunk_seg[(size_t)c] = s;

    Tmp tmp(ctx);  // the sort's buffers, and the handle's until it owns them
    float4* rec = nullptr;
    int32_t *d_chunk_seg = nullptr, *d_seg_chunk = nullptr;
    int64_t* d_off = nullptr;
    PCP_TRY(tmp.get(&rec, (size_t)nch * 64));
    PCP_TRY(tmp.get(&d_chunk_seg, (size_t)nch));
    PCP_TRY(tmp.get(&d_seg_chunk, (size_t)nseg + 1));
    PCP_TRY(tmp.get(&d_off, (size_t)nseg + 1));
    PCP_HIP(ctx, hipMemcpyAsync(d_seg_chunk, seg_chunk.data(), ((size_t)nseg + 1) * sizeof(int32_t),
                                hipMemcpyHostToDevice, ctx->stream));
    PCP_HIP(ctx, hipMemcpyAsync(d_off, seg_offsets, ((size_t)nseg + 1) * sizeof(int64_t), hipMemcpyHostToDevice,
                                ctx->stream));
    if (nch > 0)
        PCP_HIP(ctx, hipMemcpyAsync(d_chunk_seg, chunk_seg.data(), (size_t)nch * sizeof(int32_t),
                                    hipMemcpyHostToDevice, ctx->stream));
    if (nq > 0) {
        uint64_t *k0 = nullptr, *k1 = nullptr;
        uint32_t *v0 = nullptr, *v1 = nullptr;
        PCP_TRY(tmp.get(&k0, (size_t)nq));
        PCP_TRY(tmp.get(&k1, (size_t)nq));
        PCP_TRY(tmp.get(&v0, (size_t)nq));
        PCP_TRY(tmp.get(&v1, (size_t)nq));
        unsigned cbits = 1, sbits = 0;  // cell keys are in [0, query_key_end], segments in [0, nseg)
        while (cbits < 32 && ((uint64_t)1 << cbits) <= (uint64_t)query_key_end(g)) cbits++;
        while (((int64_t)1 << sbits) < nseg) sbits++;
        const size_t stride_f = q_stride / sizeof(float);
        hipLaunchKernelGGL(k_batch_sort_keys, dim3(grid_for(nq, kBB, 8192)), dim3(kBB), 0, ctx->stream, g, q_dev,
                           stride_f, nq, (const int64_t*)d_off, nseg, cbits, k0, v0);
        PCP_TRY(sort_pairs<RecSortConfig>(tmp, k0, k1, v0, v1, (size_t)nq, 0u, cbits + sbits));
        hipLaunchKernelGGL(k_batch_gather, dim3(grid_for(nch * 64, kBB, 8192)), dim3(kBB), 0, ctx->stream, q_dev,
                           stride_f, (const uint32_t*)v1, (const int64_t*)d_off, (const int32_t*)d_chunk_seg,
                           (const int32_t*)d_seg_chunk, nch * 64, rec);
        PCP_LAUNCH_CHECK(ctx);
    }
    // the host arrays above are read by the copies until here
    PCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pcp_icp_batch* b = new pcp_icp_batch();
    b->owner = ctx;
    ctx_retain(ctx);
    b->target = target;
    b->nq = nq;
    b->nseg = nseg;
    b->nch = nch;
    b->rec = tmp.release(rec);
    b->chunk_seg = tmp.release(d_chunk_seg);
    b->seg_chunk = tmp.release(d_seg_chunk);
    *out = b;
    return PCP_OK;
}

int64_t pcp_icp_batch_queries(const pcp_icp_batch* b) { return b ? b->nq : -1; }
int pcp_icp_batch_segments(const pcp_icp_batch* b) { return b ? b->nseg : -1; }

int pcp_icp_batch_keys_dev(pcp_ctx* ctx, pcp_icp_batch* b, const double* T_dev, float rmax, uint64_t* keys_dev) {
    if (!ctx || !b || !(rmax >= 0.f) || (b->nseg > 0 && !T_dev) || (b->nq > 0 && !keys_dev)) return PCP_ERR_ARG;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    if (b->nch == 0) return PCP_OK;
    batch_launch_search(ctx, b, T_dev, rmax, keys_dev);
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

int pcp_icp_batch_accumulate_plane(pcp_ctx* ctx, pcp_icp_batch* b, const double* T_dev, const uint64_t* keys_dev,
                                   const pcp_icp_planes* planes, double* acc_dev) {
    if (!ctx || !b || !planes || (b->nseg > 0 && (!T_dev || !acc_dev)) || (b->nq > 0 && !keys_dev))
        return PCP_ERR_ARG;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    if (b->nseg == 0) return PCP_OK;
    Tmp tmp(ctx);
    double* part = nullptr;
    PCP_TRY(tmp.get(&part, (size_t)b->nch * kPAcc));
    if (b->nch > 0) batch_launch_acc(ctx, b, T_dev, keys_dev, planes, part);
    batch_launch_sum_solve(ctx, b, part, acc_dev, nullptr, nullptr);
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

int pcp_icp_batch_solve_plane_dev(pcp_ctx* ctx, const double* acc_dev, int nseg, double* T_dev, double* stats_dev) {
    if (!ctx || nseg < 0 || nseg > 65535 || (nseg > 0 && (!acc_dev || !T_dev || !stats_dev))) return PCP_ERR_ARG;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    if (nseg == 0) return PCP_OK;
    hipLaunchKernelGGL(k_batch_solve, dim3((nseg + 63) / 64), dim3(64), 0, ctx->stream, acc_dev, nseg, T_dev,
                       stats_dev);
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

int pcp_icp_batch_run_plane_dev(pcp_ctx* ctx, pcp_icp_batch* b, const pcp_icp_planes* planes, double* T_dev,
                                float rmax, int iters, double* stats_dev) {
    if (!ctx || !b || !planes || iters < 0 || !(rmax >= 0.f) || (b->nseg > 0 && (!T_dev || !stats_dev)))
        return PCP_ERR_ARG;
    if (planes->n != b->target->n_in)
        return set_error(ctx, PCP_ERR_ARG, "pcp_icp_batch_run_plane_dev: %lld plane records for a target of %lld points",
                         (long long)planes->n, (long long)b->target->n_in);
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    if (b->nseg == 0) return PCP_OK;
    Tmp tmp(ctx);
    uint64_t* keys = nullptr;
    double* part = nullptr;
    PCP_TRY(tmp.get(&keys, (size_t)b->nq));
    PCP_TRY(tmp.get(&part, (size_t)b->nch * kPAcc));
    for (int it = 0; it < iters; it++) {
        if (b->nch > 0) {
            batch_launch_search(ctx, b, T_dev, rmax, keys);
            batch_launch_acc(ctx, b, T_dev, keys, planes, part);
        }
        batch_launch_sum_solve(ctx, b, part, nullptr, T_dev, stats_dev);
    }
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

}  // extern "C"
