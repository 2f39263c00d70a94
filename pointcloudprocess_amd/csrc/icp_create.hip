// Making and unmaking an ICP handle: the query sort of the create path, the handle's buffers and
// grids, its options.
//
// Owned here: QuerySort and its kernels (k_query_keys, k_split_queries, k_first_at_least), icp_alloc
// and icp_make, pcp_icp_check_sizes / create / create_with_target / set_options / destroy,
// icp_graph_drop (also called by icp.hip's re-capture), and the two facts of a handle that other
// files may ask for (icp_target, icp_query_count).  The handle is icp_handle.hpp's; the cell key the
// queries are sorted by is icp_search.hpp's.
#include "sortcfg.hpp"

#include "icp_handle.hpp"

namespace pcp {
namespace {

// ---- query order (pcp_icp_create): queries sorted once by target-grid cell in brick-major
// order (8x8x8-cell bricks, cell order inside a brick -- brick order alone measured 5 % slower
// searches; stable, so input order inside a cell), carried as float4 {x, y, z, bits(index)}
// through the radix sort; non-finite queries get key query_key_end (after every cell) and
// are dropped.
__global__ void k_query_keys(GridDesc g, const float* q, size_t stride_f, int64_t n, uint32_t* key, float4* rec) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float* p = q + (size_t)i * stride_f;
        const float x = p[0], y = p[1], z = p[2];
        const bool fin = isfinite(x) && isfinite(y) && isfinite(z);
        uint32_t k = query_key_end(g);  // past every brick: non-finite queries sort last
        if (fin) k = query_cell_key(g, x, y, z);
        key[i] = k;
        rec[i] = make_float4(x, y, z, __int_as_float((int)i));
    }
}

// the sorted {x, y, z, bits(index)} records -> 12-byte xyz + index arrays
__global__ void k_split_queries(const float4* qs, int64_t n, QXyz* q, int32_t* qi) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 v = qs[i];
        q[i] = QXyz{v.x, v.y, v.z};
        qi[i] = __float_as_int(v.w);
    }
}

// number of finite queries = first position of the sentinel key in the sorted keys
// (a single-address atomic per wave costs ~9 ms at 50M queries; this costs nothing)
__global__ void k_first_at_least(const uint32_t* sorted, int64_t n, uint32_t key, unsigned long long* out) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (sorted[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    *out = (unsigned long long)lo;
}

}  // namespace
}  // namespace pcp

extern "C" {

int pcp_icp_check_sizes(int64_t n_target, int64_t nq) {
    if (n_target < 0 || nq < 0) return PCP_ERR_ARG;
    if (nq >= ((int64_t)1 << 31)) return PCP_ERR_ARG;
    // ld16(): 32-bit byte offsets into the fp32 target (n_target records + the far sentinel)
    if (n_target + 1 >= ((int64_t)1 << 28)) return PCP_ERR_CAPACITY;
    return PCP_OK;
}

}  // extern "C"

namespace pcp {
namespace {

// the query sort of an ICP handle between its launch and its completion: keys of the octant-block
// bricks of the target grid, a stable radix sort with the 16-byte records as payload, the count
// of finite queries
struct QuerySort {
    Tmp blocks;
    uint32_t *k0 = nullptr, *k1 = nullptr;
    float4 *r0 = nullptr, *qs = nullptr;
    unsigned long long* d_cnt = nullptr;
    char* tmp = nullptr;
    hipEvent_t done = nullptr;
    int64_t nq = 0;
    explicit QuerySort(pcp_ctx* ctx) : blocks(ctx) {}
    // The blocks go back to the cache in ctx->stream's order, so only once that stream has waited
    // for `done` (or the side stream was synchronised after a failure): every path of the two
    // create functions calls this there, and none leaves the blocks to the guard's scope exit.
    void release() { blocks.free_all(); }
};

int icp_check_grid(pcp_ctx* ctx, const GridDesc& g, int64_t n_target, int64_t nq) {
    if (int rc = pcp_icp_check_sizes(n_target, nq))
        return set_error(ctx, rc, rc == PCP_ERR_CAPACITY ? "ICP target must have < 2^28 - 1 points (32-bit record offsets)"
                                                         : "ICP supports < 2^31 queries");
    if (g.nbricks * 64 >= ((int64_t)1 << 32) ||
        qbricks(g, 0) * qbricks(g, 1) * qbricks(g, 2) * kQBrick * kQBrick * kQBrick >= ((int64_t)1 << 32))
        return set_error(ctx, PCP_ERR_UNSUPPORTED, "ICP target grid too large for 32-bit cell keys");
    return PCP_OK;
}

// enqueue the query sort on `st` (after everything enqueued so far on ctx->stream); `s.done` is
// recorded on `st` when it is complete
int qsort_launch(pcp_ctx* ctx, hipStream_t st, const GridDesc& g, const float* q, size_t q_stride, int64_t nq,
                 QuerySort& s) {
    s.nq = nq;
    PCP_TRY(s.blocks.get(&s.k0, nq));
    PCP_TRY(s.blocks.get(&s.k1, nq));
    PCP_TRY(s.blocks.get(&s.r0, nq));
    PCP_TRY(s.blocks.get(&s.qs, nq + 1));
    PCP_TRY(s.blocks.get(&s.d_cnt, 1));
    PCP_HIP(ctx, s.blocks.event(&s.done));
    unsigned bits = 1;  // keys are in [0, query_key_end]
    while (bits < 32 && ((uint64_t)1 << bits) <= (uint64_t)query_key_end(g)) bits++;
    size_t tb = 0;
    if (nq > 0) {
        PCP_HIP(ctx, rocprim::radix_sort_pairs<RecSortConfig>(nullptr, tb, s.k0, s.k1, s.r0, s.qs, (size_t)nq, 0u, bits, st));
        PCP_TRY(s.blocks.get(&s.tmp, tb));
    }
    // Every block the side stream uses is allocated above, before `go` is recorded: a block the
    // context cache hands out after that point could still be in use by main-stream work the side
    // stream does not wait for.
    if (st != ctx->stream) {  // the side stream starts after the main stream's work so far
        hipEvent_t go = nullptr;
        PCP_HIP(ctx, event_get(ctx, &go));
        hipError_t e = hipEventRecord(go, ctx->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, go, 0);
        event_put(ctx, go);  // (reused only by a later record on ctx->stream: stream-ordered)
        if (e != hipSuccess) return hip_fail(ctx, e, "query sort stream order", __FILE__, __LINE__);
    }
    PCP_HIP(ctx, hipMemsetAsync(s.d_cnt, 0, sizeof(unsigned long long), st));
    if (nq > 0) {
        hipLaunchKernelGGL(k_query_keys, dim3(grid_for(nq, 256)), dim3(256), 0, st, g, q, q_stride / sizeof(float), nq,
                           s.k0, s.r0);
        PCP_HIP(ctx, rocprim::radix_sort_pairs<RecSortConfig>(s.tmp, tb, s.k0, s.k1, s.r0, s.qs, (size_t)nq, 0u, bits, st));
        hipLaunchKernelGGL(k_first_at_least, dim3(1), dim3(1), 0, st, s.k1, nq, query_key_end(g), s.d_cnt);
    }
    PCP_HIP(ctx, hipGetLastError());
    PCP_HIP(ctx, hipEventRecord(s.done, st));
    return PCP_OK;
}

// the sorted records -> 12-byte xyz + original indices, on ctx->stream after the sort
int qsort_finish(pcp_ctx* ctx, Tmp& tmp, QuerySort& s, QXyz** q3, int32_t** qi, int64_t* nfin) {
    PCP_HIP(ctx, hipStreamWaitEvent(ctx->stream, s.done, 0));
    unsigned long long hc = 0;
    PCP_HIP(ctx, hipMemcpyAsync(&hc, s.d_cnt, sizeof(hc), hipMemcpyDeviceToHost, ctx->stream));
    PCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *nfin = (int64_t)hc;
    PCP_TRY(tmp.get(q3, s.nq + 1));
    PCP_TRY(tmp.get(qi, s.nq + 1));
    if (*nfin > 0)
        hipLaunchKernelGGL(k_split_queries, dim3(grid_for(*nfin, 256)), dim3(256), 0, ctx->stream,
                           (const float4*)s.qs, *nfin, *q3, *qi);
    PCP_HIP(ctx, hipGetLastError());
    return PCP_OK;
}

// The handle's grids, then its blocks and events, all through icp->mem: a failure at any point
// leaves them to pcp_icp_destroy.  The order and the sizes of the requests are part of the create
// time: the context cache serves them from the blocks the query sort has just released.
int icp_alloc(pcp_icp* icp) {
    pcp_ctx* ctx = icp->owner;
    Tmp& mem = icp->mem;
    int dev_cus = 256;  // one attribute query (the whole hipDeviceProp_t costs ~0.1 ms per create)
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) == hipSuccess && cus > 0)
        dev_cus = cus;
    const int64_t want = (icp->nq + kIcpBlock - 1) / kIcpBlock;
    icp->nb_fast = (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)dev_cus * PCP_OCT_WAVES));
    icp->nb_fast_l = (int)std::max<int64_t>(1, std::min<int64_t>(icp->nb_fast, (int64_t)dev_cus * PCP_OCT_WAVES_LIST));
    icp->nb_ring = (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)dev_cus * PCP_RING_WAVES));
    const int64_t nwaves = (int64_t)icp->nb_fast * (kIcpBlock / 64);
    const int64_t nwaves_l = (int64_t)icp->nb_fast_l * (kIcpBlock / 64);  // the smaller grid: larger segments
    const int64_t nchunks64 = (icp->nq + 63) / 64;
    icp->fb_seg = ((nchunks64 + nwaves_l - 1) / nwaves_l) * 64;
    icp->nb_ver = (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)dev_cus * PCP_VER_WAVES));
    const int64_t nwaves_v = (int64_t)icp->nb_ver * (kIcpBlock / 64);
    icp->sv_seg = ((nchunks64 + nwaves_v - 1) / nwaves_v) * 64;  // contiguous ranges: <= this per wave
    icp->nseg_v = nwaves_v;
    PCP_TRY(mem.get(&icp->partials, (size_t)(icp->nb_ver + icp->nb_fast + icp->nb_ring) * kAcc));
    PCP_TRY(mem.get(&icp->acc, kAcc));
    PCP_TRY(mem.get(&icp->pilot_acc, kAcc));
    PCP_TRY(mem.get(&icp->pose_dev, 1));
    // 12-byte cache records when every position (and the far sentinel) fits 26 bits
    icp->narrow = icp->target->n + 1 < (int64_t)kPos26;
    const int rw = icp->narrow ? 3 : 4;  // words per record
    PCP_TRY(mem.get(&icp->cand, (size_t)(icp->nq + 1) * rw));
    PCP_TRY(mem.get(&icp->pose_hist, kHist * 12));
    // the first launch over a dense grid (the octant pass over every query) writes every cache
    // record before any pass reads one: only the sentinel record needs its value then (an 800 MB
    // memset at 50M queries, ~0.1 ms of the pre-iteration span, otherwise).  An empty record has
    // no positions and D = 0 (wide: NaN), so it is never settled from.
    const bool cand_all = !icp->target->g.dense;
    const int64_t r0 = cand_all ? 0 : icp->nq, nr = cand_all ? icp->nq + 1 : 1;
    if (icp->narrow)
        PCP_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)(icp->cand + r0 * rw), (int)kPos26, (size_t)(nr * rw), ctx->stream));
    else
        PCP_HIP(ctx, hipMemsetAsync(icp->cand + r0 * rw, 0xff, (size_t)nr * 16, ctx->stream));
    PCP_HIP(ctx, hipMemsetAsync(icp->pose_hist, 0, kHist * 12 * sizeof(float), ctx->stream));
    PCP_HIP(ctx, hipMemsetAsync(icp->pose_dev, 0, sizeof(PoseBlock), ctx->stream));
    PCP_TRY(mem.get(&icp->sv, (size_t)icp->nseg_v * icp->sv_seg + 1));
    PCP_TRY(mem.get(&icp->sv_count, (size_t)icp->nseg_v));
    PCP_TRY(mem.get(&icp->sv_off, (size_t)icp->nseg_v + 1));
    PCP_TRY(mem.get(&icp->svc, icp->nq + 1));
    const int64_t fb_cap = std::max<int64_t>(nwaves * icp->fb_seg, icp->nq);
    PCP_TRY(mem.get(&icp->fb, (size_t)fb_cap + 1));
    PCP_TRY(mem.get(&icp->fb_count, (size_t)nwaves));
    PCP_TRY(mem.get(&icp->fb_off, (size_t)nwaves + 1));
    PCP_TRY(mem.get(&icp->fbc, icp->nq + 1));
    for (hipEvent_t* ev : {&icp->ev0, &icp->ev1, &icp->ev_mid, &icp->ev_ver}) PCP_HIP(ctx, mem.event(ev));
    return PCP_OK;
}

// the handle over sorted queries (q3, qi: blocks of ctx's cache, the handle's from here on)
int icp_make(pcp_ctx* ctx, const pcp_index* target, QXyz* q3, int32_t* qi, int64_t nfin, int64_t nq, pcp_icp** out) {
    pcp_icp* icp = new pcp_icp(ctx);
    ctx_retain(ctx);
    icp->target = target;
    icp->nq = nfin;
    icp->nq_in = nq;
    icp->q = icp->mem.adopt(q3);
    icp->qidx = icp->mem.adopt(qi);
    if (const int rc = icp_alloc(icp)) {
        pcp_icp_destroy(icp);
        return rc;
    }
    *out = icp;
    return PCP_OK;
}

}  // namespace

// common.hpp: the handle's facts the point-to-plane loop (icp_plane.hip) checks its arguments by
const pcp_index* icp_target(const pcp_icp* icp) { return icp->target; }
int64_t icp_query_count(const pcp_icp* icp) { return icp->nq_in; }

void icp_graph_drop(pcp_icp* icp) {
    if (!icp->gexec) return;
    (void)hipSetDevice(icp->owner->device);
    (void)hipDeviceSynchronize();
    (void)hipGraphExecDestroy(icp->gexec);
    icp->gexec = nullptr;
}

}  // namespace pcp

extern "C" {

int pcp_icp_create(pcp_ctx* ctx, const pcp_index* target, const float* q, size_t q_stride, int64_t nq,
                   pcp_icp** out) {
    if (!ctx || !target || !out || nq < 0 || (nq > 0 && !q)) return PCP_ERR_ARG;
    if (target->is_f64) return pcp::set_error(ctx, PCP_ERR_ARG, "ICP target must be an fp32 index");
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    *out = nullptr;
    if (q_stride == 0) q_stride = 3 * sizeof(float);
    if (q_stride % sizeof(float)) return pcp::set_error(ctx, PCP_ERR_ARG, "query stride must be whole floats");
    PCP_TRY(pcp::icp_check_grid(ctx, target->g, target->n, nq));
    pcp::Tmp tmp(ctx);  // q3, qi until the handle owns them
    pcp::QuerySort s(ctx);
    pcp::QXyz* q3 = nullptr;
    int32_t* qi = nullptr;
    int64_t nfin = 0;
    int rc = pcp::qsort_launch(ctx, ctx->stream, target->g, q, q_stride, nq, s);
    if (!rc) rc = pcp::qsort_finish(ctx, tmp, s, &q3, &qi, &nfin);
    s.release();  // early: the handle's buffers are served from these blocks
    if (rc) return rc;
    return pcp::icp_make(ctx, target, tmp.release(q3), tmp.release(qi), nfin, nq, out);
}

int pcp_icp_create_with_target(pcp_ctx* ctx, const float* target_xyz, size_t t_stride, int64_t n_target,
                               double cell_size, const float* q, size_t q_stride, int64_t nq, pcp_index** index_out,
                               pcp_icp** icp_out) {
    if (!ctx || !index_out || !icp_out || nq < 0 || (nq > 0 && !q) || n_target < 0 || (n_target > 0 && !target_xyz))
        return PCP_ERR_ARG;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    *index_out = nullptr;
    *icp_out = nullptr;
    if (q_stride == 0) q_stride = 3 * sizeof(float);
    if (q_stride % sizeof(float)) return pcp::set_error(ctx, PCP_ERR_ARG, "query stride must be whole floats");
    // the query sort needs only the target grid's geometry: it runs on the side stream while the
    // target's cell sort runs on the main stream (two independent radix sorts overlapped)
    pcp::Tmp tmp(ctx);  // q3, qi until the handle owns them
    pcp::QuerySort s(ctx);
    bool launched = false;
    const pcp::GeomHook hook = [&](const pcp::GridDesc& g) -> int {
        PCP_TRY(pcp::icp_check_grid(ctx, g, n_target, nq));
        hipStream_t side = nullptr;
        PCP_TRY(pcp::side_stream(ctx, &side));
        launched = true;
        return pcp::qsort_launch(ctx, side, g, q, q_stride, nq, s);
    };
    pcp_index* ix = nullptr;
    int rc = pcp::index_build_f32_hooked(ctx, target_xyz, t_stride, n_target, cell_size, &ix, hook);
    pcp::QXyz* q3 = nullptr;
    int32_t* qi = nullptr;
    int64_t nfin = 0;
    if (!rc && !launched) rc = pcp::qsort_launch(ctx, ctx->stream, ix->g, q, q_stride, nq, s);
    if (!rc) rc = pcp::qsort_finish(ctx, tmp, s, &q3, &qi, &nfin);
    if (rc && launched) (void)hipStreamSynchronize(ctx->side);  // the side stream's work is over
    s.release();  // early: the handle's buffers are served from these blocks
    if (!rc) rc = pcp::icp_make(ctx, ix, tmp.release(q3), tmp.release(qi), nfin, nq, icp_out);
    if (rc) {
        if (ix) pcp_index_destroy(ix);
        return rc;
    }
    *index_out = ix;
    return PCP_OK;
}

int pcp_icp_set_options(pcp_icp* icp, int oct_lanes_first, int oct_lanes_list, int ring_lanes, int ablate) {
    if (!icp) return PCP_ERR_ARG;
    auto lanes = [](int v) { return v == 0 || v == 1 || v == 2 || v == 4 || v == 8; };
    pcp_ctx* ctx = icp->owner;
    // every check and allocation first: a failed call leaves the handle as it was
    if (!lanes(oct_lanes_first) || !lanes(oct_lanes_list) || !lanes(ring_lanes) || ablate < 0)
        return pcp::set_error(ctx, PCP_ERR_ARG, "pcp_icp_set_options: lanes must be 0, 1, 2, 4 or 8; ablate >= 0");
    const bool widen = (ablate & PCP_ICP_OPT_WIDE_CACHE) && icp->narrow;
    if (widen && icp->launches > 0)
        return pcp::set_error(ctx, PCP_ERR_ARG, "PCP_ICP_OPT_WIDE_CACHE only before the handle's first launch");
    if (widen) {  // re-create the records in the 16-byte form
        uint32_t* w = nullptr;
        PCP_TRY(icp->mem.get(&w, (size_t)(icp->nq + 1) * 4));
        if (hipMemsetAsync(w, 0xff, (size_t)(icp->nq + 1) * 16, ctx->stream) != hipSuccess) {
            icp->mem.free(w);
            return pcp::set_error(ctx, PCP_ERR_HIP, "pcp_icp_set_options: memset");
        }
        icp->mem.free(icp->cand);
        icp->cand = w;
        icp->narrow = false;
    }
    pcp::icp_graph_drop(icp);  // captured with the old lanes / flags
    icp->oct_g_first = oct_lanes_first ? oct_lanes_first : 1;
    icp->oct_g_list = oct_lanes_list;
    icp->ring_g = ring_lanes;
    icp->dbg = ablate & ~(PCP_ICP_OPT_WIDE_CACHE | PCP_ICP_OPT_GRAPH | PCP_ICP_OPT_NO_LOOKAHEAD |
                          PCP_ICP_OPT_NO_PILOT | PCP_ICP_OPT_PILOT_ALWAYS);
    icp->graph = (ablate & PCP_ICP_OPT_GRAPH) != 0;
    icp->no_look = (ablate & PCP_ICP_OPT_NO_LOOKAHEAD) != 0;
    icp->no_pilot = (ablate & PCP_ICP_OPT_NO_PILOT) != 0;
    icp->pilot_always = (ablate & PCP_ICP_OPT_PILOT_ALWAYS) != 0;
    return PCP_OK;
}

int pcp_icp_destroy(pcp_icp* icp) {
    if (!icp) return PCP_ERR_ARG;
    pcp_ctx* owner = icp->owner;
    (void)hipSetDevice(owner->device);
    pcp::icp_graph_drop(icp);
    delete icp;  // icp->mem gives its blocks and events back to the owner
    pcp::ctx_release(owner);
    return PCP_OK;
}

}  // extern "C"
