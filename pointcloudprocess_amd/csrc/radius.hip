// Exact fp64 radius search over the uniform-grid index: the FLANN contract of
// KdTreeFLANN::radiusSearch (kd_tree.h:863-903) as a count pass and a fill pass over CSR rows.
//
// One lane per query; d2 is FLANN L2_Simple<double> with contraction off, so the strict d2 < r2
// test and the (d2, j) row order are the reference's bit for bit.  The near pass walks the cell
// rings (grid.hpp) and defers a query whose radius reaches past them to the far pass, the
// brick-level ring search over the deferred list; a radius that reaches past the rings for every
// query goes straight to the far pass.
#include "knn_search.hpp"

namespace pcp {
namespace {

// Both kernels run as the near pass (FAR = false: every query, cell rings only) and as the far
// pass (FAR = true: the brick-level search, over the deferred list, or over every query when the
// list is null).  Deferred queries are few but each is expensive, so the far pass gives every one
// its own wave (lane 0) to spread them over all CUs instead of packing them into a few waves.
template <bool FAR>
__device__ __forceinline__ int64_t work_count(const FarList& f, int64_t n) {
    if (FAR && f.list) return (threadIdx.x & 63) ? 0 : (int64_t)*f.count * 64;
    return n;
}
template <bool FAR>
__device__ __forceinline__ int64_t work_item(const FarList& f, int64_t w) {
    return (FAR && f.list) ? (int64_t)f.list[w >> 6] : w;
}

// K4 count pass: #points with d2 < r2 (strict, FLANN RadiusResultSet), truncated to max_nn
struct CountVisitor {
    const double4* pts;
    double qx, qy, qz, r2, b;
    uint32_t cnt;
    __device__ double bound() const { return b; }
    __device__ void visit(uint32_t s, uint32_t e) {
        uint32_t t = s;
        for (; t + 4 <= e; t += 4) {
            const double4 p0 = pts[t], p1 = pts[t + 1], p2 = pts[t + 2], p3 = pts[t + 3];
            cnt += (l2_simple(qx, qy, qz, p0) < r2 ? 1u : 0u) + (l2_simple(qx, qy, qz, p1) < r2 ? 1u : 0u) +
                   (l2_simple(qx, qy, qz, p2) < r2 ? 1u : 0u) + (l2_simple(qx, qy, qz, p3) < r2 ? 1u : 0u);
        }
        for (; t < e; t++) cnt += l2_simple(qx, qy, qz, pts[t]) < r2 ? 1u : 0u;
    }
};

template <bool FAR>
__global__ __launch_bounds__(kB) void k_radius_count(GridDesc g, const double4* pts, const double* q, size_t qstride,
                                                     int64_t nq, double r2, uint32_t cap, double mc, int32_t* ocnt,
                                                     FarList far) {
    const int64_t nw = work_count<FAR>(far, nq);
    for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < nw; w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = work_item<FAR>(far, w);
        const double* qp = qptr(q, qstride, i);
        CountVisitor v{pts, qp[0], qp[1], qp[2], r2, r2 * (1.0 + 1e-12), 0u};
        if (finite3(v.qx, v.qy, v.qz) && !ring_search<double, CountVisitor, FAR>(g, v.qx, v.qy, v.qz, mc, v)) {
            defer(far, i);
            continue;
        }
        ocnt[i] = (int32_t)(v.cnt < cap ? v.cnt : cap);
    }
}

// K4 fill pass.  A row that max_nn does not truncate (m < cap) receives its points in
// visiting order (k_sort_rows orders it afterwards); a possibly truncated row (m == cap)
// keeps the m best found so far sorted by (d2, j) by insertion.
struct FillVisitor {
    const double4* pts;
    double qx, qy, qz, r2, b;
    int32_t* ri;
    double* rd;
    int64_t m, filled;
    bool append;
    __device__ double bound() const { return b; }
    __device__ void visit(uint32_t s, uint32_t e) {
        if (append) {  // batched loads; entries appended in visiting order
            uint32_t t = s;
            for (; t + 4 <= e; t += 4) {
                double4 p[4];
#pragma unroll
                for (int u = 0; u < 4; u++) p[u] = pts[t + u];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const double d = l2_simple(qx, qy, qz, p[u]);
                    if (d < r2 && filled < m) { rd[filled] = d; ri[filled] = (int)p[u].w; filled++; }
                }
            }
            for (; t < e; t++) {
                const double4 p = pts[t];
                const double d = l2_simple(qx, qy, qz, p);
                if (d < r2 && filled < m) { rd[filled] = d; ri[filled] = (int)p.w; filled++; }
            }
            return;
        }
        for (uint32_t t = s; t < e; t++) {
            const double4 p = pts[t];
            const double d = l2_simple(qx, qy, qz, p);
            if (!(d < r2)) continue;
            const int j = (int)p.w;
            int64_t pos;
            if (filled < m) pos = filled++;
            else if (lex_less(d, j, rd[m - 1], ri[m - 1])) pos = m - 1;
            else continue;
            while (pos > 0 && lex_less(d, j, rd[pos - 1], ri[pos - 1])) {
                rd[pos] = rd[pos - 1];
                ri[pos] = ri[pos - 1];
                pos--;
            }
            rd[pos] = d;
            ri[pos] = j;
        }
    }
};

// Orders each appended CSR row by (d2, j) and maps j -> caller index.  One wave per row:
// rows up to kSortMax elements are bitonic-sorted in the wave's LDS slice; longer rows
// (rare) are insertion-sorted by lane 0 in place.
constexpr int kSortMax = 1024;
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(256) void k_sort_rows(const int64_t* off, int64_t nq, uint32_t cap, int32_t* ri,
                                                   double* rd, const int32_t* mapping, int identity) {
    __shared__ double sd[4][kSortMax];
    __shared__ int sj[4][kSortMax];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t nw = (int64_t)gridDim.x * 4;
    for (int64_t row = (int64_t)blockIdx.x * 4 + w; row < nq; row += nw) {
        const int64_t o = off[row], m = off[row + 1] - o;
        if (m <= 0 || (uint64_t)m >= cap) {  // empty, or an insertion-sorted (truncatable) row
            if (!identity)
                for (int64_t t = lane; t < m; t += 64) ri[o + t] = mapping[ri[o + t]];
            continue;
        }
        if (m > kSortMax) {
            if (lane == 0) {
                for (int64_t a = 1; a < m; a++) {
                    const double d = rd[o + a];
                    const int j = ri[o + a];
                    int64_t p = a;
                    while (p > 0 && lex_less(d, j, rd[o + p - 1], ri[o + p - 1])) {
                        rd[o + p] = rd[o + p - 1];
                        ri[o + p] = ri[o + p - 1];
                        p--;
                    }
                    rd[o + p] = d;
                    ri[o + p] = j;
                }
            }
            wave_lds_sync();
            if (!identity)
                for (int64_t t = lane; t < m; t += 64) ri[o + t] = mapping[ri[o + t]];
            continue;
        }
        int N = 1;
        while (N < m) N <<= 1;
        for (int t = lane; t < N; t += 64) {
            sd[w][t] = t < m ? rd[o + t] : INFINITY;
            sj[w][t] = t < m ? ri[o + t] : INT_MAX;
        }
        wave_lds_sync();
        for (int k = 2; k <= N; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = lane; t < N; t += 64) {
                    const int u = t ^ j;
                    if (u > t) {
                        const double a = sd[w][t], b = sd[w][u];
                        const int ja = sj[w][t], jb = sj[w][u];
                        const bool up = (t & k) == 0;
                        if (up == lex_less(b, jb, a, ja)) {
                            sd[w][t] = b; sd[w][u] = a;
                            sj[w][t] = jb; sj[w][u] = ja;
                        }
                    }
                }
                wave_lds_sync();
            }
        for (int t = lane; t < m; t += 64) {
            rd[o + t] = sd[w][t];
            ri[o + t] = identity ? sj[w][t] : mapping[sj[w][t]];
        }
        wave_lds_sync();
    }
}

template <bool FAR>
__global__ __launch_bounds__(kB) void k_radius_fill(GridDesc g, const double4* pts, const double* q, size_t qstride,
                                                    int64_t nq, double r2, uint32_t cap, double mc,
                                                    const int64_t* off, int32_t* oidx, double* od2, FarList far) {
    const int64_t nw = work_count<FAR>(far, nq);
    for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < nw; w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = work_item<FAR>(far, w);
        const int64_t o = off[i], m = off[i + 1] - o;
        if (m <= 0) continue;
        const double* qp = qptr(q, qstride, i);
        FillVisitor v{pts, qp[0], qp[1], qp[2], r2, r2 * (1.0 + 1e-12), oidx + o, od2 + o, m, 0,
                      (uint64_t)m < cap};
        if (!ring_search<double, FillVisitor, FAR>(g, v.qx, v.qy, v.qz, mc, v))
            defer(far, i);  // the far pass rebuilds the row from scratch
    }
}

// max_nn == 0 or > total => unlimited (kd_tree.h:873-883)
uint32_t radius_cap(const pcp_index* ix, uint32_t max_nn) {
    if (max_nn == 0 || (int64_t)max_nn >= ix->n) return UINT32_MAX;
    return max_nn;
}

// a fixed radius that reaches past the near pass's cell rings goes straight to the far pass
bool radius_needs_far(const pcp_index* ix, double radius) { return radius * ix->g.inv_h >= (double)kCellRings; }

// The launches of one pass over nq queries, a... being the kernels' arguments before their
// FarList: the far kernel alone over every query (far_only), or the near kernel with a deferred
// list of the call's and the far kernel over that list.
template <typename Kern, typename... A>
int near_then_far(Tmp& tmp, bool far_only, int64_t nq, Kern near, Kern far, A... a) {
    const hipStream_t st = tmp.ctx->stream;
    if (far_only) {
        hipLaunchKernelGGL(far, dim3(blocks_for(nq)), dim3(kB), 0, st, a..., FarList{nullptr, nullptr});
        return PCP_OK;
    }
    FarBuf fb;
    PCP_TRY(fb.alloc(tmp, nq));
    hipLaunchKernelGGL(near, dim3(blocks_for(nq)), dim3(kB), 0, st, a..., fb.f);
    hipLaunchKernelGGL(far, dim3(kFarBlocks), dim3(kB), 0, st, a..., fb.f);
    return PCP_OK;
}

}  // namespace
}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_radius_count(pcp_ctx* ctx, const pcp_index* ix, const double* q, size_t qstride, int64_t nq, double radius,
                     uint32_t max_nn, int32_t* ocnt) {
    PCP_TRY(check_f64_index(ctx, ix));
    if (nq < 0 || (nq > 0 && (!q || !ocnt)) || !(radius >= 0))
        return set_error(ctx, PCP_ERR_ARG, "pcp_radius_count: bad arguments");
    if (qstride == 0) qstride = 3 * sizeof(double);
    if (nq == 0) return PCP_OK;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    const double4* pts = (const double4*)ix->pts;
    const uint32_t cap = radius_cap(ix, max_nn);
    const double mc = cell_margin64(ix->g);
    Tmp tmp(ctx);
    PCP_TRY(near_then_far(tmp, radius_needs_far(ix, radius), nq, k_radius_count<false>, k_radius_count<true>, ix->g, pts,
                          q, qstride, nq, radius * radius, cap, mc, ocnt));
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

int pcp_radius_fill(pcp_ctx* ctx, const pcp_index* ix, const double* q, size_t qstride, int64_t nq, double radius,
                    uint32_t max_nn, const int64_t* off, int32_t* oidx, double* od2) {
    PCP_TRY(check_f64_index(ctx, ix));
    if (nq < 0 || (nq > 0 && (!q || !off || !oidx || !od2)) || !(radius >= 0))
        return set_error(ctx, PCP_ERR_ARG, "pcp_radius_fill: bad arguments");
    if (qstride == 0) qstride = 3 * sizeof(double);
    if (nq == 0) return PCP_OK;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    const double4* pts = (const double4*)ix->pts;
    const double mc = cell_margin64(ix->g);
    const uint32_t cap = radius_cap(ix, max_nn);
    Tmp tmp(ctx);
    PCP_TRY(near_then_far(tmp, radius_needs_far(ix, radius), nq, k_radius_fill<false>, k_radius_fill<true>, ix->g, pts,
                          q, qstride, nq, radius * radius, cap, mc, off, oidx, od2));
    hipLaunchKernelGGL(k_sort_rows, dim3(grid_for((nq + 3) / 4, 1, 1 << 16)), dim3(256), 0, ctx->stream, off, nq, cap,
                       oidx, od2, ix->mapping, ix->identity);
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

}  // extern "C"
