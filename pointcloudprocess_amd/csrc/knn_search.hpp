// What the exact fp64 grid searches share (knn.hip, radius.hip, knn_lod.hip): the block size and
// pruning margin, the lane-per-query top-k visitor, the deferred-query list that links a near
// pass to its far pass, and the host helpers that pick a compile-time K and size a launch.
// The searches themselves are grid.hpp's (ring_search, row_window_search) and topk.hpp's.
#pragma once
#include <cfloat>
#include <climits>
#include <cmath>
#include <type_traits>

#include "grid.hpp"
#include "topk.hpp"

namespace pcp {

constexpr int kB = 256;

// pruning margin in cell units: floor() rounding of query and point cell coordinates
__host__ __device__ inline double cell_margin64(const GridDesc& g) {
    const int nmax = g.n[0] > g.n[1] ? (g.n[0] > g.n[2] ? g.n[0] : g.n[2]) : (g.n[1] > g.n[2] ? g.n[1] : g.n[2]);
    return 1e-9 + 8e-16 * (double)nmax;
}

// Candidates of a cell are loaded PCP_KNN_BATCH (or 2 for the wide top-k) at a time before
// they are pushed, so the loads of a batch are in flight together instead of one dependent
// round trip per candidate.  Push order is unchanged (and irrelevant: (d2, j) order).
#ifndef PCP_KNN_BATCH
#define PCP_KNN_BATCH 4
#endif
template <int K>
struct KnnVisitor {
    static constexpr int U = K <= 16 ? PCP_KNN_BATCH : 2;
    const double4* pts;
    double qx, qy, qz;
    TopK<K> top;
    // a known upper bound on the query's k-th d2 (the tile's: k points it already holds), or inf
    double cap = INFINITY;
    // pruning radius^2 (1e-12 covers the rounding of the cell-box bound and of d2)
    __device__ double bound() const { return fmin(top.kth(), cap) * (1.0 + 1e-12); }
    __device__ __forceinline__ void take(double d, int j) {
        if (d <= cap * (1.0 + 1e-12)) top.push(d, j);
    }
    __device__ void visit(uint32_t s, uint32_t e) {
        uint32_t t = s;
        for (; t + U <= e; t += U) {
            double4 p[U];
#pragma unroll
            for (int u = 0; u < U; u++) p[u] = pts[t + u];
#pragma unroll
            for (int u = 0; u < U; u++) take(l2_simple(qx, qy, qz, p[u]), (int)p[u].w);
        }
        for (; t < e; t++) {
            const double4 p = pts[t];
            take(l2_simple(qx, qy, qz, p), (int)p.w);
        }
    }
};

__device__ __forceinline__ const double* qptr(const double* q, size_t stride, int64_t i) {
    return (const double*)((const char*)q + (size_t)i * stride);
}

// Two-pass scheduling of the ring search (grid.hpp): the near pass runs the cell rings only and
// appends queries whose bound reaches past them to `list`; the far pass takes exactly those --
// one wave per query for kNN and the normals (knn_coop.hpp), the brick-level ring search over the
// list for radius search (radius.hip).  Keeps the common path's register footprint small.
struct FarList {
    int32_t* list;
    uint32_t* count;
    // optional, per entry: an upper bound on the query's exact k-th d2 (the k-th exact d2 of a
    // set of k points the earlier pass already holds), so the next pass prunes from the start
    double* ub = nullptr;
};

__device__ __forceinline__ void defer(const FarList& f, int64_t i, double ub = INFINITY) {
    const uint32_t at = atomicAdd(f.count, 1u);
    f.list[at] = (int32_t)i;
    if (f.ub) f.ub[at] = ub;
}

// deferred-query list of one call (blocks of the call's Tmp)
struct FarBuf {
    FarList f{nullptr, nullptr};
    int alloc(Tmp& tmp, int64_t n, bool with_ub = false) {
        PCP_TRY(tmp.get(&f.list, n));
        PCP_TRY(tmp.get(&f.count, 1));
        if (with_ub) PCP_TRY(tmp.get(&f.ub, n));
        PCP_HIP(tmp.ctx, hipMemsetAsync(f.count, 0, sizeof(uint32_t), tmp.ctx->stream));
        return PCP_OK;
    }
};
constexpr unsigned kFarBlocks = 2048;

// The one place a run-time k picks a compile-time list size: calls
// f(std::integral_constant<int, KV>{}) with the smallest KV of {1, 4, 8, 16, 32, 64} that holds
// k entries.  f is instantiated for the sizes up to KMAX only; the caller has refused k > KMAX
// (PCP_ERR_UNSUPPORTED), for which nothing is called.
template <int KMAX, int KV = 1, typename F>
inline void with_k(int k, F&& f) {
    if constexpr (KV <= KMAX) {
        if (k <= KV) f(std::integral_constant<int, KV>{});
        else with_k<KMAX, (KV == 1 ? 4 : 2 * KV)>(k, f);
    }
}

inline unsigned blocks_for(int64_t n) { return grid_for(n, kB, 1 << 22); }

inline int check_f64_index(pcp_ctx* ctx, const pcp_index* ix) {
    if (!ctx || !ix) return PCP_ERR_ARG;
    if (!ix->is_f64) return set_error(ctx, PCP_ERR_ARG, "fp64 (FLANN-contract) index required");
    return PCP_OK;
}

}  // namespace pcp
