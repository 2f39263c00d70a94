// Exact fp64 neighbour queries over the uniform-grid index: the FLANN contract of
// KdTreeFLANN::nearestKSearch (kd_tree.h:814-845) and the per-point PCA normals of
// calculate_feature.cpp:119-206 over kNN neighbourhoods.  Radius search is radius.hip's, the
// kd_tree_lod search knn_lod.hip's, the per-segment plane fit plane_fit.hip's; what they share
// with this file is knn_search.hpp.
//
// One lane per query.  The k best (d2, internal j) pairs live in registers (compile-time
// K, unrolled branch-free insertion) and the ring search (grid.hpp) visits cells nearest
// first, pruning with the current k-th distance.  d2 is FLANN L2_Simple<double>
// ((0 + d0^2) + d1^2) + d2^2 with contraction off (the build compiles -ffp-contract=off),
// so distances are bit-identical to the reference's and ties break on internal j exactly
// like FLANN's "first found in index order" result set after sorting.  Queries whose k-th
// neighbour lies past the cell rings go to the wave-per-query far pass (knn_coop.hpp).
#include <cstdlib>
#include <vector>

#include "sortcfg.hpp"

#include "knn_coop.hpp"
#include "pca.hpp"

#ifndef PCP_NORMALS_STATS
#define PCP_NORMALS_STATS 0  // profiling builds: per-phase counters of pcp_normals_knn on stderr
#endif

namespace pcp {
namespace {

#ifndef PCP_T_WB  // window rows per batch of cell-start loads (tiled normals)
#define PCP_T_WB 5
#endif
// K3: batch nearestKSearch, the near pass (cell rings only; k_knn_coop takes the deferred rows).
// Rows ascending by (d2, internal j), indices mapped through index_mapping_ (kd_tree.h:837-842);
// entries past min(k, size) are -1 / +inf.
template <int K>
__global__ __launch_bounds__(kB) void k_knn(GridDesc g, const double4* pts, const int32_t* mapping, int identity,
                                            const double* q, size_t qstride, int64_t nq, int k, int kk,
                                            double mc, int32_t* oidx, double* od2, FarList far) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nq; i += (int64_t)gridDim.x * blockDim.x) {
        const double* qp = qptr(q, qstride, i);
        KnnVisitor<K> v;
        v.pts = pts;
        v.qx = qp[0]; v.qy = qp[1]; v.qz = qp[2];
        v.top.init(kk);
        if (kk > 0 && finite3(v.qx, v.qy, v.qz) &&
            !ring_search<double, KnnVisitor<K>, false>(g, v.qx, v.qy, v.qz, mc, v)) {
            defer(far, i);
            continue;
        }
        int32_t* ri = oidx + i * k;
        double* rd = od2 + i * k;
        v.top.for_each_ascending(kk, [&](int r, double d, int j) {
            const bool ok = j != INT_MAX;
            ri[r] = ok ? (identity ? j : mapping[j]) : -1;
            if (od2) rd[r] = ok ? d : INFINITY;
        });
        for (int r = kk; r < k; r++) {
            ri[r] = -1;
            if (od2) rd[r] = INFINITY;
        }
    }
}

template <int K>
__global__ __launch_bounds__(kB) void k_knn_coop(GridDesc g, const double4* pts, const int32_t* mapping, int identity,
                                                 const double* q, size_t qstride, int k, int kk, double mc,
                                                 int32_t* oidx, double* od2, FarList far) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x / 64), cnt = *far.count;
    for (int64_t w = blockIdx.x * (int64_t)(blockDim.x / 64) + (threadIdx.x >> 6); w < cnt; w += nwaves) {
        const int64_t i = far.list[w];
        const double* qp = qptr(q, qstride, i);
        CoopVisitor<K> v;
        v.pts = pts;
        v.qx = qp[0]; v.qy = qp[1]; v.qz = qp[2];
        v.top.init(kk);
        coop_search<K>(g, mc, v, lane, kk);
        double md;
        int mj;
        coop_merge<K>(v, kk, lane, md, mj);
        // entry r < kk (<= 64) is lane r's; the lanes stride over the padding [kk, k), which
        // reaches past the wave when k > 64 over an index of at most 64 points
        for (int r = lane; r < k; r += 64) {
            const bool ok = r < kk && mj != INT_MAX;
            oidx[i * k + r] = ok ? (identity ? mj : mapping[mj]) : -1;
            if (od2) od2[i * k + r] = ok ? md : INFINITY;
        }
    }
}

template <int K>
__global__ __launch_bounds__(kB, 2) void k_normals_coop(GridDesc g, const double4* pts, const int32_t* mapping,
                                                     int identity, const int32_t* pos_of_j, int kk, double mc,
                                                     pcp_plane* out, int64_t n_out, FarList far,
                                                     unsigned long long* dbg) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x / 64), cnt = *far.count;
    for (int64_t w = blockIdx.x * (int64_t)(blockDim.x / 64) + (threadIdx.x >> 6); w < cnt; w += nwaves) {
        const int64_t s = far.list[w];
        const double4 qp = pts[s];
        CoopVisitor<K> v;
        v.pts = pts;
        v.qx = qp.x; v.qy = qp.y; v.qz = qp.z;
        v.top.init(kk);
        if (far.ub) v.shared = far.ub[w];  // the earlier passes' k-th: pruning from the first ring
        // dbg: null, or 16 counters of the profiling build (PCP_NORMALS_STATS)
        int shells = 0;
        const long long t0 = dbg ? (long long)clock64() : 0;
        long long tk[5] = {t0, 0, 0, 0, 0};
        coop_search<K>(g, mc, v, lane, kk, dbg ? &shells : nullptr, dbg ? tk : nullptr);
        if (dbg && lane == 0) {  // shells walked and cycles per deferred query
            const unsigned long long dt = (unsigned long long)((long long)clock64() - t0);
            atomicAdd(dbg + 0, 1ull);
            atomicAdd(dbg + 1, (unsigned long long)shells);
            atomicMax(dbg + 2, (unsigned long long)shells);
            atomicAdd(dbg + 3, dt);
            atomicMax(dbg + 4, dt);
            atomicAdd(dbg + 9, (unsigned long long)(tk[0] - t0));  // ring phase
            atomicAdd(dbg + 10, (unsigned long long)tk[1]);        // kth_bound in the shells
            if (dt >= dbg[4]) {  // the slowest query's coordinates and phases (racy, debugging only)
                dbg[11] = (unsigned long long)(tk[0] - t0);
                dbg[12] = (unsigned long long)tk[1];
                dbg[13] = (unsigned long long)tk[2];
                dbg[14] = (unsigned long long)tk[3];
                dbg[15] = (unsigned long long)tk[4];
                dbg[5] = (unsigned long long)__double_as_longlong(qp.x);
                dbg[6] = (unsigned long long)__double_as_longlong(qp.y);
                dbg[7] = (unsigned long long)__double_as_longlong(qp.z);
                dbg[8] = (unsigned long long)__double_as_longlong(v.shared);
            }
        }
        double md;
        int mj;
        coop_merge<K>(v, kk, lane, md, mj);
        const int jq = (int)qp.w;
        const int64_t oi = identity ? jq : mapping[jq];
        if (oi >= n_out) continue;
        // mean and X X^T, sequential in kNN order (calculate_feature.cpp:131-164), wave-uniform;
        // lane r fetches the r-th neighbour once (all loads in flight together), the sums then
        // walk the lanes in order through shuffles
        double4 pr = make_double4(0.0, 0.0, 0.0, 0.0);
        if (lane < kk && mj != INT_MAX) pr = pts[pos_of_j[mj]];
        double xa = 0, ya = 0, za = 0;
        for (int r = 0; r < kk; r++) {
            xa += __shfl(pr.x, r, 64); ya += __shfl(pr.y, r, 64); za += __shfl(pr.z, r, 64);
        }
        xa /= kk; ya /= kk; za /= kk;
        double c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0;
        for (int r = 0; r < kk; r++) {
            const double4 p = make_double4(__shfl(pr.x, r, 64), __shfl(pr.y, r, 64), __shfl(pr.z, r, 64), 0.0);
            const double x0 = p.x - xa, x1 = p.y - ya, x2 = p.z - za;
            c00 += x0 * x0; c01 += x0 * x1; c02 += x0 * x2;
            c11 += x1 * x1; c12 += x1 * x2; c22 += x2 * x2;
        }
        if (lane == 0) {
            const double C[9] = {c00, c01, c02, c01, c11, c12, c02, c12, c22};
            pcp_plane pl;
            plane_from_cov(C, xa, ya, za, pl);
            out[oi] = pl;
        }
    }
}

// F1 PCA core (eigen_sym3, plane_from_cov): pca.hpp

__global__ void k_plane_default(pcp_plane* out, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = pcp_plane{0.f, 0.f, 0.f, 0.f, 1.f, 0.f};  // rpca's N <= 3 branch (:353-361)
}

// the call's deferral counters into the context's two words (pcp_normals_knn_last_deferred);
// b null: the second word is unused
__global__ void k_keep_deferred(const uint32_t* a, const uint32_t* b, uint32_t* out) {
    out[0] = *a;
    out[1] = b ? *b : 0u;
}

// The near pass of the normals (k_normals_coop takes the deferred rows).
// queries = the indexed points themselves, walked in the index's spatial order
// `in`: the sorted positions to process (the tiled kernel's uncertified queries), or every
// point when in.list is null
// ROWS (the near pass over the tiled kernel's uncertified queries): the row walk below; its
// own instantiation, so the all-points ring path does not carry its registers
template <int K, bool ROWS = false>
__global__ __launch_bounds__(kB) void k_normals(GridDesc g, const double4* pts, const int32_t* mapping, int identity,
                                                const int32_t* pos_of_j, int64_t n, int kk, double mc,
                                                pcp_plane* out, int64_t n_out, FarList far,
                                                FarList in = FarList{nullptr, nullptr}) {
    const int64_t nw = in.list ? (int64_t)*in.count : n;
    for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < nw; w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = in.list ? (int64_t)in.list[w] : w;
        const double4 qp = pts[s];
        KnnVisitor<K> v;
        v.pts = pts;
        v.qx = qp.x; v.qy = qp.y; v.qz = qp.z;
        v.top.init(kk);
        // the tile's k-th: its kk points lie within its window (+-2 cells), inside this pass's
        // window, so the walk below still finds kk points under the cap
        if (ROWS && in.ub) v.cap = in.ub[w];
        // the near pass over the tiled kernel's uncertified queries, on dense grids, walks the
        // window by rows (the queries are indexed points, so they lie inside the grid).  Not for
        // every point: a large k over a dense neighbourhood fills its list faster cell by cell
        // (measured: k = 32 over all 8.86M C3 points 32.7 -> 67.0 ms by rows; the tile's 10.9K
        // uncertified rows 0.3 ms faster, k = 8 0.3 ms)
        const bool done = (ROWS && g.dense)
                              ? row_window_search<KnnVisitor<K>>(g, v.qx, v.qy, v.qz, mc, v)
                              : ring_search<double, KnnVisitor<K>, false>(g, v.qx, v.qy, v.qz, mc, v);
        if (!done) {
            // the tile's bound or the window's own k-th, whichever is smaller
            defer(far, s, fmin(in.ub ? in.ub[w] : INFINITY, v.top.kth()));
            continue;
        }
        const int jq = (int)qp.w;
        const int64_t oi = identity ? jq : mapping[jq];
        if (oi >= n_out) continue;
        // mean and X X^T, sequential in kNN order (:131-164)
        pcp_plane pl;
        plane_from_sequence(kk, [&](auto use) {
            v.top.for_each_ascending(kk, [&](int, double, int j) {
                const double4 p = pts[pos_of_j[j]];
                use(p.x, p.y, p.z);
            });
        }, pl);
        out[oi] = pl;
    }
}

// F1 over kNN, tiled (dense grids, k <= 32): one wave per 64 consecutive sorted points.
// The wave copies the union of its queries' neighbourhoods -- the box of their cells grown by
// R cells, one contiguous point run per (y, z) row -- into LDS as fp32 coordinates relative to
// the box corner plus the sorted position.  Every lane then scans the whole list (uniform trip
// count, broadcast LDS reads, no divergence) keeping its M = K + kTileSlack (1) smallest packed keys
// (bits(fp32 d2) & ~1023 | list index) and the (M+1)-th as a bound with a v_med3_u32 network
// (M + 1 VALU ops per candidate instead of the fp64 register top-k's divergent shifts).  The
// kept candidates are re-ranked by the exact FLANN fp64 (d2, j) and sorted; the lane's result
// is certified when its k-th exact d2 lies strictly below both the bound on every uncached
// list point (the (M+1)-th key less the fp32 error) and the squared distance to the box faces
// (points outside the box).  Uncertified lanes go to the exact two-level search (k_normals'
// row walk, then k_normals_coop), so the output is that of the exact path bit for bit.
constexpr int kTileCap = 2048;   // union points per wave (11-bit list index)
constexpr int kTileRows = 255;   // (y, z) rows per wave (255: the wave's LDS fits 8 waves per CU)
constexpr int kTileQ = 16383;    // 14-bit fixed-point coordinates: squared distances fit in int32
constexpr int kTileExt = 96;     // box extent (cells) cap: keeps the fixed-point step fine
constexpr int kLaneR = 2;        // largest window half-width of the per-lane window scan
constexpr int kTileSlack = 1;    // keys kept per lane beyond k (the re-rank's slack; 2-4 slower, 0 defers 10x the rows)
// (dy, dz) of row i of a 5 x 5 (y, z) window, rows by squared distance (the first 9 are the 3 x 3
// window): (dy + 2) | (dz + 2) << 3 in 6-bit fields, 10 to a word (i is wave-uniform: scalar ops)
__device__ __forceinline__ void window_row(int i, int& dy, int& dz) {
    const uint64_t w = i < 10 ? 0x50964b6ca6914d2ull : (i < 20 ? 0x8438c860c702890ull : 0x804901ull);
    const uint32_t v = (uint32_t)(w >> (6 * (i % 10))) & 63u;
    dy = (int)(v & 7u) - 2;
    dz = (int)(v >> 3) - 2;
}
__device__ __forceinline__ uint32_t umed3_(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// squared distance of two packed 14-bit points: (x | y << 16, z) -- v_pk_sub_i16 + v_dot2_i32_i16
__device__ __forceinline__ uint32_t qd2(uint32_t qxy, int qz, uint32_t pxy, int pz) {
    uint32_t dxy;
    asm("v_pk_sub_i16 %0, %1, %2" : "=v"(dxy) : "v"(qxy), "v"(pxy));
    const int dz = qz - pz;
    int r;
    asm("v_dot2_i32_i16 %0, %1, %1, %2" : "=v"(r) : "v"(dxy), "v"(__mul24(dz, dz)));  // |dz| < 2^14: v_mul_i32_i24, full rate
    return (uint32_t)r;
}
__device__ __forceinline__ int wmin_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wmax_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
// keeps a loaded value live on every lane: a load whose result is only used under a per-lane
// condition is otherwise sunk into a branch with its own wait, one round trip per load
__device__ __forceinline__ void pin(uint32_t& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void pin(double& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ int quant14(double v, double inv) {
    const double t = rint(v * inv);
    return (int)(t < 0.0 ? 0.0 : (t > (double)kTileQ ? (double)kTileQ : t));
}

// the union box of the lanes with `in` set, grown by R cells; its rows' point runs are listed
// (start and exclusive prefix in s_rs / s_rb) when `write` is set
struct TileBox {
    int x0, x1, y0, y1, z0, z1, ny, nrow;
    uint32_t total;  // points in the box (0xffffffff: too many rows / too wide)
};
__device__ __forceinline__ TileBox tile_box(const GridDesc& g, int cx, int cy, int cz, bool in, int R, int lane,
                                            uint32_t* s_rs, uint32_t* s_rb, bool write) {
    TileBox b;
    b.x0 = max(wmin_i(in ? cx : INT_MAX) - R, 0), b.x1 = min(wmax_i(in ? cx : INT_MIN) + R, g.n[0] - 1);
    b.y0 = max(wmin_i(in ? cy : INT_MAX) - R, 0), b.y1 = min(wmax_i(in ? cy : INT_MIN) + R, g.n[1] - 1);
    b.z0 = max(wmin_i(in ? cz : INT_MAX) - R, 0), b.z1 = min(wmax_i(in ? cz : INT_MIN) + R, g.n[2] - 1);
    b.ny = b.y1 - b.y0 + 1;
    b.nrow = b.ny * (b.z1 - b.z0 + 1);
    b.total = 0xffffffffu;
    const int ext = max(max(b.x1 - b.x0, b.y1 - b.y0), b.z1 - b.z0) + 1;
    if (b.nrow > kTileRows || ext > kTileExt) return b;
    // every row's cell starts first (unconditional loads of a clamped row: one round trip for
    // the whole box), then the prefix sums
    constexpr int kRowIt = (kTileRows + 63) / 64;
    uint32_t st_[kRowIt], en_[kRowIt];
#pragma unroll
    for (int it = 0; it < kRowIt; it++) {
        const int r = it * 64 + lane;
        const int rc = r < b.nrow ? r : 0;
        const int y = b.y0 + rc % b.ny, z = b.z0 + rc / b.ny;
        st_[it] = g.cstart[dense_id(g, b.x0, y, z)];
        en_[it] = g.cstart[dense_id(g, b.x1, y, z) + 1];
    }
#pragma unroll
    for (int it = 0; it < kRowIt; it++) pin(st_[it]), pin(en_[it]);
    uint32_t carry = 0;
#pragma unroll
    for (int it = 0; it < kRowIt; it++) {
        const int r0 = it * 64;
        if (r0 >= b.nrow) break;
        const int r = r0 + lane;
        const uint32_t st = r < b.nrow ? st_[it] : 0u;
        const uint32_t cnt = r < b.nrow ? en_[it] - st_[it] : 0u;
        uint32_t inc = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (write && r < b.nrow) {
            s_rs[r] = st;
            s_rb[r] = carry + inc - cnt;
        }
        carry += __shfl(inc, 63, 64);
    }
    if (write && lane == 0) s_rb[b.nrow] = carry;
    b.total = carry;
    return b;
}

// query order of the tiled kernel: sorted positions by 8x8x8-cell brick (stable, so row-major
// inside a brick), so that a wave's 64 queries are neighbours in all three axes -- in the index's
// row-major order the points of one x-row of a facade are metres apart
constexpr int kTileBrick = 3;  // log2 brick edge (cells)
// Inside a brick the key continues with `lb` bits of a Morton code of the point's position
// (cell and sub-cell: 2^(lb/3) steps per brick edge), so a wave's 64 queries form a compact
// patch instead of a run along one x-row of cells (lb = 0: index order inside the brick).
__device__ __forceinline__ uint32_t spread3(uint32_t v) {  // bits b -> 3b
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x30000ffu;
    v = (v | (v << 8)) & 0x300f00fu;
    v = (v | (v << 4)) & 0x30c30c3u;
    v = (v | (v << 2)) & 0x9249249u;
    return v;
}
__global__ void k_brick_keys(GridDesc g, const double4* pts, int64_t n, int lb, uint32_t* key, uint32_t* pos) {
    const int nbx = (g.n[0] + 7) >> kTileBrick, nby = (g.n[1] + 7) >> kTileBrick;
    const int sub = lb / 3 - kTileBrick;  // sub-cell bits per axis (>= 0 when lb > 0)
    for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        const double4 p = pts[s];
        const double fx = cell_f<double>(g, p.x, 0), fy = cell_f<double>(g, p.y, 1), fz = cell_f<double>(g, p.z, 2);
        const int cx = clampi((int)floor(fx), 0, g.n[0] - 1), cy = clampi((int)floor(fy), 0, g.n[1] - 1),
                  cz = clampi((int)floor(fz), 0, g.n[2] - 1);
        uint32_t k = (uint32_t)(((int64_t)(cz >> kTileBrick) * nby + (cy >> kTileBrick)) * nbx + (cx >> kTileBrick));
        if (lb > 0) {
            const double sc = (double)(1 << sub);
            auto loc = [&](double f, int c) {  // position in the brick, 2^(3 + sub) steps
                const int q = (c & ((1 << kTileBrick) - 1)) << sub;
                const int t = (int)((f - (double)c) * sc);
                return (uint32_t)(q + (t < 0 ? 0 : (t >= (1 << sub) ? (1 << sub) - 1 : t)));
            };
            k = (k << lb) | spread3(loc(fx, cx)) | (spread3(loc(fy, cy)) << 1) | (spread3(loc(fz, cz)) << 2);
        }
        key[s] = k;
        pos[s] = (uint32_t)s;
    }
}

template <int K>
__global__ __launch_bounds__(64, 2) void k_normals_tile(GridDesc g, const double4* pts, const int32_t* mapping,
                                                     int identity, int64_t n, int kk, int R, double mc,
                                                     pcp_plane* out, int64_t n_out, FarList far,
                                                     unsigned long long* stats, const uint32_t* order) {
    constexpr int M = K + kTileSlack;
    constexpr uint32_t kMax = 0xffffffffu;
    __shared__ uint2 s_u[kTileCap];
    __shared__ uint32_t s_rs[kTileRows], s_rb[kTileRows + 1];
    __shared__ uint8_t s_row[kTileCap];  // the (y, z) row of each staged point
    const int lane = threadIdx.x;
    // the next chunk's sorted positions are loaded a chunk ahead (the chain order -> point ->
    // cells -> rows -> staging starts one round trip shorter)
    uint32_t s_next = blockIdx.x * 64 < n ? order[min((int64_t)blockIdx.x * 64 + lane, n - 1)] : 0u;
    for (int64_t c = blockIdx.x; c * 64 < n; c += gridDim.x) {
        const bool valid = c * 64 + lane < n;
        const int64_t s = s_next;  // a sorted position
        {
            const int64_t cn = c + gridDim.x;
            if (cn * 64 < n) s_next = order[min(cn * 64 + lane, n - 1)];
        }
        const double4 q = pts[s];
        const int cx = cell_i<double>(g, q.x, 0), cy = cell_i<double>(g, q.y, 1), cz = cell_i<double>(g, q.z, 2);
        // Groups of lanes, each staged and scanned on its own: the whole wave when its box fits
        // the LDS list; else the runs of lanes in one query brick (the wave's queries are in
        // brick order, so a wave that crosses into a distant brick -- the next row of bricks --
        // splits there), cut to at most 16 lanes if a run still does not fit.  A group whose box
        // does not fit even then takes the exact search.
        int grp = 0, G = 1;
        bool over = false;  // this lane's group does not fit: deferred
        // the whole wave's box, listed at once (the common case: no second pass of row starts)
        wave_lds_fence();  // the previous chunk's readers are done with the lists
        const TileBox bw = tile_box(g, cx, cy, cz, valid, R, lane, s_rs, s_rb, true);
        const bool whole = bw.total <= (uint32_t)kTileCap;
        if (!whole) {
            const int nbx = (g.n[0] + 7) >> kTileBrick, nby = (g.n[1] + 7) >> kTileBrick;
            const int bxq = clampi(cx, 0, g.n[0] - 1) >> kTileBrick, byq = clampi(cy, 0, g.n[1] - 1) >> kTileBrick,
                      bzq = clampi(cz, 0, g.n[2] - 1) >> kTileBrick;
            const uint32_t bid = (uint32_t)(((int64_t)bzq * nby + byq) * nbx + bxq);
            const uint32_t prev = (uint32_t)__shfl_up((int)bid, 1, 64);
            const uint64_t below = lane == 63 ? ~0ull : ((2ull << lane) - 1);  // lanes <= this one
            const uint64_t heads = __ballot(lane == 0 || bid != prev);
            const int run = __popcll(heads & below) - 1;
            const int rstart = 63 - __clzll(heads & below);
            const int nruns = __popcll(heads);
            for (int pass = 0; pass < 2; pass++) {
                G = pass == 0 ? nruns : nruns * 4;
                grp = pass == 0 ? run : run * 4 + (lane - rstart) / 16;
                bool bad = false;
                for (int gi = 0; gi < G; gi++) {
                    const bool in = valid && grp == gi;
                    if (!__ballot(in)) continue;
                    const TileBox b = tile_box(g, cx, cy, cz, in, R, lane, s_rs, s_rb, false);
                    if (b.total > (uint32_t)kTileCap) {
                        bad = true;
                        over = over || grp == gi;
                    }
                }
                if (!bad) break;
                if (pass == 0) over = false;
            }
        }
        if (over) {  // this lane's group takes the exact search
            if (valid) defer(far, s);
            if (stats) atomicAdd(stats + 1, 1ull);
        }
        if (stats && lane == 0 && G > 1) atomicAdd(stats + 3, (unsigned long long)G);
        for (int gi = 0; gi < G; gi++) {
            const bool mine = grp == gi && !over;
            if (!__ballot(mine && valid)) continue;  // an empty or deferred group
            TileBox b = bw;
            if (!whole) {
                wave_lds_fence();  // the previous group's readers are done with the lists
                b = tile_box(g, cx, cy, cz, mine && valid, R, lane, s_rs, s_rb, true);
            }
            const uint32_t total = b.total;
            wave_lds_fence();
            // 14-bit fixed point relative to the box corner, one step for all three axes
            const double ox = g.o[0] + (double)b.x0 * g.h, oy = g.o[1] + (double)b.y0 * g.h,
                         oz = g.o[2] + (double)b.z0 * g.h;
            const int ext = max(max(b.x1 - b.x0, b.y1 - b.y0), b.z1 - b.z0) + 1;
            const double step = (double)ext * g.h / (double)kTileQ, inv = 1.0 / step;
            // e advances by 64 per step, so each lane's row only moves forward: a short walk
            // instead of a binary search, and the row of every staged point is kept (one byte)
            // for the re-rank's list index -> position lookups.  kSB entries per lane per step:
            // their rows first, then kSB unconditional loads (a lane past the list reads position
            // 0), so a step waits on one round trip, not kSB
            int rw = 0;
            constexpr int kSB = 4;  // staged points per lane per load batch (8: neutral)
            for (uint32_t e0 = lane; e0 < total; e0 += 64 * kSB) {
                uint32_t pi[kSB];
#pragma unroll
                for (int u = 0; u < kSB; u++) {
                    const uint32_t e = e0 + 64u * u;
                    const bool on = e < total;
                    while (on && s_rb[rw + 1] <= e) rw++;
                    if (on) s_row[e] = (uint8_t)rw;
                    pi[u] = on ? s_rs[rw] + (e - s_rb[rw]) : 0u;
                }
                double px[kSB], py[kSB], pz[kSB];
#pragma unroll
                for (int u = 0; u < kSB; u++) {
                    const double4* pp = pts + pi[u];
                    px[u] = pp->x;
                    py[u] = pp->y;
                    pz[u] = pp->z;
                }
#pragma unroll
                for (int u = 0; u < kSB; u++) {
                    pin(px[u]), pin(py[u]), pin(pz[u]);
                }
#pragma unroll
                for (int u = 0; u < kSB; u++) {
                    const uint32_t e = e0 + 64u * u;
                    if (e < total)
                        s_u[e] = make_uint2((uint32_t)quant14(px[u] - ox, inv) | ((uint32_t)quant14(py[u] - oy, inv) << 16),
                                            (uint32_t)quant14(pz[u] - oz, inv));
                }
            }
            wave_lds_fence();
            const uint32_t qxy = (uint32_t)quant14(q.x - ox, inv) | ((uint32_t)quant14(q.y - oy, inv) << 16);
            const int qz = quant14(q.z - oz, inv);
            uint32_t t[M + 1];
#pragma unroll
            for (int i = 0; i <= M; i++) t[i] = kMax;
            // keys: the float bits of the integer d2 (relative precision 2^-12 after the index
            // bits, whatever the step) | list index
            auto key = [&](uint32_t d, uint32_t e) {
                return (__float_as_uint((float)d) & ~(uint32_t)(kTileCap - 1)) | e;
            };
            auto insert = [&](uint32_t x) {
#pragma unroll
                for (int i = M; i >= 1; i--) t[i] = umed3_(t[i - 1], t[i], x);
                t[0] = min(t[0], x);
            };
            // Per-lane windows (R <= kLaneR): each lane scans only the rows of ITS OWN
            // (2R+1)^2 (y, z) window -- the x-range of its +-R cells, nearest rows first -- from
            // the staged list, instead of every point of the wave's union box (a compact patch's
            // union box holds 4-10x a lane's window).  The lanes walk their own row lists (kept in
            // LDS after the staged points) in lockstep with per-lane LDS addresses, and the
            // insertion network runs only when some lane's key is below its current (M+1)-th
            // (insertion of a larger key is a no-op on every slot).  Every window point not kept
            // has a key >= the final (M+1)-th, so the list bound below is unchanged; the box-face
            // bound becomes the lane's window faces.
            bool lane_path = false;
            const bool act = mine && valid;
            const int wx0 = max(cx - R, b.x0), wx1 = min(cx + R, b.x1);
            if (R <= kLaneR) {
                constexpr int kW = (2 * kLaneR + 1) * (2 * kLaneR + 1);
                const int nwin = R >= 2 ? 25 : (R == 1 ? 9 : 1);
                // the LDS run [a, e) of every window row as a | e << 16 (0: empty / outside the
                // box).  The cell-start loads of all kW rows are unconditional (cell 0 for a row
                // outside) and issued before any is used: one round trip, not one per row
                // row (dy, dz) of the window: cell (wx0, cy + dy, cz + dz) = the lane's base cell
                // plus a uniform offset (scalar: dy, dz are constants of the unrolled loop)
                const int64_t cbase = act ? dense_id(g, wx0, cy, cz) : 0;
                const int64_t sy = g.n[0], sz = (int64_t)g.n[0] * g.n[1];
                const uint32_t xw = (uint32_t)(wx1 - wx0 + 1);
                const int rbase = (cy - b.y0) + (cz - b.z0) * b.ny;
                uint32_t run[kW];
                constexpr int kWB = PCP_T_WB;  // rows per batch of cell-start loads
#pragma unroll
                for (int i0 = 0; i0 < kW; i0 += kWB) {
                    uint32_t ca[kWB], cb[kWB], okm = 0;
#pragma unroll
                    for (int u = 0; u < kWB && i0 + u < kW; u++) {
                        int dy, dz;
                        window_row(i0 + u, dy, dz);
                        const int y = cy + dy, z = cz + dz;
                        const bool ok = act && i0 + u < nwin && y >= b.y0 && y <= b.y1 && z >= b.z0 && z <= b.z1;
                        okm |= ok ? 1u << u : 0u;
                        const int64_t c0 = ok ? cbase + dy * sy + dz * sz : 0;
                        ca[u] = g.cstart[c0];
                        cb[u] = g.cstart[ok ? c0 + xw : 0];
                    }
#pragma unroll
                    for (int u = 0; u < kWB && i0 + u < kW; u++) pin(ca[u]), pin(cb[u]);
#pragma unroll
                    for (int u = 0; u < kWB && i0 + u < kW; u++) {
                        int dy, dz;
                        window_row(i0 + u, dy, dz);
                        const bool ok = (okm >> u) & 1u;
                        const int r = ok ? rbase + dy + dz * b.ny : 0;
                        const uint32_t a0 = s_rb[r] + (ca[u] - s_rs[r]);
                        run[i0 + u] = ok && cb[u] > ca[u] ? a0 | ((a0 + (cb[u] - ca[u])) << 16) : 0u;
                    }
                }
                uint32_t* s_w = reinterpret_cast<uint32_t*>(s_u);
                int nr = 0, excl = 0;
                if (2 * total + 64u * kW <= 2u * kTileCap) {
                    // room for a fixed kW-word region per lane at the end of the list (odd stride:
                    // the lanes' reads of one slot fall in distinct banks)
                    lane_path = true;
                    excl = 2 * kTileCap - 64 * kW + lane * kW;
#pragma unroll
                    for (int i = 0; i < kW; i++)
                        if (run[i]) s_w[excl + nr++] = run[i];
                } else {
#pragma unroll
                    for (int i = 0; i < kW; i++) nr += run[i] ? 1 : 0;  // this lane's non-empty rows
                    excl = nr;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const int t2 = __shfl_up(excl, o, 64);
                        if (lane >= o) excl += t2;
                    }
                    const int tot_rows = __shfl(excl, 63, 64);
                    excl -= nr;
                    lane_path = 2 * total + (uint32_t)tot_rows <= 2u * kTileCap;
                    if (lane_path) {  // compacted after the staged points
                        excl += 2 * (int)total;
                        int j = excl;
#pragma unroll
                        for (int i = 0; i < kW; i++)
                            if (run[i]) s_w[j++] = run[i];
                    }
                }
                if (lane_path) {
                    wave_lds_fence();
                    uint32_t rp = (uint32_t)excl, rend = (uint32_t)(excl + nr);
                    uint32_t e = 0, ee = 0;
                    for (;;) {
                        if (e >= ee && rp < rend) {
                            const uint32_t wr = s_w[rp++];
                            e = wr & 0xffffu;
                            ee = wr >> 16;
                        }
                        const bool on = e < ee;
                        if (__ballot(on) == 0) break;
                        const uint2 pp = s_u[on ? e : 0u];
                        const uint32_t x = on ? key(qd2(qxy, qz, pp.x, (int)pp.y), e) : kMax;
                        e += on ? 1u : 0u;
                        if (__ballot(x < t[M]) != 0) insert(x);
                    }
                    if (stats && lane == 0) atomicAdd(stats + 20, 1ull);
                }
            }
            if (!lane_path) {
                uint32_t e = 0;
                for (; e + 4 <= total; e += 4) {
                    uint2 p[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) p[u] = s_u[e + u];
#pragma unroll
                    for (int u = 0; u < 4; u++) insert(key(qd2(qxy, qz, p[u].x, (int)p[u].y), e + u));
                }
                for (; e < total; e++) {
                    const uint2 pp = s_u[e];
                    insert(key(qd2(qxy, qz, pp.x, (int)pp.y), e));
                }
                if (stats && lane == 0) atomicAdd(stats + 21, 1ull);
            }
            if (!mine) continue;  // (no wave-wide operation follows)
            // the faces of the scanned region (the box, or the lane's window) that have grid cells
            // beyond them bound every point outside the list (taken before the re-rank, so that
            // only b2 stays live across it)
            int fx0 = b.x0, fx1 = b.x1, fy0 = b.y0, fy1 = b.y1, fz0 = b.z0, fz1 = b.z1;
            if (lane_path) {
                fx0 = wx0; fx1 = wx1;
                fy0 = max(cy - R, b.y0); fy1 = min(cy + R, b.y1);
                fz0 = max(cz - R, b.z0); fz1 = min(cz + R, b.z1);
            }
            double bd = INFINITY;
            if (fx0 > 0) bd = fmin(bd, q.x - (g.o[0] + (double)fx0 * g.h));
            if (fx1 < g.n[0] - 1) bd = fmin(bd, g.o[0] + (double)(fx1 + 1) * g.h - q.x);
            if (fy0 > 0) bd = fmin(bd, q.y - (g.o[1] + (double)fy0 * g.h));
            if (fy1 < g.n[1] - 1) bd = fmin(bd, g.o[1] + (double)(fy1 + 1) * g.h - q.y);
            if (fz0 > 0) bd = fmin(bd, q.z - (g.o[2] + (double)fz0 * g.h));
            if (fz1 < g.n[2] - 1) bd = fmin(bd, g.o[2] + (double)(fz1 + 1) * g.h - q.z);
            bd -= mc * g.h + 1e-12 * (fabs(q.x) + fabs(q.y) + fabs(q.z) + 1.0);
            const double b2 = bd > 0.0 ? bd * bd * (1.0 - 1e-12) : (bd == INFINITY ? INFINITY : 0.0);
            // exact FLANN re-rank of the kept candidates.  The fp64 records are gathered in
            // batches of kRB unconditional loads (a slot without a candidate reads position 0 and
            // is discarded), so a wave waits on M / kRB round trips instead of one per candidate
            // (a load under a per-lane condition is a branch with its own wait).
            constexpr int kRB = 8;  // fp64 records per gather batch of the re-rank and PCA (16: slower)
            double D[M];
            uint32_t P[M];
#pragma unroll
            for (int i = 0; i < M; i++) {
                const bool has = t[i] != kMax;
                const uint32_t ei = t[i] & (uint32_t)(kTileCap - 1);
                const int r = s_row[has ? ei : 0u];
                P[i] = has ? s_rs[r] + (ei - s_rb[r]) : 0u;
            }
#pragma unroll
            for (int i0 = 0; i0 < M; i0 += kRB) {
                double px[kRB], py[kRB], pz[kRB];
#pragma unroll
                for (int u = 0; u < kRB && i0 + u < M; u++) {
                    const double4* pp = pts + P[i0 + u];
                    px[u] = pp->x;
                    py[u] = pp->y;
                    pz[u] = pp->z;
                }
#pragma unroll
                for (int u = 0; u < kRB && i0 + u < M; u++) {
                    pin(px[u]), pin(py[u]), pin(pz[u]);
                }
#pragma unroll
                for (int u = 0; u < kRB && i0 + u < M; u++)
                    D[i0 + u] = t[i0 + u] != kMax ? l2_simple(q.x, q.y, q.z, make_double4(px[u], py[u], pz[u], 0.0))
                                                  : INFINITY;
            }
            // every list point not kept: its quantised distance is >= sqrt(float(t[M] & ~2047))
            // steps (the int -> float rounding is covered by the 2^-20), and quantisation moves
            // each coordinate of both points by <= step / 2
            double lb = INFINITY;
            if (t[M] != kMax) {
                const double v =
                    (sqrt((double)__uint_as_float(t[M] & ~(uint32_t)(kTileCap - 1))) * (1.0 - 0x1p-20) -
                     1.7320508075688772 - 1e-3) * step;
                lb = v > 0.0 ? v * v * (1.0 - 1e-12) : 0.0;
            }
            // sort (d2, j) ascending: odd-even transposition rounds until no swap (the approximate
            // order is almost exact, so this ends after one or two rounds)
            bool any = true;
            while (any) {
                any = false;
#pragma unroll
                for (int par = 0; par < 2; par++) {
#pragma unroll
                    for (int i = par; i + 1 < M; i += 2) {
                        bool gt = D[i] > D[i + 1];
                        if (D[i] == D[i + 1] && D[i] != INFINITY)
                            gt = (int)pts[P[i]].w > (int)pts[P[i + 1]].w;
                        const double dl = gt ? D[i + 1] : D[i], dh = gt ? D[i] : D[i + 1];
                        const uint32_t pl = gt ? P[i + 1] : P[i], ph = gt ? P[i] : P[i + 1];
                        D[i] = dl; D[i + 1] = dh; P[i] = pl; P[i + 1] = ph;
                        any = any || gt;
                    }
                }
            }
            double dk = INFINITY;
#pragma unroll
            for (int i = 0; i < M; i++)
                if (i == kk - 1) dk = D[i];
            if (!valid) continue;
            if (!(dk < lb && dk < b2)) {
                defer(far, s, dk);  // dk: the k-th exact d2 of the kept points, an upper bound
                if (stats) atomicAdd(stats + (dk < lb ? 2 : 0), 1ull);
                continue;
            }
            const int jq = (int)q.w;
            const int64_t oi = identity ? jq : mapping[jq];
            if (oi >= n_out) continue;
            // mean, sequential in kNN order (calculate_feature.cpp:131-142); the records again in
            // batches of unconditional loads (P[i] is a valid position for every i)
            double xa = 0, ya = 0, za = 0;
#pragma unroll
            for (int i0 = 0; i0 < K; i0 += kRB) {
                double px[kRB], py[kRB], pz[kRB];
#pragma unroll
                for (int u = 0; u < kRB && i0 + u < K; u++) {
                    const double4* pp = pts + P[i0 + u];
                    px[u] = pp->x;
                    py[u] = pp->y;
                    pz[u] = pp->z;
                }
#pragma unroll
                for (int u = 0; u < kRB && i0 + u < K; u++) {
                    pin(px[u]), pin(py[u]), pin(pz[u]);
                }
#pragma unroll
                for (int u = 0; u < kRB && i0 + u < K; u++) {
                    if (i0 + u < kk) {
                        xa += px[u]; ya += py[u]; za += pz[u];
                    }
                }
            }
            xa /= kk; ya /= kk; za /= kk;
            double c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0;
#pragma unroll
            for (int i0 = 0; i0 < K; i0 += kRB) {
                double px[kRB], py[kRB], pz[kRB];
#pragma unroll
                for (int u = 0; u < kRB && i0 + u < K; u++) {
                    const double4* pp = pts + P[i0 + u];
                    px[u] = pp->x;
                    py[u] = pp->y;
                    pz[u] = pp->z;
                }
#pragma unroll
                for (int u = 0; u < kRB && i0 + u < K; u++) {
                    pin(px[u]), pin(py[u]), pin(pz[u]);
                }
#pragma unroll
                for (int u = 0; u < kRB && i0 + u < K; u++) {
                    if (i0 + u < kk) {
                        const double a0 = px[u] - xa, a1 = py[u] - ya, a2 = pz[u] - za;
                        c00 += a0 * a0; c01 += a0 * a1; c02 += a0 * a2;
                        c11 += a1 * a1; c12 += a1 * a2; c22 += a2 * a2;
                    }
                }
            }
            const double C[9] = {c00, c01, c02, c01, c11, c12, c02, c12, c22};
            pcp_plane pl;
            plane_from_cov(C, xa, ya, za, pl);
            out[oi] = pl;
        }
    }
}

// K7 (main_blend.cpp:306-325): argmin over queries of the 1-NN d2, strict '<' from an
// initial bound, so the first query wins ties.  Per-block lexicographic (d2, i) minimum.
__global__ __launch_bounds__(kB) void k_argmin_d2(const double* d2, int64_t n, double* pd, int64_t* pi) {
    double bd = INFINITY;
    int64_t bi = INT64_MAX;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double d = d2[i];
        if (d < bd || (d == bd && i < bi)) { bd = d; bi = i; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bd, o, 64);
        const int64_t oi = __shfl_xor(bi, o, 64);
        if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
    }
    __shared__ double sd[kB / 64];
    __shared__ int64_t si[kB / 64];
    if ((threadIdx.x & 63) == 0) { sd[threadIdx.x >> 6] = bd; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kB / 64; w++)
            if (sd[w] < bd || (sd[w] == bd && si[w] < bi)) { bd = sd[w]; bi = si[w]; }
        pd[blockIdx.x] = bd;
        pi[blockIdx.x] = bi;
    }
}

}  // namespace
}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_knn(pcp_ctx* ctx, const pcp_index* ix, const double* q, size_t qstride, int64_t nq, int k,
            int32_t* oidx, double* od2) {
    if (ctx) ctx->knn_far_set = false;
    PCP_TRY(check_f64_index(ctx, ix));
    if (nq < 0 || k <= 0 || (nq > 0 && (!q || !oidx))) return set_error(ctx, PCP_ERR_ARG, "pcp_knn: bad arguments");
    if (qstride == 0) qstride = 3 * sizeof(double);
    if (nq == 0) return PCP_OK;
    const int kk = (int)(k < ix->n ? k : ix->n);  // kd_tree.h:820-821
    if (kk > 64) return set_error(ctx, PCP_ERR_UNSUPPORTED, "pcp_knn: k=%d > 64 not supported yet", k);
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->knn_far) PCP_HIP(ctx, hipMalloc(&ctx->knn_far, sizeof(uint32_t)));
    const double mc = cell_margin64(ix->g);
    const double4* pts = (const double4*)ix->pts;
    Tmp tmp(ctx);
    FarBuf fb;
    PCP_TRY(fb.alloc(tmp, nq));
    with_k<64>(kk, [&](auto kc) {
        constexpr int KV = decltype(kc)::value;
        hipLaunchKernelGGL(k_knn<KV>, dim3(blocks_for(nq)), dim3(kB), 0, ctx->stream, ix->g, pts, ix->mapping,
                           ix->identity, q, qstride, nq, k, kk, mc, oidx, od2, fb.f);
        hipLaunchKernelGGL(k_knn_coop<KV>, dim3(kFarBlocks), dim3(kB), 0, ctx->stream, ix->g, pts, ix->mapping,
                           ix->identity, q, qstride, k, kk, mc, oidx, od2, fb.f);
    });
    PCP_LAUNCH_CHECK(ctx);
    // the far list's length for pcp_knn_last_far, stream-ordered before the list's block is reused
    PCP_HIP(ctx, hipMemcpyAsync(ctx->knn_far, fb.f.count, sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
    ctx->knn_far_set = true;
    return PCP_OK;
}

int pcp_knn_last_far(pcp_ctx* ctx, int64_t* n) {
    if (!ctx || !n) return PCP_ERR_ARG;
    *n = 0;
    if (!ctx->knn_far_set) return PCP_OK;
    uint32_t h = 0;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    PCP_HIP(ctx, hipMemcpyAsync(&h, ctx->knn_far, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    PCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n = h;
    return PCP_OK;
}

int pcp_normals_knn(pcp_ctx* ctx, const pcp_index* ix, int k, pcp_plane* out, int64_t n_out) {
    PCP_TRY(check_f64_index(ctx, ix));
    ctx->nrm_mode = 0;
    if (k <= 0 || n_out < 0 || (n_out > 0 && !out)) return set_error(ctx, PCP_ERR_ARG, "pcp_normals_knn: bad arguments");
    if (n_out < ix->n_in) return set_error(ctx, PCP_ERR_CAPACITY, "pcp_normals_knn: n_out < cloud size");
    const int kk = (int)(k < ix->n ? k : ix->n);
    if (kk > 32) return set_error(ctx, PCP_ERR_UNSUPPORTED, "pcp_normals_knn: k=%d > 32 not supported yet", k);
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    if (n_out > 0) hipLaunchKernelGGL(k_plane_default, dim3(blocks_for(n_out)), dim3(kB), 0, ctx->stream, out, n_out);
    if (ix->n == 0 || kk <= 3) return PCP_OK;  // rpca's N > 3 guard (calculate_feature.cpp:237)
    if (!ctx->nrm_deferred) PCP_HIP(ctx, hipMalloc(&ctx->nrm_deferred, 2 * sizeof(uint32_t)));
    const double mc = cell_margin64(ix->g);
    const double4* pts = (const double4*)ix->pts;
    Tmp tmp(ctx);
    FarBuf fb;
    PCP_TRY(fb.alloc(tmp, ix->n, true));
    const int tile_R = kk <= 8 ? 1 : 2;  // the tile's window half-width in cells
    // per-phase counters of profiling builds (PCP_NORMALS_STATS): the tile's [0, 4) and [20, 22),
    // the far pass's [4, 20)
    unsigned long long* st = nullptr;
#if PCP_NORMALS_STATS
    PCP_TRY(tmp.get(&st, 24));
    PCP_HIP(ctx, hipMemsetAsync(st, 0, 24 * sizeof(unsigned long long), ctx->stream));
#endif
    // the wave-per-query pass over the queries of `list`
    auto far_pass = [&](auto kc, const FarList& list) {
        constexpr int KV = decltype(kc)::value;
        hipLaunchKernelGGL(k_normals_coop<KV>, dim3(kFarBlocks), dim3(kB), 0, ctx->stream, ix->g, pts, ix->mapping,
                           ix->identity, ix->pos_of_j, kk, mc, out, n_out, list, st ? st + 4 : nullptr);
    };
    if (ix->g.dense) {
        const unsigned nbt = (unsigned)std::min<int64_t>((ix->n + 63) / 64, 1 << 20);
        // brick order of the queries: (brick key, sorted position) radix-sorted
        uint32_t *k0, *k1, *v0, *order;
        PCP_TRY(tmp.get(&k0, ix->n));
        PCP_TRY(tmp.get(&k1, ix->n));
        PCP_TRY(tmp.get(&v0, ix->n));
        PCP_TRY(tmp.get(&order, ix->n));
        const int64_t nbr = (int64_t)((ix->g.n[0] + 7) >> kTileBrick) * ((ix->g.n[1] + 7) >> kTileBrick) *
                            ((ix->g.n[2] + 7) >> kTileBrick);
        unsigned bits = 1;
        while (bits < 32 && ((int64_t)1 << bits) < nbr) bits++;
        // Morton bits inside the brick: cell + sub-cell (12) when the key still fits 32 bits
        const int lb = bits + 12 <= 32 ? 12 : (bits + 9 <= 32 ? 9 : 0);
        hipLaunchKernelGGL(k_brick_keys, dim3(blocks_for(ix->n)), dim3(kB), 0, ctx->stream, ix->g, pts, ix->n, lb, k0,
                           v0);
        bits += (unsigned)lb;
        PCP_TRY(sort_pairs(tmp, k0, k1, v0, order, (size_t)ix->n, 0u, bits));
        FarBuf fb2;  // the near pass's own deferred queries
        PCP_TRY(fb2.alloc(tmp, ix->n, true));
        // the tile's uncertified queries: the lane-per-query near pass (cell rings), its own
        // deferrals then the wave-per-query pass (all of them straight to the wave-per-query pass
        // measured slower)
        with_k<32>(kk, [&](auto kc) {
            // the tile has no K = 1: 1 and 4 both use 4
            constexpr int KV = decltype(kc)::value < 4 ? 4 : decltype(kc)::value;
            hipLaunchKernelGGL(k_normals_tile<KV>, dim3(nbt), dim3(64), 0, ctx->stream, ix->g, pts, ix->mapping,
                               ix->identity, ix->n, kk, tile_R, mc, out, n_out, fb.f, st, order);
            hipLaunchKernelGGL((k_normals<KV, true>), dim3(blocks_for(ix->n)), dim3(kB), 0, ctx->stream, ix->g, pts,
                               ix->mapping, ix->identity, ix->pos_of_j, ix->n, kk, mc, out, n_out, fb2.f, fb.f);
            far_pass(std::integral_constant<int, KV>{}, fb2.f);
        });
        hipLaunchKernelGGL(k_keep_deferred, dim3(1), dim3(1), 0, ctx->stream, fb.f.count, fb2.f.count,
                           ctx->nrm_deferred);
        PCP_LAUNCH_CHECK(ctx);
        ctx->nrm_mode = 1;
#if PCP_NORMALS_STATS
        {
            unsigned long long h[24];
            unsigned c1 = 0, c2 = 0;
            PCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
            PCP_HIP(ctx, hipMemcpy(h, st, sizeof(h), hipMemcpyDeviceToHost));
            PCP_HIP(ctx, hipMemcpy(&c1, fb.f.count, 4, hipMemcpyDeviceToHost));
            PCP_HIP(ctx, hipMemcpy(&c2, fb2.f.count, 4, hipMemcpyDeviceToHost));
            const unsigned long long* d = h + 4;
            fprintf(stderr, "normals stats: n=%lld k=%d tile deferred %u (list bound %llu, box %llu, oversize %llu), "
                    "near deferred %u; far pass: %llu queries, shells mean %.1f max %llu, cycles mean %.0f max %llu "
                    "(slowest: ring %llu, kth %llu, bricks %llu, rows+points %llu, mid-shell %llu; at %.2f %.2f %.2f)\n",
                    (long long)ix->n, k, c1, h[0], h[2], h[1], c2, d[0], d[0] ? (double)d[1] / d[0] : 0.0, d[2],
                    d[0] ? (double)d[3] / d[0] : 0.0, d[4], d[11], d[12], d[13], d[14], d[15],
                    __builtin_bit_cast(double, d[5]), __builtin_bit_cast(double, d[6]), __builtin_bit_cast(double, d[7]));
        }
#endif
        return PCP_OK;
    }
    with_k<32>(kk, [&](auto kc) {
        constexpr int KV = decltype(kc)::value;
        hipLaunchKernelGGL(k_normals<KV>, dim3(blocks_for(ix->n)), dim3(kB), 0, ctx->stream, ix->g, pts, ix->mapping,
                           ix->identity, ix->pos_of_j, ix->n, kk, mc, out, n_out, fb.f, FarList{nullptr, nullptr});
        far_pass(kc, fb.f);
    });
    hipLaunchKernelGGL(k_keep_deferred, dim3(1), dim3(1), 0, ctx->stream, fb.f.count, (const uint32_t*)nullptr,
                       ctx->nrm_deferred);
    PCP_LAUNCH_CHECK(ctx);
    ctx->nrm_mode = 2;
    return PCP_OK;
}

int pcp_normals_knn_last_deferred(pcp_ctx* ctx, int64_t* tile_deferred, int64_t* far_queries) {
    if (!ctx || !tile_deferred || !far_queries) return PCP_ERR_ARG;
    *tile_deferred = *far_queries = 0;
    if (!ctx->nrm_mode) return PCP_OK;
    uint32_t h[2] = {0, 0};
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    PCP_HIP(ctx, hipMemcpyAsync(h, ctx->nrm_deferred, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    PCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->nrm_mode == 1) {
        *tile_deferred = h[0];
        *far_queries = h[1];
    } else {
        *tile_deferred = -1;
        *far_queries = h[0];
    }
    return PCP_OK;
}

int pcp_nearest_query(pcp_ctx* ctx, const pcp_index* ix, const double* q, size_t qstride, int64_t nq,
                      double init_bound, int64_t* best_q, double* best_d2) {
    PCP_TRY(check_f64_index(ctx, ix));
    if (nq < 0 || (nq > 0 && !q) || !best_q || !best_d2)
        return set_error(ctx, PCP_ERR_ARG, "pcp_nearest_query: bad arguments");
    *best_q = -1;
    *best_d2 = init_bound;
    if (nq == 0 || ix->n == 0) return PCP_OK;
    int32_t* idx = nullptr;
    double* d2 = nullptr;
    double* pd = nullptr;
    int64_t* pi = nullptr;
    const unsigned nb = grid_for(nq, kB, 1024);
    Tmp tmp(ctx);
    PCP_TRY(tmp.get(&idx, nq));
    PCP_TRY(tmp.get(&d2, nq));
    PCP_TRY(tmp.get(&pd, nb));
    PCP_TRY(tmp.get(&pi, nb));
    int rc = pcp_knn(ctx, ix, q, qstride, nq, 1, idx, d2);
    if (!rc) {
        hipLaunchKernelGGL(k_argmin_d2, dim3(nb), dim3(kB), 0, ctx->stream, d2, nq, pd, pi);
        std::vector<double> hd(nb);
        std::vector<int64_t> hi(nb);
        hipError_t e = hipMemcpyAsync(hd.data(), pd, nb * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hi.data(), pi, nb * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = hip_fail(ctx, e, "nearest_query", __FILE__, __LINE__);
        // lexicographic (d2, query) minimum == the sequential strict-'<' scan's winner
        double bd = INFINITY;
        int64_t bi = INT64_MAX;
        for (unsigned b = 0; b < nb && !rc; b++)
            if (hd[b] < bd || (hd[b] == bd && hi[b] < bi)) { bd = hd[b]; bi = hi[b]; }
        if (!rc && bd < init_bound) { *best_d2 = bd; *best_q = bi; }
    }
    return rc;
}

}  // extern "C"
