// The ICP correspondence contract's device arithmetic, shared by the single-pair kernels (icp.hip)
// and the batched ones (icp_batch.hip) so that both paths run one set of expressions: the fp32
// pose chain (every kernel that needs a query's image under the pose calls xform), the fp32 d2,
// the running (d2, target index) winner and the exact row search over the fp32 grid index, plus
// the cell key both query sorts order by.  What is done with a found pair is icp_pair.hpp's.
#pragma once
#include "grid.hpp"

namespace pcp {

// q' = R q + t: x' = fmaf(R02,z,fmaf(R01,y,fmaf(R00,x,t0))), R row-major.  The one place the chain
// is written: its nesting order is the bit-exact contract with the oracle.
__device__ __forceinline__ void xform_rt(const float (&R)[9], const float (&t)[3], const float4 q, float& x, float& y,
                                         float& z) {
    x = __fmaf_rn(R[2], q.z, __fmaf_rn(R[1], q.y, __fmaf_rn(R[0], q.x, t[0])));
    y = __fmaf_rn(R[5], q.z, __fmaf_rn(R[4], q.y, __fmaf_rn(R[3], q.x, t[1])));
    z = __fmaf_rn(R[8], q.z, __fmaf_rn(R[7], q.y, __fmaf_rn(R[6], q.x, t[2])));
}
// under a's pose.  A: anything with float R[9] and t[3].
template <typename A>
__device__ __forceinline__ void xform(const A& a, const float4 q, float& x, float& y, float& z) {
    xform_rt(a.R, a.t, q, x, y, z);
}
// the same chain for a query read from a caller's strided float array
template <typename A>
__device__ __forceinline__ void xform(const A& a, const float* q, float& x, float& y, float& z) {
    xform(a, make_float4(q[0], q[1], q[2], 0.f), x, y, z);
}

// running 1-NN: best d2, its target index (tie order) and its position in the scanned array
#ifndef PCP_SCAN_UNROLL
#define PCP_SCAN_UNROLL 4
#endif
// the contract's fp32 d2: fmaf(dz,dz,fmaf(dy,dy,dx*dx))
__device__ __forceinline__ float icp_d2(float qx, float qy, float qz, const float4 p) {
    const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
    return __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, dx * dx));
}

// position of candidate v of four concatenated rows (row prefixes c1 <= c2 <= c3, per-row
// offsets o0..o3): register selects only (an indexed form was lowered to an LDS table of
// pointers plus a scratch load per candidate)
__device__ __forceinline__ uint32_t cat_addr(uint32_t v, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t o0,
                                             uint32_t o1, uint32_t o2, uint32_t o3) {
    const uint32_t a = v < c3 ? o2 : o3;
    const uint32_t b = v < c2 ? o1 : a;
    return v + (v < c1 ? o0 : b);
}

struct Best {
    float bd;
    int bj;
    uint32_t bk;
    float px, py, pz;  // filled by fetch() once the scan is over
    __device__ __forceinline__ void consider(float qx, float qy, float qz, const float4 p, uint32_t k) {
        const float d2 = icp_d2(qx, qy, qz, p);
        const int id = __float_as_int(p.w);
        // "<=" on the index: re-visiting the current winner (a provisional bound) refreshes bk
        const bool take = d2 < bd || (d2 == bd && id <= bj);
        bd = take ? d2 : bd;
        bj = take ? id : bj;
        bk = take ? k : bk;
    }
    // candidates [s, e) of `pts` (LDS or global); loads issued 4 at a time so the memory
    // latency of a candidate is not serialised behind the previous update
    template <typename P>
    __device__ __forceinline__ void scan(const P* pts, uint32_t s, uint32_t e, float qx, float qy, float qz) {
        uint32_t k = s;
        for (; k + 4 <= e; k += 4) {
            const float4 p0 = pts[k], p1 = pts[k + 1], p2 = pts[k + 2], p3 = pts[k + 3];
            consider(qx, qy, qz, p0, k);
            consider(qx, qy, qz, p1, k + 1);
            consider(qx, qy, qz, p2, k + 2);
            consider(qx, qy, qz, p3, k + 3);
        }
        for (; k < e; k++) consider(qx, qy, qz, pts[k], k);
    }
    // rows r = 0..3 ([rs[r], rs[r] + rn[r])) scanned as one concatenated list, 4 loads in flight
    template <typename P, int NR>
    __device__ __forceinline__ void scan_rows(const P* pts, const uint32_t (&rs)[NR], const uint32_t (&rn)[NR],
                                              float qx, float qy, float qz) {
        static_assert(NR == 3 || NR == 4, "3 or 4 rows");
        const uint32_t c1 = rn[0], c2 = c1 + rn[1], c3 = c2 + rn[2], L = NR == 4 ? c3 + rn[NR - 1] : c3;
        const uint32_t o0 = rs[0], o1 = rs[1] - c1, o2 = rs[2] - c2, o3 = rs[NR - 1] - c3;
        const uint32_t c3e = NR == 4 ? c3 : 0xffffffffu;  // 3 rows: never past the third
        auto addr = [=](uint32_t v) { return cat_addr(v, c1, c2, c3e, o0, o1, o2, o3); };
        uint32_t v = 0;
        constexpr int U = PCP_SCAN_UNROLL;
        for (; v + U <= L; v += U) {
            uint32_t k[U];
            float4 p[U];
#pragma unroll
            for (int u = 0; u < U; u++) k[u] = addr(v + u);
#pragma unroll
            for (int u = 0; u < U; u++) p[u] = pts[k[u]];
#pragma unroll
            for (int u = 0; u < U; u++) consider(qx, qy, qz, p[u], k[u]);
        }
        for (; v < L; v++) {
            const uint32_t k = addr(v);
            consider(qx, qy, qz, pts[k], k);
        }
    }
    // G lanes per query: lane `sub` of the group takes entries sub, sub + G, ... of the same
    // ranges (strided scan / scan_rows), then merge_group() gives every lane of the group the
    // group's (d2, index) winner.  A lane prunes with its own bound, which is never below the
    // group's, so nothing the group's winner needs is skipped.
    template <int G, typename P>
    __device__ __forceinline__ void scan_g(const P* pts, uint32_t s, uint32_t e, float qx, float qy, float qz,
                                           uint32_t sub) {
        if (G == 1) {
            scan(pts, s, e, qx, qy, qz);
            return;
        }
        uint32_t k = s + sub;
        for (; k + 3 * G < e; k += 4 * G) {
            const float4 p0 = pts[k], p1 = pts[k + G], p2 = pts[k + 2 * G], p3 = pts[k + 3 * G];
            consider(qx, qy, qz, p0, k);
            consider(qx, qy, qz, p1, k + G);
            consider(qx, qy, qz, p2, k + 2 * G);
            consider(qx, qy, qz, p3, k + 3 * G);
        }
        for (; k < e; k += G) consider(qx, qy, qz, pts[k], k);
    }
    template <int G, typename P, int NR>
    __device__ __forceinline__ void scan_rows_g(const P* pts, const uint32_t (&rs)[NR], const uint32_t (&rn)[NR],
                                                float qx, float qy, float qz, uint32_t sub) {
        if (G == 1) {
            scan_rows(pts, rs, rn, qx, qy, qz);
            return;
        }
        static_assert(NR == 3 || NR == 4, "3 or 4 rows");
        const uint32_t c1 = rn[0], c2 = c1 + rn[1], c3 = c2 + rn[2], L = NR == 4 ? c3 + rn[NR - 1] : c3;
        const uint32_t o0 = rs[0], o1 = rs[1] - c1, o2 = rs[2] - c2, o3 = rs[NR - 1] - c3;
        const uint32_t c3e = NR == 4 ? c3 : 0xffffffffu;
        auto addr = [=](uint32_t v) { return cat_addr(v, c1, c2, c3e, o0, o1, o2, o3); };
        uint32_t v = sub;
        constexpr int U = PCP_SCAN_UNROLL;
        for (; v + (U - 1) * G < L; v += U * G) {
            uint32_t k[U];
            float4 p[U];
#pragma unroll
            for (int u = 0; u < U; u++) k[u] = addr(v + u * G);
#pragma unroll
            for (int u = 0; u < U; u++) p[u] = pts[k[u]];
#pragma unroll
            for (int u = 0; u < U; u++) consider(qx, qy, qz, p[u], k[u]);
        }
        for (; v < L; v += G) {
            const uint32_t k = addr(v);
            consider(qx, qy, qz, pts[k], k);
        }
    }
    template <int G>
    __device__ __forceinline__ void merge_group() {
#pragma unroll
        for (int s = 1; s < G; s <<= 1) {
            const float od = __shfl_xor(bd, s, 64);
            const int oj = __shfl_xor(bj, s, 64);
            const uint32_t ok = (uint32_t)__shfl_xor((int)bk, s, 64);
            const bool t = od < bd || (od == bd && oj < bj);
            bd = t ? od : bd;
            bj = t ? oj : bj;
            bk = t ? ok : bk;
        }
    }
    template <typename P>
    __device__ __forceinline__ void fetch(const P* pts) {
        const float4 p = pts[bk];
        px = p.x; py = p.y; pz = p.z;
    }
};

// Exact 1-NN within sqrt(b.bd) by rows of cells: the rows (y,z) that intersect the sphere's
// bounding box are visited nearest-first, and each row is scanned over the x-range of cells
// still within the (shrinking) bound -- one contiguous point range per row on a dense grid.
// Rows and cells are pruned conservatively (margin mc cells, 2e-5 relative on d2), so the
// winner equals an exhaustive lexicographic (d2, index) search.
template <int G = 1>
__device__ __forceinline__ void box_search(const GridDesc& g, const float4* tp, float qx, float qy,
                                           float qz, float mc, Best& b, uint32_t sub = 0) {
    const float fx = cell_f<float>(g, qx, 0), fy = cell_f<float>(g, qy, 1), fz = cell_f<float>(g, qz, 2);
    const int cy = (int)floorf(fy), cz = (int)floorf(fz);
    const float ly = fy - (float)cy, lz = fz - (float)cz;
    const float inv_h2 = g.inv_hf * g.inv_hf;
    const float rc = sqrtf(b.bd * 1.00002f * inv_h2) + mc;  // initial radius in cells
    // G > 1: rows are pruned by the group's bound as of its last merge (every lane of the group
    // then cuts the same x-range, so the strided entries still partition it)
    float gb = b.bd;
    const int ry = (int)ceilf(rc) + 1, rz = ry;
    for (int oz = 0; oz <= 2 * rz; oz++) {
        const int dz = (oz & 1) ? -((oz + 1) >> 1) : (oz >> 1);  // 0, -1, +1, -2, +2, ...
        const int z = cz + dz;
        if (z < 0 || z >= g.n[2]) continue;
        const float gz = dz < 0 ? (lz + (float)(-dz - 1)) : (dz > 0 ? (1.f - lz + (float)(dz - 1)) : 0.f);
        const float gz2 = gz > mc ? (gz - mc) * (gz - mc) : 0.f;
        for (int oy = 0; oy <= 2 * ry; oy++) {
            const int dy = (oy & 1) ? -((oy + 1) >> 1) : (oy >> 1);
            const int y = cy + dy;
            if (y < 0 || y >= g.n[1]) continue;
            const float gy = dy < 0 ? (ly + (float)(-dy - 1)) : (dy > 0 ? (1.f - ly + (float)(dy - 1)) : 0.f);
            const float gyz2 = gz2 + (gy > mc ? (gy - mc) * (gy - mc) : 0.f);
            const float lim = (G == 1 ? b.bd : gb) * 1.00002f * inv_h2 - gyz2;  // remaining x extent^2 (cells)
            if (lim < 0.f) continue;
            const float rx = sqrtf(lim) + mc;
            const int xa = max((int)floorf(fx - rx), 0), xb = min((int)floorf(fx + rx), g.n[0] - 1);
            if (xa > xb) continue;
            if (g.dense) {
                const int64_t c = dense_id(g, xa, y, z);
                b.scan_g<G>(tp, g.cstart[c], g.cstart[c + (xb - xa + 1)], qx, qy, qz, sub);
            } else {
                for (int x = xa; x <= xb; x++) {
                    uint32_t s, e;
                    if (cell_range(g, x, y, z, s, e)) b.scan_g<G>(tp, s, e, qx, qy, qz, sub);
                }
            }
        }
        b.merge_group<G>();  // the group's bound prunes the next plane
        gb = b.bd;
    }
    b.merge_group<G>();
}

// the pruning margin of box_search in cell units: far above the fp32 rounding of the cell
// coordinates of a grid of this many cells per axis
__host__ __device__ inline float search_margin(const GridDesc& g) {
    const int nmax = g.n[0] > g.n[1] ? (g.n[0] > g.n[2] ? g.n[0] : g.n[2]) : (g.n[1] > g.n[2] ? g.n[1] : g.n[2]);
    return 1e-5f + 8e-7f * (float)nmax;
}

// ---- the key the query sorts order by: the 8x8x8-cell brick of the octant block origin
// floor(f - 1/2) of the single-pair search pass, then the cell inside it, so that 64 consecutive
// sorted queries scan the target rows of about one brick.  query_key_end (past every brick) is
// the key of a non-finite query.
constexpr int kQBrick = 8;  // edge (cells) of the query-order bricks (the index's bricks are 4)
__host__ __device__ inline int64_t qbricks(const GridDesc& g, int a) { return (g.n[a] + kQBrick - 1) / kQBrick; }
__host__ __device__ inline uint32_t query_key_end(const GridDesc& g) {
    return (uint32_t)(qbricks(g, 0) * qbricks(g, 1) * qbricks(g, 2) * kQBrick * kQBrick * kQBrick);
}
__device__ __forceinline__ uint32_t query_cell_key(const GridDesc& g, float x, float y, float z) {
    const int cx = clampi((int)floorf(cell_f<float>(g, x, 0) - 0.5f), 0, g.n[0] - 1);
    const int cy = clampi((int)floorf(cell_f<float>(g, y, 1) - 0.5f), 0, g.n[1] - 1);
    const int cz = clampi((int)floorf(cell_f<float>(g, z, 2) - 0.5f), 0, g.n[2] - 1);
    constexpr int B = kQBrick;
    const int64_t b = ((int64_t)(cz / B) * qbricks(g, 1) + cy / B) * qbricks(g, 0) + cx / B;
    return (uint32_t)(b * B * B * B + ((cz % B) * B + cy % B) * B + cx % B);
}

}  // namespace pcp
