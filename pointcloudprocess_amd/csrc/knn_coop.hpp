// The far pass of the exact fp64 kNN, wave-cooperative: one query per wave (included by knn.hip
// alone, by k_knn_coop and k_normals_coop).  The deferred queries are the few whose k-th
// neighbour lies beyond the near pass's cell rings -- isolated points, where one lane walking
// rings of bricks alone took milliseconds.  Here the cells of each Chebyshev ring (then the
// bricks of each brick ring) are dealt round-robin over the 64 lanes; every lane keeps its own
// exact top-k of what it scanned, pruned by min(own k-th, the wave's shared bound), where the
// shared bound -- the minimum over lanes of their k-th -- is an upper bound on the global k-th (a
// superset has a smaller k-th), refreshed at each ring.  Every point within the final global
// k-th distance was scanned by some lane, so merging the lanes' lists (k rounds of a wave-wide
// lexicographic argmin) gives the exact FLANN (d2, j) order.
#pragma once
#include "knn_search.hpp"

namespace pcp {
namespace {  // one includer: internal linkage, as when this code stood in knn.hip (K = 64 is not inlined)

template <int K>
struct CoopVisitor {
    const double4* pts;
    double qx, qy, qz;
    double shared = INFINITY;  // wave-uniform
    TopK<K> top;
    __device__ double bound() const { return fmin(top.kth(), shared) * (1.0 + 1e-12); }
    __device__ double ubound() const { return shared * (1.0 + 1e-12); }
    // a point beyond the wave's shared bound (an upper bound on the global k-th) cannot be in
    // the result: only the cheap compare, not the K-slot insertion (which a lane's own list,
    // empty until it has seen k points, would otherwise take for every point)
    __device__ __forceinline__ void take(double d, int j) {
        if (d <= shared * (1.0 + 1e-12)) top.push(d, j);
    }
};
// An upper bound on the wave's exact k-th d2 within 2^-20 of it, without copying the lists:
// the smallest tau (a double whose low word is all ones) with at least kk list entries <= tau,
// by bisection on tau's high word; each step counts the entries with one compare per slot into
// a lane mask and popcounts (SALU), no cross-lane moves.  +inf when fewer than kk are finite.
template <int K>
__device__ double kth_bound(const TopK<K>& top, int kk) {
    auto count = [&](double t) {
        int c = 0;
#pragma unroll
        for (int i = 0; i < K; i++) c += __popcll(__ballot(i < kk && top.d[i] <= t));
        return c;
    };
    if (count(DBL_MAX) < kk) return INFINITY;
    uint32_t lo = 0, hi = 0x7fefffffu;  // DBL_MAX's high word
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (count(__hiloint2double((int)mid, (int)0xffffffffu)) >= kk) hi = mid;
        else lo = mid + 1;
    }
    return __hiloint2double((int)hi, (int)0xffffffffu);
}

// An upper bound on the wave's exact k-th d2, cheap enough to refresh inside a shell: the
// kk-th smallest of the lanes' own best d2 (a subset of the union, so its kk-th smallest is at
// least the union's), by a 64-lane bitonic sort; +inf until kk lanes hold a point.
template <int K>
__device__ double wave_kth_of_bests(const TopK<K>& top, int kk, int lane) {
    double x = INFINITY;
#pragma unroll
    for (int i = 0; i < K; i++)
        if (i == kk - 1) x = top.d[i];
#pragma unroll
    for (int k2 = 2; k2 <= 64; k2 <<= 1)
#pragma unroll
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            const double y = __shfl_xor(x, j, 64);
            const bool up = (lane & k2) == 0, lower = (lane & j) == 0;
            x = (lower == up) ? fmin(x, y) : fmax(x, y);
        }
    return __shfl(x, kk - 1, 64);
}

// bricks per lane per batch of the far pass's shells (8 spilled the K = 32 lists to scratch:
// ~700 bytes per lane, every list update a round trip to memory)
constexpr int kCoopBB = 4;

// a wave's LDS writes made visible to its own later reads (release, wave barrier, acquire)
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// shells / tk: null, or the profiling build's per-query counters (PCP_NORMALS_STATS, knn.hip): brick
// shells walked; the clock at the end of the ring phase, then cycles in the shells' kth_bound, in
// brick coordinates / pruning / occupancy loads, in rows and points, in the mid-shell bound.
// They stay run-time pointers: as compile-time code the default build's C3 line measured slower
// (DESIGN 5.3).
template <int K>
__device__ void coop_search(const GridDesc& g, double mc, CoopVisitor<K>& v, int lane, int kk,
                            int* shells = nullptr, long long* tk = nullptr) {
    const double fx = cell_f<double>(g, v.qx, 0), fy = cell_f<double>(g, v.qy, 1), fz = cell_f<double>(g, v.qz, 2);
    const int cx = (int)floor(fx), cy = (int)floor(fy), cz = (int)floor(fz);
    const double lx = fx - cx, ly = fy - cy, lz = fz - cz;
    const double h2 = g.h * g.h;
    const double dmin = fmin(fmin(fmin(lx, 1 - lx), fmin(ly, 1 - ly)), fmin(lz, 1 - lz));
    int far = 0;
    far = max(far, max(cx - (g.n[0] - 1), -cx));
    far = max(far, max(cy - (g.n[1] - 1), -cy));
    far = max(far, max(cz - (g.n[2] - 1), -cz));
    const int rmax = far + max(g.n[0], max(g.n[1], g.n[2]));
    const int smax = min(rmax, kCellRings);
    // Point ranges gathered one per lane (a cell, or a row's one or two runs), then their points
    // dealt flat over the lanes -- point p to lane p % 64, its range found by a binary search of
    // the ranges' prefix in LDS -- so no lane runs a long range as a serial chain of loads while
    // the others wait.  Wave-uniform call.
    __shared__ uint32_t s_fr[kB / 64][4][64];  // per wave: the ranges' prefix, starts, lengths
    uint32_t* const f_pre = s_fr[threadIdx.x >> 6][0];
    uint32_t* const f_s1 = s_fr[threadIdx.x >> 6][1];
    uint32_t* const f_l1 = s_fr[threadIdx.x >> 6][2];
    uint32_t* const f_s2 = s_fr[threadIdx.x >> 6][3];
    constexpr int kFlatU = 2;  // points per lane in flight (4 spilled the K = 32 lists to scratch)
    auto flat_visit = [&](uint32_t s1, uint32_t l1, uint32_t s2, uint32_t l2) {
        const uint32_t cnt = l1 + l2;
        uint32_t inc = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t tv = (uint32_t)__shfl_up((int)inc, o, 64);
            if (lane >= o) inc += tv;
        }
        const uint32_t tot = (uint32_t)__shfl((int)inc, 63, 64);
        if (tot == 0) return;
        f_pre[lane] = inc - cnt;
        f_s1[lane] = s1;
        f_l1[lane] = l1;
        f_s2[lane] = s2;
        wave_lds_fence();
        for (uint32_t p0 = 0; p0 < tot; p0 += 64u * kFlatU) {  // wave-uniform
            uint32_t idx[kFlatU];
#pragma unroll
            for (int u = 0; u < kFlatU; u++) {
                const uint32_t pp = p0 + (uint32_t)lane + 64u * u;
                // the owner: the last lane whose prefix is <= pp (an empty lane shares its prefix
                // with the next, so the last one is the non-empty owner)
                int o = 0;
#pragma unroll
                for (int b = 32; b >= 1; b >>= 1) o += f_pre[o + b] <= pp ? b : 0;
                const uint32_t off = pp - f_pre[o], a1 = f_l1[o];
                idx[u] = pp < tot ? (off < a1 ? f_s1[o] + off : f_s2[o] + (off - a1)) : ~0u;
            }
            double4 q4[kFlatU];
#pragma unroll
            for (int u = 0; u < kFlatU; u++) q4[u] = v.pts[idx[u] != ~0u ? idx[u] : 0u];
#pragma unroll
            for (int u = 0; u < kFlatU; u++)
                if (idx[u] != ~0u) v.take(l2_simple(v.qx, v.qy, v.qz, q4[u]), (int)q4[u].w);
        }
        wave_lds_fence();  // the next call rewrites f_*
    };
    uint32_t t = 0;  // the wave's cell / brick counter: item t belongs to lane t % 64
    uint32_t rs = 0, rl = 0;  // this lane's pending cell range (flushed every 64 items)
    for (int s = 0; s <= smax + 1; s++) {
        if (s > 0) {
            v.shared = fmin(v.shared, kth_bound<K>(v.top, kk));
            const double rmin = (double)(s - 1) + dmin - mc;
            if (rmin > 0 && rmin * rmin * h2 > v.ubound()) return;
        }
        if (s > smax) break;
        const int z0 = max(cz - s, 0), z1 = min(cz + s, g.n[2] - 1);
        const int y0 = max(cy - s, 0), y1 = min(cy + s, g.n[1] - 1);
        const int x0 = max(cx - s, 0), x1 = min(cx + s, g.n[0] - 1);
        if (z0 > z1 || y0 > y1 || x0 > x1) continue;
        for (int z = z0; z <= z1; z++) {
            const bool zface = (z == cz - s) || (z == cz + s);
            const double gz2 = sq_gap(axis_gap<double>(z, cz, lz), mc);
            if (gz2 * h2 > v.ubound()) continue;
            for (int y = y0; y <= y1; y++) {
                const bool yface = zface || (y == cy - s) || (y == cy + s);
                const double gyz2 = gz2 + sq_gap(axis_gap<double>(y, cy, ly), mc);
                if (gyz2 * h2 > v.ubound()) continue;
                const int step = yface ? 1 : 2 * s;
                for (int x = yface ? x0 : cx - s; x <= x1; x += (step > 0 ? step : 1)) {
                    if (x < x0) continue;
                    const bool mine = (t & 63u) == (uint32_t)lane;
                    t++;
                    if (mine && (gyz2 + sq_gap(axis_gap<double>(x, cx, lx), mc)) * h2 <= v.bound()) {
                        uint32_t st, en;
                        if (cell_range(g, x, y, z, st, en)) {
                            rs = st;
                            rl = en - st;
                        }
                    }
                    if ((t & 63u) == 0u) {  // (uniform) a chunk of 64 cells: its points, flat
                        flat_visit(rs, rl, 0u, 0u);
                        rl = 0u;
                    }
                }
            }
        }
        flat_visit(rs, rl, 0u, 0u);  // the ring's last partial chunk
        rl = 0u;
    }
    if (rmax <= kCellRings) return;
    // bricks of 4x4x4 cells, rings outward, the cells phase 1 covered skipped
    const int bx = cx >> 2, by = cy >> 2, bz = cz >> 2;
    const double ox = fx - 4 * bx, oy = fy - 4 * by, oz = fz - 4 * bz;
    const double bdmin = fmin(fmin(fmin(ox, 4 - ox), fmin(oy, 4 - oy)), fmin(oz, 4 - oz));
    int farb = 0;
    farb = max(farb, max(bx - (g.nb[0] - 1), -bx));
    farb = max(farb, max(by - (g.nb[1] - 1), -by));
    farb = max(farb, max(bz - (g.nb[2] - 1), -bz));
    const int sbmax = farb + max(g.nb[0], max(g.nb[1], g.nb[2]));
    __shared__ int4 s_flat[kB / 64][64 * kCoopBB];  // per wave: a batch's occupied bricks {x, y, z, word}
    __shared__ uint16_t s_rows[kB / 64][64 * kCoopBB * 16];  // per wave: their non-empty rows (brick << 4 | row)
    int4* const flat = s_flat[threadIdx.x >> 6];
    uint16_t* const rows = s_rows[threadIdx.x >> 6];
    // rings closer than `farb` lie wholly outside the grid (a query far away from it)
    if (tk) tk[0] = clock64();
    for (int sb = farb; sb <= sbmax; sb++) {
        if (shells) (*shells)++;
        const long long c0 = tk ? (long long)clock64() : 0;
        v.shared = fmin(v.shared, kth_bound<K>(v.top, kk));
        if (tk) tk[1] += (long long)clock64() - c0;
        if (sb > 0) {
            const double rmin = (double)(4 * (sb - 1)) + bdmin - mc;
            if (rmin > 0 && rmin * rmin * h2 > v.ubound()) return;
        }
        // the shell's bricks inside the grid: two z-faces, two y-faces (z strictly inside), two
        // x-faces (y and z strictly inside), each a rectangle clipped to the grid; brick t of the
        // shell goes to lane t % 64
        const int X0 = max(bx - sb, 0), X1 = min(bx + sb, g.nb[0] - 1);
        const int Y0 = max(by - sb, 0), Y1 = min(by + sb, g.nb[1] - 1);
        const int Z0 = max(bz - sb, 0), Z1 = min(bz + sb, g.nb[2] - 1);
        if (X0 > X1 || Y0 > Y1 || Z0 > Z1) continue;
        const int Yi0 = max(by - sb + 1, 0), Yi1 = min(by + sb - 1, g.nb[1] - 1);
        const int Zi0 = max(bz - sb + 1, 0), Zi1 = min(bz + sb - 1, g.nb[2] - 1);
        int64_t area[6];
        int fixc[6];
        const int nx = X1 - X0 + 1, ny = Y1 - Y0 + 1, nyi = max(Yi1 - Yi0 + 1, 0), nzi = max(Zi1 - Zi0 + 1, 0);
        for (int f = 0; f < 6; f++) {
            const int sgn = (f & 1) ? 1 : -1;
            if (f < 2) {  // z = bz -+ sb
                fixc[f] = bz + sgn * sb;
                area[f] = (fixc[f] >= 0 && fixc[f] < g.nb[2] && (sb > 0 || f == 0)) ? (int64_t)nx * ny : 0;
            } else if (f < 4) {  // y = by -+ sb, z inside
                fixc[f] = by + sgn * sb;
                area[f] = (sb > 0 && fixc[f] >= 0 && fixc[f] < g.nb[1]) ? (int64_t)nx * nzi : 0;
            } else {  // x = bx -+ sb, y and z inside
                fixc[f] = bx + sgn * sb;
                area[f] = (sb > 0 && fixc[f] >= 0 && fixc[f] < g.nb[0]) ? (int64_t)nyi * nzi : 0;
            }
        }
        const int64_t total = area[0] + area[1] + area[2] + area[3] + area[4] + area[5];
        // bricks t = lane + 64 u: the occupancy words of a batch are loaded together (mostly
        // empty bricks around isolated queries: one dependent load each would serialise)
        constexpr int kBB = kCoopBB;
        for (int64_t base = 0; base < total; base += 64 * kBB) {  // wave-uniform trip count
            const long long cb0 = tk ? (long long)clock64() : 0;
            const int64_t t0 = base + lane;
            int bxs[kBB], bys[kBB], bzs[kBB];
            int32_t occ[kBB];
            uint32_t msk[kBB], bat[kBB];  // row masks and flat[] positions of this lane's bricks
#pragma unroll
            for (int u = 0; u < kBB; u++) {
                const int64_t t = t0 + 64 * u;
                int xb = 0, yb = 0, zb = 0;
                bool live = t < total;
                if (live) {
                    int f = 0;
                    int64_t r = t;
                    while (r >= area[f]) { r -= area[f]; f++; }
                    if (f < 2) {
                        xb = X0 + (int)(r % nx); yb = Y0 + (int)(r / nx); zb = fixc[f];
                    } else if (f < 4) {
                        xb = X0 + (int)(r % nx); zb = Zi0 + (int)(r / nx); yb = fixc[f];
                    } else {
                        yb = Yi0 + (int)(r % nyi); zb = Zi0 + (int)(r / nyi); xb = fixc[f];
                    }
                    const double gz = zb < bz ? (oz + 4.0 * (bz - zb - 1)) : (zb > bz ? (4.0 - oz + 4.0 * (zb - bz - 1)) : 0.0);
                    const double gy = yb < by ? (oy + 4.0 * (by - yb - 1)) : (yb > by ? (4.0 - oy + 4.0 * (yb - by - 1)) : 0.0);
                    const double gx = xb < bx ? (ox + 4.0 * (bx - xb - 1)) : (xb > bx ? (4.0 - ox + 4.0 * (xb - bx - 1)) : 0.0);
                    live = (sq_gap(gz, mc) + sq_gap(gy, mc) + sq_gap(gx, mc)) * h2 <= v.bound();
                }
                bxs[u] = xb; bys[u] = yb; bzs[u] = zb;
                occ[u] = live ? g.brick[((int64_t)zb * g.nb[1] + yb) * g.nb[0] + xb] : -1;
            }
            const long long cb1 = tk ? (long long)clock64() : 0;
            if (tk) tk[2] += cb1 - cb0;  // brick coordinates, pruning and occupancy loads
            // The batch's occupied bricks are listed in LDS, then their rows that hold points
            // (the brick word's row mask on dense fp64 grids; all 16 rows otherwise) as one flat
            // item list dealt round-robin over the lanes: every lane's round is one row's
            // cstart round trip, and empty rows cost none.
            uint32_t nocc = 0, nrow = 0;
            uint32_t myrows = 0;
#pragma unroll
            for (int u = 0; u < kBB; u++) {
                const uint64_t m = __ballot(occ[u] >= 0);
                if (occ[u] >= 0) {
                    const uint32_t at = nocc + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                                         __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                    flat[at] = make_int4(bxs[u], bys[u], bzs[u], occ[u]);
                    bat[u] = at;
                    const uint32_t rm = (g.dense && occ[u] > 0) ? (uint32_t)occ[u] & 0xffffu : 0xffffu;
                    msk[u] = rm;
                    myrows += (uint32_t)__popc(rm);
                } else {
                    msk[u] = 0u;
                }
                nocc += (uint32_t)__popcll(m);
            }
            // exclusive scan of the lanes' row counts -> this lane's first row slot
            uint32_t incl = myrows;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t tv = (uint32_t)__shfl_up((int)incl, o, 64);
                if (lane >= o) incl += tv;
            }
            nrow = (uint32_t)__shfl((int)incl, 63, 64);
            uint32_t slot = incl - myrows;
#pragma unroll
            for (int u = 0; u < kBB; u++) {
                uint32_t rm = msk[u];
                while (rm) {
                    const uint32_t r = (uint32_t)__builtin_ctz(rm);
                    rm &= rm - 1u;
                    rows[slot++] = (uint16_t)((bat[u] << 4) | r);
                }
            }
            wave_lds_fence();
            // Rows in chunks of 64, one per lane: the lane resolves its row to at most two point
            // ranges (one cstart round trip for the whole chunk), then the chunk's points are
            // dealt flat over the lanes -- point p to lane p % 64, its range found by a binary
            // search of the ranges' prefix in LDS -- so a long row no longer runs as one lane's
            // serial chain of loads while the others wait.
            for (uint32_t r0 = 0; r0 < nrow; r0 += 64) {
                const uint32_t ir = r0 + (uint32_t)lane;
                uint32_t s1 = 0, l1 = 0, s2 = 0, l2 = 0;
                do {
                    if (ir >= nrow) break;
                    const uint32_t it = rows[ir];
                    const int4 bk = flat[it >> 4];
                    const int y = 4 * bk.y + (int)(it & 3), z = 4 * bk.z + (int)((it >> 2) & 3);
                    if (y >= g.n[1] || z >= g.n[2]) break;
                    const double cyz2 = sq_gap(axis_gap<double>(z, cz, lz), mc) + sq_gap(axis_gap<double>(y, cy, ly), mc);
                    if (cyz2 * h2 > v.bound()) break;
                    const bool yzin = abs(z - cz) <= kCellRings && abs(y - cy) <= kCellRings;
                    int xa = 4 * bk.x, xe = min(4 * bk.x + 3, g.n[0] - 1);
                    while (xa <= xe && (cyz2 + sq_gap(axis_gap<double>(xa, cx, lx), mc)) * h2 > v.bound()) xa++;
                    while (xe >= xa && (cyz2 + sq_gap(axis_gap<double>(xe, cx, lx), mc)) * h2 > v.bound()) xe--;
                    if (xa > xe) break;
                    const int64_t rb = g.dense ? dense_id(g, 0, y, z) : (int64_t)bk.w * 64 + local_of(0, y, z);
                    auto range = [&](int x0, int x1, uint32_t& st, uint32_t& len) {  // cells [x0, x1]
                        if (x0 > x1) return;
                        const int64_t c0 = g.dense ? rb + x0 : rb + (x0 & 3);
                        st = g.cstart[c0];
                        len = g.cstart[c0 + (x1 - x0) + 1] - st;
                    };
                    if (yzin) {
                        range(xa, min(xe, cx - kCellRings - 1), s1, l1);
                        range(max(xa, cx + kCellRings + 1), xe, s2, l2);
                    } else {
                        range(xa, xe, s1, l1);
                    }
                } while (false);
                flat_visit(s1, l1, s2, l2);
            }
            wave_lds_fence();  // the next batch rewrites flat[]
            const long long cb2 = tk ? (long long)clock64() : 0;
            if (tk) tk[3] += cb2 - cb1;  // the occupied bricks' rows and points
            // tighten the shared bound mid-shell (the exact k-th is refreshed per shell)
            if (kk <= 64) v.shared = fmin(v.shared, wave_kth_of_bests<K>(v.top, kk, lane));
            if (tk) tk[4] += (long long)clock64() - cb2;
        }
    }
}

// merge the lanes' top-k lists: round r leaves the r-th (d2, j) of the query in lane r's
// (md, mj) (r < kk); every lane must call it
template <int K>
__device__ __forceinline__ void coop_merge(CoopVisitor<K>& v, int kk, int lane, double& md, int& mj) {
    v.top.normalize(kk);
    md = INFINITY;
    mj = INT_MAX;
    for (int r = 0; r < kk; r++) {
        double bd = v.top.best_d();
        int bj = v.top.best_j(), bl = lane;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double od = __shfl_xor(bd, o, 64);
            const int oj = __shfl_xor(bj, o, 64), ol = __shfl_xor(bl, o, 64);
            const bool take = lex_less(od, oj, bd, bj);
            bd = take ? od : bd;
            bj = take ? oj : bj;
            bl = take ? ol : bl;
        }
        if (lane == bl && bj != INT_MAX) v.top.pop_best();
        if (lane == r) { md = bd; mj = bj; }
    }
}

}  // namespace
}  // namespace pcp
