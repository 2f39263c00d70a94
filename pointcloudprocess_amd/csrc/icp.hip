// ICP correspondence/transform loop (replaces the trimesh2 ICP() call inside
// PointCloudHelper::get_rot_icp, point_cloud_helper.cpp:75-166; callers main_blend.cpp:106,
// 818, 887 and point_cloud_closure via main_blend).
//
// Per iteration one fused kernel: transform-on-load of each (spatially sorted) query by
// the current pose (fp32 fmaf chain, the contract in DESIGN.md §ICP), exact 1-NN within
// rmax over the fp32 grid index (ring search, lexicographic (d2, target index)), and the
// 24 double accumulators reduced per wavefront (shuffles) -> per workgroup (LDS) -> one
// fixed-order pass over the workgroup partials.  The host solves the 3x3 Kabsch/Umeyama
// problem (pcp_icp_solve) and composes the pose.
//
// Owned here: the search kernels and their caches, the launch (icp_args, icp_fallback, icp_chain,
// icp_launch), k_make_keys, and the step, run, keys and getter entry points.  The handle is
// icp_handle.hpp's, its creation icp_create.hip's, the pose block's kernels icp_pose.hpp's, the 3x3
// solve icp_solve.hpp's and the loops over exchanged keys icp_shard.hip's.
// The search arithmetic is icp_search.hpp's; the key's layout, the pose cast, the Kabsch terms of
// a pair and the block reductions of the key kernels are icp_pair.hpp's.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "icp_handle.hpp"
#include "icp_pose.hpp"
#include "wave_acc.hpp"

namespace pcp {
namespace {

// sorted query i as {x, y, z, 0}
__device__ __forceinline__ float4 ldq(const IcpArgs& a, int64_t i) {
    const QXyz v = a.q[i];
    return make_float4(v.x, v.y, v.z, 0.f);
}

// The pose and the launch index as the kernels use them: from the handle's pose block.  The test is
// never false (icp_args always sets a.pose).  It is kept for the code it makes: without it the
// register allocation of the search kernels shifts and k_icp_ring takes one more spill slot (36 ->
// 40 B of scratch; profiles/icp_split/stage2_regs.txt).
__device__ __forceinline__ void load_pose(IcpArgs& a) {
    if (a.pose) {
        a.launch = a.pose->launch;
#pragma unroll
        for (int k = 0; k < 9; k++) a.R[k] = a.pose->cur[k];
#pragma unroll
        for (int k = 0; k < 3; k++) a.t[k] = a.pose->cur[9 + k];
    }
}
// the look-ahead map: equal to the pose when beta = 0
__device__ __forceinline__ void load_pose_c(IcpArgs& a) {
#pragma unroll
    for (int k = 0; k < 9; k++) a.Rc[k] = a.pose->c[k];
#pragma unroll
    for (int k = 0; k < 3; k++) a.tc[k] = a.pose->c[9 + k];
}

// Ablation switches for profiling (pcp_icp_set_options, PCP_ICP_ABLATE_*); results are wrong
// when any is set.
constexpr int kDbgNoScan = PCP_ICP_ABLATE_NO_SCAN, kDbgNoAccum = PCP_ICP_ABLATE_NO_ACCUM,
              kDbgNoFallback = PCP_ICP_ABLATE_NO_FALLBACK, kDbgNoVerify = PCP_ICP_ABLATE_NO_VERIFY;

// xform (icp_search.hpp) is q' = R q + t under this launch's pose.  The same chain under the
// look-ahead map: the search centre c (the verify pass rebuilds exactly this from the launch's
// history slot)
__device__ __forceinline__ void xform_c(const IcpArgs& a, const float4 q, float& x, float& y, float& z) {
    xform_rt(a.Rc, a.tc, q, x, y, z);
}

// min / max of non-NaN floats as one v_med3_f32 (fminf/fmaxf add canonicalizing v_max ops)
__device__ __forceinline__ float fmin_nn(float a, float b) { return __builtin_amdgcn_fmed3f(a, b, -INFINITY); }
__device__ __forceinline__ float fmax_nn(float a, float b) { return __builtin_amdgcn_fmed3f(a, b, INFINITY); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ int wave_min_i(int v) {
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

// Main pass (dense grid).  Wave-autonomous, one query per lane: waves take 64-query chunks
// of the spatially sorted query set (grid-stride, so the 4 waves of a workgroup work on
// adjacent chunks and share L1), transform each query, and scan its 2x2x2 "octant" block
// of cells straight from the x-rows of the dense table.  The octant holds every target
// within (0.5 - mc) cells of the query: a winner with d2 <= cert2 is the exact 1-NN, and
// "nothing within rmax" is certified when rmax^2 <= cert2.  Other queries keep their
// provisional octant winner (a valid upper bound for the exact fallback search) and go to
// the wave's fallback segment (ballot + mbcnt, no atomics).
// Accumulators: per chunk, fp32 products centred on the chunk's first query are summed
// across the wave (wave_acc.hpp), un-centred in fp64 and kept in LDS -- no accumulator
// registers, so the kernel fits 8 waves per SIMD.

// Add one chunk's accepted pairs (lanes with ok) to the wave's fp64 accumulators S (LDS):
// fp32 products centred on lane 0's query, summed across the wave and un-centred in fp64
// (wave_acc.hpp: reduce-scatter butterfly, one lane per accumulator).  Every lane of the wave
// must call it (full EXEC).
__device__ __forceinline__ void chunk_accumulate(bool ok, float qx, float qy, float qz, const Best& b,
                                                 double* S, int lane) {
    if (!__ballot(ok)) return;
    const float ccx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qx), 0));
    const float ccy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qy), 0));
    const float ccz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qz), 0));
    const float x0 = ok ? qx - ccx : 0.f, x1 = ok ? qy - ccy : 0.f, x2 = ok ? qz - ccz : 0.f;
    const float p0 = ok ? b.px - ccx : 0.f, p1 = ok ? b.py - ccy : 0.f, p2 = ok ? b.pz - ccz : 0.f;
    const float v[23] = {ok ? 1.f : 0.f, x0, x1, x2, p0, p1, p2,
                         x0 * p0, x0 * p1, x0 * p2, x1 * p0, x1 * p1, x1 * p2, x2 * p0, x2 * p1, x2 * p2,
                         x0 * x0, x0 * x1, x0 * x2, x1 * x1, x1 * x2, x2 * x2, ok ? b.bd : 0.f};
    wave_accumulate(v, S, lane, ccx, ccy, ccz);
}

// XCD-blocked work split: workgroups are dealt round-robin over the 8 XCDs, so workgroup b
// runs on XCD b % 8.  The 64-query chunks [0, nch) are cut into np = min(8, grid) contiguous
// parts, one per XCD, and each part is handed out grid-stride to that XCD's waves: spatially
// adjacent chunks then share one L2 (their cell rows and target points) instead of being
// fetched once per XCD.
struct XcdSplit {
    int64_t c0, c1, w, nw;  // this wave's part [c0, c1), its index and the part's wave count
};
__device__ __forceinline__ XcdSplit xcd_split(int64_t nch, int kW) {
    const int np = min(8, (int)gridDim.x);
    const int part = (int)(blockIdx.x % np);
    const int64_t nblk = ((int64_t)gridDim.x - part + np - 1) / np;  // workgroups of this part
    XcdSplit x;
    x.c0 = part * nch / np;
    x.c1 = (part + 1) * nch / np;
    x.w = (int64_t)(blockIdx.x / np) * kW + (threadIdx.x >> 6);
    x.nw = nblk * kW;
    return x;
}

__device__ __forceinline__ void write_wave_partials(double (*s_acc)[kAcc], double* out) {
    __syncthreads();
    if (threadIdx.x < kAcc) {
        double s = 0.0;
        if (threadIdx.x < kAcc - 1)
            for (int w = 0; w < kIcpBlock / 64; w++) s += s_acc[w][threadIdx.x];
        out[threadIdx.x] = s;
    }
}

// Per-lane accumulation: each lane sums its accepted pairs in fp32, centred on the
// (transformed) first query of the wave's current stretch of chunks, into 23 registers; every
// kFlush chunks (and at the end) the wave reduces them and un-centres the totals in fp64 into
// the wave's LDS accumulators (wave_acc.hpp).  A stretch is at most kFlush * 64
// consecutive sorted queries (a few metres), so the centred fp32 products stay small.
#ifndef PCP_KFLUSH  // chunks per accumulator stretch
#define PCP_KFLUSH 32
#endif
constexpr int kFlush = PCP_KFLUSH;
struct LaneAcc {
    float v[kAcc - 1];  // n, A(3), B(3), AB(9), AA(6), D  (centred on c)
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int k = 0; k < kAcc - 1; k++) v[k] = 0.f;
    }
    __device__ __forceinline__ void add(float qx, float qy, float qz, float px, float py, float pz, float d2,
                                        float cx, float cy, float cz) {
        const float x[3] = {qx - cx, qy - cy, qz - cz}, p[3] = {px - cx, py - cy, pz - cz};
        v[0] += 1.f;
#pragma unroll
        for (int k = 0; k < 3; k++) { v[1 + k] += x[k]; v[4 + k] += p[k]; }
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int k = 0; k < 3; k++) v[7 + 3 * r + k] = __fmaf_rn(x[r], p[k], v[7 + 3 * r + k]);
        v[16] = __fmaf_rn(x[0], x[0], v[16]);
        v[17] = __fmaf_rn(x[0], x[1], v[17]);
        v[18] = __fmaf_rn(x[0], x[2], v[18]);
        v[19] = __fmaf_rn(x[1], x[1], v[19]);
        v[20] = __fmaf_rn(x[1], x[2], v[20]);
        v[21] = __fmaf_rn(x[2], x[2], v[21]);
        v[22] += d2;
    }
    // whole wave (full EXEC): totals -> S (fp64, un-centred).  Always inlined: as a call, the
    // stretch flush spilled a 160 B/lane frame to scratch.
    __device__ __attribute__((always_inline)) void flush(double* S, int lane, float cx, float cy, float cz) {
        wave_accumulate(v, S, lane, cx, cy, cz);
        zero();
    }
};

// ---- candidate cache (a Verlet-style neighbour list per query)
// The search that last settled query i left its record: the positions of its kCache nearest
// targets (or fewer) and D, a lower bound on the distance from the query, at that launch's pose
// q_s, to every target point NOT cached.  With q_t the query at the
// current pose and Delta = |q_t - q_s|, every uncached point p has |q_t - p| >= D - Delta
// (triangle inequality).  So if the nearest cached point is closer than D - Delta (with
// relative margins far above the fp32 rounding of d2), it is the exact 1-NN under the
// contract -- the same (d2, index) winner an exhaustive search returns, cached ties included
// -- and the query is settled without a search; the bound moves to D - Delta.
constexpr int kCache = 3;

// The record (per sorted query; the verify pass streams it every launch):
//   wide   (16 B): {c0, c1, c2, dlb}, dlb = bits(D) & ~0xff | (launch & 255) -- D rounded down to
//                  15 mantissa bits (still a lower bound), the slot of the pose history;
//   narrow (12 B, targets < 2^26 - 2): c0 | x0 << 26, c1 | x1 << 26, c2 | x2 << 26 with the 18-bit
//                  word x = (launch & 63) | code(D) << 6, code(D) = D in units of cell / 1024 as a
//                  4-bit exponent and 8-bit mantissa, rounded down (0: D < 1 unit; 0xfff caps D at
//                  ~32 cells).  An empty slot is 2^26 - 1 (above every position and the sentinel).
// A smaller D only sends more queries to the search, so every rounding is down.
struct CacheRec {
    uint32_t c0, c1, c2;  // positions, ~0u = empty slot
    uint32_t slot;        // launch of the search & hist_mask
    float D;
};
__device__ __forceinline__ uint32_t dcode12(float D, float inv_unit) {
    const float x = D * inv_unit;
    if (!(x >= 1.f)) return 0u;
    const uint32_t b = __float_as_uint(x);
    const uint32_t e = (b >> 23) - 127u;
    return e >= 15u ? 0xfffu : ((e + 1u) << 8) | ((b >> 15) & 0xffu);
}
__device__ __forceinline__ float ddecode12(uint32_t c, float unit) {
    return c ? __uint_as_float((((c >> 8) + 126u) << 23) | ((c & 0xffu) << 15)) * unit : 0.f;
}
// the raw words of record i (narrow: .w unused)
__device__ __forceinline__ uint4 cache_raw(const IcpArgs& a, int64_t i) {
    if (a.narrow) {
        const uint3 w = *(const uint3*)(a.cand + 3 * i);
        return make_uint4(w.x, w.y, w.z, 0u);
    }
    return ((const uint4*)a.cand)[i];
}
__device__ __forceinline__ CacheRec cache_dec(const IcpArgs& a, const uint4 w) {
    CacheRec r;
    if (a.narrow) {
        auto pos = [](uint32_t v) { const uint32_t c = v & kPos26; return c == kPos26 ? ~0u : c; };
        r.c0 = pos(w.x);
        r.c1 = pos(w.y);
        r.c2 = pos(w.z);
        const uint32_t x = (w.x >> 26) | ((w.y >> 26) << 6) | ((w.z >> 26) << 12);
        r.slot = x & 63u;
        r.D = ddecode12(x >> 6, a.dunit);
    } else {
        r.c0 = w.x;
        r.c1 = w.y;
        r.c2 = w.z;
        r.slot = w.w & 0xffu;
        r.D = __uint_as_float(w.w & ~0xffu);
    }
    return r;
}
__device__ __forceinline__ CacheRec cache_load(const IcpArgs& a, int64_t i) { return cache_dec(a, cache_raw(a, i)); }
__device__ __forceinline__ void cache_store(const IcpArgs& a, int64_t i, uint32_t c0, uint32_t c1, uint32_t c2, float D,
                                            uint32_t launch) {
    if (a.narrow) {
        auto pos = [](uint32_t c) { return c == ~0u ? kPos26 : c; };
        const uint32_t x = (launch & 63u) | (dcode12(D, a.inv_dunit) << 6);
        *(uint3*)(a.cand + 3 * i) =
            make_uint3(pos(c0) | ((x & 63u) << 26), pos(c1) | (((x >> 6) & 63u) << 26), pos(c2) | ((x >> 12) << 26));
    } else {
        ((uint4*)a.cand)[i] = make_uint4(c0, c1, c2, (__float_as_uint(fmaxf(D, 0.f)) & ~0xffu) | (launch & 0xffu));
    }
}

// the cached candidates' winner under the current pose, by (d2, target index)
struct CacheBest {
    float bd = INFINITY;
    int bj = 0x7fffffff;
    uint32_t bk = ~0u;
    float4 P = make_float4(0.f, 0.f, 0.f, 0.f);
};
__device__ __forceinline__ CacheBest cache_best(const float4* tp, const CacheRec& cd, float qx, float qy, float qz) {
    const uint32_t c[3] = {cd.c0, cd.c1, cd.c2};
    float4 p[kCache];
#pragma unroll
    for (int s = 0; s < kCache; s++) p[s] = c[s] != ~0u ? tp[c[s]] : make_float4(0.f, 0.f, 0.f, 0.f);
    CacheBest r;
#pragma unroll
    for (int s = 0; s < kCache; s++) {
        if (c[s] == ~0u) continue;
        const float d2 = icp_d2(qx, qy, qz, p[s]);
        const int id = __float_as_int(p[s].w);
        if (d2 < r.bd || (d2 == r.bd && id < r.bj)) {
            r.bd = d2;
            r.bj = id;
            r.bk = c[s];
            r.P = p[s];
        }
    }
    return r;
}

// 16-byte record of a table by element index.  The byte offset is 32-bit (so the load can use
// the saddr + 32-bit VGPR offset form): pcp_icp_check_sizes() keeps every table this reads
// (the fp32 target incl. its far sentinel) below 2^28 records = 4 GB.
template <typename V>
__device__ __forceinline__ V ld16(const V* base, uint32_t idx) {
    return *(const V*)((const char*)base + (size_t)(idx * 16u));
}

// ---- verify pass (every query, every launch after the first)
// Settles a query from its cache (above): q_s is recomputed exactly from the pose of the
// launch s that searched it (pose history in LDS), so the bound is |q_t - q_s| (not a sum of
// steps) and nothing is written for a settled query.  "No correspondence" is settled the same
// way when the nearest cached point is beyond rmax.  Everything else goes to the search list
// (per-wave segments, compacted afterwards).  Wave w owns the contiguous chunk range
// [w*nch/nwaves, (w+1)*nch/nwaves) of the sorted queries; accumulation is per lane (fp32,
// centred on the stretch's first query).
__global__ void __launch_bounds__(kIcpBlock, PCP_VER_WAVES) k_icp_verify(IcpArgs a) {
    __shared__ float4 s_pose[kHist][3];
    constexpr int kW = kIcpBlock / 64;
    __shared__ double s_acc[kW][kAcc];
    for (int k = threadIdx.x; k < kHist * 3; k += blockDim.x)
        s_pose[k / 3][k % 3] = ((const float4*)a.pose_hist)[k];
    load_pose(a);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t gw = (int64_t)blockIdx.x * kW + wid;
    const int64_t nch = (a.nq + 63) / 64;
    // contiguous ranges: wave w owns chunks [w*nch/nwaves, (w+1)*nch/nwaves)
    const int64_t nwaves = (int64_t)gridDim.x * kW;
    const int64_t cstart_ = gw * nch / nwaves;
    const int64_t nsteps = (gw + 1) * nch / nwaves - cstart_;
    if (lane < kAcc) s_acc[wid][lane] = 0.0;
    __syncthreads();
    uint32_t svn = 0;
    LaneAcc acc;
    acc.zero();
    const float r2m = a.r2 * 1.0003f;
    // software pipeline: the query, cache and bound words two chunks ahead, the cached points'
    // gathers one chunk ahead (this chunk's were issued during the previous one)
    const uint4 none = make_uint4(~0u, ~0u, ~0u, ~0u);
    auto raw = [&](int64_t k, float4& q, uint4& cd) {
        const int64_t i = (cstart_ + k) * 64 + lane;
        if (k < nsteps && i < a.nq) {
            q = ldq(a, i);
            cd = cache_raw(a, i);
        } else {
            q = make_float4(0.f, 0.f, 0.f, 0.f);
            cd = none;
            cd.w = 0u;
        }
    };
    auto gather = [&](const uint4 cd, float4& p0, float4& p1, float4& p2) {
        // an empty slot reads the far sentinel tp[ntp]: d2 = inf
        const CacheRec r = cache_dec(a, cd);
        p0 = ld16(a.tp, min(r.c0, a.ntp));
        p1 = ld16(a.tp, min(r.c1, a.ntp));
        p2 = ld16(a.tp, min(r.c2, a.ntp));
    };
    float4 q1, q2;
    uint4 c1_, c2_;
    float4 g0, g1, g2;
    raw(0, q1, c1_);
    raw(1, q2, c2_);
    gather(c1_, g0, g1, g2);
    for (int64_t k0 = 0; k0 < nsteps; k0 += kFlush) {  // stretches of kFlush chunks
        const int64_t k1 = min(k0 + (int64_t)kFlush, nsteps);
        // centre: the stretch's first query under the current pose (wave-uniform)
        float ccx, ccy, ccz;
        xform(a, ldq(a, (cstart_ + k0) * 64), ccx, ccy, ccz);
        ccx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ccx)));
        ccy = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ccy)));
        ccz = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ccz)));
        for (int64_t k = k0; k < k1; k++) {
            const int64_t i = (cstart_ + k) * 64 + lane;
            const bool valid = i < a.nq;
            const float4 qq = q1;
            const CacheRec rec = cache_dec(a, c1_);
            const float4 p0 = g0, p1 = g1, p2 = g2;
            // issue chunk c+1's gathers and chunk c+2's words before using chunk c's
            gather(c2_, g0, g1, g2);
            q1 = q2;
            c1_ = c2_;
            raw(k + 2, q2, c2_);
            float qx, qy, qz;
            xform(a, qq, qx, qy, qz);
            // winner among the cached points by (d2, target index); an empty slot never wins
            float m = INFINITY, px = 0.f, py = 0.f, pz = 0.f;
            int mj = 0x7fffffff;
            auto take = [&](const float4 p) {
                const float e = icp_d2(qx, qy, qz, p);
                const int id = __float_as_int(p.w);
                const bool t = e < m || (e == m && id < mj);
                m = t ? e : m;
                mj = t ? id : mj;
                px = t ? p.x : px;
                py = t ? p.y : py;
                pz = t ? p.z : pz;
            };
            take(p0);
            take(p1);
            take(p2);
            // the query at the pose of its last search
            const uint32_t sl = rec.slot;
            const float4 A = s_pose[sl][0], B = s_pose[sl][1], C = s_pose[sl][2];
            const float ex = qx - __fmaf_rn(A.z, qq.z, __fmaf_rn(A.y, qq.y, __fmaf_rn(A.x, qq.x, C.y)));
            const float ey = qy - __fmaf_rn(B.y, qq.z, __fmaf_rn(B.x, qq.y, __fmaf_rn(A.w, qq.x, C.z)));
            const float ez = qz - __fmaf_rn(C.x, qq.z, __fmaf_rn(B.w, qq.y, __fmaf_rn(B.z, qq.x, C.w)));
            const float delta = sqrtf(__fmaf_rn(ez, ez, __fmaf_rn(ey, ey, ex * ex))) * 1.00001f + 1e-7f;
            const float lb = rec.D * 0.99998f - delta;  // every uncached point is >= lb
            // the nearest cached point is the exact 1-NN (it beats lb), or nothing is within rmax
            const float thr = fminf(m * 1.0003f, r2m);
            bool ok = valid && ((a.launch - sl) & a.hist_mask) < a.max_age && lb > 0.f && thr + 1e-12f < lb * lb;
            ok = ok && !(a.dbg & kDbgNoVerify);
            const bool srch = valid && !ok;
            const uint64_t msk = __ballot(srch);
            if (srch) {
                const uint32_t pos = svn + __builtin_amdgcn_mbcnt_hi((uint32_t)(msk >> 32),
                                                                   __builtin_amdgcn_mbcnt_lo((uint32_t)msk, 0u));
                a.sv[gw * a.sv_seg + pos] = (int32_t)i;
            }
            svn += (uint32_t)__popcll(msk);
            if (ok && m <= a.r2 && !(a.dbg & kDbgNoAccum)) acc.add(qx, qy, qz, px, py, pz, m, ccx, ccy, ccz);
        }
        acc.flush(s_acc[wid], lane, ccx, ccy, ccz);
    }
    if (lane == 0) {
        a.sv_count[gw] = svn;
    }
    write_wave_partials(s_acc, a.partials + (int64_t)blockIdx.x * kAcc);
}

// running 3-NN (kCache = 3): d0 <= d1 <= d2 with positions, d3 = the 4th smallest d2 scanned
struct Top3 {
    float d0 = INFINITY, d1 = INFINITY, d2 = INFINITY, d3 = INFINITY;
    uint32_t p0 = ~0u, p1 = ~0u, p2 = ~0u;
    // insertion as three independent compare-swaps from the bottom (flat selects: a nested
    // select form was lowered to branches and register moves)
    __device__ __forceinline__ void consider(float qx, float qy, float qz, const float4 p, uint32_t k) {
        float x = icp_d2(qx, qy, qz, p);
        uint32_t kx = k;
        cswap(d2, p2, x, kx);
        d3 = fmin_nn(d3, x);  // what fell out of the top 3
        cswap(d1, p1, d2, p2);
        cswap(d0, p0, d1, p1);
    }
    // (a, pa) <- the smaller of (a, pa), (b, pb) by d2; (b, pb) <- the larger (ties keep a)
    __device__ __forceinline__ static void cswap(float& a, uint32_t& pa, float& b, uint32_t& pb) {
        const bool t = b < a;
        const float lo = fmin_nn(a, b), hi = fmax_nn(a, b);
        const uint32_t ql = t ? pb : pa, qh = t ? pa : pb;
        a = lo;
        b = hi;
        pa = ql;
        pb = qh;
    }
    __device__ __forceinline__ void scan4(const float4* pts, const uint32_t (&rs)[4], const uint32_t (&rn)[4],
                                          float qx, float qy, float qz) {
        const uint32_t c1 = rn[0], c2 = c1 + rn[1], c3 = c2 + rn[2], L = c3 + rn[3];
        const uint32_t o0 = rs[0], o1 = rs[1] - c1, o2 = rs[2] - c2, o3 = rs[3] - c3;
        auto addr = [=](uint32_t v) { return cat_addr(v, c1, c2, c3, o0, o1, o2, o3); };
        constexpr int U = PCP_SCAN_UNROLL;
        uint32_t v = 0;
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
};

// running 3-NN on packed keys: key = (bits(d2) & ~255) | v, v the candidate's index in the
// concatenated octant list (< 256).  Non-negative floats order like their bits, so a
// v_med3_u32 network keeps the 4 smallest keys -- values and list indices together -- in 4 VALU
// ops per candidate (the compare-swap form, Top3, needs 16).  The truncated d2 only chooses
// WHICH points are cached: the winner among them is decided on the exact d2 afterwards, and
// the 4th key with its low byte cleared bounds the d2 of every scanned point not kept (an
// uncached point's key is >= t3, so its d2 bits are >= t3 & ~255).
constexpr uint32_t kKeyMax = 0x7f7fffffu;  // FLT_MAX: above every real key
constexpr uint32_t kMaxOctList = 256;       // list indices that fit the key's low byte
// median of three u32 (one v_med3_u32; the float form adds canonicalizing ops on bit-cast keys)
__device__ __forceinline__ uint32_t umed3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// position of candidate v of the concatenated rows, or the far sentinel `sent` past the list
__device__ __forceinline__ uint32_t cat_addr_l(uint32_t v, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t L,
                                               uint32_t o0, uint32_t o1, uint32_t o2, uint32_t o3, uint32_t sent) {
    const uint32_t d = v < L ? o3 : sent - v;
    const uint32_t c = v < c3 ? o2 : d;
    const uint32_t b = v < c2 ? o1 : c;
    return v + (v < c1 ? o0 : b);
}
__device__ __forceinline__ int wave_max_u(int v) {
    v = max(v, __shfl_xor(v, 1, 64));
    v = max(v, __shfl_xor(v, 2, 64));
    v = max(v, __shfl_xor(v, 4, 64));
    v = max(v, __shfl_xor(v, 8, 64));
    v = max(v, __shfl_xor(v, 16, 64));
    v = max(v, __shfl_xor(v, 32, 64));
    return v;
}
// A look-ahead search ranks every candidate twice: by its distance to the search centre c (Top3P:
// what is cached) and by its distance to the query at this launch's pose q_t (Min2P: this
// launch's own result).  Min2P keeps the 2 smallest packed keys at q_t.  When their d2 bits differ
// above the low byte the first is the strict minimum over the scanned points, so the exact
// (d2, index) winner; otherwise (a tie or a near-tie within 256 ulps) the query is left to the
// exact fallback pass.
struct Min2P {
    uint32_t u0 = kKeyMax, u1 = kKeyMax;
    __device__ __forceinline__ void consider(float qx, float qy, float qz, const float4 p, uint32_t v) {
        const uint32_t x = (__float_as_uint(icp_d2(qx, qy, qz, p)) & ~0xffu) | v;
        u1 = umed3(u0, u1, x);
        u0 = min(u0, x);
    }
};
struct Top3P {
    uint32_t t0 = kKeyMax, t1 = kKeyMax, t2 = kKeyMax, t3 = kKeyMax;
    __device__ __forceinline__ void consider(float qx, float qy, float qz, const float4 p, uint32_t v) {
        const float d = icp_d2(qx, qy, qz, p);
        const uint32_t x = (__float_as_uint(d) & ~0xffu) | v;
        t3 = umed3(t2, t3, x);
        t2 = umed3(t1, t2, x);
        t1 = umed3(t0, t1, x);
        t0 = min(t0, x);
    }
    // the wave's lists with a uniform trip count Lg = ceil(longest list / G), rounded up to whole
    // batches of U loads and no further (lanes past their own list read the far sentinel: d2 = inf,
    // never kept), the next batch's loads issued before this batch's keys are formed (software
    // pipeline: two batches in flight wherever a next batch exists).  With G lanes per
    // query, lane `sub` of the group takes list entries sub, sub + G, sub + 2G, ...: the group's
    // loads of one step are G consecutive records of a row (one or two cache lines), so a wave
    // instruction touches ~64 / G lines instead of 64 (what bounds the sparse search lists).
    // LOOK: (qx, qy, qz) is the search centre c, and every candidate is also ranked at the query's
    // current position (tx, ty, tz) into m2 (same loads, a second distance).
    template <int G, bool LOOK = false>
    __device__ __forceinline__ void scan4(const float4* pts, uint32_t sent, const uint32_t (&rs)[4],
                                          const uint32_t (&rn)[4], uint32_t Lw, float qx, float qy, float qz,
                                          uint32_t sub, Min2P* m2 = nullptr, float tx = 0.f, float ty = 0.f,
                                          float tz = 0.f) {
        const uint32_t c1 = rn[0], c2 = c1 + rn[1], c3 = c2 + rn[2], L = c3 + rn[3];
        const uint32_t o0 = rs[0], o1 = rs[1] - c1, o2 = rs[2] - c2, o3 = rs[3] - c3;
        auto lv = [=](uint32_t v) { return v * G + sub; };  // this lane's v-th list entry
        auto addr = [=](uint32_t v) { return cat_addr_l(lv(v), c1, c2, c3, L, o0, o1, o2, o3, sent); };
        const uint32_t Lg = (Lw + G - 1) / G;
        if (Lg == 0) return;  // a chunk of empty lists loads nothing
        constexpr int U = 4;
        float4 A[U], B[U];
        auto load = [&](float4 (&R)[U], uint32_t v) {
#pragma unroll
            for (int u = 0; u < U; u++) R[u] = ld16(pts, addr(v + u));
        };
        auto rank = [&](const float4 (&R)[U], uint32_t v) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                consider(qx, qy, qz, R[u], lv(v + u));
                if constexpr (LOOK) m2->consider(tx, ty, tz, R[u], lv(v + u));
            }
        };
        // two register sets, no copies: the next batch's loads are in flight while this batch's
        // keys are formed.  No batch is issued at or past Lg (Lg is wave-uniform: scalar
        // branches).  The loop has one exit and runs only while both of its batches exist; the last
        // one or two batches are ranked on paths of their own, so the wait before a ranking counts
        // the same loads in flight on every path into it.  (A load skipped under a branch that
        // joins before the ranking makes that wait a full one: the join takes the stricter count.)
        load(A, 0);
        uint32_t v = 0;
        for (; v + 2 * U < Lg; v += 2 * U) {  // batches v + U and v + 2U both exist
            load(B, v + U);
            __builtin_amdgcn_sched_barrier(0);  // keep B's loads ahead of A's keys
            rank(A, v);
            load(A, v + 2 * U);
            __builtin_amdgcn_sched_barrier(0);
            rank(B, v + U);
        }
        if (v + U < Lg) {  // two batches left
            load(B, v + U);
            __builtin_amdgcn_sched_barrier(0);
            rank(A, v);
            rank(B, v + U);
        } else {
            rank(A, v);
        }
    }
    // the G lanes of a query merge their 4 smallest keys: per butterfly step the 4 smallest of
    // two ascending lists are min(t_i, u_{3-i}) (a bitonic sequence), sorted by two stages of
    // compare-exchange.  Keys of one query are distinct (the list index is in the low byte)
    // except kKeyMax.  Afterwards every lane of the group holds the group's t0..t3.
    template <int G>
    __device__ __forceinline__ void merge_group() {
#pragma unroll
        for (int s = 1; s < G; s <<= 1) {
            const uint32_t u0 = xor_lane(t0, s), u1 = xor_lane(t1, s), u2 = xor_lane(t2, s), u3 = xor_lane(t3, s);
            const uint32_t c0 = min(t0, u3), c1 = min(t1, u2), c2 = min(t2, u1), c3 = min(t3, u0);
            const uint32_t l02 = min(c0, c2), h02 = max(c0, c2), l13 = min(c1, c3), h13 = max(c1, c3);
            t0 = min(l02, l13);
            t1 = max(l02, l13);
            t2 = min(h02, h13);
            t3 = max(h02, h13);
        }
    }
    // lane ^ s inside a quad by DPP quad_perm (s = 1, 2), else a bpermute
    __device__ __forceinline__ static uint32_t xor_lane(uint32_t v, int s) {
        if (s == 1) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, false);  // [1,0,3,2]
        if (s == 2) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xf, 0xf, false);  // [2,3,0,1]
        return (uint32_t)__shfl_xor((int)v, s, 64);
    }
};

// ---- search pass (the verify pass's list; every query at the first launch)
// One query per lane, 64-query chunks grid-stride over the list.  Each query scans its whole
// 2x2x2 "octant" block of cells (the four x-rows [floor(f - 1/2), +1]) keeping its 3 nearest.
// The octant holds every target within m = the query's distance to its faces (>= 1/2 cell,
// less the margin).  The nearest is the exact 1-NN when d0 <= m^2 and d0 < d3 (every point
// tied with it is cached, and the cache order by index decides); "nothing within rmax" is
// certified when rmax <= m.  The cache is refreshed either way (D = min(d3, m) bounds every
// uncached point); unsettled queries go to the fallback list.
//
// The scan keeps packed (d2, list index) keys (Top3P, 4 VALU ops per candidate) with a
// wave-uniform trip count; a chunk with a list longer than 256 candidates (the key's low byte)
// uses the compare-swap form (Top3).  Both end in the same OctResult: the exact (d2, index)
// winner among the 3 kept, its coordinates, the 3 cached positions and the first-uncached bound.
struct OctResult {
    float d0 = INFINITY;       // exact d2 of the winner among the kept points
    uint32_t win = ~0u;        // its sorted position (~0u: nothing scanned)
    float wx = 0.f, wy = 0.f, wz = 0.f;
    uint32_t c0 = ~0u, c1 = ~0u, c2 = ~0u;  // the cache: positions of the 3 kept points
    float dnext = INFINITY;    // lower bound on the d2 of every scanned point not kept
    bool uniq = false;         // look-ahead scans: d0 / win are this launch's exact winner
    float d1t = 0.f;           // look-ahead scans: lower bound on the d2 AT q_t of every scanned point but win
};

__device__ __forceinline__ void take_exact(OctResult& o, const float4 p, uint32_t pos, float qx, float qy, float qz,
                                           int& wj) {
    const float e = icp_d2(qx, qy, qz, p);
    const int id = __float_as_int(p.w);
    const bool t = pos != ~0u && (e < o.d0 || (e == o.d0 && id < wj));
    o.d0 = t ? e : o.d0;
    wj = t ? id : wj;
    o.win = t ? pos : o.win;
    o.wx = t ? p.x : o.wx;
    o.wy = t ? p.y : o.wy;
    o.wz = t ? p.z : o.wz;
}

// v of lane (group base + src) of this lane's G-lane group (groups of G consecutive lanes; G = 2
// and 4 by DPP quad permutes, inside the quad, no LDS)
template <int G>
__device__ __forceinline__ uint32_t grp_bcast(uint32_t v, int src) {
    if constexpr (G == 1) return v;
    if constexpr (G == 2) {  // quad_perm [s, s, 2 + s, 2 + s]
        return src == 0 ? (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0 | 0 << 2 | 2 << 4 | 2 << 6, 0xf, 0xf, false)
                        : (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 1 | 1 << 2 | 3 << 4 | 3 << 6, 0xf, 0xf, false);
    }
    if constexpr (G == 4) {  // quad_perm [s, s, s, s]
        switch (src) {
            case 0: return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x00, 0xf, 0xf, false);
            case 1: return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x55, 0xf, 0xf, false);
            case 2: return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xAA, 0xf, 0xf, false);
            default: return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xFF, 0xf, 0xf, false);
        }
    }
    const int lane = (int)(threadIdx.x & 63);
    return (uint32_t)__shfl((int)v, (lane & ~(G - 1)) | src, 64);
}
template <int G>
__device__ __forceinline__ uint32_t grp_xor(uint32_t v, int s) {
    if (s == 1) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, false);  // [1,0,3,2]
    if (s == 2) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xf, 0xf, false);  // [2,3,0,1]
    return (uint32_t)__shfl_xor((int)v, s, 64);
}

// The octant's 4 x-rows (y = by + (r & 1), z = bz + (r >> 1), cells [xa, xb], xb - xa + 1 = 1 or
// 2): each row's point range [rs, rs + rn) from the cell starts.  A row's start and end are two
// of the three consecutive words at its first cell, loaded as one 12-byte vector (the cell table
// carries a pad word past its end for that).  With G lanes per query the group's lanes load
// different rows (lane sub: rows sub, sub + G, ...) and exchange them inside the group, so a wave
// issues 4 / G row loads instead of 8 (the loads of a sparse search list each touch a line per
// query: what bounds those launches, TA busy ~75 %).
template <int G>
__device__ __forceinline__ void octant_rows(const GridDesc& g, bool scanq, int bx, int by, int bz, uint32_t sub,
                                            uint32_t (&rs)[4], uint32_t (&rn)[4]) {
    const int xa = max(bx, 0), xb = min(bx + 1, g.n[0] - 1);
    constexpr int PER = G >= 4 ? 1 : 4 / G;  // rows this lane loads
    uint32_t ls[PER], le[PER];
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int r = (int)sub + k * G;
        const int y = by + (r & 1), z = bz + (r >> 1);
        const bool in = scanq && r < 4 && xa <= xb && y >= 0 && y < g.n[1] && z >= 0 && z < g.n[2];
        uint3 t = make_uint3(0u, 0u, 0u);
        if (in) t = *(const uint3*)(g.cstart + dense_id(g, xa, y, z));
        ls[k] = t.x;
        le[k] = xb > xa ? t.z : t.y;
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t s0 = G == 1 ? ls[r] : grp_bcast<G>(ls[(r / G) % PER], r % G);
        const uint32_t e0 = G == 1 ? le[r] : grp_bcast<G>(le[(r / G) % PER], r % G);
        rs[r] = s0;
        rn[r] = e0 - s0;
    }
}

// packed-key scan (every lane's list < 256 candidates); G lanes per query share its list.  The
// exact re-rank of the 3 kept points: with G > 1 the group's lanes gather different kept points
// and reduce the exact (d2, index) winner inside the group (1 or 2 gathers per lane, not 3).
template <int G>
__device__ __forceinline__ OctResult octant_packed(const IcpArgs& a, const uint32_t (&rs)[4], const uint32_t (&rn)[4],
                                                   uint32_t Lw, float qx, float qy, float qz, uint32_t sub) {
    Top3P k;
    k.scan4<G>(a.tp, a.ntp, rs, rn, Lw, qx, qy, qz, sub);
    k.merge_group<G>();
    const uint32_t c1 = rn[0], c2 = c1 + rn[1], c3 = c2 + rn[2], L = c3 + rn[3];
    const uint32_t o0 = rs[0], o1 = rs[1] - c1, o2 = rs[2] - c2, o3 = rs[3] - c3;
    OctResult o;
    o.c0 = k.t0 != kKeyMax ? cat_addr_l(k.t0 & 0xffu, c1, c2, c3, L, o0, o1, o2, o3, a.ntp) : ~0u;
    o.c1 = k.t1 != kKeyMax ? cat_addr_l(k.t1 & 0xffu, c1, c2, c3, L, o0, o1, o2, o3, a.ntp) : ~0u;
    o.c2 = k.t2 != kKeyMax ? cat_addr_l(k.t2 & 0xffu, c1, c2, c3, L, o0, o1, o2, o3, a.ntp) : ~0u;
    int wj = 0x7fffffff;
    if constexpr (G == 1) {
        const float4 p0 = ld16(a.tp, min(o.c0, a.ntp)), p1 = ld16(a.tp, min(o.c1, a.ntp)),
                     p2 = ld16(a.tp, min(o.c2, a.ntp));
        take_exact(o, p0, o.c0, qx, qy, qz, wj);
        take_exact(o, p1, o.c1, qx, qy, qz, wj);
        take_exact(o, p2, o.c2, qx, qy, qz, wj);
    } else {
        constexpr int PER = G >= 3 ? 1 : 2;  // kept points per lane: G = 2: lane 0 {c0, c2}, lane 1 {c1}
#pragma unroll
        for (int s = 0; s < PER; s++) {
            const uint32_t kslot = sub + (uint32_t)(s * G);
            const uint32_t c = kslot == 0 ? o.c0 : (kslot == 1 ? o.c1 : (kslot == 2 ? o.c2 : ~0u));
            take_exact(o, ld16(a.tp, min(c, a.ntp)), c, qx, qy, qz, wj);
        }
        // the group's winner by (d2, index): butterfly over the group (every lane ends with it)
#pragma unroll
        for (int m = 1; m < G; m <<= 1) {
            const float od = __uint_as_float(grp_xor<G>(__float_as_uint(o.d0), m));
            const int oj = (int)grp_xor<G>((uint32_t)wj, m);
            const uint32_t ow = grp_xor<G>(o.win, m);
            const float ox = __uint_as_float(grp_xor<G>(__float_as_uint(o.wx), m));
            const float oy = __uint_as_float(grp_xor<G>(__float_as_uint(o.wy), m));
            const float oz = __uint_as_float(grp_xor<G>(__float_as_uint(o.wz), m));
            const bool t = ow != ~0u && (o.win == ~0u || od < o.d0 || (od == o.d0 && oj < wj));
            o.d0 = t ? od : o.d0;
            wj = t ? oj : wj;
            o.win = t ? ow : o.win;
            o.wx = t ? ox : o.wx;
            o.wy = t ? oy : o.wy;
            o.wz = t ? oz : o.wz;
        }
    }
    o.dnext = k.t3 == kKeyMax ? INFINITY : __uint_as_float(k.t3 & ~0xffu);
    return o;
}

// Look-ahead form of the two scans: the cache (c0..c2, dnext) ranks by the distance to the search
// centre (cx, cy, cz); the winner (d0, win, w*) is this launch's own result, the nearest scanned
// point to the query's current position (qx, qy, qz).  o.uniq: d0 is exact and strictly below every
// other scanned point's d2 (packed form) or the (d2, index) winner (compare-swap form); without it
// d0 is only a lower bound and the query goes to the fallback.  The scatter / key kernels and the
// fallback read this launch's winner from the cache, so a winner that is not among the 3 nearest
// to c takes the third's place, and that point's distance then bounds the uncached ones.
template <int G>
__device__ __forceinline__ OctResult octant_packed_la(const IcpArgs& a, const uint32_t (&rs)[4],
                                                      const uint32_t (&rn)[4], uint32_t Lw, float cx, float cy, float cz,
                                                      float qx, float qy, float qz, uint32_t sub) {
    Top3P k;
    Min2P m;
    k.scan4<G, true>(a.tp, a.ntp, rs, rn, Lw, cx, cy, cz, sub, &m, qx, qy, qz);
    k.merge_group<G>();
#pragma unroll
    for (int s = 1; s < G; s <<= 1) {  // the group's 2 smallest (keys of one query are distinct)
        const uint32_t o0 = Top3P::xor_lane(m.u0, s), o1 = Top3P::xor_lane(m.u1, s);
        const uint32_t hi = max(m.u0, o0);
        m.u0 = min(m.u0, o0);
        m.u1 = min(hi, min(m.u1, o1));
    }
    const uint32_t c1 = rn[0], c2 = c1 + rn[1], c3 = c2 + rn[2], L = c3 + rn[3];
    const uint32_t o0 = rs[0], o1 = rs[1] - c1, o2 = rs[2] - c2, o3 = rs[3] - c3;
    OctResult o;
    o.c0 = k.t0 != kKeyMax ? cat_addr_l(k.t0 & 0xffu, c1, c2, c3, L, o0, o1, o2, o3, a.ntp) : ~0u;
    o.c1 = k.t1 != kKeyMax ? cat_addr_l(k.t1 & 0xffu, c1, c2, c3, L, o0, o1, o2, o3, a.ntp) : ~0u;
    o.c2 = k.t2 != kKeyMax ? cat_addr_l(k.t2 & 0xffu, c1, c2, c3, L, o0, o1, o2, o3, a.ntp) : ~0u;
    o.dnext = k.t3 == kKeyMax ? INFINITY : __uint_as_float(k.t3 & ~0xffu);
    const bool any = m.u0 != kKeyMax;
    o.uniq = any && (m.u1 & ~0xffu) > (m.u0 & ~0xffu);
    o.d0 = any ? __uint_as_float(m.u0 & ~0xffu) : INFINITY;
    o.d1t = __uint_as_float(m.u1 & ~0xffu);  // every other scanned point's key is >= u1 (FLT_MAX: none)
    if (any) {
        const uint32_t w = cat_addr_l(m.u0 & 0xffu, c1, c2, c3, L, o0, o1, o2, o3, a.ntp);
        if (w != o.c0 && w != o.c1 && w != o.c2) {  // (then 4 or more were scanned: t2 is a real key)
            o.c2 = w;
            o.dnext = __uint_as_float(k.t2 & ~0xffu);
        }
        const float4 p = ld16(a.tp, w);  // every lane of the group: one address
        o.win = w;
        o.wx = p.x;
        o.wy = p.y;
        o.wz = p.z;
        if (o.uniq) o.d0 = icp_d2(qx, qy, qz, p);
    }
    return o;
}

// running (d2, index) winner of the compare-swap scan at the query's current position
__device__ __noinline__ OctResult octant_exact_la(const IcpArgs& a, uint32_t rs0, uint32_t rs1, uint32_t rs2,
                                                  uint32_t rs3, uint32_t rn0, uint32_t rn1, uint32_t rn2, uint32_t rn3,
                                                  float cx, float cy, float cz, float qx, float qy, float qz) {
    const uint32_t rs[4] = {rs0, rs1, rs2, rs3}, rn[4] = {rn0, rn1, rn2, rn3};
    struct {
        Top3 b;
        Best w{INFINITY, 0x7fffffff, ~0u, 0.f, 0.f, 0.f};
    } t;
    for (int r = 0; r < 4; r++)
        for (uint32_t k = rs[r]; k < rs[r] + rn[r]; k++) {
            const float4 p = ld16(a.tp, k);
            t.b.consider(cx, cy, cz, p, k);
            t.w.consider(qx, qy, qz, p, k);
        }
    OctResult o;
    o.c0 = t.b.p0;
    o.c1 = t.b.p1;
    o.c2 = t.b.p2;
    o.dnext = t.b.d3;
    o.uniq = t.w.bk != ~0u;
    if (o.uniq) {
        if (t.w.bk != o.c0 && t.w.bk != o.c1 && t.w.bk != o.c2) {
            o.c2 = t.w.bk;
            o.dnext = t.b.d2;
        }
        t.w.fetch(a.tp);
        o.d0 = t.w.bd;
        o.win = t.w.bk;
        o.wx = t.w.px;
        o.wy = t.w.py;
        o.wz = t.w.pz;
    }
    return o;
}

// compare-swap scan (a chunk with a list of 256 or more candidates)
__device__ __noinline__ OctResult octant_exact(const IcpArgs& a, uint32_t rs0, uint32_t rs1, uint32_t rs2, uint32_t rs3,
                                               uint32_t rn0, uint32_t rn1, uint32_t rn2, uint32_t rn3, float qx, float qy,
                                               float qz) {
    const uint32_t rs[4] = {rs0, rs1, rs2, rs3}, rn[4] = {rn0, rn1, rn2, rn3};
    Top3 b;
    b.scan4(a.tp, rs, rn, qx, qy, qz);
    OctResult o;
    o.c0 = b.p0;
    o.c1 = b.p1;
    o.c2 = b.p2;
    const float4 p0 = ld16(a.tp, min(b.p0, a.ntp)), p1 = ld16(a.tp, min(b.p1, a.ntp)), p2 = ld16(a.tp, min(b.p2, a.ntp));
    int wj = 0x7fffffff;
    take_exact(o, p0, o.c0, qx, qy, qz, wj);
    take_exact(o, p1, o.c1, qx, qy, qz, wj);
    take_exact(o, p2, o.c2, qx, qy, qz, wj);
    o.dnext = b.d3;
    return o;
}

// G lanes per query (G = 1: one query per lane; G > 1: the G lanes of a group split the query's
// list, merge their keys, and only the group's first lane writes, accumulates and lists).  A
// chunk is 64 / G queries.  G > 1 serves the sparse search lists of later launches, whose
// lanes no longer share candidate lines.
constexpr int kOctW = kIcpBlock / 64;
//
// LOOK (the search lists of a handle with the look-ahead on, and its first launch after a pilot
// step): the cache and D are taken around the centre c = T_c q (k_pose_set, k_pilot_map), which
// lies ahead on the query's path, so the cached ball outlives more of the coming steps.  The
// certificate of the verify pass is geometry about c alone, whatever c is.  The block scanned is
// the one around q_t = T_t q, as in the plain form: this launch's own result, the nearest scanned
// point to q_t, is certified by q_t's distance to its faces (>= 1/2 cell) exactly as there, so the
// look-ahead sends no query to the fallback that the plain form would settle; D is cut by c's
// distance to those same faces (a c outside the block gets D = 0: nothing is settled from it).
// PILOT (k_icp_pilot): the plain scan over every pilot_stride-th chunk, accumulating the octant's
// own winners within rmax; it writes no cache record and no list.
template <int G, bool LOOK, bool PILOT = false>
__device__ __forceinline__ void octant_run(const IcpArgs& a, const int32_t* list, int64_t n,
                                           double (*s_acc)[kAcc]) {
    constexpr int kW = kOctW;
    constexpr int QPC = 64 / G;  // queries per chunk
    static_assert(!PILOT || (G == 1 && !LOOK), "the pilot is the plain one-lane scan");
    const GridDesc& g = a.g;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int slot = lane / G;
    const uint32_t sub = (uint32_t)(lane % G);
    const bool lead = sub == 0;
    const int64_t gw = (int64_t)blockIdx.x * kW + wid;  // global wave id = fallback segment
    uint32_t fbn = 0;  // wave-uniform count of this wave's fallback entries
    const int64_t nwaves = (int64_t)gridDim.x * kW;
    // entry j of the work: the list's, the j-th query, or (PILOT) lane j % 64 of sampled chunk j / 64
    auto query_of = [&](int64_t j) -> int64_t {
        if constexpr (PILOT) return (j >> 6) * a.pilot_stride * 64 + (j & 63);
        return list ? (int64_t)list[j] : j;
    };
    int64_t in_ = 0;
    float4 qn = make_float4(0.f, 0.f, 0.f, 0.f);
    if (gw * QPC + slot < n) {
        in_ = query_of(gw * QPC + slot);
        if (!PILOT || in_ < a.nq) qn = ldq(a, in_);
    }
    for (int64_t c = gw; c * QPC < n; c += nwaves) {  // grid-stride (an XCD split measured slower here)
        const int64_t j = c * QPC + slot;
        const int64_t i = in_;
        const bool valid = j < n && (!PILOT || i < a.nq);  // (the last sampled chunk may be partial)
        const float4 qraw = qn;
        if (j + QPC * nwaves < n) {  // prefetch the next chunk's query
            in_ = query_of(j + QPC * nwaves);
            if (!PILOT || in_ < a.nq) qn = ldq(a, in_);
        }
        float qx = 0.f, qy = 0.f, qz = 0.f, fx = 0.f, fy = 0.f, fz = 0.f, dout = 0.f;
        float cx = 0.f, cy = 0.f, cz = 0.f, delta = 0.f;  // LOOK: the centre, |q_t - c| rounded up
        int bx = 0, by = 0, bz = 0;
        bool outside = true;
        if (valid) {
            xform(a, qraw, qx, qy, qz);
            if constexpr (LOOK) {
                xform_c(a, qraw, cx, cy, cz);
                const float ex = qx - cx, ey = qy - cy, ez = qz - cz;
                const float e2 = __fmaf_rn(ez, ez, __fmaf_rn(ey, ey, ex * ex));
                delta = e2 > 0.f ? sqrtf(e2) * 1.00001f + 1e-7f : 0.f;
            }
            // the block is placed from q_t in both forms: q_t is never off-centre in it
            fx = cell_f<float>(g, qx, 0), fy = cell_f<float>(g, qy, 1), fz = cell_f<float>(g, qz, 2);
            bx = (int)floorf(fx - a.rho), by = (int)floorf(fy - a.rho), bz = (int)floorf(fz - a.rho);
            // a query farther than rmax from the grid's box (a target-sharded rank: the queries
            // of the other shards) is settled "no correspondence" without a scan, with D = that
            // distance (every target lies inside the box)
            const float ox = fmaxf(fmaxf(-fx, fx - (float)g.n[0]), 0.f);
            const float oy = fmaxf(fmaxf(-fy, fy - (float)g.n[1]), 0.f);
            const float oz = fmaxf(fmaxf(-fz, fz - (float)g.n[2]), 0.f);
            dout = fmaxf(sqrtf(__fmaf_rn(oz, oz, __fmaf_rn(oy, oy, ox * ox))) - a.mc, 0.f) * g.hf;
            outside = dout * dout > a.r2 * 1.0001f;
        }
        const bool scanq = !outside;
        uint32_t rs[4], rn[4];
        octant_rows<G>(g, scanq, bx, by, bz, sub, rs, rn);
        const uint32_t len = rn[0] + rn[1] + rn[2] + rn[3];
        const uint32_t Lw = (uint32_t)__builtin_amdgcn_readfirstlane(wave_max_u((int)len));  // wave-uniform
        OctResult o;
        if (!(a.dbg & kDbgNoScan)) {
            if constexpr (LOOK) {
                if (Lw <= kMaxOctList)
                    o = octant_packed_la<G>(a, rs, rn, Lw, cx, cy, cz, qx, qy, qz, sub);
                else
                    o = octant_exact_la(a, rs[0], rs[1], rs[2], rs[3], rn[0], rn[1], rn[2], rn[3], cx, cy, cz, qx,
                                        qy, qz);
            } else {
                if (Lw <= kMaxOctList)
                    o = octant_packed<G>(a, rs, rn, Lw, qx, qy, qz, sub);
                else
                    o = octant_exact(a, rs[0], rs[1], rs[2], rs[3], rn[0], rn[1], rn[2], rn[3], qx, qy, qz);
            }
        }
        bool settled = false, found = false;
        if (valid) {
            // this query's certified radius (cells): its distance to the nearest face of the
            // 2x2x2 block (>= 0.5 cell), less the margin
            const float m = fminf(fminf(fminf(fx - (float)bx, (float)(bx + 2) - fx),
                                        fminf(fy - (float)by, (float)(by + 2) - fy)),
                                  fminf(fz - (float)bz, (float)(bz + 2) - fz)) - a.mc;
            const float rr = m * g.hf;
            const float cert2 = fmaxf(a.cert2, rr * rr * (1.f - 2e-5f));
            float mD = m;  // the cache's radius: the centre's distance to the same faces
            if constexpr (LOOK) {
                // c's own distance to the faces of the block scanned (around q_t): every target
                // nearer to c than that was scanned.  Not positive: c is outside the block, D = 0
                // and the record never settles anything.
                const float ux = cell_f<float>(g, cx, 0), uy = cell_f<float>(g, cy, 1), uz = cell_f<float>(g, cz, 2);
                mD = fminf(fminf(fminf(ux - (float)bx, (float)(bx + 2) - ux),
                                 fminf(uy - (float)by, (float)(by + 2) - uy)),
                           fminf(uz - (float)bz, (float)(bz + 2) - uz)) - a.mc;
                // o.d0 is exact with o.uniq, else a lower bound on every scanned point's d2
                found = o.uniq && o.d0 <= a.r2;
                settled = (found ? o.d0 <= cert2 : (o.d0 > a.r2 && a.r2 <= cert2)) || outside ||
                          (a.dbg & kDbgNoFallback);
            } else {
                found = o.d0 <= a.r2;
                settled = (found ? (o.d0 < o.dnext && o.d0 <= cert2) : a.r2 <= cert2) || outside ||
                          (a.dbg & kDbgNoFallback);
            }
            if constexpr (PILOT) {
                // the octant's nearest within rmax, certified or not: a prediction needs no exactness,
                // and leaving out the far pairs (the ones that move the pose most) measured a first
                // step 20 % short on the C4 registration
                settled = found;
            } else {
                // the cache: the 3 nearest; settled: D bounds every uncached point for the verify
                // pass.  Unsettled: the fallback pass (which overwrites the cache) gets the
                // octant's first uncached d2 instead.
                // (unsettled: the message is the octant's first uncached distance, rounded down)
                // (LOOK: dout and dnext's fallback message are bounds at q_t, D is one at c)
                const float D = outside ? fmaxf(dout - delta, 0.f) * 0.9999f
                                        : (settled ? fminf(sqrtf(o.dnext), (mD > 0.f ? mD : 0.f) * g.hf) * 0.9999f
                                                   // (LOOK: dnext is measured from c and the fallback's skip
                                                   // proof needs the bound at q_t: dnext less |q_t - c|, or
                                                   // the second smallest d2 at q_t -- the winner is cached,
                                                   // so every uncached point is at least that far)
                                                   : fmaxf(sqrtf(o.dnext) - delta, LOOK ? sqrtf(o.d1t) : 0.f) *
                                                         0.99999f);
                if (lead) cache_store(a, i, o.c0, o.c1, o.c2, D, a.launch);
            }
        }
        if constexpr (!PILOT) {
            // ---- fallback list (ballot + mbcnt, no atomics) and accumulators
            const bool fb = valid && lead && !settled;
            const uint64_t fbm = __ballot(fb);
            if (fb) {
                const uint32_t pos = fbn + __builtin_amdgcn_mbcnt_hi((uint32_t)(fbm >> 32),
                                                                   __builtin_amdgcn_mbcnt_lo((uint32_t)fbm, 0u));
                a.fb[gw * a.fb_seg + pos] = (int32_t)i;
            }
            fbn += (uint32_t)__popcll(fbm);
        }
        const bool acc_ok = valid && lead && settled && found && !(a.dbg & kDbgNoAccum);
        const Best w{o.d0, 0, o.win, o.wx, o.wy, o.wz};
        chunk_accumulate(acc_ok, qx, qy, qz, w, s_acc[wid], lane);
    }
    if constexpr (!PILOT) {
        if (lane == 0) {  // every wave of the grid writes its count: no zeroing pass needed
            a.fb_count[gw] = fbn;
        }
    }
}

// Lanes per query by the list's density (measured per launch on the C4 bench registration,
// tools/gpu_octg_ab.sh): dense lists share candidate lines between neighbouring queries and
// want one lane each; sparse ones want the group form.
__device__ __forceinline__ int octant_lanes(int64_t n, int64_t nq) {
    if (n * 100 > nq * 36) return 1;
    if (n * 100 > nq * 8) return 2;
    return 4;
}

// MINW: the first (dense) launch runs at PCP_OCT_WAVES waves/SIMD; the search lists of later
// launches at PCP_OCT_WAVES_LIST, whose larger register budget measured faster on them.  A grid
// smaller than the partial rows / list segments sized for the first launch zeroes the rest.
// LOOK: the look-ahead form (octant_run), for the search lists unless PCP_ICP_OPT_NO_LOOKAHEAD.
template <int MINW, bool LOOK>
__global__ void __launch_bounds__(kIcpBlock, MINW) k_icp_octant(IcpArgs a, const int32_t* list,
                                                                 const uint32_t* list_n) {
    // the first launch after a pilot step: the form that beta_0 (k_pilot_map) did not choose exits
    if (a.when_beta && (a.pose->beta > 0.f) != (a.when_beta == 1)) return;
    load_pose(a);
    if constexpr (LOOK) load_pose_c(a);
    __shared__ double s_acc[kOctW][kAcc];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t n = list ? (int64_t)*list_n : a.nq;
    if (lane < kAcc) s_acc[wid][lane] = 0.0;
    const int G = a.oct_g ? a.oct_g : octant_lanes(n, a.nq);  // uniform over the grid
    if (G == 1)
        octant_run<1, LOOK>(a, list, n, s_acc);
    else if (G == 2)
        octant_run<2, LOOK>(a, list, n, s_acc);
    else if (G == 4)
        octant_run<4, LOOK>(a, list, n, s_acc);
    else
        octant_run<8, LOOK>(a, list, n, s_acc);
    write_wave_partials(s_acc, a.partials + (int64_t)blockIdx.x * kAcc);
    for (int64_t r = gridDim.x + blockIdx.x; r < a.nb_fast; r += gridDim.x)
        if (threadIdx.x < kAcc) a.partials[r * kAcc + threadIdx.x] = 0.0;
    if (lane == 0) {
        const int64_t nw = (int64_t)gridDim.x * kOctW;
        for (int64_t sg = nw + (int64_t)blockIdx.x * kOctW + wid; sg < a.nseg; sg += nw) {
            a.fb_count[sg] = 0u;
        }
    }
}

// Pilot step (before a handle's first launch, dense grid): the plain octant scan under the first
// launch's pose over every a.pilot_stride-th 64-query chunk of the sorted queries -- a spatially
// uniform sample, since the queries are sorted by cell -- accumulating the nearest scanned target of
// every query that has one within rmax (the exact winner for most).  One Kabsch step over these sums (k_pilot_map) predicts the second pose.  `nsamp`
// sampled chunks, one per wave, grid-stride; workgroup b writes partial row b.
__global__ void __launch_bounds__(kIcpBlock, PCP_OCT_WAVES) k_icp_pilot(IcpArgs a, int64_t nsamp) {
    load_pose(a);
    __shared__ double s_acc[kOctW][kAcc];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane < kAcc) s_acc[wid][lane] = 0.0;
    octant_run<1, false, true>(a, nullptr, nsamp * 64, s_acc);
    write_wave_partials(s_acc, a.partials + (int64_t)blockIdx.x * kAcc);
}

// Fallback / general pass: exact box search (dense or sparse grid), starting from the
// octant pass's provisional winner when it has one.  Queries come from the compacted
// fallback list (or are all queries when ring_all is set, i.e. on a sparse grid); waves
// take 64-entry chunks grid-stride and accumulate like the octant pass.
// G lanes per query: the lanes of a query split its rows (Best::scan_rows_g / scan_g) and
// merge after each plane; the group's first lane writes and accumulates.  Measured per launch
// (profiles/r02_ring): the short fallback lists of later launches are latency-bound and run
// ~35 % faster with G = 4, while the long early lists (wide "nothing within rmax" boxes of
// short rows, whose per-row bookkeeping G lanes would repeat) want one lane per query.
// G is picked on the device from the list's length (ring_lanes) unless IcpArgs::ring_g fixes it.
__device__ __forceinline__ int ring_lanes(int64_t n, int64_t nq) {
    if (n * 1000 > nq) return 1;
    if (n * 8000 > nq) return 2;
    return 4;
}
template <int G>
__device__ __forceinline__ void ring_run(IcpArgs& a, double (*s_acc)[kAcc], const int32_t* list, const uint32_t* list_n) {
    constexpr int kW = kIcpBlock / 64;
    constexpr int QPC = 64 / G;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint32_t sub = (uint32_t)(lane % G);
    const bool lead = sub == 0;
    const int64_t n = a.ring_all ? a.nq : (int64_t)*list_n;
    const XcdSplit xs = xcd_split((n + QPC - 1) / QPC, kW);
    for (int64_t c = xs.c0 + xs.w; c < xs.c1; c += xs.nw) {
        const int64_t j = c * QPC + lane / G;
        const bool valid = j < n;
        Best b{a.r2, 0x7fffffff, 0u, 0.f, 0.f, 0.f};
        float qx = 0.f, qy = 0.f, qz = 0.f;
        int64_t i = 0;
        if (valid) {
            i = a.ring_all ? j : list[j];
            const float4 qraw = ldq(a, i);
            xform(a, qraw, qx, qy, qz);
            // provisional: the cache's best (refreshed by the search pass), an upper bound
            const CacheRec cd = cache_load(a, i);
            const CacheBest cbst = cache_best(a.tp, cd, qx, qy, qz);
            if (cbst.bd <= b.bd) {
                b.bd = cbst.bd;
                b.bj = cbst.bj;
                b.bk = cbst.bk;
            }
            // the search pass left this launch's octant message: the 4th smallest distance of
            // its octant (rounded down).  Above the cached best, every octant point tied with
            // that best is cached, so the cached best IS the octant's (d2, index) winner and its
            // cells need no rescan.  (A look-ahead search ranked what it cached around its centre
            // c = T_c q, and its message is already weakened by |q_t - c| to a bound at q_t.)
            const bool skip_oct = !a.ring_all && cd.slot == (a.launch & a.hist_mask) && cd.D * cd.D > cbst.bd;
            bool done = false;
            if (!a.ring_all) {
                // stage 2: the 3x3x3 cells around the query (less the octant's when it was
                // searched completely), rows and end cells pruned by the bound, as 3 planes of 3
                // x-rows scanned like the octant pass; certifies any winner within the distance
                // to the block's faces (>= 1 cell).  Only what is left goes to the general search.
                const GridDesc& g = a.g;
                const float fx = cell_f<float>(g, qx, 0), fy = cell_f<float>(g, qy, 1), fz = cell_f<float>(g, qz, 2);
                const int cx = (int)floorf(fx), cy = (int)floorf(fy), cz = (int)floorf(fz);
                const float lx = fx - (float)cx, ly = fy - (float)cy, lz = fz - (float)cz;
                // the block the octant pass scanned: placed from q_t in every form (octant_run),
                // by the same expression
                const int bxo = (int)floorf(fx - a.rho), byo = (int)floorf(fy - a.rho),
                          bzo = (int)floorf(fz - a.rho);
                const float inv_h2 = g.inv_hf * g.inv_hf;
                const float gxl = sq_gap(lx, a.mc), gxr = sq_gap(1.f - lx, a.mc);
                for (int dz = -1; dz <= 1; dz++) {
                    const int z = cz + dz;
                    const float lim = b.bd * 1.00002f * inv_h2;  // the bound in cells^2 (shrinks)
                    const float gz2 = sq_gap(axis_gap<float>(z, cz, lz), a.mc);
                    uint32_t rs[3], rn[3];
#pragma unroll
                    for (int r = 0; r < 3; r++) {
                        const int y = cy - 1 + r;
                        const float gyz = gz2 + sq_gap(axis_gap<float>(y, cy, ly), a.mc);
                        int xlo = max(cx - 1, 0), xhi = min(cx + 1, g.n[0] - 1);
                        if (skip_oct && y >= byo && y <= byo + 1 && z >= bzo && z <= bzo + 1) {
                            // cells [bxo, bxo + 1] were scanned: cut them off the end they cover
                            if (bxo <= xlo) xlo = max(xlo, bxo + 2);
                            else if (bxo + 1 >= xhi) xhi = min(xhi, bxo - 1);
                        }
                        if (xlo == cx - 1 && gyz + gxl > lim) xlo = cx;
                        if (xhi == cx + 1 && gyz + gxr > lim) xhi = cx;
                        const bool in = y >= 0 && y < g.n[1] && z >= 0 && z < g.n[2] && gyz <= lim && xlo <= xhi;
                        const int64_t cc = in ? dense_id(g, xlo, y, z) : 0;
                        rs[r] = in ? g.cstart[cc] : 0u;
                        rn[r] = in ? g.cstart[cc + (xhi - xlo + 1)] - rs[r] : 0u;
                    }
                    b.scan_rows_g<G>(a.tp, rs, rn, qx, qy, qz, sub);
                    b.merge_group<G>();
                }
                const float m = fminf(fminf(fminf(fx - (float)(cx - 1), (float)(cx + 2) - fx),
                                            fminf(fy - (float)(cy - 1), (float)(cy + 2) - fy)),
                                      fminf(fz - (float)(cz - 1), (float)(cz + 2) - fz)) - a.mc;
                const float rr = m * g.hf;
                const float c2 = rr * rr * (1.f - 2e-5f);
                const bool found = b.bj != 0x7fffffff;
                done = (found && b.bd <= c2) || (!found && a.r2 <= c2);
            }
            if (!done) box_search<G>(a.g, a.tp, qx, qy, qz, a.mc, b, sub);
            const bool ok = b.bj != 0x7fffffff;
            // no bound kept: the next launch searches it again
            if (lead) {
                cache_store(a, i, ok ? b.bk : ~0u, ~0u, ~0u, 0.f, a.launch);
            }
        }
        const bool acc_ok = valid && lead && b.bj != 0x7fffffff && !(a.dbg & kDbgNoAccum);
        if (acc_ok) b.fetch(a.tp);
        chunk_accumulate(acc_ok, qx, qy, qz, b, s_acc[wid], lane);
    }
}

__global__ void __launch_bounds__(kIcpBlock, PCP_RING_WAVES) k_icp_ring(IcpArgs a, double* partials,
                                                                        const int32_t* list, const uint32_t* list_n) {
    load_pose(a);
    constexpr int kW = kIcpBlock / 64;
    __shared__ double s_acc[kW][kAcc];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane < kAcc) s_acc[wid][lane] = 0.0;
    const int64_t n = a.ring_all ? a.nq : (int64_t)*list_n;
    const int G = a.ring_g ? a.ring_g : (a.ring_all ? 1 : ring_lanes(n, a.nq));  // uniform
    if (G == 1)
        ring_run<1>(a, s_acc, list, list_n);
    else if (G == 2)
        ring_run<2>(a, s_acc, list, list_n);
    else if (G == 4)
        ring_run<4>(a, s_acc, list, list_n);
    else
        ring_run<8>(a, s_acc, list, list_n);
    write_wave_partials(s_acc, partials + (int64_t)blockIdx.x * kAcc);
}

// Concatenate per-wave list segments (segment s holds cnt[s] entries at s * seg_cap) into one
// list, in one launch with no separate scan: block b (4 waves: segments 4b .. 4b + 3) finds the
// exclusive prefix of the counts before its first segment by summing them itself (at most nseg
// counts, L2-resident), and the block holding the last segment writes the total to *total (where
// the consumers read the list length).  The list keeps segment order, entry for entry.
__global__ void __launch_bounds__(256) k_list_compact(const int32_t* __restrict__ seg, const uint32_t* __restrict__ cnt,
                                                      int64_t nseg, int64_t seg_cap, int32_t* __restrict__ out,
                                                      uint32_t* __restrict__ total) {
    __shared__ uint32_t s_part[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t s0 = (int64_t)blockIdx.x * 4;
    uint32_t acc = 0;
    for (int64_t i = threadIdx.x; i < s0; i += 256) acc += cnt[i];
    for (int o = 32; o > 0; o >>= 1) acc += (uint32_t)__shfl_xor((int)acc, o, 64);
    if (lane == 0) s_part[w] = acc;
    __syncthreads();
    const uint32_t base = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    uint32_t c[4];
#pragma unroll
    for (int k = 0; k < 4; k++) c[k] = s0 + k < nseg ? cnt[s0 + k] : 0u;
    uint32_t off = base;
#pragma unroll
    for (int k = 0; k < 3; k++) off += k < w ? c[k] : 0u;
    const int64_t sg = s0 + w;
    if (sg < nseg)
        for (uint32_t k = (uint32_t)lane; k < c[w]; k += 64) out[off + k] = seg[sg * seg_cap + k];
    if (s0 + 4 >= nseg && threadIdx.x == 0) *total = base + c[0] + c[1] + c[2] + c[3];
}

// fixed-order reduction of nb partial rows of 24 doubles -> out[24]: thread t sums column
// t % 24 over the rows b = t / 24 (mod 32) -- coalesced row reads, no barrier per column --
// then 24 threads add the 32 group sums in order.  Slot 23 (unused by the solve) carries the
// number of fallback queries of the iteration (*fb_total, or 0 without a fallback list).
constexpr int kRedGroups = 32;
__global__ void __launch_bounds__(kAcc * kRedGroups) k_reduce_partials(const double* __restrict__ part, int nb,
                                                                       double* out, const uint32_t* fb_total) {
    __shared__ double s[kRedGroups][kAcc];
    const int k = threadIdx.x % kAcc, grp = threadIdx.x / kAcc;
    double v = 0.0;
    int b = grp;
    for (; b + 7 * kRedGroups < nb; b += 8 * kRedGroups) {  // 8 loads in flight, summed in order
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; u++) x[u] = part[(int64_t)(b + u * kRedGroups) * kAcc + k];
#pragma unroll
        for (int u = 0; u < 8; u++) v += x[u];
    }
    for (; b < nb; b += kRedGroups) v += part[(int64_t)b * kAcc + k];
    s[grp][k] = v;
    __syncthreads();
    if (threadIdx.x < kAcc) {
        double t = 0.0;
        for (int j = 0; j < kRedGroups; j++) t += s[j][threadIdx.x];
        out[threadIdx.x] = threadIdx.x == kAcc - 1 ? (fb_total ? (double)*fb_total : 0.0) : t;
    }
}

// sorted-order winners -> caller (original query) order; d2 recomputed from the winner's
// position under the same pose (the same fp32 expression, so bit-identical)
__global__ void k_scatter_corr(IcpArgs a, int32_t* idx, float* d2) {
    load_pose(a);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.nq;
         i += (int64_t)gridDim.x * blockDim.x) {
        const float4 qq = ldq(a, i);
        const int oq = a.qidx[i];
        float x, y, z;
        xform(a, qq, x, y, z);
        const CacheBest w = cache_best(a.tp, cache_load(a, i), x, y, z);  // the settled winner is cached
        const bool ok = w.bd <= a.r2;
        idx[oq] = ok ? w.bj : -1;
        d2[oq] = ok ? w.bd : INFINITY;
    }
}

__global__ void k_fill_corr(int32_t* idx, float* d2, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        idx[i] = -1;
        d2[i] = INFINITY;
    }
}

// ---- target-sharded mode: per-query u64 key = (fp32 bits of d2) << 32 |
// global target index, so a MIN over ranks is the lexicographic (d2, index) winner (non-
// negative fp32 bit patterns order like the values).  No correspondence = INT64_MAX.  The layout
// and what is done with a pair are icp_pair.hpp's.
__global__ void k_fill_keys(uint64_t* keys, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        keys[i] = kNoKey;
}

__global__ void k_make_keys(IcpArgs a, uint32_t offset, uint64_t* keys) {
    load_pose(a);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.nq; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 qq = ldq(a, i);
        const int oq = a.qidx[i];
        float x, y, z;
        xform(a, qq, x, y, z);
        const CacheBest w = cache_best(a.tp, cache_load(a, i), x, y, z);
        keys[oq] = w.bd <= a.r2 ? key_make(w.bd, (uint32_t)w.bj + offset) : kNoKey;
    }
}

}  // namespace

// What the kernels read that is the same at every launch of the handle with this rmax: the target,
// the queries, the caches, the lists and the search constants.  A launch adds dbg, oct_g, its
// partials, when_beta and pilot_stride; R, t and launch are the kernels' own (load_pose).
IcpArgs icp_args(const pcp_icp* icp, float rmax) {
    const pcp_index* tg = icp->target;
    IcpArgs a{};
    a.g = tg->g;
    a.tp = (const float4*)tg->pts;
    a.q = icp->q;
    a.qidx = icp->qidx;
    a.nq = icp->nq;
    a.pose = icp->pose_dev;  // every kernel reads the pose and the launch index from HBM
    a.r2 = rmax * rmax;
    a.mc = search_margin(a.g);  // >> fp32 rounding of the cell coordinates
    a.rho = 0.5f;
    // exact radius of the octant block: (0.5 - mc) cells, shrunk for fp32 d2 rounding
    const double rr = (0.5 - (double)a.mc) * a.g.h;
    a.cert2 = (float)(rr * rr * (1.0 - 1e-5));
    a.cand = icp->cand;
    a.narrow = icp->narrow ? 1 : 0;
    a.hist_mask = icp->narrow ? 63u : (uint32_t)(kHist - 1);
    a.max_age = icp->narrow ? 32u : 128u;
    a.dunit = (float)(a.g.h / 1024.0);
    a.inv_dunit = (float)(1024.0 / a.g.h);
    a.pose_hist = icp->pose_hist;
    a.ntp = (uint32_t)tg->n;
    a.sv = icp->sv;
    a.sv_count = icp->sv_count;
    a.sv_off = icp->sv_off;
    a.sv_seg = icp->sv_seg;
    a.nseg_v = icp->nseg_v;
    a.fb = icp->fb;
    a.fb_count = icp->fb_count;
    a.fb_off = icp->fb_off;
    a.fb_seg = icp->fb_seg;
    a.nb_fast = icp->nb_fast;
    a.nseg = (int64_t)icp->nb_fast * (kIcpBlock / 64);
    a.ring_all = a.g.dense ? 0 : 1;
    a.ring_g = icp->ring_g;
    return a;
}

// One correspondence launch under the pose T (a host 4x4) or T_dev (a device one): exactly one is
// non-null.
struct LaunchReq {
    const double* T = nullptr;
    const double* T_dev = nullptr;
    float rmax = 0.f;
    double* acc_dev = nullptr;     // the launch's 24 sums
    int32_t* corr_idx = nullptr;   // optional: the correspondences in caller order ...
    float* corr_d2 = nullptr;      // ... and their d2
    IcpArgs* keys_args = nullptr;  // the keys path: correspondences only -- nothing is accumulated, no pilot
                                   // step (what is built on the keys minimises something else), no graph;
                                   // receives the launch's arguments for k_make_keys
    static LaunchReq host(const double* T, float rmax, double* acc) { return {T, nullptr, rmax, acc}; }
    static LaunchReq dev(const double* T_dev, float rmax, double* acc) { return {nullptr, T_dev, rmax, acc}; }
};

using OctKernel = void (*)(IcpArgs, const int32_t*, const uint32_t*);
// the dense first launch in its look-ahead form (after a pilot step): waves per SIMD and its grid
// (6 waves/SIMD: 80 VGPRs and 144 B of scratch against 128 VGPRs and none at 4, but measured 0.11 ms
// faster on the 50M first launch; the list launches of the same form stay at 4)
#ifndef PCP_OCT_WAVES_LOOK0
#define PCP_OCT_WAVES_LOOK0 6
#endif
int nb_look0(const pcp_icp* icp) { return PCP_OCT_WAVES_LOOK0 < PCP_OCT_WAVES ? icp->nb_fast_l : icp->nb_fast; }

// The tail of every launch, on `st`: concatenate the octant pass's per-wave fallback segments into
// one list, then the exact fallback pass over it (a sparse grid has no octant pass and no list: the
// fallback pass takes every query).  Its partials are the last of the launch.
void icp_fallback(pcp_icp* icp, hipStream_t st, IcpArgs& a) {
    uint32_t* const fbc_n = icp->fb_off + a.nseg;  // the list's length follows its segments' offsets
    if (a.g.dense)
        hipLaunchKernelGGL(k_list_compact, dim3((unsigned)((a.nseg + 3) / 4)), dim3(256), 0, st,
                           (const int32_t*)icp->fb, (const uint32_t*)icp->fb_count, a.nseg, a.fb_seg, icp->fbc, fbc_n);
    a.partials = icp->partials + (int64_t)(icp->nb_ver + icp->nb_fast) * kAcc;
    hipLaunchKernelGGL(k_icp_ring, dim3(icp->nb_ring), dim3(kIcpBlock), 0, st, a, a.partials,
                       (const int32_t*)icp->fbc, (const uint32_t*)fbc_n);
}

// The five kernels of a dense-grid launch after the first, on `st` (the context's stream, or a
// stream under graph capture): verify what the candidate caches can settle, concatenate the
// per-wave search segments, octant search of that list (`oct`), then icp_fallback.  `a` carries
// oct_g.
int icp_chain(pcp_icp* icp, hipStream_t st, IcpArgs& a, OctKernel oct) {
    pcp_ctx* ctx = icp->ctx;
    uint32_t* const svc_n = icp->sv_off + a.nseg_v;  // the search list's length, as the fallback list's
    a.partials = icp->partials;
    hipLaunchKernelGGL(k_icp_verify, dim3(icp->nb_ver), dim3(kIcpBlock), 0, st, a);
    hipLaunchKernelGGL(k_list_compact, dim3((unsigned)((a.nseg_v + 3) / 4)), dim3(256), 0, st,
                       (const int32_t*)icp->sv, (const uint32_t*)icp->sv_count, a.nseg_v, a.sv_seg, icp->svc, svc_n);
    if (icp->dbg) PCP_HIP(ctx, hipEventRecord(icp->ev_ver, st));
    a.partials += (int64_t)icp->nb_ver * kAcc;
    hipLaunchKernelGGL(oct, dim3(icp->nb_fast_l), dim3(kIcpBlock), 0, st, a, (const int32_t*)icp->svc,
                       (const uint32_t*)svc_n);
    if (icp->dbg) PCP_HIP(ctx, hipEventRecord(icp->ev_mid, st));
    icp_fallback(icp, st, a);
    return PCP_OK;
}

int icp_launch(pcp_icp* icp, const LaunchReq& rq) {
    pcp_ctx* ctx = icp->ctx;
    const bool keys = rq.keys_args != nullptr;
    IcpArgs a = icp_args(icp, rq.rmax);
    a.dbg = icp->dbg | (keys ? kDbgNoAccum : 0);
    LookAhead la{};
    for (int k = 0; k < 3; k++) {
        la.lo[k] = (float)(a.g.o[k] - rq.rmax);
        la.hi[k] = (float)(a.g.o[k] + a.g.n[k] * a.g.h + rq.rmax);
    }
    la.alpha = kLookAlpha;
    la.cap = kLookCap;
    la.off = icp->no_look ? 1 : 0;
    hipLaunchKernelGGL(k_pose_set, dim3(1), dim3(1), 0, ctx->stream, rq.T_dev, rq.T_dev ? Pose32{} : pose32(rq.T), la,
                       icp->pose_dev, icp->pose_hist + (icp->launches & (icp->narrow ? 63 : kHist - 1)) * 12,
                       (uint32_t)icp->launches);
    hipEvent_t e0 = icp->ev0, e1 = icp->ev1;
    if (rq.T_dev) {  // device-resident loop: one event pair per launch, read by pcp_icp_kernel_ms
        if (icp->ntev == icp->tev.size()) {
            std::pair<hipEvent_t, hipEvent_t> pr{nullptr, nullptr};
            PCP_HIP(ctx, icp->mem.event(&pr.first));
            PCP_HIP(ctx, icp->mem.event(&pr.second));
            icp->tev.push_back(pr);
        }
        e0 = icp->tev[icp->ntev].first;
        e1 = icp->tev[icp->ntev].second;
        icp->ntev++;
    }
    PCP_HIP(ctx, hipEventRecord(e0, ctx->stream));
    const bool verify = a.g.dense && icp->launches > 0;  // the first launch has nothing cached
    icp->has_pred = icp->has_pred && icp->launches == 0;  // (a prediction serves the first launch only)
    icp->last_verified = verify;
    // the search lists: the look-ahead form unless it is switched off (beta = 0: T_c = T_t).  Launch
    // 1 has no step ratio yet, so beta = 0 there too, and the plain form is the faster one on its
    // long list (measured 1.57 against 1.88 ms on the C4 registration).  A captured graph is
    // replayed at every later launch, so it holds the look-ahead form and starts at launch 2:
    // replayed and plain launches then run the same kernels at every launch.
    const OctKernel oct_graph =
        icp->no_look ? k_icp_octant<PCP_OCT_WAVES_LIST, false> : k_icp_octant<PCP_OCT_WAVES_LIST, true>;
    const OctKernel oct_list = icp->launches <= 1 ? k_icp_octant<PCP_OCT_WAVES_LIST, false> : oct_graph;
    if (verify) {
        a.oct_g = icp->oct_g_list;
        // A device-pose launch after the first is the same five kernels every time with the same
        // arguments: the launch index is read from the device (k_pose_set) and the pose was already.
        // With PCP_ICP_OPT_GRAPH the chain is captured once per handle into a HIP graph and replayed --
        // one launch instead of five (measured: host enqueue is not what the loop waits for, and the
        // replayed chain ran 0.5 % slower, so it is off by default).
        const bool graph = icp->graph && rq.T_dev && !icp->dbg && !rq.corr_idx && !keys && !icp->graph_off &&
                           oct_list == oct_graph;
        if (graph && icp->gexec && icp->graph_r2 != a.r2) {  // captured for another rmax
            icp_graph_drop(icp);                              // (it selects the owner's device)
            PCP_HIP(ctx, hipSetDevice(ctx->device));
        }
        if (graph && !icp->gexec) {  // captured on the context's side stream (capture enqueues nothing)
            hipStream_t cap = nullptr;
            hipError_t e = side_stream(ctx, &cap) == PCP_OK ? hipSuccess : hipErrorInvalidValue;
            hipGraph_t gr = nullptr;
            if (e == hipSuccess) e = hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal);
            if (e == hipSuccess) {
                (void)icp_chain(icp, cap, a, oct_graph);
                e = hipStreamEndCapture(cap, &gr);
            }
            if (e == hipSuccess) e = hipGraphInstantiate(&icp->gexec, gr, nullptr, nullptr, 0);
            if (gr) (void)hipGraphDestroy(gr);
            if (e != hipSuccess) {  // launch the kernels one by one from now on
                icp->gexec = nullptr;
                icp->graph_off = true;
                (void)hipGetLastError();
            }
            icp->graph_r2 = a.r2;
        }
        if (graph && icp->gexec) PCP_HIP(ctx, hipGraphLaunch(icp->gexec, ctx->stream));
        else PCP_TRY(icp_chain(icp, ctx->stream, a, oct_list));
    } else {
        // the first launch (nothing cached: the octant search takes every query) or a sparse grid
        // (the fallback pass takes every query)
        double* const part_o = icp->partials + (int64_t)icp->nb_ver * kAcc;
        const int nb_idle = a.g.dense ? icp->nb_ver : icp->nb_ver + icp->nb_fast;
        PCP_HIP(ctx, hipMemsetAsync(icp->partials, 0, (size_t)nb_idle * kAcc * sizeof(double), ctx->stream));
        if (a.g.dense) {
            if (icp->dbg) PCP_HIP(ctx, hipEventRecord(icp->ev_ver, ctx->stream));
            a.partials = part_o;
            a.oct_g = icp->oct_g_first;
            // The handle's first launch can look ahead too: a predicted second pose -- the caller's
            // (pcp_icp_predict_first), or by default on a large handle one Kabsch step over a sample
            // of the queries (the pilot) -- gives beta_0 and T_c (k_pilot_map).  beta_0 is known on
            // the device only, so both forms of the search are enqueued and the one it did not
            // choose exits at once: beta_0 = 0 runs exactly the plain first launch.
            const bool pilot = !keys && !icp->has_pred && !icp->no_pilot && !icp->dbg && icp->nq > 0 &&
                               (icp->pilot_always || icp->nq >= kPilotMinQueries);
            const bool look0 = icp->launches == 0 && !icp->no_look && (icp->has_pred || pilot);
            if (look0) {
                PilotPred pred{};
                if (icp->has_pred) {
                    pred.on = 1;
                    for (int k = 0; k < 16; k++) pred.T1[k] = icp->pred[k];
                } else {
                    const int64_t nch = (icp->nq + 63) / 64;
                    a.pilot_stride = std::max<int64_t>(1, nch / kPilotChunks);
                    const int64_t nsamp = (nch + a.pilot_stride - 1) / a.pilot_stride;
                    const int nbp = (int)std::min<int64_t>((nsamp + kOctW - 1) / kOctW, icp->nb_fast);
                    hipLaunchKernelGGL(k_icp_pilot, dim3(nbp), dim3(kIcpBlock), 0, ctx->stream, a, nsamp);
                    hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(kAcc * kRedGroups), 0, ctx->stream,
                                       (const double*)part_o, nbp, icp->pilot_acc, (const uint32_t*)nullptr);
                }
                hipLaunchKernelGGL(k_pilot_map, dim3(1), dim3(1), 0, ctx->stream, (const double*)icp->pilot_acc, pred,
                                   la, icp->pose_dev, icp->pose_hist);
                a.when_beta = 1;
                hipLaunchKernelGGL((k_icp_octant<PCP_OCT_WAVES_LOOK0, true>), dim3(nb_look0(icp)), dim3(kIcpBlock), 0,
                                   ctx->stream, a, (const int32_t*)nullptr, (const uint32_t*)nullptr);
                a.when_beta = 2;
            }
            hipLaunchKernelGGL((k_icp_octant<PCP_OCT_WAVES, false>), dim3(icp->nb_fast), dim3(kIcpBlock), 0,
                               ctx->stream, a, (const int32_t*)nullptr, (const uint32_t*)nullptr);
            a.when_beta = 0;
        }
        if (icp->dbg) PCP_HIP(ctx, hipEventRecord(icp->ev_mid, ctx->stream));
        icp_fallback(icp, ctx->stream, a);
    }
    PCP_HIP(ctx, hipEventRecord(e1, ctx->stream));
    hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(kAcc * kRedGroups), 0, ctx->stream, icp->partials,
                       icp->nb_ver + icp->nb_fast + icp->nb_ring, rq.acc_dev,
                       a.g.dense ? (const uint32_t*)(icp->fb_off + a.nseg) : nullptr);
    if (rq.corr_idx) {
        if (icp->nq_in > icp->nq)  // non-finite queries were dropped at create time
            hipLaunchKernelGGL(k_fill_corr, dim3(grid_for(icp->nq_in, 256)), dim3(256), 0, ctx->stream, rq.corr_idx,
                               rq.corr_d2, icp->nq_in);
        if (icp->nq > 0)
            hipLaunchKernelGGL(k_scatter_corr, dim3(grid_for(icp->nq, 256)), dim3(256), 0, ctx->stream, a,
                               rq.corr_idx, rq.corr_d2);
    }
    if (keys) *rq.keys_args = a;
    icp->launches++;
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

}  // namespace pcp

extern "C" {

int pcp_icp_step(pcp_ctx* ctx, pcp_icp* icp, const double T[16], float rmax, double* acc_dev,
                 int32_t* corr_idx, float* corr_d2) {
    if (!ctx || !icp || !T || !acc_dev || (corr_idx && !corr_d2) || !(rmax >= 0.f)) return PCP_ERR_ARG;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    icp->ctx = ctx;
    pcp::LaunchReq rq = pcp::LaunchReq::host(T, rmax, acc_dev);
    rq.corr_idx = corr_idx;
    rq.corr_d2 = corr_d2;
    PCP_TRY(pcp::icp_launch(icp, rq));
    double fbn = 0.0;
    PCP_HIP(ctx, hipMemcpyAsync(&fbn, acc_dev + 23, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    uint32_t nsv = (uint32_t)icp->nq;  // sparse grid / first launch: every query is searched
    if (icp->last_verified)
        PCP_HIP(ctx, hipMemcpyAsync(&nsv, icp->sv_off + icp->nseg_v, sizeof(nsv),
                                    hipMemcpyDeviceToHost, ctx->stream));
    PCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    icp->last_fallback = (uint32_t)fbn;
    icp->last_searched = nsv;
    float ms = 0.f;
    PCP_HIP(ctx, hipEventElapsedTime(&ms, icp->ev0, icp->ev1));
    icp->last_ms = ms;
    icp->last_launches = 1;
    if (icp->dbg) {
        float m1 = 0.f, mv = 0.f;
        (void)hipEventElapsedTime(&m1, icp->ev0, icp->ev_mid);
        (void)hipEventElapsedTime(&mv, icp->ev0, icp->ev_ver);
        std::fprintf(stderr, "[pcp icp dbg=%d] verify %.4f ms  octant %.4f ms  fallback %.4f ms  searched %u  "
                     "n_fallback %u\n", icp->dbg, mv, m1 - mv, ms - m1, nsv, icp->last_fallback);
    }
    return PCP_OK;
}

// pcp_icp_keys / pcp_icp_keys_dev: one launch for the correspondences only, then their keys.
// T (host) or T_dev (device pose) -- exactly one is non-null
static int icp_keys(pcp_ctx* ctx, pcp_icp* icp, const double* T, const double* T_dev, float rmax,
                    int64_t target_offset, uint64_t* keys_dev) {
    if (!ctx || !icp || (!T && !T_dev) || !keys_dev || !(rmax >= 0.f) || target_offset < 0 ||
        target_offset + pcp_index_size(icp->target) > ((int64_t)1 << 32))
        return PCP_ERR_ARG;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    icp->ctx = ctx;
    pcp::IcpArgs a{};
    pcp::LaunchReq rq = T_dev ? pcp::LaunchReq::dev(T_dev, rmax, icp->acc) : pcp::LaunchReq::host(T, rmax, icp->acc);
    rq.keys_args = &a;  // correspondences only
    PCP_TRY(pcp::icp_launch(icp, rq));
    if (icp->nq_in > icp->nq)
        hipLaunchKernelGGL(pcp::k_fill_keys, dim3(pcp::grid_for(icp->nq_in, 256)), dim3(256), 0, ctx->stream, keys_dev,
                           icp->nq_in);
    if (icp->nq > 0)
        hipLaunchKernelGGL(pcp::k_make_keys, dim3(pcp::grid_for(icp->nq, 256)), dim3(256), 0, ctx->stream, a,
                           (uint32_t)target_offset, keys_dev);
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

int pcp_icp_keys(pcp_ctx* ctx, pcp_icp* icp, const double T[16], float rmax, int64_t target_offset,
                 uint64_t* keys_dev) {
    return icp_keys(ctx, icp, T, nullptr, rmax, target_offset, keys_dev);
}

int pcp_icp_keys_dev(pcp_ctx* ctx, pcp_icp* icp, const double* T_dev, float rmax, int64_t target_offset,
                     uint64_t* keys_dev) {
    return icp_keys(ctx, icp, nullptr, T_dev, rmax, target_offset, keys_dev);
}

int pcp_icp_solve(const double acc[24], int do_scale, double dT[16]) {
    if (!acc || !dT) return PCP_ERR_ARG;
    return pcp::icp_solve(acc, do_scale, dT);
}

int pcp_icp_run(pcp_ctx* ctx, pcp_icp* icp, double T[16], float rmax, int iters, int do_scale, double eps,
                float* err) {
    if (!ctx || !icp || !T || iters < 0) return PCP_ERR_ARG;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    icp->ctx = ctx;
    double e = -1.0, ms_total = 0.0;
    int launches = 0;
    const pcp::LaunchReq rq = pcp::LaunchReq::host(T, rmax, icp->acc);  // (T is updated in place below)
    for (int it = 0; it < iters; it++) {
        PCP_TRY(pcp::icp_launch(icp, rq));
        double acc[24];
        PCP_HIP(ctx, hipMemcpyAsync(acc, icp->acc, sizeof(acc), hipMemcpyDeviceToHost, ctx->stream));
        PCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        float ms = 0.f;
        PCP_HIP(ctx, hipEventElapsedTime(&ms, icp->ev0, icp->ev1));
        ms_total += ms;
        launches++;
        double dT[16];
        if (pcp::icp_solve(acc, do_scale, dT) != PCP_OK) {
            e = -1.0;
            break;
        }
        e = std::sqrt(acc[22] / acc[0]);
        double Tn[16];
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) {
                double s = 0;
                for (int k = 0; k < 4; k++) s += dT[4 * i + k] * T[4 * k + j];
                Tn[4 * i + j] = s;
            }
        std::memcpy(T, Tn, sizeof(Tn));
        if (eps > 0) {
            double rot = std::fabs(dT[0] - 1) + std::fabs(dT[5] - 1) + std::fabs(dT[10] - 1) +
                         std::fabs(dT[1]) + std::fabs(dT[2]) + std::fabs(dT[6]);
            double tr = std::fabs(dT[3]) + std::fabs(dT[7]) + std::fabs(dT[11]);
            if (rot < eps && tr < eps) break;
        }
    }
    icp->last_ms = ms_total;
    icp->last_launches = launches;
    if (err) *err = (float)e;
    return e < 0 ? PCP_ERR_ICP : PCP_OK;
}

int pcp_icp_step_dev(pcp_ctx* ctx, pcp_icp* icp, const double* T_dev, float rmax, double* acc_dev) {
    if (!ctx || !icp || !T_dev || !acc_dev || !(rmax >= 0.f)) return PCP_ERR_ARG;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    icp->ctx = ctx;
    return pcp::icp_launch(icp, pcp::LaunchReq::dev(T_dev, rmax, acc_dev));
}

int pcp_icp_solve_dev(pcp_ctx* ctx, const double* acc_dev, int do_scale, double* T_dev, double* stats_dev) {
    if (!ctx || !acc_dev || !T_dev || !stats_dev) return PCP_ERR_ARG;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(pcp::k_icp_solve_dev, dim3(1), dim3(1), 0, ctx->stream, acc_dev, do_scale, T_dev, stats_dev);
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

int pcp_icp_run_dev(pcp_ctx* ctx, pcp_icp* icp, double* T_dev, float rmax, int iters, int do_scale,
                    double* stats_dev) {
    if (!ctx || !icp || !T_dev || !stats_dev || iters < 0 || !(rmax >= 0.f)) return PCP_ERR_ARG;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    icp->ctx = ctx;
    const pcp::LaunchReq rq = pcp::LaunchReq::dev(T_dev, rmax, icp->acc);
    for (int it = 0; it < iters; it++) {
        PCP_TRY(pcp::icp_launch(icp, rq));
        hipLaunchKernelGGL(pcp::k_icp_solve_dev, dim3(1), dim3(1), 0, ctx->stream, (const double*)icp->acc, do_scale,
                           T_dev, stats_dev);
    }
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

int pcp_icp_kernel_ms(pcp_ctx* ctx, pcp_icp* icp, double* ms, int* launches) {
    if (!ctx || !icp) return PCP_ERR_ARG;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    double tot = 0.0;
    for (size_t i = 0; i < icp->ntev; i++) {
        PCP_HIP(ctx, hipEventSynchronize(icp->tev[i].second));
        float m = 0.f;
        PCP_HIP(ctx, hipEventElapsedTime(&m, icp->tev[i].first, icp->tev[i].second));
        tot += m;
    }
    if (ms) *ms = tot;
    if (launches) *launches = (int)icp->ntev;
    icp->ntev = 0;
    return PCP_OK;
}

int pcp_icp_last_fallback(const pcp_icp* icp, int64_t* n) {
    if (!icp || !n) return PCP_ERR_ARG;
    *n = icp->last_fallback;
    return PCP_OK;
}

int pcp_icp_last_searched(const pcp_icp* icp, int64_t* n) {
    if (!icp || !n) return PCP_ERR_ARG;
    *n = icp->last_searched;
    return PCP_OK;
}

int pcp_icp_last_lookahead(const pcp_icp* icp, double* beta, double* max_offset_m) {
    if (!icp || !icp->ctx) return PCP_ERR_ARG;
    pcp_ctx* ctx = icp->ctx;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    float w[2] = {0.f, 0.f};
    PCP_HIP(ctx, hipMemcpyAsync(w, &icp->pose_dev->beta, sizeof(w), hipMemcpyDeviceToHost, ctx->stream));
    PCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (beta) *beta = w[0];
    if (max_offset_m) *max_offset_m = w[1];
    return PCP_OK;
}

int pcp_icp_predict_first(pcp_icp* icp, const double T1[16]) {
    if (!icp || !T1) return PCP_ERR_ARG;
    if (icp->launches > 0)
        return pcp::set_error(icp->owner, PCP_ERR_ARG, "pcp_icp_predict_first only before the handle's first launch");
    std::memcpy(icp->pred, T1, sizeof(icp->pred));
    icp->has_pred = true;
    return PCP_OK;
}

int pcp_icp_pilot_info(const pcp_icp* icp, int64_t* stride, int64_t* chunks, int64_t* pairs) {
    if (!icp || !icp->ctx) return PCP_ERR_ARG;
    pcp_ctx* ctx = icp->ctx;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    float w = -1.f;
    PCP_HIP(ctx, hipMemcpyAsync(&w, &icp->pose_dev->pilot_pairs, sizeof(w), hipMemcpyDeviceToHost, ctx->stream));
    PCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const bool ran = icp->launches > 0 && w >= 0.f;
    const int64_t nch = (icp->nq + 63) / 64, s = std::max<int64_t>(1, nch / pcp::kPilotChunks);
    if (stride) *stride = ran ? s : 0;
    if (chunks) *chunks = ran ? (nch + s - 1) / s : 0;
    if (pairs) *pairs = ran ? (int64_t)w : -1;
    return PCP_OK;
}

int pcp_icp_last_kernel_ms(const pcp_icp* icp, double* ms, int* launches) {
    if (!icp) return PCP_ERR_ARG;
    if (ms) *ms = icp->last_ms;
    if (launches) *launches = icp->last_launches;
    return PCP_OK;
}

}  // extern "C"
