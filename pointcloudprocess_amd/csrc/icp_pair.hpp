// What a consumer does with one 64-bit correspondence key and the pair it names, written once: the
// key's layout, the fp32 cast of a pose, the usable-pair test / residual / 30 terms of the
// point-to-plane accumulation (pcp.h I2, I3b, I5), the 23 terms of the Kabsch accumulation, and the
// fixed-order block reductions behind them.  icp.hip, icp_shard.hip, icp_plane.hip, icp_trim.hip and
// icp_batch.hip build their key kernels from these, so "the same arithmetic" is the same text.
#pragma once
#include "icp_plane_solve.hpp"
#include "icp_search.hpp"

namespace pcp {

// ---- the key: (fp32 bits of d2) << 32 | target index, so an unsigned MIN is the lexicographic
// (d2, index) winner (non-negative fp32 bit patterns order like the values); INT64_MAX = no pair
constexpr uint64_t kNoKey = 0x7fffffffffffffffull;
__device__ __forceinline__ uint64_t key_make(uint32_t d2_bits, uint32_t index) {
    return ((uint64_t)d2_bits << 32) | index;
}
__device__ __forceinline__ uint64_t key_make(float d2, uint32_t index) { return key_make(__float_as_uint(d2), index); }
__device__ __forceinline__ uint32_t key_index(uint64_t key) { return (uint32_t)key; }
__device__ __forceinline__ uint32_t key_d2_bits(uint64_t key) { return (uint32_t)(key >> 32); }
__device__ __forceinline__ float key_d2(uint64_t key) { return __uint_as_float(key_d2_bits(key)); }

// ---- the pose the contract's fp32 chain (xform, icp_search.hpp) runs on: a row-major 4x4 of
// doubles cast entry by entry
struct Pose32 {
    float R[9], t[3];
};
__host__ __device__ inline Pose32 pose32(const double* T) {
    Pose32 p;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) p.R[3 * r + c] = (float)T[4 * r + c];
        p.t[r] = (float)T[4 * r + 3];
    }
    return p;
}

// ---- point-to-plane: the record pair a key names
struct PlanePair {
    float4 p, n;
};
// usable (pcp.h I2): a pair, its index inside the table, a valid normal.  The normal half is
// loaded first and the point half only for a valid record.
__device__ __forceinline__ bool plane_pair(uint64_t key, const float4* rec, uint64_t nrec, PlanePair& pr) {
    const uint64_t j = key_index(key);
    if (key == kNoKey || j >= nrec) return false;
    pr.n = rec[2 * j + 1];
    if (!plane_valid(pr.n.x, pr.n.y, pr.n.z)) return false;
    pr.p = rec[2 * j];
    return true;
}
// r = n . (Tq - p) at the query image (x, y, z).  Widened fp32 values, plain fp64 operations (no
// contraction) in this order: negating n negates r exactly.
__device__ __forceinline__ double plane_residual(float x, float y, float z, const PlanePair& pr) {
    const double qx = x, qy = y, qz = z, nx = pr.n.x, ny = pr.n.y, nz = pr.n.z;
    return (nx * (qx - (double)pr.p.x) + ny * (qy - (double)pr.p.y)) + nz * (qz - (double)pr.p.z);
}
// the pair's 30 terms (pcp.h): 1, the upper triangle of J J^T with J = (Tq x n, n), r J, r^2, d2.
// Negating n negates J and r, so every term is unchanged.
__device__ __forceinline__ void plane_terms(float x, float y, float z, const PlanePair& pr, uint64_t key,
                                            double term[kPAcc]) {
    const double qx = x, qy = y, qz = z, nx = pr.n.x, ny = pr.n.y, nz = pr.n.z;
    double J[6];
    J[0] = qy * nz - qz * ny;
    J[1] = qz * nx - qx * nz;
    J[2] = qx * ny - qy * nx;
    J[3] = nx; J[4] = ny; J[5] = nz;
    const double r = plane_residual(x, y, z, pr);
    term[0] = 1.0;
    int k = 1;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = a; b < 6; b++) term[k++] = J[a] * J[b];
#pragma unroll
    for (int a = 0; a < 6; a++) term[22 + a] = r * J[a];
    term[28] = r * r;
    term[29] = (double)key_d2(key);
}

// ---- Kabsch: acc += the pair's 23 terms n, A(3), B(3), AB(9), AA(6), D for the query image qv and
// its target pv.  Products of widened fp32 values are exact in fp64.
constexpr int kAcc = 24;  // the 23 sums, then the fallback count of the search kernels
__device__ __forceinline__ void kabsch_terms(const double qv[3], const double pv[3], uint64_t key,
                                             double acc[kAcc - 1]) {
    acc[0] += 1.0;
#pragma unroll
    for (int c = 0; c < 3; c++) { acc[1 + c] += qv[c]; acc[4 + c] += pv[c]; }
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) acc[7 + 3 * r + c] += qv[r] * pv[c];
    acc[16] += qv[0] * qv[0]; acc[17] += qv[0] * qv[1]; acc[18] += qv[0] * qv[2];
    acc[19] += qv[1] * qv[1]; acc[20] += qv[1] * qv[2]; acc[21] += qv[2] * qv[2];
    acc[22] += (double)key_d2(key);
}

// ---- reductions of a block of kPairBlock threads (whole block calls).  The trees are fixed: lanes
// by xor offsets 32 .. 1, then waves 0 .. 3, so a sum is the same bit for bit on every run.
constexpr int kPairBlock = 256;
constexpr int kPairWaves = kPairBlock / 64;

// per-lane sums acc[0 .. N) -> row[0 .. NOUT) of the block; row[N .. NOUT) = 0
template <int N, int NOUT = N>
__device__ __forceinline__ void block_partials(const double (&acc)[N], double* row) {
    __shared__ double sm[kPairWaves][NOUT];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; k++) {
        double v = acc[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) sm[wv][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < NOUT) {
        double v = 0.0;
        if (NOUT == N || threadIdx.x < N)
            for (int w = 0; w < kPairWaves; w++) v += sm[w][threadIdx.x];
        row[threadIdx.x] = v;
    }
}

// one block: out[k] = sum over the nb rows of block_partials, k = 0 .. N (out may be LDS; ends with
// a barrier)
template <int N>
__device__ __forceinline__ void sum_partials(const double* part, int nb, double* out) {
    __shared__ double s[kPairBlock];
    for (int k = 0; k < N; k++) {
        double v = 0.0;
        for (int b = threadIdx.x; b < nb; b += kPairBlock) v += part[(int64_t)b * N + k];
        s[threadIdx.x] = v;
        __syncthreads();
        for (int o = kPairBlock / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[k] = s[0];
        __syncthreads();
    }
}

// the block's total of cnt.  Every thread may read it, and the callers use it in thread 0 only: a
// total that is block-uniform to the compiler keeps the one atomic that follows a plain add.
__device__ __forceinline__ uint32_t block_count(uint32_t cnt) {
    __shared__ uint32_t sm[kPairWaves];
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = cnt;
    __syncthreads();
    uint32_t t = 0;
    for (int w = 0; w < kPairWaves; w++) t += sm[w];
    return t;
}

}  // namespace pcp
