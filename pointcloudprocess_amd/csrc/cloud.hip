// Cloud-level passes over AoS48 PointXYZRGBA clouds (point_type.h:9-82, 48-byte stride):
//   getMinMax3D       point_cloud_helper.h:59-90     (V2)
//   compute3DCentroid point_cloud_helper.h:193-230   (I3)
//   transformPointCloud point_cloud_helper.h:92-127  (I2)
//   VoxelGrid::applyFilter voxel_grid.h:811-1056     (V3)
//   remove_duplicate  point_cloud_helper.cpp:42-63   (V4)
//   get_rot_icp       point_cloud_helper.cpp:75-166  (I1, front-end of the ICP kernels)
// and, for a span of segments with one pose each (not in the reference): the moved segments'
// min/max (V, pcp_minmax_segments_aos48) and get_rot_icp's staging around the batch loops (I5d).
//
// All passes stream the 48-byte records once (HBM-bound).  The voxel sort is rocPRIM's
// device radix sort (LSD, stable) on u32 voxel keys; keying, run detection and the
// per-voxel averaging are the kernels below.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>


#include "sortcfg.hpp"

namespace pcp {
namespace {

constexpr int kB = 256;
constexpr int kRedBlocks = 1024;

struct P48 {
    double x, y, z, w;
    uint32_t rgba, stamp_id, pad0, pad1;
};
static_assert(sizeof(P48) == PCP_AOS48_STRIDE, "AoS48 layout");

__device__ __forceinline__ double wave_min(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// V2: per-block min/max of data[0..3] over (finite unless is_dense) points.  Eigen's
// min/max on a non-NaN running value are exact, so any reduction order gives the
// reference's result; max starts at DBL_MIN (point_cloud_helper.h:64-65).
__global__ __launch_bounds__(kB) void k_minmax48(const P48* in, int64_t n, int is_dense, double* part) {
    double mn[4] = {DBL_MAX, DBL_MAX, DBL_MAX, DBL_MAX}, mx[4] = {DBL_MIN, DBL_MIN, DBL_MIN, DBL_MIN};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const P48 p = in[i];
        if (!is_dense && !finite3(p.x, p.y, p.z)) continue;
        const double v[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
        for (int a = 0; a < 4; a++) {
            if (v[a] < mn[a]) mn[a] = v[a];
            if (mx[a] < v[a]) mx[a] = v[a];
        }
    }
    __shared__ double sm[kB / 64][8];
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const double a0 = wave_min(mn[a]), a1 = wave_max(mx[a]);
        if (ln == 0) { sm[wv][a] = a0; sm[wv][4 + a] = a1; }
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        double r = sm[0][threadIdx.x];
        for (int w = 1; w < kB / 64; w++) r = threadIdx.x < 4 ? fmin(r, sm[w][threadIdx.x]) : fmax(r, sm[w][threadIdx.x]);
        part[blockIdx.x * 8 + threadIdx.x] = r;
    }
}

// I2: p <- R p + t with Eigen's lazy product order ((r0 x + r1 y) + r2 z) + t.
struct Xf {
    double m[12];
};
__device__ __forceinline__ void xform(const Xf& T, double x, double y, double z, double o[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double acc = T.m[4 * r + 0] * x;
        acc = acc + T.m[4 * r + 1] * y;
        acc = acc + T.m[4 * r + 2] * z;
        o[r] = acc + T.m[4 * r + 3];
    }
}

__global__ __launch_bounds__(kB) void k_transform48(const P48* in, P48* out, int64_t n, int is_dense, Xf T) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        P48 p = in[i];
        if (is_dense || finite3(p.x, p.y, p.z)) {
            double o[3];
            xform(T, p.x, p.y, p.z, o);
            p.x = o[0]; p.y = o[1]; p.z = o[2];
        }
        out[i] = p;
    }
}

// V4 step 1-2: copyPointCloud (registered fields only, data[3] = 1) fused with the
// centring transform (point_cloud_helper.cpp:46-53)
__global__ __launch_bounds__(kB) void k_copy_centre(const P48* in, P48* out, int64_t n, int is_dense, Xf T) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const P48 s = in[i];
        P48 p{s.x, s.y, s.z, 1.0, s.rgba, s.stamp_id, 0u, 0u};
        if (is_dense || finite3(p.x, p.y, p.z)) {
            double o[3];
            xform(T, p.x, p.y, p.z, o);
            p.x = o[0]; p.y = o[1]; p.z = o[2];
        }
        out[i] = p;
    }
}

// V3 keying (voxel_grid.h:928-943): ijk_a = (int)(double(p_a*inv_a) - min_b_a), linear index
// i + j*div_b0 + k*div_b0*div_b1 in wrapping int32 arithmetic, kept as u32.
struct VoxGeom {
    double inv[3];
    double min_b[3];
    uint32_t mul1, mul2;
};

__global__ __launch_bounds__(kB) void k_vox_flag(const P48* in, int64_t n, int is_dense, uint32_t* flag) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const P48 p = in[i];
        flag[i] = (is_dense || finite3(p.x, p.y, p.z)) ? 1u : 0u;
    }
}

__global__ __launch_bounds__(kB) void k_vox_key(const P48* in, int64_t n, int is_dense, VoxGeom g,
                                                const uint32_t* pos, uint32_t* keys, uint32_t* vals) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const P48 p = in[i];
        if (!is_dense && !finite3(p.x, p.y, p.z)) continue;
        const int i0 = (int)((p.x * g.inv[0]) - g.min_b[0]);
        const int i1 = (int)((p.y * g.inv[1]) - g.min_b[1]);
        const int i2 = (int)((p.z * g.inv[2]) - g.min_b[2]);
        const uint32_t idx = (uint32_t)i0 + (uint32_t)i1 * g.mul1 + (uint32_t)i2 * g.mul2;
        const uint32_t o = is_dense ? (uint32_t)i : pos[i];
        keys[o] = idx;
        vals[o] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(kB) void k_run_heads(const uint32_t* keys, int64_t m, uint32_t* head) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x)
        head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// head[] holds the exclusive scan of the run-head flags: run r starts at the i whose flag
// was set and whose scan value is r.
__global__ __launch_bounds__(kB) void k_run_starts(const uint32_t* keys, const uint32_t* headscan, int64_t m,
                                                   uint32_t* start) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x)
        if (i == 0 || keys[i] != keys[i - 1]) start[headscan[i]] = (uint32_t)i;
}

// V3 averaging (voxel_grid.h:985-1054), one lane per voxel, members in input order
// (the stable restatement of the unstable std::sort).
__global__ __launch_bounds__(kB) void k_vox_reduce(const P48* in, const uint32_t* keys, const uint32_t* vals,
                                                   const uint32_t* start, int64_t nvox, int64_t m, int all_data,
                                                   P48* out, uint32_t* out_vidx) {
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t s = start[v];
        const uint32_t e = v + 1 < nvox ? start[v + 1] : (uint32_t)m;
        P48 o{0, 0, 0, 1.0, 0u, 0u, 0u, 0u};
        const double dn = (double)(e - s);
        if (!all_data) {
            double c0 = 0, c1 = 0, c2 = 0;
            for (uint32_t t = s; t < e; t++) {
                const P48 p = in[vals[t]];
                c0 += p.x; c1 += p.y; c2 += p.z;
            }
            o.x = c0 / dn; o.y = c1 / dn; o.z = c2 / dn;
        } else {
            // x,y,z,rgba,stamp_id through static_cast<float> (concatenate.h:153), then the
            // r,g,b bytes (voxel_grid.h:995-1004); first member assigned, the rest added
            double c[8];
            for (uint32_t t = s; t < e; t++) {
                const P48 p = in[vals[t]];
                const double tv[8] = {(double)(float)p.x, (double)(float)p.y, (double)(float)p.z,
                                      (double)(float)p.rgba, (double)(float)p.stamp_id,
                                      (double)((p.rgba >> 16) & 0xFF), (double)((p.rgba >> 8) & 0xFF),
                                      (double)(p.rgba & 0xFF)};
                if (t == s) {
#pragma unroll
                    for (int f = 0; f < 8; f++) c[f] = tv[f];
                } else {
#pragma unroll
                    for (int f = 0; f < 8; f++) c[f] += tv[f];
                }
            }
#pragma unroll
            for (int f = 0; f < 8; f++) c[f] /= dn;  // :1034
            o.x = c[0]; o.y = c[1]; o.z = c[2];
            o.rgba = (uint32_t)c[3];
            o.stamp_id = (uint32_t)c[4];
            const float r = (float)c[5], gg = (float)c[6], b = (float)c[7];  // :1045-1050
            o.rgba = (uint32_t)(((int)r << 16) | ((int)gg << 8) | (int)b);
        }
        out[v] = o;
        if (out_vidx) out_vidx[v] = keys[s];
    }
}

// I1: float(p - c) vertices (point_cloud_helper.cpp:89-104)
__global__ __launch_bounds__(kB) void k_centre_f32(const P48* in, int64_t n, double c0, double c1, double c2, float* v) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const P48 p = in[i];
        v[3 * i + 0] = (float)(p.x - c0);
        v[3 * i + 1] = (float)(p.y - c1);
        v[3 * i + 2] = (float)(p.z - c2);
    }
}

// ---- passes over a span of segments, each with its own pose: one launch whatever nseg is.
// The host cuts every segment into tiles of kSegTile records (segtab[nseg + 1 + s] = the first tile
// of segment s, empty segments own none); a workgroup takes whole tiles, finds a tile's segment by
// bisection of that table (uniform over the workgroup) and reads the segment's pose once per tile.
constexpr int kSegTile = 2048;
constexpr int kSegBlocks = 1 << 16;

struct SegTile {
    int s;
    int64_t begin, end;  // records [begin, end) of the span
};
__device__ __forceinline__ SegTile seg_tile(const int64_t* segtab, int nseg, int64_t t) {
    const int64_t* first = segtab + nseg + 1;
    int lo = 0, hi = nseg;  // first[lo] <= t < first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= t) lo = mid; else hi = mid;
    }
    SegTile r;
    r.s = lo;
    r.begin = segtab[lo] + (t - first[lo]) * kSegTile;
    r.end = r.begin + kSegTile < segtab[lo + 1] ? r.begin + kSegTile : segtab[lo + 1];
    return r;
}
__device__ __forceinline__ Xf load_xf(const double* T16) {
    Xf x;
#pragma unroll
    for (int i = 0; i < 12; i++) x.m[i] = T16[i];
    return x;
}

// the workgroup's min / max of 4 + 4 running values into dst[0..7] (k_minmax48's reduction)
__device__ __forceinline__ void block_minmax8(const double mn[4], const double mx[4], double (*sm)[8], double* dst) {
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const double a0 = wave_min(mn[a]), a1 = wave_max(mx[a]);
        if (ln == 0) { sm[wv][a] = a0; sm[wv][4 + a] = a1; }
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        double r = sm[0][threadIdx.x];
        for (int w = 1; w < kB / 64; w++) r = threadIdx.x < 4 ? fmin(r, sm[w][threadIdx.x]) : fmax(r, sm[w][threadIdx.x]);
        dst[threadIdx.x] = r;
    }
    __syncthreads();  // sm is reused by the caller's next tile
}

// V2 of transformPointCloud(segment s, T_s), per tile, without the moved copy: k_transform48's
// rule (a non-finite point of a non-dense cloud stays as it is), then k_minmax48's (a non-finite
// point of a non-dense cloud is skipped; data[3] rides along untransformed).
__global__ __launch_bounds__(kB) void k_minmax_seg_tiles(const P48* in, const int64_t* segtab, int nseg,
                                                         int64_t ntiles, const double* Ts, int is_dense,
                                                         double* part /* ntiles x 8 */) {
    __shared__ double sm[kB / 64][8];
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const SegTile st = seg_tile(segtab, nseg, t);
        const Xf T = load_xf(Ts + 16 * (int64_t)st.s);
        double mn[4] = {DBL_MAX, DBL_MAX, DBL_MAX, DBL_MAX}, mx[4] = {DBL_MIN, DBL_MIN, DBL_MIN, DBL_MIN};
        for (int64_t i = st.begin + threadIdx.x; i < st.end; i += kB) {
            const P48 p = in[i];
            double v[4] = {p.x, p.y, p.z, p.w};
            if (is_dense || finite3(p.x, p.y, p.z)) xform(T, p.x, p.y, p.z, v);
            if (!is_dense && !finite3(v[0], v[1], v[2])) continue;
#pragma unroll
            for (int a = 0; a < 4; a++) {
                if (v[a] < mn[a]) mn[a] = v[a];
                if (mx[a] < v[a]) mx[a] = v[a];
            }
        }
        block_minmax8(mn, mx, sm, part + 8 * t);
    }
}

// one workgroup per segment: its tiles' rows into row s (an empty segment: DBL_MAX / DBL_MIN)
__global__ __launch_bounds__(kB) void k_minmax_seg_rows(const double* part, const int64_t* segtab, int nseg,
                                                        double* rows /* nseg x 8 */) {
    __shared__ double sm[kB / 64][8];
    const int s = blockIdx.x;
    const int64_t* first = segtab + nseg + 1;
    double mn[4] = {DBL_MAX, DBL_MAX, DBL_MAX, DBL_MAX}, mx[4] = {DBL_MIN, DBL_MIN, DBL_MIN, DBL_MIN};
    for (int64_t t = first[s] + threadIdx.x; t < first[s + 1]; t += kB) {
#pragma unroll
        for (int a = 0; a < 4; a++) {
            const double lo = part[8 * t + a], hi = part[8 * t + 4 + a];
            if (lo < mn[a]) mn[a] = lo;
            if (mx[a] < hi) mx[a] = hi;
        }
    }
    block_minmax8(mn, mx, sm, rows + 8 * (int64_t)s);
}

// I5d staging: q32_i = float(xform(T0_s, p_i) - c), k_transform48's rule for a non-finite point of
// a non-dense cloud (it stays, and its fp32 image is non-finite: a query without a key), then
// k_centre_f32's arithmetic.
__global__ __launch_bounds__(kB) void k_stage_seg_f32(const P48* in, const int64_t* segtab, int nseg, int64_t ntiles,
                                                      const double* Ts, int is_dense, double c0, double c1, double c2,
                                                      float* v) {
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const SegTile st = seg_tile(segtab, nseg, t);
        const Xf T = load_xf(Ts + 16 * (int64_t)st.s);
        for (int64_t i = st.begin + threadIdx.x; i < st.end; i += kB) {
            const P48 p = in[i];
            double o[3] = {p.x, p.y, p.z};
            if (is_dense || finite3(p.x, p.y, p.z)) xform(T, p.x, p.y, p.z, o);
            v[3 * i + 0] = (float)(o[0] - c0);
            v[3 * i + 1] = (float)(o[1] - c1);
            v[3 * i + 2] = (float)(o[2] - c2);
        }
    }
}

}  // namespace

namespace {

// segment rules of pcp_icp_batch_create over a span of n records
bool seg_offsets_ok(const int64_t* off, int nseg, int64_t n) {
    if (!off || nseg < 0 || nseg > 65535 || off[0] != 0 || off[nseg] != n) return false;
    for (int s = 0; s < nseg; s++)
        if (off[s + 1] < off[s]) return false;
    return true;
}

// The device tables of the segment passes: segtab = offsets (nseg + 1) ++ first tile per segment
// (nseg + 1), Ts = nseg x 16 poses (the identity for a null T_host: the passes then run xform with
// it, so a null pose and an explicit identity give the same bits).  The uploads read this object's
// host arrays, so it waits for the stream before they go.
struct SegTable {
    pcp_ctx* ctx;
    std::vector<int64_t> h;
    std::vector<double> hT;
    int64_t* segtab = nullptr;
    double* Ts = nullptr;
    int64_t ntiles = 0;
    bool inflight = false;
    explicit SegTable(pcp_ctx* c) : ctx(c) {}
    ~SegTable() {
        if (inflight) (void)hipStreamSynchronize(ctx->stream);
    }
    int upload(Tmp& tmp, const int64_t* off, int nseg, const double* T_host) {
        h.assign(2 * ((size_t)nseg + 1), 0);
        for (int s = 0; s <= nseg; s++) h[s] = off[s];
        for (int s = 0; s < nseg; s++) {
            h[(size_t)nseg + 1 + s] = ntiles;
            ntiles += (off[s + 1] - off[s] + kSegTile - 1) / kSegTile;
        }
        h[2 * (size_t)nseg + 1] = ntiles;
        hT.resize(16 * (size_t)nseg);
        for (size_t i = 0; i < hT.size(); i++) hT[i] = T_host ? T_host[i] : (i % 16 % 5 == 0 ? 1.0 : 0.0);
        PCP_TRY(tmp.get(&segtab, h.size()));
        PCP_TRY(tmp.get(&Ts, hT.size()));
        inflight = true;
        PCP_HIP(ctx, hipMemcpyAsync(segtab, h.data(), h.size() * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
        if (nseg > 0)
            PCP_HIP(ctx, hipMemcpyAsync(Ts, hT.data(), hT.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        return PCP_OK;
    }
    unsigned grid() const { return (unsigned)(ntiles < kSegBlocks ? (ntiles > 0 ? ntiles : 1) : kSegBlocks); }
};

}  // namespace

int minmax_aos48_dev(pcp_ctx* ctx, const void* in, int64_t n, int is_dense, double mn[4], double mx[4]) {
    for (int a = 0; a < 4; a++) { mn[a] = DBL_MAX; mx[a] = DBL_MIN; }
    if (n <= 0) return PCP_OK;
    const unsigned nb = grid_for(n, kB, kRedBlocks);
    Tmp tmp(ctx);
    double* part;
    PCP_TRY(tmp.get(&part, 8 * (size_t)nb));
    hipLaunchKernelGGL(k_minmax48, dim3(nb), dim3(kB), 0, ctx->stream, (const P48*)in, n, is_dense, part);
    std::vector<double> h(8 * nb);
    hipError_t e = hipMemcpyAsync(h.data(), part, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "minmax", __FILE__, __LINE__);
    for (unsigned b = 0; b < nb; b++)
        for (int a = 0; a < 4; a++) {
            if (h[8 * b + a] < mn[a]) mn[a] = h[8 * b + a];
            if (mx[a] < h[8 * b + 4 + a]) mx[a] = h[8 * b + 4 + a];
        }
    return PCP_OK;
}

int centroid_aos48_dev(pcp_ctx* ctx, const void* in, int64_t n, int is_dense, double c[4], uint32_t* count) {
    if (n <= 0) {  // point_cloud_helper.h:197-198: centroid untouched, 0 returned
        if (count) *count = 0;
        return PCP_OK;
    }
    // the reference's sequential left fold, bit for bit (point_cloud_helper.h:199-227)
    double s[4];
    PCP_TRY(seqfold_aos48(ctx, in, n, nullptr, 0, is_dense, s));
    const uint32_t cp = is_dense ? (uint32_t)n : (uint32_t)s[3];
    const double dn = is_dense ? (double)n : (double)cp;  // size() (size_t) or unsigned cp
    c[0] = s[0] / dn; c[1] = s[1] / dn; c[2] = s[2] / dn; c[3] = 0.0 / dn;
    if (count) *count = cp;
    return PCP_OK;
}

static Xf make_xf(const double T[16]) {
    Xf x;
    for (int i = 0; i < 12; i++) x.m[i] = T[i];
    return x;
}

// V3 on device: returns the voxel count through *n_out
static int voxel_filter_impl(pcp_ctx* ctx, const P48* in, int64_t n, int is_dense, const double leaf[3], int all_data,
                             P48* out, int64_t* n_out, uint32_t* out_vidx) {
    *n_out = 0;
    if (n <= 0) return PCP_OK;  // voxel_grid.h:815-820
    if (n >= (int64_t)1 << 32) return set_error(ctx, PCP_ERR_ARG, "voxel filter supports < 2^32 points");
    hipStream_t st = ctx->stream;
    // setLeafSize (voxel_grid.h:538-549): inverse by array division
    VoxGeom g;
    for (int a = 0; a < 3; a++) g.inv[a] = 1.0 / leaf[a];
    double mn[4], mx[4];
    PCP_TRY(minmax_aos48_dev(ctx, in, n, is_dense, mn, mx));  // :831
    int min_b[3], max_b[3], div_b[3];
    for (int a = 0; a < 3; a++) {  // :835-843, truncating casts
        min_b[a] = (int)(double)(mn[a] * g.inv[a]);
        max_b[a] = (int)(double)(mx[a] * g.inv[a]);
        div_b[a] = max_b[a] - min_b[a] + 1;
        g.min_b[a] = (double)min_b[a];
    }
    g.mul1 = (uint32_t)div_b[0];  // divb_mul_ in wrapping int32 (:847)
    g.mul2 = (uint32_t)div_b[0] * (uint32_t)div_b[1];

    Tmp tmp(ctx);
    uint32_t *k0, *k1, *v0, *v1, *head, *flag = nullptr;
    PCP_TRY(tmp.get(&k0, n));
    PCP_TRY(tmp.get(&k1, n));
    PCP_TRY(tmp.get(&v0, n));
    PCP_TRY(tmp.get(&v1, n));
    PCP_TRY(tmp.get(&head, n + 1));
    int64_t m = n;
    if (!is_dense) {
        PCP_TRY(tmp.get(&flag, n + 1));
        hipLaunchKernelGGL(k_vox_flag, dim3(grid_for(n, kB)), dim3(kB), 0, st, in, n, is_dense, flag);
        uint32_t valid = 0;
        PCP_TRY(scan_u32_inplace(ctx, flag, n, &valid));
        m = valid;
    }
    hipLaunchKernelGGL(k_vox_key, dim3(grid_for(n, kB)), dim3(kB), 0, st, in, n, is_dense, g, flag, k0, v0);
    PCP_LAUNCH_CHECK(ctx);
    if (m == 0) return PCP_OK;
    // stable LSD radix sort by the u32 key (voxel_grid.h:948)
    PCP_TRY(sort_pairs(tmp, k0, k1, v0, v1, (size_t)m, 0, 32));
    // runs of equal keys = voxels (:952-960)
    hipLaunchKernelGGL(k_run_heads, dim3(grid_for(m, kB)), dim3(kB), 0, st, k1, m, head);
    uint32_t nvox = 0;
    PCP_TRY(scan_u32_inplace(ctx, head, m, &nvox));
    uint32_t* start = k0;  // reuse
    hipLaunchKernelGGL(k_run_starts, dim3(grid_for(m, kB)), dim3(kB), 0, st, k1, head, m, start);
    hipLaunchKernelGGL(k_vox_reduce, dim3(grid_for(nvox, kB)), dim3(kB), 0, st, in, k1, v1, start,
                       (int64_t)nvox, m, all_data, out, out_vidx);
    PCP_LAUNCH_CHECK(ctx);
    PCP_HIP(ctx, hipStreamSynchronize(st));
    *n_out = nvox;
    return PCP_OK;
}

}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_minmax_aos48(pcp_ctx* ctx, const void* in, int64_t n, int is_dense, double mn[4], double mx[4]) {
    if (!ctx || n < 0 || (n > 0 && !in) || !mn || !mx) return set_error(ctx, PCP_ERR_ARG, "pcp_minmax_aos48: bad arguments");
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    return minmax_aos48_dev(ctx, in, n, is_dense, mn, mx);
}

int pcp_minmax_segments_aos48(pcp_ctx* ctx, const void* in, int64_t n, const int64_t* seg_offsets, int nseg,
                              int is_dense, const double* T_host, double* mn, double* mx) {
    if (!ctx || n < 0 || (n > 0 && !in) || !seg_offsets_ok(seg_offsets, nseg, n) || (nseg > 0 && (!mn || !mx)))
        return set_error(ctx, PCP_ERR_ARG, "pcp_minmax_segments_aos48: bad arguments");
    if (nseg == 0) return PCP_OK;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    Tmp tmp(ctx);
    SegTable tab(ctx);
    PCP_TRY(tab.upload(tmp, seg_offsets, nseg, T_host));
    double *part = nullptr, *rows = nullptr;
    PCP_TRY(tmp.get(&part, 8 * (size_t)tab.ntiles));
    PCP_TRY(tmp.get(&rows, 8 * (size_t)nseg));
    if (tab.ntiles > 0)
        hipLaunchKernelGGL(k_minmax_seg_tiles, dim3(tab.grid()), dim3(kB), 0, ctx->stream, (const P48*)in,
                           (const int64_t*)tab.segtab, nseg, tab.ntiles, (const double*)tab.Ts, is_dense, part);
    hipLaunchKernelGGL(k_minmax_seg_rows, dim3(nseg), dim3(kB), 0, ctx->stream, (const double*)part,
                       (const int64_t*)tab.segtab, nseg, rows);
    PCP_LAUNCH_CHECK(ctx);
    std::vector<double> h(8 * (size_t)nseg);
    PCP_HIP(ctx, hipMemcpyAsync(h.data(), rows, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    tab.inflight = false;
    for (int s = 0; s < nseg; s++)
        for (int a = 0; a < 4; a++) {
            mn[4 * s + a] = h[8 * (size_t)s + a];
            mx[4 * s + a] = h[8 * (size_t)s + 4 + a];
        }
    return PCP_OK;
}

int pcp_centroid_aos48(pcp_ctx* ctx, const void* in, int64_t n, int is_dense, double c[4], uint32_t* count) {
    if (!ctx || n < 0 || (n > 0 && !in) || !c) return set_error(ctx, PCP_ERR_ARG, "pcp_centroid_aos48: bad arguments");
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    return centroid_aos48_dev(ctx, in, n, is_dense, c, count);
}

int pcp_centroid_concat_aos48(pcp_ctx* ctx, const void* a, int64_t na, const void* b, int64_t nb, int is_dense,
                              double c[4], uint32_t* count) {
    if (!ctx || na < 0 || nb < 0 || (na > 0 && !a) || (nb > 0 && !b) || !c)
        return set_error(ctx, PCP_ERR_ARG, "pcp_centroid_concat_aos48: bad arguments");
    if (na + nb == 0) {
        if (count) *count = 0;
        return PCP_OK;
    }
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    double s[4];
    PCP_TRY(seqfold_aos48(ctx, a, na, b, nb, is_dense, s));
    const uint32_t cp = is_dense ? (uint32_t)(na + nb) : (uint32_t)s[3];
    const double dn = is_dense ? (double)(na + nb) : (double)cp;
    c[0] = s[0] / dn; c[1] = s[1] / dn; c[2] = s[2] / dn; c[3] = 0.0 / dn;
    if (count) *count = cp;
    return PCP_OK;
}

int pcp_transform_aos48(pcp_ctx* ctx, const void* in, void* out, int64_t n, int is_dense, const double T[16]) {
    if (!ctx || n < 0 || (n > 0 && (!in || !out)) || !T) return set_error(ctx, PCP_ERR_ARG, "pcp_transform_aos48: bad arguments");
    if (n == 0) return PCP_OK;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_transform48, dim3(grid_for(n, kB)), dim3(kB), 0, ctx->stream, (const P48*)in, (P48*)out, n,
                       is_dense, make_xf(T));
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

int pcp_voxel_filter(pcp_ctx* ctx, const void* in, int64_t n, int is_dense, const double leaf[3], int all_data,
                     void* out, int64_t* n_out, uint32_t* out_vidx) {
    if (!ctx || n < 0 || (n > 0 && (!in || !out)) || !leaf || !n_out)
        return set_error(ctx, PCP_ERR_ARG, "pcp_voxel_filter: bad arguments");
    for (int a = 0; a < 3; a++)
        if (!(leaf[a] > 0)) return set_error(ctx, PCP_ERR_ARG, "pcp_voxel_filter: leaf sizes must be > 0");
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    return voxel_filter_impl(ctx, (const P48*)in, n, is_dense, leaf, all_data, (P48*)out, n_out, out_vidx);
}

int pcp_remove_duplicate(pcp_ctx* ctx, const void* in, int64_t n, int is_dense, float leaf, void* out, int64_t* n_out) {
    if (!ctx || n < 0 || (n > 0 && (!in || !out)) || !n_out || !(leaf > 0))
        return set_error(ctx, PCP_ERR_ARG, "pcp_remove_duplicate: bad arguments");
    *n_out = 0;
    if (n == 0) return PCP_OK;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    double c[4] = {0, 0, 0, 0};
    PCP_TRY(centroid_aos48_dev(ctx, in, n, is_dense, c, nullptr));  // :45
    double T[16] = {1, 0, 0, -c[0], 0, 1, 0, -c[1], 0, 0, 1, -c[2], 0, 0, 0, 1};
    Tmp tmp(ctx);
    P48* cen = nullptr;  // the centred copy
    PCP_TRY(tmp.get(&cen, n));
    hipLaunchKernelGGL(k_copy_centre, dim3(grid_for(n, kB)), dim3(kB), 0, ctx->stream, (const P48*)in, cen, n, is_dense,
                       make_xf(T));
    const double lf = (double)leaf;  // float leaf widened (:57)
    const double l3[3] = {lf, lf, lf};
    int64_t m = 0;
    int rc = voxel_filter_impl(ctx, cen, n, is_dense, l3, 1, (P48*)out, &m, nullptr);
    if (rc == PCP_OK && m > 0) {
        T[3] = c[0]; T[7] = c[1]; T[11] = c[2];  // :60-61
        hipLaunchKernelGGL(k_transform48, dim3(grid_for(m, kB)), dim3(kB), 0, ctx->stream, (const P48*)out, (P48*)out,
                           m, 1, make_xf(T));
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = hip_fail(ctx, e, "remove_duplicate", __FILE__, __LINE__);
    }
    if (rc == PCP_OK) *n_out = m;
    return rc;
}

int pcp_get_rot_icp(pcp_ctx* ctx, const void* src, int64_t ns, int src_dense, const void* tmp, int64_t nt,
                    int tmp_dense, double M[16], float rmax, int iters, int do_scale, double cell_size, float* err) {
    if (!ctx || ns < 0 || nt < 0 || (ns > 0 && !src) || (nt > 0 && !tmp) || !M || iters < 0)
        return set_error(ctx, PCP_ERR_ARG, "pcp_get_rot_icp: bad arguments");
    if (err) *err = -1.0f;
    for (int i = 0; i < 16; i++) M[i] = (i % 5 == 0) ? 1.0 : 0.0;
    // the reference passes maxdist = 0 (point_cloud_helper.cpp:127), which makes trimesh2 derive
    // its own threshold from the clouds' overlap (ICP.h:17-28; library absent, not restated):
    // this build needs an explicit correspondence distance and says so instead of guessing one
    if (!(rmax > 0.f))
        return set_error(ctx, PCP_ERR_UNSUPPORTED,
                         "pcp_get_rot_icp: rmax must be > 0 (trimesh2's automatic maxdist = 0 is not provided)");
    if (ns == 0 || nt == 0) return PCP_OK;  // ICP fails: err < 0 (ICP.h:26-28)
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    // joint centroid over cloud_all = src ++ temp (point_cloud_helper.cpp:78-83): one sequential
    // fold over the concatenation; cloud_all.is_dense = src.is_dense && temp.is_dense
    // (PointCloud::operator+=), so a non-dense input skips non-finite points of both
    double s[4];
    const int joint_dense = src_dense && tmp_dense;
    PCP_TRY(seqfold_aos48(ctx, src, ns, tmp, nt, joint_dense, s));
    const double dn = joint_dense ? (double)(ns + nt) : (double)(uint32_t)s[3];  // size() / unsigned cp
    const double c[3] = {s[0] / dn, s[1] / dn, s[2] / dn};
    float* fs = nullptr;
    float* ft = nullptr;
    Tmp bufs(ctx);
    PCP_TRY(bufs.get(&fs, 3 * (size_t)ns));
    int rc = bufs.get(&ft, 3 * (size_t)nt);
    pcp_index* ix = nullptr;
    pcp_icp* icp = nullptr;
    if (rc == PCP_OK) {
        hipLaunchKernelGGL(k_centre_f32, dim3(grid_for(ns, kB)), dim3(kB), 0, ctx->stream, (const P48*)src, ns, c[0],
                           c[1], c[2], fs);
        hipLaunchKernelGGL(k_centre_f32, dim3(grid_for(nt, kB)), dim3(kB), 0, ctx->stream, (const P48*)tmp, nt, c[0],
                           c[1], c[2], ft);
        rc = pcp_index_build_f32(ctx, fs, 3 * sizeof(float), ns, cell_size, &ix);
    }
    if (rc == PCP_OK) rc = pcp_icp_create(ctx, ix, ft, 3 * sizeof(float), nt, &icp);
    double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    float e = -1.0f;
    if (rc == PCP_OK) {
        rc = pcp_icp_run(ctx, icp, T, rmax, iters, do_scale, 0.0, &e);
        if (rc == PCP_ERR_ICP) rc = PCP_OK;  // failure is reported through err < 0
    }
    if (rc == PCP_OK) {
        std::memcpy(M, T, sizeof(T));
        for (int r = 0; r < 3; r++) {  // t' = (t - R c) + c (:164)
            double rcv = M[4 * r] * c[0];
            rcv = rcv + M[4 * r + 1] * c[1];
            rcv = rcv + M[4 * r + 2] * c[2];
            M[4 * r + 3] = (M[4 * r + 3] - rcv) + c[r];
        }
        if (err) *err = e;
    }
    if (icp) pcp_icp_destroy(icp);
    if (ix) pcp_index_destroy(ix);
    return rc;
}

// I5d: pcp_get_rot_icp's staging for a span of frames, each moved by its own fp64 pose, around the
// point-to-point batch loops of I5c (called as they are).  The centre is the target's own centroid.
int pcp_get_rot_icp_batch(pcp_ctx* ctx, const void* target, int64_t nt, int target_dense, const void* frames, int64_t nq,
                          int frames_dense, const int64_t* seg_offsets, int nseg, const double* T0_host, float rmax,
                          int iters, int do_scale, const float* trim, double cell_size, double* mat_rot, float* err,
                          int32_t* steps, int64_t* kept) {
    if (!ctx || nt < 0 || nq < 0 || (nt > 0 && !target) || (nq > 0 && !frames) || !seg_offsets_ok(seg_offsets, nseg, nq) ||
        iters < 0 || (trim && !trim_args_ok(trim[0], trim[1], trim[2])) || (nseg > 0 && (!mat_rot || !err)))
        return set_error(ctx, PCP_ERR_ARG, "pcp_get_rot_icp_batch: bad arguments");
    if (int rc = pcp_icp_check_sizes(nt, nq))
        return set_error(ctx, rc, "pcp_get_rot_icp_batch: target or frames too large (pcp_icp_check_sizes)");
    if (!(rmax > 0.f))
        return set_error(ctx, PCP_ERR_UNSUPPORTED,
                         "pcp_get_rot_icp_batch: rmax must be > 0 (trimesh2's automatic maxdist = 0 is not provided)");
    if (nseg == 0) return PCP_OK;
    const size_t B = (size_t)nseg;
    // poses (16 B), stats (4 B), trim rows (4 B u64, zero until a trimmed iteration writes them)
    std::vector<double> pose(24 * B, 0.0);
    for (size_t s = 0; s < B; s++)
        for (int i = 0; i < 16; i += 5) pose[16 * s + i] = 1.0;
    double* stats = pose.data() + 16 * B;
    struct StreamWait {  // pose is read and written by stream-ordered copies: no return path frees it under one
        pcp_ctx* ctx;
        bool on = false;
        ~StreamWait() {
            if (on) (void)hipStreamSynchronize(ctx->stream);
        }
    } wait{ctx};
    double c[4] = {0, 0, 0, 0};
    if (nt > 0 && nq > 0) {
        PCP_HIP(ctx, hipSetDevice(ctx->device));
        PCP_TRY(centroid_aos48_dev(ctx, target, nt, target_dense, c, nullptr));
        Tmp bufs(ctx);
        // handles are destroyed on every path, the batch before its target index
        struct Handles {
            pcp_index* ix = nullptr;
            pcp_icp_batch* batch = nullptr;
            ~Handles() {
                if (batch) pcp_icp_batch_destroy(batch);
                if (ix) pcp_index_destroy(ix);
            }
        } h;
        float *ft = nullptr, *fq = nullptr;
        double* dpose = nullptr;
        PCP_TRY(bufs.get(&ft, 3 * (size_t)nt));
        PCP_TRY(bufs.get(&fq, 3 * (size_t)nq));
        PCP_TRY(bufs.get(&dpose, pose.size()));
        {
            SegTable tab(ctx);
            PCP_TRY(tab.upload(bufs, seg_offsets, nseg, T0_host));
            hipLaunchKernelGGL(k_centre_f32, dim3(grid_for(nt, kB)), dim3(kB), 0, ctx->stream, (const P48*)target, nt,
                               c[0], c[1], c[2], ft);
            hipLaunchKernelGGL(k_stage_seg_f32, dim3(tab.grid()), dim3(kB), 0, ctx->stream, (const P48*)frames,
                               (const int64_t*)tab.segtab, nseg, tab.ntiles, (const double*)tab.Ts, frames_dense, c[0],
                               c[1], c[2], fq);
            PCP_LAUNCH_CHECK(ctx);
            PCP_TRY(pcp_index_build_f32(ctx, ft, 3 * sizeof(float), nt, cell_size, &h.ix));  // waits for the stream
            bufs.free(tab.segtab);
            bufs.free(tab.Ts);
        }
        PCP_TRY(pcp_icp_batch_create(ctx, h.ix, fq, 3 * sizeof(float), nq, seg_offsets, nseg, &h.batch));
        bufs.free(fq);  // the handle keeps its own copy
        wait.on = true;
        PCP_HIP(ctx, hipMemcpyAsync(dpose, pose.data(), pose.size() * sizeof(double), hipMemcpyHostToDevice,
                                    ctx->stream));
        double* dstats = dpose + 16 * B;
        if (trim)
            PCP_TRY(pcp_icp_batch_run_trimmed_dev(ctx, h.batch, ft, 3 * sizeof(float), nt, dpose, rmax, trim[0],
                                                  trim[1], trim[2], iters, do_scale, dstats,
                                                  (uint64_t*)(dstats + 4 * B)));
        else
            PCP_TRY(pcp_icp_batch_run_dev(ctx, h.batch, ft, 3 * sizeof(float), nt, dpose, rmax, iters, do_scale,
                                          dstats));
        hipError_t e = hipMemcpyAsync(pose.data(), dpose, pose.size() * sizeof(double), hipMemcpyDeviceToHost,
                                      ctx->stream);
        const hipError_t e2 = hipStreamSynchronize(ctx->stream);
        wait.on = false;
        if (e == hipSuccess) e = e2;
        if (e != hipSuccess) return hip_fail(ctx, e, "pcp_get_rot_icp_batch", __FILE__, __LINE__);
    }
    for (size_t s = 0; s < B; s++) {
        double* M = mat_rot + 16 * s;
        const double* st = stats + 4 * s;
        if (st[3] > 0) {  // un-centring in pcp_get_rot_icp's order; a segment that never solved: the exact identity
            std::memcpy(M, pose.data() + 16 * s, 16 * sizeof(double));
            for (int r = 0; r < 3; r++) {
                double rcv = M[4 * r] * c[0];
                rcv = rcv + M[4 * r + 1] * c[1];
                rcv = rcv + M[4 * r + 2] * c[2];
                M[4 * r + 3] = (M[4 * r + 3] - rcv) + c[r];
            }
        } else {
            for (int i = 0; i < 16; i++) M[i] = (i % 5 == 0) ? 1.0 : 0.0;
        }
        err[s] = (st[0] == 0 && st[3] > 0) ? (float)st[1] : -1.0f;
        if (steps) steps[s] = (int32_t)st[3];
        if (kept) {
            uint64_t row[PCP_ICP_TRIM_STATS];
            std::memcpy(row, pose.data() + 20 * B + 4 * s, sizeof(row));
            kept[s] = (int64_t)row[1];
        }
    }
    return PCP_OK;
}

// pcp_get_rot_icp's staging (joint centroid, fp32 centring, fp32 target index, query set, the
// un-centring of t) around the point-to-plane device loop: the build's own contract (pcp.h, I2).
// trim = {frac, mult, d_floor} runs the trimmed loop (I3; by_plane: the loop that trims by the plane
// residual, I3b) and reports the pairs its last iteration kept; trim == nullptr is the plain loop.
static int get_rot_plane(pcp_ctx* ctx, const char* who, const void* src, int64_t ns, int src_dense, const void* tmp,
                         int64_t nt, int tmp_dense, double M[16], float rmax, const float* trim, bool by_plane,
                         int iters, int normals_k, double cell_size, float* err, int64_t* kept_out) {
    if (!ctx || ns < 0 || nt < 0 || (ns > 0 && !src) || (nt > 0 && !tmp) || !M || iters < 0 ||
        (trim && !trim_args_ok(trim[0], trim[1], trim[2])))
        return set_error(ctx, PCP_ERR_ARG, "%s: bad arguments", who);
    if (err) *err = -1.0f;
    if (kept_out) *kept_out = 0;
    for (int i = 0; i < 16; i++) M[i] = (i % 5 == 0) ? 1.0 : 0.0;
    if (!(rmax > 0.f))
        return set_error(ctx, PCP_ERR_UNSUPPORTED,
                         "%s: rmax must be > 0 (trimesh2's automatic maxdist = 0 is not provided)", who);
    if (ns == 0 || nt == 0) return PCP_OK;  // ICP fails: err < 0
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    double s[4];
    const int joint_dense = src_dense && tmp_dense;
    PCP_TRY(seqfold_aos48(ctx, src, ns, tmp, nt, joint_dense, s));
    const double dn = joint_dense ? (double)(ns + nt) : (double)(uint32_t)s[3];
    const double c[3] = {s[0] / dn, s[1] / dn, s[2] / dn};
    float* fs = nullptr;
    float* ft = nullptr;
    pcp_plane* nrm = nullptr;
    double* pose = nullptr;  // T (16), stats (4), the trimmed loop's trim stats (4 x u64)
    const size_t npose = trim ? 24 : 20;
    Tmp bufs(ctx);
    PCP_TRY(bufs.get(&fs, 3 * (size_t)ns));
    PCP_TRY(bufs.get(&ft, 3 * (size_t)nt));
    PCP_TRY(bufs.get(&pose, npose));
    // handles are destroyed on every path, the ICP handle before its target index
    struct Handles {
        pcp_index* ix = nullptr;
        pcp_index* ix64 = nullptr;
        pcp_icp* icp = nullptr;
        pcp_icp_planes* planes = nullptr;
        ~Handles() {
            if (planes) pcp_icp_planes_destroy(planes);
            if (icp) pcp_icp_destroy(icp);
            if (ix64) pcp_index_destroy(ix64);
            if (ix) pcp_index_destroy(ix);
        }
    } h;
    hipLaunchKernelGGL(k_centre_f32, dim3(grid_for(ns, kB)), dim3(kB), 0, ctx->stream, (const P48*)src, ns, c[0], c[1],
                       c[2], fs);
    hipLaunchKernelGGL(k_centre_f32, dim3(grid_for(nt, kB)), dim3(kB), 0, ctx->stream, (const P48*)tmp, nt, c[0], c[1],
                       c[2], ft);
    PCP_TRY(pcp_index_build_f32(ctx, fs, 3 * sizeof(float), ns, cell_size, &h.ix));
    PCP_TRY(pcp_icp_create(ctx, h.ix, ft, 3 * sizeof(float), nt, &h.icp));
    // normals over the caller's fp64 points (translation-invariant, so not the centred copy); the
    // index drops the same non-finite points as the fp32 one and keeps the caller indices
    PCP_TRY(pcp_index_build_f64(ctx, (const double*)src, PCP_AOS48_STRIDE, ns, nullptr, 0, 0.0, &h.ix64));
    PCP_TRY(bufs.get(&nrm, (size_t)ns));
    PCP_TRY(pcp_normals_knn(ctx, h.ix64, normals_k, nrm, ns));
    pcp_index_destroy(h.ix64);
    h.ix64 = nullptr;
    PCP_TRY(pcp_icp_planes_create(ctx, fs, 3 * sizeof(float), (const float*)nrm, sizeof(pcp_plane), ns, &h.planes));
    bufs.free(nrm);
    double T[24] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0};
    PCP_HIP(ctx, hipMemcpyAsync(pose, T, npose * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (trim && by_plane)
        PCP_TRY(pcp_icp_run_plane_rtrimmed_dev(ctx, h.icp, h.planes, ft, 3 * sizeof(float), nt, pose, rmax, trim[0],
                                               trim[1], trim[2], iters, pose + 16, (uint64_t*)(pose + 20)));
    else if (trim)
        PCP_TRY(pcp_icp_run_plane_trimmed_dev(ctx, h.icp, h.planes, ft, 3 * sizeof(float), nt, pose, rmax, trim[0],
                                              trim[1], trim[2], iters, pose + 16, (uint64_t*)(pose + 20)));
    else
        PCP_TRY(pcp_icp_run_plane_dev(ctx, h.icp, h.planes, ft, 3 * sizeof(float), nt, pose, rmax, iters, pose + 16));
    PCP_HIP(ctx, hipMemcpyAsync(T, pose, npose * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(M, T, 16 * sizeof(double));
    for (int r = 0; r < 3; r++) {  // t' = (t - R c) + c, as pcp_get_rot_icp
        double rcv = M[4 * r] * c[0];
        rcv = rcv + M[4 * r + 1] * c[1];
        rcv = rcv + M[4 * r + 2] * c[2];
        M[4 * r + 3] = (M[4 * r + 3] - rcv) + c[r];
    }
    // stats: a failed solve (or no solved iteration) reports err = -1, as pcp_get_rot_icp does
    if (err) *err = (T[16] < 0 || T[19] < 1.0) ? -1.0f : (float)T[17];
    if (trim && kept_out) {
        uint64_t st[PCP_ICP_TRIM_STATS];
        std::memcpy(st, T + 20, sizeof(st));
        *kept_out = (int64_t)st[1];
    }
    return PCP_OK;
}

int pcp_get_rot_icp_plane(pcp_ctx* ctx, const void* src, int64_t ns, int src_dense, const void* tmp, int64_t nt,
                          int tmp_dense, double M[16], float rmax, int iters, int normals_k, double cell_size,
                          float* err) {
    return get_rot_plane(ctx, "pcp_get_rot_icp_plane", src, ns, src_dense, tmp, nt, tmp_dense, M, rmax, nullptr, false,
                         iters, normals_k, cell_size, err, nullptr);
}

int pcp_get_rot_icp_plane_trimmed(pcp_ctx* ctx, const void* src, int64_t ns, int src_dense, const void* tmp, int64_t nt,
                                  int tmp_dense, double M[16], float rmax, float frac, float mult, float d_floor,
                                  int iters, int normals_k, double cell_size, float* err, int64_t* kept_out) {
    const float trim[3] = {frac, mult, d_floor};
    return get_rot_plane(ctx, "pcp_get_rot_icp_plane_trimmed", src, ns, src_dense, tmp, nt, tmp_dense, M, rmax, trim,
                         false, iters, normals_k, cell_size, err, kept_out);
}

int pcp_get_rot_icp_plane_rtrimmed(pcp_ctx* ctx, const void* src, int64_t ns, int src_dense, const void* tmp, int64_t nt,
                                   int tmp_dense, double M[16], float rmax, float frac, float mult, float d_floor,
                                   int iters, int normals_k, double cell_size, float* err, int64_t* kept_out) {
    const float trim[3] = {frac, mult, d_floor};
    return get_rot_plane(ctx, "pcp_get_rot_icp_plane_rtrimmed", src, ns, src_dense, tmp, nt, tmp_dense, M, rmax, trim,
                         true, iters, normals_k, cell_size, err, kept_out);
}

}  // extern "C"
