// K6: the kd_tree_lod KdTree search (kd_tree_lod/kd_tree.cpp:29-117).
// fp32 kNN over the float vertices float(p - c) (kd_tree_lod/kd_tree.cpp:39-43, 62-68;
// the trimesh2 search is external: exact k nearest, ties by vertex index), each neighbour then
// matched back to the fp64 cloud.  One lane per query over two grid indexes built per call.
#include <algorithm>

#include "knn_search.hpp"

namespace pcp {
namespace {

template <int K>
struct LodVisitor {
    const float4* pts;
    float qx, qy, qz;
    TopK<K, float> top;
    __device__ float bound() const { return top.kth() * (1.0f + 1e-5f); }
    __device__ void visit(uint32_t s, uint32_t e) {
        for (uint32_t t = s; t < e; t++) {
            const float4 p = pts[t];
            const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
            float d = dx * dx;
            d = d + dy * dy;
            d = d + dz * dz;
            top.push(d, __float_as_int(p.w));
        }
    }
};

// first original j with point_dis2(k_point, cloud[j]) <= FLT_EPSILON (kd_tree.cpp:91-105)
struct MatchVisitor {
    const double4* pts;
    const int32_t* mapping;
    int identity;
    double kx, ky, kz;
    int best;
    double bestd;
    __device__ double bound() const { return (double)FLT_EPSILON * (1.0 + 1e-9); }
    __device__ void visit(uint32_t s, uint32_t e) {
        for (uint32_t t = s; t < e; t++) {
            const double4 p = pts[t];
            const double dx = kx - p.x, dy = ky - p.y, dz = kz - p.z;
            double d = dx * dx + dy * dy;  // pow(.,2) + pow(.,2) + pow(.,2)
            d = d + dz * dz;
            if (d <= (double)FLT_EPSILON) {
                const int jo = identity ? (int)p.w : mapping[(int)p.w];
                if (jo < best) { best = jo; bestd = d; }
            }
        }
    }
};

template <int K>
__global__ __launch_bounds__(kB) void k_lod(GridDesc gf, const float4* fpts, GridDesc gd, const double4* dpts,
                                            const int32_t* dmap, int didentity, const char* cloud, int64_t n,
                                            const char* q, int64_t nq, int k, int kk, float mcf, double mcd,
                                            int ci0, int ci1, int ci2, int32_t* oidx, double* od2) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nq; i += (int64_t)gridDim.x * blockDim.x) {
        const double* qp = (const double*)(q + i * PCP_AOS48_STRIDE);
        LodVisitor<K> v;
        v.pts = fpts;
        v.qx = (float)(qp[0] - ci0); v.qy = (float)(qp[1] - ci1); v.qz = (float)(qp[2] - ci2);
        v.top.init(kk);
        ring_search<float>(gf, v.qx, v.qy, v.qz, mcf, v);
        const double* last = (const double*)(cloud + (n - 1) * PCP_AOS48_STRIDE);
        v.top.for_each_ascending(kk, [&](int r, float, int jv) {
            int index = -1;
            double d2 = INFINITY;
            if (jv != INT_MAX) {
                const double* vp = (const double*)(cloud + (int64_t)jv * PCP_AOS48_STRIDE);
                // vertex float(p - c), neighbour rebuilt as double(float + float(c)) (:71-73)
                const float fx = (float)(vp[0] - ci0), fy = (float)(vp[1] - ci1), fz = (float)(vp[2] - ci2);
                MatchVisitor m{dpts, dmap, didentity, (double)(float)(fx + (float)ci0),
                               (double)(float)(fy + (float)ci1), (double)(float)(fz + (float)ci2), INT_MAX, 0.0};
                ring_search<double>(gd, m.kx, m.ky, m.kz, mcd, m);
                if (m.best != INT_MAX) {
                    index = m.best;
                    d2 = m.bestd;
                } else {  // no match: k_dis2 = residual to the last scanned point (:100)
                    const double dx = m.kx - last[0], dy = m.ky - last[1], dz = m.kz - last[2];
                    double dd = dx * dx + dy * dy;
                    d2 = dd + dz * dz;
                }
            }
            oidx[i * k + r] = index;
            od2[i * k + r] = d2;
        });
        for (int r = kk; r < k; r++) {
            oidx[i * k + r] = -1;
            od2[i * k + r] = INFINITY;
        }
    }
}

__global__ void k_lod_vertices(const char* cloud, int64_t n, int ci0, int ci1, int ci2, float* v) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double* p = (const double*)(cloud + i * PCP_AOS48_STRIDE);
        v[3 * i + 0] = (float)(p[0] - ci0);
        v[3 * i + 1] = (float)(p[1] - ci1);
        v[3 * i + 2] = (float)(p[2] - ci2);
    }
}

}  // namespace
}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_knn_lod(pcp_ctx* ctx, const void* cloud, int64_t n, const void* q, int64_t nq, int k, int32_t* oidx,
                double* od2) {
    if (!ctx || n < 0 || nq < 0 || k <= 0 || (n > 0 && !cloud) || (nq > 0 && (!q || !oidx || !od2)))
        return set_error(ctx, PCP_ERR_ARG, "pcp_knn_lod: bad arguments");
    if (n == 0 || nq == 0) return PCP_OK;
    const int kk = (int)(k < n ? k : n);
    if (kk > 32) return set_error(ctx, PCP_ERR_UNSUPPORTED, "pcp_knn_lod: k=%d > 32 not supported yet", k);
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    // c = Vector3i truncation of the centroid (kd_tree_lod/kd_tree.cpp:33-37)
    double c[4];
    uint32_t cnt = 0;
    PCP_TRY(centroid_aos48_dev(ctx, cloud, n, 1, c, &cnt));
    const int ci0 = (int)c[0], ci1 = (int)c[1], ci2 = (int)c[2];
    float* v = nullptr;
    Tmp tmp(ctx);
    PCP_TRY(tmp.get(&v, 3 * (size_t)n));
    hipLaunchKernelGGL(k_lod_vertices, dim3(blocks_for(n)), dim3(kB), 0, ctx->stream, (const char*)cloud, n, ci0, ci1,
                       ci2, v);
    pcp_index* fi = nullptr;
    pcp_index* di = nullptr;
    int rc = pcp_index_build_f32(ctx, v, 3 * sizeof(float), n, 0.0, &fi);
    if (rc == PCP_OK) rc = pcp_index_build_f64(ctx, (const double*)cloud, PCP_AOS48_STRIDE, n, nullptr, 0, 0.0, &di);
    if (rc == PCP_OK) {
        const GridDesc& gf = fi->g;
        const int nmax = std::max(gf.n[0], std::max(gf.n[1], gf.n[2]));
        const float mcf = 1e-5f + 8e-7f * (float)nmax;
        with_k<32>(kk, [&](auto kc) {
            constexpr int KV = decltype(kc)::value;
            hipLaunchKernelGGL(k_lod<KV>, dim3(blocks_for(nq)), dim3(kB), 0, ctx->stream, fi->g,
                               (const float4*)fi->pts, di->g, (const double4*)di->pts, di->mapping, di->identity,
                               (const char*)cloud, n, (const char*)q, nq, k, kk, mcf, cell_margin64(di->g), ci0, ci1,
                               ci2, oidx, od2);
        });
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = hip_fail(ctx, e, "k_lod", __FILE__, __LINE__);
    }
    if (fi) pcp_index_destroy(fi);
    if (di) pcp_index_destroy(di);
    return rc;
}

}  // extern "C"
