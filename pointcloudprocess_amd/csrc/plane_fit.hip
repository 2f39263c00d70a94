// F1 batch: one plane per CSR segment, points xyz[idx[t]] (or xyz[t]) for t in
// [off[s], off[s+1]), accumulated sequentially in segment order (calculate_feature.cpp:
// 131-164) -- calculate_plan_parameter_h_points per segment, and the radius variant
// (calculate_feature.h:15, F4) when the segments are radiusSearch rows.  Uses no index.
#include "pca.hpp"

namespace pcp {
namespace {

constexpr int kB = 256;

__global__ __launch_bounds__(kB) void k_plane_segments(const double* xyz, size_t stride, const int64_t* off,
                                                       const int32_t* idx, int64_t nseg, pcp_plane* out) {
    for (int64_t sg = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; sg < nseg;
         sg += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = off[sg], e = off[sg + 1];
        const int64_t h = e - s;
        if (h <= 0) {
            out[sg] = pcp_plane{0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
            continue;
        }
        pcp_plane pl;
        plane_from_sequence(h, [&](auto use) {
            for (int64_t t = s; t < e; t++) {
                const double* p = (const double*)((const char*)xyz + (size_t)(idx ? (int64_t)idx[t] : t) * stride);
                use(p[0], p[1], p[2]);
            }
        }, pl);
        out[sg] = pl;
    }
}

}  // namespace
}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_plane_fit_segments(pcp_ctx* ctx, const double* xyz, size_t stride, const int64_t* off, const int32_t* idx,
                           int64_t nseg, pcp_plane* out) {
    if (!ctx || nseg < 0 || (nseg > 0 && (!xyz || !off || !out)))
        return set_error(ctx, PCP_ERR_ARG, "pcp_plane_fit_segments: bad arguments");
    if (stride == 0) stride = 3 * sizeof(double);
    if (nseg == 0) return PCP_OK;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_plane_segments, dim3(grid_for(nseg, kB, 1 << 22)), dim3(kB), 0, ctx->stream, xyz, stride, off,
                       idx, nseg, out);
    PCP_LAUNCH_CHECK(ctx);
    return PCP_OK;
}

}  // extern "C"
