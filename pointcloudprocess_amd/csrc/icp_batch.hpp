// What icp_batch.hip, icp_batch_trim.hip and icp_batch_p2p.hip share of a batch handle
// (include/pcp.h, I5 / I5b / I5c): the handle with its padded chunk layout, the chunk grid, and the
// launches an iteration is put together from -- the search and the plane pair (icp_batch.hip), the
// per-segment trim (icp_batch_trim.hip), the point-to-point pair (icp_batch_p2p.hip).
#pragma once
#include "icp_pair.hpp"

// Segments are padded to whole 64-query chunks of the sorted layout: segment s owns the chunks
// [seg_chunk[s], seg_chunk[s + 1]), that is the slots [64 seg_chunk[s], 64 seg_chunk[s + 1]).
struct pcp_icp_batch {
    pcp_ctx* owner = nullptr;         // the creating context: owns the buffers (a lifetime reference)
    const pcp_index* target = nullptr;  // borrowed
    int64_t nq = 0;                   // queries passed to pcp_icp_batch_create
    int nseg = 0;
    int64_t nch = 0;                  // 64-query chunks of the padded sorted layout
    float4* rec = nullptr;            // 64 * nch: {x, y, z, bits(original index)}; a pad slot has index -1
    int32_t* chunk_seg = nullptr;     // nch: the segment of a chunk
    int32_t* seg_chunk = nullptr;     // nseg + 1: the first chunk of a segment
};

namespace pcp {

constexpr int kBB = 256;          // 4 waves = 4 chunks per block of the wave-per-chunk kernels
constexpr int kBW = kBB / 64;

inline unsigned chunk_grid(int64_t nch) { return (unsigned)((nch + kBW - 1) / kBW); }

// one launch each on ctx's stream, no check of the launch; the first two need nch > 0
void batch_launch_search(pcp_ctx* ctx, const pcp_icp_batch* b, const double* T_dev, float rmax, uint64_t* keys);
void batch_launch_acc(pcp_ctx* ctx, const pcp_icp_batch* b, const double* T_dev, const uint64_t* keys,
                      const pcp_icp_planes* pl, double* part /* nch x 30 */);
// per segment: the sum of its chunks' partials -> row s of acc_out when given, then solve_apply on
// T + 16 s, stats + 4 s when T is given
void batch_launch_sum_solve(pcp_ctx* ctx, const pcp_icp_batch* b, const double* part, double* acc_out, double* T,
                            double* stats);

// the per-segment trim of I5b on ctx's stream, three launches (icp_batch_trim.hip): skeys is 64 * nch
// keys of the caller's guard memory; planes == nullptr ranks the keys' own high words and reads no
// pose; out == keys trims in place
void launch_trim(pcp_ctx* ctx, const pcp_icp_batch* b, const double* T_dev, const uint64_t* keys,
                 const pcp_icp_planes* planes, float frac, float mult, float d_floor, uint64_t* out, uint64_t* trim,
                 uint64_t* skeys);

// the point-to-point pair of launches (icp_batch_p2p.hip, I5c), as the plane pair above: the chunks'
// 24 Kabsch partials from the caller's target cloud (t_stride_f floats apart, n_target points; needs
// nch > 0), then per segment their sum -> row s of acc_out when given and the Kabsch step on
// T + 16 s, stats + 4 s when T is given
void batch_launch_acc_kabsch(pcp_ctx* ctx, const pcp_icp_batch* b, const double* T_dev, const uint64_t* keys,
                             const float* target_xyz, size_t t_stride_f, int64_t n_target,
                             double* part /* nch x 24 */);
void batch_launch_sum_solve_kabsch(pcp_ctx* ctx, const pcp_icp_batch* b, const double* part, double* acc_out,
                                   int do_scale, double* T, double* stats);

}  // namespace pcp
