// What icp_batch.hip and icp_batch_trim.hip share of a batch handle (include/pcp.h, I5 / I5b): the
// handle with its padded chunk layout, the chunk grid, and the launches of the three kernels of an
// untrimmed iteration (defined in icp_batch.hip), which the trimmed loops put their trim between.
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

}  // namespace pcp
