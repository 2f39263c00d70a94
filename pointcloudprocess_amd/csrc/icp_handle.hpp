// The ICP handle and what the files built on it share (icp.hip, icp_create.hip, icp_shard.hip):
// the handle, the sorted-query record, the kernels' argument block, the pose block's layout and the
// sizes that both the kernels' launch bounds and the handle's grids are computed from.  Internal.
#pragma once
#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

#include "icp_pair.hpp"

namespace pcp {
// a sorted query's coordinates: 12 bytes (one global_load_dwordx3 per lane)
struct QXyz {
    float x, y, z;
};

// The pose block of a handle (pcp_icp::pose_dev): one device block of 32-bit words that k_pose_set
// (and k_pilot_map) write before a launch's kernels, which read the pose, the launch index and the
// look-ahead map from it; the host getters read beta, off and pilot_pairs.  A pose is 12 floats: R
// row-major, then t.
struct PoseBlock {
    float cur[12];      // this launch's pose
    float prev[12];     // the previous launch's
    uint32_t launch;    // this launch's index (mod 2^32): read on the device, so a captured graph replays
    float step;         // the size of the step prev -> cur (step_size)
    float beta;         // the look-ahead factor of this launch, 0 = none
    float off;          // beta * step: the largest offset of a search centre (m)
    float c[12];        // the look-ahead map T_c: where the searches centre (= cur when beta = 0)
    float pilot_pairs;  // the pilot's pair count, -1 = no pilot ran
};
constexpr int kPoseWords = sizeof(PoseBlock) / 4;
// the names replace word offsets that were written as numbers: the byte layout stays what it was
static_assert(offsetof(PoseBlock, cur) == 0 && offsetof(PoseBlock, prev) == 4 * 12 &&
              offsetof(PoseBlock, launch) == 4 * 24 && offsetof(PoseBlock, step) == 4 * 25 &&
              offsetof(PoseBlock, beta) == 4 * 26 && offsetof(PoseBlock, off) == 4 * 27 &&
              offsetof(PoseBlock, c) == 4 * 28 && offsetof(PoseBlock, pilot_pairs) == 4 * 40 && kPoseWords == 41,
              "pose block layout");
}  // namespace pcp

struct pcp_icp {
    explicit pcp_icp(pcp_ctx* c) : ctx(c), owner(c), mem(c) {}
    pcp_ctx* ctx;                 // the context of the last call (launches go to its stream): NOT retained
    pcp_ctx* owner;               // the creating context: a lifetime reference
    pcp::Tmp mem;                 // every device block and event below, held on `owner`: pcp_icp_destroy
                                  // gives back what it holds, so nothing here is freed by name
    const pcp_index* target = nullptr;
    int64_t nq = 0;               // finite queries
    int64_t nq_in = 0;            // queries passed to pcp_icp_create
    pcp::QXyz* q = nullptr;       // sorted queries, 12-byte xyz (the verify stream reads 12 B, not 16)
    int32_t* qidx = nullptr;      // their original indices (read only for caller-order outputs)
    uint32_t* cand = nullptr;     // per sorted query: its cache record (cache_load / cache_store): the
                                  // sorted-target positions of its 3 nearest targets at its last search
                                  // (the winner is always among them), the launch slot s of that search
                                  // and D, a lower bound on the distance from the query, at that launch's
                                  // pose, to every target NOT cached.  12 bytes when the target has fewer
                                  // than 2^26 - 2 points (narrow), else 16
    bool narrow = false;
    float* pose_hist = nullptr;   // 256 x 12 floats: the pose of launch t at slot t & hist_mask
    int64_t launches = 0;         // correspondence launches so far (the first has nothing to verify)
    bool last_verified = false;   // the last launch ran the verify pass
    int32_t* sv = nullptr;        // verify pass: per-wave segments of uncertified queries (sv_seg each)
    uint32_t* sv_count = nullptr;
    uint32_t* sv_off = nullptr;   // [nseg_v]: the search list's length (k_list_compact)
    int32_t* svc = nullptr;       // compacted search list
    int64_t sv_seg = 0;
    int64_t nseg_v = 0;           // verify list segments: one per wave, or one per chunk (XCD split)
    int nb_ver = 0;
    int32_t* fb = nullptr;        // fallback lists: one segment of fb_seg entries per octant WG
    uint32_t* fb_count = nullptr; // per octant wave: entries in its segment
    uint32_t* fb_off = nullptr;   // [nseg]: the fallback list's length (k_list_compact)
    int32_t* fbc = nullptr;       // compacted fallback list
    int64_t fb_seg = 0;
    double* partials = nullptr;   // (nb_ver + nb_fast + nb_ring) * 24
    double* acc = nullptr;        // 24 (scratch for pcp_icp_run)
    int nb_fast = 0, nb_ring = 0;
    int nb_fast_l = 0;            // octant grid of the list launches (<= nb_fast)
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_mid = nullptr, ev_ver = nullptr;
    pcp::PoseBlock* pose_dev = nullptr;  // this launch's pose, the previous one, the look-ahead state
    std::vector<std::pair<hipEvent_t, hipEvent_t>> tev;  // per-launch timing events (device loop)
    size_t ntev = 0;              // pairs recorded since the last pcp_icp_kernel_ms
    int dbg = 0;                  // ablation flags (pcp_icp_set_options; profiling only: results are wrong)
    int oct_g_first = 1;          // lanes per query of the octant pass: first launch (all queries)
    int oct_g_list = 0;           // ... and the verify pass's search lists (0: by the list's density)
    int ring_g = 0;               // lanes per query of the fallback pass, 0 = by the list's length
    double last_ms = 0.0;
    int last_launches = 0;
    uint32_t last_fallback = 0;
    uint32_t last_searched = 0;   // queries the verify pass could not certify (searched)
    hipGraphExec_t gexec = nullptr;  // the verify .. fallback section of a device-pose launch (icp_launch)
    float graph_r2 = 0.f;            // the rmax^2 it was captured with
    bool graph_off = false;          // capture failed: plain launches
    bool graph = false;              // PCP_ICP_OPT_GRAPH
    bool no_look = false;            // PCP_ICP_OPT_NO_LOOKAHEAD: beta = 0, the plain search kernels
    bool no_pilot = false;           // PCP_ICP_OPT_NO_PILOT: no pilot step before the first launch
    bool pilot_always = false;       // PCP_ICP_OPT_PILOT_ALWAYS: the pilot below kPilotMinQueries too
    bool has_pred = false;           // pcp_icp_predict_first: pred replaces the pilot's estimate
    double pred[16] = {};            // the caller's predicted second pose
    double* pilot_acc = nullptr;     // 24: the pilot's reduced accumulators
};

namespace pcp {

constexpr int kIcpBlock = 256;
#ifndef PCP_OCT_WAVES_LIST  // the octant pass over the verify pass's lists: more registers, fewer waves
#define PCP_OCT_WAVES_LIST 4
#endif
#ifndef PCP_OCT_WAVES
#define PCP_OCT_WAVES 6
#endif
#ifndef PCP_VER_WAVES   // verify (per-lane accumulators: ~100 VGPRs)
#define PCP_VER_WAVES 4
#endif

#ifndef PCP_RING_WAVES
#define PCP_RING_WAVES 6
#endif

struct IcpArgs {
    GridDesc g;
    const float4* tp;   // sorted target points
    const QXyz* q;      // sorted queries (xyz)
    const int32_t* qidx;  // their original indices
    int64_t nq;
    float R[9], t[3];   // this launch's pose: not set by the host, load_pose reads it from `pose`
    float Rc[9], tc[3]; // the look-ahead map T_c of this launch (k_pose_set): where the searches centre
    float r2;
    float cert2;        // certified radius^2 of the 2x2x2 octant search
    float rho;          // octant half-width in cell units (0.5 - margin)
    float mc;           // cell-unit margin for pruning
    double* partials;
    uint32_t* cand;     // cache records (cache_load / cache_store)
    int narrow;         // 12-byte records
    uint32_t hist_mask; // pose history slot of a launch: launch & hist_mask (63 narrow, 255 wide)
    uint32_t max_age;   // older caches are searched again (so their slot is never reused)
    float dunit, inv_dunit;  // narrow D code unit (cell size / 1024)
    const float* pose_hist;
    uint32_t launch;    // this launch's index (mod 2^32): load_pose's too
    uint32_t ntp;       // target points (tp[ntp] is the far sentinel)
    int32_t* sv;        // verify pass output segments (sv_seg entries per wave)
    uint32_t* sv_count;
    uint32_t* sv_off;
    int64_t sv_seg;
    int64_t nseg_v;     // verify-pass waves
    int32_t* fb;
    uint32_t* fb_count;
    uint32_t* fb_off;   // [nseg]: the compacted fallback list's length
    int64_t fb_seg;
    int nb_fast;
    int64_t nseg;       // fallback segments (= waves of the octant kernel)
    int ring_all;       // ring kernel: process every query (sparse grid) instead of the list
    int dbg;            // ablation flags (pcp_icp_set_options; profiling only)
    int oct_g;          // octant pass lanes per query: 1, 2, 4, 8, or 0 = by the list's density
    int ring_g;         // fallback pass lanes per query: 1, 2, 4, 8, or 0 = by the list's length
    const PoseBlock* pose;  // the handle's pose block
    int when_beta;      // first launch after a pilot: 1 = run only if the pose block's beta > 0, 2 = only
                        // if it is 0 (the look-ahead and the plain kernel are both enqueued), 0 = always
    int64_t pilot_stride;  // k_icp_pilot: every pilot_stride-th 64-query chunk is sampled
};

constexpr uint32_t kPos26 = (1u << 26) - 1;
constexpr int kHist = 256;  // pose history slots allocated (narrow records use 64 of them)

// Destroy the handle's captured launch graph, if it has one, once its last replay has run
// (icp_create.hip).  The wait is for the owner's device: the stream the graph was replayed on belongs
// to the context of the last call, which the handle does not keep alive.  Leaves the owner's device
// selected.
void icp_graph_drop(pcp_icp* icp);

}  // namespace pcp
