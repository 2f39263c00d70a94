// Shared internals of libpcp (HIP, gfx950).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <unordered_map>

#include <vector>

#include "../../include/pcp.h"

struct pcp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // a non-blocking stream for work that overlaps the main stream inside one call (the query
    // sort of pcp_icp_create_with_target); created on first use, ordered by events both ways
    hipStream_t side = nullptr;
    std::string last_error;
    // grow-only scratch arena (one per context; contexts are not shared across threads)
    void* scratch = nullptr;
    size_t scratch_bytes = 0;
    uint32_t bf_fallback = 0;  // queries of the last pcp_knn_bruteforce that needed the exact scan
    // deferral counts of the last pcp_normals_knn (pcp_normals_knn_last_deferred): two device
    // words the call copies its list counters into, stream-ordered; allocated on first use.
    // nrm_mode: 0 nothing searched, 1 dense grid {tile's list, near pass's list}, 2 sparse
    // grid {near pass's list, unused}
    uint32_t* nrm_deferred = nullptr;
    int nrm_mode = 0;
    // deferred queries of the last pcp_knn (pcp_knn_last_far): one device word the call copies
    // its far list's counter into, stream-ordered; allocated on first use.  knn_far_set: false
    // when the call returned before searching
    uint32_t* knn_far = nullptr;
    bool knn_far_set = false;
    // look-back scan state (scan.hip): per-tile status words tagged with the call's epoch, so
    // no clearing pass is needed per call; [tiles] u64 status, then the tile counter and total
    uint64_t* scan_status = nullptr;
    // timing events returned by destroyed ICP handles, reused by the next (creating and
    // destroying ~44 events per registration cost ~0.3 ms of host time)
    std::vector<hipEvent_t> event_pool;
    int64_t scan_tiles = 0;
    uint32_t scan_epoch = 0;
    // Caching device allocator for the library's internal buffers (index builds, ICP state,
    // per-call scratch): blocks are reused in stream order on this context's stream instead
    // of paying a synchronising hipMalloc/hipFree each time.  Objects allocated through a
    // context must be destroyed before it.
    std::multimap<size_t, void*> free_blocks;
    std::unordered_map<void*, size_t> block_size;
    size_t cached_bytes = 0;
    // pcp_ctx_alloc_stats: bytes handed out now, their peak, hipMalloc calls of cache_alloc
    size_t out_bytes = 0, peak_bytes = 0;
    int64_t n_hipmalloc = 0;
    size_t cache_cap = (size_t)16 << 30;  // set from the device size at create (a third of HBM)
    // lifetime: every index / ICP handle / CloudGrid made on the context holds a reference, so
    // the objects may be destroyed before OR after pcp_ctx_destroy (a garbage-collected host
    // language finalises them in any order): destroy marks the context closing, frees what no
    // object uses, and the last object's destroy finishes the job
    int live = 0;
    bool closing = false;
};

namespace pcp {

int set_error(pcp_ctx* ctx, int code, const char* fmt, ...);
int hip_fail(pcp_ctx* ctx, hipError_t e, const char* what, const char* file, int line);
// scratch of at least `bytes` (invalidates earlier scratch pointers)
int scratch(pcp_ctx* ctx, size_t bytes, void** out);
// the context's side stream (created on first use)
int side_stream(pcp_ctx* ctx, hipStream_t* out);

#define PCP_HIP(ctx, expr)                                                           \
    do {                                                                             \
        hipError_t _e = (expr);                                                      \
        if (_e != hipSuccess) return ::pcp::hip_fail((ctx), _e, #expr, __FILE__, __LINE__); \
    } while (0)

#define PCP_TRY(expr)                 \
    do {                              \
        int _rc = (expr);             \
        if (_rc != PCP_OK) return _rc; \
    } while (0)

#define PCP_LAUNCH_CHECK(ctx) PCP_HIP(ctx, hipGetLastError())

// cached device allocation of `bytes` (>= 1) on ctx; dfree returns it to ctx's cache
int cache_alloc(pcp_ctx* ctx, size_t bytes, void** p);
void dfree(pcp_ctx* ctx, void* p);
void cache_release(pcp_ctx* ctx);
// object lifetime references on a context (see pcp_ctx::live)
void ctx_retain(pcp_ctx* ctx);
void ctx_release(pcp_ctx* ctx);
// a timing event from ctx's pool (or a new one); event_put returns it to the pool
hipError_t event_get(pcp_ctx* ctx, hipEvent_t* ev);
void event_put(pcp_ctx* ctx, hipEvent_t ev);

template <typename T>
int dmalloc(pcp_ctx* ctx, T** p, size_t count) {
    void* v = nullptr;
    const int rc = cache_alloc(ctx, (count ? count : 1) * sizeof(T), &v);
    *p = (T*)v;
    return rc;
}

// One owner for device blocks and timing events: the temporaries of one call, or everything an ICP
// handle keeps (icp_handle.hpp).  get() takes a block from ctx's cache, event() an event from its
// pool, and the destructor gives back whatever is still held, so no return path leaks.  The cache
// serves later requests of the same call from freed blocks: a temporary that is dead before a later
// allocation is returned there with free(), not left to scope exit, or the call's peak footprint
// grows.
struct Tmp {
    pcp_ctx* ctx;
    std::vector<void*> held;
    std::vector<hipEvent_t> events;
    explicit Tmp(pcp_ctx* c) : ctx(c) {}
    Tmp(const Tmp&) = delete;
    Tmp& operator=(const Tmp&) = delete;
    ~Tmp() { free_all(); }
    template <typename T>
    int get(T** p, size_t count) {
        PCP_TRY(dmalloc(ctx, p, count));
        held.push_back((void*)*p);
        return PCP_OK;
    }
    hipError_t event(hipEvent_t* ev) {
        const hipError_t e = event_get(ctx, ev);
        if (e == hipSuccess) events.push_back(*ev);
        return e;
    }
    // take over a block of ctx's cache that another guard released
    template <typename T>
    T* adopt(T* p) {
        held.push_back((void*)p);
        return p;
    }
    // hand a block over to a longer-lived owner: the guard no longer frees it
    template <typename T>
    T* release(T* p) {
        for (void*& q : held)
            if (q == (void*)p) q = nullptr;
        return p;
    }
    // early free: the block goes back to the cache now and p is cleared
    template <typename T>
    void free(T*& p) {
        dfree(ctx, release(p));
        p = nullptr;
    }
    void free_all() {
        for (void* p : held) dfree(ctx, p);
        held.clear();
        for (hipEvent_t ev : events) event_put(ctx, ev);
        events.clear();
    }
};

inline unsigned grid_for(int64_t n, int block, int64_t cap = 1 << 20) {
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

// a caller's byte stride between xyz triples: 0 means packed; whole floats, at least 3
inline int check_stride(pcp_ctx* ctx, size_t* stride) {
    if (*stride == 0) *stride = 3 * sizeof(float);
    if (*stride % sizeof(float) || *stride < 3 * sizeof(float))
        return set_error(ctx, PCP_ERR_ARG, "strides must be whole floats, at least 3");
    return PCP_OK;
}

// ---------------------------------------------------------------- device helpers
__device__ __forceinline__ bool finite3(double x, double y, double z) {
    return isfinite(x) && isfinite(y) && isfinite(z);
}

// compute3DCentroid's sequential fp64 fold of x/y/z over the AoS48 records seg0 ++ seg1, bit-exact
// (fold.hip); s_host[3] = number of points summed (finite ones when !is_dense).
int seqfold_aos48(pcp_ctx* ctx, const void* p0, int64_t n0, const void* p1, int64_t n1, int is_dense,
                  double s_host[4]);
// compute3DCentroid over n AoS48 records (cloud.hip): c = the centroid, *count = the points
// summed; n <= 0 leaves c untouched.  Syncs.
int centroid_aos48_dev(pcp_ctx* ctx, const void* in, int64_t n, int is_dense, double c[4], uint32_t* count);

// What code that does not include icp_handle.hpp may know of an ICP handle (icp_create.hip): its
// target index and the number of queries passed to pcp_icp_create (the length of a pcp_icp_keys_dev
// buffer).
const pcp_index* icp_target(const pcp_icp* icp);
int64_t icp_query_count(const pcp_icp* icp);

// pcp_icp_trim_keys (icp_trim.hip) for callers that have checked the arguments (trim_args_ok and
// the pointers) and own the work memory (trim_work_bytes, reusable from call to call).
size_t trim_work_bytes();
bool trim_args_ok(float frac, float mult, float d_floor);
int trim_keys_async(pcp_ctx* ctx, const uint64_t* keys, int64_t n, float frac, float mult, float d_floor,
                    uint64_t* out, uint64_t* trim, uint32_t* work);
// its selection alone: trim = {m, 0, sel, bits of cut}; a filter of the caller's adds the kept keys
// to trim[1] (n == 0: the complete stats)
int trim_select_async(pcp_ctx* ctx, const uint64_t* keys, int64_t n, float frac, float mult, float d_floor,
                      uint64_t* trim, uint32_t* work);
// the filter after it: out[i] = keys[i] where the key ranked for pair i passes trim's cut, else "no
// pair"; the ranked key is rkeys[i], or keys[i] itself when rkeys is null.  out may be keys.
int trim_filter_async(pcp_ctx* ctx, const uint64_t* keys, const uint64_t* rkeys, int64_t n, uint64_t* out,
                      uint64_t* trim);

// Exclusive scan of `n` uint32 values in place (values' total must fit uint32).
// Returns the total through *total_dev (device, optional) and *total_host (optional, syncs).
int scan_u32_inplace(pcp_ctx* ctx, uint32_t* data, int64_t n, uint32_t* total_host);
// Exclusive scan of int32 counts into int64 offsets (n+1 entries).
int scan_i32_to_i64(pcp_ctx* ctx, const int32_t* in, int64_t n, int64_t* out, int64_t* total_host);

// ---------------------------------------------------------------- grid description
// Uniform grid of cubic cells.  Dense mode (the MI355X default whenever the table fits the
// HBM budget): cstart has one entry per cell of the bounding grid, linear id
// (z*ny + y)*nx + x, so a row of cells along x is one contiguous point range.  Sparse
// mode (huge sparse bounding boxes): 4x4x4 bricks, a dense brick table maps a brick to a
// slot (or -1) and each slot owns 64 consecutive cstart entries.
struct GridDesc {
    double o[3];      // origin (bbox min)
    double h, inv_h;  // cell size
    float of[3];
    float hf, inv_hf;
    int n[3];         // cells per axis
    int nb[3];        // bricks per axis
    int64_t nbricks;
    int64_t nslots;
    int dense;                // 1: cstart is indexed by the linear cell id (x fastest)
    int64_t ncells;           // dense: n[0]*n[1]*n[2]
    const int32_t* brick;     // nbricks (sparse mode only)
    const uint32_t* cstart;   // dense: ncells + 1 ; sparse: 64*nslots + 1
};


}  // namespace pcp

struct pcp_index {
    int is_f64 = 0;
    pcp::GridDesc g{};
    int64_t n_in = 0;        // size of the cloud passed in (n, or n_indices)
    int64_t n = 0;           // valid points (total_nr_points_)
    int identity = 0;
    int32_t* brick = nullptr;
    uint32_t* cstart = nullptr;
    void* pts = nullptr;        // float4[n] or double4[n], sorted by (slot, local cell)
    int32_t* mapping = nullptr; // internal j -> caller index (n)
    int32_t* sorted_j = nullptr; // sorted position -> internal j (n)
    int32_t* pos_of_j = nullptr; // internal j -> sorted position (n, fp64 index only)
    // fp16 cell-relative index (C5, h16.hip): per sorted point its offset from its cell's
    // origin as 3 x fp16 (+ 16-bit pad) and its dense cell id; pts is released after the build
    int is_h16 = 0;
    uint2* h16 = nullptr;
    uint32_t* cell = nullptr;
    pcp_ctx* owner = nullptr;
};
