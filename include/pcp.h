/*
 * pcp.h -- C-ABI of libpcp, the MI355X (gfx950) implementation of the kNN-driven geometry
 * hot path of RioWong/PointCloudProcess.
 *
 * Plain C: opaque handles, plain pointers and sizes, int status codes (0 = OK, < 0 =
 * error; pcp_last_error(ctx) has the message).  No torch / HIP types in any signature:
 * streams are passed as `void*` (a hipStream_t, NULL = the device's default stream).
 *
 * Memory: every array argument named *_dev is DEVICE memory (hipMalloc'd, or a torch
 * tensor's data_ptr()); host arrays are named *_host.  pcp_malloc/pcp_memcpy_* let a host
 * caller (include/pcp_pcl.hpp, the drop-in C++ shim) stage data without including HIP.
 *
 * Each entry point names the reference interface it replaces (file:line in the reference
 * tree).  The C++ shim that restores the reference's own class signatures on top of this
 * ABI is include/pcp_pcl.hpp; bindings for other hosts are in INTEGRATION.md.
 */
#ifndef PCP_H
#define PCP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCP_ABI_VERSION 1

/* ----------------------------------------------------------------------- status codes */
enum pcp_status {
    PCP_OK = 0,
    PCP_ERR_ARG = -1,         /* bad argument (null handle, negative size, k <= 0, ...) */
    PCP_ERR_HIP = -2,         /* a HIP runtime call failed */
    PCP_ERR_NOMEM = -3,       /* device allocation failed */
    PCP_ERR_EMPTY = -4,       /* empty input where the reference would crash / return */
    PCP_ERR_UNSUPPORTED = -5, /* option not implemented (e.g. do_affine) */
    PCP_ERR_ICP = -6,         /* ICP failed: < 3 correspondences (ICP.h:26-28 err < 0) */
    PCP_ERR_CAPACITY = -7     /* caller-provided output buffer too small */
};

/* ----------------------------------------------------------------------- point layout */
/* PointXYZRGBA (point_type.h:9-82): 48-byte stride, x/y/z doubles at 0/8/16, data[3] at
 * 24, rgba u32 at 32, stamp_id u32 at 36, 8 pad bytes. */
#define PCP_AOS48_STRIDE 48

/* PlanSegment subset written by the normals kernel (data_struct.h:188-198). */
typedef struct pcp_plane {
    float normal_x, normal_y, normal_z;
    float min_value;  /* lambda3, calculate_feature.cpp:198 */
    float curvature;  /* lambda3/(l1+l2+l3), calculate_feature.cpp:199 */
    float distance;   /* -(n . mean), calculate_feature.cpp:197 */
} pcp_plane;

/* LAS_POINT_PROPERTY (data_struct.h:161-172): the per-point record of
 * calculate_plan_parameter_rpca; 48 bytes, the reference's layout. */
typedef struct pcp_point_property {
    float normal_x, normal_y, normal_z;
    double distance;
    double curvature;
    int32_t point_id, segment_id;
    float dis_from_point_plane;
} pcp_point_property;

/* ----------------------------------------------------------------------- context */
typedef struct pcp_ctx pcp_ctx;     /* device, stream, scratch arena, last error */
typedef struct pcp_index pcp_index; /* device-resident uniform-grid index over a cloud */
typedef struct pcp_icp pcp_icp;     /* device-resident ICP query set */

int         pcp_abi_version(void);
int         pcp_ctx_create(int device, void* stream, pcp_ctx** out);
int         pcp_ctx_destroy(pcp_ctx* ctx);
int         pcp_ctx_set_stream(pcp_ctx* ctx, void* stream);
void*       pcp_ctx_stream(pcp_ctx* ctx);
const char* pcp_last_error(const pcp_ctx* ctx);
int         pcp_sync(pcp_ctx* ctx);
/* Diagnostics: the context's internal device allocator (index builds, ICP state, per-call
 * temporaries; not pcp_malloc).  out[0] = blocks currently handed out, out[1] = their bytes,
 * out[2] = the peak of out[1] since pcp_ctx_create, out[3] = hipMalloc calls made so far.  A call
 * that returns, with or without an error, leaves out[0] where it was plus what the handles it
 * created own.  No reference counterpart. */
int         pcp_ctx_alloc_stats(const pcp_ctx* ctx, int64_t out[4]);
/* Diagnostics: on SIGSEGV/SIGBUS/SIGILL/SIGFPE/SIGABRT print the faulting library (dladdr) and
 * native frames to stderr, then chain to the previously installed handler (no reference
 * counterpart; the reference process has no fault reporting). */
int         pcp_fault_report_install(void);
/* Build provenance: SHA-1 of the sources libpcp.so was built from (csrc sources and headers,
 * include/pcp.h, the Makefile, in sorted name order); tests compare it with the tree. */
const char* pcp_build_id(void);

int pcp_malloc(pcp_ctx* ctx, void** dev_ptr, size_t bytes);
int pcp_free(pcp_ctx* ctx, void* dev_ptr);
int pcp_memcpy_h2d(pcp_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int pcp_memcpy_d2h(pcp_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int pcp_memset(pcp_ctx* ctx, void* dst_dev, int value, size_t bytes);

/* ----------------------------------------------------------------------- K: spatial index */
/* Replaces KdTreeFLANN<PointT>::setInputCloud (kd_tree.h:772-798) + convertCloudToArray
 * (kd_tree.h:928-997): drops non-finite points, keeps index_mapping_, identity when no
 * drop and no `indices`.  xyz_dev: doubles with `stride_bytes` between points (48 for
 * AoS48, 24 for packed xyz).  indices_dev: optional subset (NULL = whole cloud).
 * cell_size <= 0 picks a size from the data.  The index owns a device copy of the points. */
int pcp_index_build_f64(pcp_ctx* ctx, const double* xyz_dev, size_t stride_bytes, int64_t n,
                        const int32_t* indices_dev, int64_t n_indices, double cell_size,
                        pcp_index** out);
/* fp32 variant (trimesh2 float vertices, point_cloud_helper.cpp:89-104, the ICP target). */
int pcp_index_build_f32(pcp_ctx* ctx, const float* xyz_dev, size_t stride_bytes, int64_t n,
                        double cell_size, pcp_index** out);
int pcp_index_destroy(pcp_index* index);
int64_t pcp_index_size(const pcp_index* index);          /* total_nr_points_ */
int pcp_index_identity_mapping(const pcp_index* index);  /* identity_mapping_ */
double pcp_index_cell_size(const pcp_index* index);
int64_t pcp_index_cells(const pcp_index* index);         /* allocated cell slots */
/* Spatially sorted copy of the indexed points: fp32 index -> float4 {x,y,z,bits(idx)};
 * fp64 index -> double4 {x,y,z,(double)internal j}. Borrowed device pointer. */
const void* pcp_index_sorted_points(const pcp_index* index);

/* Batch KdTreeFLANN::nearestKSearch (kd_tree.h:814-845), exact fp64: k clamped to the
 * index size, rows ascending by (d2, internal j), d2 = ((0+d0^2)+d1^2)+d2^2 (FLANN
 * L2_Simple<double>), indices mapped through index_mapping_.  Outputs are nq*k; entries
 * past the clamped k are -1 / +inf.  out_d2_dev may be NULL (indices only). */
int pcp_knn(pcp_ctx* ctx, const pcp_index* index, const double* q_dev, size_t q_stride_bytes,
            int64_t nq, int k, int32_t* out_idx_dev, double* out_d2_dev);
/* Queries of the last pcp_knn on this context (pcp_nearest_query's included) whose k-th
 * neighbour lay beyond the near pass's cell rings and were answered by the exact
 * wave-per-query pass (diagnostic).  No reference counterpart.  0 when the call returned
 * before searching (argument error, nq == 0, PCP_ERR_UNSUPPORTED).  pcp_knn itself stays
 * asynchronous; this call waits for the stream. */
int pcp_knn_last_far(pcp_ctx* ctx, int64_t* n);

/* C5 (BASELINE configs[4]): fp16 cell-relative index + radius search with fused normals.
 * pcp_index_build_h16 sorts the cloud (fp32 xyz) into cells of `cell_size` (1 mm <= h <= 0.5 m:
 * below 1 mm the metre offsets would reach fp16's subnormal range; PCP_ERR_UNSUPPORTED; dense table) and stores each point as fp16 offsets from its cell origin (8 B) + its cell id.
 * Queries are the indexed points whose caller index is < n_owned (the rest are a multi-GPU
 * slab's halo).  pcp_h16_radius_count: per owned point the number of points with d2 < r^2
 * (itself included), r <= cell size; pcp_scan_counts -> offsets; pcp_h16_radius_fill: the
 * rows in index order (radiusSearch with setSortedResults(false), kd_tree.h:739-753,863-903)
 * as global_id_dev[caller] (or the caller index when NULL), and optionally one F1 plane per
 * row (calculate_plan_parameter(cloud, radius), calculate_feature.h:15) from fp32 sums.
 * The hit test and the plane sums run on the matrix cores (fp32 d^2 - r^2 expansion, f16 moment
 * features in cell units with fp32 accumulation): pairs within 3e-4 m of the radius may differ from an exact
 * search (the fp16 offsets' quantisation).  n_owned must not exceed the indexed
 * cloud's size (PCP_ERR_ARG).
 * Memory: the fill takes 64 B per owned point of scratch for the plane sums (with normals),
 * released when it returns; neither call keeps state in the index between calls, so calls on
 * one index from different threads only need the context's usual serialisation. */
int pcp_index_build_h16(pcp_ctx* ctx, const float* xyz_dev, size_t stride_bytes, int64_t n,
                        double cell_size, pcp_index** out);
int pcp_h16_radius_count(pcp_ctx* ctx, const pcp_index* index, float radius, int64_t n_owned,
                         int32_t* count_dev);
int pcp_h16_radius_fill(pcp_ctx* ctx, const pcp_index* index, float radius, int64_t n_owned,
                        const int64_t* offsets_dev, const int32_t* global_id_dev,
                        int32_t* idx_dev, pcp_plane* normals_dev);

/* Batch KdTreeFLANN::radiusSearch (kd_tree.h:863-903): d2 < radius*radius (strict),
 * sorted by (d2, internal j), truncated to max_nn (0 or > size = unlimited).
 * Two-phase CSR: pcp_radius_count writes per-query counts; the caller scans them into
 * offsets (nq+1, int64) and calls pcp_radius_fill. */
int pcp_radius_count(pcp_ctx* ctx, const pcp_index* index, const double* q_dev,
                     size_t q_stride_bytes, int64_t nq, double radius, uint32_t max_nn,
                     int32_t* out_count_dev);
int pcp_radius_fill(pcp_ctx* ctx, const pcp_index* index, const double* q_dev,
                    size_t q_stride_bytes, int64_t nq, double radius, uint32_t max_nn,
                    const int64_t* offsets_dev, int32_t* out_idx_dev, double* out_d2_dev);
/* Exclusive scan helper for the CSR offsets: offsets[0]=0 ... offsets[nq]=total. */
int pcp_scan_counts(pcp_ctx* ctx, const int32_t* count_dev, int64_t n, int64_t* offsets_dev,
                    int64_t* total_host);

/* Callers' reduction over K3 (main_blend.cpp:306-325 find_cloud_nearest_point_in_kdtree):
 * the query whose 1-NN d2 is smallest, strict '<' against init_bound (9999 there), so the
 * first query wins ties.  *best_q = -1 when no query beats init_bound. */
int pcp_nearest_query(pcp_ctx* ctx, const pcp_index* index, const double* q_dev,
                      size_t q_stride_bytes, int64_t nq, double init_bound, int64_t* best_q_host,
                      double* best_d2_host);

/* Brute-force kNN (BASELINE config 2): fp32 MFMA ranking of |p|^2 - 2 q.p over LDS tiles,
 * certified + re-ranked in fp64, falling back to an exact fp64 scan for any query whose
 * candidate set cannot be certified.  Same output contract as pcp_knn (no index). */
int pcp_knn_bruteforce(pcp_ctx* ctx, const double* target_dev, size_t t_stride_bytes,
                       int64_t nt, const double* q_dev, size_t q_stride_bytes, int64_t nq,
                       int k, int32_t* out_idx_dev, double* out_d2_dev);
/* Queries of the last pcp_knn_bruteforce on this context whose MFMA candidate set could
 * not be certified and were re-done by the exact fp64 scan (diagnostic). */
int pcp_knn_bruteforce_last_fallback(const pcp_ctx* ctx, int64_t* n);

/* kd_tree_lod KdTree::nearestKSearch (kd_tree_lod/kd_tree.cpp:78-117) over an AoS48 cloud:
 * integer-truncated centroid, float search, first j with point_dis2 <= FLT_EPSILON
 * (else -1), k_dis2 = residual of the last scanned j (reference quirk). */
int pcp_knn_lod(pcp_ctx* ctx, const void* cloud_aos48_dev, int64_t n, const void* q_aos48_dev,
                int64_t nq, int k, int32_t* out_idx_dev, double* out_d2_dev);

/* ----------------------------------------------------------------------- V: cloud ops */
/* PointCloudHelper::getMinMax3D(cloud, Vector4d&, Vector4d&) (point_cloud_helper.h:59-90). */
int pcp_minmax_aos48(pcp_ctx* ctx, const void* in_dev, int64_t n, int is_dense,
                     double min_host[4], double max_host[4]);
/* getMinMax3D of transformPointCloud(segment s, T_s) for every segment of a span of AoS48 records,
 * without the moved copies: row s of min_host / max_host (nseg x 4) is what pcp_minmax_aos48 returns
 * for pcp_transform_aos48(records [off[s], off[s + 1]), T_host + 16 s), both with is_dense -- the
 * same arithmetic ((r0 x + r1 y) + r2 z) + t in fp64, a non-finite point left alone by the transform
 * and skipped by the min/max when !is_dense, data[3] untransformed, DBL_MAX / DBL_MIN for a segment
 * without a counted point (the reference's DBL_MIN start of the max included).  Min and max are exact
 * in any order, so the rows agree bit for bit (up to the sign of a zero, which no order fixes).
 * T_host == NULL is the identity for every segment, run through the same arithmetic.  Segment rules
 * are pcp_icp_batch_create's (I5): offsets start at 0, end at n, never decrease; 0 <= nseg <= 65535;
 * empty segments are legal; PCP_ERR_ARG otherwise, and a rejected call writes nothing.  nseg == 0
 * writes nothing.  One pass over the records in two launches whatever nseg is (tiles of 2048
 * records that never straddle a segment; then one workgroup per segment over its tiles' rows), one
 * nseg x 64 byte copy back and one host synchronisation. */
int pcp_minmax_segments_aos48(pcp_ctx* ctx, const void* in_aos48_dev, int64_t n,
                              const int64_t* seg_offsets_host /* nseg + 1 */, int nseg, int is_dense,
                              const double* T_host /* nseg x 16 row-major, NULL = identity */,
                              double* min_host /* nseg x 4 */, double* max_host /* nseg x 4 */);
/* compute3DCentroid (point_cloud_helper.h:193-230): the reference's sequential left fold,
 * bit for bit, evaluated as a parallel scan of exact chunk transfer maps (fold.hip). */
int pcp_centroid_aos48(pcp_ctx* ctx, const void* in_dev, int64_t n, int is_dense,
                       double c_host[4], uint32_t* count_host);
/* compute3DCentroid of cloud_all = a ++ b (get_rot_icp, point_cloud_helper.cpp:78-83:
 * `*cloud_all += *src; *cloud_all += *temp;` then one fold; is_dense = a && b dense). */
int pcp_centroid_concat_aos48(pcp_ctx* ctx, const void* a_dev, int64_t na, const void* b_dev,
                              int64_t nb, int is_dense, double c_host[4], uint32_t* count_host);
/* transformPointCloud (point_cloud_helper.h:92-127), row-major 4x4, in == out allowed. */
int pcp_transform_aos48(pcp_ctx* ctx, const void* in_dev, void* out_dev, int64_t n,
                        int is_dense, const double T_host[16]);

/* VoxelGrid<PointXYZRGBA>::filter -> applyFilter (voxel_grid.h:811-1056) with
 * setLeafSize(l[0],l[1],l[2]) (voxel_grid.h:538-549) and setDownsampleAllData.
 * out_dev must hold n points; *n_out receives the voxel count; out_voxel_idx_dev
 * (optional) receives each output's u32 linear voxel index. */
int pcp_voxel_filter(pcp_ctx* ctx, const void* in_aos48_dev, int64_t n, int is_dense,
                     const double leaf_host[3], int downsample_all_data, void* out_aos48_dev,
                     int64_t* n_out, uint32_t* out_voxel_idx_dev);
/* PointCloudHelper::remove_duplicate(cloud, float leaf) (point_cloud_helper.cpp:42-63). */
int pcp_remove_duplicate(pcp_ctx* ctx, const void* in_aos48_dev, int64_t n, int is_dense,
                         float leaf, void* out_aos48_dev, int64_t* n_out);

/* ----------------------------------------------------------------------- F: normals */
/* Per-point PCA normals over the kNN(k) neighbourhood of every indexed point
 * (calculate_feature.cpp:233 neighbourhood + calculate_plan_parameter_h_points
 * :119-206).  Output in caller-index order (n = size of the cloud passed to the build,
 * points dropped as non-finite get {0,0,0,1}); sign: largest-|.| component positive. */
int pcp_normals_knn(pcp_ctx* ctx, const pcp_index* index, int k, pcp_plane* out_dev,
                    int64_t n_out);
/* Which search passes the last pcp_normals_knn on this context used (diagnostic).
 * *tile_deferred: queries the tile pass could not certify and handed on (-1: sparse grid,
 * no tile ran); *far_queries: queries answered by the exact wave-per-query pass.  Both 0
 * when the call returned before searching (k <= 3 after clamping, empty index, error).
 * pcp_normals_knn itself stays asynchronous; this call waits for the stream. */
int pcp_normals_knn_last_deferred(pcp_ctx* ctx, int64_t* tile_deferred, int64_t* far_queries);

/* F3: CalculateFeature::calculate_plan_parameter_rpca(cloud, radius (unused), Pr, epi)
 * (calculate_feature.cpp:208-368; the pipeline's normals entry, static.cpp:17) over the
 * caller's kNN rows knn_idx_dev (n x k int32, k <= 20, ascending d2, -1 padded: pcp_knn of
 * the cloud's own points with k = 20; N of a row is its leading run of non-negative indices,
 * nothing behind the first -1 is read).  Deterministic contract (the reference seeds rand()
 * with time(NULL)): the 3 neighbours of iteration i of point j are
 * splitmix64(seed, j, i, slot) % N; sorts are stable; min_value ties keep the earlier
 * iteration.  segment_id and dis_from_point_plane are written 0 (the reference leaves them
 * uninitialised).  Normal sign: largest-|.| component positive (OpenCV's is unpinned). */
int pcp_normals_rpca(pcp_ctx* ctx, const double* xyz_dev, size_t stride_bytes, int64_t n,
                     const int32_t* knn_idx_dev, int k, float pr, float epi, uint64_t seed,
                     pcp_point_property* out_dev);

/* One plane per CSR segment (calculate_plan_parameter_h_points, calculate_feature.cpp:
 * 119-206, per segment; with radiusSearch rows as segments this is the declared-only
 * calculate_plan_parameter(cloud, radius), calculate_feature.h:15).  Segment s covers
 * points xyz[idx[t]] (idx_dev NULL: xyz[t]) for t in [offsets[s], offsets[s+1]), summed
 * in that order; an empty segment gets {0,0,0,0,1,0}. */
int pcp_plane_fit_segments(pcp_ctx* ctx, const double* xyz_dev, size_t stride_bytes,
                           const int64_t* offsets_dev, const int32_t* idx_dev, int64_t nseg,
                           pcp_plane* out_dev);

/* Region growing over rpca planes: TreeExtration::region_growning (extraction_tree.cpp:66-272,
 * live body :177-271) as point_segment calls it (static.cpp:8-21).  index: fp64 index over the
 * n points of xyz_dev (kdtree.setInputCloud(Cloud)); props_dev: the n records of
 * pcp_normals_rpca, whose segment_id is rewritten (-1 = UNSEGMENTATION).  Kept segments, in
 * label order: segment s = seg_points_host[seg_offsets_host[s] .. seg_offsets_host[s+1]) in
 * the reference's push order, seeded by point seg_seeds_host[s] (its normal and Distance are
 * the PlanSegment's).  Buffers: seg_offsets n+1, seg_points n, seg_seeds n (host). */
int pcp_region_growing(pcp_ctx* ctx, const pcp_index* index, const double* xyz_dev, size_t stride_bytes, int64_t n,
                       pcp_point_property* props_dev, double distance_t, double cosfa_t,
                       int64_t* seg_offsets_host, int32_t* seg_points_host, int32_t* seg_seeds_host,
                       int64_t* n_seg);

/* ----------------------------------------------------------------------- I: ICP */
/* ICP correspondence/transform loop (point_cloud_helper.cpp:75-166 get_rot_icp ->
 * trimesh2 ICP(), point_cloud_closure + main_blend callers).  The target is an fp32
 * index (pcp_index_build_f32); the query set is sorted spatially once here. */
int pcp_icp_create(pcp_ctx* ctx, const pcp_index* target, const float* q_dev,
                   size_t q_stride_bytes, int64_t nq, pcp_icp** out);
/* Size limits pcp_icp_create enforces (host only, no device call): PCP_ERR_ARG for
 * nq >= 2^31 or a negative size, PCP_ERR_CAPACITY for a target of 2^28 - 1 or more valid
 * points (the search passes address the fp32 target with 32-bit byte offsets). */
int pcp_icp_check_sizes(int64_t n_target, int64_t nq);
/* pcp_index_build_f32 + pcp_icp_create in one call: the query set's sort runs on a second
 * stream while the target's cell sort runs (the two radix sorts of the create overlap).  Same
 * results and handles as the two calls; destroy both (the ICP handle first). */
int pcp_icp_create_with_target(pcp_ctx* ctx, const float* target_dev, size_t target_stride_bytes,
                               int64_t n_target, double cell_size, const float* q_dev,
                               size_t q_stride_bytes, int64_t nq, pcp_index** index_out,
                               pcp_icp** icp_out);
/* Test / profiling controls of an ICP handle (not needed by callers):
 *   oct_lanes_first: lanes per query of the octant search pass at the first launch (1, 2, 4, 8;
 *     0 = 1 lane); oct_lanes_list: the same over the later search lists (0 = by the list's density);
 *   ring_lanes: lanes per query of the fallback pass (1, 2, 4, 8; 0 = by the list's length);
 *   ablate: PCP_ICP_ABLATE_* flags that switch passes off for profiling -- results are WRONG
 *     while any is set.
 * A failed call (PCP_ERR_ARG with the reason in pcp_last_error) leaves the handle unchanged.
 * Results are identical for every lane choice. */
#define PCP_ICP_ABLATE_NO_SCAN 1
#define PCP_ICP_ABLATE_NO_ACCUM 4
#define PCP_ICP_ABLATE_NO_FALLBACK 8
#define PCP_ICP_ABLATE_NO_VERIFY 64
/* not an ablation: keep 16-byte cache records although the target fits the 12-byte form
 * (< 2^26 - 2 points); only before the handle's first launch.  Results are identical. */
#define PCP_ICP_OPT_WIDE_CACHE 128
/* not an ablation: device-pose launches from the handle's third on replay ONE captured HIP graph
 * of the verify .. fallback section instead of enqueueing its five kernels (results are identical;
 * the second launch still runs the plain search kernel, PCP_ICP_OPT_NO_LOOKAHEAD below).
 * Off by default: the device loop is host-asynchronous, so enqueueing is never what the GPU
 * waits for, and the replayed section measured 0.5 % slower per iteration. */
#define PCP_ICP_OPT_GRAPH 256
/* not an ablation: switch the look-ahead search centre off.  By default a query that has to be
 * searched again is searched around a point ahead of it on its path, c = T_c q with
 * T_c = T_t + beta (T_t - T_{t-1}), so that its cache certifies more of the coming launches
 * (DESIGN.md 5.1); beta comes from the ratio of the last two steps and is 0 at the second launch
 * and whenever the step did not shrink; the first launch's comes from the pilot step (below).
 * With this flag beta = 0 on every launch and the search kernels are the plain ones.  Results
 * are identical either way. */
#define PCP_ICP_OPT_NO_LOOKAHEAD 512
/* The pilot step.  Before the first launch of a handle over a dense grid, one Kabsch step over a
 * spatially uniform sample of the queries (every S-th 64-query chunk of the sorted queries,
 * S = max(1, chunks / 8192)) predicts the second pose T_1, and the first launch searches around
 * c = T_c q with T_c = T_0 + beta_0 (T_1 - T_0), beta_0 = min(1.5, 45 mm / largest displacement of
 * the predicted step): its caches then outlive the two largest steps of the registration.  When
 * the pilot finds fewer than 3 pairs or non-finite sums, or predicts no motion, beta_0 = 0 and the
 * first launch is the plain one.  On by default when the look-ahead is on and the handle has at
 * least 2^25 queries (below that the pilot costs more than 5 % of the first launch).  Only
 * pcp_icp_step / _step_dev / _run / _run_dev launches take it: the point-to-plane, trimmed and
 * batched loops minimise something else and run without it (unmeasured there).
 *   PCP_ICP_OPT_NO_PILOT: never run the pilot (the first launch as before, unless
 *     pcp_icp_predict_first supplied a pose).
 *   PCP_ICP_OPT_PILOT_ALWAYS: run it below the size threshold too (tests).
 * Results are identical either way. */
#define PCP_ICP_OPT_NO_PILOT 1024
#define PCP_ICP_OPT_PILOT_ALWAYS 2048
int pcp_icp_set_options(pcp_icp* icp, int oct_lanes_first, int oct_lanes_list, int ring_lanes, int ablate);
int pcp_icp_destroy(pcp_icp* icp);
/* One iteration at pose T (row-major 4x4 double, cast to fp32 for the kernel):
 * correspondences within rmax + the 24 accumulators ([23] = queries that
 * needed the exact fallback search, a diagnostic) written to acc_dev
 * (device, 24 doubles).  corr_idx_dev / corr_d2_dev (optional, nq each) receive the
 * winner per query in the ORIGINAL query order (-1 / +inf when rejected). */
int pcp_icp_step(pcp_ctx* ctx, pcp_icp* icp, const double T_host[16], float rmax,
                 double* acc_dev, int32_t* corr_idx_dev, float* corr_d2_dev);
/* Target-sharded multi-GPU mode: each rank indexes one shard of the
 * target (global indices [target_offset, target_offset + shard size)) and runs the ICP query
 * set against it.  pcp_icp_keys writes, per query in the ORIGINAL order (nq keys), the u64
 * key (fp32 bits of d2) << 32 | global target index, or INT64_MAX when no target of this
 * shard is within rmax; an element-wise MIN over ranks (all-reduce) yields the global
 * lexicographic (d2, index) winner.  pcp_icp_accumulate_keys then adds the 24 accumulators
 * of the queries whose global winner lies in this rank's shard [lo, hi) (shard_xyz_dev:
 * the shard's fp32 points in shard order); a SUM over ranks gives the full accumulators. */
int pcp_icp_keys(pcp_ctx* ctx, pcp_icp* icp, const double T_host[16], float rmax,
                 int64_t target_offset, uint64_t* keys_dev);
int pcp_icp_accumulate_keys(pcp_ctx* ctx, pcp_icp* icp, const double T_host[16],
                            const uint64_t* keys_dev, int64_t lo, int64_t hi,
                            const float* shard_xyz_dev, size_t shard_stride_bytes,
                            double* acc_dev);
/* Device-resident form of the target-sharded loop (pose T_dev: row-major 4x4 doubles in HBM),
 * in which no rank holds more of the target than its own shard:
 *   1. pcp_icp_keys_dev = pcp_icp_keys at the device pose (this rank's local winners);
 *   2. ReduceScatter(MIN) of the keys: each rank gets the global winners of its slice of the
 *      queries (original order);
 *   3. pcp_keys_owner: per key of the slice, the shard s owning its global target index
 *      (bounds_dev[s] <= index < bounds_dev[s + 1], nshards + 1 int64 entries), 255 for none;
 *      AllGather of these bytes gives every rank the owner of every query's winner;
 *   4. pcp_icp_accumulate_owned: the 24 accumulators of the queries (q_dev: ALL the queries in
 *      the original order) whose winner this rank owns (owner == rank), read from its own
 *      shard (shard_xyz_dev, global indices [lo, hi)) through its local keys (keys_dev: the
 *      rank's step-1 keys -- for an owned query they equal the global MIN);
 *   5. all_reduce(SUM) of the 24 accumulators, pcp_icp_solve_dev.
 * (point_cloud_helper.cpp:75-166 ICP correspondence/transform step). */
int pcp_icp_keys_dev(pcp_ctx* ctx, pcp_icp* icp, const double* T_dev, float rmax,
                     int64_t target_offset, uint64_t* keys_dev);
int pcp_keys_owner(pcp_ctx* ctx, const uint64_t* keys_dev, int64_t n, const int64_t* bounds_dev, int nshards,
                   uint8_t* owner_dev);
int pcp_icp_accumulate_owned(pcp_ctx* ctx, const double* T_dev, const float* q_dev, size_t q_stride_bytes,
                             int64_t nq, const uint64_t* keys_dev, const uint8_t* owner_dev, int rank,
                             int64_t lo, int64_t hi, const float* shard_xyz_dev, size_t shard_stride_bytes,
                             double* acc_dev);
/* Co-partitioned (slab) multi-GPU mode: latch *flag_dev = 1 when the owned queries' box
 * (host, {x0,x1,y0,y1,z0,z1}) under the device pose reaches outside x in [lo, hi], i.e.
 * the rank's target halo no longer certifies its correspondences (one thread, on the
 * context stream). */
int pcp_slab_guard(pcp_ctx* ctx, const double* T_dev, const double box_host[6], double lo,
                   double hi, int* flag_dev);
/* Host Kabsch/Umeyama solve of the increment dT from 24 accumulators (host memory): with qm, pm
 * the means and S = acc[7..15] - n qm pm^T = U diag(s) V^T (one-sided Jacobi), R = V diag(1, 1,
 * det(V U^T)) U^T, sc = (s0 + s1 + det s2) / sum |q - qm|^2 with do_scale (else 1), t = pm - sc R qm;
 * dT = [sc R, t].  Planar and collinear pairs complete their basis to a proper rotation.
 * Rank 0 -- s0 <= 64 eps max(|acc[7..15]|, n |qm| |pm|), i.e. S is no more than the rounding of
 * the sums it is formed from (every pair at one target point, or every query at one point) --
 * prefers no rotation: dT = [I, pm - qm] with scale 1, PCP_OK.
 * PCP_ERR_ICP (dT untouched) when acc[0] < 3 or any of acc[0..22] is a NaN or an infinity. */
int pcp_icp_solve(const double acc_host[24], int do_scale, double dT_host[16]);
/* Full loop: T_inout (row-major), `iters` iterations (stops early when the increment's
 * rotation and translation fall below eps, eps <= 0 = never).  *err = RMS distance of
 * the last iteration's correspondences. */
int pcp_icp_run(pcp_ctx* ctx, pcp_icp* icp, double T_inout[16], float rmax, int iters,
                int do_scale, double eps, float* err);
/* Device time (ms) of the last pcp_icp_step/pcp_icp_run correspondence kernels
 * (sum over iterations) and the number of launches it covers, from hipEvents. */
int pcp_icp_last_kernel_ms(const pcp_icp* icp, double* ms, int* launches);
/* Device-resident iteration (no host round trip per iteration; multi-GPU callers insert
 * their all-reduce of acc_dev between the two calls on the same stream).  T_dev: 16 doubles
 * row-major in device memory.  pcp_icp_step_dev = pcp_icp_step for the pose in T_dev.
 * pcp_icp_solve_dev: pcp_icp_solve's solve of acc_dev in one device thread (the same code, rank 0
 * and refusals included) and T_dev <- dT * T_dev; stats_dev (4 doubles, zeroed by the caller) =
 * [status (0 ok, -1 failed), sqrt(acc[22] / acc[0]) = rms of the last solved step, running sum of
 * acc[23] (fallback queries), iterations solved].  A refused solve (fewer than 3 pairs, a
 * non-finite accumulator) latches status -1 and leaves T_dev, the rms and the iteration count as
 * they were; every later call on those stats returns at once, so T_dev stays frozen.
 * pcp_icp_run_dev = iters x (step_dev + solve_dev), no convergence test (get_rot_icp with a
 * fixed iteration count; point_cloud_helper.cpp:75-166). */
int pcp_icp_step_dev(pcp_ctx* ctx, pcp_icp* icp, const double* T_dev, float rmax, double* acc_dev);
int pcp_icp_solve_dev(pcp_ctx* ctx, const double* acc_dev, int do_scale, double* T_dev, double* stats_dev);
int pcp_icp_run_dev(pcp_ctx* ctx, pcp_icp* icp, double* T_dev, float rmax, int iters, int do_scale,
                    double* stats_dev);
/* Device ms of the correspondence kernels of every pcp_icp_step_dev / pcp_icp_run_dev launch
 * since the previous call (waits for them), and how many launches that was; resets. */
int pcp_icp_kernel_ms(pcp_ctx* ctx, pcp_icp* icp, double* ms, int* launches);
/* Queries of the last pcp_icp_step that needed the exact ring-search fallback (the fast
 * octant pass could not certify their nearest neighbour). */
int pcp_icp_last_fallback(const pcp_icp* icp, int64_t* n);
/* Queries of the last pcp_icp_step that the verify pass could not settle (searched). */
int pcp_icp_last_searched(const pcp_icp* icp, int64_t* n);
/* The look-ahead of the handle's last launch (waits for it): beta, and the largest offset
 * |c - q_t| (metres) over the corners of the target grid's box grown by rmax.  Both 0 when the
 * launch searched around q_t itself. */
int pcp_icp_last_lookahead(const pcp_icp* icp, double* beta, double* max_offset_m);
/* The caller's prediction of the pose of the handle's SECOND launch (row-major 4x4), from a motion
 * prior say: it replaces the pilot step (none is run) and the first launch looks ahead towards it
 * as described at PCP_ICP_OPT_NO_PILOT, whatever the handle's size.  Only before the first launch
 * (PCP_ERR_ARG afterwards); ignored on a sparse grid and with PCP_ICP_OPT_NO_LOOKAHEAD.  A wrong
 * prediction costs later searches, never exactness; one equal to the first pose or not finite gives
 * beta_0 = 0. */
int pcp_icp_predict_first(pcp_icp* icp, const double T1[16]);
/* What the pilot step of the handle's first launch did (waits for it): the chunk stride S, the
 * number of 64-query chunks it sampled (chunks 0, S, 2S, ...) and the pairs it accumulated.
 * stride = chunks = 0 and pairs = -1 when no pilot ran. */
int pcp_icp_pilot_info(const pcp_icp* icp, int64_t* stride, int64_t* chunks, int64_t* pairs);

/* PointCloudHelper::get_rot_icp (point_cloud_helper.cpp:75-166) on AoS48 clouds:
 * joint centroid (sequential fold over src ++ temp; non-finite points skipped unless both
 * clouds are dense, as cloud_all.is_dense = src.is_dense && temp.is_dense), float cast,
 * ICP(query = temp -> target = src), un-centring t' = t - R c + c.  mat_rot row-major.
 * Returns PCP_OK and *err (< 0 on failure).
 * CONTRACT DIFFERENCE (trimesh2 is absent): the reference calls
 * trimesh::ICP(..., maxdist = 0, ...) (point_cloud_helper.cpp:127), letting trimesh2 pick its
 * distance threshold from the overlap, and returns trimesh2's error.  Here rmax is explicit and
 * must be > 0 (rmax <= 0 -> PCP_ERR_UNSUPPORTED), the ICP is the build's deterministic
 * point-to-point contract, and *err is the RMS distance (m) of the accepted pairs (d <= rmax)
 * of the last iteration.  The reference's callers' thresholds on err (main.cpp:127-128:
 * 0.13 / 0.22, used at main_blend.cpp:79-103) were tuned on trimesh2's value and are NOT
 * calibrated for this one. */
int pcp_get_rot_icp(pcp_ctx* ctx, const void* src_aos48_dev, int64_t ns, int src_is_dense,
                    const void* temp_aos48_dev, int64_t nt, int temp_is_dense,
                    double mat_rot_host[16], float rmax, int iters, int do_scale,
                    double cell_size, float* err);

/* ----------------------------------------------------------------------- I2: point-to-plane ICP
 * The build's OWN point-to-plane contract, NOT parity with trimesh2: the reference registers
 * through trimesh2's ICP() (point_cloud_helper.cpp:127), a library that is absent here; by its
 * published source it minimises point-to-plane distances over normals it estimates itself.  The
 * entries below minimise sum (n_j . (T q_i - p_j))^2 over the exact nearest-neighbour pairs
 * (i, j) of the search above, with the per-point PCA normals of pcp_normals_knn; nothing in
 * them restates trimesh2's weighting, sampling or rejection.
 *
 * Plane table (pcp_icp_planes): one 32-byte record {px,py,pz,0, nx,ny,nz,0} per target point at
 * the target's CALLER index, so a pair costs one 32-byte gather.  target_xyz_dev: fp32 points
 * (stride 0 = 12); normals_dev: packed fp32 normals (stride 0 = 12) or the rows of
 * pcp_normals_knn (stride 24, normal at offset 0).  A record is INVALID, and stored with a zero
 * normal, when !(nx^2 + ny^2 + nz^2 >= 0.25) in fp32 (the {0,0,0,1,..} rows pcp_normals_knn
 * writes for dropped points, a NaN normal) or when its point or normal is not finite.
 * pcp_icp_planes_valid counts the other records (pcp_icp_planes_create waits for that count).
 * The handle holds a reference on its context like an index; it owns one allocator block.
 *
 * pcp_icp_accumulate_plane: the 30 accumulators over the queries i < nq (original order) whose
 * key (pcp_icp_keys_dev) is not INT64_MAX, whose target index j = key & 0xffffffff is < the
 * table's size (a larger index is skipped, never read) and whose record j is valid:
 *   q' = R q + t with the pose cast to fp32 and the fp32 fmaf chain of the point-to-point loop;
 *   p, n widened to fp64; c = q' x n, r = n . (q' - p) in fp64 without contraction; J = (c, n);
 *   [0] pairs, [1..21] upper triangle of sum J J^T row-major (00..05, 11..15, .., 55),
 *   [22..27] sum r J, [28] sum r^2, [29] sum of the keys' fp32 d2.
 * nq == 0 writes 30 zeros.  The result is a plain sum (negating every normal leaves it bit for
 * bit unchanged), so target-sharded callers may all-reduce it before the solve.
 *
 * pcp_icp_solve_plane (host memory only): minimises sum (r + J . x)^2 over x = (omega, t), i.e.
 * A x = -b, with the rotation unknowns scaled by s = sqrt(trace(A_ww) / trace(A_tt)) (the RMS
 * lever arm), the system divided by its largest diagonal entry and factored by unpivoted LDL^T.
 * It FAILS (PCP_ERR_ICP, dT = identity) when n < 6, trace(A_tt) == 0 or any pivot <= 1e-10:
 * numerically singular systems only (one exact plane, two orthogonal planes), not thin ones.
 * dT = [exp([omega]x) by Rodrigues, t], exactly rigid.
 * pcp_icp_solve_plane_dev: the same in one device thread, T_dev <- dT * T_dev; stats_dev (4
 * doubles, zeroed by the caller) = [status (0 ok, -1 failed: T frozen from then on),
 * sqrt([29] / n) = RMS point distance, sqrt([28] / n) = RMS plane distance, iterations solved].
 * pcp_icp_run_plane_dev = iters x (pcp_icp_keys_dev at offset 0, accumulate, solve) on the
 * context's stream with no host round trip; nq must be the handle's query count and the table's
 * size the target index's caller size (PCP_ERR_ARG otherwise). */
#define PCP_ICP_PLANE_ACC 30
typedef struct pcp_icp_planes pcp_icp_planes;  /* packed {p, n} table of an ICP target */

int pcp_icp_planes_create(pcp_ctx* ctx, const float* target_xyz_dev, size_t t_stride_bytes,
                          const float* normals_dev, size_t n_stride_bytes, int64_t n,
                          pcp_icp_planes** out);
int pcp_icp_planes_destroy(pcp_icp_planes* planes);
int64_t pcp_icp_planes_size(const pcp_icp_planes* planes);
int64_t pcp_icp_planes_valid(const pcp_icp_planes* planes);  /* records with a usable normal */

int pcp_icp_accumulate_plane(pcp_ctx* ctx, const double* T_dev, const float* q_dev, size_t q_stride_bytes,
                             int64_t nq, const uint64_t* keys_dev, const pcp_icp_planes* planes,
                             double* acc_dev /* 30 */);
int pcp_icp_solve_plane(const double acc_host[30], double dT_host[16]);
int pcp_icp_solve_plane_dev(pcp_ctx* ctx, const double* acc_dev, double* T_dev, double* stats_dev /* 4 */);
int pcp_icp_run_plane_dev(pcp_ctx* ctx, pcp_icp* icp, const pcp_icp_planes* planes, const float* q_dev,
                          size_t q_stride_bytes, int64_t nq, double* T_dev, float rmax, int iters,
                          double* stats_dev);
/* pcp_get_rot_icp with the point-to-plane loop above (again the build's own contract, not
 * trimesh2's): joint centroid and fp32 centring as pcp_get_rot_icp, an fp64 index over src
 * (automatic cell size) for pcp_normals_knn(normals_k) -- normals are translation-invariant --
 * the plane table, pcp_icp_run_plane_dev from the identity, the same un-centring of t.  Non-finite
 * src points keep their caller index and get an invalid record.  rmax <= 0 -> PCP_ERR_UNSUPPORTED;
 * normals_k errors are pcp_normals_knn's.  *err = RMS point distance (m) of the accepted pairs of
 * the last iteration; a failed solve returns PCP_OK with *err = -1. */
int pcp_get_rot_icp_plane(pcp_ctx* ctx, const void* src_aos48_dev, int64_t ns, int src_is_dense,
                          const void* temp_aos48_dev, int64_t nt, int temp_is_dense,
                          double mat_rot_host[16], float rmax, int iters, int normals_k,
                          double cell_size, float* err);

/* ----------------------------------------------------------------------- I3: trimmed correspondences
 * A data-driven rejection distance under the build's OWN contract (the reference's maxdist = 0
 * lets trimesh2 choose one; that library is absent and nothing here restates it): an exact order
 * statistic of the pairs' squared POINT distances decides which pairs of an iteration are kept.
 *
 * pcp_icp_trim_keys, over n keys as pcp_icp_keys* writes them:
 *   Valid keys.  A key is valid when it is not INT64_MAX.  m is the number of valid keys.
 *     b_i = key_i >> 32 is an unsigned 32-bit integer.  For the keys pcp_icp_keys* writes, b_i is
 *     the bit pattern of a finite non-negative fp32 d2; the unsigned order of the b_i is then the
 *     order of the distances.
 *   Selection.  r = (uint64) floor((double)frac * (double)(m - 1)), computed on the device in
 *     fp64.  sel is the r-th smallest b_i, counted from 0 with multiplicity, in unsigned order.
 *     sel = 0 when m == 0.  The selection is exact: no sampling and no approximate histogram
 *     answer.
 *   Cut.  All steps are fp32, round-to-nearest, without contraction: m2 = mult * mult,
 *     c = m2 * as_float(sel), f2 = d_floor * d_floor, cut = f2 when c is NaN, else max(c, f2)
 *     (f2 when the two compare equal).
 *   Keep.  Key i is kept iff it is valid and as_float(b_i) <= cut as a float comparison; a NaN
 *     pattern is rejected.  keys_out[i] is keys[i] unchanged when kept, including its low 32
 *     bits; otherwise it is exactly INT64_MAX.  Invalid keys stay INT64_MAX.
 *   Aliasing.  keys_out_dev == keys_dev (in place) is allowed, and then only the rejected keys
 *     are stored.  Any other overlap is the caller's error.
 *   Stats.  trim_dev = {m, kept, sel, bits of cut}, written every call.  n == 0 writes
 *     {0, 0, 0, bits(f2)} and touches no key.
 *   Arguments.  PCP_ERR_ARG for: a null context or a null trim_dev; n < 0 or n >= 2^31; null
 *     key pointers with n > 0; frac outside [0, 1] or NaN; mult or d_floor negative or not
 *     finite.  These checks read nothing through ctx.
 *   Execution.  Asynchronous on the context's stream, with no host synchronisation.
 *     Temporaries come from the per-call guard and are released on return, so
 *     pcp_ctx_alloc_stats balances, error paths included.  The result is bit-for-bit the same on
 *     every run: integer histograms and no float atomics.  The keys are read four times (three
 *     radix-select passes over digits of 11, 11 and 10 bits, and the filter).
 * The statistic is the POINT distance: on a sparse cloud it is dominated by the sampling spacing,
 * which is why the rule is a quantile (frac) times a multiplier, not a multiple of the median.
 *
 * Trimmed keys compose with everything that reads keys: pcp_icp_accumulate_plane, and for the
 * point-to-point minimisation pcp_keys_owner (one shard, bounds = {0, n_target}) followed by
 * pcp_icp_accumulate_owned; all of them skip INT64_MAX.
 *
 * pcp_icp_run_plane_trimmed_dev = iters x (pcp_icp_keys_dev at offset 0, pcp_icp_trim_keys in
 * place, accumulate, solve) on the context's stream with no host round trip.  Arguments and
 * stats_dev as pcp_icp_run_plane_dev, plus the trim's; trim_dev receives the stats of the last
 * iteration's trim (untouched when iters == 0).  rmax stays the search bound: the trim only
 * tightens it.  A trim that leaves fewer than 6 pairs makes the solve fail and freezes T. */
#define PCP_ICP_TRIM_STATS 4
int pcp_icp_trim_keys(pcp_ctx* ctx, const uint64_t* keys_dev, int64_t n, float frac, float mult,
                      float d_floor, uint64_t* keys_out_dev, uint64_t* trim_dev /* 4 */);
int pcp_icp_run_plane_trimmed_dev(pcp_ctx* ctx, pcp_icp* icp, const pcp_icp_planes* planes,
                                  const float* q_dev, size_t q_stride_bytes, int64_t nq, double* T_dev,
                                  float rmax, float frac, float mult, float d_floor, int iters,
                                  double* stats_dev /* 4 */, uint64_t* trim_dev /* 4: last iteration */);
/* pcp_get_rot_icp_plane through the trimmed loop: the same steps (joint centroid, centring,
 * normals, plane table, un-centring), rmax <= 0 -> PCP_ERR_UNSUPPORTED as there, the trim's
 * argument rules for frac, mult and d_floor.  *kept_out (optional) = the pairs kept by the last
 * iteration's trim (0 when nothing ran). */
int pcp_get_rot_icp_plane_trimmed(pcp_ctx* ctx, const void* src_aos48_dev, int64_t ns, int src_is_dense,
                                  const void* temp_aos48_dev, int64_t nt, int temp_is_dense,
                                  double mat_rot_host[16], float rmax, float frac, float mult,
                                  float d_floor, int iters, int normals_k, double cell_size, float* err,
                                  int64_t* kept_out);

/* ----------------------------------------------------------------------- I3b: trim by plane residual
 * The same rule as I3 over another statistic: the squared PLANE residual of a pair under the
 * current pose, the quantity the point-to-plane loop minimises.  For a correct pair it is the
 * sensor noise whatever the sampling spacing, so an order statistic of it separates clutter a few
 * decimetres off a surface from good pairs, which the point distance of a sparse cloud cannot.
 * Again the build's OWN contract.  One more key filter in front of the unchanged
 * pcp_icp_accumulate_plane, as pcp_icp_trim_keys is.
 *
 * pcp_icp_trim_keys_plane, over n keys as pcp_icp_keys* writes them, the n queries q_dev they
 * belong to (original order, stride 0 = 12), the device pose T_dev and the target's plane table:
 *   Usable pairs.  Key i is usable iff it is not INT64_MAX, its index j = key & 0xffffffff is < the
 *     table's size (a larger index is never read), record j is valid by pcp_icp_planes's rule, and
 *     its statistic rho_i is not NaN.  m is the number of usable pairs.
 *   Statistic.  q' = R q + t with the pose cast to fp32 and the fp32 fmaf chain of
 *     pcp_icp_accumulate_plane; p, n and q' widened to fp64;
 *     r = (nx * (q'x - px) + ny * (q'y - py)) + nz * (q'z - pz) in plain fp64 operations in that
 *     order, without contraction; rho = (float)(r * r): one fp64 product rounded to nearest fp32.
 *     +inf is an ordinary value.  b_i is the bit pattern of rho_i, a non-negative fp32, so the
 *     unsigned order of the b_i is the order of the |r|.
 *   Selection, cut, keep.  pcp_icp_trim_keys's rules word for word over the b_i of the usable
 *     pairs: r = (uint64) floor((double)frac * (double)(m - 1)) on the device in fp64; sel = the
 *     r-th smallest b_i, counted from 0 with multiplicity, exact, 0 when m == 0; m2 = mult * mult,
 *     c = m2 * as_float(sel), f2 = d_floor * d_floor in fp32, cut = f2 when c is NaN, else
 *     max(c, f2); pair i is kept iff it is usable and rho_i <= cut.  mult and d_floor therefore act
 *     on the plane distance |r|.
 *   Output.  keys_out[i] is keys[i] unchanged when kept, all 64 bits: the high word is still the
 *     POINT d2, so accumulator [29] and stats[1] of the loop keep their meaning.  Every other key
 *     is exactly INT64_MAX, the unusable ones pcp_icp_accumulate_plane would have skipped anyway
 *     included.  Hence pcp_icp_accumulate_plane(keys_out)[0] == kept.
 *   Invariance.  Negating every normal of the table negates r exactly, so keys_out and trim_dev
 *     are bit for bit unchanged.
 *   Aliasing.  keys_out_dev == keys_dev (in place) is allowed, and then only rejected keys are
 *     stored.  Any other overlap is the caller's error.
 *   Stats.  trim_dev = {m, kept, sel, bits of cut}, written every call.  n == 0 writes
 *     {0, 0, 0, bits(f2)} and touches no key.
 *   Arguments.  PCP_ERR_ARG for: a null context, trim_dev, T_dev or planes; n < 0 or n >= 2^31;
 *     null key or query pointers with n > 0; frac outside [0, 1] or NaN; mult or d_floor negative
 *     or not finite; a stride that is not a whole number of floats or is below 12 (0 = 12).  A
 *     rejected call writes nothing.
 *   Execution.  Asynchronous on the context's stream, with no host synchronisation; temporaries
 *     (n residual keys and the select's work memory) come from the per-call guard, so
 *     pcp_ctx_alloc_stats balances, error paths included; the result is bit-for-bit the same on
 *     every run.  Three steps: a residual pass that writes (b_i << 32 | low word of the key) for a
 *     usable pair and INT64_MAX otherwise; pcp_icp_trim_keys's radix select over those residual
 *     keys; a filter pass that reads residual key i and keeps or rejects key i.
 *
 * pcp_icp_run_plane_rtrimmed_dev = iters x (pcp_icp_keys_dev at offset 0, pcp_icp_trim_keys_plane
 * in place at the iteration's pose, accumulate, solve): the arguments, argument checks and stats of
 * pcp_icp_run_plane_trimmed_dev.  A trim that leaves fewer than 6 pairs makes the solve fail and
 * freezes T.
 * pcp_get_rot_icp_plane_rtrimmed: pcp_get_rot_icp_plane_trimmed through that loop; every argument
 * and output as there. */
int pcp_icp_trim_keys_plane(pcp_ctx* ctx, const double* T_dev, const float* q_dev, size_t q_stride_bytes,
                            int64_t n, const uint64_t* keys_dev, const pcp_icp_planes* planes,
                            float frac, float mult, float d_floor,
                            uint64_t* keys_out_dev, uint64_t* trim_dev /* 4 */);
int pcp_icp_run_plane_rtrimmed_dev(pcp_ctx* ctx, pcp_icp* icp, const pcp_icp_planes* planes,
                                   const float* q_dev, size_t q_stride_bytes, int64_t nq, double* T_dev,
                                   float rmax, float frac, float mult, float d_floor, int iters,
                                   double* stats_dev /* 4 */, uint64_t* trim_dev /* 4: last iteration */);
int pcp_get_rot_icp_plane_rtrimmed(pcp_ctx* ctx, const void* src_aos48_dev, int64_t ns, int src_is_dense,
                                   const void* temp_aos48_dev, int64_t nt, int temp_is_dense,
                                   double mat_rot_host[16], float rmax, float frac, float mult,
                                   float d_floor, int iters, int normals_k, double cell_size, float* err,
                                   int64_t* kept_out);

/* ----------------------------------------------------------------------- I5: batched registration
 * Many frame-sized query sets against ONE target in one launch chain (the reference re-registers
 * every frame of a span on its own: do_mul_frame_icp with is_do_sep_icp, process_loop_icp,
 * find_reliable).  A pcp_icp handle costs a sort, its allocations and about ten dependent launches
 * per iteration whatever its size; here B segments with B device poses share one fp32 target
 * index and one plane table, and an iteration is three launches whatever B is.  The single-pair
 * handle, with its neighbour cache, stays the path for large query sets.  The point-to-plane
 * contract is I2's, per segment.
 *
 * Segments.  Segment s is the queries [seg_offsets[s], seg_offsets[s + 1]) of q_dev (fp32 xyz,
 *   stride 0 = 12).  seg_offsets_host has nseg + 1 entries, starts at 0, ends at nq and never
 *   decreases; empty segments are legal, and so are nseg == 0 (then nq == 0) and nq == 0.
 *   pcp_icp_batch_create copies the queries (q_dev may be released after it returns) and waits for
 *   the stream.  PCP_ERR_ARG for: a null context, target, seg_offsets_host or out; a null q_dev with
 *   nq > 0; nq < 0 or nq >= 2^31; nseg < 0 or nseg > 65535; offsets that break the rule above; a
 *   stride that is not a whole number of floats or is below 12; a target that is not an fp32 index.
 *   The target's size limits are pcp_icp_check_sizes's, its grid's pcp_icp_create's.  The handle
 *   holds a reference on its context and borrows the target, as pcp_icp does; it owns three
 *   allocator blocks, returned by pcp_icp_batch_destroy, so pcp_ctx_alloc_stats balances.  Per-call
 *   temporaries of every entry come from the per-call guard, error paths included.
 *
 * Poses.  T_dev is nseg x 16 doubles: segment s has the row-major 4x4 at T_dev + 16 s.  stats_dev
 *   is nseg x 4 doubles, zeroed by the caller: row s is pcp_icp_solve_plane_dev's stats of segment s.
 *
 * pcp_icp_batch_keys_dev writes keys_dev[i] for every query i < nq, in the ORIGINAL order.  The
 *   keys of segment s are, bit for bit, what pcp_icp_keys_dev(ctx, h_s, T_dev + 16 s, rmax, 0, ..)
 *   writes for a pcp_icp h_s created over that segment's queries alone on the same target:
 *     R, t = the pose's 3x4 cast to fp32;
 *     q'x = fmaf(R02, qz, fmaf(R01, qy, fmaf(R00, qx, t0))), rows 1 and 2 alike (fp32, round to
 *       nearest);
 *     d2(j) = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) with d = q' - p_j in fp32, over EVERY finite
 *       target point p_j (j its caller index);
 *     the winner is the lexicographic minimum of (d2, j): the nearest point, the lower caller
 *       index among equal d2 (duplicate points included);
 *     r2 = rmax * rmax in fp32; the pair is accepted iff d2 <= r2 (equality accepts);
 *     key = (bits of the winner's d2) << 32 | j when accepted; INT64_MAX when the query has a
 *       non-finite coordinate, its image q' has one, or no target lies within rmax.
 *   The search is exact for every rmax >= 0 and every pose: rmax many cells wide, images outside
 *   the grid's box, dense and brick (sparse) cell tables.  A segment whose pose is a large rotation
 *   loses the locality of the create-time sort; that costs time, never exactness.  PCP_ERR_ARG for
 *   null pointers and !(rmax >= 0).
 *
 * pcp_icp_batch_accumulate_plane: row s of acc_dev (nseg x 30) is the 30 sums of I2
 *   (pcp_icp_accumulate_plane) over segment s's queries at the pose T_dev + 16 s, paired through
 *   keys_dev (nq keys, original order): the same per-pair arithmetic and the same skips (INT64_MAX,
 *   an index at or past the table's size, an invalid record).  An empty segment writes 30 zeros.
 *   The sum's order is fixed by the handle alone (per 64-query chunk of the segment's sorted
 *   queries a butterfly over the lanes, then the chunks in a fixed order): bit for bit the same on
 *   every run, with no float atomics, and independent of the other segments.  It is a plain sum,
 *   but its order is not pcp_icp_accumulate_plane's: the two agree to rounding, not bit for bit.
 *
 * pcp_icp_batch_solve_plane_dev: device thread s runs pcp_icp_solve_plane_dev's solve on row s of
 *   acc_dev, T_dev + 16 s and stats_dev + 4 s.  A failed solve latches stats[4 s] = -1 and freezes
 *   that segment's pose only (its stats[4 s + 1 .. 3] stay as they were); the others carry on.  An
 *   empty segment, or one with fewer than 6 pairs, fails.
 *
 * pcp_icp_batch_run_plane_dev = iters x (keys, accumulate, solve) over all segments on the context's
 *   stream, with no host round trip and no allocation inside the loop: three launches per iteration
 *   whatever nseg is, and poses bit-identical to calling the three entries in turn.  The plane
 *   table's size must be the target index's caller size (PCP_ERR_ARG otherwise).
 *
 * Not here: the trims of I3 / I3b per segment, and the trimmed loops, are I5b below; the
 * point-to-point minimisation over a batch is I5c; pcp_icp_trim_keys itself over a batch's keys
 * takes ONE quantile across all segments, not one per segment. */
typedef struct pcp_icp_batch pcp_icp_batch;
int pcp_icp_batch_create(pcp_ctx* ctx, const pcp_index* target, const float* q_dev, size_t q_stride_bytes,
                         int64_t nq, const int64_t* seg_offsets_host /* nseg + 1 */, int nseg,
                         pcp_icp_batch** out);
int pcp_icp_batch_destroy(pcp_icp_batch* batch);
int64_t pcp_icp_batch_queries(const pcp_icp_batch* batch);  /* nq as passed */
int pcp_icp_batch_segments(const pcp_icp_batch* batch);
int pcp_icp_batch_keys_dev(pcp_ctx* ctx, pcp_icp_batch* batch, const double* T_dev /* nseg x 16 */, float rmax,
                           uint64_t* keys_dev /* nq, ORIGINAL order */);
int pcp_icp_batch_accumulate_plane(pcp_ctx* ctx, pcp_icp_batch* batch, const double* T_dev,
                                   const uint64_t* keys_dev, const pcp_icp_planes* planes,
                                   double* acc_dev /* nseg x 30 */);
int pcp_icp_batch_solve_plane_dev(pcp_ctx* ctx, const double* acc_dev, int nseg, double* T_dev,
                                  double* stats_dev /* nseg x 4 */);
int pcp_icp_batch_run_plane_dev(pcp_ctx* ctx, pcp_icp_batch* batch, const pcp_icp_planes* planes, double* T_dev,
                                float rmax, int iters, double* stats_dev /* nseg x 4, zeroed by the caller */);

/* ----------------------------------------------------------------------- I5b: per-segment trims of a batch
 * The trims of I3 and I3b applied to every segment of a pcp_icp_batch separately: one exact order
 * statistic, one cut and one kept count PER SEGMENT, in a fixed number of launches whatever nseg and
 * the segment sizes are.  Frames that overlap the map only in part, each at its own distance from
 * convergence, need their own quantile; one pooled quantile over all keys is wrong for them.  With
 * off = the seg_offsets passed to pcp_icp_batch_create:
 *
 * Per segment, bit for bit.  For every segment s the output keys [off[s], off[s + 1]) and row s of
 *   trim_dev (nseg x 4: {m, kept, sel, bits of cut}) are exactly what the single entry writes for
 *   that slice alone:
 *     pcp_icp_batch_trim_keys: pcp_icp_trim_keys(keys_dev + off[s], n_s, frac, mult, d_floor, ..);
 *     pcp_icp_batch_trim_keys_plane: pcp_icp_trim_keys_plane over that slice of keys, segment s's
 *       queries and the pose T_dev + 16 s.
 *   The valid (I3) and usable (I3b) rules, r = (uint64) floor((double)frac * (double)(m - 1)) on
 *   the device in fp64, sel = the exact r-th smallest b_i of the segment counted from 0 with
 *   multiplicity (0 when m == 0), the fp32 cut m2 = mult * mult, c = m2 * as_float(sel),
 *   f2 = d_floor * d_floor, cut = f2 when c is NaN, else max(c, f2), and keep iff as_float(b_i) <= cut
 *   are those sections' word for word.  A kept key is unchanged in all 64 bits; every other written
 *   key is exactly INT64_MAX.
 * Queries.  The plane trim reads the handle's own copy of the queries (pcp_icp_batch_create copies
 *   them, a non-finite query included: its rho is NaN, so its pair is not usable).  keys_dev is nq
 *   keys in the ORIGINAL query order, as pcp_icp_batch_keys_dev writes them.
 * Shared parameters.  frac, mult and d_floor are one scalar each, shared by all segments.
 * Empty and invalid segments.  An empty segment writes the row {0, 0, 0, bits(f2)}.  A segment
 *   whose keys are all invalid (I3) or unusable (I3b) writes {0, 0, 0, bits(f2)} and every key of it
 *   is INT64_MAX afterwards.  nseg == 0 writes nothing and returns PCP_OK.
 * Aliasing.  keys_out_dev == keys_dev (in place) is allowed: the point trim then stores only the
 *   rejected valid keys, the plane trim every key not kept (a pair without a usable plane record is
 *   still a pair in keys).  Out of place every one of the nq keys is written.  Any other overlap
 *   is the caller's error.
 * Composition.  pcp_icp_batch_accumulate_plane(keys_out)[s][0] == kept[s] for the plane trim.
 * Arguments.  PCP_ERR_ARG for: a null context or batch; a null trim_dev with nseg > 0, and for the
 *   plane trim a null T_dev or planes with nseg > 0; null key pointers with nq > 0; frac outside
 *   [0, 1] or NaN; mult or d_floor negative or not finite.  The loops add: iters < 0, !(rmax >= 0),
 *   a null stats_dev with nseg > 0, and a plane table whose size is not the target index's caller
 *   size.  A rejected call writes nothing.
 * Execution.  Asynchronous on the context's stream, no host synchronisation.  Three launches: a
 *   statistic pass (one 64-query chunk per wave) that writes, per slot of the handle's padded
 *   layout, (b_i << 32 | low word of the key) for a valid / usable pair and INT64_MAX otherwise;
 *   one workgroup per segment that runs I3's radix select (digits of 11, 11 and 10 bits) over its
 *   own slots with the histogram and the state in shared memory, and writes the segment's row; a
 *   filter pass (one chunk per wave) that keeps or rejects key i and adds the kept count to its row
 *   with an integer atomic.  Counting is integer only and there are no float atomics: the result
 *   is bit for bit the same on every run.  The handle still owns exactly three allocator blocks;
 *   the 64-bit statistic per slot is per-call guard memory, so pcp_ctx_alloc_stats balances on every
 *   path, error paths included.  A segment is selected by ONE workgroup: the single handle with
 *   pcp_icp_trim_keys stays the path for one very large query set.
 *
 * pcp_icp_batch_run_plane_trimmed_dev / _rtrimmed_dev = iters x (pcp_icp_batch_keys_dev, the point /
 *   plane trim in place at the iteration's poses, pcp_icp_batch_accumulate_plane, sum + solve) over
 *   all segments, with no host round trip and no allocation inside the loop: SIX launches per
 *   iteration (search, statistic, select, filter, accumulate, sum + solve) whatever nseg and the
 *   segment sizes are.  Poses and stats are bit-identical to calling the four entries in turn.
 *   stats_dev as pcp_icp_batch_run_plane_dev (nseg x 4, zeroed by the caller); trim_dev receives
 *   the rows of the last iteration's trim and is untouched when iters == 0.  rmax stays the search
 *   bound.  A segment left with fewer than 6 pairs fails its solve and freezes: that segment only,
 *   the others carry on, and a frozen segment is still trimmed every iteration.
 *
 * Not here: per-segment frac, mult or d_floor; a select split over several workgroups for one very
 * large segment; pcp_get_rot_icp_*-style wrappers.  The point-to-point loops, plain and with the
 * point trim, are I5c. */
int pcp_icp_batch_trim_keys(pcp_ctx* ctx, pcp_icp_batch* batch, const uint64_t* keys_dev /* nq, ORIGINAL order */,
                            float frac, float mult, float d_floor,
                            uint64_t* keys_out_dev, uint64_t* trim_dev /* nseg x 4 */);
int pcp_icp_batch_trim_keys_plane(pcp_ctx* ctx, pcp_icp_batch* batch, const double* T_dev /* nseg x 16 */,
                                  const uint64_t* keys_dev, const pcp_icp_planes* planes,
                                  float frac, float mult, float d_floor,
                                  uint64_t* keys_out_dev, uint64_t* trim_dev /* nseg x 4 */);
int pcp_icp_batch_run_plane_trimmed_dev(pcp_ctx* ctx, pcp_icp_batch* batch, const pcp_icp_planes* planes,
                                        double* T_dev, float rmax, float frac, float mult, float d_floor,
                                        int iters, double* stats_dev /* nseg x 4 */,
                                        uint64_t* trim_dev /* nseg x 4: last iteration */);
int pcp_icp_batch_run_plane_rtrimmed_dev(pcp_ctx* ctx, pcp_icp_batch* batch, const pcp_icp_planes* planes,
                                         double* T_dev, float rmax, float frac, float mult, float d_floor,
                                         int iters, double* stats_dev /* nseg x 4 */,
                                         uint64_t* trim_dev /* nseg x 4: last iteration */);

/* ----------------------------------------------------------------------- I5c: point-to-point over a batch
 * The get_rot_icp contract (point-to-point, with do_scale: pcp_icp_solve, pcp_icp_run_dev) for
 * every segment of a pcp_icp_batch: the ported callers re-register every frame of a span through
 * get_rot_icp (do_mul_frame_icp with is_do_sep_icp), one handle and about thirteen dependent
 * launches per iteration each; here an iteration is three launches whatever nseg is, or six with
 * the per-segment point trim of I5b.  Nothing is fused: a loop is its entries in turn.
 *
 * Target points.  target_xyz_dev is the fp32 cloud the target index was built from, point j at
 *   its CALLER index (stride 0 = 12): the fp32 index keeps no caller-order copy, so the caller
 *   passes it, as pcp_icp_accumulate_owned takes its shard.  pcp_icp_batch_accumulate skips, and
 *   never reads, a key whose index is >= n_target; in the loops n_target must be the index's caller
 *   size (PCP_ERR_ARG otherwise).
 *
 * pcp_icp_batch_accumulate: row s of acc_dev (nseg x PCP_ICP_ACC) is the 24 accumulators of
 *   pcp_icp_solve over segment s's queries whose key (keys_dev: nq keys, ORIGINAL order) is not
 *   INT64_MAX: n, A = sum q' (3), B = sum p (3), AB = sum q' p^T (9, row-major), AA = sum q' q'^T
 *   (upper triangle 00 01 02 11 12 22), D = sum d2, with
 *     q' = the fp32 fmaf chain of I5 at the fp32 cast of the pose T_dev + 16 s (the handle's own
 *       copy of the query), p = target_xyz[j], both widened to fp64: every product of widened fp32
 *       values is exact, and [22] adds the key's fp32 d2 (its high word);
 *     [23] (pcp_icp_step_dev's fallback count) is written 0.
 *   An empty segment writes 24 zeros.  The order of the sum is fixed by the handle alone: per
 *   64-slot chunk of the segment's sorted, padded queries a butterfly over lane offsets 32 .. 1;
 *   then the segment's chunks in eight interleaved groups (group g adds chunks g, g + 8, .. in
 *   order); then the groups in order.  The result is bit for bit the same on every run, uses no
 *   float atomics and is independent of the other segments.  It agrees with
 *   pcp_icp_accumulate_owned over the same pairs to rounding, not bit for bit.
 *
 * pcp_icp_batch_solve_dev: device thread s runs exactly pcp_icp_solve_dev's step on row s of
 *   acc_dev, T_dev + 16 s and stats_dev + 4 s (stats as there: status, RMS point distance of the
 *   last solved step, running sum of [23], steps solved; zeroed by the caller).  It returns at once
 *   when stats[4 s] < 0; stats[4 s + 2] += acc[23]; then pcp_icp_solve(acc, do_scale) -- rank 0,
 *   the planar and collinear completions, the refusals on n < 3 or a non-finite sum, all as there.
 *   On refusal stats[4 s] = -1 and nothing else of that segment changes; otherwise
 *   stats[4 s + 1] = sqrt(acc[22] / acc[0]), stats[4 s + 3] += 1 and T_s <- dT * T_s.  do_scale is
 *   one flag for all segments.  A refused segment freezes alone; the others carry on.
 *
 * pcp_icp_batch_run_dev = iters x (pcp_icp_batch_keys_dev, accumulate, sum + solve) on the context's
 *   stream: three launches per iteration whatever nseg is, no host round trip and no allocation
 *   inside the loop.  Poses and stats are bit-identical to calling the three entries in turn.
 *
 * pcp_icp_batch_run_trimmed_dev = iters x (keys, pcp_icp_batch_trim_keys in place, accumulate, sum +
 *   solve): six launches per iteration, bit-identical to the four entries in turn.  trim_dev
 *   receives the last iteration's rows (nseg x 4, as I5b) and is untouched when iters == 0.  A
 *   frozen segment is still searched and trimmed every iteration.
 *
 * Arguments.  PCP_ERR_ARG for: a null context or batch; a null T_dev, acc_dev, stats_dev or trim_dev
 *   with nseg > 0; null keys with nq > 0; a null target_xyz_dev with n_target > 0; n_target < 0; a
 *   stride that is not a whole number of floats or is below 12; nseg outside [0, 65535] in the solve
 *   entry; iters < 0; !(rmax >= 0); frac, mult and d_floor as I5b.  Every check comes before the
 *   first device call and a rejected call writes nothing.  nseg == 0 returns PCP_OK and writes
 *   nothing.  Temporaries (the loop's keys, the chunks' partial sums, the trim's statistic) come from
 *   the per-call guard, so pcp_ctx_alloc_stats balances on every path.
 *
 * Not here: a fused search + accumulate kernel; per-segment do_scale or trim parameters; the
 * plane-residual trim (it needs a plane table).  The pcp_get_rot_icp-style wrapper with fp64
 * centring is I5d. */
#define PCP_ICP_ACC 24
int pcp_icp_batch_accumulate(pcp_ctx* ctx, pcp_icp_batch* batch, const double* T_dev /* nseg x 16 */,
                             const uint64_t* keys_dev /* nq, ORIGINAL order */,
                             const float* target_xyz_dev, size_t t_stride_bytes, int64_t n_target,
                             double* acc_dev /* nseg x 24 */);
int pcp_icp_batch_solve_dev(pcp_ctx* ctx, const double* acc_dev, int nseg, int do_scale,
                            double* T_dev, double* stats_dev /* nseg x 4 */);
int pcp_icp_batch_run_dev(pcp_ctx* ctx, pcp_icp_batch* batch, const float* target_xyz_dev, size_t t_stride_bytes,
                          int64_t n_target, double* T_dev, float rmax, int iters, int do_scale,
                          double* stats_dev /* nseg x 4, zeroed by the caller */);
int pcp_icp_batch_run_trimmed_dev(pcp_ctx* ctx, pcp_icp_batch* batch, const float* target_xyz_dev,
                                  size_t t_stride_bytes, int64_t n_target, double* T_dev, float rmax,
                                  float frac, float mult, float d_floor, int iters, int do_scale,
                                  double* stats_dev, uint64_t* trim_dev /* nseg x 4: last iteration */);

/* ----------------------------------------------------------------------- I5d: get_rot_icp over a span of frames
 * pcp_get_rot_icp's staging around the loops of I5c, for the caller those loops were built for:
 * do_mul_frame_icp with is_do_sep_icp (main_blend.cpp:839-904) re-registers every frame of a span,
 * each moved by its own fp64 pose, against the map around it.  One call registers nseg AoS48 frames
 * (records [off[s], off[s + 1]) of frames_aos48_dev, at map coordinates) against ONE AoS48 target
 * and returns nseg un-centred 4x4s and nseg errors.  The contract is the build's own, as I1's.
 *
 * Centre.  c = pcp_centroid_aos48(target, target_is_dense): the sequential-fold centroid of the
 *   TARGET ALONE.  CONTRACT DIFFERENCE from pcp_get_rot_icp, whose c is the joint centroid of
 *   src ++ temp: the frames lie inside the target's box by construction (the caller cuts the target
 *   around them), so the target's centroid centres both to fp32's precision, and it needs no pass
 *   over the moved frames.  Any c is removed again by the un-centring below; it only decides where
 *   the fp32 roundings fall.
 * Staging.  For record i of segment s, in one launch whatever nseg is:
 *     moved_i = ((r0 x + r1 y) + r2 z) + t in fp64 with T0_host + 16 s (pcp_transform_aos48's
 *       arithmetic; T0_host == NULL: the identity, through the same arithmetic); the point is left as
 *       it is when !frames_is_dense and it is non-finite;
 *     q32_i = ((float)(moved.x - c0), (float)(moved.y - c1), (float)(moved.z - c2)), packed xyz.
 *   A non-finite q32_i is an ordinary query that gets no key (I5).  The target is centred the same
 *   way without a pose: (float)(p - c).
 * Loop.  pcp_index_build_f32(cell_size) over the centred target, pcp_icp_batch_create over the
 *   staged queries with seg_offsets_host, identity poses and zeroed stats, then pcp_icp_batch_run_dev
 *   (rmax, iters, do_scale), or pcp_icp_batch_run_trimmed_dev when trim_host = {frac, mult, d_floor}
 *   is given; the centred fp32 target is the caller-order cloud of I5c.  Those entries are called as
 *   they are, so poses and stats are bit for bit what a caller gets who stages the same fp32 arrays
 *   and calls them.
 * Results.  With T_s, stats_s the pose and stats row of segment s after the loop:
 *     mat_rot[s] = T_s with t'_r = (t_r - rcv) + c_r, rcv = R_r0 c0; rcv += R_r1 c1; rcv += R_r2 c2
 *       (pcp_get_rot_icp's order), when stats_s[3] > 0; the exact identity for a segment that never
 *       solved (iters == 0, fewer than 3 pairs);
 *     err[s] = (float)stats_s[1] when stats_s[0] == 0 and stats_s[3] > 0, else -1;
 *     steps[s] = stats_s[3] (optional); kept[s] = the kept count of the last iteration's trim row
 *       (optional; 0 without trim_host or with iters == 0).
 *   The caller composes final_s = mat_rot[s] * T0_s.  One device-to-host copy brings poses, stats
 *   and trim rows.
 * Correspondences.  Per-frame registration (pcp_get_rot_icp against the map points of each frame's
 *   own +-3 m box) and this call pair a query image with the same map point as long as that image
 *   stays at least rmax inside its frame's own box: every point within rmax of it is then in both
 *   targets.  The two results then differ only by the fp32 centring (another c) and the order of
 *   the sums.  A frame whose surroundings hold no map point gets err = -1 and the identity here; the
 *   reference skips such a frame because its cache_t is empty.
 * Edges.  rmax <= 0: PCP_ERR_UNSUPPORTED (as pcp_get_rot_icp; nothing is written).  nseg == 0:
 *   PCP_OK, nothing written.  n_target == 0 or nq == 0: PCP_OK, identities, err = -1, steps = 0,
 *   kept = 0.  PCP_ERR_ARG for: a null context or seg_offsets_host; a null cloud with a positive
 *   size; negative sizes; offsets that break pcp_icp_batch_create's rules (nq in place of its nq);
 *   nseg outside [0, 65535]; iters < 0; trim_host values that break I5b's rules; a null mat_rot_host
 *   or err_host with nseg > 0.  Sizes beyond pcp_icp_check_sizes's limits return its code.  Every
 *   check comes before the first device call and a rejected call writes nothing.  The index, the
 *   batch handle and every temporary are released on every path: pcp_ctx_alloc_stats balances. */
int pcp_get_rot_icp_batch(pcp_ctx* ctx, const void* target_aos48_dev, int64_t n_target, int target_is_dense,
                          const void* frames_aos48_dev, int64_t nq, int frames_is_dense,
                          const int64_t* seg_offsets_host /* nseg + 1 */, int nseg,
                          const double* T0_host /* nseg x 16, NULL = identity */,
                          float rmax, int iters, int do_scale, const float* trim_host /* NULL or {frac, mult, d_floor} */,
                          double cell_size, double* mat_rot_host /* nseg x 16 */, float* err_host /* nseg */,
                          int32_t* steps_host /* nseg, optional */, int64_t* kept_host /* nseg, optional, trim only */);

/* ----------------------------------------------------------------------- I4: pose lines
 * Host-only (no device work): n frames' poses as row-major 4x4 doubles, rots[16 * i].
 *
 * pcp_pose_interpolate: do_transform_interpolation (main_blend.cpp:934-980): frames
 * [start, end] re-posed by the slerp-interpolated correction of
 * rot[end] * rot[start]^-1 applied to rot[start].
 * pcp_pose_lum_elch: PointCloudClosure::do_lum_elch (point_cloud_closure.cpp:194-233):
 * rots[i] = E_i * rots[i] over [start, end], E_i the weight-(i-start)/(len-1) share of `loop`.
 * pcp_pose_loop_closure: PointCloudClosure::do_loop_closure (point_cloud_closure.cpp:235-276):
 * splice the optimised span opt (matched by stamp) into ori, spread the start jump over the
 * `window` (400 in the reference) preceding frames, carry the end jump to every later frame.
 * PCP_ERR_ARG where the reference returns false (stamp not found, span length mismatch). */
int pcp_pose_interpolate(double* rots_host, int64_t n, int64_t start, int64_t end);
int pcp_pose_lum_elch(double* rots_host, int64_t n, int64_t start, int64_t end, const double loop_host[16]);
int pcp_pose_loop_closure(double* ori_host, const uint64_t* ori_stamps_host, int64_t n_ori, const double* opt_host,
                          const uint64_t* opt_stamps_host, int64_t n_opt, int64_t window);

/* ----------------------------------------------------------------------- CloudGrid
 * The map cache that builds every ICP target (cloud_grid.h:37-88; callers main_blend.cpp:263,
 * 471, 792-795, 1027): 1 m cells keyed by ((int)x, (int)y), each holding the points kept by
 * add_cloud_internal's sequential 4 cm de-duplication, replayed exactly per cell on the GPU.
 * Clouds are device AoS48 records.
 *
 * pcp_grid_add_cloud: CloudGrid::add_cloud_internal (cloud_grid.cpp:34-78).
 * pcp_grid_clear: CloudGrid::clear (:218-224).
 * pcp_grid_points: get_grid_cloud(CloudPtr&) (:150-158): every kept point, cells in
 * ((int)x, (int)y) order (the reference's is its hash map's), kept order within a cell.
 * pcp_grid_box: get_cloud_with_pos (:84-131): cells i in [i0, i1), j in [j0, j1) in the
 * reference's loop order (the shim derives the ranges from min/max or the pose as it does);
 * out_dev NULL = count only.
 * pcp_grid_match: get_grid_cloud(src, src_out, dst, dis) (:160-216): src points with a grid
 * point of their cell within Chebyshev `dis` (cells spanning < 1.5 m in z skipped) and those
 * grid points once each, in the reference's push order; cap >= pcp_grid_size suffices.
 * pcp_grid_last_dedupe: which path the last pcp_grid_add_cloud's de-duplication took: out[0] =
 * cells whose sub-cell hash filled up (> 3/4 of its slots), so the rest of the cell was tested
 * by a brute scan of its kept points; out[1] = new arrivals tested by that scan.  Both 0 after
 * an add of 0 points.  Results do not depend on the path; tests use this to know it ran.
 *
 * Non-finite input: a point with non-finite or out-of-int-range x or y goes to the cell the
 * x86-64 reference binary puts it in, INT_MIN on that axis ((int) of such a value is undefined
 * in C++; cvttsd2si answers INT_MIN).  NaN z is an ordinary kept point: never a duplicate,
 * ignored by the z range, and it passes the Chebyshev test on z. */
typedef struct pcp_grid pcp_grid;
int pcp_grid_create(pcp_ctx* ctx, pcp_grid** out);
int pcp_grid_destroy(pcp_grid* grid);
int pcp_grid_clear(pcp_ctx* ctx, pcp_grid* grid);
int pcp_grid_add_cloud(pcp_ctx* ctx, pcp_grid* grid, const void* cloud_dev, int64_t n);
int64_t pcp_grid_size(const pcp_grid* grid);
int64_t pcp_grid_cells(const pcp_grid* grid);
int pcp_grid_last_dedupe(const pcp_grid* grid, int64_t out[2]);
int pcp_grid_points(pcp_ctx* ctx, const pcp_grid* grid, void* out_dev, int64_t cap, int64_t* n_out);
int pcp_grid_box(pcp_ctx* ctx, const pcp_grid* grid, int i0, int i1, int j0, int j1, void* out_dev, int64_t cap,
                 int64_t* n_out);
int pcp_grid_match(pcp_ctx* ctx, const pcp_grid* grid, const void* src_dev, int64_t n_src, float dis,
                   void* src_out_dev, int64_t* n_src_out, void* dst_dev, int64_t cap, int64_t* n_dst);

/* ----------------------------------------------------------------------- PCD / LZF I/O
 * Host-only (caller buffers; pinned host memory then stages to the device in one copy).
 * pcp_pcd_write: io::savePCDFile / savePCDFileBinary -> PCDWriter::writeBinary
 * (pcd_helper.h:489-610) or writeBinaryCompressed (:628-790) of n PointXYZRGBA records:
 * the header of generateHeader (:321-371; fields x y z rgba stamp_id, point_type.h:326-332),
 * then packed records, or SoA planes LZF-compressed behind (compressed, uncompressed) u32
 * sizes.  width/height <= 0: n x 1.  PCP_ERR_EMPTY for n == 0 (the reference throws).
 * pcp_pcd_read: io::loadPCDFile (pcd_helper.h:1374-1378 -> PCDReader, pcd_helper.cpp:71-1395)
 * of DATA ascii / binary / binary_compressed; out_host NULL = size query (*n_out = POINTS).
 * Header fields must be PCL datatypes (F 4/8, U/I 1/2/4) or PCP_ERR_ARG; a negative POINTS,
 * WIDTH or HEIGHT, or a DATA section shorter than the header promises, is PCP_ERR_ARG.
 * pcp_pcd_read_ex also reports the header's WIDTH/HEIGHT and is_dense as PCDReader sets it
 * (pcd_helper.cpp:863, 1124-1179: 0 when a binary / binary_compressed field value is
 * non-finite; ascii files stay dense); any of the three may be NULL.
 * pcp_lzf_compress / pcp_lzf_decompress: lzfCompress / lzfDecompress (lzf.cpp:86-415);
 * return the output size, 0 on failure. */
int pcp_pcd_write(const char* path, const void* pts_host, int64_t n, int64_t width, int64_t height, int compressed);
int pcp_pcd_read(const char* path, void* out_host, int64_t cap, int64_t* n_out);
int pcp_pcd_read_ex(const char* path, void* out_host, int64_t cap, int64_t* n_out, int64_t* width_out,
                    int64_t* height_out, int* dense_out);
size_t pcp_lzf_compress(const void* in_host, size_t in_len, void* out_host, size_t out_len);
size_t pcp_lzf_decompress(const void* in_host, size_t in_len, void* out_host, size_t out_len);

#ifdef __cplusplus
}
#endif
#endif /* PCP_H */
