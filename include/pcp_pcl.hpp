// pcp_pcl.hpp -- drop-in C++ surface of the RioWong/PointCloudProcess hot path, on top of
// the libpcp C-ABI (pcp.h).  Header-only; needs neither Eigen, Boost, FLANN, OpenCV nor
// trimesh2.  Class and method names, argument meaning and visible error behaviour follow the
// reference (namespace cloud_blend_double, macros.h:6):
//
//   KdTreeFLANN<PointT>   kd_tree.h:659-997   (exact kNN / radius, index_mapping_)
//   KdTree (lod)          kd_tree_lod/kd_tree.h, .cpp:29-117  (as cloud_blend_double::lod::KdTree)
//   VoxelGrid<PointT>     voxel_grid.h:496-1056
//   CalculateFeature      calculate_feature.h:11-16
//   PointCloudHelper      point_cloud_helper.h:16-233 (remove_duplicate, get_rot_icp,
//                         transformPointCloud, compute3DCentroid, getMinMax3D, point_dis2)
//   CloudStampRot         cloud_stamp_rot.h:7-39
//   PointXYZRGBA / PointCloud / PlanSegment / LAS_POINT_PROPERTY (point_type.h, point_cloud.h,
//   data_struct.h)
//
// Matrices: every Matrix4d / Vector4d parameter is a template accepting anything with
// operator()(int,int) / operator[](int) (Eigen::Matrix4d works unchanged; Mat4d/Vec4d below
// serve callers without Eigen).
//
// Device: all calls run on one process-wide pcp context (device PCP_DEVICE env or 0, the
// device's default stream).  const searches may be called concurrently from OpenMP threads
// (calculate_feature.cpp:216-233): per-point nearestKSearch / radiusSearch calls on one tree
// are coalesced (detail::Combiner): whichever caller finds no batch running takes every
// pending request and runs them as one launch per distinct k (or radius), so T threads cost
// about one launch per T queries.  The batch methods (nearestKSearchBatch /
// radiusSearchBatch / normals) remain the fast path.
// Non-zero pcp status -> the reference's visible behaviour: empty results for searches,
// PCLException for VoxelGrid, err = -1 for ICP (SURVEY.md §8(b) "Errors").
#ifndef PCP_PCL_HPP
#define PCP_PCL_HPP

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <exception>
#include <map>
#include <memory>
#include <mutex>
#include <utility>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "pcp.h"

namespace cloud_blend_double {

// ------------------------------------------------------------------ types
struct alignas(16) PointXYZRGBA {  // point_type.h:9-89 (EIGEN_ALIGN16, 48 bytes)
    union {
        double data[4];
        struct {
            double x, y, z;
        };
    };
    union {
        uint32_t rgba;
        struct {
            uint8_t b, g, r, a;
        };
    };
    uint32_t stamp_id;
    PointXYZRGBA() : rgba(0), stamp_id(0) {
        data[0] = data[1] = data[2] = 0.0;
        data[3] = 1.0;
    }
    PointXYZRGBA(double x_, double y_, double z_) : PointXYZRGBA() { x = x_; y = y_; z = z_; }
};
static_assert(sizeof(PointXYZRGBA) == PCP_AOS48_STRIDE, "PointXYZRGBA must be the 48-byte AoS record");

template <class PointT>
class PointCloud {  // point_cloud.h:295-311 (the fields the hot path uses)
public:
    typedef std::shared_ptr<PointCloud<PointT>> Ptr;
    typedef std::shared_ptr<const PointCloud<PointT>> ConstPtr;
    std::vector<PointT> points;
    uint32_t width = 0, height = 1;
    bool is_dense = true;
    size_t size() const { return points.size(); }
    bool empty() const { return points.empty(); }
    void push_back(const PointT& p) { points.push_back(p); width = (uint32_t)points.size(); height = 1; }
    void clear() { points.clear(); width = 0; }
    PointT& operator[](size_t i) { return points[i]; }
    const PointT& operator[](size_t i) const { return points[i]; }
    Ptr makeShared() const { return Ptr(new PointCloud<PointT>(*this)); }
    // point_cloud.h:130-147: append, width = size, height = 1, dense only if both were
    PointCloud& operator+=(const PointCloud& rhs) {
        points.insert(points.end(), rhs.points.begin(), rhs.points.end());
        width = (uint32_t)points.size();
        height = 1;
        is_dense = is_dense && rhs.is_dense;
        return *this;
    }
};

typedef PointXYZRGBA CloudItem;  // cmm_types.h:11-14
typedef PointCloud<CloudItem> Cloud;
typedef Cloud::Ptr CloudPtr;
typedef Cloud::ConstPtr CloudConstPtr;

struct PlanSegment {  // data_struct.h:188-198
    unsigned short SegmentID = 0;
    std::vector<int> PointID;
    float normal_x = 0, normal_y = 0, normal_z = 0;
    float min_value = 0;
    float curvature = 0;
    float Distance = 0;
};

struct LAS_POINT_PROPERTY {  // data_struct.h:161-172
    float normal_x, normal_y, normal_z;
    double Distance;
    double curvature;
    int PointID;
    int SegmentID;
    float dis_from_point_plane;
};

struct alignas(16) PointC {  // point_type.h:244-316 (64 bytes; the kd-tree uses x, y, z)
    double x = 0, y = 0, z = 0, w = 1.0;
    uint64_t stamp = 0;
    double angle_z = 0;
    double distance_sqr = 0;
};

class PCLException : public std::runtime_error {  // exception.h:11
public:
    explicit PCLException(const std::string& m) : std::runtime_error(m) {}
};

// Minimal row-major 4x4 / 4-vector for callers without Eigen.
struct Mat4d {
    double m[16];
    static Mat4d Identity() {
        Mat4d r;
        for (int i = 0; i < 16; i++) r.m[i] = (i % 5 == 0) ? 1.0 : 0.0;
        return r;
    }
    double& operator()(int r, int c) { return m[4 * r + c]; }
    double operator()(int r, int c) const { return m[4 * r + c]; }
    Mat4d operator*(const Mat4d& b) const {
        Mat4d o;
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) {
                double s = 0;
                for (int k = 0; k < 4; k++) s += (*this)(i, k) * b(k, j);
                o(i, j) = s;
            }
        return o;
    }
};
struct Vec4d {
    double v[4] = {0, 0, 0, 0};
    double& operator[](int i) { return v[i]; }
    double operator[](int i) const { return v[i]; }
    double& operator()(int i) { return v[i]; }
    double operator()(int i) const { return v[i]; }
};

// ------------------------------------------------------------------ device plumbing
namespace detail {

inline void check(int rc, pcp_ctx* ctx, const char* what) {
    if (rc != PCP_OK) throw PCLException(std::string(what) + ": " + (ctx ? pcp_last_error(ctx) : "no context"));
}

class Device {
public:
    static Device& get() {
        static Device d;
        return d;
    }
    pcp_ctx* ctx() { return ctx_; }
    std::mutex& mutex() { return mu_; }

private:
    Device() {
        const char* e = std::getenv("PCP_DEVICE");
        int rc = pcp_ctx_create(e ? std::atoi(e) : 0, nullptr, &ctx_);
        if (rc != PCP_OK) throw PCLException("pcp_ctx_create failed (is libpcp built and a GPU visible?)");
    }
    ~Device() { pcp_ctx_destroy(ctx_); }
    pcp_ctx* ctx_ = nullptr;
    std::mutex mu_;
};

// grow-only device buffer
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void* reserve(size_t bytes) {
        if (!p_ || bytes > cap_) {
            release();
            pcp_ctx* c = Device::get().ctx();
            check(pcp_malloc(c, &p_, bytes ? bytes : 1), c, "pcp_malloc");
            cap_ = bytes;
        }
        return p_;
    }
    void* upload(const void* host, size_t bytes) {
        reserve(bytes);
        pcp_ctx* c = Device::get().ctx();
        if (bytes) check(pcp_memcpy_h2d(c, p_, host, bytes), c, "pcp_memcpy_h2d");
        return p_;
    }
    void download(void* host, size_t bytes) const {
        pcp_ctx* c = Device::get().ctx();
        if (bytes) check(pcp_memcpy_d2h(c, host, p_, bytes), c, "pcp_memcpy_d2h");
    }
    void* ptr() const { return p_; }

private:
    void release() {
        if (p_) pcp_free(Device::get().ctx(), p_);
        p_ = nullptr;
        cap_ = 0;
    }
    void* p_ = nullptr;
    size_t cap_ = 0;
};

template <class PointT>
inline void require_xyz_double_layout() {
    static_assert(sizeof(PointT) % 8 == 0, "PointT must start with x,y,z doubles (point_type.h)");
}

// query points -> packed xyz doubles
template <class PointT>
inline std::vector<double> pack_xyz(const std::vector<PointT>& q) {
    std::vector<double> v(3 * q.size());
    for (size_t i = 0; i < q.size(); i++) {
        v[3 * i] = q[i].x;
        v[3 * i + 1] = q[i].y;
        v[3 * i + 2] = q[i].z;
    }
    return v;
}

// Flat combining of concurrent single requests: submit() enqueues r; a caller that finds no
// batch running becomes the combiner, takes every pending request (its own included) and runs
// them with run(batch); others wait and take over if theirs is still pending when that batch
// ends.  The combiner first waits up to kWindowUs for as many requests as the recent batches
// held (the callers released by the last batch are usually about to come back), so T busy
// threads settle into batches of about T; the hint decays by one per batch when they stop.
// Each request's results are written by the combiner before `done` is set under the lock; a
// failure is re-thrown in every thread whose request was in the failed batch.
template <class Req>
class Combiner {
public:
    template <class Run>
    void submit(Req* r, Run&& run) {
        std::unique_lock<std::mutex> lk(m_);
        q_.push_back(r);
        arrive_.notify_one();
        while (!r->done) {
            if (busy_) {
                cv_.wait(lk);
                continue;
            }
            busy_ = true;
            if (q_.size() < hint_)
                arrive_.wait_for(lk, std::chrono::microseconds(kWindowUs), [&] { return q_.size() >= hint_; });
            std::vector<Req*> batch;
            batch.swap(q_);
            hint_ = std::max(batch.size(), hint_ > 1 ? hint_ - 1 : (size_t)1);
            lk.unlock();
            std::exception_ptr err;
            try {
                run(batch);
            } catch (...) {
                err = std::current_exception();
            }
            lk.lock();
            for (Req* b : batch) {
                b->err = err;
                b->done = true;
            }
            busy_ = false;
            cv_.notify_all();
        }
        if (r->err) std::rethrow_exception(r->err);
    }

private:
    static constexpr int kWindowUs = 100;
    std::mutex m_;
    std::condition_variable cv_, arrive_;
    std::vector<Req*> q_;
    bool busy_ = false;
    size_t hint_ = 1;
};

}  // namespace detail

// ------------------------------------------------------------------ K: KdTreeFLANN
template <class PointT>
class KdTreeFLANN {
public:
    typedef std::shared_ptr<KdTreeFLANN<PointT>> Ptr;
    typedef std::shared_ptr<const KdTreeFLANN<PointT>> ConstPtr;
    typedef typename PointCloud<PointT>::ConstPtr PointCloudConstPtr;
    typedef std::shared_ptr<const std::vector<int>> IndicesConstPtr;

    explicit KdTreeFLANN(bool sorted = true) : sorted_(sorted) { detail::require_xyz_double_layout<PointT>(); }

    // kd_tree.h:772-798: non-finite points dropped, index_mapping_ kept.  The index is
    // reference-counted, so copies of the tree share it safely (the reference's copy
    // constructor shallow-copied raw pointers, kd_tree.h:721-734).
    void setInputCloud(const PointCloudConstPtr& cloud, const IndicesConstPtr& indices = IndicesConstPtr()) {
        input_ = cloud;
        indices_ = indices;
        st_.reset();
        if (!cloud) return;  // reference: silent return (kd_tree.h:784-787)
        std::shared_ptr<State> s(new State);
        pcp_ctx* c = detail::Device::get().ctx();
        std::lock_guard<std::mutex> lk(detail::Device::get().mutex());
        const size_t n = cloud->points.size();
        const double* xyz = (const double*)s->cloud.upload(cloud->points.data(), n * sizeof(PointT));
        const int32_t* ind = nullptr;
        if (indices) ind = (const int32_t*)s->indices.upload(indices->data(), indices->size() * sizeof(int));
        detail::check(pcp_index_build_f64(c, xyz, sizeof(PointT), (int64_t)n, ind,
                                          indices ? (int64_t)indices->size() : 0, 0.0, &s->index),
                      c, "pcp_index_build_f64");
        st_ = s;
    }
    PointCloudConstPtr getInputCloud() const { return input_; }
    IndicesConstPtr getIndices() const { return indices_; }
    void setEpsilon(float eps) { epsilon_ = eps; }  // searches stay exact (the callers' eps = 0)
    float getEpsilon() const { return epsilon_; }
    void setSortedResults(bool sorted) { sorted_ = sorted; }  // sorted is a valid unsorted order
    Ptr makeShared() const { return Ptr(new KdTreeFLANN<PointT>(*this)); }

    // kd_tree.h:814-845
    int nearestKSearch(const PointT& point, int k, std::vector<int>& k_indices,
                       std::vector<double>& k_sqr_distances) const {
        k_indices.clear();
        k_sqr_distances.clear();
        if (!st_ || k <= 0) return 0;
        const int64_t n = pcp_index_size(st_->index);
        if (k > n) k = (int)n;
        if (k == 0) return 0;
        KnnReq r{{point.x, point.y, point.z}, k, &k_indices, &k_sqr_distances};
        st_->knn_q.submit(&r, [this](std::vector<KnnReq*>& b) { run_knn_batch(b); });
        return k;
    }
    int nearestKSearch(const PointCloud<PointT>& cloud, int index, int k, std::vector<int>& k_indices,
                       std::vector<double>& k_sqr_distances) const {  // kd_tree.h:446-452
        return nearestKSearch(cloud.points[index], k, k_indices, k_sqr_distances);
    }
    int nearestKSearch(int index, int k, std::vector<int>& k_indices,
                       std::vector<double>& k_sqr_distances) const {  // kd_tree.h:494-505
        const PointT& p = indices_ ? input_->points[(*indices_)[index]] : input_->points[index];
        return nearestKSearch(p, k, k_indices, k_sqr_distances);
    }

    // kd_tree.h:863-903
    int radiusSearch(const PointT& point, double radius, std::vector<int>& k_indices,
                     std::vector<double>& k_sqr_distances, unsigned int max_nn = 0) const {
        k_indices.clear();
        k_sqr_distances.clear();
        if (!st_) return 0;
        RadReq r{{point.x, point.y, point.z}, radius, max_nn, &k_indices, &k_sqr_distances};
        st_->rad_q.submit(&r, [this](std::vector<RadReq*>& b) { run_radius_batch(b); });
        return (int)k_indices.size();
    }
    int radiusSearch(const PointCloud<PointT>& cloud, int index, double radius, std::vector<int>& k_indices,
                     std::vector<double>& k_sqr_distances, unsigned int max_nn = 0) const {  // :538-545
        return radiusSearch(cloud.points[index], radius, k_indices, k_sqr_distances, max_nn);
    }
    int radiusSearch(int index, double radius, std::vector<int>& k_indices, std::vector<double>& k_sqr_distances,
                     unsigned int max_nn = 0) const {  // :590-601
        const PointT& p = indices_ ? input_->points[(*indices_)[index]] : input_->points[index];
        return radiusSearch(p, radius, k_indices, k_sqr_distances, max_nn);
    }

    // ---- batch extensions (one launch for many queries)
    // find_cloud_nearest_point_in_kdtree (main_blend.cpp:306-325): the query whose 1-NN d2 is
    // smallest (strict '<' from 9999, the first wins ties), or a default point when none beats it
    PointT nearestQuery(const PointCloud<PointT>& cloud) const {
        if (!st_ || cloud.points.empty()) return PointT();
        pcp_ctx* c = detail::Device::get().ctx();
        std::lock_guard<std::mutex> lk(detail::Device::get().mutex());
        std::vector<double> qh = detail::pack_xyz(cloud.points);
        detail::DevBuf q;
        q.upload(qh.data(), qh.size() * sizeof(double));
        int64_t best = -1;
        double bd = 0;
        detail::check(pcp_nearest_query(c, st_->index, (const double*)q.ptr(), 24, (int64_t)cloud.points.size(), 9999.0,
                                        &best, &bd), c, "pcp_nearest_query");
        return best >= 0 ? cloud.points[best] : PointT();
    }
    // rows of k: k_indices[i*k + r] (-1 / +inf past the tree size)
    void nearestKSearchBatch(const std::vector<PointT>& queries, int k, std::vector<int>& k_indices,
                             std::vector<double>& k_sqr_distances) const {
        k_indices.clear();
        k_sqr_distances.clear();
        if (!st_ || k <= 0 || queries.empty()) return;
        run_knn(queries, k, k_indices, k_sqr_distances);
    }
    // CSR: neighbours of query i are [offsets[i], offsets[i+1])
    void radiusSearchBatch(const std::vector<PointT>& queries, double radius, std::vector<int64_t>& offsets,
                           std::vector<int>& k_indices, std::vector<double>& k_sqr_distances,
                           unsigned int max_nn = 0) const {
        offsets.assign(queries.size() + 1, 0);
        k_indices.clear();
        k_sqr_distances.clear();
        if (!st_ || queries.empty()) return;
        run_radius(detail::pack_xyz(queries), radius, max_nn, offsets, k_indices, k_sqr_distances);
    }

    // device-side handles for callers that keep their data in HBM (pcp.h)
    const pcp_index* index() const { return st_ ? st_->index : nullptr; }
    const double* device_cloud() const { return st_ ? (const double*)st_->cloud.ptr() : nullptr; }

private:
    // one coalesced per-point request (nearestKSearch / radiusSearch)
    struct KnnReq {
        double xyz[3];
        int k;
        std::vector<int>* idx;
        std::vector<double>* d2;
        bool done = false;
        std::exception_ptr err;
    };
    struct RadReq {
        double xyz[3];
        double radius;
        unsigned int max_nn;
        std::vector<int>* idx;
        std::vector<double>* d2;
        bool done = false;
        std::exception_ptr err;
    };
    struct State {
        pcp_index* index = nullptr;
        detail::DevBuf cloud, indices;
        detail::Combiner<KnnReq> knn_q;
        detail::Combiner<RadReq> rad_q;
        detail::DevBuf sq, scnt, soff, soi, sod;  // search scratch (grow-only, device mutex held)
        ~State() {
            if (index) pcp_index_destroy(index);
        }
    };
    // one launch per distinct k; row r of request i -> its vectors
    void run_knn_batch(std::vector<KnnReq*>& b) const {
        std::map<int, std::vector<KnnReq*>> by_k;
        for (KnnReq* r : b) by_k[r->k].push_back(r);
        for (auto& g : by_k) {
            const int k = g.first;
            std::vector<double> qh(3 * g.second.size());
            for (size_t i = 0; i < g.second.size(); i++)
                for (int d = 0; d < 3; d++) qh[3 * i + d] = g.second[i]->xyz[d];
            std::vector<int> idx;
            std::vector<double> d2;
            run_knn_xyz(qh, k, idx, d2);
            for (size_t i = 0; i < g.second.size(); i++) {
                g.second[i]->idx->assign(idx.begin() + i * k, idx.begin() + (i + 1) * k);
                g.second[i]->d2->assign(d2.begin() + i * k, d2.begin() + (i + 1) * k);
            }
        }
    }
    // one launch per distinct (radius, max_nn)
    void run_radius_batch(std::vector<RadReq*>& b) const {
        std::map<std::pair<double, unsigned int>, std::vector<RadReq*>> by_r;
        for (RadReq* r : b) by_r[{r->radius, r->max_nn}].push_back(r);
        for (auto& g : by_r) {
            std::vector<double> qh(3 * g.second.size());
            for (size_t i = 0; i < g.second.size(); i++)
                for (int d = 0; d < 3; d++) qh[3 * i + d] = g.second[i]->xyz[d];
            std::vector<int64_t> off;
            std::vector<int> idx;
            std::vector<double> d2;
            run_radius(qh, g.first.first, g.first.second, off, idx, d2);
            for (size_t i = 0; i < g.second.size(); i++) {
                g.second[i]->idx->assign(idx.begin() + off[i], idx.begin() + off[i + 1]);
                g.second[i]->d2->assign(d2.begin() + off[i], d2.begin() + off[i + 1]);
            }
        }
    }
    void run_radius(const std::vector<double>& qh, double radius, unsigned int max_nn, std::vector<int64_t>& offsets,
                    std::vector<int>& k_indices, std::vector<double>& k_sqr_distances) const {
        pcp_ctx* c = detail::Device::get().ctx();
        std::lock_guard<std::mutex> lk(detail::Device::get().mutex());
        const int64_t nq = (int64_t)(qh.size() / 3);
        offsets.assign(nq + 1, 0);
        detail::DevBuf &q = st_->sq, &cnt = st_->scnt, &off = st_->soff, &oi = st_->soi, &od = st_->sod;  // under the device mutex
        q.upload(qh.data(), qh.size() * sizeof(double));
        cnt.reserve(nq * sizeof(int32_t));
        off.reserve((nq + 1) * sizeof(int64_t));
        detail::check(pcp_radius_count(c, st_->index, (const double*)q.ptr(), 24, nq, radius, max_nn,
                                       (int32_t*)cnt.ptr()), c, "pcp_radius_count");
        int64_t total = 0;
        detail::check(pcp_scan_counts(c, (const int32_t*)cnt.ptr(), nq, (int64_t*)off.ptr(), &total), c,
                      "pcp_scan_counts");
        oi.reserve(total * sizeof(int32_t));
        od.reserve(total * sizeof(double));
        detail::check(pcp_radius_fill(c, st_->index, (const double*)q.ptr(), 24, nq, radius, max_nn,
                                      (const int64_t*)off.ptr(), (int32_t*)oi.ptr(), (double*)od.ptr()), c,
                      "pcp_radius_fill");
        off.download(offsets.data(), (nq + 1) * sizeof(int64_t));
        k_indices.resize(total);
        k_sqr_distances.resize(total);
        oi.download(k_indices.data(), total * sizeof(int32_t));
        od.download(k_sqr_distances.data(), total * sizeof(double));
    }
    void run_knn(const std::vector<PointT>& queries, int k, std::vector<int>& idx, std::vector<double>& d2) const {
        run_knn_xyz(detail::pack_xyz(queries), k, idx, d2);
    }
    void run_knn_xyz(const std::vector<double>& qh, int k, std::vector<int>& idx, std::vector<double>& d2) const {
        pcp_ctx* c = detail::Device::get().ctx();
        std::lock_guard<std::mutex> lk(detail::Device::get().mutex());
        const int64_t nq = (int64_t)(qh.size() / 3);
        detail::DevBuf &q = st_->sq, &oi = st_->soi, &od = st_->sod;  // under the device mutex
        q.upload(qh.data(), qh.size() * sizeof(double));
        oi.reserve(nq * k * sizeof(int32_t));
        od.reserve(nq * k * sizeof(double));
        detail::check(pcp_knn(c, st_->index, (const double*)q.ptr(), 24, nq, k, (int32_t*)oi.ptr(),
                              (double*)od.ptr()), c, "pcp_knn");
        idx.resize(nq * k);
        d2.resize(nq * k);
        oi.download(idx.data(), idx.size() * sizeof(int32_t));
        od.download(d2.data(), d2.size() * sizeof(double));
    }
    PointCloudConstPtr input_;
    IndicesConstPtr indices_;
    std::shared_ptr<State> st_;
    float epsilon_ = 0.f;
    bool sorted_ = true;
};

// ------------------------------------------------------------------ K6: kd_tree_lod KdTree
namespace lod {
class KdTree {  // kd_tree_lod/kd_tree.h (cloud_blend_double::KdTree in the lod build)
public:
    void setInputCloud(PointCloud<PointXYZRGBA>::ConstPtr cloud) {
        cloud_ = cloud;
        if (cloud) dev_.upload(cloud->points.data(), cloud->points.size() * sizeof(PointXYZRGBA));
    }
    // kd_tree.cpp:78-117, including the k_dis2 quirk (residual of the last scanned point)
    int nearestKSearch(const PointXYZRGBA& point, int k, std::vector<int>& k_indices, std::vector<double>& k_dis2) {
        k_indices.clear();
        k_dis2.clear();
        if (!cloud_ || cloud_->points.empty() || k <= 0) return 0;
        const int64_t n = (int64_t)cloud_->points.size();
        const int kk = (int)(k < n ? k : n);
        pcp_ctx* c = detail::Device::get().ctx();
        std::lock_guard<std::mutex> lk(detail::Device::get().mutex());
        detail::DevBuf q, oi, od;
        q.upload(&point, sizeof(PointXYZRGBA));
        oi.reserve(k * sizeof(int32_t));
        od.reserve(k * sizeof(double));
        detail::check(pcp_knn_lod(c, dev_.ptr(), n, q.ptr(), 1, k, (int32_t*)oi.ptr(), (double*)od.ptr()), c,
                      "pcp_knn_lod");
        k_indices.resize(kk);
        k_dis2.resize(kk);
        oi.download(k_indices.data(), kk * sizeof(int32_t));
        od.download(k_dis2.data(), kk * sizeof(double));
        return kk;
    }

private:
    PointCloud<PointXYZRGBA>::ConstPtr cloud_;
    detail::DevBuf dev_;
};
}  // namespace lod

// ------------------------------------------------------------------ V3: VoxelGrid
template <class PointT>
class VoxelGrid {  // voxel_grid.h:496-1056 (PointXYZRGBA records)
public:
    typedef typename PointCloud<PointT>::ConstPtr PointCloudConstPtr;
    VoxelGrid() { static_assert(sizeof(PointT) == PCP_AOS48_STRIDE, "VoxelGrid<PointXYZRGBA> only"); }
    void setInputCloud(const PointCloudConstPtr& cloud) { input_ = cloud; }
    PointCloudConstPtr getInputCloud() const { return input_; }
    void setLeafSize(double lx, double ly, double lz) {  // voxel_grid.h:538-549
        leaf_[0] = lx; leaf_[1] = ly; leaf_[2] = lz; leaf_[3] = 1.0;
    }
    template <class V4>
    void setLeafSize(const V4& l) {  // voxel_grid.h:522-536 (Vector4d)
        leaf_[0] = l[0]; leaf_[1] = l[1]; leaf_[2] = l[2]; leaf_[3] = (l[3] == 0) ? 1.0 : l[3];
    }
    Vec4d getLeafSize() const {
        Vec4d v;
        for (int i = 0; i < 4; i++) v[i] = leaf_[i];
        return v;
    }
    void setDownsampleAllData(bool d) { all_data_ = d; }
    bool getDownsampleAllData() const { return all_data_; }
    // Optional reference paths outside this build's scope: rejected loudly.
    void setSaveLeafLayout(bool s) { save_layout_ = s; }
    bool getSaveLeafLayout() const { return save_layout_; }
    void setFilterFieldName(const std::string& f) { field_ = f; }
    const std::string& getFilterFieldName() const { return field_; }
    void setFilterLimits(double lo, double hi) { lim_lo_ = lo; lim_hi_ = hi; }
    void setFilterLimitsNegative(bool n) { lim_neg_ = n; }

    // grid getters of the last filter() (voxel_grid.h:552-706)
    const int* getMinBoxCoordinates() const { return min_b_; }
    const int* getMaxBoxCoordinates() const { return max_b_; }
    const int* getNrDivisions() const { return div_b_; }
    const int* getDivisionMultiplier() const { return divb_mul_; }

    void filter(PointCloud<PointT>& output) {  // Filter::filter -> applyFilter
        if (!input_) {  // voxel_grid.h:815-820
            output.points.clear();
            output.width = 0;
            output.height = 1;
            return;
        }
        if (save_layout_ || !field_.empty())
            throw PCLException("VoxelGrid: leaf layout / field-limit filtering is not part of this build");
        pcp_ctx* c = detail::Device::get().ctx();
        std::lock_guard<std::mutex> lk(detail::Device::get().mutex());
        const int64_t n = (int64_t)input_->points.size();
        detail::DevBuf in, out;
        in.upload(input_->points.data(), n * sizeof(PointT));
        out.reserve((n ? n : 1) * sizeof(PointT));
        double mn[4], mx[4];
        detail::check(pcp_minmax_aos48(c, in.ptr(), n, input_->is_dense ? 1 : 0, mn, mx), c, "pcp_minmax_aos48");
        for (int a = 0; a < 3; a++) {  // voxel_grid.h:835-847
            min_b_[a] = (int)(double)(mn[a] * (1.0 / leaf_[a]));
            max_b_[a] = (int)(double)(mx[a] * (1.0 / leaf_[a]));
            div_b_[a] = max_b_[a] - min_b_[a] + 1;
        }
        divb_mul_[0] = 1;
        divb_mul_[1] = div_b_[0];
        divb_mul_[2] = (int)((uint32_t)div_b_[0] * (uint32_t)div_b_[1]);
        int64_t m = 0;
        const int rc = pcp_voxel_filter(c, in.ptr(), n, input_->is_dense ? 1 : 0, leaf_, all_data_ ? 1 : 0,
                                        out.ptr(), &m, nullptr);
        if (rc != PCP_OK) throw PCLException(std::string("VoxelGrid::filter: ") + pcp_last_error(c));
        output.points.resize(m);
        out.download(output.points.data(), m * sizeof(PointT));
        output.width = (uint32_t)m;
        output.height = 1;
        output.is_dense = true;
    }

private:
    PointCloudConstPtr input_;
    double leaf_[4] = {0, 0, 0, 1};
    bool all_data_ = true;  // voxel_grid.h:499
    bool save_layout_ = false;
    std::string field_;
    double lim_lo_ = -1e308, lim_hi_ = 1e308;
    bool lim_neg_ = false;
    int min_b_[3] = {0, 0, 0}, max_b_[3] = {0, 0, 0}, div_b_[3] = {0, 0, 0}, divb_mul_[3] = {0, 0, 0};
};

// ------------------------------------------------------------------ I: PointCloudHelper
class PointCloudHelper {  // point_cloud_helper.h:10-237 (the hot-path members)
public:
    // getMinMax3D(cloud, Vector4d&, Vector4d&) (:59-90): max starts at DBL_MIN
    template <class PointT, class V4>
    static void getMinMax3D(const PointCloud<PointT>& cloud, V4& min_pt, V4& max_pt) {
        static_assert(sizeof(PointT) == PCP_AOS48_STRIDE, "AoS48 records");
        pcp_ctx* c = detail::Device::get().ctx();
        std::lock_guard<std::mutex> lk(detail::Device::get().mutex());
        detail::DevBuf in;
        in.upload(cloud.points.data(), cloud.points.size() * sizeof(PointT));
        double mn[4], mx[4];
        detail::check(pcp_minmax_aos48(c, in.ptr(), (int64_t)cloud.points.size(), cloud.is_dense ? 1 : 0, mn, mx), c,
                      "pcp_minmax_aos48");
        for (int a = 0; a < 4; a++) { min_pt[a] = mn[a]; max_pt[a] = mx[a]; }
    }
    // getMinMax3D(cloud, PointT&, PointT&) (:22-57): the same reduction, only x/y/z of the
    // two points are written (the other fields keep their values)
    template <class PointT>
    static void getMinMax3D(const PointCloud<PointT>& cloud, PointT& min_pt, PointT& max_pt) {
        double mn[4], mx[4];
        getMinMax3D(cloud, mn, mx);
        min_pt.x = mn[0]; min_pt.y = mn[1]; min_pt.z = mn[2];
        max_pt.x = mx[0]; max_pt.y = mx[1]; max_pt.z = mx[2];
    }
    // compute3DCentroid (:193-230): the reference's sequential fold, bit for bit (fold.hip)
    template <class PointT, class V4>
    static unsigned int compute3DCentroid(const PointCloud<PointT>& cloud, V4& centroid) {
        if (cloud.points.empty()) return 0;
        pcp_ctx* c = detail::Device::get().ctx();
        std::lock_guard<std::mutex> lk(detail::Device::get().mutex());
        detail::DevBuf in;
        in.upload(cloud.points.data(), cloud.points.size() * sizeof(PointT));
        double cc[4];
        uint32_t cnt = 0;
        detail::check(pcp_centroid_aos48(c, in.ptr(), (int64_t)cloud.points.size(), cloud.is_dense ? 1 : 0, cc, &cnt),
                      c, "pcp_centroid_aos48");
        for (int a = 0; a < 4; a++) centroid[a] = cc[a];
        return cnt;
    }
    // transformPointCloud (:92-127)
    template <class PointT, class M>
    static void transformPointCloud(const PointCloud<PointT>& in, PointCloud<PointT>& out, const M& transform) {
        static_assert(sizeof(PointT) == PCP_AOS48_STRIDE, "AoS48 records");
        double T[16];
        for (int r = 0; r < 4; r++)
            for (int col = 0; col < 4; col++) T[4 * r + col] = transform(r, col);
        pcp_ctx* c = detail::Device::get().ctx();
        std::lock_guard<std::mutex> lk(detail::Device::get().mutex());
        const int64_t n = (int64_t)in.points.size();
        detail::DevBuf buf;
        buf.upload(in.points.data(), n * sizeof(PointT));
        detail::check(pcp_transform_aos48(c, buf.ptr(), buf.ptr(), n, in.is_dense ? 1 : 0, T), c,
                      "pcp_transform_aos48");
        if (&out != &in) {
            out.width = in.width;
            out.height = in.height;
            out.is_dense = in.is_dense;
        }
        out.points.resize(n);
        buf.download(out.points.data(), n * sizeof(PointT));
    }
    // remove_duplicate(cloud, float leaf) (point_cloud_helper.cpp:42-63)
    static void remove_duplicate(CloudPtr cloud_src, const float voxel_grid_size) {
        if (!cloud_src) return;
        pcp_ctx* c = detail::Device::get().ctx();
        std::lock_guard<std::mutex> lk(detail::Device::get().mutex());
        const int64_t n = (int64_t)cloud_src->points.size();
        detail::DevBuf in, out;
        in.upload(cloud_src->points.data(), n * sizeof(CloudItem));
        out.reserve((n ? n : 1) * sizeof(CloudItem));
        int64_t m = 0;
        detail::check(pcp_remove_duplicate(c, in.ptr(), n, cloud_src->is_dense ? 1 : 0, voxel_grid_size, out.ptr(), &m),
                      c, "pcp_remove_duplicate");
        cloud_src->points.resize(m);
        out.download(cloud_src->points.data(), m * sizeof(CloudItem));
        cloud_src->width = (uint32_t)m;
        cloud_src->height = 1;
        cloud_src->is_dense = true;
    }
    // (:65-73): keep the result only when at least min_num points survive
    static void remove_duplicate(CloudPtr cloud_src, const float voxel_grid_size, int min_num) {
        CloudPtr tmp(new Cloud(*cloud_src));
        remove_duplicate(tmp, voxel_grid_size);
        if ((int)tmp->size() >= min_num) *cloud_src = *tmp;
    }
    // get_rot_icp (:75-166): returns err (< 0 on failure); do_affine is outside this build.
    // CONTRACT DIFFERENCE -- read before porting a caller.  The reference's get_rot_icp has no
    // iteration count or distance parameters: it calls trimesh::ICP(..., maxdist = 0, ...)
    // (:127), so trimesh2 (absent from the tree) chooses its own threshold from the overlap and
    // its own stopping rule, and returns ITS error measure.  This build runs its deterministic
    // point-to-point ICP for `iters` iterations with the explicit correspondence distance
    // `maxdist` (defaults below are this build's choice: 20 iterations, 0.25 m), and err is the
    // RMS distance (m) of the pairs accepted (d <= maxdist) in the last iteration.  The
    // reference's thresholds on err (main.cpp:127-128: 0.13 / 0.22, used at main_blend.cpp:79-103)
    // were tuned on trimesh2's value and are NOT calibrated for this one.  maxdist <= 0 (the
    // reference's "automatic") is rejected: err = -1.
    static constexpr int kIcpIters = 20;
    static constexpr float kIcpMaxDist = 0.25f;
    template <class M>
    static float get_rot_icp(CloudPtr cloud_src, CloudPtr cloud_temp, M& mat_rot, bool do_scale = false,
                             bool do_affine = false, int iters = kIcpIters, float maxdist = kIcpMaxDist) {
        for (int r = 0; r < 4; r++)
            for (int col = 0; col < 4; col++) mat_rot(r, col) = (r == col) ? 1.0 : 0.0;
        if (do_affine || !cloud_src || !cloud_temp || !(maxdist > 0.f)) return -1.0f;
        pcp_ctx* c = detail::Device::get().ctx();
        std::lock_guard<std::mutex> lk(detail::Device::get().mutex());
        detail::DevBuf s, t;
        s.upload(cloud_src->points.data(), cloud_src->points.size() * sizeof(CloudItem));
        t.upload(cloud_temp->points.data(), cloud_temp->points.size() * sizeof(CloudItem));
        double Mh[16];
        float err = -1.0f;
        const int rc = pcp_get_rot_icp(c, s.ptr(), (int64_t)cloud_src->size(), cloud_src->is_dense ? 1 : 0, t.ptr(),
                                       (int64_t)cloud_temp->size(), cloud_temp->is_dense ? 1 : 0, Mh, maxdist, iters,
                                       do_scale ? 1 : 0, 0.0, &err);
        if (rc != PCP_OK) return -1.0f;
        for (int r = 0; r < 4; r++)
            for (int col = 0; col < 4; col++) mat_rot(r, col) = Mh[4 * r + col];
        return err;
    }
    // get_rot_icp for every frame of a span in one call (pcp.h I5d; not in the reference): frame s,
    // moved by T0s[s], is registered against `cache` (point-to-point, no scale), all frames in the
    // same three launches per iteration.  out_rots[s] receives the un-centred 4x4 (the frame's
    // pose is out_rots[s] * T0s[s]) and out_errs[s] the RMS pair distance, -1 for a frame that
    // found no pairs (its out_rots[s] is the identity).  The centre is the cache's own centroid, not
    // get_rot_icp's joint one.  A null frame counts as empty.  Returns false, with identities and
    // -1s, when the call is rejected (maxdist <= 0, T0s.size() != frames.size()).
    template <class M>
    static bool get_rot_icp_batch(CloudPtr cache, const std::vector<CloudPtr>& frames, const std::vector<M>& T0s,
                                  std::vector<M>& out_rots, std::vector<float>& out_errs, int iters = kIcpIters,
                                  float maxdist = kIcpMaxDist) {
        const size_t B = frames.size();
        out_rots.resize(B);
        out_errs.assign(B, -1.0f);
        for (size_t s = 0; s < B; s++)
            for (int r = 0; r < 4; r++)
                for (int col = 0; col < 4; col++) out_rots[s](r, col) = (r == col) ? 1.0 : 0.0;
        if (!cache || T0s.size() != B || B > 65535 || !(maxdist > 0.f) || iters < 0) return false;
        if (B == 0) return true;
        std::vector<int64_t> off(B + 1, 0);
        std::vector<CloudItem> span;
        std::vector<double> T0(16 * B), Mh(16 * B);
        bool dense = true;
        for (size_t s = 0; s < B; s++) {
            if (frames[s]) {
                span.insert(span.end(), frames[s]->points.begin(), frames[s]->points.end());
                dense = dense && frames[s]->is_dense;
            }
            off[s + 1] = (int64_t)span.size();
            for (int r = 0; r < 4; r++)
                for (int col = 0; col < 4; col++) T0[16 * s + 4 * r + col] = T0s[s](r, col);
        }
        pcp_ctx* c = detail::Device::get().ctx();
        std::lock_guard<std::mutex> lk(detail::Device::get().mutex());
        detail::DevBuf t, f;
        t.upload(cache->points.data(), cache->points.size() * sizeof(CloudItem));
        f.upload(span.data(), span.size() * sizeof(CloudItem));
        const int rc = pcp_get_rot_icp_batch(c, t.ptr(), (int64_t)cache->size(), cache->is_dense ? 1 : 0, f.ptr(),
                                             (int64_t)span.size(), dense ? 1 : 0, off.data(), (int)B, T0.data(), maxdist,
                                             iters, 0, nullptr, 0.0, Mh.data(), out_errs.data(), nullptr, nullptr);
        if (rc != PCP_OK) return false;
        for (size_t s = 0; s < B; s++)
            for (int r = 0; r < 4; r++)
                for (int col = 0; col < 4; col++) out_rots[s](r, col) = Mh[16 * s + 4 * r + col];
        return true;
    }
    // point_dis2 (point_cloud_helper.h:20): pow(dx,2)+pow(dy,2)+pow(dz,2)
    static double point_dis2(const PointXYZRGBA& p1, const PointXYZRGBA& p2) {
        const double dx = p1.x - p2.x, dy = p1.y - p2.y, dz = p1.z - p2.z;
        return dx * dx + dy * dy + dz * dz;
    }
};

// ------------------------------------------------------------------ F: CalculateFeature
class CalculateFeature {  // calculate_feature.h:11-16
public:
    // calculate_feature.cpp:28-33
    int compute_iteration_number(float Pr, float epi, int /*h_free*/) {
        return (int)(std::log10(1 - Pr) / std::log10(1 - std::pow(1 - epi, 3)));
    }
    // F1 (calculate_feature.cpp:119-206) over all points of `cloud`
    PlanSegment calculate_plan_parameter_h_points(CloudPtr cloud) {
        PlanSegment out;
        if (!cloud || cloud->points.empty()) return out;
        pcp_plane p = fit(cloud->points.data(), cloud->points.size());
        copy(p, out);
        return out;
    }
    // F2 (:35-117): the same PCA on 3 points
    PlanSegment calculate_plan_parameter_3points(CloudItem points[3]) {
        PlanSegment out;
        pcp_plane p = fit(points, 3);
        copy(p, out);
        return out;
    }
    // F4 (declared-only, calculate_feature.h:15): F1 over each point's radius neighbourhood
    std::shared_ptr<LAS_POINT_PROPERTY> calculate_plan_parameter(CloudPtr cloud, double radius) {
        return per_point(cloud, [&](KdTreeFLANN<CloudItem>& tree, std::vector<int64_t>& off, std::vector<int>& idx) {
            std::vector<double> d2;
            tree.radiusSearchBatch(cloud->points, radius, off, idx, d2);
        });
    }
    // F3 (:208-368): robust RPCA normals over each point's kNN(20) on the GPU
    // (pcp_normals_rpca).  Deterministic: the reference's rand() draws (srand(time) :210, :249)
    // are a counter-based hash of (seed, point, iteration, slot); `seed` is this build's
    // addition.  radius is unused, as in the reference.
    std::shared_ptr<LAS_POINT_PROPERTY> calculate_plan_parameter_rpca(CloudPtr cloud, double /*radius*/, float pr,
                                                                       float epi, uint64_t seed = 0) {
        static_assert(sizeof(LAS_POINT_PROPERTY) == sizeof(pcp_point_property), "LAS_POINT_PROPERTY layout");
        const size_t n = cloud ? cloud->points.size() : 0;
        std::shared_ptr<LAS_POINT_PROPERTY> res(new LAS_POINT_PROPERTY[n ? n : 1],
                                                std::default_delete<LAS_POINT_PROPERTY[]>());
        if (!n) return res;
        KdTreeFLANN<CloudItem> tree;
        tree.setInputCloud(cloud);
        const int k = 20;  // calculate_feature.cpp:233
        std::vector<int> idx;
        std::vector<double> d2;
        tree.nearestKSearchBatch(cloud->points, k, idx, d2);
        pcp_ctx* c = detail::Device::get().ctx();
        std::lock_guard<std::mutex> lk(detail::Device::get().mutex());
        detail::DevBuf didx, dout;
        didx.upload(idx.data(), idx.size() * sizeof(int));
        dout.reserve(n * sizeof(pcp_point_property));
        detail::check(pcp_normals_rpca(c, tree.device_cloud(), sizeof(CloudItem), (int64_t)n,
                                       (const int32_t*)didx.ptr(), k, pr, epi, seed, (pcp_point_property*)dout.ptr()),
                      c, "pcp_normals_rpca");
        dout.download(res.get(), n * sizeof(LAS_POINT_PROPERTY));
        return res;
    }

private:
    static void copy(const pcp_plane& p, PlanSegment& o) {
        o.normal_x = p.normal_x; o.normal_y = p.normal_y; o.normal_z = p.normal_z;
        o.min_value = p.min_value; o.curvature = p.curvature; o.Distance = p.distance;
    }
    static pcp_plane fit(const CloudItem* pts, size_t n) {
        pcp_ctx* c = detail::Device::get().ctx();
        std::lock_guard<std::mutex> lk(detail::Device::get().mutex());
        detail::DevBuf xyz, off, out;
        xyz.upload(pts, n * sizeof(CloudItem));
        const int64_t o[2] = {0, (int64_t)n};
        off.upload(o, sizeof(o));
        out.reserve(sizeof(pcp_plane));
        detail::check(pcp_plane_fit_segments(c, (const double*)xyz.ptr(), sizeof(CloudItem), (const int64_t*)off.ptr(),
                                             nullptr, 1, (pcp_plane*)out.ptr()), c, "pcp_plane_fit_segments");
        pcp_plane p;
        out.download(&p, sizeof(p));
        return p;
    }
    template <class Neigh>
    std::shared_ptr<LAS_POINT_PROPERTY> per_point(CloudPtr cloud, Neigh neigh) {
        const size_t n = cloud ? cloud->points.size() : 0;
        std::shared_ptr<LAS_POINT_PROPERTY> res(new LAS_POINT_PROPERTY[n ? n : 1],
                                                std::default_delete<LAS_POINT_PROPERTY[]>());
        if (!n) return res;
        KdTreeFLANN<CloudItem> tree;
        tree.setInputCloud(cloud);
        std::vector<int64_t> off;
        std::vector<int> idx;
        neigh(tree, off, idx);
        std::vector<pcp_plane> planes(n);
        {
            pcp_ctx* c = detail::Device::get().ctx();
            std::lock_guard<std::mutex> lk(detail::Device::get().mutex());
            detail::DevBuf doff, didx, dout;
            doff.upload(off.data(), off.size() * sizeof(int64_t));
            didx.upload(idx.data(), idx.size() * sizeof(int));
            dout.reserve(n * sizeof(pcp_plane));
            detail::check(pcp_plane_fit_segments(c, tree.device_cloud(), sizeof(CloudItem), (const int64_t*)doff.ptr(),
                                                 (const int32_t*)didx.ptr(), (int64_t)n, (pcp_plane*)dout.ptr()),
                          c, "pcp_plane_fit_segments");
            dout.download(planes.data(), n * sizeof(pcp_plane));
        }
        for (size_t i = 0; i < n; i++) {
            LAS_POINT_PROPERTY& r = res.get()[i];
            r.normal_x = planes[i].normal_x;
            r.normal_y = planes[i].normal_y;
            r.normal_z = planes[i].normal_z;
            r.Distance = planes[i].distance;
            r.curvature = planes[i].curvature;
            r.PointID = (int)i;
            r.SegmentID = 0;
            r.dis_from_point_plane = 0.f;
        }
        return res;
    }
};

// ------------------------------------------------------------------ F: TreeExtration (region growing)
class TreeExtration {  // extraction_tree.h (the region-growing members)
public:
    // extraction_tree.cpp:36-44 (float arithmetic, cmath's float sqrt)
    float compute_included_angle_between_vector(float vx1, float vy1, float vz1, float vx2, float vy2, float vz2) {
        const float n_n1 = vx1 * vx2 + vy1 * vy2 + vz1 * vz2;
        const float n_n = std::sqrt(vx1 * vx1 + vy1 * vy1 + vz1 * vz1);
        const float n1_n1 = std::sqrt(vx2 * vx2 + vy2 * vy2 + vz2 * vz2);
        return std::abs(n_n1 / (n_n * n1_n1));
    }
    // extraction_tree.cpp:47-64
    float compute_distance_from_point_to_plane(const CloudItem* a_point, float a, float b, float c, float d) {
        const float x1 = (float)a_point->x, y1 = (float)a_point->y, z1 = (float)a_point->z;
        const double g = std::sqrt(a * a + b * b + c * c);
        const double f1 = a * x1, f2 = b * y1, f3 = c * z1, f4 = d;
        return (float)(std::abs(f1 + f2 + f3 + f4) / g);
    }
    // extraction_tree.cpp:66-272 through pcp_region_growing (kNN(50) graph and the plane test on
    // the GPU, the sequential seed walk on the host).  PointProperty's SegmentID is rewritten,
    // as in the reference (shared array).  radius is unused, as in the reference.
    std::vector<PlanSegment> region_growning(std::shared_ptr<LAS_POINT_PROPERTY> PointProperty, CloudPtr& Cloud,
                                             double distanceT, double /*radius*/, double cosfaT) {
        std::vector<PlanSegment> out;
        const size_t n = Cloud ? Cloud->points.size() : 0;
        if (!n) return out;
        KdTreeFLANN<CloudItem> tree;
        tree.setInputCloud(Cloud);
        std::vector<int64_t> off(n + 1);
        std::vector<int32_t> pts(n), seeds(n);
        int64_t nseg = 0;
        {
            pcp_ctx* c = detail::Device::get().ctx();
            std::lock_guard<std::mutex> lk(detail::Device::get().mutex());
            detail::DevBuf props;
            props.upload(PointProperty.get(), n * sizeof(LAS_POINT_PROPERTY));
            detail::check(pcp_region_growing(c, tree.index(), tree.device_cloud(), sizeof(CloudItem), (int64_t)n,
                                             (pcp_point_property*)props.ptr(), distanceT, cosfaT, off.data(),
                                             pts.data(), seeds.data(), &nseg),
                          c, "pcp_region_growing");
            props.download(PointProperty.get(), n * sizeof(LAS_POINT_PROPERTY));
        }
        out.resize((size_t)nseg);
        for (int64_t s = 0; s < nseg; s++) {
            PlanSegment& t = out[s];
            const LAS_POINT_PROPERTY& sp = PointProperty.get()[seeds[s]];
            t.SegmentID = (unsigned short)s;
            t.PointID.assign(pts.begin() + off[s], pts.begin() + off[s + 1]);
            t.normal_x = sp.normal_x;
            t.normal_y = sp.normal_y;
            t.normal_z = sp.normal_z;
            t.Distance = (float)sp.Distance;
        }
        return out;
    }
};

// static.cpp:8-21
inline void point_segment(CloudPtr src_cloud, std::vector<PlanSegment>& Segment, uint64_t seed = 0) {
    const double radius = 0.15, cosfa_t = 0.940, distance_t = 0.5, radius_in_growning = 0.2;
    const float pr = 0.99f, epi = 0.5f;
    CalculateFeature Feature;
    std::shared_ptr<LAS_POINT_PROPERTY> PointProperty = Feature.calculate_plan_parameter_rpca(src_cloud, radius, pr,
                                                                                               epi, seed);
    TreeExtration Tree;
    Segment = Tree.region_growning(PointProperty, src_cloud, distance_t, radius_in_growning, cosfa_t);
}
// static.cpp:24-36
inline void tree_filter(CloudPtr src_cloud, CloudPtr dst_cloud) {
    std::vector<PlanSegment> Segment;
    point_segment(src_cloud, Segment);
    for (const PlanSegment& s : Segment)
        if (s.PointID.size() > 50)
            for (int j : s.PointID) dst_cloud->push_back(src_cloud->points[j]);
}
// static.cpp:37-52
inline void shaft_filter(CloudPtr src_cloud, CloudPtr dst_cloud) {
    std::vector<PlanSegment> Segment;
    point_segment(src_cloud, Segment);
    Cloud tmp;
    for (const PlanSegment& s : Segment)
        if (std::abs(s.normal_z) < 0.30)
            for (int j : s.PointID) tmp.push_back(src_cloud->points[j]);
    *dst_cloud = tmp;
}
// static.cpp:55-79
inline void ground_filter(CloudPtr src_cloud, CloudPtr dst_cloud) {
    std::vector<PlanSegment> Segment;
    point_segment(src_cloud, Segment);
    std::vector<uint8_t> ground(src_cloud->points.size(), 0);
    for (const PlanSegment& s : Segment)
        if (std::abs(s.normal_z) > 0.9)
            for (int j : s.PointID) ground[j] = 1;
    for (size_t k = 0; k < src_cloud->points.size(); k++)
        if (!ground[k]) dst_cloud->push_back(src_cloud->points[k]);
}

// ------------------------------------------------------------------ I4: CloudStampRot
class CloudStampRot {  // cloud_stamp_rot.h:7-39 (pose record; composition stays on the host)
public:
    CloudStampRot() : _rot(Mat4d::Identity()) {}
    explicit CloudStampRot(bool) : _rot(Mat4d::Identity()), _is_valid(false) {}
    CloudStampRot(uint64_t stamp, const Mat4d& rot, CloudPtr cloud_line, double value_icp)
        : _stamp(stamp), _rot(rot), _cloud_line(cloud_line), _cloud_line_src(new Cloud(*cloud_line)),
          _is_valid(true), _value_icp(value_icp) {}
    uint64_t _stamp = 0;
    Mat4d _rot;
    CloudPtr _cloud_line;
    CloudPtr _cloud_line_src;
    bool _is_valid = false;
    double _value_icp = 0.0;
    double _time_stamp_d = 0.0;
    std::string _time_stamp_str;
};

// ------------------------------------------------------------------ CloudGrid (map cache)
// cloud_grid.h:37-88: the reference's singleton over a boost hash map of 1 m cells; here the
// cells and their de-duplicated points live on the device (pcp_grid_*, cloudgrid.hip) and the
// members below stage clouds through the C-ABI.  Output clouds are filled in the reference's
// order (get_grid_cloud(CloudPtr&): cell key order instead of the hash map's).
class CloudGrid {
public:
    static const int MAX_DIS = 60;
    static CloudGrid& instance() {
        static CloudGrid g;
        return g;
    }
    void clear() { detail::check(pcp_grid_clear(ctx(), g_), ctx(), "CloudGrid::clear"); }
    void add_cloud_internal(CloudPtr newpoint) {  // cloud_grid.cpp:34-78
        std::lock_guard<std::mutex> lk(detail::Device::get().mutex());
        const size_t n = newpoint->points.size();
        detail::DevBuf in;
        in.upload(newpoint->points.data(), n * sizeof(PointXYZRGBA));
        detail::check(pcp_grid_add_cloud(ctx(), g_, in.ptr(), (int64_t)n), ctx(), "CloudGrid::add_cloud_internal");
    }
    template <class M>
    void get_cloud_with_pos(CloudPtr& cloud_cache, const M& cur_rot, int dis = MAX_DIS) {  // :84-108
        const int irow = (int)(float)cur_rot(0, 3), icol = (int)(float)cur_rot(1, 3);  // Matrix4f entries
        box(cloud_cache, irow - dis, irow + dis, icol - dis, icol + dis);
    }
    void get_cloud_with_pos(CloudPtr& cloud_cache, const PointXYZRGBA& min_xyz, const PointXYZRGBA& max_xyz) {
        // for (int i = min_xyz.x; i < max_xyz.x; i++) (:118-119)
        box(cloud_cache, (int)min_xyz.x, (int)std::ceil(max_xyz.x), (int)min_xyz.y, (int)std::ceil(max_xyz.y));
    }
    void get_grid_cloud(CloudPtr& cloud) {  // :150-158
        std::lock_guard<std::mutex> lk(detail::Device::get().mutex());
        int64_t n = pcp_grid_size(g_);
        detail::DevBuf out;
        out.reserve((size_t)n * sizeof(PointXYZRGBA));
        detail::check(pcp_grid_points(ctx(), g_, out.ptr(), n, &n), ctx(), "CloudGrid::get_grid_cloud");
        cloud->points.resize((size_t)n);
        out.download(cloud->points.data(), (size_t)n * sizeof(PointXYZRGBA));
    }
    void get_grid_cloud(CloudPtr src_cloud, CloudPtr src_cloud_out, CloudPtr dst_cloud, float dis_threshold) {
        std::lock_guard<std::mutex> lk(detail::Device::get().mutex());  // :160-216
        const size_t n = src_cloud->points.size();
        const int64_t cap = pcp_grid_size(g_);
        detail::DevBuf in, so, dst;
        in.upload(src_cloud->points.data(), n * sizeof(PointXYZRGBA));
        so.reserve(n * sizeof(PointXYZRGBA));
        dst.reserve((size_t)cap * sizeof(PointXYZRGBA));
        int64_t ns = 0, nd = 0;
        detail::check(pcp_grid_match(ctx(), g_, in.ptr(), (int64_t)n, dis_threshold, so.ptr(), &ns, dst.ptr(), cap, &nd),
                      ctx(), "CloudGrid::get_grid_cloud");
        dst_cloud->points.resize((size_t)nd);
        dst.download(dst_cloud->points.data(), (size_t)nd * sizeof(PointXYZRGBA));
        std::vector<PointXYZRGBA> tmp((size_t)ns);
        so.download(tmp.data(), (size_t)ns * sizeof(PointXYZRGBA));
        src_cloud_out->points.swap(tmp);
    }
    ~CloudGrid() { pcp_grid_destroy(g_); }

private:
    CloudGrid() { detail::check(pcp_grid_create(ctx(), &g_), ctx(), "CloudGrid"); }
    static pcp_ctx* ctx() { return detail::Device::get().ctx(); }
    void box(CloudPtr& cache, int i0, int i1, int j0, int j1) {
        std::lock_guard<std::mutex> lk(detail::Device::get().mutex());
        int64_t n = 0;
        detail::check(pcp_grid_box(ctx(), g_, i0, i1, j0, j1, nullptr, 0, &n), ctx(), "CloudGrid::get_cloud_with_pos");
        detail::DevBuf out;
        out.reserve((size_t)n * sizeof(PointXYZRGBA));
        if (n) detail::check(pcp_grid_box(ctx(), g_, i0, i1, j0, j1, out.ptr(), n, &n), ctx(), "CloudGrid::box");
        cache->points.resize((size_t)n);
        out.download(cache->points.data(), (size_t)n * sizeof(PointXYZRGBA));
    }
    pcp_grid* g_ = nullptr;
};

// ------------------------------------------------------------------ PCD I/O (pcd_helper.h)
namespace io {
// io::loadPCDFile (pcd_helper.h:1374-1378): ascii / binary / binary_compressed; 0 or -1.
// width / height come from the header and is_dense is set as PCDReader sets it
// (pcd_helper.cpp:863, 1124-1179: false when a binary field value is non-finite).
inline int loadPCDFile(const std::string& file_name, Cloud& cloud) {
    int64_t n = 0, w = 0, h = 0;
    int dense = 1;
    if (pcp_pcd_read_ex(file_name.c_str(), nullptr, 0, &n, nullptr, nullptr, nullptr) != PCP_OK) return -1;
    cloud.points.resize((size_t)n);
    if (pcp_pcd_read_ex(file_name.c_str(), cloud.points.data(), n, &n, &w, &h, &dense) != PCP_OK) return -1;
    cloud.width = (uint32_t)w;
    cloud.height = (uint32_t)h;
    cloud.is_dense = dense != 0;
    return 0;
}
// io::savePCDFile(binary_mode = true) / savePCDFileBinary -> writeBinary (:489-610); the
// reference throws IOException on an empty cloud or an I/O error
inline int savePCDFileBinary(const std::string& file_name, const Cloud& cloud) {
    const int rc = pcp_pcd_write(file_name.c_str(), cloud.points.data(), (int64_t)cloud.points.size(), 0, 0, 0);
    if (rc != PCP_OK) throw PCLException("[pcl::PCDWriter::writeBinary] " + file_name);
    return 0;
}
inline int savePCDFile(const std::string& file_name, const Cloud& cloud, bool binary_mode = true) {
    if (!binary_mode) throw PCLException("savePCDFile: ASCII output is not provided by this build");
    return savePCDFileBinary(file_name, cloud);
}
// PCDWriter::writeBinaryCompressed (:628-790)
inline int savePCDFileBinaryCompressed(const std::string& file_name, const Cloud& cloud) {
    const int rc = pcp_pcd_write(file_name.c_str(), cloud.points.data(), (int64_t)cloud.points.size(), 0, 0, 1);
    if (rc != PCP_OK) throw PCLException("[pcl::PCDWriter::writeBinaryCompressed] " + file_name);
    return 0;
}
}  // namespace io

// ------------------------------------------------------------------ find_reliable
class Rot {  // main_blend.cpp:282-297
public:
    int ID;
    Mat4d _matrix;
    uint64_t TimeStamp;
    int _const100;
    double icperr;
    bool is_valid;
    Rot(int id, const Mat4d& mat, uint64_t timestamp, double icp_value)
        : ID(id), _matrix(mat), TimeStamp(timestamp), _const100(100), icperr(icp_value), is_valid(false) {}
};

// find_cloud_nearest_point_in_kdtree (main_blend.cpp:306-325): the per-point loop as one
// batched nearest search with a single MIN reduction (pcp_nearest_query)
inline CloudItem find_cloud_nearest_point_in_kdtree(CloudPtr cloud, KdTreeFLANN<CloudItem>& kdtree) {
    return kdtree.nearestQuery(*cloud);
}

// find_reliable (main_blend.cpp:327-380): frames whose neighbours' closest points agree
inline void find_reliable(std::vector<Rot>& rots, std::string cloud_files_dir, float icp_threshold) {
    const float dis_threshold = 0.06f;
    auto path = [&](uint64_t st) { return cloud_files_dir + "/" + std::to_string(st) + ".pcd"; };
    auto xform = [](const Mat4d& m, const CloudItem& p, double o[4]) {
        const double v[4] = {p.x, p.y, p.z, p.data[3]};
        for (int r = 0; r < 4; r++) o[r] = m(r, 0) * v[0] + m(r, 1) * v[1] + m(r, 2) * v[2] + m(r, 3) * v[3];
    };
    for (int i = 1; i + 1 < (int)rots.size(); i++) {
        if (!(rots[i].icperr >= 0 && rots[i].icperr <= icp_threshold && rots[i - 1].icperr >= 0 && rots[i + 1].icperr >= 0))
            continue;
        CloudPtr left(new Cloud), right(new Cloud), centra(new Cloud);
        io::loadPCDFile(path(rots[i - 1].TimeStamp), *left);
        io::loadPCDFile(path(rots[i + 1].TimeStamp), *right);
        io::loadPCDFile(path(rots[i].TimeStamp), *centra);
        KdTreeFLANN<CloudItem> kdtree;
        kdtree.setInputCloud(centra);
        double a[4], b[4];
        const CloudItem lp = find_cloud_nearest_point_in_kdtree(left, kdtree);
        xform(rots[i - 1]._matrix, lp, a);
        xform(rots[i]._matrix, lp, b);
        const double dis_left = std::pow(a[0] - b[0], 2) + std::pow(a[1] - b[1], 2) + std::pow(a[2] - b[2], 2);
        const CloudItem rp = find_cloud_nearest_point_in_kdtree(right, kdtree);
        xform(rots[i]._matrix, rp, a);
        xform(rots[i + 1]._matrix, rp, b);
        const double dis_right = std::pow(a[0] - b[0], 2) + std::pow(a[1] - b[1], 2) + std::pow(a[2] - b[2], 2);
        if (dis_left < dis_threshold && dis_right < dis_threshold) rots[i].is_valid = true;
    }
}

// PointCloudHelper::change_cloud_rgb (point_cloud_helper.cpp:178-186)
inline void change_cloud_rgb(CloudPtr cloud_src, int r, int g, int b) {
    const uint32_t rgb = (uint32_t)r << 16 | (uint32_t)g << 8 | (uint32_t)b;
    for (CloudItem& p : cloud_src->points) p.rgba = rgb;
}

// do_mul_frame_icp (main_blend.cpp:641-931) over the device path: the pose line and the
// threshold the reference reads from g_status are parameters; the map cache is
// CloudGrid::instance().  Frames are loaded in the reference's order (the frames between the two
// ends, then the walk back from start_index and the walk forward from end_index until valid_count
// consecutive frames have 0 < icp value < min_icp_threshold), concatenated, recoloured,
// de-duplicated (4 cm) and optionally shaft-filtered; the map cache around them (+-30 m box, or
// get_grid_cloud at 1 m) registers them with get_rot_icp(do_scale); with is_do_sep_icp each frame
// is then registered against its own +-3 m box.  Every loaded frame's pose is set in `line`.
inline float do_mul_frame_icp(std::vector<CloudStampRot>& line, double min_icp_threshold,
                              const std::unordered_map<uint64_t, std::string>& stamp_filename_map, int start_index,
                              int end_index, int valid_count, bool is_do_sep_icp, bool is_mul_seg,
                              bool is_shaft_filter) {
    std::vector<uint64_t> stamps;
    std::vector<std::string> files;
    auto take = [&](int i) {
        const auto it = stamp_filename_map.find(line[i]._stamp);
        if (it == stamp_filename_map.end()) return;
        files.push_back(it->second);
        stamps.push_back(line[i]._stamp);
    };
    for (int i = start_index + 1; i < end_index; i++) take(i);
    const int size = (int)line.size();
    int k = 0, l = start_index, last = -1;
    do {  // (:684-712); (size_t)last < size is false for the unset -1
        if (l < 0) break;
        const float v = (float)line[l]._value_icp;
        if (v > 0 && v < min_icp_threshold) {
            k++;
            if (last >= 0 && last < size && last != l + 1) k = 0;
            last = l;
        }
        take(l--);
    } while (k < valid_count);
    k = 0, l = end_index, last = -1;
    do {  // (:717-745)
        if (l >= size) break;
        const float v = (float)line[l]._value_icp;
        if (v > 0 && v < min_icp_threshold) {
            k++;
            if (last >= 0 && last != l - 1) k = 0;
            last = l;
        }
        take(l++);
    } while (k < valid_count);
    std::vector<CloudPtr> clouds(files.size());
    CloudPtr frame(new Cloud);
    for (size_t i = 0; i < files.size(); i++) {
        clouds[i].reset(new Cloud);
        io::loadPCDFile(files[i], *clouds[i]);
        frame->points.insert(frame->points.end(), clouds[i]->points.begin(), clouds[i]->points.end());
        frame->is_dense = frame->is_dense && clouds[i]->is_dense;
    }
    frame->width = (uint32_t)frame->points.size();
    frame->height = 1;
    change_cloud_rgb(frame, 255, 0, 0);
    PointCloudHelper::remove_duplicate(frame, 0.04f);
    if (is_shaft_filter) shaft_filter(frame, frame);
    CloudPtr cache(new Cloud);
    if (!is_mul_seg) {
        CloudItem mn, mx;
        PointCloudHelper::getMinMax3D(*frame, mn, mx);
        const float d = 30;
        mn.x -= d; mn.y -= d; mn.z -= d;
        mx.x += d; mx.y += d; mx.z += d;
        CloudGrid::instance().get_cloud_with_pos(cache, mn, mx);
    } else {
        CloudGrid::instance().get_grid_cloud(frame, frame, cache, 1.0f);
    }
    Mat4d rot = Mat4d::Identity();
    const float dis = PointCloudHelper::get_rot_icp(cache, frame, rot, true, false);
    for (size_t i = 0; i < stamps.size(); i++) {
        Mat4d final_rot = rot;
        if (is_do_sep_icp) {
            CloudPtr moved(new Cloud);
            PointCloudHelper::transformPointCloud(*clouds[i], *moved, rot);
            CloudItem mn, mx;
            PointCloudHelper::getMinMax3D(*moved, mn, mx);
            const float d = 3;
            mn.x -= d; mn.y -= d; mn.z -= d;
            mx.x += d; mx.y += d; mx.z += d;
            CloudPtr cache_t(new Cloud);
            CloudGrid::instance().get_cloud_with_pos(cache_t, mn, mx);
            Mat4d rot_split = Mat4d::Identity();
            if (cache_t->size() > 0) PointCloudHelper::get_rot_icp(cache_t, moved, rot_split, false, false);
            final_rot = rot_split * rot;
        }
        for (CloudStampRot& r : line)  // get_cloud_rot_with_stamp: the first entry of the stamp
            if (r._stamp == stamps[i]) {
                r._rot = final_rot;
                break;
            }
    }
    return dis;
}

// pose lines: the reference's Eigen composition restated in libpcp (pcp_pose_*, host-only)
namespace detail {
inline std::vector<double> pack_rots(const std::vector<CloudStampRot>& r) {
    std::vector<double> a(16 * r.size());
    for (size_t i = 0; i < r.size(); i++) std::memcpy(&a[16 * i], r[i]._rot.m, 16 * sizeof(double));
    return a;
}
inline void unpack_rots(const std::vector<double>& a, std::vector<CloudStampRot>& r) {
    for (size_t i = 0; i < r.size(); i++) std::memcpy(r[i]._rot.m, &a[16 * i], 16 * sizeof(double));
}
}  // namespace detail

// do_transform_interpolation (main_blend.cpp:934-980)
inline void do_transform_interpolation(std::vector<CloudStampRot>& line, int start_index, int end_index) {
    std::vector<double> a = detail::pack_rots(line);
    detail::check(pcp_pose_interpolate(a.data(), (int64_t)line.size(), start_index, end_index), nullptr,
                  "do_transform_interpolation");
    detail::unpack_rots(a, line);
}

class PointCloudClosure {  // point_cloud_closure.cpp:44-276 (the pose-line and overlap members)
public:
    struct same_segment {  // point_cloud_closure.h:15-21
        uint64_t base_start_stamp, base_end_stamp, frame_start_stamp, frame_end_stamp;
    };
    // get_overlap_stamp (:44-180): the per-point radiusSearch(10) loop as one batched search
    static void get_overlap_stamp(const std::vector<CloudStampRot>& rots, std::vector<same_segment>& overlap_segs) {
        auto minus_abs = [](uint64_t a, uint64_t b) { return a > b ? a - b : b - a; };
        typename PointCloud<PointC>::Ptr pts(new PointCloud<PointC>());
        for (size_t i = 0; i + 1 < rots.size(); i++) {
            const double x = rots[i]._rot(0, 3), y = rots[i]._rot(1, 3), z = rots[i]._rot(2, 3);
            const double dx = rots[i + 1]._rot(0, 3) - x, dy = rots[i + 1]._rot(1, 3) - y, dz = rots[i + 1]._rot(2, 3) - z;
            PointC d;
            d.x = x; d.y = y; d.z = z;
            d.stamp = rots[i]._stamp;
            d.angle_z = std::atan2(dy, dx) * 57.29578;  // RAD2DEG (macros.h:15)
            d.distance_sqr = std::pow(dx, 2) + std::pow(dy, 2) + std::pow(dz, 2);
            if (d.angle_z < 0) d.angle_z += 360.0f;
            if (d.distance_sqr <= 0.1) continue;
            pts->push_back(d);
        }
        overlap_segs.clear();
        if (pts->points.empty()) return;
        KdTreeFLANN<PointC> tree;
        tree.setInputCloud(pts);
        std::vector<int64_t> off;
        std::vector<int> idx;
        std::vector<double> d2;
        tree.radiusSearchBatch(pts->points, 10, off, idx, d2);
        std::vector<std::pair<uint64_t, uint64_t>> pairs;
        for (size_t i = 0; i < pts->points.size(); i++) {
            const PointC& cp = pts->points[i];
            for (int64_t t = off[i]; t < off[i + 1]; t++) {
                const PointC& q = pts->points[idx[t]];
                if (q.stamp <= cp.stamp || minus_abs(cp.stamp, q.stamp) < 6000) continue;
                if (std::abs(cp.angle_z - q.angle_z) >= 20.0f) continue;
                double avg = (cp.angle_z + q.angle_z) / 2.0 - 90;
                avg = avg / 180.0 * M_PI;
                const double k = std::tan(avg), b = cp.y - k * cp.x;
                if (std::abs(0 - k * q.x + q.y - b) / std::sqrt(k * k + 1) > 1.5) continue;
                pairs.emplace_back(cp.stamp, q.stamp);
                break;
            }
        }
        if (pairs.empty()) return;
        uint64_t bs = pairs[0].first, fs = pairs[0].second;
        for (size_t i = 1; i < pairs.size(); i++) {
            if (minus_abs(pairs[i].first, pairs[i - 1].first) > 10 || minus_abs(pairs[i].second, pairs[i - 1].second) > 10) {
                overlap_segs.push_back({bs, pairs[i - 1].first, fs, pairs[i - 1].second});
                bs = pairs[i].first;
                fs = pairs[i].second;
            }
        }
        overlap_segs.push_back({bs, pairs.back().first, fs, pairs.back().second});
        for (auto& sg : overlap_segs)
            if (sg.frame_start_stamp > sg.frame_end_stamp) std::swap(sg.frame_start_stamp, sg.frame_end_stamp);
    }
    static int get_index_from_rots(const std::vector<CloudStampRot>& rots, uint64_t stamp) {
        for (size_t i = 0; i < rots.size(); i++)
            if (rots[i]._stamp == stamp) return (int)i;
        return -1;
    }
    template <class M>
    static bool do_lum_elch(std::vector<CloudStampRot>& rots, int start_index, int end_index, const M& loop_transform) {
        double L[16];
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) L[4 * r + c] = loop_transform(r, c);
        std::vector<double> a = detail::pack_rots(rots);
        if (pcp_pose_lum_elch(a.data(), (int64_t)rots.size(), start_index, end_index, L) != PCP_OK) return false;
        detail::unpack_rots(a, rots);
        return true;
    }
    static bool do_loop_closure(std::vector<CloudStampRot>& ori_rots, const std::vector<CloudStampRot>& opt_rots) {
        if (opt_rots.empty()) return false;
        std::vector<double> a = detail::pack_rots(ori_rots), b = detail::pack_rots(opt_rots);
        std::vector<uint64_t> sa(ori_rots.size()), sb(opt_rots.size());
        for (size_t i = 0; i < ori_rots.size(); i++) sa[i] = ori_rots[i]._stamp;
        for (size_t i = 0; i < opt_rots.size(); i++) sb[i] = opt_rots[i]._stamp;
        if (pcp_pose_loop_closure(a.data(), sa.data(), (int64_t)sa.size(), b.data(), sb.data(), (int64_t)sb.size(),
                                  400) != PCP_OK)
            return false;  // "cannot find stamp in rots" / "rots count not equal"
        detail::unpack_rots(a, ori_rots);
        return true;
    }
};

}  // namespace cloud_blend_double

#endif  // PCP_PCL_HPP
