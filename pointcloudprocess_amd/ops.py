"""Python host layer over the C-ABI (include/pcp.h) for device-resident clouds.

torch is plumbing only: it owns device memory and the stream; every computation is a
libpcp HIP kernel.  Clouds in the reference layout (PointXYZRGBA, point_type.h:9-82) are
uint8 tensors of shape (n, 48); xyz clouds are float64/float32 tensors of shape (n, 3).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check

POINT48 = np.dtype(
    [("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("w", "<f8"), ("rgba", "<u4"),
     ("stamp_id", "<u4"), ("pad", "<u4", (2,))])
PLANE = np.dtype([("normal_x", "<f4"), ("normal_y", "<f4"), ("normal_z", "<f4"),
                  ("min_value", "<f4"), ("curvature", "<f4"), ("distance", "<f4")])


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Context:
    """pcp_ctx bound to a device and to torch's current stream on that device."""

    def __init__(self, device=0):
        self.lib = _lib.load()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        idx = self.device.index or 0
        stream = torch.cuda.current_stream(self.device).cuda_stream
        h = C.c_void_p()
        rc = self.lib.pcp_ctx_create(idx, C.c_void_p(stream), C.byref(h))
        if rc != 0:
            raise _lib.PcpError(rc, f"pcp_ctx_create(device={idx}) failed")
        self.h = h

    def check(self, rc):
        return check(rc, self.h)

    def sync(self):
        self.check(self.lib.pcp_sync(self.h))

    def alloc_stats(self):
        """(blocks handed out, their bytes, peak bytes, hipMalloc calls) of the internal allocator."""
        out = (C.c_int64 * 4)()
        self.check(self.lib.pcp_ctx_alloc_stats(self.h, out))
        return tuple(out)

    def close(self):
        if getattr(self, "h", None):
            self.lib.pcp_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def cloud_to_device(cloud_np, device):
    """numpy POINT48 structured array -> (n, 48) uint8 device tensor."""
    arr = np.ascontiguousarray(cloud_np)
    assert arr.dtype.itemsize == 48
    t = torch.from_numpy(arr.view(np.uint8).reshape(len(arr), 48))
    return t.to(device)


def cloud_to_host(t):
    a = t.detach().cpu().contiguous().numpy().reshape(-1)
    return a.view(POINT48)


class GridIndex:
    """pcp_index over a cloud.  fp64 (KdTreeFLANN contract) or fp32 (ICP target)."""

    def __init__(self, ctx, xyz, cell_size=0.0, indices=None, stride_bytes=None):
        self.ctx = ctx
        lib = ctx.lib
        self.src = xyz  # keep alive
        h = C.c_void_p()
        n = xyz.shape[0]
        if xyz.dtype == torch.uint8:  # AoS48
            stride = 48
            self.f64 = True
        else:
            self.f64 = xyz.dtype == torch.float64
            stride = stride_bytes or xyz.stride(0) * xyz.element_size()
        if self.f64:
            self.indices = None if indices is None else indices.to(ctx.device, torch.int32).contiguous()
            ni = 0 if self.indices is None else self.indices.numel()
            ctx.check(lib.pcp_index_build_f64(ctx.h, _ptr(xyz), stride, n, _ptr(self.indices), ni,
                                              float(cell_size), C.byref(h)))
        else:
            if indices is not None:
                raise ValueError("fp32 index does not take an indices subset")
            ctx.check(lib.pcp_index_build_f32(ctx.h, _ptr(xyz), stride, n, float(cell_size), C.byref(h)))
        self.h = h

    @property
    def size(self):
        return self.ctx.lib.pcp_index_size(self.h)

    @property
    def cell_size(self):
        return self.ctx.lib.pcp_index_cell_size(self.h)

    @property
    def identity_mapping(self):
        return bool(self.ctx.lib.pcp_index_identity_mapping(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.pcp_index_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def _qstride(q):
    if q.dtype == torch.uint8:
        return 48
    return q.stride(0) * q.element_size()


def knn(index, q, k):
    """Batch nearestKSearch: (nq, k) int32 indices and float64 sqr distances."""
    ctx = index.ctx
    nq = q.shape[0]
    idx = torch.empty((nq, k), dtype=torch.int32, device=ctx.device)
    d2 = torch.empty((nq, k), dtype=torch.float64, device=ctx.device)
    ctx.check(ctx.lib.pcp_knn(ctx.h, index.h, _ptr(q), _qstride(q), nq, int(k), _ptr(idx), _ptr(d2)))
    return idx, d2


def knn_last_far(ctx):
    """Queries of the last knn (or nearest_query) on ctx that the near pass deferred to the
    exact wave-per-query pass; 0 when the call returned before searching.  Waits for the
    stream (diagnostic)."""
    n = C.c_int64()
    ctx.check(ctx.lib.pcp_knn_last_far(ctx.h, C.byref(n)))
    return n.value


def radius(index, q, r, max_nn=0):
    """Batch radiusSearch -> CSR (offsets int64 (nq+1), idx int32, d2 float64)."""
    ctx = index.ctx
    nq = q.shape[0]
    cnt = torch.empty(nq, dtype=torch.int32, device=ctx.device)
    ctx.check(ctx.lib.pcp_radius_count(ctx.h, index.h, _ptr(q), _qstride(q), nq, float(r), int(max_nn),
                                       _ptr(cnt)))
    offs = torch.empty(nq + 1, dtype=torch.int64, device=ctx.device)
    total = C.c_int64()
    ctx.check(ctx.lib.pcp_scan_counts(ctx.h, _ptr(cnt), nq, _ptr(offs), C.byref(total)))
    idx = torch.empty(max(total.value, 1), dtype=torch.int32, device=ctx.device)
    d2 = torch.empty(max(total.value, 1), dtype=torch.float64, device=ctx.device)
    ctx.check(ctx.lib.pcp_radius_fill(ctx.h, index.h, _ptr(q), _qstride(q), nq, float(r), int(max_nn),
                                      _ptr(offs), _ptr(idx), _ptr(d2)))
    return offs, idx[:total.value], d2[:total.value]


class H16Index:
    """C5 fp16 cell-relative index over an (n, 3) fp32 cloud (pcp_index_build_h16)."""

    def __init__(self, ctx, xyz, cell_size):
        self.ctx = ctx
        self.src = xyz
        h = C.c_void_p()
        ctx.check(ctx.lib.pcp_index_build_h16(ctx.h, _ptr(xyz), xyz.stride(0) * xyz.element_size(), xyz.shape[0],
                                              float(cell_size), C.byref(h)))
        self.h = h

    def radius_normals(self, r, n_owned=None, global_id=None, normals=True):
        """Rows (offsets int64 (n_owned+1), idx int32) of the owned points + their planes."""
        ctx = self.ctx
        n_owned = self.src.shape[0] if n_owned is None else int(n_owned)
        cnt = torch.empty(max(n_owned, 1), dtype=torch.int32, device=ctx.device)
        ctx.check(ctx.lib.pcp_h16_radius_count(ctx.h, self.h, float(r), n_owned, _ptr(cnt)))
        offs = torch.empty(n_owned + 1, dtype=torch.int64, device=ctx.device)
        total = C.c_int64()
        ctx.check(ctx.lib.pcp_scan_counts(ctx.h, _ptr(cnt), n_owned, _ptr(offs), C.byref(total)))
        idx = torch.empty(max(total.value, 1), dtype=torch.int32, device=ctx.device)
        nrm = torch.empty((max(n_owned, 1), 6), dtype=torch.float32, device=ctx.device) if normals else None
        ctx.check(ctx.lib.pcp_h16_radius_fill(ctx.h, self.h, float(r), n_owned, _ptr(offs), _ptr(global_id),
                                              _ptr(idx), _ptr(nrm)))
        return offs, idx[:total.value], (nrm[:n_owned] if normals else None)

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.pcp_index_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def nearest_query(index, q, init_bound=9999.0):
    """find_cloud_nearest_point_in_kdtree: (query index or -1, its 1-NN d2)."""
    ctx = index.ctx
    bq, bd = C.c_int64(), C.c_double()
    ctx.check(ctx.lib.pcp_nearest_query(ctx.h, index.h, _ptr(q), _qstride(q), q.shape[0], float(init_bound),
                                        C.byref(bq), C.byref(bd)))
    return bq.value, bd.value


def plane_fit_segments(ctx, xyz, offsets, idx=None):
    """One PlanSegment per CSR segment of xyz rows (F1 per segment)."""
    nseg = offsets.numel() - 1
    out = torch.empty((max(nseg, 1), 6), dtype=torch.float32, device=ctx.device)
    ctx.check(ctx.lib.pcp_plane_fit_segments(ctx.h, _ptr(xyz), _qstride(xyz), _ptr(offsets), _ptr(idx), nseg,
                                             _ptr(out)))
    return out[:nseg]


def normals_radius(index, r, max_nn=0):
    """calculate_plan_parameter(cloud, radius) (calculate_feature.h:15, declared-only in the
    reference; the build defines it as F1 over each point's radiusSearch neighbourhood)."""
    xyz = index.src
    offs, idx, _ = radius(index, xyz, r, max_nn)
    return plane_fit_segments(index.ctx, xyz, offs, idx)


def knn_bruteforce(ctx, target, q, k):
    nt, nq = target.shape[0], q.shape[0]
    idx = torch.empty((nq, k), dtype=torch.int32, device=ctx.device)
    d2 = torch.empty((nq, k), dtype=torch.float64, device=ctx.device)
    ctx.check(ctx.lib.pcp_knn_bruteforce(ctx.h, _ptr(target), _qstride(target), nt, _ptr(q), _qstride(q),
                                         nq, int(k), _ptr(idx), _ptr(d2)))
    return idx, d2


def knn_bruteforce_last_fallback(ctx):
    n = C.c_int64()
    ctx.check(ctx.lib.pcp_knn_bruteforce_last_fallback(ctx.h, C.byref(n)))
    return n.value


def knn_lod(ctx, cloud, q, k):
    nq = q.shape[0]
    idx = torch.empty((nq, k), dtype=torch.int32, device=ctx.device)
    d2 = torch.empty((nq, k), dtype=torch.float64, device=ctx.device)
    ctx.check(ctx.lib.pcp_knn_lod(ctx.h, _ptr(cloud), cloud.shape[0], _ptr(q), nq, int(k), _ptr(idx),
                                  _ptr(d2)))
    return idx, d2


def minmax(ctx, cloud, is_dense=True):
    mn, mx = (C.c_double * 4)(), (C.c_double * 4)()
    ctx.check(ctx.lib.pcp_minmax_aos48(ctx.h, _ptr(cloud), cloud.shape[0], int(is_dense), mn, mx))
    return np.array(mn[:]), np.array(mx[:])


def _seg_args(seg_offsets, T):
    """(offsets array, nseg, poses array or None) of a span of segments with one 4x4 each (one 4x4
    for all, or B of them)."""
    off = [int(v) for v in seg_offsets]
    if not off:
        raise ValueError("seg_offsets needs at least one entry")
    B = len(off) - 1
    Tm = None
    if T is not None:
        T = np.asarray(T, dtype=np.float64)
        T = np.broadcast_to(T.reshape(1, 16), (B, 16)) if T.size == 16 else T.reshape(B, 16)
        Tm = (C.c_double * (16 * B))(*np.ascontiguousarray(T).reshape(-1))
    return (C.c_int64 * len(off))(*off), B, Tm


def minmax_segments(ctx, cloud, seg_offsets, T=None, is_dense=True):
    """(mn, mx), each (B, 4): row s is minmax(transform(cloud[off[s]:off[s + 1]], T[s])) bit for bit,
    in one pass with no moved copy and one host synchronisation whatever B is (pcp.h V).  T: None
    (the identity), one 4x4 for all segments, or B of them."""
    off, B, Tm = _seg_args(seg_offsets, T)
    mn, mx = (C.c_double * (4 * B))(), (C.c_double * (4 * B))()
    n = cloud.shape[0]
    ctx.check(ctx.lib.pcp_minmax_segments_aos48(ctx.h, _ptr(cloud) if n else None, n, off, B, int(is_dense), Tm,
                                                mn, mx))
    return np.array(mn[:]).reshape(B, 4), np.array(mx[:]).reshape(B, 4)


def centroid(ctx, cloud, is_dense=True):
    c = (C.c_double * 4)()
    cnt = C.c_uint32()
    ctx.check(ctx.lib.pcp_centroid_aos48(ctx.h, _ptr(cloud), cloud.shape[0], int(is_dense), c,
                                         C.byref(cnt)))
    return np.array(c[:]), cnt.value


def centroid_concat(ctx, a, b, is_dense=True):
    """compute3DCentroid of a ++ b (the joint centroid of get_rot_icp)."""
    c = (C.c_double * 4)()
    cnt = C.c_uint32()
    ctx.check(ctx.lib.pcp_centroid_concat_aos48(ctx.h, _ptr(a), a.shape[0], _ptr(b), b.shape[0], int(is_dense),
                                                c, C.byref(cnt)))
    return np.array(c[:]), cnt.value


def transform(ctx, cloud, T, is_dense=True, out=None):
    out = torch.empty_like(cloud) if out is None else out
    Tm = _lib.f64arr(np.asarray(T, dtype=np.float64).reshape(16))
    ctx.check(ctx.lib.pcp_transform_aos48(ctx.h, _ptr(cloud), _ptr(out), cloud.shape[0], int(is_dense), Tm))
    return out


def voxel_filter(ctx, cloud, leaf, is_dense=True, downsample_all=True, with_voxel_idx=False):
    n = cloud.shape[0]
    out = torch.empty((max(n, 1), 48), dtype=torch.uint8, device=ctx.device)
    vidx = torch.empty(max(n, 1), dtype=torch.int32, device=ctx.device) if with_voxel_idx else None
    lf = (leaf, leaf, leaf) if np.isscalar(leaf) else tuple(leaf)
    nout = C.c_int64()
    ctx.check(ctx.lib.pcp_voxel_filter(ctx.h, _ptr(cloud), n, int(is_dense), _lib.f64arr(lf),
                                       int(downsample_all), _ptr(out), C.byref(nout), _ptr(vidx)))
    m = nout.value
    if with_voxel_idx:
        return out[:m], vidx[:m].view(torch.int32)
    return out[:m]


def remove_duplicate(ctx, cloud, leaf, is_dense=True):
    n = cloud.shape[0]
    out = torch.empty((max(n, 1), 48), dtype=torch.uint8, device=ctx.device)
    nout = C.c_int64()
    ctx.check(ctx.lib.pcp_remove_duplicate(ctx.h, _ptr(cloud), n, int(is_dense), float(leaf), _ptr(out),
                                           C.byref(nout)))
    return out[:nout.value]


def normals_knn(index, k):
    ctx = index.ctx
    n_out = index.src.shape[0]  # outputs are indexed by the caller's cloud index
    out = torch.empty((max(n_out, 1), 6), dtype=torch.float32, device=ctx.device)
    ctx.check(ctx.lib.pcp_normals_knn(ctx.h, index.h, int(k), _ptr(out), n_out))
    return out[:n_out]


def normals_knn_last_deferred(ctx):
    """(tile_deferred, far_queries) of the last normals_knn on ctx: the queries the tile pass
    handed on (-1 on a sparse grid, where no tile runs) and those the exact wave-per-query
    pass answered.  Waits for the stream (diagnostic)."""
    t, f = C.c_int64(), C.c_int64()
    ctx.check(ctx.lib.pcp_normals_knn_last_deferred(ctx.h, C.byref(t), C.byref(f)))
    return t.value, f.value


POINT_PROPERTY = np.dtype([("normal_x", "<f4"), ("normal_y", "<f4"), ("normal_z", "<f4"), ("pad", "<u4"),
                           ("distance", "<f8"), ("curvature", "<f8"), ("point_id", "<i4"),
                           ("segment_id", "<i4"), ("dis_from_point_plane", "<f4"), ("pad2", "<u4")])


def normals_rpca(ctx, xyz, knn_idx, pr=0.99, epi=0.5, seed=0):
    """F3 robust normals (calculate_plan_parameter_rpca) from the cloud's kNN(20) rows;
    returns a (n, 48) uint8 device tensor of LAS_POINT_PROPERTY records."""
    n = xyz.shape[0]
    k = knn_idx.shape[1]
    out = torch.empty((max(n, 1), 48), dtype=torch.uint8, device=ctx.device)
    ctx.check(ctx.lib.pcp_normals_rpca(ctx.h, _ptr(xyz), xyz.stride(0) * xyz.element_size(), n,
                                       _ptr(knn_idx.contiguous()), int(k), float(pr), float(epi),
                                       int(seed), _ptr(out)))
    return out[:n]


class ICP:
    """Device-resident ICP of a query set against an fp32 grid index (the target)."""

    def __init__(self, target_index, q, _handle=None):
        self.index = target_index
        self.ctx = ctx = target_index.ctx
        self.q = q
        h = C.c_void_p()
        if _handle is None:
            ctx.check(ctx.lib.pcp_icp_create(ctx.h, target_index.h, _ptr(q), q.stride(0) * q.element_size(),
                                             q.shape[0], C.byref(h)))
        else:
            h = _handle
        self.h = h
        self.nq_in = q.shape[0]
        self.acc = torch.zeros(24, dtype=torch.float64, device=ctx.device)

    @classmethod
    def with_target(cls, ctx, target, q, cell_size):
        """The fp32 index of `target` and the ICP handle of `q` in one call
        (pcp_icp_create_with_target: the two pre-iteration sorts overlap).  Returns the ICP; its
        .index is the GridIndex (close the ICP, then the index)."""
        hi, hq = C.c_void_p(), C.c_void_p()
        ctx.check(ctx.lib.pcp_icp_create_with_target(ctx.h, _ptr(target), target.stride(0) * target.element_size(),
                                                     target.shape[0], float(cell_size), _ptr(q),
                                                     q.stride(0) * q.element_size(), q.shape[0], C.byref(hi),
                                                     C.byref(hq)))
        index = GridIndex.__new__(GridIndex)
        index.ctx, index.src, index.h, index.f64, index.indices = ctx, target, hi, False, None
        return cls(index, q, _handle=hq)

    WIDE_CACHE = 128  # PCP_ICP_OPT_WIDE_CACHE
    GRAPH = 256       # PCP_ICP_OPT_GRAPH
    NO_LOOKAHEAD = 512  # PCP_ICP_OPT_NO_LOOKAHEAD
    NO_PILOT = 1024     # PCP_ICP_OPT_NO_PILOT
    PILOT_ALWAYS = 2048  # PCP_ICP_OPT_PILOT_ALWAYS

    def set_options(self, oct_lanes_first=1, oct_lanes_list=0, ring_lanes=0, ablate=0, wide_cache=False,
                    graph=False, lookahead=True, pilot=None):
        """Test / profiling controls (pcp_icp_set_options): lanes per query of the octant pass
        (first launch, later lists; 0 = by density) and of the fallback pass (0 = by length);
        `ablate` switches passes off (results are then wrong); `wide_cache` keeps 16-byte cache
        records (before the first step); `graph` replays one captured HIP graph per device-pose
        launch; `lookahead=False` searches around the query itself instead of ahead on its path
        (results are identical in all three cases); `pilot`: the pilot step before the first launch,
        None = by the handle's size, True = always, False = never (results are identical)."""
        flags = (int(ablate) | (self.WIDE_CACHE if wide_cache else 0) | (self.GRAPH if graph else 0) |
                 (0 if lookahead else self.NO_LOOKAHEAD) |
                 (0 if pilot is None else (self.PILOT_ALWAYS if pilot else self.NO_PILOT)))
        self.ctx.check(self.ctx.lib.pcp_icp_set_options(self.h, int(oct_lanes_first), int(oct_lanes_list),
                                                        int(ring_lanes), flags))

    def step(self, T, rmax, corr=False):
        """One iteration at pose T; returns the (device) accumulators (+ correspondences)."""
        ctx = self.ctx
        Tm = _lib.f64arr(np.asarray(T, dtype=np.float64).reshape(16))
        ci = cd = None
        if corr:
            ci = torch.empty(self.q.shape[0], dtype=torch.int32, device=ctx.device)
            cd = torch.empty(self.q.shape[0], dtype=torch.float32, device=ctx.device)
        ctx.check(ctx.lib.pcp_icp_step(ctx.h, self.h, Tm, float(rmax), _ptr(self.acc), _ptr(ci), _ptr(cd)))
        return (self.acc, ci, cd) if corr else self.acc

    def run(self, T0, rmax, iters, do_scale=False, eps=0.0):
        ctx = self.ctx
        T = _lib.f64arr(np.asarray(T0, dtype=np.float64).reshape(16))
        err = C.c_float()
        rc = ctx.lib.pcp_icp_run(ctx.h, self.h, T, float(rmax), int(iters), int(do_scale), float(eps),
                                 C.byref(err))
        if rc not in (0, -6):
            ctx.check(rc)
        return float(err.value), np.array(T[:]).reshape(4, 4)

    # ---- device-resident loop: the pose stays in HBM, no host round trip per iteration
    def new_pose(self, T0=None):
        """(T_dev, stats_dev): a device pose (16 fp64, row-major) and zeroed stats (4 fp64)."""
        T = torch.as_tensor(np.eye(4) if T0 is None else np.asarray(T0, dtype=np.float64), dtype=torch.float64)
        return T.reshape(16).to(self.ctx.device).contiguous(), torch.zeros(4, dtype=torch.float64,
                                                                        device=self.ctx.device)

    def step_dev(self, T_dev, rmax):
        ctx = self.ctx
        ctx.check(ctx.lib.pcp_icp_step_dev(ctx.h, self.h, _ptr(T_dev), float(rmax), _ptr(self.acc)))
        return self.acc

    def solve_dev(self, acc, T_dev, stats, do_scale=False):
        ctx = self.ctx
        ctx.check(ctx.lib.pcp_icp_solve_dev(ctx.h, _ptr(acc), int(do_scale), _ptr(T_dev), _ptr(stats)))

    def run_dev(self, T_dev, stats, rmax, iters, do_scale=False):
        ctx = self.ctx
        ctx.check(ctx.lib.pcp_icp_run_dev(ctx.h, self.h, _ptr(T_dev), float(rmax), int(iters), int(do_scale),
                                          _ptr(stats)))

    # ---- point-to-plane loop (pcp.h I2: the build's own contract, not trimesh2's)
    def solve_plane_dev(self, acc, T_dev, stats):
        """Device 6x6 solve of the 30 plane accumulators: T_dev <- dT * T_dev, stats =
        [status, RMS point distance, RMS plane distance, iterations solved]."""
        ctx = self.ctx
        assert acc.dtype == torch.float64 and acc.numel() >= 30
        ctx.check(ctx.lib.pcp_icp_solve_plane_dev(ctx.h, _ptr(acc), _ptr(T_dev), _ptr(stats)))

    def run_plane_dev(self, planes, q, T_dev, stats, rmax, iters):
        """iters x (keys_dev, icp_accumulate_plane, solve_plane_dev) with no host round trip; q:
        the handle's queries in their original order (n x 3 fp32)."""
        ctx = self.ctx
        n = q.shape[0]
        ctx.check(ctx.lib.pcp_icp_run_plane_dev(ctx.h, self.h, planes.h, _ptr(q) if n else None,
                                                q.stride(0) * q.element_size(), n, _ptr(T_dev), float(rmax),
                                                int(iters), _ptr(stats)))

    def run_plane_trimmed_dev(self, planes, q, T_dev, stats, rmax, frac, mult=1.0, d_floor=0.0, iters=4, trim=None):
        """run_plane_dev with icp_trim_keys(frac, mult, d_floor) in place between the keys and the
        accumulation of every iteration (pcp.h I3).  Returns trim: the last iteration's
        [m, kept, sel, bits of cut] (int64 device tensor, 4)."""
        ctx = self.ctx
        n = q.shape[0]
        trim = torch.zeros(4, dtype=torch.int64, device=ctx.device) if trim is None else trim
        assert trim.dtype == torch.int64 and trim.numel() >= 4
        ctx.check(ctx.lib.pcp_icp_run_plane_trimmed_dev(ctx.h, self.h, planes.h, _ptr(q) if n else None,
                                                        q.stride(0) * q.element_size(), n, _ptr(T_dev), float(rmax),
                                                        float(frac), float(mult), float(d_floor), int(iters),
                                                        _ptr(stats), _ptr(trim)))
        return trim

    def run_plane_rtrimmed_dev(self, planes, q, T_dev, stats, rmax, frac, mult=1.0, d_floor=0.0, iters=4, trim=None):
        """run_plane_trimmed_dev with icp_trim_keys_plane in place of icp_trim_keys: every iteration
        trims by the pairs' plane residual at its pose (pcp.h I3b).  Returns trim as there."""
        ctx = self.ctx
        n = q.shape[0]
        trim = torch.zeros(4, dtype=torch.int64, device=ctx.device) if trim is None else trim
        assert trim.dtype == torch.int64 and trim.numel() >= 4
        ctx.check(ctx.lib.pcp_icp_run_plane_rtrimmed_dev(ctx.h, self.h, planes.h, _ptr(q) if n else None,
                                                         q.stride(0) * q.element_size(), n, _ptr(T_dev), float(rmax),
                                                         float(frac), float(mult), float(d_floor), int(iters),
                                                         _ptr(stats), _ptr(trim)))
        return trim

    def kernel_ms(self):
        """(ms, launches) of the device-loop correspondence kernels since the last call."""
        ms, n = C.c_double(), C.c_int()
        self.ctx.check(self.ctx.lib.pcp_icp_kernel_ms(self.ctx.h, self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def keys(self, T, rmax, target_offset=0):
        """Target-sharded mode: per-query int64 keys (fp32 d2 bits << 32 | global target
        index, INT64_MAX = none) in the original query order."""
        ctx = self.ctx
        keys = torch.empty(self.nq_in, dtype=torch.int64, device=ctx.device)
        Tm = _lib.f64arr(np.asarray(T, dtype=np.float64).reshape(16))
        ctx.check(ctx.lib.pcp_icp_keys(ctx.h, self.h, Tm, float(rmax), int(target_offset), _ptr(keys)))
        return keys

    def keys_dev(self, T_dev, rmax, target_offset=0, out=None):
        """keys() at the device pose T_dev (no host round trip)."""
        ctx = self.ctx
        keys = torch.empty(self.nq_in, dtype=torch.int64, device=ctx.device) if out is None else out
        assert keys.dtype == torch.int64 and keys.numel() >= self.nq_in and keys.is_contiguous()
        ctx.check(ctx.lib.pcp_icp_keys_dev(ctx.h, self.h, _ptr(T_dev), float(rmax), int(target_offset), _ptr(keys)))
        return keys

    def accumulate_keys(self, T, keys, lo, hi, shard_xyz):
        """24 accumulators of the queries whose (MIN-reduced) winner is in [lo, hi)."""
        ctx = self.ctx
        Tm = _lib.f64arr(np.asarray(T, dtype=np.float64).reshape(16))
        ctx.check(ctx.lib.pcp_icp_accumulate_keys(ctx.h, self.h, Tm, _ptr(keys), int(lo), int(hi), _ptr(shard_xyz),
                                                  shard_xyz.stride(0) * shard_xyz.element_size(), _ptr(self.acc)))
        return self.acc

    def last_kernel_ms(self):
        ms, n = C.c_double(), C.c_int()
        self.ctx.check(self.ctx.lib.pcp_icp_last_kernel_ms(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def last_searched(self):
        """Queries of the last step the verify pass could not settle (they were searched)."""
        n = C.c_int64()
        self.ctx.check(self.ctx.lib.pcp_icp_last_searched(self.h, C.byref(n)))
        return n.value

    def last_lookahead(self):
        """(beta, largest offset in metres) of the last launch's look-ahead search centre."""
        b, m = C.c_double(), C.c_double()
        self.ctx.check(self.ctx.lib.pcp_icp_last_lookahead(self.h, C.byref(b), C.byref(m)))
        return b.value, m.value

    def last_fallback(self):
        n = C.c_int64()
        self.ctx.check(self.ctx.lib.pcp_icp_last_fallback(self.h, C.byref(n)))
        return n.value

    def predict_first(self, T1):
        """The caller's prediction of the second launch's pose (before the first launch): the first
        launch looks ahead towards it and no pilot step runs (pcp_icp_predict_first)."""
        Tm = _lib.f64arr(np.asarray(T1, dtype=np.float64).reshape(16))
        self.ctx.check(self.ctx.lib.pcp_icp_predict_first(self.h, Tm))

    def pilot_info(self):
        """(stride, sampled chunks, pairs) of the first launch's pilot step; (0, 0, -1): none ran."""
        s, c, n = C.c_int64(), C.c_int64(), C.c_int64()
        self.ctx.check(self.ctx.lib.pcp_icp_pilot_info(self.h, C.byref(s), C.byref(c), C.byref(n)))
        return s.value, c.value, n.value

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.pcp_icp_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def keys_owner(ctx, keys, bounds, out=None):
    """Per key (int64, global target index in the low 32 bits), the shard owning its winner:
    s with bounds[s] <= index < bounds[s + 1] (bounds: int64 device tensor, nshards + 1), 255
    for no correspondence.  uint8 device tensor."""
    n = keys.numel()
    out = torch.empty(n, dtype=torch.uint8, device=ctx.device) if out is None else out
    assert keys.dtype == torch.int64 and bounds.dtype == torch.int64 and out.numel() >= n
    ctx.check(ctx.lib.pcp_keys_owner(ctx.h, _ptr(keys), n, _ptr(bounds), bounds.numel() - 1, _ptr(out)))
    return out


def accumulate_owned(ctx, T_dev, q, keys, owner, rank, lo, hi, shard_xyz, acc=None):
    """Accumulators of the queries q (n x 3 fp32, ALL queries, original order) whose winner
    this rank owns (owner == rank), read from its own shard (global indices [lo, hi)) through
    its local keys: the device-resident target-sharded loop's accumulation."""
    acc = torch.zeros(24, dtype=torch.float64, device=ctx.device) if acc is None else acc
    n = q.shape[0]
    assert keys.numel() >= n and keys.dtype == torch.int64 and owner.numel() >= n and owner.dtype == torch.uint8
    ctx.check(ctx.lib.pcp_icp_accumulate_owned(ctx.h, _ptr(T_dev), _ptr(q) if n else None,
                                               q.stride(0) * q.element_size(), n, _ptr(keys), _ptr(owner), int(rank),
                                               int(lo), int(hi), _ptr(shard_xyz),
                                               shard_xyz.stride(0) * shard_xyz.element_size(), _ptr(acc)))
    return acc


def slab_guard(ctx, T_dev, box, lo, hi, flag):
    """Latch flag[0] = 1 when the owned queries' box leaves x in [lo, hi] under T_dev."""
    ctx.check(ctx.lib.pcp_slab_guard(ctx.h, _ptr(T_dev), _lib.f64arr(np.asarray(box, dtype=np.float64).reshape(6)),
                                     float(lo), float(hi), _ptr(flag)))


def icp_solve(acc, do_scale=False):
    a = np.asarray(acc, dtype=np.float64).reshape(24)
    dT = (C.c_double * 16)()
    rc = _lib.load().pcp_icp_solve(_lib.f64arr(a), int(do_scale), dT)
    return rc, np.array(dT[:]).reshape(4, 4)


class IcpPlanes:
    """pcp_icp_planes: the packed {point, normal} table of an ICP target, one 32-byte record per
    target point at its caller index.  target_xyz: (n, >= 3) fp32; normals: (n, 3) fp32 or the
    (n, 6) rows of normals_knn."""

    def __init__(self, ctx, target_xyz, normals):
        self.ctx = ctx
        n = target_xyz.shape[0]
        assert target_xyz.dtype == torch.float32 and normals.dtype == torch.float32 and normals.shape[0] == n
        h = C.c_void_p()
        ctx.check(ctx.lib.pcp_icp_planes_create(ctx.h, _ptr(target_xyz) if n else None,
                                                target_xyz.stride(0) * target_xyz.element_size(),
                                                _ptr(normals) if n else None,
                                                normals.stride(0) * normals.element_size(), n, C.byref(h)))
        self.h = h

    @property
    def size(self):
        return self.ctx.lib.pcp_icp_planes_size(self.h)

    @property
    def valid(self):
        """Records with a usable normal (|n|^2 >= 0.25, finite point and normal)."""
        return self.ctx.lib.pcp_icp_planes_valid(self.h)

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.pcp_icp_planes_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def icp_accumulate_plane(ctx, T_dev, q, keys, planes, acc=None):
    """The 30 point-to-plane accumulators of the queries q (n x 3 fp32, original order) under the
    device pose T_dev, paired by their keys (ICP.keys_dev) with the records of `planes`."""
    acc = torch.zeros(30, dtype=torch.float64, device=ctx.device) if acc is None else acc
    n = q.shape[0]
    assert keys.numel() >= n and keys.dtype in (torch.int64, torch.uint64) and acc.numel() >= 30
    ctx.check(ctx.lib.pcp_icp_accumulate_plane(ctx.h, _ptr(T_dev), _ptr(q) if n else None,
                                               q.stride(0) * q.element_size(), n, _ptr(keys) if n else None,
                                               planes.h, _ptr(acc)))
    return acc


class ICPBatch:
    """pcp_icp_batch (pcp.h I5): B query segments registered against one fp32 target index, one
    device pose per segment, three launches per point-to-plane iteration whatever B is.  q: (n, >= 3)
    fp32 device tensor; seg_offsets: B + 1 non-decreasing integers from 0 to n (segment s is
    q[seg_offsets[s]:seg_offsets[s + 1]]).  Keys are in q's order.  The trimmed loops (pcp.h I5b) trim
    every segment by its own quantile and take six launches per iteration, again whatever B is.  The
    point-to-point loops (pcp.h I5c: accumulate, solve_dev, run_dev, run_trimmed_dev) minimise the
    get_rot_icp objective per segment in the same three / six launches; they read the target's points
    from the cloud the index was built from, which the caller passes."""

    def __init__(self, target_index, q, seg_offsets):
        self.index = target_index
        self.ctx = ctx = target_index.ctx
        off = [int(v) for v in seg_offsets]
        if not off:
            raise ValueError("seg_offsets needs at least one entry")
        self.nseg = len(off) - 1
        self.nq = n = q.shape[0]
        h = C.c_void_p()
        ctx.check(ctx.lib.pcp_icp_batch_create(ctx.h, target_index.h, _ptr(q) if n else None,
                                               q.stride(0) * q.element_size(), n, (C.c_int64 * len(off))(*off),
                                               self.nseg, C.byref(h)))
        self.h = h

    def new_poses(self, T0=None):
        """(T_dev, stats): device poses (B, 16) fp64 row-major -- the identity, one 4x4 for all, or
        B of them -- and zeroed stats (B, 4)."""
        B = self.nseg
        T = np.eye(4) if T0 is None else np.asarray(T0, dtype=np.float64)
        T = np.broadcast_to(T.reshape(-1, 16), (B, 16)) if T.size == 16 else T.reshape(B, 16)
        return (torch.as_tensor(np.array(T), dtype=torch.float64).to(self.ctx.device).contiguous(),
                torch.zeros((B, 4), dtype=torch.float64, device=self.ctx.device))

    def _check_poses(self, T_dev, stats=None):
        assert T_dev.dtype == torch.float64 and T_dev.numel() >= 16 * self.nseg and T_dev.is_contiguous()
        if stats is not None:
            assert stats.dtype == torch.float64 and stats.numel() >= 4 * self.nseg and stats.is_contiguous()

    def keys_dev(self, T_dev, rmax, out=None):
        """Per query (q's order) the int64 key of its exact nearest target within rmax under its
        segment's pose, INT64_MAX for none: per segment, ICP.keys_dev's keys bit for bit."""
        ctx = self.ctx
        keys = torch.empty(self.nq, dtype=torch.int64, device=ctx.device) if out is None else out
        assert keys.dtype == torch.int64 and keys.numel() >= self.nq and keys.is_contiguous()
        self._check_poses(T_dev)
        ctx.check(ctx.lib.pcp_icp_batch_keys_dev(ctx.h, self.h, _ptr(T_dev), float(rmax), _ptr(keys)))
        return keys

    def accumulate_plane(self, T_dev, keys, planes, acc=None):
        """(B, 30): per segment the point-to-plane accumulators of icp_accumulate_plane."""
        ctx = self.ctx
        acc = torch.zeros((self.nseg, 30), dtype=torch.float64, device=ctx.device) if acc is None else acc
        assert acc.dtype == torch.float64 and acc.numel() >= 30 * self.nseg and acc.is_contiguous()
        assert keys.dtype == torch.int64 and keys.numel() >= self.nq and keys.is_contiguous()
        self._check_poses(T_dev)
        ctx.check(ctx.lib.pcp_icp_batch_accumulate_plane(ctx.h, self.h, _ptr(T_dev), _ptr(keys), planes.h, _ptr(acc)))
        return acc

    def solve_plane_dev(self, acc, T_dev, stats):
        """Per segment ICP.solve_plane_dev: T_dev[s] <- dT_s * T_dev[s]; a failed solve latches
        stats[s, 0] = -1 and freezes that segment's pose only."""
        ctx = self.ctx
        assert acc.dtype == torch.float64 and acc.numel() >= 30 * self.nseg and acc.is_contiguous()
        self._check_poses(T_dev, stats)
        ctx.check(ctx.lib.pcp_icp_batch_solve_plane_dev(ctx.h, _ptr(acc), self.nseg, _ptr(T_dev), _ptr(stats)))

    def run_plane_dev(self, planes, T_dev, stats, rmax, iters):
        """iters x (keys_dev, accumulate_plane, solve_plane_dev) with no host round trip."""
        ctx = self.ctx
        self._check_poses(T_dev, stats)
        ctx.check(ctx.lib.pcp_icp_batch_run_plane_dev(ctx.h, self.h, planes.h, _ptr(T_dev), float(rmax), int(iters),
                                                      _ptr(stats)))

    # ---- per-segment trims (pcp.h I5b): one quantile, cut and kept count per segment
    def _trim_io(self, keys, out):
        out = torch.empty_like(keys) if out is None else out
        assert keys.dtype == torch.int64 and out.dtype == torch.int64
        assert keys.numel() >= self.nq and out.numel() >= self.nq and keys.is_contiguous() and out.is_contiguous()
        return out, torch.zeros((self.nseg, 4), dtype=torch.int64, device=self.ctx.device)

    def trim_keys(self, keys, frac, mult=1.0, d_floor=0.0, out=None):
        """icp_trim_keys on every segment's slice of keys (q's order) separately.  out=None writes a
        new tensor, out=keys works in place.  Returns (keys_out, trim) with trim (B, 4) int64: per
        segment [m, kept, sel, bits of cut]."""
        ctx = self.ctx
        out, trim = self._trim_io(keys, out)
        ctx.check(ctx.lib.pcp_icp_batch_trim_keys(ctx.h, self.h, _ptr(keys) if self.nq else None, float(frac),
                                                  float(mult), float(d_floor), _ptr(out) if self.nq else None,
                                                  _ptr(trim) if self.nseg else None))
        return out, trim

    def trim_keys_plane(self, T_dev, keys, planes, frac, mult=1.0, d_floor=0.0, out=None):
        """icp_trim_keys_plane on every segment separately: its slice of keys, its queries (the
        handle's copy) and its pose T_dev[s].  out and the return values as trim_keys."""
        ctx = self.ctx
        out, trim = self._trim_io(keys, out)
        self._check_poses(T_dev)
        ctx.check(ctx.lib.pcp_icp_batch_trim_keys_plane(ctx.h, self.h, _ptr(T_dev), _ptr(keys) if self.nq else None,
                                                        planes.h, float(frac), float(mult), float(d_floor),
                                                        _ptr(out) if self.nq else None,
                                                        _ptr(trim) if self.nseg else None))
        return out, trim

    def _run_trimmed(self, fn, planes, T_dev, stats, rmax, frac, mult, d_floor, iters, trim):
        ctx = self.ctx
        self._check_poses(T_dev, stats)
        trim = torch.zeros((self.nseg, 4), dtype=torch.int64, device=ctx.device) if trim is None else trim
        assert trim.dtype == torch.int64 and trim.numel() >= 4 * self.nseg and trim.is_contiguous()
        ctx.check(fn(ctx.h, self.h, planes.h, _ptr(T_dev), float(rmax), float(frac), float(mult), float(d_floor),
                     int(iters), _ptr(stats), _ptr(trim) if self.nseg else None))
        return trim

    def run_plane_trimmed_dev(self, planes, T_dev, stats, rmax, frac, mult=1.0, d_floor=0.0, iters=4, trim=None):
        """run_plane_dev with trim_keys(frac, mult, d_floor) in place between the keys and the
        accumulation of every iteration: six launches per iteration whatever B and the segment sizes
        are.  A segment left with fewer than 6 pairs freezes alone.  Returns trim: the last
        iteration's (B, 4) rows [m, kept, sel, bits of cut] (int64 device tensor)."""
        return self._run_trimmed(self.ctx.lib.pcp_icp_batch_run_plane_trimmed_dev, planes, T_dev, stats, rmax, frac,
                                 mult, d_floor, iters, trim)

    def run_plane_rtrimmed_dev(self, planes, T_dev, stats, rmax, frac, mult=1.0, d_floor=0.0, iters=4, trim=None):
        """run_plane_trimmed_dev with trim_keys_plane in place of trim_keys: every iteration trims each
        segment by its pairs' plane residual at its pose.  Six launches per iteration; returns trim
        as there."""
        return self._run_trimmed(self.ctx.lib.pcp_icp_batch_run_plane_rtrimmed_dev, planes, T_dev, stats, rmax, frac,
                                 mult, d_floor, iters, trim)

    # ---- point-to-point (pcp.h I5c): the get_rot_icp contract per segment
    @staticmethod
    def _target(target_xyz):
        """(pointer, stride in bytes, points) of the target cloud, (n, >= 3) fp32 at caller index."""
        assert target_xyz.dtype == torch.float32 and target_xyz.dim() == 2 and target_xyz.shape[1] >= 3
        assert target_xyz.stride(1) == 1 or target_xyz.shape[0] == 0
        n = target_xyz.shape[0]
        return _ptr(target_xyz) if n else None, target_xyz.stride(0) * target_xyz.element_size() if n else 0, n

    def accumulate(self, T_dev, keys, target_xyz, acc=None):
        """(B, 24): per segment the Kabsch accumulators of pcp_icp_solve over its pairs; target_xyz:
        the cloud the target index was built from.  [23] is 0."""
        ctx = self.ctx
        acc = torch.zeros((self.nseg, 24), dtype=torch.float64, device=ctx.device) if acc is None else acc
        assert acc.dtype == torch.float64 and acc.numel() >= 24 * self.nseg and acc.is_contiguous()
        assert keys.dtype == torch.int64 and keys.numel() >= self.nq and keys.is_contiguous()
        self._check_poses(T_dev)
        tp, ts, tn = self._target(target_xyz)
        ctx.check(ctx.lib.pcp_icp_batch_accumulate(ctx.h, self.h, _ptr(T_dev), _ptr(keys), tp, ts, tn, _ptr(acc)))
        return acc

    def solve_dev(self, acc, T_dev, stats, do_scale=False):
        """Per segment ICP.solve_dev: T_dev[s] <- dT_s * T_dev[s]; a refused solve latches
        stats[s, 0] = -1 and freezes that segment's pose only."""
        ctx = self.ctx
        assert acc.dtype == torch.float64 and acc.numel() >= 24 * self.nseg and acc.is_contiguous()
        self._check_poses(T_dev, stats)
        ctx.check(ctx.lib.pcp_icp_batch_solve_dev(ctx.h, _ptr(acc), self.nseg, int(do_scale), _ptr(T_dev),
                                                  _ptr(stats)))

    def run_dev(self, target_xyz, T_dev, stats, rmax, iters, do_scale=False):
        """iters x (keys_dev, accumulate, solve_dev) with no host round trip: three launches per
        iteration whatever B is."""
        ctx = self.ctx
        self._check_poses(T_dev, stats)
        tp, ts, tn = self._target(target_xyz)
        ctx.check(ctx.lib.pcp_icp_batch_run_dev(ctx.h, self.h, tp, ts, tn, _ptr(T_dev), float(rmax), int(iters),
                                                int(do_scale), _ptr(stats)))

    def run_trimmed_dev(self, target_xyz, T_dev, stats, rmax, frac, mult=1.0, d_floor=0.0, iters=4, do_scale=False,
                        trim=None):
        """run_dev with trim_keys(frac, mult, d_floor) in place between the keys and the accumulation
        of every iteration: six launches per iteration.  A segment left with fewer than 3 pairs
        freezes alone.  Returns trim: the last iteration's (B, 4) rows [m, kept, sel, bits of cut]."""
        ctx = self.ctx
        self._check_poses(T_dev, stats)
        trim = torch.zeros((self.nseg, 4), dtype=torch.int64, device=ctx.device) if trim is None else trim
        assert trim.dtype == torch.int64 and trim.numel() >= 4 * self.nseg and trim.is_contiguous()
        tp, ts, tn = self._target(target_xyz)
        ctx.check(ctx.lib.pcp_icp_batch_run_trimmed_dev(ctx.h, self.h, tp, ts, tn, _ptr(T_dev), float(rmax),
                                                        float(frac), float(mult), float(d_floor), int(iters),
                                                        int(do_scale), _ptr(stats),
                                                        _ptr(trim) if self.nseg else None))
        return trim

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.pcp_icp_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def icp_trim_keys(ctx, keys, frac, mult=1.0, d_floor=0.0, out=None):
    """Trim correspondence keys (pcp.h I3): keep the valid keys whose fp32 d2 (the high word) is <=
    max(mult^2 * the frac-quantile of the valid d2, d_floor^2); the others become INT64_MAX.
    out=None writes a new tensor, out=keys works in place.  Returns (keys_out, trim) with trim =
    [m, kept, sel, bits of cut] as an int64 device tensor."""
    n = keys.numel()
    out = torch.empty_like(keys) if out is None else out
    assert keys.dtype == torch.int64 and out.dtype == torch.int64 and out.numel() >= n
    assert keys.is_contiguous() and out.is_contiguous()
    trim = torch.zeros(4, dtype=torch.int64, device=ctx.device)
    ctx.check(ctx.lib.pcp_icp_trim_keys(ctx.h, _ptr(keys) if n else None, n, float(frac), float(mult),
                                        float(d_floor), _ptr(out) if n else None, _ptr(trim)))
    return out, trim


def icp_trim_keys_plane(ctx, T_dev, q, keys, planes, frac, mult=1.0, d_floor=0.0, out=None):
    """Trim correspondence keys by the plane residual (pcp.h I3b): keep the usable pairs of the
    queries q (n x 3 fp32, original order) whose squared residual (n . (T q - p))^2 under the device
    pose T_dev is <= max(mult^2 * the frac-quantile of those residuals, d_floor^2); the other keys
    become INT64_MAX, the kept ones stay as they are.  out and the return values as icp_trim_keys."""
    n = q.shape[0]
    out = torch.empty_like(keys) if out is None else out
    assert keys.dtype == torch.int64 and out.dtype == torch.int64 and keys.numel() >= n and out.numel() >= n
    assert keys.is_contiguous() and out.is_contiguous()
    trim = torch.zeros(4, dtype=torch.int64, device=ctx.device)
    ctx.check(ctx.lib.pcp_icp_trim_keys_plane(ctx.h, _ptr(T_dev), _ptr(q) if n else None,
                                              q.stride(0) * q.element_size(), n, _ptr(keys) if n else None, planes.h,
                                              float(frac), float(mult), float(d_floor), _ptr(out) if n else None,
                                              _ptr(trim)))
    return out, trim


def icp_solve_plane(acc):
    """Host 6x6 solve of 30 plane accumulators: (rc, dT); rc = -6 (PCP_ERR_ICP) and the identity
    for a numerically singular system."""
    a = np.asarray(acc, dtype=np.float64).reshape(30)
    dT = (C.c_double * 16)()
    rc = _lib.load().pcp_icp_solve_plane(_lib.f64arr(a), dT)
    return rc, np.array(dT[:]).reshape(4, 4)


def get_rot_icp(ctx, src, temp, rmax, iters=20, do_scale=False, cell_size=0.0, src_dense=True,
                temp_dense=True):
    M = (C.c_double * 16)()
    err = C.c_float()
    ctx.check(ctx.lib.pcp_get_rot_icp(ctx.h, _ptr(src), src.shape[0], int(src_dense), _ptr(temp),
                                      temp.shape[0], int(temp_dense), M, float(rmax), int(iters),
                                      int(do_scale), float(cell_size), C.byref(err)))
    return float(err.value), np.array(M[:]).reshape(4, 4)


def get_rot_icp_batch(ctx, target, frames, seg_offsets, rmax, T0=None, iters=20, do_scale=False, trim=None,
                      cell_size=0.0, target_dense=True, frames_dense=True):
    """get_rot_icp for B frames in one call (pcp.h I5d): frames[off[s]:off[s + 1]] moved by T0[s]
    (None: the identity; one 4x4 for all; or B of them) is registered against target, both (n, 48)
    records at map coordinates, centred on the target's centroid.  trim = (frac, mult, d_floor) runs
    the loop with the per-segment point trim.  Returns (err (B,) float32, mats (B, 4, 4), steps (B,)
    int32, kept (B,) int64 or None without trim); the frame's pose is mats[s] @ T0[s]; err[s] = -1
    and mats[s] = the identity for a frame that found no pairs."""
    off, B, Tm = _seg_args(seg_offsets, T0)
    M = (C.c_double * (16 * B))()
    err = (C.c_float * B)()
    steps = (C.c_int32 * B)()
    kept = (C.c_int64 * B)() if trim is not None else None
    tr = (C.c_float * 3)(*[float(v) for v in trim]) if trim is not None else None
    nt, nq = target.shape[0], frames.shape[0]
    ctx.check(ctx.lib.pcp_get_rot_icp_batch(ctx.h, _ptr(target) if nt else None, nt, int(target_dense),
                                            _ptr(frames) if nq else None, nq, int(frames_dense), off, B, Tm,
                                            float(rmax), int(iters), int(do_scale), tr, float(cell_size), M, err,
                                            steps, kept))
    return (np.array(err[:], dtype=np.float32), np.array(M[:]).reshape(B, 4, 4), np.array(steps[:], dtype=np.int32),
            np.array(kept[:], dtype=np.int64) if kept is not None else None)


def get_rot_icp_plane(ctx, src, temp, rmax, iters=4, normals_k=16, cell_size=0.0, src_dense=True,
                      temp_dense=True):
    """get_rot_icp with the point-to-plane loop over normals_knn(normals_k) of src: (err, M);
    err = RMS point distance of the last iteration's pairs, -1 when the solve failed."""
    M = (C.c_double * 16)()
    err = C.c_float()
    ctx.check(ctx.lib.pcp_get_rot_icp_plane(ctx.h, _ptr(src), src.shape[0], int(src_dense), _ptr(temp),
                                            temp.shape[0], int(temp_dense), M, float(rmax), int(iters),
                                            int(normals_k), float(cell_size), C.byref(err)))
    return float(err.value), np.array(M[:]).reshape(4, 4)


def get_rot_icp_plane_trimmed(ctx, src, temp, rmax, frac, mult=1.0, d_floor=0.0, iters=4, normals_k=16,
                              cell_size=0.0, src_dense=True, temp_dense=True):
    """get_rot_icp_plane through the trimmed loop (pcp.h I3): (err, M, kept); kept = the pairs the
    last iteration's trim kept."""
    M = (C.c_double * 16)()
    err = C.c_float()
    kept = C.c_int64()
    ctx.check(ctx.lib.pcp_get_rot_icp_plane_trimmed(ctx.h, _ptr(src), src.shape[0], int(src_dense), _ptr(temp),
                                                    temp.shape[0], int(temp_dense), M, float(rmax), float(frac),
                                                    float(mult), float(d_floor), int(iters), int(normals_k),
                                                    float(cell_size), C.byref(err), C.byref(kept)))
    return float(err.value), np.array(M[:]).reshape(4, 4), int(kept.value)


def get_rot_icp_plane_rtrimmed(ctx, src, temp, rmax, frac, mult=1.0, d_floor=0.0, iters=4, normals_k=16,
                               cell_size=0.0, src_dense=True, temp_dense=True):
    """get_rot_icp_plane_trimmed through the loop that trims by the plane residual (pcp.h I3b):
    (err, M, kept) as there."""
    M = (C.c_double * 16)()
    err = C.c_float()
    kept = C.c_int64()
    ctx.check(ctx.lib.pcp_get_rot_icp_plane_rtrimmed(ctx.h, _ptr(src), src.shape[0], int(src_dense), _ptr(temp),
                                                     temp.shape[0], int(temp_dense), M, float(rmax), float(frac),
                                                     float(mult), float(d_floor), int(iters), int(normals_k),
                                                     float(cell_size), C.byref(err), C.byref(kept)))
    return float(err.value), np.array(M[:]).reshape(4, 4), int(kept.value)
