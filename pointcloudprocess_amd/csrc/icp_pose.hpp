// The look-ahead pose block's kernels (included by icp.hip alone): k_pose_set before every launch,
// k_pilot_map before the first, their step measure and constants, and the device-resident loop's
// solve, k_icp_solve_dev.  The block's layout is icp_handle.hpp's, the solve icp_solve.hpp's.
#pragma once
#include "icp_handle.hpp"
#include "icp_solve.hpp"

namespace pcp {

// The pose block before a launch (k_pose_set): prev <- cur, then cur <- R, t of T_dev (row-major
// 4x4 doubles cast to fp32, as on the host) or of the host-cast hp (pose32) when T_dev is null.
// The look-ahead map. ICP steps are almost collinear and shrink geometrically (ratio r per
// launch), so a query's remaining path from q_t is about (q_t - q_{t-1}) r / (1 - r) along the
// last step.  A search centred at c = T_c q, T_c = T_t + beta (T_t - T_{t-1}) with
// beta = alpha r / (1 - r), puts the cached ball around the path still to come instead of around
// its start.  T_c is an affine map, written to this launch's history slot (where the verify pass
// rebuilds c) and beside the pose (where the search kernels read it).  Exactness never depends on
// it: the certificate holds for any centre; beta only decides how many later searches there are.
// The step's size is its largest displacement over the corners of `box`, the target grid's box
// grown by rmax (it holds every query that can have a correspondence); beta = 0 at the second
// launch (no ratio yet), when the step did not shrink (a pose jump included), and it is cut so
// that no corner's offset exceeds cap.  The first launch has no step behind it at all: its beta
// comes from a predicted second pose (the pilot step or the caller's, k_pilot_map), else it is 0.
struct LookAhead {
    float lo[3], hi[3];  // the box
    float alpha, cap;    // fraction of the predicted remaining path; largest offset (m)
    int off;             // PCP_ICP_OPT_NO_LOOKAHEAD
};
#ifndef PCP_LOOK_ALPHA
#define PCP_LOOK_ALPHA 0.5f
#endif
constexpr float kLookAlpha = PCP_LOOK_ALPHA, kLookCap = 0.02f, kLookRmax = 0.9f;
// The first launch's look-ahead (k_pilot_map): beta_0 = min(kPilotAlpha, kPilotCap / s_1) with s_1
// the predicted first step's size.  The first step is the largest of the registration and the
// second is still large, so the centre goes further than one step when the cap allows
// (tools/sim_icp_pilot.py sweeps both).
#ifndef PCP_PILOT_ALPHA
#define PCP_PILOT_ALPHA 1.5f
#endif
#ifndef PCP_PILOT_CAP
#define PCP_PILOT_CAP 0.045f
#endif
constexpr float kPilotAlpha = PCP_PILOT_ALPHA, kPilotCap = PCP_PILOT_CAP;
constexpr int64_t kPilotChunks = 8192;  // the pilot samples about this many 64-query chunks
// the pilot runs by default from this many queries: its cost is about constant (three launches and
// ~8K chunks, ~0.06 ms), below 5 % of a first launch that takes ~44 us per million queries
constexpr int64_t kPilotMinQueries = (int64_t)1 << 25;

// the size of the step from pose `prev` to pose `cur` (12 floats each: R row-major, t): the largest
// displacement y - T_prev T_cur^-1 y = y - (M y - v) over the corners y of the box
__device__ double step_size(const float* cur, const float* prev, const LookAhead& la) {
    double A[9], B[9], ta[3], tb[3], Ai[9], BA[9], v[3];
    for (int k = 0; k < 9; k++) { A[k] = cur[k]; B[k] = prev[k]; }
    for (int k = 0; k < 3; k++) { ta[k] = cur[9 + k]; tb[k] = prev[9 + k]; }
    const double det = det3(A);
    Ai[0] = A[4] * A[8] - A[5] * A[7]; Ai[1] = A[2] * A[7] - A[1] * A[8]; Ai[2] = A[1] * A[5] - A[2] * A[4];
    Ai[3] = A[5] * A[6] - A[3] * A[8]; Ai[4] = A[0] * A[8] - A[2] * A[6]; Ai[5] = A[2] * A[3] - A[0] * A[5];
    Ai[6] = A[3] * A[7] - A[4] * A[6]; Ai[7] = A[1] * A[6] - A[0] * A[7]; Ai[8] = A[0] * A[4] - A[1] * A[3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++)
            BA[3 * r + c] = (B[3 * r] * Ai[c] + B[3 * r + 1] * Ai[3 + c] + B[3 * r + 2] * Ai[6 + c]) / det;
    for (int r = 0; r < 3; r++) v[r] = BA[3 * r] * ta[0] + BA[3 * r + 1] * ta[1] + BA[3 * r + 2] * ta[2] - tb[r];
    double s2 = 0.0;
    for (int c = 0; c < 8; c++) {
        const double y[3] = {c & 1 ? la.hi[0] : la.lo[0], c & 2 ? la.hi[1] : la.lo[1], c & 4 ? la.hi[2] : la.lo[2]};
        double d2 = 0.0;
        for (int r = 0; r < 3; r++) {
            const double d = y[r] - (BA[3 * r] * y[0] + BA[3 * r + 1] * y[1] + BA[3 * r + 2] * y[2]) + v[r];
            d2 += d * d;
        }
        s2 = fmax(s2, d2);
    }
    return sqrt(s2);
}

__global__ void k_pose_set(const double* T, Pose32 hp, LookAhead la, PoseBlock* pose, float* hist, uint32_t launch) {
    float* const cur = pose->cur;
    pose->launch = launch;
    for (int k = 0; k < 12; k++) pose->prev[k] = cur[k];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) cur[3 * r + c] = T ? (float)T[4 * r + c] : hp.R[3 * r + c];
        cur[9 + r] = T ? (float)T[4 * r + 3] : hp.t[r];
    }
    // this step's displacement of a point y (target frame)
    const float step = launch > 0 ? (float)step_size(cur, pose->prev, la) : 0.f, prev = pose->step;
    float beta = 0.f;
    // launch 1 has no previous step, so no ratio and no look-ahead; launch 0's comes from the pilot
    // step, if there is one (k_pilot_map overwrites the words written here)
    const float ratio = launch == 1 ? 0.f : (prev > 0.f ? step / prev : 0.f);
    if (!la.off && launch > 0 && step > 0.f && ratio > 0.f && ratio < 1.f) {  // (false for a NaN)
        const float r = fminf(ratio, kLookRmax);
        beta = la.alpha * r / (1.f - r);
        if (beta * step > la.cap) beta = la.cap / step;
    }
    pose->step = step;
    pose->beta = beta;
    pose->off = beta * step;
    if (launch == 0) pose->pilot_pairs = -1.f;
    // T_c: beta = 0 gives the pose itself, bit for bit
    for (int k = 0; k < 12; k++) pose->c[k] = __fmaf_rn(beta, cur[k] - pose->prev[k], cur[k]);
    for (int k = 0; k < 12; k++) hist[k] = pose->c[k];
}

// The first launch's look-ahead map, after k_pose_set(launch 0) and before the first search.  One
// thread.  The predicted second pose T_1 is the caller's (pred.on: pcp_icp_predict_first) or one
// Kabsch step (no scale) over the pilot's sums, dT * T_0 with T_0 the fp32 pose of the block; then
// beta_0 = min(kPilotAlpha, kPilotCap / s_1), s_1 the step's size as in k_pose_set, and
// T_c = T_0 + beta_0 (T_1 - T_0) goes to the pose block and to history slot 0.  A refused solve
// (fewer than 3 pairs, non-finite sums), a non-finite prediction or s_1 = 0 leave beta_0 = 0 and the
// block as k_pose_set wrote it: the first launch is then the plain one.
struct PilotPred {
    int on;
    double T1[16];
};
__global__ void k_pilot_map(const double* acc, PilotPred pred, LookAhead la, PoseBlock* pose, float* hist) {
    const float* const cur = pose->cur;
    double T1[16];
    if (pred.on) {
        for (int k = 0; k < 16; k++) T1[k] = pred.T1[k];
    } else {
        double a[24], dT[16];
        for (int k = 0; k < 24; k++) a[k] = acc[k];
        pose->pilot_pairs = (float)a[0];
        if (icp_solve(a, 0, dT) != PCP_OK) return;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 4; j++) {
                double v = j == 3 ? dT[4 * i + 3] : 0.0;
                for (int k = 0; k < 3; k++) v += dT[4 * i + k] * (double)(j == 3 ? cur[9 + k] : cur[3 * k + j]);
                T1[4 * i + j] = v;
            }
    }
    float p1[12];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) p1[3 * r + c] = (float)T1[4 * r + c];
        p1[9 + r] = (float)T1[4 * r + 3];
    }
    for (int k = 0; k < 12; k++)
        if (!(fabsf(p1[k]) <= 3.4028234e38f)) return;  // (false for a NaN)
    const float step = (float)step_size(p1, cur, la);
    if (la.off || !(step > 0.f) || !(step <= 3.4028234e38f)) return;
    const float beta = fminf(kPilotAlpha, kPilotCap / step);
    float Tc[12];
    for (int k = 0; k < 12; k++) {
        Tc[k] = __fmaf_rn(beta, p1[k] - cur[k], cur[k]);
        if (!(fabsf(Tc[k]) <= 3.4028234e38f)) return;
    }
    pose->beta = beta;
    pose->off = beta * step;
    for (int k = 0; k < 12; k++) pose->c[k] = hist[k] = Tc[k];
}

// One thread: solve the 3x3 problem of acc, T <- dT * T (device pose), stats as in pcp.h
// (the host loop of pcp_icp_run, minus the convergence test).  A failed solve latches
// stats[0] = -1 and freezes T.
__global__ void k_icp_solve_dev(const double* acc, int do_scale, double* T, double* stats) {
    if (stats[0] < 0) return;
    double a[24], dT[16], Tn[16];
    for (int k = 0; k < 24; k++) a[k] = acc[k];
    stats[2] += a[23];
    if (icp_solve(a, do_scale, dT) != PCP_OK) {
        stats[0] = -1.0;
        return;
    }
    stats[1] = sqrt(a[22] / a[0]);
    stats[3] += 1.0;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double v = 0;
            for (int k = 0; k < 4; k++) v += dT[4 * i + k] * T[4 * k + j];
            Tn[4 * i + j] = v;
        }
    for (int k = 0; k < 16; k++) T[k] = Tn[k];
}

}  // namespace pcp
