// The 3x3 Kabsch / Umeyama solve of the 24 accumulators (pcp_icp_solve), host and device: the
// device-resident loop (k_icp_solve_dev) and the pilot step (k_pilot_map) run the same code.
#pragma once
#include <cmath>

#include "common.hpp"

namespace pcp {

// One-sided Jacobi SVD of a 3x3 matrix: A = U diag(s) V^T (columns of U, V).
// (host and device: the device-resident loop solves on the GPU with the same code)
__host__ __device__ inline void svd3(const double Ain[9], double U[9], double s[3], double V[9]) {
    double A[9];
    for (int i = 0; i < 9; i++) A[i] = Ain[i];
    for (int i = 0; i < 9; i++) V[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0.0;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                double al = 0, be = 0, ga = 0;
                for (int r = 0; r < 3; r++) {
                    al += A[3 * r + p] * A[3 * r + p];
                    be += A[3 * r + q] * A[3 * r + q];
                    ga += A[3 * r + p] * A[3 * r + q];
                }
                if (ga == 0.0 || fabs(ga) <= 1e-300) continue;
                double conv = fabs(ga) / sqrt(al * be);
                if (!(conv > 1e-15)) continue;
                off = fmax(off, conv);
                double zeta = (be - al) / (2.0 * ga);
                double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
                for (int r = 0; r < 3; r++) {
                    double ap = A[3 * r + p], aq = A[3 * r + q];
                    A[3 * r + p] = c * ap - sn * aq;
                    A[3 * r + q] = sn * ap + c * aq;
                    double vp = V[3 * r + p], vq = V[3 * r + q];
                    V[3 * r + p] = c * vp - sn * vq;
                    V[3 * r + q] = sn * vp + c * vq;
                }
            }
        if (off < 1e-15) break;
    }
    for (int c = 0; c < 3; c++) {
        double n = 0;
        for (int r = 0; r < 3; r++) n += A[3 * r + c] * A[3 * r + c];
        s[c] = sqrt(n);
    }
    // order singular values descending (permute U/V columns consistently)
    int ord[3] = {0, 1, 2};
    for (int i = 0; i < 3; i++)
        for (int j = i + 1; j < 3; j++)
            if (s[ord[j]] > s[ord[i]]) { const int tmp = ord[i]; ord[i] = ord[j]; ord[j] = tmp; }
    double A2[9], V2[9], s2[3];
    for (int c = 0; c < 3; c++) {
        s2[c] = s[ord[c]];
        for (int r = 0; r < 3; r++) { A2[3 * r + c] = A[3 * r + ord[c]]; V2[3 * r + c] = V[3 * r + ord[c]]; }
    }
    for (int i = 0; i < 9; i++) V[i] = V2[i];
    for (int c = 0; c < 3; c++) s[c] = s2[c];
    const double tiny = 1e-14 * (s[0] > 0 ? s[0] : 1.0);
    for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) U[3 * r + c] = s[c] > tiny ? A2[3 * r + c] / s[c] : 0.0;
    // complete a rank-deficient basis: u2 = u0 x u1 (planar clouds have rank 2)
    if (!(s[2] > tiny)) {
        double u0[3] = {U[0], U[3], U[6]}, u1[3] = {U[1], U[4], U[7]};
        if (!(s[1] > tiny)) {  // rank 1: any unit vector orthogonal to u0
            double a[3] = {fabs(u0[0]) < 0.9 ? 1.0 : 0.0, fabs(u0[0]) < 0.9 ? 0.0 : 1.0, 0.0};
            double d = a[0] * u0[0] + a[1] * u0[1] + a[2] * u0[2];
            for (int r = 0; r < 3; r++) u1[r] = a[r] - d * u0[r];
            double nn = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
            for (int r = 0; r < 3; r++) { u1[r] /= nn; U[3 * r + 1] = u1[r]; }
        }
        double u2[3] = {u0[1] * u1[2] - u0[2] * u1[1], u0[2] * u1[0] - u0[0] * u1[2], u0[0] * u1[1] - u0[1] * u1[0]};
        for (int r = 0; r < 3; r++) U[3 * r + 2] = u2[r];
    }
}

__host__ __device__ inline double det3(const double M[9]) {
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) +
           M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// S = acc[7..15] - n qm pm^T cancels down from `scale` = max(|acc[7..15]|, n |qm| |pm|): each entry
// carries a few eps * scale of rounding, so a largest singular value within kRank0 eps * scale is
// noise, not a direction (every pair at one target point, or every query at one point).
constexpr double kRank0 = 64.0, kEps = 2.220446049250313e-16;

__host__ __device__ inline int icp_solve(const double acc[24], int do_scale, double dT[16]) {
    const double n = acc[0];
    if (!(n >= 3.0)) return PCP_ERR_ICP;
    for (int k = 0; k < 23; k++)  // a NaN or an infinity among the sums (false for a NaN)
        if (!(fabs(acc[k]) <= 1.7976931348623157e308)) return PCP_ERR_ICP;
    double qm[3], pm[3], S[9];
    for (int k = 0; k < 3; k++) { qm[k] = acc[1 + k] / n; pm[k] = acc[4 + k] / n; }
    // S = sum (q - qm)(p - pm)^T ; optimal R maximises trace(R S): S = U s V^T, R = V D U^T
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) S[3 * a + b] = acc[7 + 3 * a + b] - n * qm[a] * pm[b];
    double U[9], s[3], V[9];
    svd3(S, U, s, V);
    double scale = n * sqrt((qm[0] * qm[0] + qm[1] * qm[1] + qm[2] * qm[2]) *
                            (pm[0] * pm[0] + pm[1] * pm[1] + pm[2] * pm[2]));
    for (int k = 7; k < 16; k++) scale = fmax(scale, fabs(acc[k]));
    // rank 0: no rotation is preferred, so none is made (the pairs' centroids still align)
    const bool rank0 = !(s[0] > kRank0 * kEps * scale);
    double R[9];
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            double v = 0;
            for (int k = 0; k < 3; k++) v += V[3 * a + k] * U[3 * b + k];
            R[3 * a + b] = rank0 ? (a == b ? 1.0 : 0.0) : v;
        }
    double d = det3(R) < 0 ? -1.0 : 1.0;
    if (d < 0) {  // flip the axis of the smallest singular value
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) R[3 * a + b] -= 2.0 * V[3 * a + 2] * U[3 * b + 2];
    }
    double sc = 1.0;
    if (do_scale && !rank0) {
        const double var = (acc[16] + acc[19] + acc[21]) - n * (qm[0] * qm[0] + qm[1] * qm[1] + qm[2] * qm[2]);
        if (var > 0) sc = (s[0] + s[1] + d * s[2]) / var;
    }
    for (int a = 0; a < 3; a++) {
        double t = pm[a];
        for (int b = 0; b < 3; b++) {
            dT[4 * a + b] = sc * R[3 * a + b];
            t -= sc * R[3 * a + b] * qm[b];
        }
        dT[4 * a + 3] = t;
    }
    dT[12] = dT[13] = dT[14] = 0.0;
    dT[15] = 1.0;
    return PCP_OK;
}

}  // namespace pcp
