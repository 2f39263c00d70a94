// The point-to-plane minimisation's plane table, the validity test of a record's normal and the
// 6x6 solve (pcp.h I2), shared by the single-pair loop (icp_plane.hip) and the batched one
// (icp_batch.hip): one arithmetic.  What is computed per pair is icp_pair.hpp's.
#pragma once
#include <cmath>

#include "common.hpp"

struct pcp_icp_planes {
    pcp_ctx* owner = nullptr;  // the creating context: owns rec (a lifetime reference)
    int64_t n = 0;             // records = the target's caller size
    int64_t valid = 0;         // records with a usable normal
    float4* rec = nullptr;     // 2 * n: {px,py,pz,0}, {nx,ny,nz,0}; an invalid record has n = 0
};

namespace pcp {

constexpr int kPAcc = PCP_ICP_PLANE_ACC;
constexpr double kMinPivot = 1e-10;

__device__ __forceinline__ bool plane_valid(float nx, float ny, float nz) {
    return nx * nx + ny * ny + nz * nz >= 0.25f;  // false for a NaN
}

// The 6x6 solve of pcp.h.  x = (omega, t) minimises sum (r + J . x)^2: A x = -b.  The rotation
// unknowns are scaled by the RMS lever arm s so that both 3x3 diagonal blocks have the same
// trace, the system is divided by its largest diagonal entry, and the pivots of the unpivoted
// LDL^T of that unit-scale matrix decide: <= 1e-10 is numerically singular (a plane's three
// free motions, two planes' one), and thin but determined systems stay well above it.
__host__ __device__ inline int plane_solve(const double acc[kPAcc], double dT[16]) {
    for (int i = 0; i < 16; i++) dT[i] = (i % 5 == 0) ? 1.0 : 0.0;
    if (!(acc[0] >= 6.0)) return PCP_ERR_ICP;
    double A[6][6], rhs[6];
    int k = 1;
    for (int a = 0; a < 6; a++)
        for (int b = a; b < 6; b++) {
            A[a][b] = acc[k];
            A[b][a] = acc[k++];
        }
    const double tw = A[0][0] + A[1][1] + A[2][2], tt = A[3][3] + A[4][4] + A[5][5];
    if (!(tt > 0.0) || !(tw > 0.0)) return PCP_ERR_ICP;  // tw == 0: every rotation pivot would be 0
    const double s = sqrt(tw / tt);
    double D[6];
    for (int a = 0; a < 6; a++) D[a] = a < 3 ? 1.0 / s : 1.0;
    double m = 0.0;
    for (int a = 0; a < 6; a++) {
        for (int b = 0; b < 6; b++) A[a][b] = D[a] * A[a][b] * D[b];
        rhs[a] = -(D[a] * acc[22 + a]);
        if (A[a][a] > m) m = A[a][a];
    }
    if (!(m > 0.0) || !(m < INFINITY)) return PCP_ERR_ICP;
    for (int a = 0; a < 6; a++) {
        for (int b = 0; b < 6; b++) A[a][b] /= m;
        rhs[a] /= m;
    }
    double L[6][6], d[6];
    for (int j = 0; j < 6; j++) {
        double v = A[j][j];
        for (int c = 0; c < j; c++) v -= L[j][c] * L[j][c] * d[c];
        if (!(v > kMinPivot)) return PCP_ERR_ICP;
        d[j] = v;
        for (int i = j + 1; i < 6; i++) {
            double w = A[i][j];
            for (int c = 0; c < j; c++) w -= L[i][c] * L[j][c] * d[c];
            L[i][j] = w / v;
        }
    }
    double y[6];
    for (int i = 0; i < 6; i++) {  // L z = rhs
        double v = rhs[i];
        for (int c = 0; c < i; c++) v -= L[i][c] * y[c];
        y[i] = v;
    }
    for (int i = 0; i < 6; i++) y[i] /= d[i];
    for (int i = 5; i >= 0; i--) {  // L^T y = z / d
        double v = y[i];
        for (int c = i + 1; c < 6; c++) v -= L[c][i] * y[c];
        y[i] = v;
    }
    const double w[3] = {D[0] * y[0], D[1] * y[1], D[2] * y[2]};
    for (int i = 0; i < 6; i++)
        if (!(fabs(y[i]) < INFINITY)) return PCP_ERR_ICP;  // non-finite accumulators
    // R = exp([w]x) = I + a K + b K^2, a = sin(th)/th, b = (1 - cos th)/th^2 = (sin(th/2)/(th/2))^2 / 2
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(th2);
    double ca, cb;
    if (th < 1e-4) {
        ca = 1.0 - th2 / 6.0 + th2 * th2 / 120.0;
        cb = 0.5 - th2 / 24.0 + th2 * th2 / 720.0;
    } else {
        const double h = sin(0.5 * th) / (0.5 * th);
        ca = sin(th) / th;
        cb = 0.5 * h * h;
    }
    const double K[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) {
            double k2 = 0.0;
            for (int c = 0; c < 3; c++) k2 += K[i][c] * K[c][j];
            dT[4 * i + j] = (i == j ? 1.0 : 0.0) + ca * K[i][j] + cb * k2;
        }
        dT[4 * i + 3] = y[3 + i];
    }
    return PCP_OK;
}

// one thread: solve, T <- dT * T, stats as in pcp.h.  A failed solve latches stats[0] = -1 and
// freezes T, as k_icp_solve_dev does.
__device__ inline void solve_apply(const double* a, double* T, double* stats) {
    if (stats[0] < 0) return;
    double dT[16], Tn[16];
    if (plane_solve(a, dT) != PCP_OK) {
        stats[0] = -1.0;
        return;
    }
    stats[1] = sqrt(a[29] / a[0]);
    stats[2] = sqrt(a[28] / a[0]);
    stats[3] += 1.0;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double v = 0;
            for (int c = 0; c < 4; c++) v += dT[4 * i + c] * T[4 * c + j];
            Tn[4 * i + j] = v;
        }
    for (int c = 0; c < 16; c++) T[c] = Tn[c];
}

}  // namespace pcp
