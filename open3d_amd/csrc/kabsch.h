// The rotation / translation of a least-squares rigid fit from its 3x3
// cross-covariance: the one routine behind o3dmi_compute_rt_p2point (host) and
// the RANSAC hypothesis kernel (ransac.hip), so that the two cannot drift.
//
// ComputeRtPointToPointCPU after its reduction (RegistrationCPU.cpp:640-650):
// Sxy = U D V^T, R = U diag(1, 1, det(U) det(V)) V^T, t = mean_t - R mean_s.
// The reference calls LAPACK gesvd; here a one-sided (Hestenes) Jacobi SVD in
// float64: columns of G = Sxy V are rotated pairwise until orthogonal, then
// u_i = g_i / |g_i|. The third left vector is taken as u_1 x u_2, which folds
// the reflection test into det(V): with u_3 = e (u_1 x u_2), e = det(U),
// det(U) det(V) u_3 = det(V) (u_1 x u_2). That also covers planar
// correspondence sets (sigma_3 = 0) without dividing by sigma_3.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace o3dmi {

// G[row][col]: cross-covariance (target rows, source columns), any positive
// scale; it is overwritten. ms / mt: the means of the source / target points.
// *sigma0 >= *sigma1: the two largest singular values of G (in G's scale).
__host__ __device__ inline void KabschJacobi(double G[3][3],
                                             const double* ms,
                                             const double* mt, double* R9,
                                             double* t3, double* sigma0,
                                             double* sigma1) {
    double V[3][3];
    for (int j = 0; j < 3; ++j)
        for (int k = 0; k < 3; ++k) V[j][k] = j == k ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int r = 0; r < 3; ++r) {
                    alpha += G[r][p] * G[r][p];
                    beta += G[r][q] * G[r][q];
                    gamma += G[r][p] * G[r][q];
                }
                if (gamma == 0.0 ||
                    fabs(gamma) <= 1e-17 * sqrt(alpha * beta))
                    continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double tn = (zeta >= 0 ? 1.0 : -1.0) /
                                  (fabs(zeta) +
                                   sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + tn * tn);
                const double sn = c * tn;
                for (int r = 0; r < 3; ++r) {
                    const double gp = G[r][p], gq = G[r][q];
                    G[r][p] = c * gp - sn * gq;
                    G[r][q] = sn * gp + c * gq;
                    const double vp = V[r][p], vq = V[r][q];
                    V[r][p] = c * vp - sn * vq;
                    V[r][q] = sn * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    // column order by decreasing singular value
    double sig[3];
    int ord[3] = {0, 1, 2};
    for (int c = 0; c < 3; ++c)
        sig[c] = sqrt(G[0][c] * G[0][c] + G[1][c] * G[1][c] +
                           G[2][c] * G[2][c]);
    for (int a = 0; a < 2; ++a)
        for (int b = a + 1; b < 3; ++b)
            if (sig[ord[b]] > sig[ord[a]]) {
                const int tmp = ord[a];
                ord[a] = ord[b];
                ord[b] = tmp;
            }
    double u[3][3], v[3][3];  // u[i] / v[i] = i-th singular vectors
    for (int i = 0; i < 3; ++i)
        for (int r = 0; r < 3; ++r) v[i][r] = V[r][ord[i]];
    const double s0 = sig[ord[0]], s1 = sig[ord[1]];
    *sigma0 = s0;
    *sigma1 = s1;
    if (!(s0 > 0)) {
        // all correspondences coincide with their means: rotation undetermined,
        // the least-squares answer is the pure translation.
        for (int i = 0; i < 9; ++i) R9[i] = (i % 4 == 0) ? 1.0 : 0.0;
        for (int k = 0; k < 3; ++k) t3[k] = mt[k] - ms[k];
        return;
    }
    for (int r = 0; r < 3; ++r) u[0][r] = G[r][ord[0]] / s0;
    if (s1 > 1e-300 && s1 > 1e-15 * s0) {
        double d = 0, nrm = 0;
        for (int r = 0; r < 3; ++r) u[1][r] = G[r][ord[1]] / s1;
        for (int r = 0; r < 3; ++r) d += u[1][r] * u[0][r];
        for (int r = 0; r < 3; ++r) {
            u[1][r] -= d * u[0][r];
            nrm += u[1][r] * u[1][r];
        }
        nrm = sqrt(nrm);
        for (int r = 0; r < 3; ++r) u[1][r] /= nrm;
    } else {
        // rank one: any unit vector orthogonal to u_0
        int m = 0;
        for (int r = 1; r < 3; ++r)
            if (fabs(u[0][r]) < fabs(u[0][m])) m = r;
        double e[3] = {0, 0, 0};
        e[m] = 1.0;
        double d = u[0][m], nrm = 0;
        for (int r = 0; r < 3; ++r) {
            u[1][r] = e[r] - d * u[0][r];
            nrm += u[1][r] * u[1][r];
        }
        nrm = sqrt(nrm);
        for (int r = 0; r < 3; ++r) u[1][r] /= nrm;
    }
    u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
    u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
    u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
    const double detV =
            v[0][0] * (v[1][1] * v[2][2] - v[1][2] * v[2][1]) -
            v[0][1] * (v[1][0] * v[2][2] - v[1][2] * v[2][0]) +
            v[0][2] * (v[1][0] * v[2][1] - v[1][1] * v[2][0]);
    const double sgn = detV < 0 ? -1.0 : 1.0;
    for (int j = 0; j < 3; ++j)
        for (int k = 0; k < 3; ++k)
            R9[j * 3 + k] = u[0][j] * v[0][k] + u[1][j] * v[1][k] +
                            sgn * u[2][j] * v[2][k];
    for (int j = 0; j < 3; ++j)
        t3[j] = mt[j] - (R9[j * 3 + 0] * ms[0] + R9[j * 3 + 1] * ms[1] +
                         R9[j * 3 + 2] * ms[2]);
}

}  // namespace o3dmi
