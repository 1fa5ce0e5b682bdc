// Quadric error minimiser shared by the mesh kernels (mesh_clean.hip: clustering representatives, mesh_decimate.hip: edge-collapse positions).
// x = xbar + A+ (-b - A xbar) in fp64 for a symmetric 3x3 A = (s00 s01 s02 s11 s12 s22): A+ from a cyclic Jacobi eigen-solve without the
// eigenvalues below QEF_EIG_CUT of the largest; x = xbar when the largest is not positive.  Only + - * / sqrt: under -ffp-contract=off the
// result is the same on every launch and restates bit for bit in NumPy (tests/qem_restatement.py).
#pragma once
#include "common.h"

#define QEF_EIG_CUT 1e-3

namespace {

// eigen-decomposition of the symmetric 3x3 s (s00 s01 s02 s11 s12 s22) by cyclic Jacobi: w = eigenvalues, columns of v = eigenvectors
__device__ void qef_jacobi(const double s[6], double w[3], double v[3][3]) {
    double a[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 32; ++sweep) {
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
        const double dia = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2];
        if (!(off > 1e-36 * dia)) break;
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            if (a[p][q] == 0.0) continue;
            const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
            for (int k = 0; k < 3; ++k) {            // a <- a J (columns p, q)
                const double akp = a[k][p], akq = a[k][q];
                a[k][p] = c * akp - sn * akq;
                a[k][q] = sn * akp + c * akq;
            }
            for (int k = 0; k < 3; ++k) {            // a <- J^T a (rows p, q)
                const double apk = a[p][k], aqk = a[q][k];
                a[p][k] = c * apk - sn * aqk;
                a[q][k] = sn * apk + c * aqk;
            }
            for (int k = 0; k < 3; ++k) {
                const double vkp = v[k][p], vkq = v[k][q];
                v[k][p] = c * vkp - sn * vkq;
                v[k][q] = sn * vkp + c * vkq;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = a[i][i];
}

// x = xb + A+ (-b - A xb), A = s; r = -b - A xb, x = xb + sum over the kept eigenpairs of v (v . r) / w
__device__ void qef_solve(const double s[6], const double b[3], const double xb[3], double x[3]) {
    double w[3], v[3][3];
    qef_jacobi(s, w, v);
    const double wmax = fmax(w[0], fmax(w[1], w[2]));
    const double r[3] = {-b[0] - (s[0] * xb[0] + s[1] * xb[1] + s[2] * xb[2]), -b[1] - (s[1] * xb[0] + s[3] * xb[1] + s[4] * xb[2]),
                         -b[2] - (s[2] * xb[0] + s[4] * xb[1] + s[5] * xb[2])};
#pragma unroll
    for (int j = 0; j < 3; ++j) x[j] = xb[j];
    if (wmax > 0.0) {
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            if (!(w[e] >= QEF_EIG_CUT * wmax)) continue;
            const double c = (v[0][e] * r[0] + v[1][e] * r[1] + v[2][e] * r[2]) / w[e];
#pragma unroll
            for (int j = 0; j < 3; ++j) x[j] += c * v[j][e];
        }
    }
}

}  // namespace
