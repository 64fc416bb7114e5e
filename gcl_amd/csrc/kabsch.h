// The fp64 3 x 3 Kabsch solution shared by the registration back-ends (sc2pcr.hip: weighted, per seed and per refinement
// step; ransac.hip: unweighted, per minimal sample; icp.hip: the fp64 rotation, per ICP update).
#pragma once
#include "common.h"

#include <math.h>

namespace gcl {

// ---- 3 x 3 SVD (one-sided Jacobi, fp64) and the weighted Kabsch solution (common.py:7-45) ---------------------
// H = A^T W B;  R = V diag(1, 1, det(V U^T)) U^T with singular values in DESCENDING order (torch.svd);  t = cb - R ca
// One body, two exits: PACK = true rounds R and t to the 3 x 4 float rows the registration kernels keep (kabsch_from_H);
// PACK = false hands out the fp64 rotation before any packing (kabsch_rotation, R9 row-major).
template <bool PACK>
static __host__ __device__ void kabsch_solve(const double H[9], const double ca[3], const double cb[3], float* T12, double* R9) {
  double A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[i][j] = H[3 * i + j];
  // H = U S V^T  <=>  one-sided Jacobi on the columns of H: H J1 J2 ... = U S, V = J1 J2 ...
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double al = 0, be = 0, ga = 0;
        for (int i = 0; i < 3; ++i) { al += A[i][p] * A[i][p]; be += A[i][q] * A[i][q]; ga += A[i][p] * A[i][q]; }
        off = fmax(off, fabs(ga) / (sqrt(al * be) + 1e-300));
        if (fabs(ga) <= 1e-300) continue;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int i = 0; i < 3; ++i) {
          const double ap = A[i][p], aq = A[i][q];
          A[i][p] = c * ap - s * aq; A[i][q] = s * ap + c * aq;
          const double vp = V[i][p], vq = V[i][q];
          V[i][p] = c * vp - s * vq; V[i][q] = s * vp + c * vq;
        }
      }
    if (off < 1e-15) break;
  }
  double sg[3];
  int ord[3] = {0, 1, 2};
  for (int j = 0; j < 3; ++j) sg[j] = sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
  for (int a = 0; a < 2; ++a)
    for (int b = a + 1; b < 3; ++b)
      if (sg[ord[b]] > sg[ord[a]]) { int tmp = ord[a]; ord[a] = ord[b]; ord[b] = tmp; }
  double U[3][3], Vs[3][3];
  for (int j = 0; j < 3; ++j) {
    const int c = ord[j];
    for (int i = 0; i < 3; ++i) { Vs[i][j] = V[i][c]; U[i][j] = sg[c] > 1e-300 ? A[i][c] / sg[c] : 0.0; }
  }
  // rank-deficient H: complete U to an orthonormal basis (the result is then not unique, as in the reference)
  const double smax = sg[ord[0]];
  if (sg[ord[1]] <= 1e-12 * smax || smax <= 1e-300) {
    if (smax <= 1e-300) { U[0][0] = 1; U[1][0] = 0; U[2][0] = 0; }
    const int m = fabs(U[0][0]) < 0.9 ? 0 : 1;     // any vector not parallel to u0
    double e[3] = {0, 0, 0};
    e[m] = 1;
    double dp = e[0] * U[0][0] + e[1] * U[1][0] + e[2] * U[2][0], nn = 0;
    for (int i = 0; i < 3; ++i) { U[i][1] = e[i] - dp * U[i][0]; nn += U[i][1] * U[i][1]; }
    nn = sqrt(nn);
    for (int i = 0; i < 3; ++i) U[i][1] /= nn;
  }
  if (sg[ord[2]] <= 1e-12 * smax || smax <= 1e-300) {
    U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
    U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
    U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
  }
  // d = det(V U^T) = det(V) det(U)
  auto det3 = [](const double M[3][3]) {
    return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
           M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
  };
  const double d = det3(Vs) * det3(U);
  double R[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[i][j] = Vs[i][0] * U[j][0] + Vs[i][1] * U[j][1] + d * Vs[i][2] * U[j][2];
  if constexpr (!PACK) {
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) R9[3 * i + j] = R[i][j];
    return;
  }
  for (int i = 0; i < 3; ++i) {
    const float r0 = (float)R[i][0], r1 = (float)R[i][1], r2 = (float)R[i][2];
    T12[4 * i] = r0; T12[4 * i + 1] = r1; T12[4 * i + 2] = r2;
    T12[4 * i + 3] = (float)(cb[i] - ((double)r0 * ca[0] + (double)r1 * ca[1] + (double)r2 * ca[2]));
  }
}

static __host__ __device__ void kabsch_from_H(const double H[9], const double ca[3], const double cb[3], float* T12) {
  kabsch_solve<true>(H, ca, cb, T12, nullptr);
}
static __host__ __device__ void kabsch_rotation(const double H[9], double R9[9]) { kabsch_solve<false>(H, nullptr, nullptr, nullptr, R9); }

}  // namespace gcl
