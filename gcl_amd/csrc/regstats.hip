// Per-pair registration statistics of a batch of pairs in ONE launch (gcl_registration_stats): the scoring half of the
// reference's SC2-PCR benchmark loops (scripts/SC2_PCR/test_KITTI.py:46-69, test_3DMatch.py:46-73, evaluate_metric.py
// TransformationLoss / ClassificationLoss), which there is ~25 small torch operations and three sklearn calls on host copies
// per pair.
//
// One workgroup of 256 threads per pair.  Thread t takes the correspondences t, t + 256, ... of its pair in ascending order:
//   - the two labels in fp32, as the reference forms them: w = R p + t (an fma chain over x, y, z), d = sqrt(dx^2 + dy^2 +
//     dz^2) in fp32, label = d < inlier_threshold -- under gt_trans (gt label) and under pred_trans (predicted label,
//     scripts/SC2_PCR/SC2_PCR.py:406-408);
//   - |R p + t - q| under pred_trans once more in fp64 from the fp32 inputs, for the RMSE column.
// The three counts are integers (exact, order-free); the fp64 sum is reduced in a fixed order (a thread's terms ascending,
// then a binary tree over the 256 threads in LDS), so a table is the same on every run.  Thread 0 forms RE, TE and the ratios
// in fp64 from the fp32 matrices and the integer counts.  No atomics, nothing read back.
#include "common.h"

#include <math.h>

namespace gcl {

constexpr int RS_THREADS = 256;

struct rs_pose {
  float r[9], t[3];
};
__device__ __forceinline__ rs_pose rs_load(const float* __restrict__ m16) {
  rs_pose T;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) T.r[3 * i + j] = m16[4 * i + j];
    T.t[i] = m16[4 * i + 3];
  }
  return T;
}
// |R p + t - q| in fp32: every product and sum rounded as written
__device__ __forceinline__ float rs_dist32(const rs_pose& T, float x, float y, float z, float qx, float qy, float qz) {
  const float dx = __builtin_fmaf(T.r[2], z, __builtin_fmaf(T.r[1], y, T.r[0] * x)) + T.t[0] - qx;
  const float dy = __builtin_fmaf(T.r[5], z, __builtin_fmaf(T.r[4], y, T.r[3] * x)) + T.t[1] - qy;
  const float dz = __builtin_fmaf(T.r[8], z, __builtin_fmaf(T.r[7], y, T.r[6] * x)) + T.t[2] - qz;
  return sqrtf(__builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)));
}
__device__ __forceinline__ double rs_dist64(const rs_pose& T, float x, float y, float z, float qx, float qy, float qz) {
  const double X = x, Y = y, Z = z;
  const double dx = (double)T.r[0] * X + (double)T.r[1] * Y + (double)T.r[2] * Z + (double)T.t[0] - (double)qx;
  const double dy = (double)T.r[3] * X + (double)T.r[4] * Y + (double)T.r[5] * Z + (double)T.t[1] - (double)qy;
  const double dz = (double)T.r[6] * X + (double)T.r[7] * Y + (double)T.r[8] * Z + (double)T.t[2] - (double)qz;
  return sqrt(dx * dx + dy * dy + dz * dz);
}

__global__ void __launch_bounds__(RS_THREADS) k_registration_stats(
    const float* __restrict__ src, const float* __restrict__ tgt, int n_cap, const int* __restrict__ counts,
    const float* __restrict__ pred_trans, const float* __restrict__ gt_trans, float inlier_threshold, double re_thre,
    double te_thre, double* __restrict__ stats, float* __restrict__ pred_labels, float* __restrict__ gt_labels) {
  __shared__ int s_cnt[3][RS_THREADS];
  __shared__ double s_sum[RS_THREADS];
  const int b = blockIdx.x, t = threadIdx.x;
  int n = counts ? counts[b] : n_cap;
  n = n < 0 ? 0 : (n > n_cap ? n_cap : n);
  const rs_pose P = rs_load(pred_trans + 16 * (long long)b), G = rs_load(gt_trans + 16 * (long long)b);
  const float* __restrict__ s = src + 3 * (long long)b * n_cap;
  const float* __restrict__ q = tgt + 3 * (long long)b * n_cap;
  int n_gt = 0, n_pred = 0, n_both = 0;
  double sum = 0.0;
  for (int i = t; i < n_cap; i += RS_THREADS) {
    float lp = 0.f, lg = 0.f;
    if (i < n) {                                       // rows at or beyond the pair's count are never read
      const float x = s[3 * i], y = s[3 * i + 1], z = s[3 * i + 2];
      const float qx = q[3 * i], qy = q[3 * i + 1], qz = q[3 * i + 2];
      const bool g = rs_dist32(G, x, y, z, qx, qy, qz) < inlier_threshold;
      const bool p = rs_dist32(P, x, y, z, qx, qy, qz) < inlier_threshold;
      n_gt += g;
      n_pred += p;
      n_both += g && p;
      sum += rs_dist64(P, x, y, z, qx, qy, qz);
      lp = p ? 1.f : 0.f;
      lg = g ? 1.f : 0.f;
    }
    if (pred_labels) pred_labels[(long long)b * n_cap + i] = lp;
    if (gt_labels) gt_labels[(long long)b * n_cap + i] = lg;
  }
  s_cnt[0][t] = n_gt;
  s_cnt[1][t] = n_pred;
  s_cnt[2][t] = n_both;
  s_sum[t] = sum;
  __syncthreads();
  for (int w = RS_THREADS / 2; w > 0; w >>= 1) {       // fixed tree: the same sum on every run
    if (t < w) {
      s_cnt[0][t] += s_cnt[0][t + w];
      s_cnt[1][t] += s_cnt[1][t + w];
      s_cnt[2][t] += s_cnt[2][t + w];
      s_sum[t] += s_sum[t + w];
    }
    __syncthreads();
  }
  if (t != 0) return;
  n_gt = s_cnt[0][0];
  n_pred = s_cnt[1][0];
  n_both = s_cnt[2][0];
  double trace = 0.0, te2 = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) trace += (double)P.r[k] * (double)G.r[k];          // trace(R^T R_gt)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double d = (double)P.t[k] - (double)G.t[k];
    te2 += d * d;
  }
  double cosv = (trace - 1.0) / 2.0;
  cosv = cosv < -1.0 ? -1.0 : (cosv > 1.0 ? 1.0 : cosv);
  const double re = acos(cosv) * 180.0 / 3.14159265358979323846;
  const double te = 100.0 * sqrt(te2);
  double* o = stats + 10 * (long long)b;
  o[0] = (re < re_thre && te < te_thre) ? 1.0 : 0.0;
  o[1] = re;
  o[2] = te;
  o[3] = (double)n_gt;
  o[4] = n > 0 ? (double)n_gt / (double)n : 0.0;
  o[5] = (double)n_both;
  o[6] = n_pred > 0 ? (double)n_both / (double)n_pred : 0.0;                     // sklearn: zero division -> 0
  o[7] = n_gt > 0 ? (double)n_both / (double)n_gt : 0.0;
  o[8] = (n_pred + n_gt) > 0 ? 2.0 * (double)n_both / ((double)n_pred + (double)n_gt) : 0.0;
  o[9] = n > 0 ? s_sum[0] / (double)n : 0.0;
}

}  // namespace gcl

using namespace gcl;

extern "C" {

int gcl_registration_stats(const float* src_corr, const float* tgt_corr, int32_t batch, int32_t n_cap, const int32_t* counts,
                           const float* pred_trans, const float* gt_trans, float inlier_threshold, float re_thre,
                           float te_thre, double* stats, float* pred_labels, float* gt_labels, void* stream) {
  GCL_CHECK_ARG(batch >= 0 && n_cap >= 0, "gcl_registration_stats: negative size (batch = %d, n_cap = %d)", batch, n_cap);
  GCL_CHECK_ARG(pred_trans && gt_trans && stats, "gcl_registration_stats: null pointer (pred_trans, gt_trans or stats)");
  GCL_CHECK_ARG(n_cap == 0 || (src_corr && tgt_corr), "gcl_registration_stats: null pointer (src_corr or tgt_corr)");
  if (batch == 0) return GCL_OK;
  hipLaunchKernelGGL(k_registration_stats, dim3((unsigned)batch), dim3(RS_THREADS), 0, (hipStream_t)stream, src_corr,
                     tgt_corr, n_cap, counts, pred_trans, gt_trans, inlier_threshold, (double)re_thre, (double)te_thre, stats,
                     pred_labels, gt_labels);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

}  // extern "C"
