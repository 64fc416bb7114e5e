// The validation step's arithmetic for a ragged batch of pairs (lib/colocation_trainer.py:306-379 of the reference calls it
// once per pair on the host): the robust pose of util/transform_estimation.py:97-126 and the five per-pair meters.
//
//   gcl_irls_pose_batch  one workgroup per pair.  The algorithm of gcl_amd/util/transform_estimation.py::
//                        est_quad_linear_robust in fp64: n_iter re-weighted Gauss-Newton steps on
//                        w^2 [-[p]x | I] x = w^2 (q - p), each solved through its 6 x 6 normal equations with partial
//                        pivoting, the step applied as Rz Ry Rx + t, w = par / (|p - q| + par), par halved every
//                        halve_every steps, trans = step trans.  A thread owns the rows t, t + VP_THREADS, ... of its pair
//                        for the whole call, so the current points (fp64, in the caller's scratch) are only ever read by
//                        the thread that wrote them.  One pass over the rows per step: move the row by the previous step,
//                        weigh it, add its terms.
//                        The normal matrix [[ |p|^2 I - p p^T, [p]x ], [ -[p]x, I ]] summed with w^2 and its right-hand side
//                        (p x d, d) hold 16 distinct sums (6 second moments, 3 first moments, the weight, 6 of the
//                        right-hand side); the other entries are copies, negations or zero.  Each sum is reduced in a fixed
//                        order: a thread's rows ascending, the xor butterfly over the wave, the waves ascending in LDS.  No
//                        atomics: a pair's result does not depend on the run or on what else is in the batch.
//   gcl_val_stats_batch  one workgroup per pair: corr_dist over the pair's first cloud, RTE, RRE and the hit ratio of its
//                        correspondences, in fp64 from the fp32 points; integer counts, the one fp64 sum over a fixed tree.
//
// Every loop is bounded by n_iter, 6, the block size or the pair's row count; a pair whose offsets do not lie in
// 0 <= lo <= hi <= total is treated as empty, so no row outside the arrays is ever addressed.
#include "common.h"

#include <math.h>

// every product and sum is rounded on its own (the host function and the numpy restatements round them so)
#pragma clang fp contract(off)

namespace gcl {

constexpr int VP_THREADS = 512, VP_WAVES = VP_THREADS / 64;
constexpr int VP_SUMS = 16;
constexpr int VS_THREADS = 256;
// a pivot below this fraction of the largest entry its column had before elimination is a zero pivot: a rank-deficient
// system (all rows equal, all rows on a line) leaves rounding residue of ~1e-16 of that size where exact arithmetic leaves 0
constexpr double VP_PIVOT_REL = 0x1p-40;

struct vp_step {
  double r[9], t[3];
};

// x of M x = g by Gaussian elimination with partial pivoting on the augmented rows a[6][7] (LDS: the pivot row is indexed
// by a run-time value); false: a zero or non-finite pivot, or a non-finite solution
__device__ bool vp_solve6(double (*a)[7], double* x) {
  double colmax[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double m = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) m = fmax(m, fabs(a[r][c]));
    colmax[c] = m;
  }
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    int piv = c;
    double best = fabs(a[c][c]);
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      const double v = fabs(a[r][c]);
      if (v > best) {
        best = v;
        piv = r;
      }
    }
    if (piv != c) {
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const double tmp = a[c][k];
        a[c][k] = a[piv][k];
        a[piv][k] = tmp;
      }
    }
    const double p = a[c][c];
    if (!(fabs(p) > VP_PIVOT_REL * colmax[c]) || !isfinite(p)) {      // also catches NaN and an all-zero column
      ok = false;
      a[c][c] = 1.0;                                                   // keep going on fixed bounds; the result is discarded
    }
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      const double f = a[r][c] / a[c][c];
#pragma unroll
      for (int k = c; k < 7; ++k) a[r][k] -= f * a[c][k];
    }
  }
#pragma unroll
  for (int c = 5; c >= 0; --c) {
    double s = a[c][6];
#pragma unroll
    for (int k = c + 1; k < 6; ++k) s -= a[c][k] * x[k];
    x[c] = s / a[c][c];
    ok = ok && isfinite(x[c]);
  }
  return ok;
}

// R = Rz(x2) Ry(x1) Rx(x0), t = x[3:]
__device__ void vp_get_trans(const double* x, vp_step& s) {
  const double cx = cos(x[0]), sx = sin(x[0]), cy = cos(x[1]), sy = sin(x[1]), cz = cos(x[2]), sz = sin(x[2]);
  s.r[0] = cz * cy;
  s.r[1] = cz * sy * sx - sz * cx;
  s.r[2] = cz * sy * cx + sz * sx;
  s.r[3] = sz * cy;
  s.r[4] = sz * sy * sx + cz * cx;
  s.r[5] = sz * sy * cx - cz * sx;
  s.r[6] = -sy;
  s.r[7] = cy * sx;
  s.r[8] = cy * cx;
  s.t[0] = x[3];
  s.t[1] = x[4];
  s.t[2] = x[5];
}

__device__ __forceinline__ void vp_identity16(double* T) {
  for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.0 : 0.0;
}

__global__ void __launch_bounds__(VP_THREADS) k_irls_pose(
    const float* __restrict__ src, const float* __restrict__ tgt, long long total, const long long* __restrict__ offsets,
    const float* __restrict__ weight, int n_iter, double par0, int halve_every, double* __restrict__ cur,
    double* __restrict__ T_out, int* __restrict__ status) {
  __shared__ double s_part[VP_SUMS][VP_WAVES];
  __shared__ double s_sum[VP_SUMS];
  __shared__ double s_a[6][7];
  __shared__ vp_step s_step, s_tr;
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  long long lo = offsets[b], hi = offsets[b + 1];
  if (!(lo >= 0 && hi > lo && hi <= total)) {            // an empty pair (or offsets outside the arrays): no row is touched
    if (t == 0) {
      vp_identity16(T_out + 16 * (long long)b);
      status[b] = 1;
    }
    return;
  }
  if (t == 0) {                                          // the accumulated transform: thread 0's, kept out of registers
    for (int k = 0; k < 9; ++k) s_tr.r[k] = (k % 4 == 0) ? 1.0 : 0.0;
    s_tr.t[0] = s_tr.t[1] = s_tr.t[2] = 0.0;
  }
  bool bad = false;
  double par = par0;                                     // the par that weighs the rows of the step being summed
  for (int it = 0; it < n_iter; ++it) {
    vp_step st;
    if (it > 0) st = s_step;
    double acc[VP_SUMS];
#pragma unroll
    for (int k = 0; k < VP_SUMS; ++k) acc[k] = 0.0;
    for (long long i = lo + t; i < hi; i += VP_THREADS) {
      const double qx = tgt[3 * i], qy = tgt[3 * i + 1], qz = tgt[3 * i + 2];
      double px, py, pz, w;
      if (it == 0) {
        px = src[3 * i];
        py = src[3 * i + 1];
        pz = src[3 * i + 2];
        w = weight ? (double)weight[i] : 1.0;
      } else {
        const double x = cur[3 * i], y = cur[3 * i + 1], z = cur[3 * i + 2];
        px = x * st.r[0] + y * st.r[1] + z * st.r[2] + st.t[0];
        py = x * st.r[3] + y * st.r[4] + z * st.r[5] + st.t[1];
        pz = x * st.r[6] + y * st.r[7] + z * st.r[8] + st.t[2];
        const double ex = px - qx, ey = py - qy, ez = pz - qz;
        w = par / (sqrt(ex * ex + ey * ey + ez * ez) + par);
      }
      cur[3 * i] = px;
      cur[3 * i + 1] = py;
      cur[3 * i + 2] = pz;
      const double w2 = w * w, dx = qx - px, dy = qy - py, dz = qz - pz;
      const double wx = w2 * px, wy = w2 * py, wz = w2 * pz;
      acc[0] += wx * px;
      acc[1] += wy * py;
      acc[2] += wz * pz;
      acc[3] += wx * py;
      acc[4] += wx * pz;
      acc[5] += wy * pz;
      acc[6] += wx;
      acc[7] += wy;
      acc[8] += wz;
      acc[9] += w2;
      acc[10] += wy * dz - wz * dy;                      // w^2 (p x d)
      acc[11] += wz * dx - wx * dz;
      acc[12] += wx * dy - wy * dx;
      acc[13] += w2 * dx;
      acc[14] += w2 * dy;
      acc[15] += w2 * dz;
    }
    if (it > 0 && it % halve_every == 0) par *= 0.5;     // from here on: the par of step `it`, which weighs step it + 1's rows
#pragma unroll
    for (int k = 0; k < VP_SUMS; ++k) {
      const double v = wave_sum(acc[k]);
      if (lane == 0) s_part[k][wave] = v;
    }
    __syncthreads();
    if (t < VP_SUMS) {
      double v = s_part[t][0];
      for (int w_ = 1; w_ < VP_WAVES; ++w_) v += s_part[t][w_];
      s_sum[t] = v;
    }
    __syncthreads();
    if (t == 0) {
      const double xx = s_sum[0], yy = s_sum[1], zz = s_sum[2], xy = s_sum[3], xz = s_sum[4], yz = s_sum[5];
      const double sx = s_sum[6], sy = s_sum[7], sz = s_sum[8], sw = s_sum[9];
      const double m[6][6] = {{yy + zz, -xy, -xz, 0.0, -sz, sy}, {-xy, xx + zz, -yz, sz, 0.0, -sx},
                              {-xz, -yz, xx + yy, -sy, sx, 0.0}, {0.0, sz, -sy, sw, 0.0, 0.0},
                              {-sz, 0.0, sx, 0.0, sw, 0.0},      {sy, -sx, 0.0, 0.0, 0.0, sw}};
      for (int r = 0; r < 6; ++r) {
        for (int c = 0; c < 6; ++c) s_a[r][c] = m[r][c];
        s_a[r][6] = s_sum[10 + r];
      }
      double x[6];
      const bool ok = vp_solve6(s_a, x);
      vp_step s;
      vp_get_trans(x, s);
      if (!ok || bad) {                                  // flagged: the remaining steps run on the identity, on the same bounds
        bad = true;
        for (int k = 0; k < 9; ++k) s.r[k] = (k % 4 == 0) ? 1.0 : 0.0;
        s.t[0] = s.t[1] = s.t[2] = 0.0;
      }
      const vp_step tr = s_tr;
      vp_step nt;                                        // trans = step trans
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c)
          nt.r[3 * r + c] = s.r[3 * r] * tr.r[c] + s.r[3 * r + 1] * tr.r[3 + c] + s.r[3 * r + 2] * tr.r[6 + c];
        nt.t[r] = s.r[3 * r] * tr.t[0] + s.r[3 * r + 1] * tr.t[1] + s.r[3 * r + 2] * tr.t[2] + s.t[r];
      }
      s_tr = nt;
      s_step = s;
    }
    __syncthreads();
  }
  if (t != 0) return;
  double* T = T_out + 16 * (long long)b;
  vp_identity16(T);
  if (!bad) {
    const vp_step tr = s_tr;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) T[4 * r + c] = tr.r[3 * r + c];
      T[4 * r + 3] = tr.t[r];
    }
  }
  status[b] = bad ? 1 : 0;
}

__global__ void __launch_bounds__(VS_THREADS) k_val_stats(
    const float* __restrict__ src, const float* __restrict__ tgt, long long total, const long long* __restrict__ offsets,
    const float* __restrict__ xyz0, long long total0, const long long* __restrict__ offsets0,
    const double* __restrict__ T_est, const double* __restrict__ T_gt, const int* __restrict__ status, double max_dist,
    double thresh, double* __restrict__ out) {
  __shared__ int s_cnt[VS_THREADS];
  __shared__ double s_sum[VS_THREADS];
  const int b = blockIdx.x, t = threadIdx.x;
  double E[12], G[12];                                   // rows of [R | t]
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) {
      E[4 * r + c] = T_est[16 * (long long)b + 4 * r + c];
      G[4 * r + c] = T_gt[16 * (long long)b + 4 * r + c];
    }
  long long lo = offsets[b], hi = offsets[b + 1];
  if (!(lo >= 0 && hi >= lo && hi <= total)) lo = hi = 0;
  long long lo0 = offsets0[b], hi0 = offsets0[b + 1];
  if (!(lo0 >= 0 && hi0 >= lo0 && hi0 <= total0)) lo0 = hi0 = 0;
  int hits = 0;
  for (long long i = lo + t; i < hi; i += VS_THREADS) {
    const double x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
    const double dx = G[0] * x + G[1] * y + G[2] * z + G[3] - (double)tgt[3 * i];
    const double dy = G[4] * x + G[5] * y + G[6] * z + G[7] - (double)tgt[3 * i + 1];
    const double dz = G[8] * x + G[9] * y + G[10] * z + G[11] - (double)tgt[3 * i + 2];
    hits += sqrt(dx * dx + dy * dy + dz * dz + 1e-6) < thresh;
  }
  double sum = 0.0;
  for (long long i = lo0 + t; i < hi0; i += VS_THREADS) {
    const double x = xyz0[3 * i], y = xyz0[3 * i + 1], z = xyz0[3 * i + 2];
    const double dx = (E[0] * x + E[1] * y + E[2] * z + E[3]) - (G[0] * x + G[1] * y + G[2] * z + G[3]);
    const double dy = (E[4] * x + E[5] * y + E[6] * z + E[7]) - (G[4] * x + G[5] * y + G[6] * z + G[7]);
    const double dz = (E[8] * x + E[9] * y + E[10] * z + E[11]) - (G[8] * x + G[9] * y + G[10] * z + G[11]);
    sum += fmin(sqrt(dx * dx + dy * dy + dz * dz), max_dist);
  }
  s_cnt[t] = hits;
  s_sum[t] = sum;
  __syncthreads();
  for (int w = VS_THREADS / 2; w > 0; w >>= 1) {         // fixed tree: the same sum on every run
    if (t < w) {
      s_cnt[t] += s_cnt[t + w];
      s_sum[t] += s_sum[t + w];
    }
    __syncthreads();
  }
  if (t != 0) return;
  double trace = 0.0, te2 = 0.0;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) trace += E[4 * r + c] * G[4 * r + c];      // trace(R_est^T R_gt)
    const double d = E[4 * r + 3] - G[4 * r + 3];
    te2 += d * d;
  }
  const long long n = hi - lo, n0 = hi0 - lo0;
  double* o = out + 6 * (long long)b;
  o[0] = n0 > 0 ? s_sum[0] / (double)n0 : 0.0;
  o[1] = sqrt(te2);
  o[2] = acos((trace - 1.0) / 2.0);                       // no clamp: NaN (trace > 3 by rounding) is the caller's signal
  o[3] = n > 0 ? (double)((float)s_cnt[0] / (float)n) : 0.0;     // the reference's float32 mean of 0 / 1 values, bit for bit
  o[4] = (double)n;
  o[5] = status ? (double)status[b] : 0.0;
}

}  // namespace gcl

using namespace gcl;

extern "C" {

int64_t gcl_irls_pose_scratch_len(int64_t total) { return total > 0 ? 3 * total : 0; }

int gcl_irls_pose_batch(const float* src, const float* tgt, int64_t total, const int64_t* offsets, int32_t B,
                        const float* weight, int32_t n_iter, double par0, int32_t halve_every, double* scratch, double* T,
                        int32_t* status, void* stream) {
  GCL_CHECK_ARG(B >= 1, "gcl_irls_pose_batch: B = %d (at least one pair)", B);
  GCL_CHECK_ARG(total >= 0, "gcl_irls_pose_batch: total = %lld is negative", (long long)total);
  GCL_CHECK_ARG(n_iter >= 0, "gcl_irls_pose_batch: n_iter = %d is negative", n_iter);
  GCL_CHECK_ARG(par0 > 0.0, "gcl_irls_pose_batch: par0 = %g (must be positive)", par0);
  GCL_CHECK_ARG(halve_every >= 1, "gcl_irls_pose_batch: halve_every = %d (at least 1)", halve_every);
  GCL_CHECK_ARG(offsets && T && status, "gcl_irls_pose_batch: null pointer (offsets, T or status)");
  GCL_CHECK_ARG(total == 0 || (src && tgt), "gcl_irls_pose_batch: null pointer (src or tgt)");
  GCL_CHECK_ARG(total == 0 || scratch, "gcl_irls_pose_batch: null pointer (scratch: 3 * total doubles)");
  hipLaunchKernelGGL(k_irls_pose, dim3((unsigned)B), dim3(VP_THREADS), 0, (hipStream_t)stream, src, tgt, (long long)total,
                     (const long long*)offsets, weight, n_iter, par0, halve_every, scratch, T, status);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_val_stats_batch(const float* src, const float* tgt, int64_t total, const int64_t* offsets, const float* xyz0,
                        int64_t total0, const int64_t* offsets0, int32_t B, const double* T_est, const double* T_gt,
                        const int32_t* status, double max_dist, double thresh, double* out, void* stream) {
  GCL_CHECK_ARG(B >= 1, "gcl_val_stats_batch: B = %d (at least one pair)", B);
  GCL_CHECK_ARG(total >= 0 && total0 >= 0, "gcl_val_stats_batch: negative size (total = %lld, total0 = %lld)",
                (long long)total, (long long)total0);
  GCL_CHECK_ARG(offsets && offsets0 && T_est && T_gt && out,
                "gcl_val_stats_batch: null pointer (offsets, offsets0, T_est, T_gt or out)");
  GCL_CHECK_ARG(total == 0 || (src && tgt), "gcl_val_stats_batch: null pointer (src or tgt)");
  GCL_CHECK_ARG(total0 == 0 || xyz0, "gcl_val_stats_batch: null pointer (xyz0)");
  hipLaunchKernelGGL(k_val_stats, dim3((unsigned)B), dim3(VS_THREADS), 0, (hipStream_t)stream, src, tgt, (long long)total,
                     (const long long*)offsets, xyz0, (long long)total0, (const long long*)offsets0, T_est, T_gt, status,
                     max_dist, thresh, out);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

}  // extern "C"
