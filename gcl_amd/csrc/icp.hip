// Point-to-point ICP for a ragged batch of scan pairs: open3d's RegistrationICP with TransformationEstimationPointToPoint
// as the pair loaders call it to refine the odometry pose (lib/data_loaders.py:447-474, lib/complement_data_loader.py:369-399)
// and as scripts/SC2_PCR/benchmark_utils.py:40-56 offers it.  All arithmetic is fp64 from the fp32 points (DESIGN.md "ICP").
//
//   k_icp_setup   the target points once in sorted-cell order (x, y, z, the row within the pair's own target), so that a
//                 cell's candidates are contiguous; T = init, the pairs' control words, the pairs' first blocks.
//   k_icp_step    the correspondences under the current T and their 17 sums.  A block serves ICP_QB consecutive source rows
//                 of ONE pair, counted from the pair's own first row; ICP_LPQ = 16 lanes serve one query: the 27 cells
//                 around p = T x are 9 runs of the pair's sorted keys (fpgrid.h), read as one stream of candidates, the
//                 minimum of (d2, row) taken over the lanes.  The query's result goes to its LDS slot; then thread t forms the
//                 17 terms of row t, the waves add them in a butterfly and the four waves are added in wave order: one partial
//                 per block, no atomics.
//   k_icp_update  one workgroup per pair: the partials added in block order, fitness / rmse, status and convergence rules,
//                 the Kabsch update (kabsch.h) and T <- U T; sets the pair's `done` word.
//
// Blocks of a finished pair return on reading `done`.  Every candidate position comes out of a binary search over the pair's
// own key range and is used as a position in that range only; the row stored beside a point is compared and written, never
// dereferenced.  The search of k_icp_step has a TWIN in multiway.hip (k_info_step): a change to one belongs in both.
#include "common.h"
#include "fpgrid.h"
#include "kabsch.h"

#include <math.h>

namespace gcl {

constexpr int ICP_QB = 256;             // source rows per block = threads per block
constexpr int ICP_LPQ = 16;             // lanes per query: 1 and 64 were measured slower (profiles/icp_probe.txt)
constexpr int ICP_SUMS = 17;            // sum p (3), sum q (3), sum p q^T (9), sum d2, n
constexpr int ICP_MAX_ITERATION = 1000000;

__global__ void __launch_bounds__(256) k_icp_setup(const float* __restrict__ xyz1, long long total1,
                                                   const long long* __restrict__ off0, const long long* __restrict__ off1, int B,
                                                   const long long* __restrict__ skeys, const long long* __restrict__ order,
                                                   const double* __restrict__ init, float4* __restrict__ sorted,
                                                   long long* __restrict__ blk_off, int* __restrict__ done,
                                                   double* __restrict__ T, double* __restrict__ stats, int* __restrict__ status) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < total1) {
    const long long j = order[i];
    int b = (int)(skeys[i] >> 48);
    b = b < 0 ? 0 : (b >= B ? B - 1 : b);
    float4 v = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
    if (j >= 0 && j < total1) v = make_float4(xyz1[3 * j], xyz1[3 * j + 1], xyz1[3 * j + 2], __int_as_float((int)(j - off1[b])));
    sorted[i] = v;
  }
  if (i < B) {
    for (int c = 0; c < 16; ++c) T[16 * i + c] = init[16 * i + c];
    for (int c = 0; c < 4; ++c) stats[4 * i + c] = 0.0;
    done[i] = 0;
    status[i] = 0;
  }
  if (i == 0) {
    long long acc = 0;
    blk_off[0] = 0;
    for (int b = 0; b < B; ++b) {
      const long long n0 = off0[b + 1] - off0[b];
      acc += n0 > 0 ? (n0 + ICP_QB - 1) / ICP_QB : 0;
      blk_off[b + 1] = acc;
    }
  }
}

// (d2, row) of a is below that of b
__device__ __forceinline__ bool icp_less(double da, int ra, double db, int rb) { return da < db || (da == db && ra < rb); }

__global__ void __launch_bounds__(ICP_QB) k_icp_step(const float* __restrict__ xyz0, const long long* __restrict__ off0,
                                                     const long long* __restrict__ off1, int B,
                                                     const long long* __restrict__ blk_off, const float4* __restrict__ sorted,
                                                     const long long* __restrict__ skeys, const double* __restrict__ T,
                                                     const int* __restrict__ done, double inv_edge, double r2,
                                                     double* __restrict__ partials, int* __restrict__ corr) {
  __shared__ double s_d2[ICP_QB];
  __shared__ int s_pos[ICP_QB];                       // the correspondence's position in the pair's sorted targets, -1: none
  __shared__ int s_row[ICP_QB];
  __shared__ double s_wave[ICP_QB / 64][ICP_SUMS];
  const int b = fp_cloud_of(blk_off, B, (long long)blockIdx.x);
  if (done[b]) return;                                // block-uniform
  const long long row0 = off0[b] + ((long long)blockIdx.x - blk_off[b]) * ICP_QB;
  const long long rows = off0[b + 1] - row0;
  const int nq = rows < ICP_QB ? (int)rows : ICP_QB;  // this block's queries
  const long long t_lo = off1[b];
  const int n1 = (int)(off1[b + 1] - t_lo);
  const long long* __restrict__ keys = skeys + t_lo;
  const float4* __restrict__ tgt = sorted + t_lo;
  double M[12];
#pragma unroll
  for (int c = 0; c < 12; ++c) M[c] = T[16 * b + c];

  // group g of LPQ lanes serves the slots g, g + GROUPS, ...: LPQ rounds cover the block's ICP_QB rows
  constexpr int LPQ = ICP_LPQ, GROUPS = ICP_QB / LPQ;
  const int g = threadIdx.x / LPQ, l = threadIdx.x % LPQ;
  for (int round = 0; round < LPQ; ++round) {
    const int slot = round * GROUPS + g;
    if (slot >= nq) continue;                         // uniform over the group's lanes
    const float* x = xyz0 + 3 * (row0 + slot);
    const double x0 = x[0], x1 = x[1], x2 = x[2];
    const double px = M[0] * x0 + M[1] * x1 + M[2] * x2 + M[3];
    const double py = M[4] * x0 + M[5] * x1 + M[6] * x2 + M[7];
    const double pz = M[8] * x0 + M[9] * x1 + M[10] * x2 + M[11];
    const int cx = fp_cell(px, inv_edge), cy = fp_cell(py, inv_edge), cz = fp_cell(pz, inv_edge);
    const int z0 = cz > FP_CELL_MIN ? cz - 1 : cz, z1 = cz < FP_CELL_MAX ? cz + 1 : cz;
    double best = INFINITY;
    int best_row = 0x7fffffff, best_pos = -1;
    // lanes 0 .. 8: the run of column (cx + l % 3 - 1, cy + l / 3 - 1), z cells z0 .. z1
    int run_lo = 0, run_len = 0;
    if (l < 9) {
      const int cxx = cx + l % 3 - 1, cyy = cy + l / 3 - 1;
      if (cxx >= FP_CELL_MIN && cxx <= FP_CELL_MAX && cyy >= FP_CELL_MIN && cyy <= FP_CELL_MAX) {
        run_lo = (int)fp_lower_bound(keys, n1, fp_key(b, cxx, cyy, z0));
        const int run_hi = (int)fp_lower_bound(keys, n1, fp_key(b, cxx, cyy, z1) + 1);
        run_len = run_hi > run_lo ? run_hi - run_lo : 0;
      }
    }
    int lo9[9], pre9[10];
    pre9[0] = 0;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      lo9[r] = __shfl(run_lo, r, LPQ);
      pre9[r + 1] = pre9[r] + __shfl(run_len, r, LPQ);
    }
    const int total = pre9[9] < n1 ? pre9[9] : n1;  // the runs are disjoint: never more than n1 candidates
    for (int c0 = l; c0 < total; c0 += LPQ) {
      int s = lo9[0] + c0;
#pragma unroll
      for (int r = 1; r < 9; ++r)
        if (c0 >= pre9[r]) s = lo9[r] + (c0 - pre9[r]);
      if (s < 0 || s >= n1) continue;
      const float4 c = tgt[s];
      const double d = fp_d2(px, py, pz, c.x, c.y, c.z);
      const int row = __float_as_int(c.w);
      if (d <= r2 && icp_less(d, row, best, best_row)) { best = d; best_row = row; best_pos = s; }
    }
#pragma unroll
    for (int o = LPQ / 2; o > 0; o >>= 1) {
      const double od = __shfl_xor(best, o, LPQ);
      const int orow = __shfl_xor(best_row, o, LPQ), opos = __shfl_xor(best_pos, o, LPQ);
      if (opos >= 0 && icp_less(od, orow, best, best_row)) { best = od; best_row = orow; best_pos = opos; }
    }
    if (l == 0) { s_d2[slot] = best; s_pos[slot] = best_pos; s_row[slot] = best_row; }
  }
  __syncthreads();

  // thread t: the 17 terms of row t
  double v[ICP_SUMS];
#pragma unroll
  for (int c = 0; c < ICP_SUMS; ++c) v[c] = 0.0;
  const int t = threadIdx.x;
  if (t < nq) {
    const int pos = s_pos[t];
    if (pos >= 0 && pos < n1) {
      const float* x = xyz0 + 3 * (row0 + t);
      const double x0 = x[0], x1 = x[1], x2 = x[2];
      const double p[3] = {M[0] * x0 + M[1] * x1 + M[2] * x2 + M[3], M[4] * x0 + M[5] * x1 + M[6] * x2 + M[7],
                           M[8] * x0 + M[9] * x1 + M[10] * x2 + M[11]};
      const float4 c = tgt[pos];
      const double q[3] = {c.x, c.y, c.z};
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        v[a] = p[a];
        v[3 + a] = q[a];
#pragma unroll
        for (int e = 0; e < 3; ++e) v[6 + 3 * a + e] = p[a] * q[e];
      }
      v[15] = s_d2[t];
      v[16] = 1.0;
    }
    if (corr) corr[row0 + t] = (pos >= 0 && pos < n1) ? s_row[t] : -1;
  }
#pragma unroll
  for (int c = 0; c < ICP_SUMS; ++c) v[c] = wave_sum(v[c]);
  if ((t & 63) == 0)
#pragma unroll
    for (int c = 0; c < ICP_SUMS; ++c) s_wave[t >> 6][c] = v[c];
  __syncthreads();
  if (t < ICP_SUMS) {
    double s = s_wave[0][t];
    for (int w = 1; w < ICP_QB / 64; ++w) s += s_wave[w][t];
    partials[(long long)blockIdx.x * ICP_SUMS + t] = s;
  }
}

constexpr int ICP_UPD_THREADS = 256, ICP_UPD_CHUNK = 64;   // partials staged through LDS, 64 blocks at a time

__global__ void __launch_bounds__(ICP_UPD_THREADS) k_icp_update(const long long* __restrict__ off0,
                                                                const long long* __restrict__ blk_off,
                                                                const double* __restrict__ partials, int it, int max_iteration,
                                                                double rel_fitness, double rel_rmse, int* __restrict__ done,
                                                                double* __restrict__ T, double* __restrict__ stats,
                                                                int* __restrict__ status) {
  __shared__ double s_part[ICP_UPD_CHUNK * ICP_SUMS];
  __shared__ double s_sum[ICP_SUMS];
  const int b = blockIdx.x;
  if (done[b]) return;                                 // block-uniform
  const int t = threadIdx.x;
  // the partials in block order: every thread fetches (one latency per chunk), thread c < 17 adds entry c of block after block
  double s = 0.0;
  const long long k_hi = blk_off[b + 1];
  for (long long k0 = blk_off[b]; k0 < k_hi; k0 += ICP_UPD_CHUNK) {
    const int blocks = k_hi - k0 < ICP_UPD_CHUNK ? (int)(k_hi - k0) : ICP_UPD_CHUNK;
    for (int i = t; i < blocks * ICP_SUMS; i += ICP_UPD_THREADS) s_part[i] = partials[k0 * ICP_SUMS + i];
    __syncthreads();
    if (t < ICP_SUMS)
      for (int u = 0; u < blocks; ++u) s += s_part[u * ICP_SUMS + t];
    __syncthreads();
  }
  if (t < ICP_SUMS) s_sum[t] = s;
  __syncthreads();
  if (t != 0) return;
  const double n = s_sum[16];
  const long long n0 = off0[b + 1] - off0[b];
  const double fitness = n0 > 0 ? n / (double)n0 : 0.0;
  const double rmse = n > 0.0 ? sqrt(s_sum[15] / n) : 0.0;
  const double prev_fitness = stats[4 * b], prev_rmse = stats[4 * b + 1];
  stats[4 * b] = fitness;
  stats[4 * b + 1] = rmse;
  stats[4 * b + 2] = n;
  stats[4 * b + 3] = (double)it;                       // updates applied to init so far
  const int st = n == 0.0 ? 1 : (n < 3.0 ? 2 : 0);
  const bool converged = it > 0 && fabs(fitness - prev_fitness) < rel_fitness && fabs(rmse - prev_rmse) < rel_rmse;
  if (st != 0 || converged || it >= max_iteration) {
    status[b] = st;
    done[b] = 1;
    return;
  }
  double mp[3], mq[3], H[9], R[9];
  for (int a = 0; a < 3; ++a) { mp[a] = s_sum[a] / n; mq[a] = s_sum[3 + a] / n; }
  for (int a = 0; a < 3; ++a)
    for (int e = 0; e < 3; ++e) H[3 * a + e] = s_sum[6 + 3 * a + e] - n * mp[a] * mq[e];
  kabsch_rotation(H, R);
  double U[3][4], Tn[12];
  for (int a = 0; a < 3; ++a) {
    for (int e = 0; e < 3; ++e) U[a][e] = R[3 * a + e];
    U[a][3] = mq[a] - (R[3 * a] * mp[0] + R[3 * a + 1] * mp[1] + R[3 * a + 2] * mp[2]);
  }
  double* Tb = T + 16 * b;
  for (int a = 0; a < 3; ++a)
    for (int c = 0; c < 4; ++c)
      Tn[4 * a + c] = U[a][0] * Tb[c] + U[a][1] * Tb[4 + c] + U[a][2] * Tb[8 + c] + U[a][3] * Tb[12 + c];
  for (int c = 0; c < 12; ++c) Tb[c] = Tn[c];
}

static inline int64_t icp_blocks_bound(int64_t total0, int32_t n_pairs) { return cdiv(total0, ICP_QB) + n_pairs; }

// scratch layout (bytes): sorted targets | partials | blk_off | done
static inline int64_t icp_off_partials(int64_t total1) { return 16 * total1; }
static inline int64_t icp_off_blk(int64_t total0, int64_t total1, int32_t n_pairs) {
  return icp_off_partials(total1) + 8 * ICP_SUMS * icp_blocks_bound(total0, n_pairs);
}
static inline int64_t icp_off_done(int64_t total0, int64_t total1, int32_t n_pairs) {
  return icp_off_blk(total0, total1, n_pairs) + 8 * ((int64_t)n_pairs + 2);
}

}  // namespace gcl

using namespace gcl;

extern "C" {

int64_t gcl_icp_scratch_bytes(int64_t total0, int64_t total1, int32_t n_pairs) {
  if (total0 < 0 || total0 > 0x7fffffffll || total1 < 0 || total1 > 0x7fffffffll || n_pairs < 1 ||
      n_pairs > GCL_FPFH_MAX_CLOUDS)
    return 0;
  return icp_off_done(total0, total1, n_pairs) + 4 * (int64_t)n_pairs;
}

static int icp_check_offsets(const char* name, const int64_t* off, int32_t n_pairs, int64_t* total) {
  GCL_CHECK_ARG(off, "gcl_icp_register_batch: null pointer (%s)", name);
  GCL_CHECK_ARG(off[0] == 0, "gcl_icp_register_batch: %s[0] = %lld, not 0", name, (long long)off[0]);
  for (int32_t b = 0; b < n_pairs; ++b)
    GCL_CHECK_ARG(off[b + 1] >= off[b], "gcl_icp_register_batch: %s descends at pair %d", name, b);
  GCL_CHECK_ARG(off[n_pairs] <= 0x7fffffffll, "gcl_icp_register_batch: %s ends at %lld rows, above 2^31 - 1", name,
                (long long)off[n_pairs]);
  *total = off[n_pairs];
  return GCL_OK;
}

int gcl_icp_register_batch(const float* xyz0, const int64_t* offsets0_host, const int64_t* offsets0, const float* xyz1,
                           const int64_t* offsets1_host, const int64_t* offsets1, int32_t n_pairs,
                           const int64_t* sorted_keys, const int64_t* order, double max_correspondence_distance,
                           const double* init, int32_t max_iteration, double relative_fitness, double relative_rmse,
                           void* scratch, double* T, double* stats, int32_t* status, int32_t* corr, void* stream) {
  GCL_CHECK_ARG(n_pairs >= 1 && n_pairs <= GCL_FPFH_MAX_CLOUDS, "gcl_icp_register_batch: n_pairs = %d not in 1 .. %d", n_pairs,
                GCL_FPFH_MAX_CLOUDS);
  const float radius = (float)max_correspondence_distance;
  GCL_CHECK_ARG(max_correspondence_distance > 0.0 && radius > 0.f && radius < 3.0e38f,
                "gcl_icp_register_batch: max_correspondence_distance must be positive and finite");
  GCL_CHECK_ARG(max_iteration >= 0 && max_iteration <= ICP_MAX_ITERATION,
                "gcl_icp_register_batch: max_iteration = %d not in 0 .. %d", max_iteration, ICP_MAX_ITERATION);
  GCL_CHECK_ARG(relative_fitness == relative_fitness && relative_rmse == relative_rmse,
                "gcl_icp_register_batch: a convergence threshold is not a number");
  int64_t total0 = 0, total1 = 0;
  if (int rc = icp_check_offsets("offsets0_host", offsets0_host, n_pairs, &total0)) return rc;
  if (int rc = icp_check_offsets("offsets1_host", offsets1_host, n_pairs, &total1)) return rc;
  GCL_CHECK_ARG(offsets0 && offsets1 && init && scratch && T && stats && status,
                "gcl_icp_register_batch: null pointer (offsets0, offsets1, init, scratch, T, stats or status)");
  GCL_CHECK_ARG((total0 == 0 || xyz0) && (total1 == 0 || (xyz1 && sorted_keys && order)),
                "gcl_icp_register_batch: null pointer (xyz0, xyz1, sorted_keys or order)");
  int64_t blocks = 0;
  for (int32_t b = 0; b < n_pairs; ++b) blocks += cdiv(offsets0_host[b + 1] - offsets0_host[b], ICP_QB);

  char* base = (char*)scratch;
  float4* sorted = (float4*)base;
  double* partials = (double*)(base + icp_off_partials(total1));
  long long* blk_off = (long long*)(base + icp_off_blk(total0, total1, n_pairs));
  int* done = (int*)(base + icp_off_done(total0, total1, n_pairs));
  const long long* off0 = (const long long*)offsets0;
  const long long* off1 = (const long long*)offsets1;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_setup = total1 > n_pairs ? total1 : n_pairs;
  hipLaunchKernelGGL(k_icp_setup, dim3((unsigned)cdiv(n_setup, 256)), dim3(256), 0, st, xyz1, (long long)total1, off0, off1,
                     n_pairs, (const long long*)sorted_keys, (const long long*)order, init, sorted, blk_off, done, T, stats,
                     status);
  GCL_CHECK_LAUNCH();
  const double inv_edge = fp_inv_edge(radius), r2 = max_correspondence_distance * max_correspondence_distance;
  for (int it = 0; it <= max_iteration; ++it) {
    if (blocks > 0) {
      const dim3 grid((unsigned)blocks), block(ICP_QB);
      hipLaunchKernelGGL(k_icp_step, grid, block, 0, st, xyz0, off0, off1, n_pairs, blk_off, sorted,
                         (const long long*)sorted_keys, T, done, inv_edge, r2, partials, corr);
      GCL_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_icp_update, dim3((unsigned)n_pairs), dim3(ICP_UPD_THREADS), 0, st, off0, blk_off, partials, it,
                       max_iteration, relative_fitness, relative_rmse, done, T, stats, status);
    GCL_CHECK_LAUNCH();
  }
  return GCL_OK;
}

}  // extern "C"
