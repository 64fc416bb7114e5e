// FPFH descriptors (Rusu et al. 2009, as open3d computes them): radius neighbour lists, surface normals, SPFH and FPFH.
// The reference only LOADS these descriptors from files made with open3d (scripts/SC2_PCR/dataset.py:66-74, 220-228);
// here they are made on the device.  All arithmetic is fp64 from the fp32 inputs (DESIGN.md "FPFH").
//
//   gcl_fpfh_cell_keys   one thread per point: its cell of a uniform grid with edge ~radius as a 63-bit key
//                        (cloud, cx, cy, cz), z the lowest field.  The caller sorts the keys (any sort; ties in any order).
//   gcl_fpfh_neighbours  one wave per query point: the 27 cells around it are 9 runs of the sorted keys (the three z cells
//                        of one (x, y) column are adjacent), found by 18 binary searches; the runs are read as ONE stream of
//                        candidates, 64 per step, and merged into a sorted list of at most max_nn entries in LDS by rank
//                        (every entry counts the entries below it: keys (d2, row) are distinct, so ranks are a permutation).
//                        Exact for any number of candidates; nothing is truncated but by the (d2, row) order itself.
//   gcl_fpfh_normals     one thread per point: mean, covariance, cyclic Jacobi (fixed sweeps), orientation to the viewpoint.
//   gcl_fpfh_spfh        one wave per point: a lane per neighbour forms the pair features and its three bins; the 33 counts
//                        are INTEGERS (LDS atomics), so the row does not depend on the order of the lanes.
//   gcl_fpfh_combine     one wave per point, a lane per histogram entry: the 1 / d2 weighted sum of the neighbours' SPFH rows
//                        in list order, the per-feature normalisation to 100, plus the point's own SPFH row.
//
// Every loop over the lists or the grid is bounded by max_nn, by 64 halvings or by the number of points; a list entry is
// used only after it has been checked against [0, n), so a -1 (or any stale word) is never dereferenced.
#include "common.h"
#include "fpgrid.h"

#include <math.h>

// every product and sum below is rounded on its own, as the numpy restatement (tests/fpfh_oracle.py) rounds them
#pragma clang fp contract(off)

namespace gcl {

constexpr int FP_THREADS = 256, FP_WAVES = FP_THREADS / 64;
constexpr int FP_MAX_NN = 128;          // GCL_FPFH_MAX_NN
constexpr int FP_BINS = 33;
constexpr int FP_SWEEPS = 12;           // cyclic Jacobi on a symmetric 3 x 3 converges quadratically: 6 - 7 sweeps reach 1e-16

#define FP_WAVE_SYNC()                                      \
  do {                                                      \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  \
    __builtin_amdgcn_wave_barrier();                        \
  } while (0)

__global__ void __launch_bounds__(FP_THREADS) k_fpfh_cell_keys(const float* __restrict__ xyz, long long n,
                                                              const long long* __restrict__ off, int B, double inv_edge,
                                                              long long* __restrict__ keys) {
  const long long i = (long long)blockIdx.x * FP_THREADS + threadIdx.x;
  if (i >= n) return;
  const int b = fp_cloud_of(off, B, i);
  keys[i] = fp_key(b, fp_cell(xyz[3 * i], inv_edge), fp_cell(xyz[3 * i + 1], inv_edge), fp_cell(xyz[3 * i + 2], inv_edge));
}

__device__ __forceinline__ bool fp_less(double da, int ra, double db, int rb) { return da < db || (da == db && ra < rb); }

__global__ void __launch_bounds__(FP_THREADS) k_fpfh_neighbours(
    const float* __restrict__ xyz, long long n, const long long* __restrict__ off, int B,
    const long long* __restrict__ skeys, const long long* __restrict__ order, double inv_edge, double r2, int K,
    int* __restrict__ idx, int* __restrict__ cnt) {
  __shared__ double s_ld[FP_WAVES][FP_MAX_NN];      // the list, ascending (d2, row)
  __shared__ int s_lr[FP_WAVES][FP_MAX_NN];
  __shared__ double s_cd[FP_WAVES][64];             // the candidates of one step
  __shared__ int s_cr[FP_WAVES][64];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * FP_WAVES + w;
  if (i >= n) return;                                // wave-uniform; no block-wide barrier below
  double* ld = s_ld[w];
  int* lr = s_lr[w];
  double* cd = s_cd[w];
  int* cr = s_cr[w];
  const double qx = xyz[3 * i], qy = xyz[3 * i + 1], qz = xyz[3 * i + 2];
  const int b = fp_cloud_of(off, B, i);
  const long long row_lo = off[b], row_hi = off[b + 1];
  const int cx = fp_cell((float)qx, inv_edge), cy = fp_cell((float)qy, inv_edge), cz = fp_cell((float)qz, inv_edge);

  // lanes 0 .. 8: the run of sorted positions of column (cx + l % 3 - 1, cy + l / 3 - 1), z cells cz - 1 .. cz + 1
  long long run_lo = 0, run_len = 0;
  if (lane < 9) {
    const int x = cx + lane % 3 - 1, y = cy + lane / 3 - 1;
    if (x >= FP_CELL_MIN && x <= FP_CELL_MAX && y >= FP_CELL_MIN && y <= FP_CELL_MAX) {
      const int z0 = cz > FP_CELL_MIN ? cz - 1 : cz, z1 = cz < FP_CELL_MAX ? cz + 1 : cz;
      run_lo = fp_lower_bound(skeys, n, fp_key(b, x, y, z0));
      const long long run_hi = fp_lower_bound(skeys, n, fp_key(b, x, y, z1) + 1);
      run_len = run_hi > run_lo ? run_hi - run_lo : 0;
    }
  }
  long long lo9[9], pre9[10];
  pre9[0] = 0;
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    lo9[r] = __shfl(run_lo, r);
    pre9[r + 1] = pre9[r] + __shfl(run_len, r);
  }
  const long long total = pre9[9] < n ? pre9[9] : n;          // the runs are disjoint: never more than n candidates

  int L = 0;                                                   // entries in the list (wave-uniform)
  for (long long g0 = 0; g0 < total; g0 += 64) {
    // this lane's candidate
    const long long g = g0 + lane;
    double d2 = INFINITY;
    int row = 0x7fffffff;
    if (g < total) {
      long long s = lo9[0] + g;
#pragma unroll
      for (int r = 1; r < 9; ++r)
        if (g >= pre9[r]) s = lo9[r] + (g - pre9[r]);
      const long long j = (s >= 0 && s < n) ? order[s] : -1;
      if (j >= row_lo && j < row_hi) {                         // own cloud only, and a valid row of xyz
        const double d = fp_d2(qx, qy, qz, xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]);
        const bool in = d <= r2 && (L < K || fp_less(d, (int)j, ld[K - 1], lr[K - 1]));
        if (in) { d2 = d; row = (int)j; }
      }
    }
    const bool valid = row != 0x7fffffff;
    if (__ballot(valid) == 0ull) continue;                     // nothing enters the list at this step
    cd[lane] = d2;
    cr[lane] = row;
    // this lane's list entries, read before anything is moved
    const int t0 = lane, t1 = lane + 64;
    double e0d = 0, e1d = 0;
    int e0r = 0, e1r = 0;
    if (t0 < L) { e0d = ld[t0]; e0r = lr[t0]; }
    if (t1 < L) { e1d = ld[t1]; e1r = lr[t1]; }
    FP_WAVE_SYNC();
    // ranks in the union of the list and the valid candidates
    int rank0 = t0, rank1 = t1, rankc = 0;
    for (int c = 0; c < 64; ++c) {
      const double xd = cd[c];
      const int xr = cr[c];                                    // invalid: (inf, INT_MAX), below nothing
      rank0 += fp_less(xd, xr, e0d, e0r);
      rank1 += fp_less(xd, xr, e1d, e1r);
      rankc += fp_less(xd, xr, d2, row);
    }
    if (valid) {                                               // + list entries below the candidate (lower bound, <= 8 steps)
      int a = 0, z = L;
      for (int it = 0; it < 8 && a < z; ++it) {
        const int mid = (a + z) >> 1;
        if (fp_less(ld[mid], lr[mid], d2, row)) a = mid + 1; else z = mid;
      }
      rankc += a;
    }
    FP_WAVE_SYNC();                                            // every read of the old list is done
    if (t0 < L && rank0 < K) { ld[rank0] = e0d; lr[rank0] = e0r; }
    if (t1 < L && rank1 < K) { ld[rank1] = e1d; lr[rank1] = e1r; }
    if (valid && rankc < K) { ld[rankc] = d2; lr[rankc] = row; }
    L += __popcll(__ballot(valid));
    L = L < K ? L : K;
    FP_WAVE_SYNC();
  }
  for (int t = lane; t < K; t += 64) idx[i * K + t] = t < L ? lr[t] : -1;
  if (lane == 0) cnt[i] = L;
}

// ---- normals ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FP_THREADS) k_fpfh_normals(const float* __restrict__ xyz, long long n,
                                                            const int* __restrict__ idx, const int* __restrict__ cnt, int K,
                                                            const float* __restrict__ viewpoint,
                                                            const long long* __restrict__ off, int B,
                                                            float* __restrict__ normals) {
  const long long i = (long long)blockIdx.x * FP_THREADS + threadIdx.x;
  if (i >= n) return;
  const int* __restrict__ nb = idx + i * K;
  int k = cnt[i];
  k = k < 0 ? 0 : (k > K ? K : k);
  double m[3] = {0, 0, 0};
  int used = 0;
  for (int t = 0; t < k; ++t) {
    const long long j = nb[t];
    if (j < 0 || j >= n) continue;
    m[0] += (double)xyz[3 * j]; m[1] += (double)xyz[3 * j + 1]; m[2] += (double)xyz[3 * j + 2];
    ++used;
  }
  float* o = normals + 3 * i;
  if (used < 3) { o[0] = 0.f; o[1] = 0.f; o[2] = 1.f; return; }
  m[0] /= used; m[1] /= used; m[2] /= used;
  double A[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int t = 0; t < k; ++t) {
    const long long j = nb[t];
    if (j < 0 || j >= n) continue;
    const double a = (double)xyz[3 * j] - m[0], b = (double)xyz[3 * j + 1] - m[1], c = (double)xyz[3 * j + 2] - m[2];
    A[0][0] += a * a; A[0][1] += a * b; A[0][2] += a * c; A[1][1] += b * b; A[1][2] += b * c; A[2][2] += c * c;
  }
  A[0][0] /= used; A[0][1] /= used; A[0][2] /= used; A[1][1] /= used; A[1][2] /= used; A[2][2] /= used;
  A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[2][1] = A[1][2];
  // cyclic Jacobi: A <- J^T A J, V <- V J
  for (int sweep = 0; sweep < FP_SWEEPS; ++sweep)
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        const double apq = A[p][q];
        if (fabs(apq) <= 1e-300) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int r = 0; r < 3; ++r) {                          // columns p, q
          const double arp = A[r][p], arq = A[r][q];
          A[r][p] = c * arp - s * arq; A[r][q] = s * arp + c * arq;
          const double vrp = V[r][p], vrq = V[r][q];
          V[r][p] = c * vrp - s * vrq; V[r][q] = s * vrp + c * vrq;
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {                          // rows p, q
          const double apr = A[p][r], aqr = A[q][r];
          A[p][r] = c * apr - s * aqr; A[q][r] = s * apr + c * aqr;
        }
      }
  double ev = A[0][0], nx = V[0][0], ny = V[1][0], nz = V[2][0];           // smallest eigenvalue, ties: the first
  if (A[1][1] < ev) { ev = A[1][1]; nx = V[0][1]; ny = V[1][1]; nz = V[2][1]; }
  if (A[2][2] < ev) { ev = A[2][2]; nx = V[0][2]; ny = V[1][2]; nz = V[2][2]; }
  const double len = sqrt(nx * nx + ny * ny + nz * nz);
  nx /= len; ny /= len; nz /= len;
  double vx = 0, vy = 0, vz = 0;
  if (viewpoint) {
    const int b = fp_cloud_of(off, B, i);
    vx = viewpoint[3 * b]; vy = viewpoint[3 * b + 1]; vz = viewpoint[3 * b + 2];
  }
  const double dot = nx * (vx - (double)xyz[3 * i]) + ny * (vy - (double)xyz[3 * i + 1]) + nz * (vz - (double)xyz[3 * i + 2]);
  if (dot < 0) { nx = -nx; ny = -ny; nz = -nz; }
  o[0] = (float)nx; o[1] = (float)ny; o[2] = (float)nz;
}

// ---- SPFH -------------------------------------------------------------------------------------------------
__device__ __forceinline__ int fp_bin(double v) {
  const int h = (int)floor(v);
  return h < 0 ? 0 : (h > 10 ? 10 : h);
}

// open3d ComputePairFeatures (Feature.cpp), the three angular features of the pair (p1, n1), (p2, n2)
__device__ __forceinline__ void fp_pair(const double p1[3], const double n1[3], const double p2[3], const double n2[3],
                                        double f[3]) {
  f[0] = f[1] = f[2] = 0.0;
  double dp[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
  const double d = sqrt((dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2]);
  if (d == 0.0) return;
  const double a1 = ((n1[0] * dp[0] + n1[1] * dp[1]) + n1[2] * dp[2]) / d;
  const double a2 = ((n2[0] * dp[0] + n2[1] * dp[1]) + n2[2] * dp[2]) / d;
  double u[3], o[3], f3;
  if (fabs(a1) < fabs(a2)) {
    for (int c = 0; c < 3; ++c) { u[c] = n2[c]; o[c] = n1[c]; dp[c] = -dp[c]; }
    f3 = -a2;
  } else {
    for (int c = 0; c < 3; ++c) { u[c] = n1[c]; o[c] = n2[c]; }
    f3 = a1;
  }
  double v[3] = {dp[1] * u[2] - dp[2] * u[1], dp[2] * u[0] - dp[0] * u[2], dp[0] * u[1] - dp[1] * u[0]};
  const double vn = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  if (vn == 0.0) return;
  v[0] /= vn; v[1] /= vn; v[2] /= vn;
  const double wv[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
  f[1] = (v[0] * o[0] + v[1] * o[1]) + v[2] * o[2];
  f[0] = atan2((wv[0] * o[0] + wv[1] * o[1]) + wv[2] * o[2], (u[0] * o[0] + u[1] * o[1]) + u[2] * o[2]);
  f[2] = f3;
}

__global__ void __launch_bounds__(FP_THREADS) k_fpfh_spfh(const float* __restrict__ xyz, const float* __restrict__ normals,
                                                         long long n, const int* __restrict__ idx,
                                                         const int* __restrict__ cnt, int K, float* __restrict__ spfh) {
  __shared__ int s_hist[FP_WAVES][FP_BINS];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * FP_WAVES + w;
  if (i >= n) return;                                // wave-uniform
  int* hist = s_hist[w];
  if (lane < FP_BINS) hist[lane] = 0;
  FP_WAVE_SYNC();
  int k = cnt[i];
  k = k < 0 ? 0 : (k > K ? K : k);
  const double p1[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  const double n1[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
  const double PI = 3.14159265358979323846;
  for (int t = 1 + lane; t < k; t += 64) {           // entry 0 is the point itself
    const long long j = idx[i * K + t];
    if (j < 0 || j >= n) continue;
    const double p2[3] = {xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]};
    const double n2[3] = {normals[3 * j], normals[3 * j + 1], normals[3 * j + 2]};
    double f[3];
    fp_pair(p1, n1, p2, n2, f);
    atomicAdd(&hist[fp_bin(11.0 * (f[0] + PI) / (2.0 * PI))], 1);
    atomicAdd(&hist[11 + fp_bin(11.0 * (f[1] + 1.0) / 2.0)], 1);
    atomicAdd(&hist[22 + fp_bin(11.0 * (f[2] + 1.0) / 2.0)], 1);
  }
  FP_WAVE_SYNC();
  if (lane < FP_BINS) {
    const double inc = k > 1 ? 100.0 / (double)(k - 1) : 0.0;
    spfh[i * FP_BINS + lane] = (float)((double)hist[lane] * inc);
  }
}

// ---- FPFH -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FP_THREADS) k_fpfh_combine(const float* __restrict__ xyz, const float* __restrict__ spfh,
                                                            long long n, const int* __restrict__ idx,
                                                            const int* __restrict__ cnt, int K, int normalize,
                                                            float* __restrict__ out) {
  __shared__ double s_w[FP_WAVES][FP_MAX_NN];        // d2 of list entry t, 0: skip it
  __shared__ int s_j[FP_WAVES][FP_MAX_NN];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * FP_WAVES + w;
  if (i >= n) return;                                // wave-uniform
  int k = cnt[i];
  k = k < 0 ? 0 : (k > K ? K : k);
  const double qx = xyz[3 * i], qy = xyz[3 * i + 1], qz = xyz[3 * i + 2];
  for (int t = lane; t < k; t += 64) {
    const long long j = idx[i * K + t];
    double d2 = 0.0;
    if (t >= 1 && j >= 0 && j < n) d2 = fp_d2(qx, qy, qz, xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]);
    s_w[w][t] = d2;
    s_j[w][t] = d2 != 0.0 ? (int)j : 0;
  }
  FP_WAVE_SYNC();
  const int c = lane < FP_BINS ? lane : 0;           // lanes 33 .. 63 shadow entry 0 and write nothing
  double F = 0.0;
  for (int t = 1; t < k; ++t) {
    const double d2 = s_w[w][t];
    if (d2 == 0.0) continue;                         // a duplicate of the point (or an entry that is no row)
    F += (double)spfh[(long long)s_j[w][t] * FP_BINS + c] / d2;
  }
  // s[feature] = the sum of its 11 entries, in entry order
  const int base = 11 * (c / 11);
  double s = 0.0;
  for (int u = 0; u < 11; ++u) s += __shfl(F, base + u);
  double v = 0.0;
  if (k > 1) v = F * (s != 0.0 ? 100.0 / s : 0.0) + (double)spfh[i * FP_BINS + c];
  float r = (float)v;
  if (normalize) {                                   // f / (|f|_2 + 1e-6), dataset.py:73-74
    double sq = 0.0;
    for (int u = 0; u < FP_BINS; ++u) { const double x = (double)__shfl(r, u); sq += x * x; }
    r = (float)((double)r / (sqrt(sq) + 1e-6));
  }
  if (lane < FP_BINS) out[i * FP_BINS + lane] = r;
}

}  // namespace gcl

using namespace gcl;

extern "C" {

static int fp_check_clouds(const char* who, int64_t n, const int64_t* offsets, int32_t n_clouds) {
  GCL_CHECK_ARG(n >= 0 && n <= 0x7fffffffll, "%s: n = %lld out of range", who, (long long)n);
  GCL_CHECK_ARG(n_clouds >= 1 && n_clouds <= GCL_FPFH_MAX_CLOUDS, "%s: n_clouds = %d not in 1 .. %d", who, n_clouds,
                GCL_FPFH_MAX_CLOUDS);
  GCL_CHECK_ARG(offsets, "%s: null pointer (offsets)", who);
  return GCL_OK;
}

int gcl_fpfh_cell_keys(const float* xyz, int64_t n, const int64_t* offsets, int32_t n_clouds, float radius, int64_t* keys,
                       void* stream) {
  if (int rc = fp_check_clouds("gcl_fpfh_cell_keys", n, offsets, n_clouds)) return rc;
  GCL_CHECK_ARG(radius > 0.f && radius < 3.0e38f, "gcl_fpfh_cell_keys: radius must be positive and finite");
  if (n == 0) return GCL_OK;
  GCL_CHECK_ARG(xyz && keys, "gcl_fpfh_cell_keys: null pointer (xyz or keys)");
  hipLaunchKernelGGL(k_fpfh_cell_keys, dim3((unsigned)cdiv(n, FP_THREADS)), dim3(FP_THREADS), 0, (hipStream_t)stream, xyz,
                     (long long)n, (const long long*)offsets, n_clouds, fp_inv_edge(radius), (long long*)keys);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_fpfh_neighbours(const float* xyz, int64_t n, const int64_t* offsets, int32_t n_clouds, const int64_t* sorted_keys,
                        const int64_t* order, float radius, int32_t max_nn, int32_t* idx, int32_t* cnt, void* stream) {
  if (int rc = fp_check_clouds("gcl_fpfh_neighbours", n, offsets, n_clouds)) return rc;
  GCL_CHECK_ARG(radius > 0.f && radius < 3.0e38f, "gcl_fpfh_neighbours: radius must be positive and finite");
  GCL_CHECK_ARG(max_nn >= 1 && max_nn <= FP_MAX_NN, "gcl_fpfh_neighbours: max_nn = %d not in 1 .. %d", max_nn, FP_MAX_NN);
  if (n == 0) return GCL_OK;
  GCL_CHECK_ARG(xyz && sorted_keys && order && idx && cnt,
                "gcl_fpfh_neighbours: null pointer (xyz, sorted_keys, order, idx or cnt)");
  const double r = (double)radius;
  hipLaunchKernelGGL(k_fpfh_neighbours, dim3((unsigned)cdiv(n, FP_WAVES)), dim3(FP_THREADS), 0, (hipStream_t)stream, xyz,
                     (long long)n, (const long long*)offsets, n_clouds, (const long long*)sorted_keys,
                     (const long long*)order, fp_inv_edge(radius), r * r, max_nn, idx, cnt);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_fpfh_normals(const float* xyz, int64_t n, const int32_t* idx, const int32_t* cnt, int32_t max_nn,
                     const float* viewpoint, const int64_t* offsets, int32_t n_clouds, float* normals, void* stream) {
  if (int rc = fp_check_clouds("gcl_fpfh_normals", n, offsets, n_clouds)) return rc;
  GCL_CHECK_ARG(max_nn >= 1 && max_nn <= FP_MAX_NN, "gcl_fpfh_normals: max_nn = %d not in 1 .. %d", max_nn, FP_MAX_NN);
  if (n == 0) return GCL_OK;
  GCL_CHECK_ARG(xyz && idx && cnt && normals, "gcl_fpfh_normals: null pointer (xyz, idx, cnt or normals)");
  hipLaunchKernelGGL(k_fpfh_normals, dim3((unsigned)cdiv(n, FP_THREADS)), dim3(FP_THREADS), 0, (hipStream_t)stream, xyz,
                     (long long)n, idx, cnt, max_nn, viewpoint, (const long long*)offsets, n_clouds, normals);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_fpfh_spfh(const float* xyz, const float* normals, int64_t n, const int32_t* idx, const int32_t* cnt, int32_t max_nn,
                  float* spfh, void* stream) {
  GCL_CHECK_ARG(n >= 0 && n <= 0x7fffffffll, "gcl_fpfh_spfh: n = %lld out of range", (long long)n);
  GCL_CHECK_ARG(max_nn >= 1 && max_nn <= FP_MAX_NN, "gcl_fpfh_spfh: max_nn = %d not in 1 .. %d", max_nn, FP_MAX_NN);
  if (n == 0) return GCL_OK;
  GCL_CHECK_ARG(xyz && normals && idx && cnt && spfh, "gcl_fpfh_spfh: null pointer (xyz, normals, idx, cnt or spfh)");
  hipLaunchKernelGGL(k_fpfh_spfh, dim3((unsigned)cdiv(n, FP_WAVES)), dim3(FP_THREADS), 0, (hipStream_t)stream, xyz, normals,
                     (long long)n, idx, cnt, max_nn, spfh);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_fpfh_combine(const float* xyz, const float* spfh, int64_t n, const int32_t* idx, const int32_t* cnt, int32_t max_nn,
                     int32_t normalize, float* fpfh, void* stream) {
  GCL_CHECK_ARG(n >= 0 && n <= 0x7fffffffll, "gcl_fpfh_combine: n = %lld out of range", (long long)n);
  GCL_CHECK_ARG(max_nn >= 1 && max_nn <= FP_MAX_NN, "gcl_fpfh_combine: max_nn = %d not in 1 .. %d", max_nn, FP_MAX_NN);
  if (n == 0) return GCL_OK;
  GCL_CHECK_ARG(xyz && spfh && idx && cnt && fpfh, "gcl_fpfh_combine: null pointer (xyz, spfh, idx, cnt or fpfh)");
  GCL_CHECK_ARG(spfh != fpfh, "gcl_fpfh_combine: fpfh must not alias spfh (a row reads its neighbours' SPFH rows)");
  hipLaunchKernelGGL(k_fpfh_combine, dim3((unsigned)cdiv(n, FP_WAVES)), dim3(FP_THREADS), 0, (hipStream_t)stream, xyz, spfh,
                     (long long)n, idx, cnt, max_nn, normalize != 0, fpfh);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

}  // extern "C"
