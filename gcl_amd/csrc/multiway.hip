// Multiway registration (lib/complement_data_loader.py:407-516): the two pieces beside the pairwise ICP of icp.hip.
//
// 1. open3d's get_information_matrix_from_point_clouds for a ragged batch of pairs, restated from its published source
//    (DESIGN.md "Multiway registration"): sum G^T G over the correspondences of p = T x, a function of ten sums of the TARGET
//    points.
//      k_info_setup   the target points once in sorted-cell order (as k_icp_setup keeps them) and the pairs' first blocks
//      k_info_step    the correspondence of every source row (the search of k_icp_step, restated here so that icp.hip
//                     compiles to what it did) and its ten terms; 256 rows of one pair per block, a butterfly per wave, the
//                     waves added in wave order: one partial per block, no atomics
//      k_info_finish  one workgroup per pair: the partials added in block order, the 6 x 6 assembled
// 2. open3d's global_optimization with GlobalOptimizationLevenbergMarquardt for a batch of small graphs:
//      k_multiway_compose  one thread per graph: nodes, edges and flags of the reference's full_registration from the ICPs
//      k_posegraph         one workgroup per graph runs posegraph.h with its working set in LDS
//
// Nothing is read back and nothing is added atomically: a pair's matrix and a graph's result are bitwise the same alone,
// anywhere in a batch and on every run.
#include "common.h"
#include "fpgrid.h"
#include "posegraph.h"

#include <math.h>

namespace gcl {

constexpr int INFO_QB = 256;            // source rows per block = threads per block
constexpr int INFO_LPQ = 16;            // lanes per query: the ICP search's measured choice, not measured again at 0.075 m
constexpr int INFO_SUMS = 10;           // n, sum q (3), sum of xx xy xz yy yz zz

__global__ void __launch_bounds__(256) k_info_setup(const float* __restrict__ xyz1, long long total1,
                                                    const long long* __restrict__ off0, const long long* __restrict__ off1, int B,
                                                    const long long* __restrict__ skeys, const long long* __restrict__ order,
                                                    float4* __restrict__ sorted, long long* __restrict__ blk_off) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < total1) {
    const long long j = order[i];
    int b = (int)(skeys[i] >> 48);
    b = b < 0 ? 0 : (b >= B ? B - 1 : b);
    float4 v = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
    if (j >= 0 && j < total1) v = make_float4(xyz1[3 * j], xyz1[3 * j + 1], xyz1[3 * j + 2], __int_as_float((int)(j - off1[b])));
    sorted[i] = v;
  }
  if (i == 0) {
    long long acc = 0;
    blk_off[0] = 0;
    for (int b = 0; b < B; ++b) {
      const long long n0 = off0[b + 1] - off0[b];
      acc += n0 > 0 ? (n0 + INFO_QB - 1) / INFO_QB : 0;
      blk_off[b + 1] = acc;
    }
  }
}

// (d2, row) of a is below that of b
__device__ __forceinline__ bool mw_less(double da, int ra, double db, int rb) { return da < db || (da == db && ra < rb); }

__global__ void __launch_bounds__(INFO_QB) k_info_step(const float* __restrict__ xyz0, const long long* __restrict__ off0,
                                                       const long long* __restrict__ off1, int B,
                                                       const long long* __restrict__ blk_off, const float4* __restrict__ sorted,
                                                       const long long* __restrict__ skeys, const double* __restrict__ T,
                                                       double inv_edge, double r2, double* __restrict__ partials) {
  __shared__ int s_pos[INFO_QB];                      // the correspondence's position in the pair's sorted targets, -1: none
  __shared__ double s_wave[INFO_QB / 64][INFO_SUMS];
  const int b = fp_cloud_of(blk_off, B, (long long)blockIdx.x);
  const long long row0 = off0[b] + ((long long)blockIdx.x - blk_off[b]) * INFO_QB;
  const long long rows = off0[b + 1] - row0;
  const int nq = rows < INFO_QB ? (int)(rows < 0 ? 0 : rows) : INFO_QB;
  const long long t_lo = off1[b];
  const int n1 = (int)(off1[b + 1] - t_lo);
  const long long* __restrict__ keys = skeys + t_lo;
  const float4* __restrict__ tgt = sorted + t_lo;
  double M[12];
#pragma unroll
  for (int c = 0; c < 12; ++c) M[c] = T[16 * b + c];

  constexpr int LPQ = INFO_LPQ, GROUPS = INFO_QB / LPQ;
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
    const int total = pre9[9] < n1 ? pre9[9] : n1;    // the runs are disjoint: never more than n1 candidates
    for (int c0 = l; c0 < total; c0 += LPQ) {
      int s = lo9[0] + c0;
#pragma unroll
      for (int r = 1; r < 9; ++r)
        if (c0 >= pre9[r]) s = lo9[r] + (c0 - pre9[r]);
      if (s < 0 || s >= n1) continue;
      const float4 c = tgt[s];
      const double d = fp_d2(px, py, pz, c.x, c.y, c.z);
      const int row = __float_as_int(c.w);
      if (d <= r2 && mw_less(d, row, best, best_row)) { best = d; best_row = row; best_pos = s; }
    }
#pragma unroll
    for (int o = LPQ / 2; o > 0; o >>= 1) {
      const double od = __shfl_xor(best, o, LPQ);
      const int orow = __shfl_xor(best_row, o, LPQ), opos = __shfl_xor(best_pos, o, LPQ);
      if (opos >= 0 && mw_less(od, orow, best, best_row)) { best = od; best_row = orow; best_pos = opos; }
    }
    if (l == 0) s_pos[slot] = best_pos;
  }
  __syncthreads();

  // thread t: the ten terms of row t, all of the TARGET point (products of two floats: exact in fp64)
  double v[INFO_SUMS];
#pragma unroll
  for (int c = 0; c < INFO_SUMS; ++c) v[c] = 0.0;
  const int t = threadIdx.x;
  if (t < nq) {
    const int pos = s_pos[t];
    if (pos >= 0 && pos < n1) {
      const float4 c = tgt[pos];
      const double qx = c.x, qy = c.y, qz = c.z;
      v[0] = 1.0;
      v[1] = qx; v[2] = qy; v[3] = qz;
      v[4] = qx * qx; v[5] = qx * qy; v[6] = qx * qz;
      v[7] = qy * qy; v[8] = qy * qz; v[9] = qz * qz;
    }
  }
#pragma unroll
  for (int c = 0; c < INFO_SUMS; ++c) v[c] = wave_sum(v[c]);
  if ((t & 63) == 0)
#pragma unroll
    for (int c = 0; c < INFO_SUMS; ++c) s_wave[t >> 6][c] = v[c];
  __syncthreads();
  if (t < INFO_SUMS) {
    double s = s_wave[0][t];
    for (int w = 1; w < INFO_QB / 64; ++w) s += s_wave[w][t];
    partials[(long long)blockIdx.x * INFO_SUMS + t] = s;
  }
}

constexpr int INFO_FIN_THREADS = 256, INFO_FIN_CHUNK = 64;   // partials staged through LDS, 64 blocks at a time

__global__ void __launch_bounds__(INFO_FIN_THREADS) k_info_finish(const long long* __restrict__ blk_off,
                                                                  const double* __restrict__ partials,
                                                                  double* __restrict__ info) {
  __shared__ double s_part[INFO_FIN_CHUNK * INFO_SUMS];
  __shared__ double s_sum[INFO_SUMS];
  const int b = blockIdx.x, t = threadIdx.x;
  double s = 0.0;
  const long long k_hi = blk_off[b + 1];
  for (long long k0 = blk_off[b]; k0 < k_hi; k0 += INFO_FIN_CHUNK) {
    const int blocks = k_hi - k0 < INFO_FIN_CHUNK ? (int)(k_hi - k0) : INFO_FIN_CHUNK;
    for (int i = t; i < blocks * INFO_SUMS; i += INFO_FIN_THREADS) s_part[i] = partials[k0 * INFO_SUMS + i];
    __syncthreads();
    if (t < INFO_SUMS)
      for (int u = 0; u < blocks; ++u) s += s_part[u * INFO_SUMS + t];
    __syncthreads();
  }
  if (t < INFO_SUMS) s_sum[t] = s;
  __syncthreads();
  if (t >= 36) return;
  // G rows (0, z, -y, 1, 0, 0), (-z, 0, x, 0, 1, 0), (y, -x, 0, 0, 0, 1): the upper triangle, mirrored
  const double n = s_sum[0], x = s_sum[1], y = s_sum[2], z = s_sum[3];
  const double xx = s_sum[4], xy = s_sum[5], xz = s_sum[6], yy = s_sum[7], yz = s_sum[8], zz = s_sum[9];
  // 0.0 - v, not -v: a pair without correspondences gives the all-bits-zero matrix, no -0.0 in it
  const double U[36] = {zz + yy, 0.0 - xy, 0.0 - xz, 0.0,     0.0 - z, y,
                        0.0,     zz + xx,  0.0 - yz, z,       0.0,     0.0 - x,
                        0.0,     0.0,      yy + xx,  0.0 - y, x,       0.0,
                        0.0,     0.0,      0.0,      n,       0.0,     0.0,
                        0.0,     0.0,      0.0,      0.0,     n,       0.0,
                        0.0,     0.0,      0.0,      0.0,     0.0,     n};
  const int i = t / 6, j = t % 6;
  info[36 * (long long)b + t] = i <= j ? U[6 * i + j] : U[6 * j + i];
}

static inline int64_t info_blocks_bound(int64_t total0, int32_t n_pairs) { return cdiv(total0, INFO_QB) + n_pairs; }
// scratch layout (bytes): sorted targets | partials | blk_off
static inline int64_t info_off_partials(int64_t total1) { return 16 * total1; }
static inline int64_t info_off_blk(int64_t total0, int64_t total1, int32_t n_pairs) {
  return info_off_partials(total1) + 8 * INFO_SUMS * info_blocks_bound(total0, n_pairs);
}

// ---- the graphs of full_registration ------------------------------------------------------------------------------------
// Graph g has the nodes node_off[g] .. node_off[g + 1] - 1 and, as edges, every pair s < t of them in the order of the
// reference's double loop; T_icp holds the pairs' transformations in that order.
__global__ void __launch_bounds__(64) k_multiway_compose(const int* __restrict__ node_off, const int* __restrict__ edge_off,
                                                         int n_graphs, int total_nodes, int total_edges,
                                                         const double* __restrict__ T_icp, double* __restrict__ nodes,
                                                         int* __restrict__ edges, int* __restrict__ uncertain) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= n_graphs) return;
  const int n_lo = node_off[g], n = node_off[g + 1] - n_lo, e_lo = edge_off[g], m = edge_off[g + 1] - e_lo;
  if (n < 1 || n > PG_MAX_NODES || m != n * (n - 1) / 2 || n_lo < 0 || n_lo + n > total_nodes || e_lo < 0 ||
      e_lo + m > total_edges)
    return;                                            // k_posegraph reports the structure
  double odo[16], next[16];
  for (int c = 0; c < 16; ++c) odo[c] = (c % 5 == 0) ? 1.0 : 0.0;
  for (int c = 0; c < 16; ++c) nodes[16 * (long long)n_lo + c] = odo[c];
  int k = 0;
  for (int s = 0; s < n; ++s)
    for (int t = s + 1; t < n; ++t, ++k) {
      edges[2 * (e_lo + k)] = s;
      edges[2 * (e_lo + k) + 1] = t;
      uncertain[e_lo + k] = t != s + 1;
    }
  for (int t = 1; t < n; ++t) {
    const int s = t - 1, idx = s * n - s * (s + 1) / 2;             // the edge (t - 1, t)
    pg_mul(T_icp + 16 * (long long)(e_lo + idx), odo, next);
    for (int c = 0; c < 16; ++c) odo[c] = next[c];
    pg_rigid_inv(odo, nodes + 16 * (long long)(n_lo + t));
  }
}

struct PgBlock {
  __host__ __device__ int rank() const {
#if defined(__HIP_DEVICE_COMPILE__)
    return threadIdx.x;
#else
    return 0;
#endif
  }
  __host__ __device__ int size() const {
#if defined(__HIP_DEVICE_COMPILE__)
    return blockDim.x;
#else
    return 1;
#endif
  }
  __host__ __device__ void sync() const {
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
  }
};

constexpr int PG_THREADS = 256;
constexpr int PG_BAD_STRUCTURE = 4;

__global__ void __launch_bounds__(PG_THREADS) k_posegraph(const int* __restrict__ node_off, const int* __restrict__ edge_off,
                                                          int total_nodes, int total_edges, const double* __restrict__ nodes,
                                                          const int* __restrict__ edges, const double* __restrict__ edge_T,
                                                          const double* __restrict__ edge_info,
                                                          const int* __restrict__ uncertain, PgParams P,
                                                          double* __restrict__ poses, double* __restrict__ conf,
                                                          int* __restrict__ kept, double* __restrict__ stats,
                                                          int* __restrict__ status) {
  __shared__ PgWork W;
  __shared__ int s_src[PG_MAX_EDGES], s_dst[PG_MAX_EDGES], s_unc[PG_MAX_EDGES];
  __shared__ int s_bad;
  const int g = blockIdx.x, t = threadIdx.x;
  const int n_lo = node_off[g], n = node_off[g + 1] - n_lo, e_lo = edge_off[g], m = edge_off[g + 1] - e_lo;
  // the structure was validated by the caller; a graph that is not what it said is left alone (block-uniform)
  if (n < 1 || n > PG_MAX_NODES || m < 0 || m > PG_MAX_EDGES || n_lo < 0 || n_lo + n > total_nodes || e_lo < 0 ||
      e_lo + m > total_edges || P.reference_node < 0 || P.reference_node >= n) {
    if (t == 0) status[g] = PG_BAD_STRUCTURE;
    return;
  }
  if (t == 0) s_bad = 0;
  __syncthreads();
  if (t < m) {
    const int s = edges[2 * (e_lo + t)], d = edges[2 * (e_lo + t) + 1];
    s_src[t] = s;
    s_dst[t] = d;
    s_unc[t] = uncertain[e_lo + t] != 0;
    if (s < 0 || s >= n || d < 0 || d >= n || s == d) s_bad = 1;
  }
  __syncthreads();
  if (s_bad) {
    if (t == 0) status[g] = PG_BAD_STRUCTURE;
    return;
  }
  PgGraph G;
  G.n = n;
  G.m = m;
  G.src = s_src;
  G.dst = s_dst;
  G.uncertain = s_unc;
  G.nodes = nodes + 16 * (long long)n_lo;
  G.edge_T = edge_T + 16 * (long long)e_lo;
  G.edge_info = edge_info + 36 * (long long)e_lo;
  pg_global_optimization(PgBlock(), G, W, P, poses + 16 * (long long)n_lo, conf + e_lo, kept + e_lo, stats + PG_STATS * g,
                         status + g);
}

}  // namespace gcl

using namespace gcl;

extern "C" {

int64_t gcl_info_scratch_bytes(int64_t total0, int64_t total1, int32_t n_pairs) {
  if (total0 < 0 || total0 > 0x7fffffffll || total1 < 0 || total1 > 0x7fffffffll || n_pairs < 1 ||
      n_pairs > GCL_FPFH_MAX_CLOUDS)
    return 0;
  return info_off_blk(total0, total1, n_pairs) + 8 * ((int64_t)n_pairs + 2);
}

static int info_check_offsets(const char* name, const int64_t* off, int32_t n_pairs, int64_t* total) {
  GCL_CHECK_ARG(off, "gcl_info_matrix_batch: null pointer (%s)", name);
  GCL_CHECK_ARG(off[0] == 0, "gcl_info_matrix_batch: %s[0] = %lld, not 0", name, (long long)off[0]);
  for (int32_t b = 0; b < n_pairs; ++b)
    GCL_CHECK_ARG(off[b + 1] >= off[b], "gcl_info_matrix_batch: %s descends at pair %d", name, b);
  GCL_CHECK_ARG(off[n_pairs] <= 0x7fffffffll, "gcl_info_matrix_batch: %s ends at %lld rows, above 2^31 - 1", name,
                (long long)off[n_pairs]);
  *total = off[n_pairs];
  return GCL_OK;
}

int gcl_info_matrix_batch(const float* xyz0, const int64_t* offsets0_host, const int64_t* offsets0, const float* xyz1,
                          const int64_t* offsets1_host, const int64_t* offsets1, int32_t n_pairs, const int64_t* sorted_keys,
                          const int64_t* order, const double* transformation, double max_correspondence_distance,
                          void* scratch, double* info, void* stream) {
  GCL_CHECK_ARG(n_pairs >= 1 && n_pairs <= GCL_FPFH_MAX_CLOUDS, "gcl_info_matrix_batch: n_pairs = %d not in 1 .. %d", n_pairs,
                GCL_FPFH_MAX_CLOUDS);
  const float radius = (float)max_correspondence_distance;
  GCL_CHECK_ARG(max_correspondence_distance > 0.0 && radius > 0.f && radius < 3.0e38f,
                "gcl_info_matrix_batch: max_correspondence_distance must be positive and finite");
  int64_t total0 = 0, total1 = 0;
  if (int rc = info_check_offsets("offsets0_host", offsets0_host, n_pairs, &total0)) return rc;
  if (int rc = info_check_offsets("offsets1_host", offsets1_host, n_pairs, &total1)) return rc;
  GCL_CHECK_ARG(offsets0 && offsets1 && transformation && scratch && info,
                "gcl_info_matrix_batch: null pointer (offsets0, offsets1, transformation, scratch or info)");
  GCL_CHECK_ARG((total0 == 0 || xyz0) && (total1 == 0 || (xyz1 && sorted_keys && order)),
                "gcl_info_matrix_batch: null pointer (xyz0, xyz1, sorted_keys or order)");
  int64_t blocks = 0;
  for (int32_t b = 0; b < n_pairs; ++b) blocks += cdiv(offsets0_host[b + 1] - offsets0_host[b], INFO_QB);

  char* base = (char*)scratch;
  float4* sorted = (float4*)base;
  double* partials = (double*)(base + info_off_partials(total1));
  long long* blk_off = (long long*)(base + info_off_blk(total0, total1, n_pairs));
  const long long* off0 = (const long long*)offsets0;
  const long long* off1 = (const long long*)offsets1;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_setup = total1 > 1 ? total1 : 1;
  hipLaunchKernelGGL(k_info_setup, dim3((unsigned)cdiv(n_setup, 256)), dim3(256), 0, st, xyz1, (long long)total1, off0, off1,
                     n_pairs, (const long long*)sorted_keys, (const long long*)order, sorted, blk_off);
  GCL_CHECK_LAUNCH();
  if (blocks > 0) {
    const double inv_edge = fp_inv_edge(radius), r2 = max_correspondence_distance * max_correspondence_distance;
    hipLaunchKernelGGL(k_info_step, dim3((unsigned)blocks), dim3(INFO_QB), 0, st, xyz0, off0, off1, n_pairs, blk_off, sorted,
                       (const long long*)sorted_keys, transformation, inv_edge, r2, partials);
    GCL_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_info_finish, dim3((unsigned)n_pairs), dim3(INFO_FIN_THREADS), 0, st, blk_off, partials, info);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_multiway_compose(const int32_t* node_offsets, const int32_t* edge_offsets, int32_t n_graphs, int32_t total_nodes,
                         int32_t total_edges, const double* T_icp, double* nodes, int32_t* edges, int32_t* uncertain,
                         void* stream) {
  GCL_CHECK_ARG(n_graphs >= 1 && total_nodes >= 1 && total_edges >= 0,
                "gcl_multiway_compose: n_graphs = %d, total_nodes = %d, total_edges = %d", n_graphs, total_nodes, total_edges);
  GCL_CHECK_ARG(node_offsets && edge_offsets && nodes && (total_edges == 0 || (T_icp && edges && uncertain)),
                "gcl_multiway_compose: null pointer");
  hipLaunchKernelGGL(k_multiway_compose, dim3((unsigned)cdiv(n_graphs, 64)), dim3(64), 0, (hipStream_t)stream, node_offsets,
                     edge_offsets, n_graphs, total_nodes, total_edges, T_icp, nodes, edges, uncertain);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_posegraph_optimize_batch(const double* nodes, const int32_t* node_offsets, const int32_t* edges,
                                 const int32_t* edge_offsets, const double* edge_T, const double* edge_info,
                                 const int32_t* uncertain, int32_t n_graphs, int32_t total_nodes, int32_t total_edges,
                                 const double* params, double* poses, double* confidence, int32_t* kept, double* stats,
                                 int32_t* status, void* stream) {
  GCL_CHECK_ARG(n_graphs >= 1 && total_nodes >= 1 && total_edges >= 0,
                "gcl_posegraph_optimize_batch: n_graphs = %d, total_nodes = %d, total_edges = %d", n_graphs, total_nodes,
                total_edges);
  GCL_CHECK_ARG(nodes && node_offsets && edge_offsets && params && poses && stats && status,
                "gcl_posegraph_optimize_batch: null pointer (nodes, offsets, params, poses, stats or status)");
  GCL_CHECK_ARG(total_edges == 0 || (edges && edge_T && edge_info && uncertain && confidence && kept),
                "gcl_posegraph_optimize_batch: null pointer (edges, edge_T, edge_info, uncertain, confidence or kept)");
  for (int i = 0; i < PG_PARAMS; ++i)
    GCL_CHECK_ARG(params[i] == params[i], "gcl_posegraph_optimize_batch: params[%d] is not a number", i);
  const PgParams P = pg_params(params);
  GCL_CHECK_ARG(P.max_correspondence_distance > 0.0 && P.reference_node >= 0 && P.reference_node < PG_MAX_NODES &&
                    P.max_iteration >= 0 && P.max_iteration <= 1000 && P.max_iteration_lm >= 1 &&
                    P.max_iteration_lm <= 100,
                "gcl_posegraph_optimize_batch: a parameter is out of range");
  hipLaunchKernelGGL(k_posegraph, dim3((unsigned)n_graphs), dim3(PG_THREADS), 0, (hipStream_t)stream, node_offsets,
                     edge_offsets, total_nodes, total_edges, nodes, edges, edge_T, edge_info, uncertain, P, poses, confidence,
                     kept, stats, status);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

}  // extern "C"
