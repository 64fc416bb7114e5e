// Feature-match recall (generalization_ETH/evaluate.py): 3-D nearest point with a fused row gather, and the mutual filter
// with the inlier count under a known transformation.
//
// Reference: generalization_ETH/evaluate.py:110-122 (find_nearest_voxel_feature: pytorch3d knn_points, K = 1, ~5000
// keypoints against the 10^5 - 10^6 voxel points of a fragment), :63-77 (calculate_M: two sklearn KDTrees and a Python
// loop on the CPU), :160-169 (inlier count under gtTrans, numpy on the host).
//
// ---- k_nn3_rowmin -----------------------------------------------------------------------------------------------------
// Exact brute force.  A thread owns NN3_QPT queries in registers; the points are read with WAVE-UNIFORM addresses (the
// compiler turns them into scalar loads: no LDS, no barrier in the loop), four points per step, so that one step's twelve
// floats serve 64 x NN3_QPT x 4 pairs.  The distance is the DIFFERENCE form, (qx - px)^2 + (qy - py)^2 + (qz - pz)^2 as
//   d2 = fma(dz, dz, fma(dy, dy, dx * dx)),
// never |q|^2 + |p|^2 - 2 q.p: at |x| ~ 800 m the terms of the expansion are ~10^6 with an fp32 ulp of 0.06 - 0.12 m^2,
// and the neighbouring voxel of a 5 cm grid is 2.5e-3 m^2 away; the difference form is good to a few 2^-24 relative.
// Plain fp32 operations, not the packed pair forms: a pair is three subtractions, a product, two FMAs, a comparison and two
// selects, of which only the first six could be packed, and a packed operation needs its operands in adjacent registers --
// the query or point pairs would have to be duplicated (the (a_c, a_c) layout of k_nn_rowmin) for six of nine
// instructions.  The compiler is free to pair them where it sees a gain.
// Grid = (NN3_TQ-query tiles) x (chunks of p): m ~ 5000 alone gives 20 tiles, the chunks put ~2000 workgroups on the 256
// CUs.  The four waves of a workgroup take every fourth group of four points of the chunk, ascending within a thread
// (strict <: the lowest index stays), the waves are folded through LDS (value, then index), and the chunks by k_nn3_merge
// in ascending chunk order (strict <), as k_nn_rowmin / k_nn_merge do.  Whichever kernel writes the final arg-minimum of
// a tile also copies the tile's feature rows (desc[i] = feat[argmin[i]]): the indices are in LDS at that point.
#include "common.h"

#include <math.h>

namespace gcl {

constexpr int NN3_QPT = 4;               // queries per thread
constexpr int NN3_TQ = 64 * NN3_QPT;     // queries per workgroup: query k of lane l is row tile * NN3_TQ + k * 64 + l
constexpr int NN3_STEP = 4;              // points per step of a wave
constexpr int NN3_GRAN = 4 * NN3_STEP;   // points per step of a workgroup: chunks are multiples of this
constexpr int NN3_MIN_CHUNK = 256;       // fewer points than this per workgroup do not pay for its launch and merge
constexpr int NN3_WG_TARGET = 2048;      // workgroups wanted on the chip (8 per CU)

// desc rows of a tile from its final arg-minima (in LDS): consecutive threads copy consecutive channels of a row
__device__ __forceinline__ void nn3_gather_tile(const int* idx, int q0, int nq, const float* __restrict__ feat, int c,
                                                float* __restrict__ desc) {
  const long long total = (long long)nq * c;
  for (long long e = threadIdx.x; e < total; e += 256) {
    const int q = (int)(e / c), ch = (int)(e - (long long)q * c);
    desc[(long long)(q0 + q) * c + ch] = feat[(long long)idx[q] * c + ch];
  }
}

__global__ void __launch_bounds__(256) k_nn3_rowmin(const float* __restrict__ q, int m, const float* __restrict__ p, int n,
                                                    int chunk, float* __restrict__ out_v, int* __restrict__ out_i,
                                                    float* __restrict__ d2min, const float* __restrict__ feat, int c,
                                                    float* __restrict__ desc) {
  __shared__ float rv[4][NN3_TQ];
  __shared__ int ri[4][NN3_TQ];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q0 = blockIdx.x * NN3_TQ;
  const int jb = blockIdx.y * chunk;
  const int je = (jb + chunk < n) ? jb + chunk : n;
  float qx[NN3_QPT], qy[NN3_QPT], qz[NN3_QPT], best[NN3_QPT];
  int besti[NN3_QPT];
#pragma unroll
  for (int k = 0; k < NN3_QPT; ++k) {
    const int row = q0 + k * 64 + lane;
    const bool ok = row < m;
    qx[k] = ok ? q[3 * (long long)row] : 0.f;
    qy[k] = ok ? q[3 * (long long)row + 1] : 0.f;
    qz[k] = ok ? q[3 * (long long)row + 2] : 0.f;
    best[k] = INFINITY;
    besti[k] = jb;          // a row of NaN / overflowing distances keeps an index inside the chunk
  }
  // whole groups of four points, then the chunk's last, partial group (only the last chunk has one)
  const int full_end = jb + (je - jb) / NN3_STEP * NN3_STEP;
  for (int j = jb + w * NN3_STEP; j < full_end; j += NN3_GRAN) {
    const float* __restrict__ pj = p + 3 * (long long)j;
    float pv[3 * NN3_STEP];
#pragma unroll
    for (int e = 0; e < 3 * NN3_STEP; ++e) pv[e] = pj[e];
#pragma unroll
    for (int s = 0; s < NN3_STEP; ++s) {
#pragma unroll
      for (int k = 0; k < NN3_QPT; ++k) {
        const float dx = qx[k] - pv[3 * s], dy = qy[k] - pv[3 * s + 1], dz = qz[k] - pv[3 * s + 2];
        const float d2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
        if (d2 < best[k]) {
          best[k] = d2;
          besti[k] = j + s;
        }
      }
    }
  }
  if (full_end < je && ((full_end - jb) / NN3_STEP) % 4 == w) {
    for (int j = full_end; j < je; ++j) {
      const float px = p[3 * (long long)j], py = p[3 * (long long)j + 1], pz = p[3 * (long long)j + 2];
#pragma unroll
      for (int k = 0; k < NN3_QPT; ++k) {
        const float dx = qx[k] - px, dy = qy[k] - py, dz = qz[k] - pz;
        const float d2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
        if (d2 < best[k]) {
          best[k] = d2;
          besti[k] = j;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NN3_QPT; ++k) {
    rv[w][k * 64 + lane] = best[k];
    ri[w][k * 64 + lane] = besti[k];
  }
  __syncthreads();
  const int t = threadIdx.x, row = q0 + t;
  float bv = rv[0][t];
  int bi = ri[0][t];
#pragma unroll
  for (int u = 1; u < 4; ++u) {
    const float v = rv[u][t];
    const int i2 = ri[u][t];
    if (v < bv || (v == bv && i2 < bi)) {
      bv = v;
      bi = i2;
    }
  }
  if (gridDim.y > 1) {
    if (row < m) {
      out_v[(long long)blockIdx.y * m + row] = bv;
      out_i[(long long)blockIdx.y * m + row] = bi;
    }
    return;
  }
  if (row < m) {
    if (d2min) d2min[row] = bv;
    out_i[row] = bi;
  }
  if (desc) {
    __syncthreads();        // every thread has read the four waves' entries of ri
    ri[0][t] = bi;
    __syncthreads();
    nn3_gather_tile(ri[0], q0, (m - q0 < NN3_TQ) ? m - q0 : NN3_TQ, feat, c, desc);
  }
}

__global__ void __launch_bounds__(256) k_nn3_merge(const float* __restrict__ part_v, const int* __restrict__ part_i, int m,
                                                   int n_chunks, float* __restrict__ d2min, int* __restrict__ argmin,
                                                   const float* __restrict__ feat, int c, float* __restrict__ desc) {
  __shared__ int idx[256];
  const int q0 = blockIdx.x * 256, r = q0 + threadIdx.x;
  int bi = 0;
  if (r < m) {
    float bv = part_v[r];
    bi = part_i[r];
    for (int k = 1; k < n_chunks; ++k) {      // chunks hold ascending index ranges: strict < keeps the lowest index
      const float v = part_v[(long long)k * m + r];
      if (v < bv) {
        bv = v;
        bi = part_i[(long long)k * m + r];
      }
    }
    if (d2min) d2min[r] = bv;
    argmin[r] = bi;
  }
  if (desc) {
    idx[threadIdx.x] = bi;
    __syncthreads();
    nn3_gather_tile(idx, q0, (m - q0 < 256) ? m - q0 : 256, feat, c, desc);
  }
}

// points per chunk: as many chunks as it takes to put ~NN3_WG_TARGET workgroups on the chip, a multiple of NN3_GRAN
// points each and NN3_MIN_CHUNK at the least
static int nn3_chunk_rows(int m, int n) {
  const long long tiles = cdiv(m, NN3_TQ);
  long long want = cdiv(NN3_WG_TARGET, tiles);
  const long long grans = cdiv(n, NN3_GRAN);
  if (want > grans) want = grans;
  if (want < 1) want = 1;
  long long chunk = cdiv(grans, want) * NN3_GRAN;
  if (chunk < NN3_MIN_CHUNK) chunk = NN3_MIN_CHUNK;
  return (int)chunk;
}

// ---- k_mutual_match -----------------------------------------------------------------------------------------------------
// ONE workgroup walks the sources in tiles of 1024, ascending: a source i is kept iff nn10[nn01[i]] == i; its place in
// `pairs` is the number of kept sources before it (wave ballot + the waves' counts in LDS + the running base), so the list
// is dense, ascending in i and the same from run to run -- no atomic decides an order.  m0 ~ 5000 is five tiles; the work
// is two dependent 4-byte reads per source, far too little to spread over the chip, and a scene enqueues one such launch
// per pair of fragments behind two 1-NN searches that do fill it.  The inlier count (integers: any order gives the same
// sum) is folded the same way.  Residuals are fp32: |kp0[i] - (R kp1[j] + t)| with the product as an FMA chain per row.
// (The body is a device function: k_mutual_match runs it in its one workgroup, k_mutual_match_batch in one workgroup per pair.)
__device__ __forceinline__ void mutual_match_body(const int* __restrict__ nn01, int m0, const int* __restrict__ nn10, int m1,
                                                  const float* __restrict__ kp0, const float* __restrict__ kp1,
                                                  const float* __restrict__ T, float tau, int* __restrict__ pairs,
                                                  int* __restrict__ stats) {
  __shared__ int wcount[16], winl[16];
  __shared__ int base_s, inl_s;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  float Tm[12];
  if (T) {
#pragma unroll
    for (int e = 0; e < 12; ++e)      // the same twelve values in every lane: kept in scalar registers
      Tm[e] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(T[e])));
  }
  if (t == 0) {
    base_s = 0;
    inl_s = 0;
  }
  __syncthreads();
  for (int i0 = 0; i0 < m0; i0 += 1024) {
    const int i = i0 + t;
    int j = -1;
    bool keep = false;
    if (i < m0) {
      j = nn01[i];
      if ((unsigned)j < (unsigned)m1) keep = nn10[j] == i;      // an index outside [0, m1) is never dereferenced
    }
    bool inl = false;
    if (keep && T) {
      const float x = kp1[3 * (long long)j], y = kp1[3 * (long long)j + 1], z = kp1[3 * (long long)j + 2];
      const float dx = kp0[3 * (long long)i] - __builtin_fmaf(Tm[2], z, __builtin_fmaf(Tm[1], y, __builtin_fmaf(Tm[0], x, Tm[3])));
      const float dy = kp0[3 * (long long)i + 1] - __builtin_fmaf(Tm[6], z, __builtin_fmaf(Tm[5], y, __builtin_fmaf(Tm[4], x, Tm[7])));
      const float dz = kp0[3 * (long long)i + 2] - __builtin_fmaf(Tm[10], z, __builtin_fmaf(Tm[9], y, __builtin_fmaf(Tm[8], x, Tm[11])));
      inl = sqrtf(__builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx))) < tau;
    }
    const unsigned long long mk = __ballot(keep), mi = __ballot(inl);
    if (lane == 0) {
      wcount[w] = __popcll(mk);
      winl[w] = __popcll(mi);
    }
    __syncthreads();
    int before = base_s, tile_total = 0, tile_inl = 0;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      if (u < w) before += wcount[u];
      tile_total += wcount[u];
      tile_inl += winl[u];
    }
    if (keep) {
      const int at = before + __popcll(mk & ((1ull << lane) - 1ull));
      pairs[2 * (long long)at] = i;
      pairs[2 * (long long)at + 1] = j;
    }
    __syncthreads();        // everyone has read base_s and the waves' counts
    if (t == 0) {
      base_s += tile_total;
      inl_s += tile_inl;
    }
    __syncthreads();
  }
  if (t == 0) {
    stats[0] = base_s;
    stats[1] = inl_s;
  }
}

__global__ void __launch_bounds__(1024) k_mutual_match(const int* __restrict__ nn01, int m0, const int* __restrict__ nn10,
                                                       int m1, const float* __restrict__ kp0, const float* __restrict__ kp1,
                                                       const float* __restrict__ T, float tau, int* __restrict__ pairs,
                                                       int* __restrict__ stats) {
  mutual_match_body(nn01, m0, nn10, m1, kp0, kp1, T, tau, pairs, stats);
}

// one workgroup per pair of the table: eight pairs fill eight CUs at once instead of one CU eight times in a row
__global__ void __launch_bounds__(1024) k_mutual_match_batch(const gcl_mutual_job* __restrict__ jobs, float tau) {
  const gcl_mutual_job* __restrict__ j = jobs + blockIdx.x;
  mutual_match_body(j->nn01, j->m0, j->nn10, j->m1, j->xyz0, j->xyz1, j->T, tau, j->pairs, j->count);
}

// ---- k_mutual_corr ------------------------------------------------------------------------------------------------------
// The correspondences a registration with open3d's mutual filter runs on, as point rows, with their number left on the
// device.  ONE workgroup, as k_mutual_match and for its reasons, in two walks over the sources: the first counts the mutual
// pairs, the second writes -- the compacted rows (same ballot / LDS placement: dense, ascending in i, no atomic) followed by
// zero rows when there are at least min_count of them, else every source beside its nearest target (open3d: "too few
// correspondences after mutual filter, fall back to original correspondences").  Which branch runs is uniform over the
// workgroup.  A target index outside [0, m1) is never dereferenced: such a row of the fall-back has a zero target.
__device__ __forceinline__ void mutual_corr_body(const int* __restrict__ nn01, int m0, const int* __restrict__ nn10, int m1,
                                                 const float* __restrict__ xyz0, const float* __restrict__ xyz1,
                                                 int min_count, float* __restrict__ src, float* __restrict__ tgt,
                                                 int* __restrict__ count) {
  __shared__ int wcount[16];
  __shared__ int base_s;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  int mine = 0;
  for (int i = t; i < m0; i += 1024) {
    const int j = nn01[i];
    if ((unsigned)j < (unsigned)m1 && nn10[j] == i) ++mine;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
  if (lane == 0) wcount[w] = mine;
  __syncthreads();
  int n_mutual = 0;
#pragma unroll
  for (int u = 0; u < 16; ++u) n_mutual += wcount[u];
  __syncthreads();        // the waves' counts are reused below
  if (n_mutual < min_count) {
    for (int i = t; i < m0; i += 1024) {
      const int j = nn01[i];
      const bool ok = (unsigned)j < (unsigned)m1;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        src[3 * (long long)i + c] = xyz0[3 * (long long)i + c];
        tgt[3 * (long long)i + c] = ok ? xyz1[3 * (long long)j + c] : 0.f;
      }
    }
    if (t == 0) {
      count[0] = m0;
      count[1] = n_mutual;
    }
    return;
  }
  if (t == 0) base_s = 0;
  __syncthreads();
  for (int i0 = 0; i0 < m0; i0 += 1024) {
    const int i = i0 + t;
    int j = -1;
    bool keep = false;
    if (i < m0) {
      j = nn01[i];
      if ((unsigned)j < (unsigned)m1) keep = nn10[j] == i;
    }
    const unsigned long long mk = __ballot(keep);
    if (lane == 0) wcount[w] = __popcll(mk);
    __syncthreads();
    int before = base_s, tile_total = 0;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      if (u < w) before += wcount[u];
      tile_total += wcount[u];
    }
    if (keep) {
      const long long at = before + __popcll(mk & ((1ull << lane) - 1ull));
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        src[3 * at + c] = xyz0[3 * (long long)i + c];
        tgt[3 * at + c] = xyz1[3 * (long long)j + c];
      }
    }
    __syncthreads();        // everyone has read base_s and the waves' counts
    if (t == 0) base_s += tile_total;
    __syncthreads();
  }
  for (long long e = 3 * (long long)n_mutual + t; e < 3 * (long long)m0; e += 1024) {
    src[e] = 0.f;
    tgt[e] = 0.f;
  }
  if (t == 0) {
    count[0] = n_mutual;
    count[1] = n_mutual;
  }
}

__global__ void __launch_bounds__(1024) k_mutual_corr(const int* __restrict__ nn01, int m0, const int* __restrict__ nn10, int m1,
                                                      const float* __restrict__ xyz0, const float* __restrict__ xyz1,
                                                      int min_count, float* __restrict__ src, float* __restrict__ tgt,
                                                      int* __restrict__ count) {
  mutual_corr_body(nn01, m0, nn10, m1, xyz0, xyz1, min_count, src, tgt, count);
}

__global__ void __launch_bounds__(1024) k_mutual_corr_batch(const gcl_mutual_job* __restrict__ jobs, int min_count) {
  const gcl_mutual_job* __restrict__ j = jobs + blockIdx.x;
  mutual_corr_body(j->nn01, j->m0, j->nn10, j->m1, j->xyz0, j->xyz1, min_count, j->src, j->tgt, j->count);
}

}  // namespace gcl

using namespace gcl;

extern "C" {

int64_t gcl_nn3_scratch_len(int32_t m, int32_t n) {
  if (m <= 0 || n <= 0) return 0;
  const long long n_chunks = cdiv(n, nn3_chunk_rows(m, n));
  return n_chunks > 1 ? 2 * n_chunks * (long long)m : 0;
}

int gcl_nn3_rowmin(const float* q, int32_t m, const float* p, int32_t n, const float* feat, int32_t c, int32_t* scratch,
                   float* d2min, int32_t* argmin, float* desc, void* stream) {
  GCL_CHECK_ARG(m >= 0, "gcl_nn3_rowmin: negative query count (%d)", m);
  GCL_CHECK_ARG(n > 0, "gcl_nn3_rowmin: no points to search (n = %d)", n);
  GCL_CHECK_ARG((feat != nullptr) == (desc != nullptr),
                "gcl_nn3_rowmin: feat and desc go together (the fused gather needs both, or neither)");
  GCL_CHECK_ARG(!feat || c >= 1, "gcl_nn3_rowmin: feature width must be >= 1 (got %d)", c);
  if (m == 0) return GCL_OK;
  GCL_CHECK_ARG(q && p && argmin, "gcl_nn3_rowmin: null pointer (q, p and argmin are required)");
  const int chunk = nn3_chunk_rows(m, n);
  const int n_chunks = (int)cdiv(n, chunk);
  GCL_CHECK_ARG(n_chunks == 1 || scratch, "gcl_nn3_rowmin: scratch (int32[gcl_nn3_scratch_len]) is required");
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)cdiv(m, NN3_TQ), (unsigned)n_chunks);
  if (n_chunks == 1) {
    hipLaunchKernelGGL(k_nn3_rowmin, grid, dim3(256), 0, st, q, m, p, n, chunk, (float*)nullptr, argmin, d2min, feat, c, desc);
  } else {
    float* pv = (float*)scratch;
    int* pi = scratch + (long long)n_chunks * m;
    hipLaunchKernelGGL(k_nn3_rowmin, grid, dim3(256), 0, st, q, m, p, n, chunk, pv, pi, (float*)nullptr,
                       (const float*)nullptr, 0, (float*)nullptr);
    hipLaunchKernelGGL(k_nn3_merge, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, st, (const float*)pv, (const int*)pi, m,
                       n_chunks, d2min, argmin, feat, c, desc);
  }
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_mutual_match(const int32_t* nn01, int32_t m0, const int32_t* nn10, int32_t m1, const float* kp0, const float* kp1,
                     const float* T, float tau, int32_t* pairs, int32_t* stats, void* stream) {
  GCL_CHECK_ARG(m0 >= 0 && m1 >= 0, "gcl_mutual_match: negative size (m0 = %d, m1 = %d)", m0, m1);
  GCL_CHECK_ARG(stats, "gcl_mutual_match: null pointer (stats)");
  GCL_CHECK_ARG(m0 == 0 || (nn01 && pairs), "gcl_mutual_match: null pointer (nn01, pairs)");
  GCL_CHECK_ARG(m0 == 0 || m1 == 0 || nn10, "gcl_mutual_match: null pointer (nn10)");
  GCL_CHECK_ARG(!T || (kp0 && kp1), "gcl_mutual_match: a transformation needs both keypoint arrays (null kp0 / kp1)");
  hipLaunchKernelGGL(k_mutual_match, dim3(1), dim3(1024), 0, (hipStream_t)stream, nn01, m0, nn10, m1, kp0, kp1, T, tau, pairs,
                     stats);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_mutual_correspondences(const int32_t* nn01, int32_t m0, const int32_t* nn10, int32_t m1, const float* xyz0,
                               const float* xyz1, int32_t min_count, float* src, float* tgt, int32_t* count, void* stream) {
  GCL_CHECK_ARG(m0 >= 1 && m1 >= 1, "gcl_mutual_correspondences: sizes must be >= 1 (m0 = %d, m1 = %d)", m0, m1);
  GCL_CHECK_ARG(nn01 && nn10 && xyz0 && xyz1 && src && tgt && count, "gcl_mutual_correspondences: null pointer");
  hipLaunchKernelGGL(k_mutual_corr, dim3(1), dim3(1024), 0, (hipStream_t)stream, nn01, m0, nn10, m1, xyz0, xyz1, min_count,
                     src, tgt, count);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_mutual_match_batch(const gcl_mutual_job* jobs_host, const gcl_mutual_job* jobs, int32_t n_pairs, float tau,
                           void* stream) {
  GCL_CHECK_ARG(n_pairs >= 1, "gcl_mutual_match_batch: the number of pairs must be >= 1 (got %d)", n_pairs);
  GCL_CHECK_ARG(jobs_host && jobs, "gcl_mutual_match_batch: null pointer (the table on the host and its device copy)");
  for (int i = 0; i < n_pairs; ++i) {
    const gcl_mutual_job& j = jobs_host[i];
    GCL_CHECK_ARG(j.m0 >= 0 && j.m1 >= 0, "gcl_mutual_match_batch: pair %d: negative size (m0 = %d, m1 = %d)", i, j.m0, j.m1);
    GCL_CHECK_ARG(j.count, "gcl_mutual_match_batch: pair %d: null pointer (count)", i);
    GCL_CHECK_ARG(j.m0 == 0 || (j.nn01 && j.pairs), "gcl_mutual_match_batch: pair %d: null pointer (nn01, pairs)", i);
    GCL_CHECK_ARG(j.m0 == 0 || j.m1 == 0 || j.nn10, "gcl_mutual_match_batch: pair %d: null pointer (nn10)", i);
    GCL_CHECK_ARG(!j.T || (j.xyz0 && j.xyz1),
                  "gcl_mutual_match_batch: pair %d: a transformation needs both keypoint arrays (null xyz0 / xyz1)", i);
  }
  hipLaunchKernelGGL(k_mutual_match_batch, dim3((unsigned)n_pairs), dim3(1024), 0, (hipStream_t)stream, jobs, tau);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_mutual_correspondences_batch(const gcl_mutual_job* jobs_host, const gcl_mutual_job* jobs, int32_t n_pairs,
                                     int32_t min_count, void* stream) {
  GCL_CHECK_ARG(n_pairs >= 1, "gcl_mutual_correspondences_batch: the number of pairs must be >= 1 (got %d)", n_pairs);
  GCL_CHECK_ARG(jobs_host && jobs, "gcl_mutual_correspondences_batch: null pointer (the table on the host and its device copy)");
  for (int i = 0; i < n_pairs; ++i) {
    const gcl_mutual_job& j = jobs_host[i];
    GCL_CHECK_ARG(j.m0 >= 1 && j.m1 >= 1, "gcl_mutual_correspondences_batch: pair %d: sizes must be >= 1 (m0 = %d, m1 = %d)", i,
                  j.m0, j.m1);
    GCL_CHECK_ARG(j.nn01 && j.nn10 && j.xyz0 && j.xyz1 && j.src && j.tgt && j.count,
                  "gcl_mutual_correspondences_batch: pair %d: null pointer", i);
  }
  hipLaunchKernelGGL(k_mutual_corr_batch, dim3((unsigned)n_pairs), dim3(1024), 0, (hipStream_t)stream, jobs, min_count);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

}  // extern "C"
