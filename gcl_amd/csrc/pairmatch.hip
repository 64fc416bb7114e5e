// Ground-truth correspondences of scan pairs: get_matching_indices (util/pointcloud.py:53-66) for a ragged
// batch of B pairs in the launches of one.
//
// The reference moves cloud 0 by the ground-truth transform and runs one open3d KD-tree radius query per point; every (i, j)
// inside the radius is a positive pair, per source row nearest first, cut to the first K when K is given.  Here the target
// clouds are voxelised (one point per voxel) and carry the coordinate hash table gcl_unique_coords built, so a radius query is
// a scan of the (2R+1)^3 voxels around the query, R = floor(radius / voxel) + 1 <= 4 -- the search of k_colocation_hits
// (data.hip) with the same arithmetic, so that the repository's two matchers agree:
//   q  = ((x m0 + y m1) + z m2) + t     in fp64 from the fp32 point, no contraction, NOT rounded to fp32
//   d2 = ((ex ex + ey ey) + ez ez)      against the fp32 target point widened to fp64
//   hit: d2 < r r (strictly);  order within a source row: (d2, j) ascending
// Unlike the co-location groups, K = None has no small bound (251 hits per query at radius 3.9 voxels), so the per-query order
// cannot live in registers: ONE WAVE serves one query, its lanes share the candidate voxels, the hits go to an LDS list of the
// wave, and every hit's place is its rank in that list (the number of hits that order before it -- (d2, j) is a total order,
// as the merge by rank of k_fpfh_neighbours).  Count, scan, emit: the emit pass recomputes the hits instead of reading them
// back from a scratch whose size would only be known after the count.
// No atomics, no floating-point accumulation; every index is compared bit-exactly with tests/pair_matches_oracle.py.
#include "common.h"

namespace gcl {

constexpr int PM_QUERIES = 4;        // queries (= waves) per workgroup
constexpr int PM_MAXC = 729;         // candidate voxels of a query, 9^3: the capacity of a query's hit list
constexpr int PM_MAXR = 4;
constexpr int PM_BAD_OFFSETS = 1, PM_BAD_RADIUS = 2;      // status words (meta[1])

// meta[1] = 0, or why the batch is refused (then no kernel of the batch writes anything else): offsets that are not
// 0 <= o[b] <= o[b+1] <= total, or a radius that is not in (0, radius_max]
__global__ void __launch_bounds__(256) k_pair_check(const long long* __restrict__ off0, long long total0,
                                                    const long long* __restrict__ off1, long long total1, int B,
                                                    const double* __restrict__ radii, double radius_max, long long* meta) {
  int bad = 0;
  for (int b = threadIdx.x; b < B; b += 256) {
    const long long a0 = off0[b], e0 = off0[b + 1], a1 = off1[b], e1 = off1[b + 1];
    if (a0 < 0 || a0 > e0 || e0 > total0 || a1 < 0 || a1 > e1 || e1 > total1) bad |= PM_BAD_OFFSETS;
    const double r = radii[b];
    if (!(r > 0.0 && r <= radius_max)) bad |= PM_BAD_RADIUS;
  }
  const int any_off = __syncthreads_or(bad & PM_BAD_OFFSETS), any_rad = __syncthreads_or(bad & PM_BAD_RADIUS);   // predicates
  if (threadIdx.x == 0) meta[1] = any_off ? PM_BAD_OFFSETS : (any_rad ? PM_BAD_RADIUS : 0);
}

// floor, clamped well outside the packable +-32768 so that the window's additions cannot overflow (pack_ok then says no)
__device__ __forceinline__ int pm_floor(double v) { return (int)fmin(fmax(floor(v), -100000.0), 100000.0); }

// One wave per source row.  EMIT = false: cnt[i] = number of kept hits.  EMIT = true: the kept hits, in order, at
// pairs[row_off[i] ...].
template <bool EMIT>
__global__ void __launch_bounds__(64 * PM_QUERIES) k_pair_matches(
    const float* __restrict__ xyz0, long long total0, const long long* __restrict__ off0, const float* __restrict__ xyz1,
    const long long* __restrict__ off1, const long long* __restrict__ table_row0, int B, const Slot* __restrict__ table,
    long long cap, int cloud0, int cloud_stride, float voxel, const double* __restrict__ trans,
    const double* __restrict__ radii, int K, int absolute, const long long* __restrict__ meta, int* __restrict__ cnt,
    const int* __restrict__ row_off, long long* __restrict__ pairs, long long pairs_cap) {
  __shared__ double s_d[PM_QUERIES][PM_MAXC];
  __shared__ int s_j[PM_QUERIES][PM_MAXC];
  if (meta[1] != 0) return;                                  // refused batch (uniform: every thread leaves)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * PM_QUERIES + wave;
  // the pair of row i: the last b with off0[b] <= i (an empty cloud shares its start with the next one); wave-uniform
  int b = -1;
  if (i < total0 && off0[0] <= i && i < off0[B]) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (off0[mid] <= i) lo = mid; else hi = mid - 1;
    }
    b = lo;
  }
  int n = 0;                                                 // hits of the query (wave-uniform)
  long long base1 = 0;
  if (b >= 0) {
    const double* m = trans + 12 * (long long)b;
    const double x = xyz0[3 * i], y = xyz0[3 * i + 1], z = xyz0[3 * i + 2];
    const double qx = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(x, m[0]), __dmul_rn(y, m[1])), __dmul_rn(z, m[2])), m[3]);
    const double qy = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(x, m[4]), __dmul_rn(y, m[5])), __dmul_rn(z, m[6])), m[7]);
    const double qz = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(x, m[8]), __dmul_rn(y, m[9])), __dmul_rn(z, m[10])), m[11]);
    const double radius = radii[b], r2 = __dmul_rn(radius, radius);
    // The query's voxel, by the division the table's coordinates were made with (floor(x / voxel)) but in fp64: its error is
    // ~1e-12 voxels at the edge of the packable range, where a product with an fp32 1 / voxel would be off by 2e-3 voxels
    // and the +-R window could miss the outermost voxel of a hit.
    const double vd = (double)voxel;
    const double tx = qx / vd, ty = qy / vd, tz = qz / vd;
    const int bx = pm_floor(tx), by = pm_floor(ty), bz = pm_floor(tz);
    const int R = (int)(radius / vd) + 1;                    // <= PM_MAXR: k_pair_check passed
    // The box test of k_colocation_hits: a voxel whose BOX is farther from the query than the radius cannot hold a hit and is
    // skipped before its probe.  Per-axis gaps in voxel units, shortened by 0.004 voxels (a point within one fp32 rounding
    // below a voxel face is filed under the voxel above: 2e-3 voxels at +-32767), so the test only ever errs towards probing.
    const float fx = (float)(tx - (double)bx), fy = (float)(ty - (double)by), fz = (float)(tz - (double)bz);
    const float rv = (float)(radius / vd), rv2 = rv * rv * 1.0001f;
    auto gap2 = [](int d, float f) {
      const float g = fmaxf((d > 0 ? (float)d - f : (d < 0 ? f - (float)(d + 1) : 0.f)) - 0.004f, 0.f);
      return g * g;
    };
    const int W = 2 * R + 1, W3 = W * W * W;
    const unsigned MW = 65535u / (unsigned)W + 1u;           // (v * MW) >> 16 == v / W for v < 729 (W <= 9)
    const int cloud = cloud0 + b * cloud_stride;
    base1 = off1[b];
    const long long n1 = off1[b + 1] - base1;
    const long long val0 = table_row0 ? table_row0[b] : base1;      // the table's value of the target's first row
    for (int c0 = 0; c0 < W3; c0 += 64) {                    // <= 12 rounds, the same number for every lane
      const int cand = c0 + lane;
      bool hit = false;
      double d2 = 0.0;
      long long rel = 0;
      if (cand < W3) {
        const unsigned t = ((unsigned)cand * MW) >> 16, uz = (t * MW) >> 16;
        const int dz = (int)uz - R, dy = (int)(t - uz * W) - R, dx = (int)((unsigned)cand - t * W) - R;
        const int vx = bx + dx, vy = by + dy, vz = bz + dz;
        if (gap2(dx, fx) + gap2(dy, fy) + gap2(dz, fz) <= rv2 && pack_ok(cloud, vx, vy, vz)) {
          const long long s = table_find(table, cap, pack_key(cloud, vx, vy, vz));
          if (s >= 0) {
            rel = table[s].val - val0;
            if (rel >= 0 && rel < n1) {                      // a -1 or foreign value is never dereferenced
              const long long j = base1 + rel;
              const double ex = __dsub_rn((double)xyz1[3 * j], qx);
              const double ey = __dsub_rn((double)xyz1[3 * j + 1], qy);
              const double ez = __dsub_rn((double)xyz1[3 * j + 2], qz);
              d2 = __dadd_rn(__dadd_rn(__dmul_rn(ex, ex), __dmul_rn(ey, ey)), __dmul_rn(ez, ez));
              hit = d2 < r2;                                 // strictly inside (nanoflann's test)
            }
          }
        }
      }
      const unsigned long long mask = __ballot(hit);
      if (EMIT && hit) {
        const int slot = n + __popcll(mask & ((1ull << lane) - 1ull));
        s_d[wave][slot] = d2;
        s_j[wave][slot] = (int)rel;
      }
      n += __popcll(mask);
    }
  }
  const int kept = (K > 0 && n > K) ? K : n;
  if (!EMIT) {
    if (lane == 0 && i < total0) cnt[i] = kept;
    return;
  }
  __syncthreads();                                           // the lists are complete (every wave of the block gets here)
  if (kept == 0) return;
  const long long o = row_off[i];
  const long long add0 = absolute ? 0 : off0[b], add1 = absolute ? base1 : 0;
  for (int t = lane; t < n; t += 64) {
    const double d = s_d[wave][t];
    const int j = s_j[wave][t];
    int rank = 0;
    for (int u = 0; u < n; ++u) {
      const double du = s_d[wave][u];
      rank += (du < d || (du == d && s_j[wave][u] < j)) ? 1 : 0;
    }
    if (rank < kept && o + rank < pairs_cap) {
      pairs[2 * (o + rank)] = i - add0;
      pairs[2 * (o + rank) + 1] = (long long)j + add1;
    }
  }
}

// matches before source row e (0 <= e <= total0)
__device__ __forceinline__ long long pm_before(const int* cnt, const int* row_off, long long total0, long long e) {
  if (total0 == 0 || e == 0) return 0;
  return e == total0 ? (long long)row_off[e - 1] + cnt[e - 1] : (long long)row_off[e];
}

__global__ void k_pair_totals(const int* __restrict__ cnt, const int* __restrict__ row_off, long long total0,
                              const long long* __restrict__ off0, int B, long long* meta) {
  if (meta[1] != 0) return;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b == 0) meta[0] = pm_before(cnt, row_off, total0, total0);
  if (b < B) meta[2 + b] = pm_before(cnt, row_off, total0, off0[b + 1]) - pm_before(cnt, row_off, total0, off0[b]);
}

static int pm_check_args(const char* who, const void* xyz0, int64_t total0, const void* off0, const void* xyz1, int64_t total1,
                         const void* off1, int32_t B, const void* table, int64_t cap, int32_t cloud0, int32_t cloud_stride,
                         float voxel, const void* trans, const void* radii, double radius_max, int32_t K) {
  GCL_CHECK_ARG(off0 && off1 && table && trans && radii && (xyz0 || total0 == 0) && (xyz1 || total1 == 0),
                "%s: null pointer", who);
  GCL_CHECK_ARG(B >= 1 && total0 >= 0 && total1 >= 0 && K >= 0 && cap >= 2 && (cap & (cap - 1)) == 0, "%s: bad sizes", who);
  GCL_CHECK_ARG(cloud0 >= 0 && cloud_stride >= 0 && (int64_t)cloud0 + (int64_t)(B - 1) * cloud_stride < 65535,
                "%s: cloud ids must stay below 65535", who);
  GCL_CHECK_ARG(total0 <= 0x7fffffffll / PM_MAXC, "%s: too many source rows for 32-bit match offsets", who);
  GCL_CHECK_ARG(voxel > 0 && radius_max > 0, "%s: radius and voxel size must be positive", who);
  GCL_CHECK_ARG(radius_max / (double)voxel < (double)PM_MAXR,
                "%s: radius / voxel = %g, supported below %d (at most 9^3 candidate voxels per query)", who,
                radius_max / (double)voxel, PM_MAXR);
  return GCL_OK;
}

}  // namespace gcl

using namespace gcl;

extern "C" {

int64_t gcl_pair_matches_scratch_len(int64_t total0) {
  return total0 <= 0 ? 64 : total0 + total0 / 2048 + 64;      // row offsets + the scan's block totals
}

int gcl_pair_matches_count(const float* xyz0, int64_t total0, const int64_t* offsets0, const float* xyz1, int64_t total1,
                           const int64_t* offsets1, const int64_t* table_row0, int32_t n_pairs, const int64_t* table,
                           int64_t cap, int32_t cloud0, int32_t cloud_stride, float voxel, const double* trans,
                           const double* radii, double radius_max, int32_t K, int32_t* cnt, int32_t* scratch, int64_t* meta,
                           void* stream) {
  int rc = pm_check_args("gcl_pair_matches_count", xyz0, total0, offsets0, xyz1, total1, offsets1, n_pairs, table, cap, cloud0,
                         cloud_stride, voxel, trans, radii, radius_max, K);
  if (rc) return rc;
  GCL_CHECK_ARG(scratch && meta && (cnt || total0 == 0), "gcl_pair_matches_count: null pointer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_pair_check, dim3(1), dim3(256), 0, st, (const long long*)offsets0, (long long)total0,
                     (const long long*)offsets1, (long long)total1, n_pairs, radii, radius_max, (long long*)meta);
  GCL_CHECK_LAUNCH();
  if (total0 > 0) {
    hipLaunchKernelGGL(k_pair_matches<false>, dim3((unsigned)cdiv(total0, PM_QUERIES)), dim3(64 * PM_QUERIES), 0, st, xyz0,
                       (long long)total0, (const long long*)offsets0, xyz1, (const long long*)offsets1,
                       (const long long*)table_row0, n_pairs, (const Slot*)table, (long long)cap, cloud0, cloud_stride, voxel,
                       trans, radii, K, 0, (const long long*)meta, cnt, (const int*)nullptr, (long long*)nullptr, 0ll);
    GCL_CHECK_LAUNCH();
    // (a refused batch leaves cnt as it was: the scan then runs over whatever it holds, into the scratch only)
    rc = gcl_exclusive_scan_i32(cnt, total0, scratch, scratch + total0, stream);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_pair_totals, dim3((unsigned)cdiv(n_pairs, 256)), dim3(256), 0, st, (const int*)cnt, (const int*)scratch,
                     (long long)total0, (const long long*)offsets0, n_pairs, (long long*)meta);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_pair_matches_emit(const float* xyz0, int64_t total0, const int64_t* offsets0, const float* xyz1, int64_t total1,
                          const int64_t* offsets1, const int64_t* table_row0, int32_t n_pairs, const int64_t* table,
                          int64_t cap, int32_t cloud0, int32_t cloud_stride, float voxel, const double* trans,
                          const double* radii, double radius_max, int32_t K, int32_t absolute, const int32_t* scratch,
                          const int64_t* meta, int64_t* pairs, int64_t n_matches, void* stream) {
  int rc = pm_check_args("gcl_pair_matches_emit", xyz0, total0, offsets0, xyz1, total1, offsets1, n_pairs, table, cap, cloud0,
                         cloud_stride, voxel, trans, radii, radius_max, K);
  if (rc) return rc;
  GCL_CHECK_ARG(scratch && meta && n_matches >= 0 && (pairs || n_matches == 0), "gcl_pair_matches_emit: null pointer");
  if (total0 == 0 || n_matches == 0) return GCL_OK;
  hipLaunchKernelGGL(k_pair_matches<true>, dim3((unsigned)cdiv(total0, PM_QUERIES)), dim3(64 * PM_QUERIES), 0,
                     (hipStream_t)stream, xyz0, (long long)total0, (const long long*)offsets0, xyz1,
                     (const long long*)offsets1, (const long long*)table_row0, n_pairs, (const Slot*)table, (long long)cap,
                     cloud0, cloud_stride, voxel, trans, radii, K, absolute, (const long long*)meta, (int*)nullptr, scratch,
                     (long long*)pairs, (long long)n_matches);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

}  // extern "C"
