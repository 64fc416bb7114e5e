// The uniform neighbour grid shared by the radius searches (fpfh.hip: the lists of the FPFH descriptors; icp.hip: the nearest
// target of point-to-point ICP): a point's cell as a 63-bit key (cloud, cx, cy, cz), z the lowest field, the search in the
// sorted keys, and the squared distance both searches compare against r2.
#pragma once
#include "common.h"

#include <math.h>

namespace gcl {

constexpr int FP_CELL_MAX = 32767, FP_CELL_MIN = -32768;

// d2 = (dx dx + dy dy) + dz dz, each operation rounded (an fma would give other bits)
__device__ __forceinline__ double fp_d2(double ax, double ay, double az, double bx, double by, double bz) {
  const double dx = ax - bx, dy = ay - by, dz = az - bz;
  return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

// cloud of row i: the b with off[b] <= i < off[b + 1] (off ascending, off[0] = 0, off[B] = n); at most 32 halvings
__device__ __forceinline__ int fp_cloud_of(const long long* __restrict__ off, int B, long long i) {
  int lo = 0, hi = B - 1;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ int fp_cell(double x, double inv_edge) {
  const double c = floor(x * inv_edge);
  // the clamp is monotone and 1-Lipschitz: two cells that differ by at most one still do after it, so the 27-cell scan stays
  // complete; a non-finite coordinate lands in a border cell and fails the distance test there
  return c >= (double)FP_CELL_MAX ? FP_CELL_MAX : (c <= (double)FP_CELL_MIN ? FP_CELL_MIN : (int)c);
}
__device__ __forceinline__ long long fp_key(int b, int cx, int cy, int cz) {
  return ((long long)b << 48) | ((long long)(cx - FP_CELL_MIN) << 32) | ((long long)(cy - FP_CELL_MIN) << 16) |
         (long long)(cz - FP_CELL_MIN);
}

// first position in the ascending keys[0, n) whose key is >= k; at most 64 halvings
__device__ __forceinline__ long long fp_lower_bound(const long long* __restrict__ keys, long long n, long long k) {
  long long lo = 0, hi = n;
  for (int it = 0; it < 64 && lo < hi; ++it) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

static inline double fp_inv_edge(float radius) {
  // an edge a little above the radius: two points with d2 <= r2 as rounded are never two cells apart
  return 1.0 / ((double)radius * 1.000001);
}

}  // namespace gcl
