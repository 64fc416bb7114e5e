// The raw-scan loaders' per-point arithmetic, shared by csrc/data.hip (voxelisation, voxel representatives) and csrc/nghb.hip
// (the complement loaders' neighbourhood crop): one statement of every expression, so that a point is the same number
// wherever it is evaluated.
#pragma once
#include "common.h"

namespace gcl {

__device__ __forceinline__ int floor_to_int(float v) { return (int)floorf(v); }

struct CloudOffsets {
  long long off[65];      // point offsets of up to 64 clouds + the total
};

// chunks of CENT_CHUNK points from a cloud's first point on: a block per chunk reduces in an order that depends on nothing but
// the point's position in ITS cloud (gcl_cloud_centroids), or in no order at all (gcl_nghb_range_max)
constexpr int CENT_CHUNK = 1024;
struct CloudChunks {
  long long off[65];      // point offsets, as CloudOffsets
  int chunk0[65];         // first chunk of every cloud + the total
};

// the cloud of chunk b: last c with chunk0[c] <= b (an empty cloud owns no chunk)
__device__ __forceinline__ int chunk_cloud(const CloudChunks& cc, int n_clouds, int b) {
  int lo = 0, hi = n_clouds - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cc.chunk0[mid] <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// q = ((x0 r0 + x1 r1) + x2 r2) + t in fp32 with T (row-major 3 x 4, fp64) rounded to fp32 first: apply_transform of the
// co-location and complement loaders (lib/colocation_data_loader.py:80-85, lib/complement_data_loader.py:65-70).  No product
// is contracted with a sum (`__fmul_rn` and its kin are plain operators to this compiler and fuse like them).
__device__ __forceinline__ void affine_point_f32(float x0, float x1, float x2, const double* __restrict__ T, float q[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float r0 = (float)T[4 * k], r1 = (float)T[4 * k + 1], r2 = (float)T[4 * k + 2], t = (float)T[4 * k + 3];
    q[k] = ((x0 * r0 + x1 * r1) + x2 * r2) + t;
  }
}

// (x^2 + y^2) + z^2 in fp32, every operation rounded: numpy's (xyz ** 2).sum(-1) of a float32 [P, 3] array
__device__ __forceinline__ float range2_f32(const float y[3]) {
#pragma clang fp contract(off)
  return (y[0] * y[0] + y[1] * y[1]) + y[2] * y[2];
}

// ---- the loader's augmentation on the device: rotation about the cloud's centroid and the sample's scale, folded into the two
// kernels that touch every point anyway (lib/colocation_data_loader.py:349-370, lib/data_loaders.py:476-492) ----------------
// aug: double[n_clouds][12] from the host = R (9, row-major), the scale (1.0: none), rotated (0 / 1), one spare;
// aff: double[n_clouds][12] = T_c = [R | R (-centroid)] from k_cloud_affines.
// A cloud that is not rotated stays float32 in both of the reference's loaders: y = x * fp32(scale).  A rotated cloud is
//   AUG_F32 (co-location loaders: apply_transform casts the transform to float32, colocation_data_loader.py:80-85):
//           y = ((x0 r0 + x1 r1) + x2 r2) + t in fp32, y * fp32(scale), floor(y / fp32(voxel)), representative y;
//   AUG_F64 (pair loaders keep float64 through sparse_quantize, data_loaders.py:125-129):
//           the same expression in fp64, scale * y, floor(y / voxel) by fp64 division, representative fp32(y).
// No product is contracted with a sum: the blocks below switch contraction off (`__fmul_rn` and its kin are plain operators
// to this compiler and fuse like them).  AUG_NONE is the key-less path: y = x.
enum { AUG_NONE = 0, AUG_F32 = 1, AUG_F64 = 2 };

template <int MODE>
__device__ __forceinline__ void loader_point(const float* __restrict__ p, int cloud, const double* __restrict__ aug,
                                             const double* __restrict__ aff, float voxel, double voxel_d, float y[3], int v[3]) {
  const float x0 = p[0], x1 = p[1], x2 = p[2];
  if constexpr (MODE == AUG_NONE) {
    y[0] = x0; y[1] = x1; y[2] = x2;
    // floor(xyz / voxel_size) with the correctly rounded fp32 division numpy performs (util/misc.py:117)
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = floor_to_int(__fdiv_rn(y[k], voxel));
  } else {
    const double scale = aug[12 * cloud + 9];
    const bool rotated = aug[12 * cloud + 10] != 0.0;
    const double* T = aff + 12 * cloud;
    if (!rotated) {
      y[0] = x0 * (float)scale; y[1] = x1 * (float)scale; y[2] = x2 * (float)scale;
#pragma unroll
      for (int k = 0; k < 3; ++k) v[k] = floor_to_int(__fdiv_rn(y[k], voxel));
    } else if constexpr (MODE == AUG_F32) {
      float q[3];
      affine_point_f32(x0, x1, x2, T, q);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        y[k] = q[k] * (float)scale;
        v[k] = floor_to_int(__fdiv_rn(y[k], voxel));
      }
    } else {
#pragma clang fp contract(off)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double q = (((double)x0 * T[4 * k] + (double)x1 * T[4 * k + 1]) + (double)x2 * T[4 * k + 2]) + T[4 * k + 3];
        const double yd = scale * q;
        y[k] = (float)yd;
        v[k] = (int)floor(yd / voxel_d);
      }
    }
  }
}

}  // namespace gcl
