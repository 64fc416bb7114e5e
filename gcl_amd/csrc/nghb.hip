// The complement pair loaders' neighbourhood cloud (PairComplementKittiDataset / PairComplementNuscenesDataset.__getitem__,
// lib/complement_data_loader.py:576-628, :1028-1060) for every side of a batch at once.  A SIDE is one centre scan of a pair
// (side 2 b + s of sample b) with the complement SCANS that are merged into its neighbourhood:
//
//   c = f32(M_k) x                 every complement scan k moved into its centre scan's frame          (:576-579)
//   c = f32(T_s) c                 and, where the side is rotated, by the centre scan's T_s = [R | R (-centroid)], applied to
//                                  the ROUNDED result of the first transform -- two float32 transforms, never one composed (:609-612)
//   max_s = max (x^2 + y^2) + z^2  over the centre scan moved by f32(T_s), before any scale              (:623-624)
//   keep c  <=>  (cx^2 + cy^2) + cz^2 < max_s        strictly, in float32                                (:627-628)
//   the kept points of a side in scan order, then point order                                            (:625-626)
//
// Every expression is loader.h's (apply_transform in float32, products and sums uncontracted), so a point that goes on to
// gcl_voxel_coords_aug / gcl_loader_points_aug is the number numpy makes of it, bit for bit.
#include "common.h"
#include "loader.h"

#include <limits.h>

namespace gcl {

constexpr int NGHB_MAX_SCANS = GCL_NGHB_MAX_SCANS;
struct ScanTable {
  long long off[NGHB_MAX_SCANS + 1];      // point offsets of the complement scans + the total
  unsigned char side[NGHB_MAX_SCANS];     // the side a scan belongs to
};

// max over a centre cloud of the squared range of its moved points.  A maximum does not depend on the order it is taken in:
// a fixed LDS tree per chunk of CENT_CHUNK points, then an INTEGER atomic max on the bit pattern (non-negative floats order like
// unsigned integers) -- the result is the same alone, anywhere in a batch and on every run.  max_bits is zero on entry (0.0f).
__global__ void __launch_bounds__(256) k_nghb_range_max(const float* __restrict__ xyz, CloudChunks cc, int n_clouds,
                                                        const double* __restrict__ aug, const double* __restrict__ aff,
                                                        unsigned* __restrict__ max_bits) {
  __shared__ float sh[256];
  const int b = blockIdx.x, t = threadIdx.x;
  const int c = chunk_cloud(cc, n_clouds, b);
  const long long first = cc.off[c] + (long long)(b - cc.chunk0[c]) * CENT_CHUNK;
  const long long last = first + CENT_CHUNK < cc.off[c + 1] ? first + CENT_CHUNK : cc.off[c + 1];
  const bool rotated = aug[12 * c + 10] != 0.0;
  float m = 0.f;
  for (long long i = first + t; i < last; i += 256) {
    float y[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    if (rotated) affine_point_f32(y[0], y[1], y[2], aff + 12 * c, y);
    m = fmaxf(m, range2_f32(y));
  }
  sh[t] = m;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) sh[t] = fmaxf(sh[t], sh[t + w]);
    __syncthreads();
  }
  if (t == 0) atomicMax(max_bits + c, __float_as_uint(sh[0]));
}

// one thread per complement point of the whole batch: the one or two float32 transforms, the squared range, the strict compare
__global__ void __launch_bounds__(256) k_nghb_flags(const float* __restrict__ cmpl, long long pc, ScanTable st, int n_scans,
                                                    const double* __restrict__ scan_aff, const double* __restrict__ aug,
                                                    const double* __restrict__ aff, const float* __restrict__ max_r2,
                                                    float* __restrict__ moved, int* __restrict__ flags) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pc) return;
  int lo = 0, hi = n_scans - 1;      // the scan of point i: last k with off[k] <= i (an empty scan owns no point)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (st.off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  const int s = st.side[lo];
  float c[3];
  affine_point_f32(cmpl[3 * i], cmpl[3 * i + 1], cmpl[3 * i + 2], scan_aff + 12 * lo, c);
  if (aug[12 * s + 10] != 0.0) affine_point_f32(c[0], c[1], c[2], aff + 12 * s, c);
  moved[3 * i] = c[0]; moved[3 * i + 1] = c[1]; moved[3 * i + 2] = c[2];
  flags[i] = range2_f32(c) < max_r2[s] ? 1 : 0;
}

// order-preserving compaction: pos = exclusive scan of the flags; kept[s] = kept points of side s, kept[n_sides] = all of them
__global__ void __launch_bounds__(256) k_nghb_compact(const float* __restrict__ moved, const int* __restrict__ flags,
                                                      const int* __restrict__ pos, long long pc, CloudOffsets so, int n_sides,
                                                      float* __restrict__ out, int* __restrict__ kept) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n_sides) {
    const int total = pos[pc - 1] + flags[pc - 1];
    const long long a = i < n_sides ? so.off[i] : 0, e = i < n_sides ? so.off[i + 1] : pc;
    kept[i] = (e < pc ? pos[e] : total) - (a < pc ? pos[a] : total);
  }
  if (i >= pc || !flags[i]) return;
  const long long o = pos[i];
  out[3 * o] = moved[3 * i]; out[3 * o + 1] = moved[3 * i + 1]; out[3 * o + 2] = moved[3 * i + 2];
}

static bool ascending_to(const int64_t* off, int32_t n, int64_t total) {
  if (off[0] != 0 || off[n] != total) return false;
  for (int c = 0; c < n; ++c)
    if (off[c + 1] < off[c]) return false;
  return true;
}

}  // namespace gcl

using namespace gcl;

extern "C" {

int gcl_nghb_range_max(const float* xyz, int64_t p, const int64_t* cloud_offsets_host, int32_t n_clouds, const double* aug_dev,
                       const double* aff_dev, float* max_dev, void* stream) {
  GCL_CHECK_ARG(p >= 0 && n_clouds >= 0, "gcl_nghb_range_max: negative count");
  GCL_CHECK_ARG(n_clouds >= 1 && n_clouds <= 64, "gcl_nghb_range_max: 1 <= clouds <= 64");
  GCL_CHECK_ARG(cloud_offsets_host && aug_dev && aff_dev && max_dev && (xyz || p == 0), "gcl_nghb_range_max: null pointer");
  GCL_CHECK_ARG(ascending_to(cloud_offsets_host, n_clouds, p),
                "gcl_nghb_range_max: ascending offsets, offsets[0] = 0, offsets[clouds] = p");
  CloudChunks cc;
  int64_t chunks = 0;
  for (int c = 0; c <= n_clouds; ++c) {
    cc.off[c] = cloud_offsets_host[c];
    cc.chunk0[c] = (int)chunks;
    if (c < n_clouds) chunks += cdiv(cloud_offsets_host[c + 1] - cloud_offsets_host[c], CENT_CHUNK);
  }
  GCL_CHECK_ARG(chunks <= INT_MAX / 4, "gcl_nghb_range_max: too many points");
  GCL_CHECK_HIP(hipMemsetAsync(max_dev, 0, (size_t)n_clouds * sizeof(float), (hipStream_t)stream));      // 0.0f: an empty cloud
  if (chunks == 0) return GCL_OK;
  hipLaunchKernelGGL(k_nghb_range_max, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, xyz, cc, n_clouds, aug_dev,
                     aff_dev, (unsigned*)max_dev);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_nghb_flags(const float* cmpl, int64_t pc, const int64_t* scan_offsets_host, const int32_t* scan_side_host,
                   int32_t n_scans, int32_t n_sides, const double* scan_aff_dev, const double* aug_dev, const double* aff_dev,
                   const float* max_dev, float* moved, int32_t* flags, void* stream) {
  GCL_CHECK_ARG(pc >= 0 && n_scans >= 0 && n_sides >= 0, "gcl_nghb_flags: negative count");
  GCL_CHECK_ARG(n_sides >= 1 && n_sides <= 64, "gcl_nghb_flags: 1 <= sides <= 64 (the centre clouds of gcl_nghb_range_max)");
  GCL_CHECK_ARG(n_scans <= NGHB_MAX_SCANS, "gcl_nghb_flags: more than %d complement scans", NGHB_MAX_SCANS);
  GCL_CHECK_ARG(pc <= INT_MAX / 4, "gcl_nghb_flags: too many points");
  if (n_scans == 0) {
    GCL_CHECK_ARG(pc == 0, "gcl_nghb_flags: points without a scan");
    return GCL_OK;
  }
  GCL_CHECK_ARG(scan_offsets_host && scan_side_host, "gcl_nghb_flags: null pointer");
  GCL_CHECK_ARG(ascending_to(scan_offsets_host, n_scans, pc),
                "gcl_nghb_flags: ascending offsets, offsets[0] = 0, offsets[scans] = pc");
  for (int k = 0; k < n_scans; ++k)
    GCL_CHECK_ARG(scan_side_host[k] >= 0 && scan_side_host[k] < n_sides && (k == 0 || scan_side_host[k] >= scan_side_host[k - 1]),
                  "gcl_nghb_flags: scan %d: its side must be in 0 .. sides - 1 and not below the scan's before it", k);
  if (pc == 0) return GCL_OK;
  GCL_CHECK_ARG(cmpl && scan_aff_dev && aug_dev && aff_dev && max_dev && moved && flags, "gcl_nghb_flags: null pointer");
  ScanTable st;
  for (int k = 0; k <= n_scans; ++k) st.off[k] = scan_offsets_host[k];
  for (int k = 0; k < n_scans; ++k) st.side[k] = (unsigned char)scan_side_host[k];
  hipLaunchKernelGGL(k_nghb_flags, dim3((unsigned)cdiv(pc, 256)), dim3(256), 0, (hipStream_t)stream, cmpl, (long long)pc, st,
                     n_scans, scan_aff_dev, aug_dev, aff_dev, max_dev, moved, flags);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int64_t gcl_nghb_scratch_len(int64_t pc) {
  if (pc <= 0 || pc > INT_MAX / 4) return 0;
  return pc + pc / 2048 + 64;      // the flags' prefix sums + gcl_exclusive_scan_i32's scratch
}

int gcl_nghb_compact(const float* moved, const int32_t* flags, int64_t pc, const int64_t* side_offsets_host, int32_t n_sides,
                     int32_t* scratch, float* out, int32_t* kept_dev, void* stream) {
  GCL_CHECK_ARG(pc >= 0 && n_sides >= 0, "gcl_nghb_compact: negative count");
  GCL_CHECK_ARG(n_sides >= 1 && n_sides <= 64, "gcl_nghb_compact: 1 <= sides <= 64");
  GCL_CHECK_ARG(pc <= INT_MAX / 4, "gcl_nghb_compact: too many points");
  GCL_CHECK_ARG(side_offsets_host && kept_dev, "gcl_nghb_compact: null pointer");
  GCL_CHECK_ARG(ascending_to(side_offsets_host, n_sides, pc),
                "gcl_nghb_compact: ascending offsets, offsets[0] = 0, offsets[sides] = pc");
  if (pc == 0) {
    GCL_CHECK_HIP(hipMemsetAsync(kept_dev, 0, (size_t)(n_sides + 1) * sizeof(int32_t), (hipStream_t)stream));
    return GCL_OK;
  }
  GCL_CHECK_ARG(moved && flags && scratch && out, "gcl_nghb_compact: null pointer");
  int* pos = scratch;
  const int rc = gcl_exclusive_scan_i32(flags, pc, pos, scratch + pc, stream);
  if (rc) return rc;
  CloudOffsets so;
  for (int c = 0; c <= n_sides; ++c) so.off[c] = side_offsets_host[c];
  hipLaunchKernelGGL(k_nghb_compact, dim3((unsigned)cdiv(pc > n_sides ? pc : n_sides + 1, 256)), dim3(256), 0,
                     (hipStream_t)stream, moved, (const int*)flags, (const int*)pos, (long long)pc, so, n_sides, out, kept_dev);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

}  // extern "C"
