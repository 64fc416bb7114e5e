// Native step runtime: one C call enqueues a whole pass (include/gcl_amd.h, "Native step runtime").
//
//   gcl_maps_build     = what CoordinateManager.__init__ / _build_stride_maps / get_kernel_map / KernelMap.sorted_table /
//                        KernelMap.pairs do from Python (gcl_amd/MinkowskiEngine/core.py), for all maps of a network;
//   gcl_plan_forward / = what ops.Tape records and replays (gcl_amd/MinkowskiEngine/ops.py: _SparseConvFn, _BatchNormFn,
//   gcl_plan_backward    Tape.backward) for a network given as operator records.
//
// Reference path: model/resunet.py:173-232 (ResUNet2.forward), model/residual_block.py:37-53, and the coordinate manager
// ME builds behind lib/colocation_trainer.py:843-845.  Both families call the SAME extern "C" entries the per-operator
// path calls, with the same arguments in the same order, so results are bitwise identical (tests/test_gpu_plan.py); what
// disappears is ~560 Python -> ctypes round trips (~40 us each) per training step.
// Memory: bump allocation from the caller's arena, nothing is freed inside a pass (288 GB of HBM: a 0.5 M-voxel step
// uses a few GB); a dry run of the same code sizes the arena.
#include "common.h"

#include <string.h>

#include <algorithm>
#include <new>
#include <utility>
#include <vector>

namespace gcl {

// ---------------------------------------------------------------------------------------------------
// small elementwise kernels of the plan path
// ---------------------------------------------------------------------------------------------------
// max |v| of what a workgroup wrote -> the tensor's amax slot (same value gcl_amax would measure in a pass of its own)
__device__ __forceinline__ float amax4p(float m, const float4& v) {
  return fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
}
__device__ __forceinline__ void publish_amax_wg(float m, int* slot) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  __shared__ float wm[4];
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0)
    amax_slot_publish(slot, __float_as_int(fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]))), blockIdx.x);
}

// MEF.relu: torch.relu semantics (NaN propagates); amax (optional): zero-initialised slot that receives max|y|
__global__ void __launch_bounds__(256) k_relu_fwd(const float4* __restrict__ x, long long n4, float4* __restrict__ y,
                                                  int* amax) {
  float m = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    float4 v = x[i];
    v.x = v.x < 0.f ? 0.f : v.x;
    v.y = v.y < 0.f ? 0.f : v.y;
    v.z = v.z < 0.f ? 0.f : v.z;
    v.w = v.w < 0.f ? 0.f : v.w;
    y[i] = v;
    m = amax4p(m, v);
  }
  if (amax) publish_amax_wg(m, amax);
}
// aten::threshold_backward(g, y, 0): g where y > 0, else 0
__global__ void __launch_bounds__(256) k_relu_bwd(const float4* __restrict__ g, const float4* __restrict__ y, long long n4,
                                                  float4* __restrict__ gx, int* amax) {
  float m = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    float4 a = g[i];
    const float4 b = y[i];
    a.x = b.x > 0.f ? a.x : 0.f;
    a.y = b.y > 0.f ? a.y : 0.f;
    a.z = b.z > 0.f ? a.z : 0.f;
    a.w = b.w > 0.f ? a.w : 0.f;
    gx[i] = a;
    m = amax4p(m, a);
  }
  if (amax) publish_amax_wg(m, amax);
}
// ME.cat(a, b): y[r] = a[r] | b[r]   (channel counts are multiples of 4)
// sa / sb (both or neither): the inputs' amax slots -- the cat's slot becomes their elementwise maximum (a valid slot of
// max(value a, value b); was a launch of its own, k_slot_max) and nothing is measured
__global__ void __launch_bounds__(256) k_cat2(const float4* __restrict__ a, int ca4, const float4* __restrict__ b, int cb4,
                                              long long n, float4* __restrict__ y, int* amax, const int* __restrict__ sa,
                                              const int* __restrict__ sb) {
  if (sa && blockIdx.x == 0)
    for (int w = threadIdx.x; w < AMAX_WORDS; w += 256) amax[w] = max(sa[w], sb[w]);
  if (sa) amax = nullptr;
  const int c4 = ca4 + cb4;
  const long long total = n * c4;
  float m = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long r = i / c4;
    const int q = (int)(i - r * c4);
    const float4 v = q < ca4 ? a[r * ca4 + q] : b[r * cb4 + (q - ca4)];
    y[i] = v;
    m = amax4p(m, v);
  }
  if (amax) publish_amax_wg(m, amax);
}
// ME.cat whose left input was written in place by its producer: copy the right input's columns, y[r][ca..] = b[r]
// planes (round 5): the cat's plane image gets these columns too, at the scale of `amax` -- then a slot that already holds a
// bound of the WHOLE cat (the left input's BatchNorm statistics launch folded this input's maximum in): nothing is published
__global__ void __launch_bounds__(256) k_cat_right(const float4* __restrict__ b, int cb4, long long n, int ca4,
                                                   float4* __restrict__ y, int* amax, unsigned short* __restrict__ planes) {
  const int c4 = ca4 + cb4;
  const long long total = n * cb4;
  const float pscale = planes ? amax_scale(amax) : 1.f;
  float m = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long r = i / cb4;
    const int q = (int)(i - r * cb4);
    const float4 v = b[i];
    y[r * c4 + ca4 + q] = v;
    if (planes) store_planes4(planes, r, (long long)c4 * 4, (ca4 + q) * 4, v, pscale);
    m = amax4p(m, v);
  }
  if (amax && !planes) publish_amax_wg(m, amax);
}
// y = a + b for row-major [n, c] operands with row pitches (floats; a column slice of a wider tensor has pitch > c);
// b == NULL: y = a (materialises a slice)
__global__ void __launch_bounds__(256) k_add2_ld(const float* __restrict__ a, int a_ld, const float* __restrict__ b, int b_ld,
                                                 long long n, int c4, float4* __restrict__ y) {
  const long long total = n * c4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long r = i / c4;
    const int q = (int)(i - r * c4);
    float4 u = reinterpret_cast<const float4*>(a + r * a_ld)[q];
    if (b) {
      const float4 v = reinterpret_cast<const float4*>(b + r * b_ld)[q];
      u = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
    }
    y[i] = u;
  }
}
__global__ void __launch_bounds__(256) k_add2(const float4* __restrict__ a, const float4* __restrict__ b, long long n4,
                                              float4* __restrict__ y) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const float4 u = a[i], v = b[i];
    y[i] = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
  }
}
// rows of a row-major [n_src, cv] tensor of V (float4, or float for a column of scalars; row pitch ld floats: a column slice
// has pitch > its width) picked by a row list: out[j] = src[rows[j]], or `pad` in every component where rows[j] is the -1
// padding or lies outside the tensor
template <typename V>
__device__ __forceinline__ V splat(float v);
template <>
__device__ __forceinline__ float splat<float>(float v) { return v; }
template <>
__device__ __forceinline__ float4 splat<float4>(float v) { return make_float4(v, v, v, v); }
template <typename V>
__global__ void __launch_bounds__(256) k_gather_rows(const float* __restrict__ src, int ld, long long n_src,
                                                     const int* __restrict__ rows, long long cap, int cv, float pad,
                                                     V* __restrict__ out) {
  const long long total = cap * cv;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long j = i / cv;
    const int q = (int)(i - j * cv);
    const long long r = rows[j];
    out[i] = (r >= 0 && r < n_src) ? reinterpret_cast<const V*>(src + r * ld)[q] : splat<V>(pad);
  }
}
// the inverse: dst[rows[j]] = src[j] for the rows of the list that lie inside dst ([n_dst, c4 float4], row pitch ld floats);
// the list holds a row at most once and the caller has zero-filled dst
__global__ void __launch_bounds__(256) k_scatter_rows(const float4* __restrict__ src, const int* __restrict__ rows,
                                                      long long cap, int c4, long long n_dst, float* __restrict__ dst,
                                                      int ld) {
  const long long total = cap * c4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long j = i / c4;
    const int q = (int)(i - j * c4);
    const long long r = rows[j];
    if (r >= 0 && r < n_dst) reinterpret_cast<float4*>(dst + r * ld)[q] = src[i];
  }
}
// dst[rows[j]] += src[j] (src: [cap, c4 float4], row pitch src_ld floats): the list holds a row at most once, so one
// thread owns an element of dst
__global__ void __launch_bounds__(256) k_scatter_add_rows(const float* __restrict__ src, int src_ld,
                                                          const int* __restrict__ rows, long long cap, int c4,
                                                          long long n_dst, float* __restrict__ dst, int ld) {
  const long long total = cap * c4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long j = i / c4;
    const int q = (int)(i - j * c4);
    const long long r = rows[j];
    if (r < 0 || r >= n_dst) continue;
    const float4 a = reinterpret_cast<const float4*>(src + j * src_ld)[q];
    float4* d = reinterpret_cast<float4*>(dst + r * ld) + q;
    float4 v = *d;
    v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
    *d = v;
  }
}
// slots[rows[j]] = j for the rows of the list inside [0, n); the caller has filled slots with -1
__global__ void __launch_bounds__(256) k_row_slots(const int* __restrict__ rows, long long cap, long long n,
                                                   int* __restrict__ slots) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= cap) return;
  const long long r = rows[j];
  if (r >= 0 && r < n) slots[r] = (int)j;
}
// k_scatter_rows for the output of a forward pass that ran the row normalisation on the rows of a list: the same move, and
// the rows of the compact tensors that belong to no row of dst (-1 padding, ids outside dst) are made inert in place --
// y[j] = 0, norm[j] = 1 -- whatever the normalisation left there (0 / 0 when the row in front of it is zero)
__global__ void __launch_bounds__(256) k_scatter_rows_inert(float4* __restrict__ y, float* __restrict__ norm,
                                                            const int* __restrict__ rows, long long cap, int c4,
                                                            long long n_dst, float* __restrict__ dst, int ld) {
  const long long total = cap * c4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long j = i / c4;
    const int q = (int)(i - j * c4);
    const long long r = rows[j];
    if (r >= 0 && r < n_dst) {
      reinterpret_cast<float4*>(dst + r * ld)[q] = y[i];
    } else {
      y[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q == 0) norm[j] = 1.f;
    }
  }
}
// touched-row list (gcl_touched_rows): flag[r] = 1 for every row an index array names; ids outside [0, n) are dropped
__global__ void __launch_bounds__(256) k_touch_rows(const long long* __restrict__ ids, long long count, long long n,
                                                    int* __restrict__ flag) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const long long r = ids[i];
  if (r >= 0 && r < n) flag[r] = 1;
}
// ... and for the members of the selected groups: one workgroup per selection, index[goff[g] .. goff[g + 1])
__global__ void __launch_bounds__(64) k_touch_groups(const long long* __restrict__ index, long long n_index,
                                                     const long long* __restrict__ goff, long long n_groups,
                                                     const long long* __restrict__ sel, long long n,
                                                     int* __restrict__ flag) {
  const long long g = sel[blockIdx.x];
  if (g < 0 || g >= n_groups) return;
  long long b = goff[g], e = goff[g + 1];
  if (b < 0) b = 0;
  if (e > n_index) e = n_index;
  for (long long j = b + threadIdx.x; j < e; j += 64) {
    const long long r = index[j];
    if (r >= 0 && r < n) flag[r] = 1;
  }
}
// pos = exclusive scan of flag: the flagged rows in ascending order, -1 behind them, the count (which may exceed cap: the
// list is then cut, and the caller's bound was wrong)
__global__ void __launch_bounds__(256) k_touch_emit(const int* __restrict__ flag, const int* __restrict__ pos, long long n,
                                                    int* __restrict__ rows, long long cap, int* __restrict__ n_touched) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int total = pos[n - 1] + flag[n - 1];
  if (i == 0) *n_touched = total;
  if (i < n && flag[i] && pos[i] < cap) rows[pos[i]] = (int)i;
  if (i < cap && i >= total) rows[i] = -1;
}
// identity pair list of a kernel_size-1 convolution: p[i] = i for i < n, -1 padding (CoordinateManager.identity_pairs)
__global__ void __launch_bounds__(256) k_identity_pairs(int* __restrict__ p, long long n, long long total) {
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < total) p[i] = i < n ? (int)i : -1;
}

// coords.hip (internal entry points shared by the two translation units)
void fill32(void* p, long long n_words, unsigned v, hipStream_t st);
void tables_fill(int64_t* tables, long long slots, int32_t* zero4, hipStream_t st);
int coords_insert_impl(const int32_t* coords, int64_t n, int64_t* table, int64_t cap, int32_t* status, bool table_ready,
                       void* stream);
int stride_map_impl(const int32_t* coords_in, int64_t n_in, const int32_t* n_in_dev, int32_t t_out, int64_t* table_out,
                    int64_t cap_out, int32_t* scratch, int32_t* coords_out, int32_t* n_out_dev, int32_t* status,
                    int64_t* index_out, bool table_ready, void* stream);

static inline unsigned grid_for(long long items, unsigned cap = 4096) {
  long long g = cdiv(items > 0 ? items : 1, 256);
  return (unsigned)(g > cap ? cap : g);
}

// ---------------------------------------------------------------------------------------------------
// arena
// ---------------------------------------------------------------------------------------------------
struct Arena {
  char* base;
  long long size, off;
  bool dry;          // size the pass only: no launch, pointers are never dereferenced
  void* take(long long bytes) {
    off = (off + 255) & ~255ll;
    char* p = base + off;
    off += bytes > 0 ? bytes : 0;
    return p;
  }
  template <typename T>
  T* take_n(long long count) { return (T*)take(count * (long long)sizeof(T)); }
  bool fits() const { return dry || off <= size; }
};

static char* const DRY_BASE = (char*)0x100000;    // dry runs hand out fake non-null addresses that are never dereferenced

static long long pow2_cap(long long n) {
  long long cap = 64;
  while (cap < 2 * n) cap *= 2;
  return cap;
}

#define PLAN_CALL(expr)          \
  do {                           \
    if (!A.dry) {                \
      int rc_ = (expr);          \
      if (rc_ != GCL_OK) return rc_; \
    }                            \
  } while (0)

// ---------------------------------------------------------------------------------------------------
// maps
// ---------------------------------------------------------------------------------------------------
static int level_of(int t) {
  int l = 0;
  while ((1 << l) < t) ++l;
  return ((1 << l) == t) ? l : -1;
}

static int maps_build(const int32_t* coords, long long n, const gcl_map_spec* specs, int n_specs, int n_levels, Arena& A,
                      int32_t* pinned, gcl_maps_desc* out, hipStream_t st, hipStream_t side = nullptr) {
  void* stream = (void*)st;
  memset(out, 0, sizeof(*out));
  out->n_levels = n_levels;
  out->n_maps = n_specs;
  // level 0: the input coordinates and their hash table (CoordinateManager.__init__)
  const long long cap0 = pow2_cap(n);
  out->coords[0] = (int32_t*)coords;
  out->n_rows[0] = n;
  out->cap[0] = cap0;
  // the hash tables of ALL levels side by side (same capacity each): one EMPTY fill for the lot
  int64_t* tables_all = A.take_n<int64_t>(cap0 * 2 * n_levels);
  for (int l = 0; l < n_levels; ++l) {
    out->table[l] = tables_all + (long long)l * cap0 * 2;
    out->cap[l] = cap0;
  }
  // status words, the levels' meta words and every map's counts in ONE block: one zero fill, one read-back copy
  const long long n_meta = 8 * (n_levels > 1 ? n_levels - 1 : 1);
  int32_t* status = A.take_n<int32_t>(4 + n_meta + 128ll * GCL_MAX_MAPS);
  if (!A.dry) tables_fill(tables_all, cap0 * n_levels, status, st);
  PLAN_CALL(coords_insert_impl(coords, n, out->table[0], cap0, status, true, stream));
  // levels 1 ..: one chain of launches, row counts stay on the device (CoordinateManager._build_stride_maps)
  // one zero fill for the levels' meta words AND every map's per-offset counts (gcl_kernel_map then counts by integer
  // atomics: no reduction launch per map)
  int32_t* meta = status + 4;
  int32_t* counts_all = meta + n_meta;
  if (!A.dry) GCL_CHECK_HIP(hipMemsetAsync(meta, 0, sizeof(int32_t) * (size_t)(n_meta + 128ll * GCL_MAX_MAPS), st));
  const int32_t* cb = coords;
  const int32_t* n_dev = nullptr;
  for (int l = 1; l < n_levels; ++l) {
    int32_t* scratch = A.take_n<int32_t>(gcl_scan_scratch_len(n));
    out->coords[l] = A.take_n<int32_t>(n * 4);
    // (the level's status words, meta + 8 (l - 1) + 4, are zero from the block's fill above)
    PLAN_CALL(stride_map_impl(cb, n, n_dev, 1 << l, out->table[l], cap0, scratch, out->coords[l], meta + 8 * (l - 1),
                              meta + 8 * (l - 1) + 4, nullptr, true, stream));
    cb = out->coords[l];
    n_dev = meta + 8 * (l - 1);
    out->n_rows[l] = n;        // upper bound until the read-back below
  }
  if (!A.dry) {     // the first of the two host syncs: input status + level sizes
    GCL_CHECK_HIP(hipMemcpyAsync(pinned, status, sizeof(int32_t) * (4 + (n_levels > 1 ? 8 * (n_levels - 1) : 0)),
                                 hipMemcpyDeviceToHost, st));
    GCL_CHECK_HIP(hipStreamSynchronize(st));
    for (int j = 0; j < 4; ++j) out->status[j] = pinned[j];
    GCL_CHECK_ARG(pinned[0] == 0, "%d coordinates outside the packable range (batch < 65535, |x|,|y|,|z| < 32768)", pinned[0]);
    GCL_CHECK_ARG(pinned[1] == 0, "%d duplicate coordinates: ME.SparseTensor expects unique rows (use ME.utils.sparse_quantize)",
                  pinned[1]);
    for (int l = 1; l < n_levels; ++l) {
      GCL_CHECK_ARG(pinned[4 + 8 * (l - 1) + 4] == 0, "%d strided coordinates outside the packable range",
                    pinned[4 + 8 * (l - 1) + 4]);
      out->n_rows[l] = pinned[4 + 8 * (l - 1)];
    }
  }
  // kernel maps (CoordinateManager.get_kernel_map), one presence bitmap per coordinate table
  int32_t* bitmap[2][GCL_MAX_LEVELS] = {{nullptr}, {nullptr}};      // [built on the side stream][level]
  bool any_pairs = false;      // pair lists wanted (training): their counts are read back; inference skips the D2H copies
  for (int s = 0; s < n_specs; ++s) any_pairs = any_pairs || (specs[s].pairs != 0 && specs[s].kernel_size > 1);
  // SPLIT build (gcl_maps_build_split, inference): once the level sizes are on the host nothing below waits for the host
  // again, so the maps of the input level alone (what the first layers of a network use) stay on `stream` and every other
  // map and its sorted tables go to `side` -- they are built BESIDE the first layers' convolutions, which the caller can
  // enqueue on `stream` straight away (gcl_maps_desc.late_mask / ready_event tell the plan where to wait).  The dry run
  // reserves for the split (one more presence bitmap per level).
  const bool split = (side != nullptr || A.dry) && !any_pairs;
  auto on_side = [&](const gcl_map_spec& sp) { return split && !(sp.t_in == 1 && sp.stride == 1); };
  // SMALL builds (<= 65 536 input rows, one stream): every neighbour table of the build is pre-filled with -1 by ONE launch
  // over the arena range that holds them (gcl_kernel_map flag bit 3) instead of a fill per map -- a pass over one pair of
  // clouds pays ~ 4.8 us of dispatch latency per dependent launch.  The launches are collected first, issued after the fill.
  struct MapLaunch { int s, src5, flags; int32_t *bitmap, *scratch; void* stream; };
  MapLaunch launches[GCL_MAX_MAPS];
  int n_launches = 0;
  const MapShape mshape = map_launch_shape(n, 1, 0);
  const bool prefill = !A.dry && !side && mshape.prefill;
  char* fill_lo = nullptr;
  for (int s = 0; s < n_specs; ++s) {
    const gcl_map_spec& sp = specs[s];
    gcl_map_desc& d = out->maps[s];
    d.t_in = sp.t_in;
    d.kernel_size = sp.kernel_size;
    d.stride = sp.stride;
    d.K = sp.kernel_size * sp.kernel_size * sp.kernel_size;
    d.level_in = level_of(sp.t_in);
    d.level_out = level_of(sp.t_in * sp.stride);
    GCL_CHECK_ARG(d.level_in >= 0 && d.level_out >= 0 && d.level_out < n_levels && (sp.stride == 1 || sp.stride == 2),
                  "gcl_maps_build: map %d (t_in %d, stride %d) is outside the %d levels built", s, sp.t_in, sp.stride, n_levels);
    GCL_CHECK_ARG(sp.kernel_size == 1 || sp.kernel_size == 3 || sp.kernel_size == 5, "gcl_maps_build: kernel size 1, 3 or 5");
    d.n_in = out->n_rows[d.level_in];
    d.n_out = out->n_rows[d.level_out];
    if (sp.kernel_size == 1) {
      GCL_CHECK_ARG(sp.stride == 1, "gcl_maps_build: kernel_size 1 with stride > 1");
      continue;      // identity pairs only, after the counts are known (nothing to count here)
    }
    const int sd = on_side(sp) ? 1 : 0;
    void* mstream = (sd && side) ? (void*)side : stream;
    if (sd) out->late_mask |= 1 << s;
    d.nbr = A.take_n<int32_t>((long long)d.K * d.n_out);
    if (!fill_lo) fill_lo = (char*)d.nbr;
    const bool same = sp.stride == 1;
    d.nbr_t = same ? nullptr : A.take_n<int32_t>((long long)d.K * d.n_in);
    d.counts = counts_all + 128 * s;
    // a 3^3 stride-1 map of a table whose 5^3 stride-1 map is already built: 27 of its rows
    int src5 = -1;
    for (int q = 0; q < s && same && sp.kernel_size == 3; ++q)
      if (specs[q].t_in == sp.t_in && specs[q].kernel_size == 5 && specs[q].stride == 1 && out->maps[q].nbr) src5 = q;
    if (src5 >= 0) {
      launches[n_launches++] = MapLaunch{s, src5, 0, nullptr, nullptr, mstream};
      continue;
    }
    // the presence bitmap (2 MB) pays when the table is much larger than it; a table of <= 8 MB (<= 256 k slots: a pass over
    // a few clouds) sits in the caches itself and the bitmap's fill + build are two launches per level for nothing
    const bool use_bitmap = A.dry || mshape.use_bitmap;      // (every level's table has the input level's capacity)
    const bool bitmap_valid = use_bitmap && bitmap[sd][d.level_in] != nullptr;     // shared by the maps of ONE stream only
    if (use_bitmap && !bitmap_valid) bitmap[sd][d.level_in] = A.take_n<int32_t>(gcl_kernel_map_bitmap_len());
    int32_t* scratch = A.take_n<int32_t>(gcl_kernel_map_scratch_len(sp.kernel_size, d.n_out));
    launches[n_launches++] = MapLaunch{s, -1, (same ? 1 : 0) | (bitmap_valid ? 2 : 0) | 4 | (prefill ? 8 : 0),
                                       use_bitmap ? bitmap[sd][d.level_in] : nullptr, scratch, mstream};
  }
  if (prefill && fill_lo) fill32(fill_lo, (long long)((A.base + A.off) - fill_lo) / 4, 0xFFFFFFFFu, st);
  for (int q = 0; q < n_launches; ++q) {
    const MapLaunch& L = launches[q];
    const gcl_map_spec& sp = specs[L.s];
    gcl_map_desc& d = out->maps[L.s];
    if (L.src5 >= 0)
      PLAN_CALL(gcl_kernel_map_3_from_5(out->maps[L.src5].nbr, out->maps[L.src5].counts, d.n_out, d.nbr, d.counts, L.stream));
    else
      PLAN_CALL(gcl_kernel_map(out->coords[d.level_out], d.n_out, out->table[d.level_in], out->cap[d.level_in],
                               sp.kernel_size, sp.t_in, L.flags, L.bitmap, L.scratch, d.nbr, d.nbr_t, d.n_in, d.counts, L.stream));
    if (!A.dry && any_pairs)   // without pair lists nobody waits for this copy: it would outlive the call (pinned re-use)
      GCL_CHECK_HIP(hipMemcpyAsync(pinned + 128 * (L.s + 1), d.counts, sizeof(int32_t) * d.K, hipMemcpyDeviceToHost, st));
  }
  // mask-sorted tables (KernelMap.sorted_table) of all maps in ONE gcl_table_sort_multi sequence (14 launches instead of
  // 14 per table; same results); K > 27 tables are used as they are
  gcl_sort_job jobs[2][2 * GCL_MAX_MAPS];      // [on the side stream][job]
  int n_jobs[2] = {0, 0};
  for (int s = 0; s < n_specs; ++s) {
    const gcl_map_spec& sp = specs[s];
    gcl_map_desc& d = out->maps[s];
    if (sp.kernel_size == 1) continue;
    for (int tr = 0; tr < 2; ++tr) {
      if (!(sp.tables & (1 << tr))) continue;
      const int32_t* tbl = tr ? d.nbr_t : d.nbr;
      GCL_CHECK_ARG(tbl, "gcl_maps_build: map %d has no transposed table (stride 1)", s);
      const long long rows = tr ? d.n_in : d.n_out;
      GCL_CHECK_ARG(d.K == 27, "gcl_maps_build: sorted tables are built for 3^3 kernels");
      int32_t* scratch = A.take_n<int32_t>(gcl_table_sort_scratch_len(rows));
      int32_t* order = A.take_n<int32_t>(rows);
      int32_t* sorted = A.take_n<int32_t>((long long)d.K * rows);
      int32_t* mask = A.take_n<int32_t>(cdiv(rows, 32));
      const int sd = on_side(sp) ? 1 : 0;
      jobs[sd][n_jobs[sd]++] = gcl_sort_job{tbl, d.K, rows, scratch, order, sorted, mask, d.counts};
      if (tr) { d.tbl_t = sorted; d.order_t = order; d.mask_t = mask; }
      else { d.tbl_n = sorted; d.order_n = order; d.mask_n = mask; }
    }
  }
  for (int s = 0; s < n_specs; ++s) {      // presence words of the first layer's table (occupancy path of the stem kernels)
    if (!(specs[s].tables & 4) || specs[s].kernel_size == 1) continue;
    gcl_map_desc& d = out->maps[s];
    d.presence = A.take_n<uint32_t>(d.n_out * ((d.K + 31) / 32));
    PLAN_CALL(gcl_presence_bits(d.nbr, d.K, d.n_out, d.presence, (on_side(specs[s]) && side) ? (void*)side : stream));
  }
  for (int sd = 0; sd < 2; ++sd) {      // the main stream's tables first: the first layers wait for them
    void* sstream = (sd && side) ? (void*)side : stream;
    if (n_jobs[sd]) PLAN_CALL(gcl_table_sort_multi(jobs[sd], n_jobs[sd], sstream));
  }
  if (!side) out->late_mask = 0;       // (dry run / one stream: nothing is late)
  // the second host sync: per-offset pair counts -> padded segment offsets -> pair lists (KernelMap.pairs); skipped when
  // no map asks for pair lists (inference): counts_host / n_pairs / seg_off then stay zero
  if (!A.dry && any_pairs) GCL_CHECK_HIP(hipStreamSynchronize(st));
  for (int s = 0; s < n_specs; ++s) {
    const gcl_map_spec& sp = specs[s];
    gcl_map_desc& d = out->maps[s];
    if (sp.kernel_size == 1) {
      if (!sp.pairs) continue;
      const long long total = cdiv(d.n_in, GCL_PAIR_CHUNK) * GCL_PAIR_CHUNK;
      d.pair_in = d.pair_out = A.take_n<int32_t>(total);
      d.seg_off[0] = 0;
      d.seg_off[1] = total;
      d.n_pairs = d.n_in;
      d.counts_host[0] = (int32_t)d.n_in;
      if (!A.dry) {
        hipLaunchKernelGGL(k_identity_pairs, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, st, d.pair_in, (long long)d.n_in,
                           total);
        GCL_CHECK_LAUNCH();
      }
      continue;
    }
    if (!any_pairs && !A.dry) continue;
    long long total = 0;
    d.seg_off[0] = 0;
    for (int k = 0; k < d.K; ++k) {
      // dry run: every output row could own every offset
      const long long c = A.dry ? d.n_out : (long long)pinned[128 * (s + 1) + k];
      d.counts_host[k] = (int32_t)c;
      d.n_pairs += c;
      total += cdiv(c, GCL_PAIR_CHUNK) * GCL_PAIR_CHUNK;
      d.seg_off[k + 1] = total;
    }
    if (!sp.pairs) continue;
    const long long len = total > 0 ? total : 1;
    int32_t* both = A.take_n<int32_t>(2 * len);
    d.pair_in = both;
    d.pair_out = both + len;
    int32_t* scratch = A.take_n<int32_t>((long long)d.K * cdiv(d.n_out, 1024) + d.K + 1);
    PLAN_CALL(gcl_kernel_map_pairs(d.nbr, d.K, d.n_out, d.seg_off, scratch, d.pair_in, d.pair_out, stream));
    // cell limits of the weight gradient's range-grouped launches: a function of the map, made here once (side stream)
    // instead of by every convolution that uses the map (k_pair_bounds: 9 launches per step on the weight-gradient stream)
    // (dry run: n_out is an upper bound of the level's rows and gcl_conv_bwd_weight_bounds_len is not monotone in the row
    // count -- the range length doubles as the level grows -- so the bound reserves for the SHORTEST range, 512 rows)
    const long long nb = !A.dry ? gcl_conv_bwd_weight_bounds_len(d.K, d.n_out)
                                : (d.n_out >= 32768 && d.K > 1 && d.K <= 27 ? (long long)d.K * (cdiv(d.n_out, 512) + 1) : 0);
    if (nb > 0 && total > 0) {
      d.dw_bounds = A.take_n<int32_t>(nb);
      PLAN_CALL(gcl_conv_bwd_weight_bounds(d.pair_out, d.seg_off, d.K, d.n_out, d.dw_bounds, stream));
    }
  }
  out->arena_used = A.off;
  if (!A.fits()) {
    set_error("gcl_maps_build: arena too small (%lld bytes needed, %lld given)", A.off, A.size);
    return GCL_ERR_ARENA;
  }
  return GCL_OK;
}

// ---------------------------------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------------------------------
struct RowView;
struct TState {            // a tensor of the pass (forward value or gradient)
  float* ptr = nullptr;
  RowView* rv = nullptr;     // a gradient kept compact: ptr is [rv->cap, c] (row pitch ld), the rows rv->rows of a tensor that
                             // is exactly zero in every other row (the backward pass of a plan_backward call with a list)
  int32_t* amax = nullptr;   // amax slot that holds max|tensor|, or NULL = not measured yet
  void* planes = nullptr;    // gcl_split_planes image, or NULL = not made yet
  int ld = 0;                // row pitch in floats when the tensor is a column slice of a wider one (gradients of ME.cat
                             // inputs: slices of the gradient of the cat's output), 0 = its own channel count
  bool plane_only = false;   // ptr is NULL on purpose: every reader takes `planes` (analyse_graph), no fp32 form exists
};

// in front of every launch that reads the fp32 form of a tensor: a reader the analysis overlooked ends here, on the host
#define NEED_F32(ts, rec, what)                                                                                          \
  GCL_CHECK_ARG(!(ts).plane_only, "gcl_plan: record %d reads %s in fp32, but the plan keeps that tensor as a plane image " \
                                  "only (reader analysis of gcl_plan_create)", (int)(rec), what)

struct OpSaved {           // what the backward pass of a record needs from its forward pass
  float* conv_out = nullptr;            // CONVBN: the convolution output (the BatchNorm input)
  unsigned long long* mask = nullptr;   // CONVBN with relu: sign bits of the output
  float *mean = nullptr, *rstd = nullptr;
  float* xrange = nullptr;              // CONVBN in bound mode: per-channel minimum / maximum of conv_out ([2][c])
  int32_t* x_amax = nullptr;
  float* norm = nullptr;                // ROWNORM
};

struct ProfRec {
  hipEvent_t e0, e1;
  double kind, pairs, cin, cout, n_in, n_out, K;
};

struct PassState {        // everything one forward pass leaves behind for its backward pass
  const gcl_maps_desc* maps = nullptr;
  gcl_maps_desc maps_copy;
  std::vector<TState> t, g;
  std::vector<OpSaved> saved;
  std::vector<void*> params;
  Arena A{DRY_BASE, 0, 0, true};
  int32_t* slot_pool = nullptr;
  long long n_slots = 0, next_slot = 0;
  bool slots_exhausted = false;
  int32_t* w_amax = nullptr;        // [n_weights][GCL_AMAX_WORDS]
  unsigned char *pack_fwd = nullptr, *pack_bwd = nullptr;
  void* state = nullptr;
  bool forward_done = false, bwd_packed = false;
  std::vector<char> relu_masked;    // backward pass: RELU record whose backward the consumer's epilogue has already applied
  hipEvent_t fwd_packs = nullptr;      // recorded on the aux stream behind the forward packs of the pass
  bool fwd_packs_pending = false;
  int32_t* not_ones = nullptr;      // per input row of the pass: its cloud has a feature that differs from 1.0f (table path)
  void* key = nullptr;              // the pass's arena: how gcl_plan_backward / gcl_plan_release find it
  // forward pass that ran the touched-row suffix on the rows of a list (fwd_cap > 0): the list, parked with the pass.  The
  // tensors of the suffix -- its input included -- and its saved operands are then compact [fwd_cap, c] tensors
  const int32_t* fwd_rows = nullptr;
  long long fwd_cap = 0;
  bool keep_twins = false;          // Plan::keep_fp32 as it stood when the pass was sized: both passes of one arena agree
};

struct Readers {      // who reads a tensor, by record: found once, what every analysis of the record graph asks
  int maker = -1;             // the record that makes it (-1: the plan's input)
  std::vector<int> x, x2;     // the records that read it as x / as x2, ascending; a record that reads it as both is in both
  bool output = false;        // the last record's output: the caller reads it
  int count() const { return (int)(x.size() + x2.size()); }      // (a record that reads it twice counts twice)
  bool only(int rec) const {      // nobody but record rec reads it
    return !output && std::count(x.begin(), x.end(), rec) + std::count(x2.begin(), x2.end(), rec) == count();
  }
};

struct Plan : PassState {   // the base part is the pass being enqueued right now
  std::vector<PassState*> passes;   // passes waiting for their backward pass (several forwards may be outstanding)
  std::vector<gcl_plan_op> ops;
  int n_tensors = 0, n_params = 0, n_bn = 0, presplit = 128;
  std::vector<int> worder;          // parameter ids of the MFMA-shaped kernels (amax slot / pack order)
  std::vector<int> widx;            // parameter id -> position in worder, -1 otherwise
  std::vector<int> wmode;           // per position: input-gradient pack mode (1 | 2), 0 = no input gradient needed
  std::vector<long long> wK, wcin, wcout, off_fwd, off_bwd;
  long long bytes_fwd = 0, bytes_bwd = 0, wgs_fwd = 0, wgs_bwd = 0;
  int n_bwd = 0;
  std::vector<char> made;           // tensor id -> produced by a record of the plan
  std::vector<Readers> readers;     // tensor id -> who makes and who reads it (analyse_graph)
  std::vector<char> fuse_relu;      // record i is a CONV whose only consumer is the RELU record i + 1: one launch writes relu(y)
  std::vector<int> cat_left;        // record i is a CONVBN whose output is only the LEFT input of CAT record cat_left[i]: its
                                    // BatchNorm apply pass writes into the cat's output (row pitch = the cat's width)
  std::vector<int> mask_from;       // record i is a convolution whose input is the output of RELU record mask_from[i] and that
                                    // ReLU's only consumer: its input-gradient epilogue applies the ReLU's backward (-1: no)
  // plane-only tensors (analyse_graph): record i is a CONVBN in bound mode whose output y (po_fwd) / whose BatchNorm
  // input gradient dx (po_bwd) every reader takes as a plane image -- the apply pass writes no fp32 twin and the arena holds
  // none.  keep_fp32 (gcl_plan_set_keep_fp32, tests): every twin is written, as if both vectors were all zero
  std::vector<char> po_fwd, po_bwd;
  bool keep_fp32 = false;
  // device tables (inside the caller's `state` buffer), re-uploaded when a parameter pointer changes
  std::vector<long long> host_tables, uploaded;
  // optional second stream for the weight gradients (off the critical path of the backward pass)
  hipStream_t aux = nullptr;
  std::vector<hipEvent_t> events;
  size_t events_used = 0;
  bool aux_dirty = false;
  // touched-row suffix: the records [suffix_first, ops.size()) are row-local (ROWNORM, RELU, kernel_size-1 CONV), form one
  // chain, and nothing but the chain reads its input (ops.size(): no such suffix).  A caller that knows which rows of dy can
  // be non-zero hands them over for ONE backward pass (gcl_plan_set_touched_rows), which then runs these records on those
  // rows only (suffix_backward)
  int suffix_first = 0;
  bool suffix_rows_ok = false;      // every CONV of the suffix has a shape gcl_conv_bwd_weight_rows takes
  const int32_t* touched = nullptr;
  long long touched_cap = 0;
  long long suffix_rows_used = 0;   // rows the suffix of the latest backward pass ran on (0: all of them, the dense records)
  long long suffix_fwd_rows_used = 0;   // ... of the latest training-mode forward pass
  // profiling
  bool profile = false;
  std::vector<ProfRec> prof;
  size_t prof_used = 0;
};

static long long state_words(const Plan& P) { return (long long)P.worder.size() * (2 + 8 + 8); }

static int32_t* new_slot(Plan& P) {      // slots are used once per pass (they start zeroed); the pool is sized for the worst case
  if (P.next_slot >= P.n_slots) {
    P.slots_exhausted = true;
    return P.slot_pool;
  }
  return P.slot_pool + (P.next_slot++) * GCL_AMAX_WORDS;
}

// rec: the record on whose behalf the tensor is measured / split (error texts)
static int ensure_amax(Plan& P, TState& ts, long long numel, hipStream_t st, int rec) {
  Arena& A = P.A;
  if (ts.amax) return GCL_OK;
  NEED_F32(ts, rec, "a tensor whose max-abs slot is missing");
  ts.amax = new_slot(P);
  PLAN_CALL(gcl_amax(ts.ptr, numel, ts.amax, 1, (void*)st));
  return GCL_OK;
}

static int ensure_planes(Plan& P, TState& ts, long long n, int c, hipStream_t st, int rec) {
  Arena& A = P.A;
  if (ts.planes) return GCL_OK;
  NEED_F32(ts, rec, "a tensor whose plane image is missing");
  ts.planes = A.take(n * c * 4);
  PLAN_CALL(gcl_split_planes(ts.ptr, n, c, ts.amax, ts.planes, (void*)st));
  return GCL_OK;
}

// The weight gradient of a record is needed only by the optimizer: with an aux stream it is enqueued there, ordered
// behind everything the main stream has issued so far (its operands), and the main stream goes on with the input-gradient
// chain.  join_aux makes the main stream wait for all of it (end of a backward segment).
// fork / join events are re-used pass after pass (recording re-arms them): the next one, created when the pool is used up
static hipError_t next_event(Plan& P, hipEvent_t* e) {
  if (P.events_used == P.events.size()) {
    hipEvent_t fresh;
    const hipError_t err = hipEventCreateWithFlags(&fresh, hipEventDisableTiming);
    if (err != hipSuccess) return err;
    P.events.push_back(fresh);
  }
  *e = P.events[P.events_used++];
  return hipSuccess;
}

static hipStream_t fork_aux(Plan& P, hipStream_t st) {
  if (!P.aux || P.A.dry) return st;
  hipEvent_t e;
  if (next_event(P, &e) != hipSuccess || hipEventRecord(e, st) != hipSuccess || hipStreamWaitEvent(P.aux, e, 0) != hipSuccess)
    return st;
  P.aux_dirty = true;
  return P.aux;
}

static int join_aux(Plan& P, hipStream_t st) {
  if (!P.aux || !P.aux_dirty || P.A.dry) return GCL_OK;
  hipEvent_t e;
  GCL_CHECK_HIP(next_event(P, &e));
  GCL_CHECK_HIP(hipEventRecord(e, P.aux));
  GCL_CHECK_HIP(hipStreamWaitEvent(st, e, 0));
  P.aux_dirty = false;
  return GCL_OK;
}

struct ProfScope {      // brackets one launch with events when profiling is armed
  Plan& P;
  hipStream_t st;
  ProfRec* r = nullptr;
  ProfScope(Plan& P_, hipStream_t st_, int kind, double pairs, int cin, int cout, long long n_in, long long n_out, int K)
      : P(P_), st(st_) {
    if (!P.profile || P.A.dry) return;
    if (P.prof_used == P.prof.size()) {
      ProfRec nr{};
      if (hipEventCreate(&nr.e0) != hipSuccess || hipEventCreate(&nr.e1) != hipSuccess) return;
      P.prof.push_back(nr);
    }
    r = &P.prof[P.prof_used++];
    r->kind = kind; r->pairs = pairs; r->cin = cin; r->cout = cout; r->n_in = (double)n_in; r->n_out = (double)n_out; r->K = K;
    (void)hipEventRecord(r->e0, st);
  }
  ~ProfScope() { if (r) (void)hipEventRecord(r->e1, st); }
};

// The Cin <= 4 first layer, convolved by the VALU stem kernels on the fp32 weights.  Decided from the record alone, so the
// constructor, the reader analysis and both passes agree: K > 1 stands for the map's kernel_size > 1, because check_maps pins
// m.K == op.K for the maps of every pass and a map's K is kernel_size^3.
static bool is_conv(const gcl_plan_op& op) { return op.kind == GCL_OP_CONVBN || op.kind == GCL_OP_CONV; }
static bool stem_shape(const gcl_plan_op& op) {
  return op.cin <= 4 && (op.cout % 32) == 0 && !op.transpose && op.K > 1 && op.bias < 0;
}

// the first layer's convolution into the caller's [n_out, cout] block.  Its occupancy rows are measured once per pass, per cloud
// (the reference's training loaders jitter the centre cloud of a sample only), spread to rows: device flags, no host decision
static int stem_forward(Plan& P, int i, long long n_in, long long n_out, float* y, hipStream_t st) {
  Arena& A = P.A;
  const gcl_plan_op& op = P.ops[i];
  const gcl_map_desc& m = P.maps->maps[op.map];
  const TState& x = P.t[op.x];
  NEED_F32(x, i, "its input (first layer)");
  if (m.presence && !P.not_ones) {
    constexpr int CLOUD_FLAGS = 4096;      // batch indices beyond this take the table path
    int32_t* cloud = A.take_n<int32_t>(CLOUD_FLAGS);
    P.not_ones = A.take_n<int32_t>(n_in);
    PLAN_CALL(gcl_not_ones_rows(x.ptr, op.cin, P.maps->coords[op.level_in], n_in, cloud, CLOUD_FLAGS, P.not_ones, (void*)st));
  }
  PLAN_CALL(gcl_stem_fwd(x.ptr, (const float*)P.params[op.w], m.nbr, n_out, op.K, op.cin, op.cout, y, m.presence,
                         m.presence ? P.not_ones : nullptr, (void*)st));
  return GCL_OK;
}

// the mask-sorted table of a map a launch walks: over the map's output rows, or (transposed) over its input rows; a
// kernel_size-1 map has none
struct SortedTable {
  const int32_t *tbl = nullptr, *order = nullptr, *mask = nullptr;
};
static SortedTable sorted_table(const gcl_map_desc& m, bool transposed) {
  if (m.kernel_size == 1) return SortedTable();
  return transposed ? SortedTable{m.tbl_t, m.order_t, m.mask_t} : SortedTable{m.tbl_n, m.order_n, m.mask_n};
}

// The fp16x3 launch of a CONVBN / CONV record off the first layer, in training and in inference alike: conv_prepare makes
// what it reads besides x (the packs, max|x|, the map's sorted table; `who`: the entry, for the error text) ...
static int conv_prepare(Plan& P, int i, long long n_in, const char* who, hipStream_t st) {
  const gcl_plan_op& op = P.ops[i];
  const gcl_map_desc& m = P.maps->maps[op.map];
  if (P.fwd_packs_pending && !P.A.dry) {      // first convolution that reads the packs forward_setup made on the aux stream
    GCL_CHECK_HIP(hipStreamWaitEvent(st, P.fwd_packs, 0));
    P.fwd_packs_pending = false;
  }
  GCL_CHECK_ARG(P.A.dry || m.kernel_size == 1 || sorted_table(m, op.transpose).tbl,
                "%s: record %d needs a sorted table the maps do not carry", who, i);
  return ensure_amax(P, P.t[op.x], n_in * op.cin, st, i);
}
// ... and conv_launch issues it with the operands of the caller's mode (gcl_conv_fwd_fused's, `stats` as the flags define it)
static int conv_launch(Plan& P, int i, bool planes, long long n_in, long long n_out, const float* bias, const float* col_scale,
                       const float* residual, int relu, int32_t* y_amax, float* y, float* stats, int flags, hipStream_t st) {
  Arena& A = P.A;
  const gcl_plan_op& op = P.ops[i];
  const gcl_map_desc& m = P.maps->maps[op.map];
  const TState& x = P.t[op.x];
  const SortedTable T = sorted_table(m, op.transpose);
  const int wi = P.widx[op.w];
  if (!planes) NEED_F32(x, i, "its input");
  ProfScope ps(P, st, 0, (double)(m.kernel_size > 1 ? m.n_pairs : n_out), op.cin, op.cout, n_in, n_out, op.K);
  PLAN_CALL(gcl_conv_fwd_fused(planes ? (const float*)x.planes : x.ptr, n_in, planes ? 1 : 0, P.pack_fwd + P.off_fwd[wi], 4, x.amax,
                               P.w_amax + (long long)wi * GCL_AMAX_WORDS, T.tbl, T.order, T.mask, n_out, op.K, op.cin, op.cout,
                               bias, col_scale, residual, relu, y_amax, y, stats, flags, (void*)st));
  return GCL_OK;
}

// The convolution of a CONVBN / CONV record in a training pass (ops._SparseConvFn.forward), which is all of a CONV record
// rows > 0: a kernel_size-1 record of the touched-row suffix whose input is a compact [rows, cin] tensor
struct ConvOut {
  int rc;
  float* y;         // [n_out, cout]
  float* stats;     // CONVBN off the first layer: sum, squares, min, max per column and 128-row tile
};
static ConvOut conv_forward(Plan& P, int i, hipStream_t st, long long rows = 0) {
  Arena& A = P.A;
  const gcl_plan_op& op = P.ops[i];
  const long long n_in = rows > 0 ? rows : P.maps->n_rows[op.level_in], n_out = rows > 0 ? rows : P.maps->n_rows[op.level_out];
  TState& x = P.t[op.x];
  ConvOut out{GCL_OK, A.take_n<float>(n_out * op.cout), nullptr};
  if (op.kind == GCL_OP_CONV) P.t[op.y].ptr = out.y;
  if (stem_shape(op)) {
    out.rc = stem_forward(P, i, n_in, n_out, out.y, st);
    return out;
  }
  if ((out.rc = conv_prepare(P, i, n_in, "gcl_plan_forward", st))) return out;
  P.saved[i].x_amax = x.amax;
  const bool planes = op.cin >= P.presplit;
  if (planes && (out.rc = ensure_planes(P, x, n_in, op.cin, st, i))) return out;
  if (op.kind == GCL_OP_CONVBN) out.stats = A.take_n<float>(cdiv(n_out, 128) * 4 * op.cout);
  int32_t* relu_amax = nullptr;
  if (op.kind == GCL_OP_CONV && P.fuse_relu[i]) {      // the epilogue applies the ReLU record that follows: both tensor ids name relu(conv(x))
    relu_amax = P.t[op.y].amax = new_slot(P);
    P.t[P.ops[i + 1].y] = P.t[op.y];
  }
  out.rc = conv_launch(P, i, planes, n_in, n_out, op.bias >= 0 ? (const float*)P.params[op.bias] : nullptr, nullptr, nullptr,
                       relu_amax ? 1 : 0, relu_amax, out.y, out.stats, 0, st);
  return out;
}

static int upload_tables(Plan& P, hipStream_t st) {
  // [ptrs n | sizes n | fwd desc n x 8 | bwd desc n_bwd x 8]  (WeightAmaxGroup.refresh / .packed)
  const size_t n = P.worder.size();
  std::vector<long long>& h = P.host_tables;
  h.assign((size_t)state_words(P), 0);
  P.wgs_fwd = P.wgs_bwd = 0;
  size_t row = 0;      // of the input-gradient descriptors: one per kernel that needs an input gradient
  auto desc = [&](long long* d, size_t q, long long mode, long long off, long long& wgs) {
    d[0] = h[q]; d[1] = P.wK[q]; d[2] = P.wcin[q]; d[3] = P.wcout[q]; d[4] = mode; d[5] = (long long)q; d[6] = off; d[7] = wgs;
    wgs += cdiv(h[n + q], 256);
  };
  for (size_t q = 0; q < n; ++q) {
    h[q] = (long long)(uintptr_t)P.params[P.worder[q]];
    h[n + q] = P.wK[q] * P.wcin[q] * P.wcout[q];
    desc(&h[2 * n + 8 * q], q, 0, P.off_fwd[q], P.wgs_fwd);
    if (P.wmode[q]) desc(&h[2 * n + 8 * n + 8 * row++], q, P.wmode[q], P.off_bwd[q], P.wgs_bwd);
  }
  if (h != P.uploaded) {      // parameters were (re-)seated: rare; the copy is finished before the vector can change
    GCL_CHECK_HIP(hipMemcpyAsync(P.state, h.data(), h.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    GCL_CHECK_HIP(hipStreamSynchronize(st));
    P.uploaded = h;
  }
  return GCL_OK;
}

// The compact [cap, c] result of the touched-row suffix as a dense tensor: *out = a zero-filled [n, c] tensor that holds
// src[j] in row rows[j].  norm (the forward pass behind a row normalisation): src and norm are the saved y and norm, whose
// rows that belong to no row of the output are made inert on the way (k_scatter_rows_inert)
static int spread_rows(Plan& P, float* src, float* norm, const int32_t* rows, long long cap, int c, long long n, float** out,
                       hipStream_t st) {
  Arena& A = P.A;
  float* dst = A.take_n<float>(n * c);
  *out = dst;
  if (A.dry) return GCL_OK;
  GCL_CHECK_HIP(hipMemsetAsync(dst, 0, (size_t)(n * c) * sizeof(float), st));
  if (!norm) return gcl_scatter_rows(src, rows, cap, c, n, dst, c, (void*)st);
  hipLaunchKernelGGL(k_scatter_rows_inert, dim3(grid_for(cap * c / 4)), dim3(256), 0, st, (float4*)src, norm, (const int*)rows,
                     cap, c / 4, n, dst, c);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

struct FwdArgs {      // what a forward pass is given.  Its mode is stated here, once, and kept nowhere in the plan
  const float* x;
  bool eval;            // inference (gcl_plan_forward_eval): BatchNorm in eval mode folded into the convolution epilogue
  void* const* bn;      // per BatchNorm -- training: running mean, variance; inference: scale, shift, mean, rstd (NULL: sizing)
  bool repack;          // inference: max|W| and the packed kernels, which persist in the state buffer, are made again
};

// Head of a forward pass: the state of the pass reset, its amax slot pool, max|W| and the packed kernels
static int forward_setup(Plan& P, const FwdArgs& a, hipStream_t st) {
  Arena& A = P.A;
  const size_t nw = P.worder.size();
  P.t.assign(P.n_tensors, TState());
  P.g.assign(P.n_tensors, TState());
  P.saved.assign(P.ops.size(), OpSaved());
  if (P.profile && !A.dry) P.prof_used = 0;      // records of a profiled pass stay readable until the next profiled pass
  if (!A.dry) P.events_used = 0;
  // amax slots of the pass: one zero fill (ops.amax_slot hands out slots of a zero-filled pool)
  P.n_slots = 4 * (long long)P.n_tensors + 2 * (long long)P.ops.size() + 16;
  P.next_slot = 0;
  P.slots_exhausted = false;
  P.not_ones = nullptr;
  P.fwd_packs_pending = false;
  P.slot_pool = A.take_n<int32_t>(P.n_slots * GCL_AMAX_WORDS);
  if (!A.dry) GCL_CHECK_HIP(hipMemsetAsync(P.slot_pool, 0, (size_t)P.n_slots * GCL_AMAX_WORDS * sizeof(int32_t), st));
  // all convolution kernels: max|W| in one launch, forward packs in one launch (WeightAmaxGroup)
  if (a.eval) {      // inference: max|W| and the packed kernels persist in the caller's state buffer from pass to pass
    char* base = (char*)P.state + ((state_words(P) * 8 + 255) & ~255ll);
    P.w_amax = (int32_t*)base;
    P.pack_fwd = (unsigned char*)(base + (((long long)nw * GCL_AMAX_WORDS * 4 + 255) & ~255ll));
  } else {
    P.w_amax = A.take_n<int32_t>((long long)nw * GCL_AMAX_WORDS);
    P.pack_fwd = (unsigned char*)A.take(P.bytes_fwd);
  }
  P.bwd_packed = false;
  const bool on_aux = !a.eval && P.aux && P.n_bwd;      // training with an aux stream: the packs are made there
  const long long* tab = (const long long*)P.state;
  if (nw && !A.dry) {
    int rc = upload_tables(P, st);
    if (rc) return rc;
    if (!a.eval || a.repack) {
      // on the aux stream max|W| and the forward packs are made beside the first layer (whose kernels read the fp32
      // weights); the main stream waits for them in front of its first packed convolution (conv_prepare)
      hipStream_t ps = on_aux ? fork_aux(P, st) : st;
      PLAN_CALL(gcl_amax_multi((const float* const*)tab, (const int64_t*)(tab + nw), (int32_t)nw, P.w_amax, (void*)ps));
      PLAN_CALL(gcl_pack_weights_multi((const int64_t*)(tab + 2 * nw), (int32_t)nw, P.wgs_fwd, 4, P.w_amax, P.pack_fwd, (void*)ps));
      if (ps != st) {
        GCL_CHECK_HIP(next_event(P, &P.fwd_packs));
        GCL_CHECK_HIP(hipEventRecord(P.fwd_packs, ps));
        P.fwd_packs_pending = true;
      }
    }
  }
  // ... and so are the input-gradient packs (needed by the first record of the backward pass): now, beside the forward
  // convolutions, instead of at the head of the backward pass
  if (on_aux) {
    P.pack_bwd = (unsigned char*)A.take(P.bytes_bwd);
    if (!A.dry) {
      hipStream_t ws = fork_aux(P, st);
      PLAN_CALL(gcl_pack_weights_multi((const int64_t*)(tab + 2 * nw + 8 * nw), P.n_bwd, P.wgs_bwd, 4, P.w_amax, P.pack_bwd,
                                       (void*)ws));
    }
    P.bwd_packed = true;
  }
  P.t[0].ptr = (float*)a.x;
  return GCL_OK;
}

// ME.conv_bn in a training pass (ops._SparseConvFn, ops._BatchNormFn): convolution, batch statistics, apply pass
static int convbn_forward(Plan& P, int i, const gcl_plan_op& op, long long n_out, void* const* bn_stats, hipStream_t st) {
  Arena& A = P.A;
  const ConvOut conv = conv_forward(P, i, st);
  if (conv.rc) return conv.rc;
  OpSaved& sv = P.saved[i];
  sv.conv_out = conv.y;
  const int c = op.cout;
  sv.mean = A.take_n<float>(2 * c);
  sv.rstd = sv.mean + c;
  float* rm = (float*)bn_stats[2 * op.bn];
  float* rv = (float*)bn_stats[2 * op.bn + 1];
  // y that is only the left input of an ME.cat is written straight into the cat's output (row pitch = its width); the cat
  // record then copies the other input's columns only
  const gcl_plan_op* cat = P.cat_left[i] >= 0 ? &P.ops[P.cat_left[i]] : nullptr;
  // Bound mode (round 5): this BatchNorm's output is at least `presplit` channels wide, i.e. its consumers read a
  // plane image: the statistics launch bounds max|y| from the epilogue's column ranges and the apply pass writes the
  // image itself -- into the image of the ME.cat it writes in place, if so (no gcl_split_planes pass; ops.py mirrors the
  // slot values: _BatchNormFn, cat_features).  Needs the residual's / the cat partner's max-abs slots, which their
  // producers have published.
  const int32_t* res_amax = op.x2 >= 0 ? P.t[op.x2].amax : nullptr;
  const int32_t* cat_amax = cat ? P.t[cat->x2].amax : nullptr;
  const bool bound = conv.stats && c >= P.presplit && (c % 32) == 0 && (op.x2 < 0 || res_amax) &&
                     (!cat || (cat_amax && (cat->cout % 32) == 0));
  int32_t* bound_slot = bound ? new_slot(P) : nullptr;
  if (conv.stats) {       // column sums (and ranges) from the convolution epilogue
    if (bound) sv.xrange = A.take_n<float>(2 * c);
    PLAN_CALL(gcl_bn_stats_from_tiles_range(conv.stats, cdiv(n_out, 128), n_out, c, op.eps, op.momentum, rm, rv, sv.mean, sv.rstd,
                                            sv.xrange, (const float*)P.params[op.bn_w], (const float*)P.params[op.bn_b], op.relu,
                                            res_amax, cat_amax, bound_slot, (void*)st));
  } else {
    double* scratch = A.take_n<double>(gcl_bn_scratch_len(n_out, c));
    PLAN_CALL(gcl_bn_stats(conv.y, n_out, c, op.eps, op.momentum, rm, rv, scratch, sv.mean, sv.rstd, (void*)st));
  }
  // the tensor the apply pass writes: y, or the cat's output, which gets the slot of max|y| (the right half adds its own) and
  // the image.  plane-only: every reader of y takes the image (analyse_graph) -- no fp32 block in the arena, no fp32 store
  TState& y = P.t[op.y];
  TState& dst = cat ? P.t[cat->y] : y;
  const int width = cat ? cat->cout : c;
  dst.plane_only = !cat && bound && !P.keep_twins && P.po_fwd[i];
  dst.ptr = dst.plane_only ? nullptr : A.take_n<float>(n_out * width);
  dst.amax = bound ? bound_slot : new_slot(P);
  if (bound) dst.planes = A.take(n_out * width * 4);
  if (cat) {      // y: a column slice of the cat; the image belongs to the cat (this tensor's only consumer)
    y.ptr = dst.ptr;
    y.ld = width;
    y.amax = dst.amax;
  }
  if (op.relu) sv.mask = A.take_n<unsigned long long>(gcl_bn_mask_len(n_out, c));
  if (op.x2 >= 0) NEED_F32(P.t[op.x2], i, "its residual operand");
  PLAN_CALL(gcl_bn_apply_planes(conv.y, n_out, c, sv.mean, sv.rstd, (const float*)P.params[op.bn_w],
                                (const float*)P.params[op.bn_b], op.x2 >= 0 ? P.t[op.x2].ptr : nullptr, op.relu, y.ptr, y.ld,
                                (uint64_t*)sv.mask, y.amax, bound ? dst.planes : nullptr, (void*)st));
  return GCL_OK;
}

// ME.conv_bn in inference (ops.conv_bn_eval): conv + BatchNorm(running stats) + residual + ReLU, one launch
static int convbn_forward_eval(Plan& P, int i, const gcl_plan_op& op, long long n_out, void* const* bn_eval, hipStream_t st) {
  Arena& A = P.A;
  const long long n_in = P.maps->n_rows[op.level_in];
  TState& y = P.t[op.y];
  const int c = op.cout;
  const float* res = op.x2 >= 0 ? P.t[op.x2].ptr : nullptr;
  if (op.x2 >= 0) NEED_F32(P.t[op.x2], i, "its residual operand");
  y.ptr = A.take_n<float>(n_out * c);
  y.amax = new_slot(P);
  void* const* be = bn_eval ? bn_eval + 4 * op.bn : nullptr;      // scale, shift, mean, rstd
  int rc;
  if (stem_shape(op)) {      // the first layer: VALU convolution, then the BatchNorm apply pass
    float* cy = A.take_n<float>(n_out * c);
    unsigned long long* mask = op.relu ? A.take_n<unsigned long long>(gcl_bn_mask_len(n_out, c)) : nullptr;
    if ((rc = stem_forward(P, i, n_in, n_out, cy, st))) return rc;
    PLAN_CALL(gcl_bn_apply(cy, n_out, c, (const float*)be[2], (const float*)be[3], (const float*)P.params[op.bn_w],
                           (const float*)P.params[op.bn_b], res, op.relu, y.ptr, (uint64_t*)mask, y.amax, (void*)st));
    return GCL_OK;
  }
  if ((rc = conv_prepare(P, i, n_in, "gcl_plan_forward_eval", st))) return rc;
  // scratch of the offset-group launches (small deep layers of an inference pass; 0: the shape / size takes another kernel)
  const bool walks = sorted_table(P.maps->maps[op.map], op.transpose).tbl != nullptr;
  const long long gs_len = walks ? gcl_conv_fwd_groups_scratch_len(n_out, op.K, op.cin, c) : 0;
  float* gscratch = gs_len > 0 ? A.take_n<float>(gs_len) : nullptr;
  return conv_launch(P, i, false, n_in, n_out, be ? (const float*)be[1] : nullptr, be ? (const float*)be[0] : nullptr, res,
                     op.relu, y.amax, y.ptr, gscratch, GCL_CONV_TALL, st);
}

// compact: the record belongs to the touched-row suffix of a pass that runs it on the n_out rows of its list
static int relu_forward(Plan& P, int i, const gcl_plan_op& op, long long n_out, bool compact, hipStream_t st) {
  Arena& A = P.A;
  TState& y = P.t[op.y];
  if (i > 0 && P.fuse_relu[i - 1]) {      // written by the convolution in front of it
    if (compact) y = P.t[op.x];           // (the gathered rows of it when the suffix starts here)
    return GCL_OK;
  }
  const long long n4 = n_out * op.cout / 4;
  NEED_F32(P.t[op.x], i, "its input");
  y.ptr = A.take_n<float>(n_out * op.cout);
  y.amax = new_slot(P);        // published by the kernel itself: the consumer needs no gcl_amax pass
  if (!A.dry) {
    hipLaunchKernelGGL(k_relu_fwd, dim3(grid_for(n4)), dim3(256), 0, st, (const float4*)P.t[op.x].ptr, n4, (float4*)y.ptr, y.amax);
    GCL_CHECK_LAUNCH();
  }
  return GCL_OK;
}

static int cat_forward(Plan& P, int i, const gcl_plan_op& op, long long n_out, hipStream_t st) {
  Arena& A = P.A;
  const TState &xa = P.t[op.x], &xb = P.t[op.x2];
  TState& y = P.t[op.y];
  const int ca = op.cin, cb = op.cout - op.cin;
  NEED_F32(xa, i, "its left input");
  NEED_F32(xb, i, "its right input");
  if (xa.ld == op.cout && xa.ptr == y.ptr && y.ptr) {      // left input already in place (cat_left)
    if (!A.dry) {
      hipLaunchKernelGGL(k_cat_right, dim3(grid_for(n_out * cb / 4)), dim3(256), 0, st, (const float4*)xb.ptr, cb / 4, n_out,
                         ca / 4, (float4*)y.ptr, y.amax, (unsigned short*)y.planes);
      GCL_CHECK_LAUNCH();
    }
    return GCL_OK;
  }
  y.ptr = A.take_n<float>(n_out * op.cout);
  y.amax = new_slot(P);
  // max|cat| = the larger of the inputs' slots when both are known (ops.cat_features: a slot may hold a BatchNorm's
  // bound instead of the measured maximum, and both paths must hand the consumers the same value); else measured
  const bool both = xa.amax && xb.amax;
  if (!A.dry) {
    hipLaunchKernelGGL(k_cat2, dim3(grid_for(n_out * op.cout / 4)), dim3(256), 0, st, (const float4*)xa.ptr, ca / 4,
                       (const float4*)xb.ptr, cb / 4, n_out, (float4*)y.ptr, y.amax, both ? (const int*)xa.amax : nullptr,
                       both ? (const int*)xb.amax : nullptr);
    GCL_CHECK_LAUNCH();
  }
  return GCL_OK;
}

static int rownorm_forward(Plan& P, int i, const gcl_plan_op& op, long long n_out, hipStream_t st) {
  Arena& A = P.A;
  NEED_F32(P.t[op.x], i, "its input");
  float* y = P.t[op.y].ptr = A.take_n<float>(n_out * op.cout);
  P.saved[i].norm = A.take_n<float>(n_out);
  PLAN_CALL(gcl_row_normalize_fwd(P.t[op.x].ptr, n_out, op.cout, y, P.saved[i].norm, (void*)st));
  return GCL_OK;
}

// the forward pass of record i.  rows > 0: a record of the touched-row suffix, on the rows of the pass's list
static int forward_record(Plan& P, int i, const FwdArgs& a, long long rows, hipStream_t st) {
  const gcl_plan_op& op = P.ops[i];
  const long long n_out = rows > 0 ? rows : P.maps->n_rows[op.level_out];
  switch (op.kind) {
    case GCL_OP_CONVBN: return a.eval ? convbn_forward_eval(P, i, op, n_out, a.bn, st) : convbn_forward(P, i, op, n_out, a.bn, st);
    case GCL_OP_CONV: return conv_forward(P, i, st, rows).rc;
    case GCL_OP_RELU: return relu_forward(P, i, op, n_out, rows > 0, st);
    case GCL_OP_CAT: return cat_forward(P, i, op, n_out, st);
    case GCL_OP_ROWNORM: return rownorm_forward(P, i, op, n_out, st);
  }
  set_error("gcl_plan_forward: unknown record kind %d", op.kind);
  return GCL_ERR_ARG;
}

// Head of the touched-row suffix on the rows of the pass's list: its input gathered once (the dense tensor's max-abs slot
// bounds the rows picked from it: no gcl_amax pass); the records of the suffix then run with fwd_cap rows
static int suffix_gather(Plan& P, hipStream_t st) {
  Arena& A = P.A;
  const gcl_plan_op& op = P.ops[P.suffix_first];
  TState& xs = P.t[op.x];
  NEED_F32(xs, P.suffix_first, "the input of the touched-row suffix");
  float* cx = A.take_n<float>(P.fwd_cap * op.cin);
  PLAN_CALL(gcl_gather_rows(xs.ptr, xs.ld ? xs.ld : op.cin, P.maps->n_rows[op.level_in], P.fwd_rows, P.fwd_cap, op.cin, 0.f, cx,
                            (void*)st));
  int32_t* slot = xs.amax;
  xs = TState();      // nothing but the suffix reads this tensor, in either pass
  xs.ptr = cx;
  xs.amax = slot;
  return GCL_OK;
}

// maps of a split build (gcl_maps_build_split): the first record that uses a map made on the side stream waits for it
static int late_maps_wait(const gcl_maps_desc& M, const gcl_plan_op& op, bool* pending, hipStream_t st) {
  if (!is_conv(op) || !((M.late_mask >> op.map) & 1)) return GCL_OK;
  GCL_CHECK_HIP(hipStreamWaitEvent(st, (hipEvent_t)M.ready_event, 0));
  *pending = false;
  return GCL_OK;
}

// The last record's output for the caller.  A pass that ran the suffix on a list hands out a dense tensor all the same: the
// rows of the list hold the features, every other row is zero -- and the padding rows of a saved y and norm become (0, 1)
static int forward_output(Plan& P, float** y_out, hipStream_t st) {
  const int last = (int)P.ops.size() - 1;
  const gcl_plan_op& op = P.ops[last];
  NEED_F32(P.t[op.y], last, "its output (the caller's)");
  *y_out = P.t[op.y].ptr;
  if (P.fwd_cap <= 0) return GCL_OK;
  return spread_rows(P, *y_out, op.kind == GCL_OP_ROWNORM ? P.saved[last].norm : nullptr, P.fwd_rows, P.fwd_cap, op.cout,
                     P.maps->n_rows[op.level_out], y_out, st);
}

static int plan_forward(Plan& P, const FwdArgs& a, float** y_out, hipStream_t st) {
  const gcl_maps_desc& M = *P.maps;
  int rc = forward_setup(P, a, st);
  if (rc) return rc;
  bool late_pending = !P.A.dry && M.ready_event && M.late_mask;
  for (int i = 0; i < (int)P.ops.size(); ++i) {
    const long long rows = (P.fwd_cap > 0 && i >= P.suffix_first) ? P.fwd_cap : 0;
    if (rows > 0 && i == P.suffix_first && (rc = suffix_gather(P, st))) return rc;
    if (late_pending && (rc = late_maps_wait(M, P.ops[i], &late_pending, st))) return rc;
    if ((rc = forward_record(P, i, a, rows, st))) return rc;
  }
  if (late_pending) GCL_CHECK_HIP(hipStreamWaitEvent(st, (hipEvent_t)M.ready_event, 0));      // (the arena outlives the side stream's work)
  return forward_output(P, y_out, st);
}

struct RowView {
  const int32_t* rows = nullptr;
  long long cap = 0, n = 0;
  bool parked = false;
  std::vector<std::pair<const float*, float*>> gathered;
  int32_t* slots = nullptr;      // [n]: a row's position in the list, -1 off it (row_slots: made when a kernel first needs it)
  long long n_rows(const gcl_maps_desc& M, int level) const { return cap > 0 ? cap : M.n_rows[level]; }
};

static int contiguous(Plan& P, TState& g, long long rows, int c, hipStream_t st);

// a compact gradient (g.rv) as the dense [n, c] tensor it stands for: for readers that take no list
static int densify(Plan& P, TState& g, int c, hipStream_t st) {
  if (!g.rv || !g.ptr) return GCL_OK;
  const RowView& V = *g.rv;
  int rc;
  if ((rc = contiguous(P, g, V.cap, c, st))) return rc;
  float* dense;
  if ((rc = spread_rows(P, g.ptr, nullptr, V.rows, V.cap, c, V.n, &dense, st))) return rc;
  g = TState();
  g.ptr = dense;
  return GCL_OK;
}

// Tape.backward's give(): the first gradient of a tensor is kept, later ones are added in arrival order
// gptr: [rows, c] with row pitch ld floats (0 = c: contiguous; numel = rows * c); rv: gptr is compact (TState::rv)
static int give(Plan& P, int tensor, float* gptr, long long numel, hipStream_t st, int32_t* amax = nullptr, int ld = 0,
                int c = 0, RowView* rv = nullptr) {
  Arena& A = P.A;
  if (tensor < 0 || !P.made[tensor] || !gptr) return GCL_OK;
  TState& g = P.g[tensor];
  if (!g.ptr) {
    g = TState();
    g.ptr = gptr;
    g.ld = ld;
    g.rv = rv;
    g.amax = amax;        // published by the producing kernel (valid while the gradient stays this one tensor)
    return GCL_OK;
  }
  if (g.rv || rv) {      // two gradients of which one is compact meet outside a convolution epilogue: added as dense tensors
    GCL_CHECK_ARG(c > 0 && c % 4 == 0, "gcl_plan_backward: a compact gradient needs its channel count");
    TState in;
    in.ptr = gptr;
    in.ld = ld;
    in.rv = rv;
    numel = (g.rv ? g.rv : rv)->n * c;
    int rc;
    if ((rc = densify(P, g, c, st)) || (rc = densify(P, in, c, st))) return rc;
    gptr = in.ptr;
    ld = in.ld;
  }
  float* sum = A.take_n<float>(numel);
  if (!A.dry) {
    if (g.ld || ld) {
      GCL_CHECK_ARG(c > 0 && c % 4 == 0, "gcl_plan_backward: a sliced gradient needs its channel count");
      hipLaunchKernelGGL(k_add2_ld, dim3(grid_for(numel / 4)), dim3(256), 0, st, (const float*)g.ptr, g.ld ? g.ld : c,
                         (const float*)gptr, ld ? ld : c, numel / c, c / 4, (float4*)sum);
    } else {
      hipLaunchKernelGGL(k_add2, dim3(grid_for(numel / 4)), dim3(256), 0, st, (const float4*)g.ptr, (const float4*)gptr,
                         numel / 4, (float4*)sum);
    }
    GCL_CHECK_LAUNCH();
  }
  g = TState();
  g.ptr = sum;
  return GCL_OK;
}

// a gradient that is a column slice, for consumers that want contiguous rows: copied once (rare paths only -- the
// BatchNorm backward kernels and the convolution epilogue read slices as they are)
static int contiguous(Plan& P, TState& g, long long rows, int c, hipStream_t st) {
  if (!g.ld || !g.ptr) return GCL_OK;
  Arena& A = P.A;
  float* out = A.take_n<float>(rows * c);
  if (!A.dry) {
    hipLaunchKernelGGL(k_add2_ld, dim3(grid_for(rows * c / 4)), dim3(256), 0, st, (const float*)g.ptr, g.ld, (const float*)nullptr,
                       0, rows, c / 4, (float4*)out);
    GCL_CHECK_LAUNCH();
  }
  g = TState();
  g.ptr = out;
  return GCL_OK;
}

// The rows the backward of a record runs on, and where its saved operands come from.  cap == 0: every row of the record's
// level, the saved tensors as they are.  cap > 0: the rows of a list (rows[cap]: distinct rows of [0, n) ascending, -1
// padding) -- the records of the touched-row suffix run through the entries the dense pass calls, with cap rows, on compact
// [cap, c] tensors.  A row's results do not depend on the other rows of a launch, and a row of dy that is zero gives a zero
// row of every gradient and adds nothing to a weight gradient: the input gradient is the dense pass's row for row, the weight
// gradients are its sums over fewer rows in other groups.  The -1 padding rows are zero rows throughout (their norm reads 1:
// no 0 / 0).  The saved operands are gathered onto the list, each once (`gathered`); after a forward pass that ran the
// suffix on this list (`parked`, P.fwd_cap > 0) they ARE the compact tensors, with inert padding rows.
// *out = the saved operand src ([n, c], row pitch ld) on the rows of V; pad: the value of its padding rows
static int saved_rows(Plan& P, RowView& V, const float* src, int ld, int c, float pad, hipStream_t st, const float** out) {
  Arena& A = P.A;
  *out = src;
  if (V.cap <= 0 || V.parked) return GCL_OK;
  for (auto& e : V.gathered)
    if (e.first == src) {
      *out = e.second;
      return GCL_OK;
    }
  float* rows = A.take_n<float>(V.cap * c);
  PLAN_CALL(gcl_gather_rows(src, ld, V.n, V.rows, V.cap, c, pad, rows, (void*)st));
  V.gathered.push_back({src, rows});
  *out = rows;
  return GCL_OK;
}
static int saved_rows(Plan& P, RowView& V, const TState& t, int c, hipStream_t st, const float** out, int rec) {
  if (V.cap > 0 && !V.parked) NEED_F32(t, rec, "a saved operand it gathers onto a row list");
  return saved_rows(P, V, t.ptr, t.ld ? t.ld : c, c, 0.f, st, out);
}

// V.slots, made once per list
static int row_slots(Plan& P, RowView& V, hipStream_t st) {
  Arena& A = P.A;
  if (V.slots) return GCL_OK;
  V.slots = A.take_n<int32_t>(V.n);
  PLAN_CALL(gcl_row_slots(V.rows, V.cap, V.n, V.slots, (void*)st));
  return GCL_OK;
}

// ops._SparseConvFn.backward for record i with output gradient dy (dy.amax set when a producer published it)
static int conv_backward(Plan& P, int i, TState dy, RowView& V, void* const* grads, hipStream_t st) {
  Arena& A = P.A;
  const gcl_plan_op& op = P.ops[i];
  const gcl_maps_desc& M = *P.maps;
  const gcl_map_desc& m = M.maps[op.map];
  const long long n_in = V.n_rows(M, op.level_in), n_out = V.n_rows(M, op.level_out);
  TState& x = P.t[op.x];
  float* dW = (float*)grads[op.w];
  int rc;
  if (stem_shape(op)) {
    NEED_F32(x, i, "its input (first layer)");
    NEED_F32(dy, i, "its output gradient (first layer)");
    float* scratch = A.take_n<float>(gcl_stem_bwd_weight_scratch_len(op.K, op.cin, op.cout, n_out));
    hipStream_t ws = fork_aux(P, st);
    ProfScope ps(P, ws, 2, (double)m.n_pairs, op.cin, op.cout, n_in, n_out, op.K);
    PLAN_CALL(gcl_stem_bwd_weight(x.ptr, dy.ptr, m.nbr, n_out, op.K, op.cin, op.cout, scratch, dW, m.presence,
                                  m.presence ? P.not_ones : nullptr, (void*)ws));
    return GCL_OK;
  }
  const int wi = P.widx[op.w];
  if ((rc = ensure_amax(P, dy, n_out * op.cout, st, i))) return rc;
  const int32_t* w_amax = P.w_amax + (long long)wi * GCL_AMAX_WORDS;
  const double pairs = (double)(m.kernel_size > 1 ? m.n_pairs : n_out);
  // kernel_size 1: both operands of the weight gradient streamed once in fp32, no pair list (as ops._ConvFn.backward decides)
  const long long rows_len = m.kernel_size == 1 ? gcl_conv_bwd_weight_rows_scratch_len(op.cin, op.cout, 4, n_in) : 0;
  const bool pl_w = rows_len <= 0 && op.cin >= P.presplit && op.cout >= P.presplit;      // weight gradient on plane images
  const bool pl_x = op.cout >= P.presplit;                              // input gradient reads dy's plane image
  if ((pl_w || (pl_x && P.made[op.x])) && (rc = ensure_planes(P, dy, n_out, op.cout, st, i))) return rc;
  if (pl_w) {
    x.amax = P.saved[i].x_amax;
    if ((rc = ensure_planes(P, x, n_in, op.cin, st, i))) return rc;
  }
  // every launch below that takes the fp32 form of x or dy: a plane-only tensor has none
  if (!pl_w) NEED_F32(x, i, "its input (weight gradient)");
  if (!pl_w) NEED_F32(dy, i, "its output gradient (weight gradient)");
  if (!pl_x && P.made[op.x]) NEED_F32(dy, i, "its output gradient (input gradient)");
  if (P.made[op.x] && !P.g[op.x].ptr && P.mask_from[i] >= 0) NEED_F32(x, i, "its input (ReLU mask of the input-gradient epilogue)");
  if (op.bias >= 0) NEED_F32(dy, i, "its output gradient (bias gradient)");
  const float* xr;      // the fp32 rows of x: what the row-stream weight gradient and a ReLU mask in the epilogue read
  if ((rc = saved_rows(P, V, x, op.cin, st, &xr, i))) return rc;
  // every operand of the weight gradient is enqueued: fork here, so that it runs beside the input gradient below
  hipStream_t ws = fork_aux(P, st);
  if (P.made[op.x]) {      // input gradient: the same output-stationary kernel over the opposite table
    // mirrored offsets over the same table on a stride-1 map, the plain transpose over the opposite table otherwise
    const int mode = (m.kernel_size > 1 && !op.transpose && m.stride == 1) ? 2 : 1;
    const SortedTable T = sorted_table(m, !op.transpose && m.stride != 1);
    const int32_t *tbl = T.tbl, *order = T.order, *mask = T.mask;
    GCL_CHECK_ARG(mode == P.wmode[wi], "gcl_plan_backward: record %d: input-gradient pack mode mismatch", i);
    GCL_CHECK_ARG(A.dry || m.kernel_size == 1 || tbl, "gcl_plan_backward: record %d needs a sorted table the maps do not carry", i);
    const bool pl = pl_x;
    float* acc = P.g[op.x].ptr;       // a gradient that already reached x through another path: added in the epilogue
    const int acc_ld = P.g[op.x].ld;  // ... possibly a column slice of a cat's gradient
    // ... or compact, the listed rows of a gradient that is zero elsewhere: the launch runs plain, and one launch on those
    // rows adds them to its output (the same single fp32 addition per element as the epilogue's)
    const RowView* acc_rows = P.g[op.x].rv;
    GCL_CHECK_ARG(!acc_rows || (V.cap <= 0 && acc_rows->n == n_in && op.cin % 4 == 0),
                  "gcl_plan_backward: record %d: a compact gradient waits at an input of another shape", i);
    float* dx = A.take_n<float>(n_in * op.cin);
    int32_t* dx_amax = nullptr;
    {
      ProfScope ps(P, st, acc && !acc_rows ? 1 : 0, pairs, op.cout, op.cin, n_out, n_in, op.K);
      if (acc && !acc_rows)
        PLAN_CALL(gcl_conv_fwd_fused_ld(pl ? (const float*)dy.planes : dy.ptr, n_out, pl ? 1 : 0, P.pack_bwd + P.off_bwd[wi], 4,
                                        dy.amax, w_amax, tbl, order, mask, n_in, op.K, op.cout, op.cin, nullptr, nullptr, acc,
                                        acc_ld, 0, nullptr, dx, nullptr, 0, (void*)st));
      else if (!acc && P.mask_from[i] >= 0) {
        // x came out of a ReLU that nothing else reads: its backward (g where y > 0) in this epilogue, max|g| published
        dx_amax = new_slot(P);
        PLAN_CALL(gcl_conv_fwd_fused(pl ? (const float*)dy.planes : dy.ptr, n_out, pl ? 1 : 0, P.pack_bwd + P.off_bwd[wi], 4,
                                     dy.amax, w_amax, tbl, order, mask, n_in, op.K, op.cout, op.cin, nullptr, nullptr, xr, 2,
                                     dx_amax, dx, nullptr, 0, (void*)st));
        if (P.relu_masked.size() != P.ops.size()) P.relu_masked.assign(P.ops.size(), 0);
        P.relu_masked[P.mask_from[i]] = 1;
      } else
        PLAN_CALL(gcl_conv_fwd(pl ? (const float*)dy.planes : dy.ptr, n_out, pl ? 1 : 0, P.pack_bwd + P.off_bwd[wi], 4, dy.amax,
                               w_amax, tbl, order, mask, n_in, op.K, op.cout, op.cin, nullptr, dx, nullptr, 0, (void*)st));
    }
    if (acc_rows)
      PLAN_CALL(gcl_scatter_add_rows(acc, acc_ld ? acc_ld : op.cin, acc_rows->rows, acc_rows->cap, op.cin, n_in, dx, op.cin,
                                     (void*)st));
    P.g[op.x] = TState();
    P.g[op.x].ptr = dx;
    P.g[op.x].amax = dx_amax;
  }
  if (rows_len > 0) {
    float* scratch = A.take_n<float>(rows_len);
    ProfScope ps(P, ws, 3, pairs, op.cin, op.cout, n_in, n_out, op.K);
    PLAN_CALL(gcl_conv_bwd_weight_rows(xr, dy.ptr, n_in, op.cin, op.cout, 4, P.saved[i].x_amax, dy.amax, scratch, dW,
                                       (void*)ws));
  } else {      // weight gradient over the compacted pair lists
    GCL_CHECK_ARG(V.cap <= 0, "gcl_plan_backward: record %d: the pair-list weight gradient does not run on a row list", i);
    const int32_t *pa = m.pair_in, *pb = m.pair_out;
    if (op.transpose) { pa = m.pair_out; pb = m.pair_in; }
    GCL_CHECK_ARG(A.dry || (pa && pb), "gcl_plan_backward: record %d needs pair lists the maps do not carry", i);
    const int sorted_side = m.kernel_size == 1 ? 0 : (op.transpose ? 1 : 2);     // the map's out rows ascend per offset
    const long long n_sorted = sorted_side == 1 ? n_in : (sorted_side == 2 ? n_out : 0);
    float* scratch = A.take_n<float>(gcl_conv_bwd_weight_scratch_len(op.K, op.cin, op.cout, m.seg_off[op.K], n_sorted));
    const bool pl = pl_w;
    ProfScope ps(P, ws, 2, pairs, op.cin, op.cout, n_in, n_out, op.K);
    // m.dw_bounds: over the map's pair_out with n_out(map) rows -- the sorted list of this launch on either side
    const int32_t* rgb = (sorted_side != 0 && n_sorted == m.n_out) ? m.dw_bounds : nullptr;
    PLAN_CALL(gcl_conv_bwd_weight_rg(pl ? (const float*)x.planes : x.ptr, n_in, pl ? (const float*)dy.planes : dy.ptr, n_out,
                                     pl ? 1 : 0, sorted_side, pa, pb, m.seg_off, op.K, op.cin, op.cout, 4, P.saved[i].x_amax,
                                     dy.amax, scratch, dW, rgb, (void*)ws));
  }
  if (op.bias >= 0) {
    double* scratch = A.take_n<double>(gcl_bn_scratch_len(n_out, op.cout));
    PLAN_CALL(gcl_col_sum(dy.ptr, n_out, op.cout, scratch, (float*)grads[op.bias], (void*)ws));
  }
  return GCL_OK;
}

// Tape.backward for record i on the rows of V: takes the gradient of the record's output out of P.g and gives the gradients
// of its inputs
static int backward_record(Plan& P, int i, RowView& V, void* const* grads, hipStream_t st) {
  Arena& A = P.A;
  const gcl_maps_desc& M = *P.maps;
  const gcl_plan_op& op = P.ops[i];
  const long long n_out = V.n_rows(M, op.level_out), n_in = V.n_rows(M, op.level_in);
  TState g = P.g[op.y];
  P.g[op.y] = TState();
  if (!g.ptr) return GCL_OK;
  int rc;
  // a compact gradient stays compact through an ME.cat and into the first BatchNorm backward, which mixes the rows: its
  // statistics pass reads the listed rows only, its apply pass takes g through the list's slots and leaves dres compact
  // -- every other record reads it as the dense tensor it stands for
  const bool rows_ok = g.rv && V.cap <= 0 && g.rv->n == n_out &&
                       (op.kind == GCL_OP_CAT || (op.kind == GCL_OP_CONVBN && (!op.relu || P.saved[i].mask)));
  if (g.rv && !rows_ok && (rc = densify(P, g, op.cout, st))) return rc;
  RowView* const rv = g.rv;      // the list of a gradient that stays compact in this record
  switch (op.kind) {
    case GCL_OP_CONVBN: {
      const OpSaved& sv = P.saved[i];
      const int c = op.cout;
      float* sum_g = (float*)grads[op.bn_b];
      float* sum_gx = (float*)grads[op.bn_w];
      double* scratch = A.take_n<double>(gcl_bn_scratch_len(n_out, c));
      // bound mode: dx is read as a plane image by the input gradient (and by the weight gradient when both widths allow)
      const bool bound = sv.xrange && c >= P.presplit && !stem_shape(op);
      // plane-only: the input gradient and the weight gradient of this record both read dx as a plane image
      // (analyse_graph) -- no fp32 block, no fp32 store.  The row-list apply pass keeps its fp32 dx: the analysis
      // leaves out every record a compact gradient can reach
      TState d;
      d.plane_only = bound && !P.keep_twins && P.po_bwd[i];
      GCL_CHECK_ARG(!(d.plane_only && rv), "gcl_plan_backward: record %d: a compact gradient reached a BatchNorm whose input "
                                           "gradient the plan keeps as a plane image only", i);
      d.ptr = d.plane_only ? nullptr : A.take_n<float>(n_out * c);
      d.amax = new_slot(P);
      if (rv) {
        if ((rc = row_slots(P, *rv, st))) return rc;
        PLAN_CALL(gcl_bn_bwd_reduce_rows(sv.conv_out, g.ptr, g.ld, rv->slots, (const uint64_t*)sv.mask, n_out, c, sv.mean, sv.rstd,
                                         op.relu, scratch, sum_g, sum_gx, sv.xrange, (const float*)P.params[op.bn_w],
                                         bound ? d.amax : nullptr, (void*)st));
      } else {
        PLAN_CALL(gcl_bn_bwd_reduce_range(sv.conv_out, g.ptr, g.ld, nullptr, (const uint64_t*)sv.mask, n_out, c, sv.mean, sv.rstd,
                                          op.relu, scratch, sum_g, sum_gx, sv.xrange, (const float*)P.params[op.bn_w],
                                          bound ? d.amax : nullptr, (void*)st));
      }
      if (bound) d.planes = A.take(n_out * c * 4);
      const long long res_rows = rv ? rv->cap : n_out;
      float* dres = op.x2 >= 0 ? A.take_n<float>(res_rows * c) : nullptr;
      if (rv)
        PLAN_CALL(gcl_bn_bwd_apply_rows(sv.conv_out, g.ptr, g.ld, rv->slots, (const uint64_t*)sv.mask, n_out, c, sv.mean, sv.rstd,
                                        (const float*)P.params[op.bn_w], sum_g, sum_gx, op.relu, d.ptr, dres, d.amax, d.planes,
                                        (void*)st));
      else
        PLAN_CALL(gcl_bn_bwd_apply_planes(sv.conv_out, g.ptr, g.ld, nullptr, (const uint64_t*)sv.mask, n_out, c, sv.mean,
                                          sv.rstd, (const float*)P.params[op.bn_w], sum_g, sum_gx, op.relu, d.ptr, dres,
                                          d.amax, d.planes, (void*)st));
      if ((rc = conv_backward(P, i, d, V, grads, st))) return rc;
      return give(P, op.x2, dres, res_rows * c, st, nullptr, 0, c, rv);
    }
    case GCL_OP_CONV:
      if ((rc = contiguous(P, g, n_out, op.cout, st))) return rc;
      return conv_backward(P, i, g, V, grads, st);
    case GCL_OP_RELU: {
      if ((size_t)i < P.relu_masked.size() && P.relu_masked[i]) {      // applied by the consumer's input-gradient epilogue
        P.relu_masked[i] = 0;
        return give(P, op.x, g.ptr, n_out * op.cout, st, g.amax, g.ld, op.cout);
      }
      if ((rc = contiguous(P, g, n_out, op.cout, st))) return rc;
      const float* y;
      NEED_F32(P.t[op.y], i, "its saved output");
      if ((rc = saved_rows(P, V, P.t[op.y], op.cout, st, &y, i))) return rc;
      const long long numel = n_out * op.cout;
      float* gx = A.take_n<float>(numel);
      int32_t* slot = new_slot(P);
      if (!A.dry) {
        hipLaunchKernelGGL(k_relu_bwd, dim3(grid_for(numel / 4)), dim3(256), 0, st, (const float4*)g.ptr, (const float4*)y,
                           numel / 4, (float4*)gx, slot);
        GCL_CHECK_LAUNCH();
      }
      return give(P, op.x, gx, numel, st, slot, 0, op.cout);
    }
    case GCL_OP_CAT: {
      // the gradients of the two inputs ARE the column slices of g: handed on as views (row pitch = the cat's width); their
      // readers -- the BatchNorm backward kernels, a convolution epilogue that adds a waiting gradient -- take the pitch
      // (a compact gradient is split the same way: the slices of its cap rows)
      const int ca = op.cin, cb = op.cout - op.cin;
      const long long rows = rv ? rv->cap : n_out;
      if ((rc = contiguous(P, g, rows, op.cout, st))) return rc;
      if ((rc = give(P, op.x, g.ptr, rows * ca, st, nullptr, op.cout, ca, rv))) return rc;
      return give(P, op.x2, g.ptr + ca, rows * cb, st, nullptr, op.cout, cb, rv);
    }
    case GCL_OP_ROWNORM: {
      if ((rc = contiguous(P, g, n_out, op.cout, st))) return rc;
      const float *y, *norm;
      NEED_F32(P.t[op.y], i, "its saved output");
      if ((rc = saved_rows(P, V, P.t[op.y], op.cout, st, &y, i))) return rc;
      if ((rc = saved_rows(P, V, P.saved[i].norm, 1, 1, 1.f, st, &norm))) return rc;
      float* dx = A.take_n<float>(n_in * op.cin);
      int32_t* slot = new_slot(P);
      PLAN_CALL(gcl_row_normalize_bwd(y, g.ptr, norm, n_out, op.cout, dx, slot, (void*)st));
      return give(P, op.x, dx, n_in * op.cin, st, slot, 0, op.cin);
    }
    default:
      set_error("gcl_plan_backward: unknown record kind %d", op.kind);
      return GCL_ERR_ARG;
  }
}

// The touched-row suffix on the rows of V's list: dy gathered onto it, the records on cap rows, and the compact gradient of the
// suffix's input handed on compact (TState::rv = &V, which has to outlive the records that read it): no zero-filled dense
// tensor -- the records behind it keep it compact up to the first BatchNorm backward (backward_record)
static int suffix_backward(Plan& P, const float* dy, void* const* grads, RowView& V, hipStream_t st) {
  Arena& A = P.A;
  const gcl_plan_op &head = P.ops[P.suffix_first], &tail = P.ops.back();
  V.n = P.maps->n_rows[head.level_in];
  V.parked = P.fwd_cap > 0;
  float* dyc = A.take_n<float>(V.cap * tail.cout);
  PLAN_CALL(gcl_gather_rows(dy, tail.cout, V.n, V.rows, V.cap, tail.cout, 0.f, dyc, (void*)st));
  P.g[tail.y] = TState();
  P.g[tail.y].ptr = dyc;
  int rc;
  for (int i = (int)P.ops.size() - 1; i >= P.suffix_first; --i)
    if ((rc = backward_record(P, i, V, grads, st))) return rc;
  const TState g = P.g[head.x];      // nothing but the suffix reads this tensor: the compact gradient is all of it
  P.g[head.x] = TState();
  // the room of the dense [n, cin] gradient stays reserved: a densify() behind the suffix -- a segment that ends in front of
  // the first BatchNorm backward, a compact gradient that meets a dense one -- takes as much, and the sizing has to cover it
  A.take_n<float>(V.n * head.cin);
  if (!g.ptr) return GCL_OK;      // the suffix's input wants no gradient
  return give(P, head.x, g.ptr, V.cap * head.cin, st, nullptr, 0, head.cin, &V);
}

static int tensor_width(const Plan& P, int tensor) {      // channels of a tensor a record of the plan produces
  const int maker = P.readers[tensor].maker;
  return maker >= 0 ? P.ops[maker].cout : 0;
}

static int plan_backward(Plan& P, const float* dy, void* const* grads, int first, int last, hipStream_t st,
                         const int32_t* rows = nullptr, long long cap = 0) {
  Arena& A = P.A;
  const gcl_maps_desc& M = *P.maps;
  const size_t nw = P.worder.size();
  const int n_ops = (int)P.ops.size();
  if (last == (int)P.ops.size()) {
    P.g[P.ops.back().y] = TState();
    P.g[P.ops.back().y].ptr = (float*)dy;
  }
  if (P.bwd_packed && last == (int)P.ops.size()) {
    int rcj = join_aux(P, st);      // packs made on the aux stream during the forward pass
    if (rcj) return rcj;
  }
  if (!P.bwd_packed) {       // input-gradient packs of all kernels in one launch (WeightAmaxGroup.packed("bwd"))
    P.pack_bwd = (unsigned char*)A.take(P.bytes_bwd);
    if (P.n_bwd && !A.dry) {
      const long long* tab = (const long long*)P.state;
      PLAN_CALL(gcl_pack_weights_multi((const int64_t*)(tab + 2 * nw + 8 * nw), P.n_bwd, P.wgs_bwd, 4, P.w_amax, P.pack_bwd,
                                       (void*)st));
    }
    P.bwd_packed = true;
  }
  // touched-row suffix: on the rows of a list when there is one and it is short, else dense like every other record
  int top = last - 1, rc;
  long long reserve_to = 0;
  RowView list;      // the list of this call: the compact gradients behind the suffix point at it
  if (last == n_ops && !A.dry) P.suffix_rows_used = 0;
  if (last == n_ops && P.suffix_first < n_ops && P.suffix_rows_ok && first <= P.suffix_first) {
    const long long n = M.n_rows[P.ops[P.suffix_first].level_in];
    // counted: the same calls without a launch, which leave nothing behind but *end, the arena offset they reached
    auto run = [&](const int32_t* r, long long c, bool counted, long long* end) {
      RowView scratch_view;      // a counted run leaves no gradient behind that could name its list
      RowView& V = counted ? scratch_view : list;
      V.rows = r;
      V.cap = c;
      const Arena a0 = A;
      const long long slot0 = P.next_slot;
      std::vector<TState> g0;
      std::vector<char> masked0;
      if (counted) {
        g0 = P.g;
        masked0 = P.relu_masked;
        A.dry = true;
      }
      const int rcs = suffix_backward(P, dy, grads, V, st);
      *end = A.off;
      if (counted) {
        A = a0;
        P.next_slot = slot0;
        P.g = g0;
        P.relu_masked = masked0;
      }
      return rcs;
    };
    long long end = 0;
    if (P.fwd_cap > 0) {      // the forward pass ran the suffix on its list and sized the arena for these calls (dry: that sizing)
      rows = P.fwd_rows;
      cap = P.fwd_cap;
    } else if (A.dry) {      // sizing: room for the largest list that takes this path (2 cap < n), or for the dense records
      cap = 0;
      if ((n - 1) / 2 > 0 && (rc = run(nullptr, (n - 1) / 2, true, &reserve_to))) return rc;
    } else if (!rows || cap <= 0 || 2 * cap >= n || run(rows, cap, true, &end) != GCL_OK || end > A.size) {
      cap = 0;      // no list, a long one, or an arena sized for another bound: the dense records
    }
    if (cap > 0) {
      if ((rc = run(rows, cap, false, &end))) return rc;
      top = P.suffix_first - 1;
      if (!A.dry) P.suffix_rows_used = cap;
    }
  }
  RowView dense;
  for (int i = top; i >= first; --i) {
    if (reserve_to && i == P.suffix_first - 1 && A.off < reserve_to) A.off = reserve_to;
    if ((rc = backward_record(P, i, dense, grads, st))) return rc;
  }
  if (reserve_to && A.off < reserve_to) A.off = reserve_to;
  // a segment that ends in front of the first BatchNorm backward: the gradients that wait for the next call wait dense
  for (size_t t = 0; t < P.g.size(); ++t)
    if (P.g[t].rv && (rc = densify(P, P.g[t], tensor_width(P, (int)t), st))) return rc;
  return join_aux(P, st);      // the caller may hand the gradients of this segment to a collective / the optimizer next
}

// gcl_plan_create, step 1: the records name tensors in the order they are made and every parameter once, in shapes the
// plan's kernels take.  Leaves made, widx and n_bn behind
static int validate_records(Plan& P) {
  for (size_t q = 0; q < P.worder.size(); ++q) {
    const int p = P.worder[q];
    GCL_CHECK_ARG(p >= 0 && p < P.n_params && P.widx[p] < 0, "gcl_plan_create: weight_order[%d] is no parameter id, or a second "
                                                               "mention of one", (int)q);
    P.widx[p] = (int)q;
  }
  std::vector<char> seen_param(P.n_params, 0);
  auto claim = [&](int p) {       // every parameter belongs to exactly one record (its gradient is written, not added)
    if (p < 0 || p >= P.n_params || seen_param[p]) return false;
    seen_param[p] = 1;
    return true;
  };
  auto tensor_ok = [&](int t) { return t >= 0 && t < P.n_tensors; };
  for (int i = 0; i < (int)P.ops.size(); ++i) {
    const gcl_plan_op& op = P.ops[i];
    bool ok = tensor_ok(op.x) && tensor_ok(op.y) && op.y != 0 && !P.made[op.y] && (op.x == 0 || P.made[op.x]) &&
              op.level_in >= 0 && op.level_in < GCL_MAX_LEVELS && op.level_out >= 0 && op.level_out < GCL_MAX_LEVELS &&
              op.cin > 0 && op.cout > 0 && (op.x2 < 0 || (tensor_ok(op.x2) && P.made[op.x2]));
    if (ok && is_conv(op)) {
      ok = claim(op.w) && op.map >= 0 && op.map < GCL_MAX_MAPS && op.K >= 1 && op.K <= 125;
      if (ok && op.bias >= 0) ok = claim(op.bias) && op.kind == GCL_OP_CONV;
      if (ok && op.kind == GCL_OP_CONVBN) ok = claim(op.bn_w) && claim(op.bn_b) && op.bn >= 0 && op.cout % 4 == 0;
      if (ok && op.kind == GCL_OP_CONVBN && op.bn + 1 > P.n_bn) P.n_bn = op.bn + 1;
      // the first layer has no input gradient; MFMA shapes otherwise (generic VALU shapes stay on the per-operator path)
      if (ok) ok = stem_shape(op) ? op.x == 0 : (op.cin % 32) == 0 && (op.cout % 32) == 0 && op.K <= 27 && P.widx[op.w] >= 0;
    } else if (ok && op.kind == GCL_OP_CAT) {
      ok = op.x2 >= 0 && op.cin % 4 == 0 && (op.cout - op.cin) > 0 && (op.cout - op.cin) % 4 == 0 && op.level_in == op.level_out;
    } else if (ok) {
      ok = (op.kind == GCL_OP_RELU || op.kind == GCL_OP_ROWNORM) && op.cin == op.cout && op.cout % 4 == 0 && op.level_in == op.level_out;
    }
    GCL_CHECK_ARG(ok, "gcl_plan_create: record %d is malformed, or of a kind or shape the plan does not take", i);
    P.made[op.y] = 1;
  }
  return GCL_OK;
}

// step 2: per kernel of weight_order its shape, its input-gradient pack mode and its place in the packs
static int weight_tables(Plan& P) {
  for (const gcl_plan_op& op : P.ops) {
    if (!is_conv(op) || stem_shape(op)) continue;
    const int q = P.widx[op.w];
    P.wK[q] = op.K; P.wcin[q] = op.cin; P.wcout[q] = op.cout;
    // input-gradient layout recorded by the forward pass: mirrored offsets on a stride-1 map, plain transpose otherwise
    // (the caller tells stride-1 3^3 / 5^3 maps apart through `transpose` and level_in == level_out)
    if (op.x != 0) P.wmode[q] = (op.K > 1 && !op.transpose && op.level_in == op.level_out) ? 2 : 1;
  }
  for (size_t q = 0; q < P.worder.size(); ++q) {
    GCL_CHECK_ARG(P.wK[q], "gcl_plan_create: weight_order names a parameter no record uses");
    const long long bytes = (gcl_pack_weights_bytes((int)P.wK[q], (int)P.wcin[q], (int)P.wcout[q], 4) + 255) / 256 * 256;
    P.off_fwd[q] = P.bytes_fwd;
    P.bytes_fwd += bytes;
    if (P.wmode[q]) {
      P.off_bwd[q] = P.bytes_bwd;
      P.bytes_bwd += bytes;
      ++P.n_bwd;
    }
  }
  return GCL_OK;
}

// step 3: who reads what, once, and the decisions both passes take from it
static void analyse_graph(Plan& P) {
  const int n_ops = (int)P.ops.size();
  P.readers.assign(P.n_tensors, Readers());
  for (int i = 0; i < n_ops; ++i) {
    const gcl_plan_op& o = P.ops[i];
    P.readers[o.y].maker = i;
    P.readers[o.x].x.push_back(i);
    if (o.x2 >= 0) P.readers[o.x2].x2.push_back(i);
  }
  P.readers[P.ops.back().y].output = true;       // the plan's output keeps its own tensor
  P.fuse_relu.assign(n_ops, 0);
  P.cat_left.assign(n_ops, -1);
  P.mask_from.assign(n_ops, -1);
  for (int i = 0; i < n_ops; ++i) {
    const gcl_plan_op& a = P.ops[i];
    if (!is_conv(a) || a.cin <= 4) continue;
    const Readers &out = P.readers[a.y], &in = P.readers[a.x];
    const int next = out.x.empty() ? -1 : out.x[0];
    // CONV directly followed by the RELU that alone reads it (model/resunet.py:222-224: conv1_tr, MEF.relu, final): the
    // convolution's epilogue applies the ReLU and publishes max|y|
    if (a.kind == GCL_OP_CONV && next == i + 1 && P.ops[next].kind == GCL_OP_RELU && out.only(next)) P.fuse_relu[i] = 1;
    if (a.kind == GCL_OP_CONVBN && out.count() == 1 && !out.output && next > i && P.ops[next].kind == GCL_OP_CAT) P.cat_left[i] = next;
    if (in.maker >= 0 && P.ops[in.maker].kind == GCL_OP_RELU && in.count() == 1 && !in.output) P.mask_from[i] = in.maker;
  }
  // touched-row suffix: the longest chain of row-local records that ends at the last record (each one the only reader of the
  // record in front of it), cut at the front until nothing but the chain reads its input (model/resunet.py:222-230: conv1_tr,
  // MEF.relu, final, the row normalisation -- behind the ME.cat)
  auto row_local = [](const gcl_plan_op& o) {
    return o.kind == GCL_OP_ROWNORM || o.kind == GCL_OP_RELU ||
           (o.kind == GCL_OP_CONV && o.K == 1 && !o.transpose && o.level_in == o.level_out && o.cin > 4);
  };
  int s = n_ops;
  while (s > 0 && row_local(P.ops[s - 1]) &&
         (s == n_ops || (P.ops[s].x == P.ops[s - 1].y && P.readers[P.ops[s - 1].y].count() == 1)))
    --s;
  while (s < n_ops && P.readers[P.ops[s].x].count() != 1) ++s;
  P.suffix_first = s;
  P.suffix_rows_ok = true;
  for (int i = s; i < n_ops; ++i)
    if (P.ops[i].kind == GCL_OP_CONV && gcl_conv_bwd_weight_rows_scratch_len(P.ops[i].cin, P.ops[i].cout, 4, 128) <= 0)
      P.suffix_rows_ok = false;
  // Plane-only tensors: which tensors exist as a plane image only.  A CONVBN record in bound mode writes the
  // fp16 hi/lo image of its output y (forward apply pass) and of its BatchNorm input gradient dx (backward apply pass) beside
  // the fp32 tensor, the same number of bytes again.  The default is to keep the fp32 twin; it is dropped only when the record
  // can run in bound mode and EVERY reader provably takes the image:
  //   y  (po_fwd): each reader is a convolution record in front of the touched-row suffix with kernel size > 1 and both
  //                widths >= presplit -- its forward launch (cin >= presplit) and its pair-list weight gradient (pl_w) read
  //                x.planes.  Anything else keeps fp32: a residual operand or an ME.cat input (x2, the in-place cat_left
  //                case), a ReLU / row normalisation, a kernel_size-1 record (row-stream weight gradient), a narrow record
  //                (fp32 weight gradient), the ReLU-mask epilogue (mask_from), the first layer, the suffix (gathers fp32 rows),
  //                the plan's output (the caller's), a tensor nobody reads.
  //   dx (po_bwd): the tensor never leaves backward_record -- its readers are the record's own input gradient (cout >= presplit:
  //                the image) and weight gradient (the image iff pl_w: kernel size > 1, cin >= presplit), so it crosses no
  //                segment cut and reaches no give().  A bias gradient (gcl_col_sum) or the first layer would read fp32, and
  //                a record a compact gradient (TState::rv) can reach runs the row-list apply pass, which keeps its fp32 dx.
  // The passes re-check the run-time half (`bound`) and every fp32 read (NEED_F32): a reader this analysis overlooked is an
  // error return, not a null pointer in a kernel.
  P.po_fwd.assign(n_ops, 0);
  P.po_bwd.assign(n_ops, 0);
  // tensors whose gradient can arrive compact: the suffix's input, and from there the inputs of an ME.cat and the residual
  // operand of a CONVBN that takes a compact gradient (its dres stays compact) -- backward_record's rows_ok
  std::vector<char> may_rv(P.n_tensors, 0);
  if (P.suffix_first < n_ops) may_rv[P.ops[P.suffix_first].x] = 1;
  for (int i = n_ops - 1; i >= 0; --i) {
    const gcl_plan_op& o = P.ops[i];
    if (!may_rv[o.y]) continue;
    if (o.kind == GCL_OP_CAT) may_rv[o.x] = may_rv[o.x2] = 1;
    if (o.kind == GCL_OP_CONVBN && o.x2 >= 0) may_rv[o.x2] = 1;
  }
  for (int i = 0; i < n_ops && i < P.suffix_first; ++i) {
    const gcl_plan_op& o = P.ops[i];
    // bound mode as convbn_forward decides it: column ranges from the MFMA epilogue, a wide output, the residual's slot known
    bool bound = o.kind == GCL_OP_CONVBN && !stem_shape(o) && o.cout >= P.presplit && (o.cout % 32) == 0;
    if (bound && o.x2 >= 0) {
      const int maker = P.readers[o.x2].maker;
      const int k = maker >= 0 ? P.ops[maker].kind : 0;
      bound = k == GCL_OP_CONVBN || k == GCL_OP_RELU || k == GCL_OP_CAT;      // producers that publish max|x2|
    }
    if (!bound) continue;
    P.po_bwd[i] = o.K > 1 && o.cin >= P.presplit && o.bias < 0 && !may_rv[o.y];
    const Readers& R = P.readers[o.y];
    bool ok = P.cat_left[i] < 0 && !R.output && R.x2.empty() && !R.x.empty();
    for (int j : R.x) {
      const gcl_plan_op& r = P.ops[j];
      ok = ok && j < P.suffix_first && is_conv(r) && !stem_shape(r) && r.K > 1 && r.cin >= P.presplit && r.cout >= P.presplit &&
           P.mask_from[j] < 0;
    }
    P.po_fwd[i] = ok;
  }
}

static int check_maps(const Plan& P, const gcl_maps_desc* M) {
  GCL_CHECK_ARG(M && M->n_levels >= 1 && M->n_levels <= GCL_MAX_LEVELS && M->n_maps >= 0 && M->n_maps <= GCL_MAX_MAPS,
                "gcl_plan: bad maps descriptor");
  for (size_t i = 0; i < P.ops.size(); ++i) {
    const gcl_plan_op& op = P.ops[i];
    GCL_CHECK_ARG(op.level_in < M->n_levels && op.level_out < M->n_levels, "gcl_plan: record %d uses a level the maps lack", (int)i);
    if (op.kind == GCL_OP_CONVBN || op.kind == GCL_OP_CONV) {
      GCL_CHECK_ARG(op.map >= 0 && op.map < M->n_maps, "gcl_plan: record %d names map %d of %d", (int)i, op.map, M->n_maps);
      const gcl_map_desc& m = M->maps[op.map];
      GCL_CHECK_ARG(m.K == op.K, "gcl_plan: record %d expects K = %d, map %d has %d", (int)i, op.K, op.map, m.K);
      const int lin = op.transpose ? m.level_out : m.level_in, lout = op.transpose ? m.level_in : m.level_out;
      GCL_CHECK_ARG(lin == op.level_in && lout == op.level_out, "gcl_plan: record %d and map %d disagree on the levels", (int)i, op.map);
    }
  }
  return GCL_OK;
}

}  // namespace gcl

using namespace gcl;

extern "C" {

// Dry run of a pass -- the forward pass of inference, the forward and the whole backward pass of training -- with P's maps and
// parameters as they stand: *need = the arena bytes it takes.  P.A comes back as it was.  Training with a.bn NULL: nobody reads them
static int dry_pass(Plan& P, FwdArgs a, long long* need) {
  std::vector<void*> nulls(2 * (P.n_bn > 0 ? P.n_bn : 1), nullptr), gn(P.n_params, nullptr);
  if (!a.eval && !a.bn) a.bn = nulls.data();
  const Arena real = P.A;
  P.A = Arena{DRY_BASE, 0, 0, true};      // (nothing is profiled in a dry run: ProfScope)
  float* y = nullptr;
  int rc = plan_forward(P, a, &y, nullptr);
  if (rc == GCL_OK && !a.eval) rc = plan_backward(P, (const float*)DRY_BASE, gn.data(), 0, (int)P.ops.size(), nullptr);
  *need = P.A.off;
  P.A = real;
  P.relu_masked.clear();      // (a run that stopped early leaves no ReLU flagged as applied)
  return rc;
}

// Binds the plan to a pass (maps, parameters, state buffer, the fp32-twins setting) and sizes it by a dry run: *need.
// With an arena the pass is about to be enqueued: the maps are copied -- the backward pass runs after the caller may have
// released its descriptor -- and the pass must fit, so that nothing is launched into an arena that cannot hold it
static int bind_pass(Plan& P, const char* who, const gcl_maps_desc* maps, void* const* params, void* state, void* arena,
                     long long arena_bytes, const FwdArgs& a, long long* need) {
  int rc = check_maps(P, maps);
  if (rc) return rc;
  P.maps = maps;
  if (arena) {
    P.maps_copy = *maps;
    P.maps = &P.maps_copy;
    P.A = Arena{(char*)arena, arena_bytes, 0, false};
  }
  if (params) P.params.assign(params, params + P.n_params);
  else P.params.assign(P.n_params, nullptr);
  P.state = state;
  P.forward_done = false;
  P.keep_twins = P.keep_fp32;      // parked with the pass: its backward pass follows the sizing made here
  if ((rc = dry_pass(P, a, need))) return rc;
  if (arena && *need > arena_bytes) {
    set_error("%s: arena too small (%lld bytes needed, %lld given)", who, *need, arena_bytes);
    return GCL_ERR_ARENA;
  }
  return GCL_OK;
}

// behind a pass that was enqueued: it stayed inside its arena and inside its amax slot pool (new_slot)
static int check_pass(const Plan& P, const char* who) {
  if (!P.A.fits()) {
    set_error("%s: arena overrun", who);
    return GCL_ERR_ARENA;
  }
  GCL_CHECK_ARG(!P.slots_exhausted, "%s: amax slot pool exhausted", who);
  return GCL_OK;
}

// A forward pass waits for its backward pass in a slot of P.passes, under its arena: park moves the pass being enqueued
// there, unpark brings it back
static void park(Plan& P, PassState* slot) {
  *slot = std::move(static_cast<PassState&>(P));
  slot->maps = &slot->maps_copy;
  static_cast<PassState&>(P) = PassState();
}
static void unpark(Plan& P, PassState* slot) {
  static_cast<PassState&>(P) = std::move(*slot);
  P.maps = &P.maps_copy;
}

int64_t gcl_maps_arena_bytes(int64_t n, const gcl_map_spec* specs_host, int32_t n_specs, int32_t n_levels) {
  if (n <= 0 || !specs_host || n_specs < 0 || n_specs > GCL_MAX_MAPS || n_levels < 1 || n_levels > GCL_MAX_LEVELS) return -1;
  Arena A{DRY_BASE, 0, 0, true};
  gcl_maps_desc d;
  if (maps_build(nullptr, n, specs_host, n_specs, n_levels, A, nullptr, &d, nullptr) != GCL_OK) return -1;
  return A.off + 4096;
}

int gcl_maps_build_split(const int32_t* coords, int64_t n, const gcl_map_spec* specs_host, int32_t n_specs, int32_t n_levels,
                         void* arena, int64_t arena_bytes, void* pinned_host, gcl_maps_desc* out_host, void* stream,
                         void* side_stream) {
  GCL_CHECK_ARG(coords && specs_host && arena && pinned_host && out_host, "gcl_maps_build: null pointer");
  GCL_CHECK_ARG(side_stream != stream || !side_stream, "gcl_maps_build_split: the side stream must differ from the stream");
  GCL_CHECK_ARG(n > 0, "gcl_maps_build: empty SparseTensor");
  GCL_CHECK_ARG(n_specs >= 0 && n_specs <= GCL_MAX_MAPS && n_levels >= 1 && n_levels <= GCL_MAX_LEVELS,
                "gcl_maps_build: at most %d maps and %d levels", GCL_MAX_MAPS, GCL_MAX_LEVELS);
  // read-back area (int32): row 0 = input status + per-level meta, row s + 1 = the pair counts of map s; 128 words per row
  // size check BEFORE the first launch (the dry run's upper bound -- every level as large as the input -- is what
  // gcl_maps_arena_bytes tells callers to reserve): a short arena must not be written past its end
  const int64_t need = gcl_maps_arena_bytes(n, specs_host, n_specs, n_levels);
  GCL_CHECK_ARG(need >= 0, "gcl_maps_build: bad map specification");
  if (arena_bytes < need) {
    set_error("gcl_maps_build: arena too small (%lld bytes needed, %lld given)", (long long)need, (long long)arena_bytes);
    return GCL_ERR_ARENA;
  }
  Arena A{(char*)arena, arena_bytes, 0, false};
  return maps_build(coords, n, specs_host, n_specs, n_levels, A, (int32_t*)pinned_host, out_host, (hipStream_t)stream,
                    (hipStream_t)side_stream);
}

int gcl_maps_build(const int32_t* coords, int64_t n, const gcl_map_spec* specs_host, int32_t n_specs, int32_t n_levels,
                   void* arena, int64_t arena_bytes, void* pinned_host, gcl_maps_desc* out_host, void* stream) {
  return gcl_maps_build_split(coords, n, specs_host, n_specs, n_levels, arena, arena_bytes, pinned_host, out_host, stream, nullptr);
}

void* gcl_plan_create(const gcl_plan_op* ops_host, int32_t n_ops, int32_t n_tensors, int32_t n_params,
                      const int32_t* weight_order_host, int32_t n_weights, int32_t presplit_min_c) {
  if (!ops_host || n_ops <= 0 || n_tensors <= 1 || n_params <= 0 || n_weights < 0 || (n_weights && !weight_order_host)) {
    set_error("gcl_plan_create: bad argument");
    return nullptr;
  }
  Plan* P = new (std::nothrow) Plan();
  if (!P) {
    set_error("gcl_plan_create: out of host memory");
    return nullptr;
  }
  P->ops.assign(ops_host, ops_host + n_ops);
  P->n_tensors = n_tensors;
  P->n_params = n_params;
  P->presplit = presplit_min_c > 0 ? presplit_min_c : 128;
  P->worder.assign(weight_order_host, weight_order_host + n_weights);
  P->widx.assign(n_params, -1);
  P->made.assign(n_tensors, 0);
  for (std::vector<long long>* v : {&P->wK, &P->wcin, &P->wcout, &P->off_fwd, &P->off_bwd}) v->assign((size_t)n_weights, 0);
  P->wmode.assign((size_t)n_weights, 0);
  if (validate_records(*P) != GCL_OK || weight_tables(*P) != GCL_OK) {      // (each has set its own error text)
    delete P;
    return nullptr;
  }
  analyse_graph(*P);
  return P;
}

void gcl_plan_destroy(void* plan) {
  Plan* P = (Plan*)plan;
  if (!P) return;
  for (ProfRec& r : P->prof) {
    (void)hipEventDestroy(r.e0);
    (void)hipEventDestroy(r.e1);
  }
  for (PassState* q : P->passes) delete q;
  for (hipEvent_t e : P->events) (void)hipEventDestroy(e);
  delete P;
}

int64_t gcl_plan_state_bytes(const void* plan) {
  if (!plan) return -1;
  return state_words(*(const Plan*)plan) * 8 + 256;
}

static int64_t sized_pass(void* plan, const char* who, const gcl_maps_desc* maps_host, bool eval) {
  long long need = 0;
  if (!plan || bind_pass(*(Plan*)plan, who, maps_host, nullptr, DRY_BASE, nullptr, 0, FwdArgs{nullptr, eval, nullptr, true}, &need))
    return -1;
  return need + 4096;
}

int64_t gcl_plan_arena_bytes(void* plan, const gcl_maps_desc* maps_host) {
  return sized_pass(plan, "gcl_plan_arena_bytes", maps_host, false);
}

int gcl_plan_forward(void* plan, const gcl_maps_desc* maps_host, const float* x, void* const* params_host,
                     void* const* bn_stats_host, void* state, void* arena, int64_t arena_bytes, float** y_out_host,
                     void* stream) {
  Plan* P = (Plan*)plan;
  GCL_CHECK_ARG(P && maps_host && x && params_host && bn_stats_host && state && arena && y_out_host, "gcl_plan_forward: null pointer");
  const FwdArgs a{x, false, bn_stats_host, true};
  long long need = 0;      // (both passes)
  int rc = bind_pass(*P, "gcl_plan_forward", maps_host, params_host, state, arena, arena_bytes, a, &need);
  if (rc) return rc;
  // a list handed over before the pass: the touched-row suffix runs on its rows in this pass too, under the rules of the
  // backward pass -- a suffix, shapes the row-stream weight gradient takes, 2 cap < n_rows, and room in the arena for both
  // passes (the same calls, counted)
  const int n_ops = (int)P->ops.size();
  P->suffix_fwd_rows_used = 0;
  if (P->touched && P->touched_cap > 0 && P->suffix_first < n_ops && P->suffix_rows_ok && P->ops.back().cout % 4 == 0 &&
      2 * P->touched_cap < maps_host->n_rows[P->ops[P->suffix_first].level_in]) {
    P->fwd_rows = P->touched;
    P->fwd_cap = P->touched_cap;
    if (dry_pass(*P, a, &need) != GCL_OK || need > arena_bytes) {
      P->fwd_rows = nullptr;
      P->fwd_cap = 0;
    }
  }
  rc = plan_forward(*P, a, y_out_host, (hipStream_t)stream);
  if (rc == GCL_OK) rc = check_pass(*P, "gcl_plan_forward");
  P->forward_done = rc == GCL_OK;
  if (rc != GCL_OK) {
    P->fwd_rows = nullptr;
    P->fwd_cap = 0;
    return rc;
  }
  if (P->fwd_cap > 0) {      // the list is parked with the pass; its backward pass needs no second one
    P->suffix_fwd_rows_used = P->fwd_cap;
    P->touched = nullptr;
    P->touched_cap = 0;
  }
  // park the pass under its arena until gcl_plan_backward / gcl_plan_release asks for it
  PassState* slot = nullptr;
  for (PassState* q : P->passes)
    if (!q->forward_done || q->key == arena) slot = q;
  if (!slot) {
    slot = new (std::nothrow) PassState();
    GCL_CHECK_ARG(slot, "gcl_plan_forward: out of host memory");
    P->passes.push_back(slot);
  }
  P->key = arena;
  park(*P, slot);
  return GCL_OK;
}

int64_t gcl_plan_eval_state_bytes(const void* plan) {
  if (!plan) return -1;
  const Plan& P = *(const Plan*)plan;
  return ((state_words(P) * 8 + 255) & ~255ll) + (((long long)P.worder.size() * GCL_AMAX_WORDS * 4 + 255) & ~255ll) +
         P.bytes_fwd + 256;
}

int64_t gcl_plan_eval_arena_bytes(void* plan, const gcl_maps_desc* maps_host) {
  return sized_pass(plan, "gcl_plan_eval_arena_bytes", maps_host, true);
}

int gcl_plan_forward_eval(void* plan, const gcl_maps_desc* maps_host, const float* x, void* const* params_host,
                          void* const* bn_eval_host, int32_t repack, void* state, void* arena, int64_t arena_bytes,
                          float** y_out_host, void* stream) {
  Plan* P = (Plan*)plan;
  GCL_CHECK_ARG(P && maps_host && x && params_host && bn_eval_host && state && arena && y_out_host,
                "gcl_plan_forward_eval: null pointer");
  const FwdArgs a{x, true, bn_eval_host, repack != 0};
  long long need = 0;
  int rc = bind_pass(*P, "gcl_plan_forward_eval", maps_host, params_host, state, arena, arena_bytes, a, &need);
  if (rc == GCL_OK) rc = plan_forward(*P, a, y_out_host, (hipStream_t)stream);
  if (rc == GCL_OK) rc = check_pass(*P, "gcl_plan_forward_eval");
  static_cast<PassState&>(*P) = PassState();      // nothing waits for a backward pass
  return rc;
}

int gcl_plan_release(void* plan, void* arena) {
  Plan* P = (Plan*)plan;
  GCL_CHECK_ARG(P, "gcl_plan_release: null plan");
  bool found = false;
  for (PassState* q : P->passes)
    if (q->forward_done && q->key == arena) found = true;
  // the forward pass forked packs / max|W| onto the aux stream; they are joined at the head of gcl_plan_backward, which
  // never comes for this pass.  The caller frees the arena to the MAIN stream's allocator next: drain the aux stream
  // first (rare path -- a training-mode pass under no_grad, or an output dropped without backward)
  if (found && P->aux && P->aux_dirty) {
    GCL_CHECK_HIP(hipStreamSynchronize(P->aux));
    P->aux_dirty = false;
  }
  for (PassState* q : P->passes)
    if (q->forward_done && q->key == arena) *q = PassState();
  return GCL_OK;
}

int gcl_plan_backward(void* plan, void* arena, const float* dy, void* const* grads_host, int32_t first_op,
                      int32_t last_op, void* stream) {
  Plan* P = (Plan*)plan;
  GCL_CHECK_ARG(P, "gcl_plan_backward: null pointer");
  const int32_t* rows = P->touched;      // the list is good for this call only
  const long long cap = P->touched_cap;
  P->touched = nullptr;
  P->touched_cap = 0;
  GCL_CHECK_ARG(grads_host, "gcl_plan_backward: null pointer");
  PassState* slot = nullptr;
  for (PassState* q : P->passes)
    if (q->forward_done && q->key == arena) slot = q;
  GCL_CHECK_ARG(slot, "gcl_plan_backward: no forward pass to differentiate in this arena");
  GCL_CHECK_ARG(first_op >= 0 && first_op < last_op && last_op <= (int)P->ops.size(), "gcl_plan_backward: bad record range");
  GCL_CHECK_ARG(last_op != (int)P->ops.size() || dy, "gcl_plan_backward: the last segment needs dy");
  if (slot->fwd_cap > 0) {      // the forward pass ran the suffix on its own list: dense operands do not exist
    GCL_CHECK_ARG(!rows || (rows == slot->fwd_rows && cap == slot->fwd_cap),
                  "gcl_plan_backward: the forward pass of this arena ran the touched-row suffix on another list");
    GCL_CHECK_ARG(last_op <= P->suffix_first || (first_op <= P->suffix_first && last_op == (int)P->ops.size()),
                  "gcl_plan_backward: the record range [%d, %d) cuts the touched-row suffix [%d, %d), which the forward pass "
                  "ran on the rows of a list: there are no dense operands to fall back to",
                  (int)first_op, (int)last_op, P->suffix_first, (int)P->ops.size());
  }
  unpark(*P, slot);
  int rc = plan_backward(*P, dy, grads_host, first_op, last_op, (hipStream_t)stream, rows, cap);
  if (rc == GCL_OK) rc = check_pass(*P, "gcl_plan_backward");
  if (first_op == 0 || rc != GCL_OK) P->forward_done = false;      // the pass is finished (or broken): its slot is free again
  park(*P, slot);
  return rc;
}

int gcl_plan_set_aux_stream(void* plan, void* stream) {
  Plan* P = (Plan*)plan;
  GCL_CHECK_ARG(P, "gcl_plan_set_aux_stream: null plan");
  P->aux = (hipStream_t)stream;
  return GCL_OK;
}

int gcl_plan_set_keep_fp32(void* plan, int32_t keep) {
  Plan* P = (Plan*)plan;
  GCL_CHECK_ARG(P, "gcl_plan_set_keep_fp32: null plan");
  P->keep_fp32 = keep != 0;
  return GCL_OK;
}

int gcl_plan_plane_only(const void* plan, int32_t* flags_host, int32_t n_ops) {
  const Plan* P = (const Plan*)plan;
  GCL_CHECK_ARG(P && flags_host && n_ops == (int32_t)P->ops.size(), "gcl_plan_plane_only: flags_host must hold one word per record");
  int n = 0;
  for (int i = 0; i < n_ops; ++i) {
    flags_host[i] = P->keep_fp32 ? 0 : (P->po_fwd[i] ? 1 : 0) | (P->po_bwd[i] ? 2 : 0);
    n += (flags_host[i] & 1) + (flags_host[i] >> 1);
  }
  return n;
}

int gcl_plan_touched_suffix(const void* plan) {
  if (!plan) return -1;
  return ((const Plan*)plan)->suffix_first;
}

int gcl_gather_rows(const float* src, int32_t ld, int64_t n_src, const int32_t* rows, int64_t cap, int32_t c, float pad,
                    float* out, void* stream) {
  GCL_CHECK_ARG(src && rows && out && n_src > 0 && cap > 0 && c > 0 && ld >= c, "gcl_gather_rows: bad argument");
  const bool vec = c % 4 == 0 && ld % 4 == 0 && (((uintptr_t)src | (uintptr_t)out) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(k_gather_rows<float4>, dim3(grid_for(cap * c / 4)), dim3(256), 0, (hipStream_t)stream, src, ld,
                       (long long)n_src, (const int*)rows, (long long)cap, c / 4, pad, (float4*)out);
  else
    hipLaunchKernelGGL(k_gather_rows<float>, dim3(grid_for(cap * c)), dim3(256), 0, (hipStream_t)stream, src, ld,
                       (long long)n_src, (const int*)rows, (long long)cap, c, pad, out);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_scatter_rows(const float* src, const int32_t* rows, int64_t cap, int32_t c, int64_t n_dst, float* dst, int32_t ld,
                     void* stream) {
  GCL_CHECK_ARG(src && rows && dst && n_dst > 0 && cap > 0, "gcl_scatter_rows: bad argument");
  GCL_CHECK_ARG(c > 0 && c % 4 == 0 && ld >= c && ld % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0,
                "gcl_scatter_rows: channel count and row pitch must be multiples of 4, the tensors 16-byte aligned");
  hipLaunchKernelGGL(k_scatter_rows, dim3(grid_for(cap * c / 4)), dim3(256), 0, (hipStream_t)stream, (const float4*)src,
                     (const int*)rows, (long long)cap, c / 4, (long long)n_dst, dst, ld);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_scatter_add_rows(const float* src, int32_t src_ld, const int32_t* rows, int64_t cap, int32_t c, int64_t n_dst,
                         float* dst, int32_t ld, void* stream) {
  GCL_CHECK_ARG(src && rows && dst && n_dst > 0 && cap > 0, "gcl_scatter_add_rows: bad argument");
  GCL_CHECK_ARG(c > 0 && c % 4 == 0 && ld >= c && ld % 4 == 0 && src_ld >= c && src_ld % 4 == 0 &&
                    (((uintptr_t)src | (uintptr_t)dst) & 15) == 0,
                "gcl_scatter_add_rows: channel count and row pitches must be multiples of 4, the tensors 16-byte aligned");
  hipLaunchKernelGGL(k_scatter_add_rows, dim3(grid_for(cap * c / 4)), dim3(256), 0, (hipStream_t)stream, src, src_ld,
                     (const int*)rows, (long long)cap, c / 4, (long long)n_dst, dst, ld);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_row_slots(const int32_t* rows, int64_t cap, int64_t n, int32_t* slots, void* stream) {
  GCL_CHECK_ARG(rows && slots && n > 0 && cap > 0 && cap < (1ll << 31), "gcl_row_slots: bad argument");
  GCL_CHECK_HIP(hipMemsetAsync(slots, 0xff, (size_t)n * sizeof(int32_t), (hipStream_t)stream));
  hipLaunchKernelGGL(k_row_slots, dim3((unsigned)cdiv(cap, 256)), dim3(256), 0, (hipStream_t)stream, (const int*)rows,
                     (long long)cap, (long long)n, slots);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int64_t gcl_plan_suffix_rows_used(const void* plan) {
  if (!plan) return -1;
  return ((const Plan*)plan)->suffix_rows_used;
}

int64_t gcl_plan_suffix_fwd_rows_used(const void* plan) {
  if (!plan) return -1;
  return ((const Plan*)plan)->suffix_fwd_rows_used;
}

int gcl_plan_set_touched_rows(void* plan, const int32_t* rows, int64_t cap) {
  Plan* P = (Plan*)plan;
  GCL_CHECK_ARG(P, "gcl_plan_set_touched_rows: null plan");
  GCL_CHECK_ARG((rows && cap > 0) || (!rows && cap == 0), "gcl_plan_set_touched_rows: a list needs a positive length");
  P->touched = rows;
  P->touched_cap = cap;
  return GCL_OK;
}

int64_t gcl_touched_rows_scratch_len(int64_t n_rows) { return n_rows > 0 ? gcl_scan_scratch_len(n_rows) : 0; }

int gcl_touched_rows(const int64_t* index, int64_t n_index, const int64_t* goff, int64_t n_groups, const int64_t* sel,
                     int32_t n_sel, const int64_t* rows_a, int32_t n_a, const int64_t* rows_b, int32_t n_b, int64_t n_rows,
                     int32_t* scratch, int32_t* rows, int64_t cap, int32_t* n_touched, void* stream) {
  GCL_CHECK_ARG(scratch && rows && n_touched && n_rows > 0 && n_rows < (1ll << 31) && cap > 0,
                "gcl_touched_rows: bad argument");
  GCL_CHECK_ARG(n_sel >= 0 && n_a >= 0 && n_b >= 0 && n_index >= 0 && n_groups >= 0, "gcl_touched_rows: negative count");
  GCL_CHECK_ARG(n_sel == 0 || (index && goff && sel), "gcl_touched_rows: group selections need index, goff and sel");
  GCL_CHECK_ARG((n_a == 0 || rows_a) && (n_b == 0 || rows_b), "gcl_touched_rows: null row array");
  hipStream_t st = (hipStream_t)stream;
  int32_t *flag = scratch, *pos = scratch + n_rows, *bs = scratch + 2 * n_rows;
  GCL_CHECK_HIP(hipMemsetAsync(flag, 0, (size_t)n_rows * sizeof(int32_t), st));
  if (n_sel)
    hipLaunchKernelGGL(k_touch_groups, dim3((unsigned)n_sel), dim3(64), 0, st, (const long long*)index, (long long)n_index,
                       (const long long*)goff, (long long)n_groups, (const long long*)sel, (long long)n_rows, flag);
  if (n_a)
    hipLaunchKernelGGL(k_touch_rows, dim3((unsigned)cdiv(n_a, 256)), dim3(256), 0, st, (const long long*)rows_a, (long long)n_a,
                       (long long)n_rows, flag);
  if (n_b)
    hipLaunchKernelGGL(k_touch_rows, dim3((unsigned)cdiv(n_b, 256)), dim3(256), 0, st, (const long long*)rows_b, (long long)n_b,
                       (long long)n_rows, flag);
  GCL_CHECK_LAUNCH();
  int rc = gcl_exclusive_scan_i32(flag, n_rows, pos, bs, stream);
  if (rc) return rc;
  const long long items = n_rows > cap ? n_rows : cap;
  hipLaunchKernelGGL(k_touch_emit, dim3((unsigned)cdiv(items, 256)), dim3(256), 0, st, (const int*)flag, (const int*)pos,
                     (long long)n_rows, rows, (long long)cap, n_touched);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

// A HIP stream restricted to a share of the chip's CUs (hipExtStreamCreateWithCUMask): the lowest `percent` % of the mask
// bits.  Experiment hook for the weight-gradient stream (GCL_AUX_CU_PCT, native.py): how much of the main chain's slowdown
// beside the weight gradients is bought back by giving them fewer CUs.
int gcl_stream_create_cu_share(int32_t percent, int32_t low_priority, void** stream_out) {
  GCL_CHECK_ARG(stream_out && percent >= 1 && percent <= 100, "gcl_stream_create_cu_share: percent must be 1..100");
  int dev = 0;
  hipDeviceProp_t prop;
  GCL_CHECK_HIP(hipGetDevice(&dev));
  GCL_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
  const int n_cu = prop.multiProcessorCount, words = (n_cu + 31) / 32;
  int on = (int)((long long)n_cu * percent / 100);
  if (on < 8) on = 8;
  std::vector<uint32_t> mask((size_t)words, 0u);
  for (int i = 0; i < on && i < n_cu; ++i) mask[(size_t)i >> 5] |= 1u << (i & 31);
  hipStream_t st = nullptr;
  GCL_CHECK_HIP(hipExtStreamCreateWithCUMask(&st, (uint32_t)words, mask.data()));
  (void)low_priority;      // hipExtStreamCreateWithCUMask has no priority argument
  *stream_out = (void*)st;
  return GCL_OK;
}

int gcl_stream_destroy(void* stream) {
  if (stream) GCL_CHECK_HIP(hipStreamDestroy((hipStream_t)stream));
  return GCL_OK;
}

int gcl_plan_profile(void* plan, int32_t enable) {
  Plan* P = (Plan*)plan;
  GCL_CHECK_ARG(P, "gcl_plan_profile: null plan");
  P->profile = enable != 0;
  return GCL_OK;
}

int gcl_plan_profile_read(void* plan, double* records_host, int32_t max_records) {
  Plan* P = (Plan*)plan;
  if (!P || !records_host) return GCL_ERR_ARG;
  int n = 0;
  for (size_t i = 0; i < P->prof_used && n < max_records; ++i) {
    const ProfRec& r = P->prof[i];
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) continue;
    double* o = records_host + 8 * n++;
    o[0] = r.kind; o[1] = ms; o[2] = r.pairs; o[3] = r.cin; o[4] = r.cout; o[5] = r.n_in; o[6] = r.n_out; o[7] = r.K;
  }
  return n;
}

}  // extern "C"
