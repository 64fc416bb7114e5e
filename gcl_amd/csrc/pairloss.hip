// Pair-trainer losses (fp32): positional-key mask, triplet terms, contrastive pair terms.
//
// Reference: lib/trainer.py:198-212 (generate_rand_negative_pairs), :253-273 (contrastive loss with random negatives),
// :545-592 (triplet_loss), :671-744 (hardest triplet_loss), util/misc.py:43-55 (_hash).  The reference evaluates each of
// these losses as 25 - 40 small torch launches around a device -> host copy of the arg-minima and np.isin on the CPU;
// here the membership test is one hash-table probe on the device, every term of a loss is one launch and its mean a
// second one (one workgroup, fp64 sums in a fixed tree: the value does not depend on the launch), and the backward pass
// is one launch of float atomics into caller-zeroed buffers, like every other loss backward of this library -- or, through
// the *_emit entries, the same kernel writing contribution records for gcl_ordered_row_sum (losssink.h, ordered.hip).
//
// Layout of a row in a wave: a feature row of C <= 16 / 32 / 64 channels takes a quarter / half / whole wave (lane =
// channel inside its sub-wave), so a wave works on 4 / 2 / 1 triplets at a time and the atomic instruction of the
// backward pass covers whole 64 / 128-byte row segments.  Distances keep the (a - b)^2 form of lib/metrics.py:22-25.
#include "common.h"
#include "losssink.h"

#include <limits.h>
#include <math.h>

namespace gcl {

__device__ __forceinline__ float sub_sum(float v, int width) {      // sum over the `width` lanes of a sub-wave
  for (int o = width >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ bool row_ok(long long r, long long n) { return r >= 0 && r < n; }

// ---- positional-key mask: key(r0, r1) = r0 + r1 * seed (util/misc.py:43-55), wrapping int64 like numpy -----------------
__global__ void k_pk_fill(Slot* t, long long cap) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cap) {
    t[i].key = EMPTY_KEY;
    t[i].val = 0;
  }
}

__global__ void k_pk_insert(const long long* __restrict__ pos, long long n_pos, unsigned long long seed, Slot* t,
                            long long cap) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pos) return;
  table_insert(t, cap, (unsigned long long)pos[2 * i] + (unsigned long long)pos[2 * i + 1] * seed);
}

// candidate t: (ap[t][0], ap[t][1]) when b is NULL; else the row of column `col` of ap[t] paired with rb = b[arg[t]]
// (arg NULL: b[t]) on the other side.  keep[t] = the candidate's key is not a positive pair's; b_out[t] = rb.
__global__ void k_pk_probe(const long long* __restrict__ ap, int col, const long long* __restrict__ b,
                           const int* __restrict__ arg, long long nb, int m, unsigned long long seed,
                           const Slot* __restrict__ t, long long cap, long long* __restrict__ b_out,
                           unsigned char* __restrict__ keep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  long long r0 = ap[2 * (long long)i], r1 = ap[2 * (long long)i + 1];
  if (b) {
    const long long j = arg ? (long long)arg[i] : (long long)i;
    const bool ok = j >= 0 && j < nb;
    const long long rb = ok ? b[j] : -1;
    if (b_out) b_out[i] = rb;
    if (!ok) {                      // an arg-minimum outside the candidate list: dropped, never dereferenced
      keep[i] = 0;
      return;
    }
    if (col == 0) r1 = rb; else r0 = rb;
  }
  const unsigned long long key = (unsigned long long)r0 + (unsigned long long)r1 * seed;
  keep[i] = table_find(t, cap, key) < 0 ? 1 : 0;
}

// ---- triplet terms --------------------------------------------------------------------------------------------------
// Triplet t: the positive pair ap[t] = (row of F0, row of F1), the negative row neg[t], tag[t] = side | set << 1.
//   side 0: anchor = F0[ap[t][0]], positive = F1[ap[t][1]], negative = F1[neg[t]]
//   side 1: anchor = F1[ap[t][1]], positive = F0[ap[t][0]], negative = F0[neg[t]]
// work = float [3 m]: term, d_pos, d_neg.  A triplet with a row outside its cloud gets term -1 (dropped everywhere).
struct TripletRows {
  const float *fa, *fo;      // anchor's cloud, the other cloud
  long long ra, rp, rn;
  bool valid;
};

__device__ __forceinline__ TripletRows triplet_rows(const float* f0, long long n0, const float* f1, long long n1,
                                                    const long long* __restrict__ ap, const long long* __restrict__ neg,
                                                    const unsigned char* __restrict__ tag, long long t) {
  TripletRows r;
  const long long i0 = ap[2 * t], i1 = ap[2 * t + 1];
  const int side = tag[t] & 1;
  r.fa = side ? f1 : f0;
  r.fo = side ? f0 : f1;
  r.ra = side ? i1 : i0;
  r.rp = side ? i0 : i1;
  r.rn = neg[t];
  const long long na = side ? n1 : n0, no = side ? n0 : n1;
  r.valid = row_ok(r.ra, na) && row_ok(r.rp, no) && row_ok(r.rn, no);
  return r;
}

template <int W>
__global__ void __launch_bounds__(256) k_triplet_terms(const float* __restrict__ f0, long long n0,
                                                       const float* __restrict__ f1, long long n1, int c,
                                                       const long long* __restrict__ ap, const long long* __restrict__ neg,
                                                       const unsigned char* __restrict__ tag, int m, float margin,
                                                       float* __restrict__ work) {
  constexpr int R = 64 / W;
  const int lane = threadIdx.x & 63, sub = lane / W, ch = lane % W, wave = threadIdx.x >> 6;
  const long long t = ((long long)blockIdx.x * 4 + wave) * R + sub;
  const bool live = t < m;
  float a = 0.f, p = 0.f, n = 0.f;
  bool valid = false;
  if (live) {
    const TripletRows r = triplet_rows(f0, n0, f1, n1, ap, neg, tag, t);
    valid = r.valid;
    if (valid && ch < c) {
      a = r.fa[r.ra * c + ch];
      p = r.fo[r.rp * c + ch];
      n = r.fo[r.rn * c + ch];
    }
  }
  const float dp2 = sub_sum((a - p) * (a - p), W), dn2 = sub_sum((a - n) * (a - n), W);     // every lane takes part
  if (live && ch == 0) {
    const float dpos = sqrtf(dp2 + 1e-7f), dneg = sqrtf(dn2 + 1e-7f);
    const float v = dpos + margin - dneg;
    work[t] = valid ? (v != v ? v : fmaxf(v, 0.f)) : -1.f;
    work[(long long)m + t] = dpos;
    work[2ll * m + t] = dneg;
  }
}

// out[0] = mean term over the kept triplets (0 / 0 = NaN, torch's mean of nothing), out[1] = their number, then for
// every set s = 0, 1, 2 at out[2 + 6 s]: {kept, all, mean d_pos kept, mean d_neg kept, mean d_pos all, mean d_neg all}.
constexpr int TRIPLET_OUT = 20;
__global__ void __launch_bounds__(256) k_triplet_reduce(const float* __restrict__ work,
                                                        const unsigned char* __restrict__ tag,
                                                        const unsigned char* __restrict__ keep, int m,
                                                        float* __restrict__ out) {
  __shared__ double red[256];
  __shared__ double tot[TRIPLET_OUT];
  const int tid = threadIdx.x;
  double acc[TRIPLET_OUT];
#pragma unroll
  for (int q = 0; q < TRIPLET_OUT; ++q) acc[q] = 0.0;
  for (int t = tid; t < m; t += 256) {
    const float term = work[t];
    const double dp = work[(long long)m + t], dn = work[2ll * m + t];
    const bool valid = !(term < 0.f);
    const bool k = valid && (!keep || keep[t]);
    const int s = min((int)(tag[t] >> 1), 2);
    if (k) {
      acc[0] += (double)term;
      acc[1] += 1.0;
    }
#pragma unroll
    for (int s2 = 0; s2 < 3; ++s2) {
      const bool in = valid && s == s2;
      acc[2 + 6 * s2] += (in && k) ? 1.0 : 0.0;
      acc[3 + 6 * s2] += in ? 1.0 : 0.0;
      acc[4 + 6 * s2] += (in && k) ? dp : 0.0;
      acc[5 + 6 * s2] += (in && k) ? dn : 0.0;
      acc[6 + 6 * s2] += in ? dp : 0.0;
      acc[7 + 6 * s2] += in ? dn : 0.0;
    }
  }
#pragma unroll
  for (int q = 0; q < TRIPLET_OUT; ++q) {
    red[tid] = acc[q];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) tot[q] = red[0];
    __syncthreads();
  }
  if (tid == 0) {
    out[0] = (float)(tot[0] / tot[1]);
    out[1] = (float)tot[1];
    for (int s = 0; s < 3; ++s) {
      const double* q = tot + 2 + 6 * s;
      float* o = out + 2 + 6 * s;
      o[0] = (float)q[0];
      o[1] = (float)q[1];
      o[2] = (float)(q[2] / q[0]);
      o[3] = (float)(q[3] / q[0]);
      o[4] = (float)(q[4] / q[1]);
      o[5] = (float)(q[5] / q[1]);
    }
  }
}

// SINK (losssink.h): float atomics into dF0 / dF1, or records.  TWO record lists, one per cloud, with the same slots
// 3 t (anchor), 3 t + 1 (positive), 3 t + 2 (negative): a contribution stands in the list of the cloud it goes to, and the
// slot of the other list keeps its -1.
template <int W, class SINK>
__global__ void __launch_bounds__(256) k_triplet_bwd(const float* __restrict__ f0, long long n0,
                                                     const float* __restrict__ f1, long long n1, int c,
                                                     const long long* __restrict__ ap, const long long* __restrict__ neg,
                                                     const unsigned char* __restrict__ tag,
                                                     const unsigned char* __restrict__ keep, int m,
                                                     const float* __restrict__ work, const float* __restrict__ out,
                                                     const float* __restrict__ g, SINK sink) {
  constexpr int R = 64 / W;
  const int lane = threadIdx.x & 63, sub = lane / W, ch = lane % W, wave = threadIdx.x >> 6;
  const long long t = ((long long)blockIdx.x * 4 + wave) * R + sub;
  if (t >= m || ch >= c) return;
  if (keep && !keep[t]) return;
  if (!(work[t] > 0.f)) return;                    // inactive hinge, or a dropped triplet (-1)
  const TripletRows r = triplet_rows(f0, n0, f1, n1, ap, neg, tag, t);
  if (!r.valid) return;
  const float gs = g[0] / out[1];
  const float a = r.fa[r.ra * c + ch], p = r.fo[r.rp * c + ch], n = r.fo[r.rn * c + ch];
  const float u = gs * (a - p) / work[(long long)m + t], v = gs * (a - n) / work[2ll * m + t];
  const int da = tag[t] & 1, d_o = da ^ 1;             // the anchor's cloud, the other cloud
  sink.put(da, 3 * t, r.ra, c, ch, u - v, false);
  sink.put(d_o, 3 * t + 1, r.rp, c, ch, -u, false);
  sink.put(d_o, 3 * t + 2, r.rn, c, ch, v, false);
}

// ---- pair terms -----------------------------------------------------------------------------------------------------
// Pair t = (row of F0, row of F1) = pairs[t]; d2 = |F0[a] - F1[b]|^2.  work = float [m]: d2 (-1: a row outside its cloud).
//   PT_SQ      d2                                  (lib/trainer.py:266)
//   PT_SQ_POS  relu(d2 - thresh)                   (:459)
//   PT_NEG     relu(thresh - sqrt(d2 + eps))^2     (:269-270 with eps 1e-4, :460-461 with eps 1e-7)
//   PT_DIST    sqrt(d2 + eps)                      (:573, a statistic: forward only)
constexpr int PT_SQ = 0, PT_SQ_POS = 1, PT_NEG = 2, PT_DIST = 3;

template <int W>
__global__ void __launch_bounds__(256) k_pair_d2(const float* __restrict__ f0, long long n0, const float* __restrict__ f1,
                                                 long long n1, int c, const long long* __restrict__ pairs, int m,
                                                 float* __restrict__ work) {
  constexpr int R = 64 / W;
  const int lane = threadIdx.x & 63, sub = lane / W, ch = lane % W, wave = threadIdx.x >> 6;
  const long long t = ((long long)blockIdx.x * 4 + wave) * R + sub;
  const bool live = t < m;
  float a = 0.f, b = 0.f;
  bool valid = false;
  if (live) {
    const long long ra = pairs[2 * t], rb = pairs[2 * t + 1];
    valid = row_ok(ra, n0) && row_ok(rb, n1);
    if (valid && ch < c) {
      a = f0[ra * c + ch];
      b = f1[rb * c + ch];
    }
  }
  const float d2 = sub_sum((a - b) * (a - b), W);
  if (live && ch == 0) work[t] = valid ? d2 : -1.f;
}

__device__ __forceinline__ float pair_term(float d2, int mode, float thresh, float eps) {
  if (mode == PT_SQ) return d2;
  if (mode == PT_SQ_POS) {
    const float v = d2 - thresh;
    return v != v ? v : fmaxf(v, 0.f);
  }
  const float D = sqrtf(d2 + eps);
  if (mode == PT_DIST) return D;
  const float h = thresh - D;
  return h != h ? h : fmaxf(h, 0.f) * fmaxf(h, 0.f);
}

// out[0] = mean term over the kept pairs (NaN for none), out[1] = their number
__global__ void __launch_bounds__(256) k_pair_reduce(const float* __restrict__ work, const unsigned char* __restrict__ keep,
                                                     int m, int mode, float thresh, float eps, float* __restrict__ out) {
  __shared__ double rs[256], rc[256];
  const int tid = threadIdx.x;
  double s = 0.0, cnt = 0.0;
  for (int t = tid; t < m; t += 256) {
    const float d2 = work[t];
    if (d2 < 0.f || (keep && !keep[t])) continue;
    s += (double)pair_term(d2, mode, thresh, eps);
    cnt += 1.0;
  }
  rs[tid] = s;
  rc[tid] = cnt;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      rs[tid] += rs[tid + o];
      rc[tid] += rc[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[0] = (float)(rs[0] / rc[0]);
    out[1] = (float)rc[0];
  }
}

// SINK: as k_triplet_bwd; slot t of list 0 (row of F0) and of list 1 (row of F1)
template <int W, class SINK>
__global__ void __launch_bounds__(256) k_pair_bwd(const float* __restrict__ f0, long long n0, const float* __restrict__ f1,
                                                  long long n1, int c, const long long* __restrict__ pairs,
                                                  const unsigned char* __restrict__ keep, int m, int mode, float thresh,
                                                  float eps, const float* __restrict__ work, const float* __restrict__ out,
                                                  const float* __restrict__ g, SINK sink) {
  constexpr int R = 64 / W;
  const int lane = threadIdx.x & 63, sub = lane / W, ch = lane % W, wave = threadIdx.x >> 6;
  const long long t = ((long long)blockIdx.x * 4 + wave) * R + sub;
  if (t >= m || ch >= c) return;
  if (keep && !keep[t]) return;
  const float d2 = work[t];
  if (d2 < 0.f) return;
  const long long ra = pairs[2 * t], rb = pairs[2 * t + 1];
  if (!row_ok(ra, n0) || !row_ok(rb, n1)) return;
  const float gs = g[0] / out[1];
  float coef;                                      // d term / d d2, times 2, times gs
  if (mode == PT_SQ) coef = 2.f * gs;
  else if (mode == PT_SQ_POS) coef = (d2 - thresh > 0.f) ? 2.f * gs : 0.f;
  else {
    const float D = sqrtf(d2 + eps), h = thresh - D;
    coef = (h > 0.f) ? -2.f * h / D * gs : 0.f;
  }
  if (coef == 0.f) return;
  const float diff = f0[ra * c + ch] - f1[rb * c + ch];
  sink.put(0, t, ra, c, ch, coef * diff, false);
  sink.put(1, t, rb, c, ch, -coef * diff, false);
}

static int sub_width(int c) { return c <= 16 ? 16 : (c <= 32 ? 32 : 64); }
static unsigned row_grid(int m, int w) { return (unsigned)cdiv(m, 4 * (64 / w)); }

}  // namespace gcl

using namespace gcl;

#define PL_DISPATCH(KERNEL, W, GRID, ST, ...)                                                       \
  do {                                                                                              \
    if ((W) == 16) hipLaunchKernelGGL(KERNEL<16>, dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);       \
    else if ((W) == 32) hipLaunchKernelGGL(KERNEL<32>, dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);  \
    else hipLaunchKernelGGL(KERNEL<64>, dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);                 \
  } while (0)
// the backward kernels: the sink is the second template argument
#define PL_DISPATCH_SINK(KERNEL, SINK, W, GRID, ST, ...)                                                       \
  do {                                                                                                         \
    if ((W) == 16) hipLaunchKernelGGL((KERNEL<16, SINK>), dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);          \
    else if ((W) == 32) hipLaunchKernelGGL((KERNEL<32, SINK>), dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);     \
    else hipLaunchKernelGGL((KERNEL<64, SINK>), dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);                    \
  } while (0)

extern "C" {

int gcl_pair_key_table(const int64_t* pos_pairs, int64_t n_pos, int64_t seed, int64_t* table, int64_t cap, void* stream) {
  GCL_CHECK_ARG(table && (pos_pairs || n_pos == 0), "gcl_pair_key_table: null pointer");
  GCL_CHECK_ARG(n_pos >= 0 && seed > 0, "gcl_pair_key_table: n_pos must be >= 0 and seed > 0");
  GCL_CHECK_ARG(cap >= 64 && cap >= 2 * n_pos && (cap & (cap - 1)) == 0,
                "gcl_pair_key_table: cap must be a power of two >= max(64, 2 n_pos)");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_pk_fill, dim3((unsigned)cdiv(cap, 256)), dim3(256), 0, st, (Slot*)table, (long long)cap);
  if (n_pos > 0)
    hipLaunchKernelGGL(k_pk_insert, dim3((unsigned)cdiv(n_pos, 256)), dim3(256), 0, st, (const long long*)pos_pairs,
                       (long long)n_pos, (unsigned long long)seed, (Slot*)table, (long long)cap);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_pair_key_mask(const int64_t* ap, int32_t col, const int64_t* b, const int32_t* b_arg, int64_t nb, int32_t m,
                      int64_t seed, const int64_t* table, int64_t cap, int64_t* b_out, uint8_t* keep, void* stream) {
  GCL_CHECK_ARG(m >= 0 && seed > 0, "gcl_pair_key_mask: m must be >= 0 and seed > 0");
  if (m == 0) return GCL_OK;
  GCL_CHECK_ARG(ap && table && keep, "gcl_pair_key_mask: null pointer");
  GCL_CHECK_ARG(col == 0 || col == 1, "gcl_pair_key_mask: col must be 0 or 1 (got %d)", col);
  GCL_CHECK_ARG(b || (!b_arg && !b_out), "gcl_pair_key_mask: b_arg / b_out need the candidate rows b");
  GCL_CHECK_ARG(!b || nb >= (b_arg ? 1 : (int64_t)m), "gcl_pair_key_mask: b holds fewer rows than the candidates need");
  GCL_CHECK_ARG(cap >= 64 && (cap & (cap - 1)) == 0, "gcl_pair_key_mask: cap must be a power of two >= 64");
  hipLaunchKernelGGL(k_pk_probe, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, (hipStream_t)stream, (const long long*)ap,
                     col, (const long long*)b, b_arg, (long long)nb, m, (unsigned long long)seed, (const Slot*)table,
                     (long long)cap, (long long*)b_out, keep);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int64_t gcl_triplet_scratch_len(int32_t m) { return m > 0 ? 3 * (int64_t)m : 0; }

int gcl_triplet_fwd(const float* f0, int64_t n0, const float* f1, int64_t n1, int32_t c, const int64_t* ap,
                    const int64_t* neg, const uint8_t* tag, const uint8_t* keep, int32_t m, float margin, float* work,
                    float* out, void* stream) {
  GCL_CHECK_ARG(out && m >= 0, "gcl_triplet_fwd: null output / negative m");
  GCL_CHECK_ARG(c >= 1 && c <= 64, "gcl_triplet_fwd: feature width must be <= 64 (got %d)", c);
  GCL_CHECK_ARG(m == 0 || (f0 && f1 && ap && neg && tag && work), "gcl_triplet_fwd: null pointer");
  GCL_CHECK_ARG(n0 >= 0 && n1 >= 0, "gcl_triplet_fwd: negative row count");
  hipStream_t st = (hipStream_t)stream;
  const int w = sub_width(c);
  if (m > 0)
    PL_DISPATCH(k_triplet_terms, w, row_grid(m, w), st, f0, (long long)n0, f1, (long long)n1, c, (const long long*)ap,
                (const long long*)neg, tag, m, margin, work);
  hipLaunchKernelGGL(k_triplet_reduce, dim3(1), dim3(256), 0, st, (const float*)work, tag, keep, m, out);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_triplet_bwd(const float* f0, int64_t n0, const float* f1, int64_t n1, int32_t c, const int64_t* ap,
                    const int64_t* neg, const uint8_t* tag, const uint8_t* keep, int32_t m, const float* work,
                    const float* out, const float* g, float* df0, float* df1, void* stream) {
  GCL_CHECK_ARG(m >= 0, "gcl_triplet_bwd: negative m");
  GCL_CHECK_ARG(c >= 1 && c <= 64, "gcl_triplet_bwd: feature width must be <= 64 (got %d)", c);
  if (m == 0) return GCL_OK;
  GCL_CHECK_ARG(f0 && f1 && ap && neg && tag && work && out && g && df0 && df1, "gcl_triplet_bwd: null pointer");
  GCL_CHECK_ARG(n0 >= 0 && n1 >= 0, "gcl_triplet_bwd: negative row count");
  const int w = sub_width(c);
  const AtomicSink sink{{df0, df1}};
  PL_DISPATCH_SINK(k_triplet_bwd, AtomicSink, w, row_grid(m, w), (hipStream_t)stream, f0, (long long)n0, f1, (long long)n1,
                   c, (const long long*)ap, (const long long*)neg, tag, keep, m, work, out, g, sink);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int64_t gcl_triplet_records(int32_t m) { return m > 0 ? 3 * (int64_t)m : 0; }

int gcl_triplet_bwd_emit(const float* f0, int64_t n0, const float* f1, int64_t n1, int32_t c, const int64_t* ap,
                         const int64_t* neg, const uint8_t* tag, const uint8_t* keep, int32_t m, const float* work,
                         const float* out, const float* g, int32_t* rec_row0, float* rec_val0, int32_t* rec_row1,
                         float* rec_val1, int32_t n_rec, void* stream) {
  GCL_CHECK_ARG(m >= 0 && n_rec >= 0, "gcl_triplet_bwd_emit: negative count (m = %d, n_rec = %d)", m, n_rec);
  GCL_CHECK_ARG(c >= 1 && c <= 64, "gcl_triplet_bwd_emit: feature width must lie in 1 .. 64 (got %d)", c);
  GCL_CHECK_ARG(n_rec >= 3 * (int64_t)m, "gcl_triplet_bwd_emit: n_rec = %d is below gcl_triplet_records(m) = 3 m", n_rec);
  GCL_CHECK_ARG(n_rec == 0 || (rec_row0 && rec_val0 && rec_row1 && rec_val1),
                "gcl_triplet_bwd_emit: null pointer (the record lists)");
  GCL_CHECK_ARG(m == 0 || (f0 && f1 && ap && neg && tag && work && out && g), "gcl_triplet_bwd_emit: null pointer");
  GCL_CHECK_ARG(n0 >= 0 && n1 >= 0 && n0 <= INT_MAX && n1 <= INT_MAX,
                "gcl_triplet_bwd_emit: row counts must lie in 0 .. 2^31 - 1 (record rows are int32)");
  hipStream_t st = (hipStream_t)stream;
  rec_fill(rec_row0, n_rec, st);
  rec_fill(rec_row1, n_rec, st);
  if (m > 0) {
    const int w = sub_width(c);
    const RecordSink sink{{rec_row0, rec_row1}, {rec_val0, rec_val1}, (long long)n_rec};
    PL_DISPATCH_SINK(k_triplet_bwd, RecordSink, w, row_grid(m, w), st, f0, (long long)n0, f1, (long long)n1, c,
                     (const long long*)ap, (const long long*)neg, tag, keep, m, work, out, g, sink);
  }
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int64_t gcl_pair_terms_scratch_len(int32_t m) { return m > 0 ? (int64_t)m : 0; }

int gcl_pair_terms_fwd(const float* f0, int64_t n0, const float* f1, int64_t n1, int32_t c, const int64_t* pairs,
                       const uint8_t* keep, int32_t m, int32_t mode, float thresh, float eps, float* work, float* out,
                       void* stream) {
  GCL_CHECK_ARG(out && m >= 0, "gcl_pair_terms_fwd: null output / negative m");
  GCL_CHECK_ARG(c >= 1 && c <= 64, "gcl_pair_terms_fwd: feature width must be <= 64 (got %d)", c);
  GCL_CHECK_ARG(mode >= PT_SQ && mode <= PT_DIST, "gcl_pair_terms_fwd: unknown mode %d", mode);
  GCL_CHECK_ARG(m == 0 || (f0 && f1 && pairs && work), "gcl_pair_terms_fwd: null pointer");
  GCL_CHECK_ARG(n0 >= 0 && n1 >= 0 && eps >= 0.f, "gcl_pair_terms_fwd: negative row count / eps");
  hipStream_t st = (hipStream_t)stream;
  const int w = sub_width(c);
  if (m > 0)
    PL_DISPATCH(k_pair_d2, w, row_grid(m, w), st, f0, (long long)n0, f1, (long long)n1, c, (const long long*)pairs, m,
                work);
  hipLaunchKernelGGL(k_pair_reduce, dim3(1), dim3(256), 0, st, (const float*)work, keep, m, mode, thresh, eps, out);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_pair_terms_bwd(const float* f0, int64_t n0, const float* f1, int64_t n1, int32_t c, const int64_t* pairs,
                       const uint8_t* keep, int32_t m, int32_t mode, float thresh, float eps, const float* work,
                       const float* out, const float* g, float* df0, float* df1, void* stream) {
  GCL_CHECK_ARG(m >= 0, "gcl_pair_terms_bwd: negative m");
  GCL_CHECK_ARG(c >= 1 && c <= 64, "gcl_pair_terms_bwd: feature width must be <= 64 (got %d)", c);
  GCL_CHECK_ARG(mode >= PT_SQ && mode < PT_DIST, "gcl_pair_terms_bwd: mode %d has no backward pass", mode);
  if (m == 0) return GCL_OK;
  GCL_CHECK_ARG(f0 && f1 && pairs && work && out && g && df0 && df1, "gcl_pair_terms_bwd: null pointer");
  GCL_CHECK_ARG(n0 >= 0 && n1 >= 0 && eps >= 0.f, "gcl_pair_terms_bwd: negative row count / eps");
  const int w = sub_width(c);
  const AtomicSink sink{{df0, df1}};
  PL_DISPATCH_SINK(k_pair_bwd, AtomicSink, w, row_grid(m, w), (hipStream_t)stream, f0, (long long)n0, f1, (long long)n1, c,
                   (const long long*)pairs, keep, m, mode, thresh, eps, work, out, g, sink);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int64_t gcl_pair_terms_records(int32_t m) { return m > 0 ? (int64_t)m : 0; }

int gcl_pair_terms_bwd_emit(const float* f0, int64_t n0, const float* f1, int64_t n1, int32_t c, const int64_t* pairs,
                            const uint8_t* keep, int32_t m, int32_t mode, float thresh, float eps, const float* work,
                            const float* out, const float* g, int32_t* rec_row0, float* rec_val0, int32_t* rec_row1,
                            float* rec_val1, int32_t n_rec, void* stream) {
  GCL_CHECK_ARG(m >= 0 && n_rec >= 0, "gcl_pair_terms_bwd_emit: negative count (m = %d, n_rec = %d)", m, n_rec);
  GCL_CHECK_ARG(c >= 1 && c <= 64, "gcl_pair_terms_bwd_emit: feature width must lie in 1 .. 64 (got %d)", c);
  GCL_CHECK_ARG(mode >= PT_SQ && mode < PT_DIST, "gcl_pair_terms_bwd_emit: mode %d has no backward pass", mode);
  GCL_CHECK_ARG(n_rec >= (int64_t)m, "gcl_pair_terms_bwd_emit: n_rec = %d is below gcl_pair_terms_records(m) = m", n_rec);
  GCL_CHECK_ARG(n_rec == 0 || (rec_row0 && rec_val0 && rec_row1 && rec_val1),
                "gcl_pair_terms_bwd_emit: null pointer (the record lists)");
  GCL_CHECK_ARG(m == 0 || (f0 && f1 && pairs && work && out && g), "gcl_pair_terms_bwd_emit: null pointer");
  GCL_CHECK_ARG(n0 >= 0 && n1 >= 0 && n0 <= INT_MAX && n1 <= INT_MAX && eps >= 0.f,
                "gcl_pair_terms_bwd_emit: row counts must lie in 0 .. 2^31 - 1 (record rows are int32), eps >= 0");
  hipStream_t st = (hipStream_t)stream;
  rec_fill(rec_row0, n_rec, st);
  rec_fill(rec_row1, n_rec, st);
  if (m > 0) {
    const int w = sub_width(c);
    const RecordSink sink{{rec_row0, rec_row1}, {rec_val0, rec_val1}, (long long)n_rec};
    PL_DISPATCH_SINK(k_pair_bwd, RecordSink, w, row_grid(m, w), st, f0, (long long)n0, f1, (long long)n1, c,
                     (const long long*)pairs, keep, m, mode, thresh, eps, work, out, g, sink);
  }
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

}  // extern "C"
