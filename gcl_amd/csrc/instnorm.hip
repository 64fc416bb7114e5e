// InstanceNorm over the rows of [n, c]: every cloud of a batch normalised on its own (model/common.py:7-8,
// ME.MinkowskiInstanceNorm), all clouds in a fixed number of launches, rows in any order, fused with the residual add and
// ReLU like the BatchNorm of norm.hip.
//
// A cloud is a list of rows: cloud b owns rows[seg_off[b] .. seg_off[b + 1]) (rows == NULL: the positions themselves, the
// clouds are contiguous), in the order the rows have in the tensor; row_cloud[r] is the cloud of row r.  A batch index
// without rows is an empty cloud: no workgroup reads or writes anything for it.
//
// SUMMATION ORDER.  On one cloud the statistics passes are the arithmetic of norm.hip's k_bn_reduce / bn_reduce_partials /
// reduce_runs / k_bn_stats_final / k_bn_bwd_final run on that cloud alone -- restated here (those helpers are local to
// their file), and kept equal bit for bit by tests/test_gpu_instnorm.py:
//   * cloud b is cut into chunks of in_rows_per_wg(rows_b, c) of its rows (1024 halved down to 64 until there are 1024
//     chunks), one workgroup per chunk; thread t -> channel quad t % (c/4), row lane t / (c/4); a thread adds its rows in
//     ascending order into fp64 sums; the row lanes of a quad are added in order through LDS;
//   * the chunk sums of a cloud are two channel-major runs [2][c][chunks_b] at chunk_off[b] * 2 c of the scratch;
//   * one workgroup per (cloud, channel) adds a run: thread t elements t, t + 256, ... in four chains, then the fixed
//     16 x 16 tree; the conversions to fp32 are k_bn_stats_final's / k_bn_bwd_final's.
// Nothing depends on timing and no floating-point atomic is used: the same bits on every run.
//
// LAUNCHES (forward and backward alike): k_in_prep (one workgroup: the prefix chunk_off of the clouds' chunk counts and
// 1 / rows_b), k_in_reduce (cdiv(n, 64) + n_clouds workgroups, an upper bound of the chunk total known without reading
// seg_off on the host since no chunk is smaller than 64 rows; each finds its (cloud, chunk) in chunk_off, the surplus
// exits), k_in_final (c x n_clouds workgroups) and one grid-stride apply pass over all n c / 4 quads that fetches
// mean / rstd / sum_g / sum_gx / inv_n of a quad's row through row_cloud ([n_clouds, c] tables: they stay in L2).
//
// inv_n is 1.0f / (float)rows_b computed on the DEVICE where gcl_bn_bwd_apply computes 1.0f / (float)n on the host: the
// two agree because hipcc's default fp32 divide is correctly rounded (no fast-math, no approximate-divide flag here).
//
// The element expressions are bn_fwd_one's and bn_bwd_one's with the roundings of the BatchNorm kernels written out (fp
// contraction is off in them and every fused multiply-add is explicit): in k_bn_bwd_apply the products w rs and sum_g / n
// are loop invariants rounded on their own, here they vary per row and the compiler would otherwise fuse them differently.
#include "common.h"

namespace gcl {
namespace {

__host__ __device__ inline int in_rows_per_wg(long long n, int c) {      // norm.hip: bn_rows_per_wg
  int rows = 1024;
  while (rows > 64 && n / rows < 1024) rows >>= 1;
  (void)c;
  return rows;
}
__host__ __device__ inline long long in_chunks(long long rows, int c) {
  const int per = in_rows_per_wg(rows, c);
  return rows > 0 ? (rows + per - 1) / per : 0;
}

bool in_c_ok(int c) { return c >= 4 && c % 4 == 0 && (256 % (c / 4)) == 0; }      // what gcl_bn_stats takes

// ReLU sign bits: element quad e of the WHOLE tensor -> bit (e & 63) of the four words mask[(e >> 6) * 4 + component]
__device__ __forceinline__ float4 in_mask_as_y(const unsigned long long* __restrict__ mask, long long e) {
  const unsigned long long* m = mask + (e >> 6) * 4;
  const int b = (int)(e & 63);
  return make_float4((float)((m[0] >> b) & 1), (float)((m[1] >> b) & 1), (float)((m[2] >> b) & 1),
                     (float)((m[3] >> b) & 1));
}
__device__ __forceinline__ void in_relu_gate(float4& g, const float4& yv) {
  g.x = yv.x > 0.f ? g.x : 0.f; g.y = yv.y > 0.f ? g.y : 0.f;
  g.z = yv.z > 0.f ? g.z : 0.f; g.w = yv.w > 0.f ? g.w : 0.f;
}

// reduce_runs of norm.hip: ordered sum of one channel's two runs of chunk sums.  Valid in thread 0.
__device__ __forceinline__ void in_reduce_runs(const double* __restrict__ p1, const double* __restrict__ p2, int n_part,
                                               double& s, double& ss) {
  __shared__ double red[2][256];
  __shared__ double red2[2][16];
  const int t = threadIdx.x;
  double a0 = 0, a1 = 0, a2 = 0, a3 = 0, b0 = 0, b1 = 0, b2 = 0, b3 = 0;
  int w = t;
  for (; w + 768 < n_part; w += 1024) {
    a0 += p1[w];
    a1 += p1[w + 256];
    a2 += p1[w + 512];
    a3 += p1[w + 768];
    b0 += p2[w];
    b1 += p2[w + 256];
    b2 += p2[w + 512];
    b3 += p2[w + 768];
  }
  for (; w < n_part; w += 256) {
    a0 += p1[w];
    b0 += p2[w];
  }
  red[0][t] = (a0 + a1) + (a2 + a3);
  red[1][t] = (b0 + b1) + (b2 + b3);
  __syncthreads();
  if (t < 32) {      // lanes 0..15: the sums' 16 groups, lanes 16..31: the second run's
    const int which = t >> 4, g = t & 15;
    double u = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) u += red[which][g * 16 + q];
    red2[which][g] = u;
  }
  __syncthreads();
  s = 0;
  ss = 0;
  if (t == 0) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      s += red2[0][q];
      ss += red2[1][q];
    }
  }
}

__device__ __forceinline__ void in_publish_amax(float m, int* amax_bits) {      // norm.hip: publish_amax
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  __shared__ float wm[4];
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    amax_slot_publish(amax_bits, __float_as_int(fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]))), blockIdx.x);
  }
}
// a row's cloud as an index into the [n_clouds, c] tables (an id outside them reads cloud 0's constants, not past the tables)
__device__ __forceinline__ long long in_cloud(int v, int n_clouds) { return (unsigned)v < (unsigned)n_clouds ? v : 0; }
__device__ __forceinline__ float in_amax4(float m, const float4& v) {
  return fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
}

}  // namespace

// chunk_off[b] = chunks of the clouds before b (chunk_off[n_clouds]: all), inv_n[b] = 1 / rows_b.  One workgroup: thread t
// takes a span of consecutive clouds, the 256 span sums are scanned by thread 0.
__global__ void __launch_bounds__(256) k_in_prep(const long long* __restrict__ seg_off, int n_clouds, int c,
                                                 long long* __restrict__ chunk_off, float* __restrict__ inv_n) {
  __shared__ long long part[256];
  const int t = threadIdx.x;
  const int per = (n_clouds + 255) / 256;
  const int b0 = min(t * per, n_clouds), b1 = min(b0 + per, n_clouds);
  long long s = 0;
  for (int b = b0; b < b1; ++b) s += in_chunks(seg_off[b + 1] - seg_off[b], c);
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    long long a = 0;
    for (int i = 0; i < 256; ++i) {
      const long long v = part[i];
      part[i] = a;
      a += v;
    }
    chunk_off[n_clouds] = a;
  }
  __syncthreads();
  long long a = part[t];
  for (int b = b0; b < b1; ++b) {
    const long long rows_b = seg_off[b + 1] - seg_off[b];
    chunk_off[b] = a;
    inv_n[b] = rows_b > 0 ? 1.0f / (float)rows_b : 0.f;      // correctly rounded: the value gcl_bn_bwd_apply gets from its host
    a += in_chunks(rows_b, c);
  }
}

// k_bn_reduce on the chunk this workgroup owns: thread t -> channel quad cq = t % (c/4), row lane rl = t / (c/4), its rows
// (positions rl, rl + rstep, ... of the chunk) ascending; four rows in flight (the row indices, then the rows)
template <bool BWD>
__global__ void __launch_bounds__(256) k_in_reduce(const float* __restrict__ x, const float* __restrict__ dy, long long n, int c,
                                                   const long long* __restrict__ seg_off, const int* __restrict__ rows,
                                                   int n_clouds, const long long* __restrict__ chunk_off,
                                                   const float* __restrict__ mean, const float* __restrict__ rstd,
                                                   const unsigned long long* __restrict__ mask,
                                                   double* __restrict__ partial) {
  __shared__ double red[2][256][4];
  const long long w = blockIdx.x;
  if (w >= chunk_off[n_clouds]) return;      // surplus workgroup
  int lo = 0, hi = n_clouds;                 // chunk_off[lo] <= w < chunk_off[hi]; ends on the cloud that owns chunk w
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (chunk_off[mid] <= w) lo = mid; else hi = mid;
  }
  const int b = lo;
  const long long first = seg_off[b], rows_b = seg_off[b + 1] - first;
  // a table that does not describe n rows (or more chunks than the grid and the scratch were sized for): touch nothing
  if (first < 0 || rows_b <= 0 || first + rows_b > n || chunk_off[b + 1] > (long long)gridDim.x) return;
  const int per = in_rows_per_wg(rows_b, c);
  const long long nwg = chunk_off[b + 1] - chunk_off[b], k = w - chunk_off[b];
  const long long r_begin = k * per;
  long long r_end = r_begin + per;
  if (r_end > rows_b) r_end = rows_b;
  const int cq_n = c >> 2;
  const int cq = threadIdx.x % cq_n, rl = threadIdx.x / cq_n, rstep = 256 / cq_n;
  double s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
  float4 mu = make_float4(0, 0, 0, 0), rs = make_float4(1, 1, 1, 1);
  if (BWD) {
    mu = reinterpret_cast<const float4*>(mean + (long long)b * c)[cq];
    rs = reinterpret_cast<const float4*>(rstd + (long long)b * c)[cq];
  }
  const float4 z4 = make_float4(0, 0, 0, 0);
  for (long long r0 = r_begin + rl; r0 < r_end; r0 += 4 * rstep) {
    long long row[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long r = r0 + (long long)u * rstep;
      row[u] = r < r_end ? (rows ? (long long)rows[first + r] : first + r) : -1;
      if ((unsigned long long)row[u] >= (unsigned long long)n) row[u] = -1;      // not a row of x: adds nothing
    }
    float4 xv[4], gv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      xv[u] = gv[u] = z4;
      if (row[u] < 0) continue;
      xv[u] = reinterpret_cast<const float4*>(x + row[u] * c)[cq];
      if (BWD) gv[u] = reinterpret_cast<const float4*>(dy + row[u] * c)[cq];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (row[u] < 0) continue;
      const float4 v = xv[u];
      if (!BWD) {
        s0[0] += v.x; s0[1] += v.y; s0[2] += v.z; s0[3] += v.w;
        s1[0] += (double)v.x * v.x; s1[1] += (double)v.y * v.y;
        s1[2] += (double)v.z * v.z; s1[3] += (double)v.w * v.w;
      } else {
        float4 g = gv[u];
        if (mask) in_relu_gate(g, in_mask_as_y(mask, row[u] * cq_n + cq));
        s0[0] += g.x; s0[1] += g.y; s0[2] += g.z; s0[3] += g.w;
        s1[0] += (double)g.x * ((v.x - mu.x) * rs.x); s1[1] += (double)g.y * ((v.y - mu.y) * rs.y);
        s1[2] += (double)g.z * ((v.z - mu.z) * rs.z); s1[3] += (double)g.w * ((v.w - mu.w) * rs.w);
      }
    }
  }
  // bn_reduce_partials: the row lanes of a channel quad in order -> entry k of the cloud's channel-major runs
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    red[0][threadIdx.x][j] = s0[j];
    red[1][threadIdx.x][j] = s1[j];
  }
  __syncthreads();
  if (rl == 0) {
    double* p = partial + chunk_off[b] * 2 * c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double a = 0, d = 0;
      for (int q = 0; q < rstep; ++q) {
        a += red[0][q * cq_n + cq][j];
        d += red[1][q * cq_n + cq][j];
      }
      p[(long long)(cq * 4 + j) * nwg + k] = a;
      p[(long long)(c + cq * 4 + j) * nwg + k] = d;
    }
  }
}

// one workgroup per (channel, cloud).  !BWD: out0 / out1 = mean / rstd (k_bn_stats_final), BWD: sum_g / sum_gx (k_bn_bwd_final)
template <bool BWD>
__global__ void __launch_bounds__(256) k_in_final(const double* __restrict__ partial, const long long* __restrict__ seg_off,
                                                  const long long* __restrict__ chunk_off, int c, float eps,
                                                  float* __restrict__ out0, float* __restrict__ out1) {
#pragma clang fp contract(off)
  const int ch = blockIdx.x, b = blockIdx.y;
  const long long n = seg_off[b + 1] - seg_off[b];
  if (n <= 0) return;      // empty cloud
  const int nwg = (int)(chunk_off[b + 1] - chunk_off[b]);
  const double* p = partial + chunk_off[b] * 2 * c;
  double s, ss;
  in_reduce_runs(p + (long long)ch * nwg, p + ((long long)c + ch) * nwg, nwg, s, ss);
  if (threadIdx.x != 0) return;
  const long long o = (long long)b * c + ch;
  if (!BWD) {
    double m = s / (double)n;
    double var = __builtin_fma(-m, m, ss / (double)n);      // ss / n - m * m as k_bn_stats_final rounds it
    if (var < 0) var = 0;
    out0[o] = (float)m;
    out1[o] = (float)(1.0 / sqrt(var + (double)eps));
  } else {
    out0[o] = (float)s;
    out1[o] = (float)ss;
  }
}

// Both apply kernels: thread -> element quads e, e + S, e + 2S, ... with S = gridDim.x * 256, a multiple of c / 4 (c / 4
// divides 256), so a thread's channel quad never changes and its row advances by S / (c/4): weight / bias are loaded once,
// the per-cloud constants per quad through row_cloud.  Two quads in flight per thread.
struct InFwdC { float4 mu, rs; };
__device__ __forceinline__ float4 in_fwd_one(const float4& xv, const float4& rv, bool has_res, int relu, const InFwdC& k,
                                             const float4& wv, const float4& bv) {
#pragma clang fp contract(off)
  float4 o;      // bn_fwd_one: (x - mu) * rs * w + b, the last two fused
  o.x = __builtin_fmaf((xv.x - k.mu.x) * k.rs.x, wv.x, bv.x);
  o.y = __builtin_fmaf((xv.y - k.mu.y) * k.rs.y, wv.y, bv.y);
  o.z = __builtin_fmaf((xv.z - k.mu.z) * k.rs.z, wv.z, bv.z);
  o.w = __builtin_fmaf((xv.w - k.mu.w) * k.rs.w, wv.w, bv.w);
  if (has_res) { o.x += rv.x; o.y += rv.y; o.z += rv.z; o.w += rv.w; }
  if (relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
  return o;
}
__device__ __forceinline__ void in_mask_store(unsigned long long* __restrict__ mask, long long e, const float4& o, bool ok) {
  // e - lane is a multiple of 64 (grid stride and block size are): one ballot per component
  unsigned long long b0 = __ballot(ok && o.x > 0.f), b1 = __ballot(ok && o.y > 0.f), b2 = __ballot(ok && o.z > 0.f),
                     b3 = __ballot(ok && o.w > 0.f);
  if (ok && (threadIdx.x & 63) == 0) {
    unsigned long long* m = mask + (e >> 6) * 4;
    m[0] = b0; m[1] = b1; m[2] = b2; m[3] = b3;
  }
}

__global__ void __launch_bounds__(256) k_in_apply(const float* __restrict__ x, long long total4, int c,
                                                  const int* __restrict__ row_cloud, const float* __restrict__ mean,
                                                  const float* __restrict__ rstd, const float* __restrict__ weight,
                                                  const float* __restrict__ bias, const float* __restrict__ residual,
                                                  int relu, float* __restrict__ y, unsigned long long* __restrict__ mask,
                                                  int* amax_bits, int n_clouds) {
  const int cq_n = c >> 2;
  const long long S = (long long)gridDim.x * blockDim.x;
  const long long e0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long rstep = S / cq_n;
  long long row_e = e0 / cq_n;
  const int q0 = (int)(e0 % cq_n);
  const float4 wv = reinterpret_cast<const float4*>(weight)[q0], bv = reinterpret_cast<const float4*>(bias)[q0];
  const float4 z4 = make_float4(0, 0, 0, 0);
  float am = 0.f;
  // wave-uniform trip count (e - lane is the same for the wave's lanes; the ballots need the whole wave)
  for (long long e = e0; e - (threadIdx.x & 63) < total4; e += 2 * S) {
    const long long f = e + S;
    const bool oka = e < total4, okb = f < total4;
    const long long ca = oka ? in_cloud(row_cloud[row_e], n_clouds) : 0, cb = okb ? in_cloud(row_cloud[row_e + rstep], n_clouds) : 0;
    float4 xa = z4, xb = z4, ra = z4, rb = z4;
    if (oka) xa = reinterpret_cast<const float4*>(x)[e];
    if (okb) xb = reinterpret_cast<const float4*>(x)[f];
    if (residual) {
      if (oka) ra = reinterpret_cast<const float4*>(residual)[e];
      if (okb) rb = reinterpret_cast<const float4*>(residual)[f];
    }
    InFwdC ka, kb;
    ka.mu = reinterpret_cast<const float4*>(mean)[ca * cq_n + q0]; ka.rs = reinterpret_cast<const float4*>(rstd)[ca * cq_n + q0];
    kb.mu = reinterpret_cast<const float4*>(mean)[cb * cq_n + q0]; kb.rs = reinterpret_cast<const float4*>(rstd)[cb * cq_n + q0];
    const float4 oa = in_fwd_one(xa, ra, residual != nullptr, relu, ka, wv, bv);
    const float4 ob = in_fwd_one(xb, rb, residual != nullptr, relu, kb, wv, bv);
    if (oka) { reinterpret_cast<float4*>(y)[e] = oa; am = in_amax4(am, oa); }
    if (okb) { reinterpret_cast<float4*>(y)[f] = ob; am = in_amax4(am, ob); }
    row_e += 2 * rstep;
    if (mask) {
      in_mask_store(mask, e, oa, oka);
      if (f - (threadIdx.x & 63) < total4) in_mask_store(mask, f, ob, okb);
    }
  }
  if (amax_bits) in_publish_amax(am, amax_bits);
}

struct InBwdC { float4 mu, rs, sg, sx; float inv_n; };
__device__ __forceinline__ InBwdC in_bwd_c(const float* mean, const float* rstd, const float* sum_g, const float* sum_gx,
                                           const float* inv_n, long long cloud, int cq_n, int q0) {
  InBwdC k;
  const long long o = cloud * cq_n + q0;
  k.mu = reinterpret_cast<const float4*>(mean)[o]; k.rs = reinterpret_cast<const float4*>(rstd)[o];
  k.sg = reinterpret_cast<const float4*>(sum_g)[o]; k.sx = reinterpret_cast<const float4*>(sum_gx)[o];
  k.inv_n = inv_n[cloud];
  return k;
}
// bn_bwd_one: w rs (g - sum_g / n - xhat sum_gx / n) with k_bn_bwd_apply's roundings: w rs and sum_g / n rounded on their own
// (loop invariants there), the xhat term subtracted by one fused multiply-add
__device__ __forceinline__ float in_bwd_1(float x, float g, float w, float mu, float rs, float sg, float sx, float inv_n) {
#pragma clang fp contract(off)
  const float t = g - sg * inv_n;
  const float p = (x - mu) * rs * sx;
  return (w * rs) * __builtin_fmaf(-inv_n, p, t);
}
__device__ __forceinline__ float4 in_bwd_one(const float4& xv, const float4& g, const float4& wv, const InBwdC& k) {
  float4 o;
  o.x = in_bwd_1(xv.x, g.x, wv.x, k.mu.x, k.rs.x, k.sg.x, k.sx.x, k.inv_n);
  o.y = in_bwd_1(xv.y, g.y, wv.y, k.mu.y, k.rs.y, k.sg.y, k.sx.y, k.inv_n);
  o.z = in_bwd_1(xv.z, g.z, wv.z, k.mu.z, k.rs.z, k.sg.z, k.sx.z, k.inv_n);
  o.w = in_bwd_1(xv.w, g.w, wv.w, k.mu.w, k.rs.w, k.sg.w, k.sx.w, k.inv_n);
  return o;
}

__global__ void __launch_bounds__(256) k_in_bwd_apply(const float* __restrict__ x, const float* __restrict__ dy,
                                                      long long total4, int c, const int* __restrict__ row_cloud,
                                                      const float* __restrict__ inv_n, const float* __restrict__ mean,
                                                      const float* __restrict__ rstd, const float* __restrict__ weight,
                                                      const float* __restrict__ sum_g, const float* __restrict__ sum_gx,
                                                      const unsigned long long* __restrict__ mask,
                                                      float* __restrict__ dx, float* __restrict__ dres, int* amax_bits,
                                                      int n_clouds) {
  const int cq_n = c >> 2;
  const long long S = (long long)gridDim.x * blockDim.x;
  const long long e0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long rstep = S / cq_n;
  long long row_e = e0 / cq_n;
  const int q0 = (int)(e0 % cq_n);
  const float4 wv = reinterpret_cast<const float4*>(weight)[q0];
  const float4 z4 = make_float4(0, 0, 0, 0);
  float am = 0.f;
  for (long long e = e0; e < total4; e += 2 * S) {
    const long long f = e + S;
    const bool okb = f < total4;
    const long long ca = in_cloud(row_cloud[row_e], n_clouds), cb = okb ? in_cloud(row_cloud[row_e + rstep], n_clouds) : ca;
    float4 xa = reinterpret_cast<const float4*>(x)[e], ga = reinterpret_cast<const float4*>(dy)[e];
    float4 xb = z4, gb = z4;
    if (okb) {
      xb = reinterpret_cast<const float4*>(x)[f];
      gb = reinterpret_cast<const float4*>(dy)[f];
    }
    const InBwdC ka = in_bwd_c(mean, rstd, sum_g, sum_gx, inv_n, ca, cq_n, q0);
    const InBwdC kb = in_bwd_c(mean, rstd, sum_g, sum_gx, inv_n, cb, cq_n, q0);
    row_e += 2 * rstep;
    if (mask) {
      in_relu_gate(ga, in_mask_as_y(mask, e));
      if (okb) in_relu_gate(gb, in_mask_as_y(mask, f));
    }
    const float4 oa = in_bwd_one(xa, ga, wv, ka);
    reinterpret_cast<float4*>(dx)[e] = oa;
    am = in_amax4(am, oa);
    if (dres) reinterpret_cast<float4*>(dres)[e] = ga;
    if (okb) {
      const float4 ob = in_bwd_one(xb, gb, wv, kb);
      reinterpret_cast<float4*>(dx)[f] = ob;
      am = in_amax4(am, ob);
      if (dres) reinterpret_cast<float4*>(dres)[f] = gb;
    }
  }
  if (amax_bits) in_publish_amax(am, amax_bits);
}

namespace {

constexpr int IN_MAX_CLOUDS = 65535;      // the grid's y extent; a packed coordinate holds no larger batch index either

struct InScratch {      // the scratch of one call: the chunk sums, then chunk_off [n_clouds + 1], then inv_n [n_clouds]
  double* partial;
  long long* chunk_off;
  float* inv_n;
  unsigned grid;        // workgroups of the statistics pass
};
InScratch in_scratch(double* scratch, int64_t n, int32_t n_clouds, int32_t c) {
  const int64_t wgs = cdiv(n, 64) + n_clouds;
  InScratch s;
  s.partial = scratch;
  s.chunk_off = reinterpret_cast<long long*>(scratch + wgs * 2 * c);
  s.inv_n = reinterpret_cast<float*>(s.chunk_off + n_clouds + 1);
  s.grid = (unsigned)wgs;
  return s;
}
unsigned in_apply_grid(long long total4) {
  long long g = cdiv(total4, 256);
  return (unsigned)(g > 4096 ? 4096 : g);
}

}  // namespace
}  // namespace gcl

using namespace gcl;

extern "C" {

int64_t gcl_in_scratch_len(int64_t n, int32_t n_clouds, int32_t c) {
  if (n <= 0 || n_clouds < 1 || c < 1) return 0;
  return (cdiv(n, 64) + n_clouds) * 2 * c + (n_clouds + 1) + (n_clouds + 1) / 2;
}

int gcl_in_fwd(const float* x, int64_t n, int32_t c, const int64_t* seg_off, const int32_t* rows, const int32_t* row_cloud,
               int32_t n_clouds, float eps, const float* weight, const float* bias, const float* residual, int32_t relu,
               double* scratch, float* mean, float* rstd, float* y, uint64_t* relu_mask, int32_t* y_amax, void* stream) {
  GCL_CHECK_ARG(x && seg_off && row_cloud && weight && bias && scratch && mean && rstd && y, "gcl_in_fwd: null pointer");
  GCL_CHECK_ARG(n > 0 && n <= 0x7fffffffll && in_c_ok(c), "gcl_in_fwd: unsupported shape n=%lld c=%d (c/4 must divide 256)",
                (long long)n, c);
  GCL_CHECK_ARG(n_clouds >= 1 && n_clouds <= IN_MAX_CLOUDS, "gcl_in_fwd: n_clouds=%d outside 1 .. %d", n_clouds, IN_MAX_CLOUDS);
  GCL_CHECK_ARG(!relu || relu_mask, "gcl_in_fwd: relu_mask is required when relu is set");
  hipStream_t st = (hipStream_t)stream;
  const InScratch s = in_scratch(scratch, n, n_clouds, c);
  const long long* so = (const long long*)seg_off;
  hipLaunchKernelGGL(k_in_prep, dim3(1), dim3(256), 0, st, so, n_clouds, c, s.chunk_off, s.inv_n);
  hipLaunchKernelGGL(k_in_reduce<false>, dim3(s.grid), dim3(256), 0, st, x, (const float*)nullptr, (long long)n, c, so,
                     (const int*)rows, n_clouds, (const long long*)s.chunk_off, (const float*)nullptr, (const float*)nullptr,
                     (const unsigned long long*)nullptr, s.partial);
  hipLaunchKernelGGL(k_in_final<false>, dim3((unsigned)c, (unsigned)n_clouds), dim3(256), 0, st, (const double*)s.partial, so,
                     (const long long*)s.chunk_off, c, eps, mean, rstd);
  const long long total4 = n * (c / 4);
  hipLaunchKernelGGL(k_in_apply, dim3(in_apply_grid(total4)), dim3(256), 0, st, x, total4, c, (const int*)row_cloud,
                     (const float*)mean, (const float*)rstd, weight, bias, residual, relu, y,
                     (unsigned long long*)(relu ? relu_mask : nullptr), (int*)y_amax, n_clouds);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_in_bwd(const float* x, const float* dy, int64_t n, int32_t c, const int64_t* seg_off, const int32_t* rows,
               const int32_t* row_cloud, int32_t n_clouds, const float* mean, const float* rstd, const float* weight,
               int32_t relu, const uint64_t* relu_mask, double* scratch, float* sum_g, float* sum_gx, float* dx, float* dres,
               int32_t* dx_amax, void* stream) {
  GCL_CHECK_ARG(x && dy && seg_off && row_cloud && mean && rstd && weight && scratch && sum_g && sum_gx && dx,
                "gcl_in_bwd: null pointer");
  GCL_CHECK_ARG(n > 0 && n <= 0x7fffffffll && in_c_ok(c), "gcl_in_bwd: unsupported shape n=%lld c=%d (c/4 must divide 256)",
                (long long)n, c);
  GCL_CHECK_ARG(n_clouds >= 1 && n_clouds <= IN_MAX_CLOUDS, "gcl_in_bwd: n_clouds=%d outside 1 .. %d", n_clouds, IN_MAX_CLOUDS);
  GCL_CHECK_ARG(!relu || relu_mask, "gcl_in_bwd: relu_mask is required when relu is set");
  hipStream_t st = (hipStream_t)stream;
  const InScratch s = in_scratch(scratch, n, n_clouds, c);
  const long long* so = (const long long*)seg_off;
  const unsigned long long* mask = (const unsigned long long*)(relu ? relu_mask : nullptr);
  hipLaunchKernelGGL(k_in_prep, dim3(1), dim3(256), 0, st, so, n_clouds, c, s.chunk_off, s.inv_n);
  hipLaunchKernelGGL(k_in_reduce<true>, dim3(s.grid), dim3(256), 0, st, x, dy, (long long)n, c, so, (const int*)rows, n_clouds,
                     (const long long*)s.chunk_off, mean, rstd, mask, s.partial);
  hipLaunchKernelGGL(k_in_final<true>, dim3((unsigned)c, (unsigned)n_clouds), dim3(256), 0, st, (const double*)s.partial, so,
                     (const long long*)s.chunk_off, c, 0.f, sum_g, sum_gx);
  const long long total4 = n * (c / 4);
  hipLaunchKernelGGL(k_in_bwd_apply, dim3(in_apply_grid(total4)), dim3(256), 0, st, x, dy, total4, c, (const int*)row_cloud,
                     (const float*)s.inv_n, mean, rstd, weight, (const float*)sum_g, (const float*)sum_gx, mask, dx, dres,
                     (int*)dx_amax, n_clouds);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

}  // extern "C"
