// Feature-matching RANSAC registration on the device: open3d's registration_ransac_based_on_feature_matching on a set of
// putative correspondences (scripts/test_kitti.py:171-178, generalization_ETH/evaluate.py:171-186), restated for gfx950.
//
// open3d draws its minimal samples from std::mt19937 inside an OpenMP loop; here hypothesis h is a pure function of
// (seed, h) -- a splitmix64 counter generator -- so that the run is reproducible and an oracle can enumerate exactly the
// hypotheses the kernels draw (tests/ransac_oracle.py).  Per hypothesis, in open3d's order:
//   1. draw ransac_n correspondence indices (a repeated index rejects the hypothesis: status -3),
//   2. CorrespondenceCheckerBasedOnEdgeLength on the sample, before any pose (status -1),
//   3. TransformationEstimationPointToPoint(false) on the sample: centroids and H in fp64, kabsch_from_H, fp32 [R | t],
//   4. CorrespondenceCheckerBasedOnDistance on the sample (status -2),
//   5. EvaluateRANSACBasedOnCorrespondence over all n correspondences: inlier count and sum of squared inlier distances.
// The winner is the hypothesis of the highest count, then the lower sum, then the lower h (IsBetterRANSACThan + a total order).
//
// Hypotheses are processed in chunks of consecutive ids.  Steps 1-2 reject ~ 90-95 % of a chunk and step 4 some of the
// rest (the random samples whose edge lengths happen to agree), so every expensive stage runs on a COMPACTED list: the draw kernel leaves one ballot word per wave and one count per workgroup, k_rs_compact turns them into
// the ascending list of survivors (a workgroup's offset is the sum of the counts before it: no atomic append, the list does
// not depend on arrival order), the pose kernel runs the fp64 Jacobi with every lane busy and leaves the same kind of flags,
// and a second compaction lists what is scored.  Scoring takes one hypothesis per WAVE and one of RS_PARTS ranges of the
// correspondences per workgroup row: a lane sums the squared inlier distances of its correspondences in index order in fp64,
// the 64 sums meet in a butterfly, and k_rs_best adds the RS_PARTS partial sums in range order.  The ranges depend on n
// only, so a hypothesis' score is the same bits whatever the chunk length.  (One hypothesis per LANE over LDS-staged tiles,
// every lane reading the same address, was built and measured too: it needs thousands of scored hypotheses per chunk to
// fill the chip and won only when most samples are all-inlier ones -- 3.16 against 3.90 ms at an inlier share of 0.6, but
// 1.61 against 0.75 ms at 0.3 and 1.24 against 0.50 ms at 0.05, profiles/ransac_probe.txt -- and is not kept.)
// After every chunk k_rs_best updates the best hypothesis and, with 0 < confidence < 1, the id limit
// ceil(log(1 - confidence) / log(1 - (best count / n)^ransac_n)) in a control block on the device; the kernels of a later
// chunk that starts at or behind the limit return at once (status -4).  The host enqueues every chunk and never waits.
//
// A BATCH of pairs (gcl_ransac_register_batch) runs through the same kernels with the pair as the grid's z dimension: every
// pair has its own control block and its own slice of the scratch layout (`stride` bytes apart), and the launches of a chunk
// cover all pairs -- a registration is ~100 dependent launches of a few microseconds, so a batch costs the launches of one
// pair.  A pair's correspondence count and seed live in its control block (k_rs_init reads the count from the device,
// clamped to [0, n_cap]), so the pairs of a batch may have different lengths and nothing the host does depends on them; a
// pair with fewer than ransac_n correspondences starts with limit 0 and is skipped by every chunk.  One pair alone
// (gcl_ransac_register) is a batch of one: the same kernels, the same arithmetic, the same bits.
#include "common.h"
#include "kabsch.h"

#include <math.h>

#include <algorithm>

namespace gcl {

constexpr int RS_PARTS = 8;                 // correspondence ranges of the score (partials added in range order)
constexpr int RS_DEFAULT_CHUNK = 1 << 18;
constexpr int RS_MAX_CHUNK = 1 << 20;
constexpr int RS_MAX_N = 1 << 24;           // record indices 2 i + 1 stay far inside an int
constexpr int RS_SCORE_GRID = 1024;         // score workgroups per range at most, grid-stride above
constexpr long long RS_NO_LIMIT = 0x7fffffffffffffffll;
constexpr int RS_MAX_BATCH = 65535;         // the pair is blockIdx.z
constexpr int RS_SEED_GROUP = 32;           // seeds travel as kernel arguments, this many pairs per k_rs_init launch

struct RsCtrl {
  long long limit;        // a chunk whose first id is >= limit does nothing
  unsigned long long seed;
  int n, pad;             // the pair's correspondence count (rows from n on are never read); with limit and seed in the
                          // block's first 32 bytes: what every kernel reads first comes in one scalar load
  double best_sse;
  int best_h, best_count;
  int covered, scored;
  int n_a, n_b;           // survivors of steps 1-2 / of step 4 in the current chunk
  float best_T[12];
};
struct RsSeeds { unsigned long long s[RS_SEED_GROUP]; };

// pair `pair`'s copy of a scratch array (the slices are `stride` bytes apart) / of a [batch, row] output
template <class T>
__device__ __forceinline__ T* rs_at(T* p, int pair, size_t stride) {
  return reinterpret_cast<T*>(reinterpret_cast<size_t>(p) + (size_t)pair * stride);
}

__device__ __forceinline__ int rs_draw(unsigned long long seed, long long h, int j, int n) {
  unsigned long long z = seed + (unsigned long long)(4 * h + j + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (int)(((z >> 32) * (unsigned long long)n) >> 32);
}

// squared length of R s + t - t' in the difference form: the translation meets the target first, then one fma per column --
// every kernel that compares or sums this distance calls this one chain, so that they agree bit for bit
__device__ __forceinline__ float rs_resid2(const float* T, const float4& s, const float4& g) {
  const float x = __builtin_fmaf(T[0], s.x, __builtin_fmaf(T[1], s.y, __builtin_fmaf(T[2], s.z, T[3] - g.x)));
  const float y = __builtin_fmaf(T[4], s.x, __builtin_fmaf(T[5], s.y, __builtin_fmaf(T[6], s.z, T[7] - g.y)));
  const float z = __builtin_fmaf(T[8], s.x, __builtin_fmaf(T[9], s.y, __builtin_fmaf(T[10], s.z, T[11] - g.z)));
  return __builtin_fmaf(z, z, __builtin_fmaf(y, y, x * x));
}
__device__ __forceinline__ float rs_dist(const float4& a, const float4& b) {
  const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
  return sqrtf(__builtin_fmaf(dz, dz, __builtin_fmaf(dx, dx, dy * dy)));
}

// control block + the correspondences as 32-byte records {s, 0, t', 0}: two 16-byte loads per drawn sample, whole tiles
// (pairs pair0 .. pair0 + gridDim.z - 1; the count comes from n_dev when given: negative reads as 0, above n_cap as n_cap)
__global__ void __launch_bounds__(256) k_rs_init(const float* __restrict__ src, const float* __restrict__ tgt, int n_cap,
                                                 const int* __restrict__ n_dev, int ransac_n, int pair0, RsSeeds seeds,
                                                 float4* __restrict__ pk, RsCtrl* ctrl, size_t stride) {
  const int pair = pair0 + blockIdx.z;
  const int n = n_dev ? min(max(n_dev[pair], 0), n_cap) : n_cap;
  src += (size_t)pair * n_cap * 3;
  tgt += (size_t)pair * n_cap * 3;
  pk = rs_at(pk, pair, stride);
  ctrl = rs_at(ctrl, pair, stride);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    ctrl->n = n;
    ctrl->pad = 0;
    ctrl->seed = seeds.s[blockIdx.z];
    ctrl->limit = n < ransac_n ? 0 : RS_NO_LIMIT;      // too few correspondences: nothing is drawn, every chunk is skipped
    ctrl->best_sse = 0.0;
    ctrl->best_h = -1;
    ctrl->best_count = 0;
    ctrl->covered = ctrl->scored = 0;
    ctrl->n_a = ctrl->n_b = 0;
    for (int k = 0; k < 12; ++k) ctrl->best_T[k] = (k % 5 == 0) ? 1.f : 0.f;
  }
  if (i < n) {
    pk[2 * i] = make_float4(src[3 * i], src[3 * i + 1], src[3 * i + 2], 0.f);
    pk[2 * i + 1] = make_float4(tgt[3 * i], tgt[3 * i + 1], tgt[3 * i + 2], 0.f);
  }
}

// steps 1-2 for hypothesis h0 + (thread): ballot word per wave, survivor count per workgroup
template <int RN>
__global__ void __launch_bounds__(256) k_rs_draw(const RsCtrl* __restrict__ ctrl, long long h0, int m,
                                                 const float4* __restrict__ pk, float sim,
                                                 unsigned long long* __restrict__ mask, int* __restrict__ bcnt,
                                                 int* __restrict__ hyp_status, size_t stride, long long status_stride) {
  const int pair = blockIdx.z;
  ctrl = rs_at(ctrl, pair, stride);
  pk = rs_at(pk, pair, stride);
  mask = rs_at(mask, pair, stride);
  bcnt = rs_at(bcnt, pair, stride);
  if (hyp_status) hyp_status += (size_t)pair * status_stride;
  const int e = blockIdx.x * 256 + threadIdx.x;
  const bool live = e < m;
  const long long h = h0 + e;
  const long long limit = ctrl->limit;
  const int n = ctrl->n;
  const unsigned long long seed = ctrl->seed;
  if (h0 >= limit) {      // uniform over the pair
    if (hyp_status && live) hyp_status[h] = -4;
    return;
  }
  int status = 0;
  if (live) {
    int idx[RN];
#pragma unroll
    for (int j = 0; j < RN; ++j) idx[j] = rs_draw(seed, h, j, n);
#pragma unroll
    for (int a = 0; a < RN; ++a)
#pragma unroll
      for (int b = a + 1; b < RN; ++b)
        if (idx[a] == idx[b]) status = -3;
    if (status == 0 && sim > 0.f) {
      float4 s[RN], t[RN];
#pragma unroll
      for (int j = 0; j < RN; ++j) { s[j] = pk[2 * idx[j]]; t[j] = pk[2 * idx[j] + 1]; }
#pragma unroll
      for (int a = 0; a < RN; ++a)
#pragma unroll
        for (int b = a + 1; b < RN; ++b) {
          const float ds = rs_dist(s[a], s[b]), dt = rs_dist(t[a], t[b]);
          if (!(ds >= dt * sim && dt >= ds * sim)) status = -1;
        }
    }
    if (status != 0 && hyp_status) hyp_status[h] = status;
  }
  const bool pass = live && status == 0;
  const unsigned long long w = __ballot(pass);
  __shared__ int wc[4];
  if ((threadIdx.x & 63) == 0) {
    mask[blockIdx.x * 4 + (threadIdx.x >> 6)] = w;
    wc[threadIdx.x >> 6] = __popcll(w);
  }
  __syncthreads();
  if (threadIdx.x == 0) bcnt[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// ordered compaction of the flagged items 0 .. n_items - 1 (ballot words `mask`, per-workgroup counts `bcnt`): list[] holds
// them in ascending order, *n_out their number.  A workgroup's offset is the sum of the counts before it (integers: any
// order of summation), an item's place inside it the number of set bits before its own.  First pass: the m hypotheses of the
// chunk -> n_a; second: the n_a survivors -> n_b.
__global__ void __launch_bounds__(256) k_rs_compact(RsCtrl* ctrl, long long h0, int second, int m,
                                                    const unsigned long long* __restrict__ mask,
                                                    const int* __restrict__ bcnt, int* __restrict__ list, size_t stride) {
  const int pair = blockIdx.z;
  ctrl = rs_at(ctrl, pair, stride);
  mask = rs_at(mask, pair, stride);
  bcnt = rs_at(bcnt, pair, stride);
  list = rs_at(list, pair, stride);
  if (h0 >= ctrl->limit) return;
  const int n_items = second ? ctrl->n_a : m;
  int* n_out = second ? &ctrl->n_b : &ctrl->n_a;
  const int b = blockIdx.x, t = threadIdx.x;
  if (n_items == 0 && b == 0 && t == 0) *n_out = 0;
  if (b * 256 >= n_items) return;
  __shared__ int red[256];
  int part = 0;
  for (int q = t; q < b; q += 256) part += bcnt[q];
  red[t] = part;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  const int off = red[0];
  const int w = t >> 6, lane = t & 63;
  int before = 0;
  for (int q = 0; q < w; ++q) before += __popcll(mask[b * 4 + q]);
  const unsigned long long mw = mask[b * 4 + w];
  if ((mw >> lane) & 1ull) list[off + before + __popcll(mw & ((1ull << lane) - 1ull))] = b * 256 + t;
  if (t == 0 && (b + 1) * 256 >= n_items) *n_out = off + bcnt[b];
}

// steps 3-4 for survivor p of the first list (every lane holds one): pose to poses[p], flags of the second compaction
template <int RN>
__global__ void __launch_bounds__(256) k_rs_pose(const RsCtrl* __restrict__ ctrl, long long h0, const float4* __restrict__ pk,
                                                 float check2, const int* __restrict__ list_a,
                                                 float* __restrict__ poses, unsigned long long* __restrict__ mask,
                                                 int* __restrict__ bcnt, int* __restrict__ hyp_status, size_t stride,
                                                 long long status_stride) {
  const int pair = blockIdx.z;
  ctrl = rs_at(ctrl, pair, stride);
  pk = rs_at(pk, pair, stride);
  list_a = rs_at(list_a, pair, stride);
  poses = rs_at(poses, pair, stride);
  mask = rs_at(mask, pair, stride);
  bcnt = rs_at(bcnt, pair, stride);
  if (hyp_status) hyp_status += (size_t)pair * status_stride;
  if (h0 >= ctrl->limit) return;
  const int n_a = ctrl->n_a, n = ctrl->n;
  const unsigned long long seed = ctrl->seed;
  if ((int)blockIdx.x * 256 >= n_a) return;
  const int p = blockIdx.x * 256 + threadIdx.x;
  bool pass = false;
  if (p < n_a) {
    const long long h = h0 + list_a[p];
    float4 s[RN], t[RN];
    double ca[3] = {0, 0, 0}, cb[3] = {0, 0, 0};
#pragma unroll
    for (int j = 0; j < RN; ++j) {
      const int i = rs_draw(seed, h, j, n);
      s[j] = pk[2 * i];
      t[j] = pk[2 * i + 1];
      ca[0] += (double)s[j].x; ca[1] += (double)s[j].y; ca[2] += (double)s[j].z;
      cb[0] += (double)t[j].x; cb[1] += (double)t[j].y; cb[2] += (double)t[j].z;
    }
    for (int c = 0; c < 3; ++c) { ca[c] /= (double)RN; cb[c] /= (double)RN; }
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < RN; ++j) {
      const double a[3] = {(double)s[j].x - ca[0], (double)s[j].y - ca[1], (double)s[j].z - ca[2]};
      const double b[3] = {(double)t[j].x - cb[0], (double)t[j].y - cb[1], (double)t[j].z - cb[2]};
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) H[3 * r + c] += a[r] * b[c];
    }
    float T[12];
    kabsch_from_H(H, ca, cb, T);
    pass = true;
    if (check2 > 0.f) {
#pragma unroll
      for (int j = 0; j < RN; ++j)
        if (!(rs_resid2(T, s[j], t[j]) <= check2)) pass = false;
    }
    float4* out = reinterpret_cast<float4*>(poses + (size_t)p * 12);
    out[0] = make_float4(T[0], T[1], T[2], T[3]);
    out[1] = make_float4(T[4], T[5], T[6], T[7]);
    out[2] = make_float4(T[8], T[9], T[10], T[11]);
    if (!pass && hyp_status) hyp_status[h] = -2;
  }
  const unsigned long long w = __ballot(pass);
  __shared__ int wc[4];
  if ((threadIdx.x & 63) == 0) {
    mask[blockIdx.x * 4 + (threadIdx.x >> 6)] = w;
    wc[threadIdx.x >> 6] = __popcll(w);
  }
  __syncthreads();
  if (threadIdx.x == 0) bcnt[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// step 5, one hypothesis per WAVE: lane l takes correspondences i0 + l, i0 + l + 64, ... of the range
// [part * per, (part + 1) * per) from the packed records (20 KB per range at n = 5000, shared by the waves of a CU through
// its L1), the 64 sums are added by a butterfly
__global__ void __launch_bounds__(256) k_rs_score_wave(const RsCtrl* __restrict__ ctrl, long long h0,
                                                       const float4* __restrict__ pk, float thr2,
                                                       const int* __restrict__ list_b, const float* __restrict__ poses,
                                                       int* __restrict__ pcount, double* __restrict__ psse, size_t stride) {
  const int pair = blockIdx.z;
  ctrl = rs_at(ctrl, pair, stride);
  pk = rs_at(pk, pair, stride);
  list_b = rs_at(list_b, pair, stride);
  poses = rs_at(poses, pair, stride);
  pcount = rs_at(pcount, pair, stride);
  psse = rs_at(psse, pair, stride);
  if (h0 >= ctrl->limit) return;
  const int n_b = ctrl->n_b, n = ctrl->n;
  const int lane = threadIdx.x & 63, part = blockIdx.y;
  const int per = (n + RS_PARTS - 1) / RS_PARTS;
  const int i0 = min(n, part * per), i1 = min(n, i0 + per);
  for (int q = blockIdx.x * 4 + (threadIdx.x >> 6); q < n_b; q += gridDim.x * 4) {      // uniform over the wave
    const float* tp = poses + (size_t)list_b[q] * 12;
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = tp[k];
    int cnt = 0;
    double sse = 0.0;
    for (int i = i0 + lane; i < i1; i += 64) {
      const float d2 = rs_resid2(T, pk[2 * i], pk[2 * i + 1]);
      if (d2 < thr2) {
        ++cnt;
        sse += (double)d2;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    sse = wave_sum(sse);
    if (lane == 0) {
      pcount[(size_t)q * RS_PARTS + part] = cnt;
      psse[(size_t)q * RS_PARTS + part] = sse;
    }
  }
}

__device__ __forceinline__ bool rs_better(int c, double s, int h, int c2, double s2, int h2) {      // (c, s, h) beats (c2, s2, h2)
  if (h < 0) return false;
  if (h2 < 0) return true;
  return c > c2 || (c == c2 && (s < s2 || (s == s2 && h < h2)));
}

// end of a chunk (one workgroup per pair): the scored hypotheses' totals and statuses, the best of them against the best so far,
// the counters of info[] and the early-stop limit
__global__ void __launch_bounds__(1024) k_rs_best(RsCtrl* ctrl, long long h0, int m, int ransac_n, double confidence,
                                                  const int* __restrict__ list_a, const int* __restrict__ list_b,
                                                  const float* __restrict__ poses, const int* __restrict__ pcount,
                                                  const double* __restrict__ psse, int* __restrict__ hyp_status, size_t stride,
                                                  long long status_stride) {
  const int pair = blockIdx.z;
  ctrl = rs_at(ctrl, pair, stride);
  list_a = rs_at(list_a, pair, stride);
  list_b = rs_at(list_b, pair, stride);
  poses = rs_at(poses, pair, stride);
  pcount = rs_at(pcount, pair, stride);
  psse = rs_at(psse, pair, stride);
  if (hyp_status) hyp_status += (size_t)pair * status_stride;
  if (h0 >= ctrl->limit) return;
  const int n_b = ctrl->n_b, n = ctrl->n, t = threadIdx.x;
  __shared__ int bc[1024], bh[1024], bq[1024];
  __shared__ double bs[1024];
  int c_best = 0, h_best = -1, q_best = 0;
  double s_best = 0.0;
  for (int q = t; q < n_b; q += 1024) {
    int c = 0;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < RS_PARTS; ++k) { c += pcount[(size_t)q * RS_PARTS + k]; s += psse[(size_t)q * RS_PARTS + k]; }
    const int h = (int)(h0 + list_a[list_b[q]]);
    if (hyp_status) hyp_status[h] = c;
    if (c > 0 && rs_better(c, s, h, c_best, s_best, h_best)) { c_best = c; s_best = s; h_best = h; q_best = q; }
  }
  bc[t] = c_best; bs[t] = s_best; bh[t] = h_best; bq[t] = q_best;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (t < o && rs_better(bc[t + o], bs[t + o], bh[t + o], bc[t], bs[t], bh[t])) {
      bc[t] = bc[t + o]; bs[t] = bs[t + o]; bh[t] = bh[t + o]; bq[t] = bq[t + o];
    }
    __syncthreads();
  }
  if (t == 0) {
    if (rs_better(bc[0], bs[0], bh[0], ctrl->best_count, ctrl->best_sse, ctrl->best_h)) {
      ctrl->best_count = bc[0];
      ctrl->best_sse = bs[0];
      ctrl->best_h = bh[0];
      const float* tp = poses + (size_t)list_b[bq[0]] * 12;
      for (int k = 0; k < 12; ++k) ctrl->best_T[k] = tp[k];
    }
    ctrl->covered += m;
    ctrl->scored += n_b;
    if (confidence > 0.0 && confidence < 1.0 && ctrl->best_count > 0) {
      const double f = (double)ctrl->best_count / (double)n;
      long long lim = 0;
      if (f < 1.0) {
        double pw = f;
        for (int k = 1; k < ransac_n; ++k) pw *= f;
        const double den = log(1.0 - pw);      // 1 - f^k rounds to 1 for f^k < 2^-53: log = 0, no limit
        const double v = den < 0.0 ? ceil(log(1.0 - confidence) / den) : INFINITY;
        lim = (v < 9.0e18) ? (long long)v : RS_NO_LIMIT;
      }
      ctrl->limit = lim;
    }
  }
}

// outputs: the [4, 4] transformation, info, fit and the winner's inlier labels (the score's own comparison; 0 from the
// pair's count on)
__global__ void __launch_bounds__(256) k_rs_finish(const RsCtrl* __restrict__ ctrl, const float4* __restrict__ pk, int n_cap,
                                                   float thr2, float* trans16, int* info, float* fit, float* labels,
                                                   size_t stride) {
  const int pair = blockIdx.z;
  ctrl = rs_at(ctrl, pair, stride);
  pk = rs_at(pk, pair, stride);
  trans16 += (size_t)pair * 16;
  info += (size_t)pair * 4;
  fit += (size_t)pair * 2;
  if (labels) labels += (size_t)pair * n_cap;
  const int n = ctrl->n;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool found = ctrl->best_h >= 0 && ctrl->best_count > 0;
  if (i < 16) trans16[i] = i < 12 ? (found ? ctrl->best_T[i] : ((i % 5 == 0) ? 1.f : 0.f)) : (i == 15 ? 1.f : 0.f);
  if (i == 0) {
    info[0] = found ? ctrl->best_h : -1;
    info[1] = found ? ctrl->best_count : 0;
    info[2] = ctrl->covered;
    info[3] = ctrl->scored;
    fit[0] = found ? (float)((double)ctrl->best_count / (double)n) : 0.f;
    fit[1] = found ? (float)sqrt(ctrl->best_sse / (double)ctrl->best_count) : 0.f;
  }
  if (labels && i < n_cap) {
    float lab = 0.f;
    if (found && i < n) {
      float T[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) T[k] = ctrl->best_T[k];
      lab = rs_resid2(T, pk[2 * i], pk[2 * i + 1]) < thr2 ? 1.f : 0.f;
    }
    labels[i] = lab;
  }
}

static size_t rs_up256(size_t b) { return (b + 255) & ~(size_t)255; }
struct RsLayout { size_t ctrl, pk, mask, bcnt, list_a, list_b, poses, pcount, psse, total; };
static int rs_chunk(int chunk) { return chunk <= 0 ? RS_DEFAULT_CHUNK : std::min(chunk, RS_MAX_CHUNK); }
static RsLayout rs_layout(int n, int chunk) {
  RsLayout L;
  const size_t c = (size_t)cdiv(chunk, 256) * 256;
  size_t o = 0;
  L.ctrl = o;   o += 256;
  L.pk = o;     o += rs_up256((size_t)n * 32);
  L.mask = o;   o += rs_up256(c / 64 * 8);
  L.bcnt = o;   o += rs_up256(c / 256 * 4);
  L.list_a = o; o += rs_up256(c * 4);
  L.list_b = o; o += rs_up256(c * 4);
  L.poses = o;  o += rs_up256(c * 48);
  L.pcount = o; o += rs_up256(c * RS_PARTS * 4);
  L.psse = o;   o += rs_up256(c * RS_PARTS * 8);
  L.total = o;
  return L;
}

}  // namespace gcl

using namespace gcl;

extern "C" {

int32_t gcl_ransac_default_chunk(void) { return RS_DEFAULT_CHUNK; }

int64_t gcl_ransac_scratch_bytes(int32_t n, int32_t chunk) {
  if (n <= 0 || n > RS_MAX_N || chunk < 0) return 0;
  return (int64_t)rs_layout(n, rs_chunk(chunk)).total;
}

// the launches of a batch (one pair: a batch of one).  n_dev: device counts or NULL (n_cap for every pair); seeds: HOST array
static void rs_enqueue(const float* src, const float* tgt, int batch, int n_cap, const int* n_dev, int ransac_n,
                       float edge_similarity, float check_distance, float max_corr_distance, int max_iteration,
                       float confidence, const uint64_t* seeds, int chunk, void* scratch, float* trans16, int* info, float* fit,
                       float* labels, int* hyp_status, hipStream_t st) {
  const int ch = rs_chunk(chunk);
  const RsLayout L = rs_layout(n_cap, ch);
  const size_t stride = L.total;
  const long long ss = max_iteration;
  char* base = (char*)scratch;
  RsCtrl* ctrl = (RsCtrl*)(base + L.ctrl);
  float4* pk = (float4*)(base + L.pk);
  unsigned long long* mask = (unsigned long long*)(base + L.mask);
  int* bcnt = (int*)(base + L.bcnt);
  int *list_a = (int*)(base + L.list_a), *list_b = (int*)(base + L.list_b);
  float* poses = (float*)(base + L.poses);
  int* pcount = (int*)(base + L.pcount);
  double* psse = (double*)(base + L.psse);
  const float thr2 = max_corr_distance * max_corr_distance;
  const float check2 = check_distance > 0.f ? check_distance * check_distance : 0.f;
  const unsigned B = (unsigned)batch;
  for (int p0 = 0; p0 < batch; p0 += RS_SEED_GROUP) {
    const int g = std::min(RS_SEED_GROUP, batch - p0);
    RsSeeds sd;
    for (int k = 0; k < RS_SEED_GROUP; ++k) sd.s[k] = k < g ? (unsigned long long)seeds[p0 + k] : 0ull;
    hipLaunchKernelGGL(k_rs_init, dim3((unsigned)cdiv(n_cap, 256), 1, (unsigned)g), dim3(256), 0, st, src, tgt, n_cap, n_dev,
                       ransac_n, p0, sd, pk, ctrl, stride);
  }
  for (long long h0 = 0; h0 < max_iteration; h0 += ch) {
    const int m = (int)std::min<long long>(ch, max_iteration - h0);
    const dim3 grid((unsigned)cdiv(m, 256), 1, B);
    if (ransac_n == 3) {
      hipLaunchKernelGGL(k_rs_draw<3>, grid, dim3(256), 0, st, (const RsCtrl*)ctrl, h0, m, (const float4*)pk, edge_similarity,
                         mask, bcnt, hyp_status, stride, ss);
    } else {
      hipLaunchKernelGGL(k_rs_draw<4>, grid, dim3(256), 0, st, (const RsCtrl*)ctrl, h0, m, (const float4*)pk, edge_similarity,
                         mask, bcnt, hyp_status, stride, ss);
    }
    hipLaunchKernelGGL(k_rs_compact, grid, dim3(256), 0, st, ctrl, h0, 0, m, (const unsigned long long*)mask,
                       (const int*)bcnt, list_a, stride);
    if (ransac_n == 3) {
      hipLaunchKernelGGL(k_rs_pose<3>, grid, dim3(256), 0, st, (const RsCtrl*)ctrl, h0, (const float4*)pk, check2,
                         (const int*)list_a, poses, mask, bcnt, hyp_status, stride, ss);
    } else {
      hipLaunchKernelGGL(k_rs_pose<4>, grid, dim3(256), 0, st, (const RsCtrl*)ctrl, h0, (const float4*)pk, check2,
                         (const int*)list_a, poses, mask, bcnt, hyp_status, stride, ss);
    }
    hipLaunchKernelGGL(k_rs_compact, grid, dim3(256), 0, st, ctrl, h0, 1, m, (const unsigned long long*)mask,
                       (const int*)bcnt, list_b, stride);
    hipLaunchKernelGGL(k_rs_score_wave, dim3((unsigned)std::min<long long>(cdiv(m, 4), RS_SCORE_GRID), RS_PARTS, B), dim3(256),
                       0, st, (const RsCtrl*)ctrl, h0, (const float4*)pk, thr2, (const int*)list_b, (const float*)poses, pcount,
                       psse, stride);
    hipLaunchKernelGGL(k_rs_best, dim3(1, 1, B), dim3(1024), 0, st, ctrl, h0, m, ransac_n, (double)confidence,
                       (const int*)list_a, (const int*)list_b, (const float*)poses, (const int*)pcount, (const double*)psse,
                       hyp_status, stride, ss);
  }
  hipLaunchKernelGGL(k_rs_finish, dim3((unsigned)cdiv(std::max(n_cap, 16), 256), 1, B), dim3(256), 0, st, (const RsCtrl*)ctrl,
                     (const float4*)pk, n_cap, thr2, trans16, info, fit, labels, stride);
}

int gcl_ransac_register(const float* src, const float* tgt, int32_t n, int32_t ransac_n, float edge_similarity,
                        float check_distance, float max_corr_distance, int32_t max_iteration, float confidence,
                        uint64_t seed, int32_t chunk, void* scratch, float* trans16, int32_t* info, float* fit, float* labels,
                        int32_t* hyp_status, void* stream) {
  GCL_CHECK_ARG(src && tgt && scratch && trans16 && info && fit, "gcl_ransac_register: null pointer");
  GCL_CHECK_ARG(ransac_n == 3 || ransac_n == 4, "gcl_ransac_register: ransac_n must be 3 or 4, got %d", ransac_n);
  GCL_CHECK_ARG(n >= ransac_n, "gcl_ransac_register: n = %d correspondences, fewer than ransac_n = %d", n, ransac_n);
  GCL_CHECK_ARG(n <= RS_MAX_N, "gcl_ransac_register: n = %d correspondences, more than %d", n, RS_MAX_N);
  GCL_CHECK_ARG(max_iteration >= 1, "gcl_ransac_register: max_iteration must be >= 1, got %d", max_iteration);
  GCL_CHECK_ARG(max_corr_distance > 0.f, "gcl_ransac_register: max_corr_distance must be > 0");
  GCL_CHECK_ARG(chunk >= 0, "gcl_ransac_register: chunk must be >= 0 (0 = default), got %d", chunk);
  rs_enqueue(src, tgt, 1, n, nullptr, ransac_n, edge_similarity, check_distance, max_corr_distance, max_iteration, confidence,
             &seed, chunk, scratch, trans16, info, fit, labels, hyp_status, (hipStream_t)stream);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int64_t gcl_ransac_batch_scratch_bytes(int32_t batch, int32_t n_cap, int32_t chunk) {
  if (batch < 1 || batch > RS_MAX_BATCH || n_cap <= 0 || n_cap > RS_MAX_N || chunk < 0) return 0;
  return (int64_t)batch * (int64_t)rs_layout(n_cap, rs_chunk(chunk)).total;
}

int gcl_ransac_register_batch(const float* src, const float* tgt, int32_t batch, int32_t n_cap, const int32_t* n_dev,
                              int32_t ransac_n, float edge_similarity, float check_distance, float max_corr_distance,
                              int32_t max_iteration, float confidence, const uint64_t* seeds, int32_t chunk, void* scratch,
                              float* trans16, int32_t* info, float* fit, float* labels, int32_t* hyp_status, void* stream) {
  GCL_CHECK_ARG(src && tgt && seeds && scratch && trans16 && info && fit, "gcl_ransac_register_batch: null pointer");
  GCL_CHECK_ARG(batch >= 1 && batch <= RS_MAX_BATCH, "gcl_ransac_register_batch: batch must be in [1, %d], got %d",
                RS_MAX_BATCH, batch);
  GCL_CHECK_ARG(ransac_n == 3 || ransac_n == 4, "gcl_ransac_register_batch: ransac_n must be 3 or 4, got %d", ransac_n);
  GCL_CHECK_ARG(n_cap >= ransac_n, "gcl_ransac_register_batch: n_cap = %d correspondences, fewer than ransac_n = %d", n_cap,
                ransac_n);
  GCL_CHECK_ARG(n_cap <= RS_MAX_N, "gcl_ransac_register_batch: n_cap = %d correspondences, more than %d", n_cap, RS_MAX_N);
  GCL_CHECK_ARG(max_iteration >= 1, "gcl_ransac_register_batch: max_iteration must be >= 1, got %d", max_iteration);
  GCL_CHECK_ARG(max_corr_distance > 0.f, "gcl_ransac_register_batch: max_corr_distance must be > 0");
  GCL_CHECK_ARG(chunk >= 0, "gcl_ransac_register_batch: chunk must be >= 0 (0 = default), got %d", chunk);
  rs_enqueue(src, tgt, batch, n_cap, n_dev, ransac_n, edge_similarity, check_distance, max_corr_distance, max_iteration,
             confidence, seeds, chunk, scratch, trans16, info, fit, labels, hyp_status, (hipStream_t)stream);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

}  // extern "C"
