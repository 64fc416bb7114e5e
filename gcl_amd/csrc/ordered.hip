// The ordered row sum: contribution records (destination row, value[c]) added into dF in ascending list position.
//
// The loss backward kernels scatter their contributions with float atomics, whose landing order changes from run to run and
// with it the rounding of every row that receives more than one.  Their *_emit twins (loss.hip, pairloss.hip: the same
// kernel bodies with a RecordSink, losssink.h) write the contributions as a LIST instead, at positions that depend on the
// inputs only; gcl_ordered_row_sum then gives, for every row named by at least one record,
//     dF[row] = fl(... fl(fl(dF[row] + v_1) + v_2) ... + v_k)       in fp32, over the row's records in ascending position,
// which is one of the results the atomic kernels may produce, and the same one every time.
//
// How.  Integer atomics count and place, but nothing is added before a row's record ids stand in ascending order:
//   k_ors_zero     the two counters and count[n_rows] = 0
//   k_ors_count    rank[i] = atomicAdd(count[row_i], 1)        (which record gets which rank is arbitrary)
//   k_ors_place    the record of rank 0 claims its row's segment of ids[] (start[row] = atomicAdd(placed, count[row])) and
//                  appends the row to rows[] (both in arbitrary order: neither enters a sum)
//   k_ors_scatter  ids[start[row_i] + rank[i]] = i             (a row's segment: its record ids, unordered)
//   k_ors_sum      ONE WAVE PER NAMED ROW, lane = channel.  The wave walks its segment in windows of ORS_WINDOW consecutive
//                  record ids [lo, lo + ORS_WINDOW): every id of the segment inside the window sets bit (id - lo) of a bitmap
//                  in LDS (integer or: the bitmap does not depend on the order), the bits are then read in ascending
//                  order -- that IS the ascending order of the ids, record ids being distinct -- and each one's value row is
//                  added to the lane's accumulator, which started from dF[row]; lo then jumps to the lowest id beyond the
//                  window.  Any number of records per row: a row with more ids than a window holds, or spread further apart,
//                  takes more passes over its segment.  The row is written with one plain store per lane.
// No host read anywhere: the grid of k_ors_sum is n_rec workgroups (a bound of the named rows), the surplus leaves at once.
#include "common.h"
#include "losssink.h"

#include <limits.h>

namespace gcl {

constexpr int ORS_WINDOW = 1024;      // record ids per pass of k_ors_sum: 16 words of 64 bits in LDS

__global__ void __launch_bounds__(256) k_rec_fill(int* __restrict__ rec_row, long long n_rec) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n_rec) rec_row[i] = -1;
}

void rec_fill(int* rec_row, long long n_rec, hipStream_t stream) {
  if (n_rec > 0) hipLaunchKernelGGL(k_rec_fill, dim3((unsigned)cdiv(n_rec, 256)), dim3(256), 0, stream, rec_row, n_rec);
}

// scratch (int32 words): [0] ids placed so far, [1] rows named so far, count[n_rows], start[n_rows], rank[n_rec],
// ids[n_rec], rows[n_rec]
struct OrsScratch {
  int *ctr, *count, *start, *rank, *ids, *rows;
};
static OrsScratch ors_scratch(int32_t* s, long long n_rec, long long n_rows) {
  OrsScratch o;
  o.ctr = s;
  o.count = s + 2;
  o.start = o.count + n_rows;
  o.rank = o.start + n_rows;
  o.ids = o.rank + n_rec;
  o.rows = o.ids + n_rec;
  return o;
}

__global__ void __launch_bounds__(256) k_ors_zero(int* __restrict__ head, long long n) {      // ctr[2] and count[n_rows]
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) head[i] = 0;
}

__device__ __forceinline__ bool ors_named(int r, int n_rows) { return r >= 0 && r < n_rows; }

__global__ void __launch_bounds__(256) k_ors_count(const int* __restrict__ rec_row, int n_rec, int n_rows,
                                                   int* __restrict__ count, int* __restrict__ rank) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rec) return;
  const int r = rec_row[i];
  rank[i] = ors_named(r, n_rows) ? atomicAdd(&count[r], 1) : -1;
}

__global__ void __launch_bounds__(256) k_ors_place(const int* __restrict__ rec_row, int n_rec, const int* __restrict__ rank,
                                                   const int* __restrict__ count, int* __restrict__ ctr,
                                                   int* __restrict__ start, int* __restrict__ rows) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rec || rank[i] != 0) return;
  const int r = rec_row[i];
  start[r] = atomicAdd(&ctr[0], count[r]);       // segments tile ids[0 .. named records): the sum of the counts <= n_rec
  rows[atomicAdd(&ctr[1], 1)] = r;               // one entry per named row: <= n_rec of them
}

__global__ void __launch_bounds__(256) k_ors_scatter(const int* __restrict__ rec_row, int n_rec,
                                                     const int* __restrict__ rank, const int* __restrict__ start,
                                                     int* __restrict__ ids) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rec || rank[i] < 0) return;
  ids[start[rec_row[i]] + rank[i]] = (int)i;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}

__global__ void __launch_bounds__(64) k_ors_sum(const float* __restrict__ rec_val, int c, const int* __restrict__ ctr,
                                                const int* __restrict__ rows, const int* __restrict__ count,
                                                const int* __restrict__ start, const int* __restrict__ ids,
                                                float* __restrict__ df) {
  __shared__ unsigned long long bm[ORS_WINDOW / 64];
  const int lane = threadIdx.x;
  if ((int)blockIdx.x >= ctr[1]) return;                                  // uniform: before any barrier
  const int r = rows[blockIdx.x];
  const int k = count[r];
  const int* __restrict__ seg = ids + start[r];
  float acc = (lane < c) ? df[(long long)r * c + lane] : 0.f;
  int lo = INT_MAX;
  for (int q = lane; q < k; q += 64) lo = min(lo, seg[q]);
  lo = wave_min(lo);
  while (lo != INT_MAX) {                                                 // uniform: lo is the wave's minimum
    if (lane < ORS_WINDOW / 64) bm[lane] = 0ull;
    __syncthreads();
    int next = INT_MAX;
    for (int q = lane; q < k; q += 64) {
      const int id = seg[q];
      if (id < lo) continue;                                              // added by an earlier pass
      const int p = id - lo;
      if (p < ORS_WINDOW) atomicOr(&bm[p >> 6], 1ull << (p & 63));
      else next = min(next, id);
    }
    next = wave_min(next);
    __syncthreads();
    for (int j = 0; j < ORS_WINDOW / 64; ++j) {
      unsigned long long w = bm[j];                                       // the same word in every lane
      while (w) {
        const long long id = (long long)lo + j * 64 + (__ffsll(w) - 1);
        w &= w - 1;
        if (lane < c) acc += rec_val[id * c + lane];
      }
    }
    __syncthreads();                                                      // every lane has read the bitmap: it may be cleared
    lo = next;
  }
  if (lane < c) df[(long long)r * c + lane] = acc;
}

}  // namespace gcl

using namespace gcl;

extern "C" {

int32_t gcl_ordered_row_sum_window(void) { return ORS_WINDOW; }

int64_t gcl_ordered_row_sum_scratch_len(int32_t n_rec, int64_t n_rows) {
  if (n_rec <= 0 || n_rows <= 0 || n_rows > INT_MAX) return 0;
  return 2 + 2 * n_rows + 3 * (int64_t)n_rec;
}

int gcl_ordered_row_sum(const int32_t* rec_row, const float* rec_val, int32_t n_rec, int32_t c, int64_t n_rows,
                        int32_t* scratch, float* df, void* stream) {
  GCL_CHECK_ARG(n_rec >= 0, "gcl_ordered_row_sum: negative record count (%d)", n_rec);
  GCL_CHECK_ARG(n_rows >= 0 && n_rows <= INT_MAX, "gcl_ordered_row_sum: n_rows must lie in 0 .. 2^31 - 1 (rows are int32)");
  GCL_CHECK_ARG(c >= 1 && c <= 64, "gcl_ordered_row_sum: row width must lie in 1 .. 64 (got %d)", c);
  if (n_rec == 0 || n_rows == 0) return GCL_OK;
  GCL_CHECK_ARG(rec_row && rec_val && scratch && df, "gcl_ordered_row_sum: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const OrsScratch s = ors_scratch(scratch, n_rec, n_rows);
  const int nr = (int)n_rows;
  const unsigned g = (unsigned)cdiv(n_rec, 256);
  hipLaunchKernelGGL(k_ors_zero, dim3((unsigned)cdiv(2 + n_rows, 256)), dim3(256), 0, st, scratch, (long long)(2 + n_rows));
  hipLaunchKernelGGL(k_ors_count, dim3(g), dim3(256), 0, st, (const int*)rec_row, n_rec, nr, s.count, s.rank);
  hipLaunchKernelGGL(k_ors_place, dim3(g), dim3(256), 0, st, (const int*)rec_row, n_rec, (const int*)s.rank,
                     (const int*)s.count, s.ctr, s.start, s.rows);
  hipLaunchKernelGGL(k_ors_scatter, dim3(g), dim3(256), 0, st, (const int*)rec_row, n_rec, (const int*)s.rank,
                     (const int*)s.start, s.ids);
  hipLaunchKernelGGL(k_ors_sum, dim3((unsigned)n_rec), dim3(64), 0, st, rec_val, c, (const int*)s.ctr, (const int*)s.rows,
                     (const int*)s.count, (const int*)s.start, (const int*)s.ids, df);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

}  // extern "C"
