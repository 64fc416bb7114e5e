// Where a loss backward kernel puts a contribution (destination row, value of one channel): the SINK is a template
// parameter of the kernel, so that the atomic entry and its *_emit twin are two instantiations of ONE body -- the value
// expressions are the same code.
//
//   AtomicSink   df[which][row * c + ch] += v with a float atomic (what the kernels have always done; a lane whose value
//                is exactly 0 is skipped where the kernel says so)
//   RecordSink   record `slot` of list `which` := (row, v): rec_row[slot] = row, rec_val[slot * c + ch] = v.  The value is
//                stored whole (zeros included); a slot the kernel never reaches keeps the -1 the entry filled in before
//                the launch.  A slot at or past n_rec (a capacity the caller chose too small) is dropped, never written.
//
// `which` selects the cloud of the pair losses (0: F0 / dF0, 1: F1 / dF1); the group losses use list 0 only.
#pragma once

namespace gcl {

struct AtomicSink {
  static constexpr bool kRecords = false;
  float* df[2];
  __device__ __forceinline__ void put(int which, long long, long long row, int c, int ch, float v, bool skip_zero) const {
    if (!skip_zero || v != 0.f) atomicAdd(&df[which][row * c + ch], v);
  }
};

struct RecordSink {
  static constexpr bool kRecords = true;
  int* row[2];
  float* val[2];
  long long n_rec;
  __device__ __forceinline__ void put(int which, long long slot, long long r, int c, int ch, float v, bool) const {
    if (slot >= n_rec) return;
    if (ch == 0) row[which][slot] = (int)r;
    val[which][slot * c + ch] = v;
  }
};

// rec_row[0 .. n_rec) = -1, one launch on `stream` (ordered.hip): what every *_emit entry does before its kernel
void rec_fill(int* rec_row, long long n_rec, hipStream_t stream);

}  // namespace gcl
