// Host build of the fp64 3 x 3 Kabsch solution of the registration back-ends (gcl_amd/csrc/kabsch.h, the very header the
// kernels include): TEST INFRASTRUCTURE, loaded by tests/test_oracle_kabsch.py through ctypes, never linked into the
// product library.  Compiled host-only (oracle/Makefile), so it runs without a GPU.
//
// H [n, 9] row-major, ca / cb [n, 3]; problem i is independent of every other.
#include "../gcl_amd/csrc/kabsch.h"

extern "C" {

// T12 float [n, 12]: the rows of [R | t] as the kernels pack them (kabsch_from_H)
void kabsch_host_pack(const double* H, const double* ca, const double* cb, long long n, float* T12) {
  for (long long i = 0; i < n; ++i) gcl::kabsch_from_H(H + 9 * i, ca + 3 * i, cb + 3 * i, T12 + 12 * i);
}

// R9 double [n, 9]: the fp64 rotation before any packing (kabsch_rotation)
void kabsch_host_rotation(const double* H, long long n, double* R9) {
  for (long long i = 0; i < n; ++i) gcl::kabsch_rotation(H + 9 * i, R9 + 9 * i);
}

}  // extern "C"
