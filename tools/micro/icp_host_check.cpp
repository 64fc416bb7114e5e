// The HOST side of the ICP entry (csrc/icp.hip) under AddressSanitizer + UBSan, as a stand-alone program: scratch sizing and the
// argument validation, which reads the two host offset arrays before anything is launched.  No device work: every call below
// is refused (or sized) on the host, so the program needs no GPU and never runs a kernel.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -o icp_host_check tools/micro/icp_host_check.cpp gcl_amd/csrc/icp.hip gcl_amd/csrc/coords.hip && ./icp_host_check
//
// Exit status 0 and "icp_host_check: ok" when every expectation holds and the sanitizers stay silent.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/gcl_amd.h"

static int failures = 0;

#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static int call(const int64_t* o0, const int64_t* o1, int32_t n_pairs, double dist, int32_t max_iteration, void* dev) {
  // `dev` stands for every device pointer: validation never dereferences one
  return gcl_icp_register_batch((const float*)dev, o0, (const int64_t*)dev, (const float*)dev, o1, (const int64_t*)dev, n_pairs,
                                (const int64_t*)dev, (const int64_t*)dev, dist, (const double*)dev, max_iteration, 1e-6, 1e-6,
                                dev, (double*)dev, (double*)dev, (int32_t*)dev, nullptr, nullptr);
}

static bool refused(int rc, const char* word) { return rc == GCL_ERR_ARG && std::strstr(gcl_last_error(), word) != nullptr; }

int main() {
  // scratch sizing: out-of-range arguments give 0, the layout grows with both sides and the pair count
  EXPECT(gcl_icp_scratch_bytes(-1, 0, 1) == 0 && gcl_icp_scratch_bytes(0, -1, 1) == 0);
  EXPECT(gcl_icp_scratch_bytes(0, 0, 0) == 0 && gcl_icp_scratch_bytes(0, 0, GCL_FPFH_MAX_CLOUDS + 1) == 0);
  EXPECT(gcl_icp_scratch_bytes(int64_t(1) << 31, 0, 1) == 0 && gcl_icp_scratch_bytes(0, int64_t(1) << 31, 1) == 0);
  EXPECT(gcl_icp_scratch_bytes(0, 0, 1) > 0);
  const int64_t big = gcl_icp_scratch_bytes(0x7fffffff, 0x7fffffff, GCL_FPFH_MAX_CLOUDS);
  EXPECT(big > 16ll * 0x7fffffff && big < (int64_t(1) << 40));
  EXPECT(gcl_icp_scratch_bytes(1000, 2000, 3) >= 16 * 2000 + 136 * (4 + 3));

  // the offsets live in exactly sized heap blocks: a read past n_pairs + 1 entries is an ASan report
  void* dev = nullptr;
  {
    std::vector<int64_t> ok{0, 10}, late{1, 10}, down{0, 5, 3}, three{0, 4, 10};
    EXPECT(refused(call(ok.data(), ok.data(), 0, 0.2, 30, dev), "n_pairs"));
    EXPECT(refused(call(ok.data(), ok.data(), 1, 0.0, 30, dev), "positive"));
    EXPECT(refused(call(ok.data(), ok.data(), 1, -0.2, 30, dev), "positive"));
    EXPECT(refused(call(ok.data(), ok.data(), 1, std::nan(""), 30, dev), "positive"));
    EXPECT(refused(call(ok.data(), ok.data(), 1, std::numeric_limits<double>::infinity(), 30, dev), "positive"));
    EXPECT(refused(call(ok.data(), ok.data(), 1, 1e-60, 30, dev), "positive"));          // underflows the grid's float edge
    EXPECT(refused(call(ok.data(), ok.data(), 1, 0.2, -1, dev), "max_iteration"));
    EXPECT(refused(call(nullptr, ok.data(), 1, 0.2, 30, dev), "offsets0_host"));
    EXPECT(refused(call(ok.data(), nullptr, 1, 0.2, 30, dev), "offsets1_host"));
    EXPECT(refused(call(late.data(), ok.data(), 1, 0.2, 30, dev), "not 0"));
    EXPECT(refused(call(three.data(), down.data(), 2, 0.2, 30, dev), "descends"));
    // valid host arguments, null device pointers: refused before any launch
    EXPECT(refused(call(ok.data(), ok.data(), 1, 0.2, 30, dev), "null pointer"));
    EXPECT(refused(call(three.data(), three.data(), 2, 0.2, 200, dev), "null pointer"));
  }
  {
    // the largest batch: n_pairs + 1 offsets, every pair one row; and a total above 2^31 - 1
    std::vector<int64_t> many(GCL_FPFH_MAX_CLOUDS + 1);
    for (size_t b = 0; b < many.size(); ++b) many[b] = (int64_t)b;
    EXPECT(refused(call(many.data(), many.data(), GCL_FPFH_MAX_CLOUDS, 0.2, 30, dev), "null pointer"));
    many.back() = int64_t(1) << 31;
    EXPECT(refused(call(many.data(), many.data(), GCL_FPFH_MAX_CLOUDS, 0.2, 30, dev), "2^31"));
  }
  std::printf(failures ? "icp_host_check: %d FAILED\n" : "icp_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
