// Runs gcl_amd/csrc/posegraph.h on the host over the graphs of a text file and prints poses and solve counts: the same text
// the kernel compiles, here as one thread, so that host tools (a sanitizer, gdb) can look at it.
//
//   python tests/multiway_scenes.py > graphs.txt
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -std=c++17 -I gcl_amd/csrc \
//       tools/micro/posegraph_host_check.cpp -o tools/micro/posegraph_host_check
//   tools/micro/posegraph_host_check graphs.txt
//
// File: the number of graphs; per graph "n m", m lines "source target uncertain", then 16 n node, 16 m edge and 36 m
// information numbers.
#include "posegraph.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static bool read_doubles(FILE* f, std::vector<double>& v, size_t n) {
  v.resize(n);
  for (size_t i = 0; i < n; ++i)
    if (fscanf(f, "%lf", &v[i]) != 1) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s graphs.txt\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  int graphs = 0;
  if (fscanf(f, "%d", &graphs) != 1 || graphs < 0) return 2;
  const double params[gcl::PG_PARAMS] = {0.075, 0.25, 1.0, 0, 100, 1e-6, 1e-6, 1e-6, 1e-6, 20, 2.0 / 3.0, 1.0 / 3.0};
  std::vector<gcl::PgWork> work(1);
  int failures = 0;
  for (int g = 0; g < graphs; ++g) {
    int n = 0, m = 0;
    if (fscanf(f, "%d %d", &n, &m) != 2 || n < 1 || n > gcl::PG_MAX_NODES || m < 0 || m > gcl::PG_MAX_EDGES) {
      fprintf(stderr, "graph %d: bad size\n", g);
      return 2;
    }
    std::vector<int> src(m), dst(m), unc(m);
    for (int k = 0; k < m; ++k)
      if (fscanf(f, "%d %d %d", &src[k], &dst[k], &unc[k]) != 3 || src[k] < 0 || src[k] >= dst[k] || dst[k] >= n) {
        fprintf(stderr, "graph %d: bad edge %d\n", g, k);
        return 2;
      }
    std::vector<double> nodes, edge_T, info;
    if (!read_doubles(f, nodes, 16 * (size_t)n) || !read_doubles(f, edge_T, 16 * (size_t)m) ||
        !read_doubles(f, info, 36 * (size_t)m)) {
      fprintf(stderr, "graph %d: short file\n", g);
      return 2;
    }
    std::vector<double> poses(16 * (size_t)n), conf(m), stats(gcl::PG_STATS);
    std::vector<int> kept(m);
    int status = -1;
    const gcl::PgGraph G{n, m, src.data(), dst.data(), unc.data(), nodes.data(), edge_T.data(), info.data()};
    gcl::pg_global_optimization(gcl::PgSerial(), G, work[0], gcl::pg_params(params), poses.data(), conf.data(), kept.data(),
                                stats.data(), &status);
    int dropped = 0;
    for (int k = 0; k < m; ++k) dropped += !kept[k];
    printf("graph %d: %d nodes, %d edges, status %d, solves %g + %g, residual %.6e, %d edges dropped\n", g, n, m, status,
           stats[0], stats[1], stats[2], dropped);
    for (int i = 0; i < n; ++i) {
      printf("  node %d:", i);
      for (int c = 0; c < 12; ++c) printf(" %.12f", poses[16 * i + c]);
      printf("\n");
    }
    failures += status != 0;
  }
  fclose(f);
  return failures ? 1 : 0;
}
