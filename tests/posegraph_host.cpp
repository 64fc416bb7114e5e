// The host build of gcl_amd/csrc/posegraph.h for tests/test_oracle_multiway.py: one graph, one thread.
#include "posegraph.h"
extern "C" void pg_host(int n, int m, const int* src, const int* dst, const int* uncertain, const double* nodes,
                        const double* edge_T, const double* edge_info, const double* params, double* poses, double* conf,
                        int* kept, double* stats, int* status) {
  static gcl::PgWork W;
  gcl::pg_global_optimization(gcl::PgSerial(), gcl::PgGraph{n, m, src, dst, uncertain, nodes, edge_T, edge_info}, W,
                              gcl::pg_params(params), poses, conf, kept, stats, status);
}
