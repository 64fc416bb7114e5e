// Pose-graph optimisation of one small graph in fp64: open3d's GlobalOptimization with GlobalOptimizationLevenbergMarquardt
// (a line process on the uncertain edges, two passes, edge pruning between them), restated from its published source in
// DESIGN.md "Multiway registration".  The same text compiles for the kernel (multiway.hip: one workgroup per graph, the
// working set in LDS) and for the host (tests and tools/micro/posegraph_host_check.cpp): a `Team` says who runs it --
// PgSerial is one thread, the kernel's team is a workgroup -- and every function here is entered by the whole team with
// the same arguments.  Work is dealt by rank; every sum is taken by one thread in a fixed order (edge order, then
// row-major), so the result does not depend on the team's size.  Scalars that steer the control flow are recomputed by
// every thread from shared values after a sync(): the flow is uniform.
//
// The rule for the shared working set: a value that every thread reads (conf, r, r_new, b, delta, x, H's diagonal, L's
// pivots) is written only between two sync()s that all its readers have passed.  Where each sync stands:
//   pg_errors             leaves with one: e and r are there for pg_residual on every thread
//   pg_update_confidence  enters with one (pg_residual on every thread is done with conf and r), leaves with one
//   pg_linear_system      one between the per-edge A, g and the per-entry H, b; leaves with one (H, b for every thread)
//   pg_solve              one after L = H + lambda I; two per column of the factorisation (the scaled column and its
//                         unscaled copy `col`, then the trailing update); one per column of either substitution: leaves with delta
//   pg_pass, accepting    one in front of the copies T_new -> T, e_new -> e, r_new -> r (every thread is done with delta, b,
//                         r_new and conf: rho and the stop tests are in registers), one behind them
//   pg_global_optimization  around the set-up, around the pruning of the edges, in front of the results
//
// This header includes nothing of the device runtime: a host compiler reads it as plain C++.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PG_HD __host__ __device__
#else
#define PG_HD
#endif

namespace gcl {

constexpr int PG_MAX_NODES = 8, PG_MAX_EDGES = 28, PG_DIM = 6 * PG_MAX_NODES;
constexpr int PG_STATS = 3;   // linear solves of pass 1, of pass 2, the final residual

// status of a graph
constexpr int PG_OK = 0, PG_NO_CORRESPONDENCE = 1, PG_NON_FINITE = 2, PG_BREAKDOWN = 3;

struct PgSerial {
  PG_HD int rank() const { return 0; }
  PG_HD int size() const { return 1; }
  PG_HD void sync() const {}
};

struct PgParams {
  double max_correspondence_distance, edge_prune_threshold, preference_loop_closure;
  int reference_node;
  // GlobalOptimizationConvergenceCriteria
  int max_iteration;
  double min_relative_increment, min_relative_residual_increment, min_right_term, min_residual;
  int max_iteration_lm;
  double upper_scale_factor, lower_scale_factor;
};

constexpr int PG_PARAMS = 12;
// the twelve numbers of PgParams in declaration order, as doubles (what a foreign caller passes)
PG_HD inline PgParams pg_params(const double* o) {
  PgParams P;
  P.max_correspondence_distance = o[0];
  P.edge_prune_threshold = o[1];
  P.preference_loop_closure = o[2];
  P.reference_node = (int)o[3];
  P.max_iteration = (int)o[4];
  P.min_relative_increment = o[5];
  P.min_relative_residual_increment = o[6];
  P.min_right_term = o[7];
  P.min_residual = o[8];
  P.max_iteration_lm = (int)o[9];
  P.upper_scale_factor = o[10];
  P.lower_scale_factor = o[11];
  return P;
}

struct PgGraph {              // one graph's slice of the flat arrays
  int n, m;
  const int* src;             // [m]
  const int* dst;             // [m]
  const int* uncertain;       // [m]
  const double* nodes;        // [n, 16]
  const double* edge_T;       // [m, 16]
  const double* edge_info;    // [m, 36]
};

struct PgWork {               // the team's shared working set (LDS in the kernel): about 52 KB
  double H[PG_DIM * PG_DIM];
  double L[PG_DIM * PG_DIM];  // H + lambda I, factorised in place: unit lower triangle below, D on the diagonal
  double b[PG_DIM], y[PG_DIM], delta[PG_DIM], col[PG_DIM], x[PG_DIM];
  double A[PG_MAX_EDGES][36]; // Js^T I Js
  double g[PG_MAX_EDGES][6];  // Js^T I e
  double Xinv[PG_MAX_EDGES][16];
  double e[PG_MAX_EDGES][6], e_new[PG_MAX_EDGES][6];
  double r[PG_MAX_EDGES], r_new[PG_MAX_EDGES];          // e^T I e
  double conf[PG_MAX_EDGES];
  double T[PG_MAX_NODES][16], T_new[PG_MAX_NODES][16];
  int active[PG_MAX_EDGES];
  int bad;                    // a non-finite input was seen
};

// ---- 4 x 4 row-major helpers ------------------------------------------------------------------------------------------
PG_HD inline void pg_mul(const double* A, const double* B, double* C) {
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double s = A[4 * i] * B[j];
      for (int k = 1; k < 4; ++k) s += A[4 * i + k] * B[4 * k + j];
      C[4 * i + j] = s;
    }
}

// [R^T | -R^T t]
PG_HD inline void pg_rigid_inv(const double* A, double* C) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) C[4 * i + j] = A[4 * j + i];
    C[4 * i + 3] = -((A[i] * A[3] + A[4 + i] * A[7]) + A[8 + i] * A[11]);
    C[12 + i] = 0.0;
  }
  C[15] = 1.0;
}

PG_HD inline void pg_lin6(const double* M, double* v) {
  v[0] = (M[9] - M[6]) / 2.0;
  v[1] = (M[2] - M[8]) / 2.0;
  v[2] = (M[4] - M[1]) / 2.0;
  v[3] = M[3];
  v[4] = M[7];
  v[5] = M[11];
}

// R = Rz(v2) Ry(v1) Rx(v0), t = v[3:6]
PG_HD inline void pg_vec2mat(const double* v, double* M) {
  const double sa = sin(v[0]), ca = cos(v[0]), sb = sin(v[1]), cb = cos(v[1]), sc = sin(v[2]), cc = cos(v[2]);
  M[0] = cb * cc;  M[1] = sa * sb * cc - ca * sc;  M[2] = ca * sb * cc + sa * sc;   M[3] = v[3];
  M[4] = cb * sc;  M[5] = sa * sb * sc + ca * cc;  M[6] = ca * sb * sc - sa * cc;   M[7] = v[4];
  M[8] = -sb;      M[9] = sa * cb;                 M[10] = ca * cb;                 M[11] = v[5];
  M[12] = 0.0;     M[13] = 0.0;                    M[14] = 0.0;                     M[15] = 1.0;
}

PG_HD inline void pg_mat2vec(const double* M, double* v) {
  const double sy = hypot(M[0], M[4]);
  if (sy > 1e-6) {
    v[0] = atan2(M[9], M[10]);
    v[1] = atan2(-M[8], sy);
    v[2] = atan2(M[4], M[0]);
  } else {
    v[0] = atan2(-M[6], M[5]);
    v[1] = atan2(-M[8], sy);
    v[2] = 0.0;
  }
  v[3] = M[3];
  v[4] = M[7];
  v[5] = M[11];
}

PG_HD inline double pg_quad(const double* I, const double* e) {      // e^T I e, row-major
  double s = 0.0;
  for (int i = 0; i < 6; ++i) {
    double t = I[6 * i] * e[0];
    for (int j = 1; j < 6; ++j) t += I[6 * i + j] * e[j];
    s += e[i] * t;
  }
  return s;
}

// ---- the pieces of a pass --------------------------------------------------------------------------------------------
// e = lin6(X^-1 T_t^-1 T_s) and e^T I e of every active edge under the poses T
template <class Team>
PG_HD void pg_errors(const Team& tm, const PgGraph& G, const PgWork& W, const double (*T)[16], double (*e)[6], double* r) {
  for (int k = tm.rank(); k < G.m; k += tm.size()) {
    if (!W.active[k]) continue;
    double Ti[16], P[16], M[16];
    pg_rigid_inv(T[G.dst[k]], Ti);
    pg_mul(W.Xinv[k], Ti, P);
    pg_mul(P, T[G.src[k]], M);
    pg_lin6(M, e[k]);
    r[k] = pg_quad(G.edge_info + 36 * k, e[k]);
  }
  tm.sync();
}

// sum over the active edges of c r + w (sqrt(c) - 1)^2, in edge order (every thread, the same number).  It reads conf and r
// of every edge: nobody may write either before a sync() that all its readers have passed.
PG_HD inline double pg_residual(const PgGraph& G, const PgWork& W, const double* r, double w) {
  double s = 0.0;
  for (int k = 0; k < G.m; ++k)
    if (W.active[k]) {
      const double q = sqrt(W.conf[k]) - 1.0;
      s += W.conf[k] * r[k] + w * (q * q);
    }
  return s;
}

// Enters with a sync: every thread has finished the sums it takes over ALL edges from the old confidences and from r
// (pg_residual, which the caller runs on every thread just before) by the time thread k overwrites conf[k].  Leaves with one:
// the new confidences are there for pg_linear_system.
template <class Team>
PG_HD void pg_update_confidence(const Team& tm, const PgGraph& G, PgWork& W, double w) {
  tm.sync();
  for (int k = tm.rank(); k < G.m; k += tm.size())
    if (W.active[k] && G.uncertain[k]) {
      const double t = w / (w + W.r[k]);
      W.conf[k] = t * t;
    }
  tm.sync();
}

// H and b from the poses W.T, the errors W.e and the confidences
template <class Team>
PG_HD void pg_linear_system(const Team& tm, const PgGraph& G, PgWork& W) {
  for (int k = tm.rank(); k < G.m; k += tm.size()) {
    if (!W.active[k]) continue;
    double Ti[16], P[16], J[36];                    // J[6 r + i] = Js[r][i]
    pg_rigid_inv(W.T[G.dst[k]], Ti);
    pg_mul(W.Xinv[k], Ti, P);
    const double* Ts = W.T[G.src[k]];
    for (int i = 0; i < 6; ++i) {
      double GT[16], M[16], v[6];
      for (int c = 0; c < 16; ++c) GT[c] = 0.0;
      // rows of G_i T_s: the generator about x has (1,2) = -1, (2,1) = 1, and so on cyclically; G_3 .. G_5 have a one at (i - 3, 3)
      if (i < 3) {
        const int a = (i + 1) % 3, c2 = (i + 2) % 3;
        for (int c = 0; c < 4; ++c) { GT[4 * a + c] = -Ts[4 * c2 + c]; GT[4 * c2 + c] = Ts[4 * a + c]; }
      } else {
        for (int c = 0; c < 4; ++c) GT[4 * (i - 3) + c] = Ts[12 + c];
      }
      pg_mul(P, GT, M);
      pg_lin6(M, v);
      for (int rr = 0; rr < 6; ++rr) J[6 * rr + i] = v[rr];
    }
    const double* I = G.edge_info + 36 * k;
    double IJ[36], Ie[6];                           // I Js, I e
    for (int rr = 0; rr < 6; ++rr) {
      for (int i = 0; i < 6; ++i) {
        double s = I[6 * rr] * J[i];
        for (int q = 1; q < 6; ++q) s += I[6 * rr + q] * J[6 * q + i];
        IJ[6 * rr + i] = s;
      }
      double s = I[6 * rr] * W.e[k][0];
      for (int q = 1; q < 6; ++q) s += I[6 * rr + q] * W.e[k][q];
      Ie[rr] = s;
    }
    for (int i = 0; i < 6; ++i) {
      for (int j = 0; j < 6; ++j) {
        double s = J[i] * IJ[j];
        for (int q = 1; q < 6; ++q) s += J[6 * q + i] * IJ[6 * q + j];
        W.A[k][6 * i + j] = s;
      }
      double s = J[i] * Ie[0];
      for (int q = 1; q < 6; ++q) s += J[6 * q + i] * Ie[q];
      W.g[k][i] = s;
    }
  }
  tm.sync();
  // Jt = -Js: the four blocks of an edge are +-c A, the two right-hand sides -+c g.  One thread per entry, edges in order.
  const int N = 6 * G.n;
  for (int idx = tm.rank(); idx < N * N + N; idx += tm.size()) {
    double s = 0.0;
    if (idx < N * N) {
      const int i = idx / N, j = idx % N, a = i / 6, c = j / 6, ii = i % 6, jj = j % 6;
      for (int k = 0; k < G.m; ++k) {
        if (!W.active[k]) continue;
        const int sn = G.src[k], tn = G.dst[k];
        if (a == c) {
          if (sn == a || tn == a) s += W.conf[k] * W.A[k][6 * ii + jj];
        } else if ((sn == a && tn == c) || (tn == a && sn == c)) {
          s -= W.conf[k] * W.A[k][6 * ii + jj];
        }
      }
      W.H[i * PG_DIM + j] = s;
    } else {
      const int i = idx - N * N, a = i / 6, ii = i % 6;
      for (int k = 0; k < G.m; ++k) {
        if (!W.active[k]) continue;
        if (G.src[k] == a) s -= W.conf[k] * W.g[k][ii];
        if (G.dst[k] == a) s += W.conf[k] * W.g[k][ii];
      }
      W.b[i] = s;
    }
  }
  tm.sync();
}

// (H + lambda I) delta = b by L D L^T without pivoting; false when a pivot is not positive and finite
template <class Team>
PG_HD bool pg_solve(const Team& tm, int N, PgWork& W, double lambda) {
  for (int idx = tm.rank(); idx < N * N; idx += tm.size()) {
    const int i = idx / N, j = idx % N;
    W.L[i * PG_DIM + j] = W.H[i * PG_DIM + j] + (i == j ? lambda : 0.0);
  }
  for (int i = tm.rank(); i < N; i += tm.size()) W.y[i] = W.b[i];
  tm.sync();
  for (int j = 0; j < N; ++j) {
    const double d = W.L[j * PG_DIM + j];
    if (!(d > 0.0) || !(d < INFINITY)) return false;                 // uniform: every thread reads the same d
    for (int i = j + 1 + tm.rank(); i < N; i += tm.size()) {
      W.col[i] = W.L[i * PG_DIM + j];
      W.L[i * PG_DIM + j] = W.col[i] / d;
    }
    tm.sync();
    const int R = N - j - 1;
    for (int idx = tm.rank(); idx < R * R; idx += tm.size()) {
      const int i = j + 1 + idx / R, k = j + 1 + idx % R;
      if (k <= i) W.L[i * PG_DIM + k] -= W.L[i * PG_DIM + j] * W.col[k];
    }
    tm.sync();
  }
  // L y = b, column by column
  for (int j = 0; j < N; ++j) {
    for (int i = j + 1 + tm.rank(); i < N; i += tm.size()) W.y[i] -= W.L[i * PG_DIM + j] * W.y[j];
    tm.sync();
  }
  for (int i = tm.rank(); i < N; i += tm.size()) W.delta[i] = W.y[i] / W.L[i * PG_DIM + i];
  tm.sync();
  // L^T delta = y / D, from the last column back
  for (int j = N - 1; j > 0; --j) {
    for (int i = tm.rank(); i < j; i += tm.size()) W.delta[i] -= W.L[j * PG_DIM + i] * W.delta[j];
    tm.sync();
  }
  return true;
}

PG_HD inline double pg_max(const double* v, int n) {
  double m = v[0];
  for (int i = 1; i < n; ++i) m = v[i] > m ? v[i] : m;
  return m;
}

PG_HD inline double pg_norm(const double* v, int n) {
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += v[i] * v[i];
  return sqrt(s);
}

// One pass over the active edges from the poses W.T and the confidences W.conf.  Returns PG_OK, PG_NO_CORRESPONDENCE
// (w == 0, nothing done) or PG_BREAKDOWN; *solves counts the linear solves, *residual is the final one.
template <class Team>
PG_HD int pg_pass(const Team& tm, const PgGraph& G, PgWork& W, const PgParams& P, double* solves, double* residual_out) {
  const int N = 6 * G.n;
  *solves = 0.0;
  *residual_out = 0.0;
  double info55 = 0.0;
  int n_active = 0;
  for (int k = 0; k < G.m; ++k)
    if (W.active[k]) { info55 += G.edge_info[36 * k + 35]; ++n_active; }
  const double w = n_active > 0 ? P.preference_loop_closure * (P.max_correspondence_distance * P.max_correspondence_distance) *
                                      (info55 / (double)n_active)
                                : 0.0;
  if (!(w > 0.0)) return PG_NO_CORRESPONDENCE;
  pg_errors(tm, G, W, W.T, W.e, W.r);
  double residual = pg_residual(G, W, W.r, w);                       // every thread; update_confidence syncs before it writes
  pg_update_confidence(tm, G, W, w);
  pg_linear_system(tm, G, W);
  double dmax = W.H[0];
  for (int i = 1; i < N; ++i) dmax = W.H[i * PG_DIM + i] > dmax ? W.H[i * PG_DIM + i] : dmax;
  double lambda = 1e-5 * dmax, nu = 2.0;
  for (int i = tm.rank(); i < G.n; i += tm.size()) pg_mat2vec(W.T[i], W.x + 6 * i);
  tm.sync();
  *residual_out = residual;
  if (pg_max(W.b, N) < P.min_right_term) return PG_OK;
  bool stop = false;
  for (int iter = 0; !stop; ++iter) {
    int trials = 0;
    double rho = 0.0;
    do {
      if (!pg_solve(tm, N, W, lambda)) return PG_BREAKDOWN;
      *solves += 1.0;
      if (pg_norm(W.delta, N) < P.min_relative_increment * (pg_norm(W.x, N) + P.min_relative_increment)) {
        stop = true;
      } else {
        for (int i = tm.rank(); i < G.n; i += tm.size()) {
          double U[16];
          pg_vec2mat(W.delta + 6 * i, U);
          pg_mul(U, W.T[i], W.T_new[i]);
        }
        tm.sync();
        pg_errors(tm, G, W, W.T_new, W.e_new, W.r_new);
        const double fresh = pg_residual(G, W, W.r_new, w);
        double den = 0.0;
        for (int i = 0; i < N; ++i) den += W.delta[i] * (lambda * W.delta[i] + W.b[i]);
        rho = (residual - fresh) / (den + 1e-3);
        if (rho > 0.0) {
          if (residual - fresh < P.min_relative_residual_increment * residual) { stop = true; break; }
          double alpha = 2.0 * rho - 1.0;
          alpha = 1.0 - alpha * alpha * alpha;
          alpha = alpha < P.upper_scale_factor ? alpha : P.upper_scale_factor;
          lambda *= P.lower_scale_factor > alpha ? P.lower_scale_factor : alpha;
          nu = 2.0;
          residual = fresh;
          tm.sync();                                                 // everyone has read delta, b and r_new
          for (int idx = tm.rank(); idx < 16 * G.n; idx += tm.size()) W.T[idx / 16][idx % 16] = W.T_new[idx / 16][idx % 16];
          for (int idx = tm.rank(); idx < 6 * G.m; idx += tm.size()) W.e[idx / 6][idx % 6] = W.e_new[idx / 6][idx % 6];
          for (int k = tm.rank(); k < G.m; k += tm.size()) W.r[k] = W.r_new[k];
          tm.sync();
          for (int i = tm.rank(); i < G.n; i += tm.size()) pg_mat2vec(W.T[i], W.x + 6 * i);
          pg_update_confidence(tm, G, W, w);
          pg_linear_system(tm, G, W);
          *residual_out = residual;
          if (pg_max(W.b, N) < P.min_right_term) { stop = true; break; }
        } else {
          lambda *= nu;
          nu *= 2.0;
        }
      }
      ++trials;
      stop = stop || trials >= P.max_iteration_lm;
    } while (!(rho > 0.0 || stop));
    stop = stop || residual < P.min_residual || iter >= P.max_iteration;
  }
  return PG_OK;
}

// The whole of global_optimization for one graph.  poses [n, 16], conf [m], kept [m], stats [PG_STATS], status [1].
template <class Team>
PG_HD void pg_global_optimization(const Team& tm, const PgGraph& G, PgWork& W, const PgParams& P, double* poses, double* conf,
                                  int* kept, double* stats, int* status) {
  if (tm.rank() == 0) W.bad = 0;
  tm.sync();
  // a non-finite input: x - x is 0 for every finite x
  int bad = 0;
  for (int idx = tm.rank(); idx < 16 * G.n; idx += tm.size()) bad |= !(G.nodes[idx] - G.nodes[idx] == 0.0);
  for (int idx = tm.rank(); idx < 16 * G.m; idx += tm.size()) bad |= !(G.edge_T[idx] - G.edge_T[idx] == 0.0);
  for (int idx = tm.rank(); idx < 36 * G.m; idx += tm.size()) bad |= !(G.edge_info[idx] - G.edge_info[idx] == 0.0);
  if (bad) W.bad = 1;                                                 // every writer writes the same value
  for (int idx = tm.rank(); idx < 16 * G.n; idx += tm.size()) W.T[idx / 16][idx % 16] = G.nodes[idx];
  for (int k = tm.rank(); k < G.m; k += tm.size()) {
    pg_rigid_inv(G.edge_T + 16 * k, W.Xinv[k]);
    W.conf[k] = 1.0;
    W.active[k] = 1;
  }
  tm.sync();
  int st = W.bad ? PG_NON_FINITE : PG_OK;
  double solves[2] = {0.0, 0.0}, residual = 0.0;
  if (st == PG_OK) st = pg_pass(tm, G, W, P, &solves[0], &residual);
  if (st == PG_OK) {
    tm.sync();
    for (int k = tm.rank(); k < G.m; k += tm.size()) W.active[k] = !G.uncertain[k] || W.conf[k] > P.edge_prune_threshold;
    tm.sync();
    st = pg_pass(tm, G, W, P, &solves[1], &residual);
  }
  tm.sync();
  if (st == PG_OK) {
    // T_i <- T_ref(input) T_ref(result)^-1 T_i(result)
    double Ri[16], F[16];
    pg_rigid_inv(W.T[P.reference_node], Ri);
    pg_mul(G.nodes + 16 * P.reference_node, Ri, F);
    for (int i = tm.rank(); i < G.n; i += tm.size()) pg_mul(F, W.T[i], poses + 16 * i);
    for (int k = tm.rank(); k < G.m; k += tm.size()) {
      conf[k] = W.conf[k];
      kept[k] = W.active[k];
    }
  } else {
    for (int idx = tm.rank(); idx < 16 * G.n; idx += tm.size()) poses[idx] = G.nodes[idx];
    for (int k = tm.rank(); k < G.m; k += tm.size()) {
      conf[k] = 1.0;
      kept[k] = 1;
    }
    solves[0] = solves[1] = residual = 0.0;
  }
  if (tm.rank() == 0) {
    stats[0] = solves[0];
    stats[1] = solves[1];
    stats[2] = residual;
    *status = st;
  }
}

}  // namespace gcl
