// The host set-up of the algebraic multigrid (csrc/amg.hip solves with what this file builds).
//
// Plain C++ on std::vector, free of HIP: tests/host/amg_setup_check.cpp runs it under the sanitizers on the CPU.
//   set-up (host, once): the degree-1 stiffness matrix is assembled from the operator's geometry
//     tensor (trilinear hexahedra with the 2-point GLL rule: a 7..27-point stencil); smoothed
//     aggregation (Vanek, Mandel, Brezina 1996) builds the hierarchy: strength graph
//     |a_ij| >= theta sqrt(a_ii a_jj), greedy aggregation, piecewise-constant tentative
//     prolongator, one damped-Jacobi smoothing step P = (I - 4/(3 rho) D^-1 A) T, Galerkin
//     product P^T A P; the last level is inverted densely.  Dirichlet rows (identity rows of the
//     operator) stay out of the coarse spaces.
//
// Every sparse row -- a product's, a prolongator's, one gathered from other ranks -- is made by build_rows; what moves
// between ranks is written and read in two halves, the all-reduce between them left to the caller.  A function that
// can refuse its input returns the refusal's text (empty: accepted).
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace pmg
{
namespace amg_setup
{
struct StageTimer
{
  bool on = std::getenv("PMG_AMG_TIMING") != nullptr;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  const char* tag = "set-up"; // ("update": the laps of pmg_amg_update_values)
  void lap(const char* what)
  {
    if (!on)
      return;
    const auto t1 = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[pmg_amg %s] %-28s %8.1f ms\n", tag, what, std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
  }
};

struct HostCsr
{
  int n = 0, m = 0; // rows, columns
  std::vector<int> rp, ci;
  std::vector<double> v;
  long long nnz() const { return (long long)ci.size(); }
};

// ---- host threads for the set-up ------------------------------------------------------------
// The set-up runs on the host.  Its row-wise loops are cut into fixed blocks of rows that a few threads pull from a
// counter; every block's result depends on the block alone and partial sums are combined in block order, so the
// hierarchy is bit-identical whatever the number of threads -- which the replicated form relies on: every rank must
// build the same hierarchy.
inline int host_threads()
{
  static int cached = 0;
  if (cached == 0)
  {
    int n = (int)std::thread::hardware_concurrency();
    if (n < 1)
      n = 1;
    if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) // the container's CPU quota, not the host's core count
    {
      char q[32] = {0};
      long long per = 0;
      if (std::fscanf(f, "%31s %lld", q, &per) == 2 && std::strcmp(q, "max") != 0 && per > 0)
        n = std::min<long long>(n, std::max<long long>(1, (std::atoll(q) + per / 2) / per));
      std::fclose(f);
    }
    n = std::min(n, 16);
    if (const char* e = std::getenv("PMG_HOST_THREADS"))
      n = std::max(1, std::atoi(e));
    cached = n;
  }
  return cached;
}
constexpr int ROW_BLOCK = 4096;
// f(block, first row, last row (exclusive), thread) for every block of [0, n)
template <typename F>
void for_row_blocks(int n, F f)
{
  const int nb = (n + ROW_BLOCK - 1) / ROW_BLOCK;
  const int T = std::min(host_threads(), std::max(nb, 1));
  if (T <= 1)
  {
    for (int b = 0; b < nb; ++b)
      f(b, b * ROW_BLOCK, std::min(n, (b + 1) * ROW_BLOCK), 0);
    return;
  }
  std::atomic<int> next(0);
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t)
    th.emplace_back([&, t] {
      for (int b = next.fetch_add(1); b < nb; b = next.fetch_add(1))
        f(b, b * ROW_BLOCK, std::min(n, (b + 1) * ROW_BLOCK), t);
    });
  for (auto& x : th)
    x.join();
}
// rows produced block by block -> one CSR matrix (row lengths in C.rp[i + 1] on entry)
inline void assemble_blocks(HostCsr& C, const std::vector<std::vector<int>>& bci, const std::vector<std::vector<double>>& bv)
{
  for (int i = 0; i < C.n; ++i)
    C.rp[i + 1] += C.rp[i];
  C.ci.resize(C.rp[C.n]);
  C.v.resize(C.rp[C.n]);
  for_row_blocks(C.n, [&](int b, int r0, int, int) {
    std::copy(bci[b].begin(), bci[b].end(), C.ci.begin() + C.rp[r0]);
    std::copy(bv[b].begin(), bv[b].end(), C.v.begin() + C.rp[r0]);
  });
}

// The one row builder: an [n x m] matrix whose row i is what fill(i, add) adds through add(column, value).  Entries of
// one column are summed in the order they arrive, from 0.0; the row is stored sorted by column, without its exact
// zeros where drop_zeros is set.  Columns must lie in [0, m).
template <typename Fill>
HostCsr build_rows(int n, int m, bool drop_zeros, Fill fill)
{
  HostCsr C;
  C.n = n;
  C.m = m;
  C.rp.assign(n + 1, 0);
  const int nb = (n + ROW_BLOCK - 1) / ROW_BLOCK, T = host_threads();
  std::vector<std::vector<int>> bci(nb), marker(T);
  std::vector<std::vector<double>> bv(nb), acc(T);
  for_row_blocks(n, [&](int blk, int r0, int r1, int t) {
    if (marker[t].empty())
    {
      marker[t].assign(std::max(m, 1), -1);
      acc[t].assign(std::max(m, 1), 0.0);
    }
    std::vector<int>& mk = marker[t];
    std::vector<double>& ac = acc[t];
    std::vector<int> cols;
    for (int i = r0; i < r1; ++i)
    {
      cols.clear();
      auto add = [&](int c, double val) {
        if (mk[c] != i)
        {
          mk[c] = i;
          ac[c] = 0.0;
          cols.push_back(c);
        }
        ac[c] += val;
      };
      fill(i, add);
      std::sort(cols.begin(), cols.end());
      int len = 0;
      for (int c : cols)
        if (!drop_zeros || ac[c] != 0.0)
        {
          bci[blk].push_back(c);
          bv[blk].push_back(ac[c]);
          ++len;
        }
      C.rp[i + 1] = len;
    }
  });
  assemble_blocks(C, bci, bv);
  return C;
}

// ---- host sparse algebra -------------------------------------------------------------------
inline HostCsr transpose(const HostCsr& A)
{
  HostCsr T;
  T.n = A.m;
  T.m = A.n;
  T.rp.assign(T.n + 1, 0);
  for (int c : A.ci)
    T.rp[c + 1]++;
  for (int i = 0; i < T.n; ++i)
    T.rp[i + 1] += T.rp[i];
  T.ci.resize(A.ci.size());
  T.v.resize(A.v.size());
  std::vector<int> pos(T.rp.begin(), T.rp.end() - 1);
  for (int i = 0; i < A.n; ++i)
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k)
    {
      const int p = pos[A.ci[k]]++;
      T.ci[p] = i;
      T.v[p] = A.v[k];
    }
  return T;
}

// C = A B (Gustavson), rows sorted by column, explicit zeros kept
inline HostCsr spgemm(const HostCsr& A, const HostCsr& B)
{
  return build_rows(A.n, B.m, false, [&](int i, auto& add) {
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k)
    {
      const int j = A.ci[k];
      const double a = A.v[k];
      for (int l = B.rp[j]; l < B.rp[j + 1]; ++l)
        add(B.ci[l], a * B.v[l]);
    }
  });
}

// the rows `rows[0 .. n)` of A, in that order; only the columns below `m` (the result's column count)
template <typename Index>
HostCsr take_rows(const HostCsr& A, const Index* rows, int n, int m)
{
  HostCsr C;
  C.n = n;
  C.m = m;
  C.rp.assign(n + 1, 0);
  for (int i = 0; i < n; ++i)
  {
    const int g = rows ? (int)rows[i] : i;
    for (int e = A.rp[g]; e < A.rp[g + 1]; ++e)
      if (A.ci[e] < m)
      {
        C.ci.push_back(A.ci[e]);
        C.v.push_back(A.v[e]);
      }
    C.rp[i + 1] = (int)C.ci.size();
  }
  return C;
}

inline std::vector<double> diagonal(const HostCsr& A)
{
  std::vector<double> d(A.n, 0.0);
  for (int i = 0; i < A.n; ++i)
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k)
      if (A.ci[k] == i)
        d[i] = A.v[k];
  return d;
}

// largest eigenvalue of D^-1 A by the power method (A SPD: D^-1 A has real positive eigenvalues);
// fixed seed and iteration count, so the hierarchy is reproducible
inline double lambda_max_jacobi(const HostCsr& A, const std::vector<double>& d, int its)
{
  const int n = A.n;
  if (n == 0)
    return 1.0;
  std::mt19937_64 gen(12345);
  std::uniform_real_distribution<double> U(0.5, 1.0);
  std::vector<double> x(n), y(n);
  for (double& v : x)
    v = U(gen);
  double lam = 1.0;
  const int nb = (n + ROW_BLOCK - 1) / ROW_BLOCK;
  std::vector<double> py(nb), px(nb);
  for (int it = 0; it < its; ++it)
  {
    for_row_blocks(n, [&](int blk, int r0, int r1, int) {
      double sy = 0, sx = 0;
      for (int i = r0; i < r1; ++i)
      {
        double s = 0;
        for (int k = A.rp[i]; k < A.rp[i + 1]; ++k)
          s += A.v[k] * x[A.ci[k]];
        y[i] = s / d[i];
        sy += y[i] * y[i];
        sx += x[i] * x[i];
      }
      py[blk] = sy;
      px[blk] = sx;
    });
    double nrm = 0, xn = 0;
    for (int blk = 0; blk < nb; ++blk) // block order: the same sums whatever the number of threads
    {
      nrm += py[blk];
      xn += px[blk];
    }
    nrm = std::sqrt(nrm);
    if (!(nrm > 0))
      return 1.0;
    lam = nrm / std::sqrt(xn);
    for_row_blocks(n, [&](int, int r0, int r1, int) {
      for (int i = r0; i < r1; ++i)
        x[i] = y[i] / nrm;
    });
  }
  return lam;
}

// Greedy aggregation on the strength graph.  agg[i] = aggregate of node i, -1 = the node takes no
// part in the coarse space (no strong connection: Dirichlet rows, isolated nodes).
inline int aggregate(const HostCsr& A, const std::vector<double>& d, double theta, std::vector<int>& agg)
{
  const int n = A.n;
  std::vector<int> srp(n + 1, 0), sci;
  std::vector<double> sw;
  for (int i = 0; i < n; ++i)
  {
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k)
    {
      const int j = A.ci[k];
      if (j != i && std::fabs(A.v[k]) >= theta * std::sqrt(std::fabs(d[i] * d[j])) && A.v[k] != 0.0)
      {
        sci.push_back(j);
        sw.push_back(std::fabs(A.v[k]));
      }
    }
    srp[i + 1] = (int)sci.size();
  }
  agg.assign(n, -2); // -2 = undecided
  int na = 0;
  for (int i = 0; i < n; ++i)
    if (srp[i] == srp[i + 1])
      agg[i] = -1;
  // pass 1: a node whose whole strong neighbourhood is free becomes a root
  for (int i = 0; i < n; ++i)
  {
    if (agg[i] != -2)
      continue;
    bool free_nb = true;
    for (int k = srp[i]; k < srp[i + 1] && free_nb; ++k)
      free_nb = agg[sci[k]] == -2;
    if (!free_nb)
      continue;
    agg[i] = na;
    for (int k = srp[i]; k < srp[i + 1]; ++k)
      agg[sci[k]] = na;
    ++na;
  }
  // pass 2: leftovers join the aggregate (of pass 1) they are most strongly tied to
  std::vector<int> agg1(agg);
  for (int i = 0; i < n; ++i)
  {
    if (agg[i] != -2)
      continue;
    double best = 0;
    int to = -2;
    for (int k = srp[i]; k < srp[i + 1]; ++k)
      if (agg1[sci[k]] >= 0 && sw[k] > best)
      {
        best = sw[k];
        to = agg1[sci[k]];
      }
    if (to >= 0)
      agg[i] = to;
  }
  // pass 3: what is still free forms aggregates of its own
  for (int i = 0; i < n; ++i)
  {
    if (agg[i] != -2)
      continue;
    agg[i] = na;
    for (int k = srp[i]; k < srp[i + 1]; ++k)
      if (agg[sci[k]] == -2)
        agg[sci[k]] = na;
    ++na;
  }
  return na;
}

// the normalised piecewise-constant tentative prolongator: T[i, agg[i]] = 1 / sqrt(size of the aggregate)
inline std::vector<double> tentative_weights(const std::vector<int>& agg, int na)
{
  std::vector<int> size(std::max(na, 1), 0);
  for (int a : agg)
    if (a >= 0)
      size[a]++;
  std::vector<double> t(agg.size(), 0.0);
  for (size_t i = 0; i < agg.size(); ++i)
    if (agg[i] >= 0)
      t[i] = 1.0 / std::sqrt((double)size[agg[i]]);
  return t;
}

// P = (I - omega D^-1 A) T: the rows of A (its columns may go beyond them: the ghosts of a rank), agg[j] and t[j] the
// aggregate number (< 0: none) and the weight of column j, d the diagonal of the rows; exact zeros are not stored
inline HostCsr smoothed_prolongator(const HostCsr& A, const std::vector<double>& d, const std::vector<int>& agg,
                                    const std::vector<double>& t, int na, double omega)
{
  return build_rows(A.n, na, true, [&](int i, auto& add) {
    if (agg[i] < 0)
      return;
    add(agg[i], t[i]);
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k)
    {
      const int j = A.ci[k];
      if (agg[j] >= 0)
        add(agg[j], -omega * A.v[k] / d[i] * t[j]);
    }
  });
}

// dense inverse of an SPD matrix by Cholesky (n <= a few thousand); returns false if not SPD
// ... of the dense matrix L [n x n] (its lower triangle is read), factorised in place
inline bool dense_spd_inverse(int n, std::vector<double>& L, std::vector<double>& inv)
{
  for (int j = 0; j < n; ++j) // in-place lower Cholesky
  {
    double s = L[(size_t)j * n + j];
    for (int k = 0; k < j; ++k)
      s -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
    if (!(s > 0.0))
      return false;
    const double ljj = std::sqrt(s);
    L[(size_t)j * n + j] = ljj;
    for (int i = j + 1; i < n; ++i)
    {
      double t = L[(size_t)i * n + j];
      for (int k = 0; k < j; ++k)
        t -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
      L[(size_t)i * n + j] = t / ljj;
    }
  }
  inv.assign((size_t)n * n, 0.0);
  std::vector<double> col(n);
  for (int c = 0; c < n; ++c) // solve L L^T x = e_c
  {
    for (int i = 0; i < n; ++i)
    {
      double t = (i == c) ? 1.0 : 0.0;
      for (int k = 0; k < i; ++k)
        t -= L[(size_t)i * n + k] * col[k];
      col[i] = t / L[(size_t)i * n + i];
    }
    for (int i = n - 1; i >= 0; --i)
    {
      double t = col[i];
      for (int k = i + 1; k < n; ++k)
        t -= L[(size_t)k * n + i] * col[k];
      col[i] = t / L[(size_t)i * n + i];
    }
    for (int i = 0; i < n; ++i)
      inv[(size_t)i * n + c] = col[i];
  }
  return true;
}
inline std::vector<double> dense_of(const HostCsr& A)
{
  const int n = A.n;
  std::vector<double> D((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i)
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k)
      D[(size_t)i * n + A.ci[k]] = A.v[k];
  return D;
}
inline bool dense_spd_inverse(const HostCsr& A, std::vector<double>& inv)
{
  std::vector<double> L = dense_of(A);
  return dense_spd_inverse(A.n, L, inv);
}

// ---- level 0 ---------------------------------------------------------------------------------
// The owned block [n rows] of the degree-1 stiffness matrix of the listed cells, from host copies of the operator's
// data: dofmap [cells x 8], G [cells x 8 points x 6], kappa [cells], bc [total], react (nullptr: none) [n] the
// operator's diagonal term.  Ghost rows are another rank's; ghost columns are kept (total columns) where the
// hierarchy is `replicated` and dropped (n columns) from a rank-local one.
inline HostCsr assemble_level0(const std::vector<int32_t>& dofmap, const std::vector<double>& G,
                               const std::vector<double>& kappa, const std::vector<int8_t>& bc,
                               const std::vector<int32_t>& cells, const double* react, int n, int total, bool replicated)
{
  constexpr int W = 32; // row capacity of the table (a trilinear hex mesh has <= 27); what is longer spills
  std::vector<int> cnt(n, 0), cols((size_t)n * W, -1);
  std::vector<double> vals((size_t)n * W, 0.0);
  std::map<int, std::vector<std::pair<int, double>>> spill; // by row
  auto add = [&](int row, int col, double v) {
    int* rc = cols.data() + (size_t)row * W;
    double* rv = vals.data() + (size_t)row * W;
    const int c = cnt[row];
    for (int k = 0; k < c; ++k)
      if (rc[k] == col)
      {
        rv[k] += v;
        return;
      }
    if (c < W)
    {
      rc[c] = col;
      rv[c] = v;
      cnt[row] = c + 1;
      return;
    }
    for (auto& e : spill[row])
      if (e.first == col)
      {
        e.second += v;
        return;
      }
    spill[row].emplace_back(col, v);
  };
  for (int32_t c : cells)
  {
    const int32_t* dm = dofmap.data() + (size_t)c * 8;
    const double* Gc = G.data() + (size_t)c * 48;
    double Ke[8][8] = {};
    // collocated basis on the 2-point GLL rule: at quadrature point q only the basis functions of
    // q itself and of its three axis neighbours have a gradient; l_0' = -1, l_1' = +1
    for (int q = 0; q < 8; ++q)
    {
      const double* g = Gc + q * 6; // (G00, G01, G02, G11, G12, G22), src/laplacian.hpp:99-111
      const double Gm[3][3] = {{g[0], g[1], g[2]}, {g[1], g[3], g[4]}, {g[2], g[4], g[5]}};
      const int qa = (q >> 2) & 1, qb = (q >> 1) & 1, qc = q & 1;
      const int node[4] = {q, q ^ 4, q ^ 2, q ^ 1};
      const double sa = qa ? 1.0 : -1.0, sb = qb ? 1.0 : -1.0, sc = qc ? 1.0 : -1.0;
      const double grad[4][3] = {{sa, sb, sc}, {-sa, 0, 0}, {0, -sb, 0}, {0, 0, -sc}};
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
        {
          double v = 0;
          for (int d = 0; d < 3; ++d)
            for (int e = 0; e < 3; ++e)
              v += grad[i][d] * Gm[d][e] * grad[j][e];
          Ke[node[i]][node[j]] += kappa[c] * v;
        }
    }
    for (int i = 0; i < 8; ++i)
    {
      const int row = dm[i];
      if (row >= n || bc[row])
        continue; // ghost rows are another rank's; Dirichlet rows are identity rows
      for (int j = 0; j < 8; ++j)
      {
        const int col = dm[j];
        if (bc[col] || (!replicated && col >= n))
          continue; // Dirichlet columns: masked; ghost columns: dropped from a rank-local hierarchy
        add(row, col, Ke[i][j]);
      }
    }
  }
  // the diagonal term of the operator (pmg_laplacian_set_reaction, pmg_laplacian_set_robin): its vector on the diagonal
  // of the owned, unmarked rows (the vector is zero on marked dofs; a row no cell lists keeps its identity)
  if (react)
    for (int i = 0; i < n; ++i)
      if (!bc[i] && cnt[i] > 0 && react[i] != 0.0)
        add(i, i, react[i]);
  HostCsr A0;
  A0.n = n;
  A0.m = replicated ? total : n;
  A0.rp.assign(n + 1, 0);
  std::vector<std::pair<int, double>> row;
  for (int i = 0; i < n; ++i)
  {
    row.clear();
    for (int k = 0; k < cnt[i]; ++k)
      row.emplace_back(cols[(size_t)i * W + k], vals[(size_t)i * W + k]);
    if (cnt[i] == W && spill.count(i))
      row.insert(row.end(), spill[i].begin(), spill[i].end());
    if (row.empty())
      row.emplace_back(i, 1.0); // Dirichlet dof, or a dof of no listed cell: identity row
    std::sort(row.begin(), row.end());
    for (auto& e : row)
    {
      A0.ci.push_back(e.first);
      A0.v.push_back(e.second);
    }
    A0.rp[i + 1] = (int)A0.ci.size();
  }
  return A0;
}

// ---- the coarsening loop ---------------------------------------------------------------------
struct Hierarchy
{
  std::vector<HostCsr> A, P; // A_l, and P_l: level l + 1 -> l
  std::vector<double> lmax;  // the smoothing bound of every level: 1.05 x 20 power steps on D^-1 A_l
};
// theta0: strength threshold of the first coarsening done here (halved from level to level)
inline std::string coarsen(HostCsr&& A0, double theta0, Hierarchy& H)
{
  StageTimer tm;
  const int max_levels = 12, coarsest_max = 800;
  H.A.push_back(std::move(A0));
  double theta = theta0;
  while (true)
  {
    const HostCsr& A = H.A.back();
    const std::vector<double> d = diagonal(A);
    for (int i = 0; i < A.n; ++i)
      if (!(d[i] > 0.0))
        return "pmg_amg_create: non-positive diagonal entry on level " + std::to_string(H.A.size() - 1);
    const double rho = 1.05 * lambda_max_jacobi(A, d, 20);
    tm.lap("power method");
    H.lmax.push_back(rho);
    if (A.n <= coarsest_max || (int)H.A.size() >= max_levels)
      break;
    std::vector<int> agg;
    const int na = aggregate(A, d, theta, agg);
    tm.lap("aggregation");
    if (na == 0 || na >= A.n)
      break; // nothing to coarsen
    HostCsr P = smoothed_prolongator(A, d, agg, tentative_weights(agg, na), na, 4.0 / (3.0 * rho));
    tm.lap("smoothed prolongator");
    HostCsr R = transpose(P);
    tm.lap("transpose");
    HostCsr AP = spgemm(A, P);
    tm.lap("A P");
    HostCsr Ac = spgemm(R, AP);
    tm.lap("R (A P)");
    H.P.push_back(std::move(P));
    H.A.push_back(std::move(Ac));
    theta *= 0.5;
  }
  tm.lap("(levels done)");
  return "";
}

// ---- between the ranks: what is written before the caller's all-reduce (a sum) and read after it -------------------
// The maximum of a small non-negative integer (< slots) from sums: a unary code.
inline std::vector<double> unary_code(int v, int slots)
{
  std::vector<double> code(slots, 0.0);
  code[v] = 1.0;
  return code;
}
inline int unary_max(const std::vector<double>& code)
{
  int m = 0;
  for (int w = 0; w < (int)code.size(); ++w)
    if (code[w] > 0.0)
      m = w;
  return m;
}

inline int longest_row(const HostCsr& A)
{
  int w = 0;
  for (int i = 0; i < A.n; ++i)
    w = std::max(w, A.rp[i + 1] - A.rp[i]);
  return w;
}

// Rows as padded (column + 1, value) slot tables of width W, 0 = empty: row i of A goes to row row_of(i) of the zeroed
// tables gc, gv, its column c as col_of(c) + 1.
template <typename RowOf, typename ColOf>
void rows_to_slots(const HostCsr& A, int W, RowOf row_of, ColOf col_of, std::vector<double>& gc, std::vector<double>& gv)
{
  for (int i = 0; i < A.n; ++i)
  {
    const size_t g = (size_t)row_of(i);
    int k = 0;
    for (int e = A.rp[i]; e < A.rp[i + 1]; ++e, ++k)
    {
      gc[g * W + k] = (double)(col_of(A.ci[e]) + 1);
      gv[g * W + k] = A.v[e];
    }
  }
}
// ... and back: the [n x m] matrix of the tables.  *bad = a column outside [0, m) that a slot names (-1: none); the
// matrix is not built then.
inline HostCsr rows_from_slots(const std::vector<double>& gc, const std::vector<double>& gv, int n, int W, int m,
                               long long* bad)
{
  *bad = -1;
  for (size_t k = 0; k < (size_t)n * W; ++k)
    if (gc[k] > 0.5 && !(gc[k] - 0.5 < (double)m))
      *bad = (long long)(gc[k] - 0.5);
  if (*bad >= 0)
    return HostCsr();
  return build_rows(n, m, false, [&](int g, auto& add) {
    for (int k = 0; k < W; ++k)
      if (gc[(size_t)g * W + k] > 0.5)
        add((int)(gc[(size_t)g * W + k] - 0.5), gv[(size_t)g * W + k]);
  });
}
// the last empty row of A, -1 if it has none
inline int empty_row(const HostCsr& A)
{
  for (int i = A.n - 1; i >= 0; --i)
    if (A.rp[i] == A.rp[i + 1])
      return i;
  return -1;
}

// The keyed gather of an [n1 x n1] matrix that is the sum of the ranks' shares: (row * n1 + column + 1, value) pairs,
// every rank's in a segment of its own of one long array.  The segments are ordered by a key that every rank marks with
// its entry count (+ 0.25: a rank with an empty share still marks its key) in a summed marker vector.
inline void segment_of(const std::vector<double>& marker, int64_t mykey, long long* offset, long long* total)
{
  *offset = *total = 0;
  for (size_t g = 0; g < marker.size(); ++g)
    if (marker[g] > 0.0)
    {
      const long long c = (long long)marker[g];
      if ((int64_t)g < mykey)
        *offset += c;
      *total += c;
    }
}
inline void write_segment(const HostCsr& share, long long offset, std::vector<double>& keys, std::vector<double>& vals)
{
  long long o = offset;
  for (int I = 0; I < share.n; ++I)
    for (int e = share.rp[I]; e < share.rp[I + 1]; ++e, ++o)
    {
      keys[(size_t)o] = (double)((long long)I * share.m + share.ci[e]) + 1.0; // + 1: 0 = empty
      vals[(size_t)o] = share.v[e];
    }
}
// bucket by row, then every row sorted by column with its duplicates added in the order of the segments: the same sums
// on every rank
inline std::string rows_from_segments(const std::vector<double>& keys, const std::vector<double>& vals, int n1, HostCsr& A1)
{
  const size_t cnt = keys.size();
  std::vector<int> rstart(n1 + 1, 0);
  for (size_t o = 0; o < cnt; ++o)
  {
    if (!(keys[o] > 0.5))
      return "pmg_amg_create_distributed: two ranks share a segment of the gather";
    rstart[(int)(((long long)(keys[o] - 0.5)) / n1) + 1]++;
  }
  for (int I = 0; I < n1; ++I)
    rstart[I + 1] += rstart[I];
  std::vector<int> ecol(cnt);
  std::vector<double> eval(cnt);
  std::vector<int> pos(rstart.begin(), rstart.end() - 1);
  for (size_t o = 0; o < cnt; ++o)
  {
    const long long k = (long long)(keys[o] - 0.5);
    const int I = (int)(k / n1), J = (int)(k - (long long)I * n1);
    const int p = pos[I]++;
    ecol[(size_t)p] = J;
    eval[(size_t)p] = vals[o];
  }
  A1 = build_rows(n1, n1, false, [&](int I, auto& add) {
    for (int p = rstart[I]; p < rstart[I + 1]; ++p)
      add(ecol[(size_t)p], eval[(size_t)p]);
  });
  return "";
}

// ---- the constant null space -------------------------------------------------------------------
// The coarsest-level matrix of a hierarchy whose level 0 (n0 rows) has the constants as its null space (DESIGN.md
// section 19): v = P_{L-2}^T ... P_0^T 1, the ones restricted through the hierarchy's own transfers, and
// D = A_c + gamma v v^T with gamma = max diag(A_c) / (v^T v), dense.  Returns 0, 1 where the transfers do not end on
// the coarsest level, 2 where the restricted ones vanish.
inline int nullspace_shifted(int n0, const std::vector<HostCsr>& Ps, const HostCsr& Ac, std::vector<double>& D)
{
  std::vector<double> v((size_t)n0, 1.0);
  for (const HostCsr& P : Ps) // v <- P^T v
  {
    std::vector<double> c((size_t)P.m, 0.0);
    for (int i = 0; i < P.n; ++i)
      for (int k = P.rp[i]; k < P.rp[i + 1]; ++k)
        c[P.ci[k]] += P.v[k] * v[i];
    v.swap(c);
  }
  const int n = Ac.n;
  if ((int)v.size() != n)
    return 1;
  double vv = 0.0, dmax = 0.0;
  for (int i = 0; i < n; ++i)
    vv += v[i] * v[i];
  for (double d : diagonal(Ac))
    dmax = std::max(dmax, d);
  if (!(vv > 0.0) || !(dmax > 0.0))
    return 2;
  const double gamma = dmax / vv;
  D = dense_of(Ac);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      D[(size_t)i * n + j] += gamma * v[i] * v[j];
  return 0;
}
} // namespace amg_setup
} // namespace pmg
