// The renewal of an AMG hierarchy after a coefficient change (pmg_amg_update_values; csrc/amg.hip runs it on the
// device).  The aggregates of the creation are kept; every value is recomputed from the operator's current data.
//
// Two parts, both free of HIP calls, so tests/host/amg_update_check.cpp runs a whole update on the CPU under the
// sanitizers:
//   the plan (host, once)  the frozen aggregates and tentative weights, recomputed from the created matrices with the
//     creation's own deterministic `aggregate`; the STRUCTURAL patterns of P_l, R_l, (A P)_l and A_{l+1} -- the created
//     P_l stores no exact zero, so its pattern depends on the coefficient it was created for and cannot be reused.
//     A stored entry of A_l counts for P_l where SOME coefficient can make it non-zero (a "live" entry): all of them
//     but those of A_0 that only the body diagonal of a cell couples -- no quadrature point sees both ends of it, so
//     such an entry is an exact zero whatever the tensor -- and what only they reach further down --;
//     the permutation from the values of P_l to those of R_l; the incidence lists of level 0; the start vector of every
//     level's power method.
//   the row routines       one output row each, as plain functions on pointers.  `sub` of `W` lanes share a row: on the
//     device W lanes of one wavefront, on the host sub = 0, W = 1.  A row builds up in a copy `acc` (LDS on the device).
//     In a product the lanes take the entries of ONE row of the right factor, which are distinct columns, so their
//     updates never collide; the entries of the left factor follow in program order.  No atomics: the sums of an entry
//     are added in the same order whatever W is, and two updates from the same data give the same bytes.
#pragma once

#include "amg_setup.hpp"

#if defined(__HIPCC__)
#define PMG_HD __host__ __device__
#else
#define PMG_HD
#endif
// between two left-factor entries of a row: the next one's updates stay behind this one's (one wavefront, whose LDS
// operations retire in order)
#if defined(__HIP_DEVICE_COMPILE__)
#define PMG_ROW_FENCE() __builtin_amdgcn_wave_barrier()
#else
#define PMG_ROW_FENCE() ((void)0)
#endif

namespace pmg
{
// first position k in the sorted cols[0 .. len) with cols[k] >= col (where the pattern holds col: its position)
PMG_HD inline int row_position(const int32_t* __restrict__ cols, int len, int32_t col)
{
  int lo = 0, hi = len;
  while (lo < hi)
  {
    const int mid = (lo + hi) >> 1;
    if (cols[mid] < col)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

namespace amg_renew
{
using amg_setup::HostCsr;

constexpr size_t ROW_COPY_BYTES = 64 * 1024; // the LDS a workgroup can have: the longest row copy

// lanes per row from the mean row length (upload_csr of amg.hip)
inline int lanes_for(double mean)
{
  return mean > 48 ? 32 : mean > 24 ? 16 : mean > 10 ? 8 : mean > 4 ? 4 : 2;
}
inline int lanes_for(const HostCsr& B) { return lanes_for(B.n ? (double)B.nnz() / B.n : 1.0); }

// ---- the row routines ------------------------------------------------------------------------------------------
// The finished copy of a row goes to the matrix; with dinv, the inverse of its diagonal entry too (0 where the entry is
// not positive or not stored: the update refuses such a level).
PMG_HD inline void store_row(int row, int sub, int W, const int* __restrict__ rp, const int* __restrict__ ci,
                             const double* acc, double* __restrict__ vals, double* __restrict__ dinv)
{
  PMG_ROW_FENCE();
  const int rs = rp[row], len = rp[row + 1] - rs;
  for (int k = sub; k < len; k += W)
    vals[rs + k] = acc[k];
  if (dinv && sub == 0)
  {
    const int dpos = row_position(ci + rs, len, row);
    const double d = (dpos < len && ci[rs + dpos] == row) ? acc[dpos] : 0.0;
    dinv[row] = d > 0.0 ? 1.0 / d : 0.0;
  }
}

// Row `row` of A_0 on its kept pattern: the degree-1 element matrices in closed form, the sums of assemble_level0
// (amg_setup.hpp).  inc_*: the (cell, cell-local node) incidences of the row in ascending cell order, listed cells
// only; Gc [cell][8][6] the geometry tensor, kappa per cell, react the operator's diagonal vector (nullptr: none).
// At point q only the basis functions of q and of its three axis neighbours q ^ 4, q ^ 2, q ^ 1 have a gradient
// (l_0' = -1, l_1' = +1).  The pattern has no marked column and one entry in an identity row, so a position found by
// the search counts only where it holds the column searched for.
PMG_HD inline void point_gradient(int node, int q, double g[3])
{
  const double sa = (q & 4) ? 1.0 : -1.0, sb = (q & 2) ? 1.0 : -1.0, sc = (q & 1) ? 1.0 : -1.0;
  const int d = node ^ q;
  g[0] = d == 0 ? sa : d == 4 ? -sa : 0.0;
  g[1] = d == 0 ? sb : d == 2 ? -sb : 0.0;
  g[2] = d == 0 ? sc : d == 1 ? -sc : 0.0;
}
PMG_HD inline void level0_row(int row, int sub, int W, const int* __restrict__ rp, const int* __restrict__ ci,
                              const int* __restrict__ inc_off, const int* __restrict__ inc_cell,
                              const int* __restrict__ inc_loc, const int32_t* __restrict__ dofmap,
                              const double* __restrict__ Gc, const double* __restrict__ kappa,
                              const int8_t* __restrict__ bc, const double* __restrict__ react, double* acc)
{
  const int rs = rp[row], len = rp[row + 1] - rs;
  const int* cols = ci + rs;
  for (int k = sub; k < len; k += W)
    acc[k] = 0.0;
  PMG_ROW_FENCE();
  const int dpos = row_position(cols, len, row);
  const int m0 = inc_off[row], m1 = inc_off[row + 1];
  if (bc[row] || m0 == m1) // a marked dof, or a dof of no listed cell: the identity row
  {
    if (sub == 0 && dpos < len && cols[dpos] == row)
      acc[dpos] = 1.0;
    return;
  }
  for (int m = m0; m < m1; ++m)
  {
    const int cell = inc_cell[m], i = inc_loc[m];
    const double* G = Gc + (size_t)cell * 48;
    const int32_t* dm = dofmap + (size_t)cell * 8;
    const double kap = kappa[cell];
    for (int j = sub; j < 8; j += W)
    {
      const int32_t col = dm[j];
      if (bc[col])
        continue;
      double s = 0.0;
      for (int q = 0; q < 8; ++q)
      {
        const int di = i ^ q, dj = j ^ q;
        if ((di & (di - 1)) || (dj & (dj - 1))) // neither q nor an axis neighbour of q
          continue;
        double gi[3], gj[3];
        point_gradient(i, q, gi);
        point_gradient(j, q, gj);
        const double* g = G + q * 6; // (G00, G01, G02, G11, G12, G22)
        const double Gm[3][3] = {{g[0], g[1], g[2]}, {g[1], g[3], g[4]}, {g[2], g[4], g[5]}};
        double v = 0.0;
        for (int d = 0; d < 3; ++d)
          for (int e = 0; e < 3; ++e)
            v += gi[d] * Gm[d][e] * gj[e];
        s += v;
      }
      const int pos = row_position(cols, len, col);
      if (pos < len && cols[pos] == col)
        acc[pos] += kap * s;
    }
    PMG_ROW_FENCE();
  }
  if (react && sub == 0 && react[row] != 0.0 && dpos < len && cols[dpos] == row)
    acc[dpos] += react[row];
}

// this lane's share of (A x)[row]: the entries sub, sub + W, ...
PMG_HD inline double row_dot(int row, int sub, int W, const int* __restrict__ rp, const int* __restrict__ ci,
                             const double* __restrict__ v, const double* __restrict__ x)
{
  double s = 0.0;
  const int e = rp[row + 1];
  for (int k = rp[row] + sub; k < e; k += W)
    s += v[k] * x[ci[k]];
  return s;
}

// Row `row` of P = (I - omega D^-1 A) T on its structural pattern (an empty row where agg[row] < 0).  A lane takes the
// columns sub, sub + W, ... of the row and walks the row of A for each: the terms of an entry are added in the order of
// smoothed_prolongator (amg_setup.hpp), from 0.0, the tentative weight first.
PMG_HD inline void prolongator_row(int row, int sub, int W, const int* __restrict__ Arp, const int* __restrict__ Aci,
                                   const double* __restrict__ Av, const int* __restrict__ agg,
                                   const double* __restrict__ t, double omega, const int* __restrict__ Prp,
                                   const int* __restrict__ Pci, double* __restrict__ Pv)
{
  const int ps = Prp[row], plen = Prp[row + 1] - ps;
  if (plen == 0)
    return;
  const int as = Arp[row], ae = Arp[row + 1];
  double d = 0.0;
  for (int k = as; k < ae; ++k)
    if (Aci[k] == row)
      d = Av[k];
  for (int c = sub; c < plen; c += W)
  {
    const int a = Pci[ps + c];
    double s = 0.0;
    if (a == agg[row])
      s += t[row];
    for (int k = as; k < ae; ++k)
    {
      const int j = Aci[k];
      if (agg[j] == a)
        s += -omega * Av[k] / d * t[j];
    }
    Pv[ps + c] = s;
  }
}

// Row `row` of C = A B on the pattern of C (which holds every column the row reaches), into the copy acc.
PMG_HD inline void product_row(int row, int sub, int W, const int* __restrict__ Arp, const int* __restrict__ Aci,
                               const double* __restrict__ Av, const int* __restrict__ Brp,
                               const int* __restrict__ Bci, const double* __restrict__ Bv,
                               const int* __restrict__ Crp, const int* __restrict__ Cci, double* acc)
{
  const int cs = Crp[row], len = Crp[row + 1] - cs;
  const int* cols = Cci + cs;
  for (int k = sub; k < len; k += W)
    acc[k] = 0.0;
  PMG_ROW_FENCE();
  for (int k = Arp[row]; k < Arp[row + 1]; ++k)
  {
    const int j = Aci[k];
    const double a = Av[k];
    const int e = Brp[j + 1];
    for (int l = Brp[j] + sub; l < e; l += W)
    {
      const int pos = row_position(cols, len, Bci[l]);
      if (pos < len && cols[pos] == Bci[l])
        acc[pos] += a * Bv[l];
    }
    PMG_ROW_FENCE();
  }
}

// ---- the plan ----------------------------------------------------------------------------------------------------
struct RenewLevel // the transfer below level l
{
  std::vector<int> agg;  // frozen aggregates of level l (-1: outside the coarse space)
  std::vector<double> t; // ... and tentative weights
  int na = 0;
  HostCsr P, R, AP;       // structural patterns (their values: scratch of a host run)
  std::vector<int> rperm; // R.v[p] = P.v[rperm[p]]
};
struct RenewPlan
{
  std::vector<HostCsr> A;              // structural pattern of every level; A[0] is the created one
  std::vector<RenewLevel> lv;          // levels - 1 of them
  std::vector<std::vector<double>> x0; // start vector of every level's power method
  std::vector<int> inc_off, inc_cell, inc_loc; // level 0: dof -> (cell, cell-local node), ascending cell order
};

// The live entries of A_0, as a pattern inside A0's: the diagonal, and every (row, column) that two nodes i, j of a
// listed cell with i ^ j != 7 couple.  At quadrature point q only q and q ^ 1, q ^ 2, q ^ 4 have a gradient
// (level0_row), so a cell never couples the two ends of a body diagonal: where no other cell couples them, the stored
// entry is zero for every coefficient.
inline HostCsr live_level0(const HostCsr& A0, const std::vector<int32_t>& dofmap, const std::vector<int32_t>& cells)
{
  std::vector<char> live(A0.ci.size(), 0);
  auto mark = [&](int row, int col) {
    const int rs = A0.rp[row], len = A0.rp[row + 1] - rs;
    const int pos = row_position(A0.ci.data() + rs, len, col);
    if (pos < len && A0.ci[rs + pos] == col)
      live[rs + pos] = 1;
  };
  for (int i = 0; i < A0.n; ++i)
    mark(i, i);
  for (int32_t c : cells)
    for (int i = 0; i < 8; ++i)
    {
      const int32_t row = dofmap[(size_t)c * 8 + i];
      if (row < 0 || row >= A0.n)
        continue;
      for (int j = 0; j < 8; ++j)
        if ((i ^ j) != 7)
          mark(row, dofmap[(size_t)c * 8 + j]);
    }
  HostCsr Lv;
  Lv.n = A0.n;
  Lv.m = A0.m;
  Lv.rp.assign(A0.n + 1, 0);
  for (int i = 0; i < A0.n; ++i)
  {
    for (int k = A0.rp[i]; k < A0.rp[i + 1]; ++k)
      if (live[k])
        Lv.ci.push_back(A0.ci[k]);
    Lv.rp[i + 1] = (int)Lv.ci.size();
  }
  Lv.v.assign(Lv.ci.size(), 0.0);
  return Lv;
}

// the pattern of a matrix whose row i reaches the columns fill(i, reach) names, sorted
template <typename Fill>
HostCsr pattern_rows(int n, int m, Fill fill)
{
  return amg_setup::build_rows(n, m, false, [&](int i, auto& add) { fill(i, [&](int c) { add(c, 0.0); }); });
}
inline HostCsr pattern_product(const HostCsr& A, const HostCsr& B)
{
  return pattern_rows(A.n, B.m, [&](int i, auto reach) {
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k)
      for (int l = B.rp[A.ci[k]]; l < B.rp[A.ci[k] + 1]; ++l)
        reach(B.ci[l]);
  });
}
// the transposed pattern and where each of its entries comes from
inline HostCsr pattern_transpose(const HostCsr& P, std::vector<int>& from)
{
  HostCsr T;
  T.n = P.m;
  T.m = P.n;
  T.rp.assign(T.n + 1, 0);
  for (int c : P.ci)
    T.rp[c + 1]++;
  for (int i = 0; i < T.n; ++i)
    T.rp[i + 1] += T.rp[i];
  T.ci.resize(P.ci.size());
  T.v.assign(P.ci.size(), 0.0);
  from.resize(P.ci.size());
  std::vector<int> pos(T.rp.begin(), T.rp.end() - 1);
  for (int i = 0; i < P.n; ++i)
    for (int k = P.rp[i]; k < P.rp[i + 1]; ++k)
    {
      const int p = pos[P.ci[k]]++;
      T.ci[p] = i;
      from[p] = k;
    }
  return T;
}

inline std::vector<double> power_start(int n)
{
  std::mt19937_64 gen(12345); // lambda_max_jacobi's
  std::uniform_real_distribution<double> U(0.5, 1.0);
  std::vector<double> x(n);
  for (double& v : x)
    v = U(gen);
  return x;
}

// The plan of a hierarchy from its created matrices `created` (A_l with the values of the creation) and the level-0
// inputs: dofmap [cells x 8], the listed cells, n rows.  Returns the refusal's text (empty: accepted).
inline std::string plan_renewal(const std::vector<HostCsr>& created, const std::vector<int32_t>& dofmap,
                                const std::vector<int32_t>& cells, RenewPlan& plan)
{
  const int L = (int)created.size();
  if (L == 0)
    return "pmg_amg_update_values: the hierarchy has no level";
  plan = RenewPlan();
  plan.A.push_back(created[0]);
  HostCsr live = live_level0(created[0], dofmap, cells); // the live entries of A_l, inside plan.A[l]'s pattern
  double theta = 0.08;
  for (int l = 0; l + 1 < L; ++l, theta *= 0.5)
  {
    RenewLevel lv;
    lv.na = amg_setup::aggregate(created[l], amg_setup::diagonal(created[l]), theta, lv.agg);
    if (lv.na != created[l + 1].n)
      return "pmg_amg_update_values: internal: the aggregation of level " + std::to_string(l) + " gives " +
             std::to_string(lv.na) + " aggregates, the hierarchy has " + std::to_string(created[l + 1].n);
    lv.t = amg_setup::tentative_weights(lv.agg, lv.na);
    const HostCsr& A = plan.A[l];
    const std::vector<int>& agg = lv.agg;
    lv.P = pattern_rows(A.n, lv.na, [&](int i, auto reach) {
      if (agg[i] < 0)
        return;
      reach(agg[i]);
      for (int k = live.rp[i]; k < live.rp[i + 1]; ++k)
        if (agg[live.ci[k]] >= 0)
          reach(agg[live.ci[k]]);
    });
    lv.R = pattern_transpose(lv.P, lv.rperm);
    // the products are taken on the STORED pattern of A_l, as the creation's are: they contain the created ones
    lv.AP = pattern_product(A, lv.P);
    HostCsr Ac = pattern_product(lv.R, lv.AP);
    live = pattern_product(lv.R, pattern_product(live, lv.P));
    for (const HostCsr* C : {&lv.AP, &Ac})
    {
      const int w = amg_setup::longest_row(*C);
      if ((size_t)w * sizeof(double) > ROW_COPY_BYTES)
        return "pmg_amg_update_values: a row of a product of level " + std::to_string(l) + " has " + std::to_string(w) +
               " entries, more than the row copy holds (" + std::to_string(ROW_COPY_BYTES / sizeof(double)) + ")";
    }
    plan.lv.push_back(std::move(lv));
    plan.A.push_back(std::move(Ac));
  }
  for (const HostCsr& A : plan.A)
    plan.x0.push_back(power_start(A.n));
  {
    const int w = amg_setup::longest_row(plan.A[0]);
    if ((size_t)w * sizeof(double) > ROW_COPY_BYTES)
      return "pmg_amg_update_values: a row of level 0 has " + std::to_string(w) + " entries, more than the row copy holds";
  }
  // level 0: the incidences of every row, cells ascending (the order assemble_level0 is given them in does not matter
  // to the pattern; the sums of a renewal are in ascending cell order)
  const int n = plan.A[0].n;
  std::vector<int32_t> sorted(cells);
  std::sort(sorted.begin(), sorted.end());
  plan.inc_off.assign(n + 1, 0);
  for (int32_t c : sorted)
    for (int i = 0; i < 8; ++i)
    {
      const int32_t dof = dofmap[(size_t)c * 8 + i];
      if (dof >= 0 && dof < n)
        plan.inc_off[dof + 1]++;
    }
  for (int i = 0; i < n; ++i)
    plan.inc_off[i + 1] += plan.inc_off[i];
  plan.inc_cell.resize(plan.inc_off[n]);
  plan.inc_loc.resize(plan.inc_off[n]);
  std::vector<int> pos(plan.inc_off.begin(), plan.inc_off.end() - 1);
  for (int32_t c : sorted)
    for (int i = 0; i < 8; ++i)
    {
      const int32_t dof = dofmap[(size_t)c * 8 + i];
      if (dof >= 0 && dof < n)
      {
        plan.inc_cell[pos[dof]] = c;
        plan.inc_loc[pos[dof]++] = i;
      }
    }
  return "";
}
} // namespace amg_renew
} // namespace pmg
