// The renewal of an AMG hierarchy (csrc/amg_renew.hpp) run whole on the host: tests/test_amg_update_host.py compiles
// this program under the address and undefined-behaviour sanitizers and compares what it writes with scipy.
//
//   amg_update_check CASE OUT
//
// CASE (written by the test): int32 ncells, ndofs; int32 dofmap[ncells x 8]; int8 bc[ndofs]; double kappa[ncells];
// double G[ncells x 8 x 6] the hierarchy is created for; double G[ncells x 8 x 6] and double react[ndofs] after the
// change.  One rank, every cell listed.
// The program creates the hierarchy (amg_setup.hpp), plans the renewal, and runs one update through the row routines
// the device kernels call -- one lane per row, the rows in the blocks of the set-up's threaded loops.
// OUT: int32 L; the created A_l; then the renewed A_l, P_l, R_l, (A P)_l as int32 rows, columns, nnz, rowptr, colidx,
// double values; the permutation of every R_l (int32 nnz, int32[nnz]); double bound[L].
// Then a hand-made matrix with a negative diagonal entry: the update must refuse its level; and one with a row longer
// than the kernels' row copy: the plan must refuse it, naming the length.
// Exit status 0 and "OK" on success.
#include "amg_renew.hpp"

#include <fstream>

using namespace pmg::amg_setup;
using namespace pmg::amg_renew;

template <typename T>
static std::vector<T> get(std::ifstream& f, size_t count)
{
  std::vector<T> v(count);
  f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(sizeof(T) * count));
  if (!f)
  {
    std::fprintf(stderr, "the case file is too short\n");
    std::exit(2);
  }
  return v;
}
template <typename T>
static void put(std::ofstream& f, const std::vector<T>& v)
{
  f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(sizeof(T) * v.size()));
}
static void put(std::ofstream& f, const HostCsr& M)
{
  put(f, std::vector<int32_t>{M.n, M.m, (int32_t)M.nnz()});
  put(f, M.rp);
  put(f, M.ci);
  put(f, M.v);
}

// the longest row of M as a row copy
static std::vector<std::vector<double>> row_copies(const HostCsr& M)
{
  return std::vector<std::vector<double>>(host_threads(), std::vector<double>(std::max(longest_row(M), 1)));
}

// 20 power steps as the device takes them, the sums in block order
static double power_bound(const HostCsr& A, const std::vector<double>& dinv, std::vector<double> x)
{
  const int n = A.n;
  if (n == 0)
    return 1.0;
  std::vector<double> y(n);
  const int nb = (n + ROW_BLOCK - 1) / ROW_BLOCK;
  std::vector<double> py(nb), px(nb);
  double lam = 1.0;
  for (int it = 0; it < 20; ++it)
  {
    for_row_blocks(n, [&](int blk, int r0, int r1, int) {
      double sy = 0, sx = 0;
      for (int i = r0; i < r1; ++i)
      {
        y[i] = row_dot(i, 0, 1, A.rp.data(), A.ci.data(), A.v.data(), x.data()) * dinv[i];
        sy += y[i] * y[i];
        sx += x[i] * x[i];
      }
      py[blk] = sy;
      px[blk] = sx;
    });
    double nrm = 0, xn = 0;
    for (int blk = 0; blk < nb; ++blk)
    {
      nrm += py[blk];
      xn += px[blk];
    }
    nrm = std::sqrt(nrm);
    if (!(nrm > 0))
      return 1.0;
    lam = nrm / std::sqrt(xn);
    for (int i = 0; i < n; ++i)
      x[i] = y[i] / nrm;
  }
  return lam;
}

// The levels below a level 0 whose values and inverse diagonal are in place: the sequence of pmg_amg_update_values.
// Returns the refusal's text (empty: done).
static std::string renew_levels(RenewPlan& plan, std::vector<double> dinv, std::vector<double>& bound)
{
  const int L = (int)plan.A.size();
  bound.assign(L, 0.0);
  for (int l = 0; l < L; ++l)
  {
    HostCsr& A = plan.A[l];
    for (int i = 0; i < A.n; ++i)
      if (!(dinv[i] > 0.0))
        return "non-positive diagonal entry on level " + std::to_string(l);
    bound[l] = 1.05 * power_bound(A, dinv, plan.x0[l]);
    if (l + 1 == L)
      break;
    RenewLevel& lv = plan.lv[l];
    const double omega = 4.0 / (3.0 * bound[l]);
    for_row_blocks(A.n, [&](int, int r0, int r1, int) {
      for (int i = r0; i < r1; ++i)
        prolongator_row(i, 0, 1, A.rp.data(), A.ci.data(), A.v.data(), lv.agg.data(), lv.t.data(), omega, lv.P.rp.data(),
                        lv.P.ci.data(), lv.P.v.data());
    });
    for (size_t p = 0; p < lv.rperm.size(); ++p)
      lv.R.v[p] = lv.P.v[lv.rperm[p]];
    auto acc = row_copies(lv.AP);
    for_row_blocks(A.n, [&](int, int r0, int r1, int t) {
      for (int i = r0; i < r1; ++i)
      {
        product_row(i, 0, 1, A.rp.data(), A.ci.data(), A.v.data(), lv.P.rp.data(), lv.P.ci.data(), lv.P.v.data(),
                    lv.AP.rp.data(), lv.AP.ci.data(), acc[t].data());
        store_row(i, 0, 1, lv.AP.rp.data(), lv.AP.ci.data(), acc[t].data(), lv.AP.v.data(), nullptr);
      }
    });
    HostCsr& Ac = plan.A[l + 1];
    dinv.assign(Ac.n, 0.0);
    acc = row_copies(Ac);
    for_row_blocks(Ac.n, [&](int, int r0, int r1, int t) {
      for (int i = r0; i < r1; ++i)
      {
        product_row(i, 0, 1, lv.R.rp.data(), lv.R.ci.data(), lv.R.v.data(), lv.AP.rp.data(), lv.AP.ci.data(),
                    lv.AP.v.data(), Ac.rp.data(), Ac.ci.data(), acc[t].data());
        store_row(i, 0, 1, Ac.rp.data(), Ac.ci.data(), acc[t].data(), Ac.v.data(), dinv.data());
      }
    });
  }
  return "";
}

// a 3 x 3 tridiagonal matrix with diagonal (2, -1, 2): one level, refused
static bool negative_diagonal_is_refused()
{
  HostCsr A;
  A.n = A.m = 3;
  A.rp = {0, 2, 5, 7};
  A.ci = {0, 1, 0, 1, 2, 1, 2};
  A.v = {2.0, -0.5, -0.5, -1.0, -0.5, -0.5, 2.0};
  RenewPlan plan;
  plan.A.push_back(A);
  plan.x0.push_back(power_start(3));
  std::vector<double> dinv(3, -1.0), acc(3), bound;
  for (int i = 0; i < 3; ++i)
  {
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k)
      acc[k - A.rp[i]] = A.v[k];
    store_row(i, 0, 1, A.rp.data(), A.ci.data(), acc.data(), plan.A[0].v.data(), dinv.data());
  }
  const std::string refused = renew_levels(plan, dinv, bound);
  return dinv[0] == 0.5 && dinv[1] == 0.0 && dinv[2] == 0.5 && refused == "non-positive diagonal entry on level 0";
}

// a one-level matrix whose first row has 8200 entries, more than the row copy of the kernels holds: the plan refuses
// it and names the length
static bool long_row_is_refused()
{
  const int n = 8200;
  HostCsr A;
  A.n = A.m = n;
  A.rp.assign(n + 1, 0);
  for (int j = 0; j < n; ++j)
  {
    A.ci.push_back(j);
    A.v.push_back(j == 0 ? (double)n : -0.5);
  }
  A.rp[1] = n;
  for (int i = 1; i < n; ++i)
  {
    A.ci.insert(A.ci.end(), {0, i});
    A.v.insert(A.v.end(), {-0.5, 2.0});
    A.rp[i + 1] = (int)A.ci.size();
  }
  RenewPlan plan;
  const std::string refused = plan_renewal({A}, {}, {}, plan);
  return refused.find("a row of level 0 has 8200 entries") != std::string::npos;
}

int main(int argc, char** argv)
{
  if (argc != 3)
  {
    std::fprintf(stderr, "usage: %s CASE OUT\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1], std::ios::binary);
  const std::vector<int32_t> head = get<int32_t>(in, 2);
  const int ncells = head[0], n = head[1];
  const std::vector<int32_t> dofmap = get<int32_t>(in, (size_t)ncells * 8);
  const std::vector<int8_t> bc = get<int8_t>(in, (size_t)n);
  const std::vector<double> kappa = get<double>(in, (size_t)ncells), G0 = get<double>(in, (size_t)ncells * 48),
                            G1 = get<double>(in, (size_t)ncells * 48), react = get<double>(in, (size_t)n);
  std::vector<int32_t> cells(ncells);
  for (int c = 0; c < ncells; ++c)
    cells[c] = c;

  Hierarchy H;
  std::string refused = coarsen(assemble_level0(dofmap, G0, kappa, bc, cells, nullptr, n, n, false), 0.08, H);
  if (!refused.empty())
  {
    std::fprintf(stderr, "refused: %s\n", refused.c_str());
    return 1;
  }
  RenewPlan plan;
  refused = plan_renewal(H.A, dofmap, cells, plan);
  if (!refused.empty())
  {
    std::fprintf(stderr, "refused: %s\n", refused.c_str());
    return 1;
  }
  // level 0 from the changed data
  HostCsr& A0 = plan.A[0];
  std::vector<double> dinv(n, 0.0);
  {
    auto acc = row_copies(A0);
    for_row_blocks(n, [&](int, int r0, int r1, int t) {
      for (int i = r0; i < r1; ++i)
      {
        level0_row(i, 0, 1, A0.rp.data(), A0.ci.data(), plan.inc_off.data(), plan.inc_cell.data(), plan.inc_loc.data(),
                   dofmap.data(), G1.data(), kappa.data(), bc.data(), react.data(), acc[t].data());
        store_row(i, 0, 1, A0.rp.data(), A0.ci.data(), acc[t].data(), A0.v.data(), dinv.data());
      }
    });
  }
  std::vector<double> bound;
  refused = renew_levels(plan, dinv, bound);
  if (!refused.empty())
  {
    std::fprintf(stderr, "refused: %s\n", refused.c_str());
    return 1;
  }
  std::ofstream out(argv[2], std::ios::binary);
  const int L = (int)plan.A.size();
  put(out, std::vector<int32_t>{L});
  for (const HostCsr& A : H.A)
    put(out, A);
  for (const HostCsr& A : plan.A)
    put(out, A);
  for (const RenewLevel& lv : plan.lv)
    put(out, lv.P);
  for (const RenewLevel& lv : plan.lv)
    put(out, lv.R);
  for (const RenewLevel& lv : plan.lv)
    put(out, lv.AP);
  for (const RenewLevel& lv : plan.lv)
  {
    put(out, std::vector<int32_t>{(int32_t)lv.rperm.size()});
    put(out, lv.rperm);
  }
  put(out, bound);
  out.close();
  const bool negative = negative_diagonal_is_refused(), longrow = long_row_is_refused();
  std::printf("levels %d threads %d negative diagonal %s long row %s\n", L, host_threads(),
              negative ? "refused" : "ACCEPTED", longrow ? "refused" : "ACCEPTED");
  if (!out || !negative || !longrow)
    return 1;
  std::printf("OK\n");
  return 0;
}
