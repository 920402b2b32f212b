// The AMG host set-up (csrc/amg_setup.hpp) run on its own, host only: tests/test_amg_setup_host.py compiles this
// program under the address and undefined-behaviour sanitizers and compares what it writes with the numpy restatement.
//
//   amg_setup_check CASE OUT
//
// CASE (written by the test): int32 ncells, ndofs; int32 dofmap[ncells x 8]; int8 bc[ndofs]; double kappa[ncells];
// double G[ncells x 8 x 6].  One rank, every cell listed, no diagonal term.
// OUT: int32 L; every A_l, then every P_l, as int32 rows, columns, nnz, rowptr[rows + 1], colidx[nnz], double
// values[nnz]; double bound[L].
// Then both gathers between two synthetic ranks (the rows of A_0 cut in two), the tables added here in place of the
// all-reduce: the matrix must come back entry for entry.  Exit status 0 and "OK" on success.
#include "amg_setup.hpp"

#include <fstream>

using namespace pmg::amg_setup;

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

static bool same(const HostCsr& A, const HostCsr& B)
{
  return A.n == B.n && A.m == B.m && A.rp == B.rp && A.ci == B.ci && A.v == B.v;
}
static void add_to(std::vector<double>& sum, const std::vector<double>& part)
{
  for (size_t k = 0; k < sum.size(); ++k)
    sum[k] += part[k];
}
// rows [r0, r1) of A, the other rows empty
static HostCsr rows_of_rank(const HostCsr& A, int r0, int r1)
{
  HostCsr S;
  S.n = A.n, S.m = A.m;
  S.rp.assign(A.n + 1, 0);
  for (int i = 0; i < A.n; ++i)
  {
    if (i >= r0 && i < r1)
      for (int e = A.rp[i]; e < A.rp[i + 1]; ++e)
      {
        S.ci.push_back(A.ci[e]);
        S.v.push_back(A.v[e]);
      }
    S.rp[i + 1] = (int)S.ci.size();
  }
  return S;
}

// the padded slot tables: each rank writes its rows, the tables are summed, the sum is decoded
static bool slots_round_trip(const HostCsr& A)
{
  const int half = A.n / 2, bounds[3] = {0, half, A.n};
  std::vector<double> code(256, 0.0);
  for (int r = 0; r < 2; ++r)
    add_to(code, unary_code(longest_row(rows_of_rank(A, bounds[r], bounds[r + 1])), 256));
  const int W = unary_max(code);
  if (W != longest_row(A))
    return false;
  std::vector<double> gc((size_t)A.n * W, 0.0), gv(gc);
  auto id = [](int i) { return i; };
  for (int r = 0; r < 2; ++r)
  {
    std::vector<double> c((size_t)A.n * W, 0.0), v(c);
    rows_to_slots(rows_of_rank(A, bounds[r], bounds[r + 1]), W, id, id, c, v);
    add_to(gc, c);
    add_to(gv, v);
  }
  long long bad = 0;
  const HostCsr B = rows_from_slots(gc, gv, A.n, W, A.m, &bad);
  return bad < 0 && empty_row(B) < 0 && same(A, B);
}

// the keyed segments: rank 0 holds the entries at even positions, rank 1 those at odd ones, and each one half of every
// diagonal entry (0.5 v + 0.5 v == v), so that the decoder has repeated columns to add
static bool segments_round_trip(const HostCsr& A)
{
  HostCsr share[2];
  for (int r = 0; r < 2; ++r)
  {
    share[r].n = A.n, share[r].m = A.m;
    share[r].rp.assign(A.n + 1, 0);
    for (int i = 0; i < A.n; ++i)
    {
      for (int e = A.rp[i]; e < A.rp[i + 1]; ++e)
        if (A.ci[e] == i || (e & 1) == r)
        {
          share[r].ci.push_back(A.ci[e]);
          share[r].v.push_back(A.ci[e] == i ? 0.5 * A.v[e] : A.v[e]);
        }
      share[r].rp[i + 1] = (int)share[r].ci.size();
    }
  }
  const int64_t key[2] = {0, A.n / 2}; // the smallest global dof each rank owns
  std::vector<double> marker(A.n, 0.0);
  for (int r = 0; r < 2; ++r)
    marker[(size_t)key[r]] += (double)share[r].nnz() + 0.25;
  long long offset[2], total[2];
  for (int r = 0; r < 2; ++r)
    segment_of(marker, key[r], &offset[r], &total[r]);
  if (total[0] != total[1] || total[0] != share[0].nnz() + share[1].nnz() || offset[0] != 0 || offset[1] != share[0].nnz())
    return false;
  std::vector<double> keys((size_t)total[0], 0.0), vals(keys);
  for (int r = 0; r < 2; ++r)
  {
    std::vector<double> k((size_t)total[0], 0.0), v(k);
    write_segment(share[r], offset[r], k, v);
    add_to(keys, k);
    add_to(vals, v);
  }
  HostCsr B;
  return rows_from_segments(keys, vals, A.n, B).empty() && same(A, B);
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
  const std::vector<double> kappa = get<double>(in, (size_t)ncells), G = get<double>(in, (size_t)ncells * 48);
  std::vector<int32_t> cells(ncells);
  for (int c = 0; c < ncells; ++c)
    cells[c] = c;

  HostCsr A0 = assemble_level0(dofmap, G, kappa, bc, cells, nullptr, n, n, false);
  const bool slots = slots_round_trip(A0), segments = segments_round_trip(A0);
  Hierarchy H;
  const std::string refused = coarsen(std::move(A0), 0.08, H);
  if (!refused.empty())
  {
    std::fprintf(stderr, "refused: %s\n", refused.c_str());
    return 1;
  }
  std::ofstream out(argv[2], std::ios::binary);
  put(out, std::vector<int32_t>{(int32_t)H.A.size()});
  for (const HostCsr& A : H.A)
    put(out, A);
  for (const HostCsr& P : H.P)
    put(out, P);
  put(out, H.lmax);
  out.close();
  std::printf("levels %d threads %d slots %s segments %s\n", (int)H.A.size(), host_threads(), slots ? "back" : "LOST",
              segments ? "back" : "LOST");
  if (!out || !slots || !segments)
    return 1;
  std::printf("OK\n");
  return 0;
}
