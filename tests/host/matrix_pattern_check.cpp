// The host pattern of the assembled operator and its diag / off-diag split (csrc/matrix_pattern.hpp) run on their own,
// host only: tests/test_matrix_pattern_host.py compiles this program under the address and undefined-behaviour
// sanitizers and compares what it writes with the oracle's pattern.
//
//   matrix_pattern_check CASE OUT
//
// CASE (written by the test, one rank's level): int32 ncells, N, size_local, num_ghosts, n_applied;
// int32 dofmap[ncells x N]; int32 applied[n_applied] (the cells the operator applies, ascending).
// OUT: int32 rows, cols, nnz, n_boundary; int32 rowptr[rows + 1], colidx[nnz], off_diag_offset[rows],
// boundary_rows[n_boundary]; int32 inc_off[rows + 1].
// Then the two-phase product of matrix.hip -- the owned columns of every row stored, the ghost columns of the boundary
// rows added -- executed serially on small-integer values and a small-integer vector: it must equal the one-pass
// product exactly, and must leave the ghost entries of its output alone.  Exit status 0 and "OK" on success.
#include "matrix_pattern.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>

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
static int bad(const char* what, long long at)
{
  std::fprintf(stderr, "FAILED: %s (at %lld)\n", what, at);
  return 1;
}

int main(int argc, char** argv)
{
  if (argc != 3)
  {
    std::fprintf(stderr, "usage: matrix_pattern_check CASE OUT\n");
    return 2;
  }
  std::ifstream in(argv[1], std::ios::binary);
  const std::vector<int32_t> head = get<int32_t>(in, 5);
  const int32_t ncells = head[0], N = head[1], n = head[2], ncols = head[2] + head[3], n_applied = head[4];
  const std::vector<int32_t> dofmap = get<int32_t>(in, (size_t)ncells * N);
  const std::vector<int32_t> cells = get<int32_t>(in, (size_t)n_applied);
  for (int32_t c : cells)
    if (c < 0 || c >= ncells)
      return bad("an applied cell out of range", c);
  for (int32_t d : dofmap)
    if (d < 0 || d >= ncols)
      return bad("a dofmap entry out of range", d);

  std::vector<int32_t> inc_off, inc_cell, inc_loc, rp, ci, od, brows;
  int longest = 0;
  const long long nnz =
      pmg::matrix_pattern(n, ncols, N, cells, dofmap.data(), inc_off, inc_cell, inc_loc, rp, ci, &longest);
  if (nnz != (long long)ci.size() || (n > 0 && rp[n] != nnz))
    return bad("nnz and the arrays disagree", nnz);
  pmg::matrix_split(n, rp, ci, od, brows);

  // what the kernels rely on: incidences of owned rows only, name the row; sorted rows that hold their diagonal;
  // the split inside its row; the longest row
  int seen_longest = 0;
  for (int32_t i = 0; i < n; ++i)
  {
    for (int32_t m = inc_off[i]; m < inc_off[i + 1]; ++m)
    {
      if (dofmap[(size_t)inc_cell[m] * N + inc_loc[m]] != i)
        return bad("an incidence does not name its row", i);
      if (m > inc_off[i] && inc_cell[m] <= inc_cell[m - 1])
        return bad("incidences not in ascending cell order", i);
    }
    bool diag = false;
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k)
    {
      if (k > rp[i] && ci[k] <= ci[k - 1])
        return bad("columns not strictly ascending", i);
      if (ci[k] < 0 || ci[k] >= ncols)
        return bad("a column out of range", i);
      diag = diag || ci[k] == i;
    }
    if (!diag)
      return bad("a row without its diagonal", i);
    if (od[i] < rp[i] || od[i] > rp[i + 1])
      return bad("off_diag_offset outside its row", i);
    seen_longest = std::max(seen_longest, rp[i + 1] - rp[i]);
  }
  if (seen_longest != longest)
    return bad("the longest row", longest);

  // the two-phase product on exact values
  std::vector<double> v((size_t)nnz), x((size_t)ncols), one((size_t)ncols, 9.0), two((size_t)ncols, 9.0);
  for (long long k = 0; k < nnz; ++k)
    v[(size_t)k] = (double)((k * 7 + 3) % 9 - 4);
  for (int32_t j = 0; j < ncols; ++j)
    x[j] = (double)((j * 5 + 1) % 7 - 3);
  for (int32_t i = 0; i < n; ++i)
  {
    double acc = 0.0;
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k)
      acc += v[k] * x[ci[k]];
    one[i] = acc;
  }
  for (int32_t i = 0; i < n; ++i) // the diag phase: every row over [rp[i], od[i]), stored
  {
    double acc = 0.0;
    for (int32_t k = rp[i]; k < od[i]; ++k)
    {
      if (ci[k] >= n)
        return bad("a ghost column in the diag phase", i);
      acc += v[k] * x[ci[k]];
    }
    two[i] = acc;
  }
  long long off_terms = 0;
  for (int32_t r : brows) // the off-diag phase: the boundary rows over [od[r], rp[r + 1]), added
  {
    double acc = 0.0;
    for (int32_t k = od[r]; k < rp[r + 1]; ++k)
    {
      if (ci[k] < n)
        return bad("an owned column in the off-diag phase", r);
      acc += v[k] * x[ci[k]];
      ++off_terms;
    }
    two[r] += acc;
  }
  for (int32_t i = 0; i < ncols; ++i)
    if (one[i] != two[i])
      return bad("the two-phase product differs from the one-pass product", i);
  for (int32_t i = n; i < ncols; ++i)
    if (two[i] != 9.0)
      return bad("a ghost entry of the output was written", i);

  std::ofstream out(argv[2], std::ios::binary);
  put(out, std::vector<int32_t>{n, ncols, (int32_t)nnz, (int32_t)brows.size()});
  put(out, rp);
  put(out, ci);
  put(out, od);
  put(out, brows);
  put(out, inc_off);
  std::printf("rows %d cols %d nnz %lld boundary rows %zu off-diag terms %lld lanes %d %d\nOK\n", n, ncols, nnz,
              brows.size(), off_terms, pmg::matrix_lanes_per_row(n ? (double)nnz / n : 1.0),
              pmg::matrix_lanes_per_row(brows.empty() ? 1.0 : (double)off_terms / (double)brows.size()));
  return 0;
}
