// The sparsity pattern of the assembled operator (matrix.hip) and its diag / off-diag split, on the host: plain C++ on
// std::vector, no HIP call, so a stand-alone program can include this header alone
// (tests/host/matrix_pattern_check.cpp).
//
// Rows are the n owned dofs; columns are local indices in [0, ncols), ncols = n + ghosts, sorted within a row, so the
// ghost columns of a row come last and one position per row -- off_diag_offset, the array of src/csr.hpp:114-126 --
// splits it into the part a product can form before the halo has arrived and the part that needs it.
#pragma once

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pmg
{
// The pattern of dolfinx's create_sparsity_pattern from a dofmap: dof -> (cell, local node) incidences in ascending
// cell order, kept for the rows [0, n) only (a ghost dof is a column, never a row), then per row the sorted distinct
// dofs of its cells, ghost cells included (a row no listed cell touches keeps its diagonal).  Every dofmap entry of a
// listed cell lies in [0, ncols).  Returns the nnz; the arrays are filled only while it fits int32.
inline long long matrix_pattern(int32_t n, int32_t ncols, int N, const std::vector<int32_t>& cells,
                                const int32_t* dofmap, std::vector<int32_t>& inc_off, std::vector<int32_t>& inc_cell,
                                std::vector<int32_t>& inc_loc, std::vector<int32_t>& rp, std::vector<int32_t>& ci,
                                int* longest)
{
  inc_off.assign((size_t)n + 1, 0);
  for (int32_t c : cells)
    for (int t = 0; t < N; ++t)
    {
      const int32_t d = dofmap[(size_t)c * N + t];
      if (d < n)
        inc_off[(size_t)d + 1]++;
    }
  for (int32_t i = 0; i < n; ++i)
    inc_off[i + 1] += inc_off[i];
  inc_cell.resize(inc_off[n]);
  inc_loc.resize(inc_off[n]);
  {
    std::vector<int32_t> at(inc_off.begin(), inc_off.end() - 1);
    for (int32_t c : cells) // ascending: the order of the sums
      for (int t = 0; t < N; ++t)
      {
        const int32_t d = dofmap[(size_t)c * N + t];
        if (d >= n)
          continue;
        const int32_t k = at[d]++;
        inc_cell[k] = c;
        inc_loc[k] = t;
      }
  }
  rp.assign((size_t)n + 1, 0);
  ci.clear();
  std::vector<int32_t> seen((size_t)std::max(ncols, n), -1), row;
  long long nnz = 0;
  *longest = 0;
  for (int32_t i = 0; i < n; ++i)
  {
    row.clear();
    row.push_back(i);
    seen[i] = i;
    for (int32_t m = inc_off[i]; m < inc_off[i + 1]; ++m)
    {
      const int32_t* dm = dofmap + (size_t)inc_cell[m] * N;
      for (int t = 0; t < N; ++t)
        if (seen[dm[t]] != i)
        {
          seen[dm[t]] = i;
          row.push_back(dm[t]);
        }
    }
    nnz += (long long)row.size();
    *longest = std::max(*longest, (int)row.size());
    if (nnz <= INT32_MAX)
    {
      std::sort(row.begin(), row.end());
      ci.insert(ci.end(), row.begin(), row.end());
      rp[i + 1] = (int32_t)nnz;
    }
  }
  return nnz;
}

// The split of a pattern with sorted rows: off_diag_offset[i] = the position in ci of row i's first column >= n
// (rp[i + 1] where it has none), and the ascending list of the boundary rows, those with at least one such column.
inline void matrix_split(int32_t n, const std::vector<int32_t>& rp, const std::vector<int32_t>& ci,
                         std::vector<int32_t>& off_diag_offset, std::vector<int32_t>& boundary_rows)
{
  off_diag_offset.assign((size_t)n, 0);
  boundary_rows.clear();
  for (int32_t i = 0; i < n; ++i)
  {
    const int32_t od = (int32_t)(std::lower_bound(ci.begin() + rp[i], ci.begin() + rp[i + 1], n) - ci.begin());
    off_diag_offset[i] = od;
    if (od < rp[i + 1])
      boundary_rows.push_back(i);
  }
}

// lanes of a wavefront that share a row whose column range has this mean length (a power of two, 4 .. 64)
inline int matrix_lanes_per_row(double mean)
{
  return mean > 96 ? 64 : mean > 48 ? 32 : mean > 20 ? 16 : mean > 10 ? 8 : 4;
}
} // namespace pmg
