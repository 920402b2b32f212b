// The drivers' diffusion tensor (--kappa-tensor): one symmetric positive-definite tensor per cell with eigenvalues
// (1, 2 + x, 4), rotated by Rz(0.6 + 0.8 y) Rx(0.4 + 0.5 z), at the cell centre (x, y, z) = the mean of the cell's
// eight vertices.  Returns [ncells][6] as (xx, xy, xz, yy, yz, zz), the layout of
// pmg_laplacian_set_coefficient_tensor.
#pragma once

#include "box_mesh.hpp"

#include <cmath>
#include <cstdint>
#include <vector>

namespace examples
{
inline std::vector<double> rotating_tensor(const std::vector<double>& xgeom,
                                           const std::vector<std::int32_t>& geom_dofmap)
{
  const std::size_t ncells = geom_dofmap.size() / 8;
  std::vector<double> kt(6 * ncells);
  for (std::size_t c = 0; c < ncells; ++c)
  {
    double x[3] = {0, 0, 0};
    for (int k = 0; k < 8; ++k)
      for (int d = 0; d < 3; ++d)
        x[d] += 0.125 * xgeom[3 * (std::size_t)geom_dofmap[8 * c + k] + d];
    const double az = 0.6 + 0.8 * x[1], ax = 0.4 + 0.5 * x[2];
    const double cz = std::cos(az), sz = std::sin(az), cx = std::cos(ax), sx = std::sin(ax);
    // R = Rz Rx, columns = the principal directions
    const double R[3][3] = {{cz, -sz * cx, sz * sx}, {sz, cz * cx, -cz * sx}, {0.0, sx, cx}};
    const double lam[3] = {1.0, 2.0 + x[0], 4.0};
    double M[3][3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j)
        M[i][j] = R[i][0] * lam[0] * R[j][0] + R[i][1] * lam[1] * R[j][1] + R[i][2] * lam[2] * R[j][2];
    double* t = kt.data() + 6 * c;
    t[0] = M[0][0], t[1] = M[0][1], t[2] = M[0][2], t[3] = M[1][1], t[4] = M[1][2], t[5] = M[2][2];
  }
  return kt;
}

// The drivers' reaction coefficient (--reaction S): sigma_c = S (1 + x_c) at the cell centre.  Returns [ncells], the
// layout of pmg_laplacian_set_reaction.
inline std::vector<double> linear_reaction(const std::vector<double>& xgeom,
                                           const std::vector<std::int32_t>& geom_dofmap, double S)
{
  const std::size_t ncells = geom_dofmap.size() / 8;
  std::vector<double> sigma(ncells);
  for (std::size_t c = 0; c < ncells; ++c)
  {
    double x = 0;
    for (int k = 0; k < 8; ++k)
      x += 0.125 * xgeom[3 * (std::size_t)geom_dofmap[8 * c + k]];
    sigma[c] = S * (1.0 + x);
  }
  return sigma;
}

// The drivers' Robin boundary (--robin A): the Dirichlet marker is kept on the face x = 0 only, and the other five
// faces of the box carry alpha = A (1 + y) at their facet points.  `ef` are the exterior facets of the cells held
// (local facet 0 lies on x = 0 and is dropped), `dofmap` the ascending dofmap of degree P and `x` the dof coordinates
// [ndofs][3].  Returns the facet lists and alpha [nfacets][nd * nd], the layout of pmg_laplacian_set_robin.
struct RobinBoundary
{
  std::vector<std::int32_t> cells;
  std::vector<std::int8_t> local_facets;
  std::vector<double> alpha;
};
inline RobinBoundary linear_robin(const ExteriorFacets& ef, const std::vector<std::int32_t>& dofmap,
                                  const std::vector<double>& x, int P, double A)
{
  const std::size_t nd = P + 1, nf = nd * nd, N = nf * nd;
  RobinBoundary out;
  for (std::size_t F = 0; F < ef.cells.size(); ++F)
  {
    if (ef.local_facets[F] == 0)
      continue;
    out.cells.push_back(ef.cells[F]);
    out.local_facets.push_back(ef.local_facets[F]);
    for (std::int32_t t : facet_nodes(P, ef.local_facets[F]))
      out.alpha.push_back(A * (1.0 + x[3 * (std::size_t)dofmap[(std::size_t)ef.cells[F] * N + t] + 1]));
  }
  return out;
}
// ... and its marker: `bc_marker` (the whole boundary) restricted to the dofs on x = 0
inline void keep_marker_on_x0(std::vector<std::int8_t>& bc_marker, const std::vector<double>& x)
{
  for (std::size_t d = 0; d < bc_marker.size(); ++d)
    if (x[3 * d] > 1e-12)
      bc_marker[d] = 0;
}
} // namespace examples
