// Structured hex mesh of a box and its GLL Lagrange function spaces, single rank:
// what the reference's drivers get from dolfinx (create_box, create_functionspace,
// locate_dofs_topological; examples/pmg/main.cpp:425-470, :196-240).  Cells, dofs
// and vertices are numbered lexicographically (x slowest); the dofs of a cell are
// ordered t = a*nd^2 + b*nd + c like the kernel's thread index (src/laplacian.hpp:173).
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <vector>

namespace examples
{
struct BoxMesh
{
  int n;                                  // cells per direction
  std::vector<double> xgeom;              // [npoints][3]
  std::vector<std::int32_t> geom_dofmap;  // [ncells][8], k = i*4 + j*2 + l
  std::int32_t ncells() const { return n * n * n; }
  std::int32_t npoints() const { return (n + 1) * (n + 1) * (n + 1); }

  explicit BoxMesh(int n_) : n(n_)
  {
    const int nv = n + 1;
    xgeom.resize((std::size_t)3 * nv * nv * nv);
    for (int i = 0; i < nv; ++i)
      for (int j = 0; j < nv; ++j)
        for (int k = 0; k < nv; ++k)
        {
          const std::size_t v = ((std::size_t)i * nv + j) * nv + k;
          xgeom[3 * v + 0] = (double)i / n;
          xgeom[3 * v + 1] = (double)j / n;
          xgeom[3 * v + 2] = (double)k / n;
        }
    geom_dofmap.resize((std::size_t)8 * n * n * n);
    for (int cx = 0; cx < n; ++cx)
      for (int cy = 0; cy < n; ++cy)
        for (int cz = 0; cz < n; ++cz)
        {
          const std::size_t c = ((std::size_t)cx * n + cy) * n + cz;
          for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j)
              for (int l = 0; l < 2; ++l)
                geom_dofmap[8 * c + i * 4 + j * 2 + l] = ((cx + i) * nv + (cy + j)) * nv + cz + l;
        }
  }
};

/// The drivers' --curved G: the box bent by a fixed smooth map and described by a coordinate element of degree G
/// (pmg_amd.h "curved cells").  From the vertices and the 8-node dofmap of any box mesh of this directory (BoxMesh,
/// BrickPartition) it makes the degree-G node grid of every cell -- the GLL nodes `gll` of degree G at the trilinear
/// positions between the cell's own corners, k = (i (G+1) + j)(G+1) + l, one node set per cell (a shared node may be
/// stored once per cell) -- and maps every node.  G = 1: the straight-sided mesh through the mapped vertices.
inline void curved_map(double* x)
{
  const double a = x[0], b = x[1], c = x[2];
  x[0] = a + 0.05 * std::sin(2.0 * b + c);
  x[1] = b + 0.05 * std::sin(2.0 * c + a);
  x[2] = c + 0.05 * std::sin(2.0 * a + b);
}
struct CurvedGeometry
{
  int degree;
  std::vector<double> xgeom;             // [ncells * (G+1)^3][3]
  std::vector<std::int32_t> geom_dofmap; // [ncells][(G+1)^3]

  CurvedGeometry(const std::vector<double>& vertices, const std::vector<std::int32_t>& corner_dofmap, int G,
                 const std::vector<double>& gll)
      : degree(G)
  {
    const int m = G + 1, ng = m * m * m;
    const std::size_t ncells = corner_dofmap.size() / 8;
    xgeom.resize(3 * ncells * ng);
    geom_dofmap.resize(ncells * ng);
    for (std::size_t c = 0; c < ncells; ++c)
      for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j)
          for (int l = 0; l < m; ++l)
          {
            const std::size_t node = c * ng + (std::size_t)(i * m + j) * m + l;
            double x[3] = {0, 0, 0};
            for (int k = 0; k < 8; ++k)
            {
              const double wgt = ((k & 4) ? gll[i] : 1.0 - gll[i]) * ((k & 2) ? gll[j] : 1.0 - gll[j])
                                 * ((k & 1) ? gll[l] : 1.0 - gll[l]);
              for (int d = 0; d < 3; ++d)
                x[d] += wgt * vertices[3 * (std::size_t)corner_dofmap[8 * c + k] + d];
            }
            curved_map(x);
            for (int d = 0; d < 3; ++d)
              xgeom[3 * node + d] = x[d];
            geom_dofmap[node] = (std::int32_t)node;
          }
  }
};

/// Degree-P space on the mesh: dofmap, Dirichlet marker on the whole boundary
/// (examples/mat_free/main.cpp:163-165,236-240), dof coordinates.
struct FunctionSpace
{
  int degree;
  std::int32_t ndofs;
  std::vector<std::int32_t> dofmap;   // [ncells][(P+1)^3]
  std::vector<std::int8_t> bc_marker; // [ndofs]
  std::vector<double> x;              // [ndofs][3]

  /// gll: the P+1 GLL points on [0,1] (pmg_gll_table).
  FunctionSpace(const BoxMesh& mesh, int P, const std::vector<double>& gll) : degree(P)
  {
    const int n = mesh.n, nd = P + 1, m = n * P + 1;
    ndofs = m * m * m;
    dofmap.resize((std::size_t)mesh.ncells() * nd * nd * nd);
    for (int cx = 0; cx < n; ++cx)
      for (int cy = 0; cy < n; ++cy)
        for (int cz = 0; cz < n; ++cz)
        {
          const std::size_t c = ((std::size_t)cx * n + cy) * n + cz;
          std::int32_t* d = dofmap.data() + c * nd * nd * nd;
          for (int a = 0; a < nd; ++a)
            for (int b = 0; b < nd; ++b)
              for (int e = 0; e < nd; ++e)
                d[(a * nd + b) * nd + e] = ((cx * P + a) * m + (cy * P + b)) * m + cz * P + e;
        }
    bc_marker.assign(ndofs, 0);
    x.resize((std::size_t)3 * ndofs);
    std::vector<double> line(m);
    for (int c = 0; c < n; ++c)
      for (int a = 0; a < nd; ++a)
        line[c * P + a] = (c + gll[a]) / n;
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j)
        for (int k = 0; k < m; ++k)
        {
          const std::size_t d = ((std::size_t)i * m + j) * m + k;
          x[3 * d + 0] = line[i];
          x[3 * d + 1] = line[j];
          x[3 * d + 2] = line[k];
          if (i == 0 || j == 0 || k == 0 || i == m - 1 || j == m - 1 || k == m - 1)
            bc_marker[d] = 1;
        }
  }
};

/// The nd * nd ascending cell-local node numbers t = a*nd^2 + b*nd + c of the face `local_facet` = 2 * axis + side
/// (side 0: xi_axis = 0, side 1: xi_axis = 1), in the order of the facet points of pmg_laplacian_assemble_neumann:
/// s = i*nd + j over the two remaining axes in increasing axis order, by ascending coordinate.
inline std::vector<std::int32_t> facet_nodes(int P, int local_facet)
{
  const int nd = P + 1, axis = local_facet / 2, fixed = (local_facet % 2) ? P : 0;
  std::vector<std::int32_t> t((std::size_t)nd * nd);
  for (int i = 0; i < nd; ++i)
    for (int j = 0; j < nd; ++j)
      t[(std::size_t)i * nd + j] = axis == 0   ? (fixed * nd + i) * nd + j
                                   : axis == 1 ? (i * nd + fixed) * nd + j
                                               : (i * nd + j) * nd + fixed;
  return t;
}

/// Exterior faces of a list of cells given by their global cell coordinates in an n[0] x n[1] x n[2] grid:
/// (cells, local facets = 2 * axis + side), ordered by cell, then facet.
struct ExteriorFacets
{
  std::vector<std::int32_t> cells;
  std::vector<std::int8_t> local_facets;
};
template <typename Coords>
inline ExteriorFacets exterior_facets(const Coords& cell_coords, const int (&n)[3])
{
  ExteriorFacets out;
  std::int32_t c = 0;
  for (const auto& cc : cell_coords)
  {
    for (int axis = 0; axis < 3; ++axis)
      for (int side = 0; side < 2; ++side)
        if (cc[axis] == (side ? n[axis] - 1 : 0))
        {
          out.cells.push_back(c);
          out.local_facets.push_back((std::int8_t)(2 * axis + side));
        }
    ++c;
  }
  return out;
}
/// ... of the whole single-rank mesh (cells lexicographic, x slowest)
inline ExteriorFacets exterior_facets(const BoxMesh& mesh)
{
  const int n = mesh.n;
  std::vector<std::array<int, 3>> cells;
  cells.reserve((std::size_t)n * n * n);
  for (int cx = 0; cx < n; ++cx)
    for (int cy = 0; cy < n; ++cy)
      for (int cz = 0; cz < n; ++cz)
        cells.push_back({cx, cy, cz});
  const int nn[3] = {n, n, n};
  return exterior_facets(cells, nn);
}

/// Cells per direction so that the degree-P space has about `ndofs` dofs
/// (the drivers' --ndofs, examples/pmg/main.cpp:425-440).
inline int cells_for_ndofs(std::size_t ndofs, int P)
{
  const double m = std::cbrt((double)ndofs);
  const int n = (int)std::lround((m - 1.0) / P);
  return n < 1 ? 1 : n;
}
} // namespace examples
