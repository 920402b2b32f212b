// The kernels that build the geometry tensor, shared by the FP64 tensor (laplacian.hip) and the float tensor
// (laplacian_f32.hip), and launch_geometry, which picks one:
//
//   dense_geometry_kernel   a thread per point walks the dense table [3][nq][ng] (jacobian()): the trilinear element
//                           (NG = 8, 48 table values per point), and caller tables of a coordinate element of degree
//                           g >= 2 (pmg_laplacian_create_curved), where no tensor product can be assumed (NG = 0).
//   curved_geometry_kernel  the library's own tensor-product element of degree g >= 2: one workgroup owns the points of
//                           one patch slot (several slots at P <= 2, as LiftShape groups cells, so that a wavefront is
//                           full), stages the cell's 3 (g+1)^3 coordinates in LDS once and sum-factorises dx/dxi:
//                           contract along z with L and L', then along y, then every thread finishes its own point with
//                           3 * 3 * (g+1) FMAs.  A thread per point with the dense table would read 2 * 3 * (g+1)^3
//                           values per point (162 at g = 2, 750 at g = 4).
//
// Both form adj(J) and |det J| (adjugate) and G from them (point_tensor), write zeros into empty slots, and hand the six
// values to `out(slot, q, g)`: the caller's layout of the tensor (gpos for the FP64 tensor, the float layout rounds).
#pragma once

#include "laplacian.hpp"

namespace pmg
{
// slots per workgroup and threads of the cooperative kernel (LiftShape's rule: 8 cells at degree 1, 3 at degree 2)
inline int curved_slots_per_group(int N) { return N >= 64 ? 1 : (64 + N - 1) / N; }
inline int curved_threads(int N) { return ((curved_slots_per_group(N) * N + 63) / 64) * 64; }
// LDS doubles of one slot: coordinates X[3][m^3], after z A[2][3][m^2][nd], after y B[3][3][m][nd^2]
__host__ __device__ constexpr int curved_slot_doubles(int nd, int m) { return 3 * m * m * m + 6 * m * m * nd + 9 * m * nd * nd; }
inline size_t curved_lds_bytes(int nd, int m)
{
  return sizeof(double) * ((size_t)2 * nd * m + (size_t)curved_slots_per_group(nd * nd * nd) * curved_slot_doubles(nd, m));
}

// Patch slots [slot0, slot0 + nslots), `cpw` of them per workgroup; M = g + 1.  L, Lp [nd][M]: the coordinate element's
// 1-D basis and derivative at the GLL points.  Node k = (i M + j) M + l, point q = (a nd + b) nd + c: i and a run along
// the cell's x axis, l and c along z.
template <int M, typename Out>
__global__ void __launch_bounds__(768)
    curved_geometry_kernel(long long slot0, long long nslots, int nd, int cpw, const int32_t* __restrict__ pcell,
                           const double* __restrict__ xgeom, const int32_t* __restrict__ geom_dofmap,
                           const double* __restrict__ L, const double* __restrict__ Lp, const double* __restrict__ w,
                           const double* __restrict__ kfield, const int32_t* __restrict__ dofmap,
                           const double* __restrict__ ktensor, Out out)
{
  constexpr int M2 = M * M, M3 = M2 * M;
  extern __shared__ double lds[];
  const int nsq = nd * nd, N = nsq * nd;
  const int per = curved_slot_doubles(nd, M);
  double* sL = lds;           // [nd][M]
  double* sLp = sL + nd * M;  // [nd][M]
  double* cells = sLp + nd * M;
  const int tid = threadIdx.x, nt = blockDim.x;
  const long long first = (long long)blockIdx.x * cpw; // relative to slot0

  for (int i = tid; i < nd * M; i += nt)
  {
    sL[i] = L[i];
    sLp[i] = Lp[i];
  }
  // the cells' coordinates: X[comp][k]; an empty slot and one past the end stage zeros (their points are not computed)
  for (int i = tid; i < cpw * M3; i += nt)
  {
    const int ci = i / M3, k = i - ci * M3;
    const long long rel = first + ci;
    const int c = rel < nslots ? pcell[slot0 + rel] : -1;
    double x0 = 0, x1 = 0, x2 = 0;
    if (c >= 0)
    {
      const double* xk = xgeom + 3 * (size_t)geom_dofmap[(size_t)c * M3 + k];
      x0 = xk[0], x1 = xk[1], x2 = xk[2];
    }
    double* X = cells + ci * per;
    X[k] = x0;
    X[M3 + k] = x1;
    X[2 * M3 + k] = x2;
  }
  __syncthreads();
  // along z: A[v][comp][ij][c] = sum_l (v ? L' : L)[c][l] X[comp][ij M + l]
  for (int i = tid; i < cpw * 3 * M2 * nd; i += nt)
  {
    const int ci = i / (3 * M2 * nd), r = i - ci * (3 * M2 * nd);
    const int row = r / nd, c = r - row * nd; // row = comp * M2 + ij
    const double* X = cells + ci * per + row * M;
    double a0 = 0, a1 = 0;
#pragma unroll
    for (int l = 0; l < M; ++l)
    {
      a0 += sL[c * M + l] * X[l];
      a1 += sLp[c * M + l] * X[l];
    }
    double* A = cells + ci * per + 3 * M3;
    A[row * nd + c] = a0;
    A[(3 * M2 + row) * nd + c] = a1;
  }
  __syncthreads();
  // along y: B[v][comp][i][b nd + c]; v = 0: L_y L_z (for d/dx), 1: L'_y L_z (d/dy), 2: L_y L'_z (d/dz)
  for (int i = tid; i < cpw * 3 * M * nsq; i += nt)
  {
    const int ci = i / (3 * M * nsq), r = i - ci * (3 * M * nsq);
    const int row = r / nsq, bc = r - row * nsq; // row = comp * M + i
    const int b = bc / nd, c = bc - b * nd;
    const double* A0 = cells + ci * per + 3 * M3 + (size_t)row * M * nd + c; // [j][c] of (comp, i)
    const double* A1 = A0 + 3 * M2 * nd;
    double b0 = 0, b1 = 0, b2 = 0;
#pragma unroll
    for (int j = 0; j < M; ++j)
    {
      const double l = sL[b * M + j], lp = sLp[b * M + j];
      b0 += l * A0[j * nd];
      b1 += lp * A0[j * nd];
      b2 += l * A1[j * nd];
    }
    double* B = cells + ci * per + 3 * M3 + 6 * M2 * nd;
    B[row * nsq + bc] = b0;
    B[(3 * M + row) * nsq + bc] = b1;
    B[(6 * M + row) * nsq + bc] = b2;
  }
  __syncthreads();
  // along x, one point per thread
  if (tid >= cpw * N)
    return;
  const int ci = tid / N, q = tid - ci * N;
  const long long rel = first + ci;
  if (rel >= nslots)
    return;
  const long long slot = slot0 + rel;
  const int c = pcell[slot];
  double g[6] = {0, 0, 0, 0, 0, 0};
  if (c >= 0)
  {
    const int a = q / nsq, bc = q - a * nsq;
    const double* B = cells + ci * per + 3 * M3 + 6 * M2 * nd + bc;
    double J[3][3];
#pragma unroll
    for (int comp = 0; comp < 3; ++comp)
    {
      double j0 = 0, j1 = 0, j2 = 0;
#pragma unroll
      for (int i = 0; i < M; ++i)
      {
        const int row = comp * M + i;
        j0 += sLp[a * M + i] * B[row * nsq];
        j1 += sL[a * M + i] * B[(3 * M + row) * nsq];
        j2 += sL[a * M + i] * B[(6 * M + row) * nsq];
      }
      J[comp][0] = j0, J[comp][1] = j1, J[comp][2] = j2;
    }
    double K[3][3], detJ;
    adjugate(J, K, detJ);
    point_tensor(K, detJ, c, N, q, w, kfield, dofmap, ktensor, g);
  }
  out(slot, q, g);
}

// A thread per point with the dense table [3][nq][NG]; NG = 8: the trilinear element, 0: `ng` nodes (caller tables).
// Threads of a wavefront walk q, so the dofmap read is contiguous; the kfield gather follows the dofmap like the
// apply's x.
template <int NG, typename Out>
__global__ void dense_geometry_kernel(long long slot0, long long nslots, int nq, int ng,
                                      const int32_t* __restrict__ pcell, const double* __restrict__ xgeom,
                                      const int32_t* __restrict__ geom_dofmap, const double* __restrict__ dphi,
                                      const double* __restrict__ w, const double* __restrict__ kfield,
                                      const int32_t* __restrict__ dofmap, const double* __restrict__ ktensor, Out out)
{
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= nslots * nq)
    return;
  long long slot = gid / nq;
  const int q = (int)(gid - slot * nq);
  slot += slot0;
  const int c = pcell[slot];
  double g[6] = {0, 0, 0, 0, 0, 0};
  if (c >= 0)
  {
    double K[3][3], detJ;
    jacobian<NG>(xgeom, geom_dofmap + (size_t)c * (NG ? NG : ng), dphi, nq, q, ng, K, detJ);
    point_tensor(K, detJ, c, nq, q, w, kfield, dofmap, ktensor, g);
  }
  out(slot, q, g);
}

// The tensor of the slots [slot0, slot0 + nslots) through `out`, the one place that picks the kernel: per point over
// the 8 nodes of the trilinear element; at degree >= 2 the cooperative kernel with the library's own tabulation, the
// per-point kernel over the dense table with the caller's
template <typename Out>
void launch_geometry(pmg_laplacian op, long long slot0, long long nslots, Out out, hipStream_t s)
{
  if (nslots <= 0)
    return;
  if (!op->geom_L) // (the 1-D tables exist at degree >= 2 with the library's tabulation only)
  {
    const long long n = nslots * op->N;
    auto launch = [&](auto ng) {
      dense_geometry_kernel<decltype(ng)::value, Out><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(
          slot0, nslots, op->N, op->ng, op->pcell, op->xgeom, op->geom_dofmap, op->dphi_geom, op->gweights, op->kfield,
          op->dofmap, op->ktensor, out);
    };
    op->ng == 8 ? launch(std::integral_constant<int, 8>{}) : launch(std::integral_constant<int, 0>{});
    return;
  }
  const int cpw = curved_slots_per_group(op->N), threads = curved_threads(op->N), m = op->geom_degree + 1;
  const unsigned blocks = (unsigned)((nslots + cpw - 1) / cpw);
  const size_t lds = curved_lds_bytes(op->nd, m);
  auto launch = [&](auto mm) {
    curved_geometry_kernel<decltype(mm)::value, Out><<<blocks, threads, lds, s>>>(
        slot0, nslots, op->nd, cpw, op->pcell, op->xgeom, op->geom_dofmap, op->geom_L, op->geom_Lp, op->gweights,
        op->kfield, op->dofmap, op->ktensor, out);
  };
  switch (m)
  {
  case 3: launch(std::integral_constant<int, 3>{}); break;
  case 4: launch(std::integral_constant<int, 4>{}); break;
  default: launch(std::integral_constant<int, 5>{}); break;
  }
}
} // namespace pmg

