// The cell-wise bilinear form of the diffusion term (pmg_amd.h "per-cell bilinear form"):
//     e_c(u, v) = sum over the points q of cell c of  (grad_ref v)_q^T G_q (grad_ref u)_q     [ x kappa_c ]
// -- the adjoint gradient with respect to the per-cell coefficient, dJ/dkappa_c = -e_c(u, lambda), a cell's energy
// e_c(u, u), and their sum, the total energy.  One value per cell, one launch, no scatter: nothing is shared between
// cells, so there is no colouring and no atomic, and the sum of a cell is taken in a fixed order.
//
// G_q is formed in place from the mesh (jacobian + point_tensor, as the lifting kernel does), not read from the stored
// tensor: the kernel is then independent of the tensor's slot layout, of batched-geometry mode (no resident tensor), of
// the affine mode, of the chain form and of both recompute switches, and the nodal field, the per-cell tensor and a
// curved coordinate element arrive through the two shared definitions unchanged.
#include "laplacian.hpp"

#include <cstdint>

using namespace pmg;

namespace
{
// One thread per node, LiftShape's workgroups.  u and v of the cell are gathered into LDS through the ascending dofmap
// (bc != nullptr: a marked dof reads as 0 in both); every thread contracts both with D along the three axes at its own
// point, forms G_q and the point's term dv^T G_q du; the workgroup sums the terms of each of its cells.
template <int ND>
__global__ void __launch_bounds__(LiftShape<ND>::THREADS)
    cell_form_kernel(int32_t ncells, const int32_t* __restrict__ dofmap, const int8_t* __restrict__ bc,
                     const double* __restrict__ xgeom, const int32_t* __restrict__ geom_dofmap, int ng,
                     const double* __restrict__ dphi, const double* __restrict__ w, const double* __restrict__ D,
                     const double* __restrict__ kfield, const double* __restrict__ ktensor,
                     const double* __restrict__ kappa, const double* u, const double* v, double* __restrict__ out)
{
  using Sh = LiftShape<ND>;
  constexpr int N = Sh::N, CPW = Sh::CPW, NW = Sh::THREADS / 64;
  __shared__ double us[CPW * N], vs[CPW * N], Ds[ND * ND], red[NW * CPW];
  const int tid = threadIdx.x;
  if (tid < ND * ND)
    Ds[tid] = D[tid];
  // (one cell per workgroup: the cell number is written as uniform over the workgroup, so that what depends on the
  // cell alone -- its geometry nodes, its tensor, kappa -- is read once per wavefront, not once per lane)
  const int ci = CPW == 1 ? 0 : tid / N, t = tid - ci * N;
  const long long cl = (long long)blockIdx.x * CPW + ci;
  const bool active = (CPW == 1 ? tid < N : ci < CPW) && cl < ncells;
  const int32_t cell = active ? (int32_t)cl : 0;
  if (active)
  {
    const int32_t dof = dofmap[(size_t)cell * N + t];
    const bool marked = bc && bc[dof] != 0;
    // a select, not a product: whatever sits in a marked entry (a NaN included) stays out
    us[ci * N + t] = marked ? 0.0 : u[dof];
    vs[ci * N + t] = marked ? 0.0 : v[dof];
  }
  __syncthreads();
  double term = 0.0;
  if (active)
  {
    const int a = t / (ND * ND), bb = (t / ND) % ND, c = t % ND;
    // the geometry first: six values stay live across the contractions, not the Jacobian's gathers across their sums
    double G[6];
    {
      double K[3][3], detJ;
      jacobian(xgeom, geom_dofmap + (size_t)cell * ng, dphi, N, t, ng, K, detJ);
      point_tensor(K, detJ, cell, N, t, w, kfield, dofmap, ktensor, G);
    }
    const double *ue = us + ci * N, *ve = vs + ci * N;
    double du0 = 0, du1 = 0, du2 = 0, dv0 = 0, dv1 = 0, dv2 = 0;
#pragma unroll
    for (int i = 0; i < ND; ++i)
    {
      const double da = Ds[a * ND + i], db = Ds[bb * ND + i], dc = Ds[c * ND + i];
      const int ia = (i * ND + bb) * ND + c, ib = (a * ND + i) * ND + c, ic = (a * ND + bb) * ND + i;
      du0 += da * ue[ia];
      du1 += db * ue[ib];
      du2 += dc * ue[ic];
      dv0 += da * ve[ia];
      dv1 += db * ve[ib];
      dv2 += dc * ve[ic];
    }
    term = dv0 * (G[0] * du0 + G[1] * du1 + G[2] * du2) + dv1 * (G[1] * du0 + G[3] * du1 + G[4] * du2)
           + dv2 * (G[2] * du0 + G[4] * du1 + G[5] * du2);
  }
  // The cell's sum, in an order that depends on the degree alone: wavefront shuffles, then (where a cell spans
  // wavefronts) their partial sums through LDS, added by one lane in wavefront order.  Idle lanes carry 0.
  if constexpr (CPW > 1 && 64 % N == 0)
  {
    // degree 1: a cell is an aligned group of N lanes of the one wavefront
#pragma unroll
    for (int off = N / 2; off > 0; off >>= 1)
      term += __shfl_down(term, off, N);
    if (active && t == 0)
      out[cell] = kappa ? kappa[cell] * term : term;
  }
  else
  {
    // one cell per workgroup (degree >= 3), or cells that straddle the wavefronts (degree 2): each wavefront sums,
    // cell by cell, the lanes that belong to the cell
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int k = 0; k < CPW; ++k)
    {
      const double s = wave_sum(ci == k ? term : 0.0);
      if (lane == 0)
        red[wave * CPW + k] = s;
    }
    __syncthreads();
    const long long mine = (long long)blockIdx.x * CPW + tid;
    if (tid < CPW && mine < ncells)
    {
      double s = 0.0;
#pragma unroll
      for (int wv = 0; wv < NW; ++wv)
        s += red[wv * CPW + tid];
      out[mine] = kappa ? kappa[mine] * s : s;
    }
  }
}

template <int ND>
void launch_cell_form(pmg_laplacian op, const double* u, const double* v, double* out, int flags, hipStream_t s)
{
  using Sh = LiftShape<ND>;
  const unsigned blocks = (unsigned)(((long long)op->ncells + Sh::CPW - 1) / Sh::CPW);
  cell_form_kernel<ND><<<blocks, Sh::THREADS, 0, s>>>(
      op->ncells, op->dofmap, (flags & PMG_CELL_FORM_CONSTRAINED) ? op->bc : nullptr, op->xgeom, op->geom_dofmap, op->ng,
      op->dphi_geom, op->gweights, op->D, op->kfield, op->ktensor, (flags & PMG_CELL_FORM_KAPPA) ? op->kappa : nullptr, u,
      v, out);
}
} // namespace

extern "C" int pmg_laplacian_cell_form(pmg_laplacian op, const double* u, const double* v, double* out_cells, int flags,
                                       pmg_stream stream)
{
  PMG_REQUIRE(op && u && v && out_cells, "pmg_laplacian_cell_form: NULL argument");
  PMG_REQUIRE((flags & ~(PMG_CELL_FORM_KAPPA | PMG_CELL_FORM_CONSTRAINED)) == 0,
              "pmg_laplacian_cell_form: unknown flag bits 0x%x", flags & ~(PMG_CELL_FORM_KAPPA | PMG_CELL_FORM_CONSTRAINED));
  const size_t total = (size_t)op->layout->total(), nc = (size_t)op->ncells;
  PMG_REQUIRE(!overlaps(out_cells, nc, u, total) && !overlaps(out_cells, nc, v, total),
              "pmg_laplacian_cell_form: out_cells must not overlap u or v");
  if (op->ncells == 0)
    return PMG_OK;
  hipStream_t s = S(stream);
  PMG_TRY(with_degree(op->P, [&](auto P) {
    launch_cell_form<decltype(P)::value + 1>(op, u, v, out_cells, flags, s);
    return PMG_OK;
  }));
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}
