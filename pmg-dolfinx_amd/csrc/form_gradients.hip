// The derivatives of v_m^T A u_m with respect to the operator's coefficients (pmg_amd.h "coefficient gradients of the
// form"): the per-cell scalar kappa_c, the nodal field kq, the per-cell tensor K_c and the per-cell reaction sigma_c.
// Every coefficient enters A linearly, and every derivative is made of what the cell form computes at a point -- adj(J),
// |det J| and the two reference gradients -- so one kernel forms the point geometry once (jacobian(), the shared
// definition) and emits every gradient that was asked for:
//     pu = adj(J)^T gradref u, pv likewise, t_q = pv . T_c pu, s_q = w_q / |det J|
//     d_kappa[c]     = sum_q s_q kq_q t_q
//     d_field[n]    += kappa_c s_q t_q                 for the points (c, q) of the listed cells on dof n (atomics)
//     d_tensor[c][k] = kappa_c sum_q s_q kq_q m_k,     m = pv pu^T symmetrised onto (xx, xy, xz, yy, yz, zz)
//     d_sigma[c]     = sum_q w_q |det J| u_q v_q
// An output that is not asked for (NULL) is a uniform branch not taken.  The per-cell sums are the cell form's: a fixed
// tree per wavefront, then the wavefronts' partial sums in wavefront order; each output has its own sum, so an output
// has the same bytes whichever others are computed beside it.
#include "laplacian.hpp"

#include <cstdint>

using namespace pmg;

namespace
{
constexpr int NV = 8; // per-cell sums: d_kappa, the six of d_tensor, d_sigma

// One thread per node, LiftShape's workgroups, as cell_form_kernel: u and v of the cell through the ascending dofmap
// into LDS (bc != nullptr: a marked dof reads as 0 in both), the geometry first, the contractions after.
template <int ND>
__global__ void __launch_bounds__(LiftShape<ND>::THREADS)
    form_gradients_kernel(int32_t ncells, const int32_t* __restrict__ dofmap, const int8_t* __restrict__ bc,
                          const int8_t* __restrict__ listed, const double* __restrict__ xgeom,
                          const int32_t* __restrict__ geom_dofmap, int ng, const double* __restrict__ dphi,
                          const double* __restrict__ w, const double* __restrict__ D,
                          const double* __restrict__ kfield, const double* __restrict__ ktensor,
                          const double* __restrict__ kappa, const double* u, const double* v,
                          double* __restrict__ d_kappa, double* __restrict__ d_field, double* __restrict__ d_tensor,
                          double* __restrict__ d_sigma)
{
  using Sh = LiftShape<ND>;
  constexpr int N = Sh::N, CPW = Sh::CPW, NW = Sh::THREADS / 64;
  // (degree 1: a cell is an aligned group of N lanes of the one wavefront and is summed by shuffles of that width)
  constexpr bool CELL_IN_LANES = CPW > 1 && 64 % N == 0;
  static_assert(!CELL_IN_LANES || NW == 1, "cells summed inside the wavefront: one wavefront");
  static_assert(NV * CPW <= Sh::THREADS, "one thread per cell and sum writes the results");
  __shared__ double us[CPW * N], vs[CPW * N], Ds[ND * ND], red[NV][NW * CPW];
  const int tid = threadIdx.x;
  if (tid < ND * ND)
    Ds[tid] = D[tid];
  // (one cell per workgroup: the cell number is uniform over the workgroup, so that what depends on the cell alone --
  // its geometry nodes, its tensor, kappa, the listed byte -- is read once per wavefront, not once per lane)
  const int ci = CPW == 1 ? 0 : tid / N, t = tid - ci * N;
  const long long cl = (long long)blockIdx.x * CPW + ci;
  const bool active = (CPW == 1 ? tid < N : ci < CPW) && cl < ncells;
  const int32_t cell = CPW == 1 ? (int32_t)blockIdx.x : (active ? (int32_t)cl : 0);
  int32_t dof = 0;
  if (active)
  {
    dof = dofmap[(size_t)cell * N + t];
    const bool marked = bc && bc[dof] != 0;
    // a select, not a product: whatever sits in a marked entry (a NaN included) stays out
    us[ci * N + t] = marked ? 0.0 : u[dof];
    vs[ci * N + t] = marked ? 0.0 : v[dof];
  }
  __syncthreads();
  double tk = 0.0, tt[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ts = 0.0;
  if (active)
  {
    const int a = t / (ND * ND), bb = (t / ND) % ND, c = t % ND;
    double K[3][3], detJ;
    jacobian(xgeom, geom_dofmap + (size_t)cell * ng, dphi, N, t, ng, K, detJ);
    // the geometry first, with the point's two scale factors, the contractions after: twelve values stay live across
    // them.  (A branch between the contractions and their first use -- the field's -- is where the compiler sinks
    // every product of the unrolled loop to, holding all its LDS reads until then: 180 VGPRs at degree 7, scratch at
    // degree 8.)
    const double wq = w[t], s = wq / detJ;
    const double skq = kfield ? s * kfield[dof] : s;
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
    // K = adj(J): row = reference direction, column = physical direction
    const double pu0 = K[0][0] * du0 + K[1][0] * du1 + K[2][0] * du2;
    const double pu1 = K[0][1] * du0 + K[1][1] * du1 + K[2][1] * du2;
    const double pu2 = K[0][2] * du0 + K[1][2] * du1 + K[2][2] * du2;
    const double pv0 = K[0][0] * dv0 + K[1][0] * dv1 + K[2][0] * dv2;
    const double pv1 = K[0][1] * dv0 + K[1][1] * dv1 + K[2][1] * dv2;
    const double pv2 = K[0][2] * dv0 + K[1][2] * dv1 + K[2][2] * dv2;
    if (d_kappa || d_field)
    {
      double r0 = pu0, r1 = pu1, r2 = pu2;
      if (ktensor)
      {
        const double* kt = ktensor + (size_t)cell * 6;
        r0 = kt[0] * pu0 + kt[1] * pu1 + kt[2] * pu2;
        r1 = kt[1] * pu0 + kt[3] * pu1 + kt[4] * pu2;
        r2 = kt[2] * pu0 + kt[4] * pu1 + kt[5] * pu2;
      }
      const double tq = pv0 * r0 + pv1 * r1 + pv2 * r2;
      tk = skq * tq;
      // the field's own value is divided out: s, not s kq.  One add per point; the lanes of a wavefront run through the
      // cell's dofs in ascending order, whole rows of nd consecutive dofs.
      if (d_field && listed[cell])
        atomicAdd(&d_field[dof], kappa[cell] * (s * tq));
    }
    if (d_tensor)
    {
      // (a packed off-diagonal value fills two entries of the matrix)
      tt[0] = skq * (pv0 * pu0);
      tt[1] = skq * (pv0 * pu1 + pv1 * pu0);
      tt[2] = skq * (pv0 * pu2 + pv2 * pu0);
      tt[3] = skq * (pv1 * pu1);
      tt[4] = skq * (pv1 * pu2 + pv2 * pu1);
      tt[5] = skq * (pv2 * pu2);
    }
    if (d_sigma)
      ts = wq * detJ * (ue[t] * ve[t]);
  }
  // The cells' sums, in an order that depends on the degree alone: each requested value into its row of `red`, one
  // entry per wavefront and cell.  Idle lanes carry 0.
  const int wave = tid >> 6, lane = tid & 63;
  auto stage = [&](double term, int j) {
    if constexpr (CELL_IN_LANES)
    {
#pragma unroll
      for (int off = N / 2; off > 0; off >>= 1)
        term += __shfl_down(term, off, N);
      if (ci < CPW && t == 0)
        red[j][ci] = term;
    }
    else
    {
#pragma unroll
      for (int k = 0; k < CPW; ++k)
      {
        const double s = wave_sum(ci == k ? term : 0.0);
        if (lane == 0)
          red[j][wave * CPW + k] = s;
      }
    }
  };
  if (d_kappa)
    stage(tk, 0);
  if (d_tensor)
  {
#pragma unroll
    for (int k = 0; k < 6; ++k)
      stage(tt[k], 1 + k);
  }
  if (d_sigma)
    stage(ts, 7);
  __syncthreads();
  // thread (j, k) adds the wavefronts' partial sums of value j of the workgroup's cell k, in wavefront order
  const int j = tid / CPW, k = tid - j * CPW;
  const long long mine = (long long)blockIdx.x * CPW + k;
  if (j < NV && mine < ncells)
  {
    double* out = j == 0 ? d_kappa : (j == 7 ? d_sigma : d_tensor);
    if (out)
    {
      double s = red[j][k];
#pragma unroll
      for (int wv = 1; wv < NW; ++wv)
        s += red[j][wv * CPW + k];
      if (j == 0 || j == 7)
        out[mine] = s;
      else
        out[mine * 6 + (j - 1)] = kappa[mine] * s;
    }
  }
}

template <int ND>
void launch_form_gradients(pmg_laplacian op, const double* u, const double* v, double* d_kappa, double* d_field,
                           double* d_tensor, double* d_sigma, int flags, hipStream_t s)
{
  using Sh = LiftShape<ND>;
  const unsigned blocks = (unsigned)(((long long)op->ncells + Sh::CPW - 1) / Sh::CPW);
  form_gradients_kernel<ND><<<blocks, Sh::THREADS, 0, s>>>(
      op->ncells, op->dofmap, (flags & PMG_CELL_FORM_CONSTRAINED) ? op->bc : nullptr, op->cell_listed, op->xgeom,
      op->geom_dofmap, op->ng, op->dphi_geom, op->gweights, op->D, op->kfield, op->ktensor, op->kappa, u, v, d_kappa,
      d_field, d_tensor, d_sigma);
}
} // namespace

extern "C" int pmg_laplacian_form_gradients(pmg_laplacian op, const double* u, const double* v, double* d_kappa,
                                            double* d_field, double* d_tensor, double* d_sigma, int flags,
                                            pmg_stream stream)
{
  PMG_REQUIRE(op && u && v, "pmg_laplacian_form_gradients: NULL argument (op, u or v)");
  PMG_REQUIRE(d_kappa || d_field || d_tensor || d_sigma, "pmg_laplacian_form_gradients: all four outputs are NULL");
  PMG_REQUIRE((flags & ~PMG_CELL_FORM_CONSTRAINED) == 0,
              "pmg_laplacian_form_gradients: illegal flag bits 0x%x (PMG_CELL_FORM_CONSTRAINED is the only flag)",
              flags & ~PMG_CELL_FORM_CONSTRAINED);
  const size_t total = (size_t)op->layout->total(), nc = (size_t)op->ncells;
  const double* arr[6] = {u, v, d_kappa, d_field, d_tensor, d_sigma};
  const size_t len[6] = {total, total, nc, total, 6 * nc, nc};
  for (int i = 2; i < 6; ++i)
    for (int k = 0; k < i; ++k)
      PMG_REQUIRE(!overlaps(arr[i], len[i], arr[k], len[k]),
                  "pmg_laplacian_form_gradients: an output must not overlap u, v or another output");
  hipStream_t s = S(stream);
  if (d_field && total > 0)
    PMG_HIP(hipMemsetAsync(d_field, 0, sizeof(double) * total, s));
  if (op->ncells == 0)
    return PMG_OK;
  PMG_TRY(with_degree(op->P, [&](auto P) {
    launch_form_gradients<decltype(P)::value + 1>(op, u, v, d_kappa, d_field, d_tensor, d_sigma, flags, s);
    return PMG_OK;
  }));
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}
