// Boundary data of the matrix-free operator (pmg_amd.h "boundary data"): Dirichlet lifting, set_bc and the Neumann
// load, i.e. dolfinx's fem::apply_lifting / fem::set_bc and an inner(h, v) * ds term, computed on the device from the
// operator the caller already has.  All three are set-up calls at O(surface) cost: none of them touches the stored
// tensor, the patch plan or any launch of the apply.
//
// The lifting needs the UNCONSTRAINED operator on the cells that hold a marked dof (on a box: the boundary shell).
// Those cells recompute their geometry in the kernel, exactly as the tensor kernels do, instead of reading the stored
// tensor: the kernel is then independent of the tensor's layout, of batched-geometry mode (no resident tensor), of the
// affine mode and of the chain form, and the shell is a small share of the mesh (9 % of the cells at 64^3).
#include "laplacian.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>

using namespace pmg;

namespace
{
// b[dof] -= alpha * (A_cell u_cell)[t] for the unmarked owned rows of the listed cells, with
// u_cell[t] = marked(dof) ? g[dof] - x0[dof] : 0 -- the element kernel of src/laplacian.hpp:143-278 without its row and
// column treatment, G_q computed in place (src/laplacian.hpp:72-111, as point_tensor: w_q / detJ, times the nodal
// coefficient when one is set, and with the per-cell diffusion tensor between the two adjugates when one is set).
// Unmarked entries of g and x0 are never read.
template <int ND>
__global__ void __launch_bounds__(LiftShape<ND>::THREADS)
    lifting_kernel(int nlift, const int32_t* __restrict__ lift_cells, const int32_t* __restrict__ dofmap,
                   const int8_t* __restrict__ bc, int32_t size_local, const double* __restrict__ xgeom,
                   const int32_t* __restrict__ geom_dofmap, int ng, const double* __restrict__ dphi,
                   const double* __restrict__ w, const double* __restrict__ D, const double* __restrict__ kfield,
                   const double* __restrict__ ktensor, const double* __restrict__ kappa, const double* __restrict__ g,
                   const double* __restrict__ x0, double alpha, double* __restrict__ b)
{
  using Sh = LiftShape<ND>;
  constexpr int N = Sh::N, CPW = Sh::CPW;
  __shared__ double u[CPW * N], f0[CPW * N], f1[CPW * N], f2[CPW * N], Ds[ND * ND];
  const int tid = threadIdx.x;
  if (tid < ND * ND)
    Ds[tid] = D[tid];
  const int ci = tid / N, t = tid - ci * N;
  const long long li = (long long)blockIdx.x * CPW + ci;
  const bool active = ci < CPW && li < nlift;
  const int a = t / (ND * ND), bb = (t / ND) % ND, c = t % ND;
  int32_t cell = 0, dof = 0;
  bool marked = false;
  if (active)
  {
    cell = lift_cells[li];
    dof = dofmap[(size_t)cell * N + t];
    marked = bc[dof] != 0;
    double v = 0.0;
    if (marked) // a select, not a product: whatever sits in the unmarked entries stays out
    {
      v = g[dof];
      if (x0)
        v -= x0[dof];
    }
    u[ci * N + t] = v;
  }
  __syncthreads();
  if (active)
  {
    const double* ue = u + ci * N;
    double d0 = 0, d1 = 0, d2 = 0;
#pragma unroll
    for (int i = 0; i < ND; ++i)
    {
      d0 += Ds[a * ND + i] * ue[(i * ND + bb) * ND + c];
      d1 += Ds[bb * ND + i] * ue[(a * ND + i) * ND + c];
      d2 += Ds[c * ND + i] * ue[(a * ND + bb) * ND + i];
    }
    double K[3][3], detJ;
    jacobian(xgeom, geom_dofmap + (size_t)cell * ng, dphi, N, t, ng, K, detJ);
    double s = w[t] / detJ;
    if (kfield)
      s *= kfield[dof];
    const double kc = kappa[cell];
    if (ktensor)
    {
      // G d = s K (T (K^T d)) without forming G: three 3-vectors instead of the six entries and the nine of K T
      const double* kt = ktensor + (size_t)cell * 6;
      const double p0 = K[0][0] * d0 + K[1][0] * d1 + K[2][0] * d2;
      const double p1 = K[0][1] * d0 + K[1][1] * d1 + K[2][1] * d2;
      const double p2 = K[0][2] * d0 + K[1][2] * d1 + K[2][2] * d2;
      const double r0 = kt[0] * p0 + kt[1] * p1 + kt[2] * p2;
      const double r1 = kt[1] * p0 + kt[3] * p1 + kt[4] * p2;
      const double r2 = kt[2] * p0 + kt[4] * p1 + kt[5] * p2;
      const double ks = kc * s;
      f0[ci * N + t] = ks * (K[0][0] * r0 + K[0][1] * r1 + K[0][2] * r2);
      f1[ci * N + t] = ks * (K[1][0] * r0 + K[1][1] * r1 + K[1][2] * r2);
      f2[ci * N + t] = ks * (K[2][0] * r0 + K[2][1] * r1 + K[2][2] * r2);
    }
    else
    {
      double G[6];
      metric(K, s, G);
      f0[ci * N + t] = kc * (G[0] * d0 + G[1] * d1 + G[2] * d2);
      f1[ci * N + t] = kc * (G[1] * d0 + G[3] * d1 + G[4] * d2);
      f2[ci * N + t] = kc * (G[2] * d0 + G[4] * d1 + G[5] * d2);
    }
  }
  __syncthreads();
  if (active && !marked && dof < size_local)
  {
    const double *e0 = f0 + ci * N, *e1 = f1 + ci * N, *e2 = f2 + ci * N;
    double y = 0;
#pragma unroll
    for (int i = 0; i < ND; ++i)
      y += Ds[i * ND + a] * e0[(i * ND + bb) * ND + c] + Ds[i * ND + bb] * e1[(a * ND + i) * ND + c]
           + Ds[i * ND + c] * e2[(a * ND + bb) * ND + i];
    atomicAdd(&b[dof], -alpha * y);
  }
}

// b[i] = alpha * (g[i] - x0[i]) on the marked owned entries
__global__ void set_bc_kernel(int n, const int8_t* __restrict__ bc, const double* __restrict__ g,
                              const double* __restrict__ x0, double alpha, double* __restrict__ b)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && bc[i])
    b[i] = alpha * (x0 ? g[i] - x0[i] : g[i]);
}

// The facet point gid = F * nd^2 + s of the listed facets, s = i * nd + j over the two remaining axes in increasing
// axis order: its dof and its surface weight w1[i] w1[j] |row `axis` of adj(J)|.  false (and no geometry computed) for
// a marked dof and for one at or past `ndofs`.
__device__ __forceinline__ bool facet_point(long long gid, int nd, const int32_t* __restrict__ fcells,
                                            const int8_t* __restrict__ flocal, const int32_t* __restrict__ dofmap,
                                            const int8_t* __restrict__ bc, int32_t ndofs,
                                            const double* __restrict__ xgeom, const int32_t* __restrict__ geom_dofmap, int ng,
                                            const double* __restrict__ dphi, const double* __restrict__ w1,
                                            int32_t& dof, double& wdS)
{
  const int nf = nd * nd, N = nf * nd;
  const long long F = gid / nf;
  const int sp = (int)(gid - F * nf), i = sp / nd, j = sp - i * nd;
  const int cell = fcells[F], lf = flocal[F], axis = lf >> 1, fixed = (lf & 1) ? nd - 1 : 0;
  const int t = axis == 0 ? (fixed * nd + i) * nd + j : axis == 1 ? (i * nd + fixed) * nd + j : (i * nd + j) * nd + fixed;
  dof = dofmap[(size_t)cell * N + t];
  if (bc[dof] || dof >= ndofs)
    return false;
  double K[3][3], detJ;
  jacobian(xgeom, geom_dofmap + (size_t)cell * ng, dphi, N, t, ng, K, detJ);
  const double* r = K[axis];
  const double dS = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  wdS = w1[i] * w1[j] * dS;
  return true;
}

// One thread per facet point: b[dof] += w1[i] w1[j] |dS| h[facet][s] on unmarked owned rows.
__global__ void neumann_kernel(long long npoints, int nd, const int32_t* __restrict__ fcells,
                               const int8_t* __restrict__ flocal, const double* __restrict__ h,
                               const int32_t* __restrict__ dofmap, const int8_t* __restrict__ bc, int32_t size_local,
                               const double* __restrict__ xgeom, const int32_t* __restrict__ geom_dofmap, int ng,
                               const double* __restrict__ dphi, const double* __restrict__ w1,
                               double* __restrict__ b)
{
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= npoints)
    return;
  int32_t dof;
  double wdS;
  if (facet_point(gid, nd, fcells, flocal, dofmap, bc, size_local, xgeom, geom_dofmap, ng, dphi, w1, dof, wdS))
    atomicAdd(&b[dof], wdS * h[gid]);
}

// The face mass of a Robin term, one thread per facet point: d[dof] += w1[i] w1[j] |dS| alpha[facet][s] on the
// unmarked dofs, ghosts included (`total` = size_local + num_ghosts: a ghost entry holds this rank's facets only).
__global__ void robin_kernel(long long npoints, int nd, const int32_t* __restrict__ fcells,
                             const int8_t* __restrict__ flocal, const double* __restrict__ alpha,
                             const int32_t* __restrict__ dofmap, const int8_t* __restrict__ bc, int32_t total,
                             const double* __restrict__ xgeom, const int32_t* __restrict__ geom_dofmap, int ng,
                             const double* __restrict__ dphi, const double* __restrict__ w1, double* __restrict__ d)
{
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= npoints)
    return;
  int32_t dof;
  double wdS;
  if (facet_point(gid, nd, fcells, flocal, dofmap, bc, total, xgeom, geom_dofmap, ng, dphi, w1, dof, wdS))
    atomicAdd(&d[dof], wdS * alpha[gid]);
}

// Are the (host) facet lists those of cells the operator holds, and of local facets 0..5?
int check_facets(pmg_laplacian op, const char* who, int32_t nfacets, const int32_t* facet_cells,
                 const int8_t* facet_local)
{
  for (int32_t i = 0; i < nfacets; ++i)
  {
    const int32_t c = facet_cells[i];
    PMG_REQUIRE(c >= 0 && c < op->ncells, "%s: facet %d: cell %d outside [0, %d)", who, i, c, op->ncells);
    PMG_REQUIRE(op->listed[c], "%s: facet %d: cell %d is not among the operator's cells", who, i, c);
    PMG_REQUIRE(facet_local[i] >= 0 && facet_local[i] <= 5, "%s: facet %d: local facet %d outside 0..5", who, i,
                (int)facet_local[i]);
  }
  return PMG_OK;
}

// The listed cells (lcells and bcells) that hold a marked dof, from the ascending dofmap and the marker, read back
// once as the constructor does for the patches.
int build_lift_list(pmg_laplacian op, hipStream_t s)
{
  const int N = op->N, total = op->layout->total();
  std::vector<int32_t> dm((size_t)op->ncells * N);
  std::vector<int8_t> bc(total);
  if (!dm.empty())
    PMG_HIP(hipMemcpyAsync(dm.data(), op->dofmap, sizeof(int32_t) * dm.size(), hipMemcpyDeviceToHost, s));
  if (total > 0)
    PMG_HIP(hipMemcpyAsync(bc.data(), op->bc, sizeof(int8_t) * total, hipMemcpyDeviceToHost, s));
  PMG_HIP(hipStreamSynchronize(s));
  std::vector<int32_t> cells;
  for (int32_t c : op->pcell_h)
  {
    if (c < 0)
      continue;
    const int32_t* d = dm.data() + (size_t)c * N;
    bool any = false;
    for (int t = 0; t < N && !any; ++t)
      any = bc[d[t]] != 0;
    if (any)
      cells.push_back(c);
  }
  std::sort(cells.begin(), cells.end());
  PMG_HIP(hipMalloc(&op->lift_cells, sizeof(int32_t) * (cells.empty() ? 1 : cells.size())));
  if (!cells.empty())
    PMG_HIP(hipMemcpy(op->lift_cells, cells.data(), sizeof(int32_t) * cells.size(), hipMemcpyHostToDevice));
  op->n_lift = (int32_t)cells.size();
  return PMG_OK;
}

template <int ND>
void launch_lifting(pmg_laplacian op, const double* g, const double* x0, double alpha, double* b, hipStream_t s)
{
  using Sh = LiftShape<ND>;
  const unsigned blocks = (unsigned)((op->n_lift + Sh::CPW - 1) / Sh::CPW);
  lifting_kernel<ND><<<blocks, Sh::THREADS, 0, s>>>(op->n_lift, op->lift_cells, op->dofmap, op->bc,
                                                   op->layout->size_local, op->xgeom, op->geom_dofmap, op->ng, op->dphi_geom,
                                                   op->gweights, op->D, op->kfield, op->ktensor, op->kappa, g, x0, alpha,
                                                   b);
}
} // namespace

extern "C" int pmg_laplacian_apply_lifting(pmg_laplacian op, double* g, const double* x0, double alpha, double* b,
                                           pmg_stream stream)
{
  PMG_REQUIRE(op && g && b, "pmg_laplacian_apply_lifting: NULL argument");
  const size_t total = (size_t)op->layout->total();
  PMG_REQUIRE(!overlaps(b, total, g, total) && !overlaps(b, total, x0, total),
              "pmg_laplacian_apply_lifting: b must not alias g or x0");
  hipStream_t s = S(stream);
  if (op->n_lift < 0)
  {
    PMG_TRY(not_capturing(s, "pmg_laplacian_apply_lifting: the first call of an operator builds its cell list on the "
                             "host: not inside a stream capture"));
    PMG_TRY(build_lift_list(op, s));
  }
  PMG_TRY(scatter_fwd_whole(op->layout, g, s)); // ghosts of g (side effect, as pmg_laplacian_apply has on `in`)
  if (op->n_lift == 0)
    return PMG_OK;
  PMG_TRY(with_degree(op->P, [&](auto P) {
    launch_lifting<decltype(P)::value + 1>(op, g, x0, alpha, b, s);
    return PMG_OK;
  }));
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}

extern "C" int pmg_laplacian_lift_cell_count(pmg_laplacian op) { return op ? op->n_lift : -1; }

extern "C" int pmg_laplacian_set_bc(pmg_laplacian op, const double* g, const double* x0, double alpha, double* b,
                                    pmg_stream stream)
{
  PMG_REQUIRE(op && g && b, "pmg_laplacian_set_bc: NULL argument");
  const size_t total = (size_t)op->layout->total();
  PMG_REQUIRE(!overlaps(b, total, g, total) && !overlaps(b, total, x0, total), "pmg_laplacian_set_bc: b must not alias g or x0");
  const int n = op->layout->size_local;
  if (n > 0)
    set_bc_kernel<<<(n + 255) / 256, 256, 0, S(stream)>>>(n, op->bc, g, x0, alpha, b);
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}

extern "C" int pmg_laplacian_assemble_neumann(pmg_laplacian op, int32_t nfacets, const int32_t* facet_cells,
                                              const int8_t* facet_local, const double* h, double* b, pmg_stream stream)
{
  PMG_REQUIRE(op && b, "pmg_laplacian_assemble_neumann: NULL argument");
  PMG_REQUIRE(nfacets >= 0, "pmg_laplacian_assemble_neumann: negative facet count");
  if (nfacets == 0) // (an empty h has no address to ask for)
    return PMG_OK;
  PMG_REQUIRE(h && facet_cells && facet_local, "pmg_laplacian_assemble_neumann: NULL argument");
  const size_t nf = (size_t)op->nd * op->nd;
  PMG_REQUIRE(!overlaps(b, (size_t)op->layout->total(), h, (size_t)nfacets * nf),
              "pmg_laplacian_assemble_neumann: b must not alias h");
  PMG_TRY(check_facets(op, "pmg_laplacian_assemble_neumann", nfacets, facet_cells, facet_local));
  hipStream_t s = S(stream);
  PMG_TRY(not_capturing(s, "pmg_laplacian_assemble_neumann: not inside a stream capture (it uploads the facet lists)"));
  int32_t* d_cells = nullptr;
  int8_t* d_local = nullptr;
  PMG_HIP(hipMalloc(&d_cells, sizeof(int32_t) * nfacets));
  hipError_t e = hipMalloc(&d_local, sizeof(int8_t) * nfacets);
  if (e == hipSuccess)
    e = hipMemcpyAsync(d_cells, facet_cells, sizeof(int32_t) * nfacets, hipMemcpyHostToDevice, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(d_local, facet_local, sizeof(int8_t) * nfacets, hipMemcpyHostToDevice, s);
  if (e == hipSuccess)
  {
    const long long np = (long long)nfacets * (long long)nf;
    neumann_kernel<<<(unsigned)((np + 255) / 256), 256, 0, s>>>(np, op->nd, d_cells, d_local, h, op->dofmap, op->bc,
                                                              op->layout->size_local, op->xgeom, op->geom_dofmap, op->ng,
                                                              op->dphi_geom, op->W1, b);
    e = hipGetLastError();
  }
  if (e == hipSuccess)
    e = hipStreamSynchronize(s); // the lists are released below, the caller's host arrays on return
  (void)hipFree(d_cells);
  (void)hipFree(d_local);
  if (e != hipSuccess)
    return fail(PMG_ERR_HIP, "pmg_laplacian_assemble_neumann: %s", hipGetErrorString(e));
  return PMG_OK;
}

extern "C" int pmg_laplacian_has_robin(pmg_laplacian op) { return op ? (op->has_robin ? 1 : 0) : -1; }

extern "C" int pmg_laplacian_set_robin(pmg_laplacian op, int32_t nfacets, const int32_t* facet_cells,
                                       const int8_t* facet_local, const double* alpha, pmg_stream stream)
{
  PMG_REQUIRE(op, "pmg_laplacian_set_robin: NULL argument");
  PMG_REQUIRE(nfacets >= 0, "pmg_laplacian_set_robin: negative facet count");
  PMG_REQUIRE(nfacets == 0 || (alpha && facet_cells && facet_local), "pmg_laplacian_set_robin: NULL argument");
  PMG_TRY(check_facets(op, "pmg_laplacian_set_robin", nfacets, facet_cells, facet_local));
  hipStream_t s = S(stream);
  PMG_TRY(not_capturing(s, "pmg_laplacian_set_robin: not inside a stream capture (it allocates and synchronises)"));
  pmg_layout l = op->layout;
  const int total = l->total();
  const long long np = (long long)nfacets * op->nd * op->nd;
  // (a rank without a facet takes part with a count of zero, so the call is collective whatever each rank lists)
  PMG_TRY(require_valid(l, np, alpha, FiniteNonNegative{},
                        "pmg_laplacian_set_robin: %lld facet points have a value that is not finite and >= 0", s));
  if (nfacets == 0)
  {
    if (!op->has_robin)
      return PMG_OK;
    op->has_robin = false; // (a reaction term stays: the vector becomes d_sigma)
    return laplacian_data_changed(op, DATA_DIAGONAL_TERM, s);
  }
  int32_t* d_cells = nullptr;
  int8_t* d_local = nullptr;
  double* d_new = op->robin_buf;
  hipError_t e = hipSuccess;
  if (!d_new)
    e = hipMalloc(&d_new, sizeof(double) * (total ? total : 1));
  if (e == hipSuccess)
    e = hipMalloc(&d_cells, sizeof(int32_t) * nfacets);
  if (e == hipSuccess)
    e = hipMalloc(&d_local, sizeof(int8_t) * nfacets);
  if (e == hipSuccess)
    e = hipMemcpyAsync(d_cells, facet_cells, sizeof(int32_t) * nfacets, hipMemcpyHostToDevice, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(d_local, facet_local, sizeof(int8_t) * nfacets, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) // (nothing of the operator has changed so far: a failed allocation leaves it as it was)
  {
    op->robin_buf = d_new;
    // (summed with atomics in no fixed order: two sets of the same values agree to rounding, not bit for bit)
    e = hipMemsetAsync(op->robin_buf, 0, sizeof(double) * (total ? total : 1), s);
  }
  if (e == hipSuccess)
  {
    robin_kernel<<<(unsigned)((np + 255) / 256), 256, 0, s>>>(np, op->nd, d_cells, d_local, alpha, op->dofmap, op->bc,
                                                            total, op->xgeom, op->geom_dofmap, op->ng, op->dphi_geom, op->W1,
                                                            op->robin_buf);
    e = hipGetLastError();
  }
  if (e == hipSuccess)
    e = hipStreamSynchronize(s); // the lists are released below, the caller's host arrays on return
  (void)hipFree(d_cells);
  (void)hipFree(d_local);
  if (e != hipSuccess)
  {
    if (!op->robin_buf)
      (void)hipFree(d_new);
    return fail(PMG_ERR_HIP, "pmg_laplacian_set_robin: %s", hipGetErrorString(e));
  }
  op->has_robin = true;
  return laplacian_data_changed(op, DATA_DIAGONAL_TERM, s);
}
