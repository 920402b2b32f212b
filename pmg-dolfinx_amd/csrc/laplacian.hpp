// The operator handle, shared by the FP64 (laplacian.hip) and FP32 (laplacian_f32.hip) forms of the apply.
#pragma once

#include "common.hpp"
#include "patches.hpp"

#include <algorithm>

struct pmg_laplacian_s
{
  pmg_layout layout = nullptr;
  int P = 0, nd = 0, N = 0, K = 0;
  int32_t ncells = 0, npoints = 0;
  // caller-owned
  const double* kappa = nullptr;
  const int32_t* dofmap = nullptr;
  const double* xgeom = nullptr;
  const int32_t* geom_dofmap = nullptr;
  const int8_t* bc = nullptr;
  // marked entries among the owned ones, counted at creation, and their sum over the ranks (-1: not yet reduced;
  // laplacian_require_singular)
  long long n_marked = 0, n_marked_global = -1;
  // cell-local node order of the caller's arrays (pmg_amd.h): the kernels index nodes by ascending coordinate, so a
  // caller in another order gets an ascending copy of its dofmap (op->dofmap then points to it) and its
  // quadrature-indexed arrays are permuted on the way in (tables) and out (get_geometry)
  int node_order = PMG_NODES_ASCENDING;
  int32_t* dofmap_own = nullptr; // [ncells * N], ascending order; nullptr = the caller's array is used as it is
  int32_t* qperm = nullptr;      // [N] device: caller's cell-local number -> ascending; nullptr = identity
  // owned
  double2* G = nullptr;        // [nslots][3][N]
  // nodal coefficient (pmg_laplacian_set_coefficient_field): folded into G, and into the float tensor, where they are
  // built (point_tensor); nullptr = none
  double* kfield = nullptr;    // [size_local + num_ghosts], ghosts filled by the layout's forward scatter
  long long kfield_epoch = 0;  // bumped when kfield is allocated or freed (laplacian_capture_state, batch mode)
  // per-cell diffusion tensor (pmg_laplacian_set_coefficient_tensor): symmetric positive definite, physical
  // coordinates, (xx, xy, xz, yy, yz, zz); folded into G, the float tensor and Gaff where they are built
  // (G_q = adj(J) K_c adj(J)^T w_q / detJ); nullptr = none.  Allocating or freeing it bumps kfield_epoch.
  double* ktensor = nullptr;   // [ncells][6]
  // reaction term (pmg_laplacian_set_reaction): y = A x + react .* x on unmarked rows.  GLL collocation makes the mass
  // matrix diagonal, so the term is one vector, react[dof] = sum over the listed cells' points on the dof of
  // sigma_c w_q detJ_q (0 on marked dofs); it does not depend on G.  The apply kernels start the first patch's
  // accumulator of a dof at react[dof] * x[dof] (stiffness_column.hpp); nullptr = none.  With a Robin boundary term
  // (pmg_laplacian_set_robin) the vector is d_sigma + d_R, or d_R alone: see sigma_buf / robin_buf below.
  double* react = nullptr;     // [size_local + num_ghosts], ghost entries as diag_inv's: this rank's cells only
  float* react32 = nullptr;    // float copy, present while react and the float tensor G32 both are
  // the two allocations behind them, made on first need and kept until the handle goes: a term that is removed and set
  // again has its vectors where a captured graph of the first one read them (laplacian_capture_state tells set from
  // removed, not one allocation from the next)
  double* react_buf = nullptr;
  float* react32_buf = nullptr;
  // The vector has two components, set and removed independently: d_sigma (pmg_laplacian_set_reaction) and d_R, the
  // face mass of a Robin boundary term (pmg_laplacian_set_robin, boundary.hip).  Each is kept in a buffer of its own,
  // made on first need and kept with the handle; `react` is an exact copy of the only one present, or d_sigma + d_R in
  // that order (laplacian_data_changed), always in react_buf.
  double* sigma_buf = nullptr; // d_sigma [size_local + num_ghosts]
  double* robin_buf = nullptr; // d_R     [size_local + num_ghosts]
  bool has_sigma = false, has_robin = false;
  bool diag_computed = false;  // diag_inv came from pmg_laplacian_compute_diag_inverse (it follows a change of field)
  double* Gaff = nullptr;      // [nslots][6] constant tensor K K^T / detJ of each (affine) cell (K Kc K^T / detJ with a coefficient tensor)
  double* W1 = nullptr;        // [2][nd] + 1: 1-D GLL weights, the nodes on [0,1], the column-tensor switch (1 = on)
  // Recomputed tensor (pmg_laplacian_set_tensor_recompute, laplacian_recomputes_tensor): the apply of a trilinear
  // operator forms G in its layer march from Ccell instead of streaming it.  Ccell follows the geometry alone; it is
  // built when the form is first chosen (at creation where it is the default) and kept.
  double* Ccell = nullptr;     // [nslots][8][3] monomial coefficients c_ijk of x = sum c_ijk xi^i eta^j zeta^k, m = 4i+2j+k
  bool own_tables = false;     // the library built the coordinate element's tabulation and the weights itself
  int recompute_request = -1;  // -1 = automatic (per degree), 0 = always stream, 1 = recompute where eligible
  int recompute_identity_request = -1; // the same for degree 4 (pmg_laplacian_set_tensor_recompute_identity)
  int column_tensor_request = -1;      // the column-constant branch of either form (pmg_laplacian_set_column_tensor): 0 = off
  bool all_affine = false;     // every listed cell is a parallelepiped
  int geometry_mode = 0;       // 0 = stored G (reference data structure), 1 = affine cells
  double* D = nullptr;         // [nd*nd]
  double* dphi_geom = nullptr; // [3][N][ng]
  // coordinate element (pmg_laplacian_create_curved): tensor-product Lagrange of degree geom_degree, ng = (g + 1)^3
  // nodes per cell in ascending tensor order.  geom_L / geom_Lp [nd][g + 1]: its 1-D basis and derivative at the
  // operator's GLL points, present when the library built the tabulation itself and g >= 2 -- the cell-cooperative
  // geometry kernel contracts with them (tensor_kernels.hpp); nullptr with caller tables (per-point dense path).
  int geom_degree = 1, ng = 8;
  double* geom_L = nullptr;
  double* geom_Lp = nullptr;
  double* gweights = nullptr;  // [N]
  int32_t* pcell = nullptr;    // [npatch*K]
  int32_t* pncell = nullptr;   // [npatch]
  int32_t* bzero = nullptr;    // dofs first written by the (atomic) boundary launch
  int32_t n_bzero = 0;
  int32_t* poff = nullptr;     // [npatch+1]
  uint32_t* pdofs = nullptr;
  int32_t* lmap_id = nullptr;  // [npatch]
  uint16_t* lmaps = nullptr;   // [nuniq][K*N]
  int32_t npatch = 0;
  std::vector<int32_t> launch_first, launch_count;
  // two halves of the interior on two streams (PatchPlan::launch_stream): the second stream and its fork / order /
  // join events
  std::vector<int8_t> launch_stream;
  int launch_signal = -1, launch_wait = -1;
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_order = nullptr, ev_join = nullptr;
  std::vector<int32_t> pcell_h, pncell_h; // host copies for components that share the patches
  long long npdofs = 0;
  int max_m = 0;
  int n_launch_l = 0;
  int n_plain = 0;
  bool needs_zero = false; // some local dof belongs to no listed cell
  // chain form of the interior launches (patches.hpp ChainPlan, stiffness_chain_kernel): available / in use
  bool chain_ok = false, chain_on = false;
  uint32_t* cdofs = nullptr;
  uint32_t* ccar = nullptr;
  int32_t* chain_off = nullptr;
  int32_t* chain_patch = nullptr;
  std::vector<int32_t> chain_first, chain_count; // chains of each colour
  bool stream_policy = true; // the stored tensor exceeds the Infinity Cache: nt loads / stores (launch_stiffness)
  bool stream_policy32 = false; // the same decision for the float tensor, taken where it is built (laplacian_f32_prepare)
  double* diag_inv = nullptr; // [size_local + num_ghosts]
  bool have_diag = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  long long launches = 0; // full operator applications' kernel launches since creation
  long long applies = 0;
  // geometry batching (src/laplacian.hpp:383-396): > 0 = G is not resident; it is recomputed for
  // `batch_patches` patches at a time into a buffer of that size, in every application
  int32_t batch_patches = 0;
  // in-situ timing of the stiffness launches (pmg_laplacian_set_profiling)
  bool profiling = false;
  std::vector<hipEvent_t> prof_events; // pairs: before / after a run of launches
  size_t prof_used = 0;
  long long prof_launches = 0;
  // single-precision form of the operator (laplacian_f32.hip; built on first use, freed with the handle)
  float2* G32 = nullptr;          // [nslots][layer c][3][nd*nd]: G (without kappa, with the coefficient field), rounded once (the default layout of G)
  float* D32 = nullptr;           // [nd*nd]
  float* diag32 = nullptr;        // [size_local + num_ghosts] float copy of diag_inv
  long long diag_version = 0;     // bumped whenever diag_inv changes; diag32 is current while the two agree
  long long diag32_version = -1;
  // boundary data (boundary.hip): the listed cells that hold a marked dof, built on the first
  // pmg_laplacian_apply_lifting (n_lift < 0: not yet) and freed with the handle; which cells are listed at all
  // (host, built at creation)
  int32_t* lift_cells = nullptr;
  int32_t n_lift = -1;
  std::vector<char> listed;
  // the same on the device, one byte per cell of the dofmap, uploaded with the cell lists at creation: which cells the
  // apply visits (pmg_laplacian_form_gradients sums d_field over them alone)
  int8_t* cell_listed = nullptr;
};

namespace pmg
{
// Is a tensor of this many bytes, read once per application, streamed past the Infinity Cache (nt loads and stores)?
// Asked where a tensor is built or resized, never per application; it reads PMG_STREAM_POLICY (laplacian.hip).
bool streams_past_the_cache(long long tensor_bytes);

// The launches [l0, l1) of the operator's plan under `form` (patches.hpp for_each_launch_step) as HIP calls on `s` and
// on the operator's second stream; launch(step, stream) issues the kernels of a PATCHES or CHAINS step.  Both precisions
// apply through this walk.  With profiling on, the walk is bracketed by a pair of events and the steps that launch are
// counted (pmg_laplacian_read_profile).
template <typename L>
int walk_launches(pmg_laplacian op, int l0, int l1, ApplyForm form, hipStream_t s, L&& launch)
{
  const bool prof = op->profiling && l1 > l0;
  if (prof)
  {
    while (op->prof_events.size() < op->prof_used + 2)
    {
      hipEvent_t e;
      PMG_HIP(hipEventCreate(&e));
      op->prof_events.push_back(e);
    }
    PMG_HIP(hipEventRecord(op->prof_events[op->prof_used], s));
  }
  int issued = 0;
  // (inside a stream capture the fork and the join make the two halves two branches of the graph)
  PMG_TRY(for_each_launch_step(*op, op->chain_first, op->chain_count, l0, l1, form, [&](const LaunchStep& st) -> int {
    switch (st.kind)
    {
    case LaunchStep::FORK:
      PMG_HIP(hipEventRecord(op->ev_fork, s));
      PMG_HIP(hipStreamWaitEvent(op->stream2, op->ev_fork, 0));
      break;
    case LaunchStep::WAIT_ORDER:
      PMG_HIP(hipStreamWaitEvent(s, op->ev_order, 0));
      break;
    case LaunchStep::RECORD_ORDER:
      PMG_HIP(hipEventRecord(op->ev_order, op->stream2));
      break;
    case LaunchStep::JOIN:
      PMG_HIP(hipEventRecord(op->ev_join, op->stream2));
      PMG_HIP(hipStreamWaitEvent(s, op->ev_join, 0));
      break;
    default:
      PMG_TRY(launch(st, st.stream ? op->stream2 : s));
      ++issued;
    }
    return PMG_OK;
  }));
  PMG_HIP(hipGetLastError());
  if (prof)
  {
    PMG_HIP(hipEventRecord(op->prof_events[op->prof_used + 1], s));
    op->prof_used += 2;
    op->prof_launches += issued;
  }
  return PMG_OK;
}

// ---- validation of a caller's device array: what one entry must be ... ----
struct FinitePositive // finite and > 0 (the nodal field)
{
  __device__ bool operator()(const double* __restrict__ v, long long i) const
  {
    return v[i] > 0.0 && v[i] <= 1.79769313486231570e308; // NaN fails the first comparison, +inf the second
  }
};
struct FiniteNonNegative // finite and >= 0; all zeros is legal (reaction and Robin values)
{
  __device__ bool operator()(const double* __restrict__ v, long long i) const
  {
    return v[i] >= 0.0 && v[i] <= 1.79769313486231570e308;
  }
};
struct FiniteSpd // six values (xx, xy, xz, yy, yz, zz) per entry: finite, symmetric positive definite (the cell tensor)
{
  __device__ bool operator()(const double* __restrict__ v, long long i) const
  {
    const double* t = v + i * 6;
    const double xx = t[0], xy = t[1], xz = t[2], yy = t[3], yz = t[4], zz = t[5];
    bool ok = true;
    for (int d = 0; d < 6; ++d)
      ok = ok && fabs(t[d]) <= 1.79769313486231570e308; // NaN and +-inf fail
    // leading minors: xx > 0, xx yy - xy^2 > 0, det > 0
    const double m2 = xx * yy - xy * xy;
    const double det = xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz) + xz * (xy * yz - yy * xz);
    return ok && xx > 0.0 && m2 > 0.0 && det > 0.0;
  }
};

// ... the number of entries of v[0, n) that are not, added to *bad (zeroed by the caller) ...
template <typename Valid>
__global__ void count_invalid_kernel(long long n, const double* __restrict__ v, double* __restrict__ bad, Valid valid)
{
  int mine = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    mine += !valid(v, i);
  if (mine)
    atomicAdd(bad, (double)mine);
}

// ... and the refusal: the count is summed over the ranks through the layout's reduction slot, so all of them refuse,
// or none (a rank with n = 0 takes part with a count of zero: the call is collective).  `message` is the caller's, with
// one %lld for the count.  Reads back: not inside a stream capture.
template <typename Valid>
int require_valid(pmg_layout l, long long n, const double* v, Valid valid, const char* message, hipStream_t s)
{
  double* bad = red_slot(l, 0);
  PMG_HIP(hipMemsetAsync(bad, 0, sizeof(double), s));
  if (n > 0)
    count_invalid_kernel<<<(unsigned)std::min<long long>((n + 255) / 256, 1024), 256, 0, s>>>(n, v, bad, valid);
  PMG_HIP(hipGetLastError());
  PMG_TRY(reduce_slots_async(l, 0, 1, false, s));
  double nbad = 0.0;
  PMG_TRY(fetch_slots(l, 0, 1, &nbad, s));
  if (nbad != 0.0)
    return fail(PMG_ERR_INVALID, message, (long long)nbad);
  return PMG_OK;
}

// adj(J) and |det J| of a Jacobian: the one cofactor expansion.  Full expansion along the first row (the reference's
// :97 drops to the diagonal-J special case).  |det J|: a cell's local frame may be left-handed (vertex order of an
// imported mesh); the volume measure, G, the load and the reaction weights do not depend on it.  K keeps its sign: it
// enters G twice and the facet measure through a norm.  (fabs changes no bit of a positive determinant.)
__device__ __forceinline__ void adjugate(const double J[3][3], double K[3][3], double& detJ)
{
  K[0][0] = J[1][1] * J[2][2] - J[1][2] * J[2][1];
  K[0][1] = -J[0][1] * J[2][2] + J[0][2] * J[2][1];
  K[0][2] = J[0][1] * J[1][2] - J[0][2] * J[1][1];
  K[1][0] = -J[1][0] * J[2][2] + J[1][2] * J[2][0];
  K[1][1] = J[0][0] * J[2][2] - J[0][2] * J[2][0];
  K[1][2] = -J[0][0] * J[1][2] + J[0][2] * J[1][0];
  K[2][0] = J[1][0] * J[2][1] - J[1][1] * J[2][0];
  K[2][1] = -J[0][0] * J[2][1] + J[0][1] * J[2][0];
  K[2][2] = J[0][0] * J[1][1] - J[0][1] * J[1][0];
  detJ = fabs(J[0][0] * K[0][0] + J[0][1] * K[1][0] + J[0][2] * K[2][0]);
}

// ---- geometry: J, adj(J), |det| at one quadrature point (src/laplacian.hpp:72-97) of a cell whose coordinate element
// has NG nodes (dense table [3][nq][NG], gdofs = the cell's nodes).  NG = 8, the trilinear element: the node loop is
// unrolled over a compile-time count.  NG = 0: the run-time count `ng` (degree >= 2). ----
template <int NG>
__device__ inline void jacobian(const double* __restrict__ xgeom, const int32_t* __restrict__ gdofs,
                                const double* __restrict__ dphi, int nq, int q, int ng, double K[3][3], double& detJ)
{
  static_assert(NG == 8 || NG == 0, "a compile-time node count other than the trilinear element's has no instantiation");
  double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  const int n = NG ? NG : ng;
  const double *t0 = dphi + (size_t)q * ng, *t1 = t0 + (size_t)nq * ng, *t2 = t1 + (size_t)nq * ng; // (NG = 0)
  for (int k = 0; k < n; ++k)
  {
    const double* xk = xgeom + 3 * (size_t)gdofs[k];
    const double x0 = xk[0], x1 = xk[1], x2 = xk[2];
    const double d0 = NG ? dphi[(0 * nq + q) * NG + k] : t0[k], d1 = NG ? dphi[(1 * nq + q) * NG + k] : t1[k],
                 d2 = NG ? dphi[(2 * nq + q) * NG + k] : t2[k];
    J[0][0] += x0 * d0;
    J[0][1] += x0 * d1;
    J[0][2] += x0 * d2;
    J[1][0] += x1 * d0;
    J[1][1] += x1 * d1;
    J[1][2] += x1 * d2;
    J[2][0] += x2 * d0;
    J[2][1] += x2 * d1;
    J[2][2] += x2 * d2;
  }
  adjugate(J, K, detJ);
  // The trilinear form has always rounded J00 K00 on its own and fused the other two products onto it; left to the
  // compiler, the expression in adjugate() rounds J01 K10 first here, which moves |det J| of a sheared cell by a few
  // ulps (profiles/point_geometry.md).  Degree-1 operators keep their bits: the contraction is written out.
  if constexpr (NG == 8)
    detJ = fabs(fma(J[0][2], K[2][0], fma(J[0][1], K[1][0], J[0][0] * K[0][0])));
}

// The same for a run-time node count: the trilinear element goes to its own form, so a degree-1 operator computes
// what it always did.
__device__ inline void jacobian(const double* __restrict__ xgeom, const int32_t* __restrict__ gdofs,
                                const double* __restrict__ dphi, int nq, int q, int ng, double K[3][3], double& detJ)
{
  if (ng == 8)
    return jacobian<8>(xgeom, gdofs, dphi, nq, q, 8, K, detJ);
  jacobian<0>(xgeom, gdofs, dphi, nq, q, ng, K, detJ);
}

// ---- the six entries of adj(J) adj(J)^T * s (src/laplacian.hpp:99-111); K = adj(J) as jacobian() returns it ----
__device__ __forceinline__ void metric(const double K[3][3], double s, double g[6])
{
  g[0] = (K[0][0] * K[0][0] + K[0][1] * K[0][1] + K[0][2] * K[0][2]) * s;
  g[1] = (K[1][0] * K[0][0] + K[1][1] * K[0][1] + K[1][2] * K[0][2]) * s;
  g[2] = (K[2][0] * K[0][0] + K[2][1] * K[0][1] + K[2][2] * K[0][2]) * s;
  g[3] = (K[1][0] * K[1][0] + K[1][1] * K[1][1] + K[1][2] * K[1][2]) * s;
  g[4] = (K[2][0] * K[1][0] + K[2][1] * K[1][1] + K[2][2] * K[1][2]) * s;
  g[5] = (K[2][0] * K[2][0] + K[2][1] * K[2][1] + K[2][2] * K[2][2]) * s;
}

// ---- the six entries of adj(J) T adj(J)^T * s for a symmetric T = (xx, xy, xz, yy, yz, zz) in physical coordinates:
// M = adj(J) T (nine dot products from the six values), then the upper triangle of M adj(J)^T.  K = adj(J) as
// jacobian() returns it (row = reference direction, column = physical direction). ----
__device__ __forceinline__ void tensor_geometry(const double K[3][3], const double t[6], double s, double g[6])
{
  double M[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
  {
    M[a][0] = K[a][0] * t[0] + K[a][1] * t[1] + K[a][2] * t[2];
    M[a][1] = K[a][0] * t[1] + K[a][1] * t[3] + K[a][2] * t[4];
    M[a][2] = K[a][0] * t[2] + K[a][1] * t[4] + K[a][2] * t[5];
  }
  g[0] = (M[0][0] * K[0][0] + M[0][1] * K[0][1] + M[0][2] * K[0][2]) * s;
  g[1] = (M[1][0] * K[0][0] + M[1][1] * K[0][1] + M[1][2] * K[0][2]) * s;
  g[2] = (M[2][0] * K[0][0] + M[2][1] * K[0][1] + M[2][2] * K[0][2]) * s;
  g[3] = (M[1][0] * K[1][0] + M[1][1] * K[1][1] + M[1][2] * K[1][2]) * s;
  g[4] = (M[2][0] * K[1][0] + M[2][1] * K[1][1] + M[2][2] * K[1][2]) * s;
  g[5] = (M[2][0] * K[2][0] + M[2][1] * K[2][1] + M[2][2] * K[2][2]) * s;
}

// G_q from adj(J) and |det J| at the point q of cell c, the one place that forms it: w_q / detJ, times the nodal
// coefficient at the point's own dof (kfield, optional; GLL collocation: the points are the nodes), with the per-cell
// tensor between the two adjugates when one is set (ktensor, optional, [ncells][6]).  The tensor's six values are one
// 48-byte read per cell, the same address for (nearly) every lane of a wavefront; the address depends on the cell
// alone, not on anything computed per point.  The read is written inside the branch, after the caller's Jacobian:
// hoisted above it, it holds twelve more registers across the Jacobian's gathers (in the 8-node per-point kernel 68
// VGPRs and 7 waves per SIMD instead of 60 and 8, with or without a tensor).  Without a tensor the branch is uniform
// and not taken.
__device__ __forceinline__ void point_tensor(const double K[3][3], double detJ, int c, int nq, int q, const double* w,
                                             const double* kfield, const int32_t* dofmap, const double* ktensor,
                                             double g[6])
{
  double s = w[q] / detJ;
  if (kfield)
    s *= kfield[dofmap[(size_t)c * nq + q]];
  if (ktensor)
    tensor_geometry(K, ktensor + (size_t)c * 6, s, g);
  else
    metric(K, s, g);
}

// ---- the cell-local kernels that form G_q in place (boundary.hip: lifting; cell_form.hip: the bilinear form) ----
// One thread per node.  Degree >= 3: one cell per workgroup (64 .. 729 nodes, rounded up to whole wavefronts);
// degree <= 2: several cells, so that a full workgroup has at least 64 busy lanes.
template <int ND>
struct LiftShape
{
  static constexpr int N = ND * ND * ND;
  static constexpr int CPW = N >= 64 ? 1 : (64 + N - 1) / N; // 8 cells at degree 1, 3 at degree 2
  static constexpr int THREADS = ((CPW * N + 63) / 64) * 64;
};

// the sum over the 64 lanes of a wavefront, in lane 0: a fixed tree (the cell-local kernels' per-cell sums)
__device__ __forceinline__ double wave_sum(double x)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    x += __shfl_down(x, off, 64);
  return x;
}

// do p[0, np) and q[0, nq) share memory?
inline bool overlaps(const double* p, size_t np, const double* q, size_t nq)
{
  if (!p || !q)
    return false;
  const uintptr_t a = (uintptr_t)p, c = (uintptr_t)q;
  return a < c + nq * sizeof(double) && c < a + np * sizeof(double);
}
} // namespace pmg
