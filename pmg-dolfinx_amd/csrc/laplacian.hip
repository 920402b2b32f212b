// Matrix-free GLL-collocated Laplacian for gfx950: geometry tensor, the
// sum-factorised stiffness kernel, matrix-free diagonal, collocated load vector.
// Replaces src/laplacian.hpp (geometry_computation :22-113, stiffness_operator
// :143-278, MatFreeLaplacian :284-526) of the reference.
//
// Work decomposition: cells are grouped into coloured patches (patches.hpp: 2x2x8
// cells at P = 4); one workgroup of up to 8 wavefronts applies the operator to one
// patch.  A wavefront takes whole cells (2 at P = 4; at P = 8 two wavefronts share
// one), a lane owns the column of nd points above (a, b), keeps it in registers and
// marches through the nd layers (stiffness_column_kernel, stiffness_column.hpp).
//
// HBM layout (owned by the handle):
//   G      [slot][layer c][3][nd*nd] double2 : (G00,G01) (G02,G11) (G12,G22) per
//          quadrature point, slot = patch * K + position in the patch, so one layer
//          of one cell is 3 contiguous runs of nd*nd double2 (the reference stores
//          [cell][q][6] AoS, 48-byte stride per lane, src/laplacian.hpp:221-227);
//          P = 2 uses the line-aligned flat variant described at gflat() (geometry_kernels.hpp).
//   pdofs  [poff[p] .. poff[p+1]) uint32 : sorted dofs of patch p, Dirichlet and
//          "already written" flags in the top bits -- replaces the per-thread
//          dofmap load + dependent 1-byte bc_marker gather (:182-189) and the
//          zero-fill of y (:466).
//   lmaps  [table][K*N] uint16 : position of (cell slot, layer-major local dof) in the
//          patch list; identical patches share one table (a structured box has one
//          table for all interior patches, so it stays in L2).
//   D      [nd][nd] double : 1-D derivative table (LDS -> registers / SGPRs).
//
// LDS per workgroup: patch x values and patch y accumulators (2 * max_m doubles, 43 KB
// at P = 4) plus three nd x nd slices per cell in flight.  Cell contributions are summed
// with LDS FP64 atomics (ds_add_f64), the global write is a plain store /
// read-modify-write (coloured launches) or one global atomic per patch dof (merged
// launches of small levels and of the boundary shell).
//
// Roofline: HBM-bound, AI 0.85 (P=1) .. 2.05 (P=8) flop/B; algorithmic bytes per
// cell 48N + 4N + 8 + 17U (model "storedG").
//
// One translation unit, five files and two headers.  stiffness_layer.hpp (a real header, shared with laplacian_f32.hip)
// holds the layer march of the four apply kernels: fences, loads, the lane's table rows, the two halves of a layer, the
// packed positions and the tensor stream; tensor_kernels.hpp (shared likewise) the kernels that build the geometry
// tensor.  The fragments are included below, inside the anonymous namespace, in this order:
//   geometry_kernels.hpp  layout of G (gflat, gpatch, gpos); affine-tensor, export, diagonal, load and reaction kernels
//   stiffness_column.hpp  Shape<P> and its policies, write-back, diagnostic stamps, stiffness_column_kernel
//   stiffness_chain.hpp   ChainShape<P>, stiffness_chain_kernel (P = 4)
//   stiffness_restrict.hpp  stiffness_restrict_kernel: the apply fused with the restriction of r - A z
//   laplacian.hip         the host side: launch plan, run_launches, the C ABI
#include "laplacian.hpp"
#include "tensor_kernels.hpp"
#include "stiffness_layer.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>

using namespace pmg;


namespace
{
#include "geometry_kernels.hpp"
#include "stiffness_column.hpp"
#include "stiffness_chain.hpp"
#include "stiffness_restrict.hpp"

// where the geometry kernels (tensor_kernels.hpp) put a point's six values: the stored tensor's layout
struct TensorOut64
{
  double2* G; // absolute slot positions (batch_geometry)
  int nd, K;
  __device__ __forceinline__ void operator()(long long slot, int q, const double g[6]) const
  {
    G[gpos(nd, K, slot, q, 0)] = make_double2(g[0], g[1]);
    G[gpos(nd, K, slot, q, 1)] = make_double2(g[2], g[3]);
    G[gpos(nd, K, slot, q, 2)] = make_double2(g[4], g[5]);
  }
};

__global__ void zero_list_kernel(int n, const int32_t* __restrict__ idx, double* __restrict__ y)
{
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    y[idx[i]] = 0.0;
}

// geometry of the patches [first, first + count) into the (batch) buffer; returns the base pointer
// to hand to kernels that index G by absolute patch slot
const double2* batch_geometry(pmg_laplacian op, int first, int count, hipStream_t s)
{
  double2* base = op->G - (size_t)first * gpatch(op->nd, op->K);
  launch_geometry(op, (long long)first * op->K, (long long)count * op->K, TensorOut64{base, op->nd, op->K}, s);
  return base;
}

// The two tensors that are rebuilt in place, by the constructor and by laplacian_data_changed: the resident G (in
// batched-geometry mode there is none: every application recomputes its batches) ...
int rebuild_resident_tensor(pmg_laplacian op, hipStream_t s)
{
  if (op->batch_patches == 0 && op->npatch > 0)
    batch_geometry(op, 0, op->npatch, s);
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}

// ... and Gaff, one constant tensor per (affine) cell
int rebuild_affine_tensor(pmg_laplacian op, hipStream_t s)
{
  const long long nslots = (long long)op->npatch * op->K;
  if (nslots > 0)
    affine_geometry_kernel<<<(unsigned)((nslots + 255) / 256), 256, 0, s>>>(nslots, op->geom_degree, op->pcell,
                                                                           op->xgeom, op->geom_dofmap, op->ktensor,
                                                                           op->Gaff);
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}

// ---- the recomputed tensor (GEO_RECOMPUTE, stiffness_layer.hpp) ----
// Degrees whose column kernel (and fused pair) has the form, and those where it is the automatic choice: decided by
// measurement, profiles/tensor_recompute.md.  From P = 3 the 15 values per lane do not fit beside the march as it is
// written for these degrees.
constexpr bool recompute_form(int P) { return P == 1 || P == 2; }
constexpr bool recompute_default(int P) { return P == 1 || P == 2; }
// Degree 4 has the form with its transposes by identity (transposes_by_identity, stiffness_column.hpp), which is what
// makes the 15 values fit.  It has a switch of its own (pmg_laplacian_set_tensor_recompute_identity): the first one
// keeps its contract, under which a degree-4 operator has no form.  Automatic = on, by measurement
// (profiles/tensor_recompute_p4.md).
constexpr bool recompute_identity_form(int P) { return P == 4; }
constexpr bool recompute_identity_default(int P) { return P == 4; }
constexpr bool recompute_kernel(int P) { return recompute_form(P) || recompute_identity_form(P); }

// Could this operator's apply recompute its tensor at all?  What never changes after creation: a trilinear coordinate
// element with the library's own tabulation and weights, at a degree that has the form.
bool recompute_possible(pmg_laplacian op) { return op->geom_degree == 1 && op->own_tables && recompute_kernel(op->P); }
// (each degree listens to its own switch)
bool recompute_wanted(pmg_laplacian op)
{
  if (recompute_identity_form(op->P))
    return op->recompute_identity_request == 1
           || (op->recompute_identity_request < 0 && recompute_identity_default(op->P));
  return op->recompute_request == 1 || (op->recompute_request < 0 && recompute_default(op->P));
}
// ... and does its next application?  The one place that decides: resident geometry in the stored mode, no nodal field
// and no per-cell tensor (both are folded into G where it is built, and the form carries neither), not the chain form
// (degree 4: the chain kernel streams).  Evaluated at every use, so it follows a field or tensor that is set or
// removed, the geometry mode, the batching and the chain form.
bool recomputes_tensor(pmg_laplacian op)
{
  return recompute_possible(op) && recompute_wanted(op) && op->Ccell && op->batch_patches == 0
         && op->geometry_mode == 0 && !op->kfield && !op->ktensor && !op->chain_on;
}
// The column-constant branch of the form (TensorStream::column_constant, stiffness_layer.hpp): items whose Jacobian does
// not change down their columns form the tensor once per item.  A switch of its own (pmg_laplacian_set_column_tensor),
// automatic = on by measurement (profiles/column_tensor.md); it only means something where the apply recomputes.
bool hoists_column_tensor(pmg_laplacian op)
{
  return column_branch(op->P) && recomputes_tensor(op) && op->column_tensor_request != 0;
}
// The kernels of the form read the request from W1's last entry (stiffness_column.hpp): written at creation and by the
// setter.  Synchronous, on the default stream: not inside a stream capture.
int store_column_switch(pmg_laplacian op)
{
  const double on = op->column_tensor_request != 0 ? 1.0 : 0.0;
  PMG_HIP(hipMemcpy(op->W1 + 2 * op->nd, &on, sizeof(on), hipMemcpyHostToDevice));
  return PMG_OK;
}

// How many of the operator's items qualify, by the predicate the apply evaluates (TensorStream::column_constant on the
// lanes' values of an item, formed as the kernels form them): one wavefront per item, count[0] += qualifies,
// count[1] += 1.
template <int P>
__global__ void __launch_bounds__(64)
    column_items_kernel(const double* __restrict__ Ccell, const double* __restrict__ W1,
                        const int32_t* __restrict__ pncell, unsigned long long* __restrict__ count)
{
  using Sh = Shape<P>;
  constexpr int ND = Sh::ND, K = Sh::K, NQ2 = Sh::NQ2, CW = Sh::CW, ITEMS = Sh::ITEMS, WL = CW * NQ2;
  static_assert(Sh::WPC == 1, "the recomputed form covers the one-wave-per-item shapes only");
  const int p = blockIdx.x / ITEMS, it = blockIdx.x - p * ITEMS;
  if (it >= (pncell[p] + CW - 1) / CW)
    return;
  const int lane = threadIdx.x;
  const int lw = lane < WL ? lane : WL - 1; // (the lane's column, cell and slot: stiffness_column_kernel)
  const int cw = lw / NQ2, ab = lw - cw * NQ2;
  const int a = ab / ND, b = ab - a * ND;
  const int slot = it * CW + cw;
  const int slotc = slot < K ? slot : K - 1;
  TensorStream<double2, ND, WL, GEO_RECOMPUTE, false, 0, false, 1> gs;
  gs.prime_recompute(Ccell + ((size_t)p * K + slotc) * 24, W1[ND + a], W1[ND + b], W1[a] * W1[b], W1 + ND);
  const bool constant = gs.column_constant();
  if (lane == 0)
  {
    atomicAdd(&count[0], constant ? 1ull : 0ull);
    atomicAdd(&count[1], 1ull);
  }
}

// Ccell, built once when the form is first chosen (the geometry never changes)
int ensure_cell_coefficients(pmg_laplacian op, hipStream_t s)
{
  if (op->Ccell || !recompute_possible(op) || !recompute_wanted(op))
    return PMG_OK;
  const long long nslots = (long long)op->npatch * op->K;
  PMG_HIP(hipMalloc(&op->Ccell, sizeof(double) * 24 * (nslots ? nslots : 1)));
  if (nslots > 0)
    cell_coefficient_kernel<<<(unsigned)((nslots * 3 + 255) / 256), 256, 0, s>>>(nslots, op->pcell, op->xgeom,
                                                                                 op->geom_dofmap, op->Ccell);
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}

// f(first patch, patch count, G base) over all patches: once with the resident tensor, or batch by
// batch with the tensor recomputed into the batch buffer
template <typename F>
int for_each_geometry_chunk(pmg_laplacian op, hipStream_t s, F f)
{
  if (op->npatch == 0)
    return PMG_OK;
  if (op->batch_patches <= 0)
    f(0, op->npatch, op->G);
  else
    for (int first = 0; first < op->npatch; first += op->batch_patches)
    {
      const int count = std::min(op->batch_patches, op->npatch - first);
      f(first, count, batch_geometry(op, first, count, s));
    }
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}

// The (GEO, NT) instantiation of an apply kernel that an operator runs, chosen in one place: launch(GEO, NT) is called
// with the two as std::integral_constant / std::bool_constant, and with the per-slot array the form reads beside G
// (Gaff, Ccell).  Cache policy: a tensor that is read once per application and is larger than the
// Infinity Cache is streamed (nt), so that it does not displace x, y and the tables; a tensor that fits stays resident
// between two applications under the default policy (streams_past_the_cache; profiles/kernel_tuning_r03.md).  The
// affine mode and the recomputed form read no tensor: AFFINE_NT is the kernel's one instantiation for them.
template <int G>
using geo_constant = std::integral_constant<int, G>;
template <int P, bool AFFINE_NT, typename F>
void apply_variant(pmg_laplacian op, F launch)
{
  if constexpr (recompute_kernel(P))
  {
    if (recomputes_tensor(op))
      return launch(geo_constant<GEO_RECOMPUTE>{}, std::bool_constant<AFFINE_NT>{}, (const double*)op->Ccell);
  }
  if (op->geometry_mode == 1)
    launch(geo_constant<GEO_AFFINE>{}, std::bool_constant<AFFINE_NT>{}, (const double*)op->Gaff);
  else if (P >= NT_FROM && op->stream_policy)
    launch(geo_constant<GEO_STORED>{}, std::true_type{}, (const double*)op->Gaff);
  else
    launch(geo_constant<GEO_STORED>{}, std::false_type{}, (const double*)op->Gaff);
}

template <int P>
int launch_stiffness(pmg_laplacian op, const double* x, double* y, int first, int count,
                     int atomic_out, hipStream_t s)
{
  if (count <= 0)
    return PMG_OK;
  if (op->batch_patches > 0 && op->geometry_mode == 0 && count > op->batch_patches)
  {
    for (int f = first; f < first + count; f += op->batch_patches) // :384-412
      PMG_TRY(launch_stiffness<P>(op, x, y, f, std::min(op->batch_patches, first + count - f), atomic_out, s));
    return PMG_OK;
  }
  const double2* G = op->G;
  if (op->batch_patches > 0 && op->geometry_mode == 0)
    G = batch_geometry(op, first, count, s); // :391-396
  apply_variant<P, (P >= NT_FROM)>(op, [&](auto geo, auto nt, const double* Gcell) { // (no stream: nt is for the y stores)
    constexpr int GEO = decltype(geo)::value;
    constexpr bool NT = decltype(nt)::value;
    stiffness_column_kernel<P, GEO, NT><<<count, Shape<P>::WTHREADS, 0, s>>>(
        x, y, G, Gcell, op->W1, op->poff, op->pdofs, op->lmap_id, op->lmaps, op->pcell, op->pncell, op->kappa, op->D,
        op->react, first, atomic_out);
  });
  op->launches++;
  return PMG_OK;
}

// the chains [first, first + count) of one chain colour (stiffness_chain_kernel)
static int launch_chains(pmg_laplacian op, const double* x, double* y, int first, int count, hipStream_t s)
{
  if constexpr (chain_form(4))
  {
    if (op->P != 4)
      return fail(PMG_ERR_INVALID, "internal: chain form at degree %d", op->P);
    auto launch = [&](auto nt) {
      stiffness_chain_kernel<4, decltype(nt)::value><<<count, ChainShape<4>::THREADS, 0, s>>>(
          x, y, op->G, op->poff, op->cdofs, op->ccar, op->lmap_id, op->lmaps, op->pcell, op->pncell, op->kappa, op->D,
          op->chain_off, op->chain_patch, first);
    };
    op->stream_policy ? launch(std::true_type{}) : launch(std::false_type{});
    op->launches++;
  }
  return PMG_OK;
}

// The form of an application, from everything in the operator's state that bears on it.  Two streams need the resident
// tensor.  Chains need it too, in the stored (not the affine) mode, and no reaction term: the chain kernel's carried
// dofs have no first patch to start from, and the form is opt-in and measured slower.
ApplyForm apply_form(pmg_laplacian op)
{
  const bool resident = op->batch_patches == 0;
  return {resident && !op->launch_stream.empty(),
          resident && op->chain_on && op->geometry_mode == 0 && !op->react, resident};
}

// launches [l0, l1) of the plan, in stream order
int run_launches(pmg_laplacian op, const double* x, double* y, int l0, int l1, hipStream_t s)
{
  return walk_launches(op, l0, l1, apply_form(op), s, [&](const LaunchStep& st, hipStream_t sl) {
    if (st.kind == LaunchStep::CHAINS)
      return launch_chains(op, x, y, st.first, st.count, sl);
    return with_degree(op->P, [&](auto P) {
      return launch_stiffness<decltype(P)::value>(op, x, y, st.first, st.count, st.atomic_out, sl);
    });
  });
}

// (fine degree, coarse degree) pairs stiffness_restrict_kernel is instantiated for
#define PMG_FOR_FUSED_PAIRS(X) X(2, 1) X(4, 2) X(3, 1) X(6, 3)

// all patches of the operator in one launch of the fused kernel (cache policy and affine mode as launch_stiffness)
template <int P, int PC>
int launch_stiffness_restrict(pmg_laplacian op, const TransferView& tv, const double* z, const double* r,
                              double* coarse, hipStream_t s)
{
  constexpr int cm = RestrictShape<P, PC>::CM;
  PMG_REQUIRE(tv.cmax_m <= cm, "internal: a patch holds %d coarse dofs, the fused kernel %d", tv.cmax_m, cm);
  const RestrictLists R{tv.cpoff, tv.clmap_id, tv.cpdofs, tv.clmaps, tv.pmult, tv.M1};
  apply_variant<P, false>(op, [&](auto geo, auto nt, const double* Gcell) {
    constexpr int GEO = decltype(geo)::value;
    constexpr bool NT = decltype(nt)::value;
    stiffness_restrict_kernel<P, PC, GEO, NT><<<op->npatch, Shape<P>::WTHREADS, 0, s>>>(
        z, r, coarse, op->G, Gcell, op->W1, op->poff, op->pdofs, op->lmap_id, op->lmaps, op->pcell, op->pncell,
        op->kappa, op->D, op->react, R);
  });
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}

} // namespace

namespace pmg
{
// tensor bytes above which the stream is non-temporal.  The Infinity Cache holds 256 MiB, but inside a V-cycle the
// smoother's vectors pass through it between two applications: measured per cycle, default / nt policy, at 24^3
// cells (83 MB) 0.417 / 0.445 ms, 32^3 (196 MB) 0.821 / 0.809, 40^3 1.59 / 1.46, 64^3 5.71 / 5.10.
// PMG_STREAM_POLICY=0 / 1 forces the default / the streaming policy (measurements).
bool streams_past_the_cache(long long tensor_bytes)
{
  if (const char* e = std::getenv("PMG_STREAM_POLICY"))
    return e[0] != '0';
  return tensor_bytes > (128LL << 20);
}

// Is the fused apply-and-restrict available on this operator towards degree `coarse_degree`?  (pmg_amd.h,
// pmg_interpolator_restrict_residual: no ghosts, resident geometry, an instantiated pair -- which leaves out the
// shared-item degrees 5 and 8)
bool laplacian_fuses_restriction(pmg_laplacian op, int coarse_degree)
{
  if (op->layout->num_ghosts != 0 || op->batch_patches != 0)
    return false;
#define X(F, C)                                                                                                      \
  if (op->P == F && coarse_degree == C)                                                                              \
    return true;
  PMG_FOR_FUSED_PAIRS(X)
#undef X
  return false;
}

// coarse = P^T (r - A z) without A z ever reaching memory: the coarse vector is zero-filled, then ALL patches of the
// operator run in one launch (no colour order: nothing is written to a fine vector).  Counts as one application
// (pmg_multigrid_apply_counts); it is not part of the stiffness profile, which keeps describing the plain kernel.
int laplacian_apply_restrict(pmg_laplacian op, const TransferView& tv, const double* z, const double* r,
                             double* coarse, hipStream_t s)
{
  PMG_REQUIRE(laplacian_fuses_restriction(op, tv.ndc - 1) && tv.ndf == op->nd && tv.fv.pdofs == op->pdofs
                  && tv.fv.npatch == op->npatch && tv.lf == op->layout,
              "laplacian_apply_restrict: not available for this operator and transfer");
  launch_zero(tv.lc->total(), coarse, s);
  if (op->npatch > 0)
  {
#define X(F, C)                                                                                                      \
  if (op->P == F && tv.ndc - 1 == C)                                                                                 \
    PMG_TRY((launch_stiffness_restrict<F, C>(op, tv, z, r, coarse, s)));
    PMG_FOR_FUSED_PAIRS(X)
#undef X
    op->launches++;
  }
  op->applies++;
  return PMG_OK;
}

const double* laplacian_diag_inv(pmg_laplacian op) { return op->diag_inv; }
// matrix.hip, amg.hip: the reaction and Robin components summed (rebuild_diagonal_term); nullptr = none
const double* laplacian_reaction(pmg_laplacian op) { return op->react; }
pmg_layout laplacian_layout(pmg_laplacian op) { return op->layout; }
long long laplacian_launches(pmg_laplacian op) { return op->applies; }
LaplacianInputs laplacian_inputs(pmg_laplacian op) { return {op->P, op->ncells, op->dofmap, op->bc, op->kappa}; }

// what a captured graph of launches of this operator depends on; -1 = not capturable right now
long long laplacian_capture_state(pmg_laplacian op)
{
  if (op->profiling)
    return -1;
  // (diagonal term, reaction or Robin: the first component set and the last one removed change a kernel argument of
  // every apply launch, and which launches an operator in chain form issues; a later set of either, and the second
  // component beside the first, rewrite the vector in place)
  // (batched geometry: the captured geometry launches carry the field's and the coefficient tensor's addresses -- one
  // epoch counts both; the resident tensor is rebuilt in place, as everything else that follows the operator's data
  // (laplacian_data_changed states what follows what), so a graph over it stays valid)
  const long long field = op->batch_patches > 0 ? (op->kfield_epoch & 0x3fff) << 44 : 0;
  // (recomputed tensor: another kernel, reading another array; its column-constant branch: a value the kernels read, and
  // keyed all the same, so that a graph is captured under the setting it replays)
  return ((long long)op->geometry_mode << 40) ^ ((long long)op->batch_patches << 8) ^ (long long)(op->have_diag ? 1 : 0)
         ^ (long long)(op->chain_on ? 2 : 0) ^ (long long)(op->react ? 4 : 0) ^ (long long)(recomputes_tensor(op) ? 8 : 0)
         ^ (long long)(hoists_column_tensor(op) ? 16 : 0) ^ field;
}

PatchView laplacian_patches(pmg_laplacian op)
{
  PatchView v;
  v.P = op->P;
  v.K = op->K;
  v.N = op->N;
  v.npatch = op->npatch;
  v.max_m = op->max_m;
  v.pcell_h = &op->pcell_h;
  v.pncell_h = &op->pncell_h;
  v.launch_first = &op->launch_first;
  v.launch_count = &op->launch_count;
  v.n_launch_l = op->n_launch_l;
  v.merged = op->n_plain == 0;
  v.pcell = op->pcell;
  v.pncell = op->pncell;
  v.poff = op->poff;
  v.pdofs = op->pdofs;
  v.lmap_id = op->lmap_id;
  v.lmaps = op->lmaps;
  v.npdofs = op->npdofs;
  return v;
}

// Does an application zero-fill its whole output first (every first writer adds with atomics: the merged launch of a
// small level)?  Then a caller that hands over an output that is zero already can skip the fill
// (laplacian_apply_zeroed; the smoother's vector kernels clear the vector behind themselves).
bool laplacian_wants_zeroed_output(pmg_laplacian op)
{
  return zero_fills_output(op->needs_zero, op->launch_first.size(), op->n_bzero, op->layout->total());
}

// Interior and boundary patches in ONE launch behind a whole exchange?  Only where both lists add with atomics
// anyway (the merged form of a small level) and the geometry is resident -- the two launches of the plan, walked whole,
// are then one step over all patches -- and the layout's exchange is one launch (halo windows).  The transfers of the
// level follow the operator (interpolate.hip).
bool laplacian_single_launch(pmg_laplacian op)
{
  if (op->launch_first.size() != 2)
    return false;
  int steps = 0, all = 0;
  for_each_launch_step(*op, op->chain_first, op->chain_count, 0, 2, apply_form(op), [&](const LaunchStep& st) {
    steps += st.launches();
    all += st.kind == LaunchStep::PATCHES && st.atomic_out && st.count == op->npatch;
    return PMG_OK;
  });
  return steps == 1 && all == 1 && layout_exchanges_whole(op->layout);
}

// operator()(in, out), src/laplacian.hpp:462-482 + impl_operator :373-460
static int apply_impl(pmg_laplacian op, double* in, double* out, bool out_is_zero, hipStream_t s,
                      bool exchange = true)
{
  pmg_layout l = op->layout;
  const int nl = (int)op->launch_first.size();
  // :466 -- but only where needed: dofs no patch touches, or (most of the vector) dofs whose
  // first writer adds with atomics; everything else is stored by its first writer
  const bool zero_all = laplacian_wants_zeroed_output(op);
  if (zero_all && !out_is_zero)
    launch_zero(l->total(), out, s);
  if (op->n_bzero > 0 && !zero_all)
    zero_list_kernel<<<(op->n_bzero + 255) / 256 > 1024 ? 1024 : (op->n_bzero + 255) / 256, 256, 0, s>>>(
        op->n_bzero, op->bzero, out);
  // A small level (every launch adds with atomics: the merged form) on a window layout: the exchange whole, in one
  // launch, then ALL patches in one launch -- two launches instead of four; there is nothing an interior launch of a
  // few microseconds could hide (laplacian_single_launch).
  if (laplacian_single_launch(op))
  {
    if (exchange)
      PMG_TRY(scatter_fwd_whole(l, in, s));
    PMG_TRY(run_launches(op, in, out, 0, nl, s));
    op->applies++;
    return PMG_OK;
  }
  if (exchange)
    PMG_TRY(pmg_scatter_fwd_begin(l, in, (pmg_stream)s));        // :378
  PMG_TRY(run_launches(op, in, out, 0, op->n_launch_l, s));      // :380-413 interior cells
  if (exchange)
    PMG_TRY(pmg_scatter_fwd_end(l, in, (pmg_stream)s));          // :425
  PMG_TRY(run_launches(op, in, out, op->n_launch_l, nl, s));     // :429-455 boundary cells
  op->applies++;
  return PMG_OK;
}
int laplacian_apply(pmg_laplacian op, double* in, double* out, hipStream_t s) { return apply_impl(op, in, out, false, s); }
// The ghost entries of `in` are current already (the caller's bookkeeping, solvers.hip local_correction): the same
// application without its halo exchange.
int laplacian_apply_ghosts_current(pmg_laplacian op, double* in, double* out, hipStream_t s)
{
  return apply_impl(op, in, out, false, s, false);
}
// `out` is zero over the whole layout already (only meaningful when laplacian_wants_zeroed_output)
int laplacian_apply_zeroed(pmg_laplacian op, double* in, double* out, hipStream_t s)
{
  return apply_impl(op, in, out, laplacian_wants_zeroed_output(op), s);
}
} // namespace pmg

// The one constructor: every pmg_laplacian_create_* ends here (the trilinear ones with geom_degree = 1)
extern "C" int pmg_laplacian_create_curved(
    pmg_laplacian* out, pmg_layout layout, int degree, int32_t ncells, const double* kappa,
    const int32_t* dofmap, const double* xgeom, int32_t npoints, int geom_degree, const int32_t* geom_dofmap,
    const double* dphi_geometry, const double* G_weights, const int32_t* lcells, int32_t n_lcells,
    const int32_t* bcells, int32_t n_bcells, const int8_t* bc_marker, int node_order, const int32_t* custom_perm1d,
    pmg_stream stream)
{
  PMG_REQUIRE(out, "pmg_laplacian_create: NULL handle");
  *out = nullptr;
  PMG_REQUIRE(layout, "pmg_laplacian_create: NULL handle");
  if (degree < 1 || degree > PMG_MAX_DEGREE)
    return fail(PMG_ERR_INVALID, "Unsupported degree"); // src/laplacian.hpp:346
  PMG_REQUIRE(geom_degree >= 1 && geom_degree <= PMG_MAX_GEOM_DEGREE,
              "pmg_laplacian_create: geometry degree %d outside 1..%d", geom_degree, PMG_MAX_GEOM_DEGREE);
  PMG_REQUIRE((dphi_geometry != nullptr) == (G_weights != nullptr) || geom_degree == 1,
              "pmg_laplacian_create: dphi_geometry and G_weights are both given or both NULL");
  const int g = geom_degree, gm = g + 1, ng = gm * gm * gm;
  PMG_REQUIRE(ncells >= 0 && n_lcells >= 0 && n_bcells >= 0 && n_lcells + n_bcells <= ncells,
              "pmg_laplacian_create: cell lists (%d + %d) exceed ncells (%d)", n_lcells, n_bcells,
              ncells);
  PMG_REQUIRE(ncells == 0 || (kappa && dofmap && xgeom && geom_dofmap && bc_marker),
              "pmg_laplacian_create: NULL array");
  PMG_REQUIRE((n_lcells == 0 || lcells) && (n_bcells == 0 || bcells),
              "pmg_laplacian_create: NULL cell list");
  PMG_REQUIRE(npoints >= 0, "pmg_laplacian_create: negative npoints");
  {
    std::vector<char> seen(ncells, 0);
    for (int set = 0; set < 2; ++set)
    {
      const int32_t* list = set ? bcells : lcells;
      const int n = set ? n_bcells : n_lcells;
      for (int i = 0; i < n; ++i)
      {
        PMG_REQUIRE(list[i] >= 0 && list[i] < ncells,
                    "pmg_laplacian_create: cell list entry %d out of range", list[i]);
        PMG_REQUIRE(!seen[list[i]], "pmg_laplacian_create: cell %d listed twice", list[i]);
        seen[list[i]] = 1;
      }
    }
  }

  hipStream_t s = S(stream);
  auto* op = new pmg_laplacian_s;
  HandleGuard<pmg_laplacian> guard(op, pmg_laplacian_destroy);
  op->layout = layout;
  op->P = degree;
  op->nd = degree + 1;
  op->N = op->nd * op->nd * op->nd;
  op->K = patch_shape(degree).K();
  {
    const int kk[9] = {0, Shape<1>::K, Shape<2>::K, Shape<3>::K, Shape<4>::K, Shape<5>::K,
                       Shape<6>::K, Shape<7>::K, Shape<8>::K};
    PMG_REQUIRE(kk[degree] == op->K, "internal: patch shape / kernel shape mismatch");
  }
  op->ncells = ncells;
  op->npoints = npoints;
  op->kappa = kappa;
  op->dofmap = dofmap;
  op->xgeom = xgeom;
  op->geom_dofmap = geom_dofmap;
  op->bc = bc_marker;
  const int nd = op->nd, N = op->N;
  const int total = layout->total();

  // cell-local node order: everything below (patch tables, diagonal, load vector, the transfers and the AMG that
  // read op->dofmap) works on an ascending dofmap; a caller in another order gets a permuted copy, made once
  std::vector<int32_t> perm1d;
  PMG_TRY(node_permutation(node_order, degree, custom_perm1d, perm1d));
  op->node_order = node_order;
  if (!is_identity(perm1d))
  {
    const std::vector<int32_t> p3 = cell_permutation(nd, perm1d);
    PMG_TRY(upload(&op->qperm, p3.data(), p3.size(), s));
    PMG_HIP(hipMalloc(&op->dofmap_own, sizeof(int32_t) * ((size_t)ncells * N ? (size_t)ncells * N : 1)));
    PMG_TRY(permute_rows_i32(ncells, N, op->qperm, dofmap, op->dofmap_own, s));
    PMG_HIP(hipStreamSynchronize(s)); // p3 goes out of scope
    op->dofmap = dofmap = op->dofmap_own;
  }

  // 1-D tables (basix's job in the reference, src/laplacian.hpp:302-317)
  std::vector<double> pts(nd), wts(nd), D(nd * nd);
  gll_table(nd, pts.data(), wts.data());
  lagrange_derivative_table(nd, pts.data(), D.data());
  PMG_TRY(upload(&op->D, D.data(), D.size(), s));

  // coordinate-element derivatives at the GLL points, [3][N][ng] (ng = 8: the trilinear element), and
  // the 3-D weights (examples/pmg/main.cpp:216-238)
  op->geom_degree = g;
  op->ng = ng;
  op->own_tables = !(dphi_geometry && G_weights);
  if (dphi_geometry && G_weights)
  {
    PMG_HIP(hipMalloc(&op->dphi_geom, sizeof(double) * 3 * ng * N));
    PMG_HIP(hipMalloc(&op->gweights, sizeof(double) * N));
    if (op->qperm) // the caller's tables are indexed by ITS quadrature-point numbers
    {
      PMG_TRY(permute_rows_f64(3, N, ng, op->qperm, dphi_geometry, op->dphi_geom, s));
      PMG_TRY(permute_rows_f64(1, N, 1, op->qperm, G_weights, op->gweights, s));
    }
    else
    {
      PMG_HIP(hipMemcpyAsync(op->dphi_geom, dphi_geometry, sizeof(double) * 3 * ng * N,
                             hipMemcpyDeviceToDevice, s));
      PMG_HIP(hipMemcpyAsync(op->gweights, G_weights, sizeof(double) * N, hipMemcpyDeviceToDevice, s));
    }
  }
  else
  {
    // the element's 1-D basis and derivative at the GLL points, L / Lp [nd][g + 1]; the dense table is their product
    std::vector<double> L((size_t)nd * gm), Lp((size_t)nd * gm), dphi((size_t)3 * ng * N), w3(N);
    coordinate_element_tables_1d(nd, pts.data(), g, L.data(), Lp.data());
    coordinate_element_table_3d(nd, gm, L.data(), Lp.data(), dphi.data());
    for (int a = 0; a < nd; ++a)
      for (int b = 0; b < nd; ++b)
        for (int c = 0; c < nd; ++c)
          w3[(a * nd + b) * nd + c] = wts[a] * wts[b] * wts[c];
    PMG_TRY(upload(&op->dphi_geom, dphi.data(), dphi.size(), s));
    PMG_TRY(upload(&op->gweights, w3.data(), w3.size(), s));
    if (g >= 2) // the cell-cooperative geometry kernel contracts with the 1-D tables (tensor_kernels.hpp)
    {
      PMG_REQUIRE(curved_lds_bytes(nd, gm) <= 64 * 1024, "internal: the curved geometry kernel needs %zu bytes of LDS",
                  curved_lds_bytes(nd, gm));
      PMG_TRY(upload(&op->geom_L, L.data(), L.size(), s));
      PMG_TRY(upload(&op->geom_Lp, Lp.data(), Lp.size(), s));
    }
    PMG_HIP(hipStreamSynchronize(s)); // host vectors go out of scope
  }

  // ---- patches (host): needs the dofmap, the Dirichlet marker and cell centroids ----
  PatchPlan plan;
  ChainPlan cplan;
  {
    std::vector<int32_t> h_dofmap((size_t)ncells * N), h_gd((size_t)ncells * ng);
    std::vector<int8_t> h_bc(total);
    std::vector<double> h_x((size_t)npoints * 3);
    PMG_HIP(hipMemcpyAsync(h_dofmap.data(), dofmap, sizeof(int32_t) * h_dofmap.size(),
                           hipMemcpyDeviceToHost, s));
    PMG_HIP(hipMemcpyAsync(h_gd.data(), geom_dofmap, sizeof(int32_t) * h_gd.size(),
                           hipMemcpyDeviceToHost, s));
    PMG_HIP(hipMemcpyAsync(h_bc.data(), bc_marker, sizeof(int8_t) * h_bc.size(),
                           hipMemcpyDeviceToHost, s));
    PMG_HIP(hipMemcpyAsync(h_x.data(), xgeom, sizeof(double) * h_x.size(), hipMemcpyDeviceToHost, s));
    PMG_HIP(hipStreamSynchronize(s));
    for (int32_t i = 0; i < layout->size_local; ++i)
      op->n_marked += h_bc[i] != 0;
    for (size_t i = 0; i < h_gd.size(); ++i) // all (g+1)^3 nodes of every cell
      PMG_REQUIRE(h_gd[i] >= 0 && h_gd[i] < npoints, "pmg_laplacian_create: geometry dofmap entry %d out of range",
                  h_gd[i]);
    // the 8 corner nodes of a cell, k = i*4 + j*2 + l, at their tensor positions among the (g+1)^3
    int corner[8];
    for (int k = 0; k < 8; ++k)
      corner[k] = (((k >> 2) & 1) * g * gm + ((k >> 1) & 1) * g) * gm + (k & 1) * g;
    std::vector<float> centroid((size_t)ncells * 3); // mean of the corners
    for (int32_t c = 0; c < ncells; ++c)
      for (int a = 0; a < 3; ++a)
      {
        double v = 0;
        for (int k = 0; k < 8; ++k)
          v += h_x[3 * (size_t)h_gd[(size_t)c * ng + corner[k]] + a];
        centroid[(size_t)c * 3 + a] = (float)(v * 0.125);
      }
    PMG_TRY(build_patch_plan(plan, degree, ncells, h_dofmap.data(), h_bc.data(), total,
                             centroid.data(), lcells, n_lcells, bcells, n_bcells));
    // affine (parallelepiped) cells: node (i,j,l) = x0 + xi_i e1 + xi_j e2 + xi_l e3 with the edges e1, e2, e3 from the
    // corner x0 and xi the element's 1-D nodes -- every one of the (g+1)^3 nodes, so a cell with parallelepiped corners
    // and a displaced mid-edge node is not affine
    std::vector<double> xi(gm), xiw(gm);
    gll_table(gm, xi.data(), xiw.data());
    op->all_affine = (n_lcells + n_bcells) > 0;
    for (int set = 0; set < 2 && op->all_affine; ++set)
    {
      const int32_t* list = set ? bcells : lcells;
      const int n = set ? n_bcells : n_lcells;
      for (int i = 0; i < n && op->all_affine; ++i)
      {
        const int32_t* gd = h_gd.data() + (size_t)list[i] * ng;
        const double* v[8];
        for (int k = 0; k < 8; ++k)
          v[k] = h_x.data() + 3 * (size_t)gd[corner[k]];
        double diam = 0, dev = 0;
        for (int a = 0; a < 3; ++a)
        {
          const double e1 = v[4][a] - v[0][a], e2 = v[2][a] - v[0][a], e3 = v[1][a] - v[0][a];
          diam += std::fabs(e1) + std::fabs(e2) + std::fabs(e3);
          if (g == 1)
            dev += std::fabs(v[3][a] - (v[0][a] + e2 + e3)) + std::fabs(v[5][a] - (v[0][a] + e1 + e3))
                   + std::fabs(v[6][a] - (v[0][a] + e1 + e2)) + std::fabs(v[7][a] - (v[0][a] + e1 + e2 + e3));
          else
            for (int ni = 0; ni < gm; ++ni)
              for (int nj = 0; nj < gm; ++nj)
                for (int nl = 0; nl < gm; ++nl)
                  dev += std::fabs(h_x[3 * (size_t)gd[(ni * gm + nj) * gm + nl] + a]
                                   - (v[0][a] + xi[ni] * e1 + xi[nj] * e2 + xi[nl] * e3));
        }
        if (dev > 1e-12 * diam)
          op->all_affine = false;
      }
    }
    // chain form of the interior launches (stiffness_chain_kernel).  PMG_CHAIN=0 never, =1 where a colour's chains
    // fill the GPU (one workgroup per chain and compute unit), =2 whenever chains exist (tests on small meshes).
    if (chain_form(degree) && (unsigned long long)plan.npatch * (unsigned long long)gpatch(nd, op->K) < (1ull << 32))
    {
      const char* e = std::getenv("PMG_CHAIN");
      const int mode = e ? std::atoi(e) : 0; // (not set: never)
      if (mode > 0)
      {
        int dev = 0, cus = 256;
        if (hipGetDevice(&dev) == hipSuccess)
          (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        PMG_TRY(build_chain_plan(cplan, plan, total, h_bc.data(), centroid.data(), mode >= 2 ? 1 : (cus * 3) / 4));
      }
    }
    // is every local dof written by some patch?  (else out must be zero-filled first)
    std::vector<char> touched(total, 0);
    for (uint32_t v : plan.pdofs)
      touched[v & PD_MASK] = 1;
    for (int i = 0; i < total && !op->needs_zero; ++i)
      op->needs_zero = !touched[i];
  }
  op->npatch = plan.npatch;
  op->pcell_h = plan.pcell;
  op->pncell_h = plan.pncell;
  op->npdofs = (long long)plan.pdofs.size();
  op->max_m = plan.max_M;
  op->launch_first = plan.launch_first;
  op->launch_count = plan.launch_count;
  op->n_launch_l = plan.n_launch_l;
  op->n_plain = plan.n_plain;
  op->launch_stream = plan.launch_stream;
  op->launch_signal = plan.launch_signal;
  op->launch_wait = plan.launch_wait;
  if (!op->launch_stream.empty())
  {
    PMG_HIP(hipStreamCreateWithFlags(&op->stream2, hipStreamNonBlocking));
    PMG_HIP(hipEventCreateWithFlags(&op->ev_fork, hipEventDisableTiming));
    PMG_HIP(hipEventCreateWithFlags(&op->ev_order, hipEventDisableTiming));
    PMG_HIP(hipEventCreateWithFlags(&op->ev_join, hipEventDisableTiming));
  }
  PMG_TRY(upload(&op->pcell, plan.pcell.data(), plan.pcell.size(), s));
  PMG_TRY(upload(&op->pncell, plan.pncell.data(), plan.pncell.size(), s));
  op->listed.assign(ncells, 0);
  for (int32_t c : op->pcell_h)
    if (c >= 0)
      op->listed[c] = 1;
  PMG_TRY(upload(reinterpret_cast<char**>(&op->cell_listed), op->listed.data(), op->listed.size(), s));
  op->n_bzero = (int32_t)plan.bzero.size();
  PMG_TRY(upload(&op->bzero, plan.bzero.data(), plan.bzero.size(), s));
  PMG_TRY(upload(&op->poff, plan.poff.data(), plan.poff.size(), s));
  PMG_TRY(upload(&op->pdofs, plan.pdofs.data(), plan.pdofs.size(), s));
  PMG_TRY(upload(&op->lmap_id, plan.lmap_id.data(), plan.lmap_id.size(), s));
  PMG_TRY(upload(&op->lmaps, plan.lmaps.data(), plan.lmaps.size(), s));
  if (cplan.ok)
  {
    PMG_TRY(upload(&op->cdofs, cplan.cdofs.data(), cplan.cdofs.size(), s));
    PMG_TRY(upload(&op->ccar, cplan.ccar.data(), cplan.ccar.size(), s));
    PMG_TRY(upload(&op->chain_off, cplan.chain_off.data(), cplan.chain_off.size(), s));
    PMG_TRY(upload(&op->chain_patch, cplan.chain_patch.data(), cplan.chain_patch.size(), s));
    op->chain_first = cplan.launch_first;
    op->chain_count = cplan.launch_count;
    op->chain_ok = op->chain_on = true;
  }

  const long long nslots = (long long)plan.npatch * op->K;
  {
    std::vector<double> w1(wts);
    w1.insert(w1.end(), pts.begin(), pts.end());
    // ... and the switch of the column-constant branch; PMG_COLUMN_TENSOR=0 / 1 sets it (measurements)
    if (const char* e = std::getenv("PMG_COLUMN_TENSOR"))
      op->column_tensor_request = e[0] != '0' ? 1 : 0;
    w1.push_back(op->column_tensor_request != 0 ? 1.0 : 0.0);
    PMG_TRY(upload(&op->W1, w1.data(), w1.size(), s));
    PMG_HIP(hipStreamSynchronize(s)); // w1 goes out of scope
  }
  // PMG_TENSOR_RECOMPUTE=0 / 1 forces the streamed / (where eligible) the recomputed form (measurements)
  if (const char* e = std::getenv("PMG_TENSOR_RECOMPUTE"))
    op->recompute_request = e[0] != '0' ? 1 : 0;
  // ... and PMG_TENSOR_RECOMPUTE_IDENTITY=0 / 1 the same for the degree-4 form, which listens to this one alone
  if (const char* e = std::getenv("PMG_TENSOR_RECOMPUTE_IDENTITY"))
    op->recompute_identity_request = e[0] != '0' ? 1 : 0;
  PMG_TRY(ensure_cell_coefficients(op, s));
  PMG_HIP(hipMalloc(&op->Gaff, sizeof(double) * 6 * (nslots ? nslots : 1)));
  PMG_TRY(rebuild_affine_tensor(op, s));
  {
    const size_t gsize = (size_t)op->npatch * gpatch(nd, op->K);
    PMG_HIP(hipMalloc(&op->G, sizeof(double2) * (gsize ? gsize : 1)));
    PMG_HIP(hipMemsetAsync(op->G, 0, sizeof(double2) * (gsize ? gsize : 1), s)); // padding, empty slots
  }
  op->stream_policy = streams_past_the_cache((long long)sizeof(double2) * gpatch(nd, op->K) * op->npatch);
  PMG_HIP(hipMalloc(&op->diag_inv, sizeof(double) * (total ? total : 1)));
  PMG_HIP(hipEventCreate(&op->ev0));
  PMG_HIP(hipEventCreate(&op->ev1));
  PMG_TRY(rebuild_resident_tensor(op, s));
  PMG_HIP(hipStreamSynchronize(s)); // plan's host vectors are released on return
  *out = guard.release();
  return PMG_OK;
}

extern "C" int pmg_laplacian_create_ordered(
    pmg_laplacian* out, pmg_layout layout, int degree, int32_t ncells, const double* kappa,
    const int32_t* dofmap, const double* xgeom, int32_t npoints, const int32_t* geom_dofmap,
    const double* dphi_geometry, const double* G_weights, const int32_t* lcells, int32_t n_lcells,
    const int32_t* bcells, int32_t n_bcells, const int8_t* bc_marker, int node_order, const int32_t* custom_perm1d,
    pmg_stream stream)
{
  return pmg_laplacian_create_curved(out, layout, degree, ncells, kappa, dofmap, xgeom, npoints, 1, geom_dofmap,
                                     dphi_geometry, G_weights, lcells, n_lcells, bcells, n_bcells, bc_marker,
                                     node_order, custom_perm1d, stream);
}

extern "C" int pmg_laplacian_geometry_degree(pmg_laplacian op) { return op ? op->geom_degree : -1; }

extern "C" int pmg_laplacian_create_with_tables(
    pmg_laplacian* out, pmg_layout layout, int degree, int32_t ncells, const double* kappa,
    const int32_t* dofmap, const double* xgeom, int32_t npoints, const int32_t* geom_dofmap,
    const double* dphi_geometry, const double* G_weights, const int32_t* lcells, int32_t n_lcells,
    const int32_t* bcells, int32_t n_bcells, const int8_t* bc_marker, pmg_stream stream)
{
  return pmg_laplacian_create_ordered(out, layout, degree, ncells, kappa, dofmap, xgeom, npoints, geom_dofmap,
                                      dphi_geometry, G_weights, lcells, n_lcells, bcells, n_bcells, bc_marker,
                                      PMG_NODES_ASCENDING, nullptr, stream);
}

extern "C" int pmg_laplacian_node_order(pmg_laplacian op) { return op ? op->node_order : -1; }

extern "C" int pmg_laplacian_create(pmg_laplacian* out, pmg_layout layout, int degree,
                                    int32_t ncells, const double* kappa, const int32_t* dofmap,
                                    const double* xgeom, int32_t npoints,
                                    const int32_t* geom_dofmap, const int32_t* lcells,
                                    int32_t n_lcells, const int32_t* bcells, int32_t n_bcells,
                                    const int8_t* bc_marker, pmg_stream stream)
{
  return pmg_laplacian_create_with_tables(out, layout, degree, ncells, kappa, dofmap, xgeom,
                                          npoints, geom_dofmap, nullptr, nullptr, lcells, n_lcells,
                                          bcells, n_bcells, bc_marker, stream);
}

extern "C" int pmg_laplacian_destroy(pmg_laplacian op)
{
  if (!op)
    return PMG_OK;
  (void)hipFree(op->G);
  (void)hipFree(op->dofmap_own);
  (void)hipFree(op->qperm);
  (void)hipFree(op->D);
  (void)hipFree(op->Gaff);
  (void)hipFree(op->Ccell);
  (void)hipFree(op->kfield);
  (void)hipFree(op->ktensor);
  (void)hipFree(op->react_buf);
  (void)hipFree(op->sigma_buf);
  (void)hipFree(op->robin_buf);
  (void)hipFree(op->react32_buf);
  (void)hipFree(op->W1);
  (void)hipFree(op->dphi_geom);
  (void)hipFree(op->geom_L);
  (void)hipFree(op->geom_Lp);
  (void)hipFree(op->gweights);
  (void)hipFree(op->pcell);
  (void)hipFree(op->pncell);
  (void)hipFree(op->bzero);
  (void)hipFree(op->poff);
  (void)hipFree(op->pdofs);
  (void)hipFree(op->lmap_id);
  (void)hipFree(op->lmaps);
  (void)hipFree(op->cdofs);
  (void)hipFree(op->ccar);
  (void)hipFree(op->chain_off);
  (void)hipFree(op->chain_patch);
  (void)hipFree(op->diag_inv);
  (void)hipFree(op->G32);
  (void)hipFree(op->D32);
  (void)hipFree(op->diag32);
  (void)hipFree(op->lift_cells);
  (void)hipFree(op->cell_listed);
  for (hipEvent_t e : op->prof_events)
    (void)hipEventDestroy(e);
  for (hipEvent_t e : {op->ev_fork, op->ev_order, op->ev_join})
    if (e)
      (void)hipEventDestroy(e);
  if (op->stream2)
    (void)hipStreamDestroy(op->stream2);
  if (op->ev0)
    (void)hipEventDestroy(op->ev0);
  if (op->ev1)
    (void)hipEventDestroy(op->ev1);
  delete op;
  return PMG_OK;
}

#ifdef PMG_STAMPS
// diagnostic builds only (tools/stamp_apply.py); not part of the ABI
extern "C" int pmg_debug_set_stamp_buffer(unsigned long long* buffer, int workgroups)
{
  PMG_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_buffer), &buffer, sizeof(buffer)));
  PMG_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_capacity), &workgroups, sizeof(workgroups)));
  return PMG_OK;
}
#endif

extern "C" int pmg_laplacian_degree(pmg_laplacian op) { return op ? op->P : -1; }

extern "C" int pmg_laplacian_is_affine(pmg_laplacian op) { return op ? (op->all_affine ? 1 : 0) : -1; }

extern "C" int pmg_laplacian_set_geometry_mode(pmg_laplacian op, int mode)
{
  PMG_REQUIRE(op && (mode == 0 || mode == 1), "pmg_laplacian_set_geometry_mode: bad argument");
  if (mode == 1)
  {
    PMG_REQUIRE(op->all_affine, "pmg_laplacian_set_geometry_mode: the mesh has non-affine cells");
    PMG_REQUIRE(!op->kfield, "pmg_laplacian_set_geometry_mode: the affine mode streams one tensor per cell and cannot "
                             "carry the coefficient field (remove it with pmg_laplacian_set_coefficient_field(op, "
                             "NULL, stream) first)");
  }
  op->geometry_mode = mode;
  return PMG_OK;
}

// The two switches of the recomputed tensor: pmg_laplacian_set_tensor_recompute for the degrees of recompute_form,
// pmg_laplacian_set_tensor_recompute_identity for those of recompute_identity_form.  Neither moves the other.
static int set_recompute_request(pmg_laplacian op, int mode, bool identity, const char* who)
{
  PMG_REQUIRE(op && mode >= -1 && mode <= 1, "%s: bad argument", who);
  hipStream_t s = nullptr; // (the first choice of the form builds the cell coefficients: not inside a stream capture)
  int& request = identity ? op->recompute_identity_request : op->recompute_request;
  const int before = request;
  request = mode;
  if (mode == 1)
  {
    const bool form = identity ? recompute_identity_form(op->P) : recompute_form(op->P);
    const char* why = op->geom_degree != 1           ? "the coordinate element is not trilinear"
                      : !op->own_tables              ? "the operator was created with the caller's tables"
                      : !form                        ? (identity ? "the form with the transposes by identity exists at "
                                                                   "degree 4 only"
                                                                 : "the form exists at degrees 1 and 2 only")
                      : op->batch_patches != 0       ? "the geometry is batched"
                      : op->geometry_mode != 0       ? "the operator is in the affine mode"
                      : op->kfield                   ? "a nodal coefficient field is set"
                      : op->ktensor                  ? "a per-cell coefficient tensor is set"
                      : op->chain_on                 ? "the operator is in the chain form"
                                                     : nullptr;
    if (why)
    {
      request = before;
      return fail(PMG_ERR_INVALID, "%s: this operator cannot recompute its tensor: %s", who, why);
    }
  }
  PMG_TRY(ensure_cell_coefficients(op, s));
  PMG_HIP(hipStreamSynchronize(s));
  return PMG_OK;
}

extern "C" int pmg_laplacian_set_tensor_recompute(pmg_laplacian op, int mode)
{
  return set_recompute_request(op, mode, false, "pmg_laplacian_set_tensor_recompute");
}

extern "C" int pmg_laplacian_tensor_recomputed(pmg_laplacian op)
{
  return op ? (recompute_form(op->P) && recomputes_tensor(op) ? 1 : 0) : -1;
}

extern "C" int pmg_laplacian_set_tensor_recompute_identity(pmg_laplacian op, int mode)
{
  return set_recompute_request(op, mode, true, "pmg_laplacian_set_tensor_recompute_identity");
}

extern "C" int pmg_laplacian_tensor_recomputed_identity(pmg_laplacian op)
{
  return op ? (recompute_identity_form(op->P) && recomputes_tensor(op) ? 1 : 0) : -1;
}

// The column-constant branch of the recomputed form.  The request stands while the operator's state moves: whether an
// application takes the branch is decided where the form is (hoists_column_tensor).
extern "C" int pmg_laplacian_set_column_tensor(pmg_laplacian op, int mode)
{
  PMG_REQUIRE(op && mode >= -1 && mode <= 1, "pmg_laplacian_set_column_tensor: bad argument");
  if (mode == 1 && recomputes_tensor(op) && !column_branch(op->P))
    return fail(PMG_ERR_INVALID, "pmg_laplacian_set_column_tensor: the recomputed form of degree %d has no "
                                 "column-constant branch (degrees 2 and 4 have it)", op->P);
  if (mode == 1 && !recomputes_tensor(op))
    return fail(PMG_ERR_INVALID, "pmg_laplacian_set_column_tensor: the column-constant tensor is a branch of the "
                                 "recomputed form, and this operator's apply does not recompute its tensor "
                                 "(pmg_laplacian_set_tensor_recompute, pmg_laplacian_set_tensor_recompute_identity)");
  const int before = op->column_tensor_request;
  op->column_tensor_request = mode;
  if ((before != 0) != (mode != 0))
    PMG_TRY(store_column_switch(op));
  return PMG_OK;
}

extern "C" int pmg_laplacian_column_tensor(pmg_laplacian op) { return op ? (hoists_column_tensor(op) ? 1 : 0) : -1; }

extern "C" int pmg_laplacian_column_tensor_items(pmg_laplacian op, long long* qualifying, long long* total,
                                                 pmg_stream stream)
{
  PMG_REQUIRE(op && qualifying && total, "pmg_laplacian_column_tensor_items: NULL argument");
  PMG_REQUIRE(recompute_possible(op) && column_branch(op->P) && op->Ccell,
              "pmg_laplacian_column_tensor_items: the operator has no recomputed form with the column-constant branch, "
              "or has not chosen the form yet");
  hipStream_t s = S(stream);
  PMG_TRY(not_capturing(s, "pmg_laplacian_column_tensor_items: allocates and reads back, not inside a stream capture"));
  unsigned long long* count = nullptr;
  unsigned long long host[2] = {0, 0};
  PMG_HIP(hipMalloc(&count, sizeof(host)));
  int err = PMG_OK;
  if (hipMemsetAsync(count, 0, sizeof(host), s) != hipSuccess)
    err = fail(PMG_ERR_HIP, "pmg_laplacian_column_tensor_items: hipMemsetAsync failed");
  if (err == PMG_OK && op->npatch > 0)
    err = with_degree(op->P, [&](auto P) {
      constexpr int p = decltype(P)::value;
      if constexpr (recompute_kernel(p) && column_branch(p))
        column_items_kernel<p><<<(unsigned)op->npatch * Shape<p>::ITEMS, 64, 0, s>>>(op->Ccell, op->W1, op->pncell, count);
      return PMG_OK;
    });
  if (err == PMG_OK
      && (hipGetLastError() != hipSuccess
          || hipMemcpyAsync(host, count, sizeof(host), hipMemcpyDeviceToHost, s) != hipSuccess
          || hipStreamSynchronize(s) != hipSuccess))
    err = fail(PMG_ERR_HIP, "pmg_laplacian_column_tensor_items: the count failed");
  (void)hipFree(count);
  PMG_TRY(err);
  *qualifying = (long long)host[0];
  *total = (long long)host[1];
  return PMG_OK;
}

extern "C" int pmg_laplacian_apply(pmg_laplacian op, double* in, double* out, pmg_stream stream)
{
  PMG_REQUIRE(op && in && out, "pmg_laplacian_apply: NULL argument");
  PMG_REQUIRE(in != out, "pmg_laplacian_apply: in and out alias");
  return laplacian_apply(op, in, out, S(stream));
}

extern "C" int pmg_laplacian_get_diag_inverse(pmg_laplacian op, double* diag_inv,
                                              pmg_stream stream)
{
  PMG_REQUIRE(op && diag_inv, "pmg_laplacian_get_diag_inverse: NULL argument");
  PMG_REQUIRE(op->have_diag, "pmg_laplacian_get_diag_inverse: diagonal not set");
  PMG_HIP(hipMemcpyAsync(diag_inv, op->diag_inv, sizeof(double) * op->layout->total(),
                         hipMemcpyDeviceToDevice, S(stream)));
  return PMG_OK;
}

extern "C" int pmg_laplacian_set_diag_inverse(pmg_laplacian op, const double* diag_inv,
                                              pmg_stream stream)
{
  PMG_REQUIRE(op && diag_inv, "pmg_laplacian_set_diag_inverse: NULL argument");
  PMG_HIP(hipMemcpyAsync(op->diag_inv, diag_inv, sizeof(double) * op->layout->total(),
                         hipMemcpyDeviceToDevice, S(stream)));
  op->have_diag = true;
  op->diag_computed = false;
  op->diag_version++;
  return PMG_OK;
}

extern "C" int pmg_laplacian_compute_diag_inverse(pmg_laplacian op, pmg_stream stream)
{
  PMG_REQUIRE(op, "pmg_laplacian_compute_diag_inverse: NULL argument");
  hipStream_t s = S(stream);
  const int total = op->layout->total();
  PMG_HIP(hipMemsetAsync(op->diag_inv, 0, sizeof(double) * total, s));
  PMG_TRY(for_each_geometry_chunk(op, s, [&](int first, int count, const double2* G) {
    const long long nslots = (long long)count * op->K, n = nslots * op->N;
    diagonal_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>((long long)first * op->K, nslots, op->nd, op->K,
                                                              op->pcell, G, op->dofmap, op->bc, op->kappa, op->D,
                                                              op->diag_inv);
  }));
  if (total > 0)
    diag_invert_kernel<<<(total + 255) / 256, 256, 0, s>>>(total, op->bc, op->react, op->diag_inv);
  PMG_HIP(hipGetLastError());
  op->have_diag = true;
  op->diag_computed = true;
  op->diag_version++;
  return PMG_OK;
}

// react = d_sigma + d_R, in that order (both components present)
__global__ void diagonal_term_sum_kernel(int n, const double* __restrict__ a, const double* __restrict__ b,
                                         double* __restrict__ out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    out[i] = a[i] + b[i];
}

// The one vector the kernels read, from its components (d_sigma in sigma_buf, d_R in robin_buf): an exact copy of the
// only component present, or d_sigma + d_R, always in react_buf, so a second set or a second component rewrites it at
// the address a captured graph read it from; nullptr when neither is present.  apply_form,
// pmg_laplacian_launches_per_apply and laplacian_capture_state read `react` itself.
static int rebuild_diagonal_term(pmg_laplacian op, hipStream_t s)
{
  const int total = op->layout->total();
  const size_t bytes = sizeof(double) * (total ? total : 1);
  if (!op->has_sigma && !op->has_robin)
  {
    op->react = nullptr; // (the allocations stay with the handle: laplacian.hpp)
    op->react32 = nullptr;
    return PMG_OK;
  }
  if (!op->react_buf)
    PMG_HIP(hipMalloc(&op->react_buf, bytes));
  op->react = op->react_buf;
  if (op->has_sigma && op->has_robin)
  {
    if (total > 0)
      diagonal_term_sum_kernel<<<(total + 255) / 256, 256, 0, s>>>(total, op->sigma_buf, op->robin_buf, op->react);
    PMG_HIP(hipGetLastError());
  }
  else
    PMG_HIP(hipMemcpyAsync(op->react, op->has_sigma ? op->sigma_buf : op->robin_buf, bytes, hipMemcpyDeviceToDevice,
                           s));
  return PMG_OK;
}

namespace pmg
{
// What the operator derives from its data, and from which of it -- the statement of the dependencies, which the setters
// and laplacian_capture_state rely on:
//
//   G         follows the geometry, the nodal field and the per-cell tensor; only while resident (in batched-geometry
//             mode every application recomputes its batches from the same three)
//   Gaff      follows the geometry and the tensor (the affine mode refuses a field)
//   G32       follows what G follows, once it exists (the first FP32 use builds it)
//   react     follows sigma_buf and robin_buf, the two components of the diagonal term
//   react32   follows react, while G32 exists
//   diag_inv  follows G, react and kappa, once pmg_laplacian_compute_diag_inverse has computed it (a diagonal the
//             caller set is the caller's)
//   diag32    follows diag_inv, lazily, by version (laplacian_f32_diag)
//
// `changed` names the data that was set or removed (OperatorData).  Everything that follows it is rebuilt here, in this
// order, each in its own buffer -- so a captured graph of this operator's launches stays valid; what changes a kernel
// argument or the launch list instead is in laplacian_capture_state.  Then waits for the stream: the setter's caller may
// free its array on return.
int laplacian_data_changed(pmg_laplacian op, unsigned changed, hipStream_t s)
{
  const bool tensors = (changed & (DATA_FIELD | DATA_TENSOR)) != 0;
  if (tensors)
    PMG_TRY(rebuild_resident_tensor(op, s));
  if (changed & DATA_TENSOR)
    PMG_TRY(rebuild_affine_tensor(op, s));
  if (tensors)
    PMG_TRY(laplacian_f32_refresh(op, s));
  if (changed & DATA_DIAGONAL_TERM)
  {
    PMG_TRY(rebuild_diagonal_term(op, s));
    PMG_TRY(laplacian_f32_reaction(op, s));
  }
  if (op->have_diag && op->diag_computed)
    PMG_TRY(pmg_laplacian_compute_diag_inverse(op, (pmg_stream)s));
  PMG_HIP(hipStreamSynchronize(s));
  return PMG_OK;
}
} // namespace pmg

extern "C" int pmg_laplacian_has_coefficient_field(pmg_laplacian op) { return op ? (op->kfield ? 1 : 0) : -1; }

extern "C" int pmg_laplacian_set_coefficient_field(pmg_laplacian op, const double* kq, pmg_stream stream)
{
  PMG_REQUIRE(op, "pmg_laplacian_set_coefficient_field: NULL argument");
  hipStream_t s = S(stream);
  PMG_TRY(not_capturing(
      s, "pmg_laplacian_set_coefficient_field: not inside a stream capture (it allocates and synchronises)"));
  pmg_layout l = op->layout;
  double* released = nullptr;
  if (!kq)
  {
    if (!op->kfield)
      return PMG_OK;
    released = op->kfield;
    op->kfield = nullptr;
    op->kfield_epoch++;
  }
  else
  {
    PMG_REQUIRE(op->geometry_mode == 0,
                "pmg_laplacian_set_coefficient_field: the affine mode streams one tensor per cell and cannot carry a "
                "field (return to the stored tensor with pmg_laplacian_set_geometry_mode(op, 0) first)");
    PMG_TRY(require_valid(
        l, l->size_local, kq, FinitePositive{},
        "pmg_laplacian_set_coefficient_field: %lld entries of the field are not finite and greater than 0", s));
    if (!op->kfield)
    {
      PMG_HIP(hipMalloc(&op->kfield, sizeof(double) * (l->total() ? l->total() : 1)));
      op->kfield_epoch++;
    }
    PMG_HIP(hipMemcpyAsync(op->kfield, kq, sizeof(double) * l->size_local, hipMemcpyDeviceToDevice, s));
    if (l->num_ghosts > 0)
    {
      PMG_HIP(hipMemsetAsync(op->kfield + l->size_local, 0, sizeof(double) * l->num_ghosts, s));
      PMG_TRY(scatter_fwd_whole(l, op->kfield, s));
    }
  }
  PMG_TRY(laplacian_data_changed(op, DATA_FIELD, s)); // (it waits for the stream: the caller may free kq on return)
  if (released)
    PMG_HIP(hipFree(released));
  return PMG_OK;
}

extern "C" int pmg_laplacian_has_coefficient_tensor(pmg_laplacian op) { return op ? (op->ktensor ? 1 : 0) : -1; }

extern "C" int pmg_laplacian_set_coefficient_tensor(pmg_laplacian op, const double* kt, pmg_stream stream)
{
  PMG_REQUIRE(op, "pmg_laplacian_set_coefficient_tensor: NULL argument");
  hipStream_t s = S(stream);
  PMG_TRY(not_capturing(
      s, "pmg_laplacian_set_coefficient_tensor: not inside a stream capture (it allocates and synchronises)"));
  double* released = nullptr;
  if (!kt)
  {
    if (!op->ktensor)
      return PMG_OK;
    released = op->ktensor;
    op->ktensor = nullptr;
    op->kfield_epoch++;
  }
  else
  {
    // (a cell that is a ghost elsewhere is counted on each rank that holds it)
    PMG_TRY(require_valid(
        op->layout, op->ncells, kt, FiniteSpd{},
        "pmg_laplacian_set_coefficient_tensor: %lld cells have a tensor that is not finite and positive definite", s));
    if (!op->ktensor)
    {
      PMG_HIP(hipMalloc(&op->ktensor, sizeof(double) * 6 * (size_t)(op->ncells ? op->ncells : 1)));
      op->kfield_epoch++;
    }
    PMG_HIP(hipMemcpyAsync(op->ktensor, kt, sizeof(double) * 6 * (size_t)op->ncells, hipMemcpyDeviceToDevice, s));
  }
  PMG_TRY(laplacian_data_changed(op, DATA_TENSOR, s)); // (it waits for the stream: the caller may free kt on return)
  if (released)
    PMG_HIP(hipFree(released));
  return PMG_OK;
}

extern "C" int pmg_laplacian_has_reaction(pmg_laplacian op) { return op ? (op->has_sigma ? 1 : 0) : -1; }

namespace pmg
{
int laplacian_require_singular(pmg_laplacian op, const char* who, hipStream_t s)
{
  PMG_REQUIRE(!op->has_sigma, "%s: the constant null space is set, but the operator has a reaction term: it is not "
                              "singular and a projection would be wrong", who);
  PMG_REQUIRE(!op->has_robin, "%s: the constant null space is set, but the operator has a Robin term: it is not "
                              "singular and a projection would be wrong", who);
  if (op->n_marked_global < 0) // (collective on several ranks: every rank of a null-space solve gets here)
    PMG_TRY(sum_count_over_ranks(op->layout, op->n_marked, &op->n_marked_global,
                                 "the first null-space solve with an operator of several ranks counts its marked rows "
                                 "over the ranks and reads the count back: issue one outside the stream capture",
                                 s));
  PMG_REQUIRE(op->n_marked_global == 0, "%s: the constant null space is set, but the operator has %lld marked "
                                        "(Dirichlet) rows: it is not singular", who, op->n_marked_global);
  return PMG_OK;
}
} // namespace pmg

extern "C" int pmg_laplacian_set_reaction(pmg_laplacian op, const double* sigma, pmg_stream stream)
{
  PMG_REQUIRE(op, "pmg_laplacian_set_reaction: NULL argument");
  hipStream_t s = S(stream);
  PMG_TRY(not_capturing(s, "pmg_laplacian_set_reaction: not inside a stream capture (it allocates and synchronises)"));
  const int total = op->layout->total();
  if (!sigma)
  {
    if (!op->has_sigma)
      return PMG_OK;
    op->has_sigma = false; // (a Robin term stays: the vector becomes d_R)
  }
  else
  {
    // (a cell that is a ghost elsewhere is counted on each rank that holds it)
    PMG_TRY(require_valid(op->layout, op->ncells, sigma, FiniteNonNegative{},
                          "pmg_laplacian_set_reaction: %lld cells have a value that is not finite and >= 0", s));
    if (!op->sigma_buf)
      PMG_HIP(hipMalloc(&op->sigma_buf, sizeof(double) * (total ? total : 1)));
    op->has_sigma = true;
    // (summed with atomics in no fixed order: two sets of the same values agree to rounding, not bit for bit)
    PMG_HIP(hipMemsetAsync(op->sigma_buf, 0, sizeof(double) * (total ? total : 1), s));
    const long long nslots = (long long)op->npatch * op->K, n = nslots * op->N;
    if (n > 0)
      reaction_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(nslots, op->N, op->ng, op->pcell, op->xgeom, op->geom_dofmap,
                                                                 op->dphi_geom, op->gweights, op->dofmap, op->bc,
                                                                 sigma, op->sigma_buf);
    PMG_HIP(hipGetLastError());
  }
  return laplacian_data_changed(op, DATA_DIAGONAL_TERM, s); // (it waits for the stream: the caller may free sigma)
}

extern "C" int pmg_laplacian_get_geometry(pmg_laplacian op, double* G_out, pmg_stream stream)
{
  PMG_REQUIRE(op && G_out, "pmg_laplacian_get_geometry: NULL argument");
  hipStream_t s = S(stream);
  PMG_HIP(hipMemsetAsync(G_out, 0, sizeof(double) * 6 * (size_t)op->ncells * op->N, s));
  PMG_TRY(for_each_geometry_chunk(op, s, [&](int first, int count, const double2* G) {
    const long long nslots = (long long)count * op->K, n = nslots * op->N;
    geometry_export_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>((long long)first * op->K, nslots, op->nd,
                                                                     op->K, op->pcell, op->qperm, G, G_out);
  }));
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}

namespace pmg
{
// used by matrix.hip: the resident tensor as [ncells][nq][6] with q in the library's own (ascending) node order,
// whatever order the operator was created with -- the assembled matrix lives in the operator's dof numbering
int laplacian_geometry_ascending(pmg_laplacian op, double* G_out, hipStream_t s)
{
  PMG_REQUIRE(op->batch_patches == 0, "the geometry tensor is not resident (batched-geometry mode)");
  PMG_HIP(hipMemsetAsync(G_out, 0, sizeof(double) * 6 * (size_t)op->ncells * op->N, s));
  const long long nslots = (long long)op->npatch * op->K, n = nslots * op->N;
  if (n > 0)
    geometry_export_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(0, nslots, op->nd, op->K, op->pcell, nullptr,
                                                                     op->G, G_out);
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}
} // namespace pmg

extern "C" int pmg_laplacian_assemble_rhs(pmg_laplacian op, const double* f, double* b,
                                          pmg_stream stream)
{
  PMG_REQUIRE(op && f && b, "pmg_laplacian_assemble_rhs: NULL argument");
  hipStream_t s = S(stream);
  PMG_HIP(hipMemsetAsync(b, 0, sizeof(double) * op->layout->total(), s));
  const long long nslots = (long long)op->npatch * op->K;
  const long long n = nslots * op->N;
  if (n > 0)
    rhs_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(nslots, op->N, op->ng, op->pcell, op->xgeom,
                                                          op->geom_dofmap, op->dphi_geom,
                                                          op->gweights, op->dofmap, op->bc,
                                                          op->kappa, f, b);
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}

extern "C" int pmg_laplacian_time_kernel(pmg_laplacian op, const double* in, double* out, int reps,
                                         double* ms_per_launch, pmg_stream stream)
{
  PMG_REQUIRE(op && in && out && ms_per_launch && reps > 0,
              "pmg_laplacian_time_kernel: bad argument");
  hipStream_t s = S(stream);
  const int nl = (int)op->launch_first.size();
  PMG_REQUIRE(nl > 0, "pmg_laplacian_time_kernel: operator has no cells");
  // every launch of one operator application (all colours, both cell lists),
  // exactly the kernels pmg_laplacian_apply issues, without halo or zero-fill
  PMG_HIP(hipEventRecord(op->ev0, s));
  for (int r = 0; r < reps; ++r)
    PMG_TRY(run_launches(op, in, out, 0, nl, s));
  PMG_HIP(hipEventRecord(op->ev1, s));
  PMG_HIP(hipEventSynchronize(op->ev1));
  float ms = 0.f;
  PMG_HIP(hipEventElapsedTime(&ms, op->ev0, op->ev1));
  *ms_per_launch = (double)ms / reps / pmg_laplacian_launches_per_apply(op);
  return PMG_OK;
}

// src/laplacian.hpp:383-396 (examples/mat_free/main.cpp:34-50 --batch_size)
extern "C" int pmg_laplacian_set_geometry_batch(pmg_laplacian op, long long batch_cells)
{
  PMG_REQUIRE(op && batch_cells >= 0, "pmg_laplacian_set_geometry_batch: bad argument");
  int32_t bp = 0;
  if (batch_cells > 0)
  {
    const long long want = (batch_cells + op->K - 1) / op->K;
    bp = (int32_t)std::min<long long>(std::max<long long>(want, 1), std::max(op->npatch, 1));
  }
  if (bp == op->batch_patches)
    return PMG_OK;
  PMG_HIP(hipDeviceSynchronize()); // nothing may still read the tensor
  (void)hipFree(op->G);
  op->G = nullptr;
  const size_t per_patch = (size_t)gpatch(op->nd, op->K);
  const size_t gsize = per_patch * (size_t)(bp > 0 ? bp : op->npatch);
  PMG_HIP(hipMalloc(&op->G, sizeof(double2) * (gsize ? gsize : 1)));
  PMG_HIP(hipMemset(op->G, 0, sizeof(double2) * (gsize ? gsize : 1))); // padding of the flat layout
  PMG_HIP(hipStreamSynchronize(nullptr)); // (null-stream fill: not ordered against the caller's non-blocking stream)
  op->batch_patches = bp;
  op->stream_policy = streams_past_the_cache((long long)sizeof(double2) * gsize);
  if (bp == 0 && op->npatch > 0) // back to the resident tensor (on the null stream, as the fill above)
  {
    PMG_TRY(rebuild_resident_tensor(op, nullptr));
    PMG_HIP(hipDeviceSynchronize());
  }
  return PMG_OK;
}

extern "C" long long pmg_laplacian_geometry_bytes(pmg_laplacian op)
{
  if (!op)
    return -1;
  return (long long)sizeof(double2) * gpatch(op->nd, op->K) * (op->batch_patches > 0 ? op->batch_patches : op->npatch);
}

extern "C" int pmg_laplacian_set_profiling(pmg_laplacian op, int flag)
{
  PMG_REQUIRE(op, "pmg_laplacian_set_profiling: NULL argument");
  op->profiling = flag != 0;
  op->prof_used = 0;
  op->prof_launches = 0;
  return PMG_OK;
}

extern "C" int pmg_laplacian_read_profile(pmg_laplacian op, double* total_ms, long long* launches)
{
  PMG_REQUIRE(op && total_ms && launches, "pmg_laplacian_read_profile: NULL argument");
  double sum = 0.0;
  for (size_t i = 0; i + 1 < op->prof_used; i += 2)
  {
    PMG_HIP(hipEventSynchronize(op->prof_events[i + 1]));
    float ms = 0.f;
    PMG_HIP(hipEventElapsedTime(&ms, op->prof_events[i], op->prof_events[i + 1]));
    sum += ms;
  }
  *total_ms = sum;
  *launches = op->prof_launches;
  op->prof_used = 0;
  op->prof_launches = 0;
  return PMG_OK;
}

// number of stiffness-kernel launches one operator application issues
extern "C" int pmg_laplacian_launches_per_apply(pmg_laplacian op)
{
  if (!op)
    return -1;
  // (the two walks of apply_impl; a whole walk may coalesce them: laplacian_single_launch)
  int n = 0;
  const int nl = (int)op->launch_first.size();
  const auto count = [&](const LaunchStep& st) { return n += st.launches(), PMG_OK; };
  for_each_launch_step(*op, op->chain_first, op->chain_count, 0, op->n_launch_l, apply_form(op), count);
  for_each_launch_step(*op, op->chain_first, op->chain_count, op->n_launch_l, nl, apply_form(op), count);
  return n;
}

// Chain form of the interior launches (stiffness_chain_kernel): 1 = in use, 0 = not; set: PMG_ERR_INVALID if the
// operator has no chains (small or merged level, no tensor grid of patches, another degree).
extern "C" int pmg_laplacian_chain_form(pmg_laplacian op) { return !op ? -1 : op->chain_on ? 1 : 0; }
extern "C" int pmg_laplacian_chain_available(pmg_laplacian op) { return !op ? -1 : op->chain_ok ? 1 : 0; }
extern "C" int pmg_laplacian_set_chain_form(pmg_laplacian op, int on)
{
  PMG_REQUIRE(op, "pmg_laplacian_set_chain_form: NULL argument");
  if (on && !op->chain_ok)
    return fail(PMG_ERR_INVALID, "pmg_laplacian_set_chain_form: the operator has no chains of patches");
  op->chain_on = on != 0;
  return PMG_OK;
}

// 2 if the interior launches of an application run as two halves on two streams, else 1
extern "C" int pmg_laplacian_apply_streams(pmg_laplacian op)
{
  return !op ? -1 : apply_form(op).two_streams ? 2 : 1;
}

