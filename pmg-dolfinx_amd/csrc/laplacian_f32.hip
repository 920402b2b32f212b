// Single-precision form of the operator: the stiffness apply of the FP32 V-cycle (solvers.hip mg_apply_f32) and of
// pmg_laplacian_apply_f32.
//
// Same patch plan as the FP64 apply (laplacian.hip): one workgroup per patch, the patch's x values and y sums in
// LDS, the colours launched in plan order with plain stores, the merged launch of a small level and of the boundary
// shell adding with float atomics, bzero cleared first, Dirichlet rows y = x written by their first patch.  What
// changes is the width of every byte: the stored tensor is float (24 B per quadrature point instead of 48), the vectors
// are float, and the cell sums meet in LDS with ds_add_f32.  kappa is read from the caller's array in every
// application and multiplies the cell's input, as in the FP64 kernels (the caller may change it between two).
//
// The tensor (without kappa) is computed in FP64 from the mesh (the Jacobian of laplacian.hpp) and rounded once, on the
// first FP32 use of the operator; it is never converted from the FP64 tensor (which may not be resident: batched
// geometry).
//
// One kernel form for every degree: the column scheme of laplacian.hip -- a lane owns the (a, b) column of a cell,
// keeps the column's values in registers and marches through the nd layers; the x and y contractions pass one nd x nd
// slice through LDS, the z contraction stays in registers.  The layer march, the lane's table rows, the tensor stream (GD
// layers deep here), the fences and the loads are the FP64 kernels' own, instantiated for float
// (stiffness_layer.hpp).  Half-width registers let
// every degree run eight wavefronts per workgroup where it has the items (P = 6: 49 of 64 lanes, P = 7: 64 of 64),
// and P = 5 / P = 8 share one item of 7 / 3 cells between four wavefronts as the FP64 kernel does.
#include "laplacian.hpp"
#include "tensor_kernels.hpp"
#include "stiffness_layer.hpp"

#include <algorithm>

using namespace pmg;

namespace
{
template <int P>
struct Shape32
{
  static constexpr int ND = P + 1;
  static constexpr int N = ND * ND * ND;
  static constexpr int NQ2 = ND * ND;
  static constexpr PatchShape PS = patch_shape(P);
  static constexpr int K = PS.bx * PS.by * PS.bz;
  static constexpr int MAXM = PS.max_m;
  static constexpr bool SHARED_ITEM = P == 5 || P == 8; // one item of K cells over four wavefronts (patches.hpp)
  static constexpr int CW = SHARED_ITEM ? K : (NQ2 <= 64 ? 64 / NQ2 : 1); // cells per item
  static constexpr int WPC = SHARED_ITEM ? 4 : (NQ2 + 63) / 64;            // wavefronts per item
  static_assert(CW * NQ2 <= 64 * WPC, "an item's columns need a lane each");
  static constexpr int WL = CW * NQ2; // columns of an item
  static constexpr int ITEMS = (K + CW - 1) / CW;
  static constexpr int NWMAX = 8;
  static constexpr int NG = ITEMS < NWMAX / WPC ? ITEMS : NWMAX / WPC; // items in flight per workgroup
  static constexpr int NW = NG * WPC;
  static constexpr int THREADS = NW * 64;
  static constexpr int ITER = (MAXM + THREADS - 1) / THREADS; // patch list entries per thread
  // layers of the tensor in flight per wavefront: a float layer is half the bytes of a double one, so twice as many
  // are needed for the same bytes in flight per compute unit
  static constexpr int GD = (P == 1 || P == 4) ? 2 : 3; // (P = 4: two, or the six wavefronts per SIMD below spill)
  // waves per SIMD the register allocation must leave room for: three workgroups of eight wavefronts per compute unit
  // up to P = 4 (the tensor stream needs the wavefronts), what the cell loop needs above
  static constexpr int MIN_WAVES = P <= 4 ? 6 : 1;
  static_assert(MAXM <= 65535, "patch positions are 16-bit");
};

// Where the geometry kernels (tensor_kernels.hpp) put a point's six values: G32 [slot][layer c][pair][a*nd+b].  The
// values are formed in double, nodal coefficient and per-cell tensor folded in (point_tensor); this is the one rounding.
struct TensorOut32
{
  float2* G;
  int nd;
  __device__ __forceinline__ void operator()(long long slot, int q, const double g[6]) const
  {
    const int nsq = nd * nd, nq = nsq * nd;
    const int a = q / nsq, b = (q - a * nsq) / nd, cc = q - a * nsq - b * nd;
    float2* o = G + (size_t)slot * 3 * nq + (size_t)cc * 3 * nsq + a * nd + b;
    o[0] = make_float2((float)g[0], (float)g[1]);
    o[nsq] = make_float2((float)g[2], (float)g[3]);
    o[2 * nsq] = make_float2((float)g[4], (float)g[5]);
  }
};

template <int P, bool NT>
__global__ void __launch_bounds__(Shape32<P>::THREADS, Shape32<P>::MIN_WAVES)
    stiffness_f32_kernel(const float* __restrict__ x, float* __restrict__ y, const float2* __restrict__ G,
                         const int32_t* __restrict__ poff, const uint32_t* __restrict__ pdofs,
                         const int32_t* __restrict__ lmap_id, const uint16_t* __restrict__ lmaps,
                         const int32_t* __restrict__ pcell, const int32_t* __restrict__ pncell,
                         const double* __restrict__ kappa, const float* __restrict__ Dg,
                         const float* __restrict__ react, int first, int atomic_out)
{
  using Sh = Shape32<P>;
  constexpr int ND = Sh::ND, N = Sh::N, K = Sh::K, NQ2 = Sh::NQ2, NG = Sh::NG, WPC = Sh::WPC, WL = Sh::WL;
  constexpr int MAXM = Sh::MAXM, THREADS = Sh::THREADS, CW = Sh::CW, ITER = Sh::ITER, GD = Sh::GD;
  constexpr bool SHARED = WPC > 1; // the item's wavefronts exchange their slices through workgroup barriers
  __shared__ float sD[ND * ND];
  __shared__ float sx[MAXM];
  __shared__ float sy[MAXM];
  __shared__ float sq[NG * WL];
  __shared__ float sgr[NG * WL];
  __shared__ float sgs[NG * WL];
  __shared__ float skap[K];

  const int p = first + blockIdx.x;
  const int t = threadIdx.x;
  const int off = poff[p];
  const int M = poff[p + 1] - off; // 1 <= M <= MAXM
  const int table = lmap_id[p];
  const int nc = pncell[p];

  // gather: x (zero on Dirichlet dofs, src/laplacian.hpp:186-189) and, in a coloured launch, the sums the earlier
  // colours stored for the dofs they share with this patch
  // (unconditional loads with clamped indices, all issued before the first is used)
  {
    uint32_t m[ITER];
    float xv[ITER], yv[ITER];
#pragma unroll
    for (int k = 0; k < ITER; ++k)
    {
      const int i = t + k * THREADS;
      m[k] = pdofs[off + (i < M ? i : M - 1)];
    }
#pragma unroll
    for (int k = 0; k < ITER; ++k)
    {
      const uint32_t dof = m[k] & PD_MASK;
      const bool acc = !atomic_out && (m[k] & (PD_ACC | PD_BC)) == PD_ACC;
      xv[k] = x[dof];
      // (no sum to continue: the reaction vector where the operator has one, else x again -- stiffness_column.hpp)
      yv[k] = *(acc ? (const float*)(y + dof) : react ? react + dof : x + dof);
    }
#pragma unroll
    for (int k = 0; k < ITER; ++k)
    {
      const int i = t + k * THREADS;
      if (i < M)
      {
        const bool acc = !atomic_out && (m[k] & (PD_ACC | PD_BC)) == PD_ACC;
        sx[i] = (m[k] & PD_BC) ? 0.0f : xv[k];
        const bool starts = react && !(m[k] & (PD_ACC | PD_BC)); // the dof's first patch starts at react * x
        sy[i] = acc ? yv[k] : starts ? yv[k] * xv[k] : 0.0f;
      }
    }
  }
  if (t < ND * ND)
    sD[t] = Dg[t];
  for (int i = t; i < K; i += THREADS) // kappa of the patch's cells (empty slots: any finite value, never added)
  {
    const int c = pcell[(size_t)p * K + i];
    skap[i] = (float)kappa[c >= 0 ? c : 0];
  }
  lds_barrier();

  const int wave = (t >> 6) / WPC, lane = (t & 63) + 64 * ((t >> 6) % WPC);
  const bool lane_ok = lane < WL;
  const int lw = lane_ok ? lane : WL - 1; // idle lanes shadow the last column (finite values, no contribution)
  const int cw = lw / NQ2, ab = lw - cw * NQ2;
  const int a = ab / ND, b = ab - a * ND;
  LaneTables<float, ND> T;
  T.fill((const __attribute__((address_space(3))) float*)sD, a, b);
  float* q_s = sq + wave * WL + cw * NQ2;
  float* gr_s = sgr + wave * WL + cw * NQ2;
  float* gs_s = sgs + wave * WL + cw * NQ2;
  // wavefronts that share an item exchange slices through workgroup barriers: all of them run the same item count
  const int items = WPC > 1 ? (((nc + CW - 1) / CW + NG - 1) / NG) * NG : (nc + CW - 1) / CW;
  const uint16_t* lmb = lmaps + (size_t)table * (K * N);
  for (int it = wave; it < items; it += NG)
  {
    const int slot = it * CW + cw;
    const int slotc = slot < K ? slot : K - 1;
    const unsigned lmo = (unsigned)(slotc * N + ab);
    int l[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k)
      l[k] = lmb[lmo + (unsigned)(k * NQ2)];
    // layers 0 .. GD-1 in flight, slot k % GD refilled with layer k + GD once layer k is read
    TensorStream<float2, ND, WL, GEO_STORED, false, 0, NT, GD> gs;
    gs.prime(G + (size_t)p * K * 3 * N, (unsigned)(slotc * 3 * N + ab));
    // kappa multiplies the cell's input once (the operator is linear in it), as in the FP64 kernels
    const float kap = skap[slotc];
    float u[ND], Aq[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k)
    {
      u[k] = kap * sx[l[k]];
      Aq[k] = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < ND; ++k)
    {
      float2 g01, g23, g45;
      gs.take(k, 1.0f, g01, g23, g45);
      float fr, fs, ft;
      layer_forward<ND, false, SHARED>(k, u, T, Dg, q_s, a, b, ab, g01, g23, g45, 1.0f, fr, fs, ft);
      layer_backward<ND, false, SHARED>(k, fr, fs, ft, T, Dg, gr_s, gs_s, a, b, ab, Aq);
    }
    // every lane adds (lanes without a cell add an exact zero: no branch around the accumulation, and the sum is read
    // ahead of the select, see the epilogue of stiffness_column_kernel)
    const bool contributes = lane_ok && slot < nc;
#pragma unroll
    for (int k = 0; k < ND; ++k)
    {
      const float Ak = Aq[k];
      atomicAdd(&sy[l[k]], contributes ? Ak : 0.0f); // ds_add_f32
    }
  }
  // write-back: sums of the non-Dirichlet dofs (store onto the earlier colours' values, or a float atomic in a merged
  // launch); the Dirichlet rows y = x by the first patch that holds them (src/laplacian.hpp:273-274).  The list is
  // re-read before the closing barrier, so that no dependent load sits behind it.
  int tw = t;
  asm volatile("" : "+v"(tw)); // (opaque: the list addresses are not computed ahead and held through the cell loop)
  uint32_t mk[ITER];
#pragma unroll
  for (int k = 0; k < ITER; ++k)
  {
    const int i = tw + k * THREADS;
    mk[k] = pdofs[off + (i < M ? i : M - 1)];
  }
  lds_barrier();
#pragma unroll
  for (int k = 0; k < ITER; ++k)
  {
    const int i = tw + k * THREADS;
    if (i >= M)
      break;
    const uint32_t m = mk[k];
    const uint32_t dof = m & PD_MASK;
    if (!(m & PD_BC))
    {
      if (atomic_out)
        atomicAdd(&y[dof], sy[i]);
      else if constexpr (NT)
        __builtin_nontemporal_store(sy[i], &y[dof]);
      else
        y[dof] = sy[i];
    }
    else if (!(m & PD_ACC))
      y[dof] = x[dof];
  }
}

__global__ void zero_list_f32_kernel(int n, const int32_t* __restrict__ idx, float* __restrict__ y)
{
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    y[idx[i]] = 0.0f;
}

__global__ void fill_f32_kernel(int n, float* __restrict__ y)
{
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    y[i] = 0.0f;
}

__global__ void to_float_kernel(int n, const double* __restrict__ in, float* __restrict__ out)
{
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    out[i] = (float)in[i];
}

int grid_for(long long n) { return (int)std::min<long long>((n + 255) / 256, 2048); }

// one launch of the float stiffness kernel over the patches [first, first + count); the tensor streams past the
// Infinity Cache under the FP64 rule at half the bytes (stream_policy32: nt loads and stores)
int launch_patches_f32(pmg_laplacian op, const float* x, float* y, int first, int count, int atomic_out, hipStream_t s)
{
  PMG_TRY(with_degree(op->P, [&](auto degree) {
    constexpr int P = decltype(degree)::value;
    auto launch = [&](auto nt) {
      stiffness_f32_kernel<P, decltype(nt)::value><<<count, Shape32<P>::THREADS, 0, s>>>(
          x, y, op->G32, op->poff, op->pdofs, op->lmap_id, op->lmaps, op->pcell, op->pncell, op->kappa, op->D32,
          op->react32, first, atomic_out);
    };
    (P >= NT_FROM && op->stream_policy32) ? launch(std::true_type{}) : launch(std::false_type{});
    return PMG_OK;
  }));
  op->launches++;
  return PMG_OK;
}
} // namespace

namespace pmg
{
// Can this operator run in FP32?  (0 = yes, else the refusal has been recorded)
int laplacian_f32_supported(pmg_laplacian op, const char* who)
{
  pmg_layout l = op->layout;
  PMG_REQUIRE(l->num_ghosts == 0 && !l->multi_rank() && !l->win,
              "%s: FP32 is single-domain only (the layout has ghosts or a communicator)", who);
  PMG_REQUIRE(op->batch_patches == 0, "%s: FP32 needs the resident geometry (the operator is in batched-geometry mode)",
              who);
  return PMG_OK;
}

// The float tensor, (re)computed in place from the geometry and the coefficient field (if one is set)
int laplacian_f32_refresh(pmg_laplacian op, hipStream_t s)
{
  if (!op->G32)
    return PMG_OK;
  launch_geometry(op, 0, (long long)op->npatch * op->K, TensorOut32{op->G32, op->nd}, s); // the FP64 tensor's routine
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}

// The float copy of the reaction vector: in use exactly while the vector and the float tensor both exist (allocated
// once, rewritten in place by a later set of the reaction or the Robin term; the removal of the last of the two takes
// it out of use with the vector -- laplacian_data_changed)
int laplacian_f32_reaction(pmg_laplacian op, hipStream_t s)
{
  if (!op->G32 || !op->react)
    return PMG_OK;
  const int total = op->layout->total();
  if (!op->react32_buf)
    PMG_HIP(hipMalloc(&op->react32_buf, sizeof(float) * (total ? total : 1)));
  op->react32 = op->react32_buf;
  if (total > 0)
    to_float_kernel<<<grid_for(total), 256, 0, s>>>(total, op->react, op->react32);
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}

// The float tensor and 1-D table, built on the first FP32 use (outside any stream capture: it allocates)
int laplacian_f32_prepare(pmg_laplacian op, hipStream_t s)
{
  if (op->G32)
    return PMG_OK;
  const long long nslots = (long long)op->npatch * op->K, n = nslots * op->N;
  PMG_HIP(hipMalloc(&op->G32, sizeof(float2) * 3 * (size_t)(n > 0 ? n : 1)));
  PMG_HIP(hipMalloc(&op->D32, sizeof(float) * op->nd * op->nd));
  to_float_kernel<<<1, 256, 0, s>>>(op->nd * op->nd, op->D, op->D32);
  op->stream_policy32 = streams_past_the_cache((long long)sizeof(float2) * 3 * n);
  PMG_TRY(laplacian_f32_reaction(op, s));
  return laplacian_f32_refresh(op, s);
}

// float copy of the operator's diagonal inverse, refreshed when the diagonal has changed since; `*changed` (optional)
// tells the caller that a conversion was enqueued
int laplacian_f32_diag(pmg_laplacian op, const float** d, hipStream_t s, bool* changed)
{
  const int total = op->layout->total();
  if (changed)
    *changed = false;
  if (!op->diag32)
    PMG_HIP(hipMalloc(&op->diag32, sizeof(float) * (total ? total : 1)));
  if (op->diag32_version != op->diag_version)
  {
    if (total > 0)
      to_float_kernel<<<grid_for(total), 256, 0, s>>>(total, op->diag_inv, op->diag32);
    PMG_HIP(hipGetLastError());
    op->diag32_version = op->diag_version;
    if (changed)
      *changed = true;
  }
  *d = op->diag32;
  return PMG_OK;
}
long long laplacian_diag_version(pmg_laplacian op) { return op->diag_version; }

// out = A in in FP32, with the semantics of laplacian_apply on a layout without ghosts: out is overwritten, the
// Dirichlet rows are out = in, every launch of the plan in its order (the two-stream and chain forms of the FP64
// apply are not used).  The operator must have been prepared (laplacian_f32_prepare).
int laplacian_apply_f32(pmg_laplacian op, const float* in, float* out, hipStream_t s)
{
  pmg_layout l = op->layout;
  if (laplacian_wants_zeroed_output(op))
  {
    if (l->total() > 0)
      fill_f32_kernel<<<grid_for(l->total()), 256, 0, s>>>(l->total(), out);
  }
  else if (op->n_bzero > 0)
    zero_list_f32_kernel<<<grid_for(op->n_bzero), 256, 0, s>>>(op->n_bzero, op->bzero, out);
  // (the default form: one stream, no chains)
  PMG_TRY(walk_launches(op, 0, (int)op->launch_first.size(), ApplyForm{}, s, [&](const LaunchStep& st, hipStream_t sl) {
    return launch_patches_f32(op, in, out, st.first, st.count, st.atomic_out, sl);
  }));
  op->applies++;
  return PMG_OK;
}
} // namespace pmg

extern "C" int pmg_laplacian_apply_f32(pmg_laplacian op, float* in, float* out, pmg_stream stream)
{
  PMG_REQUIRE(op && in && out, "pmg_laplacian_apply_f32: NULL argument");
  PMG_REQUIRE(in != out, "pmg_laplacian_apply_f32: in and out alias");
  PMG_TRY(laplacian_f32_supported(op, "pmg_laplacian_apply_f32"));
  hipStream_t s = S(stream);
  PMG_TRY(laplacian_f32_prepare(op, s));
  return laplacian_apply_f32(op, in, out, s);
}
