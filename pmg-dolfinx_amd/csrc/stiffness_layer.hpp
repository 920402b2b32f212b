// The layer march of the stiffness apply, defined once for its four kernels: stiffness_column_kernel
// (stiffness_column.hpp), stiffness_restrict_kernel (stiffness_restrict.hpp), stiffness_chain_kernel
// (stiffness_chain.hpp) and stiffness_f32_kernel (laplacian_f32.hip).
//
// A lane owns the column of nd points above (a, b) of a cell and keeps it in registers.  One layer k of the march:
// write the slice u(., ., k), contract x and y through LDS and z in registers, form the three fluxes from the six
// tensor entries, contract back, accumulate.  The scalar type T is double or float, T2 the matching pair.
//
// Everything here is forced inline into the kernel that calls it: the callers' register allocations were tuned
// against measured spills.  Against the text written out in each kernel, every kernel keeps 0 bytes of scratch and its
// occupancy; the instruction order differs in all of them and a few register counts move (affine column kernels at
// P = 4, 6, 7: 6 VGPRs more; P = 8 stored: 2 fewer).  The table and the timings are in profiles/layer_march.md.
#pragma once

#include "laplacian.hpp" // adjugate, metric: the recomputed tensor is formed with the geometry kernels' expressions

#include <hip/hip_runtime.h>

namespace pmg
{
// where an apply kernel's tensor comes from (a template argument of the column and restrict kernels)
constexpr int GEO_STORED = 0;    // the stored tensor G is streamed
constexpr int GEO_AFFINE = 1;    // one constant tensor per (parallelepiped) cell
constexpr int GEO_RECOMPUTE = 2; // trilinear cells: G is formed in the layer march from the cell's 24 coefficients

// ---- synchronisation of a slice exchange (also of the patch transfers' wave-private scratch, interpolate.hip) -----
// LDS executes a wavefront's instructions in order: where one wavefront owns the slices a compiler fence is all the
// exchange needs, no s_barrier and no waitcnt.
__device__ __forceinline__ void wave_fence()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains
// the vector-memory counter (s_waitcnt vmcnt(0)), which would stall every wave on
// the G loads issued at the top of the kernel; nothing in these kernels passes data
// between threads through global memory, so LDS ordering is all that is needed
// (cdna_hip_programming.md, "Pipelining across barriers").
__device__ __forceinline__ void lds_barrier()
{
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// SHARED: several wavefronts share the item and exchange its slices through workgroup barriers
template <bool SHARED>
__device__ __forceinline__ void slice_sync()
{
  if constexpr (SHARED)
    lds_barrier();
  else
    wave_fence();
}

// ---- loads ----------------------------------------------------------------------------------------------------
// Cache policy.  The G stream is read exactly once per application and is ~6x larger
// than the MALL: it is loaded non-temporally (nt bit) so that it does not displace x, y,
// the dof lists and the shared tables from L2 / MALL, and the write-back stores of y are
// non-temporal as well.  Measured at P = 4, 64^3: 505 -> 475 us with nt stores, -> 430 us
// with nt G loads on top; the sc0 / sc1 bits make no difference; nt on the x / y gathers
// or on the dof lists is slower.
// At P = 1 (8 quadrature points per cell, every dof shared by 8 cells) the default
// policy is faster (1610 vs 1750 us at 256^3), so the hint starts at P = 2.
constexpr int NT_FROM = 2;
template <typename T2>
struct scalar_of;
template <>
struct scalar_of<double2>
{
  using type = double;
};
template <>
struct scalar_of<float2>
{
  using type = float;
};
template <bool NT, typename T2> // T2: double2 or float2
__device__ __forceinline__ T2 gload(const T2* p)
{
  if constexpr (NT)
  {
    typedef typename scalar_of<T2>::type vec2 __attribute__((ext_vector_type(2)));
    vec2 v = __builtin_nontemporal_load(reinterpret_cast<const vec2*>(p));
    return T2(v.x, v.y);
  }
  else
    return *p;
}

// Slice reads.  The compiler pairs neighbouring LDS reads into ds_read2_b64; issued one by one
// (volatile LDS loads are not paired) the FP64 kernel is 7 % faster at P = 5 and 4 % at P = 8, unchanged at
// P <= 4 and slower at P = 6, 7 (profiles/kernel_tuning_r02.md).
template <bool UNPAIRED, typename T>
__device__ __forceinline__ T slice_load(T& v)
{
  if constexpr (UNPAIRED)
    return *(__attribute__((address_space(3))) volatile T*)&v;
  else
    return v;
}

// ---- the lane's rows / columns of the 1-D table, in registers ---------------------------------------------------
// (4 nd values; re-reading them from LDS in every layer frees the registers for one more wave per SIMD but is 15 %
// slower at every degree, profiles/kernel_tuning_r02.md)
template <typename T, int ND>
struct LaneTables
{
  T Da[ND], Db[ND], DTa[ND], DTb[ND]; // D[a][.], D[b][.], D[.][a], D[.][b]
  // sD: the LDS copy of D (typed as such: the index arithmetic of an LDS address is 32-bit)
  __device__ __forceinline__ void fill(const __attribute__((address_space(3))) T* sD, int a, int b)
  {
#pragma unroll
    for (int mm = 0; mm < ND; ++mm)
    {
      Da[mm] = sD[a * ND + mm];
      Db[mm] = sD[b * ND + mm];
      DTa[mm] = sD[mm * ND + a];
      DTb[mm] = sD[mm * ND + b];
    }
  }
};

// ---- one layer --------------------------------------------------------------------------------------------------
// Two parts, because the chain kernel issues its tensor refill between them.  q_s / gr_s / gs_s are the cell's three
// nd x nd slices in LDS, Dg the 1-D table in global memory: its entries in row k are wave-uniform (scalar loads).
//
// Forward: u(., ., k) into the slice; qr, qs, qt; the three fluxes times `scale`.
template <int ND, bool UNPAIRED, bool SHARED, typename T, typename T2>
__device__ __forceinline__ void layer_forward(int k, const T (&u)[ND], const LaneTables<T, ND>& D,
                                              const T* Dg, T* q_s, int a, int b, int ab, const T2& g01,
                                              const T2& g23, const T2& g45, T scale, T& fr, T& fs, T& ft)
{
  q_s[ab] = u[k];
  slice_sync<SHARED>();
  T qr = 0, qs = 0, qt = 0;
#pragma unroll
  for (int mm = 0; mm < ND; ++mm)
  {
    qr += D.Da[mm] * slice_load<UNPAIRED>(q_s[mm * ND + b]); // d/dx: sum over a, src/laplacian.hpp:195-199
    qs += D.Db[mm] * slice_load<UNPAIRED>(q_s[a * ND + mm]); // d/dy: sum over b, :206-210
    qt += Dg[k * ND + mm] * u[mm];                           // d/dz: registers, uniform table, :214-218
  }
  fr = scale * (g01.x * qr + g01.y * qs + g23.x * qt); // :233
  fs = scale * (g01.y * qr + g23.y * qs + g45.x * qt); // :234
  ft = scale * (g23.x * qr + g45.x * qs + g45.y * qt); // :235
}

// Backward: the x and y fluxes into their slices, the two transposed contractions, the z one in registers.
template <int ND, bool UNPAIRED, bool SHARED, typename T>
__device__ __forceinline__ void layer_backward(int k, T fr, T fs, T ft, const LaneTables<T, ND>& D,
                                               const T* Dg, T* gr_s, T* gs_s, int a, int b, int ab,
                                               T (&Aq)[ND])
{
  gr_s[ab] = fr;
  gs_s[ab] = fs;
  slice_sync<SHARED>();
  T acc = 0;
#pragma unroll
  for (int mm = 0; mm < ND; ++mm)
  {
    acc += D.DTa[mm] * slice_load<UNPAIRED>(gr_s[mm * ND + b]); // :246-251
    acc += D.DTb[mm] * slice_load<UNPAIRED>(gs_s[a * ND + mm]); // :255-259
    Aq[mm] += Dg[k * ND + mm] * ft;                             // :263-267
  }
  Aq[k] += acc;
  slice_sync<SHARED>();
}

// Backward by the barycentric identity beside the recomputed tensor (transposes_by_identity, stiffness_column.hpp: the
// identity and what it is worth are stated there): the transposed contractions as forward ones of the scaled fluxes,
//     (D^T f)_i = 2 D_ii f_i - rho_i sum_j D_ij (f_j / rho_j),
// so the lane needs rho and 1 / rho for its a and b instead of the columns D[.][a], D[.][b].  2 D_aa and 2 D_bb are
// not held either: they are picked per layer out of the rows D[a][.], D[b][.] the lane holds anyway, by ND - 1 selects
// each on an opaque copy of the column index (the copy keeps the picked values from being formed ahead of the layer
// loop and held through it).
template <int ND, bool UNPAIRED, bool SHARED, typename T>
__device__ __forceinline__ void layer_backward_identity(int k, T fr, T fs, T ft, const LaneTables<T, ND>& D,
                                                        const T* Dg, T* gr_s, T* gs_s, int a, int b, int ab, T rho_a,
                                                        T irho_a, T rho_b, T irho_b, T (&Aq)[ND])
{
  gr_s[ab] = fr * irho_a;
  gs_s[ab] = fs * irho_b;
  slice_sync<SHARED>();
  T sx_ = 0, sy_ = 0;
#pragma unroll
  for (int mm = 0; mm < ND; ++mm)
  {
    sx_ += D.Da[mm] * slice_load<UNPAIRED>(gr_s[mm * ND + b]); // :246-251
    sy_ += D.Db[mm] * slice_load<UNPAIRED>(gs_s[a * ND + mm]); // :255-259
    Aq[mm] += Dg[k * ND + mm] * ft;                            // :263-267
  }
  int abv = ab;
  asm volatile("" : "+v"(abv));
  const int av = abv / ND, bv = abv - av * ND;
  T daa = D.Da[0], dbb = D.Db[0];
#pragma unroll
  for (int mm = 1; mm < ND; ++mm)
  {
    daa = av == mm ? D.Da[mm] : daa;
    dbb = bv == mm ? D.Db[mm] : dbb;
  }
  Aq[k] += 2 * (daa * fr + dbb * fs) - (rho_a * sx_ + rho_b * sy_);
  slice_sync<SHARED>();
}

// ---- patch positions, two to a register -------------------------------------------------------------------------
// Positions in a patch list are 16-bit.  Where a kernel needs a column's positions again behind the layer loop it
// holds them packed through it, and opaque, so that the unpacked values are not kept alongside.
template <int N>
__device__ __forceinline__ void pack_positions(const int (&l)[N], unsigned (&lp)[(N + 1) / 2])
{
#pragma unroll
  for (int k = 0; k < N; k += 2)
    lp[k / 2] = (unsigned)l[k] | (k + 1 < N ? (unsigned)l[k + 1] << 16 : 0u);
#pragma unroll
  for (int j = 0; j < (N + 1) / 2; ++j)
    asm volatile("" : "+v"(lp[j]));
}
__device__ __forceinline__ unsigned packed_position(const unsigned* lp, int k)
{
  return (lp[k / 2] >> (16 * (k & 1))) & 0xffffu;
}

// ---- the tensor stream of the column and restrict kernels: one layer ahead of the march ---------------------------
// Four forms.  Default layout: the lane's three pairs of layers 0 .. GD-1 in flight in registers, slot k % GD
// refilled with layer k + GD once layer k is taken.  Flat layout (FLAT, P = 2): the item's next layer as loaded,
// NJ x 64 pairs with a layer stride of LS, handed over to the lanes through `gb` in LDS.  Affine cells (AFF):
// G_q = w_a w_b w_c Gc with one constant tensor Gc per cell, no stream.  Trilinear cells (RCP): x = sum c_ijk xi^i
// eta^j zeta^k on [0,1]^3, so down the lane's column (xi_a, eta_b fixed) dx/dxi and dx/deta are linear in zeta and
// dx/dzeta is constant: 15 values per lane, from which layer k forms J(zeta_k), adj(J), |det J| and the six entries
// w_a w_b w_k adj(J) adj(J)^T / |det J| with the geometry kernels' own adjugate() and metric() -- the stored tensor to
// rounding, no stream.  adj adj^T / det is homogeneous of degree one in J, so w_a w_b is folded into the 15 values.
// Where the two slopes vanish in every lane of an item the tensor is formed once, ahead of the march (column_constant,
// hoist_column, take_column; the callers branch, stiffness_column.hpp column_branch).
template <typename T2, int ND, int WL, int GEO, bool FLAT, int LS, bool NT, int GD>
struct TensorStream
{
  using T = typename scalar_of<T2>::type;
  static constexpr bool AFF = GEO == GEO_AFFINE, RCP = GEO == GEO_RECOMPUTE;
  static_assert(!(FLAT && GEO != GEO_STORED), "the flat layout is a layout of the stored tensor");
  static constexpr int GPS = ND * ND; // stride between the three pairs of a layer
  static constexpr int FL = 3 * WL, NJ = (FL + 63) / 64;
  T2 gq[AFF || RCP || FLAT ? 1 : GD][3];
  T2 gfl[FLAT ? NJ : 1]; // flat layout: the next layer as loaded
  int eo[FLAT ? NJ : 1]; // the lane's elements of a layer (clamped: the tail lanes re-read the last one)
  T gc[AFF ? 6 : 1];
  T jc[RCP ? 5 : 1][3]; // dx/dxi at zeta = 0 and its slope in zeta, dx/deta likewise, dx/dzeta; times w_a w_b
  const T* zeta;        // the 1-D GLL nodes (wave-uniform reads)
  const T2* base;    // scalar base: the patch (default layout) or the item (flat layout)
  unsigned lane_off; // default layout: the lane's (layer 0, pair 0) as a 32-bit offset (a 64-bit per-lane pointer
                     // costs two registers, and a spilled one is reloaded behind a wait that drains the memory counter)
  T2* gb;            // flat layout: the wavefront's NJ x 64 pairs in LDS
  int lane, lw;      // flat layout: the lane, and the column it works on

  // default layout: request layers 0 .. GD-1
  __device__ __forceinline__ void prime(const T2* patch, unsigned lane_off_)
  {
    static_assert(GEO == GEO_STORED && !FLAT);
    base = patch;
    lane_off = lane_off_;
#pragma unroll
    for (int d = 0; d < GD; ++d)
      fetch(d, d);
  }
  // flat layout: request layer 0 of the item
  __device__ __forceinline__ void prime_flat(const T2* item, T2* gb_, int lane_, int lw_)
  {
    static_assert(FLAT);
    base = item;
    gb = gb_;
    lane = lane_;
    lw = lw_;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj)
      eo[jj] = lane + 64 * jj < FL ? lane + 64 * jj : FL - 1;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj)
      gfl[jj] = gload<NT>(base + eo[jj]);
  }
  // affine cells: the cell's constant tensor times `fold`
  __device__ __forceinline__ void prime_affine(const T* ga, T fold)
  {
    static_assert(AFF);
#pragma unroll
    for (int d = 0; d < 6; ++d)
      gc[d] = fold * ga[d];
  }
  // trilinear cells: cc = the cell's eight coefficient vectors [4 i + 2 j + k][3] (all zero in an empty slot), (xi, eta)
  // the lane's column, `fold` its weights w_a w_b, nodes the 1-D GLL nodes
  __device__ __forceinline__ void prime_recompute(const T* cc, T xi, T eta, T fold, const T* nodes)
  {
    static_assert(RCP);
    zeta = nodes;
#pragma unroll
    for (int i = 0; i < 3; ++i)
    {
      const T c001 = cc[3 + i], c010 = cc[6 + i], c011 = cc[9 + i], c100 = cc[12 + i], c101 = cc[15 + i],
              c110 = cc[18 + i], c111 = cc[21 + i];
      const T e1 = c011 + c111 * xi;
      jc[0][i] = fold * (c100 + c110 * eta);
      jc[1][i] = fold * (c101 + c111 * eta);
      jc[2][i] = fold * (c010 + c110 * xi);
      jc[3][i] = fold * e1;
      jc[4][i] = fold * (c001 + c101 * xi + e1 * eta);
    }
  }
  // Trilinear cells: is J constant down every column of the item?  The slopes jc[1], jc[3] of
  // every lane are exactly zero where the cells' zeta-cross coefficients c101, c011, c111 vanish: the top face is a
  // translate of the bottom face (boxes, tensor grids, extruded meshes).  J, adj(J), det J, the reciprocal and
  // adj adj^T / |det J| are then those of layer 0 in every layer, and only w_k changes.  Six compares and one ballot,
  // wave-uniform; idle lanes and clamped slots hold copies of real columns, empty slots zeros: they decide with the rest.
  __device__ __forceinline__ bool column_constant() const
  {
    static_assert(RCP);
    bool varies = false;
#pragma unroll
    for (int i = 0; i < 3; ++i)
      varies = varies || jc[1][i] != 0 || jc[3][i] != 0;
    return __builtin_amdgcn_ballot_w64(varies) == 0;
  }
  // ... then the tensor without w_k once per item, ahead of the march and in the storage of jc; the layers take it as
  // it is (take_column) and w_k rides on the scale of the fluxes.  J is what take() forms with the slopes at zero, bit
  // for bit; against take() the six entries differ by where w_k multiplies.
  __device__ __forceinline__ void hoist_column()
  {
    static_assert(RCP);
    T J[3][3], g[6];
#pragma unroll
    for (int i = 0; i < 3; ++i)
    {
      J[i][0] = jc[0][i];
      J[i][1] = jc[2][i];
      J[i][2] = jc[4][i];
    }
    // (take()'s expressions, with its reciprocal and its guard: an empty slot still gives G = 0)
    T K[3][3], detJ;
    adjugate(J, K, detJ);
    T r = __builtin_amdgcn_rcp(detJ);
    r = fma(fma(-detJ, r, 1.0), r, r);
    r = fma(fma(-detJ, r, 1.0), r, r);
    metric(K, detJ > 0 ? r : 0, g);
#pragma unroll
    for (int i = 0; i < 3; ++i)
    {
      jc[0][i] = g[i];
      jc[1][i] = g[3 + i];
    }
  }
  __device__ __forceinline__ void take_column(T2& g01, T2& g23, T2& g45) const
  {
    static_assert(RCP);
    g01.x = jc[0][0], g01.y = jc[0][1];
    g23.x = jc[0][2], g23.y = jc[1][0];
    g45.x = jc[1][1], g45.y = jc[1][2];
  }
  __device__ __forceinline__ void fetch(int slot, int layer)
  {
    gq[slot][0] = gload<NT>(base + (lane_off + (unsigned)(layer * 3 * GPS)));
    gq[slot][1] = gload<NT>(base + (lane_off + (unsigned)(layer * 3 * GPS + GPS)));
    gq[slot][2] = gload<NT>(base + (lane_off + (unsigned)(layer * 3 * GPS + 2 * GPS)));
  }
  // layer k's three pairs (affine and trilinear cells: times `sc`), and the refill behind them
  __device__ __forceinline__ void take(int k, T sc, T2& g01, T2& g23, T2& g45)
  {
    if constexpr (AFF)
    {
      g01.x = sc * gc[0], g01.y = sc * gc[1];
      g23.x = sc * gc[2], g23.y = sc * gc[3];
      g45.x = sc * gc[4], g45.y = sc * gc[5];
    }
    else if constexpr (RCP)
    {
      const T z = zeta[k];
      T J[3][3], K[3][3], detJ, g[6];
#pragma unroll
      for (int i = 0; i < 3; ++i)
      {
        J[i][0] = jc[0][i] + z * jc[1][i];
        J[i][1] = jc[2][i] + z * jc[3][i];
        J[i][2] = jc[4][i];
      }
      adjugate(J, K, detJ);
      // 1 / |det J| from the hardware's estimate and two Newton steps: full precision for a normal determinant, without
      // the scaling and fix-up instructions of an IEEE division (the march is bound by its FP64 issue in this form).
      // (an empty slot: J = 0, and G = 0 as the stored tensor has it)
      T r = __builtin_amdgcn_rcp(detJ);
      r = fma(fma(-detJ, r, 1.0), r, r);
      r = fma(fma(-detJ, r, 1.0), r, r);
      metric(K, detJ > 0 ? sc * r : 0, g);
      g01.x = g[0], g01.y = g[1];
      g23.x = g[2], g23.y = g[3];
      g45.x = g[4], g45.y = g[5];
    }
    else if constexpr (FLAT)
    {
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj)
        gb[lane + 64 * jj] = gfl[jj]; // as loaded ...
      wave_fence();
      g01 = gb[lw]; // ... and as used: [pair][cell of the item][column]
      g23 = gb[WL + lw];
      g45 = gb[2 * WL + lw];
      if (k + 1 < ND)
      {
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj)
          gfl[jj] = gload<NT>(base + (k + 1) * LS + eo[jj]);
      }
    }
    else
    {
      g01 = gq[k % GD][0];
      g23 = gq[k % GD][1];
      g45 = gq[k % GD][2];
      if (k + GD < ND) // refill the slot with layer k + GD
        fetch(k % GD, k + GD);
    }
  }
};
} // namespace pmg
