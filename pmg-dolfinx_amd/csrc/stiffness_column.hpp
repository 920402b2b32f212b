// Private fragment of laplacian.hip, included there and nowhere else (inside its anonymous namespace, after
// geometry_kernels.hpp): Shape<P> and its policies, the write-back shared with the diagnostic stamps, and the column
// form of the stiffness kernel.  The layer march, the lane's table rows, the tensor stream, the fences and the loads
// are those of stiffness_layer.hpp, shared with the restrict, chain and FP32 kernels; what is written out here is the
// gather, the cell loop and the transposition by identity of P = 5 (P = 4 takes it beside the recomputed tensor, through
// layer_backward_identity of stiffness_layer.hpp).

template <int P>
struct Shape
{
  static constexpr int ND = P + 1;
  static constexpr int N = ND * ND * ND;
  static constexpr PatchShape PS = patch_shape(P);
  static constexpr int K = PS.bx * PS.by * PS.bz; // cells per patch
  static constexpr int MAXM = PS.max_m;           // patch dofs held in LDS
  // An item is CW whole cells worked on by WPC waves, a lane one (a, b) column of one of the cells.  Where nd^2 divides
  // 64 badly a wave per cell group idles many lanes (P = 5: 36 of 64, P = 8: 81 of 128); there four waves share an
  // item of 7 (P = 5: 252 of 256 lanes) or 3 (P = 8: 243 of 256) cells and exchange their slices through workgroup
  // barriers instead of wave-private fences -- worth it only with ONE item per workgroup, i.e. patches of exactly CW
  // cells (round 3, profiles/kernel_tuning_r03.md section 12: P = 5 532 -> 466 us, P = 8 495 -> 421; P = 4 and P = 6,
  // 78 % of the lanes busy, lose or gain nothing this way).
  static constexpr int NQ2 = ND * ND;
  static constexpr bool SHARED_ITEM = P == 5 || P == 8;
  static constexpr int CW = P == 5 ? 7 : P == 8 ? 3 : (NQ2 <= 64 ? 64 / NQ2 : 1);
  static constexpr int WPC = SHARED_ITEM ? 4 : (NQ2 + 63) / 64; // waves that share one item
  static_assert(CW * NQ2 <= 64 * WPC, "an item's columns need a lane each");
  static constexpr int ITEMS = (K + CW - 1) / CW;  // wave-items per full patch
  // measured (profiles/kernel_roofline_r01.md, profiles/kernel_tuning_r02.md): 4 waves and more
  // workgroups per CU for the register-heavy degrees and P = 3, 8 waves otherwise
  static constexpr int NWMAX = (P == 3 || P == 5 || P == 6 || P == 8) ? 4 : 8;
  static constexpr int NG = ITEMS < NWMAX / WPC ? ITEMS : NWMAX / WPC; // items in flight per workgroup
  static constexpr int NW = NG * WPC;                                  // waves per workgroup
  static constexpr int WTHREADS = NW * 64;
  static constexpr int WITER = (MAXM + WTHREADS - 1) / WTHREADS;
  static_assert(MAXM <= 65535, "patch positions are 16-bit");
};

// ---- write-back of a patch's sums, shared by the kernels below --------------------------------------------
// Round 4, read at the ISA level: written as one loop "load the list entry, branch on it, store", the write-back was six
// DEPENDENT round trips per thread -- `global_load_dword; s_waitcnt vmcnt(0); ... global_store` per entry, and since
// the counter retires in order every one of those waits also covered the acknowledgement of the previous entry's
// store.  So: the list entries are re-read in ONE pass of unconditional loads (clamped index), issued by every
// wavefront as it leaves the cell loop, BEFORE the barrier that ends the accumulation; behind the barrier the stores
// go out back to back; the rare Dirichlet rows (y = x, src/laplacian.hpp:273-274: one more load each) come last, in a
// pass of their own that interior patches skip.
template <int ITER, int THREADS>
__device__ __forceinline__ void patch_list_reload(uint32_t (&mk)[ITER], const uint32_t* __restrict__ pd, int M, int t)
{
#pragma unroll
  for (int k = 0; k < ITER; ++k)
  {
    const int i = t + k * THREADS;
    mk[k] = pd[i < M ? i : M - 1];
  }
}
template <int ITER, int THREADS, bool NT>
__device__ __forceinline__ void patch_write_back(const uint32_t (&mk)[ITER], int M, int t, const double* sy,
                                                 const double* __restrict__ x, double* __restrict__ y, int atomic_out)
{
  bool bc_row = false;
#pragma unroll
  for (int k = 0; k < ITER; ++k)
  {
    const int i = t + k * THREADS;
    const uint32_t dof = mk[k] & PD_MASK;
    const bool mine = i < M;
    if (mine && !(mk[k] & PD_BC))
    {
      const double v = sy[i];
      if (atomic_out)
        atomicAdd(&y[dof], v); // merged launch (global_atomic_add_f64)
      else if constexpr (NT)
        __builtin_nontemporal_store(v, &y[dof]);
      else
        y[dof] = v;
    }
    bc_row |= mine && (mk[k] & (PD_BC | PD_ACC)) == PD_BC;
  }
  if (__builtin_amdgcn_ballot_w64(bc_row) != 0) // wave-uniform: interior patches never enter
  {
#pragma unroll
    for (int k = 0; k < ITER; ++k)
    {
      const int i = t + k * THREADS;
      if (i < M && (mk[k] & (PD_BC | PD_ACC)) == PD_BC)
        y[mk[k] & PD_MASK] = x[mk[k] & PD_MASK]; // :273-274
    }
  }
}

// ---- diagnostic build only (-DPMG_STAMPS): where a wavefront spends its time -----------------------------------
// Every wavefront keeps up to eight readings of the constant 100 MHz clock (s_memrealtime: 10 ns ticks) in scalar
// registers and lane 0 stores them once, at its end, to a buffer of their own: [workgroup][wavefront][8].  No stamp
// executes in the product build; the timings of a stamped build are read for their SHARES only
// (cdna_hip_programming.md, In-kernel stamps).
#ifdef PMG_STAMPS
__device__ unsigned long long* g_stamp_buffer = nullptr;
__device__ int g_stamp_capacity = 0; // workgroups the buffer has room for
#define PMG_STAMP_DECL unsigned long long stamp_[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define PMG_STAMP(i)                                                                                                  \
  do                                                                                                                  \
  {                                                                                                                   \
    __builtin_amdgcn_sched_barrier(0);                                                                                \
    stamp_[i] = __builtin_amdgcn_s_memrealtime();                                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                                                \
  } while (0)
#define PMG_STAMP_FLUSH(nwaves)                                                                                       \
  do                                                                                                                  \
  {                                                                                                                   \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); /* 7: the stores of the write-back are acknowledged */            \
    PMG_STAMP(7);                                                                                                     \
    if ((threadIdx.x & 63) == 0 && g_stamp_buffer && (int)blockIdx.x < g_stamp_capacity)                              \
      for (int i_ = 0; i_ < 8; ++i_)                                                                                  \
        g_stamp_buffer[((size_t)blockIdx.x * (nwaves) + (threadIdx.x >> 6)) * 8 + i_] = stamp_[i_];                   \
  } while (0)
#else
#define PMG_STAMP_DECL
#define PMG_STAMP(i)
#define PMG_STAMP_FLUSH(nwaves)
#endif

// ---- the hot kernel, column form --------------------------------------
//
// One workgroup per patch, NW wavefronts.  Phase 0 / write-back as in the block
// kernel.  In between every wavefront works on its own: it takes CW whole cells
// (2 at P = 4), a lane owns the column of nd points above (a, b), keeps the
// column's dofs and results in registers and marches through the nd layers
// (the register-blocked 2-D scheme of libParanumal / hipBone).  Per layer the x
// and y contractions exchange one nd x nd slice through a wave-private LDS
// region -- LDS executes a wave's instructions in order, so no s_barrier and no
// waitcnt is needed inside the cell loop, only a compiler fence; the z
// contraction stays in registers with wave-uniform table entries (scalar loads).
// A cell costs 4*nd LDS reads per point instead of 12*nd, the 1-D tables for the
// lane's a and b sit in registers, and the layer-(k+1) slice of G is in flight
// while layer k is computed.
// P = 5 and P = 8 read their slices one by one (slice_load, stiffness_layer.hpp)
constexpr bool unpaired_slice_reads(int P) { return P == 5 || P == 8; }

// degrees whose kernel keeps the patch's dof list in LDS for the write-back (4 bytes per patch dof).  Round 4, two
// rounds on one box against the list re-read from global memory: P = 5 454 against 460 - 470 us, P = 7 368 - 372 against
// 376, P = 8 410 - 411 against 420; P = 4 +0.5 % (within noise, left out); P = 6 474 - 482 against 441 - 445 (the 9.6 KB
// cost it a workgroup per CU).
constexpr bool list_in_lds(int P) { return P == 5 || P == 7 || P == 8; }
// ---- the transposed table without its registers (round 4) ----
// The transposed table by an identity.  For Lagrange polynomials on ANY distinct nodes D_ij = (l_j / l_i) /
// (x_i - x_j), i != j, with the barycentric weights l, hence D_ji = -(l_i / l_j)^2 D_ij and
//     (D^T f)_i = 2 D_ii f_i - rho_i sum_j D_ij (f_j / rho_j),       rho_i = (l_i / l_0)^2 = -D_0i / D_i0,
// i.e. the backward contraction is the FORWARD one applied to the scaled fluxes: the five registers of D[.][a] (and
// the nine shift coefficients a DPP direction would need for its transpose) become rho, 1 / rho and 2 D_ii.  Same
// value to rounding (tests: 1e-12 against the oracle), not bit for bit.  Both directions still go through their LDS
// slices (the y contractions as DPP row shifts were measured and removed: profiles/dpp_identity_r04.txt).
// P = 5 is the one degree where the identity pays: 129 registers instead of 164, and asked for four wavefronts per SIMD
// the allocator finds 128 without a spill -- four workgroups per unit instead of three (33 KB of LDS each): 432 - 444
// against 452 - 459 us at 51^3, 223 - 225 against 230 - 232 us at 40^3 (profiles/kernel_tuning_r04.md section 12).
// P = 4 takes the identity in the recomputed form only (GEO_RECOMPUTE, stiffness_layer.hpp): there the lane holds the 15
// values of its column's Jacobian beside the march, and the ten registers of DTa, DTb are what does not fit -- with them
// the column kernel spills 62 registers at 128, with rho, 1 / rho in their place none (profiles/tensor_recompute_p4.md).
// The streamed and the affine kernel of P = 4 keep their tables: their code objects are unchanged.
constexpr bool transposes_by_identity(int P, int GEO) { return P == 5 || (P == 4 && GEO == GEO_RECOMPUTE); }
// Degrees whose recomputed form has the column-constant branch (TensorStream::column_constant, stiffness_layer.hpp; the
// fused kernels follow their fine degree).  Degree 1 is left out by measurement: two layers per column leave one tensor
// to save, and with the branch its kernel was 2 us per cycle slower on a mesh where every item takes it (20.0 against
// 19.1 us per launch, profiles/column_tensor.md) -- it keeps the code object it had.
constexpr bool column_branch(int P) { return P == 2 || P == 4; }
// minimum waves per SIMD the register allocation has to leave room for: two workgroups per CU up to
// P = 4; the register-heavy degrees take what they need (profiles/kernel_resources_r02.md)
template <int P, int GEO>
constexpr int min_waves_per_simd()
{
  // (P = 5 with the identity: the allocator lands on 129 registers; asked for four wavefronts per SIMD it has to find 128)
  return P <= 4 ? (2 * Shape<P>::NW + 3) / 4 : transposes_by_identity(P, GEO) ? 4 : 1;
}
// GEO: where the tensor comes from (stiffness_layer.hpp).  Gcell: the per-slot data of the two forms without a stream,
// [slot][6] constant tensors (GEO_AFFINE) or [slot][24] trilinear coefficients (GEO_RECOMPUTE).  W1 [2][nd] + 1: the 1-D
// GLL weights, then the nodes, then the switch of the column-constant branch (non-zero = on).
template <int P, int GEO, bool NT>
__global__ void __launch_bounds__(Shape<P>::WTHREADS, (min_waves_per_simd<P, GEO>()))
    stiffness_column_kernel(const double* __restrict__ x, double* __restrict__ y,
                            const double2* __restrict__ G, const double* __restrict__ Gcell,
                            const double* __restrict__ W1, const int32_t* __restrict__ poff,
                            const uint32_t* __restrict__ pdofs,
                            const int32_t* __restrict__ lmap_id,
                            const uint16_t* __restrict__ lmaps, const int32_t* __restrict__ pcell,
                            const int32_t* __restrict__ pncell, const double* __restrict__ kappa,
                            const double* __restrict__ Dg, const double* __restrict__ react, int first,
                            int atomic_out)
{
  using Sh = Shape<P>;
  constexpr int ND = Sh::ND, N = Sh::N, K = Sh::K, NQ2 = Sh::NQ2, CW = Sh::CW, NG = Sh::NG, WPC = Sh::WPC;
  constexpr int MAXM = Sh::MAXM, THREADS = Sh::WTHREADS, ITER = Sh::WITER;
  constexpr int WL = CW * NQ2; // columns of one item (a wave, or WPC waves sharing a cell)
  // NT: streaming cache policy for G and the y write-back (chosen per operator, launch_stiffness)
  constexpr bool AFF = GEO == GEO_AFFINE, RCP = GEO == GEO_RECOMPUTE;
  static_assert(!RCP || WPC == 1, "the recomputed form covers the one-wave-per-item shapes only");
  constexpr bool UNPAIRED = unpaired_slice_reads(P);
  constexpr bool SHARED = WPC > 1; // the item's wavefronts exchange their slices through workgroup barriers
  __shared__ double sD[ND * ND];
  __shared__ double skap[K];
  __shared__ double sx[MAXM];
  __shared__ double sy[MAXM];
  // The patch's dof list, kept for the write-back (round 4): under load a dependent global load costs ~2 us even when
  // it hits in L2 (in-kernel stamps, profiles/kernel_tuning_r04.md), and re-reading the list was one such round trip
  // per workgroup behind its closing barrier.
  constexpr bool LIST_IN_LDS = list_in_lds(P);
  __shared__ uint32_t sm[LIST_IN_LDS ? MAXM : 1];
  // (recomputed form: the three slices of every item in flight in ONE array, one address register, as the restrict
  // kernel has them)
  __shared__ double sq[(RCP ? 3 : 1) * NG * WL];
  __shared__ double sgr[RCP ? 1 : NG * WL];
  __shared__ double sgs[RCP ? 1 : NG * WL];
  // flat G layout: one layer of the item, as loaded (NJ x 64 double2), for the hand-over to the lanes
  constexpr bool FLAT = GEO == GEO_STORED && WPC == 1 && gflat(ND);
  constexpr int FL = 3 * WL, NJ = (FL + 63) / 64, LS = gls(ND);
  __shared__ double2 sgb[FLAT ? NG * NJ * 64 : 1];

  PMG_STAMP_DECL;
  PMG_STAMP(0); // entry
  const int p = first + blockIdx.x;
  const int t = threadIdx.x;
  const int off = poff[p];
  const int M = poff[p + 1] - off; // 1 <= M <= MAXM
  const int table = lmap_id[p];
  const int nc = pncell[p];

  // ---- phase 0: gather (unconditional loads, clamped indices: counted vmcnt waits)
  {
    uint32_t m[ITER];
#pragma unroll
    for (int k = 0; k < ITER; ++k)
    {
      const int i = t + k * THREADS;
      m[k] = pdofs[off + (i < M ? i : M - 1)];
    }
    const int cellk = pcell[(size_t)p * K + (t < K ? t : K - 1)];
    const double dval = Dg[t < ND * ND ? t : ND * ND - 1];
    double xv[ITER], yv[ITER];
#pragma unroll
    for (int k = 0; k < ITER; ++k)
    {
      const uint32_t dof = m[k] & PD_MASK;
      const bool acc = !atomic_out && (m[k] & (PD_ACC | PD_BC)) == PD_ACC;
      xv[k] = x[dof];
      // (an entry that does not accumulate loads all the same: the reaction vector where the operator has one --
      // `react` is a kernel argument, the branch wave-uniform -- and otherwise x again, an L2-hot dummy)
      const double* ya = acc ? (const double*)(y + dof) : react ? (react + dof) : (x + dof);
      yv[k] = *ya;
    }
    const double kapk = kappa[cellk >= 0 ? cellk : 0];
#pragma unroll
    for (int k = 0; k < ITER; ++k)
    {
      const int i = t + k * THREADS;
      if (i < M)
      {
        const bool acc = !atomic_out && (m[k] & (PD_ACC | PD_BC)) == PD_ACC;
        sx[i] = (m[k] & PD_BC) ? 0.0 : xv[k]; // src/laplacian.hpp:186-189
        // the dof's FIRST patch (PD_ACC clear, in coloured and merged launches alike: patches.hpp) starts its sum at
        // the reaction term react[dof] * x[dof]; Dirichlet rows carry none (y = x)
        const bool starts = react && !(m[k] & (PD_ACC | PD_BC));
        sy[i] = acc ? yv[k] : starts ? yv[k] * xv[k] : 0.0;
        if constexpr (LIST_IN_LDS)
          sm[i] = m[k];
      }
    }
    if (t < ND * ND)
      sD[t] = dval;
    for (int i = t; i < K; i += THREADS)
      skap[i] = (i == t) ? kapk : kappa[pcell[(size_t)p * K + i] >= 0 ? pcell[(size_t)p * K + i] : 0];
  }
  PMG_STAMP(1); // gathered values written to LDS
  lds_barrier();
  PMG_STAMP(2); // behind the gather's barrier

  // ---- cell loop: each wave on its own
  // (nd^2 > 64, i.e. P = 8: WPC waves share a cell, the slices are exchanged between
  // them, so the fences inside the layer loop become workgroup barriers and every
  // wave runs the same number of items)
  const int wave = (t >> 6) / WPC, lane = (t & 63) + 64 * ((t >> 6) % WPC);
  constexpr bool IDT = transposes_by_identity(P, GEO);
  // the lanes past the item's columns idle on a copy of the last column
  const bool lane_ok = lane < WL;
  const int lw = lane_ok ? lane : WL - 1;
  const int cw = lw / NQ2;          // cell of this lane inside the wave item
  const int ab = lw - cw * NQ2;     // column: a = x index, b = y index
  const int a = ab / ND, b = ab - a * ND;
  LaneTables<double, ND> T;
  T.fill((const __attribute__((address_space(3))) double*)sD, a, b);
  // the identity's constants (see transposes_by_identity): rho, 1 / rho, 2 D_ii for the lane's a and b
  // (beside the recomputed tensor 2 D_ii is not held: layer_backward_identity picks it per layer)
  double rho_a = 1.0, irho_a = 1.0, d2a = 0.0, rho_b = 1.0, irho_b = 1.0, d2b = 0.0;
  if constexpr (IDT)
  {
    rho_a = a == 0 ? 1.0 : -sD[a] / sD[a * ND];
    rho_b = b == 0 ? 1.0 : -sD[b] / sD[b * ND];
    irho_a = 1.0 / rho_a;
    irho_b = 1.0 / rho_b;
    d2a = 2.0 * sD[a * ND + a];
    d2b = 2.0 * sD[b * ND + b];
  }
  const double wab = AFF ? W1[a] * W1[b] : 0.0; // 1-D GLL weights of the lane's column
  double* q_s = sq + wave * WL + cw * NQ2;  // this cell's slices
  double* gr_s = RCP ? q_s + NG * WL : sgr + wave * WL + cw * NQ2;
  double* gs_s = RCP ? q_s + 2 * NG * WL : sgs + wave * WL + cw * NQ2;
  double* gr_w = gr_s + ab; // where the lane writes its x flux (the identity path of P = 5)
  const int items = WPC > 1 ? (((nc + CW - 1) / CW + NG - 1) / NG) * NG : (nc + CW - 1) / CW;

  for (int it = wave; it < items; it += NG)
  {
#ifdef PMG_STAMPS
    if (it >= wave + NG)
      PMG_STAMP(3); // first item done (overwritten by later items: the start of the LAST item)
#endif
    const int slot = it * CW + cw;
    const int slotc = slot < K ? slot : K - 1;
    // (scalar bases + 32-bit lane offsets: a 64-bit per-lane pointer costs two registers, and a spilled one is reloaded
    // behind a wait that drains the memory counter)
    const uint16_t* lmb = lmaps + (size_t)table * (K * N);
    const unsigned lmo = (unsigned)(slotc * N + ab);
    int l[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k)
      l[k] = lmb[lmo + (unsigned)(k * NQ2)];
    // the tensor, one layer ahead of the march (affine cells: G_q = w_a w_b w_c * Gc, one constant tensor Gc per cell)
    // (trilinear cells: formed in the march from the cell's coefficients and the column's (xi_a, eta_b))
    TensorStream<double2, ND, WL, GEO, FLAT, LS, NT, 1> gs;
    if constexpr (AFF)
      gs.prime_affine(Gcell + ((size_t)p * K + slotc) * 6, 1.0);
    else if constexpr (RCP)
    {
      // (the column's weights and nodes are read per item, from an opaque copy of the column index: held through the
      // layer loop they are six registers the march has no room for)
      int abv = ab;
      asm volatile("" : "+v"(abv));
      const int av = abv / ND, bv = abv - av * ND;
      gs.prime_recompute(Gcell + ((size_t)p * K + slotc) * 24, W1[ND + av], W1[ND + bv], W1[av] * W1[bv], W1 + ND);
    }
    else if constexpr (FLAT) // (the item index is wave-uniform: a scalar base plus 32-bit lane offsets)
      gs.prime_flat(G + (size_t)p * gpatch(ND, K) + (size_t)__builtin_amdgcn_readfirstlane(it) * ND * LS,
                    sgb + wave * (NJ * 64), lane, lw);
    else
      gs.prime(G + (size_t)p * ((long long)K * 3 * N), (unsigned)(slotc * 3 * N + ab));
    // (identity modes: kappa multiplies the cell's INPUT once -- the operator is linear in it, same value to rounding --
    // and the positions are held two to a register through the layer loop; so they are in the recomputed form)
    const double kap = IDT ? 1.0 : skap[slotc];
    double u[ND], Aq[ND];
    {
      const double kin = IDT ? skap[slotc] : 1.0;
#pragma unroll
      for (int k = 0; k < ND; ++k)
      {
        u[k] = IDT ? kin * sx[l[k]] : sx[l[k]];
        Aq[k] = 0.0;
      }
    }
    unsigned lp[IDT || RCP ? (ND + 1) / 2 : 1];
    if constexpr (IDT || RCP)
      pack_positions(l, lp);
    // Recomputed tensor: the wavefront decides for its item whether J is constant down every column (column_constant),
    // outside the unrolled loop (inside it every layer holds both forms' operands).  hoisted: the item's tensor is formed
    // once, ahead of the loop and without w_k, which multiplies the fluxes instead (beside the identity kap is the
    // constant 1: no instruction more); otherwise the march is the one below.  The switch of the branch
    // (pmg_laplacian_set_column_tensor) is one more entry of W1, behind the weights and the nodes: a scalar load per
    // item from an array the march reads anyway, no kernel argument held through the loop (the null-ness of G, tried
    // first, cost the degree-4 kernels 44 and 56 bytes of scratch).
    if constexpr (RCP && column_branch(P))
    {
      auto march = [&](auto hoisted) {
#pragma unroll
        for (int k = 0; k < ND; ++k)
        {
          double2 g01, g23, g45;
          if constexpr (decltype(hoisted)::value)
            gs.take_column(g01, g23, g45);
          else
            gs.take(k, W1[k], g01, g23, g45);
          double fr, fs, ft;
          layer_forward<ND, UNPAIRED, SHARED>(k, u, T, Dg, q_s, a, b, ab, g01, g23, g45,
                                              decltype(hoisted)::value ? kap * W1[k] : kap, fr, fs, ft);
          if constexpr (IDT)
            layer_backward_identity<ND, UNPAIRED, SHARED>(k, fr, fs, ft, T, Dg, gr_s, gs_s, a, b, ab, rho_a, irho_a,
                                                          rho_b, irho_b, Aq);
          else
            layer_backward<ND, UNPAIRED, SHARED>(k, fr, fs, ft, T, Dg, gr_s, gs_s, a, b, ab, Aq);
        }
      };
      if (W1[2 * ND] != 0.0 && gs.column_constant())
      {
        gs.hoist_column();
        march(std::true_type{});
      }
      else
        march(std::false_type{});
    }
    else
    {
#pragma unroll
    for (int k = 0; k < ND; ++k)
    {
      double2 g01, g23, g45;
      // w_a w_b w_c; W1[k] is wave-uniform (scalar load)
      gs.take(k, AFF ? wab * W1[k] : RCP ? W1[k] : 0.0, g01, g23, g45);
      double fr, fs, ft;
      layer_forward<ND, UNPAIRED, SHARED>(k, u, T, Dg, q_s, a, b, ab, g01, g23, g45, kap, fr, fs, ft);
      if constexpr (IDT)
      {
        // the transposes as forward contractions of the scaled fluxes (see transposes_by_identity)
        *gr_w = fr * irho_a;
        gs_s[ab] = fs * irho_b;
        slice_sync<SHARED>();
        double sx_ = 0.0, sy_ = 0.0;
#pragma unroll
        for (int mm = 0; mm < ND; ++mm)
        {
          sx_ += T.Da[mm] * slice_load<UNPAIRED>(gr_s[mm * ND + b]); // :246-251
          sy_ += T.Db[mm] * slice_load<UNPAIRED>(gs_s[a * ND + mm]); // :255-259
          Aq[mm] += Dg[k * ND + mm] * ft;                            // :263-267
        }
        Aq[k] += (d2a * fr + d2b * fs) - (rho_a * sx_ + rho_b * sy_);
        slice_sync<SHARED>();
      }
      else
        layer_backward<ND, UNPAIRED, SHARED>(k, fr, fs, ft, T, Dg, gr_s, gs_s, a, b, ab, Aq);
    }
    }
    // Every lane adds (no branch: a conditional here lets the compiler sink the
    // whole accumulation into it and keep every layer's operands live); lanes
    // without a cell (idle lanes, slots past the patch's cells -- their indices
    // were clamped onto a real slot) add an exact zero.  The sum is read AHEAD of the select: written
    // `contributes ? Aq[k] : 0.0` the read itself is conditional, and since the layer functions take Aq by reference
    // it stays a branch until they are inlined -- into which the accumulation is then sunk (spills at P = 4, 5 affine).
    const bool contributes = lane_ok && slot < nc;
#pragma unroll
    for (int k = 0; k < ND; ++k)
    {
      const int lk = IDT || RCP ? (int)packed_position(lp, k) : l[k];
      const double Ak = Aq[k];
      atomicAdd(&sy[lk], contributes ? Ak : 0.0); // :270,277 -- in LDS (ds_add_f64)
    }
  }
  // ---- write back (plain stores; the accumulator started from the earlier colours' y)
  {
    // (the thread index made opaque here: otherwise the list addresses are computed ahead of the cell loop and
    // held -- or spilled -- through it)
    PMG_STAMP(4); // cell loop done
    int tw = t;
    asm volatile("" : "+v"(tw));
    uint32_t mk[ITER];
    if constexpr (!LIST_IN_LDS)
      patch_list_reload<ITER, THREADS>(mk, pdofs + off, M, tw);
    lds_barrier();
    if constexpr (LIST_IN_LDS)
    {
#pragma unroll
      for (int k = 0; k < ITER; ++k)
        mk[k] = sm[tw + k * THREADS < M ? tw + k * THREADS : M - 1];
    }
    PMG_STAMP(5); // behind the barrier that ends the accumulation
    patch_write_back<ITER, THREADS, NT>(mk, M, tw, sy, x, y, atomic_out);
    PMG_STAMP(6); // stores issued
    PMG_STAMP_FLUSH(Sh::NW);
  }
}
