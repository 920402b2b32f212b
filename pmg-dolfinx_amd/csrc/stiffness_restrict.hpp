// Private fragment of laplacian.hip, included there and nowhere else (inside its anonymous namespace, after
// stiffness_column.hpp): the operator application fused with the restriction of the residual it would feed.
//
// The last application of a pre-smooth, q = A z, is written to memory, read back once by the restriction as r - q and
// never used again.  The restriction is linear and, for conforming spaces, additive over cells: P[f, c] is the same
// from every cell that holds the fine dof f and zero for every coarse dof outside those cells, so
//     P^T (r - A z) = sum over cells  P_cell^T (r|cell / mult - A_cell z)          (mult: cells that hold the dof).
// The patch workgroup of the apply therefore restricts each cell's own contribution straight from its registers: it
// never sums into the fine output, never writes q and never waits on a colour -- all patches of the operator go in ONE
// launch.  On Dirichlet rows the apply's rule is q = z (stiffness_column.hpp, patch_write_back), so their share is
// (r - z) / mult and the cell's product is dropped there.  A reaction term (pmg_laplacian_set_reaction) is diagonal,
// and so is a Robin term (pmg_laplacian_set_robin; the two arrive summed in one vector):
// r - (A + D) z = (r - d z) - A z, so the unmarked rows' share is (r - d z) / mult and nothing else moves.
//
// The gather and the cell loop follow stiffness_column_kernel (WPC == 1 shapes; the transposition identity at P = 4 with
// the recomputed tensor only); the
// layer march, the lane's table rows, the tensor stream and the packed positions are the shared ones of
// stiffness_layer.hpp.  `sy` holds the residual shares instead of the output sums.  Behind the layer
// loop the lane owns w(a, b, .) = share - A_cell z of its column: z is contracted in registers with the 1-D
// interpolation table M1 (wave-uniform entries), x and y through the wave's slice arrays, and the (PC + 1)^3 results
// are added to an LDS accumulator over the patch's coarse dofs, which goes to the coarse vector with one atomic per
// patch coarse dof, as restrict_patch_kernel does (interpolate.hip).
template <int P, int PC>
struct RestrictShape
{
  using Sh = Shape<P>;
  static_assert(Sh::WPC == 1, "the fused form covers the one-wave-per-item shapes only");
  static constexpr int NDC = PC + 1, NC = NDC * NDC * NDC;
  static constexpr int CM = Sh::K * NC < Sh::MAXM ? Sh::K * NC : Sh::MAXM; // coarse dofs of a patch: never more
  static constexpr int CITER = (CM + Sh::WTHREADS - 1) / Sh::WTHREADS;
  static constexpr int BCW = Sh::WITER * Sh::WTHREADS / 64; // 64-bit words of the Dirichlet bit map
};

// the coarse side of a patched transfer, as the kernel reads it (TransferView, patches.hpp)
struct RestrictLists
{
  const int32_t *cpoff, *clmap_id;
  const uint32_t* cpdofs;
  const uint16_t* clmaps;
  const uint8_t* pmult;
  const double* M1; // [P + 1][PC + 1]
};

// waves per SIMD the allocation has to leave room for: the column kernel's, with two exceptions.  P = 2: the coarse
// sums push the workgroup past 80 KB of LDS, so one workgroup per CU is what runs.  P = 3: asked for the four the
// column kernel reaches, the allocation stays at 128 registers instead of 129.  (P = 6, asked for the column kernel's
// three: spills.)  The recomputed form at P = 2 has no hand-over buffer for the flat layout: two workgroups fit again.
template <int P, int GEO>
constexpr int restrict_waves_per_simd()
{
  return P == 2 ? (GEO == GEO_RECOMPUTE ? 4 : 2) : P == 3 ? 4 : min_waves_per_simd<P, GEO>();
}

// (GEO, Gcell, W1: as in stiffness_column_kernel)
template <int P, int PC, int GEO, bool NT>
__global__ void __launch_bounds__(Shape<P>::WTHREADS, (restrict_waves_per_simd<P, GEO>()))
    stiffness_restrict_kernel(const double* __restrict__ z, const double* __restrict__ r, double* __restrict__ coarse,
                              const double2* __restrict__ G, const double* __restrict__ Gcell,
                              const double* __restrict__ W1, const int32_t* __restrict__ poff,
                              const uint32_t* __restrict__ pdofs, const int32_t* __restrict__ lmap_id,
                              const uint16_t* __restrict__ lmaps, const int32_t* __restrict__ pcell,
                              const int32_t* __restrict__ pncell, const double* __restrict__ kappa,
                              const double* __restrict__ Dg, const double* __restrict__ react, RestrictLists R)
{
  using Sh = Shape<P>;
  using Rs = RestrictShape<P, PC>;
  constexpr int ND = Sh::ND, N = Sh::N, K = Sh::K, NQ2 = Sh::NQ2, CW = Sh::CW, NG = Sh::NG;
  constexpr int MAXM = Sh::MAXM, THREADS = Sh::WTHREADS, ITER = Sh::WITER;
  constexpr int NDC = Rs::NDC, NC = Rs::NC, CM = Rs::CM, CITER = Rs::CITER;
  constexpr int WL = CW * NQ2;
  constexpr bool UNPAIRED = unpaired_slice_reads(P);
  constexpr bool AFF = GEO == GEO_AFFINE, RCP = GEO == GEO_RECOMPUTE;
  __shared__ double sD[ND * ND];
  __shared__ double sM[ND * NDC];
  // (P = 4 with the recomputed tensor: the transposes by identity, as in the column kernel)
  constexpr bool IDT = transposes_by_identity(P, GEO);
  // affine mode: the 1-D weights, read per item instead of held per lane; identity: 1 / rho_i, read per layer
  __shared__ double sW[AFF || IDT ? ND : 1];
  __shared__ double skap[K];
  __shared__ double sx[MAXM];
  __shared__ double sy[MAXM]; // the residual shares r / mult ((r - z) / mult on Dirichlet rows)
  __shared__ double sc[CM];   // the patch's coarse sums
  __shared__ unsigned long long sbc[Rs::BCW]; // bit i: patch entry i is a Dirichlet row
  __shared__ double ssl[3 * NG * WL]; // the three slices of every item in flight, in ONE array: one address register
  constexpr bool FLAT = GEO == GEO_STORED && gflat(ND);
  constexpr int FL = 3 * WL, NJ = (FL + 63) / 64, LS = gls(ND);
  __shared__ double2 sgb[FLAT ? NG * NJ * 64 : 1];

  const int p = blockIdx.x;
  const int t = threadIdx.x;
  const int off = poff[p];
  const int M = poff[p + 1] - off; // 1 <= M <= MAXM
  const int table = lmap_id[p];
  const int nc = pncell[p];
  const int ctable = __builtin_amdgcn_readfirstlane(R.clmap_id[p]);
  const int coff = R.cpoff[p];
  const int Mc = R.cpoff[p + 1] - coff; // 1 <= Mc <= CM

  // ---- phase 0: gather (unconditional loads, clamped indices)
  {
    uint32_t m[ITER];
    uint8_t mu[ITER];
#pragma unroll
    for (int k = 0; k < ITER; ++k)
    {
      const int i = t + k * THREADS;
      const int ic = off + (i < M ? i : M - 1);
      m[k] = pdofs[ic];
      mu[k] = R.pmult[ic];
    }
    const int cellk = pcell[(size_t)p * K + (t < K ? t : K - 1)];
    const double dval = Dg[t < ND * ND ? t : ND * ND - 1];
    const double mval = R.M1[t < ND * NDC ? t : ND * NDC - 1];
    double zv[ITER], rv[ITER];
#pragma unroll
    for (int k = 0; k < ITER; ++k)
    {
      const uint32_t dof = m[k] & PD_MASK;
      zv[k] = z[dof];
      rv[k] = r[dof];
    }
    const double kapk = kappa[cellk >= 0 ? cellk : 0];
#pragma unroll
    for (int k = 0; k < ITER; ++k)
    {
      const int i = t + k * THREADS;
      const bool bc = i < M && (m[k] & PD_BC);
      if (i < M)
      {
        sx[i] = bc ? 0.0 : zv[k];                                   // src/laplacian.hpp:186-189
        sy[i] = (bc ? rv[k] - zv[k] : rv[k]) / (double)mu[k];       // src/interpolate.hpp:81-82
      }
      // reaction term (wave-uniform branch on the kernel argument): the residual is r - (A + D) z = (r - d z) - A z.
      // Every cell that holds the dof adds its share once, in whichever patch it lies, so the diagonal part is
      // spread like r itself: the share of an unmarked row becomes (r - d z) / mult in every patch -- not a start
      // value of the dof's first patch as in the column kernel, whose accumulator is per dof where this one is per
      // cell.  Loaded here, behind the other gathers, so that no third array of registers is held.
      if (react)
      {
        const double dv = react[m[k] & PD_MASK];
        if (i < M && !bc)
          sy[i] = (rv[k] - dv * zv[k]) / (double)mu[k];
      }
      const unsigned long long rows = __builtin_amdgcn_ballot_w64(bc); // the wave's entries are i & ~63 .. + 63
      if ((t & 63) == 0)
        sbc[i >> 6] = rows;
    }
    if (t < ND * ND)
      sD[t] = dval;
    if (t < ND * NDC)
      sM[t] = mval;
    if constexpr (AFF)
    {
      if (t < ND)
        sW[t] = W1[t];
    }
    if constexpr (IDT) // 1 / rho_i = -D_i0 / D_0i
    {
      if (t < ND)
        sW[t] = t == 0 ? 1.0 : -Dg[t * ND] / Dg[t];
    }
    for (int i = t; i < K; i += THREADS)
      skap[i] = (i == t) ? kapk : kappa[pcell[(size_t)p * K + i] >= 0 ? pcell[(size_t)p * K + i] : 0];
    for (int i = t; i < CM; i += THREADS)
      sc[i] = 0.0;
  }
  lds_barrier();

  // ---- cell loop: each wave on its own (stiffness_column_kernel)
  const int wave = t >> 6, lane = t & 63;
  const bool lane_ok = lane < WL;
  const int lw = lane_ok ? lane : WL - 1;
  const int cw = lw / NQ2;
  const int ab = lw - cw * NQ2;
  const int a = ab / ND, b = ab - a * ND;
  LaneTables<double, ND> T;
  T.fill((const __attribute__((address_space(3))) double*)sD, a, b);
  // the identity's rho for the lane's a and b (1 / rho is read per layer from sW: the kernel has no registers for it)
  double rho_a = 1.0, rho_b = 1.0;
  if constexpr (IDT)
  {
    rho_a = a == 0 ? 1.0 : -sD[a] / sD[a * ND];
    rho_b = b == 0 ? 1.0 : -sD[b] / sD[b * ND];
  }
  double* q_s = ssl + wave * WL + cw * NQ2; // this cell's slices
  double* gr_s = q_s + NG * WL;
  double* gs_s = q_s + 2 * NG * WL;
  // the lane's coarse point (i, j) = (a, b) of a layer; lanes past the coarse points idle on a copy of the last one
  // (worked out again from an opaque copy of the column index wherever they are needed: two integer operations
  // instead of registers held through the layer loop -- or spilled there)
  const bool coarse_ok = lane_ok && a < NDC && b < NDC;
  auto coarse_point = [](int abv, int& i, int& j, int bound) {
    asm volatile("" : "+v"(abv));
    const int av = abv / ND, bv = abv - av * ND;
    i = av < bound ? av : bound - 1;
    j = bv < bound ? bv : bound - 1;
  };
  const int items = (nc + CW - 1) / CW;

  for (int it = wave; it < items; it += NG)
  {
    const int slot = it * CW + cw;
    const int slotc = slot < K ? slot : K - 1;
    const uint16_t* lmb = lmaps + (size_t)table * (K * N);
    const unsigned lmo = (unsigned)(slotc * N + ab);
    int l[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k)
      l[k] = lmb[lmo + (unsigned)(k * NQ2)];
    // where the lane's coarse results go (plain t order: (i * ndc + j) * ndc + k), requested with the fine positions
    const uint16_t* clb = R.clmaps + (size_t)ctable * (K * NC);
    int ic, jc;
    coarse_point(ab, ic, jc, NDC);
    const unsigned clo = (unsigned)(slotc * NC + (ic * NDC + jc) * NDC);
    // (held two to a register through the layer loop, and opaque, so that the unpacked values are not kept alongside)
    int lc[NDC];
#pragma unroll
    for (int k = 0; k < NDC; ++k)
      lc[k] = clb[clo + (unsigned)k];
    unsigned lcp[(NDC + 1) / 2];
    pack_positions(lc, lcp);
    TensorStream<double2, ND, WL, GEO, FLAT, LS, NT, 1> gs;
    if constexpr (AFF)
    {
      // (kappa and the column's weights w_a w_b folded into the cell's constant tensor: same value to rounding; the
      // layer's weight w_c scales the three fluxes)
      int av, bv;
      coarse_point(ab, av, bv, ND);
      gs.prime_affine(Gcell + ((size_t)p * K + slotc) * 6, skap[slotc] * (sW[av] * sW[bv]));
    }
    else if constexpr (RCP)
    {
      // (the column's weights and nodes read per item, as the affine mode's weights; kappa scales the fluxes)
      int av, bv;
      coarse_point(ab, av, bv, ND);
      gs.prime_recompute(Gcell + ((size_t)p * K + slotc) * 24, W1[ND + av], W1[ND + bv], W1[av] * W1[bv], W1 + ND);
    }
    else if constexpr (FLAT)
      gs.prime_flat(G + (size_t)p * gpatch(ND, K) + (size_t)__builtin_amdgcn_readfirstlane(it) * ND * LS,
                    sgb + wave * (NJ * 64), lane, lw);
    else
      gs.prime(G + (size_t)p * ((long long)K * 3 * N), (unsigned)(slotc * 3 * N + ab));
    // (identity: kappa multiplies the cell's input once, as in the column kernel -- same value to rounding)
    const double kap = AFF || IDT ? 1.0 : skap[slotc];
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
    // (the fine positions as well: the epilogue needs them again)
    unsigned lp[(ND + 1) / 2];
    pack_positions(l, lp);
    // (recomputed tensor: the item's tensor once, ahead of the loop, where J is constant down its columns; the switch
    // is W1's last entry -- as in the column kernel)
    if constexpr (RCP)
    {
      static_assert(column_branch(P), "a fused pair with the recomputed form and no column-constant branch");
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
          layer_forward<ND, UNPAIRED, false>(k, u, T, Dg, q_s, a, b, ab, g01, g23, g45,
                                             decltype(hoisted)::value ? kap * W1[k] : kap, fr, fs, ft);
          if constexpr (IDT)
          {
            int av, bv;
            coarse_point(ab, av, bv, ND);
            layer_backward_identity<ND, UNPAIRED, false>(k, fr, fs, ft, T, Dg, gr_s, gs_s, a, b, ab, rho_a, sW[av],
                                                         rho_b, sW[bv], Aq);
          }
          else
            layer_backward<ND, UNPAIRED, false>(k, fr, fs, ft, T, Dg, gr_s, gs_s, a, b, ab, Aq);
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
      gs.take(k, 1.0, g01, g23, g45);
      double fr, fs, ft;
      // (affine cells: W1[k] is wave-uniform, a scalar load)
      layer_forward<ND, UNPAIRED, false>(k, u, T, Dg, q_s, a, b, ab, g01, g23, g45, AFF ? W1[k] : kap, fr, fs, ft);
      static_assert(!IDT, "the identity is taken beside the recomputed tensor only");
      layer_backward<ND, UNPAIRED, false>(k, fr, fs, ft, T, Dg, gr_s, gs_s, a, b, ab, Aq);
    }
    }
    // ---- the cell's share of the restricted residual.  w = share - A_cell z down the lane's column; the product is
    // dropped on Dirichlet rows (a select, no branch: see the column kernel's epilogue).
    // (the lane's coarse point opaque here as well: otherwise its columns of M1 are read ahead of the layer loop and
    // held through it, as the thread index of the column kernel's write-back would be)
    int ie, je;
    coarse_point(ab, ie, je, NDC);
    double w[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k)
    {
      const int lk = (int)packed_position(lp, k);
      const bool bc = (sbc[lk >> 6] >> (lk & 63)) & 1ull;
      const double Ak = Aq[k]; // (read ahead of the select: see the column kernel's epilogue)
      w[k] = sy[lk] - (bc ? 0.0 : Ak);
    }
    // z in registers: M1[c][k] is wave-uniform (scalar loads)
    double tz[NDC];
#pragma unroll
    for (int k = 0; k < NDC; ++k)
    {
      tz[k] = 0.0;
#pragma unroll
      for (int c = 0; c < ND; ++c)
        tz[k] += R.M1[c * NDC + k] * w[c];
    }
    const bool contributes = coarse_ok && slot < nc;
#pragma unroll
    for (int k = 0; k < NDC; ++k)
    {
      q_s[ab] = tz[k];
      wave_fence();
      double vx = 0.0; // x: (a', b) -> (i, b)
#pragma unroll
      for (int mm = 0; mm < ND; ++mm)
        vx += sM[mm * NDC + ie] * q_s[mm * ND + b];
      gr_s[ab] = vx; // (lanes with a >= NDC hold a copy of row NDC - 1: written to their own place, never read)
      wave_fence();
      double vy = 0.0; // y: (i, b') -> (i, j)
#pragma unroll
      for (int mm = 0; mm < ND; ++mm)
        vy += sM[mm * NDC + je] * gr_s[ie * ND + mm];
      if (contributes)
        atomicAdd(&sc[packed_position(lcp, k)], vy); // in LDS (ds_add_f64)
      wave_fence();
    }
  }
  // ---- patch end: the coarse sums, one atomic per patch coarse dof (coarse was zero-filled by the host).  The coarse
  // list is requested by every wavefront as it leaves the cell loop, in front of the barrier that ends the accumulation
  // (as the column kernel re-reads its fine list: the thread index opaque, so that nothing is held through the loop).
  int tw = t;
  asm volatile("" : "+v"(tw));
  uint32_t cm[CITER];
#pragma unroll
  for (int j = 0; j < CITER; ++j)
  {
    const int i = tw + j * THREADS;
    cm[j] = R.cpdofs[coff + (i < Mc ? i : Mc - 1)];
  }
  lds_barrier();
#pragma unroll
  for (int j = 0; j < CITER; ++j)
  {
    const int i = tw + j * THREADS;
    if (i < Mc)
      atomicAdd(&coarse[cm[j] & PD_MASK], sc[i]);
  }
}
