// Private fragment of laplacian.hip, included there and nowhere else (inside its anonymous namespace): the layout of
// the stored geometry tensor G, and the affine-tensor, export, diagonal, load-vector and reaction kernels.  (The kernels
// that build G are in tensor_kernels.hpp, shared with the float tensor.)

// Layout of the stored geometry tensor G (double2 pairs (G00,G01)(G02,G11)(G12,G22)).  Two layouts:
//   default: [slot][layer c][pair][a*nd+b]
//   flat (P = 2, gflat()): [patch][item][layer c][pair][cell of the item][a*nd+b],
//     every (item, layer) block padded to whole 128-byte lines -- a wavefront then reads its item's
//     layer as NJ full-width loads of 64 consecutive double2 (whole lines, none shared between two
//     load instructions) and hands the values to the lanes that use them through LDS.  Pays where
//     the per-cell planes are short and misaligned: P = 2 (seven 144-byte pieces per load
//     instruction otherwise), 765 -> 674 us at 128^3; slower at P = 1, 3, 4 (1485 -> 1524, 513 -> 549,
//     458 -> 480 us), so only P = 2 uses it.
__host__ __device__ constexpr bool gflat(int nd) { return nd == 3; } // P = 2 only
__host__ __device__ constexpr int gcw(int nd) // cells of an item (Shape<P>::CW)
{
  return nd == 6 ? 7 : nd == 9 ? 3 : nd * nd <= 64 ? 64 / (nd * nd) : 1;
}
__host__ __device__ constexpr int gls(int nd) { return ((3 * gcw(nd) * nd * nd + 7) / 8) * 8; } // layer stride
__host__ __device__ constexpr long long gpatch(int nd, int K)
{
  return gflat(nd) ? (long long)((K + gcw(nd) - 1) / gcw(nd)) * nd * gls(nd) : (long long)K * 3 * nd * nd * nd;
}
// absolute position of (patch slot, quadrature point q = (a,b,c), component pair)
__device__ __forceinline__ size_t gpos(int nd, int K, long long slot, int q, int pair)
{
  const int nsq = nd * nd, N = nsq * nd;
  const int a = q / nsq, b = (q - a * nsq) / nd, c = q - a * nsq - b * nd;
  if (!gflat(nd))
    return (size_t)slot * 3 * N + (c * 3 + pair) * nsq + a * nd + b;
  // flat: [patch][item][layer c][pair][cell of the item][a*nd+b]
  const long long per_patch = gpatch(nd, K), p = slot / K;
  const size_t base = (size_t)p * per_patch;
  const int sl = (int)(slot - p * K), cw = gcw(nd), item = sl / cw;
  const size_t row = (size_t)(item * nd + c) * gls(nd);
  return base + row + pair * (cw * nsq) + (sl - item * cw) * nsq + a * nd + b;
}

// Constant geometry tensor of an affine cell: K K^T / detJ at the cell centre
// (q-independent when the cell is a parallelepiped); G_q = w_q * this.  ktensor (optional): the per-cell diffusion
// tensor, constant over the cell like the rest: K Kc K^T / detJ.  g: the coordinate element's degree; the four corners
// that span the cell sit at the tensor positions (0,0,0), (0,0,g), (0,g,0), (g,0,0) of its (g+1)^3 nodes.
__global__ void affine_geometry_kernel(long long nslots, int gdeg, const int32_t* __restrict__ pcell,
                                       const double* __restrict__ xgeom,
                                       const int32_t* __restrict__ geom_dofmap,
                                       const double* __restrict__ ktensor, double* __restrict__ Gaff)
{
  long long slot = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= nslots)
    return;
  int c = pcell[slot];
  double g[6] = {0, 0, 0, 0, 0, 0};
  if (c >= 0)
  {
    const int m = gdeg + 1;
    const int32_t* gd = geom_dofmap + (size_t)c * m * m * m;
    const double* x0 = xgeom + 3 * (size_t)gd[0];
    const double* xz = xgeom + 3 * (size_t)gd[gdeg];         // (0,0,g)
    const double* xy = xgeom + 3 * (size_t)gd[gdeg * m];     // (0,g,0)
    const double* xx = xgeom + 3 * (size_t)gd[gdeg * m * m]; // (g,0,0)
    double J[3][3];
    for (int i = 0; i < 3; ++i)
    {
      J[i][0] = xx[i] - x0[i];
      J[i][1] = xy[i] - x0[i];
      J[i][2] = xz[i] - x0[i];
    }
    double K[3][3], detJ;
    adjugate(J, K, detJ);
    const double s = 1.0 / detJ;
    if (ktensor)
    {
      double t[6];
      for (int d = 0; d < 6; ++d)
        t[d] = ktensor[(size_t)c * 6 + d];
      tensor_geometry(K, t, s, g);
    }
    else
      metric(K, s, g);
  }
  for (int d = 0; d < 6; ++d)
    Gaff[slot * 6 + d] = g[d];
}

// Monomial coefficients of a trilinear cell's map, x = sum c_ijk xi^i eta^j zeta^k on [0,1]^3, from its eight vertices
// v[4 i + 2 j + l]: Ccell[slot][4 i + 2 j + k][3]; an empty slot holds zeros.  Read by the recomputed form of the apply
// (TensorStream, stiffness_layer.hpp).
__global__ void cell_coefficient_kernel(long long nslots, const int32_t* __restrict__ pcell,
                                        const double* __restrict__ xgeom, const int32_t* __restrict__ geom_dofmap,
                                        double* __restrict__ Ccell)
{
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= nslots * 3)
    return;
  const long long slot = gid / 3;
  const int i = (int)(gid - slot * 3);
  const int c = pcell[slot];
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (c >= 0)
    for (int k = 0; k < 8; ++k)
      v[k] = xgeom[3 * (size_t)geom_dofmap[(size_t)c * 8 + k] + i];
  double* o = Ccell + slot * 24 + i;
  o[0] = v[0];
  o[3] = v[1] - v[0];                                              // zeta
  o[6] = v[2] - v[0];                                              // eta
  o[9] = (v[3] - v[2]) - (v[1] - v[0]);                            // eta zeta
  o[12] = v[4] - v[0];                                             // xi
  o[15] = (v[5] - v[4]) - (v[1] - v[0]);                           // xi zeta
  o[18] = (v[6] - v[4]) - (v[2] - v[0]);                           // xi eta
  o[21] = ((v[7] - v[6]) - (v[5] - v[4])) - ((v[3] - v[2]) - (v[1] - v[0])); // xi eta zeta
}

// paired slot layout -> the reference's [cell][q][6]
// (qperm: the caller's quadrature-point number -> ascending; nullptr = the caller's order is ascending)
__global__ void geometry_export_kernel(long long slot0, long long nslots, int nd, int K,
                                       const int32_t* __restrict__ pcell, const int32_t* __restrict__ qperm,
                                       const double2* __restrict__ G, double* __restrict__ out)
{
  const int nq = nd * nd * nd;
  long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= nslots * nq)
    return;
  long long slot = gid / nq;
  const int qc = (int)(gid - slot * nq); // the caller's number of the point
  const int q = qperm ? qperm[qc] : qc;
  slot += slot0;
  int c = pcell[slot];
  if (c < 0)
    return;
  double2 a = G[gpos(nd, K, slot, q, 0)], b = G[gpos(nd, K, slot, q, 1)],
          d = G[gpos(nd, K, slot, q, 2)];
  double* o = out + ((size_t)c * nq + qc) * 6;
  o[0] = a.x;
  o[1] = a.y;
  o[2] = b.x;
  o[3] = b.y;
  o[4] = d.x;
  o[5] = d.y;
}

// ---- matrix-free diagonal (replaces the CSR detour of examples/pmg/main.cpp:274-279) ----
__global__ void diagonal_kernel(long long slot0, long long nslots, int nd, int K,
                                const int32_t* __restrict__ pcell,
                                const double2* __restrict__ G, const int32_t* __restrict__ dofmap,
                                const int8_t* __restrict__ bc, const double* __restrict__ kappa,
                                const double* __restrict__ D, double* __restrict__ diag)
{
  const int N = nd * nd * nd, nsq = nd * nd;
  long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= nslots * N)
    return;
  long long slot = gid / N;
  int t = (int)(gid - slot * N);
  slot += slot0;
  int cell = pcell[slot];
  if (cell < 0)
    return;
  int a = t / nsq, b = (t - a * nsq) / nd, c = t - a * nsq - b * nd;
  auto Gq = [&](int q, int pair) { return G[gpos(nd, K, slot, q, pair)]; };
  double s = 0.0;
  for (int q = 0; q < nd; ++q)
  {
    double da = D[q * nd + a], db = D[q * nd + b], dc = D[q * nd + c];
    s += da * da * Gq(q * nsq + b * nd + c, 0).x; // G00 at (q,b,c)
    s += db * db * Gq(a * nsq + q * nd + c, 1).y; // G11 at (a,q,c)
    s += dc * dc * Gq(a * nsq + b * nd + q, 2).y; // G22 at (a,b,q)
  }
  double daa = D[a * nd + a], dbb = D[b * nd + b], dcc = D[c * nd + c];
  s += 2.0
       * (Gq(t, 0).y * daa * dbb + Gq(t, 1).x * daa * dcc + Gq(t, 2).x * dbb * dcc);
  int32_t dof = dofmap[(size_t)cell * N + t];
  if (!bc[dof])
    atomicAdd(&diag[dof], kappa[cell] * s);
}

// (react, optional: the diagonal term's vector -- reaction and Robin components summed --, added to the diagonal of A
// before the inversion; zero on marked dofs)
__global__ void diag_invert_kernel(int n, const int8_t* __restrict__ bc, const double* __restrict__ react,
                                   double* __restrict__ d)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
  {
    double v = d[i];
    if (react)
      v += react[i];
    d[i] = bc[i] ? 1.0 : (v != 0.0 ? 1.0 / v : 0.0);
  }
}

// ---- GLL-collocated load vector ----
__global__ void rhs_kernel(long long nslots, int nq, int ng, const int32_t* __restrict__ pcell,
                           const double* __restrict__ xgeom,
                           const int32_t* __restrict__ geom_dofmap,
                           const double* __restrict__ dphi, const double* __restrict__ w,
                           const int32_t* __restrict__ dofmap, const int8_t* __restrict__ bc,
                           const double* __restrict__ kappa, const double* __restrict__ f,
                           double* __restrict__ b)
{
  long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= nslots * nq)
    return;
  long long slot = gid / nq;
  int q = (int)(gid - slot * nq);
  int c = pcell[slot];
  if (c < 0)
    return;
  int32_t dof = dofmap[(size_t)c * nq + q];
  if (bc[dof])
    return; // set_bc: b[bc] = 0 (b is zeroed first)
  double K[3][3], detJ;
  jacobian(xgeom, geom_dofmap + (size_t)c * ng, dphi, nq, q, ng, K, detJ);
  atomicAdd(&b[dof], kappa[c] * w[q] * detJ * f[dof]);
}

// ---- reaction vector: d[dof] = sum over the listed cells' points on the dof of sigma_c w_q detJ_q, the weights of
// rhs_kernel with sigma in place of kappa and f = 1 (d is zeroed first; marked dofs stay 0: their rows are y = x) ----
__global__ void reaction_kernel(long long nslots, int nq, int ng, const int32_t* __restrict__ pcell,
                                const double* __restrict__ xgeom, const int32_t* __restrict__ geom_dofmap,
                                const double* __restrict__ dphi, const double* __restrict__ w,
                                const int32_t* __restrict__ dofmap, const int8_t* __restrict__ bc,
                                const double* __restrict__ sigma, double* __restrict__ d)
{
  long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= nslots * nq)
    return;
  long long slot = gid / nq;
  int q = (int)(gid - slot * nq);
  int c = pcell[slot];
  if (c < 0)
    return;
  int32_t dof = dofmap[(size_t)c * nq + q];
  if (bc[dof])
    return;
  double K[3][3], detJ;
  jacobian(xgeom, geom_dofmap + (size_t)c * ng, dphi, nq, q, ng, K, detJ);
  atomicAdd(&d[dof], sigma[c] * w[q] * detJ);
}
