// Building blocks of the FP32 V-cycle (pmg_multigrid_set_precision, solvers.hip): the Chebyshev smoother's fused
// vector passes, the patch-form transfers and the conversions between the caller's FP64 vectors and the cycle's
// float ones.  Same algorithms and the same pass structure as the FP64 forms (vector.hip, interpolate.hip,
// solvers.hip cheb_iterate) at half the bytes per dof; every scalar coefficient is formed in FP64 and rounded once.
#include "common.hpp"
#include "patches.hpp"

#include <algorithm>

using namespace pmg;

namespace pmg
{
int laplacian_apply_f32(pmg_laplacian op, const float* in, float* out, hipStream_t s);
TransferView interp_transfer_view(pmg_interpolator ip);
bool interp_is_patched(pmg_interpolator ip);
} // namespace pmg

namespace
{
constexpr int EW32_THREADS = 256;
int ew32_blocks(long long n)
{
  const long long b = (n + EW32_THREADS - 1) / EW32_THREADS;
  return (int)std::max(1LL, std::min(b, 4096LL));
}
template <typename F>
__global__ void ew32_kernel(int n, F f)
{
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    f(i);
}
template <typename F>
void ew32(int n, F f, hipStream_t s)
{
  if (n > 0)
    ew32_kernel<<<ew32_blocks(n), EW32_THREADS, 0, s>>>(n, f);
}

// Chebyshev passes (vector.hip ChebInitF / ChebFirstF / ChebStepF / ChebResidualF / ChebLastF)
struct ChebInit32
{ // r = b - q ; z = c0 dinv r   (q == nullptr: r = b)
  float *r, *z;
  const float *b, *q, *dinv;
  float c0;
  __device__ void operator()(int i) const
  {
    const float vr = b[i] - (q ? q[i] : 0.0f);
    r[i] = vr;
    z[i] = c0 * dinv[i] * vr;
  }
};
struct ChebFirst32
{ // from x == 0: r -= q ; z_2 = c1 z_1 + c2 dinv r ; x = z_1 + z_2
  float *x, *r, *z;
  const float *q, *dinv;
  float c1, c2;
  int keep_rz;
  __device__ void operator()(int i) const
  {
    const float z1 = z[i], vr = r[i] - q[i];
    const float z2 = c1 * z1 + c2 * dinv[i] * vr;
    if (keep_rz)
    {
      r[i] = vr;
      z[i] = z2;
    }
    x[i] = z1 + z2;
  }
};
struct ChebStep32
{ // r -= q ; z_new = c1 z + c2 dinv r ; x += (z if both) + z_new
  float *x, *r, *z;
  const float *q, *dinv;
  float c1, c2;
  int both, keep_rz;
  __device__ void operator()(int i) const
  {
    float vz = z[i], vx = x[i];
    if (both)
      vx += vz;
    const float vr = r[i] - q[i];
    vz = c1 * vz + c2 * dinv[i] * vr;
    if (keep_rz)
    {
      r[i] = vr;
      z[i] = vz;
    }
    x[i] = vx + vz;
  }
};
struct Sub32
{ // r -= q
  float* r;
  const float* q;
  __device__ void operator()(int i) const { r[i] -= q[i]; }
};
struct ChebLast32
{ // x (+)= z ; r -= q
  float *x, *r;
  const float *z, *q;
  int assign;
  __device__ void operator()(int i) const
  {
    x[i] = (assign ? 0.0f : x[i]) + z[i];
    r[i] -= q[i];
  }
};
struct Add32
{ // x += z
  float* x;
  const float* z;
  __device__ void operator()(int i) const { x[i] += z[i]; }
};
struct Copy32
{
  float* x;
  const float* z;
  __device__ void operator()(int i) const { x[i] = z[i]; }
};
struct Zero32
{
  float* x;
  __device__ void operator()(int i) const { x[i] = 0.0f; }
};
struct MaskBc32
{
  float* b;
  const int8_t* bc;
  __device__ void operator()(int i) const
  {
    if (bc[i])
      b[i] = 0.0f;
  }
};
// conversions
struct ToF32
{ // out = float(in - sub)   (sub optional: the defect rhs - A y of a cycle from a non-zero guess)
  float* out;
  const double *in, *sub;
  __device__ void operator()(int i) const { out[i] = (float)(sub ? in[i] - sub[i] : in[i]); }
};
struct FromF32
{ // out (+)= double(in)
  double* out;
  const float* in;
  int add;
  __device__ void operator()(int i) const { out[i] = (add ? out[i] : 0.0) + (double)in[i]; }
};

// ---- patch-form transfers in FP32 (interpolate.hip prolong_patch_kernel / restrict_patch_kernel) ----
__device__ __forceinline__ void tfence32()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ void tbarrier32()
{
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
constexpr int cpw32(int ndf) { return ndf * ndf * ndf <= 32 ? 2 : 1; } // cells per wavefront pass

struct Transfer32Args
{
  int first, K, max_mf, max_mc;
  const int32_t *poff, *lmap_id, *pncell, *cpoff, *clmap_id;
  const uint32_t *pdofs, *cpdofs;
  const uint16_t *lmaps, *clmaps;
  const uint8_t* pmult;
  const float* M1;
};

// fine += P coarse: every fine patch dof is written by the first patch (in launch order) that holds it
template <int NDC, int NDF>
__global__ void prolong_add_f32_kernel(Transfer32Args A, const float* __restrict__ coarse, float* __restrict__ fine)
{
  extern __shared__ __attribute__((aligned(16))) float smem32[];
  constexpr int ndc = NDC, ndf = NDF, Nc = ndc * ndc * ndc, Nf = ndf * ndf * ndf;
  constexpr int n1 = ndf * ndc * ndc, n2 = ndf * ndf * ndc;
  constexpr int CPW = cpw32(NDF), HL = 64 / CPW;
  float* sM = smem32;           // [ndf*ndc]
  float* sc = sM + ndf * ndc;   // [max_mc]
  float* sf = sc + A.max_mc;    // [max_mf]
  float* scratch = sf + A.max_mf;
  const int p = A.first + blockIdx.x, t = threadIdx.x, nthr = blockDim.x;
  const int off = A.poff[p], Mf = A.poff[p + 1] - off;
  const int coff = A.cpoff[p], Mc = A.cpoff[p + 1] - coff;
  const int nc = A.pncell[p];
  for (int i = t; i < ndf * ndc; i += nthr)
    sM[i] = A.M1[i];
  for (int i = t; i < Mc; i += nthr)
    sc[i] = coarse[A.cpdofs[coff + i] & PD_MASK];
  tbarrier32();
  const int wave = t >> 6, lane = t & 63, nw = nthr >> 6;
  const int half = lane / HL, ll = lane - half * HL;
  float* uc = scratch + (size_t)(wave * CPW + half) * (Nc + n1 + n2);
  float* t1 = uc + Nc;
  float* t2 = t1 + n1;
  const uint16_t* cl = A.clmaps + (size_t)A.clmap_id[p] * A.K * Nc;
  const uint16_t* fl = A.lmaps + (size_t)A.lmap_id[p] * A.K * Nf;
  for (int slot0 = wave * CPW; slot0 < nc; slot0 += nw * CPW)
  {
    const int slot = slot0 + half;
    const bool mine = slot < nc;
    const int sl = mine ? slot : nc - 1;
    for (int o = ll; o < Nc; o += HL)
      uc[o] = sc[cl[(size_t)sl * Nc + o]];
    tfence32();
    for (int o = ll; o < n1; o += HL) // (a, j, k): sum over i
    {
      const int a = o / (ndc * ndc), jk = o - a * ndc * ndc;
      float w = 0.0f;
#pragma unroll
      for (int i = 0; i < ndc; ++i)
        w += sM[a * ndc + i] * uc[i * ndc * ndc + jk];
      t1[o] = w;
    }
    tfence32();
    for (int o = ll; o < n2; o += HL) // (a, b, k): sum over j
    {
      const int a = o / (ndf * ndc), r = o - a * ndf * ndc, b = r / ndc, k = r - b * ndc;
      float w = 0.0f;
#pragma unroll
      for (int j = 0; j < ndc; ++j)
        w += sM[b * ndc + j] * t1[(a * ndc + j) * ndc + k];
      t2[o] = w;
    }
    tfence32();
    for (int o = ll; o < Nf; o += HL) // (a, b, c): sum over k
    {
      const int a = o / (ndf * ndf), r = o - a * ndf * ndf, b = r / ndf, c = r - b * ndf;
      float w = 0.0f;
#pragma unroll
      for (int k = 0; k < ndc; ++k)
        w += sM[c * ndc + k] * t2[(a * ndf + b) * ndc + k];
      if (mine)
        sf[fl[(size_t)sl * Nf + (c * ndf * ndf + a * ndf + b)]] = w; // shared dofs: identical values
    }
    tfence32();
  }
  tbarrier32();
  for (int i = t; i < Mf; i += nthr)
  {
    const uint32_t m = A.pdofs[off + i];
    if (!(m & PD_ACC)) // this patch is the first writer of the dof
      fine[m & PD_MASK] += sf[i];
  }
}

// coarse += R (fine - fine_sub): multiplicity-weighted transpose, patch sums added with float atomics
template <int NDC, int NDF>
__global__ void restrict_f32_kernel(Transfer32Args A, const float* __restrict__ fine,
                                    const float* __restrict__ fine_sub, float* __restrict__ coarse)
{
  extern __shared__ __attribute__((aligned(16))) float smem32[];
  constexpr int ndc = NDC, ndf = NDF, Nc = ndc * ndc * ndc, Nf = ndf * ndf * ndf;
  constexpr int n1 = ndf * ndc * ndc, n2 = ndf * ndf * ndc;
  constexpr int CPW = cpw32(NDF), HL = 64 / CPW;
  float* sM = smem32;
  float* sc = sM + ndf * ndc;     // [max_mc] coarse accumulators
  float* sf = sc + A.max_mc;      // [max_mf] weighted fine values
  float* scratch = sf + A.max_mf; // per wave and cell of the pass: w[Nf] t2[n2] t1[n1]
  const int p = A.first + blockIdx.x, t = threadIdx.x, nthr = blockDim.x;
  const int off = A.poff[p], Mf = A.poff[p + 1] - off;
  const int coff = A.cpoff[p], Mc = A.cpoff[p + 1] - coff;
  const int nc = A.pncell[p];
  for (int i = t; i < ndf * ndc; i += nthr)
    sM[i] = A.M1[i];
  for (int i = t; i < Mf; i += nthr)
  {
    const uint32_t dof = A.pdofs[off + i] & PD_MASK;
    const float v = fine_sub ? fine[dof] - fine_sub[dof] : fine[dof];
    sf[i] = v / (float)A.pmult[off + i];
  }
  for (int i = t; i < Mc; i += nthr)
    sc[i] = 0.0f;
  tbarrier32();
  const int wave = t >> 6, lane = t & 63, nw = nthr >> 6;
  const int half = lane / HL, ll = lane - half * HL;
  float* w = scratch + (size_t)(wave * CPW + half) * (Nf + n1 + n2);
  float* t2 = w + Nf;
  float* t1 = t2 + n2;
  const uint16_t* cl = A.clmaps + (size_t)A.clmap_id[p] * A.K * Nc;
  const uint16_t* fl = A.lmaps + (size_t)A.lmap_id[p] * A.K * Nf;
  for (int slot0 = wave * CPW; slot0 < nc; slot0 += nw * CPW)
  {
    const int slot = slot0 + half;
    const bool mine = slot < nc;
    const int sl = mine ? slot : nc - 1;
    for (int o = ll; o < Nf; o += HL)
    {
      const int a = o / (ndf * ndf), r = o - a * ndf * ndf, b = r / ndf, c = r - b * ndf;
      w[o] = sf[fl[(size_t)sl * Nf + (c * ndf * ndf + a * ndf + b)]];
    }
    tfence32();
    for (int o = ll; o < n2; o += HL) // (a, b, k): sum over c
    {
      const int ab = o / ndc, k = o - ab * ndc;
      float v = 0.0f;
#pragma unroll
      for (int c = 0; c < ndf; ++c)
        v += sM[c * ndc + k] * w[ab * ndf + c];
      t2[o] = v;
    }
    tfence32();
    for (int o = ll; o < n1; o += HL) // (a, j, k): sum over b
    {
      const int a = o / (ndc * ndc), r = o - a * ndc * ndc, j = r / ndc, k = r - j * ndc;
      float v = 0.0f;
#pragma unroll
      for (int b = 0; b < ndf; ++b)
        v += sM[b * ndc + j] * t2[(a * ndf + b) * ndc + k];
      t1[o] = v;
    }
    tfence32();
    for (int o = ll; o < Nc; o += HL) // (i, j, k): sum over a
    {
      const int i = o / (ndc * ndc), jk = o - i * ndc * ndc;
      float v = 0.0f;
#pragma unroll
      for (int a = 0; a < ndf; ++a)
        v += sM[a * ndc + i] * t1[a * ndc * ndc + jk];
      if (mine)
        atomicAdd(&sc[cl[(size_t)sl * Nc + o]], v); // in LDS
    }
    tfence32();
  }
  tbarrier32();
  for (int i = t; i < Mc; i += nthr)
    atomicAdd(&coarse[A.cpdofs[coff + i] & PD_MASK], sc[i]);
}

#define PMG_FOR_PAIRS32(X)                                                                                            \
  X(2, 3) X(2, 4) X(2, 5) X(2, 6) X(2, 7) X(2, 8) X(2, 9) X(3, 4) X(3, 5) X(3, 6) X(3, 7) X(3, 8) X(3, 9) X(4, 5)     \
  X(4, 6) X(4, 7) X(4, 8) X(4, 9) X(5, 6) X(5, 7) X(5, 8) X(5, 9) X(6, 7) X(6, 8) X(6, 9) X(7, 8) X(7, 9) X(8, 9)

int transfer32_lds(int ndc, int ndf, int bytes)
{
#define X(C, F)                                                                                                       \
  if (ndc == C && ndf == F)                                                                                           \
  {                                                                                                                   \
    PMG_HIP(hipFuncSetAttribute((const void*)prolong_add_f32_kernel<C, F>,                                            \
                                hipFuncAttributeMaxDynamicSharedMemorySize, bytes));                                  \
    PMG_HIP(hipFuncSetAttribute((const void*)restrict_f32_kernel<C, F>, hipFuncAttributeMaxDynamicSharedMemorySize,   \
                                bytes));                                                                              \
    return PMG_OK;                                                                                                    \
  }
  PMG_FOR_PAIRS32(X)
#undef X
  return fail(PMG_ERR_INVALID, "unsupported degree pair");
}

// LDS of one transfer workgroup, and its wavefronts (the FP64 kernels' count: the float scratch fits a fortiori)
size_t transfer32_shm(const TransferView& v)
{
  const int ndc = v.ndc, ndf = v.ndf;
  const size_t per_wave = (size_t)cpw32(ndf) * ((size_t)ndf * ndf * ndf + ndf * ndc * ndc + ndf * ndf * ndc);
  const size_t base = (size_t)ndf * ndc + v.cmax_m + v.fv.max_m;
  return sizeof(float) * (base + (size_t)v.pwaves * per_wave);
}

Transfer32Args args32(const TransferView& v, const float* M1, int first)
{
  Transfer32Args A;
  A.first = first;
  A.K = v.fv.K;
  A.max_mf = v.fv.max_m;
  A.max_mc = v.cmax_m;
  A.poff = v.fv.poff;
  A.lmap_id = v.fv.lmap_id;
  A.pncell = v.fv.pncell;
  A.cpoff = v.cpoff;
  A.clmap_id = v.clmap_id;
  A.pdofs = v.fv.pdofs;
  A.cpdofs = v.cpdofs;
  A.lmaps = v.fv.lmaps;
  A.clmaps = v.clmaps;
  A.pmult = v.pmult;
  A.M1 = M1;
  return A;
}
} // namespace

namespace pmg
{
void launch_to_f32(int n, const double* in, const double* sub, float* out, hipStream_t s)
{
  ew32(n, ToF32{out, in, sub}, s);
}
void launch_from_f32(int n, const float* in, double* out, bool add, hipStream_t s)
{
  ew32(n, FromF32{out, in, add ? 1 : 0}, s);
}
void launch_zero_f32(int n, float* x, hipStream_t s) { ew32(n, Zero32{x}, s); }
void launch_mask_bc_f32(int n, float* b, const int8_t* bc, hipStream_t s) { ew32(n, MaskBc32{b, bc}, s); }

// Can the FP32 transfers run on this interpolator?  (0 = yes, else the refusal has been recorded)
int transfer_f32_supported(pmg_interpolator ip, const char* who)
{
  PMG_REQUIRE(interp_is_patched(ip),
              "%s: the FP32 transfers need a patch-form interpolator (pmg_interpolator_create_with_operator)", who);
  const TransferView v = interp_transfer_view(ip);
  for (pmg_layout l : {v.lc, v.lf})
    PMG_REQUIRE(l->num_ghosts == 0 && !l->multi_rank() && !l->win,
                "%s: the FP32 transfers are single-domain only (a layout has ghosts or a communicator)", who);
  return PMG_OK;
}

// The interpolator's float copy of its 1-D table, built (and the LDS limits set) on first use; patch form only
int transfer_f32_prepare(pmg_interpolator ip, const float** M1)
{
  float*& m = interp_m1_f32(ip);
  if (!m)
  {
    const TransferView v = interp_transfer_view(ip);
    const size_t shm = transfer32_shm(v);
    PMG_REQUIRE(shm <= 160 * 1024, "FP32 transfer kernels need %zu bytes of LDS", shm);
    if (shm > 48 * 1024)
      PMG_TRY(transfer32_lds(v.ndc, v.ndf, (int)shm));
    const int n = v.ndf * v.ndc;
    std::vector<double> h(n);
    PMG_HIP(hipMemcpy(h.data(), v.M1, sizeof(double) * n, hipMemcpyDeviceToHost));
    std::vector<float> f(h.begin(), h.end());
    float* d = nullptr;
    PMG_HIP(hipMalloc(&d, sizeof(float) * n));
    const hipError_t e = hipMemcpy(d, f.data(), sizeof(float) * n, hipMemcpyHostToDevice);
    if (e != hipSuccess)
    {
      (void)hipFree(d);
      return fail(PMG_ERR_HIP, "transfer_f32_prepare: %s", hipGetErrorString(e));
    }
    m = d;
  }
  *M1 = m;
  return PMG_OK;
}

// fine += P coarse (all patches of the fine operator, one launch: no halo on a single domain)
int prolong_add_f32(pmg_interpolator ip, const float* M1, const float* coarse, float* fine, hipStream_t s)
{
  const TransferView v = interp_transfer_view(ip);
  const int np = v.fv.npatch;
  if (np <= 0)
    return PMG_OK;
  const Transfer32Args A = args32(v, M1, 0);
  const size_t shm = transfer32_shm(v);
#define X(C, F)                                                                                                       \
  if (v.ndc == C && v.ndf == F)                                                                                       \
  {                                                                                                                   \
    prolong_add_f32_kernel<C, F><<<np, v.pwaves * 64, shm, s>>>(A, coarse, fine);                                     \
    PMG_HIP(hipGetLastError());                                                                                       \
    return PMG_OK;                                                                                                    \
  }
  PMG_FOR_PAIRS32(X)
#undef X
  return fail(PMG_ERR_INVALID, "unsupported degree pair");
}

// coarse = R (fine - fine_sub); fine_sub may be NULL
int restrict_f32(pmg_interpolator ip, const float* M1, const float* fine, const float* fine_sub, float* coarse,
                 hipStream_t s)
{
  const TransferView v = interp_transfer_view(ip);
  launch_zero_f32(v.lc->total(), coarse, s);
  const int np = v.fv.npatch;
  if (np <= 0)
    return PMG_OK;
  const Transfer32Args A = args32(v, M1, 0);
  const size_t shm = transfer32_shm(v);
#define X(C, F)                                                                                                       \
  if (v.ndc == C && v.ndf == F)                                                                                       \
  {                                                                                                                   \
    restrict_f32_kernel<C, F><<<np, v.pwaves * 64, shm, s>>>(A, fine, fine_sub, coarse);                              \
    PMG_HIP(hipGetLastError());                                                                                       \
    return PMG_OK;                                                                                                    \
  }
  PMG_FOR_PAIRS32(X)
#undef X
  return fail(PMG_ERR_INVALID, "unsupported degree pair");
}

// cheb_iterate (solvers.hip) in FP32 on one level without ghosts: the same passes, coefficients formed in FP64
int cheb_iterate_f32(const ChebWork32& w, pmg_laplacian A, const float* dinv, int n, double lmax, int max_iter,
                     float* x, const float* b, int need_r, bool x_zero, hipStream_t s, bool* split)
{
  if (split)
    *split = false;
  const float c0 = (float)(4.0 / (3.0 * lmax));
  if (x_zero)
    ew32(n, ChebInit32{w.r, w.z, b, nullptr, dinv, c0}, s);
  else
  {
    PMG_TRY(laplacian_apply_f32(A, x, w.q, s));
    ew32(n, ChebInit32{w.r, w.z, b, w.q, dinv, c0}, s);
  }
  for (int i = 1; i <= max_iter; ++i)
  {
    const bool last = (i == max_iter);
    if (last && !need_r)
    {
      if (max_iter == 1)
      {
        if (x_zero)
          ew32(n, Copy32{x, w.z}, s);
        else
          ew32(n, Add32{x, w.z}, s);
      }
      break;
    }
    PMG_TRY(laplacian_apply_f32(A, w.z, w.q, s));
    if (last)
    {
      if (max_iter == 1)
        ew32(n, ChebLast32{x, w.r, w.z, w.q, x_zero ? 1 : 0}, s);
      else if (need_r == ResidualSplit && split)
        *split = true;
      else
        ew32(n, Sub32{w.r, w.q}, s);
      break;
    }
    const float c1 = (float)((2.0 * i - 1.0) / (2.0 * i + 3.0));
    const float c2 = (float)((8.0 * i + 4.0) / (2.0 * i + 3.0) / lmax);
    const int keep_rz = (i + 1 == max_iter && need_r == ResidualNone) ? 0 : 1;
    if (x_zero && i == 1)
      ew32(n, ChebFirst32{x, w.r, w.z, w.q, dinv, c1, c2, keep_rz}, s);
    else
      ew32(n, ChebStep32{x, w.r, w.z, w.q, dinv, c1, c2, i == 1 ? 1 : 0, keep_rz}, s);
  }
  if (max_iter == 0 && x_zero)
    launch_zero_f32(n, x, s);
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}
} // namespace pmg

extern "C" int pmg_interpolator_interpolate_add_f32(pmg_interpolator ip, const float* coarse, float* fine,
                                                    pmg_stream stream)
{
  PMG_REQUIRE(ip && coarse && fine, "pmg_interpolator_interpolate_add_f32: NULL argument");
  PMG_TRY(transfer_f32_supported(ip, "pmg_interpolator_interpolate_add_f32"));
  const float* M1 = nullptr;
  PMG_TRY(transfer_f32_prepare(ip, &M1));
  return prolong_add_f32(ip, M1, coarse, fine, S(stream));
}

extern "C" int pmg_interpolator_reverse_interpolate_f32(pmg_interpolator ip, const float* fine, const float* fine_sub,
                                                        float* coarse, pmg_stream stream)
{
  PMG_REQUIRE(ip && fine && coarse, "pmg_interpolator_reverse_interpolate_f32: NULL argument");
  PMG_TRY(transfer_f32_supported(ip, "pmg_interpolator_reverse_interpolate_f32"));
  const float* M1 = nullptr;
  PMG_TRY(transfer_f32_prepare(ip, &M1));
  return restrict_f32(ip, M1, fine, fine_sub, coarse, S(stream));
}
