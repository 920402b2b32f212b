// Algebraic multigrid for the coarsest (degree 1) level of the p-multigrid hierarchy.
//
// The reference solves its coarsest level with PETSc's KSPCG (at most 60 iterations) preconditioned
// by hypre BoomerAMG on an assembled aijhipsparse matrix (src/amg.hpp:33-47, wired in at
// src/pmg.hpp:106-107 through examples/pmg/main.cpp:331-335).  hypre and PETSc are third-party
// arithmetic that is not part of this repository; this file is the library's own solver for that
// slot, written for the same inputs the degree-1 operator already has:
//
//   set-up (host, once): smoothed aggregation on the assembled degree-1 stiffness matrix -- the algorithm and
//     all of its host code are in amg_setup.hpp (free of HIP, checked on the CPU); this file downloads the
//     operator's data for it, moves its tables between the ranks and uploads what it built.
//   renewal (device, after a coefficient change): pmg_amg_update_values recomputes every value of the hierarchy on
//     the aggregates of the set-up -- plan and row routines in amg_renew.hpp, kernels and sequence below.
//   cycle (device): V(k, k) with the same 4th-kind Chebyshev / Jacobi smoother as the p-levels
//     (cheb_iterate), lean form (the pre-smoother leaves the residual, the post-smoother skips its
//     last product), CSR products one sub-wavefront per row.  Nothing synchronises the host.
//   solve: either a fixed number of cycles from a zero initial guess (a fixed linear operator: the
//     p-multigrid cycle stays a valid CG preconditioner and can be captured in a graph), or the
//     reference's shape -- CG on the matrix-free operator preconditioned by one cycle, to a
//     relative tolerance, at most max_iter iterations.
//
// Several ranks, two forms.  Replicated (pmg_amg_create_replicated, what the harness uses): the owned
// rows are gathered once, with global column indices, into the global degree-1 matrix on every rank
// (coarse-grid agglomeration); a solve is ONE all-reduce of the zero-padded right-hand side followed by
// the single-rank solve of the whole coarse problem on every rank -- identical arithmetic everywhere, no
// communication inside, the same iteration counts as on one rank.  The degree-1 level is 1/64 of the
// p = 4 dofs, so the redundant work stays small next to a fine-level smooth.  Rank-local
// (pmg_amg_create on a distributed operator): the hierarchy of the rank's owned block as a block
// preconditioner of a distributed Krylov solve (ghost couplings dropped from the preconditioner only):
// no gather, but 9 -> 31 -> 38 -> 40 CG iterations on 1 -> 2 -> 4 -> 8 ranks (tools/amg_rank_scaling.py).
//
// Parity: unpinned by the reference (third-party arithmetic, no fixture).  The tests compare the
// device cycle with a numpy restatement of the same hierarchy (oracle/amg_oracle.py) and check the
// solver's defining properties (symmetry, contraction, h-independent iteration counts).
#include "amg_renew.hpp"
#include "amg_setup.hpp"
#include "common.hpp"
#include "laplacian.hpp"
#include "patches.hpp"

#include <memory>

using namespace pmg;
using namespace pmg::amg_setup;

namespace
{
int accepted(const std::string& refused) { return refused.empty() ? PMG_OK : fail(PMG_ERR_INVALID, "%s", refused.c_str()); }

struct DevCsr
{
  int n = 0, m = 0, tpr = 4; // threads per row of the product kernels
  int* rp = nullptr;
  int* ci = nullptr;
  double* v = nullptr;
};

template <typename T>
int to_device(T** dst, const std::vector<T>& src)
{
  PMG_HIP(hipMalloc(dst, sizeof(T) * std::max<size_t>(src.size(), 1)));
  if (!src.empty())
    PMG_HIP(hipMemcpy(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
  return PMG_OK;
}

// device scratch of the set-up, freed on every way out
struct Scratch
{
  double* p = nullptr;
  Scratch() = default;
  Scratch(const Scratch&) = delete;
  ~Scratch() { (void)hipFree(p); }
  int alloc(size_t n)
  {
    PMG_HIP(hipMalloc(&p, sizeof(double) * std::max<size_t>(n, 1)));
    return PMG_OK;
  }
};

int upload_csr(DevCsr& d, const HostCsr& h)
{
  d.n = h.n;
  d.m = h.m;
  const double avg = h.n ? (double)h.nnz() / h.n : 1.0;
  d.tpr = avg > 48 ? 32 : avg > 24 ? 16 : avg > 10 ? 8 : avg > 4 ? 4 : 2;
  PMG_TRY(to_device(&d.rp, h.rp));
  PMG_TRY(to_device(&d.ci, h.ci));
  PMG_TRY(to_device(&d.v, h.v));
  return PMG_OK;
}

void free_csr(DevCsr& d)
{
  (void)hipFree(d.rp);
  (void)hipFree(d.ci);
  (void)hipFree(d.v);
  d = DevCsr();
}

// ---- device products: TPR lanes of a wavefront share a row ------------------------------------
// MODE 0: y = A x    1: y = b - A x    2: y += A x
template <int TPR, int MODE>
__global__ void csr_product_kernel(int n, const int* __restrict__ rp, const int* __restrict__ ci,
                                   const double* __restrict__ v, const double* __restrict__ x,
                                   const double* __restrict__ b, double* __restrict__ y)
{
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int row = gid / TPR, sub = gid % TPR;
  double acc = 0.0;
  if (row < n)
  {
    const int e = rp[row + 1];
    for (int k = rp[row] + sub; k < e; k += TPR)
      acc += v[k] * x[ci[k]];
  }
#pragma unroll
  for (int off = TPR / 2; off > 0; off >>= 1)
    acc += __shfl_down(acc, off, TPR);
  if (row < n && sub == 0)
  {
    if (MODE == 0)
      y[row] = acc;
    else if (MODE == 1)
      y[row] = b[row] - acc;
    else
      y[row] += acc;
  }
}

template <int MODE>
int csr_product(const DevCsr& A, const double* x, const double* b, double* y, hipStream_t s)
{
  if (A.n == 0)
    return PMG_OK;
  const long long threads = (long long)A.n * A.tpr;
  const int blocks = (int)((threads + 255) / 256);
  switch (A.tpr)
  {
  case 2:
    csr_product_kernel<2, MODE><<<blocks, 256, 0, s>>>(A.n, A.rp, A.ci, A.v, x, b, y);
    break;
  case 4:
    csr_product_kernel<4, MODE><<<blocks, 256, 0, s>>>(A.n, A.rp, A.ci, A.v, x, b, y);
    break;
  case 8:
    csr_product_kernel<8, MODE><<<blocks, 256, 0, s>>>(A.n, A.rp, A.ci, A.v, x, b, y);
    break;
  case 16:
    csr_product_kernel<16, MODE><<<blocks, 256, 0, s>>>(A.n, A.rp, A.ci, A.v, x, b, y);
    break;
  default:
    csr_product_kernel<32, MODE><<<blocks, 256, 0, s>>>(A.n, A.rp, A.ci, A.v, x, b, y);
    break;
  }
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}

// y = Ainv b, dense n x n, one wavefront per row
__global__ void dense_apply_kernel(int n, const double* __restrict__ Ainv, const double* __restrict__ b,
                                   double* __restrict__ y)
{
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (row >= n)
    return;
  double acc = 0.0;
  for (int k = lane; k < n; k += 64)
    acc += Ainv[(size_t)row * n + k] * b[k];
  for (int off = 32; off > 0; off >>= 1)
    acc += __shfl_down(acc, off, 64);
  if (lane == 0)
    y[row] = acc;
}

} // namespace

struct AmgLevel
{
  DevCsr A, P, R;
  double* dinv = nullptr;
  double lmax = 1.0;
  int n = 0;
  // work vectors of the level (x and b of level 0 are the caller's)
  double *x = nullptr, *b = nullptr, *r = nullptr, *z = nullptr, *q = nullptr;
  long long nnz = 0;
};

struct AmgRenewal; // what pmg_amg_update_values plans on its first call (below)

struct pmg_amg_s
{
  pmg_laplacian op = nullptr; // the degree-1 operator (Krylov mode applies it)
  pmg_layout layout = nullptr;
  std::vector<AmgLevel> levels;
  double* dense_inv = nullptr; // coarsest level, n x n: the inverse in use, one of the two below (nullptr: smooth it)
  int n_coarsest = 0;
  // Constant null space (pmg_amg_set_nullspace).  Both inverses are kept once built, so a captured cycle never holds
  // a freed address: the plain one of the set-up (nullptr where its Cholesky stopped) and that of A_c + gamma v v^T.
  int nullspace = PMG_NULLSPACE_NONE;
  double *dense_inv_plain = nullptr, *dense_inv_null = nullptr;
  int smoother_its = 2;
  int cycles = 0;       // > 0: stationary mode, that many cycles per solve
  int max_iter = 60;    // Krylov mode (src/amg.hpp:39-40)
  double rtol = 1e-5;   // KSP's default relative tolerance
  pmg_cg cg = nullptr;  // work vectors of the Krylov mode
  double* xc = nullptr; // stationary mode with several cycles: correction
  int last_iterations = 0;
  // Replicated form (several ranks): the hierarchy is built on the GATHERED global matrix, every rank
  // solves the whole coarse problem (one all-reduce of the zero-padded right-hand side per solve, no
  // communication inside the solve); gid = global index of the owned dofs
  bool replicated = false;
  int32_t n_global = 0;
  int32_t* gid = nullptr;       // [size_local] device
  double* d0_dinv = nullptr;    // [size_local + ghosts] this rank's rows of the level-0 inverse diagonal (dist0)
  double *gb = nullptr, *gx = nullptr; // [n_global] device
  double* h_stage = nullptr;    // pinned, [n_global]: the callback route of the all-reduce
  pmg_layout glayout = nullptr; // the replicated problem seen as one rank's (Krylov work vectors)
  // Distributed fine level (replicated form, default): level 0 -- three quarters of a cycle's work -- stays on the
  // partitioned degree-1 operator (matrix-free application with its halo exchange, the layout's own smoother data);
  // only the levels below it are replicated.  A cycle then moves ONE all-reduce of a level-1 vector (1/9 of the
  // level-0 size) instead of a level-0 one, and every rank smooths its own share of level 0 instead of all of it.
  bool dist0 = false;
  bool distributed_setup = false; // level 0 was never gathered: the fully replicated solve is not available
  DevCsr P0l, R0l; // the level 0 -> 1 transfer restricted to the owned dofs: [size_local x n1], [n1 x size_local]
  double *d0_r = nullptr, *d0_z = nullptr, *d0_q = nullptr, *d0_b = nullptr, *d0_xc = nullptr; // on the layout
  pmg_cg cg0 = nullptr; // Krylov mode on the layout (distributed dot products)
  // host copy of the hierarchy for pmg_amg_export (tests)
  std::vector<HostCsr> hA, hP;
  std::vector<double> hlmax;
  // Renewal (pmg_amg_update_values): the plan and its device arrays, made by the first call; the number of successful
  // calls; the values of hA and hP are behind the device's (pmg_amg_export downloads them); an update stopped half-way
  // (a non-positive diagonal, a failed call), after which the solves refuse the hierarchy until one succeeds; the plain
  // coarsest inverse is that of the current A_c (false: its Cholesky stopped in the last update)
  AmgRenewal* renewal = nullptr;
  long long updates = 0;
  bool host_stale = false, unusable = false, plain_valid = true;
};

namespace
{
int alloc_d(double** p, size_t n)
{
  PMG_HIP(hipMalloc(p, sizeof(double) * std::max<size_t>(n, 1)));
  // hipMemset runs on the NULL stream and returns before it has run; the caller's stream is usually a non-blocking
  // one (torch's), which the null stream does not order: a kernel issued there right behind this call could be
  // overtaken by the fill (seen once as a smoother with a zero diagonal).  Set-up code: wait for it.
  PMG_HIP(hipMemset(*p, 0, sizeof(double) * std::max<size_t>(n, 1)));
  PMG_HIP(hipStreamSynchronize(nullptr));
  return PMG_OK;
}

// The smooths of the hierarchy: k steps on a plain product (a CSR level, the fine operator), single domain.
SmoothCall smooth_call(int k, int need_r, bool x_zero)
{
  SmoothCall c;
  c.k = k, c.need_r = need_r, c.x_zero = x_zero;
  return c;
}
SmoothData<double> smooth_data(const ChebWork<double>& w, ApplyFn A, const double* dinv, int n, double lmax, double* x,
                               const double* b, hipStream_t s)
{
  SmoothData<double> d;
  d.w = w;
  d.apply[SmoothStep::PLAIN] = std::move(A);
  d.dinv = dinv, d.n = d.n_total = n, d.lmax = lmax, d.x = x, d.b = b, d.s = s;
  return d;
}

// The front level of a solve -- level 0 as the form of the hierarchy has it: a CSR level of the hierarchy (rank-local,
// fully replicated) or the partitioned matrix-free operator (distributed fine level).  The levels below it are always
// CSR levels, seen through the same struct.
struct Front
{
  ApplyFn apply;                 // the smoother's operator
  double *r, *z, *q;             // work vectors
  const double* dinv;
  int n;
  double lmax;
  std::function<int()> restrict_r; // b of the level below = R r (summed over the ranks where the front is partitioned)
  std::function<int(double*)> prolong; // x += P (x of the level below)
  // what a solve needs on top of a cycle
  std::function<int(double*, const double*, double*)> residual; // out = b - A x
  ApplyFn A = nullptr;           // the operator of the Krylov mode
  pmg_cg cg = nullptr;           // ... and its work object
  double *xc = nullptr, *rb = nullptr; // stationary mode: correction and residual
  size_t total = 0;              // length of x with its ghosts
};

Front csr_front(AmgLevel* lv, hipStream_t s)
{
  Front f;
  f.apply = [lv, s](double* in, double* out) { return csr_product<0>(lv->A, in, nullptr, out, s); };
  f.r = lv->r, f.z = lv->z, f.q = lv->q, f.dinv = lv->dinv, f.n = lv->n, f.lmax = lv->lmax;
  f.restrict_r = [lv, s] { return csr_product<0>(lv->R, lv->r, nullptr, lv[1].b, s); };
  f.prolong = [lv, s](double* x) { return csr_product<2>(lv->P, lv[1].x, nullptr, x, s); }; // x += P x_c
  return f;
}

// One V(k, k) cycle on level l, `f` its view: x = cycle(b), from a zero initial guess.
int amg_cycle(pmg_amg amg, const Front& f, int l, double* x, const double* b, hipStream_t s)
{
  const int L = (int)amg->levels.size();
  if (l == L - 1 && amg->dense_inv)
  {
    if (f.n > 0)
      dense_apply_kernel<<<(f.n * 64 + 255) / 256, 256, 0, s>>>(f.n, amg->dense_inv, b, x);
    PMG_HIP(hipGetLastError());
    return PMG_OK;
  }
  const SmoothData<double> sd = smooth_data({f.r, f.z, f.q}, f.apply, f.dinv, f.n, f.lmax, x, b, s);
  if (l == L - 1)
  {
    // a coarsest level too large to invert: smooth it harder
    return cheb_iterate(smooth_call(4 * amg->smoother_its, ResidualNone, true), sd);
  }
  AmgLevel& lc = amg->levels[l + 1];
  PMG_TRY(cheb_iterate(smooth_call(amg->smoother_its, ResidualUpdated, true), sd)); // leaves r = b - A x
  PMG_TRY(f.restrict_r());
  PMG_TRY(amg_cycle(amg, csr_front(&lc, s), l + 1, lc.x, lc.b, s));
  PMG_TRY(f.prolong(x));
  PMG_TRY(cheb_iterate(smooth_call(amg->smoother_its, ResidualNone, false), sd));
  return PMG_OK;
}

// scatter the owned entries into a zero global vector / read them back
__global__ void to_global_kernel(int n, const int32_t* __restrict__ gid, const double* __restrict__ v,
                                 double* __restrict__ g)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    g[gid[i]] = v[i];
}
__global__ void from_global_kernel(int n, const int32_t* __restrict__ gid, const double* __restrict__ g,
                                   double* __restrict__ v)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    v[i] = g[gid[i]];
}

// ---- sums over the ranks of a layout: the communicator on device memory, or the callbacks on host memory -----------
constexpr size_t ALLREDUCE_CHUNK = (size_t)1 << 24; // what fits the transports
int callback_allreduce_sum(pmg_layout l, double* h, size_t n)
{
  for (size_t o = 0; o < n; o += ALLREDUCE_CHUNK)
    if (l->allreduce(l->user, h + o, (int)std::min(ALLREDUCE_CHUNK, n - o)) != 0)
      return fail(PMG_ERR_INVALID, "allreduce callback failed");
  return PMG_OK;
}

// a host array (set-up only)
int host_allreduce_sum(pmg_layout l, double* v, size_t n, hipStream_t s)
{
  if (!l->multi_rank() || n == 0)
    return PMG_OK;
  if (!l->comm)
    return callback_allreduce_sum(l, v, n);
  Scratch d;
  PMG_TRY(d.alloc(std::min(n, ALLREDUCE_CHUNK)));
  for (size_t o = 0; o < n; o += ALLREDUCE_CHUNK)
  {
    const size_t m = std::min(ALLREDUCE_CHUNK, n - o);
    if (hipMemcpyAsync(d.p, v + o, sizeof(double) * m, hipMemcpyHostToDevice, s) != hipSuccess)
      return fail(PMG_ERR_HIP, "host_allreduce_sum: copy failed");
    PMG_TRY(comm_allreduce(l, d.p, (int)m, false, s));
    if (hipMemcpyAsync(v + o, d.p, sizeof(double) * m, hipMemcpyDeviceToHost, s) != hipSuccess)
      return fail(PMG_ERR_HIP, "host_allreduce_sum: copy failed");
    if (hipStreamSynchronize(s) != hipSuccess)
      return fail(PMG_ERR_HIP, "host_allreduce_sum: synchronise failed");
  }
  return PMG_OK;
}

// a device vector (solve time), the callbacks through the pinned stage
int device_allreduce_sum(pmg_amg amg, double* v, int n, hipStream_t s)
{
  pmg_layout l = amg->layout;
  if (l->comm)
    return comm_allreduce(l, v, n, false, s);
  if (l->allreduce)
  {
    PMG_HIP(hipMemcpyAsync(amg->h_stage, v, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    PMG_HIP(hipStreamSynchronize(s));
    PMG_TRY(callback_allreduce_sum(l, amg->h_stage, (size_t)n));
    PMG_HIP(hipMemcpyAsync(v, amg->h_stage, sizeof(double) * n, hipMemcpyHostToDevice, s));
  }
  return PMG_OK;
}

// the maximum over the ranks of a small non-negative integer (< slots, which the caller has checked)
int host_allreduce_max(pmg_layout l, int v, int slots, int* out, hipStream_t s)
{
  std::vector<double> code = unary_code(v, slots);
  PMG_TRY(host_allreduce_sum(l, code.data(), code.size(), s));
  *out = unary_max(code);
  return PMG_OK;
}

// level 0 of the hierarchy in front: the rank-local form (x, b of n entries, `total` with the ghosts; the Krylov mode
// applies the matrix-free operator) and the fully replicated one (gathered vectors, the assembled level 0)
Front assembled_front(pmg_amg amg, bool gathered, hipStream_t s)
{
  AmgLevel* l0 = &amg->levels[0];
  Front f = csr_front(l0, s);
  f.residual = [l0, s](double* x, const double* b, double* out) { return csr_product<1>(l0->A, x, b, out, s); };
  f.A = f.apply;
  if (!gathered)
  {
    pmg_laplacian op = amg->op;
    f.A = [op, s](double* in, double* out) { return laplacian_apply(op, in, out, s); };
  }
  f.cg = amg->cg, f.xc = amg->xc, f.rb = l0->b;
  f.total = gathered ? (size_t)l0->n : (size_t)amg->layout->total();
  return f;
}

// level 0 on the partitioned matrix-free operator, the levels below it replicated
Front distributed_front(pmg_amg amg, hipStream_t s)
{
  pmg_laplacian op = amg->op;
  Front f;
  f.apply = f.A = [op, s](double* in, double* out) { return laplacian_apply(op, in, out, s); };
  // The inverse diagonal of the hierarchy's OWN level-0 matrix, restricted to this rank (d0_dinv): the bound lmax
  // was computed for D^-1 A with that diagonal, and the operator's diag_inv may never have been computed or may have
  // been replaced by the caller (pmg_laplacian_set_diag_inverse) -- ADVICE r03.
  f.r = amg->d0_r, f.z = amg->d0_z, f.q = amg->d0_q, f.dinv = amg->d0_dinv;
  f.n = amg->layout->size_local, f.lmax = amg->levels[0].lmax;
  f.restrict_r = [amg, s] {
    AmgLevel& l1 = amg->levels[1];
    PMG_TRY(csr_product<0>(amg->R0l, amg->d0_r, nullptr, l1.b, s)); // this rank's share of R r
    return device_allreduce_sum(amg, l1.b, l1.n, s);                // replicated from here down
  };
  f.prolong = [amg, s](double* x) { return csr_product<2>(amg->P0l, amg->levels[1].x, nullptr, x, s); }; // owned rows
  f.residual = [amg, s](double* x, const double* b, double* out) {
    PMG_TRY(laplacian_apply(amg->op, x, amg->d0_q, s));
    launch_axpy(amg->layout->size_local, out, -1.0, amg->d0_q, b, s);
    return PMG_OK;
  };
  f.cg = amg->cg0, f.xc = amg->d0_xc, f.rb = amg->d0_b;
  f.total = (size_t)amg->layout->total();
  return f;
}

// the solve on the front's vectors: a fixed number of cycles, or CG preconditioned by one cycle
int solve(pmg_amg amg, const Front& f, double* x, const double* b, hipStream_t s)
{
  // the Krylov mode calls cg_iterate itself, so the refusals of pmg_cg_solve are repeated here: a reaction or Robin
  // term attached to the operator after pmg_amg_set_nullspace is refused, not projected (flags and a cached count)
  if (amg->nullspace == PMG_NULLSPACE_CONSTANT)
    PMG_TRY(laplacian_require_singular(amg->op, "pmg_amg_solve", s));
  if (amg->cycles > 0)
  {
    PMG_TRY(amg_cycle(amg, f, 0, x, b, s));
    for (int c = 1; c < amg->cycles; ++c) // x += cycle(b - A x)
    {
      PMG_TRY(f.residual(x, b, f.rb));
      PMG_TRY(amg_cycle(amg, f, 0, f.xc, f.rb, s));
      launch_add(f.n, x, f.xc, s);
    }
    if (amg->nullspace == PMG_NULLSPACE_CONSTANT) // (single domain: the mode is refused on the replicated forms)
      PMG_TRY(remove_mean_async(amg->layout, x, nullptr, s));
    amg->last_iterations = amg->cycles;
    return PMG_OK;
  }
  // the reference's shape: CG (<= max_iter, rtol) on the operator, preconditioned by one cycle
  PMG_HIP(hipMemsetAsync(x, 0, sizeof(double) * f.total, s)); // KSP-style zero initial guess
  const PrecondFn M = [amg, &f, s](double* z, const double* r) { return amg_cycle(amg, f, 0, z, r, s); };
  PMG_TRY(pmg_cg_set_max_iterations(f.cg, amg->max_iter));
  PMG_TRY(pmg_cg_set_tolerance(f.cg, amg->rtol));
  return cg_iterate(f.cg, f.A, nullptr, &M, false, x, b, &amg->last_iterations, s);
}
} // namespace

namespace pmg
{
pmg_layout amg_layout(pmg_amg amg) { return amg->layout; }

// stationary cycles are stream-ordered and capturable; the Krylov mode synchronises the host (and so
// does the callback route of the replicated form's all-reduce)
long long amg_capture_state(pmg_amg amg)
{
  if (amg->cycles <= 0 || (amg->replicated && !amg->layout->comm && amg->layout->allreduce))
    return -1;
  // (a renewal changes what a captured cycle has in its kernel arguments: the bounds, the coarsest inverse in use)
  return ((long long)amg->cycles << 16) ^ amg->smoother_its ^ (amg->replicated ? 1 << 30 : 0) ^ (amg->dist0 ? 1 << 29 : 0) ^
         (amg->nullspace ? 1 << 28 : 0) ^ (amg->updates << 32);
}

// x = (approximately) A^-1 b on the coarsest p-level, x zero on entry is not assumed
int amg_solve(pmg_amg amg, double* x, const double* b, hipStream_t s)
{
  Range range("pmg:amg_solve");
  PMG_REQUIRE(!amg->unusable, "pmg_amg_solve: the last pmg_amg_update_values of this hierarchy did not finish; it is "
                              "unusable until an update succeeds");
  pmg_layout l = amg->layout;
  const int n = l->size_local;
  if (amg->replicated && amg->dist0)
    return solve(amg, distributed_front(amg, s), x, b, s);
  if (amg->replicated)
  {
    // gather the right-hand side (zero-padded global vector, summed over the ranks), solve the WHOLE
    // coarse problem on every rank -- identical arithmetic everywhere, no communication inside -- and keep
    // the owned entries
    const int ng = amg->n_global;
    PMG_HIP(hipMemsetAsync(amg->gb, 0, sizeof(double) * ng, s));
    if (n > 0)
      to_global_kernel<<<(n + 255) / 256, 256, 0, s>>>(n, amg->gid, b, amg->gb);
    PMG_HIP(hipGetLastError());
    PMG_TRY(device_allreduce_sum(amg, amg->gb, ng, s));
    PMG_TRY(solve(amg, assembled_front(amg, true, s), amg->gx, amg->gb, s));
    if (n > 0)
      from_global_kernel<<<(n + 255) / 256, 256, 0, s>>>(n, amg->gid, amg->gx, x);
    PMG_HIP(hipGetLastError());
    return PMG_OK;
  }
  PMG_REQUIRE(amg->cycles == 0 || !l->multi_rank(),
              "pmg_amg: stationary cycles of a rank-local hierarchy are a single-rank solver; on several ranks "
              "use the Krylov mode or the replicated hierarchy (pmg_amg_create_replicated)");
  return solve(amg, assembled_front(amg, false, s), x, b, s);
}
} // namespace pmg

// ---- set-up: what amg_setup.hpp builds, moved to the device ------------------------------------------------------
namespace
{
// the coarsening loop on A0 and its levels on the device; level0_len: length of the first level's vectors
int build_hierarchy(pmg_amg amg, HostCsr&& A0, size_t level0_len, double theta0 = 0.08)
{
  Hierarchy H;
  PMG_TRY(accepted(coarsen(std::move(A0), theta0, H)));
  StageTimer tm;
  const int L = (int)H.A.size();
  amg->levels.resize(L);
  for (int l = 0; l < L; ++l)
  {
    AmgLevel& lv = amg->levels[l];
    lv.n = H.A[l].n;
    lv.nnz = H.A[l].nnz();
    lv.lmax = H.lmax[l];
    PMG_TRY(upload_csr(lv.A, H.A[l]));
    std::vector<double> dinv = diagonal(H.A[l]);
    for (double& v : dinv)
      v = 1.0 / v;
    PMG_TRY(to_device(&lv.dinv, dinv));
    if (l + 1 < L)
    {
      PMG_TRY(upload_csr(lv.P, H.P[l]));
      PMG_TRY(upload_csr(lv.R, transpose(H.P[l])));
    }
    const size_t len = (l == 0) ? level0_len : (size_t)lv.n;
    PMG_TRY(alloc_d(&lv.r, len));
    PMG_TRY(alloc_d(&lv.z, len));
    PMG_TRY(alloc_d(&lv.q, len));
    PMG_TRY(alloc_d(&lv.b, len)); // level 0: the residual of the second and later stationary cycles
    if (l > 0)
      PMG_TRY(alloc_d(&lv.x, len));
  }
  PMG_TRY(alloc_d(&amg->xc, level0_len));
  // coarsest level: dense inverse when small enough
  std::vector<double> inv;
  if (H.A.back().n <= 4096 && dense_spd_inverse(H.A.back(), inv))
  {
    amg->n_coarsest = H.A.back().n;
    PMG_TRY(to_device(&amg->dense_inv_plain, inv));
    amg->dense_inv = amg->dense_inv_plain;
  }
  tm.lap("upload + dense inverse");
  amg->hA = std::move(H.A);
  amg->hP = std::move(H.P);
  amg->hlmax = std::move(H.lmax);
  return PMG_OK;
}

// the vectors of a fine level that stays on the layout (distributed fine level)
int alloc_fine_vectors(pmg_amg amg)
{
  const size_t total = (size_t)amg->layout->total();
  for (double** p : {&amg->d0_r, &amg->d0_z, &amg->d0_q, &amg->d0_b, &amg->d0_xc, &amg->d0_dinv})
    PMG_TRY(alloc_d(p, total));
  return PMG_OK;
}

// the replicated problem of ng rows seen as one rank's: its layout and Krylov work object, the pinned stage of the
// callback all-reduce
int make_gathered_layout(pmg_amg amg, size_t ng)
{
  PMG_HIP(hipHostMalloc(&amg->h_stage, sizeof(double) * std::max<size_t>(ng, 1), hipHostMallocDefault));
  PMG_TRY(pmg_layout_create(&amg->glayout, (int32_t)ng, 0, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr,
                            nullptr));
  return pmg_cg_create(&amg->cg, amg->glayout);
}

// the level 0 -> 1 transfer on the owned dofs (Pl: their rows of P_0) and the Krylov object on the layout
int upload_fine_transfer(pmg_amg amg, const HostCsr& Pl)
{
  PMG_TRY(upload_csr(amg->P0l, Pl));
  PMG_TRY(upload_csr(amg->R0l, transpose(Pl)));
  PMG_TRY(pmg_cg_create(&amg->cg0, amg->layout));
  amg->dist0 = true;
  return PMG_OK;
}
} // namespace

// ---- distributed set-up (round 4): the first coarsening per rank ------------------------------------------------
// pmg_amg_create_replicated gathers the GLOBAL degree-1 matrix on every rank and coarsens it there (2.1 M rows and
// ~2.5 s per rank at 8 x 64^3).  Here no rank ever holds the global level-0 matrix:
//   * every rank aggregates its OWNED dofs (aggregates do not cross rank boundaries) and numbers its aggregates
//     globally by the smallest global dof number among their members (one all-reduce of a marker vector; no rank
//     numbers needed);
//   * the tentative prolongator of the ghost dofs (aggregate number, weight) arrives through the layout's own forward
//     scatter, so the owned rows of P_0 = (I - omega D^-1 A_0) T are smoothed with the FULL rows of A_0 (a first
//     version smoothed with the rank's own block only: 13 instead of 9 iterations on 8 ranks);
//   * A_0 P_0 on the owned rows needs the rows of P_0 of the ghost dofs: ONE layer of overlap, moved as padded
//     (column, value) tables through the same forward scatter -- any exchange mechanism, callbacks included;
//   * every rank forms its SHARE of A_1 = P_0^T A_0 P_0 (the sum over its owned fine rows) and level 1 -- about 1/9 of
//     level 0 -- is the sum of the shares, gathered on every rank as (position, value) pairs in per-rank segments of
//     one all-reduced array; the hierarchy below it is built and solved replicated, exactly as the solve phase has done
//     since round 3 (level 0 smoothed on the partitioned operator, one all-reduce of a level-1 vector per cycle);
//   * the smoothing bound of level 0 comes from a power method on the partitioned matrix-free operator.
namespace
{
// largest eigenvalue of D^-1 A of the PARTITIONED operator by the power method on the device (the operator's own halo
// exchange, the layout's reductions); the start vector depends on the global dof number only, so every partition of the
// same problem iterates on the same vector
int lambda_max_distributed(pmg_amg amg, const int64_t* global_index, const double* dinv_d, int its, double* lam,
                           hipStream_t s)
{
  pmg_layout l = amg->layout;
  const int n = l->size_local, total = l->total();
  std::vector<double> x0(total, 0.0);
  for (int i = 0; i < n; ++i)
  {
    uint64_t h = (uint64_t)global_index[i] * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    x0[i] = 0.5 + 0.5 * (double)(h >> 11) / 9007199254740992.0;
  }
  double *x = amg->d0_r, *q = amg->d0_q;
  PMG_HIP(hipMemcpyAsync(x, x0.data(), sizeof(double) * total, hipMemcpyHostToDevice, s));
  PMG_HIP(hipStreamSynchronize(s));
  double value = 1.0;
  for (int it = 0; it < its; ++it)
  {
    PMG_TRY(laplacian_apply(amg->op, x, q, s));
    launch_pointwise(n, q, q, dinv_d, s);
    double qq = 0.0, xx = 0.0;
    PMG_TRY(dot_host(l, q, q, &qq, s));
    PMG_TRY(dot_host(l, x, x, &xx, s));
    if (!(qq > 0.0) || !(xx > 0.0))
      break;
    value = std::sqrt(qq / xx);
    PMG_HIP(hipMemcpyAsync(x, q, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
    PMG_TRY(pmg_vec_scale(l, x, 1.0 / std::sqrt(qq), (pmg_stream)s));
  }
  *lam = value;
  return PMG_OK;
}
} // namespace

// one scalar per local dof moved owner -> ghost through the layout's forward scatter (host arrays of `total` entries)
static int host_scatter_fwd(pmg_layout layout, std::vector<double>& h, double* dv, hipStream_t s)
{
  const int n = layout->size_local, total = layout->total(), ng = total - n;
  PMG_HIP(hipMemcpyAsync(dv, h.data(), sizeof(double) * total, hipMemcpyHostToDevice, s));
  PMG_TRY(pmg_scatter_fwd_begin(layout, dv, (pmg_stream)s));
  PMG_TRY(pmg_scatter_fwd_end(layout, dv, (pmg_stream)s));
  if (ng > 0)
    PMG_HIP(hipMemcpyAsync(h.data() + n, dv + n, sizeof(double) * ng, hipMemcpyDeviceToHost, s));
  PMG_HIP(hipStreamSynchronize(s));
  return PMG_OK;
}

// (B) global numbers of the aggregates: rank among all aggregates' smallest global member.  number[a] = the global
// number of the rank's aggregate a, *n1 = how many there are on all ranks
static int number_aggregates(pmg_layout layout, const std::vector<int>& agg, int na, const int64_t* global_index,
                             int64_t n_global, std::vector<int64_t>& number, int* n1, hipStream_t s)
{
  number.assign(na, INT64_MAX);
  for (size_t i = 0; i < agg.size(); ++i)
    if (agg[i] >= 0)
      number[agg[i]] = std::min(number[agg[i]], global_index[i]);
  std::vector<double> marker((size_t)n_global, 0.0);
  for (int a = 0; a < na; ++a)
  {
    PMG_REQUIRE(number[a] != INT64_MAX, "pmg_amg_create_distributed: empty aggregate");
    marker[(size_t)number[a]] = 1.0;
  }
  PMG_TRY(host_allreduce_sum(layout, marker.data(), marker.size(), s));
  *n1 = 0;
  std::vector<int32_t> cid((size_t)n_global, -1);
  for (int64_t g = 0; g < n_global; ++g)
    if (marker[(size_t)g] > 0.5)
    {
      PMG_REQUIRE(marker[(size_t)g] < 1.5, "pmg_amg_create_distributed: dof %lld is owned by two ranks", (long long)g);
      cid[(size_t)g] = (*n1)++;
    }
  for (int a = 0; a < na; ++a)
    number[a] = cid[(size_t)number[a]];
  PMG_REQUIRE(*n1 > 0, "pmg_amg_create_distributed: nothing to coarsen");
  return PMG_OK;
}

// (D) Pl [n x n1] with the rows of the ghost dofs below it [total x n1]: padded (column + 1, value) tables, one slot
// per exchange through the layout's forward scatter
static int with_ghost_rows(pmg_layout layout, const HostCsr& Pl, double* dv, HostCsr& Pext, hipStream_t s)
{
  const int n = layout->size_local, total = layout->total();
  const int wloc = longest_row(Pl);
  int W = 0;
  PMG_REQUIRE(wloc >= 0 && wloc < 4096, "pmg_amg: a row with %d entries", wloc);
  PMG_TRY(host_allreduce_max(layout, wloc, 4096, &W, s));
  std::vector<double> gc((size_t)total * W, 0.0), gv((size_t)total * W, 0.0), h(total, 0.0);
  auto same = [](int i) { return i; };
  rows_to_slots(Pl, W, same, same, gc, gv);
  for (int k = 0; k < W; ++k)
    for (std::vector<double>* tab : {&gc, &gv})
    {
      for (int i = 0; i < n; ++i)
        h[i] = (*tab)[(size_t)i * W + k];
      PMG_TRY(host_scatter_fwd(layout, h, dv, s));
      for (int g = n; g < total; ++g)
        (*tab)[(size_t)g * W + k] = h[g];
    }
  long long bad = -1;
  Pext = rows_from_slots(gc, gv, total, W, Pl.m, &bad);
  PMG_REQUIRE(bad < 0, "pmg_amg_create_distributed: a ghost's prolongator row names aggregate %d", (int)bad);
  return PMG_OK;
}

// (F) level 1 on every rank = the sum of the shares: (row * n1 + column, value) pairs in the rank's own segment of one
// long array (segments ordered by the rank's smallest owned global dof number: no rank numbers needed), summed over
// the ranks, then assembled row by row
static int gather_level1(pmg_layout layout, HostCsr&& share, const int64_t* global_index, int64_t n_global, HostCsr& A1,
                         hipStream_t s)
{
  const int n = layout->size_local, n1 = share.n;
  int64_t mykey = INT64_MAX;
  for (int i = 0; i < n; ++i)
    mykey = std::min(mykey, global_index[i]);
  PMG_REQUIRE(n == 0 || mykey != INT64_MAX, "pmg_amg_create_distributed: no owned dof");
  std::vector<double> marker((size_t)n_global, 0.0);
  if (n > 0)
    marker[(size_t)mykey] = (double)share.nnz() + 0.25; // + 0.25: a rank with an empty share still marks its key
  PMG_TRY(host_allreduce_sum(layout, marker.data(), marker.size(), s));
  long long offset = 0, totalcnt = 0;
  segment_of(marker, mykey, &offset, &totalcnt);
  std::vector<double>().swap(marker);
  std::vector<double> keys((size_t)totalcnt, 0.0), vals((size_t)totalcnt, 0.0);
  write_segment(share, offset, keys, vals);
  share = HostCsr();
  PMG_TRY(host_allreduce_sum(layout, keys.data(), keys.size(), s));
  PMG_TRY(host_allreduce_sum(layout, vals.data(), vals.size(), s));
  return accepted(rows_from_segments(keys, vals, n1, A1));
}

// The distributed set-up from the owned rows A0 [n x total] of level 0, steps (A) to (F) of the comment above.
static int amg_create_distributed_tail(pmg_amg amg, HostCsr&& A0, const int64_t* global_index, int64_t n_global,
                                       hipStream_t s)
{
  pmg_layout layout = amg->layout;
  const int n = layout->size_local, total = layout->total();
  amg->distributed_setup = true;
  StageTimer tm;
  const std::vector<double> d = diagonal(A0); // the diagonal of the owned rows: the smoother's D
  for (int i = 0; i < n; ++i)
    PMG_REQUIRE(d[i] > 0.0, "pmg_amg_create_distributed: row %d has no positive diagonal", i);
  // what the solve needs on the layout, and the smoothing bound of level 0 first (the prolongator uses it)
  PMG_TRY(alloc_fine_vectors(amg));
  std::vector<double> dinv(total, 1.0);
  for (int i = 0; i < n; ++i)
    dinv[i] = 1.0 / d[i];
  PMG_HIP(hipMemcpy(amg->d0_dinv, dinv.data(), sizeof(double) * dinv.size(), hipMemcpyHostToDevice));
  double lam0 = 1.0;
  PMG_TRY(lambda_max_distributed(amg, global_index, amg->d0_dinv, 20, &lam0, s));
  const double rho0 = 1.05 * lam0;
  tm.lap("level-0 bound (power method on the partitioned operator)");

  // (A) aggregation of the OWNED dofs on the rank's own block (aggregates do not cross rank boundaries)
  std::vector<int> agg;
  const int na = aggregate(take_rows<int>(A0, nullptr, n, n), d, 0.08, agg);
  tm.lap("aggregation of the owned dofs");
  std::vector<int64_t> number;
  int n1 = 0;
  PMG_TRY(number_aggregates(layout, agg, na, global_index, n_global, number, &n1, s));
  tm.lap("global aggregate numbers");

  // (C) the tentative prolongator on owned AND ghost dofs (aggregate number + 1 and weight 1 / sqrt(size): one scalar
  // exchange each), then the owned rows of P_0 = (I - 4 / (3 rho) D^-1 A_0) T with the FULL rows of A_0 -- ghost
  // couplings included, so the columns of a rank's rows may be neighbours' aggregates
  Scratch dv;
  PMG_TRY(dv.alloc((size_t)total));
  std::vector<double> tcol(total, 0.0), tval = tentative_weights(agg, na);
  tval.resize(total, 0.0);
  for (int i = 0; i < n; ++i)
    if (agg[i] >= 0)
      tcol[i] = (double)(number[agg[i]] + 1);
  PMG_TRY(host_scatter_fwd(layout, tcol, dv.p, s));
  PMG_TRY(host_scatter_fwd(layout, tval, dv.p, s));
  std::vector<int> cagg(total);
  for (int j = 0; j < total; ++j)
    cagg[j] = tcol[j] > 0.5 ? (int)(tcol[j] - 0.5) : -1;
  const HostCsr Pl = smoothed_prolongator(A0, d, cagg, tval, n1, 4.0 / (3.0 * rho0)); // [n x n1], global coarse columns
  tm.lap("smoothed prolongator (owned rows)");

  HostCsr Pext; // (D)
  PMG_TRY(with_ghost_rows(layout, Pl, dv.p, Pext, s));
  tm.lap("prolongator rows of the ghosts (one layer of overlap)");

  // (E) this rank's SHARE of A_1 = P_0^T A_0 P_0: sum over its owned fine rows i of P_i^T (A_0 P_0)_i -- entries in the
  // rows of its own aggregates and, along the interfaces, of its neighbours'
  HostCsr A1part = spgemm(transpose(Pl), spgemm(A0, Pext)); // [n1 x n1]
  tm.lap("Galerkin product of the owned rows");
  HostCsr A1;
  PMG_TRY(gather_level1(layout, std::move(A1part), global_index, n_global, A1, s));
  tm.lap("gather of level 1 (sum of the ranks' shares)");

  PMG_TRY(build_hierarchy(amg, std::move(A1), (size_t)n1, 0.04)); // level 1's threshold: half of level 0's 0.08
  // (build_hierarchy leaves the solution vector of ITS first level to the caller; here that level is level 1 of the
  // solve and needs one of its own)
  PMG_TRY(alloc_d(&amg->levels[0].x, (size_t)n1));
  // level 0 in front of it: lives on the layout, has no assembled matrix on the device
  AmgLevel l0;
  l0.n = n;
  l0.nnz = A0.nnz();
  l0.lmax = rho0;
  amg->levels.insert(amg->levels.begin(), l0);
  amg->hA.insert(amg->hA.begin(), std::move(A0));
  amg->hP.insert(amg->hP.begin(), Pl);
  amg->hlmax.insert(amg->hlmax.begin(), rho0);
  PMG_TRY(upload_fine_transfer(amg, Pl));
  PMG_TRY(make_gathered_layout(amg, (size_t)std::max(n1, 1)));
  tm.lap("hierarchy below level 1 + uploads");
  return PMG_OK;
}

struct Level0Inputs // host copies of what level 0 is assembled from
{
  std::vector<int32_t> dofmap, cells; // cells: the ones the operator lists (both cell lists), from its patches
  std::vector<int8_t> bc;
  std::vector<double> kappa, G, react;
};
static int download_operator(pmg_laplacian op, pmg_stream stream, Level0Inputs& h)
{
  const LaplacianInputs in = laplacian_inputs(op);
  pmg_layout layout = laplacian_layout(op);
  const int n = layout->size_local, total = layout->total();
  hipStream_t s = S(stream);
  h.dofmap.resize((size_t)in.ncells * 8);
  h.bc.resize(total);
  h.kappa.resize(in.ncells);
  h.G.resize((size_t)in.ncells * 8 * 6);
  Scratch dG;
  PMG_TRY(dG.alloc(h.G.size()));
  PMG_TRY(pmg_laplacian_get_geometry(op, dG.p, stream));
  if (!h.G.empty() && hipMemcpyAsync(h.G.data(), dG.p, sizeof(double) * h.G.size(), hipMemcpyDeviceToHost, s) != hipSuccess)
    return fail(PMG_ERR_HIP, "pmg_amg_create: copy of the geometry tensor failed");
  if (hipStreamSynchronize(s) != hipSuccess)
    return fail(PMG_ERR_HIP, "pmg_amg_create: synchronise failed");
  if (in.ncells > 0)
  {
    PMG_HIP(hipMemcpy(h.dofmap.data(), in.dofmap, sizeof(int32_t) * h.dofmap.size(), hipMemcpyDeviceToHost));
    PMG_HIP(hipMemcpy(h.kappa.data(), in.kappa, sizeof(double) * h.kappa.size(), hipMemcpyDeviceToHost));
  }
  if (total > 0)
    PMG_HIP(hipMemcpy(h.bc.data(), in.bc, sizeof(int8_t) * h.bc.size(), hipMemcpyDeviceToHost));
  for (int32_t c : *laplacian_patches(op).pcell_h)
    if (c >= 0)
      h.cells.push_back(c);
  if (const double* dreact = laplacian_reaction(op))
  {
    h.react.resize(n);
    if (n > 0)
      PMG_HIP(hipMemcpy(h.react.data(), dreact, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  }
  return PMG_OK;
}

// The replicated gather: every rank contributes its owned rows with global column ids in fixed-width slots of a zero
// global table; the sum over the ranks is the global matrix, which replaces A0.
static int gather_level0(pmg_layout layout, HostCsr& A0, const int64_t* global_index, int64_t n_global, hipStream_t s)
{
  const int wloc = longest_row(A0);
  int W = 1;
  PMG_REQUIRE(wloc < 256, "pmg_amg_create_replicated: a row with %d entries", wloc);
  PMG_TRY(host_allreduce_max(layout, wloc, 256, &W, s));
  W = std::max(W, 1);
  const size_t ng = (size_t)n_global;
  std::vector<double> gc(ng * W, 0.0), gv(ng * W, 0.0);
  auto global = [global_index](int i) { return global_index[i]; };
  rows_to_slots(A0, W, global, global, gc, gv);
  PMG_TRY(host_allreduce_sum(layout, gc.data(), gc.size(), s));
  PMG_TRY(host_allreduce_sum(layout, gv.data(), gv.size(), s));
  long long bad = -1;
  A0 = rows_from_slots(gc, gv, (int)ng, W, (int)ng, &bad);
  PMG_REQUIRE(bad < 0, "pmg_amg_create_replicated: a gathered row names column %lld", bad);
  PMG_REQUIRE(empty_row(A0) < 0, "pmg_amg_create_replicated: global dof %lld is owned by no rank", (long long)empty_row(A0));
  return PMG_OK;
}

// `global_index` == nullptr: the hierarchy of this rank's own block.  Otherwise the replicated form.
// distributed_setup: the first coarsening per rank, only the levels below it gathered (pmg_amg_create_distributed)
static int amg_create(pmg_amg* out, pmg_laplacian op, const int64_t* global_index, int64_t n_global,
                      pmg_stream stream, bool distributed_setup = false)
{
  PMG_REQUIRE(out && op, "pmg_amg_create: NULL argument");
  const int degree = laplacian_inputs(op).degree;
  PMG_REQUIRE(degree == 1, "pmg_amg_create: the operator must have degree 1 (it has degree %d)", degree);
  hipStream_t s = S(stream);
  pmg_layout layout = laplacian_layout(op);
  const int n = layout->size_local, total = layout->total();
  const bool replicated = global_index != nullptr;
  if (replicated)
  {
    PMG_REQUIRE(n_global >= n && n_global < ((int64_t)1 << 31), "pmg_amg_create_replicated: bad global size");
    for (int i = 0; i < total; ++i)
      PMG_REQUIRE(global_index[i] >= 0 && global_index[i] < n_global,
                  "pmg_amg_create_replicated: global index %lld out of range", (long long)global_index[i]);
  }
  auto* amg = new pmg_amg_s;
  HandleGuard<pmg_amg> guard(amg, pmg_amg_destroy);
  amg->op = op;
  amg->layout = layout;
  amg->replicated = replicated;
  amg->n_global = replicated ? (int32_t)n_global : 0;

  StageTimer tmc;
  // ---- level 0: assemble the owned block of the degree-1 stiffness matrix ----
  HostCsr A0;
  {
    Level0Inputs h;
    PMG_TRY(download_operator(op, stream, h));
    A0 = assemble_level0(h.dofmap, h.G, h.kappa, h.bc, h.cells, h.react.empty() ? nullptr : h.react.data(), n, total,
                         replicated);
  }
  tmc.lap("level-0 assembly");
  if (replicated && distributed_setup)
  {
    PMG_TRY(amg_create_distributed_tail(amg, std::move(A0), global_index, n_global, s));
    tmc.lap("distributed first coarsening + hierarchy below it");
    PMG_HIP(hipStreamSynchronize(s));
    *out = guard.release();
    return PMG_OK;
  }
  size_t level0_len = (size_t)total;
  if (replicated)
  {
    PMG_TRY(gather_level0(layout, A0, global_index, n_global, s));
    level0_len = (size_t)n_global;
    const std::vector<int32_t> gid(global_index, global_index + n);
    PMG_TRY(to_device(&amg->gid, gid));
    PMG_TRY(alloc_d(&amg->gb, level0_len));
    PMG_TRY(alloc_d(&amg->gx, level0_len));
    PMG_TRY(make_gathered_layout(amg, level0_len));
  }
  else
    PMG_TRY(pmg_cg_create(&amg->cg, layout));
  tmc.lap("gather (replicated form)");
  PMG_TRY(build_hierarchy(amg, std::move(A0), level0_len));
  if (replicated && amg->levels.size() >= 2)
  {
    // the distributed fine level: the rows of P_0 of this rank's owned dofs, in the layout's numbering, and the owned
    // rows of the assembled level-0 diagonal (levels[0].dinv is indexed by global row)
    PMG_TRY(alloc_fine_vectors(amg));
    if (n > 0)
      from_global_kernel<<<(n + 255) / 256, 256, 0, s>>>(n, amg->gid, amg->levels[0].dinv, amg->d0_dinv);
    PMG_HIP(hipGetLastError());
    PMG_TRY(upload_fine_transfer(amg, take_rows(amg->hP[0], global_index, n, amg->hP[0].m)));
  }
  PMG_HIP(hipStreamSynchronize(s));
  *out = guard.release();
  return PMG_OK;
}

extern "C" int pmg_amg_create(pmg_amg* out, pmg_laplacian op, pmg_stream stream)
{
  return amg_create(out, op, nullptr, 0, stream);
}

extern "C" int pmg_amg_create_replicated(pmg_amg* out, pmg_laplacian op, const int64_t* global_index,
                                         int64_t n_global, pmg_stream stream)
{
  PMG_REQUIRE(global_index, "pmg_amg_create_replicated: NULL global index");
  return amg_create(out, op, global_index, n_global, stream);
}

extern "C" int pmg_amg_create_distributed(pmg_amg* out, pmg_laplacian op, const int64_t* global_index,
                                          int64_t n_global, pmg_stream stream)
{
  PMG_REQUIRE(global_index, "pmg_amg_create_distributed: NULL global index");
  return amg_create(out, op, global_index, n_global, stream, true);
}

// ---- renewal: every value of the hierarchy recomputed on the device, the aggregates kept ---------------------------
// pmg_amg_update_values.  The plan and the row routines are in amg_renew.hpp (free of HIP, run whole on the CPU by
// tests/host/amg_update_check.cpp); here are the kernels around the routines -- a sub-wavefront per output row, the row
// in an LDS copy -- the power method with its sums in a fixed order (grid partials, a one-block finish), and the
// sequence of a call.  A level's bound goes to the host once per call (omega = 4 / (3 rho) and the smoother's bound are
// kernel arguments); the coarsest inverse stays the host's Cholesky.
struct AmgRenewal
{
  amg_renew::RenewPlan plan;
  int *inc_off = nullptr, *inc_cell = nullptr, *inc_loc = nullptr; // level 0: the rows' incidences
  int cap0 = 1;
  double* Gc = nullptr; // [cells][8][6]: the operator's tensor in the order the row routine reads it, refilled per call
  struct Level
  {
    int* agg = nullptr;
    double* t = nullptr;
    DevCsr AP;
    int* rperm = nullptr;
    double* x0 = nullptr;
    int wP = 2, wAP = 2, wA = 2, capAP = 1, capA = 1; // lanes per row and longest row of the three kernels
  };
  std::vector<Level> lv;
  double* partials = nullptr; // [3][blocks of the largest level's power step]
  double* scal = nullptr;     // lambda, norm, rows without a positive diagonal, stopped
  double* h_scal = nullptr;   // pinned copy
  AmgRenewal() = default;
  AmgRenewal(const AmgRenewal&) = delete;
  ~AmgRenewal()
  {
    for (void* p : {(void*)inc_off, (void*)inc_cell, (void*)inc_loc, (void*)Gc, (void*)partials, (void*)scal})
      (void)hipFree(p);
    if (h_scal)
      (void)hipHostFree(h_scal);
    for (Level& l : lv)
    {
      (void)hipFree(l.agg);
      (void)hipFree(l.t);
      (void)hipFree(l.rperm);
      (void)hipFree(l.x0);
      free_csr(l.AP);
    }
  }
};

static int nullspace_inverse(pmg_amg amg, std::vector<double>& inv);

namespace
{
// W lanes (a power of two <= 32) share a row, blockDim.x / W rows per block, one LDS copy of `cap` doubles per row
struct RowLaunch
{
  int W = 2, cap = 1;
  unsigned blocks = 0, threads = 0;
  size_t lds = 0;
};
RowLaunch row_launch(int n, int W, int cap)
{
  RowLaunch r;
  r.W = W;
  r.cap = std::max(cap, 1);
  const int groups =
      (int)std::max<size_t>(1, std::min<size_t>(256 / W, amg_renew::ROW_COPY_BYTES / (sizeof(double) * r.cap)));
  r.threads = (unsigned)(W * groups);
  r.blocks = (unsigned)((n + groups - 1) / groups);
  r.lds = sizeof(double) * (size_t)r.cap * groups;
  return r;
}

__global__ void __launch_bounds__(256)
    renew_level0_kernel(int n, int W, int cap, const int* __restrict__ rp, const int* __restrict__ ci,
                        double* __restrict__ vals, double* __restrict__ dinv, const int* __restrict__ inc_off,
                        const int* __restrict__ inc_cell, const int* __restrict__ inc_loc,
                        const int32_t* __restrict__ dofmap, const double* __restrict__ Gc,
                        const double* __restrict__ kappa, const int8_t* __restrict__ bc, const double* __restrict__ react)
{
  extern __shared__ double renew_rows[];
  const int groups = blockDim.x / W, g = threadIdx.x / W, sub = threadIdx.x - g * W;
  const int row = blockIdx.x * groups + g;
  if (row >= n)
    return;
  double* acc = renew_rows + (size_t)g * cap;
  amg_renew::level0_row(row, sub, W, rp, ci, inc_off, inc_cell, inc_loc, dofmap, Gc, kappa, bc, react, acc);
  amg_renew::store_row(row, sub, W, rp, ci, acc, vals, dinv);
}

// C = A B on the pattern of C; dinv (optional): the inverse diagonal of C
__global__ void __launch_bounds__(256)
    renew_product_kernel(int n, int W, int cap, const int* __restrict__ Arp, const int* __restrict__ Aci,
                         const double* __restrict__ Av, const int* __restrict__ Brp, const int* __restrict__ Bci,
                         const double* __restrict__ Bv, const int* __restrict__ Crp, const int* __restrict__ Cci,
                         double* __restrict__ Cv, double* __restrict__ dinv)
{
  extern __shared__ double renew_rows[];
  const int groups = blockDim.x / W, g = threadIdx.x / W, sub = threadIdx.x - g * W;
  const int row = blockIdx.x * groups + g;
  if (row >= n)
    return;
  double* acc = renew_rows + (size_t)g * cap;
  amg_renew::product_row(row, sub, W, Arp, Aci, Av, Brp, Bci, Bv, Crp, Cci, acc);
  amg_renew::store_row(row, sub, W, Crp, Cci, acc, Cv, dinv);
}

__global__ void __launch_bounds__(256)
    renew_prolongator_kernel(int n, int W, const int* __restrict__ Arp, const int* __restrict__ Aci,
                             const double* __restrict__ Av, const int* __restrict__ agg, const double* __restrict__ t,
                             double omega, const int* __restrict__ Prp, const int* __restrict__ Pci,
                             double* __restrict__ Pv)
{
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int row = (int)(gid / W), sub = (int)(gid - (long long)row * W);
  if (row < n)
    amg_renew::prolongator_row(row, sub, W, Arp, Aci, Av, agg, t, omega, Prp, Pci, Pv);
}

// R = P^T: its values through the planned permutation
__global__ void __launch_bounds__(256)
    renew_gather_kernel(long long nnz, const int* __restrict__ from, const double* __restrict__ Pv, double* __restrict__ Rv)
{
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < nnz)
    Rv[k] = Pv[from[k]];
}

// One step of the power method on D^-1 A: y = D^-1 A x and the block's partials of y . y, x . x and of the number of
// rows without a positive diagonal (dinv = 0), each a tree over the block's 256 slots: a fixed order.
template <int TPR>
__global__ void __launch_bounds__(256)
    renew_power_kernel(int n, const int* __restrict__ rp, const int* __restrict__ ci, const double* __restrict__ v,
                       const double* __restrict__ dinv, const double* __restrict__ x, double* __restrict__ y,
                       double* __restrict__ partials)
{
  __shared__ double red[3][256];
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int row = gid / TPR, sub = gid % TPR;
  double acc = row < n ? amg_renew::row_dot(row, sub, TPR, rp, ci, v, x) : 0.0;
#pragma unroll
  for (int off = TPR / 2; off > 0; off >>= 1)
    acc += __shfl_down(acc, off, TPR);
  double yy = 0.0, xx = 0.0, bad = 0.0;
  if (row < n && sub == 0)
  {
    const double di = dinv[row], yi = acc * di, xi = x[row];
    y[row] = yi;
    yy = yi * yi;
    xx = xi * xi;
    bad = di > 0.0 ? 0.0 : 1.0;
  }
  red[0][threadIdx.x] = yy;
  red[1][threadIdx.x] = xx;
  red[2][threadIdx.x] = bad;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1)
  {
    if ((int)threadIdx.x < off)
      for (int c = 0; c < 3; ++c)
        red[c][threadIdx.x] += red[c][threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x < 3)
    partials[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = red[threadIdx.x][0];
}

// ... the finish, one block: scal = {lambda = |y| / |x|, |y|, bad rows, stopped}.  Where |y| is not positive the
// iteration stops with lambda = 1 (lambda_max_jacobi's answer) and the later steps leave scal alone.
__global__ void __launch_bounds__(256)
    renew_power_finish_kernel(int nb, const double* __restrict__ partials, double* __restrict__ scal)
{
  __shared__ double red[3][256];
  for (int c = 0; c < 3; ++c)
  {
    double a = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256)
      a += partials[(size_t)c * nb + b];
    red[c][threadIdx.x] = a;
  }
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1)
  {
    if ((int)threadIdx.x < off)
      for (int c = 0; c < 3; ++c)
        red[c][threadIdx.x] += red[c][threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0 && scal[3] == 0.0)
  {
    const double nrm = sqrt(red[0][0]);
    scal[2] = red[2][0];
    if (!(nrm > 0.0))
    {
      scal[0] = 1.0;
      scal[3] = 1.0;
    }
    else
    {
      scal[0] = nrm / sqrt(red[1][0]);
      scal[1] = nrm;
    }
  }
}

__global__ void __launch_bounds__(256)
    renew_power_scale_kernel(int n, const double* __restrict__ y, const double* __restrict__ scal, double* __restrict__ x)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && scal[3] == 0.0)
    x[i] = y[i] / scal[1];
}

unsigned power_blocks(const DevCsr& A) { return (unsigned)(((long long)A.n * A.tpr + 255) / 256); }

// 20 power steps on D^-1 A_l from the level's start vector, in the level's own work vectors
int renew_power_bound(pmg_amg amg, int l, double* lam, hipStream_t s)
{
  AmgRenewal& R = *amg->renewal;
  AmgLevel& lv = amg->levels[l];
  const DevCsr& A = lv.A;
  *lam = 1.0;
  if (A.n == 0)
    return PMG_OK;
  double *x = lv.z, *y = lv.q;
  const unsigned nb = power_blocks(A), nv = (unsigned)((A.n + 255) / 256);
  PMG_HIP(hipMemcpyAsync(x, R.lv[l].x0, sizeof(double) * A.n, hipMemcpyDeviceToDevice, s));
  PMG_HIP(hipMemsetAsync(R.scal, 0, sizeof(double) * 4, s));
  for (int it = 0; it < 20; ++it)
  {
    switch (A.tpr)
    {
    case 2: renew_power_kernel<2><<<nb, 256, 0, s>>>(A.n, A.rp, A.ci, A.v, lv.dinv, x, y, R.partials); break;
    case 4: renew_power_kernel<4><<<nb, 256, 0, s>>>(A.n, A.rp, A.ci, A.v, lv.dinv, x, y, R.partials); break;
    case 8: renew_power_kernel<8><<<nb, 256, 0, s>>>(A.n, A.rp, A.ci, A.v, lv.dinv, x, y, R.partials); break;
    case 16: renew_power_kernel<16><<<nb, 256, 0, s>>>(A.n, A.rp, A.ci, A.v, lv.dinv, x, y, R.partials); break;
    default: renew_power_kernel<32><<<nb, 256, 0, s>>>(A.n, A.rp, A.ci, A.v, lv.dinv, x, y, R.partials); break;
    }
    renew_power_finish_kernel<<<1, 256, 0, s>>>((int)nb, R.partials, R.scal);
    renew_power_scale_kernel<<<nv, 256, 0, s>>>(A.n, y, R.scal, x);
  }
  PMG_HIP(hipGetLastError());
  PMG_HIP(hipMemcpyAsync(R.h_scal, R.scal, sizeof(double) * 4, hipMemcpyDeviceToHost, s));
  PMG_HIP(hipStreamSynchronize(s));
  if (R.h_scal[2] > 0.0)
    return fail(PMG_ERR_NUMERIC, "pmg_amg_update_values: non-positive diagonal entry on level %d", l);
  *lam = R.h_scal[0];
  return PMG_OK;
}

// the values of hA and hP as the device has them (their patterns are the device's)
int refresh_host(pmg_amg amg)
{
  for (size_t l = 0; l < amg->hA.size(); ++l)
    if (amg->hA[l].nnz() > 0)
      PMG_HIP(hipMemcpy(amg->hA[l].v.data(), amg->levels[l].A.v, sizeof(double) * amg->hA[l].v.size(),
                        hipMemcpyDeviceToHost));
  for (size_t l = 0; l < amg->hP.size(); ++l)
    if (amg->hP[l].nnz() > 0)
      PMG_HIP(hipMemcpy(amg->hP[l].v.data(), amg->levels[l].P.v, sizeof(double) * amg->hP[l].v.size(),
                        hipMemcpyDeviceToHost));
  amg->host_stale = false;
  return PMG_OK;
}

// a device matrix on a new (larger) pattern: the old arrays are freed
int replace_csr(DevCsr& d, const HostCsr& pattern)
{
  free_csr(d);
  return upload_csr(d, pattern);
}

// The first call: the plan (host), its device arrays, and the hierarchy's matrices moved to the structural patterns
// where those are larger than the created ones.
int renewal_plan(pmg_amg amg)
{
  pmg_laplacian op = amg->op;
  const LaplacianInputs in = laplacian_inputs(op);
  std::vector<int32_t> dofmap((size_t)in.ncells * 8), cells;
  if (in.ncells > 0)
    PMG_HIP(hipMemcpy(dofmap.data(), in.dofmap, sizeof(int32_t) * dofmap.size(), hipMemcpyDeviceToHost));
  for (int32_t c : *laplacian_patches(op).pcell_h)
    if (c >= 0)
      cells.push_back(c);
  std::unique_ptr<AmgRenewal> R(new AmgRenewal);
  PMG_TRY(accepted(amg_renew::plan_renewal(amg->hA, dofmap, cells, R->plan)));
  const amg_renew::RenewPlan& plan = R->plan;
  const int L = (int)plan.A.size();
  PMG_REQUIRE(L == (int)amg->levels.size(), "pmg_amg_update_values: internal: the plan has %d levels", L);
  PMG_TRY(to_device(&R->inc_off, plan.inc_off));
  PMG_TRY(to_device(&R->inc_cell, plan.inc_cell));
  PMG_TRY(to_device(&R->inc_loc, plan.inc_loc));
  R->cap0 = longest_row(plan.A[0]);
  PMG_HIP(hipMalloc(&R->Gc, sizeof(double) * 48 * std::max<size_t>((size_t)in.ncells, 1)));
  R->lv.resize(L);
  for (int l = 0; l < L; ++l)
  {
    AmgRenewal::Level& rl = R->lv[l];
    PMG_TRY(to_device(&rl.x0, plan.x0[l]));
    if (l + 1 == L)
      break;
    const amg_renew::RenewLevel& pl = plan.lv[l];
    PMG_TRY(to_device(&rl.agg, pl.agg));
    PMG_TRY(to_device(&rl.t, pl.t));
    PMG_TRY(to_device(&rl.rperm, pl.rperm));
    PMG_TRY(upload_csr(rl.AP, pl.AP));
    rl.wP = amg_renew::lanes_for(pl.P);
    rl.wAP = amg_renew::lanes_for(pl.P); // lanes take the entries of a row of the right factor
    rl.wA = amg_renew::lanes_for(pl.AP);
    rl.capAP = longest_row(pl.AP);
    rl.capA = longest_row(plan.A[l + 1]);
  }
  PMG_HIP(hipMalloc(&R->scal, sizeof(double) * 4));
  PMG_HIP(hipHostMalloc(&R->h_scal, sizeof(double) * 4, hipHostMallocDefault));
  // the hierarchy on the structural patterns (a level whose pattern the creation already had keeps its arrays)
  for (int l = 0; l < L; ++l)
  {
    AmgLevel& lv = amg->levels[l];
    if (plan.A[l].nnz() != amg->hA[l].nnz())
      PMG_TRY(replace_csr(lv.A, plan.A[l]));
    amg->hA[l] = plan.A[l];
    lv.nnz = plan.A[l].nnz();
    if (l + 1 < L)
    {
      if (plan.lv[l].P.nnz() != amg->hP[l].nnz())
      {
        PMG_TRY(replace_csr(lv.P, plan.lv[l].P));
        PMG_TRY(replace_csr(lv.R, plan.lv[l].R));
      }
      amg->hP[l] = plan.lv[l].P;
    }
  }
  amg->host_stale = true;
  unsigned nb = 1;
  for (const AmgLevel& lv : amg->levels)
    nb = std::max(nb, power_blocks(lv.A));
  PMG_HIP(hipMalloc(&R->partials, sizeof(double) * 3 * nb));
  amg->renewal = R.release();
  return PMG_OK;
}

// every call: the values, level by level
int renewal_values(pmg_amg amg, hipStream_t s)
{
  AmgRenewal& R = *amg->renewal;
  const amg_renew::RenewPlan& plan = R.plan;
  pmg_laplacian op = amg->op;
  const int L = (int)amg->levels.size();
  StageTimer tm;
  tm.tag = "update";
  auto lap = [&](const char* what) {
    if (tm.on)
      (void)hipStreamSynchronize(s);
    tm.lap(what);
  };
  {
    AmgLevel& l0 = amg->levels[0];
    PMG_TRY(laplacian_geometry_ascending(op, R.Gc, s));
    lap("tensor in point order");
    if (l0.n > 0)
    {
      const RowLaunch k = row_launch(l0.n, 8, R.cap0);
      renew_level0_kernel<<<k.blocks, k.threads, k.lds, s>>>(l0.n, k.W, k.cap, l0.A.rp, l0.A.ci, l0.A.v, l0.dinv,
                                                             R.inc_off, R.inc_cell, R.inc_loc, op->dofmap, R.Gc,
                                                             op->kappa, op->bc, laplacian_reaction(op));
      PMG_HIP(hipGetLastError());
    }
    lap("level-0 values");
  }
  for (int l = 0; l < L; ++l)
  {
    AmgLevel& lv = amg->levels[l];
    double lam = 1.0;
    PMG_TRY(renew_power_bound(amg, l, &lam, s));
    lv.lmax = amg->hlmax[l] = 1.05 * lam;
    lap("power method");
    if (l + 1 == L)
      break;
    AmgLevel& lc = amg->levels[l + 1];
    const AmgRenewal::Level& rl = R.lv[l];
    const double omega = 4.0 / (3.0 * lv.lmax);
    if (lv.n > 0)
    {
      const unsigned blocks = (unsigned)(((long long)lv.n * rl.wP + 255) / 256);
      renew_prolongator_kernel<<<blocks, 256, 0, s>>>(lv.n, rl.wP, lv.A.rp, lv.A.ci, lv.A.v, rl.agg, rl.t, omega,
                                                      lv.P.rp, lv.P.ci, lv.P.v);
      const long long nnz = plan.lv[l].P.nnz();
      if (nnz > 0)
        renew_gather_kernel<<<(unsigned)((nnz + 255) / 256), 256, 0, s>>>(nnz, rl.rperm, lv.P.v, lv.R.v);
      PMG_HIP(hipGetLastError());
      lap("smoothed prolongator, transpose");
      const RowLaunch k = row_launch(lv.n, rl.wAP, rl.capAP);
      renew_product_kernel<<<k.blocks, k.threads, k.lds, s>>>(lv.n, k.W, k.cap, lv.A.rp, lv.A.ci, lv.A.v, lv.P.rp,
                                                              lv.P.ci, lv.P.v, rl.AP.rp, rl.AP.ci, rl.AP.v, nullptr);
      PMG_HIP(hipGetLastError());
      lap("A P");
    }
    if (lc.n > 0)
    {
      const RowLaunch k = row_launch(lc.n, rl.wA, rl.capA);
      renew_product_kernel<<<k.blocks, k.threads, k.lds, s>>>(lc.n, k.W, k.cap, lv.R.rp, lv.R.ci, lv.R.v, rl.AP.rp,
                                                              rl.AP.ci, rl.AP.v, lc.A.rp, lc.A.ci, lc.A.v, lc.dinv);
      PMG_HIP(hipGetLastError());
      lap("R (A P)");
    }
  }
  // the coarsest inverse(s): the host's Cholesky of the downloaded A_c, uploaded into the allocations that exist
  PMG_HIP(hipStreamSynchronize(s));
  amg->host_stale = true;
  HostCsr& Ac = amg->hA.back();
  if (Ac.n <= 4096)
  {
    if (amg->dense_inv_null)
      PMG_TRY(refresh_host(amg)); // the restricted ones go through every renewed transfer
    else if (Ac.nnz() > 0)
      PMG_HIP(hipMemcpy(Ac.v.data(), amg->levels.back().A.v, sizeof(double) * Ac.v.size(), hipMemcpyDeviceToHost));
    std::vector<double> inv;
    amg->plain_valid = dense_spd_inverse(Ac, inv);
    if (amg->plain_valid)
    {
      amg->n_coarsest = Ac.n;
      if (!amg->dense_inv_plain)
        PMG_TRY(to_device(&amg->dense_inv_plain, inv));
      else if (!inv.empty())
        PMG_HIP(hipMemcpy(amg->dense_inv_plain, inv.data(), sizeof(double) * inv.size(), hipMemcpyHostToDevice));
    }
    if (amg->dense_inv_null)
    {
      PMG_TRY(nullspace_inverse(amg, inv));
      if (!inv.empty())
        PMG_HIP(hipMemcpy(amg->dense_inv_null, inv.data(), sizeof(double) * inv.size(), hipMemcpyHostToDevice));
    }
    amg->dense_inv = amg->nullspace == PMG_NULLSPACE_CONSTANT ? amg->dense_inv_null
                     : amg->plain_valid                       ? amg->dense_inv_plain
                                                              : nullptr;
  }
  lap("coarsest inverse");
  return PMG_OK;
}
} // namespace

extern "C" int pmg_amg_update_values(pmg_amg amg, pmg_stream stream)
{
  PMG_REQUIRE(amg, "pmg_amg_update_values: NULL argument");
  PMG_REQUIRE(!amg->replicated, "pmg_amg_update_values: the replicated and distributed hierarchies are not renewed in "
                                "place; the single-domain form (pmg_amg_create) only");
  PMG_REQUIRE(!amg->layout->multi_rank() && amg->layout->num_ghosts == 0,
              "pmg_amg_update_values: the layout has several ranks or ghosts; the single-domain form only");
  PMG_REQUIRE(amg->op->batch_patches == 0, "pmg_amg_update_values: the operator is in batched-geometry mode, its tensor "
                                           "G is not resident (pmg_laplacian_set_geometry_batch(op, 0) keeps it)");
  hipStream_t s = S(stream);
  PMG_TRY(not_capturing(s, "pmg_amg_update_values: the stream is being captured; the call synchronises it"));
  PMG_HIP(hipStreamSynchronize(s));
  if (!amg->renewal)
    PMG_TRY(renewal_plan(amg));
  amg->unusable = true; // until every level is through
  PMG_TRY(renewal_values(amg, s));
  amg->unusable = false;
  ++amg->updates;
  return PMG_OK;
}

extern "C" long long pmg_amg_updates(pmg_amg amg) { return amg ? amg->updates : -1; }

extern "C" int pmg_amg_destroy(pmg_amg amg)
{
  if (!amg)
    return PMG_OK;
  delete amg->renewal;
  for (AmgLevel& lv : amg->levels)
  {
    free_csr(lv.A);
    free_csr(lv.P);
    free_csr(lv.R);
    (void)hipFree(lv.dinv);
    (void)hipFree(lv.x);
    (void)hipFree(lv.b);
    (void)hipFree(lv.r);
    (void)hipFree(lv.z);
    (void)hipFree(lv.q);
  }
  (void)hipFree(amg->dense_inv_plain);
  (void)hipFree(amg->dense_inv_null);
  (void)hipFree(amg->xc);
  (void)hipFree(amg->gid);
  (void)hipFree(amg->d0_dinv);
  (void)hipFree(amg->gb);
  (void)hipFree(amg->gx);
  if (amg->h_stage)
    (void)hipHostFree(amg->h_stage);
  free_csr(amg->P0l);
  free_csr(amg->R0l);
  (void)hipFree(amg->d0_r);
  (void)hipFree(amg->d0_z);
  (void)hipFree(amg->d0_q);
  (void)hipFree(amg->d0_b);
  (void)hipFree(amg->d0_xc);
  pmg_cg_destroy(amg->cg0);
  pmg_cg_destroy(amg->cg);
  pmg_layout_destroy(amg->glayout);
  delete amg;
  return PMG_OK;
}

extern "C" int pmg_amg_set_smoother_iterations(pmg_amg amg, int k)
{
  PMG_REQUIRE(amg && k >= 1, "pmg_amg_set_smoother_iterations: bad argument");
  amg->smoother_its = k;
  return PMG_OK;
}

extern "C" int pmg_amg_set_cycles(pmg_amg amg, int cycles)
{
  PMG_REQUIRE(amg && cycles >= 0, "pmg_amg_set_cycles: bad argument");
  amg->cycles = cycles;
  return PMG_OK;
}

// Replicated form: 1 (default where the hierarchy has a second level) = level 0 stays on the partitioned operator,
// only the levels below are replicated; 0 = the whole hierarchy replicated (round 2's form).
extern "C" int pmg_amg_set_distributed_fine_level(pmg_amg amg, int enable)
{
  PMG_REQUIRE(amg, "pmg_amg_set_distributed_fine_level: NULL argument");
  PMG_REQUIRE(amg->replicated, "pmg_amg_set_distributed_fine_level: not a replicated hierarchy");
  PMG_REQUIRE(!enable || amg->cg0, "pmg_amg_set_distributed_fine_level: the hierarchy has one level only");
  PMG_REQUIRE(enable || !amg->distributed_setup,
              "pmg_amg_set_distributed_fine_level: this hierarchy was set up without gathering its level 0 "
              "(pmg_amg_create_distributed): it cannot be replicated in the solve");
  amg->dist0 = enable != 0;
  return PMG_OK;
}

extern "C" int pmg_amg_set_krylov(pmg_amg amg, int max_iter, double rtol)
{
  PMG_REQUIRE(amg && max_iter >= 0 && rtol >= 0.0, "pmg_amg_set_krylov: bad argument");
  amg->max_iter = max_iter;
  amg->rtol = rtol;
  amg->cycles = 0;
  return PMG_OK;
}

extern "C" int pmg_amg_solve(pmg_amg amg, double* x, const double* b, int* iterations, pmg_stream stream)
{
  PMG_REQUIRE(amg && x && b, "pmg_amg_solve: NULL argument");
  PMG_REQUIRE(x != b, "pmg_amg_solve: x and b alias");
  PMG_TRY(amg_solve(amg, x, b, S(stream)));
  if (iterations)
    *iterations = amg->last_iterations;
  return PMG_OK;
}

extern "C" int pmg_amg_cycle(pmg_amg amg, double* x, const double* b, pmg_stream stream)
{
  PMG_REQUIRE(amg && x && b && x != b, "pmg_amg_cycle: bad argument");
  PMG_REQUIRE(!amg->replicated, "pmg_amg_cycle: a replicated hierarchy works on gathered vectors; use pmg_amg_solve");
  PMG_REQUIRE(!amg->unusable, "pmg_amg_cycle: the last pmg_amg_update_values of this hierarchy did not finish; it is "
                              "unusable until an update succeeds");
  if (amg->nullspace == PMG_NULLSPACE_CONSTANT)
    PMG_TRY(laplacian_require_singular(amg->op, "pmg_amg_cycle", S(stream)));
  PMG_TRY(amg_cycle(amg, csr_front(&amg->levels[0], S(stream)), 0, x, b, S(stream)));
  if (amg->nullspace == PMG_NULLSPACE_CONSTANT)
    PMG_TRY(remove_mean_async(amg->layout, x, nullptr, S(stream)));
  return PMG_OK;
}

// The coarsest-level inverse of a hierarchy whose level 0 has the constants as its null space:
// v = P_{L-2}^T ... P_0^T 1, the ones restricted through the hierarchy's own transfers, and the inverse of
// A_c + gamma v v^T with gamma = max diag(A_c) / (v^T v), by the Cholesky factorisation of the plain inverse.
static int nullspace_inverse(pmg_amg amg, std::vector<double>& inv)
{
  const int n = amg->hA.back().n;
  std::vector<double> D;
  const int rc = nullspace_shifted(amg->hA[0].n, amg->hP, amg->hA.back(), D);
  PMG_REQUIRE(rc != 1, "pmg_amg_set_nullspace: internal: the transfers do not end on the coarsest level");
  if (rc == 2)
    return fail(PMG_ERR_NUMERIC, "pmg_amg_set_nullspace: the restricted ones vanish on the coarsest level");
  if (!dense_spd_inverse(n, D, inv))
    return fail(PMG_ERR_NUMERIC, "pmg_amg_set_nullspace: A_c + gamma v v^T of the coarsest level (%d rows) is not "
                                 "positive definite: the operator's null space is not the constants", n);
  return PMG_OK;
}

extern "C" int pmg_amg_set_nullspace(pmg_amg amg, int mode)
{
  PMG_REQUIRE(mode == PMG_NULLSPACE_NONE || mode == PMG_NULLSPACE_CONSTANT, "pmg_amg_set_nullspace: unknown mode %d",
              mode);
  PMG_REQUIRE(amg, "pmg_amg_set_nullspace: NULL argument");
  if (mode == PMG_NULLSPACE_CONSTANT)
  {
    PMG_REQUIRE(!amg->replicated, "pmg_amg_set_nullspace: the replicated and distributed hierarchies do not take a "
                                  "null space; the single-domain form (pmg_amg_create) only");
    PMG_REQUIRE(!amg->layout->multi_rank(), "pmg_amg_set_nullspace: the layout has several ranks; the single-domain "
                                            "form only");
    PMG_TRY(laplacian_require_singular(amg->op, "pmg_amg_set_nullspace", nullptr));
    if (!amg->dense_inv_null && !amg->hA.empty() && amg->hA.back().n <= 4096)
    {
      if (amg->host_stale)
        PMG_TRY(refresh_host(amg));
      std::vector<double> inv;
      PMG_TRY(nullspace_inverse(amg, inv));
      PMG_TRY(to_device(&amg->dense_inv_null, inv));
      amg->n_coarsest = amg->hA.back().n;
    }
    amg->dense_inv = amg->dense_inv_null; // (nullptr: a coarsest level too large to invert keeps smoothing)
  }
  else
    amg->dense_inv = amg->plain_valid ? amg->dense_inv_plain : nullptr;
  amg->nullspace = mode;
  PMG_TRY(pmg_cg_set_nullspace(amg->cg, mode)); // the Krylov mode's work object
  return PMG_OK;
}

extern "C" int pmg_amg_nullspace(pmg_amg amg) { return amg ? amg->nullspace : PMG_ERR_INVALID; }

extern "C" int pmg_amg_num_levels(pmg_amg amg) { return amg ? (int)amg->levels.size() : -1; }

extern "C" int pmg_amg_level_info(pmg_amg amg, int level, long long* rows, long long* nnz, double* lambda_max)
{
  PMG_REQUIRE(amg && level >= 0 && level < (int)amg->levels.size(), "pmg_amg_level_info: bad level");
  if (rows)
    *rows = amg->levels[level].n;
  if (nnz)
    *nnz = amg->levels[level].nnz;
  if (lambda_max)
    *lambda_max = amg->levels[level].lmax;
  return PMG_OK;
}

// which = 0: A_level, 1: P_level (level -> level + 1).  Call with NULL arrays for the sizes.
extern "C" int pmg_amg_export(pmg_amg amg, int level, int which, long long* rows, long long* cols, long long* nnz,
                              int32_t* rowptr, int32_t* colidx, double* values)
{
  PMG_REQUIRE(amg && level >= 0 && (which == 0 || which == 1), "pmg_amg_export: bad argument");
  if (amg->host_stale) // after pmg_amg_update_values: the device's current values, on the structural patterns
    PMG_TRY(refresh_host(amg));
  const std::vector<HostCsr>& src = which == 0 ? amg->hA : amg->hP;
  PMG_REQUIRE(level < (int)src.size(), "pmg_amg_export: no such level");
  const HostCsr& M = src[level];
  if (rows)
    *rows = M.n;
  if (cols)
    *cols = M.m;
  if (nnz)
    *nnz = M.nnz();
  if (rowptr)
    std::copy(M.rp.begin(), M.rp.end(), rowptr);
  if (colidx)
    std::copy(M.ci.begin(), M.ci.end(), colidx);
  if (values)
    std::copy(M.v.begin(), M.v.end(), values);
  return PMG_OK;
}
