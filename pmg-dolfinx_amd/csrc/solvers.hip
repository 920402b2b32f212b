// Solver layer: 4th-kind Chebyshev smoother, Jacobi-PCG with Lanczos eigenvalue
// estimate, p-multigrid V-cycle.  Replaces src/chebyshev.hpp, src/cg.hpp and
// src/pmg.hpp.  Everything is enqueued on the caller's stream; the only host
// synchronisations are the CG dot products (their values steer the iteration,
// src/cg.hpp:182,195,206) and an optional residual norm of the V-cycle.
//
// The smoother issues one fused vector pass per Chebyshev step (r -= q;
// z = c1 z + c2 D^-1 r; x += z : 5 reads + 3 writes per dof; x takes each correction in
// the pass that computes it, so no pass follows the last apply) where the reference issues
// 5 Thrust launches (src/chebyshev.hpp:73-83), and the V-cycle drops the residual
// recomputations that only feed log lines (src/pmg.hpp:76-89,114-117,132-143):
// the residual a pre-smooth leaves in its recurrence IS b - A u (:86-87), and the
// last A z of a post-smooth changes neither x nor anything that is read again.
#include "common.hpp"

#include <cstdlib>

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace pmg;

struct pmg_chebyshev_s
{
  pmg_layout layout = nullptr;
  double eig_min = 0, eig_max = 1;
  int max_iter = 1;
  double *r = nullptr, *z = nullptr, *q = nullptr; // work vectors (src/chebyshev.hpp:28-32)
  // the recomputed form (pmg_chebyshev_set_recompute): -1 automatic, 0 never, 1 wherever it applies; the two further
  // product vectors are allocated on its first use; recomputed = smooths that have taken it
  int recompute_mode = -1;
  double *q1 = nullptr, *q2 = nullptr;
  long long recomputed = 0;
};

struct pmg_cg_s
{
  pmg_layout layout = nullptr;
  int max_iter = 0;
  double rtol = 0;
  bool store = false;
  double *r = nullptr, *y = nullptr, *p = nullptr; // src/cg.hpp:101-104
  double* zold = nullptr;                           // flexible variant only
  bool flexible = false;
  int nullspace = PMG_NULLSPACE_NONE; // pmg_cg_set_nullspace
  std::vector<double> alphas, betas, residuals;
};

struct pmg_multigrid_s
{
  int L = 0;
  std::vector<pmg_layout> layouts;
  const int8_t* bc0 = nullptr;
  std::vector<pmg_laplacian> ops;
  std::vector<pmg_chebyshev> smoothers;
  std::vector<pmg_interpolator> interps;
  std::vector<double*> u, b; // per level (finest level uses the caller's vectors)
  std::vector<int> counts;
  // optional coarse solver (src/pmg.hpp:106-107): the library's CG, or any solve(x, b) of the caller
  pmg_cg coarse = nullptr;
  pmg_coarse_solve_fn coarse_fn = nullptr;
  void* coarse_user = nullptr;
  pmg_amg coarse_amg = nullptr;
  // assembled levels (pmg_multigrid_set_level_matrix): where mats[i] is set, the matrix's product and inverse diagonal
  // stand for every application of ops[i] in the cycle; mat_applies[i] counts them for pmg_multigrid_apply_counts
  std::vector<pmg_matrix> mats;
  std::vector<long long> mat_applies;
  // hipGraph replay of the cycle (pmg_multigrid_set_graph): one executable graph per
  // (rhs, y, zero-guess, configuration) seen
  struct GraphEntry
  {
    const double* rhs;
    double* y;
    bool y_zero;
    uint64_t config;
    hipGraphExec_t exec;
    std::vector<int> counts;
    int fused_count;
    std::vector<int> recomputed; // per level: smooths of the captured cycle in the recomputed form
  };
  int graph_mode = -1; // pmg_multigrid_set_graph: 1 replay when capturable, 0 never, -1 (default) automatic: use_graph()
  std::vector<GraphEntry> graphs;
  hipStream_t capture_stream = nullptr;
  long long graph_replays = 0;
  // restriction fused into the pre-smooth's last application (pmg_multigrid_set_fused_restriction): -1 automatic,
  // 0 never; fused_count = how many the last cycle issued
  int fused_mode = -1;
  int fused_count = 0;
  // FP32 cycle (pmg_multigrid_set_precision): float vectors of every level, allocated on the first FP32 cycle; the
  // operators and interpolators hold their own float forms (laplacian_f32.hip, interpolate.hip)
  int precision = PMG_PRECISION_FP64;
  std::vector<float*> u32, b32;
  std::vector<ChebWork<float>> w32;
  std::vector<const float*> dinv32;   // per level, the operators' float diagonals (refreshed by mg_prepare_f32)
  std::vector<const float*> M1_32;    // per interpolator, its float 1-D table (owned by the interpolator)
};

namespace pmg
{
// src/chebyshev.hpp:46-91: the steps of smooth_plan.hpp as calls on d.s.  T = float: the same steps on the float passes
// (vector.hip); every coefficient is formed in FP64 and rounded once.
template <typename T>
int cheb_iterate(const SmoothCall& call, const SmoothData<T>& d)
{
  PMG_REQUIRE(call.fp64 == (sizeof(T) == 8), "cheb_iterate: the call's scalar type is not the data's");
  const ChebWork<T>& w = d.w;
  const int n = d.n, ng = call.ghosts;
  T* const x = d.x;
  T* const product[3] = {w.q, w.q1, w.q2}; // by SmoothStep::Buffer
  hipStream_t s = d.s;
  PMG_TRY(for_each_smooth_step(call, [&](const SmoothStep& st) -> int {
    T* const clear_q = st.clear_q ? w.q : nullptr;
    const T c1 = (T)cheb_c1(st.i), c2 = (T)cheb_c2(st.i, d.lmax);
    switch (st.kind)
    {
    case SmoothStep::APPLY: return d.apply[st.variant](st.in_x ? x : w.z, product[st.out]);
    case SmoothStep::INIT:
      launch_cheb_init(n, w.r, w.z, d.b, st.with_q ? w.q : nullptr, d.dinv, (T)cheb_c0(d.lmax), s, clear_q, d.n_total);
      break;
    case SmoothStep::FIRST:
      launch_cheb_first(n, x, w.r, w.z, w.q, d.dinv, c1, c2, st.x_final, s, clear_q, d.n_total);
      break;
    case SmoothStep::STEP:
      launch_cheb_step(n, x, w.r, w.z, w.q, d.dinv, c1, c2, st.both, st.x_final, s, clear_q, d.n_total);
      break;
    case SmoothStep::LAST: launch_cheb_last(n, x, w.r, w.z, w.q, st.assign, s); break;
    case SmoothStep::RESIDUAL: launch_cheb_residual(n, w.r, w.q, s); break;
    case SmoothStep::ADD: launch_add(n, x, w.z, s); break;
    case SmoothStep::GHOST_ADD: launch_add(ng, x + n, w.z + n, s); break;
    case SmoothStep::COPY: PMG_HIP(hipMemcpyAsync(x, w.z, sizeof(T) * n, hipMemcpyDeviceToDevice, s)); break;
    case SmoothStep::ZERO_X: launch_zero(n, x, s); break;
    case SmoothStep::ZERO_GHOSTS: launch_zero(ng, x + n, s); break;
    case SmoothStep::RECOMPUTE:
      if constexpr (sizeof(T) == 8)
      {
        const double c[5] = {cheb_c0(d.lmax), cheb_c1(1), cheb_c2(1, d.lmax), cheb_c1(2), cheb_c2(2, d.lmax)};
        launch_cheb_recompute(n, st.stage, st.stage == 3 ? x : nullptr, st.r_out ? w.r : nullptr,
                              st.stage < 3 || st.r_out ? w.z : nullptr, d.b, st.with_q ? w.q : nullptr,
                              st.stage >= 2 ? w.q1 : nullptr, st.with_q2 ? w.q2 : nullptr, d.dinv, c, s);
      }
      break;
    }
    return PMG_OK;
  }));
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}
template int cheb_iterate<double>(const SmoothCall&, const SmoothData<double>&);
template int cheb_iterate<float>(const SmoothCall&, const SmoothData<float>&);
} // namespace pmg

namespace
{
int mg_apply_graph(pmg_multigrid mg, const double* rhs, double* y, bool y_zero, hipStream_t s, bool* done);
bool use_graph(pmg_multigrid mg);
// every captured cycle holds the device pointers of the objects it was captured with: any change of
// the multigrid's parts invalidates all of them
void drop_graphs(pmg_multigrid mg);

template <typename T>
int alloc_vec(pmg_layout l, T** p)
{
  size_t n = l->total() ? l->total() : 1;
  PMG_HIP(hipMalloc(p, sizeof(T) * n));
  PMG_HIP(hipMemset(*p, 0, sizeof(T) * n));
  PMG_HIP(hipStreamSynchronize(nullptr)); // the fill runs on the null stream, which non-blocking streams do not order
  return PMG_OK;
}

// Does this smoother's mode ask for the recomputed form?  On request, or by default where the level's vectors are
// streamed: there a pass costs its bytes and three passes less per smooth show in the cycle
// (profiles/chebyshev_recompute.md); a resident level's passes are cheap and the form would only add two vectors.
// Which calls take it is the schedule's business (smooth_plan.hpp).
bool wants_recompute(pmg_chebyshev sm)
{
  return sm->recompute_mode >= 0 ? sm->recompute_mode == 1 : vector_streams(sm->layout->size_local);
}

// the form's two further product vectors, on first use; a stream that is being captured cannot allocate: the call then
// keeps the stored form (mg_apply_graph allocates before it captures)
int recompute_buffers(pmg_chebyshev sm, hipStream_t s)
{
  if (sm->q1 && sm->q2)
    return PMG_OK;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (s && hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone)
    return PMG_OK;
  if (!sm->q1)
    PMG_TRY(alloc_vec(sm->layout, &sm->q1));
  if (!sm->q2)
    PMG_TRY(alloc_vec(sm->layout, &sm->q2));
  return PMG_OK;
}

// The call of smoother `sm`: the one place where a SmoothCall is read off the library's objects.  A = the matrix-free
// operator it runs on, nullptr for a plain product (an assembled matrix, the float apply): no output rule, no
// recomputed form.  track_ghosts / ghosts_current: the exchange bookkeeping of the V-cycle (local_correction); it holds
// for every operator that refreshes the ghosts of its input -- the matrix-free one and a distributed matrix
// (`exchanging`) --, not for the float apply, which is single-domain.
SmoothCall smoother_call(pmg_chebyshev sm, pmg_laplacian A, int need_r, bool x_zero, bool track_ghosts = false,
                         bool ghosts_current = false, bool exchanging = false)
{
  SmoothCall c;
  c.k = sm->max_iter;
  c.need_r = need_r;
  c.x_zero = x_zero;
  c.zeroed_output = A && laplacian_wants_zeroed_output(A);
  c.ghosts = (A || exchanging) && track_ghosts ? sm->layout->num_ghosts : 0;
  c.ghosts_current = (A || exchanging) && ghosts_current;
  c.allow_recompute = A && wants_recompute(sm);
  return c;
}

// src/chebyshev.hpp:46-91 on the operator `A`: the call as smoother_call made it
int cheb_solve(pmg_chebyshev sm, pmg_laplacian A, double* x, const double* b, SmoothCall call, hipStream_t s)
{
  pmg_layout l = sm->layout;
  PMG_REQUIRE(laplacian_layout(A) == l, "Chebyshev: operator and smoother layouts differ");
  if (call.allow_recompute && smooth_outcome(call).recomputed)
    PMG_TRY(recompute_buffers(sm, s));
  call.allow_recompute = call.allow_recompute && sm->q1 && sm->q2;
  // eig_range[0] is unused (src/chebyshev.hpp:51); no per-call D2D copy of the diagonal (:53)
  SmoothData<double> d;
  d.w = {sm->r, sm->z, sm->q, sm->q1, sm->q2};
  d.apply[SmoothStep::PLAIN] = [A, s](double* in, double* out) { return laplacian_apply(A, in, out, s); };
  d.apply[SmoothStep::ZEROED_OUTPUT] = [A, s](double* in, double* out) { return laplacian_apply_zeroed(A, in, out, s); };
  d.apply[SmoothStep::GHOSTS_CURRENT] = [A, s](double* in, double* out)
  { return laplacian_apply_ghosts_current(A, in, out, s); };
  d.dinv = laplacian_diag_inv(A);
  d.n = l->size_local, d.n_total = l->total();
  d.lmax = sm->eig_max;
  d.x = x, d.b = b, d.s = s;
  PMG_TRY(cheb_iterate(call, d));
  if (smooth_outcome(call).recomputed)
    sm->recomputed++;
  return PMG_OK;
}

// the same smoother on the assembled operator `M`: its product (on several ranks with its halo exchange, or without
// where the call's bookkeeping says the ghosts are current), its own inverse diagonal; *applies (optional) counts the
// products issued
int cheb_solve_matrix(pmg_chebyshev sm, pmg_matrix M, double* x, const double* b, const SmoothCall& call, hipStream_t s,
                      long long* applies = nullptr)
{
  pmg_layout l = sm->layout;
  PMG_REQUIRE(matrix_layout(M) == l, "Chebyshev: matrix and smoother layouts differ");
  SmoothData<double> d;
  d.w = {sm->r, sm->z, sm->q};
  d.apply[SmoothStep::PLAIN] = [M, s](double* in, double* out) { return matrix_apply(M, in, out, s); };
  d.apply[SmoothStep::GHOSTS_CURRENT] = [M, s](double* in, double* out)
  { return matrix_apply_ghosts_current(M, in, out, s); };
  d.dinv = matrix_diag_inv(M);
  d.n = l->size_local, d.n_total = l->total();
  d.lmax = sm->eig_max;
  d.x = x, d.b = b, d.s = s;
  PMG_TRY(cheb_iterate(call, d));
  if (applies)
    *applies += smooth_outcome(call).applications;
  return PMG_OK;
}

// Does level i's pre-smooth hand its last application to the restriction (stiffness_restrict_kernel)?  The level has
// no assembled matrix and the transfer below it fuses on the level's operator (interp_fuses_residual: patch form, no
// ghosts, resident geometry, an instantiated pair); pmg_multigrid_set_fused_restriction(mg, 0) turns it off.
bool fuses_restriction(pmg_multigrid mg, int i)
{
  if (mg->fused_mode == 0 || i <= 0 || mg->mats[i] || !interp_fuses_residual(mg->interps[i - 1], mg->ops[i]))
    return false;
  // measurements: PMG_FUSED_DEGREES=4 (or 2,4 ...) fuses below these fine degrees only, 0 nowhere
  if (const char* e = std::getenv("PMG_FUSED_DEGREES"))
  {
    const int P = pmg_laplacian_degree(mg->ops[i]);
    for (const char* c = e; *c; ++c)
      if (*c - '0' == P)
        return true;
    return false;
  }
  return true;
}

// applications of level i's operator so far, in either form
long long level_applies(pmg_multigrid mg, int i) { return laplacian_launches(mg->ops[i]) + mg->mat_applies[i]; }

// Exchange bookkeeping on several ranks (round 4).  u_i leaves its pre-smooth with current ghosts (the smoother adds
// the ghosts of every applied correction, cheb_iterate); the patch form of the prolongation computes the correction on
// EVERY local cell, ghost cells included, from the coarse ghosts it has just received, and adds it to every patch dof it
// writes first -- ghost dofs too: u_i + P u_{i-1} therefore has current ghosts without an exchange of its own, and the
// first application of the post-smooth runs without one (19 -> 17 exchanges per cycle of three levels with k = 3).
// Values at a ghost dof are computed from another cell than on the owner: equal to rounding, not bit for bit.
bool local_correction(pmg_multigrid mg, int level)
{
  if (const char* e = std::getenv("PMG_LOCAL_CORRECTION")) // tests / measurements: 0 = an exchange per application
    if (e[0] == '0')
      return false;
  return level > 0 && mg->layouts[level]->num_ghosts > 0 && interp_is_patched(mg->interps[level - 1]);
}

// Is every part of the multigrid fit for the FP32 cycle?  (the refusals of pmg_multigrid_set_precision)
int mg_check_f32(pmg_multigrid mg, const char* who)
{
  for (int i = 0; i < mg->L; ++i)
  {
    pmg_layout l = mg->layouts[i];
    PMG_REQUIRE(l->num_ghosts == 0 && !l->multi_rank() && !l->win,
                "%s: the FP32 cycle is single-domain only (level %d's layout has ghosts or a communicator)", who, i);
  }
  for (size_t i = 0; i < mg->interps.size(); ++i)
    PMG_REQUIRE(interp_is_patched(mg->interps[i]),
                "%s: the FP32 cycle needs patch-form interpolators (pmg_interpolator_create_with_operator; level %zu)",
                who, i);
  for (pmg_laplacian op : mg->ops)
    PMG_TRY(laplacian_f32_supported(op, who));
  return PMG_OK;
}

void free_f32(pmg_multigrid mg)
{
  for (float* p : mg->u32)
    (void)hipFree(p);
  for (float* p : mg->b32)
    (void)hipFree(p);
  for (const ChebWork<float>& w : mg->w32)
  {
    (void)hipFree(w.r);
    (void)hipFree(w.z);
    (void)hipFree(w.q);
  }
  mg->u32.clear();
  mg->b32.clear();
  mg->w32.clear();
}

// Everything the FP32 cycle reads besides its vectors, current on `s`: float vectors, the operators' float tensors,
// float diagonals (re-converted after a change of diag_inv) and transfer tables.  Allocates on first use -- called
// outside any capture (mg_apply_graph prepares before it captures; inside the capture this is a no-op).
int mg_prepare_f32(pmg_multigrid mg, hipStream_t s)
{
  const int L = mg->L;
  PMG_TRY(mg_check_f32(mg, "pmg_multigrid_apply"));
  if ((int)mg->u32.size() != L)
  {
    mg->u32.assign(L, nullptr);
    mg->b32.assign(L, nullptr);
    mg->w32.assign(L, ChebWork<float>{});
    for (int i = 0; i < L; ++i)
    {
      PMG_TRY(alloc_vec(mg->layouts[i], &mg->u32[i]));
      PMG_TRY(alloc_vec(mg->layouts[i], &mg->b32[i]));
      PMG_TRY(alloc_vec(mg->layouts[i], &mg->w32[i].r));
      PMG_TRY(alloc_vec(mg->layouts[i], &mg->w32[i].z));
      PMG_TRY(alloc_vec(mg->layouts[i], &mg->w32[i].q));
    }
  }
  mg->M1_32.assign(L - 1, nullptr);
  for (int i = 0; i < L - 1; ++i)
    PMG_TRY(transfer_f32_prepare(mg->interps[i], &mg->M1_32[i]));
  mg->dinv32.assign(L, nullptr);
  for (int i = 0; i < L; ++i)
  {
    PMG_TRY(laplacian_f32_prepare(mg->ops[i], s));
    PMG_TRY(laplacian_f32_diag(mg->ops[i], &mg->dinv32[i], s, nullptr));
  }
  return PMG_OK;
}

// The smooths of a cycle: before the restriction (levels > 0), in place of a coarse solver (level 0), behind the
// prolongation (levels > 0).
enum SmoothRole
{
  PreSmooth,
  CoarseSmooth,
  PostSmooth
};
bool has_coarse_solver(pmg_multigrid mg) { return mg->coarse_amg || mg->coarse || mg->coarse_fn; }
bool cycle_smooths(pmg_multigrid mg, int i, SmoothRole role)
{
  return role == CoarseSmooth ? i == 0 && !(has_coarse_solver(mg) && mg->L > 1) : i > 0; // src/pmg.hpp:106-109
}
// The call of level i's smoother in that role, for a cycle whose finest iterate is zero on entry or not: what mg_apply
// issues, and what mg_apply_graph asks before it captures.
//   x_zero   u[i < L-1] = 0 (src/pmg.hpp:63-64) is folded into the smoothers' x_zero path; the FP32 cycle starts every
//            level from zero (defect correction at the finest)
//   need_r   the pre-smooth leaves the residual to the restriction in the form that restriction consumes
//   ghosts   several ranks: the iterate leaves the pre-smooth with current ghosts and, with local_correction, still has
//            them in front of the post-smooth, whose first application then runs without an exchange
SmoothCall level_call(pmg_multigrid mg, int i, SmoothRole role, bool y_zero)
{
  pmg_chebyshev sm = mg->smoothers[i];
  if (mg->precision == PMG_PRECISION_FP32) // the float apply: a plain product, single domain
  {
    SmoothCall c = smoother_call(sm, nullptr, role == PreSmooth ? ResidualSplit : ResidualNone, role != PostSmooth);
    c.fp64 = false;
    return c;
  }
  int need_r = ResidualNone;
  if (role == PreSmooth)
    need_r = fuses_restriction(mg, i)                          ? ResidualFused
             : interp_restricts_difference(mg->interps[i - 1]) ? ResidualSplit
                                                               : ResidualUpdated;
  const bool x_zero = role != PostSmooth && (i == mg->L - 1 ? y_zero : true);
  const bool local = local_correction(mg, i);
  return smoother_call(sm, mg->mats[i] ? nullptr : mg->ops[i], need_r, x_zero, local && role == PreSmooth,
                       local && role == PostSmooth, mg->mats[i] != nullptr);
}

// the smoother of level i on whichever form of the operator the level has (pmg_multigrid_set_level_matrix)
int level_smooth(pmg_multigrid mg, int i, double* x, const double* b, const SmoothCall& call, hipStream_t s)
{
  if (mg->mats[i])
    return cheb_solve_matrix(mg->smoothers[i], mg->mats[i], x, b, call, s, &mg->mat_applies[i]);
  return cheb_solve(mg->smoothers[i], mg->ops[i], x, b, call, s);
}

// the smoother of level i in FP32: the same steps on the operator's float form
int level_smooth_f32(pmg_multigrid mg, int i, const SmoothCall& call, hipStream_t s)
{
  pmg_laplacian op = mg->ops[i];
  SmoothData<float> d;
  d.w = mg->w32[i];
  d.apply[SmoothStep::PLAIN] = [op, s](float* in, float* out) { return laplacian_apply_f32(op, in, out, s); };
  d.dinv = mg->dinv32[i];
  d.n = mg->layouts[i]->size_local, d.n_total = mg->layouts[i]->total();
  d.lmax = mg->smoothers[i]->eig_max;
  d.x = mg->u32[i], d.b = mg->b32[i], d.s = s;
  return cheb_iterate(call, d);
}

// u[0] = the coarse solver's answer to b[0], in FP64 (src/pmg.hpp:106-107): the library's own AMG (amg.hip), or,
// KSP-style from a zero initial guess, the library's CG or the caller's callback
int coarse_solve(pmg_multigrid mg, hipStream_t s)
{
  if (mg->coarse_amg)
    return amg_solve(mg->coarse_amg, mg->u[0], mg->b[0], s);
  launch_zero(mg->layouts[0]->total(), mg->u[0], s);
  if (mg->coarse_fn)
  {
    if (mg->coarse_fn(mg->coarse_user, mg->u[0], mg->b[0], (pmg_stream)s) != 0)
      return fail(PMG_ERR_INVALID, "the coarse-solver callback failed");
    return PMG_OK;
  }
  int its = 0;
  return pmg_cg_solve(mg->coarse, mg->ops[0], mg->u[0], mg->b[0], nullptr, &its, (pmg_stream)s);
}

// The V-cycle in FP32 (pmg_multigrid_set_precision): the caller's FP64 rhs / y at the finest level only.
//   zero guess: y = double(V32(float(rhs)));
//   otherwise (defect correction): y += double(V32(float(rhs - A y))), the defect formed with the FP64 operator -- the
//   cycle is affine, so this is the FP64 cycle to float rounding, and stationary cycles keep converging below the
//   float accuracy of a single cycle.
// A Krylov, AMG or callback coarse solver runs in FP64 on the library's existing objects: b_0 is converted up and
// u_0 down around it; the smoother-only coarse level runs in FP32.
int mg_apply_f32(pmg_multigrid mg, const double* rhs, double* y, bool y_zero, hipStream_t s)
{
  const int L = mg->L;
  mg->fused_count = 0; // (the FP32 cycle does not fuse)
  std::vector<long long> before(L);
  for (int i = 0; i < L; ++i)
    before[i] = laplacian_launches(mg->ops[i]);
  PMG_TRY(mg_prepare_f32(mg, s));
  Range cycle("pmg:vcycle_f32");
  const int nf = mg->layouts[L - 1]->size_local;
  if (y_zero)
    launch_to_f32(nf, rhs, nullptr, mg->b32[L - 1], s);
  else
  {
    double* q = mg->smoothers[L - 1]->q; // FP64 work vector of the finest level
    PMG_TRY(laplacian_apply(mg->ops[L - 1], y, q, s));
    launch_to_f32(nf, rhs, q, mg->b32[L - 1], s);
  }
  for (int i = L - 1; i > 0; --i)
  {
    const SmoothCall pre = level_call(mg, i, PreSmooth, y_zero);
    {
      Range rg("pmg:pre_smooth");
      PMG_TRY(level_smooth_f32(mg, i, pre, s));
    }
    Range rg("pmg:restrict");
    const bool split = smooth_outcome(pre).left_to_consumer == SmoothOutcome::LeftSplit;
    PMG_TRY(restrict_f32(mg->interps[i - 1], mg->M1_32[i - 1], mg->w32[i].r, split ? mg->w32[i].q : nullptr,
                         mg->b32[i - 1], s));
  }
  const int n0 = mg->layouts[0]->size_local;
  if (L > 1)
    launch_mask_bc(n0, mg->b32[0], mg->bc0, s);
  {
    Range rg("pmg:coarse_solve");
    if (!cycle_smooths(mg, 0, CoarseSmooth)) // FP64 on the existing objects
    {
      launch_from_f32(n0, mg->b32[0], mg->b[0], false, s);
      PMG_TRY(coarse_solve(mg, s));
      launch_to_f32(n0, mg->u[0], nullptr, mg->u32[0], s);
    }
    else
      PMG_TRY(level_smooth_f32(mg, 0, level_call(mg, 0, CoarseSmooth, y_zero), s));
  }
  for (int i = 0; i < L - 1; ++i)
  {
    {
      Range rg("pmg:prolong");
      PMG_TRY(prolong_add_f32(mg->interps[i], mg->M1_32[i], mg->u32[i], mg->u32[i + 1], s));
    }
    Range rg("pmg:post_smooth");
    PMG_TRY(level_smooth_f32(mg, i + 1, level_call(mg, i + 1, PostSmooth, y_zero), s));
  }
  launch_from_f32(nf, mg->u32[L - 1], y, !y_zero, s);
  for (int i = 0; i < L; ++i)
    mg->counts[i] = (int)(laplacian_launches(mg->ops[i]) - before[i]);
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}

// src/pmg.hpp:56-155 (lean form, see the file header)
int mg_apply(pmg_multigrid mg, const double* rhs, double* y, bool y_zero, hipStream_t s)
{
  const int L = mg->L;
  PMG_REQUIRE((int)mg->ops.size() == L && (int)mg->smoothers.size() == L
                  && (int)mg->interps.size() == L - 1,
              "MultigridPreconditioner: operators / solvers / interpolators not set");
  if (mg->precision == PMG_PRECISION_FP32)
    return mg_apply_f32(mg, rhs, y, y_zero, s);
  std::vector<long long> before(L);
  for (int i = 0; i < L; ++i)
    before[i] = level_applies(mg, i);
  // u[L-1] = y, b[L-1] = rhs (:65,68) -- used in place; every smooth's call comes from level_call
  Range cycle("pmg:vcycle");
  mg->u[L - 1] = y;
  mg->fused_count = 0;
  for (int i = L - 1; i > 0; --i)
  {
    const double* bi = (i == L - 1) ? rhs : mg->b[i];
    const SmoothCall pre = level_call(mg, i, PreSmooth, y_zero);
    {
      Range rg("pmg:pre_smooth");
      PMG_TRY(level_smooth(mg, i, mg->u[i], bi, pre, s)); // :83-87
    }
    Range rg("pmg:restrict");
    switch (smooth_outcome(pre).left_to_consumer)
    {
    case SmoothOutcome::LeftFused: // the smoother's last application and the restriction of r - A z in one kernel
      PMG_TRY(interp_restrict_residual(mg->interps[i - 1], mg->ops[i], mg->smoothers[i]->z, mg->smoothers[i]->r,
                                       mg->b[i - 1], s));
      mg->fused_count++;
      break;
    case SmoothOutcome::LeftSplit: // the residual r - q is formed by the restriction's gather
      PMG_TRY(interp_restrict_difference(mg->interps[i - 1], mg->smoothers[i]->r, mg->smoothers[i]->q,
                                         mg->b[i - 1], s));
      break;
    case SmoothOutcome::LeftNone:
      PMG_TRY(interp_restrict(mg->interps[i - 1], mg->smoothers[i]->r, mg->b[i - 1], s)); // :92
    }
  }
  if (L > 1)
    launch_mask_bc(mg->layouts[0]->size_local, mg->b[0], mg->bc0, s); // :100-103
  {
    Range rg("pmg:coarse_solve");
    const double* b0 = (L == 1) ? rhs : mg->b[0];
    if (!cycle_smooths(mg, 0, CoarseSmooth)) // :106-107
      PMG_TRY(coarse_solve(mg, s));
    else
      PMG_TRY(level_smooth(mg, 0, mg->u[0], b0, level_call(mg, 0, CoarseSmooth, y_zero), s)); // :109
  }
  for (int i = 0; i < L - 1; ++i)
  {
    {
      Range rg("pmg:prolong");
      if (interp_is_patched(mg->interps[i]))
        PMG_TRY(interp_prolong_add(mg->interps[i], mg->u[i], mg->u[i + 1], s)); // :123 + :129 in one pass
      else
      {
        double* du = mg->smoothers[i + 1]->q;                            // work vector as du
        PMG_TRY(interp_prolong(mg->interps[i], mg->u[i], du, s));        // :123
        launch_add(mg->layouts[i + 1]->size_local, mg->u[i + 1], du, s); // :129
      }
    }
    Range rg("pmg:post_smooth");
    const double* bi = (i + 1 == L - 1) ? rhs : mg->b[i + 1];
    PMG_TRY(level_smooth(mg, i + 1, mg->u[i + 1], bi, level_call(mg, i + 1, PostSmooth, y_zero), s)); // :138
  }
  for (int i = 0; i < L; ++i)
    mg->counts[i] = (int)(level_applies(mg, i) - before[i]);
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}
} // namespace

// ------------------------------------------------------------- Chebyshev --
extern "C" int pmg_chebyshev_create(pmg_chebyshev* out, pmg_layout layout, double eig_min,
                                    double eig_max)
{
  PMG_REQUIRE(out && layout, "pmg_chebyshev_create: NULL argument");
  PMG_REQUIRE(eig_max > 0.0, "pmg_chebyshev_create: eig_max must be positive");
  auto* sm = new pmg_chebyshev_s;
  HandleGuard<pmg_chebyshev> guard(sm, pmg_chebyshev_destroy);
  sm->layout = layout;
  sm->eig_min = eig_min;
  sm->eig_max = eig_max;
  PMG_TRY(alloc_vec(layout, &sm->r));
  PMG_TRY(alloc_vec(layout, &sm->z));
  PMG_TRY(alloc_vec(layout, &sm->q));
  if (const char* e = std::getenv("PMG_CHEB_RECOMPUTE")) // the initial mode of pmg_chebyshev_set_recompute
    if ((e[0] == '0' || e[0] == '1') && !e[1])
      sm->recompute_mode = e[0] - '0';
  *out = guard.release();
  return PMG_OK;
}

extern "C" int pmg_chebyshev_destroy(pmg_chebyshev sm)
{
  if (!sm)
    return PMG_OK;
  (void)hipFree(sm->r);
  (void)hipFree(sm->z);
  (void)hipFree(sm->q);
  (void)hipFree(sm->q1);
  (void)hipFree(sm->q2);
  delete sm;
  return PMG_OK;
}

extern "C" int pmg_chebyshev_set_recompute(pmg_chebyshev sm, int mode)
{
  PMG_REQUIRE(sm, "pmg_chebyshev_set_recompute: NULL argument");
  PMG_REQUIRE(mode >= -1 && mode <= 1, "pmg_chebyshev_set_recompute: mode %d (-1 automatic, 0 never, 1 wherever it applies)",
              mode);
  sm->recompute_mode = mode; // (part of the key of a multigrid's captured cycles: capture_config)
  return PMG_OK;
}

extern "C" long long pmg_chebyshev_recomputed(pmg_chebyshev sm) { return sm ? sm->recomputed : -1; }

extern "C" int pmg_chebyshev_set_max_iterations(pmg_chebyshev sm, int max_iter)
{
  PMG_REQUIRE(sm && max_iter >= 0, "pmg_chebyshev_set_max_iterations: bad argument");
  sm->max_iter = max_iter;
  return PMG_OK;
}

extern "C" int pmg_chebyshev_solve(pmg_chebyshev sm, pmg_laplacian A, double* x, const double* b,
                                   pmg_stream stream)
{
  PMG_REQUIRE(sm && A && x && b, "pmg_chebyshev_solve: NULL argument");
  return cheb_solve(sm, A, x, b, smoother_call(sm, A, ResidualNone, false), S(stream));
}

extern "C" int pmg_chebyshev_solve_matrix(pmg_chebyshev sm, pmg_matrix M, double* x, const double* b,
                                          pmg_stream stream)
{
  PMG_REQUIRE(sm && M && x && b, "pmg_chebyshev_solve_matrix: NULL argument");
  return cheb_solve_matrix(sm, M, x, b, smoother_call(sm, nullptr, ResidualNone, false), S(stream));
}

// -------------------------------------------------------------------- CG --
extern "C" int pmg_cg_create(pmg_cg* out, pmg_layout layout)
{
  PMG_REQUIRE(out && layout, "pmg_cg_create: NULL argument");
  auto* cg = new pmg_cg_s;
  HandleGuard<pmg_cg> guard(cg, pmg_cg_destroy);
  cg->layout = layout;
  PMG_TRY(alloc_vec(layout, &cg->r));
  PMG_TRY(alloc_vec(layout, &cg->y));
  PMG_TRY(alloc_vec(layout, &cg->p));
  *out = guard.release();
  return PMG_OK;
}

extern "C" int pmg_cg_destroy(pmg_cg cg)
{
  if (!cg)
    return PMG_OK;
  (void)hipFree(cg->r);
  (void)hipFree(cg->y);
  (void)hipFree(cg->p);
  (void)hipFree(cg->zold);
  delete cg;
  return PMG_OK;
}

extern "C" int pmg_cg_set_max_iterations(pmg_cg cg, int max_iter)
{
  PMG_REQUIRE(cg && max_iter >= 0, "pmg_cg_set_max_iterations: bad argument");
  cg->max_iter = max_iter; // src/cg.hpp:107-113
  cg->alphas.reserve(max_iter);
  cg->betas.reserve(max_iter);
  cg->residuals.reserve(max_iter);
  return PMG_OK;
}

extern "C" int pmg_cg_set_tolerance(pmg_cg cg, double rtol)
{
  PMG_REQUIRE(cg, "pmg_cg_set_tolerance: NULL argument");
  cg->rtol = rtol;
  return PMG_OK;
}

extern "C" int pmg_cg_store_coefficients(pmg_cg cg, int flag)
{
  PMG_REQUIRE(cg, "pmg_cg_store_coefficients: NULL argument");
  cg->store = flag != 0;
  return PMG_OK;
}

namespace
{
// cg_iterate for an operator whose null space is the constants (pmg_cg_set_nullspace), with
// Pi = I - 1 1^T / N:
//   r_0 = Pi (b - A x_0);  z = M r;  rz = r . z - (1 . r)(1 . z) / N;  p = Pi z + beta p;  alpha = rz / (p . y);
//   after the loop x <- Pi x.
// Pi z is never formed on its own: r . z, 1 . r and 1 . z come out of one pass over r and z (cg_sums3_async; the
// Jacobi branch forms z = dinv r in it), the shift (1 . z) / N is applied inside the direction kernel, and the
// projected rz is formed from the slots -- on the device for alpha and beta, on the host, by the same expression
// (projected_rz), for the stopping test.  An iteration issues the launches of the plain loop and keeps its one fetch;
// a solve adds the projections of r_0 and of x and one first-direction kernel (p_0 = Pi z_0 written from z_0, where
// the plain loop preconditions straight into p).
// Flexible variant: r . Pi z_old = r . z_old - (1 . r)(1 . z_old) / N with last iteration's 1 . z carried on the host.
// Result slots: 1 = p.y, 2 = r.z, 3 = 1.r, 4 = 1.z, 5 = r.z_old.
int cg_iterate_nullspace(pmg_cg cg, const ApplyFn& A, const double* dinv, const PrecondFn* M, bool flex, double* x,
                         const double* b, int* iterations, hipStream_t s)
{
  pmg_layout l = cg->layout;
  const int n = l->size_local;
  double *r = cg->r, *y = cg->y, *p = cg->p;
  double N = 0.0;
  PMG_TRY(layout_global_size(l, &N, s));
  PMG_REQUIRE(N > 0.0, "CG with the constant null space: the layout has no entries");
  auto precondition_and_sums = [&]() -> int
  {
    if (M)
      PMG_TRY((*M)(y, r));
    PMG_TRY(cg_sums3_async(l, r, y, M ? nullptr : dinv, 2, s));
    return PMG_OK;
  };
  PMG_TRY(A(x, y));
  launch_axpy(n, r, -1.0, y, b, s);
  PMG_TRY(remove_mean_async(l, r, nullptr, s)); // r_0 = Pi (b - A x_0)
  PMG_TRY(precondition_and_sums());
  PMG_TRY(reduce_slots_async(l, 2, 3, false, s));
  launch_cg_direction_null(n, p, y, true, 1.0, red_slot(l, 2), nullptr, 0.0, N, s); // p_0 = Pi z_0
  if (flex)
    PMG_HIP(hipMemcpyAsync(cg->zold, y, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
  double v0[3] = {0, 0, 0};
  PMG_TRY(fetch_slots(l, 2, 3, v0, s));
  const double rnorm0 = projected_rz(v0[0], v0[1], v0[2], N);
  double sz_old = v0[2];
  double rnorm = rnorm0;
  const double rtol2 = cg->rtol * cg->rtol;
  if (!std::isfinite(rnorm0) || rnorm0 < 0.0)
    return fail(PMG_ERR_NUMERIC, "CG: r . M^-1 r = %g at the start is not a non-negative finite number", rnorm0);
  int k = 0;
  while (rnorm0 != 0.0 && k < cg->max_iter)
  {
    ++k;
    Range range("pmg:cg_iteration");
    PMG_TRY(A(p, y));
    PMG_TRY(dot_async(l, p, y, 1, s));
    PMG_TRY(reduce_slots_async(l, 1, 1, false, s));
    launch_cg_update2_null(n, x, r, p, y, red_slot(l, 2), N, red_slot(l, 1), s);
    PMG_TRY(precondition_and_sums());
    if (flex)
      PMG_TRY(dot_async(l, r, cg->zold, 5, s));
    PMG_TRY(reduce_slots_async(l, 2, flex ? 4 : 3, false, s));
    launch_cg_direction_null(n, p, y, false, rnorm, red_slot(l, 2), flex ? red_slot(l, 5) : nullptr, sz_old, N, s);
    if (flex)
      PMG_HIP(hipMemcpyAsync(cg->zold, y, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
    double v[5] = {0, 0, 0, 0, 0};
    PMG_TRY(fetch_slots(l, 1, flex ? 5 : 4, v, s)); // the iteration's one host synchronisation
    const double alpha = rnorm / v[0];
    const double rnorm_new = projected_rz(v[1], v[2], v[3], N);
    const double beta = (rnorm_new - (flex ? projected_rz(v[4], v[2], sz_old, N) : 0.0)) / rnorm;
    sz_old = v[3];
    rnorm = rnorm_new;
    if (rnorm / rnorm0 < rtol2)
      break;
    if (cg->store)
    {
      cg->alphas.push_back(alpha);
      cg->betas.push_back(beta);
      cg->residuals.push_back(rnorm);
    }
  }
  PMG_TRY(remove_mean_async(l, x, nullptr, s)); // x <- Pi x
  if (!cg->store || rnorm0 == 0.0)
  {
    cg->residuals.clear();
    cg->residuals.push_back(rnorm);
  }
  if (iterations)
    *iterations = k;
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}
} // namespace

namespace pmg
{
// src/cg.hpp:147-222 over any operator `A`; the preconditioner is `M` (z = M r) if given, else the
// diagonal `dinv` (the reference's hard-wired Jacobi, :161,192).
int cg_iterate(pmg_cg cg, const ApplyFn& A, const double* dinv, const PrecondFn* M, bool flexible, double* x,
               const double* b, int* iterations, hipStream_t s)
{
  pmg_layout l = cg->layout;
  const int n = l->size_local;
  double *r = cg->r, *y = cg->y, *p = cg->p;
  const bool precond = M != nullptr;
  auto precondition = [&](double* out_z, const double* in_r) -> int
  {
    if (precond)
      return (*M)(out_z, in_r);
    launch_pointwise(n, out_z, in_r, dinv, s); // :161,192
    return PMG_OK;
  };
  // Flexible CG (Polak-Ribiere beta) for a preconditioner that is not a fixed linear operator --
  // the V-cycle with a Krylov coarse solver: one more vector (the previous z), one more dot product
  const bool flex = flexible && precond;
  if (flex && !cg->zold)
    PMG_TRY(alloc_vec(l, &cg->zold));
  if (cg->nullspace == PMG_NULLSPACE_CONSTANT)
    return cg_iterate_nullspace(cg, A, dinv, M, flex, x, b, iterations, s);
  PMG_TRY(A(x, y)); // :159
  launch_axpy(n, r, -1.0, y, b, s);     // :160
  PMG_TRY(precondition(p, r));          // :161
  if (flex)
    PMG_HIP(hipMemcpyAsync(cg->zold, p, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
  double rnorm0;
  PMG_TRY(dot_host(l, p, r, &rnorm0, s)); // :163
  double rnorm = rnorm0;
  const double rtol2 = cg->rtol * cg->rtol;
  if (!std::isfinite(rnorm0) || rnorm0 < 0.0) // a poisoned right-hand side / operator, or an indefinite preconditioner
    return fail(PMG_ERR_NUMERIC, "CG: r . M^-1 r = %g at the start is not a non-negative finite number", rnorm0);
  if (rnorm0 == 0.0) // r = 0: x already solves the system; :206 would divide by zero
  {
    if (iterations)
      *iterations = 0;
    cg->residuals.assign(1, rnorm0);
    return PMG_OK;
  }
  // The loop keeps its scalars on the device: p.y, r.z (and r.z_old) are reduced there (one
  // ncclAllReduce each when the layout has a communicator), alpha and beta are formed inside the
  // update kernels, and the host reads the values ONCE per iteration, at its end, for the stopping
  // test and the Lanczos record -- the reference takes two blocking MPI_Allreduce per iteration
  // (src/cg.hpp:182,195).  Result slots: 1 = p.y, 2 = r.z, 3 = r.z_old.
  int k = 0;
  while (k < cg->max_iter)
  {
    ++k;
    Range range("pmg:cg_iteration"); // src/cg.hpp:174,219
    PMG_TRY(A(p, y)); // :179
    PMG_TRY(dot_async(l, p, y, 1, s));
    PMG_TRY(reduce_slots_async(l, 1, 1, false, s));
    if (precond)
    {
      launch_cg_update2(n, x, r, p, y, rnorm, red_slot(l, 1), s); // :182-189
      PMG_TRY(precondition(y, r));
    }
    else
      launch_cg_update(n, x, r, y, p, dinv, rnorm, red_slot(l, 1), s); // :182-192 fused
    PMG_TRY(dot_async(l, r, y, 2, s)); // :195
    if (flex)
      PMG_TRY(dot_async(l, r, cg->zold, 3, s));
    PMG_TRY(reduce_slots_async(l, 2, flex ? 2 : 1, false, s));
    // :196,211 -- issued before the stopping test is known; if the loop ends here the new
    // direction is simply never used
    launch_cg_direction(n, p, y, rnorm, red_slot(l, 2), flex ? red_slot(l, 3) : nullptr, s);
    if (flex)
      PMG_HIP(hipMemcpyAsync(cg->zold, y, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
    double v[3] = {0, 0, 0};
    PMG_TRY(fetch_slots(l, 1, flex ? 3 : 2, v, s)); // the iteration's one host synchronisation
    const double alpha = rnorm / v[0]; // :182
    const double rnorm_new = v[1];
    // flexible: r_new . (z_new - z_old) / (r_old . z_old)
    const double beta = (flex ? rnorm_new - v[2] : rnorm_new) / rnorm;
    rnorm = rnorm_new;
    if (rnorm / rnorm0 < rtol2) // :206
      break;
    if (cg->store) // :213-218
    {
      cg->alphas.push_back(alpha);
      cg->betas.push_back(beta);
      cg->residuals.push_back(rnorm);
    }
  }
  if (!cg->store)
  {
    cg->residuals.clear();
    cg->residuals.push_back(rnorm);
  }
  if (iterations)
    *iterations = k;
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}
} // namespace pmg

extern "C" int pmg_cg_solve(pmg_cg cg, pmg_laplacian A, double* x, const double* b,
                            pmg_multigrid precond, int* iterations, pmg_stream stream)
{
  PMG_REQUIRE(cg && A && x && b, "pmg_cg_solve: NULL argument");
  PMG_REQUIRE(laplacian_layout(A) == cg->layout, "pmg_cg_solve: operator and solver layouts differ");
  hipStream_t s = S(stream);
  if (cg->nullspace != PMG_NULLSPACE_NONE)
    PMG_TRY(laplacian_require_singular(A, "pmg_cg_solve", s));
  const ApplyFn apply = [A, s](double* in, double* out) { return laplacian_apply(A, in, out, s); };
  // the V-cycle from a zero initial guess: folded into the smoothers' x_zero path, no memset of z
  const PrecondFn vcycle = [precond, s](double* z, const double* r) -> int
  {
    bool done = false;
    if (use_graph(precond))
      PMG_TRY(mg_apply_graph(precond, r, z, true, s, &done));
    return done ? PMG_OK : mg_apply(precond, r, z, true, s);
  };
  return cg_iterate(cg, apply, laplacian_diag_inv(A), precond ? &vcycle : nullptr, cg->flexible, x, b, iterations, s);
}

extern "C" int pmg_cg_solve_matrix(pmg_cg cg, pmg_matrix M, double* x, const double* b, pmg_multigrid precond,
                                   int* iterations, pmg_stream stream)
{
  PMG_REQUIRE(cg && M && x && b, "pmg_cg_solve_matrix: NULL argument");
  PMG_REQUIRE(matrix_layout(M) == cg->layout, "pmg_cg_solve_matrix: matrix and solver layouts differ");
  hipStream_t s = S(stream);
  if (cg->nullspace != PMG_NULLSPACE_NONE)
    PMG_TRY(laplacian_require_singular(matrix_source(M), "pmg_cg_solve_matrix", s));
  const ApplyFn apply = [M, s](double* in, double* out) { return matrix_apply(M, in, out, s); };
  const PrecondFn vcycle = [precond, s](double* z, const double* r) -> int
  {
    bool done = false;
    if (use_graph(precond))
      PMG_TRY(mg_apply_graph(precond, r, z, true, s, &done));
    return done ? PMG_OK : mg_apply(precond, r, z, true, s);
  };
  return cg_iterate(cg, apply, matrix_diag_inv(M), precond ? &vcycle : nullptr, cg->flexible, x, b, iterations, s);
}

extern "C" int pmg_cg_set_flexible(pmg_cg cg, int flag)
{
  PMG_REQUIRE(cg, "pmg_cg_set_flexible: NULL argument");
  cg->flexible = flag != 0;
  return PMG_OK;
}

extern "C" int pmg_cg_set_nullspace(pmg_cg cg, int mode)
{
  PMG_REQUIRE(mode == PMG_NULLSPACE_NONE || mode == PMG_NULLSPACE_CONSTANT, "pmg_cg_set_nullspace: unknown mode %d",
              mode);
  PMG_REQUIRE(cg, "pmg_cg_set_nullspace: NULL argument");
  cg->nullspace = mode;
  return PMG_OK;
}

extern "C" int pmg_cg_nullspace(pmg_cg cg) { return cg ? cg->nullspace : PMG_ERR_INVALID; }

extern "C" int pmg_cg_coefficients(pmg_cg cg, double* alphas, double* betas, int capacity)
{
  PMG_REQUIRE(cg, "pmg_cg_coefficients: NULL argument");
  int n = (int)cg->alphas.size();
  for (int i = 0; i < n && i < capacity; ++i)
  {
    if (alphas)
      alphas[i] = cg->alphas[i];
    if (betas)
      betas[i] = cg->betas[i];
  }
  return n;
}

// src/cg.hpp:121-142
extern "C" int pmg_cg_compute_eigenvalues(pmg_cg cg, double* eigs, int capacity)
{
  PMG_REQUIRE(cg && eigs, "pmg_cg_compute_eigenvalues: NULL argument");
  const int ne = (int)cg->alphas.size();
  if (ne < 2)
    return fail(PMG_ERR_INVALID, "Insufficient data to compute eigenvalues"); // :125
  PMG_REQUIRE(capacity >= ne, "pmg_cg_compute_eigenvalues: capacity %d < %d", capacity, ne);
  std::vector<double> d(ne, 0.0), e(ne, 0.0);
  for (int i = 0; i < ne; ++i)
    d[i] = 1.0 / cg->alphas[i];
  for (int i = 0; i < ne - 1; ++i)
  {
    d[i + 1] += cg->betas[i] / cg->alphas[i];
    e[i] = std::sqrt(cg->betas[i]) / cg->alphas[i];
  }
  if (pmg_tqli(d.data(), e.data(), ne) != PMG_OK)
    return fail(PMG_ERR_NUMERIC, "Eigenvalue estimate failed"); // :138
  std::sort(d.begin(), d.end());
  for (int i = 0; i < ne; ++i)
    eigs[i] = d[i];
  return ne;
}

extern "C" int pmg_cg_residual(pmg_cg cg, double* rnorm)
{
  PMG_REQUIRE(cg && rnorm, "pmg_cg_residual: NULL argument");
  PMG_REQUIRE(!cg->residuals.empty(), "pmg_cg_residual: no residual recorded");
  *rnorm = cg->residuals.back(); // src/cg.hpp:144
  return PMG_OK;
}

// -------------------------------------------------------------- multigrid --
extern "C" int pmg_multigrid_create(pmg_multigrid* out, int nlevels, const pmg_layout* layouts,
                                    const int8_t* bc_marker_coarsest)
{
  PMG_REQUIRE(out && layouts && nlevels >= 1, "pmg_multigrid_create: bad argument");
  PMG_REQUIRE(bc_marker_coarsest, "pmg_multigrid_create: NULL bc marker");
  auto* mg = new pmg_multigrid_s;
  HandleGuard<pmg_multigrid> guard(mg, pmg_multigrid_destroy);
  mg->L = nlevels;
  mg->layouts.assign(layouts, layouts + nlevels);
  mg->bc0 = bc_marker_coarsest;
  mg->u.assign(nlevels, nullptr);
  mg->b.assign(nlevels, nullptr);
  mg->counts.assign(nlevels, 0);
  mg->mats.assign(nlevels, nullptr);
  mg->mat_applies.assign(nlevels, 0);
  for (int i = 0; i < nlevels - 1; ++i) // src/pmg.hpp:35-41 (finest level: caller's vectors)
  {
    PMG_TRY(alloc_vec(layouts[i], &mg->u[i]));
    PMG_TRY(alloc_vec(layouts[i], &mg->b[i]));
  }
  *out = guard.release();
  return PMG_OK;
}

extern "C" int pmg_multigrid_set_coarse_solver(pmg_multigrid mg, pmg_cg coarse)
{
  PMG_REQUIRE(mg, "pmg_multigrid_set_coarse_solver: NULL argument");
  PMG_REQUIRE(!coarse || coarse->layout == mg->layouts[0],
              "pmg_multigrid_set_coarse_solver: the solver is not on the coarsest layout");
  drop_graphs(mg);
  mg->coarse = coarse;
  mg->coarse_fn = nullptr;
  mg->coarse_amg = nullptr;
  return PMG_OK;
}

extern "C" int pmg_multigrid_set_coarse_amg(pmg_multigrid mg, pmg_amg amg)
{
  PMG_REQUIRE(mg, "pmg_multigrid_set_coarse_amg: NULL argument");
  PMG_REQUIRE(!amg || amg_layout(amg) == mg->layouts[0],
              "pmg_multigrid_set_coarse_amg: the solver is not on the coarsest layout");
  drop_graphs(mg);
  mg->coarse_amg = amg;
  if (amg)
  {
    mg->coarse = nullptr;
    mg->coarse_fn = nullptr;
  }
  return PMG_OK;
}

extern "C" int pmg_multigrid_set_coarse_callback(pmg_multigrid mg, pmg_coarse_solve_fn solve, void* user)
{
  PMG_REQUIRE(mg, "pmg_multigrid_set_coarse_callback: NULL argument");
  drop_graphs(mg);
  mg->coarse_fn = solve;
  mg->coarse_user = user;
  if (solve)
  {
    mg->coarse = nullptr;
    mg->coarse_amg = nullptr;
  }
  return PMG_OK;
}

extern "C" int pmg_multigrid_destroy(pmg_multigrid mg)
{
  if (!mg)
    return PMG_OK;
  for (int i = 0; i < mg->L - 1; ++i)
  {
    (void)hipFree(mg->u[i]);
    (void)hipFree(mg->b[i]);
  }
  for (auto& g : mg->graphs)
    (void)hipGraphExecDestroy(g.exec);
  if (mg->capture_stream)
    (void)hipStreamDestroy(mg->capture_stream);
  free_f32(mg);
  delete mg;
  return PMG_OK;
}

extern "C" int pmg_multigrid_set_operators(pmg_multigrid mg, const pmg_laplacian* ops)
{
  PMG_REQUIRE(mg && ops, "pmg_multigrid_set_operators: NULL argument");
  for (int i = 0; i < mg->L; ++i)
    PMG_REQUIRE(ops[i] && laplacian_layout(ops[i]) == mg->layouts[i],
                "pmg_multigrid_set_operators: level %d layout mismatch", i);
  drop_graphs(mg);
  mg->ops.assign(ops, ops + mg->L);
  return PMG_OK;
}

extern "C" int pmg_multigrid_set_solvers(pmg_multigrid mg, const pmg_chebyshev* smoothers)
{
  PMG_REQUIRE(mg && smoothers, "pmg_multigrid_set_solvers: NULL argument");
  for (int i = 0; i < mg->L; ++i)
    PMG_REQUIRE(smoothers[i] && smoothers[i]->layout == mg->layouts[i],
                "pmg_multigrid_set_solvers: level %d layout mismatch", i);
  drop_graphs(mg);
  mg->smoothers.assign(smoothers, smoothers + mg->L);
  return PMG_OK;
}

extern "C" int pmg_multigrid_set_interpolators(pmg_multigrid mg, const pmg_interpolator* interp)
{
  PMG_REQUIRE(mg && (interp || mg->L == 1), "pmg_multigrid_set_interpolators: NULL argument");
  drop_graphs(mg);
  mg->interps.clear();
  for (int i = 0; i < mg->L - 1; ++i)
  {
    PMG_REQUIRE(interp[i], "pmg_multigrid_set_interpolators: level %d is NULL", i);
    mg->interps.push_back(interp[i]);
  }
  return PMG_OK;
}

namespace
{
void drop_graphs(pmg_multigrid mg)
{
  for (auto& g : mg->graphs)
    (void)hipGraphExecDestroy(g.exec);
  mg->graphs.clear();
}

// What a captured cycle depends on besides its two vectors; -1: this configuration cannot be
// captured (a host synchronisation or a host callback inside the cycle, in-situ timing events)
// Is the cycle replayed as a hipGraph?  Explicitly on / off (pmg_multigrid_set_graph), or by default: on one rank the
// launches are issued ahead of the GPU anyway and a replay buys nothing (5.40 against 5.42 ms at config 2); on several
// ranks an eager exchange costs the host more than the GPU (profiles/exchange_overhead_r02.txt; four ranks on one GPU,
// round 4: 8.4 ms eager against 6.3 ms replayed at 64^3 in total), so the cycle is captured BY DEFAULT wherever the
// capture holds nothing but kernels -- every exchange through halo windows, every reduction of the cycle through a
// communicator made of windows.  A cycle whose exchanges are RCCL calls is captured on request only: that capture
// has run on one GPU (a rank as its own partner), never between two, and a runtime that misbehaves there would take
// the caller's run down rather than fail a check (PMG_GRAPH_AUTO=rccl includes it in the default, =0 turns the
// default off).
bool use_graph(pmg_multigrid mg)
{
  if (mg->graph_mode >= 0)
    return mg->graph_mode == 1;
  const char* e = std::getenv("PMG_GRAPH_AUTO");
  if (e && e[0] == '0')
    return false;
  const bool rccl_too = e && std::string(e) == "rccl";
  bool several = false;
  for (int i = 0; i < mg->L; ++i)
  {
    pmg_layout l = mg->layouts[i];
    if (!l->multi_rank() && !l->win)
      continue;
    several = true;
    if (l->exchange && !l->comm && !l->win)
      return false; // callbacks: host code in the cycle
    if (!l->win && !rccl_too)
      return false; // grouped ncclSend / ncclRecv in the capture
    if (mg->coarse_amg && i == 0 && l->comm && !l->comm->wcomm && !rccl_too)
      return false; // the replicated coarse solve's ncclAllReduce in the capture
  }
  return several;
}

long long capture_config(pmg_multigrid mg)
{
  uint64_t h = 1469598103934665603ull;
  auto mix = [&h](uint64_t v) { h = (h ^ v) * 1099511628211ull; };
  for (int i = 0; i < mg->L; ++i)
  {
    pmg_layout l = mg->layouts[i];
    // halo: the caller's callbacks are host code inside the cycle.  The library's grouped ncclSend / ncclRecv are
    // captured on the capture stream itself (comm_exchange_begin; forking to the communicator's stream inside a
    // capture crashes RCCL 2.26).
    if (l->exchange && !l->comm && !l->win)
      return -1;
    // first use of a peer connection / of the collective must not fall inside a capture: eager until every level's
    // layout has exchanged once (and, with the replicated AMG's all-reduce, the communicator has reduced once)
    if (!comm_capture_ready(l, i == 0 && mg->coarse_amg != nullptr))
      return -1;
    const long long st = laplacian_capture_state(mg->ops[i]);
    if (st < 0)
      return -1;
    mix((uint64_t)st);
    // identities: a graph replays the device pointers of the objects it was captured with (the setters drop the
    // cache as well; this covers an object replaced by another one at the same address only by accident)
    mix((uint64_t)(uintptr_t)mg->ops[i]);
    mix((uint64_t)(uintptr_t)mg->smoothers[i]);
    mix((uint64_t)(uintptr_t)mg->mats[i]); // the set of assembled levels
    mix((uint64_t)(uintptr_t)l->comm);
    mix((uint64_t)(uintptr_t)l->win);
    if (i + 1 < mg->L)
      mix((uint64_t)(uintptr_t)mg->interps[i]);
    mix((uint64_t)mg->smoothers[i]->max_iter);
    mix((uint64_t)(mg->smoothers[i]->recompute_mode + 1)); // the form decides which buffers the cycle's kernels hold
    uint64_t bits;
    static_assert(sizeof(bits) == sizeof(double), "");
    memcpy(&bits, &mg->smoothers[i]->eig_max, sizeof(bits));
    mix(bits);
  }
  if (mg->coarse || mg->coarse_fn) // Krylov coarse solve / caller's solver: host in the loop
    return -1;
  mix((uint64_t)mg->precision);
  mix((uint64_t)(mg->fused_mode + 1));
  if (mg->precision == PMG_PRECISION_FP32) // the float diagonals are converted when the cycle is captured
    for (int i = 0; i < mg->L; ++i)
      mix((uint64_t)laplacian_diag_version(mg->ops[i]));
  if (mg->coarse_amg)
  {
    const long long st = amg_capture_state(mg->coarse_amg);
    if (st < 0)
      return -1;
    mix((uint64_t)st);
    mix((uint64_t)(uintptr_t)mg->coarse_amg);
  }
  return (long long)(h >> 1);
}

// mg_apply through a graph: captured on the library's own stream the first time a
// (vectors, configuration) combination is seen, replayed on the caller's stream afterwards
int mg_apply_graph(pmg_multigrid mg, const double* rhs, double* y, bool y_zero, hipStream_t s, bool* done)
{
  *done = false;
  if ((int)mg->ops.size() != mg->L || (int)mg->smoothers.size() != mg->L || (int)mg->interps.size() != mg->L - 1)
    return PMG_OK; // mg_apply reports it
  const long long cfg = capture_config(mg);
  if (cfg < 0)
    return PMG_OK;
  for (auto& g : mg->graphs)
    if (g.rhs == rhs && g.y == y && g.y_zero == y_zero && g.config == (uint64_t)cfg)
    {
      PMG_HIP(hipGraphLaunch(g.exec, s));
      mg->counts = g.counts;
      mg->fused_count = g.fused_count;
      for (int i = 0; i < mg->L; ++i)
        mg->smoothers[i]->recomputed += g.recomputed[i];
      mg->graph_replays++;
      *done = true;
      return PMG_OK;
    }
  if (mg->precision == PMG_PRECISION_FP32) // allocations and conversions on the caller's stream, outside the capture
    PMG_TRY(mg_prepare_f32(mg, s));
  else // ... and so are the product vectors of the smoothers of which a call of this cycle takes the recomputed form
    for (int i = 0; i < mg->L; ++i)
      for (SmoothRole role : {PreSmooth, CoarseSmooth, PostSmooth})
        if (cycle_smooths(mg, i, role) && smooth_outcome(level_call(mg, i, role, y_zero)).recomputed)
          PMG_TRY(recompute_buffers(mg->smoothers[i], s));
  std::vector<long long> recomputed_before(mg->L);
  for (int i = 0; i < mg->L; ++i)
    recomputed_before[i] = mg->smoothers[i]->recomputed;
  if (!mg->capture_stream)
    PMG_HIP(hipStreamCreateWithFlags(&mg->capture_stream, hipStreamNonBlocking));
  PMG_HIP(hipStreamBeginCapture(mg->capture_stream, hipStreamCaptureModeRelaxed));
  const int rc = mg_apply(mg, rhs, y, y_zero, mg->capture_stream);
  hipGraph_t graph = nullptr;
  const hipError_t e = hipStreamEndCapture(mg->capture_stream, &graph);
  if (rc != PMG_OK)
  {
    if (graph)
      (void)hipGraphDestroy(graph);
    return rc;
  }
  if (e != hipSuccess || !graph)
    return fail(PMG_ERR_HIP, "capturing the V-cycle failed: %s", hipGetErrorString(e));
  pmg_multigrid_s::GraphEntry g{rhs, y, y_zero, (uint64_t)cfg, nullptr, mg->counts, mg->fused_count, {}};
  for (int i = 0; i < mg->L; ++i)
    g.recomputed.push_back((int)(mg->smoothers[i]->recomputed - recomputed_before[i]));
  const hipError_t ei = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (ei != hipSuccess)
    return fail(PMG_ERR_HIP, "instantiating the V-cycle graph failed: %s", hipGetErrorString(ei));
  if (mg->graphs.size() >= 16) // callers that cycle through many vectors: keep the cache small
    drop_graphs(mg);
  mg->graphs.push_back(g);
  PMG_HIP(hipGraphLaunch(g.exec, s));
  mg->graph_replays++;
  *done = true;
  return PMG_OK;
}
} // namespace

extern "C" int pmg_multigrid_set_graph(pmg_multigrid mg, int enable)
{
  PMG_REQUIRE(mg, "pmg_multigrid_set_graph: NULL argument");
  drop_graphs(mg);
  mg->graph_mode = enable < 0 ? -1 : (enable != 0 ? 1 : 0);
  return PMG_OK;
}

extern "C" int pmg_multigrid_set_fused_restriction(pmg_multigrid mg, int mode)
{
  PMG_REQUIRE(mg, "pmg_multigrid_set_fused_restriction: NULL argument");
  PMG_REQUIRE(mode == -1 || mode == 0, "pmg_multigrid_set_fused_restriction: mode %d (-1 automatic, 0 never)", mode);
  drop_graphs(mg);
  mg->fused_mode = mode;
  return PMG_OK;
}

extern "C" int pmg_multigrid_fused_restrictions(pmg_multigrid mg) { return mg ? mg->fused_count : -1; }

extern "C" int pmg_multigrid_set_precision(pmg_multigrid mg, int precision)
{
  PMG_REQUIRE(mg, "pmg_multigrid_set_precision: NULL argument");
  PMG_REQUIRE(precision == PMG_PRECISION_FP64 || precision == PMG_PRECISION_FP32,
              "pmg_multigrid_set_precision: unknown precision %d (PMG_PRECISION_FP64 or PMG_PRECISION_FP32)", precision);
  if (precision == PMG_PRECISION_FP32)
  {
    for (int i = 0; i < mg->L; ++i)
      PMG_REQUIRE(!mg->mats[i],
                  "pmg_multigrid_set_precision: level %d has an assembled matrix and there is no FP32 matrix "
                  "(pmg_multigrid_set_level_matrix(mg, %d, NULL) removes it)", i, i);
    PMG_TRY(mg_check_f32(mg, "pmg_multigrid_set_precision"));
  }
  drop_graphs(mg);
  mg->precision = precision;
  return PMG_OK;
}

extern "C" int pmg_multigrid_set_level_matrix(pmg_multigrid mg, int level, pmg_matrix M)
{
  PMG_REQUIRE(mg, "pmg_multigrid_set_level_matrix: NULL argument");
  PMG_REQUIRE(level >= 0 && level < mg->L, "pmg_multigrid_set_level_matrix: level %d of %d", level, mg->L);
  if (M)
  {
    PMG_REQUIRE(matrix_layout(M) == mg->layouts[level],
                "pmg_multigrid_set_level_matrix: the matrix is not on level %d's layout", level);
    PMG_REQUIRE(mg->precision != PMG_PRECISION_FP32,
                "pmg_multigrid_set_level_matrix: the cycle runs in FP32 and there is no FP32 matrix "
                "(pmg_multigrid_set_precision(mg, PMG_PRECISION_FP64) first)");
  }
  drop_graphs(mg);
  mg->mats[level] = M;
  return PMG_OK;
}

extern "C" int pmg_multigrid_precision(pmg_multigrid mg) { return mg ? mg->precision : PMG_ERR_INVALID; }

extern "C" long long pmg_multigrid_graph_replays(pmg_multigrid mg) { return mg ? mg->graph_replays : -1; }

extern "C" int pmg_multigrid_apply(pmg_multigrid mg, const double* rhs, double* y, double* rnorm,
                                   pmg_stream stream)
{
  PMG_REQUIRE(mg && rhs && y, "pmg_multigrid_apply: NULL argument");
  hipStream_t s = S(stream);
  bool done = false;
  if (use_graph(mg))
    PMG_TRY(mg_apply_graph(mg, rhs, y, false, s, &done));
  if (!done)
    PMG_TRY(mg_apply(mg, rhs, y, false, s));
  if (rnorm) // src/pmg.hpp:141-150
  {
    const int L = mg->L;
    pmg_chebyshev sm = mg->smoothers[L - 1];
    if (mg->mats[L - 1]) // the level's residual in the level's form
      PMG_TRY(matrix_apply(mg->mats[L - 1], y, sm->q, s));
    else
      PMG_TRY(laplacian_apply(mg->ops[L - 1], y, sm->q, s));
    launch_axpy(mg->layouts[L - 1]->size_local, sm->r, -1.0, sm->q, rhs, s);
    double v;
    PMG_TRY(dot_host(mg->layouts[L - 1], sm->r, sm->r, &v, s));
    *rnorm = std::sqrt(v);
  }
  return PMG_OK;
}

extern "C" int pmg_multigrid_apply_counts(pmg_multigrid mg, int* counts, int capacity)
{
  PMG_REQUIRE(mg && counts, "pmg_multigrid_apply_counts: NULL argument");
  for (int i = 0; i < mg->L && i < capacity; ++i)
    counts[i] = mg->counts[i];
  return mg->L;
}
