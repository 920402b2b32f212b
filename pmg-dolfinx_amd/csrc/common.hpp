// Shared definitions of the pmg_amd library (gfx950 only).
#pragma once

#include "../../include/pmg_amd.h"
#include "smooth_plan.hpp"

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <functional>
#include <string>
#include <type_traits>
#include <vector>

namespace pmg
{
extern thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...);

#define PMG_HIP(call)                                                                              \
  do                                                                                               \
  {                                                                                                \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return pmg::fail(PMG_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),         \
                       __FILE__, __LINE__);                                                        \
  } while (0)

#define PMG_TRY(call)                                                                              \
  do                                                                                               \
  {                                                                                                \
    int rc_ = (call);                                                                              \
    if (rc_ != PMG_OK)                                                                             \
      return rc_;                                                                                  \
  } while (0)

#define PMG_REQUIRE(cond, ...)                                                                     \
  do                                                                                               \
  {                                                                                                \
    if (!(cond))                                                                                   \
      return pmg::fail(PMG_ERR_INVALID, __VA_ARGS__);                                              \
  } while (0)

inline hipStream_t S(pmg_stream s) { return reinterpret_cast<hipStream_t>(s); }

// refuses, with the caller's message, a call that allocates, synchronises or reads back while `s` is being captured
inline int not_capturing(hipStream_t s, const char* what)
{
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  PMG_HIP(hipStreamIsCapturing(s, &cap));
  PMG_REQUIRE(cap == hipStreamCaptureStatusNone, "%s", what);
  return PMG_OK;
}

// a device copy of the host array src[0, n) (at least one element is allocated), stream-ordered
template <typename T>
int upload(T** dst, const T* src, size_t n, hipStream_t s)
{
  PMG_HIP(hipMalloc(dst, sizeof(T) * (n ? n : 1)));
  if (n)
    PMG_HIP(hipMemcpyAsync(*dst, src, sizeof(T) * n, hipMemcpyHostToDevice, s));
  return PMG_OK;
}

constexpr int MAXND = PMG_MAX_DEGREE + 1;

// f(std::integral_constant<int, P>{}) -> int for the run-time degree P: the one dispatch onto the kernels' degree
template <typename F>
int with_degree(int P, F&& f)
{
  switch (P)
  {
  case 1: return f(std::integral_constant<int, 1>{});
  case 2: return f(std::integral_constant<int, 2>{});
  case 3: return f(std::integral_constant<int, 3>{});
  case 4: return f(std::integral_constant<int, 4>{});
  case 5: return f(std::integral_constant<int, 5>{});
  case 6: return f(std::integral_constant<int, 6>{});
  case 7: return f(std::integral_constant<int, 7>{});
  case 8: return f(std::integral_constant<int, 8>{});
  default: return fail(PMG_ERR_INVALID, "Unsupported degree"); // src/laplacian.hpp:346,479
  }
}
static_assert(PMG_MAX_DEGREE == 8, "with_degree lists the degrees");

// 1-D tables on the host (tables.cpp)
void gll_table(int n, double* x, double* w);
void lagrange_derivative_table(int n, const double* x, double* D);
void lagrange_eval_table(int nc, const double* xc, int nf, const double* xf, double* M);
// coordinate element of degree g: its 1-D basis / derivative at the n points x, L / Lp [n][g+1], and the dense
// tabulation dphi[3][nd^3][m^3] they give (tables.hip)
void coordinate_element_tables_1d(int n, const double* x, int g, double* L, double* Lp);
void coordinate_element_table_3d(int nd, int m, const double* L, const double* Lp, double* dphi);

// Cell-local node order (pmg_amd.h "cell-local node order"; tables.hip).  perm1d[j] = ascending position of the
// caller's 1-D node j; node_permutation validates / builds it, cell_permutation expands it to the nd^3 cell-local
// numbers (perm3[t_caller] = t_ascending, t = ja*nd^2 + jb*nd + jc).
int node_permutation(int node_order, int degree, const int32_t* custom, std::vector<int32_t>& perm1d);
std::vector<int32_t> cell_permutation(int nd, const std::vector<int32_t>& perm1d);
inline bool is_identity(const std::vector<int32_t>& p)
{
  for (size_t i = 0; i < p.size(); ++i)
    if (p[i] != (int32_t)i)
      return false;
  return true;
}
// out[row * n + perm[t]] (x width) = in[row * n + t] (x width) on the device; perm is a device array of n entries
int permute_rows_i32(long long nrows, int n, const int32_t* perm_d, const int32_t* in, int32_t* out, hipStream_t s);
int permute_rows_f64(long long nrows, int n, int width, const int32_t* perm_d, const double* in, double* out,
                     hipStream_t s);

// Kernel-argument copy of a small dense table (<= 9x9), passed by value.
struct Table
{
  double v[MAXND * MAXND];
};
} // namespace pmg

// Destroys a half-built handle when a constructor returns early through
// PMG_REQUIRE / PMG_TRY / PMG_HIP; release() hands the finished handle over.
template <typename H>
struct HandleGuard
{
  H h;
  int (*destroy)(H);
  HandleGuard(H handle, int (*d)(H)) : h(handle), destroy(d) {}
  HandleGuard(const HandleGuard&) = delete;
  HandleGuard& operator=(const HandleGuard&) = delete;
  ~HandleGuard()
  {
    if (h)
      destroy(h);
  }
  H release()
  {
    H t = h;
    h = nullptr;
    return t;
  }
};

struct ncclComm;
struct pmg_window_s;
struct pmg_window_comm_s;

// One process's communicator: RCCL (comm.hip) or, without any transport library, a window of device memory that
// every rank has mapped (window.hip: reductions and set-up gathers as direct stores + flags; the halo of its layouts
// then has to be halo windows as well).
struct pmg_comm_s
{
  ncclComm* comm = nullptr;
  pmg_window_comm_s* wcomm = nullptr;
  int rank = 0, nranks = 1;
  hipStream_t stream = nullptr; // every RCCL call of this communicator is issued here, in program order
  hipEvent_t ev_in = nullptr, ev_out = nullptr; // reductions: compute stream -> comm stream -> compute stream
  bool reduced_eagerly = false; // an all-reduce has been issued outside a capture (see comm_capture_ready)
};

struct pmg_layout_s
{
  int32_t size_local = 0, num_ghosts = 0, n_send = 0, n_recv = 0;
  // native communicator (comm.hip): when set, the exchange and the reductions are issued by the
  // library on RCCL and the callbacks below are not used
  pmg_comm_s* comm = nullptr;
  std::vector<int32_t> nb_rank, nb_send, nb_recv; // neighbour ranks and per-neighbour counts
  hipEvent_t ev_packed = nullptr, ev_arrived = nullptr;
  // staging of the native exchange (owned): every neighbour's segment starts on a 256-byte boundary -- RCCL moves a
  // 7-segment halo 22 % faster than with segments that are only 8-byte aligned (tools/time_halo_alignment.py);
  // *_pos[i] = place of list entry i in the padded buffer, *_off[k] = start of neighbour k's segment
  double *c_send = nullptr, *c_recv = nullptr;
  int32_t *send_pos = nullptr, *recv_pos = nullptr;
  std::vector<size_t> send_off, recv_off;
  // halo windows (window.hip): when set, the neighbour exchange is direct stores into the neighbours' windows;
  // the reductions still go through `comm` or the callbacks
  pmg_window_s* win = nullptr;
  bool exchange_inline = false; // the exchange in flight was issued on the compute stream (graph capture)
  bool exchanged_eagerly = false; // an exchange of this layout has been issued outside a capture (comm_capture_ready)
  const int32_t* send_idx = nullptr;
  const int32_t* recv_idx = nullptr;
  double* send_buf = nullptr;
  double* recv_buf = nullptr;
  pmg_exchange_fn exchange = nullptr;
  pmg_allreduce_fn allreduce = nullptr;
  pmg_allreduce_fn allreduce_max = nullptr;
  void* user = nullptr;
  // reduction scratch (owned)
  double* d_partials = nullptr; // [RED_BLOCKS] block partials + [RED_SLOTS] results
  double* h_result = nullptr;   // pinned, [RED_SLOTS]
  // the constant null space (pmg_vec_remove_mean, pmg_cg_set_nullspace): partials of up to three sums formed in one
  // pass, [3][RED_BLOCKS] behind the result slots of d_partials (not owned separately), and N, the number of owned
  // entries over all ranks (-1: not yet counted; layout_global_size)
  double* d_partials_multi = nullptr;
  long long global_size = -1;
  long long fwd_scatters = 0; // forward scatters issued (pmg_layout_forward_scatters: exchange bookkeeping tests)
  bool multi_rank() const { return comm != nullptr || allreduce != nullptr; }
  int32_t total() const { return size_local + num_ghosts; }
};

namespace pmg
{
constexpr int RED_BLOCKS = 1024;
constexpr int RED_THREADS = 256;
constexpr int RED_SLOTS = 8;

// comm.hip -- native (RCCL) exchange and reductions of a layout that has a communicator
int comm_exchange_begin(pmg_layout l, bool reverse, hipStream_t s);
int comm_exchange_end(pmg_layout l, hipStream_t s);
int comm_allreduce(pmg_layout l, double* d_values, int n, bool max, hipStream_t s);
int comm_allreduce(pmg_comm c, double* d_values, int n, bool max, hipStream_t s);
bool comm_capture_ready(pmg_layout l, bool with_allreduce);

// window.hip -- the exchange of a layout that has halo windows (x: the whole vector, owned entries first)
int window_exchange_begin(pmg_layout l, bool reverse, const double* x, hipStream_t s);
int window_exchange_end(pmg_layout l, bool reverse, double* x, hipStream_t s);
int window_exchange_whole(pmg_layout l, double* x, hipStream_t s);
// owner -> ghost exchange of x, complete on return of the stream: one launch on a window layout, begin + end otherwise
int scatter_fwd_whole(pmg_layout l, double* x, hipStream_t s);
// is the exchange of this layout one that a small level should take whole, in front of ONE launch over all its cells,
// rather than split around the interior cells' launch?  (halo windows; PMG_FUSED_EXCHANGE=0 in the environment: never)
bool layout_exchanges_whole(pmg_layout l);
void window_destroy(pmg_layout l);
// ... and the reductions / set-up gathers of a communicator made of windows
int wcomm_allreduce(pmg_comm c, double* d_values, int n, bool max, hipStream_t s);
int wcomm_allgather(pmg_comm c, const void* send, size_t bytes, void* recv);
void wcomm_destroy(pmg_comm c);

// Profiling ranges (roctx, bound at run time; no-ops when libroctx64 is absent).  The reference
// annotates each CG iteration (src/amd_gpu.hpp:236-252, src/cg.hpp:174,219); here every phase of
// the V-cycle carries a range as well, so a rocprofv3 --marker-trace reads like the algorithm.
void range_push(const char* name);
void range_pop();
struct Range
{
  explicit Range(const char* name) { range_push(name); }
  Range(const Range&) = delete;
  Range& operator=(const Range&) = delete;
  ~Range() { range_pop(); }
};

// solvers.hip -- the 4th-kind Chebyshev / Jacobi smoother (src/chebyshev.hpp:46-91) and the CG loop
// (src/cg.hpp:147-222) over ANY operator and preconditioner given as callables (the matrix-free
// Laplacian, an assembled CSR level of the AMG hierarchy; the diagonal, a V-cycle, an AMG cycle)
// The smoother and its vector passes exist for T = double and, for the FP32 V-cycle, T = float.
template <typename T>
struct ChebWork
{
  T *r = nullptr, *z = nullptr, *q = nullptr;
  T *q1 = nullptr, *q2 = nullptr; // the recomputed form's further products: its three go to q, q1 and q2
};
template <typename T>
using ApplyFnT = std::function<int(T* in, T* out)>;
using ApplyFn = ApplyFnT<double>;
using PrecondFn = std::function<int(double* z, const double* r)>;
int cg_iterate(pmg_cg cg, const ApplyFn& A, const double* dinv, const PrecondFn* M, bool flexible, double* x,
               const double* b, int* iterations, hipStream_t s);
// The smoother's control flow is not here: smooth_plan.hpp decides once, on the host, which applications and passes a
// call issues (SmoothCall -> for_each_smooth_step) and what it leaves to its consumer (smooth_outcome).  cheb_iterate
// is the interpreter: it turns each step into the launch_cheb_* / launch_add / launch_zero / hipMemcpyAsync call below
// or into an application through apply[step.variant], and returns the visitor's refusal for a call that cannot be
// scheduled.  The caller fills in the SmoothCall from what it knows (steps, what it can consume of the residual, the
// operator's output rule, the ghost bookkeeping, the smoother's mode and buffers) and the data the steps work on.
template <typename T>
struct SmoothData
{
  ChebWork<T> w;        // r, z, q; q1 and q2 where the call allows the recomputed form
  ApplyFnT<T> apply[3]; // by SmoothStep::Variant: plain, zeroed-output, ghosts-current -- those the call can ask for
  const T* dinv = nullptr;
  int n = 0, n_total = 0; // owned entries; with the ghosts behind them (read only with call.ghosts or zeroed_output)
  double lmax = 1;
  T* x = nullptr;
  const T* b = nullptr;
  hipStream_t s = nullptr;
};
template <typename T>
int cheb_iterate(const SmoothCall& call, const SmoothData<T>& d);

// vector.hip -- stream-ordered building blocks used by the solvers
// local dot of the owned entries into the result slot `slot` of the layout (device)
int dot_async(pmg_layout l, const double* a, const double* b, int slot, hipStream_t s);
double* red_slot(pmg_layout l, int slot);
// sum / maximise the slots [slot, slot + n) over the ranks; the device slots then hold the global values
int reduce_slots_async(pmg_layout l, int slot, int n, bool max, hipStream_t s);
// ... and bring them to the host: the one host synchronisation of a reduction
int fetch_slots(pmg_layout l, int slot, int n, double* host_out, hipStream_t s);
int dot_host(pmg_layout l, const double* a, const double* b, double* result, hipStream_t s);
void launch_axpy(int n, double* r, double alpha, const double* x, const double* y, hipStream_t s);
void launch_pointwise(int n, double* w, const double* x, const double* y, hipStream_t s);
// Chebyshev fused passes (src/chebyshev.hpp:57-83)
// clear_q (optional): the operator's output, zeroed over [0, n_total) behind the update (see ThenClearF)
void launch_cheb_init(int n, double* r, double* z, const double* b, const double* q, const double* dinv, double c0,
                      hipStream_t s, double* clear_q = nullptr, int n_total = 0);
void launch_cheb_step(int n, double* x, double* r, double* z, const double* q, const double* dinv, double c1, double c2,
                      bool both, int x_final, hipStream_t s, double* clear_q = nullptr, int n_total = 0);
void launch_cheb_first(int n, double* x, double* r, double* z, const double* q, const double* dinv, double c1,
                       double c2, int x_final, hipStream_t s, double* clear_q = nullptr, int n_total = 0);
void launch_cheb_residual(int n, double* r, const double* q, hipStream_t s);
// the recomputed form's kernels (stage 1, 2, 3 of ChebRecomputeF); c = {c0, c1 and c2 of step 1, c1 and c2 of step 2}
void launch_cheb_recompute(int n, int stage, double* x, double* r_out, double* z_out, const double* b,
                           const double* q0, const double* q1, const double* q2, const double* dinv, const double c[5],
                           hipStream_t s);
// does a level of n dofs stream its vectors (the nt policy of the smoother kernels)?
bool vector_streams(int n);
void launch_add(int n, double* x, const double* z, hipStream_t s);
void launch_cheb_last(int n, double* x, double* r, const double* z, const double* q, bool assign, hipStream_t s);
void launch_zero(int n, double* x, hipStream_t s);
void launch_mask_bc(int n, double* b, const int8_t* bc, hipStream_t s);
// The same passes for the FP32 cycle: one element per lane, default cache policy.  They have no zeroed-output form: a
// non-null clear_q ends the process with a message (the smooth's schedule refuses such an operator before it gets here).
void launch_cheb_init(int n, float* r, float* z, const float* b, const float* q, const float* dinv, float c0,
                      hipStream_t s, float* clear_q = nullptr, int n_total = 0);
void launch_cheb_step(int n, float* x, float* r, float* z, const float* q, const float* dinv, float c1, float c2,
                      bool both, int x_final, hipStream_t s, float* clear_q = nullptr, int n_total = 0);
void launch_cheb_first(int n, float* x, float* r, float* z, const float* q, const float* dinv, float c1,
                       float c2, int x_final, hipStream_t s, float* clear_q = nullptr, int n_total = 0);
void launch_cheb_residual(int n, float* r, const float* q, hipStream_t s);
void launch_add(int n, float* x, const float* z, hipStream_t s);
void launch_cheb_last(int n, float* x, float* r, const float* z, const float* q, bool assign, hipStream_t s);
void launch_zero(int n, float* x, hipStream_t s);
void launch_mask_bc(int n, float* b, const int8_t* bc, hipStream_t s);
// CG fused passes (src/cg.hpp:160-211); alpha = rnorm / *d_py and beta = (*d_new - *d_sub) / rnorm are
// formed on the device from the reduced scalars, so no host round trip sits between the kernels
void launch_cg_update(int n, double* x, double* r, double* y, const double* p, const double* dinv,
                      double rnorm, const double* d_py, hipStream_t s);
void launch_cg_update2(int n, double* x, double* r, const double* p, const double* y, double rnorm,
                       const double* d_py, hipStream_t s);
void launch_cg_direction(int n, double* p, const double* y, double rnorm, const double* d_new,
                         const double* d_sub, hipStream_t s);
// The constant null space (pmg_cg_set_nullspace).  r . z of the projected iteration,
// r . z - (1 . r)(1 . z) / N: the ONE expression, evaluated on the device for alpha and beta and on the host for the
// stopping test, with its roundings fixed so that both get the same bits.
__host__ __device__ inline double projected_rz(double rz, double sum_r, double sum_z, double N)
{
#pragma clang fp contract(off)
  const double t = sum_r * sum_z;
  return rz - t / N;
}
// r . z, 1 . r, 1 . z of the owned entries -> result slots [slot, slot + 3) in one pass; with dinv, z = dinv r is formed
// and stored in that pass
int cg_sums3_async(pmg_layout l, const double* r, double* z, const double* dinv, int slot, hipStream_t s);
// x += alpha p ; r -= alpha y with alpha = projected_rz(d_rz[0..2], N) / *d_py
void launch_cg_update2_null(int n, double* x, double* r, const double* p, const double* y, const double* d_rz,
                            double N, const double* d_py, hipStream_t s);
// p = (z - d_rz[2] / N) + beta p, beta = (projected_rz(d_rz[0..2]) - projected_rz(*d_sub, d_rz[1], sz_old)) / rnorm
// (d_sub optional: the flexible variant); first: p = z - d_rz[2] / N, p is not read
void launch_cg_direction_null(int n, double* p, const double* z, bool first, double rnorm, const double* d_rz,
                              const double* d_sub, double sz_old, double N, hipStream_t s);
// sum of one host count over the layout's ranks (slot 7); one rank: no device work; several: collective, synchronises
// and reads back -- refused with `what` inside a stream capture
int sum_count_over_ranks(pmg_layout l, long long mine, long long* total, const char* what, hipStream_t s);
// N = owned entries over all ranks (cached in the layout; the first call on several ranks reduces and reads back)
int layout_global_size(pmg_layout l, double* N, hipStream_t s);
// x <- x - (sum x) / N, or with weights x <- x - (w . x) / (w . 1), over size_local + num_ghosts entries; no host
// synchronisation (result slots 6 and 7), capturable
int remove_mean_async(pmg_layout l, double* x, const double* w, hipStream_t s);
// the operator can carry the constant null space: no marked row on any rank, no reaction, no Robin term -- else the
// refusal (PMG_ERR_INVALID), in `who`'s name.  The count of marked rows is reduced once per operator and cached.
int laplacian_require_singular(pmg_laplacian op, const char* who, hipStream_t s);
pmg_laplacian matrix_source(pmg_matrix M);
// laplacian.hip -- the matrix-free operator, as the solvers, the AMG set-up and the assembled operator use it
int laplacian_apply(pmg_laplacian op, double* in, double* out, hipStream_t s);
int laplacian_apply_zeroed(pmg_laplacian op, double* in, double* out, hipStream_t s);
int laplacian_apply_ghosts_current(pmg_laplacian op, double* in, double* out, hipStream_t s);
bool laplacian_wants_zeroed_output(pmg_laplacian op);
bool laplacian_single_launch(pmg_laplacian op); // a small level on halo windows: the exchange whole, then one launch
const double* laplacian_diag_inv(pmg_laplacian op);
const double* laplacian_reaction(pmg_laplacian op); // the diagonal term, d_sigma + d_R; nullptr = none
// An input of the operator was set or removed -- the nodal field, the per-cell tensor, a component of the diagonal term
// (pmg_laplacian_set_reaction, pmg_laplacian_set_robin) --: rebuild, in place, everything that follows it (the
// dependency list is at the definition); waits for the stream.  `changed`: a sum of OperatorData values.
enum OperatorData : unsigned
{
  DATA_FIELD = 1,
  DATA_TENSOR = 2,
  DATA_DIAGONAL_TERM = 4
};
int laplacian_data_changed(pmg_laplacian op, unsigned changed, hipStream_t s);
pmg_layout laplacian_layout(pmg_laplacian op);
long long laplacian_launches(pmg_laplacian op);
long long laplacian_capture_state(pmg_laplacian op); // -1 = not capturable right now
int laplacian_geometry_ascending(pmg_laplacian op, double* G_out, hipStream_t s);
struct LaplacianInputs
{
  int degree;
  int32_t ncells;
  const int32_t* dofmap; // device
  const int8_t* bc;      // device
  const double* kappa;   // device
};
LaplacianInputs laplacian_inputs(pmg_laplacian op);
// interpolate.hip -- the p-transfers of the V-cycle
int interp_prolong(pmg_interpolator ip, double* coarse, double* fine, hipStream_t s);
int interp_restrict(pmg_interpolator ip, double* fine, double* coarse, hipStream_t s);
int interp_prolong_add(pmg_interpolator ip, double* coarse, double* fine, hipStream_t s);
bool interp_is_patched(pmg_interpolator ip);
bool interp_restricts_difference(pmg_interpolator ip);
int interp_restrict_difference(pmg_interpolator ip, double* fine, const double* fine_sub, double* coarse,
                               hipStream_t s);
bool interp_fuses_residual(pmg_interpolator ip, pmg_laplacian op);
int interp_restrict_residual(pmg_interpolator ip, pmg_laplacian op, const double* z, const double* r, double* coarse,
                             hipStream_t s);
// amg.hip -- the coarse solver
int amg_solve(pmg_amg amg, double* x, const double* b, hipStream_t s);
pmg_layout amg_layout(pmg_amg amg);
long long amg_capture_state(pmg_amg amg);
// matrix.hip -- the assembled form of a level's operator
// (a distributed matrix refreshes the ghost entries of `in`; _ghosts_current trusts them: no exchange, one launch)
int matrix_apply(pmg_matrix M, double* in, double* out, hipStream_t s);
int matrix_apply_ghosts_current(pmg_matrix M, const double* in, double* out, hipStream_t s);
const double* matrix_diag_inv(pmg_matrix M);
pmg_layout matrix_layout(pmg_matrix M);

// ---- the FP32 V-cycle (pmg_multigrid_set_precision; single domain only) ----
// It runs the smoother loop, the vector passes and the patch-form transfer kernels of the FP64 cycle instantiated for
// float (solvers.hip, vector.hip, interpolate.hip); its own are the float stiffness apply (laplacian_f32.hip) and the
// conversions between the caller's FP64 vectors and the cycle's float ones (vector.hip).
int laplacian_f32_supported(pmg_laplacian op, const char* who); // PMG_OK, or the refusal (ghosts, batched geometry)
int laplacian_f32_prepare(pmg_laplacian op, hipStream_t s);      // float tensor and table on first use (allocates)
int laplacian_f32_reaction(pmg_laplacian op, hipStream_t s);     // bring the float copy of the reaction vector up to date (if the float tensor exists)
int laplacian_f32_refresh(pmg_laplacian op, hipStream_t s);      // recompute the float tensor in place (if it exists)
int laplacian_f32_diag(pmg_laplacian op, const float** d, hipStream_t s, bool* changed);
long long laplacian_diag_version(pmg_laplacian op);
int laplacian_apply_f32(pmg_laplacian op, const float* in, float* out, hipStream_t s);
int transfer_f32_prepare(pmg_interpolator ip, const float** M1); // the float table, built on first use (allocates)
int prolong_add_f32(pmg_interpolator ip, const float* M1, const float* coarse, float* fine, hipStream_t s);
int restrict_f32(pmg_interpolator ip, const float* M1, const float* fine, const float* fine_sub, float* coarse,
                 hipStream_t s);
void launch_to_f32(int n, const double* in, const double* sub, float* out, hipStream_t s); // out = in (- sub)
void launch_from_f32(int n, const float* in, double* out, bool add, hipStream_t s);        // out (+)= in
} // namespace pmg
