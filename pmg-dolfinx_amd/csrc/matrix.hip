// The assembled operator: the BC-treated stiffness matrix in CSR on the device, applied by SpMV.  Replaces
// acc::MatrixOperator(a, bcs) of src/csr.hpp:58-131,205-260 next to the matrix-free operator (laplacian.hip).
//
//   pattern (host, once)  dolfinx's create_sparsity_pattern: row i couples to every dof that shares a cell with i;
//                         columns sorted, int32.  Built from the operator's own (ascending) copy of the dofmap, so the
//                         caller's cell-local node order does not reach the matrix.  Dirichlet rows and columns stay in
//                         the pattern as explicit zeros (fem::assemble_matrix + set_diagonal, :84-86).
//   values (device)       matrix_values_kernel: the element matrix in closed form from the stored geometry tensor --
//                         never "the cell operator applied to N unit vectors".  Row-wise gather: a sub-wavefront per
//                         row walks the (cell, local node) incidences of the row in ascending cell order, its lanes
//                         take the cell's nodes j, and the sums build up in an LDS copy of the row that is stored once.
//                         No atomics, no zero-fill, the same bits on every assembly.
//   product (device)      matrix_product_kernel: one launch, a sub-wavefront per row, width from the mean row length.
//
// Several ranks (pmg_matrix_create_distributed): rows are the owned dofs, columns local indices with the ghosts behind
// the owned ones, so the ghost columns of a row come last and off_diag_offset[i] (src/csr.hpp:114-126) splits it.
// Every rank holds the ghost-cell layer, so its owned rows are complete locally and no matrix value travels.  The product
// follows src/csr.hpp:252-270: scatter begin, the diag part of all rows, scatter end, the off-diag part of the boundary
// rows (matrix_range_product_kernel), with the routing of the matrix-free operator's apply_impl.  The host pattern and
// the split are in matrix_pattern.hpp.
#include "amg_renew.hpp"
#include "laplacian.hpp"
#include "matrix_pattern.hpp"

#include <algorithm>
#include <climits>
#include <cmath>

using namespace pmg;

struct pmg_matrix_s
{
  pmg_laplacian op = nullptr; // source of G, kappa, the BC marker and the dofmap; must outlive the matrix
  pmg_layout layout = nullptr;
  int nd = 0, N = 0;
  int32_t n = 0;     // rows = size_local
  int32_t ncols = 0; // columns = size_local + num_ghosts
  long long nnz = 0;
  int32_t* rp = nullptr; // [n + 1]
  int32_t* ci = nullptr; // [nnz], sorted within a row
  double* v = nullptr;   // [nnz]
  double* dinv = nullptr; // [n] inverse diagonal, BC rows 1 (src/csr.hpp:100-110)
  // dof -> (cell, cell-local node) incidences, ascending cell order: the row-wise gather's work list
  int32_t* inc_off = nullptr;
  int32_t* inc_cell = nullptr;
  int32_t* inc_loc = nullptr;
  long long n_inc = 0;
  int cap = 0;  // longest row (the LDS copy of a row in the values kernel)
  int tpr = 16; // lanes per row of the product
  double* partials = nullptr; // [NORM_BLOCKS] of the Frobenius norm
  // the distributed form: does a product exchange the halo of its input (the layout has ghosts or a communicator)?
  bool exchanges = false;
  int32_t* od = nullptr;    // [n] off_diag_offset: the position of the row's first ghost column
  int32_t* brows = nullptr; // [n_brows] the rows with a ghost column, ascending
  int32_t n_brows = 0;
  int tpr_diag = 16, tpr_off = 4; // lanes per row of the two phases, each from its own mean range length
};

namespace
{
constexpr int NORM_BLOCKS = 256;
constexpr size_t LDS_LIMIT = 64 * 1024;

template <typename T>
int to_device(T** dst, const T* src, size_t count)
{
  PMG_HIP(hipMalloc(dst, sizeof(T) * std::max<size_t>(count, 1)));
  if (count)
    PMG_HIP(hipMemcpy(*dst, src, sizeof(T) * count, hipMemcpyHostToDevice));
  return PMG_OK;
}

// (row_position, the search of a column in a sorted row: amg_renew.hpp, shared with the AMG's renewal)

// Values of the rows [0, n) on the existing pattern, and the inverse diagonal.
// W lanes (a power of two <= 64, so a group never spans two wavefronts) share a row; blockDim.x / W rows per block.
// LDS: the 1-D derivative table D[q * ND + i] = l_i'(x_q), then one copy of `cap` doubles per row of the block.
// With i = (a,b,c) the row's node in the cell and j = (a2,b2,c2), G the six stored components at a point
// (Gc[cell][q][6]: G00 G01 G02 G11 G12 G22, q ascending):
//   Ae[i][j] = kappa * ( [b=b2][c=c2] sum_q D[q,a] D[q,a2] G00(q,b,c) + the two analogues
//                      + [c=c2] ( D[a2,a] D[b,b2] G01(a2,b,c) + D[a,a2] D[b2,b] G01(a,b2,c) ) + the G02, G12 analogues )
// (oracle/pmg_oracle.py Laplacian.diagonal is the i = j case); j that shares no index with i gives an explicit zero.
// Lanes of a group hold different j of ONE cell, i.e. different columns, so the LDS updates of a cell never collide;
// cells follow each other in program order of the one wavefront, whose LDS operations retire in order.
template <int ND>
__global__ void __launch_bounds__(256)
    matrix_values_kernel(int n, int W, int cap, const int32_t* __restrict__ rp, const int32_t* __restrict__ ci,
                         double* __restrict__ vals, double* __restrict__ dinv, const int32_t* __restrict__ inc_off,
                         const int32_t* __restrict__ inc_cell, const int32_t* __restrict__ inc_loc,
                         const int32_t* __restrict__ dofmap, const double* __restrict__ Gc,
                         const double* __restrict__ kappa, const int8_t* __restrict__ bc, const double* __restrict__ Dg,
                         const double* __restrict__ react)
{
  constexpr int NSQ = ND * ND, N = NSQ * ND;
  extern __shared__ double lds[];
  double* D = lds;
  for (int i = threadIdx.x; i < NSQ; i += blockDim.x)
    D[i] = Dg[i];
  __syncthreads();
  const int groups = blockDim.x / W;
  const int g = threadIdx.x / W, sub = threadIdx.x - g * W;
  const int row = blockIdx.x * groups + g;
  if (row >= n)
    return;
  double* acc = lds + NSQ + (size_t)g * cap;
  const int rs = rp[row], len = rp[row + 1] - rs;
  const int32_t* cols = ci + rs;
  for (int k = sub; k < len; k += W)
    acc[k] = 0.0;
  const int dpos = row_position(cols, len, row);
  if (bc[row]) // set_diagonal(1.0), src/csr.hpp:86; the rest of the row stays zero
  {
    if (sub == 0)
      acc[dpos] = 1.0;
  }
  else
  {
    for (int m = inc_off[row]; m < inc_off[row + 1]; ++m)
    {
      const int cell = inc_cell[m], t = inc_loc[m];
      const int a = t / NSQ, b = (t / ND) % ND, c = t % ND;
      const double kap = kappa[cell];
      const double* G = Gc + (size_t)cell * N * 6;
      const int32_t* dm = dofmap + (size_t)cell * N;
      for (int j = sub; j < N; j += W)
      {
        const int a2 = j / NSQ, b2 = (j / ND) % ND, c2 = j % ND;
        const bool ea = a2 == a, eb = b2 == b, ec = c2 == c;
        if (!(ea || eb || ec))
          continue;
        const int32_t col = dm[j];
        if (bc[col]) // Dirichlet column: dropped, the entry stays an explicit zero
          continue;
        double s = 0.0;
        if (eb && ec)
          for (int q = 0; q < ND; ++q)
            s += D[q * ND + a] * D[q * ND + a2] * G[((q * ND + b) * ND + c) * 6 + 0];
        if (ea && ec)
          for (int q = 0; q < ND; ++q)
            s += D[q * ND + b] * D[q * ND + b2] * G[((a * ND + q) * ND + c) * 6 + 3];
        if (ea && eb)
          for (int q = 0; q < ND; ++q)
            s += D[q * ND + c] * D[q * ND + c2] * G[((a * ND + b) * ND + q) * 6 + 5];
        if (ec)
          s += D[a2 * ND + a] * D[b * ND + b2] * G[((a2 * ND + b) * ND + c) * 6 + 1]
               + D[a * ND + a2] * D[b2 * ND + b] * G[((a * ND + b2) * ND + c) * 6 + 1];
        if (eb)
          s += D[a2 * ND + a] * D[c * ND + c2] * G[((a2 * ND + b) * ND + c) * 6 + 2]
               + D[a * ND + a2] * D[c2 * ND + c] * G[((a * ND + b) * ND + c2) * 6 + 2];
        if (ea)
          s += D[b2 * ND + b] * D[c * ND + c2] * G[((a * ND + b2) * ND + c) * 6 + 4]
               + D[b * ND + b2] * D[c2 * ND + c] * G[((a * ND + b) * ND + c2) * 6 + 4];
        acc[row_position(cols, len, col)] += kap * s;
      }
      __builtin_amdgcn_wave_barrier(); // the next cell's updates stay behind this cell's
    }
    // the diagonal term of the operator (pmg_laplacian_set_reaction, pmg_laplacian_set_robin: their summed vector):
    // unmarked rows only
    if (react && sub == 0)
      acc[dpos] += react[row];
  }
  __builtin_amdgcn_wave_barrier();
  for (int k = sub; k < len; k += W)
    vals[rs + k] = acc[k];
  if (sub == 0)
  {
    const double d = acc[dpos];
    dinv[row] = d != 0.0 ? 1.0 / d : 0.0;
  }
}

// y = A x: TPR lanes of a wavefront share a row (the form of amg.hip's csr_product_kernel, up to a whole wavefront)
template <int TPR>
__global__ void __launch_bounds__(256)
    matrix_product_kernel(int n, const int32_t* __restrict__ rp, const int32_t* __restrict__ ci,
                          const double* __restrict__ v, const double* __restrict__ x, double* __restrict__ y)
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
    y[row] = acc;
}

// The range form of the product, the two phases of a distributed product (src/csr.hpp:252-270): TPR lanes share a row
// and walk the columns [first[row], last[row]) only.
//   LISTED = false  the diag phase: every row i < count over [rp[i], od[i]); y[i] is STORED (an empty range stores 0)
//   LISTED = true   the off-diag phase: the rows rows[i], i < count, over [od[r], rp[r + 1]); the sum is ADDED to y[r]
// One group writes a row per phase and the phases are stream-ordered: no atomics.
template <int TPR, bool LISTED>
__global__ void __launch_bounds__(256)
    matrix_range_product_kernel(int count, const int32_t* __restrict__ rows, const int32_t* __restrict__ first,
                                const int32_t* __restrict__ last, const int32_t* __restrict__ ci,
                                const double* __restrict__ v, const double* __restrict__ x, double* __restrict__ y)
{
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = gid / TPR, sub = gid % TPR;
  double acc = 0.0;
  int row = 0;
  if (i < count)
  {
    row = LISTED ? rows[i] : i;
    const int e = last[row];
    for (int k = first[row] + sub; k < e; k += TPR)
      acc += v[k] * x[ci[k]];
  }
#pragma unroll
  for (int off = TPR / 2; off > 0; off >>= 1)
    acc += __shfl_down(acc, off, TPR);
  if (i < count && sub == 0)
  {
    if (LISTED)
      y[row] += acc;
    else
      y[row] = acc;
  }
}

// block partials of sum v^2, each block over a fixed contiguous share: the same bits on every call
__global__ void __launch_bounds__(256)
    matrix_square_sum_kernel(long long nnz, const double* __restrict__ v, double* __restrict__ partials)
{
  __shared__ double red[256];
  const long long per = (nnz + gridDim.x - 1) / gridDim.x;
  const long long first = per * blockIdx.x, last = first + per < nnz ? first + per : nnz;
  double acc = 0.0;
  for (long long k = first + threadIdx.x; k < last; k += blockDim.x)
    acc += v[k] * v[k];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1)
  {
    if ((int)threadIdx.x < off)
      red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0)
    partials[blockIdx.x] = red[0];
}

template <int ND>
void launch_values(pmg_matrix M, int W, int groups, size_t lds, const double* Gc, hipStream_t s)
{
  const pmg_laplacian op = M->op;
  matrix_values_kernel<ND><<<(M->n + groups - 1) / groups, W * groups, lds, s>>>(
      M->n, W, M->cap, M->rp, M->ci, M->v, M->dinv, M->inc_off, M->inc_cell, M->inc_loc, op->dofmap, Gc, op->kappa,
      op->bc, op->D, laplacian_reaction(op));
}

// one phase of the distributed product: the diag part of all rows (stored), or the off-diag part of the boundary rows
// (added); a rank without boundary rows launches nothing in the second
int launch_range(pmg_matrix M, bool off_diag, const double* in, double* out, hipStream_t s)
{
  const int count = off_diag ? M->n_brows : M->n;
  if (count == 0)
    return PMG_OK;
  const int tpr = off_diag ? M->tpr_off : M->tpr_diag;
  const unsigned blocks = (unsigned)(((long long)count * tpr + 255) / 256);
#define PMG_RANGE_(T)                                                                                                  \
  case T:                                                                                                              \
    if (off_diag)                                                                                                      \
      matrix_range_product_kernel<T, true><<<blocks, 256, 0, s>>>(count, M->brows, M->od, M->rp + 1, M->ci, M->v, in,  \
                                                                  out);                                                \
    else                                                                                                               \
      matrix_range_product_kernel<T, false><<<blocks, 256, 0, s>>>(count, nullptr, M->rp, M->od, M->ci, M->v, in,      \
                                                                   out);                                               \
    break;
  switch (tpr)
  {
    PMG_RANGE_(4)
    PMG_RANGE_(8)
    PMG_RANGE_(16)
    PMG_RANGE_(32)
  default:
    PMG_RANGE_(64)
  }
#undef PMG_RANGE_
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}

// does a vector of this layout have a halo to exchange?
bool layout_is_distributed(pmg_layout l) { return l->num_ghosts > 0 || l->multi_rank() || l->win || l->exchange; }

// pmg_matrix_create_from_laplacian keeps its contract: one domain (pmg_matrix_create_distributed takes any layout)
int check_single_domain(pmg_laplacian op, const char* who)
{
  PMG_REQUIRE(!layout_is_distributed(op->layout),
              "%s: the assembled operator is single-domain only (the layout has ghosts or a communicator); the "
              "distributed form with its diag / off-diag split is a follow-up",
              who);
  return PMG_OK;
}

int check_source(pmg_laplacian op, const char* who)
{
  PMG_REQUIRE(op->batch_patches == 0,
              "%s: the operator is in batched-geometry mode, its tensor G is not resident "
              "(pmg_laplacian_set_geometry_batch(op, 0) keeps it)",
              who);
  return PMG_OK;
}

int assemble_values(pmg_matrix M, hipStream_t s)
{
  pmg_laplacian op = M->op;
  PMG_TRY(check_source(op, "pmg_matrix_update_values"));
  if (M->n == 0)
    return PMG_OK;
  // the stored tensor as [cell][q][6]: one pass over G, held for the assembly only
  double* Gc = nullptr;
  PMG_HIP(hipMalloc(&Gc, sizeof(double) * 6 * std::max<size_t>((size_t)op->ncells * M->N, 1)));
  int rc = laplacian_geometry_ascending(op, Gc, s);
  if (rc == PMG_OK)
  {
    const int W = M->N <= 8 ? 8 : M->N <= 32 ? 32 : 64;
    const size_t table = sizeof(double) * M->nd * M->nd, rowb = sizeof(double) * (size_t)M->cap;
    const int groups = (int)std::max<size_t>(1, std::min<size_t>(256 / W, (LDS_LIMIT - table) / rowb));
    const size_t lds = table + rowb * groups;
    rc = with_degree(M->nd - 1, [&](auto P) {
      launch_values<decltype(P)::value + 1>(M, W, groups, lds, Gc, s);
      return PMG_OK;
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
      rc = fail(PMG_ERR_HIP, "matrix_values_kernel: %s", hipGetErrorString(e));
  }
  const hipError_t es = hipStreamSynchronize(s); // Gc is released below
  (void)hipFree(Gc);
  if (rc == PMG_OK && es != hipSuccess)
    return fail(PMG_ERR_HIP, "pmg_matrix_update_values: %s", hipGetErrorString(es));
  return rc;
}
} // namespace

namespace pmg
{
// used by solvers.hip
// out = A in over whole rows, one launch: a single domain, or the ghost entries of `in` are current
int matrix_apply_ghosts_current(pmg_matrix M, const double* in, double* out, hipStream_t s)
{
  if (M->n == 0)
    return PMG_OK;
  const long long threads = (long long)M->n * M->tpr;
  const unsigned blocks = (unsigned)((threads + 255) / 256);
  switch (M->tpr)
  {
  case 4: matrix_product_kernel<4><<<blocks, 256, 0, s>>>(M->n, M->rp, M->ci, M->v, in, out); break;
  case 8: matrix_product_kernel<8><<<blocks, 256, 0, s>>>(M->n, M->rp, M->ci, M->v, in, out); break;
  case 16: matrix_product_kernel<16><<<blocks, 256, 0, s>>>(M->n, M->rp, M->ci, M->v, in, out); break;
  case 32: matrix_product_kernel<32><<<blocks, 256, 0, s>>>(M->n, M->rp, M->ci, M->v, in, out); break;
  default: matrix_product_kernel<64><<<blocks, 256, 0, s>>>(M->n, M->rp, M->ci, M->v, in, out); break;
  }
  PMG_HIP(hipGetLastError());
  return PMG_OK;
}

// operator()(x, y), src/csr.hpp:252-270, with the routing of the matrix-free operator's apply_impl (laplacian.hip).  On
// a distributed matrix the ghost entries of `in` are refreshed and those of `out` are not touched.
int matrix_apply(pmg_matrix M, double* in, double* out, hipStream_t s)
{
  if (!M->exchanges)
    return matrix_apply_ghosts_current(M, in, out, s);
  pmg_layout l = M->layout;
  // a small level on halo windows (the operator's own rule): the exchange whole, in one launch, then whole rows
  if (laplacian_single_launch(M->op))
  {
    PMG_TRY(scatter_fwd_whole(l, in, s));
    return matrix_apply_ghosts_current(M, in, out, s);
  }
  PMG_TRY(pmg_scatter_fwd_begin(l, in, (pmg_stream)s)); // :254
  PMG_TRY(launch_range(M, false, in, out, s));          // :256-261 the owned columns of every row
  PMG_TRY(pmg_scatter_fwd_end(l, in, (pmg_stream)s));   // :263
  PMG_TRY(launch_range(M, true, in, out, s));           // :265-269 the ghost columns of the boundary rows
  return PMG_OK;
}
const double* matrix_diag_inv(pmg_matrix M) { return M->dinv; }
pmg_layout matrix_layout(pmg_matrix M) { return M->layout; }
pmg_laplacian matrix_source(pmg_matrix M) { return M->op; }
} // namespace pmg

namespace
{
// MatrixOperator(a, bcs), src/csr.hpp:66-131: the body of both constructors, in `who`'s name
int matrix_create(pmg_matrix* out, pmg_laplacian op, hipStream_t s, const char* who)
{
  PMG_TRY(check_source(op, who));
  auto* M = new pmg_matrix_s;
  HandleGuard<pmg_matrix> guard(M, pmg_matrix_destroy);
  M->op = op;
  M->layout = op->layout;
  M->nd = op->nd;
  M->N = op->N;
  M->n = op->layout->size_local;
  M->ncols = op->layout->total();
  M->exchanges = layout_is_distributed(op->layout);
  const int N = M->N;
  // the operator's own dofmap (ascending node order) and the cells it applies
  std::vector<int32_t> h_dofmap((size_t)op->ncells * N);
  if (!h_dofmap.empty())
    PMG_HIP(hipMemcpyAsync(h_dofmap.data(), op->dofmap, sizeof(int32_t) * h_dofmap.size(), hipMemcpyDeviceToHost, s));
  PMG_HIP(hipStreamSynchronize(s));
  std::vector<int32_t> cells;
  for (int32_t c : op->pcell_h)
    if (c >= 0)
      cells.push_back(c);
  std::sort(cells.begin(), cells.end());
  for (int32_t c : cells)
    for (int t = 0; t < N; ++t)
    {
      const int32_t d = h_dofmap[(size_t)c * N + t];
      PMG_REQUIRE(d >= 0 && d < M->ncols, "%s: dofmap entry %d out of range", who, d);
    }
  std::vector<int32_t> inc_off, inc_cell, inc_loc, rp, ci, od, brows;
  const long long nnz =
      matrix_pattern(M->n, M->ncols, N, cells, h_dofmap.data(), inc_off, inc_cell, inc_loc, rp, ci, &M->cap);
  PMG_REQUIRE(nnz <= INT32_MAX, "%s: the pattern has %lld non-zeros, more than int32 indices hold", who, nnz);
  PMG_REQUIRE(sizeof(double) * ((size_t)M->cap + M->nd * M->nd) <= LDS_LIMIT,
              "%s: a row of %d entries exceeds the %zu the assembly holds in LDS", who, M->cap,
              LDS_LIMIT / sizeof(double) - M->nd * M->nd);
  M->nnz = nnz;
  M->n_inc = (long long)inc_cell.size();
  M->tpr = matrix_lanes_per_row(M->n ? (double)nnz / M->n : 1.0);
  // the split: each phase of the product takes its lanes from its own mean range length
  matrix_split(M->n, rp, ci, od, brows);
  M->n_brows = (int32_t)brows.size();
  long long n_off = 0;
  for (int32_t r : brows)
    n_off += rp[r + 1] - od[r];
  M->tpr_diag = matrix_lanes_per_row(M->n ? (double)(nnz - n_off) / M->n : 1.0);
  M->tpr_off = matrix_lanes_per_row(M->n_brows ? (double)n_off / M->n_brows : 1.0);
  PMG_TRY(to_device(&M->rp, rp.data(), rp.size()));
  PMG_TRY(to_device(&M->ci, ci.data(), ci.size()));
  PMG_TRY(to_device(&M->od, od.data(), od.size()));
  PMG_TRY(to_device(&M->brows, brows.data(), brows.size()));
  PMG_TRY(to_device(&M->inc_off, inc_off.data(), inc_off.size()));
  PMG_TRY(to_device(&M->inc_cell, inc_cell.data(), inc_cell.size()));
  PMG_TRY(to_device(&M->inc_loc, inc_loc.data(), inc_loc.size()));
  PMG_HIP(hipMalloc(&M->v, sizeof(double) * std::max<size_t>((size_t)nnz, 1)));
  PMG_HIP(hipMalloc(&M->dinv, sizeof(double) * std::max<size_t>((size_t)M->n, 1)));
  PMG_HIP(hipMalloc(&M->partials, sizeof(double) * NORM_BLOCKS));
  PMG_TRY(assemble_values(M, s));
  *out = guard.release();
  return PMG_OK;
}
} // namespace

// MatrixOperator(a, bcs) on one domain
extern "C" int pmg_matrix_create_from_laplacian(pmg_matrix* out, pmg_laplacian op, pmg_stream stream)
{
  PMG_REQUIRE(out && op, "pmg_matrix_create_from_laplacian: NULL argument");
  *out = nullptr;
  PMG_TRY(check_single_domain(op, "pmg_matrix_create_from_laplacian"));
  return matrix_create(out, op, S(stream), "pmg_matrix_create_from_laplacian");
}

// ... and on any layout: rows = the owned dofs, columns = owned and ghost dofs, split per row
extern "C" int pmg_matrix_create_distributed(pmg_matrix* out, pmg_laplacian op, pmg_stream stream)
{
  PMG_REQUIRE(out && op, "pmg_matrix_create_distributed: NULL argument");
  *out = nullptr;
  return matrix_create(out, op, S(stream), "pmg_matrix_create_distributed");
}

extern "C" int pmg_matrix_destroy(pmg_matrix M)
{
  if (!M)
    return PMG_OK;
  (void)hipFree(M->rp);
  (void)hipFree(M->ci);
  (void)hipFree(M->od);
  (void)hipFree(M->brows);
  (void)hipFree(M->v);
  (void)hipFree(M->dinv);
  (void)hipFree(M->inc_off);
  (void)hipFree(M->inc_cell);
  (void)hipFree(M->inc_loc);
  (void)hipFree(M->partials);
  delete M;
  return PMG_OK;
}

extern "C" int pmg_matrix_update_values(pmg_matrix M, pmg_stream stream)
{
  PMG_REQUIRE(M, "pmg_matrix_update_values: NULL argument");
  return assemble_values(M, S(stream));
}

// operator()(x, y), src/csr.hpp:220-260 (no transpose: the operator is symmetric).  The signature is the single-domain
// one; a distributed matrix writes the ghost entries of `in`, as the reference's operator does through its scatter.
extern "C" int pmg_matrix_apply(pmg_matrix M, const double* in, double* out, pmg_stream stream)
{
  PMG_REQUIRE(M && in && out, "pmg_matrix_apply: NULL argument");
  PMG_REQUIRE(in != out, "pmg_matrix_apply: in and out alias");
  return matrix_apply(M, const_cast<double*>(in), out, S(stream));
}

extern "C" int pmg_matrix_apply_ghosts_current(pmg_matrix M, const double* in, double* out, pmg_stream stream)
{
  PMG_REQUIRE(M && in && out, "pmg_matrix_apply_ghosts_current: NULL argument");
  PMG_REQUIRE(in != out, "pmg_matrix_apply_ghosts_current: in and out alias");
  return matrix_apply_ghosts_current(M, in, out, S(stream));
}

// get_diag_inverse, src/csr.hpp:205-209
extern "C" int pmg_matrix_get_diag_inverse(pmg_matrix M, double* diag_inv, pmg_stream stream)
{
  PMG_REQUIRE(M && diag_inv, "pmg_matrix_get_diag_inverse: NULL argument");
  if (M->n > 0)
    PMG_HIP(hipMemcpyAsync(diag_inv, M->dinv, sizeof(double) * M->n, hipMemcpyDeviceToDevice, S(stream)));
  return PMG_OK;
}

extern "C" long long pmg_matrix_rows(pmg_matrix M) { return M ? (long long)M->n : -1; }

extern "C" long long pmg_matrix_cols(pmg_matrix M) { return M ? (long long)M->ncols : -1; }

extern "C" long long pmg_matrix_nnz(pmg_matrix M) { return M ? M->nnz : -1; }

// device bytes held: row pointers, columns, values, inverse diagonal, the incidence lists of update_values and the
// split (off_diag_offset, boundary rows)
extern "C" long long pmg_matrix_bytes(pmg_matrix M)
{
  if (!M)
    return -1;
  return (long long)sizeof(int32_t) * 2 * ((long long)M->n + 1) + (long long)(sizeof(int32_t) + sizeof(double)) * M->nnz
         + (long long)sizeof(double) * M->n + 2LL * sizeof(int32_t) * M->n_inc
         + (long long)sizeof(int32_t) * ((long long)M->n + M->n_brows);
}

// the "A norm" of src/csr.hpp:95-99
extern "C" int pmg_matrix_frobenius_norm(pmg_matrix M, double* norm)
{
  PMG_REQUIRE(M && norm, "pmg_matrix_frobenius_norm: NULL argument");
  double sum = 0.0;
  if (M->nnz > 0)
  {
    matrix_square_sum_kernel<<<NORM_BLOCKS, 256, 0, nullptr>>>(M->nnz, M->v, M->partials);
    PMG_HIP(hipGetLastError());
    double h[NORM_BLOCKS];
    PMG_HIP(hipMemcpy(h, M->partials, sizeof(h), hipMemcpyDeviceToHost));
    for (double p : h)
      sum += p;
  }
  // several ranks: every owned row lives on exactly one rank, so the global norm is the all-reduced sum of squares
  // (collective; result slot 7, no solver's)
  if (pmg_layout l = M->layout; l->multi_rank())
  {
    PMG_HIP(hipMemcpy(red_slot(l, 7), &sum, sizeof(double), hipMemcpyHostToDevice));
    PMG_TRY(reduce_slots_async(l, 7, 1, false, nullptr));
    PMG_TRY(fetch_slots(l, 7, 1, &sum, nullptr));
  }
  *norm = std::sqrt(sum);
  return PMG_OK;
}

// the split of the rows: off_diag_offset[rows] and the boundary-row list; NULL arrays: sizes only
extern "C" int pmg_matrix_export_split(pmg_matrix M, int32_t* off_diag_offset, long long* n_boundary_rows,
                                       int32_t* boundary_rows)
{
  PMG_REQUIRE(M, "pmg_matrix_export_split: NULL argument");
  if (n_boundary_rows)
    *n_boundary_rows = M->n_brows;
  PMG_HIP(hipDeviceSynchronize());
  if (off_diag_offset && M->n)
    PMG_HIP(hipMemcpy(off_diag_offset, M->od, sizeof(int32_t) * (size_t)M->n, hipMemcpyDeviceToHost));
  if (boundary_rows && M->n_brows)
    PMG_HIP(hipMemcpy(boundary_rows, M->brows, sizeof(int32_t) * (size_t)M->n_brows, hipMemcpyDeviceToHost));
  return PMG_OK;
}

extern "C" int pmg_matrix_export(pmg_matrix M, long long* rows, long long* nnz, int32_t* row_ptr, int32_t* cols,
                                 double* values)
{
  PMG_REQUIRE(M, "pmg_matrix_export: NULL argument");
  if (rows)
    *rows = M->n;
  if (nnz)
    *nnz = M->nnz;
  PMG_HIP(hipDeviceSynchronize());
  if (row_ptr)
    PMG_HIP(hipMemcpy(row_ptr, M->rp, sizeof(int32_t) * ((size_t)M->n + 1), hipMemcpyDeviceToHost));
  if (cols && M->nnz)
    PMG_HIP(hipMemcpy(cols, M->ci, sizeof(int32_t) * (size_t)M->nnz, hipMemcpyDeviceToHost));
  if (values && M->nnz)
    PMG_HIP(hipMemcpy(values, M->v, sizeof(double) * (size_t)M->nnz, hipMemcpyDeviceToHost));
  return PMG_OK;
}
