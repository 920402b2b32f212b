/* pmg_amd.h -- C ABI of the MI355X-native matrix-free p-multigrid hot path.
 *
 * One shared library (pmg-dolfinx_amd/lib/libpmg_amd.so, built for gfx950 by
 * __graft_entry__.build()).  Plain pointers and sizes only; every device
 * pointer is caller-owned unless stated otherwise and must stay valid for the
 * lifetime of the handle that was given it (the reference's objects hold
 * non-owning std::span's of device memory in exactly the same way,
 * src/laplacian.hpp:500-509).  All functions return 0 on success and a
 * negative code on failure; pmg_last_error() returns the message of the last
 * failure on the calling thread (the reference throws std::runtime_error for
 * the same conditions -- src/laplacian.hpp:346,479, src/vector.hpp:343,
 * src/cg.hpp:125,138 -- and print+exit(1)s on HIP errors, src/util.hpp:10-18).
 * Nothing here is thread safe; one host thread per GPU, like the reference.
 *
 * The reference's interface for this path is header-only C++ duck typing over
 * dolfinx types; each entry point below names the reference
 * member it replaces.  dolfinx's IndexMap/Scatterer inputs are flattened to
 * arrays.  INTEGRATION.md shows the thin C++ adapter a maintainer would add on
 * the reference side.
 *
 * All citations are relative to Wells-Group/pmg-dolfinx @ 2024_08_07.
 */
#ifndef PMG_AMD_H
#define PMG_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMG_OK 0
#define PMG_ERR_INVALID -1   /* bad argument / unsupported degree / size mismatch */
#define PMG_ERR_HIP -2       /* a HIP runtime call failed */
#define PMG_ERR_NUMERIC -3   /* e.g. TQLI did not converge */
#define PMG_MAX_DEGREE 8

typedef void* pmg_stream; /* hipStream_t (0 = default stream) */

typedef struct pmg_layout_s* pmg_layout;
typedef struct pmg_comm_s* pmg_comm;
typedef struct pmg_laplacian_s* pmg_laplacian;
typedef struct pmg_chebyshev_s* pmg_chebyshev;
typedef struct pmg_cg_s* pmg_cg;
typedef struct pmg_interpolator_s* pmg_interpolator;
typedef struct pmg_multigrid_s* pmg_multigrid;
typedef struct pmg_amg_s* pmg_amg;
typedef struct pmg_matrix_s* pmg_matrix;

const char* pmg_last_error(void);
int pmg_version(void);

/* ---- host-side tables (no GPU needed) ------------------------------------
 * What the reference gets from basix at construction time.
 * pmg_gll_table: n-point Gauss-Lobatto-Legendre rule on [0,1]
 *   (basix make_quadrature(gll, interval), src/laplacian.hpp:307-309).
 * pmg_lagrange_derivative_table: D[q*n+i] = l_i'(x_q) on the GLL nodes
 *   (second half of element1D.tabulate(1,...), src/laplacian.hpp:312-317).
 * pmg_interpolation_table: M[j*(pc+1)+k] = l^coarse_k(x^fine_j)
 *   (1-D factor of basix::compute_interpolation_operator, src/interpolate.hpp:118).
 * pmg_tqli: eigenvalues of a symmetric tridiagonal matrix, in place on d
 *   (tqli(), src/cg.hpp:55-84). */
int pmg_gll_table(int n, double* points, double* weights);
int pmg_lagrange_derivative_table(int n, double* D);
int pmg_interpolation_table(int p_coarse, int p_fine, double* M);
int pmg_tqli(double* d, double* e, int n);

/* ---- cell-local node order --------------------------------------------------
 * The reference takes its dofmaps from a basix tensor-product element
 * (basix::create_tp_element, examples/pmg/main.cpp:83-87) and its 1-D tables and quadrature
 * points from basix as well (src/laplacian.hpp:302-317, src/interpolate.hpp:118): the
 * cell-local index is t = ja*nd^2 + jb*nd + jc in both, but the 1-D index j runs over the
 * nodes in BASIX order -- vertex 0, vertex 1, then the interior nodes from left to right
 * ("endpoints first"; that the dofs and the GLL points share this order is why "phi is the
 * identity" in src/laplacian.hpp:200-202).  The kernels of this library index nodes by
 * ASCENDING coordinate.  Every entry point that receives or returns an array indexed by a
 * cell-local node or quadrature-point number therefore has an `_ordered` form that takes
 * the caller's order; the library applies it ONCE, at construction, where the caller's
 * arrays are turned into its own (a permuted copy of the dofmap: 4 N bytes per cell, held
 * by the handle), so the kernels and everything behind them are unaffected.
 *
 *   PMG_NODES_ASCENDING       j = position by coordinate (the plain entry points)
 *   PMG_NODES_ENDPOINTS_FIRST basix: j = 0 -> x = 0, j = 1 -> x = 1, j >= 2 -> interior node j - 1
 *   PMG_NODES_CUSTOM          perm1d[j] = ascending position of the caller's 1-D node j, j < degree + 1
 *
 * Arrays affected: dofmap (operator, interpolator), dphi_geometry [3][nq][8] and G_weights [nq]
 * when the caller supplies them, the geometry tensor returned by pmg_laplacian_get_geometry
 * ([ncells][nq][6], q in the operator's node order).  NOT affected: vectors and everything indexed by
 * a (global or local) dof number -- bc_marker, f and b of pmg_laplacian_assemble_rhs, diag_inv --,
 * the vertex order of geom_dofmap (two nodes per direction: both orders coincide), cell lists.
 * pmg_node_permutation writes perm1d[degree + 1] for any of the three orders (custom: validated copy).
 * The *_ordered table functions return what basix would: points / weights / D rows and columns /
 * M rows (fine) and columns (coarse) in the given order. */
#define PMG_NODES_ASCENDING 0
#define PMG_NODES_ENDPOINTS_FIRST 1
#define PMG_NODES_CUSTOM 2
int pmg_node_permutation(int node_order, int degree, const int32_t* custom_perm1d, int32_t* perm1d);
int pmg_gll_table_ordered(int n, int node_order, const int32_t* custom_perm1d, double* points, double* weights);
int pmg_lagrange_derivative_table_ordered(int n, int node_order, const int32_t* custom_perm1d, double* D);
int pmg_interpolation_table_ordered(int p_coarse, int p_fine, int node_order, const int32_t* custom_coarse,
                                    const int32_t* custom_fine, double* M);

/* ---- distributed vector layout -------------------------------------------
 * Replaces the data members of acc::Vector (src/vector.hpp:83-96,304-324): a
 * vector is a caller-owned device array of size_local + num_ghosts doubles
 * (block size 1), described by a layout.  send_indices (owned positions packed
 * for the neighbours, == Scatterer::local_indices()) and recv_indices (ghost
 * positions, relative to size_local, == Scatterer::remote_indices()) are device
 * arrays; send_buffer / recv_buffer are caller-owned device staging buffers of
 * n_send / n_recv doubles.
 *
 * The exchange itself is the caller's (the reference delegates it to
 * dolfinx::common::Scatterer over MPI, src/vector.hpp:203-206,215): `exchange`
 * is called with phase 0 after the pack kernel has been enqueued on `stream`
 * (start moving send_buffer -> the neighbours' recv_buffer, asynchronously with
 * respect to `stream`), and with phase 1 before the unpack kernel is enqueued
 * (make `stream` wait for the arrival).  Phases 2 / 3 are the same for the
 * reverse scatter (recv_buffer -> the owners' send_buffer).  It must return 0.  If `exchange`
 * is non-NULL it is called on every scatter, also when n_send == n_recv == 0 (the
 * caller's exchange is typically a collective); pass NULL on a single rank.
 *
 * `allreduce_sum` sums `n` host doubles over all ranks in place (the
 * reference's MPI_Allreduce, src/vector.hpp:350); NULL on a single rank. */
typedef int (*pmg_exchange_fn)(void* user, int phase, pmg_stream stream);
typedef int (*pmg_allreduce_fn)(void* user, double* values, int n);

int pmg_layout_create(pmg_layout* out, int32_t size_local, int32_t num_ghosts, int32_t n_send,
                      const int32_t* send_indices, double* send_buffer, int32_t n_recv,
                      const int32_t* recv_indices, double* recv_buffer, pmg_exchange_fn exchange,
                      pmg_allreduce_fn allreduce_sum, void* user);
int pmg_layout_destroy(pmg_layout l);
int32_t pmg_layout_size_local(pmg_layout l);
int32_t pmg_layout_num_ghosts(pmg_layout l);
/* Optional: the maximum over all ranks of n host doubles, in place (the reference's
 * MPI_Allreduce(MPI_MAX) of norm(linf), src/vector.hpp:383-385); `user` is the pointer given
 * to pmg_layout_create.  Without it pmg_vec_norm(linf) fails on a layout that has an
 * allreduce_sum callback (several ranks), because a sum cannot stand in for a maximum. */
int pmg_layout_set_allreduce_max(pmg_layout l, pmg_allreduce_fn allreduce_max);

/* ---- native communicator: RCCL over xGMI, issued by the library -------------
 * The alternative to the two callbacks above for one-process-per-GPU runs on one node: the
 * library itself posts the neighbour exchange (one group of ncclSend/ncclRecv per scatter, on
 * the communicator's own stream, ordered against the compute stream with events -- no host
 * synchronisation, no callback) and sums the scalars of the reductions with ncclAllReduce on
 * device memory.  This is the role of dolfinx's Scatterer + MPI in the reference
 * (src/vector.hpp:94,203-206,215,350).  RCCL is bound at run time (librccl.so.1).
 *
 *   pmg_comm_unique_id : rank 0 obtains the 128-byte id (ncclGetUniqueId) and hands it to the
 *                        other ranks by whatever means the caller has (a file, MPI_Bcast,
 *                        torch.distributed.broadcast ...);
 *   pmg_comm_create    : collective over all ranks (ncclCommInitRank) on the current device;
 *   pmg_layout_set_comm: attaches the communicator and the neighbour list of the halo plan --
 *                        neighbour i receives send_buffer[sum(send_counts[:i]) ...) and fills
 *                        recv_buffer[sum(recv_counts[:i]) ...), i.e. the index lists given to
 *                        pmg_layout_create are grouped by neighbour in this order.  Every rank
 *                        of the communicator must call every scatter / reduction of a layout
 *                        in the same order (they are collectives), also a rank with no
 *                        neighbours.  The communicator must outlive the layout. */
#define PMG_COMM_ID_BYTES 128
int pmg_comm_unique_id(char* id /* [PMG_COMM_ID_BYTES] */);
int pmg_comm_create(pmg_comm* out, int rank, int nranks, const char* id);
int pmg_comm_destroy(pmg_comm comm);
/* 1 if a halo exchange captured into a hipGraph keeps its overlap with the interior cells (the communicator's stream is
 * forked into the capture), 0 if this process's HIP runtime cannot end such a capture (7.0.x: unbounded recursion in
 * hipStreamEndCapture) and the captured exchange is issued on the capturing stream instead. */
int pmg_comm_capture_overlaps(void);
/* Set-up helper, blocking (where the reference's set-up calls MPI_Allgather): `bytes` bytes of host memory from every
 * rank, in rank order, into recv[size * bytes] on every rank. */
int pmg_comm_allgather(pmg_comm comm, const void* send, size_t bytes, void* recv);
/* values[0 .. n) (device memory) summed over the ranks in place, ordered on `stream` (MPI_Allreduce(MPI_IN_PLACE, SUM)). */
int pmg_comm_allreduce_sum(pmg_comm comm, double* values, int n, pmg_stream stream);
int pmg_comm_rank(pmg_comm comm);
int pmg_comm_size(pmg_comm comm);
int pmg_layout_set_comm(pmg_layout l, pmg_comm comm, int32_t n_neighbors, const int32_t* neighbor_ranks,
                        const int32_t* send_counts, const int32_t* recv_counts);

/* ---- halo windows: the neighbour exchange as direct stores into the neighbours' memory ----
 * A second route for the exchange of src/vector.hpp:186-238 between the GPUs of one node, next to the grouped
 * ncclSend / ncclRecv above: every rank owns a *window* of device memory which its neighbours map (hipIpc) and store
 * their packed values into; arrival and consumption are signalled by counters in a small flag block, double-buffered.
 * An exchange is two kernels on the compute stream (gather + store + signal; wait + copy + acknowledge): no second
 * stream, no host work beyond the two launches, capturable into a hipGraph on any runtime.  The reductions still use
 * the layout's communicator or callbacks.
 *
 *   pmg_window_alloc / _open / _close / _free : window memory (zeroed, fine-grained where the runtime offers it) and
 *       its 64-byte interprocess handle; the caller passes the handles between the ranks by whatever means it has
 *       (a file, MPI, torch.distributed.all_gather_object).  A rank that is its own neighbour passes its own pointers.
 *   pmg_layout_window_describe : for a plan (per-neighbour counts, in the order of the index lists given to
 *       pmg_layout_create) the size of the window in doubles and, per neighbour k, where in MY window k's values land
 *       (fwd_offsets: owner -> ghost; rev_offsets: ghost -> owner).  The flag block has PMG_WINDOW_FLAG_WORDS uint64.
 *   pmg_layout_set_windows : attaches my window and flag block and, per neighbour k, its mapped window and flag
 *       block, the size of its window (what IT got from describe), the offsets IT got from describe for ME, and my
 *       position in ITS neighbour list (nb_slot).  All memory must outlive the layout.
 * Every rank must call every scatter of a layout in the same order.  A wait that exceeds PMG_WINDOW_TIMEOUT_MS
 * (default 5000) ends the kernel and fails the next scatter of the layout with PMG_ERR_HIP. */
#define PMG_WINDOW_HANDLE_BYTES 64
#define PMG_WINDOW_MAX_NEIGHBORS 64
#define PMG_WINDOW_FLAG_WORDS (4 * PMG_WINDOW_MAX_NEIGHBORS + 8)
#define PMG_WINDOW_ERR_NO_ARRIVAL 1
#define PMG_WINDOW_ERR_SLOT_BUSY 2
int pmg_window_alloc(size_t bytes, void** ptr, char* handle /* [PMG_WINDOW_HANDLE_BYTES] */);
/* 1: the last pmg_window_alloc of this process obtained fine-grained device memory, 0: ordinary, -1: none yet */
int pmg_window_fine_grained(void);
int pmg_window_open(const char* handle, void** ptr);
int pmg_window_close(void* ptr);
int pmg_window_free(void* ptr);
/* A communicator made of windows: the reductions and the set-up gathers of the ranks of one node without a transport
 * library (no RCCL, no MPI): every rank allocates one window of PMG_COMM_WINDOW_BYTES with pmg_window_alloc, hands its
 * handle to all ranks, maps theirs (pmg_window_open; windows[rank] is its own pointer) and creates the communicator.
 * An all-reduce of up to PMG_COMM_WINDOW_CHUNK doubles is two kernels on the caller's stream (stores into every rank's window + flags; wait + combine in rank
 * order, so every rank gets the same bits), replays from a hipGraph, and costs no host work beyond the two launches.
 * Layouts on such a communicator need halo windows for their exchange (pmg_layout_set_windows).  Every rank must issue
 * the reductions of the communicator in the same order, one stream at a time.  The windows must outlive it. */
#define PMG_COMM_WINDOW_MAX_RANKS 16
#define PMG_COMM_WINDOW_CHUNK 16384 /* doubles per rank and exchange; longer vectors go chunk by chunk */
#define PMG_COMM_WINDOW_BYTES \
  (8 * (2 * PMG_COMM_WINDOW_MAX_RANKS + 8 + 2 * PMG_COMM_WINDOW_MAX_RANKS * PMG_COMM_WINDOW_CHUNK))
int pmg_comm_create_windows(pmg_comm* out, int rank, int nranks, void* const* windows /* [nranks] */);
int pmg_layout_window_describe(int32_t n_neighbors, const int32_t* send_counts, const int32_t* recv_counts,
                               int64_t* window_doubles, int64_t* fwd_offsets, int64_t* rev_offsets);
int pmg_layout_set_windows(pmg_layout l, int32_t n_neighbors, const int32_t* send_counts, const int32_t* recv_counts,
                           double* window, uint64_t* flags, double* const* nb_window, uint64_t* const* nb_flags,
                           const int64_t* nb_window_doubles, const int64_t* nb_fwd_offset, const int64_t* nb_rev_offset,
                           const int32_t* nb_slot);

/* Vector::scatter_fwd_begin / scatter_fwd_end (src/vector.hpp:186-238): owner ->
 * ghost update of x; pack/unpack run on `stream` without host synchronisation. */
int pmg_scatter_fwd_begin(pmg_layout l, const double* x, pmg_stream stream);
/* Forward scatters issued on the layout since its creation (one per operator application, prolongation or
 * restriction that needs its input's ghosts; the V-cycle skips those whose ghosts are current already, see
 * pmg_multigrid_apply).  For tests and for pricing a cycle's exchanges. */
long long pmg_layout_forward_scatters(pmg_layout l);
int pmg_scatter_fwd_end(pmg_layout l, double* x, pmg_stream stream);
/* Vector::scatter_rev_begin / _end (src/vector.hpp:249-286): ghost -> owner,
 * accumulated into the owned entries.  Not used on the hot path. */
int pmg_scatter_rev_begin(pmg_layout l, const double* x, pmg_stream stream);
int pmg_scatter_rev_end(pmg_layout l, double* x, pmg_stream stream);

/* ---- BLAS-1 (free functions of src/vector.hpp:333-454) ---------------------
 * Ranges follow the reference: set and scale touch owned+ghost entries
 * (:109-115, :413-418); axpy, copy, pointwise_mult and the reductions touch the
 * owned entries only (:398-407, :424-431, :438-447, :334-352).
 * Alignment: a vector needs the 8 bytes of a double, no more -- a sub-span of a larger
 * allocation is a legal argument here and wherever a function takes a vector (smoothers, CG,
 * the V-cycle).  Operands that all sit on 16-byte boundaries take the double2 kernels, any other
 * combination the scalar ones, with the same results to rounding.
 * A NaN in the owned entries comes out of every reduction, norm(linf) included. */
int pmg_vec_set(pmg_layout l, double* x, double value, pmg_stream stream);
int pmg_vec_scale(pmg_layout l, double* x, double alpha, pmg_stream stream);
int pmg_vec_copy(pmg_layout l, double* dst, const double* src, pmg_stream stream);
/* r = alpha * x + y */
int pmg_vec_axpy(pmg_layout l, double* r, double alpha, const double* x, const double* y,
                 pmg_stream stream);
/* w = x .* y */
int pmg_vec_pointwise_mult(pmg_layout l, double* w, const double* x, const double* y,
                           pmg_stream stream);
/* Synchronous reductions (block until the value is on the host, then allreduce). */
int pmg_vec_inner_product(pmg_layout l, const double* a, const double* b, double* result,
                          pmg_stream stream);
int pmg_vec_squared_norm(pmg_layout l, const double* a, double* result, pmg_stream stream);
/* norm_type 0 = l2, 1 = linf (max |a_i|; the reference's abs-after-max slip,
 * src/vector.hpp:381-382, is not reproduced). */
int pmg_vec_norm(pmg_layout l, const double* a, int norm_type, double* result, pmg_stream stream);
/* Remove the mean (not in the reference): x <- x - (sum x_i) / N with w == NULL, N the number of owned entries over
 * all ranks; with weights x <- x - (w . x) / (w . 1) -- w the lumped mass (pmg_laplacian_assemble_rhs of ones) gives
 * a zero integral mean.  The sums run over the owned entries through the layout's reduction path, the subtraction
 * over size_local + num_ghosts entries (the ghosts stay consistent).  The mean is the quotient sum / N, read by the
 * subtracting kernel from the device: no host synchronisation, and the call can be captured in a graph.  N is
 * counted once per layout (on several ranks that first call reduces and reads back: not inside a capture). */
int pmg_vec_remove_mean(pmg_layout l, double* x, const double* w, pmg_stream stream);

/* ---- matrix-free Laplacian (acc::MatFreeLaplacian, src/laplacian.hpp:284-526)
 * Arguments mirror the reference constructor (:289-297); all arrays are device
 * pointers except the two cell lists, which are host arrays like the
 * reference's std::vector<int>:
 *   kappa          [ncells]               DG-0 coefficient per cell (times the nodal field of
 *                  pmg_laplacian_set_coefficient_field, when one is set -- "variable coefficient" below)
 *   dofmap         [ncells * (degree+1)^3] local dof of (cell, t), t = a*nd^2+b*nd+c with a, b, c the
 *                  node numbers along x, y, z by ASCENDING coordinate (a basix / dolfinx dofmap numbers
 *                  the 1-D nodes endpoints first: use pmg_laplacian_create_ordered for it)
 *   xgeom          [3 * npoints]          vertex coordinates
 *   geom_dofmap    [8 * ncells]           cell vertices, tensor-product order k = i*4+j*2+l
 *   bc_marker      [size_local+num_ghosts] 1 on Dirichlet dofs
 *   lcells/bcells  cells that touch no ghost dof / cells that do (+ ghost cells),
 *                  src/mesh.hpp:105-143
 * The reference also takes dphi_geometry and G_weights from the caller
 * (basix tabulations of the trilinear coordinate element and the 3-D GLL
 * weights); they are fully determined by `degree`, so the library builds them
 * itself -- pass them to pmg_laplacian_create_with_tables to override.
 * The constructor precomputes the geometry tensor G for every listed cell
 * (geometry_computation, :22-113, with the determinant expanded correctly and G
 * tied to the cell, not to its position in the launched list -- SURVEY.md quirks
 * Q1, Q2) and groups the cells into coloured patches (its own copy of the
 * dofmap in patch form); it reads dofmap, bc_marker, xgeom and geom_dofmap back
 * to the host once for that.
 * Cell orientation is free: the local axes of a cell (the i, j, l of geom_dofmap, the a, b, c of dofmap -- the same
 * three axes in both) may run along any of the cell's edge directions, either way, in any order, and differently from
 * cell to cell, as in an imported mesh; a left-handed cell (det J < 0) is as good as a right-handed one.  Every
 * volume measure is |det J| (the reference's assembled path, src/precompute.hpp:96,230; its matrix-free kernel takes
 * the signed value): "detJ" below -- in G, in the load vector and in the reaction vector -- stands for |det J_q|.
 * adj(J) keeps its sign: it enters G twice and the facet measure through a norm.  For a right-handed cell nothing
 * changes, bit for bit.  A cell whose determinant changes sign inside the cell is not a valid cell.
 * What the library requires of a mesh: hexahedra with trilinear geometry (or, through pmg_laplacian_create_curved
 * below, with a tensor-product coordinate element of degree up to 4), and a CONFORMING dofmap -- two cells hold the
 * same dof exactly where they share the vertex, edge or face that carries it.  Nothing about structure or valence: an
 * edge may be shared by any number of cells (3 and 5 are tested), a vertex likewise (3 to 10), blocks may meet with
 * local axes that do not line up, the domain may have re-entrant corners and cavities, a partition interface need not
 * be a plane.  The patches are formed from cell centroids and dof sets alone; a group of cells with more distinct dofs
 * than a patch holds is halved until it fits.  The optional forms are taken only where the mesh allows them and are
 * refused before anything is launched otherwise: the two-stream split (PMG_APPLY_STREAMS) needs patch colours that
 * separate the two halves, the chain form (PMG_CHAIN) a tensor grid of patches; a mesh that has neither runs the
 * plain patch form.  The one hard limit: a patch colouring of more than 64 colours is refused with PMG_ERR_INVALID by
 * the constructor (no mesh of the suite needs more than 16).
 * Degrees 1..PMG_MAX_DEGREE are supported (the reference stops at 5, :335-346). */
int pmg_laplacian_create(pmg_laplacian* out, pmg_layout layout, int degree, int32_t ncells,
                         const double* kappa, const int32_t* dofmap, const double* xgeom,
                         int32_t npoints, const int32_t* geom_dofmap, const int32_t* lcells,
                         int32_t n_lcells, const int32_t* bcells, int32_t n_bcells,
                         const int8_t* bc_marker, pmg_stream stream);
int pmg_laplacian_create_with_tables(pmg_laplacian* out, pmg_layout layout, int degree,
                                     int32_t ncells, const double* kappa, const int32_t* dofmap,
                                     const double* xgeom, int32_t npoints,
                                     const int32_t* geom_dofmap, const double* dphi_geometry,
                                     const double* G_weights, const int32_t* lcells,
                                     int32_t n_lcells, const int32_t* bcells, int32_t n_bcells,
                                     const int8_t* bc_marker, pmg_stream stream);
/* The same for a caller whose cell-local node numbering is not ascending (see "cell-local node order"
 * above): `dofmap`, and dphi_geometry / G_weights when given (both may be NULL), are indexed in
 * `node_order`; custom_perm1d [degree + 1] only for PMG_NODES_CUSTOM.  A dolfinx / basix caller passes
 * PMG_NODES_ENDPOINTS_FIRST with the arrays exactly as the reference's constructor receives them
 * (src/laplacian.hpp:289-297).  The operator keeps its own ascending copy of the dofmap. */
int pmg_laplacian_create_ordered(pmg_laplacian* out, pmg_layout layout, int degree, int32_t ncells,
                                 const double* kappa, const int32_t* dofmap, const double* xgeom, int32_t npoints,
                                 const int32_t* geom_dofmap, const double* dphi_geometry, const double* G_weights,
                                 const int32_t* lcells, int32_t n_lcells, const int32_t* bcells, int32_t n_bcells,
                                 const int8_t* bc_marker, int node_order, const int32_t* custom_perm1d,
                                 pmg_stream stream);
int pmg_laplacian_node_order(pmg_laplacian op); /* PMG_NODES_* the operator was created with */
/* ---- curved cells: a coordinate element of degree 1..PMG_MAX_GEOM_DEGREE
 * The mesh requirement above ("trilinear geometry") is the geom_degree = 1 case of this constructor, which all the
 * others call.  Conventions:
 *   coordinate element  the tensor-product Lagrange element of degree g = geom_degree on the hexahedron.  Its 1-D nodes
 *                  are the GLL points of degree g on [0, 1] (pmg_gll_table(g + 1)); for g <= 2 these are the
 *                  equispaced points.  A caller with another node family passes its own tabulation (last entry).
 *   geom_dofmap    [ncells * (g+1)^3]  the cell's nodes, k = (i*(g+1) + j)*(g+1) + l with i, j, l the node numbers
 *                  along the cell's axes x, y, z by ASCENDING coordinate -- for g = 1 the k = i*4+j*2+l above.  The
 *                  axes are the same three as those of `dofmap`.  `node_order` applies to `dofmap`, to the rows (q) of
 *                  dphi_geometry and to G_weights only: the geometry nodes are always in ascending tensor order (a
 *                  geometry dofmap in another order, e.g. a dolfinx hex27 one, is permuted by the caller).
 *   xgeom          [3 * npoints] as before.  A node shared by two cells may be stored once or once per cell; the
 *                  library relies on neither.
 *   frames         cell frames and left-handed cells work as for g = 1: measures are |det J|, adj(J) keeps its sign.
 *   caller tables  dphi_geometry [3][nq][(g+1)^3] and G_weights [nq], both given or both NULL, override the library's
 *                  tabulation: q in the caller's node_order, k in ascending tensor order.
 * Every entry of geom_dofmap must lie in [0, npoints); a geom_degree outside 1..PMG_MAX_GEOM_DEGREE is refused with
 * PMG_ERR_INVALID.  On any refusal *out is NULL.  With the library's own tabulation the tensor of a g >= 2 operator is
 * built by a cell-cooperative, sum-factorised kernel; with caller tables, which need not be a tensor product, by a
 * thread per point over the dense table.  The stored tensor is per quadrature point already, so the apply kernels, the
 * diagonal, the assembled matrix, the transfers and the smoothers are those of a trilinear mesh.  A cell is affine
 * (pmg_laplacian_is_affine) only if every one of its (g+1)^3 nodes sits where the affine map of its corners puts it. */
#define PMG_MAX_GEOM_DEGREE 4
int pmg_laplacian_create_curved(pmg_laplacian* out, pmg_layout layout, int degree, int32_t ncells, const double* kappa,
                                const int32_t* dofmap, const double* xgeom, int32_t npoints, int geom_degree,
                                const int32_t* geom_dofmap, const double* dphi_geometry, const double* G_weights,
                                const int32_t* lcells, int32_t n_lcells, const int32_t* bcells, int32_t n_bcells,
                                const int8_t* bc_marker, int node_order, const int32_t* custom_perm1d,
                                pmg_stream stream);
int pmg_laplacian_geometry_degree(pmg_laplacian op); /* 1..PMG_MAX_GEOM_DEGREE; -1 for NULL */
/* Host, no GPU: what the coordinate element's tabulate(1, GLL points of `degree`) returns, dphi[3][nq][(g+1)^3] with
 * q in node_order and k in ascending tensor order -- the table the library builds for itself. */
int pmg_coordinate_element_table(int degree, int geom_degree, int node_order, const int32_t* custom_perm1d,
                                 double* dphi);
int pmg_laplacian_destroy(pmg_laplacian op);
/* operator()(in, out), :462-482: zeroes `out` (ghosts included), updates the
 * ghosts of `in` (side effect, as in the reference), interior cells overlap
 * the halo exchange, then the boundary cells. */
int pmg_laplacian_apply(pmg_laplacian op, double* in, double* out, pmg_stream stream);
/* The same application in FP32 (the operator of the FP32 V-cycle, pmg_multigrid_set_precision): `in` and `out` are
 * device arrays of size_local floats; `out` is overwritten, Dirichlet rows are out = in, interior and boundary cell
 * lists are both applied.  The geometry tensor is computed in FP64 from the mesh and rounded to float once -- 24 bytes
 * per quadrature point, built on the first FP32 use and freed with the operator; kappa is read from the caller's array
 * in every application (as in pmg_laplacian_apply: the caller may change it between two).  The patch plan and its
 * launches are the FP64 apply's, the cell sums are float.  Refused with PMG_ERR_INVALID: a layout with
 * ghosts or a communicator (FP32 is single-domain only), an operator in batched-geometry mode.  The geometry mode
 * (affine cells) and the chain form do not apply: the float form always streams its stored tensor. */
int pmg_laplacian_apply_f32(pmg_laplacian op, float* in, float* out, pmg_stream stream);
/* get_diag_inverse / set_diag_inverse, :484-495 (owned+ghost entries). */
int pmg_laplacian_get_diag_inverse(pmg_laplacian op, double* diag_inv, pmg_stream stream);
int pmg_laplacian_set_diag_inverse(pmg_laplacian op, const double* diag_inv, pmg_stream stream);
/* Matrix-free inverse diagonal of the BC-treated operator, stored in the
 * operator: replaces "assemble a CSR to read its diagonal"
 * (examples/pmg/main.cpp:274-279, src/csr.hpp:100-110).  BC rows give 1. */
int pmg_laplacian_compute_diag_inverse(pmg_laplacian op, pmg_stream stream);
/* The precomputed geometry tensor in the reference's layout [ncells][nq][6]
 * (:99-111), for parity tests.  `G_out` is a device array; q = ja*nd^2 + jb*nd + jc in the node order
 * the operator was created with (ascending unless pmg_laplacian_create_ordered said otherwise).  It is the tensor
 * as the kernels read it: with a coefficient field set, G_q carries the field's value at its point. */
int pmg_laplacian_get_geometry(pmg_laplacian op, double* G_out, pmg_stream stream);
/* Variable coefficient: -div(kappa(x) grad u) with kappa a function of the operator's own space (not in the
 * reference, whose coefficient is one value per cell).  With GLL collocation the quadrature points are the nodes, so
 * such a coefficient is one value per (cell, point), kq[dof(cell, q)], and it is folded into the stored tensor where
 * the tensor is built: every form of the apply streams the same 48 bytes per point as without a field, and the
 * diagonal, the assembled matrix (pmg_matrix_*) and the AMG set-up read that one tensor.  The effective coefficient
 * is kappa[cell] * kq[dof(cell, q)]: the per-cell array keeps its meaning and is still read in every application.
 *
 * `kq` is a device array of size_local owned nodal values in the operator's dof numbering (entries beyond size_local
 * are ignored); the library copies them and fills the ghost entries of its copy with the layout's own forward
 * scatter, so a caller on several ranks need not have scattered the array -- there the call is collective -- and
 * may free it on return.  kq = NULL removes the field and restores the tensor without one bit for bit.  Every owned
 * entry must be finite and greater than 0 (one small reduction, summed over the ranks); otherwise PMG_ERR_INVALID
 * and nothing has changed.  The call rebuilds what depends on the tensor: the resident FP64 tensor (in batched-
 * geometry mode every application folds the field in as it recomputes its batch), the float tensor if it has been
 * built, and the inverse diagonal if it came from pmg_laplacian_compute_diag_inverse (a diagonal installed with
 * pmg_laplacian_set_diag_inverse is left alone).  An assembled matrix follows with pmg_matrix_update_values; a
 * smoother's eigenvalue bound and an AMG hierarchy are the caller's to renew (the hierarchy in place, with
 * pmg_amg_update_values).  All buffers are rebuilt in place and
 * keep their addresses, so a captured V-cycle graph over the resident tensor stays valid (an FP32 cycle re-captures
 * because the diagonal changed; in batched-geometry mode the captured geometry launches carry the field's address,
 * and setting the first field or removing it re-captures).  Like the other set-up calls it allocates and
 * synchronises the stream: not inside a stream capture (refused).  The affine geometry mode streams one tensor per
 * cell and cannot carry a field: pmg_laplacian_set_geometry_mode(op, 1) is refused while a field is set, and
 * setting a field is refused in affine mode (PMG_ERR_INVALID both ways).
 * pmg_laplacian_has_coefficient_field: 1 / 0. */
int pmg_laplacian_set_coefficient_field(pmg_laplacian op, const double* kq, pmg_stream stream);
int pmg_laplacian_has_coefficient_field(pmg_laplacian op);
/* Full-tensor diffusion: -div(K grad u) with K symmetric positive definite and constant per cell (not in the
 * reference).  The stored tensor G_q = adj(J) adj(J)^T w_q / detJ (detJ = |det J_q|) enters the form linearly, and with a tensor K_c it
 * becomes G_q = adj(J) K_c adj(J)^T w_q / detJ: still six symmetric entries per point, so every form of the apply
 * streams the same bytes as without one, and the diagonal, the assembled matrix (pmg_matrix_*) and the AMG set-up read
 * that one tensor.  The effective coefficient is kappa[cell] * kq[dof(cell, q)] * K[cell]: the per-cell array and the
 * nodal field keep their meaning and combine with it.
 *
 * `kt` is a device array [ncells][6], one tensor per local cell, ghost cells included -- exactly the cells kappa
 * covers -- with the components in physical coordinates in the order (xx, xy, xz, yy, yz, zz), the order of G.  The
 * library copies it; the caller may free it on return.  kt = NULL removes the tensor and restores the stored tensor
 * without one bit for bit.  Every component must be finite and every tensor positive definite (leading minors:
 * xx > 0, xx yy - xy^2 > 0, det > 0; one small reduction over the cells, summed over the ranks, so all ranks refuse
 * or none does -- on several ranks the call is collective); otherwise PMG_ERR_INVALID, the message names how many
 * cells failed, and nothing has changed.  The call rebuilds what depends on the tensor, in place and at the same
 * addresses: the resident FP64 tensor (in batched-geometry mode every application folds the tensor in as it recomputes
 * its batch), the float tensor if it has been built, the per-cell tensor of the affine mode (it becomes
 * adj(J) K adj(J)^T / detJ), and the inverse diagonal if it came from pmg_laplacian_compute_diag_inverse (a diagonal
 * installed with pmg_laplacian_set_diag_inverse is left alone).  An assembled matrix follows with
 * pmg_matrix_update_values; a smoother's eigenvalue bound and an AMG hierarchy are the caller's to renew (the hierarchy
 * in place, with pmg_amg_update_values).  A captured
 * V-cycle graph over the resident tensor stays valid (an FP32 cycle re-captures because the diagonal changed; in
 * batched-geometry mode the captured geometry launches carry the tensor's address, and setting the first tensor or
 * removing it re-captures).  Like the other set-up calls it allocates and synchronises the stream: not inside a stream
 * capture (refused).  A per-cell tensor is constant over an affine cell, so unlike the nodal field it works in the
 * affine geometry mode, in either order of the two calls.  pmg_laplacian_apply_lifting follows the tensor;
 * pmg_laplacian_assemble_rhs and pmg_laplacian_assemble_neumann do not read it.
 * pmg_laplacian_has_coefficient_tensor: 1 / 0, -1 for NULL. */
int pmg_laplacian_set_coefficient_tensor(pmg_laplacian op, const double* kt, pmg_stream stream);
int pmg_laplacian_has_coefficient_tensor(pmg_laplacian op);
/* Reaction term: -div(K grad u) + sigma u with sigma >= 0 constant per cell (not in the reference) -- an implicit
 * step of the heat equation (M / dt + K), a screened Poisson problem, a Robin-type penalty.  With GLL collocation the
 * quadrature points are the nodes, so the mass matrix is diagonal and the term is one vector over the dofs,
 *   d[dof] = sum over the listed cells c that hold the dof, at the cell's point q on it, of sigma[c] * w_q * detJ_q
 * (detJ_q = |det J_q|; the weights of pmg_laplacian_assemble_rhs with sigma in place of kappa and f = 1; 0 on marked dofs).  The operator
 * becomes y = A x + d .* x on unmarked rows; Dirichlet rows stay y = x.  d does not depend on the stored tensor, so
 * the call combines freely with kappa, the nodal field, the coefficient tensor, both geometry modes and batched
 * geometry.  No apply form takes a further pass over the vectors: in the FP64 and FP32 patch kernels the first patch
 * of a dof starts its sum at d * x where it started at 0, and the fused restriction (pmg_interpolator_restrict_residual)
 * spreads r - d z over the cells where it spread r.  The chain form
 * (pmg_laplacian_set_chain_form) does not carry the term: while one is set, the operator's interior runs as the
 * column launches, and pmg_laplacian_launches_per_apply counts those.
 *
 * `sigma` is a device array [ncells], one value per local cell, ghost cells included -- exactly the cells kappa
 * covers.  The library keeps d, not sigma; the caller may free sigma on return.  sigma = NULL removes the term and
 * restores every apply form (FP64, FP32, fused restriction) bit for bit; a computed inverse diagonal is recomputed by
 * the code of an operator without a term, whose atomic sums meet in no fixed order, so it agrees with that operator's
 * to rounding as two computations of it always do.  Every value must be finite and >= 0 (all zeros is
 * legal; one small reduction over the cells, summed over the ranks, so all ranks refuse or none does -- on several
 * ranks the call is collective); otherwise PMG_ERR_INVALID, the message names how many cells failed, and nothing has
 * changed.  The call builds, and a later call rebuilds in place at the same addresses: d over size_local +
 * num_ghosts (ghost entries hold this rank's cells only, as those of the computed diagonal), its float copy if the
 * float tensor has been built (otherwise the first FP32 use builds it), and the inverse diagonal if it came from
 * pmg_laplacian_compute_diag_inverse -- 1 / (diag(A) + d), 1 on marked rows (a diagonal installed with
 * pmg_laplacian_set_diag_inverse is left alone).  d is summed with atomics: two sets of the same values agree to
 * rounding, not bit for bit.  An assembled matrix follows with pmg_matrix_update_values (d on the diagonal of the
 * unmarked rows); a smoother's eigenvalue bound and an AMG hierarchy (d on the diagonal of its level 0) are the
 * caller's to renew (the hierarchy in place, with pmg_amg_update_values).  The first set and the removal change a
 * kernel argument, so cached V-cycle graphs re-capture; a
 * second set with other values keeps them valid.  Like the other set-up calls it allocates and synchronises the
 * stream: not inside a stream capture (refused).  pmg_laplacian_apply_lifting, pmg_laplacian_set_bc,
 * pmg_laplacian_assemble_rhs and pmg_laplacian_assemble_neumann do not change: a diagonal term couples no unmarked row
 * to a marked column.
 * pmg_laplacian_has_reaction: 1 / 0, -1 for NULL: "a sigma is set".  A Robin boundary term (pmg_laplacian_set_robin,
 * below) is a second component of the same vector, set and removed independently: while one is set, sigma = NULL
 * leaves the vector equal to that component, and "d" above reads d_sigma + d_R. */
int pmg_laplacian_set_reaction(pmg_laplacian op, const double* sigma, pmg_stream stream);
int pmg_laplacian_has_reaction(pmg_laplacian op);
/* GLL-collocated load vector b_i = sum_cells kappa * w_q * detJ_q * f_i at q = i, detJ_q = |det J_q|
 * (what dolfinx assemble_vector does for L = inner(f, v)*dx with the GLL rule,
 * examples/pmg/poisson.py:40; examples/pmg/main.cpp:289-295), then set_bc:
 * b[bc] = 0.  `f` holds the nodal values of the source term.  The scaling is by the per-cell kappa only (the
 * reference's manufactured load), also when a coefficient field is set: a caller with a field passes the nodal
 * values of its own f. */
int pmg_laplacian_assemble_rhs(pmg_laplacian op, const double* f, double* b, pmg_stream stream);
/* ---- boundary data: Dirichlet lifting, set_bc and the Neumann load (not in the reference's library: its drivers
 * call dolfinx's fem::apply_lifting and fem::set_bc, examples/cg/main.cpp:231-236, examples/mat_free/main.cpp:253-255)
 * The right-hand side of a problem with non-zero Dirichlet values and prescribed fluxes, computed on the device from
 * the operator the caller already has, at O(surface) cost: no second operator with an empty marker, no full-volume
 * apply.  `g`, `x0` and `b` are device arrays of size_local + num_ghosts entries in the operator's dof numbering.
 * Unmarked entries of g and x0 are never read (they may hold anything, a NaN included).  Only the owned rows of b are
 * meaningful afterwards, as with pmg_laplacian_assemble_rhs.  None of the calls touches the stored tensor, the patch
 * plan or a launch of the apply, and all of them work in every geometry mode, with batched geometry, with the chain
 * form and with a coefficient field (the lifting recomputes the geometry of its cells from the mesh).
 *
 * pmg_laplacian_apply_lifting -- dolfinx fem::apply_lifting(b, {a}, {{bc}}, {x0}, alpha) for this operator:
 *     b[i] -= alpha * sum_{j marked} A_ij * (g[j] - x0[j])     for every owned, unmarked row i,
 *   A the UNCONSTRAINED operator (no row / column treatment) with the current coefficient kappa[cell] * kq[dof(cell,q)].
 *   x0 may be NULL (= 0).  Marked rows of b are not touched.  The ghosts of g are refreshed with the layout's forward
 *   scatter (a side effect, as pmg_laplacian_apply has on `in`; collective on several ranks); the ghosts of x0 are the
 *   caller's to have scattered.  The first call of an operator reads the dofmap and the marker back once and keeps the
 *   list of cells that hold a marked dof (pmg_laplacian_lift_cell_count; -1 before): that call is refused inside a
 *   stream capture.  One workgroup per listed cell sums through atomics: two calls agree to rounding, not bit for bit.
 * pmg_laplacian_set_bc -- dolfinx fem::set_bc(b, {bc}, x0, alpha): b[i] = alpha * (g[i] - x0[i]) on every marked
 *   i < size_local; x0 may be NULL.  Also the way to put g into an initial guess (alpha = 1, x0 = NULL).
 * pmg_laplacian_assemble_neumann -- the GLL-collocated int_Gamma h v ds over the listed facets:
 *     b[i] += sum over facets F and face points s of F with dof(F, s) = i:  w1[i1] * w1[i2] * |dS| * h[F][s]
 *   on unmarked owned rows.  facet_cells / facet_local are HOST arrays; a cell may come from either cell list, ghost
 *   cells included (each rank lists the exterior facets of all cells it holds, so owned rows are complete without a
 *   reverse scatter).  Local facet number = 2 * axis + side: axis 0, 1, 2 are the cell's reference axes in the tensor
 *   order of geom_dofmap (k = i*4 + j*2 + l) and of the ascending node number t = a*nd^2 + b*nd + c; side 0 is the face
 *   xi_axis = 0, side 1 the face xi_axis = 1 -- also for an operator created in another cell-local node order.  `h` is
 *   a device array [nfacets][nd*nd], s = i1*nd + i2 over the two remaining axes in increasing axis order, by ascending
 *   coordinate: one value per facet point, not per dof, because a dof on an edge between two Neumann faces has two
 *   normals.  |dS| is the Euclidean norm of row `axis` of adj(J) at the point (the outward area vector is +- that row;
 *   the sign belongs to the caller's h = flux . n).  nfacets == 0 is a no-op.  It uploads the lists and waits for the
 *   stream: refused inside a stream capture.
 * Refused with PMG_ERR_INVALID and nothing written: a NULL op, g or b, a NULL h or NULL facet lists with nfacets > 0;
 * b overlapping g, x0 or h; a facet cell outside [0, ncells) or not in the operator's cell lists; a local facet outside
 * 0..5. */
int pmg_laplacian_apply_lifting(pmg_laplacian op, double* g, const double* x0, double alpha, double* b, pmg_stream stream);
int pmg_laplacian_set_bc(pmg_laplacian op, const double* g, const double* x0, double alpha, double* b, pmg_stream stream);
int pmg_laplacian_assemble_neumann(pmg_laplacian op, int32_t nfacets, const int32_t* facet_cells,
                                   const int8_t* facet_local, const double* h, double* b, pmg_stream stream);
int pmg_laplacian_lift_cell_count(pmg_laplacian op);
/* ---- Robin boundary term: K grad u . n + alpha u = g on the listed facets (not in the reference: its drivers get
 * boundary terms from dolfinx forms).  The weak form gains int_Gamma alpha u v ds on the operator and int_Gamma g v ds
 * on the right-hand side.  With GLL collocation the face quadrature points are the face nodes, so the face mass matrix
 * is diagonal, with the weights pmg_laplacian_assemble_neumann uses:
 *     d_R[dof] = sum over listed facets F and points s with dof(F, s) = dof:  w1[i1] * w1[i2] * |dS| * alpha[F][s],
 * zero on marked dofs, over size_local + num_ghosts (ghost entries hold this rank's facets only, as the other diagonal
 * vectors do).  The operator becomes y = A x + (d_sigma + d_R) .* x on unmarked rows, d_sigma the vector of
 * pmg_laplacian_set_reaction; marked rows stay y = x.  The two terms are set and removed independently; each component
 * is kept in a buffer of its own, and the kernels read one vector: an exact copy of the only component present, or
 * d_sigma + d_R in that order, always in the same allocation once it exists.  So everything said of the reaction term
 * holds for this one through the same code: no apply form takes a further pass (FP64, FP32, fused restriction), the
 * chain form is bypassed while either term is set (pmg_laplacian_launches_per_apply counts the column launches), the
 * float copy and an inverse diagonal computed by pmg_laplacian_compute_diag_inverse -- 1 / (diag(A) + d_sigma + d_R)
 * -- follow the call, pmg_matrix_update_values and pmg_amg_create* read the summed vector, and the smoother's
 * eigenvalue bound and an AMG hierarchy are the caller's to renew (the hierarchy in place, with
 * pmg_amg_update_values).  Setting either term a second time, or adding the
 * second term beside the first, rewrites the vector in place: cached V-cycle graphs stay valid.  The first term set and
 * the last term removed change a kernel argument: they re-capture.  pmg_laplacian_set_reaction(op, NULL) while a Robin
 * term is set leaves the vector equal to d_R.
 *
 * facet_cells / facet_local are HOST arrays with the conventions of pmg_laplacian_assemble_neumann: local facet =
 * 2 * axis + side, ghost cells included (each rank lists the exterior facets of all cells it holds), and the same
 * refusals for a cell outside the operator's lists and a facet outside 0..5.  `alpha` is a DEVICE array
 * [nfacets][nd*nd], one value per facet point in the order of `h` there (s = i1*nd + i2, ascending coordinate, also
 * for an operator created in another cell-local node order); per facet point, not per dof: a dof on an edge between two
 * Robin faces gets both faces' weights.  Every value must be finite and >= 0 (all zeros is legal); the bad values are
 * counted on the device and the count is summed over the ranks, so all ranks refuse or none does: PMG_ERR_INVALID, the
 * message names the count, nothing has changed.  nfacets == 0 removes the term (alpha and the lists may then be NULL);
 * a rank that holds no listed facet passes 0 too.  The call is collective on several ranks in every case.  It
 * allocates and synchronises the stream: refused inside a stream capture.  d_R is summed with atomics: two sets of
 * the same values agree to rounding, not bit for bit.
 * pmg_laplacian_apply_lifting, pmg_laplacian_set_bc, pmg_laplacian_assemble_rhs and pmg_laplacian_assemble_neumann do
 * not change: a diagonal term couples no unmarked row to a marked column.  The Robin data g (= alpha u_inf for a
 * convective boundary alpha (u - u_inf)) enters the right-hand side through pmg_laplacian_assemble_neumann with h = g.
 * pmg_laplacian_has_robin: 1 / 0, -1 for NULL; pmg_laplacian_has_reaction keeps meaning "a sigma is set". */
int pmg_laplacian_set_robin(pmg_laplacian op, int32_t nfacets, const int32_t* facet_cells,
                            const int8_t* facet_local, const double* alpha, pmg_stream stream);
int pmg_laplacian_has_robin(pmg_laplacian op);
/* ---- per-cell bilinear form: cell energies and the gradient with respect to kappa (not in the reference) ----
 * The diffusion term's bilinear form, cell by cell:
 *     out_cells[c] = sum over the quadrature points q of cell c of  (grad_ref v)_q^T G_q (grad_ref u)_q   [ x kappa[c] ]
 * with G_q = adj(J) K_c adj(J)^T w_q / |det J| kq[dof(c, q)], the tensor the apply uses (the nodal field kq and the
 * per-cell tensor K_c where they are set, curved cells included), WITHOUT kappa unless PMG_CELL_FORM_KAPPA is given;
 * with it, kappa[c] is read at call time, as the apply reads it.  The sum over the listed cells of the value with both
 * flags is v_m . (A u_m) of the operator (u_m, v_m: the vectors with their marked entries zeroed); the value with
 * PMG_CELL_FORM_CONSTRAINED alone is v^T (dA/dkappa_c) u of the boundary-treated A, so that for a functional J(x) of
 * the solution of A x = b the adjoint gradient is dJ/dkappa_c = -out_cells[c] with u = x and v = lambda = A^-1 dJ/dx;
 * u == v gives the energy of a function, cell by cell.
 *
 * `u` and `v` are device arrays of size_local + num_ghosts doubles in the operator's dof numbering; they may be the
 * same array.  `out_cells` is a device array of `ncells` doubles, one per cell of the operator's dofmap in the caller's
 * cell numbering: EVERY cell gets a value, ghost cells and cells in neither cell list included.
 * NO EXCHANGE: unlike pmg_laplacian_apply, the call does not scatter: the ghost entries of u and v must be current
 * (pmg_scatter_fwd_begin / _end) -- they are read as they are.  The call is not collective.
 * Only the diffusion form is computed.  The reaction and Robin terms (pmg_laplacian_set_reaction,
 * pmg_laplacian_set_robin) are not part of it: setting them does not change a bit of the result, and their own
 * sensitivities (the per-cell mass and the per-facet mass forms) are not provided.
 * The geometry is formed in place from the mesh, so the call works, with the same code, whatever the tensor's layout,
 * in batched-geometry mode, in the affine mode, with the chain form and with either recompute switch.  It is ONE kernel
 * launch on `stream` without host synchronisation or allocation: it can be captured.  A cell's sum is taken in a fixed
 * order without atomics: two calls on the same data give the same bytes.
 * Refused with PMG_ERR_INVALID and out_cells untouched: a NULL op, u, v or out_cells; a flag bit other than the two
 * below; out_cells overlapping u or v. */
#define PMG_CELL_FORM_KAPPA        1  /* multiply by kappa[cell], read at call time like the apply */
#define PMG_CELL_FORM_CONSTRAINED  2  /* marked dofs of u and v read as zero: v^T (dA/dkappa_c) u of the BC-treated A */
int pmg_laplacian_cell_form(pmg_laplacian op, const double* u, const double* v, double* out_cells,
                            int flags, pmg_stream stream);
/* ---- coefficient gradients of the form: kappa, nodal field, tensor, reaction (not in the reference) ----
 * The derivatives of v_m^T A u_m with respect to each coefficient that enters A linearly, from ONE kernel that forms
 * the point geometry once.  At the point q of cell c, with K = adj(J), detJ = |det J|, du / dv the reference gradients
 * of u / v, pu_d = sum_r K[r][d] du_r (pv likewise), T_c the cell's coefficient tensor (the identity when none is set),
 * kq_q = kq[dof(c, q)] (1 when no field is set), kappa_c read at call time and t_q = pv . T_c pu, each output is the
 * derivative with respect to its own coefficient, which is divided out; all the others stay in, as currently set:
 *     d_kappa[c]     = sum_q (w_q / detJ) kq_q t_q                   (pmg_laplacian_cell_form without PMG_CELL_FORM_KAPPA)
 *     d_field[n]     = sum over the points (c, q) with dof(c, q) = n, c in the operator's two cell lists, of
 *                      kappa_c (w_q / detJ) t_q
 *     d_tensor[c][k] = kappa_c sum_q (w_q / detJ) kq_q m_k,  k over (xx, xy, xz, yy, yz, zz), m_xx = pv_x pu_x,
 *                      m_xy = pv_x pu_y + pv_y pu_x: a packed off-diagonal value fills two entries of the matrix
 *     d_sigma[c]     = sum_q w_q detJ u_q v_q                        (the lumped cell mass form: the derivative of the
 *                      d .* x term of pmg_laplacian_set_reaction)
 * A gradient is defined whether or not its coefficient is currently set: it is then taken at kq = 1 or T = I.  For a
 * functional J(x) of the solution of A x = b the adjoint gradients are minus these outputs with u = x,
 * v = lambda = A^-1 dJ/dx and PMG_CELL_FORM_CONSTRAINED.  The Robin coefficient's sensitivity is not provided.
 *
 * `u`, `v`: device arrays of size_local + num_ghosts doubles, as for pmg_laplacian_cell_form; they may be the same
 * array.  Each output is a device array or NULL: d_kappa [ncells], d_field [size_local + num_ghosts], d_tensor
 * [ncells][6], d_sigma [ncells].  A NULL output is not computed and costs nothing.  The per-cell outputs get a value
 * for EVERY cell of the dofmap, ghost cells and cells in neither cell list included; d_field sums over the cells of the
 * two cell lists only, the cells the apply visits: entries that no listed cell touches are exactly 0.  d_field is NOT
 * zero on marked dofs: the point on a marked node still sees the unmarked dofs of its lines.  On a ghost-layer
 * partition the owned entries of d_field are complete; ghost entries hold this rank's cells only, as those of the
 * computed diagonal do.
 * `flags`: 0 or PMG_CELL_FORM_CONSTRAINED (marked dofs of u and v read as zero, by a select: a NaN in a marked entry
 * stays out).  PMG_CELL_FORM_KAPPA and every other bit are refused.
 * NO EXCHANGE, not collective: the ghost entries of u and v are read as they are.
 * The geometry is formed in place from the mesh, so the call works in every state the cell form works in (curved
 * cells, batched geometry, the affine mode, the chain form, either recompute switch).  With d_field given, one fill of
 * d_field with zeros on `stream` comes first; then ONE kernel launch.  No host synchronisation and no allocation: the
 * call can be captured.  The per-cell sums are taken in a fixed order without atomics: two calls on the same data give
 * the same bytes, and an output has the same bytes whichever other outputs are requested beside it.  d_field is summed
 * with FP64 atomics: it agrees to rounding from call to call.
 * Refused with PMG_ERR_INVALID and nothing written: a NULL op, u or v; all four outputs NULL; an illegal flag bit; an
 * output overlapping u, v or another output. */
int pmg_laplacian_form_gradients(pmg_laplacian op, const double* u, const double* v,
                                 double* d_kappa,  /* [ncells]                  or NULL */
                                 double* d_field,  /* [size_local + num_ghosts] or NULL */
                                 double* d_tensor, /* [ncells][6]               or NULL */
                                 double* d_sigma,  /* [ncells]                  or NULL */
                                 int flags, pmg_stream stream);
int pmg_laplacian_degree(pmg_laplacian op);
/* Geometry mode of the apply.  0 (default): the reference's data structure, the
 * stored tensor G[cell][q][6] is streamed (48 bytes per quadrature point).
 * 1: affine cells -- when every cell is a parallelepiped, G_q = w_q * Gc with one
 * constant tensor per cell, so the kernel reads 48 bytes per CELL instead (same
 * result to rounding; not in the reference; SURVEY.md 8d calls this byte model
 * separate from storedG).  Fails if the mesh has a non-affine cell, or while a
 * coefficient field is set (pmg_laplacian_set_coefficient_field).  A per-cell coefficient tensor
 * (pmg_laplacian_set_coefficient_tensor) is constant over a cell and is carried by both modes. */
int pmg_laplacian_is_affine(pmg_laplacian op);
int pmg_laplacian_set_geometry_mode(pmg_laplacian op, int mode);
/* Recomputed tensor (not in the reference).  Where the coordinate element is trilinear the Jacobian down a column of
 * quadrature points is linear in the column's coordinate, so the degree-1 and degree-2 apply kernels can form G_q in
 * their layer march from 24 coefficients per cell (192 bytes) instead of streaming 48 bytes per point; same result to
 * rounding (about 1e-15 of max |y|).  G is still built and kept: the diagonal, pmg_laplacian_get_geometry, the
 * assembled matrix, the AMG set-up and the FP32 cycle read it.
 * An operator is eligible when it was created without caller tables and with geometry degree 1, its degree is 1 or 2,
 * the geometry is resident (no batching), the geometry mode is 0, and neither a nodal coefficient field nor a per-cell
 * coefficient tensor is set; eligibility is evaluated at every application, so setting a field falls back to the
 * stream and removing it returns to the recomputed form.
 * mode -1 (default): automatic -- on at both degrees (profiles/tensor_recompute.md); 0: always stream;
 * 1: recompute where eligible -- PMG_ERR_INVALID with the reason if the operator is not eligible now, nothing changes.
 * PMG_TENSOR_RECOMPUTE=0 / 1 in the environment, read at creation, sets mode 0 / 1 (1 without the error: an ineligible
 * operator streams); a measurement switch like PMG_STREAM_POLICY.  The first choice of the form builds the
 * coefficients on the default stream: not inside a stream capture.  A graph captured by pmg_multigrid_set_graph is
 * re-captured when the choice changes.
 * pmg_laplacian_tensor_recomputed: 1 if the next application recomputes, 0 if it streams, -1 for NULL. */
int pmg_laplacian_set_tensor_recompute(pmg_laplacian op, int mode);
int pmg_laplacian_tensor_recomputed(pmg_laplacian op);
/* The recomputed tensor at degree 4.  The same form, in the degree-4 apply kernel and the fused (4, 2) restriction;
 * the 15 values of a column's Jacobian fit beside the layer march because these two kernels take their transposed
 * contractions by the barycentric identity (D^T f as the forward contraction of the scaled fluxes) instead of holding
 * the transposed table.  Same result to rounding.  It has a switch of its own: the pair above keeps its contract, under
 * which a degree-4 operator reports 0 and refuses mode 1.  Neither switch moves the other.
 * Eligible is a degree-4 operator that meets the conditions above and is not in the chain form
 * (pmg_laplacian_set_chain_form); evaluated at every application.  The FP32 cycle keeps the float tensor.
 * mode -1 (default): automatic -- on (profiles/tensor_recompute_p4.md); 0: always stream; 1: recompute where
 * eligible -- PMG_ERR_INVALID with the reason if the operator is not eligible now, nothing changes.
 * PMG_TENSOR_RECOMPUTE_IDENTITY=0 / 1 in the environment, read at creation, sets mode 0 / 1 (1 without the error).
 * The choice is part of what a captured graph is keyed by, and the first choice builds the cell coefficients on the
 * default stream, as above.
 * pmg_laplacian_tensor_recomputed_identity: 1 if the next application of a degree-4 operator recomputes, 0 if it
 * streams (every other degree: 0), -1 for NULL. */
int pmg_laplacian_set_tensor_recompute_identity(pmg_laplacian op, int mode);
int pmg_laplacian_tensor_recomputed_identity(pmg_laplacian op);
/* One tensor per column where the Jacobian is constant in the column's direction (not in the reference).  Down a
 * column of a trilinear cell J depends on the column's coordinate through the cell's coefficients c101, c011, c111
 * alone.  Where they vanish -- the top face is a translate of the bottom face: boxes, tensor grids, octree cubes,
 * meshes extruded from arbitrary quadrilaterals -- adj(J) adj(J)^T / |det J| is the same in every layer and only the
 * layer's weight changes.  With the switch on, the kernels of the recomputed form at degrees 2 and 4 (the fused
 * restrictions (2, 1) and (4, 2) included; degree 1, with two layers per column, is left out by measurement) decide per
 * work item -- the cells one wavefront marches through together -- whether every
 * column's two slopes are exactly zero, and then form the tensor once per item instead of once per layer; every other
 * item runs the general march unchanged, so a mixed mesh takes both paths.  No promise from the caller and no second
 * array; same result to rounding.  It is wider than the affine mode, which stays opt-in and separate.
 * mode -1 (default): automatic -- on (profiles/column_tensor.md); 0: every item forms its tensor per layer; 1: on --
 * PMG_ERR_INVALID if the operator's next application does not recompute its tensor (the branch has no meaning
 * outside that form) or its degree is 1, nothing changes.  A request of -1 or 1 stands while the operator's state moves; it takes effect
 * whenever the apply recomputes.  PMG_COLUMN_TENSOR=0 / 1 in the environment, read at creation, sets mode 0 / 1
 * (without the error).  The choice is part of what a captured graph is keyed by.
 * pmg_laplacian_column_tensor: 1 if the next application runs the kernels with the branch, 0 if not, -1 for NULL.
 * pmg_laplacian_column_tensor_items: how many of the operator's work items qualify, and how many there are, counted
 * on the device with the kernels' own test; for an operator of degree 2 or 4 that has built the form's cell coefficients
 * (PMG_ERR_INVALID otherwise).  Allocates and reads back: not inside a stream capture. */
int pmg_laplacian_set_column_tensor(pmg_laplacian op, int mode);
int pmg_laplacian_column_tensor(pmg_laplacian op);
int pmg_laplacian_column_tensor_items(pmg_laplacian op, long long* qualifying, long long* total, pmg_stream stream);
/* Geometry batching (src/laplacian.hpp:383-396; examples/mat_free/main.cpp:34-50 --batch_size):
 * with batch_cells > 0 the tensor G is not kept; every application recomputes it for about
 * batch_cells cells at a time (rounded up to whole patches) into a buffer of that size, right
 * before the cells' stiffness launch -- the reference's memory / time trade, bit-identical
 * results.  0 (default) keeps G resident: 48 bytes per quadrature point, 1.57 GB for 64^3 cells of degree 4 (the
 * card has 288 GB).  pmg_laplacian_geometry_bytes
 * returns the size of the tensor buffer currently held. */
int pmg_laplacian_set_geometry_batch(pmg_laplacian op, long long batch_cells);
long long pmg_laplacian_geometry_bytes(pmg_laplacian op);
/* One operator application issues one stiffness-kernel launch per patch colour of the
 * interior cell list (8 on a structured box) plus one for the boundary list; on a small
 * level -- fewer patch dofs in the interior list than 2 M (degree 1) / 6 M (degree >= 2) --
 * the colours are merged into one launch that accumulates with atomics.
 * pmg_set_merge_threshold overrides that limit for operators created afterwards (0: always
 * coloured launches, a huge value: always merged, negative: the defaults above); process-wide,
 * for tests and tuning.
 *
 * Opt-in (PMG_APPLY_STREAMS=1 in the environment when the operator is created; =2 also on small levels, for tests):
 * the interior of a large level (>= 2048 patches, colours launched one by one) is cut in two halves whose colour
 * sequences run on two streams -- the caller's and one the operator owns, forked and joined with events; inside a stream
 * capture they become two branches of the graph -- so that each half fills the other's launch tails.  The halves share
 * dofs only across the cut; one event between the sequences orders those (patches.hip).  Off by default: the three
 * events per application cost more than the tails they hide (profiles/kernel_tuning_r04.md).
 * pmg_laplacian_apply_streams returns 1 or 2. */
int pmg_laplacian_launches_per_apply(pmg_laplacian op);
int pmg_laplacian_apply_streams(pmg_laplacian op);
/* Chain form of the interior launches (degree 4; csrc/patches.hpp ChainPlan, stiffness_chain_kernel): the interior
 * patches of a large level strung together along the axis with the fewest patch positions, one persistent workgroup
 * of sixteen wavefronts per chain; the gather of the next patch and the write-back of the previous one run under the
 * cell loop of the patch in hand, dofs shared by consecutive patches stay in LDS, a chain colour is one launch (four
 * on a box instead of eight patch colours).  Same sums as the patch launches to rounding.  Built when the operator is
 * created if PMG_CHAIN=1 (where every colour's chains fill the GPU) or =2 (whenever the patches form a tensor grid;
 * tests); PMG_CHAIN=0 never.  _chain_available: 1 if the operator has chains; _chain_form: 1 if they are in use;
 * _set_chain_form switches (PMG_ERR_INVALID when there are none).  The boundary cell list, merged small levels,
 * the affine mode and batched geometry keep the patch launches. */
int pmg_laplacian_chain_available(pmg_laplacian op);
int pmg_laplacian_chain_form(pmg_laplacian op);
int pmg_laplacian_set_chain_form(pmg_laplacian op, int on);
int pmg_set_merge_threshold(long long patch_dofs);
/* Dominant-kernel timing hook for bench.py: enqueue `reps` times every
 * stiffness-kernel launch of one operator application (no halo, no zero-fill)
 * bracketed by HIP events on `stream`; returns the mean milliseconds per launch
 * (= time per application / pmg_laplacian_launches_per_apply). */
int pmg_laplacian_time_kernel(pmg_laplacian op, const double* in, double* out, int reps,
                              double* ms_per_launch, pmg_stream stream);

/* In-situ timing of the same kernels where they run (inside a smoother, a V-cycle, a CG
 * iteration): while profiling is on, every run of stiffness-kernel launches an operator
 * application issues is bracketed by a pair of HIP events on the launch stream (a few
 * microseconds of host time per application -- leave it off in timed loops).
 * pmg_laplacian_read_profile waits for the recorded events, returns the summed milliseconds
 * and the number of stiffness launches they cover, and resets the record. */
int pmg_laplacian_set_profiling(pmg_laplacian op, int flag);
int pmg_laplacian_read_profile(pmg_laplacian op, double* total_ms, long long* launches);

/* ---- Chebyshev smoother (acc::Chebyshev, src/chebyshev.hpp:19-106) -------- */
int pmg_chebyshev_create(pmg_chebyshev* out, pmg_layout layout, double eig_min, double eig_max);
int pmg_chebyshev_destroy(pmg_chebyshev s);
int pmg_chebyshev_set_max_iterations(pmg_chebyshev s, int max_iter);
/* solve(A, x, b, verbose), :46-91.  x is in/out. */
int pmg_chebyshev_solve(pmg_chebyshev s, pmg_laplacian A, double* x, const double* b,
                        pmg_stream stream);
/* The recomputed form of a smooth of two or three steps: the residual is never stored, every operator product goes to
 * a vector of its own and each vector kernel forms what it needs from b, the products and the inverse diagonal -- three
 * passes over the level's vectors less per smooth, the same operator applications and launches, and the same
 * arithmetic: results equal the stored form's bit for bit.  It costs two more work vectors on the smoother, allocated
 * on first use.  mode: -1 automatic (the default: on levels of 4 Mi dofs and more, whose vectors are streamed), 0
 * never, 1 wherever it applies.  It applies to FP64 smooths on the matrix-free operator that return no residual or
 * feed the fused restriction, with coloured operator launches (no zeroed output) and no ghost bookkeeping; every
 * other smooth runs the stored loop whatever the mode.  The environment variable PMG_CHEB_RECOMPUTE=0|1 is read once,
 * by pmg_chebyshev_create, as the initial mode.  A multigrid's captured cycles are keyed on the mode. */
int pmg_chebyshev_set_recompute(pmg_chebyshev s, int mode);
/* Smooths of this smoother that have taken the recomputed form so far (a replayed graph counts what it captured). */
long long pmg_chebyshev_recomputed(pmg_chebyshev s);

/* ---- Jacobi-PCG + Lanczos eigenvalue estimate (acc::CGSolver, src/cg.hpp:93-250) */
int pmg_cg_create(pmg_cg* out, pmg_layout layout);
int pmg_cg_destroy(pmg_cg s);
int pmg_cg_set_max_iterations(pmg_cg s, int max_iter);
int pmg_cg_set_tolerance(pmg_cg s, double rtol);
int pmg_cg_store_coefficients(pmg_cg s, int flag);
/* solve(A, x, b), :147-222; *iterations receives the iteration count.  If
 * `precond` is non-NULL the V-cycle (zero initial guess) replaces the hard-wired
 * Jacobi preconditioner (not in the reference). */
int pmg_cg_solve(pmg_cg s, pmg_laplacian A, double* x, const double* b, pmg_multigrid precond,
                 int* iterations, pmg_stream stream);
/* Flexible variant (not in the reference): with a V-cycle preconditioner that is not a fixed
 * linear operator -- a Krylov coarse solver inside -- beta = r_new.(z_new - z_old) / r_old.z_old
 * keeps the recurrence residual honest.  No effect without `precond`. */
int pmg_cg_set_flexible(pmg_cg s, int flag);
/* Null space of the operator (not in the reference).  PMG_NULLSPACE_NONE (default): the iteration above.
 * PMG_NULLSPACE_CONSTANT: the operator has no Dirichlet row, no reaction and no Robin term, so A 1 = 0 -- the pure
 * Neumann problem.  With Pi = I - 1 1^T / N the solver runs r_0 = Pi (b - A x_0), z = M r,
 * rz = r . z - (1 . r)(1 . z) / N, p = Pi z + beta p, alpha = rz / (p . y), stops on rz / rz_0 as before and ends with
 * x <- Pi x: a right-hand side with a constant component is projected, not diverged on, and the result has zero mean.
 * An iteration issues the launches of the plain one and reads no vector an extra time (the three sums come out of one
 * pass, the shift is applied inside the direction kernel).  What a solve adds: the projection of r_0, the final
 * projection of x, and one first-direction kernel (z_0 is formed beside r and p_0 = Pi z_0 written from it, where the
 * plain loop preconditions straight into p).  Works with pmg_cg_set_flexible and with pmg_cg_solve_matrix; a solver installed with
 * pmg_multigrid_set_coarse_solver honours its own mode.  Refused with PMG_ERR_INVALID (message in pmg_last_error): an
 * unknown mode, here; a solve with the mode on and an operator that has a marked row (on any rank), a reaction term
 * or a Robin term.  pmg_cg_nullspace returns the mode. */
#define PMG_NULLSPACE_NONE 0
#define PMG_NULLSPACE_CONSTANT 1
int pmg_cg_set_nullspace(pmg_cg s, int mode);
int pmg_cg_nullspace(pmg_cg s);
/* alphas()/betas(), :118-119; returns the number stored. */
int pmg_cg_coefficients(pmg_cg s, double* alphas, double* betas, int capacity);
/* compute_eigenvalues(), :121-142: sorted ascending; returns the count or <0. */
int pmg_cg_compute_eigenvalues(pmg_cg s, double* eigs, int capacity);
int pmg_cg_residual(pmg_cg s, double* rnorm);

/* ---- assembled operator (acc::MatrixOperator, src/csr.hpp:58-131,205-260) ----
 * The BC-treated stiffness matrix in CSR on the device, applied by SpMV: the second operator type behind the
 * reference's interface (examples/pmg/main.cpp:69,285,457-458 solve<MatrixOperator>; examples/cg/main.cpp:224;
 * examples/mat_free/main.cpp:270-288 --mat_comp; test/test_csr.cpp).
 *
 * pmg_matrix_create_from_laplacian restates MatrixOperator(a, bcs), src/csr.hpp:66-131, from what the operator
 * already holds -- its own (ascending) copy of the dofmap, the stored geometry tensor, the caller's kappa and BC
 * marker -- so the matrix lives in the operator's dof numbering and the cell-local node order the operator was
 * created with does not change it.
 *   pattern: dolfinx's create_sparsity_pattern (:76-77) -- row i couples to every dof that shares a cell with i --,
 *            columns sorted within a row, int32 indices, built once on the host.  Dirichlet rows and columns stay in
 *            the pattern as explicit zeros with a unit diagonal (:84-86), so nnz equals the reference's.
 *   values:  one HIP kernel evaluates the element matrices in closed form and sums them row by row (a sub-wavefront
 *            per row gathers from the cells incident to the row: no atomics, two assemblies give the same bits).
 * kappa is read at ASSEMBLY time only (unlike pmg_laplacian_apply, which reads it in every application):
 * pmg_matrix_update_values re-evaluates the values and the inverse diagonal on the existing pattern.  The geometry
 * mode (affine cells) and the chain form of the operator do not matter: assembly always reads the stored tensor.
 * `op` must outlive the matrix.  Degrees 1..PMG_MAX_DEGREE.
 * Refused with PMG_ERR_INVALID (message in pmg_last_error; *out stays NULL): a layout with ghosts or a communicator
 * (single-domain only; the distributed diag / off-diag form of :114-126 is a follow-up), an operator in
 * batched-geometry mode (G is not resident), a pattern whose nnz does not fit int32 (the message states the nnz).
 * (This entry point keeps its single-domain contract; pmg_matrix_create_distributed below takes any layout.) */
int pmg_matrix_create_from_laplacian(pmg_matrix* out, pmg_laplacian op, pmg_stream stream);
/* The same matrix on ANY layout, several ranks included (the reference's operator is distributed by construction,
 * src/csr.hpp:114-126,252-270).  On a layout without ghosts and without a communicator the arrays are those of
 * pmg_matrix_create_from_laplacian.
 *   rows:    the size_local owned dofs.  A ghost dof is a column, never a row.
 *   columns: local indices in [0, size_local + num_ghosts), sorted, so the ghost columns of a row come last.
 *   pattern: row i couples to every dof of every local cell, ghost cells included, that contains i.  Every rank holds
 *            the ghost-cell layer, so its owned rows are complete locally: no matrix value is exchanged.  Dirichlet
 *            rows and columns (ghost columns included) stay as explicit zeros with a unit diagonal.
 *   split:   off_diag_offset[i] = the position of row i's first column >= size_local (the reference's array), and the
 *            ascending list of the boundary rows, the rows with at least one ghost column (pmg_matrix_export_split).
 * The product is scatter begin / owned columns of all rows / scatter end / ghost columns of the boundary rows; a level
 * whose operator takes its exchange whole (halo windows, merged plan) does so here as well, in front of one launch.
 * The remaining refusals are those above: batched geometry, nnz above int32, a row that does not fit LDS. */
int pmg_matrix_create_distributed(pmg_matrix* out, pmg_laplacian op, pmg_stream stream);
int pmg_matrix_destroy(pmg_matrix M);
int pmg_matrix_update_values(pmg_matrix M, pmg_stream stream);
/* operator()(x, y), src/csr.hpp:220-260: out = A in; the owned entries of `out` are overwritten (no zero-fill needed).
 * No transpose variant: the operator is symmetric.  On a distributed matrix the call exchanges the halo of `in`: it
 * REFRESHES THE GHOST ENTRIES OF `in` (the const of the signature covers the owned entries only) and leaves the ghost
 * entries of `out` alone.  Collective over the layout's ranks. */
int pmg_matrix_apply(pmg_matrix M, const double* in, double* out, pmg_stream stream);
/* The same product where the ghost entries of `in` are current already (the caller has exchanged them): no exchange,
 * ONE launch over whole rows; `in` is not written.  What the V-cycle issues for the first product of a post-smooth.  On
 * a matrix without ghost columns this is pmg_matrix_apply. */
int pmg_matrix_apply_ghosts_current(pmg_matrix M, const double* in, double* out, pmg_stream stream);
/* get_diag_inverse, src/csr.hpp:100-110,205-209: the owned entries; BC rows give 1. */
int pmg_matrix_get_diag_inverse(pmg_matrix M, double* diag_inv, pmg_stream stream);
/* num_rows and nnz of src/csr.hpp:91-93 (the reference's nnz() accessor); device bytes held by the handle. */
long long pmg_matrix_rows(pmg_matrix M);
long long pmg_matrix_cols(pmg_matrix M); /* size_local + num_ghosts */
long long pmg_matrix_nnz(pmg_matrix M);
long long pmg_matrix_bytes(pmg_matrix M);
/* The "A norm" logged at src/csr.hpp:95-99: sqrt(sum of squared values), over all ranks (every owned row lives on
 * exactly one rank; the local sum of squares goes through the layout's all-reduce: collective). */
int pmg_matrix_frobenius_norm(pmg_matrix M, double* norm);
/* Host copy of the device arrays the reference uploads at src/csr.hpp:114-130 (tests): this rank's rows with local
 * column numbers.  NULL arrays: sizes only. */
int pmg_matrix_export(pmg_matrix M, long long* rows, long long* nnz, int32_t* row_ptr, int32_t* cols, double* values);
/* ... and the split: off_diag_offset[rows] (positions in cols) and boundary_rows[*n_boundary_rows], ascending.  NULL
 * arrays: sizes only.  A matrix on a layout without ghosts has off_diag_offset[i] = row_ptr[i + 1] and no boundary
 * row. */
int pmg_matrix_export_split(pmg_matrix M, int32_t* off_diag_offset, long long* n_boundary_rows, int32_t* boundary_rows);
/* Chebyshev::solve / CGSolver::solve with an acc::MatrixOperator as the operator (src/chebyshev.hpp:46-91,
 * src/cg.hpp:147-222 are templated on it): the semantics of pmg_chebyshev_solve / pmg_cg_solve with the matrix's
 * product and the matrix's own inverse diagonal. */
int pmg_chebyshev_solve_matrix(pmg_chebyshev s, pmg_matrix M, double* x, const double* b, pmg_stream stream);
int pmg_cg_solve_matrix(pmg_cg s, pmg_matrix M, double* x, const double* b, pmg_multigrid precond, int* iterations,
                        pmg_stream stream);

/* ---- p-transfer (Interpolator<T>, src/interpolate.hpp:93-329) -------------
 * Coarse (Q1) and fine (Q2) spaces on the same cells; dofmaps as for the
 * operator; lcells/bcells as there. */
int pmg_interpolator_create(pmg_interpolator* out, pmg_layout layout_coarse,
                            pmg_layout layout_fine, int degree_coarse, int degree_fine,
                            int32_t ncells, const int32_t* dofmap_coarse,
                            const int32_t* dofmap_fine, const int32_t* lcells, int32_t n_lcells,
                            const int32_t* bcells, int32_t n_bcells, pmg_stream stream);
/* Same, sharing the cell patches (grouping, colours, launch order) of the
 * fine-level operator: both transfers then run one workgroup per patch with LDS
 * accumulation -- no global atomics, no zero-fill -- and the prolongation can be
 * fused with the correction.  fine_operator may be NULL (== pmg_interpolator_create);
 * otherwise it must outlive the interpolator, which reads its patch tables. */
int pmg_interpolator_create_with_operator(pmg_interpolator* out, pmg_layout layout_coarse,
                                          pmg_layout layout_fine, int degree_coarse,
                                          int degree_fine, int32_t ncells,
                                          const int32_t* dofmap_coarse, const int32_t* dofmap_fine,
                                          const int32_t* lcells, int32_t n_lcells,
                                          const int32_t* bcells, int32_t n_bcells,
                                          pmg_laplacian fine_operator, pmg_stream stream);
/* The same with both dofmaps in the caller's cell-local node order (see "cell-local node order"; the
 * reference's Interpolator receives the dofmaps of two basix tensor-product spaces, src/interpolate.hpp:104-107,
 * and its operator from basix::compute_interpolation_operator in that order, :118).  custom_* [degree + 1] only for
 * PMG_NODES_CUSTOM.  fine_operator may be NULL; if given, it may have been created in any node order. */
int pmg_interpolator_create_ordered(pmg_interpolator* out, pmg_layout layout_coarse, pmg_layout layout_fine,
                                    int degree_coarse, int degree_fine, int32_t ncells,
                                    const int32_t* dofmap_coarse, const int32_t* dofmap_fine,
                                    const int32_t* lcells, int32_t n_lcells, const int32_t* bcells,
                                    int32_t n_bcells, pmg_laplacian fine_operator, int node_order,
                                    const int32_t* custom_coarse, const int32_t* custom_fine, pmg_stream stream);
int pmg_interpolator_destroy(pmg_interpolator ip);
/* interpolate(Q1_vector, Q2_vector), :186-239: prolongation, updates the ghosts of `coarse`. */
int pmg_interpolator_interpolate(pmg_interpolator ip, double* coarse, double* fine,
                                 pmg_stream stream);
/* fine += P coarse in one pass: interpolate + the axpy of src/pmg.hpp:123-129
 * (only for interpolators created with an operator). */
int pmg_interpolator_interpolate_add(pmg_interpolator ip, double* coarse, double* fine,
                                     pmg_stream stream);
/* reverse_interpolate(Q2_vector, Q1_vector), :246-303: restriction (multiplicity-
 * weighted transpose), updates the ghosts of `fine`, zeroes `coarse` first. */
int pmg_interpolator_reverse_interpolate(pmg_interpolator ip, double* fine, double* coarse,
                                         pmg_stream stream);
/* coarse = R (r - A z) in ONE kernel (not in the reference): the application of the fine-level operator `op` to z
 * and the restriction of the residual it would feed, fused -- A z is never written, `coarse` is overwritten (it is
 * zero-filled first and does not depend on its old contents), no fine vector is written.  The restriction is additive
 * over cells for conforming spaces, so every patch workgroup of the apply restricts its cells' own contributions
 * (r / multiplicity - A_cell z; on Dirichlet rows, where the apply sets (A z)_i = z_i, (r - z) / multiplicity) and all
 * patches run in one launch without colours.  Same value as pmg_laplacian_apply followed by the restriction of the
 * difference, to rounding.  It counts as one application of `op` (pmg_multigrid_apply_counts) and is not part of the
 * stiffness profile (pmg_laplacian_read_profile keeps describing the plain kernel).
 * Available -- otherwise PMG_ERR_INVALID with a message -- only where ALL of these hold:
 *   - `ip` was created with `op` as its fine operator (patch form: pmg_interpolator_create_with_operator);
 *   - the fine layout has no ghosts;
 *   - the geometry of `op` is resident (pmg_laplacian_set_geometry_batch(op, 0));
 *   - the degree pair (coarse, fine) is one of 1-2, 2-4, 1-3, 3-6 (the shared-item degrees 5 and 8 are not covered).
 * Kappa, the coefficient field, the affine mode and the cache policy work as in pmg_laplacian_apply. */
int pmg_interpolator_restrict_residual(pmg_interpolator ip, pmg_laplacian op, const double* z, const double* r,
                                       double* coarse, pmg_stream stream);
/* The two transfers of the FP32 V-cycle (pmg_multigrid_set_precision) on float device arrays of the layouts' sizes:
 * fine += P coarse, and coarse = R (fine - fine_sub) (`coarse` is overwritten; fine_sub may be NULL: coarse = R fine).
 * The float copy of the 1-D table is built on the first FP32 use and freed with the interpolator.  Refused with
 * PMG_ERR_INVALID: an interpolator created without an operator, a layout with ghosts or a communicator. */
int pmg_interpolator_interpolate_add_f32(pmg_interpolator ip, const float* coarse, float* fine, pmg_stream stream);
int pmg_interpolator_reverse_interpolate_f32(pmg_interpolator ip, const float* fine, const float* fine_sub,
                                             float* coarse, pmg_stream stream);

/* ---- V-cycle (acc::MultigridPreconditioner, src/pmg.hpp:16-184) -----------
 * Levels are ordered coarse -> fine like the reference's vectors.  The handle
 * allocates its own work vectors (:35-41).  coarse solve = smoother[0] unless
 * pmg_multigrid_set_coarse_solver is used (:106-109). */
int pmg_multigrid_create(pmg_multigrid* out, int nlevels, const pmg_layout* layouts,
                         const int8_t* bc_marker_coarsest);
int pmg_multigrid_destroy(pmg_multigrid mg);
int pmg_multigrid_set_operators(pmg_multigrid mg, const pmg_laplacian* ops);          /* :48 */
int pmg_multigrid_set_solvers(pmg_multigrid mg, const pmg_chebyshev* smoothers);      /* :44 */
int pmg_multigrid_set_interpolators(pmg_multigrid mg, const pmg_interpolator* interp); /* :50-53 */
/* set_coarse_solver, :46,106-109: the coarsest level is solved by `coarse` -- pmg_cg_solve on
 * operator[0] from a zero initial guess with the solver's own iteration cap and tolerance --
 * instead of smoother[0]; NULL restores the smoother.  The reference's coarse solver is a Krylov
 * solve too (PETSc KSPCG, at most 60 iterations, src/amg.hpp:36-44) but preconditioned by hypre
 * BoomerAMG, third-party arithmetic that is out of scope here: the library's CG is
 * Jacobi-preconditioned.  `coarse` must live on the coarsest layout and outlive `mg`. */
int pmg_multigrid_set_coarse_solver(pmg_multigrid mg, pmg_cg coarse);
/* The same hook for ANY coarse solver -- the reference's CoarseSolver concept is "a type with
 * solve(Vector& x, Vector& b)" (src/amg.hpp:67, called at src/pmg.hpp:106-107): `solve` receives
 * the coarsest-level solution (zeroed beforehand) and right-hand side as device arrays of
 * size_local + num_ghosts doubles and the stream the cycle runs on; it returns 0 on success.
 * NULL restores the smoother.  (pmg_amg below is the library's own such solver.) */
typedef int (*pmg_coarse_solve_fn)(void* user, double* x, double* b, pmg_stream stream);
int pmg_multigrid_set_coarse_callback(pmg_multigrid mg, pmg_coarse_solve_fn solve, void* user);
/* ---- algebraic multigrid for the coarsest level (the role of CoarseSolverType<T>, src/amg.hpp) ----
 * The reference solves its degree-1 level with PETSc KSPCG (<= 60 iterations, default relative
 * tolerance 1e-5) preconditioned by hypre BoomerAMG (src/amg.hpp:33-47).  Those are third-party;
 * pmg_amg is the library's own solver for that slot: smoothed-aggregation AMG on the assembled
 * degree-1 matrix (built on the host from the operator's geometry tensor; cycles run on the device
 * with the same Chebyshev/Jacobi smoother as the p-levels), used either
 *   - Krylov mode (default, the reference's shape): CG on the matrix-free operator preconditioned
 *     by one AMG V-cycle, zero initial guess, max_iter / rtol as set (60, 1e-5); or
 *   - stationary mode (pmg_amg_set_cycles(n > 0)): n AMG V-cycles from a zero initial guess -- a
 *     fixed linear operator without host synchronisation (single rank only).
 * `op` must be a degree-1 operator and outlive the solver.
 * Several ranks: pmg_amg_create builds the hierarchy of the rank's own block (a block preconditioner
 * for the Krylov mode; iteration counts grow with the number of ranks).  pmg_amg_create_replicated
 * gathers the owned rows of all ranks -- `global_index` [size_local + num_ghosts] (host) is the global
 * number of every local dof, dolfinx's IndexMap::local_to_global; n_global < 2^31 -- into the global
 * matrix on every rank: a solve is then one all-reduce of the zero-padded right-hand side (on the
 * layout's communicator, or through its allreduce callback) and the single-rank solve of the whole
 * coarse problem on every rank; both modes work, with one rank's iteration counts.  Collective. */
int pmg_amg_create(pmg_amg* out, pmg_laplacian op, pmg_stream stream);
int pmg_amg_create_replicated(pmg_amg* out, pmg_laplacian op, const int64_t* global_index, int64_t n_global,
                              pmg_stream stream);
/* The same solver set up WITHOUT gathering the global degree-1 matrix (round 4): every rank aggregates its owned
 * dofs on its own block (ghost couplings lumped), smooths its prolongator rows with that block, obtains the prolongator
 * rows of its ghost dofs through the layout's own forward scatter (one layer of overlap; any exchange mechanism),
 * forms its rows of P^T A P, and only level 1 -- about 1/9 of level 0 -- is gathered and coarsened further on every
 * rank.  The solve is the replicated form's with the distributed fine level (level 0 smoothed on the partitioned
 * operator, one all-reduce of a level-1 vector per cycle); pmg_amg_set_distributed_fine_level(amg, 0) is refused.
 * The hierarchy depends on the partition (aggregates do not cross rank boundaries); iteration counts stay within one
 * of the gathered (= single-rank) hierarchy's: 10 against 10 on eight ranks of 64^3 cells
 * (tools/amg_setup_scaling.py), where the rank-local block preconditioner of pmg_amg_create takes 40.  Collective. */
int pmg_amg_create_distributed(pmg_amg* out, pmg_laplacian op, const int64_t* global_index, int64_t n_global,
                               pmg_stream stream);
int pmg_amg_destroy(pmg_amg amg);
int pmg_amg_set_smoother_iterations(pmg_amg amg, int k); /* Chebyshev degree per pre/post smooth (2) */
int pmg_amg_set_cycles(pmg_amg amg, int cycles);
int pmg_amg_set_krylov(pmg_amg amg, int max_iter, double rtol);
/* Replicated form only.  1 (the default when the hierarchy has more than one level): level 0 of the hierarchy -- the
 * degree-1 level itself, three quarters of a cycle's work -- is smoothed on the PARTITIONED operator (matrix-free
 * application with its halo exchange), each rank restricts its owned residual, ONE all-reduce of a level-1 vector
 * (about 1/9 of the level-0 size) forms the replicated right-hand side of level 1, and only the levels from 1 down are
 * solved redundantly on every rank.  0: the whole hierarchy replicated, one all-reduce of a level-0 vector per solve
 * (the redundant work then grows with the rank count).  Same arithmetic up to summation order either way. */
int pmg_amg_set_distributed_fine_level(pmg_amg amg, int enable);
/* Null space of the degree-1 operator (PMG_NULLSPACE_NONE, the default, or PMG_NULLSPACE_CONSTANT; single-domain
 * hierarchies only).  The set-up is untouched -- pmg_amg_export returns the same bytes either way.  With the mode on:
 *   - the coarsest level is inverted as A_c + gamma v v^T, v = P_{L-2}^T ... P_0^T 1 the ones restricted through the
 *     hierarchy's own transfers (v = 1 on a hierarchy of one level) and gamma = max diag(A_c) / (v^T v): the exact
 *     solve of every coarse right-hand side a mean-free residual restricts to, and a rank-one SPD perturbation where
 *     the level is only nearly singular.  A Cholesky factorisation that fails is PMG_ERR_NUMERIC, not a fall back to
 *     smoothing; a coarsest level too large to invert keeps smoothing;
 *   - pmg_amg_cycle and the stationary solve end with x <- x - mean(x), on the device (capturable);
 *   - the Krylov mode runs its CG with PMG_NULLSPACE_CONSTANT.
 * Setting PMG_NULLSPACE_NONE restores the plain inverse.  Refused with PMG_ERR_INVALID: an unknown mode, a replicated
 * or distributed hierarchy, an operator with marked rows, a reaction term or a Robin term -- here, and again by
 * pmg_amg_solve and pmg_amg_cycle while the mode is on (a term attached to the operator afterwards is refused, not
 * projected). */
int pmg_amg_set_nullspace(pmg_amg amg, int mode);
int pmg_amg_nullspace(pmg_amg amg);
/* solve(x, b) of src/amg.hpp:67-68; *iterations = CG iterations (or cycles) used. */
int pmg_amg_solve(pmg_amg amg, double* x, const double* b, int* iterations, pmg_stream stream);
/* One V-cycle of the hierarchy from a zero initial guess: x = M b (the preconditioner alone). */
int pmg_amg_cycle(pmg_amg amg, double* x, const double* b, pmg_stream stream);
int pmg_amg_num_levels(pmg_amg amg);
int pmg_amg_level_info(pmg_amg amg, int level, long long* rows, long long* nnz, double* lambda_max);
/* Host copy of the hierarchy (tests): which = 0 the matrix of `level`, 1 the prolongator from
 * level + 1 to `level`; CSR.  Call with NULL arrays first to learn the sizes. */
int pmg_amg_export(pmg_amg amg, int level, int which, long long* rows, long long* cols, long long* nnz,
                   int32_t* rowptr, int32_t* colidx, double* values);
/* Renew the hierarchy in place after the operator's data changed (pmg_laplacian_set_coefficient_field, _tensor,
 * set_reaction, set_robin): every value -- A_0 from the operator's stored tensor, kappa, the marker and the diagonal
 * vector; per level the inverse diagonal, the bound 1.05 x 20 power steps, P_l = (I - 4/(3 rho_l) D^-1 A_l) T_l, its
 * transpose, A_l P_l and A_{l+1} -- is recomputed on the device; the coarsest inverse (both, with the null-space mode
 * on) is the host's Cholesky of the downloaded A_c, uploaded in place.  The aggregates, the tentative weights and the
 * level sizes stay those of the creation, and so does the handle: a multigrid object keeps it (its cached V-cycle
 * graphs re-capture: the bounds are kernel arguments).  The first call plans on the host: the structural patterns of
 * P_l (every aggregate that an entry of the row of A_l reaches which some coefficient can make non-zero, stored zeros
 * of the current values included -- the created P_l stores no exact zero, so its pattern depends on the coefficient it
 * was created for; left out are only the entries of A_0 between the two ends of a cell's body diagonal, which no
 * quadrature point couples), of its transpose and of the two products on the stored patterns; a level whose structural pattern is larger than the created one gets new device arrays, and a scratch copy
 * of the tensor (48 doubles per cell) is kept.  Later calls allocate nothing.  Sums are in a fixed order and there are
 * no atomics: two updates from the same data give the same bytes.  Afterwards pmg_amg_level_info reports the new
 * bounds and the structural entry counts, pmg_amg_export downloads the current values on the structural patterns
 * (explicit zeros are possible) and pmg_amg_updates is one higher.  Refused with PMG_ERR_INVALID, nothing touched:
 * NULL; a replicated or distributed hierarchy or a layout with several ranks; an operator in batched-geometry mode;
 * a row of a product longer than the 8192 entries of the kernels' row copy (first call); a call inside a stream
 * capture -- the call synchronises the stream.  A level without a positive diagonal returns PMG_ERR_NUMERIC naming
 * the level; pmg_amg_solve and pmg_amg_cycle then refuse the hierarchy until an update succeeds.  The p-levels'
 * smoother bounds and pmg_laplacian_compute_diag_inverse stay the caller's business. */
int pmg_amg_update_values(pmg_amg amg, pmg_stream stream);
/* successful pmg_amg_update_values calls since the creation (0 after it); -1 for NULL */
long long pmg_amg_updates(pmg_amg amg);
/* set_coarse_solver (src/pmg.hpp:46) with the library's AMG; NULL restores the smoother. */
int pmg_multigrid_set_coarse_amg(pmg_multigrid mg, pmg_amg amg);

/* apply(x = rhs, y = initial guess in / result out, verbose), :56-155.  If
 * rnorm is non-NULL the final residual norm ||b - A y|| is computed (the
 * reference prints it when verbose, :147-150) -- this costs one extra apply and a
 * host synchronisation. */
int pmg_multigrid_apply(pmg_multigrid mg, const double* rhs, double* y, double* rnorm,
                        pmg_stream stream);
/* Exchanges of a cycle on several ranks: every operator application refreshes the ghosts of its input
 * (src/laplacian.hpp:378,425) -- except the first application of a post-smooth when the transfers share the operator's
 * patches: the iterate leaves its pre-smooth with current ghosts (the smoother adds the ghost entries of every applied
 * correction), the prolongation computes the coarse correction on the ghost cells too, so u + P u_c has current ghosts
 * without an exchange of its own.  Three levels, Chebyshev(3): 17 exchanges per cycle instead of 19.
 * PMG_LOCAL_CORRECTION=0 in the environment restores one exchange per application. */
/* hipGraph replay of the cycle.  enable > 0: pmg_multigrid_apply (and the V-cycle preconditioner inside
 * pmg_cg_solve) captures the cycle's ~120 launches into a graph the first time it sees a (rhs, y) pair and replays it
 * afterwards with one hipGraphLaunch on the caller's stream: same kernels, same order, same results.  enable == 0:
 * never.  enable < 0, the default: automatic -- on one rank eager (the launches run ahead of the GPU anyway: a replay
 * buys nothing), on several ranks replayed wherever the capture holds nothing but kernels (every exchange through halo
 * windows, the cycle's reductions through a communicator made of windows), because an eager exchange costs the host
 * more than the GPU; a cycle whose exchanges are RCCL calls is replayed on request only (enable > 0, or
 * PMG_GRAPH_AUTO=rccl in the environment; PMG_GRAPH_AUTO=0 turns the automatic choice off): that capture has run on
 * one GPU, never between two.
 * Captured only when nothing in the cycle needs the host: no exchange callbacks, no Krylov / callback coarse solver, no
 * in-situ profiling; otherwise the call runs eagerly as before.  Layouts with a pmg_comm ARE captured: the grouped
 * send / receive of every halo exchange is recorded into the graph (on a HIP >= 7.2 runtime as a parallel branch that
 * keeps its overlap with the interior cells, pmg_comm_capture_overlaps).  A change of a smoother's iteration count or
 * bound, of a geometry mode or of the coarse solver is noticed (new graph); calling this function again drops the
 * cached graphs (do that after replacing an operator's diagonal or any caller-owned array in place). */
int pmg_multigrid_set_graph(pmg_multigrid mg, int enable);
long long pmg_multigrid_graph_replays(pmg_multigrid mg);
/* Number of stiffness-kernel launches issued by the last pmg_multigrid_apply,
 * per level (coarse -> fine); for the byte accounting in bench.py. */
int pmg_multigrid_apply_counts(pmg_multigrid mg, int* counts, int capacity);
/* Restriction fused into the pre-smooth's last application (pmg_interpolator_restrict_residual).  mode -1, the
 * default: automatic -- on every level below whose transfer the fused form is available (see there) and which has no
 * level matrix (pmg_multigrid_set_level_matrix), the FP64 cycle does not issue the pre-smooth's last A z nor the
 * restriction of r - A z but the one fused kernel; a smoother of one iteration keeps its own path.  Everywhere else --
 * layouts with ghosts, batched geometry, other degree pairs, interpolators without patches, the FP32 cycle -- the cycle
 * runs exactly as without this switch.  mode 0: never.  The mode is part of the graph key and setting it drops the
 * cached graphs.  Results agree with the unfused cycle to rounding; pmg_multigrid_apply_counts is the same in both.
 * pmg_multigrid_fused_restrictions: how many fused kernels the last pmg_multigrid_apply issued (levels - 1 at most). */
int pmg_multigrid_set_fused_restriction(pmg_multigrid mg, int mode);
int pmg_multigrid_fused_restrictions(pmg_multigrid mg);
/* Precision of the cycle (not in the reference).  PMG_PRECISION_FP64 (default): everything in FP64, as above.
 * PMG_PRECISION_FP32: every later pmg_multigrid_apply, and the V-cycle preconditioner inside pmg_cg_solve, runs the
 * smoothers, operators (pmg_laplacian_apply_f32) and transfers of every level in FP32; rhs and y stay double.
 *   - zero initial guess (the preconditioner): y = V32(rhs) converted to double;
 *   - non-zero y (stationary cycles): defect correction, y += V32(rhs - A y) with the FP64 operator forming the
 *     defect -- equal to the FP64 cycle to float rounding, so repeated cycles converge below float accuracy;
 *   - a coarse AMG / CG / callback solver keeps running in FP64 (b_0 converted up, u_0 down); the smoother-only coarse
 *     level runs in FP32;
 *   - smoother bounds and iteration counts are the pmg_chebyshev objects'; the float Jacobi diagonal is a copy of the
 *     operator's diag_inv, refreshed after pmg_laplacian_set_diag_inverse / _compute_diag_inverse;
 *   - graph replay (pmg_multigrid_set_graph) works as in FP64, the precision is part of the graph's key.
 * Switching precision drops the cached graphs.  Refused with PMG_ERR_INVALID (message in pmg_last_error): an unknown
 * precision; FP32 when a level's layout has ghosts or a communicator (single-domain only), an interpolator is not in
 * patch form (pmg_interpolator_create_with_operator), or an operator is in batched-geometry mode -- checked here and
 * again by each FP32 cycle.  pmg_multigrid_precision returns the current mode. */
#define PMG_PRECISION_FP64 0
#define PMG_PRECISION_FP32 1
int pmg_multigrid_set_precision(pmg_multigrid mg, int precision);
/* set_operators with acc::MatrixOperator levels (src/pmg.hpp:48 in solve<MatrixOperator>,
 * examples/pmg/main.cpp:285,348-355), one opt-in switch per level: every operator application the cycle issues on
 * `level` -- the smoother's, and whatever forms that level's residual -- becomes the matrix's product with the
 * matrix's inverse diagonal; NULL removes the matrix again.  The level's pmg_laplacian stays attached and the
 * transfers keep running on its patches.  pmg_multigrid_apply_counts keeps counting applications per level whichever
 * form ran them.  The set of level matrices is part of the graph key (a cached graph is never replayed after it
 * changes).  Refused with PMG_ERR_INVALID: a matrix on another layout than the level's; a matrix together with
 * PMG_PRECISION_FP32, in either order (there is no FP32 matrix).  A coarse AMG / CG / callback solver is unaffected.
 * On a level of several ranks `M` is a distributed matrix (pmg_matrix_create_distributed); the cycle's exchange
 * bookkeeping then holds as on a matrix-free level: where the iterate's ghosts are current the post-smooth's first
 * product runs without an exchange, so a cycle issues the same number of forward scatters in either form.
 * `M` must outlive `mg` or be removed first. */
int pmg_multigrid_set_level_matrix(pmg_multigrid mg, int level, pmg_matrix M);
int pmg_multigrid_precision(pmg_multigrid mg);

#ifdef __cplusplus
}
#endif
#endif /* PMG_AMD_H */
