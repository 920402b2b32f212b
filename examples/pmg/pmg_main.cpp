// p-multigrid driver: the MI355X counterpart of the reference's examples/pmg/main.cpp:solve
// (:41-380), written against the reference's own type spellings through include/pmg_amd.hpp
// (PMG_AMD_DOLFINX_NAMESPACE): the smoother set-up, interpolators, V-cycle wiring and the cycle loop
// below are the reference's lines :306-365; what stands above them replaces dolfinx (mesh, function
// spaces, index maps, load vector).  Defaults are BASELINE config 2: 64^3 hexes, degrees 1,2,4,
// Chebyshev(3).  Per level: operator (:270-272), matrix-free inverse diagonal (replaces the CSR
// assembly of :274-279), load vector of f = -div(kappa grad(sin 2 pi x sin 3 pi y sin 4 pi z)) / kappa
// sampled at the GLL nodes (examples/pmg/poisson.py:6-8,30,35-40; :289-300).
//
//   --amg            coarse solver on the degree-1 level (:331-335): CG <= 60 iterations, rtol 1e-5,
//                    preconditioned by the library's algebraic multigrid (hypre's role)
//   --amg-cycles N   the same hierarchy as N stationary AMG cycles instead of the Krylov solve
//   --amg-renew      (implies --amg) the AMG is created on the degree-1 operator BEFORE --kappa-field, --kappa-tensor,
//                    --reaction and --robin are applied to it and renewed in place after them (pmg_amg_update_values);
//                    one line reports levels, rows and the renewal's milliseconds; everything else as without the flag
//   --csr [LEVELS]   the listed levels (comma-separated indices; default all) as assembled CSR matrices
//   --coarse-cg      Jacobi-preconditioned CG (60 iterations) as the coarse solver
//   --pcg            additionally solve with CG preconditioned by the cycle (random right-hand side
//                    with --random-rhs)
//   --ranks px,py,pz one process per GPU and brick (the reference runs under mpirun -n 8,
//                    examples/pmg/submit.sh:29): halo exchange and reductions on the library's RCCL
//                    communicator.  Rank and world size come from --rank / RANK (OMPI_COMM_WORLD_RANK,
//                    PMI_RANK); the GPU from LOCAL_RANK; rank 0 publishes the communicator id in
//                    --id-file.  examples/pmg/run_ranks.sh launches the processes.
//   --graph          time the cycles as hipGraph replays (one launch per cycle; with --ranks the grouped send/recv of
//                    every halo exchange are captured on the compute stream: no host work per exchange)
//   --fp32-cycle     run the V-cycle's smoothers, operators and transfers in FP32 (pmg_multigrid_set_precision); the
//                    stationary cycles, PCG and residuals stay FP64.  Single domain only: refused with --ranks
//   --kappa-field    the smooth nodal coefficient 1 + 0.5 sin(2 pi x) cos(2 pi y) + z on every level
//   --kappa-tensor   a per-cell diffusion tensor on every level: eigenvalues (1, 2 + x, 4), rotated by
//                    Rz(0.6 + 0.8 y) Rx(0.4 + 0.5 z) at the cell centre (pmg_laplacian_set_coefficient_tensor);
//                    combines with --kappa-field, --amg, --pcg, --fp32-cycle, --csr
//   --robin A        a Robin boundary K grad u . n + alpha u = 0 on every level: the Dirichlet marker is kept on the
//                    face x = 0 only, the other five faces carry alpha = A (1 + y) at their facet points
//                    (pmg_laplacian_set_robin); combines with every flag --reaction combines with, and with it
//   --reaction S     the reaction term sigma u on every level, sigma_c = S (1 + x_c) at the cell centre
//                    (pmg_laplacian_set_reaction); combines with --kappa-field, --kappa-tensor, --amg, --pcg,
//                    --fp32-cycle, --csr
//   --curved G       the box bent by a fixed smooth map (examples/common/box_mesh.hpp: curved_map) with a coordinate
//                    element of degree G = 1..4 (pmg_laplacian_create_curved); G = 1: the straight-sided mesh through
//                    the mapped vertices.  The data of the other flags stay functions of the box coordinates;
//                    combines with --kappa-field, --kappa-tensor, --reaction, --robin, --fp32-cycle, --csr, --amg, --pcg
//   --neumann        the pure Neumann problem: no Dirichlet marker on any level, the load made compatible with
//                    acc::remove_mean, the constant null space set on the outer CG, the coarse CG and the AMG
//                    (pmg_cg_set_nullspace / pmg_amg_set_nullspace).  On the undeformed unit box with constant
//                    coefficient the load is that of u = cos pi x cos pi y cos pi z (zero normal derivative on every
//                    face, zero mean) and --pcg prints the largest nodal error after removing the lumped-mass mean.
//                    Combines with --kappa-field, --kappa-tensor, --curved, --fp32-cycle, --csr, --graph, --amg-cycles;
//                    refused with --reaction or --robin (the operator is then not singular) and with --amg on
//                    several ranks
//   --check-partition px,py,pz   host-only consistency check of the brick partition (no GPU)
//   --node-order basix   the dofmaps handed over in basix's cell-local node order (endpoints first), as dolfinx
//                    gives them to the reference (examples/pmg/main.cpp:83-87); same numbers as without
//   --output FILE    write the solution as a legacy VTK file of the fine-level GLL points (:369-379)
#define PMG_AMD_DOLFINX_NAMESPACE
#include "../common/box_mesh.hpp"
#include "../common/brick_partition.hpp"
#include "../common/rank_launch.hpp"
#include "../common/rotating_tensor.hpp"
#include "pmg_amd.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <random>
#include <sstream>
#include <tuple>

using namespace dolfinx; // examples/pmg/main.cpp:29
using T = double;        // :30
using DeviceVector = dolfinx::acc::Vector<T, acc::Device::HIP>; // :33
using pmg_amd::check;
using pmg_amd::device_array;
using pmg_amd::hip_check;

/// The coarse solver of the reference is CoarseSolverType<T> (src/amg.hpp): anything with
/// solve(DeviceVector& x, DeviceVector& y).  Here: the library's AMG (Krylov or stationary mode).
template <typename U>
using CoarseSolverType = pmg_amd::acc::AmgSolver<acc::Vector<U, acc::Device::HIP>>;

namespace
{
/// What `V[i]->element()->basix_element()` of the reference reaches: the degree.
struct Element
{
  pmg_amd::LagrangeElement e;
  const pmg_amd::LagrangeElement& basix_element() const { return e; }
};
struct Space
{
  std::shared_ptr<Element> el;
  examples::PartitionLevel lv;
  std::shared_ptr<Element> element() const { return el; }
};

struct Options : examples::RankOptions
{
  int n = 64, cheb_its = 3, cycles = 10, amg_cycles = 0;
  std::vector<int> orders = {1, 2, 4};
  bool pcg = false, coarse_cg = false, use_amg = false, random_rhs = false, graph = false, fp32_cycle = false;
  std::string output;
  pmg_amd::NodeOrder node_order = pmg_amd::NodeOrder::ascending; // of the dofmaps handed to the library
  bool amg_gather = false; // --amg-setup gathered
  bool amg_renew = false;  // --amg-renew: the AMG created before the coefficient options, renewed in place after them
  bool kappa_field = false;    // --kappa-field: the smooth nodal coefficient 1 + 0.5 sin(2 pi x) cos(2 pi y) + z
  bool kappa_tensor = false;   // --kappa-tensor: per-cell tensor, eigenvalues (1, 2 + x, 4) rotated by Rz(0.6 + 0.8 y) Rx(0.4 + 0.5 z)
  double reaction = 0.0;       // --reaction S: sigma_c = S (1 + x_c); 0 = no term
  double robin = 0.0;          // --robin A: Dirichlet on x = 0 only, alpha = A (1 + y) on the other five faces; 0 = no term
  bool neumann = false;        // --neumann: no Dirichlet marker, compatible load, constant null space on every solver
  int curved = 0;              // --curved G: the box bent by examples::curved_map, coordinate element of degree G; 0 = the unit box
  bool csr = false;            // --csr [levels]: assembled levels (solve<acc::MatrixOperator<T>>, :285,457-458)
  std::vector<int> csr_levels; // empty with --csr: every level
};
using examples::parse3;

template <typename FineOperator>
void solve(const Options& o)
{
  const int size = o.ranks[0] * o.ranks[1] * o.ranks[2];
  const bool root = o.rank == 0;
  const std::vector<int>& order = o.orders;
  const T kappa = 2.0; // :190-193

  std::shared_ptr<const pmg_amd::Communicator> comm = examples::bootstrap(o);

  examples::BrickPartition mesh(o.n, o.ranks, o.rank);
  device_array<T> constants(std::vector<T>(mesh.ncells, kappa));
  // --curved G: the degree-G node grid of every local cell, mapped (the adapter infers G from the dofmap's width)
  std::vector<double> gll_g(o.curved + 1), w_g(o.curved + 1);
  if (o.curved)
    check(pmg_gll_table(o.curved + 1, gll_g.data(), w_g.data()));
  const examples::CurvedGeometry bent(mesh.xgeom, mesh.geom_dofmap, o.curved ? o.curved : 1,
                                      o.curved ? gll_g : std::vector<double>{0.0, 1.0});
  if (o.curved && root)
    std::printf("Curved cells: coordinate element of degree %d\n", o.curved);
  device_array<T> geom_x_d(o.curved ? bent.xgeom : mesh.xgeom);
  device_array<std::int32_t> geom_x_dofmap_d(o.curved ? bent.geom_dofmap : mesh.geom_dofmap);
  std::span<const T> device_constants = constants.span(), geom_x = geom_x_d.span();
  std::span<const std::int32_t> geom_x_dofmap = geom_x_dofmap_d.span();

  // function spaces, index maps, device copies of the dofmaps and Dirichlet markers (:83-257)
  std::vector<std::shared_ptr<Space>> V(order.size());
  std::vector<std::shared_ptr<const common::IndexMap>> maps(V.size());
  std::vector<device_array<std::int32_t>> dofmaps_d(V.size());
  std::vector<device_array<std::int8_t>> bc_markers_d(V.size());
  std::vector<std::span<const std::int32_t>> device_dofmaps(V.size());
  std::vector<std::span<const std::int8_t>> bc_marker_d_span(V.size());
  std::vector<std::span<const T>> geometry_dphi_d_span(V.size()), Gweights_d_span(V.size()); // from the degree
  std::vector<int> lcells, bcells; // src/mesh.hpp:105-143; the same split on every level
  for (std::size_t i = 0; i < V.size(); i++)
  {
    const int P = order[i], nd = P + 1;
    std::vector<double> gll(nd), w(nd);
    check(pmg_gll_table(nd, gll.data(), w.data()));
    V[i] = std::make_shared<Space>(Space{std::make_shared<Element>(Element{{P}}), mesh.level(P, gll)});
    if (o.robin > 0.0) // Dirichlet on x = 0 only; the other five faces carry the Robin term
      examples::keep_marker_on_x0(V[i]->lv.bc_marker, V[i]->lv.x);
    if (o.neumann) // natural conditions on the whole boundary
      std::fill(V[i]->lv.bc_marker.begin(), V[i]->lv.bc_marker.end(), std::int8_t(0));
    const examples::PartitionLevel& lv = V[i]->lv;
    if (comm)
      maps[i] = std::make_shared<const common::IndexMap>(lv.size_local, lv.num_ghosts, lv.send_indices,
                                                         lv.recv_indices, comm, lv.neighbors, lv.send_counts,
                                                         lv.recv_counts, o.halo());
    else
      maps[i] = std::make_shared<const common::IndexMap>(lv.size_local, lv.num_ghosts);
    if (i == V.size() - 1) // :97 (finest space)
      std::tie(lcells, bcells) = pmg_amd::compute_boundary_cells(lv.dofmap, mesh.ncells_owned, mesh.ncells,
                                                                 nd * nd * nd, lv.size_local);
    // --node-order basix: hand the library the dofmaps as dolfinx holds them (endpoints first per direction,
    // examples/pmg/main.cpp:83-87); the brick partition generates them ascending
    if (o.node_order == pmg_amd::NodeOrder::ascending)
      dofmaps_d[i].assign(lv.dofmap);
    else
      dofmaps_d[i].assign(pmg_amd::dofmap_in_node_order(lv.dofmap, P, o.node_order));
    bc_markers_d[i].assign(lv.bc_marker);
    device_dofmaps[i] = dofmaps_d[i].span();
    bc_marker_d_span[i] = bc_markers_d[i].span();
    if (root)
      std::printf("Level %zu: degree %d, %lld dofs (rank 0: %d owned + %d ghosts, %zu neighbours)\n", i, P,
                  (long long)mesh.global_ndofs(P), lv.size_local, lv.num_ghosts, lv.neighbors.size());
  }

  // --neumann on the undeformed unit box with constant coefficient: the manufactured problem
  const bool manufactured = o.neumann && !o.curved && !o.kappa_field && !o.kappa_tensor;
  std::vector<std::shared_ptr<FineOperator>> operators(V.size());
  std::vector<std::shared_ptr<DeviceVector>> bs(V.size());
  std::shared_ptr<CoarseSolverType<T>> coarse_solver; // :331-335
  for (std::size_t i = 0; i < V.size(); i++)
  {
    operators[i] = std::make_shared<acc::MatFreeLaplacian<T>>(
        order[i], device_constants, device_dofmaps[i], geom_x, geom_x_dofmap, geometry_dphi_d_span[i],
        Gweights_d_span[i], lcells, bcells, bc_marker_d_span[i], 0, o.node_order); // :270-272
    const examples::PartitionLevel& lv = V[i]->lv;
    if (i == 0 && o.amg_renew) // the hierarchy of the operator as created (constant kappa, no term); renewed below
      coarse_solver = std::make_shared<CoarseSolverType<T>>(*operators[0], maps[0]);
    if (o.kappa_field) // -div(kappa kq(x) grad u): the field at this level's dof coordinates, before the diagonal
    {
      std::vector<T> kh(lv.ndofs());
      for (std::int32_t d = 0; d < lv.ndofs(); ++d)
        kh[d] = 1.0 + 0.5 * std::sin(2 * M_PI * lv.x[3 * d]) * std::cos(2 * M_PI * lv.x[3 * d + 1]) + lv.x[3 * d + 2];
      DeviceVector kq(maps[i], 1);
      hip_check(hipMemcpy(kq.mutable_array().data(), kh.data(), sizeof(T) * kh.size(), hipMemcpyHostToDevice), "H2D");
      operators[i]->set_coefficient_field(kq);
    }
    if (o.kappa_tensor) // -div(kappa K grad u): one tensor per cell, the same cells on every level
    {
      device_array<T> kt(examples::rotating_tensor(mesh.xgeom, mesh.geom_dofmap));
      operators[i]->handle(maps[i]); // the handle is created with the first index map the operator sees
      operators[i]->set_coefficient_tensor(kt.span());
    }
    if (o.reaction > 0.0) // -div(kappa grad u) + sigma u: one value per cell, the same cells on every level
    {
      device_array<T> sigma(examples::linear_reaction(mesh.xgeom, mesh.geom_dofmap, o.reaction));
      operators[i]->handle(maps[i]);
      operators[i]->set_reaction(sigma.span());
    }
    if (o.robin > 0.0) // K grad u . n + alpha u = 0 on the five faces other than x = 0, at this level's facet points
    {
      const examples::RobinBoundary rb
          = examples::linear_robin(mesh.exterior_facets(), lv.dofmap, lv.x, order[i], o.robin);
      device_array<T> alpha(rb.alpha);
      operators[i]->handle(maps[i]);
      operators[i]->set_robin(rb.cells, rb.local_facets, alpha.span()); // (collective: a rank without a facet calls too)
    }
    operators[i]->compute_diag_inverse(maps[i]);                  // replaces :274-279 (no CSR)
    if (i == 0 && o.amg_renew) // pmg_amg_update_values: every value from the operator's current data, aggregates kept
    {
      auto t0 = std::chrono::steady_clock::now();
      coarse_solver->update_values();
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      std::printf("AMG renewed in place: %d levels, %lld rows, %.2f ms\n", coarse_solver->num_levels(),
                  (long long)lv.size_local, ms);
    }

    std::vector<T> fh(lv.ndofs());
    const double pi = M_PI, c2 = (4.0 + 9.0 + 16.0) * pi * pi;
    for (std::int32_t d = 0; d < lv.ndofs(); ++d)
      fh[d] = manufactured // -div(grad u) of u = cos pi x cos pi y cos pi z
                  ? 3.0 * pi * pi * std::cos(pi * lv.x[3 * d]) * std::cos(pi * lv.x[3 * d + 1]) * std::cos(pi * lv.x[3 * d + 2])
                  : c2 * std::sin(2 * pi * lv.x[3 * d]) * std::sin(3 * pi * lv.x[3 * d + 1]) * std::sin(4 * pi * lv.x[3 * d + 2]);
    DeviceVector f(maps[i], 1);
    hip_check(hipMemcpy(f.mutable_array().data(), fh.data(), sizeof(T) * fh.size(), hipMemcpyHostToDevice), "H2D");
    bs[i] = std::make_shared<DeviceVector>(maps[i], 1);
    operators[i]->assemble_rhs(f, *bs[i]); // :289-300
    if (o.neumann) // 1 . b = 0: the right-hand side is compatible
      acc::remove_mean(*bs[i]);
  }

  // --csr: the listed levels (default: all) as assembled matrices, the reference's solve<acc::MatrixOperator<T>>
  // (examples/pmg/main.cpp:285,457-458); the eigenvalue estimate, the smoother and the residual of such a level run
  // on the matrix, the transfers stay on the matrix-free operator's patches
  std::vector<std::shared_ptr<acc::MatrixOperator<T>>> matrices(V.size());
  if (o.csr)
    for (std::size_t i = 0; i < V.size(); i++)
    {
      if (!o.csr_levels.empty() && std::find(o.csr_levels.begin(), o.csr_levels.end(), (int)i) == o.csr_levels.end())
        continue;
      matrices[i] = std::make_shared<acc::MatrixOperator<T>>(*operators[i], maps[i]);
      const T a_norm = matrices[i]->norm(); // over all ranks: every rank calls
      if (root)
        std::printf("Level %zu: CSR nnz = %zu, A norm = %.15e\n", i, matrices[i]->nnz(), a_norm);
    }

  // ---------------------------------------------------------------------------------------------
  // From here to the end of the cycle loop: examples/pmg/main.cpp:303-367 (logging calls dropped,
  // Chebyshev degree and cycle count from the command line).

  // Create chebyshev smoother for each level
  std::vector<std::shared_ptr<acc::Chebyshev<DeviceVector>>> smoothers(V.size());
  for (std::size_t i = 0; i < V.size(); i++)
  {
    dolfinx::acc::CGSolver<DeviceVector> cg(maps[i], 1);
    cg.set_max_iterations(20);
    cg.set_tolerance(1e-6);
    cg.store_coefficients(true);

    DeviceVector x(maps[i], 1);

    x.set(T{0.0});
    DeviceVector y(maps[i], 1);
    y.set(T{1.0});

    [[maybe_unused]] int its = matrices[i] ? cg.solve(*matrices[i], x, y, false) : cg.solve(*operators[i], x, y, false);
    std::vector<T> eign = cg.compute_eigenvalues();
    std::sort(eign.begin(), eign.end());
    if (root)
      std::printf("Eigenvalues level %zu: %.17g - %.17g\n", i, eign.front(), eign.back());
    std::array<T, 2> eig_range = {0.1 * eign.back(), 1.1 * eign.back()};
    smoothers[i] = std::make_shared<acc::Chebyshev<DeviceVector>>(maps[i], 1, eig_range);
    smoothers[i]->set_max_iterations(o.cheb_its);
  }

  // Create Matrix-Free Interpolators
  std::vector<std::shared_ptr<Interpolator<T>>> matfree_interpolators(V.size() - 1);

  for (int i = 0; i < (int)V.size() - 1; ++i)
  {
    matfree_interpolators[i] = std::make_shared<Interpolator<T>>(
        V[i]->element()->basix_element(), V[i + 1]->element()->basix_element(), device_dofmaps[i],
        device_dofmaps[i + 1], lcells, bcells, o.node_order);
  }

  if (o.use_amg)
  {
    auto t0 = std::chrono::steady_clock::now();
    if (coarse_solver) // --amg-renew: created and renewed above
      ;
    else if (size > 1) // first coarsening per rank, level 1 gathered on every rank (--amg-setup gathered: the global
                  // degree-1 matrix on every rank instead); one all-reduce of a level-1 vector per cycle
      coarse_solver = std::make_shared<CoarseSolverType<T>>(*operators[0], maps[0], V[0]->lv.local_to_global,
                                                           mesh.global_ndofs(order[0]), o.amg_gather);
    else
      coarse_solver = std::make_shared<CoarseSolverType<T>>(*operators[0], maps[0]);
    if (o.amg_cycles > 0)
      coarse_solver->set_cycles(o.amg_cycles);
    if (o.neumann)
      coarse_solver->set_nullspace(true);
    if (root)
      std::printf("AMG coarse solver: %d levels, set-up %.2f s, %s\n", coarse_solver->num_levels(),
                  std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(),
                  o.amg_cycles > 0 ? "stationary cycles" : "CG <= 60 iterations, rtol 1e-5");
  }

  using SolverType = acc::Chebyshev<DeviceVector>;
  using PMG = acc::MultigridPreconditioner<DeviceVector, FineOperator, SolverType, CoarseSolverType<T>,
                                           Interpolator<T>>;

  PMG pmg(maps, 1, bc_marker_d_span[0]);
  pmg.set_solvers(smoothers);
  pmg.set_operators(operators);
  pmg.set_coarse_solver(coarse_solver);

  // Sets matrix-free kernels to do interpolation
  pmg.set_interpolators(matfree_interpolators);

  std::shared_ptr<dolfinx::acc::CGSolver<DeviceVector>> coarse_cg;
  if (o.coarse_cg && !o.use_amg) // a second coarse-solver type through the C ABI's native CG hook
  {
    coarse_cg = std::make_shared<dolfinx::acc::CGSolver<DeviceVector>>(maps[0], 1);
    coarse_cg->set_max_iterations(60);
    coarse_cg->set_tolerance(1e-5);
    coarse_cg->set_nullspace(o.neumann);
    check(pmg_multigrid_set_coarse_solver(pmg.handle(), coarse_cg->handle()));
  }

  for (std::size_t i = 0; i < V.size(); i++)
    if (matrices[i])
      pmg.set_level_matrix((int)i, matrices[i]->matrix_handle());

  if (o.fp32_cycle)
  {
    pmg.set_precision(PMG_PRECISION_FP32);
    if (root)
      std::printf("Cycle precision: fp32\n");
  }

  // Create solution vector
  DeviceVector x(maps.back(), 1);
  x.set(T{0.0});

  if (root)
    std::printf("Norm of b = %.15e\n", acc::norm(*bs.back()));
  else
    (void)acc::norm(*bs.back()); // reductions are collective
  int niter = o.cycles;
  for (int i = 0; i < niter; i++)
  {
    const T rnorm = pmg.apply(*bs.back(), x, true);
    if (root)
      std::printf("Cycle %d: residual norm = %.15e\n", i + 1, rnorm);
  }
  // ---------------------------------------------------------------------------------------------
  {
    const T xn = acc::norm(x);
    if (root)
      std::printf("Norm of x = %.15e\n", xn);
  }

  // --graph: the timed cycles replayed as one hipGraph each (with --ranks: the halo exchange captured with them)
  if (o.graph)
    check(pmg_multigrid_set_graph(pmg.handle(), 1));
  // timing of the cycle alone (no residual evaluation)
  hipEvent_t e0, e1;
  hip_check(hipEventCreate(&e0), "event");
  hip_check(hipEventCreate(&e1), "event");
  const int reps = 10;
  pmg.apply(*bs.back(), x, false);
  hip_check(hipEventRecord(e0, nullptr), "record");
  for (int i = 0; i < reps; ++i)
    pmg.apply(*bs.back(), x, false);
  hip_check(hipEventRecord(e1, nullptr), "record");
  hip_check(hipEventSynchronize(e1), "sync");
  float ms = 0;
  hip_check(hipEventElapsedTime(&ms, e0, e1), "elapsed");
  if (root)
    std::printf("V-cycle: %.3f ms, %.3f GDoF/s%s\n", ms / reps,
                (double)mesh.global_ndofs(order.back()) / (ms * 1e-3 / reps) * 1e-9,
                o.graph ? (pmg_multigrid_graph_replays(pmg.handle()) > 0 ? " (hipGraph replays)" : " (not capturable: eager)")
                        : "");
  if (o.graph)
    check(pmg_multigrid_set_graph(pmg.handle(), 0));

  if (o.pcg)
  {
    dolfinx::acc::CGSolver<DeviceVector> cg(maps.back(), 1);
    cg.set_max_iterations(100);
    cg.set_tolerance(1e-8);
    // with a Krylov coarse solve inside, the cycle is not a fixed linear operator
    cg.set_flexible(o.coarse_cg || (o.use_amg && o.amg_cycles == 0)); // (stationary AMG cycles: a fixed operator)
    cg.set_nullspace(o.neumann);
    DeviceVector rhs(maps.back(), 1);
    if (o.random_rhs)
    {
      const examples::PartitionLevel& lv = V.back()->lv;
      std::vector<T> g(lv.ndofs());
      for (std::int32_t d = 0; d < lv.ndofs(); ++d) // a function of the GLOBAL dof: the same vector on any partition
      {
        std::mt19937_64 gen(0x9E3779B97F4A7C15ull ^ (std::uint64_t)lv.local_to_global[d]);
        g[d] = lv.bc_marker[d] ? 0.0 : std::normal_distribution<T>()(gen);
      }
      hip_check(hipMemcpy(rhs.mutable_array().data(), g.data(), sizeof(T) * g.size(), hipMemcpyHostToDevice), "H2D");
    }
    else
      acc::copy(rhs, *bs.back());
    if (o.neumann)
      acc::remove_mean(rhs);
    x.set(0.0);
    const int its = cg.solve(*operators.back(), x, rhs, pmg, false);
    DeviceVector Ax(maps.back(), 1), r(maps.back(), 1);
    (*operators.back())(x, Ax);
    acc::axpy(r, -1.0, Ax, rhs); // r = b - A x
    const T rn = acc::norm(r), bn = acc::norm(rhs), xn = acc::norm(x);
    if (root)
      std::printf("PCG with V-cycle preconditioner: %d iterations, |b - A x| / |b| = %.3e, Norm of x = %.15e\n", its,
                  rn / bn, xn);
    if (manufactured && !o.random_rhs)
    {
      // the constant of the solution is fixed by a zero integral mean: lumped-mass weights (assemble_rhs of ones), on
      // the computed solution and on the nodal values of u alike
      const examples::PartitionLevel& lv = V.back()->lv;
      std::vector<T> uh(lv.ndofs());
      for (std::int32_t d = 0; d < lv.ndofs(); ++d)
        uh[d] = std::cos(M_PI * lv.x[3 * d]) * std::cos(M_PI * lv.x[3 * d + 1]) * std::cos(M_PI * lv.x[3 * d + 2]);
      DeviceVector ones(maps.back(), 1), mass(maps.back(), 1), u(maps.back(), 1);
      ones.set(T{1.0});
      operators.back()->assemble_rhs(ones, mass);
      hip_check(hipMemcpy(u.mutable_array().data(), uh.data(), sizeof(T) * uh.size(), hipMemcpyHostToDevice), "H2D");
      acc::remove_mean(u, mass);
      acc::remove_mean(x, mass);
      acc::axpy(r, -1.0, u, x); // r = x - u
      const T err = acc::norm(r, dolfinx::la::Norm::linf);
      if (root)
        std::printf("Neumann manufactured solution: max nodal error = %.6e\n", err);
    }
  }

  if (!o.output.empty()) // :369-379 (VTX there; here the fine-level points of this rank as legacy VTK)
  {
    const examples::PartitionLevel& lv = V.back()->lv;
    auto xv = x.thrust_vector(); // :373
    std::vector<T> u(xv.size());
    thrust::copy(xv.begin(), xv.end(), u.begin()); // :374
    const std::string name = size > 1 ? o.output + "." + std::to_string(o.rank) : o.output;
    std::ofstream f(name);
    f << "# vtk DataFile Version 3.0\npmg_amd solution, degree " << order.back() << "\nASCII\nDATASET POLYDATA\nPOINTS "
      << lv.size_local << " double\n";
    f.precision(17);
    for (std::int32_t d = 0; d < lv.size_local; ++d)
      f << lv.x[3 * d] << " " << lv.x[3 * d + 1] << " " << lv.x[3 * d + 2] << "\n";
    f << "POINT_DATA " << lv.size_local << "\nSCALARS u double 1\nLOOKUP_TABLE default\n";
    for (std::int32_t d = 0; d < lv.size_local; ++d)
      f << u[d] << "\n";
    if (root)
      std::printf("Solution written to %s\n", name.c_str());
  }
}
} // namespace

int main(int argc, char** argv)
{
  Options o;
  std::size_t ndofs = 0;
  std::string check_dims;
  o.rank = examples::default_rank();
  try
  {
    for (int i = 1; i < argc; ++i)
    {
      auto next = [&]() -> const char* { return i + 1 < argc ? argv[++i] : "0"; };
      if (!std::strcmp(argv[i], "--n"))
        o.n = std::atoi(next());
      else if (!std::strcmp(argv[i], "--ndofs")) // dofs per rank, like the reference (:412-435)
        ndofs = std::strtoull(next(), nullptr, 10);
      else if (!std::strcmp(argv[i], "--orders"))
      {
        o.orders.clear();
        std::stringstream ss(next());
        for (std::string tok; std::getline(ss, tok, ',');)
          o.orders.push_back(std::atoi(tok.c_str()));
      }
      else if (!std::strcmp(argv[i], "--smoother-its"))
        o.cheb_its = std::atoi(next());
      else if (!std::strcmp(argv[i], "--cycles"))
        o.cycles = std::atoi(next());
      else if (!std::strcmp(argv[i], "--pcg"))
        o.pcg = true;
      else if (!std::strcmp(argv[i], "--random-rhs"))
        o.random_rhs = true;
      else if (!std::strcmp(argv[i], "--graph"))
        o.graph = true;
      else if (!std::strcmp(argv[i], "--fp32-cycle"))
        o.fp32_cycle = true;
      else if (!std::strcmp(argv[i], "--kappa-field"))
        o.kappa_field = true;
      else if (!std::strcmp(argv[i], "--kappa-tensor"))
        o.kappa_tensor = true;
      else if (!std::strcmp(argv[i], "--reaction") && i + 1 < argc)
        o.reaction = std::atof(argv[++i]);
      else if (!std::strcmp(argv[i], "--robin") && i + 1 < argc)
        o.robin = std::atof(argv[++i]);
      else if (!std::strcmp(argv[i], "--neumann"))
        o.neumann = true;
      else if (!std::strcmp(argv[i], "--curved") && i + 1 < argc)
      {
        o.curved = std::atoi(argv[++i]);
        if (o.curved < 1 || o.curved > PMG_MAX_GEOM_DEGREE)
          throw std::runtime_error("--curved takes a geometry degree 1..4");
      }
      else if (!std::strcmp(argv[i], "--csr"))
      {
        o.csr = true;
        if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') // optional list of level indices
        {
          std::stringstream ss(argv[++i]);
          for (std::string tok; std::getline(ss, tok, ',');)
            o.csr_levels.push_back(std::atoi(tok.c_str()));
        }
      }
      else if (!std::strcmp(argv[i], "--coarse-cg"))
        o.coarse_cg = true;
      else if (!std::strcmp(argv[i], "--amg"))
        o.use_amg = true;
      else if (!std::strcmp(argv[i], "--amg-cycles"))
      {
        o.use_amg = true;
        o.amg_cycles = std::atoi(next());
      }
      else if (!std::strcmp(argv[i], "--ranks"))
        o.ranks = parse3(next());
      else if (!std::strcmp(argv[i], "--rank"))
        o.rank = std::atoi(next());
      else if (!std::strcmp(argv[i], "--native-comm")) // one rank through the RCCL communicator anyway
        o.native_comm = true;
      else if (!std::strcmp(argv[i], "--comm"))
      {
        const std::string how = next();
        if (how != "windows" && how != "rccl")
          throw std::runtime_error("--comm rccl | windows");
        o.window_comm = how == "windows";
      }
      else if (!std::strcmp(argv[i], "--halo"))
      {
        const std::string how = next();
        if (how != "windows" && how != "exchange")
          throw std::runtime_error("--halo exchange | windows");
        o.windows = how == "windows";
      }
      else if (!std::strcmp(argv[i], "--id-file"))
        o.id_file = next();
      else if (!std::strcmp(argv[i], "--amg-renew"))
        o.use_amg = o.amg_renew = true;
      else if (!std::strcmp(argv[i], "--amg-setup"))
      {
        const std::string v = next();
        if (v != "gathered" && v != "distributed")
          throw std::runtime_error("--amg-setup distributed | gathered");
        o.amg_gather = v == "gathered";
      }
      else if (!std::strcmp(argv[i], "--node-order"))
      {
        const std::string v = next();
        if (v == "basix" || v == "endpoints_first")
          o.node_order = pmg_amd::NodeOrder::endpoints_first;
        else if (v == "ascending")
          o.node_order = pmg_amd::NodeOrder::ascending;
        else
          throw std::runtime_error("--node-order ascending | basix");
      }
      else if (!std::strcmp(argv[i], "--output"))
        o.output = next();
      else if (!std::strcmp(argv[i], "--check-partition"))
        check_dims = next();
      else
      {
        std::cout << "usage: pmg [--n cells_per_direction | --ndofs N_per_rank] [--orders 1,2,4] [--smoother-its K]\n"
                     "           [--cycles C] [--pcg [--random-rhs]] [--amg [--amg-renew] | --amg-cycles N | --coarse-cg] [--graph] [--fp32-cycle] [--csr [LEVELS]]\n"
                     "           [--kappa-field] [--kappa-tensor] [--reaction S] [--robin A] [--curved G] [--neumann]\n"
                     "           [--ranks px,py,pz [--rank r] [--id-file F]] [--native-comm] [--halo exchange|windows]\n"
                     "           [--comm rccl|windows]\n"
                     "           [--node-order ascending|basix] [--amg-setup distributed|gathered]\n"
                     "           [--output FILE]\n"
                     "           [--check-partition px,py,pz]\n";
        return !std::strcmp(argv[i], "--help") || !std::strcmp(argv[i], "-h") ? 0 : 2;
      }
    }
    if (o.orders.empty() || !std::is_sorted(o.orders.begin(), o.orders.end())
        || std::adjacent_find(o.orders.begin(), o.orders.end()) != o.orders.end())
      throw std::runtime_error("--orders must be strictly ascending (coarse to fine)");
    const int size = o.ranks[0] * o.ranks[1] * o.ranks[2];
    if (o.fp32_cycle && size > 1)
      throw std::runtime_error("--fp32-cycle is single-domain only (--ranks asks for " + std::to_string(size)
                               + " ranks)");
    if (o.neumann && (o.reaction > 0.0 || o.robin > 0.0))
      throw std::runtime_error("--neumann with --reaction or --robin: the operator is then not singular, and "
                               "projecting out the constants would be wrong");
    if (o.amg_renew && size > 1)
      throw std::runtime_error("--amg-renew on several ranks: pmg_amg_update_values serves the single-domain hierarchy");
    if (o.neumann && o.use_amg && size > 1)
      throw std::runtime_error("--neumann with --amg on several ranks: the replicated and distributed AMG take no "
                               "null space");
    if (ndofs) // cells per direction of the whole mesh so that a rank holds about ndofs fine dofs
      o.n = examples::cells_for_ndofs(ndofs * (std::size_t)size, o.orders.back());
    if (!check_dims.empty())
    {
      const auto dims = parse3(check_dims.c_str());
      for (int P : o.orders)
      {
        std::vector<double> gll(P + 1), w(P + 1);
        check(pmg_gll_table(P + 1, gll.data(), w.data()));
        const std::string err = examples::check_partition(o.n, dims, P, gll);
        if (!err.empty())
          throw std::runtime_error("partition check failed at degree " + std::to_string(P) + ": " + err);
      }
      std::printf("partition %dx%dx%d of %d^3 cells consistent for every degree\n", dims[0], dims[1], dims[2], o.n);
      return 0;
    }
    examples::select_device(o);
    solve<acc::MatFreeLaplacian<T>>(o);
  }
  catch (const std::exception& ex)
  {
    std::cerr << "error: " << ex.what() << "\n";
    return 1;
  }
  return 0;
}
