// Matrix-free Laplacian apply driver: the MI355X counterpart of the reference's
// examples/mat_free/main.cpp (BASELINE config 1 with the defaults --n 16 --degree 1).
// Unit cube, n^3 hexes, degree P, kappa = 2 (:132), Dirichlet marker on all exterior
// dofs (:163-165,236-240), u = 1 (:250-256), nreps applies timed, ||u||, ||y|| printed
// (:267-268).  --mat_comp compares y with the product of the assembled CSR operator
// (acc::MatrixOperator, as the reference does, :270-288; any degree) and, at degree 1, also
// with the 7-point stencil the collocated P=1 operator reduces to, evaluated on the host.
// --kappa-field sets the smooth nodal coefficient 1 + 0.5 sin(2 pi x) cos(2 pi y) + z on the operator (not in the
// reference); the stencil comparison, which is for a constant coefficient, is then left out.
// --kappa-tensor sets the per-cell diffusion tensor with eigenvalues (1, 2 + x, 4) rotated by
// Rz(0.6 + 0.8 y) Rx(0.4 + 0.5 z) at the cell centre (not in the reference); it combines with --kappa-field, and the
// stencil comparison is left out as well.
// --reaction S adds the reaction term sigma u with sigma_c = S (1 + x_c) at the cell centre (not in the reference;
// pmg_laplacian_set_reaction); it combines with the two above, and the stencil comparison is left out as well.
// --robin A keeps the Dirichlet marker on the face x = 0 only and puts a Robin term with alpha = A (1 + y) at the facet
// points of the other five faces (not in the reference; pmg_laplacian_set_robin); it combines with the three above,
// and the stencil comparison is left out as well.
// --neumann removes the Dirichlet marker altogether: the singular, pure Neumann operator (the one pmg_cg_set_nullspace
// and pmg_amg_set_nullspace are for); with --mat_comp the matrix-free product is compared with the CSR product of that
// operator on a vector that is not constant.  The stencil comparison is left out as well.
// --curved G (1..4) bends the box by a fixed smooth map (examples/common/box_mesh.hpp: curved_map) and hands the library
// a coordinate element of degree G (pmg_laplacian_create_curved through the adapter, which infers G from the geometry
// dofmap's width); G = 1 is the straight-sided mesh through the mapped vertices.  It combines with every flag above
// (their data stay functions of the box coordinates); the stencil comparison is left out as well.
// --lift restates the right-hand side the reference's driver has commented out (:252-255): u = the assembled load of
// f = 0 (:133,143: the interpolation of f is commented out as well), lifted with the boundary value 1.3 (:165) and
// set_bc -- pmg_laplacian_assemble_rhs, _apply_lifting, _set_bc on the one operator -- instead of u = 1.
// --cell-form prints, after the apply y = A u, the sum over the cells of the per-cell bilinear form e_c(u, u)
// (pmg_laplacian_cell_form with kappa, marked dofs read as zero; not in the reference) beside u_m . y, u_m = u with its
// marked entries zeroed, and their relative difference: the two are the same number, computed by two kernels.  It
// combines with --kappa-field, --kappa-tensor and --curved (the reaction and Robin terms are not part of the form).
// --form-gradients prints, after the apply, the three Euler sums of pmg_laplacian_form_gradients (marked dofs read as
// zero; not in the reference) at u and a second vector v -- sum_c kappa_c d_kappa[c], sum_n kq_n d_field[n] and
// sum_c T_c . d_tensor[c]: A_diff is linear in each coefficient -- beside u_m . (A_diff v_m) from an apply of the
// operator without its reaction term, and their relative differences; sum_c sigma_c d_sigma[c] is printed beside
// u_m . ((A - A_diff) v_m).  It combines with --kappa-field, --kappa-tensor, --reaction and --curved.
// Single rank.
#include "../common/box_mesh.hpp"
#include "../common/rotating_tensor.hpp"
#include "pmg_amd.hpp"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

using namespace pmg_amd;
using T = double;                                          // examples/mat_free/main.cpp:31
using DeviceVector = acc::Vector<T, acc::Device::HIP>;

int main(int argc, char** argv)
{
  int n = 16, degree = 1, nreps = 1000;
  std::size_t ndofs = 0;
  bool mat_comp = false, kappa_field = false, kappa_tensor = false, lift = false, cell_form = false, form_gradients = false;
  bool neumann = false; // --neumann: no Dirichlet marker (the singular, pure Neumann operator)
  double reaction = 0.0; // S of --reaction; 0 = no term
  double robin = 0.0;    // A of --robin; 0 = no term
  int curved = 0;        // G of --curved; 0 = the unit box, trilinear
  std::size_t batch_size = 0; // :38,46-50: cells whose geometry tensor is held at a time (0 = all, resident)
  for (int i = 1; i < argc; ++i)
  {
    auto next = [&]() -> const char* { return i + 1 < argc ? argv[++i] : "0"; };
    if (!std::strcmp(argv[i], "--n"))
      n = std::atoi(next());
    else if (!std::strcmp(argv[i], "--ndofs"))
      ndofs = std::strtoull(next(), nullptr, 10);
    else if (!std::strcmp(argv[i], "--degree"))
      degree = std::atoi(next());
    else if (!std::strcmp(argv[i], "--nreps"))
      nreps = std::atoi(next());
    else if (!std::strcmp(argv[i], "--mat_comp"))
      mat_comp = true;
    else if (!std::strcmp(argv[i], "--kappa-field"))
      kappa_field = true;
    else if (!std::strcmp(argv[i], "--kappa-tensor"))
      kappa_tensor = true;
    else if (!std::strcmp(argv[i], "--reaction"))
      reaction = std::atof(next());
    else if (!std::strcmp(argv[i], "--robin"))
      robin = std::atof(next());
    else if (!std::strcmp(argv[i], "--neumann"))
      neumann = true;
    else if (!std::strcmp(argv[i], "--curved"))
      curved = std::atoi(next());
    else if (!std::strcmp(argv[i], "--lift"))
      lift = true;
    else if (!std::strcmp(argv[i], "--cell-form"))
      cell_form = true;
    else if (!std::strcmp(argv[i], "--form-gradients"))
      form_gradients = true;
    else if (!std::strcmp(argv[i], "--batch_size"))
      batch_size = std::strtoull(next(), nullptr, 10);
    else
    {
      std::cout << "usage: mat_free [--n cells_per_direction | --ndofs N] [--degree P] [--nreps R] [--mat_comp] "
                   "[--batch_size cells] [--kappa-field] [--kappa-tensor] [--reaction S] [--robin A] [--curved G] [--lift] [--neumann] [--cell-form] [--form-gradients]\n";
      return !std::strcmp(argv[i], "--help") || !std::strcmp(argv[i], "-h") ? 0 : 2;
    }
  }
  try
  {
    if (degree < 1 || degree > PMG_MAX_DEGREE)
      throw std::runtime_error("Unsupported degree");
    if (ndofs)
      n = examples::cells_for_ndofs(ndofs, degree);
    const int nd = degree + 1;
    std::vector<double> gll(nd), w(nd);
    check(pmg_gll_table(nd, gll.data(), w.data()));

    examples::BoxMesh mesh(n);
    examples::FunctionSpace V(mesh, degree, gll);
    std::cout << "Mesh " << n << "^3 hexes, degree " << degree << ", " << V.ndofs << " dofs\n";

    if (robin > 0.0) // Dirichlet on x = 0 only; the other five faces carry the Robin term
      examples::keep_marker_on_x0(V.bc_marker, V.x);

    if (neumann) // natural conditions on the whole boundary: the operator the null-space solvers work on
      std::fill(V.bc_marker.begin(), V.bc_marker.end(), std::int8_t(0));

    auto map = std::make_shared<const IndexMap>(V.ndofs, 0);
    const double kappa_value = 2.0; // :132
    device_array<double> kappa(std::vector<double>(mesh.ncells(), kappa_value));
    if (curved < 0 || curved > PMG_MAX_GEOM_DEGREE)
      throw std::runtime_error("--curved takes a geometry degree 1..4");
    std::vector<double> gll_g(curved + 1), w_g(curved + 1);
    if (curved)
      check(pmg_gll_table(curved + 1, gll_g.data(), w_g.data()));
    const examples::CurvedGeometry bent(mesh.xgeom, mesh.geom_dofmap, curved ? curved : 1,
                                        curved ? gll_g : std::vector<double>{0.0, 1.0});
    if (curved)
      std::cout << "Curved cells: coordinate element of degree " << curved << "\n";
    device_array<std::int32_t> dofmap(V.dofmap), xdofmap(curved ? bent.geom_dofmap : mesh.geom_dofmap);
    device_array<double> xgeom(curved ? bent.xgeom : mesh.xgeom);
    device_array<std::int8_t> bc(V.bc_marker);
    // one rank: no ghost dofs, so every cell comes out local (src/mesh.hpp:105-143)
    auto [lcells, bcells] = compute_boundary_cells(V.dofmap, mesh.ncells(), mesh.ncells(), nd * nd * nd, V.ndofs);

    auto t0 = std::chrono::steady_clock::now();
    acc::MatFreeLaplacian<T> op(degree, kappa.span(), dofmap.span(), xgeom.span(), xdofmap.span(), {}, {}, lcells,
                                bcells, bc.span(), batch_size);
    DeviceVector u(map, 1), y(map, 1);
    u.set(1.0);
    std::vector<double> kt_h, sigma_h, kq_h; // host copies of the coefficients that are set (--form-gradients)
    if (kappa_tensor)
    {
      kt_h = examples::rotating_tensor(mesh.xgeom, mesh.geom_dofmap);
      device_array<double> kt(kt_h);
      op.handle(map); // the handle is created with the first index map the operator sees
      op.set_coefficient_tensor(kt.span()); // the library copies it
    }
    if (reaction > 0.0)
    {
      sigma_h = examples::linear_reaction(mesh.xgeom, mesh.geom_dofmap, reaction);
      device_array<double> sigma(sigma_h);
      op.handle(map);
      op.set_reaction(sigma.span()); // the library keeps the vector it builds from it
    }
    if (robin > 0.0)
    {
      const examples::RobinBoundary rb
          = examples::linear_robin(examples::exterior_facets(mesh), V.dofmap, V.x, degree, robin);
      device_array<double> alpha(rb.alpha);
      op.handle(map);
      op.set_robin(rb.cells, rb.local_facets, alpha.span()); // the library keeps the vector it builds from it
    }
    if (kappa_field || kappa_tensor || reaction > 0.0 || robin > 0.0 || neumann) // (--neumann: u = 1 is the null vector)
    {
      std::vector<double> kh(V.ndofs);
      // u = 1 lies in the kernel of the operator away from the boundary whatever the coefficient: a vector that
      // shows the coefficient everywhere
      for (std::size_t d = 0; d < kh.size(); ++d)
        kh[d] = std::sin(1.0 + 3 * V.x[3 * d] + 5 * V.x[3 * d + 1] * V.x[3 * d + 2]);
      u.copy_from_host(kh);
    }
    if (kappa_field)
    {
      std::vector<double> kh(V.ndofs);
      for (std::size_t d = 0; d < kh.size(); ++d)
        kh[d] = 1.0 + 0.5 * std::sin(2 * M_PI * V.x[3 * d]) * std::cos(2 * M_PI * V.x[3 * d + 1]) + V.x[3 * d + 2];
      DeviceVector kq(map, 1);
      kq.copy_from_host(kh);
      op.set_coefficient_field(kq);
      kq_h = kh;
    }
    if (lift)
    {
      DeviceVector f(map, 1), g(map, 1);
      f.set(0.0);
      g.set(1.3); // read on the marked dofs only
      op.assemble_rhs(f, u);   // fem::assemble_vector(b, *L)
      op.apply_lifting(g, u);  // fem::apply_lifting(b, {a}, {{bc}}, {}, 1)
      op.set_bc(g, u);         // fem::set_bc(b, {bc})
      std::printf("Lifted right-hand side: %d of %d cells hold a Dirichlet dof\n",
                  pmg_laplacian_lift_cell_count(op.handle(map)), (int)mesh.ncells());
    }
    op(u, y); // creates the handle (geometry, patches) and warms up
    hip_check(hipDeviceSynchronize(), "sync");
    auto t1 = std::chrono::steady_clock::now();
    std::cout << "Create matfree operator: " << std::chrono::duration<double>(t1 - t0).count() << " s\n";
    std::printf("Geometry tensor held: %.3f MB%s\n", pmg_laplacian_geometry_bytes(op.handle(map)) * 1e-6,
                batch_size ? " (recomputed batch by batch in every apply)" : " (resident)");

    hipEvent_t e0, e1;
    hip_check(hipEventCreate(&e0), "event");
    hip_check(hipEventCreate(&e1), "event");
    hip_check(hipEventRecord(e0, nullptr), "record");
    for (int i = 0; i < nreps; ++i)
      op(u, y);
    hip_check(hipEventRecord(e1, nullptr), "record");
    hip_check(hipEventSynchronize(e1), "sync");
    float ms = 0;
    hip_check(hipEventElapsedTime(&ms, e0, e1), "elapsed");
    const double per = ms * 1e-3 / nreps;
    const double N = (double)nd * nd * nd, U = (double)degree * degree * degree;
    const double bytes = (48 * N + 4 * N + 8 + 17 * U) * mesh.ncells(); // SURVEY 8d, model storedG
    std::printf("Mat-free Matvec: %d reps, %.3f us per apply, %.3f GDoF/s, %.1f GB/s algorithmic\n", nreps, per * 1e6,
                V.ndofs / per * 1e-9, bytes / per * 1e-9);
    std::printf("Norm of u = %.15e\n", acc::norm(u));
    std::printf("Norm of y = %.15e\n", acc::norm(y));

    if (cell_form)
    {
      // sum_c e_c(u, u) with kappa and the marked dofs read as zero = u_m . (A u_m) = u_m . y (marked columns of A are
      // masked, and u_m is zero on the marked rows)
      device_array<double> e(mesh.ncells());
      op.cell_form(u, u, e.span(), true, true);
      hip_check(hipDeviceSynchronize(), "sync");
      const std::vector<double> eh = e.to_host(), uh = u.data_copy(), yh = y.data_copy();
      double energy = 0.0, dot = 0.0;
      for (double v : eh)
        energy += v;
      for (std::size_t d = 0; d < (std::size_t)V.ndofs; ++d)
        if (!V.bc_marker[d])
          dot += uh[d] * yh[d];
      std::printf("Cell form: sum_c e_c(u, u) = %.15e\n", energy);
      std::printf("Cell form: u_m . y = %.15e\n", dot);
      std::printf("Cell form: relative difference = %.3e\n", std::fabs(energy - dot) / std::fabs(dot));
    }

    if (form_gradients)
    {
      if (robin > 0.0)
        throw std::runtime_error("--form-gradients does not combine with --robin");
      const std::size_t nc = mesh.ncells();
      std::vector<double> vh(V.ndofs);
      for (std::size_t d = 0; d < vh.size(); ++d)
        vh[d] = std::cos(2.0 + 2 * V.x[3 * d] - 3 * V.x[3 * d + 1] + 4 * V.x[3 * d] * V.x[3 * d + 2]);
      DeviceVector v(map, 1), yv(map, 1), yd(map, 1);
      v.copy_from_host(vh);
      device_array<double> dk(nc), df((std::size_t)V.ndofs), dt(6 * nc), ds(nc);
      op.form_gradients(u, v, dk.span(), df.span(), dt.span(), ds.span(), true);
      op(v, yv); // A v
      if (reaction > 0.0)
        op.clear_reaction();
      op(v, yd); // A_diff v
      if (reaction > 0.0)
      {
        device_array<double> sigma(sigma_h);
        op.set_reaction(sigma.span()); // the operator as it was
      }
      hip_check(hipDeviceSynchronize(), "sync");
      const std::vector<double> dkh = dk.to_host(), dfh = df.to_host(), dth = dt.to_host(), dsh = ds.to_host(),
                                uh = u.data_copy(), yvh = yv.data_copy(), ydh = yd.data_copy();
      double s_kappa = 0.0, s_field = 0.0, s_tensor = 0.0, s_sigma = 0.0, dot = 0.0, dot_r = 0.0;
      for (std::size_t c = 0; c < nc; ++c)
      {
        s_kappa += kappa_value * dkh[c];
        if (kappa_tensor)
          for (int k = 0; k < 6; ++k)
            s_tensor += kt_h[6 * c + k] * dth[6 * c + k]; // (an off-diagonal entry of d_tensor counts both of the matrix)
        else
          s_tensor += dth[6 * c] + dth[6 * c + 3] + dth[6 * c + 5];
        if (reaction > 0.0)
          s_sigma += sigma_h[c] * dsh[c];
      }
      for (std::size_t d = 0; d < (std::size_t)V.ndofs; ++d)
      {
        s_field += (kappa_field ? kq_h[d] : 1.0) * dfh[d];
        if (!V.bc_marker[d])
        {
          dot += uh[d] * ydh[d];
          dot_r += uh[d] * (yvh[d] - ydh[d]);
        }
      }
      auto rel = [](double a, double b) { return std::fabs(a - b) / std::fabs(b); };
      std::printf("Form gradients: u_m . (A_diff v_m) = %.15e\n", dot);
      std::printf("Form gradients: sum_c kappa_c d_kappa[c] = %.15e\n", s_kappa);
      std::printf("Form gradients: sum_n kq_n d_field[n] = %.15e\n", s_field);
      std::printf("Form gradients: sum_c T_c . d_tensor[c] = %.15e\n", s_tensor);
      std::printf("Form gradients: relative difference (kappa) = %.3e\n", rel(s_kappa, dot));
      std::printf("Form gradients: relative difference (field) = %.3e\n", rel(s_field, dot));
      std::printf("Form gradients: relative difference (tensor) = %.3e\n", rel(s_tensor, dot));
      if (reaction > 0.0)
      {
        std::printf("Form gradients: u_m . ((A - A_diff) v_m) = %.15e\n", dot_r);
        std::printf("Form gradients: sum_c sigma_c d_sigma[c] = %.15e\n", s_sigma);
        std::printf("Form gradients: relative difference (sigma) = %.3e\n", rel(s_sigma, dot_r));
      }
    }

    if (mat_comp)
    {
      // the assembled operator on the same vector (examples/mat_free/main.cpp:270-288), any degree
      acc::MatrixOperator<T> mat(op, map);
      DeviceVector zc(map, 1), ec(map, 1);
      mat(u, zc);
      hip_check(hipEventRecord(e0, nullptr), "record");
      for (int i = 0; i < nreps; ++i)
        mat(u, zc);
      hip_check(hipEventRecord(e1, nullptr), "record");
      hip_check(hipEventSynchronize(e1), "sync");
      hip_check(hipEventElapsedTime(&ms, e0, e1), "elapsed");
      std::printf("CSR Matvec: %d reps, %.3f us per apply\n", nreps, ms * 1e3 / nreps);
      std::printf("CSR nnz = %zu\n", mat.nnz());
      acc::axpy(ec, -1.0, y, zc);
      if (degree != 1 || kappa_field || kappa_tensor || reaction > 0.0 || robin > 0.0 || curved || neumann)
      {
        std::printf("Norm of z = %.15e\n", acc::norm(zc));
        std::printf("Norm of error = %.3e\n", acc::norm(ec));
        return 0;
      }
      std::printf("CSR error norm = %.3e\n", acc::norm(ec)); // the stencil comparison below keeps its own lines
      // rows of the collocated P=1 operator on a uniform grid: kappa*h*(6 u_c - sum of the 6 neighbours),
      // Dirichlet columns masked, Dirichlet rows y = u
      const int m = n + 1;
      const double h = 1.0 / n, kap = 2.0;
      std::vector<double> uh = u.data_copy(), z(V.ndofs);
      auto at = [&](int i, int j, int k) {
        const std::size_t d = ((std::size_t)i * m + j) * m + k;
        return V.bc_marker[d] ? 0.0 : uh[d];
      };
      for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j)
          for (int k = 0; k < m; ++k)
          {
            const std::size_t d = ((std::size_t)i * m + j) * m + k;
            z[d] = V.bc_marker[d] ? uh[d]
                                  : kap * h
                                        * (6 * at(i, j, k) - at(i - 1, j, k) - at(i + 1, j, k) - at(i, j - 1, k)
                                           - at(i, j + 1, k) - at(i, j, k - 1) - at(i, j, k + 1));
          }
      DeviceVector zd(map, 1), e(map, 1);
      zd.copy_from_host(z);
      acc::axpy(e, -1.0, y, zd);
      std::printf("Norm of z = %.15e\n", acc::norm(zd));
      std::printf("Norm of error = %.3e\n", acc::norm(e));
    }
  }
  catch (const std::exception& ex)
  {
    std::cerr << "error: " << ex.what() << "\n";
    return 1;
  }
  return 0;
}
