// Stand-alone host checker of the launch plans (patches.hpp): the patch plan, the chain plan and the coarse lists of
// the patch-form transfers.  The kernels trust these lists blindly -- plain stores and read-modify-writes, no atomics
// and no zero-fill on the coloured path -- so a wrong list is a data race on the device that the parity tests see only
// when the race happens to lose.  This program needs no GPU: it is compiled host-only together with csrc/patches.hip
// (tests/test_patch_plans.py, with the address and undefined-behaviour sanitizers), builds plans for meshes it
// generates itself, checks every structural invariant, and then EXECUTES each schedule serially in exact integer
// arithmetic, in several legal orders, against the plain cell-by-cell scatter-add.  The schedule is the library's own:
// the steps of an application (forks, waits, patch and chain launches, records, joins) and the zero-fill rule come from
// the functions the operator's apply walks (patches.hpp for_each_launch_step, zero_fills_output); the checker's own are
// the generic meaning of the steps, the linearisations it draws from that and the serial execution.
//
//   plan_check <group>        run the cases of one group; one line per case, then a summary line with coverage flags
//   plan_check --list         the group names
//   plan_check --mutate       corrupt valid plans one field at a time; every corruption must be reported
//
// Exit status 0 = every case passed (in --mutate: every corruption was detected).
#include "patches.hpp"

#include "brick_partition.hpp"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <numeric>
#include <random>
#include <set>
#include <string>
#include <vector>

namespace pmg
{
// (the library's own live in tables.hip, next to code that needs a GPU)
thread_local std::string g_last_error;
int fail(int code, const char* fmt, ...)
{
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
  std::printf("  pmg::fail(%d): %s\n", code, buf);
  return code;
}
} // namespace pmg

using namespace pmg;

namespace
{
struct Violation
{
  std::string invariant, what;
};
[[noreturn]] void violate(const char* invariant, const char* fmt, ...)
{
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  throw Violation{invariant, buf};
}
#define CHECK(cond, invariant, ...)                                                                                    \
  do                                                                                                                   \
  {                                                                                                                    \
    if (!(cond))                                                                                                       \
      violate(invariant, __VA_ARGS__);                                                                                 \
  } while (0)

// ---- coverage -------------------------------------------------------------------------------------------------------
const char* const FLAGS[] = {"tensor_grouping", "morton_grouping", "halved_group", "halved_group_high_degree",
                             "merged_interior", "coloured_interior", "split_plan", "split_refused", "split_refused_colours",
                             "empty_launch_in_split", "chain_ok", "chain_refused_merged", "chain_refused_split",
                             "chain_refused_grid", "chain_refused_colours", "chain_refused_few_chains",
                             "boundary_only", "interior_only", "single_cell_patch", "ragged_blocks", "below_one_patch",
                             "empty_plan", "zero_all_rule", "bzero_list_rule", "coarse_coloured", "coarse_merged",
                             "coarse_refused", "form_two_calls", "form_whole", "coalesced_step", "fp32_unsplit",
                             "form_chains"};
std::set<std::string> g_cov;
void cover(const char* f) { g_cov.insert(f); }

// ---- meshes ---------------------------------------------------------------------------------------------------------
struct Geo
{
  int n[3] = {0, 0, 0};
  std::vector<std::array<int, 3>> cc; // cell coordinates on the n[0] x n[1] x n[2] grid (empty on a multi-block mesh)
  std::vector<std::array<int32_t, 8>> verts; // multi-block meshes: the cells' vertices, order i*4 + j*2 + k
  int32_t nverts = 0;
  std::vector<float> cen;             // [ncells*3]
  std::vector<int32_t> lcells, bcells;
  bool expect_morton = false;
  int32_t ncells() const { return (int32_t)(verts.empty() ? cc.size() : verts.size()); }
};
struct Space
{
  int P = 0;
  int32_t ndofs = 0;
  std::vector<int32_t> dofmap;
  std::vector<int8_t> bc;
};
enum Lists
{
  ALL_L,
  ALL_B,
  NONE,
  SLAB // the cells of the first x layer are "boundary" cells, the rest "local"
};
enum Bc
{
  BC_NONE,
  BC_SURFACE,
  BC_RANDOM
};

void set_centroids(Geo& g, double jitter, bool twist, uint32_t seed)
{
  std::mt19937 rng(seed);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  g.cen.resize((size_t)3 * g.ncells());
  for (int32_t c = 0; c < g.ncells(); ++c)
  {
    double x[3];
    for (int a = 0; a < 3; ++a)
      x[a] = (g.cc[c][a] + 0.5 + jitter * u(rng)) / g.n[a];
    if (twist)
    {
      const double y0 = x[0] + 0.12 * x[1] * x[2], y1 = x[1] + 0.10 * x[0] * x[2], y2 = x[2] + 0.08 * x[0] * x[1];
      x[0] = y0, x[1] = y1, x[2] = y2;
    }
    for (int a = 0; a < 3; ++a)
      g.cen[(size_t)3 * c + a] = (float)x[a];
  }
}

// hole_pct: that share of the cells is removed at random; shuffle: the cell order is permuted
Geo box_geo(int nx, int ny, int nz, Lists lists, bool shuffle = false, double jitter = 0.0, bool twist = false,
            int hole_pct = 0, uint32_t seed = 1)
{
  Geo g;
  g.n[0] = nx, g.n[1] = ny, g.n[2] = nz;
  std::mt19937 rng(seed * 7919u + 13u);
  for (int i = 0; i < nx; ++i)
    for (int j = 0; j < ny; ++j)
      for (int k = 0; k < nz; ++k)
        if (hole_pct == 0 || (int)(rng() % 100u) >= hole_pct)
          g.cc.push_back({i, j, k});
  if (shuffle)
    std::shuffle(g.cc.begin(), g.cc.end(), rng);
  set_centroids(g, jitter, twist, seed + 101u);
  g.expect_morton = jitter > 0.0 || twist;
  for (int32_t c = 0; c < g.ncells(); ++c)
  {
    if (lists == ALL_L || (lists == SLAB && g.cc[c][0] > 0))
      g.lcells.push_back(c);
    else if (lists == ALL_B || lists == SLAB)
      g.bcells.push_back(c);
  }
  if (shuffle) // the lists need not be ascending either
  {
    std::shuffle(g.lcells.begin(), g.lcells.end(), rng);
    std::shuffle(g.bcells.begin(), g.bcells.end(), rng);
  }
  return g;
}

// continuous tensor space of degree P on the geometry's grid; perm_seed != 0: random dof numbering
Space box_space(const Geo& g, int P, Bc bcmode, uint32_t perm_seed = 0)
{
  Space s;
  s.P = P;
  const int nd = P + 1, N = nd * nd * nd;
  const int64_t m[3] = {(int64_t)g.n[0] * P + 1, (int64_t)g.n[1] * P + 1, (int64_t)g.n[2] * P + 1};
  s.ndofs = (int32_t)(m[0] * m[1] * m[2]);
  std::vector<int32_t> perm(s.ndofs);
  std::iota(perm.begin(), perm.end(), 0);
  if (perm_seed)
  {
    std::mt19937 rng(perm_seed);
    std::shuffle(perm.begin(), perm.end(), rng);
  }
  s.dofmap.resize((size_t)g.ncells() * N);
  for (int32_t c = 0; c < g.ncells(); ++c)
    for (int a = 0; a < nd; ++a)
      for (int b = 0; b < nd; ++b)
        for (int e = 0; e < nd; ++e)
          s.dofmap[(size_t)c * N + (a * nd + b) * nd + e]
              = perm[((g.cc[c][0] * P + a) * m[1] + (g.cc[c][1] * P + b)) * m[2] + g.cc[c][2] * P + e];
  s.bc.assign(s.ndofs, 0);
  std::mt19937 rng(perm_seed + 77u);
  for (int64_t i = 0; i < m[0]; ++i)
    for (int64_t j = 0; j < m[1]; ++j)
      for (int64_t k = 0; k < m[2]; ++k)
      {
        const int32_t d = perm[(i * m[1] + j) * m[2] + k];
        if (bcmode == BC_SURFACE)
          s.bc[d] = i == 0 || j == 0 || k == 0 || i == m[0] - 1 || j == m[1] - 1 || k == m[2] - 1;
        else if (bcmode == BC_RANDOM)
          s.bc[d] = rng() % 10u == 0;
      }
  return s;
}

// every cell with dofs of its own: no two cells share a fine dof
Space discontinuous_space(const Geo& g, int P)
{
  Space s;
  s.P = P;
  const int N = (P + 1) * (P + 1) * (P + 1);
  s.ndofs = g.ncells() * N;
  s.dofmap.resize((size_t)s.ndofs);
  std::iota(s.dofmap.begin(), s.dofmap.end(), 0);
  s.bc.assign(s.ndofs, 0);
  return s;
}

// one rank's brick with its ghost shell (examples/common/brick_partition.hpp); the cell lists by the rule of
// compute_boundary_cells: cells that touch no ghost dof are local, the others and every ghost cell boundary
void brick(int n, std::array<int, 3> dims, int rank, int P, Geo& g, Space& s)
{
  examples::BrickPartition part(n, dims, rank);
  std::vector<double> gll(P + 1);
  for (int i = 0; i <= P; ++i)
    gll[i] = (double)i / P; // (only the dof coordinates depend on it)
  const examples::PartitionLevel lv = part.level(P, gll);
  g = Geo();
  g.n[0] = g.n[1] = g.n[2] = n;
  g.cc = part.cell_coords;
  set_centroids(g, 0.0, false, 1);
  s = Space();
  s.P = P;
  s.ndofs = lv.ndofs();
  s.dofmap = lv.dofmap;
  s.bc = lv.bc_marker;
  const int N = (P + 1) * (P + 1) * (P + 1);
  for (int32_t c = 0; c < part.ncells; ++c)
  {
    bool mark = c >= part.ncells_owned;
    for (int k = 0; !mark && k < N; ++k)
      mark = lv.dofmap[(size_t)c * N + k] >= lv.size_local;
    (mark ? g.bcells : g.lcells).push_back(c);
  }
}

// ---- multi-block meshes ---------------------------------------------------------------------------------------------
// Blocks of mx x my x mz cells each, given by the numbers of their eight corners (order i*4 + j*2 + k) in a list of
// points; blocks that name the same corners meet there, with whatever local axes each of them has.  Everything is
// identified topologically and exactly: a lattice point of a block, and a node of a cell, by its integer trilinear
// weights on the corners it depends on -- the same point seen from two blocks or two cells has the same weights on the
// same corners, whichever way their axes run.
using WeightKey = std::vector<std::pair<int32_t, int32_t>>;
WeightKey weight_key(const int32_t (&corner)[8], int n0, int i0, int n1, int i1, int n2, int i2)
{
  WeightKey key;
  const int w0[2] = {n0 - i0, i0}, w1[2] = {n1 - i1, i1}, w2[2] = {n2 - i2, i2};
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b)
      for (int e = 0; e < 2; ++e)
        if (w0[a] * w1[b] * w2[e] != 0)
          key.push_back({corner[a * 4 + b * 2 + e], w0[a] * w1[b] * w2[e]});
  std::sort(key.begin(), key.end());
  return key;
}

struct BlockMesh
{
  std::vector<std::array<int32_t, 8>> corner; // per block
  std::vector<std::array<double, 3>> x;       // the points the corners name
  int m[3] = {1, 1, 1};
};
enum Map
{
  MAP_NONE,
  MAP_BEND, // x += 0.3 z y: every centroid gets an x of its own
  MAP_TWIST
};

// lists: ALL_L / ALL_B / NONE as for a box; SLAB: the cells of block 0 are "boundary" cells (a partition between blocks)
Geo block_geo(const BlockMesh& bm, Map map, Lists lists, bool shuffle = false, uint32_t seed = 1)
{
  Geo g;
  g.expect_morton = true;
  std::map<WeightKey, int32_t> vertex;
  std::vector<int> block_of;
  std::vector<std::array<double, 3>> centre;
  for (size_t b = 0; b < bm.corner.size(); ++b)
  {
    int32_t cn[8];
    std::copy(bm.corner[b].begin(), bm.corner[b].end(), cn);
    for (int i = 0; i < bm.m[0]; ++i)
      for (int j = 0; j < bm.m[1]; ++j)
        for (int k = 0; k < bm.m[2]; ++k)
        {
          std::array<int32_t, 8> v;
          for (int a = 0; a < 2; ++a)
            for (int e = 0; e < 2; ++e)
              for (int f = 0; f < 2; ++f)
              {
                const WeightKey key = weight_key(cn, bm.m[0], i + a, bm.m[1], j + e, bm.m[2], k + f);
                v[a * 4 + e * 2 + f] = vertex.emplace(key, (int32_t)vertex.size()).first->second;
              }
          g.verts.push_back(v);
          block_of.push_back((int)b);
          const double t[3] = {(i + 0.5) / bm.m[0], (j + 0.5) / bm.m[1], (k + 0.5) / bm.m[2]};
          std::array<double, 3> c = {0, 0, 0};
          for (int a = 0; a < 2; ++a)
            for (int e = 0; e < 2; ++e)
              for (int f = 0; f < 2; ++f)
                for (int d = 0; d < 3; ++d)
                  c[d] += (a ? t[0] : 1 - t[0]) * (e ? t[1] : 1 - t[1]) * (f ? t[2] : 1 - t[2]) * bm.x[cn[a * 4 + e * 2 + f]][d];
          if (map == MAP_BEND)
            c[0] += 0.3 * c[2] * c[1];
          if (map == MAP_TWIST)
            c = {c[0] + 0.12 * c[1] * c[2], c[1] + 0.10 * c[0] * c[2], c[2] + 0.08 * c[0] * c[1]};
          centre.push_back(c);
        }
  }
  g.nverts = (int32_t)vertex.size();
  std::vector<int32_t> order(g.verts.size());
  std::iota(order.begin(), order.end(), 0);
  std::mt19937 rng(seed * 7919u + 13u);
  if (shuffle)
    std::shuffle(order.begin(), order.end(), rng);
  std::vector<std::array<int32_t, 8>> verts(order.size());
  g.cen.resize(3 * order.size());
  for (size_t c = 0; c < order.size(); ++c)
  {
    verts[c] = g.verts[order[c]];
    for (int d = 0; d < 3; ++d)
      g.cen[3 * c + d] = (float)centre[order[c]][d];
    const bool boundary = lists == ALL_B || (lists == SLAB && block_of[order[c]] == 0);
    if (lists != NONE)
      (boundary ? g.bcells : g.lcells).push_back((int32_t)c);
  }
  g.verts.swap(verts);
  if (shuffle)
  {
    std::shuffle(g.lcells.begin(), g.lcells.end(), rng);
    std::shuffle(g.bcells.begin(), g.bcells.end(), rng);
  }
  return g;
}

// k rhombic sectors (0, a_s, a_s + a_{s+1}, a_{s+1}) around the z axis: an edge shared by k cells, vertices of valence 2k
BlockMesh star_blocks(int k, int m, int nz)
{
  BlockMesh bm;
  bm.m[0] = bm.m[1] = m, bm.m[2] = nz;
  const double pi = 3.14159265358979323846;
  // points: 2 on the axis, then per sector a_s and a_s + a_{s+1}, each at z = 0 and z = 1
  bm.x.push_back({0, 0, 0});
  bm.x.push_back({0, 0, 1});
  for (int s = 0; s < k; ++s)
    for (int far = 0; far < 2; ++far)
      for (int z = 0; z < 2; ++z)
      {
        const double a0 = 2 * pi * s / k, a1 = 2 * pi * (s + 1) / k;
        bm.x.push_back({std::cos(a0) + far * std::cos(a1), std::sin(a0) + far * std::sin(a1), (double)z});
      }
  auto ray = [&](int s, int far, int z) { return 2 + ((s % k) * 2 + far) * 2 + z; };
  for (int s = 0; s < k; ++s)
    bm.corner.push_back({0, 1, ray(s + 1, 0, 0), ray(s + 1, 0, 1), ray(s, 0, 0), ray(s, 0, 1), ray(s, 1, 0), ray(s, 1, 1)});
  return bm;
}

// an inner cube and six frusta whose local axis 0 is radial; three of them are left-handed
BlockMesh ogrid_blocks(int m)
{
  BlockMesh bm;
  bm.m[0] = bm.m[1] = bm.m[2] = m;
  for (int shell = 0; shell < 2; ++shell)
    for (int v = 0; v < 8; ++v)
    {
      const double s = shell ? 1.0 : 0.4;
      bm.x.push_back({(2 * ((v >> 2) & 1) - 1) * s, (2 * ((v >> 1) & 1) - 1) * s, (2 * (v & 1) - 1) * s});
    }
  bm.corner.push_back({0, 1, 2, 3, 4, 5, 6, 7});
  for (int axis = 0; axis < 3; ++axis)
    for (int side = 0; side < 2; ++side)
    {
      const int b = axis == 0 ? 1 : 0, c = axis == 2 ? 1 : 2;
      std::array<int32_t, 8> cn;
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j)
          for (int e = 0; e < 2; ++e)
          {
            int bit[3];
            bit[axis] = side, bit[b] = j, bit[c] = e;
            cn[i * 4 + j * 2 + e] = 8 * i + bit[0] * 4 + bit[1] * 2 + bit[2];
          }
      bm.corner.push_back(cn);
    }
  return bm;
}

// a box grid with a re-entrant notch along one vertical edge and one interior cell removed: a tensor grid of centroids
// with gaps, columns of cells that stop and resume
Geo notched_geo(int nx, int ny, int nz, Lists lists, bool shuffle = false, uint32_t seed = 1)
{
  Geo g;
  g.n[0] = nx, g.n[1] = ny, g.n[2] = nz;
  for (int i = 0; i < nx; ++i)
    for (int j = 0; j < ny; ++j)
      for (int k = 0; k < nz; ++k)
      {
        const bool notch = i >= (nx + 1) / 2 && j >= (ny + 1) / 2 && k >= nz / 4 && k < nz / 2;
        const bool hole = i == 1 && j == 1 && k == (3 * nz) / 4;
        if (!notch && !hole)
          g.cc.push_back({i, j, k});
      }
  std::mt19937 rng(seed * 7919u + 13u);
  if (shuffle)
    std::shuffle(g.cc.begin(), g.cc.end(), rng);
  set_centroids(g, 0.0, false, seed);
  for (int32_t c = 0; c < g.ncells(); ++c)
  {
    if (lists == ALL_L || (lists == SLAB && g.cc[c][0] > 0))
      g.lcells.push_back(c);
    else if (lists == ALL_B || lists == SLAB)
      g.bcells.push_back(c);
  }
  return g;
}

// continuous space of degree P on a multi-block mesh; BC_SURFACE: the dofs of the faces that belong to one cell only
Space mesh_space(const Geo& g, int P, Bc bcmode, uint32_t perm_seed = 0)
{
  Space s;
  s.P = P;
  const int nd = P + 1, N = nd * nd * nd;
  std::map<WeightKey, int32_t> dof;
  s.dofmap.resize((size_t)g.ncells() * N);
  for (int32_t c = 0; c < g.ncells(); ++c)
  {
    int32_t v[8];
    std::copy(g.verts[c].begin(), g.verts[c].end(), v);
    for (int a = 0; a < nd; ++a)
      for (int b = 0; b < nd; ++b)
        for (int e = 0; e < nd; ++e)
          s.dofmap[(size_t)c * N + (a * nd + b) * nd + e]
              = dof.emplace(weight_key(v, P, a, P, b, P, e), (int32_t)dof.size()).first->second;
  }
  s.ndofs = (int32_t)dof.size();
  // the count by topology: V + E (P-1) + F (P-1)^2 + C (P-1)^3
  std::set<std::array<int32_t, 2>> edges;
  std::map<std::array<int32_t, 4>, int> faces;
  for (int32_t c = 0; c < g.ncells(); ++c)
    for (int axis = 0; axis < 3; ++axis)
    {
      const int bit = 4 >> axis;
      for (int v = 0; v < 8; ++v)
        if (!(v & bit))
        {
          std::array<int32_t, 2> e = {g.verts[c][v], g.verts[c][v | bit]};
          std::sort(e.begin(), e.end());
          edges.insert(e);
        }
      for (int side = 0; side < 2; ++side)
      {
        std::array<int32_t, 4> f;
        int k = 0;
        for (int v = 0; v < 8; ++v)
          if (((v & bit) != 0) == (side != 0))
            f[k++] = g.verts[c][v];
        std::sort(f.begin(), f.end());
        faces[f]++;
      }
    }
  const long long want = g.nverts + (long long)edges.size() * (P - 1) + (long long)faces.size() * (P - 1) * (P - 1)
                         + (long long)g.ncells() * (P - 1) * (P - 1) * (P - 1);
  CHECK(s.ndofs == want, "mesh generator", "degree %d: %d dofs by identification, %lld by counting", P, s.ndofs, want);
  std::vector<int32_t> perm(s.ndofs);
  std::iota(perm.begin(), perm.end(), 0);
  if (perm_seed)
  {
    std::mt19937 rng(perm_seed);
    std::shuffle(perm.begin(), perm.end(), rng);
  }
  for (int32_t& d : s.dofmap)
    d = perm[d];
  s.bc.assign(s.ndofs, 0);
  if (bcmode == BC_RANDOM)
  {
    std::mt19937 rng(perm_seed + 77u);
    for (int32_t d = 0; d < s.ndofs; ++d)
      s.bc[d] = rng() % 10u == 0;
  }
  else if (bcmode == BC_SURFACE)
    for (int32_t c = 0; c < g.ncells(); ++c)
      for (int axis = 0; axis < 3; ++axis)
        for (int side = 0; side < 2; ++side)
        {
          const int bit = 4 >> axis;
          std::array<int32_t, 4> f;
          int k = 0;
          for (int v = 0; v < 8; ++v)
            if (((v & bit) != 0) == (side != 0))
              f[k++] = g.verts[c][v];
          std::sort(f.begin(), f.end());
          if (faces[f] != 1)
            continue;
          for (int t = 0; t < N; ++t)
          {
            const int idx[3] = {t / (nd * nd), (t / nd) % nd, t % nd};
            if (idx[axis] == (side ? P : 0))
              s.bc[s.dofmap[(size_t)c * N + t]] = 1;
          }
        }
  return s;
}

Space space_of(const Geo& g, int P, Bc bcmode, uint32_t perm_seed = 0)
{
  return g.verts.empty() ? box_space(g, P, bcmode, perm_seed) : mesh_space(g, P, bcmode, perm_seed);
}

// ---- the settings a plan is built under -----------------------------------------------------------------------------
constexpr long long THR_DEFAULT = -1, THR_COLOURED = 0, THR_MERGED = 1LL << 40;
long long g_threshold = THR_DEFAULT;
int g_streams = 0;
void configure(long long threshold, int streams)
{
  g_threshold = threshold;
  g_streams = streams;
  pmg_set_merge_threshold(threshold);
  if (streams > 0)
    setenv("PMG_APPLY_STREAMS", std::to_string(streams).c_str(), 1);
  else
    unsetenv("PMG_APPLY_STREAMS");
}

int build(PatchPlan& pl, const Geo& g, const Space& s)
{
  return build_patch_plan(pl, s.P, g.ncells(), s.dofmap.data(), s.bc.data(), s.ndofs, g.cen.data(), g.lcells.data(),
                          (int32_t)g.lcells.size(), g.bcells.data(), (int32_t)g.bcells.size());
}

// launch index of every patch; checks that the launches tile [0, npatch) in order
std::vector<int32_t> launch_of_patches(const PatchPlan& pl)
{
  const int nl = (int)pl.launch_first.size();
  CHECK(pl.launch_count.size() == (size_t)nl, "launch ranges", "launch_first has %d entries, launch_count %zu", nl,
        pl.launch_count.size());
  std::vector<int32_t> lo(pl.npatch, -1);
  int next = 0;
  for (int l = 0; l < nl; ++l)
  {
    CHECK(pl.launch_first[l] == next && pl.launch_count[l] >= 0, "launch ranges",
          "launch %d starts at patch %d with %d patches, expected start %d", l, pl.launch_first[l], pl.launch_count[l],
          next);
    CHECK(next + pl.launch_count[l] <= pl.npatch, "launch ranges", "launch %d runs past the last patch", l);
    for (int q = 0; q < pl.launch_count[l]; ++q)
      lo[next + q] = l;
    next += pl.launch_count[l];
  }
  CHECK(next == pl.npatch, "launch ranges", "the launches cover %d of %d patches", next, pl.npatch);
  return lo;
}

// ---- the library's schedule ---------------------------------------------------------------------------------------------
// The steps of one operator application come from the library (patches.hpp for_each_launch_step): a sequence of walks
// (l0, l1) under one form, as its callers issue them.  Nothing below restates which steps a plan yields.
struct Application
{
  const char* name;
  std::vector<LaunchStep> steps;
};
enum Walks
{
  TWO_CALLS, // (0, n_launch_l) then (n_launch_l, nl): an application with its halo exchange between the two
  WHOLE      // (0, nl): the timing loop, the single launch of a small level, the FP32 apply
};
Application application(const char* name, const PatchPlan& pl, const ChainPlan* cp, Walks walks, ApplyForm form)
{
  static const std::vector<int32_t> none;
  Application app{name, {}};
  const int nl = (int)pl.launch_first.size();
  auto walk = [&](int l0, int l1) {
    for_each_launch_step(pl, cp ? cp->launch_first : none, cp ? cp->launch_count : none, l0, l1, form,
                         [&](const LaunchStep& st) { return app.steps.push_back(st), 0; });
  };
  if (walks == TWO_CALLS)
  {
    walk(0, pl.n_launch_l);
    walk(pl.n_launch_l, nl);
  }
  else
    walk(0, nl);
  return app;
}
ApplyForm fp64_form(bool chains = false)
{
  ApplyForm f;
  f.two_streams = true;
  f.chains = chains;
  return f;
}

// What a sequence of steps means, whatever rule produced it.  A stream runs its steps in issue order.  The fork makes the
// second stream wait for what the caller's has been given so far, the join the caller's for the second.  A wait for the
// ordering event follows the latest record issued before it; with none it orders nothing.
struct StepOrder
{
  std::vector<std::vector<int>> pred; // direct edges pred[i] -> i
  std::vector<int> on;                // the stream whose order step i joins
};
StepOrder step_order(const std::vector<LaunchStep>& steps)
{
  StepOrder so{std::vector<std::vector<int>>(steps.size()), std::vector<int>(steps.size(), 0)};
  int last[2] = {-1, -1}, recorded = -1;
  for (int i = 0; i < (int)steps.size(); ++i)
  {
    int on = 0, also = -1;
    switch (steps[i].kind)
    {
    case LaunchStep::FORK: on = 1, also = last[0]; break;
    case LaunchStep::JOIN: also = last[1]; break;
    case LaunchStep::WAIT_ORDER: also = recorded; break;
    case LaunchStep::RECORD_ORDER: on = 1, recorded = i; break;
    case LaunchStep::PATCHES: on = steps[i].stream; break;
    case LaunchStep::CHAINS: break;
    }
    if (last[on] >= 0)
      so.pred[i].push_back(last[on]);
    if (also >= 0)
      so.pred[i].push_back(also);
    last[on] = i;
    so.on[i] = on;
  }
  return so;
}

// a linearisation of the steps that the relation allows: steps of stream `prefer` as early as possible
std::vector<int> linearise(const std::vector<LaunchStep>& steps, int prefer)
{
  const int n = (int)steps.size();
  const StepOrder so = step_order(steps);
  std::vector<char> done(n, 0);
  std::vector<int> out;
  while ((int)out.size() < n)
  {
    int pick = -1;
    for (int pass = 0; pass < 2 && pick < 0; ++pass)
      for (int i = 0; i < n && pick < 0; ++i)
      {
        if (done[i] || (pass == 0 && so.on[i] != prefer))
          continue;
        bool ready = true;
        for (int q : so.pred[i])
          ready = ready && done[q];
        if (ready)
          pick = i;
      }
    CHECK(pick >= 0, "two streams", "the step order has a cycle");
    done[pick] = 1;
    out.push_back(pick);
  }
  return out;
}

// Two launch steps that touch a common dof are ordered as their patches are.  (Patches of one plain launch are
// disjoint: checked with the colours.)
void check_ordering(const PatchPlan& pl, int32_t ndofs, const Application& app)
{
  const int n = (int)app.steps.size();
  const StepOrder so = step_order(app.steps);
  std::vector<std::vector<char>> hb(n, std::vector<char>(n, 0));
  for (int i = 0; i < n; ++i) // (edges point forward in issue order: one sweep closes the relation)
    for (int q : so.pred[i])
    {
      hb[q][i] = 1;
      for (int r = 0; r < q; ++r)
        if (hb[r][q])
          hb[r][i] = 1;
    }
  std::vector<int> step_of(pl.npatch, -1);
  for (int i = 0; i < n; ++i)
    if (app.steps[i].kind == LaunchStep::PATCHES)
      for (int p = app.steps[i].first; p < app.steps[i].first + app.steps[i].count; ++p)
      {
        CHECK(p >= 0 && p < pl.npatch && step_of[p] < 0, "schedule", "%s: patch %d is launched twice or out of range",
              app.name, p);
        step_of[p] = i;
      }
  std::vector<int32_t> last_step(ndofs, -1);
  for (int p = 0; p < pl.npatch; ++p)
  {
    CHECK(step_of[p] >= 0, "schedule", "%s: patch %d is never launched", app.name, p);
    for (int i = pl.poff[p]; i < pl.poff[p + 1]; ++i)
    {
      const int32_t d = (int32_t)(pl.pdofs[i] & PD_MASK);
      const int q = last_step[d], t = step_of[p];
      CHECK(q < 0 || q == t || hb[q][t], "two streams: launches that share a dof are ordered",
            "%s: the launches at patches %d and %d both touch dof %d (patch %d) and nothing orders them", app.name,
            app.steps[q].first, app.steps[t].first, d, p);
      last_step[d] = t;
    }
  }
}

// ---- exact arithmetic ------------------------------------------------------------------------------------------------
// integer-valued contributions: every partial sum is an integer far below 2^53, so any order gives the same bits
inline double contrib(int32_t cell, int t) { return (double)(((uint32_t)cell * 31u + (uint32_t)t * 7u) % 13u + 1u); }
inline double xval(int32_t d) { return (double)((uint32_t)d % 17u + 1u); }
inline bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

struct Reference
{
  std::vector<double> y;
  std::vector<char> touched;
  bool all_touched = true;
};
Reference reference_apply(const Geo& g, const Space& s)
{
  Reference r;
  const int N = (s.P + 1) * (s.P + 1) * (s.P + 1);
  r.y.assign(s.ndofs, 0.0);
  r.touched.assign(s.ndofs, 0);
  for (int set = 0; set < 2; ++set)
    for (int32_t c : (set ? g.bcells : g.lcells))
      for (int t = 0; t < N; ++t)
      {
        const int32_t d = s.dofmap[(size_t)c * N + t];
        r.touched[d] = 1;
        if (!s.bc[d])
          r.y[d] += contrib(c, t);
      }
  for (int32_t d = 0; d < s.ndofs; ++d)
  {
    if (r.touched[d] && s.bc[d])
      r.y[d] = xval(d);
    r.all_touched = r.all_touched && r.touched[d];
  }
  return r;
}

enum Order
{
  FORWARD,
  REVERSED,
  SHUFFLED,
  LOCKSTEP, // every patch of the launch gathers before any of them stores (what a full wave of workgroups does)
  N_ORDERS
};
const char* const ORDER_NAME[] = {"forward", "reversed", "shuffled", "lockstep"};

std::vector<int> patch_order(int first, int count, Order o)
{
  std::vector<int> v(count);
  std::iota(v.begin(), v.end(), first);
  if (o == REVERSED)
    std::reverse(v.begin(), v.end());
  if (o == SHUFFLED)
  {
    std::mt19937 rng(12345u + (uint32_t)first);
    std::shuffle(v.begin(), v.end(), rng);
  }
  return v;
}

// the sums of a patch's cells at its dofs, by the local map
void patch_sums(const PatchPlan& pl, int p, std::vector<double>& sum)
{
  const int K = pl.K, N = pl.N, nd = (int)std::lround(std::cbrt((double)N));
  sum.assign(pl.poff[p + 1] - pl.poff[p], 0.0);
  const uint16_t* lm = pl.lmaps.data() + (size_t)pl.lmap_id[p] * K * N;
  for (int sl = 0; sl < pl.pncell[p]; ++sl)
    for (int t = 0; t < N; ++t)
      sum[lm[(size_t)sl * N + table_index(nd, t)]] += contrib(pl.pcell[(size_t)p * K + sl], t);
}

// what an application clears first: everything where the library's rule says so, else the listed dofs
void clear_output(const PatchPlan& pl, const Reference& ref, std::vector<double>& y)
{
  if (zero_fills_output(!ref.all_touched, pl.launch_first.size(), (long long)pl.bzero.size(), (long long)y.size()))
  {
    std::fill(y.begin(), y.end(), 0.0);
    cover("zero_all_rule");
  }
  else
  {
    for (int32_t d : pl.bzero)
      y[d] = 0.0;
    if (!pl.bzero.empty())
      cover("bzero_list_rule");
  }
}

// one launch of the patch kernel (stiffness_column.hpp: the gather of phase 0 and patch_write_back)
void run_patch_launch(const PatchPlan& pl, const LaunchStep& st, Order o, std::vector<double>& y)
{
  const bool atomic_out = st.atomic_out != 0;
  const std::vector<int> order = patch_order(st.first, st.count, o == LOCKSTEP ? FORWARD : o);
  std::vector<std::vector<double>> acc(order.size());
  std::vector<double> sum;
  auto gather = [&](size_t i) {
    const int p = order[i];
    patch_sums(pl, p, sum);
    acc[i].assign(sum.size(), 0.0);
    for (size_t k = 0; k < sum.size(); ++k)
    {
      const uint32_t m = pl.pdofs[pl.poff[p] + k];
      const bool rd = !atomic_out && (m & (PD_ACC | PD_BC)) == PD_ACC;
      acc[i][k] = (rd ? y[m & PD_MASK] : 0.0) + sum[k];
    }
  };
  auto store = [&](size_t i) {
    const int p = order[i];
    for (size_t k = 0; k < acc[i].size(); ++k)
    {
      const uint32_t m = pl.pdofs[pl.poff[p] + k];
      const uint32_t d = m & PD_MASK;
      if (!(m & PD_BC))
      {
        if (atomic_out)
          y[d] += acc[i][k];
        else
          y[d] = acc[i][k];
      }
      else if (!(m & PD_ACC))
        y[d] = xval((int32_t)d);
    }
  };
  if (o == LOCKSTEP)
  {
    for (size_t i = 0; i < order.size(); ++i)
      gather(i);
    for (size_t i = 0; i < order.size(); ++i)
      store(i);
  }
  else
    for (size_t i = 0; i < order.size(); ++i)
    {
      gather(i);
      store(i);
    }
}

void compare(const Reference& ref, const std::vector<double>& y, const char* what, const char* order, int lin)
{
  for (size_t d = 0; d < y.size(); ++d)
    CHECK(same_bits(y[d], ref.y[d]), what, "dof %zu: schedule gives %.17g, the cell-by-cell sum %.17g (%s, patches %s, "
          "linearisation %d)", d, y[d], ref.y[d], ref.touched[d] ? "touched" : "untouched", order, lin);
}

void run_chain_launch(const PatchPlan& pl, const ChainPlan& cp, const LaunchStep& st, Order o, std::vector<double>& y);

// every step of an application, serially: in each linearisation the step order allows and each order of the patches
// inside a launch (a chain is walked in order: no lockstep there)
void interpret(const PatchPlan& pl, const ChainPlan* cp, const Reference& ref, const Application& app)
{
  bool second_stream = false;
  for (const LaunchStep& st : app.steps)
    second_stream = second_stream || st.kind == LaunchStep::FORK;
  const int nlin = second_stream ? 2 : 1;
  for (int lin = 0; lin < nlin; ++lin)
  {
    const std::vector<int> seq = linearise(app.steps, nlin == 1 ? 0 : (lin == 0 ? 1 : 0));
    for (int o = 0; o < (cp ? LOCKSTEP : N_ORDERS); ++o)
    {
      std::vector<double> y(ref.y.size(), std::numeric_limits<double>::quiet_NaN());
      clear_output(pl, ref, y);
      for (int i : seq)
        if (app.steps[i].kind == LaunchStep::PATCHES)
          run_patch_launch(pl, app.steps[i], (Order)o, y);
        else if (app.steps[i].kind == LaunchStep::CHAINS)
          run_chain_launch(pl, *cp, app.steps[i], (Order)o, y);
      compare(ref, y, app.name, ORDER_NAME[o], lin);
    }
  }
}

int count_steps(const Application& app, LaunchStep::Kind kind)
{
  return (int)std::count_if(app.steps.begin(), app.steps.end(), [&](const LaunchStep& st) { return st.kind == kind; });
}

// the forms in which the library walks a plan without chains
std::vector<Application> plan_applications(const PatchPlan& pl)
{
  std::vector<Application> apps;
  apps.push_back(application("serial interpretation", pl, nullptr, TWO_CALLS, fp64_form()));
  cover("form_two_calls");
  apps.push_back(application("serial interpretation of the whole walk", pl, nullptr, WHOLE, fp64_form()));
  cover("form_whole");
  int nonempty = 0;
  for (int32_t c : pl.launch_count)
    nonempty += c > 0;
  if (count_steps(apps.back(), LaunchStep::PATCHES) < nonempty)
    cover("coalesced_step");
  // (a cell list has at most one atomic launch, so neither call of an application finds two to coalesce:
  // pmg_laplacian_launches_per_apply counts these steps and documents one per non-empty launch of the plan)
  CHECK(count_steps(apps[0], LaunchStep::PATCHES) == nonempty, "schedule",
        "the two calls of an application issue %d launches for %d non-empty launches of the plan",
        count_steps(apps[0], LaunchStep::PATCHES), nonempty);
  if (!pl.launch_stream.empty())
  {
    CHECK(count_steps(apps[0], LaunchStep::FORK) == 1 && count_steps(apps[0], LaunchStep::JOIN) == 1
              && count_steps(apps[1], LaunchStep::FORK) == 1 && count_steps(apps[1], LaunchStep::JOIN) == 1,
          "schedule", "a split plan is walked without one fork and one join");
    // the FP32 apply: the same plan, one stream
    apps.push_back(application("serial interpretation of the FP32 walk", pl, nullptr, WHOLE, ApplyForm{}));
    for (const LaunchStep& st : apps.back().steps)
      CHECK(st.kind == LaunchStep::PATCHES && st.stream == 0, "schedule", "the FP32 walk of a split plan is split");
    cover("fp32_unsplit");
  }
  return apps;
}

void interpret_plan(const PatchPlan& pl, const Reference& ref)
{
  for (const Application& app : plan_applications(pl))
    interpret(pl, nullptr, ref, app);
}

// ---- structural invariants of a patch plan ----------------------------------------------------------------------------
void check_plan(const Geo& g, const Space& s, const PatchPlan& pl)
{
  const int P = s.P, nd = P + 1, N = nd * nd * nd;
  const PatchShape shp = patch_shape(P);
  const int K = shp.K(), np = pl.npatch;
  CHECK(pl.K == K && pl.N == N, "sizes", "K = %d, N = %d, expected %d, %d", pl.K, pl.N, K, N);
  CHECK(np >= 0 && pl.pcell.size() == (size_t)np * K && pl.pncell.size() == (size_t)np
            && pl.poff.size() == (size_t)np + 1 && pl.lmap_id.size() == (size_t)np,
        "sizes", "array sizes do not match npatch = %d", np);
  CHECK(pl.lmaps.size() == (size_t)pl.nuniq * K * N, "sizes", "lmaps holds %zu entries for %d maps", pl.lmaps.size(),
        pl.nuniq);

  // cells
  std::vector<int8_t> set_of(g.ncells(), -1);
  for (int32_t c : g.lcells)
    set_of[c] = 0;
  for (int32_t c : g.bcells)
    set_of[c] = 1;
  std::vector<int32_t> slots(g.ncells(), 0);
  std::vector<int8_t> pset(np, -1);
  for (int p = 0; p < np; ++p)
  {
    CHECK(pl.pncell[p] >= 1 && pl.pncell[p] <= K, "cells", "patch %d holds %d cells (K = %d)", p, pl.pncell[p], K);
    for (int sl = 0; sl < K; ++sl)
    {
      const int32_t c = pl.pcell[(size_t)p * K + sl];
      CHECK((c >= 0) == (sl < pl.pncell[p]), "cells: slots are filled cells first",
            "patch %d slot %d holds %d with pncell = %d", p, sl, c, pl.pncell[p]);
      if (c < 0)
        continue;
      CHECK(c < g.ncells() && set_of[c] >= 0, "cells", "patch %d slot %d: cell %d is in neither cell list", p, sl, c);
      slots[c]++;
      CHECK(pset[p] < 0 || pset[p] == set_of[c], "cells", "patch %d mixes cells of both lists (cell %d)", p, c);
      pset[p] = set_of[c];
    }
    CHECK(p == 0 || pset[p - 1] <= pset[p], "cells: lcells patches precede bcells patches",
          "patch %d of the local list follows patch %d of the boundary list", p, p - 1);
    if (pl.pncell[p] == 1)
      cover("single_cell_patch");
  }
  for (int32_t c = 0; c < g.ncells(); ++c)
    CHECK(slots[c] == (set_of[c] >= 0 ? 1 : 0), "cells: every listed cell in exactly one slot",
          "cell %d is in %d patch slots", c, slots[c]);
  int np_l = 0;
  while (np_l < np && pset[np_l] == 0)
    ++np_l;

  // patch dof lists, local maps, Dirichlet flags
  CHECK(pl.poff[0] == 0 && (size_t)pl.poff[np] == pl.pdofs.size(), "poff", "poff spans [%d, %d], pdofs holds %zu",
        pl.poff[0], pl.poff[np], pl.pdofs.size());
  int maxlen = 0;
  std::vector<int32_t> want;
  for (int p = 0; p < np; ++p)
  {
    want.clear();
    for (int sl = 0; sl < pl.pncell[p]; ++sl)
    {
      const int32_t c = pl.pcell[(size_t)p * K + sl];
      want.insert(want.end(), s.dofmap.begin() + (size_t)c * N, s.dofmap.begin() + (size_t)(c + 1) * N);
    }
    std::sort(want.begin(), want.end());
    want.erase(std::unique(want.begin(), want.end()), want.end());
    const int len = pl.poff[p + 1] - pl.poff[p];
    CHECK(len == (int)want.size(), "patch dof list", "patch %d lists %d dofs, its cells have %zu", p, len, want.size());
    for (int i = 0; i < len; ++i)
    {
      const uint32_t m = pl.pdofs[pl.poff[p] + i];
      CHECK((int32_t)(m & PD_MASK) == want[i], "patch dof list: ascending, exactly the dofs of the cells",
            "patch %d entry %d is dof %u, expected %d", p, i, m & PD_MASK, want[i]);
      CHECK(((m & PD_BC) != 0) == (s.bc[want[i]] != 0), "PD_BC", "patch %d entry %d (dof %d): flag %d, marker %d", p, i,
            want[i], (m & PD_BC) != 0, s.bc[want[i]]);
    }
    CHECK(len <= pl.max_M, "max_M", "patch %d lists %d dofs, max_M = %d", p, len, pl.max_M);
    maxlen = std::max(maxlen, len);
    CHECK(pl.lmap_id[p] >= 0 && pl.lmap_id[p] < pl.nuniq, "lmaps", "patch %d: lmap_id %d of %d", p, pl.lmap_id[p],
          pl.nuniq);
    const uint16_t* lm = pl.lmaps.data() + (size_t)pl.lmap_id[p] * K * N;
    for (int sl = 0; sl < pl.pncell[p]; ++sl)
    {
      const int32_t c = pl.pcell[(size_t)p * K + sl];
      for (int t = 0; t < N; ++t)
      {
        const int pos = lm[(size_t)sl * N + table_index(nd, t)];
        CHECK(pos < len && want[pos] == s.dofmap[(size_t)c * N + t], "lmaps",
              "patch %d slot %d node %d: position %d, which is not dof %d", p, sl, t, pos, s.dofmap[(size_t)c * N + t]);
      }
    }
  }
  CHECK(pl.max_M == maxlen && pl.max_M <= shp.max_m, "max_M", "max_M = %d, longest list %d, capacity %d", pl.max_M,
        maxlen, shp.max_m);

  // launches
  const std::vector<int32_t> lo = launch_of_patches(pl);
  const int nl = (int)pl.launch_first.size();
  CHECK(pl.n_launch_l >= 0 && pl.n_launch_l <= nl, "launch ranges", "n_launch_l = %d of %d launches", pl.n_launch_l, nl);
  CHECK((pl.n_launch_l < nl ? pl.launch_first[pl.n_launch_l] : np) == np_l,
        "launch ranges: the first n_launch_l launches hold exactly the lcells patches",
        "they hold %d patches, the local list has %d", pl.n_launch_l < nl ? pl.launch_first[pl.n_launch_l] : np, np_l);
  CHECK(pl.n_plain == 0 || pl.n_plain == pl.n_launch_l, "n_plain", "n_plain = %d, n_launch_l = %d", pl.n_plain,
        pl.n_launch_l);
  CHECK((np_l > 0) == (pl.n_launch_l > 0), "launch ranges", "%d local patches in %d launches", np_l, pl.n_launch_l);

  // colour disjointness and first touchers
  std::vector<int32_t> first_launch(s.ndofs, INT32_MAX), first_patch(s.ndofs, -1), stamp(s.ndofs, -1),
      stamp_patch(s.ndofs, -1), nfirst(s.ndofs, 0);
  for (int p = 0; p < np; ++p)
    for (int i = pl.poff[p]; i < pl.poff[p + 1]; ++i)
    {
      const uint32_t m = pl.pdofs[i];
      const int32_t d = (int32_t)(m & PD_MASK);
      if (lo[p] < pl.n_plain)
      {
        CHECK(stamp[d] != lo[p], "colour disjointness", "patches %d and %d of plain launch %d share dof %d",
              stamp_patch[d], p, lo[p], d);
        stamp[d] = lo[p];
        stamp_patch[d] = p;
      }
      if (first_patch[d] < 0) // (patches are in launch order)
      {
        first_patch[d] = p;
        first_launch[d] = lo[p];
      }
      if (!(m & PD_ACC))
      {
        ++nfirst[d];
        // a merged launch keeps the order of the colours it replaced: the first patch in plan order is the one and
        // only patch of the earliest pre-merge launch
        CHECK(first_patch[d] == p, "first toucher", "patch %d (launch %d) lacks PD_ACC on dof %d, which patch %d "
              "(launch %d) touches first", p, lo[p], d, first_patch[d], first_launch[d]);
      }
    }
  for (int32_t d = 0; d < s.ndofs; ++d)
    CHECK(first_patch[d] < 0 || nfirst[d] == 1, "first toucher: exactly one entry without PD_ACC",
          "dof %d (first patch %d, launch %d) has %d such entries", d, first_patch[d], first_launch[d], nfirst[d]);
  // bzero
  {
    std::vector<int32_t> want_z;
    for (int32_t d = 0; d < s.ndofs; ++d)
      if (first_patch[d] >= 0 && !s.bc[d] && first_launch[d] >= pl.n_plain)
        want_z.push_back(d);
    std::vector<int32_t> got(pl.bzero);
    std::sort(got.begin(), got.end());
    CHECK(std::adjacent_find(got.begin(), got.end()) == got.end(), "bzero: no duplicates", "dof %d is listed twice",
          *std::adjacent_find(got.begin(), got.end()));
    std::vector<int32_t> diff;
    std::set_symmetric_difference(got.begin(), got.end(), want_z.begin(), want_z.end(), std::back_inserter(diff));
    CHECK(diff.empty(), "bzero: exactly the non-Dirichlet dofs whose first toucher is an atomic launch",
          "dof %d is %s (first launch %d, n_plain %d); %zu differences", diff[0],
          std::binary_search(got.begin(), got.end(), diff[0]) ? "listed but should not be" : "missing",
          diff[0] >= 0 && diff[0] < s.ndofs ? first_launch[diff[0]] : -1, pl.n_plain, diff.size());
  }

  // two streams
  if (!pl.launch_stream.empty())
  {
    CHECK(pl.launch_stream.size() == (size_t)nl, "two streams", "launch_stream has %zu entries for %d launches",
          pl.launch_stream.size(), nl);
    CHECK(pl.n_plain == pl.n_launch_l && pl.n_plain > 1, "two streams", "a split plan with a merged interior");
    for (int l = 0; l < nl; ++l)
      CHECK(pl.launch_stream[l] == (l < pl.n_launch_l ? l % 2 : 0), "two streams: launch_stream alternates 0, 1",
            "launch %d is on stream %d", l, pl.launch_stream[l]);
    CHECK(pl.launch_signal >= 0 && pl.launch_signal < pl.n_launch_l && pl.launch_stream[pl.launch_signal] == 1,
          "two streams: launch_signal names a launch of stream 1", "launch_signal = %d", pl.launch_signal);
    CHECK(pl.launch_wait >= 0 && pl.launch_wait < pl.n_launch_l && pl.launch_stream[pl.launch_wait] == 0,
          "two streams: launch_wait names a launch of stream 0", "launch_wait = %d", pl.launch_wait);
    CHECK(pl.launch_signal < pl.launch_wait, "two streams: the event is recorded before it is waited for",
          "launch_signal = %d, launch_wait = %d", pl.launch_signal, pl.launch_wait);
    for (int l = 0; l < pl.n_launch_l; ++l)
      if (pl.launch_count[l] == 0)
        cover("empty_launch_in_split");
  }
  else
    CHECK(pl.launch_signal == -1 && pl.launch_wait == -1, "two streams", "signal / wait set without launch_stream");
  for (const Application& app : plan_applications(pl))
    check_ordering(pl, s.ndofs, app);
}

// ---- chain plan --------------------------------------------------------------------------------------------------------
void check_chain(const Space& s, const PatchPlan& pl, const ChainPlan& cp)
{
  int npi = 0;
  for (int l = 0; l < pl.n_launch_l; ++l)
    npi += pl.launch_count[l];
  CHECK(cp.cdofs.size() == pl.pdofs.size() && cp.ccar.size() == pl.pdofs.size(), "chain sizes",
        "cdofs / ccar hold %zu / %zu entries, pdofs %zu", cp.cdofs.size(), cp.ccar.size(), pl.pdofs.size());
  const int nchain = (int)cp.chain_off.size() - 1;
  CHECK(nchain >= 1 && cp.chain_off[0] == 0 && cp.chain_off[nchain] == npi && (int)cp.chain_patch.size() == npi,
        "chains partition the interior patches", "%d chains over %zu patches, %d interior patches", nchain,
        cp.chain_patch.size(), npi);
  std::vector<int> chain_of(npi, -1), pos_of(npi, -1);
  for (int ch = 0; ch < nchain; ++ch)
  {
    CHECK(cp.chain_off[ch + 1] > cp.chain_off[ch], "chains partition the interior patches", "chain %d is empty", ch);
    for (int i = cp.chain_off[ch]; i < cp.chain_off[ch + 1]; ++i)
    {
      const int p = cp.chain_patch[i];
      CHECK(p >= 0 && p < npi && chain_of[p] < 0, "chains partition the interior patches",
            "chain %d position %d: patch %d is out of range or in two chains", ch, i - cp.chain_off[ch], p);
      chain_of[p] = ch;
      pos_of[p] = i - cp.chain_off[ch];
    }
  }
  const int ncl = (int)cp.launch_first.size();
  CHECK(cp.launch_count.size() == (size_t)ncl && ncl >= 1, "chain launches", "%d / %zu entries", ncl,
        cp.launch_count.size());
  std::vector<int> claunch(nchain, -1);
  int next = 0;
  for (int l = 0; l < ncl; ++l)
  {
    // (no empty colour: the profile of an application counts one kernel launch per chain colour)
    CHECK(cp.launch_first[l] == next && cp.launch_count[l] > 0, "chain launches tile the chains",
          "launch %d starts at chain %d with %d chains, expected start %d", l, cp.launch_first[l], cp.launch_count[l], next);
    for (int q = 0; q < cp.launch_count[l]; ++q)
      claunch[next++] = l;
  }
  CHECK(next == nchain, "chain launches tile the chains", "%d of %d chains", next, nchain);

  // who touches each dof: chains of one launch are disjoint, inside a chain only neighbours share
  std::vector<int32_t> seen_launch(s.ndofs, -1), seen_chain(s.ndofs, -1), seen_pos(s.ndofs, -1),
      first_claunch(s.ndofs, INT32_MAX), nbcfirst(s.ndofs, 0);
  for (int ch = 0; ch < nchain; ++ch)
    for (int c = 0; c < cp.chain_off[ch + 1] - cp.chain_off[ch]; ++c)
    {
      const int p = cp.chain_patch[cp.chain_off[ch] + c];
      for (int i = pl.poff[p]; i < pl.poff[p + 1]; ++i)
      {
        const int32_t d = (int32_t)(pl.pdofs[i] & PD_MASK);
        if (seen_chain[d] == ch)
          CHECK(seen_pos[d] == c - 1 || seen_pos[d] == c, "within a chain only consecutive patches share dofs",
                "chain %d: patches at positions %d and %d share dof %d", ch, seen_pos[d], c, d);
        else
          CHECK(seen_launch[d] != claunch[ch], "no two chains of one launch share a dof",
                "chains %d and %d of chain launch %d share dof %d", seen_chain[d], ch, claunch[ch], d);
        seen_chain[d] = ch;
        seen_pos[d] = c;
        seen_launch[d] = claunch[ch];
        first_claunch[d] = std::min(first_claunch[d], (int32_t)claunch[ch]);
      }
    }
  // the flags, with the meaning stiffness_chain.hpp gives them: a Dirichlet dof is never carried, skipped or read
  for (int p = 0; p < npi; ++p)
  {
    const int ch = chain_of[p], c = pos_of[p], len = cp.chain_off[ch + 1] - cp.chain_off[ch];
    const int prev = c > 0 ? cp.chain_patch[cp.chain_off[ch] + c - 1] : -1;
    const int nxt = c + 1 < len ? cp.chain_patch[cp.chain_off[ch] + c + 1] : -1;
    auto position = [&](int q, uint32_t d) -> int {
      if (q < 0)
        return -1;
      const uint32_t *b = pl.pdofs.data() + pl.poff[q], *e = pl.pdofs.data() + pl.poff[q + 1];
      const uint32_t* it = std::lower_bound(b, e, d, [](uint32_t m, uint32_t v) { return (m & PD_MASK) < v; });
      return it != e && (*it & PD_MASK) == d ? (int)(it - b) : -1;
    };
    for (int i = pl.poff[p]; i < pl.poff[p + 1]; ++i)
    {
      const uint32_t d = pl.pdofs[i] & PD_MASK, v = cp.cdofs[i], w = cp.ccar[i];
      const bool isbc = s.bc[d] != 0;
      CHECK((v & CD_MASK) == d && ((v & CD_BC) != 0) == isbc, "cdofs", "patch %d entry %d: cdofs %#x for dof %u "
            "(Dirichlet %d)", p, i - pl.poff[p], v, d, isbc);
      const int in_prev = position(prev, d), in_next = position(nxt, d);
      CHECK(((v & CD_SKIP) != 0) == (!isbc && in_next >= 0), "CD_SKIP", "chain %d patch %d dof %u: flag %d, next "
            "patch %d %s it", ch, p, d, (v & CD_SKIP) != 0, nxt, in_next >= 0 ? "holds" : "does not hold");
      const uint32_t want_car = (!isbc && in_prev >= 0) ? (uint32_t)in_prev : CC_NONE;
      CHECK((w & 0xffffu) == want_car && (w & ~(CC_ACC | 0xffffu)) == 0, "ccar", "chain %d patch %d dof %u: carry "
            "position %#x, expected %#x (previous patch %d)", ch, p, d, w & 0xffffu, want_car, prev);
      const bool want_acc = !isbc && in_prev < 0 && first_claunch[d] < claunch[ch];
      CHECK(((w & CC_ACC) != 0) == want_acc, "CC_ACC", "chain %d (launch %d) patch %d dof %u: flag %d, first chain "
            "launch of the dof %d, carried %d", ch, claunch[ch], p, d, (w & CC_ACC) != 0, first_claunch[d],
            in_prev >= 0);
      if (v & CD_BCFIRST)
      {
        CHECK(isbc, "CD_BCFIRST", "patch %d: set on dof %u, which is no Dirichlet dof", p, d);
        ++nbcfirst[d];
      }
    }
  }
  for (int32_t d = 0; d < s.ndofs; ++d)
    CHECK(nbcfirst[d] == (s.bc[d] && seen_chain[d] >= 0 ? 1 : 0), "CD_BCFIRST: exactly one entry per Dirichlet dof",
          "dof %d has %d", d, nbcfirst[d]);
}

// one launch of stiffness_chain_kernel: the chains of a step, each walked in order
void run_chain_launch(const PatchPlan& pl, const ChainPlan& cp, const LaunchStep& st, Order o, std::vector<double>& y)
{
  for (int ch : patch_order(st.first, st.count, o))
  {
    const int len = cp.chain_off[ch + 1] - cp.chain_off[ch];
    std::vector<double> prev, cur, sum, ynext;
    auto read_y = [&](int p) { // the gather of a patch is issued before the previous patch's write-back
      ynext.assign(pl.poff[p + 1] - pl.poff[p], 0.0);
      for (size_t k = 0; k < ynext.size(); ++k)
        if (cp.ccar[pl.poff[p] + k] & CC_ACC)
          ynext[k] = y[cp.cdofs[pl.poff[p] + k] & CD_MASK];
    };
    read_y(cp.chain_patch[cp.chain_off[ch]]);
    for (int c = 0; c < len; ++c)
    {
      const int p = cp.chain_patch[cp.chain_off[ch] + c];
      patch_sums(pl, p, sum);
      cur.assign(sum.size(), 0.0);
      for (size_t k = 0; k < sum.size(); ++k)
      {
        const uint32_t w = cp.ccar[pl.poff[p] + k], cpos = w & 0xffffu;
        CHECK(cpos == CC_NONE || cpos < prev.size(), "ccar", "chain %d patch %d entry %zu: carry position %u of %zu",
              ch, p, k, cpos, prev.size());
        cur[k] = ynext[k] + (cpos != CC_NONE ? prev[cpos] : 0.0) + sum[k];
      }
      if (c + 1 < len)
        read_y(cp.chain_patch[cp.chain_off[ch] + c + 1]);
      for (size_t k = 0; k < sum.size(); ++k)
      {
        const uint32_t v = cp.cdofs[pl.poff[p] + k];
        if (!(v & (CD_BC | CD_SKIP)))
          y[v & CD_MASK] = cur[k];
        if (v & CD_BCFIRST)
          y[v & CD_MASK] = xval((int32_t)(v & CD_MASK));
      }
      prev.swap(cur);
    }
  }
}

// the chain form of an application: the library's chain steps in place of the interior launches, then the boundary's
void interpret_chain(const PatchPlan& pl, const ChainPlan& cp, const Reference& ref)
{
  for (Walks walks : {TWO_CALLS, WHOLE})
  {
    const Application app = application("serial interpretation of the chain form", pl, &cp, walks, fp64_form(true));
    CHECK(count_steps(app, LaunchStep::CHAINS) == (int)cp.launch_count.size(), "schedule",
          "%d chain steps for %zu chain colours", count_steps(app, LaunchStep::CHAINS), cp.launch_count.size());
    const int np_l = pl.n_launch_l < (int)pl.launch_first.size() ? pl.launch_first[pl.n_launch_l] : pl.npatch;
    for (const LaunchStep& st : app.steps)
      CHECK(st.kind != LaunchStep::PATCHES || st.first >= np_l, "schedule",
            "the chain form launches the interior patches from %d as well", st.first);
    interpret(pl, &cp, ref, app);
    cover("form_chains");
  }
}

// number of distinct patch positions per axis (tolerance as in build_chain_plan) -- is the interior a tensor grid?
void patch_positions(const Geo& g, const PatchPlan& pl, int npi, int (&npos)[3])
{
  for (int a = 0; a < 3; ++a)
  {
    std::vector<float> v(npi);
    for (int p = 0; p < npi; ++p)
    {
      double sum = 0;
      for (int sl = 0; sl < pl.pncell[p]; ++sl)
        sum += g.cen[(size_t)3 * pl.pcell[(size_t)p * pl.K + sl] + a];
      v[p] = (float)(sum / pl.pncell[p]);
    }
    std::sort(v.begin(), v.end());
    const float tol = 1e-4f * std::max(v.back() - v.front(), 1e-30f);
    int n = 0;
    float last = 0.f;
    for (int p = 0; p < npi; ++p)
      if (p == 0 || v[p] - last > tol)
      {
        ++n;
        last = v[p];
      }
    npos[a] = n;
  }
}
bool interior_is_patch_grid(const Geo& g, const PatchPlan& pl, int npi)
{
  int npos[3];
  patch_positions(g, pl, npi, npos);
  return (long long)npos[0] * npos[1] * npos[2] == npi;
}

// ---- the launches a merged range replaced -------------------------------------------------------------------------
// A merged launch (the boundary list always, the interior of a small level) stands for the colours the builder gave its
// patches; the order of the patches and the PD_ACC flags still follow them.  The flags alone do not tell where one
// colour ends, so the colours are recovered from plans of the same cells that keep them: the interior's from the plan
// built with threshold 0, the boundary list's from a plan that is handed that list as its interior list.  Both must
// reproduce the patches cell for cell.  With that index: no two patches of one pre-merge launch share a dof, and an
// entry lacks PD_ACC exactly when its pre-merge launch is the earliest that touches the dof.
void check_plan(const Geo& g, const Space& s, const PatchPlan& pl);
void check_premerge(const Geo& g, const Space& s, const PatchPlan& pl)
{
  const std::vector<int32_t> lo = launch_of_patches(pl);
  const int np = pl.npatch, nl = (int)pl.launch_first.size(), K = pl.K;
  const int np_l = pl.n_launch_l < nl ? pl.launch_first[pl.n_launch_l] : np;
  std::vector<int32_t> pre(np, -1);
  const long long thr = g_threshold;
  const int streams = g_streams;
  int base = 0;
  if (pl.n_plain > 0 || np_l == 0)
  {
    for (int p = 0; p < np_l; ++p)
      pre[p] = lo[p];
    base = pl.n_launch_l;
  }
  else
  {
    PatchPlan col;
    configure(THR_COLOURED, 0);
    const int rc = build(col, g, s);
    configure(thr, streams);
    CHECK(rc == PMG_OK, "build_patch_plan", "the coloured twin failed: %s", g_last_error.c_str());
    CHECK(col.pcell == pl.pcell && col.poff == pl.poff && col.pdofs == pl.pdofs && col.lmap_id == pl.lmap_id,
          "merged plan equals the coloured plan up to its launch list", "patches, lists or flags differ");
    check_plan(g, s, col); // (its interior launches are plain: their disjointness is checked there)
    const std::vector<int32_t> clo = launch_of_patches(col);
    for (int p = 0; p < np_l; ++p)
      pre[p] = clo[p];
    base = col.n_launch_l;
  }
  if (np_l < np)
  {
    Geo gb = g;
    gb.lcells = g.bcells;
    gb.bcells.clear();
    PatchPlan twin;
    configure(THR_COLOURED, 0);
    const int rc = build(twin, gb, s);
    configure(thr, streams);
    CHECK(rc == PMG_OK, "build_patch_plan", "the boundary list as an interior list failed: %s", g_last_error.c_str());
    CHECK(twin.npatch == np - np_l
              && std::equal(twin.pcell.begin(), twin.pcell.end(), pl.pcell.begin() + (size_t)np_l * K),
          "pre-merge launches", "the boundary list alone gives other patches (%d against %d)", twin.npatch, np - np_l);
    const std::vector<int32_t> tlo = launch_of_patches(twin);
    CHECK(twin.n_plain == twin.n_launch_l, "pre-merge launches", "the twin of the boundary list is merged");
    for (int p = np_l; p < np; ++p)
      pre[p] = base + tlo[p - np_l];
  }
  std::vector<int32_t> stamp(s.ndofs, -1), stamp_patch(s.ndofs, -1), first(s.ndofs, INT32_MAX);
  for (int p = 0; p < np; ++p)
  {
    CHECK(p == 0 || pre[p - 1] <= pre[p], "pre-merge launches", "patch %d (pre-merge launch %d) follows patch %d (%d)",
          p, pre[p], p - 1, pre[p - 1]);
    for (int i = pl.poff[p]; i < pl.poff[p + 1]; ++i)
    {
      const int32_t d = (int32_t)(pl.pdofs[i] & PD_MASK);
      CHECK(stamp[d] != pre[p], "colour disjointness before the merge",
            "patches %d and %d of pre-merge launch %d (launch %d of the plan) share dof %d", stamp_patch[d], p, pre[p],
            lo[p], d);
      stamp[d] = pre[p];
      stamp_patch[d] = p;
      first[d] = std::min(first[d], pre[p]);
    }
  }
  for (int p = 0; p < np; ++p)
    for (int i = pl.poff[p]; i < pl.poff[p + 1]; ++i)
    {
      const int32_t d = (int32_t)(pl.pdofs[i] & PD_MASK);
      CHECK(((pl.pdofs[i] & PD_ACC) == 0) == (first[d] == pre[p]), "first toucher: in the earliest pre-merge launch",
            "patch %d (pre-merge launch %d) dof %d: PD_ACC %d, earliest pre-merge launch %d", p, pre[p], d,
            (pl.pdofs[i] & PD_ACC) != 0, first[d]);
    }
}

enum ChainExpect
{
  CH_NOT_TRIED,
  CH_OK,
  CH_REFUSE_MERGED,
  CH_REFUSE_SPLIT,
  CH_REFUSE_GRID,
  CH_REFUSE_COLOURS,
  CH_REFUSE_FEW,
  CH_ANY // accepted or refused: whichever it is, it is classified, checked as that and reported
};
constexpr int PRODUCTION_MIN_CHAINS = (256 * 3) / 4; // laplacian.hip: three quarters of the compute units

void run_chain(const Geo& g, const Space& s, const PatchPlan& pl, const Reference& ref, ChainExpect expect,
               int min_chains)
{
  ChainPlan cp;
  CHECK(build_chain_plan(cp, pl, s.ndofs, s.bc.data(), g.cen.data(), min_chains) == PMG_OK, "build_chain_plan",
        "it failed: %s", g_last_error.c_str());
  int npi = 0;
  for (int l = 0; l < pl.n_launch_l; ++l)
    npi += pl.launch_count[l];
  if (expect == CH_ANY)
  {
    const bool col = pl.n_plain > 1 && pl.n_plain == pl.n_launch_l;
    if (cp.ok)
      expect = CH_OK;
    else if (!pl.launch_stream.empty())
      expect = CH_REFUSE_SPLIT;
    else if (!col)
      expect = CH_REFUSE_MERGED;
    else if (!interior_is_patch_grid(g, pl, npi))
      expect = CH_REFUSE_GRID;
    else
    {
      // as many positions as patches, and still refused: two patches at one position, patches of a chain that share
      // dofs without being neighbours, or too many chain colours -- the builder keeps the patch form in each case
      std::printf("     chain plan: refused on a patch grid\n");
      return;
    }
    static const char* const what[] = {"", "accepted", "refused: merged level", "refused: split plan",
                                       "refused: no patch grid"};
    std::printf("     chain plan: %s (%zu chain launches for %d patch colours)\n", what[expect], cp.launch_first.size(),
                pl.n_plain);
  }
  CHECK(cp.ok == (expect == CH_OK), "chain plan: accepted or refused as expected", "ok = %d, expectation %d "
        "(n_plain %d, n_launch_l %d, split %d, %d interior patches, min_chains %d)", cp.ok, expect, pl.n_plain,
        pl.n_launch_l, !pl.launch_stream.empty(), npi, min_chains);
  const bool coloured = pl.n_plain > 1 && pl.n_plain == pl.n_launch_l, split = !pl.launch_stream.empty();
  switch (expect)
  {
  case CH_OK:
    CHECK(coloured && !split, "chain plan", "accepted on a merged or split level");
    check_chain(s, pl, cp);
    interpret_chain(pl, cp, ref);
    CHECK((int)cp.launch_first.size() < pl.n_plain, "chain plan: fewer launches than patch colours", "%zu against %d",
          cp.launch_first.size(), pl.n_plain);
    for (int32_t n : cp.launch_count)
      CHECK(n >= min_chains, "chain plan: min_chains", "a launch of %d chains, min_chains = %d", n, min_chains);
    cover("chain_ok");
    break;
  case CH_REFUSE_MERGED:
    CHECK(!coloured && !split, "chain refusal", "the level is not merged");
    cover("chain_refused_merged");
    break;
  case CH_REFUSE_SPLIT:
    CHECK(split, "chain refusal", "the plan is not split");
    cover("chain_refused_split");
    break;
  case CH_REFUSE_GRID:
    CHECK(coloured && !split && !interior_is_patch_grid(g, pl, npi), "chain refusal",
          "the patches do form a tensor grid");
    cover("chain_refused_grid");
    break;
  case CH_REFUSE_COLOURS:
  case CH_REFUSE_FEW:
  {
    CHECK(coloured && !split && interior_is_patch_grid(g, pl, npi), "chain refusal", "another refusal applies");
    // the same plan is accepted / refused when only min_chains changes
    ChainPlan other;
    build_chain_plan(other, pl, s.ndofs, s.bc.data(), g.cen.data(), 1);
    CHECK(other.ok == (expect == CH_REFUSE_FEW), "chain refusal", "with min_chains = 1 ok = %d", other.ok);
    cover(expect == CH_REFUSE_FEW ? "chain_refused_few_chains" : "chain_refused_colours");
    break;
  }
  default:
    break;
  }
}

// ---- coarse lists of the transfers --------------------------------------------------------------------------------------
int build_coarse(CoarsePlan& cp, const Geo& g, const Space& coarse, const PatchPlan& pl)
{
  const int Nc = (coarse.P + 1) * (coarse.P + 1) * (coarse.P + 1);
  return build_coarse_plan(cp, pl.K, Nc, pl.npatch, pl.pcell.data(), pl.pncell.data(), pl.launch_first,
                           pl.launch_count, pl.n_plain, g.ncells(), coarse.dofmap.data(), coarse.ndofs);
}

void check_coarse(const Geo& g, const Space& coarse, const PatchPlan& pl, const CoarsePlan& cp)
{
  const int Nc = (coarse.P + 1) * (coarse.P + 1) * (coarse.P + 1), K = pl.K, np = pl.npatch;
  const std::vector<int32_t> lo = launch_of_patches(pl);
  CHECK(cp.cpoff.size() == (size_t)np + 1 && cp.clmap_id.size() == (size_t)np && cp.cpoff[0] == 0
            && (size_t)cp.cpoff[np] == cp.cpdofs.size() && cp.clmaps.size() % ((size_t)K * Nc) == 0,
        "coarse sizes", "array sizes do not match npatch = %d", np);
  const int nuniq = (int)(cp.clmaps.size() / ((size_t)K * Nc));
  std::vector<int32_t> first(coarse.ndofs, INT32_MAX), want;
  int cmax = 1;
  for (int pass = 0; pass < 2; ++pass)
    for (int p = 0; p < np; ++p)
    {
      want.clear();
      for (int sl = 0; sl < pl.pncell[p]; ++sl)
      {
        const int32_t c = pl.pcell[(size_t)p * K + sl];
        want.insert(want.end(), coarse.dofmap.begin() + (size_t)c * Nc, coarse.dofmap.begin() + (size_t)(c + 1) * Nc);
      }
      std::sort(want.begin(), want.end());
      want.erase(std::unique(want.begin(), want.end()), want.end());
      if (pass == 0)
      {
        for (int32_t d : want)
          first[d] = std::min(first[d], lo[p]);
        cmax = std::max(cmax, (int)want.size());
        continue;
      }
      const int len = cp.cpoff[p + 1] - cp.cpoff[p];
      CHECK(len == (int)want.size(), "coarse list", "patch %d lists %d coarse dofs, its cells have %zu", p, len,
            want.size());
      for (int i = 0; i < len; ++i)
      {
        const uint32_t m = cp.cpdofs[cp.cpoff[p] + i];
        CHECK((int32_t)(m & PD_MASK) == want[i] && !(m & PD_BC), "coarse list: sorted, unique, exactly the dofs of the "
              "cells", "patch %d entry %d is %#x, expected dof %d", p, i, m, want[i]);
        CHECK(((m & PD_ACC) != 0) == (first[want[i]] < lo[p]), "coarse PD_ACC: set exactly when an earlier launch "
              "touched the dof", "patch %d (launch %d) dof %d: flag %d, first launch %d", p, lo[p], want[i],
              (m & PD_ACC) != 0, first[want[i]]);
      }
      CHECK(cp.clmap_id[p] >= 0 && cp.clmap_id[p] < nuniq, "clmaps", "patch %d: clmap_id %d of %d", p, cp.clmap_id[p],
            nuniq);
      const uint16_t* lm = cp.clmaps.data() + (size_t)cp.clmap_id[p] * K * Nc;
      for (int sl = 0; sl < pl.pncell[p]; ++sl)
        for (int k = 0; k < Nc; ++k)
        {
          const int pos = lm[(size_t)sl * Nc + k];
          const int32_t d = coarse.dofmap[(size_t)pl.pcell[(size_t)p * K + sl] * Nc + k];
          CHECK(pos < len && want[pos] == d, "clmaps", "patch %d slot %d node %d: position %d, which is not dof %d", p,
                sl, k, pos, d);
        }
    }
  CHECK(cp.cmax == cmax, "cmax", "cmax = %d, longest coarse list %d", cp.cmax, cmax);

  // the restriction, serially and exactly: the transpose scatter-add of integer weights
  std::vector<double> ref(coarse.ndofs, 0.0);
  for (int set = 0; set < 2; ++set)
    for (int32_t c : (set ? g.bcells : g.lcells))
      for (int k = 0; k < Nc; ++k)
        ref[coarse.dofmap[(size_t)c * Nc + k]] += contrib(c, k);
  const int nl = (int)pl.launch_first.size();
  std::vector<double> sum;
  auto sums = [&](int p) {
    sum.assign(cp.cpoff[p + 1] - cp.cpoff[p], 0.0);
    const uint16_t* lm = cp.clmaps.data() + (size_t)cp.clmap_id[p] * K * Nc;
    for (int sl = 0; sl < pl.pncell[p]; ++sl)
      for (int k = 0; k < Nc; ++k)
        sum[lm[(size_t)sl * Nc + k]] += contrib(pl.pcell[(size_t)p * K + sl], k);
  };
  for (int form = 0; form < 2; ++form) // 0: coloured (plain launches store), 1: merged (zero-fill, every patch adds)
    for (int o = 0; o < N_ORDERS; ++o)
    {
      // (zero-filled first in both forms: interpolate.hip launch_zero; the coloured launches must not rely on it)
      std::vector<double> y(coarse.ndofs, 0.0);
      if (form == 0)
        for (int p = 0; p < np; ++p)
          if (lo[p] < pl.n_plain)
            for (int i = cp.cpoff[p]; i < cp.cpoff[p + 1]; ++i)
              y[cp.cpdofs[i] & PD_MASK] = std::numeric_limits<double>::quiet_NaN();
      for (int l = 0; l < nl; ++l)
      {
        const bool atomic_out = form == 1 || l >= pl.n_plain;
        const std::vector<int> order = patch_order(pl.launch_first[l], pl.launch_count[l], o == LOCKSTEP ? FORWARD : (Order)o);
        std::vector<std::vector<double>> acc(order.size());
        auto gather = [&](size_t i) {
          const int p = order[i];
          sums(p);
          acc[i] = sum;
          for (size_t k = 0; k < sum.size(); ++k)
          {
            const uint32_t m = cp.cpdofs[cp.cpoff[p] + k];
            if (!atomic_out && (m & PD_ACC))
              acc[i][k] += y[m & PD_MASK];
          }
        };
        auto store = [&](size_t i) {
          const int p = order[i];
          for (size_t k = 0; k < acc[i].size(); ++k)
          {
            const uint32_t d = cp.cpdofs[cp.cpoff[p] + k] & PD_MASK;
            if (atomic_out)
              y[d] += acc[i][k];
            else
              y[d] = acc[i][k];
          }
        };
        if (o == LOCKSTEP)
        {
          for (size_t i = 0; i < order.size(); ++i)
            gather(i);
          for (size_t i = 0; i < order.size(); ++i)
            store(i);
        }
        else
          for (size_t i = 0; i < order.size(); ++i)
          {
            gather(i);
            store(i);
          }
      }
      for (int32_t d = 0; d < coarse.ndofs; ++d)
        CHECK(same_bits(y[d], ref[d]), form ? "serial interpretation of the merged restriction"
                                            : "serial interpretation of the coloured restriction",
              "coarse dof %d: schedule gives %.17g, the transpose scatter-add %.17g (patches %s)", d, y[d], ref[d],
              ORDER_NAME[o]);
    }
  cover(pl.n_plain > 0 ? "coarse_coloured" : "coarse_merged");
}

// ---- cases -----------------------------------------------------------------------------------------------------------
struct Case
{
  std::string name;
  Geo g;
  Space s;
  long long threshold = THR_DEFAULT;
  int streams = 0;
  ChainExpect chain = CH_NOT_TRIED;
  int min_chains = 1;
  std::vector<int> coarse_degrees; // transfers from these degrees to s.P
  uint32_t coarse_perm = 0;
  bool expect_split = false, expect_split_refused = false, expect_split_refused_colours = false;
  bool observe = false; // no expectation about the split: what the builder decides is checked and reported
};

void note_coverage(const Case& c, const PatchPlan& pl)
{
  const PatchShape shp = patch_shape(c.s.P);
  const int K = shp.K();
  int full_blocks = 0, full_other = 0, shorter[2] = {0, 0}, np_l = 0;
  for (int p = 0; p < pl.npatch; ++p)
  {
    int lo[3] = {1 << 30, 1 << 30, 1 << 30}, hi[3] = {-1, -1, -1};
    for (int sl = 0; sl < (c.g.cc.empty() ? 0 : pl.pncell[p]); ++sl)
      for (int a = 0; a < 3; ++a)
      {
        lo[a] = std::min(lo[a], c.g.cc[pl.pcell[(size_t)p * K + sl]][a]);
        hi[a] = std::max(hi[a], c.g.cc[pl.pcell[(size_t)p * K + sl]][a]);
      }
    const bool block = hi[0] - lo[0] + 1 == shp.bx && hi[1] - lo[1] + 1 == shp.by && hi[2] - lo[2] + 1 == shp.bz;
    const bool local = p < (pl.n_launch_l < (int)pl.launch_first.size() ? pl.launch_first[pl.n_launch_l] : pl.npatch);
    np_l += local;
    if (pl.pncell[p] == K)
      (block ? full_blocks : full_other)++;
    else
      shorter[local ? 0 : 1]++;
  }
  if (!c.g.expect_morton && K > 1 && full_blocks > 0 && full_other == 0)
    cover("tensor_grouping");
  // (the blocks of an axis are balanced: a size that the patch shape does not divide shortens all of them)
  if (!c.g.expect_morton && K > 1 && c.g.ncells() > K && shorter[0] + shorter[1] > 0)
    cover("ragged_blocks");
  if (c.g.expect_morton && K > 1 && full_other > 0)
    cover("morton_grouping");
  // Morton chunks hold exactly K cells except the last of a list: a second short patch is a halved group
  if (c.g.expect_morton && K > 1 && (shorter[0] > 1 || shorter[1] > 1))
  {
    cover("halved_group");
    if (c.s.P >= 5)
      cover("halved_group_high_degree");
  }
  if (pl.npatch > 0 && c.g.ncells() < K && full_blocks + full_other == 0)
    cover("below_one_patch");
  if (pl.npatch == 0)
    cover("empty_plan");
  if (pl.npatch > 0 && np_l == 0)
    cover("boundary_only");
  if (pl.npatch > 0 && np_l == pl.npatch)
    cover("interior_only");
  if (pl.n_plain == 0 && np_l > 1)
    cover("merged_interior");
  if (pl.n_plain > 1)
    cover("coloured_interior");
  if (!pl.launch_stream.empty() && pl.launch_signal > 1 && pl.launch_wait > 0)
    cover("split_plan");
}

void run_case(const Case& c)
{
  configure(c.threshold, c.streams);
  PatchPlan pl;
  CHECK(build(pl, c.g, c.s) == PMG_OK, "build_patch_plan", "it failed: %s", g_last_error.c_str());
  check_plan(c.g, c.s, pl);
  const Reference ref = reference_apply(c.g, c.s);
  interpret_plan(pl, ref);
  note_coverage(c, pl);
  if (c.expect_split)
    CHECK(!pl.launch_stream.empty(), "case", "the plan was expected to be split over two streams");
  if (c.expect_split_refused)
  {
    CHECK(pl.launch_stream.empty() && c.streams == 2 && pl.n_plain > 1, "case", "the split was expected to be refused");
    cover("split_refused");
  }
  check_premerge(c.g, c.s, pl);
  if (c.streams == 2 && pl.launch_stream.empty() && pl.n_plain > 1)
  {
    // Was the split attempted and refused by the colours (kb >= ka in build_patch_plan)?  It is attempted on a coloured
    // level with at least 16 interior patches and four distinct patch positions along some axis; the cut between the two
    // middle positions leaves both halves non-empty, so only the colour test can have refused it.
    int npi = 0, npos[3];
    for (int l = 0; l < pl.n_launch_l; ++l)
      npi += pl.launch_count[l];
    patch_positions(c.g, pl, npi, npos);
    const bool attempted = npi >= 16 && std::max(npos[0], std::max(npos[1], npos[2])) >= 4;
    if (attempted)
      cover("split_refused_colours");
    else if (c.observe)
      cover("split_refused");
    if (c.expect_split_refused_colours)
      CHECK(attempted, "case", "the split was expected to be attempted: %d interior patches, %d x %d x %d positions",
            npi, npos[0], npos[1], npos[2]);
  }
  else if (c.expect_split_refused_colours)
    violate("case", "the split was expected to be refused by the colours");
  if (c.chain != CH_NOT_TRIED)
    run_chain(c.g, c.s, pl, ref, c.chain, c.min_chains);
  for (int pc : c.coarse_degrees)
  {
    const Space coarse = space_of(c.g, pc, BC_NONE, c.coarse_perm);
    CoarsePlan cp;
    CHECK(build_coarse(cp, c.g, coarse, pl) == PMG_OK, "build_coarse_plan", "degrees %d -> %d: %s", pc, c.s.P,
          g_last_error.c_str());
    check_coarse(c.g, coarse, pl, cp);
  }
  std::printf("ok   %-44s P=%d cells=%d patches=%d launches=%zu n_plain=%d split=%d bzero=%zu\n", c.name.c_str(),
              c.s.P, c.g.ncells(), pl.npatch, pl.launch_first.size(), pl.n_plain, !pl.launch_stream.empty(),
              pl.bzero.size());
}

Case mk(std::string name, Geo g, Space s, long long thr = THR_DEFAULT, int streams = 0)
{
  Case c;
  c.name = std::move(name);
  c.g = std::move(g);
  c.s = std::move(s);
  c.threshold = thr;
  c.streams = streams;
  return c;
}

std::string nm(const char* fmt, ...)
{
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return buf;
}

// a mesh of px x py x pz whole patches of degree P
Geo patches_geo(int P, int px, int py, int pz, Lists lists, bool shuffle = false)
{
  const PatchShape sh = patch_shape(P);
  return box_geo(px * sh.bx, py * sh.by, pz * sh.bz, lists, shuffle);
}

const char* const GROUPS[] = {"boxes", "permuted", "irregular", "lists", "coloured", "split", "chains", "transfers",
                              "chains_production", "multiblock"};

std::vector<Case> cases_of(const std::string& group)
{
  std::vector<Case> v;
  const long long THR[3] = {THR_DEFAULT, THR_COLOURED, THR_MERGED};
  const char* const THRN[3] = {"default", "coloured", "merged"};
  if (group == "boxes")
  {
    // every degree: whole patches, ragged last blocks, less than one patch; the three thresholds and markers in turn
    for (int P = 1; P <= 8; ++P)
    {
      const PatchShape sh = patch_shape(P);
      const int k = P % 3;
      {
        Geo g = patches_geo(P, 2, 2, 2, ALL_L);
        v.push_back(mk(nm("box whole patches P%d %s", P, THRN[k]), g, box_space(g, P, (Bc)(P % 3)), THR[k]));
      }
      {
        Geo g = box_geo(sh.bx + 1, 2 * sh.by + 1, sh.bz + (sh.bz > 2 ? sh.bz / 2 : 1), ALL_L);
        v.push_back(mk(nm("box ragged P%d %s", P, THRN[(k + 1) % 3]), g, box_space(g, P, (Bc)((P + 1) % 3)),
                       THR[(k + 1) % 3]));
      }
      {
        Geo g = box_geo(1, 1, sh.bz > 1 ? sh.bz - 1 : 1, ALL_L);
        v.push_back(mk(nm("box below one patch P%d", P), g, box_space(g, P, BC_SURFACE), THR[(k + 2) % 3]));
      }
    }
    Geo g1 = box_geo(1, 1, 1, ALL_L);
    v.push_back(mk("one cell P1", g1, box_space(g1, 1, BC_NONE)));
    v.push_back(mk("one cell P8 boundary list", box_geo(1, 1, 1, ALL_B), box_space(g1, 8, BC_SURFACE)));
  }
  else if (group == "permuted")
  {
    for (int P : {1, 2, 4, 5, 7})
      for (int mode = 1; mode <= 3; ++mode) // shuffled cells, permuted dofs, both
      {
        const PatchShape sh = patch_shape(P);
        Geo g = box_geo(sh.bx + 1, 2 * sh.by, sh.bz + 1, P == 4 ? SLAB : ALL_L, (mode & 1) != 0, 0.0, false, 0, 40 + P);
        v.push_back(mk(nm("box %s%s P%d", mode & 1 ? "cells shuffled " : "", mode & 2 ? "dofs permuted" : "", P), g,
                       box_space(g, P, (Bc)(mode % 3), mode & 2 ? 900 + P : 0), THR[(P + mode) % 3]));
      }
  }
  else if (group == "irregular")
  {
    // jittered / twisted centroids and holes: the Morton path; scattered chunks exceed max_m and are halved
    {
      Geo g = box_geo(8, 8, 24, ALL_L, true, 0.3, false, 40, 3);
      v.push_back(mk("P1 jitter + holes: halved Morton chunks", g, box_space(g, 1, BC_RANDOM, 31), THR_COLOURED));
    }
    {
      Geo g = box_geo(8, 8, 24, SLAB, false, 0.3, false, 40, 4);
      v.push_back(mk("P1 jitter + holes, two lists, merged", g, box_space(g, 1, BC_SURFACE), THR_MERGED));
    }
    {
      Geo g = box_geo(4, 4, 9, ALL_L, false, 0.3, false, 35, 5);
      v.push_back(mk("P5 jitter + holes: halved", g, box_space(g, 5, BC_RANDOM, 55), THR_COLOURED));
    }
    {
      Geo g = box_geo(3, 3, 7, ALL_L, true, 0.25, false, 30, 6);
      v.push_back(mk("P7 jitter + holes", g, box_space(g, 7, BC_NONE), THR_DEFAULT));
    }
    {
      Geo g = box_geo(4, 5, 9, ALL_L, false, 0.0, true, 0, 7);
      v.push_back(mk("P4 twisted centroids", g, box_space(g, 4, BC_SURFACE), THR_COLOURED));
    }
    {
      Geo g = box_geo(5, 4, 17, SLAB, false, 0.0, true, 20, 8);
      v.push_back(mk("P2 twisted centroids + holes, two lists", g, box_space(g, 2, BC_RANDOM, 71), THR_DEFAULT));
    }
    {
      Geo g = box_geo(4, 4, 16, ALL_L, false, 0.0, false, 25, 9); // holes only: still a tensor grid of centroids
      v.push_back(mk("P3 holes on a tensor grid", g, box_space(g, 3, BC_SURFACE), THR_COLOURED));
    }
    {
      Geo g = box_geo(3, 3, 8, ALL_B, true, 0.3, false, 30, 10);
      v.push_back(mk("P6 jitter + holes, boundary list only", g, box_space(g, 6, BC_RANDOM, 12), THR_DEFAULT));
    }
  }
  else if (group == "lists")
  {
    // bricks with their ghost shells, as a 1x1x2, 2x1x1 and 2x2x2 decomposition hands them over
    const std::array<int, 3> dims[3] = {{1, 1, 2}, {2, 1, 1}, {2, 2, 2}};
    int i = 0;
    for (const auto& d : dims)
      for (int P : {1, 3, 4, 6})
      {
        const int size = d[0] * d[1] * d[2];
        Case c;
        c.name = nm("brick %dx%dx%d rank %d P%d %s", d[0], d[1], d[2], size - 1 - (i % 2), P, THRN[i % 3]);
        brick(P <= 2 ? 10 : 6, d, size - 1 - (i % 2), P, c.g, c.s);
        c.threshold = THR[i % 3];
        ++i;
        v.push_back(c);
      }
    for (int P : {2, 4, 5, 8})
    {
      Geo gl = patches_geo(P, 2, 1, 2, ALL_L), gb = patches_geo(P, 2, 1, 2, ALL_B), gn = patches_geo(P, 1, 1, 1, NONE);
      v.push_back(mk(nm("empty bcells P%d", P), gl, box_space(gl, P, BC_SURFACE), THR[P % 3]));
      v.push_back(mk(nm("empty lcells P%d", P), gb, box_space(gb, P, BC_SURFACE), THR[(P + 1) % 3]));
      v.push_back(mk(nm("both lists empty P%d", P), gn, box_space(gn, P, BC_RANDOM)));
    }
    Geo gs = box_geo(6, 5, 9, SLAB, true, 0.0, false, 0, 21);
    v.push_back(mk("slab of boundary cells P4 shuffled", gs, box_space(gs, 4, BC_RANDOM, 5), THR_COLOURED));
  }
  else if (group == "coloured")
  {
    // threshold 0 and at least two patches per axis: eight colours launched one by one
    for (int P : {1, 2, 4, 6, 8})
      for (int b = 0; b < 3; ++b)
      {
        Geo g = patches_geo(P, 2, 2 + (b == 1), 2 + (b == 2), b == 2 ? SLAB : ALL_L, b == 1);
        v.push_back(mk(nm("coloured %dx%dx%d cells P%d bc %d", g.n[0], g.n[1], g.n[2], P, b), g,
                       box_space(g, P, (Bc)b, b == 1 ? 17 + P : 0), THR_COLOURED));
      }
  }
  else if (group == "split")
  {
    // PMG_APPLY_STREAMS=2: at least 16 interior patches and four patch positions along one axis
    struct
    {
      int P, px, py, pz;
    } shapes[] = {{4, 2, 2, 4}, {1, 2, 2, 4}, {2, 2, 2, 5}, {5, 4, 4, 1}, {3, 6, 2, 2}, {8, 2, 4, 3}, {7, 2, 2, 6}};
    int i = 0;
    for (auto sh : shapes)
    {
      for (int b = 0; b < 2; ++b)
      {
        Geo g = patches_geo(sh.P, sh.px, sh.py, sh.pz, b ? SLAB : ALL_L, b != 0);
        Case c = mk(nm("split %dx%dx%d patches P%d%s", sh.px, sh.py, sh.pz, sh.P, b ? " shuffled, two lists" : ""), g,
                    box_space(g, sh.P, (Bc)((i + b) % 3), b ? 300 + i : 0), THR_COLOURED, 2);
        c.expect_split = !b; // (the slab takes a layer of patches away: whatever the builder decides is checked)
        v.push_back(c);
      }
      ++i;
    }
    {
      Geo g = patches_geo(4, 2, 2, 4, ALL_L);
      v.push_back(mk("split asked of a merged level P4", g, box_space(g, 4, BC_SURFACE), THR_MERGED, 2));
      Case c = mk("split asked with too few patches P4", patches_geo(4, 2, 2, 3, ALL_L), Space(), THR_COLOURED, 2);
      c.s = box_space(c.g, 4, BC_SURFACE);
      c.expect_split_refused = true;
      v.push_back(c);
      Case d = mk("split asked with three positions per axis P6", patches_geo(6, 3, 3, 3, ALL_L), Space(), THR_COLOURED,
                  2);
      d.s = box_space(d.g, 6, BC_NONE);
      d.expect_split_refused = true;
      v.push_back(d);
    }
    {
      // irregular: Morton patches have no layer structure; the builder splits only if the colours separate
      Geo g = box_geo(6, 6, 30, ALL_L, false, 0.3, false, 20, 61);
      v.push_back(mk("split asked of Morton patches P4", g, box_space(g, 4, BC_RANDOM, 9), THR_COLOURED, 2));
      Geo h = box_geo(5, 5, 29, ALL_L, true, 0.0, false, 15, 62);
      v.push_back(mk("split asked of a grid with holes P3", h, box_space(h, 3, BC_SURFACE), THR_COLOURED, 2));
      Geo r = box_geo(5, 3, 41, ALL_L, false, 0.0, false, 0, 63);
      Case rc = mk("split of ragged blocks P4: refused by the colours", r, box_space(r, 4, BC_SURFACE), THR_COLOURED, 2);
      rc.expect_split_refused_colours = true;
      v.push_back(rc);
    }
  }
  else if (group == "chains")
  {
    auto chain_case = [&](std::string name, Geo g, int P, Bc b, long long thr, int streams, ChainExpect e, int minc,
                          uint32_t perm = 0) {
      Case c = mk(std::move(name), g, box_space(g, P, b, perm), thr, streams);
      c.chain = e;
      c.min_chains = minc;
      v.push_back(c);
    };
    for (int P : {4, 3, 1, 6})
      for (int b = 0; b < 3; ++b)
        chain_case(nm("chains 2x2x%d patches P%d bc %d", 2 + b, P, b), patches_geo(P, 2, 2, 2 + b, ALL_L, b == 1), P,
                   (Bc)b, THR_COLOURED, 0, CH_OK, 1, b == 2 ? 50 + P : 0);
    chain_case("chains 3x2x4 patches P4, two lists", patches_geo(4, 3, 2, 4, SLAB), 4, BC_SURFACE, THR_COLOURED, 0,
               CH_OK, 1);
    chain_case("chains 4x3x2 patches P4 random markers", patches_geo(4, 4, 3, 2, ALL_L), 4, BC_RANDOM, THR_COLOURED, 0,
               CH_OK, 2, 77);
    chain_case("chains refused: production min_chains", patches_geo(4, 2, 2, 3, ALL_L), 4, BC_SURFACE, THR_COLOURED, 0,
               CH_REFUSE_FEW, PRODUCTION_MIN_CHAINS);
    chain_case("chains refused: merged level", patches_geo(4, 2, 2, 2, ALL_L), 4, BC_SURFACE, THR_MERGED, 0,
               CH_REFUSE_MERGED, 1);
    chain_case("chains refused: default threshold merges", patches_geo(4, 2, 2, 2, ALL_L), 4, BC_SURFACE, THR_DEFAULT, 0,
               CH_REFUSE_MERGED, PRODUCTION_MIN_CHAINS);
    chain_case("chains refused: split plan", patches_geo(4, 2, 2, 4, ALL_L), 4, BC_SURFACE, THR_COLOURED, 2,
               CH_REFUSE_SPLIT, 1);
    chain_case("chains refused: holes, no patch grid", box_geo(4, 4, 24, ALL_L, false, 0.0, false, 30, 81), 4,
               BC_SURFACE, THR_COLOURED, 0, CH_REFUSE_GRID, 1);
    chain_case("chains refused: Morton patches", box_geo(4, 4, 24, ALL_L, false, 0.3, false, 0, 82), 4, BC_NONE,
               THR_COLOURED, 0, CH_REFUSE_GRID, 1);
    chain_case("chains refused: as many chain colours", patches_geo(4, 2, 2, 1, ALL_L), 4, BC_SURFACE, THR_COLOURED, 0,
               CH_REFUSE_COLOURS, 1);
  }
  else if (group == "chains_production")
  {
    // the production min_chains on the smallest level it accepts: 28 x 28 chains, four colours of 196
    Geo g = patches_geo(3, 28, 28, 2, ALL_L);
    Case c = mk("chains 28x28x2 patches P3, production min_chains", g, box_space(g, 3, BC_SURFACE), THR_COLOURED, 0);
    c.chain = CH_OK;
    c.min_chains = PRODUCTION_MIN_CHAINS;
    v.push_back(c);
  }
  else if (group == "transfers")
  {
    // every pair of degrees on a small mesh, all three thresholds in turn
    int i = 0;
    for (int pf = 2; pf <= 8; ++pf)
    {
      const PatchShape sh = patch_shape(pf);
      Geo g = box_geo(std::min(2 * sh.bx, 4), std::min(2 * sh.by, 4), std::min(2 * sh.bz, 9), i % 2 ? SLAB : ALL_L,
                      i % 2 != 0, 0.0, false, 0, 90 + i);
      Case c = mk(nm("transfers 1..%d -> %d %s", pf - 1, pf, THRN[i % 3]), g, box_space(g, pf, BC_SURFACE, i % 2 ? 400 + i : 0),
                  THR[i % 3]);
      for (int pc = 1; pc < pf; ++pc)
        c.coarse_degrees.push_back(pc);
      c.coarse_perm = i % 2 ? 0 : 500 + i;
      v.push_back(c);
      ++i;
    }
    {
      Geo g = patches_geo(4, 2, 2, 2, ALL_L);
      Case c = mk("transfers 1, 2 -> 4 coloured", g, box_space(g, 4, BC_SURFACE), THR_COLOURED);
      c.coarse_degrees = {1, 2};
      v.push_back(c);
      Geo h = patches_geo(2, 2, 2, 2, SLAB);
      Case d = mk("transfers 1 -> 2 coloured, two lists", h, box_space(h, 2, BC_NONE, 33), THR_COLOURED);
      d.coarse_degrees = {1};
      d.coarse_perm = 34;
      v.push_back(d);
      Geo m = box_geo(4, 4, 12, SLAB, true, 0.3, false, 30, 95);
      Case e = mk("transfers 1, 3 -> 6 Morton patches", m, box_space(m, 6, BC_RANDOM, 35), THR_COLOURED);
      e.coarse_degrees = {1, 3};
      v.push_back(e);
      Case s2 = mk("transfers 2 -> 4 split plan", patches_geo(4, 2, 2, 4, ALL_L), Space(), THR_COLOURED, 2);
      s2.s = box_space(s2.g, 4, BC_SURFACE);
      s2.coarse_degrees = {2};
      v.push_back(s2);
      for (const auto& dm : {std::array<int, 3>{1, 1, 2}, std::array<int, 3>{2, 2, 2}})
      {
        Case b;
        b.name = nm("transfers 2 -> 4 brick %dx%dx%d", dm[0], dm[1], dm[2]);
        brick(6, dm, 0, 4, b.g, b.s);
        b.threshold = dm[0] == 1 ? THR_COLOURED : THR_DEFAULT;
        // (the coarse space on the brick's own cell grid: a numbering of its own, conforming all the same)
        b.coarse_degrees = {2};
        v.push_back(b);
      }
    }
  }
  else if (group == "multiblock")
  {
    // Meshes that are no boxes: stars of 3 and 5 sectors (an edge shared by 3 / 5 cells, vertices of valence 6 / 10, a
    // Jacobian per sector; bent: every centroid with an x of its own), the O-grid (edges of 3 cells, vertices of 4 and
    // 6, left-handed blocks; twisted) and the notched grid (re-entrant edges, a cavity, columns of cells that stop and
    // resume).  Sizes per degree: a handful of patches at least.  Nothing is expected of the split and the chains but
    // that the builder's decision is consistent and the resulting schedule exact.
    struct Size
    {
      int P, star_m, star_nz, ogrid_m, nx, ny, nz;
      std::vector<int> coarse;
    };
    const Size sizes[] = {{1, 4, 16, 6, 8, 8, 32, {}},    {2, 4, 16, 6, 8, 8, 32, {1}}, {4, 4, 8, 4, 4, 4, 32, {1, 2}},
                          {5, 2, 7, 2, 3, 3, 14, {2}}, {8, 2, 3, 2, 3, 3, 6, {4}}};
    int i = 0;
    for (const Size& z : sizes)
      for (int mesh = 0; mesh < 4; ++mesh)
        for (int form = 0; form < 2; ++form)
        {
          // form 0: one cell list, coloured, the exterior marked; form 1: two lists (a partition between blocks / a
          // slab), cells shuffled, dofs permuted, random markers, merged or the default threshold
          const Lists lists = form ? SLAB : ALL_L;
          const bool bent = form == 0;
          Geo g;
          const char* name = "";
          switch (mesh)
          {
          case 0: g = block_geo(star_blocks(3, z.star_m, z.star_nz), bent ? MAP_BEND : MAP_NONE, lists, form, 70 + i); name = "star3"; break;
          case 1: g = block_geo(star_blocks(5, z.star_m, z.star_nz), bent ? MAP_BEND : MAP_NONE, lists, form, 70 + i); name = "star5"; break;
          case 2: g = block_geo(ogrid_blocks(z.ogrid_m), bent ? MAP_TWIST : MAP_NONE, lists, form, 70 + i); name = "ogrid"; break;
          default: g = notched_geo(z.nx, z.ny, z.nz, lists, form, 70 + i); name = "notched"; break;
          }
          const long long thr = form == 0 ? THR_COLOURED : (i % 2 ? THR_MERGED : THR_DEFAULT);
          Case c = mk(nm("%s%s P%d %s%s", name, bent && mesh < 3 ? (mesh == 2 ? " twisted" : " bent") : "", z.P,
                         form ? (i % 2 ? "merged" : "default") : "coloured", form ? ", two lists, shuffled" : ""),
                      g, Space(), thr);
          c.s = space_of(c.g, z.P, form ? BC_RANDOM : BC_SURFACE, form ? 600 + i : 0);
          c.chain = CH_ANY;
          c.coarse_degrees = z.coarse;
          c.coarse_perm = form ? 700 + i : 0;
          c.observe = true;
          v.push_back(c);
          ++i;
        }
    // the two-stream split and the chains, asked of levels that are large enough to get them
    for (int P : {1, 4})
      for (int mesh = 0; mesh < 4; ++mesh)
      {
        Geo g;
        const char* name = "";
        switch (mesh)
        {
        case 0: g = block_geo(star_blocks(5, 4, P == 1 ? 64 : 8), MAP_NONE, ALL_L); name = "star5"; break;
        case 1: g = block_geo(star_blocks(3, 4, P == 1 ? 96 : 12), MAP_BEND, ALL_L); name = "star3 bent"; break;
        case 2: g = block_geo(ogrid_blocks(P == 1 ? 9 : 4), MAP_TWIST, ALL_L); name = "ogrid twisted"; break;
        default: g = P == 1 ? notched_geo(8, 8, 96, ALL_L) : notched_geo(4, 4, 48, ALL_L); name = "notched"; break;
        }
        for (int streams : {2, 0})
        {
          Case c = mk(nm("%s P%d, %s", name, P, streams ? "split asked" : "chains asked"), g, Space(), THR_COLOURED, streams);
          c.s = space_of(c.g, P, BC_SURFACE);
          c.chain = CH_ANY;
          c.observe = true;
          v.push_back(c);
        }
      }
  }
  return v;
}

// a discontinuous fine space under a continuous coarse one: the coloured restriction would race; it must be refused
void run_nonconforming()
{
  Geo g = patches_geo(2, 2, 2, 2, ALL_L);
  const Space fine = discontinuous_space(g, 2), coarse = box_space(g, 1, BC_NONE);
  configure(THR_COLOURED, 0);
  PatchPlan pl;
  CHECK(build(pl, g, fine) == PMG_OK, "build_patch_plan", "it failed: %s", g_last_error.c_str());
  check_plan(g, fine, pl);
  interpret_plan(pl, reference_apply(g, fine));
  CHECK(pl.n_plain >= 1, "case", "the non-conforming case needs a plain launch");
  CoarsePlan cp;
  const int rc = build_coarse(cp, g, coarse, pl);
  CHECK(rc == PMG_ERR_INVALID, "build_coarse_plan refuses non-conforming spaces", "it returned %d", rc);
  // the merged form adds with atomics into a zero-filled vector: nothing to refuse there
  configure(THR_MERGED, 0);
  Geo g2 = patches_geo(2, 2, 2, 2, SLAB);
  const Space fine2 = discontinuous_space(g2, 2);
  CHECK(build(pl, g2, fine2) == PMG_OK, "build_patch_plan", "it failed: %s", g_last_error.c_str());
  std::printf("     (n_plain = %d, %zu launches)\n", pl.n_plain, pl.launch_first.size());
  if (pl.n_plain == 0)
  {
    CHECK(build_coarse(cp, g2, coarse, pl) == PMG_OK, "build_coarse_plan", "merged form refused: %s",
          g_last_error.c_str());
    check_coarse(g2, box_space(g2, 1, BC_NONE), pl, cp);
  }
  cover("coarse_refused");
  std::printf("ok   %-44s\n", "non-conforming spaces are refused");
}

int run_group(const std::string& group)
{
  int n = 0;
  std::string current;
  try
  {
    for (const Case& c : cases_of(group))
    {
      current = c.name;
      run_case(c);
      ++n;
    }
    if (group == "transfers")
    {
      current = "non-conforming spaces are refused";
      run_nonconforming();
      ++n;
    }
  }
  catch (const Violation& v)
  {
    std::printf("FAIL %s\n  invariant: %s\n  %s\n", current.c_str(), v.invariant.c_str(), v.what.c_str());
    return 1;
  }
  if (n == 0)
  {
    std::printf("no such group: %s\n", group.c_str());
    return 2;
  }
  std::printf("SUMMARY group=%s cases=%d violations=0 coverage=", group.c_str(), n);
  bool sep = false;
  for (const std::string& f : g_cov)
  {
    std::printf("%s%s", sep ? "," : "", f.c_str());
    sep = true;
  }
  std::printf("\n");
  return 0;
}

// ---- mutations ---------------------------------------------------------------------------------------------------------
struct Fixture
{
  Geo g;
  Space s, coarse;
  PatchPlan pl;
  ChainPlan ch;
  CoarsePlan co;
  Reference ref;
};

void check_everything(const Fixture& f, bool structure = true)
{
  if (structure)
  {
    check_plan(f.g, f.s, f.pl);
    check_premerge(f.g, f.s, f.pl);
  }
  interpret_plan(f.pl, f.ref);
  if (f.ch.ok)
  {
    if (structure)
      check_chain(f.s, f.pl, f.ch);
    interpret_chain(f.pl, f.ch, f.ref);
  }
  if (structure && !f.co.cpoff.empty())
    check_coarse(f.g, f.coarse, f.pl, f.co);
}

int run_mutations()
{
  // two valid plans: a coloured level with chains, a boundary launch and transfers; and a split plan
  Fixture a, b;
  a.g = patches_geo(4, 2, 2, 3, SLAB);
  a.s = box_space(a.g, 4, BC_SURFACE);
  a.coarse = box_space(a.g, 2, BC_NONE);
  configure(THR_COLOURED, 0);
  int rc = build(a.pl, a.g, a.s);
  rc |= build_chain_plan(a.ch, a.pl, a.s.ndofs, a.s.bc.data(), a.g.cen.data(), 1);
  rc |= build_coarse(a.co, a.g, a.coarse, a.pl);
  a.ref = reference_apply(a.g, a.s);
  b.g = patches_geo(4, 2, 2, 4, SLAB);
  b.s = box_space(b.g, 4, BC_SURFACE);
  configure(THR_COLOURED, 2);
  rc |= build(b.pl, b.g, b.s);
  b.ref = reference_apply(b.g, b.s);
  try
  {
    if (rc != PMG_OK || !a.ch.ok || b.pl.launch_stream.empty() || a.pl.bzero.empty())
      violate("mutation fixtures", "rc = %d, chain ok = %d, split = %d, bzero = %zu", rc, a.ch.ok,
              !b.pl.launch_stream.empty(), a.pl.bzero.size());
    check_everything(a);
    check_everything(b);
  }
  catch (const Violation& v)
  {
    std::printf("FAIL the unmutated plans\n  invariant: %s\n  %s\n", v.invariant.c_str(), v.what.c_str());
    return 1;
  }
  std::printf("ok   the unmutated plans pass\n");

  // entries to corrupt
  auto find_entry = [](const std::vector<uint32_t>& v, size_t lo, size_t hi, std::function<bool(size_t)> pred) {
    for (size_t i = lo; i < hi; ++i)
      if (pred(i))
        return (long long)i;
    return -1LL;
  };
  const size_t n_int = a.pl.poff[a.pl.launch_first[a.pl.n_launch_l]]; // entries of the interior patches
  struct Mutation
  {
    const char* name;
    std::function<bool(Fixture&)> apply; // false: nothing to corrupt was found (counts as a failure)
    bool on_split;
  };
  std::vector<Mutation> muts = {
      {"set PD_ACC on a first toucher",
       [&](Fixture& f) {
         long long i = find_entry(f.pl.pdofs, 0, n_int, [&](size_t k) { return !(f.pl.pdofs[k] & (PD_ACC | PD_BC)); });
         return i >= 0 && (f.pl.pdofs[i] |= PD_ACC, true);
       },
       false},
      {"clear PD_ACC on a later toucher",
       [&](Fixture& f) {
         long long i = find_entry(f.pl.pdofs, 0, n_int, [&](size_t k) { return (f.pl.pdofs[k] & (PD_ACC | PD_BC)) == PD_ACC; });
         return i >= 0 && (f.pl.pdofs[i] &= ~PD_ACC, true);
       },
       false},
      {"move a patch into the launch of a neighbour",
       [&](Fixture& f) {
         // the last patch of launch 0 becomes the first patch of launch 1, whose patches it touches
         if (f.pl.n_plain < 2 || f.pl.launch_count[0] < 1)
           return false;
         f.pl.launch_count[0]--;
         f.pl.launch_first[1]--;
         f.pl.launch_count[1]++;
         return true;
       },
       false},
      {"drop one bzero entry",
       [&](Fixture& f) {
         f.pl.bzero.erase(f.pl.bzero.begin() + f.pl.bzero.size() / 2);
         return true;
       },
       false},
      {"shift launch_wait by +2",
       [&](Fixture& f) {
         f.pl.launch_wait += 2;
         return true;
       },
       true},
      {"shift launch_signal by -2",
       [&](Fixture& f) {
         f.pl.launch_signal -= 2;
         return true;
       },
       true},
      {"clear one CD_SKIP",
       [&](Fixture& f) {
         long long i = find_entry(f.ch.cdofs, 0, n_int, [&](size_t k) { return (f.ch.cdofs[k] & CD_SKIP) != 0; });
         return i >= 0 && (f.ch.cdofs[i] &= ~CD_SKIP, true);
       },
       false},
      {"change one ccar position",
       [&](Fixture& f) {
         long long i = find_entry(f.ch.ccar, 0, n_int, [&](size_t k) { return (f.ch.ccar[k] & 0xffffu) != CC_NONE; });
         return i >= 0 && (f.ch.ccar[i] = (f.ch.ccar[i] & ~0xffffu) | (((f.ch.ccar[i] & 0xffffu) + 1u) & 0x7fffu), true);
       },
       false},
      {"set a second CD_BCFIRST",
       [&](Fixture& f) {
         long long i = find_entry(f.ch.cdofs, 0, n_int,
                                  [&](size_t k) { return (f.ch.cdofs[k] & (CD_BC | CD_BCFIRST)) == CD_BC; });
         return i >= 0 && (f.ch.cdofs[i] |= CD_BCFIRST, true);
       },
       false},
      {"swap two entries of one lmaps row",
       [&](Fixture& f) {
         uint16_t* lm = f.pl.lmaps.data() + (size_t)f.pl.lmap_id[0] * f.pl.K * f.pl.N;
         if (lm[0] == lm[1])
           return false;
         std::swap(lm[0], lm[1]);
         return true;
       },
       false},
      {"set PD_ACC on a coarse first toucher",
       [&](Fixture& f) {
         long long i = find_entry(f.co.cpdofs, 0, f.co.cpdofs.size(), [&](size_t k) { return !(f.co.cpdofs[k] & PD_ACC); });
         return i >= 0 && (f.co.cpdofs[i] |= PD_ACC, true);
       },
       false},
      {"clear PD_ACC on a coarse later toucher",
       [&](Fixture& f) {
         long long i = find_entry(f.co.cpdofs, 0, f.co.cpdofs.size(), [&](size_t k) { return (f.co.cpdofs[k] & PD_ACC) != 0; });
         return i >= 0 && (f.co.cpdofs[i] &= ~PD_ACC, true);
       },
       false},
  };
  int missed = 0;
  for (const Mutation& m : muts)
  {
    Fixture f = m.on_split ? b : a;
    bool detected = false;
    std::string how;
    if (!m.apply(f))
      how = "nothing to corrupt was found";
    else
      try
      {
        check_everything(f);
        how = "every check passed";
      }
      catch (const Violation& v)
      {
        detected = true;
        how = v.invariant + ": " + v.what;
      }
    std::printf("%s %-44s %s\n", detected ? "ok  " : "FAIL", m.name, how.c_str());
    missed += !detected;
    // for information: does the serial interpretation alone see it?  (a second y = x of a Dirichlet row, or a local
    // map whose two swapped positions receive the same sums, changes no result)
    if (detected)
    {
      bool seen = false;
      try
      {
        check_everything(f, false);
      }
      catch (const Violation&)
      {
        seen = true;
      }
      std::printf("       (the serial interpretation alone: %s)\n", seen ? "reports it" : "does not see it");
    }
  }
  std::printf("SUMMARY mutations=%zu undetected=%d\n", muts.size(), missed);
  return missed ? 1 : 0;
}
} // namespace

int main(int argc, char** argv)
{
  if (argc != 2)
  {
    std::printf("usage: plan_check <group> | --list | --mutate\n");
    return 2;
  }
  const std::string arg = argv[1];
  if (arg == "--list")
  {
    for (const char* gname : GROUPS)
      std::printf("%s\n", gname);
    std::printf("FLAGS");
    for (const char* f : FLAGS)
      std::printf(" %s", f);
    std::printf("\n");
    return 0;
  }
  if (arg == "--mutate")
    return run_mutations();
  return run_group(arg);
}
