// Stand-alone host checker of the Chebyshev smooth's schedule (csrc/smooth_plan.hpp).  The library's smoother loop is an
// interpreter of the steps for_each_smooth_step yields; the contracts between those steps -- which buffer an
// application writes, which pass clears w.q for the next zeroed-output application, which pass no longer writes r and
// z, what is left to the consumer, when the ghosts of x are current -- are seen on the device only by parity tests,
// and only when they happen to lose.  This program needs no GPU: it takes the steps from the same visitor, gives each
// its generic meaning on std::vector<T> (the per-entry arithmetic of every pass restated from the functor comments in
// csrc/vector.hip) and executes every call of the full product of SmoothCall's fields on a small dense operator with
// ghosts, against the plain loop of src/chebyshev.hpp:46-91.  Compiled host-only with the address and
// undefined-behaviour sanitizers and -ffp-contract=off (tests/test_smooth_plans.py); never loaded into Python.
//
//   smooth_check fp64|fp32   run the cases of one scalar type; one line per failing case, then a summary line
//   smooth_check --list      the group names and the coverage flags
//   smooth_check --mutate    corrupt valid schedules one step at a time; every corruption must be reported
//
// Exit status 0 = every case passed (in --mutate: every corruption was detected).
//
// What the smoother guarantees about w.q for a zeroed-output operator, which the checks below assert: a smooth does
// NOT rely on w.q being zero on entry.  Its first application is the plain (or ghosts-current) variant, which fills for itself,
// or, from x = 0, follows the init pass, which clears w.q; so w.q enters every case as NaN.  On return w.q is zero only
// where the last step that touches it is a clearing pass: in every ResidualNone call.  Behind a call that returns a
// residual it holds the last product.
#include "smooth_plan.hpp"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <set>
#include <string>
#include <vector>

namespace pmg
{
// (the library's own lives in tables.hip, next to code that needs a GPU)
std::string g_last_error;
int fail(int code, const char* fmt, ...)
{
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
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

const char* const GROUPS[] = {"fp64", "fp32"};
const char* const FLAGS[] = {"k0", "one_step_none", "one_step_residual", "x_zero", "need_none", "need_updated",
                             "need_split", "need_fused", "left_none", "left_split", "left_fused", "recomputed_k2",
                             "recomputed_k3", "zeroed_output", "ghosts", "ghosts_current", "float", "refused_zeroed",
                             "refused_recompute", "design_pass_counts"};
std::set<std::string> g_cov;
void cover(const char* f) { g_cov.insert(f); }

// ---- the operator ---------------------------------------------------------------------------------------------------
// N owned entries and NG ghosts behind them, each a copy of an owned entry.  The operator reads all NT entries of its
// input: a row of M has a column per ghost, so a stale ghost is a wrong product.  With current ghosts it is the
// symmetric, strictly diagonally dominant S = M folded onto the owners.
constexpr int N = 7, NG = 3, NT = N + NG;
const int OWNER[NG] = {2, 5, 0};

template <typename T>
struct Problem
{
  T M[N][NT];
  T dinv[N], b[N], x0[N];
  double lmax = 0;
  Problem()
  {
    double S[N][N];
    for (int i = 0; i < N; ++i)
      for (int j = 0; j < N; ++j)
      {
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        S[i][j] = i == j ? 4.0 + 0.3 * i : -1.0 / (1.5 + (hi - lo)) - 0.05 * std::sin(7.0 * lo + 3.0 * hi);
      }
    for (int i = 0; i < N; ++i)
    {
      double row = 0;
      for (int j = 0; j < N; ++j)
      {
        M[i][j] = (T)S[i][j];
        row += std::fabs(S[i][j]) / S[i][i];
      }
      lmax = row > lmax ? row : lmax; // Gershgorin bound of D^-1 S
      for (int g = 0; g < NG; ++g)     // a share of the owner's column goes through the ghost
      {
        const double share = (0.25 + 0.125 * g) * S[i][OWNER[g]];
        M[i][N + g] = (T)share;
        M[i][OWNER[g]] = (T)(S[i][OWNER[g]] - share);
      }
      dinv[i] = (T)(1.0 / S[i][i]);
      b[i] = (T)(std::cos(1.0 + 2.0 * i) + 0.1 * i);
      x0[i] = (T)(0.5 * std::sin(3.0 + i) - 0.2);
    }
  }
};

template <typename T>
using Vec = std::vector<T>;

// out = A in.  Every variant but GHOSTS_CURRENT refreshes the ghosts of its input first; ZEROED_OUTPUT adds into an
// output that must be zero over [0, NT), the others assign the owned entries and leave the ghost entries alone.
template <typename T>
void apply(const Problem<T>& p, SmoothStep::Variant v, Vec<T>& in, Vec<T>& out)
{
  if (v != SmoothStep::GHOSTS_CURRENT)
    for (int g = 0; g < NG; ++g)
      in[N + g] = in[OWNER[g]];
  if (v == SmoothStep::ZEROED_OUTPUT)
    for (int i = 0; i < NT; ++i)
      CHECK(out[i] == T(0), "zeroed_output_is_zero", "entry %d of the output of a zeroed-output application holds %g", i,
            (double)out[i]);
  for (int i = 0; i < N; ++i)
  {
    T acc = T(0);
    for (int j = 0; j < NT; ++j)
      acc += p.M[i][j] * in[j];
    out[i] = v == SmoothStep::ZEROED_OUTPUT ? out[i] + acc : acc;
  }
}

// ---- the two correction helpers of vector.hip, their roundings spelled out ------------------------------------------
template <typename T>
T first_correction(T c0, T d, T r)
{
  const T cd = c0 * d; // two rounded products
  return cd * r;
}
template <typename T>
T correction(T c1, T z, T c2, T d, T r)
{
  const T cd = c2 * d; // two rounded products ...
  const T t = cd * r;
  return std::fma(c1, z, t); // ... and one fused multiply-add
}

// ---- the reference: the loop of src/chebyshev.hpp:46-91 -------------------------------------------------------------
template <typename T>
struct Reference
{
  Vec<T> x, r;
};
template <typename T>
Reference<T> reference(const Problem<T>& p, int k, bool x_zero)
{
  Vec<T> x(NT, T(0)), r(NT, T(0)), z(NT, T(0)), q(NT, T(0));
  if (!x_zero)
    for (int i = 0; i < N; ++i)
      x[i] = p.x0[i];
  apply(p, SmoothStep::PLAIN, x, q); // r = b - A x
  for (int i = 0; i < N; ++i)
    r[i] = p.b[i] - q[i];
  for (int i = 0; i < N; ++i) // z = c0 dinv r
    z[i] = first_correction((T)cheb_c0(p.lmax), p.dinv[i], r[i]);
  for (int s = 1; s <= k; ++s)
  {
    for (int i = 0; i < N; ++i) // x += z
      x[i] += z[i];
    apply(p, SmoothStep::PLAIN, z, q); // r -= A z
    for (int i = 0; i < N; ++i)
      r[i] -= q[i];
    for (int i = 0; i < N; ++i) // z = c1 z + c2 dinv r
      z[i] = correction((T)cheb_c1(s), z[i], (T)cheb_c2(s, p.lmax), p.dinv[i], r[i]);
  }
  return {x, r};
}

// ---- the steps, executed ------------------------------------------------------------------------------------------
template <typename T>
struct State
{
  Vec<T> x, r, z, q, q1, q2;
  int applications = 0, launches = 0;
  int passes = 0; // vector reads + writes over the owned entries, without the clearing of w.q
  bool recomputed = false;
  Vec<T>& product(SmoothStep::Buffer b) { return b == SmoothStep::Q ? q : b == SmoothStep::Q1 ? q1 : q2; }
};

template <typename T>
void execute(const Problem<T>& p, const SmoothStep& st, State<T>& s)
{
  const T c0 = (T)cheb_c0(p.lmax);
  if (st.kind == SmoothStep::APPLY)
  {
    s.applications++;
    apply(p, st.variant, st.in_x ? s.x : s.z, s.product(st.out));
    return;
  }
  s.launches++;
  const T c1 = (T)cheb_c1(st.i), c2 = (T)cheb_c2(st.i, p.lmax);
  switch (st.kind)
  {
  case SmoothStep::APPLY: break;
  case SmoothStep::INIT: // r = b - q ; z = c0 dinv r; without q: r = b
    for (int i = 0; i < N; ++i)
    {
      const T vr = p.b[i] - (st.with_q ? s.q[i] : T(0));
      s.r[i] = vr;
      s.z[i] = first_correction(c0, p.dinv[i], vr);
    }
    s.passes += 4 + (st.with_q ? 1 : 0);
    break;
  case SmoothStep::FIRST: // first step from x == 0: r -= q ; z_2 = c1 z_1 + c2 dinv r ; x = z_1 + z_2
  case SmoothStep::STEP:  // r -= q ; z_new = c1 z + c2 dinv r ; x += (z if both) + z_new
    for (int i = 0; i < N; ++i)
    {
      T vz = s.z[i], vx = st.kind == SmoothStep::FIRST ? vz : s.x[i];
      if (st.kind == SmoothStep::STEP && st.both)
        vx += vz;
      const T vr = s.r[i] - s.q[i];
      vz = correction(c1, vz, c2, p.dinv[i], vr);
      if (st.x_final != 2) // 2: nobody reads r and z after this step: they are not written
      {
        s.r[i] = vr;
        s.z[i] = vz;
      }
      s.x[i] = vx + vz;
    }
    s.passes += (st.kind == SmoothStep::FIRST ? 4 : 5) + 1 + (st.x_final != 2 ? 2 : 0);
    break;
  case SmoothStep::LAST: // x (+)= z ; r -= q
    for (int i = 0; i < N; ++i)
    {
      s.x[i] = (st.assign ? T(0) : s.x[i]) + s.z[i];
      s.r[i] -= s.q[i];
    }
    s.passes += (st.assign ? 3 : 4) + 2;
    break;
  case SmoothStep::RESIDUAL: // r -= q
    for (int i = 0; i < N; ++i)
      s.r[i] -= s.q[i];
    s.passes += 3;
    break;
  case SmoothStep::ADD: // x += z
    for (int i = 0; i < N; ++i)
      s.x[i] += s.z[i];
    s.passes += 3;
    break;
  case SmoothStep::GHOST_ADD:
    for (int i = N; i < NT; ++i)
      s.x[i] += s.z[i];
    break;
  case SmoothStep::COPY:
    for (int i = 0; i < N; ++i)
      s.x[i] = s.z[i];
    s.passes += 2;
    break;
  case SmoothStep::ZERO_X:
    for (int i = 0; i < N; ++i)
      s.x[i] = T(0);
    s.passes += 1;
    break;
  case SmoothStep::ZERO_GHOSTS:
    for (int i = N; i < NT; ++i)
      s.x[i] = T(0);
    break;
  case SmoothStep::RECOMPUTE:
    // STAGE 1: z = z_1 = c0 dinv (b - q0)
    // STAGE 2: r_1 = (b - q0) - q1; z = z_2 = c1a z_1 + c2a dinv r_1
    // STAGE 3: r_2 = r_1 - q2; z_3 = c1b z_2 + c2b dinv r_2; x = ((x + z_1) + z_2) + z_3 (two steps: without the
    //          q2 part); with r_out the last residual and correction are written.  Without q0: r_0 = b, x is assigned.
    s.recomputed = true;
    for (int i = 0; i < N; ++i)
    {
      const T d = p.dinv[i];
      T vx = (st.stage == 3 && st.with_q) ? s.x[i] : T(0);
      T vr = st.with_q ? p.b[i] - s.q[i] : p.b[i];
      T vz = first_correction(c0, d, vr);
      if (st.stage >= 2)
      {
        if (st.stage == 3)
          vx = st.with_q ? vx + vz : vz;
        vr -= s.q1[i];
        vz = correction((T)cheb_c1(1), vz, (T)cheb_c2(1, p.lmax), d, vr);
        if (st.stage == 3)
        {
          vx += vz;
          if (st.with_q2)
          {
            vr -= s.q2[i];
            vz = correction((T)cheb_c1(2), vz, (T)cheb_c2(2, p.lmax), d, vr);
            vx += vz;
          }
        }
      }
      if (st.stage == 3)
      {
        s.x[i] = vx;
        if (st.r_out)
        {
          s.r[i] = vr;
          s.z[i] = vz;
        }
      }
      else
        s.z[i] = vz;
    }
    s.passes += 2 + (st.with_q ? 1 : 0) + (st.stage >= 2 ? 1 : 0) + (st.with_q2 ? 1 : 0); // b dinv q0 q1 q2
    s.passes += st.stage == 3 ? (st.with_q ? 2 : 1) + (st.r_out ? 2 : 0) : 1;             // x in and out, r z | z
    break;
  }
  if (st.clear_q) // ThenClearF: w.q = 0 over [0, n_total) behind the pass
    for (int i = 0; i < NT; ++i)
      s.q[i] = T(0);
}

const char* const NEED[] = {"none", "updated", "split", "fused"};
std::string name_of(const SmoothCall& c)
{
  char buf[160];
  snprintf(buf, sizeof buf, "%s k=%d need_r=%s x_zero=%d zeroed=%d ghosts=%d current=%d recompute=%d",
           c.fp64 ? "fp64" : "fp32", c.k, NEED[c.need_r], c.x_zero, c.zeroed_output, c.ghosts, c.ghosts_current,
           c.allow_recompute);
  return buf;
}

template <typename T>
bool all_finite(const Vec<T>& v, int n)
{
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i]))
      return false;
  return true;
}

// Execute `steps` for the call and check everything the call promises.  `counts`: compare against smooth_outcome as
// well (off for mutated step lists, which are to be caught by what they compute).
template <typename T>
void run_steps(const SmoothCall& c, const std::vector<SmoothStep>& steps, SmoothOutcome::Left left, bool counts)
{
  const Problem<T> p;
  const T nan = std::numeric_limits<T>::quiet_NaN();
  // r, z, q, q1, q2 carry a previous call's contents in the library, and so does an x that counts as zero
  State<T> s;
  s.x.assign(NT, nan);
  s.r = s.z = s.q = s.q1 = s.q2 = s.x;
  if (!c.x_zero)
    for (int i = 0; i < N; ++i)
      s.x[i] = p.x0[i];
  if (c.ghosts_current)
    for (int g = 0; g < NG; ++g)
      s.x[N + g] = s.x[OWNER[g]];
  for (const SmoothStep& st : steps)
    execute(p, st, s);

  const Reference<T> ref = reference(p, c.k, c.x_zero);
  // no stale reads: nothing that was not written by this call reaches x or a promised output
  CHECK(all_finite(s.x, N), "no_stale_read", "x holds a NaN");
  // the iterate: every form performs the reference's roundings in the reference's order
  for (int i = 0; i < N; ++i)
    CHECK(s.x[i] == ref.x[i], "iterate", "x[%d] = %.17g, the reference has %.17g", i, (double)s.x[i], (double)ref.x[i]);
  // the residual, in the form the caller was promised
  if (c.need_r != ResidualNone)
  {
    Vec<T> res = s.r;
    if (left == SmoothOutcome::LeftSplit)
    {
      CHECK(all_finite(s.q, N), "no_stale_read", "the consumer's w.q holds a NaN");
      for (int i = 0; i < N; ++i)
        res[i] = s.r[i] - s.q[i];
    }
    else if (left == SmoothOutcome::LeftFused)
    {
      CHECK(all_finite(s.z, N), "no_stale_read", "the consumer's w.z holds a NaN");
      Vec<T> z = s.z, Az(NT, nan);
      apply(p, SmoothStep::PLAIN, z, Az);
      for (int i = 0; i < N; ++i)
        res[i] = s.r[i] - Az[i];
    }
    CHECK(all_finite(s.r, N), "no_stale_read", "w.r holds a NaN");
    for (int i = 0; i < N; ++i)
      CHECK(res[i] == ref.r[i], "residual", "residual[%d] = %.17g, the reference has %.17g", i, (double)res[i],
            (double)ref.r[i]);
    // tracked ghosts: every correction that has been applied has reached the ghosts of x.  Where the last application
    // is left to the consumer, so is the refresh of z's ghosts that comes with it: the ghosts of x then lack exactly
    // that correction (the fused restriction runs without ghosts, so the library never asks for the two together).
    if (c.ghosts > 0)
      for (int g = 0; g < NG; ++g)
      {
        const T have = left == SmoothOutcome::LeftFused ? s.x[N + g] + s.z[OWNER[g]] : s.x[N + g];
        CHECK(have == s.x[OWNER[g]], "ghosts_current_on_return", "ghost %d of x = %.17g, its owner has %.17g", g,
              (double)have, (double)s.x[OWNER[g]]);
      }
  }
  else if (c.zeroed_output) // w.q is clear behind a call that leaves nothing in it (see the file header)
    for (int i = 0; i < NT; ++i)
      CHECK(s.q[i] == T(0), "q_clear_on_return", "w.q[%d] = %g on return", i, (double)s.q[i]);
  if (!counts)
    return;
  const SmoothOutcome o = smooth_outcome(c);
  CHECK(o.left_to_consumer == left, "outcome", "smooth_outcome and the walk disagree on what is left to the consumer");
  CHECK(o.applications == s.applications && o.vector_launches == s.launches && o.recomputed == s.recomputed, "outcome",
        "smooth_outcome says %d applications, %d launches, recomputed %d; executed %d, %d, %d", o.applications,
        o.vector_launches, o.recomputed, s.applications, s.launches, s.recomputed);
  // Applications: A x unless x counts as zero, one per step, minus the last one where nobody needs it: in a call that
  // returns no residual (k >= 1), and where it is the consumer's (LeftFused).  Both forms.
  const bool last_skipped = (c.need_r == ResidualNone && c.k >= 1) || left == SmoothOutcome::LeftFused;
  CHECK(s.applications == (c.x_zero ? 0 : 1) + c.k - (last_skipped ? 1 : 0), "applications", "%d applications",
        s.applications);
  // what is left, by the rule of the one-step paths
  const SmoothOutcome::Left expect = c.k >= 2 && c.need_r == ResidualSplit   ? SmoothOutcome::LeftSplit
                                     : c.k >= 2 && c.need_r == ResidualFused ? SmoothOutcome::LeftFused
                                                                             : SmoothOutcome::LeftNone;
  CHECK(left == expect, "outcome", "left_to_consumer %d, expected %d", (int)left, (int)expect);
  // the pass counts of DESIGN section 4.2 (k = 3, x != 0): stored 19 / 21, recomputed 16 / 18
  if (c.k == 3 && !c.x_zero && (c.need_r == ResidualNone || left == SmoothOutcome::LeftFused))
  {
    const int want = (s.recomputed ? 16 : 19) + (c.need_r == ResidualNone ? 0 : 2);
    CHECK(s.passes == want, "design_pass_counts", "%d passes over the owned entries, DESIGN 4.2 says %d", s.passes,
          want);
    cover("design_pass_counts");
  }
}

std::vector<SmoothStep> steps_of(const SmoothCall& c, SmoothOutcome::Left* left, int* rc)
{
  std::vector<SmoothStep> steps;
  *rc = for_each_smooth_step(
      c,
      [&steps](const SmoothStep& st)
      {
        steps.push_back(st);
        return PMG_OK;
      },
      left);
  return steps;
}

void run_as(const SmoothCall& c, const std::vector<SmoothStep>& steps, SmoothOutcome::Left left, bool counts)
{
  if (c.fp64)
    run_steps<double>(c, steps, left, counts);
  else
    run_steps<float>(c, steps, left, counts);
}

// the full product of the fields, for one scalar type
template <typename F>
void for_each_call(bool fp64, F&& f)
{
  for (int k = 0; k <= 5; ++k)
    for (int need_r = ResidualNone; need_r <= ResidualFused; ++need_r)
      for (int bits = 0; bits < 32; ++bits)
      {
        SmoothCall c;
        c.k = k, c.need_r = need_r, c.fp64 = fp64;
        c.x_zero = bits & 1, c.zeroed_output = bits & 2, c.ghosts = (bits & 4) ? NG : 0;
        c.ghosts_current = bits & 8, c.allow_recompute = bits & 16;
        f(c);
      }
}

int run_group(const std::string& group)
{
  const bool fp64 = group == "fp64";
  int cases = 0, refused = 0, violations = 0;
  for_each_call(fp64, [&](const SmoothCall& c) {
    SmoothOutcome::Left left;
    int rc;
    const std::vector<SmoothStep> steps = steps_of(c, &left, &rc);
    try
    {
      // the refusals are exactly: float with a zeroed-output operator, float with the recomputed form allowed
      const bool refuse = !c.fp64 && (c.zeroed_output || c.allow_recompute);
      CHECK((rc != PMG_OK) == refuse, "refusals", "the visitor returned %d", rc);
      if (refuse)
      {
        const char* word = c.zeroed_output ? "zeroed-output" : "recomputed";
        CHECK(g_last_error.find(word) != std::string::npos, "refusals", "the message is '%s'", g_last_error.c_str());
        CHECK(steps.empty() && smooth_outcome(c).applications == 0, "refusals", "a refused call has steps");
        cover(c.zeroed_output ? "refused_zeroed" : "refused_recompute");
        refused++;
        return;
      }
      run_as(c, steps, left, true);
      cases++;
      const bool recomputed = !steps.empty() && smooth_outcome(c).recomputed;
      if (c.k == 0)
        cover("k0");
      if (c.k == 1)
        cover(c.need_r == ResidualNone ? "one_step_none" : "one_step_residual");
      if (c.x_zero)
        cover("x_zero");
      cover(c.need_r == ResidualNone      ? "need_none"
            : c.need_r == ResidualUpdated ? "need_updated"
            : c.need_r == ResidualSplit   ? "need_split"
                                          : "need_fused");
      cover(left == SmoothOutcome::LeftNone ? "left_none" : left == SmoothOutcome::LeftSplit ? "left_split" : "left_fused");
      if (recomputed)
        cover(c.k == 2 ? "recomputed_k2" : "recomputed_k3");
      if (c.zeroed_output)
        cover("zeroed_output");
      if (c.ghosts)
        cover("ghosts");
      if (c.ghosts_current)
        cover("ghosts_current");
      if (!c.fp64)
        cover("float");
    }
    catch (const Violation& v)
    {
      violations++;
      std::printf("FAIL %s: [%s] %s\n", name_of(c).c_str(), v.invariant.c_str(), v.what.c_str());
    }
  });
  std::string cov;
  for (const std::string& f : g_cov)
    cov += (cov.empty() ? "" : ",") + f;
  std::printf("SUMMARY group=%s cases=%d refused=%d violations=%d coverage=%s\n", group.c_str(), cases, refused,
              violations, cov.c_str());
  return violations == 0 ? 0 : 1;
}

// ---- mutations ------------------------------------------------------------------------------------------------------
// Every single corruption of a valid schedule that changes what is computed must be reported by the value checks alone
// (the counts are not compared).  Left out, because they change nothing that anyone reads: a swap of a ghost-range pass
// with an owned-range pass (disjoint entries) or of the zeroing of x's ghosts with an application of z (disjoint
// vectors), x_final 2 -> 1 (r and z written though dead), clear_q switched ON.
bool ghost_range(const SmoothStep& st) { return st.kind == SmoothStep::GHOST_ADD || st.kind == SmoothStep::ZERO_GHOSTS; }
bool commute(const SmoothStep& a, const SmoothStep& b)
{
  if (a.kind != SmoothStep::APPLY && b.kind != SmoothStep::APPLY)
    return ghost_range(a) != ghost_range(b);
  return (a.kind == SmoothStep::ZERO_GHOSTS && !b.in_x) || (b.kind == SmoothStep::ZERO_GHOSTS && !a.in_x);
}

int run_mutations()
{
  auto call = [](int k, int need_r, bool x_zero, bool zeroed, int ghosts, bool recompute) {
    SmoothCall c;
    c.k = k, c.need_r = need_r, c.x_zero = x_zero, c.zeroed_output = zeroed, c.ghosts = ghosts;
    c.allow_recompute = recompute;
    return c;
  };
  const SmoothCall bases[] = {call(3, ResidualUpdated, false, true, NG, false), call(3, ResidualFused, false, false, 0, true),
                              call(2, ResidualNone, true, true, 0, false),     call(3, ResidualSplit, true, false, NG, false),
                              call(1, ResidualUpdated, false, false, NG, false), call(2, ResidualNone, false, false, 0, true)};
  int mutations = 0, undetected = 0;
  for (const SmoothCall& c : bases)
  {
    SmoothOutcome::Left left;
    int rc;
    const std::vector<SmoothStep> steps = steps_of(c, &left, &rc);
    run_as(c, steps, left, true); // (the base itself is valid)
    auto attempt = [&](const char* what, size_t at, const std::vector<SmoothStep>& mutated) {
      mutations++;
      try
      {
        run_as(c, mutated, left, false);
        undetected++;
        std::printf("FAIL undetected: %s at step %zu of %s\n", what, at, name_of(c).c_str());
      }
      catch (const Violation& v)
      {
        std::printf("ok   %s at step %zu of %s: [%s]\n", what, at, name_of(c).c_str(), v.invariant.c_str());
      }
    };
    for (size_t j = 0; j < steps.size(); ++j)
    {
      std::vector<SmoothStep> m = steps;
      m.erase(m.begin() + j);
      attempt("dropped step", j, m);
      if (j + 1 < steps.size() && !commute(steps[j], steps[j + 1]))
      {
        m = steps;
        std::swap(m[j], m[j + 1]);
        attempt("swapped steps", j, m);
      }
      if ((steps[j].kind == SmoothStep::STEP || steps[j].kind == SmoothStep::FIRST) && steps[j].x_final != 2)
      {
        m = steps;
        m[j].x_final = 2;
        attempt("x_final set to 2", j, m);
      }
      if (steps[j].clear_q)
      {
        m = steps;
        m[j].clear_q = false;
        attempt("clear_q dropped", j, m);
      }
      if (steps[j].kind == SmoothStep::APPLY)
      {
        m = steps;
        m[j].out = (SmoothStep::Buffer)((steps[j].out + 1) % 3);
        attempt("application output redirected", j, m);
      }
    }
  }
  std::printf("SUMMARY group=mutate mutations=%d undetected=%d\n", mutations, undetected);
  return undetected == 0 ? 0 : 1;
}
} // namespace

int main(int argc, char** argv)
{
  const std::string arg = argc > 1 ? argv[1] : "";
  if (arg == "--list")
  {
    for (const char* g : GROUPS)
      std::printf("%s\n", g);
    std::printf("FLAGS\n");
    for (const char* f : FLAGS)
      std::printf("%s\n", f);
    return 0;
  }
  try
  {
    if (arg == "--mutate")
      return run_mutations();
    for (const char* g : GROUPS)
      if (arg == g)
        return run_group(arg);
  }
  catch (const Violation& v)
  {
    std::printf("FAIL [%s] %s\n", v.invariant.c_str(), v.what.c_str());
    return 1;
  }
  std::fprintf(stderr, "usage: smooth_check fp64|fp32|--list|--mutate\n");
  return 2;
}
