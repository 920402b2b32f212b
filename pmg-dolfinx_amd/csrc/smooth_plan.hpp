// The schedule of one Chebyshev smooth (src/chebyshev.hpp:46-91): which operator applications and vector passes a call
// issues, in which order, into which buffers, and what it leaves to its consumer, is decided here and nowhere else.
// cheb_iterate (solvers.hip) turns the steps into HIP calls, the callers read smooth_outcome instead of asking the
// conditions again, and the host checker (tests/host/smooth_check.cpp) executes the steps serially on std::vector.
// No HIP call, nothing on the heap.
#pragma once

#include "../../include/pmg_amd.h"

namespace pmg
{
int fail(int code, const char* fmt, ...);

// what the caller wants of the residual b - A x
enum : int
{
  ResidualNone = 0,    // only x is wanted: the loop's last application is skipped
  ResidualUpdated = 1, // w.r = b - A x on return (costs that last application)
  ResidualSplit = 2,   // the caller can subtract while it gathers: the last "r -= q" may be left to it
                       // (SmoothOutcome::LeftSplit: b - A x = w.r - w.q)
  ResidualFused = 3    // the caller can form A w.z on the fly (interp_restrict_residual): the last application itself
                       // may be left to it (SmoothOutcome::LeftFused: b - A x = w.r - A w.z)
};
// A one-step smoother, whose only kernel updates x and r together, keeps its own path under ResidualSplit and
// ResidualFused and leaves nothing: w.r = b - A x.  A caller that cannot consume either asks for ResidualUpdated.

// Everything that decides the sequence, and nothing else.
struct SmoothCall
{
  int k = 1;                    // steps
  int need_r = ResidualNone;    // Residual*
  bool x_zero = false;          // x counts as 0 on entry, whatever it holds (A 0 = 0, so r = b and x := z)
  // The operator's launch accumulates with atomics (a merged small level): its output must be zero over [0, n_total).
  // The vector passes then clear w.q behind themselves and every application after the first takes the zeroed-output
  // variant (no zero-fill kernels); the first application of x takes the plain one, which fills for itself.
  bool zeroed_output = false;
  // Ghost bookkeeping of the iterate (several ranks): every application refreshes the ghost entries of its INPUT, so
  // the ghosts of z are current right behind A z.  With ghosts > 0 (the number of ghost entries behind the n owned
  // ones) the smooth adds them to the ghosts of x there, a pass over the ghost range only: after a smooth that returns
  // its residual, x has current ghosts without an exchange of its own.
  int ghosts = 0;
  bool ghosts_current = false;  // the ghosts of x are current on entry: the first application, A x, needs no exchange
  bool allow_recompute = false; // the recomputed form may be taken: the smoother's mode asks for it, q1 and q2 exist
  bool fp64 = true;             // the scalar type: double, or float (the FP32 cycle)
};

struct SmoothStep
{
  enum Kind
  {
    APPLY,       // out = A in
    INIT,        // r = b (- q) ; z = c0 dinv r                                      (ChebInitF)
    FIRST,       // first step from x = 0: r -= q ; z = c1 z + c2 dinv r ; x = z_1 + z  (ChebFirstF)
    STEP,        // r -= q ; z = c1 z + c2 dinv r ; x += (z_1 if both) + z            (ChebStepF)
    LAST,        // the only step of a one-step smoother with a residual: x (+)= z ; r -= q  (ChebLastF)
    RESIDUAL,    // r -= q                                                           (ChebResidualF)
    ADD,         // x += z
    GHOST_ADD,   // the same over the ghost entries
    COPY,        // x = z
    ZERO_X,      // x = 0
    ZERO_GHOSTS, // the ghost entries of x = 0
    RECOMPUTE    // stage 1, 2, 3 of the recomputed form                             (ChebRecomputeF)
  } kind;
  // APPLY
  enum Variant
  {
    PLAIN,
    ZEROED_OUTPUT, // adds into an output that is zero over [0, n_total)
    GHOSTS_CURRENT // trusts the ghosts of its input
  } variant = PLAIN;
  enum Buffer
  {
    Q,
    Q1,
    Q2
  } out = Q;
  bool in_x = false; // the input is x (else z)
  // the vector passes
  int i = 0;            // the step whose coefficients the pass takes: c0 (i = 0), c1(i) and c2(i); RECOMPUTE: stage - 1
  bool clear_q = false; // w.q = 0 over [0, n_total) behind the pass (ThenClearF)
  bool with_q = false;  // INIT: r = b - q (else r = b); RECOMPUTE: q0 = w.q is read (else from x = 0)
  bool both = false;    // STEP: the first step, which adds z_1 as well
  int x_final = 0;      // FIRST, STEP: 1, 2 the last correction enters x; 2: r and z are dead and not written
  bool assign = false;  // LAST: x = z
  int stage = 0;        // RECOMPUTE
  bool with_q2 = false; // RECOMPUTE stage 3: a smooth of three steps
  bool r_out = false;   // RECOMPUTE stage 3: r and z are written as well (the fused restriction reads them)
};

struct SmoothOutcome
{
  enum Left
  {
    LeftNone,  // the caller's residual, where it asked for one, is w.r
    LeftSplit, // b - A x = w.r - w.q
    LeftFused  // b - A x = w.r - A w.z; x is final
  };
  bool recomputed = false;
  Left left_to_consumer = LeftNone;
  int applications = 0;
  int vector_launches = 0; // every step that is no application
};

// The coefficients of the 4th-kind Chebyshev recurrence (src/chebyshev.hpp:68,80,83): formed in FP64 here, rounded once
// to the scalar type where a pass takes them.
inline double cheb_c0(double lmax) { return 4.0 / (3.0 * lmax); }
inline double cheb_c1(int i) { return (2.0 * i - 1.0) / (2.0 * i + 3.0); }
inline double cheb_c2(int i, double lmax) { return (8.0 * i + 4.0) / (2.0 * i + 3.0) / lmax; }

// f(const SmoothStep&) -> int (PMG_OK to go on) for the steps of the call, in issue order; *left (optional) is what the
// call leaves to its consumer.
//   stored form      A x (skipped from x = 0); init; then per step an application of z and one fused pass.  x absorbs
//                    the correction z_{i+1} in the pass that computes it (the first adds z_1 and z_2), so after the
//                    last application only the residual is left to update, and only where it is wanted.
//   recomputed form  FP64, k = 2 or 3, ResidualNone or ResidualFused, plain operator outputs, no ghost bookkeeping:
//                    q0 = A x, q1 = A z_1, q2 = A z_2 each in a buffer of its own and three (k = 2: two) passes that
//                    form the residual ((b - q0) - q1) - q2 in registers.  The last application is never issued.
//                    Launches and applications are those of the stored form.
template <typename F>
int for_each_smooth_step(const SmoothCall& c, F&& f, SmoothOutcome::Left* left = nullptr)
{
  if (left)
    *left = SmoothOutcome::LeftNone;
  if (!c.fp64 && c.zeroed_output)
    return fail(PMG_ERR_INVALID, "cheb_iterate: the FP32 passes have no zeroed-output form");
  if (!c.fp64 && c.allow_recompute) // the float loop keeps the stored form: no silent mixing
    return fail(PMG_ERR_INVALID, "cheb_iterate: the FP32 passes have no recomputed form");
  const int k = c.k;
  SmoothStep st{};
  auto apply = [&](SmoothStep::Variant v, bool in_x, SmoothStep::Buffer out)
  {
    st = SmoothStep{SmoothStep::APPLY};
    st.variant = v, st.in_x = in_x, st.out = out;
    return f(st);
  };
  auto pass = [&](SmoothStep::Kind kind, int i, bool clear_q) -> SmoothStep&
  {
    st = SmoothStep{kind};
    st.i = i, st.clear_q = clear_q;
    return st;
  };
#define PMG_EMIT_(expr)                                                                                                \
  do                                                                                                                   \
  {                                                                                                                    \
    if (const int rc_ = (expr); rc_ != PMG_OK)                                                                         \
      return rc_;                                                                                                      \
  } while (0)

  if (c.allow_recompute && (k == 2 || k == 3) && (c.need_r == ResidualNone || c.need_r == ResidualFused)
      && !c.zeroed_output && c.ghosts == 0 && !c.ghosts_current)
  {
    const bool fused = c.need_r == ResidualFused;
    if (!c.x_zero)
      PMG_EMIT_(apply(SmoothStep::PLAIN, true, SmoothStep::Q)); // :56
    for (int stage = 1; stage <= 3; ++stage)
    {
      if (stage == 2 && k == 2)
        continue;
      SmoothStep& p = pass(SmoothStep::RECOMPUTE, stage - 1, false);
      p.stage = stage, p.with_q = !c.x_zero, p.with_q2 = stage == 3 && k == 3, p.r_out = stage == 3 && fused;
      PMG_EMIT_(f(p));
      if (stage < 3)
        PMG_EMIT_(apply(SmoothStep::PLAIN, false, stage == 1 ? SmoothStep::Q1 : SmoothStep::Q2)); // :76
    }
    if (fused && left)
      *left = SmoothOutcome::LeftFused; // x is final; w.r and w.z are what the consumer reads
    return PMG_OK;
  }

  const bool clear = c.zeroed_output; // the passes leave w.q zero for the next application ...
  const SmoothStep::Variant next = clear ? SmoothStep::ZEROED_OUTPUT : SmoothStep::PLAIN; // ... which needs no fill
  if (c.x_zero)
  {
    PMG_EMIT_(f(pass(SmoothStep::INIT, 0, clear)));
    if (c.ghosts > 0)
      PMG_EMIT_(f(pass(SmoothStep::ZERO_GHOSTS, 0, false)));
  }
  else
  {
    PMG_EMIT_(apply(c.ghosts_current ? SmoothStep::GHOSTS_CURRENT : SmoothStep::PLAIN, true, SmoothStep::Q)); // :56
    pass(SmoothStep::INIT, 0, clear).with_q = true;                                                          // :57,67-68
    PMG_EMIT_(f(st));
  }
  for (int i = 1; i <= k; ++i)
  {
    const bool last = i == k;
    if (last && c.need_r == ResidualNone)
    {
      if (k == 1) // a one-step smoother: z_1 is all there is (:73)
        PMG_EMIT_(f(pass(c.x_zero ? SmoothStep::COPY : SmoothStep::ADD, 0, false)));
      break;
    }
    if (last && c.need_r == ResidualFused && k > 1)
    {
      if (left)
        *left = SmoothOutcome::LeftFused; // x is final (x_final below); w.r and w.z are what the consumer reads
      break;
    }
    PMG_EMIT_(apply(next, false, SmoothStep::Q)); // :76
    if (c.ghosts > 0)                             // the ghosts of z are current now: the iterate's ghosts absorb them
      PMG_EMIT_(f(pass(SmoothStep::GHOST_ADD, 0, false)));
    if (last) // a residual is wanted: the new z would not be used, only x and r are (:73,77)
    {
      if (k == 1)
      {
        pass(SmoothStep::LAST, 0, false).assign = c.x_zero;
        PMG_EMIT_(f(st));
      }
      else if (c.need_r == ResidualSplit)
      {
        if (left)
          *left = SmoothOutcome::LeftSplit;
      }
      else
        PMG_EMIT_(f(pass(SmoothStep::RESIDUAL, 0, false)));
      break;
    }
    // the last correction enters x here (1); when no residual is wanted either, r and z are dead behind this step (2)
    SmoothStep& p = pass(c.x_zero && i == 1 ? SmoothStep::FIRST : SmoothStep::STEP, i, clear); // :73,77,80-83
    p.both = i == 1 && !c.x_zero;
    p.x_final = i + 1 == k ? (c.need_r == ResidualNone ? 2 : 1) : 0;
    PMG_EMIT_(f(p));
  }
  if (k == 0 && c.x_zero)
    PMG_EMIT_(f(pass(SmoothStep::ZERO_X, 0, false)));
  return PMG_OK;
#undef PMG_EMIT_
}

// What the call comes to, from the same walk; a call that cannot be scheduled comes to nothing (the visitor has said why).
inline SmoothOutcome smooth_outcome(const SmoothCall& c)
{
  SmoothOutcome o;
  const int rc = for_each_smooth_step(
      c,
      [&o](const SmoothStep& st)
      {
        if (st.kind == SmoothStep::APPLY)
          o.applications++;
        else
          o.vector_launches++;
        o.recomputed = o.recomputed || st.kind == SmoothStep::RECOMPUTE;
        return PMG_OK;
      },
      &o.left_to_consumer);
  return rc == PMG_OK ? o : SmoothOutcome{};
}
} // namespace pmg
