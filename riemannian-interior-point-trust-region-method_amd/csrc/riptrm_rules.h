// riptrm_rules.h — the scalar rules of RIPTRM.run / outer_step / inner_run / inner_step / tCG, once.
//
// The three device engines (MachineT in riptrm_kernels.hip, riptrm_si::Eng, riptrm_gr::Eng) keep
// their own vector work, reductions, barriers, phases and park / resume; every scalar decision of
// the method is taken here.  Scalar in, scalar out: no reductions, no knowledge of an engine's
// storage, and no memory access except tol2() (one table read) and the two writers, which store
// through the pointer they are given.  The build uses -ffp-contract=off, so an expression here
// gives the bits it gave when it stood inline in an engine; keep the parenthesisation.
//
// One exception: tcg_math (riptrm_kernels.hip; k_state's and k_persist's register-resident tCG iteration)
// keeps an inline copy of the tCG rules: on the header it gave the same bits but --dim 1000 --batch 1 ran
// 0.6-1.1% slower (profiles/r9_ab_rules_header.json).  Change the tCG rules in both places.
//
// Where the engines differ on purpose (behaviour, not noise; decide deliberately before changing):
//   - tCG's !isfinite(d_Hd) guard: MachineT (tcg_math, tcg_step) and the Grassmann tCG stop with
//     RIPTRM_TCG_NONFINITE before tcg_curvature; k_si has no guard.  It stays at the call sites.
//   - non-finite checks: Grassmann checks ls, norm_c, Delta, normdx, ared and pred (and a NaN
//     residual); MachineT checks NORMR0, Delta and the residual; k_si checks none.
//   - a log row without inner info: MachineT does not zero the row and writes the last ST_I_* values
//     with HAS_INFO = 0 (ROW_KEEP); k_si and k_gr zero the row and set DUAL_CLIPPING = -1 (ROW_BLANK).
//   - feasibility: MachineT derives x / y feasibility from counts, the other two from minima
//     (vector work, in the engines).
//   - k_gr writes HAS_MINEIG / MINEIGVALHW only in its EXACT instantiation (with_mineig).
//   - stats: MachineT::finish_write adds RIPTRM_STAT_RHS and LOG_BASE and does not zero the block;
//     the other two zero it (write_stats' `zero`).
#pragma once
#include "riptrm_device.h"

namespace riptrm {
namespace rules {

constexpr int TCG_CONTINUE = -1;

// ---- tCG, RIPTRM.py:100-214 ----------------------------------------------------------------------
// Curvature step (:100-160): the interior step length alpha with <eta, eta>_P = e_Pe_new, and whether
// the step leaves the region or the curvature is not positive (boundary).  Then tcg_boundary gives
// the step eta += tau delta that reaches the boundary, and the reason.
struct Curvature {
  double alpha, e_Pe_new;
  bool boundary;
};
__device__ __forceinline__ Curvature tcg_curvature(double d_Hd, double z_r, double e_Pd, double d_Pd, double e_Pe,
                                                   double Delta) {
  Curvature c;
  c.alpha = 0.0;
  if (d_Hd != 0.0) {
    c.alpha = z_r / d_Hd;
    c.e_Pe_new = (e_Pe + 2.0 * c.alpha * e_Pd) + (c.alpha * c.alpha) * d_Pd;
  } else {
    c.e_Pe_new = e_Pe;
  }
  c.boundary = d_Hd <= 0.0 || c.e_Pe_new >= Delta * Delta;
  return c;
}
struct Boundary {
  double tau;
  int stop;
};
__device__ __forceinline__ Boundary tcg_boundary(double d_Hd, double e_Pd, double d_Pd, double e_Pe, double Delta) {
  const double D2 = Delta * Delta;
  Boundary b;
  b.tau = (-e_Pd + sqrt(e_Pd * e_Pd + d_Pd * (D2 - e_Pe))) / d_Pd;
  b.stop = d_Hd <= 0.0 ? RIPTRM_TCG_NEGATIVE_CURVATURE : RIPTRM_TCG_EXCEEDED_TR;
  return b;
}

// Target test (:180-190).  nr0t = pow(nr0, tCG_theta): the caller decides where it is evaluated.
__device__ __forceinline__ int tcg_target(double j, int mininner, double norm_r, double nr0, double nr0t, double kappa) {
  if (j >= (double)mininner && norm_r <= nr0 * fmin(nr0t, kappa))
    return kappa < nr0t ? RIPTRM_TCG_REACHED_TARGET_LINEAR : RIPTRM_TCG_REACHED_TARGET_SUPERLINEAR;
  return TCG_CONTINUE;
}

// Next direction (:192-214) with z = r, so the new <z, r> is r_r: delta' = -r + beta delta (then
// projected by the engine), and afterwards its scalars.  stop = RIPTRM_TCG_MAX_INNER_ITER when
// range(maxinner) is exhausted: Python's j then stays maxinner - 1.
__device__ __forceinline__ double tcg_beta(double r_r, double z_r) { return r_r / z_r; }
struct Advance {
  double z_r, e_Pd, d_Pd, j;
  int stop;
};
__device__ __forceinline__ Advance tcg_advance(double j, int maxinner, double beta, double r_r, double e_Pd, double d_Pd,
                                               double alpha) {
  Advance a;
  a.z_r = r_r;
  a.e_Pd = beta * (e_Pd + alpha * d_Pd);
  a.d_Pd = r_r + (beta * beta) * d_Pd;
  const bool exhausted = j + 1.0 >= (double)maxinner;
  a.j = exhausted ? j : j + 1.0;
  a.stop = exhausted ? RIPTRM_TCG_MAX_INNER_ITER : TCG_CONTINUE;
  return a;
}

// ---- outer loop, RIPTRM.py:866-896 and :931-959 ---------------------------------------------------
// base_solver.check_stoppingcriterion: maxtime before maxiter, tolresid over both
__device__ __forceinline__ int outer_stop(double rt, double outer_it, double residual, const riptrm_options& opt) {
  int stop = RIPTRM_STOP_NONE;
  if (rt >= opt.maxtime) stop = RIPTRM_STOP_MAXTIME;
  else if (outer_it >= (double)opt.maxiter) stop = RIPTRM_STOP_MAXITER;
  if (residual <= opt.tolresid) stop = RIPTRM_STOP_TOLRESID;
  return stop;
}
// restart_every cycling (benchmark windows): back to (x0, y0, mu_0, Delta_0) after outer iteration k, 2k, ...
__device__ __forceinline__ bool restart_due(double outer_it, const riptrm_options& opt) {
  const int k = opt.restart_every;
  return k > 0 && outer_it > 0.0 && fmod(outer_it, (double)k) == 0.0;
}
// index into the per-outer-iteration tables (mu, tolL, tolC, tol2): the last entry repeats
__device__ __forceinline__ int tab_index(int mu_idx, int tab_len) { return mu_idx < tab_len ? mu_idx : tab_len - 1; }
// outer_step tail (:889-896): the next barrier parameter's index, the radius floor
__device__ __forceinline__ void outer_tail(double& mu_idx, double& Delta, const riptrm_options& opt) {
  mu_idx += 1.0;
  const double mn = opt.minimal_initial_tr_radius;
  Delta = Delta > mn ? Delta : mn;
}
// forcing_function_second_order(mu) (:613); reads the table if there is one
__device__ __forceinline__ double tol2(const riptrm_options& opt, int ti, double mu) {
  return opt.tol2_table ? opt.tol2_table[ti] : mu;
}

// ---- step acceptance, update_xy_TR_radius RIPTRM.py:631-705 ---------------------------------------
__device__ __forceinline__ double red_reg(double lb_c, const riptrm_options& opt) {
  return fmax(1.0, fabs(lb_c)) * 2.220446049250313e-16 * opt.reduction_regularization;
}
struct Radius {
  double Dn;
  int ru;
};
__device__ __forceinline__ Radius radius_update(double ared, double pred, double normdx, double Delta,
                                                const riptrm_options& opt) {
  Radius r;
  if (ared < 0.25 * pred) {
    r.ru = RIPTRM_RU_REDUCED;
    r.Dn = 0.25 * Delta;
  } else if (ared >= 0.75 * pred && fabs(normdx - Delta) <= 1e-15) {
    r.ru = RIPTRM_RU_EXPANDED;
    const double d2 = 2.0 * Delta;
    r.Dn = d2 < opt.maximal_tr_radius ? d2 : opt.maximal_tr_radius;
  } else {
    r.ru = RIPTRM_RU_UNCHANGED;
    r.Dn = Delta;
  }
  return r;
}
__device__ __forceinline__ bool accepted(double ared, double pred, const riptrm_options& opt) {
  return ared > opt.rho * pred;
}
// dual clipping (:681-683): the interval's right end with the 3-argument np.maximum quirk, then
// y <- min(max(yN, const_left min(y, mu / sN, 1)), iright)
__device__ __forceinline__ double clip_right(double mu, const riptrm_options& opt) {
  const double cr = opt.const_right;
  return np_max(cr, cr / mu);
}
__device__ __forceinline__ double clip_dual(double y, double yN, double sN, double mu, double iright,
                                            const riptrm_options& opt) {
  const double il = opt.const_left * np_min(np_min(y, mu / sN), 1.0);
  return np_min(np_max(yN, il), iright);
}

// ---- inner_run's limits, RIPTRM.py:810-847 --------------------------------------------------------
// 0, or the RIPTRM_IS_MAX_* status the reset reports (the iteration limit wins over the time limit).
// Without inner_maxtime the limit is maxtime on the whole run's clock.
__device__ __forceinline__ int inner_limit(double tn, double t_start, double t_inner, double clock_hz, double inner_it,
                                           const riptrm_options& opt) {
  double rt, lim;
  if (opt.inner_maxtime < 0.0) {
    lim = opt.maxtime;
    rt = (tn - t_start) / clock_hz;
  } else {
    lim = opt.inner_maxtime;
    rt = (tn - t_inner) / clock_hz;
  }
  const bool tmo = rt >= lim;
  const bool imax = opt.inner_maxiter >= 0 && inner_it >= (double)opt.inner_maxiter;
  if (!(tmo || imax)) return 0;
  return imax ? RIPTRM_IS_MAX_ITER_EXCEEDED : RIPTRM_IS_MAX_TIME_EXCEEDED;
}

// ---- records --------------------------------------------------------------------------------------
struct Info {  // inner-iteration record of solver_status (RIPTRM.py:986-1023)
  double has, num, status, tr, dxtype, normdx, minx, miny, compl_, hasratio, ratio, ru, dc, hasmin, mineig;
};
// a row without inner info (solver_status(..., inner_info=None)): ROW_KEEP leaves the row as it is
// and writes inf's fields with HAS_INFO = 0; ROW_BLANK zeroes the row and sets DUAL_CLIPPING = -1
enum RowStyle : int { ROW_KEEP = 0, ROW_BLANK = 1 };

// One log row at L.  ev: cost, distance, residual, gradnorm, complvio, dualvio, manvio, maxvio,
// meanvio, maxabsy.  time: log_time() of the row.
__device__ __forceinline__ double log_time(bool first, double t_now, double t_start, double clock_hz) {
  return first ? 0.0 : (t_now - t_start) / clock_hz;   // the solve's first row has time 0
}
__device__ __forceinline__ void write_log_row(double* L, RowStyle style, double outer_it, double time,
                                              const double (&ev)[10], double mu, double tcg_iters, const Info& inf,
                                              bool has_info, bool with_mineig) {
  if (style == ROW_BLANK)
    for (int k = 0; k < RIPTRM_LOG_NFIELDS; ++k) L[k] = 0.0;
  L[RIPTRM_LOG_ITERATION] = outer_it;
  L[RIPTRM_LOG_TIME] = time;
  L[RIPTRM_LOG_COST] = ev[0];
  L[RIPTRM_LOG_DISTANCE] = ev[1];
  L[RIPTRM_LOG_RESIDUAL] = ev[2];
  L[RIPTRM_LOG_GRADNORM] = ev[3];
  L[RIPTRM_LOG_COMPLVIOLATION] = ev[4];
  L[RIPTRM_LOG_DUALVIOLATION] = ev[5];
  L[RIPTRM_LOG_MANVIOLATION] = ev[6];
  L[RIPTRM_LOG_MAXVIOLATION] = ev[7];
  L[RIPTRM_LOG_MEANVIOLATION] = ev[8];
  L[RIPTRM_LOG_MU] = mu;
  L[RIPTRM_LOG_MAXABSLAGMULT] = ev[9];
  L[RIPTRM_LOG_TCG_ITERS] = tcg_iters;
  if (has_info || style == ROW_KEEP) {
    L[RIPTRM_LOG_HAS_INFO] = has_info ? inf.has : 0.0;
    L[RIPTRM_LOG_NUM_INNER] = inf.num;
    L[RIPTRM_LOG_INNER_STATUS] = inf.status;
    L[RIPTRM_LOG_TR_RADIUS] = inf.tr;
    L[RIPTRM_LOG_DXTYPE] = inf.dxtype;
    L[RIPTRM_LOG_NORMDX] = inf.normdx;
    L[RIPTRM_LOG_MINXFEASI] = inf.minx;
    L[RIPTRM_LOG_MINYFEASI] = inf.miny;
    L[RIPTRM_LOG_COMPL] = inf.compl_;
    L[RIPTRM_LOG_HAS_RATIO] = inf.hasratio;
    L[RIPTRM_LOG_ARED_PRED] = inf.ratio;
    L[RIPTRM_LOG_RADIUS_UPDATE] = inf.ru;
    L[RIPTRM_LOG_DUAL_CLIPPING] = inf.dc;
    if (with_mineig) {
      L[RIPTRM_LOG_HAS_MINEIG] = inf.hasmin;
      L[RIPTRM_LOG_MINEIGVALHW] = inf.mineig;
    }
  } else {
    L[RIPTRM_LOG_DUAL_CLIPPING] = -1.0;
  }
}

struct Stats {
  double outer_it, inner_total, tcg_total, passes, stop_code, stop_rt, residual, log_count, log_over, phase, error, mu,
      Delta, last_j, last_stop;
};
// The result record at o; zero: clear the whole block first (fields an engine does not have read 0)
__device__ __forceinline__ void write_stats(double* o, bool zero, const Stats& st) {
  if (zero)
    for (int k = 0; k < RIPTRM_STAT_NFIELDS; ++k) o[k] = 0.0;
  o[RIPTRM_STAT_OUTER_ITERS] = st.outer_it;
  o[RIPTRM_STAT_INNER_ITERS] = st.inner_total;
  o[RIPTRM_STAT_TCG_ITERS] = st.tcg_total;
  o[RIPTRM_STAT_PASSES] = st.passes;
  o[RIPTRM_STAT_STOP_CODE] = st.stop_code;
  o[RIPTRM_STAT_STOP_RUNTIME] = st.stop_rt;
  o[RIPTRM_STAT_FINAL_RESIDUAL] = st.residual;
  o[RIPTRM_STAT_LOG_COUNT] = st.log_count;
  o[RIPTRM_STAT_LOG_OVERFLOW] = st.log_over;
  o[RIPTRM_STAT_PHASE] = st.phase;
  o[RIPTRM_STAT_ERROR] = st.error;
  o[RIPTRM_STAT_MU] = st.mu;
  o[RIPTRM_STAT_TR_RADIUS] = st.Delta;
  o[RIPTRM_STAT_TCG_LAST_J] = st.last_j;
  o[RIPTRM_STAT_TCG_LAST_STOP] = st.last_stop;
}

}  // namespace rules
}  // namespace riptrm
