// riptrm_grassmann.hip — RIPTRM (tCG path) for the Rosenbrock problem on Grassmann(n, k), MI355X (gfx950).
//
// Problem (src/Rosenbrock/coordinator.py:33-95): X is n x k with X^T X = I, v = X.flatten() (row-major,
// N = n k entries), f = sum_{i < N-1} alpha (v_{i+1} - v_i)^2 + (1 - v_i)^2 and the N constraints
// g_i = -v_i - lb <= 0 (slack s = v + lb).  f is quadratic: its Euclidean Hessian is the constant
// tridiagonal operator T, egrad f = T v - 2 (1, .., 1, 0).  The reference config has n = 5, k = 3, so one
// workgroup runs one instance's WHOLE solve in one launch, as riptrm_si.hip does: NT = 64 ceil(N / 64)
// threads, thread l owns element l = (l / k, l % k) of every n x k vector.
//
// Math = tests/rosenbrock_oracle.py::RosenbrockVectorized (pymanopt's Grassmann restated), with
// P_X(U) = U - X (X^T U), Y the multipliers as n x k, G_L = egrad f - Y:
//   HwCur(V)  = P_X(T V + (Y o P_X(V)) / S) - V (X^T G_L)        RIPTRM.py:491-571, :729
//   c         = P_X(egrad f - mu / S)                             RIPTRM.py:730
//   dy        = -y + mu / s - y o vec(P_X(dx)) / s                RIPTRM.py:743
//   retraction: A = X + U, G = A^T A = V L V^T, A V L^-1/2 V^T    (the polar factor; pymanopt u @ vt)
//   dist(X, Y) = || arccos(min(sigma(X^T Y), 1)) ||_2
// Control flow = RIPTRM.py:41-216 (tCG), :574-629, :631-705, :707-896, :909-976, the plain loops of
// riptrm_si.hip.
//
// LDS per instance (dynamic, gr_lds_doubles): 13 vectors of NT doubles (X, Y, S, eta, Heta, r, delta,
// H delta, c, the trial point, G_L and two scratch vectors), four 8 x 8 factors (X^T U products, the
// polar factor, X^T G_L, the Jacobi rotations), 8 singular values and the 2 NT / 64 reduction slots:
//   N <= 64 (the reference's 5 x 3):  8.6 KiB  (18 instances would fit the 160 KiB of a compute unit)
//   N = 512 (the limit):             54.2 KiB  (2 workgroups of 8 waves per compute unit)
// Registers, not LDS, bound the occupancy: the state machine is inlined into one kernel and takes 255
// VGPRs, i.e. one wave per SIMD: 4 one-wave workgroups per compute unit at N <= 64 (what
// riptrm_gr_launch_info reports).  A batch of 256 instances is one workgroup per compute unit anyway.
// The iterates a thread alone reads (the outer step's start, the initial point, the previous log row's
// point) stay in its registers.  T u is a neighbour exchange (element l reads l - 1 and l + 1 across row
// ends); the k x k products are k^2 sums over n, one thread each, in row order; the k x k Jacobi work
// runs on wave 0: a one-sided (Hestenes) cyclic Jacobi in which every lane rotates the rows it owns and
// the column products are DPP wave sums, so it needs no barrier until it is done.  For the symmetric
// positive definite G it yields G = V L V^T (G V has orthogonal columns of norms L); for X^T Y and for X
// itself (the rank test of src/Rosenbrock/simulator.py:107-114) it yields the singular values directly
// rather than through the eigenvalues of C^T C, which would square away the digits arccos needs.
//
// Exact_RepMat (RIPTRM.py:433-444, :599-617) is the EXACT instantiation of the same engine, k_gr_exact: in
// place of tcg() it builds the matrix of HwCur in the pinned Householder frame of X (rosenbrock.basisfun =
// riptrm_grassmann_ops.h's Ops::qr_frame, which k_gr_so shares together with the pieces of HwCur; the
// reference's upper-triangle mirror, which on this problem depends on the frame) and calls the LDS subproblem
// solver of riptrm_trs.h; with second_order_stationarity the same matrix at the trial point gives
// mineigvalHw.  The tCG kernels k_gr are compiled as they were (DESIGN.md 7e has the resource table).
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <cstring>
#include <string>
#include "riptrm_ctx.h"
#include "riptrm_rules.h"
#include "riptrm_wave.h"
#include "riptrm_trs.h"
#include "riptrm_grassmann_ops.h"

namespace riptrm_gr {

#pragma clang fp contract(off)

using namespace riptrm_gr_dev;
namespace rules = riptrm::rules;
using rules::Info;
using riptrm::round_up;

constexpr int NKMAX = RIPTRM_GR_NKMAX;
constexpr int NVEC = 13;

enum Mode : int { MODE_SOLVE = 0, MODE_HVP = 1, MODE_TCG = 2, MODE_OPS = 3, MODE_EXACT = 4 };

struct GRParams {
  int32_t n, k, batch, cap, mode, tab_len;
  double clock_hz;
  const double* alpha;
  int64_t alpha_stride;
  const double* lb;
  int64_t lb_stride;
  double* x;       // batch x N   current point / result
  double* y;       // batch x N
  double* eta;     // batch x N
  double* heta;    // batch x N
  double* stats;   // batch x RIPTRM_STAT_NFIELDS
  double* log;     // batch x cap x RIPTRM_LOG_NFIELDS
  double* trail;   // batch x cap x 2 N: the (x, y) of every log record (TRAIL instantiation), or null
  const double* in_x;
  const double* in_y;
  const double* in_mu;
  const double* in_delta;
  const double* in_v;
  double* out_v;
  double* out_retr;
  double* out_dist;
  int32_t* out_rank;
  const double* mu_tab;
  const double* tolL_tab;
  const double* tolC_tab;
  riptrm_options opt;
  // MODE_EXACT outputs (riptrm_gr_exact); out_v takes dx
  double* out_A;        // batch x d x d
  double* out_a;        // batch x d
  double* out_lam;      // batch
  double* out_mineig;   // batch
  int32_t* out_kind;    // batch  RIPTRM_TRS_*, or RIPTRM_TCG_NONFINITE / RIPTRM_TCG_EIGFAIL
};

struct Layout {
  int64_t off_x, off_y, off_eta, off_heta, off_stats, off_log, total;
};

inline Layout make_layout(int n, int k, int batch, int cap) {
  Layout L;
  const int64_t v = 8LL * batch * n * k;
  int64_t o = 0;
  L.off_x = o;     o = round_up(o + v, 256);
  L.off_y = o;     o = round_up(o + v, 256);
  L.off_eta = o;   o = round_up(o + v, 256);
  L.off_heta = o;  o = round_up(o + v, 256);
  L.off_stats = o; o = round_up(o + 8LL * batch * RIPTRM_STAT_NFIELDS, 256);
  L.off_log = o;   o = round_up(o + 8LL * batch * cap * RIPTRM_LOG_NFIELDS, 256);
  L.total = o;
  return L;
}

__host__ __device__ constexpr int gr_lds_doubles(int NT) { return NVEC * NT + 4 * KK + KMAX + 2 * (NT / 64); }

// ---- Exact_RepMat (the EXACT instantiation) -------------------------------------------------------
// The subproblem's work area (riptrm_trs::work_doubles(d): the matrix, its eigenvectors, the vectors
// and the Jacobi rotation table) sits behind k_gr's own area and the frame's 2 KMAX scalars (column
// dots, reflector scales).  The frame's reflectors, the frame vector and its image take R, DEL and
// HETA, which only tCG uses.  The workgroup has FRAME_NT_MAX threads at most, and the limit on d is what
// fits one workgroup's 160 KiB at that width.
__host__ __device__ constexpr int gr_exact_lds_doubles(int NT, int d) {
  return gr_lds_doubles(NT) + 2 * KMAX + riptrm_trs::work_doubles(d);
}
constexpr int exact_dim_max() {
  int d = 0;
  while (d < riptrm_trs::DIM_MAX && (int64_t)gr_exact_lds_doubles(FRAME_NT_MAX, d + 1) * 8 <= LDS_LIMIT) ++d;
  return d;
}
constexpr int EXACT_DMAX = exact_dim_max();
static_assert(EXACT_DMAX >= 80, "every shape with k (n - k) <= 80 must fit");

template <int NT, bool TRAIL, bool EXACT = false>
struct Eng : Ops {
  const GRParams& P;
  const int b;
  lf *Y, *S, *ETA, *HETA, *R, *DEL, *HD, *C, *XN, *GL, *W2;   // NT doubles each, with Ops' X and W1
  lf *M1, *M2, *MG, *VV;   // KMAX x KMAX factors (row stride k)
  lf *SIG;                 // KMAX singular values
  riptrm_trs::Blk<NT> blk;
  // EXACT only: the frame (Ops' REF = R, BETA and CW), the frame vector FV = DEL and its image
  // FH = HETA, the subproblem's work area
  lf *FV, *FH;
  double* trs_lds;

  __device__ __forceinline__ Eng(const GRParams& P_, int b_, double* lds)
      : Ops(P_.n, P_.k), P(P_), b(b_), blk(lds + NVEC * NT + 4 * KK + KMAX) {
    lf* base = (lf*)lds;
    X = base;            Y = base + NT;       S = base + 2 * NT;    ETA = base + 3 * NT;
    HETA = base + 4 * NT; R = base + 5 * NT;   DEL = base + 6 * NT;  HD = base + 7 * NT;
    C = base + 8 * NT;   XN = base + 9 * NT;  GL = base + 10 * NT;  W1 = base + 11 * NT;
    W2 = base + 12 * NT;
    lf* f = base + NVEC * NT;
    M1 = f; M2 = f + KK; MG = f + 2 * KK; VV = f + 3 * KK; SIG = f + 4 * KK;
    REF = R; FV = DEL; FH = HETA;
    CW = base + gr_lds_doubles(NT); BETA = CW + KMAX;
    trs_lds = lds + gr_lds_doubles(NT) + 2 * KMAX;
    alpha = P.alpha[(int64_t)b * P.alpha_stride];
    lb = P.lb[(int64_t)b * P.lb_stride];
  }

  __device__ __forceinline__ double bsum(double v) { return blk.sum(v); }
  __device__ __forceinline__ double bmin(double v) { return blk.min(v); }
  __device__ __forceinline__ double bmax(double v) { return blk.max(v); }
  __device__ __forceinline__ double dot(const lf* a, const lf* c) { return bsum(act ? a[l] * c[l] : 0.0); }

  __device__ __forceinline__ double cost(const lf* Xp) {
    double t = 0.0;
    if (act && l < N - 1) {
      const double v = Xp[l], d = Xp[l + 1] - v, o = 1.0 - v;
      t = alpha * d * d + o * o;
    }
    return bsum(t);
  }

  // OUT = P_Xp(U) = U - Xp (Xp^T U); OUT may be U.  Xp, U visible; OUT visible on return
  __device__ __forceinline__ void proj_to(lf* OUT, const lf* Xp, const lf* U) {
    xtu(M1, Xp, U);
    const double v = act ? U[l] - rowmul(Xp, M1) : 0.0;
    OUT[l] = v;
    __syncthreads();
  }

  // ---- one-sided cyclic Jacobi on the r x k matrix B (row stride k), wave 0 ------------------------
  // Rotates column pairs until they are orthogonal: SIG = the column norms = B's singular values; with
  // wantv, VV = the accumulated rotations (B0 VV has the orthogonal columns).  Lane t owns rows t,
  // t + 64, .. of B and row t of VV; the column products are wave sums, identical on every lane, so
  // control flow is uniform.  B visible before; SIG / VV visible on return.
  __device__ __forceinline__ void jacobi(lf* B, int r, bool wantv) {
    if (l < 64) {
      if (wantv && l < k)
        for (int c = 0; c < k; ++c) VV[l * k + c] = (c == l) ? 1.0 : 0.0;
      for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < k - 1; ++p)
          for (int q = p + 1; q < k; ++q) {
            double a = 0.0, c2 = 0.0, g = 0.0;
            for (int row = l; row < r; row += 64) {
              const double bp = B[row * k + p], bq = B[row * k + q];
              a = a + bp * bp;
              c2 = c2 + bq * bq;
              g = g + bp * bq;
            }
            a = riptrm_wave::wave_sum(a);
            c2 = riptrm_wave::wave_sum(c2);
            g = riptrm_wave::wave_sum(g);
            if (g != 0.0 && fabs(g) > 1e-15 * sqrt(a * c2)) {
              rotated = true;
              const double zeta = (c2 - a) / (2.0 * g);
              const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
              const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
              for (int row = l; row < r; row += 64) {
                const double bp = B[row * k + p], bq = B[row * k + q];
                B[row * k + p] = cs * bp - sn * bq;
                B[row * k + q] = sn * bp + cs * bq;
              }
              if (wantv && l < k) {
                const double vp = VV[l * k + p], vq = VV[l * k + q];
                VV[l * k + p] = cs * vp - sn * vq;
                VV[l * k + q] = sn * vp + cs * vq;
              }
            }
          }
        if (!rotated) break;
      }
      for (int j = 0; j < k; ++j) {
        double a = 0.0;
        for (int row = l; row < r; row += 64) {
          const double bj = B[row * k + j];
          a = a + bj * bj;
        }
        a = riptrm_wave::wave_sum(a);
        if (l == 0) SIG[j] = sqrt(a);
      }
    }
    __syncthreads();
  }

  // OUT = the polar factor of Xp + U (pymanopt Grassmann.retraction); OUT may be Xp or U (it is written
  // after their last read).  Xp, U visible; OUT visible on return
  __device__ __forceinline__ void retract_to(lf* OUT, const lf* Xp, const lf* U) {
    W2[l] = act ? Xp[l] + U[l] : 0.0;
    __syncthreads();
    xtu(M1, W2, W2);
    jacobi(M1, k, true);
    if (l < kk) {   // V L^-1/2 V^T
      const int a = l / k, c = l % k;
      double acc = 0.0;
      for (int j = 0; j < k; ++j) acc = acc + (VV[a * k + j] * VV[c * k + j]) / sqrt(SIG[j]);
      M2[l] = acc;
    }
    __syncthreads();
    const double v = rowmul(W2, M2);
    OUT[l] = v;
    __syncthreads();
  }

  // pymanopt Grassmann.dist: the 2-norm of the principal angles.  A, B visible
  __device__ __forceinline__ double dist(const lf* A, const lf* B) {
    xtu(M1, A, B);
    jacobi(M1, k, false);
    double acc = 0.0;
    for (int j = 0; j < k; ++j) {
      const double s = SIG[j];
      const double th = acos(s < 1.0 ? s : 1.0);
      acc = acc + th * th;
    }
    return sqrt(acc);
  }

  // numpy.linalg.matrix_rank(Xp) == k (src/Rosenbrock/simulator.py:107-114).  Xp visible
  __device__ __forceinline__ bool full_rank(const lf* Xp) {
    W2[l] = act ? Xp[l] : 0.0;
    __syncthreads();
    jacobi(W2, n, false);
    double smax = 0.0;
    for (int j = 0; j < k; ++j) smax = fmax(smax, SIG[j]);
    const double tol = smax * (double)(n > k ? n : k) * DBL_EPSILON;   // numpy's finfo(float64).eps
    int rank = 0;
    for (int j = 0; j < k; ++j) rank += (SIG[j] > tol) ? 1 : 0;
    return rank == k;
  }

  // ---- the inner iteration's operators at (X, Y, mu) ----------------------------------------------
  // S, G_L, X^T G_L and c; returns f(X).  X, Y visible
  __device__ __forceinline__ double prepare(double mu) {
    const double s = act ? X[l] + lb : 1.0;
    const double ef = egrad_f(X);
    S[l] = s;
    GL[l] = act ? ef - Y[l] : 0.0;
    W2[l] = act ? ef - mu / s : 0.0;
    __syncthreads();
    xtu(MG, X, GL);
    proj_to(C, X, W2);
    return cost(X);
  }
  // OUT = HwCur(V); OUT is not V.  V visible; OUT visible on return
  __device__ __forceinline__ void hw(lf* OUT, const lf* V) {
    proj_to(W1, X, V);
    const double tv = Tu(V);
    W2[l] = act ? tv + (Y[l] * W1[l]) / S[l] : 0.0;
    __syncthreads();
    xtu(M1, X, W2);
    const double v = act ? (W2[l] - rowmul(X, M1)) - rowmul(V, MG) : 0.0;
    OUT[l] = v;
    __syncthreads();
  }
  // || P_Xp(egrad f(Xp) - y) ||.  Xp visible; y = this thread's multiplier
  __device__ __forceinline__ double gradlag_norm(const lf* Xp, double y) {
    const double ef = egrad_f(Xp);
    W2[l] = act ? ef - y : 0.0;
    __syncthreads();
    proj_to(W1, Xp, W2);
    const double g = act ? W1[l] : 0.0;
    return sqrt(bsum(g * g));
  }

  // ---- tCG, RIPTRM.py:41-216 (eta0 = 0, identity preconditioner); eta / Heta in ETA / HETA -------
  __device__ __forceinline__ int tcg(double Delta, int& jout, double& hvps) {
    const int maxinner = k * (n - k);   // manifold.dim
    ETA[l] = 0.0;
    HETA[l] = 0.0;
    R[l] = C[l];
    DEL[l] = -C[l];
    __syncthreads();
    double e_Pe = 0.0;
    double r_r = dot(R, R);
    double norm_r = sqrt(r_r);
    const double norm_r0 = norm_r;
    double z_r = r_r;
    double d_Pd = z_r;
    double e_Pd = 0.0;
    double model = 0.0;
    int stop = RIPTRM_TCG_MAX_INNER_ITER;
    int j = 0;
    const double nr0t = pow(norm_r0, P.opt.tcg_theta);   // constant over the run
    for (j = 0; j < maxinner; ++j) {
      hw(HD, DEL);
      hvps += 1.0;
      const double d_Hd = dot(DEL, HD);
      if (!isfinite(d_Hd)) {
        stop = RIPTRM_TCG_NONFINITE;
        break;
      }
      const rules::Curvature cv = rules::tcg_curvature(d_Hd, z_r, e_Pd, d_Pd, e_Pe, Delta);
      const double al = cv.alpha;
      if (cv.boundary) {
        const rules::Boundary bd = rules::tcg_boundary(d_Hd, e_Pd, d_Pd, e_Pe, Delta);
        ETA[l] = ETA[l] + bd.tau * DEL[l];
        HETA[l] = HETA[l] + bd.tau * HD[l];
        __syncthreads();
        stop = bd.stop;
        break;
      }
      e_Pe = cv.e_Pe_new;
      const double ne = ETA[l] + al * DEL[l];
      const double nh = HETA[l] + al * HD[l];
      const double cl = act ? C[l] : 0.0;
      const double nm = bsum(act ? ne * cl : 0.0) + 0.5 * bsum(act ? ne * nh : 0.0);
      if (nm >= model) {
        stop = RIPTRM_TCG_MODEL_INCREASED;
        break;
      }
      ETA[l] = ne;
      HETA[l] = nh;
      model = nm;
      const double rn = R[l] + al * HD[l];
      R[l] = rn;
      r_r = bsum(act ? rn * rn : 0.0);
      norm_r = sqrt(r_r);
      const int target = rules::tcg_target((double)j, P.opt.tcg_mininner, norm_r, norm_r0, nr0t, P.opt.tcg_kappa);
      if (target != rules::TCG_CONTINUE) {
        __syncthreads();
        stop = target;
        break;
      }
      const double beta = rules::tcg_beta(r_r, z_r);
      DEL[l] = -rn + beta * DEL[l];
      __syncthreads();
      proj_to(DEL, X, DEL);
      const rules::Advance av = rules::tcg_advance((double)j, maxinner, beta, r_r, e_Pd, d_Pd, al);
      z_r = av.z_r;
      e_Pd = av.e_Pd;
      d_Pd = av.d_Pd;
      if (av.stop != rules::TCG_CONTINUE) break;   // stop is RIPTRM_TCG_MAX_INNER_ITER already; j stays
    }
    __syncthreads();
    if (j >= maxinner) j = maxinner - 1;  // maxinner = 0 only (op_tcg): no iteration ran, j = -1
    jout = j;
    return stop;
  }

  // ---- Exact_RepMat, RIPTRM.py:433-444 and :599-617, in the pinned frame ---------------------------
  // The frame is Ops::qr_frame (riptrm_grassmann_ops.h, = rosenbrock.basisfun): coordinate c of a horizontal
  // U is element k k + c of Q^T U
  // selfadj_operator2matrix (utils.py:565-573) of HwCur at the prepared point (X, Y, S, X^T G_L) in the
  // frame of X: A[i][j] = <b_i, HwCur(b_j)> for i <= j, mirrored -- not the symmetric part; with want_a
  // the coordinates of c too (RIPTRM.py:438-440).  Returns false if an entry is not finite
  __device__ __forceinline__ bool repmat(riptrm_trs::Work& w, bool want_a, double& hvps) {
    const int d = w.dim, lda = w.lda;
    qr_frame(blk);
    for (int j = 0; j < d; ++j) {
      FV[l] = (l == kk + j) ? 1.0 : 0.0;
      __syncthreads();
      apply_q(FV);
      hw(FH, FV);
      hvps += 1.0;
      apply_qt(FH);
      if (act && l >= kk && l - kk <= j) {
        const double v = FH[l];
        w.A[(l - kk) * lda + j] = v;
        w.A[j * lda + (l - kk)] = v;
      }
      __syncthreads();
    }
    double bad = 0.0;
    for (int e = l; e < d * d; e += NT)
      if (!isfinite(w.A[(e / d) * lda + e % d])) bad = 1.0;
    if (want_a) {
      FH[l] = act ? C[l] : 0.0;
      __syncthreads();
      apply_qt(FH);
      if (act && l >= kk) {
        const double v = FH[l];
        w.a[l - kk] = v;
        if (!isfinite(v)) bad = 1.0;
      }
    }
    const bool ok = !(bsum(bad) > 0.0);
    __syncthreads();
    return ok;
  }
  // compute_direction's Exact_RepMat branch at the prepared point: dx into ETA; returns RIPTRM_TRS_*,
  // RIPTRM_TCG_NONFINITE (a matrix entry, the linear term or the solution) or RIPTRM_TCG_EIGFAIL
  // (eigenvalues that are not finite).  lam1 (may be null) gets TRSgep's multiplier
  __device__ __forceinline__ int trs_direction(double Delta, double& hvps, double* lam1) {
    riptrm_trs::Work w = riptrm_trs::make_work(trs_lds, k * (n - k));
    ETA[l] = 0.0;
    if (!repmat(w, true, hvps)) return RIPTRM_TCG_NONFINITE;
    const riptrm_trs::Result r = riptrm_trs::trs_solve<NT>(blk, w, Delta, P.opt.trs_tolhardcase);
    double be = 0.0, bx = 0.0;
    for (int i = l; i < w.dim; i += NT) {
      if (!isfinite(w.ev[i])) be = 1.0;
      if (!isfinite(w.x[i])) bx = 1.0;
    }
    be = bsum(be);
    bx = bsum(bx);
    if (be > 0.0) return RIPTRM_TCG_EIGFAIL;
    if (bx > 0.0) return RIPTRM_TCG_NONFINITE;
    ETA[l] = (act && l >= kk) ? w.x[l - kk] : 0.0;   // dx = sum_i coeff_i b_i = Q [0; coeff]
    __syncthreads();
    apply_q(ETA);
    if (lam1) *lam1 = r.lam1;
    return RIPTRM_TRS_BOUNDARY + r.kind;
  }
  // the smallest eigenvalue of the same matrix at the prepared point (RIPTRM.py:599-613); code = 0,
  // RIPTRM_ERR_NONFINITE or RIPTRM_ERR_EIGEN
  __device__ __forceinline__ double mineig_here(double& hvps, int& code) {
    riptrm_trs::Work w = riptrm_trs::make_work(trs_lds, k * (n - k));
    code = RIPTRM_ERR_NONE;
    if (!repmat(w, false, hvps)) {
      code = RIPTRM_ERR_NONFINITE;
      return NAN;
    }
    const double me = riptrm_trs::min_eig<NT>(blk, w);
    double be = 0.0;
    for (int i = l; i < w.dim; i += NT)
      if (!isfinite(w.ev[i])) be = 1.0;
    if (bsum(be) > 0.0 || !isfinite(me)) code = RIPTRM_ERR_EIGEN;
    return me;
  }

  // ---- utils.py:342-368 at (X, Y); xprev = this thread's element of the previous row's point -------
  __device__ __forceinline__ void evaluation(double xprev, double (&ev)[10]) {
    const double y = act ? Y[l] : 0.0;
    const double f = cost(X);
    const double gradnorm = gradlag_norm(X, y);
    const double g = act ? -X[l] - lb : 0.0;
    const double cv = act ? y * g : 0.0;
    const double sq_compl = bsum(cv * cv);
    const double nv = act ? fmax(-y, 0.0) : 0.0;
    const double sq_nonneg = bsum(nv * nv);
    const double iv = act ? fmax(g, 0.0) : 0.0;
    const double sq_ineq = bsum(iv * iv);
    const double maxvio = bmax(iv);
    const double meanvio = bsum(iv) / (double)N;
    const double maxy = bmax(act ? fabs(y) : -INFINITY);
    double manvio = 0.0;
    if (P.opt.manvio_kind == RIPTRM_MANVIO_GRASSMANN_RANK && !full_rank(X)) manvio = INFINITY;
    W1[l] = xprev;
    __syncthreads();
    const double dst = dist(W1, X);
    ev[0] = f;
    ev[1] = dst;
    ev[2] = sqrt(((((gradnorm * gradnorm + sq_compl) + sq_nonneg) + sq_ineq) + 0.0) + manvio * manvio);
    ev[3] = gradnorm;
    ev[4] = sqrt(sq_compl);
    ev[5] = sqrt(sq_nonneg);
    ev[6] = manvio;
    ev[7] = maxvio;
    ev[8] = meanvio;
    ev[9] = maxy;
  }

  __device__ __forceinline__ double now() {
    const double t = (l == 0) ? (double)wall_clock64() : -INFINITY;
    return bmax(t);
  }

  __device__ __forceinline__ void log_row(const double (&ev)[10], double outer_it, double mu, const Info& inf,
                                          bool has_info, double tcg_iters, double t_now, double t_start, double& count, double& overflow) {
    if constexpr (TRAIL) {   // the evaluated point into the record's own slot (X, Y are what evaluation() read)
      const int64_t capt = P.opt.log_capacity < P.cap ? P.opt.log_capacity : P.cap;
      if (capt > 0 && act) {
        double* Tp = P.trail + ((int64_t)b * P.cap + riptrm::log_slot((int)count, capt)) * (2 * (int64_t)N);
        Tp[l] = X[l];
        Tp[N + l] = Y[l];
      }
    }
    if (l == 0) {
      const int cnt = (int)count;
      const int64_t capl = P.opt.log_capacity < P.cap ? P.opt.log_capacity : P.cap;
      if (capl > 0) {
        if (cnt >= capl) overflow += 1.0;   // a record leaves the middle of the log (head + latest kept)
        double* L = P.log + ((int64_t)b * P.cap + riptrm::log_slot(cnt, capl)) * RIPTRM_LOG_NFIELDS;
        rules::write_log_row(L, rules::ROW_BLANK, outer_it, rules::log_time(cnt == 0, t_now, t_start, P.clock_hz), ev, mu,
                             tcg_iters, inf, has_info, EXACT);
      } else {
        overflow += 1.0;
      }
    }
    count += 1.0;
  }

  __device__ __forceinline__ double mu_at(int idx) const { return P.mu_tab[rules::tab_index(idx, P.tab_len)]; }
  __device__ __forceinline__ double load(const double* base) const { return act ? base[(int64_t)b * N + l] : 0.0; }
  __device__ __forceinline__ void store(double* base, double v) const {
    if (act) base[(int64_t)b * N + l] = v;
  }
  // the current point (X, Y) <- this thread's (x, y)
  __device__ __forceinline__ void set_point(double x, double y) {
    X[l] = x;
    Y[l] = y;
    __syncthreads();
  }

  // ---- the whole run: RIPTRM.run / outer_step / inner_run / inner_step ----------------------------
  __device__ __forceinline__ void solve() {
    double xI = load(P.in_x), yI = load(P.in_y);
    set_point(xI, yI);
    double x0 = xI, y0 = yI, xPrev = xI, xHead = xI;
    double outer_it = 0.0, mu_idx = 0.0, mu = mu_at(0), Delta = P.opt.initial_tr_radius;
    double inner_total = 0.0, tcg_total = 0.0, hvps = 0.0, log_count = 0.0, log_over = 0.0;
    double stop_code = RIPTRM_STOP_NONE, stop_rt = 0.0, residual = 0.0, last_j = 0.0, last_stop = 0.0;
    double Delta0 = 0.0, inner_it = 0.0, t_inner = 0.0;
    int err = (k * (n - k) == 0) ? RIPTRM_ERR_NO_TCG_ITER : RIPTRM_ERR_NONE;
    const double t_start = now();
    Info info{};
    bool have_info = false;
    const bool save_inner = P.opt.save_inner_iteration != 0;
    while (true) {
      double ev[10];
      // outer loop head, RIPTRM.py:931-959
      evaluation(xHead, ev);
      double tn = now();
      if (outer_it == 0.0 || !save_inner)
        log_row(ev, outer_it, mu, info, outer_it != 0.0 && have_info, last_j + 1.0, tn, t_start, log_count, log_over);
      residual = ev[2];
      xHead = act ? X[l] : 0.0;
      const double rt = (tn - t_start) / P.clock_hz;
      if (err != RIPTRM_ERR_NONE) {   // manifold.dim = 0
        stop_rt = rt;
        break;
      }
      if (isnan(ev[2])) {   // a NaN KKT residual would iterate on the NaN point: stop, keep (x, y)
        err = RIPTRM_ERR_NONFINITE;
        stop_rt = rt;
        break;
      }
      const int stop = rules::outer_stop(rt, outer_it, ev[2], P.opt);
      if (stop != RIPTRM_STOP_NONE) {
        stop_code = stop;
        stop_rt = rt;
        break;
      }
      // restart_every cycling (benchmark windows)
      if (rules::restart_due(outer_it, P.opt)) {
        set_point(xI, yI);
        mu_idx = 0.0;
        mu = mu_at(0);
        Delta = P.opt.initial_tr_radius;
      }
      outer_it += 1.0;
      x0 = act ? X[l] : 0.0;
      y0 = act ? Y[l] : 0.0;
      Delta0 = Delta;
      xPrev = x0;
      inner_it = 0.0;
      t_inner = now();
      const int ti = rules::tab_index((int)mu_idx, P.tab_len);
      const double tolL = P.tolL_tab[ti], tolC = P.tolC_tab[ti];
      while (true) {  // inner_run, RIPTRM.py:785-847
        inner_it += 1.0;
        const double DeltaStep = Delta;
        const double f_cur = prepare(mu);
        const double y = act ? Y[l] : 0.0, s = act ? S[l] : 1.0;
        // the log barrier of the iterate (RIPTRM.py:650-653) must be finite: a slack <= 0 would make
        // every later ared NaN and the inner loop endless
        const double ls = bsum(act ? log(s) : 0.0);
        const double norm_c = sqrt(dot(C, C));
        if (!isfinite(ls) || !isfinite(norm_c) || !isfinite(Delta)) {
          err = RIPTRM_ERR_NONFINITE;
          break;
        }
        int jj = 0;
        int tstop;
        if constexpr (EXACT) {
          tstop = trs_direction(Delta, hvps, nullptr);
          jj = -1;   // no tCG iterations
          if (tstop == RIPTRM_TCG_EIGFAIL) {
            err = RIPTRM_ERR_EIGEN;
            break;
          }
        } else {
          tstop = tcg(Delta, jj, hvps);
        }
        tcg_total += (double)jj + 1.0;
        last_j = jj;
        last_stop = tstop;
        const double normdx = sqrt(dot(ETA, ETA));
        if (tstop == RIPTRM_TCG_NONFINITE || !isfinite(normdx)) {
          err = RIPTRM_ERR_NONFINITE;
          break;
        }
        proj_to(W1, X, ETA);
        const double dy = act ? ((-y + mu * (1.0 / s)) - (y * W1[l]) / s) : 0.0;
        retract_to(XN, X, ETA);
        const double xN = act ? XN[l] : 0.0;
        const double yN = act ? y + dy : 0.0;
        const double sN = act ? xN + lb : 1.0;
        const double minx = bmin(act ? sN : INFINITY);
        const double miny = bmin(act ? yN : INFINITY);
        const bool xfeas = minx > 0.0 && bmin(act ? (sN > 0.0 ? 1.0 : 0.0) : 1.0) > 0.0;
        const bool yfeas = bmin(act ? (yN > 0.0 ? 1.0 : 0.0) : 1.0) > 0.0;
        const double cvv = act ? yN * sN - mu : 0.0;
        const double compl_ = sqrt(bsum(cvv * cvv));
        info = Info{1.0, inner_it, 0.0, DeltaStep, (double)tstop, normdx, minx, miny, compl_, 0.0, 0.0, 0.0, -1.0,
                    0.0, 0.0};
        have_info = true;
        bool mineig_ok = true;
        if constexpr (EXACT) {
          if (P.opt.second_order_stationarity) {   // RIPTRM.py:599-613: HwNew's matrix at (xNew, yNew)
            // recomputed at the next step where the reference reuses HwNewmatrix (:687-692): the frame is
            // deterministic, so the two are equal.  The operators move to the trial point and back
            const double xc = act ? X[l] : 0.0;
            set_point(xN, yN);
            prepare(mu);
            int code;
            const double me = mineig_here(hvps, code);
            set_point(xc, y);
            prepare(mu);
            if (code != RIPTRM_ERR_NONE) {
              err = code;
              break;
            }
            mineig_ok = me >= -rules::tol2(P.opt, ti, mu);
            info.hasmin = 1.0;
            info.mineig = me;
          }
        }
        bool converged = false;
        if (xfeas) {
          const double normgl = gradlag_norm(XN, yN);
          converged = yfeas && normgl <= tolL && compl_ <= tolC;
          if constexpr (EXACT) converged = converged && mineig_ok;
        }
        if (converged) {  // RIPTRM.py:762-766
          set_point(xN, yN);
          info.status = RIPTRM_IS_CONVERGED;
        } else if (!xfeas) {  // RIPTRM.py:769-775
          info.status = RIPTRM_IS_PRIMAL_INFEASIBLE;
          Delta = P.opt.gamma * normdx;
        } else {  // update_xy_TR_radius, RIPTRM.py:631-705
          const double fN = cost(XN);
          const double lsN = bsum(act ? log(sN) : 0.0);
          const double lb_c = f_cur - mu * ls;
          const double lb_n = fN - mu * lsN;
          double ared = lb_c - lb_n;
          hw(HD, ETA);
          hvps += 1.0;
          double pred = (0.0 - 0.5 * dot(HD, ETA)) - dot(C, ETA);
          const double red_reg = rules::red_reg(lb_c, P.opt);
          ared = ared + red_reg;
          pred = pred + red_reg;
          if (!isfinite(ared) || !isfinite(pred)) {
            err = RIPTRM_ERR_NONFINITE;
            break;
          }
          const rules::Radius ra = rules::radius_update(ared, pred, normdx, Delta, P.opt);
          info.hasratio = 1.0;
          info.ratio = ared / pred;
          info.ru = ra.ru;
          if (rules::accepted(ared, pred, P.opt)) {
            const double iright = rules::clip_right(mu, P.opt);
            const double yc = act ? rules::clip_dual(y, yN, sN, mu, iright, P.opt) : 0.0;
            const double nd = bsum((act && yc != yN) ? 1.0 : 0.0);
            set_point(xN, yc);
            info.status = RIPTRM_IS_SUCCESSFUL;
            info.dc = nd > 0.0 ? 1.0 : 0.0;
          } else {
            info.status = RIPTRM_IS_UNSUCCESSFUL;
          }
          Delta = ra.Dn;
        }
        // inner_run tail, RIPTRM.py:810-847
        inner_total += 1.0;
        tn = now();
        if (save_inner) {
          evaluation(xPrev, ev);
          log_row(ev, outer_it, mu, info, true, last_j + 1.0, tn, t_start, log_count, log_over);
        }
        xPrev = act ? X[l] : 0.0;
        bool exitflag = converged;
        const int limit = rules::inner_limit(tn, t_start, t_inner, P.clock_hz, inner_it, P.opt);
        if (limit != 0) {
          info.status = limit;
          exitflag = true;
          set_point(x0, y0);
          xPrev = x0;
          Delta = Delta0;
        }
        if (exitflag) break;
      }
      if (err != RIPTRM_ERR_NONE) {   // the reference's do_exit_on_error break: the outer step's start
        set_point(x0, y0);
        stop_rt = (now() - t_start) / P.clock_hz;
        break;
      }
      // outer_step tail, RIPTRM.py:889-896
      rules::outer_tail(mu_idx, Delta, P.opt);
      mu = mu_at((int)mu_idx);
    }
    store(P.x, act ? X[l] : 0.0);
    store(P.y, act ? Y[l] : 0.0);
    if (l == 0) {
      const double phase = err != RIPTRM_ERR_NONE ? riptrm::PH_ERROR : riptrm::PH_DONE;
      rules::write_stats(P.stats + (int64_t)b * RIPTRM_STAT_NFIELDS, true,
                         rules::Stats{outer_it, inner_total, tcg_total, hvps, stop_code, stop_rt, residual, log_count,
                                      log_over, phase, (double)err, mu, Delta, last_j, last_stop});
    }
  }

  __device__ __forceinline__ void op_hvp() {
    set_point(load(P.in_x), load(P.in_y));
    prepare(P.in_mu[b]);
    DEL[l] = load(P.in_v);
    __syncthreads();
    hw(HD, DEL);
    store(P.out_v, act ? HD[l] : 0.0);
  }

  __device__ __forceinline__ void op_tcg() {
    set_point(load(P.in_x), load(P.in_y));
    prepare(P.in_mu[b]);
    int j = 0;
    double hv = 0.0;
    const int stop = tcg(P.in_delta[b], j, hv);
    store(P.eta, act ? ETA[l] : 0.0);
    store(P.heta, act ? HETA[l] : 0.0);
    if (l == 0) {
      double* o = P.stats + (int64_t)b * RIPTRM_STAT_NFIELDS;
      o[RIPTRM_STAT_TCG_LAST_J] = j;
      o[RIPTRM_STAT_TCG_LAST_STOP] = stop;
      o[RIPTRM_STAT_PASSES] = hv;
    }
  }

  // P_x(u), the retraction of u at x, dist(x, y), matrix_rank(x) == k
  __device__ __forceinline__ void op_ops() {
    X[l] = load(P.in_x);
    ETA[l] = load(P.in_v);
    R[l] = load(P.in_y);
    __syncthreads();
    proj_to(HD, X, ETA);
    store(P.out_v, act ? HD[l] : 0.0);
    retract_to(XN, X, ETA);
    store(P.out_retr, act ? XN[l] : 0.0);
    const double d = dist(X, R);
    const bool fr = full_rank(X);
    if (l == 0) {
      P.out_dist[b] = d;
      P.out_rank[b] = fr ? 1 : 0;
    }
  }

  // riptrm_gr_exact: A, a, dx, the kind and lam1 at (x, y, mu, Delta), and the smallest eigenvalue of A
  __device__ __forceinline__ void op_exact() {
    set_point(load(P.in_x), load(P.in_y));
    prepare(P.in_mu[b]);
    const int d = k * (n - k);
    double hv = 0.0;
    riptrm_trs::Work w = riptrm_trs::make_work(trs_lds, d);
    const bool ok = repmat(w, true, hv);
    for (int e = l; e < d * d; e += NT) P.out_A[(int64_t)b * d * d + e] = w.A[(e / d) * w.lda + e % d];
    for (int e = l; e < d; e += NT) P.out_a[(int64_t)b * d + e] = w.a[e];
    __syncthreads();
    int code = RIPTRM_ERR_NONE;
    const double me = ok ? mineig_here(hv, code) : NAN;
    double lam = NAN;
    const int kind = trs_direction(P.in_delta[b], hv, &lam);
    store(P.out_v, act ? ETA[l] : 0.0);
    if (l == 0) {
      P.out_kind[b] = kind;
      P.out_lam[b] = lam;
      P.out_mineig[b] = code == RIPTRM_ERR_NONE ? me : NAN;
      P.stats[(int64_t)b * RIPTRM_STAT_NFIELDS + RIPTRM_STAT_PASSES] = hv;
    }
  }
};

template <int NT, bool TRAIL>
__global__ void __launch_bounds__(NT) k_gr(GRParams P) {
  extern __shared__ double gr_lds[];
  const int b = blockIdx.x;
  if (b >= P.batch) return;
  Eng<NT, TRAIL> e(P, b, gr_lds);
  if (P.mode == MODE_SOLVE) e.solve();
  else if (P.mode == MODE_HVP) e.op_hvp();
  else if (P.mode == MODE_TCG) e.op_tcg();
  else e.op_ops();
}

// The Exact_RepMat solve and its operator entry point: an instantiation of its own, so the tCG kernels
// above compile as they always did
template <int NT, bool TRAIL>
__global__ void __launch_bounds__(NT) k_gr_exact(GRParams P) {
  extern __shared__ double gr_lds[];
  const int b = blockIdx.x;
  if (b >= P.batch) return;
  Eng<NT, TRAIL, true> e(P, b, gr_lds);
  if (P.mode == MODE_SOLVE) e.solve();
  else e.op_exact();
}

struct Bound {
  riptrm_gr_problem prob;
  int batch = 0, cap = 0;
  Layout L{};
  char* ws = nullptr;
  double* trail = nullptr;   // riptrm_gr_bind_trail
};

}  // namespace riptrm_gr

using namespace riptrm_gr;

void riptrm_gr_release(riptrm_gr::Bound* s) { delete s; }
const riptrm_gr_problem* riptrm_gr_bound_problem(const riptrm_gr::Bound* s, int32_t* batch) {
  *batch = s->batch;
  return &s->prob;
}

static bool gr_dims_ok(int32_t n, int32_t k, int32_t batch, int32_t cap) {
  return k >= 1 && k <= KMAX && n >= k && (int64_t)n * k <= NKMAX && batch >= 1 && cap >= 0;
}

static GRParams gr_params(riptrm_ctx* c, int mode) {
  Bound* s = c->gr;
  GRParams P;
  std::memset(&P, 0, sizeof(P));
  P.n = s->prob.n;
  P.k = s->prob.k;
  P.batch = s->batch;
  P.cap = s->cap;
  P.mode = mode;
  P.clock_hz = c->clock_hz;
  P.alpha = s->prob.alpha;
  P.alpha_stride = s->prob.alpha_stride;
  P.lb = s->prob.lb;
  P.lb_stride = s->prob.lb_stride;
  P.x = (double*)(s->ws + s->L.off_x);
  P.y = (double*)(s->ws + s->L.off_y);
  P.eta = (double*)(s->ws + s->L.off_eta);
  P.heta = (double*)(s->ws + s->L.off_heta);
  P.stats = (double*)(s->ws + s->L.off_stats);
  P.log = (double*)(s->ws + s->L.off_log);
  P.opt.struct_size = (int32_t)sizeof(riptrm_options);
  P.opt.tcg_theta = 1.0;   // RIPTRM.py:330-332 defaults for the operator entry points
  P.opt.tcg_kappa = 0.1;
  P.opt.tcg_mininner = 1;
  return P;
}

static int gr_launch(riptrm_ctx* c, const GRParams& P) {
  return with_nt<gr_threads(NKMAX)>(gr_threads(P.n * P.k), [&](auto nt) -> int {
    constexpr int NT = decltype(nt)::value;
    const size_t shm = (size_t)gr_lds_doubles(NT) * sizeof(double);
    if (P.trail) hipLaunchKernelGGL((k_gr<NT, true>), dim3((unsigned)P.batch), dim3(NT), shm, c->stream, P);
    else hipLaunchKernelGGL((k_gr<NT, false>), dim3((unsigned)P.batch), dim3(NT), shm, c->stream, P);
    HIPCHK(c, hipGetLastError());
    return RIPTRM_OK;
  });
}

static bool gr_exact_ok(int n, int k) {
  const int d = k * (n - k);
  return d >= 1 && d <= EXACT_DMAX;
}

static int gr_launch_exact(riptrm_ctx* c, const GRParams& P) {   // callers checked gr_exact_ok
  return with_nt<FRAME_NT_MAX>(gr_threads(P.n * P.k), [&](auto nt) -> int {
    constexpr int NT = decltype(nt)::value;
    const size_t shm = (size_t)gr_exact_lds_doubles(NT, P.k * (P.n - P.k)) * sizeof(double);
    const void* fn = P.trail ? (const void*)k_gr_exact<NT, true> : (const void*)k_gr_exact<NT, false>;
    if (shm > 64 * 1024) HIPCHK(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
    if (P.trail) hipLaunchKernelGGL((k_gr_exact<NT, true>), dim3((unsigned)P.batch), dim3(NT), shm, c->stream, P);
    else hipLaunchKernelGGL((k_gr_exact<NT, false>), dim3((unsigned)P.batch), dim3(NT), shm, c->stream, P);
    HIPCHK(c, hipGetLastError());
    return RIPTRM_OK;
  });
}

extern "C" {

int64_t riptrm_gr_workspace_bytes(int32_t n, int32_t k, int32_t batch, int32_t cap) {
  if (!gr_dims_ok(n, k, batch, cap)) return -1;
  return make_layout(n, k, batch, cap).total;
}

int64_t riptrm_gr_workspace_offset(int32_t n, int32_t k, int32_t batch, int32_t cap, int32_t kind) {
  if (!gr_dims_ok(n, k, batch, cap)) return -1;
  const riptrm_gr::Layout L = make_layout(n, k, batch, cap);
  switch (kind) {
    case 0: return L.off_x;
    case 1: return L.off_y;
    case 2: return L.off_eta;
    case 3: return L.off_heta;
    case 4: return L.off_stats;
    case 5: return L.off_log;
    default: return -1;
  }
}

int riptrm_gr_bind(riptrm_ctx* ctx, const riptrm_gr_problem* prob, int32_t batch, void* ws, int64_t ws_bytes,
                   int32_t cap) {
  if (!ctx) return RIPTRM_E_ARG;
  if (!prob || prob->struct_size != (int32_t)sizeof(riptrm_gr_problem))
    return fail(ctx, RIPTRM_E_ARG, "gr_bind: riptrm_gr_problem.struct_size mismatch");
  if (!gr_dims_ok(prob->n, prob->k, batch, cap))
    return fail(ctx, RIPTRM_E_ARG, "gr_bind: need 1 <= k <= RIPTRM_GR_KMAX, k <= n, n k <= RIPTRM_GR_NKMAX, batch >= 1");
  if (!prob->alpha || !prob->lb || !ws || prob->alpha_stride < 0 || prob->lb_stride < 0)
    return fail(ctx, RIPTRM_E_ARG, "gr_bind: bad argument");
  if (((uintptr_t)ws % 256) != 0) return fail(ctx, RIPTRM_E_ARG, "gr_bind: workspace must be 256-byte aligned");
  const riptrm_gr::Layout L = make_layout(prob->n, prob->k, batch, cap);
  if (ws_bytes < L.total) return fail(ctx, RIPTRM_E_ARG, "gr_bind: workspace too small");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemsetAsync(ws, 0, (size_t)L.total, ctx->stream));
  if (!ctx->gr) ctx->gr = new Bound();
  ctx->gr->prob = *prob;
  ctx->gr->batch = batch;
  ctx->gr->cap = cap;
  ctx->gr->L = L;
  ctx->gr->ws = (char*)ws;
  ctx->gr->trail = nullptr;
  return RIPTRM_OK;
}

int64_t riptrm_gr_trail_bytes(int32_t n, int32_t k, int32_t batch, int32_t cap) {
  if (!gr_dims_ok(n, k, batch, cap)) return -1;
  return 8LL * batch * cap * 2 * n * k;
}

int riptrm_gr_bind_trail(riptrm_ctx* ctx, void* trail, int64_t bytes) {
  if (!ctx) return RIPTRM_E_ARG;
  if (!ctx->gr) return fail(ctx, RIPTRM_E_STATE, "gr_bind_trail: riptrm_gr_bind first");
  Bound* s = ctx->gr;
  if (trail) {
    if (((uintptr_t)trail % 8) != 0) return fail(ctx, RIPTRM_E_ARG, "gr_bind_trail: the trail must be 8-byte aligned");
    if (s->cap < 1 || bytes < riptrm_gr_trail_bytes(s->prob.n, s->prob.k, s->batch, s->cap))
      return fail(ctx, RIPTRM_E_ARG, "gr_bind_trail: trail too small (riptrm_gr_trail_bytes of the bound shape)");
  }
  s->trail = (double*)trail;
  return RIPTRM_OK;
}

int riptrm_gr_hvp(riptrm_ctx* ctx, const double* x, const double* y, const double* mu, const double* v, double* out) {
  if (!ctx) return RIPTRM_E_ARG;
  if (!ctx->gr) return fail(ctx, RIPTRM_E_STATE, "gr_hvp: riptrm_gr_bind first");
  if (!x || !y || !mu || !v || !out) return fail(ctx, RIPTRM_E_ARG, "gr_hvp: bad argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  GRParams P = gr_params(ctx, MODE_HVP);
  P.in_x = x;
  P.in_y = y;
  P.in_mu = mu;
  P.in_v = v;
  P.out_v = out;
  return gr_launch(ctx, P);
}

int riptrm_gr_tcg(riptrm_ctx* ctx, const riptrm_options* opt, const double* x, const double* y, const double* mu,
                  const double* delta) {
  if (!ctx) return RIPTRM_E_ARG;
  if (!ctx->gr) return fail(ctx, RIPTRM_E_STATE, "gr_tcg: riptrm_gr_bind first");
  if (!x || !y || !mu || !delta) return fail(ctx, RIPTRM_E_ARG, "gr_tcg: bad argument");
  if (opt && opt->struct_size != (int32_t)sizeof(riptrm_options))
    return fail(ctx, RIPTRM_E_ARG, "gr_tcg: riptrm_options.struct_size mismatch");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  GRParams P = gr_params(ctx, MODE_TCG);
  if (opt) P.opt = *opt;
  P.in_x = x;
  P.in_y = y;
  P.in_mu = mu;
  P.in_delta = delta;
  return gr_launch(ctx, P);
}

int riptrm_gr_ops(riptrm_ctx* ctx, const double* x, const double* u, const double* y, double* proj, double* retr,
                  double* dist, int32_t* fullrank) {
  if (!ctx) return RIPTRM_E_ARG;
  if (!ctx->gr) return fail(ctx, RIPTRM_E_STATE, "gr_ops: riptrm_gr_bind first");
  if (!x || !u || !y || !proj || !retr || !dist || !fullrank) return fail(ctx, RIPTRM_E_ARG, "gr_ops: bad argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  GRParams P = gr_params(ctx, MODE_OPS);
  P.in_x = x;
  P.in_v = u;
  P.in_y = y;
  P.out_v = proj;
  P.out_retr = retr;
  P.out_dist = dist;
  P.out_rank = fullrank;
  return gr_launch(ctx, P);
}

int riptrm_gr_solve(riptrm_ctx* ctx, const riptrm_options* opt, const double* x0, const double* y0,
                    const double* mu_table, const double* tolL_table, const double* tolC_table, int32_t table_len) {
  if (!ctx) return RIPTRM_E_ARG;
  if (!ctx->gr) return fail(ctx, RIPTRM_E_STATE, "gr_solve: riptrm_gr_bind first");
  if (!opt || opt->struct_size != (int32_t)sizeof(riptrm_options))
    return fail(ctx, RIPTRM_E_ARG, "gr_solve: riptrm_options.struct_size mismatch");
  if (!x0 || !y0 || !mu_table || !tolL_table || !tolC_table || table_len <= 0)
    return fail(ctx, RIPTRM_E_ARG, "gr_solve: bad argument");
  if (opt->log_capacity > ctx->gr->cap) return fail(ctx, RIPTRM_E_ARG, "gr_solve: log_capacity exceeds bound capacity");
  if (opt->trs_solver != RIPTRM_TRS_SOLVER_TCG && opt->trs_solver != RIPTRM_TRS_SOLVER_EXACT_REPMAT)
    return fail(ctx, RIPTRM_E_ARG, "gr_solve: unknown TRS_solver");
  const bool exact = opt->trs_solver == RIPTRM_TRS_SOLVER_EXACT_REPMAT;
  if (exact && !gr_exact_ok(ctx->gr->prob.n, ctx->gr->prob.k))
    return fail(ctx, RIPTRM_E_ARG, "gr_solve: Exact_RepMat needs 1 <= k (n - k) <= riptrm_gr_exact_dim_max() (" +
                                       std::to_string(EXACT_DMAX) + "), got " +
                                       std::to_string(ctx->gr->prob.k * (ctx->gr->prob.n - ctx->gr->prob.k)));
  HIPCHK(ctx, hipSetDevice(ctx->device));
  GRParams P = gr_params(ctx, MODE_SOLVE);
  P.opt = *opt;
  P.in_x = x0;
  P.in_y = y0;
  P.mu_tab = mu_table;
  P.tolL_tab = tolL_table;
  P.tolC_tab = tolC_table;
  P.tab_len = table_len;
  P.trail = ctx->gr->trail;   // only the solve logs: the operator entry points launch the plain kernel
  return exact ? gr_launch_exact(ctx, P) : gr_launch(ctx, P);
}

int32_t riptrm_gr_exact_dim_max(void) { return EXACT_DMAX; }

int64_t riptrm_gr_exact_lds_bytes(int32_t n, int32_t k) {
  if (!gr_dims_ok(n, k, 1, 0) || !gr_exact_ok(n, k)) return -1;
  return (int64_t)gr_exact_lds_doubles(gr_threads(n * k), k * (n - k)) * 8;
}

int riptrm_gr_exact(riptrm_ctx* ctx, double tolhardcase, const double* x, const double* y, const double* mu,
                    const double* delta, double* A, double* a, double* dx, int32_t* kind, double* lam1,
                    double* mineig) {
  if (!ctx) return RIPTRM_E_ARG;
  if (!ctx->gr) return fail(ctx, RIPTRM_E_STATE, "gr_exact: riptrm_gr_bind first");
  if (!x || !y || !mu || !delta || !A || !a || !dx || !kind || !lam1 || !mineig)
    return fail(ctx, RIPTRM_E_ARG, "gr_exact: bad argument");
  if (!gr_exact_ok(ctx->gr->prob.n, ctx->gr->prob.k))
    return fail(ctx, RIPTRM_E_ARG, "gr_exact: need 1 <= k (n - k) <= riptrm_gr_exact_dim_max() (" +
                                       std::to_string(EXACT_DMAX) + "), got " +
                                       std::to_string(ctx->gr->prob.k * (ctx->gr->prob.n - ctx->gr->prob.k)));
  HIPCHK(ctx, hipSetDevice(ctx->device));
  GRParams P = gr_params(ctx, MODE_EXACT);
  P.opt.trs_tolhardcase = tolhardcase;
  P.in_x = x;
  P.in_y = y;
  P.in_mu = mu;
  P.in_delta = delta;
  P.out_A = A;
  P.out_a = a;
  P.out_v = dx;
  P.out_kind = kind;
  P.out_lam = lam1;
  P.out_mineig = mineig;
  return gr_launch_exact(ctx, P);
}

int riptrm_gr_launch_info(riptrm_ctx* ctx, int32_t* lds_bytes, int32_t* threads, int32_t* wg_per_cu) {
  if (!ctx) return RIPTRM_E_ARG;
  if (!ctx->gr) return fail(ctx, RIPTRM_E_STATE, "gr_launch_info: riptrm_gr_bind first");
  if (!lds_bytes || !threads || !wg_per_cu) return fail(ctx, RIPTRM_E_ARG, "gr_launch_info: bad argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int nt = gr_threads(ctx->gr->prob.n * ctx->gr->prob.k);
  int wg = 0;
  const hipError_t e = with_nt<gr_threads(NKMAX)>(nt, [&](auto t) {
    constexpr int NT = decltype(t)::value;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&wg, (const void*)k_gr<NT, false>, NT,
                                                        (size_t)gr_lds_doubles(NT) * sizeof(double));
  });
  HIPCHK(ctx, e);
  *lds_bytes = (int32_t)(gr_lds_doubles(nt) * sizeof(double));
  *threads = nt;
  *wg_per_cu = wg;
  return RIPTRM_OK;
}

}  // extern "C"
