// riptrm_grassmann_so.hip — second-order residual of the Rosenbrock problem on Grassmann(n, k), MI355X (gfx950).
//
// src/Rosenbrock/simulator.py:60-105 logs, on every row, the smallest eigenvalue and the condition number
// of the Lagrangian's Hessian restricted to the tangent directions orthogonal to the active constraints'
// gradients.  One workgroup per point (x, y) computes them here, in its own kernel: k_gr
// (riptrm_grassmann.hip) already takes 255 VGPRs and spills.
//
// The operator.  With G_L = egrad f - Y, pymanopt's ehess -> rhess gives H(V) = P_X(T V) - V (X^T G_L).
// The cost depends on the entries of X, not on span(X), so X^T G_L is not symmetric and H is not
// self-adjoint on the horizontal space; a matrix filled from one triangle (utils.py:565-573) then depends
// on the tangent basis.  This kernel represents the symmetric part,
//   H_s(V) = P_X(T V [+ (Y o P_X V) / S]) - V sym(X^T G_L)          ([..] with barrier = 1: HwCur),
// which is basis-independent and equals H whenever X^T G_L is symmetric.
//
// Per point, d = k (n - k) <= RIPTRM_TRS_DIM_MAX:
//   1. Householder QR of X = Q [R; 0]: the k reflectors (n x k numbers) are kept and applied; frame vector
//      (a, b) is Q e_{k+a} e_b^T and the coordinates of a horizontal U are rows k.. of Q^T U (coordinate
//      c = a k + b is element k k + c of the row-major n x k layout).
//   2. M (d x d): column c = the coordinates of H_s(frame vector c), the arithmetic of k_gr's hw();
//      symmetrised as (M + M^T) / 2.
//   3. Active set {i : |-v_i - lb| < active_tol} (simulator.py:15-24); gradient i in coordinates is
//      -(Q^T E_i)[k:, :].
//   4. Independent active gradients: index order, modified Gram-Schmidt applied twice, kept iff the
//      residual norm exceeds linindtol; a dropped gradient is not used again.
//   5. Householder QR of the d x r block of kept gradients; its reflectors applied to M from both sides in
//      place: the trailing (d - r) x (d - r) block is Z^T M Z (no null basis is drawn).
//   6. All eigenvalues of that block by the LDS Jacobi of riptrm_trs.h.
//
// Workgroup: NT = 64 ceil(n k / 64) threads as in k_gr (d <= 96 and k <= 8 give n k <= 160: at most three
// waves); thread l owns element l of every n x k vector.  LDS (dynamic, so_lds_doubles): M and the
// gradient block, d (d | 1) + d d doubles (147 KiB at d = 96), five n x k vectors, the Jacobi rotation
// table and a few short vectors: 156.3 KiB at (97, 1), 158.8 KiB at (20, 8), the largest.  Nothing lives
// in HBM scratch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cstring>
#include <string>
#include "riptrm_ctx.h"
#include "riptrm_wave.h"
#include "riptrm_trs.h"
#include "riptrm_grassmann_ops.h"

namespace riptrm_gr_so {

#pragma clang fp contract(off)

using namespace riptrm_gr_dev;

constexpr int DMAX = riptrm_trs::DIM_MAX;
constexpr int NVEC = 5;

struct SOParams {
  int32_t n, k, npoints, ninst, barrier;
  const double* alpha;
  int64_t alpha_stride;
  const double* lb;
  int64_t lb_stride;
  const double* x;            // point p at x + p point_stride, n k doubles
  const double* y;
  int64_t point_stride;
  const int32_t* inst;        // point -> bound instance (NULL: p)
  const double* active_tol;
  int64_t active_tol_stride;
  double linindtol;
  const double* mu;           // per point, NULL allowed; read only with barrier
  double* out;                // npoints x RIPTRM_GR_SO_NFIELDS
};

__host__ __device__ constexpr int so_lds_doubles(int NT, int d) {
  return NVEC * NT + 3 * KK + KMAX + 2 * (NT / 64) + 3 * DMAX + d * riptrm_trs::lda_of(d) + d * d +
         riptrm_trs::ROT_FIELDS * (DMAX / 2 + 1);
}

template <int NT>
struct SO : Ops {
  const SOParams& P;
  const int d, lda;
  lf *V, *W2;                  // NT doubles each, with Ops' X, W1 and REF
  lf *M1, *MG;                 // k x k factors
  lf *GC, *UB, *WV;            // DMAX each: scratch / eigenvalues, step-5 reflector scales, a matrix-vector product
  lf *A, *B, *ROT;             // M (d x lda), the kept gradients (column j at B + j d), the Jacobi rotation table
  riptrm_trs::Blk<NT> blk;

  __device__ __forceinline__ SO(const SOParams& P_, double* lds)
      : Ops(P_.n, P_.k), P(P_), d(P_.k * (P_.n - P_.k)), lda(riptrm_trs::lda_of(P_.k * (P_.n - P_.k))),
        blk(lds + NVEC * NT + 3 * KK + KMAX) {
    lf* base = (lf*)lds;
    X = base;  V = base + NT;  W1 = base + 2 * NT;  W2 = base + 3 * NT;  REF = base + 4 * NT;
    lf* f = base + NVEC * NT;
    M1 = f;  MG = f + KK;  CW = f + 2 * KK;  BETA = f + 3 * KK;
    lf* c = f + 3 * KK + KMAX + 2 * (NT / 64);
    GC = c;  UB = c + DMAX;  WV = c + 2 * DMAX;
    A = c + 3 * DMAX;
    B = A + d * lda;
    ROT = B + d * d;
  }

  __device__ __forceinline__ double bsum(double v) { return blk.sum(v); }

  // ---- H_s from the pieces of k_gr's HwCur (Ops::Tu, xtu, rowmul) ------------------------------------
  // W2 = H_s(V) at (X, y, s); y, s = this thread's multiplier and slack.  V visible; W2 visible on return
  __device__ __forceinline__ void hs(double y, double s) {
    double pv = 0.0;
    if (P.barrier) {
      xtu(M1, X, V);
      pv = act ? V[l] - rowmul(X, M1) : 0.0;
      __syncthreads();
    }
    const double tv = Tu(V);
    W2[l] = act ? (P.barrier ? tv + (y * pv) / s : tv) : 0.0;
    __syncthreads();
    xtu(M1, X, W2);
    const double v = act ? (W2[l] - rowmul(X, M1)) - rowmul(V, MG) : 0.0;
    __syncthreads();
    W2[l] = v;
    __syncthreads();
  }

  __device__ __forceinline__ void write_out(int p, double mineig, double maxeig, double cond, double nulldim,
                                            double nactive, double nindep, double info) {
    if (l == 0) {
      double* o = P.out + (int64_t)p * RIPTRM_GR_SO_NFIELDS;
      o[RIPTRM_GR_SO_MINEIG] = mineig;
      o[RIPTRM_GR_SO_MAXEIG] = maxeig;
      o[RIPTRM_GR_SO_COND] = cond;
      o[RIPTRM_GR_SO_NULLDIM] = nulldim;
      o[RIPTRM_GR_SO_NACTIVE] = nactive;
      o[RIPTRM_GR_SO_NINDEP] = nindep;
      o[RIPTRM_GR_SO_INFO] = info;
    }
  }

  __device__ __forceinline__ void run(int p) {
    const int b = P.inst ? P.inst[p] : p;
    if (b < 0 || b >= P.ninst) {   // uniform: no bound instance to read alpha and lb from
      write_out(p, NAN, NAN, NAN, NAN, NAN, NAN, 1.0);
      return;
    }
    alpha = P.alpha[(int64_t)b * P.alpha_stride];
    lb = P.lb[(int64_t)b * P.lb_stride];
    const double tol = P.active_tol[(int64_t)p * P.active_tol_stride];
    const double x = act ? P.x[(int64_t)p * P.point_stride + l] : 0.0;
    const double y = act ? P.y[(int64_t)p * P.point_stride + l] : 0.0;
    const double s = act ? x + lb : 1.0;
    const double mu = (P.barrier && P.mu) ? P.mu[p] : 0.0;
    const bool okin = isfinite(x) && isfinite(y) && isfinite(alpha) && isfinite(lb) && isfinite(mu) && !isnan(tol);
    if (bsum(okin ? 0.0 : 1.0) > 0.0) {
      write_out(p, NAN, NAN, NAN, NAN, NAN, NAN, 1.0);
      return;
    }
    X[l] = x;
    V[l] = 0.0;
    __syncthreads();
    // sym(X^T G_L)
    const double ef = egrad_f(X);
    W1[l] = act ? ef - y : 0.0;
    __syncthreads();
    xtu(M1, X, W1);
    if (l < kk) MG[l] = 0.5 * (M1[l] + M1[(l % k) * k + l / k]);
    __syncthreads();
    qr_frame(blk);   // step 1
    // ---- step 2: M, one operator application per column --------------------------------------------
    for (int c = 0; c < d; ++c) {
      V[l] = (l == kk + c) ? 1.0 : 0.0;
      __syncthreads();
      apply_q(V);
      hs(y, s);
      apply_qt(W2);
      if (act && l >= kk) A[(l - kk) * lda + c] = W2[l];
      __syncthreads();
    }
    double bad = 0.0;
    for (int e = l; e < d * d; e += NT)
      if (!isfinite(A[(e / d) * lda + e % d])) bad = 1.0;
    if (bsum(bad) > 0.0) {
      write_out(p, NAN, NAN, NAN, NAN, NAN, NAN, 1.0);
      return;
    }
    __syncthreads();
    for (int e = l; e < d * d; e += NT) {
      const int i = e / d, j = e % d;
      if (i < j) {
        const double m = 0.5 * (A[i * lda + j] + A[j * lda + i]);
        A[i * lda + j] = m;
        A[j * lda + i] = m;
      }
    }
    __syncthreads();
    // ---- steps 3, 4: the independent active gradients, orthonormalised, into B ----------------------
    int nactive = 0, r = 0;
    for (int i = 0; i < N; ++i) {
      if (!(fabs(-X[i] - lb) < tol)) continue;   // uniform: X is visible to every thread
      nactive += 1;
      if (r >= d) continue;                      // d kept gradients span the horizontal space
      V[l] = (l == i) ? -1.0 : 0.0;
      __syncthreads();
      apply_qt(V);
      if (l < 64) {   // wave 0: lane t owns coordinates t and t + 64
        const bool h0 = l < d, h1 = l + 64 < d;
        double g0 = h0 ? V[kk + l] : 0.0, g1 = h1 ? V[kk + l + 64] : 0.0;
        for (int pass = 0; pass < 2; ++pass)
          for (int j = 0; j < r; ++j) {
            const double q0 = h0 ? B[j * d + l] : 0.0, q1 = h1 ? B[j * d + l + 64] : 0.0;
            const double dt = riptrm_wave::wave_sum(q0 * g0 + q1 * g1);
            g0 = g0 - dt * q0;
            g1 = g1 - dt * q1;
          }
        const double nrm = sqrt(riptrm_wave::wave_sum(g0 * g0 + g1 * g1));
        if (nrm > P.linindtol) {
          if (h0) B[r * d + l] = g0 / nrm;
          if (h1) B[r * d + l + 64] = g1 / nrm;
        }
        if (l == 0) GC[0] = nrm;
      }
      __syncthreads();
      const bool keep = GC[0] > P.linindtol;
      __syncthreads();
      if (keep) r += 1;
    }
    // ---- step 5: Householder QR of B (d x r); the reflectors stay in B's columns ------------------------
    for (int j = 0; j < r; ++j) {
      lf* u = B + j * d;
      double t = 0.0;
      for (int e = j + l; e < d; e += NT) t = t + u[e] * u[e];
      const double nrm = sqrt(bsum(t));
      const double bjj = u[j];
      const double ah = bjj >= 0.0 ? -nrm : nrm;
      const double beta = nrm > 0.0 ? 1.0 / (nrm * (nrm + fabs(bjj))) : 0.0;
      __syncthreads();
      if (l == 0) {
        u[j] = bjj - ah;
        UB[j] = beta;
      }
      __syncthreads();
      for (int c = j + 1 + l; c < r; c += NT) {   // one thread per later column
        lf* w = B + c * d;
        double acc = 0.0;
        for (int e = j; e < d; ++e) acc = acc + u[e] * w[e];
        acc = beta * acc;
        for (int e = j; e < d; ++e) w[e] = w[e] - acc * u[e];
      }
      __syncthreads();
    }
    // M <- H_j M H_j, j = 0 .. r - 1: the trailing block becomes Z^T M Z
    for (int j = 0; j < r; ++j) {
      const lf* u = B + j * d;
      const double beta = UB[j];
      const int h = d - j;
      for (int t = l; t < d; t += NT) {   // u^T M, one thread per column
        double acc = 0.0;
        for (int i = j; i < d; ++i) acc = acc + u[i] * A[i * lda + t];
        WV[t] = acc;
      }
      __syncthreads();
      for (int e = l; e < h * d; e += NT) {
        const int i = j + e / d, t = e % d;
        A[i * lda + t] = A[i * lda + t] - (beta * u[i]) * WV[t];
      }
      __syncthreads();
      for (int i = l; i < d; i += NT) {   // M u, one thread per row
        double acc = 0.0;
        for (int t = j; t < d; ++t) acc = acc + A[i * lda + t] * u[t];
        WV[i] = acc;
      }
      __syncthreads();
      for (int e = l; e < d * h; e += NT) {
        const int i = e / h, t = j + e % h;
        A[i * lda + t] = A[i * lda + t] - (beta * WV[i]) * u[t];
      }
      __syncthreads();
    }
    // ---- step 6: the eigenvalues of the trailing block ------------------------------------------------
    const int m = d - r;
    if (m == 0) {   // simulator.py:91-93: 0 and None
      write_out(p, 0.0, NAN, NAN, 0.0, (double)nactive, (double)r, 0.0);
      return;
    }
    lf* T = A + r * lda + r;
    for (int e = l; e < m * m; e += NT) {
      const int i = e / m, j = e % m;
      if (i < j) {
        const double v = 0.5 * (T[i * lda + j] + T[j * lda + i]);
        T[i * lda + j] = v;
        T[j * lda + i] = v;
      }
    }
    __syncthreads();
    riptrm_trs::Work w;
    w.A = T;
    w.V = nullptr;
    w.a = w.x = w.p = w.r = w.q = w.cgx = w.g = nullptr;
    w.ev = GC;
    w.rot = ROT;
    w.dim = m;
    w.lda = lda;
    riptrm_trs::jacobi<NT>(blk, w, false);
    double lo = INFINITY, hi = -INFINITY, nf = 0.0;
    for (int i = l; i < m; i += NT) {
      const double e = GC[i];
      if (!isfinite(e)) nf = 1.0;
      lo = fmin(lo, e);
      hi = fmax(hi, e);
    }
    lo = blk.min(lo);
    hi = blk.max(hi);
    if (bsum(nf) > 0.0) {
      write_out(p, NAN, NAN, NAN, NAN, NAN, NAN, 1.0);
      return;
    }
    write_out(p, lo, hi, hi / lo, (double)m, (double)nactive, (double)r, 0.0);
  }
};

template <int NT>
__global__ void __launch_bounds__(NT) k_gr_so(SOParams P) {
  extern __shared__ double so_lds[];
  const int p = blockIdx.x;
  if (p >= P.npoints) return;
  SO<NT> e(P, so_lds);
  e.run(p);
}

}  // namespace riptrm_gr_so

using namespace riptrm_gr_so;

extern "C" {

int riptrm_gr_second_order(riptrm_ctx* ctx, const double* x, const double* y, int64_t point_stride, const int32_t* inst,
                           int32_t npoints, const double* active_tol, int64_t active_tol_stride, double linindtol,
                           int32_t barrier, const double* mu, double* out) {
  if (!ctx) return RIPTRM_E_ARG;
  if (!ctx->gr) return fail(ctx, RIPTRM_E_STATE, "gr_second_order: riptrm_gr_bind first");
  int32_t batch = 0;
  const riptrm_gr_problem* prob = riptrm_gr_bound_problem(ctx->gr, &batch);
  const int n = prob->n, k = prob->k, N = n * k, d = k * (n - k);
  if (d < 1 || d > DMAX)
    return fail(ctx, RIPTRM_E_ARG, "gr_second_order: need 1 <= k (n - k) <= RIPTRM_TRS_DIM_MAX (" + std::to_string(DMAX) +
                                       "), got " + std::to_string(d));
  if (!x || !y || !active_tol || !out || npoints < 0 || point_stride < N)
    return fail(ctx, RIPTRM_E_ARG, "gr_second_order: bad argument");
  if ((active_tol_stride != 0 && active_tol_stride != 1) || (barrier != 0 && barrier != 1) || !(linindtol >= 0.0))
    return fail(ctx, RIPTRM_E_ARG, "gr_second_order: active_tol_stride and barrier are 0 or 1, linindtol >= 0");
  if (!inst && npoints > batch)
    return fail(ctx, RIPTRM_E_ARG, "gr_second_order: more points than bound instances need an instance map");
  if (npoints == 0) return RIPTRM_OK;
  const int nt = gr_threads(N);
  const size_t shm = (size_t)so_lds_doubles(nt, d) * sizeof(double);
  if (nt > FRAME_NT_MAX || shm > (size_t)LDS_LIMIT)
    return fail(ctx, RIPTRM_E_ARG, "gr_second_order: the shape does not fit one workgroup's LDS");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  SOParams P;
  std::memset(&P, 0, sizeof(P));
  P.n = n;
  P.k = k;
  P.npoints = npoints;
  P.ninst = batch;
  P.barrier = barrier;
  P.alpha = prob->alpha;
  P.alpha_stride = prob->alpha_stride;
  P.lb = prob->lb;
  P.lb_stride = prob->lb_stride;
  P.x = x;
  P.y = y;
  P.point_stride = point_stride;
  P.inst = inst;
  P.active_tol = active_tol;
  P.active_tol_stride = active_tol_stride;
  P.linindtol = linindtol;
  P.mu = mu;
  P.out = out;
  return with_nt<FRAME_NT_MAX>(nt, [&](auto t) -> int {
    constexpr int NT = decltype(t)::value;
    if (shm > 64 * 1024)
      HIPCHK(ctx, hipFuncSetAttribute((const void*)k_gr_so<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
    hipLaunchKernelGGL(k_gr_so<NT>, dim3((unsigned)P.npoints), dim3(NT), shm, ctx->stream, P);
    HIPCHK(ctx, hipGetLastError());
    return RIPTRM_OK;
  });
}

}  // extern "C"
