// riptrm_grassmann_ops.h — device helpers, and the host's workgroup-size dispatch, shared by the
// Grassmann(n, k) kernels: k_gr / k_gr_exact (riptrm_grassmann.hip) and k_gr_so (riptrm_grassmann_so.hip).
//
// One workgroup of gr_threads(n k) threads works on one point; thread l owns element l = (l / k, l % k)
// of every row-major n x k vector in LDS.  Ops holds that indexing, the pieces of HwCur both kernels
// use (the tridiagonal Hessian of f, the k x k products) and THE pinned tangent frame: the Exact_RepMat
// matrix (k_gr_exact), the second-order residual (k_gr_so) and rosenbrock.basisfun are statements in one
// basis only because this is the frame's single definition on the device.  The operator is not
// self-adjoint, so a change of sign convention or summation order here changes the
// reference's matrix: rosenbrock.basisfun has to follow it.
//
// Ops is not a template, so the structs deriving from it find its names without this->; qr_frame alone
// needs the block reducer (riptrm_trs::Blk<NT>) and takes it as an argument.  The derived struct's
// constructor points X, W1, REF, CW and BETA into its own LDS layout and sets alpha and lb.
#pragma once
#include <type_traits>
#include "../../include/riptrm.h"
#include "riptrm_trs.h"

namespace riptrm_gr_dev {

#pragma clang fp contract(off)

constexpr int KMAX = RIPTRM_GR_KMAX;
constexpr int KK = KMAX * KMAX;
constexpr int LDS_LIMIT = 160 * 1024;   // one workgroup's LDS on a compute unit

typedef riptrm_trs::lds_f64 lf;

__host__ __device__ constexpr int gr_threads(int N) { return (N + 63) / 64 * 64; }
// The kernels that hold a d x d matrix in the frame (k_gr_exact, k_gr_so): d <= RIPTRM_TRS_DIM_MAX and
// k <= KMAX give n k = d + k^2 <= 160, three waves at most
constexpr int FRAME_NT_MAX = 192;
static_assert(riptrm_trs::DIM_MAX + KK <= FRAME_NT_MAX, "n k = d + k^2 must fit FRAME_NT_MAX threads");

// The workgroup size is a template parameter (riptrm_trs::Blk): f(std::integral_constant<int, NT>) for
// NT = nt, a multiple of 64 up to NT_MAX (the callers checked the shape).  Written out in ascending order:
// the kernels are emitted in the order f is instantiated
template <int NT_MAX, class F>
inline auto with_nt(int nt, F&& f) {
  static_assert(NT_MAX == FRAME_NT_MAX || NT_MAX == gr_threads(RIPTRM_GR_NKMAX), "the two widths in use");
  using std::integral_constant;
  if (nt == 64) return f(integral_constant<int, 64>{});
  if (nt == 128) return f(integral_constant<int, 128>{});
  if constexpr (NT_MAX == FRAME_NT_MAX) {
    return f(integral_constant<int, 192>{});
  } else {
    if (nt == 192) return f(integral_constant<int, 192>{});
    if (nt == 256) return f(integral_constant<int, 256>{});
    if (nt == 320) return f(integral_constant<int, 320>{});
    if (nt == 384) return f(integral_constant<int, 384>{});
    if (nt == 448) return f(integral_constant<int, 448>{});
    return f(integral_constant<int, 512>{});
  }
}

struct Ops {
  const int l, n, k, N, kk;
  const int li, lj;
  const bool act;
  double alpha, lb;
  lf *X, *W1, *REF;   // NT doubles each: the point, a scratch vector, column j = reflector j of X's QR
  lf *CW, *BETA;      // k column dots, k reflector scales

  __device__ __forceinline__ Ops(int n_, int k_)
      : l((int)threadIdx.x), n(n_), k(k_), N(n_ * k_), kk(k_ * k_), li((int)threadIdx.x / k_),
        lj((int)threadIdx.x % k_), act((int)threadIdx.x < n_ * k_), alpha(0.0), lb(0.0) {}

  // ---- the tridiagonal Hessian of f: (T u)_l, neighbours through LDS (u visible to every thread) ----
  __device__ __forceinline__ double Tu(const lf* U) {
    if (!act) return 0.0;
    const double u = U[l];
    double acc = 0.0;
    if (l < N - 1) {
      const double d = U[l + 1] - u;
      acc = -2.0 * alpha * d + 2.0 * u;
    }
    if (l > 0) {
      const double dm = u - U[l - 1];
      acc = acc + 2.0 * alpha * dm;
    }
    return acc;
  }
  __device__ __forceinline__ double egrad_f(const lf* Xp) { return Tu(Xp) - ((act && l < N - 1) ? 2.0 : 0.0); }

  // ---- k x k products: M = A^T B, one thread per entry, rows in order.  A, B visible; M visible on return ----
  __device__ __forceinline__ void xtu(lf* M, const lf* A, const lf* B) {
    if (l < kk) {
      const int a = l / k, c = l % k;
      double acc = 0.0;
      for (int i = 0; i < n; ++i) acc = acc + A[i * k + a] * B[i * k + c];
      M[l] = acc;
    }
    __syncthreads();
  }
  // this thread's element of A M (A n x k, M k x k)
  __device__ __forceinline__ double rowmul(const lf* A, const lf* M) {
    double acc = 0.0;
    if (act)
      for (int c = 0; c < k; ++c) acc = acc + A[li * k + c] * M[c * k + lj];
    return acc;
  }

  // ---- the pinned frame (rosenbrock.basisfun): Householder QR X = Q [R; 0], the k reflectors into REF /
  // BETA; frame vector a k + b = Q e_{k+a} e_b^T and the coordinates of a horizontal U are rows k.. of
  // Q^T U, coordinate c = element k k + c of the row-major layout.  X visible
  template <class Blk>
  __device__ __forceinline__ void qr_frame(Blk& blk) {
    W1[l] = act ? X[l] : 0.0;
    REF[l] = 0.0;
    __syncthreads();
    for (int j = 0; j < k; ++j) {
      const double w = W1[l];
      const double nrm = sqrt(blk.sum((act && lj == j && li >= j) ? w * w : 0.0));
      const double xjj = W1[j * k + j];
      const double ah = xjj >= 0.0 ? -nrm : nrm;
      const double beta = nrm > 0.0 ? 1.0 / (nrm * (nrm + fabs(xjj))) : 0.0;   // 2 / (v^T v)
      __syncthreads();
      if (act && lj == j && li >= j) REF[l] = (li == j) ? xjj - ah : w;
      if (l == 0) BETA[j] = beta;
      __syncthreads();
      if (l < k) {
        double acc = 0.0;
        if (l > j)
          for (int i = j; i < n; ++i) acc = acc + REF[i * k + j] * W1[i * k + l];
        CW[l] = acc;
      }
      __syncthreads();
      if (act && lj > j && li >= j) W1[l] = w - (beta * CW[lj]) * REF[li * k + j];
      __syncthreads();
    }
  }
  // U <- H_j U for reflector j (U n x k, in place).  U visible before and after
  __device__ __forceinline__ void reflect(lf* U, int j) {
    if (l < k) {
      double acc = 0.0;
      for (int i = j; i < n; ++i) acc = acc + REF[i * k + j] * U[i * k + l];
      CW[l] = acc;
    }
    __syncthreads();
    if (act && li >= j) U[l] = U[l] - (BETA[j] * CW[lj]) * REF[li * k + j];
    __syncthreads();
  }
  __device__ __forceinline__ void apply_qt(lf* U) {   // U <- Q^T U
    for (int j = 0; j < k; ++j) reflect(U, j);
  }
  __device__ __forceinline__ void apply_q(lf* U) {    // U <- Q U
    for (int j = k - 1; j >= 0; --j) reflect(U, j);
  }
};

}  // namespace riptrm_gr_dev
