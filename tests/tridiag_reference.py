"""Plain-NumPy restatement of LAPACK dsytd2 (lower) -- TEST INFRASTRUCTURE ONLY: the exact reference
the distributed tridiagonal reduction (csrc/riptrm_tri.h k_tridiag_dist) is judged against.

    for i = 0 .. m - 2:   (alpha, x) = (A[i+1, i], A[i+2:, i]);  dlarfg -> v (v[0] = 1), tau, beta = e[i]
                          p = tau A[i+1:, i+1:] v;  w = p - (tau (p . v) / 2) v;  A[i+1:, i+1:] -= v w^T + w v^T
                          d[i + 1] = A[i + 1, i + 1]
Three entry points:
  * tridiag_longdouble: np.longdouble (the x86 80-bit format, eps 1.08e-19: ~3 more digits than fp64),
  * tridiag_f64: float64, one more summation order of the same algorithm (beside dsytrd),
  * tridiag_f64_tagged: float64 with the device's exchange rule emulated: st_pair overwrites the last
    mantissa bit of every exchanged p_l and A_{l, i+1} by pair_bit(pass), pass = i + 1.  The device
    forms p from untagged registers, then every workgroup reads the tagged p and the tagged column
    i + 1 (from which d[i + 1], the next column, its reflector and e[i + 1] come); the trailing
    rank-two update runs on the untagged registers with the w, v made from the tagged values.
`forward_error` is the bar's metric; `null_bar` the bar itself (4 x the worst CPU fp64 variant + 2 eps).
"""
import numpy as np


def pair_bit(p):
    """riptrm_tri.h pair_bit: the tag bit of pass p."""
    return ((p + 1) >> 1) & 1


def _tag(x, bit):
    """x (float64 array) with every last mantissa bit set to `bit` (st_pair's lo & ~1 | t)."""
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return ((u & ~np.uint64(1)) | np.uint64(bit)).view(np.float64)


def _reflector(alpha, x):
    """dlarfg without its rescaling loop (as the device): (v tail, tau, beta)."""
    s = x @ x
    if s == 0:
        return x * 0, alpha * 0, alpha
    beta = -np.copysign(np.sqrt(alpha * alpha + s), alpha)
    return x * (1 / (alpha - beta)), (beta - alpha) / beta, beta


def _reduce(A, dtype, tagged):
    A = np.array(A, dtype=dtype)
    A = np.tril(A) + np.tril(A, -1).T     # the lower triangle only (the update below keeps A bitwise symmetric)
    m = A.shape[0]
    d = np.zeros(m, dtype=dtype)
    e = np.zeros(max(m - 1, 0), dtype=dtype)
    d[0] = A[0, 0]
    col = A[1:, 0].copy()           # column i below the diagonal, as the reflector sees it
    for i in range(m - 1):
        vt, tau, beta = _reflector(col[0], col[1:])
        e[i] = beta
        v = np.concatenate([np.ones(1, dtype=dtype), vt])
        S = A[i + 1:, i + 1:]
        p = tau * (S @ v)
        c1 = S[:, 0].copy()                                   # column i + 1 before this step's update
        if tagged:
            p = _tag(p, pair_bit(i + 1))
            c1 = _tag(c1, pair_bit(i + 1))
        w = p + (-0.5 * tau * (p @ v)) * v
        d[i + 1] = c1[0] - (v[0] * w[0] + w[0] * v[0])
        col = c1[1:] - (v[1:] * w[0] + w[1:] * v[0])          # column i + 1 of the updated matrix
        U = np.outer(v[1:], w[1:])
        U += U.T                                              # v w^T + w v^T: bitwise symmetric
        S[1:, 1:] -= U
    return d, e


def tridiag_longdouble(A):
    return _reduce(A, np.longdouble, False)


def tridiag_f64(A):
    return _reduce(A, np.float64, False)


def tridiag_f64_tagged(A):
    return _reduce(A, np.float64, True)


EPS = float(np.finfo(np.float64).eps)


def forward_error(d, e, d_ref, e_ref, nrm):
    """max(|d - d_ref|, |e - e_ref|) / ||A||_2; e with its sign, except where |e_ref| <= 4 eps ||A||
    (there the reflector's sign is arbitrary: magnitudes)."""
    d_ref = np.asarray(d_ref, dtype=np.longdouble)
    e_ref = np.asarray(e_ref, dtype=np.longdouble)
    d = np.asarray(d, dtype=np.longdouble)
    e = np.asarray(e, dtype=np.longdouble)[:len(e_ref)]
    tiny = np.abs(e_ref) <= 4 * EPS * nrm
    de = np.where(tiny, np.abs(np.abs(e) - np.abs(e_ref)), np.abs(e - e_ref))
    err = max(np.max(np.abs(d - d_ref)), np.max(de) if len(de) else 0.0)
    return float(err / nrm) if nrm > 0 else float(err)


def cpu_variants(A):
    """The three CPU fp64 reductions of A: {name: (d, e)}."""
    from scipy.linalg import lapack
    _, dl, el, _, info = lapack.dsytrd(np.asarray(A, dtype=np.float64), lower=1)
    assert info == 0
    return {"dsytrd": (dl, el), "f64": tridiag_f64(A), "f64_tagged": tridiag_f64_tagged(A)}


def null_errors(A, ref=None):
    """(reference (d, e) in longdouble, ||A||_2, {variant: err against the reference})."""
    ref = tridiag_longdouble(A) if ref is None else ref
    nrm = float(np.linalg.norm(np.asarray(A, dtype=np.float64), 2))
    return ref, nrm, {k: forward_error(v[0], v[1], ref[0], ref[1], nrm) for k, v in cpu_variants(A).items()}


def null_bar(errs):
    """4 x the worst CPU fp64 variant + 2 eps (the floor for inputs every CPU variant reduces exactly)."""
    return 4.0 * max(errs.values()) + 2.0 * EPS


def assert_within_null_bar(A, d, e, what):
    """The bar on one reduced matrix (d, e from the device); returns (err, CPU errs, bar)."""
    m = A.shape[0]
    ref, nrm, errs = null_errors(A)
    err = forward_error(d, e[:m - 1], ref[0], ref[1], nrm)
    bar = null_bar(errs)
    print(f"[tridiag] {what}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) +
          f", gpu {err:.2e} (bar {bar:.2e}, gpu / null {err / max(max(errs.values()), 1e-300):.2f})", flush=True)
    assert np.isfinite(d).all() and np.isfinite(e).all(), what
    assert err <= bar, (what, err, bar, errs)
    return err, errs, bar


def assert_within_fp64_null(A, d, e, what):
    """Orders where the longdouble pass is too slow for a test (~12 s at 1000): |device - dsytrd| <=
    4 x |dsytrd - float64 restatement|, both as max over d, e relative to ||A||_2."""
    from scipy.linalg import lapack
    m = A.shape[0]
    _, dl, el, _, info = lapack.dsytrd(A, lower=1)
    assert info == 0
    dr, er = tridiag_f64(A)
    nrm = np.linalg.norm(A, 2)
    null = max(np.max(np.abs(dl - dr)), np.max(np.abs(el - er))) / nrm
    err = max(np.max(np.abs(d - dl)), np.max(np.abs(e[:m - 1] - el))) / nrm
    print(f"[tridiag] {what}: |dsytrd - f64| {null:.2e}, |gpu - dsytrd| {err:.2e}", flush=True)
    assert err <= 4.0 * null, (what, err, null)
    return err, null


# ---- the matrices ---------------------------------------------------------------------------------

def clustered(m, rs, gaps=(1e-4, 1e-8, 1e-12)):
    """Q diag(lam) Q^T: exact doubles, near-doubles at the relative gaps, a triple at the bottom."""
    lam = np.sort(rs.randn(m) * 3.0)
    lam[1] = lam[0]
    lam[2] = lam[0]
    for k, g in enumerate(gaps):
        i = 10 + 7 * k
        lam[i + 1] = lam[i] * (1.0 + g)
    lam = np.sort(lam)
    Q, _ = np.linalg.qr(rs.randn(m, m))
    A = (Q * lam) @ Q.T
    return (A + A.T) / 2


KINDS = ("random", "frame", "clustered", "diag", "tridiag", "block", "rank1")


def matrices(m, seed=None):
    """The test matrices of order m, {kind: A}, from RandomState(1000 + m): the first three drawn as
    test_sym_tridiag_matches_lapack always drew them (clustered from order 40); diag(randn); a symmetric tridiagonal;
    block-diagonal with a seam at m // 3 between two dense random blocks; I + u u^T."""
    rs = np.random.RandomState(1000 + m if seed is None else seed)
    out = {}
    M0 = rs.randn(m, m)
    out["random"] = M0 + M0.T
    D = rs.randn(m, m) / np.sqrt(m)
    out["frame"] = D + D.T + np.diag(np.where(rs.rand(m) < 0.3, 10.0 ** rs.uniform(2, 6, m), 0.0))
    if m >= 40:
        out["clustered"] = clustered(m, rs)
    out["diag"] = np.diag(rs.randn(m))
    t = rs.randn(m - 1)
    out["tridiag"] = np.diag(rs.randn(m)) + np.diag(t, 1) + np.diag(t, -1)
    s = m // 3
    B = np.zeros((m, m))
    X = rs.randn(s, s)
    Y = rs.randn(m - s, m - s)
    B[:s, :s] = X + X.T
    B[s:, s:] = Y + Y.T
    out["block"] = B
    u = rs.randn(m)
    out["rank1"] = np.eye(m) + np.outer(u, u)
    return out
