"""The exact reference of the tridiagonal reduction (tests/tridiag_reference.py) pinned on the CPU:
the longdouble reduction against the same algorithm at 50 digits (mpmath), the float64 entry against
LAPACK dsytrd, the tag emulation against its own definition."""
import numpy as np
import pytest

import tridiag_reference as R

mpmath = pytest.importorskip("mpmath")
EPS_LD = float(np.finfo(np.longdouble).eps)


def _mp_reduce(A):
    """dsytd2 (lower) at 50 digits: (d, e) as lists of mpf."""
    mp = mpmath.mp
    m = A.shape[0]
    M = [[mp.mpf(float(A[max(i, j), min(i, j)])) for j in range(m)] for i in range(m)]
    d, e = [M[0][0]], []
    for i in range(m - 1):
        alpha = M[i + 1][i]
        x = [M[j][i] for j in range(i + 2, m)]
        s = mp.fsum(t * t for t in x)
        if s == 0:
            tau, beta, v = mp.mpf(0), alpha, [mp.mpf(1)] + [mp.mpf(0)] * len(x)
        else:
            beta = -mp.sign(alpha) * mp.sqrt(alpha * alpha + s) if alpha != 0 else -mp.sqrt(s)
            tau = (beta - alpha) / beta
            v = [mp.mpf(1)] + [t / (alpha - beta) for t in x]
        e.append(beta)
        n = m - i - 1
        p = [tau * mp.fsum(M[i + 1 + r][i + 1 + c] * v[c] for c in range(n)) for r in range(n)]
        a2 = -tau * mp.fsum(p[r] * v[r] for r in range(n)) / 2
        w = [p[r] + a2 * v[r] for r in range(n)]
        for r in range(n):
            for c in range(n):
                M[i + 1 + r][i + 1 + c] -= v[r] * w[c] + w[r] * v[c]
        d.append(M[i + 1][i + 1])
    return d, e


def _err_mp(d, e, dm, em, nrm):
    """max(|d - d_mp|, |e - e_mp|) / ||A|| evaluated at 50 digits."""
    mp = mpmath.mp
    conv = _to_mpf
    worst = mp.mpf(0)
    for a, b in zip(d, dm):
        worst = max(worst, abs(conv(a) - b))
    for a, b in zip(e, em):
        worst = max(worst, abs(conv(a) - b))
    return float(worst / nrm)


def _to_mpf(x):
    """A float64 or longdouble scalar as an exact mpf (mantissa and exponent by frexp; both formats'
    mantissas fit two float64 halves)."""
    mp = mpmath.mp
    x = np.longdouble(x)
    hi = np.float64(x)
    lo = np.float64(x - np.longdouble(hi))
    return mp.mpf(float(hi)) + mp.mpf(float(lo))


@pytest.mark.parametrize("m", [5, 16, 24])
@pytest.mark.parametrize("kind", ["random", "frame", "block", "rank1", "diag", "tridiag"])
def test_longdouble_reduction_matches_50_digit_reduction(m, kind):
    """The longdouble reduction is the bar's 'exact' value: its own error against the 50-digit reduction
    must be negligible beside the fp64 variants' -- the formats' eps ratio is 2^-11; 1 / 128 leaves the
    16 x that two rounding realisations of one algorithm may differ by (the CPU variants differ from
    each other by up to 12 x), and stays far below the bar's factor 4.  Inputs that reduce exactly
    (diag, tridiag) must reduce exactly in longdouble too (floor: 2 eps_longdouble)."""
    if EPS_LD > 2e-19:
        pytest.skip("np.longdouble is not the 80-bit format here")
    mpmath.mp.dps = 50
    A = R.matrices(m)[kind]
    nrm = float(np.linalg.norm(A, 2))
    dm, em = _mp_reduce(A)
    dl, el = R.tridiag_longdouble(A)
    err_ld = _err_mp(dl, el, dm, em, nrm)
    err_64 = max(_err_mp(v[0], v[1], dm, em, nrm) for k, v in R.cpu_variants(A).items() if k != "f64_tagged")
    print(f"[tridiag ref] m={m} {kind}: longdouble {err_ld:.2e}, fp64 {err_64:.2e}")
    assert np.isfinite(np.asarray(dl, dtype=np.float64)).all() and np.isfinite(np.asarray(el, dtype=np.float64)).all()
    assert err_ld <= err_64 / 128 + 2 * EPS_LD, (err_ld, err_64)
    # forward_error's own arithmetic (longdouble) agrees with the 50-digit evaluation of the same thing
    dv, ev = R.tridiag_f64(A)
    assert abs(R.forward_error(dv, ev, dl, el, nrm) - _err_mp(dv, ev, dm, em, nrm)) <= 4 * err_ld + 2 * EPS_LD


@pytest.mark.parametrize("m", [24, 64, 150])
@pytest.mark.parametrize("kind", ["random", "frame", "block", "rank1", "diag", "tridiag"])
def test_float64_restatement_matches_dsytrd_at_the_null_bar(m, kind):
    """The float64 entry held to the bar the GPU is held to, with the other two CPU variants (dsytrd,
    the tagged restatement) as the null: err <= 4 x their worst + 2 eps against the longdouble
    reduction; on diagonal / tridiagonal input it and dsytrd return the input's diagonals bitwise."""
    A = R.matrices(m)[kind]
    ref, nrm, errs = R.null_errors(A)
    print(f"[tridiag ref] m={m} {kind}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    others = {k: v for k, v in errs.items() if k != "f64"}
    assert errs["f64"] <= R.null_bar(others), errs
    if kind in ("diag", "tridiag"):
        cv = R.cpu_variants(A)
        for k in ("dsytrd", "f64"):
            np.testing.assert_array_equal(cv[k][0], np.diag(A))
            np.testing.assert_array_equal(cv[k][1], np.diag(A, -1))


def test_tag_rule():
    """pair_bit and the tag as riptrm_tri.h st_pair defines them: bit ((pass + 1) >> 1) & 1 -- 1 on each
    parity's first pass (1, 2), alternating between the passes that share a parity; the tag overwrites
    the last mantissa bit and nothing else (0.0 with bit 1 is the denormal 2^-1074), and the tagged
    reduction of a diagonal or tridiagonal matrix moves each entry by at most one ulp."""
    assert [R.pair_bit(p) for p in range(1, 9)] == [1, 1, 0, 0, 1, 1, 0, 0]
    x = np.array([0.0, 1.0, -3.5, np.pi])
    t1, t0 = R._tag(x, 1), R._tag(x, 0)
    assert t1[0] == 2.0 ** -1074 and t0[0] == 0.0
    assert (np.abs(t1 - x) <= np.spacing(np.abs(x))).all() and (np.abs(t0 - x) <= np.spacing(np.abs(x))).all()
    assert (t1.view(np.uint64) & np.uint64(1) == 1).all() and (t0.view(np.uint64) & np.uint64(1) == 0).all()
    for kind in ("diag", "tridiag"):
        A = R.matrices(64)[kind]
        d, e = R.tridiag_f64_tagged(A)
        assert (np.abs(d - np.diag(A)) <= np.spacing(np.abs(np.diag(A)))).all()
        assert (np.abs(e - np.diag(A, -1)) <= np.spacing(np.abs(np.diag(A, -1)))).all()
        assert (d != np.diag(A)).any()     # the tag is really applied
