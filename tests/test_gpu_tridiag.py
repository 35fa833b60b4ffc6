"""The distributed tridiagonal reduction (riptrm_sym_tridiag, csrc/riptrm_tri.h k_tridiag_dist) against
an exact reference of the same algorithm, and its launch / ABI edges.

Bar (null-calibrated, DESIGN §3's way): err(X) = max(|d_X - d_ref|, |e_X - e_ref|) / ||A||_2 against the
np.longdouble restatement of dsytd2 (tests/tridiag_reference.py, pinned on the CPU by
tests/test_tridiag_reference.py); e with its sign except where |e_ref| <= 4 eps ||A||.  The null is the
worst of three CPU fp64 reductions of the same matrix -- LAPACK dsytrd, the float64 restatement, the
float64 restatement with the exchange's mantissa tag bit emulated -- and the GPU passes at
err <= 4 x null + 2 eps.  (The clustered matrices have a triple eigenvalue: their T must split, past
the split d and e are not determined by A, every CPU variant is O(1) from the reference there and the
bar says so; their check is the spectrum.)"""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import tridiag_reference as R

ORDERS = [64, 150, 256, 257, 512, 513]   # EL = 4 | 8 | 16 changes at 256 / 257 and 512 / 513


def _reduce_gpu(mats):
    import trs
    A = torch.tensor(np.stack(mats), dtype=torch.float64, device="cuda")
    d, e, info = trs.sym_tridiag(A)
    torch.cuda.synchronize()
    return d.cpu().numpy(), e.cpu().numpy(), info.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _gpu_batch(m):
    """Every kind of order m reduced in one batch (several matrices per cooperative launch): once."""
    mats = R.matrices(m)
    d, e, info = _reduce_gpu([mats[k] for k in R.KINDS])
    return mats, {k: (d[i], e[i], int(info[i])) for i, k in enumerate(R.KINDS)}


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("m", ORDERS)
def test_sym_tridiag_forward_error(m, kind):
    """d, e against the longdouble reduction at the null-calibrated bar, every kind at every order where
    the register layout changes.  Diagonal and tridiagonal input take the tau = 0 branch at every column
    (block-diagonal at the seam): there the published p = 0 carries the tag bit (the denormal 2^-1074) and
    d, |e| must come back as the input's diagonals within one ulp per entry (the tag's own reach)."""
    import scipy.linalg as sl
    mats, out = _gpu_batch(m)
    A = mats[kind]
    d, e, info = out[kind]
    assert info == 0
    R.assert_within_null_bar(A, d, e, f"m={m} {kind}")
    nrm = np.linalg.norm(A, 2)
    wt = sl.eigvalsh_tridiagonal(d, e[:m - 1])
    werr = np.max(np.abs(wt - np.linalg.eigvalsh(A)))
    assert werr <= 1e-13 * nrm * max(1.0, np.sqrt(m) / 4), (kind, werr / nrm)
    if kind in ("diag", "tridiag"):
        d0, e0 = np.diag(A), np.diag(A, -1)
        assert (np.abs(d - d0) <= np.spacing(np.abs(d0))).all(), np.max(np.abs(d - d0))
        assert (np.abs(np.abs(e[:m - 1]) - np.abs(e0)) <= np.spacing(np.abs(e0))).all()
        # every sum on these inputs is exact, so the tag is all that moves an entry: the emulation's values
        dt, et = R.tridiag_f64_tagged(A)
        np.testing.assert_array_equal(d, dt)
        np.testing.assert_array_equal(e[:m - 1], et)


def test_sym_tridiag_order_1024():
    """TRI_MAX: every lane and register holds a column (j0 + EL == m), 64 workgroups.  (No longdouble pass
    here: ~12 s on the CPU.)  |GPU - dsytrd| <= 4 x |dsytrd - float64 restatement| on the random matrix
    -- the distance between two CPU reductions as the null -- and T's spectrum.  (Order 1000 the same way
    in test_gpu_trs.py::test_sym_tridiag_matches_lapack.)"""
    import scipy.linalg as sl
    m = 1024
    rs = np.random.RandomState(1000 + m)
    M0 = rs.randn(m, m)
    A = M0 + M0.T
    d, e, info = _reduce_gpu([A])
    assert (info == 0).all()
    R.assert_within_fp64_null(A, d[0], e[0], f"m={m} random")
    nrm = np.linalg.norm(A, 2)
    werr = np.max(np.abs(sl.eigvalsh_tridiagonal(d[0], e[0][:m - 1]) - np.linalg.eigvalsh(A)))
    assert werr <= 1e-13 * nrm * max(1.0, np.sqrt(m) / 4), werr / nrm


@pytest.mark.parametrize("m,batch", [(64, 1100), (200, 300)])
def test_sym_tridiag_more_matrices_than_one_launch(m, batch):
    """More matrices than one cooperative launch holds (at most 4 workgroups of 512 threads per CU on 256
    CUs, G = 1 workgroup per matrix at order 64 and 4 at 200): the host loop re-zeroes the granule grid
    and launches again with k0 > 0.  Eight distinct matrices tiled: d, e bitwise periodic with period 8
    and bitwise those of the eight reduced as one batch."""
    mats = R.matrices(m)
    rs = np.random.RandomState(m)
    eight = [mats[k] for k in R.KINDS] + [rs.randn(m, m)]
    eight[-1] = eight[-1] + eight[-1].T
    d8, e8, i8 = _reduce_gpu(eight)
    assert (i8 == 0).all()
    d, e, info = _reduce_gpu([eight[k % 8] for k in range(batch)])
    assert (info == 0).all(), np.nonzero(info)[0][:10]
    for k in range(batch):
        assert np.array_equal(d[k], d8[k % 8]) and np.array_equal(e[k], e8[k % 8]), k


def _raw_call(dim, batch, A, lda, a_stride, d, e, de_stride, info):
    import trs
    ctx = trs._context(A.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    ctx.check(ctx.lib.riptrm_sym_tridiag(ctx.h, dim, batch, p(A), lda, a_stride, p(d), p(e), de_stride, p(info)),
              "riptrm_sym_tridiag")
    torch.cuda.synchronize()


SENTINEL = 1.2345e300   # finite: a kernel that read it would carry it into d, e


@pytest.mark.parametrize("m", [64, 257])
def test_sym_tridiag_strides_and_read_only_input(m):
    """The ABI of include/riptrm.h as the packed Python wrapper never calls it: lda = dim + 3,
    a_stride = dim lda + 5, de_stride = dim + 7, every padding double a sentinel.  The results are
    bitwise the packed call's; the padding of d, e (e's entry m - 1 included: e has m - 1 entries) and
    all of A are unchanged."""
    mats = R.matrices(m)
    three = [mats["random"], mats["frame"], mats["block"]]
    dp, ep, ip = _reduce_gpu(three)
    B, lda, des = 3, m + 3, m + 7
    a_stride = m * lda + 5
    Ah = np.full(B * a_stride, SENTINEL)
    for k, M in enumerate(three):
        Ah[k * a_stride:k * a_stride + m * lda].reshape(m, lda)[:, :m] = M
    A = torch.tensor(Ah, device="cuda")
    d = torch.full((B * des,), SENTINEL, dtype=torch.float64, device="cuda")
    e = torch.full((B * des,), SENTINEL, dtype=torch.float64, device="cuda")
    info = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    _raw_call(m, B, A, lda, a_stride, d, e, des, info)
    assert (info.cpu().numpy() == 0).all()
    np.testing.assert_array_equal(A.cpu().numpy(), Ah)        # A is not written
    dh, eh = d.cpu().numpy().reshape(B, des), e.cpu().numpy().reshape(B, des)
    np.testing.assert_array_equal(dh[:, :m], dp)
    np.testing.assert_array_equal(eh[:, :m - 1], ep[:, :m - 1])
    assert (dh[:, m:] == SENTINEL).all() and (eh[:, m - 1:] == SENTINEL).all()


@pytest.mark.parametrize("m", [64, 257])
def test_sym_tridiag_reads_the_lower_triangle_only(m):
    """tril(A) with finite garbage above the diagonal gives bitwise the symmetric input's d, e."""
    A = R.matrices(m)["random"]
    G = np.tril(A) + np.triu(np.random.RandomState(m).randn(m, m) * 1e3, 1)
    d, e, info = _reduce_gpu([A, G])
    assert (info == 0).all()
    np.testing.assert_array_equal(d[1], d[0])
    np.testing.assert_array_equal(e[1], e[0])


@pytest.mark.parametrize("dim,lda_off,des_off", [(63, 0, 0), (1025, 0, 0), (64, -1, 0), (64, 0, -1)])
def test_sym_tridiag_argument_checks(dim, lda_off, des_off):
    """dim outside 64 .. 1024, lda < dim and de_stride < dim are refused before anything is launched,
    with a message that names the limits."""
    lda, des = dim + lda_off, dim + des_off
    A = torch.zeros(dim * dim, dtype=torch.float64, device="cuda")
    d = torch.zeros(dim, dtype=torch.float64, device="cuda")
    e = torch.zeros(dim, dtype=torch.float64, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError) as ei:
        _raw_call(dim, 1, A, lda, dim * lda, d, e, des, info)
    msg = str(ei.value)
    for limit in ("64 <= dim <= 1024", "lda >= dim", "a_stride >= dim * lda", "de_stride >= dim"):
        assert limit in msg, msg
