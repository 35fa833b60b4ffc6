"""GPU parity of the Exact_RepMat subproblem solver (csrc/riptrm_trs.hip) against the reference's
own formulation restated in oracle/trs_oracle.py::trs_gep (RIPTRM.py:218-299: the 2n x 2n pencil
(MM0, -MM1) + SciPy CG interior candidate + hard-case refinement).

Bar: same `type`; x within 1e-8 relative (the pencil's QZ and the device's Jacobi + secular Newton
agree to that level: tests/test_trs_oracle.py pins the same bound between the two CPU forms).  The
interior candidate is a CG iterate stopped at rtol 1e-5 whose value moves with the mat-vec summation
order (up to ~1e-5 relative at dim 77, cond ~1e3): there both must pass the reference's acceptance
test ||A p1 + a|| / ||a|| < 1e-5 (RIPTRM.py:246), agree to 1e-4 and in model value to 1e-8;
lam1 within 1e-8; the smallest eigenvalue (RIPTRM.py:611) within 1e-11 relative to ||A||.  Hard
case: the sign of the q_min component is arbitrary in both, so the model values are compared."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import trs_oracle as T


def _obj(A, a, x):
    return 0.5 * x @ A @ x + a @ x


def _cases(seed, count, dims):
    rs = np.random.RandomState(seed)
    out = []
    for t in range(count):
        n = dims[t % len(dims)]
        M = rs.randn(n, n)
        kind = t % 4
        if kind == 0:                 # positive definite, small radius -> boundary
            A = M @ M.T + 0.1 * np.eye(n)
            Del = 10 ** rs.uniform(-2, -0.5)
        elif kind == 1:               # positive definite, large radius -> interior
            A = M @ M.T + np.eye(n)
            Del = 100.0
        else:                         # indefinite -> boundary
            A = M + M.T
            Del = 10 ** rs.uniform(-2, 1)
        out.append((A, rs.randn(n), Del))
    return out


def _solve(cases, tol=1e-8):
    from trs import trs_gep_batched
    dim = cases[0][0].shape[0]
    A = torch.tensor(np.stack([c[0] for c in cases]), device="cuda")
    a = torch.tensor(np.stack([c[1] for c in cases]), device="cuda")
    D = torch.tensor([c[2] for c in cases], dtype=torch.float64, device="cuda")
    x, lam1, kind, mineig = trs_gep_batched(A, a, D, tol)
    torch.cuda.synchronize()
    return x.cpu().numpy(), lam1.cpu().numpy(), kind.cpu().numpy(), mineig.cpu().numpy()


@pytest.mark.parametrize("dim", [1, 2, 5, 17, 40, 49, 64, 77, 96])
def test_trs_gep_matches_pencil_oracle(dim):
    from trs import KIND_NAMES
    cases = _cases(dim, 12, [dim])
    x, lam1, kind, mineig = _solve(cases)
    for b, (A, a, Del) in enumerate(cases):
        xr, lr, kr = T.trs_gep(A, a, Del, 1e-8)
        assert KIND_NAMES[int(kind[b])] == kr, (b, KIND_NAMES[int(kind[b])], kr)
        if kr == "interior":   # both are CG iterates meeting the reference's own acceptance test
            assert np.linalg.norm(x[b] - xr) <= 1e-4 * np.linalg.norm(xr), b
            assert np.linalg.norm(A @ x[b] + a) / np.linalg.norm(a) < 1e-5, b
            assert abs(_obj(A, a, x[b]) - _obj(A, a, xr)) <= 1e-8 * abs(_obj(A, a, xr)), b
        else:
            assert np.linalg.norm(x[b] - xr) <= 1e-8 * max(np.linalg.norm(xr), 1e-300), (b, kr)
        assert abs(lam1[b] - lr) <= 1e-8 * max(1.0, abs(lr)), (b, lam1[b], lr)
        ev = np.linalg.eigvalsh(A)[0]
        assert abs(mineig[b] - ev) <= 1e-11 * max(1.0, np.abs(A).max() * dim), (b, mineig[b], ev)


def test_trs_gep_hard_case():
    rs = np.random.RandomState(7)
    cases = []
    for _ in range(6):
        n = 9
        Q, _ = np.linalg.qr(rs.randn(n, n))
        lam = np.sort(rs.randn(n))
        lam[0] = -3.0
        A = Q @ np.diag(lam) @ Q.T
        g = rs.randn(n)
        g[0] = 0.0
        cases.append((A, Q @ g, 5.0))
    x, lam1, kind, _ = _solve(cases)
    for b, (A, a, Del) in enumerate(cases):
        xr, lr, kr = T.trs_gep(A, a, Del, 1e-8)
        assert kr == "hardcase_1" and int(kind[b]) == 8
        assert np.isclose(lam1[b], lr, rtol=1e-8)
        assert np.isclose(np.linalg.norm(x[b]), Del, rtol=1e-12)
        assert np.isclose(_obj(A, a, x[b]), _obj(A, a, xr), rtol=1e-10)


def test_trs_gep_reference_signature():
    from trs import TRSgep
    A, a, Del = _cases(3, 1, [12])[0]
    x, lam1, kind = TRSgep(A, a, np.eye(12), Del, 1e-8)
    xr, lr, kr = T.trs_gep(A, a, Del, 1e-8)
    assert kind == kr and np.allclose(x, xr, rtol=1e-8, atol=1e-12)
    with pytest.raises(NotImplementedError):
        TRSgep(A, a, 2 * np.eye(12), Del, 1e-8)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("dim", [97, 149, 150, 200, 256, 257, 392, 512, 513, 999, 1024, 1025])
def test_trs_gep_above_lds_size_matches_oracle(dim):
    """dim > RIPTRM_TRS_DIM_MAX: the HBM service (csrc/riptrm_trs_big.hip) against the reference's
    pencil (dims up to 392) and, from 512 up, the eigh formulation trs_oracle.trs_eigh (the pencil's QZ on
    1998 x 1998 takes ~90 s per case on the CPU; measured on these cases while choosing the bar:
    trs_eigh vs pencil 5e-14 in x, 6e-14 in lam1 at 999, <= 2e-14 at 97 / 200).  256 / 257 and 512 / 513
    are the orders where the tridiagonal path's register layout changes (riptrm_tri.h tri_el), 1024 /
    1025 the two sides of RIPTRM_TRS_TRI_MAX (1024: every lane and register of the layout full; 1025:
    rocSOLVER).  Orders <= 149 take
    the hand-written eigensolver (riptrm_eig.h) and SciPy's CG in its eigen-coordinates (k_cg_diag);
    orders 150 .. 1024 (RIPTRM_TRS_TRI_MIN..) the distributed tridiagonalisation and the subproblem in
    T's coordinates (riptrm_tri.h: Sturm bisection, secular Newton on partitioned LDL^T solves, the CG
    on T); 149 / 150 are the two sides of that boundary.  Same bar as the LDS path."""
    from trs import KIND_NAMES
    cases = _cases(dim, 4, [dim])
    if dim >= 999:
        cases = [cases[0], cases[2], cases[1]]
    x, lam1, kind, mineig = _solve(cases)
    for b, (A, a, Del) in enumerate(cases):
        xr, lr, kr = (T.trs_eigh if dim >= 512 else T.trs_gep)(A, a, Del, 1e-8)
        print(f"[trs] dim {dim} case {b} {kr}", flush=True)
        assert KIND_NAMES[int(kind[b])] == kr, (b, KIND_NAMES[int(kind[b])], kr)
        if kr == "interior":
            assert np.linalg.norm(x[b] - xr) <= 1e-4 * np.linalg.norm(xr), b
            assert np.linalg.norm(A @ x[b] + a) / np.linalg.norm(a) < 1e-5, b
            assert abs(_obj(A, a, x[b]) - _obj(A, a, xr)) <= 1e-8 * abs(_obj(A, a, xr)), b
        else:
            assert np.linalg.norm(x[b] - xr) <= 1e-8 * max(np.linalg.norm(xr), 1e-300), (b, kr)
        assert abs(lam1[b] - lr) <= 1e-8 * max(1.0, abs(lr)), (b, lam1[b], lr)
        ev = np.linalg.eigvalsh(A)[0]
        assert abs(mineig[b] - ev) <= 1e-11 * max(1.0, np.abs(A).max() * dim), (b, mineig[b], ev)


@pytest.mark.parametrize("dim", [200, 999])
def test_tri_wave_solves_match_one_lane_solves(dim, monkeypatch):
    """The tridiagonal path's subproblem solves on the whole wave (riptrm_tri.h PartSolve: 64 interior
    blocks eliminated in parallel, the separators' Schur complement by Thomas) against the one-lane
    LDL^T of the same T (RIPTRM_TRI_SERIAL=1): the same secular Newton and CG-skip decisions on
    reorderings of one factorisation, so the same kinds and, to rounding, the same steps and
    multipliers (x within 1e-10 relative, lam1 within 1e-11 relative)."""
    cases = _cases(dim, 4, [dim])
    monkeypatch.delenv("RIPTRM_TRI_SERIAL", raising=False)
    xw, lw, kw, mw = _solve(cases)
    monkeypatch.setenv("RIPTRM_TRI_SERIAL", "1")
    xs, ls, ks, ms = _solve(cases)
    np.testing.assert_array_equal(kw, ks)
    np.testing.assert_array_equal(mw, ms)   # the extreme eigenvalues do not depend on the solves
    for b in range(len(cases)):
        assert np.linalg.norm(xw[b] - xs[b]) <= 1e-10 * np.linalg.norm(xs[b]), (b, np.linalg.norm(xw[b] - xs[b]))
        assert abs(lw[b] - ls[b]) <= 1e-11 * max(1.0, abs(ls[b])), (b, lw[b], ls[b])


@pytest.mark.parametrize("n", [120, 250])
def test_trs_gep_hard_case_above_lds_size(n):
    """The hard case (a orthogonal to lam_min's eigenvector): at 120 the eigen-coordinates of
    riptrm_eig.h; at 250 the tridiagonal path detects it (riptrm_tri.h k_tri_solve: the component of
    H^T a on the twisted eigenvector of lam_min) and hands the subproblem to the eigendecomposition
    path (rocSOLVER dsyevd), which solves it as at 120."""
    rs = np.random.RandomState(8)
    cases = []
    for _ in range(2):
        Q, _ = np.linalg.qr(rs.randn(n, n))
        lam = np.sort(rs.randn(n))
        lam[0] = -3.0
        A = Q @ np.diag(lam) @ Q.T
        g = rs.randn(n)
        g[0] = 0.0
        x2 = np.linalg.norm(g[1:] / (lam[1:] - lam[0]))   # ||(A - lam_min I)^+ a||: the radius must exceed it
        cases.append((A, Q @ g, 2.0 * x2))
    x, lam1, kind, _ = _solve(cases)
    for b, (A, a, Del) in enumerate(cases):
        xr, lr, kr = T.trs_gep(A, a, Del, 1e-8)
        # the device takes the hard case from the eigendecomposition (a orthogonal to q_min); the
        # pencil detects it through ||x|| < tolhardcase of its eigenvector and at this size misses
        # it on the second case (CPU: trs_gep 'boundary' with model value -108.29, trs_eigh
        # 'hardcase_1' with -132.80, the true minimum): there the device must be no worse
        assert int(kind[b]) == 8, b
        assert np.isclose(np.linalg.norm(x[b]), Del, rtol=1e-12)
        if kr == "hardcase_1":
            assert np.isclose(lam1[b], lr, rtol=1e-8)
            assert np.isclose(_obj(A, a, x[b]), _obj(A, a, xr), rtol=1e-10)
        else:
            assert kr == "boundary" and np.isclose(lam1[b], lr, rtol=1e-6)
            assert _obj(A, a, x[b]) <= _obj(A, a, xr) + 1e-10 * abs(_obj(A, a, xr))
            xe, le, ke = T.trs_eigh(A, a, Del, 1e-8)
            assert ke == "hardcase_1" and np.isclose(_obj(A, a, x[b]), _obj(A, a, xe), rtol=1e-10)


def _clustered(m, rs, gaps):
    """Q diag(lam) Q^T with prescribed eigenvalue clusters: lam has exact doubles, near-doubles at the
    given relative gaps and a triple at the bottom (the hard case's multiplicity)."""
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


@pytest.mark.parametrize("m", [1, 2, 3, 50, 97, 100, 150, 199])
def test_sym_eig_matches_lapack(m):
    """The hand-written batched eigensolver (riptrm_sym_eig, csrc/riptrm_eig.h) against LAPACK
    (numpy.linalg.eigh): random symmetric matrices, the kind of matrix Exact_RepMat builds (a
    shifted frame matrix with a few huge diagonal entries y_i / x_i) and clustered spectra (exact and
    near-multiple eigenvalues, a triple at the bottom).  Eigenvalues within 1e-13 ||A||, residual
    ||A v - lam v|| and orthogonality ||V V^T - I|| within 1e-12 (scaled)."""
    import trs
    rs = np.random.RandomState(m)
    mats = [rs.randn(m, m)]
    mats[0] = mats[0] + mats[0].T
    D = rs.randn(m, m) / np.sqrt(m)
    D = D + D.T + np.diag(np.where(rs.rand(m) < 0.3, 10.0 ** rs.uniform(2, 6, m), 0.0))
    mats.append(D)
    if m >= 40:
        mats.append(_clustered(m, rs, (1e-4, 1e-8, 1e-12)))
    A = torch.tensor(np.stack(mats), dtype=torch.float64, device="cuda")
    w, V, info = trs.sym_eig(A)
    torch.cuda.synchronize()
    w, V, info = w.cpu().numpy(), V.cpu().numpy(), info.cpu().numpy()
    assert (info == 0).all()
    for k, M in enumerate(mats):
        nrm = np.linalg.norm(M, 2)
        ref = np.linalg.eigvalsh(M)
        assert np.max(np.abs(w[k] - ref)) <= 1e-13 * max(nrm, 1e-300) * max(1.0, np.sqrt(m) / 4), (k, np.max(np.abs(w[k] - ref)) / nrm)
        R = V[k] @ M - w[k][:, None] * V[k]
        assert np.max(np.linalg.norm(R, axis=1)) <= 1e-12 * nrm, (k, np.max(np.linalg.norm(R, axis=1)) / nrm)
        O = V[k] @ V[k].T - np.eye(m)
        assert np.max(np.abs(O)) <= 1e-12, (k, np.max(np.abs(O)))
    w2, V2, _ = trs.sym_eig(A, vectors=False)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(w2.cpu().numpy(), w)     # the same bisection with or without vectors
    w3, V3, _ = trs.sym_eig(A[-1:].contiguous())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(w3.cpu().numpy()[0], w[-1])   # batch-independent bits
    np.testing.assert_array_equal(V3.cpu().numpy()[0], V[-1])


@pytest.mark.parametrize("m", [64, 200, 257, 513, 1000])
def test_sym_tridiag_matches_lapack(m):
    """The distributed tridiagonal reduction (riptrm_sym_tridiag, csrc/riptrm_tri.h k_tridiag_dist: the
    Exact_RepMat HBM service's first stage from order 150 on, one cooperative launch of ~m / 16..64
    workgroups exchanging p = tau A v per column) against LAPACK dsytrd (lower: the same dsytd2
    reflector convention, scipy.linalg.lapack.dsytrd).  Three matrices per batch (several matrices per
    launch): random, frame-like (O(1) part plus diagonal barrier terms up to 1e6), clustered spectrum.
    T's eigenvalues within 1e-13 ||A|| max(1, sqrt(m) / 4) of eigvalsh(A) (the reduction is backward
    stable), and d, e of the random matrix at the null-calibrated bar of tests/test_gpu_tridiag.py:
    within 4 x the worst of three CPU fp64 reductions + 2 eps of the longdouble reduction (at 1000,
    where that pass takes ~12 s: |GPU - dsytrd| <= 4 x |dsytrd - float64 restatement|); the frame-like
    and clustered ones are held to it at the orders of test_gpu_tridiag.py; a matrix reduced alone
    gives the same bits."""
    import scipy.linalg as sl
    import trs
    import tridiag_reference as R
    rs = np.random.RandomState(1000 + m)
    M0 = rs.randn(m, m)
    mats = [M0 + M0.T]
    D = rs.randn(m, m) / np.sqrt(m)
    mats.append(D + D.T + np.diag(np.where(rs.rand(m) < 0.3, 10.0 ** rs.uniform(2, 6, m), 0.0)))
    mats.append(_clustered(m, rs, (1e-4, 1e-8, 1e-12)))
    A = torch.tensor(np.stack(mats), dtype=torch.float64, device="cuda")
    d, e, info = trs.sym_tridiag(A)
    torch.cuda.synchronize()
    d, e, info = d.cpu().numpy(), e.cpu().numpy(), info.cpu().numpy()
    assert (info == 0).all(), info
    for k, M in enumerate(mats):
        nrm = np.linalg.norm(M, 2)
        wt = sl.eigvalsh_tridiagonal(d[k], e[k][:m - 1])
        ref = np.linalg.eigvalsh(M)
        err = np.max(np.abs(wt - ref))
        assert err <= 1e-13 * nrm * max(1.0, np.sqrt(m) / 4), (k, err / nrm)
    if m < 1000:
        R.assert_within_null_bar(mats[0], d[0], e[0], f"m={m} random")
    else:
        R.assert_within_fp64_null(mats[0], d[0], e[0], f"m={m} random")
    d1, e1, _ = trs.sym_tridiag(A[1:2].contiguous())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d1.cpu().numpy()[0], d[1])
    np.testing.assert_array_equal(e1.cpu().numpy()[0], e[1])


def _block(rs, m, pd, first):
    """diag(A1, A2) with a seam at m // 3: positive definite blocks, or indefinite ones with lam_min in
    the first (first=True) or the second block, one below the other block's smallest eigenvalue."""
    s = m // 3
    A = np.zeros((m, m))
    X, Y = rs.randn(s, s), rs.randn(m - s, m - s)
    if pd:
        A[:s, :s] = X @ X.T + np.eye(s)
        A[s:, s:] = Y @ Y.T + np.eye(m - s)
        return A
    A[:s, :s] = X + X.T
    A[s:, s:] = Y + Y.T
    l1, l2 = np.linalg.eigvalsh(A[:s, :s])[0], np.linalg.eigvalsh(A[s:, s:])[0]
    if first:
        A[:s, :s] += (l2 - 1.0 - l1) * np.eye(s)
    else:
        A[s:, s:] += (l1 - 1.0 - l2) * np.eye(m - s)
    return A


def _split_cases(m):
    """Subproblems whose T = H^T A H splits (some e_j = 0 after k_tri_solve's |e_j| <= 4 eps ||T|| rule):
    block-diagonal, diagonal and tridiagonal A; small radii on indefinite matrices (boundary) and a
    large radius on positive definite ones (interior: the CG runs on a T with zero couplings)."""
    rs = np.random.RandomState(7000 + m)
    t = rs.randn(m - 1)
    tri = np.diag(rs.randn(m)) + np.diag(t, 1) + np.diag(t, -1)
    tri_pd = np.diag(4.0 + rs.rand(m)) + np.diag(t / np.abs(t).max(), 1) + np.diag(t / np.abs(t).max(), -1)
    return [("block, lam_min in the first block", _block(rs, m, False, True), rs.randn(m), 0.1),
            ("block, lam_min in the second block", _block(rs, m, False, False), rs.randn(m), 1.0),
            ("block, positive definite", _block(rs, m, True, False), rs.randn(m), 100.0),
            ("diagonal", np.diag(rs.permutation(np.linspace(-2.0, 3.0, m))), rs.randn(m), 0.5),
            ("diagonal, positive definite", np.diag(rs.permutation(np.linspace(1.0, 5.0, m))), rs.randn(m), 100.0),
            ("tridiagonal", tri, rs.randn(m), 1.0),
            ("tridiagonal, positive definite", tri_pd, rs.randn(m), 100.0)]


def _check_against_oracle(cases, oracle, x, lam1, kind, mineig):
    """The bars of this module's docstring on solved cases (what, A, a, Del)."""
    from trs import KIND_NAMES
    kinds = []
    for b, (what, A, a, Del) in enumerate(cases):
        dim = A.shape[0]
        xr, lr, kr = oracle(A, a, Del, 1e-8)
        kinds.append(kr)
        print(f"[trs] dim {dim} {what}: {kr}, device {KIND_NAMES[int(kind[b])]}", flush=True)
        assert KIND_NAMES[int(kind[b])] == kr, (what, KIND_NAMES[int(kind[b])], kr)
        if kr == "interior":
            assert np.linalg.norm(x[b] - xr) <= 1e-4 * np.linalg.norm(xr), what
            assert np.linalg.norm(A @ x[b] + a) / np.linalg.norm(a) < 1e-5, what
            assert abs(_obj(A, a, x[b]) - _obj(A, a, xr)) <= 1e-8 * abs(_obj(A, a, xr)), what
        else:
            assert np.linalg.norm(x[b] - xr) <= 1e-8 * max(np.linalg.norm(xr), 1e-300), (what, kr)
        assert abs(lam1[b] - lr) <= 1e-8 * max(1.0, abs(lr)), (what, lam1[b], lr)
        ev = np.linalg.eigvalsh(A)[0]
        assert abs(mineig[b] - ev) <= 1e-11 * max(1.0, np.abs(A).max() * dim), (what, mineig[b], ev)
    return kinds


@pytest.mark.parametrize("m", [150, 257, 513])
def test_trs_gep_split_tridiagonal(m):
    """A dense random matrix never splits, so k_tri_solve's split handling (riptrm_tri.h: e_j -> 0 where
    |e_j| <= 4 eps ||T||, twisted_min's block search, the LDL^T solves and the CG on a T with zero
    couplings) is reached here: _split_cases, against the pencil (150) or the eigh formulation (257,
    513: the two agree on these cases' kinds, checked on the CPU when the cases were chosen) at the
    bars of test_trs_gep_above_lds_size_matches_oracle.  These inputs also take the reduction's tau = 0
    branches (every column of a diagonal or tridiagonal matrix, the seam of a block-diagonal one)."""
    cases = _split_cases(m)
    x, lam1, kind, mineig = _solve([c[1:] for c in cases])
    kinds = _check_against_oracle(cases, T.trs_gep if m == 150 else T.trs_eigh, x, lam1, kind, mineig)
    assert kinds == ["boundary", "boundary", "interior", "boundary", "interior", "boundary", "interior"], kinds


@pytest.mark.parametrize("m", [150, 257, 513])
def test_trs_gep_multiple_smallest_eigenvalue(m):
    """A triple lam_min with a generic a is no hard case, but the tridiagonal path's twisted eigenvector
    spans one direction of the eigenspace only: k_tri_solve must hand the subproblem to the
    eigendecomposition path (Sturm count above lam_min + 1e-12 max(1, |lambda|_max) > 1).  _clustered
    is indefinite, so at radius 1 the oracle's kind is boundary (trs_gep and trs_eigh agree on it, CPU);
    kind, x and lam1 at the boundary bars, the model value within 1e-10 relative (the hard-case tests'
    bar), against trs_eigh."""
    rs = np.random.RandomState(9000 + m)
    cases = [("triple lam_min", _clustered(m, rs, (1e-4, 1e-8, 1e-12)), rs.randn(m), 1.0)]
    x, lam1, kind, mineig = _solve([c[1:] for c in cases])
    kinds = _check_against_oracle(cases, T.trs_eigh, x, lam1, kind, mineig)
    assert kinds == ["boundary"]
    _, A, a, Del = cases[0]
    xr, _, _ = T.trs_eigh(A, a, Del, 1e-8)
    assert np.isclose(_obj(A, a, x[0]), _obj(A, a, xr), rtol=1e-10)


def _scipy_cg_decision(A, a, Del):
    """The reference's interior candidate (RIPTRM.py:243-248): SciPy's CG on A p = -a (rtol 1e-5, at
    most 10 m iterations) and its eligibility: (eligible, p1, relative true residual)."""
    import scipy.sparse.linalg as sla
    p1, _ = sla.cg(A, -a)
    rr = np.linalg.norm(A @ p1 + a) / np.linalg.norm(a)
    return bool(rr < 1e-5 and p1 @ p1 < Del ** 2), p1, rr


def _hard_cg_cases(m, rs):
    """Subproblems whose interior candidate is delicate: positive definite with condition numbers
    1e2 .. 1e9 (SciPy's CG needs many iterations; its true residual drifts from the recurrence's),
    the radius just above / below ||A^-1 a|| (the p1^T p1 >= Del^2 test), a nearly singular matrix,
    and an indefinite one with one small negative eigenvalue (CG on an indefinite A)."""
    out = []
    Q, _ = np.linalg.qr(rs.randn(m, m))
    for cond in (1e2, 1e5, 1e7, 1e9):
        lam = np.geomspace(1.0, cond, m)[::-1] / cond * 10.0
        A = (Q * lam) @ Q.T
        A = (A + A.T) / 2
        a = rs.randn(m)
        xn = np.linalg.norm(np.linalg.solve(A, -a))
        out.append((A, a, 10.0 * xn, f"pd cond {cond:.0e}, large radius"))
        out.append((A, a, xn * (1 + 1e-3), f"pd cond {cond:.0e}, radius just above ||A^-1 a||"))
        out.append((A, a, xn * (1 - 1e-3), f"pd cond {cond:.0e}, radius just below"))
    lam = np.sort(np.abs(rs.randn(m))) + 0.1
    lam[0] = 1e-10
    A = (Q * lam) @ Q.T
    A = (A + A.T) / 2
    a = rs.randn(m)
    out.append((A, a, 1e3, "nearly singular"))
    a0 = a - Q[:, 0] * (Q[:, 0] @ a)   # no component on the near-null direction: an interior solution
    out.append((A, a0, 10.0 * np.linalg.norm(np.linalg.lstsq(A, -a0, rcond=1e-8)[0]), "nearly singular, interior"))
    lam = np.sort(np.abs(rs.randn(m))) + 0.5
    lam[0] = -1e-3
    A = (Q * lam) @ Q.T
    A = (A + A.T) / 2
    out.append((A, rs.randn(m), 1e3, "indefinite, small negative eigenvalue"))
    return out


@pytest.mark.timeout(600)
@pytest.mark.parametrize("m", [120, 199, 300])
def test_compact_cg_matches_dense_cg_on_delicate_subproblems(m, monkeypatch):
    """at orders 97..199 the HBM service runs SciPy's CG (RIPTRM.py:243-248) in the
    eigen-coordinates of A (k_cg_diag on diag(lam) y = -Q^T a) instead of on A.  The two are the same
    iteration only in exact arithmetic, so on subproblems where the interior candidate is delicate
    (_hard_cg_cases) the default path is held against the dense CG on A (RIPTRM_BIG_EIG=r: k_cg_wave
    / k_cg_wg and rocSOLVER) and against the reference's own decision (SciPy on the CPU):
    * where the reference's decision is stable under summation order (SciPy's CG on three symmetric
      permutations P A P^T of the same subproblem decide alike), both device paths must take it:
      the same kind; an interior x meets the reference's own test (true residual < 1e-5, inside the
      radius) with SciPy's model value to within the two CG iterates' own error bound, a boundary x within 1e-8;
    * where it is not stable (a genuine tie of the reference itself), each device path must still
      return a candidate the reference could have returned (an interior x passing its test, or the
      boundary solution).
    At least 2/3 of the cases must be stable (the test is not vacuous)."""
    from trs import KIND_NAMES
    rs = np.random.RandomState(m)
    cases = _hard_cg_cases(m, rs)
    A = [c[0] for c in cases]
    solved = {}
    for mode in ("default", "r"):
        if mode == "r":
            monkeypatch.setenv("RIPTRM_BIG_EIG", "r")
        else:
            monkeypatch.delenv("RIPTRM_BIG_EIG", raising=False)
        solved[mode] = _solve([(c[0], c[1], c[2]) for c in cases])
    stable = 0
    for b, (Ab, a, Del, what) in enumerate(cases):
        ok, p1, rr = _scipy_cg_decision(Ab, a, Del)
        decisions = [ok]
        for sd in (1, 2, 3):
            p = np.random.RandomState(sd).permutation(m)
            decisions.append(_scipy_cg_decision(np.ascontiguousarray(Ab[p][:, p]), a[p], Del)[0])
        xb, lb, kb = T.trs_eigh(Ab, a, Del, 1e-8)   # the boundary / hard-case candidate
        ref_kind = "interior" if ok and _obj(Ab, a, p1) <= _obj(Ab, a, xb) else kb
        robust = len(set(decisions)) == 1
        stable += robust
        for mode in ("default", "r"):
            x, lam1, kind, _ = solved[mode]
            k = KIND_NAMES[int(kind[b])]
            print(f"[cg] m={m} {what}: scipy rr {rr:.1e} eligible {decisions} -> {ref_kind}; {mode}: {k}", flush=True)
            if k == "interior":
                assert np.linalg.norm(Ab @ x[b] + a) / np.linalg.norm(a) < 1e-5 and x[b] @ x[b] < Del ** 2, (what, mode)
                assert _obj(Ab, a, x[b]) <= _obj(Ab, a, xb) + 1e-10 * abs(_obj(Ab, a, xb)) + \
                    10 * m * np.finfo(float).eps * np.linalg.norm(Ab, 2) * max(x[b] @ x[b], xb @ xb), (what, mode)
            else:   # the boundary solution: x within 1e-8, or (at condition numbers 1e9, where both solves
                # of the secular equation carry ~eps cond) on the sphere with the same model value to 1e-8
                assert np.linalg.norm(x[b] - xb) <= 1e-8 * max(np.linalg.norm(xb), 1e-300) or \
                    (abs(np.linalg.norm(x[b]) - Del) <= 1e-10 * Del and
                     abs(_obj(Ab, a, x[b]) - _obj(Ab, a, xb)) <= 1e-8 * abs(_obj(Ab, a, xb))), (what, mode, k)
            if robust:
                assert k == ref_kind, (what, mode, k, ref_kind, decisions)
                if k == "interior":
                    # both are CG iterates at rtol 1e-5, so x moves by up to cond x 1e-5 and the model
                    # value by each iterate's own error r^T A^-1 r / 2 <= ||r||^2 / (2 lam_min)
                    # (plus the evaluation's own rounding, ~m eps ||A|| ||x||^2)
                    lmin = max(np.linalg.eigvalsh(Ab)[0], 1e-300)
                    rx, rp = np.linalg.norm(Ab @ x[b] + a), np.linalg.norm(Ab @ p1 + a)
                    ev_err = 10 * m * np.finfo(float).eps * np.linalg.norm(Ab, 2) * max(x[b] @ x[b], p1 @ p1)
                    bound = (rx * rx + rp * rp) / (2.0 * lmin) + 1e-8 * abs(_obj(Ab, a, p1)) + ev_err
                    assert abs(_obj(Ab, a, x[b]) - _obj(Ab, a, p1)) <= bound, (what, mode)
    assert stable >= 2 * len(cases) // 3, stable
