"""CPU tests of Exact_RepMat for Rosenbrock on Grassmann(n, k): the pinned frame (``rosenbrock.basisfun``),
its classifier, why the frame and its order are part of the contract, and the calibration of
tests/test_gpu_rosenbrock_exact.py's trajectory test.  No GPU."""
import numpy as np
import pytest

import rosenbrock
import rosenbrock_exact as X
import rosenbrock_oracle as R
from parity import compare_until_flip

PINNED = rosenbrock.basisfun   # the feature: every test here checks it or calibrates the GPU tests of it

SHAPES = [(5, 3), (7, 1), (9, 8), (13, 5), (16, 4), (64, 8)]   # tests/test_gpu_rosenbrock.py's


@pytest.mark.parametrize("n,k", SHAPES)
def test_frame_is_orthonormal_horizontal_and_the_helpers(n, k):
    import rosenbrock
    rs = np.random.RandomState(31 * n + k)
    for x in (R.feasible_point(n, k, rs), R.initial_point(n, k)[0], -np.linalg.qr(rs.randn(n, k))[0]):
        basis = rosenbrock.basisfun(None, x)
        d = k * (n - k)
        assert len(basis) == d and all(b.shape == (n, k) for b in basis)
        F = np.array([b.ravel() for b in basis])
        assert np.max(np.abs(F @ F.T - np.eye(d))) <= 16 * X.EPS
        assert max(np.max(np.abs(x.T @ b)) for b in basis) <= 16 * X.EPS
        assert max(np.max(np.abs(b - h)) for b, h in zip(basis, X.frame(x))) <= 16 * X.EPS
        # vector a k + b has the single column b
        for c, b in enumerate(basis):
            assert not np.delete(b, c % k, axis=1).any()


def _random_basis(seed):
    def f(manifold, x):
        n, k = x.shape
        rs = np.random.RandomState(seed)
        vs = []
        for _ in range(k * (n - k)):
            v = rs.randn(n, k)
            v = v - x @ (x.T @ v)
            for q in vs:
                v = v - np.sum(q * v) * q
            vs.append(v / np.linalg.norm(v))
        return vs
    return f


def test_classifier():
    import rosenbrock
    assert rosenbrock.rosenbrock_basis_kind(rosenbrock.basisfun) == 1
    assert rosenbrock.rosenbrock_basis_kind(lambda manifold, x: X.frame(x)) == 1   # an independent implementation

    def swapped(manifold, x):
        b = X.frame(x)
        b[0], b[1] = b[1], b[0]
        return b

    for bad in (None, _random_basis(0), swapped, lambda manifold, x: X.frame(x)[:-1], lambda manifold, x: 0):
        with pytest.raises(NotImplementedError, match="Rosenbrock.*basisfun=rosenbrock.basisfun"):
            rosenbrock.rosenbrock_basis_kind(bad)


def test_basisfun_serves_the_reference_procedure():
    """``rosenbrock.basisfun`` handed to the reference's own steps (selfadj_operator2matrix, TRSgep): the
    same matrix as in the helper frame, to rounding."""
    import rosenbrock
    from oracle.trs_oracle import selfadj_operator2matrix
    n, k, alpha = 5, 3, 1e3
    rs = np.random.RandomState(4)
    x, y = R.feasible_point(n, k, rs), 0.5 + rs.rand(n * k)
    P = X.RosenbrockExact(n, k, alpha)
    _, _, Hw, _ = P.begin_inner(x, y, 0.1)
    A = selfadj_operator2matrix(P.manifold, x, Hw, rosenbrock.basisfun(P.manifold, x))
    B, _ = X.matrix_and_linear_term(n, k, alpha, x, y, 0.1)
    assert np.max(np.abs(A - B)) <= 32 * 6 * X.EPS * X.scale_of(n, k, alpha, x, y)


def test_the_mirrored_triangle_is_not_the_symmetric_part():
    """Why the frame and its order are part of the contract: at (5, 3), alpha = 1e3 the reference's matrix
    (upper triangle mirrored) is farther from the symmetric part than 100 times the GPU test's bar on a
    matrix entry, and another order of the same vectors gives another matrix."""
    n, k, alpha = 5, 3, 1e3
    rs = np.random.RandomState(4)
    x, y = R.feasible_point(n, k, rs), 0.5 + rs.rand(n * k)
    P = X.RosenbrockExact(n, k, alpha)
    _, _, Hw, _ = P.begin_inner(x, y, 0.1)
    basis = P.tangent_basis(x)
    F = np.array([b.ravel() for b in basis])
    full = F @ np.array([Hw(b).ravel() for b in basis]).T          # <b_i, Hw(b_j)>
    mirrored, _ = X.matrix_and_linear_term(n, k, alpha, x, y, 0.1)
    bar = 32 * len(basis) * X.EPS * X.scale_of(n, k, alpha, x, y)
    gap = np.max(np.abs(mirrored - 0.5 * (full + full.T)))
    print(f"mirrored vs symmetric part: {gap:.3g} = {gap / bar:.3g} bars")
    assert gap > 100 * bar
    p = [1, 0] + list(range(2, len(basis)))
    from oracle.trs_oracle import selfadj_operator2matrix
    other = selfadj_operator2matrix(P.manifold, x, Hw, [basis[i] for i in p])
    assert np.max(np.abs(other - mirrored[np.ix_(p, p)])) > 100 * bar


def test_the_two_cpu_forms_of_trsgep_part_on_the_uncalibrated_instance():
    """Why (5, 3) at alpha = 1e7 is not a trajectory instance: the pencil (trs_gep) and the eigendecomposition
    (trs_eigh) runs of the same oracle leave compare_until_flip's bar on the CPU alone, in the radius of row 18
    (gamma ||dx|| of an interior CG step: 0.0760428 against 0.0761994)."""
    n, k, alpha = X.UNCALIBRATED
    assert alpha not in X.TRAJECTORY_INSTANCES[(n, k)]
    ref, alt = X.solve(n, k, alpha), X.solve_eigh_form(n, k, alpha)
    with pytest.raises(AssertionError, match="TR_radius"):
        compare_until_flip(alt.log, ref.log, tight_rows=20, late_row=20)
    assert ref.log["dxtype"][:19] == alt.log["dxtype"][:19]
    assert abs(ref.log["TR_radius"][18] - alt.log["TR_radius"][18]) > 1e-3 * ref.log["TR_radius"][18]


@pytest.fixture(scope="module")
def runs():
    return {(n, k, a): X.solve(n, k, a) for (n, k), al in X.TRAJECTORY_INSTANCES.items() for a in al}


@pytest.mark.parametrize("n,k,alpha", [(n, k, a) for (n, k), al in X.TRAJECTORY_INSTANCES.items() for a in al])
def test_order_variants_stay_within_the_trajectory_bar(n, k, alpha, runs):
    """Calibration of the GPU trajectory test, as tests/test_rosenbrock_oracle.py does for tCG: the same
    arithmetic in another rounding order, the other CPU form of TRSgep (trs_eigh, the device's) and the run with
    the radius-expansion tie of row 1 taken the other way pass compare_until_flip against the base run; every
    outer iteration converges; both direction types occur and mineigvalHw takes both signs."""
    ref = runs[(n, k, alpha)]
    it, st = ref.log["iteration"], ref.log["inner_status"]
    last = [st[i] for i in range(1, len(it)) if i == len(it) - 1 or it[i + 1] != it[i]]
    assert last == ["converged"] * X.option_for(n, k)["maxiter"]
    kinds = {v for v in ref.log["dxtype"] if v is not None}
    assert kinds == {"boundary", "interior"}
    me = [v for v in ref.log["mineigvalHw"] if v is not None]
    assert len(me) == len(it) - 1 and min(me) < 0 < max(me)
    for v in X.order_variants(n, k, alpha):
        compare_until_flip(v.log, ref.log, tight_rows=20, late_row=20)
