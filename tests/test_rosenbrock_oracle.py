"""CPU checks of the Rosenbrock-on-Grassmann oracle (tests/rosenbrock_oracle.py), the checker of
tests/test_gpu_rosenbrock.py: the cost is the quadratic the closed forms assume, the closed forms
agree with the coordinator taken literally, the manifold class behaves like pymanopt's Grassmann, and
the reference's own rounding variants stay inside the unchanged trajectory bar
(tests/parity.py::compare_until_flip) on the instances the GPU trajectory test uses."""
import numpy as np
import pytest

import rosenbrock_oracle as R
from parity import compare_until_flip

SHAPES = [(5, 3), (13, 5), (16, 4)]
TRAJ_OPT = R.TRAJECTORY_OPTION
fixed_clock = R.fixed_clock


def test_cost_is_the_quadratic_with_hessian_T():
    rs = np.random.RandomState(0)
    for n, k in SHAPES:
        P = R.RosenbrockVectorized(n, k, 1e7)
        Ps = R.RosenbrockStructured(n, k, 1e7)
        X = R.feasible_point(n, k, rs)
        U = rs.randn(n, k)
        t = 1e-3
        f0 = P.cost(X)
        model = t * np.sum(P.egrad(X) * U) + 0.5 * t * t * np.sum(U * P.Tu(U))
        for cost in (P.cost, Ps.cost):
            err = abs((cost(X + t * U) - cost(X)) - model)
            assert err <= 1e-10 * abs(f0), (n, k, err, f0)
        assert abs(Ps.cost(X) - f0) <= 1e-13 * abs(f0)


@pytest.mark.parametrize("n,k", SHAPES)
@pytest.mark.parametrize("alpha", [1.0, 1e7])
def test_structured_and_vectorized_agree(n, k, alpha):
    rs = np.random.RandomState(7 * n + k)
    Pv = R.RosenbrockVectorized(n, k, alpha)
    Ps = R.RosenbrockStructured(n, k, alpha)
    M = Pv.manifold

    def close(a, b, what):
        a, b = np.asarray(a, float), np.asarray(b, float)
        scale = max(np.max(np.abs(b)), 1e-300)
        assert np.max(np.abs(a - b)) <= 1e-12 * scale, (what, np.max(np.abs(a - b)) / scale)

    for trial in range(3):
        X = R.feasible_point(n, k, rs)
        y = 0.5 + rs.rand(n * k)
        mu = [0.1, 1e-3, 1e-6][trial]
        V = M.projection(X, rs.randn(n, k))
        cv, sv, Hv, c_v = Pv.begin_inner(X, y, mu)
        cs, ss, Hs, c_s = Ps.begin_inner(X, y, mu)
        close(cv, cs, "cost")
        close(sv, ss, "slack")
        close(Hv(V), Hs(V), "Hw")
        close(c_v, c_s, "c")
        close(Pv.dy(X, y, sv, mu, V), Ps.dy(X, y, ss, mu, V), "dy")
        close(Pv.gradlag(X, y), Ps.gradlag(X, y), "gradlag")
        mv = R.rank_manvio(k)
        rv, rs_ = Pv.residual(X, y, mv), Ps.residual(X, y, mv)
        close(rv[0], rs_[0], "residual")
        close(rv[1:4], rs_[1:4], "residual parts")
        close(Pv.maxmeanviolations(X), Ps.maxmeanviolations(X), "violations")


@pytest.mark.parametrize("n,k", SHAPES + [(7, 1), (9, 8)])
def test_grassmann_class(n, k):
    rs = np.random.RandomState(n + 31 * k)
    M = R.Grassmann(n, k, polar="gram")
    Ms = R.Grassmann(n, k, polar="svd")
    X = R.feasible_point(n, k, rs)
    U = M.projection(X, rs.randn(n, k))
    assert np.max(np.abs(X.T @ U)) <= 1e-14 * k * np.max(np.abs(U))
    U = U / np.linalg.norm(U)
    # Step lengths up to 1 (the solver's first radius is sqrt(k) / 8).  The Gram form's loss of
    # orthogonality is eps cond(A^T A) = eps (1 + ||U||^2), so the 1e-14 k bar holds on these steps.
    for scale in (1e-3, 0.2, 1.0):
        Rg = M.retraction(X, scale * U)
        assert np.linalg.norm(Rg.T @ Rg - np.eye(k)) <= 1e-14 * k
        u, _, vt = np.linalg.svd(X + scale * U, full_matrices=False)
        Rs = u @ vt
        assert np.linalg.norm(Rs.T @ Rs - np.eye(k)) <= 1e-14 * k
        assert np.max(np.abs(Rs - Ms.retraction(X, scale * U))) == 0.0
        assert np.max(np.abs(Rg @ Rg.T - Rs @ Rs.T)) <= 1e-13   # the same subspace
        assert np.max(np.abs(Rg - Rs)) <= 1e-13                 # and the same frame: the polar factor
    Y = M.retraction(X, 0.7 * U)
    # "dist(X, X) = 0, and dist is symmetric" cannot hold to the bit in pymanopt's formula, so this
    # departs from the plain wording with bounds worked out from the formats.  On an exactly orthonormal
    # frame (the coordinator's start) it is exactly 0.  On a frame orthonormal to delta = ||X^T X - I||
    # the singular values of X^T X are >= 1 - delta (plus their own rounding) and arccos(1 - d) =
    # sqrt(2 d), so dist(X, X) <= sqrt(2 k delta) ~ 1e-7: numpy's own value is not 0 there.
    E = np.eye(n)[:, :k]
    assert M.dist(E, E) == 0.0
    delta = np.linalg.norm(X.T @ X - np.eye(k), 2) + 4 * np.finfo(float).eps
    assert M.dist(X, X) <= np.sqrt(2 * k * delta)
    # Symmetry: X^T Y and Y^T X are transposes with the same singular values, which LAPACK returns to a
    # few ulp of the largest (1); at this well-separated Y (angles ~0.1..0.7, arccos' slope < 10) that is
    # 1e-14 in the distance
    assert abs(M.dist(X, Y) - M.dist(Y, X)) <= 1e-14 * np.sqrt(k)
    assert M.dim == k * (n - k) and M.typical_dist == np.sqrt(k)
    assert R.rank_manvio(k)(X) == 0
    if k > 1:
        Xb = X.copy()
        Xb[:, 1] = Xb[:, 0]
        assert R.rank_manvio(k)(Xb) == np.inf


def _instances():
    out = [(n, k, a) for (n, k), alphas in R.TRAJECTORY_INSTANCES.items() for a in alphas]
    return out + R.TRAJECTORY_EXTRA


@pytest.mark.parametrize("n,k,alpha", _instances())
def test_order_variants_stay_within_the_trajectory_bar(n, k, alpha):
    """Calibration of tests/test_gpu_rosenbrock.py's trajectory test: the same arithmetic in another
    rounding order (three seeds) passes compare_until_flip against the base oracle run, and every outer
    iteration of the base run converges."""
    ref = R.solve(n, k, alpha, option=TRAJ_OPT, clock=fixed_clock)
    it, st = ref.log["iteration"], ref.log["inner_status"]
    last = [st[i] for i in range(1, len(it)) if i == len(it) - 1 or it[i + 1] != it[i]]
    assert last == ["converged"] * 6
    for v in R.order_variants(n, k, alpha, option=TRAJ_OPT, seeds=(1, 2, 3), clock=fixed_clock):
        compare_until_flip(v.log, ref.log, tight_rows=20, late_row=20)


def test_structured_run_matches_vectorized_run():
    ref = R.solve(5, 3, 100.0, option=TRAJ_OPT, clock=fixed_clock)
    st = R.solve(5, 3, 100.0, option=TRAJ_OPT, clock=fixed_clock, structured=True)
    compare_until_flip(st.log, ref.log)
    assert np.max(np.abs(st.x @ st.x.T - ref.x @ ref.x.T)) <= 1e-6


def test_host_side_problem_coordinator_and_manvio_classifier():
    """The host pieces that need no GPU: the descriptor's defaults are the coordinator's, the drop-in
    module builds it from a cfg, and the option classifier tells the simulator's rank function from 0."""
    import importlib.util
    import os
    import rosenbrock
    from engine import C
    from RIPTRM import _any_manvio_kind
    pkg = os.path.dirname(os.path.abspath(rosenbrock.__file__))
    spec = importlib.util.spec_from_file_location("rosenbrock_dropin_coordinator_cpu",
                                                  os.path.join(pkg, "dropin", "Rosenbrock", "coordinator.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    prob = mod.Coordinator({"n": 5, "k": 3, "alpha": 1e7, "problem_coordinator_name": "coordinator"}).run()
    x0, y0 = R.initial_point(5, 3)
    assert isinstance(prob, rosenbrock.RosenbrockProblem) and (prob.n, prob.k, prob.alpha, prob.lb) == (5, 3, 1e7, R.LB)
    assert np.array_equal(prob.initialpoint, x0) and np.array_equal(prob.initialineqLagmult, y0)
    assert (prob.num_ineqconstraints, prob.has_eqconstraints, prob.manifold_dim) == (15, False, 6)
    assert prob.typical_dist == R.Grassmann(5, 3).typical_dist
    xr = R.feasible_point(5, 3, np.random.RandomState(0))
    assert abs(prob.cost(xr) - R.RosenbrockStructured(5, 3, 1e7).cost(xr)) <= 1e-13 * prob.cost(xr)
    assert rosenbrock.rosenbrock_manvio_kind(rosenbrock.manviofun) == C["RIPTRM_MANVIO_GRASSMANN_RANK"]
    assert _any_manvio_kind(rosenbrock.manviofun) == C["RIPTRM_MANVIO_GRASSMANN_RANK"]
    assert rosenbrock.rosenbrock_manvio_kind(lambda problem, x: 0) == C["RIPTRM_MANVIO_ZERO"]

    def reference_style(problem, x):   # reads k from the problem's manifold, as the simulator's does
        return 0 if np.linalg.matrix_rank(x) == problem.manifold._p else np.inf

    assert rosenbrock.rosenbrock_manvio_kind(reference_style) == C["RIPTRM_MANVIO_GRASSMANN_RANK"]
    assert _any_manvio_kind(reference_style) == C["RIPTRM_MANVIO_GRASSMANN_RANK"]
    with pytest.raises(NotImplementedError):
        rosenbrock.rosenbrock_manvio_kind(lambda problem, x: 1.0)
    if not __import__("torch").cuda.is_available():   # no GPU: an error, not a fallback
        with pytest.raises(RuntimeError):
            rosenbrock.RosenbrockBatch(5, 3, 1)
