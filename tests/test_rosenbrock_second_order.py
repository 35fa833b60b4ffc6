"""CPU facts behind the device's second-order residual (tests/rosenbrock_second_order.py) and the host
side of the callback: its classifier, ``resolve_options`` and the log assembly.

The bar is the GPU test's: 32 d eps scale on an eigenvalue, scale = 4 alpha + 2 + ||X^T G_L||_2.  On the
GPU test's inputs (six shapes, three alphas, four active-set sizes each) the reference's procedure with
(A + A^T) / 2 in a drawn basis differs from ``sym_check`` by at most 9.9 d eps scale over seeds 1..3
(the (97, 1) points; below 2.2 elsewhere): a basis drawn and orthogonalised once by Gram-Schmidt is
orthonormal to about 1e-14 at d = 96, and that is what the figure measures.
"""
import numpy as np
import pytest

import rosenbrock_second_order as S
from rosenbrock_oracle import RosenbrockStructured, feasible_point


@pytest.mark.parametrize("n,k", S.SHAPES)
def test_symmetrised_drawn_basis_stays_within_the_gpu_bar(n, k):
    al, xs, ys, tols = S.inputs(n, k)
    ref = S.reference(n, k)
    worst = 0.0
    for p in range(len(al)):
        P = RosenbrockStructured(n, k, al[p])
        r = ref[p]
        assert r["nulldim"] > 0
        for seed in (1, 2, 3):
            lo, hi = S.drawn_check(P, xs[p], ys[p], tols[p], seed, symmetrise=True)
            err = max(abs(lo - r["mineig"]), abs(hi - r["maxeig"]))
            worst = max(worst, err / (r["bar"] / 32.0))
            assert err <= r["bar"], (p, seed, lo, r["mineig"], hi, r["maxeig"], r["bar"])
    print(f"({n}, {k}): worst |drawn - sym| = {worst:.3g} d eps scale")


def test_upper_triangle_mirror_depends_on_the_drawn_basis():
    """The finding: X^T G_L is not symmetric, so the operator is not self-adjoint and the matrix filled
    from its upper triangle changes with the basis draw, far beyond rounding; the symmetric part does not."""
    rs = np.random.RandomState(7)
    P = RosenbrockStructured(5, 3, 1e3)
    x, y = feasible_point(5, 3, rs), 0.1 + rs.rand(15)
    GL = P.euclidean_gradient(x) - y.reshape(5, 3)
    assert np.linalg.norm(x.T @ GL - (x.T @ GL).T) > 1.0
    bar = S.bar_of(P, x, y)
    mirrored = [S.drawn_check(P, x, y, 1e-5, s)[0] for s in (1, 2, 3, 4)]
    assert max(mirrored) - min(mirrored) > 100 * bar, (mirrored, bar)
    sym = S.sym_check(P, x, y, 1e-5)["mineig"]
    averaged = [S.drawn_check(P, x, y, 1e-5, s, symmetrise=True)[0] for s in (1, 2, 3, 4)]
    assert max(abs(v - sym) for v in averaged) <= bar, (averaged, sym, bar)


def test_callback_kind():
    import rosenbrock as RB
    assert RB.rosenbrock_callback_kind(None) == RB.CALLBACK_NONE
    assert RB.rosenbrock_callback_kind(lambda problem, x, y, z, eval: eval) == RB.CALLBACK_NONE
    assert RB.rosenbrock_callback_kind(lambda problem, xCur, option, eval: eval) == RB.CALLBACK_NONE
    assert RB.rosenbrock_callback_kind(RB.callbackfun) == RB.CALLBACK_SECOND_ORDER

    def wrong_key(problem, x, y, z, eval):
        eval["first_order_residual"] = 0.0
        return eval

    def wrong_value(problem, x, y, z, eval):
        eval["second_order_residual"] = 1.0
        eval["condition_number"] = 1.0
        return eval

    for f in (wrong_key, wrong_value):
        with pytest.raises(NotImplementedError):
            RB.rosenbrock_callback_kind(f)


def test_callback_kind_accepts_the_procedure_of_the_reference():
    """A callback written against the attributes src/Rosenbrock/simulator.py:60-98 reads (active
    constraints, their Riemannian gradients, random tangent vectors, the Hessians) is recognised on the
    probe, where k = 1 makes its upper-triangle matrix basis-independent."""
    import rosenbrock as RB

    def procedure(problem, x, y, z, eval):
        M = problem.manifold
        act = [i for i in range(problem.num_ineqconstraints) if abs(problem.ineqconstraints_all[i](x)) < 1e-5]
        basis = []
        for i in act:
            v = problem.ineqconstraints_riemannian_gradient(i)(x)
            for q in basis:
                v = v - M.inner_product(x, q, v) * q
            if M.norm(x, v) > 1e-12:
                basis.append(v / M.norm(x, v))
        null = []
        for _ in range(M.dim - len(basis)):
            v = M.random_tangent_vector(x)
            for q in basis + null:
                v = v - M.inner_product(x, q, v) * q
            null.append(v / M.norm(x, v))

        def H(v):
            out = problem.riemannian_hessian(x, v)
            for i in range(problem.num_ineqconstraints):
                out = out + y[i] * problem.ineqconstraints_riemannian_hessian_all[i](x, v)
            return out

        A = np.zeros((len(null), len(null)))
        for j in range(len(null)):
            Hj = H(null[j])
            for i in range(j + 1):
                A[i, j] = A[j, i] = M.inner_product(x, Hj, null[i])
        ev = np.linalg.eigvalsh(A)
        eval["second_order_residual"] = ev[0]
        eval["condition_number"] = ev[-1] / ev[0]
        return eval

    assert RB.rosenbrock_callback_kind(procedure) == RB.CALLBACK_SECOND_ORDER


def test_resolve_options_with_and_without_the_classifier():
    import engine
    import rosenbrock as RB
    identity = lambda problem, x, y, z, eval: eval
    base = {"TRS_solver": "tCG"}
    assert engine.resolve_options(base, 1.0, 16).callback_kind == 0
    for cb in (identity, RB.callbackfun):   # today's behaviour without a classifier: any callback raises
        with pytest.raises(NotImplementedError):
            engine.resolve_options(dict(base, callbackfun=cb), 1.0, 16)
    kw = dict(callback_classifier=RB.rosenbrock_callback_kind)
    assert engine.resolve_options(base, 1.0, 16, **kw).callback_kind == RB.CALLBACK_NONE
    assert engine.resolve_options(dict(base, callbackfun=identity), 1.0, 16, **kw).callback_kind == RB.CALLBACK_NONE
    ro = engine.resolve_options(dict(base, callbackfun=RB.callbackfun), 1.0, 16, **kw)
    assert ro.callback_kind == RB.CALLBACK_SECOND_ORDER

    def other(problem, x, y, z, eval):
        eval["something"] = 1
        return eval

    with pytest.raises(NotImplementedError):
        engine.resolve_options(dict(base, callbackfun=other), 1.0, 16, **kw)


def test_log_assembly_puts_the_callback_columns_after_meanviolation():
    import engine
    import rosenbrock as RB
    ro = engine.resolve_options({"TRS_solver": "tCG"}, 1.0, 16)
    rows = np.zeros((3, engine.NLOG))
    rows[:, engine.C["RIPTRM_LOG_ITERATION"]] = [0, 1, 1]
    so = {"mineig": np.array([-2.5, 0.0, np.nan]), "cond": np.array([-4.0, np.nan, np.nan])}
    cols = RB.second_order_columns(so)
    assert cols["condition_number"][0] == -4.0 and cols["condition_number"][1] is None
    res = engine.BatchResult(x=None, y=None, stats=np.zeros((1, engine.NSTAT)), raw_log=[rows], ro=ro,
                             dropped=np.zeros(1), callback_cols=[cols])
    log = res.log(0)
    keys = list(log)
    at = keys.index("meanviolation")
    assert keys[at + 1:at + 4] == ["second_order_residual", "condition_number", "mu"]
    assert log["second_order_residual"][:2] == [-2.5, 0.0] and np.isnan(log["second_order_residual"][2])
    assert log["condition_number"] == [-4.0, None, None]
    assert all(len(v) == 3 for v in log.values())
    plain = engine.BatchResult(x=None, y=None, stats=np.zeros((1, engine.NSTAT)), raw_log=[rows], ro=ro,
                               dropped=np.zeros(1)).log(0)
    assert [q for q in keys if q not in cols] == list(plain)
    with pytest.raises(RuntimeError):
        engine.BatchResult(x=None, y=None, stats=np.zeros((1, engine.NSTAT)), raw_log=[rows[:2]], ro=ro,
                           dropped=np.zeros(1), callback_cols=[cols]).log(0)
