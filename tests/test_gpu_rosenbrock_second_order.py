"""GPU tests of the second-order residual of Rosenbrock on Grassmann(n, k) (csrc/riptrm_grassmann_so.hip,
``RosenbrockBatch.second_order``, the ``callbackfun`` path of ``RIPTRM``) against the fp64 CPU statement
of the symmetric part's eigenvalues (tests/rosenbrock_second_order.py::sym_check).

Shapes: (5, 3) d = 6 the reference's, (8, 3) d = 15, (13, 7) d = 42 (k near KMAX, N = 91: two waves),
(16, 4) d = 48 (N = 64, exactly one wave), (20, 6) d = 84, (97, 1) d = 96 the limit (k = 1, two waves).
Every shape is one launch over 12 points: alpha in {1, 1e3, 1e7} x 0, 1, 2 or 4 active constraints.

Bar on an eigenvalue: 32 d eps scale, scale = 4 alpha + 2 + ||X^T G_L||_2 (+ max(y / s) with the barrier
term), an upper bound of the operator's norm; by Weyl's inequality a backward-stable assembly of M moves an
eigenvalue by O(d eps ||M||).  The CPU's own variants stay within 9.9 d eps scale on these inputs
(tests/test_rosenbrock_second_order.py).  Counts (nactive, nindep, nulldim) are exact, and cond is bitwise
maxeig / mineig of the device's own outputs.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import rosenbrock_oracle as R
import rosenbrock_second_order as S


def _engine(n, k, alpha, cap=16):
    import rosenbrock
    alpha = np.asarray(alpha, dtype=np.float64)
    B = 1 if alpha.ndim == 0 else len(alpha)
    return rosenbrock.RosenbrockBatch(n, k, B, log_capacity=cap).load(alpha, R.LB)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _check_point(so, p, ref, where):
    assert so["info"][p] == 0, where
    assert (so["nactive"][p], so["nindep"][p], so["nulldim"][p]) == (ref["nactive"], ref["nindep"], ref["nulldim"]), where
    lo, hi = so["mineig"][p], so["maxeig"][p]
    err = max(abs(lo - ref["mineig"]), abs(hi - ref["maxeig"]))
    assert err <= ref["bar"], (where, lo, ref["mineig"], hi, ref["maxeig"], ref["bar"])
    assert _bits(so["cond"][p]) == _bits(np.float64(hi) / np.float64(lo)), where
    return err / (ref["bar"] / 32.0)


@pytest.mark.parametrize("barrier", [False, True])
@pytest.mark.parametrize("n,k", S.SHAPES)
def test_second_order_matches_the_symmetric_part(n, k, barrier):
    al, xs, ys, tols = S.inputs(n, k)
    ref = S.reference(n, k, barrier)
    eng = _engine(n, k, al)
    so = eng.second_order(xs, ys, active_tol=tols, barrier=barrier, mu=np.full(len(al), S.MU) if barrier else None)
    worst = max(_check_point(so, p, ref[p], (n, k, barrier, p)) for p in range(len(al)))
    print(f"({n}, {k}) barrier={barrier}: worst eigenvalue error {worst:.3g} d eps scale")


def test_dependent_active_gradients_are_dropped():
    """Three active entries in one column of a (5, 3) point: their gradients' coordinates live in that
    column's n - k = 2 dimensions, so the third is dependent."""
    n, k, lb = 5, 3, R.LB
    rs = np.random.RandomState(11)
    c0 = np.array([-lb, -lb, -lb, 0.6, 0.0])
    c0[4] = np.sqrt(1.0 - np.sum(c0 ** 2))
    q, _ = np.linalg.qr(np.column_stack([c0, rs.rand(n), rs.rand(n)]))
    x = q * np.sign(q[3, 0])
    assert np.max(np.abs(x[:3, 0] + lb)) < 1e-15
    y = 0.1 + rs.rand(n * k)
    P = R.RosenbrockStructured(n, k, 1e3)
    ref = S.sym_check(P, x, y, 1e-6)
    ref["bar"] = S.bar_of(P, x, y)
    assert (ref["nactive"], ref["nindep"], ref["nulldim"]) == (3, 2, 4)
    so = _engine(n, k, 1e3).second_order(x[None], y[None], active_tol=1e-6)
    _check_point(so, 0, ref, "dependent")


def test_no_direction_left():
    """(4, 2), d = 4, every constraint active: mineig 0 and no condition number (simulator.py:91-93)."""
    import rosenbrock
    rs = np.random.RandomState(5)
    x, y = R.feasible_point(4, 2, rs), 0.1 + rs.rand(8)
    so = _engine(4, 2, 10.0).second_order(x[None], y[None], active_tol=1e3)
    assert (so["nactive"][0], so["nindep"][0], so["nulldim"][0], so["info"][0]) == (8, 4, 0, 0)
    assert so["mineig"][0] == 0 and np.isnan(so["cond"][0]) and np.isnan(so["maxeig"][0])
    cols = rosenbrock.second_order_columns(so)
    assert cols["second_order_residual"] == [0.0] and cols["condition_number"] == [None]


def test_module_callbackfun_evaluates_one_point():
    """``rosenbrock.callbackfun`` called the way utils.evaluation calls a callback (utils.py:366)."""
    import rosenbrock
    prob = rosenbrock.RosenbrockProblem(n=5, k=3, alpha=1e3)
    x0, y0 = R.initial_point(5, 3)
    ev = rosenbrock.callbackfun(prob, x0, y0, [], {"cost": 1.0})
    so = _engine(5, 3, 1e3).second_order(x0[None], y0[None])
    assert list(ev) == ["cost", "second_order_residual", "condition_number"]
    assert _bits(ev["second_order_residual"]) == _bits(so["mineig"][0])
    assert _bits(ev["condition_number"]) == _bits(so["cond"][0])


def test_a_nonfinite_point_is_isolated():
    n, k = 8, 3
    al, xs, ys, tols = S.inputs(n, k)
    eng = _engine(n, k, al)
    clean = eng.second_order(xs, ys, active_tol=tols)
    bad = xs.copy()
    bad[5, 0, 0] = np.nan
    so = eng.second_order(bad, ys, active_tol=tols)
    assert so["info"][5] == 1 and np.isnan(so["mineig"][5]) and np.isnan(so["cond"][5])
    keep = np.arange(len(al)) != 5
    for key in clean:
        assert np.array_equal(_bits(clean[key].astype(np.float64))[keep], _bits(so[key].astype(np.float64))[keep]), key
    assert (so["info"][keep] == 0).all()


def test_dimension_above_the_limit_raises():
    """(30, 4): d = 104 > RIPTRM_TRS_DIM_MAX."""
    import rosenbrock
    from RIPTRM import RIPTRM
    n, k = 30, 4
    rs = np.random.RandomState(3)
    x, y = R.feasible_point(n, k, rs), np.ones(n * k)
    eng = _engine(n, k, 10.0)
    with pytest.raises(NotImplementedError):
        eng.second_order(x[None], y[None])
    X = torch.as_tensor(x.reshape(1, -1)).cuda()
    tol = torch.full((1,), 1e-5, dtype=torch.float64).cuda()
    out = torch.zeros(1, 7, dtype=torch.float64).cuda()
    rc = eng.lib.riptrm_gr_second_order(eng.ctx.h, ctypes.c_void_p(X.data_ptr()), ctypes.c_void_p(X.data_ptr()), n * k, None,
                                        1, ctypes.c_void_p(tol.data_ptr()), 0, 1e-12, 0, None,
                                        ctypes.c_void_p(out.data_ptr()))
    assert rc != 0
    with pytest.raises(RuntimeError, match="RIPTRM_TRS_DIM_MAX"):
        eng.ctx.check(rc, "riptrm_gr_second_order")
    opt = {"TRS_solver": "tCG", "second_order_stationarity": False, "manviofun": rosenbrock.manviofun,
           "tolresid": 0.0, "maxtime": 100.0, "maxiter": 2}
    prob = rosenbrock.RosenbrockProblem(n=n, k=k, alpha=10.0)
    with pytest.raises(NotImplementedError):
        RIPTRM(dict(opt, callbackfun=rosenbrock.callbackfun)).run(prob)
    out = RIPTRM(opt).run(prob)
    assert len(out.log["residual"]) > 1 and "second_order_residual" not in out.log


def _run(alphas, callback, log_capacity=None, **kw):
    import rosenbrock
    from RIPTRM import RIPTRM
    opt = {"TRS_solver": "tCG", "second_order_stationarity": False, "manviofun": rosenbrock.manviofun,
           "tolresid": 0.0, "maxtime": 100.0, "maxiter": 6}
    opt.update(kw)
    if callback:
        opt["callbackfun"] = rosenbrock.callbackfun
    solver = RIPTRM(opt)
    outs = solver.run_batch([rosenbrock.RosenbrockProblem(n=5, k=3, alpha=a) for a in alphas], log_capacity=log_capacity)
    return solver, outs


def _same(a, b):
    return [repr(v) for v in a] == [repr(v) for v in b]


def test_end_to_end_callback_columns():
    """The existing trajectory instances (5, 3), alpha 1e3 and 1e5, with and without the callback."""
    import rosenbrock
    alphas = [1e3, 1e5]
    solver, outs = _run(alphas, True)
    _, plain = _run(alphas, False)
    eng = solver.last_engine
    X, Y, inst, rows = eng.trail_points(solver.last_batch.stats)
    direct = rosenbrock.second_order_columns(eng.second_order(X, Y, inst=inst))
    X = X.cpu().numpy()
    at = 0
    for b, (o, q) in enumerate(zip(outs, plain)):
        L = len(o.log["residual"])
        assert rows[b] == L and len(o.log["second_order_residual"]) == L and len(o.log["condition_number"]) == L
        # the trail flag changes nothing else ("time" is the device's wall clock and differs run to run)
        assert [c for c in o.log if c not in ("second_order_residual", "condition_number")] == list(q.log)
        for col in q.log:
            if col != "time":
                assert _same(o.log[col], q.log[col]), (b, col)
        assert np.array_equal(_bits(o.x), _bits(q.x)) and np.array_equal(_bits(o.ineqLagmult), _bits(q.ineqLagmult))
        # every row's values are those of its own trail point, and that point is the row's
        for col in ("second_order_residual", "condition_number"):
            assert _same(o.log[col], direct[col][at:at + L]), (b, col)
        prob = rosenbrock.RosenbrockProblem(n=5, k=3, alpha=alphas[b])
        for r in range(L):
            c = float(o.log["cost"][r])
            assert abs(prob.cost(X[at + r]) - c) <= 1e-12 * max(1.0, abs(c)), (b, r)
        assert np.array_equal(_bits(X[at + L - 1].reshape(5, 3)), _bits(o.x))
        # row 0: the coordinator's start, no active constraint
        P = R.RosenbrockStructured(5, 3, alphas[b])
        x0, y0 = R.initial_point(5, 3)
        ref = S.sym_check(P, x0, y0, 1e-5)
        assert ref["nulldim"] == 6
        bar = S.bar_of(P, x0, y0)
        lo, cond = o.log["second_order_residual"][0], o.log["condition_number"][0]
        assert abs(lo - ref["mineig"]) <= bar, (lo, ref["mineig"], bar)
        assert abs(cond * lo - ref["maxeig"]) <= 2 * bar, (cond * lo, ref["maxeig"], bar)
        at += L


def test_trail_follows_the_log_ring_on_overflow():
    """log_capacity 16 on a run of more records: the columns belong to the kept head and ring rows."""
    import rosenbrock
    from engine import C
    cap = 16
    with pytest.warns(UserWarning, match="log capacity"):
        solver, outs = _run([1e3], True, log_capacity=cap)
    eng, st = solver.last_engine, solver.last_batch.stats
    count = int(st[0, C["RIPTRM_STAT_LOG_COUNT"]])
    assert count > cap and eng.cap == cap
    h = cap // 2
    t = cap - h
    order = list(range(h)) + [h + ((count - t - h + i) % t) for i in range(t)]   # head, then the ring from its oldest
    pts = eng.trail[0, torch.as_tensor(order).cuda()]
    direct = rosenbrock.second_order_columns(eng.second_order(pts[:, 0], pts[:, 1], inst=np.zeros(cap, dtype=np.int64)))
    log = outs[0].log
    assert len(log["residual"]) == cap
    for col in ("second_order_residual", "condition_number"):
        assert _same(log[col], direct[col]), col
    prob = rosenbrock.RosenbrockProblem(n=5, k=3, alpha=1e3)
    X = pts[:, 0].cpu().numpy()
    for r in range(cap):
        c = float(log["cost"][r])
        assert abs(prob.cost(X[r]) - c) <= 1e-12 * max(1.0, abs(c)), r
    assert np.array_equal(_bits(X[cap - 1].reshape(5, 3)), _bits(outs[0].x))
