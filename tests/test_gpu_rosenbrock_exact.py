"""GPU tests of Exact_RepMat for Rosenbrock on Grassmann(n, k) in the pinned frame (the EXACT instantiation of
csrc/riptrm_grassmann.hip, ``rosenbrock.basisfun``, ``RosenbrockBatch.exact_step``) against the unmodified CPU
oracle driven through tests/rosenbrock_exact.py::RosenbrockExact (the same frame from LAPACK's QR).

Shapes: (5, 3) d = 6 the reference's, (7, 1) k = 1 (a self-adjoint operator), (9, 8) k = KMAX and n - k = 1,
(13, 5) d = 40 on two waves, (16, 4) d = 48 on exactly one wave, and the largest shape the derived limit admits
(``riptrm_gr_exact_dim_max``: d = 91, (20, 7), three waves).

Bars.  Matrix entries: the second-order test's, 32 d eps scale (scale = 4 alpha + 2 + ||X^T G_L||_2 + max(y / s),
an upper bound of ||HwCur||), for the entries of the linear term too, which also meet 32 d eps
||egrad f - mu / S||_F, the backward-error statement for the inner product of that matrix with a unit vector (the
smaller of the two wherever that norm is below scale).  Teacher-forced direction, multiplier and smallest
eigenvalue: tests/test_gpu_trs.py's bars of the dim <= 96 unit parity, unchanged (same kind; boundary x within
1e-8 relative; interior: both pass the reference's acceptance test, agree to 1e-4 and in model value to 1e-8; lam1
within 1e-8 max(1, |lam1|); the eigenvalue within 1e-11 max(1, d max|A|)) against the reference's pencil
(exact_repmat_direction) and against the CPU statement of the device's formulation (trs_eigh) -- on rows where the
CPU order variants agree on the kind; all six shapes, every 3rd row at the largest.  The bars
transfer: measured, boundary steps are within 3.3e-13 (the CPU variants' own spread on these rows: up to 4.5e-13),
interior steps within 3.8e-7 (variants 4.7e-7), eigenvalues within 4.3e-13 absolute; the test prints each figure
next to the variants' spread.  Trajectories through tests/parity.py::compare_until_flip, unchanged, which compares
the dxtype strings and the mineigvalHw column; the instances are those on which the CPU's own variants stay inside
it (tests/rosenbrock_exact.py::TRAJECTORY_INSTANCES, tests/test_rosenbrock_exact.py), all six shapes: the largest
runs the solve on three waves with 160 KiB of dynamic LDS.  RIPTRM.py:670 expands the radius of a boundary step only
if |normdx - Delta| <= 1e-15, a coin flip between two fp64 implementations once Delta is 0.25 or more
(parity.is_radius_tie); from the eye start every instance meets such a step within its first five rows (Delta_0 =
sqrt(k) / 8).  Where the device flips there -- measured: row 1 at (13, 5) and (16, 4) -- compare_until_flip compares
the rows before the tie row by row and the run after it at the outer level only (same outer iterations and end
states, residuals within 1e-3 or 10 mu); the tie row itself has the same input on both sides, so its dxtype is
asserted too, and the row values at those shapes are what the teacher-forced test checks.

One frame: at k = 1 the smallest eigenvalue of this kernel's matrix and of the second-order kernel's (barrier term
on, no active constraint) agree within one bar per kernel (test_exact_and_second_order_kernels_share_one_frame).
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import rosenbrock_exact as X
import rosenbrock_oracle as R


def _engine(n, k, B, alpha, lb=R.LB, cap=1024):
    import rosenbrock
    return rosenbrock.RosenbrockBatch(n, k, B, log_capacity=cap).load(alpha, lb)


def _opt(**kw):
    import rosenbrock
    o = {"TRS_solver": "Exact_RepMat", "second_order_stationarity": True, "basisfun": rosenbrock.basisfun,
         "manviofun": rosenbrock.manviofun, "tolresid": 0.0, "maxtime": 100.0, "maxiter": 6, "inner_maxiter": 300}
    o.update(kw)
    return o


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _largest_shape():
    """The shape with the most columns whose manifold dimension is the limit."""
    import riptrm_native as N
    lib = N.load()
    d = int(lib.riptrm_gr_exact_dim_max())
    k = max(k for k in range(1, N.CONST["RIPTRM_GR_KMAX"] + 1) if d % k == 0 and (d // k + k) * k <= N.CONST["RIPTRM_GR_NKMAX"])
    return d // k + k, k, d


def test_the_limit_admits_dimension_80_and_the_largest_shape_fits():
    import riptrm_native as N
    lib = N.load()
    n, k, d = _largest_shape()
    assert (n, k) == X.LARGEST == X.SHAPES[-1]
    assert 80 <= d <= N.CONST["RIPTRM_TRS_DIM_MAX"]
    assert 0 < lib.riptrm_gr_exact_lds_bytes(n, k) <= 160 * 1024
    for kk in range(1, 9):   # every shape with k (n - k) <= 80 inside k <= 8, n k <= 512
        for nn in range(kk + 1, 512 // kk + 1):
            if kk * (nn - kk) <= 80:
                assert 0 < lib.riptrm_gr_exact_lds_bytes(nn, kk) <= 160 * 1024, (nn, kk)
    assert lib.riptrm_gr_exact_lds_bytes(d + 2, 1) == -1   # one past the limit


@pytest.mark.parametrize("shape", range(6))
def test_matrix_and_linear_term(shape):
    n, k = X.SHAPES[shape]
    d = k * (n - k)
    rs = np.random.RandomState(13 * n + k)
    alphas = np.array(X.ALPHAS * 2)
    B = len(alphas)
    mus = np.array([0.1, 0.1, 0.1, 1e-3, 1e-3, 1e-3])
    xs = np.stack([R.feasible_point(n, k, rs) for _ in range(B)])
    ys = 0.1 + rs.rand(B, n * k)
    out = _engine(n, k, B, alphas).exact_step(xs, ys, mus, np.full(B, 0.1))
    worst = 0.0
    for b in range(B):
        A, a = X.matrix_and_linear_term(n, k, alphas[b], xs[b], ys[b], mus[b])
        P = X.RosenbrockExact(n, k, alphas[b])
        unit = d * X.EPS * X.scale_of(n, k, alphas[b], xs[b], ys[b])
        unit_a = d * X.EPS * np.linalg.norm(P.egrad(xs[b]) - mus[b] / P.slack(xs[b]).reshape(n, k))
        eA, ea = np.max(np.abs(out["A"][b] - A)), np.max(np.abs(out["a"][b] - a))
        worst = max(worst, eA / unit, ea / unit_a)
        assert np.array_equal(out["A"][b], out["A"][b].T), b            # mirrored
        assert eA <= 32 * unit, (b, eA / unit)
        assert ea <= 32 * unit and ea <= 32 * unit_a, (b, ea / unit, ea / unit_a)
        assert out["passes"][b] == 3 * d                                 # the op builds the matrix three times
    print(f"({n}, {k}) d = {d}: worst entry error {worst:.3g} d eps scale")


def _pick(rows, count=8):
    picked = [next(r for r in rows if r["kind"] == "boundary"), next(r for r in rows if r["kind"] == "interior")]
    for r in rows[::3]:
        if len(picked) >= count:
            break
        if not any(r is p for p in picked):
            picked.append(r)
    return picked


def _obj(A, a, c):
    return 0.5 * c @ A @ c + a @ c


@pytest.mark.parametrize("n,k", X.SHAPES)
def test_direction_and_mineig_teacher_forced(n, k):
    """Inputs (x, y, mu, Delta) from the oracle's alpha = 100 trajectory, rows on which the CPU order variants
    agree on the kind (rosenbrock_exact.direction_rows)."""
    alpha = 100.0
    picked = _pick(X.direction_rows(n, k, alpha, X.ROW_STRIDE.get((n, k), 1)))
    assert {"boundary", "interior"} <= {r["kind"] for r in picked} and len(picked) >= 4
    B, d = len(picked), k * (n - k)
    out = _engine(n, k, B, alpha).exact_step(np.stack([r["x"] for r in picked]), np.stack([r["y"] for r in picked]),
                                             np.array([r["mu"] for r in picked]), np.array([r["Delta"] for r in picked]))
    for b, r in enumerate(picked):
        assert out["kind"][b] == r["kind"], (b, out["kind"][b], r["kind"])
        nref = np.linalg.norm(r["dx"])
        dev = np.linalg.norm(out["dx"][b] - r["dx"]) / nref
        spread = max(np.linalg.norm(v["dx"] - r["dx"]) for v in r["variants"]) / nref
        basis = X.frame(r["x"])
        c = np.array([np.sum(out["dx"][b] * q) for q in basis])
        cr = np.array([np.sum(r["dx"] * q) for q in basis])
        unit = 1e-4 if r["kind"] == "interior" else 1e-8
        print(f"direction ({n},{k}) row {b} {r['kind']}: device {dev:.2e}, CPU variants {spread:.2e}, unit bar {unit:g}, "
              f"device / variants {dev / max(spread, 1e-300):.3g}")
        assert dev <= unit, (b, r["kind"], dev, spread)
        # the CPU statement of the device's formulation, and TRSgep's multiplier against both
        dev_e = np.linalg.norm(out["dx"][b] - r["dx_eigh"]) / nref
        dl, dle = abs(out["lam1"][b] - r["lam1"]), abs(out["lam1"][b] - r["lam1_eigh"])
        print(f"   against trs_eigh {dev_e:.2e}; lam1 {out['lam1'][b]:.6g}: pencil {dl:.2e}, trs_eigh {dle:.2e}")
        assert dev_e <= unit, (b, r["kind"], dev_e)
        assert dl <= 1e-8 * max(1.0, abs(r["lam1"])) and dle <= 1e-8 * max(1.0, abs(r["lam1_eigh"])), (b, dl, dle)
        assert abs(np.linalg.norm(out["dx"][b]) - np.linalg.norm(c)) <= 1e-12 * nref   # horizontal: all of it in the frame
        if r["kind"] == "interior":   # both are CG iterates that pass the reference's acceptance test
            assert np.linalg.norm(r["H"] @ c + r["a"]) / np.linalg.norm(r["a"]) < 1e-5, b
            mo, mr = _obj(r["H"], r["a"], c), _obj(r["H"], r["a"], cr)
            assert abs(mo - mr) <= 1e-8 * abs(mr), (b, mo, mr)
        else:
            assert abs(np.linalg.norm(out["dx"][b]) - r["Delta"]) <= 1e-12 * r["Delta"], b
        em = abs(out["mineig"][b] - r["mineig"])
        sm = max(abs(v["mineig"] - r["mineig"]) for v in r["variants"])
        ubar = 1e-11 * max(1.0, np.abs(r["H"]).max() * d)
        print(f"   mineig {out['mineig'][b]:.6g}: device {em:.2e}, CPU variants {sm:.2e}, unit bar {ubar:.2e}")
        assert em <= ubar, (b, em, sm, ubar)


@pytest.fixture(scope="module")
def oracle_runs():
    return {(n, k, a): X.recorded_run(n, k, a)[0] for (n, k), al in X.TRAJECTORY_INSTANCES.items() for a in al}


@pytest.mark.parametrize("n,k", sorted(X.TRAJECTORY_INSTANCES))
def test_trajectories_match_oracle(n, k, oracle_runs):
    """One batch per shape: eye start, y0 = 1, maxiter 6 (2 at the largest shape), tolresid 0, Exact_RepMat with the second-order test,
    inner_maxiter 300 on both sides, through RIPTRM(option).run_batch."""
    import rosenbrock
    from parity import compare_until_flip, outer_rows
    from RIPTRM import RIPTRM
    alphas = X.TRAJECTORY_INSTANCES[(n, k)]
    maxiter = X.option_for(n, k)["maxiter"]   # 6, and 2 at the largest shape (rosenbrock_exact.TRAJECTORY_MAXITER)
    solver = RIPTRM(_opt(maxiter=maxiter))
    outs = solver.run_batch([rosenbrock.RosenbrockProblem(n, k, a) for a in alphas])
    d = k * (n - k)
    for b, (a, out) in enumerate(zip(alphas, outs)):
        ref = oracle_runs[(n, k, a)]
        print(f"trajectory ({n},{k}) alpha={a:g}: outer end states {[out.log['inner_status'][i] for i in outer_rows(out.log)]}, "
              f"{len(out.log['iteration'])} rows")
        flip = compare_until_flip(out.log, ref.log, tight_rows=20, late_row=20)
        rows = len(ref.log["iteration"]) if flip is None else flip[0]
        g = np.array([np.nan if v is None else v for v in out.log["mineigvalHw"][:rows]], dtype=float)
        r = np.array([np.nan if v is None else v for v in ref.log["mineigvalHw"][:rows]], dtype=float)
        dev = np.nanmax(np.abs(g - r) / np.maximum(np.abs(r), 1e-300)) if rows > 1 else 0.0
        print(f"trajectory ({n},{k}) alpha={a:g}: {len(out.log['iteration'])} rows (oracle {len(ref.log['iteration'])}), "
              f"first flip {flip}, mineigvalHw relative deviation before it {dev:.2e}")
        if flip is not None and flip[1] == "radius_update":   # a tie: that row's step had the same input
            rows += 1
        assert out.log["dxtype"][:rows] == ref.log["dxtype"][:rows]
        assert out.log["mineigvalHw"][0] is None and all(v is not None for v in out.log["mineigvalHw"][1:])
        it, st = out.log["iteration"], out.log["inner_status"]
        last = [st[i] for i in range(1, len(it)) if i == len(it) - 1 or it[i + 1] != it[i]]
        assert last == ["converged"] * maxiter, (a, last)
        assert np.max(np.abs(out.x.T @ out.x - np.eye(k))) <= 1e-12 and out.x.min() > -R.LB
        # counters as the StableIdentification Exact path reports them: no tCG iterations, d operator
        # applications per matrix (two matrices per step) and one for pred on the steps that reach it
        res = solver.last_batch
        inner = int(res.stat(b, "INNER_ITERS"))
        assert inner == len(it) - 1 and int(res.stat(b, "TCG_ITERS")) == 0
        reached = sum(s in ("successful", "unsuccessful") for s in st)
        assert int(res.stat(b, "PASSES")) == 2 * d * inner + reached


def test_interface_names_columns_and_errors():
    import rosenbrock
    from engine import C
    from RIPTRM import RIPTRM
    prob = rosenbrock.RosenbrockProblem(5, 3, 1e3)
    out = RIPTRM(_opt(maxiter=2)).run(prob)
    assert out.name == "RIPTRM_Exact_RepMat"
    assert set(out.log["dxtype"][1:]) <= {"boundary", "interior", "hardcase_1"}
    assert all(v is not None for v in out.log["mineigvalHw"][1:])
    off = RIPTRM(_opt(maxiter=2, second_order_stationarity=False)).run(prob)
    assert off.name == "RIPTRM_Exact_RepMat" and len(off.log["mineigvalHw"]) > 1
    assert all(v is None for v in off.log["mineigvalHw"])
    # without the pinned basis: today's error, naming the way in
    for bad in ({"basisfun": None}, {}):
        o = _opt(maxiter=2)
        del o["basisfun"]
        o.update(bad)
        with pytest.raises(NotImplementedError, match="Rosenbrock.*basisfun=rosenbrock.basisfun"):
            RIPTRM(o).run(prob)

    def drawn(manifold, x):   # the reference's default: a draw
        n, k = x.shape
        rs = np.random.RandomState(0)
        vs = []
        for _ in range(k * (n - k)):
            v = rs.randn(n, k)
            v = v - x @ (x.T @ v)
            for q in vs:
                v = v - np.sum(q * v) * q
            vs.append(v / np.linalg.norm(v))
        return vs

    with pytest.raises(NotImplementedError, match="Rosenbrock"):
        RIPTRM(_opt(maxiter=2, basisfun=drawn)).run(prob)
    with pytest.raises(NotImplementedError, match="Rosenbrock"):
        _engine(5, 3, 1, 1e3).solve(*[v[None] for v in R.initial_point(5, 3)], _opt(maxiter=2, basisfun=drawn))
    # an independent implementation of the frame is accepted
    same = RIPTRM(_opt(maxiter=2, basisfun=lambda manifold, x: X.frame(x))).run(prob)
    assert np.array_equal(_bits(same.x), _bits(out.x))
    # above the limit: (30, 4), d = 104
    n, k = 30, 4
    limit = int(_engine(5, 3, 1, 1.0).exact_dim_max())
    with pytest.raises(NotImplementedError, match=str(limit)):
        RIPTRM(_opt(maxiter=2)).run(rosenbrock.RosenbrockProblem(n, k, 10.0))
    eng = _engine(n, k, 1, 10.0)
    with pytest.raises(NotImplementedError, match=str(limit)):
        eng.exact_step(R.feasible_point(n, k, np.random.RandomState(1))[None], np.ones((1, n * k)), 0.1, 0.1)
    buf = torch.zeros(n * k * 2 + 16, dtype=torch.float64).cuda()
    p = ctypes.c_void_p(buf.data_ptr())
    rc = eng.lib.riptrm_gr_exact(eng.ctx.h, 1e-8, p, p, p, p, p, p, p, p, p, p)
    assert rc == C["RIPTRM_E_ARG"]
    ro = rosenbrock.resolve_options(_opt(maxiter=2), 2.0, eng.cap, manvio_classifier=rosenbrock.rosenbrock_manvio_kind)
    tabs = ro.device_tables(eng.device)
    rc = eng.lib.riptrm_gr_solve(eng.ctx.h, ctypes.byref(ro.c_opt), p, p, ctypes.c_void_p(tabs[0].data_ptr()),
                                 ctypes.c_void_p(tabs[1].data_ptr()), ctypes.c_void_p(tabs[2].data_ptr()), len(ro.mu_tab))
    assert rc == C["RIPTRM_E_ARG"]
    with pytest.raises(RuntimeError, match=str(limit)):
        eng.ctx.check(rc, "riptrm_gr_solve")


def test_batch_instance_equals_its_solo_run_bitwise():
    from engine import C
    alphas = np.array([1.0, 1e3, 1e7, 100.0])
    x0, y0 = R.initial_point(5, 3)
    xs, ys = np.stack([x0] * 4), np.stack([y0] * 4)
    res = _engine(5, 3, 4, alphas).solve(xs, ys, _opt())
    solo = _engine(5, 3, 1, alphas[2]).solve(xs[:1], ys[:1], _opt())
    cols = [c for c in range(C["RIPTRM_LOG_NFIELDS"]) if c != C["RIPTRM_LOG_TIME"]]
    assert len(res.raw_log[2]) > 10 and res.raw_log[2].shape == solo.raw_log[0].shape
    assert np.array_equal(_bits(res.raw_log[2][:, cols]), _bits(solo.raw_log[0][:, cols]))
    assert np.array_equal(_bits(res.x[2].cpu().numpy()), _bits(solo.x[0].cpu().numpy()))
    assert np.array_equal(_bits(res.y[2].cpu().numpy()), _bits(solo.y[0].cpu().numpy()))


def test_tcg_solve_ignores_basisfun_bitwise():
    import rosenbrock
    from engine import C
    alphas = np.array([1.0, 1e3])
    x0, y0 = R.initial_point(5, 3)
    xs, ys = np.stack([x0] * 2), np.stack([y0] * 2)
    o = _opt(TRS_solver="tCG", second_order_stationarity=False)
    with_b = _engine(5, 3, 2, alphas).solve(xs, ys, o)
    del o["basisfun"]
    without = _engine(5, 3, 2, alphas).solve(xs, ys, o)
    cols = [c for c in range(C["RIPTRM_LOG_NFIELDS"]) if c != C["RIPTRM_LOG_TIME"]]
    for b in range(2):
        assert np.array_equal(_bits(with_b.raw_log[b][:, cols]), _bits(without.raw_log[b][:, cols]))
    assert np.array_equal(_bits(with_b.x.cpu().numpy()), _bits(without.x.cpu().numpy()))


def test_exact_with_the_second_order_callback():
    """The trail flag is orthogonal to the Exact path: both callback columns on every row, every other
    column as without the callback."""
    import rosenbrock
    from RIPTRM import RIPTRM
    probs = [rosenbrock.RosenbrockProblem(5, 3, a) for a in (1e3, 1e7)]
    plain = RIPTRM(_opt()).run_batch(probs)
    solver = RIPTRM(_opt(callbackfun=rosenbrock.callbackfun))
    outs = solver.run_batch(probs)
    eng = solver.last_engine
    Xp, Yp, inst, rows = eng.trail_points(solver.last_batch.stats)
    direct = rosenbrock.second_order_columns(eng.second_order(Xp, Yp, inst=inst))
    at = 0
    for o, q, r in zip(outs, plain, rows):
        L = len(o.log["residual"])
        assert r == L == len(q.log["residual"])
        for col in ("second_order_residual", "condition_number"):
            assert len(o.log[col]) == L
            assert [repr(v) for v in o.log[col]] == [repr(v) for v in direct[col][at:at + L]], col
        assert all(v is not None for v in o.log["second_order_residual"])
        for col in q.log:
            if col != "time":
                assert [repr(v) for v in o.log[col]] == [repr(v) for v in q.log[col]], col
        assert np.array_equal(_bits(o.x), _bits(q.x))
        at += L


def test_nonfinite_instance_stops_alone():
    """In a solve: one instance of four starts infeasible and stops with its own error code while the other
    three are bit-identical to the same solves without it.  In the operator entry: an infinite multiplier
    makes one instance's matrix non-finite; it reports RIPTRM_TCG_NONFINITE and a zero direction, the others'
    outputs keep their bits."""
    from engine import C
    alphas = np.array([1.0, 100.0, 1e3, 1e7])
    x0, y0 = R.initial_point(5, 3)
    xs, ys = np.stack([x0] * 4), np.stack([y0] * 4)
    xs[2, 4, 2] = -0.02
    res = _engine(5, 3, 4, alphas).solve(xs, ys, _opt())
    keep = [0, 1, 3]
    alone = _engine(5, 3, 3, alphas[keep]).solve(xs[keep], ys[keep], _opt())
    assert int(res.stat(2, "ERROR")) == C["RIPTRM_ERR_NONFINITE"] and res.error(2) is not None
    assert np.array_equal(res.x[2].cpu().numpy(), xs[2])
    cols = [c for c in range(C["RIPTRM_LOG_NFIELDS"]) if c != C["RIPTRM_LOG_TIME"]]
    for i, b in enumerate(keep):
        assert int(res.stat(b, "ERROR")) == C["RIPTRM_ERR_NONE"]
        assert res.raw_log[b].shape == alone.raw_log[i].shape and len(res.raw_log[b]) > 10
        assert np.array_equal(_bits(res.raw_log[b][:, cols]), _bits(alone.raw_log[i][:, cols]))
        assert np.array_equal(_bits(res.x[b].cpu().numpy()), _bits(alone.x[i].cpu().numpy()))
    # the new branch of the solve: a feasible start whose multiplier 1e308 sits on a slack of 0.01, where a frame
    # vector is +-1.  The residual at the outer head is inf (not NaN), the log barrier and ||c|| are finite, so the
    # instance reaches the direction; (y o P_X V) / s overflows, the matrix has an infinite entry, and the instance
    # stops there -- after the d = 6 operator applications of that one matrix -- while the others keep their bits
    ys2 = np.stack([y0] * 4)
    ys2[1, 14] = 1e308
    xs2 = np.stack([x0] * 4)
    res2 = _engine(5, 3, 4, alphas).solve(xs2, ys2, _opt())
    ref2 = _engine(5, 3, 3, alphas[[0, 2, 3]]).solve(xs2[:3], np.stack([y0] * 3), _opt())
    assert int(res2.stat(1, "ERROR")) == C["RIPTRM_ERR_NONFINITE"] and res2.error(1) is not None
    assert int(res2.stat(1, "PASSES")) == 6 and int(res2.stat(1, "INNER_ITERS")) == 0
    assert np.array_equal(res2.x[1].cpu().numpy(), x0) and np.array_equal(res2.y[1].cpu().numpy(), ys2[1])
    for i, b in enumerate([0, 2, 3]):
        assert int(res2.stat(b, "ERROR")) == C["RIPTRM_ERR_NONE"]
        assert np.array_equal(_bits(res2.raw_log[b][:, cols]), _bits(ref2.raw_log[i][:, cols]))
        assert np.array_equal(_bits(res2.x[b].cpu().numpy()), _bits(ref2.x[i].cpu().numpy()))
    rs = np.random.RandomState(2)
    pts = np.stack([R.feasible_point(5, 3, rs) for _ in range(4)])
    yy = 0.5 + rs.rand(4, 15)
    eng = _engine(5, 3, 4, alphas)
    clean = eng.exact_step(pts, yy, 0.1, 0.2)
    yb = yy.copy()
    yb[1, 7] = np.inf
    out = eng.exact_step(pts, yb, 0.1, 0.2)
    assert out["kind_code"][1] == C["RIPTRM_TCG_NONFINITE"] and not out["dx"][1].any() and np.isnan(out["mineig"][1])
    for key in ("A", "a", "dx", "lam1", "mineig", "kind_code"):
        for b in (0, 2, 3):
            assert np.array_equal(_bits(np.asarray(out[key][b], dtype=np.float64)),
                                  _bits(np.asarray(clean[key][b], dtype=np.float64))), (key, b)


@pytest.mark.parametrize("n,k", [(4, 1), (7, 1)])
def test_exact_and_second_order_kernels_share_one_frame(n, k):
    """k_gr_exact and k_gr_so take the frame from one definition (csrc/riptrm_grassmann_ops.h).  With k = 1,
    X^T G_L is a number and HwCur is self-adjoint, so the mirrored upper triangle (exact_step) and the symmetrised
    matrix (second_order with barrier=True) are one matrix up to rounding, and with no active constraint their
    smallest eigenvalues agree.  Bar: each kernel is held to bar_of (32 d eps scale) against its own CPU statement,
    so the two differ by 2 bar_of at most; on the CPU, in the basisfun frame, the two statements differ by at most
    0.013 of one such bar.  Measured on the MI355X: worst 0.0022 of the 2 bar_of bar at (4, 1), 0.0012 at (7, 1)."""
    import rosenbrock_second_order as S
    rs = np.random.RandomState(100 * n + k)
    alphas = np.repeat(S.ALPHAS, 4)
    B = len(alphas)
    xs = np.stack([R.feasible_point(n, k, rs) for _ in range(B)])
    ys = 0.1 + rs.rand(B, n * k)
    mus = np.full(B, S.MU)
    eng = _engine(n, k, B, alphas)
    ex = eng.exact_step(xs, ys, mus, np.full(B, 0.1))
    so = eng.second_order(xs, ys, barrier=True, mu=mus)
    worst = 0.0
    for b in range(B):
        bar = 2 * S.bar_of(R.RosenbrockStructured(n, k, alphas[b]), xs[b], ys[b], barrier=True)
        err = abs(ex["mineig"][b] - so["mineig"][b])
        worst = max(worst, err / bar)
        print(f"({n}, {k}) alpha={alphas[b]:g}: exact {ex['mineig'][b]:.17g}, second order {so['mineig'][b]:.17g}, "
              f"difference {err:.3g} = {err / bar:.3g} of the bar {bar:.3g}")
        assert so["info"][b] == 0 and so["nactive"][b] == 0, (b, so["nactive"][b])
        assert err <= bar, (b, err, bar)
    print(f"({n}, {k}): worst difference {worst:.3g} of 2 bar_of")
