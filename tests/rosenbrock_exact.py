"""CPU side of Exact_RepMat for Rosenbrock on Grassmann(n, k) -- TEST INFRASTRUCTURE ONLY.

``RosenbrockExact`` is ``rosenbrock_oracle.RosenbrockVectorized`` plus ``tangent_basis(x)``, the pinned
frame, and nothing else: the unmodified ``oracle.riptrm_oracle.RIPTRMOracle`` calls ``P.tangent_basis`` on
its Exact_RepMat path.  The frame here is LAPACK's Householder QR through numpy, an implementation
independent of ``rosenbrock.basisfun``: column k + a of the complete Q times e_b^T, vector a k + b.
"""
from __future__ import annotations

import functools

import numpy as np

import rosenbrock_oracle as R
from oracle.riptrm_oracle import RIPTRMOracle

EPS = np.finfo(np.float64).eps
# the shapes of the GPU tests: (5, 3) the reference's, (7, 1) k = 1 (a self-adjoint operator), (9, 8) k = KMAX
# and n - k = 1, (13, 5) d = 40 on two waves, (16, 4) d = 48 on exactly one wave
# and LARGEST, the largest shape the derived limit admits: d = 91 = riptrm_gr_exact_dim_max(), three waves,
# 163,640 B of LDS (the GPU tests check that the library's limit gives this shape)
LARGEST = (20, 7)
SHAPES = [(5, 3), (7, 1), (9, 8), (13, 5), (16, 4), LARGEST]
# teacher-forced rows looked at per shape: every row, except every 3rd at the largest shape
ROW_STRIDE = {LARGEST: 3}
ALPHAS = [1.0, 1e3, 1e7]
# trajectory instances: eye start, y0 = 1, Exact_RepMat with the second-order test; inner_maxiter bounds the
# inner loop on both sides (with the fixed clock the oracle's has no other bound).  Chosen on the CPU: on each
# the oracle's own variants (order_variants: three rounding orders and the other CPU form of TRSgep) stay
# inside tests/parity.py::compare_until_flip (tests/test_rosenbrock_exact.py).  (5, 3) at alpha = 1e7 is not
# among them: there the two CPU forms of TRSgep part (UNCALIBRATED below).
TRAJECTORY_INSTANCES = {(5, 3): [1.0, 1e3, 1e6], (7, 1): [100.0, 1e7], (9, 8): [100.0], (13, 5): [100.0],
                        (16, 4): [100.0], LARGEST: [100.0]}
# matrices of condition 3e4 .. 4e6: the pencil's boundary steps are 1e-6 .. 1e-5 from the eigendecomposition's
# on three early rows, an interior CG step (rtol 1e-5) then moves by 2e-3, and with it the radius gamma ||dx||
UNCALIBRATED = (5, 3, 1e7)
TRAJECTORY_OPTION = dict(maxiter=6, tolresid=0.0, maxtime=1e9, TRS_solver="Exact_RepMat",
                         second_order_stationarity=True, inner_maxiter=300)
# Outer iterations per shape (default 6).  RIPTRM.py:670 expands the radius of a boundary step only if
# |normdx - Delta| <= 1e-15: at Delta_0 = sqrt(k) / 8 >= 0.2 that is a coin flip between two fp64 implementations
# (parity.is_radius_tie), and row 1 of every instance is such a step.  With the tie of row 1 taken the other way
# (solve_tie_flipped) the CPU oracle itself stays inside compare_until_flip on every instance -- except at the
# largest shape from its third outer iteration on, which then runs into inner_maxiter (412 rows against 97).  So
# that shape runs two outer iterations.
TRAJECTORY_MAXITER = {LARGEST: 2}


def option_for(n, k):
    return dict(TRAJECTORY_OPTION, maxiter=TRAJECTORY_MAXITER.get((n, k), TRAJECTORY_OPTION["maxiter"]))


def frame(x):
    """The pinned frame from numpy's (LAPACK's) complete QR."""
    n, k = x.shape
    Q = np.linalg.qr(x, mode="complete")[0]
    eye = np.eye(k)
    return [np.outer(Q[:, k + a], eye[b]) for a in range(n - k) for b in range(k)]


class RosenbrockExact(R.RosenbrockVectorized):
    def tangent_basis(self, x):
        return frame(x)


def solve(n, k, alpha, option=None, manifold=None, lb=R.LB):
    """One oracle run from the coordinator's start under the fixed clock."""
    x0, y0 = R.initial_point(n, k)
    P = RosenbrockExact(n, k, alpha, lb, manifold)
    return RIPTRMOracle(R._option(k, option or option_for(n, k)), clock=R.fixed_clock).run(P, x0, y0)


class _TieFlipped(R.Grassmann):
    """The second norm the oracle takes is ||dx|| of its first step (the first is the gradient's at the outer
    head): 1e-14 relative on it turns the radius-expansion tie of row 1 the other way, nothing else."""
    calls = 0

    def norm(self, x, v):
        self.calls += 1
        r = super().norm(x, v)
        return r * (1 + 1e-14) if self.calls == 2 else r


def solve_tie_flipped(n, k, alpha, option=None):
    return solve(n, k, alpha, option, manifold=_TieFlipped(n, k, polar="gram"))


def solve_eigh_form(n, k, alpha, option=None):
    """The same oracle run with TRSgep in its other CPU form: ``oracle.trs_oracle.trs_eigh`` (the symmetric
    eigendecomposition and the secular equation, what csrc/riptrm_trs.h implements) in place of the pencil's
    rightmost eigenpair.  The two forms solve the same subproblem; on an ill-conditioned matrix the pencil's
    QZ leaves them 1e-6..1e-5 apart in a boundary step (tests/test_trs_oracle.py pins 1e-8 on its cases)."""
    from oracle import trs_oracle as T
    pencil = T.trs_gep
    T.trs_gep = lambda A, a, Del, tolhardcase=1e-4: T.trs_eigh(A, a, Del, tolhardcase)
    try:
        return solve(n, k, alpha, option)
    finally:
        T.trs_gep = pencil


def order_variants(n, k, alpha, option=None, seeds=(1, 2, 3)):
    """The CPU's own variants of one run: the same arithmetic in another rounding order (three seeds), the
    other CPU form of TRSgep, and the radius-expansion tie of row 1 taken the other way."""
    return [solve(n, k, alpha, option, manifold=R.Grassmann(n, k, polar="gram", perm_seed=s, assoc_xxt=True))
            for s in seeds] + [solve_eigh_form(n, k, alpha, option), solve_tie_flipped(n, k, alpha, option)]


def matrix_and_linear_term(n, k, alpha, x, y, mu, lb=R.LB, manifold=None):
    """(A, a): selfadj_operator2matrix of HwCur and the coordinates of cxCur in the helper frame."""
    from oracle.trs_oracle import selfadj_operator2matrix
    P = RosenbrockExact(n, k, alpha, lb, manifold)
    _, _, Hw, c = P.begin_inner(x, y, mu)
    basis = P.tangent_basis(x)
    A = selfadj_operator2matrix(P.manifold, x, Hw, basis)
    a = np.array([P.manifold.inner_product(x, c, b) for b in basis])
    return A, a


def scale_of(n, k, alpha, x, y, lb=R.LB):
    """The second-order test's upper bound of ||HwCur|| (rosenbrock_second_order.scale_of, barrier = True)."""
    import rosenbrock_second_order as S
    return S.scale_of(R.RosenbrockStructured(n, k, alpha, lb), x, y, barrier=True)


class _Recording(RosenbrockExact):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.starts = []

    def begin_inner(self, x, y, mu):
        self.starts.append((x.copy(), y.copy(), mu))
        return super().begin_inner(x, y, mu)


@functools.lru_cache(maxsize=None)
def recorded_run(n, k, alpha):
    """(the oracle's run on a trajectory instance, the (x, y, mu) of every inner step), computed once and
    shared by the trajectory and the teacher-forced tests.  Treat the result as read-only."""
    P = _Recording(n, k, alpha)
    orc = RIPTRMOracle(R._option(k, option_for(n, k)), clock=R.fixed_clock)
    x0, y0 = R.initial_point(n, k)
    res = orc.run(P, x0, y0)
    # with the second-order test every step calls begin_inner twice (the step, then the trial point)
    starts = P.starts[0::2]
    assert len(starts) == len(orc.trace) == len(res.log["iteration"]) - 1
    return res, starts, [rec["Delta"] for rec in orc.trace]


@functools.lru_cache(maxsize=None)
def direction_rows(n, k, alpha, stride=1, seeds=(1, 2, 3)):
    """Teacher-forcing inputs from the oracle's trajectory: per inner step its (x, y, mu, Delta), the
    reference direction, multiplier and kind (exact_repmat_direction: the pencil), the device formulation's
    (trs_eigh) and the smallest eigenvalue (scipy.linalg.eigh), and the same from the order variants -- only
    the steps on which every variant agrees on the kind.  stride > 1 looks at every stride-th step and at the
    first step of each kind only (the largest shape: the pencil of order 2 d four times per step is the cost).
    Treat the result as read-only."""
    import scipy.linalg
    from oracle.trs_oracle import exact_repmat_direction, trs_eigh
    res, starts, deltas = recorded_run(n, k, alpha)
    kinds = res.log["dxtype"][1:]
    look = set(range(0, len(starts), stride)) | {kinds.index(q) for q in ("boundary", "interior") if q in kinds}
    rows = []
    for i in sorted(look):
        (x, y, mu), Delta = starts[i], deltas[i]
        outs = []
        for man in [None] + [R.Grassmann(n, k, polar="gram", perm_seed=s, assoc_xxt=True) for s in seeds]:
            Q = RosenbrockExact(n, k, alpha, R.LB, man)
            _, _, Hw, c = Q.begin_inner(x, y, mu)
            basis = Q.tangent_basis(x)
            dx, lam1, kind, H = exact_repmat_direction(Q.manifold, x, Hw, c, Delta, basis, 1e-8)
            a = np.array([Q.manifold.inner_product(x, c, b) for b in basis])
            ce, le, ke = trs_eigh(H, a, Delta, 1e-8)
            outs.append(dict(dx=dx, lam1=lam1, kind=kind, H=H, a=a, kind_eigh=ke, lam1_eigh=le,
                             dx_eigh=sum(ci * bi for ci, bi in zip(ce, basis)),
                             mineig=scipy.linalg.eigh(H, eigvals_only=True)[0]))
        if all(o["kind"] == outs[0]["kind"] and o["kind_eigh"] == outs[0]["kind"] for o in outs):
            rows.append(dict(x=x, y=y, mu=mu, Delta=Delta, variants=outs[1:], **outs[0]))
    return rows
