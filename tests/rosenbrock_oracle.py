"""CPU oracle for the Rosenbrock problem on Grassmann(n, k) -- TEST INFRASTRUCTURE ONLY.

The reference's third experiment (``src/Rosenbrock/coordinator.py:33-95``): X is n x k with
X^T X = I, v = X.flatten() (row-major, N = n k entries),

    f(X) = sum_{i < N-1} alpha (v_{i+1} - v_i)^2 + (1 - v_i)^2          (:45-51)
    g_i(X) = -v_i - lb <= 0 for every entry, lb = 0.01                  (:55-71)

started at X0 = I[:, :k], y0 = ones(N) (:78-91).  The control flow is the unmodified
``oracle.riptrm_oracle.RIPTRMOracle``; this module supplies the manifold and two problem back-ends
with the interface that class consumes (``manifold``, ``cost``, ``slack``, ``gradlag``,
``begin_inner``, ``dy``, ``residual``, ``maxmeanviolations``):

* ``RosenbrockStructured`` follows the coordinator literally: the cost as the loop, one constraint
  at a time, the Lagrangian's Hessian as rhess f + sum_i y_i rhess g_i through pymanopt's
  ehess -> rhess, the polar retraction from numpy's SVD;
* ``RosenbrockVectorized`` is the closed form, the op-for-op twin of ``csrc/riptrm_grassmann.hip``:
  f is quadratic with the constant tridiagonal Hessian T, egrad f = T v - 2 (1, .., 1, 0), and with
  Y the multipliers as n x k, G_L = egrad f - Y:

      Hw(V) = P_X(T V + (Y o P_X(V)) / S) - V (X^T G_L)
      c     = P_X(egrad f - mu / S)
      dy    = -y + mu / s - y o vec(P_X(dx)) / s

Manifold formulas are pymanopt 2.x's ``Grassmann`` restated (Euclidean metric on horizontal
vectors); like the other oracles here, parity with the reference's own iterates is unpinned at
that boundary (the reference cannot run in this environment).
"""
from __future__ import annotations

import math
import time

import numpy as np

from oracle.riptrm_oracle import RIPTRMOracle

LB = 0.01


class Grassmann:
    """pymanopt.manifolds.Grassmann(n, k), one subspace.

    polar: 'svd' = pymanopt's retraction (u @ vt of the thin SVD of X + U); 'gram' = the kernel's
    (A V L^-1/2 V^T from the eigendecomposition G = A^T A = V L V^T): the same polar factor.
    perm_seed / assoc_xxt give an order variant: inner products summed in a seeded permutation and
    the projection associated as (X X^T) U -- the same arithmetic in another rounding order."""

    def __init__(self, n: int, k: int, polar: str = "svd", perm_seed=None, assoc_xxt: bool = False):
        self.n, self.k = int(n), int(k)
        self.dim = self.k * (self.n - self.k)
        self.typical_dist = math.sqrt(self.k)
        self.polar = polar
        self.assoc_xxt = bool(assoc_xxt)
        self.perm = None if perm_seed is None else np.random.RandomState(perm_seed).permutation(self.n * self.k)

    def inner_product(self, x, u, v):
        if self.perm is not None:
            w = (u * v).ravel()[self.perm]
            acc = 0.0
            for t in w:
                acc += t
            return acc
        return np.tensordot(u, v, axes=u.ndim)

    def norm(self, x, v):
        if self.perm is not None:
            return np.sqrt(self.inner_product(x, v, v))
        return np.linalg.norm(v)

    def projection(self, x, u):
        if self.assoc_xxt:
            return u - (x @ x.T) @ u
        return u - x @ (x.T @ u)

    to_tangent_space = projection

    def zero_vector(self, x):
        return np.zeros_like(x)

    def retraction(self, x, v):
        a = x + v
        if self.polar == "gram":
            lam, V = np.linalg.eigh(a.T @ a)
            return a @ ((V / np.sqrt(lam)) @ V.T)
        u, _, vt = np.linalg.svd(a, full_matrices=False)
        return u @ vt

    def dist(self, a, b):
        s = np.linalg.svd(a.T @ b, compute_uv=False)
        s = np.minimum(s, 1.0)
        return np.linalg.norm(np.arccos(s))

    def euclidean_to_riemannian_gradient(self, x, g):
        return self.projection(x, g)

    def euclidean_to_riemannian_hessian(self, x, egrad, ehess, v):
        return self.projection(x, ehess) - v @ (x.T @ egrad)


def rank_manvio(k: int):
    """src/Rosenbrock/simulator.py:107-114 as the oracle's one-argument manviofun."""
    return lambda x: 0 if np.linalg.matrix_rank(x) == k else np.inf


def initial_point(n: int, k: int):
    """coordinator.py:78-91."""
    return np.abs(np.eye(n)[:, :k]), np.ones(n * k)


class RosenbrockStructured:
    """The coordinator taken literally (+ utils.py:33-203 wrappers, RIPTRM.py:475-571 helpers)."""
    gpu_pass_accounting = False

    def __init__(self, n: int, k: int, alpha: float, lb: float = LB, manifold: Grassmann | None = None):
        self.n, self.k, self.alpha, self.lb = int(n), int(k), float(alpha), float(lb)
        self.N = self.n * self.k
        self.manifold = manifold or Grassmann(n, k, polar="svd")
        M = self.manifold
        N, shape = self.N, (self.n, self.k)
        alpha = self.alpha

        def cost(point):   # coordinator.py:45-51
            v = point.flatten()
            val = 0
            for i in range(N - 1):
                val = val + alpha * (v[i + 1] - v[i]) ** 2 + (1 - v[i]) ** 2
            return val

        def egrad(point):   # the derivative of that loop, term by term
            v = point.flatten()
            g = np.zeros(N)
            for i in range(N - 1):
                d = v[i + 1] - v[i]
                g[i] += -2 * alpha * d - 2 * (1 - v[i])
                g[i + 1] += 2 * alpha * d
            return g.reshape(shape)

        def ehess(point, u):
            w = u.flatten()
            h = np.zeros(N)
            for i in range(N - 1):
                d = w[i + 1] - w[i]
                h[i] += -2 * alpha * d + 2 * w[i]
                h[i + 1] += 2 * alpha * d
            return h.reshape(shape)

        self.cost = cost
        self.euclidean_gradient = egrad
        self.euclidean_hessian = ehess
        self.riemannian_gradient = lambda x: M.euclidean_to_riemannian_gradient(x, egrad(x))
        self.riemannian_hessian = lambda x, v: M.euclidean_to_riemannian_hessian(x, egrad(x), ehess(x, v), v)

        def mk(i):   # coordinator.py:58-63
            e = np.zeros(N)
            e[i] = -1.0
            e = e.reshape(shape)
            g = lambda x: -x.flatten()[i] - self.lb
            eg = lambda x: e.copy()
            eh = lambda x, v: np.zeros(shape)
            rg = lambda x: M.euclidean_to_riemannian_gradient(x, eg(x))
            rh = lambda x, v: M.euclidean_to_riemannian_hessian(x, eg(x), eh(x, v), v)
            return g, eg, eh, rg, rh

        cons = [mk(i) for i in range(N)]
        self.ineq = [c[0] for c in cons]
        self.ineq_rgrad = [c[3] for c in cons]
        self.ineq_rhess = [c[4] for c in cons]

    def slack(self, x):
        return np.array([-g(x) for g in self.ineq])

    def gradlag(self, x, y):   # RIPTRM.py:475-489
        vec = self.riemannian_gradient(x)
        gv = [-grad(x) for grad in self.ineq_rgrad]
        for i in range(len(y)):
            vec = vec - y[i] * gv[i]
        return vec

    def hesslag(self, x, y, dx):   # RIPTRM.py:491-523
        vec = self.riemannian_hessian(x, dx)
        hv = [-h(x, dx) for h in self.ineq_rhess]
        for i in range(len(y)):
            vec = vec - y[i] * hv[i]
        return vec

    def Gx(self, x, v):   # RIPTRM.py:525-551
        gv = [-grad(x) for grad in self.ineq_rgrad]
        vec = self.manifold.zero_vector(x)
        for idx in range(len(gv)):
            vec = vec + v[idx] * gv[idx]
        return vec

    def Gxaj(self, x, dx):   # RIPTRM.py:553-571
        gv = [-grad(x) for grad in self.ineq_rgrad]
        return np.array([self.manifold.inner_product(x, g, dx) for g in gv])

    def begin_inner(self, x, y, mu):   # RIPTRM.py:724-730
        cx = self.cost(x)
        s = self.slack(x)
        gradcostx = self.riemannian_gradient(x)
        Hw = lambda dx: self.hesslag(x, y, dx) + self.Gx(x, (y * self.Gxaj(x, dx)) / s)
        c = gradcostx - self.Gx(x, mu / s)
        return cx, s, Hw, c

    def dy(self, x, y, s, mu, dx):   # RIPTRM.py:743
        return -y + mu * (1 / s) - y * self.Gxaj(x, dx) / s

    def residual(self, x, y, manviofun):   # utils.py:269-340
        M = self.manifold
        vec = self.riemannian_gradient(x)
        for i in range(self.N):
            vec = vec + y[i] * self.ineq_rgrad[i](x)
        gradnorm = M.norm(x, vec)
        sq_compl = 0
        for i in range(self.N):
            sq_compl += (y[i] * self.ineq[i](x)) ** 2
        sq_nonneg = 0
        for v in y:
            sq_nonneg += max(-v, 0) ** 2
        sq_ineq = 0
        for i in range(self.N):
            sq_ineq += max(self.ineq[i](x), 0) ** 2
        manvio = manviofun(x)
        residual = np.sqrt(gradnorm ** 2 + sq_compl + sq_nonneg + sq_ineq + 0 + manvio ** 2)
        return residual, gradnorm, np.sqrt(sq_compl), np.sqrt(sq_nonneg), manvio

    def maxmeanviolations(self, x):   # utils.py:237-267
        mx = 0
        mean = 0
        for i in range(self.N):
            v = max(self.ineq[i](x), 0)
            mx = max(mx, v)
            mean += v
        return mx, mean / self.N


class RosenbrockVectorized:
    """The closed forms: every formula below is the one csrc/riptrm_grassmann.hip evaluates."""
    gpu_pass_accounting = False

    def __init__(self, n: int, k: int, alpha: float, lb: float = LB, manifold: Grassmann | None = None):
        self.n, self.k, self.alpha, self.lb = int(n), int(k), float(alpha), float(lb)
        self.N = self.n * self.k
        self.shape = (self.n, self.k)
        self.manifold = manifold or Grassmann(n, k, polar="gram")
        self.two = np.full(self.N, 2.0)
        self.two[-1] = 0.0

    def Tu(self, u):
        """The constant Euclidean Hessian of f on an n x k matrix."""
        w = u.ravel()
        d = w[1:] - w[:-1]
        acc = np.zeros(self.N)
        acc[:-1] = -2.0 * self.alpha * d + 2.0 * w[:-1]
        acc[1:] = acc[1:] + 2.0 * self.alpha * d
        return acc.reshape(self.shape)

    def egrad(self, x):
        return self.Tu(x) - self.two.reshape(self.shape)

    def cost(self, x):
        v = x.ravel()
        d = v[1:] - v[:-1]
        o = 1.0 - v[:-1]
        return np.sum(self.alpha * d * d + o * o)

    def slack(self, x):
        return x.ravel() + self.lb

    def gradlag(self, x, y):
        return self.manifold.projection(x, self.egrad(x) - y.reshape(self.shape))

    def begin_inner(self, x, y, mu):
        M = self.manifold
        cx = self.cost(x)
        s = self.slack(x)
        S = s.reshape(self.shape)
        Y = y.reshape(self.shape)
        ef = self.egrad(x)
        MG = x.T @ (ef - Y)

        def Hw(V):
            PV = M.projection(x, V)
            W = self.Tu(V) + (Y * PV) / S
            return M.projection(x, W) - V @ MG

        c = M.projection(x, ef - mu / S)
        return cx, s, Hw, c

    def dy(self, x, y, s, mu, dx):
        return -y + mu * (1 / s) - y * self.manifold.projection(x, dx).ravel() / s

    def residual(self, x, y, manviofun):
        gradnorm = self.manifold.norm(x, self.gradlag(x, y))
        g = -x.ravel() - self.lb
        compl = y * g
        sq_compl = compl @ compl
        neg = np.maximum(-y, 0)
        sq_nonneg = neg @ neg
        iv = np.maximum(g, 0)
        sq_ineq = iv @ iv
        manvio = manviofun(x)
        residual = np.sqrt(gradnorm ** 2 + sq_compl + sq_nonneg + sq_ineq + 0 + manvio ** 2)
        return residual, gradnorm, np.sqrt(sq_compl), np.sqrt(sq_nonneg), manvio

    def maxmeanviolations(self, x):
        iv = np.maximum(-x.ravel() - self.lb, 0)
        return max(0.0, iv.max()), iv.sum() / self.N


def _option(k, option):
    o = dict(manviofun=rank_manvio(k))
    o.update(option or {})
    return o


def solve(n, k, alpha, x0=None, y0=None, option=None, structured=False, clock=time.time, lb=LB, manifold=None):
    """One RIPTRM (tCG) run of the unmodified RIPTRMOracle; x0 / y0 default to the coordinator's."""
    xi, yi = initial_point(n, k)
    x0 = xi if x0 is None else np.asarray(x0, dtype=np.float64)
    y0 = yi if y0 is None else np.asarray(y0, dtype=np.float64)
    P = (RosenbrockStructured if structured else RosenbrockVectorized)(n, k, alpha, lb, manifold)
    return RIPTRMOracle(_option(k, option), clock=clock).run(P, x0, y0)


def order_variants(n, k, alpha, x0=None, y0=None, option=None, seeds=(1, 2, 3), clock=time.time, lb=LB):
    """Oracle runs that are the same arithmetic in another rounding order: inner products summed in
    a seeded permutation, the projection associated as (X X^T) U."""
    return [solve(n, k, alpha, x0, y0, option, clock=clock, lb=lb,
                  manifold=Grassmann(n, k, polar="gram", perm_seed=s, assoc_xxt=True)) for s in seeds]


# ---- shared test inputs ---------------------------------------------------------------------------
# The trajectory instances (eye start, y0 = 1, maxiter 6, tolresid 0, tCG): the reference's own rounding
# variants stay inside tests/parity.py::compare_until_flip on them
# (tests/test_rosenbrock_oracle.py::test_order_variants_stay_within_the_trajectory_bar).  One batch per
# shape on the GPU; the extra ones are calibrated on the CPU only.
TRAJECTORY_INSTANCES = {(5, 3): [1.0, 10.0, 100.0, 1e3, 1e5, 1e6, 1e7], (16, 4): [1.0, 100.0, 1e3]}
TRAJECTORY_EXTRA = [(8, 3, 100.0), (16, 8, 10.0)]
TRAJECTORY_OPTION = dict(maxiter=6, tolresid=0.0, maxtime=1e9)


def fixed_clock():
    return 0.0


def feasible_point(n, k, rs, lb=LB):
    """A random strictly feasible orthonormal frame.  Orthogonal columns with entries > -lb have
    nearly disjoint supports, so: a nonnegative frame with disjoint random supports (row i belongs to
    column i mod k), moved along a random horizontal direction far enough to fill every entry and
    little enough to stay above -lb / 2."""
    E = np.zeros((n, k))
    for i in range(n):
        E[i, i % k] = 0.5 + 0.5 * rs.rand()
    E /= np.linalg.norm(E, axis=0)
    M = Grassmann(n, k)
    u = M.projection(E, rs.randn(n, k))
    x = M.retraction(E, (0.4 * lb / np.max(np.abs(u))) * u)
    assert x.min() > -0.5 * lb and np.linalg.norm(x.T @ x - np.eye(k)) < 1e-13
    return x


class _Recording(RosenbrockVectorized):
    """RosenbrockVectorized that keeps the (x, y, mu) of every inner step (one begin_inner each)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.starts = []

    def begin_inner(self, x, y, mu):
        self.starts.append((x.copy(), y.copy(), mu))
        return super().begin_inner(x, y, mu)


def tcg_rows(n, k, alpha, option=None, seeds=(1, 2, 3), lb=LB):
    """Teacher-forcing inputs from an oracle trajectory: for every inner step of the run its (x, y, mu,
    Delta) and the oracle's tCG result there (eta, Heta, j, stop) -- only the steps on which the order
    variants (the same arithmetic in another rounding order) take the same exit, i.e. the rows that are
    not order-sensitive."""
    from oracle.riptrm_oracle import truncated_conjugate_gradient as tcg
    P = _Recording(n, k, alpha, lb)
    orc = RIPTRMOracle(_option(k, option or TRAJECTORY_OPTION), clock=fixed_clock)
    x0, y0 = initial_point(n, k)
    orc.run(P, x0, y0)
    rows = []
    for (x, y, mu), rec in zip(P.starts, orc.trace):
        Delta = rec["Delta"]
        outs = []
        for man in [None] + [Grassmann(n, k, polar="gram", perm_seed=s, assoc_xxt=True) for s in seeds]:
            Q = RosenbrockVectorized(n, k, alpha, lb, man)
            _, _, Hw, c = Q.begin_inner(x, y, mu)
            outs.append(tcg(Q.manifold, Hw, x, c, Delta, 1, 0.1, 1, Q.manifold.dim))
        eta, Heta, j, stop = outs[0]
        if all((o[2], o[3]) == (j, stop) for o in outs[1:]):
            rows.append(dict(x=x, y=y, mu=mu, Delta=Delta, eta=eta, Heta=Heta, j=j, stop=stop,
                             variants=[(o[0], o[1]) for o in outs[1:]]))
    return rows
