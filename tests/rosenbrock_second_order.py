"""CPU checkers for the second-order residual of Rosenbrock on Grassmann(n, k) -- TEST INFRASTRUCTURE ONLY.

The reference's Rosenbrock experiment logs the smallest eigenvalue and the condition number of the
Lagrangian's Hessian restricted to the tangent directions orthogonal to the active constraints'
gradients.  On this problem the operator pymanopt's ehess -> rhess yields is not self-adjoint (the cost
depends on the entries of X, so X^T G_L is not symmetric), and a matrix filled from its upper triangle
depends on the drawn tangent basis.  Two statements of the quantity, both on
``tests/rosenbrock_oracle.py::RosenbrockStructured``:

* ``sym_check``: the symmetric part, in a frame from ``scipy.linalg.null_space`` -- basis-independent;
  what the device is held to;
* ``drawn_check``: the procedure with a drawn basis and the upper-triangle mirror (what the reference
  does), or, with ``symmetrise=True``, the same procedure with (A + A^T) / 2.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.linalg

from rosenbrock_oracle import LB, RosenbrockStructured, feasible_point

EPS = np.finfo(np.float64).eps
SHAPES = [(5, 3), (8, 3), (13, 7), (16, 4), (20, 6), (97, 1)]
ALPHAS = [1.0, 1e3, 1e7]
ACTIVE_COUNTS = [0, 1, 2, 4]
MU = 0.1


def _operator(P, x, y, barrier, mu):
    if barrier:
        return P.begin_inner(x, y, mu)[2]
    return lambda v: P.hesslag(x, y, v)


def _active(P, x, tol):
    return [i for i in range(P.N) if abs(P.ineq[i](x)) < tol]


def _matrix(frame, H, symmetrise):
    """<frame_i, H(frame_j)>: both triangles averaged, or the upper one mirrored."""
    F = np.array([f.ravel() for f in frame])
    HF = np.array([H(f).ravel() for f in frame])
    A = F @ HF.T
    if symmetrise:
        return 0.5 * (A + A.T)
    U = np.triu(A)
    return U + np.triu(A, 1).T


def sym_check(P, x, y, tol, barrier=False, mu=None):
    """The symmetric part's eigenvalues on the complement of the active gradients.  Returns a dict:
    eig (ascending), mineig, maxeig (None when nulldim == 0; mineig is then 0), nactive, nindep, nulldim."""
    n, k = P.n, P.k
    Nx = scipy.linalg.null_space(x.T)
    frame = [np.outer(Nx[:, a], np.eye(k)[b]) for a in range(n - k) for b in range(k)]
    d = len(frame)
    M = _matrix(frame, _operator(P, x, y, barrier, mu), True)
    act = _active(P, x, tol)
    Z, rank = np.eye(d), 0
    if act:
        G = np.array([[np.sum(f * P.ineq_rgrad[i](x)) for i in act] for f in frame])
        U, sv, _ = np.linalg.svd(G, full_matrices=True)
        rank = int(np.sum(sv > 1e-10))
        Z = U[:, rank:]
    out = dict(nactive=len(act), nindep=rank, nulldim=d - rank)
    if d - rank == 0:
        out.update(eig=np.zeros(0), mineig=0.0, maxeig=None)
        return out
    ev = np.linalg.eigvalsh(Z.T @ M @ Z)
    out.update(eig=ev, mineig=ev[0], maxeig=ev[-1])
    return out


def drawn_check(P, x, y, tol, seed, symmetrise=False, linindtol=1e-12):
    """A basis of the active gradients by Gram-Schmidt in index order (kept where the residual norm
    exceeds linindtol), a null basis from seeded random horizontal vectors made orthogonal to it and to
    each other, the operator's matrix in that basis from its upper triangle (or both, symmetrise=True),
    and its eigenvalues.  Returns (mineig, maxeig), (0, None) for an empty basis."""
    M = P.manifold
    rs = np.random.RandomState(seed)
    H = _operator(P, x, y, False, None)

    def gram_schmidt(vs):
        qs, norms = [], []
        for v in vs:
            v = v.copy()
            for q in qs:
                v = v - np.sum(q * v) * q
            nv = np.linalg.norm(v)
            qs.append(v / nv)
            norms.append(nv)
        return qs, np.array(norms)

    grads = [P.ineq_rgrad[i](x) for i in _active(P, x, tol)]
    qs, norms = gram_schmidt(grads) if grads else ([], np.zeros(0))
    basis = [q for q, nv in zip(qs, norms) if nv > linindtol]
    draws = []
    for _ in range(M.dim - len(basis)):
        v = M.projection(x, rs.randn(P.n, P.k))
        v = v / np.linalg.norm(v)
        for q in basis:
            v = v - np.sum(q * v) * q
        draws.append(v)
    if not draws:
        return 0.0, None
    nullbasis, _ = gram_schmidt(draws)
    ev = np.linalg.eigvalsh(_matrix(nullbasis, H, symmetrise))
    return ev[0], ev[-1]


def scale_of(P, x, y, barrier=False):
    """An upper bound of ||H_s||: ||T|| <= 4 alpha + 2 (Gershgorin), ||sym(X^T G_L)|| <= ||X^T G_L||_2,
    and with the barrier term max(y / s)."""
    GL = P.euclidean_gradient(x) - y.reshape(P.n, P.k)
    s = 4.0 * P.alpha + 2.0 + np.linalg.norm(x.T @ GL, 2)
    if barrier:
        s += np.max(y / P.slack(x))
    return s


def bar_of(P, x, y, barrier=False):
    """The GPU test's bar on an eigenvalue: 32 d eps scale (Weyl's inequality on a backward-stable assembly)."""
    return 32.0 * P.manifold.dim * EPS * scale_of(P, x, y, barrier)


@functools.lru_cache(maxsize=None)
def inputs(n, k):
    """The GPU test's points of one shape, one launch: for every alpha and every m in ACTIVE_COUNTS a
    random feasible point, a random positive y and an active_tol between the m-th and the (m + 1)-th
    smallest |g_i|.  Returns (alpha, x, y, tol) arrays; treat them as read-only."""
    rs = np.random.RandomState(1000 * n + k)
    al, xs, ys, tols = [], [], [], []
    for alpha in ALPHAS:
        for m in ACTIVE_COUNTS:
            x = feasible_point(n, k, rs)
            g = np.sort(np.abs(-x.ravel() - LB))
            tols.append(0.5 * g[0] if m == 0 else 0.5 * (g[m - 1] + g[m]))
            al.append(alpha)
            xs.append(x)
            ys.append(0.1 + rs.rand(n * k))
    return np.array(al), np.array(xs), np.array(ys), np.array(tols)


@functools.lru_cache(maxsize=None)
def reference(n, k, barrier=False):
    """sym_check and the bar at every point of inputs(n, k), computed once and shared."""
    al, xs, ys, tols = inputs(n, k)
    out = []
    for a, x, y, t in zip(al, xs, ys, tols):
        P = RosenbrockStructured(n, k, a)
        r = sym_check(P, x, y, t, barrier=barrier, mu=MU if barrier else None)
        r["bar"] = bar_of(P, x, y, barrier)
        out.append(r)
    return out
