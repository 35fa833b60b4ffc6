"""Rosenbrock on Grassmann(n, k) on the MI355X: problem descriptor, coordinator and batched engine.

The reference (``src/Rosenbrock/coordinator.py:33-95``) builds a pymanopt Grassmann(n, k) problem
whose cost (the chained Rosenbrock-type sum over the row-major flattening of the point, weight
``alpha``) and n k bound constraints (every entry >= -0.01) are autograd closures.  The drop-in takes
the numbers instead (``RosenbrockProblem``) and runs every RIPTRM solve of a batch -- the reference's
Hydra sweep axes: alpha, the bound, start points -- inside ONE HIP launch, one workgroup per
instance (``csrc/riptrm_grassmann.hip``: 64 ceil(n k / 64) threads, one per entry of the point,
1 <= k <= RIPTRM_GR_KMAX, n k <= RIPTRM_GR_NKMAX).  ``TRS_solver='tCG'`` (what
``src/Rosenbrock/config_simulation.yaml`` selects), and ``'Exact_RepMat'`` as an opt-in: with
``option["basisfun"] = rosenbrock.basisfun`` (the pinned Householder frame; the reference's matrix depends on
the basis on this problem) the exact-direction instantiation of the same kernel runs, for manifold dimension
k (n - k) <= ``RosenbrockBatch.exact_dim_max()``; without the key it raises.  No CPU fallback.

The simulator's ``callbackfun`` (``src/Rosenbrock/simulator.py:60-105``: the second-order residual and the
condition number on every log row) runs on the device too, one workgroup per log row after the solve
(``csrc/riptrm_grassmann_so.hip``, ``RosenbrockBatch.second_order``, k (n - k) <= RIPTRM_TRS_DIM_MAX).
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Any, Dict, Optional

import numpy as np
import torch

import riptrm_native as N
from engine import BatchResult, C, OneLaunchBatch, ResolvedOptions, assemble_log, dxtype_name, ptr, resolve_options
from problems import cfg_get, cfg_has

LB = 0.01   # coordinator.py:62


@dataclass
class RosenbrockProblem:
    """Structured Rosenbrock problem (coordinator.py:33-95); the defaults are the coordinator's."""
    n: int
    k: int
    alpha: float
    lb: float = LB
    initialpoint: Any = None            # (n, k), default |I[:, :k]| (coordinator.py:78-84)
    initialineqLagmult: Any = None      # (n k,), default ones (coordinator.py:87-91)

    def __post_init__(self):
        self.n, self.k = int(self.n), int(self.k)
        self.alpha, self.lb = float(self.alpha), float(self.lb)
        if self.initialpoint is None:
            self.initialpoint = np.abs(np.eye(self.n)[:, :self.k])
        if self.initialineqLagmult is None:
            self.initialineqLagmult = np.ones(self.n * self.k)
        self.initialeqLagmult = np.array([])

    @property
    def num_ineqconstraints(self) -> int:
        return self.n * self.k

    @property
    def has_eqconstraints(self) -> bool:
        return False

    @property
    def manifold_dim(self) -> int:
        return self.k * (self.n - self.k)

    @property
    def typical_dist(self) -> float:
        return math.sqrt(self.k)   # pymanopt Grassmann.typical_dist

    def cost(self, point) -> float:
        """coordinator.py:45-51 on the host."""
        v = np.asarray(point, dtype=np.float64).flatten()
        d = v[1:] - v[:-1]
        return float(np.sum(self.alpha * d ** 2 + (1 - v[:-1]) ** 2))


def manviofun(problem, x):
    """src/Rosenbrock/simulator.py:107-114 (host copy; the device computes its own).  The reference
    reads k from problem.manifold; here it is the point's column count, so it also works without one."""
    x = np.asarray(x)
    manvio = 0
    if np.linalg.matrix_rank(x) != x.shape[1]:
        print("Rank deficient")
        manvio = np.inf
    return manvio


class _ProbeManifold:
    """What a manviofun may read of pymanopt's Grassmann(n, k): the simulator's reads ``_p``."""

    def __init__(self, n, k):
        self._n, self._p, self._k = n, k, 1
        self.n, self.p, self.k = n, k, k


class _ProbeProblem:
    def __init__(self, n, k):
        self.manifold = _ProbeManifold(n, k)
        self.n, self.k = n, k


def rosenbrock_manvio_kind(f) -> int:
    """Classify 'manviofun' for the Grassmann manifold: 0 (identically zero) or the Rosenbrock
    simulator's rank function, probed with a full-rank frame and a rank-deficient one.  The probe's
    problem carries a manifold with the column count, so the reference's own function
    (``problem.manifold._p``) is classified like this module's copy."""
    if f is None:
        return C["RIPTRM_MANVIO_ZERO"]
    import contextlib
    import io
    good = np.eye(3)[:, :2]
    bad = np.array([[1.0, 1.0], [0.0, 0.0], [0.0, 0.0]])
    probe = _ProbeProblem(3, 2)
    with contextlib.redirect_stdout(io.StringIO()):   # the simulator's function prints on the bad probe
        a, b = f(probe, good), f(probe, bad)
    if a == 0 and b == 0:
        return C["RIPTRM_MANVIO_ZERO"]
    if a == 0 and b == np.inf:
        return C["RIPTRM_MANVIO_GRASSMANN_RANK"]
    raise NotImplementedError("manviofun must be 0 or the Rosenbrock simulator's rank function "
                              "(src/Rosenbrock/simulator.py:107-114)")


CALLBACK_NONE, CALLBACK_SECOND_ORDER = 0, 1
ACTIVE_TOL, LININDTOL = 1e-5, 1e-12   # src/Rosenbrock/simulator.py:15, :60


def callbackfun(problem, x, y, z, eval):
    """``option["callbackfun"]`` with the reference's signature (src/Rosenbrock/simulator.py:100-105) for
    a ``RosenbrockProblem``: adds ``second_order_residual`` and ``condition_number`` at (x, y), computed by
    ``riptrm_gr_second_order`` (one point, one launch).  ``RIPTRM.run`` does not call it per row: it
    recognises it (``rosenbrock_callback_kind``) and evaluates every log row's point in one launch after
    the solve."""
    eng = RosenbrockBatch(problem.n, problem.k, 1, log_capacity=0).load(problem.alpha, problem.lb)
    so = eng.second_order(np.asarray(x, dtype=np.float64)[None], np.asarray(y, dtype=np.float64)[None])
    cols = second_order_columns(so)
    eval["second_order_residual"] = cols["second_order_residual"][0]
    eval["condition_number"] = cols["condition_number"][0]
    return eval


def second_order_columns(so: Dict[str, np.ndarray]) -> Dict[str, list]:
    """The two log columns of ``RosenbrockBatch.second_order``'s result: the device's NaN condition
    number (nulldim == 0, or a point it marked non-finite) is the reference's ``None``."""
    return {"second_order_residual": [np.float64(v) for v in so["mineig"]],
            "condition_number": [None if np.isnan(v) else np.float64(v) for v in so["cond"]]}


def _hessian_f(alpha, u):
    """T u for an n x k array u: the constant tridiagonal Euclidean Hessian of f on the row-major flattening."""
    w = u.ravel()
    dd = w[1:] - w[:-1]
    acc = np.zeros(w.size)
    acc[:-1] = -2.0 * alpha * dd + 2.0 * w[:-1]
    acc[1:] += 2.0 * alpha * dd
    return acc.reshape(u.shape)


def symmetric_second_order(n, k, alpha, lb, x, y, active_tol=ACTIVE_TOL):
    """(mineig, cond or None) of the symmetric-part operator H_s(V) = P_X(T V) - V sym(X^T G_L) on the
    horizontal directions orthogonal to the active gradients, in numpy on the host.  Only the callback
    classifier's probe uses it (Grassmann(3, 1)); solves use the device kernel."""
    x = np.asarray(x, dtype=np.float64).reshape(n, k)
    N = n * k

    Tu = lambda u: _hessian_f(alpha, u)
    two = np.full(N, 2.0)
    two[-1] = 0.0
    GL = Tu(x) - two.reshape(n, k) - np.asarray(y, dtype=np.float64).reshape(n, k)
    xg = x.T @ GL
    sg = 0.5 * (xg + xg.T)
    Q = np.linalg.qr(x, mode="complete")[0][:, k:]
    frame = [np.outer(Q[:, a], np.eye(k)[b]) for a in range(n - k) for b in range(k)]
    proj = lambda u: u - x @ (x.T @ u)
    M = np.array([[np.sum(f * (proj(Tu(g)) - g @ sg)) for g in frame] for f in frame])
    M = 0.5 * (M + M.T)
    act = [i for i in range(N) if abs(-x.ravel()[i] - lb) < active_tol]
    Z = np.eye(len(frame))
    if act:
        G = np.array([[-f.ravel()[i] for i in act] for f in frame])
        U, sv, _ = np.linalg.svd(G, full_matrices=True)
        Z = U[:, int(np.sum(sv > 1e-10)):]
    if Z.shape[1] == 0:
        return 0, None
    ev = np.linalg.eigvalsh(Z.T @ M @ Z)
    return ev[0], ev[-1] / ev[0]


class _CallbackProbeManifold:
    """What src/Rosenbrock/simulator.py:26-58 and utils.orthogonalize / selfadj_operator2matrix read of
    pymanopt's Grassmann(n, k)."""

    def __init__(self, n, k):
        self._n, self._p, self._k = n, k, 1
        self.dim = k * (n - k)
        self._rs = np.random.RandomState(0)

    def inner_product(self, x, u, v):
        return np.tensordot(u, v, axes=u.ndim)

    def norm(self, x, v):
        return np.linalg.norm(v)

    def projection(self, x, u):
        return u - x @ (x.T @ u)

    to_tangent_space = projection

    def zero_vector(self, x):
        return np.zeros_like(x)

    def random_tangent_vector(self, x):
        v = self.projection(x, self._rs.randn(*x.shape))
        return v / np.linalg.norm(v)


class _CallbackProbeProblem:
    """A structured Rosenbrock problem with the attributes simulator.py:60-98 reads."""

    def __init__(self, n, k, alpha, lb):
        self.n, self.k, self.alpha, self.lb = n, k, float(alpha), float(lb)
        M = self.manifold = _CallbackProbeManifold(n, k)
        N = n * k
        two = np.full(N, 2.0)
        two[-1] = 0.0

        Tu = lambda u: _hessian_f(alpha, u)
        egrad = lambda x: Tu(x) - two.reshape(n, k)
        self.riemannian_hessian = lambda x, v: M.projection(x, Tu(v)) - v @ (x.T @ egrad(x))
        unit = lambda i: -np.eye(N)[i].reshape(n, k)
        self.num_ineqconstraints, self.num_eqconstraints = N, 0
        self.ineqconstraints_all = [(lambda x, i=i: -x.ravel()[i] - lb) for i in range(N)]
        self.ineqconstraints_riemannian_gradient = lambda i: (lambda x: M.projection(x, unit(i)))
        self.ineqconstraints_riemannian_gradient_all = [self.ineqconstraints_riemannian_gradient(i) for i in range(N)]
        self.ineqconstraints_riemannian_hessian_all = [(lambda x, v, i=i: -v @ (x.T @ unit(i))) for i in range(N)]
        self.eqconstraints_all = []
        self.eqconstraints_riemannian_gradient_all = []
        self.eqconstraints_riemannian_hessian_all = []


_PROBE_EVAL = {"cost": 1.0, "distance": 0.0, "residual": 1.0, "gradnorm": 1.0, "complviolation": 0.0,
               "dualviolation": 0.0, "manviolation": 0, "maxviolation": 0.0, "meanviolation": 0.0}


def _callback_probes():
    """Two points of Grassmann(3, 1) (k = 1: X^T G_L is a number, so the reference's own function does
    not depend on its basis draw): none of the constraints active, and the first one active."""
    lb = LB
    free = np.array([[0.48], [0.6], [0.64]])
    edge = np.array([[-lb], [0.6], [math.sqrt(1.0 - 0.36 - lb * lb)]])
    y = np.array([0.7, 0.2, 1.3])
    return [(_CallbackProbeProblem(3, 1, 10.0, lb), x, y) for x in (free, edge)]


def rosenbrock_callback_kind(f) -> int:
    """Classify 'callbackfun', in the style of ``rosenbrock_manvio_kind``: CALLBACK_NONE for None or a
    callback that returns ``eval`` unchanged (the reference's default), CALLBACK_SECOND_ORDER for this
    module's ``callbackfun`` or any function that, on the probe points, adds exactly the keys
    ``second_order_residual`` and ``condition_number`` with the probe's symmetric-part values (1e-8
    relative) -- the reference's own (src/Rosenbrock/simulator.py:100-105) does.  Anything else cannot
    run on the device and raises NotImplementedError."""
    if f is None:
        return CALLBACK_NONE
    if f is callbackfun:
        return CALLBACK_SECOND_ORDER
    import contextlib
    import io
    no = NotImplementedError("callbackfun must be None, return eval unchanged, or be the Rosenbrock simulator's "
                             "second-order residual (src/Rosenbrock/simulator.py:100-105); arbitrary Python "
                             "callables cannot run on the device")
    kinds = []
    for probe, x, y in _callback_probes():
        ev = dict(_PROBE_EVAL)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                try:
                    out = f(probe, x.copy(), y.copy(), [], dict(ev))
                except TypeError:   # base_solver.py:26's four-argument default
                    out = f(probe, x.copy(), {}, dict(ev))
        except Exception as e:
            raise no from e
        if not isinstance(out, dict):
            raise no
        if out == ev:
            kinds.append(CALLBACK_NONE)
            continue
        if set(out) != set(ev) | {"second_order_residual", "condition_number"} or any(out[q] != ev[q] for q in ev):
            raise no
        lo, cond = symmetric_second_order(probe.n, probe.k, probe.alpha, probe.lb, x, y)
        close = lambda a, b: a is not None and b is not None and abs(a - b) <= 1e-8 * abs(b)
        if not (close(out["second_order_residual"], lo) and close(out["condition_number"], cond)):
            raise no
        kinds.append(CALLBACK_SECOND_ORDER)
    if len(set(kinds)) != 1:
        raise no
    return kinds[0]


def householder_complement(x):
    """Columns k.. of Q in the Householder QR X = Q [R; 0] (n x (n - k)), with the arithmetic and the sign
    convention of ``csrc/riptrm_grassmann_ops.h::qr_frame`` (the one frame of k_gr_exact and k_gr_so):
    reflector j is H_j = I - beta_j v_j v_j^T with v_j = w - ahat e_j, w = column j of H_{j-1} .. H_0 X from
    row j down, ahat = -||w|| if w_j >= 0 else +||w|| (LAPACK dlarfg's sign: R gets a non-positive diagonal
    wherever w_j >= 0), beta_j = 1 / (||w|| (||w|| + |w_j|)), and Q = H_0 H_1 .. H_{k-1}."""
    x = np.asarray(x, dtype=np.float64)
    n, k = x.shape
    W = x.copy()
    refl = []
    for j in range(k):
        w = W[j:, j].copy()
        nrm = math.sqrt(float(np.sum(w * w)))
        xjj = w[0]
        ah = -nrm if xjj >= 0.0 else nrm
        beta = 1.0 / (nrm * (nrm + abs(xjj))) if nrm > 0.0 else 0.0
        v = np.zeros(n)
        v[j:] = w
        v[j] = xjj - ah
        W[:, j + 1:] -= np.outer(v, beta * (v @ W[:, j + 1:]))
        refl.append((v, beta))
    E = np.eye(n)[:, k:]
    for v, beta in reversed(refl):
        E = E - np.outer(v, beta * (v @ E))
    return E


def basisfun(manifold, x):
    """``option["basisfun"]`` with the reference's signature (src/solver/RIPTRM.py:341, :436, :603): the
    pinned orthonormal basis of the horizontal space at x (n x k, X^T X = I) that the device uses.  Reads
    only x.  With Q from the Householder QR X = Q [R; 0] (``householder_complement``: LAPACK's sign
    convention, ahat_j = -sign(w_j) ||w||, sign(0) = +1), vector number a k + b (0 <= a < n - k,
    0 <= b < k) is Q e_{k+a} e_b^T.  Deterministic, so the reference's Exact_RepMat procedure -- the
    upper triangle of <b_i, HwCur(b_j)> mirrored (utils.py:565-573) -- is too, and the device matches it."""
    x = np.asarray(x, dtype=np.float64)
    n, k = x.shape
    E = householder_complement(x)
    eye = np.eye(k)
    return [np.outer(E[:, a], eye[b]) for a in range(n - k) for b in range(k)]


def _basis_probes():
    """Two points whose frames tell the pinned basis from a draw, a permutation or another completion:
    a generic point of Grassmann(5, 3) and one of Grassmann(4, 2) with a negative pivot."""
    rs = np.random.RandomState(20240607)
    a = np.linalg.qr(rs.randn(5, 3))[0]
    b = np.linalg.qr(rs.randn(4, 2))[0]
    if b[0, 0] > 0:
        b = -b
    return [a, b]


def rosenbrock_basis_kind(f) -> int:
    """Classify 'basisfun', in the style of ``rosenbrock_manvio_kind`` / ``rosenbrock_callback_kind``:
    returns 1 for this module's ``basisfun`` or any callable that reproduces its frame -- every vector, in
    order -- on the two probe points (1e-8, the callback classifier's probe tolerance; the vectors have
    unit norm).  Anything else (None, the reference's default draw of random_tangent_vector, another
    completion or order) raises NotImplementedError: the operator is not self-adjoint here, so the
    reference's matrix, and with it the step, depends on the basis."""
    no = NotImplementedError("TRS_solver='Exact_RepMat' for the Rosenbrock problem on Grassmann(n, k) needs the pinned "
                             "tangent basis: pass basisfun=rosenbrock.basisfun (the reference's default draws "
                             "random_tangent_vector, on which its matrix depends), or use TRS_solver='tCG'")
    if f is None:
        raise no
    if f is basisfun:
        return 1
    for x in _basis_probes():
        n, k = x.shape
        try:
            got = f(_CallbackProbeManifold(n, k), x.copy())
            want = basisfun(None, x)
            ok = len(got) == len(want) and all(np.shape(g) == w.shape and np.max(np.abs(np.asarray(g) - w)) <= 1e-8
                                               for g, w in zip(got, want))
        except Exception as e:
            raise no from e
        if not ok:
            raise no
    return 1


class Coordinator:
    """coordinator.py:13-95 with the reference's cfg keys n, k, alpha (the problem is built from the
    cfg alone, not from a dataset)."""

    def __init__(self, cfg, root: str = "."):
        for key in ("n", "k", "alpha"):
            if not cfg_has(cfg, key):
                raise AssertionError(f"cfg lacks '{key}'")
        self.cfg = cfg

    def run(self) -> RosenbrockProblem:
        return RosenbrockProblem(n=int(cfg_get(self.cfg, "n")), k=int(cfg_get(self.cfg, "k")),
                                 alpha=float(cfg_get(self.cfg, "alpha")))


class RosenbrockBatch(OneLaunchBatch):
    """A batch of Rosenbrock solves of one shape (n, k) on one GPU: one workgroup per instance, one
    launch.  alpha and lb are per instance."""

    abi = "gr"

    def __init__(self, n: int, k: int, batch: int, device: Optional[int] = None, log_capacity: int = 4096):
        super().__init__(batch, log_capacity, device)
        self.n, self.k = int(n), int(k)
        self.N = self.n * self.k
        self.point_shape, self.mult_len = (self.n, self.k), self.N
        nbytes = int(self.lib.riptrm_gr_workspace_bytes(self.n, self.k, self.batch, self.cap))
        if nbytes < 0:
            raise ValueError(f"need 1 <= k <= {N.CONST['RIPTRM_GR_KMAX']}, k <= n, "
                             f"n k <= {N.CONST['RIPTRM_GR_NKMAX']}, batch >= 1 (got n = {n}, k = {k}, batch = {batch})")
        self._allocate(nbytes)
        self._bound = False
        self.trail: Optional[torch.Tensor] = None

    def _offset(self, kind: int) -> int:
        return self.lib.riptrm_gr_workspace_offset(self.n, self.k, self.batch, self.cap, kind)

    def _per_instance(self, a) -> torch.Tensor:
        a = np.asarray(a, dtype=np.float64)
        if a.ndim == 0:
            return self._dev(a, (1,))
        if a.shape != (self.batch,):
            raise ValueError(f"per-instance values must be a scalar or of shape ({self.batch},)")
        return self._dev(a, (self.batch,))

    def load(self, alpha, lb=LB) -> "RosenbrockBatch":
        """alpha, lb: a scalar shared by the batch (stride 0) or one value per instance."""
        self.alphad = self._per_instance(alpha)
        self.lbd = self._per_instance(lb)
        pr = N.RiptrmGRProblem()
        pr.struct_size = ctypes.sizeof(N.RiptrmGRProblem)
        pr.n, pr.k = self.n, self.k
        pr.alpha, pr.alpha_stride = self.alphad.data_ptr(), (0 if self.alphad.numel() == 1 else 1)
        pr.lb, pr.lb_stride = self.lbd.data_ptr(), (0 if self.lbd.numel() == 1 else 1)
        self._sync_stream()
        self._call("bind", ctypes.byref(pr), self.batch, ctypes.c_void_p(self.ws_ptr), self.ws_bytes, self.cap)
        self._prob = pr
        self._bound = True
        self.trail = None   # riptrm_gr_bind unbinds the trail
        return self

    def ops(self, x, u, y):
        """The manifold pieces per instance: (P_x(u), the retraction of u at x, dist(x, y),
        matrix_rank(x) == k); x, u, y: (batch, n, k)."""
        X, U, Y = self._pt(x), self._pt(u), self._pt(y)
        proj, retr = torch.zeros_like(X), torch.zeros_like(X)
        dist = torch.zeros(self.batch, dtype=torch.float64, device=self.device)
        rank = torch.zeros(self.batch, dtype=torch.int32, device=self.device)
        self._sync_stream()
        self._call("ops", *map(ptr, (X, U, Y, proj, retr, dist, rank)))
        torch.cuda.synchronize(self.device)
        return proj, retr, dist, rank.bool()

    def launch_info(self) -> Dict[str, int]:
        """Dynamic LDS bytes and threads of a workgroup, workgroups per compute unit."""
        a, b, c = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        self._call("launch_info", ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        return {"lds_bytes": int(a.value), "threads": int(b.value), "workgroups_per_cu": int(c.value)}

    def second_order(self, x, y, active_tol=ACTIVE_TOL, linindtol=LININDTOL, barrier=False, mu=None,
                     inst=None) -> Dict[str, np.ndarray]:
        """The second-order residual at every point (x_p, y_p) in one launch (``riptrm_gr_second_order``).
        x: (npoints, n, k), y: (npoints, n k), numpy or tensors on the device; active_tol: a scalar or
        one per point; inst: the bound instance (alpha, lb) of every point, default point p = instance p.
        barrier: HwCur (RIPTRM.py:729) instead of the Lagrangian's Hessian.  Returns arrays per point:
        mineig, maxeig, cond (NaN where nulldim == 0), nulldim, nactive, nindep, info."""
        if not self._bound:
            raise RuntimeError("second_order: load() first")
        d = self.k * (self.n - self.k)
        if d > C["RIPTRM_TRS_DIM_MAX"]:
            raise NotImplementedError(f"second_order needs manifold dimension k (n - k) <= {C['RIPTRM_TRS_DIM_MAX']} "
                                      f"(got {d} at n = {self.n}, k = {self.k})")
        x = x if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)
        y = y if isinstance(y, torch.Tensor) else np.asarray(y, dtype=np.float64)
        P = int(x.shape[0])
        X, Y = self._dev(x.reshape(P, self.N), (P, self.N)), self._dev(y.reshape(P, self.N), (P, self.N))
        tol = np.asarray(active_tol, dtype=np.float64)
        if tol.ndim != 0 and tol.shape != (P,):
            raise ValueError(f"active_tol must be a scalar or of shape ({P},)")
        told = self._dev(tol, (1,) if tol.ndim == 0 else (P,))
        it = mud = None
        if inst is not None:
            ia = np.asarray(inst.cpu() if isinstance(inst, torch.Tensor) else inst, dtype=np.int64)
            if ia.shape != (P,) or (P and (ia.min() < 0 or ia.max() >= self.batch)):
                raise ValueError(f"inst must hold {P} instance indices in [0, {self.batch})")
            it = torch.as_tensor(ia.astype(np.int32)).to(self.device)
        elif P > self.batch:
            raise ValueError(f"{P} points for {self.batch} bound instances: pass inst")
        if barrier and mu is not None:
            mud = self._dev(mu, (P,))
        nf = C["RIPTRM_GR_SO_NFIELDS"]
        out = torch.zeros((P, nf), dtype=torch.float64, device=self.device)
        self._sync_stream()
        self._call("second_order", ptr(X), ptr(Y), self.N, ptr(it), P, ptr(told), 0 if tol.ndim == 0 else 1,
                   float(linindtol), 1 if barrier else 0, ptr(mud), ptr(out))
        torch.cuda.synchronize(self.device)
        o = out.cpu().numpy()
        res = {name: o[:, C[f"RIPTRM_GR_SO_{name.upper()}"]].copy() for name in ("mineig", "maxeig", "cond")}
        for name in ("nulldim", "nactive", "nindep", "info"):
            col = o[:, C[f"RIPTRM_GR_SO_{name.upper()}"]]
            res[name] = np.where(np.isnan(col), -1, col).astype(np.int64)
        return res

    def exact_dim_max(self) -> int:
        """The largest manifold dimension k (n - k) of the Exact_RepMat path (``riptrm_gr_exact_dim_max``)."""
        return int(self.lib.riptrm_gr_exact_dim_max())

    def _check_exact_dim(self):
        d = self.k * (self.n - self.k)
        if not 1 <= d <= self.exact_dim_max():
            raise NotImplementedError(f"TRS_solver='Exact_RepMat' for the Rosenbrock problem needs manifold dimension "
                                      f"1 <= k (n - k) <= {self.exact_dim_max()} (got {d} at n = {self.n}, k = {self.k})")

    def exact_step(self, x, y, mu, Delta, tolhardcase=1e-8) -> Dict[str, Any]:
        """The pieces of one Exact_RepMat step at (x, y, mu, Delta) per instance (``riptrm_gr_exact``) in the
        pinned frame (``basisfun``): A (batch, d, d) the mirrored-upper-triangle matrix of HwCur, a (batch, d)
        the coordinates of cxCur, dx (batch, n, k), kind (names: 'boundary', 'interior', 'hardcase_1'), lam1,
        mineig (the smallest eigenvalue of A) and passes (operator applications)."""
        if not self._bound:
            raise RuntimeError("exact_step: load() first")
        self._check_exact_dim()
        d = self.k * (self.n - self.k)
        X, Y, M, D = self._pt(x), self._mult(y), self._vec(mu), self._vec(Delta)
        f64 = dict(dtype=torch.float64, device=self.device)
        A, a, dx = torch.zeros((self.batch, d, d), **f64), torch.zeros((self.batch, d), **f64), torch.zeros_like(X)
        lam, me = torch.zeros(self.batch, **f64), torch.zeros(self.batch, **f64)
        kind = torch.zeros(self.batch, dtype=torch.int32, device=self.device)
        self._sync_stream()
        self._call("exact", float(tolhardcase), *map(ptr, (X, Y, M, D, A, a, dx, kind, lam, me)))
        torch.cuda.synchronize(self.device)
        codes = kind.cpu().numpy()
        return {"A": A.cpu().numpy(), "a": a.cpu().numpy(), "dx": dx.cpu().numpy(), "kind_code": codes,
                "kind": [dxtype_name(int(c)) for c in codes], "lam1": lam.cpu().numpy(), "mineig": me.cpu().numpy(),
                "passes": self.stats()[:, C["RIPTRM_STAT_PASSES"]].copy()}

    def bind_trail(self) -> "RosenbrockBatch":
        """Keep the (x, y) of every log record of the next solves (``riptrm_gr_bind_trail``)."""
        nbytes = int(self.lib.riptrm_gr_trail_bytes(self.n, self.k, self.batch, self.cap))
        self.trail = torch.zeros((self.batch, self.cap, 2, self.N), dtype=torch.float64, device=self.device)
        assert self.trail.numel() * 8 == nbytes
        self._call("bind_trail", ptr(self.trail), nbytes)
        return self

    def trail_points(self, st: np.ndarray):
        """(x, y, inst) of the trail's valid slots in the chronological order of ``assemble_log``, every
        instance's rows one after another, and the row count per instance: torch indexing, on the device."""
        count = st[:, C["RIPTRM_STAT_LOG_COUNT"]].astype(np.int64)
        cap = min(self.cap, int(self.ro.c_opt.log_capacity))
        bi, si, rows = [], [], []
        for b in range(self.batch):
            order, _ = assemble_log(np.arange(self.cap), int(count[b]), cap)
            bi.append(np.full(len(order), b, dtype=np.int64))
            si.append(np.asarray(order, dtype=np.int64))
            rows.append(len(order))
        bi, si = np.concatenate(bi), np.concatenate(si)
        pts = self.trail[torch.as_tensor(bi, device=self.device), torch.as_tensor(si, device=self.device)]
        return pts[:, 0].contiguous(), pts[:, 1].contiguous(), bi, rows

    def begin(self, x0, y0, option: Dict[str, Any], restart_every: int = 0) -> ResolvedOptions:
        ro = resolve_options(option, math.sqrt(self.k), self.cap, restart_every,
                             manvio_classifier=rosenbrock_manvio_kind, callback_classifier=rosenbrock_callback_kind)
        if ro.callback_kind and self.trail is None:
            self.bind_trail()
        if ro.exact:   # opt-in: the reference's matrix depends on its basis here, so the basis must be the pinned one
            rosenbrock_basis_kind(ro.option.get('basisfun'))
            self._check_exact_dim()
        return self._launch(ro, x0, y0)

    def result(self) -> BatchResult:
        res = super().result()
        if self.ro.callback_kind == CALLBACK_SECOND_ORDER:   # one launch over every row of every instance
            X, Y, inst, rows = self.trail_points(res.stats)
            so = self.second_order(X, Y, inst=inst)
            cols = second_order_columns(so)
            res.callback_cols, at = [], 0
            for r in rows:
                res.callback_cols.append({key: val[at:at + r] for key, val in cols.items()})
                at += r
        return res
