"""Rosenbrock on Grassmann(n, k) on the MI355X: problem descriptor, coordinator and batched engine.

The reference (``src/Rosenbrock/coordinator.py:33-95``) builds a pymanopt Grassmann(n, k) problem
whose cost (the chained Rosenbrock-type sum over the row-major flattening of the point, weight
``alpha``) and n k bound constraints (every entry >= -0.01) are autograd closures.  The drop-in takes
the numbers instead (``RosenbrockProblem``) and runs every RIPTRM solve of a batch -- the reference's
Hydra sweep axes: alpha, the bound, start points -- inside ONE HIP launch, one workgroup per
instance (``csrc/riptrm_grassmann.hip``: 64 ceil(n k / 64) threads, one per entry of the point,
1 <= k <= RIPTRM_GR_KMAX, n k <= RIPTRM_GR_NKMAX).  ``TRS_solver='tCG'`` (what
``src/Rosenbrock/config_simulation.yaml`` selects) only.  No CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Any, Dict, List, Optional

import numpy as np
import torch

import riptrm_native as N
from engine import BatchResult, C, NSTAT, NLOG, ResolvedOptions, TCG_NAMES, _stream_handle, assemble_log, resolve_options

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


def _has(cfg, key):
    return (key in cfg) if isinstance(cfg, dict) else hasattr(cfg, key)


def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


class Coordinator:
    """coordinator.py:13-95 with the reference's cfg keys n, k, alpha (the problem is built from the
    cfg alone, not from a dataset)."""

    def __init__(self, cfg, root: str = "."):
        for key in ("n", "k", "alpha"):
            if not _has(cfg, key):
                raise AssertionError(f"cfg lacks '{key}'")
        self.cfg = cfg

    def run(self) -> RosenbrockProblem:
        return RosenbrockProblem(n=int(_get(self.cfg, "n")), k=int(_get(self.cfg, "k")),
                                 alpha=float(_get(self.cfg, "alpha")))


class RosenbrockBatch:
    """A batch of Rosenbrock solves of one shape (n, k) on one GPU: one workgroup per instance, one
    launch.  alpha and lb are per instance."""

    def __init__(self, n: int, k: int, batch: int, device: Optional[int] = None, log_capacity: int = 4096):
        if not torch.cuda.is_available():
            raise RuntimeError("RosenbrockBatch needs a ROCm GPU (gfx950); there is no CPU fallback")
        self.lib = N.load()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.n, self.k, self.batch, self.cap = int(n), int(k), int(batch), int(log_capacity)
        self.N = self.n * self.k
        nbytes = int(self.lib.riptrm_gr_workspace_bytes(self.n, self.k, self.batch, self.cap))
        if nbytes < 0:
            raise ValueError(f"need 1 <= k <= {N.CONST['RIPTRM_GR_KMAX']}, k <= n, "
                             f"n k <= {N.CONST['RIPTRM_GR_NKMAX']}, batch >= 1 (got n = {n}, k = {k}, batch = {batch})")
        self.ctx = N.Context(self.device.index, _stream_handle(self.device))
        self.ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device=self.device)
        base = self.ws.data_ptr()
        self._pad = (-base) % 256
        self.ws_ptr = base + self._pad
        self.ws_bytes = nbytes
        self._keep: List[torch.Tensor] = []
        self.ro: Optional[ResolvedOptions] = None
        self._bound = False

    def _view(self, kind: int, shape):
        off = int(self.lib.riptrm_gr_workspace_offset(self.n, self.k, self.batch, self.cap, kind))
        count = int(np.prod(shape))
        start = self._pad + off
        return self.ws[start:start + count * 8].view(torch.float64).view(*shape)

    def x(self):
        return self._view(0, (self.batch, self.n, self.k))

    def y(self):
        return self._view(1, (self.batch, self.N))

    def eta(self):
        return self._view(2, (self.batch, self.n, self.k))

    def heta(self):
        return self._view(3, (self.batch, self.n, self.k))

    def stats(self) -> np.ndarray:
        return self._view(4, (self.batch, NSTAT)).cpu().numpy().copy()

    def log_rows(self, count: int) -> np.ndarray:
        lg = self._view(5, (self.batch, self.cap, NLOG))
        return lg[:, :max(0, min(count, self.cap))].cpu().numpy()

    def _dev(self, a, shape) -> torch.Tensor:
        if isinstance(a, torch.Tensor) and a.device == self.device and a.dtype == torch.float64:
            return a.reshape(shape).contiguous()   # already on the device: no copy
        t = torch.as_tensor(np.array(np.broadcast_to(np.asarray(a, dtype=np.float64), shape)))   # a writable copy
        return t.to(self.device).contiguous()

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
        self.ctx.set_stream(_stream_handle(self.device))
        self.ctx.check(self.lib.riptrm_gr_bind(self.ctx.h, ctypes.byref(pr), self.batch, ctypes.c_void_p(self.ws_ptr),
                                               self.ws_bytes, self.cap), "riptrm_gr_bind")
        self._prob = pr
        self._bound = True
        return self

    def _mat(self, a) -> torch.Tensor:
        return self._dev(a, (self.batch, self.n, self.k))

    def _vec(self, a) -> torch.Tensor:
        return self._dev(a, (self.batch,))

    def hvp(self, x, y, mu, v) -> torch.Tensor:
        """HwCur(v) at (x, y, mu) per instance; x, v: (batch, n, k), y: (batch, n k)."""
        X, Y, V, M = self._mat(x), self._dev(y, (self.batch, self.N)), self._mat(v), self._vec(mu)
        out = torch.zeros_like(X)
        self.ctx.set_stream(_stream_handle(self.device))
        self.ctx.check(self.lib.riptrm_gr_hvp(self.ctx.h, ctypes.c_void_p(X.data_ptr()), ctypes.c_void_p(Y.data_ptr()),
                                              ctypes.c_void_p(M.data_ptr()), ctypes.c_void_p(V.data_ptr()),
                                              ctypes.c_void_p(out.data_ptr())), "riptrm_gr_hvp")
        torch.cuda.synchronize(self.device)
        return out

    def tcg(self, x, y, mu, Delta):
        """tCG at (x, y, mu, Delta) per instance: (eta, Heta, j at exit, stop reason)."""
        X, Y, M, D = self._mat(x), self._dev(y, (self.batch, self.N)), self._vec(mu), self._vec(Delta)
        self.ctx.set_stream(_stream_handle(self.device))
        self.ctx.check(self.lib.riptrm_gr_tcg(self.ctx.h, None, ctypes.c_void_p(X.data_ptr()),
                                              ctypes.c_void_p(Y.data_ptr()), ctypes.c_void_p(M.data_ptr()),
                                              ctypes.c_void_p(D.data_ptr())), "riptrm_gr_tcg")
        torch.cuda.synchronize(self.device)
        st = self.stats()
        js = st[:, C["RIPTRM_STAT_TCG_LAST_J"]].astype(int)
        stops = [TCG_NAMES[int(s)] for s in st[:, C["RIPTRM_STAT_TCG_LAST_STOP"]]]
        return self.eta().clone(), self.heta().clone(), js, stops

    def ops(self, x, u, y):
        """The manifold pieces per instance: (P_x(u), the retraction of u at x, dist(x, y),
        matrix_rank(x) == k); x, u, y: (batch, n, k)."""
        X, U, Y = self._mat(x), self._mat(u), self._mat(y)
        proj, retr = torch.zeros_like(X), torch.zeros_like(X)
        dist = torch.zeros(self.batch, dtype=torch.float64, device=self.device)
        rank = torch.zeros(self.batch, dtype=torch.int32, device=self.device)
        self.ctx.set_stream(_stream_handle(self.device))
        self.ctx.check(self.lib.riptrm_gr_ops(self.ctx.h, *(ctypes.c_void_p(t.data_ptr()) for t in
                                                            (X, U, Y, proj, retr, dist, rank))), "riptrm_gr_ops")
        torch.cuda.synchronize(self.device)
        return proj, retr, dist, rank.bool()

    def launch_info(self) -> Dict[str, int]:
        """Dynamic LDS bytes and threads of a workgroup, workgroups per compute unit."""
        a, b, c = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        self.ctx.check(self.lib.riptrm_gr_launch_info(self.ctx.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
                       "riptrm_gr_launch_info")
        return {"lds_bytes": int(a.value), "threads": int(b.value), "workgroups_per_cu": int(c.value)}

    def begin(self, x0, y0, option: Dict[str, Any], restart_every: int = 0) -> ResolvedOptions:
        ro = resolve_options(option, math.sqrt(self.k), self.cap, restart_every,
                             manvio_classifier=rosenbrock_manvio_kind)
        if ro.exact:
            raise NotImplementedError("TRS_solver='Exact_RepMat' is not implemented for the Rosenbrock problem on "
                                      "Grassmann(n, k): the reference's tangent basis there is a draw of "
                                      "random_tangent_vector, so parity is unpinned; use TRS_solver='tCG'")
        X, Y = self._mat(x0), self._dev(y0, (self.batch, self.N))
        tabs = ro.device_tables(self.device)
        self._keep = [X, Y] + tabs
        self.ctx.set_stream(_stream_handle(self.device))
        self.ctx.check(self.lib.riptrm_gr_solve(self.ctx.h, ctypes.byref(ro.c_opt), ctypes.c_void_p(X.data_ptr()),
                                                ctypes.c_void_p(Y.data_ptr()), ctypes.c_void_p(tabs[0].data_ptr()),
                                                ctypes.c_void_p(tabs[1].data_ptr()), ctypes.c_void_p(tabs[2].data_ptr()),
                                                len(ro.mu_tab)), "riptrm_gr_solve")
        self.ro = ro
        return ro

    def solve(self, x0, y0, option: Dict[str, Any], restart_every: int = 0) -> BatchResult:
        self.begin(x0, y0, option, restart_every)
        return self.result()

    def result(self) -> BatchResult:
        torch.cuda.synchronize(self.device)
        st = self.stats()
        count = st[:, C["RIPTRM_STAT_LOG_COUNT"]].astype(np.int64)
        cap = min(self.cap, int(self.ro.c_opt.log_capacity))
        slots = self.log_rows(int(count.max()) if self.batch else 0)
        logs, dropped = [], []
        for b in range(self.batch):   # one launch per solve: no draining, head + latest records kept
            rows, drop = assemble_log(slots[b], int(count[b]), cap)
            logs.append(rows.copy())
            dropped.append(drop)
        return BatchResult(x=self.x().clone(), y=self.y().clone(), stats=st, raw_log=logs, ro=self.ro,
                           dropped=np.array(dropped))
