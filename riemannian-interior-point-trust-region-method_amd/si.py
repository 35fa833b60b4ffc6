"""StableIdentification on the MI355X: problem descriptor, coordinator and batched engine.

The reference (``src/StableIdentification/coordinator.py:13-187``) builds a pymanopt Product
(SkewSymmetric(d), SPD(d), SPD(d)) problem whose cost and m box constraints are autograd closures
over the trajectory data X / XP.  The drop-in takes the data instead (``SIProblem``) and runs every
RIPTRM solve of a batch (the ``problem_initialpoint`` / ``problem_instance`` axes) inside ONE HIP
launch, one workgroup per instance (``csrc/riptrm_si.hip``: a 64-lane wave up to d = 8, one thread per
element of a d x d block above, d <= RIPTRM_SI_DMAX).  No CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
import os
from dataclasses import dataclass, field
from typing import Any, Dict, Optional

import numpy as np

import riptrm_native as N
from engine import C, OneLaunchBatch, ResolvedOptions, bind_trs_scratch, resolve_options, trs_workspace_slots
from problems import cfg_get, cfg_has


def expand_constset(constset) -> np.ndarray:
    """constset.csv rows -> (m, 5) table [kind, r, c, p0, p1] in the reference's constraint order
    (coordinator.py:132-152): type 0/1 -> (-A_rc + ls, A_rc - rs); type 2 -> -(A_rc - c)^2 + k^2."""
    rows = []
    for row in np.atleast_2d(np.asarray(constset, dtype=np.float64)):
        t, r, c = row[0], int(row[1]), int(row[2])
        if t == 0 or t == 1:
            rows.append((0, r, c, row[3], 0.0))
            rows.append((1, r, c, row[4], 0.0))
        elif t == 2:
            rows.append((2, r, c, row[3], row[4] ** 2))
        else:
            raise ValueError("Invalid constraint type")
    return np.asarray(rows, dtype=np.float64).reshape(-1, 5)


@dataclass
class SIProblem:
    """Structured StableIdentification problem (coordinator.py:49-179)."""
    X: Any                      # (d, N): trajectories without their last column, stacked
    XP: Any                     # (d, N): without their first column
    h: float
    constset: Any               # constset.csv rows
    initialpoint: Any           # [J, R, Q] (d x d each)
    initialineqLagmult: Any     # (m,)
    initialeqLagmult: Any = field(default_factory=lambda: np.array([]))

    @property
    def d(self) -> int:
        return int(np.asarray(self.X).shape[0])

    @property
    def N(self) -> int:
        return int(np.asarray(self.X).shape[1])

    @property
    def cons(self) -> np.ndarray:
        return expand_constset(self.constset)

    @property
    def m(self) -> int:
        return int(self.cons.shape[0])

    @property
    def num_ineqconstraints(self) -> int:
        return self.m

    @property
    def has_eqconstraints(self) -> bool:
        return False

    @property
    def manifold_dim(self) -> int:
        d = self.d
        return d * (d - 1) // 2 + d * (d + 1)

    @property
    def typical_dist(self) -> float:
        # Product.typical_dist = sqrt(sum typical_dist_i^2), each sqrt(dim_i) (pymanopt)
        return math.sqrt(self.manifold_dim)

    def point_array(self) -> np.ndarray:
        return np.stack([np.asarray(a, dtype=np.float64) for a in self.initialpoint])


def synthetic_problem(d: int, seed: int, starts: int = 1, N: int = 20, Xset=(1, 2, 3, 4, 5),
                       oneboxratio: float = 0.2, twoboxratio: float = 0.1, snr: float = 10.0, h: float = 0.02):
    """A StableIdentification instance of block size d by the reference's dataset recipe
    (src/StableIdentification/generator.py:18-134, config_dataset.yaml: N 20, one-box ratio 0.2,
    two-box ratio 0.1, snr 10 dB, h 0.02, 5 trajectories), seeded (numpy legacy RandomState):
      * true (J, R, Q): skew / SPD random points, A = (J - R) Q (:55-64);
      * constraints on floor(ratio d^2) random entries of A (:66-109): one-box [A - a|A|, A + b|A|],
        two-box [-|A| - a|A|, |A| + b|A|] plus -(A - c)^2 + k^2 <= 0 with c = cc A;
      * trajectories x_i = exp(i h A) x_0 ELEMENTWISE (np.exp, as :124) from x_0 ~ U(-1000, 1000)^d,
        AWGN at snr dB (:111-120), normalised (:127-128); X / XP = the noisy ones without their
        last / first column, stacked (coordinator.py:54-90).
    One deviation: the reference draws the constraint values around the true A and then finds
    strictly interior starts with RALM (:136-207, out of scope).  Here a start is the true point
    congruence-perturbed (J + 0.05 skew noise, R, Q -> E R E^T with E = I + 0.05 sym noise), the
    constraint values are drawn around start 0's A (so it is strictly feasible: the two-box radius
    is k = kc |A - c| with kc in [0.2, 0.8)), and further starts (start 0 perturbed the same way at
    2e-3) are kept only if strictly feasible.
    y0 = ones(m).  Returns (X, XP, h, constset rows, [(x0, y0), ...])."""
    rs = np.random.RandomState(seed)

    def skew_pt():
        a = rs.randn(d, d)
        return (a - a.T) / 2

    def spd_pt():
        q, _ = np.linalg.qr(rs.randn(d, d))
        return (q * rs.uniform(0.5, 2.0, d)) @ q.T

    J, R, Q = skew_pt(), spd_pt(), spd_pt()
    A = (J - R) @ Q

    def perturb(x, eps=0.05):
        e = np.eye(d) + eps * (lambda b: (b + b.T) / 2)(rs.randn(d, d))
        return np.stack([x[0] + eps * skew_pt(), e @ x[1] @ e.T, e @ x[2] @ e.T])

    x_first = perturb(np.stack([J, R, Q]))
    A0 = (x_first[0] - x_first[1]) @ x_first[2]
    nel = d * d
    n1, n2 = int(nel * oneboxratio), int(nel * twoboxratio)
    idx = rs.permutation(nel)[:n1 + n2]
    rows = []
    for t, cind in enumerate(idx):
        r, c = cind % d, cind // d
        av = A0[r, c]
        aa = abs(av)
        if t < n1:
            rows.append([0, r, c, av - rs.uniform(0.2, 0.8) * aa, av + rs.uniform(0.2, 0.8) * aa])
        else:
            cc = rs.uniform(0.2, 0.8) * av
            k = rs.uniform(0.2, 0.8) * abs(av - cc)
            rows.append([1, r, c, -aa - rs.uniform(0.2, 0.8) * aa, aa + rs.uniform(0.2, 0.8) * aa])
            rows.append([2, r, c, cc, k])
    constset = np.asarray(rows, dtype=np.float64)
    Xs = XPs = None
    for _ in Xset:
        x0 = -1000 + 2000 * rs.rand(d)
        Xt = np.zeros((d, N))
        Xn = np.zeros((d, N))
        for i in range(N):
            xi = x0 if i == 0 else np.exp(i * h * A) @ x0
            Xt[:, i] = xi
            p = np.mean(np.abs(xi) ** 2) / 10 ** (snr / 10)
            Xn[:, i] = xi + np.sqrt(p) * rs.randn(d)
        Xn = Xn / np.linalg.norm(Xn[:, 0])
        Xs = Xn[:, :N - 1] if Xs is None else np.hstack((Xs, Xn[:, :N - 1]))
        XPs = Xn[:, 1:] if XPs is None else np.hstack((XPs, Xn[:, 1:]))
    cons = expand_constset(constset)

    def feasible(x):
        Ax = (x[0] - x[1]) @ x[2]
        for kind, r, c, p0, p1 in cons:
            kind, r, c = int(kind), int(r), int(c)
            a = Ax[r, c]
            g = (-a + p0) if kind == 0 else ((a - p0) if kind == 1 else (-(a - p0) ** 2 + p1))
            if not g < 0:
                return False
        return bool(np.all(np.linalg.eigvalsh(x[1]) > 0) and np.all(np.linalg.eigvalsh(x[2]) > 0))

    assert feasible(x_first), "start 0 must be strictly feasible by construction"
    m = cons.shape[0]
    out = [(x_first, np.ones(m))]
    tries = 0
    while len(out) < starts and tries < 100 * starts:
        tries += 1
        x = perturb(x_first, 2e-3)
        if feasible(x):
            out.append((x, np.ones(m)))
    assert len(out) == starts, "could not draw enough strictly feasible starts"
    return Xs, XPs, h, constset, out


def si_manviofun(problem, x):
    """src/StableIdentification/simulator.py:11-32 (host copy; the device computes its own)."""
    J, R, Q = x[0], x[1], x[2]
    manvio = 0
    manvio += np.linalg.norm(J + J.T)
    manvio += np.linalg.norm(R - R.T)
    manvio += np.linalg.norm(Q - Q.T)
    if not np.all(np.linalg.eigvalsh(R) > 0):
        print("R is not positive definite.")
        manvio = np.inf
    if not np.all(np.linalg.eigvalsh(Q) > 0):
        print("Q is not positive definite.")
        manvio = np.inf
    return manvio


def si_manvio_kind(f) -> int:
    """Classify 'manviofun' for the product manifold: 0 (identically zero) or the SI simulator's."""
    if f is None:
        return C["RIPTRM_MANVIO_ZERO"]
    good = [np.zeros((3, 3)), np.eye(3), np.eye(3)]
    bad = [np.ones((3, 3)), np.eye(3), np.eye(3)]
    a, b = f(None, good), f(None, bad)
    if a == 0 and b == 0:
        return C["RIPTRM_MANVIO_ZERO"]
    if a == 0 and abs(b - 6.0) < 1e-12:
        return C["RIPTRM_MANVIO_SI"]
    raise NotImplementedError("manviofun must be 0 or the StableIdentification simulator's "
                              "(src/StableIdentification/simulator.py:11-32)")


class SICoordinator:
    """coordinator.py:13-179 with the reference's cfg keys and dataset layout
    (dataset/StableIdentification/<instance>/...)."""

    def __init__(self, cfg, root: str = "."):
        for key in ("problem_name", "problem_instance", "problem_initialpoint"):
            if not cfg_has(cfg, key):
                raise AssertionError(f"cfg lacks '{key}'")
        self.cfg = cfg
        self.dataset_path = os.path.join(root, f"dataset/{cfg_get(cfg, 'problem_name')}/{cfg_get(cfg, 'problem_instance')}")

    def run(self) -> SIProblem:
        p = self.dataset_path
        noisy = bool(cfg_get(self.cfg, "is_X_noisy", True))
        Xset = list(cfg_get(self.cfg, "Xset", [1, 2, 3, 4, 5]))
        h = float(cfg_get(self.cfg, "h", 0.02))
        X = XP = None
        for i in Xset:   # coordinator.py:71-88
            Xo = np.loadtxt(f"{p}/{'noisyX' if noisy else 'X'}_{i}.csv")
            n = Xo.shape[1]
            Xc, XPc = Xo[:, :n - 1], Xo[:, 1:n]
            X = Xc if X is None else np.hstack((X, Xc))
            XP = XPc if XP is None else np.hstack((XP, XPc))
        dim = int(np.loadtxt(f"{p}/dim.csv"))
        if X.shape[0] != dim:
            raise ValueError(f"inconsistent StableIdentification dataset at {p}")
        pt = cfg_get(self.cfg, "problem_initialpoint")
        x0 = [np.loadtxt(f"{p}/init{c}_{pt}.csv") for c in "JRQ"]
        y0 = np.atleast_1d(np.loadtxt(f"{p}/initineqLagmult.csv"))
        return SIProblem(X=X, XP=XP, h=h, constset=np.loadtxt(f"{p}/constset.csv"), initialpoint=x0,
                         initialineqLagmult=y0)


class SIBatch(OneLaunchBatch):
    """A batch of StableIdentification solves on one GPU: one workgroup per instance, one launch."""

    abi = "si"

    def __init__(self, d: int, N_: int, m: int, batch: int, device: Optional[int] = None, log_capacity: int = 4096):
        super().__init__(batch, log_capacity, device)
        self.d, self.N, self.m = int(d), int(N_), int(m)
        self.dd = self.d * self.d
        self.point_shape, self.mult_len = (3, self.d, self.d), self.m
        nbytes = int(self.lib.riptrm_si_workspace_bytes(self.d, self.N, self.m, self.batch, self.cap))
        if nbytes < 0:
            raise ValueError(f"need 1 <= d <= {N.CONST['RIPTRM_SI_DMAX']}, 1 <= m <= 64 (d <= 8) or "
                             f"m <= 64 ceil(d^2 / 64) (d > 8), batch >= 1")
        self._allocate(nbytes)
        self._trs_ws = None   # (buffer, order, slots): Exact_RepMat at d >= 8 (manifold.dim > 96)

    def _offset(self, kind: int) -> int:
        return self.lib.riptrm_si_workspace_offset(self.d, self.N, self.m, self.batch, self.cap, kind)

    def load(self, X, XP, h: float, cons) -> "SIBatch":
        """X, XP: (d, N) shared by the batch or (batch, d, N); cons: (m, 5) or (batch, m, 5)."""
        X, XP, cons = np.asarray(X, np.float64), np.asarray(XP, np.float64), np.asarray(cons, np.float64)
        shared_data = X.ndim == 2
        shared_cons = cons.ndim == 2
        self.Xd = self._dev(X, X.shape)
        self.XPd = self._dev(XP, XP.shape)
        self.consd = self._dev(cons, cons.shape)
        pr = N.RiptrmSIProblem()
        pr.struct_size = ctypes.sizeof(N.RiptrmSIProblem)
        pr.d, pr.N, pr.m, pr.h = self.d, self.N, self.m, float(h)
        pr.X, pr.XP = self.Xd.data_ptr(), self.XPd.data_ptr()
        pr.data_stride = 0 if shared_data else self.d * self.N
        pr.cons = self.consd.data_ptr()
        pr.cons_stride = 0 if shared_cons else self.m * 5
        self._sync_stream()
        self._call("bind", ctypes.byref(pr), self.batch, ctypes.c_void_p(self.ws_ptr), self.ws_bytes, self.cap)
        self._prob = pr
        return self

    def begin(self, x0, y0, option: Dict[str, Any], restart_every: int = 0) -> ResolvedOptions:
        d = self.d
        tdim = d * (d - 1) // 2 + d * (d + 1)
        ro = resolve_options(option, math.sqrt(tdim), self.cap, restart_every, manvio_classifier=si_manvio_kind)
        if ro.exact and tdim > C["RIPTRM_TRS_DIM_MAX"]:
            # d >= 8: the subproblem's matrix (manifold.dim squared) no longer fits LDS; instances park
            # at each subproblem and the host's batched service (riptrm_trs_big.hip) solves them in
            # caller-owned HBM scratch, one slot per instance of a pass (riptrm_trs_bind_workspace)
            slots = trs_workspace_slots(self.lib, tdim, self.batch)
            self._trs_ws = bind_trs_scratch(self.ctx, self.lib, self.device, self._trs_ws, tdim, slots)
        return self._launch(ro, x0, y0)

    def profile_enable(self, on: bool = True):
        self._call("profile_enable", 1 if on else 0)

    def profile_read(self) -> Dict[str, float]:
        out = (ctypes.c_double * C["RIPTRM_SI_PROF_NFIELDS"])()
        self._call("profile_read", out)
        names = ("total", "prepare", "tcg", "hvp", "trial", "eval")
        return {k: float(out[i]) for i, k in enumerate(names)}
