"""LDDMM model for point sets (classic / hybrid / logdet), HIP-backed.

Mirror of diffICP/core/LDDMM.py:28-398 (`LDDMMModel`): same constructor, attributes and
methods (v, mdivsum, Hamiltonian, dtrajcost, ODE, v2p, random_p, Shoot, trajloss,
BasicQuadLossFunctor, Optimize), same return conventions.  The vector field is
    v(x) = sum_j [p_j K(x - q_j) - eta (grad K)(x - q_j)],  eta = 1/lambda or 0.
What changes is where the arithmetic happens: Shoot() runs the fused trajectory of
core/shooting.py (one fused HIP pass per ODE evaluation, exact discrete adjoint for the
backward) instead of the reference's per-reduction integrator loop.
"""
from __future__ import annotations

import math
import os
import threading
import warnings
import weakref

import torch

from .. import _lib
from ..tools.integrators import EulerIntegrator, RalstonIntegrator
from ..tools.kernel import GaussKernel, SVDpow
from ..tools.optim import LBFGS_optimization
from ..tools.spec import defspec, getspec
from .shooting import (HamiltonianFn, OdeExtFn, OdeFn, RowOrderCache, ShootCache, ShootFn,
                       complete_p1, cut_active, cut_order_for, last_shoot_cut, row_order_for, skip_p1)



# per host thread: (q0 weak reference, q0 version, sigma, extent / sigma) of the last support
# whose extent was read (LDDMMModel._raw_for): one device read per new q0 tensor
_EXTENT_MEMO = threading.local()

# Optimize's closures form loss and gradient without the autograd engine where the loss allows
# (shooting.shoot_loss_grad; env DICP_DIRECT_LOSSGRAD=0: always through autograd)
_DIRECT_LOSSGRAD = os.environ.get("DICP_DIRECT_LOSSGRAD", "1") != "0"

class Shoot(list):
    """A "shoot" variable: list of (q, p, cost[, x]) states at the nt+1 integration times
    (LDDMM.py:286-299).  The states are views into stacked trajectory tensors Q, P, C[, X]
    that stay resident on the device."""

    # The state views are formed when read: a closure reads shoot[-1] (and trajloss shoot[0]),
    # and forming all 3 (nt+1) views of every shooting was ~1500 tensor selects per diff-ICP
    # iteration, ~8% of the host floor at 2k points (tools/host_floor.py).  Indexing by an int
    # forms (and keeps) that state only.  Any other list operation first fills the list's own
    # storage with every state; from then on (`_full`) the storage is authoritative, so list
    # mutators, concatenation and comparisons behave as on a plain list.
    def __init__(self, Q, P, C, X=None, H0=None):
        super().__init__()
        self.Q, self.P, self.C, self.X = Q, P, C, X
        self.H0 = H0   # H(q0, p0) from the first ODE evaluation (differentiable), or None
        self._n = Q.shape[0]
        self._states = {}
        self._full = False

    def _state(self, t):
        if t < 0:
            t += self._n
        if not 0 <= t < self._n:
            raise IndexError("shoot index out of range")
        s = self._states.get(t)
        if s is None:
            Q, P, C, X = self.Q, self.P, self.C, self.X
            s = (Q[t], P[t], C[t]) if X is None else (Q[t], P[t], C[t], X[t])
            self._states[t] = s
        return s

    def _fill(self):
        if not self._full:
            items = [self._state(t) for t in range(self._n)]
            super().clear()
            super().extend(items)
            self._full = True

    def __getitem__(self, k):
        if self._full:
            return super().__getitem__(k)
        if isinstance(k, int):
            return self._state(k)
        self._fill()
        return super().__getitem__(k)

    def __len__(self):
        return super().__len__() if self._full else self._n

    def __iter__(self):
        if self._full:
            return super().__iter__()
        return (self._state(t) for t in range(self._n))

    def __reversed__(self):
        if self._full:
            return super().__reversed__()
        return (self._state(t) for t in reversed(range(self._n)))

    def __bool__(self):
        return len(self) > 0

    __hash__ = None

    def __radd__(self, other):
        # other + shoot: list.__add__ would read this object's (possibly unfilled) storage
        return list(other) + list(self)

    def copy(self):
        return list(self)

    def __reduce__(self):
        """Pickle / deepcopy: the stacked tensors and attributes, plus the states themselves
        once the list was filled (it may have been mutated since)."""
        state = {k: v for k, v in self.__dict__.items() if k != "_states"}
        if self._full:
            state["_items"] = list(super().__iter__())
        return (Shoot, (self.Q, self.P, self.C, self.X, self.H0), state)

    def __setstate__(self, state):
        items = state.pop("_items", None)
        self.__dict__.update(state)
        self._states = {}
        super().clear()
        if items is not None:
            super().extend(items)
            self._full = True
        else:
            self._full = False

    def detach(self):
        d = lambda t: None if t is None else t.detach()
        sh = Shoot(d(self.Q), d(self.P), d(self.C), d(self.X), d(self.H0))
        for k in ("p1_missing", "raw", "q0_key"):     # LDDMMModel.complete_shoot's inputs
            if hasattr(self, k):
                setattr(sh, k, getattr(self, k))
        return sh


def _fill_first(name):
    """list method `name` on a Shoot, after its storage is filled with every state."""
    base = getattr(list, name)

    def f(self, *a, **k):
        self._fill()
        for o in a:   # list's C methods read another Shoot's storage directly
            if isinstance(o, Shoot):
                o._fill()
        return base(self, *a, **k)

    f.__name__ = name
    f.__doc__ = base.__doc__
    return f


for _m in ("append", "extend", "insert", "pop", "remove", "sort", "reverse", "clear", "index",
           "count", "__setitem__", "__delitem__", "__iadd__", "__imul__", "__add__", "__mul__",
           "__rmul__", "__contains__", "__eq__", "__ne__", "__lt__", "__le__", "__gt__", "__ge__",
           "__repr__"):
    setattr(Shoot, _m, _fill_first(_m))
del _m


def _data_grad(dataloss, x):
    """grad dataloss(x) by autograd (zeros where the loss does not read x)."""
    with torch.enable_grad():
        x = x.detach().requires_grad_(True)
        val = dataloss(x).sum()
        g = torch.autograd.grad(val, x, allow_unused=True)[0] if val.requires_grad else None
    return torch.zeros_like(x) if g is None else g.detach()


def _autograd_data_hvp(dataloss, x, dx):
    """(Hess dataloss)(x) dx_l for the directions dx (L, ...) by torch double-backward, one
    direction at a time (zeros where the gradient does not depend on x)."""
    outs = []
    for l in range(dx.shape[0]):
        with torch.enable_grad():
            xr = x.detach().requires_grad_(True)
            val = dataloss(xr).sum()
            g = torch.autograd.grad(val, xr, create_graph=True, allow_unused=True)[0] if val.requires_grad else None
            hv = None
            if g is not None and g.requires_grad:
                hv = torch.autograd.grad(g, xr, dx[l], allow_unused=True)[0]
        outs.append(torch.zeros_like(x) if hv is None else hv.detach())
    return torch.stack(outs) if outs else dx.clone()


class LDDMMModel:

    def __init__(self, sigma=1.0, D=2, lambd=2.0, spec=defspec, gradcomponent=True,
                 withlogdet=True, version=None, computversion="hip", scheme="Ralston",
                 nonsupprev=False, nt=10):
        """Same arguments as LDDMM.py:33-65.  `version` in {classic, logdet, hybrid}
        overrides (gradcomponent, withlogdet)."""
        self.Kernel = GaussKernel(sigma, D, computversion=computversion, spec=spec)
        self.D = D
        self.lam = lambd
        self.nt = nt
        if version == "classic":
            gradcomponent, withlogdet = False, False
        elif version == "logdet":
            gradcomponent, withlogdet = True, True
        elif version == "hybrid":
            gradcomponent, withlogdet = False, True
        self.withlogdet = withlogdet
        self.gradcomponent = gradcomponent
        self.eta = 1.0 / lambd if gradcomponent else 0
        self.nonsupprev = nonsupprev
        self.scheme, self.Integrator = None, None
        self.set_integration_scheme(scheme)
        self.try_trajcost_optim = False
        self.row_split = None
        # spatial visit order of the support rows for the fused forward passes (shooting.py
        # spatial_order), memoised per q0 (the support points are fixed over an L-BFGS run);
        # only the matrix-core forward (library option fwd_alg 3) uses it: set
        # `row_orders = RowOrderCache()` together with that option
        self.row_orders = None
        # the latest trajectory per q0, reused bitwise when the same shooting is asked for
        # again (shooting.ShootCache: the first closure of each Reg_opt L-BFGS run)
        self.shoot_cache = ShootCache()

    def set_row_split(self, group=None, enable=True, exact_reduce=None, verify=None, overlap=None):
        """Split every dense Euler shooting of this model over the ranks of a torch.distributed
        group (extension; core/rowsplit.py): all ranks must make the same
        calls (the host logic runs replicated).  enable=False restores single-device shooting.
        exact_reduce / verify / overlap: see RowSplit (rank-ordered VJP sums / cross-rank bit
        checks / forward steps in column phases overlapping the all-gathers).
        The L-BFGS divergence fallback draws from a generator seeded identically on every rank
        (tools/optim.py), so the replicated iterates stay in lockstep whatever each rank's
        global RNG state is."""
        from .rowsplit import RowSplit
        self.row_split = (RowSplit(group, exact_reduce=exact_reduce, verify=verify, overlap=overlap)
                          if enable else None)

    def set_integration_scheme(self, scheme: str):
        self.scheme = scheme
        if scheme == "Euler":
            self.Integrator = EulerIntegrator
        elif scheme == "Ralston":
            self.Integrator = RalstonIntegrator
        else:
            raise ValueError(f"Unkown numerical scheme : {scheme}")

    def __setstate__(self, state):
        self.__dict__.update(state)
        if self.__dict__.get("row_orders") is not None:
            self.row_orders = RowOrderCache()
        self.shoot_cache = ShootCache()
        self.Kernel = GaussKernel(self.Kernel.sigma, self.Kernel.D, self.Kernel.computversion,
                                  spec=defspec)

    @property
    def sigma(self):
        return self.Kernel.sigma

    # ------------------------------------------------------------------------------------
    def v(self, x, q, p):
        """v(x) = KRed(x,q,p) - eta GradKRed(x,q)   (LDDMM.py:100-116)."""
        spec = getspec(x, q, p)
        if x.numel() == 0:
            return torch.empty(x.shape, **spec)
        if self.gradcomponent:
            return self.Kernel.KRed(x, q, p) - self.eta * self.Kernel.GradKRed(x, q)
        return self.Kernel.KRed(x, q, p)

    def mdivsum(self, x, q, p, rev=False):
        """-sum_k div v(x_k), shape (1,)-compatible scalar (LDDMM.py:120-138)."""
        spec = getspec(x, q, p)
        if x.numel() == 0:
            return torch.tensor([0.0], **spec)
        if rev:
            r = self.Kernel.GradKRed_rev(q, x, p).sum()
        else:
            r = (p * self.Kernel.GradKRed(q, x)).sum()
        if self.gradcomponent:
            r = r + self.eta * self.Kernel.LapKRed(q, x).sum()
        return r

    def Hamiltonian(self, q, p):
        """H(q,p) = 1/2 sum_ij [p_i.p_j K - eta (p_i-p_j).gradK - eta^2 LapK]  (LDDMM.py:142-159),
        one fused HIP pass."""
        getspec(q, p)
        return HamiltonianFn.apply(q.contiguous(), p.contiguous(), self.Kernel.sigma, float(self.eta))

    def dtrajcost(self, q, p):
        """lambda*H(q,p) + mdivsum(q,q,p) variant (LDDMM.py:163-172)."""
        getspec(q, p)
        return 0.5 * self.lam * (p * self.Kernel.KRed(q, q, p)).sum() \
            + 0.5 * self.eta * self.Kernel.LapKRed(q, q).sum()

    def ODE(self, q, p, cost, x=None):
        """d/dt (q, p, cost[, x]) (LDDMM.py:176-227); one fused HIP pass (+1 for x)."""
        spec = getspec(q, p, cost, x)
        want_div = bool(self.withlogdet)
        if self.try_trajcost_optim and self.withlogdet and self.gradcomponent and x is None:
            vq, mG, _ = OdeFn.apply(q.contiguous(), p.contiguous(), self.Kernel.sigma,
                                    float(self.eta), False)
            return vq, mG, self.dtrajcost(q, p).reshape(1)
        if x is None:
            vq, mG, dcost = OdeFn.apply(q.contiguous(), p.contiguous(), self.Kernel.sigma,
                                        float(self.eta), want_div)
            if not want_div:
                dcost = torch.tensor([0.0], **spec)
            return vq, mG, dcost
        vq, mG, dcost, vx = OdeExtFn.apply(q.contiguous(), p.contiguous(), x.contiguous(),
                                           self.Kernel.sigma, float(self.eta), want_div)
        if not want_div:
            dcost = torch.tensor([0.0], **spec)
        return vq, mG, dcost, vx

    # ------------------------------------------------------------------------------------
    def v2p(self, q, v, rcond=1e-3, alpha=1e-4, version="pinv"):
        """Momenta p with v(q,q,p) ~= v (LDDMM.py:235-253)."""
        getspec(q, v)
        rhs = v if self.eta == 0 else v + self.eta * self.Kernel.GradKRed(q, q)
        if version == "pinv":
            return self.Kernel.KpinvSolve(q, rhs, rcond)
        elif version in ("ridge_keops", "ridge_hip"):
            # device CG with the KRed mat-vec (KeOps LazyTensor.solve semantics)
            return self.Kernel.KridgeSolve_keops(q, rhs, alpha)
        elif version == "ridge_pytorch":
            return self.Kernel.KridgeSolve_pytorch(q, rhs, alpha)
        raise ValueError("unknown version")

    def random_p(self, q, rcond=1e-3, alpha=1e-4, version="svd"):
        """Momenta drawn from exp(-lambda H(q,p)) (LDDMM.py:257-280)."""
        spec = getspec(q)
        if self.eta != 0:
            raise ValueError("random_p not implemented yet when gradcomponent=True.")
        K = (-(q[:, None, :] - q[None, :, :]) ** 2 / (2 * self.Kernel.sigma ** 2)).sum(-1).exp()
        zeta = torch.randn(q.shape, **spec) / math.sqrt(self.lam)
        if version == "svd":
            return (SVDpow(K, -0.5, rcond) @ zeta).contiguous()
        elif version == "ridge":
            return torch.linalg.solve(torch.linalg.cholesky(
                K + alpha * torch.eye(K.shape[0], **spec)), zeta).contiguous()
        raise ValueError("Unknown version")

    # ------------------------------------------------------------------------------------
    def Shoot(self, q0, p0, x0=None, need_p1=True):
        """Geodesic shooting from (q0, p0[, x0]); returns the list of (q, p, cost[, x])
        at the nt+1 times (LDDMM.py:286-299).  need_p1=False (extension, used by Optimize's
        loss closures): the final momenta may be left unformed (NaN; `shoot.p1_missing`) --
        the loss never reads them, and the last step then skips the momentum update's sums."""
        getspec(q0, p0, x0)
        if self.try_trajcost_optim and self.withlogdet and self.gradcomponent and x0 is None:
            # rarely used reference variant: generic integrator over the per-step ODE
            cost0 = torch.zeros(1, dtype=q0.dtype, device=q0.device)
            return self.Integrator(self.ODE, (q0, p0, cost0), self.nt)
        q0c = q0.contiguous()
        raw = self._raw_for(q0)
        outs = ShootFn.apply(q0c, p0.contiguous(),
                             None if x0 is None else x0.contiguous(), self.Kernel.sigma,
                             float(self.eta), int(self.nt), self.scheme, bool(self.withlogdet),
                             self.row_split, getattr(self, "row_orders", None),
                             getattr(self, "shoot_cache", None), bool(need_p1), raw)
        if x0 is None:
            Q, P, C, H0 = outs
            sh = Shoot(Q, P, C, None, H0)
        else:
            sh = Shoot(*outs)
        sh.p1_missing = skip_p1(need_p1, self.scheme, x0 is not None, float(self.eta),
                                self._split(), int(self.nt))
        if sh.p1_missing:
            # what complete_shoot needs to form P[nt] exactly as this shooting would have: the
            # coordinate mode its kernels ran in and the support tensor its row order is keyed on
            sh.raw, sh.q0_key, sh.cut = raw, q0c, last_shoot_cut()
        return sh

    def _split(self):
        return self.row_split if (self.row_split is not None and self.row_split.world > 1) else None

    def complete_shoot(self, shoot):
        """Form the final momenta of a shoot made with need_p1=False (no-op otherwise)."""
        if getattr(shoot, "p1_missing", False):
            # the row visit order (fwd_alg 3 with row_orders, keyed on the shooting's own q0
            # tensor, not a view of the trajectory) and the coordinate mode (raw beyond
            # RAW_EXTENT_SIGMA) the shooting itself used, so the completed P[nt] is bitwise the
            # one a full shooting would have produced
            split = self._split()
            key = getattr(shoot, "q0_key", None)
            raw = getattr(shoot, "raw", None)
            if key is None:
                key = shoot.Q[0]
            if raw is None:
                raw = self._raw_for(key)
            order, order_l = row_order_for(getattr(self, "row_orders", None), key,
                                           float(self.eta), split, shoot.Q.shape[1])
            # a shooting on the Gaussian-cutoff path (spatial order, boxes): its own last step
            # (recorded by the shooting itself; a hand-made Shoot without the record: today's rule)
            cut = getattr(shoot, "cut", None)
            if cut is None:
                cut = cut_active(key, False, float(self.eta), self.scheme, split, int(self.nt), raw)
            cut_order = cut_order_for(getattr(self, "row_orders", None), key) if cut else None
            with _lib.coord_mode(raw):
                complete_p1(shoot.Q, shoot.P, self.Kernel.sigma, float(self.eta),
                            bool(self.withlogdet), int(self.nt),
                            order=order_l if split is not None else order, split=split,
                            C=shoot.C, cut_order=cut_order)
            shoot.p1_missing = False
            shoot.q0_key = None
        return shoot

    # ------------------------------------------------------------------------------------
    # Deformation Jacobian at carried points (extension; csrc/ext_jac.hip)
    def Dv(self, x, q, p):
        """Velocity gradient A[i, d, a] = dv_d/dx_a (x_i) of the field of (q, p), (N, D, D);
        its trace is minus the divergence row of the external-point ODE.  Inputs are detached."""
        getspec(x, q, p)
        return _lib.ode_ext_jac(x.detach(), q.detach(), p.detach(), self.Kernel.sigma, float(self.eta))[1]

    # ------------------------------------------------------------------------------------
    # RKHS inner products of velocity fields (extension; csrc/gram.hip)
    def _gram_fields(self, fields, what):
        out = []
        for k, f in enumerate(fields):
            if not (isinstance(f, (tuple, list)) and len(f) == 2):
                raise ValueError(f"field_gram: {what}[{k}] must be a pair (q, p) of tensors")
            q, p = f
            if not (isinstance(q, torch.Tensor) and isinstance(p, torch.Tensor)):
                raise ValueError(f"field_gram: {what}[{k}] must be a pair (q, p) of tensors")
            if q.dim() != 2 or q.shape[1] != self.D or p.shape != q.shape:
                raise ValueError(f"field_gram: {what}[{k}] must hold q and p both shaped (n, {self.D}), got "
                                 f"{tuple(q.shape)} and {tuple(p.shape)}")
            out.append((q.detach(), p.detach()))
        return out

    def field_gram(self, fields, others=None):
        """RKHS inner products <v_a, v_b>_V = sum_ij (p_i . p'_j) exp(-|q_i - q'_j|^2 / 2 sigma^2) of
        the velocity fields of the momenta `fields` = [(q, p), ...], each on its own support, as a
        float64 tensor: (F, F) when others is None -- the upper triangle is computed once and
        mirrored, so the result is exactly symmetric -- or the (F, G) products of fields x others.
        One _lib.rkhs_gram call (one pair-sum launch, float64 totals).  For a == b the entry is
        2 Hamiltonian(q, p).  Inputs are detached.
        Only for eta = 0 (classic / hybrid): with the gradient component the field of (q, p) is
        affine in p, not linear (v = K p - eta grad K), so a weighted mean of fields over
        different supports is not the field of any momenta and these sums are not its inner
        products.  ValueError then, and on a field of the wrong shape, dtype or device."""
        if self.eta != 0:
            raise ValueError("field_gram needs eta = 0 (gradcomponent=False): with the gradient component "
                             "the field is affine in the momenta, not linear, so a mean field over "
                             "different supports is not a model field")
        A = self._gram_fields(fields, "fields")
        B = [] if others is None else self._gram_fields(others, "others")
        both = A + B
        if not both:
            return torch.zeros((0, 0), dtype=torch.float64, device=self.Kernel.spec["device"])
        try:
            getspec(*[t for f in both for t in f])
        except ValueError:
            raise ValueError("field_gram: all fields must be on the same device and use the same dtype") from None
        nF, nG = len(A), len(B)
        offsets = [0]
        for q, _ in both:
            offsets.append(offsets[-1] + q.shape[0])
        q = torch.cat([f[0] for f in both], dim=0).contiguous()
        p = torch.cat([f[1] for f in both], dim=0).contiguous()
        if others is None:
            iu = torch.triu_indices(nF, nF)
            g = _lib.rkhs_gram(q, p, offsets, iu.t(), self.Kernel.sigma)
            G = torch.zeros((nF, nF), dtype=torch.float64, device=g.device)
            iu = iu.to(g.device)
            G[iu[0], iu[1]] = g
            G[iu[1], iu[0]] = g
            return G
        pairs = [(a, nF + b) for a in range(nF) for b in range(nG)]
        g = _lib.rkhs_gram(q, p, offsets, torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2),
                           self.Kernel.sigma)
        return g.reshape(nF, nG)

    def _support_states(self, q0, p0, need_p1=False):
        """(Q, P) of Shoot(q0, p0), without reading or writing the model's shoot_cache (need_p1
        False: the final momenta may be left unformed, as in Shoot)."""
        q0c = q0.contiguous()
        with torch.no_grad():
            Q, P, _, _ = ShootFn.apply(q0c, p0.contiguous(), None, self.Kernel.sigma, float(self.eta),
                                       int(self.nt), self.scheme, bool(self.withlogdet), self.row_split,
                                       getattr(self, "row_orders", None), None, bool(need_p1),
                                       self._raw_for(q0))
        return Q, P

    def flow_jacobian(self, q0, p0, x0, shoot=None):
        """The carried points x1 = phi(x0) of Shoot(q0, p0, x0) and the Jacobian J_i = d phi(x_i) /
        d x_i of that DISCRETE flow (the exact derivative of what the shooting computes), (N, D, D).
        The displacement gradient G = J - I is what the steps carry (entries of J near 1 would lose
        ~6e-8 per step to rounding); J = I + G is formed once at the end.
        Euler: one fused step (x, G) -> (x + dt v, G + dt A (I + G)) per time step; Ralston: the
        two stages' A1 at (x; S_t) and A2 at (x_m; S_m), S_m = S_t + (2 dt / 3) ODE(S_t).
        shoot: a forward shoot of (q0, p0) (with or without carried points) whose support states
        are reused; None: they are computed here.  Inputs are detached; the model (its
        shoot_cache included) is left as it was."""
        getspec(q0, p0, x0)
        q0, p0, x0 = q0.detach(), p0.detach(), x0.detach()
        if shoot is None:
            Q, P = self._support_states(q0, p0)
        else:
            Q, P = shoot.Q.detach(), shoot.P.detach()
        nt = Q.shape[0] - 1
        sigma, eta, dt = self.Kernel.sigma, float(self.eta), 1.0 / nt
        D = x0.shape[1]
        x, G = x0.contiguous(), None
        raw = self._raw_for(q0)
        with torch.no_grad():
            if self.scheme == "Euler":
                for t in range(nt):
                    x, G = _lib.ext_jac_step(x, G, Q[t], P[t], sigma, eta, dt)
            else:
                I = torch.eye(D, device=x.device, dtype=x.dtype)
                G = torch.zeros((x.shape[0], D, D), device=x.device, dtype=x.dtype)
                for t in range(nt):
                    q, p = Q[t], P[t]
                    v1, A1 = _lib.ode_ext_jac(x, q, p, sigma, eta)
                    with _lib.coord_mode(raw):
                        vq, mG = _lib.ode_self_fwd(q, p, sigma, eta, False)[:2]
                    qm, pm = q + (2 * dt / 3) * vq, p + (2 * dt / 3) * mG
                    B1 = A1 @ (I + G)
                    v2, A2 = _lib.ode_ext_jac(x + (2 * dt / 3) * v1, qm, pm, sigma, eta)
                    B2 = A2 @ (I + G + (2 * dt / 3) * B1)
                    x = x + (dt / 4) * v1 + (3 * dt / 4) * v2
                    G = G + (dt / 4) * B1 + (3 * dt / 4) * B2
            J = G + torch.eye(D, device=x.device, dtype=x.dtype)
        return x, J

    def flow_inverse(self, q0, p0, y1, shoot=None, tol=None, max_iter=10):
        """x0 with phi(x0) = y1 for the DISCRETE flow phi that Shoot(q0, p0, x0) / flow_jacobian
        compute: the exact inverse of that map (up to tol), not the shooting from (q1, -p1) of the
        reference's `backward`, which inverts only the continuous flow of the eta = 0 field.
        For t = nt-1 ... 0 Newton's iteration solves F_t(x_t) = x_{t+1} from x_t = x_{t+1}, F_t the
        step map of the scheme (_lib.ext_inv_step: v and A = dv/dx in one pair pass, a D x D solve
        per row; Ralston: the first stage's (v1, A1) from _lib.ode_ext_jac, the mid-states formed
        once per time step as in flow_jacobian).  Every pass returns the residual |F_t(x) - x_{t+1}|_inf
        of its INPUT x; a step stops, keeping that input, once the largest finite residual is <= tol
        or after max_iter updates (k updates cost k + 1 passes, one host read each).  Rows whose
        residual is not finite (NaN input, singular DF) take no part in the stopping test.
        tol: coordinate units; None: 1e-6 max(sigma, max finite |y1|).
        shoot: a forward shoot of (q0, p0) whose support states are reused (its final momenta are
        never read: a shoot with p1_missing stays as it is); None: they are computed here.
        Returns (x0, info): rows that did not converge are NaN in x0 (one RuntimeWarning counts
        them); info = dict(converged (N,) bool, residual (N,) float32: the largest certified
        residual over the steps, iterations: the nt update counts (entry t: step t), passes: the
        pair passes of the velocity-gradient operator made, tol).  Inputs are detached; the model
        (its shoot_cache included) is left as it was.  Single device."""
        getspec(q0, p0, y1)
        q0, p0, y1 = q0.detach(), p0.detach(), y1.detach()
        if shoot is None:
            Q, P = self._support_states(q0, p0, need_p1=False)
        else:
            Q, P = shoot.Q.detach(), shoot.P.detach()
        nt = Q.shape[0] - 1
        sigma, eta, dt = self.Kernel.sigma, float(self.eta), 1.0 / nt
        euler = self.scheme == "Euler"
        y = y1.contiguous()
        N = y.shape[0]
        raw = self._raw_for(q0)
        nan = float("nan")
        with torch.no_grad():
            if tol is None:
                a = y.abs()
                big = float(torch.where(torch.isfinite(a), a, torch.zeros_like(a)).max()) if y.numel() else 0.0
                tol = 1e-6 * max(float(sigma), big)
            tol = float(tol)
            worst = torch.zeros(N, device=y.device, dtype=y.dtype)
            iterations = [0] * nt
            passes = 0
            for t in range(nt - 1, -1, -1):
                q, p = Q[t], P[t]
                if not euler:
                    with _lib.coord_mode(raw):
                        vq, mG = _lib.ode_self_fwd(q, p, sigma, eta, False)[:2]
                    qm, pm = q + (2 * dt / 3) * vq, p + (2 * dt / 3) * mG
                x, k = y, 0
                while True:
                    if euler:
                        xn, res = _lib.ext_inv_step(x, y, q, p, sigma, eta, dt)
                        passes += 1
                    else:
                        v1, A1 = _lib.ode_ext_jac(x, q, p, sigma, eta)
                        xn, res = _lib.ext_inv_step(x, y, qm, pm, sigma, eta, dt, v1, A1)
                        passes += 2
                    finite = torch.isfinite(res)
                    rmax = float(torch.where(finite, res, torch.zeros_like(res)).max()) if N else 0.0
                    if rmax <= tol or k >= max_iter:
                        break
                    x, k = xn, k + 1
                iterations[t] = k
                worst = torch.maximum(worst, res)          # NaN stays NaN
                y = torch.where(finite[:, None], x, torch.full_like(x, nan))
            converged = worst <= tol
            x0 = torch.where(converged[:, None], y, torch.full_like(y, nan))
        bad = N - int(converged.sum())
        if bad:
            warnings.warn(f"flow_inverse: {bad} of {N} points did not converge to tol = {tol:.3g} "
                          f"within {max_iter} Newton updates per step (returned as NaN)", RuntimeWarning)
        return x0, dict(converged=converged, residual=worst, iterations=iterations, passes=passes, tol=tol)

    # ------------------------------------------------------------------------------------
    # Forward sensitivities of the shooting (extension; csrc/tlm.hip)
    def shoot_tangent(self, q0, p0, dp0, dq0=None, x0=None, dx0=None, shoot=None, trajectory=False):
        """The tangent-linear model of the DISCRETE flow Shoot(q0, p0, x0) computes: (dQ, dP, dX), the
        exact first-order change of the final support points, momenta and carried points when the
        initial ones move along dq0, dp0 (L, M, D) and dx0 (L, N, D) -- a Jacobi field along the
        geodesic, the Gauss-Newton product J d of a data term, the sensitivity of the map to a
        mode of the momenta.  A 2-D direction means L = 1 and is squeezed on return; dq0 = None
        and dx0 = None mean zero; dX is None without x0.  trajectory=True: at all nt + 1 times,
        (nt + 1, L, ., D).  The cost component gets no tangent.
        One fused pass (_lib.ode_tlm, all L directions in one launch per part) per stage.  Euler:
        dS <- dS + dt TLM(S_t; dS); Ralston: dk1 = TLM(S_t; dS), dk2 = TLM(S_m; dS + h dk1) at the
        mid-state S_m = S_t + h ODE(S_t), h = 2 dt / 3, formed once per step as in flow_jacobian,
        dS <- dS + dt/4 (dk1 + 3 dk2); the carried points are advanced the same way.
        shoot: a forward shoot of (q0, p0) whose support states are reused (its final momenta are
        never read); None: they are computed here.  Inputs are detached; the model (its shoot_cache
        included) is left as it was.  With a row split the call runs replicated on every rank.
        Only for eta = 0 (classic / hybrid): with the gradient component the field is affine in the
        momenta, not linear, and its linearisation needs higher derivatives of the kernel.
        ValueError then, and on directions of the wrong shape."""
        return self._shoot_tangent(q0, p0, dp0, dq0, x0, dx0, shoot, trajectory, True)

    def _shoot_tangent(self, q0, p0, dp0, dq0, x0, dx0, shoot, trajectory, need_support):
        """shoot_tangent; need_support=False: dQ and dP at the final time are not wanted (None), so
        the last stage runs the carried part alone."""
        if self.eta != 0:
            raise ValueError("shoot_tangent needs eta = 0 (gradcomponent=False): with the gradient component "
                             "the field is affine in the momenta, not linear, and its linearisation needs "
                             "higher derivatives of the kernel")
        getspec(q0, p0, dp0, dq0, x0, dx0)
        q0, p0, dp0 = q0.detach(), p0.detach(), dp0.detach()
        single = dp0.dim() == 2
        dp = (dp0[None] if single else dp0).contiguous()
        if dp.dim() != 3 or tuple(dp.shape[1:]) != tuple(q0.shape) or p0.shape != q0.shape:
            raise ValueError(f"shoot_tangent: dp0 must be shaped {tuple(q0.shape)} or (L, {q0.shape[0]}, "
                             f"{q0.shape[1]}), got {tuple(dp0.shape)}")
        L = dp.shape[0]

        def direction(d, rows, name):
            if d is None:
                return torch.zeros((L,) + tuple(rows.shape), device=rows.device, dtype=rows.dtype)
            d = d.detach()
            d = d[None] if d.dim() == 2 else d
            if tuple(d.shape) != (L,) + tuple(rows.shape):
                raise ValueError(f"shoot_tangent: {name} must be shaped like its points, {tuple(rows.shape)}, "
                                 f"with the {L} direction(s) of dp0 in front, got {tuple(d.shape)}")
            return d.contiguous()

        dq = direction(dq0, q0, "dq0")
        if x0 is None and dx0 is not None:
            raise ValueError("shoot_tangent: dx0 needs x0")
        x = None if x0 is None else x0.detach().contiguous()
        dx = None if x is None else direction(dx0, x, "dx0")
        if shoot is None:
            Q, P = self._support_states(q0, p0)
        else:
            Q, P = shoot.Q.detach(), shoot.P.detach()
        nt = Q.shape[0] - 1
        sigma, dt = self.Kernel.sigma, 1.0 / nt
        h = 2 * dt / 3
        euler = self.scheme == "Euler"
        raw = self._raw_for(q0)
        traj = [(dq, dp, dx)]
        with torch.no_grad():
            for t in range(nt):
                q, p = Q[t], P[t]
                last = t == nt - 1
                if euler:
                    dv, dmG, dvx = _lib.ode_tlm(q, p, dq, dp, sigma, x, dx, need_self=need_support or not last)
                    if x is not None:
                        if not last:            # the points the next step linearises at
                            x = x + dt * _lib.ode_ext_fwd(x, q, p, sigma, 0.0, False)[0]
                        dx = dx + dt * dvx
                    dq, dp = (dq + dt * dv, dp + dt * dmG) if dv is not None else (None, None)
                else:
                    with _lib.coord_mode(raw):
                        vq, mG = _lib.ode_self_fwd(q, p, sigma, 0.0, False)[:2]
                    qm, pm = q + h * vq, p + h * mG
                    dv1, dG1, dx1 = _lib.ode_tlm(q, p, dq, dp, sigma, x, dx)
                    xm = dxm = None
                    if x is not None:
                        v1 = _lib.ode_ext_fwd(x, q, p, sigma, 0.0, False)[0]
                        xm, dxm = x + h * v1, dx + h * dx1
                    dv2, dG2, dx2 = _lib.ode_tlm(qm, pm, dq + h * dv1, dp + h * dG1, sigma, xm, dxm,
                                                 need_self=need_support or not last)
                    if x is not None:
                        if not last:
                            x = x + (dt / 4) * v1 + (3 * dt / 4) * _lib.ode_ext_fwd(xm, qm, pm, sigma, 0.0, False)[0]
                        dx = dx + (dt / 4) * dx1 + (3 * dt / 4) * dx2
                    dq, dp = ((dq + (dt / 4) * dv1 + (3 * dt / 4) * dv2, dp + (dt / 4) * dG1 + (3 * dt / 4) * dG2)
                              if dv2 is not None else (None, None))
                if trajectory:
                    traj.append((dq, dp, dx))
        if trajectory:
            outs = [None if traj[-1][k] is None else torch.stack([s[k] for s in traj]) for k in range(3)]
            return tuple(o if o is None or not single else o[:, 0] for o in outs)
        return tuple(o if o is None or not single else o[0] for o in (dq, dp, dx))

    # ------------------------------------------------------------------------------------
    # Hessian-vector products of the shooting loss (extension; csrc/hvp.hip)
    def loss_hvp(self, dataloss, q0, p0, d, data_hvp=None, gauss_newton=False, shoot=None):
        """The Hessian-vector product of the loss Optimize minimises without carried points,
        L(p0) = lam H(q0, p0) + cost_nt + dataloss(q_nt), along d, shaped like d: (M, D), or
        (L, M, D) for L directions at once -- the exact second derivative of the DISCRETE Euler /
        Ralston shooting by its second-order adjoint.  With VJP = DF^T (_lib.ode_self_bwd), TLM = DF
        (_lib.ode_tlm), u(l) = (-l_p, l_q), T the third-derivative operator of the Hamiltonian and
        C the divergence sum of the hybrid model's cost channel (_lib.ode_hvp; gam = 1 with the
        log-determinant, else 0), Euler:
          dS_0 = (0, d),  dS_t+1 = dS_t + dt TLM(S_t; dS_t)                  (_shoot_tangent)
          l_nt = (grad data, 0),  l_t = l_t+1 + dt [VJP(S_t; l_t+1) + gam grad C(S_t)]
          dl_nt = (Hess data dq_nt, 0),
          dl_t = dl_t+1 + dt [VJP(S_t; dl_t+1) + T(S_t; u(l_t+1), dS_t) + gam D^2 C(S_t) dS_t]
          Hess L d = (dl_0)_p + lam K(q0, q0) d;
        Ralston (h = 2 dt / 3, S_m = S + h F(S), dS_m = dS + h TLM(S; dS), l', dl' incoming):
          m = 3dt/4 [VJP(S_m; l') + gam grad C(S_m)],  c = dt/4 l' + h m,
          l = l' + m + VJP(S; c) + dt/4 gam grad C(S)
          dm = 3dt/4 [VJP(S_m; dl') + T(S_m; u(l'), dS_m) + gam D^2 C(S_m) dS_m]
          dl = dl' + dm + VJP(S; dt/4 dl' + h dm) + T(S; u(c), dS) + dt/4 gam D^2 C(S) dS.
        l and dl run backwards together; only the dS trajectory is stored.  One _lib.ode_hvp pass
        per stage for all L directions, one VJP per stage and direction.
        gauss_newton=True: the T, D^2 C and lam K terms are dropped, leaving J^T (Hess data) J d with
        J = d q_nt / d p0 -- positive semi-definite where the data Hessian is, the usual stand-in
        where the exact Hessian is indefinite; the regulariser's own (positive definite) part
        lam K(q0, q0) d is then the caller's to add.
        The data Hessian, in order of preference: data_hvp(q1, dq1) with dq1 (L, M, D); the
        attribute dataloss.hvp of the same signature (BasicQuadLossFunctor and DiffPSR's
        QuadLossFunctor have one); torch double-backward of dataloss, one direction at a time.
        shoot: a forward shoot of (q0, p0) without carried points whose support states are reused.
        Inputs are detached; the model (its shoot_cache included) is left as it was.
        ValueError for eta != 0 (as shoot_tangent), with an active row split (the second-order
        pass has no split form), for a shoot with carried points (the loss of an external x0 is
        not covered) and for a direction of the wrong shape."""
        if self.eta != 0:
            raise ValueError("loss_hvp needs eta = 0 (gradcomponent=False): the second-order operator is that "
                             "of the Hamiltonian without the gradient component")
        if self._split() is not None:
            raise ValueError("loss_hvp: not available with an active row split")
        if shoot is not None and getattr(shoot, "X", None) is not None:
            raise ValueError("loss_hvp: the shoot carries points x0; only the loss on the support points "
                             "(Optimize with x0=None) is covered")
        getspec(q0, p0, d)
        q0, p0, d = q0.detach().contiguous(), p0.detach().contiguous(), d.detach()
        single = d.dim() == 2
        dd = (d[None] if single else d).contiguous()
        if dd.dim() != 3 or tuple(dd.shape[1:]) != tuple(q0.shape) or p0.shape != q0.shape:
            raise ValueError(f"loss_hvp: d must be shaped {tuple(q0.shape)} or (L, {q0.shape[0]}, "
                             f"{q0.shape[1]}), got {tuple(d.shape)}")
        L = dd.shape[0]
        if shoot is None:
            Q, P = self._support_states(q0, p0)
        else:
            Q, P = shoot.Q.detach(), shoot.P.detach()
        nt = Q.shape[0] - 1
        sigma, dt = self.Kernel.sigma, 1.0 / nt
        h = 2 * dt / 3
        euler = self.scheme == "Euler"
        exact = not gauss_newton
        cost = exact and bool(self.withlogdet)
        raw = self._raw_for(q0)
        sh = Shoot(Q, P, None)
        dQ, dP, _ = self._shoot_tangent(q0, p0, dd, None, None, None, sh, True, True)
        q1 = Q[nt]
        if data_hvp is None:
            data_hvp = getattr(dataloss, "hvp", None)
        if data_hvp is None:
            data_hvp = lambda x, dx: _autograd_data_hvp(dataloss, x, dx)
        dlq = data_hvp(q1, dQ[nt]).detach()
        if tuple(dlq.shape) != tuple(dd.shape):
            raise ValueError(f"loss_hvp: the data Hessian must be shaped {tuple(dd.shape)}, got {tuple(dlq.shape)}")
        dlp = torch.zeros_like(dd)
        gdiv = lambda k: torch.full((1,), k, device=q0.device, dtype=q0.dtype) if cost else None
        bwd = lambda q, p, gq, gp, g=None: _lib.ode_self_bwd(q, p, gq.contiguous(), gp.contiguous(), g, sigma, 0.0)

        def bwd_dirs(q, p, gq, gp):          # VJP(S; .) of each direction
            outs = [bwd(q, p, gq[l], gp[l]) for l in range(L)]
            if not outs:
                return torch.zeros_like(dd), torch.zeros_like(dd)
            return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])

        with torch.no_grad(), _lib.coord_mode(raw):
            if exact:
                lq, lp = _data_grad(dataloss, q1), torch.zeros_like(q1)
            for t in range(nt - 1, -1, -1):
                q, p = Q[t], P[t]
                dq, dp = dQ[t], dP[t]
                if euler:
                    gq, gp = bwd_dirs(q, p, dlq, dlp)
                    if exact:
                        tq, tp = _lib.ode_hvp(q, p, -lp, lq, dq, dp, sigma, gdiv(1.0))
                        gq, gp = gq + tq, gp + tp
                        aq, ap = bwd(q, p, lq, lp, gdiv(1.0))
                        lq, lp = lq + dt * aq, lp + dt * ap
                    dlq, dlp = dlq + dt * gq, dlp + dt * gp
                    continue
                vq, mG = _lib.ode_self_fwd(q, p, sigma, 0.0, False)[:2]
                qm, pm = q + h * vq, p + h * mG
                dmq, dmp = bwd_dirs(qm, pm, dlq, dlp)
                if exact:
                    dv1, dG1, _ = _lib.ode_tlm(q, p, dq, dp, sigma)
                    tq, tp = _lib.ode_hvp(qm, pm, -lp, lq, dq + h * dv1, dp + h * dG1, sigma, gdiv(1.0))
                    dmq, dmp = dmq + tq, dmp + tp
                dmq, dmp = (0.75 * dt) * dmq, (0.75 * dt) * dmp
                gq, gp = bwd_dirs(q, p, (0.25 * dt) * dlq + h * dmq, (0.25 * dt) * dlp + h * dmp)
                if exact:
                    mq, mp = bwd(qm, pm, lq, lp, gdiv(1.0))
                    mq, mp = (0.75 * dt) * mq, (0.75 * dt) * mp
                    cq, cp = (0.25 * dt) * lq + h * mq, (0.25 * dt) * lp + h * mp
                    tq, tp = _lib.ode_hvp(q, p, -cp, cq, dq, dp, sigma, gdiv(0.25 * dt))
                    gq, gp = gq + tq, gp + tp
                    aq, ap = bwd(q, p, cq, cp, gdiv(0.25 * dt))
                    lq, lp = lq + mq + aq, lp + mp + ap
                dlq, dlp = dlq + dmq + gq, dlp + dmp + gp
            out = dlp
            if exact and L > 0:
                out = out + self.lam * torch.stack([self.Kernel.KRed(q0, q0, dd[l]) for l in range(L)])
        return out[0] if single else out

    def loss_hessian_extremes(self, dataloss, q0, p0, steps, seed=0, gauss_newton=False):
        """The extreme eigenvalues of the Hessian loss_hvp applies, by `steps` Lanczos iterations
        with full reorthogonalisation (tools/lanczos.py; one loss_hvp per iteration, the small
        tridiagonal algebra in float64 on the host) from a random start drawn with `seed`.
        Returns (ritz, vmin, vmax): the Ritz values in ascending order (float64, on the host; as
        many as iterations ran -- fewer than `steps` on an invariant subspace) and the unit Ritz
        vectors of the smallest and the largest, shaped like p0.  ritz[0] < 0 shows a direction of
        negative curvature; ritz[-1] / ritz[0] estimates the conditioning from below."""
        from ..tools.lanczos import lanczos
        q0, p0 = q0.detach(), p0.detach()
        sh = Shoot(*self._support_states(q0, p0), None)
        matvec = lambda v: self.loss_hvp(dataloss, q0, p0, v.reshape(p0.shape), gauss_newton=gauss_newton,
                                         shoot=sh).reshape(-1)
        g = torch.Generator().manual_seed(int(seed))
        v0 = torch.randn(p0.numel(), generator=g, dtype=torch.float64).to(device=p0.device, dtype=p0.dtype)
        ritz, vecs = lanczos(matvec, v0, int(steps))
        return ritz, vecs[0].reshape(p0.shape), vecs[-1].reshape(p0.shape)

    def BasicQuadLossFunctor(self, y, cmul=1):
        y = y.detach()

        def dataloss(x):
            return ((x - y) ** 2).sum() * cmul / 2
        dataloss.hvp = lambda x, dx: cmul * dx     # loss_hvp: the Hessian is cmul I
        return dataloss

    def trajloss(self, shoot):
        """lambda*H(q0,p0) + cost_1  (LDDMM.py:318-334)."""
        arrival = shoot[-1]
        cost = arrival[2]
        is_x = len(arrival) == 4
        if not is_x and self.withlogdet and self.gradcomponent and self.try_trajcost_optim:
            return cost
        q0, p0 = shoot[0][:2]
        H0 = getattr(shoot, "H0", None)
        if H0 is None:
            H0 = self.Hamiltonian(q0, p0)
        return self.lam * H0 + cost

    # Coordinates of the fused shooting kernels (library option coord_raw).  "scaled": q' =
    # alpha (q - q_0), one packed multiply per two pairs fewer, float32-exact differences only
    # while the support spans up to ~200 sigma (2.8e-6 at 100 sigma, 1.3e-5 at 300 sigma
    # against float64, profiles/r03_extent_precision.jsonl); "raw": original units, the
    # reference's accuracy at any extent; "auto" (default): raw when q0 spans more than
    # RAW_EXTENT_SIGMA sigma (one small device read per new q0 tensor, per host thread).
    coord_mode = "auto"
    RAW_EXTENT_SIGMA = 128.0

    def _raw_for(self, q0):
        mode = self.coord_mode
        if mode == "raw":
            return True
        if mode != "auto" or q0.numel() == 0 or q0.device.type != "cuda":
            return False
        last = getattr(_EXTENT_MEMO, "last", None)
        if (last is not None and last[0]() is q0 and last[1] == q0._version
                and last[2] == float(self.Kernel.sigma)):
            return last[3] > self.RAW_EXTENT_SIGMA
        qd = q0.detach()      # q0 may require a gradient (float() of such a tensor warns)
        ext = float((qd.amax(0) - qd.amin(0)).norm()) / float(self.Kernel.sigma)
        _EXTENT_MEMO.last = (weakref.ref(q0), q0._version, float(self.Kernel.sigma), ext)
        return ext > self.RAW_EXTENT_SIGMA

    def Optimize(self, dataloss, q0, p0, x0=None, nmax=10, tol=1e-3, errthresh=1e8):
        """min_p0 trajloss + dataloss(q1 or x1) with L-BFGS (LDDMM.py:338-398).
        Returns (p0, shoot, trajl, datal, nsteps, change)."""
        getspec(q0, p0, x0)
        is_x = x0 is not None
        q0 = q0.detach()
        if is_x:
            x0 = x0.detach()

        last_eval = {}

        def lossfunc(p0):
            shoot = self.Shoot(q0, p0, x0, need_p1=False)   # the loss never reads p1
            last = shoot[-1][-1] if is_x else shoot[-1][0]
            last_eval["p0"], last_eval["shoot"] = p0.detach().clone(), shoot.detach()
            last_eval["p1_missing"] = getattr(shoot, "p1_missing", False)
            return self.trajloss(shoot) + dataloss(last)

        lossgrad = None
        batcher = getattr(_lib._tl, "batcher", None)
        # the closure forms loss and gradient directly (shooting.shoot_loss_grad: ShootFn's
        # forward and exact adjoint on THIS thread, bitwise the values of
        # lossfunc(p0).backward()) for a frame of a lockstep launch batch (core/batching.py),
        # whose adjoint must run on the frame's thread, and for every dense Euler shooting on
        # the device whose loss is lam H0 + cost + data: no autograd engine (its device-thread
        # hand-off and graph bookkeeping, ~0.1 ms of host time per closure -- the host floor,
        # tools/host_floor.py), and concurrent frames' adjoints no longer queue on the
        # engine's one device thread
        direct = (_DIRECT_LOSSGRAD and not is_x and self.scheme == "Euler" and self.row_split is None
                  and not (self.withlogdet and self.gradcomponent and self.try_trajcost_optim)
                  and q0.is_cuda)
        if (batcher is not None and not is_x) or direct:
            from .shooting import shoot_loss_grad

            def lossgrad(p0):
                if batcher is None:
                    L, g, shoot = shoot_loss_grad(self, dataloss, q0, p0)
                else:
                    with batcher.closure():   # a member of the launch batches while it evaluates
                        L, g, shoot = shoot_loss_grad(self, dataloss, q0, p0)
                last_eval["p0"], last_eval["shoot"] = p0.detach().clone(), shoot
                last_eval["p1_missing"] = getattr(shoot, "p1_missing", False)
                return L, [g]
        p0, _, nsteps, change = LBFGS_optimization([p0], lossfunc, nmax=nmax, tol=tol,
                                                   errthresh=errthresh, lossgrad=lossgrad)
        p0 = p0[0]
        with torch.no_grad():
            # final shoot (LDDMM.py:390): the kernels are deterministic, so when L-BFGS's
            # last closure evaluation was at the returned p0 its trajectory is reused
            if "p0" in last_eval and torch.equal(last_eval["p0"], p0):
                shoot = last_eval["shoot"]
                shoot.p1_missing = last_eval["p1_missing"]
                self.complete_shoot(shoot)              # the returned shoot is complete
            else:
                shoot = self.Shoot(q0, p0, x0)
            trajl = self.trajloss(shoot).item()
            datal = dataloss(shoot[-1][-1] if is_x else shoot[-1][0]).item()
        return p0, shoot, trajl, datal, nsteps, change
