"""Registration facade (mirror of diffICP/core/registrations.py:21-87, LDDMM part)."""
import warnings

import torch

from .LDDMM import LDDMMModel


def _inv_small(J):
    """Inverses of the (N, D, D) matrices J, D = 2 or 3, by cofactors (non-finite where singular)."""
    D = J.shape[-1]
    if D == 2:
        a, b, c, d = J[:, 0, 0], J[:, 0, 1], J[:, 1, 0], J[:, 1, 1]
        adj = torch.stack([d, -b, -c, a], 1).reshape(-1, 2, 2)
        return adj / (a * d - b * c)[:, None, None]
    if D != 3:
        return torch.linalg.inv(J)
    r0, r1, r2 = J[:, 0], J[:, 1], J[:, 2]
    c0, c1, c2 = torch.linalg.cross(r1, r2), torch.linalg.cross(r2, r0), torch.linalg.cross(r0, r1)
    det = (r0 * c0).sum(-1)
    return torch.stack([c0, c1, c2], 2) / det[:, None, None]


class Registration:
    def apply(self, X: torch.Tensor):
        pass

    def backward(self, Y: torch.Tensor):
        """The reference's backward map; not the inverse of apply() (that is inverse())."""
        pass

    def inverse(self, Y: torch.Tensor):
        """X with apply(X) = Y."""
        pass

    def shoot(self, X: torch.Tensor, backward=False):
        pass


class LDDMMRegistration(Registration):
    """Apply the LDDMM diffeomorphism of (q0, a0) to external points (registrations.py:47-87)."""

    def __init__(self, LMi: LDDMMModel, q0: torch.Tensor, a0: torch.Tensor):
        self.LMi = LMi
        self.q0 = q0
        self.a0 = a0

    def shoot(self, X, backward=False, previous_forwardshoot=None):
        if not backward:
            if previous_forwardshoot is not None:
                warnings.warn("variable 'previous_forwardshoot' is useless when backward=False "
                              "[default]", RuntimeWarning)
            return self.LMi.Shoot(self.q0, self.a0, X)
        if previous_forwardshoot is None:
            previous_forwardshoot = self.shoot(None)
        q1k, a1k = previous_forwardshoot[-1][0], previous_forwardshoot[-1][1]
        return self.LMi.Shoot(q1k, -a1k, X)

    def apply(self, X):
        """Y = phi_1(X) = Shoot(q0, a0, X)[-1][3]  (registrations.py:72-77)."""
        return self.shoot(X)[-1][3]

    def backward(self, Y, previous_forwardshoot=None):
        """The reference's backward map: the shooting of Y from (q1, -a1) (registrations.py:80-87).
        It is NOT the inverse of the map apply() computes: it inverts the continuous flow only,
        and only where the field is odd in the momenta (eta = 0).  The inverse is inverse()."""
        return self.shoot(Y, backward=True, previous_forwardshoot=previous_forwardshoot)[-1][3]

    # ------------------------------------------------------------------------------------
    # The registration as a tangent vector (extension; core/statistics.py)
    def tangent_field(self, side="source"):
        """The momenta (q, p) whose velocity field is this registration's tangent vector, detached:
        side "source": (q0, a0), the initial field, in the space apply() starts from; "target":
        (q1, -p1) of the forward shoot (formed with its final momenta), the state the reference's
        `backward` shoots from, in the space apply() arrives in.  Nothing of the model changes."""
        if side == "source":
            return self.q0.detach(), self.a0.detach()
        if side != "target":
            raise ValueError(f"unknown side : {side}. Choices are 'source' or 'target'")
        Q, P = self.LMi._support_states(self.q0.detach(), self.a0.detach(), need_p1=True)
        return Q[-1], -P[-1]

    # ------------------------------------------------------------------------------------
    # First-order change of the map with its momenta (extension; LDDMMModel.shoot_tangent)
    def sensitivity(self, X, da0, dq0=None, previous_forwardshoot=None):
        """d apply(X) along the change da0 of the initial momenta (and dq0 of the support points;
        None: zero): (L, N, D) for da0 (L, M, D), (N, D) for a 2-D da0 -- shoot_tangent's dX with the
        points X held fixed.  previous_forwardshoot: a forward shoot of (q0, a0) to reuse.  Only
        for eta = 0.  Inputs are detached; nothing of the model changes."""
        return self.LMi._shoot_tangent(self.q0, self.a0, da0, dq0, X, None, previous_forwardshoot, False,
                                       False)[2]

    def jacobi_field(self, da0, previous_forwardshoot=None):
        """The Jacobi field along the geodesic of (q0, a0) started by the change da0 of the initial
        momenta with the support points held fixed: (dQ, dP) at all nt + 1 times, (nt + 1, L, M, D)
        or (nt + 1, M, D) for a 2-D da0; it starts at (0, da0).  Only for eta = 0."""
        return self.LMi.shoot_tangent(self.q0, self.a0, da0, shoot=previous_forwardshoot, trajectory=True)[:2]

    # ------------------------------------------------------------------------------------
    # Exact inverse of the map apply() computes (extension; LDDMMModel.flow_inverse)
    def inverse(self, Y, previous_forwardshoot=None, tol=None, max_iter=10, return_info=False):
        """X with apply(X) = Y: the inverse of the discrete flow itself, by Newton's iteration on
        every step map (LDDMMModel.flow_inverse; tol in coordinate units, None: 1e-6 of the
        larger of sigma and max |Y|).  Rows that do not converge within max_iter updates per
        step are NaN (one RuntimeWarning).  previous_forwardshoot: a forward shoot of (q0, a0)
        to reuse.  return_info: (X, info), info as flow_inverse returns it.  Y is detached;
        nothing of the model changes."""
        X, info = self.LMi.flow_inverse(self.q0, self.a0, Y, shoot=previous_forwardshoot, tol=tol,
                                        max_iter=max_iter)
        return (X, info) if return_info else X

    def inverse_with_jacobian(self, Y):
        """(X, Jinv): X = inverse(Y) and Jinv[i] = d X_i / d Y_i, the inverse of jacobian(X)[i]
        (formed in float64, returned as float32); NaN where X is NaN."""
        X = self.inverse(Y)
        Jinv = _inv_small(self.jacobian(X).double()).to(X.dtype)     # NaN rows of X: NaN rows of J
        bad = torch.isnan(X).any(dim=1)
        return X, torch.where(bad[:, None, None], torch.full_like(Jinv, float("nan")), Jinv)

    # ------------------------------------------------------------------------------------
    # Local behaviour of the map (extension; LDDMMModel.flow_jacobian)
    def _jac_flow(self, X, backward=False, previous_forwardshoot=None):
        LM = self.LMi
        if not backward:
            return LM.flow_jacobian(self.q0, self.a0, X, shoot=previous_forwardshoot)
        if previous_forwardshoot is None:
            Q, P = LM._support_states(self.q0.detach(), self.a0.detach(), need_p1=True)
        else:
            LM.complete_shoot(previous_forwardshoot)
            Q, P = previous_forwardshoot.Q.detach(), previous_forwardshoot.P.detach()
        return LM.flow_jacobian(Q[-1], -P[-1], X)

    def jacobian(self, X, backward=False, previous_forwardshoot=None):
        """J (N, D, D), J[i] = d phi(X_i) / d X_i of the map apply() computes (backward=True: of
        the map backward() computes, the shooting from (q1, -a1)).  previous_forwardshoot: a
        forward shoot of (q0, a0) to reuse.  X is detached; nothing of the model changes."""
        return self._jac_flow(X, backward, previous_forwardshoot)[1]

    def apply_with_jacobian(self, X):
        """(Y, J): Y = apply(X) and its Jacobian, from one pass over the trajectory."""
        return self._jac_flow(X)

    def log_jacobian_det(self, X):
        """log det J at every point of X, (N,): the local volume change of apply().  The
        determinant is formed in float64 from G = J - I and returned as float32; NaN where
        det J <= 0 (the discrete map folds there)."""
        J = self.jacobian(X)
        D = J.shape[-1]
        G = J.double() - torch.eye(D, device=J.device, dtype=torch.float64)
        # det(I + G) - 1 from the entries of G: no cancellation against the unit diagonal
        if D == 2:
            e = G[:, 0, 0] + G[:, 1, 1] + G[:, 0, 0] * G[:, 1, 1] - G[:, 0, 1] * G[:, 1, 0]
        else:
            tr = G.diagonal(dim1=1, dim2=2).sum(-1)
            m2 = 0.5 * (tr * tr - (G @ G).diagonal(dim1=1, dim2=2).sum(-1))   # sum of principal 2-minors
            e = tr + m2 + torch.linalg.det(G)
        out = torch.log1p(e)
        return torch.where(e > -1.0, out, torch.full_like(out, float("nan"))).float()
