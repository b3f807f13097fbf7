"""Registration facade (mirror of diffICP/core/registrations.py:21-87, LDDMM part)."""
import warnings

import torch

from .LDDMM import LDDMMModel


class Registration:
    def apply(self, X: torch.Tensor):
        pass

    def backward(self, Y: torch.Tensor):
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
        return self.shoot(Y, backward=True, previous_forwardshoot=previous_forwardshoot)[-1][3]

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
