"""Tangent-space statistics of a fitted atlas (extension, no reference counterpart): principal
component analysis of the frames' initial velocity fields in the RKHS V of the deformation
kernel -- the standard analysis of an LDDMM atlas (its main modes of variation, and where each
subject sits on them).

The fields v_k(x) = sum_i K(x - q_ki) p_ki (eta = 0) live on their own supports; everything here
needs only their inner products
    G_jk = <v_j, v_k>_V = sum_i sum_i' (p_ji . p_ki') exp(-|q_ji - q_ki'|^2 / 2 sigma^2),
which LDDMMModel.field_gram forms in one fused pass with float64 totals (csrc/gram.hip).  With
H = I - 11^T / K the centred Gram matrix H G H = U Lambda U^T is diagonalised in float64 on the
host; mode l is the unit-norm field e_l = sum_k (U_kl / sqrt lambda_l) v_k, frame k has the score
U_kl sqrt lambda_l on it, and the variance along it is lambda_l / (K - 1).
"""
from __future__ import annotations

import math

import torch

from .registrations import LDDMMRegistration


class TangentPCA:
    """Result of TangentPCA.fit.  Host float64 attributes:
      gram (K, K)                 G_jk = <v_j, v_k>_V
      eigenvalues (L,)            lambda of H G H, descending, the kept ones
      variances (L,)              lambda / (K - 1)
      explained_variance_ratio (L,)  lambda / sum of the positive eigenvalues of H G H
      scores (K, L)               U sqrt(Lambda): frame k's coordinate on mode l
      coefficients (K, L)         U / sqrt(Lambda): mode l is the unit-norm field
                                  sum_k coefficients[k, l] v_k
    and LM, fields (the detached (q, p) pairs), rtol."""

    # Modes with lambda_l <= rtol lambda_0 are dropped.  The default sits above the noise floor
    # of the Gram entries: centring subtracts the large common part of G, and what float32 pair
    # terms under float64 totals leave behind shows up as spurious eigenvalues of about 4e-9
    # lambda_0 (a CPU probe of a rank-1 family of 6 fields of 200 points; 2e-8 with float32
    # totals, 4e-16 in float64 throughout).  1e-6 keeps two orders of magnitude above that.
    DEFAULT_RTOL = 1e-6

    @classmethod
    def fit(cls, LM, fields, rtol=DEFAULT_RTOL):
        """PCA of the velocity fields of `fields` = [(q, p), ...] (K >= 2 fields on the spec of
        the eta = 0 model LM, each on its own support).  One field_gram call."""
        fields = [(q.detach(), p.detach()) for q, p in fields]
        K = len(fields)
        if K < 2:
            raise ValueError("TangentPCA needs at least 2 fields")
        self = cls()
        self.LM, self.fields, self.rtol = LM, fields, float(rtol)
        G = LM.field_gram(fields).detach().to("cpu", torch.float64)
        self.gram = G
        H = torch.eye(K, dtype=torch.float64) - 1.0 / K
        C = H @ G @ H
        lam, U = torch.linalg.eigh(0.5 * (C + C.t()))
        lam, U = lam.flip(0), U.flip(1)
        keep = int((lam > self.rtol * lam[0]).sum()) if float(lam[0]) > 0 else 0
        total = float(lam.clamp(min=0).sum())
        self.eigenvalues = lam[:keep].clone()
        self._U = U[:, :keep].clone()
        root = self.eigenvalues.sqrt()
        self.variances = self.eigenvalues / (K - 1)
        self.explained_variance_ratio = self.eigenvalues / total if keep else self.eigenvalues.clone()
        self.scores = self._U * root
        self.coefficients = self._U / root
        return self

    @property
    def K(self):
        return len(self.fields)

    @property
    def L(self):
        return int(self.eigenvalues.numel())

    def distances(self):
        """(K, K) RKHS distances |v_j - v_k|_V: d^2 = G_jj + G_kk - 2 G_jk, clamped at 0."""
        d = self.gram.diagonal()
        return (d[:, None] + d[None, :] - 2 * self.gram).clamp(min=0).sqrt()

    def project(self, field):
        """Scores (L,) of a new field (q, p) on the kept modes: s_l = sum_k coefficients[k, l]
        (g_k - mean_j G_jk - mean_j g_j + mean_ij G_ij) with g_k = <v_k, v>_V (one field_gram
        call).  A training field gives its row of `scores`."""
        g = self.LM.field_gram(self.fields, [field]).detach().to("cpu", torch.float64)[:, 0]
        c = g - self.gram.mean(0) - g.mean() + self.gram.mean()
        return self.coefficients.t() @ c

    def mode_weights(self, l=None, t=0.0):
        """(K,) weights w with "mean + t standard deviations of mode l" = sum_k w_k v_k:
        w_k = 1 / K + t U[k, l] / sqrt(K - 1) (they sum to 1).  l None or t = 0: the mean."""
        K = self.K
        w = torch.full((K,), 1.0 / K, dtype=torch.float64)
        if l is not None and t != 0:
            if not 0 <= int(l) < self.L:
                raise IndexError(f"mode {l} of {self.L} kept modes")
            w = w + float(t) * self._U[:, int(l)] / math.sqrt(K - 1)
        return w

    def mode_field(self, l=None, t=0.0):
        """The field "mean + t standard deviations of mode l" as momenta (q, p) on the union
        support: the points of all fields one after the other, the momenta of field k scaled by
        mode_weights(l, t)[k]."""
        w = self.mode_weights(l, t)
        q = torch.cat([f[0] for f in self.fields], dim=0).contiguous()
        p = torch.cat([f[1] * float(w[k]) for k, f in enumerate(self.fields)], dim=0).contiguous()
        return q, p

    def mode_registration(self, l, t, support=None, **v2p_args):
        """The deformation of "mean + t standard deviations of mode l".
        support None: an LDDMMRegistration on the union support (K times the points).
        support (S, D), e.g. the template centres or a grid: the field is evaluated there
        (LM.v) and projected onto momenta on `support` (LM.v2p, by default version="ridge_keops",
        the device conjugate gradients, which scale); returns (registration, relative_residual)
        with relative_residual = |v(support) - target| / |target| of the projected field."""
        q, p = self.mode_field(l, t)
        if support is None:
            return LDDMMRegistration(self.LM, q, p)
        support = support.detach().contiguous()
        args = {"version": "ridge_keops"}
        args.update(v2p_args)
        with torch.no_grad():
            target = self.LM.v(support, q, p)
            ps = self.LM.v2p(support, target, **args)
            got = self.LM.v(support, support, ps)
            den = float(target.double().norm())
            res = float((got.double() - target.double()).norm()) / den if den > 0 else 0.0
        return LDDMMRegistration(self.LM, support, ps.contiguous()), res
