"""Lanczos iteration with full reorthogonalisation for the extreme eigenvalues of a symmetric
operator known only through its product (LDDMMModel.loss_hessian_extremes: the Hessian of a
registration loss through loss_hvp).  The basis vectors live where the operator does (device,
dtype of v0); the projections' coefficients and the small tridiagonal algebra are float64 on the
host.  torch and numpy only."""
import numpy as np
import torch


def lanczos(matvec, v0, steps, breakdown=1e-10):
    """matvec: v (n,) -> A v (n,), A symmetric; v0: a non-zero start (n,); steps: iterations, at
    most n are run.  Every new vector is orthogonalised against the whole basis, twice (classical
    Gram-Schmidt with one repeat), so the Ritz values do not duplicate as they converge and `steps
    = n` reproduces the spectrum.  Stops early when the residual norm falls below `breakdown` times
    the largest |alpha|, |beta| seen (an invariant subspace).  Returns (ritz, vectors): the Ritz
    values in ascending order (numpy float64, m <= steps of them) and the two extreme unit Ritz
    vectors as a tensor (2, n), smallest first."""
    n = v0.numel()
    steps = max(0, min(int(steps), n))
    nrm = float(v0.double().norm())
    if steps == 0 or not nrm > 0:
        return np.zeros(0), v0.new_zeros((2, n))
    V = [v0 / nrm]
    alpha, beta = [], []
    scale = 0.0
    for k in range(steps):
        w = matvec(V[k])
        a = float(torch.dot(w.double(), V[k].double()))
        alpha.append(a)
        scale = max(scale, abs(a))
        if k == steps - 1:
            break
        B = torch.stack(V)                                     # (k + 1, n)
        for _ in range(2):
            c = (B.double() @ w.double()).to(w.dtype)
            w = w - c @ B
        b = float(w.double().norm())
        if not b > breakdown * max(scale, b):
            break
        scale = max(scale, b)
        beta.append(b)
        V.append(w / b)
    m = len(alpha)
    Tm = np.diag(np.asarray(alpha, dtype=np.float64))
    if m > 1:
        off = np.asarray(beta[:m - 1], dtype=np.float64)
        Tm += np.diag(off, 1) + np.diag(off, -1)
    ritz, Y = np.linalg.eigh(Tm)
    B = torch.stack(V[:m])
    ext = torch.as_tensor(Y[:, [0, m - 1]].T.copy()).to(device=B.device, dtype=B.dtype)   # (2, m)
    vecs = ext @ B
    vecs = vecs / vecs.norm(dim=1, keepdim=True)
    return ritz, vecs
