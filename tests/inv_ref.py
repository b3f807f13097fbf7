"""Closed forms of the inverse of the discrete flow at carried points (test helper; CPU torch, in
the dtype of the inputs), built on jac_ref.vel_grad and the oracle's ODE.

step_map: F(x) - x and DF of one step map of oracle.torch_ref.LDDMM.Shoot's carried points,
    Euler  F = x + dt v(x; q, p),                              DF = I + dt A
    Ralston F = x + dt/4 v1 + 3 dt/4 v2, h = 2 dt / 3,         DF = I + dt/4 A1 + 3 dt/4 A2 (I + h A1)
    with (v1, A1) at (x; q_t, p_t) and (v2, A2) at (x + h v1; q_m, p_m).
newton_step: one update x+ = x - DF^-1 r, r = (x - y) + (F(x) - x), and res = |r|_inf per row (the
    residual of the INPUT x), with the arguments of _lib.ext_inv_step.
inverse: Newton on every step map for t = nt-1 ... 0 from x_t = x_{t+1}, with the stopping rule of
    LDDMMModel.flow_inverse (the largest finite residual <= tol or max_iter updates; the input
    iterate of the last pass is kept).
tests/test_ext_inv_host.py pins inverse against the oracle's Shoot in float64; the GPU tests
(tests/test_gpu_ext_inv.py) compare the kernel and the methods built on it with these.
"""
import torch

import jac_ref as J


def step_map(x, q, p, sigma, eta, dt, v1=None, A1=None):
    """(F(x) - x, DF): v1 None = Euler at (x; q, p); otherwise the Ralston second stage, (q, p)
    the mid-state."""
    D = x.shape[1]
    eye = torch.eye(D, dtype=x.dtype)
    if v1 is None:
        v, A = J.vel_grad(x, q, p, sigma, eta)
        return dt * v, eye + dt * A
    h = 2 * dt / 3
    v2, A2 = J.vel_grad(x + h * v1, q, p, sigma, eta)
    return (0.25 * dt) * v1 + (0.75 * dt) * v2, eye + (0.25 * dt) * A1 + (0.75 * dt) * (A2 @ (eye + h * A1))


def newton_step(x, y, q, p, sigma, eta, dt, v1=None, A1=None):
    """(x_next, res) as _lib.ext_inv_step."""
    inc, DF = step_map(x, q, p, sigma, eta, dt, v1, A1)
    r = (x - y) + inc
    return x - _solve(DF, r), r.abs().amax(dim=1)


def _solve(DF, r):
    """DF^-1 r per row by cofactors (D = 2, 3): non-finite where DF is singular, no exception."""
    D = r.shape[1]
    if D == 2:
        a, b, c, d = DF[:, 0, 0], DF[:, 0, 1], DF[:, 1, 0], DF[:, 1, 1]
        det = a * d - b * c
        return torch.stack([d * r[:, 0] - b * r[:, 1], a * r[:, 1] - c * r[:, 0]], 1) / det[:, None]
    r0, r1, r2 = DF[:, 0], DF[:, 1], DF[:, 2]
    c0, c1, c2 = torch.linalg.cross(r1, r2), torch.linalg.cross(r2, r0), torch.linalg.cross(r0, r1)
    det = (r0 * c0).sum(-1)
    adj = torch.stack([c0, c1, c2], 2)
    return (adj @ r[:, :, None])[:, :, 0] / det[:, None]


def support_states(ref, q0, p0):
    """[(q_t, p_t, q_m, p_m)] for t < nt from the oracle's own ODE (q_m, p_m: Ralston's mid-state,
    None for Euler)."""
    dt = 1.0 / ref.nt
    zero = torch.zeros(1, dtype=q0.dtype)
    q, p, out = q0, p0, []
    for _ in range(ref.nt):
        vq, mG, _ = ref.ODE(q, p, zero)
        if ref.scheme == "Euler":
            out.append((q, p, None, None))
            q, p = q + dt * vq, p + dt * mG
            continue
        h = 2 * dt / 3
        qm, pm = q + h * vq, p + h * mG
        vq2, mG2, _ = ref.ODE(qm, pm, zero)
        out.append((q, p, qm, pm))
        q, p = q + (0.25 * dt) * (vq + 3 * vq2), p + (0.25 * dt) * (mG + 3 * mG2)
    return out


def inverse(ref, q0, p0, y1, tol, max_iter=10):
    """(x0, info) of LDDMMModel.flow_inverse for the flow of ref.Shoot(q0, p0, x0): rows that did
    not converge are NaN; info = dict(converged, residual, iterations, passes)."""
    dt = 1.0 / ref.nt
    states = support_states(ref, q0, p0)
    y = y1
    N = y.shape[0]
    worst = torch.zeros(N, dtype=y.dtype)
    iterations = [0] * ref.nt
    passes = 0
    nan = float("nan")
    for t in range(ref.nt - 1, -1, -1):
        q, p, qm, pm = states[t]
        x, k = y, 0
        while True:
            if qm is None:
                xn, res = newton_step(x, y, q, p, ref.sigma, ref.eta, dt)
                passes += 1
            else:
                v1, A1 = J.vel_grad(x, q, p, ref.sigma, ref.eta)
                xn, res = newton_step(x, y, qm, pm, ref.sigma, ref.eta, dt, v1, A1)
                passes += 2
            finite = torch.isfinite(res) & torch.isfinite(xn).all(dim=1)
            res = torch.where(finite, res, torch.full_like(res, nan))
            rmax = float(torch.where(finite, res, torch.zeros_like(res)).max()) if N else 0.0
            if rmax <= tol or k >= max_iter:
                break
            x, k = xn, k + 1
        iterations[t] = k
        worst = torch.maximum(worst, res)
        y = torch.where(finite[:, None], x, torch.full_like(x, nan))
    converged = worst <= tol
    x0 = torch.where(converged[:, None], y, torch.full_like(y, nan))
    return x0, dict(converged=converged, residual=worst, iterations=iterations, passes=passes)


SIG, NT, LAM = 0.15, 10, 500.0
# (D, version, scheme, momentum scale): the unit-box probe at 700 carried / 500 support points
TABLE = [(D, v, s, 1.0) for v in ("hybrid", "logdet") for s in ("Euler", "Ralston") for D in (2, 3)]
STRONG = [(2, "hybrid", "Euler", 3.0), (2, "logdet", "Ralston", 3.0)]


def case(N, M, D, seed):
    """x (N, D), q (M, D) in the unit box, p = 0.02 randn (float64), as tests/test_gpu_ext_jac.py."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, D, generator=g, dtype=torch.float64)
    q = torch.rand(M, D, generator=g, dtype=torch.float64)
    p = 0.02 * torch.randn(M, D, generator=g, dtype=torch.float64)
    return x, q, p


def flow_case(D, version, scheme, scale=1.0, N=700, M=500):
    """(ref, x, q, p) of the probe: the oracle's model and the inputs of seed 5 + D."""
    from oracle import torch_ref as R
    x, q, p = case(N, M, D, 5 + D)
    ref = R.LDDMM(SIG, D, LAM, version == "logdet", True, scheme=scheme, nt=NT)
    return ref, x, q, scale * p
