"""Closed forms of the second-order operator of the eta = 0 shooting (test helper; CPU torch, any
dtype), the second-order adjoint recursions built on them, and the inputs the host and the GPU
tests share.

With H(q, p) = 1/2 sum_ij K_ij p_i.p_j, s = 1/sigma^2, z = q_i - q_j, K = exp(-s |z|^2 / 2) and
directions a = (a_q, a_p), b = (b_q, b_p): alpha = a_q,i - a_q,j, beta = b_q,i - b_q,j,
  P = p_i.p_j, P_a = a_p,i.p_j + p_i.a_p,j, P_b likewise, P_ab = a_p,i.b_p,j + b_p,i.a_p,j,
  A = s^2 (z.alpha)(z.beta) - s (alpha.beta), c = A P - s (z.alpha) P_b - s (z.beta) P_a + P_ab.
d2h:  D^2 H(S)[a, .], the operator the VJP (a = u(l) = (-l_p, l_q)) and the TLM share:
        (.)_p,i = sum_j K [ a_p,j - s (z.alpha) p_j ]
        (.)_q,i = sum_j K [ s^2 (z.alpha) P z - s P_a z - s P alpha ]
third: T(S; a, b) = grad_S (D^2 H(S)[a, b]):
        T_p,i = sum_j K { A p_j - s (z.alpha) b_p,j - s (z.beta) a_p,j }
        T_q,i = sum_j K { -s c z + [s^2 (z.beta) P - s P_b] alpha + [s^2 (z.alpha) P - s P_a] beta }
cost_grad, cost_hess: gradient and Hessian-vector product of C(q, p) = s sum_ij K (z.p_j), the
      oracle's mdivsum(q, q, p) at eta = 0; with w = p_j - p_i, dw = b_p,j - b_p,i:
        (grad C)_p,i = -s sum_j K z,     (grad C)_q,i = s sum_j K [ w - s (z.w) z ]
        (D^2 C b)_p,i = s sum_j K [ s (z.beta) z - beta ]
        (D^2 C b)_q,i = s sum_j K { -s [-s (z.beta)(z.w) + beta.w + z.dw] z - s (z.w) beta
                                    - s (z.beta) w + dw }
loss_hvp: Hessian-vector products of L(p0) = lam H(q0, p0) + cost_nt + data(q_nt) by the
      second-order adjoint of the Euler / Ralston shooting (or the Gauss-Newton product
      J^T H_data J d), the base states integrated by the oracle's own ODE in the inputs' dtype.
oracle_hvp, oracle_hessian, oracle_gauss_newton: the same by autograd through ref.Shoot -- the arbiter.
ode_hvp, ode_self_bwd: stand-ins with the signatures of _lib's (float64 inside), for the host tests.
"""
import torch

from tlm_ref import (CHUNK, FLOW_L, FLOW_M, FLOW_NT, FLOW_SIGMAS, PASS_CASES, SIZES, TOL32, TOL64,  # noqa: F401
                     nerr, oracle, r32, r64, shoot_tangent, tlm)


def _rows(fn, M):
    outs = [fn(a, min(a + CHUNK, M)) for a in range(0, M, CHUNK)]
    return tuple(torch.cat([o[k] for o in outs], -2) for k in range(len(outs[0])))


def _zK(q, a, b, s):
    z = q[a:b, None, :] - q[None, :, :]                        # (n, M, D)
    return z, torch.exp(-0.5 * s * (z * z).sum(-1))            # (n, M)


def _sym(ui, u, vi, v):
    """u_i.v_j + v_i.u_j for rows ui, vi (n, D) or (L, n, D) against columns u, v."""
    return ui @ v.transpose(-1, -2) + vi @ u.transpose(-1, -2)


def d2h(q, p, aq, ap, sigma):
    """D^2 H(S)[a, .] as (out_q, out_p), (M, D)."""
    s = 1.0 / sigma ** 2

    def rows(a, b):
        z, K = _zK(q, a, b, s)
        za = s * (z * (aq[a:b, None] - aq[None])).sum(-1)       # s (z.alpha)
        P = p[a:b] @ p.t()
        Pa = _sym(ap[a:b], ap, p[a:b], p)
        out_p = K @ ap - (K * za) @ p
        alpha = aq[a:b, None] - aq[None]
        out_q = s * (torch.einsum("nm,nmd->nd", K * (za * P - Pa), z) - torch.einsum("nm,nmd->nd", K * P, alpha))
        return out_q, out_p
    return _rows(rows, q.shape[0])


def third(q, p, aq, ap, bq, bp, sigma):
    """T(S; a, b_l) as (out_q, out_p), (L, M, D): a (M, D) shared, bq, bp (L, M, D)."""
    s = 1.0 / sigma ** 2

    def rows(a, b):
        z, K = _zK(q, a, b, s)
        alpha = aq[a:b, None] - aq[None]                        # (n, M, D)
        beta = bq[:, a:b, None] - bq[:, None]                   # (L, n, M, D)
        za = s * (z * alpha).sum(-1)                            # (n, M)
        zb = s * (z * beta).sum(-1)                             # (L, n, M)
        A = za * zb - s * (alpha * beta).sum(-1)
        P = p[a:b] @ p.t()
        Pa = _sym(ap[a:b], ap, p[a:b], p)
        Pb = _sym(bp[:, a:b], bp, p[a:b], p)
        Pab = bp[:, a:b] @ ap.t() + ap[a:b] @ bp.transpose(-1, -2)
        out_p = (K * A) @ p - (K * za) @ bp - (K * zb) @ ap
        c = A * P - za * Pb - zb * Pa + Pab
        out_q = s * (-torch.einsum("lnm,nmd->lnd", K * c, z) + torch.einsum("lnm,nmd->lnd", K * (zb * P - Pb), alpha)
                     + torch.einsum("nm,lnmd->lnd", K * (za * P - Pa), beta))
        return out_q, out_p
    return _rows(rows, q.shape[0])


def cost(q, p, sigma):
    """C(q, p) = s sum_ij K (z.p_j)."""
    s = 1.0 / sigma ** 2
    z, K = _zK(q, 0, q.shape[0], s)
    return s * (K * (z * p[None]).sum(-1)).sum()


def cost_grad(q, p, sigma):
    s = 1.0 / sigma ** 2

    def rows(a, b):
        z, K = _zK(q, a, b, s)
        w = p[None] - p[a:b, None]
        zw = (z * w).sum(-1)
        out_p = -s * torch.einsum("nm,nmd->nd", K, z)
        out_q = s * (torch.einsum("nm,nmd->nd", K, w) - s * torch.einsum("nm,nmd->nd", K * zw, z))
        return out_q, out_p
    return _rows(rows, q.shape[0])


def cost_hess(q, p, bq, bp, sigma):
    """D^2 C(S) b_l as (out_q, out_p), (L, M, D)."""
    s = 1.0 / sigma ** 2

    def rows(a, b):
        z, K = _zK(q, a, b, s)
        beta = bq[:, a:b, None] - bq[:, None]
        w = p[None] - p[a:b, None]                              # (n, M, D)
        dw = bp[:, None] - bp[:, a:b, None]                     # (L, n, M, D)
        zb = s * (z * beta).sum(-1)
        zw = (z * w).sum(-1)
        e = -zb * zw + (beta * w).sum(-1) + (z * dw).sum(-1)
        out_p = s * (torch.einsum("lnm,nmd->lnd", K * zb, z) - torch.einsum("nm,lnmd->lnd", K, beta))
        out_q = s * (-s * torch.einsum("lnm,nmd->lnd", K * e, z) - s * torch.einsum("nm,lnmd->lnd", K * zw, beta)
                     - torch.einsum("lnm,nmd->lnd", K * zb, w) + torch.einsum("nm,lnmd->lnd", K, dw))
        return out_q, out_p
    return _rows(rows, q.shape[0])


def hvp_pass(q, p, aq, ap, bq, bp, sigma, gdiv=None):
    """What the kernel computes: T(S; a, b_l) + gdiv D^2 C(S) b_l, (out_q, out_p)."""
    oq, op = third(q, p, aq, ap, bq, bp, sigma)
    if gdiv is not None:
        cq, cp = cost_hess(q, p, bq, bp, sigma)
        oq, op = oq + gdiv * cq, op + gdiv * cp
    return oq, op


def vjp(q, p, lq, lp, sigma, gdiv=None):
    """DF(S)^T l (+ gdiv grad C): what _lib.ode_self_bwd(q, p, gv = lq, gmG = lp, gdiv) returns."""
    gq, gp = d2h(q, p, -lp, lq, sigma)
    if gdiv is not None:
        cq, cp = cost_grad(q, p, sigma)
        gq, gp = gq + gdiv * cq, gp + gdiv * cp
    return gq, gp


# stand-ins for the library calls (float64 inside, the inputs' dtype and device outside)
def _d(t):
    return None if t is None else t.detach().double().cpu()


def _back(outs, like):
    return tuple(o.to(dtype=like.dtype, device=like.device).contiguous() for o in outs)


def ode_hvp(q, p, aq, ap, bq, bp, sigma, gdiv=None):
    g = None if gdiv is None else float(gdiv.reshape(-1)[0])
    return _back(hvp_pass(_d(q), _d(p), _d(aq), _d(ap), _d(bq), _d(bp), sigma, g), q)


def ode_self_bwd(q, p, gv, gmG, gdiv, sigma, eta):
    assert eta == 0
    g = None if gdiv is None else float(gdiv.reshape(-1)[0])
    return _back(vjp(_d(q), _d(p), _d(gv), _d(gmG), sigma, g), q)


# ---------------------------------------------------------------------------------------
# second-order adjoint
def states(ref, q0, p0):
    """The support states S_t of ref.Shoot, t = 0 .. nt."""
    return [(s[0], s[1]) for s in ref.Shoot(q0, p0)]


def _vjp_dirs(q, p, dlq, dlp, sigma):
    outs = [vjp(q, p, dlq[l], dlp[l], sigma) for l in range(dlq.shape[0])]
    return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])


def loss_hvp(ref, q0, p0, d, data_grad, data_hvp, gauss_newton=False):
    """Hessian-vector products (L, M, D) of L(p0) = lam H(q0, p0) + cost_nt + data(q_nt) along d
    (L, M, D): data_grad(q1) -> (M, D), data_hvp(q1, dq1 (L, M, D)) -> (L, M, D).  gauss_newton:
    J^T H_data J d alone."""
    assert ref.eta == 0
    sg, nt = ref.sigma, ref.nt
    dt = 1.0 / nt
    h = 2 * dt / 3
    gam = None if (gauss_newton or not ref.withlogdet) else 1.0
    euler = ref.scheme == "Euler"
    S = states(ref, q0, p0)
    dQ, dP, _ = shoot_tangent(ref, q0, p0, torch.zeros_like(d), d, trajectory=True)
    q1 = S[nt][0]
    lq, lp = data_grad(q1), torch.zeros_like(q1)
    dlq, dlp = data_hvp(q1, dQ[nt]), torch.zeros_like(d)
    zero = torch.zeros(1, dtype=q0.dtype)
    sc = lambda k, g: None if g is None else k * g
    for t in range(nt - 1, -1, -1):
        q, p = S[t]
        dq, dp = dQ[t], dP[t]
        if euler:
            gq, gp = _vjp_dirs(q, p, dlq, dlp, sg)
            if not gauss_newton:
                tq, tp = hvp_pass(q, p, -lp, lq, dq, dp, sg, gam)
                gq, gp = gq + tq, gp + tp
                aq, ap = vjp(q, p, lq, lp, sg, gam)
                lq, lp = lq + dt * aq, lp + dt * ap
            dlq, dlp = dlq + dt * gq, dlp + dt * gp
            continue
        k1 = ref.ODE(q, p, zero)
        qm, pm = q + h * k1[0], p + h * k1[1]
        d1 = tlm(q, p, dq, dp, sg)
        dqm, dpm = dq + h * d1[0], dp + h * d1[1]
        dmq, dmp = _vjp_dirs(qm, pm, dlq, dlp, sg)
        if not gauss_newton:
            tq, tp = hvp_pass(qm, pm, -lp, lq, dqm, dpm, sg, gam)
            dmq, dmp = dmq + tq, dmp + tp
        dmq, dmp = 0.75 * dt * dmq, 0.75 * dt * dmp
        gq, gp = _vjp_dirs(q, p, 0.25 * dt * dlq + h * dmq, 0.25 * dt * dlp + h * dmp, sg)
        if not gauss_newton:
            mq, mp = vjp(qm, pm, lq, lp, sg, gam)
            mq, mp = 0.75 * dt * mq, 0.75 * dt * mp
            cq, cp = 0.25 * dt * lq + h * mq, 0.25 * dt * lp + h * mp
            tq, tp = hvp_pass(q, p, -cp, cq, dq, dp, sg, sc(0.25 * dt, gam))
            gq, gp = gq + tq, gp + tp
            aq, ap = vjp(q, p, cq, cp, sg, sc(0.25 * dt, gam))
            lq, lp = lq + mq + aq, lp + mp + ap
        dlq, dlp = dlq + dmq + gq, dlp + dmp + gp
    if gauss_newton:
        return dlp
    from oracle import torch_ref as R
    return dlp + ref.lam * torch.stack([R.KRed(q0, q0, d[l], sg) for l in range(d.shape[0])])


def quad_data(y, cmul=1.0):
    """data(x) = cmul |x - y|^2 / 2 with its gradient and Hessian-vector product."""
    loss = lambda x: ((x - y) ** 2).sum() * cmul / 2
    return loss, (lambda x: cmul * (x - y)), (lambda x, dx: cmul * dx)


def cubic_data(y, cmul=1.0):
    """A data term with a state-dependent Hessian: cmul sum |x - y|^2 (1 + |x - y|^2) / 2."""
    def loss(x):
        r2 = ((x - y) ** 2).sum(-1)
        return (r2 * (1 + r2)).sum() * cmul / 2

    def grad(x):
        r = x - y
        return cmul * r * (1 + 2 * (r * r).sum(-1, keepdim=True))

    def hvp(x, dx):
        r = x - y
        r2 = (r * r).sum(-1, keepdim=True)
        return cmul * (dx * (1 + 2 * r2) + 4 * r * (r * dx).sum(-1, keepdim=True))
    return loss, grad, hvp


def oracle_loss(ref, q0, data):
    def f(p0):
        sh = ref.Shoot(q0, p0)
        return (ref.trajloss(sh) + data(sh[-1][0])).reshape(())
    return f


def oracle_hvp(ref, q0, p0, d, data):
    """Hessian-vector products by torch.autograd.functional.hvp through ref.Shoot, one direction
    at a time."""
    f = oracle_loss(ref, q0, data)
    return torch.stack([torch.autograd.functional.hvp(f, p0, d[l])[1] for l in range(d.shape[0])])


def oracle_hessian(ref, q0, p0, data):
    n = p0.numel()
    H = torch.autograd.functional.hessian(oracle_loss(ref, q0, data), p0).reshape(n, n)
    return 0.5 * (H + H.t())


def oracle_gauss_newton(ref, q0, p0, d, data_hvp):
    """J^T H_data J d with J = d q_nt / d p0 formed densely by autograd."""
    n = p0.numel()
    J = torch.autograd.functional.jacobian(lambda p: ref.Shoot(q0, p)[-1][0], p0).reshape(n, n)
    q1 = ref.Shoot(q0, p0)[-1][0]
    Jd = (d.reshape(-1, n) @ J.t()).reshape(d.shape)
    return (data_hvp(q1, Jd).reshape(-1, n) @ J).reshape(d.shape)


# ---------------------------------------------------------------------------------------
# shared inputs (float64 on the CPU; the tests round them to float32)
def pass_inputs(D, M, L, shift, seed=0):
    """Support points in the unit box moved by `shift`, momenta 0.05 randn, directions of unit
    scale in every slot (as tlm_ref.pass_inputs)."""
    g = torch.Generator().manual_seed(2000 * seed + 31 * M + D)
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    q = torch.rand(M, D, generator=g, dtype=torch.float64) + shift
    return dict(q=q, p=0.05 * r(M, D), aq=0.1 * r(M, D), ap=0.05 * r(M, D), bq=0.1 * r(L, M, D),
                bp=0.05 * r(L, M, D))


def flow_inputs(D, seed=0, M=FLOW_M, L=FLOW_L):
    g = torch.Generator().manual_seed(91 + 10 * seed + D)
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    q0 = torch.rand(M, D, generator=g, dtype=torch.float64)
    return dict(q0=q0, p0=0.05 * r(M, D), y=q0 + 0.05 * r(M, D), d=r(L, M, D))
