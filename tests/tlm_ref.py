"""Closed forms of the tangent-linear model (TLM) of the eta = 0 shooting (test helper; CPU torch,
any dtype) and the inputs the host and the GPU tests share.

tlm: the linearisation of oracle.torch_ref.LDDMM.ODE at (q, p) -- and of v at carried points x --
    along L directions (dq, dp, dx).  With s = 1/sigma^2, K = exp(-s |z|^2 / 2):
      self rows (z = q_i - q_j, dz = dq_i - dq_j):
        dv_i  = sum_j K [ dp_j - s (z.dz) p_j ]
        dmG_i = s sum_j K [ (dp_i.p_j + p_i.dp_j) z + (p_i.p_j) dz - s (p_i.p_j)(z.dz) z ]
      carried rows (z = x_i - q_j, dz = dx_i - dq_j):
        dvx_i = sum_j K [ dp_j - s (z.dz) p_j ]
shoot_tangent: the tangent of the discrete flow of ref.Shoot (Euler and Ralston) by these formulas,
    the base states integrated by the oracle's own ODE in the dtype of the inputs.
oracle_jvp: the same quantity by torch.autograd.functional.jvp through ref.Shoot -- the arbiter.
ode_tlm: a stand-in with the signature of _lib.ode_tlm (float64 inside), for the host tests.
tests/test_tlm_host.py pins tlm and shoot_tangent against oracle_jvp in float64 and bounds their
float32 restatement; tests/test_gpu_tlm.py compares the kernel and LDDMMModel.shoot_tangent with them.
"""
import torch

CHUNK = 256

# norm-wise tolerances: the kernel against float64 on the float32-rounded inputs, two
# float32 kernels against each other; the restatement must stay below half the first
TOL64, TOL32 = 1e-5, 2e-5

# one pass: sizes at and around the 64-lane wave, the 256-column tile, the 512-row block and the
# first column split
SIZES = (1, 63, 64, 65, 255, 256, 257, 513, 1030)
PASS_CASES = [(D, sigma, shift) for D in (2, 3) for sigma in (0.05, 0.3, 2.0) for shift in (0.0, 100.0)]
# (M, N) drawn from SIZES so that every size is an M once and an N once
PASS_SHAPES = [(1, 1030), (63, 513), (64, 257), (65, 256), (255, 255), (256, 65), (257, 64), (513, 63),
               (1030, 1), (1030, 513)]
FLOW_M, FLOW_N, FLOW_L, FLOW_NT = 130, 70, 3, 10
FLOW_SIGMAS = (0.1, 0.3)


def _pair_terms(rows, drows, q, p, dq, dp, s):
    """z, dz, K, w = s (z.dz) of the rows against the support, shaped (L?, n, M, ...)."""
    z = rows[:, None, :] - q[None, :, :]                      # (n, M, D)
    dz = drows[:, :, None, :] - dq[:, None, :, :]             # (L, n, M, D)
    K = torch.exp(-0.5 * s * (z * z).sum(-1))                 # (n, M)
    w = s * (z[None] * dz).sum(-1)                            # (L, n, M)
    return z, dz, K, w


def _dvel(K, w, p, dp):
    """sum_j K [dp_j - s (z.dz) p_j]: (L, n, D)."""
    return torch.einsum("nm,lmd->lnd", K, dp) - torch.einsum("lnm,md->lnd", K[None] * w, p)


def tlm(q, p, dq, dp, sigma, x=None, dx=None, need_self=True):
    """(dv, dmG, dvx) in the dtype of q: dq, dp (L, M, D), dx (L, N, D); rows in chunks."""
    s = 1.0 / sigma ** 2
    L, M, D = dq.shape
    dv = dmG = dvx = None
    if need_self:
        dvs, dGs = [], []
        for a in range(0, M, CHUNK):
            b = min(a + CHUNK, M)
            z, dz, K, w = _pair_terms(q[a:b], dq[:, a:b], q, p, dq, dp, s)
            dvs.append(_dvel(K, w, p, dp))
            pp = p[a:b] @ p.t()                                                       # (n, M)
            dpp = torch.einsum("lnd,md->lnm", dp[:, a:b], p) + torch.einsum("nd,lmd->lnm", p[a:b], dp)
            c = K[None] * (dpp - w * pp[None])
            dGs.append(s * (torch.einsum("lnm,nmd->lnd", c, z) + torch.einsum("nm,lnmd->lnd", K * pp, dz)))
        dv = torch.cat(dvs, 1) if dvs else dq.new_zeros((L, 0, D))
        dmG = torch.cat(dGs, 1) if dGs else dq.new_zeros((L, 0, D))
    if x is not None:
        outs = []
        for a in range(0, x.shape[0], CHUNK):
            b = min(a + CHUNK, x.shape[0])
            _, _, K, w = _pair_terms(x[a:b], dx[:, a:b], q, p, dq, dp, s)
            outs.append(_dvel(K, w, p, dp))
        dvx = torch.cat(outs, 1) if outs else dx.new_zeros((L, 0, D))
    return dv, dmG, dvx


def ode_tlm(q, p, dq, dp, sigma, x=None, dx=None, need_self=True):
    """Stand-in for _lib.ode_tlm on any device: tlm in float64, returned in the inputs' dtype."""
    d = lambda t: None if t is None else t.detach().double().cpu()
    outs = tlm(d(q), d(p), d(dq), d(dp), sigma, d(x), d(dx), need_self)
    return tuple(None if o is None else o.to(dtype=q.dtype, device=q.device).contiguous() for o in outs)


def shoot_tangent(ref, q0, p0, dq0, dp0, x0=None, dx0=None, trajectory=False):
    """(dQ, dP, dX) of the discrete flow of ref.Shoot(q0, p0, x0) (ref: oracle.torch_ref.LDDMM with
    eta = 0) along dq0, dp0 (L, M, D), dx0 (L, N, D); trajectory: at all nt + 1 times, stacked."""
    assert ref.eta == 0
    dt = 1.0 / ref.nt
    h = 2 * dt / 3
    zero = torch.zeros(1, dtype=q0.dtype)
    carried = x0 is not None

    def ode(q, p, x):
        o = ref.ODE(q, p, zero, x) if carried else ref.ODE(q, p, zero)
        return o[0], o[1], (o[3] if carried else None)

    def lin(q, p, x, dq, dp, dx):
        return tlm(q, p, dq, dp, ref.sigma, x, dx)

    def axpy(a, k, b):                     # a + k b, None passing through
        return None if a is None else a + k * b

    q, p, x = q0, p0, x0
    dq, dp, dx = dq0, dp0, dx0
    traj = [(dq, dp, dx)]
    for _ in range(ref.nt):
        k1 = ode(q, p, x)
        d1 = lin(q, p, x, dq, dp, dx)
        if ref.scheme == "Euler":
            q, p, x = axpy(q, dt, k1[0]), axpy(p, dt, k1[1]), axpy(x, dt, k1[2])
            dq, dp, dx = axpy(dq, dt, d1[0]), axpy(dp, dt, d1[1]), axpy(dx, dt, d1[2])
        else:
            qm, pm, xm = axpy(q, h, k1[0]), axpy(p, h, k1[1]), axpy(x, h, k1[2])
            k2 = ode(qm, pm, xm)
            d2 = lin(qm, pm, xm, axpy(dq, h, d1[0]), axpy(dp, h, d1[1]), axpy(dx, h, d1[2]))
            step = lambda a, b, c: None if a is None else a + (0.25 * dt) * (b + 3 * c)
            q, p, x = step(q, k1[0], k2[0]), step(p, k1[1], k2[1]), step(x, k1[2], k2[2])
            dq, dp, dx = step(dq, d1[0], d2[0]), step(dp, d1[1], d2[1]), step(dx, d1[2], d2[2])
        traj.append((dq, dp, dx))
    if not trajectory:
        return dq, dp, dx
    return tuple(None if traj[0][k] is None else torch.stack([t[k] for t in traj]) for k in range(3))


def oracle_jvp(ref, q0, p0, dq0, dp0, x0=None, dx0=None):
    """(dQ, dP, dX) at the final time by forward-mode autograd through ref.Shoot, one direction at a
    time (torch.autograd.functional.jvp: the double-backward trick, exact in the inputs' dtype)."""
    carried = x0 is not None

    def final(*state):
        last = ref.Shoot(*state)[-1]
        return (last[0], last[1], last[3]) if carried else (last[0], last[1])

    outs = []
    for l in range(dq0.shape[0]):
        prim = (q0, p0, x0) if carried else (q0, p0)
        tang = (dq0[l], dp0[l], dx0[l]) if carried else (dq0[l], dp0[l])
        outs.append(torch.autograd.functional.jvp(final, prim, tang)[1])
    dQ, dP = torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])
    return dQ, dP, (torch.stack([o[2] for o in outs]) if carried else None)


# ---------------------------------------------------------------------------------------
# shared inputs (float64 on the CPU; the tests round them to float32)
def pass_inputs(D, M, N, L, shift, seed=0):
    """Support and carried points in the unit box moved by `shift`, momenta 0.05 randn, directions
    of unit scale in every slot."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * M + N + D)
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    q = torch.rand(M, D, generator=g, dtype=torch.float64) + shift
    x = torch.rand(N, D, generator=g, dtype=torch.float64) + shift
    p = 0.05 * r(M, D)
    return dict(q=q, p=p, x=x, dq=0.1 * r(L, M, D), dp=0.05 * r(L, M, D), dx=0.1 * r(L, N, D))


def flow_inputs(D, seed=0, M=FLOW_M, N=FLOW_N, L=FLOW_L):
    g = torch.Generator().manual_seed(77 + 10 * seed + D)
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    q0 = torch.rand(M, D, generator=g, dtype=torch.float64)
    x0 = torch.rand(N, D, generator=g, dtype=torch.float64)
    p0 = 0.05 * r(M, D)
    return dict(q0=q0, p0=p0, x0=x0, dq0=0.1 * r(L, M, D), dp0=0.05 * r(L, M, D), dx0=0.1 * r(L, N, D))


def r64(d):
    """The float32-rounded inputs in float64: what the float64 reference of a float32 run sees."""
    return {k: v.float().double() for k, v in d.items()}


def r32(d):
    return {k: v.float() for k, v in d.items()}


def nerr(a, b):
    """Norm-wise relative error over a tuple of tensors (None entries skipped), the worst entry."""
    worst = 0.0
    for u, v in zip(a, b):
        if u is None and v is None:
            continue
        u, v = u.detach().double().cpu(), v.detach().double().cpu()
        n = float(v.norm())
        worst = max(worst, float((u - v).norm()) / n if n > 0 else float((u - v).norm()))
    return worst


def oracle(D, scheme, sigma, nt=FLOW_NT, version="classic"):
    """The oracle's eta = 0 models: classic, or hybrid (the cost carries the log-determinant)."""
    from oracle import torch_ref as R
    return R.LDDMM(sigma, D, 10.0, False, version == "hybrid", scheme=scheme, nt=nt)
