"""Closed forms of the deformation Jacobian at carried points (test helper; CPU torch, any dtype).

vel_grad: v(x) and the velocity gradient A = dv/dx of the LDDMM field of (q, p),
    A[i, d, a] = -s sum_j K z_a p_j[d] + eta s (delta_da sum_j K - s sum_j K z_d z_a),
    s = 1/sigma^2, z = x_i - q_j, K = exp(-s |z|^2 / 2).
flow: the recurrences of the displacement gradient G = J - I along the discrete flow of
    oracle.torch_ref.LDDMM.Shoot (Euler and Ralston), in the dtype of the inputs.
oracle_flow: the same quantity from autograd through the oracle's Shoot (the arbiter).
tests/test_ext_jac_host.py pins vel_grad and flow against oracle_flow in float64; the GPU tests
(tests/test_gpu_ext_jac.py) compare the kernels with them.
"""
import torch

CHUNK = 1024


def vel_grad(x, q, p, sigma, eta):
    """(v (N, D), A (N, D, D)) in the dtype of x, rows in chunks (memory O(CHUNK x M x D^2))."""
    s = 1.0 / sigma ** 2
    D = x.shape[1]
    eye = torch.eye(D, dtype=x.dtype)
    vs, As = [], []
    for a in range(0, x.shape[0], CHUNK):
        z = x[a:a + CHUNK, None, :] - q[None, :, :]                 # (n, M, D)
        K = torch.exp(-0.5 * s * (z * z).sum(-1))                   # (n, M)
        Kz = K[:, :, None] * z
        v = K @ p
        A = -s * torch.einsum("nmd,nma->nda", K[:, :, None] * p[None, :, :], z)
        if eta != 0:
            v = v + eta * s * Kz.sum(1)
            A = A + eta * s * (K.sum(1)[:, None, None] * eye - s * torch.einsum("nmd,nma->nda", Kz, z))
        vs.append(v)
        As.append(A)
    if not vs:
        return x.new_zeros((0, D)), x.new_zeros((0, D, D))
    return torch.cat(vs), torch.cat(As)


def step(x, G, q, p, sigma, eta, dt):
    """One Euler step (x + dt v, G + dt A (I + G)); G None = zero."""
    v, A = vel_grad(x, q, p, sigma, eta)
    if G is None:
        return x + dt * v, dt * A
    return x + dt * v, G + dt * (A + A @ G)


def flow(ref, q0, p0, x0):
    """(x1, G) of the discrete flow of ref.Shoot(q0, p0, x0) (ref: oracle.torch_ref.LDDMM), with
    the support states integrated by the oracle's own ODE in the dtype of the inputs."""
    dt = 1.0 / ref.nt
    D = x0.shape[1]
    eye = torch.eye(D, dtype=x0.dtype)
    zero = torch.zeros(1, dtype=q0.dtype)
    q, p, x = q0, p0, x0
    G = torch.zeros((x0.shape[0], D, D), dtype=x0.dtype)
    for _ in range(ref.nt):
        vq, mG, _ = ref.ODE(q, p, zero)
        v1, A1 = vel_grad(x, q, p, ref.sigma, ref.eta)
        B1 = A1 @ (eye + G)
        if ref.scheme == "Euler":
            q, p, x, G = q + dt * vq, p + dt * mG, x + dt * v1, G + dt * B1
            continue
        h = 2 * dt / 3
        qm, pm = q + h * vq, p + h * mG
        vq2, mG2, _ = ref.ODE(qm, pm, zero)
        v2, A2 = vel_grad(x + h * v1, qm, pm, ref.sigma, ref.eta)
        B2 = A2 @ (eye + G + h * B1)
        q, p = q + (0.25 * dt) * (vq + 3 * vq2), p + (0.25 * dt) * (mG + 3 * mG2)
        x, G = x + (0.25 * dt) * (v1 + 3 * v2), G + (0.25 * dt) * (B1 + 3 * B2)
    return x, G


def oracle_flow(ref, q0, p0, x0):
    """(x1, G = J - I) with J[i] = d x1_i / d x0_i by autograd through ref.Shoot: the carried
    points do not interact, so row d of every J[i] is the gradient of sum_i x1[i, d]."""
    x0 = x0.detach().clone().requires_grad_(True)
    x1 = ref.Shoot(q0, p0, x0)[-1][3]
    D = x0.shape[1]
    rows = [torch.autograd.grad(x1[:, d].sum(), x0, retain_graph=d + 1 < D)[0] for d in range(D)]
    J = torch.stack(rows, 1)
    return x1.detach(), J - torch.eye(D, dtype=x0.dtype)
