"""Shared inputs of the direct float64 parity tests of the row reductions that are otherwise
reached only through wrappers (GPU: tests/test_gpu_kernel_grads.py; that these inputs can
expose a wrong kernel, from the float64 references alone: tests/test_kernel_grads_host.py).

Every cloud is drawn in float64 and rounded to float32 first: the tensors returned here are
float64 tensors holding float32 values (t.float().double()), so the float64 reference and the
float32 kernel see the same numbers."""
import math

import torch

SIGMA = 0.25          # gradient and scalar-weight reductions
SIGMA_GMM = 0.1       # M-step and targets passes

# (M rows, N columns): the smallest shapes that reach each path of the row-reduction skeleton
# (csrc/launch.hpp: a workgroup covers 512 rows, columns split from 257 on in chunks that are
# multiples of 64, an LDS tile holds 256 columns)
SHAPES = [
    (1, 1),          # single row, single column
    (1, 700),        # one row, split columns
    (513, 1),        # second row block: one real row plus clamped tails; one column
    (150, 230),      # the shape of grad_case.check_reduction_grads: no split
    (300, 257),      # 2 chunks of 192 + 65
    (600, 1300),     # 2 row blocks; 6 chunks of 256 with a 20-column tail
    (64, 5000),      # 20 chunks
]
NO_SPLIT = (150, 230)

# operand patterns per kind: the ones tools/kernel.py issues plus one with every operand the
# kind reads (no HESSW pattern with exactly one of r2 / c2: the header defines it as a zero
# weight and nobody calls it)
GRAD_PATTERNS = {
    "HESSW": [("r1", "cw"), ("c1",), ("r1",), ("r1", "r2", "c2"), ("c1", "r2", "c2"),
              ("r1", "c1", "r2", "c2", "cw")],
    "HESSWP": [("r1", "c1")],
    "ZDOTV": [("r1", "c2"), ("c1", "c2"), ("r1", "c1", "c2")],
    "HESS3": [("r1", "c1", "r2"), ("r1", "c1", "c2"), ("r1", "c1", "r2", "c2")],
    "GRADLAP3": [("r1",), ("c1",), ("r1", "c1")],
}
FULL_PATTERN = {k: v[-1] for k, v in GRAD_PATTERNS.items()}
MSTEP_SHAPES = [(1, 1), (1, 3000), (7, 5000), (513, 300), (600, 1300)]      # (C, N)
TARGETS_SHAPES = [(1, 1), (513, 1), (600, 1300), (64, 5000)]                # (N, C)


def r32(t):
    """float64 tensor of the float32 roundings of t"""
    return t.float().double()


def grad_inputs(M, N, D, seed=None):
    """x (M, D), y (N, D) in [0, 1]^D; row vectors r1, r2 (M, D), column vectors c1, c2 (N, D)
    and the column scalar cw (N,), normal (mixed sign)."""
    # (the seeds: ZDOTV moves by only 0.9 - 1.3 % under a 1 % change of sigma at these clouds --
    # -2 % from s against +2 % x the pairs' energy from K -- and test_kernel_grads_host.py asks
    # 1 % of every pattern; with this offset the smallest figure is 1.15 %)
    g = torch.Generator().manual_seed(200000 + 1000 * D + 7 * M + N if seed is None else seed)
    rand = lambda *s: r32(torch.rand(*s, generator=g, dtype=torch.float64))
    randn = lambda *s: r32(torch.randn(*s, generator=g, dtype=torch.float64))
    return dict(x=rand(M, D), y=rand(N, D), r1=randn(M, D), r2=randn(M, D), c1=randn(N, D),
                c2=randn(N, D), cw=randn(N))


def scal_inputs(M, N, D):
    """Inputs of the GRADKSCAL / GRADLAPKSCAL tests (x, y and the column weight cw of
    grad_inputs): seeds of their own, since GRADKSCAL is as weakly sensitive to sigma as ZDOTV
    (1.25 % at the least with these)."""
    return grad_inputs(M, N, D, seed=5000 + 31 * M + N + D)


def pattern_kwargs(t, pattern):
    """The operands of one pattern; an omitted operand is None."""
    return {k: (t[k] if k in pattern else None) for k in ("r1", "r2", "c1", "c2", "cw")}


def estep64(X, mu, lpi, sigma):
    """The float64 E-step's log2-domain normaliser T2 (as tests/test_gpu_em.py _estep64)."""
    D = X.shape[1]
    lgn = D * (math.log(sigma) + 0.5 * math.log(2 * math.pi))
    D2 = ((X[:, None, :] - mu[None]) ** 2).sum(-1)
    T = (lpi[None] - D2 / (2 * sigma ** 2) - lgn).logsumexp(1)
    return (T + lgn) / math.log(2)


def gmm_inputs(N, C, D, variant="plain", seed=None):
    """Points X (N, D) and components mu (C, D) in [0, 1]^D, random weights; T2 of the float64
    E-step rounded to float32; perturbed new parameters for the targets pass.
    variant "far": the first 50 components moved 3.0 away from every point; "dead": the
    first 20 components dead (w = -inf).  Returns float64 tensors of float32 values:
    X, mu, w2 (log2 weights), T2, mu_new, lpi_new, and the index tensor `special`."""
    g = torch.Generator().manual_seed(500 * D + 3 * N + C if seed is None else seed)
    X = r32(torch.rand(N, D, generator=g, dtype=torch.float64))
    mu = torch.rand(C, D, generator=g, dtype=torch.float64)
    w = 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    special = torch.zeros(C, dtype=torch.bool)
    if variant == "far":
        mu[:50] += 3.0
        special[:50] = True
    elif variant == "dead":
        w[:20] = -math.inf
        special[:20] = True
    mu = r32(mu)
    lpi = w - w.logsumexp(0)
    w2 = r32(lpi / math.log(2))
    T2 = r32(estep64(X, mu, w2 * math.log(2), SIGMA_GMM))
    mu_new = r32(mu + 0.02 * torch.randn(C, D, generator=g, dtype=torch.float64))
    wn = w + 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    lpi_new = r32(wn - wn.logsumexp(0))
    return dict(X=X, mu=mu, w2=w2, T2=T2, mu_new=mu_new, lpi_new=lpi_new, special=special)
