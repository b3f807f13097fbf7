"""The inputs of tests/test_gpu_kernel_grads.py can expose a wrong kernel -- shown with the
float64 references alone (no GPU): leaving out any one operand of a gradient pattern, or a
1 % change of sigma, moves the reference by >= 1e-2 norm-wise, 1000 times the floor of the
GPU tolerance (1e-5); likewise every column of the targets rows and of the M-step statistics
against a 1 % change of sigma_old.  And the float64 statements of GRADKSCAL / GRADLAPKSCAL
(tests/fake_hip.py) equal float64 autograd of the oracle's KRedScal / LapKRed, as
test_host_logic.py pins the five gradient kinds: every reference the GPU file compares with
is itself anchored."""
import pytest
import torch

import fake_hip
import kernel_grads_case as KC
from conftest import rel_err
from oracle import torch_ref as R

BAR = 1e-2
HOST_SHAPES = [(150, 230), (600, 1300)]


@pytest.fixture(autouse=True)
def _float64_spec(monkeypatch):
    monkeypatch.setattr(fake_hip, "_DT", torch.float64)


def _L():
    from difficp_amd import _lib
    return _lib


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("M,N", HOST_SHAPES)
def test_grad_patterns_expose_a_dropped_operand_and_sigma(D, M, N):
    L = _L()
    t = KC.grad_inputs(M, N, D)
    for kind, patterns in KC.GRAD_PATTERNS.items():
        k = getattr(L, "GRAD_" + kind)
        for pat in patterns:
            kw = KC.pattern_kwargs(t, pat)
            full = fake_hip.gauss_red_grad(k, t["x"], t["y"], KC.SIGMA, **kw)
            assert torch.isfinite(full).all() and full.norm() > 0, (kind, pat)
            for name in pat:
                alt = fake_hip.gauss_red_grad(k, t["x"], t["y"], KC.SIGMA, **dict(kw, **{name: None}))
                e = rel_err(alt, full)
                assert e >= BAR, (kind, pat, name, e)
            alt = fake_hip.gauss_red_grad(k, t["x"], t["y"], 1.01 * KC.SIGMA, **kw)
            e = rel_err(alt, full)
            assert e >= BAR, (kind, pat, "sigma", e)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("M,N", HOST_SHAPES)
def test_scal_ops_expose_sigma_and_weight(D, M, N):
    L = _L()
    t = KC.scal_inputs(M, N, D)
    for op in (L.GRADKSCAL, L.GRADLAPKSCAL):
        full = fake_hip.gauss_red(op, t["x"], t["y"], KC.SIGMA, b=t["cw"])
        e = rel_err(fake_hip.gauss_red(op, t["x"], t["y"], 1.01 * KC.SIGMA, b=t["cw"]), full)
        assert e >= BAR, (op, "sigma", e)
        e = rel_err(fake_hip.gauss_red(op, t["x"], t["y"], KC.SIGMA, b=torch.ones_like(t["cw"])), full)
        assert e >= BAR, (op, "b", e)


@pytest.mark.parametrize("D", [2, 3])
def test_scal_ops_equal_float64_autograd(D):
    """GRADKSCAL(x, y, b = g)_i = d/dx_i sum_j g_j KRedScal(y, x, 1)_j and GRADLAPKSCAL(x, y,
    b = g)_i = d/dx_i sum_j g_j LapKRed(y, x)_j: the gradient w.r.t. the former columns x of a
    row reduction over y, the rows' cotangent g folded into the column weight."""
    L = _L()
    M, N = 150, 230
    t = KC.scal_inputs(M, N, D)
    g = t["cw"]
    one = torch.ones(M, dtype=torch.float64)
    for op, fwd in ((L.GRADKSCAL, lambda X: R.KRedScal(t["y"], X, one, KC.SIGMA)),
                    (L.GRADLAPKSCAL, lambda X: R.LapKRed(t["y"], X, KC.SIGMA))):
        X = t["x"].clone().requires_grad_(True)
        (ref,) = torch.autograd.grad((fwd(X) * g).sum(), X)
        out = fake_hip.gauss_red(op, t["x"], t["y"], KC.SIGMA, b=g)
        assert out.dtype == torch.float64
        assert rel_err(out, ref) < 1e-12, (op, rel_err(out, ref))


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("C,N", [(1, 3000), (600, 1300)])
def test_mstep_columns_expose_sigma(D, C, N):
    """The log-weight column at both shapes.  The mean columns are normalised sums: among many
    components the change of sigma nearly cancels in them (6e-4 at (600, 1300)), so their
    sensitivity is shown at the one-component shape, where T2 stays that of the old sigma and
    the points' weights change by exp(-0.02 |x - mu|^2 / (2 sigma^2))."""
    t = KC.gmm_inputs(N, C, D)
    a = (t["X"], t["T2"], t["mu"], t["w2"])
    full = fake_hip.gmm_mstep(*a, KC.SIGMA_GMM)
    alt = fake_hip.gmm_mstep(*a, 1.01 * KC.SIGMA_GMM)
    e = rel_err(alt[:, 0], full[:, 0])
    assert e >= BAR, ("log-weight", e)
    if C == 1:
        for d in range(D):
            e = rel_err(alt[:, 1 + d], full[:, 1 + d])
            assert e >= BAR, ("mean", d, e)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("N,C", [(600, 1300), (64, 5000)])
def test_targets_columns_expose_sigma(D, N, C):
    t = KC.gmm_inputs(N, C, D)
    a = (t["X"], t["T2"], t["mu"], t["w2"])
    full = fake_hip.gmm_targets(*a, KC.SIGMA_GMM, t["mu_new"], t["lpi_new"])
    alt = fake_hip.gmm_targets(*a, 1.01 * KC.SIGMA_GMM, t["mu_new"], t["lpi_new"])
    assert full.shape == (N, D + 4)
    for k in range(D + 4):
        e = rel_err(alt[:, k], full[:, k])
        assert e >= BAR, (k, e)
