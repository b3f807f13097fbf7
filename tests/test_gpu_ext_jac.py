"""Deformation Jacobian at carried points on the device (csrc/ext_jac.hip and the methods built on
it): the velocity-gradient kernel, the fused Euler step of (x, G = J - I), LDDMMModel.flow_jacobian
for both integration schemes and the LDDMMRegistration interface -- against the float64 closed
forms of tests/jac_ref.py (pinned against autograd through the oracle by
tests/test_ext_jac_host.py) and against autograd through the oracle's Shoot itself.

Tolerances (norm-wise relative): 1e-5 against float64 on the float32-rounded inputs;
2e-5 between two float32 kernels; the flow within max(1e-5, 2 e32), e32 being the error of the
same recurrence run in float32 on the CPU (the reference's own drift, computed here)."""
import functools

import pytest
import torch

import jac_ref as J
from conftest import rel_err

pytestmark = pytest.mark.gpu
SIG = 0.15
WS_ODE_EXT_JAC = 14
SHAPES = [(1, 1), (7, 300), (513, 129), (3000, 2000), (20000, 700), (700, 20000)]


def _case(N, M, D, seed):
    """x (N, D), q (M, D) in the unit box, p = 0.02 randn (float64, CPU), as tests/test_gpu_ext_pk.py."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, D, generator=g, dtype=torch.float64)
    q = torch.rand(M, D, generator=g, dtype=torch.float64)
    p = 0.02 * torch.randn(M, D, generator=g, dtype=torch.float64)
    return x, q, p


def _f32(dev, *ts):
    return [t.float().to(dev) for t in ts]


def _r64(*ts):
    """The float32-rounded inputs, in float64 (what the float64 reference sees)."""
    return [t.float().double() for t in ts]


# ---------------------------------------------------------------------------------------
# 1. kernel parity
# ---------------------------------------------------------------------------------------
def _parity(dev, N, M, D, eta, seed):
    from difficp_amd import _lib
    x, q, p = _case(N, M, D, seed)
    vx, A = _lib.ode_ext_jac(*_f32(dev, x, q, p), SIG, eta)
    assert vx.shape == (N, D) and A.shape == (N, D, D)
    v64, A64 = J.vel_grad(*_r64(x, q, p), SIG, eta)
    ev, eA = rel_err(vx, v64), rel_err(A, A64)
    print(f"ode_ext_jac N={N} M={M} D={D} eta={eta}: vx {ev:.2e}  A {eA:.2e}")
    assert ev < 1e-5
    assert eA < 1e-5


@pytest.mark.parametrize("N,M", SHAPES)
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("eta", [0.0, 2e-3])
def test_velocity_gradient_parity(dev, N, M, D, eta):
    _parity(dev, N, M, D, eta, N * 7 + M + D)


def _first_split_support(N):
    from difficp_amd import _lib
    m = 1
    while m <= 2 ** 20:
        if _lib.num_splits(WS_ODE_EXT_JAC, m, N) >= 2:
            return m
        m += 1
    pytest.fail(f"dicp_num_splits(DICP_WS_ODE_EXT_JAC, M, {N}) < 2 for every M <= 2^20")


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("eta", [0.0, 2e-3])
def test_velocity_gradient_split_columns(dev, D, eta):
    """The smallest support the library splits into column chunks (partial slabs + merge), and a
    few chunks more; two launches give the same bits (no atomics)."""
    from difficp_amd import _lib
    N = 300
    M = _first_split_support(N)
    assert _lib.num_splits(WS_ODE_EXT_JAC, M, N) >= 2
    _parity(dev, N, M, D, eta, 97 + D)
    M3 = 3 * M + 5
    assert _lib.num_splits(WS_ODE_EXT_JAC, M3, N) >= 2
    _parity(dev, N, M3, D, eta, 98 + D)
    x, q, p = _f32(dev, *_case(N, M3, D, 99))
    r1 = _lib.ode_ext_jac(x, q, p, SIG, eta)
    r2 = _lib.ode_ext_jac(x, q, p, SIG, eta)
    assert all(torch.equal(a, b) for a, b in zip(r1, r2))


@pytest.mark.parametrize("N,M", [(513, 129), (3000, 2000)])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("eta", [0.0, 2e-3])
def test_trace_is_minus_divergence(dev, N, M, D, eta):
    """Cross-check against the existing external-point forward: trace(A) = -gx, same vx."""
    from difficp_amd import _lib
    x, q, p = _f32(dev, *_case(N, M, D, N * 5 + M + D))
    vx, A = _lib.ode_ext_jac(x, q, p, SIG, eta)
    vx0, gx = _lib.ode_ext_fwd(x, q, p, SIG, eta, True)
    tr = A.diagonal(dim1=1, dim2=2).sum(-1)
    et, ev = rel_err(-tr, gx), rel_err(vx, vx0)
    print(f"trace vs -gx N={N} M={M} D={D} eta={eta}: {et:.2e}  vx {ev:.2e}")
    assert et < 2e-5
    assert ev < 2e-5


def test_empty_support_and_points(dev):
    """No support: v = 0, A = 0, and a step leaves (x, G) as they are; no carried points: empty
    outputs."""
    from difficp_amd import _lib
    x = torch.rand(37, 3, device=dev)
    G = 0.3 * torch.randn(37, 3, 3, device=dev)
    q0 = torch.empty(0, 3, device=dev)
    vx, A = _lib.ode_ext_jac(x, q0, q0, SIG, 0.0)
    assert vx.shape == (37, 3) and A.shape == (37, 3, 3) and not vx.abs().any() and not A.abs().any()
    xn, Gn = _lib.ext_jac_step(x, G, q0, q0, SIG, 2e-3, 0.1)
    assert torch.equal(xn, x) and torch.equal(Gn, G)
    xn, Gn = _lib.ext_jac_step(x, None, q0, q0, SIG, 0.0, 0.1)
    assert torch.equal(xn, x) and not Gn.abs().any()
    q = torch.rand(11, 3, device=dev)
    e = torch.empty(0, 3, device=dev)
    vx, A = _lib.ode_ext_jac(e, q, q, SIG, 0.0)
    assert vx.shape == (0, 3) and A.shape == (0, 3, 3)
    xn, Gn = _lib.ext_jac_step(e, None, q, q, SIG, 0.0, 0.1)
    assert xn.shape == (0, 3) and Gn.shape == (0, 3, 3)


# ---------------------------------------------------------------------------------------
# 2. the fused Euler step
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M", [(1031, 777), (5, 3000)])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("eta", [0.0, 2e-3])
def test_euler_step(dev, N, M, D, eta):
    """(x, G) -> (x + dt v, G + dt A (I + G)) from a random G of size ~0.3 and from G = None."""
    from difficp_amd import _lib
    x, q, p = _case(N, M, D, N + 3 * M + D)
    G = 0.3 * torch.randn(N, D, D, generator=torch.Generator().manual_seed(N + D), dtype=torch.float64)
    dt = 0.1
    xf, qf, pf, Gf = _f32(dev, x, q, p, G)
    x64, q64, p64, G64 = _r64(x, q, p, G)
    for Gd, Gr in ((Gf, G64), (None, None)):
        xn, Gn = _lib.ext_jac_step(xf, Gd, qf, pf, SIG, eta, dt)
        xr, Gnr = J.step(x64, Gr, q64, p64, SIG, eta, dt)
        ex, eG = rel_err(xn, xr), rel_err(Gn, Gnr)
        print(f"ext_jac_step N={N} M={M} D={D} eta={eta} G={'rand' if Gd is not None else 'None'}: "
              f"x {ex:.2e}  G {eG:.2e}")
        assert ex < 1e-5
        assert eG < 1e-5
        # the increment alone (dt A (I + G)), so that the carried G cannot hide it
        inc, incr = Gn.double().cpu() - (0 if Gr is None else Gr), Gnr - (0 if Gr is None else Gr)
        assert rel_err(inc, incr) < 1e-5 + 6e-8 * float(Gnr.norm() / incr.norm())
    assert torch.equal(xf.cpu(), x.float()) and torch.equal(Gf.cpu(), G.float())   # inputs untouched


# ---------------------------------------------------------------------------------------
# 3. the flow: LDDMMModel.flow_jacobian against autograd through the oracle
# ---------------------------------------------------------------------------------------
FLOW_N, FLOW_M, NT, LAM = 700, 500, 10, 500.0


@functools.lru_cache(maxsize=None)
def _flow_ref(D, version, scheme):
    """Inputs (seed 5 + D), the float64 oracle's (x1, G, q1, p1) and e32, the error of the same
    recurrence in float32 on the CPU.  Computed once per case and shared; never modified."""
    from oracle import torch_ref as R
    x, q, p = _case(FLOW_N, FLOW_M, D, 5 + D)
    ref = R.LDDMM(SIG, D, LAM, version == "logdet", True, scheme=scheme, nt=NT)
    x1, G = J.oracle_flow(ref, q, p, x)
    _, G32 = J.flow(ref, q.float(), p.float(), x.float())
    e32 = rel_err(G32, G)
    q1, p1 = ref.Shoot(q, p)[-1][:2]
    return dict(ref=ref, x=x, q=q, p=p, x1=x1, G=G, e32=e32, q1=q1, p1=p1)


def _model(dev, D, version, scheme):
    from difficp_amd.core.LDDMM import LDDMMModel
    return LDDMMModel(sigma=SIG, D=D, lambd=LAM, version=version, scheme=scheme, nt=NT,
                      spec={"device": dev, "dtype": torch.float32})


def _eye(D):
    return torch.eye(D, dtype=torch.float64)


@pytest.mark.parametrize("scheme", ["Euler", "Ralston"])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("version", ["hybrid", "logdet"])
def test_flow_jacobian(dev, scheme, D, version):
    c = _flow_ref(D, version, scheme)
    det = torch.linalg.det(c["G"] + _eye(D))
    assert float(det.min()) > 0                       # the reference map is invertible everywhere
    LM = _model(dev, D, version, scheme)
    x, q, p = _f32(dev, c["x"], c["q"], c["p"])
    x1, Jd = LM.flow_jacobian(q, p, x)
    assert x1.shape == (FLOW_N, D) and Jd.shape == (FLOW_N, D, D)
    G = Jd.double().cpu() - _eye(D)
    eG, ex = rel_err(G, c["G"]), rel_err(x1, c["x1"])
    print(f"flow_jacobian {scheme} D={D} {version}: G {eG:.2e} (e32 {c['e32']:.2e})  x1 {ex:.2e}  "
          f"|G|/|I| {float(c['G'].norm()) / (FLOW_N * D) ** 0.5:.2f}  det {float(det.min()):.2f}..{float(det.max()):.1f}")
    assert ex < 1e-5
    assert eG < max(1e-5, 2 * c["e32"])
    # a passed forward shoot (with its carried points) gives the same flow
    sh = LM.Shoot(q, p, x)
    x1s, Js = LM.flow_jacobian(q, p, x, shoot=sh)
    assert rel_err(x1s, sh[-1][3]) < 1e-6
    assert rel_err(Js.double().cpu() - _eye(D), c["G"]) < max(1e-5, 2 * c["e32"])


# ---------------------------------------------------------------------------------------
# 4. the registration interface
# ---------------------------------------------------------------------------------------
IFACE = [(2, "hybrid", "Ralston"), (3, "hybrid", "Euler"), (3, "logdet", "Euler")]


def _registration(dev, D, version, scheme):
    from difficp_amd.core.registrations import LDDMMRegistration
    c = _flow_ref(D, version, scheme)
    LM = _model(dev, D, version, scheme)
    x, q, p = _f32(dev, c["x"], c["q"], c["p"])
    return c, LM, LDDMMRegistration(LM, q, p), x


@pytest.mark.parametrize("D,version,scheme", IFACE)
def test_apply_with_jacobian_and_log_det(dev, D, version, scheme):
    c, LM, reg, X = _registration(dev, D, version, scheme)
    Xg = X.clone().requires_grad_(True)
    Y, Jd = reg.apply_with_jacobian(Xg)
    assert not Y.requires_grad and not Jd.requires_grad and Xg.grad is None   # no graph
    assert rel_err(Y, reg.apply(X)) < 1e-5
    assert rel_err(Jd.double().cpu() - _eye(D), c["G"]) < max(1e-5, 2 * c["e32"])
    assert torch.equal(reg.jacobian(X), Jd)
    ld = reg.log_jacobian_det(Xg)
    assert ld.shape == (FLOW_N,) and ld.dtype == torch.float32 and not ld.requires_grad
    ld64 = torch.logdet(c["G"] + _eye(D))
    e = float((ld.double().cpu() - ld64).abs().max())
    print(f"log_jacobian_det D={D} {version} {scheme}: max abs error {e:.2e}")
    assert e < 1e-5


@pytest.mark.parametrize("D,version,scheme", IFACE)
def test_model_and_shoot_cache_untouched(dev, D, version, scheme):
    c, LM, reg, X = _registration(dev, D, version, scheme)
    if getattr(LM, "shoot_cache", None) is None:
        pytest.fail("LDDMMModel without a shoot_cache")
    Y = reg.apply(X)
    cache = LM.shoot_cache
    before = (len(cache), cache.hits, cache.misses, cache.nbytes)
    state = {k: v for k, v in LM.__dict__.items() if k != "Kernel"}
    reg.jacobian(X)
    reg.jacobian(Y, backward=True)
    reg.apply_with_jacobian(X)
    reg.log_jacobian_det(X)
    LM.Dv(X, reg.q0, reg.a0)
    assert (len(cache), cache.hits, cache.misses, cache.nbytes) == before
    assert LM.__dict__.keys() == state.keys() | {"Kernel"}
    for k, v in state.items():
        assert LM.__dict__[k] is v


@pytest.mark.parametrize("D,version,scheme", IFACE)
def test_backward_jacobian_inverts(dev, D, version, scheme):
    """jacobian(apply(X), backward=True) @ jacobian(X) is the identity up to the discretisation
    error of the backward shooting, which the float64 oracle's own two Jacobians measure."""
    c, LM, reg, X = _registration(dev, D, version, scheme)
    _, Gb = J.oracle_flow(c["ref"], c["q1"], -c["p1"], c["x1"])
    I = _eye(D)
    nI = (FLOW_N * D) ** 0.5
    dev_ref = float(((Gb + I) @ (c["G"] + I) - I).norm()) / nI
    Jf = reg.jacobian(X)
    Jb = reg.jacobian(reg.apply(X), backward=True)
    dev_gpu = float(((Jb @ Jf).double().cpu() - I).norm()) / nI
    print(f"backward @ forward - I, D={D} {version} {scheme}: device {dev_gpu:.3e}  oracle {dev_ref:.3e}")
    assert dev_gpu <= dev_ref + 1e-4
    # a passed forward shoot gives the same backward Jacobian
    sh = reg.shoot(None)
    Jb2 = reg.jacobian(reg.apply(X), backward=True, previous_forwardshoot=sh)
    assert rel_err(Jb2, Jb) < 1e-6


def test_nan_row_stays_in_its_row(dev):
    c, LM, reg, X = _registration(dev, 3, "hybrid", "Euler")
    Xn = X.clone()
    Xn[123] = float("nan")
    Y, Jd = reg.apply_with_jacobian(Xn)
    ld = reg.log_jacobian_det(Xn)
    bad = torch.zeros(FLOW_N, dtype=torch.bool, device=dev)
    bad[123] = True
    assert bool(torch.isnan(Jd[123]).all()) and bool(torch.isnan(Y[123]).all()) and bool(torch.isnan(ld[123]))
    assert not bool(torch.isnan(Jd[~bad]).any()) and not bool(torch.isnan(ld[~bad]).any())
    Y0, J0 = reg.apply_with_jacobian(X)
    assert torch.equal(Jd[~bad], J0[~bad]) and torch.equal(Y[~bad], Y0[~bad])


def test_log_det_is_nan_where_the_map_folds(dev):
    """det J <= 0: a momentum field strong enough to fold the discrete map somewhere."""
    from difficp_amd.core.registrations import LDDMMRegistration
    c = _flow_ref(2, "hybrid", "Euler")
    LM = _model(dev, 2, "hybrid", "Euler")
    x, q, p = _f32(dev, c["x"], c["q"], 5.0 * c["p"])
    reg = LDDMMRegistration(LM, q, p)
    Jd = reg.jacobian(x)
    det = torch.linalg.det(Jd.double())
    ld = reg.log_jacobian_det(x)
    neg, pos = det < -1e-3, det > 1e-3              # away from the fold itself
    assert bool(neg.any()) and bool(pos.any())
    assert bool(torch.isnan(ld[neg]).all()) and not bool(torch.isnan(ld[pos]).any())
    assert rel_err(ld[pos], torch.log(det[pos])) < 1e-5
