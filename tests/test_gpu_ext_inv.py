"""Exact inverse of the fitted map on the device (csrc/ext_jac.hip dicp_lddmm_ext_inv_step_f32 and
the methods built on it): the fused Newton update of a step map, LDDMMModel.flow_inverse for both
integration schemes, the LDDMMRegistration / PSR interface -- against the float64 closed forms of
tests/inv_ref.py (pinned against the oracle's Shoot by tests/test_ext_inv_host.py).

Tolerances (norm-wise relative): 1e-5 against float64 on the float32-rounded inputs;
flows within max(1e-5, 2 e32), e32 being the error of the same recurrence (same stopping rule) run
in float32 on the CPU, computed here."""
import functools
import warnings

import pytest
import torch

import inv_ref as I
from conftest import rel_err

pytestmark = pytest.mark.gpu
SIG, DT = I.SIG, 0.1
WS_ODE_EXT_INV = 15


def _f32(dev, *ts):
    return [None if t is None else t.float().to(dev) for t in ts]


def _r64(*ts):
    """The float32-rounded inputs, in float64 (what the float64 reference sees)."""
    return [None if t is None else t.float().double() for t in ts]


# ---------------------------------------------------------------------------------------
# 1. the Newton update of one step map
# ---------------------------------------------------------------------------------------
def _step_inputs(N, M, D, eta, form, seed):
    """x, the support (q, p) the call gets (Ralston: the mid-state), the first stage's (v1, A1)
    (Euler: None) and y = F64(x) + 0.01 randn; float64 on the CPU."""
    from oracle import torch_ref as R
    x, q, p = I.case(N, M, D, seed)
    v1 = A1 = None
    if form == "Ralston":
        ref = R.LDDMM(SIG, D, 1.0 / eta if eta else I.LAM, eta != 0, True, scheme="Ralston", nt=10)
        vq, mG, _ = ref.ODE(q, p, torch.zeros(1, dtype=torch.float64))
        v1, A1 = I.J.vel_grad(x, q, p, SIG, eta)
        q, p = q + (2 * DT / 3) * vq, p + (2 * DT / 3) * mG
    inc, _ = I.step_map(x, q, p, SIG, eta, DT, v1, A1)
    g = torch.Generator().manual_seed(seed + 1)
    y = x + inc + 0.01 * torch.randn(N, D, generator=g, dtype=torch.float64)
    return x, y, q, p, v1, A1


def _step_parity(dev, N, M, D, eta, form, seed):
    from difficp_amd import _lib
    ins = _step_inputs(N, M, D, eta, form, seed)
    x, y, q, p, v1, A1 = _f32(dev, *ins)
    keep = [None if t is None else t.clone() for t in (x, y, q, p, v1, A1)]
    xn, res = _lib.ext_inv_step(x, y, q, p, SIG, eta, DT, v1, A1)
    assert xn.shape == (N, D) and res.shape == (N,) and xn.dtype == res.dtype == torch.float32
    x64, y64, q64, p64, v164, A164 = _r64(*ins)
    xr, rr = I.newton_step(x64, y64, q64, p64, SIG, eta, DT, v164, A164)
    _, DF = I.step_map(x64, q64, p64, SIG, eta, DT, v164, A164)
    ninv = float(torch.linalg.matrix_norm(torch.linalg.inv(DF), 2).max())
    inc, incr = xn.double().cpu() - x64, xr - x64
    ex, ei, er = rel_err(xn, xr), rel_err(inc, incr), rel_err(res, rr)
    print(f"ext_inv_step {form} N={N} M={M} D={D} eta={eta}: x_next {ex:.2e}  increment {ei:.2e}  res {er:.2e}  "
          f"max |DF^-1| {ninv:.2f}")
    assert ninv <= 2                                    # what the factor 2 below stands for
    assert ex < 1e-5
    assert ei < 1e-5 + 2 * 6e-8 * float(xr.norm() / incr.norm())
    assert er < 1e-5 + 6e-8 * float(y64.norm() / rr.norm())
    for a, b in zip((x, y, q, p, v1, A1), keep):        # inputs untouched
        assert a is None or torch.equal(a, b)
    return xn, res


@pytest.mark.parametrize("N,M", [(1, 1), (7, 300), (513, 129), (3000, 2000)])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("eta", [0.0, 2e-3])
@pytest.mark.parametrize("form", ["Euler", "Ralston"])
def test_newton_step_parity(dev, form, eta, D, N, M):
    _step_parity(dev, N, M, D, eta, form, N * 7 + M + D)


def _first_split_support(N):
    from difficp_amd import _lib
    m = 1
    while m <= 2 ** 20:
        if _lib.num_splits(WS_ODE_EXT_INV, m, N) >= 2:
            return m
        m += 1
    pytest.fail(f"dicp_num_splits(DICP_WS_ODE_EXT_INV, M, {N}) < 2 for every M <= 2^20")


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("eta", [0.0, 2e-3])
@pytest.mark.parametrize("form", ["Euler", "Ralston"])
def test_newton_step_split_columns(dev, form, eta, D):
    """The smallest support the library splits into column chunks ((v | A) through the partial
    slabs into the scratch, then the row-wise update), and a few chunks more; two launches give
    the same bits (no atomics)."""
    from difficp_amd import _lib
    N = 300
    M = _first_split_support(N)
    _step_parity(dev, N, M, D, eta, form, 97 + D)
    M3 = 3 * M + 5
    assert _lib.num_splits(WS_ODE_EXT_INV, M3, N) >= 2
    _step_parity(dev, N, M3, D, eta, form, 98 + D)
    x, y, q, p, v1, A1 = _f32(dev, *_step_inputs(N, M3, D, eta, form, 99))
    r1 = _lib.ext_inv_step(x, y, q, p, SIG, eta, DT, v1, A1)
    r2 = _lib.ext_inv_step(x, y, q, p, SIG, eta, DT, v1, A1)
    assert all(torch.equal(a, b) for a, b in zip(r1, r2))


def test_empty_support_and_points(dev):
    """No support: v = A = 0, so the Euler form gives x_next = y and res = |x - y|_inf, and the
    Ralston form F = x + dt/4 v1, DF = I + dt/4 A1; no carried points: empty outputs."""
    from difficp_amd import _lib
    g = torch.Generator().manual_seed(7)
    x = torch.rand(37, 3, generator=g).to(dev)
    y = (x.cpu() + 0.01 * torch.randn(37, 3, generator=g)).to(dev)
    q0 = torch.empty(0, 3, device=dev)
    xn, res = _lib.ext_inv_step(x, y, q0, q0, SIG, 2e-3, DT)
    assert torch.equal(xn, y) and torch.equal(res, (x - y).abs().amax(1))
    v1 = (0.1 * torch.randn(37, 3, generator=g)).to(dev)
    A1 = (0.3 * torch.randn(37, 3, 3, generator=g)).to(dev)
    xn, res = _lib.ext_inv_step(x, y, q0, q0, SIG, 0.0, DT, v1, A1)
    x64, y64, v64, A64 = _r64(x.cpu(), y.cpu(), v1.cpu(), A1.cpu())
    xr, rr = I.newton_step(x64, y64, torch.empty(0, 3, dtype=torch.float64), torch.empty(0, 3, dtype=torch.float64),
                           SIG, 0.0, DT, v64, A64)
    assert rel_err(xn, xr) < 1e-5 and rel_err(res, rr) < 1e-5
    q = torch.rand(11, 3, device=dev)
    e = torch.empty(0, 3, device=dev)
    xn, res = _lib.ext_inv_step(e, e, q, q, SIG, 0.0, DT)
    assert xn.shape == (0, 3) and res.shape == (0,)
    with pytest.raises(ValueError):
        _lib.ext_inv_step(x, y, q, q, SIG, 0.0, DT, v1=v1)          # v1 without A1
    with pytest.raises(ValueError):
        _lib.ext_inv_step(x, y[:5], q, q, SIG, 0.0, DT)


def test_singular_and_nan_rows_stay_in_their_rows(dev):
    """DF = I + dt A singular (A1 = -4/dt I with no support, Ralston form: DF = 0) and a NaN row:
    both non-finite in x_next and res, every other row bitwise as without them."""
    from difficp_amd import _lib
    g = torch.Generator().manual_seed(9)
    x, q, p = _f32(dev, *I.case(200, 150, 2, 3))
    y = x + 0.01 * torch.randn(200, 2, generator=g).to(dev)
    v1, A1 = _lib.ode_ext_jac(x, q, p, SIG, 2e-3)
    x0, r0 = _lib.ext_inv_step(x, y, q, p, SIG, 2e-3, DT, v1, A1)
    xb, yb = x.clone(), y.clone()
    yb[17] = float("nan")
    xb[101, 1] = float("inf")
    xn, res = _lib.ext_inv_step(xb, yb, q, p, SIG, 2e-3, DT, v1, A1)
    bad = torch.zeros(200, dtype=torch.bool, device=dev)
    bad[17] = bad[101] = True
    assert not bool(torch.isfinite(xn[bad]).any()) and not bool(torch.isfinite(res[bad]).any())
    assert torch.equal(xn[~bad], x0[~bad]) and torch.equal(res[~bad], r0[~bad])
    e = torch.empty(0, 2, device=dev)
    A = torch.zeros(200, 2, 2, device=dev)
    A[5] = -32.0 * torch.eye(2, device=dev)                        # dt = 1/8: DF[5] = I + dt/4 A1 = 0 exactly
    xn, res = _lib.ext_inv_step(x, y, e, e, SIG, 0.0, 0.125, torch.zeros_like(x), A)
    assert not bool(torch.isfinite(xn[5]).any()) and not bool(torch.isfinite(res[5]))
    ok = torch.ones(200, dtype=torch.bool, device=dev)
    ok[5] = False
    assert bool(torch.isfinite(xn[ok]).all()) and bool(torch.isfinite(res[ok]).all())


# ---------------------------------------------------------------------------------------
# 2. the flow: LDDMMModel.flow_inverse against the float64 points the oracle's Shoot carried
# ---------------------------------------------------------------------------------------
FLOW_N = 700


def _tol(y):
    return 1e-6 * max(SIG, float(y.abs().max()))


@functools.lru_cache(maxsize=None)
def _flow_ref(D, version, scheme, scale=1.0):
    """Inputs, the float64 oracle's x1 = phi(x) and e32, the error of inv_ref.inverse in float32
    on the CPU with the default tolerance.  Computed once per case and shared; never modified."""
    ref, x, q, p = I.flow_case(D, version, scheme, scale)
    x1 = ref.Shoot(q, p, x)[-1][3]
    x32, info = I.inverse(ref, q.float(), p.float(), x1.float(), _tol(x1.float()))
    ok = info["converged"]
    return dict(ref=ref, x=x, q=q, p=p, x1=x1, e32=rel_err(x32[ok], x[ok]), n32=int(ok.sum()))


def _model(dev, D, version, scheme):
    from difficp_amd.core.LDDMM import LDDMMModel
    return LDDMMModel(sigma=SIG, D=D, lambd=I.LAM, version=version, scheme=scheme, nt=I.NT,
                      spec={"device": dev, "dtype": torch.float32})


def _registration(dev, D, version, scheme, scale=1.0):
    from difficp_amd.core.registrations import LDDMMRegistration
    c = _flow_ref(D, version, scheme, scale)
    LM = _model(dev, D, version, scheme)
    x, q, p, x1 = _f32(dev, c["x"], c["q"], c["p"], c["x1"])
    return c, LM, LDDMMRegistration(LM, q, p), x, x1


@pytest.mark.parametrize("D,version,scheme,scale", I.TABLE)
def test_flow_inverse(dev, D, version, scheme, scale):
    c, LM, reg, X, Y = _registration(dev, D, version, scheme)
    bound = max(1e-5, 2 * c["e32"])
    x0, info = LM.flow_inverse(reg.q0, reg.a0, Y)
    tol = _tol(Y)
    e = rel_err(x0, c["x"])
    print(f"flow_inverse {scheme} D={D} {version}: {e:.2e} (e32 {c['e32']:.2e})  updates {info['iterations']}  "
          f"passes {info['passes']}  residual {float(info['residual'].max()):.2e} (tol {tol:.2e})")
    assert x0.shape == (FLOW_N, D) and not x0.requires_grad
    assert bool(info["converged"].all()) and info["converged"].shape == (FLOW_N,)
    assert len(info["iterations"]) == I.NT and max(info["iterations"]) <= 10
    assert info["passes"] == (1 if scheme == "Euler" else 2) * sum(k + 1 for k in info["iterations"])
    assert info["residual"].dtype == torch.float32 and float(info["residual"].max()) <= tol
    assert e < bound
    # on the device: both compositions are the identity
    Xi = reg.inverse(reg.apply(X))
    Yi = reg.apply(reg.inverse(Y))
    print(f"  inverse(apply(X)) {rel_err(Xi, X):.2e}  apply(inverse(Y)) {rel_err(Yi, Y):.2e}")
    assert rel_err(Xi, X) < bound and rel_err(Yi, Y) < bound
    # a passed forward shoot (with its carried points) gives the same inverse
    sh = LM.Shoot(reg.q0, reg.a0, X)
    xs, _ = LM.flow_inverse(reg.q0, reg.a0, Y, shoot=sh)
    assert rel_err(xs, x0) < 1e-6
    assert rel_err(reg.inverse(Y, previous_forwardshoot=sh), x0) < 1e-6
    if scheme == "Euler":
        # a shoot of Optimize's need_p1=False path: its final momenta are never read, nor formed
        sh = LM.Shoot(reg.q0, reg.a0, need_p1=False)
        assert sh.p1_missing
        xs, _ = LM.flow_inverse(reg.q0, reg.a0, Y, shoot=sh)
        assert rel_err(xs, x0) < 1e-6
        assert sh.p1_missing and bool(torch.isnan(sh.P[-1]).all())


@pytest.mark.parametrize("D,version,scheme,scale", I.STRONG)
def test_strong_deformation(dev, D, version, scheme, scale):
    """3x momenta (det J down to 0.06): every row converges; the error is the stopping tolerance
    times |J^-1|, not rounding, and e32 runs the same rule -- hence 4 e32."""
    c, LM, reg, X, Y = _registration(dev, D, version, scheme, scale)
    x0, info = reg.inverse(Y, return_info=True)
    e = rel_err(x0, c["x"])
    line = f"strong {scheme} D={D} {version} x{scale:g}: inverse {e:.2e} (e32 {c['e32']:.2e})  updates {info['iterations']}"
    if version == "hybrid":
        line += f"  backward {rel_err(reg.backward(Y), c['x']):.2e}"
    print(line)
    assert c["n32"] == FLOW_N
    assert bool(info["converged"].all())
    assert e < max(1e-5, 4 * c["e32"])


def test_folded_map(dev):
    """5x momenta, D = 2 hybrid Euler: the map folds (det J <= 0 at 77 of the 700 points in
    float64; the CPU float32 recurrence converges on about 520 rows).  Where the map is not
    injective Newton may find another preimage, so the converged rows are checked through apply."""
    c, LM, reg, X, Y = _registration(dev, 2, "hybrid", "Euler", 5.0)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        x0, info = reg.inverse(Y, return_info=True)
    rw = [m for m in w if issubclass(m.category, RuntimeWarning)]
    ok = info["converged"]
    print(f"folded: {int(ok.sum())} of {FLOW_N} rows converge (CPU float32: {c['n32']}); {rw[0].message if rw else ''}")
    assert len(rw) == 1 and str(FLOW_N - int(ok.sum())) in str(rw[0].message)
    assert bool(torch.isnan(x0[~ok]).all()) and bool(torch.isfinite(x0[ok]).all())
    assert int(ok.sum()) >= FLOW_N // 2 and int(ok.sum()) < FLOW_N
    assert rel_err(reg.apply(x0[ok]), Y[ok]) < 1e-5


def test_nan_row_stays_in_its_row(dev):
    c, LM, reg, X, Y = _registration(dev, 3, "logdet", "Euler")
    x0, i0 = reg.inverse(Y, return_info=True)
    Yn = Y.clone()
    Yn[123] = float("nan")
    with pytest.warns(RuntimeWarning):
        xn, info = reg.inverse(Yn, return_info=True)
    bad = torch.zeros(FLOW_N, dtype=torch.bool, device=dev)
    bad[123] = True
    assert bool(torch.isnan(xn[123]).all()) and not bool(info["converged"][123])
    assert bool(info["converged"][~bad].all())
    assert info["iterations"] == i0["iterations"]
    assert torch.equal(xn[~bad], x0[~bad]) and torch.equal(info["residual"][~bad], i0["residual"][~bad])


IFACE = [(2, "hybrid", "Ralston"), (3, "hybrid", "Euler"), (3, "logdet", "Euler")]


@pytest.mark.parametrize("D,version,scheme", IFACE)
def test_model_and_shoot_cache_untouched(dev, D, version, scheme):
    c, LM, reg, X, Y = _registration(dev, D, version, scheme)
    if getattr(LM, "shoot_cache", None) is None:
        pytest.fail("LDDMMModel without a shoot_cache")
    reg.apply(X)
    cache = LM.shoot_cache
    before = (len(cache), cache.hits, cache.misses, cache.nbytes)
    state = {k: v for k, v in LM.__dict__.items() if k != "Kernel"}
    Yg = Y.clone().requires_grad_(True)
    Xi = reg.inverse(Yg)
    assert not Xi.requires_grad and Yg.grad is None              # no graph
    reg.inverse_with_jacobian(Y)
    LM.flow_inverse(reg.q0, reg.a0, Y, tol=1e-5, max_iter=3)
    assert (len(cache), cache.hits, cache.misses, cache.nbytes) == before
    assert LM.__dict__.keys() == state.keys() | {"Kernel"}
    for k, v in state.items():
        assert LM.__dict__[k] is v


@pytest.mark.parametrize("D,version,scheme", IFACE)
def test_inverse_jacobian(dev, D, version, scheme):
    c, LM, reg, X, Y = _registration(dev, D, version, scheme)
    Xi, Jinv = reg.inverse_with_jacobian(Y)
    assert Jinv.shape == (FLOW_N, D, D) and Jinv.dtype == torch.float32 and not Jinv.requires_grad
    assert torch.equal(Xi, reg.inverse(Y))
    R = (Jinv.double() @ reg.jacobian(Xi).double()).cpu() - torch.eye(D, dtype=torch.float64)
    e = float(R.norm()) / (FLOW_N * D) ** 0.5
    print(f"Jinv @ J - I, D={D} {version} {scheme}: {e:.2e}")
    assert e < 1e-5
    Yn = Y.clone()
    Yn[5] = float("nan")
    with pytest.warns(RuntimeWarning):
        Xn, Jn = reg.inverse_with_jacobian(Yn)
    assert bool(torch.isnan(Jn[5]).all()) and bool(torch.isnan(Xn[5]).all())
    assert not bool(torch.isnan(Jn[6:]).any())


# ---------------------------------------------------------------------------------------
# 3. the PSR interface
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("support", ["decim", "grid"])
def test_psr_transfer_and_template_in_frame(dev, support):
    from difficp_amd.core.GMM import GaussianMixtureUnif
    from difficp_amd.core.LDDMM import LDDMMModel
    from difficp_amd.core.PSR import DiffPSR
    spec = {"device": dev, "dtype": torch.float32}
    g = torch.Generator().manual_seed(21)
    base = torch.rand(300, 2, generator=g)
    frames = [(base + 0.04 * torch.sin(3.0 * base.flip(1) + k)).to(dev) for k in range(2)]
    G = GaussianMixtureUnif(torch.zeros(20, 2), spec=spec)
    G.to_optimize = {"mu": True, "sigma": True, "w": True, "eta0": False}
    LM = LDDMMModel(sigma=0.2, D=2, lambd=5e2, version="logdet", scheme="Euler", nt=10, spec=spec)
    torch.manual_seed(0)
    P = DiffPSR(frames, G, LM, dataspec=spec, compspec=spec)
    P.printstuff = False
    P.reinitialize_GMM()
    P.set_support_scheme(support, rho=1.0)
    for _ in range(2):
        P.GMM_opt(max_iterations=10, tol=1e-3)
        P.Reg_opt(nmax=1, tol=1e-3)
    mu0, a0 = P.GMMi[0].mu.clone(), [a.clone() for a in P.a0]
    for k in range(2):
        assert float((P.x1[k, 0] - P.x0[k, 0]).norm()) > 1e-3     # a deformation, not the identity
        X = P.x0[k, 0]
        Xk = P.transfer(X, k, k)
        assert Xk.shape == X.shape and Xk.device == X.device and rel_err(Xk, X) < 1e-5
        l = 1 - k
        assert rel_err(P.Registration(l).apply(P.transfer(X, k, l)), P.x1[k, 0]) < 1e-5
        T = P.template_in_frame(k)
        assert T.shape == mu0.shape and rel_err(P.Registration(k).apply(T), mu0) < 1e-5
    assert torch.equal(P.GMMi[0].mu, mu0) and all(torch.equal(a, b) for a, b in zip(P.a0, a0))
