"""Forward sensitivities of the shooting on the device (csrc/tlm.hip and the methods built on it):
the tangent-linear kernel dicp_lddmm_ode_tlm_f32, LDDMMModel.shoot_tangent for both integration
schemes and the LDDMMRegistration interface -- against the float64 closed forms of tests/tlm_ref.py
(pinned against forward-mode autograd through the oracle by tests/test_tlm_host.py), against that
autograd itself and against the hand-written adjoint of the device shooting.

Tolerances (norm-wise relative): 1e-5 against float64 on the float32-rounded inputs;
2e-5 between two float32 kernels; the flow within max(1e-5, 2 e32), e32 being the error of the same
recurrence run in float32 on the CPU (the reference's own drift, computed here)."""
import functools

import pytest
import torch

import tlm_ref as T

pytestmark = pytest.mark.gpu
WS_ODE_TLM = 18
ORDER = ("q", "p", "dq", "dp")


def _dev(a, dev):
    return {k: v.float().to(dev) for k, v in a.items()}


def _call(L, a, sigma, carried=True, need_self=True, sl=slice(None)):
    """_lib.ode_tlm on the device inputs a, directions a[...][sl]."""
    return L.ode_tlm(a["q"], a["p"], a["dq"][sl], a["dp"][sl], sigma, a["x"] if carried else None,
                     a["dx"][sl] if carried else None, need_self=need_self)


def _same(u, v):
    """Bitwise equality of two result tuples (NaNs in the same places, with the same payload)."""
    return all((s is None and t is None) or torch.equal(s.view(torch.int32), t.view(torch.int32))
               for s, t in zip(u, v))


# ---------------------------------------------------------------------------------------
# 1. one pass against float64
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("D,sigma,shift", T.PASS_CASES)
def test_one_pass_vs_float64(dev, D, sigma, shift, L):
    from difficp_amd import _lib
    worst = 0.0
    for M, N in T.PASS_SHAPES:
        a = T.pass_inputs(D, M, N, L, shift)
        got = _call(_lib, _dev(a, dev), sigma)
        assert [tuple(g.shape) for g in got] == [(L, M, D), (L, M, D), (L, N, D)]
        f64 = T.r64(a)
        want = T.tlm(*[f64[k] for k in ORDER], sigma, f64["x"], f64["dx"])
        e = T.nerr(got, want)
        worst = max(worst, e)
        assert e < T.TOL64, (M, N, e)
    print(f"ode_tlm D={D} sigma={sigma} shift={shift} L={L}: worst {worst:.2e} = {worst / T.TOL64:.3f} tol")


@pytest.mark.parametrize("D", [2, 3])
def test_first_split_support(dev, D):
    """The smallest support the library splits into column chunks (partial slabs + merge): one chunk
    just below it, so the merge path is really taken; and a few chunks more."""
    from difficp_amd import _lib
    M = next(m for m in range(1, 1 << 16) if _lib.num_splits(WS_ODE_TLM, m, 300) >= 2)
    assert _lib.num_splits(WS_ODE_TLM, M - 1, 300) == 1
    for m, n in ((M, 300), (M - 1, 300), (5 * M + 77, 129)):
        a = T.pass_inputs(D, m, n, 2, 0.0, seed=1)
        got = _call(_lib, _dev(a, dev), 0.3)
        f64 = T.r64(a)
        e = T.nerr(got, T.tlm(*[f64[k] for k in ORDER], 0.3, f64["x"], f64["dx"]))
        print(f"ode_tlm D={D} M={m} N={n} ({_lib.num_splits(WS_ODE_TLM, m, n)} chunks): {e:.2e}")
        assert e < T.TOL64


# ---------------------------------------------------------------------------------------
# 2. bits
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,M,N", [(3, 1030, 513), (2, 257, 700)])
def test_bitwise_properties(dev, D, M, N):
    from difficp_amd import _lib
    a = _dev(T.pass_inputs(D, M, N, 5, 0.0, seed=2), dev)
    five = _call(_lib, a, 0.3)
    assert _same(five, _call(_lib, a, 0.3))                                   # a repeated call
    for l in range(5):                                                        # alone = among five
        alone = _call(_lib, a, 0.3, sl=slice(l, l + 1))
        assert _same(alone, [o[l:l + 1] for o in five])
    perm = [3, 0, 4, 2, 1]
    b = dict(a, **{k: a[k][perm].contiguous() for k in ("dq", "dp", "dx")})
    assert _same(_call(_lib, b, 0.3), [o[perm] for o in five])                # permuted directions
    only = _call(_lib, a, 0.3, need_self=False)
    assert only[0] is None and only[1] is None and _same(only[2:], five[2:])  # the carried part alone
    noext = _call(_lib, a, 0.3, carried=False)
    assert noext[2] is None and _same(noext[:2], five[:2])                    # the self part alone
    z = dict(a, **{k: torch.zeros_like(a[k]) for k in ("dq", "dp", "dx")})
    assert all(bool((o == 0).all()) for o in _call(_lib, z, 0.3))             # zero directions: zero


def test_non_finite_input_stays_in_its_direction_and_row(dev):
    from difficp_amd import _lib
    a = _dev(T.pass_inputs(3, 1030, 513, 4, 0.0, seed=3), dev)
    clean = _call(_lib, a, 0.3)
    b = {k: v.clone() for k, v in a.items()}
    b["dp"][2, 517, 1] = float("nan")
    out = _call(_lib, b, 0.3)
    keep = [0, 1, 3]
    assert _same([o[keep] for o in out], [o[keep] for o in clean])
    assert bool(torch.isnan(out[0][2]).any()) and bool(torch.isnan(out[2][2]).any())
    c = {k: v.clone() for k, v in a.items()}
    c["dx"][1, 300, 0] = float("nan")
    out = _call(_lib, c, 0.3)
    assert _same(out[:2], clean[:2])
    bad = torch.zeros(4, 513, dtype=torch.bool, device=dev)
    bad[1, 300] = True
    assert bool(torch.isnan(out[2][bad]).all())
    assert torch.equal(out[2][~bad], clean[2][~bad])


def test_empty_calls(dev):
    from difficp_amd import _lib
    a = _dev(T.pass_inputs(3, 40, 30, 2, 0.0), dev)
    e = lambda *shape: torch.empty(shape, device=dev)
    # no support: the field and its tangent vanish
    dv, dmG, dvx = _lib.ode_tlm(e(0, 3), e(0, 3), e(2, 0, 3), e(2, 0, 3), 0.3, a["x"], a["dx"])
    assert dv.shape == dmG.shape == (2, 0, 3) and dvx.shape == (2, 30, 3) and bool((dvx == 0).all())
    # no carried points
    dv, dmG, dvx = _lib.ode_tlm(a["q"], a["p"], a["dq"], a["dp"], 0.3, e(0, 3), e(2, 0, 3))
    assert dvx.shape == (2, 0, 3) and _same((dv, dmG), _call(_lib, a, 0.3, carried=False)[:2])
    # no direction
    out = _lib.ode_tlm(a["q"], a["p"], a["dq"][:0], a["dp"][:0], 0.3, a["x"], a["dx"][:0])
    assert [tuple(o.shape) for o in out] == [(0, 40, 3), (0, 40, 3), (0, 30, 3)]
    with pytest.raises(ValueError, match="shaped"):
        _lib.ode_tlm(a["q"], a["p"], a["dq"], a["dp"][:1], 0.3)
    with pytest.raises(ValueError, match="shaped"):
        _lib.ode_tlm(a["q"], a["p"], a["dq"], a["dp"], 0.3, a["x"], a["dx"][:, :5])
    with pytest.raises(ValueError, match="together"):
        _lib.ode_tlm(a["q"], a["p"], a["dq"], a["dp"], 0.3, a["x"])


# ---------------------------------------------------------------------------------------
# 3. the flow
# ---------------------------------------------------------------------------------------
FLOW = [(D, scheme, version, sigma) for D in (2, 3) for scheme in ("Euler", "Ralston")
        for version in ("classic", "hybrid") for sigma in T.FLOW_SIGMAS]


@functools.lru_cache(maxsize=None)
def _flow_refs(D, scheme, version, sigma):
    """(inputs, float64 jvp of the oracle on the rounded inputs, e32)."""
    ref = T.oracle(D, scheme, sigma, version=version)
    a = T.flow_inputs(D)
    want = T.oracle_jvp(ref, **T.r64(a))
    e32 = T.nerr(T.shoot_tangent(ref, **T.r32(a)), want)
    return a, want, e32


def _model(D, scheme, version, sigma):
    from difficp_amd.core.LDDMM import LDDMMModel
    return LDDMMModel(sigma=sigma, D=D, lambd=10.0, version=version, scheme=scheme, nt=T.FLOW_NT)


@pytest.mark.parametrize("D,scheme,version,sigma", FLOW)
def test_shoot_tangent_vs_oracle_jvp(dev, D, scheme, version, sigma):
    a, want, e32 = _flow_refs(D, scheme, version, sigma)
    LM = _model(D, scheme, version, sigma)
    d = _dev(a, dev)
    got = LM.shoot_tangent(d["q0"], d["p0"], d["dp0"], d["dq0"], d["x0"], d["dx0"])
    e = T.nerr(got, want)
    tol = max(T.TOL64, 2 * e32)
    print(f"shoot_tangent D={D} {scheme} {version} sigma={sigma}: {e:.2e} (e32 {e32:.2e}) = {e / tol:.3f} tol")
    assert e < tol


@pytest.mark.parametrize("D,scheme,version,sigma", FLOW)
def test_adjoint_identity_with_the_device_vjp(dev, D, scheme, version, sigma):
    """sum_k <lambda_k, (J d)_k> from shoot_tangent equals sum <grad, d> from the hand-written VJP of
    the device shooting, within 2e-5 of the Cauchy-Schwarz scale sum_k |lambda_k| |(J d)_k| (a
    cancelling dot product cannot hide an error)."""
    a, _, _ = _flow_refs(D, scheme, version, sigma)
    LM = _model(D, scheme, version, sigma)
    d = _dev(a, dev)
    Jd = LM.shoot_tangent(d["q0"], d["p0"], d["dp0"], d["dq0"], d["x0"], d["dx0"])
    g = torch.Generator().manual_seed(9 + D)
    lam = [torch.randn(t.shape[1:], generator=g).to(dev) for t in Jd]
    prim = [d[k].clone().requires_grad_(True) for k in ("q0", "p0", "x0")]
    last = LM.Shoot(*prim)[-1]
    grads = torch.autograd.grad(sum((l * o).sum() for l, o in zip(lam, (last[0], last[1], last[3]))), prim)
    dot = lambda u, v: float((u.double() * v.double()).sum())
    worst = 0.0
    for l in range(T.FLOW_L):
        lhs = sum(dot(lm, o[l]) for lm, o in zip(lam, Jd))
        rhs = sum(dot(gr, d[k][l]) for gr, k in zip(grads, ("dq0", "dp0", "dx0")))
        scale = sum(float(lm.double().norm() * o[l].double().norm()) for lm, o in zip(lam, Jd))
        worst = max(worst, abs(lhs - rhs) / scale)
    print(f"adjoint identity D={D} {scheme} {version} sigma={sigma}: {worst:.2e} = {worst / T.TOL32:.3f} tol")
    assert worst <= T.TOL32


# ---------------------------------------------------------------------------------------
# 4. the interface
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["Euler", "Ralston"])
def test_registration_interface(dev, scheme):
    from difficp_amd.core.registrations import LDDMMRegistration
    LM = _model(3, scheme, "classic", 0.3)
    d = _dev(T.flow_inputs(3), dev)
    reg = LDDMMRegistration(LM, d["q0"], d["p0"])
    dQ, dP, dX = LM.shoot_tangent(d["q0"], d["p0"], d["dp0"], x0=d["x0"])
    S = reg.sensitivity(d["x0"], d["dp0"])
    assert S.shape == (T.FLOW_L, T.FLOW_N, 3) and torch.equal(S, dX)
    assert torch.equal(reg.sensitivity(d["x0"], d["dp0"][1]), dX[1])
    jQ, jP = reg.jacobi_field(d["dp0"])
    assert jQ.shape == jP.shape == (T.FLOW_NT + 1, T.FLOW_L, T.FLOW_M, 3)
    assert bool((jQ[0] == 0).all()) and torch.equal(jP[0], d["dp0"])
    assert torch.equal(jQ[-1], dQ) and torch.equal(jP[-1], dP)
    sh = LM.Shoot(d["q0"], d["p0"], need_p1=False)
    assert torch.equal(reg.sensitivity(d["x0"], d["dp0"], previous_forwardshoot=sh), S)
    # a step along the direction moves the map by the sensitivity, to second order
    eps = 1e-2
    moved = LDDMMRegistration(LM, d["q0"], d["p0"] + eps * d["dp0"][0]).apply(d["x0"]) - reg.apply(d["x0"])
    assert T.nerr([moved / eps], [S[0]]) < 0.1


def test_logdet_model_refused_and_model_untouched(dev):
    from difficp_amd.core.registrations import LDDMMRegistration
    d = _dev(T.flow_inputs(2), dev)
    with pytest.raises(ValueError, match="eta = 0"):
        _model(2, "Euler", "logdet", 0.3).shoot_tangent(d["q0"], d["p0"], d["dp0"])
    with pytest.raises(ValueError, match="eta = 0"):
        LDDMMRegistration(_model(2, "Euler", "logdet", 0.3), d["q0"], d["p0"]).sensitivity(d["x0"], d["dp0"])
    LM = _model(2, "Euler", "classic", 0.3)
    sh = LM.Shoot(d["q0"], d["p0"])                       # fills the model's shoot_cache
    cache = LM.shoot_cache
    before, state = dict(cache.__dict__), dict(LM.__dict__)
    out = LM.shoot_tangent(d["q0"], d["p0"], d["dp0"], d["dq0"], d["x0"], d["dx0"])
    assert all(not o.requires_grad for o in out)
    assert LM.shoot_cache is cache and cache.__dict__ == before and LM.__dict__ == state
    again = LM.Shoot(d["q0"], d["p0"])
    assert torch.equal(again.Q, sh.Q) and torch.equal(again.P, sh.P)
