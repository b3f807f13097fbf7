"""Hessian-vector products of the shooting loss on the device (csrc/hvp.hip and the methods built on
it): the second-order kernel dicp_lddmm_ode_hvp_f32, LDDMMModel.loss_hvp / loss_hessian_extremes
for both integration schemes and DiffPSR.frame_hvp -- against the float64 closed forms and
recursions of tests/hvp_ref.py (pinned against autograd through the oracle by
tests/test_hvp_host.py) and against central differences of the oracle's float64 gradients.

Tolerances (norm-wise relative): 1e-5 against float64 on the float32-rounded inputs;
2e-5 between two float32 results; the flow within max(1e-5, 2 e32), e32 being the error of the same
recursion run in float32 on the CPU (the reference's own drift, computed here)."""
import functools

import pytest
import torch

import hvp_ref as H

pytestmark = pytest.mark.gpu
WS_ODE_HVP = 19
ORDER = ("q", "p", "aq", "ap", "bq", "bp")
GDIV = 0.7


def _dev(a, dev):
    return {k: v.float().to(dev) for k, v in a.items()}


def _call(L, a, sigma, gdiv=None, sl=slice(None)):
    """_lib.ode_hvp on the device inputs a, directions a[...][sl]."""
    g = None if gdiv is None else torch.full((1,), gdiv, device=a["q"].device)
    return L.ode_hvp(a["q"], a["p"], a["aq"], a["ap"], a["bq"][sl], a["bp"][sl], sigma, g)


def _same(u, v):
    """Bitwise equality of two result tuples (NaNs in the same places, with the same payload)."""
    return all(torch.equal(s.view(torch.int32), t.view(torch.int32)) for s, t in zip(u, v))


def _three(a):
    """The three calls every size is checked with: T alone, T + gdiv D^2 C, the cost terms alone."""
    zero = dict(a, aq=torch.zeros_like(a["aq"]), ap=torch.zeros_like(a["ap"]))
    return (("T", a, None), ("T+C", a, GDIV), ("C", zero, GDIV))


# ---------------------------------------------------------------------------------------
# 1. one pass against float64
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("D,sigma,shift", H.PASS_CASES)
def test_one_pass_vs_float64(dev, D, sigma, shift, L):
    from difficp_amd import _lib
    worst = 0.0
    for M in H.SIZES:
        a = H.pass_inputs(D, M, L, shift)
        f64 = H.r64(a)
        t64 = H.third(*[f64[k] for k in ORDER], sigma)
        c64 = H.cost_hess(f64["q"], f64["p"], f64["bq"], f64["bp"], sigma)
        want = {"T": t64, "T+C": tuple(t + GDIV * c for t, c in zip(t64, c64)), "C": tuple(GDIV * c for c in c64)}
        for name, inp, g in _three(_dev(a, dev)):
            got = _call(_lib, inp, sigma, g)
            assert [tuple(o.shape) for o in got] == [(L, M, D), (L, M, D)]
            e = H.nerr(got, want[name])
            worst = max(worst, e)
            assert e < H.TOL64, (M, name, e)
    print(f"ode_hvp D={D} sigma={sigma} shift={shift} L={L}: worst {worst:.2e} = {worst / H.TOL64:.3f} tol")


@pytest.mark.parametrize("D", [2, 3])
def test_first_split_support(dev, D):
    """The smallest support the library splits into column chunks (partial slabs + merge): one chunk
    just below it, so the merge path is really taken; and a few chunks more."""
    from difficp_amd import _lib
    M = next(m for m in range(1, 1 << 16) if _lib.num_splits(WS_ODE_HVP, m, 0) >= 2)
    assert _lib.num_splits(WS_ODE_HVP, M - 1, 0) == 1
    for m in (M, M - 1, 5 * M + 77):
        a = H.pass_inputs(D, m, 2, 0.0, seed=1)
        f64 = H.r64(a)
        for g in (None, GDIV):
            e = H.nerr(_call(_lib, _dev(a, dev), 0.3, g), H.hvp_pass(*[f64[k] for k in ORDER], 0.3, g))
            print(f"ode_hvp D={D} M={m} gdiv={g} ({_lib.num_splits(WS_ODE_HVP, m, 0)} chunks): {e:.2e}")
            assert e < H.TOL64


# ---------------------------------------------------------------------------------------
# 2. bits
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,M,gdiv", [(3, 1030, GDIV), (2, 257, None), (3, 300, None)])
def test_bitwise_properties(dev, D, M, gdiv):
    from difficp_amd import _lib
    a = _dev(H.pass_inputs(D, M, 5, 0.0, seed=2), dev)
    five = _call(_lib, a, 0.3, gdiv)
    assert _same(five, _call(_lib, a, 0.3, gdiv))                              # a repeated call
    for l in range(5):                                                         # alone = among five
        assert _same(_call(_lib, a, 0.3, gdiv, sl=slice(l, l + 1)), [o[l:l + 1] for o in five])
    perm = [3, 0, 4, 2, 1]
    b = dict(a, bq=a["bq"][perm].contiguous(), bp=a["bp"][perm].contiguous())
    assert _same(_call(_lib, b, 0.3, gdiv), [o[perm] for o in five])           # permuted directions
    z = dict(a, bq=torch.zeros_like(a["bq"]), bp=torch.zeros_like(a["bp"]))
    assert all(bool((o == 0).all()) for o in _call(_lib, z, 0.3, gdiv))        # b = 0: exact zeros
    if gdiv is None:                                                           # T(a, b) = T(b, a)
        ab = [o[0] for o in five]
        s = dict(a, aq=a["bq"][0].contiguous(), ap=a["bp"][0].contiguous(), bq=a["aq"][None].contiguous(),
                 bp=a["ap"][None].contiguous())
        ba = [o[0] for o in _call(_lib, s, 0.3)]
        e = H.nerr(ab, ba)
        print(f"ode_hvp D={D} M={M}: T(a, b) vs T(b, a) {e:.2e} = {e / H.TOL32:.3f} tol")
        assert e < H.TOL32


def test_non_finite_direction_stays_in_its_direction(dev):
    from difficp_amd import _lib
    a = _dev(H.pass_inputs(3, 1030, 4, 0.0, seed=3), dev)
    clean = _call(_lib, a, 0.3, GDIV)
    b = {k: v.clone() for k, v in a.items()}
    b["bp"][2, 517, 1] = float("nan")
    out = _call(_lib, b, 0.3, GDIV)
    keep = [0, 1, 3]
    assert _same([o[keep] for o in out], [o[keep] for o in clean])
    assert bool(torch.isnan(out[0][2]).any()) and bool(torch.isnan(out[1][2]).any())


def test_empty_calls(dev):
    from difficp_amd import _lib
    a = _dev(H.pass_inputs(3, 40, 2, 0.0), dev)
    e = lambda *shape: torch.empty(shape, device=dev)
    oq, op = _lib.ode_hvp(e(0, 3), e(0, 3), e(0, 3), e(0, 3), e(2, 0, 3), e(2, 0, 3), 0.3)   # no support
    assert oq.shape == op.shape == (2, 0, 3)
    out = _call(_lib, a, 0.3, GDIV, sl=slice(0, 0))                                          # no direction
    assert [tuple(o.shape) for o in out] == [(0, 40, 3), (0, 40, 3)]
    with pytest.raises(ValueError, match="shaped"):
        _lib.ode_hvp(a["q"], a["p"], a["aq"], a["ap"], a["bq"], a["bp"][:1], 0.3)
    with pytest.raises(ValueError, match="shaped"):
        _lib.ode_hvp(a["q"], a["p"], a["aq"][:5], a["ap"][:5], a["bq"], a["bp"], 0.3)
    with pytest.raises(ValueError, match="shaped"):
        _lib.ode_hvp(a["q"], a["p"][:5], a["aq"], a["ap"], a["bq"], a["bp"], 0.3)
    with pytest.raises(ValueError, match="shaped"):
        _lib.ode_hvp(a["q"], a["p"], a["aq"], a["ap"], a["bq"], a["bp"], 0.3, torch.ones(2, device=dev))


# ---------------------------------------------------------------------------------------
# 3. the flow
# ---------------------------------------------------------------------------------------
FLOW = [(D, scheme, version, sigma) for D in (2, 3) for scheme in ("Euler", "Ralston")
        for version in ("classic", "hybrid") for sigma in H.FLOW_SIGMAS]
CMUL = 3.0


@functools.lru_cache(maxsize=None)
def _flow_refs(D, scheme, version, sigma):
    """(oracle, inputs, {gauss_newton: (float64 recursion on the rounded inputs, e32)})."""
    ref = H.oracle(D, scheme, sigma, version=version)
    a = H.flow_inputs(D)
    f64, f32 = H.r64(a), H.r32(a)
    out = {}
    for gn in (False, True):
        _, g64, h64 = H.cubic_data(f64["y"], CMUL)
        _, g32, h32 = H.cubic_data(f32["y"], CMUL)
        want = H.loss_hvp(ref, f64["q0"], f64["p0"], f64["d"], g64, h64, gauss_newton=gn)
        e32 = H.nerr((H.loss_hvp(ref, f32["q0"], f32["p0"], f32["d"], g32, h32, gauss_newton=gn),), (want,))
        out[gn] = (want, e32)
    return ref, a, out


def _model(D, scheme, version, sigma):
    from difficp_amd.core.LDDMM import LDDMMModel
    return LDDMMModel(sigma=sigma, D=D, lambd=10.0, version=version, scheme=scheme, nt=H.FLOW_NT)


def _data(y):
    loss, _, hv = H.cubic_data(y, CMUL)
    data = lambda x: loss(x)
    data.hvp = hv
    return data


_DEVICE_HVP = {}


def _device_hvp(dev, D, scheme, version, sigma):
    """loss_hvp on the device, exact and Gauss-Newton, once per case."""
    key = (D, scheme, version, sigma)
    if key not in _DEVICE_HVP:
        d = _dev(_flow_refs(*key)[1], dev)
        LM = _model(*key)
        _DEVICE_HVP[key] = {gn: LM.loss_hvp(_data(d["y"]), d["q0"], d["p0"], d["d"], gauss_newton=gn)
                            for gn in (False, True)}
    return _DEVICE_HVP[key]


@pytest.mark.parametrize("D,scheme,version,sigma", FLOW)
def test_loss_hvp_vs_float64_recursion(dev, D, scheme, version, sigma):
    _, a, refs = _flow_refs(D, scheme, version, sigma)
    got = _device_hvp(dev, D, scheme, version, sigma)
    for gn in (False, True):
        want, e32 = refs[gn]
        assert got[gn].shape == want.shape
        e = H.nerr((got[gn],), (want,))
        tol = max(H.TOL64, 2 * e32)
        print(f"loss_hvp D={D} {scheme} {version} sigma={sigma} {'Gauss-Newton' if gn else 'exact'}: {e:.2e} "
              f"(e32 {e32:.2e}) = {e / tol:.3f} tol")
        assert e < tol


@pytest.mark.parametrize("D,scheme,version,sigma", FLOW)
def test_product_is_symmetric(dev, D, scheme, version, sigma):
    """|<d1, H d2> - <d2, H d1>| <= tol (|d1| |H d2| + |d2| |H d1|) with tol the bound of
    test_loss_hvp_vs_float64_recursion: the exact operator is symmetric, so this follows from that
    bound by the triangle inequality."""
    _, a, refs = _flow_refs(D, scheme, version, sigma)
    got = _device_hvp(dev, D, scheme, version, sigma)
    d = a["d"].float().double()
    for gn in (False, True):
        Hd = got[gn].double().cpu()
        tol = max(H.TOL64, 2 * refs[gn][1])
        worst = 0.0
        for i in range(H.FLOW_L):
            for j in range(i):
                lhs, rhs = float((d[i] * Hd[j]).sum()), float((d[j] * Hd[i]).sum())
                scale = float(d[i].norm() * Hd[j].norm() + d[j].norm() * Hd[i].norm())
                worst = max(worst, abs(lhs - rhs) / scale)
        print(f"symmetry D={D} {scheme} {version} sigma={sigma} gn={gn}: {worst:.2e} = {worst / tol:.3f} tol")
        assert worst <= tol


@pytest.mark.parametrize("D,scheme,version,sigma", [c for c in FLOW if c[0] == 3])
def test_consistent_with_differences_of_the_adjoint(dev, D, scheme, version, sigma):
    """The product is the central difference of the loss gradients -- the oracle's float64 autograd
    gradient at p0 +- eps d, the float64 counterpart of shoot_loss_grad, never the code under test.
    eps = 1e-4: the truncation ~ eps^2 and the rounding ~ 1e-16 / eps are both far below the bound."""
    ref, a, refs = _flow_refs(D, scheme, version, sigma)
    got = _device_hvp(dev, D, scheme, version, sigma)[False]
    f64 = H.r64(a)
    f = H.oracle_loss(ref, f64["q0"], H.cubic_data(f64["y"], CMUL)[0])

    def grad(p):
        p = p.clone().requires_grad_(True)
        return torch.autograd.grad(f(p), p)[0]

    eps = 1e-4
    l = 1
    fd = (grad(f64["p0"] + eps * f64["d"][l]) - grad(f64["p0"] - eps * f64["d"][l])) / (2 * eps)
    e = H.nerr((got[l],), (fd,))
    tol = max(H.TOL64, 2 * refs[False][1])
    print(f"central difference D={D} {scheme} {version} sigma={sigma}: {e:.2e} = {e / tol:.3f} tol")
    assert e < tol


@pytest.mark.parametrize("scheme,version", [("Euler", "hybrid"), ("Ralston", "classic")])
def test_hessian_extremes(dev, scheme, version):
    """lambda_max by Lanczos on the device against the same Lanczos over the float64 recursion on
    the CPU, within max(1e-5, 2 e32), e32 from the same Lanczos over the float32 recursion."""
    from difficp_amd.tools.lanczos import lanczos
    D, M, sigma, steps, seed = 2, 40, 0.3, 12, 4
    ref = H.oracle(D, scheme, sigma, version=version)
    a = H.flow_inputs(D, seed=5, M=M)

    def host(b):
        _, g, hv = H.cubic_data(b["y"], CMUL)
        mv = lambda v: H.loss_hvp(ref, b["q0"], b["p0"], v.reshape(1, M, D), g, hv).reshape(-1)
        gen = torch.Generator().manual_seed(seed)
        v0 = torch.randn(M * D, generator=gen, dtype=torch.float64).to(b["q0"].dtype)
        return lanczos(mv, v0, steps)[0]

    r64, r32 = host(H.r64(a)), host(H.r32(a))
    d = _dev(a, dev)
    LM = _model(D, scheme, version, sigma)
    ritz, vmin, vmax = LM.loss_hessian_extremes(_data(d["y"]), d["q0"], d["p0"], steps, seed=seed)
    assert ritz.shape == (steps,) and vmin.shape == vmax.shape == d["p0"].shape and vmax.device == d["p0"].device
    e32 = abs(r32[-1] - r64[-1]) / abs(r64[-1])
    e = abs(ritz[-1] - r64[-1]) / abs(r64[-1])
    tol = max(H.TOL64, 2 * e32)
    print(f"lambda_max {scheme} {version}: {ritz[-1]:.6e} vs {r64[-1]:.6e}: {e:.2e} (e32 {e32:.2e}) = {e / tol:.3f} tol")
    assert e < tol
    # the Ritz value is the Rayleigh quotient of its vector (an identity of the iteration)
    Hv = LM.loss_hvp(_data(d["y"]), d["q0"], d["p0"], vmax)
    assert abs(float((Hv.double() * vmax.double()).sum()) - ritz[-1]) <= 1e-3 * abs(ritz[-1])


# ---------------------------------------------------------------------------------------
# 4. the interface
# ---------------------------------------------------------------------------------------
def test_frame_hvp(dev):
    from difficp_amd.core.GMM import GaussianMixtureUnif
    from difficp_amd.core.LDDMM import LDDMMModel
    from difficp_amd.core.PSR import DiffPSR
    spec = {"device": dev, "dtype": torch.float32}
    g = torch.Generator().manual_seed(21)
    base = torch.rand(150, 2, generator=g)
    frames = [(base + 0.04 * torch.sin(3.0 * base.flip(1) + k)).to(dev) for k in range(2)]
    G = GaussianMixtureUnif(torch.zeros(10, 2), spec=spec)
    G.to_optimize = {"mu": True, "sigma": True, "w": True, "eta0": False}
    LM = LDDMMModel(sigma=0.2, D=2, lambd=5e2, version="hybrid", scheme="Euler", nt=10, spec=spec)
    torch.manual_seed(0)
    P = DiffPSR(frames, G, LM, dataspec=spec, compspec=spec)
    P.printstuff = False
    P.reinitialize_GMM()
    P.GMM_opt(max_iterations=10, tol=1e-3)
    P.Reg_opt(nmax=2, tol=1e-3)
    d = torch.randn(2, 150, 2, generator=g).to(dev)
    for k in range(2):
        got = P.frame_hvp(k, d)
        assert got.shape == d.shape and bool(torch.isfinite(got).all()) and float(got.norm()) > 0
        assert torch.equal(got, LM.loss_hvp(P.QuadLossFunctor(k), P.q0[k], P.a0[k], d))
        assert torch.equal(P.frame_hvp(k, d[1]), got[1])
        # the functor's own Hessian is the one double-backward finds
        plain = P.QuadLossFunctor(k)
        auto = LM.loss_hvp(lambda x: plain(x), P.q0[k], P.a0[k], d)
        assert H.nerr((got,), (auto,)) < H.TOL32
        gn = P.frame_hvp(k, d, gauss_newton=True)
        assert all(float((d[l] * gn[l]).sum()) >= 0 for l in range(2))
    P.set_support_scheme("grid", rho=1.0)
    with pytest.raises(ValueError, match="dense support"):
        P.frame_hvp(0, d)


def test_refusals_and_model_untouched(dev):
    d = _dev(H.flow_inputs(2), dev)
    data = _data(d["y"])
    with pytest.raises(ValueError, match="eta = 0"):
        _model(2, "Euler", "logdet", 0.3).loss_hvp(data, d["q0"], d["p0"], d["d"])
    LM = _model(2, "Euler", "hybrid", 0.3)
    with pytest.raises(ValueError, match="carries points"):
        LM.loss_hvp(data, d["q0"], d["p0"], d["d"], shoot=LM.Shoot(d["q0"], d["p0"], d["y"][:7]))
    sh = LM.Shoot(d["q0"], d["p0"])                       # fills the model's shoot_cache
    cache = LM.shoot_cache
    before, state = dict(cache.__dict__), dict(LM.__dict__)
    out = LM.loss_hvp(data, d["q0"], d["p0"], d["d"])
    assert not out.requires_grad
    assert torch.equal(LM.loss_hvp(data, d["q0"], d["p0"], d["d"], shoot=sh), out)
    assert LM.shoot_cache is cache and cache.__dict__ == before and LM.__dict__ == state
    again = LM.Shoot(d["q0"], d["p0"])
    assert torch.equal(again.Q, sh.Q) and torch.equal(again.P, sh.P)
