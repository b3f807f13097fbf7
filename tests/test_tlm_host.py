"""dicp_lddmm_ode_tlm_f32 (csrc/tlm.hip) and the forward sensitivities above it, host side only:
the float64 pin of the closed forms of tests/tlm_ref.py (which the GPU tests compare the kernel
with) against forward-mode autograd through the oracle's Shoot and against its adjoint; the bound
on their float32 restatement; the symbol, the argument checks that come before any device work and
the workspace / split routing of kind DICP_WS_ODE_TLM; and LDDMMModel.shoot_tangent,
LDDMMRegistration.sensitivity / jacobi_field over a monkeypatched _lib.ode_tlm served by tlm_ref's
dense float64 statement (the rest of the library by tests/fake_hip.py)."""
import ctypes as C
import functools
import os

import pytest
import torch

import fake_hip
import tlm_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "diff-icp_amd", "libdifficp_hip.so")
WS_ODE_TLM = 18
TLM = "dicp_lddmm_ode_tlm_f32"
FLOW = [(D, scheme, sigma) for D in (2, 3) for scheme in ("Euler", "Ralston") for sigma in T.FLOW_SIGMAS]


# ---------------------------------------------------------------------------------------------
# float64: the closed forms against the oracle
@functools.lru_cache(maxsize=None)
def _flow64(D, scheme, sigma):
    ref = T.oracle(D, scheme, sigma)
    a = T.flow_inputs(D)
    return ref, a, T.oracle_jvp(ref, **a)


@pytest.mark.parametrize("D,scheme,sigma", FLOW)
def test_recurrences_against_oracle_jvp(D, scheme, sigma):
    """shoot_tangent's recurrences are the forward-mode derivative of the oracle's Shoot: <= 1e-12
    norm-wise (measured 5e-16)."""
    ref, a, want = _flow64(D, scheme, sigma)
    got = T.shoot_tangent(ref, **a)
    e = T.nerr(got, want)
    print(f"D={D} {scheme} sigma={sigma}: shoot_tangent vs jvp {e:.1e}")
    assert min(float(w.norm()) for w in want) > 1e-2          # a real sensitivity in every slot
    assert e <= 1e-12
    traj = T.shoot_tangent(ref, **a, trajectory=True)
    assert all(t.shape[0] == ref.nt + 1 for t in traj)
    assert T.nerr([t[-1] for t in traj], got) == 0.0
    assert torch.equal(traj[0][0], a["dq0"]) and torch.equal(traj[1][0], a["dp0"])


@pytest.mark.parametrize("D,sigma", [(D, s) for D in (2, 3) for s in T.FLOW_SIGMAS])
def test_one_pass_against_oracle_jvp(D, sigma):
    """tlm is the forward-mode derivative of the oracle's ODE (with carried points) at a state."""
    ref = T.oracle(D, "Euler", sigma)
    a = T.flow_inputs(D, seed=1)
    q, p, x = a["q0"], a["p0"], a["x0"]
    zero = torch.zeros(1, dtype=torch.float64)
    rhs = lambda q, p, x: tuple(ref.ODE(q, p, zero, x)[k] for k in (0, 1, 3))
    got = T.tlm(q, p, a["dq0"], a["dp0"], sigma, x, a["dx0"])
    for l in range(T.FLOW_L):
        want = torch.autograd.functional.jvp(rhs, (q, p, x), (a["dq0"][l], a["dp0"][l], a["dx0"][l]))[1]
        assert T.nerr([g[l] for g in got], want) <= 1e-12
    # the parts are independent of each other
    assert torch.equal(T.tlm(q, p, a["dq0"], a["dp0"], sigma, x, a["dx0"], need_self=False)[2], got[2])
    assert T.tlm(q, p, a["dq0"], a["dp0"], sigma)[2] is None


@pytest.mark.parametrize("D,scheme,sigma", FLOW)
def test_adjoint_identity(D, scheme, sigma):
    """<lambda, J d> = <J^T lambda, d> with J^T lambda from reverse-mode autograd through the oracle's
    Shoot: to 1e-10 of sum_k |lambda_k| |(J d)_k| (measured 7e-14)."""
    ref, a, _ = _flow64(D, scheme, sigma)
    Jd = T.shoot_tangent(ref, **a)
    g = torch.Generator().manual_seed(5 + D)
    lam = [torch.randn(t.shape[1:], generator=g, dtype=torch.float64) for t in Jd]
    prim = [a[k].clone().requires_grad_(True) for k in ("q0", "p0", "x0")]
    last = ref.Shoot(*prim)[-1]
    grads = torch.autograd.grad(sum((l * o).sum() for l, o in zip(lam, (last[0], last[1], last[3]))), prim)
    for l in range(T.FLOW_L):
        lhs = sum(float((lm * o[l]).sum()) for lm, o in zip(lam, Jd))
        rhs = sum(float((gr * a[k][l]).sum()) for gr, k in zip(grads, ("dq0", "dp0", "dx0")))
        scale = sum(float(lm.norm() * o[l].norm()) for lm, o in zip(lam, Jd))
        assert abs(lhs - rhs) <= 1e-10 * scale


# ---------------------------------------------------------------------------------------------
# the float32 restatement stays below half the device tolerance
@pytest.mark.parametrize("D,sigma,shift", T.PASS_CASES)
def test_restatement_one_pass(D, sigma, shift):
    """tlm in float32 on the kernel tests' largest inputs against float64 on the same rounded inputs
    (measured <= 4.5e-7)."""
    a = T.pass_inputs(D, 1030, 513, 3, shift)
    order = ("q", "p", "dq", "dp")
    f32, f64 = T.r32(a), T.r64(a)
    got = T.tlm(*[f32[k] for k in order], sigma, f32["x"], f32["dx"])
    want = T.tlm(*[f64[k] for k in order], sigma, f64["x"], f64["dx"])
    e = T.nerr(got, want)
    print(f"D={D} sigma={sigma} shift={shift}: float32 restatement of one pass {e:.2e}")
    assert e < T.TOL64 / 2


@pytest.mark.parametrize("D,scheme,sigma", FLOW)
def test_restatement_flow(D, scheme, sigma):
    """shoot_tangent in float32 against the oracle's float64 jvp on the rounded inputs (measured
    <= 1.6e-6)."""
    ref = T.oracle(D, scheme, sigma)
    a = T.flow_inputs(D)
    e = T.nerr(T.shoot_tangent(ref, **T.r32(a)), T.oracle_jvp(ref, **T.r64(a)))
    print(f"D={D} {scheme} sigma={sigma}: float32 restatement of the flow {e:.2e}")
    assert e < T.TOL64 / 2


# ---------------------------------------------------------------------------------------------
# the C ABI
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built (run __graft_entry__.build())")
    h = C.CDLL(LIB)
    h.dicp_last_error.restype = C.c_char_p
    h.dicp_workspace_bytes.restype = C.c_size_t
    h.dicp_workspace_bytes.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int]
    h.dicp_num_splits.argtypes = [C.c_int, C.c_int64, C.c_int64]
    getattr(h, TLM).argtypes = [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 2 + [C.c_int64, C.c_int, C.c_int,
                                                                                  C.c_double] + [C.c_void_p] * 4 + \
        [C.c_size_t, C.c_void_p]
    return h


# addresses that are never read: every refusal below comes before any device work
PTR = dict(q=0x1000, p=0x2000, dq=0x3000, dp=0x4000, x=0x5000, dx=0x6000, dv=0x7000, dmG=0x8000, dvx=0x9000)


def _tlm(lib, M=5, N=5, L=2, D=3, sigma=0.5, ws_bytes=0, **ptr):
    a = dict(PTR, **ptr)
    return getattr(lib, TLM)(a["q"], a["p"], a["dq"], a["dp"], M, a["x"], a["dx"], N, L, D, sigma, a["dv"], a["dmG"],
                             a["dvx"], None, ws_bytes, None)


def test_symbol_exported_and_bound(lib):
    from difficp_amd import _lib
    assert hasattr(lib, TLM)
    assert TLM in _lib.EXPORTED_SYMBOLS and TLM in _lib._SIGNATURES
    assert _lib.WS_ODE_TLM == WS_ODE_TLM
    assert "ode_tlm" in _lib.FLOPS_PER_PAIR
    with open(os.path.join(ROOT, "include", "difficp_hip.h")) as f:
        header = f.read()
    assert TLM in header and "DICP_WS_ODE_TLM = 18" in header


@pytest.mark.parametrize("bad", [dict(M=-1), dict(N=-1), dict(L=-1), dict(L=65536), dict(sigma=0.0),
                                 dict(sigma=-1.0), dict(sigma=float("nan")), dict(q=None), dict(p=None),
                                 dict(dq=None), dict(dp=None), dict(dx=None), dict(dvx=None),
                                 dict(dv=PTR["dq"]), dict(dmG=PTR["p"]), dict(dvx=PTR["x"])])
def test_invalid_arguments(lib, bad):
    assert _tlm(lib, **bad) == 1
    assert b"invalid" in lib.dicp_last_error()


def test_unsupported_dimension(lib):
    assert _tlm(lib, D=7) == 2
    assert b"unsupported" in lib.dicp_last_error()
    assert _tlm(lib, D=1) == 2


def test_workspace_too_small_is_refused(lib):
    assert _tlm(lib, M=2000, N=10) == 3                       # DICP_ERR_WORKSPACE: the support is split
    assert b"workspace" in lib.dicp_last_error()


def test_nothing_to_do_is_ok(lib):
    """No direction, or no part asked for: success without touching a pointer."""
    assert _tlm(lib, L=0) == 0
    assert _tlm(lib, L=0, q=None, p=None, dq=None, dp=None, x=None, dx=None, dv=None, dmG=None, dvx=None) == 0
    assert _tlm(lib, M=0, N=0, q=None, p=None, dq=None, dp=None) == 0
    assert _tlm(lib, x=None, dx=None, dvx=None, dv=None, dmG=None) == 0      # neither part
    assert _tlm(lib, N=0, dv=None, dmG=None) == 0


def test_workspace_kind_routed(lib):
    """Bytes (of one direction) and column chunks of kind 18: non-decreasing in the support size M
    and in the number N of carried points; the bytes cover both parts' slabs."""
    sizes = [0, 1, 2, 255, 256, 257, 511, 512, 513, 1000, 1024, 1025, 2047, 2048, 2049, 5000, 20000, 32767,
             32768, 32769, 50000, 100000, 131071, 131072, 131073, 200000, 1000000]
    for D in (2, 3):
        for fixed in (0, 1, 700, 300000):
            for order in ("M", "N"):
                prev_b = prev_s = 0
                for n in sizes:
                    M, N = (n, fixed) if order == "M" else (fixed, n)
                    b, S = lib.dicp_workspace_bytes(WS_ODE_TLM, M, N, D), lib.dicp_num_splits(WS_ODE_TLM, M, N)
                    assert S >= 1 and b >= prev_b and S >= prev_s, (D, M, N)
                    if S > 1:
                        assert b >= 4 * S * D * max(2 * M, N)
                    else:
                        assert b == 0
                    prev_b, prev_s = b, S
    # dense around every point where the chunk rule changes
    for lo, hi in ((500, 530), (32700, 32800), (131000, 131200)):
        S = [lib.dicp_num_splits(WS_ODE_TLM, M, 7) for M in range(lo, hi)]
        assert S == sorted(S)
    assert lib.dicp_num_splits(WS_ODE_TLM, 512, 5) == 1 and lib.dicp_num_splits(WS_ODE_TLM, 513, 5) == 2
    assert lib.dicp_workspace_bytes(WS_ODE_TLM, 20000, 700, 7) == 0


def test_binding_refuses_host_tensors_and_bad_shapes():
    from difficp_amd import _lib
    q, d = torch.rand(4, 3), torch.rand(2, 4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.ode_tlm(q, q, d, d, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.ode_tlm(q, q, d, d, 0.5, x=q, dx=d, need_self=False)


# ---------------------------------------------------------------------------------------------
# the Python layers over the dense float64 statement
@pytest.fixture()
def patched(monkeypatch):
    from difficp_amd import _lib
    calls = []

    def fake(q, p, dq, dp, sigma, x=None, dx=None, need_self=True):
        calls.append((dq.shape[0], x is not None, need_self))
        return T.ode_tlm(q, p, dq, dp, sigma, x, dx, need_self)

    fake_hip.install(monkeypatch)
    monkeypatch.setattr(_lib, "ode_tlm", fake)
    return calls


def _model(D=2, sigma=0.3, version="classic", scheme="Euler", nt=4):
    from difficp_amd.core.LDDMM import LDDMMModel
    from difficp_amd.tools.spec import cpuspec
    return LDDMMModel(sigma=sigma, D=D, lambd=10.0, version=version, scheme=scheme, nt=nt, spec=cpuspec)


def _args(D, M=23, N=11, L=3):
    a = T.flow_inputs(D, seed=2, M=M, N=N, L=L)
    return {k: v.float() for k, v in a.items()}


@pytest.mark.parametrize("scheme", ["Euler", "Ralston"])
@pytest.mark.parametrize("version", ["classic", "hybrid"])
@pytest.mark.parametrize("D", [2, 3])
def test_shoot_tangent_is_the_reference_recurrence(patched, scheme, version, D):
    """The model's loop over the stand-in is tlm_ref.shoot_tangent over the oracle (float32 states,
    float64 passes: to float32 rounding), final time and trajectory."""
    LM = _model(D, version=version, scheme=scheme)
    a = _args(D)
    ref = T.oracle(D, scheme, LM.sigma, nt=LM.nt)
    got = LM.shoot_tangent(a["q0"], a["p0"], a["dp0"], a["dq0"], a["x0"], a["dx0"])
    want = T.shoot_tangent(ref, **{k: v.double() for k, v in a.items()})
    assert [tuple(g.shape) for g in got] == [(3, 23, D), (3, 23, D), (3, 11, D)]
    assert T.nerr(got, want) < 2e-6
    stages = LM.nt * (1 if scheme == "Euler" else 2)
    assert patched == [(3, True, True)] * stages              # one pass per stage, all directions
    traj = LM.shoot_tangent(a["q0"], a["p0"], a["dp0"], a["dq0"], a["x0"], a["dx0"], trajectory=True)
    assert [tuple(t.shape) for t in traj] == [(LM.nt + 1, 3, 23, D), (LM.nt + 1, 3, 23, D), (LM.nt + 1, 3, 11, D)]
    for t, g, first in zip(traj, got, (a["dq0"], a["dp0"], a["dx0"])):
        assert torch.equal(t[-1], g) and torch.equal(t[0], first)


def test_shapes_defaults_and_squeezing(patched):
    LM = _model(3)
    a = _args(3)
    q0, p0, x0 = a["q0"], a["p0"], a["x0"]
    dQ, dP, dX = LM.shoot_tangent(q0, p0, a["dp0"][1])
    assert dQ.shape == dP.shape == q0.shape and dX is None
    assert patched[0] == (1, False, True)
    # dq0 = None and dx0 = None are zeros
    full = LM.shoot_tangent(q0, p0, a["dp0"], torch.zeros_like(a["dq0"]), x0, torch.zeros_like(a["dx0"]))
    dflt = LM.shoot_tangent(q0, p0, a["dp0"], x0=x0)
    assert all(torch.equal(u, v) for u, v in zip(full, dflt))
    # a 2-D direction is direction 1 of the stack, squeezed
    one = LM.shoot_tangent(q0, p0, a["dp0"][1], a["dq0"][1], x0, a["dx0"][1])
    many = LM.shoot_tangent(q0, p0, a["dp0"], a["dq0"], x0, a["dx0"])
    assert [o.dim() for o in one] == [2, 2, 2]
    assert all(torch.equal(o, m[1]) for o, m in zip(one, many))
    # no direction at all
    none = LM.shoot_tangent(q0, p0, a["dp0"][:0], x0=x0)
    assert [tuple(o.shape) for o in none] == [(0, 23, 3), (0, 23, 3), (0, 11, 3)]
    with pytest.raises(ValueError, match="shaped"):
        LM.shoot_tangent(q0, p0, a["dp0"][:, :5])
    with pytest.raises(ValueError, match="shaped"):
        LM.shoot_tangent(q0, p0, a["dp0"], a["dq0"][:2])
    with pytest.raises(ValueError, match="shaped"):
        LM.shoot_tangent(q0, p0, a["dp0"], x0=x0, dx0=a["dx0"][:, :4])
    with pytest.raises(ValueError, match="x0"):
        LM.shoot_tangent(q0, p0, a["dp0"], dx0=a["dx0"])


@pytest.mark.parametrize("scheme", ["Euler", "Ralston"])
def test_linear_in_the_directions(patched, scheme):
    LM = _model(2, scheme=scheme)
    a = {k: v.double() for k, v in _args(2).items()}
    base = (a["q0"], a["p0"])
    f = lambda dp, dq, dx: LM.shoot_tangent(*base, dp, dq, a["x0"], dx)
    u = f(a["dp0"][0], a["dq0"][0], a["dx0"][0])
    v = f(a["dp0"][1], a["dq0"][1], a["dx0"][1])
    w = f(2 * a["dp0"][0] - 3 * a["dp0"][1], 2 * a["dq0"][0] - 3 * a["dq0"][1], 2 * a["dx0"][0] - 3 * a["dx0"][1])
    assert T.nerr(w, [2 * s - 3 * t for s, t in zip(u, v)]) < 1e-13
    zero = f(0 * a["dp0"], 0 * a["dq0"], 0 * a["dx0"])
    assert all(bool((z == 0).all()) for z in zero)


def test_eta_refused(patched):
    LM = _model(2, version="logdet")
    a = _args(2)
    with pytest.raises(ValueError, match="eta = 0"):
        LM.shoot_tangent(a["q0"], a["p0"], a["dp0"])
    from difficp_amd.core.registrations import LDDMMRegistration
    reg = LDDMMRegistration(LM, a["q0"], a["p0"])
    with pytest.raises(ValueError, match="eta = 0"):
        reg.sensitivity(a["x0"], a["dp0"])
    with pytest.raises(ValueError, match="eta = 0"):
        reg.jacobi_field(a["dp0"])
    assert patched == []


@pytest.mark.parametrize("scheme", ["Euler", "Ralston"])
def test_registration_interface(patched, scheme):
    from difficp_amd.core.registrations import LDDMMRegistration
    LM = _model(3, scheme=scheme)
    a = _args(3)
    reg = LDDMMRegistration(LM, a["q0"], a["p0"])
    S = reg.sensitivity(a["x0"], a["dp0"])
    # the last stage ran the carried part alone
    assert patched[-1] == (3, True, False) and all(c == (3, True, True) for c in patched[:-1])
    dX = LM.shoot_tangent(a["q0"], a["p0"], a["dp0"], x0=a["x0"])[2]
    assert S.shape == (3, 11, 3) and torch.equal(S, dX)
    assert torch.equal(reg.sensitivity(a["x0"], a["dp0"][2]), dX[2])
    S2 = reg.sensitivity(a["x0"], a["dp0"], a["dq0"])
    assert torch.equal(S2, LM.shoot_tangent(a["q0"], a["p0"], a["dp0"], a["dq0"], a["x0"])[2])
    assert not torch.equal(S2, S)
    dQ, dP = reg.jacobi_field(a["dp0"])
    assert dQ.shape == dP.shape == (LM.nt + 1, 3, 23, 3)
    assert bool((dQ[0] == 0).all()) and torch.equal(dP[0], a["dp0"])
    fin = LM.shoot_tangent(a["q0"], a["p0"], a["dp0"])
    assert torch.equal(dQ[-1], fin[0]) and torch.equal(dP[-1], fin[1])
    dQ1, dP1 = reg.jacobi_field(a["dp0"][0])
    assert dQ1.shape == (LM.nt + 1, 23, 3) and torch.equal(dQ1, dQ[:, 0])
    # a forward shoot is reused, with or without its final momenta
    sh = LM.Shoot(a["q0"], a["p0"], need_p1=False)
    assert torch.equal(reg.sensitivity(a["x0"], a["dp0"], previous_forwardshoot=sh), S)


def test_model_and_cache_untouched(patched):
    LM = _model(2)
    a = _args(2)
    a["p0"].requires_grad_(True)
    sh = LM.Shoot(a["q0"], a["p0"])
    cache = LM.shoot_cache
    before = dict(cache.__dict__)
    state = {k: v for k, v in LM.__dict__.items()}
    out = LM.shoot_tangent(a["q0"], a["p0"], a["dp0"], a["dq0"], a["x0"], a["dx0"])
    assert all(not o.requires_grad for o in out)
    assert LM.shoot_cache is cache and cache.__dict__ == before
    assert LM.__dict__ == state
    again = LM.Shoot(a["q0"], a["p0"])
    assert torch.equal(again.Q, sh.Q) and torch.equal(again.P, sh.P)
