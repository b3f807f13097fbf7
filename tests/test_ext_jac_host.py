"""dicp_lddmm_ode_ext_jac_f32 / dicp_lddmm_ext_jac_step_f32 (csrc/ext_jac.hip), host side only:
the symbols, the argument checks that come before any device work, the workspace / split routing
of kind DICP_WS_ODE_EXT_JAC, the binding's refusal of host tensors -- and the float64 pin of the
closed forms of tests/jac_ref.py (which the GPU tests compare the kernels with) against autograd
through the oracle's Shoot."""
import ctypes as C
import os

import pytest
import torch

import jac_ref as J
from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "diff-icp_amd", "libdifficp_hip.so")
WS_ODE_EXT_JAC = 14
JAC = "dicp_lddmm_ode_ext_jac_f32"
STEP = "dicp_lddmm_ext_jac_step_f32"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built (run __graft_entry__.build())")
    h = C.CDLL(LIB)
    h.dicp_last_error.restype = C.c_char_p
    h.dicp_workspace_bytes.restype = C.c_size_t
    h.dicp_workspace_bytes.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int]
    h.dicp_num_splits.argtypes = [C.c_int, C.c_int64, C.c_int64]
    getattr(h, JAC).argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_double,
                                C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    getattr(h, STEP).argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                 C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_size_t, C.c_void_p]
    return h


def _jac(lib, N, M, D, sigma=0.5):
    return getattr(lib, JAC)(None, N, None, None, M, D, sigma, 0.0, None, None, None, 0, None)


def _step(lib, N, M, D, sigma=0.5):
    return getattr(lib, STEP)(None, None, N, None, None, M, D, sigma, 0.0, 0.1, None, None, None, 0, None)


def test_symbols_exported_and_bound(lib):
    from difficp_amd import _lib
    for name in (JAC, STEP):
        assert hasattr(lib, name)
        assert name in _lib.EXPORTED_SYMBOLS and name in _lib._SIGNATURES
    assert _lib.WS_ODE_EXT_JAC == WS_ODE_EXT_JAC


@pytest.mark.parametrize("call", [_jac, _step])
def test_invalid_arguments(lib, call):
    assert call(lib, 5, 5, 3) == 1                      # NULL pointers
    assert b"invalid" in lib.dicp_last_error()
    assert call(lib, -1, 5, 3) == 1                     # negative sizes
    assert b"invalid" in lib.dicp_last_error()
    assert call(lib, 5, -1, 2) == 1
    assert call(lib, 5, 5, 3, sigma=0.0) == 1
    assert b"invalid" in lib.dicp_last_error()


@pytest.mark.parametrize("call", [_jac, _step])
def test_unsupported_dimension(lib, call):
    assert call(lib, 5, 5, 7) == 2
    assert b"unsupported" in lib.dicp_last_error()


@pytest.mark.parametrize("call", [_jac, _step])
def test_empty_calls_are_ok(lib, call):
    """No carried points: nothing to do, whatever the support (M = 0 with carried points writes
    its outputs on the device: tests/test_gpu_ext_jac.py)."""
    assert call(lib, 0, 5, 3) == 0
    assert call(lib, 0, 0, 2) == 0


def test_workspace_kind_routed(lib):
    """Wherever the pass is split over column chunks, the (vx | A) partial slabs need a workspace
    that covers the split count dicp_num_splits reports (M = support points, N = carried points)."""
    split = 0
    for M, N in [(1, 1), (300, 7), (129, 513), (2000, 3000), (700, 20000), (20000, 700), (100000, 100000)]:
        S = lib.dicp_num_splits(WS_ODE_EXT_JAC, M, N)
        assert S >= 1
        for D in (2, 3):
            b = lib.dicp_workspace_bytes(WS_ODE_EXT_JAC, M, N, D)
            if S > 1:
                split += 1
                assert b > 0 and b >= S * N * (D + D * D) * 4
            else:
                assert b == 0
    assert split > 0
    assert lib.dicp_workspace_bytes(WS_ODE_EXT_JAC, 20000, 700, 3) > 0
    assert lib.dicp_workspace_bytes(WS_ODE_EXT_JAC, 20000, 700, 2) > 0
    assert lib.dicp_workspace_bytes(WS_ODE_EXT_JAC, 20000, 700, 7) == 0
    assert lib.dicp_num_splits(WS_ODE_EXT_JAC, 5000, 0) == 1


def test_no_cpu_fallback():
    from difficp_amd import _lib
    x = torch.rand(4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.ode_ext_jac(x, x, x, 0.5, 0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.ext_jac_step(x, None, x, x, 0.5, 0.0, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.ext_jac_step(x, torch.zeros(4, 3, 3), x, x, 0.5, 1e-3, 0.1)


# ---------------------------------------------------------------------------------------
# float64: the closed form of A and both recurrences against autograd through the oracle
# ---------------------------------------------------------------------------------------
def _model(D, eta_on, scheme, nt):
    from oracle import torch_ref as R
    return R.LDDMM(0.2, D, 300.0, eta_on, True, scheme=scheme, nt=nt)


def _points(D, seed, N=40, M=30):
    g = torch.Generator().manual_seed(seed)
    q = torch.rand(M, D, generator=g, dtype=torch.float64)
    p = 0.05 * torch.randn(M, D, generator=g, dtype=torch.float64)
    x = torch.rand(N, D, generator=g, dtype=torch.float64)
    return q, p, x


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("eta_on", [False, True])
def test_closed_form_velocity_gradient(D, eta_on):
    """A = dv/dx of the oracle's v by autograd; its trace is minus the divergence rows whose sum
    is the oracle's mdivsum."""
    ref = _model(D, eta_on, "Euler", 1)
    q, p, x = _points(D, 11 + D)
    v, A = J.vel_grad(x, q, p, ref.sigma, ref.eta)
    xr = x.clone().requires_grad_(True)
    vr = ref.v(xr, q, p)
    Ar = torch.stack([torch.autograd.grad(vr[:, d].sum(), xr, retain_graph=True)[0] for d in range(D)], 1)
    assert rel_err(v, vr) < 1e-12
    assert rel_err(A, Ar) < 1e-12
    tr = A.diagonal(dim1=1, dim2=2).sum()
    assert abs(float(tr + ref.mdivsum(x, q, p))) < 1e-12 * float(A.norm())


@pytest.mark.parametrize("scheme", ["Euler", "Ralston"])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("eta_on", [False, True])
def test_recurrences_against_oracle_autograd(scheme, D, eta_on):
    ref = _model(D, eta_on, scheme, 5)
    q, p, x = _points(D, 23 + D)
    x1, G = J.flow(ref, q, p, x)
    x1r, Gr = J.oracle_flow(ref, q, p, x)
    assert float(Gr.norm()) > 1e-2                      # a deformation, not the identity
    assert rel_err(x1, x1r) < 1e-12
    assert rel_err(G, Gr) < 1e-12


def test_euler_step_is_the_flow():
    """step() chained over the oracle's support states is flow() (the GPU step test uses it)."""
    ref = _model(3, True, "Euler", 4)
    q, p, x = _points(3, 31)
    sh = ref.Shoot(q, p)
    xs, G = x, None
    for t in range(ref.nt):
        xs, G = J.step(xs, G, sh[t][0], sh[t][1], ref.sigma, ref.eta, 1.0 / ref.nt)
    x1, Gf = J.flow(ref, q, p, x)
    assert rel_err(xs, x1) < 1e-14 and rel_err(G, Gf) < 1e-13
