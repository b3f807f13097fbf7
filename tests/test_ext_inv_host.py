"""dicp_lddmm_ext_inv_step_f32 (csrc/ext_jac.hip), host side only: the symbol, the argument checks
that come before any device work, the workspace / split routing of kind DICP_WS_ODE_EXT_INV, the
binding's refusal of host tensors -- and the float64 pin of tests/inv_ref.py (which the GPU tests
compare the kernel and LDDMMModel.flow_inverse with): Newton on every step map recovers the
points the oracle's Shoot carried, where the reference's backward shooting does not."""
import ctypes as C
import functools
import os

import pytest
import torch

import inv_ref as I
from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "diff-icp_amd", "libdifficp_hip.so")
WS_ODE_EXT_JAC, WS_ODE_EXT_INV = 14, 15
INV = "dicp_lddmm_ext_inv_step_f32"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built (run __graft_entry__.build())")
    h = C.CDLL(LIB)
    h.dicp_last_error.restype = C.c_char_p
    h.dicp_workspace_bytes.restype = C.c_size_t
    h.dicp_workspace_bytes.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int]
    h.dicp_num_splits.argtypes = [C.c_int, C.c_int64, C.c_int64]
    getattr(h, INV).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                C.c_int64, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_size_t, C.c_void_p]
    return h


def _inv(lib, N, M, D, sigma=0.5, x=None, y=None, v1=None, A1=None, q=None, p=None, xn=None, res=None):
    return getattr(lib, INV)(x, y, v1, A1, N, q, p, M, D, sigma, 0.0, 0.1, xn, res, None, 0, None)


def test_symbol_exported_and_bound(lib):
    from difficp_amd import _lib
    assert hasattr(lib, INV)
    assert INV in _lib.EXPORTED_SYMBOLS and INV in _lib._SIGNATURES
    assert _lib.WS_ODE_EXT_INV == WS_ODE_EXT_INV == 15
    assert _lib.WS_ODE_EXT_JAC == WS_ODE_EXT_JAC


def test_invalid_arguments(lib):
    assert _inv(lib, 5, 5, 3) == 1                      # NULL pointers
    assert b"invalid" in lib.dicp_last_error()
    assert _inv(lib, -1, 5, 3) == 1                     # negative sizes
    assert b"invalid" in lib.dicp_last_error()
    assert _inv(lib, 5, -1, 2) == 1
    assert _inv(lib, 5, 5, 3, sigma=0.0) == 1
    assert b"invalid" in lib.dicp_last_error()


def test_unsupported_dimension(lib):
    assert _inv(lib, 5, 5, 7) == 2
    assert b"unsupported" in lib.dicp_last_error()


def test_empty_calls_are_ok(lib):
    """No carried points: nothing to do, whatever the support (M = 0 with carried points writes its
    outputs on the device: tests/test_gpu_ext_inv.py)."""
    assert _inv(lib, 0, 5, 3) == 0
    assert _inv(lib, 0, 0, 2) == 0


def test_stage_pair_and_aliasing_rejected(lib):
    """A1 without v1 (or v1 without A1), and an x_next that is x or y: refused before any device
    work -- the addresses below are never read."""
    a = dict(x=0x1000, y=0x2000, q=0x3000, p=0x4000, xn=0x5000, res=0x6000)
    assert _inv(lib, 5, 5, 3, **a, A1=0x7000) == 1
    assert b"invalid" in lib.dicp_last_error()
    assert _inv(lib, 5, 5, 3, **a, v1=0x7000) == 1
    assert b"invalid" in lib.dicp_last_error()
    assert _inv(lib, 5, 5, 2, **dict(a, xn=a["x"])) == 1
    assert b"invalid" in lib.dicp_last_error() and b"alias" in lib.dicp_last_error()
    assert _inv(lib, 5, 5, 2, **dict(a, xn=a["y"])) == 1
    assert b"invalid" in lib.dicp_last_error() and b"alias" in lib.dicp_last_error()
    assert _inv(lib, 5, 5, 2, **dict(a, y=None)) == 1
    assert _inv(lib, 5, 5, 2, **dict(a, res=None)) == 1
    assert b"invalid" in lib.dicp_last_error()


def test_workspace_kind_routed(lib):
    """The slabs of DICP_WS_ODE_EXT_JAC plus the (v | A) scratch of the N carried points; the split
    count is the velocity-gradient pass's."""
    split = 0
    for M, N in [(1, 1), (300, 7), (129, 513), (2000, 3000), (700, 20000), (20000, 700), (100000, 100000)]:
        S = lib.dicp_num_splits(WS_ODE_EXT_INV, M, N)
        assert S == lib.dicp_num_splits(WS_ODE_EXT_JAC, M, N) >= 1
        split += S > 1
        for D in (2, 3):
            b = lib.dicp_workspace_bytes(WS_ODE_EXT_INV, M, N, D)
            assert b >= lib.dicp_workspace_bytes(WS_ODE_EXT_JAC, M, N, D) + 4 * N * (D + D * D)
        assert lib.dicp_workspace_bytes(WS_ODE_EXT_INV, M, N, 7) == 0
    assert split > 0
    assert lib.dicp_workspace_bytes(WS_ODE_EXT_INV, 0, 700, 3) == 0      # no support: no pass
    assert lib.dicp_num_splits(WS_ODE_EXT_INV, 5000, 0) == 1


def test_no_cpu_fallback():
    from difficp_amd import _lib
    x = torch.rand(4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.ext_inv_step(x, x, x, x, 0.5, 0.0, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.ext_inv_step(x, x, x, x, 0.5, 1e-3, 0.1, v1=x, A1=torch.zeros(4, 3, 3))


# ---------------------------------------------------------------------------------------
# float64: Newton on the step maps inverts the oracle's Shoot; the backward shooting does not
# ---------------------------------------------------------------------------------------
def test_newton_step_solves_the_linearised_step():
    """x+ of newton_step satisfies DF (x - x+) = r, and res is |F(x) - y|_inf with F from the
    oracle's own one-step Shoot."""
    from oracle import torch_ref as R
    for D, eta_on, scheme in [(2, False, "Euler"), (3, True, "Euler"), (2, True, "Ralston"), (3, False, "Ralston")]:
        ref = R.LDDMM(I.SIG, D, I.LAM, eta_on, True, scheme=scheme, nt=1)
        x, q, p = I.case(40, 30, D, 41 + D)
        y = x + 0.01 * torch.randn(40, D, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
        q_t, p_t, qm, pm = I.support_states(ref, q, p)[0]
        if qm is None:
            v1 = A1 = None
            xn, res = I.newton_step(x, y, q_t, p_t, ref.sigma, ref.eta, 1.0)
            inc, DF = I.step_map(x, q_t, p_t, ref.sigma, ref.eta, 1.0)
        else:
            v1, A1 = I.J.vel_grad(x, q_t, p_t, ref.sigma, ref.eta)
            xn, res = I.newton_step(x, y, qm, pm, ref.sigma, ref.eta, 1.0, v1, A1)
            inc, DF = I.step_map(x, qm, pm, ref.sigma, ref.eta, 1.0, v1, A1)
        Fx = ref.Shoot(q, p, x)[-1][3]
        assert rel_err(x + inc, Fx) < 1e-13
        assert rel_err(res, (Fx - y).abs().amax(1)) < 1e-12
        assert rel_err((DF @ (x - xn)[:, :, None])[:, :, 0], Fx - y) < 1e-12
        # DF is the derivative of F: autograd through the oracle's step
        xr = x.clone().requires_grad_(True)
        Fr = ref.Shoot(q, p, xr)[-1][3]
        DFr = torch.stack([torch.autograd.grad(Fr[:, d].sum(), xr, retain_graph=True)[0] for d in range(D)], 1)
        assert rel_err(DF, DFr) < 1e-12


@functools.lru_cache(maxsize=None)
def _round_trip(D, version, scheme, scale):
    ref, x, q, p = I.flow_case(D, version, scheme, scale)
    sh = ref.Shoot(q, p, x)
    x1, q1, p1 = sh[-1][3], sh[-1][0], sh[-1][1]
    x0, info = I.inverse(ref, q, p, x1, tol=1e-13)
    xb = ref.Shoot(q1, -p1, x1)[-1][3]                  # the reference's `backward`
    return rel_err(x0, x), info, rel_err(xb, x)


@pytest.mark.parametrize("D,version,scheme,scale", I.TABLE + I.STRONG)
def test_inverse_recovers_the_carried_points(D, version, scheme, scale):
    """inv_ref.inverse of the oracle's Shoot(q, p, x)[-1][3] is x to < 1e-12 (measured <= 4e-14) in
    <= 6 updates per step (measured 3 to 4, and 5 at 3x momenta); beside it the round-trip error of
    the reference's backward shooting, which except for hybrid + Ralston is >= 1e3 times larger."""
    e, info, eb = _round_trip(D, version, scheme, scale)
    print(f"D={D} {version} {scheme} x{scale:g}: inverse {e:.1e} ({max(info['iterations'])} updates/step, "
          f"{info['passes']} passes)  backward {eb:.1e}")
    assert bool(info["converged"].all())
    assert e < 1e-12
    assert max(info["iterations"]) <= 6
    if scale == 1.0 and not (version == "hybrid" and scheme == "Ralston"):
        assert eb >= 1e3 * e
