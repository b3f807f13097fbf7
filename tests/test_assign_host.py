"""dicp_gmm_assign_f32 (csrc/assign.hip), host side only: the symbol, the argument checks that
come before any device work, the workspace / split routing of kind DICP_WS_GMM_ASSIGN and the
binding's refusal of host tensors."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "diff-icp_amd", "libdifficp_hip.so")
WS_GMM_ASSIGN = 13


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built (run __graft_entry__.build())")
    h = C.CDLL(LIB)
    h.dicp_last_error.restype = C.c_char_p
    h.dicp_workspace_bytes.restype = C.c_size_t
    h.dicp_workspace_bytes.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int]
    h.dicp_num_splits.argtypes = [C.c_int, C.c_int64, C.c_int64]
    return h


def _assign(lib, M, N, D, K):
    f = lib.dicp_gmm_assign_f32
    f.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_int,
                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    return f(None, M, None, None, N, D, 0.5, K, None, None, None, 0, None)


def test_symbol_exported_and_bound(lib):
    from difficp_amd import _lib
    assert hasattr(lib, "dicp_gmm_assign_f32")
    assert "dicp_gmm_assign_f32" in _lib.EXPORTED_SYMBOLS
    assert _lib.WS_GMM_ASSIGN == WS_GMM_ASSIGN


@pytest.mark.parametrize("D,K", [(3, 0), (3, 5), (7, 1)])
def test_unsupported_shapes_are_invalid(lib, D, K):
    assert _assign(lib, 5, 5, D, K) == 1
    assert b"invalid" in lib.dicp_last_error()


def test_null_pointers_are_invalid(lib):
    assert _assign(lib, 5, 5, 3, 1) == 1
    assert b"invalid" in lib.dicp_last_error()


def test_no_rows_is_ok(lib):
    assert _assign(lib, 0, 5, 3, 1) == 0
    assert _assign(lib, 0, 0, 2, 4) == 0


def test_workspace_kind_routed(lib):
    """Wherever the pass is split over column chunks, the partials need a workspace."""
    split = 0
    for M, N in [(256, 256), (256, 257), (256, 5000), (1000, 5000), (100000, 100000), (512, 640000)]:
        S = lib.dicp_num_splits(WS_GMM_ASSIGN, M, N)
        assert S >= 1
        for D in (2, 3):
            b = lib.dicp_workspace_bytes(WS_GMM_ASSIGN, M, N, D)
            if S > 1:
                split += 1
                assert b >= S * M * 4 * 8      # K = 4 (val, idx) pairs per row and chunk
            else:
                assert b == 0
    assert split > 0
    assert lib.dicp_workspace_bytes(WS_GMM_ASSIGN, 1000, 5000, 7) == 0
    assert lib.dicp_num_splits(WS_GMM_ASSIGN, 0, 5000) == 1


def test_no_cpu_fallback():
    import torch
    from difficp_amd import _lib
    x = torch.rand(4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.gmm_assign(x, x, None, 0.5, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.gmm_assign(x, x, torch.zeros(4), 0.5, 2)
