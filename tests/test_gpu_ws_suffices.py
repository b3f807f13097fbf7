"""The workspace that dicp_workspace_bytes reports suffices for every kernel variant the
dispatch of csrc/lddmm.hip can pick: each call runs once with a workspace of exactly that
size (a guard band behind it must stay untouched) and once with twice the size pre-filled
with NaN; both return DICP_OK and their outputs are bitwise equal.  M = 700 is ragged and
more than one row block at 2 and at 4 rows per thread; force_splits 3 makes every pass use
slabs.  A workspace that is too small makes the library return an error before any launch.
"""
import ctypes
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

M, N_EXT, SIG, DT = 700, 333, 0.25, 0.1
ROW0, NROWS, GUARD = 129, 300, 4096
WS_SELF_FWD, WS_SELF_BWD, WS_EXT_FWD, WS_EXT_BWD, WS_FWD_ROWS, WS_BWD_PART, WS_FWD_PHASED = 1, 2, 3, 4, 9, 10, 12


@pytest.fixture(scope="module")
def L():
    from difficp_amd import _lib
    return _lib


@pytest.fixture()
def forced_splits(L):
    old = L.get_option("force_splits")
    L.set_option("force_splits", 3)
    yield
    L.set_option("force_splits", old)


@pytest.fixture(scope="module")
def clouds(dev):
    """{D: (q, p, x, three (M, D) cotangent-like arrays, gdiv)}, made once and never changed."""
    g = torch.Generator().manual_seed(7)
    out = {}
    for D in (2, 3):
        r = lambda n, s=1.0: (s * torch.randn(n, D, generator=g)).float().to(dev)
        out[D] = (torch.rand(M, D, generator=g).float().to(dev), r(M, 0.1), torch.rand(N_EXT, D, generator=g).float().to(dev),
                  (r(M), r(M), r(M)), torch.ones(1, device=dev))
    return out


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def twice(L, dev, kind, m, n, D, outs, call):
    """call(ws_ptr, ws_bytes) -> rc, with outs() -> fresh output tensors made before each run."""
    nbytes = int(L.lib().dicp_workspace_bytes(kind, m, n, D))
    results = []
    for exact in (True, False):
        if exact:
            buf = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
            size = nbytes
        else:
            buf = torch.full((max(2 * nbytes, 8) // 4,), float("nan"), dtype=torch.float32, device=dev)
            size = 2 * nbytes
        o = outs()
        rc = call(o, ptr(buf), size)
        assert rc == 0, (rc, L.lib().dicp_last_error())
        if exact:
            assert bool((buf[nbytes:] == 0xA5).all()), "wrote behind the reported workspace"
        results.append(o)
    for a, b in zip(*results):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b)   # (NaN read from the workspace would compare unequal)


def fwd_cases():
    """(eta, want mG, want div, want zs, raw)"""
    for eta, mg, div, zs, raw in itertools.product((0.0, 0.02), (True, False), (True, False), (False, True), (0, 1)):
        if not (zs and eta != 0.0):
            yield eta, mg, div, zs, raw


@pytest.mark.parametrize("fwd_alg", [0, 2, 3, 5, 6])
@pytest.mark.parametrize("D", [2, 3])
def test_forward_workspace_suffices(L, dev, clouds, forced_splits, D, fwd_alg):
    q, p = clouds[D][:2]
    q_loc, p_loc = q[ROW0:ROW0 + NROWS].contiguous(), p[ROW0:ROW0 + NROWS].contiguous()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = L.lib()
    packed = fwd_alg in (2, 5, 6)
    old = L.get_option("fwd_alg")
    L.set_option("fwd_alg", fwd_alg)
    try:
        for eta, mg, div, zs, raw in fwd_cases():
            if zs and mg and not packed:
                continue   # refused by the library: the divergence rows come from the packed passes
            with L.coord_mode(bool(raw)):
                for row0, n, kind in ((0, M, WS_SELF_FWD), (ROW0, NROWS, WS_FWD_ROWS)):
                    def outs(n=n):
                        z = lambda *s: torch.zeros(*s, device=dev)
                        return (z(n, D), z(n, D) if mg else None, z(n) if div else None, z(n, D) if zs else None)

                    def step(o, ws, size, row0=row0, n=n):
                        return lib.dicp_lddmm_euler_step_zs_f32(ptr(q), ptr(p), M, row0, n, D, SIG, eta, DT, None,
                                                                ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), ws, size, st)

                    twice(L, dev, kind, n, M, D, outs, step)
                if packed:   # the two-phase step of the same slice
                    def phases(o, ws, size):
                        for phase in (0, 1):
                            rc = lib.dicp_lddmm_euler_step_phase_f32(phase, ptr(q_loc), ptr(p_loc), ptr(q), ptr(p), M, ROW0,
                                                                     NROWS, D, SIG, eta, DT, ptr(o[0]), ptr(o[1]),
                                                                     ptr(o[2]), ptr(o[3]), ws, size, st)
                            if rc:
                                return rc
                        return 0

                    twice(L, dev, WS_FWD_PHASED, NROWS, M, D, outs, phases)
    finally:
        L.set_option("fwd_alg", old)
    torch.cuda.synchronize()


@pytest.mark.parametrize("D", [2, 3])
def test_vjp_workspace_suffices(L, dev, clouds, forced_splits, D):
    q, p, _, (gv, gmG, zrows), gdiv = clouds[D]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = L.lib()
    outs = lambda: (torch.zeros(M, D, device=dev), torch.zeros(M, D, device=dev))
    for eta, mg, div, zs, raw in fwd_cases():
        b, gd = (gmG if mg else None), (gdiv if div else None)
        z = zrows[ROW0:ROW0 + NROWS].contiguous() if zs else None
        with L.coord_mode(bool(raw)):
            if not zs:
                twice(L, dev, WS_SELF_BWD, M, M, D, outs, lambda o, ws, size: lib.dicp_lddmm_ode_self_bwd_f32(
                    ptr(q), ptr(p), ptr(gv), ptr(b), ptr(gd), M, D, SIG, eta, ptr(o[0]), ptr(o[1]), ws, size, st))
            for nparts in (1, 3):
                for part in range(nparts):
                    twice(L, dev, WS_BWD_PART, M, nparts, D, outs,
                          lambda o, ws, size: lib.dicp_lddmm_ode_self_bwd_part_zs_f32(
                              ptr(q), ptr(p), ptr(gv), ptr(b), ptr(gd), M, D, SIG, eta, part, nparts, ptr(z), ROW0,
                              NROWS, ptr(o[0]), ptr(o[1]), ws, size, st))
    torch.cuda.synchronize()


@pytest.mark.parametrize("D", [2, 3])
def test_external_points_workspace_suffices(L, dev, clouds, forced_splits, D):
    q, p, x, (gv, _, _), gdiv = clouds[D]
    gvx = gv[:N_EXT].contiguous()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = L.lib()
    z = lambda *s: torch.zeros(*s, device=dev)
    for eta, div in itertools.product((0.0, 0.02), (True, False)):
        twice(L, dev, WS_EXT_FWD, M, N_EXT, D, lambda: (z(N_EXT, D), z(N_EXT) if div else None),
              lambda o, ws, size: lib.dicp_lddmm_ode_ext_fwd_f32(ptr(x), N_EXT, ptr(q), ptr(p), M, D, SIG, eta, ptr(o[0]),
                                                                 ptr(o[1]), ws, size, st))
        twice(L, dev, WS_EXT_BWD, M, N_EXT, D, lambda: (z(N_EXT, D), z(M, D), z(M, D)),   # gq, gp accumulate
              lambda o, ws, size: lib.dicp_lddmm_ode_ext_bwd_f32(ptr(x), N_EXT, ptr(q), ptr(p), M, D, SIG, eta, ptr(gvx),
                                                                 ptr(gdiv if div else None), ptr(o[0]), ptr(o[1]),
                                                                 ptr(o[2]), ws, size, st))
    torch.cuda.synchronize()
