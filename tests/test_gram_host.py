"""dicp_rkhs_gram_f32 (csrc/gram.hip) and the tangent-space statistics above it, host side only:
the symbol, the argument checks that come before any device work, the workspace / split routing of
kind DICP_WS_RKHS_GRAM, the binding's refusal of host tensors; the constant C of tests/gram_ref.py
against the float32 restatement of the kernel's arithmetic; and the Python layers
(LDDMMModel.field_gram, core/statistics.py TangentPCA, the tangent_pca entry points) over a
monkeypatched _lib.rkhs_gram served by gram_ref's dense float64 statement."""
import ctypes as C
import math
import os

import pytest
import torch

import gram_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "diff-icp_amd", "libdifficp_hip.so")
WS_RKHS_GRAM = 17


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built (run __graft_entry__.build())")
    h = C.CDLL(LIB)
    h.dicp_last_error.restype = C.c_char_p
    h.dicp_workspace_bytes.restype = C.c_size_t
    h.dicp_workspace_bytes.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int]
    h.dicp_num_splits.argtypes = [C.c_int, C.c_int64, C.c_int64]
    h.dicp_rkhs_gram_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p,
                                     C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_void_p]
    return h


def _gram(lib, F=2, max_rows=5, npairs=3, D=3, ptrs=None, ws_bytes=1 << 20):
    """ptrs: q, p, offsets, pairs, out, ws."""
    q, p, off, pr, out, ws = ptrs if ptrs is not None else (None,) * 6
    return lib.dicp_rkhs_gram_f32(q, p, off, F, max_rows, pr, npairs, D, 0.5, out, ws, ws_bytes, None)


@pytest.fixture()
def ptr():
    buf = (C.c_double * 64)()
    yield C.addressof(buf)
    del buf


def test_symbol_exported_bound_and_declared(lib):
    from difficp_amd import _lib
    assert hasattr(lib, "dicp_rkhs_gram_f32")
    assert "dicp_rkhs_gram_f32" in _lib.EXPORTED_SYMBOLS
    assert _lib.WS_RKHS_GRAM == WS_RKHS_GRAM
    assert "rkhs_gram" in _lib.FLOPS_PER_PAIR
    with open(os.path.join(ROOT, "include", "difficp_hip.h")) as fh:
        header = fh.read()
    assert "dicp_rkhs_gram_f32" in header and "DICP_WS_RKHS_GRAM = 17" in header


@pytest.mark.parametrize("D", [1, 4, 7])
def test_unsupported_dimension_is_invalid(lib, ptr, D):
    assert _gram(lib, D=D, ptrs=(ptr,) * 6) == 1       # valid pointers: the dimension is refused
    assert b"invalid" in lib.dicp_last_error()


@pytest.mark.parametrize("kw", [dict(F=-1), dict(npairs=-1), dict(max_rows=-1)])
def test_negative_sizes_are_invalid(lib, ptr, kw):
    assert _gram(lib, ptrs=(ptr,) * 6, **kw) == 1
    assert b"invalid" in lib.dicp_last_error()


@pytest.mark.parametrize("which", range(6))
def test_null_pointers_are_invalid(lib, ptr, which):
    """q, p, offsets, pairs, out and the workspace in turn: none of these calls reaches the device."""
    ptrs = [ptr] * 6
    ptrs[which] = None
    assert _gram(lib, ptrs=tuple(ptrs)) == 1
    assert b"invalid" in lib.dicp_last_error()


def test_no_pairs_is_ok_without_pointers(lib):
    assert _gram(lib, npairs=0) == 0
    assert _gram(lib, F=0, max_rows=0, npairs=0, D=2) == 0


def test_workspace_kind_routed(lib):
    """One double per (pair, row block, column chunk): the bytes grow with the pairs and cover the
    partials of dicp_num_splits column chunks of every row block; the chunk count depends on
    max_rows alone (the geometry of a pair must not depend on the other pairs of the call)."""
    for D in (2, 3):
        for M in (1, 512, 513, GR.CHUNK, GR.CHUNK + 1, 20000):
            prev = 0
            for n in (1, 2, 55, 528):
                b = lib.dicp_workspace_bytes(WS_RKHS_GRAM, M, n, D)
                S = lib.dicp_num_splits(WS_RKHS_GRAM, M, n)
                assert S == max(1, math.ceil(M / GR.CHUNK)) == lib.dicp_num_splits(WS_RKHS_GRAM, M, 1)
                assert b >= n * math.ceil(M / GR.ROWS) * S * 8
                assert b >= prev                 # in 256-byte granules
                prev = b
            assert prev > lib.dicp_workspace_bytes(WS_RKHS_GRAM, M, 1, D)
    assert lib.dicp_num_splits(WS_RKHS_GRAM, GR.SPLIT_SIZE - 1, 1) == 1
    assert lib.dicp_num_splits(WS_RKHS_GRAM, GR.SPLIT_SIZE, 1) == 2
    assert lib.dicp_workspace_bytes(WS_RKHS_GRAM, 0, 5, 3) == 0
    assert lib.dicp_workspace_bytes(WS_RKHS_GRAM, 100, 5, 4) == 0


def test_workspace_too_small_is_refused(lib, ptr):
    assert _gram(lib, ptrs=(ptr,) * 6, ws_bytes=8) == 3       # DICP_ERR_WORKSPACE
    assert b"workspace" in lib.dicp_last_error()


def test_binding_refuses_host_tensors():
    from difficp_amd import _lib
    q = torch.rand(6, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.rkhs_gram(q, q, [0, 3, 6], [(0, 1)], 0.5)


# ---------------------------------------------------------------------------------------------
# the tolerance constant
@pytest.mark.parametrize("D,sigma", GR.CASES)
def test_restatement_within_half_the_constant(D, sigma):
    """C of gram_ref is twice the restatement's largest deviation from the float64 statement: the
    deviation, recomputed here over the kernel tests' own inputs, stays below C / 2."""
    assert GR.C >= 2 * GR.MEASURED_DEVIATION
    for _, _, shift, q, p, off, pairs in GR.test_inputs([(D, sigma)]):
        dev = GR.deviation(q, p, off, pairs, sigma)
        print(f"D {D} sigma {sigma} shift {shift} pairs {len(pairs)}: deviation {dev:.3f} x 2^-24 A")
        assert dev < GR.C / 2


def test_restatement_is_the_float32_statement():
    """The restatement is not the float64 statement in disguise: it deviates by float32 amounts."""
    q, p, off = GR.fields(3)
    pairs = GR.all_pairs(len(GR.SIZES))
    assert GR.deviation(q, p, off, pairs, 0.05) > 0.05


# ---------------------------------------------------------------------------------------------
# the Python layers over the dense float64 statement
@pytest.fixture()
def patched(monkeypatch):
    from difficp_amd import _lib
    calls = []

    def fake(q, p, offsets, pairs, sigma):
        calls.append(len(torch.as_tensor(pairs).reshape(-1, 2)))
        return GR.rkhs_gram(q, p, offsets, pairs, sigma)

    monkeypatch.setattr(_lib, "rkhs_gram", fake)
    return calls


def _model(D=2, sigma=0.3, version="classic"):
    from difficp_amd.core.LDDMM import LDDMMModel
    from difficp_amd.tools.spec import cpuspec
    return LDDMMModel(sigma=sigma, D=D, lambd=10.0, version=version, spec=cpuspec)


def _ragged(D=2, sizes=(40, 7, 0, 25, 33), seed=3):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, D, generator=g), torch.randn(n, D, generator=g)) for n in sizes]


def test_field_gram_symmetric_and_cross_block(patched):
    LM = _model()
    fields = _ragged()
    G = LM.field_gram(fields)
    assert G.dtype == torch.float64 and G.shape == (5, 5)
    assert patched == [15]                                   # one call, the upper triangle only
    assert torch.equal(G, G.t())
    off = [0]
    for q, _ in fields:
        off.append(off[-1] + q.shape[0])
    q, p = torch.cat([f[0] for f in fields]), torch.cat([f[1] for f in fields])
    want = GR.rkhs_gram(q, p, off, [(a, b) for a in range(5) for b in range(5)], LM.sigma).reshape(5, 5)
    assert torch.allclose(G, want, rtol=1e-13, atol=0)
    assert bool((G[2] == 0).all())                           # the empty field
    X = LM.field_gram(fields[:2], fields[2:])
    assert patched == [15, 6] and X.shape == (2, 3)
    assert torch.equal(X, G[:2, 2:])
    # the diagonal is twice the eta = 0 Hamiltonian, written out
    q0, p0 = fields[0][0].double(), fields[0][1].double()
    K = torch.exp(-((q0[:, None] - q0[None]) ** 2).sum(-1) / (2 * LM.sigma ** 2))
    assert abs(float(G[0, 0]) - float((p0 * (K @ p0)).sum())) < 1e-12 * abs(float(G[0, 0]))


def test_field_gram_refusals(patched):
    fields = _ragged()
    with pytest.raises(ValueError, match="eta = 0"):
        _model(version="logdet").field_gram(fields)
    LM = _model()
    with pytest.raises(ValueError, match="shaped"):
        LM.field_gram(fields + [(torch.rand(4, 3), torch.rand(4, 3))])     # a 3D field, 2D model
    with pytest.raises(ValueError, match="shaped"):
        LM.field_gram([(torch.rand(4, 2), torch.rand(5, 2))])
    with pytest.raises(ValueError, match="pair"):
        LM.field_gram([torch.rand(4, 2)])
    with pytest.raises(ValueError, match="same device"):
        LM.field_gram(fields + [(torch.rand(4, 2).double(), torch.rand(4, 2).double())])
    assert patched == []


def _rank2_family(K=6, n=60, D=2, seed=5):
    """Fields on one shared support with momenta m + a_k u1 + b_k u2."""
    g = torch.Generator().manual_seed(seed)
    q = torch.rand(n, D, generator=g)
    m, u1, u2 = (torch.randn(n, D, generator=g) for _ in range(3))
    a = torch.tensor([0.5, -1.25, 2.0, 0.75, -0.5, 1.5])[:K]
    b = torch.tensor([1.0, 0.25, -0.75, -1.5, 0.5, 2.25])[:K]
    fields = [(q, m + a[k] * u1 + 0.5 * b[k] * u2) for k in range(K)]
    return q, (u1, 0.5 * u2), torch.stack([a, b], 1).double(), fields


def test_tangent_pca_rank2_family(patched):
    from difficp_amd.core.statistics import TangentPCA
    LM = _model()
    q, (u1, u2), coef, fields = _rank2_family()
    K = len(fields)
    pca = TangentPCA.fit(LM, fields)
    assert patched == [K * (K + 1) // 2]
    assert pca.L == 2 and pca.scores.shape == (K, 2) and pca.coefficients.shape == (K, 2)
    assert bool((pca.eigenvalues[:-1] >= pca.eigenvalues[1:]).all())
    H = torch.eye(K, dtype=torch.float64) - 1.0 / K
    HGH = H @ pca.gram @ H
    S = pca.scores
    assert float((S @ S.t() - HGH).norm()) <= 1e-10 * float(HGH.norm())
    # the known coefficients: H G H = Ac M Ac^T, M the Gram matrix of the two directions (the
    # float32 momenta carry the coefficients to ~1e-7)
    M = GR.rkhs_gram(torch.cat([q, q]), torch.cat([u1, u2]), [0, len(q), 2 * len(q)],
                     [(0, 0), (0, 1), (1, 0), (1, 1)], LM.sigma).reshape(2, 2)
    Ac = H @ coef
    assert float((S @ S.t() - Ac @ M @ Ac.t()).norm()) <= 1e-5 * float(HGH.norm())
    assert torch.allclose(pca.variances, pca.eigenvalues / (K - 1))
    assert abs(float(pca.explained_variance_ratio.sum()) - 1) < 1e-9
    # unit-norm, mutually orthogonal mode fields: c^T G c = I
    cg = pca.coefficients.t() @ pca.gram @ pca.coefficients
    assert float((cg - torch.eye(2, dtype=torch.float64)).abs().max()) < 1e-9
    # out-of-sample projection of a training field: its own scores, one call each
    lam0 = float(pca.eigenvalues[0])
    for k in range(K):
        n0 = len(patched)
        s = pca.project(fields[k])
        assert patched[n0:] == [K]
        assert float((s - pca.scores[k]).abs().max()) <= 1e-9 * math.sqrt(lam0)


def test_tangent_pca_distances_and_modes(patched):
    from difficp_amd.core.statistics import TangentPCA
    LM = _model()
    fields = _ragged(sizes=(40, 7, 25, 33))
    K = len(fields)
    pca = TangentPCA.fit(LM, fields)
    assert 1 <= pca.L <= K - 1
    # distances against the dense float64 norm of the difference field (q_j, p_j) + (q_k, -p_k)
    d = pca.distances()
    scale = float(pca.gram.diagonal().max())
    for j in range(K):
        for k in range(K):
            qd = torch.cat([fields[j][0], fields[k][0]])
            pd = torch.cat([fields[j][1], -fields[k][1]])
            want = float(GR.rkhs_gram(qd, pd, [0, len(qd)], [(0, 0)], LM.sigma)[0])
            assert abs(float(d[j, k]) ** 2 - max(want, 0.0)) <= 1e-9 * scale
    assert torch.equal(d, d.t()) and bool((d.diagonal() == 0).all())
    # the weights of a mode field sum to 1 for any t, and t = 0 / l = None is the mean
    for l in range(pca.L):
        for t in (-3.0, 0.0, 0.5, 2.0):
            assert abs(float(pca.mode_weights(l, t).sum()) - 1) < 1e-12
    assert torch.equal(pca.mode_weights(0, 0.0), torch.full((K,), 1.0 / K, dtype=torch.float64))
    assert torch.equal(pca.mode_weights(None, 2.0), pca.mode_weights(0, 0.0))
    with pytest.raises(IndexError):
        pca.mode_weights(pca.L, 1.0)
    # "mean + t standard deviations of mode l" lies t sqrt(variance_l) from the mean, along mode l
    qm, pm = pca.mode_field(None)
    assert qm.shape == (sum(len(f[0]) for f in fields), 2)
    for l in range(pca.L):
        t = 2.0
        ql, pl = pca.mode_field(l, t)
        assert torch.equal(ql, qm)
        n2 = float(GR.rkhs_gram(qm, pl - pm, [0, len(qm)], [(0, 0)], LM.sigma)[0])
        assert abs(n2 - t * t * float(pca.variances[l])) <= 1e-4 * t * t * float(pca.variances[l])
    reg = pca.mode_registration(0, 1.0)
    assert reg.LMi is LM and torch.equal(reg.q0, qm) and reg.a0.shape == qm.shape


def test_tangent_pca_with_an_empty_field(patched):
    from difficp_amd.core.statistics import TangentPCA
    fields = _ragged()
    assert fields[2][0].shape[0] == 0
    pca = TangentPCA.fit(_model(), fields)
    assert pca.gram.shape == (5, 5) and bool((pca.gram[2] == 0).all())
    assert pca.L >= 1 and bool(torch.isfinite(pca.scores).all())
    assert bool(torch.isfinite(pca.project(fields[2])).all())
    with pytest.raises(ValueError, match="at least 2"):
        TangentPCA.fit(_model(), fields[:1])


def test_tangent_field_source_side():
    from difficp_amd.core.registrations import LDDMMRegistration
    q, a = torch.rand(5, 2), torch.randn(5, 2).requires_grad_(True)
    reg = LDDMMRegistration(_model(), q, a)
    fq, fp = reg.tangent_field("source")
    assert torch.equal(fq, q) and torch.equal(fp, a.detach()) and not fp.requires_grad
    with pytest.raises(ValueError, match="unknown side"):
        reg.tangent_field("middle")


def test_tangent_pca_refuses_a_sharded_atlas():
    from difficp_amd.core.PSR import DiffPSR
    from difficp_amd.core.PSR_standard import DiffPSR_std
    for cls in (DiffPSR, DiffPSR_std):
        PS = object.__new__(cls)           # no fitting: only the communicator state matters
        PS.comm, PS.rank, PS.world, PS.K = True, 0, 2, 4
        with pytest.raises(ValueError, match="single process only"):
            PS.tangent_pca()
