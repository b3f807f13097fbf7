"""dicp_gmm_carry_f32 (csrc/carry.hip), host side only: the symbol, the argument checks that come
before any device work, the workspace / split routing of kind DICP_WS_GMM_CARRY, the binding's
refusal of host tensors; the tolerances of tests/carry_ref.py against a float32 restatement of
the kernel's arithmetic; and the Python layers (GaussianMixtureUnif.carry_to_points /
pool_from_points, MultiPSR.carry_to_frame / pool_to_template) over a monkeypatched
_lib.gmm_carry / _lib.gmm_estep served by carry_ref and tests/fake_hip.py, against dense float64
softmax statements written out here."""
import ctypes as C
import math
import os

import pytest
import torch

import carry_ref as CR
import fake_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "diff-icp_amd", "libdifficp_hip.so")
WS_GMM_CARRY = 16
NEG_INF = float("-inf")


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


def _carry(lib, M, N, F, D, ptrs=(None,) * 5):
    """ptrs: rows, cols, bias, feat, out (lse2 and the workspace stay NULL)."""
    f = lib.dicp_gmm_carry_f32
    f.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                  C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    rows, cols, bias, feat, out = ptrs
    return f(rows, M, cols, bias, feat, N, F, D, 0.5, out, None, None, 0, None)


def test_symbol_exported_and_bound(lib):
    from difficp_amd import _lib
    assert hasattr(lib, "dicp_gmm_carry_f32")
    assert "dicp_gmm_carry_f32" in _lib.EXPORTED_SYMBOLS
    assert _lib.WS_GMM_CARRY == WS_GMM_CARRY
    assert "gmm_carry" in _lib.FLOPS_PER_PAIR
    with open(os.path.join(ROOT, "include", "difficp_hip.h")) as fh:
        header = fh.read()
    assert "dicp_gmm_carry_f32" in header and "DICP_WS_GMM_CARRY = 16" in header


@pytest.mark.parametrize("D,F", [(1, 1), (4, 1), (7, 3), (3, 0), (2, -1)])
def test_unsupported_shapes_are_invalid(lib, D, F):
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert _carry(lib, 5, 5, F, D, (p, p, p, p, p)) == 1      # valid pointers: the shape is refused
    assert b"invalid" in lib.dicp_last_error()


def test_null_pointers_are_invalid(lib):
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    # rows, cols, feat, out in turn (a null bias reads as 0, lse2 is optional): none of these
    # calls reaches the device
    for ptrs in [(None, p, p, p, p), (p, None, p, p, p), (p, p, p, None, p), (p, p, p, p, None)]:
        assert _carry(lib, 5, 5, 2, 3, ptrs) == 1
        assert b"invalid" in lib.dicp_last_error()


def test_no_rows_is_ok(lib):
    assert _carry(lib, 0, 5, 1, 3) == 0
    assert _carry(lib, 0, 0, 40, 2) == 0


def test_workspace_kind_routed(lib):
    """Wherever the pass is split over column chunks, the partials (m, l, acc[16]) of every row and
    chunk need a workspace; its size has no channel argument."""
    split = 0
    for M, N in [(256, 256), (256, 257), (256, 5000), (1000, 5000), (100000, 100000), (512, 640000)]:
        S = lib.dicp_num_splits(WS_GMM_CARRY, M, N)
        assert S >= 1
        for D in (2, 3):
            b = lib.dicp_workspace_bytes(WS_GMM_CARRY, M, N, D)
            if S > 1:
                split += 1
                assert b >= S * M * 18 * 4
            else:
                assert b == 0
    assert split > 0
    assert lib.dicp_workspace_bytes(WS_GMM_CARRY, 1000, 5000, 7) == 0
    assert lib.dicp_num_splits(WS_GMM_CARRY, 0, 5000) == 1


def test_no_cpu_fallback():
    from difficp_amd import _lib
    x = torch.rand(4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.gmm_carry(x, x, None, torch.rand(4, 2), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.gmm_carry(x, x, torch.zeros(4), torch.rand(4, 1), 0.5)


# ---------------------------------------------------------------------------------------
# the tolerances, against the kernel's arithmetic restated in float32
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset,sigma,bscale", [(0.0, 0.1, 2.0), (100.0, 0.02, 100.0), (0.0, 0.02, 100.0)])
def test_restatement_meets_the_tolerances(offset, sigma, bscale):
    """carry_ref.restate32 (integer reference, tile-wise sums, two chunks) lies within the float64
    reference's tolerances on the GPU tests' input families; a column of weight 1e-3 dropped
    does not."""
    g = torch.Generator().manual_seed(int(offset) + int(bscale))
    M, N, F, D = 130, 1300, 5, 3
    rows = torch.rand(M, D, generator=g) + offset
    cols = torch.rand(N, D, generator=g) + offset
    bias = bscale * torch.randn(N, generator=g)
    bias[N // 2] = NEG_INF
    feat = torch.randn(N, F, generator=g)
    feat[N // 2] = float("nan")
    ref = CR.carry_ref(rows, cols, bias, feat, sigma)
    out, lse2 = CR.restate32(rows, cols, bias, feat, sigma, chunks=2)
    CR.check(out, lse2, ref, f"restatement offset {offset} sigma {sigma} bias x{bscale}")


def test_tolerance_catches_a_dropped_column():
    g = torch.Generator().manual_seed(9)
    rows, cols = torch.rand(64, 3, generator=g), torch.rand(300, 3, generator=g)
    bias, feat = 2.0 * torch.randn(300, generator=g), torch.randn(300, 3, generator=g)
    ref = CR.carry_ref(rows, cols, bias, feat, 0.1)
    # per row the heaviest column whose weight is below 1e-3 is dropped: far outside
    p = torch.where(ref.p < 1e-3, ref.p, torch.zeros_like(ref.p))
    j = p.argmax(1)
    w = p.gather(1, j[:, None])[:, 0]
    out = (ref.out - w[:, None] * feat.double()[j]) / (1 - w)[:, None]
    lse = ref.lse + torch.log2(1 - w)
    big = w > 1e-4
    assert bool(big.any())
    assert bool((((out - ref.out).abs() / ref.tol_out).max(1).values[big] > 1).all())
    assert bool((((lse - ref.lse).abs() / ref.tol_lse)[big] > 1).all())


# ---------------------------------------------------------------------------------------
# the Python layers over a served kernel
# ---------------------------------------------------------------------------------------
def _served_carry(calls):
    def gmm_carry(rows, cols, bias, feat, sigma):
        assert rows.dtype == torch.float32 and feat.dtype == torch.float32 and feat.dim() == 2
        assert rows.is_contiguous() and cols.is_contiguous() and feat.is_contiguous()
        assert bias is None or (bias.shape == (cols.shape[0],) and bias.is_contiguous())
        calls.append((tuple(rows.shape), tuple(cols.shape), tuple(feat.shape)))
        ref = CR.carry_ref(rows, cols, bias, feat, sigma)
        return ref.out.float(), ref.lse.float()
    return gmm_carry


@pytest.fixture
def served(monkeypatch):
    from difficp_amd import _lib
    fake_hip.install(monkeypatch)
    calls = []
    monkeypatch.setattr(_lib, "gmm_carry", _served_carry(calls))
    return calls


CPU = {"device": "cpu", "dtype": torch.float32}


def _mixture(D, outliers, C=12, N=150, dead=None):
    from difficp_amd.core.GMM import GaussianMixtureUnif
    g = torch.Generator().manual_seed(40 + D)
    X = torch.rand(N, D, generator=g)
    mu = torch.rand(C, D, generator=g)
    G = GaussianMixtureUnif(mu, sigma=0.15, use_outliers=outliers, spec=CPU)
    w = torch.randn(C, generator=g)
    if dead is not None:
        w[dead] = NEG_INF
    G.w = w
    if outliers:
        G.outliers["eta0"] = -0.5
    return G, X, g


def _dense(G, X):
    """float64: r (N, C) normalised over the components, gamma0 (N,) the outlier posterior."""
    x, mu, w = X.double(), G.mu.double(), G.w.double()
    t = (w - w.logsumexp(0))[None, :] - ((x[:, None, :] - mu[None, :, :]) ** 2).sum(-1) / (2 * G.sigma ** 2)
    r = torch.softmax(t, 1)
    g0 = torch.zeros(x.shape[0], dtype=torch.float64)
    if G.outliers is not None:
        T = t.logsumexp(1) - G.D * (math.log(G.sigma) + 0.5 * math.log(2 * math.pi))
        eta = G.outliers["eta0"] - math.log(G.outliers["vol0"]) - T
        g0 = torch.sigmoid(eta)
    return r, g0


@pytest.mark.parametrize("outliers", [False, True])
@pytest.mark.parametrize("D", [2, 3])
def test_carry_to_points_layer(served, D, outliers):
    from difficp_amd.core.GMM import Carried
    G, X, g = _mixture(D, outliers, dead=4)
    vals = torch.randn(G.C, 3, generator=g)
    vals[4] = float("nan")                            # a dead component's values are never read
    if outliers:
        with pytest.raises(ValueError, match="vol0"):
            G.carry_to_points(X, vals)
        G.set_vol0(X)
    state = (G.mu.clone(), G.w.clone(), G.sigma)
    r, g0 = _dense(G, X)
    want = r @ torch.nan_to_num(vals.double())
    c = G.carry_to_points(X.clone().requires_grad_(True), vals)
    assert isinstance(c, Carried) and c.values.shape == (150, 3) and c.values.dtype == torch.float32
    assert not c.values.requires_grad
    assert float((c.values.double() - want).abs().max()) < 1e-5
    assert served == [((150, D), (G.C, D), (G.C, 3))]          # one pass, no E-step pass of its own
    if outliers:
        assert float((c.log_outlier.double().exp() - g0).abs().max()) < 1e-5
    else:
        assert c.log_outlier is None
    # (C,) in, (N,) out: the first channel
    c1 = G.carry_to_points(X, vals[:, 0].double())             # any dtype is taken to the spec
    assert c1.values.shape == (150,)
    assert torch.equal(c1.values, c.values[:, 0])
    # one-hot labels: rows sum to 1
    lab = torch.eye(G.C)
    assert float((G.carry_to_points(X, lab).values.sum(1) - 1).abs().max()) < 1e-5
    for bad in (torch.zeros(G.C + 1), torch.zeros(G.C, 0), torch.zeros(G.C, 2, 2)):
        with pytest.raises(ValueError):
            G.carry_to_points(X, bad)
    assert torch.equal(G.mu, state[0]) and torch.equal(G.w, state[1]) and G.sigma == state[2]


@pytest.mark.parametrize("outliers", [False, True])
@pytest.mark.parametrize("D", [2, 3])
def test_pool_from_points_layer(served, D, outliers):
    from difficp_amd.core.GMM import Pooled
    G, X, g = _mixture(D, outliers, dead=7)
    N = X.shape[0]
    vals = torch.randn(N, 2, generator=g)
    wts = torch.rand(N, generator=g)
    wts[:5] = 0.0
    if outliers:
        with pytest.raises(ValueError, match="vol0"):
            G.pool_from_points(X, vals)
        G.set_vol0(X)
    r, g0 = _dense(G, X)
    live = torch.ones(G.C, dtype=torch.bool)
    live[7] = False
    for w in (None, wts):
        gam = r * (1 - g0)[:, None] * (1.0 if w is None else w.double()[:, None])
        mass = gam.sum(0)
        want = gam.t() @ vals.double() / mass[:, None]
        p = G.pool_from_points(X, vals, weights=w)
        assert isinstance(p, Pooled) and p.values.shape == (G.C, 2) and p.mass.shape == (G.C,)
        assert float((p.values.double() - want)[live].abs().max()) < 2e-5
        assert float(((p.mass.double() - mass) / mass)[live].abs().max()) < 2e-5
        # the dead component: NaN values, mass 0
        assert bool(torch.isnan(p.values[7]).all()) and float(p.mass[7]) == 0.0
        assert served[-1] == ((G.C, D), (N, D), (N, 2))        # rows are the components
        p1 = G.pool_from_points(X, vals[:, 1], weights=w)
        assert p1.values.shape == (G.C,)
        assert torch.equal(p1.values[live], p.values[live, 1]) and torch.equal(p1.mass, p.mass)
    # the outlier discount is there: without it the mass would be the plain responsibility sum
    if outliers:
        assert float((r.sum(0) - G.pool_from_points(X, vals).mass.double())[live].min()) > 1e-3
    # all weights zero: nothing has mass
    p = G.pool_from_points(X, vals, weights=torch.zeros(N))
    assert bool(torch.isnan(p.values).all()) and bool((p.mass == 0).all())
    # a constant field pools to itself
    p = G.pool_from_points(X, torch.full((N,), 2.5))
    assert float((p.values[live] - 2.5).abs().max()) < 1e-5
    for bad in (torch.zeros(N + 1), torch.zeros(N, 0)):
        with pytest.raises(ValueError):
            G.pool_from_points(X, bad)
    with pytest.raises(ValueError):
        G.pool_from_points(X, vals, weights=torch.ones(N + 1))


def test_multipsr_layer(served):
    """3 frames x 2 structures: carry_to_frame is carry_to_points on x1[k, s]; pool_to_template
    combines the frames' pools by mass in float64, a frame of zero weights drops out."""
    from difficp_amd.core.GMM import GaussianMixtureUnif
    from difficp_amd.core.PSR import MultiPSR
    g = torch.Generator().manual_seed(3)
    K, S, D = 3, 2, 2
    x = [[torch.rand(30 + 10 * k + 5 * s, D, generator=g) for s in range(S)] for k in range(K)]
    GMMi = [GaussianMixtureUnif(torch.rand(6 + s, D, generator=g), sigma=0.2, use_outliers=(s == 1), spec=CPU)
            for s in range(S)]
    PS = MultiPSR(x, GMMi, dataspec=CPU, compspec=CPU)
    PS.printstuff = False
    PS.GMM_opt(max_iterations=2)
    state = [(gm.mu.clone(), gm.w.clone(), gm.sigma) for gm in PS.GMMi]
    for s in range(S):
        gm = PS.GMMi[s]
        tv = torch.randn(gm.C, 2, generator=g)
        for k in range(K):
            a = PS.carry_to_frame(tv, k=k, s=s)
            b = gm.carry_to_points(PS.x1[k, s], tv)
            assert torch.equal(a.values, b.values) and a.values.shape == (PS.N[k, s], 2)
            assert (a.log_outlier is None) == (s == 0)
        vals = [torch.randn(int(PS.N[k, s]), generator=g) for k in range(K)]
        wts = [None, torch.zeros(int(PS.N[1, s])), torch.rand(int(PS.N[2, s]), generator=g)]
        num = torch.zeros(gm.C, dtype=torch.float64)
        den = torch.zeros(gm.C, dtype=torch.float64)
        for k in (0, 2):                                     # frame 1 has no mass
            r, g0 = _dense(gm, PS.x1[k, s])
            gam = r * (1 - g0)[:, None] * (1.0 if wts[k] is None else wts[k].double()[:, None])
            num += gam.t() @ vals[k].double()
            den += gam.sum(0)
        p = PS.pool_to_template(vals, s=s, weights=wts)
        assert p.values.shape == (gm.C,) and p.mass.shape == (gm.C,) and p.values.dtype == torch.float32
        assert float(((p.mass.double() - den) / den).abs().max()) < 2e-5
        assert float((p.values.double() - num / den).abs().max()) < 2e-5
        # a dict by frame, (N, F) values
        pd = PS.pool_to_template({k: vals[k][:, None] for k in range(K)}, s=s, weights=wts)
        assert pd.values.shape == (gm.C, 1) and torch.equal(pd.values[:, 0], p.values)
        # no weights: every frame counts
        assert bool((PS.pool_to_template(vals, s=s).mass > p.mass).all())
        with pytest.raises(ValueError):
            PS.pool_to_template([vals[0], vals[1][:, None], vals[2]], s=s)
    for gm, (mu, w, sigma) in zip(PS.GMMi, state):
        assert torch.equal(gm.mu, mu) and torch.equal(gm.w, w) and gm.sigma == sigma
