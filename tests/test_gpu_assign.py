"""Hard / top-k correspondences: the fused biased top-K row reduction dicp_gmm_assign_f32
(csrc/assign.hip) and the interfaces built on it -- GaussianMixtureUnif.assign / nearest_points,
MultiPSR.correspondences.

The kernel returns, per row i, the K largest val_ij = bias_j - k2 |r_i - y_j|^2 (log2 domain,
k2 = log2(e) / (2 sigma^2)) in descending order, equal values by increasing column.  The
reference is the dense float64 val of the same float32 inputs, and for every row and slot:
  (a) no index is repeated within a row;
  (b) the returned val is within tol of the float64 value of the returned index;
  (c) that float64 value is >= the slot's true order statistic - tol;
with tol = 16 eps32 (|bias_j| + k2 |r_i - y_j|^2): the difference-form arithmetic makes at most
D + 5 = 8 roundings relative to that magnitude (D subtractions, D products / fmas, the rounding of
k2, the final fma, the bias as given), and the tolerance is twice that.  No rows are excluded.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS32 = float(torch.finfo(torch.float32).eps)
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
WS_GMM_ASSIGN = 13
NEG_INF = float("-inf")


def _k2(sigma):
    return LOG2E / (2.0 * sigma ** 2)


def _dense64(rows, cols, bias, sigma):
    """float64 val (M, N) and its rounding magnitude |bias| + k2 d^2, from the float32 inputs."""
    r, c = rows.double(), cols.double()
    d2 = ((r[:, None, :] - c[None, :, :]) ** 2).sum(-1) * _k2(sigma)
    b = torch.zeros(cols.shape[0], dtype=torch.float64, device=cols.device) if bias is None else bias.double()
    return b[None, :] - d2, b.abs()[None, :] + d2


def _check_topk(idx, val, val64, mag, K, extra_tol=None):
    """Criteria (a)-(c) for every row and slot.  val64 / mag: (M, N) float64, a column that may
    not be returned at -inf; extra_tol (M, 1) or None: added to tol (callers say why)."""
    M, N = val64.shape
    assert idx.shape == (M, K) and val.shape == (M, K)
    assert idx.dtype in (torch.int32, torch.int64) and val.dtype == torch.float32
    idx = idx.long()
    live = (val64 > NEG_INF).sum(1)                              # columns that may be returned
    nfill = torch.clamp(live, max=K)
    slot = torch.arange(K, device=idx.device)[None, :]
    filled = slot < nfill[:, None]
    # unfilled slots: -1 / -inf, and only those
    assert torch.equal(idx >= 0, filled), "filled slots"
    assert bool((idx[~filled] == -1).all()) and bool((val[~filled] == NEG_INF).all())
    assert bool((idx < N).all())
    # (a) no index repeated within a row
    for a in range(K):
        for b in range(a + 1, K):
            assert not bool(((idx[:, a] == idx[:, b]) & filled[:, b]).any()), "repeated index"
    # returned in descending order of the returned float32 values
    assert bool((val[:, :-1] >= val[:, 1:]).all())
    if N == 0:
        return
    g = idx.clamp(min=0)
    v64 = val64.gather(1, g)
    tol = 16 * EPS32 * mag.gather(1, g)
    if extra_tol is not None:
        tol = tol + extra_tol
    # (b) the value of the returned index
    err = (val.double() - v64).abs()
    assert bool((err[filled] <= tol[filled]).all()), float((err - tol)[filled].max())
    # (c) the slot's true order statistic
    kk = min(K, N)
    top = torch.topk(val64, kk, dim=1).values
    if kk < K:
        top = torch.cat([top, top.new_full((M, K - kk), NEG_INF)], 1)
    short = top - v64
    assert bool((short[filled] <= tol[filled]).all()), float((short - tol)[filled].max())


# ---------------------------------------------------------------------------------------
# 1. against float64
# ---------------------------------------------------------------------------------------
MS = (1, 63, 65, 257, 1000)
NS = (1, 3, 64, 65, 300, 5000)
SIGMA = 0.1
_cases = {}


def _case(dev, D, M, N):
    """Inputs and the float64 reference of one shape, made once and shared by every K."""
    key = (D, M, N)
    if key not in _cases:
        g = torch.Generator().manual_seed(1000 * D + 7 * M + N)
        rows = torch.rand(M, D, generator=g).to(dev)
        cols = torch.rand(N, D, generator=g).to(dev)
        bias = (2.0 * torch.randn(N, generator=g)).to(dev)
        if N >= 3:
            bias[N // 2] = NEG_INF                               # a dead column
        val64, mag = _dense64(rows, cols, bias, SIGMA)
        _cases[key] = (rows, cols, bias, val64, mag)
    return _cases[key]


@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("D", [2, 3])
def test_against_float64(dev, D, K):
    from difficp_amd import _lib
    for M in MS:
        for N in NS:
            rows, cols, bias, val64, mag = _case(dev, D, M, N)
            idx, val = _lib.gmm_assign(rows, cols, bias, SIGMA, K)
            assert idx.dtype == torch.int32
            _check_topk(idx, val, val64, mag, K)
            if N >= 3:
                assert not bool((idx == N // 2).any()), "dead column returned"


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("D", [2, 3])
def test_offset_cloud_and_no_bias(dev, D, K):
    """The cloud 1000 sigma from the origin (the difference form keeps the nearest-neighbour
    decision's bits), with a bias and without one (NULL reads as 0)."""
    from difficp_amd import _lib
    g = torch.Generator().manual_seed(31 + D)
    M, N = 257, 300
    off = 1000.0 * SIGMA
    rows = (torch.rand(M, D, generator=g) + off).to(dev)
    cols = (torch.rand(N, D, generator=g) + off).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    for b in (bias, None):
        val64, mag = _dense64(rows, cols, b, SIGMA)
        idx, val = _lib.gmm_assign(rows, cols, b, SIGMA, K)
        _check_topk(idx, val, val64, mag, K)


# ---------------------------------------------------------------------------------------
# 2. ties and chunk independence
# ---------------------------------------------------------------------------------------
def _first_split_n(M):
    from difficp_amd import _lib
    n = 1
    while n <= 2 ** 20:
        if _lib.num_splits(WS_GMM_ASSIGN, M, n) >= 2:
            return n
        n += 1
    pytest.fail("dicp_num_splits(DICP_WS_GMM_ASSIGN, 256, N) < 2 for every N <= 2^20")


def _host_merge(i0, v0, i1, v1, K):
    """Two sorted lists per row, the first over the lower columns: larger val first, equal val
    the smaller column -- a stable descending sort of [first, second]."""
    v = torch.cat([v0, v1], 1)
    i = torch.cat([i0, i1], 1)
    order = torch.sort(v, dim=1, descending=True, stable=True).indices[:, :K]
    return i.gather(1, order), v.gather(1, order)


@pytest.mark.parametrize("D", [2, 3])
def test_ties_and_chunk_independence(dev, D):
    from difficp_amd import _lib
    M = 256
    N = _first_split_n(M)
    g = torch.Generator().manual_seed(5 + D)
    rows = torch.rand(M, D, generator=g).to(dev)
    point = torch.rand(1, D, generator=g)
    same = point.expand(N, D).contiguous().to(dev)
    flat = torch.full((N,), 0.25, device=dev)
    for K in (1, 2, 4):
        idx, val = _lib.gmm_assign(rows, same, flat, SIGMA, K)
        want = torch.arange(K, device=dev, dtype=torch.int32)[None, :].expand(M, K)
        assert torch.equal(idx, want), K
        assert bool((val == val[:, :1]).all())
    # a random case at that N: reproducible, and equal to the column halves merged on the host
    cols = torch.rand(N, D, generator=g).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    # a few exact ties across the cut: duplicated columns with equal bias
    h = N // 3
    cols[h + 5] = cols[2]
    bias[h + 5] = bias[2]
    cols[N - 1] = cols[h - 1]
    bias[N - 1] = bias[h - 1]
    for K in (1, 2, 4):
        idx, val = _lib.gmm_assign(rows, cols, bias, SIGMA, K)
        idx2, val2 = _lib.gmm_assign(rows, cols, bias, SIGMA, K)
        assert torch.equal(idx, idx2) and torch.equal(val, val2)
        i0, v0 = _lib.gmm_assign(rows, cols[:h].contiguous(), bias[:h].contiguous(), SIGMA, K)
        i1, v1 = _lib.gmm_assign(rows, cols[h:].contiguous(), bias[h:].contiguous(), SIGMA, K)
        i1 = torch.where(i1 >= 0, i1 + h, i1)
        im, vm = _host_merge(i0, v0, i1, v1, K)
        assert torch.equal(idx, im), K
        assert torch.equal(val, vm), K


# ---------------------------------------------------------------------------------------
# 3. edge cases
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
def test_edge_cases(dev, D):
    from difficp_amd import _lib
    g = torch.Generator().manual_seed(77 + D)
    M = 70
    rows = torch.rand(M, D, generator=g).to(dev)
    # N < K: -1 / -inf in the slots that cannot be filled
    cols = torch.rand(2, D, generator=g).to(dev)
    bias = torch.randn(2, generator=g).to(dev)
    idx, val = _lib.gmm_assign(rows, cols, bias, SIGMA, 4)
    val64, mag = _dense64(rows, cols, bias, SIGMA)
    _check_topk(idx, val, val64, mag, 4)
    assert bool((idx[:, 2:] == -1).all()) and bool((val[:, 2:] == NEG_INF).all())
    assert bool((idx[:, :2] >= 0).all())
    # no columns at all, and no rows at all
    idx, val = _lib.gmm_assign(rows, cols[:0].contiguous(), None, SIGMA, 2)
    assert bool((idx == -1).all()) and bool((val == NEG_INF).all())
    idx, val = _lib.gmm_assign(rows[:0].contiguous(), cols, bias, SIGMA, 2)
    assert idx.shape == (0, 2) and val.shape == (0, 2)
    # all columns dead: unfilled slots
    N = 300
    cols = torch.rand(N, D, generator=g).to(dev)
    dead = torch.full((N,), NEG_INF, device=dev)
    idx, val = _lib.gmm_assign(rows, cols, dead, SIGMA, 4)
    assert bool((idx == -1).all()) and bool((val == NEG_INF).all())
    # non-finite rows: -1 / NaN in every slot, the other rows untouched
    bias = torch.randn(N, generator=g).to(dev)
    clean_i, clean_v = _lib.gmm_assign(rows, cols, bias, SIGMA, 4)
    bad = rows.clone()
    bad[5, D - 1] = float("nan")
    bad[6, 0] = float("inf")
    bad[M - 1, 0] = float("-inf")
    idx, val = _lib.gmm_assign(bad, cols, bias, SIGMA, 4)
    badrows = torch.tensor([5, 6, M - 1], device=dev)
    assert bool((idx[badrows] == -1).all()) and bool(torch.isnan(val[badrows]).all())
    ok = torch.ones(M, dtype=torch.bool, device=dev)
    ok[badrows] = False
    assert torch.equal(idx[ok], clean_i[ok]) and torch.equal(val[ok], clean_v[ok])
    # the binding: float32 only, k in 1..4
    with pytest.raises(TypeError):
        _lib.gmm_assign(rows.double(), cols, bias, SIGMA, 1)
    with pytest.raises(RuntimeError, match="invalid"):
        _lib.gmm_assign(rows, cols, bias, SIGMA, 5)


# ---------------------------------------------------------------------------------------
# 4. API
# ---------------------------------------------------------------------------------------
def _mixture(dev, D, outliers, dead=True):
    from difficp_amd.core.GMM import GaussianMixtureUnif
    spec = {"device": dev, "dtype": torch.float32}
    g = torch.Generator().manual_seed(200 + D)
    X = torch.rand(700, D, generator=g)
    mu = X[torch.randperm(700, generator=g)[:90]] + 0.03 * torch.randn(90, D, generator=g)
    G = GaussianMixtureUnif(mu, sigma=0.1, use_outliers=outliers, spec=spec)
    w = torch.randn(90, generator=g)
    if dead:
        w[3] = NEG_INF
    G.w = w.to(dev)
    if outliers:
        G.outliers["eta0"] = -1.5
    return G, X.to(dev)


def _dense_log_resp(G, X, dtype):
    """log_responsibilities restated densely in `dtype` from the float32 state: (lr (N, C), the
    component LSE T (N,), the pair magnitude |lpi_c| + d^2 / (2 sigma^2))."""
    x, mu, w = X.to(dtype), G.mu.to(dtype), G.w.to(dtype)
    lpi = w - w.logsumexp(0)
    d2 = ((x[:, None, :] - mu[None, :, :]) ** 2).sum(-1) / (2 * float(G.sigma) ** 2)
    t = lpi[None, :] - d2
    T = t.logsumexp(1)
    return t - T[:, None], T, torch.nan_to_num(lpi.abs(), posinf=0.0)[None, :] + d2


def _lse_tol(G, X, T64):
    """The LSE part of a log responsibility: the project's usual max(1e-5, 2 x the float32
    restatement's own deviation), relative to max(|T_n|, 1)."""
    from conftest import rel_err
    _, T32, _ = _dense_log_resp(G, X, torch.float32)
    rel = max(1e-5, 2 * rel_err(T32, T64))
    return rel * T64.abs().clamp(min=1.0)


@pytest.mark.parametrize("outliers", [False, True])
@pytest.mark.parametrize("D", [2, 3])
def test_assign_api(dev, D, outliers):
    """assign against the top-k of the dense float64 log responsibilities.  The pair tolerance is
    criteria (b) / (c)'s 16 eps32 magnitude in natural-log units: the kernel spends at most 8 of
    the 16 roundings, and the float32 bias column w2 = (w - LSE w) log2(e) the model hands it
    (three roundings relative to |lpi_c| ~ |LSE w|) fits in the other half.  log_resp carries
    the row's LSE as well (_lse_tol)."""
    G, X = _mixture(dev, D, outliers)
    lr64, T64, mag = _dense_log_resp(G, X, torch.float64)
    lse = _lse_tol(G, X, T64)[:, None]
    if outliers:
        with pytest.raises(ValueError):
            G.assign(X, k=1)
        G.set_vol0(X)
    for k in (1, 2, 4):
        a = G.assign(X, k=k)
        assert a.index.dtype == torch.int64 and a.index.shape == (700, k)
        assert a.log_resp.dtype == torch.float32 and a.log_resp.shape == (700, k)
        # indices: criteria (a), (c) on the dense rows; values: (b) with the LSE part added
        _check_topk(a.index, a.log_resp, lr64, mag, k, extra_tol=lse)
        assert not bool((a.index == 3).any()), "dead component returned"
        if outliers:
            lgn = D * (math.log(float(G.sigma)) + 0.5 * math.log(2 * math.pi))
            eta = G.outliers["eta0"] - math.log(G.outliers["vol0"]) - (T64 - lgn)
            lo64 = eta - torch.logaddexp(torch.zeros_like(eta), eta)
            assert a.log_outlier.shape == (700,)
            err = (a.log_outlier.double() - lo64).abs() / lo64.abs().clamp(min=1.0)
            assert float(err.max()) <= 1e-5, float(err.max())
        else:
            assert a.log_outlier is None
    # the model's own dense method agrees on the winner wherever the margin is clear
    dense = G.log_responsibilities(X)
    top2 = torch.topk(lr64, 2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4
    assert torch.equal(G.assign(X).index[clear, 0], dense.argmax(1)[clear])


@pytest.mark.parametrize("outliers", [False, True])
@pytest.mark.parametrize("D", [2, 3])
def test_nearest_points_api(dev, D, outliers):
    """nearest_points against the columns of the same dense float64 matrix.  The kernel's bias is
    -T2_n, the float32 LSE of the E-step, so its LSE deviation adds to the pair tolerance of
    every criterion (the pair magnitude is |lpi_c| + d^2 / (2 sigma^2), as for assign; the
    kernel's own roundings are relative to |T2_n| + k2 d^2, and its 8 eps32 |T_n| lies inside the
    LSE part, which is at least 1e-5 |T_n|)."""
    G, X = _mixture(dev, D, outliers)
    lr64, T64, mag = _dense_log_resp(G, X, torch.float64)
    lse = _lse_tol(G, X, T64)
    live = torch.ones(90, dtype=torch.bool, device=dev)
    live[3] = False
    for k in (1, 2, 4):
        index, log_resp = G.nearest_points(X, k=k)
        assert index.dtype == torch.int64 and index.shape == (90, k) and log_resp.shape == (90, k)
        assert bool((index[3] == -1).all()) and bool((log_resp[3] == NEG_INF).all())
        # per (component, point) tolerance: gather needs it per returned point -> fold the LSE
        # part into the magnitude matrix (tol = 16 eps32 mag)
        magT = (mag + lse[:, None] / (16 * EPS32)).t().contiguous()
        _check_topk(index[live], log_resp[live], lr64.t().contiguous()[live], magT[live], k)


@pytest.mark.parametrize("outliers", [False, True])
def test_calls_change_no_state(dev, outliers):
    """mu, w, sigma and a following EM_step (its E-step hint included) are bitwise unchanged."""
    import copy
    G1, X = _mixture(dev, 3, outliers, dead=False)
    G2 = copy.deepcopy(G1)
    G1.EM_step(X)
    G2.EM_step(X)                                  # both now hold an E-step hint for X
    mu, w, sigma = G1.mu.clone(), G1.w.clone(), G1.sigma
    hint = G1._estep_hint
    Xg = X.clone().requires_grad_(True)
    G1.assign(Xg, k=2)
    G1.nearest_points(Xg, k=2)
    G1.assign(X, k=4)
    G1.nearest_points(X, k=1)
    assert Xg.grad is None
    assert torch.equal(G1.mu, mu) and torch.equal(G1.w, w) and G1.sigma == sigma
    assert G1._estep_hint is hint
    r1, r2 = G1.EM_step(X), G2.EM_step(X)
    assert torch.equal(r1[0], r2[0])
    assert float(r1[1]) == float(r2[1]) and float(r1[2]) == float(r2[2])
    assert torch.equal(G1.mu, G2.mu) and torch.equal(G1.w, G2.w) and G1.sigma == G2.sigma


def test_multipsr_correspondences(dev):
    """2 frames x 2 structures, data on the host and compute on the device: what assign /
    nearest_points of GMMi[s] return on x1[k, s], bitwise, on the data spec."""
    from difficp_amd.core.GMM import Assignment, GaussianMixtureUnif
    from difficp_amd.core.PSR import MultiPSR
    cspec = {"device": dev, "dtype": torch.float32}
    dspec = {"device": "cpu", "dtype": torch.float32}
    g = torch.Generator().manual_seed(3)
    x = [[torch.rand(40 + 10 * k + 5 * s, 2, generator=g) for s in range(2)] for k in range(2)]
    GMMi = [GaussianMixtureUnif(torch.rand(7 + s, 2, generator=g), sigma=0.2, use_outliers=(s == 1), spec=cspec)
            for s in range(2)]
    PS = MultiPSR(x, GMMi, dataspec=dspec, compspec=cspec)
    PS.printstuff = False
    PS.GMM_opt(max_iterations=3)
    state = [(gm.mu.clone(), gm.w.clone(), gm.sigma) for gm in PS.GMMi]
    for k in range(2):
        for s in range(2):
            gm, X = PS.GMMi[s], PS.x1[k, s].to(**cspec)
            a = PS.correspondences(k=k, s=s, topk=2)
            b = gm.assign(X, k=2)
            assert isinstance(a, Assignment)
            assert a.index.device.type == "cpu" and a.log_resp.device.type == "cpu"
            assert torch.equal(a.index, b.index.cpu()) and torch.equal(a.log_resp, b.log_resp.cpu())
            if s == 1:
                assert torch.equal(a.log_outlier, b.log_outlier.cpu())
            else:
                assert a.log_outlier is None
            i, lr = PS.correspondences(k=k, s=s, topk=3, direction="template")
            i2, lr2 = gm.nearest_points(X, k=3)
            assert i.device.type == "cpu" and i.shape == (gm.C, 3)
            assert torch.equal(i, i2.cpu()) and torch.equal(lr, lr2.cpu())
    with pytest.raises(ValueError):
        PS.correspondences(direction="sideways")
    for gm, (mu, w, sigma) in zip(PS.GMMi, state):
        assert torch.equal(gm.mu, mu) and torch.equal(gm.w, w) and gm.sigma == sigma


# ---------------------------------------------------------------------------------------
# 5. size
# ---------------------------------------------------------------------------------------
def test_full_size(dev):
    """100k points against 100k components, D = 3, K = 1 (the dense route would need a 40 GB
    result): completes, and 256 sampled rows meet the criteria against their float64 rows."""
    from difficp_amd.core.GMM import GaussianMixtureUnif
    n = 100_000
    g = torch.Generator().manual_seed(11)
    X = torch.rand(n, 3, generator=g).to(dev)
    mu = torch.rand(n, 3, generator=g).to(dev)
    G = GaussianMixtureUnif(mu, sigma=0.02, spec={"device": dev, "dtype": torch.float32})
    G.w = (0.5 * torch.randn(n, generator=g)).to(dev)
    a = G.assign(X, k=1)
    assert a.index.shape == (n, 1) and a.log_outlier is None
    assert bool((a.index >= 0).all()) and bool((a.index < n).all())
    rows = torch.randperm(n, generator=g)[:256].to(dev)
    Xs = X[rows].contiguous()
    lr64, T64, mag = _dense_log_resp(G, Xs, torch.float64)
    _check_topk(a.index[rows], a.log_resp[rows], lr64, mag, 1, extra_tol=_lse_tol(G, Xs, T64)[:, None])
