"""Soft label / field transfer: the fused responsibility-weighted mean dicp_gmm_carry_f32
(csrc/carry.hip) and the interfaces built on it -- GaussianMixtureUnif.carry_to_points /
pool_from_points, MultiPSR.carry_to_frame / pool_to_template.

The reference is tests/carry_ref.py: the dense float64 softmax of the same float32 inputs, with
    tol_out(i, f) = 2 [ ln2 sum_j p_ij h_ij |feat_jf - out_if| + n_acc eps32 sum_j p_ij |feat_jf| ]
    tol_lse(i)    = 2 [ sum_j p_ij h_ij + n_acc eps32 / ln2 ] + 4 eps32 |lse_i|
    h_ij = 8 eps32 (|bias_j| + k2 |r_i - y_j|^2),   n_acc = 256 + (ceil(N / 256) + 1) + 8:
the tile is 256 records, and a sum goes through ceil(chunk / 256) tile sums and S chunk partials,
at most ceil(N / 256) + 1 since a chunk holds at least 256 columns (carry_ref's docstring counts
every term).  No rows are excluded.  Dense, so every case keeps M N <= 1.5e6.

The bound checked without a GPU (tests/test_carry_host.py, carry_ref.restate32: the kernel's
arithmetic in float32 torch ops -- integer reference moved at a tile sum of 2^60, sums per tile of
256, two chunks merged in order), 130 x 1300, F = 5, a dead column with NaN features: worst
error / tolerance (out, lse) 0.004 / 0.004 for the unit cube, sigma 0.1, bias 2 N(0,1); 0.009 /
0.021 offset by 100, sigma 0.02, bias 100 N(0,1); 0.010 / 0.023 for the plain cube with those.
Every check below prints its own worst ratio; on the MI355X the worst over this file was 0.042
(out) and 0.057 (lse), both in the far-rows case of test_shift_robustness.
"""
import math

import pytest
import torch

import carry_ref as CR

pytestmark = pytest.mark.gpu

LOG2E, LN2, EPS32 = CR.LOG2E, CR.LN2, CR.EPS32
WS_GMM_CARRY = 16
NEG_INF = float("-inf")
NAN = float("nan")
FMAX = 40
MS = (1, 63, 65, 257, 513, 1000)
NS = (1, 3, 255, 257, 300, 5000)
FS = (1, 3, 16, 17, 40)
_cases = {}


def _inputs(dev, D, M, N, offset=0.0, bscale=2.0, seed=0):
    g = torch.Generator().manual_seed(1000 * D + 7 * M + N + seed)
    rows = (torch.rand(M, D, generator=g) + offset).to(dev)
    cols = (torch.rand(N, D, generator=g) + offset).to(dev)
    bias = (bscale * torch.randn(N, generator=g)).to(dev)
    feat = torch.randn(N, FMAX, generator=g).to(dev)
    if N >= 3:
        bias[N // 2] = NEG_INF                               # a dead column, its features NaN
        feat[N // 2] = NAN
    return rows, cols, bias, feat


def _case(dev, D, M, N, sigma=0.1, offset=0.0, bscale=2.0):
    """Inputs and the float64 reference (all FMAX channels) of one shape and family, made once
    and shared by every F."""
    key = (D, M, N, sigma, offset, bscale)
    if key not in _cases:
        a = _inputs(dev, D, M, N, offset, bscale)
        _cases[key] = a + (CR.carry_ref(*a, sigma),)
    return _cases[key]


def _cut(ref, F):
    return CR.CarryRef(ref.out[:, :F], ref.lse, ref.p, ref.tol_out[:, :F], ref.tol_lse)


# ---------------------------------------------------------------------------------------
# 1. against float64
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("D", [2, 3])
def test_against_float64(dev, D, F):
    from difficp_amd import _lib
    for M in MS:
        for N in NS:
            if M * N > 1.5e6:
                continue
            rows, cols, bias, feat, ref = _case(dev, D, M, N)
            out, lse2 = _lib.gmm_carry(rows, cols, bias, feat[:, :F].contiguous(), 0.1)
            assert out.dtype == torch.float32 and out.shape == (M, F) and lse2.shape == (M,)
            CR.check(out, lse2, _cut(ref, F), f"D{D} M{M} N{N} F{F}")


@pytest.mark.parametrize("offset,sigma,bscale", [(100.0, 0.1, 2.0), (0.0, 0.02, 100.0), (100.0, 0.02, 100.0),
                                                 (100.0, 0.02, 2.0), (0.0, 0.02, 2.0), (0.0, 0.1, 100.0),
                                                 (100.0, 0.1, 100.0)])
@pytest.mark.parametrize("D", [2, 3])
def test_input_families(dev, D, offset, sigma, bscale):
    """The other families of the bound's check: the cube offset by 100, sigma 0.02, bias
    100 N(0, 1), on a one-tile, a ragged and a chunked shape, F = 16 and 3."""
    from difficp_amd import _lib
    for M, N in [(257, 300), (65, 5000), (1000, 257)]:
        rows, cols, bias, feat, ref = _case(dev, D, M, N, sigma, offset, bscale)
        for F in (16, 3):
            out, lse2 = _lib.gmm_carry(rows, cols, bias, feat[:, :F].contiguous(), sigma)
            CR.check(out, lse2, _cut(ref, F), f"D{D} M{M} N{N} F{F} offset {offset} sigma {sigma} bias x{bscale}")


# ---------------------------------------------------------------------------------------
# 2. the shift needs no help from the caller
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
def test_shift_robustness(dev, D):
    from difficp_amd import _lib
    g = torch.Generator().manual_seed(50 + D)
    M, N, F = 257, 5000, 3
    cols = torch.rand(N, D, generator=g).to(dev)
    feat = torch.randn(N, F, generator=g).to(dev)
    bias = (2.0 * torch.randn(N, generator=g)).to(dev)

    def run(what, rows, cols, bias, feat, sigma):
        ref = CR.carry_ref(rows, cols, bias, feat, sigma)
        out, lse2 = _lib.gmm_carry(rows, cols, bias, feat, sigma)
        CR.check(out, lse2, ref, f"D{D} {what}")
        return ref

    # rows far from every column (displaced by 3 per coordinate, sigma 0.1: 20 to 60 sigma away,
    # every logit below -500): still the softmax over the nearest columns
    far = (torch.rand(M, D, generator=g) + 3.0).to(dev)
    ref = run("far rows", far, cols, bias, feat, 0.1)
    assert float(ref.lse.max()) < -500 and bool(torch.isfinite(ref.out).all())
    # columns by increasing and by decreasing logit of row 0 (sigma 0.02: a span of thousands
    # of log2 units, so the reference moves many times, or never after the first tile)
    rows = torch.rand(M, D, generator=g).to(dev)
    e0 = bias.double() - CR.k2_of(0.02) * ((rows[0].double()[None, :] - cols.double()) ** 2).sum(1)
    for name, desc in (("rising", False), ("falling", True)):
        o = torch.argsort(e0, descending=desc)
        assert float(e0.max() - e0.min()) > 1000
        run(name + " logits", rows, cols[o].contiguous(), bias[o].contiguous(), feat[o].contiguous(), 0.02)
    # a bias like -T2 of a far cloud
    big = (-1.0e4 + 50.0 * torch.randn(N, generator=g)).to(dev)
    run("bias near -1e4", rows, cols, big, feat, 0.1)
    # the cloud 1000 sigma from the origin, no bias
    run("offset cloud, no bias", rows + 100.0, cols + 100.0, None, feat, 0.1)


# ---------------------------------------------------------------------------------------
# 3. edge cases
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
def test_edge_cases(dev, D):
    from difficp_amd import _lib
    g = torch.Generator().manual_seed(77 + D)
    M, N, F = 70, 300, 17
    rows = torch.rand(M, D, generator=g).to(dev)
    cols = torch.rand(N, D, generator=g).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    feat = torch.randn(N, F, generator=g).to(dev)
    # no columns; no rows
    out, lse2 = _lib.gmm_carry(rows, cols[:0].contiguous(), None, feat[:0].contiguous(), 0.1)
    assert out.shape == (M, F) and bool(torch.isnan(out).all()) and bool((lse2 == NEG_INF).all())
    out, lse2 = _lib.gmm_carry(rows[:0].contiguous(), cols, bias, feat, 0.1)
    assert out.shape == (0, F) and lse2.shape == (0,)
    # all columns dead
    dead = torch.full((N,), NEG_INF, device=dev)
    out, lse2 = _lib.gmm_carry(rows, cols, dead, feat, 0.1)
    assert bool(torch.isnan(out).all()) and bool((lse2 == NEG_INF).all())
    # non-finite rows: NaN, the other rows bitwise untouched
    clean_o, clean_l = _lib.gmm_carry(rows, cols, bias, feat, 0.1)
    assert bool(torch.isfinite(clean_o).all()) and bool(torch.isfinite(clean_l).all())
    bad = rows.clone()
    bad[5, D - 1] = NAN
    bad[6, 0] = float("inf")
    bad[M - 1, 0] = NEG_INF
    out, lse2 = _lib.gmm_carry(bad, cols, bias, feat, 0.1)
    badrows = torch.tensor([5, 6, M - 1], device=dev)
    assert bool(torch.isnan(out[badrows]).all()) and bool(torch.isnan(lse2[badrows]).all())
    ok = torch.ones(M, dtype=torch.bool, device=dev)
    ok[badrows] = False
    assert torch.equal(out[ok], clean_o[ok]) and torch.equal(lse2[ok], clean_l[ok])
    # a non-finite feature in a live column: that channel is non-finite in every row (there is
    # no skipping by weight), every other channel and lse2 bitwise untouched
    for f_bad, v in ((2, NAN), (16, float("inf"))):
        fb = feat.clone()
        fb[11, f_bad] = v
        out, lse2 = _lib.gmm_carry(rows, cols, bias, fb, 0.1)
        assert not bool(torch.isfinite(out[:, f_bad]).any())
        keep = [f for f in range(F) if f != f_bad]
        assert torch.equal(out[:, keep], clean_o[:, keep]) and torch.equal(lse2, clean_l)
    # the binding: float32 only, shapes
    with pytest.raises(TypeError):
        _lib.gmm_carry(rows.double(), cols, bias, feat, 0.1)
    with pytest.raises(ValueError):
        _lib.gmm_carry(rows, cols, bias, feat[:-1].contiguous(), 0.1)
    with pytest.raises(ValueError):
        _lib.gmm_carry(rows, cols, bias[:-1].contiguous(), feat, 0.1)


# ---------------------------------------------------------------------------------------
# 4. chunks and determinism
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
def test_chunks_and_determinism(dev, D):
    from difficp_amd import _lib
    M, N = 257, 5000
    assert _lib.num_splits(WS_GMM_CARRY, M, N) > 1
    rows, cols, bias, feat, ref = _case(dev, D, M, N)
    F = 17
    f17 = feat[:, :F].contiguous()
    out, lse2 = _lib.gmm_carry(rows, cols, bias, f17, 0.1)
    out2, lse22 = _lib.gmm_carry(rows, cols, bias, f17, 0.1)
    assert torch.equal(out, out2) and torch.equal(lse2, lse22)
    # the channel blocks: F = 17 is F = 16 next to F = 1, bitwise
    o16, l16 = _lib.gmm_carry(rows, cols, bias, feat[:, :16].contiguous(), 0.1)
    o1, l1 = _lib.gmm_carry(rows, cols, bias, feat[:, 16:17].contiguous(), 0.1)
    assert torch.equal(out, torch.cat([o16, o1], 1))
    assert torch.equal(lse2, l16) and torch.equal(lse2, l1)
    # the two column halves, run separately and combined on the host through (lse2, out)
    h = N // 3
    a = _lib.gmm_carry(rows, cols[:h].contiguous(), bias[:h].contiguous(), f17[:h].contiguous(), 0.1)
    b = _lib.gmm_carry(rows, cols[h:].contiguous(), bias[h:].contiguous(), f17[h:].contiguous(), 0.1)
    oc, lc = CR.combine_halves(a[0], a[1], b[0], b[1])
    CR.check(oc, lc, _cut(ref, F), f"D{D} halves combined")
    CR.check(out, lse2, _cut(ref, F), f"D{D} whole")


# ---------------------------------------------------------------------------------------
# 5. identities against the existing kernels (each side against float64, in its own tolerance)
# ---------------------------------------------------------------------------------------
def _mixture(dev, D, outliers, dead=True, N=700, C=90):
    from difficp_amd.core.GMM import GaussianMixtureUnif
    spec = {"device": dev, "dtype": torch.float32}
    g = torch.Generator().manual_seed(200 + D)
    X = torch.rand(N, D, generator=g)
    mu = X[torch.randperm(N, generator=g)[:C]] + 0.03 * torch.randn(C, D, generator=g)
    G = GaussianMixtureUnif(mu, sigma=0.1, use_outliers=outliers, spec=spec)
    w = torch.randn(C, generator=g)
    if dead:
        w[3] = NEG_INF
    G.w = w.to(dev)
    if outliers:
        G.outliers["eta0"] = -1.5
    return G, X.to(dev)


@pytest.mark.parametrize("D", [2, 3])
def test_identities(dev, D):
    from difficp_amd import _lib
    G, X = _mixture(dev, D, False, dead=False)
    mu = G.mu.contiguous()
    _, w2, mu2 = G._columns(mu, G.w)
    sigma = float(G.sigma)
    # lse2 of (X, mu, w2) is the E-step's T2
    ref = CR.carry_ref(X, mu, w2, mu, sigma)
    out, lse2 = _lib.gmm_carry(X, mu, w2, mu, sigma)
    CR.check(out, lse2, ref, f"D{D} rows X, features mu")
    _, T2, _ = _lib.gmm_estep(X, mu, w2, mu2, sigma, 0.0, False)
    # the existing passes against the same float64 sums, in their own tolerances: carry_ref's
    # with the expansion-form magnitudes (and the M-step's row constant w2_c)
    old = CR.carry_ref(X, mu, w2, mu, sigma, expansion=True)
    Y = G.EM_step(X, skip_M=True)[0]
    CR.check(Y, T2, old, f"D{D} E-step T2 and targets Y")
    # carry_to_points(X, mu) is the E-step's targets Y
    c = G.carry_to_points(X, mu)
    assert torch.equal(c.values, out) and c.log_outlier is None
    # pool_from_points(X, X) and its mass are the M-step's means and weights
    bias = (-T2).contiguous()
    refp = CR.carry_ref(mu, X, bias, X, sigma)
    p = G.pool_from_points(X, X)
    CR.check(p.values, torch.log2(p.mass) - w2, refp, f"D{D} rows mu, features X")
    col = _lib.gmm_mstep(X, T2, mu, w2, sigma)
    oldp = CR.carry_ref(mu, X, bias, X, sigma, expansion=True, row_mag=w2)
    CR.check(col[:, 1:], col[:, 0] * LOG2E - w2, oldp, f"D{D} M-step means and log-weights")
    # one-hot labels: the rows of the carried probabilities sum to 1 (the sum, not the entries: a
    # probability below 2^-126 of the row's largest is flushed by float32 itself)
    lab = torch.eye(G.C, device=dev)
    refl = CR.carry_ref(X, mu, w2, lab, sigma)
    got = G.carry_to_points(X, lab).values
    assert bool(((got.double().sum(1) - 1).abs() <= refl.tol_out.sum(1) + G.C * EPS32).all())
    # a constant field carries and pools to itself
    for n, rows, cols, b in ((G.C, X, mu, w2), (X.shape[0], mu, X, bias)):
        const = torch.full((n, 1), 2.5, device=dev)
        refc = CR.carry_ref(rows, cols, b, const, sigma)
        got, _ = _lib.gmm_carry(rows, cols, b, const, sigma)
        assert bool(((got.double() - 2.5).abs() <= refc.tol_out).all())
    assert bool(((G.pool_from_points(X, torch.full((X.shape[0],), 2.5)).values - 2.5).abs() < 1e-5).all())


# ---------------------------------------------------------------------------------------
# 6. API
# ---------------------------------------------------------------------------------------
def _pool_bias(G, X, weights):
    """The bias column pool_from_points hands the kernel, restated: -T2 + log2 (1 - gamma0) +
    log2 weights from the float32 E-step (the reference takes the same float32 column)."""
    from difficp_amd import _lib
    mu = G.mu.contiguous()
    _, w2, mu2 = G._columns(mu, G.w)
    sigma = float(G.sigma)
    lgn = G.D * (math.log(sigma) + 0.5 * math.log(2 * math.pi))
    T, T2, _ = _lib.gmm_estep(X, mu, w2, mu2, sigma, lgn, False)
    bias = -T2
    if G.outliers is not None:
        eta = G.outliers["eta0"] - math.log(G.outliers["vol0"]) - T
        bias = bias + LOG2E * G.log_ratio_to_proba(eta)[1]
    if weights is not None:
        bias = bias + torch.log2(weights)
    return bias.contiguous(), w2


def _dense_gamma(G, X, weights):
    """float64 gamma_nc = r_nc (1 - gamma0_n) weights_n from the float32 state."""
    x, mu, w = X.double(), G.mu.double(), G.w.double()
    t = (w - w.logsumexp(0))[None, :] - ((x[:, None, :] - mu[None, :, :]) ** 2).sum(-1) / (2 * G.sigma ** 2)
    gam = torch.softmax(t, 1)
    if G.outliers is not None:
        T = t.logsumexp(1) - G.D * (math.log(G.sigma) + 0.5 * math.log(2 * math.pi))
        gam = gam * (1 - torch.sigmoid(G.outliers["eta0"] - math.log(G.outliers["vol0"]) - T))[:, None]
    if weights is not None:
        gam = gam * weights.double()[:, None]
    return gam


def _check_pool(G, X, vals, weights, p, what):
    """Pooled p against carry_ref on the restated bias (values within tol_out; mass = 2^(lse2 +
    w2) within the lse tolerance and the float32 add and exp2), and loosely against the dense
    float64 gamma (the semantics: discount, weights)."""
    bias, w2 = _pool_bias(G, X, weights)
    V = vals.reshape(X.shape[0], -1)
    ref = CR.carry_ref(G.mu, X, bias, V, float(G.sigma))
    live = torch.isfinite(w2) & torch.isfinite(ref.lse)
    got = p.values.reshape(G.C, -1)
    assert bool(torch.isnan(got[~live]).all()) and bool((p.mass[~live] == 0).all())
    assert bool(((got.double() - ref.out).abs() <= ref.tol_out)[live].all()), what
    mass64 = torch.exp2(ref.lse + w2.double())
    rel = LN2 * (ref.tol_lse + 2 * EPS32 * (ref.lse + w2.double()).abs()) + 4 * EPS32
    assert bool((((p.mass.double() - mass64) / mass64).abs() <= rel)[live].all()), what
    gam = _dense_gamma(G, X, weights)
    m = gam.sum(0)
    assert float(((p.mass.double() - m) / m)[live].abs().max()) < 1e-4, what
    want = gam.t() @ V.double() / m[:, None]
    assert float((got.double() - want)[live].abs().max()) < 1e-4 * max(1.0, float(V.abs().max())), what


@pytest.mark.parametrize("outliers", [False, True])
@pytest.mark.parametrize("D", [2, 3])
def test_gmm_api(dev, D, outliers):
    from difficp_amd.core.GMM import Carried, Pooled
    G, X = _mixture(dev, D, outliers)          # component 3 is dead
    N = X.shape[0]
    g = torch.Generator().manual_seed(7)
    cv = torch.randn(G.C, 5, generator=g).to(dev)
    cv[3] = NAN                                # never read
    pv = torch.randn(N, 3, generator=g).to(dev)
    wts = torch.rand(N, generator=g).to(dev)
    wts[:9] = 0.0
    if outliers:
        with pytest.raises(ValueError):
            G.carry_to_points(X, cv)
        with pytest.raises(ValueError):
            G.pool_from_points(X, pv)
        G.set_vol0(X)
    state = (G.mu.clone(), G.w.clone(), G.sigma)
    _, w2, _ = G._columns(G.mu.contiguous(), G.w)
    ref = CR.carry_ref(X, G.mu, w2, cv, float(G.sigma))
    c = G.carry_to_points(X.clone().requires_grad_(True), cv)
    assert isinstance(c, Carried) and c.values.shape == (N, 5) and not c.values.requires_grad
    assert bool(((c.values.double() - ref.out).abs() <= ref.tol_out).all())
    c1 = G.carry_to_points(X, cv[:, 1])
    assert c1.values.shape == (N,) and bool(((c1.values.double() - ref.out[:, 1]).abs() <= ref.tol_out[:, 1]).all())
    if outliers:
        # log gamma0 = log sigmoid(eta), eta = eta0 - log vol0 - T, T = ln2 lse2 - lgn: its slope in
        # T is at most 1, so the lse tolerance carries over, with the float32 roundings of the
        # few host operations relative to the magnitudes they act on
        lgn = D * (math.log(float(G.sigma)) + 0.5 * math.log(2 * math.pi))
        T64 = LN2 * ref.lse - lgn
        eta = G.outliers["eta0"] - math.log(G.outliers["vol0"]) - T64
        lo64 = eta - torch.logaddexp(torch.zeros_like(eta), eta)
        assert c.log_outlier.shape == (N,)
        bound = LN2 * ref.tol_lse + 8 * EPS32 * (T64.abs() + abs(lgn) + eta.abs() + lo64.abs() + 1)
        assert bool(((c.log_outlier.double() - lo64).abs() <= bound).all())
    else:
        assert c.log_outlier is None
    for w in (None, wts):
        p = G.pool_from_points(X, pv, weights=w)
        assert isinstance(p, Pooled) and p.values.shape == (G.C, 3) and p.mass.shape == (G.C,)
        _check_pool(G, X, pv, w, p, f"D{D} outliers {outliers} weights {w is not None}")
        p1 = G.pool_from_points(X, pv[:, 0], weights=w)
        assert p1.values.shape == (G.C,)
        assert torch.equal(torch.nan_to_num(p1.values), torch.nan_to_num(p.values[:, 0]))
    assert torch.equal(G.mu, state[0]) and torch.equal(G.w, state[1]) and G.sigma == state[2]


def test_multipsr_api(dev):
    """3 frames x 2 structures (about 400 points, C = 32), data on the host and compute on the
    device: carry_to_frame is carry_to_points on x1[k, s]; pool_to_template is the mass-weighted
    float64 combination of the frames' pools, each checked against carry_ref; a frame given zero
    weights drops out."""
    from difficp_amd.core.GMM import Carried, GaussianMixtureUnif, Pooled
    from difficp_amd.core.PSR import MultiPSR
    cspec = {"device": dev, "dtype": torch.float32}
    dspec = {"device": "cpu", "dtype": torch.float32}
    g = torch.Generator().manual_seed(3)
    K, S, D = 3, 2, 3
    x = [[torch.rand(60 + 10 * k + 5 * s, D, generator=g) for s in range(S)] for k in range(K)]
    GMMi = [GaussianMixtureUnif(torch.rand(32, D, generator=g), sigma=0.2, use_outliers=(s == 1), spec=cspec)
            for s in range(S)]
    PS = MultiPSR(x, GMMi, dataspec=dspec, compspec=cspec)
    PS.printstuff = False
    PS.GMM_opt(max_iterations=3)
    state = [(gm.mu.clone(), gm.w.clone(), gm.sigma) for gm in PS.GMMi]
    for s in range(S):
        gm = PS.GMMi[s]
        tv = torch.randn(gm.C, 2, generator=g)
        _, w2, _ = gm._columns(gm.mu.contiguous(), gm.w)
        for k in range(K):
            X = PS.x1[k, s].to(**cspec)
            a = PS.carry_to_frame(tv, k=k, s=s)
            assert isinstance(a, Carried) and a.values.device.type == "cpu" and a.values.shape == (X.shape[0], 2)
            ref = CR.carry_ref(X, gm.mu, w2, tv.to(dev), float(gm.sigma))
            assert bool(((a.values.double() - ref.out.cpu()).abs() <= ref.tol_out.cpu()).all())
            assert (a.log_outlier is None) == (s == 0)
        vals = [torch.randn(int(PS.N[k, s]), 2, generator=g) for k in range(K)]
        wts = [None, torch.zeros(int(PS.N[1, s])), torch.rand(int(PS.N[2, s]), generator=g)]
        num = torch.zeros(gm.C, 2, dtype=torch.float64, device=dev)
        den = torch.zeros(gm.C, dtype=torch.float64, device=dev)
        tol = torch.zeros(gm.C, 2, dtype=torch.float64, device=dev)
        for k in range(K):
            X = PS.x1[k, s].to(**cspec)
            w = None if wts[k] is None else wts[k].to(dev)
            p = gm.pool_from_points(X, vals[k].to(dev), weights=w)
            if k == 1:
                assert bool((p.mass == 0).all()) and bool(torch.isnan(p.values).all())
                continue
            _check_pool(gm, X, vals[k].to(dev), w, p, f"s{s} k{k}")
            bias, _ = _pool_bias(gm, X, w)
            ref = CR.carry_ref(gm.mu, X, bias, vals[k].to(dev), float(gm.sigma))
            m = p.mass.double()
            num += m[:, None] * ref.out
            tol += m[:, None] * ref.tol_out
            den += m
        pt = PS.pool_to_template(vals, s=s, weights=wts)
        assert isinstance(pt, Pooled) and pt.values.device.type == "cpu" and pt.values.shape == (gm.C, 2)
        # the combination itself is float64: the frames' tolerances, weighted alike, and the
        # final rounding to float32
        want = (num / den[:, None]).cpu()
        bound = (tol / den[:, None]).cpu() + EPS32 * want.abs()
        assert bool(((pt.values.double() - want).abs() <= bound).all())
        assert bool(((pt.mass.double() - den.cpu()).abs() <= EPS32 * den.cpu()).all())
        pd = PS.pool_to_template({k: vals[k][:, 0] for k in range(K)}, s=s, weights=wts)
        assert pd.values.shape == (gm.C,) and torch.equal(pd.values, pt.values[:, 0])
    for gm, (mu, w, sigma) in zip(PS.GMMi, state):
        assert torch.equal(gm.mu, mu) and torch.equal(gm.w, w) and gm.sigma == sigma
