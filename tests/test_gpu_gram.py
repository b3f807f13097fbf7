"""dicp_rkhs_gram_f32 (csrc/gram.hip) on the device: the kernel against the float64 statement of
tests/gram_ref.py within C 2^-24 A per pair (ragged sizes around the tile, row-block and chunk
boundaries, clouds at offset 100), its bitwise guarantees (repeatable, independent of the other
pairs of the call, permutation of the pair list), non-finite inputs, consistency with the
Hamiltonian and the KRed reduction, and tangent-space PCA of a DiffPSR end to end without fitting."""
import math

import pytest
import torch

import gram_ref as GR

pytestmark = pytest.mark.gpu


def _lib():
    from difficp_amd import _lib
    return _lib


def _model(dev, D, sigma=0.2, **kw):
    from difficp_amd.core.LDDMM import LDDMMModel
    args = dict(sigma=sigma, D=D, lambd=10.0, version="classic", scheme="Euler", nt=10,
                spec={"device": dev, "dtype": torch.float32})
    args.update(kw)
    return LDDMMModel(**args)


@pytest.mark.parametrize("shift", GR.SHIFTS)
@pytest.mark.parametrize("D,sigma", GR.CASES)
def test_kernel_against_float64(dev, D, sigma, shift):
    L = _lib()
    # the split pair really takes the chunk-merge path, at the smallest size that does
    assert L.num_splits(L.WS_RKHS_GRAM, GR.SPLIT_SIZE, 1) >= 2
    assert L.num_splits(L.WS_RKHS_GRAM, GR.SPLIT_SIZE - 1, 1) == 1
    for _, _, _, q, p, off, pairs in GR.test_inputs([(D, sigma)], [shift]):
        out = L.rkhs_gram(q.to(dev), p.to(dev), off, pairs, sigma)
        assert out.dtype == torch.float64 and out.shape == (len(pairs),)
        GR.check(out, q, p, off, pairs, sigma, what=f"D {D} sigma {sigma} shift {shift} pairs {len(pairs)}")


@pytest.mark.parametrize("D", [2, 3])
def test_bitwise_guarantees(dev, D):
    L = _lib()
    sigma = 0.3
    q, p, off = GR.fields(D)
    q, p = q.to(dev), p.to(dev)
    pairs = GR.all_pairs(len(GR.SIZES))
    out = L.rkhs_gram(q, p, off, pairs, sigma)
    assert torch.equal(out, L.rkhs_gram(q, p, off, pairs, sigma))
    # a permuted (and partly repeated) pair list gives the permuted outputs
    perm = torch.randperm(len(pairs), generator=torch.Generator().manual_seed(1)).tolist()
    perm = perm + perm[:7]
    again = L.rkhs_gram(q, p, off, [pairs[i] for i in perm], sigma)
    assert torch.equal(again.cpu(), out.cpu()[perm])
    # every pair alone in a call of its own, over the same fields (hence the same max_rows)
    alone = torch.stack([L.rkhs_gram(q, p, off, [pr], sigma)[0] for pr in pairs])
    assert torch.equal(alone, out)
    # the other order of a pair is the same sum over the transposed tiles: equal within rounding
    swapped = L.rkhs_gram(q, p, off, [(b, a) for a, b in pairs], sigma)
    GR.check(swapped, q, p, off, pairs, sigma, what=f"D {D} swapped")


def test_split_pair_bitwise_in_any_company(dev):
    """The pair whose columns split in two chunks: alone, and next to other pairs."""
    L = _lib()
    q, p, off = GR.fields(3, sizes=(GR.SPLIT_SIZE, 5, GR.SPLIT_SIZE), seed=1)
    q, p = q.to(dev), p.to(dev)
    alone = L.rkhs_gram(q, p, off, [(0, 2)], 0.3)
    many = L.rkhs_gram(q, p, off, [(1, 1), (0, 2), (0, 1), (2, 0), (0, 2)], 0.3)
    assert torch.equal(many[1], alone[0]) and torch.equal(many[4], alone[0])
    GR.check(many, q, p, off, [(1, 1), (0, 2), (0, 1), (2, 0), (0, 2)], 0.3, what="split pair in company")


def test_no_fields_and_empty_fields(dev):
    L = _lib()
    q = torch.rand(7, 2, device=dev)
    out = L.rkhs_gram(q, q, [0, 0, 7, 7], [(0, 0), (0, 1), (2, 1), (1, 1)], 0.5)
    assert out[:3].tolist() == [0.0, 0.0, 0.0] and float(out[3]) > 0
    e = torch.empty(0, 2, device=dev)
    assert L.rkhs_gram(e, e, [0, 0, 0], [(0, 1), (1, 1)], 0.5).tolist() == [0.0, 0.0]
    assert L.rkhs_gram(q, q, [0, 7], [], 0.5).shape == (0,)
    with pytest.raises(ValueError, match="pair indices"):
        L.rkhs_gram(q, q, [0, 7], [(0, 1)], 0.5)
    with pytest.raises(ValueError, match="offsets"):
        L.rkhs_gram(q, q, [0, 9], [(0, 0)], 0.5)


@pytest.mark.parametrize("what", ["momentum", "coordinate"])
def test_non_finite_input_stays_in_its_pairs(dev, what):
    L = _lib()
    D, sigma, bad = 3, 0.3, 5
    q, p, off = GR.fields(D)
    q, p = q.to(dev), p.to(dev)
    pairs = GR.all_pairs(len(GR.SIZES))
    clean = L.rkhs_gram(q, p, off, pairs, sigma)
    q2, p2 = q.clone(), p.clone()
    row = off[bad] + 100
    if what == "momentum":
        p2[row, 1] = float("nan")
    else:
        q2[row, 0] = float("inf")      # an infinite distance alone would give weight 0
    out = L.rkhs_gram(q2, p2, off, pairs, sigma)
    for n, (a, b) in enumerate(pairs):
        if bad in (a, b) and GR.SIZES[a] > 0 and GR.SIZES[b] > 0:
            assert not math.isfinite(float(out[n])), (a, b)
        else:
            assert torch.equal(out[n], clean[n]), (a, b)


def test_diagonal_is_twice_the_hamiltonian(dev):
    """field_gram of one field against 2 H(q, p) at eta = 0, within the forward tolerance
    tests/test_gpu_api.py holds the float32 path to (1e-5 relative)."""
    g = torch.Generator().manual_seed(4)
    for D, M in ((2, 300), (3, 700)):
        LM = _model(dev, D)
        q = torch.rand(M, D, generator=g).to(dev)
        p = (0.1 * torch.randn(M, D, generator=g)).to(dev)
        G = LM.field_gram([(q, p)])
        assert G.shape == (1, 1) and G.dtype == torch.float64
        H2 = 2.0 * float(LM.Hamiltonian(q, p))
        assert abs(float(G[0, 0]) - H2) <= 1e-5 * abs(H2)


def test_cross_form_against_kred(dev):
    """field_gram(A, B) against (p_a * KRed(q_a, q_b, p_b)).sum() formed in float64 from the
    float32 rows, within the sum of both tolerances: C 2^-24 A for the Gram entry, and for the sum
    of the rows |p_a| times the norm-wise 1e-5 that tests/test_gpu_kernels.py holds KRed to."""
    D, sigma = 3, 0.2
    LM = _model(dev, D, sigma=sigma)
    g = torch.Generator().manual_seed(9)
    sizes = (300, 513)
    fa, fb = [(torch.rand(n, D, generator=g).to(dev), torch.randn(n, D, generator=g).to(dev)) for n in sizes]
    G = LM.field_gram([fa], [fb])
    assert G.shape == (1, 1)
    kred = LM.Kernel.KRed(fa[0], fb[0], fb[1])
    composed = float((fa[1].double() * kred.double()).sum())
    q, p = torch.cat([fa[0], fb[0]]), torch.cat([fa[1], fb[1]])
    off = [0, sizes[0], sum(sizes)]
    ref, A = GR.dense(q, p, off, [(0, 1)], sigma)
    K = torch.exp(-((fa[0].double()[:, None] - fb[0].double()[None]) ** 2).sum(-1) / (2 * sigma ** 2))
    kred64 = K @ fb[1].double()
    tol = GR.C * GR.U24 * float(A[0]) + 1e-5 * float(fa[1].double().norm()) * float(kred64.norm())
    print(f"gram {float(G[0, 0])!r} composed {composed!r} float64 {float(ref[0])!r} tol {tol:.3e}")
    assert abs(float(G[0, 0]) - composed) <= tol


# ---------------------------------------------------------------------------------------------
# end to end without fitting
@pytest.fixture(scope="module")
def atlas(dev):
    from difficp_amd.core.GMM import GaussianMixtureUnif
    from difficp_amd.core.PSR import DiffPSR
    spec = {"device": dev, "dtype": torch.float32}
    g = torch.Generator().manual_seed(11)
    K, N, D, C, S = 5, 150, 2, 30, 40
    x = [torch.rand(N, D, generator=g).to(dev) for _ in range(K)]
    GM = GaussianMixtureUnif(torch.rand(C, D, generator=g), spec=spec)
    LM = _model(dev, D, sigma=0.2)
    PS = DiffPSR(x, GM, LM, dataspec=spec, compspec=spec)
    PS.printstuff = False
    PS.set_support_scheme("custom", q0=torch.rand(S, D, generator=g))
    mean = 0.05 * torch.randn(S, D, generator=g)
    mode = 0.05 * torch.randn(S, D, generator=g)
    c = torch.tensor([-1.5, -0.25, 0.5, 1.0, 2.0])
    for k in range(K):
        PS.a0[k] = (mean + c[k] * mode).to(dev)
    return PS, c.double()


def test_tangent_pca_of_a_rank1_atlas(atlas):
    PS, c = atlas
    pca = PS.tangent_pca(side="source")
    assert pca.gram.shape == (PS.K, PS.K) and pca.L == 1
    want = c - c.mean()
    s = pca.scores[:, 0]
    s = s * (1.0 if float(s @ want) > 0 else -1.0)
    s = s * float(want.norm() / s.norm())
    assert float((s - want).norm()) <= 1e-5 * float(want.norm())
    assert float(pca.explained_variance_ratio[0]) > 1 - 1e-6
    # out of sample: a training frame's projection is its score.  On the device the new column
    # <v_j, v> is summed over other tiles than the mirrored training entry, so the two agree
    # within the kernel's tolerance only: every entry is within C 2^-24 A of the float64
    # statement, a centred entry combines four of them (the entry, two means, the grand mean), of
    # the projected column and of the training column alike, and the score weighs the centred
    # column by coefficients[:, l].
    fields = [PS.Registration(j).tangent_field("source") for j in range(PS.K)]
    q, p = torch.cat([f[0] for f in fields]), torch.cat([f[1] for f in fields])
    n = fields[0][0].shape[0]
    A = GR.dense(q, p, [j * n for j in range(PS.K + 1)], GR.all_pairs(PS.K), PS.LMi.sigma)[1]
    bound = 2 * 4 * GR.C * GR.U24 * float(A.max()) * float(pca.coefficients[:, 0].abs().sum())
    k = 3
    err = float((pca.project(fields[k]) - pca.scores[k]).abs().max())
    print(f"project(training field): error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_target_side_fields_are_the_shot_states(atlas):
    PS, _ = atlas
    for k in (0, 4):
        sh = PS.LMi.Shoot(PS.q0[k], PS.a0[k])
        q1, p1 = PS.Registration(k).tangent_field("target")
        assert torch.equal(q1, sh.Q[-1]) and torch.equal(p1, -sh.P[-1])
    pca = PS.tangent_pca()                     # the template side of diff-ICP
    assert bool(torch.isfinite(pca.gram).all()) and pca.L >= 1


def test_mode_registration_on_the_template_centres(atlas):
    """The projected mode against what a float64 ridge solve with the same alpha on the same
    inputs leaves: (K + alpha I) b = target, residual |K b - target| / |target|, doubled."""
    PS, _ = atlas
    LM = PS.LMi
    pca = PS.tangent_pca(side="source")
    mu = PS.GMMi[0].mu
    alpha = 1e-4
    reg, res = pca.mode_registration(0, 2.0, support=mu, alpha=alpha)
    assert bool(torch.isfinite(reg.apply(mu)).all())
    q, p = pca.mode_field(0, 2.0)
    target = LM.v(mu, q, p).double().cpu()
    m64 = mu.double().cpu()
    Km = torch.exp(-((m64[:, None] - m64[None]) ** 2).sum(-1) / (2 * LM.sigma ** 2))
    b = torch.linalg.solve(Km + alpha * torch.eye(len(m64), dtype=torch.float64), target)
    ridge = float((Km @ b - target).norm() / target.norm())
    print(f"mode_registration: relative residual {res:.3e}, float64 ridge {ridge:.3e}")
    assert res <= 2 * ridge
    reg_u = pca.mode_registration(0, 2.0)
    assert reg_u.q0.shape[0] == PS.K * PS.q0[0].shape[0]
