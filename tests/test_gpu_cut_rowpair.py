"""The Gaussian cutoff per row pair (csrc/lddmm_sym_pk.hpp
DICP_CUT_ROWPAIR): a wave of the 4 / 6 / 8-row symmetric forward and of the 4-row packed VJP tests
each of its row pairs (128 consecutive points, two tile boxes) against a 64-column sub-tile and runs
a loop body instantiated for the active ones.

The box entries are driven as tests/test_gpu_pair_cutoff.py drives them (its _run: the first ODE
evaluation, the Euler step, the full / b = 0 / gp-only adjoint steps, boxes against boxes = NULL,
the kernels forced at small sizes).

Fixture "staircase": M points uniform in a cube of side 2 sigma, point i shifted along x by
(i // 128) s sigma, so clump k is exactly row pair k; the cloud is not sorted.  Box gaps between
clumps k apart are (k s - 2) sigma, |z'|^2 = 0.7213 (k s - 2)^2:
  s = 4: 2 apart 26 (near at T = 48), 3 apart 72 (far);
  s = 3: 1 apart 0.72 (near at T = 8), 2 apart 11.5 (far, K up to 2^-11.5).
The cases give ragged last groups for 256-, 384- and 512-row waves.
"""
import numpy as np
import pytest
import torch

import pair_cutoff_ref as PR
from oracle import torch_ref as R
from test_gpu_pair_cutoff import DT, SIG, _compact, _fields, _forced, _linf_rel, _opts, _run, _same_bits

pytestmark = pytest.mark.gpu

CASES = [(1100, 3, 4), (2100, 3, 6), (1600, 3, 8), (1100, 2, 6)]
OUTPUTS = ("v", "mG", "g", "zs0", "qn", "pn", "g1", "zs", "lq", "lp", "lq_b0", "lp_b0", "lp_gp")


def _staircase(M, D, s, seed):
    g = torch.Generator().manual_seed(seed)
    q = 2 * SIG * torch.rand(M, D, generator=g, dtype=torch.float64)
    q[:, 0] += (torch.arange(M) // 128).double() * (s * SIG)
    return q


def _mixed_cells(boxes, G, T):
    """Number of (wave of G rows, sub-tile of a later group) cells in which some but not all of
    the wave's row pairs are far, and the number in which all are."""
    rp = PR.far_mask(boxes, 128, T)
    nB, n, m = rp.shape[1], G // 128, G // 64
    mixed = whole = 0
    for A in range((nB + m - 1) // m):
        f = rp[A * n:(A + 1) * n][:, (np.arange(nB) // m) > A]
        mixed += int((f.any(0) & ~f.all(0)).sum())
        whole += int(f.all(0).sum())
    return mixed, whole


def _groups(rows):
    """Row group of the forward with `rows` rows per lane, and of the 4-row VJP."""
    return 64 * rows, 256


@pytest.mark.parametrize("M,D,rows", CASES)
def test_staircase_default_cutoff(dev, M, D, rows):
    """s = 4, T = 48: clumps three or more apart are far (|z'|^2 >= 72), so the dropped terms are
    below 2^-72 of unit-scale sums: every output within 1e-7 ||dense||_inf of the boxes = NULL run
    (the bound of test_at_the_edge_of_the_cutoff: 2^12 columns x 2^-48 x 49^2).  Both kernels'
    waves have cells with some but not all row pairs far (a condition of the fixture)."""
    q = _staircase(M, D, 4.0, M + rows)
    p, a, b, gam = _fields(M, D, M)
    with _forced(rows):
        cut = _run(dev, q, p, a, b, gam, True)
        dense = _run(dev, q, p, a, b, gam, False)
    boxes = cut["boxes"].cpu().numpy()
    assert np.array_equal(boxes.view(np.int32), PR.boxes_ref(q.float().numpy(), SIG).view(np.int32))
    for G in _groups(rows):
        mixed, whole = _mixed_cells(boxes, G, 48)
        wave = PR.far_mask(boxes, G, 48)
        print("G", G, "mixed cells", mixed, "all-far cells", whole, "wave-level far cells", int(wave.sum()))
        assert mixed > 0, G
    dev_ = {k: _linf_rel(cut[k], dense[k]) for k in OUTPUTS}
    print("cut vs dense:", dev_, "bitwise:", {k: _same_bits(cut[k], dense[k]) for k in OUTPUTS})
    for k, e in dev_.items():
        assert e <= 1e-7, (k, e)
    assert _same_bits(cut["boxes_next"], dense["boxes_next"])


@pytest.mark.parametrize("M,D,rows", CASES)
def test_staircase_run_to_run(dev, M, D, rows):
    """The same staircase run twice: bitwise equal, every output."""
    q = _staircase(M, D, 4.0, M + rows)
    p, a, b, gam = _fields(M, D, M)
    with _forced(rows):
        one = _run(dev, q, p, a, b, gam, True)
        two = _run(dev, q, p, a, b, gam, True)
    for k in one:
        assert _same_bits(one[k], two[k]), k


@pytest.mark.parametrize("M,D,rows", CASES)
def test_no_row_pair_far_is_bitwise_dense(dev, M, D, rows):
    """All points in one cube of side 2 sigma: no row pair is far from any sub-tile, every wave
    takes the all-active body, and the outputs are bitwise those of boxes = NULL."""
    q = _compact(M, D, M + rows)
    p, a, b, gam = _fields(M, D, M)
    with _forced(rows):
        cut = _run(dev, q, p, a, b, gam, True)
        dense = _run(dev, q, p, a, b, gam, False)
    assert not PR.far_mask(cut["boxes"].cpu().numpy(), 128, 48).any()
    for k in cut:
        assert _same_bits(cut[k], dense[k]), k


# ---- the partial bodies against a float64 oracle that keeps exactly the pairs a mask keeps ----
def _pair_keep(far_u, U, G, M):
    """(M, M) bool: the ordered pairs (i, j) kept when a wave (group of G rows, A = i // G) drops
    the sub-tiles of later groups B > A that far_u (row units of U points x sub-tiles) marks, and
    the pair (j, i) with them -- the symmetric kernels form both orders from one visit."""
    i = np.arange(M)
    A = i // G
    drop = far_u[(i // U)[:, None], (i // 64)[None, :]] & (A[:, None] < A[None, :])
    return ~(drop | drop.T)


class _masked_kernel:
    """oracle.torch_ref with K(x, y) multiplied by W[rows of x] (x a row slice of the cloud, y the
    whole cloud, as every reduction of LDDMM.ODE calls it); W = None is the oracle itself."""

    def __init__(self, W):
        self.W = W

    def __enter__(self):
        self.K0, W = R.K, self.W

        def K(x, y, sigma):
            k = self.K0(x, y, sigma)
            if W is None:
                return k
            r0 = x.storage_offset() // x.shape[1]
            assert y.shape[0] == W.shape[1] and r0 + x.shape[0] <= W.shape[0]
            return k * W[r0:r0 + x.shape[0]]

        R.K = K

    def __exit__(self, *exc):
        R.K = self.K0


def _oracle(dev, q, p, a, b, gam, D, W_fwd, W_bwd):
    """fp64 on dev.  The forward's outputs (v, mG, the divergence rows zs, the Euler step) over the
    pairs W_fwd keeps; the adjoint step's (full and b = 0; the gp-only step's lp is the full one's)
    over the pairs W_bwd keeps, except the divergence cotangent's gp term, which the VJP takes
    from the forward's rows zs (test_gpu_zs.py)."""
    f = lambda t: t.to(dev, torch.float64)
    q, p, a, b, gam = f(q), f(p), f(a), f(b), f(gam)
    m = R.LDDMM(SIG, D, 50.0, False, True)
    out = {}
    with torch.no_grad(), _masked_kernel(W_fwd):
        v, mG, _ = m.ODE(q, p, torch.zeros(1, dtype=q.dtype, device=dev))
        gr_f = R.GradKRed(q, q, SIG)
    out.update(v=v, mG=mG, zs0=-SIG ** 2 * gr_f, zs=-SIG ** 2 * gr_f, qn=q + DT * v, pn=p + DT * mG)
    with _masked_kernel(W_bwd):
        with torch.no_grad():
            gr_b = R.GradKRed(q, q, SIG)
        for tag, bb in (("", b), ("_b0", torch.zeros_like(b))):
            qq, pp = q.clone().requires_grad_(True), p.clone().requires_grad_(True)
            vv, mm, cc = m.ODE(qq, pp, torch.zeros(1, dtype=q.dtype, device=dev))
            Lf = (a * vv).sum() + (gam * cc).sum() + (bb * mm).sum()
            gq, gp = torch.autograd.grad(Lf, (qq, pp))
            gp = gp + gam * (gr_f - gr_b)
            out["lq" + tag], out["lp" + tag] = a + DT * gq, bb + DT * gp
    out["lp_gp"] = out["lp"]
    return {k: t.cpu() for k, t in out.items()}


PARTIAL = ("v", "mG", "zs0", "qn", "pn", "zs", "lq", "lp", "lq_b0", "lp_b0", "lp_gp")


@pytest.mark.parametrize("M,D,rows", CASES)
def test_partial_bodies_are_exact(dev, M, D, rows):
    """s = 3, pair_cutoff_log2 = 8: clumps two or more apart are far with K up to 2^-11.5, so what a
    partial body drops is far above float32 rounding.  Per output, with tau = 2 x the relative
    max-norm error of the boxes = NULL run against the unmasked fp64 oracle (the dense path, not
    the code under test): ||GPU - oracle over the pairs the row-pair mask keeps|| <= tau + 1e-7.
    The wave-level mask's oracle must differ from the row-pair one by >= 10 tau (a condition of
    the fixture; an output that misses it is not tested, but v, the Euler step's sums and one
    output of each VJP variant must remain)."""
    q = _staircase(M, D, 3.0, M + rows)
    p, a, b, gam = _fields(M, D, M)
    with _forced(rows):
        dense = _run(dev, q, p, a, b, gam, False)
        with _opts(pair_cutoff_log2=8):
            cut = _run(dev, q, p, a, b, gam, True)
    boxes = cut["boxes"].cpu().numpy()
    Gf, Gb = _groups(rows)
    for G in (Gf, Gb):
        assert _mixed_cells(boxes, G, 8)[0] > 0, G
    td = lambda W: torch.from_numpy(W).to(dev, torch.float64)
    keep = {(U, G): td(_pair_keep(PR.far_mask(boxes, U, 8), U, G, M)) for G in {Gf, Gb} for U in {128, G}}
    o_none = _oracle(dev, q, p, a, b, gam, D, None, None)
    o_rp = _oracle(dev, q, p, a, b, gam, D, keep[128, Gf], keep[128, Gb])
    o_wave = _oracle(dev, q, p, a, b, gam, D, keep[Gf, Gf], keep[Gb, Gb])
    tested = []
    for k in PARTIAL:
        tau = 2 * _linf_rel(dense[k].cpu(), o_none[k])
        sep = _linf_rel(o_wave[k], o_rp[k])
        err = _linf_rel(cut[k].cpu(), o_rp[k])
        print(k, "tau", tau, "row-pair vs wave oracle", sep, "GPU vs row-pair oracle", err,
              "GPU vs wave oracle", _linf_rel(cut[k].cpu(), o_wave[k]))
        if sep >= 10 * tau:
            tested.append(k)
            assert err <= tau + 1e-7, (k, err, tau)
    print("tested:", tested)
    assert "v" in tested, tested
    assert {"qn", "pn", "zs"} & set(tested), tested
    assert {"lq", "lp"} & set(tested) and {"lq_b0", "lp_b0"} & set(tested) and "lp_gp" in tested, tested
