"""The Gaussian cutoff of far tile pairs (dicp_pair_boxes_f32 and the
*_box_f32 steps, options pair_cutoff / pair_cutoff_log2).

The kernels are forced at small sizes as tests/test_gpu_fwd8.py does (fwd_alg 5, sym_fwd_rows
4 / 6 / 8 for the symmetric forward, sym_rp 2 for the 4-row packed VJP), sigma = 0.1, D = 3 and
one D = 2 case, M in {300, 1100, 1600, 2100}: a ragged last 64-tile and last group, more than
one 1024-row VJP block and more than one 1536-row forward block.

"Dense" is the same entry with boxes = NULL.  Where the cut can only drop terms that are zero in
float32 (or drops nothing) the outputs must be equal; the cases that drop representable mass
state their bound where they assert it.
"""
import numpy as np
import pytest
import torch

import pair_cutoff_ref as PR
from conftest import rel_err
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu

SIG = 0.1
SIZES = [300, 1100, 1600, 2100]
DT = 0.1


def _lib():
    from difficp_amd import _lib
    return _lib


class _opts:
    """Library options for a block, restored afterwards."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        L = _lib()
        self.old = {k: L.get_option(k) for k in self.kw}
        for k, v in self.kw.items():
            L.set_option(k, v)

    def __exit__(self, *a):
        L = _lib()
        for k, v in self.old.items():
            L.set_option(k, v)


def _forced(rows, **kw):
    return _opts(fwd_alg=5, sym_fwd_rows=rows, sym_rp=2, **kw)


def _group(rows):      # points per row group of the forward with `rows` rows per lane
    return 64 * rows


def _compact(M, D, seed):
    g = torch.Generator().manual_seed(seed)
    return 2 * SIG * torch.rand(M, D, generator=g, dtype=torch.float64)


def _clumps(M, M1, D, gap_sigma, seed):
    """Two cubes of side 2 sigma whose facing sides are gap_sigma * sigma apart along x,
    concatenated clump by clump (the first holds M1 points)."""
    g = torch.Generator().manual_seed(seed)
    q = 2 * SIG * torch.rand(M, D, generator=g, dtype=torch.float64)
    q[:M1, 0] = q[:M1, 0].clamp(max=2 * SIG)
    q[M1:, 0] += (2 + gap_sigma) * SIG
    return q


def _fields(M, D, seed, pscale=1.0):
    g = torch.Generator().manual_seed(seed + 77)
    p = pscale * torch.randn(M, D, generator=g, dtype=torch.float64)
    a = torch.randn(M, D, generator=g, dtype=torch.float64)
    b = torch.randn(M, D, generator=g, dtype=torch.float64)
    gam = torch.randn(1, generator=g, dtype=torch.float64)
    return p, a, b, gam


def _run(dev, q, p, a, b, gam, use_boxes):
    """Every output of the box entries at state (q, p): the first ODE evaluation, the Euler step
    (with the next state's boxes) and the three adjoint-step variants.  use_boxes=False passes
    boxes = NULL to the same entries."""
    L = _lib()
    f = lambda t: t.float().to(dev)
    qf, pf, af, bf, gf = f(q), f(p), f(a), f(b), f(gam)
    M, D = qf.shape
    boxes = L.pair_boxes(qf, SIG)
    bx = boxes if use_boxes else None
    out = {"boxes": boxes}
    zs0 = torch.empty(M, D, device=dev)
    v, mG, g = L.ode_self_fwd_box(qf, pf, SIG, 0.0, True, bx, zs_out=zs0)
    out.update(v=v, mG=mG, g=g, zs0=zs0)
    zs = torch.empty(M, D, device=dev)
    bn = torch.empty_like(boxes)
    qn, pn, g1 = L.euler_step(qf, pf, SIG, 0.0, DT, True, zs_out=zs, boxes=bx, boxes_out=bn)
    out.update(qn=qn, pn=pn, g1=g1, zs=zs, boxes_next=bn)
    lq, lp = L.euler_adjoint_step(qf, pf, af, bf, gf, SIG, 0.0, DT, zs=zs, boxes=bx)
    out.update(lq=lq, lp=lp)
    lq0, lp0 = L.euler_adjoint_step(qf, pf, af, None, gf, SIG, 0.0, DT, zs=zs, boxes=bx)   # b = 0
    out.update(lq_b0=lq0, lp_b0=lp0)
    _, lp1 = L.euler_adjoint_step(qf, pf, af, bf, gf, SIG, 0.0, DT, want_lq=False, zs=zs, boxes=bx)
    out.update(lp_gp=lp1)
    torch.cuda.synchronize()
    return out


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _linf_rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


CASES = [(M, 3, rows) for M in SIZES for rows in (4, 6, 8)] + [(1100, 2, 6)]


@pytest.mark.parametrize("M,D,rows", CASES)
def test_compact_cloud_is_bitwise_dense(dev, M, D, rows):
    """All points in a cube of side 2 sigma: no tile is far, so the steps with boxes are bitwise
    the steps with boxes = NULL, every output; the boxes are bitwise the numpy recomputation."""
    q = _compact(M, D, M + rows)
    p, a, b, gam = _fields(M, D, M)
    with _forced(rows):
        cut = _run(dev, q, p, a, b, gam, True)
        dense = _run(dev, q, p, a, b, gam, False)
    assert not PR.far_mask(cut["boxes"].cpu().numpy(), 256, 48).any()
    for k in cut:
        assert _same_bits(cut[k], dense[k]), k
    ref = PR.boxes_ref(q.float().numpy(), SIG)
    assert np.array_equal(cut["boxes"].cpu().numpy().view(np.int32), ref.view(np.int32))
    refn = PR.boxes_ref(cut["qn"].cpu().numpy(), SIG)
    assert np.array_equal(cut["boxes_next"].cpu().numpy().view(np.int32), refn.view(np.int32))


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("M,D,rows", CASES)
def test_two_clumps_30_sigma_apart(dev, M, D, rows, aligned):
    """K underflows to 0 across a 30 sigma gap (|z'|^2 >= 649), so skipping the far tiles changes
    no output (array_equal: a skipped 0 * x may differ from the dense path in the sign of a
    zero only).  The clump boundary is once a multiple of 64 and once inside a 64-tile; the
    straddling tile spans both clumps and must not be far from either."""
    M1 = (M // 2 // 64) * 64 + (0 if aligned else 40)
    q = _clumps(M, M1, D, 30.0, M + rows)
    p, a, b, gam = _fields(M, D, M)
    with _forced(rows):
        cut = _run(dev, q, p, a, b, gam, True)
        dense = _run(dev, q, p, a, b, gam, False)
    for k in cut:
        assert torch.equal(cut[k], dense[k]), k
    boxes = cut["boxes"].cpu().numpy()
    assert np.array_equal(boxes.view(np.int32), PR.boxes_ref(q.float().numpy(), SIG).view(np.int32))
    for G in (256, _group(rows)):
        far = PR.far_mask(boxes, G, 48)
        if not aligned:
            assert not far[:, M1 // 64].any()           # the straddling tile is never skipped
            assert not far[M1 // G].any()               # nor anything against its row group
        if aligned and M == 2100 and G == 256:
            off = PR.off_diagonal(far.shape[0], far.shape[1], G)
            frac = far[off].mean()
            assert frac > 0.40, frac                    # numpy gives 148 of 264


@pytest.mark.parametrize("M,D,rows", [(2100, 3, 6), (1100, 3, 4), (1600, 3, 8), (1100, 2, 6)])
def test_the_skip_branch_is_live(dev, M, D, rows):
    """The same clumps with a 4 sigma gap (|z'|^2 >= 11.5 between them) and pair_cutoff_log2 = 8:
    the far tiles hold K up to 2^-11.5, so the result (the outputs of a step taken together: the
    largest relative max-norm deviation over them) must differ from dense by more than 1e-4;
    with T = 48 nothing is far and the result is bitwise dense."""
    M1 = (M // 2 // 64) * 64
    q = _clumps(M, M1, D, 4.0, M + rows)
    p, a, b, gam = _fields(M, D, M)
    with _forced(rows):
        dense = _run(dev, q, p, a, b, gam, False)
        with _opts(pair_cutoff_log2=8):
            cut8 = _run(dev, q, p, a, b, gam, True)
        cut48 = _run(dev, q, p, a, b, gam, True)
    assert PR.far_mask(dense["boxes"].cpu().numpy(), 256, 8).any()
    assert not PR.far_mask(dense["boxes"].cpu().numpy(), 256, 48).any()
    fwd = {k: _linf_rel(cut8[k], dense[k]) for k in ("v", "mG", "zs0", "qn", "pn", "zs")}
    bwd = {k: _linf_rel(cut8[k], dense[k]) for k in ("lq", "lp", "lq_b0", "lp_b0", "lp_gp")}
    print("forward", fwd, "adjoint", bwd)
    assert max(fwd[k] for k in ("v", "mG", "zs0")) > 1e-4, fwd      # the first ODE evaluation
    assert fwd["zs"] > 1e-4, fwd                                     # the Euler step's own sums
    for k in ("lq", "lp_b0", "lp_gp"):                               # full, b = 0 and gp-only VJPs
        assert bwd[k] > 1e-4, (k, bwd)
    for k in dense:
        assert _same_bits(cut48[k], dense[k]), k


def _oracle_step(q, p, a, b, gam, D):
    """fp64: (v, mG, lq_next, lp_next) of the ODE and of its adjoint step with cotangents a, b, gam."""
    q = q.clone().requires_grad_(True)
    p = p.clone().requires_grad_(True)
    m = R.LDDMM(SIG, D, 50.0, False, True)
    v, mG, c = m.ODE(q, p, torch.zeros(1, dtype=q.dtype))
    Lf = (a.to(q.dtype) * v).sum() + (gam.to(q.dtype) * c).sum() + (b.to(q.dtype) * mG).sum()
    gq, gp = torch.autograd.grad(Lf, (q, p))
    return {"v": v.detach(), "mG": mG.detach(), "lq": a.to(q.dtype) + DT * gq, "lp": b.to(q.dtype) + DT * gp}


@pytest.mark.parametrize("M,D,rows", [(2100, 3, 6), (1100, 3, 4), (1600, 3, 8), (1100, 2, 6)])
def test_at_the_edge_of_the_cutoff(dev, M, D, rows):
    """Clumps whose facing box sides are a gap g apart with |z'|^2 = 48 (1 -+ 0.02), p, a, b ~ N(0, 1).
    Just inside: nothing is far, bitwise dense.  Just outside: ||cut - dense||_inf <= 1e-7
    ||dense||_inf per output -- at most 2^12 columns x 2^-48 x (1 + 48)^2 ~ 3.4e-8 on unit-scale
    inputs, against row magnitudes of order 1 or more from each row's own clump -- and the error
    against the fp64 oracle no larger than the dense path's plus that bound."""
    M1 = (M // 2 // 64) * 64
    p, a, b, gam = _fields(M, D, M)
    for side, bitwise in ((-1, True), (+1, False)):
        z2 = 48.0 * (1 + side * 0.02)
        gap_sigma = float(np.sqrt(z2)) / (float(PR.alpha(SIG)) * SIG)
        q = _clumps(M, M1, D, gap_sigma, M + rows)
        # every 64-tile's box has its facing side exactly at the gap: one point of each tile there
        q[0:M1:64, 0] = 2 * SIG
        q[M1::64, 0] = (2 + gap_sigma) * SIG
        with _forced(rows):
            cut = _run(dev, q, p, a, b, gam, True)
            dense = _run(dev, q, p, a, b, gam, False)
        far = PR.far_mask(cut["boxes"].cpu().numpy(), 256, 48)
        assert far.any() == (not bitwise)
        if bitwise:
            for k in cut:
                assert _same_bits(cut[k], dense[k]), k
            continue
        dev_ = {k: _linf_rel(cut[k], dense[k]) for k in cut if k not in ("boxes", "boxes_next")}
        print("edge, just outside:", dev_)
        for k, e in dev_.items():
            assert e <= 1e-7, (k, e)
        o64 = _oracle_step(q, p, a, b, gam, D)
        for k in ("v", "mG", "lq", "lp"):
            ec, ed = _linf_rel(cut[k].cpu(), o64[k]), _linf_rel(dense[k].cpu(), o64[k])
            print(k, "vs fp64: cut", ec, "dense", ed)
            assert ec <= ed + 1e-7, (k, ec, ed)


@pytest.mark.parametrize("rows", [4, 6, 8])
def test_nan_coordinate(dev, rows):
    """M = 300 with one NaN coordinate among two far clumps: the NaN sub-tile's box is NaN, is
    never far, and the cut path gives the dense path's NaN pattern."""
    M, D = 300, 3
    q = _clumps(M, 128, D, 30.0, 5)
    q[200, 1] = float("nan")
    p, a, b, gam = _fields(M, D, M)
    with _forced(rows):
        cut = _run(dev, q, p, a, b, gam, True)
        dense = _run(dev, q, p, a, b, gam, False)
    boxes = cut["boxes"].cpu().numpy()
    ref = PR.boxes_ref(q.float().numpy(), SIG)
    assert np.isnan(boxes[200 // 64]).all()
    assert np.array_equal(np.isnan(boxes), np.isnan(ref))
    assert np.array_equal(boxes[~np.isnan(ref)].view(np.int32), ref[~np.isnan(ref)].view(np.int32))
    for k in cut:
        if k in ("boxes", "boxes_next"):
            continue
        assert torch.equal(torch.isnan(cut[k]), torch.isnan(dense[k])), k
        assert torch.isnan(dense[k]).any(), k
        fin = ~torch.isnan(dense[k])
        assert torch.equal(cut[k][fin], dense[k][fin]), k


# ---- shooting -------------------------------------------------------------------------------
def _shoot(dev, q0, p0, mode, dtype=torch.float32, nt=4, rows=6):
    """Shoot + backward of a fixed scalar of the outputs; returns the outputs and gradients (cpu).
    mode None: the oracle (oracle/torch_ref.py under torch autograd, in dtype) on dev; otherwise
    the value of pair_cutoff, with the symmetric kernels forced (`rows` rows per lane)."""
    g = torch.Generator().manual_seed(3)
    wq = torch.randn(q0.shape, generator=g, dtype=torch.float64)
    wp = torch.randn(q0.shape, generator=g, dtype=torch.float64)
    if mode is None:
        m = R.LDDMM(SIG, q0.shape[1], 50.0, False, True, nt=nt)
        q = q0.to(dev, dtype).clone().requires_grad_(True)
        p = p0.to(dev, dtype).clone().requires_grad_(True)
        Q1, P1, C1 = m.Shoot(q, p)[-1]
        Lf = (wq.to(dev, dtype) * Q1).sum() + (wp.to(dev, dtype) * P1).sum() + C1.sum()
        gq, gp = torch.autograd.grad(Lf, (q, p))
        return {"q1": Q1.detach().cpu(), "p1": P1.detach().cpu(), "c1": C1.detach().reshape(1).cpu(),
                "gq": gq.cpu(), "gp": gp.cpu()}
    from difficp_amd.core.LDDMM import LDDMMModel
    with _forced(rows, pair_cutoff=mode):
        LM = LDDMMModel(sigma=SIG, D=q0.shape[1], lambd=50.0, version="hybrid", scheme="Euler", nt=nt,
                        spec={"device": dev, "dtype": torch.float32})
        q = q0.float().to(dev).requires_grad_(True)
        p = p0.float().to(dev).requires_grad_(True)
        sh = LM.Shoot(q, p)
        Q1, P1, C1 = sh[-1][:3]
        Lf = (wq.float().to(dev) * Q1).sum() + (wp.float().to(dev) * P1).sum() + C1.sum()
        gq, gp = torch.autograd.grad(Lf, (q, p))
        torch.cuda.synchronize()
    return {"q1": Q1.detach().cpu(), "p1": P1.detach().cpu(), "c1": C1.detach().reshape(1).cpu(),
            "gq": gq.cpu(), "gp": gp.cpu(), "Q": sh.Q.detach().cpu()}


_NT = 3
_ORACLE = {}


def _cloud(kind, M=3000, D=3):
    g = torch.Generator().manual_seed(17)
    if kind == "clumps":
        q0 = _clumps(M, 1472, D, 30.0, 9)
        q0 = q0[torch.randperm(M, generator=g)]          # natural order: the clumps interleaved
    else:                                                # unit cube, every third point twice
        q0 = torch.rand(M, D, generator=g, dtype=torch.float64)
        q0[2 * M // 3:] = q0[:M - 2 * M // 3].clone()
    p0 = 0.05 * torch.randn(M, D, generator=g, dtype=torch.float64)
    return q0, p0


def _oracle(kind, dev):
    """fp64 and fp32 oracle shootings of a cloud, computed once and shared (read only)."""
    if kind not in _ORACLE:
        q0, p0 = _cloud(kind)
        _ORACLE[kind] = (_shoot(dev, q0, p0, None, torch.float64, _NT),
                         _shoot(dev, q0, p0, None, torch.float32, _NT))
    return _ORACLE[kind]


@pytest.mark.parametrize("kind,rows", [("clumps", 6), ("clumps", 4), ("cube_dup", 8)])
def test_shooting_with_cutoff(dev, kind, rows):
    """LDDMMModel.Shoot plus backward at M = 3000 with pair_cutoff = 2 against pair_cutoff = 0, the
    symmetric forward (`rows` rows per lane) and the 4-row VJP forced, so every step runs a
    cutoff kernel: outputs in natural row order (row by row against the dense run), every
    quantity within max(1e-5, 2 x the fp32 oracle's own drift) of the fp64 oracle, two runs
    bitwise identical.  On the two-clump cloud the boxes of every state Q[t] mark far tile pairs
    for both kernels' row groups, so the skip is live along the trajectory."""
    from difficp_amd.core.shooting import spatial_order
    L = _lib()
    q0, p0 = _cloud(kind)
    before = dict(L.CUT_CALLS)
    cut = _shoot(dev, q0, p0, 2, nt=_NT, rows=rows)
    assert L.CUT_CALLS["fwd"] == before["fwd"] + 1
    assert L.CUT_CALLS["step"] == before["step"] + _NT - 1
    assert L.CUT_CALLS["adjoint"] == before["adjoint"] + _NT
    mid = dict(L.CUT_CALLS)
    dense = _shoot(dev, q0, p0, 0, nt=_NT, rows=rows)
    assert L.CUT_CALLS == mid                      # pair_cutoff = 0: the dense entries only
    cut2 = _shoot(dev, q0, p0, 2, nt=_NT, rows=rows)
    assert torch.equal(cut["Q"][0], q0.float())    # the trajectory comes back in natural order
    if kind == "clumps":
        perm = spatial_order(q0.float().to(dev)).long().cpu()
        for t in range(_NT):
            boxes = PR.boxes_ref(cut["Q"][t].index_select(0, perm).numpy(), SIG)
            for G in (256, _group(rows)):
                far = PR.far_mask(boxes, G, 48)
                upper = np.arange(far.shape[0])[:, None] < (np.arange(far.shape[1])[None, :] // (G // 64))
                assert far[upper].any(), (t, G)      # (a fifth of them at t = 0)
    o64, o32 = _oracle(kind, dev)
    for k in o64:
        assert torch.equal(cut[k], cut2[k]), k
        tol = max(1e-5, 2 * rel_err(o32[k], o64[k]))
        ec, ed = rel_err(cut[k], o64[k]), rel_err(dense[k], o64[k])
        print(kind, k, "vs fp64: cut", ec, "dense", ed, "tol", tol, "cut vs dense", rel_err(cut[k], dense[k]))
        assert ec <= tol, (k, ec, tol)
        assert ed <= tol, (k, ed, tol)
        # natural row order, row by row against the dense run: both are within tol of the fp64
        # oracle, so within 2 tol of each other (rows in another order would differ by O(1))
        assert rel_err(cut[k], dense[k]) <= 2 * tol, k


def test_automatic_rule(dev):
    """pair_cutoff = 1 (the default): a dense Euler self-shooting at eta = 0 takes the box entries
    at M = 100000 and not at M = 20000 and not at eta != 0 -- read from the entries the shooting
    calls (_lib.CUT_CALLS), not from timing.  A row-split shooting needs a process group, so for
    it (and the other clauses of the rule) the decision function the shooting calls is read."""
    import types

    from difficp_amd.core import shooting as S
    L = _lib()
    assert L.get_option("pair_cutoff") == 1 and L.get_option("pair_cutoff_log2") == 48
    g = torch.Generator().manual_seed(1)

    def calls(M, eta):
        q0 = torch.rand(M, 3, generator=g).to(dev)
        p0 = (0.01 * torch.randn(M, 3, generator=g)).to(dev)
        before = dict(L.CUT_CALLS)
        ctx = S.ManualCtx((False, True) + (False,) * 11)
        Q, P, C, H0 = S.ShootFn.forward(ctx, q0, p0, None, 0.1, eta, 2, "Euler", True)
        torch.cuda.synchronize()
        assert Q.shape == (3, M, 3) and torch.equal(Q[0], q0) and torch.equal(P[0], p0)
        return {k: L.CUT_CALLS[k] - before[k] for k in before}, ctx

    c, ctx = calls(100000, 0.0)
    assert c == {"fwd": 1, "step": 1, "adjoint": 0} and ctx.cut
    c, ctx = calls(20000, 0.0)
    assert c == {"fwd": 0, "step": 0, "adjoint": 0} and not ctx.cut
    c, ctx = calls(40000, 0.02)
    assert c == {"fwd": 0, "step": 0, "adjoint": 0} and not ctx.cut
    q0 = torch.rand(100000, 3, generator=g).to(dev)
    split = types.SimpleNamespace(rank=0, world=2)
    assert S.cut_active(q0, False, 0.0, "Euler", None, 2, False)
    assert not S.cut_active(q0, False, 0.0, "Euler", split, 2, False)
    assert not S.cut_active(q0, True, 0.0, "Euler", None, 2, False)       # external points
    assert not S.cut_active(q0, False, 0.0, "Ralston", None, 2, False)
    assert not S.cut_active(q0, False, 0.0, "Euler", None, 2, True)       # raw coordinates
    with _opts(pair_cutoff=0):
        assert not S.cut_active(q0, False, 0.0, "Euler", None, 2, False)
    with _opts(pair_cutoff=2):
        assert S.cut_active(q0[:3000], False, 0.0, "Euler", None, 2, False)


def test_options_move_the_epoch(dev):
    """pair_cutoff and pair_cutoff_log2 bump option_epoch (ShootCache misses across a change) and
    refuse values out of range."""
    L = _lib()
    for name, good, bad in (("pair_cutoff", 2, 3), ("pair_cutoff_log2", 40, 7), ("pair_cutoff_log2", 150, 151)):
        old, e0 = L.get_option(name), L.option_epoch()
        L.set_option(name, good)
        assert L.get_option(name) == good and L.option_epoch() == e0 + 1
        with pytest.raises(RuntimeError):
            L.set_option(name, bad)
        L.set_option(name, old)


def test_completed_shoot_is_a_fresh_shoot(dev):
    """At a size where the automatic rule cuts (40000 points): a need_p1=False shooting completed
    by complete_shoot equals, bitwise, a fresh full shooting (trajectory, cost, final momenta),
    as tests/test_gpu_model.py::test_optimize_final_shoot_complete asks below the rule's size."""
    from difficp_amd.core.LDDMM import LDDMMModel
    L = _lib()
    M, D = 40000, 3
    g = torch.Generator().manual_seed(5)
    q0 = torch.rand(M, D, generator=g).to(dev)
    p0 = (0.01 * torch.randn(M, D, generator=g)).to(dev)
    LM = LDDMMModel(sigma=0.1, D=D, lambd=1e3, version="hybrid", scheme="Euler", nt=4,
                    spec={"device": dev, "dtype": torch.float32})
    LM.shoot_cache = None
    before = dict(L.CUT_CALLS)
    sh = LM.Shoot(q0, p0, need_p1=False)
    assert sh.p1_missing and torch.isnan(sh.P[-1]).all()
    assert L.CUT_CALLS["fwd"] == before["fwd"] + 1          # the cutoff path
    assert sh.cut
    with _opts(pair_cutoff=0):      # the path is the shooting's own record, not the rule at completion
        LM.complete_shoot(sh)
    ref = LM.Shoot(q0, p0)
    assert torch.equal(sh.Q, ref.Q) and torch.equal(sh.P, ref.P) and torch.equal(sh.C, ref.C)
