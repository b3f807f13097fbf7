"""Direct float64 parity of the C-ABI entry points on the generic row-reduction skeleton
(csrc/common.hpp rowred_kernel / csrc/launch.hpp launch_rowred, and the M-step's LSE pass)
that are otherwise reached only through wrappers at one single-chunk shape:
dicp_gauss_red_grad_f32 (the five kinds of csrc/grad_ops.hpp, every operand pattern that
tools/kernel.py issues), GRADKSCAL / GRADLAPKSCAL, MIN_SQDIST_OTHER, dicp_radius_count_f32,
dicp_gmm_mstep_f32 and dicp_gmm_targets_f32 -- at the shapes of kernel_grads_case.SHAPES: one
row, one column, a second row block with clamped tail rows, two to twenty column chunks and
their workspace merge, a column tail shorter than an LDS tile.

Criterion of the Gaussian reductions (as tests/test_gpu_kernels.py): norm-wise
rel_err against the float64 statement of the formula (tests/fake_hip.py) <= max(1e-5, 4 x the
rel_err of the same statement run in float32).  GMM passes (as tests/test_gpu_em.py):
max(2e-5, 2 x the float32 run's own deviation).  The inputs are float32 values; that they can
expose a wrong kernel is shown in tests/test_kernel_grads_host.py.  Every comparison prints
its figures (DESIGN.md section 3 tabulates the largest per entry point)."""
import math

import pytest
import torch

import fake_hip
import kernel_grads_case as KC
from conftest import rel_err
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu

OPERANDS = ("r1", "r2", "c1", "c2", "cw")


def _lib():
    from difficp_amd import _lib
    return _lib


def _ws_bytes(kind, M, N, D):
    L = _lib()
    return int(L.lib().dicp_workspace_bytes(int(kind), int(M), int(N), int(D)))


def _assert_split_precondition(kind, M, N, D):
    """The shapes with N >= 257 columns really run more than one chunk (rowred_ws_bytes is 0
    exactly when there is one chunk), the no-split shape really runs one."""
    if N >= 257:
        assert _ws_bytes(kind, M, N, D) > 0, (kind, M, N, D)
    if (M, N) == KC.NO_SPLIT:
        assert _ws_bytes(kind, M, N, D) == 0, (kind, M, N, D)


_REFS = {}


def _refs(monkeypatch, key, fn):
    """(float64, float32) runs of the fake_hip statement fn(), computed once per key and left
    unchanged (both returned as float64 tensors)."""
    if key not in _REFS:
        with monkeypatch.context() as m:
            m.setattr(fake_hip, "_DT", torch.float64)
            r64 = fn()
            m.setattr(fake_hip, "_DT", torch.float32)
            r32 = fn()
        assert r64.dtype == torch.float64 and r32.dtype == torch.float64
        _REFS[key] = (r64, r32)
    return _REFS[key]


def _check(out, r64, r32, what, floor=1e-5, factor=4.0):
    e, e32 = rel_err(out, r64), rel_err(r32, r64)
    print(f"PARITY {what}: rel_err {e:.3e} float32-ref {e32:.3e}")
    assert torch.isfinite(out).all(), what
    assert e <= max(floor, factor * e32), f"{what}: rel_err {e:.3e} (float32 reference {e32:.3e})"
    return e


def _grad_call(dev, kind, t, pat, sigma=KC.SIGMA):
    L = _lib()
    f = lambda v: None if v is None else v.float().to(dev)
    kw = {k: f(v) for k, v in KC.pattern_kwargs(t, pat).items()}
    return L.gauss_red_grad(getattr(L, "GRAD_" + kind), f(t["x"]), f(t["y"]), sigma, **kw).cpu()


def _grad_refs(monkeypatch, kind, t, pat, D, M, N):
    L = _lib()
    k = getattr(L, "GRAD_" + kind)
    return _refs(monkeypatch, ("grad", kind, pat, D, M, N),
                 lambda: fake_hip.gauss_red_grad(k, t["x"], t["y"], KC.SIGMA, **KC.pattern_kwargs(t, pat)))


# ---- a ------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("M,N", KC.SHAPES)
def test_grad_kinds_vs_float64(dev, monkeypatch, D, M, N):
    L = _lib()
    _assert_split_precondition(L.WS_GRAD, M, N, D)
    t = KC.grad_inputs(M, N, D)
    for kind, patterns in KC.GRAD_PATTERNS.items():
        for pat in patterns:
            r64, r32 = _grad_refs(monkeypatch, kind, t, pat, D, M, N)
            out = _grad_call(dev, kind, t, pat)
            assert out.shape == (M, D)
            _check(out, r64, r32, f"grad {kind} {'+'.join(pat)} D={D} {M}x{N}")


# ---- b ------------------------------------------------------------------------------------
def test_grad_split_independent(dev, monkeypatch):
    L = _lib()
    D, M, N = 3, 600, 1300
    t = KC.grad_inputs(M, N, D)
    old = {k: L.get_option(k) for k in ("force_splits", "min_chunk")}
    outs = {}
    try:
        for name, fs, mc in (("one", 1, 0), ("two", 2, 0), ("auto", 0, 0), ("chunk64", 0, 64)):
            L.set_option("force_splits", fs)
            L.set_option("min_chunk", mc)
            assert (_ws_bytes(L.WS_GRAD, M, N, D) == 0) == (name == "one"), name
            for kind, pat in KC.FULL_PATTERN.items():
                r64, r32 = _grad_refs(monkeypatch, kind, t, pat, D, M, N)
                out = _grad_call(dev, kind, t, pat)
                _check(out, r64, r32, f"grad-split {name} {kind} D={D} {M}x{N}")
                outs[name, kind] = out
    finally:
        for k, v in old.items():
            L.set_option(k, v)
    for kind in KC.FULL_PATTERN:
        for name in ("two", "auto", "chunk64"):
            e = rel_err(outs[name, kind], outs["one", kind])
            assert e <= 1e-5, (kind, name, e)


# ---- c ------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
def test_grad_empty_sides(dev, D):
    L = _lib()
    t = KC.grad_inputs(5, 4, D)
    f = lambda v: v.float().to(dev)
    for kind in KC.GRAD_PATTERNS:
        k = getattr(L, "GRAD_" + kind)
        out = L.gauss_red_grad(k, f(t["x"]), f(t["y"][:0]), KC.SIGMA, r1=f(t["r1"]), c1=f(t["c1"][:0]))
        assert out.shape == (5, D) and torch.all(out == 0), kind
        out = L.gauss_red_grad(k, f(t["x"][:0]), f(t["y"]), KC.SIGMA, r1=f(t["r1"][:0]), c1=f(t["c1"]))
        assert out.shape == (0, D), kind


# ---- d ------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("M,N", KC.SHAPES)
def test_scal_ops_vs_float64(dev, monkeypatch, D, M, N):
    L = _lib()
    _assert_split_precondition(L.WS_RED, M, N, D)
    t = KC.scal_inputs(M, N, D)
    assert N == 1 or ((t["cw"] > 0).any() and (t["cw"] < 0).any())     # mixed sign
    f = lambda v: v.float().to(dev)
    for name in ("GRADKSCAL", "GRADLAPKSCAL"):
        op = getattr(L, name)
        r64, r32 = _refs(monkeypatch, ("scal", name, D, M, N),
                         lambda: fake_hip.gauss_red(op, t["x"], t["y"], KC.SIGMA, b=t["cw"]))
        out = L.gauss_red(op, f(t["x"]), f(t["y"]), KC.SIGMA, b=f(t["cw"])).cpu()
        assert out.shape == (M, D)
        _check(out, r64, r32, f"scal {name} D={D} {M}x{N}")


# ---- e ------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("N", [2, 257, 513, 1300])
def test_min_sqdist_other_rows(dev, D, N):
    """min_{j != i} |x_i - x_j|^2 per row, bit-exact: the exclusion is by index (raw int bits
    in a float slot of the column record), so an exact copy of a row elsewhere in the cloud --
    also in another column chunk or row block -- must give exactly 0, and distinct points never."""
    L = _lib()
    _assert_split_precondition(L.WS_RED, N, N, D)
    g = torch.Generator().manual_seed(77 * D + N)
    distinct = torch.rand(N, D, generator=g, dtype=torch.float64).float()
    x = distinct.clone()
    if N == 2:
        copies = [(1, 0)]
    else:   # row 0's copy sits in the last column chunk
        copies = [(0, N - 2), (N - 1, 1), (N // 2, 2)]
    for dst, src in copies:
        x[dst] = x[src]
    for cloud, dup in ((x, True), (distinct, False)):
        xd = cloud.to(dev)
        out = L.gauss_red(L.MIN_SQDIST_OTHER, xd, xd, 1.0).cpu()
        ref = R.MinSqDistOther(cloud)
        assert out.shape == (N,)
        assert torch.equal(out, ref), (dup, (out != ref).nonzero().flatten()[:8])
        if dup:
            for dst, src in copies:
                assert out[dst] == 0 and out[src] == 0, (dst, src)
            assert int((out == 0).sum()) == 2 * len(copies)
        else:
            assert torch.all(out > 0)


# ---- f ------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("M,N", [(513, 1), (600, 1300), (64, 5000)])
def test_radius_count_split_shapes(dev, D, M, N):
    """Counts bit-exact against the float32 torch arithmetic, for radii from no neighbour to
    a ball of a third of the unit cube's volume (counts 0 ... beyond N / 4)."""
    L = _lib()
    _assert_split_precondition(L.WS_RED, M, N, D)
    g = torch.Generator().manual_seed(13 * D + M + N)
    x = torch.rand(M, D, generator=g, dtype=torch.float64).float()
    y = torch.rand(N, D, generator=g, dtype=torch.float64).float()
    big = math.sqrt(1 / (3 * math.pi)) if D == 2 else (1 / (4 * math.pi)) ** (1 / 3)
    lo, hi = N, 0
    for Rad in (1e-4, 0.03, 0.1, big):
        ref = (R.SqDistF32(x, y) <= Rad ** 2).sum(1).float()
        out = L.radius_count(x.to(dev), y.to(dev), Rad).cpu()
        assert torch.equal(out, ref), (Rad, (out != ref).nonzero().flatten()[:8])
        lo, hi = min(lo, int(ref.min())), max(hi, int(ref.max()))
    assert lo == 0 and hi >= N / 4, (lo, hi)


@pytest.mark.parametrize("D", [2, 3])
def test_radius_count_grid_ties(dev, D):
    """A regular grid against itself with the radius equal to the spacing: every axis
    neighbour sits exactly on the threshold as far as float32 rounds it (spacing 0.1 is not
    a float32 number) -- decisions bit-identical to torch's."""
    L = _lib()
    n = 37 if D == 2 else 11                      # 1369 / 1331 points: 3 row blocks, 6 chunks
    ax = (torch.arange(n, dtype=torch.float64) * 0.1).float()
    x = torch.stack(torch.meshgrid(*([ax] * D), indexing="ij"), -1).reshape(-1, D).contiguous()
    M = x.shape[0]
    assert _ws_bytes(L.WS_RED, M, M, D) > 0
    Rad = 0.1
    ref = (R.SqDistF32(x, x) <= Rad ** 2).sum(1).float()
    assert 1 <= int(ref.min()) and int(ref.max()) <= 2 * D + 1
    xd = x.to(dev)
    out = L.radius_count(xd, xd, Rad).cpu()
    assert torch.equal(out, ref), (out != ref).nonzero().flatten()[:8]


# ---- g ------------------------------------------------------------------------------------
def _gmm_tol_check(out, r64, r32, what):
    return _check(out, r64, r32, what, floor=2e-5, factor=2.0)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("C,N,variant", [(C, N, "plain") for C, N in KC.MSTEP_SHAPES]
                         + [(600, 1300, "far"), (600, 1300, "dead")])
def test_mstep_rows_vs_float64(dev, monkeypatch, D, C, N, variant):
    """The (C, D + 1) statistics of dicp_gmm_mstep_f32 (rows = components, columns = points):
    the log-weight column and each mean column against float64.  "far": 50 components 3.0 away
    from every point -- a finite, very negative log-weight and a mean that still matches (log
    domain: no NaN, no zero mean); "dead": 20 components with w2 = -inf -- log-weight -inf (their
    mean entries are not defined by the header and not asserted), every live row as before."""
    L = _lib()
    if N >= 257:
        assert _ws_bytes(L.WS_GMM_MSTEP, N, C, D) > 0
    t = KC.gmm_inputs(N, C, D, variant)
    a = (t["X"], t["T2"], t["mu"], t["w2"])
    r64, r32 = _refs(monkeypatch, ("mstep", D, C, N, variant), lambda: fake_hip.gmm_mstep(*a, KC.SIGMA_GMM))
    f = lambda v: v.float().to(dev)
    out = L.gmm_mstep(*(f(v) for v in a), KC.SIGMA_GMM).cpu().double()
    assert out.shape == (C, D + 1)
    sp = t["special"]
    live = ~sp if variant == "dead" else torch.ones(C, dtype=torch.bool)
    if variant == "dead":
        assert torch.all(out[sp, 0] == -math.inf) and torch.all(r64[sp, 0] == -math.inf)
    what = f"mstep {variant} D={D} C={C} N={N}"
    _gmm_tol_check(out[live, 0], r64[live, 0], r32[live, 0], what + " logw")
    if (C, N) == (1, 1):
        # log sum gamma = log 1: the reference is T2's float32 rounding alone (~1e-7), so the
        # relative figure above compares rounding noise with rounding noise.  What float32 can
        # be held to here: the logit nc (|x - mu|^2 - T2 / nc) passes D + 4 roundings (1 / nc,
        # T2 / nc, D + 1 terms of the sum, the product with nc) of half an ulp of |T2| each
        bound = (D + 4) * 2.0 ** -24 * abs(float(t["T2"][0])) * math.log(2)
        assert abs(float(out[0, 0] - r64[0, 0])) <= bound, (float(out[0, 0]), float(r64[0, 0]), bound)
    for d in range(D):
        _gmm_tol_check(out[live, 1 + d], r64[live, 1 + d], r32[live, 1 + d], what + f" mean{d}")
    if variant == "far":
        assert torch.isfinite(out[sp]).all() and float(r64[sp, 0].max()) < -100.0
        for d in range(D):
            _gmm_tol_check(out[sp, 1 + d], r64[sp, 1 + d], r32[sp, 1 + d], what + f" far-mean{d}")


# ---- h ------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("N,C", KC.TARGETS_SHAPES)
def test_targets_rows_vs_float64(dev, monkeypatch, D, N, C):
    """Each of the D + 4 columns of dicp_gmm_targets_f32 (old responsibilities against new
    parameters) against float64; sum_c gamma is 1 in every row."""
    L = _lib()
    _assert_split_precondition(L.WS_GMM_TARGETS, N, C, D)
    t = KC.gmm_inputs(N, C, D)
    assert torch.isfinite(t["w2"]).all() and torch.isfinite(t["lpi_new"]).all()
    a = (t["X"], t["T2"], t["mu"], t["w2"], KC.SIGMA_GMM, t["mu_new"], t["lpi_new"])
    r64, r32 = _refs(monkeypatch, ("targets", D, N, C), lambda: fake_hip.gmm_targets(*a))
    f = lambda v: v.float().to(dev) if isinstance(v, torch.Tensor) else v
    out = L.gmm_targets(*(f(v) for v in a)).cpu().double()
    assert out.shape == (N, D + 4)
    for k in range(D + 4):
        _gmm_tol_check(out[:, k], r64[:, k], r32[:, k], f"targets D={D} N={N} C={C} col{k}")
    assert float((out[:, D + 2] - 1).abs().max()) <= 1e-5, float((out[:, D + 2] - 1).abs().max())
