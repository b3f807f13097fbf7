"""Float64 parity of ShootFn's discrete adjoint (core/shooting.py) on the device, for every cotangent
it accepts -- on Q[t], P[t], C[t], X[t] at every t, and H0 -- and every input (q0, p0, x0), on each
of its single-device routes: the general route (_vjp: Ralston, Euler with carried points), the
fused Euler route called directly, the captured-graph route, the cutoff route and raw coordinates.

Cases, loss, weights and the float64 / float32 oracle results come from tests/shoot_adjoint_case.py
(the reference is computed once per case, on the device in float64, and shared).  The criterion is
the project's: each gradient within max(2e-5, 4 x oracle32's rel_err) of float64,
each trajectory output within max(1e-5, 4 x oracle32's rel_err); a gradient whose reference is
identically zero must be exactly zero.  Every pattern runs with all inputs requiring a gradient and
again with p0 alone (the gp-only last step), against the same reference.  Before a case is used its
two conditions are asserted (shoot_adjoint_case.conditions): every slot bites, and the float32
oracle's error is far from being the tolerance.
"""
import pytest
import torch

import shoot_adjoint_case as S

pytestmark = pytest.mark.gpu

_CHECKED = set()


def _ref(c, dev):
    ref = S.reference(c, dev)
    if c not in _CHECKED:
        S.conditions(ref)
        _CHECKED.add(c)
    return ref


def _id(c):
    if not isinstance(c, S.Case):          # rows per lane, or a pattern
        return str(c)
    return f"{c.scheme}-{c.version}-M{c.M}-D{c.D}-N{c.N}-nt{c.nt}"


def _with_patterns(cases):
    return [(c, p) for c in cases for p in c.patterns]


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
    """The symmetric forward (`rows` rows per lane) and the 4-row packed VJP at any size, as
    tests/test_gpu_pair_cutoff.py forces them."""
    return _opts(fwd_alg=5, sym_fwd_rows=rows, sym_rp=2, **kw)


class _graphs:
    """shooting._GRAPH_ON for a block, restored afterwards."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from difficp_amd.core import shooting
        self.old = shooting._GRAPH_ON
        shooting._GRAPH_ON = self.on

    def __exit__(self, *a):
        from difficp_amd.core import shooting
        shooting._GRAPH_ON = self.old


def _both_forms(ref, pattern, dev, label, **kw):
    """All inputs requiring a gradient, then p0 alone; each checked against the reference."""
    outs = []
    for p0_only in (False, True):
        out = S.run_library(ref, pattern, dev, p0_only=p0_only, **kw)
        S.check(out, ref, pattern, p0_only, label=label)
        outs.append(out)
    return outs


def _same(a, b):
    """Bitwise equality of two run_library results (gradients, trajectory, loss)."""
    for x, y in zip(a["g"], b["g"]):
        assert (x is None) == (y is None)
        assert x is None or torch.equal(x, y)
    for f in a["traj"]:
        assert torch.equal(a["traj"][f], b["traj"][f]), f
    assert torch.equal(a["L"], b["L"])


@pytest.mark.parametrize("c,pattern", _with_patterns(S.GENERAL), ids=_id)
def test_general_route(dev, c, pattern):
    """_vjp: Ralston (both stages' VJPs), Ralston and Euler with carried points (ode_ext_bwd
    accumulating into the self VJP's gq, gp; X slots weighted at every t)."""
    _both_forms(_ref(c, dev), pattern, dev, "general")


@pytest.mark.parametrize("c,pattern", _with_patterns(S.FUSED + S.FUSED_NT), ids=_id)
def test_fused_route_direct(dev, c, pattern):
    """euler_adjoint_step with addq / addp / zs, lp = None (Q_ONLY, H_ONLY), the gC suffix sums,
    stride-0 cotangents (EXPANDED), no P[nt] (NO_P1); nt = 1 (no interior slot) and 2 at M = 129."""
    with _graphs(False):
        _both_forms(_ref(c, dev), pattern, dev, "fused")


@pytest.mark.parametrize("c,rows", S.SYM, ids=_id)
def test_fused_route_symmetric_kernels(dev, c, rows):
    """The symmetric forward and the 4-row packed VJP forced: more than one 1024-row VJP block and
    more than one 1536-row forward block at M = 2100."""
    with _graphs(False), _forced(rows):
        _both_forms(_ref(c, dev), "ALL", dev, f"fused-sym{rows}")


@pytest.mark.parametrize("pattern", S.GRAPH_PATTERNS)
@pytest.mark.parametrize("cs", S.GRAPH, ids=[_id(g[0]) for g in S.GRAPH])
def test_graph_replay(dev, cs, pattern):
    """Captured-graph route: four calls on one configuration (three distinct clouds, momenta and
    weights, then the first again), so a replay that failed to copy a new input or cotangent in
    would return the previous call's gradient.  Each call meets its own float64 reference and is
    bitwise the direct route on the same inputs; captures and replays are counted."""
    from difficp_amd.core import shooting
    refs = [_ref(c, dev) for c in cs]
    LM = S.library_model(cs[0], dev)
    order = [0, 1, 2, 0]
    with _graphs(False):
        direct = [_both_forms(r, pattern, dev, "graph-direct", LM=LM) for r in refs]
    with _graphs(True):
        n0 = dict(shooting.graph_stats)
        for p0_only in (False, True):
            for i in order:
                out = S.run_library(refs[i], pattern, dev, p0_only=p0_only, LM=LM)
                S.check(out, refs[i], pattern, p0_only, label="graph")
                _same(out, direct[i][int(p0_only)])
        n1 = dict(shooting.graph_stats)
    # per form: the backward's key is new (first use direct, second captures, then replays); the
    # forward's key is shared by both forms
    assert n1["captures"] >= n0["captures"] + 2, (n0, n1)
    assert n1["replays"] >= n0["replays"] + 2 * 3 + 3, (n0, n1)


@pytest.mark.parametrize("c,rows,pattern", [(c, rows, p) for c, rows in S.CUT for p in c.patterns],
                         ids=_id)
def test_cutoff_route(dev, c, rows, pattern):
    """_cut_backward on the interleaved two-clump cloud (the spatial order is a real permutation):
    cotangents gathered into the order, gradients scattered back; q0 and p0 gradients against the
    reference in natural row order (rows in another order would differ by O(1))."""
    from difficp_amd.core.shooting import last_shoot_cut, spatial_order
    L = _lib()
    ref = _ref(c, dev)
    perm = spatial_order(ref.q0.float().to(dev)).cpu().long()
    assert not torch.equal(perm, torch.arange(c.M))
    with _forced(rows, pair_cutoff=2):
        for p0_only in (False, True):
            before = dict(L.CUT_CALLS)
            out = S.run_library(ref, pattern, dev, p0_only=p0_only)
            assert last_shoot_cut()
            assert L.CUT_CALLS["adjoint"] == before["adjoint"] + c.nt
            assert L.CUT_CALLS["fwd"] == before["fwd"] + 1
            S.check(out, ref, pattern, p0_only, label="cutoff")


def test_raw_coordinates(dev):
    """LDDMMModel.coord_mode = "raw": the packed kernels in original units, forward and adjoint."""
    c = S.RAW
    LM = S.library_model(c, dev)
    LM.coord_mode = "raw"
    with _graphs(False):
        _both_forms(_ref(c, dev), "ALL", dev, "raw", LM=LM)


def test_cache_hit_backward(dev):
    """With a shoot_cache, a second Shoot on the same tensors is a hit, and its backward gives
    bitwise the first one's gradients (which meet the reference)."""
    from difficp_amd.core.shooting import ShootCache
    c = S.CACHE
    ref = _ref(c, dev)
    LM = S.library_model(c, dev)
    LM.shoot_cache = ShootCache()
    for p0_only in (False, True):
        tensors = S.library_inputs(ref, dev, p0_only=p0_only)
        h0 = LM.shoot_cache.hits
        first = S.run_library(ref, "ALL", dev, p0_only=p0_only, LM=LM, tensors=tensors)
        assert LM.shoot_cache.hits == h0
        second = S.run_library(ref, "ALL", dev, p0_only=p0_only, LM=LM, tensors=tensors)
        assert LM.shoot_cache.hits == h0 + 1
        S.check(first, ref, "ALL", p0_only, label="cache")
        _same(second, first)
