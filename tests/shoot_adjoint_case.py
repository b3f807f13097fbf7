"""Shared cases of the shooting-adjoint parity tests (tests/test_shoot_adjoint_host.py on CPU with
the oracle-backed kernels, tests/test_gpu_shoot_adjoint.py on the device).  No GPU needed to import.

A case is a cloud q0, momenta p0, optional carried points x0 and one weight tensor W[f][t] per
trajectory slot (f in Q, P, C, X; t = 0..nt).  One loss, written once (pattern_loss), is applied to
the float64 oracle's shoot (oracle/torch_ref.py under torch autograd) and to LDDMMModel.Shoot:

    L = sum_{(f, t) in pattern} s[f, t] <W[f][t], F[t]>  (+ s[H] lam H(q0, p0))

The per-slot scale factors s come from the float64 reference alone (Reference.scale): 1 over the
norm of the p0 gradient that the slot produces on its own (the q0 / x0 gradient where the slot
does not reach p0), so every slot contributes comparably to the compared gradients whatever the
cloud -- with unit weights the last step's momentum cotangent swamps the early slots in dense
clouds and a kernel that dropped them would pass.  `conditions` asserts exactly that (the "bite"
of each slot), and that the float32 oracle's own error is far from being the operative tolerance.

The reference (float64 gradients, the same in float32, the per-slot gradients and scales) is
computed once per case and device and shared read-only (`reference`).
"""
from collections import namedtuple

import torch

from conftest import rel_err
from oracle import torch_ref as R

PATTERNS = ("ALL", "Q_ONLY", "INTERIOR", "H_ONLY", "EXPANDED", "NO_P1")
GRAD_BASE, TRAJ_BASE = 2e-5, 1e-5     # floors of the float32 parity tolerances
BITE = 100.0                          # a dropped slot moves a gradient by >= BITE x its tolerance
ORACLE32_MAX = 1e-3                   # 4 x oracle32's own error stays below this
_IDX = {"Q": 0, "P": 1, "C": 2, "X": 3}
_INPUTS = ("q0", "p0", "x0")

# cloud: "small" -- unit cube, sigma 0.25, lambda 20, momenta 0.1 (the settings of
#                   test_gpu_model.py::test_shoot_and_grad, all three models tame at M <= 400);
#                   logdet: lambda 100 (at lambda 20 the cost slots' q0 gradient under EXPANDED,
#                   whose unit weights cannot be rescaled, leaves Q[0] a bite of 52 < 100; 508 here);
#        "cube"  -- sigma 0.1; classic / hybrid: unit cube, lambda 50, momenta 0.05; logdet: the
#                   tame settings documented in test_gpu_shoot_graph.py (3 (2D) / 1.5 (3D) wide,
#                   momenta 0.01, lambda 100);
#        "clumps" -- two cubes of side 2 sigma, 30 sigma apart, the points of the two interleaved
#                   at random (so the spatial order is a real permutation), lambda 50, momenta 0.01:
#                   in the float64 oracle |P| then grows 2.1x (M = 1100, D = 2) / 1.6x (2100, 3) over
#                   the shooting and points move up to 3 / 5 sigma -- nonlinear but tame (oracle32
#                   1e-6).  At momenta 0.05 these clumps (550 points in a 2 sigma square) explode:
#                   |P| grows 2700x, the cloud from 34 to 220 sigma, every float32 rounding 10x per
#                   step, in the oracle as in every kernel variant -- nothing to compare there
Case = namedtuple("Case", "M D N nt scheme version cloud seed patterns")


def case(M, D, version, N=0, nt=4, scheme="Euler", cloud="cube", seed=0, patterns=("ALL",)):
    return Case(M, D, N, nt, scheme, version, cloud, seed, tuple(patterns))


def settings(c):
    """(sigma, lambda, momentum scale, cloud width)"""
    if c.cloud == "small":
        return 0.25, (100.0 if c.version == "logdet" else 20.0), 0.1, 1.0
    if c.cloud == "clumps":
        return 0.1, 50.0, 0.01, None
    if c.version == "logdet":
        return 0.1, 100.0, 0.01, (3.0 if c.D == 2 else 1.5)
    return 0.1, 50.0, 0.05, 1.0


def oracle_model(c):
    sig, lam, _, _ = settings(c)
    return R.LDDMM(sig, c.D, lam, c.version == "logdet", c.version != "classic", scheme=c.scheme, nt=c.nt)


def library_model(c, dev, dtype=torch.float32):
    from difficp_amd.core.LDDMM import LDDMMModel
    sig, lam, _, _ = settings(c)
    LM = LDDMMModel(sigma=sig, D=c.D, lambd=lam, version=c.version, scheme=c.scheme, nt=c.nt,
                    spec={"device": dev, "dtype": dtype})
    LM.shoot_cache = None          # every call computes (the cache test makes its own)
    return LM


def inputs(c):
    """(q0, p0, x0 or None, W) in float64 on the CPU; W[f] is the list over t of the slot weights."""
    sig, _, pscale, width = settings(c)
    g = torch.Generator().manual_seed(100003 * c.seed + 1009 * c.M + 101 * c.N + 11 * c.D + c.nt)
    if c.cloud == "clumps":
        M1 = (c.M // 2 // 64) * 64 + 40           # the clump boundary inside a 64-tile
        q0 = 2 * sig * torch.rand(c.M, c.D, generator=g, dtype=torch.float64)
        q0[M1:, 0] += 32 * sig
        q0 = q0[torch.randperm(c.M, generator=g)]
        lo, ext = q0.amin(0), q0.amax(0) - q0.amin(0)
    else:
        q0 = width * torch.rand(c.M, c.D, generator=g, dtype=torch.float64)
        lo, ext = torch.zeros(c.D, dtype=torch.float64), torch.full((c.D,), width, dtype=torch.float64)
    p0 = pscale * torch.randn(c.M, c.D, generator=g, dtype=torch.float64)
    x0 = (lo + ext * torch.rand(c.N, c.D, generator=g, dtype=torch.float64)) if c.N else None
    W = {f: [torch.randn(c.M, c.D, generator=g, dtype=torch.float64) for _ in range(c.nt + 1)] for f in "QP"}
    W["C"] = [1.0 + torch.rand(1, generator=g, dtype=torch.float64) for _ in range(c.nt + 1)]
    if c.N:
        W["X"] = [torch.randn(c.N, c.D, generator=g, dtype=torch.float64) for _ in range(c.nt + 1)]
    return q0, p0, x0, W


def slots(c):
    fams = "QPCX" if c.N else "QPC"
    return [(f, t) for f in fams for t in range(c.nt + 1)] + ["H"]


def exempt_slots(c):
    """Slots that reach no input: C[0] = 0 always, every C[t] in the classic model (no cost)."""
    return {("C", t) for t in range(c.nt + 1)} if c.version == "classic" else {("C", 0)}


def pattern_coef(c, pattern, scale):
    """{slot: coefficient} of a cotangent pattern; slots that are absent get no term at all (so
    their cotangents reach ShootFn.backward as None or as autograd's zeros, never as 0 x NaN)."""
    nt = c.nt
    if pattern in ("ALL", "NO_P1"):
        co = {s: scale[s] for s in slots(c)}
        if pattern == "NO_P1":
            del co[("P", nt)]
        return co
    if pattern == "Q_ONLY":
        return {("Q", t): scale[("Q", t)] for t in range(nt + 1)}
    if pattern == "INTERIOR":
        fams = "PCX" if c.N else "PC"
        return {(f, t): scale[(f, t)] for f in fams for t in range(1, nt)}
    if pattern == "H_ONLY":
        return {"H": 1.0}
    raise ValueError(pattern)


def pattern_loss(states, lamH, W, coef):
    """The loss of the module docstring.  states[t] = (q, p, cost[, x]) -- the oracle's shoot (a list
    of tuples) and the library's Shoot index alike; lamH = lambda H(q0, p0); W on the states'
    device and dtype."""
    L = 0.0
    for s, cf in coef.items():
        if s == "H":
            L = L + cf * lamH
        else:
            f, t = s
            L = L + cf * (W[f][t] * states[t][_IDX[f]]).sum()
    return L


def expanded_loss(Q, P, C):
    """EXPANDED: sums of the stacked outputs; autograd hands ShootFn stride-0 cotangents."""
    return Q.sum() + P.sum() + C.sum()


def _to(W, dev, dtype):
    return {f: [w.to(dev, dtype) for w in ws] for f, ws in W.items()}


class Reference:
    """Float64 and float32 oracle results of a case: trajectory (stacked Q, P, C[, X]), the gradient
    in (q0, p0, x0) of every slot on its own (float64; unit coefficient), the scales, and per pattern
    the float64 and float32 gradients.  Everything on the CPU in float64 storage, read only."""

    def __init__(self, c, dev="cpu"):
        self.case = c
        self.q0, self.p0, self.x0, self.W = inputs(c)
        m = oracle_model(c)
        ins, sh, lamH = self._shoot(m, torch.float64, dev)
        W64 = _to(self.W, dev, torch.float64)
        self.traj = self._stack(sh)
        self.slot_grad = {}
        for s in slots(c):
            L = pattern_loss(sh, lamH, W64, {s: 1.0})
            self.slot_grad[s] = self._grad(L, ins)
        self.scale = {}
        for s, g in self.slot_grad.items():
            n = float(g[1].norm()) or max(float(gi.norm()) for gi in g if gi is not None)
            self.scale[s] = 1.0 / n if n > 0 else 1.0
        self.g64, self.g32 = {}, {}
        for pat in c.patterns:
            if pat == "EXPANDED":
                Q, P, C = (torch.stack([st[k] for st in sh]) for k in range(3))
                self.g64[pat] = self._grad(expanded_loss(Q, P, C), ins)
            else:
                co = pattern_coef(c, pat, self.scale)
                self.g64[pat] = tuple(None if self.slot_grad["H"][k] is None else
                                      sum(cf * self.slot_grad[s][k] for s, cf in co.items()) for k in range(3))
        if "ALL" in c.patterns:   # the sum over slots is the gradient of the one loss
            direct = self._grad(pattern_loss(sh, lamH, W64, pattern_coef(c, "ALL", self.scale)), ins)
            for a, b in zip(direct, self.g64["ALL"]):
                assert a is None or rel_err(a, b) < 1e-12
        # EXPANDED's own slots (unit weights and coefficients), for its bite
        self.slot_grad_exp = None
        if "EXPANDED" in c.patterns:
            ones = {f: [torch.ones_like(w) for w in ws] for f, ws in W64.items()}
            self.slot_grad_exp = {(f, t): self._grad(pattern_loss(sh, lamH, ones, {(f, t): 1.0}), ins)
                                  for f in "QPC" for t in range(c.nt + 1)}
        del sh, lamH, ins
        ins, sh, lamH = self._shoot(m, torch.float32, dev)
        W32 = _to(self.W, dev, torch.float32)
        self.traj32 = self._stack(sh)
        for pat in c.patterns:
            if pat == "EXPANDED":
                Q, P, C = (torch.stack([st[k] for st in sh]) for k in range(3))
                L = expanded_loss(Q, P, C)
            else:
                L = pattern_loss(sh, lamH, W32, pattern_coef(c, pat, self.scale))
            self.g32[pat] = self._grad(L, ins)

    def _shoot(self, m, dtype, dev):
        ins = tuple(None if t is None else t.to(dev, dtype).clone().requires_grad_(True)
                    for t in (self.q0, self.p0, self.x0))
        sh = m.Shoot(*ins)
        return ins, sh, m.lam * m.Hamiltonian(ins[0], ins[1])

    @staticmethod
    def _grad(L, ins):
        live = [i for i in ins if i is not None]
        if not L.requires_grad:     # a slot that reaches no input (the cost of the classic model)
            return tuple(None if i is None else torch.zeros(i.shape, dtype=torch.float64) for i in ins)
        gs = iter(torch.autograd.grad(L, live, retain_graph=True, allow_unused=True))
        out = []
        for i in ins:
            if i is None:
                out.append(None)
                continue
            g = next(gs)
            out.append(torch.zeros(i.shape, dtype=torch.float64) if g is None else g.detach().double().cpu())
        return tuple(out)

    def _stack(self, sh):
        names = "QPCX" if self.case.N else "QPC"
        return {f: torch.stack([st[_IDX[f]] for st in sh]).detach().double().cpu() for f in names}

    def tol(self, pattern):
        """Per input the gradient tolerance max(2e-5, 4 x oracle32's rel_err) (None: no such input)."""
        return tuple(None if g is None else max(GRAD_BASE, 4 * rel_err(g32, g))
                     for g, g32 in zip(self.g64[pattern], self.g32[pattern]))

    def traj_tol(self, f):
        return max(TRAJ_BASE, 4 * rel_err(self.traj32[f], self.traj[f]))


_REF = {}


def reference(c, dev="cpu"):
    key = (c, str(dev))
    if key not in _REF:
        _REF[key] = Reference(c, dev)
    return _REF[key]


def conditions(ref):
    """The two conditions on a case, from the oracle alone; returns the measured figures
    {"bite": smallest over patterns and slots, "oracle32": largest 4 x rel_err}.

    Bite: zeroing any single slot of a pattern moves at least one compared gradient by at least
    BITE x that gradient's tolerance (relative to the gradient's norm) -- with all inputs compared,
    and again with p0 alone for the slots that reach p0 (Q[0] = q0 and X[0] = x0 do not).  Slots
    that reach no input are exactly zero in the reference and are exactly exempt_slots(case).
    Oracle32: 4 x rel_err(g32, g64) <= ORACLE32_MAX for every pattern and compared gradient."""
    c = ref.case
    dead = {s for s, g in ref.slot_grad.items() if all(gi is None or not gi.any() for gi in g)}
    assert dead == exempt_slots(c), (dead, exempt_slots(c))
    worst_bite, worst32 = float("inf"), 0.0
    for pat in c.patterns:
        g64, tol = ref.g64[pat], ref.tol(pat)
        for k, g in enumerate(g64):
            if g is not None and g.any():
                e = 4 * rel_err(ref.g32[pat][k], g)
                worst32 = max(worst32, e)
                assert e <= ORACLE32_MAX, (c, pat, _INPUTS[k], e)
        if pat == "EXPANDED":
            contrib = {s: g for s, g in ref.slot_grad_exp.items() if s not in dead}
        else:
            contrib = {s: tuple(None if gi is None else cf * gi for gi in ref.slot_grad[s])
                       for s, cf in pattern_coef(c, pat, ref.scale).items() if s not in dead}
        ts = {t for s in contrib if s != "H" for t in [s[1]]}
        if pat in ("ALL", "NO_P1", "Q_ONLY", "EXPANDED"):   # t = 0, an interior t and t = nt are there
            assert {0, c.nt} <= ts and (c.nt < 2 or any(0 < t < c.nt for t in ts)), (pat, ts)
        for s, gs in contrib.items():
            def move(k):
                n = float(g64[k].norm())
                return float(gs[k].norm()) / (n * tol[k]) if n > 0 else 0.0
            every = max(move(k) for k in range(3) if g64[k] is not None)
            assert every >= BITE, (c, pat, s, every)
            worst_bite = min(worst_bite, every)
            if gs[1].any():                                   # the p0-only form
                assert move(1) >= BITE, (c, pat, s, "p0 only", move(1))
                worst_bite = min(worst_bite, move(1))
    return {"bite": worst_bite, "oracle32": worst32}


def library_inputs(ref, dev, dtype=torch.float32, p0_only=False):
    """Fresh leaf tensors (q0, p0, x0 or None) of the case; p0_only: only p0 requires a gradient."""
    q, p, x = (None if t is None else t.to(dev, dtype).clone() for t in (ref.q0, ref.p0, ref.x0))
    p.requires_grad_(True)
    if not p0_only:
        q.requires_grad_(True)
        if x is not None:
            x.requires_grad_(True)
    return q, p, x


def run_library(ref, pattern, dev, dtype=torch.float32, p0_only=False, LM=None, tensors=None):
    """LDDMMModel.Shoot of the case's inputs (tensors: those of an earlier library_inputs), the
    pattern's loss, and its gradients.  Returns {"g": (gq, gp, gx) (None where not asked for),
    "traj": {f: stacked output}, "L": loss}, on the CPU."""
    c = ref.case
    LM = library_model(c, dev, dtype) if LM is None else LM
    q, p, x = library_inputs(ref, dev, dtype, p0_only) if tensors is None else tensors
    sh = LM.Shoot(q, p, x, need_p1=pattern != "NO_P1")
    if pattern == "EXPANDED":
        L = expanded_loss(sh.Q, sh.P, sh.C)
    else:
        L = pattern_loss(sh, LM.lam * sh.H0, _to(ref.W, dev, dtype), pattern_coef(c, pattern, ref.scale))
    want = [t for t in (q, p, x) if t is not None and t.requires_grad]
    got = iter(torch.autograd.grad(L, want, allow_unused=True))
    g = []
    for t in (q, p, x):
        if t is None or not t.requires_grad:
            g.append(None)
        else:
            gi = next(got)
            g.append(torch.zeros(t.shape, dtype=dtype) if gi is None else gi.detach().cpu())
    traj = {"Q": sh.Q, "P": sh.P, "C": sh.C}
    if c.N:
        traj["X"] = sh.X
    return {"g": tuple(g), "traj": {f: t.detach().cpu() for f, t in traj.items()}, "L": L.detach().cpu()}


def check(out, ref, pattern, p0_only=False, grad_tol=None, traj_tol=None, label=""):
    """Assert a run_library result against the float64 reference: each gradient within grad_tol
    (default: max(2e-5, 4 x oracle32)), each trajectory output within traj_tol (default: max(1e-5,
    4 x oracle32)); where the reference is identically zero the result must be exactly zero.  Every
    figure is printed before anything is asserted.  Returns {name: (rel_err, oracle32's rel_err)}."""
    c = ref.case
    rows = []
    tol = ref.tol(pattern)
    for k, name in enumerate(_INPUTS):
        g64 = ref.g64[pattern][k]
        if g64 is None or (p0_only and k != 1):
            assert out["g"][k] is None
            continue
        t = tol[k] if grad_tol is None else grad_tol
        rows.append(("g" + name, out["g"][k], g64, ref.g32[pattern][k], t))
    for f, got in out["traj"].items():
        exp, exp32 = ref.traj[f], ref.traj32[f]
        if f == "P" and pattern == "NO_P1":      # P[nt] is not formed (NaN) or not to be read
            got, exp, exp32 = got[:c.nt], exp[:c.nt], exp32[:c.nt]
        rows.append((f, got, exp, exp32, ref.traj_tol(f) if traj_tol is None else traj_tol))
    res = {}
    for name, got, exp, exp32, t in rows:
        e, e32 = rel_err(got, exp), rel_err(exp32, exp)
        res[name] = (e, e32)
        print(f"ADJ {label} M={c.M} D={c.D} N={c.N} nt={c.nt} {c.scheme} {c.version} {pattern}"
              f"{' p0-only' if p0_only else ''} {name}: rel_err {e:.3e} oracle32 {e32:.3e} tol {t:.3e}")
    for name, got, exp, exp32, t in rows:
        assert bool(torch.isfinite(got).all()), name
        if not exp.any():
            assert not got.any(), (label, pattern, name, "reference is identically zero")
        else:
            assert res[name][0] <= t, (label, pattern, name, res[name], t)
    return res


# ---- the matrix of the device test (tests/test_gpu_shoot_adjoint.py), route by route ------------
# Each shape is the smallest at which the route's kernels have their ragged and multi-block parts.
MODELS = ("classic", "hybrid", "logdet")
_AI = ("ALL", "INTERIOR")
# general route (_vjp): Ralston, Ralston with carried points, Euler with carried points
GENERAL = [case(300, 3, v, scheme="Ralston", cloud="small", patterns=_AI) for v in MODELS] \
    + [case(130, 2, v, N=300, scheme="Ralston", cloud="small", patterns=_AI) for v in MODELS] \
    + [case(300, 3, v, N=900, cloud="small", patterns=_AI) for v in MODELS]
# fused Euler route, direct: every pattern; nt = 1 (no interior slot) and nt = 2 at M = 129
FUSED = [case(129, 2, v, cloud="small", patterns=PATTERNS) for v in MODELS] \
    + [case(1100, 3, v, patterns=PATTERNS) for v in MODELS]
FUSED_NT = [case(129, 2, v, nt=1, cloud="small", patterns=("ALL", "Q_ONLY", "H_ONLY", "EXPANDED", "NO_P1"))
            for v in MODELS] + [case(129, 2, v, nt=2, cloud="small", patterns=PATTERNS) for v in MODELS]
# the symmetric kernels forced: (case, rows per lane of the forward)
SYM = [(case(2100, 3, "hybrid"), 6), (case(2100, 3, "hybrid"), 8), (case(1100, 2, "hybrid"), 4)]
# graph replay: three calls (seeds) per configuration
GRAPH_PATTERNS = ("ALL", "Q_ONLY", "H_ONLY")
GRAPH = [[case(M, D, v, seed=s, patterns=GRAPH_PATTERNS) for s in range(3)]
         for (M, D) in ((700, 2), (1100, 3)) for v in ("hybrid", "logdet")]
# cutoff route: (case, rows)
CUT = [(case(M, D, v, cloud="clumps", patterns=_AI), rows)
       for (M, D, rows) in ((2100, 3, 6), (1100, 2, 4)) for v in ("hybrid", "classic")] \
    + [(case(1100, 2, v, nt=1, cloud="clumps"), 4) for v in ("hybrid", "classic")]
RAW = FUSED[4]        # (1100, 3) hybrid
CACHE = FUSED[4]


def gpu_cases():
    """Every distinct case of the device test."""
    cs = GENERAL + FUSED + FUSED_NT + [c for c, _ in SYM] + [c for g in GRAPH for c in g] + [c for c, _ in CUT]
    return list(dict.fromkeys(cs))
