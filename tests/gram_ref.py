"""References for the RKHS Gram kernel dicp_rkhs_gram_f32 (csrc/gram.hip):

  (a) dense(): the float64 statement, from the float32 inputs,
        out[n] = sum_{i in a} sum_{j in b} (p_i . p_j) exp(-|q_i - q_j|^2 / (2 sigma^2));
  (b) the absolute mass of each pair, A[n] = sum_ij |p_i . p_j| K_ij (returned by dense());
  (c) restate32(): the kernel's own arithmetic restated on the host in float32 -- coordinate
      differences, |z|^2 and p_i . p_j by a product and fused multiply-adds, the exponent
      nc |z|^2 in the log2 domain, one exp2 per term, the terms of a tile of TILE columns summed
      per row by one fused multiply-add each in column order -- and float64 above a tile.

rkhs_gram() has the signature of _lib.rkhs_gram and serves (a): the host tests monkeypatch it in.

Tolerance of the device result for a pair: C * 2^-24 * A[n].  C is not derived from the device:
it is twice the largest deviation of (c) from (a), in units of 2^-24 A, over the test inputs
below (fields(), every D, sigma and shift of CASES, the 55 pairs of the ragged list and the split
pair) -- twice, because v_exp_f32 and the host's exp2f may differ by an ulp each way.
tests/test_gram_host.py recomputes that deviation and asserts it stays below C / 2.
"""
import numpy as np
import torch

LOG2E = 1.4426950408889634
TILE = 256            # csrc/common.hpp kTile
CHUNK = 8 * TILE      # csrc/gram.hip kGramChunk: columns per workgroup
ROWS = 512            # csrc/gram.hip kGramRows: rows per workgroup
U24 = 2.0 ** -24

# the ragged list of the tests, and the smallest field size that splits the columns in two
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 513, 1030)
SPLIT_SIZE = CHUNK + 1
CASES = [(D, sigma) for D in (2, 3) for sigma in (0.05, 0.3, 2.0)]
SHIFTS = (0.0, 100.0)

# Largest deviation of restate32 from dense over the inputs above, in units of 2^-24 A, as
# measured on the host (test_gram_host.py::test_restatement_within_half_the_constant prints it
# per case): 9.405 at D = 3, sigma = 0.05, shift 100 (7.22 unshifted; D = 2: 1.76; sigma = 0.3:
# at most 3.97; sigma = 2: at most 0.92).  At sigma = 0.05 the exponent nc |z|^2 reaches
# hundreds, and its float32 rounding is what the small far-apart fields of the list see.
MEASURED_DEVIATION = 9.405
C = 19.0              # 2 x MEASURED_DEVIATION = 18.81, rounded up


def fields(D, shift=0.0, sizes=SIZES, seed=0):
    """(q, p, offsets): float32 clouds in the unit cube (+ shift in every coordinate), unit normal
    momenta, one field after the other."""
    g = torch.Generator().manual_seed(1000 * D + seed)
    T = sum(sizes)
    q = (torch.rand(T, D, generator=g, dtype=torch.float64) + shift).float()
    p = torch.randn(T, D, generator=g, dtype=torch.float64).float()
    offsets = [0]
    for n in sizes:
        offsets.append(offsets[-1] + n)
    return q, p, offsets


def all_pairs(F):
    return [(a, b) for a in range(F) for b in range(a, F)]


def _host(offsets, pairs):
    off = [int(o) for o in torch.as_tensor(offsets).reshape(-1).tolist()]
    pr = [(int(a), int(b)) for a, b in torch.as_tensor(pairs).reshape(-1, 2).tolist()]
    return off, pr


def dense(q, p, offsets, pairs, sigma):
    """(out, A): float64 tensors (npairs,) on q's device."""
    off, pr = _host(offsets, pairs)
    q64, p64 = q.double(), p.double()
    out = torch.zeros(len(pr), dtype=torch.float64, device=q.device)
    A = torch.zeros_like(out)
    for n, (a, b) in enumerate(pr):
        qa, pa = q64[off[a]:off[a + 1]], p64[off[a]:off[a + 1]]
        qb, pb = q64[off[b]:off[b + 1]], p64[off[b]:off[b + 1]]
        if qa.shape[0] == 0 or qb.shape[0] == 0:
            continue
        d2 = ((qa[:, None, :] - qb[None, :, :]) ** 2).sum(-1)
        t = (pa @ pb.t()) * torch.exp(-d2 / (2.0 * float(sigma) ** 2))
        out[n] = t.sum()
        A[n] = t.abs().sum()
    return out, A


def rkhs_gram(q, p, offsets, pairs, sigma):
    """Stand-in for _lib.rkhs_gram on any device: statement (a)."""
    return dense(q, p, offsets, pairs, sigma)[0]


def _fma32(a, b, c):
    """float32 fused multiply-add: the product is exact in float64; the sum is rounded to float64
    and then to float32 (a double rounding in ~2^-29 of the cases, far below what C resolves)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def restate32(q, p, offsets, pairs, sigma):
    """float64 numpy array (npairs,): the kernel's arithmetic (see the module docstring)."""
    off, pr = _host(offsets, pairs)
    qn = q.detach().cpu().numpy().astype(np.float32)
    pn = p.detach().cpu().numpy().astype(np.float32)
    D = qn.shape[1]
    nc = np.float32(-LOG2E * 0.5 * (1.0 / (float(sigma) * float(sigma))))
    dots, kers, owner = [], [], []
    for n, (a, b) in enumerate(pr):
        qa, pa = qn[off[a]:off[a + 1]], pn[off[a]:off[a + 1]]
        qb, pb = qn[off[b]:off[b + 1]], pn[off[b]:off[b + 1]]
        Ma, Mb = qa.shape[0], qb.shape[0]
        if Ma == 0 or Mb == 0:
            continue
        z = qa[:, None, 0] - qb[None, :, 0]
        d2 = z * z
        dot = pa[:, None, 0] * pb[None, :, 0]
        for d in range(1, D):
            z = qa[:, None, d] - qb[None, :, d]
            d2 = _fma32(z, z, d2)
            dot = _fma32(np.broadcast_to(pa[:, None, d], z.shape), np.broadcast_to(pb[None, :, d], z.shape), dot)
        with np.errstate(under="ignore"):
            k = np.exp2(nc * d2).astype(np.float32)
        k[k < np.float32(2.0 ** -126)] = 0          # v_exp_f32 returns no denormals
        nt = -(-Mb // TILE)
        pad = nt * TILE - Mb                         # dot = k = 0: the fma leaves the sum as it is
        dots.append(np.pad(dot, ((0, 0), (0, pad))).reshape(Ma * nt, TILE))
        kers.append(np.pad(k, ((0, 0), (0, pad))).reshape(Ma * nt, TILE))
        owner.append(np.full(Ma * nt, n))
    out = np.zeros(len(pr), dtype=np.float64)
    if not dots:
        return out
    dot, k, owner = np.concatenate(dots), np.concatenate(kers), np.concatenate(owner)
    acc = np.zeros(dot.shape[0], dtype=np.float32)
    for t in range(TILE):
        acc = _fma32(dot[:, t], k[:, t], acc)
    np.add.at(out, owner, acc.astype(np.float64))
    return out


def deviation(q, p, offsets, pairs, sigma):
    """Largest |restate32 - dense| / (2^-24 A) over the pairs with A > 0."""
    out, A = dense(q, p, offsets, pairs, sigma)
    r = restate32(q, p, offsets, pairs, sigma)
    out, A = out.cpu().numpy(), A.cpu().numpy()
    live = A > 0
    assert np.all(r[~live] == 0)
    return float(np.max(np.abs(r - out)[live] / (U24 * A[live]))) if live.any() else 0.0


def test_inputs(cases=None, shifts=None):
    """Every (D, sigma, shift, q, p, offsets, pairs) the kernel tests run: the ragged list with its
    55 unordered pairs, and the pair of two SPLIT_SIZE fields, whose columns split in two chunks."""
    for D, sigma in (CASES if cases is None else cases):
        for shift in (SHIFTS if shifts is None else shifts):
            q, p, off = fields(D, shift)
            yield D, sigma, shift, q, p, off, all_pairs(len(SIZES))
            q, p, off = fields(D, shift, sizes=(SPLIT_SIZE, SPLIT_SIZE), seed=1)
            yield D, sigma, shift, q, p, off, [(0, 1)]


test_inputs.__test__ = False    # a generator of inputs, not a test


def check(got, q, p, offsets, pairs, sigma, what=""):
    """Assert the device result `got` (npairs,) float64 within C 2^-24 A of statement (a) (formed
    in float64 on got's device), pair by pair; pairs with A = 0 (an empty field) must be exactly
    0.  Prints and returns the worst error in units of 2^-24 A."""
    got = got.detach().double()
    out, A = dense(q.to(got.device), p.to(got.device), offsets, pairs, sigma)
    assert got.shape == out.shape, what
    live = A > 0
    assert bool((got[~live] == 0).all()), f"{what}: a pair with an empty field is not 0.0"
    worst = float(((got - out).abs()[live] / (U24 * A[live])).max()) if bool(live.any()) else 0.0
    print(f"rkhs_gram {what}: worst error {worst:.3f} x 2^-24 A (tolerance {C})")
    assert worst <= C, f"{what}: error {worst} x 2^-24 A exceeds {C}"
    return worst
