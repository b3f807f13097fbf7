"""Float64 reference of the soft transfer dicp_gmm_carry_f32 (csrc/carry.hip), computed densely
from the float32 inputs, with the tolerances its tests hold the kernel to; and a float32 torch
restatement of the kernel's arithmetic, which checks those tolerances without a GPU.

    e_ij    = bias_j - k2 |r_i - y_j|^2,   k2 = log2(e) / (2 sigma^2)
    lse_i   = log2 sum_j 2^e_ij
    out_i,f = sum_j p_ij feat_j,f,         p_ij = 2^(e_ij - lse_i)

Dense (M, N): callers keep M N <= 1.5e6.  Works on any device (the tensors' own).

Tolerances: twice the first-order bound (the project's usual factor) of
    h_ij  = 8 eps32 (|bias_j| + k2 |r_i - y_j|^2)
            the eight roundings of the difference-form logit that tests/test_gpu_assign.py counts
            (D subtractions, D products / fmas, the rounding of k2, the final fma, the bias);
    n_acc = 256 + (ceil(N / 256) + 1) + 8
            the roundings a sum goes through: the 256 sequential adds of one LDS tile (kTile =
            256), the adds of the tile sums into the chunk total and of the chunk totals in the
            merge -- ceil(chunk / 256) + S of them for S chunks, at most ceil(N / 256) + 1 (a
            chunk is at least 256 columns) -- and 8 for the rest of a term (the exponential, the
            product with the feature, the final division or logarithm);
    tol_out(i, f) = 2 [ ln2 sum_j p_ij h_ij |feat_jf - out_if| + n_acc eps32 sum_j p_ij |feat_jf| ]
    tol_lse(i)    = 2 [ sum_j p_ij h_ij + n_acc eps32 / ln2 ] + 4 eps32 |lse_i|.
"""
import collections
import math

import torch

EPS32 = float(torch.finfo(torch.float32).eps)
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
NEG_INF = float("-inf")
TILE = 256

CarryRef = collections.namedtuple("CarryRef", ["out", "lse", "p", "tol_out", "tol_lse"])


def k2_of(sigma):
    return LOG2E / (2.0 * float(sigma) ** 2)


def n_acc(N):
    return TILE + (math.ceil(N / TILE) + 1) + 8


def carry_ref(rows, cols, bias, feat, sigma, expansion=False, row_mag=None):
    """CarryRef(out (M, F), lse (M,), p (M, N), tol_out (M, F), tol_lse (M,)), all float64.
    A column with bias = -inf is dead (p = 0, its feat is not read); without a live column
    lse = -inf and out = NaN; a row with a non-finite coordinate is NaN.
    expansion / row_mag: the tolerances of a pass other than carry.hip over the same sums (the
    E-step, M-step and targets kernels): its logit may come from |r|^2 - 2 r.y + |y|^2, whose
    roundings are relative to k2 (|r_i| + |y_j|)^2 instead of k2 |r_i - y_j|^2, and may carry a
    row constant of magnitude row_mag (M,) that carry.hip leaves to its caller."""
    r, c = rows.double(), cols.double()
    M, N = r.shape[0], c.shape[0]
    f = feat.double().reshape(N, -1).clone()
    F = f.shape[1]
    b = torch.zeros(N, dtype=torch.float64, device=c.device) if bias is None else bias.double()
    dead = b == NEG_INF
    d2 = ((r[:, None, :] - c[None, :, :]) ** 2).sum(-1) * k2_of(sigma)        # (M, N)
    e = b[None, :] - d2
    e[:, dead] = NEG_INF
    f[dead] = 0.0
    if N > 0:
        mx = e.max(1).values
        mx0 = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
        s = torch.exp2(e - mx0[:, None]).sum(1)
        lse = mx0 + torch.log2(s)                      # s = 0: -inf
    else:
        lse = torch.full((M,), NEG_INF, dtype=torch.float64, device=r.device)
    empty = lse == NEG_INF
    lse0 = torch.where(empty, torch.zeros_like(lse), lse)
    p = torch.exp2(e - lse0[:, None])
    p = torch.where(empty[:, None], torch.zeros_like(p), p)
    out = p @ f
    mag = d2
    if expansion:
        mag = k2_of(sigma) * (r.norm(dim=1)[:, None] + c.norm(dim=1)[None, :]) ** 2
    if row_mag is not None:
        mag = mag + row_mag.double().abs()[:, None]
    h = 8 * EPS32 * (torch.where(dead, torch.zeros_like(b), b.abs())[None, :] + mag)
    ph = p * h
    ph[:, dead] = 0.0
    na = n_acc(N)
    tol_lse = 2 * (ph.sum(1) + na * EPS32 / LN2) + 4 * EPS32 * lse.abs()
    tol_out = torch.empty_like(out)
    for k in range(F):
        dev = (f[None, :, k] - out[:, k, None]).abs()
        tol_out[:, k] = 2 * (LN2 * (ph * dev).sum(1) + na * EPS32 * (p @ f[:, k].abs()))
    nan = float("nan")
    out = torch.where(empty[:, None], torch.full_like(out, nan), out)
    bad = ~torch.isfinite(r).all(1)
    if bool(bad.any()):
        out[bad] = nan
        lse = torch.where(bad, torch.full_like(lse, nan), lse)
    return CarryRef(out, lse, p, tol_out, tol_lse)


def check(out, lse2, ref, what=""):
    """Assert out (M, F) / lse2 (M,) against ref within its tolerances, no row excluded; rows
    the reference holds non-finite must match in kind.  Returns the worst error / tolerance of
    (out, lse) over the finite entries."""
    out, lse2 = out.double(), lse2.double()
    assert out.shape == ref.out.shape and lse2.shape == ref.lse.shape, what
    fin_l = torch.isfinite(ref.lse)
    assert torch.equal(torch.isnan(lse2), torch.isnan(ref.lse)), f"{what}: NaN pattern of lse2"
    assert torch.equal(lse2 == NEG_INF, ref.lse == NEG_INF), f"{what}: -inf pattern of lse2"
    fin_o = torch.isfinite(ref.out)
    assert torch.equal(torch.isfinite(out), fin_o), f"{what}: finite pattern of out"
    ro = rl = 0.0
    if bool(fin_l.any()):
        q = ((lse2 - ref.lse).abs() / ref.tol_lse)[fin_l]
        rl = float(q.max())
    if bool(fin_o.any()):
        q = ((out - ref.out).abs() / ref.tol_out)[fin_o]
        ro = float(q.max())
    print(f"carry {what}: worst error / tolerance out {ro:.3g} lse {rl:.3g}")
    assert rl <= 1.0, f"{what}: lse2 error / tolerance {rl}"
    assert ro <= 1.0, f"{what}: out error / tolerance {ro}"
    return ro, rl


def restate32(rows, cols, bias, feat, sigma, chunks=1):
    """The kernel's arithmetic in float32 torch ops: the difference-form logit, an integer
    per-row reference m (the floor of the first tile's largest logit, moved when a tile's sum
    reaches 2^60), sums per tile of 256 columns, then into the chunk total, `chunks` column
    chunks merged in order.  Returns (out (M, F), lse2 (M,)) float32."""
    M, D = rows.shape
    N = cols.shape[0]
    feat = feat.reshape(N, -1)
    F = feat.shape[1]
    nc = torch.tensor(-k2_of(sigma), dtype=torch.float32)
    b = torch.zeros(N) if bias is None else bias
    dead = b == NEG_INF
    fz = torch.where(dead[:, None], torch.zeros_like(feat), feat)
    noref = -3.4028234663852886e38

    def logits(j0, j1):
        d2 = torch.zeros(M, j1 - j0)
        for d in range(D):
            z = rows[:, d, None] - cols[None, j0:j1, d]
            d2 = z * z + d2
        return nc * d2 + b[None, j0:j1]

    chunk = -(-N // chunks) if N else 0
    chunk = -(-chunk // 64) * 64
    parts = []
    for j0c in range(0, N, max(chunk, 1)):
        j1c = min(j0c + chunk, N)
        m = torch.full((M,), noref)
        l = torch.zeros(M)
        acc = torch.zeros(M, F)
        for j0 in range(j0c, j1c, TILE):
            j1 = min(j0 + TILE, j1c)
            e = logits(j0, j1)
            mx = torch.nan_to_num(e, nan=NEG_INF).max(1).values
            pt = torch.exp2(e - m[:, None])
            move = (pt.sum(1) >= 2.0 ** 60) | ((j0 == j0c) & (mx > m))
            mn = torch.where(move, torch.floor(mx), m)
            sc = torch.exp2(m - mn)
            l, acc, m = l * sc, acc * sc[:, None], mn
            pt = torch.exp2(e - m[:, None])
            l = l + pt.sum(1)
            acc = acc + pt @ fz[j0:j1]
        parts.append((m, l, acc))
    m = torch.full((M,), noref)
    for pm, _, _ in parts:
        m = torch.maximum(m, pm)
    l = torch.zeros(M)
    acc = torch.zeros(M, F)
    for pm, pl, pa in parts:
        sc = torch.exp2(pm - m)
        l = l + pl * sc
        acc = acc + pa * sc[:, None]
    return acc / l[:, None], m + torch.log2(l)


def combine_halves(out0, lse0, out1, lse1):
    """The transfer over the union of two column sets from the transfers over each, in float64."""
    o0, l0, o1, l1 = out0.double(), lse0.double(), out1.double(), lse1.double()
    lse = torch.logaddexp(l0 * LN2, l1 * LN2) / LN2
    w0, w1 = torch.exp2(l0 - lse), torch.exp2(l1 - lse)
    return w0[:, None] * o0 + w1[:, None] * o1, lse
