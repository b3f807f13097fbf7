"""numpy reference of the Gaussian cutoff's boxes and far predicate (csrc/lddmm_sym.hpp kCutTile,
lddmm_sym_pk.hpp pair_boxes_kernel / cut_mask), shared by tests/test_pair_cutoff_host.py and
tests/test_gpu_pair_cutoff.py."""
import numpy as np

TILE = 64
LOG2E = 1.4426950408889634


def alpha(sigma):
    """The kernels' coordinate scale: K = exp(-r^2 / (2 sigma^2)) = 2^(-|alpha z|^2)."""
    return np.float32(np.sqrt(LOG2E / (2.0 * sigma * sigma)))


def boxes_ref(q, sigma):
    """(ceil(M / 64), 2 D) float32: lo then hi of every 64 consecutive points in the scaled
    coordinates alpha (q - q_0), formed in float32 as the kernels form them; a sub-tile with a
    non-finite coordinate is all NaN."""
    q = np.asarray(q, np.float32)
    M, D = q.shape
    z = (alpha(sigma) * (q - q[0])).astype(np.float32)
    nB = (M + TILE - 1) // TILE
    out = np.empty((nB, 2 * D), np.float32)
    for s in range(nB):
        t = z[s * TILE:(s + 1) * TILE]
        if np.isfinite(t).all():
            out[s, :D], out[s, D:] = t.min(0), t.max(0)
        else:
            out[s] = np.nan
    return out


def far_mask(boxes, G, T):
    """(row groups of G points, sub-tiles) bool: the sub-tile's box is farther than sqrt(T) from
    the union of the row group's sub-tile boxes, sum_d max(0, lo_r - hi_c, lo_c - hi_r)^2 > T.
    A NaN box is never far (np.min / np.maximum keep the NaN, NaN > T is False)."""
    boxes = np.asarray(boxes, np.float32)
    nB, D = boxes.shape[0], boxes.shape[1] // 2
    n = G // TILE
    nG = (nB + n - 1) // n
    far = np.zeros((nG, nB), bool)
    with np.errstate(invalid="ignore"):
        for A in range(nG):
            sub = boxes[A * n:(A + 1) * n]
            lo_r, hi_r = sub[:, :D].min(0), sub[:, D:].max(0)
            gap = np.maximum(np.maximum(lo_r - boxes[:, D:], boxes[:, :D] - hi_r), np.float32(0))
            far[A] = (gap * gap).sum(1) > np.float32(T)
    return far


def off_diagonal(nG, nB, G):
    """(nG, nB) bool: sub-tile s is not part of row group A."""
    n = G // TILE
    return (np.arange(nB)[None, :] // n) != np.arange(nG)[:, None]
