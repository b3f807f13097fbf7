"""Host side of the Gaussian cutoff, no device: the spatial order a
cutoff shooting runs in and its inverse round-trip on ties and on sizes that are no multiple of
the 64-point tile; the numpy far predicate the GPU tests rely on (tests/pair_cutoff_ref.py)
against brute-force point distances."""
import numpy as np
import pytest
import torch

import pair_cutoff_ref as PR


@pytest.mark.parametrize("M,D", [(1, 3), (63, 3), (64, 2), (65, 3), (1000, 2), (2100, 3)])
def test_order_round_trip(M, D):
    from difficp_amd.core.shooting import inverse_order, spatial_order
    g = torch.Generator().manual_seed(M + D)
    x = torch.rand(M, D, generator=g)
    x[M // 2:] = x[:M - M // 2].clone()    # ties: every point of the first half twice
    perm = spatial_order(x)
    assert perm.dtype == torch.int32 and sorted(perm.tolist()) == list(range(M))
    inv = inverse_order(perm)
    assert inv.dtype == torch.int64
    assert torch.equal(inv[perm.long()], torch.arange(M))
    xs = x.index_select(0, perm.long())
    assert torch.equal(xs.index_select(0, inv), x)          # gather in, gather back out
    # the scatter form (what an inverse order stands for) agrees
    y = torch.empty_like(x)
    y[perm.long()] = xs
    assert torch.equal(y, x)
    # stable: tied points keep their index order, so the order is reproducible
    assert torch.equal(perm, spatial_order(x.clone()))
    dup = {}
    for pos, i in enumerate(perm.tolist()):
        dup.setdefault(tuple(x[i].tolist()), []).append(i)
    assert all(v == sorted(v) for v in dup.values())


def _cloud(kind, M, D, sigma, rng):
    if kind == "clumps":
        q = 2 * sigma * rng.random((M, D))
        q[M // 2:, 0] += 12 * sigma
        return q.astype(np.float32)
    q = rng.random((M, D)).astype(np.float32)     # sorted along x: tiles are slabs
    return q[np.argsort(q[:, 0], kind="stable")]


@pytest.mark.parametrize("kind", ["clumps", "slabs"])
@pytest.mark.parametrize("M,D,G", [(300, 3, 256), (1100, 2, 384), (1600, 3, 512), (2100, 3, 256)])
def test_far_predicate_against_point_distances(kind, M, D, G):
    """A (row group, sub-tile) pair marked far has every point pair beyond the cut (so every
    K < 2^-T); an unmarked pair's boxes are within it.  T = 8 and 48 on sigma = 0.1."""
    sigma = 0.1
    q = _cloud(kind, M, D, sigma, np.random.default_rng(M))
    boxes = PR.boxes_ref(q, sigma)
    nB = (M + 63) // 64
    assert boxes.shape == (nB, 2 * D) and boxes.dtype == np.float32
    z = float(PR.alpha(sigma)) * (q.astype(np.float64) - q[0].astype(np.float64))
    # the boxes hold their points (to float32 rounding of the scaled coordinates)
    for s in range(nB):
        t = z[s * 64:(s + 1) * 64]
        assert (t >= boxes[s, :D] - 1e-5).all() and (t <= boxes[s, D:] + 1e-5).all()
    marked = 0
    for T in (8, 48):
        far = PR.far_mask(boxes, G, T)
        assert far.shape == ((M + G - 1) // G, nB)
        assert not far[~PR.off_diagonal(far.shape[0], nB, G)].any()     # a group's own tiles: gap 0
        for A in range(far.shape[0]):
            rows = z[A * G:(A + 1) * G]
            for s in range(nB):
                cols = z[s * 64:(s + 1) * 64]
                d2 = ((rows[:, None, :] - cols[None, :, :]) ** 2).sum(-1).min()
                if far[A, s]:
                    marked += 1
                    assert d2 > T * (1 - 1e-5), (A, s, d2)
    assert marked > 0


def test_far_predicate_nan_box_is_never_far():
    sigma = 0.1
    rng = np.random.default_rng(0)
    q = (2 * sigma * rng.random((300, 3))).astype(np.float32)
    q[150:, 0] += 40 * sigma
    q[200, 1] = np.nan
    boxes = PR.boxes_ref(q, sigma)
    assert np.isnan(boxes[200 // 64]).all() and np.isfinite(np.delete(boxes, 200 // 64, 0)).all()
    far = PR.far_mask(boxes, 256, 48)
    assert not far[:, 200 // 64].any()          # the NaN sub-tile as a column
    assert not far[0].any()                     # and inside row group 0 (rows 0..255)
    assert far[1, 0] and far[1, 1]              # group 1 (rows 256..299) is far from tiles 0, 1
