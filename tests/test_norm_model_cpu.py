"""CPU: the float64 models of tests/norm_model.py against torch float64 one-liners, and the record algebra against itself."""
import numpy as np
import pytest
import torch

import norm_model as nm


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def near(a, b, rtol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= rtol * max(np.abs(b).max(), 1e-300), np.abs(a - b).max()


@pytest.mark.parametrize("G,C,slope", [(1, 3, 1.0), (5, 4, 0.25), (130, 7, 0.0), (33, 1, 0.2)])
def test_colstats_and_colsum(G, C, slope):
    X = nm.seeded("cs", G, C).standard_normal((3 * G, C)) + 0.5
    f = torch.nn.functional.leaky_relu(t64(X), slope).view(3, G, C)
    mean, var = nm.colstats64(X, G, slope)
    near(mean, f.mean(1).numpy()); near(var, f.var(1, unbiased=False).numpy(), 1e-11)
    near(nm.colsum64(X, G, slope), f.sum(1).numpy())
    near(nm.colsum64(X), t64(X).sum(0, keepdim=True).numpy())


@pytest.mark.parametrize("G,tile_rows", [(1, 1), (7, 3), (8, 3), (9, 3), (300, 128), (257, 1)])
def test_records_merge_to_the_column_statistics(G, tile_rows):
    """merge_records64(records_from_rows(X)) == colstats64(X) up to the ONE float32 rounding of each record, and exactly (1e-12) when the
    records are exact in float32 (integer rows)."""
    r = nm.seeded("rec", G, tile_rows)
    Xi = nm.int_matrix(r, 2 * G, 5)
    for mode in (0, 1):
        rec = nm.records_from_rows(Xi, tile_rows, mode, G=G, X1=Xi * 2 if mode == 1 else None)
        assert rec.dtype == np.float32 and rec.shape == (2 * nm.n_tiles(G, tile_rows), 5, 2)
        a, b = nm.merge_records64(rec, G, tile_rows, mode)
        if mode == 1:
            assert np.array_equal(a, nm.colsum64(Xi, G)) and np.array_equal(b, 2 * nm.colsum64(Xi, G))
    X = (r.standard_normal((2 * G, 5)) + 3.0).astype(np.float32)
    mean, var = nm.merge_records64(nm.records_from_rows(X, tile_rows, 0, G=G), G, tile_rows, 0)
    m64, v64 = nm.colstats64(X, G)
    bm, bv = nm.stat_bounds(m64, v64, 2.0)                      # one rounding of every sum (e |mean|) and of every M2 (e var)
    assert (np.abs(mean - m64) <= bm).all() and (np.abs(var - v64) <= bv).all()
    if tile_rows == 1:
        assert (nm.records_from_rows(X, 1, 0, G=G)[..., 1] == 0).all()


def test_naive_variance_fails_the_bound_the_merge_passes():
    """The property the bound of the GPU tests exists for, shown on the CPU in float32: tile-and-merge stays inside 32 units on the hard
    columns, E[x^2] - mean^2 leaves it by orders of magnitude where |mean| >> sigma."""
    G = 4173
    X = nm.hard_columns(nm.seeded("hard", G), G)
    m64, v64 = nm.colstats64(X, G)
    assert v64[0, nm.HARD_CONST_COL] == 0.0
    rec = nm.records_from_rows(X, 128, 0)
    n = np.minimum(128, G - np.arange(rec.shape[0]) * 128).astype(np.float32)
    cnt, a, b = np.float32(0), np.zeros(7, np.float32), np.zeros(7, np.float32)
    for t in range(rec.shape[0]):                                # Chan merges in float32, tile after tile
        nn = cnt + n[t]
        d = rec[t, :, 0] / n[t] - a
        a = a + d * (n[t] / nn)
        b = b + rec[t, :, 1] + d * d * (cnt * n[t] / nn)
        cnt = nn
    um, uv = nm.stat_units(a[None], (b / np.float32(G))[None], m64, v64)
    assert um.max() <= 32 and uv.max() <= 32, (um, uv)
    x = X.astype(np.float32)
    naive = (x * x).sum(0, dtype=np.float32) / np.float32(G) - (x.sum(0, dtype=np.float32) / np.float32(G)) ** 2
    _, un = nm.stat_units(a[None], naive[None], m64, v64)
    assert un[0, 2] > 32 and un[0, 3] > 32 and un[0, 5] > 32, un


@pytest.mark.parametrize("count,momentum,affine,running", [(1, 0.1, True, True), (640, 0.1, True, True), (5, 1.0, False, True), (7, 0.3, True, False)])
def test_bn_tail(count, momentum, affine, running):
    C, eps = 6, 1e-5
    r = nm.seeded("tail", count)
    x = t64(r.standard_normal((count, C)) * 2 + 0.5)
    gamma, beta = (r.standard_normal(C), r.standard_normal(C)) if affine else (None, None)
    rm, rv = (r.standard_normal(C), r.random(C) + 0.5) if running else (None, None)
    mean, var = x.mean(0).numpy(), x.var(0, unbiased=False).numpy()
    sc, sh, inv, mu, rm2, rv2 = nm.bn_tail64(mean, var, gamma, beta, rm, rv, count, eps, momentum)
    trm, trv = (t64(rm).clone(), t64(rv).clone()) if running else (None, None)
    if count > 1:
        out = torch.nn.functional.batch_norm(x, trm, trv, None if gamma is None else t64(gamma), None if beta is None else t64(beta),
                                             True, momentum, eps)
        near(x.numpy() * sc + sh, out.numpy(), 1e-10)
        if running:
            near(rm2, trm.numpy()); near(rv2, trv.numpy(), 1e-11)
    elif running:                                                # count == 1: torch refuses; the running variance takes var (0) itself
        near(rm2, (1 - momentum) * rm + momentum * mean); near(rv2, (1 - momentum) * rv)
    near(inv, 1.0 / np.sqrt(var + eps)); assert mu is not None and np.array_equal(mu, mean)
    if not running:
        assert rm2 is None and rv2 is None


@pytest.mark.parametrize("M,C,affine", [(1, 4, True), (3, 8, False), (65, 7, True)])
def test_bn_backward_models_against_autograd(M, C, affine):
    eps = 1e-5
    r = nm.seeded("bwd", M, C)
    y = t64(r.standard_normal((max(M, 2), C)) * 2 + 0.3).requires_grad_(True)
    M = y.shape[0]
    g = t64(r.standard_normal((M, C)))
    gamma = t64(r.standard_normal(C)) if affine else None
    out = torch.nn.functional.batch_norm(y, None, None, gamma, None, True, 0.1, eps)
    (dy,) = torch.autograd.grad((out * g).sum(), y)
    yd = y.detach()
    mean, inv = yd.mean(0), 1.0 / torch.sqrt(yd.var(0, unbiased=False) + eps)
    sums = torch.cat([g.sum(0), (g * (yd - mean) * inv).sum(0)]).numpy()
    ga = None if gamma is None else gamma.numpy()
    got = nm.bn_bwd_apply64(g.numpy(), yd.numpy(), mean.numpy(), inv.numpy(), ga, sums, M)
    near(got, dy.numpy(), 1e-9)
    p, q, rr = nm.bn_bwd_coeffs64(sums, mean.numpy(), inv.numpy(), ga, M)
    near(p * g.numpy() + q * yd.numpy() + rr, dy.numpy(), 1e-9)
    g2, s = r.standard_normal((M, C)), r.standard_normal(C)
    near(nm.bn_bwd_apply64(g.numpy(), yd.numpy(), mean.numpy(), inv.numpy(), ga, sums, M, add=(g2, s)),
         nm.bn_bwd_apply64(g.numpy() + s * g2, yd.numpy(), mean.numpy(), inv.numpy(), ga, sums, M))


@pytest.mark.parametrize("B,N,C,slope,affine", [(1, 1, 1, 1.0, False), (3, 17, 5, 0.25, True), (2, 130, 12, 0.0, True)])
def test_maxpool_and_first_row(B, N, C, slope, affine):
    r = nm.seeded("mp", B, N, C)
    sc, sh = nm.dyadic_affine(r, C, zero_at=2) if affine else (None, None)
    y = nm.tie_matrix(r, B, N, C, sc)
    assert np.abs(y).max() <= 8 and (y == np.round(y)).all()
    val, arg = nm.maxpool64(y, B, N, sc, sh, slope)
    z = t64(y) if sc is None else t64(y) * t64(sc) + t64(sh)
    z = torch.nn.functional.leaky_relu(z, slope).view(B, N, C)
    assert np.array_equal(val, z.max(1)[0].numpy())
    zn = z.numpy()
    for b in range(B):
        for c in range(C):
            first = next(n for n in range(N) if zn[b, n, c] == val[b, c])      # the rule itself, spelled out
            assert arg[b, c] == b * N + first
            if sc is not None and sc[c] == 0:
                assert first == 0
    z32 = y if sc is None else y * sc + sh                                      # the built inputs are exact in float32
    z32 = np.where(z32 > 0, z32, z32 * np.float32(slope)).astype(np.float32)
    assert z32.dtype == np.float32 and np.array_equal(z32.astype(np.float64).reshape(B, N, C), zn)


def test_tie_matrix_patterns():
    r = nm.seeded("tm")
    B, N, C = 2, 200, 12
    sc, _ = nm.dyadic_affine(r, C)
    y = nm.tie_matrix(r, B, N, C, sc).reshape(B, N, C)
    n0 = N // 3
    for b in range(B):
        for c in range(C):
            p, col, top = (c + b) % 6, y[b, :, c], 8.0 * (-1 if sc[c] < 0 else 1)
            where = list(np.nonzero(col == top)[0])
            if p == 0:
                assert (col == 3).all()
            elif p == 5:
                assert (col * top < 0).all() and np.abs(col).min() >= 5
            else:
                assert where == {1: [0, N - 1], 2: [N - 1], 3: [n0, n0 + 1], 4: [n0 + 1, n0 + 4, n0 + 16, n0 + 64]}[p]


@pytest.mark.parametrize("C,spg,rel", [(1, 0, 0), (5, 1, 1), (5, 3, 0), (4, 3, 1)])
def test_pool_finalize_rule(C, spg, rel):
    B, rows, tiles = 3, 384, 3
    r = nm.seeded("pf", C, spg, rel)
    groups = B // spg if spg else 1
    stride = C + 3 if spg else 0
    sc = np.zeros((groups, max(stride, C)), np.float32); sh = np.zeros_like(sc)
    for g in range(groups):
        sc[g, :C], sh[g, :C] = nm.dyadic_affine(r, C, zero_at=1)
    pval = r.integers(-8, 9, size=(B * tiles, C, 2)).astype(np.float32)
    pval[..., 0], pval[..., 1] = pval.max(-1), pval.min(-1)
    pval = pval.reshape(B, tiles, C, 2); pval[:, 2] = pval[:, 0]; pval = pval.reshape(B * tiles, C, 2)      # tiles 0 and 2 tie
    parg = (np.arange(B * tiles)[:, None, None] * 128 + r.integers(0, 128, size=(B * tiles, C, 2))).astype(np.int32)
    pooled, arg, yarg = nm.pool_finalize64(pval, parg, B, rows, sc, sh, 0.25, stride, spg, rel)
    for b in range(B):
        grp = b // spg if spg else 0
        for c in range(C):
            s = sc[grp, c]
            vals = pval.reshape(B, tiles, C, 2)[b, :, c, 0 if s >= 0 else 1]
            best = vals.max() if s >= 0 else vals.min()
            t = next(t for t in range(tiles) if vals[t] == best)
            assert t != 2
            want = b * rows if s == 0 else parg.reshape(B, tiles, C, 2)[b, t, c, 0 if s >= 0 else 1]
            assert arg[b, c] == want - (grp * spg * rows if rel else 0)
            z = best * s + sh[grp, c]
            assert yarg[b, c] == best and pooled[b, c] == (z if z > 0 else 0.25 * z)
