"""Plain float64 models of csrc/norm.hip (column statistics, record finalizes with their BatchNorm tails, bn_prepare, bn_bwd_apply,
maxpool, pool_finalize) and builders of inputs on which those kernels are EXACT in float32.

numpy only: nothing here touches a GPU, and nothing takes a tie order from a device -- every arg-max is numpy.argmax / argmin on the CPU,
which return the first occurrence.

Exactness of the built inputs.  Matrices hold small integers (|x| <= 8), scales are 0 or +-2^k (k in -2..2), shifts are multiples of 1/4
in [-1, 1], slopes are 0, 1/4 or 1.  Then y*scale, fmaf(y, scale, shift), the leaky ReLU and every partial sum of a few thousand such
values are multiples of 1/16 far below 2^24/16: float32 represents all of them, so a float32 kernel and a float64 model agree bit for bit
and equal values tie in both.
"""
import numpy as np

E32 = 2.0 ** -24                  # float32 unit roundoff: the "unit" of the derived bounds
ROW_TILE = 128                    # rows per record tile of colpartials_kernel and of the GEMM epilogues
SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def lrelu64(x, slope):
    x = f64(x)
    return np.where(x > 0, x, x * slope)


# ----------------------------------------------------------------------------- column statistics
def colstats64(X, G, slope=1.0):
    """mean and biased variance of lrelu(X, slope) over each group of G rows -> ([M/G, C], [M/G, C])"""
    f = lrelu64(X, slope)
    f = f.reshape(f.shape[0] // G, G, f.shape[1])
    mean = f.sum(1) / G
    return mean, ((f - mean[:, None, :]) ** 2).sum(1) / G


def colsum64(X, G=None, slope=1.0):
    f = lrelu64(X, slope)
    G = f.shape[0] if G is None else G
    return f.reshape(f.shape[0] // G, G, f.shape[1]).sum(1)


def n_tiles(G, tile_rows):
    return (G + tile_rows - 1) // tile_rows


def records_from_rows(X, tile_rows, mode, G=None, X1=None):
    """Per-tile records of the rows of X [groups*G, C] in float64, rounded ONCE to float32, laid out [groups*tiles][C][2]:
    mode 0: (sum, M2 about the tile's own mean);  mode 1: (sum of X, sum of X1) -- X1 None: (sum, 0)."""
    X = f64(X)
    M, C = X.shape
    G = M if G is None else G
    groups, tiles = M // G, n_tiles(G, tile_rows)

    def tiled(A):                                               # [groups, tiles, tile_rows, C], the ragged last tile padded with zeros
        P = np.zeros((groups, tiles * tile_rows, C), dtype=np.float64)
        P[:, :G] = f64(A).reshape(groups, G, C)
        return P.reshape(groups, tiles, tile_rows, C)

    live = tiled(np.ones((M, C)))                               # 1 for a real row, 0 for padding
    T = tiled(X)
    rec = np.zeros((groups, tiles, C, 2), dtype=np.float64)
    rec[..., 0] = T.sum(2)
    if mode == 0:
        mean_t = rec[..., 0] / live.sum(2)
        rec[..., 1] = (live * (T - mean_t[:, :, None, :]) ** 2).sum(2)
    elif X1 is not None:
        rec[..., 1] = tiled(X1).sum(2)
    return rec.reshape(groups * tiles, C, 2).astype(np.float32)


def merge_records64(rec, G, tile_rows, mode):
    """The exact combination of the records of each group of G rows (tile t holds n_t = min(tile_rows, G - t*tile_rows) rows):
    mode 0 -> (mean, biased var) with mean = sum_t S_t / G and M2 = sum_t M2_t + sum_t n_t (S_t/n_t - mean)^2;
    mode 1 -> (sum of the first slots, sum of the second).  Each [groups, C]."""
    rec = f64(rec)
    tiles = n_tiles(G, tile_rows)
    groups, C = rec.shape[0] // tiles, rec.shape[1]
    rec = rec.reshape(groups, tiles, C, 2)
    if mode == 1:
        return rec[..., 0].sum(1), rec[..., 1].sum(1)
    n = np.minimum(tile_rows, G - np.arange(tiles) * tile_rows).astype(np.float64)[None, :, None]
    mean = rec[..., 0].sum(1) / G
    m2 = rec[..., 1].sum(1) + (n * (rec[..., 0] / n - mean[:, None, :]) ** 2).sum(1)
    return mean, m2 / G


def stat_bounds(mean64, var64, factor=32.0):
    """The derived bounds of a float32 tile-and-merge statistic: |mean - mean64| <= factor e (|mean64| + sqrt(var64)) and
    |var - var64| <= factor e (var64 + |mean64| sqrt(var64)), e = 2^-24."""
    sd = np.sqrt(var64)
    return factor * E32 * (np.abs(mean64) + sd), factor * E32 * (var64 + np.abs(mean64) * sd)


def stat_units(mean, var, mean64, var64):
    """The two errors in units of e (|mean64| + sigma) and e (var64 + |mean64| sigma); 0 where the scale itself is 0 and the value exact."""
    bm, bv = stat_bounds(mean64, var64, 1.0)
    em, ev = np.abs(f64(mean) - mean64), np.abs(f64(var) - var64)
    with np.errstate(divide="ignore", invalid="ignore"):
        um = np.where(bm > 0, em / bm, np.where(em > 0, np.inf, 0.0))
        uv = np.where(bv > 0, ev / bv, np.where(ev > 0, np.inf, 0.0))
    return um, uv


# ----------------------------------------------------------------------------- BatchNorm bookkeeping
def bn_tail64(mean, var, gamma, beta, rm, rv, count, eps, momentum):
    """Train-mode BatchNorm from (mean, biased var) -> (scale, shift, invstd, mean, running_mean', running_var'); the running variance
    takes the unbiased var*count/(count-1) (var itself when count == 1).  gamma / beta None: 1 / 0.  rm None: no running statistics."""
    mean, var = f64(mean), f64(var)
    inv = 1.0 / np.sqrt(var + eps)
    ga = np.ones_like(mean) if gamma is None else f64(gamma)
    be = np.zeros_like(mean) if beta is None else f64(beta)
    sc = ga * inv
    rm2 = rv2 = None
    if rm is not None:
        unb = var * (count / (count - 1.0)) if count > 1 else var
        rm2 = (1.0 - momentum) * f64(rm) + momentum * mean
        rv2 = (1.0 - momentum) * f64(rv) + momentum * unb
    return sc, be - mean * sc, inv, mean, rm2, rv2


def bn_tail_bounds(mean, var, gamma, beta, rm, rv, count, eps, momentum):
    """Bounds on a float32 evaluation of bn_tail64 FROM THE SAME float32 (mean, var), e = 2^-24 per correctly rounded operation, 2e for a
    merely faithful sqrt or divide:  invstd: the sum var+eps (e, halved by the root), the root (2e), the divide (2e) -> 4.5e, taken as 5e;
    scale = gamma*invstd: one more product -> 6e;  shift = beta - mean*scale: 7e on the product, e on the difference -> 8e (|beta| +
    |mean*scale|);  running statistics: 1-momentum, the ratio count/(count-1), three products and a sum -> 6e (|old| + |new|) terms.
    -> (scale, shift, invstd, running_mean, running_var) absolute bounds."""
    sc, sh, inv, mu, _, _ = bn_tail64(mean, var, gamma, beta, None, None, count, eps, momentum)
    be = np.zeros_like(mu) if beta is None else np.abs(f64(beta))
    b_rm = b_rv = None
    if rm is not None:
        unb = f64(var) * (count / (count - 1.0)) if count > 1 else f64(var)
        b_rm = 6 * E32 * (np.abs((1.0 - momentum) * f64(rm)) + np.abs(momentum * mu))
        b_rv = 6 * E32 * (np.abs((1.0 - momentum) * f64(rv)) + np.abs(momentum * unb))
    return 6 * E32 * np.abs(sc), 8 * E32 * (be + np.abs(mu * sc)), 5 * E32 * inv, b_rm, b_rv


def bn_bwd_apply64(g, y, mean, invstd, gamma, sums, count, add=None):
    """dy = gamma*invstd*(g - S0/count - xhat*S1/count), xhat = (y - mean)*invstd, sums = [S0 | S1];  add = (g2, s): g + s[c]*g2 for g"""
    g, y, mean, invstd, sums = f64(g), f64(y), f64(mean), f64(invstd), f64(sums)
    C = g.shape[1]
    if add is not None:
        g = g + f64(add[1]) * f64(add[0])
    ga = 1.0 if gamma is None else f64(gamma)
    return ga * invstd * (g - sums[:C] / count - (y - mean) * invstd * (sums[C:] / count))


def bn_bwd_coeffs64(sums, mean, invstd, gamma, count):
    """(p, q, r) of dy = p*g + q*y + r:  p = gamma*invstd, q = -p*invstd*S1/count, r = -p*S0/count - q*mean"""
    sums, mean, invstd = f64(sums), f64(mean), f64(invstd)
    C = mean.shape[0]
    p = (1.0 if gamma is None else f64(gamma)) * invstd
    q = -(p * invstd) * (sums[C:] / count)
    return p, q, -(p * (sums[:C] / count)) - q * mean


# ----------------------------------------------------------------------------- pooling
def maxpool64(y, B, N, scale=None, shift=None, slope=1.0):
    """out[b,c] = max_n lrelu(y[b*N+n,c]*scale[c] + shift[c], slope) and the FIRST row that attains it, as global row b*N + n"""
    z = f64(y)
    if scale is not None:
        z = z * f64(scale) + f64(shift)
    z = lrelu64(z, slope).reshape(B, N, -1)
    return z.max(1), (z.argmax(1) + np.arange(B)[:, None] * N).astype(np.int64)


def pool_finalize64(pval, parg, B, rows, scale, shift, slope, group_stride=0, shapes_per_group=0, relative_rows=0):
    """The rule in the comment above pool_finalize_kernel on records pval / parg [B*tiles, C, 2] = (max, min) / (arg-max, arg-min):
    scale >= 0 takes the max record and scale < 0 the min record, tiles in ascending order and the first tile wins ties, scale == 0 gives
    row b*rows, relative_rows subtracts the first row of the shape's own pass.  scale / shift: [C], or [groups, group_stride] with
    shapes_per_group shapes per pass.  -> (pooled, argmax, yarg = the chosen record value)"""
    pval, parg = f64(pval), np.asarray(parg, dtype=np.int64)
    tiles, C = rows // ROW_TILE, pval.shape[1]
    pval, parg = pval.reshape(B, tiles, C, 2), parg.reshape(B, tiles, C, 2)
    scale, shift = f64(scale).reshape(-1), f64(shift).reshape(-1)
    pooled, arg, yarg = np.zeros((B, C)), np.zeros((B, C), dtype=np.int64), np.zeros((B, C))
    for b in range(B):
        grp = b // shapes_per_group if shapes_per_group > 0 else 0
        sc, sh = scale[grp * group_stride:grp * group_stride + C], shift[grp * group_stride:grp * group_stride + C]
        tmax, tmin = pval[b, :, :, 0].argmax(0), pval[b, :, :, 1].argmin(0)       # first tile on ties
        cols = np.arange(C)
        best = np.where(sc >= 0, pval[b, tmax, cols, 0], pval[b, tmin, cols, 1])
        a = np.where(sc >= 0, parg[b, tmax, cols, 0], parg[b, tmin, cols, 1])
        a = np.where(sc == 0, b * rows, a)
        if relative_rows:
            a = a - grp * shapes_per_group * rows
        pooled[b], arg[b], yarg[b] = lrelu64(best * sc + sh, slope), a, best
    return pooled, arg, yarg


# ----------------------------------------------------------------------------- builders of exact inputs
def seeded(tag, *ints):
    """A generator keyed by a tag and integers, the same in every process (no use of Python's salted hash)"""
    return np.random.default_rng([sum(ord(ch) * (i + 1) for i, ch in enumerate(tag))] + [int(i) for i in ints])


def int_matrix(r, M, C, lim=8):
    return r.integers(-lim, lim + 1, size=(M, C)).astype(np.float32)


def dyadic_affine(r, C, zero_at=None, positive=False):
    """scale[c] = +-2^k (either sign unless positive), shift[c] a multiple of 1/4 in [-1, 1]; scale[zero_at] = 0"""
    sc = r.choice(SCALES, size=C)
    if not positive:
        sc = sc * r.choice([-1.0, 1.0], size=C)
    if zero_at is not None and C > zero_at:
        sc[zero_at] = 0.0
    sh = r.integers(-4, 5, size=C) * 0.25
    return sc.astype(np.float32), sh.astype(np.float32)


N_PATTERNS = 6


def tie_matrix(r, B, N, C, scale=None):
    """Integer matrix [B*N, C] for maxpool whose (shape b, column c) carries tie pattern (c + b) % 6, written in the direction the
    column's scale makes the maximum (value +8 for scale >= 0, -8 for scale < 0, everything else |x| <= 7):
    0 a constant column;  1 the extreme at rows {0, N-1};  2 at row N-1 only;  3 at rows n0 and n0+1 (neighbouring row slices);
    4 at rows n0+1, n0+4, n0+16, n0+64 (a LATER row of an EARLIER slice of the 4-, 16- and 64-slice kernels: the lower row must still win);
    5 every value on the far side of zero, at least 5 away (all negative after the affine map: all tie at 0 under slope 0).
    n0 = N // 3.  Rows that do not exist in a short shape are left out."""
    y = r.integers(-7, 8, size=(B, N, C)).astype(np.float32)
    sgn = np.ones(C) if scale is None else np.where(np.asarray(scale) < 0, -1.0, 1.0)
    n0 = N // 3
    for b in range(B):
        for c in range(C):
            p, top = (c + b) % N_PATTERNS, 8.0 * sgn[c]
            if p == 0:
                y[b, :, c] = 3.0
            elif p == 1:
                y[b, [0, N - 1], c] = top
            elif p == 2:
                y[b, N - 1, c] = top
            elif p == 3:
                y[b, [n for n in (n0, n0 + 1) if n < N], c] = top
            elif p == 4:
                y[b, [n for n in (n0 + 1, n0 + 4, n0 + 16, n0 + 64) if n < N], c] = top
            else:
                y[b, :, c] = -sgn[c] * r.integers(5, 9, size=N)
    return y.reshape(B * N, C)


def hard_columns(r, G):
    """[G, 7] float32: columns drawn with (mean, sigma) = (0,1), (3,1), (1e3,1), (1e4,1), (100,1e-2), (-1e3,0.5) and one constant column
    (2.5: every partial sum of it is exact, so its variance is exactly 0)."""
    spec = ((0.0, 1.0), (3.0, 1.0), (1e3, 1.0), (1e4, 1.0), (100.0, 1e-2), (-1e3, 0.5))
    X = np.stack([m + s * r.standard_normal(G) for m, s in spec] + [np.full(G, 2.5)], axis=1)
    return X.astype(np.float32)


HARD_CONST_COL = 6
