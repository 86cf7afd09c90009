"""GPU: csrc/norm.hip (column reductions, record finalizes with their BatchNorm tails, bn_prepare, bn_bwd_apply, maxpool, pool_finalize)
and the pooling records of the GEMM epilogues, at the sizes where their loops and dispatches change, against the float64 models of
tests/norm_model.py.

Expectations are exact (torch.equal) wherever the inputs are built so that float32 is exact: small-integer matrices and records, dyadic
scales and shifts (norm_model's module docstring).  No expectation takes a tie order from a device: every arg-max is numpy's on the CPU.
The tolerances that remain:
  * statistics: |var - var64| <= 32 e (var64 + |mean64| sigma64) and |mean - mean64| <= 32 e (|mean64| + sigma64), e = 2^-24
    (norm_model.stat_bounds: a float32 tile-and-merge emulation stays below 4.5 and 2 units, E[x^2] - mean^2 reaches 4e3..8e4 units on the
    columns with |mean| >= 1e3 sigma -- tests/test_norm_model_cpu.py shows both on the CPU);
  * BatchNorm tails against bn_tail64 evaluated FROM THE KERNEL'S OWN float32 (mean, var): 5e..8e relative to the terms of each expression,
    counted operation by operation in norm_model.bn_tail_bounds;
  * bn_bwd_apply: rel-L2 <= 1e-5;  the coefficient vectors p, q, r: rel-L2 <= 1e-6.
Every case is at most a few hundred kilobytes; the measured worst figures are printed (pytest -s) and recorded in the docstrings."""
import numpy as np
import pytest
import torch

import norm_model as nm

pytestmark = pytest.mark.gpu

EPS = 1e-5


@pytest.fixture(scope="module")
def ops():
    from spgan import ops as o
    from spgan import _lib
    _lib.load()
    return o


@pytest.fixture(scope="module")
def lib():
    from spgan import _lib
    return _lib.load()


def cu(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def host(t):
    return None if t is None else t.detach().cpu().double().numpy()


def P(t):
    return None if t is None else t.data_ptr()


def S():
    return torch.cuda.current_stream().cuda_stream


def ok(status, what):
    assert status == 0, "%s returned status %d" % (what, status)


def same(t, want, what=""):
    """bit-for-bit (as values: float32 read into float64 is exact) against a float64 / integer numpy expectation"""
    got = t.detach().cpu().numpy()
    assert got.shape == np.shape(want), (what, got.shape, np.shape(want))
    bad = got.astype(np.float64) != np.asarray(want, dtype=np.float64)
    assert not bad.any(), "%s: %d of %d differ, first at %s: got %r want %r" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0], got[tuple(np.argwhere(bad)[0])], np.asarray(want)[tuple(np.argwhere(bad)[0])])


def within(t, want, bound, what=""):
    err = np.abs(host(t) - want)
    assert (err <= bound).all(), "%s: worst error / bound = %.3g" % (what, (err / np.maximum(bound, 1e-300)).max())
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(bound > 0, err / bound, 0.0).max())


def stats_within(mean, var, m64, v64, what):
    """the derived statistics bound (32 units) -> the measured (mean units, var units)"""
    um, uv = nm.stat_units(host(mean), host(var), m64, v64)
    assert um.max() <= 32 and uv.max() <= 32, "%s: mean %.3g units, var %.3g units (bound 32)" % (what, um.max(), uv.max())
    return float(um.max()), float(uv.max())


def rel_l2(t, want):
    return float(np.linalg.norm(host(t) - want) / max(np.linalg.norm(want), 1e-300))


# ============================================================================= a. row-slice reductions
# colpartials_kernel: 4 row slices (rows sl, sl+4, ...), the 8-in-flight loop `r + 28 < cnt` (stride 32) and the remainder loop.
#   G = 1..5: fewer rows than slices / one row per slice / a second row for slice 0;  28, 29: the loop bound for slice 0 (r = 0: 28 < cnt);
#   32, 33: one full round, one full round plus a remainder row;  61, 64, 65: the second round's bound (32 + 28 < cnt);  127, 128: the
#   largest single tile.  All of these take the ONE-launch route (tiles per group == 1: colpartials writes the group's result itself).
ONE_LAUNCH_G = [1, 2, 3, 4, 5, 28, 29, 32, 33, 61, 64, 65, 127, 128]
# two launches (colpartials + colfinalize) with a ragged last tile of 1, 127, 128 (none: 256), 1 and 1 rows over 2, 2, 2, 3 and 4 tiles
TWO_LAUNCH_G = [129, 255, 256, 257, 385]
# 64 columns per workgroup: one column, a ragged block, a full one, one column into the second block, three blocks
RED_C = [1, 63, 64, 65, 130]


def _check_reductions(ops, X, Xc, G, what):
    same(ops.colsum(Xc, G), nm.colsum64(X, G), what + " colsum")
    worst = (0.0, 0.0)
    for slope in (1.0, 0.25, 0.0):
        mean, var = ops.colstats(Xc, G, slope)
        m64, v64 = nm.colstats64(X, G, slope)
        if G <= 128:                                            # exact sum, one correctly rounded divide: pins the count
            s = nm.colsum64(X, G, slope).astype(np.float32)
            assert (s.astype(np.float64) == nm.colsum64(X, G, slope)).all()
            same(mean, s / np.float32(G), what + " mean, slope %g" % slope)
        worst = max(worst, stats_within(mean, var, m64, v64, what + " slope %g" % slope))
    return worst


@pytest.mark.parametrize("C", RED_C)
@pytest.mark.parametrize("G", ONE_LAUNCH_G + TWO_LAUNCH_G)
def test_row_slice_reductions(ops, G, C):
    """spgan_colstats / spgan_colsum on integer matrices, 3 groups: colsum exact, the mean of a single tile bit-equal to
    float32(sum) / float32(G), mean and variance inside the derived bound.  Measured worst: mean 0.61 units, variance 5.7 units."""
    X = nm.int_matrix(nm.seeded("red", G, C), 3 * G, C)
    um, uv = _check_reductions(ops, X, cu(X), G, "G=%d C=%d" % (G, C))
    print("UNITS reductions G=%d C=%d mean %.3f var %.3f" % (G, C, um, uv))


@pytest.mark.parametrize("G,C", [(33, 65), (128, 64), (257, 64), (385, 7)])
def test_row_slice_reductions_column_view(ops, G, C):
    """the same through a column-slice view (ldx > C, first column not 16-byte aligned)"""
    big = nm.int_matrix(nm.seeded("redv", G, C), 3 * G, C + 13)
    _check_reductions(ops, big[:, 5:5 + C], cu(big)[:, 5:5 + C], G, "view G=%d C=%d" % (G, C))


# ============================================================================= b. finalize loops on synthetic records
# colfinalize_body<32, 8>: slice sl walks tiles sl, sl+32, ...;  8-in-flight loop `t + 224 < tiles`, 4-in-flight loop `t + 96 < tiles`.
#   1: one record;  31, 32, 33: slices without a record / one each / a second for slice 0;  96, 97: the 4-in-flight bound for slice 0;
#   128, 129: it for every slice, then a remainder;  224, 225: the 8-in-flight bound for slice 0;  256, 257: it for every slice, then a
#   remainder;  481: 8-in-flight, then 4-in-flight (257 + 96 < 481 for slice 0 only), then single records;  2047: the last size of this geometry.
FIN_TILES_32x8 = [1, 31, 32, 33, 96, 97, 128, 129, 224, 225, 256, 257, 481, 2047]
# colfinalize_body<128, 2> (tiles >= 2048): 2048 the first size; 2049 a remainder for slice 0; 2945 = 2*1024 + 897: 8-in-flight twice
# and the 4-in-flight bound (2048 + 384 < 2945) with single records behind it; 3073 = 3*1024 + 1.
FIN_TILES_128x2 = [2048, 2049, 2945, 3073]
# <32,8>: 8 columns per workgroup -- 1, 2, 7 ragged, 8 full, 9 and 17 into the next blocks;  <128,2>: 2 columns per workgroup
FIN_C = [1, 2, 7, 8, 9, 17]


def fin_G(tiles, tile_rows):
    """rows of a group: the last tile ragged wherever a tile has more than one row"""
    return tiles * tile_rows - (1 if tile_rows > 1 else 0)


_REC = {}


def records(tiles, C, groups, tile_rows, mode):
    """(records float32 [groups*tiles, C, 2], G), built once.  mode 1: small integers (every sum exact);  mode 0: the (sum, centred M2) of
    rows drawn around column means 0, 3, -50 (sigma 1, 1, 2)."""
    key = (tiles, C, groups, tile_rows, mode)
    if key not in _REC:
        G = fin_G(tiles, tile_rows)
        r = nm.seeded("fin", *key)
        if mode == 1:
            rec = r.integers(-8, 9, size=(groups * tiles, C, 2)).astype(np.float32)
        else:
            mu, sd = np.array([0.0, 3.0, -50.0])[np.arange(C) % 3], np.array([1.0, 1.0, 2.0])[np.arange(C) % 3]
            rec = nm.records_from_rows((mu + sd * r.standard_normal((groups * G, C))).astype(np.float32), tile_rows, 0, G=G)
        _REC[key] = (rec, G)
    return _REC[key]


@pytest.mark.parametrize("tiles", FIN_TILES_32x8 + FIN_TILES_128x2)
def test_finalize_loops(ops, tiles):
    """ops._finalize over C in FIN_C, groups in {1, 3}, tile_rows in {1, 3}: mode 1 on integer records equals the exact sums, mode 0 stays
    inside the derived bound of merge_records64.  Measured worst over all sizes: mean 1.8 units, variance 2.7 units."""
    worst = (0.0, 0.0)
    for tile_rows in (1, 3):
        for C_ in FIN_C:
            for groups in (1, 3):
                what = "tiles=%d tile_rows=%d C=%d groups=%d" % (tiles, tile_rows, C_, groups)
                rec, G = records(tiles, C_, groups, tile_rows, 1)
                s0, s1 = ops._finalize(cu(rec), groups, tiles, C_, G, 1, tile_rows)
                w0, w1 = nm.merge_records64(rec, G, tile_rows, 1)
                same(s0, w0, what + " s0"); same(s1, w1, what + " s1")
                rec, G = records(tiles, C_, groups, tile_rows, 0)
                mean, var = ops._finalize(cu(rec), groups, tiles, C_, G, 0, tile_rows)
                worst = max(worst, stats_within(mean, var, *nm.merge_records64(rec, G, tile_rows, 0), what))
    print("UNITS finalize tiles=%d mean %.3f var %.3f" % (tiles, worst[0], worst[1]))


# ============================================================================= c. hard columns
HARD_G = 4173                                   # 33 tiles of 128 rows, the last one of 77


def test_hard_columns(ops):
    """Columns with (mean, sigma) = (0,1), (3,1), (1e3,1), (1e4,1), (100,1e-2), (-1e3,0.5) and a constant one, G = 4173, through ops.colstats
    and through the statistics records of gemm_nt's epilogue (weight 0.5*I: Y = X/2 exactly) with stats=True and with bn=...: variance and
    mean inside 32 units of the float64 statistics (an E[x^2] - mean^2 kernel is 4e3..8e4 units off on columns 2, 3 and 5), the constant
    column's variance exactly 0 and its invstd 1/sqrt(eps).
    Measured per column, variance units: colstats 0.22 0.44 0.04 0.03 0.01 0.04 0, gemm_nt 0.22 0.44 0.05 0.03 0.01 0.01 0;  mean units:
    colstats 0 0.43 0.25 0.80 0.06 0.06 0, gemm_nt 0 0.43 0.25 0.83 0.06 0.06 0.  Largest: 0.83."""
    X = nm.hard_columns(nm.seeded("hard", HARD_G), HARD_G)
    Xc = cu(X)
    k = nm.HARD_CONST_COL
    m64, v64 = nm.colstats64(X, HARD_G)
    assert v64[0, k] == 0.0
    mean, var = ops.colstats(Xc, HARD_G)
    um, uv = nm.stat_units(host(mean), host(var), m64, v64)
    print("UNITS hard colstats mean", np.round(um[0], 2), "var", np.round(uv[0], 2))
    assert um.max() <= 32 and uv.max() <= 32, (um, uv)
    assert var[0, k].item() == 0.0 and mean[0, k].item() == 2.5

    W = 0.5 * torch.eye(7, device="cuda")
    Y, gmean, gvar = ops.gemm_nt(Xc, W, stats=True)
    assert torch.equal(Y, Xc * 0.5)
    y64m, y64v = nm.colstats64(host(Y), HARD_G)
    um, uv = nm.stat_units(host(gmean)[None], host(gvar)[None], y64m, y64v)
    print("UNITS hard gemm_nt mean", np.round(um[0], 2), "var", np.round(uv[0], 2))
    assert um.max() <= 32 and uv.max() <= 32, (um, uv)
    assert gvar[k].item() == 0.0 and gmean[k].item() == 1.25

    gamma, beta = cu(np.linspace(0.5, 2.0, 7)), cu(np.linspace(-1.0, 1.0, 7))
    rm, rv = torch.zeros(7, device="cuda"), torch.ones(7, device="cuda")
    Y2, (sc, sh, inv, mu) = ops.gemm_nt(Xc, W, bn=(gamma, beta, rm, rv))
    assert torch.equal(Y2, Y)
    um, _ = nm.stat_units(host(mu)[None], host(gvar)[None], y64m, y64v)
    assert um.max() <= 32
    # invstd = 1/sqrt(var + eps) of a variance inside the bound: the interval that bound allows, widened by the 5e of invstd's own arithmetic
    _, bv = nm.stat_bounds(y64m, y64v)
    lo, hi = 1.0 / np.sqrt(y64v[0] + bv[0] + EPS), 1.0 / np.sqrt(y64v[0] - bv[0] + EPS)
    assert (host(inv) >= lo * (1 - 5 * nm.E32)).all() and (host(inv) <= hi * (1 + 5 * nm.E32)).all(), (host(inv), lo, hi)
    within(inv[k:k + 1], np.array([1.0 / np.sqrt(EPS)]), np.array([5 * nm.E32 / np.sqrt(EPS)]), "invstd of the constant column")
    t = nm.bn_tail64(host(mu), 1.0 / host(inv) ** 2 - EPS, host(gamma), host(beta), np.zeros(7), np.ones(7), HARD_G, EPS, ops.BN_MOMENTUM)
    within(rm, t[4], 6 * nm.E32 * np.abs(t[4]), "running mean")


# ============================================================================= d. BatchNorm tails
def fin_bn(lib, rec, tiles, C_, G, tile_rows, gamma, beta, momentum, rm, rv):
    out = torch.empty((4, C_), device="cuda")
    ok(lib.spgan_colstats_finalize_bn(P(rec), tiles, C_, G, tile_rows, P(gamma), P(beta), EPS, momentum, P(rm), P(rv),
                                      P(out[0]), P(out[1]), P(out[2]), P(out[3]), S()), "colstats_finalize_bn")
    return out


def check_tail(out4, rm_new, rv_new, mean32, var32, gamma, beta, rm_old, rv_old, count, momentum, what):
    """out4 = scale | shift | invstd | mean and the advanced running statistics against bn_tail64 from the float32 (mean32, var32)"""
    g_, b_ = host(gamma), host(beta)
    want = nm.bn_tail64(mean32, var32, g_, b_, rm_old, rv_old, count, EPS, momentum)
    bnd = nm.bn_tail_bounds(mean32, var32, g_, b_, rm_old, rv_old, count, EPS, momentum)
    u = [within(out4[0], want[0], bnd[0], what + " scale"), within(out4[1], want[1], bnd[1], what + " shift"),
         within(out4[2], want[2], bnd[2], what + " invstd")]
    same(out4[3], mean32, what + " mean")
    if rm_old is not None:
        u += [within(rm_new, want[4], bnd[3], what + " running_mean"), within(rv_new, want[5], bnd[4], what + " running_var")]
        if momentum == 1.0:
            same(rm_new, mean32, what + " running_mean at momentum 1")
    return max(u)


# (tiles, tile_rows): G = 1 (count 1), one ragged tile, 33 and 225 tiles (a second record for slice 0; the 8-in-flight loop)
@pytest.mark.parametrize("tiles,tile_rows", [(1, 1), (1, 3), (33, 3), (225, 3), (33, 1)])
@pytest.mark.parametrize("C_", [7, 9])
def test_finalize_bn_tail(ops, lib, tiles, tile_rows, C_):
    """spgan_colstats_finalize_bn on the records of (b): mean / var are those of the stand-alone finalize bit for bit; scale, shift, invstd
    and the running statistics follow bn_tail64 (gamma / beta NULL, running statistics NULL, momentum 0.1 and 1.0, count 1 at G = 1: the
    running variance takes var itself).  Measured worst: 0.33 of the bound."""
    rec, G = records(tiles, C_, 1, tile_rows, 0)
    recc = cu(rec)
    mean, var = ops._finalize(recc, 1, tiles, C_, G, 0, tile_rows)
    mean32, var32 = host(mean)[0], host(var)[0]
    if G == 1:
        assert (var32 == 0).all()
    r = nm.seeded("tail", tiles, tile_rows, C_)
    gamma, beta = cu(r.standard_normal(C_)), cu(r.standard_normal(C_))
    rm0, rv0 = r.standard_normal(C_).astype(np.float32), (r.random(C_) + 0.5).astype(np.float32)
    worst = 0.0
    for ga, be, running, momentum in ((gamma, beta, True, 0.1), (None, None, True, 0.1), (gamma, None, False, 0.1), (gamma, beta, True, 1.0)):
        rm, rv = (cu(rm0), cu(rv0)) if running else (None, None)
        out = fin_bn(lib, recc, tiles, C_, G, tile_rows, ga, be, momentum, rm, rv)
        what = "tiles=%d tile_rows=%d C=%d affine=%s running=%s momentum=%g" % (tiles, tile_rows, C_, ga is not None, running, momentum)
        worst = max(worst, check_tail(out, rm, rv, mean32, var32, ga, be, rm0 if running else None, rv0 if running else None, G, momentum, what))
        if G == 1 and running:                                  # count 1: no count/(count-1)
            within(rv, (1 - momentum) * rv0.astype(np.float64), 6 * nm.E32 * np.abs(rv0), what + " running_var at count 1")
    print("UNITS bn tail tiles=%d tile_rows=%d C=%d: %.3f of the bound" % (tiles, tile_rows, C_, worst))


# groups 2 and 3 run colfinalize_bn_groups_kernel (4-in-flight loop `t + 96 < tiles`: 97 for slice 0, 129 for every slice and a remainder,
# 225 twice for slice 0), groups 1 and 4 the sequential walk of colfinalize_body (225: its 8-in-flight loop)
@pytest.mark.parametrize("tpg", [1, 33, 97, 129, 225])
@pytest.mark.parametrize("groups", [1, 2, 3, 4])
def test_finalize_bn_groups_is_the_sequence_of_single_calls(lib, groups, tpg):
    """spgan_colstats_finalize_bn_groups == `groups` successive spgan_colstats_finalize_bn calls on the same records, torch.equal: all four
    output vectors of every group and the running statistics advanced in group order (the promise above colfinalize_bn_groups_kernel)."""
    for C_, running in ((7, True), (9, True), (8, False)):
        rec, G = records(tpg, C_, groups, 3, 0)
        recc = cu(rec)
        r = nm.seeded("grp", groups, tpg, C_)
        gamma, beta = cu(r.standard_normal(C_)), cu(r.standard_normal(C_))
        rm0, rv0 = cu(r.standard_normal(C_)), cu(r.random(C_) + 0.5)
        rm, rv = (rm0.clone(), rv0.clone()) if running else (None, None)
        out = torch.empty((4, groups, C_), device="cuda")
        ok(lib.spgan_colstats_finalize_bn_groups(P(recc), groups, tpg, C_, G, 3, P(gamma), P(beta), EPS, 0.1, P(rm), P(rv), P(out), S()), "bn_groups")
        rm1, rv1 = (rm0.clone(), rv0.clone()) if running else (None, None)
        for g in range(groups):
            one = fin_bn(lib, recc[g * tpg:(g + 1) * tpg], tpg, C_, G, 3, gamma, beta, 0.1, rm1, rv1)
            for q in range(4):
                assert torch.equal(out[q, g], one[q]), "groups=%d tpg=%d C=%d group %d vector %d" % (groups, tpg, C_, g, q)
        if running:
            assert torch.equal(rm, rm1) and torch.equal(rv, rv1), "running statistics, groups=%d tpg=%d C=%d" % (groups, tpg, C_)
            assert not torch.equal(rm, rm0)


@pytest.mark.parametrize("count_rep", [1, 3])
@pytest.mark.parametrize("split", [1, 8, 16])
def test_finalize_bn2_split(ops, lib, split, count_rep):
    """spgan_colstats_finalize_bn2, C = 17: columns below the split use layer A's vectors, the rest layer B's indexed from 0; the running
    variance counts G*count_rep rows.  Against two bn_tail64 calls, and -- count_rep 1 -- bit for bit against spgan_colstats_finalize_bn on
    the two column blocks of the records.  Measured worst: 0.29 of the bound."""
    C_, tiles = 17, 33
    rec, G = records(tiles, C_, 1, 3, 0)
    recc = cu(rec)
    mean, var = ops._finalize(recc, 1, tiles, C_, G, 0, 3)
    mean32, var32 = host(mean)[0], host(var)[0]
    r = nm.seeded("bn2", split, count_rep)
    nA, nB = split, C_ - split
    v = lambda n: r.standard_normal(n).astype(np.float32)
    gA, bA, gB, bB = v(nA), v(nA), v(nB), v(nB)
    rmA0, rvA0, rmB0, rvB0 = v(nA), np.abs(v(nA)) + 0.5, v(nB), np.abs(v(nB)) + 0.5
    t = {n: cu(a) for n, a in dict(gA=gA, bA=bA, gB=gB, bB=bB, rmA=rmA0, rvA=rvA0, rmB=rmB0, rvB=rvB0).items()}
    out = torch.empty((4, C_), device="cuda")
    ok(lib.spgan_colstats_finalize_bn2(P(recc), tiles, C_, G, 3, split, P(t["gA"]), P(t["bA"]), P(t["rmA"]), P(t["rvA"]), P(t["gB"]), P(t["bB"]),
                                       P(t["rmB"]), P(t["rvB"]), EPS, 0.1, count_rep, P(out), S()), "bn2")
    worst = 0.0
    for lo, hi, ga, be, rm_new, rv_new, rm0, rv0 in ((0, split, t["gA"], t["bA"], t["rmA"], t["rvA"], rmA0, rvA0),
                                                   (split, C_, t["gB"], t["bB"], t["rmB"], t["rvB"], rmB0, rvB0)):
        worst = max(worst, check_tail(out[:, lo:hi], rm_new, rv_new, mean32[lo:hi], var32[lo:hi], ga, be, rm0, rv0, G * count_rep, 0.1,
                                      "split=%d count_rep=%d columns %d:%d" % (split, count_rep, lo, hi)))
        if count_rep == 1:
            rm1, rv1 = cu(rm0), cu(rv0)
            one = fin_bn(lib, cu(rec[:, lo:hi]), tiles, hi - lo, G, 3, ga, be, 0.1, rm1, rv1)
            assert torch.equal(out[:, lo:hi], one) and torch.equal(rm_new, rm1) and torch.equal(rv_new, rv1)
    print("UNITS bn2 split=%d count_rep=%d: %.3f of the bound" % (split, count_rep, worst))


def _bwd_vectors(r, C_):
    return cu(r.standard_normal(C_) * 0.2), cu(np.abs(r.standard_normal(C_)) + 0.5), cu(np.abs(r.standard_normal(C_)) + 0.5)


def _coeffs(lib, s0, s1, mean, inv, gamma, count):
    C_ = s0.numel()
    coef, sums = torch.empty((3, C_), device="cuda"), torch.cat([s0.reshape(-1), s1.reshape(-1)])
    ok(lib.spgan_bn_bwd_coeffs(P(sums), P(mean), P(inv), P(gamma), C_, float(count), P(coef), S()), "bn_bwd_coeffs")
    return coef


@pytest.mark.parametrize("tiles", [1, 33, 225, 2049])
def test_finalize_bnbwd(ops, lib, tiles):
    """spgan_colstats_finalize_bnbwd: the sums are those of the stand-alone mode-1 finalize and the coefficients those of
    spgan_bn_bwd_coeffs on them, bit for bit (gamma given and NULL); once against bn_bwd_coeffs64 at rel-L2 1e-6 on non-integer records.
    Measured: p 2.3e-8, q 8.8e-8, r 6.7e-8."""
    for C_, with_gamma in ((7, True), (9, False)):
        rec, G = records(tiles, C_, 1, 3, 1)
        recc = cu(rec)
        s0, s1 = ops._finalize(recc, 1, tiles, C_, G, 1, 3)
        mean, inv, gamma = _bwd_vectors(nm.seeded("bnbwd", tiles, C_), C_)
        gamma = gamma if with_gamma else None
        o0, o1, coef = torch.empty(C_, device="cuda"), torch.empty(C_, device="cuda"), torch.empty((3, C_), device="cuda")
        ok(lib.spgan_colstats_finalize_bnbwd(P(recc), tiles, C_, G, 3, P(mean), P(inv), P(gamma), float(G), P(o0), P(o1), P(coef), S()), "bnbwd")
        assert torch.equal(o0, s0[0]) and torch.equal(o1, s1[0])
        assert torch.equal(coef, _coeffs(lib, s0, s1, mean, inv, gamma, G)), "tiles=%d C=%d" % (tiles, C_)
    if tiles == 33:
        C_ = 9
        rec = (nm.seeded("bnbwd.f", tiles).standard_normal((tiles, C_, 2)) * 5).astype(np.float32)
        G = fin_G(tiles, 3)
        mean, inv, gamma = _bwd_vectors(nm.seeded("bnbwd.v", tiles), C_)
        o0, o1, coef = torch.empty(C_, device="cuda"), torch.empty(C_, device="cuda"), torch.empty((3, C_), device="cuda")
        recc = cu(rec)
        ok(lib.spgan_colstats_finalize_bnbwd(P(recc), tiles, C_, G, 3, P(mean), P(inv), P(gamma), float(G), P(o0), P(o1), P(coef), S()), "bnbwd")
        want = nm.bn_bwd_coeffs64(np.concatenate([host(o0), host(o1)]), host(mean), host(inv), host(gamma), G)
        errs = [rel_l2(coef[i], want[i]) for i in range(3)]
        print("UNITS bn_bwd coefficients rel-L2 p %.2e q %.2e r %.2e" % tuple(errs))
        assert max(errs) <= 1e-6, errs


def test_finalize_multi(ops, lib):
    """spgan_colstats_finalize_multi, three problems with their own C and tile counts, kinds 0 (sums) and 1 (sums + coefficients) mixed:
    every problem equals its stand-alone launch bit for bit."""
    from spgan._lib import ColFinalizeArgs
    probs = [(7, 33, 1), (17, 225, 0), (2, 1, 1)]               # (C, tiles, kind): the widest problem is not the first
    arr = (ColFinalizeArgs * 3)()
    keep, want = [], []
    for i, (C_, tiles, kind) in enumerate(probs):
        rec, G = records(tiles, C_, 1, 3, 1)
        recc = cu(rec)
        s0, s1 = ops._finalize(recc, 1, tiles, C_, G, 1, 3)
        mean, inv, gamma = _bwd_vectors(nm.seeded("multi", i), C_)
        o0, o1, coef = torch.zeros(C_, device="cuda"), torch.zeros(C_, device="cuda"), torch.zeros((3, C_), device="cuda")
        a = arr[i]
        a.partials, a.tiles, a.C, a.G, a.tile_rows, a.s0, a.s1, a.kind = P(recc), tiles, C_, G, 3, P(o0), P(o1), kind
        if kind == 1:
            a.mean, a.invstd, a.gamma, a.count, a.coef = P(mean), P(inv), P(gamma), float(G), P(coef)
        keep.append((recc, mean, inv, gamma))
        want.append((o0, o1, coef, s0[0], s1[0], _coeffs(lib, s0, s1, mean, inv, gamma, G) if kind == 1 else None))
    ok(lib.spgan_colstats_finalize_multi(arr, 3, S()), "finalize_multi")
    for i, (o0, o1, coef, s0, s1, c) in enumerate(want):
        assert torch.equal(o0, s0) and torch.equal(o1, s1), "problem %d sums" % i
        if c is not None:
            assert torch.equal(coef, c), "problem %d coefficients" % i


def test_bn_prepare_edges(ops):
    """ops.bn_prepare: a slightly negative variance is clamped to 0 (invstd 1/sqrt(eps), running variance advanced with 0); count 1 takes
    var itself; eval mode reads the running statistics and leaves them alone."""
    C_ = 9
    r = nm.seeded("prep")
    mean = r.standard_normal(C_).astype(np.float32)
    var = (r.random(C_) + 0.1).astype(np.float32)
    var[2], var[5] = -1e-7, -0.0
    gamma, beta = cu(r.standard_normal(C_)), cu(r.standard_normal(C_))
    rm0, rv0 = r.standard_normal(C_).astype(np.float32), (r.random(C_) + 0.5).astype(np.float32)
    clamped = np.maximum(var, 0).astype(np.float64)
    for count in (640, 1):
        rm, rv = cu(rm0), cu(rv0)
        out = torch.stack(ops.bn_prepare(cu(mean), cu(var), gamma, beta, count, True, rm, rv))
        check_tail(out, rm, rv, mean.astype(np.float64), clamped, gamma, beta, rm0, rv0, count, ops.BN_MOMENTUM, "bn_prepare count=%d" % count)
        within(out[2, 2:3], np.array([1 / np.sqrt(EPS)]), np.array([5 * nm.E32 / np.sqrt(EPS)]), "invstd of the clamped column")
    rm, rv = cu(rm0), cu(rv0)
    out = torch.stack(ops.bn_prepare(None, None, gamma, beta, 640, False, rm, rv))
    check_tail(out, None, None, rm0.astype(np.float64), rv0.astype(np.float64), gamma, beta, None, None, 640, 0.1, "bn_prepare eval")
    same(rm, rm0, "eval leaves running_mean"); same(rv, rv0, "eval leaves running_var")


# ============================================================================= e. bn_bwd_apply
# (1,4) (3,8) (257,132): the float4 kernel (a single thread, a partial workgroup, 8481 threads: more than one workgroup and a ragged one);
# (65,70) (130,1): the scalar kernel.  add=: the apply2 launch for C % 4 == 0, col_scale_add + the plain launch otherwise.
@pytest.mark.parametrize("M,C_", [(1, 4), (3, 8), (257, 132), (65, 70), (130, 1)])
def test_bn_bwd_apply(ops, M, C_):
    """ops.bn_bwd_apply against bn_bwd_apply64, gamma None and given, with and without add=: rel-L2 <= 1e-5; two calls bit-identical.
    The kernel evaluates one expression per element from whatever sums it is given, so the sums are drawn independently of g: with the
    true column sums a single row (M = 1) would give g - S0 = 0 exactly and a relative error would measure nothing but that cancellation.
    Measured worst rel-L2: 6.7e-8."""
    r = nm.seeded("apply", M, C_)
    y = (r.standard_normal((M, C_)) * 2 + 0.3).astype(np.float32)
    g, g2 = r.standard_normal((M, C_)).astype(np.float32), r.standard_normal((M, C_)).astype(np.float32)
    s = r.standard_normal(C_).astype(np.float32)
    mean = y.astype(np.float64).mean(0).astype(np.float32)
    inv = (1.0 / np.sqrt(y.astype(np.float64).var(0) + EPS)).astype(np.float32)
    gamma = (np.abs(r.standard_normal(C_)) + 0.5).astype(np.float32)
    sums = (r.standard_normal(2 * C_) * np.sqrt(M)).astype(np.float32)
    worst = 0.0
    for ga in (None, gamma):
        for add in (None, (g2, s)):
            want = nm.bn_bwd_apply64(g, y, mean, inv, ga, sums, M, add=add)
            args = (cu(g), cu(y), cu(mean), cu(inv), cu(ga), cu(sums), M)
            kw = {} if add is None else dict(add=(cu(g2), cu(s)))
            got = ops.bn_bwd_apply(*args, **kw)
            err = rel_l2(got, want)
            worst = max(worst, err)
            assert err <= 1e-5, "M=%d C=%d gamma=%s add=%s: rel-L2 %.3e" % (M, C_, ga is not None, add is not None, err)
            assert torch.equal(got, ops.bn_bwd_apply(*args, **kw))
    print("UNITS bn_bwd_apply M=%d C=%d rel-L2 %.2e" % (M, C_, worst))


# ============================================================================= f. maxpool
def _pool_variants(r, C_):
    """(scale, shift) pairs: both signs with one zero scale (column 2 where it exists); none; for narrow C also all negative and all zero"""
    sc, sh = nm.dyadic_affine(r, C_, zero_at=2)
    out = [(sc, sh), (None, None)]
    if C_ < 3:
        out += [(-np.abs(sc), sh), (np.zeros_like(sc), sh)]
    return out


def _check_maxpool(ops, B, N, C_, ld=None):
    r = nm.seeded("pool", B, N, C_, ld or 0)
    for sc, sh in _pool_variants(r, C_):
        y = nm.tie_matrix(r, B, N, C_, sc)
        if ld is None:
            yc = cu(y)
        else:                                                   # a column-slice view with row stride ld
            big = torch.full((B * N, ld), 99.0, device="cuda")
            big[:, :C_] = cu(y)
            yc = big[:, :C_]
        for slope in (1.0, 0.25, 0.0):
            val, arg = nm.maxpool64(y, B, N, sc, sh, slope)
            out, a = ops.maxpool(yc, B, N, cu(sc), cu(sh), slope)
            what = "B=%d N=%d C=%d ld=%s affine=%s slope=%g" % (B, N, C_, ld, sc is not None, slope)
            same(out, val, what + " values"); same(a, arg, what + " arg-max")


# maxpool_v4_kernel<16> (C % 4 == 0, N < 512): 16 row slices, 8-in-flight loop `n + 112 < N`.  N = 1: one row; 15, 16, 17: slices
# without a row / one each / a second for slice 0; 112, 113: the loop bound for slice 0; 129: it for every slice and a remainder; 241: twice
# for slice 0.  C = 4: one lane; 60: a ragged 64-column block; 64: a full one; 68: one lane into the second block; 132: three blocks.
@pytest.mark.parametrize("N", [1, 15, 16, 17, 112, 113, 129, 241])
@pytest.mark.parametrize("C_", [4, 60, 64, 68, 132])
def test_maxpool_16_lanes(ops, C_, N):
    """values and arg-max (first row on ties) torch.equal to maxpool64 on tie matrices: slopes 1, 0.25, 0; scales of both signs, zero, none"""
    _check_maxpool(ops, 3, N, C_)


# maxpool_v4_kernel<4> (N >= 512 and B * ceil(C/64) < 512): 64 row slices, 8-in-flight loop `n + 448 < N`.  512: one round for every slice;
# 513, 575: a remainder row for slice 0 / for 63 slices; 961: a second round for slice 0 only (512 + 448 < 961); 1025: two rounds and a remainder
@pytest.mark.parametrize("N", [512, 513, 575, 961, 1025])
def test_maxpool_4_lanes(ops, N):
    _check_maxpool(ops, 2, N, 64)


# maxpool_kernel (C % 4 != 0, or a row stride that is no multiple of 4): 4 row slices, 64 columns per workgroup
@pytest.mark.parametrize("N", [1, 3, 4, 5, 130])
@pytest.mark.parametrize("C_,ld", [(1, None), (63, None), (65, None), (70, None), (64, 67)])
def test_maxpool_scalar(ops, C_, ld, N):
    _check_maxpool(ops, 3, N, C_, ld)


# ============================================================================= g. pool_finalize on synthetic records
def _pool_records(r, B, tiles, C_):
    """integer (max, min) records with max >= min and arbitrary rows inside each tile; tile 2 of every shape repeats tile 0's VALUES (with
    its own rows), and tile 1 lies inside tile 0's range (it ties at most): the first tile must win"""
    v = r.integers(-8, 9, size=(B, tiles, C_, 2)).astype(np.float32)
    vmax, vmin = v.max(-1), v.min(-1)
    vmax[:, 1] = np.clip(vmax[:, 1], vmin[:, 0], vmax[:, 0])
    vmin[:, 1] = np.clip(vmin[:, 1], vmin[:, 0], vmax[:, 1])
    vmax[:, 2], vmin[:, 2] = vmax[:, 0], vmin[:, 0]
    pval = np.stack([vmax, vmin], -1).reshape(B * tiles, C_, 2)
    parg = (np.arange(B * tiles)[:, None, None] * 128 + r.integers(0, 128, size=(B * tiles, C_, 2))).astype(np.int32)
    return pval, parg


@pytest.mark.parametrize("C_", [1, 64, 65])                     # 64 columns per workgroup: one thread, a full block, one column into the second
def test_pool_finalize(lib, C_):
    """spgan_pool_finalize and _groups (group_stride > C, shapes_per_group 1 and 3, relative_rows 0 and 1) on synthetic records, B = 3,
    rows = 384: the same extreme in tiles 0 and 2 gives tile 0's row, a negative scale takes the min record, a zero scale row b*rows;
    pooled, argmax and yarg torch.equal to pool_finalize64."""
    B, rows, tiles = 3, 384, 3
    r = nm.seeded("pf", C_)
    pval, parg = _pool_records(r, B, tiles, C_)
    pv, pa = cu(pval), cu(parg, torch.int32)
    zero_at = 1 if C_ > 1 else None
    variants = [nm.dyadic_affine(r, C_, zero_at=zero_at)]
    if C_ == 1:
        sc, sh = variants[0]
        variants += [(-np.abs(sc), sh), (np.zeros_like(sc), sh)]
    for sc, sh in variants:
        for slope in (0.25, 1.0):
            for with_yarg in (True, False):
                pooled, arg, yarg = torch.empty((B, C_), device="cuda"), torch.empty((B, C_), dtype=torch.int32, device="cuda"), torch.empty((B, C_), device="cuda")
                scc, shc = cu(sc), cu(sh)
                ok(lib.spgan_pool_finalize(P(pv), P(pa), B, rows, C_, P(scc), P(shc), slope, P(pooled), P(arg), P(yarg) if with_yarg else None, S()),
                   "pool_finalize")
                w = nm.pool_finalize64(pval, parg, B, rows, sc, sh, slope)
                same(pooled, w[0], "pooled"); same(arg, w[1], "argmax")
                if with_yarg:
                    same(yarg, w[2], "yarg")
    tmax = pval.reshape(B, tiles, C_, 2)                         # the tie is really there, and tile 0's row is what the model expects
    assert (tmax[:, 0] == tmax[:, 2]).all()
    for spg in (1, 3):
        groups, stride = B // spg, C_ + 3
        sc, sh = np.full((groups, stride), 7.0, np.float32), np.full((groups, stride), 7.0, np.float32)
        for g in range(groups):
            sc[g, :C_], sh[g, :C_] = nm.dyadic_affine(r, C_, zero_at=zero_at)
        for rel in (0, 1):
            pooled, arg, yarg = torch.empty((B, C_), device="cuda"), torch.empty((B, C_), dtype=torch.int32, device="cuda"), torch.empty((B, C_), device="cuda")
            scc, shc = cu(sc), cu(sh)
            ok(lib.spgan_pool_finalize_groups(P(pv), P(pa), B, rows, C_, P(scc), P(shc), stride, spg, 0.25, P(pooled), P(arg), P(yarg), rel, S()),
               "pool_finalize_groups")
            w = nm.pool_finalize64(pval, parg, B, rows, sc, sh, 0.25, stride, spg, rel)
            what = "groups: shapes_per_group=%d relative_rows=%d " % (spg, rel)
            same(pooled, w[0], what + "pooled"); same(arg, w[1], what + "argmax"); same(yarg, w[2], what + "yarg")


# ============================================================================= h. pooling records of the GEMM epilogues
def _gemm_pool(ops, B, rows, C_, K, hint):
    r = nm.seeded("gp", B, rows, C_, K)
    A = r.integers(-3, 4, size=(B * rows, K)).astype(np.float32)
    W = r.integers(-2, 3, size=(C_, K)).astype(np.float32)
    bias = r.integers(-2, 3, size=C_).astype(np.float32)
    gamma = (r.choice([-1.0, 1.0], size=C_) * (0.5 + r.random(C_))).astype(np.float32)
    gamma[3] = 0.0
    beta = r.standard_normal(C_).astype(np.float32)
    with ops.nt_tile_hint(hint):
        Y, st, pooled, arg, yarg = ops.gemm_bn_pool(cu(A), cu(W), cu(bias), (cu(gamma), cu(beta), None, None), rows, 0.2, keep_y=True)
    Yw = A.astype(np.float64) @ W.astype(np.float64).T + bias   # small integers: exact in any operand mode
    same(Y, Yw, "Y")
    scale = host(st[0])
    assert (np.sign(scale) == np.sign(gamma)).all() and (gamma < 0).any() and (gamma > 0).any()
    Y3 = Yw.reshape(B, rows, C_)
    first = np.where(scale > 0, Y3.argmax(1), np.where(scale < 0, Y3.argmin(1), 0)) + np.arange(B)[:, None] * rows
    ties = (Y3 == Y3.max(1, keepdims=True)).sum(1)
    assert (ties >= 2).any()                                    # integer outputs: maxima do repeat
    return Yw, scale, first, arg, yarg


GEMM_POOL_SHAPES = [(3, 128, 70), (2, 256, 256), (3, 384, 128)]   # a ragged column tile; the 256 x 256-tile kernel's shape; three record tiles per shape


@pytest.mark.parametrize("hint", [0, 1, 2])
@pytest.mark.parametrize("K", [8, 32])
@pytest.mark.parametrize("B,rows,C_", GEMM_POOL_SHAPES)
def test_gemm_pool_records_first_row(ops, B, rows, C_, K, hint):
    """ops.gemm_bn_pool on integer operands (every product exact, ties everywhere), gamma positive, negative and one zero, under
    nt_tile_hint 0, 1, 2: the arg-max is the first row of the max of Y for scale > 0, the first row of the min for scale < 0 and b*rows
    for scale == 0; yarg is Y at that row (the column with scale == 0 has a test of its own below)."""
    Yw, scale, first, arg, yarg = _gemm_pool(ops, B, rows, C_, K, hint)
    same(arg, first, "arg-max")
    live = scale != 0
    want = np.take_along_axis(Yw, first, axis=0)
    assert (host(yarg)[:, live] == want[:, live]).all()


def test_gemm_pool_zero_scale_yarg(ops):
    """yarg == Y at the arg-max row in the column whose scale is 0, where that row is b*rows: the same 18 cases (shapes, K, tile hints).
    The (max, min) records hold no value of that row (spgan_pool_finalize alone returns the column maximum there, 6 to 73 away from
    Y[b*rows] in these cases); ops.gemm_bn_pool fills it in with spgan_pool_zero_scale_yarg, which forms the row's product from the
    GEMM's operands -- exact here, where every product is a small integer."""
    wrong = []
    for B, rows, C_ in GEMM_POOL_SHAPES:
        for K in (8, 32):
            for hint in (0, 1, 2):
                Yw, scale, first, arg, yarg = _gemm_pool(ops, B, rows, C_, K, hint)
                dead = scale == 0
                assert dead.sum() == 1
                diff = (host(yarg) - np.take_along_axis(Yw, first, axis=0))[:, dead].ravel()
                if (diff != 0).any():
                    wrong.append(((B, rows, C_, K, hint), diff.tolist()))
    assert not wrong, wrong


@pytest.mark.parametrize("with_pro", [False, True])
def test_gemm_groups_pool_zero_scale_yarg(ops, with_pro):
    """the same through ops.gemm_bn_groups (3 passes of 2 shapes of 128 rows, each pass with its own prologue vectors and BatchNorm):
    arg-max counted from the pass's first row, first row on ties, yarg == Y there in every column, the zero-scale one included"""
    groups, spg, rows, C_, K = 3, 2, 128, 70, 8
    Mg, B = spg * rows, groups * spg
    r = nm.seeded("gpg", int(with_pro))
    A = r.integers(-3, 4, size=(groups * Mg, K)).astype(np.float32)
    W = r.integers(-2, 3, size=(C_, K)).astype(np.float32)
    bias = r.integers(-2, 3, size=C_).astype(np.float32)
    gamma = (r.choice([-1.0, 1.0], size=C_) * (0.5 + r.random(C_))).astype(np.float32)
    gamma[3] = 0.0
    beta = r.standard_normal(C_).astype(np.float32)
    Aeff, pro = A.astype(np.float64), None
    if with_pro:
        psc, psh = np.zeros((groups, K), np.float32), np.zeros((groups, K), np.float32)
        for g in range(groups):
            psc[g], psh[g] = nm.dyadic_affine(r, K)
        z = Aeff.reshape(groups, Mg, K) * psc[:, None, :] + psh[:, None, :]
        Aeff, pro = nm.lrelu64(z, 0.25).reshape(groups * Mg, K), (cu(psc), cu(psh), 0.25)
    out, pooled, arg, yarg = ops.gemm_bn_groups(cu(A), cu(W), cu(bias), (cu(gamma), cu(beta), None, None), groups, pro=pro, rows=rows, slope=0.2)
    Yw = Aeff @ W.astype(np.float64).T + bias
    scale = host(out[0]).repeat(spg, axis=0)                                    # [B, C]: the vector of each shape's pass
    assert (np.sign(scale) == np.sign(gamma)).all()
    Y3 = Yw.reshape(B, rows, C_)
    local = np.where(scale > 0, Y3.argmax(1), np.where(scale < 0, Y3.argmin(1), 0))
    same(arg, local + (np.arange(B)[:, None] % spg) * rows, "arg-max (rows of the own pass)")
    same(yarg, np.take_along_axis(Yw, local + np.arange(B)[:, None] * rows, axis=0), "yarg")


def test_adain_pool_records_first_row(ops):
    """spgan.adain_epi.forward(pool=True) + pool_from_records, N = 128, 3 shapes, C = 64, against the `out` it returns: the maximum and its
    FIRST row (numpy on the CPU).  Shape 0 repeats its rows 0..63 in rows 64..127 (every maximum twice), shape 1 is one row 128 times
    (every row ties: row 128 wins), shape 2 is unconstrained."""
    from spgan import adain_epi as ae
    B, N, C_, K = 3, 128, 64, 32
    r = nm.seeded("adain")
    style = r.integers(-2, 3, size=(B * N, K)).astype(np.float32)
    x = r.standard_normal((B * N, C_)).astype(np.float32)
    style[64:128], x[64:128] = style[0:64], x[0:64]
    style[N:2 * N], x[N:2 * N] = style[N], x[N]
    Ws, bs = r.integers(-2, 3, size=(2 * C_, K)).astype(np.float32), r.integers(-2, 3, size=2 * C_).astype(np.float32)
    xc, sc, Wc = cu(x), cu(style), cu(Ws)
    assert ae.usable(xc, sc, Wc, N) and ae.can_pool(B * N, N)
    imean, ivar = ops.colstats(xc, N, 0.2)
    out, _, rec = ae.forward(xc, sc, Wc, cu(bs), N, 0.2, imean.contiguous(), ivar.contiguous(), pool=True)
    pm, pa = ae.pool_from_records(rec, B, N)
    o = host(out)
    val, arg = nm.maxpool64(o, B, N)
    same(pm, val, "pooled"); same(pa, arg, "arg-max")
    o3 = o.reshape(B, N, C_)
    assert ((o3[0] == val[0]).sum(0) >= 2).all() and (arg[0] < 64).all() and (arg[1] == N).all()
