"""GPU: the EdgeBlock gather kernels of csrc/edge.hip (edge_stats, edge_attend_fwd, edge_attend_bwd, edge_scatter) and spgan.EdgeBlock
against the float64-autograd model of tests/edgeblock_model.py, on random and on constructed graphs.

Tolerance rule (that of test_deform_gpu.py): every quantity is compared by rel-L2 against the float64 model on the same float32 operands;
bound = max(base, 5 x rel-L2(model in float32, model in float64)), both model runs on the CPU, base 2e-6 for forward quantities and 1e-5 for
backward ones.  rel-L2 only: no "or max-abs" escape, no element is ever excluded.
Kink condition: a LeakyReLU mask is discrete, so each case takes the first seed s0, s0+1, ... (at most 20, asserted) at which the float64
model has min|z2| and min|zy| >= 32 * 2^-24 * max(1, max|z|) (edgeblock_model.kinks_clear); tests/test_edgeblock_model_cpu.py shows that
the search ends for every case below.  The softmax-range case takes delta per column: its columns differ in range by a factor 70 and no
seed clears a delta taken from the widest one (expected misses per seed: about 4).
Module cases: the EdgeBlock-vs-golden bounds of test_parity_gpu.py (3e-6 output and dx, 5e-6 parameter gradients, buffers rtol 1e-5 /
atol 1e-6, the three conv biases in front of a train-mode BatchNorm to 2e-3 absolute), or 5 x the model's float32-vs-float64 distance
where that is larger.

Found by the k = 1 case: the generic edge_attend_bwd kernel formed d*yv - dot as one fused multiply-add, i.e. with the exact product, while
`dot` holds the rounded one; at k = 1 (dot == d*yv) g2 came out as the product's rounding residue (|g2| about 1e-8) instead of 0.  The
kernel now subtracts the rounded product.  The k = 10 register kernels are untouched (their machine code is unchanged).

MEASURED on an MI355X (rel-L2 in units of 1e-7; every bound above is 2e-6 / 1e-5 or larger):
  launchers  B   N  k   H   F graph   mean  var    T   g2   gy sums2 sumsy  dP   dQ   dR
             2  50 10  12  24 random 4.0  1.4  0.9  0.9  0.7  3.0  1.5  0.9  0.8  0.8
             2  50 10  12  24 hand   3.3  1.9  0.8  0.9  0.7  2.3  1.9  1.1  1.0  0.8
             1  65 10  64 128 random 3.7  2.2  0.9  0.9  0.7  2.1  1.9  1.0  0.9  0.8
             1  65 10  64 128 hand   3.2  2.4  0.9  0.9  0.7  2.3  1.7  1.1  1.0  0.8
             1  40 10 128 256 random 4.2  2.4  0.9  0.9  0.7  2.2  1.6  0.9  0.8  0.8
             1  40 10 128 256 hand   3.1  2.3  0.9  0.9  0.7  2.5  1.8  1.1  1.0  0.8
             2  48 10   7  13 random 2.6  1.2  0.8  0.9  0.7  2.8  2.0  0.9  0.8  0.8
             2  48 10   7  13 hand   2.5  1.2  0.9  0.9  0.7  2.7  2.5  1.1  1.0  0.9
             1  77  3  16  36 random 2.4  1.6  0.7  1.0  0.6  2.5  1.2  0.6  0.6  0.6
             1  77  3  16  36 hand   0.9  1.0  0.7  0.9  0.5  1.6  1.0  1.1  1.5  0.6
             3  40 20  40  80 random 4.4  1.9  1.0  1.1  0.9  3.5  2.8  1.2  1.0  1.0
             3  40 20  40  80 hand   4.9  2.5  1.0  1.1  0.9  2.6  2.4  1.3  1.1  1.0
             2  33  1   8  16 random 1.7  1.2  0.5  0.0  0.1  0.0  0.9  0.6  0.6  0.5
             2  33  1   8  16 hand   0.7  1.1  0.6  0.0  0.1  0.0  0.9  1.2  2.2  0.6
             1  35 32   5   9 random 7.0  3.3  1.2  1.2  1.1  4.7  2.2  1.5  1.4  1.3
             1  35 32   5   9 hand   5.0  2.3  1.2  1.3  1.1  2.9  3.4  1.4  1.3  1.4
             1   3  2   4   8 random 0.6  1.7  0.8  0.9  0.5  1.2  0.9  0.6  1.1  1.8
             1   3  2   4   8 hand   0.7  1.3  0.6  0.8  0.4  1.1  1.3  0.9  1.1  0.9
  (k = 1: g2 and sums2 are exactly 0, T is bit-equal to lrelu(zy).)
  softmax range, k 10, T: 2.09e-07 (bound 2.00e-06)
  softmax range, k 10, g2: 3.82e-07 (bound 1.00e-05)
  softmax range, k 10, gy: 2.33e-07 (bound 1.00e-05)
  softmax range, k 5, T: 9.51e-08 (bound 2.00e-06)
  softmax range, k 5, g2: 1.39e-07 (bound 1.00e-05)
  softmax range, k 5, gy: 9.21e-08 (bound 1.00e-05)
  offset columns, k 10, mean: 4.14e-08 (bound 2.00e-06)
  offset columns, k 10, var: 1.58e-06 (bound 5.85e-06)
  offset columns, k 10, var of the offset columns alone: 3.40e-06
  offset columns, k 5, mean: 3.16e-08 (bound 2.00e-06)
  offset columns, k 5, var: 3.83e-06 (bound 6.99e-06)
  offset columns, k 5, var of the offset columns alone: 8.92e-06
  module  Fin Fout  k  B   N    out   dx  worst parameter gradient
            3   64 10  2  50    4.7  4.9   5.9 (conv_w.1.bias)
           32   24  5  1  77    2.5  2.7   3.8 (conv_w.3.weight)
           16  128 10  1  65    6.8  5.2   5.8 (conv_w.4.weight)
            8   40 20  2  40    3.9  3.4   5.2 (conv_w.1.weight)
"""
import numpy as np
import pytest
import torch

import edgeblock_model as em
import kernel_model as km

pytestmark = pytest.mark.gpu
FWD, BWD = 2e-6, 1e-5
ZERO_GRAD_BIASES = ("conv_w.0.bias", "conv_w.3.bias", "conv_x.0.bias")


@pytest.fixture(scope="module")
def sp():
    import spgan
    from spgan import _lib
    _lib.load()
    return spgan


def _model(c, dt):
    """Every compared quantity from the CPU model in dtype dt (the scatter on the model's own gy and sums)."""
    t = lambda n: c[n].to(dt)
    idx, slope = c["idx"], c["slope"]
    r = {}
    r["mean"], r["var"] = em.stats(t("PQR"), idx, t("b1"), t("bx"))
    r["T"], z2, zy = em.attend(t("h2pre"), t("sc2"), t("sh2"), t("PQR"), idx, t("bx"), t("scx"), t("shx"), slope)
    r["g2"], r["gy"], r["sums2"], r["sumsy"] = em.attend_bwd(t("dT"), t("h2pre"), t("sc2"), t("sh2"), t("mean2"), t("inv2"), t("PQR"), idx, t("bx"),
                                                             t("scx"), t("shx"), t("meanx"), t("invx"), slope)
    r["dPQR"] = _scatter_model(c, dt, r["gy"], r["sumsy"])
    return r, z2, zy


def _sums1(c, dt):
    t = lambda n: c[n].to(dt)
    xh = (em.pre(t("PQR"), c["idx"], t("b1"), t("bx"))[0] - t("mean1")) * t("inv1")
    return torch.cat([t("g1").sum(0), (t("g1") * xh).sum(0)])


def _scatter_model(c, dt, gy, sumsy, tol=None):
    t = lambda n: c[n].to(dt)
    return em.scatter(t("g1"), gy.to(dt), t("PQR"), c["idx"], t("b1"), t("mean1"), t("inv1"), t("gam1"), _sums1(c, dt), t("bx"), t("meanx"),
                      t("invx"), t("gamx"), sumsy.to(dt), tol=tol)


def _pqr_blocks(d, H, F_):
    return {"dP": d[:, :H], "dQ": d[:, H:H + F_], "dR": d[:, H + F_:]}


def _launch(ops, c, scatter=True):
    """Every launcher once on the case's float32 operands -> dict of GPU results."""
    g = lambda n: c[n].cuda()
    B, N = c["B"], c["N"]
    idx = c["idx"].to(torch.int32).cuda()
    r = {"idx": idx}
    r["mean"], r["var"] = ops.edge_stats(g("PQR"), idx, g("b1"), g("bx"))
    r["T"] = ops.edge_attend_fwd(g("h2pre"), g("sc2"), g("sh2"), g("PQR"), idx, g("bx"), g("scx"), g("shx"), c["slope"])
    r["g2"], r["gy"], r["sums2"], r["sumsy"] = ops.edge_attend_bwd(g("dT"), g("h2pre"), g("sc2"), g("sh2"), g("mean2"), g("inv2"), g("PQR"), idx,
                                                                   g("bx"), g("scx"), g("shx"), g("meanx"), g("invx"), c["slope"])
    if scatter:
        r["rowptr"], r["src"] = ops.csr_build(idx, B, N)
        r["dPQR"] = ops.edge_scatter(g("g1"), r["gy"], g("PQR"), idx, r["rowptr"], r["src"], g("b1"), g("mean1"), g("inv1"), g("gam1"),
                                     _sums1(c, torch.float64).float().cuda(), g("bx"), g("meanx"), g("invx"), g("gamx"), r["sumsy"])
    return r


@pytest.mark.parametrize("hand", [False, True])
@pytest.mark.parametrize("B,N,k,H,F_", em.LAUNCHER_CASES)
def test_launchers_against_float64_autograd(sp, B, N, k, H, F_, hand):
    """(2,50,10,12,24): the k = 10 register kernels on the scalar path, idle lanes, a last stats / backward tile of 4 points;
    (1,65,10,64,128): the vector path, two tiles + one point; (1,40,10,128,256): the vector path, two channel passes; (2,48,10,7,13): k = 10
    with odd H and F, unaligned rows; (1,77,3,16,36): generic k; (3,40,20,40,80): generic k = 20, a partial second channel pass;
    (2,33,1,8,16): k = 1; (1,35,32,5,9): the largest k; (1,3,2,4,8): M smaller than one workgroup's points.
    hand: edgeblock_model.hand_graph (in-degree 0, a self-looped hub, one neighbour k times, in-degrees 1, 15, 16, 17, 32, 33)."""
    ops = sp.ops
    c = em.find_launcher_case(B, N, k, H, F_, hand)
    (m64, z2, zy), (m32, _, _) = _model(c, torch.float64), _model(c, torch.float32)
    got = _launch(ops, c)
    err, bound = {}, {}
    for q, base in (("mean", FWD), ("var", FWD), ("T", FWD), ("g2", BWD), ("gy", BWD), ("sums2", BWD), ("sumsy", BWD)):
        err[q], bound[q] = em.rel(got[q], m64[q]), max(base, 5.0 * em.rel(m32[q], m64[q]))
    # the scatter is compared on the launcher's own gy and sums, so that its error is its own (the model accepts sums that are within the
    # launcher's bound of its graph's own)
    ref_d = _scatter_model(c, torch.float64, got["gy"].cpu(), got["sumsy"].cpu(), tol=max(bound["sumsy"], err["sumsy"]))
    for (q, a), b, n32, n64 in zip(_pqr_blocks(got["dPQR"], H, F_).items(), _pqr_blocks(ref_d, H, F_).values(),
                                   _pqr_blocks(m32["dPQR"], H, F_).values(), _pqr_blocks(m64["dPQR"], H, F_).values()):
        err[q], bound[q] = em.rel(a, b), max(BWD, 5.0 * em.rel(n32, n64))
    print("B %d N %d k %d H %d F %d hand %s seed %d: %s" % (B, N, k, H, F_, hand, c["seed"], {q: "%.2e" % v for q, v in err.items()}))
    for q in err:
        assert err[q] <= bound[q], (q, err[q], bound[q])
    # the CSR holds the builder's in-degrees, in-edges in ascending edge order
    assert torch.equal((got["rowptr"][1:] - got["rowptr"][:-1]).cpu().long(), c["indeg"])
    assert torch.equal(got["src"].cpu(), km.csr_build(c["idx"].to(torch.int32), B, N)[1])
    if hand:
        deg = c["indeg"].view(B, N)
        assert bool((deg[:, em.LONELY] == 0).all()) and bool((deg[:, em.HUB] == N + k - 1).all())
        for t, d in enumerate(em.hand_targets(N, k)):
            assert bool((deg[:, 3 + t] == d).all()), d
        dQ = got["dPQR"].view(B, N, H + 2 * F_)[:, em.LONELY, H:H + F_]
        assert torch.equal(dQ, torch.zeros_like(dQ))                            # gathered by nobody: exactly 0
    if k == 1:                                                                  # a softmax over one logit is 1: exact
        assert torch.equal(got["g2"], torch.zeros_like(got["g2"]))
        j = c["idx"].reshape(-1)
        yp = (c["PQR"][:, H + F_:] + c["PQR"][j, H:H + F_]) + c["bx"]           # float32, the kernel's order
        zyf = (yp.double() * c["scx"].double() + c["shx"].double()).float()     # fmaf: the exact product, one rounding of the sum
        assert torch.equal(got["T"].cpu(), torch.where(zyf > 0, zyf, zyf * torch.tensor(c["slope"], dtype=torch.float32)))
    again = _launch(ops, c)
    for q in ("mean", "var", "T", "g2", "gy", "sums2", "sumsy", "dPQR", "rowptr", "src"):
        assert torch.equal(got[q], again[q]), q                                 # two runs are bit-identical


@pytest.mark.parametrize("B,N,k,H,F_", em.SPECIAL_CASES)
def test_softmax_range(sp, B, N, k, H, F_):
    """Every fourth column of h2pre is scaled so that the logits span about +-120: expf overflows near 88.7, so a softmax without the max
    subtraction gives inf or NaN.  T, g2 and gy are finite and within the tolerance rule."""
    c = em.find_launcher_case(B, N, k, H, F_, True, "softmax")
    (m64, z2, _), (m32, _, _) = _model(c, torch.float64), _model(c, torch.float32)
    assert float(z2.abs().max()) > 100.0
    got = _launch(sp.ops, c, scatter=False)
    err = {}
    for q, base in (("T", FWD), ("g2", BWD), ("gy", BWD)):
        assert bool(torch.isfinite(got[q]).all()), q
        err[q] = em.rel(got[q], m64[q])
        bound = max(base, 5.0 * em.rel(m32[q], m64[q]))
        print("softmax range k %d %s: rel-L2 %.2e (bound %.2e)" % (k, q, err[q], bound))
    for q, base in (("T", FWD), ("g2", BWD), ("gy", BWD)):
        assert err[q] <= max(base, 5.0 * em.rel(m32[q], m64[q])), (q, err[q])


@pytest.mark.parametrize("B,N,k,H,F_", em.SPECIAL_CASES)
def test_offset_columns(sp, B, N, k, H, F_):
    """b1 and bx are 50 in every fifth column, P, Q and R spread over 0.05: a sum-of-squares variance without the tile shift would lose
    every digit (50^2 against a variance of 1e-3 is 2e6, times float32's 6e-8); edge_stats stays within the rule against float64."""
    c = em.find_launcher_case(B, N, k, H, F_, True, "offset")
    t = lambda n, dt: c[n].to(dt)
    m64 = em.stats(t("PQR", torch.float64), c["idx"], t("b1", torch.float64), t("bx", torch.float64))
    m32 = em.stats(t("PQR", torch.float32), c["idx"], t("b1", torch.float32), t("bx", torch.float32))
    got = sp.ops.edge_stats(c["PQR"].cuda(), c["idx"].to(torch.int32).cuda(), c["b1"].cuda(), c["bx"].cuda())
    for q, a, r32, r64 in zip(("mean", "var"), got, m32, m64):
        e, bound = em.rel(a, r64), max(FWD, 5.0 * em.rel(r32, r64))
        print("offset columns k %d %s: rel-L2 %.2e (bound %.2e)" % (k, q, e, bound))
        assert e <= bound, (q, e, bound)
    off = torch.cat([torch.arange(0, H, 5), H + torch.arange(0, F_, 5)])        # the offset columns on their own
    e = em.rel(got[1][off], m64[1][off])
    print("offset columns k %d var of the offset columns alone: rel-L2 %.2e" % (k, e))
    assert e <= max(FWD, 5.0 * em.rel(m32[1][off], m64[1][off])), e


@pytest.mark.parametrize("Fin,Fout,k,B,N", em.MODULE_CASES)
def test_module_against_float64_autograd(sp, Fin, Fout, k, B, N):
    """spgan.EdgeBlock, train mode, the constructed graph injected as int64, forward and backward through EdgeBlockFn: output, dx, every
    parameter gradient, the running buffers and num_batches_tracked against edgeblock_model.block in float64 + autograd."""
    c = em.find_module_case(Fin, Fout, k, B, N)
    m64, m32 = c["m64"], em.run_block(c, torch.float32)
    blk = sp.EdgeBlock(Fin, Fout, k)
    blk.load_state_dict({**blk.state_dict(), **{n: v.detach().clone() for n, v in c["params"].items()}})
    blk = blk.cuda().train()
    x = c["x"].cuda().requires_grad_(True)
    loc = (c["idx"].view(B, N * k) - (torch.arange(B) * N).view(B, 1)).cuda()
    out = blk(x, idx=loc)
    assert torch.equal(blk.last_idx.cpu().long(), c["idx"])
    (out * c["dy"].cuda()).sum().backward()
    noise = lambda q: em.rel(m32[q], m64[q])
    err = {"out": em.rel(out, m64["out"]), "dx": em.rel(x.grad, m64["dx"])}
    bound = {"out": max(3e-6, 5.0 * noise("out")), "dx": max(3e-6, 5.0 * noise("dx"))}
    for n, p in blk.named_parameters():
        if n in ZERO_GRAD_BIASES:                                               # exact zeros in float64 up to rounding: absolute bound only
            assert float((p.grad.cpu().double() - m64["grad|" + n]).abs().max()) <= 2e-3, n
            continue
        err[n], bound[n] = em.rel(p.grad, m64["grad|" + n]), max(5e-6, 5.0 * noise("grad|" + n))
    print("Fin %d Fout %d k %d B %d N %d seed %d: %s" % (Fin, Fout, k, B, N, c["seed"], {q: "%.2e" % v for q, v in err.items()}))
    for q in err:
        assert err[q] <= bound[q], (q, err[q], bound[q])
    sd = blk.state_dict()
    for bn in em.BN_LAYERS:
        for s in ("running_mean", "running_var"):
            np.testing.assert_allclose(sd[bn + "." + s].cpu().numpy(), m64["buf|" + bn + "." + s].numpy(), rtol=1e-5, atol=1e-6, err_msg=bn + "." + s)
        assert int(sd[bn + ".num_batches_tracked"]) == int(m64["buf|" + bn + ".num_batches_tracked"]) == 1
