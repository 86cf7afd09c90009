"""GPU: AdaptivePointNorm in the epilogue of its style GEMM (spgan/adain_epi.py, SPGAN_EPI_ADAIN) against the chain it replaces,
gemm_nt -> colstats -> adain_fwd (-> maxpool), on seeded inputs.

Equality rule.  The fused launch runs the GEMM main loop of the kernel the chain's GEMM runs (256 x 256 tiles where `tile_hint` forces both
there), or -- 128-row kernel -- its 128-column configuration where the chain's GEMM picks the 64-column one for K < 512.  Those two
configurations differ only in how many column tiles a wave owns: every accumulator element sees the same k-tiles of 32, the same MFMA
sequence inside a tile and the same operand values, so the sums are bit-identical and no configuration has to be forced.  The epilogue's
expressions are those of the GEMM's bias add and of adain_fwd_kernel.  Hence torch.equal everywhere; no case needs a float64 bound."""
import pytest
import torch

from spgan import fixture_rng as fr
from test_kernels_gpu import rnd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from spgan import _lib, adain_epi, nets, ops
    _lib.load()
    return ops, adain_epi, nets


def _inputs(tag, C, K, B, N):
    M = B * N
    return dict(style=rnd(tag + ".style", (M, K)), Ws=rnd(tag + ".Ws", (2 * C, K), 0.1), bs=rnd(tag + ".bs", (2 * C,), 0.5), x=rnd(tag + ".x", (M, C)),
                C=C, K=K, B=B, N=N, M=M)


def _chain(ops, d, slope, hint, x=None):
    x = d["x"] if x is None else x
    with ops.nt_tile_hint(hint):
        gb = ops.gemm_nt(d["style"], d["Ws"], d["bs"])
    imean, ivar = ops.colstats(x, d["N"], slope)
    imean, ivar = imean.contiguous(), ivar.contiguous()
    return ops.adain_fwd(x, d["N"], slope, imean, ivar, gb), gb, imean, ivar


def _fused(ops, ae, d, slope, hint, imean, ivar, x=None, **kw):
    x = d["x"] if x is None else x
    assert ae.usable(x, d["style"], d["Ws"], d["N"])
    with ops.nt_tile_hint(hint):
        return ae.forward(x, d["style"], d["Ws"], d["bs"], d["N"], slope, imean, ivar, **kw)


# (tag, C, K, B, N, tile_hint): the 256 x 256-tile kernel (M = 512; M = 768: 3 row tiles, so 5 of the 8 workgroups of the XCD map idle) and
# the 128-row kernel (whole tiles; M = 320: a row tail and shapes that straddle tiles; K = 36: a k-tail)
CASES = [("wide2", 128, 128, 2, 256, 2), ("wide3", 128, 128, 3, 256, 2), ("row3", 64, 128, 3, 128, 0), ("tail", 64, 128, 2, 160, 0), ("k36", 64, 36, 2, 128, 0)]


@pytest.mark.parametrize("slope", [1.0, 0.2])
@pytest.mark.parametrize("tag,C,K,B,N,hint", CASES)
def test_fused_equals_chain(mods, tag, C, K, B, N, hint, slope):
    """out, the kept gamma rows (second half) and -- where the shapes allow records -- the pooled maximum and its row."""
    ops, ae, _ = mods
    d = _inputs("ade." + tag, C, K, B, N)
    M = d["M"]
    if hint == 2:                                   # the forced geometry must be the one that runs: the 256 x 256-tile kernel takes these sizes
        assert M % 256 == 0 and (2 * C) % 256 == 0 and K % 32 == 0
    want, gb, imean, ivar = _chain(ops, d, slope, hint)
    pool = ae.can_pool(M, N)
    assert pool == (N % 128 == 0)
    r0 = (M // 2) if B % 2 == 0 else N              # second half of the rows (odd B: everything behind the first shape)
    out, gamma, rec = _fused(ops, ae, d, slope, hint, imean, ivar, gamma_row0=r0, pool=pool)
    assert torch.equal(out, want), "out: max |diff| %.3e" % (out - want).abs().max().item()
    assert gamma.shape == (M - r0, C) and torch.equal(gamma, gb[r0:, :C])
    gmax, garg = ops.maxpool(want, B, N)
    if pool:
        pm, pa = ae.pool_from_records(rec, B, N)
        assert torch.equal(pm, gmax) and torch.equal(pa, garg)
    else:                                           # N % 128 != 0: no records; the max-pool kernel on the fused output stays the route
        with pytest.raises(ValueError):
            _fused(ops, ae, d, slope, hint, imean, ivar, pool=True)
        pm, pa = ops.maxpool(out, B, N)
        assert torch.equal(pm, gmax) and torch.equal(pa, garg)


def test_pool_fallback_in_host_route(mods):
    """nets.adain_forward asked for records at N % 128 != 0: fused output, no records (the caller's max-pool launch stays), right result."""
    ops, ae, nets = mods
    d = _inputs("ade.tail", 64, 128, 2, 160)
    P = {"a.style.weight": d["Ws"], "a.style.bias": d["bs"]}
    out, ctx = nets.adain_forward(P, "a", d["x"], d["style"], d["N"], 0.2, fused=dict(gamma_row0=d["M"] // 2, pool=True))
    assert ctx["gamma"] is not None and ctx["gb"] is None and ctx["pool"] is None
    want = _chain(ops, d, 0.2, 0)[0]
    assert torch.equal(out, want)
    a, b = ops.maxpool(out, d["B"], d["N"]), ops.maxpool(want, d["B"], d["N"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("tag,C,K,B,N,hint", [("bwide", 128, 128, 2, 256, 2), ("brow", 64, 128, 3, 128, 0), ("btail", 64, 128, 2, 160, 0)])
def test_broadcast_x(mods, tag, C, K, B, N, hint):
    """Per-shape stride 0 (every shape reads one [N,C] block) against the same launch on the materialised repeat; the statistics of the
    one copy are those of every copy."""
    ops, ae, _ = mods
    d = _inputs("ade." + tag, C, K, B, N)
    x_one = d["x"][:N].contiguous()
    x_rep = x_one.repeat(B, 1)
    for slope in (1.0, 0.2):
        m1, v1 = ops.colstats(x_one, N, slope)
        mr, vr = ops.colstats(x_rep, N, slope)
        imean, ivar = m1.expand(B, C).contiguous(), v1.expand(B, C).contiguous()
        assert torch.equal(imean, mr) and torch.equal(ivar, vr)
        o1, g1, _ = _fused(ops, ae, d, slope, hint, imean, ivar, x=x_one, gamma_row0=0)
        o2, g2, _ = _fused(ops, ae, d, slope, hint, imean, ivar, x=x_rep, gamma_row0=0)
        assert torch.equal(o1, o2) and torch.equal(g1, g2)
        assert torch.equal(o1, _chain(ops, d, slope, hint, x=x_rep)[0])
        dout = rnd("ade.dout." + tag, (B * N, C))
        for a, b in zip(ae.backward(dout, x_one, N, slope, imean, ivar, g1), ae.backward(dout, x_rep, N, slope, imean, ivar, g1)):
            assert torch.equal(a, b)


@pytest.mark.parametrize("tag,C,K,N,hint", [("pwide", 128, 128, 256, 2), ("prow", 64, 128, 256, 0)])
def test_pool_ties_and_last_row(mods, tag, C, K, N, hint):
    """Constructed ties: identical (style, x) rows give identical outputs.  Shape 0: rows 128.. repeat rows 0..127 -- every channel's maximum
    occurs twice, in different record tiles.  Shape 1: rows 64..127 repeat rows 0..63 -- ties inside one tile.  The smaller row must win, as
    in ops.maxpool.  Shape 2: its last row is made the maximum of every channel whose style bias is not tiny."""
    ops, ae, _ = mods
    B = 3
    d = _inputs("ade." + tag, C, K, B, N)
    style, x = d["style"], d["x"]
    style[128:256] = style[0:128]; x[128:256] = x[0:128]
    style[N + 64:N + 128] = style[N:N + 64]; x[N + 64:N + 128] = x[N:N + 64]
    last = 3 * N - 1
    style[last] = 0.0                                                  # gamma = its bias there; an outlier x of the bias's sign: a large gamma*xhat
    x[last] = torch.where(d["bs"][:C] >= 0, torch.tensor(50.0, device=x.device), torch.tensor(-50.0, device=x.device))
    want, gb, imean, ivar = _chain(ops, d, 1.0, hint)
    gmax, garg = ops.maxpool(want, B, N)
    ties0 = (want[:N] == gmax[0]).sum(0)
    assert (ties0 >= 2).all() and (garg[0] < 128).all()                # different tiles, every channel
    in_tile = (garg[1] - N < 64)                                       # maxima inside the repeated 64 rows: a tie within one tile
    assert in_tile.any() and ((want[N:2 * N] == gmax[1]).sum(0)[in_tile] >= 2).all()
    assert (garg[2] == last).sum().item() >= C // 2                    # the maximum in the last row of a shape
    out, _, rec = _fused(ops, ae, d, 1.0, hint, imean, ivar, pool=True)
    pm, pa = ae.pool_from_records(rec, B, N)
    assert torch.equal(out, want) and torch.equal(pm, gmax) and torch.equal(pa, garg)


@pytest.mark.parametrize("tag,C,K,B,N,hint", [("gwide", 128, 128, 2, 256, 2), ("grow", 64, 128, 2, 128, 0), ("gtail", 64, 128, 2, 160, 0)])
def test_gamma_store_feeds_backward(mods, tag, C, K, B, N, hint):
    """gamma kept for exactly the second half of the rows: adain_bwd on it = adain_bwd on the full [M,2C] tensor, rows of that half."""
    ops, ae, _ = mods
    d = _inputs("ade." + tag, C, K, B, N)
    M, h, hb = d["M"], d["M"] // 2, B // 2
    slope = 0.2
    want, gb, imean, ivar = _chain(ops, d, slope, hint)
    out, gamma, _ = _fused(ops, ae, d, slope, hint, imean, ivar, gamma_row0=h)
    assert torch.equal(out, want) and torch.equal(gamma, gb[h:, :C])
    dout = rnd("ade.dout." + tag, (M, C))
    dx_w, dgb_w = ops.adain_bwd(dout, d["x"], N, slope, imean, ivar, gb)
    dx, dgb = ae.backward(dout[h:].contiguous(), d["x"][h:].contiguous(), N, slope, imean[hb:].contiguous(), ivar[hb:].contiguous(), gamma)
    assert torch.equal(dx, dx_w[h:]) and torch.equal(dgb, dgb_w[h:])


def test_g_pair_forward_routes_agree(mods):
    """nets.g_pair_forward at B = 2, N = 256, fused route against chain route: the clouds of both passes, pass 1's saved contexts as the
    backward consumes them (and the parameter gradients that backward produces), the generator's BatchNorm running statistics."""
    ops, ae, nets = mods
    import spgan
    from oracle import spgan_oracle as orc

    class O:
        np = 256; nk = 20; nz = 128; softmax = True; off = False; attn = False; use_head = False; eql = False; z_norm = False; small_d = False
    B, N = 2, 256
    M = B * N
    x = fr.sphere_template(N)[None].repeat(B, 1, 1).cuda()
    z_d = fr.latent(B, N, seed=5)[:, :1, :].contiguous().cuda()
    z_g = fr.latent(B, N, seed=6)[:, :1, :].contiguous().cuda()
    w = rnd("ade.e2e.w", (M, 3))
    runs = []
    real_pair = nets.g_pair_forward
    for on in (True, False):
        G = spgan.Generator(O)
        G.load_state_dict({**G.state_dict(), **fr.init_params(orc.generator_shapes(), salt=3)})
        G.cuda().train()
        assert G.pair_ok(x, z_d, z_g)
        got = {}
        nets.g_pair_forward = lambda *a, **k: got.setdefault("pre", real_pair(*a, **k))
        try:
            with ae.route(on):
                fake_d, fake_g = G.forward_pair(x, z_d, z_g)
                (fake_g * w).sum().backward()
        finally:
            nets.g_pair_forward = real_pair
        runs.append((fake_d.detach(), fake_g.detach(), got["pre"], {k: v.clone() for k, v in G.state_dict().items()},
                     {n: p.grad.clone() for n, p in G.named_parameters() if p.grad is not None}))
    (fd_a, fg_a, pa, sa, ga), (fd_b, fg_b, pb, sb, gb_) = runs
    assert torch.equal(fd_a, fd_b) and torch.equal(fg_a, fg_b)
    for name, C in (("adain1", 64), ("adain2", 128)):
        (oa, ca), (ob, cb) = pa[name], pb[name]
        assert ca["gb"] is None and ca["gamma"] is not None and cb["gb"] is not None, name   # the routes that were asked for did run
        assert torch.equal(oa, ob), name
        assert torch.equal(ca["gamma"], cb["gb"][:, :C]) and torch.equal(ca["imean"], cb["imean"]) and torch.equal(ca["ivar"], cb["ivar"]), name
        xa = ca["x"] if ca["x"].shape[0] == M else ca["x"].repeat(B, 1)
        assert torch.equal(xa, cb["x"]) and torch.equal(ca["style"], cb["style"]), name
    assert pa["adain1"][1]["x"].shape[0] == N                        # AdaIN-1 read the one shared block
    ga_, gb2 = pa["tail"][1], pb["tail"][1]
    for k in ("gmax", "garg", "y0", "y3"):
        assert torch.equal(ga_[k], gb2[k]), k
    assert torch.equal(pa["ec2"][0], pb["ec2"][0]) and torch.equal(pa["tail"][0], pb["tail"][0])
    assert sa.keys() == sb.keys() and ga.keys() == gb_.keys() and len(ga) > 10
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for k in ga:
        assert torch.equal(ga[k], gb_[k]), k
