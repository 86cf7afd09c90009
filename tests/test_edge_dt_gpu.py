"""GPU: spgan_edge_attend_bwd_dt (csrc/edge_dt.hip) -- EdgeConv2's attention backward with dT = dout . WoT formed in the launch's
accumulators -- against the chain it replaces, bit for bit.

The reference of every comparison is the existing chain on the same inputs, never the new kernel:
    ops.edge_attend_bwd(ops.gemm_nt(dout, WoT), ...)   under ops.nt_tile_hint(2)   (the 256 x 256-tile kernel, as in the train step).
Everything is compared with torch.equal: the fused launch is specified as the chain's bits (the k-order of every accumulator, the shared
per-element expressions of edge_attend.hpp, the records' summation order), so there is no tolerance to choose.

Shapes: the smallest the 256 x 256-tile kernel takes, (B, N) = (1, 256), (2, 256), (3, 256) with k = 10, F = 128, H = 64 -- 8, 16 and 24
workgroups of 32 points; at M = 768 the chain's product has three row tiles on a grid of eight (logical blocks past the end).  Inputs:
N(0,1) dout and PQR; h2pre N(0,1) with every 16th column scaled x30 (a saturated softmax: one weight 1, the others underflow); BatchNorm
scales of both signs (both LeakyReLU branches and masks); neighbour lists per shape that hold the point itself, a repeated neighbour and
the shape's first and last row.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
K, F, H = 10, 128, 64
SLOPE = 0.2
SHAPES = [(1, 256), (2, 256), (3, 256)]


@pytest.fixture(scope="module")
def sp():
    import spgan
    from spgan import _lib
    _lib.load()
    return spgan


def _inputs(B, N):
    g = torch.Generator().manual_seed(1000 * B + N)
    M = B * N
    r = lambda *s: torch.randn(*s, generator=g)
    c = {"dout": r(M, F), "WoT": r(K * F, F) * 0.1, "PQR": r(M, H + 2 * F), "h2pre": r(M * K, F)}
    c["h2pre"][:, ::16] *= 30.0
    sign = lambda n: torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    for n in ("sc2", "scx"):
        c[n] = (0.5 + torch.rand(F, generator=g)) * sign(F)
    for n in ("sh2", "shx", "bx", "mean2", "meanx"):
        c[n] = r(F) * 0.3
    for n in ("inv2", "invx"):
        c[n] = 0.5 + torch.rand(F, generator=g)
    idx = torch.randint(0, N, (B, N, K), generator=g)
    idx[:, :, 0] = torch.arange(N).view(1, N)          # the point itself
    idx[:, :, 2] = idx[:, :, 1]                        # a repeated neighbour
    idx[:, 1::7, 3] = 0                                # the shape's first row
    idx[:, 2::5, 4] = N - 1                            # ... and its last
    idx[:, 0, 5:] = N - 1
    idx[:, N - 1, 5:] = 0
    c["idx"] = (idx + (torch.arange(B) * N).view(B, 1, 1)).reshape(M, K).to(torch.int32)
    return {n: v.cuda().contiguous() for n, v in c.items()}


_CASES = {}


def _case(sp, B, N):
    """Inputs and the chain's results for one shape: computed once, shared by the tests, never modified."""
    if (B, N) not in _CASES:
        c = _inputs(B, N)
        with sp.ops.nt_tile_hint(2):
            assert sp.ops.edge_attend_bwd_dt_selected(c["dout"], c["WoT"], K, F)
            dT = sp.ops.gemm_nt(c["dout"], c["WoT"])
        ref = sp.ops.edge_attend_bwd(dT, *_tail(c))
        torch.cuda.synchronize()
        _CASES[(B, N)] = (c, ref)
    return _CASES[(B, N)]


def _tail(c):
    return (c["h2pre"], c["sc2"], c["sh2"], c["mean2"], c["inv2"], c["PQR"], c["idx"], c["bx"], c["scx"], c["shx"], c["meanx"], c["invx"], SLOPE)


@pytest.mark.parametrize("B,N", SHAPES)
def test_bit_equal_to_the_chain(sp, B, N):
    c, ref = _case(sp, B, N)
    got = sp.ops.edge_attend_bwd_dt(c["dout"], c["WoT"], *_tail(c))
    for name, a, b in zip(("g2", "gy", "sums2", "sumsy"), got, ref):
        assert bool(torch.isfinite(b).all()), name
        assert a.shape == b.shape and torch.equal(a, b), (name, int((a != b).sum()), float((a - b).abs().max()))
    # the inputs do what they are for: a saturated softmax, both LeakyReLU branches of both activations
    z2 = c["h2pre"] * c["sc2"] + c["sh2"]
    zy = ((c["PQR"][:, H + F:].repeat_interleave(K, 0) + c["PQR"][c["idx"].reshape(-1).long(), H:H + F]) + c["bx"]) * c["scx"] + c["shx"]
    assert float(z2.abs().max()) > 60.0
    for z in (z2, zy):
        assert bool((z > 0).any(0).all()) and bool((z < 0).any(0).all())


def test_two_launches_give_equal_bytes(sp):
    c, _ = _case(sp, 3, 256)
    p1, p2 = [], []
    a = sp.ops.edge_attend_bwd_dt(c["dout"], c["WoT"], *_tail(c), _part_out=p1)
    b = sp.ops.edge_attend_bwd_dt(c["dout"], c["WoT"], *_tail(c), _part_out=p2)
    for x, y in zip(a + (p1[0],), b + (p2[0],)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def _block_grads(sp, Fout, B=2, N=256, Fin=16, cpu_state=None):
    """spgan.EdgeBlock forward + backward (train mode, its own kNN graph) -> (state, [out, dx, parameter gradients...])."""
    torch.manual_seed(7)
    blk = sp.EdgeBlock(Fin, Fout, K)
    if cpu_state is not None:
        blk.load_state_dict(cpu_state)
    state = {n: v.clone() for n, v in blk.state_dict().items()}
    blk = blk.cuda().train()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, Fin, N, generator=g).cuda().requires_grad_(True)
    dy = torch.randn(B, Fout, N, generator=g).cuda()
    out = blk(x)
    (out * dy).sum().backward()
    torch.cuda.synchronize()
    return state, [out.detach(), x.grad] + [p.grad for _, p in sorted(blk.named_parameters())]


def test_route_on_equals_route_off(sp):
    """nets.edgeblock_backward through spgan.EdgeBlock at (2, 256), F = 128: the fused launch against the chain, every gradient bit-equal."""
    from spgan import edge_dt
    with sp.ops.nt_tile_hint(2):
        n0 = edge_dt.LAUNCHES[0]
        with edge_dt.route(True):
            state, on = _block_grads(sp, F)
        assert edge_dt.LAUNCHES[0] == n0 + 1
        with edge_dt.route(False):
            _, off = _block_grads(sp, F, cpu_state=state)
        assert edge_dt.LAUNCHES[0] == n0 + 1
    assert len(on) == len(off) > 10
    for i, (a, b) in enumerate(zip(on, off)):
        assert torch.equal(a, b), i


def test_chain_runs_where_the_predicate_is_false(sp):
    """F = 64, tile_hint 1, the split-bf16 operand mode and CPU tensors keep the chain: no fused launch is counted."""
    from spgan import edge_dt
    ops = sp.ops
    n0 = edge_dt.LAUNCHES[0]
    with ops.nt_tile_hint(2):
        _, g = _block_grads(sp, 64)                                     # EdgeConv1's width
        assert edge_dt.LAUNCHES[0] == n0 and all(bool(torch.isfinite(t).all()) for t in g)
    with ops.nt_tile_hint(1):                                           # the 128-row kernels sum in another order
        _, g = _block_grads(sp, F)
        assert edge_dt.LAUNCHES[0] == n0 and all(bool(torch.isfinite(t).all()) for t in g)
    prev = ops.get_mfma_operands()
    try:
        ops.set_mfma_operands("bf16x3")
        with ops.nt_tile_hint(2):
            _, g = _block_grads(sp, F)
        assert edge_dt.LAUNCHES[0] == n0 and all(bool(torch.isfinite(t).all()) for t in g)
    finally:
        ops.set_mfma_operands(prev)
    c, _ = _case(sp, 1, 256)
    with ops.nt_tile_hint(2):
        assert edge_dt.usable(c["dout"], c["WoT"], c["dout"], c["h2pre"], c["PQR"], K, F)
        assert not edge_dt.usable(c["dout"].cpu(), c["WoT"].cpu(), c["dout"].cpu(), c["h2pre"].cpu(), c["PQR"].cpu(), K, F)
        assert not edge_dt.usable(c["dout"][:, :64], c["WoT"][:640, :64], c["dout"], c["h2pre"], c["PQR"], K, 64)
        with edge_dt.route(False):
            assert not edge_dt.usable(c["dout"], c["WoT"], c["dout"], c["h2pre"], c["PQR"], K, F)
    with ops.nt_tile_hint(1):
        assert not edge_dt.usable(c["dout"], c["WoT"], c["dout"], c["h2pre"], c["PQR"], K, F)
    # the fused route is the default where it applies: a further block backward counts one launch
    with ops.nt_tile_hint(2):
        _block_grads(sp, F)
    assert edge_dt.LAUNCHES[0] == n0 + 1


def test_argument_checks(sp):
    """Null or misaligned pointers, k != 10 and F != 128 return the library's -22 before any launch."""
    from spgan import _lib
    lib = _lib.load()
    c, _ = _case(sp, 1, 256)
    M = 256
    g2 = torch.empty(M * K, F, device="cuda"); gy = torch.empty_like(g2)
    part = torch.empty(M // 32, 2 * F, 2, device="cuda")
    p = lambda t: t.data_ptr()
    vec = [p(c[n]) for n in ("sc2", "sh2", "mean2", "inv2")]
    tail = [p(c[n]) for n in ("bx", "scx", "shx", "meanx", "invx")]

    def call(dout=p(c["dout"]), WoT=p(c["WoT"]), h2=p(c["h2pre"]), k=K, F_=F, M_=M, g2p=p(g2), idx=p(c["idx"])):
        return lib.spgan_edge_attend_bwd_dt(dout, F, WoT, F, h2, *vec, p(c["PQR"]), H + 2 * F, H, F_, idx, M_, k, *tail, SLOPE, g2p, p(gy), p(part),
                                            None)
    assert call(dout=None) == -22 and call(WoT=None) == -22 and call(h2=None) == -22 and call(g2p=None) == -22 and call(idx=None) == -22
    assert call(dout=p(c["dout"]) + 4) == -22 and call(WoT=p(c["WoT"]) + 8) == -22 and call(h2=p(c["h2pre"]) + 2) == -22
    assert call(k=9) == -22 and call(k=11) == -22 and call(F_=64) == -22 and call(M_=0) == -22 and call(M_=100) == -22
    assert lib.spgan_edge_attend_bwd_dt_selected(None, F, p(c["WoT"]), F, M, K, F, 2) == 0
    assert lib.spgan_edge_attend_bwd_dt_selected(p(c["dout"]), F, p(c["WoT"]), F, M, 9, F, 2) == 0
    assert lib.spgan_edge_attend_bwd_dt_selected(p(c["dout"]) + 4, F, p(c["WoT"]), F, M, K, F, 2) == 0
    assert lib.spgan_edge_attend_bwd_dt_selected(p(c["dout"]), F, p(c["WoT"]), F, M, K, F, 1) == 0
    torch.cuda.synchronize()
