"""GPU: block_tail_bwd_reduce without the broadcast channels' row sums (want_dxs / want_dg = False, what BlockTailFn asks for when xs / g
need no gradient): the sums of the data channels are bit-identical to the full launch's, and the unwanted outputs are None."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,C,L,Cs,Cg", [(3, 5, 23, 7, 4), (2, 16, 48, 16, 512)], ids=["scalar", "vector"])
def test_reduce_without_row_sums(B, C, L, Cs, Cg):
    from spgan import block_tail as bt
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g).cuda()                                        # noqa: E731
    Y, dx, dg = rnd(B, C, L), rnd(B, Cs + C, L), rnd(B, Cg + C, L)
    scale, shift, mean, invstd = rnd(C), rnd(C), rnd(C), rnd(C).abs() + 0.5
    full = bt.block_tail_bwd_reduce(Y, dx, dg, None, Cs, Cg, scale, shift, mean, invstd)
    for want_dxs, want_dg in ((False, True), (True, False), (False, False)):
        sums, dxs, dgs = bt.block_tail_bwd_reduce(Y, dx, dg, None, Cs, Cg, scale, shift, mean, invstd, want_dxs=want_dxs, want_dg=want_dg)
        assert torch.equal(sums, full[0])
        assert (dxs is None) == (not want_dxs) and (dgs is None) == (not want_dg)
        if want_dxs:
            assert torch.equal(dxs, full[1])
        if want_dg:
            assert torch.equal(dgs, full[2])
