"""GPU: peak memory of a block's forward + backward against what a user wrote before the blocks existed -- the same spgan layer object
with the reference's tail in torch, in the reference's order (the global branch, then the layer, batch_norm, leaky_relu, repeat, cat and
add_cov where the block has one): the composition that tools/blocks_bench.py measures at full size.

The peak of either route lies inside the layer's backward, which both share, and in both the global branch's backward runs after it
(autograd runs a graph's nodes latest first).  What differs is what each route keeps alive across it.  The torch route keeps the saved
tensors of torch.max, fc and g_fc: int64 indices, every Linear's input, every BatchNorm's input and every LeakyReLU's result.  The block
keeps an int32 arg-max, the pre-norm products and the rows of xs, but neither the activated rows between the layers (its products
re-apply the affine and the LeakyReLU to their operand) nor g (formed again in backward); its tail's tensors are saved tensors, gone
with the tail's backward.  That is less at every shape, so the bound is strict:
the block's peak is below the baseline's, in the bytes the code requests from the caching allocator (requested_bytes: the sum of the
live tensors' sizes; max_memory_allocated counts the allocator's blocks, which it hands out up to 1 MiB larger than asked for, depending
on the order of earlier frees)."""
import pytest
import torch
import torch.nn.functional as F_

pytestmark = pytest.mark.gpu

# (block, constructor arguments, B, N, takes pc): a concatenating two-output block and a middle block (add_cov) with g_out
SHAPES = [("bilateral_block_l2", (16, 32, 128, 1, 8), 4, 128, True),
          ("deform_block_feat", (32, 32, 1, 8), 8, 256, False)]


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_stats()["requested_bytes.all.current"]
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.memory_stats()["requested_bytes.all.peak"] - base


@pytest.mark.parametrize("name,args,B,N,takes_pc", SHAPES, ids=[s[0] for s in SHAPES])
def test_block_peak_memory_below_torch_tail(name, args, B, N, takes_pc):
    import spgan
    g = torch.Generator().manual_seed(0)
    m = getattr(spgan, name)(*args).cuda().train()
    layer, bn, _ = m._parts()
    g_fc, add_cov = getattr(m, "g_fc", None), getattr(m, "add_cov", None)
    x = (torch.randn(B, layer.Fin, N, generator=g) * 0.7).cuda().requires_grad_(True)
    pc = (torch.rand(B, 3, N, generator=g) * 2 - 1).cuda().requires_grad_(True) if takes_pc else None
    with torch.no_grad():
        _, idx = spgan.get_edge_features(x.detach(), layer.k, return_idx=True)
    idx = spgan.ops.idx_from_local64(idx, B, N, layer.k)

    def block():
        return m(x, pc, idx=idx) if takes_pc else m(x, idx=idx)

    def baseline():
        xs = m.fc(torch.max(x, 2)[0])
        gv = g_fc(xs)
        y = layer(x, pc, idx=idx) if takes_pc else layer(x, idx=idx)
        L = y.shape[2]
        x_ec = F_.leaky_relu(F_.batch_norm(y, None, None, bn.weight, bn.bias, True, 0.1, 1e-5), 0.01)
        x_out = torch.cat((xs.view(B, -1, 1).repeat(1, 1, L), x_ec), 1)
        g_out = torch.cat((gv.view(B, -1, 1).repeat(1, 1, L), x_ec), dim=1)
        return (x_out if add_cov is None else add_cov(x_out)), g_out
    with torch.no_grad():
        cots = [torch.randn(o.shape, generator=g).cuda() for o in block()]

    def step(fn):
        def run():
            x.grad = None
            if pc is not None:
                pc.grad = None
            for p in m.parameters():
                p.grad = None
            outs = fn()
            sum((o * c).sum() for o, c in zip(outs, cots)).backward()
        return run
    for fn in (block, baseline):                # operand images, workspaces and lazily loaded code are paid once, outside the figure
        step(fn)()
    peak_block, peak_base = _peak(step(block)), _peak(step(baseline))
    print("%s: block %d bytes, torch tail %d bytes, difference %d" % (name, peak_block, peak_base, peak_block - peak_base))
    assert peak_block < peak_base
