"""CPU: the bilateral / deform blocks (tests/blocks_model.py: the layer models with the blocks' global branch, BatchNorm1d + LeakyReLU,
concatenation and add_cov around them) against the vectors captured from the reference's blocks (golden blocks.npz / blocks2.npz); the
written-out backward of the block-tail launchers' model against autograd; the modules' parameter layout against the reference's; what the
modules refuse.

Tolerances, as tests/test_bilateral_cpu.py.  float64: the model runs in float64 on float32 inputs, the golden holds the reference's float64
run on the same inputs and graph (its distance from the float32 run stored with enough mantissa bits to stay within 1e-10 of the value):
1e-9 rel-L2.
float32: within 5 x the reference's own float32-vs-float64 distance of that quantity.  A conv / linear bias in front of a train-mode
BatchNorm has a gradient that is zero up to rounding in both, compared absolutely (1e-12 in float64, times the layer's weight gradient / 100 where that is larger; 2e-3 in float32)."""
import pytest
import torch

import blocks_model as km

TAGS = list(km.CASES)


@pytest.fixture(scope="module")
def d():
    return km.load_golden()


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _module(d, tag):
    """the spgan block of the case, holding the reference's checkpoint (strict loading)"""
    import spgan
    m = km.make_module(km.CASES[tag], spgan)
    m.load_state_dict(km.golden_state_dict(d, tag), strict=True)
    return m


@pytest.fixture(scope="module")
def runs(d):
    """The model's float64 and float32 results per case, computed once, on the parameters and buffers as the module holds them after
    loading the reference's checkpoint"""
    out = {}
    for tag in TAGS:
        c = km.CASES[tag]
        gx, gg = km.golden_cotangents(d, tag)
        for dt in (torch.float64, torch.float32):
            sd = {k: v.to(dt) if v.dtype.is_floating_point else v for k, v in _module(d, tag).state_dict().items()}
            t = lambda n: torch.from_numpy(d[tag + n]).to(dt)
            out[tag, dt] = km.run(c["block"], t("|x"), t("|pc"), torch.from_numpy(d[tag + "|idx"]), gx.to(dt), None if gg is None else gg.to(dt),
                                  km.layer_k(c), sd, c["train"])
    return out


def _stored(d, tag):
    return {k[len(tag) + 1:].rsplit("|", 1)[0] for k in d if k.startswith(tag + "|") and k.endswith(("|full", "|samples"))
            and "|d64|" not in k and "num_batches_tracked" not in k}


def _zero(d, tag):
    return km.zero_grad_biases(str(n) for n in d["state_keys|" + km.CASES[tag]["block"]]) if km.CASES[tag]["train"] else ()


@pytest.mark.parametrize("tag", TAGS)
def test_model_matches_reference_float64(d, runs, tag):
    got = runs[tag, torch.float64]
    assert set(got) == _stored(d, tag)                                          # every stored quantity
    zero = _zero(d, tag)
    for q, v in got.items():
        ref64, mine = km.golden_pair(d, tag, q, v)
        err = _rel(mine, ref64)
        if q[5:] in zero or float(ref64.abs().max()) == 0.0:
            # float64 rounding of sums whose terms have the size of the layer's weight gradient (up to 1e4 behind a BatchNorm1d over four rows)
            scale = max(1.0, float(got[q[:-5] + ".weight"].abs().max()) / 100.0) if q[5:] in zero else 1.0
            assert float((mine - ref64).abs().max()) < 1e-12 * scale, (tag, q)
        else:
            assert err < 1e-9, (tag, q, err)


@pytest.mark.parametrize("tag", TAGS)
def test_model_float32_within_reference_noise(d, runs, tag):
    zero = _zero(d, tag)
    for q, v in runs[tag, torch.float32].items():
        ref64, mine = km.golden_pair(d, tag, q, v)
        if q[5:] in zero:
            assert float((mine.double() - ref64).abs().max()) <= 2e-3, (tag, q)
            continue
        err, noise = _rel(mine, ref64), km.noise(d, tag, q)
        assert err <= max(5.0 * noise, 1e-12), (tag, q, err, noise)


def test_golden_conditions_and_state_dicts(d):
    import spgan
    assert {c["block"] for c in km.CASES.values()} == set(km.BLOCKS)           # every block is captured
    for tag in TAGS:
        c = km.CASES[tag]
        keys = tuple(str(n) for n in d["state_keys|" + c["block"]])
        assert d[tag + "|near_tie_rows"].mean() <= 0.01
        assert tuple(d[tag + "|x"].shape) == (c["B"], c["Fin"], c["N"]) and tuple(d[tag + "|idx"].shape) == (c["B"], c["N"] * km.layer_k(c))
        m = km.make_module(c, spgan)
        assert tuple(m.state_dict()) == keys and len(keys) == km.STATE_COUNTS[c["block"]]       # the reference's keys, in its order
        m.load_state_dict(km.golden_state_dict(d, tag), strict=True)
        back = km.make_module(c, spgan)
        back.load_state_dict(m.state_dict(), strict=True)
        assert m.last_idx is None
        if not c["train"]:                                                      # eval mode: the reference leaves its buffers alone
            for n in keys:
                if "running" in n:
                    assert torch.equal(torch.from_numpy(d["%s|buf|%s|full" % (tag, n)]), torch.from_numpy(km.param(d, tag, n))), n
    assert d["l2|dpc|full"].any() and d["dm|grad|add_cov.0.weight|full"].any()


def test_deform_block_head_is_absent():
    """the reference's deform_block_head cannot run (a 5-D tensor into BatchNorm1d, N columns concatenated with 2N): it is left out"""
    import spgan
    from spgan import modules
    assert not hasattr(spgan, "deform_block_head") and not hasattr(modules, "deform_block_head")
    assert "deform_block_head" not in spgan.__all__ and set(km.BLOCKS) <= set(spgan.__all__)


def test_refusals():
    import spgan
    x, pc = torch.zeros(4, 8, 24), torch.zeros(4, 3, 24)
    for cls, args in ((spgan.bilateral_block_l1, (x,)), (spgan.bilateral_block_l2, (x, pc)), (spgan.bilateral_block_l3, (x, pc)),
                      (spgan.bilateral_block_l4, (x, pc))):
        with pytest.raises(ValueError, match="maxpool=20.*N=24"):
            cls(8, 16, 20, num_k=4)(*args)
    for cls in (spgan.deform_block_middle, spgan.deform_block_tail):
        m = cls(8, 16, num_k=4)                                                # constructs (state_dicts load) ...
        with pytest.raises(ValueError, match="Fin == Fout"):                   # ... and refuses to run, as the layer
            m(x, pc)
    one = torch.zeros(1, 8, 24)
    for cls, args in ((spgan.bilateral_block, (8, 16, 24)), (spgan.bilateral_block_l1, (8, 16, 24)), (spgan.deform_block_feat, (8, 16)),
                      (spgan.deform_block_feat_middle, (8, 16))):
        with pytest.raises(ValueError, match="B=1"):
            cls(*args, num_k=4)(one)
        with pytest.raises(RuntimeError, match="no CPU"):                      # eval mode with B = 1 is fine -- on the GPU
            cls(*args, num_k=4).eval()(one)
    with pytest.raises(RuntimeError, match="no CPU"):
        spgan.bilateral_block(8, 16, 3, num_k=4)(x)                            # bilateral_block ignores maxpool
    with pytest.raises(RuntimeError, match="no CPU"):
        spgan.deform_block_middle(8, 8, num_k=4)(x, pc)
    with pytest.raises(ValueError, match="k must be even"):                    # num_k // 2 follows the layers' rule
        spgan.bilateral_block(8, 16, 24, num_k=6)
    with pytest.raises(RuntimeError, match="GPU"):
        spgan.block_tail.cm_stats(torch.zeros(2, 3, 4))


@pytest.mark.parametrize("B,C,L,Cs,Cg", [(3, 5, 23, 7, 0), (2, 4, 8, 3, 6), (2, 3, 9, 0, 5)])
@pytest.mark.parametrize("train", [True, False])
def test_tail_model_backward_against_autograd(B, C, L, Cs, Cg, train):
    """blocks_model.tail_bwd (what the GPU launchers are compared with) is the derivative of blocks_model.tail_fwd behind a BatchNorm"""
    g = torch.Generator().manual_seed(B * 100 + L)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    Y, gamma, beta = r(B, C, L).requires_grad_(True), (r(C) * 0.3 + 1.0).requires_grad_(True), r(C).requires_grad_(True)
    xs, gv = (r(B, Cs).requires_grad_(True) if Cs else None), (r(B, Cg).requires_grad_(True) if Cg else None)
    rm, rv = r(C) * 0.1, torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    mean, var = km.cm_stats(Y) if train else (rm, rv)
    invstd = 1.0 / torch.sqrt(var + km.EPS)
    scale = gamma * invstd
    shift = beta - mean * scale
    out_x, out_g = km.tail_fwd(Y, xs, gv, scale, shift)
    dx, dg, ex = r(*out_x.shape), (r(*out_g.shape) if gv is not None else None), r(B, C, L)
    a = out_x[:, Cs:]
    loss = (out_x * dx).sum() + (a * ex).sum() + ((out_g * dg).sum() if gv is not None else 0.0)
    ins = [t for t in (Y, gamma, beta, xs, gv) if t is not None]
    grads = dict(zip([id(t) for t in ins], torch.autograd.grad(loss, ins)))
    with torch.no_grad():
        sums, dxs, dgv, dY = km.tail_bwd(Y, dx, dg, ex, Cs, Cg, scale, shift, mean, invstd, gamma, train)
    assert _rel(dY, grads[id(Y)]) < 1e-12 and _rel(sums[C:], grads[id(gamma)]) < 1e-12 and _rel(sums[:C], grads[id(beta)]) < 1e-12
    if xs is not None:
        assert _rel(dxs, grads[id(xs)]) < 1e-12
    if gv is not None:
        assert _rel(dgv, grads[id(gv)]) < 1e-12


def test_launcher_status_codes():
    """bad sizes and missing pointers: -22 before any launch"""
    from spgan import _lib
    lib = _lib.load()
    assert lib.spgan_cm_stats(None, 1, 1, 1, None, None) == -22 and lib.spgan_cm_stats(1, 0, 1, 1, 1, None) == -22
    assert lib.spgan_block_tail_fwd(1, None, None, 1, 1, 1, 0, 0, 1, 1, 0.01, None, None, None) == -22          # no output
    assert lib.spgan_block_tail_fwd(1, None, None, 1, 1, 1, 2, 0, 1, 1, 0.01, 1, None, None) == -22             # Cs without xs
    assert lib.spgan_block_tail_fwd(1, None, None, 1, 1, 0, 0, 0, 1, 1, 0.01, 1, None, None) == -22             # L = 0
    assert lib.spgan_block_tail_bwd_reduce(1, None, None, None, 1, 1, 1, 0, 0, 1, 1, 0.01, None, 1, 1, None, None, None) == -22
    assert lib.spgan_block_tail_bwd_apply(1, None, None, None, 1, 1, 1, 0, 0, 1, 1, 0.01, None, None, None, 1, 4.0, 1, None) == -22
    assert lib.spgan_block_tail_bwd_apply(1, None, None, None, 1, -1, 1, 0, 0, 1, 1, 0.01, 1, 1, None, None, 4.0, 1, None) == -22


def test_cached_images_do_not_outlive_their_weight():
    """edge_conv.cached_images keys on the weights' addresses: an entry must not serve a weight that was born after the entry's own weight
    died -- the allocator may hand it the dead weight's address with a fresh version counter (two blocks of one shape built one after the
    other).  Here a numpy buffer plays the allocator: the second tensor has the first one's address, shape and version counter."""
    import numpy as np
    from spgan import edge_conv
    cache, built = {}, []

    def build(a):
        built.append(float(a.sum()))
        return (a * 2,)
    buf = np.ones((3, 4), dtype=np.float32)
    w = torch.from_numpy(buf)
    assert edge_conv.cached_images(cache, [w], (), build)[0] is edge_conv.cached_images(cache, [w], (), build)[0] and built == [12.0]
    ptr, ver = w.data_ptr(), w._version
    del w
    buf *= 3.0
    w2 = torch.from_numpy(buf)
    assert (w2.data_ptr(), w2._version) == (ptr, ver)                           # the hazard: same key, same stamp
    assert float(edge_conv.cached_images(cache, [w2], (), build)[0].sum()) == 72.0 and built == [12.0, 36.0]
    assert len(cache) == 1


def test_cached_images_bookkeeping_stays_constant():
    """A live weight that is rewritten again and again (an optimiser step per training iteration) rebuilds its images every time and
    leaves one cache entry and no other bookkeeping behind."""
    import gc
    import weakref
    from spgan import edge_conv
    cache, built = {}, []
    w = torch.ones(3, 4)
    gc.collect()
    finalizers = len(weakref.finalize._registry)
    for _ in range(200):
        w.add_(0)
        edge_conv.cached_images(cache, [w], (), lambda a: (built.append(1), a * 2))
    assert len(built) == 200 and len(cache) == 1 and len(weakref.finalize._registry) == finalizers
    stamp, img, refs = cache[next(iter(cache))]
    assert len(refs) == 1 and refs[0]() is w


