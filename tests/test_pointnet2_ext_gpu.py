"""GPU: the pointnet2 extension (spgan.pointnet2_utils / pytorch_utils / pointnet2_modules; csrc/sa_group.hip) --
  * the ops against the model of tests/pointnet2_ext_model.py, indices bit for bit, gradients against the model's autograd;
  * the multi-radius ball query against one ball_query per radius, bit for bit;
  * the modules, fused=True and fused=False, against the vectors captured from the reference (tests/golden/pointnet2_ext.npz, float32 and
    float64): the error against the float64 result is bounded by the reference's own float32 error (tests/test_pointnet2_gpu.py's
    convention: FLOOR, factor 1.5);
  * one multi-tile case against the model; bit-for-bit repeats; buffer bookkeeping; the memory the hoisted route saves.
Measured on an MI355X, rel-L2 against the reference's float64 run over the outputs and gradients of the eleven non-degenerate cases: at
most 7.5e-07 fused and 7.7e-07 unfused, the reference's own float32 run at most 6.3e-07 (all below FLOOR); case xyz1 (every grouped row
exactly zero) 1.3e-05 on the features against the reference's 1.1e-05.  Memory test: 1.70 MB fused, 3.11 MB unfused, 0.78 MB grouped."""
import numpy as np
import pytest
import torch

import pointnet2_ext_model as pm
from helpers import check_bounded_by_reference_noise as check64, golden

pytestmark = pytest.mark.gpu
FLOOR = 8e-6          # tests/test_pointnet2_gpu.py
DEV = "cuda"


@pytest.fixture(scope="module")
def ext():
    from spgan import _lib, pointnet2_modules, pointnet2_utils
    _lib.load()
    return pointnet2_utils, pointnet2_modules


@pytest.fixture(scope="module")
def d():
    return golden("pointnet2_ext.npz")


def _cloud(seed, B, n):
    return torch.rand(B, n, 3, generator=torch.Generator().manual_seed(seed))


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


SHAPES = [(B, N) for B in (1, 3) for N in (1, 65, 203)]


# ------------------------------------------------------------------------------------------------------------------------ ops
@pytest.mark.parametrize("B,N", SHAPES)
def test_index_ops_equal_the_model_bit_for_bit(ext, B, N):
    pu, _ = ext
    xyz = _cloud(10 * B + N, B, N)
    for m in (1, 2, 5, N + 3):
        new_xyz = _cloud(m, B, m)
        new_xyz[:, -1] = 9.0                                              # an empty ball: every slot stays 0
        if m > 1:
            new_xyz[:, 0] = xyz[:, N // 2]                                # a centre that is a cloud point
        for nsample in (1, 2, 5, N + 7):
            # 0.08: most balls of a 65- / 203-point cloud hold fewer than 5 points (padded slots); 0.6: most are cut off at nsample
            for radius in (0.08, 0.6):
                got = pu.ball_query(radius, nsample, xyz.to(DEV), new_xyz.to(DEV))
                want = pm.ball_query(radius, nsample, xyz, new_xyz)
                assert got.dtype == torch.int32 and torch.equal(got.cpu(), want), (m, nsample, radius)
                assert int(got[:, -1].abs().max()) == 0
        dist, idx = pu.three_nn(new_xyz.to(DEV), xyz.to(DEV))
        wd, wi = pm.three_nn(new_xyz, xyz)
        assert idx.dtype == torch.int32 and torch.equal(idx.cpu(), wi)
        # the squared distances are the model's bit for bit; the device's square root is within one float32 ulp of the correctly rounded one
        assert torch.equal(torch.isinf(dist.cpu()), torch.isinf(wd))
        fin = torch.isfinite(wd)
        assert torch.allclose(dist.cpu()[fin], wd[fin], rtol=2.0 ** -23, atol=0.0)
    if N > 1:
        padded = (pm.ball_query(0.08, 5, xyz, xyz)[:, :, -1] == pm.ball_query(0.08, 5, xyz, xyz)[:, :, 0]).float().mean()
        assert padded > 0.5                                               # the small radius does pad most lists
    for npoint in (1, 2, 5):
        if npoint <= N:
            assert pm.fps_margin(xyz, npoint) > 1e-6
            got = pu.furthest_point_sample(xyz.to(DEV), npoint)
            assert got.dtype == torch.int32 and torch.equal(got.cpu(), pm.furthest_point_sample(xyz, npoint))


@pytest.mark.parametrize("C", [1, 5, 67])
@pytest.mark.parametrize("B,N", [(1, 1), (3, 65), (3, 203)])
def test_gathers_and_their_gradients_against_the_model(ext, B, N, C):
    pu, _ = ext
    g = torch.Generator().manual_seed(100 * C + N)
    feat = torch.randn(B, C, N, generator=g)
    m, K, n = 5, 6, 9
    idx1 = torch.randint(0, N, (B, m), generator=g).to(torch.int32)
    idx2 = torch.randint(0, N, (B, m, K), generator=g).to(torch.int32)
    idx2[:, :, 3:] = idx2[:, :, :1]                                       # duplicates, as a padded ball has them
    idx3 = torch.randint(0, N, (B, n, 3), generator=g).to(torch.int32)
    idx3[:, ::2, 1] = idx3[:, ::2, 0]
    w = torch.rand(B, n, 3, generator=g)
    for fn, ref, args in ((pu.gather_operation, pm.gather_operation, (idx1,)), (pu.grouping_operation, pm.grouping_operation, (idx2,)),
                          (pu.three_interpolate, pm.three_interpolate, (idx3, w))):
        fg = feat.to(DEV).requires_grad_(True)
        out = fn(fg, *[a.to(DEV) for a in args])
        fr = feat.double().requires_grad_(True)
        want = ref(fr, *[a.double() if a.is_floating_point() else a for a in args])
        gout = torch.randn(want.shape, generator=g)
        (out * gout.to(DEV)).sum().backward()
        (want * gout.double()).sum().backward()
        if fn is pu.three_interpolate:
            assert _rel(out, want) < 2e-7                                 # three products and two sums in float32
        else:
            assert torch.equal(out.detach().cpu(), want.detach().float())
        # a point is read by at most B*m*K slots here; sums of that many float32 terms
        assert _rel(fg.grad, fr.grad) < 1e-6, fn
        first = fg.grad.clone(); fg.grad = None
        (fn(fg, *[a.to(DEV) for a in args]) * gout.to(DEV)).sum().backward()
        assert torch.equal(first, fg.grad)                                # slot lists, no float atomics


@pytest.mark.parametrize("B,N", SHAPES)
def test_multi_radius_query_equals_single_queries(ext, B, N):
    pu, _ = ext
    xyz = _cloud(7 * B + N, B, N).to(DEV)
    for m in (1, 5, N + 3):
        new_xyz = _cloud(m + 1, B, m)
        new_xyz[:, -1] = 9.0
        new_xyz = new_xyz.to(DEV)
        for radii, nsamples in (([0.3], [5]), ([0.12, 0.6], [N + 7, 2]), ([0.6, 0.12, 0.3, 0.9], [1, 5, 2, N + 7])):
            got = pu.ball_query_multi(radii, nsamples, xyz, new_xyz)
            assert len(got) == len(radii)
            for r, k, t in zip(radii, nsamples, got):
                assert t.dtype == torch.int32 and torch.equal(t, pu.ball_query(r, k, xyz, new_xyz)), (m, r, k)


def test_more_radii_than_one_launch_takes(ext):
    pu, _ = ext
    xyz, new_xyz = _cloud(1, 2, 65).to(DEV), _cloud(2, 2, 7).to(DEV)
    radii = [0.1 + 0.05 * i for i in range(pu.MAX_SCALES + 2)]
    got = pu.ball_query_multi(radii, [3] * len(radii), xyz, new_xyz)
    assert all(torch.equal(t, pu.ball_query(r, 3, xyz, new_xyz)) for r, t in zip(radii, got))


# ------------------------------------------------------------------------------------------------------------------------ modules
def _golden_sd(d, tag):
    return {k: torch.from_numpy(np.asarray(d["%s|param|%s" % (tag, k)])) for k in str(d["%s|keys" % tag]).split("\n")}


def _golden_inputs(d, tag):
    cfg = pm.CASES[tag]
    names = ["unknown", "known", "unknow_feats", "known_feats"] if cfg["kind"] == "fp" else ["xyz", "features", "new_xyz"]
    return names, [torch.from_numpy(d["%s|in|%s" % (tag, n)]) if "%s|in|%s" % (tag, n) in d else None for n in names]


def _golden_gouts(d, tag):
    out, i = [], 0
    while "%s|gout%d" % (tag, i) in d:
        out.append(torch.from_numpy(d["%s|gout%d" % (tag, i)]))
        i += 1
    return out


def _run(mods, cfg, sd, inputs, gouts, fused, backward=True):
    m = pm.build(mods, cfg)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).train(cfg["training"])
    m.fused = fused
    names, tensors = inputs
    args = [None if t is None else t.to(DEV).requires_grad_(n in pm.GRAD_INPUTS) for n, t in zip(names, tensors)]
    outs = m(*args)
    outs = [o for o in (outs if isinstance(outs, tuple) else (outs,)) if o is not None]
    if backward:
        sum((o * g.to(DEV)).sum() for o, g in zip(outs, gouts)).backward()
    res = {"out%d" % i: o.detach() for i, o in enumerate(outs)}
    for n, a in zip(names, args):
        if a is not None and a.requires_grad:
            res["gin|" + n] = a.grad if a.grad is not None else torch.zeros_like(a)
    for n, p in m.named_parameters():
        res["grad|" + n] = p.grad if p.grad is not None else torch.zeros_like(p)
    for n, b in m.named_buffers():
        res["buf|" + n] = b.detach().clone()
    return res


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("tag", sorted(pm.CASES))
def test_module_against_the_reference(ext, d, tag, fused):
    """Outputs, every gradient and every buffer of every case, on both routes: the rel-L2 error against the reference's float64 result is
    at most max(1.5 x the reference's own float32 error, 8e-6)."""
    _, mods = ext
    cfg = pm.CASES[tag]
    # the capture conditions, from the stored float64 values: the routing is well defined, nothing is left out of any comparison
    for k, bound in pm.MARGINS.items():
        assert float(d["%s|margin|%s" % (tag, k)]) > bound, (tag, k)
    res = _run(mods, cfg, _golden_sd(d, tag), _golden_inputs(d, tag), _golden_gouts(d, tag), fused)
    names = [k[len(tag) + 1:-len("|f64|full")] for k in d.files if k.startswith(tag + "|") and k.endswith("|f64|full")]
    assert sorted(names) == sorted(res)
    for q in names:
        if res[q].dtype.is_floating_point:
            e_own, e_ref = check64(d, "%s|%s" % (tag, q), "%s|%s|f64" % (tag, q), res[q], floor=FLOOR, atol=1e-7)
            print("%s %s %s: own %.2e reference %.2e" % (tag, "fused" if fused else "unfused", q, e_own, e_ref))
        else:
            assert int(res[q]) == int(d["%s|%s|full" % (tag, q)]), q


@pytest.mark.parametrize("which", ["MULTI_TILE", "GROUP_ALL_LONG"])
def test_multi_tile_case_against_the_model(ext, which):
    """MULTI_TILE: more than one tile of every new kernel in every tiled dimension, ending mid-tile.  GROUP_ALL_LONG: npoint=None with 203
    rows per group, above the 128 spgan_group_max walks.  The bound is the float32 model's own error against the float64 model (factor
    1.5, FLOOR), as for the golden cases."""
    _, mods = ext
    cfg = getattr(pm, which)
    keys_shapes = [(k, tuple(v.shape)) for k, v in pm.build(mods, cfg).state_dict().items()]
    margins = dict(pm.MARGINS, kink=pm.MULTI_TILE_MARGIN, pool=pm.MULTI_TILE_MARGIN)
    seed, inputs, sd, gouts, got = pm.find_seed(cfg, margins, keys_shapes)
    assert all(got[k] > margins[k] for k in margins)
    r64 = pm.run_model(cfg, sd, inputs, torch.float64, gouts)
    r32 = pm.run_model(cfg, sd, inputs, torch.float32, gouts)
    for fused in (True, False):
        res = _run(mods, cfg, sd, inputs, gouts, fused)
        assert sorted(res) == sorted(r64)
        for q in sorted(r64):
            if not r64[q].dtype.is_floating_point:
                assert int(res[q]) == int(r64[q])
                continue
            e_ref, e_own = _rel(r32[q], r64[q]), _rel(res[q], r64[q])
            print("multi-tile %s %s: own %.2e model float32 %.2e" % ("fused" if fused else "unfused", q, e_own, e_ref))
            assert e_own <= max(1.5 * e_ref, FLOOR) or float((res[q].double().cpu() - r64[q]).abs().max()) <= 1e-7, (fused, q, e_own, e_ref)


@pytest.mark.parametrize("tag", ["msg", "nobn", "avg", "all", "given", "fp40"])
def test_repeats_are_bit_identical_and_buffers_follow_the_unfused_route(ext, d, tag):
    _, mods = ext
    cfg = pm.CASES[tag]
    a = _run(mods, cfg, _golden_sd(d, tag), _golden_inputs(d, tag), _golden_gouts(d, tag), True)
    b = _run(mods, cfg, _golden_sd(d, tag), _golden_inputs(d, tag), _golden_gouts(d, tag), True)
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    u = _run(mods, cfg, _golden_sd(d, tag), _golden_inputs(d, tag), _golden_gouts(d, tag), False)
    for k in a:
        if k.startswith("buf|"):
            if a[k].dtype.is_floating_point:
                # the same statistics from two summation orders (records of the gather against the GEMM's epilogue): float32 rounding of
                # a mean / variance over >= 130 rows, times the momentum 0.1
                assert torch.allclose(a[k], u[k], rtol=1e-5, atol=1e-7), k
            else:
                assert int(a[k]) == int(u[k]) == 1, k


def test_memory_the_hoisted_route_saves(ext):
    """On the multi-tile case the peak of a fused forward + backward lies below the unfused one by at least the bytes of one grouped
    [B*S*K, 3+C] tensor per scale -- the tensor the route does not form."""
    _, mods = ext
    cfg = pm.MULTI_TILE
    keys_shapes = [(k, tuple(v.shape)) for k, v in pm.build(mods, cfg).state_dict().items()]
    inputs = pm.case_inputs(cfg, 0)
    sd = pm.state_dict_for(keys_shapes, 0, True)
    outs = _run(mods, cfg, sd, inputs, None, True, backward=False)
    gouts = pm.cotangents([outs[k].cpu() for k in sorted(outs) if k.startswith("out")], 0)
    peak = {}
    for fused in (False, True, False, True):                              # the second pair is the measurement: allocator and library warm
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        _run(mods, cfg, sd, inputs, gouts, fused)
        torch.cuda.synchronize()
        peak[fused] = torch.cuda.max_memory_allocated() - base
    grouped = sum(cfg["B"] * cfg["npoint"] * k * (3 + cfg["C"]) * 4 for k in cfg["nsamples"])
    print("peak bytes: fused %d, unfused %d, grouped tensors %d" % (peak[True], peak[False], grouped))
    assert peak[True] <= peak[False] - grouped


def test_refusals(ext, d):
    pu, mods = ext
    cfg = pm.CASES["msg"]
    m = pm.build(mods, cfg).to(DEV)
    xyz, feats, _ = [None if t is None else t.to(DEV) for t in _golden_inputs(d, "msg")[1]]
    f = feats.clone().requires_grad_(True)
    _, out = m(xyz, f)
    with pytest.raises(RuntimeError, match="once differentiable"):
        torch.autograd.grad(out.sum(), f, create_graph=True)
    with pytest.raises(ValueError):
        m(xyz, feats[:, :, :-1])
    with pytest.raises(ValueError):
        m(xyz[:, :, :2], feats)
    with pytest.raises(ValueError):
        pu.ball_query(0.1, 0, xyz, xyz)
    with pytest.raises(ValueError):
        pu.grouping_operation(feats, torch.zeros(2, 3, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        pu.three_interpolate(feats, torch.zeros(2, 4, 3, dtype=torch.int64, device=DEV), torch.zeros(2, 4, 3, device=DEV))
    inst = mods.PointnetSAModule(mlp=[5, 6], npoint=4, radius=0.3, nsample=3, instance_norm=True).to(DEV)
    assert inst.fused and inst(xyz, feats)[1].shape == (2, 6, 4)            # always the unfused route: plain torch layers
