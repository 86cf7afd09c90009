"""CPU: spgan.pointconv_util (Common/pointconv_util.py:120-172, 199-383).  The fresh model of tests/pointconv_model.py reproduces the
vectors captured from the reference (golden G24); the new names exist in the package, the header and the ctypes table with matching
signatures and the built library exports them; a reference-layout state_dict loads strictly into every module built on the CPU and
round-trips."""
import os
import re

import numpy as np
import pytest
import torch

import pointconv_model as pcm
from helpers import check_bounded_by_reference_noise as check64, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("spgan_kde_density", "spgan_kde_density_bwd", "spgan_group_density_scale", "spgan_group_density_scale_bwd",
               "spgan_pointconv_aggregate", "spgan_pointconv_aggregate_bwd")
FLOOR = 8e-6          # the block tolerance the other float32-vs-float64 golden checks use (tests/test_pointnet2_gpu.py)
SEEDS = (("dsa", 21), ("dsa_nopts", 22), ("sa", 23), ("dsa_all", 24))


def _atol(name):
    # a conv / linear bias in front of a train-mode BatchNorm has an exactly zero gradient; the reference holds rounding noise there
    return 2e-3 if re.search(r"(convs[.\d]*|(^|\.)linear)\.bias$", name) else 1e-7


@pytest.fixture(scope="module")
def d():
    return golden("g24_pointconv.npz")


def test_bias_rule_names():
    assert _atol("mlp_convs.0.bias") == _atol("weightnet.mlp_convs.2.bias") == _atol("densitynet.mlp_convs.1.bias") == _atol("linear.bias") == 2e-3
    assert _atol("bn_linear.bias") == _atol("mlp_bns.0.bias") == _atol("linear.weight") == 1e-7


@pytest.mark.parametrize("tag", sorted(pcm.CASES))
def test_model_reproduces_reference_golden(d, tag):
    sd = pcm.case_state_dict(d, tag)
    params = {k: v.requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running" not in k}
    names = pcm.CASES[tag][2]
    args = [None if a is None else a.requires_grad_(True) for a in pcm.case_inputs(d, tag)]
    outs, bufs, used = pcm.run_model(d, tag, sd, args)
    if used[0] is not None:
        assert np.array_equal(used[0].numpy(), d[tag + "|fps0"].astype(np.int64))
        assert np.array_equal(used[1].sort(dim=-1)[0].numpy(), d[tag + "|knn0"].astype(np.int64))       # neighbour sets
    sum((o * torch.from_numpy(d["%s|gout%d" % (tag, i)].astype(np.float32))).sum() for i, o in enumerate(outs)).backward()
    for i, o in enumerate(outs):
        check64(d, "%s|out%d" % (tag, i), "%s|out%d|f64" % (tag, i), o, floor=FLOOR, atol=1e-7)
    for k, p in params.items():
        check64(d, "%s|grad|%s" % (tag, k), "%s|grad|%s|f64" % (tag, k), p.grad, floor=FLOOR, atol=_atol(k))
    for a, n in zip(args, names):
        if a is not None:
            check64(d, "%s|gin|%s" % (tag, n), "%s|gin|%s|f64" % (tag, n), a.grad, floor=FLOOR, atol=1e-7)
    assert len(bufs) == len([k for k in sd if "running" in k or "num_batches" in k])
    for k, v in bufs.items():
        if v.is_floating_point():
            check64(d, "%s|buf|%s" % (tag, k), "%s|buf|%s|f64" % (tag, k), v, floor=FLOOR)
        else:
            assert int(v) == int(d["%s|buf|%s" % (tag, k)]) == 1


def test_model_density_reproduces_reference_golden(d):
    x = pcm.case_inputs(d, "dsa")[0].transpose(1, 2).contiguous().requires_grad_(True)
    dens = pcm.compute_density(x, pcm.BANDWIDTH)
    (dens * torch.from_numpy(d["kde|gout"].astype(np.float32))).sum().backward()
    check64(d, "kde|density", "kde|density|f64", dens, floor=FLOOR)
    check64(d, "kde|gin|xyz", "kde|gin|xyz|f64", x.grad, floor=FLOOR)


def test_new_names_exist_with_header_signatures():
    import spgan
    from spgan import _lib, pointconv_util as pc
    assert spgan.pointconv_util is pc
    for name in ("square_distance", "index_points", "farthest_point_sample", "query_ball_point", "knn_point", "group", "sample_and_group",
                 "sample_and_group_all", "compute_density", "DensityNet", "WeightNet", "PointConvSetAbstraction", "PointConvDensitySetAbstraction"):
        assert hasattr(pc, name), name
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spgan_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for sym in NEW_SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % sym, txt, flags=re.S)
        assert m, "%s is not declared in include/spgan_hip.h" % sym
        decl = [a.strip() for a in m.group(1).split(",")]
        res, argtypes = _lib.SIGNATURES[sym]
        assert len(argtypes) == len(decl), (sym, len(argtypes), decl)
        for a, t in zip(decl, argtypes):
            want = _lib.P if ("*" in a or "spgan_stream_t" in a) else (_lib.F if a.startswith("float") else _lib.I)
            assert t is want, (sym, a, t)
        assert hasattr(lib, sym)
    # argument validation happens before any launch (no GPU needed)
    assert lib.spgan_kde_density(None, 1, 1, 0.1, None, None, None) == -22
    assert lib.spgan_kde_density(16, 1, 4, 0.0, 16, None, None) == -22                                  # bandwidth must be positive
    assert lib.spgan_kde_density_bwd(16, None, None, None, 1, 4, 0.1, 16, None) == -22                    # no incoming gradient at all
    assert lib.spgan_group_density_scale(16, 16, 1, 4, 1, 0, 16, None, None) == -22                       # K = 0
    assert lib.spgan_pointconv_aggregate(16, 16, None, 1, 4, 4, 8, 16, None) == -22                        # only the width 16 is built
    assert lib.spgan_pointconv_aggregate_bwd(16, 16, 16, 16, 1, 4, 4, 16, 16, 16, None, None) == -22      # dens without ddens


@pytest.mark.parametrize("tag", sorted(pcm.CASES))
def test_reference_state_dict_loads_strictly_and_round_trips(d, tag):
    from spgan import pointconv_util as pc
    kind, cargs, _ = pcm.CASES[tag]
    sd = pcm.case_state_dict(d, tag)
    torch.manual_seed(0)
    m = getattr(pc, kind)(*cargs)                       # construction needs no GPU
    own = m.state_dict()
    assert list(own.keys()) == list(sd.keys())
    assert all(tuple(own[k].shape) == tuple(sd[k].shape) and own[k].dtype == sd[k].dtype for k in sd)
    m.load_state_dict(sd, strict=True)
    back = m.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    getattr(pc, kind)(*cargs).load_state_dict(back, strict=True)


def test_standalone_nets_have_the_reference_layout():
    from spgan import pointconv_util as pc
    dn, wn = pc.DensityNet(), pc.WeightNet(3, 16)
    assert [tuple(c.weight.shape) for c in dn.mlp_convs] == [(16, 1, 1, 1), (8, 16, 1, 1), (1, 8, 1, 1)]
    assert [tuple(c.weight.shape) for c in wn.mlp_convs] == [(8, 3, 1, 1), (8, 8, 1, 1), (16, 8, 1, 1)]
    assert [tuple(c.weight.shape) for c in pc.WeightNet(3, 16, hidden_unit=[]).mlp_convs] == [(16, 3, 1, 1)]


def test_same_seed_gives_the_reference_initial_parameters(d):
    """The containers are created in the reference's order, so the capture script's seed reproduces its initial parameters."""
    from spgan import pointconv_util as pc
    for tag, seed in SEEDS:
        kind, cargs, _ = pcm.CASES[tag]
        torch.manual_seed(seed)
        m = getattr(pc, kind)(*cargs)
        for k, v in pcm.case_state_dict(d, tag).items():
            assert torch.equal(m.state_dict()[k], v), (tag, k)


def test_cpu_tensors_are_refused(d):
    from spgan import pointconv_util as pc
    for tag in ("dsa", "sa"):
        kind, cargs, _ = pcm.CASES[tag]
        with pytest.raises(RuntimeError, match="no CPU"):
            getattr(pc, kind)(*cargs)(*pcm.case_inputs(d, tag))
    with pytest.raises(RuntimeError, match="no CPU"):
        pc.compute_density(torch.zeros(1, 4, 3), 0.1)
    with pytest.raises(RuntimeError, match="no CPU"):
        pc.sample_and_group(2, 2, torch.zeros(1, 4, 3), None)
    with pytest.raises(RuntimeError, match="no CPU"):
        pc.WeightNet(3, 16)(torch.zeros(1, 3, 2, 2))
