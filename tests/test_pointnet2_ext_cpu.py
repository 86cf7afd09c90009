"""CPU: the pointnet2 extension's surface (spgan.pointnet2_utils, spgan.pytorch_utils, spgan.pointnet2_modules) carries the reference's
names, forward signatures and state_dict keys; spgan.compat registers it under the module names the reference imports; the float64 model
of tests/pointnet2_ext_model.py reproduces the vectors captured from the reference (tests/golden/pointnet2_ext.npz); the new entry points
refuse null pointers and bad sizes before any launch."""
import inspect
import sys

import numpy as np
import pytest
import torch

import pointnet2_ext_model as pm
import spgan
from helpers import golden
from spgan import _lib, compat, pointnet2_modules, pointnet2_utils, pytorch_utils

REFERENCE_IMPORTS = """\
from pointnet2.pointnet2_modules import PointnetSAModule, PointnetSAModuleMSG
from pointnet2.pointnet2_modules import PointnetFPModule
from pointnet2 import pytorch_utils as pt_utils
import pointnet2.pointnet2_utils as p2u
from metrics.pointnet2.pointnet2_modules import PointnetSAModuleMSG as MSG_a
from metrics.pointnet2_ops.pointnet2_modules import PointnetSAModuleMSG as MSG_b
from metrics.pointnet2_ops import pytorch_utils as pt_b
from metrics import pointnet2_utils as p2u_b
"""

FUNCTIONS = ("furthest_point_sample", "gather_operation", "three_nn", "three_interpolate", "grouping_operation", "ball_query")
FORWARD_ARGS = {
    "FurthestPointSampling": ["xyz", "npoint"], "GatherOperation": ["features", "idx"], "ThreeNN": ["unknown", "known"],
    "ThreeInterpolate": ["features", "idx", "weight"], "GroupingOperation": ["features", "idx"],
    "BallQuery": ["radius", "nsample", "xyz", "new_xyz"], "QueryAndGroup": ["xyz", "new_xyz", "features"],
    "GroupAll": ["xyz", "new_xyz", "features"], "RandomDropout": ["X"],
}


@pytest.fixture(scope="module")
def d():
    return golden("pointnet2_ext.npz")


@pytest.fixture
def clean_modules():
    compat.uninstall()
    before = dict(sys.modules)
    yield before
    compat.uninstall()
    for name in list(sys.modules):
        if name not in before:
            del sys.modules[name]
    sys.modules.update(before)


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


def test_surface_names_and_signatures():
    for name in FUNCTIONS:
        assert callable(getattr(pointnet2_utils, name)), name
    for name, want in FORWARD_ARGS.items():
        assert list(inspect.signature(getattr(pointnet2_utils, name).forward).parameters)[1:] == want, name
    assert list(inspect.signature(pointnet2_utils.QueryAndGroup.__init__).parameters)[1:] == ["radius", "nsample", "use_xyz"]
    assert list(inspect.signature(pointnet2_utils.GroupAll.__init__).parameters)[1:] == ["use_xyz"]
    sig = inspect.signature(pointnet2_modules.PointnetSAModuleMSG.__init__)
    assert list(sig.parameters)[1:] == ["npoint", "radii", "nsamples", "mlps", "bn", "use_xyz", "pool_method", "instance_norm", "first_layer"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for n, p in sig.parameters.items() if n != "self")
    sig = inspect.signature(pointnet2_modules.PointnetSAModule.__init__)
    assert list(sig.parameters)[1:] == ["mlp", "npoint", "radius", "nsample", "bn", "use_xyz", "pool_method", "instance_norm"]
    assert list(inspect.signature(pointnet2_modules.PointnetFPModule.__init__).parameters)[1:] == ["mlp", "bn"]
    assert list(inspect.signature(pointnet2_modules.PointnetSAModuleMSG.forward).parameters)[1:] == ["xyz", "features", "new_xyz"]
    assert list(inspect.signature(pointnet2_modules.PointnetFPModule.forward).parameters)[1:] == ["unknown", "known", "unknow_feats", "known_feats"]
    assert list(inspect.signature(pytorch_utils.SharedMLP.__init__).parameters)[1:] == ["args", "bn", "activation", "preact", "first", "name",
                                                                                       "instance_norm"]
    for name in ("SharedMLP", "Conv1d", "Conv2d", "BatchNorm1d", "BatchNorm2d", "FC"):
        assert issubclass(getattr(pytorch_utils, name), torch.nn.Sequential), name
    assert spgan.pointnet2_utils is pointnet2_utils and spgan.pointnet2_modules is pointnet2_modules and spgan.pytorch_utils is pytorch_utils
    assert {"pointnet2_utils", "pointnet2_modules", "pytorch_utils"} <= set(spgan.__all__)


def test_constructor_adds_three_and_fused_is_the_default():
    spec = [[5, 7, 9], [5, 6, 11]]
    m = pointnet2_modules.PointnetSAModuleMSG(npoint=4, radii=[0.1, 0.2], nsamples=[2, 3], mlps=spec)
    assert spec == [[8, 7, 9], [8, 6, 11]]                              # in the caller's list, as the reference does
    assert m.fused is True and m.mlps[0].layer0.conv.weight.shape == (7, 8, 1, 1)
    m = pointnet2_modules.PointnetSAModule(mlp=[5, 7], use_xyz=False)
    assert m.npoint is None and isinstance(m.groupers[0], pointnet2_utils.GroupAll) and m.mlps[0].layer0.conv.weight.shape == (7, 5, 1, 1)
    assert pointnet2_modules.PointnetFPModule(mlp=[4, 5]).fused is True
    # configurations the modules never create stay plain torch layers, on any device
    pre = pytorch_utils.SharedMLP([3, 4, 5], bn=True, preact=True, first=True)
    assert not pre.hip_route and list(pre.state_dict())[0] == "layer0.conv.weight" and "layer1.bn.bn.weight" in pre.state_dict()
    assert pre(torch.randn(2, 3, 4, 5)).shape == (2, 5, 4, 5)
    assert not pytorch_utils.SharedMLP([3, 4], bn=True, instance_norm=True).hip_route
    assert not pytorch_utils.SharedMLP([3, 4], bn=True, activation=torch.nn.Tanh()).hip_route
    fc = pytorch_utils.FC(4, 5, bn=True)
    assert list(fc.state_dict())[:2] == ["fc.weight", "bn.bn.weight"]
    assert list(pytorch_utils.Conv1d(3, 4).state_dict()) == ["conv.weight", "conv.bias"]


@pytest.mark.parametrize("tag", sorted(pm.CASES))
def test_state_dict_loads_strictly_both_ways(d, tag):
    cfg = pm.CASES[tag]
    sd = _golden_sd(d, tag)
    m = pm.build(pointnet2_modules, cfg)
    assert list(m.state_dict().keys()) == list(sd.keys())              # the reference's keys, in its order
    m.load_state_dict(sd, strict=True)
    back = m.state_dict()
    assert all(torch.equal(back[k], sd[k]) and back[k].shape == sd[k].shape for k in sd)
    assert any(".bn.bn." in k for k in sd) == cfg["bn"] and any(k.endswith("conv.bias") for k in sd) == (not cfg["bn"])


def test_reference_import_lines_resolve_to_spgan(tmp_path, clean_modules):
    assert compat.install()
    f = tmp_path / "reference_imports.py"
    f.write_text(REFERENCE_IMPORTS)
    ns = {}
    exec(compile(f.read_text(), str(f), "exec"), ns)
    assert ns["PointnetSAModule"] is pointnet2_modules.PointnetSAModule and ns["PointnetSAModuleMSG"] is pointnet2_modules.PointnetSAModuleMSG
    assert ns["MSG_a"] is ns["MSG_b"] is pointnet2_modules.PointnetSAModuleMSG and ns["PointnetFPModule"] is pointnet2_modules.PointnetFPModule
    assert ns["pt_utils"].SharedMLP is pytorch_utils.SharedMLP and ns["pt_b"].SharedMLP is pytorch_utils.SharedMLP
    assert ns["p2u"].ball_query is pointnet2_utils.ball_query and ns["p2u_b"].QueryAndGroup is pointnet2_utils.QueryAndGroup
    removed = compat.uninstall()
    assert "pointnet2.pointnet2_modules" in removed and "metrics.pointnet2_utils" in removed
    assert {k: id(v) for k, v in sys.modules.items() if k in clean_modules} == {k: id(v) for k, v in clean_modules.items() if k in sys.modules}
    assert "pointnet2" not in sys.modules and "metrics.pointnet2_ops" not in sys.modules


@pytest.mark.parametrize("tag", sorted(pm.CASES))
def test_model_reproduces_the_reference_in_float64(d, tag):
    cfg = pm.CASES[tag]
    tr = pm.Trace()
    res = pm.run_model(cfg, _golden_sd(d, tag), _golden_inputs(d, tag), torch.float64, _golden_gouts(d, tag), tr)
    names = [k[len(tag) + 1:-len("|f64|full")] for k in d.files if k.startswith(tag + "|") and k.endswith("|f64|full")]
    assert sorted(names) == sorted(res) and any(n.startswith("grad|") for n in names)
    for q in names:
        ref = torch.from_numpy(np.asarray(d["%s|%s|f64|full" % (tag, q)]))
        if ref.dtype.is_floating_point:
            err = float((res[q].double() - ref).norm() / max(float(ref.norm()), 1e-30))
            assert err < 1e-9 or float((res[q].double() - ref).abs().max()) < 1e-12, (q, err)
        else:
            assert torch.equal(res[q], ref), q
    # the capture conditions, re-asserted from the stored float64 inputs
    got = tr.margins()
    for k, bound in pm.MARGINS.items():
        assert got[k] > bound and got[k] == pytest.approx(float(d["%s|margin|%s" % (tag, k)]), rel=1e-6), (k, got[k])


def test_model_ops_keep_the_stated_rules():
    xyz = torch.tensor([[[0.0, 0, 0], [1, 0, 0], [0.5, 0, 0], [0.25, 0, 0]]])
    q = torch.tensor([[[0.0, 0, 0], [9, 9, 9]]])
    idx = pm.ball_query(0.5, 3, xyz, q)
    assert idx.tolist() == [[[0, 3, 0], [0, 0, 0]]]                    # strict <: the point at exactly r is out; padded with the first hit; empty: zeros
    assert pm.ball_query(0.51, 2, xyz, q).tolist() == [[[0, 2], [0, 0]]]          # the walk ends at nsample hits, in index order
    assert pm.furthest_point_sample(xyz, 3).tolist() == [[0, 1, 2]]
    dist, i3 = pm.three_nn(q[:, :1], xyz[:, :2])
    assert i3.tolist() == [[[0, 1, 0]]] and dist[0, 0, :2].tolist() == [0.0, 1.0] and torch.isinf(dist[0, 0, 2])


def test_new_entry_points_validate_before_launching():
    lib = _lib.load()
    a = _lib.SaQueryArgs()
    assert lib.spgan_sa_ballquery_multi(a, 1, 1, 1, 4, 2, None) == -22                      # count 0
    a.count = _lib.SA_MAX_SCALES + 1
    assert lib.spgan_sa_ballquery_multi(a, 1, 1, 1, 4, 2, None) == -22
    a.count = 1; a.nsample[0] = 2
    assert lib.spgan_sa_ballquery_multi(a, 1, 1, 1, 4, 2, None) == -22                      # no output list
    assert lib.spgan_sa_ballquery_multi(None, 1, 1, 1, 4, 2, None) == -22
    assert lib.spgan_sa_gather(None, 8, 0, 1, 8, 0, None, 1, 1, 4, 2, 3, 8, 1, 8, None, None, None) == -22
    assert lib.spgan_sa_gather(1, 4, 0, 1, 8, 0, None, 1, 1, 4, 2, 3, 8, 1, 8, None, None, None) == -22       # ldp < colp + C
    assert lib.spgan_sa_gather(1, 8, 0, 1, 8, 0, None, 1, 1, 4, 2, 0, 8, 1, 8, None, None, None) == -22       # K = 0
    assert lib.spgan_sa_scatter(None, 8, 8, 1, 1, 4, 1, 8, 0, 2, 3, 1, 8, 0, None) == -22
    assert lib.spgan_sa_scatter(1, 8, 8, 1, 1, 4, None, 8, 0, 2, 3, None, 8, 0, None) == -22     # neither output
    assert lib.spgan_sa_scatter(1, 8, 8, None, 1, 4, 1, 8, 0, 2, 3, None, 8, 0, None) == -22     # dP without the slot lists
    assert lib.spgan_sa_scatter(1, 8, 8, 1, 1, 4, 1, 8, 4, 2, 3, None, 8, 0, None) == -22        # the slice leaves dP
    assert lib.spgan_sa_rows_to_cm_slice(1, 1, 4, 3, 2, 4, 1, None) == -22                   # the slice leaves the buffer
    assert lib.spgan_sa_cm_slice_to_rows(None, 1, 4, 3, 0, 4, 1, None) == -22
    assert lib.spgan_sa_gather_tile_rows(0) == 0 and lib.spgan_sa_gather_tile_rows(5) % 5 == 0


def test_cpu_tensors_and_wrong_shapes_raise_value_error():
    xyz = torch.zeros(2, 8, 3)
    with pytest.raises(ValueError, match="GPU"):
        pointnet2_utils.ball_query(0.1, 2, xyz, xyz)
    with pytest.raises(ValueError, match="GPU"):
        pointnet2_utils.furthest_point_sample(xyz, 2)
    with pytest.raises(ValueError, match="GPU"):
        pointnet2_modules.PointnetSAModule(mlp=[0, 4], npoint=2, radius=0.1, nsample=2)(xyz)
    with pytest.raises(ValueError, match="GPU"):
        pointnet2_modules.PointnetFPModule(mlp=[4, 4])(xyz, xyz, None, torch.zeros(2, 4, 8))
    with pytest.raises(ValueError):
        pointnet2_utils.ball_query_multi([0.1], [2, 3], xyz, xyz)
