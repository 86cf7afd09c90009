"""CPU: the PointNet++ surface of spgan.pointnet_util (Common/pointnet_util.py:146-320).  The fresh model of tests/pointnet2_model.py
reproduces the vectors captured from the reference (golden G22); the new names exist in the package, the header and the ctypes table
with matching signatures; a reference-layout state_dict loads strictly into every module built on the CPU and round-trips."""
import os
import re

import numpy as np
import pytest
import torch

import pointnet2_model as pm
from helpers import check_bounded_by_reference_noise as check64, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("spgan_three_nn", "spgan_three_interpolate", "spgan_three_interpolate_bwd", "spgan_group_max", "spgan_group_max_bwd",
               "spgan_cm_to_rows", "spgan_rows_to_cm")
FLOOR = 8e-6          # the block tolerance the other float32-vs-float64 golden checks use (tests/test_benchsize_golden_gpu.py)


def _atol(name):
    # a conv bias in front of a train-mode BatchNorm has an exactly zero gradient; the reference holds rounding noise there
    return 2e-3 if re.search(r"(convs|conv_blocks)[.\d]*\.bias$", name) else 1e-7


@pytest.fixture(scope="module")
def d():
    return golden("g22_pointnet2.npz")


@pytest.mark.parametrize("tag", sorted(pm.CASES))
def test_model_reproduces_reference_golden(d, tag):
    sd = pm.case_state_dict(d, tag)
    params = {k: v.requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running" not in k}
    args = [a.requires_grad_(not n.startswith("xyz_nograd")) for a, n in zip(pm.case_inputs(d, tag), pm.CASES[tag][2])]
    outs, bufs, used = pm.run_model(d, tag, sd, args)
    if used is not None and used[0] is not None:
        assert np.array_equal(used[0].numpy(), d[tag + "|fps0"].astype(np.int64))
        balls = used[1] if isinstance(used[1], list) else [used[1]]
        for i, b in enumerate(balls):
            assert np.array_equal(b.numpy(), d["%s|ball%d" % (tag, i)].astype(np.int64))
    sum((o * torch.from_numpy(d["%s|gout%d" % (tag, i)].astype(np.float32))).sum() for i, o in enumerate(outs)).backward()
    for i, o in enumerate(outs):
        check64(d, "%s|out%d" % (tag, i), "%s|out%d|f64" % (tag, i), o, floor=FLOOR, atol=1e-7)
    for k, p in params.items():
        check64(d, "%s|grad|%s" % (tag, k), "%s|grad|%s|f64" % (tag, k), p.grad, floor=FLOOR, atol=_atol(k))
    for a, n in zip(args, pm.CASES[tag][2]):
        if a.grad is not None:
            check64(d, "%s|gin|%s" % (tag, n), "%s|gin|%s|f64" % (tag, n), a.grad, floor=FLOOR, atol=1e-7)
    for k, v in bufs.items():
        if v.is_floating_point():
            check64(d, "%s|buf|%s" % (tag, k), "%s|buf|%s|f64" % (tag, k), v, floor=FLOOR)
        else:
            assert int(v) == int(d["%s|buf|%s" % (tag, k)]) == 1


def test_model_three_nn_matches_reference_order(d):
    x1, x2 = pm.case_inputs(d, "fp")[:2]
    idx, w, ds = pm.three_nn(x1.transpose(1, 2), x2.transpose(1, 2))
    assert np.array_equal(idx.numpy(), d["fp|nn_idx"].astype(np.int64))
    np.testing.assert_allclose(ds.numpy(), d["fp|nn_dist4"], rtol=0, atol=1e-6)
    assert not (d["fp|nn_dist4"] == np.float32(-1e-8)).any()


def test_new_names_exist_with_header_signatures():
    from spgan import _lib, pointnet_util as pu
    for name in ("sample_and_group_all", "three_nn", "three_interpolate", "PointNetSetAbstraction", "PointNetSetAbstractionMsg",
                 "PointNetFeaturePropagation"):
        assert hasattr(pu, name), name
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
    assert lib.spgan_three_nn(None, None, 1, 1, 1, None, None, None) == -22
    assert lib.spgan_three_interpolate(1, 1, 1, 1, 4, 4, 2, 4, 1, 2, 0, None, None) == -22          # k > 3
    assert lib.spgan_group_max_bwd(1, 1, None, 1, 4, 1, 1, 0.0, 2, 8, 4, 1, 1, None) == -22          # no arg-max with K > 1
    assert lib.spgan_cm_to_rows(1, 1, 4, 4, 1, 3, 0, None) == -22                                      # slice wider than the row


@pytest.mark.parametrize("tag", sorted(pm.CASES))
def test_reference_state_dict_loads_strictly_and_round_trips(d, tag):
    from spgan import pointnet_util as pu
    kind, cargs, _ = pm.CASES[tag]
    sd = pm.case_state_dict(d, tag)
    torch.manual_seed(0)
    m = getattr(pu, kind)(*cargs)                       # construction needs no GPU
    own = m.state_dict()
    assert list(own.keys()) == list(sd.keys())
    assert all(tuple(own[k].shape) == tuple(sd[k].shape) and own[k].dtype == sd[k].dtype for k in sd)
    m.load_state_dict(sd, strict=True)
    back = m.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    m2 = getattr(pu, kind)(*cargs)
    m2.load_state_dict(back, strict=True)


def test_same_seed_gives_the_reference_initial_parameters(d):
    """The containers are created in the reference's order, so the capture script's seed reproduces its initial parameters."""
    from spgan import pointnet_util as pu
    for tag, seed in (("sa", 11), ("sa_all", 12), ("msg", 13), ("fp", 14), ("fp1", 15)):
        kind, cargs, _ = pm.CASES[tag]
        torch.manual_seed(seed)
        m = getattr(pu, kind)(*cargs)
        for k, v in pm.case_state_dict(d, tag).items():
            assert torch.equal(m.state_dict()[k], v), (tag, k)


def test_cpu_tensors_are_refused(d):
    from spgan import pointnet_util as pu
    for tag in ("sa", "fp"):
        kind, cargs, _ = pm.CASES[tag]
        m = getattr(pu, kind)(*cargs)
        with pytest.raises(RuntimeError, match="no CPU"):
            m(*pm.case_inputs(d, tag))
    with pytest.raises(RuntimeError, match="no CPU"):
        pu.three_nn(torch.zeros(1, 4, 3), torch.zeros(1, 2, 3))
    fp = pu.PointNetFeaturePropagation(22, [16])
    a = pm.case_inputs(d, "fp")
    with pytest.raises(NotImplementedError, match="xyz1"):
        fp(a[0].requires_grad_(True), a[1], a[2], a[3])
