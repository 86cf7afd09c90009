"""CPU: the float64 model of the approxmatch EMD (tests/approxmatch_model.py) against exact assignment, the identity the fused
backward rests on, the compat names, the ABI table and the shape rule of spgan.approxmatch."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import approxmatch_model as am
import spgan
from spgan import _lib, approxmatch, compat, gan_metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exact_cost(a, b):
    opt = pytest.importorskip("scipy.optimize")
    d = np.sqrt(((a[:, None, :].astype(np.float64) - b[None, :, :].astype(np.float64)) ** 2).sum(-1))
    r, c = opt.linear_sum_assignment(d)
    return float(d[r, c].sum())


@pytest.mark.parametrize("kind", ["cube", "sphere"])
@pytest.mark.parametrize("n", [64, 128])
def test_model_is_a_transport_plan_above_the_exact_assignment(n, kind):
    a, b = am.clouds(kind, 1, n, n, seed=3)
    r = am.approx_match(a[0], b[0])
    match = r["match"]
    assert (match >= 0).all()
    assert np.abs(match.sum(1) - r["multiL"]).max() <= 1e-6
    assert match.sum(0).max() <= r["multiR"] * (1 + 1e-6)
    assert r["cost"] >= exact_cost(a[0], b[0]) * (1 - 1e-6)


@pytest.mark.parametrize("n", [64, 128])
def test_jittered_permutation_is_nearly_exact(n):
    g = np.random.default_rng(n)
    a = g.random((n, 3)).astype(np.float32)
    b = (a[g.permutation(n)] + 1e-3 * g.standard_normal((n, 3))).astype(np.float32)
    r = am.approx_match(a, b)
    exact = exact_cost(a, b)
    assert exact * (1 - 1e-6) <= r["cost"] <= 1.02 * exact, (r["cost"], exact)


@pytest.mark.parametrize("n,m", [(48, 48), (32, 64), (64, 32)])
def test_gradients_are_sums_over_the_plan_rebuilt_from_the_records(n, m):
    """match = sum_j E_j ratioL_j ratioR_j, so cost and both gradients follow from the records alone."""
    a, b = am.clouds("cube", 1, n, m, seed=5)
    r = am.approx_match(a[0], b[0])
    plan = am.plan_from_records(r["d2"], r["ratioL"], r["ratioR"])
    assert np.abs(plan - r["match"]).max() <= 1e-14 * max(1.0, r["match"].max())
    g1, g2, cost = am.grads_from_plan(a[0], b[0], plan)
    assert np.abs(g1 - r["grad1"]).max() <= 1e-12 and np.abs(g2 - r["grad2"]).max() <= 1e-12
    assert abs(cost - r["cost"]) <= 1e-12 * r["cost"]
    assert np.abs(r["match"].sum(1) - r["multiL"]).max() <= 1e-6 and np.abs(r["match"].sum(0) - r["multiR"]).max() <= 1e-6


def test_float32_model_is_close_to_float64():
    a, b = am.clouds("cube", 1, 128, 128, seed=9)
    r64, r32 = am.approx_match(a[0], b[0]), am.approx_match(a[0], b[0], np.float32)
    assert r32["match"].dtype == np.float32
    assert abs(float(r32["cost"]) - r64["cost"]) <= 1e-5 * r64["cost"]


def test_shape_rule_and_argument_checks():
    with pytest.raises(ValueError, match="multiple"):
        am.approx_match(np.zeros((3, 3)), np.zeros((2, 3)))
    x = torch.zeros(2, 3, 3)
    for fn in (approxmatch.match_cost, approxmatch.approx_match, approxmatch.emd_approx_match):
        with pytest.raises(ValueError, match="GPU"):
            fn(x, x)                                                      # CPU tensors
        with pytest.raises(ValueError, match="float32"):
            fn(x.double(), x.double())
        with pytest.raises(ValueError, match=r"\[B, N, 3\]"):
            fn(torch.zeros(2, 3, 4), torch.zeros(2, 3, 4))
    with pytest.raises(ValueError, match="GPU"):
        approxmatch.match_cost_dense(x, x, torch.zeros(2, 3, 3))
    with pytest.raises(ValueError, match="GPU"):
        spgan.get_emd_loss(x, x, 1.0)
    with pytest.raises(ValueError, match="same N"):
        spgan.get_emd_loss(x, torch.zeros(2, 6, 3), 1.0)
    with pytest.raises(ValueError, match="emd must be"):
        spgan.metrics.emd_approx(x, x, emd="exact")
    with pytest.raises(ValueError, match="multiple"):
        approxmatch.match_cost(torch.zeros(2, 3, 3), torch.zeros(2, 2, 3))                 # n = 3, m = 2
    with pytest.raises(ValueError, match="batch sizes"):
        approxmatch.match_cost(torch.zeros(2, 4, 3), torch.zeros(3, 4, 3))
    with pytest.raises(ValueError, match="equal point counts"):
        approxmatch.emd_approx_match(torch.zeros(2, 4, 3), torch.zeros(2, 8, 3))
    assert approxmatch._batch_stride(torch.zeros(1, 4, 3).expand(5, 4, 3)) == 0
    assert approxmatch._batch_stride(torch.zeros(5, 4, 3)) == 12 and approxmatch._batch_stride(torch.zeros(1, 4, 3)) == 12
    assert approxmatch._batch_stride(torch.zeros(1, 3, 4).transpose(1, 2).expand(5, 4, 3)) == 12          # a copy is needed


def test_exports_and_keywords():
    import inspect
    for name in ("approxmatch", "MatchCostFunction", "approx_match", "match_cost", "match_cost_dense", "emd_approx_match", "get_emd_loss"):
        assert name in spgan.__all__ and hasattr(spgan, name), name
    assert spgan.model_utils.get_emd_loss is spgan.get_emd_loss
    for fn in (spgan.metrics.emd_approx, spgan.metrics.pairwise_emd, spgan.metrics.EMD_CD, spgan.metrics.compute_all_metrics,
               gan_metrics.pairwise_dists):
        assert inspect.signature(fn).parameters["emd"].default == "auction", fn.__name__
    assert list(inspect.signature(approxmatch.match_cost).parameters) == ["seta", "setb"]
    assert list(inspect.signature(approxmatch.match_cost_dense).parameters) == ["xyz1", "xyz2", "match"]


REFERENCE_IMPORTS = """\
from StructuralLosses.match_cost import match_cost
from metrics.StructuralLosses.nn_distance import nn_distance
from metrics.StructuralLosses.match_cost import match_cost as mc2
"""


def test_reference_import_lines_resolve_without_the_library():
    code = ("import sys; sys.path[:0] = [%r]\n"
            "import spgan.approxmatch\n"
            "from spgan import _lib; import torch\n"
            "assert _lib._lib is None, 'importing spgan.approxmatch loaded the shared library'\n"
            "import spgan.compat; spgan.compat.install()\n%s"
            "import spgan\n"
            "assert match_cost is spgan.approxmatch.match_cost and mc2 is match_cost and nn_distance is spgan.metrics.nn_distance\n"
            "assert _lib._lib is None and not torch.cuda.is_initialized()\n"
            "spgan.compat.uninstall(); assert 'StructuralLosses' not in sys.modules\nprint('ok')\n") % (os.path.join(ROOT, "sp-gan_amd"), REFERENCE_IMPORTS)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(ROOT))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr
    for name in ("StructuralLosses", "StructuralLosses.match_cost", "StructuralLosses.nn_distance", "metrics.StructuralLosses",
                 "metrics.StructuralLosses.match_cost", "metrics.StructuralLosses.nn_distance"):
        assert name in compat.STAND_INS, name


NEW = ("spgan_approxmatch_levels", "spgan_approxmatch_tile", "spgan_approxmatch_ws_bytes", "spgan_approxmatch_fwd", "spgan_approxmatch_bwd",
       "spgan_approxmatch_plan", "spgan_match_cost_dense_fwd", "spgan_match_cost_dense_bwd")


def test_abi_table_header_and_refusals():
    header = open(os.path.join(ROOT, "include", "spgan_hip.h")).read()
    for s in NEW:
        assert s in _lib.SIGNATURES and (s + "(") in header, s
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert hasattr(raw, s), s
    lib = _lib.load()
    assert lib.spgan_approxmatch_levels() == approxmatch.LEVELS == len(am.LEVELS) and lib.spgan_approxmatch_tile() >= 64
    assert lib.spgan_approxmatch_ws_bytes(2, 8, 4) == 2 * (8 * 3 + 4 * 2) * 8 and lib.spgan_approxmatch_ws_bytes(0, 8, 4) == 0
    X, E, big = 64, -22, 1 << 20          # never dereferenced: every call below is refused before a launch
    fwd = lib.spgan_approxmatch_fwd
    ok = [X, 12, X, 1, 4, 4, 0, X, X, X, X, big, None]
    for hole in (0, 2, 7, 8, 9, 10):
        a = list(ok)
        a[hole] = None
        assert fwd(*a) == E, hole
    for i, v in ((3, 0), (4, 0), (5, 0), (3, 65536), (4, 3), (1, 7), (6, 2), (11, 8)):      # sizes, the multiple rule (3 vs 4), stride, waves, ws
        a = list(ok)
        a[i] = v
        assert fwd(*a) == E, (i, v)
    assert fwd(X, 9, X, 1, 3, 2, 0, X, X, X, X, big, None) == E
    bwd = lib.spgan_approxmatch_bwd
    assert bwd(X, 12, X, 1, 4, 4, X, X, X, None, None, None) == E and bwd(None, 12, X, 1, 4, 4, X, X, X, X, X, None) == E
    assert bwd(X, 9, X, 1, 3, 2, X, X, X, X, X, None) == E
    plan = lib.spgan_approxmatch_plan
    assert plan(X, 12, X, 1, 4, 4, X, X, None, None) == E and plan(X, 12, X, 1, 4, 65536 * 4, X, X, X, None) == E
    assert lib.spgan_match_cost_dense_fwd(X, X, None, 1, 4, 4, X, X, big, None) == E
    assert lib.spgan_match_cost_dense_fwd(X, X, X, 1, 4, 4, X, X, 8, None) == E
    assert lib.spgan_match_cost_dense_bwd(X, X, X, 1, 4, 4, X, None, None, None) == E
    assert lib.spgan_match_cost_dense_bwd(X, X, X, 1, 3, 2, X, X, X, None) == E
