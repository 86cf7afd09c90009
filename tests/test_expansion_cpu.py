"""CPU: the ABI of the MST expansion penalty / minimum-density sampling entry points (argument refusals before any launch, refusal of
CPU tensors) and the invariants of their numpy model (tests/expansion_model.py), which the GPU tests hold the kernels to."""
import os
import re

import numpy as np
import pytest
import torch

import expansion_model as em
import spgan
from spgan import _lib, expansion_penalty, mds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("spgan_expansion_penalty_fwd", "spgan_expansion_penalty_bwd", "spgan_minimum_density_sample")


def test_symbols_declared_and_typed():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spgan_hip.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert s in _lib.SIGNATURES
    lib = _lib.load()
    for s in NEW:
        assert hasattr(lib, s)
    for name in ("expansionPenaltyFunction", "expansionPenaltyModule", "minimum_density_sample", "gather_operation"):
        assert hasattr(spgan, name) and name in spgan.__all__


def test_bad_arguments_are_refused_without_gpu():
    lib = _lib.load()
    X = 64          # never dereferenced: every call below is refused before a launch
    fwd, bwd, smp = lib.spgan_expansion_penalty_fwd, lib.spgan_expansion_penalty_bwd, lib.spgan_minimum_density_sample
    assert fwd(X, 1, 16, 1, 1.5, X, X, X, X, None) == -22            # primitive_size 1
    assert fwd(X, 1, 1026, 513, 1.5, X, X, X, X, None) == -22        # primitive_size 513
    assert fwd(X, 1, 17, 4, 1.5, X, X, X, X, None) == -22            # n % p != 0
    assert fwd(X, 0, 16, 4, 1.5, X, X, X, X, None) == -22            # B < 1
    for hole in range(5):
        ptrs = [X] * 5
        ptrs[hole] = None
        assert fwd(ptrs[0], 1, 16, 4, 1.5, ptrs[1], ptrs[2], ptrs[3], ptrs[4], None) == -22
    for hole in range(4):
        ptrs = [X] * 4
        ptrs[hole] = None
        assert bwd(ptrs[0], ptrs[1], ptrs[2], 1, 16, ptrs[3], None) == -22
    assert bwd(X, X, X, 0, 16, X, None) == -22
    assert smp(X, 1, 16, 17, X, 8192, X, None, None) == -22          # npoint > n
    assert smp(X, 1, 16, 0, X, 8192, X, None, None) == -22           # npoint < 1
    assert smp(None, 1, 16, 4, X, 8192, X, None, None) == -22
    assert smp(X, 1, 16, 4, None, 8192, X, None, None) == -22
    assert smp(X, 1, 16, 4, X, 8192, None, None, None) == -22
    assert lib.spgan_minimum_density_sample_needs_ws(16384) == 0 and lib.spgan_minimum_density_sample_needs_ws(16385) == 1
    assert smp(X, 1, 16385, 4, X, 8192, X, None, None) == -22        # this n needs density_ws
    assert lib.spgan_gather_points_cm(None, X, 1, 1, 4, 2, X, None, None) == -22
    assert lib.spgan_gather_points_cm_bwd(X, None, X, 1, 1, 4, 2, X, None) == -22


def test_wrappers_refuse_cpu_tensors_and_bad_sizes():
    x = torch.zeros(2, 16, 3)
    with pytest.raises(RuntimeError, match="no CPU"):
        spgan.expansionPenaltyModule()(x, 4, 1.5)
    with pytest.raises(RuntimeError, match="no CPU"):
        expansion_penalty.expansionPenaltyFunction.apply(x, 4, 1.5)
    with pytest.raises(RuntimeError, match="no CPU"):
        mds.minimum_density_sample(x, 4, torch.ones(2))
    with pytest.raises(RuntimeError, match="no CPU"):
        mds.gather_operation(torch.zeros(2, 3, 16), torch.zeros(2, 4, dtype=torch.int32))
    for p in (1, 513, 5):
        with pytest.raises(ValueError):
            spgan.expansionPenaltyModule()(torch.zeros(1, 1026 if p == 513 else 16, 3), p, 1.5)
    with pytest.raises(ValueError):
        spgan.expansionPenaltyModule()(torch.zeros(1, 16, 2), 4, 1.5)


@pytest.mark.parametrize("p", [2, 3, 4, 8, 64, 65, 128, 512])
def test_model_owner_invariants(p):
    """Exactly p-1 owners, distinct edges, each owned edge a tree edge; the tree spans and weighs what its edges weigh."""
    pts = np.random.default_rng(p).random((p, 3))
    par, w, _ = em.prim(pts)
    other, rounds = em.peel(par)
    owners = np.flatnonzero(other >= 0)
    assert owners.size == p - 1
    edges = {frozenset((int(t), int(other[t]))) for t in owners}
    tree = {frozenset((v, int(par[v]))) for v in range(1, p)}
    assert len(edges) == p - 1 and edges == tree
    assert 1 <= rounds <= max(1, p // 2)
    np.testing.assert_allclose(w[1:], np.linalg.norm(pts[1:] - pts[par[1:]], axis=1), rtol=1e-12)
    # a minimum spanning tree: no lighter tree by the cut property on every edge's removal (checked against a dense Prim total)
    d = np.linalg.norm(pts[:, None] - pts[None], axis=-1)
    intree = np.zeros(p, bool); intree[0] = True
    key = d[0].copy(); total = 0.0
    for _ in range(p - 1):
        key[intree] = np.inf
        v = int(np.argmin(key)); total += key[v]; intree[v] = True
        key = np.minimum(key, d[v])
    np.testing.assert_allclose(w.sum(), total, rtol=1e-12)


def test_model_tie_rules_on_a_lattice():
    """4 x 4 lattice of spacing 0.25: all candidates tie; the highest index is taken and an earlier parent is kept."""
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 2)
    pts = np.concatenate([g, np.zeros((16, 1))], 1) * 0.25
    par, w, _ = em.prim(pts, np.float32)
    assert par[4] == 0 and par[1] == 0            # step 1: vertices 1 and 4 tie at 0.25 -> 4 is taken; 1 keeps parent 0 throughout
    assert par[5] == 4                             # 5 is first reached from 4 (0.25) and keeps it when 1 offers the same length
    assert np.all(w[1:] == np.float32(0.25))
    assert em.wave_sum(w, np.float32) == np.float32(15 * 0.25)


def test_model_collinear_512_peels_in_256_rounds():
    x = np.zeros((512, 3)); x[:, 0] = np.arange(512) * 0.25
    par, w, _ = em.prim(x, np.float32)
    np.testing.assert_array_equal(par[1:], np.arange(511))
    other, rounds = em.peel(par)
    assert rounds == 256
    # the two ends walk inwards; the last edge (255, 256) goes to the larger index
    np.testing.assert_array_equal(other[:255], np.arange(1, 256))
    assert other[255] == -1 and other[256] == 255
    np.testing.assert_array_equal(other[257:], np.arange(256, 511))


def test_model_pair_owner_is_the_larger_index():
    out = em.expansion_forward(np.array([[[0, 0, 0], [0.75, 0, 0]]], dtype=np.float32), 2, 0.5, np.float32)
    np.testing.assert_array_equal(out["assignment"], [[-1, 0]])
    np.testing.assert_array_equal(out["dist"], np.array([[0, 0.75]], dtype=np.float32))
    assert out["mean_mst_length"][0] == np.float32(0.75)


def test_model_backward_matches_finite_differences():
    rng = np.random.default_rng(3)
    x = rng.random((1, 16, 3))
    out = em.expansion_forward(x, 8, 1.0)
    g = rng.standard_normal((1, 16))
    grad = em.expansion_backward(x, g, out["assignment"])
    own = out["assignment"][0] >= 0
    assert own.any() and np.all(grad[0, ~own] == 0)
    # d(c^2)/dx_j at the owner j: the documented factor-2 form is the gradient of the SQUARED length
    j = int(np.flatnonzero(own)[0]); a = int(out["assignment"][0, j])
    eps = 1e-6
    for c in range(3):
        xp = x.copy(); xp[0, j, c] += eps
        fd = (np.sum((xp[0, j] - xp[0, a]) ** 2) - np.sum((x[0, j] - x[0, a]) ** 2)) / eps
        np.testing.assert_allclose(grad[0, j, c], g[0, j] * fd, rtol=1e-4)


def test_model_sampling_is_distinct_and_starts_at_zero():
    x = np.random.default_rng(5).random((200, 3))
    picks, picked, least, A = em.mds(x, 200, 0.1)
    assert picks[0] == 0 and sorted(picks.tolist()) == list(range(200))
    np.testing.assert_array_equal(picked[1:], least[1:])
    w1 = em.mds(x, 64, 0.1, split=200)[0]
    w2 = em.mds(x, 64, 0.1, split=50)[0]
    assert not np.array_equal(w1, w2)
    # ties go to the lowest index: with a tiny t every density underflows to 0
    z = em.mds(x, 5, 1e-3)[0]
    np.testing.assert_array_equal(z, [0, 1, 2, 3, 4])
